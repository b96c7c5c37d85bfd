"""GPU suite for the iALS baseline (`--train ials`, include/pda_hip_ials.h) against the float64 restatement tests/ials_ref.py.
Every tolerance is the a-priori bound derived there, evaluated on the test's own inputs; the tests print observed / bound.

Largest observed / bound on MI355X: see DESIGN.md 5o.
"""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ials_ref as ir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NR = len(ir.ROW_LENGTHS)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def lengths():
    """The side of the kernel tests: ten rows of the lengths at which the code takes another path, over N_OTHER columns."""
    rows, cols = ir.length_graph()
    indptr, indices = ir.csr(rows, cols, NR)
    return rows, cols, indptr, indices


def graph_of(dev, rows, cols, n_rows, n_other, a0, lam, nu):
    from pda_amd import ops
    return ops.IalsGraph(rows, cols, n_rows, n_other, dev, lam=lam, alpha0=a0, nu=nu)


# ---- 1. exact normal equations ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, a0", [(32, 0.25), (32, 0.5), (64, 0.5), (128, 0.25)])
def test_the_normal_equations_are_exact_bit_for_bit(dev, lengths, d, a0):
    """Tables of multiples of 1/8, alpha0 and lam_row dyadic: every entry of (A_r, b_r) is exact in fp32 whatever the order, so dbg_normal equals
    the restatement's chunk-ordered sums bit for bit; a wrong tile, a dropped tail block or a lost chunk shows as an integer-sized difference."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER, a0, 1.0, 0.0)
    lam = (np.arange(NR) % 5 * 0.25 + 0.5).astype(np.float32)
    g.user.lam_row = torch.from_numpy(lam).to(dev)
    Z32 = ir.eighths_table(ir.N_OTHER, d, 2)
    Z = torch.from_numpy(Z32).to(dev)
    G = ops.ials_gram(Z)
    G32 = ir.gram32(Z32)
    assert torch.equal(bits(G), bits(torch.from_numpy(G32).to(dev)))
    X = torch.full((NR, d), 7.0, device=dev)
    dbg = torch.full((NR, d * d + d), float("nan"), device=dev)
    work = g.user.sub_list(range(NR), shuffle_seed=1)
    assert work.n_long == 2 and work.n_slots == 5 and work.n_work == NR - 2 + 5
    ops.ials_half_sweep(g, "user", Z, X, G=G, work=work, dbg_normal=dbg)
    got = dbg.cpu().numpy()
    for r in range(NR):
        A, b = ir.normal32(indptr, indices, Z32, G32, a0, lam, r)
        diff = np.abs(got[r, :d * d].reshape(d, d).astype(np.float64) - A).max()
        assert np.array_equal(got[r, :d * d].reshape(d, d).view(np.int32), A.view(np.int32)), (r, ir.ROW_LENGTHS[r], diff)
        assert np.array_equal(got[r, d * d:].view(np.int32), b.view(np.int32)), (r, ir.ROW_LENGTHS[r])
    x = X.cpu().numpy()
    assert (x[0] == 0).all()                                                                # the row without pairs
    assert np.isfinite(x).all() and g.buffers(d)["fail"].item() == 0                        # (the solve itself: test 2)


# ---- 2. the solve against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", ir.PARAMS, ids=lambda p: "a%g-l%g-n%g" % p)
@pytest.mark.parametrize("kind", ir.TABLES)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_the_solve_stays_inside_the_a_priori_bound(dev, lengths, d, kind, params):
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    a0, lam, nu = params
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER, a0, lam, nu)
    lam_row = ir.lam_row(np.diff(indptr), ir.N_OTHER, lam, a0, nu)
    np.testing.assert_array_equal(g.user.host_lam_row, lam_row)
    Z32 = ir.table(kind, ir.N_OTHER, d)
    X = torch.full((NR, d), float("nan"), device=dev)
    ops.ials_half_sweep(g, "user", torch.from_numpy(Z32).to(dev), X, work=g.user.sub_list(range(NR), shuffle_seed=2))
    o = ir.row_bounds(indptr, indices, Z32, a0, lam_row, range(NR))
    assert (o["kappa"] * o["eta"]).max() < 0.1                                              # the condition on the inputs (the host suite has it too)
    x = X.cpu().numpy().astype(np.float64)
    err = np.linalg.norm(x - o["x"], axis=1)
    allowed = o["bound"] * o["xnorm"]
    ratio = np.divide(err, allowed, out=np.zeros_like(err), where=allowed > 0)
    print("ials solve d=%d %s %s: observed / bound max %.3g (row of %d pairs), kappa max %.1f" %
          (d, kind, params, ratio.max(), ir.ROW_LENGTHS[int(ratio.argmax())], o["kappa"].max()))
    assert (x[0] == 0).all() and np.isfinite(x).all() and g.buffers(d)["fail"].item() == 0
    assert (err <= allowed).all(), (err / np.maximum(allowed, 1e-300)).max()


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_call(dev):
    """Two calls are bit-equal; a row solved alone equals the same row solved among 63 others; a permuted work list gives the same bits."""
    from pda_amd import ops
    d, n = 64, 64
    rs = np.random.default_rng(4)
    lens = list(ir.ROW_LENGTHS) + [int(v) for v in rs.integers(1, 60, n - NR)]
    rows, cols = ir.length_graph(seed=9, lengths=lens)
    g = graph_of(dev, rows, cols, n, ir.N_OTHER, 0.1, 0.05, 1.0)
    Z = torch.from_numpy(ir.table("gauss0.3", ir.N_OTHER, d)).to(dev)
    G = ops.ials_gram(Z)
    assert torch.equal(bits(G), bits(ops.ials_gram(Z)))

    def solve(work):
        X = torch.full((n, d), float("nan"), device=dev)
        ops.ials_half_sweep(g, "user", Z, X, G=G, work=work)
        return X

    base = solve(None)
    assert torch.isfinite(base).all()
    assert torch.equal(bits(base), bits(solve(None)))
    for seed in (1, 2):
        assert torch.equal(bits(base), bits(solve(g.user.sub_list(range(n), shuffle_seed=seed))))
    for r in (0, 3, NR - 2, NR - 1, n - 1):                                                # empty, short, one full chunk + 1, three chunks, the last
        alone = solve(g.user.sub_list([r]))
        assert torch.equal(bits(alone[r]), bits(base[r])), r
        others = torch.ones(n, dtype=torch.bool, device=dev)
        others[r] = False
        assert torch.isnan(alone[others]).all()                                             # the rows a call does not list are left as they are


# ---- 4. the loss -------------------------------------------------------------------------------------------------------------------------------------
def toy_pairs(seed=3, nu=70, ni=45, n=2500):
    g = np.random.default_rng(seed)
    return g.integers(0, nu - 1, n), np.minimum(g.zipf(1.4, n) - 1, ni - 2), nu, ni      # the last user and the last item stay without pairs


@pytest.mark.parametrize("case", ["toy-32", "toy-64", "toy-128", "lengths-64"])
def test_the_loss_equals_the_float64_objective_within_its_bound(dev, lengths, case):
    from pda_amd import ops
    d = int(case.split("-")[1])
    if case.startswith("toy"):
        u, i, nu, ni = toy_pairs()
    else:
        u, i, nu, ni = lengths[0], lengths[1], NR, ir.N_OTHER
    a0, lam, nuu = 0.1, 0.05, 1.0
    g = graph_of(dev, u, i, nu, ni, a0, lam, nuu)
    eu, ei = ir.dedup_pairs(u, i, ni)
    X32, Y32 = ir.table("gauss0.3", nu, d, seed=5), ir.table("gauss0.3", ni, d, seed=6)
    got = ops.ials_loss(g, torch.from_numpy(X32).to(dev), torch.from_numpy(Y32).to(dev)).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (3,)
    lu, li = g.user.host_lam_row, g.item.host_lam_row
    L, fit, reg = ir.objective(X32, Y32, eu, ei, a0, lu, li)
    up, ui = ir.csr(eu, ei, nu)
    bound = ir.loss_bound(X32, Y32, up, ui, a0, lu, L)
    print("ials loss %s: |L^ - L| / bound = %.3g (L = %.6g, bound = %.3g)" % (case, abs(got[0] - L) / bound, L, bound))
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound
    assert abs(got[0] - (got[1] + got[2])) <= 1e-12 * abs(L)


# ---- 5. the model ------------------------------------------------------------------------------------------------------------------------------------
def make_model(dev, d=32, **over):
    from pda_amd.model_api import IALSMF, gcn_train_pairs
    from pda_amd.parse import parse_args
    args = parse_args(["--train", "ials", "--embed_size", str(d), "--regs", "0.05", "--verbose", "0"])
    for k, v in over.items():
        setattr(args, k, v)
    u, i, nu, ni = toy_pairs()
    lists = {int(x): [] for x in range(nu)}
    for a, b in zip(u.tolist(), i.tolist()):
        lists[a].append(b)                                                                  # (with duplicates: the graph counts a pair once)
    cfg = {"n_users": nu, "n_items": ni, "gcn_train_pairs": gcn_train_pairs(lists)}
    return IALSMF(args, cfg, device=dev), (u, i, nu, ni)


def test_one_epoch_of_the_model_is_the_restatement_s_epoch(dev):
    from pda_amd.model_api import BPRMF
    m, (u, i, nu, ni) = make_model(dev)
    a0, lam, nuu = 0.1, 0.05, 1.0
    eu, ei = ir.dedup_pairs(u, i, ni)
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    lu, li = ir.lam_row(np.diff(up), ni, lam, a0, nuu), ir.lam_row(np.diff(ip), nu, lam, a0, nuu)
    np.testing.assert_array_equal(m.graph.user.host_lam_row, lu)
    np.testing.assert_array_equal(m.graph.item.host_lam_row, li)
    ref = BPRMF(m_args(), {"n_users": nu, "n_items": ni}, device=dev)                       # Xavier tables from the same seed as every model
    assert torch.equal(ref.weights["user_embedding"], m.weights["user_embedding"]) and torch.equal(ref.weights["item_embedding"], m.weights["item_embedding"])
    X0, Y0 = (m.weights[k].cpu().numpy() for k in ("user_embedding", "item_embedding"))
    out = m.train_epoch()
    assert out.dtype == torch.float64 and out.shape == (3,) and out.is_cuda
    X, Y = (m.weights[k].cpu().numpy().astype(np.float64) for k in ("user_embedding", "item_embedding"))
    bx = ir.row_bounds(up, ui, Y0, a0, lu, range(nu))
    X1 = bx["x"]
    ex = np.linalg.norm(X - X1, axis=1)
    assert (ex <= bx["bound"] * bx["xnorm"]).all()
    by = ir.row_bounds(ip, ii, X1, a0, li, range(ni), dZ=bx["bound"] * bx["xnorm"])          # the user side's error, propagated
    ey = np.linalg.norm(Y - by["x"], axis=1)
    print("ials model epoch: observed / bound max %.3g (users), %.3g (items)" %
          (np.max(ex / np.maximum(bx["bound"] * bx["xnorm"], 1e-300)), np.max(ey / np.maximum(by["bound"] * by["xnorm"], 1e-300))))
    assert np.isfinite(by["bound"]).all() and (ey <= by["bound"] * by["xnorm"]).all()
    assert (X[-1] == 0).all() and (Y[-1] == 0).all() and m.failed_pivots().item() == 0     # the user and the item without pairs
    X32, Y32 = (m.weights[k].cpu().numpy() for k in ("user_embedding", "item_embedding"))
    L, fit, reg = ir.objective(X32, Y32, eu, ei, a0, lu, li)
    bound = ir.loss_bound(X32, Y32, up, ui, a0, lu, L)
    got = out.cpu().numpy() * len(eu)
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound
    sd = m.state_dict()
    assert sd.get("model", "mf") == "mf" and not any(k in sd for k in ("mU", "vU", "mI", "vI"))
    plain = BPRMF(m_args(optimizer="sgd"), {"n_users": nu, "n_items": ni}, device=dev)
    plain.load_state_dict(sd)
    assert torch.equal(plain.weights["user_embedding"], m.weights["user_embedding"])


def m_args(**over):
    from pda_amd.parse import parse_args
    args = parse_args(["--embed_size", "32", "--verbose", "0"])
    for k, v in over.items():
        setattr(args, k, v)
    return args


def test_the_objective_does_not_rise_over_six_epochs(dev):
    """The float64 objective of the tables after every half-sweep, against the one before it.  The objective is quadratic in the rows being
    solved with its minimum at the exact row solutions, so an error dx_r costs the second-order term dx_r^T A_r dx_r <= lambda_max(A_r)
    |dx_r|^2 and nothing else: the allowance is its sum, |dx_r| from the bound of test 2 on the half-sweep's own inputs."""
    from pda_amd import ops
    m, (u, i, nu, ni) = make_model(dev)
    a0 = 0.1
    eu, ei = ir.dedup_pairs(u, i, ni)
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    lu, li = m.graph.user.host_lam_row, m.graph.item.host_lam_row
    X, Y = m.weights["user_embedding"], m.weights["item_embedding"]
    obj = lambda: ir.objective(X.cpu().numpy(), Y.cpu().numpy(), eu, ei, a0, lu, li)[0]      # noqa: E731
    last, worst = obj(), -np.inf
    for epoch in range(6):
        for side, cp, ci, lam, fixed, n in (("user", up, ui, lu, Y, nu), ("item", ip, ii, li, X, ni)):
            b = ir.row_bounds(cp, ci, fixed.cpu().numpy(), a0, lam, range(n))
            allowance = float(np.sum(b["lmax"] * (b["bound"] * b["xnorm"]) ** 2))
            ops.ials_half_sweep(m.graph, side, fixed, X if side == "user" else Y)
            now = obj()
            worst = max(worst, (now - last) / last)
            assert now <= last + allowance, (epoch, side, now - last, allowance)
            last = now
    print("ials objective over 12 half-sweeps: worst relative step %.3g, final %.6g" % (worst, last))
    assert m.failed_pivots().item() == 0


# ---- 6. through the CLI ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("ials_data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    return str(root) + "/"


def _argv(toy, save, extra=()):
    return ["--data_path", toy, "--dataset", "toy", "--train", "ials", "--test", "normal", "--epoch", "3", "--log_interval", "1", "--embed_size", "32",
            "--regs", "0.05", "--valid_set", "valid", "--pop_exp", "0.22", "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t",
            "--cuda", "0", "--eval_block", "128"] + list(extra)


def _run(module, argv):
    r = subprocess.run([sys.executable, "-m", module] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _ckpt(save):
    found = glob.glob(os.path.join(save, "**", "best_ckpt.ckpt"), recursive=True)
    assert len(found) == 1 and "_train_ials" in found[0] and "ials" in os.path.basename(os.path.dirname(found[0])), found
    return torch.load(found[0], map_location="cpu")


def test_the_cli_trains_checkpoints_and_exports(dev, toy, tmp_path):
    from pda_amd.model_api import BPRMF
    saves = [str(tmp_path / k) + "/" for k in "abc"]
    out = _run("pda_amd.train_new_api", _argv(toy, saves[0]))
    losses = [[float(x) for x in mm.groups()] for mm in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
    assert len(losses) == 3 and np.isfinite(losses).all(), out[-2000:]
    assert losses[0][0] > losses[1][0] > losses[2][0]                                       # the printed loss falls
    assert all(abs(l - (f + r)) < 2e-5 for l, f, r in losses)
    assert "recall=[" in out and "expo:" in out and "running iALS" in out                   # the metrics and the gamma search of --test normal
    sd = _ckpt(saves[0])
    assert sd.get("model", "mf") == "mf" and "mU" not in sd and tuple(sd["user_embedding"].shape) == (400, 32)
    plain = BPRMF(m_args(optimizer="sgd"), {"n_users": 400, "n_items": 300}, device=dev)
    plain.load_state_dict(sd)
    assert torch.equal(plain.weights["item_embedding"].cpu(), sd["item_embedding"])
    npz = str(tmp_path / "lists.npz")
    _run("pda_amd.export_topk", _argv(toy, saves[0], ("--export_out", npz)))
    lists = np.load(npz)
    assert lists["idx"].shape[1] == 50 and lists["idx"].shape[0] == lists["users"].shape[0] > 0 and (lists["idx"] < 300).all()
    _run("pda_amd.train_new_api", _argv(toy, saves[1]))
    _run("pda_amd.train_new_api", _argv(toy, saves[2], ("--deterministic", "1")))
    for other in saves[1:]:
        sd2 = _ckpt(other)
        for k in ("user_embedding", "item_embedding"):
            assert torch.equal(sd[k].view(torch.int32), sd2[k].view(torch.int32)), (other, k)
