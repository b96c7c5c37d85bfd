"""Reference, rounding bound, fp32 emulation and mutants of the LightGCN backbone (include/pda_hip_gcn.h) for
tests/test_lightgcn_host.py and tests/test_gpu_lightgcn.py; it holds no test.

    graph            the train graph in float64 from the pairs, restated without pda_amd: distinct edges, degrees, fl32 weights, the dense
                     symmetric A over the n_users + n_items stacked rows (small graphs only)
    propagate        E^(k+1) = A E^(k), F = mean of the L + 1 layers;  backward: (1 / (L + 1)) sum_k A^k G in Horner form
    model            loss, G = d mf / dF, and the closed-form gradient on the ego tables, with one switch per mutant
    autograd_grad    the same gradient from torch.autograd on the float64 model
    *_bound          a-priori bounds on |fp32 kernel - float64 reference| per element (derived below, not measured)
    emulate_*        the kernels' expressions in numpy float32 in the kernels' order, or with the edges of every sum in another order
    graph_case / model_case    the inputs the CPU and the GPU tests share

THE BOUND, line by line.  u = 2^-24 (one fp32 rounding, relative).  |A| is the matrix of the absolute weights (they are positive: A itself),
deg_r the edges of row r.  The weights are inputs of the kernel and of the reference alike (rounded once, on the host), and so are the tables:
their own rounding is nobody's error.  The library is built with -ffp-contract=off, so every product and every sum rounds once; the bound
holds with fused multiply-adds too (one rounding less per term).

  one product   y_r = sum_e w_e x_e over the deg_r edges of row r, the input known to b (|x^ - x| <= b):  every term takes its product's
                rounding and at most deg_r - 1 of the additions of its row, in ANY order (a cut row: the additions inside its chunk and those
                of the partial sums are still deg_r - 1 in all; additions onto zero are exact), so (1 + u)^deg_r - 1 relative.  That is
                deg_r u / (1 - deg_r u) <= (deg_r + 2) u while deg_r^2 u <= 2, i.e. up to 5 792 edges -- every row of the test graphs
                (asserted in product_bound).  With the input's own error carried through |A|:
                  p(x, b) = |A| b + (deg + 2) u |A| (|x| + b)
  layers        b_0 = 0,   b_{k+1} = p(E_k, b_k)                                                    (the Y a layer writes, unscaled)
  addend        y = add + A x (the Horner step): one more addition of the magnitude held:
                  p_add = p + u (|add + A x| + p)
  running sum   S_k = sum_{j <= k} E_j, S_0 = E_0 exact; S^_k = fl(S^_{k-1} + E^_k):
                  c_0 = 0,   c_k = c_{k-1} + b_k + u (|S_k| + c_{k-1} + b_k)
  final scale   F = fl(fl32(1 / (L + 1)) S^_L): the constant's rounding and the product's (2 u, as 2.02 u for their product):
                  f = (c_L + 2.02 u (|S_L| + c_L)) / (L + 1)              (scale 1: the multiplication is exact, the same line with 0 for 2.02 u)
  backward      the same operator on the gradient, in Horner form from the exact input H_0 = G:
                  h_0 = 0,   h_{j+1} = p(H_j, h_j) + u (|H_{j+1}| + p(H_j, h_j)),   H_{j+1} = G + A H_j
                  the last step scaled:  r = (h_L + 2.02 u (|H_L| + h_L)) / (L + 1)
  regulariser   g_r = R_r + sum over the n occurrences of row r of c row, c = fl(fl(regs) / fl(reg_div)) (3 u): each product c x_k carries
                4 roundings, the n atomic additions onto the value held, in any order, one each of at most T = |R| + n |c x| (1 + 4.04 u):
                  d_g = 1.01 (4 u n |c x| + n u T)
  reg loss      reg = c 0.5 sum sq, as tests/train_ref.py derives it for the triplet kernel (the reduction has the same shape: six roundings
                inside a lane, at most max(14, TPB) sums inside a workgroup of TPB = 2048 / d triplets, n_wg atomics):
                  d_reg = 1.01 (6 + max(14, TPB) + n_wg + 4) u reg
"""
import numpy as np

from oracle import pda_oracle as po

U32 = 2.0 ** -24
F = np.float32
CHUNK = 512               # PDA_GCN_CHUNK
DIMS = (32, 64, 128, 256)
REGS = 1e-2


# ---- the graph ---------------------------------------------------------------------------------------------------------------------------------
def graph(users, items, n_users, n_items, keep_duplicates=False):
    """dict(A float64 [N, N] dense, deg int [N], edges [(u, i)] sorted, w float32 per edge, n_users, n_items).  keep_duplicates: the mutant that
    counts a repeated pair as two edges (its A entry is the sum of both)."""
    pairs = sorted(zip((int(u) for u in users), (int(i) for i in items)))
    if not keep_duplicates:
        pairs = sorted(set(pairs))
    N = n_users + n_items
    deg = np.zeros(N, dtype=np.int64)
    for u, i in pairs:
        deg[u] += 1
        deg[n_users + i] += 1
    A = np.zeros((N, N))
    w = np.empty(len(pairs), dtype=np.float32)
    for k, (u, i) in enumerate(pairs):
        w[k] = np.float32(1.0 / np.sqrt(np.float64(deg[u] * deg[n_users + i])))
        A[u, n_users + i] += np.float64(w[k])
        A[n_users + i, u] += np.float64(w[k])
    return dict(A=A, deg=deg, edges=pairs, w=w, n_users=n_users, n_items=n_items)


def propagate(A, E0, L, mut=None):
    """-> (layers [E_0 .. E_L], F) in float64."""
    E = [np.asarray(E0, dtype=np.float64)]
    for _ in range(L):
        E.append(A @ E[-1])
    if mut == "no_ego_in_mean":
        return E, sum(E[1:]) / (L + 1)
    return E, sum(E) / (L if mut == "div_by_L" else L + 1)


def backward(A, G, L, mut=None):
    """(1 / (L + 1)) sum_{k <= L} A^k G by Horner's rule, float64; also the unscaled iterates H_0 .. H_L."""
    G = np.asarray(G, dtype=np.float64)
    H = [G]
    for _ in range(L - 1 if mut == "backward_one_short" else L):
        H.append(G + A.T @ H[-1])
    return H, H[-1] / (1.0 if mut == "backward_no_scale" else L + 1)


# ---- the bounds --------------------------------------------------------------------------------------------------------------------------------
def product_bound(g, X, b_in=0.0):
    """p(x, b) of the docstring for one product over graph g."""
    deg = g["deg"].astype(np.float64)
    assert (deg ** 2).max() * U32 <= 2.0, "a row beyond 5 792 edges: (deg + 2) u no longer covers (1 + u)^deg - 1"
    A = np.abs(g["A"])
    b = np.broadcast_to(np.asarray(b_in, dtype=np.float64), X.shape)
    return A @ b + ((deg + 2) * U32)[:, None] * (A @ (np.abs(X) + b))


def fused_bound(g, X, add=None, sum_in=None, scale=1.0):
    """One fused launch on exact inputs -> (bound on Y, bound on sum_out or None); Y is the scaled output when there is no running sum."""
    y = g["A"] @ X.astype(np.float64)
    p = product_bound(g, X)
    if add is not None:
        y = y + add
        p = p + U32 * (np.abs(y) + p)
    k = 0.0 if scale == 1.0 else 2.02 * U32
    if sum_in is None:
        return abs(scale) * (p + k * (np.abs(y) + p)), None
    s = sum_in.astype(np.float64) + y
    c = p + U32 * (np.abs(s) + p)
    return p, abs(scale) * (c + k * (np.abs(s) + c))


def propagate_bound(g, E0, L):
    E, _ = propagate(g["A"], E0, L)
    b, c, S = np.zeros_like(E[0]), np.zeros_like(E[0]), E[0].copy()
    for k in range(1, L + 1):
        b = product_bound(g, E[k - 1], b)
        S = S + E[k]
        c = c + b + U32 * (np.abs(S) + c + b)
    if L == 0:
        return c
    return (c + 2.02 * U32 * (np.abs(S) + c)) / (L + 1)


def backward_bound(g, G, L):
    H, _ = backward(g["A"], G, L)
    h = np.zeros_like(H[0])
    for j in range(L):
        p = product_bound(g, H[j], h)
        h = p + U32 * (np.abs(H[j + 1]) + p)
    if L == 0:
        return h
    return (h + 2.02 * U32 * (np.abs(H[L]) + h)) / (L + 1)


def reg_terms(E0, n_users, users, pos, neg, regs, reg_div):
    """float64: (c x the summed ego rows [N, d], occurrences [N], the reg loss)."""
    E0 = np.asarray(E0, dtype=np.float64)
    c = regs / reg_div
    rows = np.concatenate([users, n_users + pos, n_users + neg]).astype(np.int64)
    occ = np.bincount(rows, minlength=E0.shape[0])
    return c * occ[:, None] * E0, occ, c * 0.5 * (E0[rows] ** 2).sum()


def reg_bound(E0, n_users, users, pos, neg, regs, reg_div, R):
    """(d_g [N, d], d_reg) of the docstring; R: the float64 gradient the rows are added to."""
    add, occ, reg = reg_terms(E0, n_users, users, pos, neg, regs, reg_div)
    n = occ[:, None].astype(np.float64)
    T = np.abs(R) + np.abs(add) * (1 + 4.04 * U32)
    d, B = E0.shape[1], len(users)
    t = 2048 // d
    n_wg = -(-B // t)
    return 1.01 * (4 * U32 * np.abs(add) + n * U32 * T), 1.01 * (6 + max(14, t) + n_wg + 4) * U32 * reg


# ---- the model: loss and gradient on the ego tables, with the mutants' switches -----------------------------------------------------------------
MUTANTS = {
    # name -> (what it changes, the quantity on which |mutant - reference| > 10 bound must show)
    "row_normalised": ("w_ui = 1 / deg of the row instead of 1 / sqrt(deg_u deg_i)", "F"),
    "one_direction": ("users are updated from the items, items not from the users", "F"),
    "no_ego_in_mean": ("the mean runs over the layers 1 .. L, without E^(0)", "F"),
    "div_by_L": ("the sum of the L + 1 layers is divided by L", "F"),
    "dup_edges": ("a pair that occurs twice is two edges", "F"),
    "backward_one_short": ("the backward pass runs L - 1 Horner steps", "grad"),
    "backward_no_scale": ("the backward pass lacks the 1 / (L + 1)", "grad"),
    "reg_on_final": ("the regulariser reads the final rows instead of the ego rows", "grad"),
    "reg_before_backward": ("the regulariser is added before the backward pass and propagates", "grad"),
}


def mutant_graph(case, mut):
    if mut == "dup_edges":
        return graph(case["pairs"][0], case["pairs"][1], case["n_users"], case["n_items"], keep_duplicates=True)["A"]
    A = case["g"]["A"].copy()
    if mut == "row_normalised":
        deg = np.maximum(case["g"]["deg"], 1).astype(np.float64)
        A = (A > 0) / deg[:, None]
    if mut == "one_direction":
        A[case["n_users"]:, :] = 0.0
    return A


def model(case, L, pop, mut=None):
    """dict(F, loss = (loss, mf, reg), G = d mf / dF, R = the propagated gradient, grad = d loss / d E0), float64."""
    nu, b = case["n_users"], case["batch"]
    users, pos, neg = b["users"], b["pos"], b["neg"]
    pp, pn = (b["pp"], b["pn"]) if pop else (None, None)
    A = mutant_graph(case, mut) if mut in ("row_normalised", "one_direction", "dup_edges") else case["g"]["A"]
    E0 = case["E0"].astype(np.float64)
    _, Fin = propagate(A, E0, L, mut)
    fw = po.bpr_forward(Fin[:nu], Fin[nu:], users, pos, neg, pp, pn)
    _, mf, _ = po.bpr_loss(fw, 0.0, case["reg_div"])
    due, dpe, dne = po.bpr_grads(fw, 0.0, case["reg_div"], pp, pn)
    gU, gI = po.dense_grads(nu, case["n_items"], users, pos, neg, due, dpe, dne)
    G = np.concatenate([gU, gI])
    src = Fin if mut == "reg_on_final" else E0
    add, _, reg = reg_terms(src, nu, users, pos, neg, case["regs"], case["reg_div"])
    if mut == "reg_before_backward":
        _, R = backward(A, G + add, L, mut)
        grad = R
    else:
        _, R = backward(A, G, L, mut)
        grad = R + add
    return dict(F=Fin, loss=np.array([mf + reg, mf, reg]), G=G, R=R, grad=grad)


def autograd_grad(case, L, pop):
    """d loss / d E0 from torch.autograd on the float64 model (the loss as the contract writes it)."""
    import torch
    nu, b = case["n_users"], case["batch"]
    A = torch.from_numpy(np.array(case["g"]["A"]))
    E0 = torch.from_numpy(case["E0"].astype(np.float64)).requires_grad_(True)
    E, S = E0, E0
    for _ in range(L):
        E = A @ E
        S = S + E
    Fin = S / (L + 1)
    ix = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64))      # noqa: E731
    ue, pe, ne = Fin[ix(b["users"])], Fin[nu + ix(b["pos"])], Fin[nu + ix(b["neg"])]
    ps, ns = (ue * pe).sum(1), (ue * ne).sum(1)
    if pop:
        elu1 = lambda s: torch.where(s > 0, s + 1.0, torch.exp(torch.clamp(s, max=0.0)))      # noqa: E731
        ps, ns = elu1(ps) * torch.from_numpy(b["pp"].astype(np.float64)), elu1(ns) * torch.from_numpy(b["pn"].astype(np.float64))
    mf = -torch.log(torch.sigmoid(ps - ns) + 1e-10).mean()
    e_u, e_p, e_n = E0[ix(b["users"])], E0[nu + ix(b["pos"])], E0[nu + ix(b["neg"])]
    reg = case["regs"] * 0.5 * ((e_u ** 2).sum() + (e_p ** 2).sum() + (e_n ** 2).sum()) / case["reg_div"]
    loss = mf + reg
    loss.backward()
    return E0.grad.numpy(), np.array([loss.item(), mf.item(), reg.item()])


# ---- the fp32 emulation --------------------------------------------------------------------------------------------------------------------------
ORDERS = ("kernel", "reversed", "shuffled")


def emulate_spmm(ga, X, add=None, sum_in=None, scale=1.0, order="kernel"):
    """pda_gcn_spmm_f32 in numpy float32 on the arrays of pda_amd.ops.gcn_graph_arrays: per entry of the work list the edges left to right onto a
    zero accumulator, a cut row's partial sums in chunk order, then add + ., sum_in + ., scale * .  `order` other than "kernel": the edges of
    every entry (and a row's partials) reversed or shuffled -- another legal order of the same sums.  -> (Y, sum_out or None)."""
    X = np.ascontiguousarray(X, dtype=F)
    N, d = X.shape
    idx, w = ga["indices"], ga["w"]
    rng = np.random.default_rng(11)

    def perm(n):
        return np.arange(n) if order == "kernel" else (np.arange(n)[::-1] if order == "reversed" else rng.permutation(n))
    acc_rows = np.zeros((N, d), F)
    partial = np.zeros((max(1, ga["n_slots"]), d), F)
    for row, e0, e1, slot in ga["work"]:
        acc = np.zeros(d, F)
        for k in e0 + perm(e1 - e0):
            acc = acc + X[idx[k]] * w[k]
        if slot >= 0:
            partial[slot] = acc
        else:
            acc_rows[row] = acc
    for row, s0, n in ga["long_rows"]:
        acc = np.zeros(d, F)
        for j in perm(n):
            acc = acc + partial[s0 + j]
        acc_rows[row] = acc
    y = acc_rows if add is None else np.asarray(add, F) + acc_rows
    sc = F(scale)
    assert y.dtype == F
    if sum_in is None:
        return y * sc, None
    return y, (np.asarray(sum_in, F) + y) * sc


def emulate_propagate(ga, E0, L, order="kernel"):
    E0 = np.ascontiguousarray(E0, dtype=F)
    if L == 0:
        return E0
    X, S = E0, E0
    for k in range(1, L + 1):
        X, S = emulate_spmm(ga, X, sum_in=S, scale=1.0 / (L + 1) if k == L else 1.0, order=order)
    return S


def emulate_backward(ga, G, L, order="kernel"):
    G = np.ascontiguousarray(G, dtype=F)
    X = G
    for j in range(1, L + 1):
        X, _ = emulate_spmm(ga, X, add=G, scale=1.0 / (L + 1) if j == L else 1.0, order=order)
    return X


def emulate_reg(E0, n_users, users, pos, neg, regs, reg_div, R, order="kernel"):
    """pda_gcn_reg_f32's gradient part: the atomics in the batch's order (users, positives, negatives per triplet), reversed, or shuffled."""
    E0, out = np.ascontiguousarray(E0, dtype=F), np.array(R, dtype=F)
    c = F(regs) / F(reg_div)
    rows = np.stack([users, n_users + pos, n_users + neg], axis=1).reshape(-1).astype(np.int64)
    n = len(rows)
    o = np.arange(n) if order == "kernel" else (np.arange(n)[::-1] if order == "reversed" else np.random.default_rng(3).permutation(n))
    for r in rows[o]:
        out[r] = out[r] + E0[r] * c
    assert out.dtype == F
    return out


# ---- the shared cases ------------------------------------------------------------------------------------------------------------------------------
GRAPHS = ("small", "hub")
HUB_DEGREES = (CHUNK - 1, CHUNK, CHUNK + 1, 4 * CHUNK + 52)
_CACHE = {}


def graph_pairs(name):
    """(users, items, n_users, n_items).
    small: 301 users x 200 items, about 4 000 distinct pairs plus 150 repeated ones; user 0 and item 5 have no edges, user 1 and item 6 have one,
           item 0 is a hub (every third user), the last user and the last item have edges.  501 stacked rows: no multiple of the 32 / 16 / 8 / 4
           work entries a workgroup takes at d = 32 / 64 / 128 / 256 (300 x 200 would be one at d = 256).
    hub:   2 200 users x 64 items; the items 0 .. 3 have exactly CHUNK - 1, CHUNK, CHUNK + 1 and 4 CHUNK + 52 edges (one chunk, one full chunk, two
           chunks, five), the others 3 .. 40; users without an edge occur."""
    rng = np.random.default_rng(17 if name == "small" else 23)
    if name == "small":
        nu, ni = 301, 200
        u, i = rng.integers(2, nu, 3900), rng.integers(7, ni, 3900)
        hub = np.arange(2, nu, 3)
        u, i = np.concatenate([u, hub, [1, nu - 1, 4]]), np.concatenate([i, np.zeros(len(hub), np.int64), [8, ni - 1, 6]])
        rep = rng.integers(0, len(u), 150)
        u, i = np.concatenate([u, u[rep]]), np.concatenate([i, i[rep]])
    else:
        nu, ni = 2200, 64
        us, its = [], []
        for it in range(ni):
            deg = HUB_DEGREES[it] if it < 4 else int(rng.integers(3, 41))
            us.append(rng.permutation(nu - 10)[:deg] + 10 * (it % 2))        # (the users 0 .. 9 or the last ten stay out of a row)
            its.append(np.full(deg, it))
        u, i = np.concatenate(us), np.concatenate(its)
    p = rng.permutation(len(u))
    return u[p].astype(np.int64), i[p].astype(np.int64), nu, ni


def graph_case(name):
    """dict(pairs, n_users, n_items, g = graph(...)) -- computed once per process."""
    if ("g", name) not in _CACHE:
        u, i, nu, ni = graph_pairs(name)
        g = graph(u, i, nu, ni)
        g["A"].setflags(write=False)
        _CACHE[("g", name)] = dict(pairs=(u, i), n_users=nu, n_items=ni, g=g)
    return _CACHE[("g", name)]


def table(name, d, seed=0, scale=0.3):
    c = graph_case(name)
    return (scale * np.random.default_rng(1000 * d + seed).standard_normal((c["n_users"] + c["n_items"], d))).astype(F)


def model_case(name, d, B, seed=0):
    """graph_case plus ego tables E0 float32 [N, d] and a batch of B triplets with hot rows and repeated ids: a third of the positives is item
    0 (the hub of `small`), users are drawn with replacement from 40, and pp / pn are the popularity weights of the PD head."""
    key = ("m", name, d, B, seed)
    if key not in _CACHE:
        c = dict(graph_case(name))
        rng = np.random.default_rng(7 * d + B + seed)
        c["E0"] = table(name, d, seed=seed + 1)
        users = rng.integers(0, min(40, c["n_users"]), B)
        pos, neg = rng.integers(0, c["n_items"], B), rng.integers(0, c["n_items"], B)
        pos[rng.random(B) < 0.33] = 0
        c["batch"] = dict(users=users.astype(np.int32), pos=pos.astype(np.int32), neg=neg.astype(np.int32),
                          pp=(rng.uniform(0, 1, B) ** 0.22).astype(F), pn=(rng.uniform(0, 1, B) ** 0.22).astype(F))
        c["regs"], c["reg_div"] = REGS, float(B)
        _CACHE[key] = c
    return _CACHE[key]


# ---- three whole steps -----------------------------------------------------------------------------------------------------------------------------
def train_steps(case, L, pop, lr, n_steps, batches):
    """n_steps float64 reference steps (the closed-form gradient, the oracle's dense-decay Adam) from case["E0"] -> (E list, m list, v list, losses)."""
    c = dict(case)
    E = case["E0"].astype(np.float64)
    m, v = np.zeros_like(E), np.zeros_like(E)
    out = ([], [], [], [])
    for t in range(1, n_steps + 1):
        c["E0"], c["batch"] = E, batches[t - 1]
        r = model(c, L, pop)
        E, m, v = po.adam_dense_decay_step(E, m, v, r["grad"], t, lr)
        for o, x in zip(out, (E, m, v, r["loss"])):
            o.append(x)
    return out
