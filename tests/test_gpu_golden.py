"""GPU tests that touch the golden fixtures DIRECTLY (no oracle hop), and exact list equality for the popularity head on
boundary-gapped data.

* tests/golden/metrics.json (outputs of the reference's get_performance, MF/used_metric.py:4-80) goes straight through
  pda_metrics on the device.
* The popularity head evaluates exp with the hardware v_exp_f32, libm's expf differs in the last ulp, so on arbitrary data
  a list disagreement inside 1e-5 is a genuine near-tie (tests/test_gpu_score_topk.py accepts exactly that).  On data whose
  K / K+1 gap (and every gap inside the list) exceeds the reassociation bound by orders of magnitude, EXACT equality with
  the float64 restatement can be demanded -- this file builds such data and demands it ("hard parts").
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import pda_oracle as po

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def test_reference_metric_vectors_through_the_device_kernel(dev):
    from pda_amd import ops
    cases = json.load(open(os.path.join(G, "metrics.json")))
    assert len(cases) >= 11
    groups = sorted({(len(c["r"]), tuple(c["Ks"])) for c in cases})           # every list length: one call per (length, cut-offs)
    assert {(50, (20, 50)), (50, (1, 5, 10, 50))} < set(groups)
    done = 0
    for k_cols, Ks in groups:
        sub = [c for c in cases if len(c["r"]) == k_cols and tuple(c["Ks"]) == Ks]
        done += len(sub)
        topk = torch.tensor([c["r"] for c in sub], dtype=torch.int32, device=dev)
        indptr = np.zeros(len(sub) + 1, np.int64)
        indptr[1:] = np.cumsum([len(c["target"]) for c in sub])
        flat = np.concatenate([np.asarray(c["target"], np.int32) for c in sub])
        assert ops.metrics_route(k_cols) is (ops.metrics_sums if k_cols <= 64 else ops.metrics_sums_deep)   # (longer lists: the deep kernel)
        sums = ops.metrics_route(k_cols)(topk, torch.from_numpy(indptr).to(dev), torch.from_numpy(flat).to(dev),
                                         torch.tensor(Ks, dtype=torch.int32, device=dev)).cpu().numpy()
        for row, k in enumerate(("precision", "recall", "ndcg", "hit_ratio")):
            ref = np.sum([c["out"][k] for c in sub], axis=0)
            np.testing.assert_allclose(sums[row], ref, rtol=1e-12, err_msg=k)
    assert done == len(cases)


def gapped_case(seed, nU, nI, d, K, head, gap=1e-4):
    """Embeddings + popularity such that, for every user, consecutive head values around the top K + 8 differ by more than
    `gap` (relative), in float64.  Built by rejection: users whose float64 ranking has a closer pair are re-drawn."""
    rng = np.random.default_rng(seed)
    I = (rng.standard_normal((nI, d)) * 0.1).astype(np.float32)
    pop = (rng.uniform(0.05, 1, nI) ** 0.22).astype(np.float32)
    U = np.empty((nU, d), np.float32)
    for u in range(nU):
        for _ in range(2000):
            cand = (rng.standard_normal(d) * 0.1).astype(np.float32)
            s = I.astype(np.float64) @ cand.astype(np.float64)
            hv = np.where(s > 0, s + 1.0, np.exp(np.minimum(s, 0))) * pop if head else s
            top = np.sort(hv)[::-1][:K + 30]          # (15 of them may be masked train items)
            if np.min(top[:-1] - top[1:]) > gap * max(1.0, np.abs(top).max()):
                U[u] = cand
                break
        else:
            raise AssertionError("no gapped user found")
    return U, I, pop


@pytest.mark.parametrize("kernel", ["v1", "v3", "v4"])
@pytest.mark.parametrize("mode", ["0", "order", "1"])
@pytest.mark.parametrize("d", [64, 128])
def test_popularity_head_lists_are_exactly_the_float64_lists_on_gapped_data(dev, monkeypatch, kernel, mode, d):
    from pda_amd import ops
    if kernel == "v1" and mode != "0":
        pytest.skip("the exact kernel has one sweep mode")
    monkeypatch.setenv("PDA_SCORE_IMPL", "v1" if kernel == "v1" else "v2")
    monkeypatch.setenv("PDA_SCORE_KERNEL", kernel if kernel != "v1" else "v3")
    monkeypatch.setenv("PDA_SCORE_PRUNE", mode)
    nU, nI, K = 96, 700, 20          # (a small catalogue and K = 20: wide gaps between ALL consecutive head values are likely)
    U, I, pop = gapped_case(7 + d, nU, nI, d, K, head=1)
    hist = [np.unique(np.random.default_rng(u).integers(0, nI, 15)).astype(np.int32) for u in range(nU)]
    h = ops.HistoryCSR.from_lists(hist, dev, by_user=True)
    users = torch.arange(nU, dtype=torch.int32, device=dev)
    idx, val = ops.recommend_topk(torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), users, K, ops.HEAD_POP,
                                  torch.from_numpy(pop).to(dev), h)
    # float64 restatement of MF/model_api.py:113 + MF/train_new_api.py:601-604 (mask = -inf, top_k)
    indptr = np.zeros(nU + 1, np.int64)
    indptr[1:] = np.cumsum([len(x) for x in hist])
    ridx, rval = po.recommend_topk(U, I, np.arange(nU), indptr, np.concatenate(hist), K, "condition", pop)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)                       # EXACT lists
    np.testing.assert_allclose(val.cpu().numpy(), rval, rtol=1e-5, atol=1e-5)    # scores: the north_star tolerance
