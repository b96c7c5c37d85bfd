"""GPU: no call may depend on what its workspace or its output buffer held before the call.

pda_amd allocates with torch.empty: workspaces sized by the library's *_workspace_bytes functions, output key arrays, partial sums, plans,
masks and images.  The contract (include/*.h, DESIGN.md "Buffers"): everything a kernel reads from such a buffer was written earlier by the
same call.  Every case of CASES runs a family's EXISTING checks -- the functions of its tests/test_gpu_*.py, with their independent reference
(c_oracle, pda_oracle, the float64 *_ref.py restatements, rank_ref) and their tolerance -- three times, under tests/dirty_buffers.py's three
fills (0x00, 0xFF, 0x3F) of every buffer pda_amd allocates, each between guard bands, and then asserts

  1. (inside the family's checks) the result meets the reference under EVERY fill: equal garbage three times is not a pass;
  2. every tensor any pda_amd.ops call returned or was handed (workspace arguments excepted) is the same under the three fills, bit for bit.
     Only the entry points that sum floats with atomics (dirty_buffers.ATOMIC_STEPS), and calls whose INPUTS already differ because of one of
     them, are held to the case's `tol` instead -- the family's own tolerance against its reference; a deterministic call on equal inputs
     (the ordered metrics, gcn_spmm, ips_weight_sum, the MACR item prep and lists, ssm_normalize_rows, the PCC statistic, score_dense, every
     score call) must give equal bits inside a `tol` case too;
  3. no guard byte in front of or behind any buffer was touched (a *_workspace_bytes a few bytes short, a row one element too long);
  4. the functions the case is there for (`functions`: keys of dirty_buffers.alloc_sites()) did allocate -- a case that silently takes another
     path tests nothing.  tests/test_dirty_buffers_host.py holds the table closed over every torch.empty of pda_amd.

The sweeps run with PDA_CHECK_SWEEP_ERRORS=1 and the families' own identity assertions (which kernel ran).

What was read, per family, before its first run (host function and kernels): see the comment in front of each case.  Cached workspaces reused
across shapes (stale contents, no patch needed) and the C caller's view (run_case: the buffer the allocating function of SIZE_SITE handed to the library's ctypes
entry point was guarded, dirty and of exactly the size the size function reported) follow the table.
"""
import collections
import importlib

import numpy as np
import pytest
import torch

import dirty_buffers as db

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "functions run tol sizes")
# size function of the library -> the function of pda_amd that allocates its buffer (run_case: a buffer of exactly the reported size, from there)
SIZE_SITE = {
    "pda_score_topk4_workspace_bytes": "ops.score_topk_keys",
    "pda_score_topk_workspace_bytes": "ops.score_topk_keys",
    "pda_score_topk7_workspace_bytes": "ops.score_topk_funnel",
    "pda_deep_topk_workspace_bytes": "ops.recommend_topk_deep",
    "pda_metrics_deep_workspace_bytes": "ops._metrics_deep",
    "pda_pc_moments_workspace_bytes": "ops.pc_item_moments",
    "pda_pc_score_workspace_bytes": "ops.recommend_topk_pc",
    "pda_temp_pop_score_workspace_bytes": "ops.score_topk_bias_keys",
    "pda_triplet_plan_large_workspace_bytes": "ops.triplet_plan",
    "pda_bpr_step_plan_scratch_bytes": "ops.bpr_step_plan",
    "pda_bpr_grad_plan_scratch_bytes": "ops._grad_plan_args",
    "pda_metrics_ordered_workspace_bytes": "ops.metrics_sums_ordered",
    "pda_dice_rows_ws_words": "ops.dice_rows_ws",
    "pda_inbatch_workspace_bytes": "ops.inbatch_workspace",
    "pda_fullsm_workspace_bytes": "ops.fullsm_workspace",
    "pda_dau_workspace_bytes": "ops.dau_workspace",
    "pda_ials_workspace_bytes": "ops.IalsGraph.buffers",
    "pda_gcn_spmm_workspace_bytes": "ops.GcnGraph.buffers",
}
CASES = collections.OrderedDict()

# Functions that allocate with torch.empty and need no case: function -> one-line reason (tests/test_dirty_buffers_host.py accepts two kinds).
EXEMPT = {
    "model_api._MFBase.init_weights": "overwritten by torch: Tensor.uniform_ fills the whole table in the same expression (xavier_uniform_)",
    "model_api.BPRMFTempPop.init_weights": "overwritten by torch: Tensor.uniform_ fills the whole table in the same expression (xavier_uniform_)",
    "model_api.DICE.init_weights.table": "overwritten by torch: Tensor.uniform_ fills both halves in the same expression (xavier_uniform_)",
    "model_api.MACRBPRMF.init_weights": "overwritten by torch: Tensor.uniform_ fills the whole vector in the same expression (xavier_uniform_)",
    "ops.measured_peaks": "measurement tool: the destination of a timed copy_, never read",
}

SCORE_ENV = ("PDA_SCORE_LISTS", "PDA_SCORE_KERNEL", "PDA_HUGE_SPLITS", "PDA_SCORE_IMPL", "PDA_SCORE_PRUNE", "PDA_WARM_PER_SPLIT", "PDA_WARM_ONE_KERNEL",
             "PDA_WARM_MASK_TABLE", "PDA_WARM_TILES", "PDA_SCORE_FUNNEL", "PDA_SWEEP_TAIL_SHARE", "PDA_SWEEP_TAIL_OTHERS_FIRST", "PDA_SWEEP_TAIL_MIN_CHUNK",
             "PDA_TEMP_POP_KERNEL")


def case(name, functions, tol=None, sizes=()):
    """functions: what must allocate (dirty_buffers.alloc_sites() names); tol: (rtol, atol) across the fills, None = bit for bit, or (rtol, atol,
    fraction of elements that may lie outside, largest error allowed) as dirty_buffers.same_records takes them; sizes: the
    library's size functions whose buffer the case hands over at exactly the reported size (the C caller's view, see run_case)."""
    def register(fn):
        assert name not in CASES
        CASES[name] = Case(tuple(functions), fn, tol, tuple(sizes))
        return fn
    return register


def T(module):
    """A family's existing GPU test module (its checks are called as plain functions; its autouse environment is set by clean_env / score_env)."""
    return importlib.import_module(module)


def clean_env(mp, **env):
    """What the autouse fixtures of the score tests do: no forcing variable left from outside, sweep errors checked."""
    for k in SCORE_ENV:
        mp.delenv(k, raising=False)
    mp.setenv("PDA_CHECK_SWEEP_ERRORS", "1")
    for k, v in env.items():
        mp.setenv(k, v)


def score_env(mp, impl):
    """tests/test_gpu_score_topk.py's `impl` fixture: the nine scoring paths."""
    clean_env(mp, PDA_SCORE_IMPL="v1" if impl == "v1" else "v2",
              PDA_SCORE_PRUNE={"v2ord": "1", "v2order_only": "order", "k4ord": "order", "k4stop": "1", "k4huge": "order"}.get(impl, "0"),
              PDA_SCORE_LISTS={"k4many": "many", "k4huge": "huge"}.get(impl, "lds"), PDA_SCORE_KERNEL="v4" if impl.startswith("k4") else "old")


# ---------------------------------------------------------------------------------------------------------------------------------------
# Generations 1, 3 and 4 of the score + top-K call (ops.score_topk_keys, ops.topk_merge).
#   out keys [n_splits, Bu, K]     only written: every (split, row) list in full, zeros behind a short list (test_fewer_than_k_unmasked_items)
#   generation 1 / 3 workspace     pda_score_topk_workspace_bytes(Bu): cleared in full by the call (hipMemsetAsync, pda_score_prep.hip)
#   generation 4 workspace         [0, lists): counters, error word, identity word and the shared-tail records -- cleared by every call that
#                                  starts a ranking (phase 1, 3, 4; hipMemsetAsync in run_score4); phase 2 (seeded_finish) keeps phase 1's on purpose
#                                  list slots, Bloom filters, masks, regrouping bins, hand-over, user image, norms, seed, K-th values, warm-up
#                                  scores: written by the call's own kernels before its later kernels read them (bins: hipMemsetAsync)
#   item preps (cached)            header and the maxima: hipMemsetAsync; pos_of: 0xFF memset, then scattered; everything else only written
#   topk_merge out                 only written, every element (a short row completed from the history, -1 behind)
_ORACLE = {}


def _score_case(d):
    """test_gpu_score_topk.make_case at the issue's shape (300 users, 173 picked, 1 999 items, K = 50), built once per d"""
    if d not in _ORACLE:
        S = T("test_gpu_score_topk")
        rng = np.random.default_rng(100 + d)
        U, I, pop, hist = S.make_case(rng, 300, 1999, d)
        users = rng.permutation(300)[:173].astype(np.int32)
        _ORACLE[d] = (U, I, pop, hist, users)
    return _ORACLE[d]


def _score_paths(dev, mp, impl):
    S = T("test_gpu_score_topk")
    score_env(mp, impl)
    for d in (64, 256):
        U, I, pop, hist, users = _score_case(d)
        rows = [hist[u] for u in users]
        for head in (0, 1):
            for by_user in (True, False):
                for n_splits in (1, 3):
                    idx, val, keys = S.run_gpu(dev, U, I, users, 50, head, pop if head else None, hist if by_user else rows, by_user=by_user, n_splits=n_splits)
                    assert keys.shape == (n_splits, 173, 50)
                    S.check_against_oracle(idx, val, U, I, users, 50, head, pop, rows, exact=(head == 0))
    S.test_fewer_than_k_unmasked_items(dev)               # unwritten list tails show here
    S.test_exact_ties_resolve_to_lower_index(dev)
    if impl != "v1":
        S.test_bf16_tables_return_the_keys_of_the_widened_fp32_tables(dev, 64, 1, impl)
        S.test_bf16_tables_return_the_keys_of_the_widened_fp32_tables(dev, 256, 0, impl)


def _score(impl, functions):
    @case("score_" + impl, functions, sizes=() if impl == "v1" else ["pda_score_topk4_workspace_bytes" if impl.startswith("k4") else "pda_score_topk_workspace_bytes"])
    def run(dev, mp):
        _score_paths(dev, mp, impl)
    return run


_score("v1", ["ops.score_topk_keys", "ops.topk_merge"])
_score("v2", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep"])
_score("v2ord", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep_ordered", "ops.hist_reordered"])
_score("v2order_only", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep_ordered", "ops.hist_reordered"])
_score("k4nat", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep4"])
_score("k4ord", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep4", "ops.warm_mask_table"])
_score("k4stop", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep4", "ops.warm_mask_table"])
_score("k4many", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep4"])
_score("k4huge", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep4", "ops.warm_mask_table"])


# The huge geometry of generation 4 behind the two-kernel and the one-kernel warm-up (test_gpu_warm_split.both_warm_ups: the keys against the
# exact kernel's, the user image, the norms and the K-th values of the two warm-ups against each other), several splits behind the shared
# warm-up, and the shared test-free tail (test_gpu_tail_share: records exhausted, counters equal with and without sharing).
#   tail records   behind the counters, inside the memset of the counters (run_score4); test_two_calls_on_one_workspace holds a 0xFF workspace
@case("score_huge", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep4", "ops.warm_mask_table"])
def _(dev, mp):
    W = T("test_gpu_warm_split")
    clean_env(mp)
    for d, bf16 in ((64, False), (128, True)):
        # (three splits at 1 500 items: at 700 a split is four 64-item tiles, the warm-up itself, and no sweep kernel would run)
        for n_splits, nI in ((1, 700), (3, 1500)):
            rng = np.random.default_rng(1100 + d + nI)
            U, I, pop, rows = W.flat_case(rng, 1400, nI, d)
            if bf16:
                U, I = W.bf16_exact(U), W.bf16_exact(I)
            users = rng.permutation(1400)[:1100]
            for by_user in (True, False):
                _, _, st = W.both_warm_ups(dev, mp, U, I, pop, rows, users, by_user=by_user, bf16=bf16, n_splits=n_splits)
                assert st["n_splits"] == n_splits
    W.test_without_a_history(dev, mp)
    W.test_split_boundaries(dev, mp, 288)
    W.test_split_boundaries(dev, mp, 256)


@case("score_huge_tail_share", ["ops.score_topk_keys", "ops.topk_merge", "ops.item_prep4", "ops.warm_mask_table"])
def _(dev, mp):
    S = T("test_gpu_tail_share")
    clean_env(mp, PDA_SCORE_IMPL="v2", PDA_SCORE_PRUNE="order", PDA_SCORE_LISTS="huge", PDA_SCORE_KERNEL="v4", PDA_SWEEP_TAIL_MIN_CHUNK="2")
    S._cases.clear()                                       # (its shared tensors and exact keys are built under this fill)
    S.test_keys_and_counters_with_and_without_sharing(dev, mp, 2050, 1500, 64, False, 1, "steep")
    S.test_keys_and_counters_with_and_without_sharing(dev, mp, 2050, 1500, 128, True, 3, "steep")
    S.test_keys_and_counters_with_and_without_sharing(dev, mp, 2050, 1500, 64, True, 3, "flat")
    S._cases.clear()


# The seeded three-step call of an item-sharded sweep (seeded_begin / seeded_counts / seeded_finish, kth_value, sweep_from_seed).
#   c.out, c.ws      one generation-4 workspace through phase 1 and phase 2: phase 1 clears the counters, phase 2 reads phase 1's lists
#   bounds [3, Bu], counts [n_thr, Bu], seed [Bu], kth_value out [Bu]: only written, one thread per user writes every element
@case("score_seeded", ["ops.seeded_begin", "ops.seeded_counts", "ops.seeded_finish", "ops.item_prep4", "ops.topk_merge"])
def _(dev, mp):
    """test_seeded_item_shards_equal_one_shard's protocol (R = 2, head 1; R = 4: the second collective) with the shards one after the other in
    ONE thread (its threads would record their calls in an order of their own), on the score case's data, against the C oracle."""
    from pda_amd import ops
    from pda_amd.dist import shard_range
    S = T("test_gpu_score_topk")
    clean_env(mp)
    rng = np.random.default_rng(662)
    nU, nI, K = 300, 5000, 50
    U, I, pop, hist = S.make_case(rng, nU, nI, 64)
    users = rng.permutation(nU)[:173].astype(np.int32)
    Ut, It, pt, ut = (torch.from_numpy(x).to(dev) for x in (U, I, pop, users))
    h = ops.HistoryCSR(*(torch.from_numpy(x).to(dev) for x in S.csr(hist)), by_user=True)
    for R in (2, 4):
        calls = []
        for r in range(R):
            lo, hi = shard_range(nI, r, R)
            st = {}
            calls.append((ops.seeded_begin(Ut, It[lo:hi].contiguous(), ut, K, ops.HEAD_POP, pt[lo:hi].contiguous(), h, lo, 1, R, stats=st), st))
        bounds = torch.stack([c.bounds for c, _ in calls]).max(0).values                  # the MAX all-reduce
        for c, _ in calls:
            c.bounds.copy_(bounds)
        counts = [ops.seeded_counts(c) for c, _ in calls]
        assert (counts[0] is not None) == (R >= 4)
        if counts[0] is not None:
            total = torch.stack(counts).sum(0)                                            # the SUM all-reduce
            for c in counts:
                c.copy_(total)
        parts = []
        for c, st in calls:
            parts.append(ops.topk_merge(ops.seeded_finish(c), want="keys"))
            assert int(st["error"][0]) == 0
            assert ops.kernel_identity(st["kernel_id"][0])["generation"] in (0, 4)
        idx, val = ops.topk_merge(torch.stack(parts).contiguous(), ut, h)
        torch.cuda.synchronize()
        S.check_against_oracle(idx.cpu().numpy(), val.cpu().numpy(), U, I, users, K, 1, pop, [hist[u] for u in users], exact=False)


@case("score_from_seed", ["ops.sweep_from_seed", "ops.kth_value", "ops.item_prep4"])
def _(dev, mp):
    H = T("test_gpu_hot_items")
    clean_env(mp)
    H.test_sweep_from_seed_without_a_bound_is_the_plain_sweep(dev, mp)
    H.test_emulated_item_shards_with_replicated_hot_items(dev, mp, 128, 700, 5000, 20, 8, 128, "order", False)
    H.test_remap_key_items_matches_the_torch_expression(dev)


# The funnel (pda_score_topk7_*), with its in-call exact fallback (generation 4 inside the funnel's workspace).
#   [0, 256)                        counters, error and identity word: hipMemsetAsync
#   thr, tk, tmax, ncand, flags, fail_count: init7_kernel, every row;  user image, norms, residual norms: uprep5_kernel incl. padding rows
#   ecnt (list cursors)             written by every sweep7 wave before expand7_kernel reads it (clamped to cap_e there);  qcnt: written by
#                                   expand7_kernel for every (row, quarter, split) before threshold7_kernel reads it
#   fb_ws                           a generation-4 workspace: run_score4 clears its counters as in every call
@case("score_funnel", ["ops.score_topk_funnel", "ops.item_prep7", "ops.topk_merge", "ops.score_topk_keys", "ops.item_prep4"],
      sizes=["pda_score_topk7_workspace_bytes"])
def _(dev, mp):
    F = T("test_gpu_funnel")
    clean_env(mp)
    F.test_blocks_of_few_users_take_the_funnel_unforced(dev, mp, 64, 5000, 7)
    clean_env(mp)
    F.test_blocks_of_few_users_take_the_funnel_unforced(dev, mp, 128, 5000, 64)
    clean_env(mp)
    F.test_funnel_equals_the_oracle(dev, mp, 128, 50, True, True)                # bf16 tables
    clean_env(mp)
    F.test_funnel_lost_bets_and_overflowing_lists_take_the_exact_fallback(dev, mp, 128)
    clean_env(mp)
    F.test_funnel_ties_zero_rows_and_short_lists(dev, mp)


# The per-block pieces as calls of their own: user images, Bloom filters, warm-position masks, the item preps field by field, the reordered
# history.  All only written: padding rows of an image and of the mask rows are written as zeros (asserted by the families' checks).
@case("prep_user_side", ["ops.huge_user_image", "ops.funnel_user_image", "ops._bloom_out"])
def _(dev, mp):
    P, ur = T("test_gpu_user_prep"), T("user_prep_ref")
    clean_env(mp)
    P._TABLES.clear()
    for d, n in ((64, 17), (64, 257), (256, 129)):
        for bf16 in (False, True):
            for f16 in (False, True):
                P.test_every_field_of_the_user_image(dev, ur.Case(d, bf16, f16, n))
    for c in (ur.BloomCase(False, True, 33), ur.BloomCase(False, False, 31), ur.BloomCase(True, True, 33), ur.BloomCase(True, False, 70)):
        P.test_bloom_rows(dev, c)
    P.test_generation_4_skips_the_filters_of_an_ordered_prep(dev, True)
    from pda_amd import ops
    for funnel in (False, True):                           # the filters into a buffer of the call's own (ops._bloom_out)
        c = ur.BloomCase(funnel, True, 33)
        indptr, indices = ur.make_history(funnel)
        users = ur.make_bloom_users(c)
        ut, h = torch.from_numpy(users).to(dev), P.device_history(dev, funnel, True)
        if funnel:
            order, pos_of = ur.shard_order()
            prep7 = ops.item_prep7(P.item_table(dev, ur.SHARD_ITEMS), torch.from_numpy(order).to(dev))
            got = ops.funnel_bloom_rows(prep7, ut, h, ur.SHARD_OFFSET, ur.SHARD_ITEMS, 64)
        else:
            got = ops.hist_bloom_rows(ops.item_prep4(P.item_table(dev, 64), None, None), ut, h)
        assert tuple(got.shape) == (c.n, 32)
        R = ur.check_bloom(got.cpu().numpy().view(np.uint32), users, indptr, indices, True, (pos_of, ur.SHARD_OFFSET) if funnel else None)
        assert not R.failed, R.failed
    P._TABLES.clear()


@case("prep_item_side", ["ops.item_prep", "ops.item_prep_ordered", "ops.item_prep4", "ops.item_prep7"])
def _(dev, mp):
    P, pr = T("test_gpu_item_prep"), T("prep_ref")
    clean_env(mp)
    small = min(c.n for c in pr.gpu_cases())
    picked = [c for c in pr.gpu_cases() if c.d == 64 and c.n in (small, 4097)]
    assert {c.kind for c in picked} >= {"prep4", "prep7", "gen3o"}, {c.kind for c in picked}
    named = {}
    for c in picked:
        P.test_every_field_of_the_prep(dev, c)
        inp = pr.make_inputs(c)                  # every byte the layout names (the gaps between the fields belong to nobody), for the three fills
        blob, _, _ = P.build(dev, c, inp)
        for k, v in pr.named_bytes(pr.decode(c, blob, inp["pop"] is not None)).items():
            named["%s.%s" % (pr.case_id(c), k)] = np.array(v, copy=True)
    P.test_hist_reorder_rows(dev)
    return named


@case("prep_warm_mask", ["ops.warm_mask_table", "ops.warm_mask_rows", "ops.item_prep4"])
def _(dev, mp):
    M = T("test_gpu_warm_mask_table")
    clean_env(mp)
    M.test_table_rows_equal_the_per_call_kernel(dev, mp, 1000, 4, 0, "repeats")
    M.test_table_rows_equal_the_per_call_kernel(dev, mp, 1000, 2, 300, "descending")
    M.test_keys_with_the_table_without_it_and_exact(dev, mp, 64, "order", 1100)


# pda_topk_merge and pda_deep_merge (lists of the item shards): outputs only written; deep_merge's folded intermediate is written in full
# by the launches that fold into it before the next level reads it.
@case("merge", ["ops.topk_merge", "ops.deep_merge"])
def _(dev, mp):
    S, D = T("test_gpu_score_topk"), T("test_gpu_deep_shard")
    score_env(mp, "k4nat")
    S.test_merge_matches_numpy_oracle(dev)
    S.test_item_shards_merge_equals_single_device(dev)
    D.test_merge_kernel_equals_numpy_bit_for_bit(dev, 1, 55)
    D.test_merge_kernel_equals_numpy_bit_for_bit(dev, 3, 100)
    D.test_folding_equals_numpy(dev, 9, 1024)
    D.test_short_rows_across_shards_end_in_their_history_by_id(dev, 257)


# The deep lists (pda_deep_topk_*; ops._DEEP_WS is cached across calls).
#   header [0, 256)   cleared by the call (hipMemsetAsync in deep_topk -- moved there from ops.py by this change); identity word at +16
#                     written by workgroup 0 of the sweep
#   counts            one word per (split, row of the padded block): written by the sweep for every row of every tile it launches, read by the
#                     final kernel for rows < n_users only;  lists: `count` keys per (split, row) written, exactly those read
#   out_keys / idx / val   only written, K elements per row (a short row: zeros / -inf / the listed items by id, then -1)
@case("deep_lists", ["ops.recommend_topk_deep", "ops.score_dense"], sizes=["pda_deep_topk_workspace_bytes"])
def _(dev, mp):
    D = T("test_gpu_deep_topk")
    clean_env(mp)
    D.test_raw_head_equals_the_oracle_exactly(dev, 64, 100, 1999)
    D.test_raw_head_equals_the_oracle_exactly(dev, 128, 1000, 1999)
    D.test_pop_head_three_ways(dev, 128, 1000, 1999)
    D.test_pop_head_three_ways(dev, 64, 55, 1999)
    D.test_bf16_tables_equal_the_widened_fp32_tables(dev, 64, 1)
    D.test_bf16_tables_equal_the_widened_fp32_tables(dev, 128, 0)
    D.test_short_rows_end_in_their_listed_items_by_id(dev)
    D.test_identity_word_names_the_kernel(dev, 64, 1)
    D.test_chunked_users_equal_one_call(dev)


# pda_metrics_deep sums with float64 atomics unless ordered: the three fills are compared at the family's rtol against its oracle (1e-12).
@case("deep_metrics", ["ops._metrics_deep"], tol=(1e-12, 0.0), sizes=["pda_metrics_deep_workspace_bytes"])
def _(dev, mp):
    D = T("test_gpu_deep_topk")
    D.test_deep_metrics_against_the_oracle(dev, 100)
    D.test_deep_metrics_against_the_oracle(dev, 1000)


# Exact full-catalogue ranks (pda_rank_*): ops allocates the outputs with torch.zeros (no torch.empty in the family); the case holds the
# cached preps and orders it shares with the score calls.
@case("rank", ["ops.item_prep4", "ops.score_dense"])
def _(dev, mp):
    R = T("test_gpu_rank")
    clean_env(mp)
    R.dense.cache_clear()                                  # (its reference matrix is ops.score_dense's: computed under this fill)
    R.reference.cache_clear()
    for head in (0, 1):
        R.test_keys_are_the_dense_kernels_bits(dev, 64, head)
        R.test_ranks_equal_the_reference_on_the_dense_matrix(dev, 64, 1999, head)
    R.test_no_history_and_no_target(dev)
    R.test_ranks_agree_with_the_lists(dev, 64, 5000, 1)


# Metrics: pda_metrics (float64 atomics) and the ordered reduction through ops._METRICS_WS (cached): one partial sum per (block, row of sums,
# cut-off), every one written by its block before the second kernel adds them in a fixed order.
def _metrics_rows(n, K=50, n_items=3000, seed=31):
    """test_gpu_bpr_step.test_metrics_kernel's data at n rows -> (topk, indptr, flat targets)"""
    rng = np.random.default_rng(seed + n)
    topk = np.stack([rng.permutation(n_items)[:K] for _ in range(n)]).astype(np.int32)
    targets = [rng.permutation(n_items)[:rng.integers(1, 80)].astype(np.int32) for _ in range(n)]
    for r in range(0, n, 3):    # make hits likely
        targets[r][: min(5, len(targets[r]))] = topk[r][rng.permutation(K)[: min(5, len(targets[r]))]]
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([len(t) for t in targets])
    return topk, indptr, np.concatenate(targets)


def _metrics_against_the_oracle(dev, fn, n, Ks):
    from oracle import c_oracle
    B = T("test_gpu_bpr_step")
    topk, indptr, flat = _metrics_rows(n)
    Ks = np.asarray(Ks, np.int32)
    sums = fn(*B.to(dev, topk, indptr, flat, Ks))
    np.testing.assert_allclose(sums.cpu().numpy(), c_oracle.metrics(topk, indptr, flat, Ks), rtol=1e-12)
    return sums


@case("metrics", ["ops.metrics_sums_ordered"], tol=(1e-12, 0.0))
def _(dev, mp):
    from pda_amd import ops
    B, D = T("test_gpu_bpr_step"), T("test_gpu_deterministic")
    B.test_metrics_kernel(dev)
    for n in (1000, 1, 257):
        _metrics_against_the_oracle(dev, ops.metrics_sums, n, (20, 50))
    D.test_ordered_metrics_equal_the_atomic_ones_and_repeat_bit_for_bit(dev)


@case("metrics_ordered", ["ops.metrics_sums_ordered"], sizes=["pda_metrics_ordered_workspace_bytes"])
def _(dev, mp):
    from pda_amd import ops
    D = T("test_gpu_deterministic")
    for n in (1000, 1, 257):
        _metrics_against_the_oracle(dev, ops.metrics_sums_ordered, n, (20, 50))
    D.test_ordered_metrics_meet_the_reference_vectors(dev)


# Exposure counts, xQuAD re-ranking, BPR-PC (moments, user statistics, score + re-rank).
#   xquad idx / val      only written, K per row;  exposure: torch.zeros accumulators (no torch.empty)
#   pc moments out       float64 [2 d d + d + 1]: written in full by the second kernel from the workspace's per-block partials, each written first
#   pc score workspace   header (identity, fallback count) cleared by the call; minima per row block written before the re-rank reads them
@case("exposure_xquad", ["ops.xquad_rerank"])
def _(dev, mp):
    E, X = T("test_gpu_exposure"), T("test_gpu_xquad")
    clean_env(mp)
    for k_cols in (1, 50, 65):
        E.test_shapes(dev, k_cols)
    E.test_targets_empty_unsorted_duplicated_and_absent(dev)
    for variant in ("smooth", "binary"):
        X.test_lists_bit_exact(dev, 50, 20, variant)
        X.test_lists_bit_exact(dev, 65, 64, variant)
    X.test_short_rows(dev, 100, 20, "minus_one")
    X.test_rows_off_16_byte_boundaries(dev, 63)


@case("bpr_pc", ["ops.pc_item_moments", "ops.pc_user_stats", "ops.recommend_topk_pc"],
      sizes=["pda_pc_moments_workspace_bytes", "pda_pc_score_workspace_bytes"])
def _(dev, mp):
    P = T("test_gpu_bpr_pc")
    clean_env(mp)
    P.test_item_moments(dev, 64)
    for mode in ("user_id", "block_row"):
        P.test_user_stats(dev, 64, 0.3, mode)
        P.test_lists_bit_exact(dev, 64, 20, mode)
    P.test_lists_bit_exact(dev, 256, 50, "user_id")
    P.test_forced_fallback(dev)
    P.test_fill_rows_with_few_unmasked_items(dev)


# The bias head (temp_pop's score call), both kernels: the workspace is generation 1 / 3's (cleared in full by the call).
@case("score_bias_head", ["ops.score_topk_bias_keys", "ops.topk_merge"], sizes=["pda_temp_pop_score_workspace_bytes"])
def _(dev, mp):
    P = T("test_gpu_temp_pop")
    for kernel in sorted(P.KERNELS):
        for mode in ("user_id", "block_row"):
            clean_env(mp)
            P.test_bias_kernels_equal_the_oracle(dev, mp, kernel, 64, 20, mode)
        clean_env(mp)
        P.test_bias_kernel_worst_case_rounding_row(dev, mp, kernel)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Training.  Gradient accumulators, moments, tags and loss words are torch.zeros of the callers (not torch.empty); what torch.empty gives the
# training calls: the triplet plans and the large plan's cached workspace, the scratch of the planned step and gradient, sampler outputs,
# the per-family workspaces.
# Triplet plans: the LDS plan writes header, segments and flags in one workgroup; the large plan (B > 4 096) clears its header and flags
# (hipMemsetAsync) and sorts through ops._PLAN_WS, whose histogram is cleared by the call.
@case("plan", ["ops.triplet_plan", "ops.bpr_step_plan", "ops._grad_plan_args"],
      sizes=["pda_triplet_plan_large_workspace_bytes", "pda_bpr_step_plan_scratch_bytes", "pda_bpr_grad_plan_scratch_bytes"])
def _(dev, mp):
    P, D = T("test_gpu_bpr_plan"), T("test_gpu_deterministic")
    for B in (37, 300, 4097):
        P.test_triplet_plan_is_the_sorted_segmentation_of_pos_and_neg(dev, B)
    P.test_planned_exact_sgd_equals_the_oracle_on_a_hot_item_batch(dev, 32, True)
    P.test_large_plan_path_gives_the_same_tables_as_the_lds_plan(dev, mp)
    D.test_planned_gradient_matches_the_float64_oracle(dev, 64, True, D.SMALL, 1024)
    D.test_three_adam_steps_match_the_oracle(dev, "adam_step_plan")


# The fused BPR step and the Adam sweeps sum gradients with float atomics: compared across fills at the family's 1e-5.
@case("bpr_step", ["ops.sgd_step_exact", "ops.sample_triplets"], tol=(1e-5, 1e-5))
def _(dev, mp):
    B = T("test_gpu_bpr_step")
    B.test_loss_and_gradients(dev, 32, True)
    B.test_sgd_fused_update_with_duplicate_items(dev, True)
    B.test_sgd_fused_plain_user_store_with_distinct_users(dev, 32)
    B.test_exact_sgd_step_on_a_hot_item_batch_at_realistic_lr(dev, 0.05)
    B.test_bf16_tables_step(dev, 64)
    B.test_group_triplets_by_pos(dev, 37)
    B.test_sampler_semantics(dev)
    B.test_device_counter_sampler_draws_the_same_batches(dev)
    B.test_sampler_many_batches_ahead(dev)


# The Adam sweeps (2, 3, 4 streams of tables, tagged, lazy) behind the atomically summed gradient.  No torch.empty of their own; the tables are
# held to the three fills by the family's own criterion for Adam tables against its oracle, test_gpu_bpr_step.adam_close: 1e-5, fewer than
# one element in 1 000 beyond it, none beyond 2e-4 (a gradient component of the size of Adam's epsilon turns the ORDER of the atomic adds into
# 1e-5 .. 1e-4 of the element; measured here: 3e-6 between two runs under one fill, beyond 1e-5 in one run of a few).
@case("adam_sweeps", [], tol=(1e-5, 1e-5, 1e-3, 2e-4))
def _(dev, mp):
    B = T("test_gpu_bpr_step")
    B.test_reference_faithful_adam_three_steps(dev)
    B.test_exact_lazy_adam_equals_the_dense_sweep_bit_for_bit(dev, True)
    B.test_two_table_adam_sweep_equals_two_sweeps(dev)
    B.test_six_stream_adam_sweep_equals_the_seven_stream_sweep(dev, 32)
    B.test_two_launch_adam_step_equals_the_step_plus_seven_stream_sweep(dev, 64, 1)
    B.test_tagged_adam_sweep_equals_the_seven_stream_sweep_on_given_gradients(dev)


# The baselines.  Each family: the smallest parametrisation of its gradient check against the float64 restatement, and its three whole steps.
@case("temp_pop", ["ops.score_topk_bias_keys"], tol=(1e-4, 2e-5))
def _(dev, mp):
    P = T("test_gpu_temp_pop")
    clean_env(mp)
    P.test_step_loss_and_gradients(dev, 64, 3, "mixed")
    P.test_three_adam_steps_over_the_four_tables(dev, 64, 10)
    P.test_the_library_picks_the_prefiltered_kernel(dev, mp)


@case("dice", ["ops._dice_sample_out", "ops.score_dense", "ops.dice_rows_ws"], tol=(0.0, 1e-5), sizes=["pda_dice_rows_ws_words"])
def _(dev, mp):
    D, dr = T("test_gpu_dice"), T("dice_ref")
    clean_env(mp)
    D.test_gradients_and_loss_against_the_float64_restatement(dev, 32, 7)
    D.test_three_whole_steps_against_the_restatement(dev, "l1")
    D.test_sampler_equals_the_restatement_bit_for_bit(dev, *dr.PARITY_CASES[1])
    D.test_sampler_with_given_users_and_the_margin_schedule(dev)
    D.test_evaluation_paths_serve_the_concatenated_tables(dev)


@case("ips", ["ops.ips_weight_sum"], tol=(0.0, 1e-5))
def _(dev, mp):
    P = T("test_gpu_ips")
    P.test_gradients_and_loss_against_the_float64_restatement(dev, 32, 7)
    P.test_three_whole_steps_against_the_restatement(dev, "clip_norm")
    P.test_the_weight_sum_keeps_its_bits_and_is_within_an_ulp(dev)


@case("macr", ["ops.MacrItemPrep.__init__", "ops.macr_item_bias", "ops.score_topk_bias_keys"], tol=(0.0, 1e-5))
def _(dev, mp):
    M, mr = T("test_gpu_macr"), T("macr_ref")
    clean_env(mp)
    M.test_loss_and_gradients_against_the_float64_restatement(dev, 32, 7, mr.KINDS[0])
    M.test_three_whole_steps_against_the_restatement(dev, 32)
    M.test_item_prep_against_float64_and_bit_stable(dev, 64)
    M.test_lists_equal_the_contract_and_respect_the_float64_model(dev, mp, mr.LIST_SHAPES[1], 64, 50)


@case("ssm", ["ops.ssm_sample", "ops.ssm_normalize_rows"], tol=(0.0, 1e-5))
def _(dev, mp):
    S, sr = T("test_gpu_ssm"), T("ssm_ref")
    small = [c for c in sr.CASES if c[0] == 32]
    S.test_gradients_and_loss_against_the_float64_restatement(dev, small[0])
    S.test_gradients_and_loss_against_the_float64_restatement(dev, small[-1])
    S.test_three_whole_steps_against_the_restatement(dev, 1, 1)
    S.test_the_sampler_equals_its_restatement_bit_for_bit(dev, 5)
    S.test_normalised_rows_are_within_two_ulp_and_keep_their_bits(dev, 64)


# In-batch softmax, full softmax and DirectAU: a batch in which a user or an item repeats adds its rows' gradients with float atomics (the
# bit-reproducible form needs distinct users), so the fills are compared at the families' 1e-5 against their restatements.
# Their gradient checks fill the workspace with 0xFF themselves (kept); the whole steps run on the workspace as this module's fill left it.
@case("inbatch", ["ops.inbatch_workspace", "ops.inbatch_mask"], tol=(0.0, 1e-5), sizes=["pda_inbatch_workspace_bytes"])
def _(dev, mp):
    S, ir = T("test_gpu_inbatch"), T("inbatch_ref")
    small = [c for c in ir.CASES if c[0] == 32]
    S.test_gradients_and_loss_against_the_float64_restatement(dev, small[0])
    S.test_gradients_and_loss_against_the_float64_restatement(dev, small[-1])
    S.test_the_train_mask_bit_for_bit_against_python_sets(dev, 33)
    S.test_three_whole_steps_against_the_restatement(dev, 1, 1)


@case("inbatch_model", ["model_api.SSMBPRMF._inbatch_buffers", "ops.inbatch_workspace"], tol=(0.0, 1e-5))
def _(dev, mp):
    """The model's own mask buffer (torch.empty in SSMBPRMF._inbatch_buffers, written by pda_inbatch_mask each step) against python sets."""
    S, H, ir = T("test_gpu_inbatch"), T("test_inbatch_host"), T("inbatch_ref")
    from pda_amd.model_api import SSMBPRMF
    B = 2 * ir.T + 5
    c = ir.make_case(500 + B, 32, B)
    model = SSMBPRMF(H.make_args(batch_size=B), {"n_users": c["nU"], "n_items": c["nI"]}, device=dev, seed=3)
    ut, pt, ip, ix = S.to(dev, c["users"], c["pos"], *ir.csr(c["train"], c["nU"]))
    model.set_train_graph(ip, ix, None)
    loss = model.train_step(ut, pt)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
    np.testing.assert_array_equal(model._inbatch["mask"].cpu().numpy(), ir.pack_mask(ir.exclusion(c["users"], c["pos"], c["train"], c["nU"], c["nI"])))


@case("fullsm", ["ops.fullsm_workspace"], tol=(0.0, 1e-5), sizes=["pda_fullsm_workspace_bytes"])
def _(dev, mp):
    S, fr = T("test_gpu_fullsm"), T("fullsm_ref")
    small = [c for c in fr.CASES if c[0] == 32]
    S.test_gradients_loss_and_row_statistics_against_the_float64_restatement(dev, small[0])
    S.test_gradients_loss_and_row_statistics_against_the_float64_restatement(dev, small[-1])
    S.test_three_whole_steps_against_the_restatement(dev, 1, 1)
    S.test_two_calls_on_distinct_users_give_the_same_bits(dev, 256, 257)


@case("dau", ["ops.dau_workspace"], tol=(0.0, 1e-5), sizes=["pda_dau_workspace_bytes"])
def _(dev, mp):
    S, dr = T("test_gpu_dau"), T("dau_ref")
    small = [c for c in dr.CASES if c[0] == 32]
    S.test_gradients_and_loss_against_the_float64_restatement(dev, small[0])
    S.test_gradients_and_loss_against_the_float64_restatement(dev, small[-1])
    S.test_three_whole_steps_against_the_restatement(dev, 1)
    S.test_the_same_inputs_give_the_same_bits(dev, 64, 2 * dr.T + 5)


@case("dns", ["ops.dns_sample"])
def _(dev, mp):
    S = T("test_gpu_dns")
    S.test_one_candidate_is_the_triplet_sampler_bit_for_bit(dev, 37, True, 1, (0, T("dns_ref").NI))
    S.test_exact_data_give_the_restatement_itself(dev, 32, 5, 3, 37)
    S.test_rounded_data_stay_inside_the_a_priori_bound(dev, T("dns_ref").HEAD_POP, 32, 5, 5, 37)
    S.test_two_calls_are_bit_equal(dev, 32, 256)


@case("ials", ["ops.IalsGraph.buffers", "ops.ials_gram", "ops.ials_half_sweep"], sizes=["pda_ials_workspace_bytes"])
def _(dev, mp):
    from pda_amd import ops
    S, ir = T("test_gpu_ials"), T("ials_ref")
    rows, cols = ir.length_graph()
    lengths = (rows, cols) + tuple(ir.csr(rows, cols, S.NR))          # (its `lengths` fixture)
    S.test_the_normal_equations_are_exact_bit_for_bit(dev, lengths, 32, 0.25)
    S.test_the_solve_stays_inside_the_a_priori_bound(dev, lengths, 32, ir.TABLES[1], ir.PARAMS[0])
    S.test_bits_do_not_depend_on_the_call(dev)
    S.test_one_epoch_of_the_model_is_the_restatement_s_epoch(dev)
    # a work list that needs more workspace than the graph holds: ials_half_sweep takes a new one of the reported size (same bits)
    g = S.graph_of(dev, rows, cols, S.NR, ir.N_OTHER, 0.1, 0.05, 1.0)
    Z = torch.from_numpy(ir.table("gauss0.3", ir.N_OTHER, 32)).to(dev)
    G = ops.ials_gram(Z)
    base = ops.ials_half_sweep(g, "user", Z, torch.full((S.NR, 32), float("nan"), device=dev), G=G)
    b = g.buffers(32)
    assert g.user.all_rows.n_slots > 0 and b["ws"].numel() > 16
    b["ws"] = b["ws"][:16]
    again = ops.ials_half_sweep(g, "user", Z, torch.full((S.NR, 32), float("nan"), device=dev), G=G)
    assert g.buffers(32)["ws"].numel() == ops._lib.load().pda_ials_workspace_bytes(g.user.all_rows.n_slots, 32)
    assert torch.equal(S.bits(again), S.bits(base)) and bool(torch.isfinite(base).all())


# PCC: z_ws [B] is written in full by the score pass before the moments pass and the step read it (ops.pcc_workspace hands it over as it comes).
@case("pcc", ["ops.pcc_workspace"], tol=(0.0, 1e-5))
def _(dev, mp):
    S, pr = T("test_gpu_pcc"), T("pcc_ref")
    for on in pr.ONS:
        S.test_gradients_and_loss_against_the_float64_restatement(dev, 32, 7, on)
        S.test_the_statistic_is_the_float64_moments_of_its_own_scores_and_keeps_its_bits(dev, 64, 7, on)
    S.test_three_whole_steps_against_the_restatement(dev, "pos")


@case("lightgcn", ["ops.GcnGraph.buffers", "ops.gcn_spmm"], tol=(1e-5, 1e-5), sizes=["pda_gcn_spmm_workspace_bytes"])
def _(dev, mp):
    S = T("test_gpu_lightgcn")
    S._GRAPHS.clear()                                      # (its graphs keep their workspaces: built under this fill)
    for name in ("small", "hub"):
        S.test_product_against_float64_within_the_bound_and_bit_stable(dev, name, 32)
        S.test_fused_forms_equal_their_unfused_composition(dev, name, 64)
    S.test_the_step_stage_by_stage(dev, 64, 37, True)
    S.test_the_regulariser_skips_ids_outside_the_tables(dev)
    S.test_three_whole_steps_against_the_reference(dev, 32, 2, True)
    S._GRAPHS.clear()


# The evaluation driver and the drop-in model on the toy dataset of tests/test_gpu_end_to_end.py, one block; the device sampler's queues
# (sampler.DeviceSampler: [ahead, B] buffers written in full by one sampler launch per refill; the plans of the queue by pda_triplet_plan).
@case("model_api", ["ops.score_dense", "ops.topk_merge", "sampler.DeviceSampler._next_queue", "sampler.DeviceSampler._refill", "ops.bpr_step_plan"],
      tol=(1e-5, 1e-5))
def _(dev, mp):
    E = T("test_gpu_end_to_end")
    clean_env(mp)
    E.test_testing_and_predict_return_the_scores_the_recommender_ranks_by(dev, _TOY["root"], _TOY["tmp"], "s_condition")
    E.test_device_sampler_queue_is_the_per_step_sampler(dev, _TOY["root"], _TOY["tmp"], True)
    E.test_exact_sgd_through_the_trainer_takes_the_planned_step(dev, _TOY["root"], _TOY["tmp"])
    T("test_gpu_bpr_pc").test_do_recommendation_protocol(dev, _TOY["tmp"])         # the evaluation driver's protocol, block by block


_TOY = {}


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """the toy dataset of tests/test_gpu_end_to_end.py"""
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    _TOY["root"], _TOY["tmp"] = str(root) + "/", tmp_path_factory.mktemp("save")
    return _TOY


# ---------------------------------------------------------------------------------------------------------------------------------------
def run_case(name, dev, monkeypatch, fills=db.FILLS, check_functions=True, return_records=False):
    c = CASES[name]
    records, hit, extra = {}, {}, {}
    for fill in fills:
        with monkeypatch.context() as mp, db.dirty(fill) as d, db.Recorder(fill) as rec, db.reported_sizes() as sizes, \
                torch.random.fork_rng(devices=[dev]):          # (the generators' states are put back behind the case)
            db.fresh_caches()
            torch.manual_seed(20261020)              # (some of the families' checks draw their inputs from torch's generators)
            extra[fill] = c.run(dev, mp) or {}           # (a case may hand back host arrays of its own to be compared: name -> array)
            torch.cuda.synchronize()
            d.check_guards()
            hit[fill] = d.funcs()
            # The C caller's view: what the case handed the library was a guarded buffer of EXACTLY the size the library reported, dirty, and
            # Python cleared nothing in it (test_python_clears_nothing_on_the_library_s_behalf).
            table = db.alloc_sites()
            for fn in c.sizes:
                handed = {a.nbytes for a in d.allocations if db.site_function(a.site, table) == SIZE_SITE[fn]}
                assert sizes.get(fn), "%s: %s was never asked (fill 0x%02X)" % (name, fn, fill)
                assert handed & set(sizes[fn]), "%s: %s allocated no buffer of a size %s reported (%s; it allocated %s)" % (
                    name, SIZE_SITE[fn], fn, sorted(set(sizes[fn]))[:8], sorted(handed)[:8])
        db.fresh_caches()                        # (nothing allocated under a fill outlives it)
        records[fill] = rec.records
        print("%s, fill 0x%02X: %d calls recorded, %d buffers handed out, allocating functions: %s" % (
            name, fill, len(rec.records), len(d.allocations), ", ".join(sorted(hit[fill]))))
    first = fills[0]
    for fill in fills[1:]:
        what = "%s, fill 0x%02X against 0x%02X" % (name, fill, first)
        if c.tol is None:
            db.same_records(records[first], records[fill], what)
        else:
            db.same_records(records[first], records[fill], what, rtol=c.tol[0], atol=c.tol[1], outliers=c.tol[2:] or None)
        assert sorted(extra[first]) == sorted(extra[fill]), what
        for k, a in extra[first].items():
            assert np.array_equal(a, extra[fill][k]), "%s: %s differs with the fill at %d bytes" % (what, k, int((a != extra[fill][k]).sum()))
    if check_functions:
        for fill in fills:
            missing = set(c.functions) - hit[fill]
            assert not missing, "%s never allocated in %s under fill 0x%02X: the case does not run what it names" % (name, sorted(missing), fill)
    return (hit, records) if return_records else hit


@pytest.mark.parametrize("name", list(CASES))
def test_the_call_does_not_depend_on_what_its_buffers_held(dev, monkeypatch, toy, name):
    run_case(name, dev, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Cached workspaces (ops._DEEP_WS, _METRICS_WS, _PLAN_WS) and the cached preps, orders and mask tables: a call at shape B after a call at
# another shape A, in one process, finds A's state in them.  Its result must be B's result after fresh_caches(), bit for bit -- for B smaller
# than A (the buffer is reused, everything behind B's extent is A's) and for B larger (the buffer is replaced; the caches keyed on tensors are not).
def _bits_equal(a, b):
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(db._bits(x), db._bits(y)) for x, y in zip(a, b))


def _after_another_shape(calls):
    """calls: {shape name: callable -> tensors}.  Every ordered pair (A, B): B behind A equals B behind fresh_caches()."""
    fresh = {}
    for name, fn in calls.items():
        db.fresh_caches()
        fresh[name] = fn()
    for a in calls:
        for b in calls:
            if a != b:
                db.fresh_caches()
                calls[a]()
                got = calls[b]()
                torch.cuda.synchronize()
                assert _bits_equal(got, fresh[b]), "%s after %s differs from %s on fresh caches" % (b, a, b)
    db.fresh_caches()


def test_cached_deep_workspace_holds_no_state_of_the_previous_shape(dev, monkeypatch):
    from oracle import c_oracle
    from pda_amd import ops
    S = T("test_gpu_score_topk")
    clean_env(monkeypatch)
    rng = np.random.default_rng(77)
    U, I, pop, hist = S.make_case(rng, 300, 1999, 64)
    Ut, It, pt = (torch.from_numpy(x).to(dev) for x in (U, I, pop))
    h = ops.HistoryCSR(*(torch.from_numpy(x).to(dev) for x in S.csr(hist)), by_user=True)
    shapes = {"173 users, K = 1000": (rng.permutation(300)[:173].astype(np.int32), 1000), "40 users, K = 100": (rng.permutation(300)[:40].astype(np.int32), 100)}

    def call(users, K):
        ut = torch.from_numpy(users).to(dev)
        return lambda: ops.recommend_topk_deep(Ut, It, ut, K, ops.HEAD_POP, pt, h)

    _after_another_shape({name: call(*v) for name, v in shapes.items()})
    assert ops._DEEP_WS == {}
    for users, K in shapes.values():                       # ... and B behind A is the oracle's (the raw head: exact)
        ops.recommend_topk_deep(Ut, It, torch.from_numpy(shapes["173 users, K = 1000"][0]).to(dev), 1000, ops.HEAD_RAW, None, h)
        idx, val = ops.recommend_topk_deep(Ut, It, torch.from_numpy(users).to(dev), K, ops.HEAD_RAW, None, h)
        ridx, rval = c_oracle.score_topk(U, I, users, K, 0, None, *S.csr([hist[u] for u in users]), order=1)
        np.testing.assert_array_equal(val.cpu().numpy(), rval)
        np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    db.fresh_caches()


def test_cached_metrics_workspace_holds_no_state_of_the_previous_shape(dev):
    from pda_amd import ops
    B = T("test_gpu_bpr_step")

    def call(n, Ks, fn):
        args = B.to(dev, *_metrics_rows(n), np.asarray(Ks, np.int32))
        return lambda: fn(*args)

    _after_another_shape({"n = 1000, Ks = (20, 50)": call(1000, (20, 50), ops.metrics_sums_ordered),
                          "n = 257, Ks = (1, 5, 10, 50)": call(257, (1, 5, 10, 50), ops.metrics_sums_ordered),
                          "n = 1, Ks = (50,)": call(1, (50,), ops.metrics_sums_ordered),
                          "deep, n = 257, Ks = (20, 50)": call(257, (20, 50), ops.metrics_sums_deep_ordered)})
    for n, Ks in ((257, (1, 5, 10, 50)), (1000, (20, 50))):          # ... and behind each other they are the oracle's
        _metrics_against_the_oracle(dev, ops.metrics_sums_ordered, n, Ks)
    db.fresh_caches()


def test_cached_large_plan_workspace_holds_no_state_of_the_previous_batch(dev):
    from pda_amd import ops
    P = T("test_gpu_bpr_plan")

    def call(B):
        rng = np.random.default_rng(B)
        users = torch.from_numpy(rng.permutation(60000)[:B].astype(np.int32)).to(dev)
        pos, neg = (torch.from_numpy(rng.integers(0, 500, B).astype(np.int32)).to(dev) for _ in range(2))
        def run():
            # the used bytes of the plan: header, the segments' items and starts, the entries, the flags (the capacity behind them is nobody's)
            hdr, seg_item, seg_start, entries, flags = P.parse_plan(ops.triplet_plan(users, pos, neg)[0], B)
            n_seg = int(hdr[0])
            assert 0 < n_seg <= 2 * B and seg_start[n_seg] == 2 * B
            return tuple(torch.from_numpy(np.array(x, copy=True)) for x in (hdr, seg_item[:n_seg], seg_start[:n_seg + 1], entries[:2 * B], flags[:B]))
        return run

    assert ops.PLAN_LDS_MAX_B < 4097
    _after_another_shape({"B = 20000": call(20000), "B = 4097": call(4097), "B = 8192": call(8192)})
    P.test_triplet_plan_is_the_sorted_segmentation_of_pos_and_neg(dev, 20000)          # ... and the plan behind them is the segmentation
    P.test_triplet_plan_is_the_sorted_segmentation_of_pos_and_neg(dev, 4097)
    db.fresh_caches()


def test_cached_preps_orders_and_mask_tables_hold_no_state_of_the_previous_catalogue(dev, monkeypatch):
    """The prep / order / warm-mask caches are keyed on the tensors: two catalogues and two histories alive at once, each call served from the
    cache of its own -- equal to the same call on fresh caches, for every generation that caches."""
    from pda_amd import ops
    S = T("test_gpu_score_topk")
    for impl in ("v2", "v2ord", "k4ord", "k4huge"):
        score_env(monkeypatch, impl)
        calls = {}
        for nI, nu in ((1999, 173), (700, 40)):
            rng = np.random.default_rng(nI)
            U, I, pop, hist = S.make_case(rng, 300, nI, 64)
            Ut, It, pt = (torch.from_numpy(x).to(dev) for x in (U, I, pop))
            h = ops.HistoryCSR(*(torch.from_numpy(x).to(dev) for x in S.csr(hist)), by_user=True)
            ut = torch.from_numpy(rng.permutation(300)[:nu].astype(np.int32)).to(dev)
            calls["%d items, %d users" % (nI, nu)] = (lambda Ut=Ut, It=It, ut=ut, pt=pt, h=h: ops.score_topk_keys(Ut, It, ut, 50, ops.HEAD_POP, pt, h, 0, 1))
        _after_another_shape(calls)
