"""Float64 restatement of the ranking metrics (precision, recall, NDCG, hit ratio at a list of cut-offs), written from the reference's
MF/used_metric.py:4-80 and independent of any kernel, and the case table the host and the GPU tests of the metrics walk.

The reference leaves two cases undefined; this file states what the project decided for them, and every statement of the metric in the
repository (the four kernels, oracle/pda_oracle.c:oracle_metrics, oracle/pda_oracle.py:get_performance, pda_amd/used_metric.py:
get_performance) follows it.  (1) K > len(list): the reference's precision is np.mean(r[:K]), the mean over the len(list) entries there
are, and its ndcg_at_k raises on the shape mismatch of r[:K] * tp.  The decision: the cut-off of a row is kk = min(K, len(list)) for
precision (hits / kk, which is the reference's mean), for the DCG sum and for the ideal DCG (the first min(npos, kk) discounts), i.e. the
row is measured as if K were len(list): a list cannot be blamed for positions it does not have, and an ideal list of the same length
reaches NDCG 1.  Recall and hit ratio do not depend on it.  The trainer needs nothing else: it never builds a list shorter than a
cut-off it was asked for on purpose, and with --topk_max below a K the figures stay comparable with those at K = --topk_max.  (2) A row
without targets: the reference returns precision 0, NDCG 0 (its `if not dcg_max`), hit ratio 0 and recall 0/0 = NaN, which would turn
the recall of the whole evaluation into NaN; its trainer never meets the case, because it evaluates the keys of the target dictionary.
The decision: such a row adds zero to all four sums and still counts in the divisor (tot_user), so the result stays finite and a user
nothing can be recommended to counts as a miss.  Everything else is the reference: the hit vector is np.isin(r, target), so an item that
a list carries twice hits twice, a target id listed twice counts twice in npos = len(target), and ids that are no item at all (-1, ids
beyond the catalogue) are entries like any other.

Values are Python floats: precision, recall and hit ratio are one IEEE division of small integers, the two DCG sums are math.fsum of
1 / log2(k + 2)."""
import functools
import math

import numpy as np

NAMES = ("precision", "recall", "ndcg", "hit_ratio")      # the rows of `sums`, in the kernels' order
INT32_MAX = 2 ** 31 - 1
MAX_COLS = 1024

_W = [1.0 / math.log2(k + 2.0) for k in range(MAX_COLS)]   # the discount of column k               used_metric.py:46


@functools.lru_cache(maxsize=None)
def _ideal(n):
    return math.fsum(_W[:n])                               # tp[:min(maxlen, k)].sum()              :47


def row_metrics(r, target, Ks):
    """One list `r` and one target row -> [4][len(Ks)] Python floats in the order of NAMES."""
    npos = len(target)
    out = [[0.0] * len(Ks) for _ in range(4)]
    if npos == 0:                                          # decision (2)
        return out
    tset = set(int(t) for t in target)
    where = [k for k, x in enumerate(r) if int(x) in tset]   # np.isin(r, target)                    :65-67
    for q, K in enumerate(Ks):
        assert K >= 1                                      # :12
        kk = min(int(K), len(r))                           # decision (1)
        hit = [k for k in where if k < kk]
        hits = len(hit)
        out[0][q] = hits / kk                              # np.mean(r[:k])                         :4-18
        out[1][q] = hits / npos                            # np.sum(r[:k]) / all_pos_num            :55-57
        ideal = _ideal(min(npos, kk))
        out[2][q] = math.fsum(_W[k] for k in hit) / ideal if ideal else 0.0   # :39-52
        out[3][q] = min(1.0, float(hits))                  # :60-62
    return out


def matrix_rows(rows, targets, Ks):
    """-> float64 [n_rows, 4, len(Ks)]: row_metrics of every row."""
    return np.array([row_metrics(r, t, Ks) for r, t in zip(rows, targets)], dtype=np.float64).reshape(len(rows), 4, len(Ks))


def fsum_rows(per_row):
    """float64 [n, 4, n_ks] -> float64 [4, n_ks]: the exactly rounded sums over the rows."""
    per_row = np.asarray(per_row, dtype=np.float64)
    return np.array([[math.fsum(per_row[:, m, q].tolist()) for q in range(per_row.shape[2])] for m in range(4)], dtype=np.float64)


def matrix_sums(rows, targets, Ks):
    """-> float64 [4, len(Ks)]: math.fsum of row_metrics over the rows (what the kernels add to `sums`)."""
    return fsum_rows(matrix_rows(rows, targets, Ks))


def csr_of(targets):
    indptr = np.zeros(len(targets) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(t) for t in targets])
    flat = np.array([x for t in targets for x in t], dtype=np.int32)
    return indptr, flat


# ------------------------------------------------------------------------------------------------------------------------------------
# The case table
# ------------------------------------------------------------------------------------------------------------------------------------
SHORT_MAX = 64                                             # the columns pda_metrics / pda_metrics_ordered take
K_COLS_SHORT = (1, 2, 49, 50, 63, 64)                      # both kernel families
K_COLS_DEEP = (65, 100, 1023, 1024)                        # the deep pair only
K_COLS = K_COLS_SHORT + K_COLS_DEEP
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)                # every matrix(k_cols)[:n]
LARGE_K_COLS, LARGE_ROWS = 50, 16385 * 4 + 1               # the ordered sum walks 4 * 257 = 1028 waves: more than 256, the last ragged
PLACES = (0, 63, 64, 255)                                  # where a row is put in a block of 256 rows whose other rows have no targets
BLOCK_ROWS = 256
N_ITEMS = 20000                                            # the catalogue: list entries at or beyond it are no items
N_SAMPLE = 3                                               # random rows per k_cols that are also checked one by one


def ks_lists(k_cols):
    """The two lists of cut-offs of one k_cols: six unsorted ones with a repeat (1 twice, k_cols - 1, k_cols, a K > k_cols and 64: below
    64 columns 64 is that K), and a single one.  (The repeat is the cheap one: the deep kernel walks a row once per cut-off.)"""
    over = 64 if k_cols < 64 else k_cols + 3
    mid = 64 if k_cols > 64 else max(1, k_cols // 2)
    return [k_cols, 1, over, max(1, k_cols - 1), 1, mid], [k_cols]


def _list(k_cols):
    return [7 * j + 3 for j in range(k_cols)]              # distinct items of the catalogue


def _other(n, start=10000):
    return [start + 2 * j for j in range(n)]               # even ids from 10000: in no list (hand-built or random)


def hand_rows(k_cols):
    """-> [(name, list, targets)]: the rows every k_cols has."""
    base = _list(k_cols)
    rows = [("hit_last_column_only", base, [base[-1]] + _other(2)),
            ("hits_in_every_column", base, base[::-1]),
            ("no_hit", base, _other(5))]
    cuts = sorted(set(ks_lists(k_cols)[0]))
    for n in sorted({0, 1, 3 * k_cols} | {K + d for K in (1, k_cols, 64) for d in (-1, 0, 1) if K in cuts and K + d >= 0}):
        inlist = [base[c] for c in dict.fromkeys((0, k_cols // 2, k_cols - 1))][:n]      # hits in the first, a middle and the last column
        rows.append(("npos_%d" % n, base, inlist + _other(n - len(inlist))))
    twice = list(base)
    twice[-1] = twice[0]                                   # (one column: nothing to repeat, the row stays)
    rows.append(("item_twice_in_list", twice, [base[0]] + _other(1)))
    rows.append(("target_id_twice", base, [base[0], base[0]] + _other(1)))
    bad = list(base)
    bad[-1] = -1
    if k_cols > 1:
        bad[-2] = N_ITEMS + 5
    rows.append(("no_item_ids_in_list", bad, [bad[0]] + _other(2) if k_cols > 2 else _other(2)))
    rows.append(("target_int32_max", base, [INT32_MAX, base[min(1, k_cols - 1)]]))
    return rows


def random_rows(k_cols, n, seed, max_targets=10):
    """n random rows: lists of k_cols distinct odd ids out of 4 k_cols + 16 (so hits are frequent), 0 .. max_targets targets drawn with
    repeats from the same ids and from ids no list holds."""
    rng = np.random.default_rng(seed)
    n_ids = 4 * k_cols + 16
    out = []
    for _ in range(n):
        r = (2 * rng.permutation(n_ids)[:k_cols] + 1).tolist()
        t = rng.integers(0, n_ids, int(rng.integers(0, max_targets + 1)))
        t = np.where(rng.random(t.shape[0]) < 0.7, 2 * t + 1, 10000 + 2 * t)
        out.append(("random", r, t.tolist()))
    return out


def _hand_slots(n_hand):
    cand = list(dict.fromkeys([0, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256] + list(range(1, 257, 3))))
    return sorted(cand[:n_hand])


@functools.lru_cache(maxsize=None)
def matrix(k_cols):
    """-> (names, lists, targets) of max(ROW_COUNTS) rows: the hand-built rows at and around the wave and workgroup borders, random rows
    between them.  The matrix of n rows is its first n rows.  The row with 3 k_cols targets is row 256, so only the largest matrix pays
    for it (one thread walks k_cols x targets entries per cut-off)."""
    n = max(ROW_COUNTS)
    hand = hand_rows(k_cols)
    hand.sort(key=lambda x: x[0] == "npos_%d" % (3 * k_cols))          # (stable: that row last)
    slots = _hand_slots(len(hand))
    assert len(slots) == len(hand) and slots[0] == 0 and slots[-1] == n - 1
    rnd = iter(random_rows(k_cols, n - len(hand), seed=1000 + k_cols))
    at = dict(zip(slots, hand))
    rows = [at[i] if i in at else next(rnd) for i in range(n)]
    return [x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows]


@functools.lru_cache(maxsize=None)
def large_matrix():
    """LARGE_ROWS rows of LARGE_K_COLS columns: matrix(LARGE_K_COLS), then random rows with at most 3 targets."""
    names, lists, targets = matrix(LARGE_K_COLS)
    more = random_rows(LARGE_K_COLS, LARGE_ROWS - len(names), seed=77, max_targets=3)
    return names + [x[0] for x in more], lists + [x[1] for x in more], targets + [x[2] for x in more]


@functools.lru_cache(maxsize=None)
def matrix_ref(k_cols, which):
    """float64 [rows, 4, n_ks] of matrix(k_cols) at ks_lists(k_cols)[which]: computed once, read-only."""
    _, lists, targets = matrix(k_cols)
    out = matrix_rows(lists, targets, ks_lists(k_cols)[which])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def large_ref():
    _, lists, targets = large_matrix()
    out = matrix_rows(lists, targets, ks_lists(LARGE_K_COLS)[0])
    out.setflags(write=False)
    return out


def single_rows(k_cols):
    """The indices into matrix(k_cols) of the rows that are also checked one by one: every hand-built row and N_SAMPLE random rows."""
    names = matrix(k_cols)[0]
    hand = [i for i, nm in enumerate(names) if nm != "random"]
    rnd = [i for i, nm in enumerate(names) if nm == "random"]
    return hand + rnd[:: max(1, len(rnd) // N_SAMPLE)][:N_SAMPLE]


def check_table():
    """The table holds what it is meant to hold; raises AssertionError otherwise (both test files call it)."""
    required = ["hit_last_column_only", "hits_in_every_column", "no_hit", "npos_0", "npos_1", "item_twice_in_list", "target_id_twice",
                "no_item_ids_in_list", "target_int32_max"]
    assert set(K_COLS_SHORT) == {1, 2, 49, 50, 63, 64} and set(K_COLS_DEEP) == {65, 100, 1023, 1024}
    assert max(K_COLS_SHORT) == SHORT_MAX == min(K_COLS_DEEP) - 1
    for k_cols in K_COLS:
        names, lists, targets = matrix(k_cols)
        assert len(names) == max(ROW_COUNTS) and all(len(r) == k_cols for r in lists)
        a, b = ks_lists(k_cols)
        assert len(a) == 6 and len(b) == 1 and a != sorted(a) and len(set(a)) < len(a)
        assert {1, max(1, k_cols - 1), k_cols, 64} <= set(a) and max(a) > k_cols
        for nm in required + ["npos_%d" % (3 * k_cols), "npos_%d" % (k_cols - 1), "npos_%d" % k_cols, "npos_%d" % (k_cols + 1)]:
            assert nm in names, (k_cols, nm)
        by = dict(zip(names, zip(lists, targets)))
        assert by["hit_last_column_only"][1][0] == by["hit_last_column_only"][0][-1]
        assert INT32_MAX in by["target_int32_max"][1]
        assert -1 in by["no_item_ids_in_list"][0] and (k_cols == 1 or max(by["no_item_ids_in_list"][0]) >= N_ITEMS)
        assert len(set(by["target_id_twice"][1])) < len(by["target_id_twice"][1])
        assert k_cols == 1 or len(set(by["item_twice_in_list"][0])) < k_cols
        assert sum(nm == "random" for nm in names) >= 200 and any(len(t) == 0 for nm, t in zip(names, targets) if nm == "random")
        for which, ks in enumerate((a, b)):                # rows with and without hits at every cut-off, among the rows checked one by one
            ref = matrix_ref(k_cols, which)[single_rows(k_cols)]
            for q in range(len(ks)):
                assert (ref[:, 3, q] == 1.0).any() and (ref[:, 3, q] == 0.0).any(), (k_cols, ks[q])
                assert (ref[:, 0, q] == 1.0).any(), (k_cols, ks[q])                  # (hits in every column)
    assert LARGE_ROWS == 65541 and (LARGE_ROWS + 63) // 64 > 4 * 256 and LARGE_ROWS % 64 != 0
