"""xQuAD: personalised popularity re-ranking of a trained BPRMF (Abdollahpouri, Burke and Mobasher, FLAIRS 2019), the baseline the
reference leaves as a stub (MF/BPR_PC.py:904 and MF/simple_reproduce.py:854: `def gen_xquad_result(sess, model): pass`).

    head_items     the short head: the most popular items that hold --xq_head_share of the train interactions
    XQuAD_model    candidates from the BPRMF (main_branch, --xq_candidates per user: the short path up to 54, the deep path above),
                   re-ranked by pda_xquad_rerank (include/pda_hip_xquad.h) with the evaluation's own history as the user profile
    aplt           the average percentage of long-tail items in the lists, the figure the xQuAD paper reports
    main           the driver: restores the best_ckpt.ckpt of a `--train normal` run and prints BPR and xQuAD on the valid and the test set

Two item categories (short head, long tail).  The contract, the choices the paper leaves open (min-max normalised relevance, one coverage
factor per category in the smooth variant) and the argument for one wave per user are in DESIGN.md, "5e. xQuAD".

Run:  python -m pda_amd.xquad --dataset douban --train normal --xq_lambda 0.5 --xq_candidates 1000 ...  (after the same `--train normal` run)
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

from . import ops
from .bpr_pc import checkpoint_dir
from .exposure import BiasReport
from .rank_report import refuse_rank_report
from .sampler import host_generator


def train_counts(data_) -> np.ndarray:
    """int64 [n_items]: the train-list entries of each item (duplicates count)."""
    counts = np.zeros(data_.n_items, dtype=np.int64)
    for item, users in data_.train_item_list.items():
        counts[item] = len(users)
    return counts


def head_items(train_counts, share) -> np.ndarray:
    """uint8 [n_items], 1 = short head.  Items ordered by (train count descending, id ascending); the head is the shortest prefix whose counts
    sum to at least share x the total (the product in float64).  Items without a train entry are tail; an empty train set has no head."""
    counts = np.asarray(train_counts, dtype=np.int64).reshape(-1)
    share = float(share)
    if not 0.0 < share < 1.0:
        raise ValueError("the head share must lie strictly inside 0 .. 1, got %r" % (share,))
    if (counts < 0).any():
        raise ValueError("train counts must be >= 0")
    head = np.zeros(counts.shape[0], dtype=np.uint8)
    total = int(counts.sum())
    if total == 0:
        return head
    order = np.lexsort((np.arange(counts.shape[0]), -counts))
    reached = np.cumsum(counts[order]) >= share * total
    n_head = int(np.argmax(reached)) + 1
    head[order[:n_head]] = 1                      # (share < 1: the prefix ends before the items without a train entry)
    return head


def aplt(idx: torch.Tensor, is_head: torch.Tensor, Ks) -> np.ndarray:
    """float64 [len(Ks)]: the share of long-tail items among the first k columns of idx [n, K], averaged over the rows (an empty slot, id < 0,
    is no long-tail item).  Plain torch."""
    return (_tail_counts(idx, is_head, Ks) / torch.as_tensor([float(k) for k in Ks], dtype=torch.float64, device=idx.device)
            / float(max(idx.shape[0], 1))).cpu().numpy()


def _tail_counts(idx, is_head, Ks) -> torch.Tensor:
    """float64 [len(Ks)]: the long-tail items among the first k columns, summed over the rows."""
    valid = idx >= 0
    tail = valid & (is_head[idx.clamp(min=0).long()] == 0)
    return torch.stack([tail[:, :int(k)].sum(dtype=torch.float64) for k in Ks])


class ListTap:
    """Passes recommend_device through to `model` and sums the long-tail counts of the lists it returns: APLT of an evaluation.eval pass."""

    def __init__(self, model, is_head, Ks) -> None:
        self.model, self.is_head, self.Ks = model, is_head, list(Ks)
        self.reset()

    def reset(self):
        self.sums, self.rows = None, 0

    def recommend_device(self, *args, **kwargs):
        idx, val = self.model.recommend_device(*args, **kwargs)
        s = _tail_counts(idx, self.is_head, self.Ks)
        self.sums = s if self.sums is None else self.sums + s
        self.rows += idx.shape[0]
        return idx, val

    def aplt(self) -> np.ndarray:
        if self.sums is None:
            return np.zeros(len(self.Ks))
        return (self.sums.cpu().numpy() / np.asarray(self.Ks, dtype=np.float64)) / float(self.rows)


class XQuAD_model:
    """xQuAD on a DatasetApi_Model of a BPRMF: n_candidates per user by the main_branch head, K of them selected.  is_head: uint8 [n_items]
    (head_items), on the model's device."""

    def __init__(self, model, topk, lam, n_candidates, is_head, variant="smooth") -> None:
        if model.input_type != "without_pop":
            raise NotImplementedError("xQuAD re-ranks a BPRMF (--train normal)")
        self.model = model
        self.item_num = model.Recommender.n_items
        self.topk = int(topk)
        self.lam = float(lam)
        self.n_candidates = int(n_candidates)
        self.variant = variant
        if not 0.0 <= self.lam <= 1.0:
            raise ValueError("xQuAD: lambda must lie in [0, 1], got %r" % (lam,))
        if variant not in ops.XQUAD_VARIANTS:
            raise ValueError("xQuAD: variant must be 'smooth' or 'binary', not %r" % (variant,))
        if not 1 <= self.topk <= min(ops.XQUAD_MAX_K, self.n_candidates) or self.n_candidates > ops.XQUAD_MAX_N:
            raise ValueError("xQuAD selects 1 <= K <= min(%d, candidates) out of at most %d candidates, got K = %d of %d"
                             % (ops.XQUAD_MAX_K, ops.XQUAD_MAX_N, self.topk, self.n_candidates))
        if self.n_candidates > self.item_num:
            raise ValueError("xQuAD: %d candidates exceed the catalogue (%d items)" % (self.n_candidates, self.item_num))
        is_head = torch.as_tensor(is_head, dtype=torch.uint8, device=model.device).contiguous()
        if is_head.numel() != self.item_num:
            raise ValueError("is_head holds one byte per item of the catalogue")
        self.is_head = is_head
        print("xquad model:", self.item_num, "head items:", int(is_head.count_nonzero()))

    def _full_catalogue(self, items):
        n = self.item_num
        if items is None:
            return
        it = np.asarray(items).reshape(-1)
        if it.size != n or (it != np.arange(n)).any():
            raise NotImplementedError("xQuAD re-ranks lists over the full catalogue only (its categories are indexed by the global item id)")

    def candidates(self, users, mask):
        """The BPRMF's n_candidates best unlisted items of each user -> (idx int32 [n, N], val float32 [n, N])."""
        return self.model.recommend_device(users, None, "main_branch", None, mask, K=self.n_candidates)

    def recommend_device(self, batch_users, items, rec_type, pos_pop=None, mask=None, K=None, eval_pos=None, eval_users=None):
        """The signature evaluation.eval calls.  The mask that hides the train items from the candidates is the user's profile."""
        if rec_type != "main_branch":
            raise NotImplementedError("xQuAD re-ranks the main_branch head")
        self._full_catalogue(items)
        users = batch_users if torch.is_tensor(batch_users) else torch.as_tensor(np.asarray(batch_users, dtype=np.int32), device=self.model.device)
        hist = mask
        if mask is not None and not isinstance(mask, ops.HistoryCSR):
            index, _vals, shape = mask
            hist = self.model._mask_on_device(index, int(shape[0]))
        cidx, cval = self.candidates(users, hist)
        return ops.xquad_rerank(cidx, cval, self.is_head, self.lam, K or self.topk, self.variant, users, hist)


def check_flags(args, Ks):
    """The xQuAD flags, checked before anything is built -> the list length K = max(Ks)."""
    K = max(int(k) for k in Ks)
    if not 0.0 <= float(args.xq_lambda) <= 1.0:
        raise ValueError("--xq_lambda must lie in [0, 1], got %r" % (args.xq_lambda,))
    if not 0.0 < float(args.xq_head_share) < 1.0:
        raise ValueError("--xq_head_share must lie strictly inside 0 .. 1, got %r" % (args.xq_head_share,))
    if args.xq_variant not in ops.XQUAD_VARIANTS:
        raise ValueError("--xq_variant must be smooth or binary, not %r" % (args.xq_variant,))
    if K > ops.XQUAD_MAX_K:
        raise ValueError("xQuAD selects at most %d items per user, --Ks asks for %d" % (ops.XQUAD_MAX_K, K))
    if not K <= int(args.xq_candidates) <= ops.XQUAD_MAX_N:
        raise ValueError("--xq_candidates must lie in max(Ks) = %d .. %d, got %d" % (K, ops.XQUAD_MAX_N, args.xq_candidates))
    return K


def main(argv=None):
    from . import train_new_api as t
    t.configure(argv)
    args, data = t.args, t.data
    if not (args.model == "mf" and args.train in ("normal", "dice", "ips", "ssm", "ials", "pcc", "dau", "warp")):
        raise NotImplementedError("Not implement this training method.....")
    K = check_flags(args, t.Ks)
    t.check_topk_max(args)
    refuse_rank_report(args, "xquad")
    bias = BiasReport.from_args(args, data, t.Ks)
    random.seed(2020)
    np.random.seed(2020)
    torch.manual_seed(2021)
    if torch.cuda.device_count() > 1 and str(args.cuda).isdigit() and int(args.cuda) < torch.cuda.device_count():
        torch.cuda.set_device(int(args.cuda))
    device = torch.device("cuda")
    config = {"n_users": data.n_users, "n_items": data.n_items}
    args.saveID += "pop_exp-{:.2f}".format(args.pop_exp) + {"ips": "ips", "ssm": "ssm", "ials": "ials", "pcc": "pcc", "dau": "dau", "warp": "warp"}.get(args.train, "")   # train_new_api.main: the directory name
    args.wd = args.regs
    path = checkpoint_dir(args) + "best_ckpt.ckpt"
    if not os.path.exists(path):
        raise FileNotFoundError("xQuAD restores a --train %s checkpoint, and there is none at %s (train with the same flags first)" % (args.train, path))
    n_candidates = min(int(args.xq_candidates), data.n_items)
    if n_candidates < int(args.xq_candidates):
        print("xquad: the catalogue holds %d items: %d candidates per user" % (data.n_items, n_candidates))
    model = t.DatasetApi_Model(args, config, min(1024, args.batch_size), (lambda: host_generator(data, False)), device)
    model.set_sess(None)

    evaluation_model = t.evaluation(data, t.Ks, device)
    evaluation_model.set_bias_report(bias)
    if args.valid_set not in ("test", "valid"):
        print("evaluate type error.")
        sys.exit()
    print("valid in %s set" % args.valid_set)
    evaluation_model.set_evaluate_obj_pre(args.valid_set)
    print("args info:", args)
    print("top K:", t.Ks)

    print("loading prtraining model")
    model.Recommender.load_state_dict(torch.load(path, map_location=device))
    is_head = head_items(train_counts(data), args.xq_head_share)
    xq = XQuAD_model(model, K, args.xq_lambda, n_candidates, is_head, args.xq_variant)
    taps = (ListTap(model, xq.is_head, t.Ks), ListTap(xq, xq.is_head, t.Ks))

    results = {}
    for where, title_bpr, title_xq in (("valid", "BPR result of valuation:", "xQuAD result of valuation:"),
                                       ("test", "BPR result of testing", "xQuAD result of testing:")):
        if where == "test":
            evaluation_model.set_evaluate_obj_pre("test")
        evaluation_model.set_testing_popularity(None)
        out = {}
        for name, title, tap in (("bpr", title_bpr, taps[0]), ("xquad", title_xq, taps[1])):
            print(title)
            tap.reset()
            out[name] = evaluation_model.eval(tap, None, rec_type="main_branch")
            out["aplt_" + name] = tap.aplt()
            t._print_result(out[name])
            print("||---------------------------------------------- aplt@%s=[%s]" % (list(t.Ks), ", ".join("%.5f" % x for x in out["aplt_" + name])))
        print("\n")
        results[where] = out
    return results


if __name__ == "__main__":
    main()
