"""Calibrated popularity ("CP"): re-ranking of a trained model's lists so that the popularity mix of a user's list follows the popularity mix of
that user's own history (Steck, RecSys 2018: a KL divergence from a smoothed list; Abdollahpouri et al., UMAP 2021: a Jensen-Shannon divergence
over head / mid / tail groups, and the metric UPD), the user-centred baseline beside BPR-PC (pda_amd/bpr_pc.py) and xQuAD (pda_amd/xquad.py).

    cut_groups     the popularity groups: the items from the most popular down, cut at shares of the train interactions (--cp_cuts)
    Calib_model    candidates from the model (main_branch, --cp_candidates per user: the short path up to 54, the deep path above), the
                   profile from the evaluation's own history (pda_calib_profile), re-ranked by pda_calib_rerank (include/pda_hip_calib.h)
    upd            user popularity deviation: the mean Jensen-Shannon divergence between the users' profiles and their lists' group shares
    UpdTap         the integer counts of an evaluation.eval pass (pda_calib_profile, pda_calib_list_counts) that upd is computed from
    main           the driver: restores the best_ckpt.ckpt of a run with the same flags and prints BPR and CP, each with its UPD, on the valid
                   and the test set

The contract, the choices the papers leave open (min-max normalised relevance as in xQuAD, the 2^-20 grid of the divergence, the group cuts)
and the kernel are in DESIGN.md, "5w. Calibrated popularity".

Run:  python -m pda_amd.calib --dataset douban --train normal --cp_lambda 0.5 --cp_candidates 1000 ...  (after the same `--train normal` run)
"""
from __future__ import annotations

import ast
import os
import random
import sys

import numpy as np
import torch

from . import ops
from .bpr_pc import checkpoint_dir
from .exposure import BiasReport, popularity_order
from .rank_report import refuse_rank_report
from .sampler import host_generator
from .xquad import train_counts

MAX_CUTS = ops.CALIB_MAX_G - 1


def parse_cuts(cuts):
    """--cp_cuts, a list literal or a sequence -> a tuple of 1 .. 7 floats, strictly increasing inside (0, 1)."""
    if isinstance(cuts, str):
        try:
            cuts = ast.literal_eval(cuts)
        except (ValueError, SyntaxError):
            raise ValueError("--cp_cuts must be a list literal like [0.2,0.8], got %r" % (cuts,))
    try:
        out = tuple(float(c) for c in cuts)
    except TypeError:
        raise ValueError("--cp_cuts must be a list of numbers, got %r" % (cuts,))
    if not 1 <= len(out) <= MAX_CUTS:
        raise ValueError("--cp_cuts takes 1 .. %d cuts (2 .. %d groups), got %d" % (MAX_CUTS, MAX_CUTS + 1, len(out)))
    if not all(0.0 < c < 1.0 for c in out) or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("--cp_cuts must increase strictly inside 0 .. 1, got %r" % (list(out),))
    return out


def cut_groups(train_counts, cuts) -> np.ndarray:
    """uint8 [n_items]: the popularity group of each item, 0 = the most popular; len(cuts) + 1 groups.  The items are taken in
    exposure.popularity_order (train count descending, id ascending); an item is in group #{c in cuts : cum_before >= c * total}, cum_before
    the train count of the items in front of it and the product in float64.  With one cut c group 0 is exactly xquad.head_items(counts, c).
    Groups may be empty; items without a train entry fall into the last group.  An empty train set is an error."""
    counts = np.asarray(train_counts, dtype=np.int64).reshape(-1)
    cuts = parse_cuts(cuts)
    if (counts < 0).any():
        raise ValueError("train counts must be >= 0")
    total = int(counts.sum())
    if total == 0:
        raise ValueError("a train set without interactions cannot be cut into popularity groups")
    order = popularity_order(counts)
    sorted_counts = counts[order]
    cum_before = np.cumsum(sorted_counts) - sorted_counts
    groups = np.zeros(counts.shape[0], dtype=np.uint8)
    grp = np.zeros(counts.shape[0], dtype=np.int64)
    for c in cuts:
        grp += cum_before >= c * total
    groups[order] = grp.astype(np.uint8)
    return groups


def upd(prof_counts, list_counts):
    """-> (float64 [nK], int64 [nK]): the user popularity deviation at each cut-off and the rows it is the mean over.  prof_counts int [R, G]:
    the users' history entries per group; list_counts int [R, nK, G]: their lists' entries per group at each cut-off.  A row counts at a
    cut-off when its profile and its list are not empty there; its deviation is the Jensen-Shannon divergence (log2: 0 .. 1) between
    prof / sum(prof) and list / sum(list), numpy float64 on the integer counts.  No row: 0."""
    prof = np.asarray(prof_counts, dtype=np.int64)
    cnt = np.asarray(list_counts, dtype=np.int64)
    if prof.ndim != 2 or cnt.ndim != 3 or cnt.shape[0] != prof.shape[0] or cnt.shape[2] != prof.shape[1]:
        raise ValueError("upd takes profile counts [R, G] and list counts [R, nK, G], got %r and %r" % (prof.shape, cnt.shape))
    nK = cnt.shape[1]
    out, rows = np.zeros(nK, dtype=np.float64), np.zeros(nK, dtype=np.int64)
    H = prof.sum(axis=1)
    for j in range(nK):
        T = cnt[:, j, :].sum(axis=1)
        keep = (H > 0) & (T > 0)
        rows[j] = int(keep.sum())
        if not rows[j]:
            continue
        p = prof[keep].astype(np.float64) / H[keep, None].astype(np.float64)
        q = cnt[keep, j, :].astype(np.float64) / T[keep, None].astype(np.float64)
        m = 0.5 * (p + q)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(p > 0, p * np.log2(np.where(p > 0, p / m, 1.0)), 0.0)
            b = np.where(q > 0, q * np.log2(np.where(q > 0, q / m, 1.0)), 0.0)
        out[j] = float((0.5 * (a + b).sum(axis=1)).mean())
    return out, rows


class UpdTap:
    """Passes recommend_device through to `model` and keeps the integer counts UPD needs of every block: the users' profiles from the mask the
    evaluation hands over (pda_calib_profile) and the group counts of the lists returned (pda_calib_list_counts)."""

    def __init__(self, model, base, item_group, G, Ks) -> None:
        self.model, self.base, self.item_group, self.G, self.Ks = model, base, item_group, int(G), list(Ks)
        self.reset()

    def reset(self):
        self.prof, self.cnt = [], []

    def recommend_device(self, batch_users, items, rec_type, pos_pop=None, mask=None, *args, **kwargs):
        idx, val = self.model.recommend_device(batch_users, items, rec_type, pos_pop, mask, *args, **kwargs)
        users, hist = _users_and_history(self.base, batch_users, mask)
        self.prof.append(ops.calib_profile(self.item_group, self.G, idx.shape[0], users, hist).cpu())
        self.cnt.append(ops.calib_list_counts(idx, self.item_group, self.G, self.Ks).cpu())
        return idx, val

    def upd(self):
        if not self.prof:
            return np.zeros(len(self.Ks)), np.zeros(len(self.Ks), dtype=np.int64)
        return upd(torch.cat(self.prof).numpy(), torch.cat(self.cnt).numpy())


def _users_and_history(base, batch_users, mask):
    """The users on the device and the mask as a HistoryCSR (base: the DatasetApi_Model that owns the device and the COO conversion)."""
    users = batch_users if torch.is_tensor(batch_users) else torch.as_tensor(np.asarray(batch_users, dtype=np.int32), device=base.device)
    hist = mask
    if mask is not None and not isinstance(mask, ops.HistoryCSR):
        index, _vals, shape = mask
        hist = base._mask_on_device(index, int(shape[0]))
    return users, hist


class Calib_model:
    """Calibrated popularity on a DatasetApi_Model: n_candidates per user by the main_branch head, K of them selected.  item_group: uint8
    [n_items] (cut_groups) with G groups, on the model's device."""

    def __init__(self, model, topk, lam, n_candidates, item_group, G, div="js", alpha=0.01) -> None:
        if model.input_type != "without_pop":
            raise NotImplementedError("calibrated popularity re-ranks the main_branch head of a model without a popularity input")
        if getattr(model, "_shard", None) is not None:
            raise NotImplementedError("calibrated popularity re-ranks the lists of one GPU (item shards are out of its scope)")
        self.model = model
        self.item_num = model.Recommender.n_items
        self.topk = int(topk)
        self.lam = float(lam)
        self.n_candidates = int(n_candidates)
        self.div, self.alpha, self.G = div, float(alpha), int(G)
        if not 0.0 <= self.lam <= 1.0:
            raise ValueError("calibration: lambda must lie in [0, 1], got %r" % (lam,))
        if div not in ops.CALIB_DIVERGENCES:
            raise ValueError("calibration: the divergence must be 'js' or 'kl', not %r" % (div,))
        if not 0.0 < self.alpha < 1.0:
            raise ValueError("calibration: alpha must lie strictly inside 0 .. 1, got %r" % (alpha,))
        if not 2 <= self.G <= ops.CALIB_MAX_G:
            raise ValueError("calibration takes 2 .. %d popularity groups, got %r" % (ops.CALIB_MAX_G, G))
        if not 1 <= self.topk <= min(ops.CALIB_MAX_K, self.n_candidates) or self.n_candidates > ops.CALIB_MAX_N:
            raise ValueError("calibration selects 1 <= K <= min(%d, candidates) out of at most %d candidates, got K = %d of %d"
                             % (ops.CALIB_MAX_K, ops.CALIB_MAX_N, self.topk, self.n_candidates))
        if self.n_candidates > self.item_num:
            raise ValueError("calibration: %d candidates exceed the catalogue (%d items)" % (self.n_candidates, self.item_num))
        item_group = torch.as_tensor(item_group, dtype=torch.uint8, device=model.device).contiguous()
        if item_group.numel() != self.item_num:
            raise ValueError("item_group holds one byte per item of the catalogue")
        self.item_group = item_group
        print("calib model:", self.item_num, "items per group:", torch.bincount(item_group.long(), minlength=self.G).tolist())

    def _full_catalogue(self, items):
        n = self.item_num
        if items is None:
            return
        it = np.asarray(items).reshape(-1)
        if it.size != n or (it != np.arange(n)).any():
            raise NotImplementedError("calibrated popularity re-ranks lists over the full catalogue only (its groups are indexed by the global item id)")

    def candidates(self, users, mask):
        """The model's n_candidates best unlisted items of each user -> (idx int32 [n, N], val float32 [n, N])."""
        return self.model.recommend_device(users, None, "main_branch", None, mask, K=self.n_candidates)

    def profile(self, users, hist):
        return ops.calib_profile(self.item_group, self.G, users.numel(), users, hist)

    def recommend_device(self, batch_users, items, rec_type, pos_pop=None, mask=None, K=None, eval_pos=None, eval_users=None):
        """The signature evaluation.eval calls.  The mask that hides the train items from the candidates is the user's profile."""
        if rec_type != "main_branch":
            raise NotImplementedError("calibrated popularity re-ranks the main_branch head")
        self._full_catalogue(items)
        users, hist = _users_and_history(self.model, batch_users, mask)
        cidx, cval = self.candidates(users, hist)
        idx, val, _div = ops.calib_rerank(cidx, cval, self.profile(users, hist), self.item_group, self.G, self.lam, K or self.topk, self.div, self.alpha)
        return idx, val


def check_flags(args, Ks):
    """The calibration flags, checked before anything is built -> (the list length K = max(Ks), the cuts)."""
    K = max(int(k) for k in Ks)
    if not 0.0 <= float(args.cp_lambda) <= 1.0:
        raise ValueError("--cp_lambda must lie in [0, 1], got %r" % (args.cp_lambda,))
    cuts = parse_cuts(args.cp_cuts)
    if args.cp_div not in ops.CALIB_DIVERGENCES:
        raise ValueError("--cp_div must be js or kl, not %r" % (args.cp_div,))
    if not 0.0 < float(args.cp_alpha) < 1.0:
        raise ValueError("--cp_alpha must lie strictly inside 0 .. 1, got %r" % (args.cp_alpha,))
    if K > ops.CALIB_MAX_K:
        raise ValueError("calibration selects at most %d items per user, --Ks asks for %d" % (ops.CALIB_MAX_K, K))
    if not K <= int(args.cp_candidates) <= ops.CALIB_MAX_N:
        raise ValueError("--cp_candidates must lie in max(Ks) = %d .. %d, got %d" % (K, ops.CALIB_MAX_N, args.cp_candidates))
    ops.calib_ks(sorted(set(int(k) for k in Ks)), K)
    return K, cuts


def _upd_line(Ks, figures, rows) -> str:
    users = str(int(rows[0])) if len(set(int(r) for r in rows)) == 1 else "[%s]" % ", ".join(str(int(r)) for r in rows)
    return "||---------------------------------------------- upd@%s=[%s] users=%s" % (list(Ks), ", ".join("%.5f" % x for x in figures), users)


def main(argv=None):
    from . import train_new_api as t
    t.configure(argv)
    args, data = t.args, t.data
    if not (args.model == "mf" and args.train in ("normal", "dice", "ips", "ssm", "ials", "pcc", "dau", "warp")):
        raise NotImplementedError("Not implement this training method.....")
    K, cuts = check_flags(args, t.Ks)
    t.check_topk_max(args)
    refuse_rank_report(args, "calib")
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
        raise FileNotFoundError("calibration restores a --train %s checkpoint, and there is none at %s (train with the same flags first)" % (args.train, path))
    n_candidates = min(int(args.cp_candidates), data.n_items)
    if n_candidates < int(args.cp_candidates):
        print("calib: the catalogue holds %d items: %d candidates per user" % (data.n_items, n_candidates))
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
    G = len(cuts) + 1
    cp = Calib_model(model, K, args.cp_lambda, n_candidates, cut_groups(train_counts(data), cuts), G, args.cp_div, args.cp_alpha)
    ks = sorted(set(int(k) for k in t.Ks))
    taps = (UpdTap(model, model, cp.item_group, G, ks), UpdTap(cp, model, cp.item_group, G, ks))

    results = {}
    for where, title_bpr, title_cp in (("valid", "BPR result of valuation:", "CP result of valuation:"),
                                       ("test", "BPR result of testing", "CP result of testing:")):
        if where == "test":
            evaluation_model.set_evaluate_obj_pre("test")
        evaluation_model.set_testing_popularity(None)
        out = {}
        for name, title, tap in (("bpr", title_bpr, taps[0]), ("cp", title_cp, taps[1])):
            print(title)
            tap.reset()
            out[name] = evaluation_model.eval(tap, None, rec_type="main_branch")
            out["upd_" + name], out["upd_users_" + name] = tap.upd()
            t._print_result(out[name])
            print(_upd_line(ks, out["upd_" + name], out["upd_users_" + name]))
        print("\n")
        results[where] = out
    return results


if __name__ == "__main__":
    main()
