"""python -m pda_amd.export_topk <flags of the training run> --topk_max N --export_out FILE.npz

Restores the best_ckpt.ckpt of a `--train normal`, `--train dice`, `--train ips`, `--train ssm`, `--train pcc`, `--train dau` or `--train s_condition` run of pda_amd.train_new_api (same flags, as pda_amd.bpr_pc does)
and writes the ranked list of every evaluation user of --valid_set, N items deep (1 .. 1 024; above 54 through the deep path,
include/pda_hip_deep.h):

    users  int32   [n]       evaluation users, file order
    idx    int32   [n, N]    item ids, best first (train items masked)
    val    float32 [n, N]    the values they were ranked by

`normal`, `dice`, `ips`, `pcc`, `dau` and `ssm` rank by the main_branch head (`ssm` with --ssm_norm 1 and `dau` with --dau_rank cosine: on the row-normalised tables); `s_condition` by the condition head with the last-stage popularity (PDA).  For candidate generation
ahead of a re-ranker, and for offline analysis of popularity bias.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

from .bpr_pc import checkpoint_dir
from .exposure import BiasReport
from .rank_report import refuse_rank_report
from .load_data import get_popularity_from_load, load_popularity
from .sampler import host_generator


def restore(argv=None):
    """-> (args, model, evaluation_model, rec_type, popularity): the restored model of the run these flags describe, and how it ranks."""
    from . import train_new_api as t
    t.configure(argv)
    args, data = t.args, t.data
    t.check_topk_max(args)
    refuse_rank_report(args, "export_topk")
    random.seed(2020)
    np.random.seed(2020)
    torch.manual_seed(2021)
    if args.model != "mf" or args.train not in ("normal", "s_condition", "dice", "ips", "ssm", "ials", "pcc", "dau", "warp"):
        raise NotImplementedError("export_topk restores a --train normal, --train dice, --train ips, --train ssm, --train ials, --train pcc, --train dau, --train warp or --train s_condition run, not %r" % (args.train,))
    if torch.cuda.device_count() > 1 and str(args.cuda).isdigit() and int(args.cuda) < torch.cuda.device_count():
        torch.cuda.set_device(int(args.cuda))
    device = torch.device("cuda")
    config = {"n_users": data.n_users, "n_items": data.n_items}
    pop_item_all = load_popularity(args)
    with_pop = args.train == "s_condition"
    if with_pop:                                       # train_new_api.main: the directory name and the sampler's popularity
        args.saveID += "pop_exp-{:.2f} (gamma)".format(args.pop_exp)
        data.add_expo_popularity(np.power(get_popularity_from_load(pop_item_all), args.pop_exp))
        rec_type, popularity = "condition", np.power(pop_item_all[:, -2], args.pop_exp)
    else:
        args.saveID += "pop_exp-{:.2f}".format(args.pop_exp) + {"ips": "ips", "ssm": "ssm", "ials": "ials", "pcc": "pcc", "dau": "dau", "warp": "warp"}.get(args.train, "")
        rec_type, popularity = "main_branch", None
    args.wd = args.regs
    path = checkpoint_dir(args) + "best_ckpt.ckpt"
    if not os.path.exists(path):
        raise FileNotFoundError("export_topk restores a checkpoint of pda_amd.train_new_api, and there is none at %s (train with the same flags first)"
                                % path)
    model = t.DatasetApi_Model(args, config, min(1024, args.batch_size), (lambda: host_generator(data, with_pop)), device)
    model.set_sess(None)
    model.Recommender.load_state_dict(torch.load(path, map_location=device))
    evaluation_model = t.evaluation(data, t.Ks, device)
    if args.valid_set not in ("test", "valid"):
        print("evaluate type error.")
        sys.exit()
    evaluation_model.set_evaluate_obj_pre(args.valid_set)
    evaluation_model.set_testing_popularity(popularity)
    return args, model, evaluation_model, rec_type, popularity


def main(argv=None):
    args, model, ev, rec_type, popularity = restore(argv)
    if not args.export_out:
        raise ValueError("export_topk needs --export_out FILE.npz")
    pop = None if popularity is None else ev._pop_dev
    idx_parts, val_parts = [], []
    from . import train_new_api as t
    bias = BiasReport.from_args(args, t.data, t.Ks)            # --bias_report 1: the report of the lists written, without targets (no hit columns)
    acc = None if bias is None else bias.accumulator(ev.device, with_hits=False)
    for i in range(0, ev.tot_user, ev.batch_size):
        ub = ev.users_dev[i:i + ev.batch_size]
        idx, val = model.recommend_device(ub, None, rec_type, pop, ev._hist, eval_pos=i, eval_users=ev.users_dev)
        if acc is not None:
            acc.add(idx)
        idx_parts.append(idx.cpu().numpy())
        val_parts.append(val.cpu().numpy())
    out = {"users": ev.users_dev.cpu().numpy().astype(np.int32), "idx": np.concatenate(idx_parts), "val": np.concatenate(val_parts)}
    d = os.path.dirname(os.path.abspath(args.export_out))
    os.makedirs(d, exist_ok=True)
    with open(args.export_out, "wb") as f:            # (a file object: np.savez would append .npz to a name without it)
        np.savez(f, **out)
    print("export_topk: %d users x %d items (%s) -> %s" % (out["idx"].shape[0], out["idx"].shape[1], rec_type, args.export_out))
    if acc is not None:
        for line in bias.header() + bias.report(acc).lines():
            print(line)
    return out


if __name__ == "__main__":
    main()
