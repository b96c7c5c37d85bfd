"""BPR-PC: popularity-compensated re-ranking of a trained BPRMF (Zhu et al., WSDM'21; the reference's MF/BPR_PC.py).

    get_dataset_tot_popularity_for_PC   :1135-1146   train-list entries of each item + 1 (duplicates count)
    PC_model                            :669-737     the re-ranking head, on pda_pc_* (include/pda_hip_pc.h)
    main                                :1235-1412   the driver: restores the best_ckpt.ckpt of a `--train normal` run and prints BPR and
                                                     BPR-PC on the valid and the test set

The reference's script cannot be imported (it imports model classes that do not exist); its method is restated here whole.  The head
and its two quirks (one minimum of r per block of 2 048 evaluation users, the shift that can merge distinct r) are in DESIGN.md, "5b. BPR-PC".

Run:  python -m pda_amd.bpr_pc --dataset douban --train normal --pc_alpha 0.1 --pc_beta 0.1 ...  (after the same `--train normal` run)
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

from . import ops
from .exposure import BiasReport
from .rank_report import refuse_rank_report
from .load_data import load_popularity
from .sampler import host_generator

REFERENCE_BLOCK = 2048   # evaluation users per reference block (MF/BPR_PC.py:929-952): one m per block


def get_dataset_tot_popularity_for_PC(data_=None):
    """MF/BPR_PC.py:1135-1146: float64 [n_items], the number of train-list entries of each item plus one."""
    if data_ is None:
        from . import train_new_api as t
        data_ = t.data
    pop = np.zeros(data_.n_items, dtype=np.float64)
    for item, users in data_.train_item_list.items():
        pop[item] = len(users)
    pop += 1.0
    print("popularity information-- mean:{},max:{},min:{}".format(pop.mean(), pop.max(), pop.min()))
    return pop


class PC_model:
    """MF/BPR_PC.py:669-737 on a DatasetApi_Model of a BPRMF.  The item moments (independent of alpha and beta) are cached per
    (item table, popularity); k_u per evaluation list and history.  Both caches assume the tables no longer change: BPR-PC re-ranks a
    restored checkpoint."""

    def __init__(self, model, topk, alpha, beta) -> None:
        if model.input_type != "without_pop":
            raise NotImplementedError("BPR-PC re-ranks a BPRMF (--train normal)")
        self.model = model
        self.saving = True
        self.alpha = float(alpha)
        self.beta = float(beta)
        self.topk = int(topk)
        self.item_num = model.Recommender.n_items
        self._mom = None
        self._k = {}
        print("pc model:", self.item_num)

    def _tables(self):
        U, I = self.model.Recommender.score_tables()
        if U.dtype != torch.float32:
            raise TypeError("BPR-PC runs on fp32 tables only (bf16 tables are not supported)")
        return U, I

    def _pop(self, pos_pop):
        if pos_pop is None:
            raise ValueError("BPR-PC needs the item popularity (pos_pop)")
        if torch.is_tensor(pos_pop):
            return pos_pop
        return self.model._pop_on_device(pos_pop)

    def moments(self, pop):
        """The item moments for this popularity tensor (ops.pc_item_moments), kept while the same item table and tensor are passed."""
        U, I = self._tables()
        if self._mom is None or self._mom[0] is not I or self._mom[1] is not pop:
            self._mom = (I, pop, ops.pc_item_moments(I, pop))
        return self._mom[2]

    def scale(self, users, pop, hist, cache_on=None):
        """k_u of each user (ops.pc_user_stats).  cache_on: the evaluation list `users` is (kept, with hist and pop, as the cache key)."""
        key = None
        if cache_on is not None:
            key = (id(users), id(hist), id(pop))
            hit = self._k.get(key)
            if hit is not None and hit[0] is users and hit[1] is hist and hit[2] is pop:
                return hit[3]
        U, I = self._tables()
        k = ops.pc_user_stats(U, I, users, pop, self.beta, hist, self.moments(pop))[2]
        if key is not None:
            self._k[key] = (users, hist, pop, k)
        return k

    def _full_catalogue(self, items):
        n = self.item_num
        if items is None:
            return
        it = np.asarray(items).reshape(-1)
        if it.size != n or (it != np.arange(n)).any():
            raise NotImplementedError("BPR-PC ranks the full catalogue only (its norms and mask span n_items; a subset fails in the reference too)")

    def do_recommendation(self, sess, batch_users, items, rec_type, pos_pop=None, sparse_cliked_matrix=None):
        """The reference's protocol: ONE reference block of users per call, the full catalogue, the history as the COO triple
        (index, [1.0] * nnz, shape) of BPR_PC's evaluation.  -> int32 ndarray [len(batch_users), topk]."""
        self._full_catalogue(items)
        if sparse_cliked_matrix is None:
            raise ValueError("BPR-PC needs the clicked matrix (the reference feeds it with every call)")
        index, vals, shape = sparse_cliked_matrix
        if np.asarray(vals).size and not (np.asarray(vals) == 1.0).all():
            raise ValueError("BPR-PC's clicked matrix holds 1.0 per entry (set_clicked_value_type('pc'))")
        users = torch.as_tensor(np.asarray(batch_users, dtype=np.int32), device=self.model.device)
        hist = self.model._mask_on_device(index, int(shape[0]))
        pop = self._pop(pos_pop)
        U, I = self._tables()
        k = self.scale(users, pop, hist)
        idx, _ = ops.recommend_topk_pc(U, I, users, pop, k, self.alpha, self.beta, self.topk, hist, rows_per_min=max(users.numel(), 1))
        return idx.cpu().numpy()

    def recommend_device(self, batch_users, items, rec_type, pos_pop=None, mask=None, K=None, eval_pos=None, eval_users=None):
        """The signature evaluation.eval calls.  Rows eval_pos .. eval_pos + n - 1 of the evaluation list eval_users: the call must cover
        whole reference blocks of 2 048 users (the last one may be short), each with its own m.  Without eval_pos the call is one block."""
        self._full_catalogue(items)
        users = batch_users if torch.is_tensor(batch_users) else torch.as_tensor(np.asarray(batch_users, dtype=np.int32), device=self.model.device)
        n = users.numel()
        hist = mask
        if mask is not None and not isinstance(mask, ops.HistoryCSR):
            index, _vals, shape = mask
            hist = self.model._mask_on_device(index, int(shape[0]))
        pop = self._pop(pos_pop)
        U, I = self._tables()
        if eval_pos is None:
            rpm = max(n, 1)
            k = self.scale(users, pop, hist)
        else:
            total = eval_users.numel()
            if eval_pos % REFERENCE_BLOCK or (n % REFERENCE_BLOCK and eval_pos + n != total):
                raise ValueError("BPR-PC: a call covers whole reference blocks of %d evaluation users (got rows %d .. %d of %d)"
                                 % (REFERENCE_BLOCK, eval_pos, eval_pos + n, total))
            rpm = REFERENCE_BLOCK
            if hist is None or hist.mode == ops.HIST_BY_USER_ID:   # k_u of the whole evaluation list once, then slices of it
                k = self.scale(eval_users, pop, hist, cache_on=True)[eval_pos:eval_pos + n]
            else:
                k = self.scale(users, pop, hist)
        return ops.recommend_topk_pc(U, I, users, pop, k.contiguous(), self.alpha, self.beta, K or self.topk, hist, rows_per_min=rpm)


def pc_eval_block(eval_block: int) -> int:
    """--eval_block rounded down to a multiple of 2 048 (at least 2 048): the PC evaluation covers whole reference blocks per call."""
    return max(REFERENCE_BLOCK, (int(eval_block) // REFERENCE_BLOCK) * REFERENCE_BLOCK)


def checkpoint_dir(args) -> str:
    """The directory `python -m pda_amd.train_new_api --train normal` with the same flags saves best_ckpt.ckpt into (MF/BPR_PC.py:1314-1317)."""
    return args.save_dir + "{}_{}_checkpoint/wd_{}_lr_{}_a_{}_{}_train_{}/".format(args.model, args.dataset, args.wd, args.lr, args.alpha,
                                                                                     args.saveID, args.train)


def main(argv=None):
    from . import train_new_api as t
    t.configure(argv)
    args, data = t.args, t.data
    if t.check_topk_max(args) > ops.TOPK_K_V4:
        raise NotImplementedError("--topk_max %d: BPR-PC ranks at most %d items per user (its sweep keeps K + 8 candidates on chip and there is "
                                  "no PC head on the deep path)" % (args.topk_max, ops.PC_MAX_K))
    refuse_rank_report(args, "bpr_pc")
    bias = BiasReport.from_args(args, data, t.Ks)
    random.seed(2020)
    np.random.seed(2020)
    torch.manual_seed(2021)
    if torch.cuda.device_count() > 1 and str(args.cuda).isdigit() and int(args.cuda) < torch.cuda.device_count():
        torch.cuda.set_device(int(args.cuda))
    device = torch.device("cuda")
    config = {"n_users": data.n_users, "n_items": data.n_items}
    popularity_exp = args.pop_exp
    print("----- popularity_exp : ", popularity_exp)
    test_batch_size = min(1024, args.batch_size)
    load_popularity(args)                                                        # the reference reads it first (:1243)

    regs_pretain = args.regs
    if args.model == "mf" and args.train in ("normal", "dice", "ips", "ssm", "ials", "pcc", "dau", "warp"):    # :1272-1284 (a DICE, IPS or SSM checkpoint ranks by the raw head too)
        args.saveID += "pop_exp-{:.2f}".format(popularity_exp) + {"ips": "ips", "ssm": "ssm", "ials": "ials", "pcc": "pcc", "dau": "dau", "warp": "warp"}.get(args.train, "")
        print("normal MF... ")
        args.regs = args.fregs
    else:
        raise NotImplementedError("Not implement this training method.....")
    popualarity_tot = get_dataset_tot_popularity_for_PC(data)
    args.wd = regs_pretain                                                       # :1300
    path = checkpoint_dir(args) + "best_ckpt.ckpt"
    if not os.path.exists(path):
        raise FileNotFoundError("BPR-PC restores a --train %s checkpoint, and there is none at %s (train with the same flags first)" % (args.train, path))
    model = t.DatasetApi_Model(args, config, test_batch_size, (lambda: host_generator(data, False)), device)
    model.set_sess(None)

    evaluation_model = t.evaluation(data, t.Ks, device, block=pc_eval_block(args.eval_block))
    evaluation_model.set_bias_report(bias)
    if args.valid_set == "test":
        evaluation_model.set_evaluate_obj_pre("test")
        print("valid in test set")
    elif args.valid_set == "valid":
        print("valid in valid set")
        evaluation_model.set_evaluate_obj_pre("valid")
    else:
        print("evaluate type error.")
        sys.exit()
    print("args info:", args)
    print("top K:", t.Ks)

    print("loading prtraining model")
    model.Recommender.load_state_dict(torch.load(path, map_location=device))
    bpr_pc = PC_model(model, 50, args.pc_alpha, args.pc_beta)

    print("do not consider popularity ... ")
    results = {}
    for where, title_bpr, title_pc in (("valid", "BPR result of valuation:", "BPR-PC result of valuation:"),
                                       ("test", "BPR result of testing", "BPR-PC result of testing:")):
        if where == "test":
            evaluation_model.set_evaluate_obj_pre("test")
        print(title_bpr)
        evaluation_model.set_clicked_value_type("inf")
        evaluation_model.set_testing_popularity(None)
        ret = evaluation_model.eval(model, None, rec_type="main_branch")
        t._print_result(ret)
        print(title_pc)
        evaluation_model.set_clicked_value_type("pc")
        evaluation_model.set_testing_popularity(popualarity_tot)
        ret_pc = evaluation_model.eval(bpr_pc, None, rec_type="main_branch")
        t._print_result(ret_pc)
        print("\n")
        results[where] = (ret, ret_pc)
    return results


if __name__ == "__main__":
    main()
