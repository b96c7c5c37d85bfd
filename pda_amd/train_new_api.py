"""Trainer / scorer with the reference's interface (MF/train_new_api.py), running the hot path on MI355X.

    DatasetApi_Model   :538-696   wrapper that owns the model + the recommendation heads
    evaluation         :700-828   full-catalogue evaluation driver
    early_stop         :911-927
    main               :930-1338  epoch loop, evaluation cadence, checkpoints, log lines

What changed underneath: `do_recommendation` is ONE fused kernel (score + (elu+1)*pop + history mask + top-K,
pda_score_topk_f32) instead of MatMul[Bu,I] + ~8 passes + TopKV2; `evaluation.eval` scores all evaluation
users in blocks of --eval_block and reduces the metrics on the device (pda_metrics) instead of a
multiprocessing.Pool(5); a training step is the fused pda_bpr_step_f32 (+ Adam sweeps).  `sess` arguments are
accepted everywhere and may be None; `Session.run` understands the reference's fetch lists.

Run:  python -m pda_amd.train_new_api --dataset douban --train s_condition --test s_condition ... (README.md:69)
"""
from __future__ import annotations

import logging
import os
import random
import sys
from time import time

import zlib

import numpy as np
import torch

from . import ops
from .exposure import BiasReport, EvalResult
from .rank_report import RankReport
from .load_data import Data, Data2, get_popularity_from_load, load_popularity
from .model_api import (BPRMF, DAUMF, DICE, IALSMF, IPSBPRMF, MACRBPRMF, PCCBPRMF, SSMBPRMF, WARPBPRMF, BPRMFTempPop, ConditionalBPRMF, ConditionalLightGCN, Fetch, LightGCN, check_dau, check_dice,
                        check_dns, check_ials, check_ips, check_lightgcn, check_macr, check_negpop, check_pcc, check_ssm, check_warp, gcn_train_pairs, ips_item_counts, macr_c_grid)
from .parse import parse_args
from .used_metric import check_ks
from .sampler import DeviceSampler, HostDiceSampler, host_generator, host_generator_with_temp, to_device_batch

# module-level singletons of the reference (MF/batch_test.py:6-19), filled by configure()/main()
args = None
data = None
Ks = [20]
ITEM_NUM = 0
USER_NUM = 0


class OutOfRangeError(Exception):
    """End of the epoch's batch stream (tf.errors.OutOfRangeError, MF/train_new_api.py:1097)."""


class Session:
    """Minimal `tf.Session` stand-in: run([opt, loss, mf_loss, reg_loss]) performs one training step on the next
    batch of the wrapper's iterator and returns [None, loss, mf_loss, reg_loss] as python floats (one D->H sync
    per step, like the reference).  `run_async` does the same without the sync and returns the device tensor."""

    def __init__(self, model=None):
        self.model = model

    def _step(self, fetches):
        owners = {f.owner for f in fetches if isinstance(f, Fetch)}
        if len(owners) != 1:
            raise NotImplementedError("Session.run understands the trainer's fetch lists only")
        rec = owners.pop()
        if not any(f.name == "opt" for f in fetches):
            raise NotImplementedError("fetching %s without the optimiser op" % [f.name for f in fetches])
        b = self.model.next_batch()
        self._rec = rec
        return rec.train_step(*b, plan=self.model.batch_plan)

    def run_async(self, fetches):
        return self._step(fetches)

    def run(self, fetches, feed_dict=None):
        if isinstance(fetches, str) and fetches in ("training_op", "global_variables_initializer"):
            return None
        if isinstance(fetches, Fetch):
            fetches = [fetches]
        loss = self._step(fetches)
        loss = (self._rec.trainer_terms(loss) if hasattr(self._rec, "trainer_terms") else loss).tolist()      # (MACR: a row of five terms)
        pick = {"opt": None, "loss": loss[0], "mf_loss": loss[1], "reg_loss": loss[2]}
        return [pick[f.name] for f in fetches]


def reference_block_first(eval_pos: int, n: int, device=None, block: int = 2048) -> torch.Tensor:
    """Evaluation-list positions eval_pos .. eval_pos + n - 1 -> the position of the first user of the reference's evaluation block of
    `block` users each of them falls into (int64).  BPRMF(t)-pop's alpha comes from that user (quirk 2)."""
    posn = torch.arange(eval_pos, eval_pos + n, device=device, dtype=torch.int64)
    return torch.div(posn, block, rounding_mode="floor") * block


def check_topk_max(args, topk_shard=None) -> int:
    """--topk_max (an extension; 50 = the reference's graph constant): the columns of every ranking.  Above ops.TOPK_K_V4 the lists come from
    the deep path (ops.recommend_topk_deep; across item shards ops.deep_shard_keys + ops.deep_merge, for a shard object whose `deep_lists`
    is true), which has the raw and the popularity head: everything else is refused here."""
    k = getattr(args, "topk_max", None)
    k = 50 if k is None else int(k)
    if not 1 <= k <= ops.DEEP_MAX_K:
        raise ValueError("--topk_max must lie in 1 .. %d, got %d" % (ops.DEEP_MAX_K, k))
    if k > ops.TOPK_K_V4:
        if getattr(args, "train", "normal") == "temp_pop":
            raise NotImplementedError("--topk_max %d: lists deeper than %d have no bias head (--train temp_pop ranks by s + alpha beta; the deep path "
                                      "ranks by the raw and the popularity head only)" % (k, ops.TOPK_K_V4))
        if topk_shard is not None and getattr(topk_shard, "deep_lists", False) is not True:
            raise NotImplementedError("--topk_max %d: lists deeper than %d are merged across item shards by pda_amd.dist.ItemShardedTopK only "
                                      "(pda_topk_merge takes at most %d columns; this shard object has no deep_lists): evaluate on one GPU"
                                      % (k, ops.TOPK_K_V4, ops._lib.MAX_K))
    return k


class DatasetApi_Model:
    def __init__(self, args, data_config, test_batch, generator_sampler, device=None, topk_shard=None):
        topk_max = check_topk_max(args, topk_shard)
        self.args = args
        self.device = torch.device(device if device is not None else "cuda")
        self.generator_sampler = generator_sampler
        self._iter = None
        self.batch_plan = None        # pda_triplet_plan of the batch next_batch() returned last (--optimizer sgd, device sampler)
        wants_plan = getattr(args, "optimizer", "adam") == "sgd" or bool(int(getattr(args, "deterministic", 0) or 0))
        if wants_plan and getattr(generator_sampler, "distinct_users", False) and hasattr(generator_sampler, "with_plan"):
            # the exact SGD step without atomics wants the batch's plan (ops.bpr_step_plan), and so does every planned step of --deterministic 1
            generator_sampler.with_plan = True
        self.sess = None
        self.testing_model_type, self.testing_popularity = "o", None
        if getattr(args, "model", "mf") == "lightgcn":
            # the LightGCN backbone: the same two heads on the final tables of the propagated ego tables
            check_lightgcn(args)
            if topk_shard is not None:
                raise NotImplementedError("--model lightgcn with item shards: no item-parallel training or evaluation (the graph is not sharded)")
            self.input_type = "with_pop" if args.train == "s_condition" else "without_pop"
            print("dataset api with pop or temp" if args.train == "s_condition" else "dataset api without pop")
            cls = ConditionalLightGCN if args.train == "s_condition" else LightGCN
            self.Recommender = cls(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train in ("s_condition", "condition"):
            self.input_type = "with_pop"                                     # :547-549
            print("dataset api with pop or temp")
            self.Recommender = ConditionalBPRMF(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "temp_pop":
            self.input_type = "with_temp"                                    # :547-551, :570-575
            print("dataset api with pop or temp")
            self.Recommender = BPRMFTempPop(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "normal":
            self.input_type = "without_pop"                                  # :558-559
            print("dataset api without pop")
            self.Recommender = BPRMF(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "dice":
            # DICE: two embeddings per row, ranked by the raw head like a BPRMF; batches carry the sampler's mask
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = DICE(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "ips":
            # IPS / IPS-C / IPS-CN: a BPRMF whose step weighs every triplet by the inverse propensity of its positive
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = IPSBPRMF(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "pcc":
            # PCC: a BPRMF whose loss adds gamma r^2, r the batch's correlation of a score with the positive's popularity
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = PCCBPRMF(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "dau":
            # DirectAU: a BPRMF under the alignment + uniformity loss; no negatives, the lists read score_tables()
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = DAUMF(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "warp":
            # WARP: a BPRMF under the rank-weighted hinge on the first violating candidate; batches carry the sampler's coefficient
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = WARPBPRMF(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "ssm":
            # SSM: a BPRMF under the sampled-softmax loss; batches carry a [B, N] block of negatives, the lists read score_tables()
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = SSMBPRMF(args, data_config, use_dataset_api=True, device=self.device)
            #  the train mask and the logQ table come from the sampler's graph; a model that only ranks (export_topk) has no sampler
            if self.Recommender.ssm_source in ("batch", "all") and hasattr(generator_sampler, "indptr"):
                self.Recommender.set_train_graph(generator_sampler.indptr, generator_sampler.indices, generator_sampler.pool)
            #  the logQ table of a popularity proposal comes from the sampler's table
            if self.Recommender.wants_neg_logq() and getattr(generator_sampler, "neg_table", None) is not None:
                self.Recommender.set_neg_logq(torch.from_numpy(generator_sampler.neg_table.logq).to(self.device))
        elif args.train == "ials":
            # iALS: the tables of a BPRMF solved row by row; no batches, the trainer calls train_epoch()
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = IALSMF(args, data_config, use_dataset_api=True, device=self.device)
        elif args.train == "macr":
            # MACR: the tables of a BPRMF plus two branch vectors; lists ranked by (y - c) s_i through the bias head
            self.input_type = "without_pop"
            print("dataset api without pop")
            self.Recommender = MACRBPRMF(args, data_config, use_dataset_api=True, device=self.device)
        else:
            raise NotImplementedError("not implement this model: " + args.train)   # :590
        # the device sampler draws a batch's users without replacement (like the reference, :380-381): the fused SGD step may
        # then store its user rows plainly (PDA_UPD_USERS_DISTINCT)
        self.Recommender.users_distinct = bool(getattr(generator_sampler, "distinct_users", False))
        if getattr(generator_sampler, "mode", None) == "warp":
            #  the WARP sampler scores its candidates on the live tables, as the DNS sampler below does
            rec = self.Recommender
            generator_sampler.set_tables(lambda: (rec.weights["user_embedding"], rec.weights["item_embedding"]))
        if getattr(generator_sampler, "mode", None) == "dns":
            #  the DNS sampler scores its candidates on the live tables: the reverse of the set_train_graph hand-over above.  A
            # deferred Adam would leave idle rows stale under the sampler, so the dense sweep is the update whatever the size of the tables
            check_dns(args)
            rec = self.Recommender
            rec.adam_exact_lazy = False
            generator_sampler.set_tables(lambda: (rec.weights["user_embedding"], rec.weights["item_embedding"]))
        self.n_items = data_config["n_items"]
        self._shard = topk_shard            # optional pda_amd.dist.ItemShardedTopK (multi-GPU evaluation)
        self.Create_Recommendation(topk_max)

    def Create_Recommendation(self, topk_max=50):
        self.topk_max = topk_max            # "top-K hard-capped at 50" (:594); --topk_max

    # ---- training side ------------------------------------------------------------------------------
    def switch_to_training_or_reinitsampler(self, sess=None):
        """(Re)start the epoch's generator -- `sess.run(self.training_op)` in the reference (:671-672)."""
        self._iter = iter(self.generator_sampler())

    def next_batch(self):
        if self._iter is None:
            raise OutOfRangeError()
        try:
            b = next(self._iter)
        except StopIteration:
            self._iter = None
            raise OutOfRangeError() from None
        if not torch.is_tensor(b[0]):
            b = to_device_batch(b, self.device)
        self.batch_plan = getattr(self.generator_sampler, "plan", None)
        return b

    # ---- scoring side ---------------------------------------------------------------------------------
    def _tables(self, items):
        I = self.Recommender.score_tables()[1]
        if items is None or (len(items) == I.shape[0] and (len(items) == 0 or (items[0] == 0 and items[-1] == I.shape[0] - 1))):
            return I, None
        sel = torch.as_tensor(np.asarray(items, dtype=np.int64), device=self.device)
        return I.index_select(0, sel).contiguous(), sel

    def _pop_on_device(self, pos_pop):
        """The reference hands every block a FRESH ndarray (`testing_popularity[batch_item]`, MF/train_new_api.py:788) with the same
        contents: the device copy is kept while the contents stay equal, because everything ops caches per popularity vector (the
        >= 0 check, the visiting order, the item image) is keyed on the tensor object."""
        arr = np.ascontiguousarray(np.asarray(pos_pop, dtype=np.float32).reshape(-1))
        hit = getattr(self, "_pop_cache", None)
        # (bit patterns: NaN-safe, and 20 x cheaper than array_equal(equal_nan=True) -- 0.9 ms per 200 000 items, more than the block's sweep)
        if hit is not None and hit[0].shape == arr.shape and np.array_equal(hit[0].view(np.uint32), arr.view(np.uint32)):
            return hit[1]
        t = torch.as_tensor(arr, device=self.device)
        self._pop_cache = (arr.copy(), t)
        return t

    def _mask_on_device(self, index, n_rows):
        """The reference builds a block's mask triple ONCE (`set_evaluate_obj_pre`, MF/train_new_api.py:730-739) and hands the same
        ndarray over in every evaluation epoch (:791): its CSR stays on the device, keyed on the array object and guarded by its
        shape and a checksum of its bytes (a caller that refills the array in place gets a fresh conversion).  Block-row CSRs are small
        (~0.4 MB per 2 048-user block of config 3); the cache holds the blocks of one pass."""
        cache = self.__dict__.setdefault("_mask_cache", {})
        arr = index if isinstance(index, np.ndarray) else None
        probe = None
        if arr is not None and arr.ndim == 2 and arr.shape[0] > 0:
            # the guard covers the WHOLE array (an in-place refill of any row gives a fresh conversion): one pass over ~1.6 MB per 2 048-user
            # block of config 3, a few per cent of the host -> device copy it saves
            probe = (arr.shape, n_rows, str(arr.dtype), zlib.adler32(np.ascontiguousarray(arr).view(np.uint8)))
            hit = cache.get(id(arr))
            if hit is not None and hit[0]() is arr and hit[1] == probe:
                return hit[2]
        hist = ops.HistoryCSR.from_coo(index, n_rows, self.device)
        if probe is not None:
            import weakref
            key = id(arr)
            try:
                # (an entry dies with its array: a caller that builds fresh arrays per call pins nothing)
                cache[key] = (weakref.ref(arr, lambda _r, k=key, c=cache: c.pop(k, None)), probe, hist)
            except TypeError:                                   # (an ndarray subclass without weak references)
                pass
        return hist

    def do_recommendation(self, sess, batch_users, items, rec_type, pos_pop=None, sparse_cliked_matrix=None):
        """-> int32 ndarray [len(batch_users), 50] of positions inside `items` (:614-640)."""
        idx, _ = self.recommend_device(batch_users, items, rec_type, pos_pop, sparse_cliked_matrix)
        return idx.cpu().numpy()

    # the reference scores its evaluation users in blocks of this many (MF/train_new_api.py:703); BPRMF(t)-pop's alpha depends on it (quirk 2)
    REFERENCE_EVAL_BLOCK = 2048

    def temp_pop_alpha(self, users, eval_pos=None, eval_users=None):
        """alpha of BPRMF(t)-pop's bias head for a block of users (quirk 2): do_recommendation feeds temp = raw = [[0]], so every
        user of a reference block of 2 048 evaluation users gets 1 + bu of that block's FIRST user.  eval_pos: the position of users[0] in the
        evaluation list eval_users -- any block size then gives the reference's alpha; without it the block itself is one reference block."""
        n = users.numel()
        if eval_pos is None:
            first = users[:1].expand(n)
        else:
            first = eval_users.index_select(0, reference_block_first(eval_pos, n, users.device))
        return self.Recommender.user_alpha(first)

    def recommend_device(self, batch_users, items, rec_type, pos_pop=None, mask=None, K=None, eval_pos=None, eval_users=None):
        if self.input_type == "with_temp":
            if rec_type != "main_branch":
                raise NotImplementedError("temp_pop evaluates the main_branch head only (--test temp_pop)")
        elif rec_type == "macr":
            if not isinstance(self.Recommender, MACRBPRMF):
                raise NotImplementedError("the macr head needs a MACR model (--train macr)")
            head, pos_pop = None, None
        elif rec_type == "main_branch":
            head, pos_pop = ops.HEAD_RAW, None
        elif rec_type in ("main_with_pop", "condition"):
            if rec_type == "condition" and self.input_type != "with_pop":
                raise NotImplementedError("condition head needs a PD/PDA model")
            head = ops.HEAD_POP
            if pos_pop is None:
                raise ValueError("rec_type %s needs pos_pop" % rec_type)
        else:
            raise NotImplementedError("we have only implement recommendation method: main main+pop condition macr")   # :639
        users = batch_users if torch.is_tensor(batch_users) else torch.as_tensor(np.asarray(batch_users, dtype=np.int32), device=self.device)
        hist = mask
        if mask is not None and not isinstance(mask, ops.HistoryCSR):
            index, _vals, shape = mask                         # the reference's (index, [-inf]*nnz, shape) triple (:791)
            hist = self._mask_on_device(index, int(shape[0]))
        pop_t = None
        if pos_pop is not None:
            pop_t = pos_pop if torch.is_tensor(pos_pop) else self._pop_on_device(pos_pop)
        K = K or self.topk_max
        I, _sel = self._tables(items)
        if self.input_type == "with_temp":
            beta = self.Recommender.item_beta()
            if _sel is not None:
                beta = beta.index_select(0, _sel).contiguous()
            alpha = self.temp_pop_alpha(users, eval_pos, eval_users)
            return ops.recommend_topk_bias(self.Recommender.score_tables()[0], I, users, alpha, beta, K, hist)
        if rec_type == "macr":
            # (y - c) s_i = u . (s_i I_i) - c s_i: the bias head on the model's item prep (built once per evaluation), alpha = 1, beta = -c s_i
            rec = self.Recommender
            ops.check_macr_lists(rec.emb_dim, K)
            prep = rec.item_prep()
            if _sel is None:
                return ops.recommend_topk_macr(rec.score_tables()[0], I, rec.weights["w_item"], users, rec.c, K, hist, prep=prep)
            ones = torch.ones(users.numel(), dtype=torch.float32, device=self.device)
            return ops.recommend_topk_bias(rec.score_tables()[0], prep.J.index_select(0, _sel).contiguous(), users, ones,
                                           prep.bias(rec.c).index_select(0, _sel).contiguous(), K, hist)
        if self._shard is not None and _sel is None:
            self._shard.set_popularity(pop_t)
            return self._shard.topk(users, K, head, hist)
        if K > ops.TOPK_K_V4:               # deep lists (--topk_max): the exact sweep with its lists in the workspace
            return ops.recommend_topk_deep(self.Recommender.score_tables()[0], I, users, K, head, pop_t, hist)
        return ops.recommend_topk(self.Recommender.score_tables()[0], I, users, K, head, pop_t, hist)

    def rank_device(self, batch_users, rec_type, tgt_indptr, tgt_indices, pos_pop=None, mask=None):
        """--rank_report 1: the exact 0-based position of every target entry (a CSR by block row) in its user's masked full-catalogue ranking
        under the head recommend_device ranks by for this rec_type, and the length of every ranking -> (rank int32 [n_entries], -1 = does
        not rank; n_ranked int32 [B]).  Reads score_tables(), like the lists (SSM-normalised and LightGCN tables included)."""
        if self.input_type == "with_temp" or rec_type == "macr":
            raise NotImplementedError("ranks are taken by the raw and the popularity head (no temp_pop or macr head: --rank_report 0)")
        if self._shard is not None:
            raise NotImplementedError("ranks are counted on one GPU (item shards are not wired up)")
        if rec_type == "main_branch":
            head, pos_pop = ops.HEAD_RAW, None
        elif rec_type in ("main_with_pop", "condition"):
            if rec_type == "condition" and self.input_type != "with_pop":
                raise NotImplementedError("condition head needs a PD/PDA model")
            head = ops.HEAD_POP
            if pos_pop is None:
                raise ValueError("rec_type %s needs pos_pop" % rec_type)
        else:
            raise NotImplementedError("ranks exist for the rec_types main_branch, main_with_pop and condition")
        users = batch_users if torch.is_tensor(batch_users) else torch.as_tensor(np.asarray(batch_users, dtype=np.int32), device=self.device)
        pop_t = None
        if pos_pop is not None:
            pop_t = pos_pop if torch.is_tensor(pos_pop) else self._pop_on_device(pos_pop)
        U, I = self.Recommender.score_tables()
        return ops.rank_targets(U, I, users, tgt_indptr, tgt_indices, head, pop_t, mask)

    def testing(self, sess, batch_users, items, model_type, pos_pop=None):
        """Dense scores f32 [B, len(items)] (:642-669): batch_ratings / condition_ratings as the NeuRec evaluators' protocol fetches them (the
        reference imports that protocol and never calls it).  pda_score_dense_f32: every entry is the exact fmaf chain of the top-K kernels, so
        these scores equal the values do_recommendation ranks by, bit for bit (bf16 tables: widened first, as their scores are defined)."""
        if model_type not in ("main_branch", "condition", "macr"):
            raise NotImplementedError("error -- not implement this type testing method...")      # :664
        U, I = self.Recommender.score_tables()
        users = torch.as_tensor(np.asarray(batch_users, dtype=np.int32), device=self.device)
        it = np.asarray(items, dtype=np.int64).reshape(-1)
        whole = it.size == I.shape[0] and bool((it == np.arange(it.size)).all())
        it_t = None if whole else torch.as_tensor(it.astype(np.int32), device=self.device)
        if U.dtype != torch.float32:
            U, I = U.float(), I.float()
        if model_type == "macr":
            # rubi_ratings_both (:628) of a MACR model: (y - c) s_i s_u, y the exact chain, the rest element-wise torch (not a hot path)
            rec = self.Recommender
            if not isinstance(rec, MACRBPRMF):
                raise NotImplementedError("the macr ratings need a MACR model (--train macr)")
            y = ops.score_dense(U, I, users, ops.HEAD_RAW, None, it_t)
            Isel = I if it_t is None else I.index_select(0, it_t.long())
            s_i = torch.sigmoid(Isel @ rec.weights["w_item"]).view(1, -1)
            s_u = torch.sigmoid(U.index_select(0, users.long()) @ rec.weights["w_user"]).view(-1, 1)
            return ((y - rec.c) * s_i * s_u).cpu().numpy()
        pop = None
        if model_type == "condition":
            pop = torch.as_tensor(np.asarray(pos_pop, dtype=np.float32).reshape(-1), device=self.device)
        if self.input_type == "with_temp":
            if model_type != "main_branch":
                raise NotImplementedError("temp_pop has the main_branch ratings only")
            # batch_ratings of BPRMFTempPop (:380-396) for a batch fed like do_recommendation feeds it (temp = raw = [[0]]): the first user's
            # alpha for every row.  The reference's own testing() feeds no temp / raw and cannot run this model.
            beta = self.Recommender.item_beta()
            if it_t is not None:
                beta = beta.index_select(0, it_t.long())
            alpha = self.temp_pop_alpha(users)
            s = ops.score_dense(U, I, users, ops.HEAD_RAW, None, it_t)
            return (s + alpha[:, None] * beta[None, :]).cpu().numpy()
        return ops.score_dense(U, I, users, ops.HEAD_POP if model_type == "condition" else ops.HEAD_RAW, pop, it_t).cpu().numpy()

    def switch_to_testing_or_reinit(self, sess=None, feed_dict=None):
        return None

    def set_testing_way(self, model_type, popularity_exp):
        self.testing_model_type, self.testing_popularity = model_type, popularity_exp

    def set_sess(self, sess):
        self.sess = sess

    def predict(self, user_batch, item_batch):                                              # :683-696
        if item_batch is None:
            item_batch = list(range(self.n_items))
        if isinstance(self.Recommender, MACRBPRMF):
            return self.testing(self.sess, user_batch, item_batch, "macr")
        if self.testing_model_type == "o":
            return self.testing(self.sess, user_batch, item_batch, "main_branch")
        if self.testing_model_type == "condition":
            return self.testing(self.sess, user_batch, item_batch, "condition", pos_pop=self.testing_popularity[item_batch])
        raise NotImplementedError("not implement this type testing methods")


class evaluation:
    def __init__(self, data_=None, Ks_=None, device=None, block=None):
        self.data = data_ if data_ is not None else data
        self.Ks = check_ks(Ks_ if Ks_ is not None else Ks)     # (a K < 1 would divide by zero in the metrics kernels)
        self.device = torch.device(device if device is not None else "cuda")
        self.batch_size = block or (getattr(args, "eval_block", 262144) if args is not None else 262144)
        self.testing_popularity = None
        self.eval_who = "test"
        self._hist = None
        self.bias = None
        self.rank = None

    def set_rank_report(self, rank):
        """--rank_report 1 (pda_amd/rank_report.py): a RankReport makes every eval() rank its blocks' targets in the masked full catalogue
        (model.rank_device, the history mask of the lists) and return the four metrics as an EvalResult with the pass's rank lines beside
        them; None (the default) leaves eval() as it is: no kernel call, no allocation."""
        self.rank = rank

    def set_bias_report(self, bias):
        """--bias_report 1 (pda_amd/exposure.py): a BiasReport makes every eval() without an accumulator of its own count its lists and return
        the four metrics as an EvalResult with the pass's bias lines beside them; None (the default) leaves eval() as it is."""
        self.bias = bias

    def set_evaluate_obj(self, eval_who="test"):
        self.eval_who = eval_who

    def set_clicked_value_type(self, value_type):
        """MF/BPR_PC.py's evaluation feeds the history mask with -inf ('inf') or 1.0 ('pc', BPR-PC).  The CSR masks used here carry no
        values: the model that ranks decides what a listed item is worth, so this records the choice and changes nothing else."""
        if value_type not in ("inf", "pc"):
            raise ValueError("clicked value type must be 'inf' or 'pc', not %r" % (value_type,))
        self.value_type = value_type

    def set_testing_popularity(self, popularity):
        """MF/train_new_api.py:710.  The reference indexes testing_popularity[range(ITEM_NUM)] (:788): a vector longer than the
        catalogue is cut to n_items here, a shorter one is an error (there: IndexError at the first evaluation)."""
        self.testing_popularity = popularity
        if popularity is None:
            self._pop_dev = None
            return
        pop = np.asarray(popularity, dtype=np.float32).reshape(-1)
        n = self.data.n_items
        if pop.shape[0] < n:
            raise IndexError("testing popularity has %d entries for %d items" % (pop.shape[0], n))
        self._pop_dev = torch.as_tensor(np.ascontiguousarray(pop[:n]), device=self.device)

    def set_evaluate_obj_pre(self, eval_who="test"):
        """Evaluation users (file order), their targets as CSR, and the train-history mask (:713-739).
        Raises KeyError for an evaluation user without train items under Data2, like the reference."""
        self.eval_who = eval_who
        d = self.data
        self.eval_user_list = d.test_user_list if eval_who == "test" else d.valid_user_list
        users = list(self.eval_user_list.keys())
        self.tot_user = len(users)
        for u in users:
            d.train_user_list[u]                      # KeyError <=> reference (plain dict under Data2, :731)
        if self._hist is None:
            ip, ix, _ = d.train_csr(self.device)
            self._hist = ops.HistoryCSR(ip, ix, by_user=True)
        self.users_dev = torch.as_tensor(np.asarray(users, dtype=np.int32), device=self.device)
        lens = np.fromiter((len(self.eval_user_list[u]) for u in users), dtype=np.int64, count=len(users))
        tp = np.zeros(len(users) + 1, dtype=np.int64)
        np.cumsum(lens, out=tp[1:])
        flat = np.concatenate([np.asarray(self.eval_user_list[u], dtype=np.int32) for u in users]) if users else np.zeros(0, np.int32)
        self._tp_host = tp
        self._tgt_host = flat
        self.tgt_indices = torch.from_numpy(flat).to(self.device)
        self.list_batch_user = [users[i:i + self.batch_size] for i in range(0, len(users), self.batch_size)]

    def eval(self, model, sess, rec_type, exposure=None):
        """-> {'precision','recall','ndcg','hit_ratio': float64[len(Ks)]} = per-user sums / tot_user (:760-778).
        exposure: an exposure.ExposureAccumulator that every block's lists are added to (with the block's targets when it counts hits), for
        the caller to read; the metrics do not depend on it."""
        acc = exposure
        if acc is None and self.bias is not None:
            acc = self.bias.accumulator(self.device)
        if acc is not None and (getattr(model, "_shard", None) is not None or getattr(getattr(model, "model", None), "_shard", None) is not None):
            raise NotImplementedError("the bias report counts the lists of one GPU (an item-sharded evaluation is out of its scope)")
        pop = None if self.testing_popularity is None else self._pop_dev
        ks = torch.as_tensor(self.Ks, dtype=torch.int32, device=self.device)
        sums = torch.zeros((4, len(self.Ks)), dtype=torch.float64, device=self.device)
        ranks, lengths = [], []
        for i in range(0, self.tot_user, self.batch_size):
            ub = self.users_dev[i:i + self.batch_size]
            idx, _ = model.recommend_device(ub, None, rec_type, pop, self._hist, eval_pos=i, eval_users=self.users_dev)
            tp = self._tp_host[i:i + ub.numel() + 1]
            tptr = torch.from_numpy(tp - tp[0]).to(self.device)
            # --deterministic 1: the ordered reduction -- recall decides the early stop and the best checkpoint with `>=`
            det = int(getattr(args, "deterministic", 0) or 0)
            reduce = ops.metrics_route(idx.shape[1], ordered=bool(det))   # (--topk_max: lists beyond 64 columns go to the deep pair)
            tgt = self.tgt_indices[int(tp[0]):int(tp[-1])]
            reduce(idx, tptr, tgt, ks, sums)
            if acc is not None:
                if acc.hit is not None:
                    acc.add(idx, tptr, tgt)
                else:
                    acc.add(idx)
            if self.rank is not None:
                r, n = model.rank_device(ub, rec_type, tptr, tgt, pop, self._hist)
                ranks.append(r)
                lengths.append(n)
        s = (sums / float(self.tot_user)).cpu().numpy()
        ret = {"precision": s[0], "recall": s[1], "ndcg": s[2], "hit_ratio": s[3]}
        if exposure is None and acc is not None:
            ret = EvalResult(ret)
            ret.bias, ret.bias_lines = self.bias, self.bias.report(acc, self._tgt_host).lines()
        if self.rank is not None:
            ret = ret if isinstance(ret, EvalResult) else EvalResult(ret)
            ret.rank_lines = self.rank.stats(torch.cat(ranks).cpu().numpy(), torch.cat(lengths).cpu().numpy(), self._tp_host, self._tgt_host).lines()
        return ret


def early_stop(hr, ndcg, recall, precision, cur_epoch, config, stopping_step, flag_step=10):   # :911-927
    if recall >= config["best_recall"]:
        stopping_step = 0
        config.update(best_hr=hr, best_ndcg=ndcg, best_recall=recall, best_pre=precision, best_epoch=cur_epoch)
    else:
        stopping_step += 1
    should_stop = stopping_step >= flag_step
    if should_stop:
        print("Early stopping is trigger")
    return config, stopping_step, should_stop


def configure(argv=None):
    """What `from batch_test import *` does at import time in the reference (MF/batch_test.py:6-19)."""
    global args, data, Ks, ITEM_NUM, USER_NUM
    args = parse_args(argv)
    if args.train in ("s_condition", "sg_condition", "temp_pop", "us_condition"):
        data = Data2(args)
    else:
        data = Data(args)
    Ks = eval(args.Ks)            # the reference evals this literal too (batch_test.py:16)
    ITEM_NUM, USER_NUM = data.n_items, data.n_users
    return args, data


def check_temp_slots(data_, T: int):
    """BPRMF(t)-pop reads C[i, t] for the slot t of every train interaction: a slot >= T would read the init column (t == T) or past the
    table (the reference: silently 0 on a GPU).  Refused here, when the data is loaded."""
    top = -1
    for ts in data_.train_user_list_time.values():
        if ts:
            top = max(top, max(ts))
    lo = min((min(ts) for ts in data_.train_user_list_time.values() if ts), default=0)
    if top >= T or lo < 0:
        raise ValueError("train time slots span [%d, %d], the popularity file has T = %d stages: temp_pop needs 0 <= slot < T" % (lo, top, T))
    if any(t < 0 or t >= T for t in getattr(data_, "unique_times", [])):
        raise ValueError("unique_times holds a slot outside [0, %d)" % T)


def _print_result(ret):   # :1118-1123
    print("||---------------------------------------------- recall=[%.5f, %.5f], precision=[%.5f, %.5f], hit=[%.5f, %.5f], ndcg=[%.5f, %.5f]"
          % (ret["recall"][0], ret["recall"][-1], ret["precision"][0], ret["precision"][-1],
             ret["hit_ratio"][0], ret["hit_ratio"][-1], ret["ndcg"][0], ret["ndcg"][-1]))
    bias = getattr(ret, "bias", None)                # (--bias_report 1: an exposure.EvalResult)
    if bias is not None:
        for line in bias.header() + ret.bias_lines:
            print(line)
    for line in getattr(ret, "rank_lines", ()):      # (--rank_report 1)
        print(line)


def main(argv=None):
    print("*** Current working path ***")
    print(os.getcwd())
    configure(argv)
    check_topk_max(args)                   # (refusals before anything is built)
    bias = BiasReport.from_args(args, data, Ks)
    rank = RankReport.from_args(args, data)
    if args.model == "lightgcn":
        check_lightgcn(args)
    elif args.model != "mf":
        raise NotImplementedError("--model %s: mf | lightgcn" % args.model)
    check_dns(args)                        # (--neg_sampler dns)
    check_negpop(args)                     # (--neg_sampler pop)
    check_ials(args)                       # (--train ials | --test ials)
    if args.train == "dice":
        check_dice(args)
        if args.test not in ("normal", "dice"):
            raise NotImplementedError("--train dice goes with --test normal (DICE and DICE-A) or --test dice, not --test " + str(args.test))
    if args.train == "ips":
        check_ips(args)
        if args.test not in ("normal", "ips"):
            raise NotImplementedError("--train ips goes with --test normal (the raw head and the gamma search of a BPRMF) or --test ips, not --test "
                                      + str(args.test))
    if args.train == "pcc":
        check_pcc(args)
        if args.test not in ("normal", "pcc"):
            raise NotImplementedError("--train pcc goes with --test normal (the raw head and the gamma search of a BPRMF) or --test pcc, not --test "
                                      + str(args.test))
    if args.train == "dau":
        check_dau(args)
        if args.test not in ("normal", "dau"):
            raise NotImplementedError("--train dau goes with --test normal (the raw head and the gamma search of a BPRMF) or --test dau, not --test "
                                      + str(args.test))
    if args.train == "warp":
        check_warp(args)                   # (--test outside normal | warp included)
    if args.train == "ssm":
        check_ssm(args)
        if args.test not in ("normal", "ssm"):
            raise NotImplementedError("--train ssm goes with --test normal (the raw head and the gamma search of a BPRMF) or --test ssm, not --test "
                                      + str(args.test))
    if args.train == "macr":
        check_macr(args)
        if args.test != "macr":
            raise NotImplementedError("--train macr goes with --test macr (the counterfactual head and the search over c), not --test " + str(args.test))
    elif args.test == "macr":
        raise NotImplementedError("--test macr needs a MACR model (--train macr), not --train " + str(args.train))
    random.seed(2020)                      # :934-936
    np.random.seed(2020)
    torch.manual_seed(2021)
    if torch.cuda.device_count() > 1 and str(args.cuda).isdigit() and int(args.cuda) < torch.cuda.device_count():
        torch.cuda.set_device(int(args.cuda))
    device = torch.device("cuda")
    config = {"n_users": data.n_users, "n_items": data.n_items}
    popularity_exp = args.pop_exp
    print("----- popularity_exp : ", popularity_exp)
    test_batch_size = min(1024, args.batch_size)

    pop_item_all = load_popularity(args)                                         # :952-959
    last_stage_popualarity = np.power(pop_item_all[:, -2], popularity_exp)
    linear_predict_popularity = pop_item_all[:, -2] + 0.5 * (pop_item_all[:, -2] - pop_item_all[:, -3])
    linear_predict_popularity[np.where(linear_predict_popularity <= 0)] = 1e-9
    linear_predict_popularity[np.where(linear_predict_popularity > 1.0)] = 1.0
    linear_predict_popularity = np.power(linear_predict_popularity, popularity_exp)

    with_pop = False
    if args.model == "lightgcn":           # the graph's edges reach the model the way ips_item_counts does
        config["gcn_train_pairs"] = gcn_train_pairs(data.train_user_list)
        args.saveID += "gcn_layers-{}".format(args.gcn_layers)
    if args.train == "ials":               # the pairs reach the model the way a LightGCN's edges do
        config["gcn_train_pairs"] = gcn_train_pairs(data.train_user_list)
    if args.model in ("mf", "lightgcn") and args.train in ("normal", "dice", "ips", "macr", "ssm", "ials", "pcc", "dau", "warp"):   # :963-970 (DICE, IPS, SSM, PCC, DirectAU and WARP are evaluated like a BPRMF: --test normal)
        args.saveID += "pop_exp-{:.2f}".format(popularity_exp)
        print({"normal": "normal MF... ", "dice": "-------    running DICE  ----------------", "macr": "-------    running MACR  ----------------",
               "ssm": "-------    running SSM  ----------------", "ials": "-------    running iALS  ----------------",
               "pcc": "-------    running PCC  ----------------", "dau": "-------    running DirectAU  ----------------", "warp": "-------    running WARP  ----------------"}.get(args.train, "-------    running IPS  ----------------"))
        if args.train == "macr":
            args.saveID += "macr"
        if args.train == "ssm":
            args.saveID += "ssm"
        if args.train == "ials":
            args.saveID += "ials"
        if args.train == "dau":
            args.saveID += "dau"
        if args.train == "warp":
            args.saveID += "warp"
        if args.train == "ips":
            args.saveID += "ips"
            config["ips_item_counts"] = ips_item_counts(data.train_user_list, data.n_items)
        if args.train == "pcc":            # the popularities are built from the counts the propensities are built from
            args.saveID += "pcc"
            config["ips_item_counts"] = ips_item_counts(data.train_user_list, data.n_items)
        last_stage_popualarity_ori = pop_item_all[:, -2]
        linear_predict_popularity_ori = pop_item_all[:, -2] + 0.5 * (pop_item_all[:, -2] - pop_item_all[:, -3])
        # the reference masks with the already-powered array (a quirk): kept
        linear_predict_popularity_ori[np.where(linear_predict_popularity <= 0)] = 1e-9
        linear_predict_popularity_ori[np.where(linear_predict_popularity > 1.0)] = 1.0
    elif args.model in ("mf", "lightgcn") and args.train == "s_condition":       # :984-997
        print("-------    running PD & PDA model  ----------------")
        args.saveID += "pop_exp-{:.2f} (gamma)".format(popularity_exp)
        print("save_ID", args.saveID)
        popularity_matrix = get_popularity_from_load(pop_item_all)
        popularity_matrix = np.power(popularity_matrix, popularity_exp)
        print("------ popularity information after powed  ------")
        print("   each stage mean:", popularity_matrix.mean(axis=0))
        print("   each stage max:", popularity_matrix.max(axis=0))
        print("   each stage min:", popularity_matrix.min(axis=0))
        data.add_expo_popularity(popularity_matrix)
        with_pop = True
        if args.test == "normal":          # (--model lightgcn --train s_condition --test normal: the gamma search of the normal branch reads these)
            last_stage_popualarity_ori = pop_item_all[:, -2]
            linear_predict_popularity_ori = pop_item_all[:, -2] + 0.5 * (pop_item_all[:, -2] - pop_item_all[:, -3])
            linear_predict_popularity_ori[np.where(linear_predict_popularity <= 0)] = 1e-9
            linear_predict_popularity_ori[np.where(linear_predict_popularity > 1.0)] = 1.0
    elif args.model == "mf" and args.train == "temp_pop":                        # :999-1005
        print("-------    running temproal pop MF  ----------------")
        config["temp_num"] = pop_item_all.shape[1] - 1
        args.saveID += "temp_pop"
        print("save_ID", args.saveID)
        data.add_expo_popularity(None)
        check_temp_slots(data, config["temp_num"])
    else:
        raise NotImplementedError("do not implement this method")               # :1008

    neg_table = None
    if getattr(args, "neg_sampler", "uniform") == "pop":         # (check_negpop has refused everything but the device sampler of normal | s_condition | ssm sampled)
        neg_table = ops.NegPopTable(data.train_csr("cpu")[1], data.n_items, args.neg_pop_power, (0, data.n_items), device)
        print("||--- neg_sampler pop power=%g max_q=%.6g entropy=%.5f (uniform: %.5f)" % ((neg_table.power,) + neg_table.stats()))
    if args.train == "ials":               # no sampler: every epoch is two half-sweeps over all pairs
        sampler = None
    elif args.train == "temp_pop":
        if args.sampler == "device":
            sampler = DeviceSampler(data, device, False, temp_slots=config["temp_num"])
        else:
            sampler = (lambda: host_generator_with_temp(data))
    elif args.train == "dice":
        if args.sampler == "device":
            sampler = DeviceSampler(data, device, False, mode="dice", margin=args.dice_margin, margin_decay=args.dice_margin_decay)
        else:
            sampler = HostDiceSampler(data, args.dice_margin, args.dice_margin_decay)
    elif args.train == "dau":              # (check_dau has refused --sampler host) the triplet sampler without popularity columns; its negative is ignored
        sampler = DeviceSampler(data, device, False)
    elif args.train == "warp":             # (check_warp has refused --sampler host and --neg_sampler dns | pop)
        sampler = DeviceSampler(data, device, False, mode="warp", max_trials=args.warp_max_trials, margin=args.warp_margin,
                                wtab=ops.WarpWeights.build(data.n_items, args.warp_max_trials, args.warp_weight, device))
    elif args.train == "ssm":              # (check_ssm has refused --sampler host)
        if args.ssm_source in ("batch", "all"):    # in-batch negatives / the whole catalogue: the triplet sampler without popularity columns; its negative is ignored
            sampler = DeviceSampler(data, device, False)
        else:
            sampler = DeviceSampler(data, device, False, mode="ssm", n_negs=args.ssm_negs, neg_table=neg_table)
    elif getattr(args, "neg_sampler", "uniform") == "dns":       # (check_dns has refused everything but --train normal | s_condition on the device sampler)
        sampler = DeviceSampler(data, device, with_pop, mode="dns", n_cands=args.dns_candidates, topn=args.dns_topn)
    elif args.sampler == "device":
        sampler = DeviceSampler(data, device, with_pop, neg_table=neg_table)
    else:
        sampler = (lambda: host_generator(data, with_pop))
    model = DatasetApi_Model(args, config, test_batch_size, sampler, device)
    sess = Session(model)
    model.set_sess(sess)
    args.wd = args.regs                                                          # :1020

    evaluation_model = evaluation(data, Ks, device)
    evaluation_model.set_bias_report(bias)
    evaluation_model.set_rank_report(rank)
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
    print("top K:", Ks)
    if args.pretrain != 0:
        raise NotImplementedError("only --pretrain 0 exists in the reference (MF/train_new_api.py:1048)")

    rec = model.Recommender
    best_pop_expo_normal = 0
    keys = ("best_hr", "best_ndcg", "best_recall", "best_pre", "best_epoch")
    config.update({k: 0 for k in keys})
    config_main = dict(config)
    stopping_step = stopping_step_main = 0
    n_batch = data.n_train // args.batch_size + 1
    save_ckpt_dir = args.save_dir + "{}_{}_checkpoint/wd_{}_lr_{}_a_{}_{}_train_{}/".format(
        args.model, args.dataset, args.wd, args.lr, args.alpha, args.saveID, args.train)   # :1214
    t1 = time()
    print("batch_num:", n_batch, "waiting sampling...")
    fetches = ([rec.opt_pop_global, rec.loss_pop_global, rec.mf_loss_pop_global, rec.reg_loss_pop_global]
               if args.train == "s_condition" else [rec.opt, rec.loss, rec.mf_loss, rec.reg_loss])

    def save(name):
        os.makedirs(save_ckpt_dir, exist_ok=True)
        torch.save(rec.state_dict(), save_ckpt_dir + name)

    for epoch in range(args.epoch):
        if args.train == "ials":
            # no batch loop: two half-sweeps and the objective; the epoch's one host read takes (loss, fit, reg) / |S| and the failed-pivot counter
            loss, mf_loss, reg_loss, failed = torch.cat([rec.train_epoch(), rec.failed_pivots().double()]).tolist()
            if failed:
                print("ERROR: %d rows had a failed pivot (non-finite tables?)." % int(failed))
                sys.exit()
        else:
            if args.train == "dice":                    # DICE's schedule: the margin and the two loss weights decay at the start of an epoch
                rec.start_epoch(epoch, sampler.start_epoch(epoch))
            model.switch_to_training_or_reinitsampler(sess)
            rec.start_loss_rows(n_batch + 1)            # losses stay on the device, a row per step: one reduction and one sync per epoch
            extra = torch.zeros(3, dtype=torch.float64, device=device)
            try:
                while True:
                    before = rec._loss_row_i
                    row = sess.run_async(fetches)
                    if rec._loss_row_i == before:       # (a generator longer than n_batch + 1 steps: the step fell back to the ring's rows)
                        extra += rec.trainer_terms(row) if hasattr(rec, "trainer_terms") else row[:3]
            except OutOfRangeError:
                pass
            acc = rec.finish_loss_rows() + extra
            loss, mf_loss, reg_loss = (acc / n_batch).tolist()
        if np.isnan(loss):
            print("ERROR: loss is nan.")
            sys.exit()
        perf_str = "Epoch %d [%.1fs]: train==[%.5f=%.5f + %.5f]" % (epoch, time() - t1, loss, mf_loss, reg_loss)
        if args.train == "pcc":            # the epoch's mean r and r^2 over its steps: one more host read beside the loss
            perf_str += "\n||--- pcc r=%.5f r2=%.5f (gamma=%g, on=%s, pop=%s)" % (rec.take_pcc() + (rec.pcc_gamma, rec.pcc_on, rec.pcc_pop))
        if args.train == "dau":            # the epoch's mean alignment and uniformity terms over its steps: one more host read beside the loss
            perf_str += "\n||--- dau align=%.5f uni_u=%.5f uni_i=%.5f (gamma=%g, t=%g, same=%s)" % (rec.take_dau() + (rec.dau_gamma, rec.dau_t, rec.dau_same))
        if args.train == "warp":           # the epoch's trial counts, summed on the device by the sampler: one more host read beside the loss
            perf_str += "\n||--- warp trials=%.3f none=%.4f" % sampler.take_warp_stat()
        if epoch % args.log_interval != 0:
            if args.verbose > 0 and epoch % args.verbose == 0:
                print(perf_str)
            t1 = time()
            continue

        if args.test in ("condition", "s_condition"):                            # :1125-1156
            print("do not consider popularity (PD or PDG) ... ")
            print(perf_str)
            evaluation_model.set_testing_popularity(None)
            ret_main = evaluation_model.eval(model, sess, rec_type="main_branch")
            _print_result(ret_main)
            print("injecting last stage popularity.... ")
            ttt1 = time()
            evaluation_model.set_testing_popularity(last_stage_popualarity)
            ret1 = evaluation_model.eval(model, sess, rec_type="condition")
            print("||------------PDA/PDGA injecting last stage popularity testing : time: ", int(time() - ttt1))
            _print_result(ret1)
            ttt1 = time()
            evaluation_model.set_testing_popularity(linear_predict_popularity)
            ret2 = evaluation_model.eval(model, sess, rec_type="condition")
            print("||------------PDA/PDGA injecting linear predicted popularity testing : time: ", int(time() - ttt1))
            _print_result(ret2)
            ret = ret1
        elif args.test in ("temp_pop", "dice", "ips", "ssm", "ials", "pcc", "dau", "warp"):     # :1192-1200 (--test dice / ips / ssm / ials / pcc / dau / warp: the main_branch head alone)
            print(perf_str)
            ttt1 = time()
            evaluation_model.set_testing_popularity(None)
            ret_main = evaluation_model.eval(model, sess, rec_type="main_branch")
            print("test: time:", time() - ttt1)
            _print_result(ret_main)
            ret = ret_main
        elif args.test == "macr":
            # MACR: c = 0 (rubi_ratings_both_nonc) first, then the search over c; the best c by recall@Ks[0] on the validation objective
            # drives the early stop and best_ckpt.ckpt, c = 0 the main ones
            print(perf_str)
            ttt1 = time()
            evaluation_model.set_testing_popularity(None)
            rec.update_c(0.0)
            ret_main = evaluation_model.eval(model, sess, rec_type="macr")
            print("MACR without c")
            _print_result(ret_main)
            best_ret, best_c = ret_main, 0.0
            for c in macr_c_grid(args):
                rec.update_c(c)
                ret_c = evaluation_model.eval(model, sess, rec_type="macr")
                if ret_c["recall"][0] > best_ret["recall"][0]:
                    best_ret, best_c = ret_c, c
                print("c: {:.4f} best c: {:.4f}".format(c, best_c))
                _print_result(ret_c)
            rec.best_c = best_c
            rec.update_c(best_c)
            print("MACR best c: {:.6f}  test: time: {:.3f}".format(best_c, time() - ttt1))
            _print_result(best_ret)
            ret = best_ret
        elif args.test == "normal":                                              # :1159-1191
            print(perf_str)
            ttt1 = time()
            evaluation_model.set_testing_popularity(None)
            ret_main = evaluation_model.eval(model, sess, rec_type="main_branch")
            print("test: time:", time() - ttt1)
            _print_result(ret_main)
            best_ret, best_expo, not_incre, expo = ret_main, 0, 0, 0.04
            while True:                                                          # gamma-tilde line search for BPRMF-A
                evaluation_model.set_testing_popularity(np.power(last_stage_popualarity_ori, expo))
                ret_k = evaluation_model.eval(model, sess, rec_type="main_with_pop")
                if ret_k["recall"][0] < best_ret["recall"][0]:
                    not_incre += 1
                    if not_incre > 4:
                        break
                else:
                    not_incre, best_ret, best_expo = 0, ret_k, expo
                print("expo: {:.2f} best expo:{:.2f}".format(expo, best_expo))
                _print_result(ret_k)
                expo += 0.02
            if best_ret["recall"][0] >= config["best_recall"]:
                best_pop_expo_normal = best_expo
            ret = best_ret
        else:
            raise NotImplementedError("not implement this test method:" + args.test)   # :1202

        stop_flag_step = 100 // args.log_interval                                # :1210-1232
        config, stopping_step, should_stop = early_stop(ret["hit_ratio"][0], ret["ndcg"][0], ret["recall"][0],
                                                        ret["precision"][0], epoch, config, stopping_step, stop_flag_step)
        config_main, stopping_step_main, should_stop_main = early_stop(
            ret_main["hit_ratio"][0], ret_main["ndcg"][0], ret_main["recall"][0], ret_main["precision"][0], epoch,
            config_main, stopping_step_main, stop_flag_step)
        if epoch == config["best_epoch"]:
            save("best_ckpt.ckpt")
        if epoch == config_main["best_epoch"]:
            save("best_main_ckpt.ckpt")
        if args.save_flag == 1 and (epoch + 1) % 50 == 0:
            save("{}_ckpt.ckpt".format(epoch))
        if should_stop and args.early_stop == 1 and should_stop_main:
            msg = "{} dataset best epoch{}: hr:{} ndcg:{} recall:{} precision:{}".format(
                args.dataset, config["best_epoch"], config["best_hr"], config["best_ndcg"], config["best_recall"], config["best_pre"])
            print(msg)
            print("{} dataset best main epoch{}: hr:{} ndcg:{} recall:{} precision:{}".format(
                args.dataset, config_main["best_epoch"], config_main["best_hr"], config_main["best_ndcg"],
                config_main["best_recall"], config_main["best_pre"]))
            logging.info(msg)
            if args.save_flag == 1:
                os.makedirs(save_ckpt_dir, exist_ok=True)
                with open(save_ckpt_dir + "/best_epoch.txt", "w") as f:
                    print(config["best_epoch"], file=f)
            break
        t1 = time()

    # ---- final report on the best checkpoints (:1253-1327) ----------------------------------------------
    print("best epoch", config["best_epoch"])
    rec.load_state_dict(torch.load(save_ckpt_dir + "best_ckpt.ckpt", map_location=device))
    print("validation result in best epoch")
    evaluation_model.set_testing_popularity(None)
    ret = evaluation_model.eval(model, sess, rec_type="main_branch")
    print("---- result without pop:")
    _print_result(ret)
    print("|||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||||")
    print("|| ---------------- testing testset in the best epoch:  ... ")
    evaluation_model.set_evaluate_obj_pre("test")
    if args.test == "s_condition":
        evaluation_model.set_testing_popularity(None)
        ret = evaluation_model.eval(model, sess, rec_type="main_branch")
        print("---- PD/PDG result without pop at the model select by PDA/PDG-A:")
        _print_result(ret)
        evaluation_model.set_testing_popularity(last_stage_popualarity)
        ret = evaluation_model.eval(model, sess, rec_type="condition")
        print("---- PDA/PDG-A injecting last stage pop:\n", ret)
        _print_result(ret)
        evaluation_model.set_testing_popularity(linear_predict_popularity)
        ret = evaluation_model.eval(model, sess, rec_type="condition")
        print("---- result with linear pop:\n", ret)
        _print_result(ret)
    elif args.test == "normal":
        evaluation_model.set_testing_popularity(None)
        ret = evaluation_model.eval(model, sess, rec_type="main_branch")
        print("---- BPRMF result without injecting pop:")
        _print_result(ret)
        print("best_pop_expo in training:", best_pop_expo_normal)
        for name, base in (("last stage pop(best gamma)", last_stage_popualarity_ori),
                           ("linear predicted pop (best gamma)", linear_predict_popularity_ori)):
            evaluation_model.set_testing_popularity(np.power(base, best_pop_expo_normal))
            r = evaluation_model.eval(model, sess, rec_type="main_with_pop")
            print("|||---BPRMF-A with injecting %s:" % name)
            _print_result(r)
        print("----------------------------")
    elif args.test == "macr":
        evaluation_model.set_testing_popularity(None)
        rec.update_c(0.0)
        ret = evaluation_model.eval(model, sess, rec_type="macr")
        print("---- MACR without c:")
        _print_result(ret)
        rec.update_c(rec.best_c)
        ret = evaluation_model.eval(model, sess, rec_type="macr")
        print("---- MACR result with the best c of the validation (c = {:.6f}):".format(rec.best_c))
        _print_result(ret)
    elif args.test in ("temp_pop", "dice", "ips", "ssm", "ials", "pcc", "dau", "warp"):  # :1310-1314
        evaluation_model.set_testing_popularity(None)
        ret = evaluation_model.eval(model, sess, rec_type="main_branch")
        print({"temp_pop": "---- result with last pop bias for temp_pop model:", "dice": "---- DICE result (interest + conformity):"}
              .get(args.test, {"ssm": "---- SSM result:", "ials": "---- iALS result:", "pcc": "---- PCC result:", "dau": "---- DirectAU result:", "warp": "---- WARP result:"}.get(args.test, "---- IPS result:")))
        _print_result(ret)
    print("training and testing end!!!!")
    print("|||  ------------------------ best performance for model selected by PD/PDG/BPRMF ------------------- |||")
    print("main best epoch:", config_main["best_epoch"])
    rec.load_state_dict(torch.load(save_ckpt_dir + "best_main_ckpt.ckpt", map_location=device))
    evaluation_model.set_testing_popularity(None)
    ret = evaluation_model.eval(model, sess, rec_type="main_branch")
    print("---- result without injecting pop:")
    _print_result(ret)
    return config, config_main


if __name__ == "__main__":
    main()
