"""Model objects with the reference's names and constructor arguments (MF/model_api.py), backed by HIP kernels.

    ConditionalBPRMF   PD / PDA            MF/model_api.py:14-185
    BPRMFTempPop       BPRMF(t)-pop        MF/model_api.py:300-416   (temporal popularity bias; Adam sweep only)
    BPRMF              plain BPR-MF        MF/model_api.py:419-757   (only :419-471, :521-536, :695-706 are live)
    DICE               DICE / DICE-A       (no reference code: DESIGN.md 5f)   interest + conformity embeddings in one 2d-wide row; Adam sweep only
    IPSBPRMF           IPS / IPS-C / IPS-CN (no reference code: DESIGN.md 5g)  a BPRMF trained with inverse propensity weights; Adam sweep only
    PCCBPRMF           BPR + gamma r^2 (no reference code: DESIGN.md 5r)       a BPRMF trained with the popularity-correlation regulariser; Adam sweep only
    DAUMF              DirectAU            (no reference code: DESIGN.md 5s)   a BPRMF trained with the alignment + uniformity loss, no negatives; Adam sweep only
    SSMBPRMF           SSM                 (no reference code: DESIGN.md 5l)   a BPRMF trained with the sampled-softmax loss; Adam sweep only
    MACRBPRMF          MACR                MF/model_api.py:613-651, :627-628 (never driven by the reference's trainer: DESIGN.md 5h); Adam sweep only
    LightGCN           the LightGCN backbone (no reference code: DESIGN.md 5j)  ego tables propagated over the train graph; ConditionalLightGCN: PD/PDA on it
    WARPBPRMF          WARP                (no reference code: DESIGN.md 5x)   a BPRMF trained with the rank-weighted hinge on the first violating candidate; Adam sweep only
    IALSMF             iALS                (no reference code: DESIGN.md 5o)   the tables of a BPRMF solved row by row (implicit ALS); no step, train_epoch()

A TF-1 graph exposes *fetchables* (`opt`, `loss`, `mf_loss`, `reg_loss`, `batch_ratings`, ...) that the
trainer passes to `sess.run`.  Here they are light handle objects understood by `pda_amd.train_new_api.Session`,
so the reference's loop `sess.run([model.Recommender.opt, model.Recommender.loss, ...])` keeps its shape;
the direct API is `train_step(users, pos, neg[, pos_pop, neg_pop]) -> float32[3] device tensor`.

Optimisers (`args.optimizer`):
    adam       TF-1.14 AdamOptimizer semantics: m, v decayed and EVERY row updated each step [TF-ext].  Reference-faithful.  Small tables
               (up to ADAM_SWEEP_MAX_BYTES): pda_adam_step_f32 -- the step kernel sums the gradients and tags the batch's rows, the tagged
               sweep updates both tables; two launches (pda_adam_step_plan_f32 under --deterministic: three).  Larger tables, or
               --adam_sweep replay: the same arithmetic without the sweep, bit for bit -- pda_adam_lazy_f32 phase 0 (the batch's rows
               replay their idle steps), the gradient, pda_adam_lazy_f32 phase 1.
    lazy_adam  the same update restricted to the rows touched by the batch (declared deviation): the gradient, then pda_adam_rows_f32
               on the unique rows of each table.
               The gradient is pda_bpr_step_f32(DENSE_GRAD), pda_bpr_grad_plan_f32 under --deterministic, pda_bpr_step_bf16 on bf16 tables
               (_MFBase._adam_step is the one place that spells these steps out).
    sgd        plain mini-batch SGD, exact: gradients of the whole batch against the unchanged tables, then one scatter
               (pda_bpr_step_f32(PDA_UPD_NONE) + pda_sgd_apply_f32; declared deviation from MF/model_api.py:83 = Adam).
    sgd_fused  the north_star's fused in-kernel scatter update, ONE launch per step: asynchronous inside the launch (a row
               gathered by one workgroup may already carry another triplet's update -- hogwild-style, equal to `sgd` up to
               O(lr) cross terms, not bit-reproducible).  The throughput mode; `sgd` is the reference semantics.

Table type (`args.table_dtype`, extension; BASELINE config 5): with "bf16" the forward pass and the evaluation read bf16
copies of the tables (`score_tables()`), gradients stay fp32 and `weights[...]` are the fp32 masters that take the
update; the touched rows (sgd / lazy_adam) or the whole tables (adam) are re-rounded after every step.

Determinism (`args.deterministic`, extension; DESIGN.md "Deterministic training"): with 1 every step sums its gradients in the order
of the batch's plan (ops.adam_step_plan / ops.bpr_grad_plan / ops.bpr_step_plan) instead of with float atomics, so a run is a function
of its flags and data alone, bit for bit.  Combinations that cannot keep that promise are refused when the model is built.
"""
from __future__ import annotations

import copy
import math

import torch

from . import ops


class Fetch:
    """Stand-in for a TF tensor/op handle: `Session.run` dispatches on (owner, name)."""

    def __init__(self, owner, name):
        self.owner, self.name = owner, name

    def __repr__(self):
        return "<pda_amd fetch %s.%s>" % (type(self.owner).__name__, self.name)


def xavier_uniform_(t: torch.Tensor, gen: torch.Generator):
    """tf.contrib.layers.xavier_initializer(): U(-l, l), l = sqrt(6/(fan_in+fan_out)) [TF-ext]; :88-92, :523-527."""
    lim = math.sqrt(6.0 / (t.shape[0] + t.shape[1]))
    return t.uniform_(-lim, lim, generator=gen)


DET_EMBED_SIZES = (32, 64, 128, 256)      # the row widths of the planned kernels (pda_bpr_grad_plan_f32, pda_bpr_step_plan_f32)


def check_deterministic(args, data_config):
    """--deterministic 1: refuse, before anything touches the GPU, what has no bit-reproducible path."""
    opt = getattr(args, "optimizer", "adam")
    if getattr(args, "train", "normal") == "temp_pop":
        raise NotImplementedError("--deterministic: --train temp_pop sums the gradients of its four tables with float atomics")
    if opt == "sgd_fused":
        raise NotImplementedError("--deterministic: --optimizer sgd_fused updates rows inside the launch that gathers them (hogwild by design)")
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--deterministic runs on one GPU")
    if getattr(args, "table_dtype", "f32") == "bf16" and opt in ("adam", "lazy_adam"):
        raise NotImplementedError("--deterministic: --table_dtype bf16 under an Adam optimiser has no planned gradient (fp32 tables, or --optimizer sgd)")
    if int(args.embed_size) not in DET_EMBED_SIZES:
        raise NotImplementedError("--deterministic: --embed_size must be one of %s (the planned kernels)" % (DET_EMBED_SIZES,))
    if int(args.batch_size) > int(data_config["n_users"]):
        raise NotImplementedError("--deterministic: --batch_size %d > %d users -- the sampler then draws users with replacement and every batch's "
                                  "plan would be rejected" % (args.batch_size, data_config["n_users"]))


class _MFBase:
    with_pop = False
    ADAM_SWEEP_MAX_BYTES = 64 << 20      # C1/C2 (12 .. 18 MB of tables) sweep; config 3 (614 MB) and up replay

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None,
                 neg_items_api=None, pos_pop_api=None, neg_pop_api=None, device=None, seed=2021):
        self.deterministic = bool(int(getattr(args, "deterministic", 0) or 0))
        if self.deterministic:
            check_deterministic(args, data_config)
        self.n_users = data_config["n_users"]
        self.n_items = data_config["n_items"]
        self.decay = args.regs                       # MF/model_api.py:23
        self.emb_dim = args.embed_size
        self.lr = args.lr
        self.batch_size = args.batch_size            # the flag constant that divides the regulariser (:118)
        self.verbose = args.verbose
        self.optimizer = getattr(args, "optimizer", "adam")
        if self.optimizer not in ("adam", "lazy_adam", "sgd", "sgd_fused"):
            raise NotImplementedError("optimizer must be adam | lazy_adam | sgd | sgd_fused")
        self.table_dtype = getattr(args, "table_dtype", "f32")
        if self.table_dtype not in ("f32", "bf16"):
            raise NotImplementedError("table_dtype must be f32 | bf16")
        self.device = torch.device(device if device is not None else "cuda")
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)                        # tf.set_random_seed(2021), MF/train_new_api.py:936
        self.weights = self.init_weights(gen)
        self.tables16 = None
        if self.table_dtype == "bf16":
            self.tables16 = {k: v.bfloat16() for k, v in self.weights.items()}
        self._t = 0
        self._state = None
        # optimizer == "adam": the reference's dense-decay Adam either as a sweep over both tables per step (small tables) or
        # EXACTLY the same arithmetic without the sweep (ops.adam_lazy: idle rows replay their decay when next needed) once the
        # tables outgrow ADAM_SWEEP_MAX_BYTES; args.adam_exact_lazy = True | False forces one
        forced = getattr(args, "adam_exact_lazy", None)
        mode = getattr(args, "adam_sweep", "auto")
        if mode not in ("auto", "sweep", "replay", "replay_fast"):
            raise NotImplementedError("adam_sweep must be auto | sweep | replay | replay_fast")
        if forced is None and mode != "auto":
            forced = mode != "sweep"
        # replay (and auto, above 64 MB of tables): bit-identical to the sweeps -- the reference-parity optimiser and the checkpoints
        # written behind sync_optimizer stay bit-equal to the dense-decay Adam.  replay_fast is an explicit opt-in: the same catch-up
        # with a running sqrt, the hardware reciprocal and closed-form powers for m and v (PDA_ADAM_REPLAY_FAST, ~4 x less
        # arithmetic); x to 1e-6 per catch-up against the sweep (tests/test_gpu_bpr_step.py), NOT bit-equal, and the per-catch-up
        # error (~4e-8 |x|: the geometric tail is ~10 x the last term) accumulates over the row's touches of a long run
        self.adam_replay_fast = mode == "replay_fast"
        table_bytes = (self.n_users + self.n_items) * self.emb_dim * 4
        self.adam_exact_lazy = (table_bytes > self.ADAM_SWEEP_MAX_BYTES) if forced is None else bool(forced)
        self._lazy = None
        # loss buffers: a ring of 16 -- train_step returns the buffer of THIS step; it is overwritten 16 steps later, so a
        # caller may keep a handful of returned tensors and sync once (no per-step clone launch, no per-step host sync)
        self._loss_ring = torch.zeros((16, 3), dtype=torch.float32, device=self.device)
        self._loss_i = 0
        self._loss = self._loss_ring[0]
        self._statistics_params()

    # ---- parameters -----------------------------------------------------------------------------------
    def init_weights(self, gen):
        w = {}
        w["user_embedding"] = xavier_uniform_(torch.empty(self.n_users, self.emb_dim, device=self.device), gen)
        w["item_embedding"] = xavier_uniform_(torch.empty(self.n_items, self.emb_dim, device=self.device), gen)
        return w

    def _statistics_params(self):
        total = sum(int(v.numel()) for v in self.weights.values())
        if self.verbose > 0:
            print("#params: %d" % total)

    def _opt_state(self):
        if self._state is None:
            U, I = self.weights["user_embedding"], self.weights["item_embedding"]
            z = torch.zeros_like
            self._state = {"mU": z(U), "vU": z(U), "gU": z(U), "mI": z(I), "vI": z(I), "gI": z(I)}
        return self._state

    def sync_optimizer(self):
        """Exact lazy Adam: bring every row (and its moments) to the current step -- before anything reads whole tables
        (evaluation, checkpoint).  A no-op for the other optimisers and when nothing is behind."""
        if self._lazy is not None and self._lazy.synced < self._t:
            st = self._state
            ops.adam_lazy_sync(self._lazy, self.weights["user_embedding"], st["mU"], st["vU"], self.weights["item_embedding"], st["mI"],
                               st["vI"], self._t)
            if self.tables16 is not None:
                ops.refresh_rows_bf16(self.weights["user_embedding"], self.tables16["user_embedding"])
                ops.refresh_rows_bf16(self.weights["item_embedding"], self.tables16["item_embedding"])

    def _lazy_state(self):
        if self._lazy is None:
            self._lazy = ops.LazyAdamState(self.n_users, self.n_items, self.lr, self.device, fast=self.adam_replay_fast)
            self._lazy.synced = self._t - 1 if self._t > 0 else 0      # (rows are current for everything before this step)
            if self._t > 1:
                self._lazy.lastU.fill_(self._t - 1)
                self._lazy.lastI.fill_(self._t - 1)
        return self._lazy

    def score_tables(self):
        """(U, I) the evaluation kernels read: the weights, or their bf16 copies when table_dtype == 'bf16'."""
        self.sync_optimizer()
        t = self.tables16 if self.tables16 is not None else self.weights
        return t["user_embedding"], t["item_embedding"]

    # ---- the losses of an announced run of steps (the trainer's epoch, MF/train_new_api.py:1078-1095) -------------
    def start_loss_rows(self, n_steps: int):
        """The next n_steps train_step calls write their (loss, mf, reg) into consecutive rows of one zeroed float32 [n_steps, 3] block (each call
        still returns ITS row); finish_loss_rows() returns the float64 sum of the rows written.  Saves a memset launch and an accumulation
        launch per step: 32.6 -> 28 us per step through the CLI on the Douban-shaped synthetic."""
        self._loss_rows = torch.zeros((max(1, int(n_steps)), 3), dtype=torch.float32, device=self.device)
        self._loss_row_i = 0

    def finish_loss_rows(self) -> torch.Tensor:
        rows, n = self._loss_rows, self._loss_row_i
        self._loss_rows = None
        return rows[:n].double().sum(0)

    # ---- one training step (A1-A5) --------------------------------------------------------------------
    def train_step(self, users, pos, neg, pos_pop=None, neg_pop=None, plan=None) -> torch.Tensor:
        """Forward + loss + gradient + update on one batch of device tensors (int32 / float32).
        plan (--optimizer sgd): the batch's pda_triplet_plan from a sampler that guarantees distinct users -- the exact step then
        runs without atomics (ops.bpr_step_plan: two launches, bit-reproducible); without a plan the exact step is
        pda_bpr_step_f32(PDA_UPD_NONE) + pda_sgd_apply_f32, which accepts any batch.
        Returns the float32[3] device tensor (loss, mf_loss, reg_loss) of THIS step (no host sync): a view into a ring of
        16 buffers -- valid until 16 further steps have been enqueued."""
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        if not self.with_pop:
            pos_pop = neg_pop = None
        elif pos_pop is None or neg_pop is None:
            raise ValueError("PD/PDA needs pos_pop and neg_pop")
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            # a caller that announced its steps (start_loss_rows: the trainer's epoch) gets a row of ONE pre-zeroed block per step: no memset
            # launch per step, and the epoch's sum is one reduction at its end
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        if self.deterministic and plan is None:
            plan = ops.triplet_plan(users, pos, neg)[0]      # (a batch source without plans: the host sampler, injected batches)
        if self.optimizer == "sgd" and plan is not None:
            if self.tables16 is not None:
                self._plan_scratch = ops.bpr_step_plan(self.tables16["user_embedding"], self.tables16["item_embedding"], users, pos, neg, pos_pop,
                                                       neg_pop, regs=self.decay, reg_div=self.batch_size, lr=self.lr, plan=plan,
                                                       scratch=getattr(self, "_plan_scratch", None), loss_acc=self._loss, U_master=U, I_master=I)
            else:
                self._plan_scratch = ops.bpr_step_plan(U, I, users, pos, neg, pos_pop, neg_pop, regs=self.decay, reg_div=self.batch_size,
                                                       lr=self.lr, plan=plan, scratch=getattr(self, "_plan_scratch", None), loss_acc=self._loss)
            return self._loss
        if self.optimizer in ("sgd", "sgd_fused") and self.tables16 is not None:     # (bf16 forward reads the shadow tables: no in-launch race either way)
            ops.bpr_step_bf16(self.tables16["user_embedding"], self.tables16["item_embedding"], users, pos, neg, pos_pop, neg_pop, regs=self.decay,
                              reg_div=self.batch_size, lr=self.lr, mode=ops.UPD_SGD_FUSED, U_master=U, I_master=I, loss_acc=self._loss)
            return self._loss
        if self.optimizer == "sgd_fused":
            ops.bpr_step(U, I, users, pos, neg, pos_pop, neg_pop, regs=self.decay, reg_div=self.batch_size, lr=self.lr,
                         mode=ops.UPD_SGD_FUSED, loss_acc=self._loss, users_distinct=bool(getattr(self, "users_distinct", False)))
            return self._loss
        if self.optimizer == "sgd":
            sc = getattr(self, "_sgd_scratch", None)
            if sc is not None and sc[0].shape[0] != users.numel():
                sc = None
            self._sgd_scratch = ops.sgd_step_exact(U, I, users, pos, neg, pos_pop, neg_pop, regs=self.decay, reg_div=self.batch_size,
                                                   lr=self.lr, loss_acc=self._loss, scratch=sc)
            return self._loss
        return self._adam_step(U, I, users, pos, neg, pos_pop, neg_pop, plan)

    def _adam_step(self, U, I, users, pos, neg, pos_pop, neg_pop, plan):
        """One step of `adam` / `lazy_adam`: [replay: the batch's rows up to step t - 1] -> the batch's gradient summed into gU / gI -> the update
        [-> bf16 tables: the rows that moved are re-rounded into the shadows].  plan: the batch's plan under --deterministic, unused otherwise.
        An embed_size the kernels do not have is refused by the first library call (PdaHipError), before any table is written."""
        st = self._opt_state()
        self._t += 1
        lr_t = ops.adam_lr_t(self.lr, self._t)
        state = (U, st["mU"], st["vU"], st["gU"], I, st["mI"], st["vI"], st["gI"])
        batch = (users, pos, neg, pos_pop, neg_pop)
        kw = dict(regs=self.decay, reg_div=self.batch_size, loss_acc=self._loss)
        replay = self.optimizer == "adam" and self.adam_exact_lazy
        sweep = self.optimizer == "adam" and not replay
        if sweep and self.tables16 is None:
            # the reference's step fused (round 6): gradients + row tags, then the tagged sweep (cache policy by working set)
            if "tagU" not in st:
                st["tagU"], st["tagI"] = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
            tagged = (U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"])
            if self.deterministic:
                self._plan_scratch = ops.adam_step_plan(*tagged, *batch, step=self._t, lr_t=lr_t, plan=plan, scratch=getattr(self, "_plan_scratch", None), **kw)
            else:
                ops.adam_step(*tagged, *batch, step=self._t, lr_t=lr_t, users_distinct=bool(getattr(self, "users_distinct", False)), **kw)
            return self._loss
        if replay:          # the batch rows up to step t - 1: the forward pass reads them
            ops.adam_lazy(0, self._lazy_state(), *state, users, pos, neg, self._t)
            self._refresh16((users,), (pos, neg))
        if self.tables16 is not None:
            ops.bpr_step_bf16(self.tables16["user_embedding"], self.tables16["item_embedding"], *batch, mode=ops.UPD_DENSE_GRAD, gU=st["gU"], gI=st["gI"], **kw)
        elif self.deterministic:
            self._plan_scratch = ops.bpr_grad_plan(U, I, *batch, plan=plan, gU=st["gU"], gI=st["gI"], scratch=getattr(self, "_plan_scratch", None), **kw)
        else:
            ops.bpr_step(U, I, *batch, mode=ops.UPD_DENSE_GRAD, gU=st["gU"], gI=st["gI"], **kw)
        if replay:
            ops.adam_lazy(1, self._lazy, *state, users, pos, neg, self._t)
            self._refresh16((users,), (pos, neg))
        elif sweep:         # TF-1.14's dense-decay Adam on both tables in six streams: the gradient tables are read only on the batch's rows
            if "tU" not in st:
                st["tU"], st["tI"] = ops.adam_touched_bitmaps(U.shape[0], I.shape[0], U.device)
            ops.adam_mark_rows(users, pos, neg, st["tU"], st["tI"])
            ops.adam_dense_sweep3(U, st["mU"], st["vU"], st["gU"], st["tU"], I, st["mI"], st["vI"], st["gI"], st["tI"], lr_t)
            self._refresh16((None,), (None,))                   # dense decay moves every row
        else:               # lazy_adam
            ru, ri = torch.unique(users).int(), torch.unique(torch.cat([pos, neg])).int()
            ops.adam_rows(U, st["mU"], st["vU"], st["gU"], ru, lr_t)
            ops.adam_rows(I, st["mI"], st["vI"], st["gI"], ri, lr_t)
            self._refresh16((ru,), (ri,))
        return self._loss

    def _refresh16(self, user_rows, item_rows):
        """bf16 tables: re-round the given rows of the masters into the shadow tables (None: the whole table).  Nothing to do for fp32 tables."""
        if self.tables16 is None:
            return
        for rows in user_rows:
            ops.refresh_rows_bf16(self.weights["user_embedding"], self.tables16["user_embedding"], rows)
        for rows in item_rows:
            ops.refresh_rows_bf16(self.weights["item_embedding"], self.tables16["item_embedding"], rows)

    # ---- checkpoint (tf.train.Saver stand-in, MF/train_new_api.py:1014,1218-1228) ---------------------
    CKPT_FORMAT = "pda_amd/2"     # torch.save pickle of this dict -- NOT a tf.train.Saver checkpoint (see README)

    def state_dict(self):
        self.sync_optimizer()
        sd = {"format": self.CKPT_FORMAT, "embed_size": self.emb_dim, "n_users": self.n_users, "n_items": self.n_items,
              "optimizer": self.optimizer, "table_dtype": self.table_dtype,
              "user_embedding": self.weights["user_embedding"], "item_embedding": self.weights["item_embedding"],
              "adam_t": self._t}
        if self._state is not None:
            sd.update({k: v for k, v in self._state.items() if k[0] in "mv"})
        return sd

    def load_state_dict(self, sd):
        """Validates what the checkpoint was written for before touching the tables.  Files keep the reference's NAMES
        (best_ckpt.ckpt ...) but are torch pickles: a TF checkpoint of the reference cannot be read here, nor the reverse."""
        if not isinstance(sd, dict) or "user_embedding" not in sd:
            raise ValueError("not a pda_amd checkpoint (a tf.train.Saver checkpoint of the reference cannot be loaded)")
        if sd.get("model", "mf") != "mf":
            raise ValueError("checkpoint of a %s model cannot be loaded into %s" % (sd["model"], type(self).__name__))
        for key, mine in (("embed_size", self.emb_dim), ("n_users", self.n_users), ("n_items", self.n_items)):
            if key in sd and int(sd[key]) != int(mine):
                raise ValueError("checkpoint %s = %s, model has %s" % (key, sd[key], mine))
        if sd.get("table_dtype", self.table_dtype) != self.table_dtype:
            raise ValueError("checkpoint written with table_dtype=%s, model runs %s" % (sd["table_dtype"], self.table_dtype))
        if sd.get("optimizer", self.optimizer) != self.optimizer and ("mU" in sd) != (self.optimizer in ("adam", "lazy_adam")):
            raise ValueError("checkpoint written with optimizer=%s (Adam state %s), model runs %s" %
                             (sd["optimizer"], "present" if "mU" in sd else "absent", self.optimizer))
        if tuple(sd["user_embedding"].shape) != tuple(self.weights["user_embedding"].shape) or \
                tuple(sd["item_embedding"].shape) != tuple(self.weights["item_embedding"].shape):
            raise ValueError("checkpoint tables do not have the model's shape")
        self.weights["user_embedding"].copy_(sd["user_embedding"])
        self.weights["item_embedding"].copy_(sd["item_embedding"])
        if self.tables16 is not None:
            for k in self.tables16:
                ops.refresh_rows_bf16(self.weights[k], self.tables16[k])
        self._t = int(sd.get("adam_t", 0))
        self._lazy = None                     # (a checkpoint holds synced tables: every row is current for adam_t)
        if "mU" in sd:
            st = self._opt_state()
            for k in ("mU", "vU", "mI", "vI"):
                st[k].copy_(sd[k])


class BPRMF(_MFBase):
    """BPRMF.  Fetchables: opt, loss, mf_loss, reg_loss, batch_ratings  (MF/model_api.py:459-471)."""
    with_pop = False

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None,
                 neg_items_api=None, **kw):
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.opt, self.loss = Fetch(self, "opt"), Fetch(self, "loss")
        self.mf_loss, self.reg_loss = Fetch(self, "mf_loss"), Fetch(self, "reg_loss")
        self.batch_ratings = Fetch(self, "batch_ratings")


class ConditionalBPRMF(_MFBase):
    """PD/PDA.  Fetchables: opt_pop_global, loss_pop_global, mf_loss_pop_global, reg_loss_pop_global,
    batch_ratings, condition_ratings  (MF/model_api.py:62,81-83,113)."""
    with_pop = True

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None,
                 neg_items_api=None, pos_pop_api=None, neg_pop_api=None, **kw):
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api,
                         pos_pop_api, neg_pop_api, **kw)
        self.opt_pop_global, self.loss_pop_global = Fetch(self, "opt"), Fetch(self, "loss")
        self.mf_loss_pop_global, self.reg_loss_pop_global = Fetch(self, "mf_loss"), Fetch(self, "reg_loss")
        self.batch_ratings = Fetch(self, "batch_ratings")
        self.condition_ratings = Fetch(self, "condition_ratings")


class BPRMFTempPop(_MFBase):
    """BPRMF(t)-pop (MF/model_api.py:300-416).  Fetchables: opt, loss, mf_loss, reg_loss, batch_ratings.

    weights: user_embedding [n_users, d], item_embedding [n_items, d], user_temp_bias [n_users, 1], item_temp_init_bias [n_items, T + 1]
    (column t < T: the bias of time slot t, column T: the init bias), all Xavier-uniform, drawn in this order.  A step is
    pda_temp_pop_adam_step_f32: the gradients of the four tables, then TF-1.14's dense-decay Adam over all of them ("BPRMF(t)-pop",
    for the two quirks of the reference this keeps: the user bias trains on stage-0 triplets only, and one alpha per 2 048-user block)."""
    with_pop = False

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, temp_api=None,
                 raw_api=None, **kw):
        if int(getattr(args, "deterministic", 0) or 0):
            check_deterministic(args, data_config)
        if torch.device(kw.get("device") or "cuda").type != "cuda":
            raise NotImplementedError("temp_pop runs on the GPU kernels only (pda_amd has no CPU path)")
        self.temp_num = int(data_config["temp_num"])
        if self.temp_num < 1:
            raise ValueError("temp_pop needs at least one time slot (temp_num >= 1)")
        if getattr(args, "optimizer", "adam") != "adam":
            raise NotImplementedError("temp_pop runs the reference's Adam only (--optimizer adam)")
        if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep") or getattr(args, "adam_exact_lazy", None):
            raise NotImplementedError("temp_pop runs the dense Adam sweep only (--adam_sweep auto | sweep)")
        if getattr(args, "table_dtype", "f32") != "f32":
            raise NotImplementedError("temp_pop runs fp32 tables only (--table_dtype f32)")
        if int(getattr(args, "gpus", 1) or 1) > 1:
            raise NotImplementedError("temp_pop runs on one GPU")
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        if self.emb_dim not in (64, 128, 256):
            raise NotImplementedError("temp_pop: embed_size 64 / 128 / 256 (the bias-head score kernels)")
        self.adam_exact_lazy = False
        self._tp = None
        self.opt, self.loss = Fetch(self, "opt"), Fetch(self, "loss")
        self.mf_loss, self.reg_loss = Fetch(self, "mf_loss"), Fetch(self, "reg_loss")
        self.batch_ratings = Fetch(self, "batch_ratings")

    def init_weights(self, gen):
        w = super().init_weights(gen)
        w["user_temp_bias"] = xavier_uniform_(torch.empty(self.n_users, 1, device=self.device), gen)
        w["item_temp_init_bias"] = xavier_uniform_(torch.empty(self.n_items, self.temp_num + 1, device=self.device), gen)
        return w

    def _tables(self):
        w = self.weights
        return w["user_embedding"], w["item_embedding"], w["user_temp_bias"], w["item_temp_init_bias"]

    def _tp_state(self):
        if self._tp is None:
            self._tp = ops.TempPopState(*self._tables())
        return self._tp

    def item_beta(self) -> torch.Tensor:
        """beta_i = fl(C[i, T-1] + C[i, T]): the most recent stage plus the init column (:390-393), float32 [n_items]."""
        C = self.weights["item_temp_init_bias"]
        return (C[:, self.temp_num - 1] + C[:, self.temp_num]).contiguous()

    def user_alpha(self, first_users: torch.Tensor) -> torch.Tensor:
        """alpha = fl(1 + bu[u]) for the given users (the first user of each user's evaluation block: quirk 2), float32."""
        bu = self.weights["user_temp_bias"].view(-1)
        return (bu.index_select(0, first_users.long()) + 1.0).contiguous()

    def train_step(self, users, pos, neg, temps=None, raw=None, plan=None) -> torch.Tensor:
        """One BPRMF(t)-pop step.  temps: float32 (or integer) time slot of each positive; raw (= arange(B) in the reference) is not needed.
        Returns the float32[3] device tensor (loss, mf_loss, reg_loss) of this step, as the other models do."""
        if temps is None:
            raise ValueError("temp_pop needs the time slot of every positive (temps)")
        if not temps.dtype == torch.float32:
            temps = temps.to(torch.float32)
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._tp_state()
        self._t += 1
        ops.temp_pop_adam_step(*self._tables(), users, pos, neg, temps.contiguous(), st, regs=self.decay, reg_div=self.batch_size, step=self._t,
                               lr_t=ops.adam_lr_t(self.lr, self._t), loss_acc=self._loss)
        return self._loss

    CKPT_MOMENTS = ("mU", "mI", "mbu", "mC"), ("vU", "vI", "vbu", "vC")

    def state_dict(self):
        U, I, bu, C = self._tables()
        sd = {"format": self.CKPT_FORMAT, "model": "temp_pop", "embed_size": self.emb_dim, "n_users": self.n_users, "n_items": self.n_items,
              "temp_num": self.temp_num, "optimizer": self.optimizer, "table_dtype": self.table_dtype, "user_embedding": U, "item_embedding": I,
              "user_temp_bias": bu, "item_temp_init_bias": C, "adam_t": self._t}
        if self._tp is not None:
            for names, tabs in zip(self.CKPT_MOMENTS, (self._tp.m, self._tp.v)):
                sd.update(dict(zip(names, tabs)))
        return sd

    def load_state_dict(self, sd):
        if not isinstance(sd, dict) or "user_embedding" not in sd:
            raise ValueError("not a pda_amd checkpoint (a tf.train.Saver checkpoint of the reference cannot be loaded)")
        if sd.get("model", "mf") != "temp_pop":
            raise ValueError("checkpoint of a %s model cannot be loaded into BPRMFTempPop" % sd.get("model", "mf"))
        for key, mine in (("embed_size", self.emb_dim), ("n_users", self.n_users), ("n_items", self.n_items), ("temp_num", self.temp_num)):
            if int(sd[key]) != int(mine):
                raise ValueError("checkpoint %s = %s, model has %s" % (key, sd[key], mine))
        for k, t in zip(("user_embedding", "item_embedding", "user_temp_bias", "item_temp_init_bias"), self._tables()):
            if tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError("checkpoint table %s does not have the model's shape" % k)
            t.copy_(sd[k])
        self._t = int(sd.get("adam_t", 0))
        if "mU" in sd:
            st = self._tp_state()
            for names, tabs in zip(self.CKPT_MOMENTS, (st.m, st.v)):
                for n, t in zip(names, tabs):
                    t.copy_(sd[n])


DICE_EMBED_SIZES = ops.DICE_EMBED_SIZES   # --embed_size of a DICE model: the width of EACH of its two embeddings (rows of 64 / 128 / 256 floats)


def check_dice(args):
    """--train dice: refuse, before anything is built, what DICE has no kernel for.  Every message names its flag."""
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--deterministic 1: --train dice sums its gradients with float atomics (no planned gradient)")
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train dice runs fp32 tables only" % args.table_dtype)
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--optimizer %s: --train dice runs the reference's dense-decay Adam only (--optimizer adam)" % args.optimizer)
    if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep") or getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("--adam_sweep %s: --train dice runs the dense Adam sweep only (auto | sweep)" % getattr(args, "adam_sweep", "auto"))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train dice trains on one GPU" % args.gpus)
    if getattr(args, "dice_dis_loss", "l1") not in ("l1", "l2"):
        raise NotImplementedError("--dice_dis_loss %s: l1 | l2 (dcor is not implemented)" % args.dice_dis_loss)
    if int(args.embed_size) not in DICE_EMBED_SIZES:
        raise ValueError("--train dice: --embed_size is the width of each of the two embeddings and must be one of %s, got %s"
                         % (DICE_EMBED_SIZES, args.embed_size))
    for flag in ("dice_int_weight", "dice_con_weight", "dice_dis_pen", "dice_margin"):
        if not float(getattr(args, flag, 0.0)) >= 0.0:
            raise ValueError("--%s must be >= 0" % flag)
    for flag in ("dice_margin_decay", "dice_loss_decay"):
        if not 0.0 < float(getattr(args, flag, 0.9)) <= 1.0:
            raise ValueError("--%s must lie in (0, 1]" % flag)


class DICE(_MFBase):
    """DICE (Zheng et al., WWW'21).  Fetchables: opt, loss, mf_loss, reg_loss, batch_ratings.

    weights: user_embedding [n_users, 2d], item_embedding [n_items, 2d]; columns [0, d) are the interest embedding, [d, 2d) the conformity
    embedding, d = --embed_size.  Each [n, d] half is Xavier-uniform like a [n, d] table of the other models, drawn in the order user interest,
    user conformity, item interest, item conformity.  The click score s_int + s_con is the dot of two rows: score_tables() hands the 2d-wide
    tables to every evaluation path as they are.  A step is pda_dice_adam_step_f32; the loss weights follow DICE's schedule (start_epoch)."""
    with_pop = False
    LOSS_TERMS = 6           # a step's loss row: loss, mf_loss, reg_loss, L_int, L_con, L_dis

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_dice(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.adam_exact_lazy = False
        self.w_int = float(getattr(args, "dice_int_weight", 0.1))
        self.w_con = float(getattr(args, "dice_con_weight", 0.1))
        self.dis_pen = float(getattr(args, "dice_dis_pen", 0.01))
        self.dis_loss = getattr(args, "dice_dis_loss", "l1")
        self.loss_decay = float(getattr(args, "dice_loss_decay", 0.9))
        self.margin = float(getattr(args, "dice_margin", 40.0))       # the sampler's current margin, kept for the checkpoint (start_epoch)
        self._dice = None
        self._loss_ring = torch.zeros((16, self.LOSS_TERMS), dtype=torch.float32, device=self.device)
        self._loss = self._loss_ring[0]
        self.epoch_terms = None                                       # float64 [6]: the sums of the last finished epoch's loss rows
        self.opt, self.loss = Fetch(self, "opt"), Fetch(self, "loss")
        self.mf_loss, self.reg_loss = Fetch(self, "mf_loss"), Fetch(self, "reg_loss")
        self.batch_ratings = Fetch(self, "batch_ratings")

    def init_weights(self, gen):
        d = self.emb_dim

        def table(n):
            a = xavier_uniform_(torch.empty(n, d, device=self.device), gen)
            b = xavier_uniform_(torch.empty(n, d, device=self.device), gen)
            return torch.cat([a, b], dim=1).contiguous()
        return {"user_embedding": table(self.n_users), "item_embedding": table(self.n_items)}

    def _dice_state(self):
        if self._dice is None:
            self._dice = ops.DiceState(self.weights["user_embedding"], self.weights["item_embedding"])
        return self._dice

    def start_epoch(self, epoch: int, margin=None):
        """DICE's schedule: at the start of every epoch after the first, w_int and w_con are multiplied by --dice_loss_decay.  margin: the
        sampler's margin for this epoch (the sampler owns that half of the schedule); recorded for the checkpoint."""
        if epoch > 0:
            self.w_int *= self.loss_decay
            self.w_con *= self.loss_decay
        if margin is not None:
            self.margin = float(margin)

    def start_loss_rows(self, n_steps: int):
        self._loss_rows = torch.zeros((max(1, int(n_steps)), self.LOSS_TERMS), dtype=torch.float32, device=self.device)
        self._loss_row_i = 0

    def finish_loss_rows(self) -> torch.Tensor:
        """The trainer's (loss, mf_loss, reg_loss) sums; all six terms of the epoch stay in epoch_terms."""
        rows, n = self._loss_rows, self._loss_row_i
        self._loss_rows = None
        self.epoch_terms = rows[:n].double().sum(0)
        return self.epoch_terms[:3]

    def train_step(self, users, pos, neg, mask=None, plan=None) -> torch.Tensor:
        """One DICE step.  mask: 1 where the negative is the more popular item (PNSM), uint8 (bool and integer tensors are converted).
        Returns the float32 [6] device tensor (loss, mf_loss, reg_loss, L_int, L_con, L_dis) of this step: mf_loss is everything except
        reg_loss, so loss = mf_loss + reg_loss as for the other models."""
        if mask is None:
            raise ValueError("dice needs the mask of every triplet (1: the negative is the more popular item)")
        if mask.dtype != torch.uint8:
            mask = mask.to(torch.uint8)
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._dice_state()
        self._t += 1
        ops.dice_adam_step(self.weights["user_embedding"], self.weights["item_embedding"], users, pos, neg, mask.contiguous(), st,
                           w_int=self.w_int, w_con=self.w_con, dis_pen=self.dis_pen, dis_loss=self.dis_loss, regs=self.decay,
                           reg_div=self.batch_size, step=self._t, lr_t=ops.adam_lr_t(self.lr, self._t), loss_acc=self._loss)
        return self._loss

    def state_dict(self):
        sd = {"format": self.CKPT_FORMAT, "model": "dice", "embed_size": self.emb_dim, "n_users": self.n_users, "n_items": self.n_items,
              "optimizer": self.optimizer, "table_dtype": self.table_dtype, "user_embedding": self.weights["user_embedding"],
              "item_embedding": self.weights["item_embedding"], "adam_t": self._t, "dice_margin": self.margin, "dice_int_weight": self.w_int,
              "dice_con_weight": self.w_con}
        if self._dice is not None:
            sd.update({k: getattr(self._dice, k) for k in ("mU", "vU", "mI", "vI")})
        return sd

    def load_state_dict(self, sd):
        if not isinstance(sd, dict) or "user_embedding" not in sd:
            raise ValueError("not a pda_amd checkpoint (a tf.train.Saver checkpoint of the reference cannot be loaded)")
        if sd.get("format") != self.CKPT_FORMAT:
            raise ValueError("checkpoint format %r, DICE reads %s" % (sd.get("format"), self.CKPT_FORMAT))
        if sd.get("model", "mf") != "dice":
            raise ValueError("checkpoint of a %s model cannot be loaded into DICE" % sd.get("model", "mf"))
        for key, mine in (("embed_size", self.emb_dim), ("n_users", self.n_users), ("n_items", self.n_items)):
            if int(sd[key]) != int(mine):
                raise ValueError("checkpoint %s = %s, model has %s" % (key, sd[key], mine))
        for k in ("user_embedding", "item_embedding"):
            if tuple(sd[k].shape) != tuple(self.weights[k].shape):
                raise ValueError("checkpoint table %s does not have the model's shape" % k)
        for k in ("user_embedding", "item_embedding"):
            self.weights[k].copy_(sd[k])
        self._t = int(sd.get("adam_t", 0))
        self.margin = float(sd.get("dice_margin", self.margin))
        self.w_int = float(sd.get("dice_int_weight", self.w_int))
        self.w_con = float(sd.get("dice_con_weight", self.w_con))
        # a fresh state: the row tags of the steps run so far must not meet the step numbers that follow adam_t (a row whose tag equals
        # the step's is not listed, and would miss its L_dis gradient); the gradient tables are zero between steps anyway
        self._dice = None
        if "mU" in sd:
            st = self._dice_state()
            for k in ("mU", "vU", "mI", "vI"):
                getattr(st, k).copy_(sd[k])


def ips_item_counts(train_user_list, n_items: int):
    """The train interactions of every item, int64 numpy [n_items], from the loader's {user: [items]} lists: what the propensities are built from."""
    import numpy as np
    counts = np.zeros(int(n_items), dtype=np.int64)
    for items in train_user_list.values():
        if len(items):
            counts += np.bincount(np.asarray(items, dtype=np.int64), minlength=int(n_items))
    return counts


def check_ips(args):
    """--train ips: refuse, before anything is built, what the IPS step has no kernel for.  Every message names its flag."""
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--deterministic 1: --train ips sums its gradients with float atomics (no planned gradient)")
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train ips runs fp32 tables only" % args.table_dtype)
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--optimizer %s: --train ips runs the reference's dense-decay Adam only (--optimizer adam)" % args.optimizer)
    if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep") or getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("--adam_sweep %s: --train ips runs the dense Adam sweep only (auto | sweep)" % getattr(args, "adam_sweep", "auto"))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train ips trains on one GPU" % args.gpus)
    if not float(getattr(args, "ips_clip", 0.0)) >= 0.0:
        raise ValueError("--ips_clip must be >= 0 (0: no clip), got %s" % args.ips_clip)
    if getattr(args, "ips_norm", 0) not in (0, 1):
        raise ValueError("--ips_norm must be 0 or 1, got %s" % args.ips_norm)


class IPSBPRMF(BPRMF):
    """BPR-MF trained with inverse propensity scoring: IPS, IPS-C (--ips_clip C) and IPS-CN (--ips_clip C --ips_norm 1).
    Fetchables, tables, evaluation and checkpoint are those of BPRMF -- the two differ only in how they were trained; a step is
    pda_ips_adam_step_f32.  data_config["ips_item_counts"] (or set_item_counts): the train interactions per item the weights are built from;
    a model that is only restored and evaluated needs none."""

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_ips(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.adam_exact_lazy = False
        self.ips_clip = float(getattr(args, "ips_clip", 0.0))
        self.ips_norm = int(getattr(args, "ips_norm", 0))
        self.ips = None
        self._wsum = None
        if data_config.get("ips_item_counts") is not None:
            self.set_item_counts(data_config["ips_item_counts"])

    def set_item_counts(self, counts):
        if len(counts) != self.n_items:
            raise ValueError("ips_item_counts holds one number per item (%d), got %d" % (self.n_items, len(counts)))
        self.ips = ops.IpsWeights.from_counts(counts, self.ips_clip, self.device)

    def train_step(self, users, pos, neg, pos_pop=None, neg_pop=None, plan=None) -> torch.Tensor:
        """One IPS step; returns the float32 [3] device tensor (loss, mf_loss, reg_loss) of this step, as BPRMF.train_step does."""
        if self.ips is None:
            raise ValueError("IPSBPRMF needs the train interactions per item before it trains (data_config['ips_item_counts'] or set_item_counts)")
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._opt_state()
        if "tagU" not in st:
            st["tagU"], st["tagI"] = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
        if self.ips_norm and self._wsum is None:
            self._wsum = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._t += 1
        ops.ips_adam_step(U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"], users, pos, neg, self.ips.ipw,
                          wsum=self._wsum if self.ips_norm else None, regs=self.decay, reg_div=self.batch_size, step=self._t,
                          lr_t=ops.adam_lr_t(self.lr, self._t), users_distinct=bool(getattr(self, "users_distinct", False)), loss_acc=self._loss)
        return self._loss

    def state_dict(self):
        sd = super().state_dict()
        sd.update(ips_clip=self.ips_clip, ips_norm=self.ips_norm)
        return sd


def check_warp(args):
    """--train warp: refuse, before anything is built, what the WARP sampler and step have no path for.  Every message names its flag.  The
    sampler scores its candidates on the live fp32 tables of a BPRMF right before the step that trains on them (check_dns has the reasons)."""
    if getattr(args, "model", "mf") != "mf":
        raise NotImplementedError("--model %s: --train warp scores candidates on the embedding tables themselves, a LightGCN's scores live on the "
                                  "propagated tables (--model mf)" % (args.model,))
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--deterministic 1: --train warp sums its gradients with float atomics (no planned gradient; the draw alone is "
                                  "bit-reproducible)")
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train warp scores and trains fp32 tables only" % (args.table_dtype,))
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--optimizer %s: --train warp runs the reference's dense-decay Adam only (--optimizer adam)" % (args.optimizer,))
    if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep"):
        raise NotImplementedError("--adam_sweep %s: --train warp reads whole tables before every step, a replayed table's idle rows are stale then "
                                  "(--adam_sweep auto | sweep)" % (args.adam_sweep,))
    if getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("adam_exact_lazy: --train warp reads whole tables before every step, a lazy table's idle rows are stale then")
    if getattr(args, "sampler", "device") != "device":
        raise NotImplementedError("--sampler %s: --train warp draws and scores its candidates with the device sampler only (--sampler device)"
                                  % (args.sampler,))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train warp trains on one GPU (no item shards)" % (args.gpus,))
    if getattr(args, "neg_sampler", "uniform") != "uniform":
        raise NotImplementedError("--neg_sampler %s: --train warp draws its own negatives, the first violator among uniform candidates "
                                  "(--neg_sampler uniform)" % (args.neg_sampler,))
    if getattr(args, "test", "normal") not in ("normal", "warp"):
        raise NotImplementedError("--test %s: --train warp goes with --test normal (the raw head and the gamma search of a BPRMF) or --test warp"
                                  % (args.test,))
    margin = getattr(args, "warp_margin", 1.0)
    if not math.isfinite(float(margin)):
        raise ValueError("--warp_margin must be a finite number, got %s" % (margin,))
    T = getattr(args, "warp_max_trials", 64)
    if int(T) != T or not 1 <= int(T) <= ops.WARP_MAX_TRIALS:
        raise ValueError("--warp_max_trials must be an integer in 1 .. %d, got %s" % (ops.WARP_MAX_TRIALS, T))
    if getattr(args, "warp_weight", "harmonic") not in ops.WARP_WEIGHT_KINDS:
        raise ValueError("--warp_weight must be harmonic, log or none, got %s" % (args.warp_weight,))


class WARPBPRMF(BPRMF):
    """BPR-MF trained with the WARP loss: the hinge margin - (u.p - u.n) on the first of --warp_max_trials uniform candidates that
    violates --warp_margin, weighted by the rank estimate of --warp_weight.  Fetchables, tables, evaluation and checkpoint are those of BPRMF --
    the two differ only in how they were trained; a step is pda_warp_adam_step_f32 on the (users, pos, neg, coef) batches of
    DeviceSampler(mode="warp")."""

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_warp(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.adam_exact_lazy = False
        self.warp_margin = float(getattr(args, "warp_margin", 1.0))
        self.warp_max_trials = int(getattr(args, "warp_max_trials", 64))
        self.warp_weight = getattr(args, "warp_weight", "harmonic")

    def train_step(self, users, pos, neg, coef=None, neg_pop=None, plan=None) -> torch.Tensor:
        """One WARP step; returns the float32 [3] device tensor (loss, mf_loss, reg_loss) of this step, as BPRMF.train_step does."""
        if coef is None or neg_pop is not None:
            raise ValueError("WARPBPRMF trains on (users, pos, neg, coef) batches: the coefficient column of DeviceSampler(mode='warp')")
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._opt_state()
        if "tagU" not in st:
            st["tagU"], st["tagI"] = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
        self._t += 1
        ops.warp_adam_step(U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"], users, pos, neg, coef,
                           margin=self.warp_margin, regs=self.decay, reg_div=self.batch_size, step=self._t,
                           lr_t=ops.adam_lr_t(self.lr, self._t), users_distinct=bool(getattr(self, "users_distinct", False)), loss_acc=self._loss)
        return self._loss

    def state_dict(self):
        sd = super().state_dict()
        sd.update(warp_margin=self.warp_margin, warp_max_trials=self.warp_max_trials, warp_weight=self.warp_weight)
        return sd


def check_pcc(args):
    """--train pcc: refuse, before anything is built, what the popularity-correlation step has no kernel for.  Every message names its flag."""
    if getattr(args, "model", "mf") == "lightgcn":
        raise NotImplementedError("--model lightgcn: --train pcc trains the tables of a BPRMF only (--model mf)")
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--deterministic 1: --train pcc sums its gradients with float atomics (no planned gradient; the batch statistic "
                                  "alone is bit-reproducible)")
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train pcc runs fp32 tables only" % args.table_dtype)
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--optimizer %s: --train pcc runs the reference's dense-decay Adam only (--optimizer adam)" % args.optimizer)
    if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep") or getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("--adam_sweep %s: --train pcc runs the dense Adam sweep only (auto | sweep)" % getattr(args, "adam_sweep", "auto"))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train pcc trains on one GPU (the statistic is the whole batch's)" % args.gpus)
    gamma = getattr(args, "pcc_gamma", 1.0)
    if not (float(gamma) >= 0.0 and math.isfinite(float(gamma))):
        raise ValueError("--pcc_gamma must be a finite number >= 0, got %s" % (gamma,))
    if getattr(args, "pcc_on", "pos") not in ops.PCC_ON:
        raise ValueError("--pcc_on must be pos or margin, got %s" % (args.pcc_on,))
    if getattr(args, "pcc_pop", "count") not in ops.PCC_POP_MODES:
        raise ValueError("--pcc_pop must be count or log, got %s" % (args.pcc_pop,))


class PCCBPRMF(BPRMF):
    """BPR-MF trained with the popularity-correlation regulariser: the BPR loss plus --pcc_gamma times the squared Pearson
    correlation, over the batch, between a score (--pcc_on pos: of the observed pair; margin: the pairwise margin) and the popularity of the
    positive (--pcc_pop count | log).  Fetchables, tables, evaluation and checkpoint are those of BPRMF -- the two differ only in how they were
    trained; a step is pda_pcc_adam_step_f32.  data_config["ips_item_counts"] (or set_item_counts): the train interactions per item the
    popularities are built from; a model that is only restored and evaluated needs none."""

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_pcc(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.adam_exact_lazy = False
        self.pcc_gamma = float(getattr(args, "pcc_gamma", 1.0))
        self.pcc_on = getattr(args, "pcc_on", "pos")
        self.pcc_pop = getattr(args, "pcc_pop", "count")
        self.pcc = None
        self._pcc_ws = None
        self.pcc_acc = torch.zeros(2, dtype=torch.float32, device=self.device)     # += (r, r^2) of every step; take_pcc reads and clears it
        self._pcc_steps = 0
        if data_config.get("ips_item_counts") is not None:
            self.set_item_counts(data_config["ips_item_counts"])

    def set_item_counts(self, counts):
        if len(counts) != self.n_items:
            raise ValueError("ips_item_counts holds one number per item (%d), got %d" % (self.n_items, len(counts)))
        self.pcc = ops.PccPop.from_counts(counts, self.pcc_pop, self.device)

    def train_step(self, users, pos, neg, pos_pop=None, neg_pop=None, plan=None) -> torch.Tensor:
        """One PCC step; returns the float32 [3] device tensor (loss, mf_loss, reg_loss) of this step, as BPRMF.train_step does."""
        if self.pcc is None:
            raise ValueError("PCCBPRMF needs the train interactions per item before it trains (data_config['ips_item_counts'] or set_item_counts)")
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._opt_state()
        if "tagU" not in st:
            st["tagU"], st["tagI"] = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
        if self._pcc_ws is None or self._pcc_ws[0].numel() < users.numel():
            self._pcc_ws = ops.pcc_workspace(users.numel(), self.device)
        self._t += 1
        ops.pcc_adam_step(U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"], users, pos, neg, self.pcc.pop,
                          self._pcc_ws[0], self._pcc_ws[1], gamma=self.pcc_gamma, on=self.pcc_on, regs=self.decay, reg_div=self.batch_size,
                          step=self._t, lr_t=ops.adam_lr_t(self.lr, self._t), users_distinct=bool(getattr(self, "users_distinct", False)),
                          loss_acc=self._loss, pcc_acc=self.pcc_acc)
        self._pcc_steps += 1
        return self._loss

    def take_pcc(self):
        """(mean r, mean r^2) over the steps since the last call (one host read), and a fresh count."""
        r, r2 = (self.pcc_acc.double() / max(self._pcc_steps, 1)).tolist()
        self.pcc_acc.zero_()
        self._pcc_steps = 0
        return r, r2

    def state_dict(self):
        sd = super().state_dict()
        sd.update(pcc_gamma=self.pcc_gamma, pcc_on=self.pcc_on, pcc_pop=self.pcc_pop)
        return sd


def check_ssm(args):
    """--train ssm: refuse, before anything is built, what the sampled-softmax step has no kernel for.  Every message names its flag."""
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--deterministic 1: --train ssm sums its gradients with float atomics (no planned gradient)")
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train ssm runs fp32 tables only" % args.table_dtype)
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--optimizer %s: --train ssm runs the reference's dense-decay Adam only (--optimizer adam)" % args.optimizer)
    if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep") or getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("--adam_sweep %s: --train ssm runs the dense Adam sweep only (auto | sweep)" % getattr(args, "adam_sweep", "auto"))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train ssm trains on one GPU (no item shards)" % args.gpus)
    if getattr(args, "sampler", "device") != "device":
        raise NotImplementedError("--sampler %s: --train ssm draws its [B, N] negatives with the device sampler only (--sampler device)" % args.sampler)
    n = getattr(args, "ssm_negs", 64)
    if int(n) != n or not 1 <= int(n) <= ops.SSM_MAX_NEGS:
        raise ValueError("--ssm_negs must be an integer in 1 .. %d, got %s" % (ops.SSM_MAX_NEGS, n))
    tau = float(getattr(args, "ssm_tau", 0.1))
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError("--ssm_tau must be a finite number > 0, got %s" % args.ssm_tau)
    if getattr(args, "ssm_norm", 1) not in (0, 1):
        raise ValueError("--ssm_norm must be 0 or 1, got %s" % args.ssm_norm)
    source = getattr(args, "ssm_source", "sampled")
    if source not in ("sampled", "batch", "all"):
        raise ValueError("--ssm_source must be sampled, batch or all, got %s" % (source,))
    for flag in ("ssm_logq", "ssm_mask_train"):
        if getattr(args, flag, 1) not in (0, 1):
            raise ValueError("--%s must be 0 or 1, got %s" % (flag, getattr(args, flag)))
    if source == "batch":
        B = getattr(args, "batch_size", 2048)
        if int(B) != B or not 2 <= int(B) <= ops.INBATCH_MAX_B:
            raise ValueError("--batch_size must be an integer in 2 .. %d with --ssm_source batch (a row's negatives are the other rows' "
                             "positives), got %s" % (ops.INBATCH_MAX_B, B))
    if source == "all":
        B = getattr(args, "batch_size", 2048)
        if int(B) != B or not 1 <= int(B) <= ops.FULLSM_MAX_B:
            raise ValueError("--batch_size must be an integer in 1 .. %d with --ssm_source all, got %s" % (ops.FULLSM_MAX_B, B))


def check_dns(args):
    """--neg_sampler dns: refuse, before anything is built, what dynamic negative sampling has no path for.  Every message names its flag.
    The sampler scores its candidates on the live fp32 tables of a BPRMF / PD model right before the step that trains on them."""
    mode = getattr(args, "neg_sampler", "uniform")
    if mode in ("uniform", "pop"):      # (pop: check_negpop)
        return
    if mode != "dns":
        raise ValueError("--neg_sampler must be uniform, dns or pop, got %s" % (mode,))
    train = getattr(args, "train", "normal")
    if train not in ("normal", "s_condition"):
        raise NotImplementedError("--train %s: --neg_sampler dns goes with --train normal (the raw head) and --train s_condition (the popularity "
                                  "head) only" % (train,))
    if getattr(args, "model", "mf") != "mf":
        raise NotImplementedError("--model %s: --neg_sampler dns scores candidates on the embedding tables themselves, a LightGCN's scores live on "
                                  "the propagated tables (--model mf)" % (args.model,))
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --neg_sampler dns scores fp32 tables only" % (args.table_dtype,))
    if getattr(args, "adam_sweep", "auto") in ("replay", "replay_fast"):
        raise NotImplementedError("--adam_sweep %s: --neg_sampler dns reads whole tables before every step, a replayed table's idle rows are stale "
                                  "then (--adam_sweep auto | sweep)" % (args.adam_sweep,))
    if getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("adam_exact_lazy: --neg_sampler dns reads whole tables before every step, a lazy table's idle rows are stale then")
    if getattr(args, "sampler", "device") != "device":
        raise NotImplementedError("--sampler %s: --neg_sampler dns is the device sampler's (--sampler device)" % (args.sampler,))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --neg_sampler dns trains on one GPU (no item shards)" % (args.gpus,))
    M, N = getattr(args, "dns_candidates", 16), getattr(args, "dns_topn", 1)
    if int(M) != M or not 1 <= int(M) <= ops.DNS_MAX_CANDIDATES:
        raise ValueError("--dns_candidates must be an integer in 1 .. %d, got %s" % (ops.DNS_MAX_CANDIDATES, M))
    if int(N) != N or not 1 <= int(N) <= int(M):
        raise ValueError("--dns_topn must be an integer in 1 .. --dns_candidates = %d, got %s" % (int(M), N))


def check_negpop(args):
    """--neg_sampler pop: refuse, before anything is built, what popularity-weighted negative sampling has no path for.  Every message names
    its flag.  The batches have the layout of the uniform sampler's, so whatever trains on those goes through: the optimisers,
    --deterministic 1 with --train normal | s_condition, LightGCN, bf16 tables."""
    if getattr(args, "neg_sampler", "uniform") != "pop":
        return
    train = getattr(args, "train", "normal")
    if train not in ("normal", "s_condition", "ssm"):
        raise NotImplementedError("--train %s: --neg_sampler pop goes with --train normal, --train s_condition and --train ssm (--ssm_source sampled) "
                                  "only" % (train,))
    if train == "ssm" and getattr(args, "ssm_source", "sampled") != "sampled":
        raise NotImplementedError("--ssm_source %s: nothing is sampled there, --neg_sampler pop goes with --ssm_source sampled" % (args.ssm_source,))
    if getattr(args, "sampler", "device") != "device":
        raise NotImplementedError("--sampler %s: --neg_sampler pop is the device sampler's (--sampler device)" % (args.sampler,))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --neg_sampler pop trains on one GPU (no item shards)" % (args.gpus,))
    beta = getattr(args, "neg_pop_power", 0.75)
    try:
        ok = math.isfinite(float(beta)) and 0.0 <= float(beta) <= ops.NEGPOP_MAX_POWER
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("--neg_pop_power must be a finite number in [0, %g], got %s" % (ops.NEGPOP_MAX_POWER, beta))


class SSMBPRMF(BPRMF):
    """BPR-MF tables trained with the sampled-softmax loss (include/pda_hip_ssm.h): one positive and --ssm_negs sampled negatives
    per row under a softmax with temperature --ssm_tau, on cosine similarity with --ssm_norm 1.  Fetchables and checkpoint layout are those of
    BPRMF; a step is pda_ssm_adam_step_f32.  score_tables() -- what every ranking reads -- returns the raw tables for ssm_norm == 0 and the
    row-normalised tables for ssm_norm == 1 (the lists then rank by cosine similarity, the quantity the loss trained); weights[...] and the
    checkpoint always hold the RAW tables.
    --ssm_source batch (include/pda_hip_inbatch.h): a row's negatives are the other rows' positives, a step is the train mask
    (--ssm_mask_train 1) and pda_inbatch_adam_step_f32 with the logQ table (--ssm_logq 1); the trainer hands the train graph over with
    set_train_graph before the first step.  Tables, lists and checkpoint layout are the same.
    --ssm_source all (include/pda_hip_fullsm.h): a row's negatives are ALL items the user has not interacted with
    (--ssm_mask_train 1; every item with 0), the loss the other two sources estimate; a step is pda_fullsm_adam_step_f32 on the train graph of
    set_train_graph.  --ssm_negs and --ssm_logq play no part.
    --ssm_source sampled under --neg_sampler pop: the negatives come from a popularity proposal; with --ssm_logq 1 the step is
    pda_ssm_adam_step_logq_f32 on the proposal's log q, which the trainer hands over with set_neg_logq before the first step."""

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_ssm(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.adam_exact_lazy = False
        self.ssm_negs = int(getattr(args, "ssm_negs", 64))
        self.ssm_tau = float(getattr(args, "ssm_tau", 0.1))
        self.ssm_norm = int(getattr(args, "ssm_norm", 1))
        self._normed = None                  # ((U^, I^), (version of U, version of I) they were computed from)
        self.ssm_source = str(getattr(args, "ssm_source", "sampled"))
        self.ssm_logq = int(getattr(args, "ssm_logq", 1))
        self.ssm_mask_train = int(getattr(args, "ssm_mask_train", 1))
        self._graph = None                   # (train_indptr, train_indices, user_pool) of --ssm_source batch
        self._inbatch = None                 # its workspace, mask and logq, allocated once
        self._fullsm = None                  # the workspace of --ssm_source all, allocated once
        self.neg_sampler = str(getattr(args, "neg_sampler", "uniform"))
        self.neg_pop_power = float(getattr(args, "neg_pop_power", 0.75))
        self._neg_logq = None                # log q of the negatives' proposal (set_neg_logq)

    def set_train_graph(self, train_indptr, train_indices, user_pool=None):
        """--ssm_source batch | all: the train CSR on the device (int64 indptr, int32 item ids sorted inside a row) the mask is taken from, and
        (batch) the sampler's user pool the logQ table is computed for."""
        self._graph, self._inbatch, self._fullsm = (train_indptr, train_indices, user_pool), None, None

    def wants_neg_logq(self) -> bool:
        """Does a step subtract the proposal's log q?  The sampled source under --neg_sampler pop with --ssm_logq 1."""
        return self.ssm_source == "sampled" and self.neg_sampler == "pop" and bool(self.ssm_logq)

    def set_neg_logq(self, logq):
        """--neg_sampler pop with --ssm_logq 1: float32 [n_items] on the tables' device, log q_i of the proposal the negatives are drawn from
        (ops.NegPopTable.logq)."""
        self._neg_logq = logq

    def _inbatch_buffers(self, B, U, I):
        if self._inbatch is None or self._inbatch["B"] != B:
            if self._graph is None and (self.ssm_logq or self.ssm_mask_train):
                raise ValueError("--ssm_source batch with --ssm_logq 1 or --ssm_mask_train 1 needs the train graph: call set_train_graph first")
            b = dict(B=B, ws=ops.inbatch_workspace(B, U.shape[1], U.device), mask=None, logq=None)
            if self.ssm_mask_train:
                b["mask"] = torch.empty((B, ops.inbatch_mask_words(B)), dtype=torch.int32, device=U.device)
            if self.ssm_logq:
                b["logq"] = torch.from_numpy(ops.inbatch_logq(self._graph[0], self._graph[1], I.shape[0], self._graph[2])).to(U.device)
            self._inbatch = b
        return self._inbatch

    def score_tables(self):
        """ssm_norm == 1: the row-normalised tables of the current weights, recomputed when a step (or a restore) has moved them, cached otherwise."""
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        if not self.ssm_norm:
            return U, I
        ver = (U._version, I._version)
        if self._normed is None or self._normed[1] != ver:
            self._normed = ((ops.ssm_normalize_rows(U), ops.ssm_normalize_rows(I)), ver)
        return self._normed[0]

    def train_step(self, users, pos, negs=None, plan=None) -> torch.Tensor:
        """One sampled-softmax step on (users [B], pos [B], negs [B, N]); returns the float32 [3] device tensor (loss, mf_loss, reg_loss) of this
        step, as BPRMF.train_step does.  Nothing is read on the host.  --ssm_source batch | all: negs is ignored (the triplet sampler's negative)."""
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._opt_state()
        if "tagU" not in st:
            st["tagU"], st["tagI"] = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
        self._t += 1
        if self.ssm_source == "batch":
            b = self._inbatch_buffers(users.numel(), U, I)
            if b["mask"] is not None:
                ops.inbatch_mask(users, pos, self._graph[0], self._graph[1], U.shape[0], I.shape[0], out=b["mask"])
            ops.inbatch_adam_step(U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"], users, pos, b["ws"],
                                  tau=self.ssm_tau, norm=self.ssm_norm, regs=self.decay, reg_div=self.batch_size, step=self._t,
                                  lr_t=ops.adam_lr_t(self.lr, self._t), logq=b["logq"], mask=b["mask"],
                                  users_distinct=bool(getattr(self, "users_distinct", False)), loss_acc=self._loss)
            return self._loss
        if self.ssm_source == "all":
            B = users.numel()
            if self.ssm_mask_train and self._graph is None:
                raise ValueError("--ssm_source all with --ssm_mask_train 1 needs the train graph: call set_train_graph first")
            if self._fullsm is None or self._fullsm[0] != B:
                self._fullsm = (B, ops.fullsm_workspace(B, I.shape[0], I.shape[1], U.device))
            indptr, indices = (self._graph[0], self._graph[1]) if self.ssm_mask_train else (None, None)
            ops.fullsm_adam_step(U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"], users, pos,
                                 self._fullsm[1], tau=self.ssm_tau, norm=self.ssm_norm, regs=self.decay, reg_div=self.batch_size, step=self._t,
                                 lr_t=ops.adam_lr_t(self.lr, self._t), train_indptr=indptr, train_indices=indices,
                                 users_distinct=bool(getattr(self, "users_distinct", False)), loss_acc=self._loss)
            return self._loss
        logq = None
        if self.wants_neg_logq():
            if self._neg_logq is None:
                raise ValueError("--neg_sampler pop with --ssm_logq 1 needs the proposal's log q: call set_neg_logq first")
            logq = self._neg_logq
        ops.ssm_adam_step(U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"], users, pos, negs,
                          tau=self.ssm_tau, norm=self.ssm_norm, regs=self.decay, reg_div=self.batch_size, step=self._t,
                          lr_t=ops.adam_lr_t(self.lr, self._t), users_distinct=bool(getattr(self, "users_distinct", False)), loss_acc=self._loss,
                          logq=logq)
        return self._loss

    def state_dict(self):
        sd = super().state_dict()
        sd.update(ssm_negs=self.ssm_negs, ssm_tau=self.ssm_tau, ssm_norm=self.ssm_norm)
        if self.ssm_source == "batch":      # (a sampled run's checkpoint keeps the keys it had)
            sd.update(ssm_source=self.ssm_source, ssm_logq=self.ssm_logq, ssm_mask_train=self.ssm_mask_train)
        elif self.ssm_source == "all":      # (no logQ on the exact softmax)
            sd.update(ssm_source=self.ssm_source, ssm_mask_train=self.ssm_mask_train)
        elif self.neg_sampler == "pop":     # (a run under the popularity proposal: what it drew from and whether the logits were corrected)
            sd.update(neg_sampler=self.neg_sampler, neg_pop_power=self.neg_pop_power, ssm_logq=self.ssm_logq)
        return sd


DAU_RANKS = ("raw", "cosine")


def check_dau(args):
    """--train dau: refuse, before anything is built, what the DirectAU step has no kernel for.  Every message names its flag."""
    if getattr(args, "model", "mf") == "lightgcn":
        raise NotImplementedError("--model lightgcn: --train dau trains the tables of a BPRMF only (--model mf)")
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--deterministic 1: --train dau scatters the gradients of repeated ids with float atomics (no planned gradient; "
                                  "the loss terms alone are bit-reproducible)")
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train dau runs fp32 tables only" % args.table_dtype)
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--optimizer %s: --train dau runs the reference's dense-decay Adam only (--optimizer adam)" % args.optimizer)
    if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep") or getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("--adam_sweep %s: --train dau runs the dense Adam sweep only (auto | sweep)" % getattr(args, "adam_sweep", "auto"))
    if getattr(args, "sampler", "device") != "device":
        raise NotImplementedError("--sampler %s: --train dau draws its batches with the device sampler only (--sampler device)" % args.sampler)
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train dau trains on one GPU (the uniformity terms are the whole batch's)" % args.gpus)
    if getattr(args, "neg_sampler", "uniform") != "uniform":
        raise NotImplementedError("--neg_sampler %s: --train dau uses no negatives (--neg_sampler uniform; the triplet sampler's negative is "
                                  "ignored)" % args.neg_sampler)
    gamma = getattr(args, "dau_gamma", 1.0)
    if not (float(gamma) >= 0.0 and math.isfinite(float(gamma))):
        raise ValueError("--dau_gamma must be a finite number >= 0, got %s" % (gamma,))
    t = float(getattr(args, "dau_t", 2.0))
    if not 0.0 < t <= ops.DAU_MAX_T:
        raise ValueError("--dau_t must lie in (0, %g], got %s" % (ops.DAU_MAX_T, getattr(args, "dau_t", 2.0)))
    if getattr(args, "dau_same", "keep") not in ops.DAU_SAME:
        raise ValueError("--dau_same must be keep or drop, got %s" % (args.dau_same,))
    if getattr(args, "dau_rank", "raw") not in DAU_RANKS:
        raise ValueError("--dau_rank must be raw or cosine, got %s" % (args.dau_rank,))
    B = getattr(args, "batch_size", 2048)
    if int(B) != B or not 2 <= int(B) <= ops.DAU_MAX_B:
        raise ValueError("--batch_size must be an integer in 2 .. %d with --train dau (uniformity is over pairs of rows), got %s" % (ops.DAU_MAX_B, B))


class DAUMF(BPRMF):
    """BPR-MF tables trained with the DirectAU loss (include/pda_hip_dau.h): alignment of a user with its positive plus --dau_gamma
    times the mean uniformity of the batch's user rows and item rows on the unit sphere (temperature --dau_t; --dau_same keep | drop: whether
    pairs of rows with the same id count).  No negatives: the triplet sampler's negative is ignored.  Fetchables, tables, evaluation and
    checkpoint are those of BPRMF; a step is pda_dau_adam_step_f32.  score_tables() -- what every ranking reads -- returns the raw tables for
    --dau_rank raw and the row-normalised tables for --dau_rank cosine (the path --ssm_norm 1 takes); weights[...] and the checkpoint always hold
    the RAW tables."""

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_dau(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.adam_exact_lazy = False
        self.dau_gamma = float(getattr(args, "dau_gamma", 1.0))
        self.dau_t = float(getattr(args, "dau_t", 2.0))
        self.dau_same = str(getattr(args, "dau_same", "keep"))
        self.dau_rank = str(getattr(args, "dau_rank", "raw"))
        self._normed = None                  # ((U^, I^), (version of U, version of I) they were computed from)
        self._dau_ws = None                  # (B, workspace), allocated once
        self.dau_stat = torch.zeros(ops.DAU_STAT_WORDS, dtype=torch.float32, device=self.device)   # += (align, uni_U, uni_I, 1) of every step

    def score_tables(self):
        """--dau_rank cosine: the row-normalised tables of the current weights, recomputed when a step (or a restore) has moved them."""
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        if self.dau_rank != "cosine":
            return U, I
        ver = (U._version, I._version)
        if self._normed is None or self._normed[1] != ver:
            self._normed = ((ops.ssm_normalize_rows(U), ops.ssm_normalize_rows(I)), ver)
        return self._normed[0]

    def train_step(self, users, pos, neg=None, pos_pop=None, neg_pop=None, plan=None) -> torch.Tensor:
        """One DirectAU step on (users [B], pos [B]); returns the float32 [3] device tensor (loss, mf_loss, reg_loss) of this step, as
        BPRMF.train_step does.  Nothing is read on the host.  neg is ignored (the triplet sampler's negative)."""
        U, I = self.weights["user_embedding"], self.weights["item_embedding"]
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._opt_state()
        if "tagU" not in st:
            st["tagU"], st["tagI"] = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
        B = users.numel()
        if self._dau_ws is None or self._dau_ws[0] != B:
            self._dau_ws = (B, ops.dau_workspace(B, U.shape[1], U.device))
        self._t += 1
        ops.dau_adam_step(U, st["mU"], st["vU"], st["gU"], st["tagU"], I, st["mI"], st["vI"], st["gI"], st["tagI"], users, pos, self._dau_ws[1],
                          t=self.dau_t, gamma=self.dau_gamma, same=self.dau_same, regs=self.decay, reg_div=self.batch_size, step=self._t,
                          lr_t=ops.adam_lr_t(self.lr, self._t), users_distinct=bool(getattr(self, "users_distinct", False)),
                          stat=self.dau_stat, loss_acc=self._loss)
        return self._loss

    def take_dau(self):
        """(mean align, mean uni_U, mean uni_I) over the steps since the last call (one host read), and a fresh count."""
        al, uu, ui, n = self.dau_stat.double().tolist()
        self.dau_stat.zero_()
        n = max(n, 1.0)
        return al / n, uu / n, ui / n

    def state_dict(self):
        sd = super().state_dict()
        sd.update(dau_gamma=self.dau_gamma, dau_t=self.dau_t, dau_same=self.dau_same, dau_rank=self.dau_rank)
        return sd


MACR_EMBED_SIZES = ops.MACR_EVAL_EMBED_SIZES   # --embed_size of a MACR model: what its lists (the bias head) can rank


def macr_c_grid(args):
    """The values of c an evaluation tries after c = 0: np.linspace(--start, --end, --step) with --check_c 1, the single --c with --check_c 0."""
    import numpy as np
    if int(getattr(args, "check_c", 1)):
        return [float(c) for c in np.linspace(float(args.start), float(args.end), int(args.step))]
    return [float(args.c)]


def check_macr(args):
    """--train macr: refuse, before anything is built, what MACR has no kernel for.  Every message names its flag."""
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--deterministic 1: --train macr sums its gradients with float atomics (no planned gradient)")
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train macr runs fp32 tables only" % args.table_dtype)
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--optimizer %s: --train macr runs the reference's dense-decay Adam only (--optimizer adam)" % args.optimizer)
    if getattr(args, "adam_sweep", "auto") not in ("auto", "sweep") or getattr(args, "adam_exact_lazy", None):
        raise NotImplementedError("--adam_sweep %s: --train macr runs the dense Adam sweep only (auto | sweep)" % getattr(args, "adam_sweep", "auto"))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train macr trains and evaluates on one GPU" % args.gpus)
    k = getattr(args, "topk_max", None)
    if k is not None and int(k) > ops.TOPK_K_V4:
        raise NotImplementedError("--topk_max %d: MACR ranks by the bias head (u . s_i I_i - c s_i), which has no lists deeper than %d"
                                  % (int(k), ops.TOPK_K_V4))
    if int(args.embed_size) not in MACR_EMBED_SIZES:
        raise NotImplementedError("--embed_size %s: --train macr ranks by the bias-head score kernels, which take one of %s"
                                  % (args.embed_size, MACR_EMBED_SIZES))
    for flag in ("alpha", "beta", "c", "start", "end"):
        if not math.isfinite(float(getattr(args, flag, 0.0))):
            raise ValueError("--%s must be finite, got %s" % (flag, getattr(args, flag)))
    if int(getattr(args, "check_c", 1)) not in (0, 1):
        raise ValueError("--check_c must be 0 or 1, got %s" % args.check_c)
    if int(getattr(args, "check_c", 1)) and int(getattr(args, "step", 20)) < 1:
        raise ValueError("--step must be >= 1 (the number of values of c between --start and --end), got %s" % args.step)


class MACRBPRMF(BPRMF):
    """MACR on BPR-MF (Wei et al., KDD'21): the three-branch loss of MF/model_api.py:613-651 and its counterfactual inference.
    Fetchables: those of BPRMF.  weights: user_embedding, item_embedding, and the two branch vectors w_item / w_user [d, 1] (the reference's
    `item_branch` / `user_branch`), Xavier-uniform like every [fan_in, fan_out] table: U(-l, l), l = sqrt(6 / (d + 1)).  A step is
    pda_macr_adam_step_f32 with --alpha / --beta as the loss weights.  c: the constant of (y - c) s_i s_u the lists are ranked with (update_c);
    best_c: the value the last evaluation chose, kept in the checkpoint."""
    LOSS_TERMS = ops.MACR_LOSS_TERMS       # a step's loss row: loss, L_O, L_I, L_U, reg

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_macr(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.adam_exact_lazy = False
        self.alpha, self.beta = float(args.alpha), float(args.beta)          # self.alpha = args.alpha in the reference's class
        self.c = self.best_c = 0.0
        self._macr = None
        self._prep = None                    # (MacrItemPrep, item table version, w_item version)
        self._loss_ring = torch.zeros((16, self.LOSS_TERMS), dtype=torch.float32, device=self.device)
        self._loss = self._loss_ring[0]
        self.epoch_terms = None              # float64 [5]: the sums of the last finished epoch's loss rows

    def init_weights(self, gen):
        w = super().init_weights(gen)
        w["w_item"] = xavier_uniform_(torch.empty(self.emb_dim, 1, device=self.device), gen)
        w["w_user"] = xavier_uniform_(torch.empty(self.emb_dim, 1, device=self.device), gen)
        return w

    def _macr_state(self):
        if self._macr is None:
            self._macr = ops.MacrState(self.weights["user_embedding"], self.weights["item_embedding"])
        return self._macr

    def update_c(self, c):
        """MF/model_api.py:744: the constant the next lists are ranked with."""
        c = float(c)
        if not math.isfinite(c):
            raise ValueError("c must be finite, got %s" % c)
        self.c = c

    def item_prep(self):
        """sig and J = fl(sig_i I_i) of the current weights (ops.macr_item_prep), rebuilt when a step or a checkpoint moved them: once per
        evaluation, whatever the number of user blocks and of values of c."""
        I, w = self.weights["item_embedding"], self.weights["w_item"]
        if self._prep is None or self._prep[1:] != (I._version, w._version):
            prep = ops.macr_item_prep(I, w, self._prep[0] if self._prep is not None else None)
            self._prep = (prep, I._version, w._version)
        return self._prep[0]

    @staticmethod
    def trainer_terms(row):
        """(loss, mf_loss, reg_loss) of a loss row or of a sum of rows: mf_loss = L_O + alpha L_I + beta L_U, everything except reg_loss."""
        return torch.stack([row[0], row[0] - row[4], row[4]])

    def start_loss_rows(self, n_steps: int):
        self._loss_rows = torch.zeros((max(1, int(n_steps)), self.LOSS_TERMS), dtype=torch.float32, device=self.device)
        self._loss_row_i = 0

    def finish_loss_rows(self) -> torch.Tensor:
        """The trainer's (loss, mf_loss, reg_loss) sums; all five terms of the epoch stay in epoch_terms."""
        rows, n = self._loss_rows, self._loss_row_i
        self._loss_rows = None
        self.epoch_terms = rows[:n].double().sum(0)
        return self.trainer_terms(self.epoch_terms)

    def train_step(self, users, pos, neg, pos_pop=None, neg_pop=None, plan=None) -> torch.Tensor:
        """One MACR step; returns the float32 [5] device tensor (loss, L_O, L_I, L_U, reg_loss) of this step (trainer_terms: the trainer's three)."""
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._macr_state()
        w = self.weights
        self._t += 1
        ops.macr_adam_step(w["user_embedding"], w["item_embedding"], w["w_item"], w["w_user"], users, pos, neg, st, alpha=self.alpha, beta=self.beta,
                           regs=self.decay, reg_div=self.batch_size, step=self._t, lr_t=ops.adam_lr_t(self.lr, self._t),
                           users_distinct=bool(getattr(self, "users_distinct", False)), loss_acc=self._loss)
        return self._loss

    CKPT_MOMENTS = ("mU", "vU", "mI", "vI", "mW", "vW")

    def state_dict(self):
        w = self.weights
        sd = {"format": self.CKPT_FORMAT, "model": "macr", "embed_size": self.emb_dim, "n_users": self.n_users, "n_items": self.n_items,
              "optimizer": self.optimizer, "table_dtype": self.table_dtype, "user_embedding": w["user_embedding"],
              "item_embedding": w["item_embedding"], "w_item": w["w_item"], "w_user": w["w_user"], "adam_t": self._t, "macr_alpha": self.alpha,
              "macr_beta": self.beta, "macr_c": self.best_c}
        if self._macr is not None:
            sd.update({k: getattr(self._macr, k) for k in self.CKPT_MOMENTS})
        return sd

    def load_state_dict(self, sd):
        if not isinstance(sd, dict) or "user_embedding" not in sd:
            raise ValueError("not a pda_amd checkpoint (a tf.train.Saver checkpoint of the reference cannot be loaded)")
        if sd.get("format") != self.CKPT_FORMAT:
            raise ValueError("checkpoint format %r, MACRBPRMF reads %s" % (sd.get("format"), self.CKPT_FORMAT))
        if sd.get("model", "mf") != "macr":
            raise ValueError("checkpoint of a %s model cannot be loaded into MACRBPRMF (no branch vectors)" % sd.get("model", "mf"))
        for key, mine in (("embed_size", self.emb_dim), ("n_users", self.n_users), ("n_items", self.n_items)):
            if int(sd[key]) != int(mine):
                raise ValueError("checkpoint %s = %s, model has %s" % (key, sd[key], mine))
        names = ("user_embedding", "item_embedding", "w_item", "w_user")
        for k in names:
            if tuple(sd[k].shape) != tuple(self.weights[k].shape):
                raise ValueError("checkpoint table %s does not have the model's shape" % k)
        for k in names:
            self.weights[k].copy_(sd[k])
        self._t = int(sd.get("adam_t", 0))
        self.c = self.best_c = float(sd.get("macr_c", 0.0))
        self._macr = None                     # (fresh tags and zero gradient accumulators: as after DICE's restore)
        if "mU" in sd:
            st = self._macr_state()
            for k in self.CKPT_MOMENTS:
                getattr(st, k).copy_(sd[k])


GCN_EMBED_SIZES = ops.GCN_EMBED_SIZES       # --embed_size of a LightGCN model: the row widths of pda_gcn_spmm_f32


def gcn_train_pairs(train_user_list):
    """The train pairs (users int64 [n], items int64 [n]) from the loader's {user: [items]} lists: what the graph is built from (a pair that
    occurs twice is one edge: ops.gcn_graph_arrays)."""
    import numpy as np
    us = [u for u, items in train_user_list.items() if len(items)]
    if not us:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    lens = [len(train_user_list[u]) for u in us]
    return np.repeat(np.asarray(us, dtype=np.int64), lens), np.concatenate([np.asarray(train_user_list[u], dtype=np.int64) for u in us])


def check_lightgcn(args):
    """--model lightgcn: refuse, before anything is built, what the LightGCN backbone has no kernel for.  Every message names the combination."""
    train = getattr(args, "train", "normal")
    if train in ("temp_pop", "dice", "ips", "macr", "ssm"):
        raise NotImplementedError("--model lightgcn --train %s: the LightGCN backbone trains with --train normal (BPR) or s_condition (PD/PDA) only" % train)
    if train not in ("normal", "s_condition"):
        raise NotImplementedError("--model lightgcn --train %s: normal | s_condition" % train)
    test = getattr(args, "test", "normal")
    if test not in (("normal",) if train == "normal" else ("s_condition", "normal")):
        raise NotImplementedError("--model lightgcn --train %s --test %s: --train normal goes with --test normal, --train s_condition with "
                                  "--test s_condition | normal" % (train, test))
    if getattr(args, "optimizer", "adam") != "adam":
        raise NotImplementedError("--model lightgcn --optimizer %s: the gradient of a graph model is dense, it runs the reference's Adam only "
                                  "(--optimizer adam)" % args.optimizer)
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--model lightgcn --table_dtype %s: the LightGCN backbone runs fp32 tables only" % args.table_dtype)
    if int(getattr(args, "deterministic", 0) or 0):
        raise NotImplementedError("--model lightgcn --deterministic 1: the propagation is bit-reproducible, the triplet gradient under it is summed "
                                  "with float atomics (no planned gradient on the final tables)")
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--model lightgcn --gpus %s: no item-parallel training (the graph is not sharded); train on one GPU" % args.gpus)
    L = getattr(args, "gcn_layers", 3)
    if int(L) != L or not 0 <= int(L) <= ops.GCN_MAX_LAYERS:
        raise ValueError("--gcn_layers must be an integer in 0 .. %d, got %s" % (ops.GCN_MAX_LAYERS, L))
    if int(args.embed_size) not in GCN_EMBED_SIZES:
        raise NotImplementedError("--model lightgcn --embed_size %s: the product kernel takes one of %s" % (args.embed_size, GCN_EMBED_SIZES))


class LightGCN(_MFBase):
    """LightGCN (He et al., SIGIR'20; DESIGN.md 5j, include/pda_hip_gcn.h) under the BPR loss.  Fetchables: those of BPRMF.
    weights: the EGO tables user_embedding / item_embedding, Xavier-uniform from the same seed as every other model, kept as the two row
    slices of one [n_users + n_items, d] buffer so that one launch per layer serves both directions.  score_tables() returns the FINAL tables
    (the layer mean over --gcn_layers propagations): everything that ranks reads those.  data_config["gcn_train_pairs"] = (users, items), or
    set_train_pairs: the train pairs the graph is built from -- rebuilt from the data, never stored in a checkpoint."""
    with_pop = False
    MODEL_NAME = "lightgcn"

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, pos_pop_api=None,
                 neg_pop_api=None, **kw):
        check_lightgcn(args)
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, pos_pop_api, neg_pop_api, **kw)
        self.adam_exact_lazy = False
        self.gcn_layers = int(getattr(args, "gcn_layers", 3))
        self.graph = None
        self._final = None                   # ((F_U, F_I), version of the ego buffer they were computed from)
        self._G = None
        if data_config.get("gcn_train_pairs") is not None:
            self.set_train_pairs(*data_config["gcn_train_pairs"])
        self.opt, self.loss = Fetch(self, "opt"), Fetch(self, "loss")
        self.mf_loss, self.reg_loss = Fetch(self, "mf_loss"), Fetch(self, "reg_loss")
        self.batch_ratings = Fetch(self, "batch_ratings")

    def init_weights(self, gen):
        w = super().init_weights(gen)        # (the draws of _MFBase, then moved into one buffer: the same values from the same seed)
        self._E0 = torch.cat([w["user_embedding"], w["item_embedding"]], dim=0)
        return {"user_embedding": self._E0[:self.n_users], "item_embedding": self._E0[self.n_users:]}

    def set_train_pairs(self, users, items):
        self.graph = ops.GcnGraph(users, items, self.n_users, self.n_items, self.device)
        self._final = None

    def _opt_state(self):
        if self._state is None:
            z = lambda: torch.zeros_like(self._E0)      # noqa: E731
            m, v = z(), z()
            nu = self.n_users
            self._state = {"mU": m[:nu], "vU": v[:nu], "mI": m[nu:], "vI": v[nu:]}
        return self._state

    def _need_graph(self):
        if self.graph is None:
            raise ValueError("LightGCN needs the train pairs before it propagates (data_config['gcn_train_pairs'] or set_train_pairs)")
        return self.graph

    def score_tables(self):
        """The final tables of the current ego tables: recomputed when a step (or a restore) has moved them since, cached otherwise."""
        U0, I0 = self.weights["user_embedding"], self.weights["item_embedding"]
        if self.gcn_layers == 0:
            return U0, I0
        if self._final is None or self._final[1] != self._E0._version:
            F = ops.gcn_propagate(self._need_graph(), U0, I0, self.gcn_layers)
            self._final = (F, self._E0._version)
        return self._final[0]

    def train_step(self, users, pos, neg, pos_pop=None, neg_pop=None, plan=None) -> torch.Tensor:
        """One LightGCN step: propagate, the triplet gradient on the final tables (regs = 0), the backward pass, the ego-row regulariser, Adam
        over both ego tables.  No host read; returns the float32 [3] device tensor (loss, mf_loss, reg_loss) of this step."""
        if not self.with_pop:
            pos_pop = neg_pop = None
        elif pos_pop is None or neg_pop is None:
            raise ValueError("PD/PDA needs pos_pop and neg_pop")
        g = self._need_graph()
        U0, I0 = self.weights["user_embedding"], self.weights["item_embedding"]
        rows = getattr(self, "_loss_rows", None)
        if rows is not None and self._loss_row_i < rows.shape[0]:
            self._loss = rows[self._loss_row_i]
            self._loss_row_i += 1
        else:
            self._loss_i = (self._loss_i + 1) & 15
            self._loss = self._loss_ring[self._loss_i]
            self._loss.zero_()
        st = self._opt_state()
        if self._G is None:
            self._G = torch.zeros_like(self._E0)
        L = self.gcn_layers
        F_U, F_I = ops.gcn_propagate(g, U0, I0, L)
        self._final = None                   # (the graph's buffer now holds the tables of BEFORE this step's update)
        self._G.zero_()
        G_U, G_I = self._G[:self.n_users], self._G[self.n_users:]
        ops.bpr_step(F_U, F_I, users, pos, neg, pos_pop, neg_pop, regs=0.0, reg_div=self.batch_size, mode=ops.UPD_DENSE_GRAD, gU=G_U, gI=G_I,
                     loss_acc=self._loss)
        H_U, H_I = ops.gcn_backward(g, G_U, G_I, L)
        ops.gcn_reg(U0, I0, users, pos, neg, H_U, H_I, regs=self.decay, reg_div=self.batch_size, loss_acc=self._loss)
        self._t += 1
        ops.adam_dense_sweep2(U0, st["mU"], st["vU"], H_U, I0, st["mI"], st["vI"], H_I, ops.adam_lr_t(self.lr, self._t))
        return self._loss

    def state_dict(self):
        sd = {"format": self.CKPT_FORMAT, "model": self.MODEL_NAME, "gcn_layers": self.gcn_layers, "embed_size": self.emb_dim, "n_users": self.n_users,
              "n_items": self.n_items, "optimizer": self.optimizer, "table_dtype": self.table_dtype,
              "user_embedding": self.weights["user_embedding"], "item_embedding": self.weights["item_embedding"], "adam_t": self._t}
        if self._state is not None:
            sd.update(self._state)
        return sd

    def load_state_dict(self, sd):
        name = type(self).__name__
        if not isinstance(sd, dict) or "user_embedding" not in sd:
            raise ValueError("not a pda_amd checkpoint (a tf.train.Saver checkpoint of the reference cannot be loaded)")
        if sd.get("format") != self.CKPT_FORMAT:
            raise ValueError("checkpoint format %r, %s reads %s" % (sd.get("format"), name, self.CKPT_FORMAT))
        if sd.get("model", "mf") != self.MODEL_NAME:
            raise ValueError("checkpoint of a %s model cannot be loaded into %s (its tables are not ego tables)" % (sd.get("model", "mf"), name))
        for key, mine in (("embed_size", self.emb_dim), ("n_users", self.n_users), ("n_items", self.n_items), ("gcn_layers", self.gcn_layers)):
            if int(sd[key]) != int(mine):
                raise ValueError("checkpoint %s = %s, model has %s" % (key, sd[key], mine))
        for k in ("user_embedding", "item_embedding"):
            if tuple(sd[k].shape) != tuple(self.weights[k].shape):
                raise ValueError("checkpoint table %s does not have the model's shape" % k)
        for k in ("user_embedding", "item_embedding"):
            self.weights[k].copy_(sd[k])
        self._final = None
        self._t = int(sd.get("adam_t", 0))
        if "mU" in sd:
            st = self._opt_state()
            for k in ("mU", "vU", "mI", "vI"):
                st[k].copy_(sd[k])
        else:
            self._state = None


class ConditionalLightGCN(LightGCN):
    """PD / PDA on the LightGCN backbone: the matching term is the popularity head (ELU + 1) x pop^gamma of ConditionalBPRMF on the final tables.
    Fetchables: those of ConditionalBPRMF."""
    with_pop = True

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.opt_pop_global, self.loss_pop_global = Fetch(self, "opt"), Fetch(self, "loss")
        self.mf_loss_pop_global, self.reg_loss_pop_global = Fetch(self, "mf_loss"), Fetch(self, "reg_loss")
        self.condition_ratings = Fetch(self, "condition_ratings")


# ---- iALS (include/pda_hip_ials.h) ------------------------------------------------------------------------------------------------
IALS_EMBED_SIZES = ops.IALS_EMBED_SIZES     # --embed_size of an iALS model: a d x d fp32 matrix has to fit the LDS (256 does not)
IALS_SOLVERS = ("exact", "block")           # --ials_solver: the row-wise exact solve | iALS++ block steps (any of ops.IALSPP_EMBED_SIZES)


def check_ials(args):
    """--train ials: refuse, before anything is built, what the iALS baseline has no path for.  Every message names its flag.
    --lr, --optimizer, --adam_sweep, --sampler and --batch_size (for training) are unused: there is no sampler and no optimiser.
    --deterministic 1 is accepted and changes nothing: the run is a function of its flags and data either way."""
    if getattr(args, "train", "normal") != "ials":
        if getattr(args, "test", "normal") == "ials":
            raise NotImplementedError("--test ials needs an iALS model (--train ials), not --train %s" % (args.train,))
        return
    if getattr(args, "model", "mf") != "mf":
        raise NotImplementedError("--model %s: --train ials solves the two embedding tables of --model mf; a LightGCN has no closed-form row "
                                  "update" % (args.model,))
    if getattr(args, "table_dtype", "f32") != "f32":
        raise NotImplementedError("--table_dtype %s: --train ials runs fp32 tables only" % (args.table_dtype,))
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise NotImplementedError("--gpus %s: --train ials trains on one GPU (no item shards)" % (args.gpus,))
    if getattr(args, "neg_sampler", "uniform") != "uniform":
        raise NotImplementedError("--neg_sampler %s: --train ials has no sampled negatives (every unobserved pair is weighed by --ials_alpha0)"
                                  % (args.neg_sampler,))
    solver = getattr(args, "ials_solver", "exact")
    if solver not in IALS_SOLVERS:
        raise ValueError("--ials_solver must be one of %s, got %s" % (" | ".join(IALS_SOLVERS), solver))
    if solver == "block":
        if int(args.embed_size) not in ops.IALSPP_EMBED_SIZES:
            raise NotImplementedError("--embed_size %s: --train ials --ials_solver block takes one of %s" % (args.embed_size, ops.IALSPP_EMBED_SIZES))
        k = int(getattr(args, "ials_block", 32))
        if k not in ops.IALSPP_BLOCK_SIZES:
            raise ValueError("--ials_block must be one of %s, got %s" % (ops.IALSPP_BLOCK_SIZES, args.ials_block))
        if int(args.embed_size) % k:
            raise ValueError("--ials_block %d does not divide --embed_size %s" % (k, args.embed_size))
    elif int(args.embed_size) not in IALS_EMBED_SIZES:
        raise NotImplementedError("--embed_size %s: --train ials takes one of %s (a d x d fp32 matrix per row has to fit the LDS)"
                                  % (args.embed_size, IALS_EMBED_SIZES))
    if getattr(args, "test", "normal") not in ("normal", "ials"):
        raise NotImplementedError("--test %s: --train ials goes with --test normal (the raw head and the gamma search of a BPRMF) or --test ials"
                                  % (args.test,))
    regs = float(args.regs)
    if not (regs > 0.0 and math.isfinite(regs)):
        raise ValueError("--regs must be a finite number > 0 with --train ials (it is lambda: the row systems are positive definite by it), got %s"
                         % (args.regs,))
    a0 = float(getattr(args, "ials_alpha0", 0.1))
    if not (a0 >= 0.0 and math.isfinite(a0)):
        raise ValueError("--ials_alpha0 must be a finite number >= 0, got %s" % (args.ials_alpha0,))
    nu = float(getattr(args, "ials_nu", 1.0))
    if not 0.0 <= nu <= 1.0:
        raise ValueError("--ials_nu must lie in 0 .. 1, got %s" % (args.ials_nu,))
    beta = float(getattr(args, "ials_item_power", 0.0))
    if not (math.isfinite(beta) and 0.0 <= beta <= ops.IALS_ITEM_POWER_MAX):
        raise ValueError("--ials_item_power must be a finite number in 0 .. %g, got %s" % (ops.IALS_ITEM_POWER_MAX, args.ials_item_power))


class IALSMF(BPRMF):
    """Implicit ALS (Hu et al. ICDM'08 in the form of Rendle et al. RecSys'22; DESIGN.md 5o, include/pda_hip_ials.h).  Tables, fetchables,
    evaluation and checkpoint are those of BPRMF (model "mf", no optimiser state): the two differ only in how they were trained.  There is no
    step: train_epoch() is the user half-sweep, the item half-sweep and the objective.  data_config["gcn_train_pairs"] = (users, items), or
    set_train_pairs: the train pairs -- rebuilt from the data, never stored in a checkpoint; a model that is only restored and evaluated
    needs none.  --ials_solver block (iALS++, DESIGN.md 5v, include/pda_hip_ialspp.h) replaces the two half-sweeps by one exact step per block
    of --ials_block coordinates, users then items, at --embed_size up to 256; the tables keep their usual initialisation, which matters there
    (a block step starts from x), and the prediction cache is rebuilt every epoch and never checkpointed.  --ials_item_power beta > 0 (DESIGN.md
    5y, include/pda_hip_ials_itemw.h) weighs the unobserved pairs of item i by alpha0 w_i, w_i ~ (c_i + 1)^beta with mean 1, in either solver:
    the weights are rebuilt from the train pairs with the graph and never checkpointed."""

    def __init__(self, args, data_config, use_dataset_api=False, users_api=None, pos_items_api=None, neg_items_api=None, **kw):
        check_ials(args)
        if int(getattr(args, "deterministic", 0) or 0):
            # accepted, and it changes nothing: there is no plan and no atomic sum to replace, the run is a function of flags and data either way
            args = copy.copy(args)
            args.deterministic = 0
        super().__init__(args, data_config, use_dataset_api, users_api, pos_items_api, neg_items_api, **kw)
        self.optimizer = "ials"
        self.adam_exact_lazy = False
        self.ials_alpha0 = float(getattr(args, "ials_alpha0", 0.1))
        self.ials_nu = float(getattr(args, "ials_nu", 1.0))
        self.ials_solver = getattr(args, "ials_solver", "exact")
        self.ials_block = int(getattr(args, "ials_block", 32))
        self.ials_item_power = float(getattr(args, "ials_item_power", 0.0))
        self.graph = None
        if data_config.get("gcn_train_pairs") is not None:
            self.set_train_pairs(*data_config["gcn_train_pairs"])

    def set_train_pairs(self, users, items):
        self.graph = ops.IalsGraph(users, items, self.n_users, self.n_items, self.device, lam=self.decay, alpha0=self.ials_alpha0, nu=self.ials_nu,
                                   item_power=self.ials_item_power)
        iw = self.graph.item_weights
        if iw is not None:
            print("||--- ials item_power=%g w_min=%.6g w_max=%.6g" % (self.ials_item_power, float(iw.w.min()), float(iw.w.max())), flush=True)

    def train_step(self, *a, **kw):
        raise NotImplementedError("--train ials has no batch step: train_epoch() runs the two half-sweeps")

    def train_epoch(self) -> torch.Tensor:
        """One epoch: X <- argmin_X L(X, Y), then Y <- argmin_Y L(X, Y), then the objective at the new tables.  Returns the device float64 [3]
        (loss, fit, reg) / |S|, [3] read together with the failed-pivot counter by failed_pivots(); no host read here."""
        g = self.graph
        if g is None:
            raise ValueError("IALSMF needs the train pairs before it trains (data_config['gcn_train_pairs'] or set_train_pairs)")
        X, Y = self.weights["user_embedding"], self.weights["item_embedding"]
        if self.ials_solver == "block":     # iALS++: block steps from the tables as they stand -- their initialisation matters here
            return ops.ialspp_epoch(g, X, Y, self.ials_block) / max(1, g.nnz)
        ops.ials_half_sweep(g, "user", Y, X)
        ops.ials_half_sweep(g, "item", X, Y)
        return ops.ials_loss(g, X, Y) / max(1, g.nnz)

    def failed_pivots(self) -> torch.Tensor:
        """The device int32 [1] count of rows written as NaN by a failed pivot since the model was built (0 on finite tables)."""
        if self.ials_solver == "block":
            return ops.ialspp_buffers(self.graph, self.emb_dim)["fail"]
        return self.graph.buffers(self.emb_dim)["fail"]

    def state_dict(self):
        sd = super().state_dict()
        sd.update(optimizer="ials", ials_alpha0=self.ials_alpha0, ials_nu=self.ials_nu)
        if self.ials_solver == "block":     # (an exact-solver run's state dict stays as it was)
            sd.update(ials_solver="block", ials_block=self.ials_block)
        if self.ials_item_power != 0.0:     # (an unweighted run's state dict stays as it was)
            sd.update(ials_item_power=self.ials_item_power)
        return sd
