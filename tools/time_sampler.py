"""Time the three places the device sampler (pda_amd/csrc/pda_sample.h) is compiled into, on the C2 tables, B = 2048:
the fused step that draws the next batch in its own launch (HIP graph of 64 steps), pda_bpr_train_steps_f32 (64 steps per
launch) and pda_sample_batches_dev (64 batches per launch).  One JSON line; PDA_HIP_LIB selects the build (A/B against a
parent library: run the two in turn, several times each).      python tools/time_sampler.py [workload] [B]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pda_amd import _lib, ops, synthetic

wl = sys.argv[1] if len(sys.argv) > 1 else "c2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
dev = torch.device("cuda")
W = synthetic.make_workload(wl, dev)
regs, lr, seed, G = 1e-2, 1e-2, 2020, 64
kw = dict(n_pool=W.n_users, train_slots=W.hist_slots, neg_range=(0, W.n_items), pop_matrix=W.pop_train)
mk = lambda *s: (torch.empty(s, dtype=torch.int32, device=dev), torch.empty(s, dtype=torch.int32, device=dev),
                 torch.empty(s, dtype=torch.int32, device=dev), torch.empty(s, device=dev), torch.empty(s, device=dev))


def clock(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


res = {"lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)), "workload": wl, "B": B}

# 1. fused step + in-launch sampler, 64 steps per graph
U, I, bufs, loss = W.U.clone(), W.I.clone(), [mk(B), mk(B)], torch.zeros(3, device=dev)
ctr = torch.tensor([1, 0], dtype=torch.int64, device=dev)
ops.sample_triplets_into(bufs[0], W.hist_indptr, W.hist_indices, seed=seed, step_dev=ctr, parity=0, **kw)


def body(i):
    ops.bpr_step_and_sample(U, I, *bufs[i & 1], regs=regs, reg_div=B, lr=lr, next_out=bufs[(i + 1) & 1], train_indptr=W.hist_indptr,
                            train_indices=W.hist_indices, seed=seed, step_dev=ctr, parity=(i + 1) & 1, loss_acc=loss, **kw)


s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    body(0); body(1)
torch.cuda.current_stream().wait_stream(s)
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    for i in range(G):
        body(i)
res["step_sample_us_per_step"] = round(clock(g.replay, 200) / G, 3)

# 2. 64 steps in one launch
U, I, bufs = W.U.clone(), W.I.clone(), [mk(B), mk(B)]
c1 = torch.tensor([1], dtype=torch.int64, device=dev)
ops.sample_triplets_into(bufs[0], W.hist_indptr, W.hist_indices, seed=seed, step_dev=c1, **kw)
ws = [None]


def looped():
    _, ws[0] = ops.bpr_train_steps(U, I, bufs, G, regs=regs, reg_div=B, lr=lr, train_indptr=W.hist_indptr, train_indices=W.hist_indices,
                                   seed=seed, step_ctr=c1, loss_acc=loss, barrier_ws=ws[0], **kw)


res["train_steps_us_per_step"] = round(clock(looped, 200) / G, 3)
assert int(ws[0][1]) == 0

# 3. 64 batches per sampler launch
q = mk(G, B)
c2 = torch.tensor([1, 0], dtype=torch.int64, device=dev)
calls = [0]


def many():
    ops.sample_batches_into(q, W.hist_indptr, W.hist_indices, seed=seed, step_dev=c2, parity=calls[0] & 1, **kw)
    calls[0] += 1


res["sample_batches_us_per_launch"] = round(clock(many, 1000), 3)
print(json.dumps(res))
