"""GPU: bench.py honours the driver's contract -- one JSON line with the agreed fields (tiny workload so it takes seconds)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def contract_line(stdout):
    """What the driver ingests: the LAST non-empty stdout line parses as JSON, is far below the size that lost round 5's record
    (BENCH_r05.parsed == null at ~21 kB) and carries no NaN / Infinity token."""
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert lines, "no stdout"
    last = lines[-1]
    assert len(last) < 8192, len(last)
    for tok in ("NaN", "Infinity"):
        assert tok not in last
    d = json.loads(last)
    assert len([l for l in lines if l.startswith("{")]) == 1
    return d


def run_bench(tmp_path, *flags):
    extras = os.path.join(str(tmp_path), "extras.json")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--extras-path", extras] + list(flags),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = contract_line(out.stdout)
    full = json.load(open(extras))
    # the compact line is a projection of the full record
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype"):
        assert line[k] == full[k], k
    return line, full


def test_bench_emits_one_contract_line(dev, tmp_path):
    line, d = run_bench(tmp_path, "--workload", "tiny", "--steps", "2", "--warmup", "1",
                        "--eval-block", "1024", "--cpu-budget", "1", "--train-steps", "128")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "summary"):
        assert k in line, k
    lr, lc = line["roofline"], line["cpu_baseline"]
    assert lr["bound"] in ("mfma", "hbm") and lr["unit"] == "TFLOP/s" and abs(lr["frac"] - lr["achieved"] / lr["peak"]) < 1e-4
    assert lr["kernel_ms"] > 0 and lr["kernel_ms_source"] == "hip_events_per_call" and "kernel_template" in lr and "hbm" in lr
    assert lc["kind"] in ("port", "reference") and lc["cores"] >= 1 and lc["value"] > 0 and 0 < len(lc["sample"]) <= 200
    assert len(line["config"]["workload"]) <= 120 and "model" not in line["config"] and line["config"]["ranks_seen"] == 1
    assert line["summary"]["raw_head"]["roofline_frac"] > 0 and line["summary"]["extras"] == "bench_extras.json"
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "users/s" and d["value"] > 0 and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("mfma", "hbm") and r["unit"] == "TFLOP/s" and r["peak"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    t = d["train"]
    assert t["sgd_fused"]["triplets_per_s"] > 0 and t["adam_dense_reference_faithful"]["triplets_per_s"] > 0
    a = t["adam_on_headline_tables"]         # the reference's optimiser on the headline tables: with and without the sweep
    assert a["dense_sweep"]["triplets_per_s"] > 0 and a["replay"]["triplets_per_s"] > 0 and a["replay"]["final_sync_ms"] > 0
    assert a["replay_fast"]["triplets_per_s"] > 0 and a["replay_fast_graph"]["steps_taken_on_device"] >= 128
    # round 2: what one pass costs after a weight update, roofs measured on the box, the native CPU top-K, the protocol
    p = d["prep"]
    assert p["prep_ms"] > 0 and p["users_per_s_incl_prep"] > 0 and p["steps_per_pass"] >= 1
    assert r["peak_measured"] > 100 and abs(r["frac_of_measured"] - r["achieved"] / r["peak_measured"]) < 1e-9
    assert r["hbm"]["peak_measured_GBs"] > 500
    assert c["native_topk"]["value"] > 0 and c["native_topk"]["threads"] == c["cores"] and "median" in c["protocol"]
    assert d["dtype"] == "f32"
    # round 3: the raw head the reference evaluates every epoch (MF/train_new_api.py:1139-1141), the exact planned SGD step,
    # SGD on the headline workload's own tables, the CPU port cut over the host threads
    rh = d["raw_head"]
    assert rh["value"] > 0 and 0 < rh["roofline_frac"] < 1 and "RAW" in rh["kernel"]
    assert t["sgd_exact_planned"]["triplets_per_s"] > 0 and t["sgd_planned_one_launch"]["triplets_per_s"] > 0
    assert t["sgd_exact_planned_sampler_32_batches_ahead_graph"]["batches_drawn"] > 0
    big = t["sgd_on_headline_tables"]
    assert big["B2048"]["exact_planned"]["triplets_per_s"] > 0 and big["B2048"]["fused_hogwild"]["hbm_frac"] > 0
    assert c["torch_intraop_threads"]["value"] > 0
    # round 4: the reference's own block protocol (do_recommendation on 2 048-user blocks, MF/train_new_api.py:703,792), what
    # torch.distributed saw, and where kernel_ms comes from
    b = d["eval_block_2048"]
    assert b["users_per_block"] == 2048 and b["users_per_s"] > 0 and b["device_only"]["users_per_s"] >= b["users_per_s"] * 0.5
    assert d["config"]["ranks_seen"] == 1 and d["config"]["backend"] is None and len(d["config"]["workload"]) <= 120
    assert r["kernel_ms_source"] == "hip_events_per_call"


def test_bench_bf16_tables_line(dev, tmp_path):
    """BASELINE config 5's table type through the same contract (tiny shapes: d = 64)."""
    line, d = run_bench(tmp_path, "--workload", "tiny", "--table-dtype", "bf16", "--steps", "2",
                        "--warmup", "1", "--eval-block", "1024", "--no-train", "--no-cpu-baseline")
    assert line["dtype"] == "bf16" and line["cpu_baseline"] is None
    assert d["dtype"] == "bf16" and d["value"] > 0 and d["ordered_sweep"]["value"] > 0


def test_bench_bf16_train_keys(dev, tmp_path):
    """BASELINE config 5 asks for bf16 train throughput: the bf16 line carries train.sgd_bf16 (fused + refreshes, planned exact)."""
    line, d = run_bench(tmp_path, "--workload", "tiny", "--table-dtype", "bf16", "--steps", "2",
                        "--warmup", "1", "--eval-block", "1024", "--no-cpu-baseline", "--train-steps", "128")
    sb = d["train"]["sgd_bf16"]
    assert sb["bytes_per_triplet"] == 6 * 64 * 2 + 20
    for B in ("B2048",):
        assert sb[B]["exact_planned"]["triplets_per_s"] > 0 and sb[B]["fused_hogwild"]["triplets_per_s"] > 0


def test_plain_run_times_the_headline_only_and_dumps_its_lists(dev, tmp_path):
    """A plain run (no --full): the headline steps and the result line, nothing measured beside them.  --dump-outputs writes the lists
    of the last timed step -- the same in two runs with the same arguments, and the oracle's lists for those users."""
    import numpy as np
    from oracle import c_oracle
    from pda_amd import synthetic
    dumps = []
    for i in range(2):
        extras, dump = os.path.join(str(tmp_path), "extras%d.json" % i), os.path.join(str(tmp_path), "out%d" % i)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1",
                              "--eval-block", "1024", "--extras-path", extras, "--dump-outputs", dump],
                             capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        line, full = contract_line(out.stdout), json.load(open(extras))
        assert line["steps"] == 3 and line["roofline"]["kernel_ms_spread"]["calls"] == 3       # one score call per timed step
        assert line["unit"] == "users/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 1024) < 1e-6 * 1024
        for k in ("cpu_baseline", "train", "per_config", "eval_block_2048", "raw_head", "ordered_sweep", "dense_natural_order", "prep"):
            assert full[k] is None, k
        assert "peaks_measured" not in full["roofline"] and full["roofline"]["box"] == {"before": None, "after": None}
        dumps.append([np.load(os.path.join(dump, n + ".npy")) for n in ("topk_items", "topk_scores", "users")])
    items, scores, users = dumps[0]
    assert items.shape == scores.shape == (1024, 50) and users.shape == (1024,)
    assert items.dtype == users.dtype == np.float64 and scores.dtype == np.float32
    for a, b in zip(dumps[0], dumps[1]):
        np.testing.assert_array_equal(a, b)
    W = synthetic.make_workload("tiny", dev)
    ip, ix, u = W.hist_indptr.cpu().numpy(), W.hist_indices.cpu().numpy(), users.astype(np.int64)
    bptr = np.concatenate([[0], np.cumsum(ip[u + 1] - ip[u])])                 # the oracle's history rows are the block's rows
    bind = np.concatenate([ix[ip[x]:ip[x + 1]] for x in u])
    ridx, rval = c_oracle.score_topk(W.U.cpu().numpy(), W.I.cpu().numpy(), u.astype(np.int32), 50, 1, W.pop_last.cpu().numpy(),
                                     bptr, bind, order=1)
    np.testing.assert_allclose(scores, rval, rtol=2e-6, atol=1e-6)
    assert (items == ridx).mean() > 0.99          # (two items of a last-ulp near-tie may swap places, as smoke() allows)
