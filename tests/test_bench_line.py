"""CPU: the projection bench.py prints as its contract line, applied to the largest full record on file (round 5's 21 kB line,
which the driver could not parse: BENCH_r05.parsed == null), and the checker tools/profile_round.sh runs on the box."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_line_of_a_full_c3_record_stays_small():
    """The projection applied to the largest record we have on file (round 5's unparsed 21 kB line)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    full = json.load(open(os.path.join(ROOT, "profiles", "round5d_c3_bench.json")))
    text = json.dumps(b.compact_contract_line(full), allow_nan=False)
    assert len(text) < 4096
    d = json.loads(text)
    assert d["roofline"]["frac"] > 0 and d["cpu_baseline"]["cores"] >= 1 and len(json.dumps(d["summary"])) < 1200
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_contract_line import check
    check("noise\n" + text + "\n\n")


def test_dump_outputs_samples_a_fixed_set_of_rows_within_the_limit(tmp_path):
    """bench.py --dump-outputs: item ids as float64 (exact), scores as float32, user ids beside them; a block larger than the byte
    limit is cut to a fixed sample of rows, the same on every call."""
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    n, K = 5000, 50
    g = torch.Generator().manual_seed(0)
    out = {"idx": torch.randint(0, 1 << 30, (n, K), generator=g, dtype=torch.int32), "val": torch.randn(n, K, generator=g),
           "users": torch.arange(7, 7 + n, dtype=torch.int32)}
    b.dump_outputs(str(tmp_path / "all"), out)
    items = np.load(str(tmp_path / "all" / "topk_items.npy"))
    assert items.dtype == np.float64 and np.array_equal(items, out["idx"].numpy())
    assert np.array_equal(np.load(str(tmp_path / "all" / "topk_scores.npy")), out["val"].numpy())
    b.DUMP_BYTES = 1000 * (K * 12 + 8)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), out)
    got = [[np.load(str(tmp_path / d / (f + ".npy"))) for f in ("topk_items", "topk_scores", "users")] for d in ("s1", "s2")]
    for x, y in zip(*got):
        np.testing.assert_array_equal(x, y)
    items, scores, users = got[0]
    assert items.shape == scores.shape == (1000, K) and sum(x.nbytes for x in got[0]) <= b.DUMP_BYTES
    rows = users.astype(np.int64) - 7
    assert np.all(np.diff(rows) > 0) and np.array_equal(items, out["idx"].numpy()[rows]) and np.array_equal(scores, out["val"].numpy()[rows])
