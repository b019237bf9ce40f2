"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy (the dense matrix's pairs i <= j --
all of them or a fixed seeded sample -- and the kernel's hit records), so that two builds can be compared output for output;
and a plain run (no --full) that still prints the contract's line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_triangle_sample_is_the_upper_triangle_or_a_fixed_sample_of_it():
    i, j = bench.triangle_sample(7, 100)
    iu = np.triu_indices(7)
    assert np.array_equal(i, iu[0]) and np.array_equal(j, iu[1])
    n = 11211
    i, j = bench.triangle_sample(n, 1 << 16)
    assert (0 <= i).all() and (i <= j).all() and (j < n).all()
    assert 0.99 * (1 << 16) < len(i) <= 1 << 16
    lin = i * n + j
    assert (np.diff(lin) > 0).all()                      # distinct, row-major
    i2, j2 = bench.triangle_sample(n, 1 << 16)
    assert np.array_equal(i, i2) and np.array_equal(j, j2)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import oracle_lib as ol
    d = str(tmp_path / "out")
    n = 200
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--chains", str(n),
                        "--dump-outputs", d], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for k in bench.REQUIRED_KEYS:
        assert k in res, k
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["dtype"] == "int16-exact" and res["unit"] == "cells/s" and res["higher_is_better"] is True
    assert "cpu_baseline" not in res and res["detail"] is None          # the other legs are --full only
    scores, hits, count = (np.load(os.path.join(d, f + ".npy")) for f in ("scores", "hits", "hit_count"))
    assert scores.dtype == np.float32 and hits.dtype == np.float64 and hits.shape[1] == 3
    seqs = bench.synth_mu_chains(0x5EED5EEC, n)
    i, j = bench.triangle_sample(n, bench.DUMP_SCORE_PAIRS)             # every pair at this size
    assert len(i) == n * (n + 1) // 2
    want = ol.mu_gapless_pairs(seqs, i, j)
    assert np.array_equal(scores.astype(np.int64), want.astype(np.int64))
    # the hit records: every pair scoring >= the bench's threshold (HIT_MIN = 120) once, sorted
    assert int(count[0]) == len(hits) > 0
    h = hits.astype(np.int64)
    assert np.array_equal(h, h[np.lexsort((h[:, 2], h[:, 1], h[:, 0]))])
    got = {(min(a, b), max(a, b), s) for a, b, s in h.tolist()}
    assert len(got) == len(h)
    assert got == {(a, b, s) for a, b, s in zip(i.tolist(), j.tolist(), want.tolist()) if s >= 120}
