"""bench.py's plain run: one result line with the headline fields only (every other leg runs with --full), and --dump-outputs writes what the
last timed step computed -- the same arrays, bit for bit, from two runs with the same arguments (seeded init and inputs, bit-reproducible path)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_repeatable_outputs(tmp_path):
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "32",
                            "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out = [l for l in r.stdout.decode().splitlines() if l.strip()]
        assert len(out) == 1, out
        lines.append(json.loads(out[0]))
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    j = lines[0]
    assert j["steps"] == 3 and j["unit"] == "pose-clips/sec" and j["higher_is_better"] is True and j["dtype"] == "bf16"
    assert j["value"] == pytest.approx(32 * 1e3 / j["ms_per_step"], rel=1e-9)
    assert not {"eval", "parity", "roofline", "kernels", "configs", "fp32_mode", "cpu_baseline", "profile_stale"} & set(j)
    assert set(dumps[0]) == {"pred.npy", "loss_terms.npy", "params.npy", "grad.npy", "buffers.npy"}
    assert dumps[0]["pred.npy"].shape == (32, 27, 17, 3)
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20
    assert float(dumps[0]["loss_terms.npy"][0]) == j["final_loss"]
    for name, a in dumps[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        assert np.array_equal(a, dumps[1][name]), name
