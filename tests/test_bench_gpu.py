"""`bench.py` on the MI355X at a small size: a plain run prints the headline line and nothing else, `--full` adds the extra
measurements, `--dump-outputs` writes the last timed step's loss, parameters and gradients -- the same inputs on every run, and
the same outputs whether or not the timed steps carry the per-launch probe of `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "16", "--frames", "256", "--mels", "64", "--layers", "2"]
EXTRAS = ("roofline", "infonce_alone", "audio_encoder_alone", "full_last_block", "cpu_baseline")


def _bench(extra, out):
    clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra, "--dump-outputs", str(out)],
                         capture_output=True, text=True, timeout=400, env=clean, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), {n[:-4]: np.load(out / n) for n in sorted(os.listdir(out))}


@pytest.mark.timeout(1200)
def test_bench_plain_full_and_dumped_outputs(tmp_path):
    plain, a = _bench([], tmp_path / "a")
    again, b = _bench([], tmp_path / "b")
    full, c = _bench(["--full", "--no-cpu-baseline"], tmp_path / "c")
    for line in (plain, again, full):
        assert line["metric"] == "audio_text_pairs_per_sec" and line["unit"] == "pairs/s" and line["higher_is_better"] is True
        assert line["dtype"] == "bf16" and line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert abs(line["value"] - 16 / (line["ms_per_step"] * 1e-3)) < 1e-2 * line["value"]
    assert not [k for k in EXTRAS if k in plain], plain.keys()
    assert all(k in full for k in EXTRAS[:4]) and "cpu_baseline" not in full
    assert full["roofline"]["in_step_launches_timed"] > 0 and full["roofline"]["launches_timed"] > 0

    for line, d in ((plain, a), (again, b), (full, c)):
        assert sorted(d) == ["grads", "loss", "params"]
        assert d["loss"].dtype == np.float64 and d["params"].dtype == d["grads"].dtype == np.float32
        assert d["params"].shape == d["grads"].shape and sum(x.nbytes for x in d.values()) <= 64 << 20
        assert all(np.isfinite(x).all() for x in d.values()) and float(np.abs(d["grads"]).max()) > 0
        assert d["loss"].shape == (1,) and abs(float(d["loss"][0]) - line["loss"]) < 1e-4      # the loss the line reports
    # same arguments, same inputs: the outputs agree up to the summation order of the kernels; the probe of --full changes
    # how the c_fc launch is issued, not what it computes
    for d in (b, c):
        assert abs(float(d["loss"][0]) - float(a["loss"][0])) < 1e-3 * max(1.0, abs(float(a["loss"][0])))
        assert float(np.abs(d["params"] - a["params"]).max()) <= 1e-3 * float(np.abs(a["params"]).max())
        rel = float(np.linalg.norm(d["grads"] - a["grads"]) / np.linalg.norm(a["grads"]))
        assert rel < 2e-2, rel
