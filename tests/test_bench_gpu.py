"""The multi-rank bench on one GPU (bench.py --rehearse): every rank renders its tile share on
device 0, the tile-cost balance and the frame-end gather run over gloo, rank 0 assembles the
frame.  The assembled frame must equal the one-rank frame bit for bit (pixels are
independent), so the N-rank path the driver's scaling run takes is checked on real hardware
except for the RCCL transport itself."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
COMMON = ["--steps", "1", "--warmup", "1", "--frames-per-step", "4", "--width", "256", "--height", "160",
          "--cpu-seconds", "0", "--single-frames", "0", "--frame-sha"]


def _bench(*args):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *COMMON, *args], capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("n,extra", [(2, []), (3, ["--no-balance"]), (2, ["--pipeline-steps"])])
def test_multi_rank_bench_frame_equals_one_rank(n, extra):
    one = _bench("--gpus", "1")
    many = _bench("--gpus", str(n), "--rehearse", *extra)
    assert many["n_gpus"] == n and many["rehearsal"]
    assert many["frame_sha256"] == one["frame_sha256"]
    assert many["rays_per_sample"] == one["rays_per_sample"]
    # the line shows which collective backend saw how many ranks, and each rank's time
    co = many["collective"]
    assert co["backend"] == "gloo" and co["world"] == n and co["rehearsal"]
    assert len(co["rank_ms"]) == n and len(co["gather_ms_per_rank"]) == n and co["gather_ms"] >= 0
    assert co["rank_max_over_mean"] >= 1.0
    assert one["collective"]["world"] == 1 and one["collective"]["backend"] is None


FULL_ONLY = ("roofline", "cpu_baseline", "own_traversal_per_ray", "ms_per_frame_single", "ms_single_frame_latency")


def test_plain_bench_prints_the_headline_and_dumps_its_frame(tmp_path):
    """A plain run times its steps and nothing else; --dump-outputs writes the frame the last timed
    step assembled (the one --frame-sha hashes) and the counts behind rays_per_sample."""
    import hashlib

    import numpy as np
    d = _bench("--gpus", "1", "--dump-outputs", str(tmp_path / "out"))
    assert d["steps"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f32"
    assert not [k for k in FULL_ONLY if k in d]
    frame = np.load(tmp_path / "out" / "frame.npy")
    code = np.load(tmp_path / "out" / "frame_nonfinite.npy")
    assert frame.dtype == code.dtype == np.float32 and frame.shape == code.shape == (160, 256, 3)
    assert np.isfinite(frame).all() and frame.max() > 0 and np.isin(code, (0, 1, 2, 3)).all()
    # the two arrays hold the frame (a NaN's payload bits aside, so the hash is compared when this
    # small render has no NaN pixel: it has none)
    whole = frame.copy()
    for c, v in ((2, np.inf), (3, -np.inf)):
        whole[code == c] = v
    assert not frame[code != 0].any() and not (code == 1).any()
    assert hashlib.sha256(whole.tobytes()).hexdigest() == d["frame_sha256"]
    rays, samples = np.load(tmp_path / "out" / "counts.npy")
    assert samples == 256 * 160 * 4 and round(rays / samples, 4) == d["rays_per_sample"]


def test_full_bench_adds_the_roofline_and_the_one_frame_calls():
    plain = _bench("--gpus", "1")
    full = _bench("--gpus", "1", "--full", "--single-frames", "2")
    assert full["frame_sha256"] == plain["frame_sha256"] and full["rays_per_sample"] == plain["rays_per_sample"]
    assert full["roofline"]["kernel"] == "wf_trace" and "standalone" in full["roofline"]["avg_launch_ms_regime"]
    assert full["own_traversal_per_ray"]["tri"] > 0
    assert full["ms_per_frame_single"] > 0 and full["ms_single_frame_latency"] > 0
    assert "cpu_baseline" not in full  # COMMON: --cpu-seconds 0


def test_eight_rank_bench_at_full_size_frame_equals_one_rank():
    """The driver's largest configuration: 8 ranks of 1920x1080 tiles, cost-balanced map."""
    full = ["--width", "1920", "--height", "1080", "--frames-per-step", "2"]
    one = _bench("--gpus", "1", *full)
    eight = _bench("--gpus", "8", "--rehearse", *full)
    assert eight["frame_sha256"] == one["frame_sha256"]
    assert eight["rays_per_sample"] == one["rays_per_sample"]
