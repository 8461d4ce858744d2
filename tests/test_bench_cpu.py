"""bench.py contract on CPU: randOrigin for any frame count (the driver's --steps 20 --warmup 5
needs 25,601+ frames), the in-tree glibc rand() restatement against the libc and the committed
fixture, and the self-launching multi-rank path in its gloo dry-run mode."""
import ctypes
import ctypes.util
import json
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT
from rtamd import configs as cf
from rtamd import scene_lib as sl


def test_rand_origins_cover_the_driver_bench():
    n = (5 + 20) * 1024 + 1 + 64
    ro = cf.rand_origins(n)
    assert ro.shape == (n,) and ro.dtype == np.float32
    fix = cf._fixture_bits()
    assert np.array_equal(ro[:len(fix)].view(np.uint32), fix)
    assert np.all((ro >= 674764.0) & (ro <= 2 * 674764.0))
    assert np.array_equal(cf.rand_origins(100, offset=20000), ro[20000:20100])
    assert np.array_equal(cf.rand_origins(10, offset=16380), ro[16380:16390])  # straddles the fixture end


def _libc():
    name = ctypes.util.find_library("c")
    if not name:
        return None
    L = ctypes.CDLL(name)
    try:
        L.gnu_get_libc_version.restype = ctypes.c_char_p
        L.gnu_get_libc_version()
    except AttributeError:
        return None  # not glibc: its rand() is another generator
    return L


@pytest.mark.parametrize("seed", [0, 1, 20221002, 123456789, 2**31 - 1, 2**32 - 1])
def test_glibc_rand_restatement_equals_libc(seed):
    L = _libc()
    if L is None:
        pytest.skip("host libc is not glibc")
    L.srand(ctypes.c_uint(seed))
    want = np.array([L.rand() for _ in range(5000)], np.int32)
    assert np.array_equal(sl.glibc_rand(seed, 5000), want)


def _bench(*args, timeout=240):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_dry_run_driver_arguments():
    d = _bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--dry-run")
    assert d["dry_run"] and d["n_gpus"] == 1
    assert d["frames_planned"] == (5 + 20) * 1024 + 1 + 64
    assert d["pixels_covered"] == d["frame_pixels"] == 1920 * 1080


def test_bench_self_launches_two_gloo_ranks():
    d = _bench("--gpus", "2", "--steps", "20", "--warmup", "5", "--dry-run")
    assert d["n_gpus"] == 2 and d["gather_ok"]
    assert d["pixels_covered"] == 1920 * 1080
    co = d["collective"]
    assert co["backend"] == "gloo" and co["world"] == 2 and len(co["rank_ms"]) == 2


def test_bench_launcher_stops_the_other_ranks_when_one_fails():
    """A rank that exits early would leave the others waiting in the rendezvous; the launcher
    stops them and returns the failing rank's status instead of hanging."""
    t0 = time.time()
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--dry-run", "--fail-rank", "1"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])
    assert not any(ln.startswith("{") for ln in p.stdout.splitlines())
    assert time.time() - t0 < 90


def test_trace_ray_bytes_follow_the_path_state_layout():
    """bench.py's algorithmic bytes per secondary ray = queue entry + the WFState ray rows
    (float4 {o.xyz, d.x} + float2 {d.y, d.z}) + the 4-B result (the closest triangle; ADVICE r2:
    the constant had kept the 32-B ray of an older layout)."""
    import bench
    src = (ROOT / "opengl-ray-tracing-framework_amd" / "csrc" / "hip" / "rt_wavefront.h").read_text()
    assert "float4* __restrict__ ra;" in src and "float2* __restrict__ rb;" in src
    assert "float4* __restrict__ sa;" in src and "float2* __restrict__ sb;" in src
    assert "int* __restrict__ res;" in src
    assert bench.B_RAY_SECONDARY == 4 + (16 + 8) + 4
    assert bench.B_RAY_PASS1 == 4 + 16 + 4  # WFState ra/sa float4 only (p1_ray): origin from org
    assert bench.B_RAY_CAMERA == 4


def test_roofline_bound_follows_the_limiter():
    """The roofline block prices wf_trace at its STANDALONE launch time (the probe render, one frame
    group), names the limiter from the utilisations (HBM, VALU issue at the 2.4 GHz spec clock, L2)
    and reports achieved / peak / frac of that bound, the HBM roofline beside it (VERDICT r3 weak
    #4).  No field implies a clock, a bandwidth or a kernel time per step above what was measured."""
    import bench
    st = {"rays": 2_000_000_000, "samples": 800_000_000, "trace_launches": 10, "trace_ms": 160.0,
          "path_steps": 1_000_000_000, "pass0_steps": 200_000_000, "pass1_steps": 300_000_000}
    probe = {"rays": 1_000_000_000, "samples": 400_000_000, "trace_launches": 5, "trace_ms": 60.0, "frames": 7}
    vis = {"rays": 1000, "internal_pops": 3000, "tri_tests": 3000}
    prof = {"_file": "profiles/x.json", "kernels": {
        "wf_trace": {"avg_launch_ms": 16.0, "avg_launch_ms_standalone": 12.0, "hbm_bytes_per_launch": 1.2e10,
                     "SQ": {"SQ_INSTS_VALU": 6.6e9, "SQ_INSTS_SALU": 3.3e9, "SQ_ACTIVE_INST_VALU": 6.7e9,
                            "SQ_THREAD_CYCLES_VALU": 1.9e11}},
        "wf_shade": {"avg_launch_ms": 13.0, "avg_launch_ms_standalone": 6.0, "hbm_bytes_per_launch": 3.0e10}}}
    r = bench.roofline(st, vis, None, prof, probe, 2)
    assert r["kernel"] == "wf_trace" and r["avg_launch_ms"] == 12.0 and "standalone" in r["avg_launch_ms_regime"]
    # algorithmic bytes of the probe's launches: 4 B per camera ray, 32 B per other secondary ray
    assert r["hbm"]["algorithmic_bytes_per_launch"] == round((4 * 400e6 + 32 * 600e6) / 5)
    r1 = bench.roofline(st, vis, None, prof, dict(probe, p1_rays=50_000_000), 2)
    assert r["hbm"]["algorithmic_bytes_per_launch"] - r1["hbm"]["algorithmic_bytes_per_launch"] == 10_000_000 * 8
    want = 6.6e9 * 2 / (1024 * 2.4e9 * 12e-3)
    assert abs(r["valu"]["frac"] - want) < 1e-4 and r["valu"]["spec_clock_ghz"] == 2.4
    assert r["valu"]["salu_per_valu"] == 0.5
    assert r["limiter"] == max(r["utilisation"], key=r["utilisation"].get) == "valu_issue"
    assert r["bound"] == "valu_issue" and r["frac"] == r["valu"]["frac"] and r["unit"] == r["valu"]["unit"]
    assert all(0 < v < 1 for v in r["utilisation"].values())
    sh = r["kernels"]["wf_shade"]
    assert sh["path_steps_per_launch"] == 100_000_000
    assert sh["algorithmic_bytes_per_launch"] == round((88 * 200e6 + 168 * 300e6 + 176 * 500e6) / 10)
    assert 0 < sh["frac"] < sh["traffic_frac"] < 1
    # per-step kernel time implied by each per-launch figure stays within the step
    assert r["avg_launch_ms"] * r["launches_per_step"] <= st["trace_ms"] / 2 * 1.0001
    # no probe: the co-running time, labelled as such
    r2 = bench.roofline(st, None, None, None, None, 2)
    assert r2["avg_launch_ms"] == 16.0 and "co-running" in r2["avg_launch_ms_regime"] and r2["bound"] == "hbm"


def _committed_bench_line(config="C3"):
    """the newest committed bench line of a configuration in the round-4 roofline format (with a
    PMC profile), and its profile"""
    prof = ROOT / "profiles"
    found = list(prof.glob(f"r*_bench_{config}.json")) + list(prof.glob(f"r*_other_configs/bench_{config}.json"))
    for p in sorted(found, key=lambda q: str(q.relative_to(prof)), reverse=True):
        d = json.loads(p.read_text())
        if "avg_launch_ms_regime" in d.get("roofline", {}) and d["roofline"].get("profile"):
            return p, d
    return None, None


@pytest.mark.parametrize("config", ["C3", "C4", "C5"])
def test_committed_roofline_recomputes_from_the_profile(config):
    """every roofline figure of the committed bench line is recomputable from
    profiles/ and consistent with the step: frac = algorithmic bytes (or VALU instructions) per
    launch / the standalone launch time; the standalone time agrees with rocprof's standalone
    launches within 5%; wf_trace and wf_shade per-launch times x launches per step fit in the step;
    bound = limiter."""
    p, d = _committed_bench_line(config)
    if p is None:
        pytest.skip("no committed bench line with a profile yet")
    assert d["config"]["workload"].startswith(config)
    rf = d["roofline"]
    prof = json.loads((ROOT / rf["profile"]).read_text())
    kt = prof["kernels"]["wf_trace"]
    t = rf["avg_launch_ms"]
    assert abs(rf["hbm"]["achieved"] - rf["hbm"]["algorithmic_bytes_per_launch"] / (t * 1e-3) / 1e9) < 0.2
    assert abs(rf["hbm"]["frac"] - rf["hbm"]["achieved"] / 8000.0) < 1e-4
    v = rf["valu"]
    assert abs(v["achieved"] - kt["SQ"]["SQ_INSTS_VALU"] / (t * 1e-3) / 1e9) < 0.2
    assert abs(v["frac"] - v["achieved"] / (1024 * 2.4 / 2)) < 1e-4
    assert rf["bound"] == rf["limiter"] == max(rf["utilisation"], key=rf["utilisation"].get)
    std = kt.get("probe_avg_launch_ms") or kt["avg_launch_ms_standalone"]
    assert abs(std / t - 1) < 0.05, (std, t)
    assert t * rf["launches_per_step"] <= d["ms_per_step"]
    sh = rf["kernels"]["wf_shade"]
    assert sh["avg_launch_ms_standalone"] * sh["launches_per_step"] <= d["ms_per_step"]
    assert abs(sh["frac"] - sh["algorithmic_bytes_per_launch"] / (sh["avg_launch_ms_standalone"] * 1e-3) / 8e12) < 1e-3
    assert d["kernel"]["busy_ms_per_step"] <= d["ms_per_step"]


def test_cpu_baseline_records_the_host():
    import bench
    h = bench.host_cpus()
    assert h["nproc"] >= 1 and 1 <= h["affinity"] <= h["nproc"]
    assert "cpu_model" in h


def test_bench_plain_run_is_the_default():
    """--full (CPU baseline, one-frame calls, probe and visit-count frames, roofline) is off unless
    asked for; --dump-outputs names a directory and needs the assembled frame."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 3)
    assert bench.parse_args(["--full"]).full
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--dump-outputs", "d", "--no-gather"])


def test_dump_outputs_are_finite_and_hold_the_frame(tmp_path, monkeypatch):
    """The frame keeps the NaN pixels of the reference's estimator; the dump writes finite arrays:
    the frame with 0 there and a code array saying what was there.  A frame above the size budget
    is written as the same seeded pixel sample every time."""
    import bench
    rng = np.random.default_rng(3)
    f = rng.uniform(0, 4, (9, 16, 3)).astype(np.float32)
    f[2, 3, 1], f[2, 3, 2], f[8, 15, 0], f[0, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    bench.dump_outputs(tmp_path / "a", f, 7.0, 3.0)
    fr, code = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "frame_nonfinite.npy")
    assert fr.dtype == code.dtype == np.float32 and fr.shape == code.shape == f.shape
    assert np.isfinite(fr).all() and code.sum() == 1 + 2 + 3 + 1
    assert (code[2, 3, 1], code[2, 3, 2], code[8, 15, 0], code[0, 0, 0]) == (1, 2, 3, 1)
    assert np.array_equal(fr[code == 0], f[code == 0]) and not fr[code != 0].any()
    assert list(np.load(tmp_path / "a" / "counts.npy")) == [7.0, 3.0]
    assert not (tmp_path / "a" / "frame_pixels.npy").exists()
    # over the budget: n pixels, the same ones in every run
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 32 * 40)
    bench.dump_outputs(tmp_path / "b", f, 7.0, 3.0)
    bench.dump_outputs(tmp_path / "c", f, 7.0, 3.0)
    idx = np.load(tmp_path / "b" / "frame_pixels.npy")
    assert idx.dtype == np.float64 and len(idx) == 40 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "c" / "frame_pixels.npy"))
    fb, cb = np.load(tmp_path / "b" / "frame.npy"), np.load(tmp_path / "b" / "frame_nonfinite.npy")
    assert fb.shape == cb.shape == (40, 3)
    assert np.array_equal(fb, fr.reshape(-1, 3)[idx.astype(int)]) and np.array_equal(cb, code.reshape(-1, 3)[idx.astype(int)])
    assert sum(p.stat().st_size for p in (tmp_path / "b").iterdir()) <= 32 * 40 + 16 + 4 * 128  # + counts + the .npy headers


def test_bench_tile_default_follows_the_rank_count():
    """Round 5: 32-px rank tiles at N = 1, 16-px tiles at N > 1 (the cost-balanced map of smaller
    tiles evens 8 ranks out better); an explicit --tile wins."""
    import bench
    assert bench.parse_args([]).tile == 32
    assert bench.parse_args(["--gpus", "8"]).tile == 16
    assert bench.parse_args(["--gpus", "2", "--tile", "64"]).tile == 64
