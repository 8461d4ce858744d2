"""Row arena for the state of passes >= 2 (WFParams::row_compact, csrc/hip/rt_wavefront.h): in a
lean group (WFParams::p1_lean) pass 1's shade numbers its surviving paths with rows claimed from
cnt[kCntRows] and writes their state to the dense arena; queue and active entries hold rows and the
later passes run on the arena in place.  The group decides on the device: pass 1's continuation
hits (wf_p1_count, between pass 1's traces and its shade) against the arena's rows; above them it
runs on the slot arrays as before.

Every in-process case renders with the development library twice, RT_ROW_COMPACT=0 and the default,
and requires: the image equals the oracle bit for bit, `rays` and `samples` equal the oracle's, and
every rt_stats counter but the timings and trace_iters* equals the RT_ROW_COMPACT=0 run's.  24 x 16
pixels with set_finish(2, 1), so every group is a bulk group, as tests/test_gpu_p1_lean.py; at least
128 frames, two groups of >= 64.  The images are far below the size at which pass 1 sorts by
itself, so these renders take the forced sort that numbers the rows.

The statistics cannot tell where the rows lived, so the overflow and report tests read the
development library's `rows:` line (RT_DEBUG_PASSES, after pass 1's shade) in child processes: the
library decides once per process whether it reports."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import bit_mismatch, frames_for, oracle_render
from rtamd import configs as cf
from rtamd import scene_lib as sl
from rtamd.renderer import Renderer, dev_lib_path

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
W, H = 24, 16  # 384 pixels; a block-iteration (2048 paths) spans 32 pixels' 64 frames, or 31.5 pixels' 65
FINISH_DEFAULT = (2, 8 << 20)

SCATTER = sl.Material(base_color=(1, 1, 1), specular=1.0, transmission=1.0, ior=1.3, medium_type=2,
                      medium_color=(0.3, 0.7, 0.9), medium_density=0.8, medium_anisotropy=0.0)


@pytest.fixture(scope="module")
def dev():
    r = Renderer(0, lib_path=dev_lib_path())
    yield r
    r.close()


_refs = {}
_scenes = {}


def _oracle(key, sd, env_maps, frames):
    """Oracle image and counters, computed once per key and left unchanged."""
    if key not in _refs:
        img, cnt = oracle_render(sd, env_maps, W, H, frames)
        img.setflags(write=False)
        _refs[key] = (img, cnt)
    return _refs[key]


def _scatter_bunny():
    """A bunny of a scattering medium on the reference floor (C2 placement)."""
    if "scatter" not in _scenes:
        obj = cf.Obj("bunny_4000", SCATTER, (0, 0, 0), (2.2, -2.5, 3), (2, 2, 2), False)
        _scenes["scatter"] = cf.build_scene((cf.FLOOR, obj))
    return _scenes["scatter"]


def _setup(r, sd, env_maps):
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env_maps)
    r.resize(W, H)
    r.set_finish(2, 1)
    r.clear_accum()
    r.set_loop_num(0)
    r.reset_stats()


def _counters(st):
    """Every rt_stats field but the timings and the two that count wave iterations of the counting
    trace (two runs of one build differ in them)."""
    return {k: v for k, v in st.items() if not k.endswith("_ms") and not k.startswith("trace_iters")}


def _both(r, monkeypatch, sd, env_maps, fp, ro):
    """[(image, stats) with RT_ROW_COMPACT=0, (image, stats) with the default]"""
    out = []
    monkeypatch.delenv("RT_ROW_CAP", raising=False)
    try:
        for knob in ("0", None):
            if knob is None:
                monkeypatch.delenv("RT_ROW_COMPACT", raising=False)
            else:
                monkeypatch.setenv("RT_ROW_COMPACT", knob)
            _setup(r, sd, env_maps)
            st = r.render(fp, ro)
            out.append((r.read_accum(), st))
    finally:
        r.set_finish(*FINISH_DEFAULT)
    return out


def _check(off, on, ref, cnt):
    for img, st in (off, on):
        assert bit_mismatch(img, ref)[0] == 0.0
        assert st["rays"] == cnt["rays"], st
        assert st["samples"] == cnt["samples"], st
    assert _counters(on[1]) == _counters(off[1])


def _down_view():
    """One unit above the floor beside the mesh, looking down: the floor fills the frame."""
    cam = sl.camera(-90.0, -89.0, 30.0, W / H)
    return cf.frame_params(W, H, position=(7.0, -1.0, 3.0), **cam)


# ------------------------------------------------------------------ 1: C3, both integrators
@pytest.mark.parametrize("bsdf", [True, False], ids=["bsdf", "brdf"])
@pytest.mark.parametrize("n", [128, 130])
def test_mixed_view(dev, env_maps, monkeypatch, n, bsdf):
    """C3, two groups of 64 / 65 frames.  At 65 a pixel's frames straddle block-iterations, so a call
    makes many row claims; the BRDF integrator's N.L rows (s4) travel through the arena.  Paths
    survive pass 1 (path_steps beyond the first two passes), so passes >= 2 read the rows."""
    sd = cf.config_scene("C3")
    fp = cf.frame_params(W, H, enable_bsdf=bsdf)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", n, bsdf), sd, env_maps, frames)
    off, on = _both(dev, monkeypatch, sd, env_maps, fp, ro)
    assert on[1]["path_steps"] > on[1]["pass0_steps"] + on[1]["pass1_steps"] > 0, on[1]
    _check(off, on, ref, cnt)


# ------------------------------------------------------------------ 2: every pixel hits, few continuations do
def test_floor_filling_down_view(dev, env_maps, monkeypatch):
    """The floor fills the frame: every pixel is listed and few of the continuations hit anything,
    so most of pass 1's items have key 0 and a block-iteration claims few rows."""
    sd = cf.config_scene("C3")
    n = 128
    fp = _down_view()
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", n, "down"), sd, env_maps, frames)
    off, on = _both(dev, monkeypatch, sd, env_maps, fp, ro)
    assert int((dev.first_hit(fp)["triangle"] < 0).sum()) == 0
    _check(off, on, ref, cnt)
    assert on[1]["pass0_steps"] == n * W * H, on[1]


# ------------------------------------------------------------------ 3: transmissive bunny
def test_transmissive_bunny(dev, env_maps, monkeypatch):
    """A bunny of a scattering medium: a refracted continuation stays inside the mesh, so most of
    its pixels' pass-1 continuations hit and their rows are dense; scattered paths carry PF_MEDIUM
    through the arena's s5 rows."""
    sd = _scatter_bunny()
    n = 128
    fp = cf.frame_params(W, H)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("scatter", n), sd, env_maps, frames)
    off, on = _both(dev, monkeypatch, sd, env_maps, fp, ro)
    assert on[1]["path_steps"] > on[1]["pass0_steps"] + on[1]["pass1_steps"] > 0, on[1]
    _check(off, on, ref, cnt)


# ------------------------------------------------------------------ 4: pass 1 / pass 2 is the last pass
@pytest.mark.parametrize("max_bounce", [1, 2])
def test_short_paths(dev, env_maps, monkeypatch, max_bounce):
    """max_bounce 1: pass 1 is the last pass, every claimed row is a hole and nothing reads the
    arena.  max_bounce 2: pass 2 is the arena's last reader and writes no row."""
    sd = cf.config_scene("C3")
    n = 128
    fp = cf.frame_params(W, H, max_bounce=max_bounce)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", n, "mb", max_bounce), sd, env_maps, frames)
    off, on = _both(dev, monkeypatch, sd, env_maps, fp, ro)
    _check(off, on, ref, cnt)
    two = on[1]["pass0_steps"] + on[1]["pass1_steps"]
    assert on[1]["pass1_steps"] > 0 and (on[1]["path_steps"] == two if max_bounce == 1 else on[1]["path_steps"] > two), on[1]


# ------------------------------------------------------------------ 5, 6: children that print the report
_CHILD = r"""
import hashlib, json, os, sys
root, out = sys.argv[1], sys.argv[2]
sys.path[:0] = [root + "/opengl-ray-tracing-framework_amd"]
import numpy as np
from rtamd import configs as cf
from rtamd import scene_lib as sl
from rtamd.renderer import Renderer, dev_lib_path
W, H = 24, 16
env = cf.load_env()
emissive = sl.Material(emissive=(4.0, 2.5, 1.0), base_color=(0.6, 0.6, 0.6), roughness=0.5, specular=0.5)
scenes = {"C3": lambda: cf.config_scene("C3"),
          "emissive": lambda: cf.build_scene((cf.FLOOR, cf.Obj("bunny_4000", emissive, (0, 0, 0), (2.2, -2.5, 3), (2, 2, 2), False)))}
r = Renderer(0, lib_path=dev_lib_path())
res = {}
for tag, scene, n, knobs in json.loads(sys.argv[3]):
    for k in ("RT_ROW_COMPACT", "RT_ROW_CAP"):
        os.environ.pop(k, None)
    os.environ.update(knobs)
    sd = scenes[scene]()
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env)
    r.resize(W, H)
    r.set_finish(2, 1)
    r.clear_accum()
    r.set_loop_num(0)
    r.reset_stats()
    print("==== " + tag, file=sys.stderr, flush=True)
    st = r.render(cf.frame_params(W, H), cf.rand_origins(n))
    np.save(out + "/" + tag + ".npy", r.read_accum())
    res[tag] = {k: v for k, v in st.items() if not k.endswith("_ms") and not k.startswith("trace_iters")}
r.close()
print(json.dumps(res))
"""


def _child(tmp_path, runs, **env_extra):
    """Render `runs` = [(tag, scene, frames, knobs)] in one child process with RT_DEBUG_PASSES.
    Returns ({tag: counters}, {tag: image}, {tag: [per group of pass 1: (enabled, hits, cap, claimed,
    compact)]}, {tag: [pass 2's kept paths per group]})."""
    env = dict(os.environ, RT_DEBUG_PASSES="1", **env_extra)
    for k in ("RT_ROW_COMPACT", "RT_ROW_CAP", "RT_P1_LEAN"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(tmp_path), json.dumps(runs)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    rows, kept2 = {}, {}
    tag = pass_ = None
    for ln in p.stderr.splitlines():
        if ln.startswith("==== "):
            tag = ln[5:].strip()
            rows[tag], kept2[tag] = [], []
        m = re.match(r"\[rt\] group \d+ pass (\d+):", ln)
        if m:
            pass_ = int(m.group(1))
        m = re.match(r"\[rt\]\s+lists: continuations \d+ shadow rays \d+ kept paths (\d+)", ln)
        if m and pass_ == 2:
            kept2[tag].append(int(m.group(1)))
        m = re.match(r"\[rt\]\s+rows: enabled (\d) hits (\d+) cap (\d+) claimed (\d+) compact (\d)", ln)
        if m:
            rows[tag].append(tuple(int(x) for x in m.groups()))
    imgs = {t: np.load(tmp_path / (t + ".npy")) for t in stats}
    return stats, imgs, rows, kept2


def test_overflow_falls_back(env_maps, tmp_path):
    """One group of 64 frames of the C3 view (RT_GROUPS=1, so the view has one hit count).  A first
    child prints that count; a second renders with the arena capped at 1 row, at one row below the
    count and at the count: the same image (the oracle's) and counters each time; the first two run
    on the slot arrays, the third on the arena."""
    n = 64
    sd = cf.config_scene("C3")
    fp = cf.frame_params(W, H)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", n, True), sd, env_maps, frames)
    _, _, rows, _ = _child(tmp_path, [("probe", "C3", n, {})], RT_GROUPS="1")
    assert len(rows["probe"]) == 1, rows
    enabled, hits, cap, claimed, compact = rows["probe"][0]
    assert enabled == 1 and compact == 1 and 1 < hits == claimed <= cap, rows
    runs = [("cap1", "C3", n, {"RT_ROW_CAP": "1"}), ("below", "C3", n, {"RT_ROW_CAP": str(hits - 1)}),
            ("at", "C3", n, {"RT_ROW_CAP": str(hits)})]
    stats, imgs, rows, _ = _child(tmp_path, runs, RT_GROUPS="1")
    for tag, want_cap, want_compact in (("cap1", 1, 0), ("below", hits - 1, 0), ("at", hits, 1)):
        assert rows[tag] == [(1, hits, want_cap, hits if want_compact else 0, want_compact)], (tag, rows)
        assert bit_mismatch(imgs[tag], ref)[0] == 0.0, tag
        assert stats[tag]["rays"] == cnt["rays"] and stats[tag]["samples"] == cnt["samples"], (tag, stats[tag])
        assert stats[tag] == stats["at"], tag


def test_report_shows_when_the_arena_ran(tmp_path):
    """Three 128-frame renders (two groups of 64) in one child process: the arena is used by default in
    C3, where the rows claimed are pass 1's continuation hits and at least pass 2's kept paths (a hit
    path that queues nothing leaves a hole); it is off with the knob and off in a scene with an
    emissive material (no lean group)."""
    runs = [("default", "C3", 128, {}), ("knob0", "C3", 128, {"RT_ROW_COMPACT": "0"}), ("emissive", "emissive", 128, {})]
    stats, imgs, rows, kept2 = _child(tmp_path, runs)
    assert all(len(rows[t]) == 2 for t, *_ in runs), rows
    for (enabled, hits, cap, claimed, compact), kept in zip(rows["default"], kept2["default"]):
        assert enabled == 1 and compact == 1 and cap == 64 * W * H // 4, rows
        assert 0 < kept <= claimed == hits <= cap, (rows, kept2)
    assert all(r[0] == 0 and r[3] == 0 and r[4] == 0 for r in rows["knob0"] + rows["emissive"]), rows
    assert imgs["default"].tobytes() == imgs["knob0"].tobytes() and stats["default"] == stats["knob0"]
