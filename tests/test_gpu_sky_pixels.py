"""Camera-miss pixels once per frame group (WFParams::cam_miss_once, csrc/hip/rt_wavefront.h): in a
bulk group of >= 64 frames wf_cam_classify stores a miss pixel's colour once (WFState::org) and
lists the hit pixels, wf_shade<..., CAM> runs over the listed pixels' frames only, and wf_blend
blends a miss pixel from its record.  Every case equals the oracle bit for bit over the whole
image (or the rank's share), with the oracle's `rays` and `samples` and pass0_steps == samples; a
case that depends on how many pixels miss asserts that with rt_first_hit first.

The renderer is this module's own (its finisher settings and path-state size are the module's)."""
import dataclasses

import numpy as np
import pytest

from helpers import bit_mismatch, frames_for, oracle_render
from rtamd import configs as cf
from rtamd import scene_lib as sl
from rtamd import tiling
from rtamd.renderer import Renderer, dev_lib_path

pytestmark = pytest.mark.gpu

W, H = 24, 16  # 384 pixels; a CAM block-iteration (2048 paths) spans 32 pixels' 64 frames, or 31.5 pixels' 65
FINISH_DEFAULT = (2, 8 << 20)


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


_refs = {}


def _oracle(key, sd, env_maps, width, height, frames, **kw):
    """Oracle image and counters, computed once per key and left unchanged."""
    if key not in _refs:
        img, cnt = oracle_render(sd, env_maps, width, height, frames, **kw)
        img.setflags(write=False)
        _refs[key] = (img, cnt)
    return _refs[key]


def _empty_scene():
    s = sl.Scene()
    s.build_bvh(8)
    tri, nodes = s.encode()
    return cf.SceneData("empty", s.counts(), tri, nodes, s.export_soa(), s.nodes(), [])


def _setup(r, sd, env_maps, w, h, tile=32, rank=0, world=1):
    """Scene, frame, a fresh accumulation and the finisher limit at one slot: every group is a bulk
    group.  The caller restores the finisher setting."""
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env_maps)
    r.resize(w, h, tile=tile, rank=rank, world=world)
    r.set_finish(2, 1)
    r.clear_accum()
    r.set_loop_num(0)
    r.reset_stats()


def _misses(r, fp):
    """Camera rays of this rank's pixels that leave the scene (other ranks' pixels read as hits)."""
    return int((r.first_hit(fp)["triangle"] < 0).sum())


def _render(r, sd, env_maps, w, h, fp, ro, **kw):
    """(image, stats, camera misses of the view)"""
    try:
        _setup(r, sd, env_maps, w, h, **kw)
        misses = _misses(r, fp)
        st = r.render(fp, ro)
        return r.read_accum(), st, misses
    finally:
        r.set_finish(*FINISH_DEFAULT)


def _check(img, st, ref, cnt):
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == cnt["rays"], st
    assert st["samples"] == cnt["samples"], st
    assert st["pass0_steps"] == st["samples"], st
    assert st["samples"] <= st["path_steps"] <= st["rays"], st


def _down_view(w, h):
    """One unit above the floor beside the mesh, looking down: the floor fills the frame."""
    cam = sl.camera(-90.0, -89.0, 30.0, w / h)
    return cf.frame_params(w, h, position=(7.0, -1.0, 3.0), **cam)


# ------------------------------------------------------------------ 1: mixed view
@pytest.mark.parametrize("n", [128, 130])
def test_mixed_view(renderer, env_maps, n):
    """C3, two groups of 64 / 65 frames: at 65 the hit list's items of a block-iteration do not
    divide by the frame count (a pixel's frames straddle two block-iterations)."""
    sd = cf.config_scene("C3")
    fp = cf.frame_params(W, H)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", W, H, n), sd, env_maps, W, H, frames)
    img, st, misses = _render(renderer, sd, env_maps, W, H, fp, ro)
    assert 0 < misses < W * H
    _check(img, st, ref, cnt)
    assert st["samples"] == n * W * H, st


# ------------------------------------------------------------------ 2: every pixel misses
@pytest.mark.parametrize("env_on", [True, False])
def test_every_pixel_misses(renderer, env_maps, env_on):
    """The empty scene, with the environment map and with the default sky colour: the hit list is
    empty, the CAM shade and every later pass have no work, the blend runs from records alone."""
    sd = _empty_scene()
    w, h, n = 32, 16, 64
    fp = cf.frame_params(w, h, enable_env_map=env_on)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("empty", w, h, n, env_on), sd, env_maps, w, h, frames)
    try:
        img, st, misses = _render(renderer, sd, env_maps, w, h, fp, ro)
    finally:
        renderer.resize(W, H)
    assert misses == w * h
    _check(img, st, ref, cnt)
    assert st["rays"] == st["samples"] == n * w * h, st
    assert st["pass1_steps"] == 0, st


# ------------------------------------------------------------------ 3: no pixel misses
def test_no_pixel_misses(renderer, env_maps):
    """The floor fills the frame: the list holds every pixel and no record colour is used."""
    sd = cf.config_scene("C3")
    n = 64
    fp = _down_view(W, H)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", W, H, n, "down"), sd, env_maps, W, H, frames)
    img, st, misses = _render(renderer, sd, env_maps, W, H, fp, ro)
    assert misses == 0
    _check(img, st, ref, cnt)


# ------------------------------------------------------------------ 4: stale records
def test_second_camera_sees_no_record_of_the_first(renderer, env_maps):
    """Two renders on one renderer from different camera positions: the records and the hit list of
    the first view are still in the path-state set when the second view's groups start."""
    sd = cf.config_scene("C3")
    n = 128
    fp = cf.frame_params(W, H)
    pos = [float(np.float32(p) + np.float32(d)) for p, d in zip(fp.position, (0.35, 0.15, -0.25))]
    fp2 = dataclasses.replace(fp, position=pos)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", W, H, n), sd, env_maps, W, H, frames)
    ref2, cnt2 = _oracle(("C3", W, H, n, "moved"), sd, env_maps, W, H, frames_for(fp2, 1, n)[1])
    try:
        _setup(renderer, sd, env_maps, W, H)
        m1 = renderer.first_hit(fp)["triangle"] < 0
        m2 = renderer.first_hit(fp2)["triangle"] < 0
        assert (m1 & ~m2).any() and (~m1 & m2).any()  # miss -> hit and hit -> miss
        st = renderer.render(fp, ro)
        _check(renderer.read_accum(), st, ref, cnt)
        _setup(renderer, sd, env_maps, W, H)
        st2 = renderer.render(fp2, ro)
        _check(renderer.read_accum(), st2, ref2, cnt2)
    finally:
        renderer.set_finish(*FINISH_DEFAULT)


# ------------------------------------------------------------------ 5: rank share, padded tiles
def test_rank_share_with_padded_tiles(renderer, env_maps):
    """40 x 24 in 16 x 16 tiles, rank 1 of 3: tiles 1 (full) and 4 (16 x 8 of it inside the frame),
    64 frames; the rank's pixels equal the oracle's, the others stay 0."""
    w, h, T, rank, world, n = 40, 24, 16, 1, 3, 64
    sd = cf.config_scene("C3")
    fp = cf.frame_params(w, h)
    ro, frames = frames_for(fp, 1, n)
    mine = tiling.local_tiles(w, h, T, T, rank, world)
    assert len(mine) == 2
    ref, cnt, own = np.zeros((h, w, 3), np.float32), {"rays": 0, "samples": 0}, np.zeros((h, w), bool)
    for t in mine:
        x0, y0, tw, th = tiling.tile_rect(int(t), w, h, T, T)
        acc, c = _oracle(("C3", w, h, n, "tile", int(t)), sd, env_maps, w, h, frames, x0=x0, y0=y0, w=tw, h=th)
        ref[y0:y0 + th, x0:x0 + tw] = acc
        own[y0:y0 + th, x0:x0 + tw] = True
        cnt["rays"] += c["rays"]
        cnt["samples"] += c["samples"]
    assert any(tiling.tile_rect(int(t), w, h, T, T)[3] < T for t in mine)  # a partly filled tile
    try:
        _setup(renderer, sd, env_maps, w, h, tile=T, rank=rank, world=world)
        miss = (renderer.first_hit(fp)["triangle"] < 0) & own
        assert 0 < int(miss.sum()) < int(own.sum())
        st = renderer.render(fp, ro)
        img = renderer.read_accum()
    finally:
        renderer.set_finish(*FINISH_DEFAULT)
        renderer.resize(W, H)
    _check(img, st, ref, cnt)
    assert not img[~own].any()


# ------------------------------------------------------------------ 6: history
def test_blend_continues_a_stored_history(renderer, env_maps):
    """A non-zero accumulation and loop count, then 64 frames twice: two calls of 64 equal one call
    of 128 and the oracle continued from that history (the constant-colour chain of a miss pixel
    starts from the stored history with the frames' own weights)."""
    sd = cf.config_scene("C3")
    n, loop0 = 128, 5
    fp = cf.frame_params(W, H)
    hist = (np.random.default_rng(7).random((H, W, 3), np.float32) * 2.0 + 0.25).astype(np.float32)
    ro, frames = frames_for(fp, loop0 + 1, n)
    ref, cnt = _oracle(("C3", W, H, n, "history"), sd, env_maps, W, H, frames, accum=hist.copy())

    def start():
        _setup(renderer, sd, env_maps, W, H)
        renderer.write_accum(hist)
        renderer.set_loop_num(loop0)

    try:
        start()
        assert 0 < _misses(renderer, fp) < W * H
        st1 = renderer.render(fp, ro)
        one = renderer.read_accum()
        start()
        renderer.render(fp, ro[:64])
        st2 = renderer.render(fp, ro[64:])  # (the stats accumulate until reset_stats)
        two = renderer.read_accum()
    finally:
        renderer.set_finish(*FINISH_DEFAULT)
    assert renderer.loop_num == loop0 + n
    assert bit_mismatch(one, two)[0] == 0.0
    _check(one, st1, ref, cnt)
    _check(two, st2, ref, cnt)


# ------------------------------------------------------------------ 7: two bulk calls in flight
def test_two_pipelined_bulk_calls(renderer, env_maps):
    """rt_set_pipeline(2) and two consecutive 64-frame calls above the finisher limit: each runs as
    one bulk group on its own path-state set, with its own records and hit list."""
    sd = cf.config_scene("C3")
    n = 128
    fp = cf.frame_params(W, H)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", W, H, n), sd, env_maps, W, H, frames)
    try:
        _setup(renderer, sd, env_maps, W, H)
        assert 0 < _misses(renderer, fp) < W * H
        renderer.set_pipeline(2)
        renderer.render_async(fp, ro[:64])
        renderer.render_async(fp, ro[64:])
        renderer.synchronize()
        st = renderer.stats()
        img = renderer.read_accum()
    finally:
        renderer.set_pipeline(1)
        renderer.set_finish(*FINISH_DEFAULT)
    _check(img, st, ref, cnt)
    assert st["launches"] == 2, st


# ------------------------------------------------------------------ 8: switch off equals switch on
def test_switch_off_equals_switch_on(env_maps, monkeypatch):
    """The development library with RT_CAM_MISS_ONCE=0 (every frame of a miss pixel shaded and
    blended from its fin row) gives the image and counters of the default."""
    try:
        path = dev_lib_path()
    except FileNotFoundError:
        pytest.skip("lib/librtamd_dev.so is not built")
    sd = cf.config_scene("C3")
    n = 130
    fp = cf.frame_params(W, H)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("C3", W, H, n), sd, env_maps, W, H, frames)
    r = Renderer(0, lib_path=path)
    try:
        monkeypatch.delenv("RT_CAM_MISS_ONCE", raising=False)
        on, st_on, misses = _render(r, sd, env_maps, W, H, fp, ro)
        monkeypatch.setenv("RT_CAM_MISS_ONCE", "0")
        off, st_off, _ = _render(r, sd, env_maps, W, H, fp, ro)
    finally:
        r.close()
    assert 0 < misses < W * H
    assert bit_mismatch(on, off)[0] == 0.0
    _check(on, st_on, ref, cnt)
    _check(off, st_off, ref, cnt)
    for key in ("rays", "samples", "path_steps", "pass0_steps", "pass1_steps", "p1_rays", "trace_launches", "launches"):
        assert st_on[key] == st_off[key], (key, st_on, st_off)
