"""One camera traversal per pixel and frame group (WFParams::cam_shared, csrc/hip/rt_wavefront.h):
a group of several frames traces each work item's camera ray once, into frame 0's result slot, and
every frame's pass-0 shade reads that slot; the other frames' pass-0 result slots are never written.
Every case equals the oracle bit for bit over the whole image (or the rank's share of it), with the
oracle's ray count: rt_stats.rays still counts one camera ray per sample.

The renderer is this module's own (its finisher settings and path-state size are the module's)."""
import dataclasses

import numpy as np
import pytest

from helpers import bit_mismatch, frames_for, oracle_render
from rtamd import configs as cf
from rtamd import scene_lib as sl
from rtamd import tiling
from rtamd.renderer import RT_FLAG_COUNT_VISITS, RT_FLAG_NO_FINISH, RT_FLAG_SERIAL, Renderer

pytestmark = pytest.mark.gpu

W, H = 24, 16  # 384 pixels: a wave of 64 lanes holds fewer than one pixel's 65 frames, or 0.5 / 4 pixels' 128 / 16
B = cf.frame_params(W, H).max_bounce  # passes 0 .. B
FINISH_DEFAULT = (2, 8 << 20)


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


_refs = {}


def _oracle(key, sd, env_maps, width, height, frames, **window):
    """Oracle image and counters, computed once per key and left unchanged."""
    if key not in _refs:
        img, cnt = oracle_render(sd, env_maps, width, height, frames, **window)
        img.setflags(write=False)
        _refs[key] = (img, cnt)
    return _refs[key]


def _ref(config, env_maps, w, h, n, fp=None, tag=""):
    fp = fp or cf.frame_params(w, h)
    ro, frames = frames_for(fp, 1, n)
    img, cnt = _oracle((config, w, h, n, tag), cf.config_scene(config), env_maps, w, h, frames)
    return fp, ro, img, cnt


def _setup(r, sd, env_maps, w, h, bulk, tile=32, rank=0, world=1):
    """Scene, frame and a fresh accumulation; bulk: every group above the finisher's slot limit (the
    bulk kernels in every pass, as in test_bulk_groups_run_every_pass)."""
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env_maps)
    r.resize(w, h, tile=tile, rank=rank, world=world)
    r.set_finish(*((2, 1) if bulk else FINISH_DEFAULT))
    r.clear_accum()
    r.set_loop_num(0)
    r.reset_stats()


def _render(r, sd, env_maps, w, h, fp, ro, bulk, **kw):
    try:
        _setup(r, sd, env_maps, w, h, bulk, **kw)
        st = r.render(fp, ro)
        return r.read_accum(), st
    finally:
        r.set_finish(*FINISH_DEFAULT)


# ------------------------------------------------------------------ 1, 2: bulk CAM groups
@pytest.mark.parametrize("config,n", [("C3", 130), ("C3", 128), ("C4", 128)])
def test_bulk_camera_groups(renderer, env_maps, config, n):
    """Two bulk groups of 65 / 64 frames: a shade block's waves straddle pixels at 65 frames per
    pixel; wf_shade<..., CAM> builds every pixel's record from the one shared result.  C4's camera
    hits are refractive: WFState::org and pass 1's 16-B rays start from that hit."""
    fp, ro, ref, cnt = _ref(config, env_maps, W, H, n)
    img, st = _render(renderer, cf.config_scene(config), env_maps, W, H, fp, ro, bulk=True)
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == cnt["rays"], st
    assert st["samples"] == cnt["samples"] == n * W * H, st
    assert st["launches"] == 1 and st["trace_launches"] == 2 * (B + 1), st
    assert st["finish_steps"] == 0, st


# ------------------------------------------------------------------ 3: bulk groups below 64 frames
def test_bulk_groups_below_64_frames(renderer, env_maps):
    """16 frames in two bulk groups of 8: the `bulk` shade (no camera records) reads its pixel's
    result in pass 0."""
    fp, ro, ref, cnt = _ref("C3", env_maps, W, H, 16)
    img, st = _render(renderer, cf.config_scene("C3"), env_maps, W, H, fp, ro, bulk=True)
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == cnt["rays"], st
    assert st["trace_launches"] == 2 * (B + 1) and st["finish_steps"] == 0, st


# ------------------------------------------------------------------ 4: small multi-frame groups
@pytest.fixture(scope="module")
def small_refs(env_maps):
    """Oracle image and ray count after 3 and 6 progressive frames of C3 at 96 x 72 (the second
    continues the first one's accumulation)."""
    w, h = 96, 72
    sd = cf.config_scene("C3")
    ro, frames = frames_for(cf.frame_params(w, h), 1, 6)
    a3, c3 = oracle_render(sd, env_maps, w, h, frames[:3])
    a6, c6 = oracle_render(sd, env_maps, w, h, frames[3:], accum=a3)
    return {3: (a3, c3["rays"]), 6: (a6, c3["rays"] + c6["rays"])}


@pytest.mark.parametrize("flags", [0, RT_FLAG_NO_FINISH])
@pytest.mark.parametrize("n", [3, 6])
def test_small_multi_frame_groups(renderer, env_maps, small_refs, n, flags):
    """Groups of 1 + 2 and 3 + 3 frames below the finisher's limit: the plain shade reads the
    pixel's result in pass 0, then wf_finish (or, with RT_FLAG_NO_FINISH, every pass) runs."""
    w, h = 96, 72
    fp = cf.frame_params(w, h, flags=flags)
    img, st = _render(renderer, cf.config_scene("C3"), env_maps, w, h, fp, cf.rand_origins(n), bulk=False)
    ref, rays = small_refs[n]
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == rays, st
    assert (st["finish_steps"] == 0) == (flags == RT_FLAG_NO_FINISH), st


# ------------------------------------------------------------------ 5: stale results
@pytest.mark.parametrize("bulk", [True, False])
def test_second_camera_sees_no_result_of_the_first(renderer, env_maps, bulk):
    """Two renders of the same size on one renderer, the second from another camera position: the
    pass-0 result slots of frames >= 1 still hold the first call's hits (or older values), so any
    reader of an unwritten pass-0 result would shade the first camera's triangles."""
    sd = cf.config_scene("C3")
    fp, ro, ref, cnt = _ref("C3", env_maps, W, H, 128)
    img, st = _render(renderer, sd, env_maps, W, H, fp, ro, bulk)
    assert bit_mismatch(img, ref)[0] == 0.0
    pos = [float(np.float32(p) + np.float32(d)) for p, d in zip(fp.position, (0.35, 0.15, -0.25))]
    fp2, ro2, ref2, cnt2 = _ref("C3", env_maps, W, H, 128, fp=dataclasses.replace(fp, position=pos), tag="moved")
    assert bit_mismatch(ref2, ref)[0] > 0.5  # (another view: most pixels differ)
    img2, st2 = _render(renderer, sd, env_maps, W, H, fp2, ro2, bulk)
    assert bit_mismatch(img2, ref2)[0] == 0.0
    assert st2["rays"] == cnt2["rays"], st2


# ------------------------------------------------------------------ 6: rank shares, padded tiles
@pytest.mark.parametrize("bulk", [True, False])
def test_rank_share_with_padded_tiles(renderer, env_maps, bulk):
    """40 x 24 in 16 x 16 tiles, rank 1 of 3: tiles 1 (full) and 4 (16 x 8 of it inside the frame),
    64 frames; the rank's pixels equal the oracle's, the others stay 0."""
    w, h, T, rank, world, n = 40, 24, 16, 1, 3, 64
    sd = cf.config_scene("C3")
    fp = cf.frame_params(w, h)
    ro, frames = frames_for(fp, 1, n)
    mine = tiling.local_tiles(w, h, T, T, rank, world)
    assert len(mine) == 2
    ref, rays = np.zeros((h, w, 3), np.float32), 0
    for t in mine:
        x0, y0, tw, th = tiling.tile_rect(int(t), w, h, T, T)
        acc, cnt = _oracle(("C3", w, h, n, "tile", int(t)), sd, env_maps, w, h, frames, x0=x0, y0=y0, w=tw, h=th)
        ref[y0:y0 + th, x0:x0 + tw] = acc
        rays += cnt["rays"]
    assert any(tiling.tile_rect(int(t), w, h, T, T)[3] < T for t in mine)  # a partly filled tile
    try:
        img, st = _render(renderer, sd, env_maps, w, h, fp, ro, bulk, tile=T, rank=rank, world=world)
    finally:
        renderer.resize(W, H)
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == rays, st


# ------------------------------------------------------------------ 7: empty scene
@pytest.mark.parametrize("bulk", [True, False])
def test_empty_scene(renderer, env_maps, bulk):
    """No mesh: every camera ray misses in wf_trace's early-out, which writes the one result per
    work item; 64 frames of the environment."""
    s = sl.Scene()
    s.build_bvh(8)
    tri, nodes = s.encode()
    sd = cf.SceneData("empty", s.counts(), tri, nodes, s.export_soa(), s.nodes(), [])
    w, h, n = 32, 16, 64
    fp = cf.frame_params(w, h, enable_env_map=True)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = _oracle(("empty", w, h, n), sd, env_maps, w, h, frames)
    img, st = _render(renderer, sd, env_maps, w, h, fp, ro, bulk)
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == cnt["rays"] == n * w * h, st


# ------------------------------------------------------------------ 8: split calls agree
@pytest.mark.parametrize("bulk", [True, False])
@pytest.mark.parametrize("flags", [0, RT_FLAG_SERIAL])
def test_two_calls_of_64_equal_one_of_128(renderer, env_maps, flags, bulk):
    sd = cf.config_scene("C3")
    _, ro, ref, cnt = _ref("C3", env_maps, W, H, 128)
    fp = cf.frame_params(W, H, flags=flags)
    one, st1 = _render(renderer, sd, env_maps, W, H, fp, ro, bulk)
    try:
        _setup(renderer, sd, env_maps, W, H, bulk)
        renderer.render(fp, ro[:64])
        st2 = renderer.render(fp, ro[64:])
        two = renderer.read_accum()
    finally:
        renderer.set_finish(*FINISH_DEFAULT)
    assert bit_mismatch(one, two)[0] == 0.0
    assert bit_mismatch(one, ref)[0] == 0.0
    assert st1["rays"] == st2["rays"] == cnt["rays"], (st1, st2)


# ------------------------------------------------------------------ 9: counting runs
def test_counting_runs_trace_every_path_slot(renderer, env_maps):
    """RT_FLAG_COUNT_VISITS keeps one traversal per path slot: the step counters of a 4-frame call
    are the sums of four one-frame calls of the same frames (integers, the same rays).

    Checked on the parent commit's library first, as the counters' determinism was an assumption:
    it holds there too (the one-frame calls run pixel groups, the 4-frame call frame groups; the
    counters are sums over rays either way)."""
    sd = cf.config_scene("C3")
    n = 4
    fp, ro, ref, cnt = _ref("C3", env_maps, W, H, n)
    fpc = dataclasses.replace(fp, flags=RT_FLAG_COUNT_VISITS)
    img, st = _render(renderer, sd, env_maps, W, H, fpc, ro, bulk=False)
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == cnt["rays"], st
    _setup(renderer, sd, env_maps, W, H, bulk=False)
    for k in range(n):
        assert renderer.loop_num == k
        st1 = renderer.render(fpc, ro[k:k + 1])  # (the stats accumulate until reset_stats)
    assert bit_mismatch(renderer.read_accum(), ref)[0] == 0.0
    assert st1["rays"] == cnt["rays"], st1
    for key in ("internal_pops", "leaf_pops", "tri_tests"):
        assert st[key] == st1[key] > 0, (key, st, st1)
