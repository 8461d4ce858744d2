"""The motion mode of the temporal stage (rt_abi.h rt_temporal_set_motion) on the GPU against the numpy
model of tests/temporal_motion_model.py, bit for bit.

The cases of tests/temporal_motion_cases.py run through the library on their real small scenes:
rt_set_scene, rt_update_geometry, the library's own first-hit trace, the poses the model compares
read back with rt_scene_download; every analytic assertion of a case holds for the GPU's frames too.
The other tests run C3 at 64 x 36 with the loong turning.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import denoise_model as dm
import oracle as orc
import temporal_cases as tc
import temporal_model as tm
import temporal_motion_cases as mc
import temporal_motion_model as mm
from rtamd import configs as cf
from rtamd import geometry as geo
from rtamd import interactive as ia
from rtamd.renderer import (RT_ERR_ARG, RT_ERR_STATE, RT_OK, RT_TEMPORAL_REUSE_GUIDES, DenoiseParams, RtTemporalParams,
                            TemporalParams)
from test_gpu_temporal import MOVES, bits, device_floats, fp_of, same, tiled

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {k: SimpleNamespace(W=w, H=h, tile=t) for k, (w, h, t) in tc.SIZES.items()}


@pytest.fixture
def r(gpu_renderer):
    """The shared context, left in the default mode"""
    try:
        yield gpu_renderer
    finally:
        gpu_renderer.set_pipeline(1)
        gpu_renderer.set_temporal_motion(False)


@pytest.fixture(scope="module")
def c3(env_maps):
    return SimpleNamespace(sd=cf.config_scene("C3"), env=env_maps)


def pose(r):
    return r.scene_download("tri"), r.scene_download("trin")


# ------------------------------------------------------------------ the cases
class GpuStage:
    """A stage of tests/temporal_motion_cases.py on the library, every call checked against the model"""

    def __init__(self, r, z, motion):
        self.r, self.z, self.motion = r, z, motion
        self.model = mm.MotionTemporal() if motion else tm.Temporal()
        self.own = None

    def load(self, scene):
        self.r.set_temporal_motion(self.motion)
        assert self.r.get_temporal_motion() == self.motion
        self.r.set_scene_soa(scene.soa, scene.nodes)
        self.model.drop()

    def update(self, idx, p, n):
        self.r.update_geometry(idx, p, n)

    def first_hit(self, fp, W, H):
        self.own = self.r.first_hit(fp)
        return self.own

    def resize(self):
        self.r.resize(self.z.W, self.z.H, tile=self.z.tile)
        self.model.drop()

    def call(self, color, hits, fp, tp, advance=False, reset=False, reuse=False):
        import torch
        r, z = self.r, self.z
        d_frame = torch.from_numpy(np.ascontiguousarray(color, F)).cuda()
        d_hits = None
        if not reuse and hits is not self.own:  # a caller's frame; else the library traces its own
            d_hits = torch.from_numpy(tiled(hits, z.tile).view(np.uint8)).cuda()
        torch.cuda.synchronize()  # torch's stream filled the buffers the ctx stream uses
        p = TemporalParams(tp.samples, tp.max_history, tp.sigma_normal, tp.sigma_plane)
        out = r.temporal_async(fp, p, frame_ptr=d_frame.data_ptr(), hits_ptr=d_hits.data_ptr() if d_hits is not None else None,
                               advance=advance, reset=reset, reuse_guides=reuse)
        got = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
        n = r.temporal_history()
        if self.motion:
            want = self.model.call(color, hits, fp, tp, pose(r), advance=advance, reset=reset)
        else:
            want = self.model.call(color, hits, fp, tp, advance=advance, reset=reset)
        same(got, n, *want)
        return got, n


@pytest.mark.parametrize("case", list(mc.CASES))
@pytest.mark.parametrize("name", list(SIZES))
def test_cases(r, name, case):
    z = SIZES[name]
    r.set_pipeline(1)
    r.resize(z.W, z.H, tile=z.tile)
    mc.CASES[case](name, GpuStage(r, z, True), GpuStage(r, z, False))


# ------------------------------------------------------------------ C3 with the loong turning
def prepare(r, c3, name="64x36"):
    z = SIZES[name]
    r.set_pipeline(1)
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    r.resize(z.W, z.H, tile=z.tile)
    return z


def turned(sd, degrees):
    """(tri_index, p, n) of C3's last object (the loong) turned about the vertical axis"""
    k = len(sd.objects) - 1
    o = sd.objects[k]
    return geo.moved_object(sd, k, (o.rotate[0], o.rotate[1] + degrees, o.rotate[2]), o.translate, o.scale)


def test_real_mesh_chain_equals_the_model(r, c3):
    """Four views of C3 at 64 x 36, the loong turned by 4 degrees more before each but the first (and the
    camera moved): render, update, temporal with ADVANCE, denoise on its output; then a second frame of
    the last view with REUSE_GUIDES.  Outputs and history lengths equal the model's, the denoised frame
    the denoiser model's, on a mesh with interpolated normals; most moved pixels keep a history."""
    z = prepare(r, c3)
    r.set_temporal_motion(True)
    model = mm.MotionTemporal()
    cam = ia.Camera(float(F(z.W) / F(z.H)))
    for k in range(4):
        if k:
            MOVES[k - 1](cam)
            r.update_geometry(*turned(c3.sd, 4.0 * k))
        fp = fp_of(cam)
        r.reset()
        r.clear_accum()
        r.render(fp, cf.rand_origins(1, k))
        acc, hits = r.read_accum(), r.first_hit(fp)
        out = r.temporal_async(fp, TemporalParams(samples=1), advance=True)
        got = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
        want, wn = model.call(acc, hits, fp, TemporalParams(samples=1), pose(r), advance=True)
        same(got, r.temporal_history(), want, wn)
        dn = r.denoise_async(fp, DenoiseParams(), frame_ptr=out, reuse_guides=True)
        got = device_floats(r, dn, z.W * z.H * 3).reshape(z.H, z.W, 3)
        assert np.array_equal(bits(got), bits(dm.denoise(want, hits, DenoiseParams())))
        if k:
            assert model.moved.sum() >= 100 and not model.failed.any(), (k, model.moved.sum(), model.failed.sum())
            assert (model.has & model.moved).sum() > 0.5 * model.moved.sum(), (k, (model.has & model.moved).sum(), model.moved.sum())
    r.render(fp, cf.rand_origins(1, 9))
    acc = r.read_accum()
    got = r.temporal(fp, TemporalParams(samples=2), reuse_guides=True)
    want, wn = model.call(acc, hits, fp, TemporalParams(samples=2), pose(r))
    same(got, r.temporal_history(), want, wn)
    assert model.moved.sum() >= 100


def test_entry_points_agree(r):
    """rt_temporal on the accumulation with the library's own trace and a host-array update gives the
    bytes of rt_temporal_async on a caller's frame and first-hit buffer with the device form of the update."""
    import torch
    z = SIZES["70x37"]
    r.resize(z.W, z.H, tile=z.tile)
    scene = mc.CaseScene()
    fp = mc.still_camera(z.W, z.H)
    p, n = scene.card_moved((2.37 * mc.px_at(fp, z.W, 4.0), 0.0, 0.0), yaw_deg=15.0)
    c1, c2 = mc.colours(z.H, z.W, 41), mc.colours(z.H, z.W, 42)
    r.set_temporal_motion(True)
    r.set_scene_soa(scene.soa, scene.nodes)
    r.write_accum(c1)
    a1 = r.temporal(fp, advance=True, reset=True)
    r.update_geometry(scene.card, p, n)
    r.write_accum(c2)
    a2, an = r.temporal(fp, advance=True), r.temporal_history()
    assert (an == 2).sum() >= 100
    r.set_scene_soa(scene.soa, scene.nodes)
    outs = []
    for k, c in enumerate((c1, c2)):
        if k:
            r.update_geometry(torch.from_numpy(scene.card).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda())
        d_frame = torch.from_numpy(c).cuda()
        d_hits = torch.from_numpy(tiled(r.first_hit(fp), z.tile).view(np.uint8)).cuda()
        torch.cuda.synchronize()
        out = r.temporal_async(fp, frame_ptr=d_frame.data_ptr(), hits_ptr=d_hits.data_ptr(), advance=True)
        outs.append(device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3))
    assert np.array_equal(bits(outs[0]), bits(a1)) and np.array_equal(bits(outs[1]), bits(a2))
    assert np.array_equal(r.temporal_history(), an)


def test_state_is_untouched(r, c3):
    z = prepare(r, c3)
    fp = cf.frame_params(z.W, z.H)

    def frame():
        r.reset()
        r.clear_accum()
        r.render(fp, cf.rand_origins(1))
        return r.read_accum().tobytes()

    plain = frame()
    r.set_temporal_motion(True)
    assert r.get_temporal_motion() is True
    assert frame() == plain
    before = (r.loop_num, r.read_accum().tobytes(), r.stats())
    r.temporal(fp, advance=True)
    r.update_geometry(*turned(c3.sd, 3.0))
    after_update = (r.loop_num, r.read_accum().tobytes(), r.stats())
    assert after_update == before
    r.temporal(fp, advance=True)
    r.temporal_async(fp, reuse_guides=True)
    r.temporal_history()
    r.set_temporal_motion(False)
    assert (r.loop_num, r.read_accum().tobytes(), r.stats()) == before and r.get_temporal_motion() is False


def _raw(r, fp, tp, buf):
    p = fp.to_c()
    return r._L.rt_temporal(r._h, C.byref(p), C.byref(tp), buf.ctypes.data_as(C.POINTER(C.c_float)))


def test_errors(r, c3):
    z = prepare(r, c3)
    fp = cf.frame_params(z.W, z.H)
    buf = np.zeros((z.H, z.W, 3), F)
    on = C.c_int32(7)
    for bad in (2, -1, 256):
        assert r._L.rt_temporal_set_motion(r._h, bad) == RT_ERR_ARG
    assert r._L.rt_temporal_get_motion(r._h, C.byref(on)) == RT_OK and on.value == 0
    assert r._L.rt_temporal_get_motion(r._h, None) == RT_ERR_ARG
    assert r._L.rt_temporal_set_motion(None, 1) == RT_ERR_ARG
    ok = TemporalParams().to_c()
    reuse = TemporalParams().to_c(RT_TEMPORAL_REUSE_GUIDES)
    assert _raw(r, fp, ok, buf) == RT_OK and _raw(r, fp, reuse, buf) == RT_OK   # guides packed with the mode off
    assert r._L.rt_temporal_set_motion(r._h, 1) == RT_OK
    assert _raw(r, fp, reuse, buf) == RT_ERR_STATE                             # ... carry no triangle frame
    assert _raw(r, fp, ok, buf) == RT_OK and _raw(r, fp, reuse, buf) == RT_OK
    r.denoise(fp)                                                              # a fresh pack by the denoiser stores it too
    assert _raw(r, fp, reuse, buf) == RT_OK
    for flags in (8, 17):
        assert _raw(r, fp, RtTemporalParams(1, 32, 0.3, 0.01, flags), buf) == RT_ERR_ARG
    try:
        r.resize(z.W, z.H, tile=16, rank=0, world=2)
        assert r.get_temporal_motion() is True                                 # (the setting survives a resize)
        assert _raw(r, fp, ok, buf) == RT_ERR_STATE
    finally:
        r.resize(z.W, z.H)
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    assert r.get_temporal_motion() is True and _raw(r, fp, ok, buf) == RT_OK


# ------------------------------------------------------------------ interactive loop
@pytest.mark.parametrize("denoise", [False, True])
def test_session_follows_the_turning_loong(r, c3, denoise):
    """still, the loong turned, still with enable_temporal and enable_temporal_motion: each image is the
    oracle's display of the model's chain (then the denoiser model when that is on) on that tick's
    accumulation, first-hit frame and pose; the tick after the update reuses its guides."""
    W, H = 64, 36
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    s = ia.Session(r, W, H, settings=ia.Settings(max_bounce=4, enable_temporal=True, enable_temporal_motion=True,
                                                 enable_denoise=denoise))
    r.clear_accum()
    model = mm.MotionTemporal()
    moved = []
    for inp in (ia.Input(), ia.Input(geometry=[turned(c3.sd, 5.0)]), ia.Input()):
        out = s.tick(inp, delta_time=0.05)
        fp, hits = out["params"], r.first_hit(out["params"])
        want, _ = model.call(r.read_accum(), hits, fp, TemporalParams(samples=out["loop_num"]), pose(r), advance=out["loop_num"] == 1)
        moved.append((int(model.moved.sum()), int((model.moved & model.has).sum())))
        if denoise:
            want = dm.denoise(want, hits, DenoiseParams())
        assert np.array_equal(out["image"], orc.display(want, out["display_flags"]))
    assert r.get_temporal_motion() is True
    assert moved[0] == (0, 0) and min(moved[1][0], moved[2][0]) >= 100 and moved[1][1] > 0.5 * moved[1][0], moved
