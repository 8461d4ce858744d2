"""The variance mode of the display chain (rt_abi.h rt_variance_*) on the GPU against the numpy model of
tests/variance_model.py, bit for bit: the temporal stage's output, history lengths and variance, then
the denoiser's output and variance on that output, call by call.

Every case runs C3; the model's inputs are the GPU's own read_accum() and first_hit(fp).  Two sizes:

  70 x 37, tile 16   the denoiser's odd size (partial blocks in both axes); 12 NaN / inf pixels planted
  33 x 17, tile 16   one block and a partial one per axis, smaller than the halos of s = 8 and 16, so
                     every residue-class block of those iterations is partial
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import denoise_model as dm
import oracle as orc
import temporal_model as tm
import variance_model as vm
from rtamd import configs as cf
from rtamd import interactive as ia
from rtamd.renderer import RT_ERR_ARG, RT_ERR_STATE, RT_OK, DenoiseParams, RtVarianceParams, TemporalParams, VarianceParams
from test_gpu_temporal import MOVES, bits, device_floats, fp_of, same
from test_gpu_temporal_motion import pose, turned

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {"70x37": SimpleNamespace(W=70, H=37, tile=16, plant=True), "33x17": SimpleNamespace(W=33, H=17, tile=16, plant=False)}
PARAMS = {"it1": DenoiseParams(iterations=1), "it5": DenoiseParams()}
VP = VarianceParams(on=True)


@pytest.fixture
def r(gpu_renderer):
    """The shared context, left in the default modes"""
    try:
        yield gpu_renderer
    finally:
        gpu_renderer.set_pipeline(1)
        gpu_renderer.set_temporal_motion(False)
        gpu_renderer.set_variance(False)


@pytest.fixture(scope="module")
def c3(env_maps):
    return SimpleNamespace(sd=cf.config_scene("C3"), env=env_maps)


def prepare(r, c3, name):
    z = SIZES[name]
    r.set_pipeline(1)
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    r.resize(z.W, z.H, tile=z.tile)
    return z


def same_var(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{len(bad)} variances differ, first (y, x) {bad[:6].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def chain(r, model, z, fp, acc, hits, S, dp, advance, reuse=False, motion=False):
    """acc as the accumulation at LoopNum S through rt_temporal_async and rt_denoise_async on its
    output: every output, the history lengths and rt_variance_frame after each stage equal the model's"""
    r.write_accum(acc)
    r.set_loop_num(S)
    tp = TemporalParams(samples=S)
    out = r.temporal_async(fp, tp, advance=advance, reuse_guides=reuse)
    got = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
    want, wn, wv = model.call(acc, hits, fp, tp, pose(r) if motion else None, advance=advance)
    same(got, r.temporal_history(), want, wn)
    same_var(r.variance_frame(), wv)
    dn = r.denoise_async(fp, dp, frame_ptr=out, reuse_guides=True)
    got = device_floats(r, dn, z.W * z.H * 3).reshape(z.H, z.W, 3)
    wd, wdv = vm.denoise(want, hits, dp, VP, wv)
    bad = np.argwhere((bits(got) != bits(wd)).any(-1))
    assert bad.size == 0, f"{len(bad)} denoised pixels differ, first (y, x) {bad[:6].tolist()}"
    same_var(r.variance_frame(), wdv)
    return SimpleNamespace(out=want, n=wn, var=wv, dn=wd, dvar=wdv)


def planted(z, acc, hits):
    return dm.plant_nonfinite(acc, hits["triangle"] >= 0)[0] if z.plant else acc


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("name", list(SIZES))
def test_still_view_equals_the_model(r, c3, name, pname):
    """A still view from an empty history, S = 1, 2, 4, 7 (uneven chunks): the first call's variance is
    unknown everywhere (the spatial estimate guides the filter), every later one adds an estimate."""
    z = prepare(r, c3, name)
    r.set_variance(VP)
    assert r.get_variance() == VP
    fp = cf.frame_params(z.W, z.H)
    model = vm.VarianceTemporal(VP)
    r.reset()
    r.clear_accum()
    hits, done = r.first_hit(fp), 0
    hit = hits["triangle"] >= 0
    for k, S in enumerate((1, 2, 4, 7)):
        r.write_accum(np.zeros((z.H, z.W, 3), F) if k == 0 else acc)
        r.set_loop_num(done)
        r.render(fp, cf.rand_origins(S - done, done))
        acc, done = r.read_accum(), S
        w = chain(r, model, z, fp, planted(z, acc, hits), hits, S, PARAMS[pname], advance=k == 0, reuse=k > 0)
        fin = np.isfinite(planted(z, acc, hits)).all(-1)
        assert (w.var[hit & fin] >= 0).all() == (k > 0) and (w.var[~hit] == -1).all()
        assert (model.cand.st[..., 3][hit & fin] == k).all()
        assert np.isfinite(w.dn[hit]).all()
    assert 0.2 < hit.mean() < 1.0


@pytest.mark.parametrize("name", list(SIZES))
def test_moving_view_equals_the_model(r, c3, name):
    """ADVANCE across two sideways camera moves, with a second frame of the middle view between them
    (the still estimator continues the reprojected chain): v and m ride the colour's taps."""
    z = prepare(r, c3, name)
    r.set_variance(VP)
    model = vm.VarianceTemporal(VP)
    cam = ia.Camera(float(F(z.W) / F(z.H)))
    seen = []
    for k in range(3):
        if k:
            MOVES[0](cam)
        fp = fp_of(cam)
        r.reset()
        r.clear_accum()
        r.render(fp, cf.rand_origins(1, 3 * k))
        acc, hits = r.read_accum(), r.first_hit(fp)
        w = chain(r, model, z, fp, planted(z, acc, hits), hits, 1, PARAMS["it5"], advance=True)
        seen.append(int((model.cand.st[..., 3] > 0).sum()))
        if k == 1:
            r.render(fp, cf.rand_origins(1, 7))
            chain(r, model, z, fp, planted(z, r.read_accum(), hits), hits, 2, PARAMS["it1"], advance=False, reuse=True)
            assert (model.cand.st[..., 3] > 1).sum() >= 0.3 * hit_count(hits)
    assert seen[0] == 0 and seen[1] >= 0.3 * hit_count(hits) and seen[2] >= seen[1] * 0.5, seen
    assert (model.cand.st[..., 3] > 2).any() and model.has.any() and not model.has.all()


def hit_count(hits):
    return int((hits["triangle"] >= 0).sum())


def test_motion_mode_equals_the_model(r, c3):
    """Motion mode, the loong turned by one rt_update_geometry between two views: the variance texels
    follow the moved triangles through the colour's taps; then a second frame of the last view."""
    z = prepare(r, c3, "70x37")
    r.set_temporal_motion(True)
    r.set_variance(VP)
    model = vm.VarianceTemporal(VP)
    fp = cf.frame_params(z.W, z.H)
    for k in range(2):
        if k:
            r.update_geometry(*turned(c3.sd, 4.0))
        r.reset()
        r.clear_accum()
        r.render(fp, cf.rand_origins(1, k))
        acc, hits = r.read_accum(), r.first_hit(fp)
        chain(r, model, z, fp, acc, hits, 1, PARAMS["it5"], advance=True, motion=True)
    assert model.moved.sum() >= 100 and (model.has & model.moved).sum() > 0.5 * model.moved.sum()
    assert (model.cand.st[..., 3][model.moved & model.has] > 0).all()
    r.render(fp, cf.rand_origins(1, 9))
    chain(r, model, z, fp, r.read_accum(), hits, 2, PARAMS["it5"], advance=False, reuse=True, motion=True)


def test_standalone_denoise_uses_the_spatial_estimate(r, c3):
    """rt_denoise on an accumulation without a temporal stage (tools/render_png.py --denoise --variance):
    the variance is the 7 x 7 estimate everywhere; constant per-material frames come back bit for bit."""
    z = prepare(r, c3, "70x37")
    r.set_variance(VP)
    fp = cf.frame_params(z.W, z.H)
    r.reset()
    r.render(fp, cf.rand_origins(3))
    hits = r.first_hit(fp)
    acc = planted(z, r.read_accum(), hits)
    r.write_accum(acc)
    want, wv = vm.denoise(acc, hits, PARAMS["it5"], VP)
    assert np.array_equal(bits(r.denoise(fp, PARAMS["it5"])), bits(want))
    same_var(r.variance_frame(), wv)
    hit = hits["triangle"] >= 0
    assert (wv[hit] >= 0).mean() > 0.9 and (wv[~hit] == -1).all() and np.isfinite(want[hit]).all()
    first = hits["material"] == hits["material"][hit][0]
    two = (np.where(first[..., None], F(2.0), F(0.5)) * np.ones((z.H, z.W, 3), F)).astype(F)
    r.write_accum(two)
    assert np.array_equal(bits(r.denoise(fp, PARAMS["it5"])), bits(two))


# ------------------------------------------------------------------ the mode off
def test_mode_off_after_on_is_todays_chain(r, c3):
    """After the mode was on and is switched off, both stages equal the existing models bit for bit,
    rt_variance_frame has nothing to return, and the mode's buffers are gone from device memory."""
    import torch
    z = SimpleNamespace(W=640, H=360, tile=32)
    r.set_pipeline(1)
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    r.resize(z.W, z.H, tile=z.tile)
    fp = cf.frame_params(z.W, z.H)
    r.reset()
    r.render(fp, cf.rand_origins(1))
    acc, hits = r.read_accum(), r.first_hit(fp)
    dn = r.denoise_async(fp, frame_ptr=r.temporal_async(fp, advance=True), reuse_guides=True)  # (their buffers exist)
    plain = device_floats(r, dn, z.W * z.H * 3)
    free0 = torch.cuda.mem_get_info()[0]
    r.set_variance(VP)
    dn = r.denoise_async(fp, frame_ptr=r.temporal_async(fp, advance=True), reuse_guides=True)
    assert r.variance_frame().shape == (z.H, z.W)
    mode_bytes = 44 * z.W * z.H
    assert torch.cuda.mem_get_info()[0] <= free0 - 0.9 * mode_bytes
    r.set_variance(False)
    assert r.get_variance().on is False
    assert torch.cuda.mem_get_info()[0] >= free0 - 0.1 * mode_bytes
    with pytest.raises(RuntimeError):
        r.variance_frame()
    out = r.temporal_async(fp, advance=True)
    got = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
    want, wn = tm.Temporal().call(acc, hits, fp, TemporalParams(), advance=True)
    same(got, r.temporal_history(), want, wn)
    dn = r.denoise_async(fp, frame_ptr=out, reuse_guides=True)
    assert np.array_equal(bits(device_floats(r, dn, z.W * z.H * 3)), bits(plain))


def test_rendering_is_undisturbed(r, c3):
    """Accumulation, LoopNum and stats stay identical around the mode's calls, and a frame rendered
    with the mode on is the frame rendered with it off."""
    z = prepare(r, c3, "70x37")
    fp = cf.frame_params(z.W, z.H)

    def frame():
        r.reset()
        r.clear_accum()
        r.render(fp, cf.rand_origins(1))
        return r.read_accum().tobytes()

    plain = frame()
    r.set_variance(VP)
    assert frame() == plain
    before = (r.loop_num, r.read_accum().tobytes(), r.stats())
    out = r.temporal_async(fp, advance=True)
    r.denoise_async(fp, frame_ptr=out, reuse_guides=True)
    r.variance_frame()
    r.temporal(fp, reuse_guides=True)
    r.denoise(fp)
    r.variance_frame()
    r.set_variance(False)
    assert (r.loop_num, r.read_accum().tobytes(), r.stats()) == before


def test_errors_and_the_setting_survives(r, c3):
    z = prepare(r, c3, "33x17")
    fp = cf.frame_params(z.W, z.H)
    L, h = r._L, r._h
    d = RtVarianceParams()
    assert L.rt_variance_default_params(C.byref(d)) == RT_OK and (d.on, d.sigma_lum, d.max_estimates, d.flags) == (0, 1.5, 64, 0)
    assert L.rt_variance_default_params(None) == RT_ERR_ARG
    for bad in (RtVarianceParams(2, 1.5, 64, 0), RtVarianceParams(1, 0.0, 64, 0), RtVarianceParams(1, float("nan"), 64, 0),
                RtVarianceParams(1, 1.5, 0, 0), RtVarianceParams(1, 1.5, 64, 1)):
        assert L.rt_variance_set(h, C.byref(bad)) == RT_ERR_ARG
    assert L.rt_variance_set(h, None) == RT_ERR_ARG and L.rt_variance_set(None, C.byref(d)) == RT_ERR_ARG
    assert L.rt_variance_get(h, None) == RT_ERR_ARG
    assert r.get_variance() == VarianceParams()
    buf = np.zeros((z.H, z.W), F)
    assert L.rt_variance_frame(h, buf.ctypes.data_as(C.POINTER(C.c_float))) == RT_ERR_STATE
    want = VarianceParams(on=True, sigma_lum=2.0, max_estimates=8)
    r.set_variance(want)
    assert L.rt_variance_frame(h, buf.ctypes.data_as(C.POINTER(C.c_float))) == RT_ERR_STATE  # no call yet
    assert L.rt_variance_frame(h, None) == RT_ERR_ARG
    r.temporal(fp, advance=True)
    assert L.rt_variance_frame(h, buf.ctypes.data_as(C.POINTER(C.c_float))) == RT_OK
    r.resize(z.W, z.H, tile=z.tile)
    assert r.get_variance() == want
    assert L.rt_variance_frame(h, buf.ctypes.data_as(C.POINTER(C.c_float))) == RT_ERR_STATE  # dropped with the size
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    assert r.get_variance() == want
    r.temporal(fp, advance=True)
    r.temporal(fp, TemporalParams(samples=2), reuse_guides=True)
    assert (r.variance_frame() >= 0).any()


# ------------------------------------------------------------------ interactive loop
def test_session_shows_the_models_chain(r, c3):
    """Three still ticks with enable_temporal, enable_denoise and enable_variance: each image is the
    oracle's display of the model's chain on that tick's accumulation."""
    W, H = 64, 36
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    s = ia.Session(r, W, H, settings=ia.Settings(max_bounce=4, enable_temporal=True, enable_denoise=True, enable_variance=True))
    r.clear_accum()
    assert r.get_variance().on is False   # (set by the first tick)
    model = vm.VarianceTemporal(VP)
    for k in range(3):
        out = s.tick(ia.Input(), delta_time=0.05)
        fp, hits = out["params"], r.first_hit(out["params"])
        want, _, wv = model.call(r.read_accum(), hits, fp, TemporalParams(samples=out["loop_num"]), advance=out["loop_num"] == 1)
        want, _ = vm.denoise(want, hits, DenoiseParams(), VP, wv)
        assert np.array_equal(out["image"], orc.display(want, out["display_flags"])), k
    assert r.get_variance() == VP and (model.cand.st[..., 3] == 2).any()
