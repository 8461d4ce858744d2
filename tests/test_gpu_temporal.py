"""The temporal stage of the displayed frame (rt_abi.h rt_temporal*) on the GPU against the numpy model
of tests/temporal_model.py, bit for bit.

The synthetic cases of tests/temporal_cases.py run through rt_temporal_async with a caller's frame
and a caller's first-hit buffer and meet the same analytic bounds as the model alone
(tests/test_temporal_model.py).  Every other case runs C3 at the denoiser's two sizes (70 x 37 with
tile 16 and 12 planted non-finite pixels per view, 64 x 36 with tile 32); there the model's inputs
are the GPU's own read_accum() and first_hit(fp), which tests/test_gpu_parity.py and
tests/test_gpu_query.py pin to the oracle.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import denoise_model as dm
import oracle as orc
import temporal_cases as tc
import temporal_model as tm
from rtamd import configs as cf
from rtamd import interactive as ia
from rtamd import scene_lib as sl
from rtamd.renderer import (HIT_DTYPE, RT_ERR_ARG, RT_ERR_STATE, RT_OK, RT_TEMPORAL_ADVANCE, RT_TEMPORAL_REUSE_GUIDES,
                            DenoiseParams, FrameParams, Renderer, RtTemporalParams, TemporalParams)

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {k: SimpleNamespace(W=w, H=h, tile=t, plant=k == "70x37") for k, (w, h, t) in tc.SIZES.items()}
# the views of the C3 chain: a strafe, a forward step, a mouse yaw (Camera.h:83-131)
MOVES = (lambda c: c.process_keyboard(ia.RIGHT, 0.08), lambda c: c.process_keyboard(ia.FORWARD, 0.1),
         lambda c: c.process_mouse_movement(20.0, 0.0))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def device_floats(r, ptr: int, n: int) -> np.ndarray:
    """n floats at device pointer ptr, after the work queued on r's stream (hipMemcpy of the HIP
    runtime the process has loaded)."""
    r.synchronize()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(n, F)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def fp_of(cam: ia.Camera) -> FrameParams:
    return FrameParams(position=cam.position, front=cam.front, right=cam.right, up=cam.up,
                       left_bottom_corner=cam.left_bottom_corner, half_h=float(cam.half_h), half_w=float(cam.half_w))


def tiled(hits, tile):
    """(H, W) records -> RT_LAYOUT_LOCAL_TILES order of a whole-frame context (rt_first_hit_device's)"""
    H, W = hits.shape
    tiles_x, tiles_y = -(-W // tile), -(-H // tile)
    out = np.zeros(tiles_x * tiles_y * tile * tile, hits.dtype)
    py, px = np.mgrid[0:H, 0:W]
    ty, tx = py // tile, px // tile
    out[(ty * tiles_x + tx) * tile * tile + (py - ty * tile) * tile + (px - tx * tile)] = hits
    return out


@pytest.fixture(scope="module")
def c3(env_maps):
    return SimpleNamespace(sd=cf.config_scene("C3"), env=env_maps)


def prepare(r, c3, name):
    z = SIZES[name]
    r.set_pipeline(1)
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)  # (drops any display history)
    r.set_env(*c3.env)
    r.resize(z.W, z.H, tile=z.tile)
    return z


def same(got, n, want, wn):
    bad = np.argwhere((bits(got) != bits(want)).any(-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first (y, x) {bad[:6].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    bad = np.argwhere(bits(n) != bits(wn))
    assert bad.size == 0, f"{len(bad)} history lengths differ, first (y, x) {bad[:6].tolist()}"


# ------------------------------------------------------------------ the synthetic cases
def gpu_run(r, z):
    """run() of tests/temporal_cases.py: rt_temporal_async on a caller's frame and hits (torch device
    buffers), its output and rt_temporal_history checked against the model bit for bit."""
    import torch
    model = tm.Temporal()

    def run(color, hits, fp, tp, advance=False, reset=False):
        d_frame = torch.from_numpy(np.ascontiguousarray(color, F)).cuda()
        d_hits = torch.from_numpy(tiled(hits, z.tile).view(np.uint8)).cuda()
        torch.cuda.synchronize()  # torch's stream filled the buffers the ctx stream uses
        p = TemporalParams(tp.samples, tp.max_history, tp.sigma_normal, tp.sigma_plane)
        out = r.temporal_async(fp, p, frame_ptr=d_frame.data_ptr(), hits_ptr=d_hits.data_ptr(), advance=advance, reset=reset)
        got = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
        n = r.temporal_history()
        same(got, n, *model.call(color, hits, fp, tp, advance=advance, reset=reset))
        return got, n

    return run


CASES = {"linear-axis": lambda s, run: tc.case_linear_plane(s, run, "axis"),
         "linear-turned": lambda s, run: tc.case_linear_plane(s, run, "turned"),
         "revealed-material": lambda s, run: tc.case_disocclusion(s, run, "material"),
         "revealed-plane": lambda s, run: tc.case_disocclusion(s, run, "plane"),
         "tilted": tc.case_tilted_neighbour, "bookkeeping": tc.case_bookkeeping, "passthrough": tc.case_passthrough}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", list(SIZES))
def test_synthetic_cases(gpu_renderer, c3, name, case):
    r = gpu_renderer
    z = prepare(r, c3, name)
    CASES[case](name, gpu_run(r, z))


# ------------------------------------------------------------------ C3 parity
def c3_views(r, z, views=4):
    """Render one frame per view of the chain (the default camera, then MOVES one after the other);
    yields (k, fp, accumulation, first-hit frame) with the accumulation as the GPU holds it."""
    cam = ia.Camera(float(F(z.W) / F(z.H)))
    for k in range(views):
        if k:
            MOVES[k - 1](cam)
        fp = fp_of(cam)
        r.reset()
        r.clear_accum()  # (a planted NaN would survive the first frame's blend weight 0)
        r.render(fp, cf.rand_origins(1, k))
        acc, hits = r.read_accum(), r.first_hit(fp)
        if z.plant:
            acc, _ = dm.plant_nonfinite(acc, hits["triangle"] >= 0, seed=7 + k)
            assert (~np.isfinite(acc).all(-1)).sum() == 12
            r.write_accum(acc)
        yield k, fp, acc, hits


@pytest.mark.parametrize("name", list(SIZES))
def test_c3_chain_equals_the_model(gpu_renderer, c3, name):
    """Four views of C3 (still, strafe, forward step, mouse yaw), each rendered once and shown through
    rt_temporal with ADVANCE, then a second frame of the last view without it (REUSE_GUIDES): outputs
    and history lengths equal the model's, and each move exercises every class of pixel."""
    r = gpu_renderer
    z = prepare(r, c3, name)
    model = tm.Temporal()
    for k, fp, acc, hits in c3_views(r, z):
        got = r.temporal(fp, TemporalParams(samples=1), advance=True)
        want, wn = model.call(acc, hits, fp, TemporalParams(samples=1), advance=True)
        same(got, r.temporal_history(), want, wn)
        hit = hits["triangle"] >= 0
        assert np.array_equal(bits(got)[~hit], bits(acc)[~hit])
        if k == 0:
            assert not model.has.any()
            continue
        floors = ((model.taps == 4).mean(), (hit & ~model.has).sum(), ((model.taps > 0) & (model.taps < 4)).sum(), (~hit).sum())
        assert floors[0] >= 0.25 and min(floors[1:]) >= 20, (k, floors)
    r.render(fp, cf.rand_origins(1, 9))
    acc = r.read_accum()
    assert r.loop_num == 2
    got = r.temporal(fp, TemporalParams(samples=2), reuse_guides=True)
    want, wn = model.call(acc, hits, fp, TemporalParams(samples=2))
    same(got, r.temporal_history(), want, wn)
    assert model.has.sum() > 0.25 * z.W * z.H


# ------------------------------------------------------------------ entry points
def test_entry_points_agree(gpu_renderer, c3):
    """rt_temporal on the accumulation gives rt_temporal_async's bytes on a caller's frame and a
    caller's first-hit buffer; its output pointer feeds rt_denoise_async with REUSE_GUIDES, whose
    result is the denoiser model's of the temporal model's output; the display pass shows it as the
    oracle shows the model's."""
    import torch
    r = gpu_renderer
    z = prepare(r, c3, "64x36")
    model = tm.Temporal()
    for k, fp, acc, hits in c3_views(r, z, views=2):
        want = r.temporal(fp, advance=True)
        wm, wn = model.call(acc, hits, fp, TemporalParams(), advance=True)
        same(want, r.temporal_history(), wm, wn)
    assert model.has.mean() > 0.25
    d_frame = torch.from_numpy(acc.copy()).cuda()
    tiles = r.accum_device()["local_tiles"]
    d_hits = torch.zeros(tiles * z.tile * z.tile * HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream filled the buffers the ctx stream uses
    r.first_hit_device(fp, d_hits.data_ptr())
    r.write_accum(np.zeros_like(acc))  # (the accumulation is not what this call reads)
    # without ADVANCE the history stays the first view's: the same call again
    out = r.temporal_async(fp, frame_ptr=d_frame.data_ptr(), hits_ptr=d_hits.data_ptr())
    got = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
    assert np.array_equal(bits(got), bits(want))
    for flags in (0, 3):
        assert np.array_equal(r.tonemap(flags, frame_ptr=out), orc.display(want, flags)), flags
    dn = r.denoise_async(fp, DenoiseParams(), frame_ptr=out, reuse_guides=True)
    got = device_floats(r, dn, z.W * z.H * 3).reshape(z.H, z.W, 3)
    assert np.array_equal(bits(got), bits(dm.denoise(want, hits, DenoiseParams())))
    # and in the other direction: a temporal call on the denoiser's freshly traced guides
    r.write_accum(acc)
    r.denoise(fp)
    got = r.temporal(fp, reuse_guides=True)
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------ state and ordering
def test_state_is_untouched(gpu_renderer, c3):
    r = gpu_renderer
    z = prepare(r, c3, "70x37")
    fp = cf.frame_params(z.W, z.H)
    r.reset()
    r.render(fp, cf.rand_origins(1))
    before = (r.loop_num, r.read_accum().tobytes(), r.stats())
    r.temporal(fp, advance=True)
    r.temporal_async(fp, reuse_guides=True)
    r.temporal_history()
    assert (r.loop_num, r.read_accum().tobytes(), r.stats()) == before


@pytest.mark.parametrize("depth", [1, 2])
def test_a_render_queued_after_the_temporal_call_blends_after_it(gpu_renderer, c3, depth):
    """render, temporal, render without a synchronise between them: the stage saw the first frame's
    accumulation and the accumulation ends as in the serial order."""
    r = gpu_renderer
    z = prepare(r, c3, "64x36")
    fp = cf.frame_params(z.W, z.H)
    ro = cf.rand_origins(3)
    tp = TemporalParams(samples=2)

    def start():
        r.reset()
        r.clear_accum()
        r.render(fp, ro[:1])  # (a finished call: the next two are what is queued back to back)

    start()
    r.render(fp, ro[1:2])
    seen = r.read_accum()
    want_t = r.temporal(fp, tp, reset=True)
    assert np.array_equal(bits(want_t), bits(seen))  # (no history: the accumulation after two frames)
    r.render(fp, ro[2:3])
    want_acc = r.read_accum()
    assert not np.array_equal(bits(want_acc), bits(seen))
    try:
        r.set_pipeline(depth)
        start()
        r.render_async(fp, ro[1:2])
        out = r.temporal_async(fp, tp, reset=True)
        r.render_async(fp, ro[2:3])
        got_t = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
        assert np.array_equal(bits(got_t), bits(want_t))
        assert np.array_equal(bits(r.read_accum()), bits(want_acc)) and r.loop_num == 3
    finally:
        r.set_pipeline(1)


# ------------------------------------------------------------------ errors
def _raw(r, fp, tp, buf):
    p = fp.to_c()
    return r._L.rt_temporal(r._h, C.byref(p), C.byref(tp), buf.ctypes.data_as(C.POINTER(C.c_float)))


def test_errors(gpu_renderer, c3):
    r = gpu_renderer
    z = prepare(r, c3, "64x36")
    fp = cf.frame_params(z.W, z.H)
    buf = np.zeros((z.H, z.W, 3), F)
    nbuf = np.zeros((z.H, z.W), F)
    fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ok = TemporalParams().to_c()
    fresh = Renderer(0)
    try:
        assert _raw(fresh, fp, ok, buf) == RT_ERR_STATE
        s = sl.Scene()
        s.build_bvh(8)
        fresh.set_scene_soa(s.export_soa(), s.nodes())
        assert _raw(fresh, fp, ok, buf) == RT_ERR_STATE  # no rt_resize yet
        fresh.resize(z.W, z.H)
        assert _raw(fresh, fp, TemporalParams().to_c(RT_TEMPORAL_REUSE_GUIDES), buf) == RT_ERR_STATE  # before any guides
        assert fresh._L.rt_temporal_history(fresh._h, fptr(nbuf)) == RT_ERR_STATE  # before any call
    finally:
        fresh.close()
    for bad in (RtTemporalParams(0, 32, 0.3, 0.01, 0), RtTemporalParams(-1, 32, 0.3, 0.01, 0), RtTemporalParams(1, 0, 0.3, 0.01, 0),
                RtTemporalParams(1, 32, float("nan"), 0.01, 0), RtTemporalParams(1, 32, 0.0, 0.01, 0),
                RtTemporalParams(1, 32, 0.3, float("inf"), 0), RtTemporalParams(1, 32, 0.3, -0.01, 0),
                RtTemporalParams(1, 32, 0.3, 0.01, 8), RtTemporalParams(1, 32, 0.3, 0.01, 17)):
        assert _raw(r, fp, bad, buf) == RT_ERR_ARG, (bad.samples, bad.max_history, bad.sigma_normal, bad.sigma_plane, bad.flags)
    p = fp.to_c()
    assert r._L.rt_temporal(r._h, C.byref(p), None, fptr(buf)) == RT_ERR_ARG
    assert r._L.rt_temporal(r._h, C.byref(p), C.byref(ok), None) == RT_ERR_ARG
    assert r._L.rt_temporal(r._h, None, C.byref(ok), fptr(buf)) == RT_ERR_ARG
    assert r._L.rt_temporal_async(r._h, C.byref(p), C.byref(ok), None, None, None) == RT_ERR_ARG
    assert r._L.rt_temporal_history(r._h, None) == RT_ERR_ARG
    assert r._L.rt_temporal_history(r._h, fptr(nbuf)) == RT_ERR_STATE  # the scene was set since: no output
    r.reset()
    r.render(fp, cf.rand_origins(1))
    acc, hit = r.read_accum(), r.first_hit(fp)["triangle"] >= 0
    adv = TemporalParams().to_c(RT_TEMPORAL_ADVANCE)
    assert _raw(r, fp, adv, buf) == RT_OK and _raw(r, fp, adv, buf) == RT_OK
    assert r._L.rt_temporal_history(r._h, fptr(nbuf)) == RT_OK and (nbuf[hit] > 1).mean() > 0.9
    reuse = TemporalParams().to_c(RT_TEMPORAL_ADVANCE | RT_TEMPORAL_REUSE_GUIDES)
    assert _raw(r, fp, reuse, buf) == RT_OK
    try:
        # rt_resize drops the history (and the guides): the next call has none anywhere
        r.resize(z.W, z.H, tile=z.tile)
        assert _raw(r, fp, reuse, buf) == RT_ERR_STATE
        assert r._L.rt_temporal_history(r._h, fptr(nbuf)) == RT_ERR_STATE
        r.write_accum(acc)
        assert _raw(r, fp, adv, buf) == RT_OK and np.array_equal(bits(buf), bits(acc))
        assert np.array_equal(r.temporal_history(), np.where(hit, 1, 0))
        # so does rt_set_scene
        assert _raw(r, fp, adv, buf) == RT_OK and (r.temporal_history()[hit] > 1).mean() > 0.9
        r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
        assert _raw(r, fp, adv, buf) == RT_OK and np.array_equal(bits(buf), bits(acc))
        r.resize(z.W, z.H, tile=16, rank=0, world=2)
        assert _raw(r, fp, ok, buf) == RT_ERR_STATE
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            r.temporal(fp)
    finally:
        r.resize(z.W, z.H)


# ------------------------------------------------------------------ interactive loop
@pytest.mark.parametrize("denoise", [False, True])
def test_session_shows_the_temporal_frame(gpu_renderer, c3, denoise):
    """still, still, strafe, still, still with enable_temporal: each image is the oracle's display of
    the model's chain (temporal, then the denoiser model when that is on) on that tick's
    accumulation and first-hit frame; the same images with two frames in flight; with the setting
    off, the images of a Session without it."""
    r = gpu_renderer
    W, H = 64, 36
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    inputs = (ia.Input(), ia.Input(), ia.Input(keys=["d"]), ia.Input(), ia.Input())

    def run(settings, in_flight, check):
        s = ia.Session(r, W, H, settings=settings, frames_in_flight=in_flight)
        r.clear_accum()
        outs = []
        for inp in inputs:
            out = s.tick(inp, delta_time=0.05)
            if in_flight == 1:
                check(out)
            outs.append(out)
        outs = [o for o in outs if o is not None] + s.flush()
        return [o["image"] for o in outs]

    model = tm.Temporal()
    history = []

    def check_temporal(out):
        fp, hits = out["params"], r.first_hit(out["params"])
        want, _ = model.call(r.read_accum(), hits, fp, TemporalParams(samples=out["loop_num"]), advance=out["loop_num"] == 1)
        history.append(float(model.has.mean()))
        if denoise:
            want = dm.denoise(want, hits, DenoiseParams())
        assert np.array_equal(out["image"], orc.display(want, out["display_flags"]))

    def check_plain(out):
        want = r.read_accum()
        if denoise:
            want = dm.denoise(want, r.first_hit(out["params"]), DenoiseParams())
        assert np.array_equal(out["image"], orc.display(want, out["display_flags"]))

    on = ia.Settings(max_bounce=4, enable_temporal=True, enable_denoise=denoise)
    try:
        shown = run(on, 1, check_temporal)
        # (the first view has no history; the strafe and the ticks after it see the first view's last display)
        assert history[0] == history[1] == 0.0 and min(history[2:]) > 0.25
        queued = run(on, 2, None)
        assert len(shown) == len(queued) == 5 and all(np.array_equal(a, b) for a, b in zip(shown, queued))
        plain = run(ia.Settings(max_bounce=4, enable_denoise=denoise), 1, check_plain)
        off = run(ia.Settings(max_bounce=4, enable_temporal=False, enable_denoise=denoise), 1, check_plain)
        assert all(np.array_equal(a, b) for a, b in zip(plain, off))
        assert not np.array_equal(plain[3], shown[3])
    finally:
        r.set_pipeline(1)
