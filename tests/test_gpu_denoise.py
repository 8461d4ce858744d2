"""The display denoiser (rt_abi.h rt_denoise*) on the GPU against the numpy model of
tests/denoise_model.py, bit for bit.

Every case runs C3.  The model's inputs are the GPU's own read_accum() and first_hit(fp), which
tests/test_gpu_parity.py and tests/test_gpu_query.py pin to the oracle.  Two frame sizes:

  70 x 37, tile 16   both axes end in partial tiles; at s = 16 only columns 32..37 have every
                     horizontal tap in the frame and no pixel has every vertical one; a residue
                     class has at most 5 x 3 pixels.  12 NaN / inf pixels are planted.
  64 x 36, tile 32   after 2 frames
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import denoise_model as dm
import oracle as orc
from rtamd import configs as cf
from rtamd import interactive as ia
from rtamd import scene_lib as sl
from rtamd.renderer import (HIT_DTYPE, RT_DENOISE_REUSE_GUIDES, RT_ERR_ARG, RT_ERR_STATE, RT_OK, DenoiseParams, Renderer,
                            RtDenoiseParams)

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = {"70x37": SimpleNamespace(W=70, H=37, tile=16, frames=1, plant=True),
         "64x36": SimpleNamespace(W=64, H=36, tile=32, frames=2, plant=False)}
PARAMS = {"it1": DenoiseParams(iterations=1), "it3": DenoiseParams(iterations=3), "it5": DenoiseParams(),
          "tight": DenoiseParams(5, 0.25, 0.1, 0.002)}


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


@pytest.fixture(scope="module")
def c3(env_maps):
    return SimpleNamespace(sd=cf.config_scene("C3"), env=env_maps, state={}, model={})


def prepare(r, c3, name):
    """The renderer at size `name` with C3, its accumulation after the size's frames (rendered once
    per module, then restored with write_accum) and LoopNum.  Returns (size, fp, accum, hits)."""
    z = SIZES[name]
    fp = cf.frame_params(z.W, z.H)
    r.set_pipeline(1)
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    r.resize(z.W, z.H, tile=z.tile)
    if name not in c3.state:
        r.reset()
        r.render(fp, cf.rand_origins(z.frames))
        acc, hits = r.read_accum(), r.first_hit(fp)
        if z.plant:
            acc, _ = dm.plant_nonfinite(acc, hits["triangle"] >= 0)
            assert (~np.isfinite(acc).all(-1)).sum() == 12
        acc.flags.writeable = hits.flags.writeable = False
        c3.state[name] = (acc, hits)
    acc, hits = c3.state[name]
    r.write_accum(acc)
    r.set_loop_num(z.frames)
    return z, fp, acc, hits


def model(c3, name, pname):
    if (name, pname) not in c3.model:
        acc, hits = c3.state[name]
        c3.model[name, pname] = dm.denoise(acc, hits, PARAMS[pname])
    return c3.model[name, pname]


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("name", list(SIZES))
def test_denoise_equals_the_model(gpu_renderer, c3, name, pname):
    r = gpu_renderer
    z, fp, acc, hits = prepare(r, c3, name)
    got = r.denoise(fp, PARAMS[pname])
    want = model(c3, name, pname)
    bad = np.argwhere((bits(got) != bits(want)).any(-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first (y, x) {bad[:6].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    hit = hits["triangle"] >= 0
    assert 0.3 < hit.mean() < 1.0
    assert np.array_equal(bits(got)[~hit], bits(acc)[~hit])
    if z.plant:
        assert np.isfinite(got[hit]).all()


# ------------------------------------------------------------------ entry points
def test_entry_points_agree(gpu_renderer, c3):
    """rt_denoise_async on a caller's frame and a caller's first-hit buffer gives rt_denoise's
    bytes, and the display pass shows its output frame as the oracle shows the model's."""
    import torch
    r = gpu_renderer
    z, fp, acc, hits = prepare(r, c3, "64x36")
    want = r.denoise(fp, PARAMS["it5"])
    assert np.array_equal(bits(want), bits(model(c3, "64x36", "it5")))
    d_frame = torch.from_numpy(acc.copy()).cuda()
    tiles = r.accum_device()["local_tiles"]
    d_hits = torch.zeros(tiles * z.tile * z.tile * HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream filled the buffers the ctx stream uses
    r.first_hit_device(fp, d_hits.data_ptr())
    r.write_accum(np.zeros_like(acc))  # (the accumulation is not what this call reads)
    out = r.denoise_async(fp, PARAMS["it5"], frame_ptr=d_frame.data_ptr(), hits_ptr=d_hits.data_ptr())
    got = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
    assert np.array_equal(bits(got), bits(want))
    for flags in (0, 3):
        assert np.array_equal(r.tonemap(flags, frame_ptr=out), orc.display(want, flags)), flags


# ------------------------------------------------------------------ guide reuse
def test_reuse_guides(gpu_renderer, c3):
    """RT_DENOISE_REUSE_GUIDES filters with the previous call's guides, whatever fp says; a call
    without it traces them again (after rt_update_materials: with the new material ids)."""
    r = gpu_renderer
    z, fp_a, _, hits_a = prepare(r, c3, "64x36")
    fp_b = cf.frame_params(z.W, z.H, position=(0.6, 0.3, 6.0))
    dp = PARAMS["it3"]
    r.denoise(fp_a, dp)
    r.reset()
    r.render(fp_b, cf.rand_origins(1, 2))
    acc_b, hits_b = r.read_accum(), r.first_hit(fp_b)
    assert hits_b.tobytes() != hits_a.tobytes()
    got = r.denoise(fp_b, DenoiseParams(dp.iterations, flags=RT_DENOISE_REUSE_GUIDES))
    assert np.array_equal(bits(got), bits(dm.denoise(acc_b, hits_a, dp)))
    assert not np.array_equal(bits(got), bits(dm.denoise(acc_b, hits_b, dp)))
    hit = np.argwhere(hits_b["triangle"] >= 0)
    py, px = (int(v) for v in hit[len(hit) // 2])
    try:
        r.update_materials(int(hits_b[py, px]["triangle"]), 1, cf.MATERIALS["golden"].texels())
        hits_c = r.first_hit(fp_b)
        assert hits_c[py, px]["material"] != hits_b[py, px]["material"]
        got = r.denoise(fp_b, dp)
        assert np.array_equal(bits(got), bits(dm.denoise(acc_b, hits_c, dp)))
        assert not np.array_equal(bits(got), bits(dm.denoise(acc_b, hits_b, dp)))
    finally:
        r.set_scene_soa(c3.sd.soa, c3.sd.nodes)


# ------------------------------------------------------------------ state and ordering
def test_state_is_untouched(gpu_renderer, c3):
    r = gpu_renderer
    z, fp, acc, _ = prepare(r, c3, "70x37")
    before = (r.loop_num, r.read_accum().tobytes(), r.stats())
    r.denoise(fp)
    r.denoise_async(fp, reuse_guides=True)
    assert (r.loop_num, r.read_accum().tobytes(), r.stats()) == before


@pytest.mark.parametrize("depth", [1, 2])
def test_a_render_queued_after_the_denoise_blends_after_it(gpu_renderer, c3, depth):
    """render, denoise, render without a synchronise between them: the denoiser saw the first
    frame's accumulation and the accumulation ends as in the serial order."""
    r = gpu_renderer
    z, fp, _, _ = prepare(r, c3, "64x36")
    ro = cf.rand_origins(3)

    def start():
        r.reset()
        r.clear_accum()
        r.render(fp, ro[:1])  # (a finished call: the next two are what is queued back to back)

    start()
    r.render(fp, ro[1:2])
    want_dn = r.denoise(fp)
    r.render(fp, ro[2:3])
    want_acc = r.read_accum()
    try:
        r.set_pipeline(depth)
        start()
        r.render_async(fp, ro[1:2])
        out = r.denoise_async(fp)
        r.render_async(fp, ro[2:3])
        got_dn = device_floats(r, out, z.W * z.H * 3).reshape(z.H, z.W, 3)
        assert np.array_equal(bits(got_dn), bits(want_dn))
        assert np.array_equal(bits(r.read_accum()), bits(want_acc)) and r.loop_num == 3
    finally:
        r.set_pipeline(1)


# ------------------------------------------------------------------ errors
def _raw(r, fp, dp, buf):
    p = fp.to_c()
    return r._L.rt_denoise(r._h, C.byref(p), C.byref(dp), buf.ctypes.data_as(C.POINTER(C.c_float)))


def test_errors(gpu_renderer, c3):
    r = gpu_renderer
    z, fp, _, _ = prepare(r, c3, "64x36")
    buf = np.zeros((z.H, z.W, 3), F)
    ok = DenoiseParams().to_c()
    fresh = Renderer(0)
    try:
        assert _raw(fresh, fp, ok, buf) == RT_ERR_STATE
        s = sl.Scene()
        s.build_bvh(8)
        fresh.set_scene_soa(s.export_soa(), s.nodes())
        assert _raw(fresh, fp, ok, buf) == RT_ERR_STATE  # no rt_resize yet
        fresh.resize(z.W, z.H)
        assert _raw(fresh, fp, DenoiseParams().to_c(RT_DENOISE_REUSE_GUIDES), buf) == RT_ERR_STATE  # before any denoise
    finally:
        fresh.close()
    for bad in (RtDenoiseParams(0, 1.0, 0.3, 0.01, 0), RtDenoiseParams(6, 1.0, 0.3, 0.01, 0),
                RtDenoiseParams(5, float("nan"), 0.3, 0.01, 0), RtDenoiseParams(5, 1.0, 0.0, 0.01, 0),
                RtDenoiseParams(5, 1.0, 0.3, float("inf"), 0), RtDenoiseParams(5, 1.0, 0.3, -0.01, 0),
                RtDenoiseParams(5, 1.0, 0.3, 0.01, 2), RtDenoiseParams(5, 1.0, 0.3, 0.01, 5)):
        assert _raw(r, fp, bad, buf) == RT_ERR_ARG, (bad.iterations, bad.sigma_color, bad.sigma_normal, bad.sigma_plane, bad.flags)
    p = fp.to_c()
    assert r._L.rt_denoise(r._h, C.byref(p), None, buf.ctypes.data_as(C.POINTER(C.c_float))) == RT_ERR_ARG
    assert r._L.rt_denoise(r._h, C.byref(p), C.byref(ok), None) == RT_ERR_ARG
    assert r._L.rt_denoise(r._h, None, C.byref(ok), buf.ctypes.data_as(C.POINTER(C.c_float))) == RT_ERR_ARG
    assert r._L.rt_denoise_async(r._h, C.byref(p), C.byref(ok), None, None, None) == RT_ERR_ARG
    d = RtDenoiseParams()
    assert r._L.rt_denoise_default_params(C.byref(d)) == RT_OK and r._L.rt_denoise_default_params(None) == RT_ERR_ARG
    assert (d.iterations, d.sigma_color, d.sigma_normal, d.sigma_plane, d.flags) == (5, 1.0, F(0.3), F(0.01), 0)
    assert _raw(r, fp, ok, buf) == RT_OK
    reuse = DenoiseParams().to_c(RT_DENOISE_REUSE_GUIDES)
    assert _raw(r, fp, reuse, buf) == RT_OK
    try:
        r.resize(z.W, z.H, tile=z.tile)
        assert _raw(r, fp, reuse, buf) == RT_ERR_STATE  # the guides were another frame's
        r.resize(z.W, z.H, tile=16, rank=0, world=2)
        assert _raw(r, fp, ok, buf) == RT_ERR_STATE
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            r.denoise(fp)
    finally:
        r.resize(z.W, z.H)


# ------------------------------------------------------------------ interactive loop
def test_session_shows_the_denoised_frame(gpu_renderer, c3):
    """Three ticks (still, still, move) with enable_denoise: each image is the oracle's display of the
    model on that tick's accumulation and first-hit frame; the same images with two frames in
    flight; with the setting off, the display of the accumulation itself."""
    r = gpu_renderer
    W, H = 64, 36
    r.set_scene_soa(c3.sd.soa, c3.sd.nodes)
    r.set_env(*c3.env)
    inputs = (ia.Input(), ia.Input(), ia.Input(keys=["w"]))

    def run(denoise, in_flight, check):
        s = ia.Session(r, W, H, settings=ia.Settings(max_bounce=4, enable_denoise=denoise), frames_in_flight=in_flight)
        r.clear_accum()
        outs = []
        for inp in inputs:
            out = s.tick(inp, delta_time=0.05)
            if in_flight == 1:
                check(out)
            outs.append(out)
        outs = [o for o in outs if o is not None] + s.flush()
        return [o["image"] for o in outs]

    def check_denoised(out):
        want = dm.denoise(r.read_accum(), r.first_hit(out["params"]), DenoiseParams())
        assert np.array_equal(out["image"], orc.display(want, out["display_flags"]))

    def check_plain(out):
        assert np.array_equal(out["image"], orc.display(r.read_accum(), out["display_flags"]))

    try:
        shown = run(True, 1, check_denoised)
        queued = run(True, 2, None)
        assert len(shown) == len(queued) == 3 and all(np.array_equal(a, b) for a, b in zip(shown, queued))
        plain = run(False, 1, check_plain)
        assert not np.array_equal(plain[0], shown[0])
    finally:
        r.set_pipeline(1)
