"""GPU: environment maps of other shapes and contents than the one asset (tests/env_cases.py).

The device paths a map goes through (tex_index / tex_nearest, toSphericalCoord, hdrColorPdf,
SampleHdrLight, rt_light_table_kernel and the light-table cache behind rt_set_env) against the
oracle, bit for bit: maps of one and two texels, taller than wide, of odd sizes, with texels of
zero luminance and with a sun most of the cache points at, a 2048 x 1024 map whose light table takes
a second turn of the kernel's grid-stride loop, envAngle values that push u out of [0, 1] on both
sides, hdrResolution != w, and a map replaced between calls under one angle.

Images compare by bits, so a pixel the oracle makes NaN must be the same NaN on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

import env_cases as ec
from helpers import bit_mismatch, gpu_render
from rtamd import configs as cf
from rtamd.renderer import RT_ERR_ARG, RT_FLAG_MEGAKERNEL

pytestmark = pytest.mark.gpu

W, H, N = 48, 27, 2
ANGLE = 0.6
MODES = {"wavefront-bsdf": (True, 0), "wavefront-brdf": (False, 0), "megakernel": (True, RT_FLAG_MEGAKERNEL)}


def _differs(img, ref):
    """(pixels whose float32 bits differ in any channel, NaN pixels of the reference)."""
    _, diff = bit_mismatch(img, ref)
    return int(diff.sum()), int(np.any(np.isnan(ref), axis=-1).sum())


def _scene(kind):
    return ec.empty_scene() if kind == "empty" else cf.config_scene(kind)


def _check_case(r, name, scene, mode, mis=True, angle=ANGLE, res=None):
    bsdf, flags = MODES[mode]
    ref, cnt = ec.oracle_case(name, scene, bsdf, mis, angle, res)
    img_env = ec.env_pair(name)
    fp = cf.frame_params(W, H, env_angle=angle, enable_bsdf=bsdf, enable_mis=mis, flags=flags)
    sd = _scene(scene)
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(img_env[0], img_env[1], res)
    r.resize(W, H)
    r.set_loop_num(0)
    r.reset_stats()
    st = r.render(fp, cf.rand_origins(N))
    bad, nans = _differs(r.read_accum(), ref)
    print(f"{name} {scene} {mode} mis={mis} angle={angle} res={res}: {bad} pixels differ, {nans} NaN pixels, "
          f"rays gpu {st['rays']} oracle {cnt['rays']}")
    assert st["rays"] == cnt["rays"], (st["rays"], cnt["rays"])
    assert bad == 0, f"{bad} of {W * H} pixels differ from the oracle"
    return nans


@pytest.fixture(scope="module", autouse=True)
def _default_env_afterwards(gpu_renderer, env_maps):
    """The session's renderer leaves this module with the default map and one frame in flight."""
    yield
    gpu_renderer.set_pipeline(1)
    gpu_renderer.set_env(*env_maps)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ec.NAMES)
def test_map_family_matches_oracle(gpu_renderer, name, mode):
    """Every map of the family on C2 and on the empty scene, 48 x 27, 2 frames, envAngle 0.6, in
    the three modes: the wavefront path samples the light through the per-texel light table (BSDF
    and BRDF integrators), the megakernel through the cache itself.  Image and ray count equal the
    oracle's.  The oracle has NaN pixels, hundreds of the 1296, wherever a light sample's pdf is 0:
    on `one` (hdrResolution^2 / 2 == 0) and `black` throughout, on `black_texels` and `black_cols`
    where a sample lands on, or next to, a black texel (SampleHdr returns a texel's corner, so the
    fp32 lookup of that direction may name the neighbour); the GPU has them in the same places."""
    nans = _check_case(gpu_renderer, name, "C2", mode)
    if name in ("one", "black"):
        assert nans > 500, nans
    _check_case(gpu_renderer, name, "empty", mode)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["odd_sun", "black_texels"])
def test_map_family_without_mis(gpu_renderer, name, mode):
    _check_case(gpu_renderer, name, "C2", mode, mis=False)


@pytest.mark.parametrize("angle", [-1.25, -0.4, 0.0, 0.6, 3.0])
def test_env_angles_that_leave_the_unit_interval(gpu_renderer, angle):
    """u = ux + envAngle is not wrapped (RT:630): -1.25 and 3.0 clamp every lookup to the first /
    last column, the light table's included."""
    for mode in MODES:
        _check_case(gpu_renderer, "odd_sun", "C2", mode, angle=angle)


def test_hdr_resolution_other_than_the_width(gpu_renderer):
    """hdrResolution = 64 on the 100 x 37 map (p_convert of RT:1173-1186 uses it, the fetches use
    the texture's own size)."""
    for mode in MODES:
        _check_case(gpu_renderer, "odd_sun", "C2", mode, res=64)
        _check_case(gpu_renderer, "odd_sun", "C2", mode)  # and back: the table built for 64 is not reused


@pytest.mark.parametrize("angle", ec.IDENTITY_ANGLES)
@pytest.mark.parametrize("w,h", ec.IDENTITY_SIZES)
def test_texel_identity_lookup_equals_the_oracles(gpu_renderer, w, h, angle):
    """The empty scene under the texel-identity map: the GPU fetches the texel the oracle fetches
    for every camera ray, and tests/test_env_cases.py holds the oracle's frame to a float64
    statement of the lookup."""
    Wf, Hf = ec.IDENTITY_FRAME
    ref = ec.identity_oracle_render(w, h, angle)
    sd = ec.empty_scene()
    for flags in (0, RT_FLAG_MEGAKERNEL):
        fp = ec.identity_frame_params(angle)
        fp.flags = flags
        img, _ = gpu_render(gpu_renderer, sd, ec.identity_pair(w, h), Wf, Hf, fp, cf.rand_origins(1))
        assert np.array_equal(img, ref), int(np.any(img != ref, axis=-1).sum())


def _oracle_chain(sd, calls, angle):
    """The oracle through a list of (map name, first frame, frames) calls, its accumulation handed
    on through accum=; returns the image after each call and the rays of all."""
    import oracle as orc
    fp = cf.frame_params(W, H, env_angle=angle)
    acc, rays, out = None, 0, []
    for name, k0, n in calls:
        img, cache = ec.env_pair(name)
        ro = cf.rand_origins(k0 + n)
        frames = [cf.oracle_frame_params(fp, k + 1, ro[k]) for k in range(k0, k0 + n)]
        acc, cnt = orc.render(orc.OracleScene(sd.tri_enc, sd.node_enc, img, cache), frames, W, H, accum=acc)
        rays += cnt["rays"]
        out.append(acc)
    return out, rays


def test_replacing_the_map_under_one_angle(gpu_renderer):
    """rt_set_env between calls that all use envAngle 0.6: the light tables are keyed on the angle
    alone, so only rt_set_env's invalidation keeps a call from sampling the previous map's table.
    odd_sun -> odd (another size) -> odd_b (the same size, other content), each call a fresh
    image; every one equals the oracle with the map then bound."""
    r = gpu_renderer
    sd = cf.config_scene("C2")
    r.set_scene_soa(sd.soa, sd.nodes)
    r.resize(W, H)
    fp = cf.frame_params(W, H, env_angle=ANGLE)
    for name in ("odd_sun", "odd", "odd_b", "odd"):
        r.set_env(*ec.env_pair(name))
        r.clear_accum()
        r.set_loop_num(0)
        r.reset_stats()
        st = r.render(fp, cf.rand_origins(N))
        ref, cnt = ec.oracle_case(name, "C2", True, True, ANGLE)
        bad, _ = _differs(r.read_accum(), ref)
        assert bad == 0 and st["rays"] == cnt["rays"], (name, bad, st["rays"], cnt["rays"])


def test_replacing_the_map_between_pipelined_calls(gpu_renderer):
    """The same with frames in flight (rt_set_pipeline(2)): three one-frame calls under map A,
    rt_set_env(B) (which drains them), three more; the accumulation runs on through the change and
    equals the oracle's, chained through its accum= argument, after each half."""
    r = gpu_renderer
    sd = cf.config_scene("C2")
    fp = cf.frame_params(W, H, env_angle=ANGLE)
    refs, rays = _oracle_chain(sd, [("odd", 0, 3), ("odd_b", 3, 3)], ANGLE)
    ro = cf.rand_origins(6)
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*ec.env_pair("odd"))
    r.resize(W, H)
    r.set_pipeline(2)
    try:
        r.reset_stats()
        for k in range(3):
            r.render_async(fp, ro[k:k + 1])
        r.set_env(*ec.env_pair("odd_b"))
        half = r.read_accum()
        for k in range(3, 6):
            r.render_async(fp, ro[k:k + 1])
        st = r.stats()
        img = r.read_accum()
    finally:
        r.set_pipeline(1)
    assert r.loop_num == 6
    assert _differs(half, refs[0])[0] == 0
    assert _differs(img, refs[1])[0] == 0
    assert st["rays"] == rays
    # the two maps do give different images (the check above can tell them apart)
    other, _ = _oracle_chain(sd, [("odd", 0, 6)], ANGLE)
    assert _differs(other[0], refs[1])[0] > 0


def test_set_env_errors(gpu_renderer, env_maps):
    """rt_set_env refuses null pointers and non-positive sizes with RT_ERR_ARG and keeps the map it
    had; Renderer.set_env refuses a cache of another shape than the map (the library would read
    w * h * 3 floats from both)."""
    r = gpu_renderer
    sd = cf.config_scene("C2")
    img, cache = ec.env_pair("odd_sun")
    ref, cnt = ec.oracle_case("odd_sun", "C2", True, True, ANGLE)
    fp = cf.frame_params(W, H, env_angle=ANGLE)
    gpu_render(r, sd, (img, cache), W, H, fp, cf.rand_origins(N))
    L, h = r._L, r._h
    fpt = C.POINTER(C.c_float)
    a, b = img.ctypes.data_as(fpt), cache.ctypes.data_as(fpt)
    hh, ww, _ = img.shape
    for args in ((None, b, ww, hh, ww), (a, None, ww, hh, ww), (a, b, 0, hh, ww), (a, b, ww, 0, ww),
                 (a, b, -ww, hh, ww), (a, b, ww, -hh, ww), (None, None, 0, 0, 0)):
        assert L.rt_set_env(h, *args) == RT_ERR_ARG, args[2:]
    assert L.rt_set_env(None, a, b, ww, hh, ww) == RT_ERR_ARG
    for bad in (cache[:-1], cache[:, :-1], cache[..., :2], cache.reshape(-1, 3), ec.env_pair("odd")[1]):
        with pytest.raises(ValueError, match="set_env"):
            r.set_env(img, bad)
    with pytest.raises(ValueError, match="set_env"):
        r.set_env(img.reshape(-1, 3), cache.reshape(-1, 3))
    r.clear_accum()
    r.set_loop_num(0)
    r.reset_stats()
    st = r.render(fp, cf.rand_origins(N))
    assert _differs(r.read_accum(), ref)[0] == 0 and st["rays"] == cnt["rays"]
