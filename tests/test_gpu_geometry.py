"""rt_update_geometry on the GPU: the device arrays and bounds equal the CPU model's
(scn::update_geometry, tests/test_geometry_model.py) byte for byte, and queries and renders of the
updated context equal the oracle's on the moved scene (geometry_cases.moved_scene) bit for bit.

Bit equality of the fp64 fields (the edge filter's rows, the margins) rests on the device's fp64
divide and square root being correctly rounded; a differing field is reported by array and word.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import geometry_cases as gc
import oracle as orc
import query_cases as qc
from helpers import bit_mismatch, frames_for
from rtamd import configs as cf
from rtamd import interactive as ia
from rtamd import scene_lib as sl
from rtamd.renderer import (RT_ERR_ARG, RT_ERR_STATE, RT_OK, SCENE_ARRAYS, DenoiseParams, Renderer)

pytestmark = pytest.mark.gpu
F = np.float32
W, H, FRAMES = gc.W, gc.H, gc.FRAMES


@pytest.fixture(scope="module")
def case(env_maps):
    """C2, the moved bunny, the moved scene's oracle and its render of two frames (read-only)."""
    sd = gc.c2()
    idx, p, n = gc.moved("MOVE")
    tri_enc, node_enc = gc.moved_c2("MOVE")
    fp = cf.frame_params(W, H)
    ro, frames = frames_for(fp, 1, FRAMES)
    sc = orc.OracleScene(tri_enc, node_enc, *env_maps)
    ref, _ = orc.render(sc, frames, W, H)
    ref0, _ = orc.render(orc.OracleScene(sd.tri_enc, sd.node_enc, *env_maps), frames, W, H)
    for a in (ref, ref0):
        a.flags.writeable = False
    return SimpleNamespace(sd=sd, idx=idx, p=p, n=n, tri_enc=tri_enc, node_enc=node_enc, fp=fp, ro=ro, frames=frames,
                           sc=sc, ref=ref, ref0=ref0, env=env_maps)


def downloads(r):
    return {k: r.scene_download(k) for k in SCENE_ARRAYS}


def assert_equals_model(r, m, what):
    s = m.snapshot()
    gc.assert_arrays_equal(downloads(r), s.arrays, what=what)
    b = r.scene_bounds()
    got = tuple(b[k] for k in gc.BOUNDS) + (b["tri_flagged"],)
    assert got == gc.bounds_of(s), f"{what}: bounds {got} vs the model's {gc.bounds_of(s)}"


def render(r, case, scene=None):
    if scene is not None:
        scene()
    r.set_env(*case.env)
    r.resize(W, H)
    r.set_loop_num(0)
    r.render(case.fp, case.ro)
    return r.read_accum()


# ------------------------------------------------------------------ arrays and bounds
def test_compile_arrays_reach_the_device(gpu_renderer, case):
    """scene_download / scene_bounds before any update: the compile's arrays."""
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    assert_equals_model(r, gc.model(), "after rt_set_scene")


def test_one_leaf_scene(gpu_renderer):
    sd = gc.one_leaf_scene()
    r = gpu_renderer
    r.set_scene_encoded(sd.tri_enc, sd.node_enc)
    m = sl.CompiledHandle(sd.tri_enc, sd.node_enc)
    p, n = sd.tri_enc[:, 0:3] * F(0.75) + F(0.125), sd.tri_enc[:, 3:6]
    assert m.update_geometry(None, p, n) == 0
    r.update_geometry(None, p, n)
    assert_equals_model(r, m, "one leaf")


@pytest.mark.parametrize("which", ["MOVE", "STRETCH"])
def test_scattered_index_list(gpu_renderer, case, which):
    """The bunny's post-BVH indices (scattered over the list): a well-shaped move, and the stretch
    that puts most triangles above the filter's caps."""
    r = gpu_renderer
    idx, p, n = gc.moved(which)
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    m = gc.model()
    assert m.update_geometry(idx, p, n) == 0
    r.update_geometry(idx, p, n)
    assert_equals_model(r, m, which)
    p0, n0 = gc.original(idx)                              # and a second update on top of it: back again
    assert m.update_geometry(idx, p0, n0) == 0
    r.update_geometry(idx, p0, n0)
    assert_equals_model(r, m, which + " and back")


def test_full_update_without_an_index_list(gpu_renderer, case):
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    m = gc.model()
    p, n = case.tri_enc[:, 0:3], case.tri_enc[:, 3:6]
    assert m.update_geometry(None, p, n) == 0
    r.update_geometry(None, p, n)
    assert_equals_model(r, m, "tri_index = NULL")
    first = 1234                                           # a range that starts past 0
    q = p[first:first + 777] + F(0.01)
    assert m.update_geometry(None, q, n[first:first + 777], first=first) == 0
    r.update_geometry(None, q, n[first:first + 777], first=first)
    assert_equals_model(r, m, "first = 1234")


def test_device_pointer_form(gpu_renderer, case):
    """Vertices a torch operation produced on the GPU (the same values as the host case)."""
    import torch
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    m = gc.model()
    assert m.update_geometry(case.idx, case.p, case.n) == 0
    dev = torch.device("cuda", 0)
    r.update_geometry(torch.as_tensor(case.idx, device=dev), torch.as_tensor(case.p, device=dev) * 1.0,
                      torch.as_tensor(case.n, device=dev))
    assert_equals_model(r, m, "device form")
    r.update_geometry(None, torch.as_tensor(case.tri_enc[:, 0:3].copy(), device=dev),
                      torch.as_tensor(case.tri_enc[:, 3:6].copy(), device=dev))
    assert_equals_model(r, m, "device form, tri_index = NULL")


# ------------------------------------------------------------------ hits
def test_hits_equal_the_oracle_on_the_moved_scene(gpu_renderer, case):
    r = gpu_renderer
    moved = SimpleNamespace(tri_enc=case.tri_enc)
    o, d = qc.c2_rays(moved, case.sc, cf.MATERIALS["jade"].texels())   # around and inside the moved bunny's box
    rng = np.random.default_rng(7)
    inside = case.p.reshape(-1, 3).mean(axis=0).astype(F) + rng.normal(size=(256, 3)).astype(F) * F(0.05)
    o = np.concatenate([o, inside])                                     # and rays that start inside the mesh
    d = np.concatenate([d, qc._unit(rng, 256)])
    ref = qc.oracle_hits(case.sc, o, d)
    assert (ref["triangle"] >= 0).mean() > 0.3 and (ref["inside"][-256:] != 0).sum() > 64
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    r.update_geometry(case.idx, case.p, case.n)
    got = r.trace_rays(o, d)
    qc.assert_hits_equal(got, ref, "closest")
    qc.assert_hits_equal(r.trace_rays(o, d, no_cull=True), ref, "closest, RT_QUERY_NO_CULL")
    assert got.tobytes() == r.trace_rays(o, d, no_cull=True).tobytes()
    assert np.array_equal(r.trace_rays(o, d, kind="any"), (ref["triangle"] >= 0).astype(np.int32))
    r.resize(W, H)
    fresh = Renderer(0)
    try:
        fresh.set_scene_encoded(case.tri_enc, case.node_enc)
        fresh.resize(W, H)
        fh = r.first_hit(case.fp)
        assert fh.tobytes() == fresh.first_hit(case.fp).tobytes()
        rays = r.camera_rays(case.fp).reshape(-1)
        qc.assert_hits_equal(fh.reshape(-1), qc.oracle_hits(case.sc, rays["origin"], rays["dir"]), "rt_first_hit")
    finally:
        fresh.close()


# ------------------------------------------------------------------ renders
def test_render_equals_the_oracle_and_a_fresh_context(gpu_renderer, case):
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    r.update_geometry(case.idx, case.p, case.n)
    img = render(r, case)
    assert bit_mismatch(img, case.ref)[0] == 0.0
    fresh = Renderer(0)
    try:
        assert render(fresh, case, lambda: fresh.set_scene_encoded(case.tri_enc, case.node_enc)).tobytes() == img.tobytes()
    finally:
        fresh.close()


@pytest.mark.parametrize("width,rebuild", [("2", "1"), ("4", "0")])
def test_render_on_the_other_trees(gpu_dev_renderer, case, monkeypatch, width, rebuild):
    """RT_BVH_WIDTH=2: the wavefront trace on the (refitted) binary tree; RT_REBUILD=0: the 4-wide
    tree collapsed from the reference's own internal nodes."""
    monkeypatch.setenv("RT_BVH_WIDTH", width)
    monkeypatch.setenv("RT_REBUILD", rebuild)
    r = gpu_dev_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    r.update_geometry(case.idx, case.p, case.n)
    assert bit_mismatch(render(r, case), case.ref)[0] == 0.0
    m = gc.model(rebuild=rebuild == "1")
    assert m.update_geometry(case.idx, case.p, case.n) == 0
    gc.assert_arrays_equal(downloads(r), m.snapshot().arrays, what=f"width {width} rebuild {rebuild}")


def test_there_and_back(gpu_renderer, case):
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    r.update_geometry(case.idx, case.p, case.n)
    r.update_geometry(case.idx, *gc.original(case.idx))
    assert bit_mismatch(render(r, case), case.ref0)[0] == 0.0


def test_update_between_calls_in_flight(gpu_renderer, case):
    """set_pipeline(2), two one-frame calls in flight, then an update and a render: the update
    waits for the calls, so the result is the serial sequence's."""
    r = gpu_renderer
    fp = case.fp
    ro = cf.rand_origins(3)

    def run(depth):
        r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
        r.set_env(*case.env)
        r.resize(W, H)
        r.set_pipeline(depth)
        r.set_loop_num(0)
        r.render_async(fp, ro[0:1])
        r.render_async(fp, ro[1:2])
        r.update_geometry(case.idx, case.p, case.n)
        assert r.loop_num == 2                              # the update leaves LoopNum and the accumulation
        r.render_async(fp, ro[2:3])
        r.synchronize()
        return r.read_accum()
    try:
        piped = run(2)
        serial = run(1)
    finally:
        r.set_pipeline(1)
    assert piped.tobytes() == serial.tobytes()
    f0 = [cf.oracle_frame_params(fp, k + 1, ro[k]) for k in range(2)]
    acc, _ = orc.render(orc.OracleScene(case.sd.tri_enc, case.sd.node_enc, *case.env), f0, W, H)
    want, _ = orc.render(case.sc, [cf.oracle_frame_params(fp, 3, ro[2])], W, H, accum=acc)
    assert bit_mismatch(piped, want)[0] == 0.0


# ------------------------------------------------------------------ rejected calls, state
def test_rejected_calls_change_nothing(gpu_renderer, case):
    import torch
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    before, bounds = downloads(r), r.scene_bounds()
    nt = case.sd.counts["n_triangles"]
    dev = torch.device("cuda", 0)
    idx, p, n = case.idx[:300], case.p[:300], case.n[:300]

    def rejected(tri_index, pp, nn, **kw):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            r.update_geometry(tri_index, pp, nn, **kw)
        gc.assert_arrays_equal(downloads(r), before, what="after a rejected call")
        assert r.scene_bounds() == bounds
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    bad_idx = idx.copy()
    bad_idx[123] = nt
    rejected(t(bad_idx), t(p), t(n))                       # device form: an index out of range
    bad_idx[123] = -1
    rejected(t(bad_idx), t(p), t(n))
    bad_p = p.copy()
    bad_p[77, 1, 2] = np.nan
    rejected(t(idx), t(bad_p), t(n))                       # device form: a NaN position
    bad_n = n.copy()
    bad_n[299, 2, 0] = np.inf
    rejected(t(idx), t(p), t(bad_n))
    rejected(None, t(p), t(n), first=nt - 299)             # a range past the end
    rejected(bad_idx, p, n)                                # host form
    rejected(idx, bad_p, n)
    dup = idx.copy()
    dup[5] = dup[250]
    rejected(dup, p, n)
    big = p.copy()
    big[0, 0, 0] = F(2.0 ** 30)
    rejected(idx, big, n)
    L, h = r._L, r._h
    assert L.rt_update_geometry(h, None, 0, -1, *[None] * 6) == RT_ERR_ARG
    assert L.rt_update_geometry(h, None, 0, 0, *[None] * 6) == RT_OK
    assert L.rt_update_geometry(h, None, 0, 1, *[None] * 6) == RT_ERR_ARG
    assert L.rt_update_geometry_device(h, None, 0, 0, *[None] * 6) == RT_OK
    gc.assert_arrays_equal(downloads(r), before, what="count == 0")
    buf = np.zeros(16, np.uint8)
    assert L.rt_scene_download(h, 0, buf.ctypes.data, 16) == RT_ERR_ARG and L.rt_scene_download(h, 6, buf.ctypes.data, 16) == RT_ERR_ARG
    fresh = Renderer(0)
    try:
        a = sl.split_vertices(p, n)
        assert fresh._L.rt_update_geometry(fresh._h, None, 0, 300, *[sl._fp(x) for x in a]) == RT_ERR_STATE
        assert fresh._L.rt_scene_bounds(fresh._h, (C.c_double * 5)(), None) == RT_ERR_STATE
    finally:
        fresh.close()


def test_update_forgets_the_guides_and_keeps_the_rest(gpu_renderer, case):
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    img0 = render(r, case)
    r.denoise(case.fp, DenoiseParams(iterations=2))
    r.denoise_async(case.fp, DenoiseParams(iterations=2), reuse_guides=True)
    r.synchronize()
    st0, mats0 = r.stats(), r.triangle_material(int(case.idx[0]))
    r.update_geometry(case.idx, case.p, case.n)
    assert r.loop_num == FRAMES and r.read_accum().tobytes() == img0.tobytes()
    st1 = r.stats()
    assert {k: st1[k] for k in ("rays", "samples")} == {k: st0[k] for k in ("rays", "samples")}
    assert r.triangle_material(int(case.idx[0]))[1] == mats0[1]
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        r.denoise_async(case.fp, DenoiseParams(iterations=2), reuse_guides=True)
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        r.temporal_async(case.fp, reuse_guides=True)
    r.denoise(case.fp, DenoiseParams(iterations=2))       # fresh guides
    r.denoise_async(case.fp, DenoiseParams(iterations=2), reuse_guides=True)
    r.synchronize()


def test_session_tick_with_geometry(gpu_renderer, case):
    r = gpu_renderer
    r.set_scene_encoded(case.sd.tri_enc, case.sd.node_enc)
    r.set_env(*case.env)
    try:
        s = ia.Session(r, W, H, settings=ia.Settings(max_bounce=4))
        r.clear_accum()
        s.tick(delta_time=0.05)
        s.tick(delta_time=0.05)
        assert r.loop_num == 2
        out = s.tick(ia.Input(geometry=[(case.idx, case.p, case.n)]), delta_time=0.05)
        assert r.loop_num == 1 and out["loop_num"] == 1 and not s._guides_current
        fp = out["params"]
        want, _ = orc.render(case.sc, [cf.oracle_frame_params(fp, 1, out["rand_origin"])], W, H)
        assert bit_mismatch(r.read_accum(), want)[0] == 0.0
    finally:
        r.set_pipeline(1)
