"""Traversal on caller-built BVHs (tests/tree_cases.py) on the GPU, against the oracle on the same
buffers, bit for bit: leaves of up to 16 triangles, lopsided and random trees, loose boxes, and the
trees whose boxes do not nest (or that list a triangle twice), which the release library traces on
the binary tree.  Everything goes through rt_set_scene_encoded; queries compare whole records
(query_cases.assert_hits_equal), renders are 48 x 27 with 2 frames.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import geometry_cases as gc
import oracle as orc
import query_cases as qc
import tree_cases as tc
from helpers import bit_mismatch, frames_for, gpu_render
from rtamd import configs as cf
from rtamd import scene_lib as sl
from rtamd.renderer import RT_FLAG_FINISH, RT_FLAG_MEGAKERNEL, RT_FLAG_NO_FINISH, SCENE_ARRAYS

pytestmark = pytest.mark.gpu
F = np.float32
W, H, FRAMES = 48, 27, 2
SOME = ("M4", "M6", "N2")


@lru_cache(maxsize=None)
def rays():
    """query_cases.c2_rays and, for N2, its aimed family after them (read-only)."""
    env = cf.load_env()
    sd = cf.config_scene("C2")
    o, d = qc.c2_rays(sd, orc.OracleScene(sd.tri_enc, sd.node_enc, *env), cf.MATERIALS["jade"].texels())
    ao, ad = tc.aimed_rays(tc.tree("N2"))
    out = SimpleNamespace(o=o, d=d, n2_o=np.concatenate([o, ao]), n2_d=np.concatenate([d, ad]))
    for a in vars(out).values():
        a.flags.writeable = False
    return out


@lru_cache(maxsize=None)
def case(name):
    """The tree, its oracle scene, its rays and the oracle's answers to them (computed once)."""
    t = tc.tree(name)
    sc = orc.OracleScene(t.tri_enc, t.node_enc, *cf.load_env())
    o, d = (rays().n2_o, rays().n2_d) if name == "N2" else (rays().o, rays().d)
    ref = qc.oracle_hits(sc, o, d)
    ref.flags.writeable = False
    return SimpleNamespace(t=t, sc=sc, o=o, d=d, ref=ref)


@lru_cache(maxsize=None)
def oracle_frames(name, bsdf=True):
    """The oracle's two frames of the tree from C2's camera, and its ray count."""
    fp = cf.frame_params(W, H, enable_bsdf=bsdf)
    ro, frames = frames_for(fp, 1, FRAMES)
    img, cnt = orc.render(case(name).sc, frames, W, H)
    img.flags.writeable = False
    return ro, img, cnt["rays"]


def check_render(r, name, flags=0, bsdf=True):
    ro, ref, n_rays = oracle_frames(name, bsdf)
    fp = cf.frame_params(W, H, flags=flags, enable_bsdf=bsdf)
    img, st = gpu_render(r, case(name).t, cf.load_env(), W, H, fp, ro, encoded=True)
    frac, diff = bit_mismatch(img, ref)
    assert frac == 0.0, f"{name}: {int(diff.sum())} pixels differ, first (y, x) {tuple(np.argwhere(diff)[0])}"
    assert st["rays"] == n_rays


def check_queries(r, name, no_cull=False):
    c = case(name)
    hit = (c.ref["triangle"] >= 0).astype(np.int32)
    qc.assert_hits_equal(r.trace_rays(c.o, c.d), c.ref, f"{name} closest")
    assert np.array_equal(r.trace_rays(c.o, c.d, kind="any"), hit), f"{name} any-hit"
    if no_cull:
        qc.assert_hits_equal(r.trace_rays(c.o, c.d, no_cull=True), c.ref, f"{name} closest, RT_QUERY_NO_CULL")
        assert np.array_equal(r.trace_rays(c.o, c.d, kind="any", no_cull=True), hit), f"{name} any-hit, RT_QUERY_NO_CULL"


# ------------------------------------------------------------------ queries
@pytest.mark.parametrize("name", tc.ALL)
def test_ray_queries(gpu_renderer, name):
    c = case(name)
    assert 0.2 < (c.ref["triangle"] >= 0).mean() < 0.9
    gpu_renderer.set_scene_encoded(c.t.tri_enc, c.t.node_enc)
    check_queries(gpu_renderer, name, no_cull=name in ("M4", "N2"))
    if name == "N2":   # the aimed rays are where the halved box shows: the oracle's answers differ from M3's
        aimed = slice(len(rays().o), None)
        assert (c.ref["t"][aimed].view(np.uint32) != qc.oracle_hits(case("M3").sc, c.o[aimed], c.d[aimed])["t"].view(np.uint32)).sum() >= 8


@pytest.mark.parametrize("name", SOME)
def test_first_hit_frame(gpu_renderer, name):
    c, r = case(name), gpu_renderer
    r.set_scene_encoded(c.t.tri_enc, c.t.node_enc)
    r.resize(W, H)
    fp = cf.frame_params(W, H)
    cam = r.camera_rays(fp).reshape(-1)
    fh = r.first_hit(fp)
    assert fh.shape == (H, W) and (fh["triangle"] >= 0).mean() > 0.3
    qc.assert_hits_equal(fh.reshape(-1), qc.oracle_hits(c.sc, cam["origin"], cam["dir"]), f"{name} rt_first_hit")


# ------------------------------------------------------------------ renders
@pytest.mark.parametrize("finish", ["bulk", "finisher"])
@pytest.mark.parametrize("name", tc.ALL)
def test_render(gpu_renderer, name, finish):
    """BSDF mode from C2's camera: the bulk kernels alone (RT_FLAG_NO_FINISH), and the finisher from
    pass 1 on (RT_FLAG_FINISH), whose drained waves test four triangles of a leaf at once."""
    if finish == "bulk":
        check_render(gpu_renderer, name, RT_FLAG_NO_FINISH)
        return
    gpu_renderer.set_finish(1, 1 << 30)
    try:
        check_render(gpu_renderer, name, RT_FLAG_FINISH)
    finally:
        gpu_renderer.set_finish(2, 8 << 20)


@pytest.mark.parametrize("name", SOME)
def test_megakernel_render(gpu_renderer, name):
    check_render(gpu_renderer, name, RT_FLAG_MEGAKERNEL)


@pytest.mark.parametrize("name", SOME)
def test_brdf_render(gpu_renderer, name):
    check_render(gpu_renderer, name, bsdf=False)


@pytest.mark.parametrize("knob,value", [("RT_REBUILD", "0"), ("RT_COLLAPSE", "greedy"), ("RT_BVH_WIDTH", "2")])
def test_other_traversal_structures_of_the_random_tree(gpu_dev_renderer, monkeypatch, knob, value):
    """M6 through the development library: the 4-wide tree collapsed from the caller's own internal
    levels, the greedy collapse, and the binary tree."""
    monkeypatch.setenv(knob, value)
    c, r = case("M6"), gpu_dev_renderer
    check_render(r, "M6")
    want = sl.compile_scene_encoded(c.t.tri_enc, c.t.node_enc, rebuild=knob != "RT_REBUILD", greedy=knob == "RT_COLLAPSE")
    gc.assert_arrays_equal({k: r.scene_download(k) for k in ("nodes", "qnodes")}, want.arrays, names=("nodes", "qnodes"),
                           what=f"{knob}={value}")
    check_queries(r, "M6")


# ------------------------------------------------------------------ geometry updates
@pytest.mark.parametrize("name", ["M4", "N1"])
def test_geometry_update(gpu_renderer, name):
    """The mesh's triangles (by material) under geometry_cases' MOVE: the device arrays equal
    scn::update_geometry's byte for byte, and the hits the oracle's on the moved triangles under
    the refitted boxes (N1: the binary tree alone is refitted, and the scene stays on it)."""
    t, r = tc.tree(name), gpu_renderer
    idx, p, n = tc.moved_mesh(t, cf.MATERIALS["jade"].texels(), gc.moved("MOVE"))
    tri = t.tri_enc.copy()
    tri[idx, 0:3], tri[idx, 3:6] = p, n
    sc = orc.OracleScene(tri, gc.refit_node_enc(tri, t.node_enc), *cf.load_env())
    ref = qc.oracle_hits(sc, rays().o, rays().d)
    assert 0.2 < (ref["triangle"] >= 0).mean() < 0.9
    m = sl.CompiledHandle(t.tri_enc, t.node_enc)
    assert m.update_geometry(idx, p, n) == 0
    r.set_scene_encoded(t.tri_enc, t.node_enc)
    r.update_geometry(idx, p, n)
    s = m.snapshot()
    gc.assert_arrays_equal({k: r.scene_download(k) for k in SCENE_ARRAYS}, s.arrays, what=name)
    b = r.scene_bounds()
    assert tuple(b[k] for k in gc.BOUNDS) + (b["tri_flagged"],) == gc.bounds_of(s)
    assert (len(s.arrays["qnodes"]) == 1) == (name == "N1")
    qc.assert_hits_equal(r.trace_rays(rays().o, rays().d), ref, f"{name} moved")
    assert np.array_equal(r.trace_rays(rays().o, rays().d, kind="any"), (ref["triangle"] >= 0).astype(np.int32))
