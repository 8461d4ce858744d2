"""Ray queries (rt_abi.h ABI 7) on the GPU against the oracle's hitBVH, ray by ray.

Every closest-hit comparison is bitwise on t, point, normal and inside against orc_trace
(query_cases.oracle_hits); orc_trace reports no triangle index, so the library's `triangle` is
checked through what it implies: the oracle's record on that triangle alone is the same record,
its material is the scene's, and it does not depend on culling or on the direction's length.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import cull_cases
import edge_cases
import oracle as orc
import query_cases as qc
from helpers import bit_mismatch
from rtamd import configs as cf
from rtamd import interactive as ia
from rtamd import scene_lib as sl
from rtamd.renderer import (HIT_DTYPE, RAY_DTYPE, RT_ERR_ARG, RT_ERR_STATE, RT_HIT_INVALID, RT_OK, RT_QUERY_ANY,
                            RT_QUERY_CLOSEST, Renderer)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def c2(env_maps):
    """C2, its oracle scene, the 4,097 rays of query_cases.c2_rays and the oracle's answers
    (computed once; read-only)."""
    sd = cf.config_scene("C2")
    sc = orc.OracleScene(sd.tri_enc, sd.node_enc, *env_maps)
    o, d = qc.c2_rays(sd, sc, cf.MATERIALS["jade"].texels())
    ref = qc.oracle_hits(sc, o, d)
    for a in (o, d, ref):
        a.flags.writeable = False
    return SimpleNamespace(sd=sd, sc=sc, o=o, d=d, ref=ref)


@pytest.fixture(scope="module")
def c2_gpu(gpu_renderer, c2):
    """The release library's closest hits of all c2 rays (the tests of sizes, chunks and invalid
    rays compare with slices of it)."""
    gpu_renderer.set_scene_soa(c2.sd.soa, c2.sd.nodes)
    got = gpu_renderer.trace_rays(c2.o, c2.d)
    got.flags.writeable = False
    return got


def _check_triangles(sd, env, got, o, d, sample=48):
    """`triangle` and `material` of the hits: the scene's material id of that triangle, and (for a
    sample) the oracle's record on that triangle alone, which must be the same record."""
    hit = np.flatnonzero(got["triangle"] >= 0)
    tri = got["triangle"][hit]
    assert tri.max() < len(sd.tri_enc)
    assert np.array_equal(got["material"][hit], np.asarray(sd.soa["material_id"])[tri])
    for i in hit[:: max(1, len(hit) // sample)]:
        one = qc.oracle_hits(qc.single_triangle_scene(sd.tri_enc, int(got["triangle"][i]), env), o[i], d[i])
        qc.assert_hits_equal(got[i:i + 1], one, f"ray {i} on its triangle alone")


def _scene(tri_enc, node_enc, env):
    return SimpleNamespace(tri_enc=tri_enc, node_enc=node_enc), orc.OracleScene(tri_enc, node_enc, *env)


# ------------------------------------------------------------------ 1, 2: parity on a real mesh
def test_parity_on_a_real_mesh(gpu_renderer, env_maps, c2, c2_gpu):
    """4,097 rays of four families over C2: closest hits equal orc_trace bit for bit, any-hit says
    occluded exactly where orc_trace hits, and the exhaustive order gives the identical records."""
    r, got = gpu_renderer, c2_gpu
    qc.assert_hits_equal(got, c2.ref, "closest")
    hits = c2.ref["triangle"] >= 0
    for lo, hi in ((0, 1400), (1400, 2600), (2600, 3800), (3800, 4097)):  # every family finds the scene
        assert hits[lo:hi].mean() > 0.05, (lo, hits[lo:hi].mean())
    assert (~hits).sum() > 100
    _check_triangles(c2.sd, env_maps, got, c2.o, c2.d)
    r.set_scene_soa(c2.sd.soa, c2.sd.nodes)
    occ = r.trace_rays(c2.o, c2.d, kind="any")
    assert occ.dtype == np.int32 and np.array_equal(occ, hits.astype(np.int32))
    assert r.trace_rays(c2.o, c2.d, no_cull=True).tobytes() == got.tobytes()
    assert np.array_equal(r.trace_rays(c2.o, c2.d, kind="any", no_cull=True), occ)


@pytest.mark.parametrize("scale", [0.37, 5.0])
def test_non_unit_directions(gpu_renderer, c2, c2_gpu, scale):
    """Directions of length 0.37 and 5: the records equal orc_trace's on the scaled rays (t in
    units of the direction), and the closest triangle is the unit-length run's."""
    n = 1024
    o, d = c2.o[:n], (c2.d[:n] * F(scale)).astype(F)
    ref = qc.oracle_hits(c2.sc, o, d)
    gpu_renderer.set_scene_soa(c2.sd.soa, c2.sd.nodes)
    got = gpu_renderer.trace_rays(o, d)
    qc.assert_hits_equal(got, ref, f"scale {scale}")
    assert np.array_equal(got["triangle"], c2_gpu["triangle"][:n])
    assert np.array_equal(gpu_renderer.trace_rays(o, d, kind="any"), (ref["triangle"] >= 0).astype(np.int32))
    assert gpu_renderer.trace_rays(o, d, no_cull=True).tobytes() == got.tobytes()


def test_binary_tree_kernels(gpu_dev_renderer, monkeypatch, c2, c2_gpu):
    """RT_BVH_WIDTH=2 (development library): a scene without the 4-wide tree is traced by the binary
    tree's kernel, which takes closest- and any-hit rays from one queue."""
    monkeypatch.setenv("RT_BVH_WIDTH", "2")
    r, n = gpu_dev_renderer, 257
    r.set_scene_soa(c2.sd.soa, c2.sd.nodes)
    assert r.trace_rays(c2.o[:n], c2.d[:n]).tobytes() == c2_gpu[:n].tobytes()
    assert np.array_equal(r.trace_rays(c2.o[:n], c2.d[:n], kind="any"), (c2.ref["triangle"][:n] >= 0).astype(np.int32))


# ------------------------------------------------------------------ 3: adversarial traversal cases
def test_hits_exactly_on_a_shared_edge(gpu_renderer, env_maps):
    """edge_cases.diagonal_scene: the diagonal pixels' rays land on the quad's shared edge, which
    the reference's strict edge signs reject for both triangles (the ray goes on to the wall)."""
    W = 64
    es = edge_cases.diagonal_scene()
    sd, sc = _scene(es["tri_enc"], es["node_enc"], env_maps)
    d = edge_cases.diagonal_camera_rays(W)
    o = np.tile(np.array([0.0, 0.0, 3.0], F), (W, 1))
    ref = qc.oracle_hits(sc, o, d)
    wall = np.abs(ref["point"][:, 2] + F(1.0)) < 1e-4  # the wall behind the quad
    assert wall.sum() > W // 2
    gpu_renderer.set_scene_encoded(sd.tri_enc, sd.node_enc)
    got = gpu_renderer.trace_rays(o, d)
    qc.assert_hits_equal(got, ref, "diagonal")
    assert (got["triangle"][wall] == 2).all()
    assert gpu_renderer.trace_rays(o, d, no_cull=True).tobytes() == got.tobytes()


def test_cull_margin_counterexample_ray(gpu_renderer, env_maps):
    """cull_cases.old_margin_counterexample: the accepted hit lies before its own box's entry, so a
    traversal that culled that box with the round-1 margin returns the wall behind it."""
    ce = cull_cases.old_margin_counterexample()
    sd, sc = _scene(ce["tri_enc"], ce["node_enc"], env_maps)
    o, d = ce["position"][None], ce["direction"][None]
    ref = qc.oracle_hits(sc, o, d)
    assert abs(float(ref["t"][0]) - ce["t_hit"]) < 1e-3
    gpu_renderer.set_scene_encoded(sd.tri_enc, sd.node_enc)
    got = gpu_renderer.trace_rays(o, d)
    qc.assert_hits_equal(got, ref, "counterexample")
    assert got["triangle"][0] == 0  # T, not the walls
    assert gpu_renderer.trace_rays(o, d, no_cull=True).tobytes() == got.tobytes()


@pytest.mark.parametrize("swap", [False, True])
def test_exact_distance_tie_goes_to_the_oracles_winner(gpu_renderer, env_maps, swap):
    """Two coincident triangles in different leaves with different vertex normals: both are hit at
    exactly the same distance, the reference keeps the first it meets (RT:356 is strict), and the
    normal of the record says which one that was."""
    p = [np.array(v, F) for v in ((-1.0, -1.0, 0.0), (1.5, -1.0, 0.0), (0.0, 1.25, 0.0))]
    a = cull_cases._tri_enc(*p, (1, 0, 0))
    b = cull_cases._tri_enc(*p, (0, 1, 0))
    b[3] = b[4] = b[5] = np.array([0.6, 0.0, 0.8], F)  # (the other's normals are (0, 0, 1): x = 0)
    tri_enc = np.stack([b, a] if swap else [a, b])
    box = (np.min(p, 0), np.max(p, 0))
    nodes = np.zeros((4, 4, 3), F)
    nodes[1] = [(2, 3, 0), (0, 0, 0), box[0], box[1]]
    nodes[2] = [(0, 0, 0), (1, 0, 0), box[0], box[1]]
    nodes[3] = [(0, 0, 0), (1, 1, 0), box[0], box[1]]
    sd, sc = _scene(tri_enc, nodes, env_maps)
    rng = np.random.default_rng(3)
    o = np.concatenate([np.array([[0.1, -0.2, 2.0]]), rng.uniform(-0.4, 0.4, (15, 3)) + (0.1, -0.2, 2.0)]).astype(F)
    d = cull_cases.normalize_f32(np.concatenate([np.array([[0.0, 0.0, -1.0]]), rng.normal(0, 0.1, (15, 3)) + (0, 0, -1.0)]).astype(F))
    ref = qc.oracle_hits(sc, o, d)
    assert (ref["triangle"] >= 0).all()
    gpu_renderer.set_scene_encoded(sd.tri_enc, sd.node_enc)
    for no_cull in (False, True):
        got = gpu_renderer.trace_rays(o, d, no_cull=no_cull)
        qc.assert_hits_equal(got, ref, f"tie swap={swap} no_cull={no_cull}")
        winner_tilted = got["normal"][:, 0] != 0
        assert np.array_equal(got["triangle"], np.where(winner_tilted, 0 if swap else 1, 1 if swap else 0))


def test_chain_bvh_at_the_depth_limit(gpu_renderer, env_maps):
    """The 64-level chain of tests/test_gpu_parity.py: a ray down the chain stacks a far child on
    every level (the overflow stack of the query's own launches)."""
    from test_gpu_parity import _deep_chain_scene
    tri, nodes = _deep_chain_scene(64)
    sd, sc = _scene(tri, nodes, env_maps)
    rng = np.random.default_rng(9)
    o = np.concatenate([np.array([[0.0, 0.0, 5.0]]), rng.uniform(-3, 3, (64, 3)) * (1, 1, 0) + (0, 0, 5.0)]).astype(F)
    d = cull_cases.normalize_f32(np.concatenate([np.array([[0.0, 0.0, -1.0]]), rng.normal(0, 0.2, (64, 3)) + (0, 0, -1.0)]).astype(F))
    ref = qc.oracle_hits(sc, o, d)
    assert ref["triangle"][0] >= 0 and ref["point"][0, 2] == F(0.0)  # the nearest plane
    gpu_renderer.set_scene_encoded(sd.tri_enc, sd.node_enc)
    got = gpu_renderer.trace_rays(o, d)
    qc.assert_hits_equal(got, ref, "chain")
    assert got["triangle"][0] == 63
    assert np.array_equal(gpu_renderer.trace_rays(o, d, kind="any"), (ref["triangle"] >= 0).astype(np.int32))


# ------------------------------------------------------------------ 4: sizes and chunks
def _raw_trace(r, o, d, kind, extra=1):
    """rt_trace_rays into a buffer with `extra` sentinel records after out[n]."""
    n = len(o)
    rays = np.zeros(max(1, n), RAY_DTYPE)
    rays["origin"][:n], rays["dir"][:n] = o, d
    rec = HIT_DTYPE.itemsize if kind == RT_QUERY_CLOSEST else 4
    buf = np.full((n + extra) * rec, 0x5A, np.uint8)
    rc = r._L.rt_trace_rays(r._h, rays.ctypes.data, n, kind, 0, buf.ctypes.data)
    assert (buf[n * rec:] == 0x5A).all(), "the sentinel after out[n] was overwritten"
    return rc, buf[:n * rec].view(HIT_DTYPE if kind == RT_QUERY_CLOSEST else np.int32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(gpu_renderer, c2, c2_gpu, n):
    """Ray counts around the wave size: the first n records of the full batch, nothing past out[n]."""
    r = gpu_renderer
    r.set_scene_soa(c2.sd.soa, c2.sd.nodes)
    # (rays 2600..: the secondary family, hits and misses mixed)
    o, d, ref = c2.o[2600:2600 + n], c2.d[2600:2600 + n], c2_gpu[2600:2600 + n]
    rc, got = _raw_trace(r, o, d, RT_QUERY_CLOSEST)
    assert rc == RT_OK and got.tobytes() == ref.tobytes()
    rc, occ = _raw_trace(r, o, d, RT_QUERY_ANY)
    assert rc == RT_OK and np.array_equal(occ, (ref["triangle"] >= 0).astype(np.int32))


def test_chunks(gpu_dev_renderer, monkeypatch, c2, c2_gpu):
    """RT_QUERY_CHUNK=1024 (development library): 3 x 1024 + 17 rays run as four chunks and equal
    the unchunked result of the release library; nothing is written past out[n]."""
    monkeypatch.setenv("RT_QUERY_CHUNK", "1024")
    r, n = gpu_dev_renderer, 3 * 1024 + 17
    r.set_scene_soa(c2.sd.soa, c2.sd.nodes)
    rc, got = _raw_trace(r, c2.o[:n], c2.d[:n], RT_QUERY_CLOSEST)
    assert rc == RT_OK and got.tobytes() == c2_gpu[:n].tobytes()
    rc, occ = _raw_trace(r, c2.o[:n], c2.d[:n], RT_QUERY_ANY)
    assert rc == RT_OK and np.array_equal(occ, (c2_gpu["triangle"][:n] >= 0).astype(np.int32))


# ------------------------------------------------------------------ 5: invalid rays
INVALID = np.zeros((), HIT_DTYPE)
INVALID["t"], INVALID["triangle"] = -1.0, RT_HIT_INVALID


def test_invalid_rays(gpu_renderer, c2, c2_gpu):
    """Rays 3, 64 and 129 of a 130-ray batch are malformed (NaN origin, infinite direction, zero
    direction): they come back RT_HIT_INVALID, the call succeeds, and every other ray has its
    result from the batch without them.  On the device entry point a ray outside origin_bound is
    answered the same way."""
    import torch
    r, n = gpu_renderer, 130
    r.set_scene_soa(c2.sd.soa, c2.sd.nodes)
    o, d = c2.o[1300:1300 + n].copy(), c2.d[1300:1300 + n].copy()
    clean = c2_gpu[1300:1300 + n]
    o[3, 1] = np.nan
    d[64, 0] = np.inf
    d[129] = 0.0
    bad = np.zeros(n, bool)
    bad[[3, 64, 129]] = True
    got = r.trace_rays(o, d)
    assert got[~bad].tobytes() == clean[~bad].tobytes()
    assert got[bad].tobytes() == np.full(3, INVALID).tobytes()
    occ = r.trace_rays(o, d, kind="any")
    assert np.array_equal(occ[~bad], (clean["triangle"][~bad] >= 0).astype(np.int32)) and (occ[bad] == RT_HIT_INVALID).all()
    # device pointers: ray 17's origin lies outside the bound the caller states
    bound = float(np.abs(o[~bad]).max())
    o[17, 2] = F(bound * 4)
    bad[17] = True
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["dir"] = o, d
    for kind, rec in (("closest", HIT_DTYPE), ("any", np.dtype(np.int32))):
        d_rays = torch.from_numpy(rays.view(np.float32).copy()).cuda()
        d_out = torch.full((n * rec.itemsize + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # torch's stream filled the buffers the ctx stream uses
        r.trace_rays_device(d_rays.data_ptr(), n, d_out.data_ptr(), bound, kind=kind)
        r.synchronize()
        raw = d_out.cpu().numpy()
        assert (raw[n * rec.itemsize:] == 0x5A).all()
        res = raw[:n * rec.itemsize].view(rec)
        if kind == "closest":
            assert res[~bad].tobytes() == clean[~bad].tobytes()
            assert res[bad].tobytes() == np.full(4, INVALID).tobytes()
        else:
            assert np.array_equal(res[~bad], (clean["triangle"][~bad] >= 0).astype(np.int32)) and (res[bad] == RT_HIT_INVALID).all()


# ------------------------------------------------------------------ 6: empty scene, state errors
def test_empty_scene_and_state_errors(gpu_renderer, c2):
    """No triangles: every ray is the exact miss record.  Before rt_set_scene: RT_ERR_STATE; a bad
    kind, unknown flags or null pointers: RT_ERR_ARG; n == 0: RT_OK."""
    s = sl.Scene()
    s.build_bvh(8)
    gpu_renderer.set_scene_soa(s.export_soa(), s.nodes())
    got = gpu_renderer.trace_rays(c2.o[:65], c2.d[:65])
    assert got.tobytes() == np.full(65, qc.MISS).tobytes()
    assert not gpu_renderer.trace_rays(c2.o[:65], c2.d[:65], kind="any").any()
    rays = np.zeros(4, RAY_DTYPE)
    rays["dir"] = (0, 0, -1)
    out = np.zeros(4, HIT_DTYPE)
    L, h = gpu_renderer._L, gpu_renderer._h
    assert L.rt_trace_rays(h, rays.ctypes.data, 4, 2, 0, out.ctypes.data) == RT_ERR_ARG
    assert L.rt_trace_rays(h, rays.ctypes.data, 4, RT_QUERY_CLOSEST, 6, out.ctypes.data) == RT_ERR_ARG
    assert L.rt_trace_rays(h, None, 4, RT_QUERY_CLOSEST, 0, out.ctypes.data) == RT_ERR_ARG
    assert L.rt_trace_rays(h, rays.ctypes.data, 4, RT_QUERY_CLOSEST, 0, None) == RT_ERR_ARG
    assert L.rt_trace_rays(h, None, 0, RT_QUERY_CLOSEST, 0, None) == RT_OK
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        gpu_renderer.trace_rays(c2.o[:4], c2.d[:4], kind=7)
    fresh = Renderer(0)
    try:
        assert fresh._L.rt_trace_rays(fresh._h, rays.ctypes.data, 4, RT_QUERY_CLOSEST, 0, out.ctypes.data) == RT_ERR_STATE
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            fresh.pick(cf.frame_params(64, 36), 0, 0)
    finally:
        fresh.close()


# ------------------------------------------------------------------ 7: camera rays
def _camera_rays_numpy(fp, W, H):
    """wf_camera in numpy fp32, one correctly rounded operation per step, in its order:
    u = (px + 0.5) / W, d = lbc + (u * 2 * half_w) * right + (v * 2 * half_h) * up, then
    d * (1 / sqrt(d . d)) (rt_device.h normalize)."""
    px, py = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    u = (px + F(0.5)) / F(W)
    v = (py + F(0.5)) / F(H)
    a = (u * F(2.0)) * F(fp.half_w)
    b = (v * F(2.0)) * F(fp.half_h)
    lbc, right, up = (np.asarray(x, F) for x in (fp.left_bottom_corner, fp.right, fp.up))
    d = np.stack([(lbc[k] + a * right[k]) + b * up[k] for k in range(3)], axis=-1)
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    inv = F(1.0) / np.sqrt(dd)
    return (d * inv[..., None]).astype(F)


def test_camera_rays_match_the_numpy_restatement(gpu_renderer):
    W, H = 48, 40
    fp = cf.frame_params(W, H, position=(0.3, -0.2, 6.5))
    gpu_renderer.resize(W, H)
    rays = gpu_renderer.camera_rays(fp)
    assert rays.shape == (H, W)
    assert np.array_equal(rays["origin"].view(np.uint32), np.broadcast_to(np.asarray(fp.position, F), (H, W, 3)).view(np.uint32))
    assert np.array_equal(rays["dir"].view(np.uint32), _camera_rays_numpy(fp, W, H).view(np.uint32))


# ------------------------------------------------------------------ 8: first-hit frame and pick
@pytest.fixture(scope="module")
def c3(env_maps):
    sd = cf.config_scene("C3")
    return SimpleNamespace(sd=sd, sc=orc.OracleScene(sd.tri_enc, sd.node_enc, *env_maps))


def test_first_hit_frame_and_pick(gpu_renderer, env_maps, c3):
    """C3 at 64 x 36: the first-hit frame equals orc_trace on the camera rays, pixel by pixel; a
    pick equals the frame's record of its pixel; the picked triangle's material is the one the
    scene gave its object, and after rt_update_materials the new one."""
    W, H = 64, 36
    r, sd = gpu_renderer, c3.sd
    r.set_scene_soa(sd.soa, sd.nodes)
    r.resize(W, H)
    fp = cf.frame_params(W, H)
    rays = r.camera_rays(fp)
    ref = qc.oracle_hits(c3.sc, rays["origin"].reshape(-1, 3), rays["dir"].reshape(-1, 3))
    fh = r.first_hit(fp)
    assert fh.shape == (H, W)
    qc.assert_hits_equal(fh, ref, "first hit")
    assert 0.3 < (fh["triangle"] >= 0).mean() < 1.0
    _check_triangles(sd, env_maps, fh.reshape(-1), rays["origin"].reshape(-1, 3), rays["dir"].reshape(-1, 3))
    # the same frame from the caller-ray entry point (another kernel family, the same records)
    assert r.trace_rays(rays["origin"].reshape(-1, 3), rays["dir"].reshape(-1, 3)).tobytes() == fh.tobytes()
    for px, py in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (31, 7), (9, 20), (50, 30)):
        assert r.pick(fp, px, py).tobytes() == fh[py, px].tobytes(), (px, py)
    for px, py in ((-1, 0), (W, 0), (0, H)):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            r.pick(fp, px, py)
    # materials: each hit triangle carries the texels the scene encoded for its object
    plane, copper = cf.MATERIALS["plane"].texels(), cf.MATERIALS["copper"].texels()
    seen = set()
    hit = np.argwhere(fh["triangle"] >= 0)
    for py, px in hit[:: max(1, len(hit) // 40)]:
        tri = int(fh[py, px]["triangle"])
        m, mid = r.triangle_material(tri)
        assert mid == fh[py, px]["material"] and np.array_equal(m, sd.tri_enc[tri, 6:14].reshape(24))
        assert np.array_equal(m, plane) or np.array_equal(m, copper)
        seen.add(bool(np.array_equal(m, copper)))
    assert seen == {True, False}
    py, px = (int(v) for v in np.argwhere(fh["triangle"] >= 0)[len(hit) // 2])
    tri = int(fh[py, px]["triangle"])
    new = cf.MATERIALS["golden"].texels()
    try:
        r.update_materials(tri, 1, new)
        m, mid = r.triangle_material(tri)
        assert np.array_equal(m, new) and mid == np.asarray(sd.soa["materials"]).size // 24  # a new table entry
        again = r.pick(fp, px, py)
        assert again["material"] == mid and again["triangle"] == tri
        assert again["t"] == fh[py, px]["t"]
    finally:
        r.set_scene_soa(sd.soa, sd.nodes)


def test_first_hit_two_ranks_merge_to_the_single_rank_frame(gpu_renderer, c3):
    """48 x 40 in 16-px tiles (the frame is no tile multiple) over two ranks: each rank's
    RT_LAYOUT_FRAME output holds its own pixels only, and the two merge to the single-rank frame.
    A pick of another rank's pixel is refused."""
    W, H = 48, 40
    fp = cf.frame_params(W, H)
    r, sd = gpu_renderer, c3.sd
    r.set_scene_soa(sd.soa, sd.nodes)
    r.resize(W, H)
    whole, whole_rays = r.first_hit(fp), r.camera_rays(fp)
    merged, merged_rays = np.zeros((H, W), HIT_DTYPE), np.zeros((H, W), RAY_DTYPE)
    owned = np.zeros((H, W), int)
    try:
        for rank in range(2):
            r.resize(W, H, tile=16, rank=rank, world=2)
            part, part_rays = r.first_hit(fp), r.camera_rays(fp)
            ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
            mine = (ty * 3 + tx) % 2 == rank
            assert not part[~mine].tobytes().strip(b"\0") and not part_rays[~mine].tobytes().strip(b"\0")
            merged[mine], merged_rays[mine] = part[mine], part_rays[mine]
            owned += mine
            py, px = (int(v) for v in np.argwhere(~mine)[0])
            with pytest.raises(RuntimeError, match=r"\(-1\)"):
                r.pick(fp, px, py)
            py, px = (int(v) for v in np.argwhere(mine)[-1])
            assert r.pick(fp, px, py).tobytes() == whole[py, px].tobytes()
    finally:
        r.resize(W, H)
    assert (owned == 1).all()
    assert merged.tobytes() == whole.tobytes() and merged_rays.tobytes() == whole_rays.tobytes()


def test_first_hit_device_is_the_local_tile_layout(gpu_renderer, c3):
    """rt_first_hit_device: rt_hit records in local-tile order on the device, enqueued on the ctx
    stream; un-permuted on the host they are rt_first_hit's frame."""
    import torch
    W, H, T = 48, 40, 32
    fp = cf.frame_params(W, H)
    r, sd = gpu_renderer, c3.sd
    r.set_scene_soa(sd.soa, sd.nodes)
    r.resize(W, H)
    frame = r.first_hit(fp)
    tiles = r.accum_device()["local_tiles"]
    buf = torch.zeros(tiles * T * T * HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.first_hit_device(fp, buf.data_ptr())
    r.synchronize()
    loc = buf.cpu().numpy().view(HIT_DTYPE).reshape(tiles, T, T)
    tx_n = (W + T - 1) // T
    for t in range(tiles):
        y0, x0 = (t // tx_n) * T, (t % tx_n) * T
        h, w = min(T, H - y0), min(T, W - x0)
        assert loc[t, :h, :w].tobytes() == frame[y0:y0 + h, x0:x0 + w].tobytes()


# ------------------------------------------------------------------ 9: rendering is undisturbed
STAT_KEYS = ("rays", "samples", "launches", "trace_launches", "path_steps")


def test_rendering_is_undisturbed_by_queries(gpu_renderer, env_maps, c2, c3):
    """C3 at 64 x 36, rt_set_pipeline(2): the accumulation, LoopNum and the rt_stats counters of
    render calls with queries between them equal those of the same calls without.

    Whether a one-frame call is pipelined depends on whether the previous call has finished when it
    is made (tests/test_gpu_launch_structure.py: its group count, hence trace_launches, is not
    fixed), and rt_pick waits for its result as rt_read_accum does.  So the schedule with a pick
    after each call is compared with the same schedule synchronising there, every counter
    included; the free-running schedule (device-form queries only, nothing waits) compares
    everything but trace_launches, which its own timing decides; the bulk call compares all."""
    import torch
    W, H, n = 64, 36, 513
    r, sd = gpu_renderer, c3.sd
    fp = cf.frame_params(W, H)
    ro = cf.rand_origins(16)
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env_maps)
    r.resize(W, H)
    want = r.trace_rays(c2.o[:n], c2.d[:n])
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["dir"] = c2.o[:n], c2.d[:n]
    d_rays = torch.from_numpy(rays.view(np.float32).copy()).cuda()
    outs = [torch.zeros(n * HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(9)]
    torch.cuda.synchronize()  # torch's stream filled the buffers the ctx stream uses
    used = []

    def device_query(k):  # asynchronous, on the ctx stream
        used.append(outs[len(used)])
        r.trace_rays_device(d_rays.data_ptr(), n, used[-1].data_ptr(), float(np.abs(c2.o[:n]).max()))

    def queries_waiting(k):
        device_query(k)
        r.pick(fp, 5 * k + 3, 4 * k + 2)

    def run(calls, between):
        r.reset()
        r.clear_accum()
        r.reset_stats()
        for k, nf in calls:
            r.render_async(fp, ro[k:k + nf])
            between(k)
        st = r.stats()
        return r.read_accum(), r.loop_num, st

    ones = [(k, 1) for k in range(4)]
    r.set_pipeline(2)
    try:
        for with_q, without, keys in ((queries_waiting, lambda k: r.synchronize(), STAT_KEYS),
                                      (device_query, lambda k: None, tuple(k for k in STAT_KEYS if k != "trace_launches"))):
            img0, loop0, st0 = run(ones, without)
            img1, loop1, st1 = run(ones, with_q)
            assert loop0 == loop1 == 4
            assert bit_mismatch(img1, img0)[0] == 0.0
            assert {k: st1[k] for k in keys} == {k: st0[k] for k in keys}
        img0, loop0, st0 = run([(0, 16)], lambda k: None)
        img1, loop1, st1 = run([(0, 16)], queries_waiting)
        assert loop0 == loop1 == 16 and bit_mismatch(img1, img0)[0] == 0.0
        assert {k: st1[k] for k in STAT_KEYS} == {k: st0[k] for k in STAT_KEYS}
        r.synchronize()
        assert len(used) == 9
        for d_out in used:  # the queries themselves were answered
            assert d_out.cpu().numpy().tobytes() == want.tobytes()
    finally:
        r.set_pipeline(1)


# ------------------------------------------------------------------ 10: interactive pick
def test_interactive_pick(gpu_renderer, env_maps, c3):
    """Session.tick(Input(pick=(x, y))): out["pick"] is orc_trace on that pixel's camera ray, and
    the displayed image is the one the same tick shows without the pick."""
    W, H = 64, 36
    r, sd = gpu_renderer, c3.sd
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env_maps)
    x, y = 40.5, 20.25
    images = []
    for pick in (None, (x, y)):
        s = ia.Session(r, W, H, settings=ia.Settings(max_bounce=4))
        r.clear_accum()
        s.tick(ia.Input(), delta_time=0.05)
        out = s.tick(ia.Input(keys=["w"], pick=pick), delta_time=0.05)
        images.append(out["image"])
    assert np.array_equal(images[0], images[1])
    p = out["pick"]
    px, py = 40, H - 1 - 20
    assert p["pixel"] == (px, py)
    ray = r.camera_rays(out["params"])[py, px]
    ref = qc.oracle_hits(c3.sc, ray["origin"], ray["dir"])[0]
    assert ref["triangle"] >= 0 and p["triangle"] >= 0
    assert F(p["t"]).tobytes() == ref["t"].tobytes()
    assert p["point"].tobytes() == ref["point"].tobytes() and p["normal"].tobytes() == ref["normal"].tobytes()
    assert p["inside"] == bool(ref["inside"])
    assert np.array_equal(p["material"].texels(), sd.tri_enc[p["triangle"], 6:14].reshape(24))
    assert p["material_id"] == sd.soa["material_id"][p["triangle"]]
