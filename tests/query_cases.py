"""Rays and oracle answers for the ray-query tests (CPU construction: numpy and liboracle).

`oracle_hits` calls orc_trace (oracle/rt_oracle.cpp: the reference's hitBVH, RT:338-392) once per
ray and returns the answers as the binding's HIT_DTYPE records, so a query's result compares
field by field, bit by bit.  orc_trace reports no triangle index: `triangle` is 0 for a hit and -1
for a miss here, and the tests check the library's index through what it implies (the same record
from the oracle on that triangle alone, the triangle's material).

`c2_rays` is the mixed batch of the parity tests: 4,097 rays over C2 (bunny_4000 + floor) in four
families -- from a sphere around the scene at jittered interior points, from inside the mesh's box,
secondary rays off the first family's hits, and rays with one and two exactly-zero direction
components.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle as orc
from cull_cases import normalize_f32
from rtamd.renderer import HIT_DTYPE

F = np.float32
MISS = np.zeros((), HIT_DTYPE)
MISS["t"], MISS["triangle"] = -1.0, -1


def oracle_hits(sc: "orc.OracleScene", origins, dirs) -> np.ndarray:
    L = orc.lib()
    o = np.ascontiguousarray(origins, F).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    out = np.zeros(len(o), HIT_DTYPE)
    dist, pt, nrm, inside = np.zeros(1, F), np.zeros(3, F), np.zeros(3, F), C.c_int(0)
    p = lambda a: a.ctypes.data_as(orc._f32p)  # noqa: E731
    for i in range(len(o)):
        hit = L.orc_trace(C.byref(sc.c), p(o[i]), p(d[i]), p(dist), p(pt), p(nrm), C.byref(inside))
        if hit:
            out[i]["t"], out[i]["point"], out[i]["normal"], out[i]["inside"] = dist[0], pt, nrm, inside.value
        else:
            out[i] = MISS
    return out


def assert_hits_equal(got: np.ndarray, ref: np.ndarray, what: str = "") -> None:
    """t, point, normal, inside bit for bit; hit / miss alike; a miss is the exact miss record."""
    got, ref = got.reshape(-1), ref.reshape(-1)
    assert got.shape == ref.shape
    hit = ref["triangle"] >= 0
    assert np.array_equal(got["triangle"] >= 0, hit), f"{what}: hit / miss differs at {np.flatnonzero((got['triangle'] >= 0) != hit)[:8]}"
    for k in ("t", "point", "normal", "inside"):
        a = np.ascontiguousarray(got[k]).view(np.uint32).reshape(len(got), -1)
        b = np.ascontiguousarray(ref[k]).view(np.uint32).reshape(len(ref), -1)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, f"{what}: {k} differs for {bad.size} rays, first {bad[:8]}: {got[k][bad[0]]} vs {ref[k][bad[0]]}"
    miss = got[~hit]
    assert miss.tobytes() == np.full(len(miss), MISS).tobytes(), f"{what}: a miss is not the exact miss record"
    assert not got["pad_"].any()


def single_triangle_scene(sd_tri_enc: np.ndarray, tri: int, env) -> "orc.OracleScene":
    """The oracle's scene of triangle `tri` alone: one leaf holding it, in its own box."""
    t = np.ascontiguousarray(sd_tri_enc[tri:tri + 1], F)
    nodes = np.zeros((2, 4, 3), F)
    nodes[1, 1] = (1, 0, 0)
    nodes[1, 2], nodes[1, 3] = t[0, 0:3].min(0), t[0, 0:3].max(0)
    return orc.OracleScene(t, nodes, env[0], env[1])


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return normalize_f32((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F))


def c2_rays(sd, sc, mesh_material) -> tuple:
    """(origins, dirs) of the 4,097 rays; sd: cf.config_scene("C2"), sc: its OracleScene,
    mesh_material: the 24 texels of the mesh's material (its triangles give the mesh's box)."""
    rng = np.random.default_rng(20240607)
    tri = sd.tri_enc
    is_mesh = (tri[:, 6:14].reshape(len(tri), 24) == np.asarray(mesh_material, F)[None]).all(axis=1)
    pts = tri[is_mesh, 0:3].reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    # 1: from a sphere around the scene at jittered points of the mesh's box
    n1 = 1400
    o1 = (centre + 6.0 * _unit(rng, n1)).astype(F)
    target = centre + rng.uniform(-1.1, 1.1, size=(n1, 3)) * half
    d1 = normalize_f32((target - o1).astype(F))
    # 2: origins inside the mesh's box
    n2 = 1200
    o2 = (centre + rng.uniform(-1.0, 1.0, size=(n2, 3)) * half).astype(F)
    d2 = _unit(rng, n2)
    # 3: secondary rays: an earlier hit point pushed along its normal by 1e-3, hemisphere direction
    n3 = 1200
    h1 = oracle_hits(sc, o1, d1)
    src = np.flatnonzero(h1["triangle"] >= 0)
    assert src.size >= 400, "the first family hardly hits the scene"
    src = src[rng.integers(0, src.size, n3)]
    nrm = h1["normal"][src]
    o3 = (h1["point"][src] + nrm * F(1e-3)).astype(F)
    d3 = _unit(rng, n3)
    d3 = np.where((d3 * nrm).sum(1, keepdims=True) < 0, -d3, d3).astype(F)
    # 4: one (200) and two (97) exactly-zero direction components, through the mesh's box
    n4a, n4b = 200, 97
    t4 = (centre + rng.uniform(-0.9, 0.9, size=(n4a + n4b, 3)) * half).astype(F)
    d4 = _unit(rng, n4a + n4b)
    d4[np.arange(n4a), rng.integers(0, 3, n4a)] = 0.0
    keep = rng.integers(0, 3, n4b)
    for a in range(3):
        d4[n4a:, a] = np.where(keep == a, np.sign(d4[n4a:, a]) + (d4[n4a:, a] == 0), 0.0)
    d4 = normalize_f32(d4.astype(F))
    o4 = (t4 - d4 * F(5.0)).astype(F)
    assert ((d4[:n4a] == 0).sum(1) >= 1).all() and ((d4[n4a:] == 0).sum(1) == 2).all()
    o = np.concatenate([o1, o2, o3, o4]).astype(F)
    d = np.concatenate([d1, d2, d3, d4]).astype(F)
    assert len(o) == 4097 and np.isfinite(o).all() and np.isfinite(d).all()
    return o, d
