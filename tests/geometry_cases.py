"""Shared cases of the geometry-update tests (CPU construction: numpy, librtscene, liboracle).

The scene is C2 (floor + bunny_4000).  A case moves the bunny with rtamd.geometry.moved_object and
`moved_scene` states what the update must then be equal to: the reference's encodings with the new
vertices and every node box recomputed bottom-up over the unchanged topology, in numpy, with the
reference's min / max (glm: min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a) in its order
(a leaf from +-1145141919 over its triangles in ascending index, an internal node its left child
then its right one).  The oracle and a fresh context read that scene.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from rtamd import configs as cf
from rtamd import geometry as geo
from rtamd import scene_lib as sl

F = np.float32
W, H, FRAMES = 48, 27, 2
ARRAYS = ("tri", "trx", "trin", "hrec", "nodes", "qnodes")
BOUNDS = ("cull_R", "cull_K", "cull_off", "tri_k1", "tri_k0")

# the moved bunny: a rotation, a translation and a scale below 1 (its own: (0,0,0) (2.2,-2.5,3) 2)
MOVE = dict(rotate=(20.0, 75.0, -10.0), translate=(1.6, -2.45, 2.5), scale=(1.7, 1.7, 1.7))
# the flagged path: scale 3 along one axis and 0.15 along the others (of the bunny's own 2) makes
# most triangles slivers above the filter's caps.  A uniform scale of 3 flags none: S = |A|^2 /
# (|n| cos) and sin / cos are ratios and stay where they are.
STRETCH = dict(rotate=(0.0, 30.0, 0.0), translate=(2.2, -2.5, 3.0), scale=(0.3, 6.0, 0.3))


def gmin(a, b):
    return np.where(b < a, b, a)


def gmax(a, b):
    return np.where(a < b, b, a)


def c2():
    return cf.config_scene("C2")


@lru_cache(maxsize=None)
def moved(which: str = "MOVE"):
    """(tri_index, p, n) of C2's bunny under the named transform."""
    return geo.moved_object(c2(), 1, **globals()[which])


def original(idx):
    """(p, n) of C2's own triangles idx."""
    t = c2().tri_enc
    return np.ascontiguousarray(t[idx, 0:3]), np.ascontiguousarray(t[idx, 3:6])


def refit_node_enc(tri_enc: np.ndarray, node_enc: np.ndarray) -> np.ndarray:
    """node_enc with every box recomputed from tri_enc's vertices (children follow their parent in
    the reference's numbering, so the nodes are taken from the last to the first)."""
    out = node_enc.copy()
    for i in range(len(out) - 1, 0, -1):
        left, right, n, first = int(out[i, 0, 0]), int(out[i, 0, 1]), int(out[i, 1, 0]), int(out[i, 1, 1])
        if n > 0:
            lo, hi = np.full(3, 1145141919.0, F), np.full(3, -1145141919.0, F)
            for t in range(first, first + n):
                p = tri_enc[t, 0:3]
                lo = gmin(lo, gmin(p[0], gmin(p[1], p[2])))
                hi = gmax(hi, gmax(p[0], gmax(p[1], p[2])))
        else:
            assert left > i and right > i
            lo, hi = gmin(out[left, 2], out[right, 2]), gmax(out[left, 3], out[right, 3])
        out[i, 2], out[i, 3] = lo, hi
    return out


def moved_scene(idx, p, n):
    """(tri_enc, node_enc) of C2 with triangles idx at p, n and refitted boxes."""
    sd = c2()
    tri = sd.tri_enc.copy()
    tri[idx, 0:3] = p
    tri[idx, 3:6] = n
    return tri, refit_node_enc(tri, sd.node_enc)


@lru_cache(maxsize=None)
def moved_c2(which: str = "MOVE"):
    return moved_scene(*moved(which))


def model(tri_enc=None, node_enc=None, **options) -> "sl.CompiledHandle":
    """A compile of C2 (or the given encodings) that stays alive for updates."""
    sd = c2()
    return sl.CompiledHandle(sd.tri_enc if tri_enc is None else tri_enc, sd.node_enc if node_enc is None else node_enc,
                             **options)


def bounds_of(snapshot) -> tuple:
    return tuple(snapshot.scalars[k] for k in BOUNDS) + (snapshot.scalars["tri_flagged"],)


def assert_arrays_equal(got: dict, ref: dict, names=ARRAYS, what: str = "") -> None:
    for k in names:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.nbytes == b.nbytes, f"{what}: {k} has {a.nbytes} bytes, expected {b.nbytes}"
        if a.tobytes() != b.tobytes():
            aw, bw = a.view(np.uint32).reshape(-1), b.view(np.uint32).reshape(-1)
            bad = np.flatnonzero(aw != bw)
            raise AssertionError(f"{what}: {k} differs in {bad.size} words, first at word {bad[0]} "
                                 f"({aw[bad[0]]:#x} vs {bw[bad[0]]:#x})")


def one_leaf_scene():
    """The floor alone: the root is a leaf ref, neither tree has an internal node."""
    return cf.build_scene((cf.FLOOR,))
