"""BVHs the reference's builder never makes, over C2's triangles (CPU construction: numpy only).

rt_set_scene accepts any tree that passes scn::compile; the scenes of the other tests all come from
rts_scene_build_bvh(..., 8).  `build` is a second builder: a leaf cap up to 16, three split rules and
exact boxes, in the reference's encodings (edge_cases.py shows the layout: node 0 a dummy, the root
node 1, an internal row (left, right, 0) (0, 0, 0), a leaf row (0, 0, 0) (n, index, 0), then AA and
BB); nodes are numbered in pre-order and the triangles laid out in leaf order.  The perturbations
below then loosen or break the boxes.  `tree(name)` gives the named cases:

  nested (the 4-wide traversal stays)
    M1 full cap 1        M2 full cap 3       M3 full cap 9       M4 full cap 16
    M5 lopsided cap 13   M6 random cap 16
    M7   M4, every leaf box padded by 5 % of its extent, every internal box the union of its padded
         children padded again: loose but nested
    M8a / M8b   the project's own builder at leaf_size 16 / 1
  not nested
    N1   M4, leaf boxes padded by a quarter of their extent, parents exact
    N2   M3, one internal box halved along its longest axis, its upper half cut off: the deepest
         internal node that still holds at least 256 triangles (of several that deep, the one
         with the most triangles wholly in the cut-off half)
    N3   M3, one leaf box (the middle leaf's) shrunk past one of its vertices
    N4   M3, the middle leaf's range moved two triangles into its predecessor's

`check` is the self-check every tree passes on the CPU (tests/test_tree_cases.py).
"""
from __future__ import annotations

import dataclasses
from functools import lru_cache

import numpy as np

from cull_cases import normalize_f32
from rtamd import configs as cf

F = np.float32
NESTED = ("M1", "M2", "M3", "M4", "M5", "M6", "M7", "M8a", "M8b")
NOT_NESTED = ("N1", "N2", "N3", "N4")
ALL = NESTED + NOT_NESTED
N2_MIN_TRIANGLES = 256


@dataclasses.dataclass
class Tree:
    name: str
    tri_enc: np.ndarray    # (nt, 14, 3)
    node_enc: np.ndarray   # (nn, 4, 3)
    nested: bool
    perm: np.ndarray = None   # triangle i of tri_enc is triangle perm[i] of cf.config_scene("C2")
    note: dict = dataclasses.field(default_factory=dict)   # what a perturbation chose


# ------------------------------------------------------------------ reading a node_enc
def is_leaf(nodes, i) -> bool:
    return nodes[i, 1, 0] > 0


def walk(nodes):
    """Pre-order from node 1: [(node, depth)] (the root has depth 1)."""
    out, st = [], [(1, 1)]
    while st:
        i, d = st.pop()
        out.append((i, d))
        if not is_leaf(nodes, i):
            st.append((int(nodes[i, 0, 1]), d + 1))
            st.append((int(nodes[i, 0, 0]), d + 1))
    return out


def leaf_nodes(nodes):
    """The leaves in the reference's left-first order."""
    return [i for i, _ in walk(nodes) if is_leaf(nodes, i)]


def leaf_ranges(nodes):
    return [(int(nodes[i, 1, 1]), int(nodes[i, 1, 0])) for i in leaf_nodes(nodes)]


def depth(nodes) -> int:
    return max(d for _, d in walk(nodes))


def triangle_counts(nodes) -> np.ndarray:
    """Triangles below each node (children follow their parent in the numbering)."""
    cnt = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes) - 1, 0, -1):
        cnt[i] = nodes[i, 1, 0] if is_leaf(nodes, i) else cnt[int(nodes[i, 0, 0])] + cnt[int(nodes[i, 0, 1])]
    return cnt


def check(t: Tree) -> dict:
    """Every triangle in exactly one leaf (N4: its own exception), depth at most 64, two children per
    internal node, children numbered after their parent.  Returns the depth and the leaf sizes."""
    nodes, nt = t.node_enc, len(t.tri_enc)
    assert nodes.dtype == F and nodes.shape[1:] == (4, 3) and t.tri_enc.dtype == F and t.tri_enc.shape[1:] == (14, 3)
    seen = np.zeros(nt, np.int64)
    sizes = []
    for i, _ in walk(nodes):
        if is_leaf(nodes, i):
            first, n = int(nodes[i, 1, 1]), int(nodes[i, 1, 0])
            assert 1 <= n <= 16 and 0 <= first and first + n <= nt
            seen[first:first + n] += 1
            sizes.append(n)
        else:
            assert i < int(nodes[i, 0, 0]) < len(nodes) and i < int(nodes[i, 0, 1]) < len(nodes)
    if t.name == "N4":
        assert sorted(np.bincount(seen, minlength=3).tolist()) == [2, 2, nt - 4]
    else:
        assert (seen == 1).all()
    d = depth(nodes)
    assert d <= 64
    return {"depth": d, "sizes": np.bincount(sizes, minlength=17)}


# ------------------------------------------------------------------ the builder
def build(tri_enc, cap: int, split: str, seed: int = 0):
    """(tri_enc in leaf order, node_enc, that order) of a tree over tri_enc's triangles.
    full:     sorted by centroid on the longest axis, split at the median rounded up to a multiple
              of cap (every leaf but one holds exactly cap triangles);
    lopsided: the same order, the left side gets one eighth, rounded to a multiple of cap, at
              least cap;
    random:   a seeded axis (one time in four below 65 triangles: no order at all) and position
              (half the time a full leaf's worth when at most two leaves' worth remain), and a coin
              decides whether cap triangles or fewer are split further: leaves of 1 .. cap.
    Boxes are exact: a leaf's the min / max of its vertices, an internal node's the union of its
    children's."""
    tri = np.ascontiguousarray(tri_enc, F)
    v = tri[:, 0:3]
    cen = v.astype(np.float64).mean(axis=1)
    tlo, thi = v.min(axis=1), v.max(axis=1)
    rng = np.random.default_rng(seed)
    rows, order = [[(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]], []

    def split_of(ids):
        n = len(ids)
        if split == "random":
            if n == 1 or (n <= cap and rng.random() < 0.5):
                return None
            if n <= 64 and rng.random() < 0.25:
                ids = rng.permutation(ids)
            else:
                ids = ids[np.argsort(cen[ids, rng.integers(3)], kind="stable")]
            if cap < n <= 2 * cap and rng.random() < 0.5:
                return ids, cap
            return ids, int(rng.integers(1, n))
        if n <= cap:
            return None
        axis = int(np.argmax(thi[ids].max(axis=0) - tlo[ids].min(axis=0)))
        ids = ids[np.argsort(cen[ids, axis], kind="stable")]
        if split == "full":
            return ids, -(-n // (2 * cap)) * cap
        assert split == "lopsided"
        return ids, max(cap, int(n / 8 / cap + 0.5) * cap)

    def rec(ids):
        i = len(rows)
        rows.append(None)
        s = split_of(ids)
        if s is None:
            rows[i] = [(0, 0, 0), (len(ids), len(order), 0), tlo[ids].min(axis=0), thi[ids].max(axis=0)]
            order.extend(int(k) for k in ids)
            return i
        ids, pos = s
        assert 0 < pos < len(ids)
        l = rec(ids[:pos])
        r = rec(ids[pos:])
        rows[i] = [(l, r, 0), (0, 0, 0), np.minimum(rows[l][2], rows[r][2]), np.maximum(rows[l][3], rows[r][3])]
        return i
    rec(np.arange(len(tri)))
    return np.ascontiguousarray(tri[order]), np.array(rows, F), np.array(order, np.int64)


# ------------------------------------------------------------------ the box rules
def pad_leaves(nodes, frac):
    out = nodes.copy()
    for i in range(1, len(out)):
        if is_leaf(out, i):
            e = (out[i, 3] - out[i, 2]) * F(frac)
            out[i, 2], out[i, 3] = out[i, 2] - e, out[i, 3] + e
    return out


def loose_nested(nodes, frac):
    """Padded leaves; every internal box the union of its (padded) children, padded again."""
    out = pad_leaves(nodes, frac)
    for i in range(len(out) - 1, 0, -1):
        if not is_leaf(out, i):
            l, r = int(out[i, 0, 0]), int(out[i, 0, 1])
            lo, hi = np.minimum(out[l, 2], out[r, 2]), np.maximum(out[l, 3], out[r, 3])
            e = (hi - lo) * F(frac)
            out[i, 2], out[i, 3] = lo - e, hi + e
    return out


def halved_internal_box(nodes, tri_enc):
    """(node_enc, note): the chosen node keeps the lower half of its box along its longest axis."""
    cnt = triangle_counts(nodes)

    def cut(node):
        axis = int(np.argmax(nodes[node, 3] - nodes[node, 2]))
        plane = F(nodes[node, 2, axis] + (nodes[node, 3, axis] - nodes[node, 2, axis]) * F(0.5))
        first = min(f for f, _ in leaf_ranges_below(nodes, node))
        return {"node": node, "axis": axis, "plane": plane, "first": first, "count": int(cnt[node])}
    cand = [(d, i) for i, d in walk(nodes) if i != 1 and not is_leaf(nodes, i) and cnt[i] >= N2_MIN_TRIANGLES]
    deepest = max(d for d, _ in cand)
    # several nodes are that deep: the one whose cut-off half holds the most triangles, then the first
    notes = [cut(i) for d, i in cand if d == deepest]
    note = max(notes, key=lambda n: (len(_wholly_above(tri_enc, n)), -n["node"]))
    note["depth"] = deepest
    out = nodes.copy()
    node, axis = note["node"], note["axis"]
    assert out[node, 2, axis] < note["plane"] < out[node, 3, axis]
    out[node, 3, axis] = note["plane"]
    return out, note


def _wholly_above(tri_enc, n):
    idx = np.arange(n["first"], n["first"] + n["count"])
    return idx[(tri_enc[idx, 0:3, n["axis"]] > n["plane"]).all(axis=1)]


def leaf_ranges_below(nodes, node):
    out, st = [], [node]
    while st:
        i = st.pop()
        if is_leaf(nodes, i):
            out.append((int(nodes[i, 1, 1]), int(nodes[i, 1, 0])))
        else:
            st += [int(nodes[i, 0, 1]), int(nodes[i, 0, 0])]
    return out


def shrunk_leaf_box(nodes):
    leaves = leaf_nodes(nodes)
    leaf = leaves[len(leaves) // 2]
    out = nodes.copy()
    axis = int(np.argmax(out[leaf, 3] - out[leaf, 2]))
    assert out[leaf, 3, axis] > out[leaf, 2, axis]
    out[leaf, 3, axis] = out[leaf, 2, axis] + (out[leaf, 3, axis] - out[leaf, 2, axis]) * F(0.5)
    return out, {"leaf": leaf, "axis": axis}


def overlapping_leaf_range(nodes):
    leaves = leaf_nodes(nodes)
    leaf = leaves[len(leaves) // 2]
    out = nodes.copy()
    assert out[leaf, 1, 1] >= 2
    out[leaf, 1, 1] -= 2
    return out, {"leaf": leaf}


# ------------------------------------------------------------------ the named trees
@lru_cache(maxsize=None)
def _built(cap, split, seed=0):
    built = build(cf.config_scene("C2").tri_enc, cap, split, seed)
    for a in built:
        a.flags.writeable = False
    return built


_RULES = {"M1": (1, "full"), "M2": (3, "full"), "M3": (9, "full"), "M4": (16, "full"), "M5": (13, "lopsided"),
          "M6": (16, "random", 6)}


@lru_cache(maxsize=None)
def tree(name: str) -> Tree:
    if name in _RULES:
        tri, nodes, perm = _built(*_RULES[name])
        return Tree(name, tri, nodes, True, perm)
    if name in ("M8a", "M8b"):
        sd = cf.build_scene(cf.CONFIGS["C2"].objects, leaf_size=16 if name == "M8a" else 1)
        return Tree(name, sd.tri_enc, sd.node_enc, True)
    base = tree("M4" if name in ("M7", "N1") else "M3")
    note = {}
    if name == "M7":
        nodes = loose_nested(base.node_enc, 0.05)
    elif name == "N1":
        nodes = pad_leaves(base.node_enc, 0.25)
    elif name == "N2":
        nodes, note = halved_internal_box(base.node_enc, base.tri_enc)
    elif name == "N3":
        nodes, note = shrunk_leaf_box(base.node_enc)
    elif name == "N4":
        nodes, note = overlapping_leaf_range(base.node_enc)
    else:
        raise KeyError(name)
    nodes.flags.writeable = False
    return Tree(name, base.tri_enc, nodes, name == "M7", base.perm, note)


def cut_off_triangles(t: Tree) -> np.ndarray:
    """N2: the triangles below the halved node that lie wholly in the half it no longer covers."""
    return _wholly_above(t.tri_enc, t.note)


def aimed_rays(t: Tree, count: int = 256, seed: int = 20240611):
    """N2's own family: from a sphere of radius 6 around the mesh (outside the scene's triangles)
    at centroids of the cut-off triangles."""
    rng = np.random.default_rng(seed)
    cut = cut_off_triangles(t)
    assert cut.size >= 16
    target = t.tri_enc[cut[rng.integers(0, cut.size, count)], 0:3].astype(np.float64).mean(axis=1)
    u = rng.normal(size=(count, 3))
    o = (target.mean(axis=0) + 6.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)
    return o, normalize_f32((target - o).astype(F))


def moved_mesh(t: Tree, material, moved):
    """(tri_index, p, n) for rt_update_geometry on t: its triangles that carry `material` (24
    texels), with the vertices `moved` = (tri_index, p, n) gives the same triangles of C2
    (geometry_cases.moved)."""
    tri = t.tri_enc
    idx = np.flatnonzero((tri[:, 6:14].reshape(len(tri), 24) == np.asarray(material, F)[None]).all(axis=1))
    c2_idx, p, n = moved
    at = np.full(len(tri), -1, np.int64)
    at[c2_idx] = np.arange(len(c2_idx))
    src = at[t.perm[idx]]
    assert len(idx) == len(c2_idx) and (src >= 0).all()
    return idx.astype(np.int32), np.ascontiguousarray(p[src]), np.ascontiguousarray(n[src])
