"""CPU: the scene compiler of the HIP path (csrc/common/scene_compile.h), the code rt_set_scene
runs, called through librtscene.so (rts_compile_scene): the structure of the 4-wide tree for every
builder variant, the leaf ranks and records, the collapse's optimality, every rejection with its
code and message, the culling bound against the Python model of test_cull_bound.py, the encoded
entry against the SoA one, and golden hashes of the compiled C2 / C3 arrays."""
import hashlib
import itertools
import json
import math
from pathlib import Path

import numpy as np
import pytest

import edge_cases
import test_cull_bound as tcb
from rtamd import configs as cf
from rtamd import scene_lib as sl
from rtamd.renderer import RT_ERR_ARG, RT_ERR_LIMIT, RT_OK, marshal_scene_soa

GOLD = Path(__file__).resolve().parent / "golden"
F = np.float32
VARIANTS = [dict(rebuild=r, greedy=g, bfs=b) for r, g, b in itertools.product((True, False), repeat=3)]
ARRAYS = ("tri", "trx", "trin", "hrec", "mats", "nodes", "qnodes")


# ------------------------------------------------------------------------------ scenes
def hand_scene(leaves, tree=None):
    """A scene in rt_set_scene's form from `leaves`, a list of (n, 3, 3) float32 triangle arrays
    (one per leaf, consecutive in the triangle list), and `tree`, nested pairs of leaf numbers
    (default: balanced).  Reference numbering: node 0 dummy, root 1, pre-order; a leaf's box is the
    min/max of its vertices, an internal box the union of its children's."""
    leaves = [np.asarray(t, F).reshape(-1, 3, 3) for t in leaves]
    tris = np.concatenate(leaves)
    first = np.concatenate([[0], np.cumsum([len(t) for t in leaves])])
    if tree is None:
        def bal(lo, hi):
            return lo if hi - lo == 1 else (bal(lo, (lo + hi) // 2), bal((lo + hi) // 2, hi))
        tree = bal(0, len(leaves))
    rows = [dict(left=0, right=0, n=0, index=0, aa=np.zeros(3, F), bb=np.zeros(3, F))]

    def add(t):
        i = len(rows)
        rows.append(None)
        if isinstance(t, tuple):
            l, r = add(t[0]), add(t[1])
            rows[i] = dict(left=l, right=r, n=0, index=0, aa=np.minimum(rows[l]["aa"], rows[r]["aa"]),
                           bb=np.maximum(rows[l]["bb"], rows[r]["bb"]))
        else:
            v = leaves[t].reshape(-1, 3)
            rows[i] = dict(left=0, right=0, n=len(leaves[t]), index=int(first[t]), aa=v.min(0), bb=v.max(0))
        return i
    add(tree)
    nodes = {k: np.array([r[k] for r in rows], np.int32) for k in ("left", "right", "n", "index")}
    nodes["aa"] = np.stack([r["aa"] for r in rows]).astype(F)
    nodes["bb"] = np.stack([r["bb"] for r in rows]).astype(F)
    nrm = tcb.geometric_normal(tris[:, 0], tris[:, 1], tris[:, 2])
    mats = np.zeros((2, 24), F)
    mats[:, 3:6] = 0.5
    mats[1, 10] = 0.3   # roughness
    mats[:, 16] = 1.5   # ior
    soa = {"p1": tris[:, 0].copy(), "p2": tris[:, 1].copy(), "p3": tris[:, 2].copy(), "n1": nrm, "n2": nrm.copy(),
           "n3": nrm.copy(), "material_id": (np.arange(len(tris)) % 2).astype(np.int32), "materials": mats}
    return soa, nodes


def blob_leaves(centres, counts, seed=3):
    rng = np.random.default_rng(seed)
    return [(np.asarray(c, F)[None, None] + rng.normal(size=(n, 3, 3)) * 0.3).astype(F) for c, n in zip(centres, counts)]


def five_leaf_scene():
    """Five leaves always collapse to a root of four slots and one node of two (two empty slots):
    opening a slot never costs area, so the root fills up.  six_leaf_chain_scene has the node with
    one empty slot."""
    return hand_scene(blob_leaves([(0, 0, 0), (1.5, 0, 0), (5, 1, 0), (6, 4, 1), (12, 0, 2)], [2, 1, 3, 1, 2]),
                      ((0, 1), ((2, 3), 4)))


def six_leaf_chain_scene():
    """A left-to-right chain: the greedy collapse of the reference's own levels gives the root four
    slots and its child node three, so a node with exactly one empty slot."""
    return hand_scene(blob_leaves([(3 * i, 0.5 * i, 0) for i in range(6)], [1, 2, 1, 2, 1, 2]),
                      (0, (1, (2, (3, (4, 5))))))


def _from_encoded(tri_enc, node_enc):
    """The arrays of rt_set_scene_encoded's decode, restated (materials: all triangles' own)."""
    t = np.asarray(tri_enc, F).reshape(-1, 14, 3)
    n = np.asarray(node_enc, F).reshape(-1, 4, 3)
    soa = {k: t[:, i].copy() for i, k in enumerate(("p1", "p2", "p3", "n1", "n2", "n3"))}
    soa["material_id"] = np.arange(len(t), dtype=np.int32)
    soa["materials"] = t[:, 6:14].reshape(-1, 24).copy()
    nodes = {"left": n[:, 0, 0].astype(np.int32), "right": n[:, 0, 1].astype(np.int32), "n": n[:, 1, 0].astype(np.int32),
             "index": n[:, 1, 1].astype(np.int32), "aa": n[:, 2].copy(), "bb": n[:, 3].copy()}
    return soa, nodes


def diagonal():
    x = edge_cases.diagonal_scene()
    return _from_encoded(x["tri_enc"], x["node_enc"])


def c2():
    sd = cf.config_scene("C2")
    return sd.soa, sd.nodes


SCENES = {"C2": c2, "diagonal": diagonal, "five_leaf": five_leaf_scene, "six_leaf_chain": six_leaf_chain_scene}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def reference_leaves(nodes):
    """Left-first DFS of the caller's tree: [(leaf ref, node)] in rank order, and the internal
    nodes in pre-order (the order rt_set_scene numbers its binary nodes in)."""
    leaves, internal = [], []

    def go(i):
        if nodes["n"][i] > 0:
            leaves.append(((sl.LEAF_BIT | (int(nodes["index"][i]) << 4) | (int(nodes["n"][i]) - 1)), i))
            return
        internal.append(i)
        go(int(nodes["left"][i]))
        go(int(nodes["right"][i]))
    go(1)
    return leaves, internal


def as_ref(x):
    return int(x) & 0xffffffff


# ------------------------------------------------------------- 1. the 4-wide tree
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join(k for k, on in v.items() if on) or "none")
@pytest.mark.parametrize("scene", list(SCENES))
def test_wide_tree_structure(scene, variant):
    soa, nodes = SCENES[scene]()
    k = sl.compile_scene(soa, nodes, **variant)
    assert k.rc == RT_OK and k.scalars["wide"]
    q = k.arrays["qnodes"]
    leaves, _ = reference_leaves(nodes)
    box_of = {ref: (bits(nodes["aa"][i]), bits(nodes["bb"][i])) for ref, i in leaves}
    seen, deepest, visited = [], 0, set()
    stack = [(k.scalars["qroot"], 1, None, None)]
    assert not as_ref(k.scalars["qroot"]) & sl.LEAF_BIT
    while stack:
        i, level, plo, phi = stack.pop()
        assert 0 <= i < len(q) and i not in visited
        visited.add(i)
        deepest = max(deepest, level)
        lo, hi, ref = q[i]["lo"], q[i]["hi"], q[i]["ref"]
        filled = [int(r) != sl.Q_EMPTY for r in ref]
        assert filled == sorted(filled, reverse=True) and filled[0] and filled[1]  # empty slots come last
        for s in range(4):
            if not filled[s]:
                assert np.all(lo[:, s] == np.inf) and np.all(hi[:, s] == -np.inf)
                continue
            if plo is not None:   # monotone: inside the parent slot's box
                assert np.all(lo[:, s] >= plo) and np.all(hi[:, s] <= phi)
            r = as_ref(ref[s])
            if r & sl.LEAF_BIT:
                seen.append(r)
                assert np.array_equal(bits(lo[:, s]), box_of[r][0]) and np.array_equal(bits(hi[:, s]), box_of[r][1])
            else:
                assert r < len(q)
                if variant["bfs"]:
                    assert r > i
                stack.append((r, level + 1, lo[:, s].copy(), hi[:, s].copy()))
    assert sorted(seen) == sorted(ref for ref, _ in leaves) and len(set(seen)) == len(seen)
    assert len(visited) == len(q)
    if variant["bfs"]:
        assert k.scalars["qroot"] == 0
    assert k.scalars["qdepth"] == deepest
    if scene == "diagonal":
        assert [int(r) != sl.Q_EMPTY for r in q[0]["ref"]] == [True, True, False, False]
    if scene == "six_leaf_chain" and variant["greedy"] and not variant["rebuild"]:
        assert sorted(sum(int(r) == sl.Q_EMPTY for r in n["ref"]) for n in q) == [0, 1]


# ------------------------------------------------------------- 2. leaf ranks and records
@pytest.mark.parametrize("scene", ["C2", "five_leaf"])
def test_leaf_ranks_and_records(scene):
    soa, nodes = SCENES[scene]()
    k = sl.compile_scene(soa, nodes)
    tri, trin, hrec, bn = (k.arrays[a] for a in ("tri", "trin", "hrec", "nodes"))
    nt = len(soa["material_id"])
    leaves, internal = reference_leaves(nodes)
    rank_of_node = {i: r for r, (_, i) in enumerate(leaves)}
    tri_rank = np.full(nt, -1, np.int64)
    for r, (_, i) in enumerate(leaves):
        tri_rank[nodes["index"][i]:nodes["index"][i] + nodes["n"][i]] = r
    assert np.array_equal(bits(trin[1::3, 3]).astype(np.int64), tri_rank)

    def first_leaf(i):
        while nodes["n"][i] <= 0:
            i = int(nodes["left"][i])
        return i
    assert len(bn) == len(internal)
    for kk, i in enumerate(internal):
        assert bn[kk]["ref"][2] == rank_of_node[first_leaf(int(nodes["right"][i]))]
        assert np.array_equal(bits(bn[kk]["box"]), bits(np.concatenate(
            [nodes["aa"][nodes["left"][i]], nodes["bb"][nodes["left"][i]],
             nodes["aa"][nodes["right"][i]], nodes["bb"][nodes["right"][i]]])))
    assert np.array_equal(bits(trin[0::3, 3]).view(np.int32), soa["material_id"])
    assert np.all(bits(trin[2::3, 3]) == 0)
    h = hrec.reshape(nt, 8, 4)
    assert np.array_equal(bits(h[:, 0:3]), bits(tri.reshape(nt, 3, 4)))
    assert np.array_equal(bits(h[:, 3:6]), bits(trin.reshape(nt, 3, 4)))
    assert np.all(bits(h[:, 6:8]) == 0)
    ng = tcb.geometric_normal(soa["p1"], soa["p2"], soa["p3"])
    assert np.array_equal(tri.reshape(nt, 3, 4)[:, :, 3], ng, equal_nan=True)
    for c, key in enumerate(("p1", "p2", "p3")):
        assert np.array_equal(bits(tri[c::3, :3]), bits(soa[key]))
        assert np.array_equal(bits(trin[c::3, :3]), bits(soa["n" + key[1]]))


# ------------------------------------------------------------- 3. collapse optimality
def wide_area(q):
    """Summed surface area of the 4-wide nodes (each the union of its filled slots), float64."""
    total = []
    for n in q:
        f = n["ref"] != sl.Q_EMPTY
        e = n["hi"][:, f].astype(np.float64).max(1) - n["lo"][:, f].astype(np.float64).min(1)
        total.append(e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    return math.fsum(total)


@pytest.mark.parametrize("rebuild", [True, False])
@pytest.mark.parametrize("scene", ["C2", "five_leaf"])
def test_optimal_collapse_is_no_worse_than_greedy(scene, rebuild):
    soa, nodes = SCENES[scene]()
    best = wide_area(sl.compile_scene(soa, nodes, rebuild=rebuild, greedy=False).arrays["qnodes"])
    greedy = wide_area(sl.compile_scene(soa, nodes, rebuild=rebuild, greedy=True).arrays["qnodes"])
    print(f"{scene} rebuild={rebuild}: optimal {best:.6g} greedy {greedy:.6g}")
    assert best <= greedy


# ------------------------------------------------------------- 4. every rejection
def three_leaf_scene():
    return hand_scene(blob_leaves([(0, 0, 0), (3, 0, 0), (6, 1, 0)], [2, 2, 2]), ((0, 1), 2))


def chain_scene(levels):
    """A left chain `levels` deep: internal node i has the next internal node on the left and a
    one-triangle leaf on the right; the last level is a leaf."""
    n_leaves = levels
    tree = n_leaves - 1
    for leaf in range(n_leaves - 2, -1, -1):
        tree = (tree, leaf)
    return hand_scene(blob_leaves([(i, 0, 0) for i in range(n_leaves)], [1] * n_leaves), tree)


def _untouched(k):
    assert all(len(a) == 0 for a in k.arrays.values())
    assert k.scalars == dict(cull_R=0.0, cull_K=0.0, cull_off=0.0, tri_k1=0.0, tri_k0=0.0, n_tri=0, n_mats=0, root=0,
                             has_scene=0, depth=1, qroot=0, qdepth=1, tri_flagged=0, wide=False)


def _patched(what):
    soa, nodes = three_leaf_scene()
    nodes = {k: v.copy() for k, v in nodes.items()}
    what(soa, nodes)
    return sl.compile_scene(soa, nodes)


REJECTIONS = {
    "missing triangle arrays": (RT_ERR_ARG, lambda s, n: s.update(p2=None)),
    "missing node arrays": (RT_ERR_ARG, lambda s, n: n.update(aa=None)),
    "material_id out of range": (RT_ERR_ARG, lambda s, n: s["material_id"].__setitem__(3, 2)),
    "leaf with more than 16 triangles": (RT_ERR_LIMIT, lambda s, n: n["n"].__setitem__(3, 17)),
    "leaf range outside the triangle list": (RT_ERR_ARG, lambda s, n: n["index"].__setitem__(5, 5)),
    "child index out of range": (RT_ERR_ARG, lambda s, n: n["right"].__setitem__(2, 6)),
    "BVH is not a tree": (RT_ERR_ARG, lambda s, n: n["right"].__setitem__(1, 2)),
    "internal node without two children": (RT_ERR_ARG, lambda s, n: n["left"].__setitem__(2, 0)),
}


@pytest.mark.parametrize("message", list(REJECTIONS))
def test_rejections(message):
    code, what = REJECTIONS[message]
    k = _patched(what)
    assert (k.rc, k.err) == (code, message)
    _untouched(k)


def test_rejects_a_negative_count():
    for field in ("n_triangles", "n_nodes", "n_materials"):
        s, keep = marshal_scene_soa(*three_leaf_scene())
        setattr(s, field, -1)
        k = sl.compile_scene(s)
        assert (k.rc, k.err) == (RT_ERR_ARG, "negative count")
        _untouched(k)


def test_rejects_a_tree_deeper_than_64_levels():
    k = sl.compile_scene(*chain_scene(65))
    assert (k.rc, k.err) == (RT_ERR_LIMIT, "BVH deeper than 64 levels")
    _untouched(k)
    k = sl.compile_scene(*chain_scene(64))
    assert k.rc == RT_OK and k.scalars["depth"] == 64 and k.scalars["wide"]


def test_unrejected_scene_is_accepted():
    k = _patched(lambda s, n: None)
    assert k.rc == RT_OK and k.err == "" and k.scalars["wide"] and k.scalars["has_scene"] == 1


def test_triangle_in_two_leaves_keeps_the_binary_traversal():
    k = _patched(lambda s, n: n["index"].__setitem__(5, 3))   # the third leaf lists the second's triangles
    assert k.rc == RT_OK and k.scalars["has_scene"] == 1 and not k.scalars["wide"]
    assert len(k.arrays["qnodes"]) == 1 and k.arrays["qnodes"].tobytes() == bytes(128)
    assert len(k.arrays["nodes"]) == 2


def test_empty_scene_padding():
    e = {key: np.zeros((0, 3), F) for key in ("p1", "p2", "p3", "n1", "n2", "n3")}
    e.update(material_id=np.zeros(0, np.int32), materials=np.zeros((0, 24), F))
    nodes = {key: np.zeros(0, np.int32) for key in ("left", "right", "n", "index")}
    nodes.update(aa=np.zeros((0, 3), F), bb=np.zeros((0, 3), F))
    k = sl.compile_scene(e, nodes)
    assert k.rc == RT_OK and k.scalars["has_scene"] == 0 and not k.scalars["wide"]
    assert {a: len(v) for a, v in k.arrays.items()} == dict(tri=0, trx=3, trin=0, hrec=8, mats=1, nodes=1, qnodes=1,
                                                            tri_mat=0)
    assert all(not np.asarray(v).tobytes().strip(b"\0") for v in k.arrays.values())


# ------------------------------------------------------------- 5. the culling bound
def _cull_model(soa):
    p1, p2, p3 = (np.asarray(soa[key], F) for key in ("p1", "p2", "p3"))
    N = tcb.geometric_normal(p1, p2, p3)
    fin = np.isfinite(N).all(1)      # cull_bound_stats skips triangles the reference can never hit
    with np.errstate(invalid="ignore"):   # R = 0: the bound is `off` alone (inf * 0 where K = inf, unused)
        off, K = tcb.per_triangle_bound(p1[fin], p2[fin], p3[fin], N[fin], 0.0)
    well = np.isfinite(K)
    return float(np.abs(np.stack([p1, p2, p3])).max()), float(K.max()), float(off[well].max(initial=0.0))


def _cull_scene(name):
    if name in cf.CONFIGS:
        sd = cf.config_scene(name)
        return sd.soa, sd.nodes
    rng = np.random.default_rng(11)
    p1, p2, p3, _, _ = tcb.make_case(rng, 2000, name)
    tris = np.stack([p1, p2, p3], 1)
    return hand_scene([tris[i:i + 16] for i in range(0, 2000, 16)])


@pytest.mark.parametrize("name", ["C2", "C3", "C5", "edge", "vertex", "grazing", "axis", "sliver", "skim"])
def test_cull_bound_stats_against_the_model(name):
    soa, nodes = _cull_scene(name)
    k = sl.compile_scene(soa, nodes)
    assert k.rc == RT_OK
    R, K, off = _cull_model(soa)
    print(f"{name}: R {k.scalars['cull_R']!r} K {k.scalars['cull_K']!r} (model {K!r}) "
          f"off {k.scalars['cull_off']!r} (model {off!r})")
    assert k.scalars["cull_R"] == R
    assert k.scalars["cull_K"] == pytest.approx(K, rel=1e-9, abs=0.0)
    assert k.scalars["cull_off"] == pytest.approx(off, rel=1e-9, abs=0.0)
    if name in cf.CONFIGS:
        assert np.isfinite(K)


def test_vertex_outside_its_leaf_box_switches_culling_off():
    soa, nodes = three_leaf_scene()
    assert np.isfinite(sl.compile_scene(soa, nodes).scalars["cull_K"])
    soa["p2"][3, 1] = np.nextafter(nodes["bb"][4, 1], F(np.inf))   # triangle 3 lies in the leaf of node 4
    assert nodes["index"][4] <= 3 < nodes["index"][4] + nodes["n"][4]
    assert sl.compile_scene(soa, nodes).scalars["cull_K"] == np.inf


# ------------------------------------------------------------- 6. encoded against SoA
def test_encoded_entry_matches_soa_entry():
    sd = cf.config_scene("C2")
    a = sl.compile_scene(sd.soa, sd.nodes)
    b = sl.compile_scene_encoded(sd.tri_enc, sd.node_enc)
    assert a.rc == b.rc == RT_OK
    for name in ("tri", "trx", "nodes", "qnodes"):
        assert a.arrays[name].tobytes() == b.arrays[name].tobytes(), name
    nt = a.scalars["n_tri"]
    ta, tb = (bits(x.arrays["trin"]).reshape(nt, 3, 4).copy() for x in (a, b))
    ha, hb = (bits(x.arrays["hrec"]).reshape(nt, 8, 4).copy() for x in (a, b))
    for t, h in ((ta, ha), (tb, hb)):
        assert np.array_equal(h[:, 3:6], t)
        t[:, 0, 3] = 0   # the material id
        h[:, 3, 3] = 0
    assert np.array_equal(ta, tb) and np.array_equal(ha, hb)
    for x in (a, b):
        assert np.array_equal(bits(x.arrays["trin"])[0::3, 3].view(np.int32), x.arrays["tri_mat"])
    assert np.array_equal(bits(a.arrays["mats"][a.arrays["tri_mat"]]), bits(b.arrays["mats"][b.arrays["tri_mat"]]))
    sa, sb = dict(a.scalars), dict(b.scalars)
    sa.pop("n_mats"), sb.pop("n_mats")
    assert sa == sb


# ------------------------------------------------------------- 7. golden hashes
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_compiled_scene_regression(cfg):
    g = json.loads((GOLD / "compiled_scene_hashes.json").read_text())[cfg]
    sd = cf.config_scene(cfg)
    k = sl.compile_scene(sd.soa, sd.nodes)
    assert set(g) == set(ARRAYS)
    for name in ARRAYS:
        assert hashlib.sha256(k.arrays[name].tobytes()).hexdigest() == g[name], name
