"""CPU: the scene compiler on trees the reference's builder never makes (tests/tree_cases.py).

A leaf-set model restates the oracle's hitAABB (RT:303-316, with the oracle's min / max: of a NaN
and a number, the number) and the `d > 0` descent of hitBVH (RT:338-392) in numpy fp32, and walks
(a) the caller's nodes, (b) the compiled binary nodes, (c) the compiled 4-wide nodes.  For a tree
whose boxes nest the three reach the same leaves for every ray, whatever the internal levels of
(c); a tree whose boxes do not nest must stay on (b) with the caller's boxes and without culling.
The oracle itself is checked against its own answers over C2's tree: the trees hold the same
triangles, so every ray's t is the same.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import geometry_cases as gc
import oracle as orc
import query_cases as qc
import tree_cases as tc
from cull_cases import normalize_f32
from rtamd import configs as cf
from rtamd import scene_lib as sl
from rtamd.renderer import RT_OK

F = np.float32
VARIANTS = {"default": {}, "reflevels": dict(rebuild=False), "greedy": dict(greedy=True), "dfs": dict(bfs=False),
            "binary": dict(wide=False)}


# ------------------------------------------------------------------ the leaf-set model
def hit_aabb(o, inv, aa, bb):
    """hitAABB(...) > 0 for rays (o, 1 / d), (R, 3) fp32, against one box."""
    with np.errstate(invalid="ignore"):
        f, n = (bb - o) * inv, (aa - o) * inv
    tmax, tmin = np.fmax(f, n), np.fmin(f, n)
    t1 = np.fmin(tmax[:, 0], np.fmin(tmax[:, 1], tmax[:, 2]))
    t0 = np.fmax(tmin[:, 0], np.fmax(tmin[:, 1], tmin[:, 2]))
    with np.errstate(invalid="ignore"):
        d = np.where(t1 >= t0, np.where(t0 > 0, t0, t1), F(-1.0))
        return d > 0


def _reached(root, children, o, d):
    """{leaf ref: packed mask of the rays that reach it}; children(ref) -> [(ref, aa, bb)]."""
    with np.errstate(divide="ignore"):
        inv = F(1.0) / d
    out, st = {}, [(root, np.ones(len(o), bool))]
    while st:
        ref, m = st.pop()
        if ref & sl.LEAF_BIT:
            out[ref] = out.get(ref, False) | m
            continue
        for r, aa, bb in children(ref):
            mm = m & hit_aabb(o, inv, aa, bb)
            if mm.any():
                st.append((r, mm))
    return {r: np.packbits(m).tobytes() for r, m in out.items()}


def walk_caller(nodes, o, d):
    def ref_of(i):
        return (sl.LEAF_BIT | (int(nodes[i, 1, 1]) << 4) | (int(nodes[i, 1, 0]) - 1)) if tc.is_leaf(nodes, i) else i
    back = {}

    def children(ref):
        i = back.get(ref, ref)
        kids = []
        for c in (int(nodes[i, 0, 0]), int(nodes[i, 0, 1])):
            back[ref_of(c)] = c
            kids.append((ref_of(c), nodes[c, 2], nodes[c, 3]))
        return kids
    return _reached(ref_of(1), children, o, d)


def walk_binary(k, o, d):
    bn = k.arrays["nodes"]
    return _reached(k.scalars["root"] & 0xffffffff,
                    lambda i: [(int(bn[i]["ref"][s]) & 0xffffffff, bn[i]["box"][6 * s:6 * s + 3], bn[i]["box"][6 * s + 3:6 * s + 6])
                               for s in (0, 1)], o, d)


def walk_wide(k, o, d):
    q = k.arrays["qnodes"]
    return _reached(k.scalars["qroot"] & 0xffffffff,
                    lambda i: [(int(q[i]["ref"][s]) & 0xffffffff, q[i]["lo"][:, s], q[i]["hi"][:, s])
                               for s in range(4) if int(q[i]["ref"][s]) != sl.Q_EMPTY], o, d)


# ------------------------------------------------------------------ rays
@pytest.fixture(scope="module")
def c2(env_maps):
    sd = cf.config_scene("C2")
    sc = orc.OracleScene(sd.tri_enc, sd.node_enc, *env_maps)
    o, d = qc.c2_rays(sd, sc, cf.MATERIALS["jade"].texels())
    ref = qc.oracle_hits(sc, o, d)
    for a in (o, d, ref):
        a.flags.writeable = False
    return SimpleNamespace(sd=sd, sc=sc, o=o, d=d, ref=ref, env=env_maps)


def model_rays(c2, nodes):
    """600 of c2_rays (303 spread over the first three families, the 297 with zero components) and
    100 rays with a zero direction component whose origin lies exactly on a plane of a leaf box of
    that axis (lower and upper planes, +0 and -0)."""
    pick = np.concatenate([np.linspace(0, 3799, 303).astype(int), np.arange(3800, 4097)])
    rng = np.random.default_rng(77)
    leaves = tc.leaf_nodes(nodes)
    o, d = np.zeros((100, 3), F), np.zeros((100, 3), F)
    for k in range(100):
        leaf, a = leaves[rng.integers(len(leaves))], k % 3
        aa, bb = nodes[leaf, 2], nodes[leaf, 3]
        v = rng.normal(size=3)
        v[a] = 0.0
        dk = normalize_f32((v / np.linalg.norm(v)).astype(F)[None])[0]
        dk[a] = F(-0.0) if (k // 6) % 2 else F(0.0)
        p = (aa + (bb - aa) * rng.uniform(0.1, 0.9, 3).astype(F)).astype(F)
        ok = (p - dk * F(5.0)).astype(F)
        ok[a] = aa[a] if (k // 3) % 2 else bb[a]
        o[k], d[k] = ok, dk
    assert ((d == 0).sum(axis=1) == 1).all()
    return np.concatenate([c2.o[pick], o]), np.concatenate([c2.d[pick], d])


def compiled(t, **variant):
    k = sl.compile_scene_encoded(t.tri_enc, t.node_enc, **variant)
    assert k.rc == RT_OK and k.err == ""
    return k


# ------------------------------------------------------------------ 1. the trees themselves
@pytest.mark.parametrize("name", tc.ALL)
def test_tree_self_check(name):
    t = tc.tree(name)
    c = tc.check(t)
    sizes = c["sizes"]
    print(f"{name}: {len(t.node_enc) - 1} nodes, depth {c['depth']}, leaf sizes {dict((n, int(k)) for n, k in enumerate(sizes) if k)}")
    assert len(t.tri_enc) == len(cf.config_scene("C2").tri_enc)
    if name in ("M4", "M7", "N1"):
        assert sizes[16] > 0 and sizes[16] >= sizes.sum() - 1
    if name == "M5":
        assert sizes[13] > 0 and 33 <= c["depth"]
    if name == "M6":
        assert sizes[1] > 0 and sizes[16] > 0 and (sizes[1:17] > 0).all()
    if name in ("M3", "N2", "N3", "N4"):
        assert sizes[9] >= sizes.sum() - 1
    if name == "M8a":
        assert sizes[16] > 0
    if name in ("M1", "M8b"):
        assert sizes[1] == sizes.sum()
    if t.perm is not None:   # the same triangles as C2, in another order
        assert np.array_equal(np.sort(t.perm), np.arange(len(t.perm)))
        assert t.tri_enc.tobytes() == cf.config_scene("C2").tri_enc[t.perm].tobytes()


def _nests(nodes):
    """The rule of scn::compile: every child's box inside its parent's, the root exempt."""
    for i, _ in tc.walk(nodes):
        if i == 1 or tc.is_leaf(nodes, i):
            continue
        for c in (int(nodes[i, 0, 0]), int(nodes[i, 0, 1])):
            if not ((nodes[c, 2] >= nodes[i, 2]).all() and (nodes[c, 3] <= nodes[i, 3]).all()):
                return False
    return True


@pytest.mark.parametrize("name", tc.ALL)
def test_nesting_is_what_the_case_says(name):
    t = tc.tree(name)
    assert _nests(t.node_enc) == (name not in ("N1", "N2"))
    assert t.nested == (name in tc.NESTED)
    if name == "M7":   # loose: no leaf box with an extent is its triangles' min / max
        exact = tc.tree("M4").node_enc
        grown = (t.node_enc[:, 2] < exact[:, 2]) | (t.node_enc[:, 3] > exact[:, 3])
        assert grown[1:].any(axis=1).all()


# ------------------------------------------------------------------ 2. reached leaves, nested trees
@pytest.mark.parametrize("name", tc.NESTED)
def test_all_three_trees_reach_the_same_leaves(c2, name):
    t = tc.tree(name)
    o, d = model_rays(c2, t.node_enc)
    assert len(o) >= 700
    want = walk_caller(t.node_enc, o, d)
    assert len(want) > 0.25 * len(tc.leaf_nodes(t.node_enc))   # the rays do get around
    for vname, variant in VARIANTS.items():
        k = compiled(t, **variant)
        assert k.scalars["wide"] == (vname != "binary") and np.isfinite(k.scalars["cull_K"])
        assert walk_binary(k, o, d) == want, f"{name} {vname}: binary nodes"
        assert walk_wide(k, o, d) == want, f"{name} {vname}: 4-wide nodes"


# ------------------------------------------------------------------ 3. trees that do not nest
def _caller_boxes(nodes):
    """The binary nodes' boxes as scn::compile forms them: internal nodes in pre-order, each the
    left child's AA, BB then the right one's."""
    internal = [i for i, _ in tc.walk(nodes) if not tc.is_leaf(nodes, i)]
    return np.stack([np.concatenate([nodes[int(nodes[i, 0, 0]), 2], nodes[int(nodes[i, 0, 0]), 3],
                                     nodes[int(nodes[i, 0, 1]), 2], nodes[int(nodes[i, 0, 1]), 3]]) for i in internal])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["N1", "N2"])
def test_boxes_that_do_not_nest_fall_back_to_the_binary_tree(name, variant):
    t = tc.tree(name)
    k = compiled(t, **VARIANTS[variant])
    assert k.scalars["has_scene"] == 1
    assert not k.scalars["wide"]
    assert k.scalars["cull_K"] == np.inf
    assert len(k.arrays["qnodes"]) == 1 and k.arrays["qnodes"].tobytes() == bytes(128)
    assert k.scalars["qdepth"] == 1
    assert k.arrays["nodes"]["box"].tobytes() == _caller_boxes(t.node_enc).tobytes()


@pytest.mark.parametrize("name", ["N1", "N2"])
def test_geometry_update_of_a_fallen_back_scene(name):
    """scn::update_geometry and the device's refit schedule on a scene without a 4-wide tree: the
    binary tree is refitted (its boxes then nest; the scene stays on it), the 4-wide record stays
    zero, no 4-wide node is scheduled."""
    t = tc.tree(name)
    m = sl.CompiledHandle(t.tri_enc, t.node_enc)
    plan = m.refit_plan()
    assert len(plan["qlist"]) == 0 and plan["qoff"].tolist() == [0] and (plan["leaves"][:, 2] == -1).all()
    assert len(plan["leaves"]) == len(tc.leaf_nodes(t.node_enc)) and len(plan["blist"]) == len(m.snapshot().arrays["nodes"])
    idx, p, n = tc.moved_mesh(t, cf.MATERIALS["jade"].texels(), gc.moved("MOVE"))
    assert m.update_geometry(idx, p, n) == 0
    s = m.snapshot()
    assert not s.scalars["wide"] and s.scalars["cull_K"] == np.inf and s.arrays["qnodes"].tobytes() == bytes(128)
    tri = t.tri_enc.copy()
    tri[idx, 0:3], tri[idx, 3:6] = p, n
    fresh = sl.compile_scene_encoded(tri, gc.refit_node_enc(tri, t.node_enc))
    gc.assert_arrays_equal(s.arrays, fresh.arrays, names=("tri", "trx", "trin", "hrec", "nodes"), what=name)


@pytest.mark.parametrize("name", tc.NOT_NESTED)
def test_binary_nodes_reach_the_callers_leaves(c2, name):
    t = tc.tree(name)
    o, d = model_rays(c2, t.node_enc)
    if name == "N2":
        ao, ad = tc.aimed_rays(t)
        o, d = np.concatenate([o, ao]), np.concatenate([d, ad])
    want = walk_caller(t.node_enc, o, d)
    for vname, variant in VARIANTS.items():
        assert walk_binary(compiled(t, **variant), o, d) == want, f"{name} {vname}"


def test_a_shrunk_leaf_box_keeps_the_wide_tree_without_culling(c2):
    """N3: the boxes still nest, so the 4-wide tree stays and reaches the caller's leaves; a
    triangle outside its leaf box switches the culling off (cull_bound_stats)."""
    t = tc.tree("N3")
    k = compiled(t)
    assert k.scalars["wide"] and k.scalars["cull_K"] == np.inf
    o, d = model_rays(c2, t.node_enc)
    assert walk_wide(k, o, d) == walk_caller(t.node_enc, o, d)


def test_a_triangle_in_two_leaves_keeps_the_binary_tree():
    k = compiled(tc.tree("N4"))
    assert not k.scalars["wide"] and k.scalars["cull_K"] == np.inf
    assert len(k.arrays["qnodes"]) == 1 and k.arrays["qnodes"].tobytes() == bytes(128)


def test_loose_boxes_that_nest_keep_the_wide_tree():
    k, exact = compiled(tc.tree("M7")), compiled(tc.tree("M4"))
    assert k.scalars["wide"] and np.isfinite(k.scalars["cull_K"])
    assert k.scalars["cull_K"] == exact.scalars["cull_K"] and len(k.arrays["qnodes"]) > 1


def test_the_halved_box_changes_what_the_reference_computes(c2):
    """N2 has teeth: of the 256 rays aimed at triangles in the cut-off half, at least 8 get another
    answer from the oracle than on M3 (the same triangles under exact boxes)."""
    n2, m3 = tc.tree("N2"), tc.tree("M3")
    assert n2.note["count"] >= tc.N2_MIN_TRIANGLES and n2.note["node"] != 1
    o, d = tc.aimed_rays(n2)
    assert len(o) == 256
    a = qc.oracle_hits(orc.OracleScene(n2.tri_enc, n2.node_enc, *c2.env), o, d)
    b = qc.oracle_hits(orc.OracleScene(m3.tri_enc, m3.node_enc, *c2.env), o, d)
    differ = int((a["t"].view(np.uint32) != b["t"].view(np.uint32)).sum())
    print(f"N2: node {n2.note['node']} ({n2.note['count']} triangles, {len(tc.cut_off_triangles(n2))} cut off), "
          f"{differ} of 256 aimed rays differ from M3")
    assert differ >= 8


# ------------------------------------------------------------------ 4. the oracle on the nested trees
@pytest.mark.parametrize("name", tc.NESTED)
def test_oracle_finds_the_same_distances_on_every_nested_tree(c2, name):
    t = tc.tree(name)
    got = qc.oracle_hits(orc.OracleScene(t.tri_enc, t.node_enc, *c2.env), c2.o, c2.d)
    assert np.array_equal(got["triangle"] >= 0, c2.ref["triangle"] >= 0)
    assert np.array_equal(got["t"].view(np.uint32), c2.ref["t"].view(np.uint32))


# ------------------------------------------------------------------ 5. the configurations are untouched
@pytest.mark.parametrize("cfg", ["C2", "C3", "C4", "C5"])
def test_configurations_keep_the_wide_tree_and_their_culling(cfg):
    sd = cf.config_scene(cfg)
    assert _nests(sd.node_enc)
    k = sl.compile_scene(sd.soa, sd.nodes)
    assert k.rc == RT_OK and k.scalars["wide"] and np.isfinite(k.scalars["cull_K"]) and len(k.arrays["qnodes"]) > 1
