"""The geometry update's definition, scn::update_geometry (csrc/common/scene_compile.h), on the CPU:
against scn::compile itself (an identity update; a fresh compile of the moved scene with boxes
refitted in numpy), its validation, and the device's refit schedule (scn::refit_plan)."""
import numpy as np
import pytest

import geometry_cases as gc
from rtamd import scene_lib as sl

F = np.float32
RT_ERR_ARG = -1


@pytest.fixture(scope="module")
def compiled():
    return gc.model().snapshot()


def rows_zero(trx):
    return (trx.reshape(-1, 12)[:, [4, 5, 6, 8, 9, 10]] == 0).all(axis=1)


def leaf_boxes(tri):
    """{leaf ref: (lo, hi)} helper: the box of triangles [first, first + n) of a (n, 4) tri array."""
    def box(ref):
        first, n = (ref & 0x7fffffff) >> 4, (ref & 15) + 1
        lo, hi = np.full(3, 1145141919.0, F), np.full(3, -1145141919.0, F)
        for t in range(first, first + n):
            p = tri[3 * t:3 * t + 3, 0:3]
            lo = gc.gmin(lo, gc.gmin(p[0], gc.gmin(p[1], p[2])))
            hi = gc.gmax(hi, gc.gmax(p[0], gc.gmax(p[1], p[2])))
        return lo, hi
    return box


def check_wide_boxes(arrays, qroot):
    """Every WNode slot box = the numpy union of the leaf boxes below it (slot order, glm min / max)."""
    q, box = arrays["qnodes"], leaf_boxes(arrays["tri"])
    n_slots = 0

    def node(i):
        nonlocal n_slots
        lo = hi = None
        for k in range(4):
            r = int(q[i]["ref"][k])
            if r == sl.Q_EMPTY:
                assert np.all(q[i]["lo"][:, k] == np.inf) and np.all(q[i]["hi"][:, k] == -np.inf)
                continue
            l, h = box(r & 0xffffffff) if r < 0 else node(r)
            assert q[i]["lo"][:, k].tobytes() == l.tobytes() and q[i]["hi"][:, k].tobytes() == h.tobytes(), (i, k)
            n_slots += 1
            lo, hi = (l, h) if lo is None else (gc.gmin(lo, l), gc.gmax(hi, h))
        return lo, hi
    node(qroot)
    return n_slots


def test_identity_update_reproduces_the_compile(compiled):
    sd = gc.c2()
    m = gc.model()
    p, n = gc.original(np.arange(sd.counts["n_triangles"]))
    assert m.update_geometry(None, p, n) == 0
    s = m.snapshot()
    gc.assert_arrays_equal(s.arrays, compiled.arrays, what="identity, all triangles")
    assert gc.bounds_of(s) == gc.bounds_of(compiled)
    idx = gc.moved()[0]
    assert m.update_geometry(idx, *gc.original(idx)) == 0
    s = m.snapshot()
    gc.assert_arrays_equal(s.arrays, compiled.arrays, what="identity, the bunny's index list")
    assert gc.bounds_of(s) == gc.bounds_of(compiled)


@pytest.mark.parametrize("options", [{}, {"rebuild": False}, {"wide": False}, {"greedy": True, "bfs": False}])
def test_identity_update_for_every_tree_variant(options):
    sd = gc.c2()
    m = gc.model(**options)
    before = m.snapshot()
    assert m.update_geometry(None, *gc.original(np.arange(sd.counts["n_triangles"]))) == 0
    gc.assert_arrays_equal(m.snapshot().arrays, before.arrays, what=str(options))


def test_moved_bunny_equals_a_fresh_compile_of_the_refitted_scene(compiled):
    idx, p, n = gc.moved("MOVE")
    m = gc.model()
    assert m.update_geometry(idx, p, n) == 0
    s = m.snapshot()
    fresh = sl.compile_scene_encoded(*gc.moved_c2("MOVE"))
    assert fresh.rc == 0
    gc.assert_arrays_equal(s.arrays, fresh.arrays, names=("nodes", "tri", "trin", "hrec"), what="moved bunny")
    both = rows_zero(s.arrays["trx"]) | rows_zero(fresh.arrays["trx"])
    a, b = s.arrays["trx"].reshape(-1, 12)[~both], fresh.arrays["trx"].reshape(-1, 12)[~both]
    assert a.tobytes() == b.tobytes() and len(a) > 4900
    assert check_wide_boxes(s.arrays, s.scalars["qroot"]) == len(s.arrays["qnodes"]) - 1 + 870
    for k in ("cull_R", "cull_K", "cull_off"):
        assert s.scalars[k] >= fresh.scalars[k]
    # the margins only grow, whatever the fresh compile's caps give
    assert s.scalars["tri_k1"] >= compiled.scalars["tri_k1"] and s.scalars["tri_k0"] >= compiled.scalars["tri_k0"]
    # the filter is exercised, not bypassed: at most 5% of the updated triangles without rows
    flagged = int(rows_zero(s.arrays["trx"])[idx].sum())   # measured: 4 of 4968
    assert flagged <= 0.05 * len(idx)
    assert s.scalars["tri_flagged"] == int(rows_zero(s.arrays["trx"]).sum())


def test_stretched_bunny_takes_the_flagged_path(compiled):
    idx, p, n = gc.moved("STRETCH")
    m = gc.model()
    st0 = m.filter_state()
    assert m.update_geometry(idx, p, n) == 0
    s, st = m.snapshot(), m.filter_state()
    fresh = sl.compile_scene_encoded(*gc.moved_c2("STRETCH"))
    gc.assert_arrays_equal(s.arrays, fresh.arrays, names=("nodes", "tri", "trin", "hrec"), what="stretched bunny")
    zero = rows_zero(s.arrays["trx"])
    assert int(zero[idx].sum()) > len(idx) // 2              # measured: 3008 of 4968
    assert s.scalars["tri_flagged"] == int(zero.sum())
    # the caps are the compile's; the extrema stay below them and never shrink
    assert (st["s_cap"], st["sc_cap"]) == (st0["s_cap"], st0["sc_cap"])
    assert st0["s_max"] <= st["s_max"] <= st["s_cap"] and st0["sc_max"] <= st["sc_max"] <= st["sc_cap"]
    assert st["c_min"] <= st0["c_min"]
    both = zero | rows_zero(fresh.arrays["trx"])             # rows do not depend on the caps
    assert s.arrays["trx"].reshape(-1, 12)[~both].tobytes() == fresh.arrays["trx"].reshape(-1, 12)[~both].tobytes()
    check_wide_boxes(s.arrays, s.scalars["qroot"])
    # and back: the arrays are the compile's again, the bounds have not shrunk
    assert m.update_geometry(idx, *gc.original(idx)) == 0
    back = m.snapshot()
    gc.assert_arrays_equal(back.arrays, compiled.arrays, what="there and back")
    assert back.scalars["tri_flagged"] == compiled.scalars["tri_flagged"]
    for k in gc.BOUNDS:
        assert back.scalars[k] == s.scalars[k] >= compiled.scalars[k]


def test_degenerate_triangles_match_the_compile():
    sd = gc.c2()
    idx = gc.moved()[0][:64].copy()
    p, n = gc.original(idx)
    p[0:8, 1] = p[0:8, 0]                                   # zero area: two vertices coincide
    p[8:16, 2] = p[8:16, 1] = p[8:16, 0]                    # a point
    p[16:32, 2] = p[16:32, 0] + (p[16:32, 1] - p[16:32, 0]) * F(0.5) + F(1e-6)   # slivers
    p[32:40, 2] = p[32:40, 0] + (p[32:40, 1] - p[32:40, 0]) * F(2.0)             # collinear
    m = gc.model()
    assert m.update_geometry(idx, p, n) == 0
    s = m.snapshot()
    fresh = sl.compile_scene_encoded(*gc.moved_scene(idx, p, n))
    assert fresh.rc == 0
    gc.assert_arrays_equal(s.arrays, fresh.arrays, names=("nodes", "tri", "trin", "hrec"), what="degenerate")
    assert np.isnan(s.arrays["tri"].reshape(-1, 12)[idx[8:16], 3]).all()   # normalize(0): NaN normals, as compiled
    assert rows_zero(s.arrays["trx"])[idx[0:16]].all()
    both = rows_zero(s.arrays["trx"]) | rows_zero(fresh.arrays["trx"])
    assert s.arrays["trx"].reshape(-1, 12)[~both].tobytes() == fresh.arrays["trx"].reshape(-1, 12)[~both].tobytes()
    for k in ("cull_R", "cull_K", "cull_off"):              # (zero-area triangles have NaN normals: never hit)
        assert s.scalars[k] >= fresh.scalars[k]
    assert s.scalars["tri_flagged"] == int(rows_zero(s.arrays["trx"]).sum())


def test_every_validation_error_leaves_the_handle_unchanged(compiled):
    sd = gc.c2()
    nt = sd.counts["n_triangles"]
    m = gc.model()
    idx = np.array([5, 9, 100], np.int32)
    p, n = gc.original(idx)
    p = p + F(0.25)
    L = sl.lib()

    def call(tri_index, first, count, arrs):
        ti = None if tri_index is None else np.ascontiguousarray(tri_index, np.int32)
        return L.rts_compiled_update_geometry(m._h, sl._ip(ti), first, count, *[sl._fp(a) for a in arrs])
    good = sl.split_vertices(p, n)

    def bad_value(which, value):
        a = [x.copy() for x in good]
        a[which][1, 2] = value
        return a
    cases = {
        "null array": (idx, 0, 3, good[:2] + [None] + good[3:]),
        "negative count": (idx, 0, -1, good),
        "index below 0": ([5, -1, 100], 0, 3, good),
        "index past the end": ([5, nt, 100], 0, 3, good),
        "duplicate": ([5, 9, 5], 0, 3, good),
        "first with an index list": (idx, 1, 3, good),
        "range past the end": (None, nt - 2, 3, good),
        "negative first": (None, -1, 3, good),
        "NaN position": (idx, 0, 3, bad_value(0, np.nan)),
        "inf position": (idx, 0, 3, bad_value(2, np.inf)),
        "NaN normal": (idx, 0, 3, bad_value(4, np.nan)),
        "inf normal": (idx, 0, 3, bad_value(5, -np.inf)),
        "position of 2^30": (idx, 0, 3, bad_value(1, F(2.0 ** 30))),
    }
    for what, args in cases.items():
        assert call(*args) == RT_ERR_ARG, what
        s = m.snapshot()
        assert s.err, what
        gc.assert_arrays_equal(s.arrays, compiled.arrays, what=what)
        assert gc.bounds_of(s) == gc.bounds_of(compiled), what
    assert call(idx, 0, 0, [None] * 6) == 0 and call(None, 0, 0, good) == 0
    gc.assert_arrays_equal(m.snapshot().arrays, compiled.arrays, what="count == 0")
    a = bad_value(1, np.nextafter(F(2.0 ** 30), F(0)))      # the largest position accepted
    assert call(idx, 0, 3, a) == 0
    assert m.snapshot().scalars["cull_R"] == float(np.nextafter(F(2.0 ** 30), F(0)))


def check_plan(plan, arrays, scalars):
    nodes, q = arrays["nodes"], arrays["qnodes"]
    n_tri = scalars["n_tri"]
    leaves = plan["leaves"]
    cover = np.zeros(n_tri, np.int32)
    for ref, bslot, qslot, _ in leaves:
        first, n = (int(ref) & 0x7fffffff) >> 4, (int(ref) & 15) + 1
        cover[first:first + n] += 1
        if bslot >= 0:
            assert nodes[bslot // 2]["ref"][bslot % 2] == ref
        if qslot >= 0:
            assert q[qslot // 4]["ref"][qslot % 4] == ref
    assert np.all(cover == 1)                               # the leaves cover [0, n_tri) once
    for lst, off, arr, width in ((plan["blist"], plan["boff"], nodes, 2), (plan["qlist"], plan["qoff"], q, 4)):
        assert off[0] == 0 and off[-1] == len(lst) and np.all(np.diff(off) > 0 if len(lst) else True)
        assert len(set(lst.tolist())) == len(lst)           # every internal node once
        height = {}
        for h in range(1, len(off)):
            for i in lst[off[h - 1]:off[h]]:
                kids = [int(r) for r in arr[i]["ref"][:width] if r != sl.Q_EMPTY]
                hk = [0 if r < 0 else height[r] for r in kids]   # KeyError: a child not strictly lower
                assert 1 + max(hk) == h
                height[int(i)] = h
    return leaves


def test_refit_plan_of_c2(compiled):
    plan = gc.model().refit_plan()
    leaves = check_plan(plan, compiled.arrays, compiled.scalars)
    assert len(leaves) == 870 and np.all(leaves[:, 1] >= 0) and np.all(leaves[:, 2] >= 0)
    assert len(plan["blist"]) == len(compiled.arrays["nodes"]) == 869
    assert len(plan["qlist"]) == len(compiled.arrays["qnodes"])
    assert plan["blist"][-1] == compiled.scalars["root"] and plan["qlist"][-1] == compiled.scalars["qroot"]


def test_refit_plan_and_update_of_the_one_leaf_scene():
    sd = gc.one_leaf_scene()
    m = sl.CompiledHandle(sd.tri_enc, sd.node_enc)
    s0 = m.snapshot()
    assert s0.rc == 0 and s0.scalars["root"] < 0 and s0.scalars["qroot"] < 0      # the root is a leaf ref
    plan = m.refit_plan()
    check_plan(plan, s0.arrays, s0.scalars)
    assert plan["leaves"].tolist() == [[s0.scalars["root"], -1, -1, 0]]
    assert len(plan["blist"]) == 0 and len(plan["qlist"]) == 0
    nt = sd.counts["n_triangles"]
    p = sd.tri_enc[:, 0:3] + F(0.5)
    assert m.update_geometry(None, p, sd.tri_enc[:, 3:6]) == 0
    s = m.snapshot()
    gc.assert_arrays_equal(s.arrays, s0.arrays, names=("nodes", "qnodes"), what="one leaf: no node holds a box")
    assert s.arrays["tri"].reshape(nt, 3, 4)[:, :, 0:3].tobytes() == np.ascontiguousarray(p, F).tobytes()
