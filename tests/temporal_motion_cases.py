"""Small triangle scenes for the motion mode of the temporal stage (tests/test_temporal_motion_model.py on
the CPU, tests/test_gpu_temporal_motion.py on the GPU): a wall with a card in front of it, quads of
two triangles built through sl.Scene.add_triangles, and the float64 geometry the analytic checks need.

A case drives two stages through the same sequence, `on` (motion mode) and `off` (today's stage).  A
stage is anything with
    load(scene)                      the scene (rt_set_scene; drops the history)
    update(idx, p, n)                new vertices of triangles idx (rt_update_geometry)
    first_hit(fp, W, H)              the first-hit frame of the current pose
    call(color, hits, fp, tp, advance=False, reset=False, reuse=False) -> (out, n)
    resize()                         the same size again (rt_resize; drops the history)
ModelStage below is the numpy model with first-hit frames traced here in float64; the GPU stage runs
the library and compares every call with the model bit for bit.  Every builder asserts its own
premises in float64 on the frames it is given.
"""
from __future__ import annotations

import numpy as np

import temporal_cases as tc
import temporal_model as tm
import temporal_motion_model as mm
from rtamd import scene_lib as sl
from rtamd.renderer import HIT_DTYPE

F = np.float32
D = np.float64
SIZES = tc.SIZES
TP = tc.TP
bits = tc.bits
# (sizes that put no pixel centre of either frame size on a quad's diagonal: the two triangles share it)
WALL_Z, CARD_Z, WALL_HALF, CARD_HALF = -6.0, -4.0, (4.37, 2.61), (0.55, 0.47)
WALL_MAT = sl.Material(base_color=(0.7, 0.7, 0.7), roughness=0.8)
CARD_MAT = sl.Material(base_color=(0.9, 0.3, 0.2), roughness=0.6)


# ------------------------------------------------------------------------------------ scenes
def quad(cx, cy, z, hx, hy, back=False):
    """Two triangles of the rectangle (cx +- hx, cy +- hy) at depth z, normal +z (towards a camera at the
    origin looking along -z), or -z with `back` (reversed winding)"""
    a, b, c, d = (cx - hx, cy - hy, z), (cx + hx, cy - hy, z), (cx + hx, cy + hy, z), (cx - hx, cy + hy, z)
    tris = [a + b + c, a + c + d]
    if back:
        tris = [a + c + b, a + d + c]
    return np.array(tris, F)


class CaseScene:
    """soa: post-BVH arrays as rt_set_scene takes them; p, n: (n_tri, 3, 3) current vertices; card: the
    indices of the card's triangles"""

    def __init__(self, back=False):
        s = sl.Scene()
        s.add_triangles(quad(0.0, 0.0, WALL_Z, *WALL_HALF), WALL_MAT)
        s.add_triangles(quad(0.0, 0.0, CARD_Z, *CARD_HALF, back), CARD_MAT)
        s.build_bvh(8)
        self.soa, self.nodes = s.export_soa(), s.nodes()
        self.p = np.stack([self.soa[k] for k in ("p1", "p2", "p3")], axis=1).astype(F)
        self.n = np.stack([self.soa[k] for k in ("n1", "n2", "n3")], axis=1).astype(F)
        self.mid = self.soa["material_id"].astype(np.int32)
        is_card = np.isclose(self.p[:, 0, 2], CARD_Z)
        assert is_card.sum() == 2 and len(is_card) == 4 and len(set(self.mid[is_card]) | set(self.mid[~is_card])) == 2
        self.card = np.flatnonzero(is_card).astype(np.int32)
        want = -1.0 if back else 1.0
        assert np.allclose(self.n[self.card], (0.0, 0.0, want)) and np.allclose(self.n[~is_card], (0.0, 0.0, 1.0))

    def card_moved(self, shift=(0.0, 0.0, 0.0), yaw_deg=0.0, base=None):
        """(p, n) of the card's triangles of the scene's own pose (or `base`), turned about the vertical
        axis through the card's centre, then translated: float64, rounded once"""
        p, n = (self.p[self.card], self.n[self.card]) if base is None else base
        a = np.radians(yaw_deg)
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        c = np.array([0.0, 0.0, CARD_Z])
        return ((p.astype(D) - c) @ R.T + c + np.asarray(shift, D)).astype(F), (n.astype(D) @ R.T).astype(F)


def trace(fp, W, H, p, n, mid):
    """The first-hit frame of the triangles in float64 (Moeller-Trumbore on the fp32 vertices): the
    interpolated unit normal, turned against the ray (`inside` where it was turned)"""
    pos = np.asarray(fp.position, F).astype(D)
    lbc, right, up = (np.asarray(v, F).astype(D) for v in (fp.left_bottom_corner, fp.right, fp.up))
    u, v = (np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H
    d = lbc + (u[None, :, None] * 2.0 * float(F(fp.half_w))) * right + (v[:, None, None] * 2.0 * float(F(fp.half_h))) * up
    best = np.full((H, W), np.inf)
    hits = np.zeros((H, W), HIT_DTYPE)
    hits["triangle"], hits["t"] = -1, -1.0
    for t in range(len(p)):
        p1, p2, p3 = p[t].astype(D)
        e1, e2 = p2 - p1, p3 - p1
        h = np.cross(d, e2)
        a = h @ e1
        with np.errstate(all="ignore"):
            s = pos - p1
            bu = (h @ s) / a
            q = np.cross(s, e1)
            bv = (d @ q) / a
            tt = (q @ e2) / a
        ok = (np.abs(a) > 1e-12) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (tt > 0) & (tt < best)
        best = np.where(ok, tt, best)
        N = (1 - bu - bv)[..., None] * n[t, 0].astype(D) + bu[..., None] * n[t, 1].astype(D) + bv[..., None] * n[t, 2].astype(D)
        with np.errstate(all="ignore"):
            N = N / np.linalg.norm(N, axis=-1, keepdims=True)
        inside = np.einsum("...k,...k", N, d) > 0
        N = np.where(inside[..., None], -N, N)
        hits["triangle"][ok] = t
        hits["t"][ok] = (tt * np.linalg.norm(d, axis=-1))[ok]
        hits["point"][ok] = (pos + tt[..., None] * d)[ok]
        hits["normal"][ok] = N[ok]
        hits["inside"][ok] = inside[ok]
        hits["material"][ok] = mid[t]
    return hits


class ModelStage:
    def __init__(self, motion: bool):
        self.motion = motion
        self.model = mm.MotionTemporal() if motion else tm.Temporal()

    def load(self, scene: CaseScene):
        self.p, self.n, self.mid = scene.p.copy(), scene.n.copy(), scene.mid
        self.model.drop()

    def update(self, idx, p, n):
        self.p[idx], self.n[idx] = p, n

    def first_hit(self, fp, W, H):
        return trace(fp, W, H, self.p, self.n, self.mid)

    def call(self, color, hits, fp, tp, advance=False, reset=False, reuse=False):
        if self.motion:
            return self.model.call(color, hits, fp, tp, mm.pose_of(self.p, self.n), advance=advance, reset=reset)
        return self.model.call(color, hits, fp, tp, advance=advance, reset=reset)

    def resize(self):
        self.model.drop()


# ------------------------------------------------------------------------------------ helpers
def still_camera(W, H):
    return tc.camera(W, H, (0.0, 0.0, 0.0))


def px_at(fp, W, depth):
    return tc.pixel_size(fp, W, depth)


def colours(H, W, seed, lo=0.5, hi=2.0):
    return np.random.default_rng(seed).uniform(lo, hi, (H, W, 3)).astype(F)


def same(a, b, where=None):
    (oa, na), (ob, nb) = a, b
    m = np.ones(na.shape, bool) if where is None else where
    assert np.array_equal(bits(oa)[m], bits(ob)[m]) and np.array_equal(bits(na)[m], bits(nb)[m])


def on_card(scene, hits):
    return np.isin(hits["triangle"], scene.card)


def old_points(hits2, scene, p_old, p_new):
    """float64: the surface points of the current frame's card pixels where the card's old pose had
    them (the pixel's barycentrics in the new triangle, applied to the old one)"""
    P = hits2["point"].astype(D)
    out = P.copy()
    for k, t in enumerate(scene.card):
        m = hits2["triangle"] == t
        a, b, c = p_new[k].astype(D)
        M = np.stack([b - a, c - a], axis=1)                      # 3 x 2
        uv = np.linalg.lstsq(M, (P[m] - a).T, rcond=None)[0].T
        qa, qb, qc = p_old[k].astype(D)
        out[m] = qa + uv[:, :1] * (qb - qa) + uv[:, 1:] * (qc - qa)
    return out


def footprint(fp1, W, H, P, which1, wanted, among=None):
    """(x, y, whole): the float64 footprint of the points P in the history's view and whether all four
    taps lie in the frame on pixels whose triangle is in `wanted`.  Asserts that no pixel of `among`
    is within 1e-3 px of changing that class; without `among`, whole means: and stays so within 1e-3 px."""
    x, y = tc.project(fp1, W, H, P)

    def whole_at(x, y):
        whole = np.ones(x.shape, bool)
        for qx, qy, ok in tc.taps(x, y, W, H):
            whole &= ok & np.isin(which1[qy, qx], wanted)
        return whole

    whole = whole_at(x, y)
    for dx in (-1e-3, 1e-3):
        for dy in (-1e-3, 1e-3):
            near = whole_at(x + dx, y + dy)
            if among is None:
                whole = whole & near
            else:
                assert np.array_equal(near[among], whole[among]), "a footprint within 1e-3 px of a class boundary"
    return x, y, whole


# ------------------------------------------------------------------------------------ the cases
def case_nothing_moved(size, on, off):
    """Camera moves, ADVANCE and REUSE over a still scene: every output and n of the motion mode equals
    the mode-off run bit for bit."""
    W, H, _ = SIZES[size]
    scene = CaseScene()
    fp1 = still_camera(W, H)
    fp2 = tc.moved(fp1, W, H, right=3.37 * px_at(fp1, W, 6.0), up=0.29 * px_at(fp1, W, 6.0), front=-0.2)
    res = []
    for st in (on, off):
        st.load(scene)
        h1, h2 = st.first_hit(fp1, W, H), st.first_hit(fp2, W, H)
        assert on_card(scene, h1).sum() >= 100 and (h1["triangle"] >= 0).all()
        r = [st.call(colours(H, W, 1), h1, fp1, TP(), advance=True, reset=True),
             st.call(colours(H, W, 2), h2, fp2, TP(), advance=True),
             st.call(colours(H, W, 3), h2, fp2, TP(samples=2), reuse=True),
             st.call(colours(H, W, 4), h1, fp1, TP(), advance=True)]
        res.append(r)
    for a, b in zip(*res):
        same(a, b)
    assert (res[0][1][1] == 2).mean() > 0.5


def case_unmoved_beside_moved(size, on, off):
    """Only the card moves (sideways, 3.37 px at its depth; the camera strafes too).  Every pixel whose
    triangle did not move equals the mode-off run bit for bit, the strip of wall the card uncovered
    included: there n = min(S, max_history) and out == c."""
    W, H, _ = SIZES[size]
    scene = CaseScene()
    fp1 = still_camera(W, H)
    fp2 = tc.moved(fp1, W, H, right=0.41 * px_at(fp1, W, 6.0), up=0.23 * px_at(fp1, W, 6.0))
    shift = (3.37 * px_at(fp1, W, 4.0), 0.0, 0.0)
    pn = scene.card_moved(shift)
    res = []
    for st in (on, off):
        st.load(scene)
        h1 = st.first_hit(fp1, W, H)
        a = st.call(colours(H, W, 5), h1, fp1, TP(), advance=True, reset=True)
        st.update(scene.card, *pn)
        h2 = st.first_hit(fp2, W, H)
        c2 = colours(H, W, 6)
        res.append((a, st.call(c2, h2, fp2, TP(), advance=True), h1, h2))
    (a_on, b_on, h1, h2), (a_off, b_off, _, _) = res
    same(a_on, a_off)
    wall = (h2["triangle"] >= 0) & ~on_card(scene, h2)
    assert wall.sum() >= 500 and on_card(scene, h2).sum() >= 100
    same(b_on, b_off, wall)
    # the uncovered strip: wall now, and every tap of the static footprint shows the old card
    x, y, covered = footprint(fp1, W, H, h2["point"], h1["triangle"], scene.card, wall)
    strip = wall & covered
    assert strip.sum() >= 10, strip.sum()
    out, n = b_on
    assert (n[strip] == 1).all() and np.array_equal(bits(out)[strip], bits(c2)[strip])
    assert (n[wall & ~strip] == 2).mean() > 0.9


# the worst error of the fp32 model against the float64 geometry over case_translation's pixels (both
# sizes, still and moving camera), in units of the static case's bound 2^-10 change + 8 ulp, measured
# on the CPU (tests/test_temporal_motion_model.py prints it), and the bound: twice that
TRANSLATION_WORST = 0.027
TRANSLATION_BOUND = 2.0 * TRANSLATION_WORST


def case_translation(size, on, off, camera_moves):
    """The card, parallel to the image plane, carries a history colour affine in its own coordinates
    and moves in its plane by (2.37, -1.61) px at its depth; the camera stands still, or moves as in
    tc.case_linear_plane.  Pixels whose four history taps lie on the old card reproduce the function
    at their own surface points: out = (f + c) / 2, n = 2, within TRANSLATION_BOUND x (2^-10 of the
    colour's change across one pixel + 8 ulp).  Measured on the CPU model against the float64
    geometry: worst 0.0264 of that unit (0.0248, 0.0237, 0.0240, 0.0264 for the two sizes with a still
    and a moving camera: about one ulp of the value, the barycentric reconstruction adds no more),
    stated as 0.027; bound 0.054.  The same pixels of the mode-off run miss the bound for a
    majority: it fetches the history of the place, not of the surface."""
    W, H, _ = SIZES[size]
    scene = CaseScene()
    fp1 = still_camera(W, H)
    px = px_at(fp1, W, -CARD_Z)
    fp2 = tc.moved(fp1, W, H, right=2.37 * px, up=-1.61 * px, front=-0.4) if camera_moves else fp1
    shift = np.array([2.37 * px, -1.61 * px, 0.0])
    pn = scene.card_moved(shift)
    G = np.array([[0.50, 0.20, -0.10], [-0.30, 0.40, 0.25], [0.15, -0.35, 0.45]])
    c0 = np.array([6.0, 7.0, 6.5])
    f = lambda P: c0 + np.asarray(P, D) @ G.T
    res = []
    for st in (on, off):
        st.load(scene)
        h1 = st.first_hit(fp1, W, H)
        hist = f(h1["point"].astype(D)).astype(F)
        assert hist.min() > 0.5
        st.call(hist, h1, fp1, TP(), advance=True, reset=True)
        st.update(scene.card, *pn)
        h2 = st.first_hit(fp2, W, H)
        cur = colours(H, W, 8, 0.0, 4.0)
        res.append((st.call(cur, h2, fp2, TP(), advance=True), h1, h2, cur))
    (got_on, h1, h2, cur), (got_off, _, _, _) = res
    card2 = on_card(scene, h2)
    Pold = old_points(h2, scene, scene.p[scene.card], pn[0])
    x, y, whole = footprint(fp1, W, H, Pold, h1["triangle"], scene.card, card2)
    sel = card2 & whole
    assert sel.sum() >= 150, sel.sum()
    right, up = np.asarray(fp1.right, D), np.asarray(fp1.up, D)
    change = (np.abs(G @ right) + np.abs(G @ up)) * px
    want = 0.5 * (f(Pold) + cur.astype(D))
    unit = 0.5 * 2.0 ** -10 * change + 8 * tc.ulp(want)
    out, n = got_on
    ratio = (np.abs(out.astype(D) - want) / unit)[sel]
    print(f"case_translation {size} camera_moves={camera_moves}: worst error {ratio.max():.4f} of the static bound's unit")
    assert ratio.max() <= TRANSLATION_BOUND, ratio.max()
    assert (n[sel] == 2).all()
    out_off, _ = got_off
    missed = ((np.abs(out_off.astype(D) - want) / unit) > TRANSLATION_BOUND).any(-1)[sel]
    assert missed.mean() > 0.5, missed.mean()
    return float(ratio.max())


def case_rotation(size, on, off, back=False):
    """The card turns 40 degrees about the vertical axis through its centre (|dN| = 0.68 > 0.3); history
    colour 4, input 2 (powers of two: the blend is exact), sigma_plane opened to 0.5 so that the normal
    test is the only one that can tell the old card from the new.  Motion mode: the pixels whose four
    taps lie on the old card keep their history, n = 2 and out = 3 exactly.  Mode off: none of them
    does; with sigma_normal opened wide they do, so the predicted normal alone decided.  `back`: the
    card shows its back (the hit normal is the vertex normal negated): the same results pin `flip`."""
    W, H, _ = SIZES[size]
    scene = CaseScene(back)
    fp = still_camera(W, H)
    pn = scene.card_moved(yaw_deg=40.0)
    assert abs(np.linalg.norm(pn[1][0, 0].astype(D) - scene.n[scene.card][0, 0]) - 0.68) < 0.01
    tp = TP(sigma_plane=0.5)
    res = {}
    for name, st, tp2 in (("on", on, tp), ("off", off, tp), ("wide", off, TP(sigma_normal=10.0, sigma_plane=0.5))):
        st.load(scene)
        h1 = st.first_hit(fp, W, H)
        c1 = np.full((H, W, 3), 4.0, F)
        st.call(c1, h1, fp, tp, advance=True, reset=True)
        st.update(scene.card, *pn)
        h2 = st.first_hit(fp, W, H)
        res[name] = (st.call(np.full((H, W, 3), 2.0, F), h2, fp, tp2, advance=True), h1, h2)
    (out, n), h1, h2 = res["on"]
    card1, card2 = on_card(scene, h1), on_card(scene, h2)
    if back:
        assert (h1["inside"][card1] == 1).all() and (h2["inside"][card2] == 1).all() and (h1["normal"][card1][:, 2] > 0.99).all()
    Pold = old_points(h2, scene, scene.p[scene.card], pn[0])
    x, y, whole = footprint(fp, W, H, Pold, h1["triangle"], scene.card, card2)
    sel = card2 & whole
    assert sel.sum() >= 100, sel.sum()
    assert (n[sel] == 2).all() and (out[sel] == 3.0).all()
    (out_off, n_off), _, _ = res["off"]
    assert (n_off[card2] == 1).all() and (out_off[card2] == 2.0).all()
    # static footprint on the old card: the material matches and the plane test is open
    xs, ys, static_whole = footprint(fp, W, H, h2["point"], h1["triangle"], scene.card)
    (out_w, n_w), _, _ = res["wide"]
    back_again = card2 & static_whole
    assert back_again.sum() >= 100 and (n_w[back_again] == 2).all() and (out_w[back_again] == 3.0).all()


def case_pose_bookkeeping(size, on, off):
    """Two updates between two displayed frames; an update that returns every vertex to its old bits
    (static path: equals mode off); the tick after an update with REUSE_GUIDES and no ADVANCE (the
    history's pose is still the old one); RESET, a scene set and a resize drop the poses."""
    W, H, _ = SIZES[size]
    scene = CaseScene()
    fp = still_camera(W, H)
    px = px_at(fp, W, -CARD_Z)
    step1 = scene.card_moved((1.3 * px, 0.0, 0.0))
    step2 = scene.card_moved((2.45 * px, 0.7 * px, 0.0), yaw_deg=10.0)
    home = (scene.p[scene.card], scene.n[scene.card])
    c = [colours(H, W, 20 + k) for k in range(8)]
    res = []
    for st in (on, off):
        r = {}
        st.load(scene)
        h1 = st.first_hit(fp, W, H)
        r["first"] = st.call(c[0], h1, fp, TP(), advance=True, reset=True)
        st.update(scene.card, *step1)
        st.update(scene.card, *step2)                      # two updates, no display between them
        h2 = st.first_hit(fp, W, H)
        r["two"] = st.call(c[1], h2, fp, TP(), advance=True)
        r["reuse"] = st.call(c[2], h2, fp, TP(samples=2), reuse=True)   # the history is still the first frame's
        st.update(scene.card, *home)                       # every vertex back to the bits of the first frame
        h3 = st.first_hit(fp, W, H)
        r["home"] = st.call(c[3], h3, fp, TP(), reset=True, advance=True)
        st.update(scene.card, *step1)
        st.update(scene.card, *home)
        r["there-and-back"] = st.call(c[4], h3, fp, TP(), advance=True)
        # the drops: after each, the next call has no history whatever moved before it
        for k, drop in enumerate(("reset", "scene", "resize")):
            st.update(scene.card, *step2)
            if drop == "scene":
                st.load(scene)
            elif drop == "resize":
                st.resize()
            hk = st.first_hit(fp, W, H)
            r[drop] = st.call(c[5 + k], hk, fp, TP(), advance=True, reset=drop == "reset")
            assert np.array_equal(bits(r[drop][0]), bits(c[5 + k])) and (r[drop][1] == 1).all()
        r["hits"] = (h1, h2)
        res.append(r)
    r_on, r_off = res
    h1, h2 = r_on["hits"]
    for k in ("first", "home", "there-and-back", "reset", "scene", "resize"):
        same(r_on[k], r_off[k])
    assert (r_on["there-and-back"][1] == 2).all()
    # after the two updates the card's pixels kept their history in motion mode (old pose = the first
    # frame's, whatever happened between), and in the tick after it with REUSE
    Pold = old_points(h2, scene, home[0], step2[0])
    x, y, whole = footprint(fp, W, H, Pold, h1["triangle"], scene.card, on_card(scene, h2))
    sel = on_card(scene, h2) & whole
    assert sel.sum() >= 100
    assert (r_on["two"][1][sel] == 2).all() and (r_on["reuse"][1][sel] == 3).all()
    assert not (r_off["two"][1][sel] == 2).all()


def case_callers_hits(size, on, off):
    """A caller's first-hit frame with triangle indices n_triangles and 2^30 on hit pixels of a moved
    card: those pixels take the static path (the mode-off result), and nothing is read out of bounds."""
    W, H, _ = SIZES[size]
    scene = CaseScene()
    fp = still_camera(W, H)
    pn = scene.card_moved((1.7 * px_at(fp, W, -CARD_Z), 0.0, 0.0))
    res = []
    for st in (on, off):
        st.load(scene)
        h1 = st.first_hit(fp, W, H)
        st.call(colours(H, W, 30), h1, fp, TP(), advance=True, reset=True)
        st.update(scene.card, *pn)
        h2 = st.first_hit(fp, W, H).copy()
        card = on_card(scene, h2)
        yy, xx = np.nonzero(card)
        planted = np.zeros((H, W), bool)
        planted[yy[::2], xx[::2]] = True
        odd = np.zeros((H, W), bool)
        odd[yy[::4], xx[::4]] = True
        h2["triangle"][planted] = len(scene.p)
        h2["triangle"][odd] = 2 ** 30
        res.append((st.call(colours(H, W, 31), h2, fp, TP(), advance=True), planted, card))
    (a, planted, card), (b, _, _) = res
    assert planted.sum() >= 50
    same(a, b, planted)
    assert not np.array_equal(bits(a[1])[card & ~planted], bits(b[1])[card & ~planted])


CASES = {
    "nothing-moved": case_nothing_moved,
    "unmoved-beside-moved": case_unmoved_beside_moved,
    "translation-still": lambda s, on, off: case_translation(s, on, off, False),
    "translation-camera": lambda s, on, off: case_translation(s, on, off, True),
    "rotation": case_rotation,
    "back-face": lambda s, on, off: case_rotation(s, on, off, True),
    "pose-bookkeeping": case_pose_bookkeeping,
    "callers-hits": case_callers_hits,
}
