"""Synthetic first-hit frames for the temporal stage (tests/test_temporal_model.py on the CPU,
tests/test_gpu_temporal.py on the GPU): planes seen by a pinhole camera, traced in float64, with no
renderer involved, and the float64 geometry the analytic checks need.

A plane is (name, point, normal, material, keep) with keep(P) -> bool limiting its extent; the
camera is a FrameParams with exactly orthogonal unit front / right / up.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from rtamd.renderer import HIT_DTYPE, FrameParams

F = np.float32
D = np.float64
SIZES = {"70x37": (70, 37, 16), "64x36": (64, 36, 32)}   # W, H, tile: the denoiser's two sizes
HALF_H = float(np.tan(np.radians(15.0)))


def camera(W, H, position, basis="axis") -> FrameParams:
    """front = -z, right = +x, up = +y ("axis"), or the same turned about y by the 3-4-5 angle
    ("turned": unit and orthogonal to 1 ulp)."""
    if basis == "axis":
        front, right = np.array([0, 0, -1], F), np.array([1, 0, 0], F)
    else:
        front, right = np.array([0.6, 0, -0.8], F), np.array([0.8, 0, 0.6], F)
    up = np.array([0, 1, 0], F)
    half_h = F(HALF_H)
    half_w = F(half_h * F(W) / F(H))
    lbc = (front - half_w * right - half_h * up).astype(F)
    return FrameParams(position=np.asarray(position, F), front=front, right=right, up=up, left_bottom_corner=lbc,
                       half_h=float(half_h), half_w=float(half_w))


def moved(fp: FrameParams, W, H, right=0.0, up=0.0, front=0.0) -> FrameParams:
    """fp translated along its own axes (world units)"""
    pos = (np.asarray(fp.position, D) + right * np.asarray(fp.right, D) + up * np.asarray(fp.up, D)
           + front * np.asarray(fp.front, D)).astype(F)
    out = camera(W, H, pos)
    out.front, out.right, out.up, out.left_bottom_corner = fp.front, fp.right, fp.up, fp.left_bottom_corner
    return out


def pixel_size(fp: FrameParams, W, depth) -> float:
    """world units per pixel on a plane perpendicular to front at `depth`"""
    return 2.0 * float(F(fp.half_w)) * depth / W


def trace(fp: FrameParams, W, H, planes):
    """The first-hit frame of the planes: (hits (H, W) HIT_DTYPE, plane index per pixel or -1)"""
    pos = np.asarray(fp.position, F).astype(D)
    lbc, right, up = (np.asarray(v, F).astype(D) for v in (fp.left_bottom_corner, fp.right, fp.up))
    u = (np.arange(W) + 0.5) / W
    v = (np.arange(H) + 0.5) / H
    d = lbc + (u[None, :, None] * 2.0 * float(F(fp.half_w))) * right + (v[:, None, None] * 2.0 * float(F(fp.half_h))) * up
    best = np.full((H, W), np.inf)
    which = np.full((H, W), -1)
    P = np.zeros((H, W, 3))
    N = np.zeros((H, W, 3))
    for k, pl in enumerate(planes):
        p0, n = np.asarray(pl.point, D), np.asarray(pl.normal, D)
        n = n / np.linalg.norm(n)
        den = d @ n
        with np.errstate(all="ignore"):
            t = ((p0 - pos) @ n) / den
        Pk = pos + t[..., None] * d
        ok = np.isfinite(t) & (t > 0) & (t < best) & pl.keep(Pk)
        best = np.where(ok, t, best)
        which = np.where(ok, k, which)
        P = np.where(ok[..., None], Pk, P)
        N = np.where(ok[..., None], np.where((den > 0)[..., None], -n, n), N)
    hit = which >= 0
    hits = np.zeros((H, W), HIT_DTYPE)
    hits["triangle"] = which
    hits["t"] = np.where(hit, best * np.linalg.norm(d, axis=-1), -1.0)
    hits["point"] = P
    hits["normal"] = N
    hits["material"] = np.where(hit, np.array([pl.material for pl in planes])[np.maximum(which, 0)], 0)
    return hits, which


def project(fp: FrameParams, W, H, P):
    """float64 pixel coordinates (x, y) of the points P in fp's view (pixel centres at integers)"""
    pos, front, right, up, lbc = (np.asarray(v, F).astype(D) for v in
                                  (fp.position, fp.front, fp.right, fp.up, fp.left_bottom_corner))
    d = np.asarray(P, D) - pos
    k = (lbc @ front) / (d @ front)
    a = k * (d @ right) - lbc @ right
    b = k * (d @ up) - lbc @ up
    return a / (2.0 * float(F(fp.half_w))) * W - 0.5, b / (2.0 * float(F(fp.half_h))) * H - 0.5


def taps(x, y, W, H):
    """The four bilinear taps of (x, y): [(qx, qy, in_frame)], integer arrays"""
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    out = []
    for j in range(2):
        for i in range(2):
            qx, qy = x0 + i, y0 + j
            out.append((np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1), (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)))
    return out


def plane(name, point, normal, material, keep=None):
    return SimpleNamespace(name=name, point=point, normal=normal, material=material,
                           keep=keep or (lambda P: np.ones(P.shape[:-1], bool)))


def ulp(v):
    return np.spacing(np.abs(np.asarray(v, F))).astype(D)


# ---------------------------------------------------------------------------------------------
# The cases.  `run(color, hits, fp, tp, advance=False, reset=False) -> (out, n)` is the stage under
# test with one display history (the numpy model, or the GPU checked against it); every case starts
# with reset=True.  TP is anything with samples, max_history, sigma_normal, sigma_plane.
def TP(samples=1, max_history=32, sigma_normal=0.3, sigma_plane=0.01):
    return SimpleNamespace(samples=samples, max_history=max_history, sigma_normal=sigma_normal, sigma_plane=sigma_plane)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def case_linear_plane(size, run, basis="axis"):
    """A plane perpendicular to front whose history colour is affine in the world position; the
    camera then moves along right, up and front by non-integer pixel amounts.  World position is
    affine in pixel coordinates on such a plane, so the bilinear fetch reproduces the function at
    the new pixels' points: within 2^-10 of the colour's change across one pixel plus 8 ulp of the
    value.  Even pixels carry NaN input (the output is the fetched history itself), odd ones a
    finite colour (the output is the mean of both, alpha = 1/2)."""
    W, H, _ = SIZES[size]
    depth = 5.0
    fp1 = camera(W, H, (0.3, -0.2, 1.0), basis)
    front, right, up = (np.asarray(v, D) for v in (fp1.front, fp1.right, fp1.up))
    wall = plane("wall", np.asarray(fp1.position, D) + depth * front, -front, 3)
    px = pixel_size(fp1, W, depth)
    fp2 = moved(fp1, W, H, right=2.37 * px, up=-1.61 * px, front=-0.4)
    G = np.array([[0.50, 0.20, -0.10], [-0.30, 0.40, 0.25], [0.15, -0.35, 0.45]])
    c0 = np.array([6.0, 7.0, 6.5])
    f = lambda P: c0 + np.asarray(P, F).astype(D) @ G.T
    h1, w1 = trace(fp1, W, H, [wall])
    h2, w2 = trace(fp2, W, H, [wall])
    assert (w1 == 0).all() and (w2 == 0).all()
    hist = f(h1["point"]).astype(F)
    assert hist.min() > 0.5
    out, n = run(hist, h1, fp1, TP(), advance=True, reset=True)
    assert np.array_equal(bits(out), bits(hist)) and (n == 1).all()
    rng = np.random.default_rng(5)
    cur = rng.uniform(0.0, 4.0, (H, W, 3)).astype(F)
    nan = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
    cur[nan, 1] = np.nan
    out, n = run(cur, h2, fp2, TP(), advance=True)
    x, y = project(fp1, W, H, h2["point"])
    whole = (x >= 0) & (x < W - 1) & (y >= 0) & (y < H - 1)        # all four taps in the old frame
    none = (x < -1) | (x >= W) | (y < -1) | (y >= H)               # none of them
    edge = np.min([np.abs(v - b) for v, hi in ((x, W), (y, H)) for b in (-1, 0, hi - 1, hi)], axis=0)
    assert edge.min() > 1e-3, "the moves keep the float64 and the fp32 footprints in the same class"
    assert whole.mean() > 0.8 and none.sum() >= 20
    # no history: the input bit for bit (a NaN included), n = S for a finite input, 0 for a NaN
    assert np.array_equal(bits(out)[none], bits(cur)[none])
    assert np.array_equal(n[none], np.where(nan, 0, 1)[none])
    want = f(h2["point"])
    change = (np.abs(G @ right) + np.abs(G @ up)) * px
    tol = 2.0 ** -10 * change + 8 * ulp(want)
    a = whole & nan
    err = np.abs(out.astype(D) - want)
    assert (err[a] <= tol[a]).all(), (err[a] / tol[a]).max()
    assert (n[a] == 1).all()
    b = whole & ~nan
    mean = 0.5 * (want + cur.astype(D))
    err = np.abs(out.astype(D) - mean)
    assert (err[b] <= (0.5 * 2.0 ** -10 * change + 8 * ulp(mean))[b]).all()
    assert (n[b] == 2).all()
    return SimpleNamespace(whole=whole, none=none)


def _two_planes(size, variant):
    """A far wall and a nearer surface covering x < 0.1 of it: `material`: another material;
    `plane`: the wall's material (only the plane distance tells them apart); `tilted`: the wall
    itself, bent away by 30 degrees about the line x = 0.1 (same material, continuous depth: only the
    normal tells the halves apart)."""
    W, H, _ = SIZES[size]
    fp1 = camera(W, H, (0.0, 0.0, 0.0))
    far = 6.0
    if variant == "tilted":
        s, c = np.sin(np.radians(30.0)), np.cos(np.radians(30.0))
        planes = [plane("left", (0.1, 0.0, -far), (0.0, 0.0, 1.0), 1, lambda P: P[..., 0] < 0.1),
                  plane("right", (0.1, 0.0, -far), (s, 0.0, c), 1, lambda P: P[..., 0] >= 0.1)]
    else:
        planes = [plane("far", (0.0, 0.0, -far), (0.0, 0.0, 1.0), 1),
                  plane("near", (0.0, 0.0, -4.0), (0.0, 0.0, 1.0), 2 if variant == "material" else 1,
                        lambda P: P[..., 0] < 0.1)]
    px = pixel_size(fp1, W, far)
    fp2 = moved(fp1, W, H, right=3.37 * px, up=0.29 * px)  # the near edge slides left over the wall: a strip appears
    return W, H, fp1, fp2, planes


def case_disocclusion(size, run, variant):
    """After a sideways move exactly the newly revealed pixels of the far wall (no tap of the old
    frame shows the wall: float64 geometry) have n_out = min(S, max_history) and out == c bit for
    bit; every other hit pixel found a history.  With `plane` the same holds although both surfaces
    share a material, and opening sigma_plane wide makes revealed pixels find a (wrong) history:
    the plane test alone rejected them."""
    assert variant in ("material", "plane")
    W, H, fp1, fp2, planes = _two_planes(size, variant)
    h1, w1 = trace(fp1, W, H, planes)
    h2, w2 = trace(fp2, W, H, planes)
    rng = np.random.default_rng(9)
    c1 = rng.uniform(0.5, 2.0, (H, W, 3)).astype(F)
    c2 = rng.uniform(0.5, 2.0, (H, W, 3)).astype(F)
    x, y = project(fp1, W, H, h2["point"])
    edge = np.minimum(np.abs(x - np.round(x)), np.abs(y - np.round(y)))
    assert edge.min() > 1e-3
    same = np.zeros((H, W), bool)
    for qx, qy, ok in taps(x, y, W, H):
        same |= ok & (w1[qy, qx] == w2)
    revealed = (w2 == 0) & ~same
    inner = revealed & (x >= 0) & (x < W - 1)   # revealed from behind the near surface, not from off the frame
    assert inner.sum() >= 20 and (same & (w2 == 0)).sum() >= 200 and (same & (w2 == 1)).sum() >= 200
    for S, cap in ((1, 32), (3, 32), (5, 2)):
        run(c1, h1, fp1, TP(samples=S, max_history=cap), advance=True, reset=True)
        out, n = run(c2, h2, fp2, TP(samples=S, max_history=cap), advance=True)
        assert (n[~same] == min(S, cap)).all() and np.array_equal(bits(out)[~same], bits(c2)[~same])
        assert (np.abs(n[same] - min(min(S, cap) + S, cap)) <= 1e-5).all()   # (a weighted mean of equal lengths)
        if S < cap:
            assert (bits(out)[same] != bits(c2)[same]).any(-1).all()
    if variant == "plane":
        run(c1, h1, fp1, TP(), advance=True, reset=True)
        out, n = run(c2, h2, fp2, TP(sigma_plane=10.0), advance=True)
        assert (n[inner] == 2).all()
    return SimpleNamespace(revealed=revealed)


def case_tilted_neighbour(size, run):
    """A wall bent by 30 degrees about a vertical line, one material, history colour 1 on the left
    half and 4 on the right.  Pixels whose footprint straddles the bend take their history from
    their own half only (the values are powers of two: exactly); with sigma_normal opened wide the
    same pixels mix both halves, so the normal test alone rejected the taps."""
    W, H, fp1, fp2, planes = _two_planes(size, "tilted")
    h1, w1 = trace(fp1, W, H, planes)
    h2, w2 = trace(fp2, W, H, planes)
    assert (w1 >= 0).all() and (w2 >= 0).all()
    c1 = np.where((w1 == 0)[..., None], F(1.0), F(4.0)) * np.ones((H, W, 3), F)
    c2 = np.full((H, W, 3), np.nan, F)  # the output is the fetched history
    x, y = project(fp1, W, H, h2["point"])
    own = np.zeros((H, W), bool)
    other = np.zeros((H, W), bool)
    for qx, qy, ok in taps(x, y, W, H):
        own |= ok & (w1[qy, qx] == w2)
        other |= ok & (w1[qy, qx] != w2)
    straddle = own & other
    assert straddle.sum() >= H // 2
    # the other half's taps beside the bend pass the plane test (they lie within sigma_plane of the
    # pixel's own plane): float64
    P2, N2 = h2["point"].astype(D), h2["normal"].astype(D)
    passes = np.zeros((H, W), bool)
    for qx, qy, ok in taps(x, y, W, H):
        dist = np.abs(np.einsum("...k,...k", N2, h1["point"][qy, qx].astype(D) - P2)) / h2["t"]
        passes |= ok & (w1[qy, qx] != w2) & (dist <= 0.01)
    assert (passes & straddle).sum() >= H // 2
    run(c1, h1, fp1, TP(), advance=True, reset=True)
    out, n = run(c2, h2, fp2, TP(), advance=True)
    want = np.where(w2 == 0, F(1.0), F(4.0))
    assert (out[own] == want[own][:, None]).all() and (n[own] == 1).all()
    run(c1, h1, fp1, TP(), advance=True, reset=True)
    out, n = run(c2, h2, fp2, TP(sigma_normal=10.0), advance=True)
    mixed = passes & straddle
    assert (out[mixed] != want[mixed][:, None]).all()
    return SimpleNamespace(straddle=straddle)


def _still_scene(size):
    """A wall with a nearer panel of another material in front of its left part, ending below the
    top rows (camera misses above)"""
    W, H, _ = SIZES[size]
    fp = camera(W, H, (0.1, 0.05, 0.5))
    low = lambda P: P[..., 1] < 0.9
    planes = [plane("far", (0.0, 0.0, -6.0), (0.0, 0.0, 1.0), 1, low),
              plane("near", (0.0, 0.0, -4.0), (0.0, 0.0, 1.0), 2, lambda P: low(P) & (P[..., 0] < 0.1))]
    hits, which = trace(fp, W, H, planes)
    hit = which >= 0
    assert 20 <= (~hit).sum() and hit.mean() > 0.5 and len(np.unique(which)) == 3
    return W, H, fp, hits, hit


def case_bookkeeping(size, run):
    """Uniform colours, still camera.  A and B with S = 1 and ADVANCE, then C_k with samples = k,
    k = 1..4.  Every output is within 4 ulp of (n H + k C_k) / (n + k) against the frozen history H
    of length n.  Read literally (no C_k carries ADVANCE), the semantics of rt_abi.h freeze A's
    output: n = 1, H = A.  With C_1 carrying ADVANCE, as the caller's rule says for the first
    display after a restart, B's output is frozen: n = 2, H = mean(A, B), the formula
    (2 mean(A, B) + k C_k) / (2 + k).  Both are asserted."""
    W, H, fp, hits, hit = _still_scene(size)
    A, B = np.array([0.3, 1.7, 2.9]), np.array([1.1, 0.2, 3.3])
    Ck = [np.array([0.7, 2.3, 1.9]), np.array([0.9, 1.3, 2.2]), np.array([0.8, 1.6, 2.6]), np.array([0.85, 1.5, 2.4])]
    frame = lambda v: np.broadcast_to(np.asarray(v, F), (H, W, 3)).copy()
    f32 = lambda v: np.asarray(v, F).astype(D)

    def close(out, want, n, n_want):
        assert np.array_equal(bits(out)[~hit], bits(frame(c_in))[~hit]) and (n[~hit] == 0).all()
        err = np.abs(out[hit].astype(D) - want) / ulp(want)
        assert err.max() <= 4.0, err.max()
        assert (n[hit] == n_want).all()

    for first_advances in (True, False):
        c_in = A
        out, n = run(frame(A), hits, fp, TP(), advance=True, reset=True)
        assert np.array_equal(bits(out), bits(frame(A))) and (n[hit] == 1).all() and (n[~hit] == 0).all()
        c_in = B
        out, n = run(frame(B), hits, fp, TP(), advance=True)
        close(out, 0.5 * (f32(A) + f32(B)), n, 2)
        nH, Hc = (2, 0.5 * (f32(A) + f32(B))) if first_advances else (1, f32(A))
        for k in range(1, 5):
            c_in = Ck[k - 1]
            args = (frame(c_in), hits, fp, TP(samples=k))
            out, n = run(*args, advance=first_advances and k == 1)
            close(out, (nH * Hc + k * f32(c_in)) / (nH + k), n, nH + k)
            again, n2 = run(*args)   # repeated without ADVANCE: identical bits
            assert np.array_equal(bits(again), bits(out)) and np.array_equal(n2, n)
    # max_history = 2: alpha = 1/2 from the third frame on
    prev = None
    rng = np.random.default_rng(3)
    for k in range(5):
        c = rng.uniform(0.2, 3.0, 3)
        c_in = c
        out, n = run(frame(c), hits, fp, TP(max_history=2), advance=True, reset=k == 0)
        if k >= 1:
            close(out, 0.5 * (prev + f32(c)), n, 2)
        prev = out[hit].astype(D)
    # RESET: out == c, whatever came before
    out, n = run(frame(A), hits, fp, TP(samples=7), reset=True)
    assert np.array_equal(bits(out), bits(frame(A))) and (n[hit] == 7).all() and (n[~hit] == 0).all()


def case_passthrough(size, run):
    """Miss pixels and non-finite inputs without a history pass through bit for bit (n = 0); a planted
    NaN / inf with a history yields the history and its length."""
    W, H, fp, hits, hit = _still_scene(size)
    rng = np.random.default_rng(21)
    yx = np.argwhere(hit)[rng.choice(hit.sum(), 12, replace=False)]
    sel = np.zeros((H, W), bool)
    sel[yx[:, 0], yx[:, 1]] = True

    def planted(seed):
        c = np.random.default_rng(seed).uniform(0.0, 4.0, (H, W, 3)).astype(F)
        for k, (y, x) in enumerate(yx):
            if k < 3:
                c[y, x] = np.inf
            elif k < 6:
                c[y, x] = -np.inf, 1.0, np.nan
            else:
                c[y, x, k % 3] = np.frombuffer(np.uint32(0x7FC00000 + k).tobytes(), F)[0]  # NaNs with payloads
        sky = np.argwhere(~hit)[::3]
        c[sky[:, 0], sky[:, 1]] = np.inf
        return c

    c1 = planted(1)
    out, n = run(c1, hits, fp, TP(), advance=True, reset=True)
    assert np.array_equal(bits(out), bits(c1))
    assert (n[sel] == 0).all() and (n[~hit] == 0).all() and (n[hit & ~sel] == 1).all()
    c2 = np.random.default_rng(2).uniform(0.0, 4.0, (H, W, 3)).astype(F)
    out2, n2 = run(c2, hits, fp, TP(), advance=True)   # the planted pixels are no source: a fresh start there
    assert np.array_equal(bits(out2)[~hit], bits(c2)[~hit]) and (n2[~hit] == 0).all()
    assert np.isfinite(out2[hit]).all() and (n2[hit] >= 1).all()
    c3 = planted(3)
    out3, n3 = run(c3, hits, fp, TP(), advance=True)
    assert np.array_equal(bits(out3)[~hit], bits(c3)[~hit]) and (n3[~hit] == 0).all()
    # still camera: the history of a pixel is the pixel's own, within the fetch's bound (2^-10 of the
    # change across one pixel, here at most 4 in colour and 1 in length, plus 8 ulp)
    err = np.abs(out3[sel].astype(D) - out2[sel])
    assert (err <= 2.0 ** -10 * 4.0 + 8 * ulp(out2[sel])).all() and (np.abs(n3[sel] - n2[sel]) <= 2.0 ** -10).all()
