"""CPU: the culling bound of the GPU traversal against the reference's own
triangle test, evaluated in fp32 exactly as RT:241-299 does.

The GPU skips a subtree when its box entry t0 exceeds cull_limit(best) = best + 1e-3 +
1e-3*best + eps*max|1/d_a| (rt_kernels.h), with eps from cull_bound_stats (scene_compile.h):
eps = 2 (K u R + off), K = max over triangles of 44 + 70/cos(theta), u = 2^-24.  That is exact
(never drops the reference's closest hit) if every hit the reference accepts has its point
X = S + d*t within eps/2 of the triangle (so of every box holding it).  Here millions of
adversarial (triangle, ray) pairs are thrown at the restated test:
  * rays aimed at points just inside / outside an edge or a vertex (barycentric ~ +-1e-7);
  * grazing directions, |d.N| in [1e-5, 1e-3] (where t = num/dn is worst conditioned) and
    near-axis-parallel directions (a tiny |d_a| makes eps*|1/d_a| the dominant term);
  * slivers, large and tiny triangles, coordinates up to |R| = 64;
and for every accepted hit: the distance of X from the triangle's bounding box must stay below
the per-triangle bound, and the end-to-end culling statement t >= t0 - eps*max|1/d| - slack must
hold with the box entry t0 computed in fp32 as the GPU does (RT:303-316).
"""
import numpy as np
import pytest

F = np.float32
U = 2.0 ** -24


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def geometric_normal(p1, p2, p3):
    """scene_compile.h geometric_normal: the fp32 operations of normalize(cross(p2-p1, p3-p1))."""
    c = cross(p2 - p1, p3 - p1)
    with np.errstate(all="ignore"):
        inv = F(1) / np.sqrt(dot(c, c))
        return c * inv[..., None]


def hit_triangle(p1, p2, p3, N, S, d):
    """RT:253-281 in fp32, one op at a time (numpy does not contract).  Returns accepted, t."""
    with np.errstate(all="ignore"):
        dn0 = dot(N, d)
        N = np.where((dn0 > 0)[..., None], -N, N)
        dn = dot(N, d)
        ok = ~(np.abs(dn) < F(0.00001))
        t = (dot(N, p1) - dot(S, N)) / dot(d, N)
        ok &= ~(t < F(0.0005))
        P = S + d * t[..., None]
        c1 = dot(cross(p2 - p1, P - p1), N)
        c2 = dot(cross(p3 - p2, P - p2), N)
        c3 = dot(cross(p1 - p3, P - p3), N)
        ok &= ((c1 > 0) & (c2 > 0) & (c3 > 0)) | ((c1 < 0) & (c2 < 0) & (c3 < 0))
    return ok, t


def per_triangle_bound(p1, p2, p3, N, R):
    """cull_bound_stats per triangle: K u R + off (in float64), K = inf when badly conditioned."""
    a = p2.astype(np.float64) - p1.astype(np.float64)   # the edges in float64, as cull_bound_stats takes them
    b = p3.astype(np.float64) - p1.astype(np.float64)
    cx = np.cross(a, b)
    nrm = np.linalg.norm(cx, axis=-1)
    with np.errstate(all="ignore"):
        cos = np.einsum("ij,ij->i", N.astype(np.float64), cx) / nrm
    K = np.where(cos > 0.25, 44.0 + 70.0 / cos, np.inf)
    off = np.maximum(np.abs(np.einsum("ij,ij->i", a, N.astype(np.float64))),
                     np.abs(np.einsum("ij,ij->i", b, N.astype(np.float64))))
    return K * U * R + off, K


def box_dist(X, lo, hi):
    return np.max(np.maximum(np.maximum(lo - X, X - hi), 0.0), axis=-1)


def slab_entry(S, inv, lo, hi):
    """t0 of RT:309-313 in fp32."""
    f = (hi - S) * inv
    n = (lo - S) * inv
    return np.max(np.minimum(f, n), axis=-1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_case(rng, n, kind):
    scale = rng.choice([1e-3, 0.05, 1.0, 8.0], size=(n, 1))
    centre = rng.uniform(-48, 48, size=(n, 3))
    p1 = centre + rng.normal(size=(n, 3)) * scale
    p2 = centre + rng.normal(size=(n, 3)) * scale
    p3 = centre + rng.normal(size=(n, 3)) * scale
    if kind == "sliver":
        p3 = p1 + (p2 - p1) * rng.uniform(0, 1, size=(n, 1)) + rng.normal(size=(n, 3)) * scale * 1e-3
    if kind == "skim":  # near the extreme vertex along axis b, ray almost parallel to axis a != b
        P3 = np.stack([p1, p2, p3], 1)
        a = rng.integers(0, 3, size=n)
        b = (a + rng.integers(1, 3, size=n)) % 3
        vi = np.argmax(P3[np.arange(n), :, b] * rng.choice([-1, 1], size=n)[:, None], axis=1)
        w = np.abs(rng.normal(size=(n, 3))) * 10.0 ** rng.uniform(-8, -5, size=(n, 1))
        w[np.arange(n), vi] = 1.0 - (w.sum(1) - w[np.arange(n), vi])
        target = (w[:, :, None] * P3).sum(1)
        d = np.zeros((n, 3))
        d[np.arange(n), a] = rng.choice([-1, 1], size=n)
        d = _unit(d + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-7, -3, size=(n, 1)))
        S = target - d * rng.uniform(0.01, 40.0, size=(n, 1))
        return [x.astype(F) for x in (p1, p2, p3, S, d)]
    # a target near an edge or a vertex, slightly inside or outside
    w = rng.dirichlet([1, 1, 1], size=n)
    k = rng.integers(0, 3, size=n)
    w[np.arange(n), k] = rng.normal(size=n) * 1e-7
    if kind == "vertex":
        w[:] = 0.0
        w[np.arange(n), k] = 1.0
        w += rng.normal(size=(n, 3)) * 1e-7
    w /= w.sum(1, keepdims=True)
    target = w[:, 0:1] * p1 + w[:, 1:2] * p2 + w[:, 2:3] * p3
    n_true = _unit(np.cross(p2 - p1, p3 - p1))
    if kind == "grazing":
        tang = _unit(np.cross(n_true, rng.normal(size=(n, 3))))
        g = 10.0 ** rng.uniform(-5, -3, size=(n, 1))
        d = _unit(tang + g * n_true * rng.choice([-1, 1], size=(n, 1)))
    elif kind == "axis":
        d = np.zeros((n, 3))
        a = rng.integers(0, 3, size=n)
        d[np.arange(n), a] = rng.choice([-1, 1], size=n)
        d += rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-7, -2, size=(n, 1))
        d = _unit(d)
    else:
        d = _unit(rng.normal(size=(n, 3)))
    t = rng.uniform(0.01, 40.0, size=(n, 1))
    S = target - d * t
    return [x.astype(F) for x in (p1, p2, p3, S, d)]


@pytest.mark.parametrize("kind", ["edge", "vertex", "grazing", "axis", "sliver", "skim"])
def test_accepted_hits_stay_within_the_bound(kind):
    rng = np.random.default_rng({"edge": 1, "vertex": 2, "grazing": 3, "axis": 4, "sliver": 5, "skim": 6}[kind])
    worst, accepted = 0.0, 0
    for _ in range(4):
        p1, p2, p3, S, d = make_case(rng, 250_000, kind)
        N = geometric_normal(p1, p2, p3)
        ok, t = hit_triangle(p1, p2, p3, N, S, d)
        R = float(max(np.abs(np.stack([p1, p2, p3, S])).max(), 1.0))
        eps_half, K = per_triangle_bound(p1, p2, p3, N, R)
        lo = np.minimum(np.minimum(p1, p2), p3).astype(np.float64)
        hi = np.maximum(np.maximum(p1, p2), p3).astype(np.float64)
        X = S.astype(np.float64) + d.astype(np.float64) * t.astype(np.float64)[:, None]
        dist = box_dist(X, lo, hi)
        sel = ok & np.isfinite(eps_half)
        accepted += int(sel.sum())
        assert np.all(dist[sel] <= eps_half[sel]), (kind, float((dist[sel] / eps_half[sel]).max()))
        if sel.any():
            worst = max(worst, float((dist[sel] / eps_half[sel]).max()))
        # end to end: the GPU culls the box only if t0 > cull_limit(best); a hit at dist <= best
        # in that box would need t < t0 - eps*max|1/d| - margin, which must never happen
        with np.errstate(all="ignore"):
            inv = F(1) / d
            t0 = slab_entry(S, inv, np.minimum(np.minimum(p1, p2), p3), np.maximum(np.maximum(p1, p2), p3))
        eps = 2.0 * eps_half
        m = np.max(np.abs(inv.astype(np.float64)), axis=-1)
        lim_t = t0.astype(np.float64) - eps * m
        tt = t.astype(np.float64)
        assert np.all(tt[sel] + 1e-3 + 1e-3 * tt[sel] >= lim_t[sel] - 1e-30)
    assert accepted > 1000, accepted
    print(f"{kind}: {accepted} accepted hits, worst distance / bound = {worst:.3g}")


def test_scene_bound_is_finite_for_the_configurations():
    """cull_bound_stats is finite (culling stays on) for every configuration scene, and eps is
    small against the 1e-3 margin: only rays with min |d_a| below eps / 1e-3 lose culling."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "opengl-ray-tracing-framework_amd"))
    from rtamd import configs as cf
    for name in ("C2", "C3", "C5"):
        sd = cf.config_scene(name)
        tri = sd.tri_enc.astype(F)
        p1, p2, p3 = tri[:, 0], tri[:, 1], tri[:, 2]
        N = geometric_normal(p1, p2, p3)
        R = max(float(np.abs(tri[:, :3]).max()), 7.0)   # camera at (0, 0, 7)
        eps_half, K = per_triangle_bound(p1, p2, p3, N, R)
        assert np.isfinite(K).all(), name
        eps = 2.0 * float(eps_half.max())
        assert eps < 2e-4, (name, eps)


def test_round1_margin_had_a_hole():
    """The round-1 margin (best + 1e-3 + 1e-3*best, no eps*max|1/d| term) is not exact: near
    axis-parallel rays produce accepted hits several units before their own box's entry.
    tests/cull_cases.py builds a scene from one; the oracle keeps the triangle the old margin
    would cull (GPU side: tests/test_gpu_cull.py)."""
    from cull_cases import old_margin_counterexample
    import oracle as orc
    from rtamd import configs as cf
    c = old_margin_counterexample()
    assert c["t_hit"] < c["t_wall"] < c["t0_box"]
    best = np.float32(c["t_wall"]) - np.float32(1e-5)
    assert c["t0_box"] > best + 1e-3 + 1e-3 * best          # the old rule culls T's box
    hdr, cache = cf.load_env()
    fp = cull_frame_params(c)
    img, cnt = orc.render(orc.OracleScene(c["tri_enc"], c["node_enc"], hdr, cache),
                          [cf.oracle_frame_params(fp, 1, cf.rand_origins(1)[0])], 4, 4)
    assert np.all(img[..., 0] > 4.0 * np.maximum(img[..., 1], img[..., 2])), img   # T is red-emissive


def cull_frame_params(c):
    """Every pixel casts the counterexample's ray: half_w = half_h = 0, lbc = the direction."""
    from rtamd.renderer import FrameParams
    return FrameParams(position=tuple(float(x) for x in c["position"]), front=tuple(float(x) for x in c["lbc"]),
                       right=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0),
                       left_bottom_corner=tuple(float(x) for x in c["lbc"]), half_h=0.0, half_w=0.0)
