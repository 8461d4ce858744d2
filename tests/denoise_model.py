"""The display denoiser of include/rt_abi.h (rt_denoise) in numpy fp32: the model the kernels of
csrc/hip/rt_denoise.h are compared with bit for bit.

Every step is one correctly rounded fp32 operation in the order of DESIGN.md §4 (numpy float32
arithmetic is IEEE binary32 without contraction).  `exp_` restates gm::exp_ of
csrc/common/glsl_math.h (tests/test_denoise_model.py pins it to the oracle's orc_math(4, x)).

    denoise(color, hits, params) -> (H, W, 3) float32

color: (H, W, 3) float32, row 0 = bottom; hits: (H, W) HIT_DTYPE (the first-hit frame: a pixel is a
hit when triangle >= 0); params: anything with iterations, sigma_color, sigma_normal, sigma_plane
(rtamd.renderer.DenoiseParams).
"""
from __future__ import annotations

import numpy as np

F = np.float32
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))


def _exp2i(n):
    """2^n as a float for n in [-126, 127] (gm::exp2i_)"""
    return ((np.clip(n, -126, 127).astype(np.int64) + 127) << 23).astype(np.uint32).view(F)


def exp_(x) -> np.ndarray:
    x = np.atleast_1d(np.asarray(x, F))
    with np.errstate(all="ignore"):
        n = np.rint(x * F(1.44269504088896341))
        r = x - n * F(0.693359375)
        r = r - n * F(-2.12194440e-4)
        z = r * r
        y = (((((F(1.9875691500e-4) * r + F(1.3981999507e-3)) * r + F(8.3334519073e-3)) * r
               + F(4.1665795894e-2)) * r + F(1.6666665459e-1)) * r + F(5.0000001201e-1)) * z + r + F(1.0)
        ni = np.where(np.isfinite(n), n, F(0)).astype(np.int64)
        res = y * _exp2i(ni)
        res = np.where(ni > 127, (y * _exp2i(127)) * F(2.0), res)
        res = np.where(ni < -126, (y * _exp2i(ni + 64)) * _exp2i(-64), res)
        res = np.where(x < F(-103.972077083991796), F(0.0), res)
        res = np.where(x > F(88.72283905206835), F(np.inf), res)
        res = np.where(np.isnan(x), x, res)
    return res.astype(F)


def _shifted(a, s, dx, dy, fill):
    """a[y + s*dy, x + s*dx] per pixel (x, y), `fill` outside the frame"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, xs = s * dy, s * dx
    y0, y1 = max(0, -ys), min(H, H - ys)
    x0, x1 = max(0, -xs), min(W, W - xs)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + ys:y1 + ys, x0 + xs:x1 + xs]
    return out


def plant_nonfinite(color, hit, seed: int = 7, count: int = 12, n_inf: int = 3):
    """A copy of `color` with `count` non-finite pixels at seeded hit pixels: NaN in one channel, and
    +inf in all three for the first `n_inf`.  Returns (the copy, their (y, x) coordinates)."""
    rng = np.random.default_rng(seed)
    yx = np.argwhere(hit)
    yx = yx[rng.choice(len(yx), count, replace=False)]
    out = np.array(color, F)
    for k, (y, x) in enumerate(yx):
        if k < n_inf:
            out[y, x] = np.inf
        else:
            out[y, x, int(rng.integers(0, 3))] = np.nan
    return out, yx


def denoise(color, hits, params) -> np.ndarray:
    C = np.array(color, F)
    hit = hits["triangle"] >= 0
    M = np.where(hit, hits["material"], -1).astype(np.int32)
    N = np.ascontiguousarray(hits["normal"], F)
    P = np.ascontiguousarray(hits["point"], F)
    t = np.ascontiguousarray(hits["t"], F)
    sn, sp, sc = F(params.sigma_normal), F(params.sigma_plane), F(params.sigma_color)
    kn, kp, kc = F(1.0) / (sn * sn), F(1.0) / (sp * sp), F(1.0) / (sc * sc)
    with np.errstate(all="ignore"):
        it = np.where(t > 0, F(1.0) / t, F(0.0)).astype(F)
        for i in range(int(params.iterations)):
            s = 1 << i
            fin = np.isfinite(C).all(axis=-1)
            lum = (F(0.2126) * C[..., 0] + F(0.7152) * C[..., 1]) + F(0.0722) * C[..., 2]
            k = F(1.0) / (F(1.0) + np.fmax(lum, F(0.0)))
            G = C * k[..., None]
            acc = np.zeros_like(C)
            sw = np.zeros(C.shape[:2], F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    Cq, Gq = _shifted(C, s, dx, dy, 0), _shifted(G, s, dx, dy, 0)
                    Nq, Pq = _shifted(N, s, dx, dy, 0), _shifted(P, s, dx, dy, 0)
                    valid = hit & (_shifted(M, s, dx, dy, -1) == M) & _shifted(fin, s, dx, dy, False)
                    dn = N - Nq
                    dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                    dp = Pq - P
                    d = ((N[..., 0] * dp[..., 0] + N[..., 1] * dp[..., 1]) + N[..., 2] * dp[..., 2]) * it
                    dc = G - Gq
                    dc2 = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                    dc2 = np.where(fin, dc2, F(0.0))
                    e = (dn2 * kn + (d * d) * kp) + dc2 * kc
                    w = exp_(-e).reshape(e.shape) * (H5[dy + 2] * H5[dx + 2])
                    use = valid & (w > 0)
                    acc = np.where(use[..., None], acc + Cq * w[..., None], acc)
                    sw = np.where(use, sw + w, sw)
            done = hit & (sw > 0)
            C = np.where(done[..., None], acc / sw[..., None], C).astype(F)
            kc = kc * F(4.0)
    return C
