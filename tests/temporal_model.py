"""The temporal stage of the displayed frame of include/rt_abi.h (rt_temporal) in numpy fp32: the model
the kernel of csrc/hip/rt_temporal.h is compared with bit for bit.

Every step is one correctly rounded fp32 operation in the order of DESIGN.md §4 (numpy float32
arithmetic is IEEE binary32 without contraction; there are no transcendentals and floor is exact).

    t = Temporal()                       the context's display history: none yet
    out, n = t.call(color, hits, fp, tp, advance=False, reset=False)

color: (H, W, 3) float32, row 0 = bottom; hits: (H, W) HIT_DTYPE (the first-hit frame of fp's camera: a
pixel is a hit when triangle >= 0); fp: anything with position, front, right, up, left_bottom_corner,
half_h, half_w (rtamd.renderer.FrameParams); tp: anything with samples, max_history, sigma_normal,
sigma_plane (rtamd.renderer.TemporalParams).  Returns the output frame and its history lengths
(rt_temporal_history).  After a call, t.taps is the number of counting taps per pixel (0..4) and
t.has the pixels that found a history.  drop() is what rt_resize and rt_set_scene do.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

F = np.float32


def guides(hits):
    """dn_pack's two guide texels: (N, M or -1 for a miss), (P, 1/t or 0)"""
    hit = hits["triangle"] >= 0
    M = np.where(hit, hits["material"], -1).astype(np.int32)
    N = np.ascontiguousarray(hits["normal"], F)
    P = np.ascontiguousarray(hits["point"], F)
    t = np.ascontiguousarray(hits["t"], F)
    with np.errstate(all="ignore"):
        it = np.where(t > 0, F(1.0) / t, F(0.0)).astype(F)
    return SimpleNamespace(N=N, M=M, P=P, it=it)


def _dot(v, x, y, z):
    return (v[0] * x + v[1] * y) + v[2] * z


def _camera(fp):
    v = lambda a: np.asarray(a, F)
    return SimpleNamespace(pos=v(fp.position), front=v(fp.front), right=v(fp.right), up=v(fp.up),
                           lbc=v(fp.left_bottom_corner), half_w=F(fp.half_w), half_h=F(fp.half_h))


class Temporal:
    def __init__(self):
        self.drop()

    def drop(self):
        self.hist = self.cand = None   # SimpleNamespace(C=colour, n=lengths, g=guides, cam=camera)
        self.taps = self.has = None

    def call(self, color, hits, fp, tp, advance=False, reset=False):
        if reset:
            self.hist = self.cand = None
        elif advance and self.cand is not None:
            self.hist = self.cand
        self.cand = None
        C = np.array(color, F)
        g = guides(hits)
        out, n = self._resolve(C, g, tp)
        self.cand = SimpleNamespace(C=out, n=n, g=g, cam=_camera(fp))
        return out.copy(), n.copy()

    def _resolve(self, C, g, tp):
        H, W = C.shape[:2]
        S, max_n = F(tp.samples), F(tp.max_history)
        sn2, sp = F(tp.sigma_normal) * F(tp.sigma_normal), F(tp.sigma_plane)
        hit = g.M != -1
        fin = np.isfinite(C).all(axis=-1)
        acc = np.zeros_like(C)
        sn = np.zeros((H, W), F)
        sw = np.zeros((H, W), F)
        taps = np.zeros((H, W), np.int32)
        h = self.hist
        if h is not None and h.C.shape == C.shape:
            cam = h.cam
            with np.errstate(all="ignore"):
                P = g.P
                dx, dy, dz = P[..., 0] - cam.pos[0], P[..., 1] - cam.pos[1], P[..., 2] - cam.pos[2]
                df = _dot(cam.front, dx, dy, dz)
                k = _dot(cam.front, cam.lbc[0], cam.lbc[1], cam.lbc[2]) / df
                ca = k * _dot(cam.right, dx, dy, dz) - _dot(cam.right, cam.lbc[0], cam.lbc[1], cam.lbc[2])
                cb = k * _dot(cam.up, dx, dy, dz) - _dot(cam.up, cam.lbc[0], cam.lbc[1], cam.lbc[2])
                x = (ca / (F(2.0) * cam.half_w)) * F(W) - F(0.5)
                y = (cb / (F(2.0) * cam.half_h)) * F(H) - F(0.5)
                inside = hit & (df > 0) & (x >= F(-1.0)) & (x < F(W)) & (y >= F(-1.0)) & (y < F(H))
                x, y = np.where(inside, x, F(0.0)), np.where(inside, y, F(0.0))
                fx, fy = np.floor(x), np.floor(y)
                x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
                wx1, wy1 = x - fx, y - fy
                wx0, wy0 = F(1.0) - wx1, F(1.0) - wy1
                hfin = np.isfinite(h.C).all(axis=-1)
                for j in range(2):
                    for i in range(2):
                        qx, qy = x0 + i, y0 + j
                        ok = inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                        qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                        Cq, nq, Nq, Pq, Mq = h.C[qy, qx], h.n[qy, qx], h.g.N[qy, qx], h.g.P[qy, qx], h.g.M[qy, qx]
                        w = (wx1 if i else wx0) * (wy1 if j else wy0)
                        dn = g.N - Nq
                        dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                        dp = Pq - P
                        d = (g.N[..., 0] * dp[..., 0] + g.N[..., 1] * dp[..., 1]) + g.N[..., 2] * dp[..., 2]
                        use = ok & (nq > 0) & hfin[qy, qx] & (Mq == g.M) & (dn2 <= sn2) & (np.abs(d) * g.it <= sp)
                        acc = np.where(use[..., None], acc + Cq * w[..., None], acc)
                        sn = np.where(use, sn + nq * w, sn)
                        sw = np.where(use, sw + w, sw)
                        taps += use
        has = hit & (sw > 0)
        with np.errstate(all="ignore"):
            hc, hn = acc / sw[..., None], sn / sw
            n_b = np.fmin(hn + S, max_n)
            al = np.fmin(S / n_b, F(1.0))
            blend = hc + al[..., None] * (C - hc)
        out = C.copy()
        n = np.zeros((H, W), F)
        a = has & fin
        out[a], n[a] = blend[a], n_b[a]
        b = has & ~fin
        out[b], n[b] = hc[b], hn[b]
        n[hit & ~has & fin] = np.fmin(S, max_n)
        self.taps, self.has = taps, has
        return out.astype(F), n.astype(F)
