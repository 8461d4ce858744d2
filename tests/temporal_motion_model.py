"""The motion mode of the temporal stage (include/rt_abi.h rt_temporal_set_motion) in numpy fp32: the
model tp_resolve_motion of csrc/hip/rt_temporal.h is compared with bit for bit.

The static part is tests/temporal_model.py, unchanged: a pixel whose first-hit triangle moved
between the history's pose and the current one enters it with the history pose's surface point and
unit normal (Pq, Nq) in place of its own (P, N); a pixel whose `require` fails enters it with a NaN
point, which finds no history.  Every step is one fp32 operation in the order of DESIGN.md §4.

    t = MotionTemporal()
    out, n = t.call(color, hits, fp, tp, pose, advance=False, reset=False)

pose: (tri, trin), the scene's vertex records as rt_scene_download returns them ((3 n_tri, 4)
float32: texel 3 t + k holds vertex k of triangle t in xyz) at the time of the call.  After a call
t.moved is the mask of pixels that took the moved path and t.failed those whose require failed.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import temporal_model as tm

F = np.float32


def pose_of(p, n):
    """(tri, trin) from (n_tri, 3, 3) positions and normals (the .w words are not compared)"""
    p, n = np.asarray(p, F).reshape(-1, 3, 3), np.asarray(n, F).reshape(-1, 3, 3)
    tri = np.zeros((len(p) * 3, 4), F)
    trin = np.zeros((len(p) * 3, 4), F)
    tri[:, :3], trin[:, :3] = p.reshape(-1, 3), n.reshape(-1, 3)
    return tri, trin


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _bary(b1, a, b2, b, b3, c):
    return (b1[..., None] * a + b2[..., None] * b) + b3[..., None] * c


def reproject(g, T, cur, hist):
    """The guides g of the current view as the static stage must see them: (N', P', moved, failed)"""
    ctri, ctrin = (np.ascontiguousarray(a, F).reshape(-1, 3, 4)[..., :3] for a in cur)
    htri, htrin = (np.ascontiguousarray(a, F).reshape(-1, 3, 4)[..., :3] for a in hist)
    n_tri = len(ctri)
    N, P = g.N.copy(), g.P.copy()
    none = np.zeros(T.shape, bool)
    if n_tri == 0 or len(htri) != n_tri:
        return N, P, none, none
    valid = (g.M != -1) & (T >= 0) & (T < n_tri)
    t = np.clip(T, 0, n_tri - 1)
    p, n, q, m = ctri[t], ctrin[t], htri[t], htrin[t]          # (H, W, 3 vertices, 3)
    differs = (p.view(np.uint32) != q.view(np.uint32)).any((-1, -2)) | (n.view(np.uint32) != m.view(np.uint32)).any((-1, -2))
    moved = valid & differs
    with np.errstate(all="ignore"):
        e1, e2, v = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :], g.P - p[..., 0, :]
        d11, d12, d22, v1, v2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(v, e1), _dot(v, e2)
        den = d11 * d22 - d12 * d12
        b2 = (d22 * v1 - d12 * v2) / den
        b3 = (d11 * v2 - d12 * v1) / den
        b1 = (F(1.0) - b2) - b3
        f1, f2 = q[..., 1, :] - q[..., 0, :], q[..., 2, :] - q[..., 0, :]
        Pq = q[..., 0, :] + (b2[..., None] * f1 + b3[..., None] * f2)
        Nc = _bary(b1, n[..., 0, :], b2, n[..., 1, :], b3, n[..., 2, :])
        flip = _dot(g.N, Nc) < 0
        Nm = _bary(b1, m[..., 0, :], b2, m[..., 1, :], b3, m[..., 2, :])
        l = np.sqrt(_dot(Nm, Nm))
        Nq = Nm / l[..., None]
        Nq = np.where(flip[..., None], -Nq, Nq)
        ok = (den > 0) & np.isfinite(b1) & np.isfinite(b2) & np.isfinite(b3) & (l > 0) & np.isfinite(l)
    assert all(a.dtype == F for a in (den, b1, b2, b3, Pq, Nq, l))
    good, failed = moved & ok, moved & ~ok
    P[good], N[good] = Pq[good], Nq[good]
    P[failed] = np.nan   # d.front' > 0 fails: no history
    return N, P, moved, failed


class MotionTemporal(tm.Temporal):
    def drop(self):
        super().drop()
        self.moved = self.failed = None

    def call(self, color, hits, fp, tp, pose, advance=False, reset=False):
        if reset:
            self.hist = self.cand = None
        elif advance and self.cand is not None:
            self.hist = self.cand
        self.cand = None
        C = np.array(color, F)
        g = tm.guides(hits)
        seen = g
        self.moved = self.failed = np.zeros(C.shape[:2], bool)
        if self.hist is not None and self.hist.C.shape == C.shape:
            N, P, self.moved, self.failed = reproject(g, np.asarray(hits["triangle"], np.int64), pose, self.hist.pose)
            seen = SimpleNamespace(N=N, M=g.M, P=P, it=g.it)
        out, n = self._resolve(C, seen, tp)
        self.cand = SimpleNamespace(C=out, n=n, g=g, cam=tm._camera(fp), pose=tuple(np.array(a, F) for a in pose))
        return out.copy(), n.copy()
