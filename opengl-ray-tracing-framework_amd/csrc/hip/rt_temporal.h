// rt_temporal.h — temporal accumulation of the displayed frame (rt_abi.h rt_temporal*): the display
// history of the previous view, reprojected into the current one through the first-hit frame,
// tested for being the same surface and blended with the current input by sample counts.  It
// sits between the accumulation and the denoiser (rt_denoise.h) or the display pass; no
// counterpart in the reference, whose LoopNum = 0 starts the image again from nothing
// (main.cpp:326).
//
//   dn_pack      (rt_denoise.h) the current view's colour {r, g, b, k} and guide texels
//                {N.xyz, bits(M or -1)}, {P.xyz, 1/t} in frame order; k is not used here
//   tp_resolve   one lane per pixel, blocks of 32 x 8 pixels as the denoiser's, so the four taps of
//                a wave's two rows fall on a few neighbouring lines of the history.  Every texel is
//                one 16-byte read: the history {r, g, b, n} and its two guide texels.  The tap
//                addresses differ per lane (they follow the surface), so there is no staging in
//                LDS: the 2 x 2 footprints of neighbouring lanes overlap and L2 serves them.
//                Writes the candidate {r, g, b, n_out} and the W*H*3 output frame in the same pass.
//
//   tp_resolve_var, tp_resolve_motion_var   the same body in the variance mode (rt_variance_set): one
//                more 16-byte texel {l_prev, S_prev, v, m} per history tap and per output pixel, and
//                the variance of the displayed luminance as a W*H frame (tests/variance_model.py)
//
// The arithmetic is fixed (tests/temporal_model.py restates it in numpy): every
// step is one correctly rounded fp32 operation in the order written below; taps run j = 0..1
// outer (rows), i = 0..1 inner.  There are no transcendentals, and floor is exact.
//
// The projection is the inverse of camera_dir (rt_wavefront.h) under the assumption that the
// history camera's front, right and up are unit length and orthogonal, as Camera.h:160-174
// produces them: then lbc + a * right + b * up has the components (lbc.front, lbc.right + a,
// lbc.up + b) in that basis, and a point at d = P - position with d.front > 0 lies on the ray
// of (a, b) = k * (d.right, d.up) - (lbc.right, lbc.up), k = lbc.front / d.front.
#pragma once
#include "rt_denoise.h"

namespace rtd {

struct TpCall {
  const float4* __restrict__ cur;   // dn_pack's colour of the current input {r, g, b, k}
  const float4* __restrict__ g0;    // the current guides
  const float4* __restrict__ g1;
  const float4* __restrict__ hc;    // the history {r, g, b, n}; nullptr: none
  const float4* __restrict__ hg0;   // its guides
  const float4* __restrict__ hg1;
  float4* __restrict__ cand;        // this call's {r, g, b, n_out}
  float* __restrict__ out3;         // this call's W*H*3 output frame
  int W, H;
  float pos[3], front[3], right[3], up[3], lbc[3];  // the history camera
  float tw, th;                     // 2 * half_w, 2 * half_h of it
  float S, max_n;                   // samples of the input, cap of the history length
  float sn2, sp;                    // sigma_normal^2, sigma_plane
};

RTD float tp_dot(const float* a, float x, float y, float z) { return (a[0] * x + a[1] * y) + a[2] * z; }

// What the motion form reads beside TpCall (rt_temporal_set_motion): the current
// pixels' triangle indices and the vertex records {p_k, .}, {n_k, .} (3 float4 per triangle each) of
// the current pose and of the pose the history was made from
struct TpMotion {
  const int* __restrict__ tf;         // the current guides' triangle frame: T, or -1 for a miss
  const float4* __restrict__ tri;     // the current pose
  const float4* __restrict__ trin;
  const float4* __restrict__ htri;    // the history's pose
  const float4* __restrict__ htrin;
  int n_tri;
};

struct TpV3 {
  float x, y, z;
};
RTD TpV3 tp_v3(const float4 a) { return TpV3{a.x, a.y, a.z}; }
RTD TpV3 tp_sub(const TpV3 a, const TpV3 b) { return TpV3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RTD float tp_dot3(const TpV3 a, const TpV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RTD TpV3 tp_bary(float b1, const TpV3 a, float b2, const TpV3 b, float b3, const TpV3 c) {
  return TpV3{(b1 * a.x + b2 * b.x) + b3 * c.x, (b1 * a.y + b2 * b.y) + b3 * c.y, (b1 * a.z + b2 * b.z) + b3 * c.z};
}
RTD int tp_diff(const float4 a, const float4 b) {  // xyz, bitwise
  return (__float_as_int(a.x) ^ __float_as_int(b.x)) | (__float_as_int(a.y) ^ __float_as_int(b.y)) |
         (__float_as_int(a.z) ^ __float_as_int(b.z));
}

// The surface point P of triangle t (first-hit normal N) as the history's pose had it: false when t is
// no triangle of the list or none of its 18 floats moved (P, N stay: today's arithmetic).  Otherwise
// P, N become the point with P's barycentrics and its interpolated unit normal in the history's pose,
// N on the side of the surface the hit normal is on; ok = false when a `require` fails (no history).
RTD bool tp_moved(const TpMotion& m, int t, TpV3& P, TpV3& N, bool& ok) {
  if ((unsigned)t >= (unsigned)m.n_tri) return false;
  const size_t at = 3 * (size_t)t;
  const float4 cp1 = m.tri[at], cp2 = m.tri[at + 1], cp3 = m.tri[at + 2];
  const float4 cn1 = m.trin[at], cn2 = m.trin[at + 1], cn3 = m.trin[at + 2];
  const float4 hp1 = m.htri[at], hp2 = m.htri[at + 1], hp3 = m.htri[at + 2];
  const float4 hn1 = m.htrin[at], hn2 = m.htrin[at + 1], hn3 = m.htrin[at + 2];
  if (!(tp_diff(cp1, hp1) | tp_diff(cp2, hp2) | tp_diff(cp3, hp3) | tp_diff(cn1, hn1) | tp_diff(cn2, hn2) | tp_diff(cn3, hn3)))
    return false;
  ok = false;
  const TpV3 p1 = tp_v3(cp1), q1 = tp_v3(hp1);
  const TpV3 e1 = tp_sub(tp_v3(cp2), p1), e2 = tp_sub(tp_v3(cp3), p1), v = tp_sub(P, p1);
  const float d11 = tp_dot3(e1, e1), d12 = tp_dot3(e1, e2), d22 = tp_dot3(e2, e2), v1 = tp_dot3(v, e1), v2 = tp_dot3(v, e2);
  const float den = d11 * d22 - d12 * d12;
  if (!(den > 0.0f)) return true;
  const float b2 = (d22 * v1 - d12 * v2) / den, b3 = (d11 * v2 - d12 * v1) / den, b1 = (1.0f - b2) - b3;
  if (!(isfinite(b1) && isfinite(b2) && isfinite(b3))) return true;
  const TpV3 f1 = tp_sub(tp_v3(hp2), q1), f2 = tp_sub(tp_v3(hp3), q1);
  const TpV3 Pq{q1.x + (b2 * f1.x + b3 * f2.x), q1.y + (b2 * f1.y + b3 * f2.y), q1.z + (b2 * f1.z + b3 * f2.z)};
  const TpV3 Nc = tp_bary(b1, tp_v3(cn1), b2, tp_v3(cn2), b3, tp_v3(cn3));
  const bool flip = tp_dot3(N, Nc) < 0.0f;
  const TpV3 Nm = tp_bary(b1, tp_v3(hn1), b2, tp_v3(hn2), b3, tp_v3(hn3));
  const float l = sqrtf(tp_dot3(Nm, Nm));
  if (!(l > 0.0f && isfinite(l))) return true;
  const TpV3 Nq{Nm.x / l, Nm.y / l, Nm.z / l};
  P = Pq;
  N = flip ? TpV3{-Nq.x, -Nq.y, -Nq.z} : Nq;
  ok = true;
  return true;
}

// What the variance forms read and write beside TpCall (rt_variance_set; DESIGN.md §4,
// tests/variance_model.py): one state texel {l_prev, S_prev, v, m} beside each {r, g, b, n} texel of
// the history and of the candidate: the luminance and sample count of the last input seen for the
// view, the running mean of the per-sample luminance variance estimates and their number
struct TpVar {
  const float4* __restrict__ hst;   // the history's state texels (read where hc is)
  float4* st;                       // the candidate's: read first when `own`, then written
  float* __restrict__ var;          // this call's variance of the displayed luminance; -1: unknown
  int own;                          // st holds the previous call's state of the same view (no ADVANCE since)
  float max_m;                      // cap of m
};

// MOTION = false is tp_resolve as it always was; with MOTION a pixel of a moved triangle enters the
// same statements with the history pose's P and N in place of its own.  VAR adds the variance
// state: v and m ride the colour's taps, and the tail below the blend updates them.
template <bool MOTION, bool VAR>
RTD void tp_resolve_px(const TpCall& T, const TpMotion* mo, const TpVar* V) {
  const int px = (int)blockIdx.x * kDnTW + ((int)threadIdx.x & 31), py = (int)blockIdx.y * kDnTH + ((int)threadIdx.x >> 5);
  if (px >= T.W || py >= T.H) return;
  const size_t pi = (size_t)py * (size_t)T.W + (size_t)px;
  const float4 c = T.cur[pi], a = T.g0[pi];
  const int M = __float_as_int(a.w);
  const bool fin = dn_finite(c);
  float r = c.x, g = c.y, b = c.z, n = 0.0f;  // a miss, or a non-finite input without history
  float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (VAR) a miss keeps no state
  float var = -1.0f;
  if (M != -1) {
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, sw = 0.0f;
    float sv = 0.0f, sm = 0.0f, lh = 0.0f, hn_ = 0.0f;  // (VAR)
    if (T.hc) {
      const float4 p = T.g1[pi];
      TpV3 P{p.x, p.y, p.z}, N{a.x, a.y, a.z};
      bool ok = true;
      if (MOTION) tp_moved(*mo, mo->tf[pi], P, N, ok);
      const float dx = P.x - T.pos[0], dy = P.y - T.pos[1], dz = P.z - T.pos[2];
      const float df = tp_dot(T.front, dx, dy, dz);
      if (ok && df > 0.0f) {
        const float k = tp_dot(T.front, T.lbc[0], T.lbc[1], T.lbc[2]) / df;
        const float ca = k * tp_dot(T.right, dx, dy, dz) - tp_dot(T.right, T.lbc[0], T.lbc[1], T.lbc[2]);
        const float cb = k * tp_dot(T.up, dx, dy, dz) - tp_dot(T.up, T.lbc[0], T.lbc[1], T.lbc[2]);
        const float x = (ca / T.tw) * (float)T.W - 0.5f;
        const float y = (cb / T.th) * (float)T.H - 0.5f;
        // (a NaN fails the comparisons; inside them the conversions to int are exact)
        if (x >= -1.0f && x < (float)T.W && y >= -1.0f && y < (float)T.H) {
          const float fx = floorf(x), fy = floorf(y);
          const int x0 = (int)fx, y0 = (int)fy;
          const float wx1 = x - fx, wy1 = y - fy;
          const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const int qy = y0 + j;
            if (qy < 0 || qy >= T.H) continue;
#pragma unroll
            for (int i = 0; i < 2; i++) {
              const int qx = x0 + i;
              if (qx < 0 || qx >= T.W) continue;
              const size_t qi = (size_t)qy * (size_t)T.W + (size_t)qx;
              const float4 cq = T.hc[qi], aq = T.hg0[qi], bq = T.hg1[qi];
              const float w = (i ? wx1 : wx0) * (j ? wy1 : wy0);
              const float nx = N.x - aq.x, ny = N.y - aq.y, nz = N.z - aq.z;
              const float dn2 = (nx * nx + ny * ny) + nz * nz;
              const float qx_ = bq.x - P.x, qy_ = bq.y - P.y, qz_ = bq.z - P.z;
              const float d = ((N.x * qx_ + N.y * qy_) + N.z * qz_);
              if (cq.w > 0.0f && dn_finite(cq) && __float_as_int(aq.w) == M && dn2 <= T.sn2 && fabsf(d) * p.w <= T.sp) {
                sr = sr + cq.x * w;
                sg = sg + cq.y * w;
                sb = sb + cq.z * w;
                sn = sn + cq.w * w;
                if (VAR) {
                  const float4 sq = V->hst[qi];
                  sv = sv + sq.z * w;
                  sm = sm + sq.w * w;
                }
                sw = sw + w;
              }
            }
          }
        }
      }
    }
    if (sw > 0.0f) {
      const float hr = sr / sw, hg = sg / sw, hb = sb / sw, hn = sn / sw;
      if (fin) {
        n = min_(hn + T.S, T.max_n);
        const float al = min_(T.S / n, 1.0f);
        r = hr + al * (c.x - hr);
        g = hg + al * (c.y - hg);
        b = hb + al * (c.z - hb);
      } else {
        r = hr; g = hg; b = hb; n = hn;
      }
      if (VAR) {
        lh = dn_lum(hr, hg, hb);
        hn_ = hn;
      }
    } else if (fin) {
      n = min_(T.S, T.max_n);
    }
    if (VAR) {
      // One estimate e of the per-sample variance, a squared difference of two independent means:
      // the still view's new samples against its earlier ones (Welford's chunk-merge term), or
      // this input against the reprojected history
      const float lc = dn_lum(c.x, c.y, c.z);
      float lp = 0.0f, Sp = 0.0f, v0, m0, e;
      bool upd;
      if (V->own) {
        const float4 o = V->st[pi];
        lp = o.x; Sp = o.y; v0 = o.z; m0 = o.w;
        const float dS = T.S - Sp;
        const float s = (T.S * lc - Sp * lp) / dS;
        const float d = s - lp;
        e = (d * d) * ((dS * Sp) / T.S);
        upd = fin && T.S > Sp && Sp > 0.0f;
      } else {
        const bool has = sw > 0.0f;
        v0 = has ? sv / sw : 0.0f;
        m0 = has ? sm / sw : 0.0f;
        const float d = lc - lh;
        e = (d * d) / (1.0f / T.S + 1.0f / hn_);
        upd = has && fin;
      }
      upd = upd && isfinite(e);
      const float m1 = m0 + 1.0f;
      const float v1 = v0 + (e - v0) / m1;
      st = make_float4(fin ? lc : lp, fin ? T.S : Sp, upd ? v1 : v0, upd ? min_(m1, V->max_m) : m0);
      if (st.w > 0.0f) var = st.z / max_(n, T.S);
    }
  }
  T.cand[pi] = make_float4(r, g, b, n);
  float* o = T.out3 + 3 * pi;
  o[0] = r; o[1] = g; o[2] = b;
  if (VAR) {
    V->st[pi] = st;
    V->var[pi] = var;
  }
}

__global__ __launch_bounds__(256) void tp_resolve(const TpCall T) { tp_resolve_px<false, false>(T, nullptr, nullptr); }
__global__ __launch_bounds__(256) void tp_resolve_motion(const TpCall T, const TpMotion Mo) {
  tp_resolve_px<true, false>(T, &Mo, nullptr);
}
__global__ __launch_bounds__(256) void tp_resolve_var(const TpCall T, const TpVar V) { tp_resolve_px<false, true>(T, nullptr, &V); }
__global__ __launch_bounds__(256) void tp_resolve_motion_var(const TpCall T, const TpMotion Mo, const TpVar V) {
  tp_resolve_px<true, true>(T, &Mo, &V);
}

// The triangle frame of a fresh pack on a context in motion mode (the guide texels do not hold the
// triangle index): T of the rt_hit records in local-tile order, or -1 for a miss, in frame order
__global__ __launch_bounds__(256) void tp_pack_tri(const float4* __restrict__ hits, int* __restrict__ tf, int W, int H,
                                                   int tile_w, int tile_h, int tiles_x) {
  const int px = (int)(blockIdx.x * blockDim.x + threadIdx.x), py = (int)blockIdx.y;
  if (px >= W || py >= H) return;
  const int tx = px / tile_w, ty = py / tile_h;
  const size_t ti = (size_t)(ty * tiles_x + tx) * (size_t)(tile_w * tile_h) + (size_t)(py - ty * tile_h) * tile_w + (px - tx * tile_w);
  const int t = __float_as_int(hits[3 * ti + 2].x);
  tf[(size_t)py * (size_t)W + (size_t)px] = t >= 0 ? t : -1;
}

}  // namespace rtd
