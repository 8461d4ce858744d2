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

__global__ __launch_bounds__(256) void tp_resolve(const TpCall T) {
  const int px = (int)blockIdx.x * kDnTW + ((int)threadIdx.x & 31), py = (int)blockIdx.y * kDnTH + ((int)threadIdx.x >> 5);
  if (px >= T.W || py >= T.H) return;
  const size_t pi = (size_t)py * (size_t)T.W + (size_t)px;
  const float4 c = T.cur[pi], a = T.g0[pi];
  const int M = __float_as_int(a.w);
  const bool fin = dn_finite(c);
  float r = c.x, g = c.y, b = c.z, n = 0.0f;  // a miss, or a non-finite input without history
  if (M != -1) {
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, sw = 0.0f;
    if (T.hc) {
      const float4 p = T.g1[pi];
      const float dx = p.x - T.pos[0], dy = p.y - T.pos[1], dz = p.z - T.pos[2];
      const float df = tp_dot(T.front, dx, dy, dz);
      if (df > 0.0f) {
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
              const float nx = a.x - aq.x, ny = a.y - aq.y, nz = a.z - aq.z;
              const float dn2 = (nx * nx + ny * ny) + nz * nz;
              const float qx_ = bq.x - p.x, qy_ = bq.y - p.y, qz_ = bq.z - p.z;
              const float d = ((a.x * qx_ + a.y * qy_) + a.z * qz_);
              if (cq.w > 0.0f && dn_finite(cq) && __float_as_int(aq.w) == M && dn2 <= T.sn2 && fabsf(d) * p.w <= T.sp) {
                sr = sr + cq.x * w;
                sg = sg + cq.y * w;
                sb = sb + cq.z * w;
                sn = sn + cq.w * w;
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
    } else if (fin) {
      n = min_(T.S, T.max_n);
    }
  }
  T.cand[pi] = make_float4(r, g, b, n);
  float* o = T.out3 + 3 * pi;
  o[0] = r; o[1] = g; o[2] = b;
}

}  // namespace rtd
