// rt_denoise.h — the display denoiser (rt_abi.h rt_denoise*): a guided edge-avoiding a-trous wavelet
// filter (Dammertz et al. 2010) between the accumulation and the display pass.  No counterpart in
// the reference, which shows the raw accumulation (main.cpp:202-228).
//
//   dn_pack      once per pixel: the accumulation (float4, local-tile layout) or a caller's W*H*3
//                frame -> colour {r, g, b, k} in frame order, and (GUIDES) the rt_hit record of the
//                pixel (local-tile layout, as rt_first_hit_device writes it) -> the two guide
//                texels {N.xyz, bits(M or -1 for a miss)} and {P.xyz, 1/t}
//   dn_atrous_*  one iteration per launch, ping-pong between two colour frames; the last one
//                writes the W*H*3 output frame.  Its output stage computes k for the next.
//
// The arithmetic is fixed (tests/denoise_model.py restates it in numpy): every step
// is one correctly rounded fp32 operation in the order written in dn_tap / dn_store, taps run
// dy = -2..2 outer, dx = -2..2 inner, whatever the staging.  Two stagings:
//
//   dn_atrous_lds<STEP>  the block's 32 x 8 pixels plus a halo of 2*STEP in LDS, colour and
//                guides alike, read back with 16-byte reads.  A wave is two rows of 32 pixels and
//                every tap's offset is the same for all lanes, so each 16-lane group of a
//                ds_read_b128 ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...) lies in one row and reads
//                16 float4 whose indices are distinct mod 16: all 64 banks once, conflict-free for
//                any row pitch; the pitch is the staged width 32 + 4*STEP.  The staging stores go to
//                consecutive float4 per lane (8 contiguous lanes = 32 banks).  STEP = 1, 2 serve
//                s = 1, 2 (class stride 1); with class stride s the same kernel (STEP = 1) runs
//                one residue class (x mod s, y mod s) per block, where the taps are dense (s >= 8)
//   dn_atrous_direct  global reads of the 25 taps, served by L2 and the Infinity Cache (s = 4;
//                which form serves which s >= 4 was measured: rt_render.hip dn_far_lds)
//
// The variance mode (rt_abi.h rt_variance_*; tests/variance_model.py) runs dn_var_spatial once and
// then the *_var forms of the same two stagings for the same s: the colour term follows the variance
// of what is filtered, which every iteration carries on beside the colour.
#pragma once
#include "rt_device.h"

namespace rtd {

constexpr int kDnTW = 32, kDnTH = 8;  // pixels per block: a wave is two rows of 32

// An LDS texel as a native 4-float vector: a tap's read stays one ds_read_b128.  As a float4 (a
// struct) the compiler split a guide read into ds_read_b96 + ds_read_b32 and dropped the unused
// fourth word of the other (ds_read_b96): 22 LDS cycles per tap in place of 12
// (MI355X_MICROARCH §LDS: b96 8 cycles, b32 2, b128 4).  The launch times did not move (1080p,
// s = 1: 60.2 us either way): the kernel is bound by the taps' arithmetic, not by LDS.
typedef float dn_v4 __attribute__((ext_vector_type(4)));
RTD float4 dn_lds_get(const dn_v4* p, int i) {
  const dn_v4 v = p[i];
  return make_float4(v.x, v.y, v.z, v.w);
}
RTD void dn_lds_put(dn_v4* p, int i, float4 v) {
  dn_v4 t;
  t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
  p[i] = t;
}

struct DnIter {
  const float4* __restrict__ cin;   // {r, g, b, k} of the iteration's input
  float4* __restrict__ cout;        // the next iteration's input (out3 == nullptr)
  float* __restrict__ out3;         // the last iteration: W*H*3 floats
  const float4* __restrict__ g0;    // {N.xyz, bits(M or -1)}
  const float4* __restrict__ g1;    // {P.xyz, it}
  int W, H, s;
  float kn, kp, kc;
};

RTD bool dn_finite(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }

RTD float dn_k(float r, float g, float b) {
  const float lum = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
  return 1.0f / (1.0f + max_(lum, 0.0f));
}

RTD float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// What the variance forms read beside DnIter (rt_variance_set; DESIGN.md §4, tests/variance_model.py):
// the variance of the displayed luminance per pixel, -1 where it is unknown
struct DnVar {
  const float* __restrict__ vin;    // of the iteration's input
  float* __restrict__ vout;         // of its output
  float sl;                         // sigma_lum
};
constexpr float kVarEps = 1e-8f;    // keeps 0 * 1 / (sigma_lum * sqrt(0) + eps) = 0 on a constant frame

// The centre pixel p of a filter footprint
struct DnCentre {
  float4 c, a, b;   // colour, {N, M}, {P, it}
  f3 G;             // c.rgb * k
  bool fin;
  int M;
};

RTD DnCentre dn_centre(float4 c, float4 a, float4 b) {
  DnCentre p;
  p.c = c; p.a = a; p.b = b;
  p.G = mk3(c.x * c.w, c.y * c.w, c.z * c.w);
  p.fin = dn_finite(c);
  p.M = __float_as_int(a.w);
  return p;
}

// One tap q (already known to lie in the frame; a miss has M = -1 and never equals a hit's M)
RTD void dn_tap(const DnIter& I, const DnCentre& p, float4 cq, float4 aq, float4 bq, float hw, f3& sum, float& sw) {
  const float dnx = p.a.x - aq.x, dny = p.a.y - aq.y, dnz = p.a.z - aq.z;
  const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
  const float dpx = bq.x - p.b.x, dpy = bq.y - p.b.y, dpz = bq.z - p.b.z;
  const float d = ((p.a.x * dpx + p.a.y * dpy) + p.a.z * dpz) * p.b.w;
  const float dcx = p.G.x - cq.x * cq.w, dcy = p.G.y - cq.y * cq.w, dcz = p.G.z - cq.z * cq.w;
  const float dc2 = p.fin ? (dcx * dcx + dcy * dcy) + dcz * dcz : 0.0f;
  const float e = (dn2 * I.kn + (d * d) * I.kp) + dc2 * I.kc;
  const float w = exp_(-e) * hw;
  if (__float_as_int(aq.w) == p.M && dn_finite(cq) && w > 0.0f) {
    sum.x = sum.x + cq.x * w;
    sum.y = sum.y + cq.y * w;
    sum.z = sum.z + cq.z * w;
    sw = sw + w;
  }
}

RTD float dn_h(int k) { return k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f; }

// out[p]: sum / sw when any tap contributed, else the input colour, bits unchanged
RTD void dn_store(const DnIter& I, size_t q, const DnCentre& p, const f3& sum, float sw) {
  float r = p.c.x, g = p.c.y, b = p.c.z;
  if (sw > 0.0f) {
    r = sum.x / sw;
    g = sum.y / sw;
    b = sum.z / sw;
  }
  if (I.out3) {
    float* o = I.out3 + 3 * q;
    o[0] = r; o[1] = g; o[2] = b;
  } else {
    I.cout[q] = make_float4(r, g, b, dn_k(r, g, b));
  }
}

// The variance form's centre: its own variance vp (vm: known, the pixel takes the luminance term),
// its luminance and kl = 1 / (sigma_lum * sqrt(g) + eps), g the 3 x 3 Gaussian of the variance over
// the neighbours of the centre's material with a known one (dy = -1..1 outer, dx inner; global reads,
// whatever the staging of the taps)
struct DnVarCentre {
  float vp, lp, kl;
  bool vm;
};
RTD DnVarCentre dn_var_centre(const DnIter& I, const DnVar& V, const DnCentre& p, int px, int py) {
  DnVarCentre v;
  v.vp = V.vin[(size_t)py * (size_t)I.W + (size_t)px];
  v.vm = p.M != -1 && v.vp >= 0.0f;
  v.lp = dn_lum(p.c.x, p.c.y, p.c.z);
  v.kl = 0.0f;
  if (v.vm) {
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
      const int qy = py + dy;
      if (qy < 0 || qy >= I.H) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = px + dx;
        if (qx < 0 || qx >= I.W) continue;
        const size_t qi = (size_t)qy * (size_t)I.W + (size_t)qx;
        const float vq = V.vin[qi];
        const float w = (dy ? 0.25f : 0.5f) * (dx ? 0.25f : 0.5f);
        if (__float_as_int(I.g0[qi].w) == p.M && vq >= 0.0f) {
          gs = gs + vq * w;
          gw = gw + w;
        }
      }
    }
    v.kl = 1.0f / (V.sl * sqrtf(gs / gw) + kVarEps);
  }
  return v;
}

// dn_tap with the colour term |l_p - l_q| * kl where the centre's variance is known, and the tap's
// share of the output's variance
RTD void dn_tap_var(const DnIter& I, const DnCentre& p, const DnVarCentre& v, float4 cq, float4 aq, float4 bq, float vq, float hw,
                    f3& sum, float& sw, float& s2) {
  const float dnx = p.a.x - aq.x, dny = p.a.y - aq.y, dnz = p.a.z - aq.z;
  const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
  const float dpx = bq.x - p.b.x, dpy = bq.y - p.b.y, dpz = bq.z - p.b.z;
  const float d = ((p.a.x * dpx + p.a.y * dpy) + p.a.z * dpz) * p.b.w;
  float ec;
  if (v.vm) {
    ec = fabsf(v.lp - dn_lum(cq.x, cq.y, cq.z)) * v.kl;
  } else {
    const float dcx = p.G.x - cq.x * cq.w, dcy = p.G.y - cq.y * cq.w, dcz = p.G.z - cq.z * cq.w;
    ec = ((dcx * dcx + dcy * dcy) + dcz * dcz) * I.kc;
  }
  const float e = (dn2 * I.kn + (d * d) * I.kp) + (p.fin ? ec : 0.0f);
  const float w = exp_(-e) * hw;
  if (__float_as_int(aq.w) == p.M && dn_finite(cq) && w > 0.0f) {
    sum.x = sum.x + cq.x * w;
    sum.y = sum.y + cq.y * w;
    sum.z = sum.z + cq.z * w;
    sw = sw + w;
    if (vq >= 0.0f) s2 = s2 + (w * w) * vq;
  }
}

// dn_store, and the output's variance: sum(w^2 var_q) / sw^2 where the centre's was known and any
// tap contributed, else the centre's own
RTD void dn_store_var(const DnIter& I, const DnVar& V, size_t q, const DnCentre& p, const DnVarCentre& v, const f3& sum, float sw,
                      float s2) {
  dn_store(I, q, p, sum, sw);
  V.vout[q] = (sw > 0.0f && v.vm) ? s2 / (sw * sw) : v.vp;
}

// cs = 1: dense tiles, taps STEP apart (s = STEP).  cs = s (STEP = 1): blockIdx.z is the residue
// class (rx, ry) = (z % cs, z / cs) and the tile lies in the class's own coordinates,
// frame pixel = (rx + cs * cx, ry + cs * cy).
// VAR: the variance form stages one more float per texel in an LDS array of its own (a wave's
// ds_read_b32 of a tap is two rows of 32 consecutive floats: conflict-free) and leaves the 16-byte
// texels of sC, sA, sB and their conflict-free argument as they are
template <int STEP, bool VAR>
RTD void dn_atrous_lds_body(const DnIter& I, int cs, const DnVar* V) {
  constexpr int HALO = 2 * STEP, PW = kDnTW + 2 * HALO, PH = kDnTH + 2 * HALO;
  __shared__ dn_v4 sC[PH * PW], sA[PH * PW], sB[PH * PW];
  __shared__ float sV[VAR ? PH * PW : 1];
  // (the class is the slowest grid index: with rx fastest, so that the cs blocks that read the
  // same cache lines are dispatched together, 1080p took 0.62 ms instead of 0.41)
  const int rx = (int)blockIdx.z % cs, ry = (int)blockIdx.z / cs;
  const int Wc = (I.W - rx + cs - 1) / cs, Hc = (I.H - ry + cs - 1) / cs;  // the class's extent
  const int cx0 = (int)blockIdx.x * kDnTW, cy0 = (int)blockIdx.y * kDnTH;
  if (cx0 >= Wc || cy0 >= Hc) return;  // (block-uniform: a class smaller than class (0, 0))
  for (int i = (int)threadIdx.x; i < PH * PW; i += 256) {
    const int ly = i / PW, lx = i - ly * PW;
    const int cx = cx0 - HALO + lx, cy = cy0 - HALO + ly;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = c;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));  // outside the frame: never a source
    if (cx >= 0 && cy >= 0 && cx < Wc && cy < Hc) {
      const size_t q = (size_t)(ry + cs * cy) * (size_t)I.W + (size_t)(rx + cs * cx);
      c = I.cin[q];
      a = I.g0[q];
      b = I.g1[q];
      if (VAR) sV[i] = V->vin[q];
    } else if (VAR) {
      sV[i] = -1.0f;
    }
    dn_lds_put(sC, i, c);
    dn_lds_put(sA, i, a);
    dn_lds_put(sB, i, b);
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & 31, ly = (int)threadIdx.x >> 5;
  const int cx = cx0 + lx, cy = cy0 + ly;
  if (cx >= Wc || cy >= Hc) return;
  const int ci = (ly + HALO) * PW + lx + HALO;
  const DnCentre p = dn_centre(dn_lds_get(sC, ci), dn_lds_get(sA, ci), dn_lds_get(sB, ci));
  f3 sum = mk3(0.0f, 0.0f, 0.0f);
  float sw = 0.0f;
  if (VAR) {
    const int fx = rx + cs * cx, fy = ry + cs * cy;
    const DnVarCentre v = dn_var_centre(I, *V, p, fx, fy);
    float s2 = 0.0f;
    if (p.M != -1) {
#pragma unroll
      for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
          const int qi = ci + dy * STEP * PW + dx * STEP;
          dn_tap_var(I, p, v, dn_lds_get(sC, qi), dn_lds_get(sA, qi), dn_lds_get(sB, qi), sV[qi], dn_h(dy + 2) * dn_h(dx + 2), sum,
                     sw, s2);
        }
      }
    }
    dn_store_var(I, *V, (size_t)fy * (size_t)I.W + (size_t)fx, p, v, sum, sw, s2);
    return;
  }
  if (p.M != -1) {
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const int qi = ci + dy * STEP * PW + dx * STEP;
        dn_tap(I, p, dn_lds_get(sC, qi), dn_lds_get(sA, qi), dn_lds_get(sB, qi), dn_h(dy + 2) * dn_h(dx + 2), sum, sw);
      }
    }
  }
  dn_store(I, (size_t)(ry + cs * cy) * (size_t)I.W + (size_t)(rx + cs * cx), p, sum, sw);
}

template <int STEP>
__global__ __launch_bounds__(256) void dn_atrous_lds(const DnIter I, int cs) {
  dn_atrous_lds_body<STEP, false>(I, cs, nullptr);
}
template <int STEP>
__global__ __launch_bounds__(256) void dn_atrous_lds_var(const DnIter I, int cs, const DnVar V) {
  dn_atrous_lds_body<STEP, true>(I, cs, &V);
}

__global__ __launch_bounds__(256) void dn_atrous_direct(const DnIter I) {
  const int px = (int)blockIdx.x * kDnTW + ((int)threadIdx.x & 31), py = (int)blockIdx.y * kDnTH + ((int)threadIdx.x >> 5);
  if (px >= I.W || py >= I.H) return;
  const size_t pi = (size_t)py * (size_t)I.W + (size_t)px;
  const DnCentre p = dn_centre(I.cin[pi], I.g0[pi], I.g1[pi]);
  f3 sum = mk3(0.0f, 0.0f, 0.0f);
  float sw = 0.0f;
  if (p.M != -1) {
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
      const int qy = py + I.s * dy;
      if (qy < 0 || qy >= I.H) continue;
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const int qx = px + I.s * dx;
        if (qx < 0 || qx >= I.W) continue;
        const size_t qi = (size_t)qy * (size_t)I.W + (size_t)qx;
        dn_tap(I, p, I.cin[qi], I.g0[qi], I.g1[qi], dn_h(dy + 2) * dn_h(dx + 2), sum, sw);
      }
    }
  }
  dn_store(I, pi, p, sum, sw);
}

__global__ __launch_bounds__(256) void dn_atrous_direct_var(const DnIter I, const DnVar V) {
  const int px = (int)blockIdx.x * kDnTW + ((int)threadIdx.x & 31), py = (int)blockIdx.y * kDnTH + ((int)threadIdx.x >> 5);
  if (px >= I.W || py >= I.H) return;
  const size_t pi = (size_t)py * (size_t)I.W + (size_t)px;
  const DnCentre p = dn_centre(I.cin[pi], I.g0[pi], I.g1[pi]);
  const DnVarCentre v = dn_var_centre(I, V, p, px, py);
  f3 sum = mk3(0.0f, 0.0f, 0.0f);
  float sw = 0.0f, s2 = 0.0f;
  if (p.M != -1) {
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
      const int qy = py + I.s * dy;
      if (qy < 0 || qy >= I.H) continue;
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const int qx = px + I.s * dx;
        if (qx < 0 || qx >= I.W) continue;
        const size_t qi = (size_t)qy * (size_t)I.W + (size_t)qx;
        dn_tap_var(I, p, v, I.cin[qi], I.g0[qi], I.g1[qi], V.vin[qi], dn_h(dy + 2) * dn_h(dx + 2), sum, sw, s2);
      }
    }
  }
  dn_store_var(I, V, pi, p, v, sum, sw, s2);
}

// The spatial estimate of the variance mode, before the first iteration: vout = src (nullptr: all
// unknown), and where a hit pixel's is unknown the variance of luminance over the 7 x 7 neighbours
// on its surface (the centre's material, finite, |dN|^2 <= sn2, |N . dP| / t <= sp: the temporal
// stage's test), in one pass over the differences from the centre's luminance (0 when that is not
// finite); fewer than two such neighbours leave it unknown.  dy = -3..3 outer, dx inner.
__global__ __launch_bounds__(256) void dn_var_spatial(const DnIter I, const float* __restrict__ src, float* __restrict__ vout,
                                                      float sn2, float sp) {
  const int px = (int)blockIdx.x * kDnTW + ((int)threadIdx.x & 31), py = (int)blockIdx.y * kDnTH + ((int)threadIdx.x >> 5);
  if (px >= I.W || py >= I.H) return;
  const size_t pi = (size_t)py * (size_t)I.W + (size_t)px;
  float var = src ? src[pi] : -1.0f;
  const float4 a = I.g0[pi];
  const int M = __float_as_int(a.w);
  if (M != -1 && var < 0.0f) {
    const float4 c = I.cin[pi], b = I.g1[pi];
    const float ref = dn_finite(c) ? dn_lum(c.x, c.y, c.z) : 0.0f;
    float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
    for (int dy = -3; dy <= 3; dy++) {
      const int qy = py + dy;
      if (qy < 0 || qy >= I.H) continue;
#pragma unroll
      for (int dx = -3; dx <= 3; dx++) {
        const int qx = px + dx;
        if (qx < 0 || qx >= I.W) continue;
        const size_t qi = (size_t)qy * (size_t)I.W + (size_t)qx;
        const float4 cq = I.cin[qi], aq = I.g0[qi], bq = I.g1[qi];
        const float nx = a.x - aq.x, ny = a.y - aq.y, nz = a.z - aq.z;
        const float dn2 = (nx * nx + ny * ny) + nz * nz;
        const float qx_ = bq.x - b.x, qy_ = bq.y - b.y, qz_ = bq.z - b.z;
        const float d = (a.x * qx_ + a.y * qy_) + a.z * qz_;
        if (__float_as_int(aq.w) == M && dn_finite(cq) && dn2 <= sn2 && fabsf(d) * b.w <= sp) {
          const float dl = dn_lum(cq.x, cq.y, cq.z) - ref;
          s1 = s1 + dl;
          s2 = s2 + dl * dl;
          cnt = cnt + 1.0f;
        }
      }
    }
    if (cnt >= 2.0f) var = max_((s2 - (s1 * s1) / cnt) / (cnt - 1.0f), 0.0f);
  }
  vout[pi] = var;
}

// tiles: the accumulation (world == 1: local tile = global tile), or frame: W*H*3 floats.  hits:
// rt_hit records (three float4) in local-tile order; tile pixels outside the frame do not exist.
template <bool GUIDES>
__global__ __launch_bounds__(256) void dn_pack(const float4* __restrict__ tiles, const float* __restrict__ frame,
                                               const float4* __restrict__ hits, float4* __restrict__ col,
                                               float4* __restrict__ g0, float4* __restrict__ g1, int W, int H, int tile_w,
                                               int tile_h, int tiles_x) {
  const int px = (int)(blockIdx.x * blockDim.x + threadIdx.x), py = (int)blockIdx.y;
  if (px >= W || py >= H) return;
  const int tx = px / tile_w, ty = py / tile_h;
  const size_t ti = (size_t)(ty * tiles_x + tx) * (size_t)(tile_w * tile_h) + (size_t)(py - ty * tile_h) * tile_w + (px - tx * tile_w);
  const size_t pi = (size_t)py * (size_t)W + (size_t)px;
  float r, g, b;
  if (tiles) {
    const float4 v = tiles[ti];
    r = v.x; g = v.y; b = v.z;
  } else {
    const float* f = frame + 3 * pi;
    r = f[0]; g = f[1]; b = f[2];
  }
  col[pi] = make_float4(r, g, b, dn_k(r, g, b));
  if (GUIDES) {
    const float4 h0 = hits[3 * ti], h1 = hits[3 * ti + 1], h2 = hits[3 * ti + 2];
    const bool hit = __float_as_int(h2.x) >= 0;
    g0[pi] = make_float4(h1.x, h1.y, h1.z, hit ? h2.y : __int_as_float(-1));
    g1[pi] = make_float4(h0.y, h0.z, h0.w, h0.x > 0.0f ? 1.0f / h0.x : 0.0f);
  }
}

}  // namespace rtd
