// rt_query.h — ray queries on the wavefront traversal (rt_abi.h, ABI 7): hitBVH (RT:338-392) for
// rays of the caller's, and the camera pass's hit record (RT:1519-1527) per pixel.
//
// A query runs wf_trace itself (rt_wavefront.h), never a second traversal, over buffers of its own
// (rt_ctx::Query in rt_render.hip), one chunk of rays at a time:
//
//   wf_query_setup    caller rays {origin, dir} -> the trace's ray records, queue and count;
//                     malformed rays are answered here and never queued
//   wf_trace          <..., KIND = 1> closest hit / <..., KIND = 2> any hit over that queue, or the
//                     implicit camera queue <..., CAM> over wf_camera's table (first-hit frame)
//   wf_query_resolve  closest triangle per ray -> rt_hit with hit_geom's operations (the shade's),
//   wf_query_resolve_any  or the any-hit answer per ray
//   wf_query_camera   the camera rays themselves as rt_ray records (rt_camera_rays, rt_pick)
#pragma once
#include "rt_wavefront.h"

namespace rtd {

static_assert(sizeof(rt_ray) == 24 && sizeof(rt_hit) == 48, "rt_abi.h record sizes");

// Chunk-local ray i of n (6 floats each in `rays`) becomes path i of S: its record in ra / rb, the
// entry i << 1 | anyhit appended to queue[0] and counted in cnt[count_word] (zero at launch: the
// chunk's counter words, the segment claim counters among them, are cleared before it).  A ray
// with a non-finite component, an all-zero direction or an origin component beyond `bound` (the
// culling margin was derived for origins within it) is not queued: its result word gets
// RT_HIT_INVALID, which wf_trace never sees.
// A wave takes kSetupSpan consecutive rays per claim of queue space: one counter serves ~90
// atomics per us (rt_wavefront.h), and a claim per 64 rays made this kernel cost as much as the
// trace of its chunk (377 us per 2 Mi rays, profiles/query_bench_C3.md).
constexpr unsigned int kSetupIters = 16u, kSetupSpan = 64u * kSetupIters;
__global__ __launch_bounds__(256) void wf_query_setup(const WFState S, const float* __restrict__ rays, unsigned int n,
                                                      float bound, int anyhit, unsigned int count_word) {
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), waves = gridDim.x * (blockDim.x >> 6);
  for (unsigned int base = wave * kSetupSpan; base < n; base += waves * kSetupSpan) {  // (wave-uniform)
    unsigned long long valid[kSetupIters];
    unsigned int total = 0;
#pragma unroll
    for (unsigned int k = 0; k < kSetupIters; k++) {
      const unsigned int i = base + 64u * k + lane;
      bool ok = false;
      if (i < n) {
        const float* r = rays + 6 * (size_t)i;
        const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5];
        ok = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz) &&
             (dx != 0.0f || dy != 0.0f || dz != 0.0f) && fabsf(ox) <= bound && fabsf(oy) <= bound && fabsf(oz) <= bound;
        if (ok) {
          S.ra[i] = make_float4(ox, oy, oz, dx);
          S.rb[i] = make_float2(dy, dz);
        } else {
          S.res[2 * i + (unsigned)anyhit] = RT_HIT_INVALID;
        }
      }
      valid[k] = __ballot(ok);
      total += (unsigned int)__popcll(valid[k]);
    }
    unsigned int slot = 0;
    if (total) {
      if (lane == 0) slot = atomicAdd(&S.cnt[count_word], total);
      slot = (unsigned int)__shfl((int)slot, 0);
    }
#pragma unroll
    for (unsigned int k = 0; k < kSetupIters; k++) {
      if ((valid[k] >> lane) & 1ull)
        S.queue[0][slot + (unsigned int)__popcll(valid[k] & ((1ull << lane) - 1ull))] = (int)((base + 64u * k + lane) << 1) | anyhit;
      slot += (unsigned int)__popcll(valid[k]);
    }
  }
}

// The closest hits of a chunk as rt_hit records: three 16-B stores per ray.  CAM: work item i's
// camera ray (origin P.pos, direction S.cam[i]), stored at its accumulation index (local-tile
// layout); else path i's ray from ra / rb, stored at i.
template <bool CAM>
__global__ __launch_bounds__(256) void wf_query_resolve(const WFParams W, unsigned int n, float4* __restrict__ out) {
  const KParams& P = W.K;
  const WFState& S = W.S;
  for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int tri = S.res[2 * i];
    // a miss (-1) or an untraced ray (RT_HIT_INVALID): t = -1, every other field +0
    float4 h0 = make_float4(-1.0f, 0.0f, 0.0f, 0.0f), h1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int mat = 0;
    if (tri >= 0) {
      f3 ro, rd;
      if (CAM) {
        ro = mk3(P.pos[0], P.pos[1], P.pos[2]);
        rd = xyz(S.cam[i]);
      } else {
        const float4 a = S.ra[i];
        const float2 b = S.rb[i];
        ro = xyz(a);
        rd = mk3(a.w, b.x, b.y);
      }
      const HitGeom h = hit_geom(P, tri, ro, rd);
      const f3 hN = h.inside ? -h.Ns : h.Ns;  // RT:256-259
      h0 = make_float4(h.t - 0.00001f, h.Pp.x, h.Pp.y, h.Pp.z);  // RT:284
      h1 = make_float4(hN.x, hN.y, hN.z, __int_as_float(h.inside ? 1 : 0));
      mat = h.nmat;
    }
    float4* o = out + 3 * (size_t)(CAM ? S.pix_acc[i] : i);
    o[0] = h0;
    o[1] = h1;
    o[2] = make_float4(__int_as_float(tri), __int_as_float(mat), 0.0f, 0.0f);
  }
}

// The any-hit answers of a chunk: 1 occluded, 0 not, RT_HIT_INVALID untraced
__global__ __launch_bounds__(256) void wf_query_resolve_any(const WFState S, unsigned int n, int* __restrict__ out) {
  for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int r = S.res[2 * i + 1];
    out[i] = r >= 0 ? 1 : r == -1 ? 0 : RT_HIT_INVALID;
  }
}

// Camera rays as rt_ray records (6 floats): origin P.pos, direction camera_dir's.  Work item w of
// the pixel list goes to record pix_acc[w] (local-tile layout); with no list, the one pixel
// `xy_one` goes to record 0 (rt_pick).
__global__ __launch_bounds__(256) void wf_query_camera(const KParams P, const unsigned int* __restrict__ pix_xy,
                                                       const unsigned int* __restrict__ pix_acc, unsigned int n,
                                                       unsigned int xy_one, float* __restrict__ out) {
  const f3 lbc = mk3(P.lbc[0], P.lbc[1], P.lbc[2]);
  const f3 right = mk3(P.right[0], P.right[1], P.right[2]);
  const f3 up = mk3(P.up[0], P.up[1], P.up[2]);
  for (unsigned int w = blockIdx.x * blockDim.x + threadIdx.x; w < n; w += gridDim.x * blockDim.x) {
    const float4 d = camera_dir(P, lbc, right, up, pix_xy ? pix_xy[w] : xy_one);
    float* o = out + 6 * (size_t)(pix_xy ? pix_acc[w] : w);
    o[0] = P.pos[0]; o[1] = P.pos[1]; o[2] = P.pos[2];
    o[3] = d.x; o[4] = d.y; o[5] = d.z;
  }
}

}  // namespace rtd
