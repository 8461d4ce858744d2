// rt_geometry.h — the kernels of rt_update_geometry: new vertices for some triangles of the scene,
// everything derived from them recomputed on the device, both trees refitted.
//
// The definition is scn::update_geometry (csrc/common/scene_compile.h, CPU-tested); the kernels call
// the same per-triangle functions (tri_record, hit_record, trif::tri_rows, cull_tri, leaf_box,
// bnode_box, wnode_box), compiled for the device with the same -ffp-contract=off, so every array is
// the model's byte for byte as long as the device's fp64 / fp32 divide and square root are correctly
// rounded.  No render, trace, shade or query kernel reads anything new.
//
// Hand-off between workgroups happens at launch boundaries only: the leaves' boxes in one launch,
// then the internal nodes one height at a time (scn::refit_plan), a node reading boxes that earlier
// launches wrote.  The top heights, whose nodes fit one workgroup, share one single-workgroup
// launch with a workgroup barrier between heights.
#pragma once
#include <hip/hip_runtime.h>

#include "scene_compile.h"

namespace rtg {

// The check pass's result and the record pass's count.  The six doubles are kept as bit patterns:
// for non-negative doubles the unsigned order of the bits is the order of the values (+inf the
// largest), so a vector atomic max / min reduces them exactly.
struct Red {
  unsigned long long R, K, off, s_max, sc_max, c_min;
  int bad;         // some index is out of range or some value fails vertex_data_ok
  int flag_delta;  // change of tri_flagged
};

__device__ inline unsigned long long wave_max(unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ inline unsigned long long wave_min(unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ inline int wave_sum(int v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ inline unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }

// Validates the inputs (reads nothing else) and reduces the updated triangles' contributions to the
// culling bound and to the edge filter's extrema, in fp64 as the model computes them.
__global__ __launch_bounds__(256) void geo_check(const int* __restrict__ idx, int first, int count, int n_tri,
                                                 const float* __restrict__ p1, const float* __restrict__ p2,
                                                 const float* __restrict__ p3, const float* __restrict__ n1,
                                                 const float* __restrict__ n2, const float* __restrict__ n3, double s_cap,
                                                 double sc_cap, Red* __restrict__ red) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long R = 0, K = 0, off = 0, s_max = 0, sc_max = 0, c_min = dbits((double)INFINITY);
  int bad = 0;
  if (i < count) {
    const int t = idx ? idx[i] : first + i;
    float a[18];
    for (int j = 0; j < 3; j++) {
      a[j] = p1[3 * (size_t)i + j]; a[3 + j] = p2[3 * (size_t)i + j]; a[6 + j] = p3[3 * (size_t)i + j];
      a[9 + j] = n1[3 * (size_t)i + j]; a[12 + j] = n2[3 * (size_t)i + j]; a[15 + j] = n3[3 * (size_t)i + j];
    }
    if (t < 0 || t >= n_tri || !scn::vertex_data_ok(a, a + 3, a + 6, a + 9, a + 12, a + 15)) {
      bad = 1;
    } else {
      const scn::CullStats cs = scn::cull_tri(a, a + 3, a + 6);
      R = dbits(cs.R); K = dbits(cs.K); off = dbits(cs.off);
      float tri[12], trin[12], rows[12];
      scn::tri_record(a, a + 3, a + 6, a + 9, a + 12, a + 15, tri, trin);
      const trif::TriQ q = trif::tri_rows(tri, rows);
      if (trif::within_caps(q, s_cap, sc_cap)) { s_max = dbits(q.S); sc_max = dbits(q.sc); c_min = dbits(q.c); }
    }
  }
  R = wave_max(R); K = wave_max(K); off = wave_max(off);
  s_max = wave_max(s_max); sc_max = wave_max(sc_max); c_min = wave_min(c_min);
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&red->R, R); atomicMax(&red->K, K); atomicMax(&red->off, off);
    atomicMax(&red->s_max, s_max); atomicMax(&red->sc_max, sc_max); atomicMin(&red->c_min, c_min);
    if (bad) atomicOr(&red->bad, 1);
  }
}

// One lane per updated triangle (inputs checked by geo_check): its tri, trx, trin.xyz and hrec.
__global__ __launch_bounds__(256) void geo_record(const int* __restrict__ idx, int first, int count,
                                                  const float* __restrict__ p1, const float* __restrict__ p2,
                                                  const float* __restrict__ p3, const float* __restrict__ n1,
                                                  const float* __restrict__ n2, const float* __restrict__ n3, double s_cap,
                                                  double sc_cap, float4* __restrict__ tri_, float4* __restrict__ trx_,
                                                  float4* __restrict__ trin_, float4* __restrict__ hrec_,
                                                  Red* __restrict__ red) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int delta = 0;
  if (i < count) {
    const size_t t = (size_t)(idx ? idx[i] : first + i);
    float a[18], tri[12], trin[12], rows[12], h[24];
    for (int j = 0; j < 3; j++) {
      a[j] = p1[3 * (size_t)i + j]; a[3 + j] = p2[3 * (size_t)i + j]; a[6 + j] = p3[3 * (size_t)i + j];
      a[9 + j] = n1[3 * (size_t)i + j]; a[12 + j] = n2[3 * (size_t)i + j]; a[15 + j] = n3[3 * (size_t)i + j];
    }
    for (int k = 0; k < 3; k++) {
      const float4 o = tri_[3 * t + k], w = trin_[3 * t + k];
      tri[4 * k] = o.x; tri[4 * k + 1] = o.y; tri[4 * k + 2] = o.z; tri[4 * k + 3] = o.w;
      trin[4 * k] = w.x; trin[4 * k + 1] = w.y; trin[4 * k + 2] = w.z; trin[4 * k + 3] = w.w;
    }
    const bool was_flagged = !trif::within_caps(trif::tri_rows(tri, rows), s_cap, sc_cap);  // the old vertices' class
    scn::tri_record(a, a + 3, a + 6, a + 9, a + 12, a + 15, tri, trin);
    scn::hit_record(tri, trin, h);
    const bool flagged = !trif::within_caps(trif::tri_rows(tri, rows), s_cap, sc_cap);
    if (flagged) rows[4] = rows[5] = rows[6] = rows[8] = rows[9] = rows[10] = 0.0f;
    delta = (int)flagged - (int)was_flagged;
    for (int k = 0; k < 3; k++) {
      tri_[3 * t + k] = make_float4(tri[4 * k], tri[4 * k + 1], tri[4 * k + 2], tri[4 * k + 3]);
      trx_[3 * t + k] = make_float4(rows[4 * k], rows[4 * k + 1], rows[4 * k + 2], rows[4 * k + 3]);
      trin_[3 * t + k] = make_float4(trin[4 * k], trin[4 * k + 1], trin[4 * k + 2], trin[4 * k + 3]);
    }
    for (int k = 0; k < 6; k++) hrec_[8 * t + k] = make_float4(h[4 * k], h[4 * k + 1], h[4 * k + 2], h[4 * k + 3]);
  }
  delta = wave_sum(delta);
  if ((threadIdx.x & 63) == 0 && delta) atomicAdd(&red->flag_delta, delta);
}

// One lane per leaf: its box from the triangles, into its parent's side / slot in both trees.
__global__ __launch_bounds__(256) void geo_leaf(const int4* __restrict__ leaves, int n_leaves, const float4* __restrict__ tri,
                                                scn::BNode* __restrict__ nodes, scn::WNode* __restrict__ qnodes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_leaves) return;
  const int4 L = leaves[i];
  float lo[3], hi[3];
  scn::leaf_box(reinterpret_cast<const float*>(tri), L.x, lo, hi);
  if (L.y >= 0) {
    float* b = nodes[L.y >> 1].box + 6 * (L.y & 1);
    for (int a = 0; a < 3; a++) { b[a] = lo[a]; b[3 + a] = hi[a]; }
  }
  if (L.z >= 0) {
    scn::WNode& q = qnodes[L.z >> 2];
    const int s = L.z & 3;
    for (int a = 0; a < 3; a++) { q.lo[a][s] = lo[a]; q.hi[a][s] = hi[a]; }
  }
}

// Internal binary nodes of heights [h0, h1): each side that holds a node gets that node's box.
// Several workgroups: one height per launch (h1 = h0 + 1).  One workgroup: any number of heights,
// a barrier between them (the stores of a height are visible to the workgroup's own later loads).
__global__ __launch_bounds__(256) void geo_refit_b(scn::BNode* nodes, const int* __restrict__ list,
                                                   const int* __restrict__ off, int h0, int h1) {
  for (int h = h0; h < h1; h++) {
    const int end = off[h];
    for (int i = off[h - 1] + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += gridDim.x * blockDim.x) {
      scn::BNode& g = nodes[list[i]];
      for (int k = 0; k < 2; k++) {
        const int r = g.ref[k];
        if (scn::ref_is_leaf(r)) continue;
        float lo[3], hi[3];
        scn::bnode_box(nodes[r], lo, hi);
        for (int a = 0; a < 3; a++) { g.box[6 * k + a] = lo[a]; g.box[6 * k + 3 + a] = hi[a]; }
      }
    }
    if (h + 1 < h1) __syncthreads();
  }
}

// The same for the 4-wide tree: each slot that holds a node gets the union of that node's slots.
__global__ __launch_bounds__(256) void geo_refit_q(scn::WNode* qnodes, const int* __restrict__ list,
                                                   const int* __restrict__ off, int h0, int h1) {
  for (int h = h0; h < h1; h++) {
    const int end = off[h];
    for (int i = off[h - 1] + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += gridDim.x * blockDim.x) {
      scn::WNode& q = qnodes[list[i]];
      for (int k = 0; k < 4; k++) {
        const int r = q.ref[k];
        if (r == scn::Q_EMPTY || scn::ref_is_leaf(r)) continue;
        float lo[3], hi[3];
        scn::wnode_box(qnodes[r], lo, hi);
        for (int a = 0; a < 3; a++) { q.lo[a][k] = lo[a]; q.hi[a][k] = hi[a]; }
      }
    }
    if (h + 1 < h1) __syncthreads();
  }
}

}  // namespace rtg
