// dev_layout.h — where every array of the carved device allocations lives (host side, HIP-free).
//
// rt_render.hip allocates a few large blocks and hands their memory out to many arrays: the path
// state of the frame groups, the row arena that aliases part of it, the query buffers, the display
// denoiser's and the display history's frames, the frame table and the camera table.  Each layout
// below is one list: the offsets and the size to allocate come from the same add() calls, and the
// .hip file assigns base + offset.  No HIP type is visible here, so the layouts work in byte (or
// element) offsets and in element sizes that rt_render.hip ties to the kernels' types with
// static_asserts.  tests/test_dev_layout.py checks them on the CPU through rts_dev_layout
// (rt_scene.h).
#pragma once
#include <algorithm>
#include <cstddef>

namespace dvl {

// One array of an allocation: where it starts and the bytes (or elements) it holds
struct Span {
  size_t off = 0, bytes = 0;
};
// Spans of one allocation: every array starts on a 256-B boundary
struct Builder {
  size_t at = 0;
  Span add(size_t bytes) {
    const Span s{at, bytes};
    at += (bytes + 255) & ~size_t(255);
    return s;
  }
  size_t total() const { return at; }
};

// ---- path state (rtd::WFState of one frame group, rt_ctx::wfg) -----------------------------------
// The arrays with one element per path slot, in allocation order.  `bytes` is per slot; `lean_live`:
// a lean group (WFParams::p1_lean) still reads or writes the array from pass 1 on.  Not so s1 (every
// kept path is PF_ZLO) and s5, rb, sb (pass 1 has no s5 row and 16-B rays): the row arena may alias
// those four and nothing else.
enum Slot { S0, S1, S2, S3, S4, S5, RA, RB, SA, SB, RES, FIN, QUEUE0, QUEUE1, ACTIVE0, ACTIVE1, kSlotArrays };
struct SlotArray {
  const char* name;
  size_t bytes;
  bool lean_live;
};
constexpr SlotArray kSlot[kSlotArrays] = {
    {"s0", 16, true},    {"s1", 16, false},   {"s2", 16, true},     {"s3", 16, true},
    {"s4", 16, true},    {"s5", 8, false},    {"ra", 16, true},     {"rb", 8, false},
    {"sa", 16, true},    {"sb", 8, false},    {"res", 2 * 4, true}, {"fin", 16, true},
    // a queue holds two entries per slot: the split queues' shadow half (queue_s) is its upper half
    {"queue0", 2 * 4, true}, {"queue1", 2 * 4, true}, {"active0", 4, true}, {"active1", 4, true}};
constexpr size_t kCntWords = 672;  // rtd::kCntWords: the counter words of a set (WFState::cnt)

constexpr size_t slot_bytes() {
  size_t b = 0;
  for (const SlotArray& a : kSlot) b += a.bytes;
  return b;
}

// One set's arrays at arr[], queue_s[], hit, cnt from set(g); `slots` is the clamped size
struct PathState {
  size_t slots = 0, hit_cap = 0;
  Span arr[kSlotArrays], queue_s[2], hit, cnt;
  size_t set_bytes = 0, total = 0;
  size_t set(int g) const { return (size_t)g * set_bytes; }
};
inline PathState path_state(size_t paths, int n_groups) {
  PathState L;
  const size_t P = L.slots = std::max<size_t>(paths, 64);
  // the hit-pixel list: one entry per work item of a group of >= 64 frames (wf_cam_classify)
  L.hit_cap = P / 64 + 64;
  Builder b;
  for (int i = 0; i < kSlotArrays; i++) L.arr[i] = b.add(P * kSlot[i].bytes);
  for (int k = 0; k < 2; k++) L.queue_s[k] = Span{L.arr[QUEUE0 + k].off + P * 4, P * 4};
  L.hit = b.add(L.hit_cap * 4);
  L.cnt = b.add(kCntWords * 4);
  L.set_bytes = b.total();
  L.total = L.set_bytes * (size_t)n_groups;
  return L;
}

// ---- row arena (WFParams::A, rt_ctx::wfa) --------------------------------------------------------
// The state of passes >= 2 of a lean group in dense rows, one per path that survives pass 1.  A set
// has a quarter of its slots as rows (C3 keeps about 11 % of them after pass 1, C4's glass view
// nearly half: that one falls back), in whole groups of 4 rows.  A quarter is the largest share that
// needs no memory of its own: each arena array starts off * rows bytes into the slot array `host`,
// which the group has stopped using by then, and a group on the arena touches no slot array but fin.
inline constexpr size_t arena_rows(size_t slots) { return slots / 4 & ~size_t(3); }

enum Row { A_S0, A_S1, A_S2, A_S3, A_S4, A_S5, A_RA, A_RB, A_SA, A_SB, A_RES, A_RPATH, kArenaArrays };
struct ArenaArray {
  const char* name;
  size_t bytes;  // per row
  Slot host;
  size_t off;  // in units of rows
};
constexpr ArenaArray kArena[kArenaArrays] = {
    {"s0", 16, S1, 0},  {"s1", 16, S1, 16}, {"s2", 16, S1, 32}, {"s3", 16, S1, 48},
    {"s4", 16, S5, 0},  {"s5", 8, RB, 16},  {"ra", 16, S5, 16}, {"rb", 8, RB, 24},
    {"sa", 16, RB, 0},  {"sb", 8, SB, 0},   {"res", 2 * 4, SB, 8}, {"rpath", 4, SB, 16}};

constexpr size_t row_bytes() {
  size_t b = 0;
  for (const ArenaArray& a : kArena) b += a.bytes;
  return b;
}
// rows <= slots / 4 and a multiple of 4: what each host array can take, and 16-B starts
constexpr bool arena_fits() {
  for (const ArenaArray& a : kArena) {
    if (kSlot[a.host].lean_live) return false;
    if (a.off + a.bytes > 4 * kSlot[a.host].bytes) return false;
    if (a.off * 4 % 16) return false;
    for (const ArenaArray& o : kArena)
      if (&o != &a && o.host == a.host && o.off < a.off + a.bytes && a.off < o.off + o.bytes) return false;
  }
  return true;
}
static_assert(arena_fits(), "the row arena's arrays fit the slot arrays a lean group has stopped using");

struct Arena {
  size_t rows = 0;
  Span arr[kArenaArrays];  // from the set's start, as PathState::arr
};
inline Arena arena(const PathState& L) {
  Arena A;
  A.rows = arena_rows(L.slots);
  for (int i = 0; i < kArenaArrays; i++) {
    const ArenaArray& a = kArena[i];
    A.arr[i] = Span{L.arr[a.host].off + a.off * A.rows, a.bytes * A.rows};
  }
  return A;
}

// ---- ray queries (rt_ctx::Query) -----------------------------------------------------------------
// One chunk of rays: the 24-B ray records (ra / rb; one kind of ray per chunk, so sa / sb and cam
// alias them), one queue, the result words, the staged caller rays (rt_ray) and results (rt_hit) of
// the host entry points, the counters and one zero word
constexpr size_t kRayBytes = 24, kHitBytes = 48;  // sizeof(rt_ray), sizeof(rt_hit) (rt_abi.h)
struct Query {
  size_t rays = 0;  // the clamped size
  Span ra, rb, queue, res, d_in, d_out, cnt, zero;
  size_t total = 0;
};
inline Query query(size_t rays) {
  Query L;
  const size_t n = L.rays = std::max<size_t>(rays, 1024);
  Builder b;
  L.ra = b.add(n * 16);
  L.rb = b.add(n * 8);
  L.queue = b.add(n * 4);
  L.res = b.add(n * 2 * 4);
  L.d_in = b.add(n * kRayBytes);
  L.d_out = b.add(n * kHitBytes);
  L.cnt = b.add(kCntWords * 4);
  L.zero = b.add(4);
  L.total = b.total();
  return L;
}

// ---- display denoiser and display history (rt_ctx::Denoise, rt_ctx::Temporal) --------------------
// Frames of npx = W * H pixels; the first-hit frame is in local-tile layout (hit_px pixels)
struct Denoise {
  Span col[2], g0, g1, hits, out;
  size_t total = 0;
};
inline Denoise denoise(size_t npx, size_t hit_px) {
  Denoise L;
  Builder b;
  for (Span& c : L.col) c = b.add(npx * 16);
  L.g0 = b.add(npx * 16);
  L.g1 = b.add(npx * 16);
  L.hits = b.add(hit_px * kHitBytes);
  L.out = b.add(npx * 12);
  L.total = b.total();
  return L;
}
// gp[k - 1] is guide pair k: pair 0 is the denoiser's g0 / g1
struct History {
  Span col[2], gp[2][2], out;
  size_t total = 0;
};
inline History history(size_t npx) {
  History L;
  Builder b;
  for (Span& c : L.col) c = b.add(npx * 16);
  for (auto& pair : L.gp)
    for (Span& g : pair) g = b.add(npx * 16);
  L.out = b.add(npx * 12);
  L.total = b.total();
  return L;
}

// The motion mode of the display history (rt_temporal_set_motion; rt_ctx::Motion), two allocations of
// their own that exist only while the mode is on.  Poses: per {r, g, b, n} frame of History (col[k])
// a copy of the scene's vertex records d_tri and d_trin, 3 float4 per triangle each (the scene's
// size: dropped by rt_set_scene).  Triangle frames: per guide pair (0: the denoiser's, then History's
// two) the int32 first-hit triangle of each pixel (the frame's size: dropped by rt_resize).
constexpr size_t kTriRecBytes = 3 * 16;  // one triangle of d_tri, and of d_trin
struct Poses {
  Span tri[2], trin[2];
  size_t total = 0;
};
inline Poses poses(size_t n_tri) {
  Poses L;
  Builder b;
  for (int k = 0; k < 2; k++) {
    L.tri[k] = b.add(n_tri * kTriRecBytes);
    L.trin[k] = b.add(n_tri * kTriRecBytes);
  }
  L.total = b.total();
  return L;
}
struct TriFrames {
  Span tf[3];
  size_t total = 0;
};
inline TriFrames tri_frames(size_t npx) {
  TriFrames L;
  Builder b;
  for (Span& f : L.tf) f = b.add(npx * 4);
  L.total = b.total();
  return L;
}

// The variance mode of the display chain (rt_variance_set; rt_ctx::Variance), one allocation of its own
// that exists only while the mode is on (the frame's size: dropped by rt_resize).  st[k]: the state
// texel {l_prev, S_prev, v, m} beside each {r, g, b, n} texel of History's col[k].  tvar: the variance
// of the temporal stage's output; dvar: the denoiser's ping-pong pair.  44 B per pixel.
struct Variance {
  Span st[2], tvar, dvar[2];
  size_t total = 0;
};
inline Variance variance(size_t npx) {
  Variance L;
  Builder b;
  for (Span& s : L.st) s = b.add(npx * 16);
  L.tvar = b.add(npx * 4);
  for (Span& v : L.dvar) v = b.add(npx * 4);
  L.total = b.total();
  return L;
}

// ---- frame table (rt_ctx::FrameTable), in ints ---------------------------------------------------
// [cap] loop_num, [cap] rand_origin, then what wf_sobol adds: [cap][4] float2 Sobol pairs and [cap]
// float2 blend weights.  The pinned host copy holds the two uploaded sub-tables alone.
struct FrameTable {
  Span loop_num, rand_origin, sobol, blend_w;
  size_t host_total = 0, total = 0;
};
inline FrameTable frame_table(size_t cap) {
  FrameTable L;
  size_t at = 0;
  auto add = [&](size_t ints) { const Span s{at, ints}; at += ints; return s; };
  L.loop_num = add(cap);
  L.rand_origin = add(cap);
  L.host_total = at;
  L.sobol = add(cap * 4 * 2);
  L.blend_w = add(cap * 2);
  L.total = at;
  return L;
}

// ---- camera table (rt_ctx::d_cam), in float4 -----------------------------------------------------
// Per pipeline set one table of camera directions (WFState::cam) and one of camera hit points
// (WFState::org), n_valid work items each: the directions of every set, then the hit points
struct CameraTable {
  size_t n_valid = 0, sets = 0;
  Span dir(size_t p) const { return Span{p * n_valid, n_valid}; }
  Span org(size_t p) const { return Span{sets * std::max<size_t>(1, n_valid) + p * n_valid, n_valid}; }
  size_t total() const { return 2 * sets * std::max<size_t>(1, n_valid); }
};
inline CameraTable camera_table(size_t n_valid, size_t sets) { return CameraTable{n_valid, sets}; }

}  // namespace dvl
