// render_plan.h — which kernels a wavefront batch runs (host side, HIP-free).
//
// rt_render_async cuts a call into batches, a batch into frame or pixel groups, and runs each group
// as a list of passes.  Everything that is decided there and not merely looked up is decided here:
// the batch size, the pure part of pipeline admission, the groups' ranges and flags, and per pass the
// wf_trace / wf_shade instantiations with their grids, or the finisher.  rt_render.hip copies the
// facts below out of rt_ctx, calls these functions and launches what they name; DESIGN.md §4 has the
// rules as one table.  Nothing here reads the environment, allocates or includes a HIP header, so
// tests/test_render_plan.py checks the rules on the CPU through rts_render_plan (rt_scene.h) against
// a second statement of them (tests/render_plan_model.py).
//
// Every input is an int64_t in one flat struct (In), so a plan can be restated from the numbers the
// development library prints (`[rt] plan group`, kInNames / kGroupNames / kStepNames order).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "dev_layout.h"
#include "rt_abi.h"

// The release defaults of rpl::Switches (-D overrides for `make variant` as before)
#ifndef RT_SPLIT_CONT_FIRST  // split queues: the continuations' launch first (1) or the shadow rays' (0)
#define RT_SPLIT_CONT_FIRST 0  // C3 1 vs 0: -0.16% (profiles/r06_ab_split_knobs_C3.log)
#endif
#ifndef RT_CAM_SHADE  // the bulk camera pass's shade in its own instantiation (wf_shade<..., CAM>)
#define RT_CAM_SHADE 1
#endif
#ifndef RT_CAM_SHARED  // groups of several frames trace each pixel's camera ray once (WFParams::cam_shared)
#define RT_CAM_SHARED 1
#endif
#ifndef RT_CAM_MISS_ONCE  // bulk groups that run the shared camera trace and wf_shade<..., CAM> handle a pixel whose
                          // camera ray misses once per group, not once per frame (WFParams::cam_miss_once)
#define RT_CAM_MISS_ONCE 1
#endif
#ifndef RT_P1_LEAN  // groups with cam_miss_once and 16-B pass-1 rays in a scene without emissive materials: pass 1
                    // walks the hit-pixel list (no s5 row, active list or continuation queue out of pass 0:
                    // WFParams::p1_lean)
#define RT_P1_LEAN 1
#endif
#ifndef RT_CAM_SHARED_STATIC  // a bulk group's shared camera trace (one ray per work item: a small pass) runs the
                              // bulk's instantiation (0) or the small passes' (1: static shares, lane quads, every
                              // claim 64 rays): C3, 2.07 M rays of one 256-frame group standalone 0.299 vs 0.662 ms
                              // (11 ms per slot before), whole step +0.2% (noise); profiles/r07_passes256_*_C3.log,
                              // profiles/r07_ab_proc_shared_camera_C3.log
#define RT_CAM_SHARED_STATIC 0
#endif

namespace rpl {

constexpr int kMaxGroups = 4;  // rt_ctx::MAX_GROUPS

// What the context holds when the call arrives (rt_ctx's fields of the same names), and four
// constants of the kernels (rt_wavefront.h: SH_SUB, SH_SUB_CAM, SH_SUB_BULK, kP1SampleEvery)
struct Facts {
  int64_t n_groups, n_valid, frames_cap, wf_paths, finish_pass, pipe_finish_pass, finish_slots, split_kinds,
      split_passes, wide, mats_emissive, tile_cost_on, wf_hit_cap, wf_rows, order_head, pipe_depth, pipe_nomem_slots,
      n_cus, trace_bpc0, trace_bpc, finish_bpc, pipe_finish_bpc, sh_sub, sh_sub_cam, sh_sub_bulk, p1_sample_every;
};
// What the call brings: rt_frame_params' flags, enable_bsdf and max_bounce, the traced frames not
// yet run, whether every stream a pipelined call could overlap was found idle (admit_pipe), and
// for a batch whether the call runs pipelined and on which path-state set
struct Call {
  int64_t flags, enable_bsdf, max_bounce, n_left, idle, pipe, pset;
};
// Compile-time choices and, in the development library, their A/B overrides from the environment
// (rt_render.hip dev_switches, once per call).  -1: no override.
struct Switches {
  int64_t cam_shade = RT_CAM_SHADE != 0, cam_shared = RT_CAM_SHARED != 0, cam_shared_static = RT_CAM_SHARED_STATIC != 0,
          cam_miss_once = RT_CAM_MISS_ONCE != 0, p1_lean = RT_P1_LEAN != 0,
#ifdef RT_ROW_COMPACT  // (defined where the kernels read it: rt_wavefront.h)
          row_compact = RT_ROW_COMPACT != 0,
#else
          row_compact = 1,
#endif
          split_cont_first = RT_SPLIT_CONT_FIRST != 0;
  int64_t pix_split = 1;                        // RT_PIX_SPLIT=0: a batch of fewer frames than groups stays one group
  int64_t group_head = -1;                      // RT_GROUP_SPLIT: pixel group 0's work items (replaces order_head)
  int64_t finish_pass_g[kMaxGroups] = {-1, -1, -1, -1};  // RT_FINISH_PASS_G<g>
  int64_t row_cap = -1;                         // RT_ROW_CAP: at most this many arena rows
};
struct In {
  Facts f;
  Call c;
  Switches s;
};
constexpr const char* kInNames[] = {
    "n_groups", "n_valid", "frames_cap", "wf_paths", "finish_pass", "pipe_finish_pass", "finish_slots", "split_kinds",
    "split_passes", "wide", "mats_emissive", "tile_cost_on", "wf_hit_cap", "wf_rows", "order_head", "pipe_depth",
    "pipe_nomem_slots", "n_cus", "trace_bpc0", "trace_bpc", "finish_bpc", "pipe_finish_bpc", "sh_sub", "sh_sub_cam",
    "sh_sub_bulk", "p1_sample_every",
    "flags", "enable_bsdf", "max_bounce", "n_left", "idle", "pipe", "pset",
    "sw_cam_shade", "sw_cam_shared", "sw_cam_shared_static", "sw_cam_miss_once", "sw_p1_lean", "sw_row_compact",
    "sw_split_cont_first", "sw_pix_split", "sw_group_head", "sw_finish_pass_g0", "sw_finish_pass_g1", "sw_finish_pass_g2",
    "sw_finish_pass_g3", "sw_row_cap"};
constexpr int kInCount = sizeof(kInNames) / sizeof(kInNames[0]);
static_assert(sizeof(In) == kInCount * sizeof(int64_t), "In is kInCount int64_t, in kInNames' order");

// ---- the call ------------------------------------------------------------------------------------
inline bool serial(const Call& C) { return (C.flags & RT_FLAG_SERIAL) && !(C.flags & RT_FLAG_MEGAKERNEL); }
// Frames per batch.  RT_FLAG_SERIAL: one frame group per batch, as many frames as one group's path
// state holds
inline int batch_cap(const Facts& F, const Call& C) {
  if (C.flags & RT_FLAG_MEGAKERNEL) return RT_MAX_FRAMES_PER_LAUNCH;
  if (!serial(C)) return (int)F.frames_cap;
  return (int)std::max<int64_t>(1, std::min(F.frames_cap, F.wf_paths / std::max<int64_t>(1, F.n_valid)));
}
// every group gets whole 64-item blocks, and a tile-cost probe keeps one wavefront
inline bool groups_ok(const Facts& F) { return F.n_valid >= 64 * F.n_groups && !F.tile_cost_on; }
// a batch of fewer frames than groups splits by pixels instead
inline bool pix_split_ok(const Facts& F, const Switches& S, int64_t n_frames) {
  return S.pix_split && n_frames < F.n_groups && groups_ok(F);
}
inline int pipe_sets(const Facts& F) { return (int)std::min(F.pipe_depth, F.n_groups); }
// A pipelined call (rt_set_pipeline): one-frame calls, and calls of one batch (at most frames_cap
// frames) whose whole path state fits in each set ...
inline bool pipe_candidate(const Facts& F, const Call& C) {
  const int64_t n = C.n_left, nv = std::max<int64_t>(1, F.n_valid);
  return pipe_sets(F) >= 2 && !(C.flags & RT_FLAG_MEGAKERNEL) && !serial(C) && n > 0 && groups_ok(F) &&
         (n < F.n_groups || (n <= F.frames_cap && n * nv < F.pipe_nomem_slots));
}
// ... but a one-frame call with no call in flight has nothing to overlap: the pixel-split groups
// have the lower latency (C4 1080p 5.6 vs 6.8 ms synchronised).  idle_matters: probe the streams
inline bool idle_matters(const Facts& F, const Switches& S, const Call& C) {
  return pipe_candidate(F, C) && pix_split_ok(F, S, C.n_left);
}
inline bool admit_pipe(const Facts& F, const Switches& S, const Call& C) {
  return pipe_candidate(F, C) && !(pix_split_ok(F, S, C.n_left) && C.idle);
}

// ---- a batch and its groups ----------------------------------------------------------------------
// Frames [f0, f1) of the batch and work items [w0, w1); one of the two is the whole range.
// set: path-state set and overflow column; stream: 0 the caller's, k rt_ctx::aux[k].  The flags are
// WFParams' fields of the same names; cam_shared holds in pass 0 alone.
struct Group {
  int f0, f1;
  unsigned int w0, w1, slots;
  int set, stream;
  bool fuse_blend, split_g, finish;
  int fin_pass;
  bool p1_compact, cam_shared, cam_miss_once, p1_lean, row_compact;
  unsigned int row_cap;
  bool blend;   // the group ends with wf_blend (not fused into its shade)
  int n_steps;  // passes 0 .. n_steps - 1 (step()); the finisher, if any, is the last
};
struct Batch {
  int nf, G;
  bool pix_split;
  Group g[kMaxGroups];
};
constexpr const char* kGroupNames[] = {"f0", "f1", "w0", "w1", "slots", "set", "stream", "fuse_blend", "split_g", "finish",
                                       "fin_pass", "p1_compact", "cam_shared", "cam_miss_once", "p1_lean", "row_compact",
                                       "row_cap", "blend", "n_steps"};
constexpr int kGroupCount = sizeof(kGroupNames) / sizeof(kGroupNames[0]);
inline void flatten(const Group& g, int64_t* o) {
  const int64_t v[kGroupCount] = {g.f0, g.f1, g.w0, g.w1, g.slots, g.set, g.stream, g.fuse_blend, g.split_g, g.finish,
                                  g.fin_pass, g.p1_compact, g.cam_shared, g.cam_miss_once, g.p1_lean, g.row_compact,
                                  g.row_cap, g.blend, g.n_steps};
  std::copy(v, v + kGroupCount, o);
}

// bulk: above the finisher's slot budget and not fused (the wf_shade<..., SH_SUB_BULK / CAM> launches)
inline bool bulk(const Facts& F, const Group& g) { return (int64_t)g.slots > F.finish_slots && !g.fuse_blend; }
// the CAM shade: the camera pass of a bulk group of >= 64 frames
inline bool cam_shade(const Facts& F, const Switches& S, const Group& g) {
  return S.cam_shade && bulk(F, g) && g.slots && g.f1 - g.f0 >= 64;
}

// Split the batch (min(batch_cap, n_left) frames) into frame groups, one stream per group; a batch
// of fewer frames than groups (one frame per call: the reference's own usage) is split by pixels
// instead, so the groups' latency-bound late passes still overlap each other.  Needs 1 <= n_groups
// <= kMaxGroups and n_left >= 1.
inline Batch plan_batch(const Facts& F, const Switches& S, const Call& C) {
  Batch B{};
  const bool pipe = C.pipe != 0, count = (C.flags & RT_FLAG_COUNT_VISITS) != 0;
  const int nf = B.nf = (int)std::min<int64_t>(batch_cap(F, C), C.n_left);
  const bool pix_split = B.pix_split = !pipe && !serial(C) && pix_split_ok(F, S, nf);
  const int G = B.G = (pipe || serial(C)) ? 1 : pix_split ? (int)F.n_groups : (int)std::min<int64_t>(F.n_groups, nf);
  const int last_pass = (int)std::max<int64_t>(0, C.max_bounce);
  // pixel ranges of the groups: even, or after rt_order_work the costly head as group 0 and the
  // rest split evenly
  const size_t nv = (size_t)F.n_valid, b0 = (size_t)(S.group_head >= 0 ? S.group_head : std::min(F.order_head, F.n_valid));
  auto wbound = [&](int g) -> unsigned int {
    if (g <= 0) return 0u;
    if (g >= G) return (unsigned)nv;
    if (b0 > 0 && G > 1) return (unsigned)(b0 + (nv - b0) * (size_t)(g - 1) / (size_t)(G - 1));
    return (unsigned)(nv * (size_t)g / (size_t)G);
  };
  for (int k = 0; k < G; k++) {
    Group& g = B.g[k];
    g.f0 = pix_split ? 0 : k * nf / G;
    g.f1 = pix_split ? nf : (k + 1) * nf / G;
    g.w0 = pix_split ? wbound(k) : 0u;
    g.w1 = pix_split ? wbound(k + 1) : (unsigned)nv;
    const int n_frames = g.f1 - g.f0;
    const unsigned int n_work = g.w1 - g.w0;
    g.slots = (unsigned)n_frames * n_work;
    g.set = pipe ? (int)C.pset : k;
    g.stream = pipe ? 1 + (int)C.pset : k;
    // (not for frame groups of one frame each: their blends must run in frame order)
    g.fuse_blend = !pipe && n_frames == 1 && (pix_split || G == 1) && !count;
    g.blend = !g.fuse_blend;
    // bulk groups queue the two ray kinds apart (per pass in step(): passes 1 .. split_passes)
    g.split_g = F.split_kinds && F.wide && !count && !F.tile_cost_on && bulk(F, g);
    // small groups (one frame per call) end their paths in wf_finish after pass fin_pass - 1
    g.fin_pass = (int)((pipe && F.pipe_finish_pass >= 0) ? F.pipe_finish_pass : F.finish_pass);
    if (S.finish_pass_g[k] >= 0) g.fin_pass = (int)S.finish_pass_g[k];
    g.finish = !count && !F.tile_cost_on && !(C.flags & RT_FLAG_NO_FINISH) && g.fin_pass >= 1 && g.fin_pass <= last_pass &&
               ((C.flags & RT_FLAG_FINISH) || (int64_t)g.slots <= F.finish_slots);
    g.n_steps = g.finish ? g.fin_pass + 1 : last_pass + 1;
    // pass 0 queues 16-B rays (WFState::org) unless the finisher takes them over at pass 1
    g.p1_compact = !(g.finish && g.fin_pass <= 1);
    // A group of several frames traces each work item's camera ray once and every frame's shade
    // reads that result.  The counting runs (RT_FLAG_COUNT_VISITS, and with it the rt_tile_costs /
    // rt_order_work probes and the counting per-pass reports) keep one traversal per path slot:
    // their counters are the steps of the rays counted in rt_stats.rays, and the tile balance is
    // calibrated on them.
    g.cam_shared = S.cam_shared && n_frames > 1 && !count && !F.tile_cost_on;
    // the groups that run both the shared camera trace and the CAM shade: miss pixels get their
    // record and the hit pixels their list before the shade (wf_cam_classify)
    g.cam_miss_once = S.cam_miss_once && cam_shade(F, S, g) && g.cam_shared && (int64_t)n_work <= F.wf_hit_cap;
    // the lean pass-0 -> pass-1 state: pass 1 exists, reads 16-B rays and split queues, and no
    // camera hit can be emissive
    g.p1_lean = S.p1_lean && g.cam_miss_once && g.p1_compact && last_pass >= 1 && g.split_g && 1 <= F.split_passes &&
                !F.mats_emissive;
    // lean groups move the state of passes >= 2 to the row arena when pass 1's continuation hits
    // fit a quarter of the group's slots (decided on the device: rtd::rows_on); not when wf_finish
    // ends the group's paths: it reads the slot-indexed state
    g.row_compact = S.row_compact && g.p1_lean && !g.finish;
    size_t cap = std::min(dvl::arena_rows(g.slots), (size_t)F.wf_rows);
    if (S.row_cap >= 0) cap = std::min(cap, (size_t)S.row_cap);
    g.row_cap = (unsigned int)cap;
  }
  return B;
}

// ---- a group's passes ----------------------------------------------------------------------------
// Each enumerator is one wf_trace instantiation (rt_render.hip launch_trace).  *_SMALL: static first
// shares of mid-size passes (groups within finish_slots, or RT_CAM_SHARED_STATIC's camera trace);
// SHADOW / CONT: the split queues' two launches; P1_*: pass 1 over the 16-B rays pass 0 queued
// (WFState::org), in instantiations of its own so the later passes' kernel carries none of it.  The
// rest take both kinds from one queue: C = counting (RT_FLAG_COUNT_VISITS), W = the 4-wide tree,
// B = the binary tree.
enum Trace {
  CAM_SMALL, P1_SMALL, REG_SMALL, P1_SHADOW, P1_CONT_LEAN, P1_CONT, SHADOW, CONT,
  CAM_CW, P1_CW, REG_CW, CAM_CB, P1_CB, REG_CB, CAM_W, P1_W, REG_W, CAM_B, P1_B, REG_B,
  kTraceCount
};
// The shade of one pass.  fused: one frame per path-state set, the blend inside the shade
// (WFParams::fuse_blend); bulk: groups above finish_slots, SH_SUB_BULK paths per thread and
// block-iteration; cam: the camera pass of a bulk group with >= 64 frames (camera-hit records);
// cam_lean / bulk_lean: pass 0 / pass 1 of a group with WFParams::p1_lean; plain: everything else
enum Shade { PLAIN, BULK, CAM, FUSED, CAM_LEAN, BULK_LEAN, kShadeCount };

// One pass of a group: the finisher (fgrid blocks; the last step), or trace(s) and a shade.  Grids
// are in blocks of 256 threads.
struct Step {
  bool finisher;
  unsigned int fgrid;
  bool split, split_out;  // WFParams' fields (the finisher's launch carries them too)
  unsigned int cam_n;     // WFParams::cam_n: pass 0's camera paths are implicit
  bool cam_shared;
  int n_trace;            // 1, or 2 for split queues
  int trace[2];           // Trace; trace[1] = -1 when n_trace = 1
  unsigned int trace_grid;
  bool classify;          // wf_cam_classify after the trace
  unsigned int classify_grid;
  bool p1_count;          // wf_p1_count<true>, then <false>, before the shade
  unsigned int p1_grid[2];
  int shade;              // Shade
  unsigned int shade_grid;
};
constexpr const char* kStepNames[] = {"finisher", "fgrid", "split", "split_out", "cam_n", "cam_shared", "n_trace", "trace0",
                                      "trace1", "trace_grid", "classify", "classify_grid", "p1_count", "p1_grid0", "p1_grid1",
                                      "shade", "shade_grid"};
constexpr int kStepCount = sizeof(kStepNames) / sizeof(kStepNames[0]);
inline void flatten(const Step& s, int64_t* o) {
  const int64_t v[kStepCount] = {s.finisher, s.fgrid, s.split, s.split_out, s.cam_n, s.cam_shared, s.n_trace, s.trace[0],
                                 s.trace[1], s.trace_grid, s.classify, s.classify_grid, s.p1_count, s.p1_grid[0],
                                 s.p1_grid[1], s.shade, s.shade_grid};
  std::copy(v, v + kStepCount, o);
}

// Pass `pass` of group g, 0 <= pass < g.n_steps.  A pure function of the pass, not a stored array:
// rt_frame_params::max_bounce has no upper bound.
inline Step step(const Facts& F, const Switches& S, const Call& C, const Group& g, int pass) {
  Step s{};
  s.trace[0] = s.trace[1] = -1;
  s.shade = -1;
  const unsigned int n_cus = (unsigned)F.n_cus, n_frames = (unsigned)(g.f1 - g.f0), n_work = g.w1 - g.w0;
  s.split = g.split_g && pass >= 1 && pass <= F.split_passes;
  s.split_out = g.split_g && pass + 1 <= F.split_passes;
  if (g.finish && pass == g.fin_pass) {
    s.finisher = true;
    // a pipelined call's finisher leaves room for the next call's passes (rt_ctx::pipe_finish_bpc)
    s.fgrid = n_cus * (unsigned)(C.pipe ? F.pipe_finish_bpc : F.finish_bpc);
    return s;
  }
  s.cam_n = pass == 0 ? g.slots : 0u;
  s.cam_shared = pass == 0 && g.cam_shared;
  // ---- trace
  const bool count = (C.flags & RT_FLAG_COUNT_VISITS) != 0, wide = F.wide != 0;
  const bool p1 = !s.cam_n && pass == 1 && g.p1_compact;
  const bool small = (int64_t)g.slots <= F.finish_slots || (s.cam_shared && S.cam_shared_static);
  const int kind = s.cam_n ? 0 : p1 ? 1 : 2;  // camera, pass 1's 16-B rays, the rest
  s.n_trace = 1;
  s.trace_grid = n_cus * (unsigned)(pass == 0 ? F.trace_bpc0 : F.trace_bpc);
  if (small && !count && wide) {
    s.trace[0] = CAM_SMALL + kind;
  } else if (s.split && !s.cam_n && !count && wide) {  // the shadow rays, then the continuations
    s.n_trace = 2;
    for (int k = 0; k < 2; k++) {
      const bool shadow = (k == 0) != (S.split_cont_first != 0);
      s.trace[k] = p1 ? (shadow ? P1_SHADOW : g.p1_lean ? P1_CONT_LEAN : P1_CONT) : shadow ? SHADOW : CONT;
    }
  } else {
    s.trace[0] = (count ? (wide ? CAM_CW : CAM_CB) : (wide ? CAM_W : CAM_B)) + kind;
  }
  // ---- between the trace and the shade
  if (pass == 0 && g.cam_miss_once) {
    s.classify = true;  // (two blocks per CU: few waves, so few atomics on the list's counter)
    s.classify_grid = std::max(1u, std::min(2u * n_cus, (n_work + 255u) / 256u));
  }
  const bool lean0 = g.p1_lean && pass == 0, lean1 = g.p1_lean && pass == 1;
  if (lean1 && g.row_compact) {  // the hits the shade will number with rows (rtd::rows_on reads the count)
    const unsigned int items = (unsigned)std::min<size_t>(g.slots, (size_t)n_work * (size_t)n_frames);
    const unsigned int runs = (items + 255u) / 256u;
    s.p1_count = true;
    s.p1_grid[0] = std::max(1u, std::min(8u * n_cus, runs / (unsigned)F.p1_sample_every + 1u));
    s.p1_grid[1] = std::max(1u, std::min(8u * n_cus, runs));
  }
  // ---- shade
  const bool cam = s.cam_n && cam_shade(F, S, g);
  s.shade = g.fuse_blend ? FUSED : lean0 ? CAM_LEAN : cam ? CAM : lean1 ? BULK_LEAN : bulk(F, g) ? BULK : PLAIN;
  const unsigned int sub = (unsigned)(s.shade == CAM || s.shade == CAM_LEAN     ? F.sh_sub_cam
                                      : s.shade == BULK || s.shade == BULK_LEAN ? F.sh_sub_bulk
                                                                                : F.sh_sub);
  s.shade_grid = std::max(1u, std::min(4096u, (g.slots + 256u * sub - 1) / (256u * sub)));
  return s;
}

}  // namespace rpl
