// rt_render.hip — librtamd.so: the C-ABI of include/rt_abi.h over the gfx950 path-tracing
// kernels of rt_kernels.h.  Host code here uploads what the scene compiler
// (csrc/common/scene_compile.h) makes of the reference's scene description (SoA or the
// reference's own AoS encodings), owns the device buffers and launches the persistent kernel.  No fallback path: without a HIP device every
// entry point returns RT_ERR_NODEVICE / RT_ERR_HIP.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <new>
#include <string>
#include <vector>
#include <limits>

#include "rt_abi.h"
#include "rt_kernels.h"
#include "rt_wavefront.h"
#include "rt_query.h"
#include "rt_denoise.h"
#include "rt_temporal.h"

#ifndef RT_SPLIT_KINDS  // bulk groups trace shadow rays and continuations in launches of their own (round 6)
#define RT_SPLIT_KINDS 1
#endif
#ifndef RT_SPLIT_PASSES  // the last pass traced split (later ones: one launch, both kinds); C3 3 / 4 / 5 / 6 / 7 vs 8:
                         // -0.18, -0.15 / +0.19, +0.22 / -0.03 / -0.04% (profiles/r06_ab_split_passes_C3.log)
#define RT_SPLIT_PASSES 5
#endif
#include "scene_compile.h"
#include "dev_layout.h"
#include "render_plan.h"
#include "rt_geometry.h"

using rtd::GNode;
using rtd::KParams;

struct rt_ctx {
  int device = 0;
  int n_cus = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  // scene
  GNode* d_nodes = nullptr;
  rtd::QNode* d_qnodes = nullptr;
  int qroot = 0, qstack_entries = 2, n_qnodes = 0;
  bool wide = false;                          // 4-wide traversal available for this scene
  float4* d_tri = nullptr;
  float4* d_trx = nullptr;  // traversal records (tri_filter.h)
  double tri_k1 = 0.0, tri_k0 = 0.0;  // their edge-filter margin
  int tri_flagged = 0;
  float4* d_trin = nullptr;
  float4* d_hrec = nullptr;  // the shade's hit records (KParams::hrec)
  float4* d_mats = nullptr;
  int n_tri = 0, n_mats = 0, root = 0, has_scene = 0, stack_entries = 2;
  double cull_R = 0.0, cull_K = 0.0, cull_off = 0.0;  // culling bound of the scene (cull_bound_stats)
  bool scene_set = false;
  // what rt_update_geometry needs of the compile: the edge filter's state (trif::Consts), whether
  // d_qnodes holds a 4-wide tree, the binary node count and the six scene arrays' sizes in bytes
  double s_cap = 0.0, sc_cap = 0.0, s_max = 0.0, sc_max = 0.0, c_min = 1.0;
  bool qbuilt = false;
  int n_nodes = 0;
  size_t scene_bytes[6] = {};  // indexed by RT_SCENE_*
  // rt_update_geometry's refit schedule (scn::refit_plan) and staging: built by the first update
  // after a rt_set_scene, from the node arrays as they stand on the device
  struct Geometry {
    bool planned = false;
    int4* d_leaves = nullptr;
    int n_leaves = 0;
    int *d_blist = nullptr, *d_boff = nullptr, *d_qlist = nullptr, *d_qoff = nullptr;
    std::vector<int32_t> boff, qoff;
    rtg::Red* d_red = nullptr;
    float* d_stage = nullptr;  // the host form's vertex arrays (18 floats per triangle), then its indices
    size_t stage_tris = 0;
  } geo;
  std::vector<int32_t> tri_mat;  // host copy of the per-triangle material ids (for updates)
  std::vector<float> mat_table;  // host copy, 32 floats per material
  // some material's emission is not +0 (all bits): an emissive camera hit needs s2.w for Le0.y, so
  // such scenes keep the full pass-0 -> pass-1 state (WFParams::p1_lean stays 0)
  bool mats_emissive = false;
  // env
  float4* d_hdr = nullptr;
  float2* d_cache = nullptr;                  // hdrCache.rg; d_hdr = {hdrMap.rgb, hdrCache.b}
  // NEE light samples per hdrCache texel (rt_light_table_kernel) for one envAngle each: two tables,
  // so a call whose angle differs from the previous call's rebuilds the other table on its own
  // stream after the last call that read that one (an event), without draining calls in flight
  struct LightTable {
    float4* d = nullptr;
    bool valid = false;
    float angle = 0.0f;                       // the envAngle d was built for
    hipEvent_t last_use = nullptr;            // on the ctx stream after the last call that read d
    hipEvent_t built = nullptr;               // after the kernel that last built d (on that call's stream)
  };
  LightTable light[2];
  int light_cur = 0;                          // the table the last call used
  int hdr_w = 0, hdr_h = 0, hdr_res = 0;
  bool env_set = false;
  // frame
  int W = 0, H = 0, tile_w = 32, tile_h = 32, tiles_x = 0, tiles_y = 0, rank = 0, world = 1;
  int local_tiles = 0, max_local_tiles = 0;
  float4* d_accum = nullptr;
  bool frame_set = false;
  int loop_num = 0;
  // counters
  unsigned int* d_counter = nullptr;
  unsigned long long* d_stats = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;        // whole render calls
  struct TraceEv {
    hipEvent_t s, e;
    uint64_t call;  // the render call (its index in `launches`) that queued the launch
  };
  std::vector<TraceEv> trace_events;  // traversal launches
  std::vector<hipEvent_t> event_pool;
  double kernel_ms = 0.0, trace_ms = 0.0;
  // Union of the traversal launches' intervals (rt_stats.trace_busy_ms).  Each folded launch is
  // placed on a double-precision timeline by its start's offset from the previously folded
  // launch's start (busy_anchor, at busy_anchor_t ms), so an offset is a short float interval
  // however long the context lives.  Intervals that can no longer overlap a pending launch are
  // summed into busy_closed_ms and dropped: a launch of call k starts after every launch of
  // call k-2 has ended (pipelined calls wait for their set's previous call; the ctx stream joins
  // each call's streams), so folding call k's launches closes the intervals of calls <= k-2 and
  // the open list holds about two calls' worth.
  struct BusyIv {
    double lo, hi;
    uint64_t call;  // the newest call merged into the interval
  };
  hipEvent_t busy_anchor = nullptr;
  double busy_anchor_t = 0.0;
  std::vector<BusyIv> busy;
  double busy_closed_ms = 0.0;
  uint64_t launches = 0, trace_launches = 0;
  int blocks_per_cu = 0, block_lds = 0;      // megakernel
  int trace_bpc = 0, trace_bpc0 = 0;          // wavefront traversal blocks/CU (passes >= 1, pass 0)
  int trace_lds_entries = 0, trace_lds = 0;
  int split_kinds = RT_SPLIT_KINDS;  // bulk groups: shadow rays and continuations in queues of their own
  int split_passes = RT_SPLIT_PASSES;  // ... in passes 1 .. split_passes (later ones: one queue, one launch)
  // per-frame loopNum / randOrigin of one render call: pinned host staging -> device table;
  // ft[0] for batched calls, ft[1 + p] for pipelined one-frame calls on pipeline set p
  struct FrameTable {
    int* h = nullptr;                         // [cap] loop_num then [cap] rand_origin bits
    int* d = nullptr;                         // + [cap][4] float2 Sobol pairs (wf_sobol)
    size_t cap = 0;
    hipEvent_t ev = nullptr;                  // the last upload (the host table is reused after it)
  };
  FrameTable ft[5];
#ifndef RT_POOL_CHUNK_DEFAULT
#define RT_POOL_CHUNK_DEFAULT 1024
#endif
  int pool_chunk = RT_POOL_CHUNK_DEFAULT;     // rays per queue atomic in wf_trace (C3: 256 -> 512 -> 1024: +2.3%, +2.4%)
  int2* d_stack_ovf = nullptr;
  void* d_disp = nullptr;                     // rt_tonemap output (W*H*3 bytes)
  size_t disp_bytes = 0;
  void* d_gather = nullptr;                   // rt_gather on rank 0: every rank's tiles, then the frame
  // rt_gather over RCCL: the communicators (one per rank, this process drives them all) of the
  // device set ctxs[0] last gathered over, and the transport its last gather used
  std::vector<int> rccl_devs;
  std::vector<ncclComm_t> rccl_comms;
  int gather_transport = 0;
  size_t gather_bytes = 0;
  size_t stack_ovf_bytes = 0;
  // wavefront path state (one slot per local pixel)
  void* wf_mem = nullptr;
  size_t wf_paths = 0;                        // path slots per frame group
  size_t wf_hit_cap = 0;                      // entries of each set's hit-pixel list (WFState::hit)
  rtd::WFState wf{};                          // pixel lists (shared by every group)
  // Frame groups: the frames of one batch are split into n_groups independent wavefronts with
  // their own path state, run on their own streams, so the latency tail of one group's late
  // bounces overlaps the other's busy passes; blends stay in frame order (events).
  static constexpr int MAX_GROUPS = 4;
  int n_groups = 2;
  // rt_order_work's costly head: the first order_head work items (whole 64-item blocks) are the
  // costliest blocks and form pixel group 0 of a one-frame call; 0 = even split
  size_t order_head = 0;
  rtd::WFState wfg[MAX_GROUPS]{};
  rtd::WFState wfa[MAX_GROUPS]{};             // each set's row arena (WFParams::A): wf_rows rows
  size_t wf_rows = 0;
  hipStream_t aux[MAX_GROUPS] = {};
  unsigned int* d_pix = nullptr;   // pixel list of this rank: xy then accumulation index
  // tile ownership: owner[t] = rank of global tile t (default t % world; rt_set_tile_owners);
  // my_tiles = this rank's global tiles in local order; tile_src[t] = (rank, local index)
  std::vector<int32_t> owner, my_tiles;
  int* d_tile_ids = nullptr;       // my_tiles on the device (KParams.tile_ids)
  int2* d_tile_src = nullptr;      // tile_src on the device (rt_assemble_kernel)
  unsigned long long* d_tile_cost = nullptr;  // rt_tile_costs: per local tile, during the probe only
  bool tile_cost_on = false;
  bool cost_blocks = false;        // the probe counts per 64-item work block (rt_order_work)
  float4* d_cam = nullptr;         // per pixel of this rank: camera direction, u * v (wf_camera), then the
                                   // per-pixel camera hit points (WFState::org), one of each per set
  int cam_sets = 1;                // camera tables in d_cam (one per pipeline set, n_valid each)
  int n_valid = 0;                 // valid pixels of this rank (work items of the wavefront)
  int frames_cap = 1;              // frames in flight per wavefront
  size_t max_slots_req = 0;        // rt_set_max_paths (0: RT_MAX_SLOTS or the 320 Mi default)
  // path-persistent finisher (wf_finish): a frame group of at most finish_slots path slots runs
  // passes 0 .. finish_pass-1 as wavefront passes, then one wf_finish launch ends every path
  int finish_pass = 2;  // C3 1080p single frames: 1 / 2 / 3 -> 3.73 / 3.35 / 3.41 ms (off: 3.79)
  uint64_t finish_slots = uint64_t(8) << 20;
  int finish_bpc = 0;              // wf_finish blocks per CU
  // Pipelined one-frame calls (rt_set_pipeline, depth D = 2): one-frame call k runs as a single
  // group on stream aux[1 + p], p = k mod D, with path-state set wfg[p], camera table p and frame
  // table ft[1 + p], so call k+1's early passes fill the CUs that call k's latency-bound finisher
  // leaves idle.  Only the blend waits for the caller's stream (history, frame order); the caller's
  // stream still joins each call at its end.  set_free[p]: the last call on set p has finished;
  // batch_done: the last batched (non-pipelined) call has finished.
  // rt_tonemap_async: display passes read back into pinned host slots, fetched later
  static constexpr int DISP_SLOTS = 4;
  struct DisplaySlot {
    uint8_t* host = nullptr;
    size_t cap = 0, bytes = 0;
    hipEvent_t ev = nullptr;
  };
  DisplaySlot disp[DISP_SLOTS];
  int pipe_depth = 1;
  int pipe_next = 0;
  size_t pipe_nomem_slots = SIZE_MAX;  // pipelined batches this large did not fit twice
  // a pipelined call's finisher runs 2 of its 3 resident blocks per CU, leaving room for the next
  // call's passes: C3 1080p back-to-back 2.33 -> 2.10 ms (1 block: the same; synchronised 3.33 ->
  // 3.24 ms, 1 block 3.50)
  int pipe_finish_bpc = 2;
  int pipe_finish_pass = -1;  // -1: finish_pass
  hipEvent_t set_free[MAX_GROUPS] = {};
  hipEvent_t batch_done = nullptr;
  // Ray queries (rt_trace_rays, rt_first_hit, rt_pick; rt_query.h): buffers of their own, apart from
  // the render's path-state sets (a pipelined render call queued after a query starts its passes
  // while the query still runs), allocated on first use for at most one chunk of rays
  struct Query {
    void* mem = nullptr;
    size_t cap = 0;              // rays the buffers hold
    rtd::WFState S{};            // ra / rb (sa / sb, cam alias them), queue[0], res, cnt
    float* d_in = nullptr;       // staged caller rays of the host entry points (rt_ray)
    float4* d_out = nullptr;     // staged results (rt_hit, or int32 any-hit answers)
    float* d_zero = nullptr;     // one 0.0f: KParams::rand_origin of the camera trace (read, unused)
    int2* d_ovf = nullptr;       // the traversal's overflow stack of the query launches
    size_t ovf_bytes = 0;
  } q;
  // The display denoiser (rt_denoise*; rt_denoise.h): frame-order buffers of W*H pixels, allocated
  // on first use, dropped by a resize (the next call allocates the new size) and by rt_destroy
  struct Denoise {
    void* mem = nullptr;
    float4* col[2] = {nullptr, nullptr};  // ping-pong colour {r, g, b, k}
    float4* g0 = nullptr;                 // guides {N.xyz, bits(M or -1)}
    float4* g1 = nullptr;                 //        {P.xyz, 1/t}
    float4* hits = nullptr;               // the library's own first-hit frame (rt_hit, local-tile layout)
    float* out = nullptr;                 // the output frame, W*H*3 floats
    bool guides = false;                  // g0 / g1 hold a denoise or temporal call's guides for the current size
  } dn;
  // The display history (rt_temporal*; rt_temporal.h), allocated by the first temporal call,
  // dropped with the denoiser's buffers.  Nothing is copied when a call's output becomes the
  // history: the colour frames and the guide pairs change roles.  dn.g0 / dn.g1 are the current
  // guides and point at one of the three pairs (gp[0] is the denoiser's own); a fresh pack goes to
  // a pair that neither the history nor a live candidate holds.
  struct Temporal {
    void* mem = nullptr;
    float4* col[2] = {nullptr, nullptr};  // {r, g, b, n}: the history and the candidate (the last output)
    float4* gp[3][2] = {};                // guide pairs {g0, g1}
    float* out = nullptr;                 // the output frame, W*H*3 floats
    int hist = -1, cand = -1;             // index into col; -1: none
    int hist_g = -1, cand_g = -1;         // their guide pairs
    rt_frame_params hist_fp{}, cand_fp{}; // the cameras they were seen from
    long long pose_gen[2] = {-1, -1};     // motion mode: the geometry generation Motion's pose slot of col[k] holds; -1: none
    void drop() {
      hist = cand = hist_g = cand_g = -1;
      pose_gen[0] = pose_gen[1] = -1;
    }
  } tp;
  // The motion mode of the display history (rt_temporal_set_motion; dvl::Poses, dvl::TriFrames):
  // nothing of it exists while the mode is off.  Pose slot k goes with tp.col[k] (it follows its frame
  // through ADVANCE with the index) and is filled, once per generation and slot, by the temporal call
  // that writes that frame; triangle frame k goes with guide pair k and is written by a fresh pack.
  struct Motion {
    bool on = false;                      // survives rt_set_scene and rt_resize
    long long gen = 0;                    // the geometry generation: rt_update_geometry(_device) with count > 0
    void* pose_mem = nullptr;             // for n_tri triangles: freed by rt_set_scene
    float4* tri[2] = {nullptr, nullptr};
    float4* trin[2] = {nullptr, nullptr};
    void* tf_mem = nullptr;               // for W*H pixels: freed by a resize
    int* tf[3] = {nullptr, nullptr, nullptr};
    bool tf_valid[3] = {false, false, false};  // the pair's guides were packed with its triangle frame
  } mo;
  // The variance mode of the display chain (rt_variance_set; dvl::Variance): nothing of it exists
  // while the mode is off.  State frame k goes with tp.col[k], like Motion's pose slot.
  struct Variance {
    rt_variance_params p{0, 1.5f, 64, 0};  // survives rt_set_scene and rt_resize
    void* mem = nullptr;                  // for W*H pixels: freed by a resize
    float4* st[2] = {nullptr, nullptr};   // {l_prev, S_prev, v, m} beside tp.col[k]
    float* tvar = nullptr;                // the variance of tp.out
    float* dvar[2] = {nullptr, nullptr};  // the denoiser's ping-pong pair
    bool tvar_valid = false;              // tvar describes what tp.out holds
    const float* last = nullptr;          // the last output's variance (rt_variance_frame)
  } vr;
};

namespace {

// Development settings (measurement and test builds only).  The release library honours only the
// C-ABI (include/rt_abi.h); `make` also builds lib/librtamd_dev.so with -DRT_DEV, where these
// environment variables reach the code they name: the test-only culling switch of
// tests/test_gpu_cull.py (RT_CULL_EPS_SCALE), the traversal-structure variants the parity tests
// cover (RT_BVH_WIDTH, RT_REBUILD, RT_COLLAPSE, RT_QBFS) and the occupancy / grouping / finisher
// parameters the A/B tools sweep.
// rt_ctx::mats_emissive of a material table (32 floats per material, the emission first)
inline bool table_emissive(const std::vector<float>& t) {
  for (size_t k = 0; k + 32 <= t.size(); k += 32) {
    uint32_t b[3];
    memcpy(b, &t[k], sizeof(b));
    if (b[0] | b[1] | b[2]) return true;
  }
  return false;
}
inline const char* knob(const char* name) {
#ifdef RT_DEV
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

int fail(rt_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPCHK(ctx, call)                                                                        \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return fail((ctx), RT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));         \
  } while (0)

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

// The scene compiler's records are uploaded as the device's (scene_compile.h, rt_device.h)
static_assert(sizeof(scn::BNode) == sizeof(GNode) && offsetof(scn::BNode, box) == offsetof(GNode, b0) &&
              offsetof(scn::BNode, box[4]) == offsetof(GNode, b1) && offsetof(scn::BNode, box[8]) == offsetof(GNode, b2) &&
              offsetof(scn::BNode, ref) == offsetof(GNode, ref), "scn::BNode is rtd::GNode");
static_assert(sizeof(scn::WNode) == sizeof(rtd::QNode) && offsetof(scn::WNode, lo) == offsetof(rtd::QNode, lox) &&
              offsetof(scn::WNode, lo[1]) == offsetof(rtd::QNode, loy) && offsetof(scn::WNode, lo[2]) == offsetof(rtd::QNode, loz) &&
              offsetof(scn::WNode, hi) == offsetof(rtd::QNode, hix) && offsetof(scn::WNode, hi[1]) == offsetof(rtd::QNode, hiy) &&
              offsetof(scn::WNode, hi[2]) == offsetof(rtd::QNode, hiz) && offsetof(scn::WNode, ref) == offsetof(rtd::QNode, ref) &&
              offsetof(scn::WNode, pad) == offsetof(rtd::QNode, pad), "scn::WNode is rtd::QNode");

// The traversal-structure variants the parity tests cover (development builds; the release
// library compiles every scene with the defaults)
scn::Options scene_options() {
  scn::Options o;
  if (const char* e = knob("RT_REBUILD")) o.rebuild = atoi(e) != 0;
  if (const char* e = knob("RT_COLLAPSE")) o.greedy = strcmp(e, "greedy") == 0;
  if (const char* e = knob("RT_QBFS")) o.bfs = atoi(e) != 0;
  if (const char* e = knob("RT_BVH_WIDTH")) o.wide = atoi(e) != 2;
  return o;
}

// One block for a carved layout (dev_layout.h): RT_ERR_NOMEM with `what` when HBM cannot hold it
int alloc_block(rt_ctx* c, void*& mem, size_t bytes, const char* what) {
  const hipError_t me = hipMalloc(&mem, bytes);
  if (me == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    mem = nullptr;
    return fail(c, RT_ERR_NOMEM, what);
  }
  HIPCHK(c, me);
  return RT_OK;
}
// p = the array of a layout at `at`
template <typename P>
void place(P& p, void* base, dvl::Span at) {
  p = (P)(static_cast<char*>(base) + at.off);
}

int upload(rt_ctx* c, void** dst, const void* src, size_t bytes) {
  if (*dst) { (void)hipFree(*dst); *dst = nullptr; }
  if (bytes == 0) return RT_OK;
  HIPCHK(c, hipMalloc(dst, bytes));
  HIPCHK(c, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return RT_OK;
}

// Renders in flight read the scene, environment and pixel buffers: an entry point that replaces
// them first waits for them (the caller's stream joins every render call, pipelined ones too)
int drain(rt_ctx* c) {
  if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int occupancy(rt_ctx* c) {
  int lds = c->stack_entries * 256 * 8;
  int bpc = 0;
  HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, rtd::rt_path_kernel<false>, 256, lds));
  c->blocks_per_cu = std::max(1, bpc);
  c->block_lds = lds;
  // wavefront traversal: short LDS stack + global overflow
  int kl = 8;  // 16 KiB per block: LDS leaves room for 8 waves/SIMD (12 entries: 6; C3 5853 -> 5959 at 10, 6155 at 8 with the dual schedule at 8 waves)
  if (const char* e = knob("RT_LDS_STACK")) kl = atoi(e);
  if (const char* e = knob("RT_SPLIT_KINDS")) c->split_kinds = atoi(e);
  if (const char* e = knob("RT_SPLIT_PASSES")) c->split_passes = atoi(e);
  kl = std::max(1, std::min(kl, std::max(c->stack_entries, c->qstack_entries)));
  c->trace_lds_entries = kl;
  c->trace_lds = kl * 256 * 8;
  bpc = 0;
  // persistent grids: as many blocks as can be resident (the camera pass's instantiation and the
  // secondary passes' one may differ in registers)
  auto occ = [&](bool cam) {
    int b = 0;
    const hipError_t e =
        cam ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, rtd::wf_trace<false, true, true>, 256, c->trace_lds)
            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, rtd::wf_trace<false, true, false>, 256, c->trace_lds);
    return e == hipSuccess ? std::max(1, b) : 1;
  };
  c->trace_bpc0 = occ(true);  // pass 0 is the implicit camera pass
  c->trace_bpc = occ(false);
  bpc = c->trace_bpc;
  if (const char* e = knob("RT_TRACE_BPC")) c->trace_bpc0 = c->trace_bpc = std::max(1, atoi(e));
  if (const char* e = knob("RT_POOL_CHUNK")) c->pool_chunk = std::max(64, atoi(e) / 64 * 64);
  if (knob("RT_DEBUG"))
    fprintf(stderr, "[rt] trace: lds entries %d (%d B/block), occupancy API %d blocks/CU, using %d (pass 0: %d); "
            "megakernel %d\n", kl, c->trace_lds, bpc, c->trace_bpc, c->trace_bpc0, c->blocks_per_cu);
  {
    int b = 0;
    const hipError_t e = c->wide
        ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, rtd::wf_finish<true, true>, 256, c->trace_lds)
        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, rtd::wf_finish<true, false>, 256, c->trace_lds);
    // the finisher's lanes index the traversal overflow column: never more than the trace grid
    c->finish_bpc = std::max(1, std::min(e == hipSuccess ? b : 1, std::max(c->trace_bpc, c->trace_bpc0)));
    if (const char* fe = knob("RT_FINISH_BPC")) c->finish_bpc = std::max(1, std::min(c->finish_bpc, atoi(fe)));
    c->pipe_finish_bpc = 2;
    if (const char* fe = knob("RT_PIPE_FINISH_BPC")) c->pipe_finish_bpc = std::max(1, atoi(fe));
    c->pipe_finish_bpc = std::min(c->pipe_finish_bpc, c->finish_bpc);
    if (knob("RT_DEBUG"))
      fprintf(stderr, "[rt] wf_finish: occupancy API %d blocks/CU, using %d (pipelined calls %d)\n", b, c->finish_bpc,
              c->pipe_finish_bpc);
  }
  const size_t lanes = (size_t)c->n_cus * std::max(c->trace_bpc, c->trace_bpc0) * 256;
  const int entries = std::max(c->stack_entries, c->qstack_entries);
  const size_t need = (size_t)std::max(0, entries - kl) * lanes * sizeof(int2) * c->n_groups;
  if (need > c->stack_ovf_bytes) {
    dfree(c->d_stack_ovf);
    HIPCHK(c, hipMalloc(&c->d_stack_ovf, need));
    c->stack_ovf_bytes = need;
  }
  return RT_OK;
}

// The traversal stack's overflow indices, checked on the host before every launch that uses them
// (DESIGN.md §4, round 5): entry j in [KL, entries) of grid lane l of path-state set `set` lives at
// element set * ovf_group + (j - KL) * ovf_lanes + l, with ovf_lanes = trace grid blocks * 256 and
// l below that (the finisher's grid is never larger than the trace grid); a lane-quad move copies
// at most `entries` = the deepest stack of the scene's trees (3 * qdepth + 2 for the 4-wide one),
// passed to the kernels as KParams::stack_cap.
std::string ovf_layout_error(const rt_ctx* c, int set, unsigned int trace_grid_blocks) {
  const int entries = std::max(c->stack_entries, c->qstack_entries);
  const int kl = c->trace_lds_entries;
  const size_t rows = (size_t)std::max(0, entries - kl);
  const size_t lanes = (size_t)trace_grid_blocks * 256u;
  const size_t per_set = c->stack_ovf_bytes / sizeof(int2) / (size_t)std::max(1, c->n_groups);
  char buf[256];
  if (set < 0 || set >= c->n_groups) {
    snprintf(buf, sizeof buf, "overflow stack: path-state set %d of %d", set, c->n_groups);
    return buf;
  }
  if (rows > 0 && (!c->d_stack_ovf || rows * lanes > per_set)) {
    snprintf(buf, sizeof buf, "overflow stack: %zu rows x %zu lanes exceed %zu entries per set", rows, lanes, per_set);
    return buf;
  }
  if ((unsigned)(c->finish_bpc * c->n_cus) > trace_grid_blocks || c->pipe_finish_bpc > c->finish_bpc) {
    snprintf(buf, sizeof buf, "overflow stack: finisher grid %d x %d above the trace grid %u", c->finish_bpc,
             c->n_cus, trace_grid_blocks);
    return buf;
  }
  return std::string();
}

// One wf_trace launch: rpl::Trace names the instantiation (render_plan.h has what each is for)
void launch_trace(rt_ctx* c, int trace, dim3 grid, const rtd::WFParams& WP, hipStream_t st) {
#define RT_TRACE(name, ...) \
  case rpl::name: hipLaunchKernelGGL((rtd::wf_trace<__VA_ARGS__>), grid, dim3(256), c->trace_lds, st, WP); break
  switch (trace) {
    RT_TRACE(CAM_SMALL, false, true, true, true);
    RT_TRACE(P1_SMALL, false, true, false, true, true);
    RT_TRACE(REG_SMALL, false, true, false, true);
    RT_TRACE(P1_SHADOW, false, true, false, false, true, 2);
    RT_TRACE(P1_CONT_LEAN, false, true, false, false, true, 1, true);
    RT_TRACE(P1_CONT, false, true, false, false, true, 1);
    RT_TRACE(SHADOW, false, true, false, false, false, 2);
    RT_TRACE(CONT, false, true, false, false, false, 1);
    RT_TRACE(CAM_CW, true, true, true);
    RT_TRACE(P1_CW, true, true, false, false, true);
    RT_TRACE(REG_CW, true, true, false);
    RT_TRACE(CAM_CB, true, false, true);
    RT_TRACE(P1_CB, true, false, false, false, true);
    RT_TRACE(REG_CB, true, false, false);
    RT_TRACE(CAM_W, false, true, true);
    RT_TRACE(P1_W, false, true, false, false, true);
    RT_TRACE(REG_W, false, true, false);
    RT_TRACE(CAM_B, false, false, true);
    RT_TRACE(P1_B, false, false, false, false, true);
    RT_TRACE(REG_B, false, false, false);
  }
#undef RT_TRACE
}

// One wf_shade launch: rpl::Shade x the integrator
void launch_shade(int shade, bool bsdf, dim3 grid, hipStream_t st, const rtd::WFParams& WP) {
#define RT_SHADE(name, BSDF, ...) \
  case 2 * rpl::name + BSDF: hipLaunchKernelGGL((rtd::wf_shade<BSDF, __VA_ARGS__>), grid, dim3(256), 0, st, WP); break
  switch (2 * shade + (bsdf ? 1 : 0)) {
    RT_SHADE(FUSED, true, true);
    RT_SHADE(CAM, true, false, rtd::SH_SUB_CAM, true);
    RT_SHADE(CAM_LEAN, true, false, rtd::SH_SUB_CAM, true, true);
    RT_SHADE(BULK_LEAN, true, false, rtd::SH_SUB_BULK, false, true);
    RT_SHADE(BULK, true, false, rtd::SH_SUB_BULK);
    RT_SHADE(PLAIN, true, false);
    RT_SHADE(FUSED, false, true);
    RT_SHADE(CAM, false, false, rtd::SH_SUB_CAM, true);
    RT_SHADE(CAM_LEAN, false, false, rtd::SH_SUB_CAM, true, true);
    RT_SHADE(BULK_LEAN, false, false, rtd::SH_SUB_BULK, false, true);
    RT_SHADE(BULK, false, false, rtd::SH_SUB_BULK);
    RT_SHADE(PLAIN, false, false);
  }
#undef RT_SHADE
}

// wf_finish: one lane per remaining path, trace + shade until the path ends
void launch_finish(rt_ctx* c, bool bsdf, dim3 grid, hipStream_t st, const rtd::WFParams& WP) {
  if (bsdf && c->wide) hipLaunchKernelGGL((rtd::wf_finish<true, true>), grid, dim3(256), c->trace_lds, st, WP);
  else if (bsdf) hipLaunchKernelGGL((rtd::wf_finish<true, false>), grid, dim3(256), c->trace_lds, st, WP);
  else if (c->wide) hipLaunchKernelGGL((rtd::wf_finish<false, true>), grid, dim3(256), c->trace_lds, st, WP);
  else hipLaunchKernelGGL((rtd::wf_finish<false, false>), grid, dim3(256), c->trace_lds, st, WP);
}

hipEvent_t take_event(rt_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
#define TAKE_EVENT(ctx, ev)                                                                      \
  do {                                                                                           \
    (ev) = take_event(ctx);                                                                      \
    if (!(ev)) return fail((ctx), RT_ERR_HIP, "hipEventCreate failed");                          \
  } while (0)

// Timing events of launches not yet folded into kernel_ms / trace_ms: a front end that never
// calls rt_synchronize (it waits on its own stream or events) would otherwise grow these lists
// without bound.  Past `cap` pending pairs, the oldest are waited for, folded and recycled.
// a finished render call's (start, end) events: its duration into acc_ms
int fold_pair(rt_ctx* c, const std::pair<hipEvent_t, hipEvent_t>& e, double& acc_ms) {
  float ms = 0.0f;
  HIPCHK(c, hipEventElapsedTime(&ms, e.first, e.second));
  acc_ms += ms;
  c->event_pool.push_back(e.first);
  c->event_pool.push_back(e.second);
  return RT_OK;
}
// a finished traversal launch: its duration into trace_ms and its interval into the union
// (rt_ctx::busy; pairs arrive in queue order)
int fold_trace(rt_ctx* c, const rt_ctx::TraceEv& e) {
  float ms = 0.0f, a = 0.0f;
  HIPCHK(c, hipEventElapsedTime(&ms, e.s, e.e));
  c->trace_ms += ms;
  if (c->busy_anchor) HIPCHK(c, hipEventElapsedTime(&a, c->busy_anchor, e.s));
  double lo = c->busy_anchor_t + (double)a, hi = lo + (double)std::max(ms, 0.0f);
  if (c->busy_anchor) c->event_pool.push_back(c->busy_anchor);
  c->busy_anchor = e.s;  // this launch's start is the next one's reference
  c->busy_anchor_t = lo;
  c->event_pool.push_back(e.e);
  auto& v = c->busy;
  // close what no pending launch can overlap any more (calls <= e.call - 2)
  size_t keep = 0;
  for (const auto& iv : v) {
    if (iv.call + 2 <= e.call) c->busy_closed_ms += iv.hi - iv.lo;
    else v[keep++] = iv;
  }
  v.resize(keep);
  // merge [lo, hi] into the sorted disjoint list
  uint64_t call = e.call;
  auto it = std::upper_bound(v.begin(), v.end(), lo, [](double x, const rt_ctx::BusyIv& iv) { return x < iv.lo; });
  if (it != v.begin() && std::prev(it)->hi >= lo) {
    --it;
    lo = it->lo;
    hi = std::max(hi, it->hi);
    call = std::max(call, it->call);
    it = v.erase(it);
  }
  while (it != v.end() && it->lo <= hi) {
    hi = std::max(hi, it->hi);
    call = std::max(call, it->call);
    it = v.erase(it);
  }
  v.insert(it, rt_ctx::BusyIv{lo, hi, call});
  return RT_OK;
}

// Past `cap` pending pairs, the oldest are waited for, folded and recycled.  Pairs of one call can
// sit on different streams (frame / pixel groups, pipelined sets), so each pair is waited for
// itself (in queue order: cheap once the first is done).
int fold_events(rt_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& ev, double& acc_ms, size_t cap) {
  if (ev.size() <= cap) return RT_OK;
  const size_t n = ev.size() - cap / 2;
  for (size_t i = 0; i < n; i++) {
    HIPCHK(c, hipEventSynchronize(ev[i].second));
    const int rc = fold_pair(c, ev[i], acc_ms);
    if (rc) return rc;
  }
  ev.erase(ev.begin(), ev.begin() + (ptrdiff_t)n);
  return RT_OK;
}
int fold_trace_events(rt_ctx* c, size_t cap) {
  auto& ev = c->trace_events;
  if (ev.size() <= cap) return RT_OK;
  const size_t n = ev.size() - cap / 2;
  for (size_t i = 0; i < n; i++) {
    HIPCHK(c, hipEventSynchronize(ev[i].e));
    const int rc = fold_trace(c, ev[i]);
    if (rc) return rc;
  }
  ev.erase(ev.begin(), ev.begin() + (ptrdiff_t)n);
  return RT_OK;
}
constexpr size_t kMaxPendingEvents = 4096;

// Frames in flight per launch = path-state budget / pixels of this rank.  The state grows on
// demand in reserve_path_state, so interactive 1-frame use stays small.  More frames per launch
// amortise the per-pass latency floor of the few longest rays (C3 1080p: 16 frames 1.07, 64
// frames 0.94 ms/frame; 161 vs 80 frames +1.8%, all 512 of a bench step at once +2.2%).
void update_frames_cap(rt_ctx* c, size_t nv) {
  size_t max_slots = size_t(320) << 20;  // 184 B each: 62 GB of the 288 GB HBM3E
  if (const char* e = knob("RT_MAX_SLOTS")) max_slots = (size_t)strtoull(e, nullptr, 10);
  if (c->max_slots_req) max_slots = c->max_slots_req;
  c->frames_cap = (int)std::max<size_t>(1, std::min<size_t>(RT_MAX_FRAMES_PER_LAUNCH, max_slots / std::max<size_t>(1, nv)));
}

// Path-state buffers of the wavefront path: `paths` slots for each of the n_groups frame groups
// and each set's row arena, laid out by dvl::path_state and dvl::arena.  RT_ERR_NOMEM when HBM
// cannot hold them (the caller then runs fewer frames at a time).
static_assert(rt_ctx::MAX_GROUPS <= 4, "rtd::GroupCounters holds 4 groups' counters");
// dev_layout.h cannot see the kernels' types: its element sizes are theirs
constexpr rtd::WFState* kWF = nullptr;  // (sizeof operands only)
constexpr size_t slot_b(dvl::Slot s) { return dvl::kSlot[s].bytes; }
constexpr size_t row_b(dvl::Row r) { return dvl::kArena[r].bytes; }
static_assert(slot_b(dvl::S0) == sizeof(*kWF->s0) && slot_b(dvl::S1) == sizeof(*kWF->s1) && slot_b(dvl::S2) == sizeof(*kWF->s2) &&
              slot_b(dvl::S3) == sizeof(*kWF->s3) && slot_b(dvl::S4) == sizeof(*kWF->s4) && slot_b(dvl::S5) == sizeof(*kWF->s5) &&
              slot_b(dvl::RA) == sizeof(*kWF->ra) && slot_b(dvl::RB) == sizeof(*kWF->rb) && slot_b(dvl::SA) == sizeof(*kWF->sa) &&
              slot_b(dvl::SB) == sizeof(*kWF->sb) && slot_b(dvl::RES) == 2 * sizeof(*kWF->res) && slot_b(dvl::FIN) == sizeof(*kWF->fin) &&
              slot_b(dvl::QUEUE0) == 2 * sizeof(*kWF->queue[0]) && slot_b(dvl::QUEUE1) == 2 * sizeof(*kWF->queue[1]) &&
              slot_b(dvl::ACTIVE0) == sizeof(*kWF->active[0]) && slot_b(dvl::ACTIVE1) == sizeof(*kWF->active[1]) &&
              sizeof(*kWF->hit) == 4 && sizeof(*kWF->cnt) == 4 && dvl::kCntWords == rtd::kCntWords,
              "dvl::kSlot holds the element sizes of rtd::WFState's slot arrays");
static_assert(row_b(dvl::A_S0) == sizeof(*kWF->s0) && row_b(dvl::A_S1) == sizeof(*kWF->s1) && row_b(dvl::A_S2) == sizeof(*kWF->s2) &&
              row_b(dvl::A_S3) == sizeof(*kWF->s3) && row_b(dvl::A_S4) == sizeof(*kWF->s4) && row_b(dvl::A_S5) == sizeof(*kWF->s5) &&
              row_b(dvl::A_RA) == sizeof(*kWF->ra) && row_b(dvl::A_RB) == sizeof(*kWF->rb) && row_b(dvl::A_SA) == sizeof(*kWF->sa) &&
              row_b(dvl::A_SB) == sizeof(*kWF->sb) && row_b(dvl::A_RES) == 2 * sizeof(*kWF->res) && row_b(dvl::A_RPATH) == sizeof(*kWF->rpath),
              "dvl::kArena holds the element sizes of the row arena's arrays");
static_assert(dvl::kRayBytes == sizeof(rt_ray) && dvl::kHitBytes == sizeof(rt_hit), "dvl's staging records are rt_abi.h's");
int alloc_wavefront(rt_ctx* c, size_t paths) {
  if (c->wf_mem && c->wf_paths >= paths) return RT_OK;
  if (c->wf_mem) {  // grow: earlier launches on the streams may still read the old state
    HIPCHK(c, hipDeviceSynchronize());
    (void)hipFree(c->wf_mem);
    c->wf_mem = nullptr;
  }
  const dvl::PathState L = dvl::path_state(paths, c->n_groups);
  const dvl::Arena A = dvl::arena(L);
  if (int rc = alloc_block(c, c->wf_mem, L.total, "path state does not fit in device memory")) {
    if (rc == RT_ERR_NOMEM) c->wf_paths = 0;
    return rc;
  }
  for (int g = 0; g < c->n_groups; g++) {
    char* const set = static_cast<char*>(c->wf_mem) + L.set(g);
    rtd::WFState& w = c->wfg[g];
    auto slot = [&](auto& p, dvl::Slot s) { place(p, set, L.arr[s]); };
    slot(w.s0, dvl::S0); slot(w.s1, dvl::S1); slot(w.s2, dvl::S2); slot(w.s3, dvl::S3); slot(w.s4, dvl::S4); slot(w.s5, dvl::S5);
    slot(w.ra, dvl::RA); slot(w.rb, dvl::RB); slot(w.sa, dvl::SA); slot(w.sb, dvl::SB);
    slot(w.res, dvl::RES); slot(w.fin, dvl::FIN);
    for (int k = 0; k < 2; k++) {
      slot(w.queue[k], dvl::Slot(dvl::QUEUE0 + k));
      place(w.queue_s[k], set, L.queue_s[k]);
      slot(w.active[k], dvl::Slot(dvl::ACTIVE0 + k));
    }
    place(w.hit, set, L.hit);
    place(w.cnt, set, L.cnt);
    // the row arena: its own rows of the path state, everything else as the slot-indexed state
    rtd::WFState& a = c->wfa[g];
    a = w;
    auto row = [&](auto& p, dvl::Row r) { place(p, set, A.arr[r]); };
    row(a.s0, dvl::A_S0); row(a.s1, dvl::A_S1); row(a.s2, dvl::A_S2); row(a.s3, dvl::A_S3); row(a.s4, dvl::A_S4); row(a.s5, dvl::A_S5);
    row(a.ra, dvl::A_RA); row(a.rb, dvl::A_RB); row(a.sa, dvl::A_SA); row(a.sb, dvl::A_SB);
    row(a.res, dvl::A_RES); row(a.rpath, dvl::A_RPATH);
  }
  c->wf_rows = A.rows;
  c->wf_paths = L.slots;
  c->wf_hit_cap = L.hit_cap;
  return RT_OK;
}

// The refit schedule of rt_update_geometry (the next update builds the current tree's)
void geo_drop(rt_ctx* c) {
  rt_ctx::Geometry& g = c->geo;
  dfree(g.d_leaves); dfree(g.d_blist); dfree(g.d_boff); dfree(g.d_qlist); dfree(g.d_qoff);
  g.n_leaves = 0;
  g.boff.clear();
  g.qoff.clear();
  g.planned = false;
}

// The motion mode's two allocations (rt_ctx::Motion): the poses of the display history's frames, and
// the triangle frames of the guide pairs.  The callers have drained the context.
void motion_free_poses(rt_ctx* c) {
  rt_ctx::Motion& m = c->mo;
  if (m.pose_mem) (void)hipFree(m.pose_mem);
  m.pose_mem = nullptr;
  c->tp.pose_gen[0] = c->tp.pose_gen[1] = -1;
}
void motion_free_frames(rt_ctx* c) {
  rt_ctx::Motion& m = c->mo;
  if (m.tf_mem) (void)hipFree(m.tf_mem);
  m.tf_mem = nullptr;
  for (bool& v : m.tf_valid) v = false;
}
// The variance mode's allocation (rt_ctx::Variance), the setting kept
void variance_free(rt_ctx* c) {
  rt_ctx::Variance& v = c->vr;
  if (v.mem) (void)hipFree(v.mem);
  v.mem = nullptr;
  v.tvar_valid = false;
  v.last = nullptr;
}

// ---- rt_update_geometry (rt_geometry.h; the definition is scn::update_geometry)
// The refit schedule and the reduction cell, on the first update after a rt_set_scene: the node
// arrays come from the device, so a context that never updates geometry keeps no copy of them
int geo_prepare(rt_ctx* c) {
  rt_ctx::Geometry& g = c->geo;
  if (!g.d_red) HIPCHK(c, hipMalloc(&g.d_red, sizeof(rtg::Red)));
  if (g.planned) return RT_OK;
  std::vector<scn::BNode> nodes((size_t)c->n_nodes);
  std::vector<scn::WNode> qnodes((size_t)c->n_qnodes);
  HIPCHK(c, hipMemcpy(nodes.data(), c->d_nodes, nodes.size() * sizeof(scn::BNode), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(qnodes.data(), c->d_qnodes, qnodes.size() * sizeof(scn::WNode), hipMemcpyDeviceToHost));
  const scn::RefitPlan P = scn::refit_plan(nodes.data(), nodes.size(), c->root, qnodes.data(), qnodes.size(), c->qroot,
                                           c->qbuilt, c->has_scene != 0, c->n_tri);
  int rc;
  if ((rc = upload(c, (void**)&g.d_leaves, P.leaves.data(), P.leaves.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(c, (void**)&g.d_blist, P.blist.data(), P.blist.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(c, (void**)&g.d_boff, P.boff.data(), P.boff.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(c, (void**)&g.d_qlist, P.qlist.data(), P.qlist.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(c, (void**)&g.d_qoff, P.qoff.data(), P.qoff.size() * sizeof(int32_t)))) return rc;
  g.n_leaves = (int)(P.leaves.size() / 4);
  g.boff = P.boff;
  g.qoff = P.qoff;
  g.planned = true;
  return RT_OK;
}

// The internal nodes of one tree, lowest height first: one launch per height, and one
// single-workgroup launch for the top heights from the first one on after which every height's
// nodes fit a workgroup
template <typename Node, typename Kernel>
void geo_refit_tree(rt_ctx* c, Kernel kernel, Node* nodes, const int* d_list, const int* d_off,
                           const std::vector<int32_t>& off) {
  const int H = (int)off.size() - 1;  // heights 1 .. H
  int top = H + 1;
  while (top > 1 && off[top - 1] - off[top - 2] <= 256) top--;
  for (int h = 1; h < top; h++)
    hipLaunchKernelGGL(kernel, dim3((off[h] - off[h - 1] + 255) / 256), dim3(256), 0, c->stream, nodes, d_list, d_off, h,
                       h + 1);
  if (top <= H) hipLaunchKernelGGL(kernel, dim3(1), dim3(256), 0, c->stream, nodes, d_list, d_off, top, H + 1);
}

}  // namespace

extern "C" {

int rt_create(int hip_device, rt_ctx** out) {
  if (!out) return RT_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RT_ERR_NODEVICE;
  if (hip_device < 0 || hip_device >= n) return RT_ERR_NODEVICE;
  rt_ctx* c = new (std::nothrow) rt_ctx();
  if (!c) return RT_ERR_NOMEM;
  c->device = hip_device;
  if (hipSetDevice(hip_device) != hipSuccess) { delete c; return RT_ERR_HIP; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, hip_device) != hipSuccess) { delete c; return RT_ERR_HIP; }
  c->n_cus = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return RT_ERR_HIP; }
  c->own_stream = true;
  if (const char* e = knob("RT_GROUPS")) c->n_groups = std::max(1, std::min(rt_ctx::MAX_GROUPS, atoi(e)));
  if (const char* e = knob("RT_FINISH_PASS")) c->finish_pass = std::max(0, atoi(e));
  if (const char* e = knob("RT_PIPE_FINISH_PASS")) c->pipe_finish_pass = std::max(0, atoi(e));
  if (const char* e = knob("RT_FINISH_SLOTS")) c->finish_slots = (uint64_t)strtoull(e, nullptr, 10);
  if (hipMalloc(&c->d_counter, 64) != hipSuccess || hipMalloc(&c->d_stats, rtd::kStatWords * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->d_stats, 0, rtd::kStatWords * sizeof(unsigned long long)) != hipSuccess) {
    rt_destroy(c);
    return RT_ERR_HIP;
  }
  *out = c;
  return RT_OK;
}

int rt_destroy(rt_ctx* c) {
  if (!c) return RT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& a : c->aux) if (a) (void)hipStreamSynchronize(a);
  for (auto& e : c->events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (auto& e : c->set_free) if (e) (void)hipEventDestroy(e);
  if (c->batch_done) (void)hipEventDestroy(c->batch_done);
  if (c->busy_anchor) (void)hipEventDestroy(c->busy_anchor);
  dfree(c->d_nodes); dfree(c->d_qnodes); dfree(c->d_tri); dfree(c->d_trx); dfree(c->d_trin); dfree(c->d_hrec); dfree(c->d_mats);
  for (auto& t : c->light) {
    dfree(t.d);
    if (t.last_use) (void)hipEventDestroy(t.last_use);
    if (t.built) (void)hipEventDestroy(t.built);
  }
  geo_drop(c);
  dfree(c->geo.d_red); dfree(c->geo.d_stage);
  dfree(c->d_hdr); dfree(c->d_cache); dfree(c->d_accum); dfree(c->d_counter); dfree(c->d_stats);
  for (auto& e : c->trace_events) { (void)hipEventDestroy(e.s); (void)hipEventDestroy(e.e); }
  for (auto e : c->event_pool) (void)hipEventDestroy(e);
  if (c->wf_mem) (void)hipFree(c->wf_mem);
  for (auto& a : c->aux) if (a) (void)hipStreamDestroy(a);
  for (auto& d : c->disp) {
    if (d.ev) (void)hipEventDestroy(d.ev);
    if (d.host) (void)hipHostFree(d.host);
  }
  for (auto& t : c->ft) {
    if (t.ev) (void)hipEventDestroy(t.ev);
    if (t.h) (void)hipHostFree(t.h);
    dfree(t.d);
  }
  dfree(c->d_pix);
  dfree(c->d_tile_ids);
  dfree(c->d_tile_src);
  dfree(c->d_tile_cost);
  dfree(c->d_cam);
  dfree(c->d_stack_ovf);
  if (c->q.mem) (void)hipFree(c->q.mem);
  dfree(c->q.d_ovf);
  if (c->dn.mem) (void)hipFree(c->dn.mem);
  if (c->tp.mem) (void)hipFree(c->tp.mem);
  motion_free_poses(c);
  motion_free_frames(c);
  variance_free(c);
  dfree(c->d_disp);
  dfree(c->d_gather);
  for (auto& m : c->rccl_comms) (void)ncclCommDestroy(m);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return RT_OK;
}

const char* rt_last_error(const rt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int rt_device_info(const rt_ctx* c, int32_t* n_cus, int32_t* blocks_per_cu, int32_t* lds_bytes_per_block) {
  if (!c) return RT_ERR_ARG;
  if (n_cus) *n_cus = c->n_cus;
  if (blocks_per_cu) *blocks_per_cu = c->blocks_per_cu;
  if (lds_bytes_per_block) *lds_bytes_per_block = c->block_lds;
  return RT_OK;
}


int rt_set_scene(rt_ctx* c, const rt_scene_soa* s) {
  if (!c || !s) return RT_ERR_ARG;
  // a rejected scene touches neither the device nor the context
  scn::Compiled k;
  std::string why;
  if (int rc = scn::compile(s, scene_options(), k, why)) return fail(c, rc, why);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = drain(c)) return rc;
  // the old buffers no longer describe a scene from here on: a failure below leaves the context
  // without one (renders and queries then refuse) rather than with a mix of old and new buffers
  c->scene_set = false;
  c->tp.drop();  // the display history shows another scene
  c->vr.tvar_valid = false;  // (and so do the variance frames)
  c->vr.last = nullptr;
  motion_free_poses(c);  // (its poses are another triangle list's)
  c->mo.gen = 0;
  geo_drop(c);   // and the refit schedule is another tree's
  int rc;
  if ((rc = upload(c, (void**)&c->d_qnodes, k.qnodes.data(), k.qnodes.size() * sizeof(scn::WNode)))) return rc;
  if ((rc = upload(c, (void**)&c->d_nodes, k.nodes.data(), k.nodes.size() * sizeof(scn::BNode)))) return rc;
  if ((rc = upload(c, (void**)&c->d_tri, k.tri.data(), k.tri.size() * sizeof(float)))) return rc;
  if ((rc = upload(c, (void**)&c->d_trx, k.trx.data(), k.trx.size() * sizeof(float)))) return rc;
  if ((rc = upload(c, (void**)&c->d_trin, k.trin.data(), k.trin.size() * sizeof(float)))) return rc;
  if ((rc = upload(c, (void**)&c->d_hrec, k.hrec.data(), k.hrec.size() * sizeof(float)))) return rc;
  if ((rc = upload(c, (void**)&c->d_mats, k.mats.data(), k.mats.size() * sizeof(float)))) return rc;
  c->n_qnodes = (int)k.qnodes.size();
  c->tri_k1 = k.tri_k1; c->tri_k0 = k.tri_k0; c->tri_flagged = k.tri_flagged;
  c->n_tri = k.n_tri;
  c->n_mats = k.n_mats;
  c->root = k.root;
  c->has_scene = k.has_scene;
  c->cull_R = k.cull_R; c->cull_K = k.cull_K; c->cull_off = k.cull_off;
  c->stack_entries = std::max(2, k.depth + 1);
  c->wide = k.wide;
  c->qroot = k.qroot;
  c->qstack_entries = std::max(2, 3 * k.qdepth + 2);
  c->s_cap = k.s_cap; c->sc_cap = k.sc_cap; c->s_max = k.s_max; c->sc_max = k.sc_max; c->c_min = k.c_min;
  c->qbuilt = k.qbuilt;
  c->n_nodes = (int)k.nodes.size();
  {
    const size_t b[6] = {k.tri.size() * sizeof(float), k.trx.size() * sizeof(float), k.trin.size() * sizeof(float),
                         k.hrec.size() * sizeof(float), k.nodes.size() * sizeof(scn::BNode),
                         k.qnodes.size() * sizeof(scn::WNode)};
    std::copy(b, b + 6, c->scene_bytes);
  }
  c->tri_mat = std::move(k.tri_mat);
  c->mat_table = std::move(k.mats);
  c->mats_emissive = table_emissive(c->mat_table);
  c->scene_set = true;
  return occupancy(c);
}

int rt_set_scene_encoded(rt_ctx* c, const float* tri_enc, int32_t n_triangles, const float* node_enc, int32_t n_nodes) {
  if (!c || n_triangles < 0 || n_nodes < 0 || (n_triangles && !tri_enc) || (n_nodes && !node_enc)) return RT_ERR_ARG;
  scn::Decoded d;
  scn::decode(tri_enc, n_triangles, node_enc, n_nodes, d);
  return rt_set_scene(c, &d.soa);
}

int rt_update_materials(rt_ctx* c, int32_t first, int32_t count, const rt_material* m) {
  if (!c || !m || first < 0 || count < 0) return RT_ERR_ARG;
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "no scene");
  if ((int64_t)first + count > c->n_tri) return fail(c, RT_ERR_ARG, "range outside the triangle list");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = drain(c)) return rc;
  float packed[32];
  scn::pack_material(*m, packed);
  int id = -1;
  for (int k = 0; k < c->n_mats; k++)
    if (!memcmp(&c->mat_table[32 * k], packed, sizeof(packed))) { id = k; break; }
  if (id < 0) {
    id = c->n_mats;
    c->mat_table.resize(32 * (size_t)(id + 1));
    memcpy(&c->mat_table[32 * id], packed, sizeof(packed));
    c->n_mats++;
    c->mats_emissive = table_emissive(c->mat_table);
    int rc = upload(c, (void**)&c->d_mats, c->mat_table.data(), c->mat_table.size() * sizeof(float));
    if (rc) return rc;
  }
  for (int i = first; i < first + count; i++) c->tri_mat[i] = id;
  if (count > 0) {
    hipLaunchKernelGGL(rtd::rt_set_material_kernel, dim3((count + 255) / 256), dim3(256), 0, c->stream,
                       c->d_trin, c->d_hrec, first, count, id);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

// ---- rt_update_geometry (rt_geometry.h; the definition is scn::update_geometry)
int rt_update_geometry_device(rt_ctx* c, const void* tri_index_dev, int32_t first, int32_t count, const void* p1,
                              const void* p2, const void* p3, const void* n1, const void* n2, const void* n3) {
  if (!c) return RT_ERR_ARG;
  if (count < 0) return fail(c, RT_ERR_ARG, "negative count");
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "no scene");
  if (count == 0) return RT_OK;
  if (!p1 || !p2 || !p3 || !n1 || !n2 || !n3) return fail(c, RT_ERR_ARG, "missing vertex arrays");
  if (tri_index_dev && first != 0) return fail(c, RT_ERR_ARG, "first must be 0 with an index list");
  if (!tri_index_dev && (first < 0 || (int64_t)first + count > c->n_tri))
    return fail(c, RT_ERR_ARG, "range outside the triangle list");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = drain(c)) return rc;
  if (int rc = geo_prepare(c)) return rc;
  rt_ctx::Geometry& g = c->geo;
  auto bits = [](double x) {
    unsigned long long b;
    memcpy(&b, &x, 8);
    return b;
  };
  auto value = [](unsigned long long b) {
    double x;
    memcpy(&x, &b, 8);
    return x;
  };
  rtg::Red red{bits(c->cull_R), bits(c->cull_K), bits(c->cull_off), bits(c->s_max), bits(c->sc_max), bits(c->c_min), 0, 0};
  HIPCHK(c, hipMemcpyAsync(g.d_red, &red, sizeof(red), hipMemcpyHostToDevice, c->stream));
  const dim3 grid((count + 255) / 256), block(256);
  const int* idx = static_cast<const int*>(tri_index_dev);
  const float *q1 = static_cast<const float*>(p1), *q2 = static_cast<const float*>(p2), *q3 = static_cast<const float*>(p3);
  const float *m1 = static_cast<const float*>(n1), *m2 = static_cast<const float*>(n2), *m3 = static_cast<const float*>(n3);
  hipLaunchKernelGGL(rtg::geo_check, grid, block, 0, c->stream, idx, first, count, c->n_tri, q1, q2, q3, m1, m2, m3, c->s_cap,
                     c->sc_cap, g.d_red);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&red, g.d_red, sizeof(red), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (red.bad)  // (nothing of the scene has been written)
    return fail(c, RT_ERR_ARG, "a triangle index is out of range, a value is not finite or a position is 2^30 or more");
  hipLaunchKernelGGL(rtg::geo_record, grid, block, 0, c->stream, idx, first, count, q1, q2, q3, m1, m2, m3, c->s_cap, c->sc_cap,
                     c->d_tri, c->d_trx, c->d_trin, c->d_hrec, g.d_red);
  HIPCHK(c, hipGetLastError());
  c->dn.guides = false;  // the denoise / temporal guides show the old surfaces (the history stays: the caller resets)
  c->mo.gen++;           // a new pose: in motion mode the history follows the moved triangles from its own
  if (g.n_leaves > 0) {
    hipLaunchKernelGGL(rtg::geo_leaf, dim3((g.n_leaves + 255) / 256), block, 0, c->stream, g.d_leaves, g.n_leaves, c->d_tri,
                       reinterpret_cast<scn::BNode*>(c->d_nodes), reinterpret_cast<scn::WNode*>(c->d_qnodes));
    geo_refit_tree(c, rtg::geo_refit_b, reinterpret_cast<scn::BNode*>(c->d_nodes), g.d_blist, g.d_boff, g.boff);
    geo_refit_tree(c, rtg::geo_refit_q, reinterpret_cast<scn::WNode*>(c->d_qnodes), g.d_qlist, g.d_qoff, g.qoff);
    HIPCHK(c, hipGetLastError());
  }
  int delta = 0;
  HIPCHK(c, hipMemcpyAsync(&delta, &g.d_red->flag_delta, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // the constants the next call turns into kernel arguments (fill_scene_kparams): none shrinks
  c->cull_R = value(red.R); c->cull_K = value(red.K); c->cull_off = value(red.off);
  c->s_max = value(red.s_max); c->sc_max = value(red.sc_max); c->c_min = value(red.c_min);
  trif::Consts k;
  k.s_max = c->s_max; k.sc_max = c->sc_max; k.c_min = c->c_min;
  trif::form_margin(k);
  c->tri_k1 = k.k1; c->tri_k0 = k.k0;
  c->tri_flagged += delta;
  return RT_OK;
}

int rt_update_geometry(rt_ctx* c, const int32_t* tri_index, int32_t first, int32_t count, const float* p1, const float* p2,
                       const float* p3, const float* n1, const float* n2, const float* n3) {
  if (!c) return RT_ERR_ARG;
  if (count < 0) return fail(c, RT_ERR_ARG, "negative count");
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "no scene");
  if (count == 0) return RT_OK;
  if (!p1 || !p2 || !p3 || !n1 || !n2 || !n3) return fail(c, RT_ERR_ARG, "missing vertex arrays");
  if (tri_index) {  // (the device form cannot see a duplicate: two lanes would write one triangle)
    if (first != 0) return fail(c, RT_ERR_ARG, "first must be 0 with an index list");
    std::vector<char> seen((size_t)c->n_tri, 0);
    for (int i = 0; i < count; i++) {
      const int t = tri_index[i];
      if (t < 0 || t >= c->n_tri) return fail(c, RT_ERR_ARG, "triangle index out of range");
      if (seen[t]) return fail(c, RT_ERR_ARG, "duplicate triangle index");
      seen[t] = 1;
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = drain(c)) return rc;  // (the staging of the previous update is no longer read)
  rt_ctx::Geometry& g = c->geo;
  if (g.stage_tris < (size_t)count) {
    dfree(g.d_stage);
    g.stage_tris = 0;
    HIPCHK(c, hipMalloc(&g.d_stage, (size_t)count * 19 * sizeof(float)));
    g.stage_tris = (size_t)count;
  }
  const size_t n3f = 3 * (size_t)count;
  const float* src[6] = {p1, p2, p3, n1, n2, n3};
  for (int k = 0; k < 6; k++)
    HIPCHK(c, hipMemcpyAsync(g.d_stage + k * n3f, src[k], n3f * sizeof(float), hipMemcpyHostToDevice, c->stream));
  int* d_idx = reinterpret_cast<int*>(g.d_stage + 6 * n3f);
  if (tri_index) HIPCHK(c, hipMemcpyAsync(d_idx, tri_index, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return rt_update_geometry_device(c, tri_index ? d_idx : nullptr, first, count, g.d_stage, g.d_stage + n3f,
                                   g.d_stage + 2 * n3f, g.d_stage + 3 * n3f, g.d_stage + 4 * n3f, g.d_stage + 5 * n3f);
}

int rt_scene_download(rt_ctx* c, int32_t which, void* out, size_t bytes) {
  if (!c) return RT_ERR_ARG;
  if (which < 0 || which > RT_SCENE_QNODES || !out) return fail(c, RT_ERR_ARG, "unknown array or null output");
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "no scene");
  if (bytes != c->scene_bytes[which]) return fail(c, RT_ERR_ARG, "the array has another size");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = drain(c)) return rc;
  const void* src[6] = {c->d_tri, c->d_trx, c->d_trin, c->d_hrec, c->d_nodes, c->d_qnodes};
  HIPCHK(c, hipMemcpy(out, src[which], bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_scene_array_bytes(rt_ctx* c, int32_t which, size_t* bytes) {
  if (!c) return RT_ERR_ARG;
  if (which < 0 || which > RT_SCENE_QNODES || !bytes) return fail(c, RT_ERR_ARG, "unknown array or null output");
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "no scene");
  *bytes = c->scene_bytes[which];
  return RT_OK;
}

int rt_scene_bounds(rt_ctx* c, double out[5], int32_t* tri_flagged) {
  if (!c) return RT_ERR_ARG;
  if (!out) return fail(c, RT_ERR_ARG, "null output");
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "no scene");
  out[0] = c->cull_R; out[1] = c->cull_K; out[2] = c->cull_off; out[3] = c->tri_k1; out[4] = c->tri_k0;
  if (tri_flagged) *tri_flagged = c->tri_flagged;
  return RT_OK;
}

int rt_set_env(rt_ctx* c, const float* hdr, const float* cache, int32_t w, int32_t h, int32_t res) {
  if (!c || !hdr || !cache || w <= 0 || h <= 0) return RT_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = drain(c)) return rc;
  // {hdrMap.rgb, hdrCache.b} per texel (a direction's colour and pdf in one fetch) + hdrCache.rg
  std::vector<float4> a((size_t)w * h);
  std::vector<float2> b((size_t)w * h);
  for (size_t i = 0; i < a.size(); i++) {
    a[i] = make_float4(hdr[3 * i], hdr[3 * i + 1], hdr[3 * i + 2], cache[3 * i + 2]);
    b[i] = make_float2(cache[3 * i], cache[3 * i + 1]);
  }
  int rc;
  if ((rc = upload(c, (void**)&c->d_hdr, a.data(), a.size() * sizeof(float4)))) return rc;
  if ((rc = upload(c, (void**)&c->d_cache, b.data(), b.size() * sizeof(float2)))) return rc;
  for (auto& t : c->light) {  // (drained above: no call reads them)
    dfree(t.d);
    HIPCHK(c, hipMalloc(&t.d, a.size() * 2 * sizeof(float4)));
    t.valid = false;
  }
  c->hdr_w = w; c->hdr_h = h; c->hdr_res = res;
  c->env_set = true;
  return RT_OK;
}

// (Re)build everything that depends on the tiling: the tile tables, the accumulation buffer
// (zeroed), this rank's pixel list (its tiles in local order, 8x8 blocks inside a tile: ray
// coherence) and the wavefront state sized for it.
static int apply_tiling(rt_ctx* c, int width, int height, const rt_tiling& tl, std::vector<int32_t> owner) {
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = drain(c)) return rc;  // renders in flight read the buffers replaced below
  // the old pixel lists / accumulation no longer describe the frame from here on: a failure
  // below leaves the context un-sized (rt_render_async then refuses) rather than half-resized
  c->frame_set = false;
  if (c->dn.mem) (void)hipFree(c->dn.mem);  // the denoiser's frames and guides are the old size's
  c->dn = rt_ctx::Denoise{};
  if (c->tp.mem) (void)hipFree(c->tp.mem);  // and so is the display history
  c->tp = rt_ctx::Temporal{};
  motion_free_frames(c);  // and its triangle frames
  variance_free(c);       // and the variance mode's frames
  c->W = width; c->H = height;
  c->tile_w = tl.tile_w; c->tile_h = tl.tile_h; c->rank = tl.rank; c->world = tl.world;
  c->tiles_x = (width + tl.tile_w - 1) / tl.tile_w;
  c->tiles_y = (height + tl.tile_h - 1) / tl.tile_h;
  const int total = c->tiles_x * c->tiles_y;
  std::vector<int> count(tl.world, 0);
  std::vector<int2> src(total);
  c->my_tiles.clear();
  for (int t = 0; t < total; t++) {
    src[t] = make_int2(owner[t], count[owner[t]]++);
    if (owner[t] == tl.rank) c->my_tiles.push_back(t);
  }
  c->owner = std::move(owner);
  c->local_tiles = (int)c->my_tiles.size();
  c->max_local_tiles = *std::max_element(count.begin(), count.end());
  dfree(c->d_accum);
  size_t bytes = (size_t)std::max(1, c->max_local_tiles) * tl.tile_w * tl.tile_h * sizeof(float4);
  HIPCHK(c, hipMalloc(&c->d_accum, bytes));
  HIPCHK(c, hipMemset(c->d_accum, 0, bytes));
  dfree(c->d_tile_ids);
  dfree(c->d_tile_src);
  dfree(c->d_tile_cost);
  HIPCHK(c, hipMalloc(&c->d_tile_ids, std::max<size_t>(1, c->my_tiles.size()) * sizeof(int)));
  HIPCHK(c, hipMalloc(&c->d_tile_src, std::max<size_t>(1, src.size()) * sizeof(int2)));
  if (!c->my_tiles.empty())
    HIPCHK(c, hipMemcpy(c->d_tile_ids, c->my_tiles.data(), c->my_tiles.size() * sizeof(int), hipMemcpyHostToDevice));
  if (!src.empty()) HIPCHK(c, hipMemcpy(c->d_tile_src, src.data(), src.size() * sizeof(int2), hipMemcpyHostToDevice));
  std::vector<unsigned int> xy, acc;
  const int tpx = tl.tile_w * tl.tile_h;
  for (int lt = 0; lt < c->local_tiles; lt++) {
    const int gt = c->my_tiles[lt];
    const int tx = gt % c->tiles_x, ty = gt / c->tiles_x;
    for (int r = 0; r < tpx; r++) {
      const int blk = r >> 6, in = r & 63, bxs = tl.tile_w >> 3;
      const int lx = (blk % bxs) * 8 + (in & 7), ly = (blk / bxs) * 8 + (in >> 3);
      const int px = tx * tl.tile_w + lx, py = ty * tl.tile_h + ly;
      if (px >= width || py >= height) continue;
      xy.push_back((unsigned)px | ((unsigned)py << 16));
      acc.push_back((unsigned)(lt * tpx + ly * tl.tile_w + lx));
    }
  }
  c->n_valid = (int)xy.size();
  c->order_head = 0;
  dfree(c->d_pix);
  dfree(c->d_cam);
  const size_t nv = std::max<size_t>(1, xy.size());
  HIPCHK(c, hipMalloc(&c->d_pix, 2 * nv * sizeof(unsigned int)));
  HIPCHK(c, hipMalloc(&c->d_cam, dvl::camera_table(xy.size(), 1).total() * sizeof(float4)));
  c->cam_sets = 1;
  if (!xy.empty()) {
    HIPCHK(c, hipMemcpy(c->d_pix, xy.data(), xy.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_pix + nv, acc.data(), acc.size() * 4, hipMemcpyHostToDevice));
  }
  update_frames_cap(c, nv);
  int rc = alloc_wavefront(c, nv);
  if (rc) return rc;
  c->wf.pix_xy = c->d_pix;
  c->wf.pix_acc = c->d_pix + nv;
  c->wf.cam = c->d_cam;
  c->frame_set = true;
  c->loop_num = 0;
  return RT_OK;
}

int rt_resize(rt_ctx* c, int32_t width, int32_t height, const rt_tiling* t) {
  if (!c || width <= 0 || height <= 0) return RT_ERR_ARG;
  rt_tiling tl = t ? *t : rt_tiling{32, 32, 0, 1};
  if (tl.tile_w <= 0 || tl.tile_h <= 0 || (tl.tile_w % 8) || (tl.tile_h % 8) || tl.world <= 0 || tl.rank < 0 ||
      tl.rank >= tl.world)
    return fail(c, RT_ERR_ARG, "bad tiling (tile sizes must be positive multiples of 8, 0 <= rank < world)");
  if (width > 65535 || height > 65535) return fail(c, RT_ERR_LIMIT, "frame larger than 65535");
  const int total = ((width + tl.tile_w - 1) / tl.tile_w) * ((height + tl.tile_h - 1) / tl.tile_h);
  std::vector<int32_t> owner(total);
  for (int g = 0; g < total; g++) owner[g] = g % tl.world;  // interleaved default
  return apply_tiling(c, width, height, tl, std::move(owner));
}

int rt_set_tile_owners(rt_ctx* c, const int32_t* owner, int32_t n_tiles) {
  if (!c || !owner || n_tiles <= 0) return RT_ERR_ARG;
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "rt_resize first");
  if (n_tiles != c->tiles_x * c->tiles_y) return fail(c, RT_ERR_ARG, "n_tiles differs from the frame's tile count");
  for (int g = 0; g < n_tiles; g++)
    if (owner[g] < 0 || owner[g] >= c->world) return fail(c, RT_ERR_ARG, "tile owner outside [0, world)");
  const rt_tiling tl{c->tile_w, c->tile_h, c->rank, c->world};
  return apply_tiling(c, c->W, c->H, tl, std::vector<int32_t>(owner, owner + n_tiles));
}

int rt_get_tile_owners(const rt_ctx* c, int32_t* owner, int32_t n_tiles) {
  if (!c || !owner) return RT_ERR_ARG;
  if (!c->frame_set) return RT_ERR_STATE;
  if (n_tiles != (int32_t)c->owner.size()) return RT_ERR_ARG;
  memcpy(owner, c->owner.data(), c->owner.size() * sizeof(int32_t));
  return RT_OK;
}

int rt_reset(rt_ctx* c) {
  if (!c) return RT_ERR_ARG;
  c->loop_num = 0;
  return RT_OK;
}
int rt_set_loop_num(rt_ctx* c, int32_t n) {
  if (!c || n < 0) return RT_ERR_ARG;
  c->loop_num = n;
  return RT_OK;
}
int rt_set_max_paths(rt_ctx* c, uint64_t slots) {
  if (!c) return RT_ERR_ARG;
  c->max_slots_req = (size_t)slots;
  if (c->frame_set) update_frames_cap(c, (size_t)c->n_valid);
  return RT_OK;
}

int rt_get_loop_num(const rt_ctx* c, int32_t* n) {
  if (!c || !n) return RT_ERR_ARG;
  *n = c->loop_num;
  return RT_OK;
}
int rt_set_finish(rt_ctx* c, int32_t pass, uint64_t max_slots) {
  if (!c || pass < 0) return RT_ERR_ARG;
  c->finish_pass = pass;
  c->finish_slots = max_slots;
  return RT_OK;
}

int rt_set_pipeline(rt_ctx* c, int32_t depth) {
  if (!c || depth < 1) return RT_ERR_ARG;
  int rc = rt_synchronize(c);  // calls in flight keep the sets they were given
  if (rc) return rc;
  c->pipe_depth = std::min<int>(depth, 2);  // streams aux[1], aux[2]
  c->pipe_next = 0;
  return RT_OK;
}

int rt_clear_accum(rt_ctx* c) {
  if (!c) return RT_ERR_ARG;
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "rt_resize first");
  HIPCHK(c, hipSetDevice(c->device));
  size_t bytes = (size_t)std::max(1, c->max_local_tiles) * c->tile_w * c->tile_h * sizeof(float4);
  HIPCHK(c, hipMemsetAsync(c->d_accum, 0, bytes, c->stream));
  return RT_OK;
}

}  // extern "C"

// The steps of rt_render_async, in the order they run.
namespace {

#ifdef RT_DEV
#include "rt_dev_report.h"
#endif

// What one rt_render_async call decided, on its stack, handed from step to step.
struct RenderCall {
  struct Frame { int loop_num, ro_bits; };
  std::vector<Frame> frames;       // the traced frames' (loopNum, randOrigin bits), in call order
  int n_traced = 0;                // frames.size()
  int loop_end = 0;                // rt_ctx::loop_num after the call
  rpl::Switches sw;                // the planner's switches for this call (plan_switches)
  int pipe_sets = 0;
  bool pipe = false, serial = false;
  int pset = 0;                    // pipelined: path-state set, camera table, overflow column, stream aux[1 + pset]
  hipStream_t ps = nullptr;        // the stream that runs this call
  hipEvent_t e_entry = nullptr;    // pipelined: the caller's stream at entry (the blend waits for it)
  rt_ctx::LightTable* LT = nullptr;
  const int* d_loop = nullptr;     // the frame table on the device (stage_frame_table)
  const float* d_ro = nullptr;
  float2* d_sobol = nullptr;
  float2* d_blendw = nullptr;
};

// main.cpp:175: LoopNum++ while below maxIterations; frames at the cap copy history (R12).  Listed
// before anything can fail; stage_frame_table moves rt_ctx::loop_num, so a call that fails before
// it leaves loop_num untouched.
void list_traced_frames(const rt_ctx* c, const rt_frame_params* fp, const float* rand_origin, int n_frames, RenderCall& call) {
  int ln = c->loop_num;
  for (int k = 0; k < n_frames; k++) {
    if (fp->max_iterations == -1 || ln < fp->max_iterations) ln++;
    if (!(fp->max_iterations == -1 || ln < fp->max_iterations)) continue;
    RenderCall::Frame f{ln, 0};
    memcpy(&f.ro_bits, &rand_origin[k], 4);
    call.frames.push_back(f);
  }
  call.n_traced = (int)call.frames.size();
  call.loop_end = ln;
}

// The planner's inputs (render_plan.h): the context as it stands (reserve_path_state moves
// frames_cap and the path state's sizes, so batches copy it again) ...
rpl::Facts plan_facts(const rt_ctx* c) {
  auto i64 = [](uint64_t v) { return (int64_t)std::min<uint64_t>(v, (uint64_t)INT64_MAX); };
  return rpl::Facts{c->n_groups, c->n_valid, c->frames_cap, i64(c->wf_paths), c->finish_pass, c->pipe_finish_pass,
                    i64(c->finish_slots), c->split_kinds, c->split_passes, c->wide, c->mats_emissive, c->tile_cost_on,
                    i64(c->wf_hit_cap), i64(c->wf_rows), i64(c->order_head), c->pipe_depth, i64(c->pipe_nomem_slots),
                    c->n_cus, c->trace_bpc0, c->trace_bpc, c->finish_bpc, c->pipe_finish_bpc, rtd::SH_SUB, rtd::SH_SUB_CAM,
                    rtd::SH_SUB_BULK, (int64_t)rtd::kP1SampleEvery};
}
// ... and the switches: the release defaults, in the development library with the A/B settings of
// this call's environment (the tests flip them between calls)
rpl::Switches plan_switches(const rt_ctx* c) {
  rpl::Switches S;
#ifdef RT_DEV
  auto off = [](const char* name, int64_t& v) {  // (A/B: these only switch off)
    if (const char* e = knob(name)) v = v && atoi(e) != 0;
  };
  off("RT_PIX_SPLIT", S.pix_split);
  off("RT_CAM_SHARED", S.cam_shared);
  off("RT_CAM_MISS_ONCE", S.cam_miss_once);
  off("RT_P1_LEAN", S.p1_lean);
  off("RT_ROW_COMPACT", S.row_compact);
  if (const char* e = knob("RT_CAM_SHARED_STATIC")) S.cam_shared_static = atoi(e) != 0;
  if (const char* e = knob("RT_GROUP_SPLIT"))  // group 0's share of the work items, in whole blocks
    S.group_head = (int64_t)std::min((size_t)c->n_valid, ((size_t)((double)c->n_valid * atof(e)) + 63) / 64 * 64);
  for (int g = 0; g < rpl::kMaxGroups; g++) {
    char kn[32];
    snprintf(kn, sizeof(kn), "RT_FINISH_PASS_G%d", g);
    if (const char* e = knob(kn)) S.finish_pass_g[g] = std::max(0, atoi(e));
  }
  if (const char* e = knob("RT_ROW_CAP")) S.row_cap = (int64_t)std::min<uint64_t>(strtoull(e, nullptr, 10), (uint64_t)INT64_MAX);  // (tests: rows)
#else
  (void)c;
#endif
  return S;
}
rpl::Call plan_call(const rt_frame_params* fp, const RenderCall& call, int n_left) {
  return rpl::Call{fp->flags, fp->enable_bsdf, fp->max_bounce, n_left, 0, call.pipe, call.pset};
}

// a pipelined call (rt_set_pipeline): see rt_ctx::pipe_depth and rpl::admit_pipe; here only the
// look at the streams it asks for
void admit_pipeline(rt_ctx* c, const rt_frame_params* fp, RenderCall& call) {
  const rpl::Facts F = plan_facts(c);
  rpl::Call C = plan_call(fp, call, call.n_traced);
  call.sw = plan_switches(c);
  call.pipe_sets = rpl::pipe_sets(F);
  call.serial = rpl::serial(C);
  if (rpl::idle_matters(F, call.sw, C)) {
    bool idle = !(c->batch_done && hipEventQuery(c->batch_done) != hipSuccess);
    for (int q = 0; q < call.pipe_sets && idle; q++)
      if (c->set_free[q] && hipEventQuery(c->set_free[q]) != hipSuccess) idle = false;
    (void)hipGetLastError();  // (hipErrorNotReady is a status, not an error)
    C.idle = idle;
  }
  call.pipe = rpl::admit_pipe(F, call.sw, C);
}

// Path state for the call's batches (it only grows) and the frame groups' streams
int reserve_path_state(rt_ctx* c, int n_frames, RenderCall& call) {
  const int n = call.n_traced;
  const size_t nv = std::max<size_t>(1, (size_t)c->n_valid);
  int rc = RT_ERR_NOMEM;
  if (call.pipe && n >= c->n_groups) {  // a pipelined batch: the whole call in one set
    rc = alloc_wavefront(c, (size_t)n * nv);
    if (rc == RT_ERR_NOMEM) {  // not both sets: this size runs as frame groups from now on
      c->pipe_nomem_slots = std::min(c->pipe_nomem_slots, (size_t)n * nv);
      call.pipe = false;
    } else if (rc) {
      return rc;
    }
  }
  while (rc == RT_ERR_NOMEM) {  // a budget larger than free HBM runs fewer frames at a time
    const int per_group = (std::min(c->frames_cap, n_frames) + c->n_groups - 1) / c->n_groups;
    rc = alloc_wavefront(c, (size_t)per_group * nv);
    if (rc != RT_ERR_NOMEM || per_group <= 1) break;
    c->frames_cap = std::max(1, std::min(c->frames_cap, n_frames) / 2);
  }
  if (rc) return rc;
  for (int g = 1; g < c->n_groups; g++)
    if (!c->aux[g]) HIPCHK(c, hipStreamCreateWithFlags(&c->aux[g], hipStreamNonBlocking));
  return RT_OK;
}

// The stream that runs this call: pipelined sets on aux[1], aux[2] (aux[1] is also the second
// frame group's stream: a pipelined call waits for unpipelined ones anyway, and a fourth stream
// measured as losing the overlap, GPU_MAX_HW_QUEUES being 4); every other call on the caller's
int enter_pipelined_set(rt_ctx* c, RenderCall& call) {
  call.pset = call.pipe ? c->pipe_next : 0;
  call.ps = call.pipe ? c->aux[1 + call.pset] : c->stream;
  if (!call.pipe) return RT_OK;
  const int pset = call.pset, pipe_sets = call.pipe_sets;
  c->pipe_next = (c->pipe_next + 1) % pipe_sets;
  if (!call.ps) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->aux[1 + pset], hipStreamNonBlocking));
    call.ps = c->aux[1 + pset];
  }
  if (c->cam_sets < pipe_sets) {  // one camera table per set (a call may move the camera)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(c->d_cam);
    HIPCHK(c, hipMalloc(&c->d_cam, dvl::camera_table((size_t)c->n_valid, (size_t)pipe_sets).total() * sizeof(float4)));
    c->cam_sets = pipe_sets;
    c->wf.cam = c->d_cam;
  }
  TAKE_EVENT(c, call.e_entry);
  HIPCHK(c, hipEventRecord(call.e_entry, c->stream));
  // the set's previous call and the last batched call have finished with its state
  if (c->set_free[pset]) HIPCHK(c, hipStreamWaitEvent(call.ps, c->set_free[pset], 0));
  if (c->batch_done) HIPCHK(c, hipStreamWaitEvent(call.ps, c->batch_done, 0));
  return RT_OK;
}

// The traced frames' (loopNum, randOrigin) go to a device table in one upload; wf_sobol adds
// their Sobol pairs and blend weights.  rt_ctx::loop_num moves here.
int stage_frame_table(rt_ctx* c, const rt_frame_params* fp, int n_frames, RenderCall& call) {
  const int n_traced = call.n_traced;
  const bool wavefront = !(fp->flags & RT_FLAG_MEGAKERNEL);
  rt_ctx::FrameTable& T = c->ft[call.pipe ? 1 + call.pset : 0];
  if (n_frames > 0 && (size_t)n_frames > T.cap) {
    if (T.ev) HIPCHK(c, hipEventSynchronize(T.ev));
    if (T.h) (void)hipHostFree(T.h);
    T.h = nullptr;
    if (T.d) HIPCHK(c, hipStreamSynchronize(c->stream));  // calls in flight read the old table
    dfree(T.d);
    const size_t cap = std::max<size_t>(call.pipe ? 16 : 1024, (size_t)n_frames);
    HIPCHK(c, hipHostMalloc((void**)&T.h, dvl::frame_table(cap).host_total * sizeof(int)));
    HIPCHK(c, hipMalloc((void**)&T.d, dvl::frame_table(cap).total * sizeof(int)));
    T.cap = cap;
  }
  const dvl::FrameTable F = dvl::frame_table(T.cap);  // (the host copy: its first two sub-tables)
  int* const h_ro = T.h + F.rand_origin.off;
  int* const d_ro = T.d + F.rand_origin.off;
  if (!T.ev) HIPCHK(c, hipEventCreateWithFlags(&T.ev, hipEventDisableTiming));
  HIPCHK(c, hipEventSynchronize(T.ev));  // the previous upload from this table has read T.h
  c->loop_num = call.loop_end;
  for (int k = 0; k < n_traced; k++) {
    T.h[k] = call.frames[k].loop_num;
    h_ro[k] = call.frames[k].ro_bits;
  }
  // small calls hand the pairs to wf_sobol as kernel arguments, which writes the table
  rtd::InlineFrames IF;
  memset(&IF, 0, sizeof(IF));
  if (n_traced > 0 && n_traced <= RT_INLINE_FRAMES && wavefront) {
    IF.n_inline = n_traced;
    for (int k = 0; k < n_traced; k++) {
      IF.loop[k] = T.h[k];
      memcpy(&IF.ro[k], &h_ro[k], 4);
    }
  } else if (n_traced > 0) {
    HIPCHK(c, hipMemcpyAsync(T.d, T.h, (size_t)n_traced * sizeof(int), hipMemcpyHostToDevice, call.ps));
    HIPCHK(c, hipMemcpyAsync(d_ro, h_ro, (size_t)n_traced * sizeof(int), hipMemcpyHostToDevice, call.ps));
  }
  HIPCHK(c, hipEventRecord(T.ev, call.ps));
  call.d_loop = T.d;
  call.d_ro = reinterpret_cast<const float*>(d_ro);
  call.d_sobol = reinterpret_cast<float2*>(T.d + F.sobol.off);
  call.d_blendw = reinterpret_cast<float2*>(T.d + F.blend_w.off);
  if (n_traced > 0 && wavefront) {
    hipLaunchKernelGGL(rtd::wf_sobol, dim3((4 * n_traced + 255) / 256), dim3(256), 0, call.ps, T.d,
                       reinterpret_cast<float*>(d_ro), call.d_sobol, call.d_blendw, n_traced, IF);
    HIPCHK(c, hipGetLastError());
  }
  return RT_OK;
}

// NEE light table for this call's envAngle (SampleHdrLight): the table built for this angle, or
// the other one rebuilt on this call's stream once the last call that read it has finished (a
// device-side wait: an interactive envAngle drag keeps its frames in flight)
int bind_light_table(rt_ctx* c, const rt_frame_params* fp, RenderCall& call) {
  rt_ctx::LightTable*& LT = call.LT;
  LT = &c->light[c->light_cur];
  if (call.n_traced <= 0 || (fp->flags & RT_FLAG_MEGAKERNEL)) return RT_OK;
  auto same = [&](const rt_ctx::LightTable& t) {
    return t.valid && __builtin_memcmp(&t.angle, &fp->env_angle, sizeof(float)) == 0;
  };
  if (!same(*LT)) {
    const int other = c->light_cur ^ 1;
    LT = &c->light[other];
    c->light_cur = other;
    if (!same(*LT)) {
      if (LT->last_use) HIPCHK(c, hipStreamWaitEvent(call.ps, LT->last_use, 0));
      const rtd::Env E{c->d_hdr, c->d_cache, LT->d, c->hdr_w, c->hdr_h, c->hdr_res, fp->env_angle, fp->env_intensity};
      const unsigned int n = (unsigned int)(c->hdr_w * c->hdr_h);
      hipLaunchKernelGGL(rtd::rt_light_table_kernel, dim3(std::max(1u, std::min(4096u, (n + 255) / 256))), dim3(256),
                         0, call.ps, E, LT->d);
      HIPCHK(c, hipGetLastError());
      if (!LT->built) HIPCHK(c, hipEventCreateWithFlags(&LT->built, hipEventDisableTiming));
      HIPCHK(c, hipEventRecord(LT->built, call.ps));
      LT->angle = fp->env_angle;
      LT->valid = true;
    }
  }
  // every call that reads the table waits for its build, which may still run on another call's
  // stream (a pipelined call on aux[1] rebuilt it; this one runs on aux[2] with the same angle)
  if (LT->built) HIPCHK(c, hipStreamWaitEvent(call.ps, LT->built, 0));
  return RT_OK;
}

// The scene's part of the kernel parameters: traversal structure, triangles, materials and the
// culling bound for ray origins within origin_R of the axes (render calls: the camera position;
// queries: the caller's rays)
void fill_scene_kparams(const rt_ctx* c, double origin_R, KParams& P) {
  P.nodes = c->d_nodes; P.root = c->root; P.has_scene = c->has_scene; P.stack_entries = c->stack_entries;
  P.stack_cap = std::max(c->stack_entries, c->qstack_entries);
  P.qnodes = c->d_qnodes; P.qroot = c->qroot; P.n_qnodes = c->n_qnodes; P.n_tri = c->n_tri;
  {  // eps of the culling bound for these origins and the scene's points
    const double R = std::max(c->cull_R, origin_R);
    // x (1 + 2^-9): the fp32 rounding of eps * max|1/d| and of the sum in cull_limit
    const double eps = 2.0 * (c->cull_K * 0x1p-24 * R * (1.0 + 0x1p-10) + c->cull_off) * (1.0 + 0x1p-9);
    // RT_CULL_EPS_SCALE (tests only, read on every call): 0 restores the round-1 heuristic margin,
    // whose hole tests/test_gpu_cull.py demonstrates
    const char* es = knob("RT_CULL_EPS_SCALE");
    const double sc = es ? atof(es) : 1.0;
    P.cull_eps = (eps * sc < 1e30) ? (float)(eps * sc) : INFINITY;
  }
  P.tri = c->d_tri; P.trin = c->d_trin; P.hrec = c->d_hrec; P.mats = c->d_mats;
  {  // edge-filter margin, rounded up (x (1 + 2^-20)); RT_TRI_MARGIN_SCALE (tests only, read on
     // every call): 0 makes the filter decide every point, the negative control of
     // tests/test_gpu_tri_filter.py
    const char* ms = knob("RT_TRI_MARGIN_SCALE");
    const double sc = ms ? atof(ms) : 1.0;
    P.trx = c->d_trx;
    P.tri_k1 = (float)(c->tri_k1 * sc * (1.0 + 0x1p-20));
    P.tri_k0 = (float)(c->tri_k0 * sc * (1.0 + 0x1p-20));
  }
}

// The kernel parameters every batch of the call shares; the batch loop sets loop_num,
// rand_origin, sobol, blend_w and n_frames
void fill_kparams(const rt_ctx* c, const rt_frame_params* fp, const RenderCall& call, KParams& P) {
  memset(&P, 0, sizeof(P));
  memcpy(P.pos, fp->position, 12); memcpy(P.lbc, fp->left_bottom_corner, 12);
  memcpy(P.right, fp->right, 12); memcpy(P.up, fp->up, 12);
  P.half_w = fp->half_w; P.half_h = fp->half_h;
  P.enable_mis = fp->enable_mis; P.enable_env = fp->enable_env_map; P.enable_bsdf = fp->enable_bsdf;
  P.env_intensity = fp->env_intensity; P.env_angle = fp->env_angle;
  P.max_bounce = fp->max_bounce; P.flags = fp->flags;
  P.W = c->W; P.H = c->H; P.tile_w = c->tile_w; P.tile_h = c->tile_h; P.tiles_x = c->tiles_x;
  P.rank = c->rank; P.world = c->world; P.tile_ids = c->d_tile_ids;
  P.tile_cost = c->tile_cost_on ? c->d_tile_cost : nullptr;
  P.cost_blocks = c->cost_blocks ? 1 : 0;
  P.n_work = (unsigned)c->local_tiles * (unsigned)(c->tile_w * c->tile_h);
  double origin_R = 0.0;  // the call's ray origins: the camera position, scene points
  for (int a = 0; a < 3; a++) origin_R = std::max(origin_R, std::fabs((double)fp->position[a]));
  fill_scene_kparams(c, origin_R, P);
  P.hdr = c->d_hdr; P.cache = c->d_cache; P.light = call.LT->d;
  P.hdr_w = c->hdr_w; P.hdr_h = c->hdr_h; P.hdr_res = c->hdr_res;
  P.accum = c->d_accum; P.counter = c->d_counter; P.stats = c->d_stats;
}

// RT_FLAG_MEGAKERNEL: the batch in one persistent rt_path_kernel launch on the caller's stream
int megakernel_batch(rt_ctx* c, const rt_frame_params* fp, const KParams& P) {
  HIPCHK(c, hipMemsetAsync(c->d_counter, 0, 4, c->stream));
  unsigned int max_blocks = (P.n_work + 255) / 256;
  unsigned int grid = std::min<unsigned int>((unsigned)(c->n_cus * c->blocks_per_cu), max_blocks);
  if (fp->flags & RT_FLAG_COUNT_VISITS)
    hipLaunchKernelGGL(rtd::rt_path_kernel<true>, dim3(grid), dim3(256), c->block_lds, c->stream, P);
  else
    hipLaunchKernelGGL(rtd::rt_path_kernel<false>, dim3(grid), dim3(256), c->block_lds, c->stream, P);
  HIPCHK(c, hipGetLastError());
  c->trace_launches++;
  return RT_OK;
}

// One wavefront batch: what the planner decided from `in` (B: the groups, each with its own path
// state and stream) and the kernel parameters and streams that go with it (plan_groups)
struct GroupPlan {
  rpl::In in;
  rpl::Batch B;
  rtd::WFParams WG[rt_ctx::MAX_GROUPS];
  hipStream_t sg[rt_ctx::MAX_GROUPS];
  float4* cam = nullptr;           // this call's camera table (wf_camera writes it, every group reads it)
  hipEvent_t prev_blend = nullptr; // after the previous frame group's blend (blend_and_join)
};
static_assert(rpl::kMaxGroups == rt_ctx::MAX_GROUPS, "the planner's groups are rt_ctx's");

// The batch's groups as rpl::plan_batch cuts them (P: the batch's frames), the pointers of their
// kernel parameters, and the overflow column's layout check
int plan_groups(rt_ctx* c, const RenderCall& call, const KParams& P, GroupPlan& plan) {
  const rpl::Batch& B = plan.B = rpl::plan_batch(plan.in.f, plan.in.s, plan.in.c);
  const unsigned int trace_grid = (unsigned)(c->n_cus * std::max(c->trace_bpc, c->trace_bpc0));
  unsigned long long* d_wave_log = nullptr;  // COUNT builds (RT_DEBUG_PASSES)
#ifdef RT_DEV
  if (int rc = dev_wave_log(c, d_wave_log)) return rc;
#endif
  const size_t ovf_group = c->stack_ovf_bytes / sizeof(int2) / (size_t)c->n_groups;
  // the call's camera directions and camera hit points (WFState::org): one table of each per set
  const dvl::CameraTable CT = dvl::camera_table((size_t)c->n_valid, (size_t)c->cam_sets);
  const size_t cam_set = call.pipe ? (size_t)call.pset : 0;
  plan.cam = c->wf.cam + CT.dir(cam_set).off;
  float4* const org = c->wf.cam + CT.org(cam_set).off;
  for (int g = 0; g < B.G; g++) {
    const rpl::Group& G = B.g[g];
    rtd::WFParams& WP = plan.WG[g];
    WP.K = P;
    WP.K.loop_num = P.loop_num + G.f0;
    WP.K.rand_origin = P.rand_origin + G.f0;
    WP.K.sobol = P.sobol + 4 * G.f0;
    WP.K.blend_w = P.blend_w + G.f0;
    WP.K.n_frames = G.f1 - G.f0;
    WP.K.n_work = G.w1 - G.w0;
    WP.K.lds_entries = c->trace_lds_entries;
    WP.K.pool_chunk = c->pool_chunk;
    WP.K.stack_ovf = c->d_stack_ovf ? c->d_stack_ovf + (size_t)G.set * ovf_group : nullptr;
    WP.K.ovf_lanes = trace_grid * 256u;
    {
      const std::string e = ovf_layout_error(c, G.set, trace_grid);
      if (!e.empty()) return fail(c, RT_ERR_STATE, e);
    }
    WP.K.wave_log = d_wave_log;
#ifdef RT_DEV
    // RT_DEBUG_WAVES_ONLY: the per-wave timeline without the per-ray step histogram (whose atomics
    // on a few lines would set the pass times)
    if (d_wave_log && knob("RT_DEBUG_WAVES_ONLY")) WP.K.flags |= rtd::kFlagNoRayHist;
#endif
    WP.S = c->wfg[G.set];
    WP.S.pix_xy = c->wf.pix_xy + G.w0;
    WP.S.pix_acc = c->wf.pix_acc + G.w0;
    WP.S.cam = plan.cam + G.w0;
    WP.S.org = org + G.w0;
    WP.A = c->wfa[G.set];  // (the arena's own arrays; the per-call tables as S)
    WP.A.pix_xy = WP.S.pix_xy;
    WP.A.pix_acc = WP.S.pix_acc;
    WP.A.cam = WP.S.cam;
    WP.A.org = WP.S.org;
    // the group's flags: those that wf_cam_classify and the kernels after it read enter after
    // pass 0's trace (run_group_passes)
    WP.n_frames = G.f1 - G.f0;
    WP.pass = 0;
    WP.cam_n = 0u;
    WP.cam_shared = 0;
    WP.cam_miss_once = 0;
    WP.p1_lean = 0;
    WP.row_compact = 0;
    WP.row_cap = 0u;
    WP.fuse_blend = G.fuse_blend ? 1 : 0;
    WP.p1_compact = G.p1_compact ? 1 : 0;
    plan.sg[g] = G.stream == 0 ? c->stream : c->aux[G.stream];
  }
  return RT_OK;
}

// Camera directions of this call's pixels (every group reads them; wf_camera also zeroes the
// groups' pass counters), then the aux streams start after everything already queued on the
// caller's stream
int launch_camera_and_fork(rt_ctx* c, const RenderCall& call, GroupPlan& plan) {
  rtd::WFParams WC = plan.WG[0];
  WC.K.n_work = (unsigned)c->n_valid;
  WC.S.pix_xy = c->wf.pix_xy;
  WC.S.pix_acc = c->wf.pix_acc;
  WC.S.cam = plan.cam;
  rtd::GroupCounters Z;
  memset(&Z, 0, sizeof(Z));
  Z.n = plan.B.G;
  for (int g = 0; g < plan.B.G; g++) Z.cnt[g] = plan.WG[g].S.cnt;
  hipLaunchKernelGGL(rtd::wf_camera, dim3(std::max(1u, std::min<unsigned int>(2048u, ((unsigned)c->n_valid + 255) / 256))),
                     dim3(256), 0, call.ps, WC, Z);
  HIPCHK(c, hipGetLastError());
  if (plan.B.G > 1) {
    hipEvent_t es;
    TAKE_EVENT(c, es);
    HIPCHK(c, hipEventRecord(es, c->stream));
    for (int g = 1; g < plan.B.G; g++) HIPCHK(c, hipStreamWaitEvent(plan.sg[g], es, 0));
    c->event_pool.push_back(es);  // reusable once the waits are enqueued
  }
  return RT_OK;
}

// Group g's wavefront passes on its stream, as rpl::step lists them: trace(s) + shade per pass, or
// the finisher as the last step
int run_group_passes(rt_ctx* c, GroupPlan& plan, int g) {
  const rpl::In& in = plan.in;
  const rpl::Group& G = plan.B.g[g];
  rtd::WFParams& WP = plan.WG[g];  // (its pass counters were zeroed by wf_camera)
  const hipStream_t st = plan.sg[g];
  const bool bsdf = in.c.enable_bsdf != 0;
#ifdef RT_DEV
  if (dev_passes()) dev_plan_report(plan.in, plan.B, g);
#endif
  for (int pass = 0; pass < G.n_steps; pass++) {
    const rpl::Step s = rpl::step(in.f, in.s, in.c, G, pass);
    WP.pass = pass;
    WP.split = s.split ? 1 : 0;
    WP.split_out = s.split_out ? 1 : 0;
    if (s.finisher) {
#ifdef RT_DEV
      if (dev_passes()) return dev_finish_report(c, bsdf, dim3(s.fgrid), st, WP, g, pass);
#endif
      launch_finish(c, bsdf, dim3(s.fgrid), st, WP);
      HIPCHK(c, hipGetLastError());
      break;
    }
    WP.cam_n = s.cam_n;
    WP.cam_shared = s.cam_shared ? 1 : 0;
    hipEvent_t t0, t1;
    TAKE_EVENT(c, t0);
    TAKE_EVENT(c, t1);
    HIPCHK(c, hipEventRecord(t0, st));
    for (int k = 0; k < s.n_trace; k++) launch_trace(c, s.trace[k], dim3(s.trace_grid), WP, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(t1, st));
    c->trace_events.push_back({t0, t1, c->launches});
    c->trace_launches++;
#ifdef RT_DEV
    if (dev_passes()) if (int rc = dev_pass_report(c, st, WP, g, pass, t0, t1)) return rc;
#endif
    if (pass == 0) {  // from here to the group's wf_blend
      WP.cam_miss_once = G.cam_miss_once ? 1 : 0;
      WP.p1_lean = G.p1_lean ? 1 : 0;
      WP.row_compact = G.row_compact ? 1 : 0;
      WP.row_cap = G.row_cap;
    }
    if (s.classify) {  // (neither a trace nor a render launch in rt_stats)
      hipLaunchKernelGGL(rtd::wf_cam_classify, dim3(s.classify_grid), dim3(256), 0, st, WP);
      HIPCHK(c, hipGetLastError());
    }
    if (s.p1_count) {
      hipLaunchKernelGGL(rtd::wf_p1_count<true>, dim3(s.p1_grid[0]), dim3(256), 0, st, WP);
      hipLaunchKernelGGL(rtd::wf_p1_count<false>, dim3(s.p1_grid[1]), dim3(256), 0, st, WP);
      HIPCHK(c, hipGetLastError());
    }
    launch_shade(s.shade, bsdf, dim3(s.shade_grid), st, WP);
    HIPCHK(c, hipGetLastError());
#ifdef RT_DEV
    if (dev_passes() && pass == 1) if (int rc = dev_rows_report(c, st, WP)) return rc;
#endif
  }
  return RT_OK;
}

// Group g's blend into the accumulation and, after the last group's, the caller's stream joins
// the groups
int blend_and_join(rt_ctx* c, RenderCall& call, GroupPlan& plan, int g) {
  const hipStream_t st = plan.sg[g];
  const int G = plan.B.G;
  // progressive blend in frame order: group g after group g-1 (pixel groups blend
  // disjoint pixels: no order between them)
  if (plan.prev_blend) {
    HIPCHK(c, hipStreamWaitEvent(st, plan.prev_blend, 0));
    c->event_pool.push_back(plan.prev_blend);
    plan.prev_blend = nullptr;
  }
  if (call.e_entry) {  // pipelined: after the caller's work on the accumulation and the previous call
    HIPCHK(c, hipStreamWaitEvent(st, call.e_entry, 0));
    c->event_pool.push_back(call.e_entry);  // reusable once the wait is enqueued
    call.e_entry = nullptr;
  }
  if (plan.B.g[g].blend) {
    hipLaunchKernelGGL(rtd::wf_blend, dim3(std::max(1u, std::min<unsigned int>(2048u, ((unsigned)c->n_valid + 255) / 256))),
                       dim3(256), 0, st, plan.WG[g]);
    HIPCHK(c, hipGetLastError());
  }
  if (!plan.B.pix_split && g + 1 < G) {
    TAKE_EVENT(c, plan.prev_blend);
    HIPCHK(c, hipEventRecord(plan.prev_blend, st));
  }
  if (g + 1 < G) return RT_OK;
  // the caller's stream joins the last group (frame groups finish in order through their
  // blends) or every group (pixel groups)
  for (int j = plan.B.pix_split ? 1 : G - 1; j < G && G > 1; j++) {
    hipEvent_t ej;
    TAKE_EVENT(c, ej);
    HIPCHK(c, hipEventRecord(ej, plan.sg[j]));
    HIPCHK(c, hipStreamWaitEvent(c->stream, ej, 0));
    c->event_pool.push_back(ej);
  }
  return RT_OK;
}

// The batch's end on the call's stream: its timing pair, what later calls wait for, and the
// folds that bound the pending events
int close_batch(rt_ctx* c, const RenderCall& call, hipEvent_t e0, hipEvent_t e1) {
  const int pset = call.pset;
  HIPCHK(c, hipEventRecord(e1, call.ps));
  if (call.pipe) {  // the caller's stream joins the call; the set is free again after it
    if (c->set_free[pset]) c->event_pool.push_back(c->set_free[pset]);
    TAKE_EVENT(c, c->set_free[pset]);
    HIPCHK(c, hipEventRecord(c->set_free[pset], call.ps));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->set_free[pset], 0));
  } else if (call.pipe_sets >= 2) {  // pipelined calls that follow start after this batch
    if (!c->batch_done) HIPCHK(c, hipEventCreateWithFlags(&c->batch_done, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->batch_done, c->stream));
  }
  if (!call.LT->last_use) HIPCHK(c, hipEventCreateWithFlags(&call.LT->last_use, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(call.LT->last_use, c->stream));
  c->events.push_back({e0, e1});
  c->launches++;
  if (int rc = fold_trace_events(c, kMaxPendingEvents)) return rc;
  return fold_events(c, c->events, c->kernel_ms, kMaxPendingEvents);
}

}  // namespace

extern "C" {

int rt_render_async(rt_ctx* c, const rt_frame_params* fp, const float* rand_origin, int32_t n_frames) {
  if (!c || !fp || n_frames < 0 || (n_frames && !rand_origin)) return RT_ERR_ARG;
  if (!c->scene_set || !c->env_set || !c->frame_set) return fail(c, RT_ERR_STATE, "set_scene, set_env and resize first");
  const bool mega = (fp->flags & RT_FLAG_MEGAKERNEL) != 0;
  if (mega && !fp->enable_bsdf)
    return fail(c, RT_ERR_ARG, "BRDF mode (enable_bsdf = 0) runs on the wavefront path only");
  HIPCHK(c, hipSetDevice(c->device));
  RenderCall call;
  list_traced_frames(c, fp, rand_origin, n_frames, call);
  admit_pipeline(c, fp, call);
  if (!mega && n_frames > 0)
    if (int rc = reserve_path_state(c, n_frames, call)) return rc;
  if (int rc = enter_pipelined_set(c, call)) return rc;
  if (int rc = stage_frame_table(c, fp, n_frames, call)) return rc;
  if (int rc = bind_light_table(c, fp, call)) return rc;
  KParams P;
  fill_kparams(c, fp, call, P);
  for (int done = 0, nf = 0; done < call.n_traced; done += nf) {
    GroupPlan plan;
    plan.in = rpl::In{plan_facts(c), plan_call(fp, call, call.n_traced - done), call.sw};
    nf = std::min(rpl::batch_cap(plan.in.f, plan.in.c), call.n_traced - done);
    P.loop_num = call.d_loop + done;
    P.rand_origin = call.d_ro + done;
    P.sobol = call.d_sobol + 4 * (size_t)done;
    P.blend_w = call.d_blendw + done;
    P.n_frames = nf;
    if (P.n_work == 0) continue;  // an empty share: nothing to launch, nothing timed
    hipEvent_t e0, e1;
    TAKE_EVENT(c, e0);
    TAKE_EVENT(c, e1);
    HIPCHK(c, hipEventRecord(e0, call.ps));
    if (mega) {
      if (int rc = megakernel_batch(c, fp, P)) return rc;
    } else {
      if (int rc = plan_groups(c, call, P, plan)) return rc;
      if (int rc = launch_camera_and_fork(c, call, plan)) return rc;
      for (int g = 0; g < plan.B.G; g++) {
        if (int rc = run_group_passes(c, plan, g)) return rc;
        if (int rc = blend_and_join(c, call, plan, g)) return rc;
      }
    }
    if (int rc = close_batch(c, call, e0, e1)) return rc;
  }
  return RT_OK;
}

int rt_synchronize(rt_ctx* c) {
  if (!c) return RT_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // (the stream joins every group and pipelined set of each call, so all pairs have finished)
  for (auto& e : c->events) {
    const int rc = fold_pair(c, e, c->kernel_ms);
    if (rc) return rc;
  }
  c->events.clear();
  for (auto& e : c->trace_events) {
    const int rc = fold_trace(c, e);
    if (rc) return rc;
  }
  c->trace_events.clear();
  return RT_OK;
}

int rt_abi_version(void) { return RT_ABI_VERSION; }
int rt_gather_last_transport(const rt_ctx* c) { return c ? c->gather_transport : RT_ERR_ARG; }

// rt_stats_get and rt_render write the ABI-3 struct (through p1_rays), the size every binding of
// that header allocated; the fields added since reach a caller only through rt_stats_get_sized
// with its own sizeof(rt_stats)
constexpr size_t kStatsBytesAbi3 = offsetof(rt_stats, pass0_steps);
static_assert(kStatsBytesAbi3 == 13 * 8, "the ABI-3 rt_stats is 13 eight-byte fields");
int stats_fill(rt_ctx* c, rt_stats* st);

int rt_stats_get_sized(rt_ctx* c, rt_stats* st, size_t bytes) {
  if (!c || !st) return RT_ERR_ARG;
  rt_stats full;
  const int rc = stats_fill(c, &full);
  if (rc) return rc;
  memcpy(st, &full, std::min(bytes, sizeof(full)));
  return RT_OK;
}

int rt_stats_get(rt_ctx* c, rt_stats* st) { return rt_stats_get_sized(c, st, kStatsBytesAbi3); }

int stats_fill(rt_ctx* c, rt_stats* st) {
  if (!c || !st) return RT_ERR_ARG;
  int rc = rt_synchronize(c);
  if (rc) return rc;
  memset(st, 0, sizeof(*st));
  std::vector<unsigned long long> all(rtd::kStatWords);
  HIPCHK(c, hipMemcpy(all.data(), c->d_stats, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const unsigned long long* h = all.data();
  unsigned long long shard[3] = {0, 0, 0};  // the per-wave flushes' shard lines (rays, samples, finish steps)
  for (unsigned int s = 0; s < rtd::kStatShards; s++)
    for (int k = 0; k < 3; k++) shard[k] += h[rtd::stats_shard(s) + k];
  st->rays = h[0] + shard[0]; st->samples = h[1] + shard[1];
  st->internal_pops = h[2]; st->leaf_pops = h[3]; st->tri_tests = h[4];
  st->launches = c->launches;
  st->kernel_ms = c->kernel_ms;
  st->trace_launches = c->trace_launches;
  st->trace_ms = c->trace_ms;
  st->trace_iters = h[5];
  st->trace_iters_max = h[6];
  const unsigned long long* ps = h + 16;
  st->path_steps = ps[0];
  st->p1_rays = ps[1];
  st->pass0_steps = ps[2];
  st->pass1_steps = ps[3];
  st->finish_steps = ps[4] + shard[2];
  double busy = c->busy_closed_ms;
  for (const auto& iv : c->busy) busy += iv.hi - iv.lo;
  st->trace_busy_ms = busy;
  return RT_OK;
}

int rt_stats_reset(rt_ctx* c) {
  if (!c) return RT_ERR_ARG;
  int rc = rt_synchronize(c);
  if (rc) return rc;
  HIPCHK(c, hipMemset(c->d_stats, 0, rtd::kStatWords * sizeof(unsigned long long)));
  c->kernel_ms = 0.0;
  c->launches = 0;
  c->trace_ms = 0.0;
  c->trace_launches = 0;
  c->busy.clear();
  c->busy_closed_ms = 0.0;
  return RT_OK;
}

// Per-tile cost probe for a balanced tile assignment (rt_set_tile_owners): renders n_frames with
// the visit-counting trace, which adds every ray's node + triangle steps (+ RT_COST_PER_RAY) to
// its tile's counter.  Integer counts of a deterministic render: the same on every rank and box.
// LoopNum and the accumulation are restored afterwards; the stats counters include the probe.
// One probe render (COUNT build of wf_trace) whose per-ray traversal steps accumulate into n_bins
// costs: per local tile, or per 64-item work block (blocks); accumulation and LoopNum restored.
static int cost_probe(rt_ctx* c, const rt_frame_params* fp, const float* rand_origin, int32_t n_frames, uint64_t* costs,
                      size_t n_bins, bool blocks) {
  int rc = rt_synchronize(c);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t abytes = (size_t)std::max(1, c->max_local_tiles) * c->tile_w * c->tile_h * sizeof(float4);
  void* saved = nullptr;
  HIPCHK(c, hipMalloc(&saved, abytes));
  HIPCHK(c, hipMemcpy(saved, c->d_accum, abytes, hipMemcpyDeviceToDevice));
  const int loop = c->loop_num;
  dfree(c->d_tile_cost);
  hipError_t he = hipMalloc(&c->d_tile_cost, n_bins * sizeof(unsigned long long));
  if (he == hipSuccess) he = hipMemset(c->d_tile_cost, 0, n_bins * sizeof(unsigned long long));
  if (he != hipSuccess) {
    (void)hipFree(saved);
    return fail(c, RT_ERR_HIP, std::string("cost probe: ") + hipGetErrorString(he));
  }
  rt_frame_params q = *fp;
  q.flags = (q.flags | RT_FLAG_COUNT_VISITS) & ~RT_FLAG_MEGAKERNEL;
  // rt_order_work ranks blocks by their camera rays alone: the camera pass is the same in every
  // frame (R6), so the order does not depend on the probe frame's random bounces (C3 1080p, 10
  // probe frames: single frames 2.85-2.89 ms with it, 2.85-3.10 ms from whole-path costs)
  if (blocks) q.max_bounce = 0;
  c->tile_cost_on = true;
  c->cost_blocks = blocks;
  rc = rt_render(c, &q, rand_origin, n_frames, nullptr);
  c->tile_cost_on = false;
  c->cost_blocks = false;
  if (rc == RT_OK) {
    he = hipMemcpy(costs, c->d_tile_cost, n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) rc = fail(c, RT_ERR_HIP, std::string("cost probe: ") + hipGetErrorString(he));
  } else {
    (void)rt_synchronize(c);  // whatever the failed call queued has finished with the accumulation
  }
  // the accumulation is left as it was, on the error path too (the probe frames may have blended)
  he = hipMemcpy(c->d_accum, saved, abytes, hipMemcpyDeviceToDevice);
  if (he != hipSuccess && rc == RT_OK) rc = fail(c, RT_ERR_HIP, std::string("cost probe: ") + hipGetErrorString(he));
  (void)hipFree(saved);
  dfree(c->d_tile_cost);
  c->loop_num = loop;
  return rc;
}

#ifndef RT_ORDER_HEAD_FRAC
#define RT_ORDER_HEAD_FRAC 0.05
#endif
int rt_order_work(rt_ctx* c, const rt_frame_params* fp, const float* rand_origin, int32_t n_frames) {
  if (!c || !fp || !rand_origin || n_frames <= 0) return RT_ERR_ARG;
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "rt_resize first");
  const size_t nv = (size_t)c->n_valid, nb = nv / 64;  // whole 64-item blocks (a partial one stays last)
  if (nb < 2) return RT_OK;
  std::vector<uint64_t> cost((nv + 63) / 64);
  int rc = cost_probe(c, fp, rand_origin, n_frames, cost.data(), cost.size(), true);
  if (rc) return rc;
  std::vector<uint32_t> sorted(nb), order;
  for (size_t b = 0; b < nb; b++) sorted[b] = (uint32_t)b;
  std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
  // the costliest RT_ORDER_HEAD_FRAC of the blocks first: a one-frame call runs them as their own
  // small pixel group beside the rest, so the paths with the longest bounce chains reach their
  // finisher early (C3 1080p: 3.23 -> 3.09 ms synchronised; head 3 / 8 / 12%: -1 / -2.5 / -1.5%;
  // an even split with every group's share dealt round-robin: the round-2 default); the rest
  // follow in descending order, dealt round-robin into the remaining groups' ranges
  int G = std::max(1, c->n_groups);
  double head_frac = G >= 2 ? RT_ORDER_HEAD_FRAC : 0.0;
  if (const char* e = knob("RT_ORDER_RANGES")) G = std::max(1, atoi(e));  // (measurement)
  if (const char* e = knob("RT_ORDER_HEAD")) head_frac = atof(e);         // (measurement)
  order.reserve(nb);
  const size_t head = std::min(nb, (size_t)((double)nb * std::max(0.0, head_frac)));
  for (size_t k = 0; k < head; k++) order.push_back(sorted[k]);
  if (head > 0) G = std::max(1, G - 1);
  for (int g = 0; g < G; g++)
    for (size_t k = head + (size_t)g; k < nb; k += (size_t)G) order.push_back(sorted[k]);
  c->order_head = head * 64;
  // permute the pixel list (xy then accumulation index) by whole blocks: a wave keeps its 8x8
  // block, and the blocks whose rays cost most are queued (and claimed) first
  std::vector<unsigned int> pix(2 * nv), out(2 * nv);
  HIPCHK(c, hipMemcpy(pix.data(), c->d_pix, 2 * nv * sizeof(unsigned int), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < nb; k++)
    for (size_t j = 0; j < 64; j++) {
      out[k * 64 + j] = pix[(size_t)order[k] * 64 + j];
      out[nv + k * 64 + j] = pix[nv + (size_t)order[k] * 64 + j];
    }
  for (size_t j = nb * 64; j < nv; j++) {
    out[j] = pix[j];
    out[nv + j] = pix[nv + j];
  }
  HIPCHK(c, hipMemcpy(c->d_pix, out.data(), 2 * nv * sizeof(unsigned int), hipMemcpyHostToDevice));
  return RT_OK;
}

int rt_tile_costs(rt_ctx* c, const rt_frame_params* fp, const float* rand_origin, int32_t n_frames, uint64_t* costs) {
  if (!c || !fp || !rand_origin || !costs || n_frames <= 0) return RT_ERR_ARG;
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "rt_resize first");
  if (c->local_tiles == 0) return RT_OK;
  return cost_probe(c, fp, rand_origin, n_frames, costs, (size_t)c->local_tiles, false);
}

int rt_render(rt_ctx* c, const rt_frame_params* fp, const float* rand_origin, int32_t n_frames, rt_stats* st) {
  int rc = rt_render_async(c, fp, rand_origin, n_frames);
  if (rc) return rc;
  return st ? rt_stats_get(c, st) : rt_synchronize(c);
}

// the display pass into c->d_disp on the ctx stream (after every render call queued before it)
static int display_kernel(rt_ctx* c, const float* frame_device, int32_t flags) {
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "resize first");
  if (!frame_device && c->world != 1)
    return fail(c, RT_ERR_STATE, "a multi-rank context displays an assembled frame (rt_assemble_frame)");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)c->W * c->H * 3;
  if (bytes > c->disp_bytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier display may still read it
    dfree(c->d_disp);
    HIPCHK(c, hipMalloc(&c->d_disp, bytes));
    c->disp_bytes = bytes;
  }
  dim3 grid((c->W + 255) / 256, c->H);
  hipLaunchKernelGGL(rtd::rt_display_kernel, grid, dim3(256), 0, c->stream,
                     frame_device ? nullptr : c->d_accum, frame_device, (unsigned char*)c->d_disp, c->W, c->H,
                     c->tile_w, c->tile_h, c->tiles_x, (int)flags);
  HIPCHK(c, hipGetLastError());
  return RT_OK;
}

int rt_tonemap(rt_ctx* c, const float* frame_device, int32_t flags, uint8_t* rgb8_host) {
  if (!c || !rgb8_host) return RT_ERR_ARG;
  if (int rc = display_kernel(c, frame_device, flags)) return rc;
  HIPCHK(c, hipMemcpyAsync(rgb8_host, c->d_disp, (size_t)c->W * c->H * 3, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_tonemap_async(rt_ctx* c, const float* frame_device, int32_t flags, int32_t slot) {
  if (!c || slot < 0 || slot >= rt_ctx::DISP_SLOTS) return RT_ERR_ARG;
  rt_ctx::DisplaySlot& d = c->disp[slot];
  if (d.ev) HIPCHK(c, hipEventSynchronize(d.ev));  // the slot's previous image has been copied out
  if (int rc = display_kernel(c, frame_device, flags)) return rc;
  const size_t bytes = (size_t)c->W * c->H * 3;
  if (bytes > d.cap) {
    if (d.host) (void)hipHostFree(d.host);
    d.host = nullptr;
    d.cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&d.host, bytes));
    d.cap = bytes;
  }
  if (!d.ev) HIPCHK(c, hipEventCreateWithFlags(&d.ev, hipEventDisableTiming));
  HIPCHK(c, hipMemcpyAsync(d.host, c->d_disp, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(d.ev, c->stream));
  d.bytes = bytes;
  return RT_OK;
}

int rt_display_fetch(rt_ctx* c, int32_t slot, uint8_t* rgb8_host) {
  if (!c || !rgb8_host || slot < 0 || slot >= rt_ctx::DISP_SLOTS) return RT_ERR_ARG;
  rt_ctx::DisplaySlot& d = c->disp[slot];
  if (!d.ev || !d.bytes) return fail(c, RT_ERR_STATE, "rt_display_fetch: nothing displayed into this slot");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(d.ev));
  memcpy(rgb8_host, d.host, d.bytes);
  return RT_OK;
}

int rt_get_stream(const rt_ctx* c, void** stream) {
  if (!c || !stream) return RT_ERR_ARG;
  *stream = (void*)c->stream;
  return RT_OK;
}

int rt_set_stream(rt_ctx* c, void* stream) {
  if (!c) return RT_ERR_ARG;
  int rc = rt_synchronize(c);
  if (rc) return rc;
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  if (stream) {
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
  } else {
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return RT_OK;
}

static int accum_transfer(rt_ctx* c, float* host, int32_t layout, bool to_host) {
  if (!c || !host || (layout != RT_LAYOUT_FRAME && layout != RT_LAYOUT_LOCAL_TILES)) return RT_ERR_ARG;
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "rt_resize first");
  int rc = rt_synchronize(c);
  if (rc) return rc;
  const size_t tpx = (size_t)c->tile_w * c->tile_h;
  std::vector<float4> buf((size_t)std::max(1, c->max_local_tiles) * tpx);
  HIPCHK(c, hipMemcpy(buf.data(), c->d_accum, buf.size() * sizeof(float4), hipMemcpyDeviceToHost));
  for (int lt = 0; lt < c->local_tiles; lt++) {
    int gt = c->my_tiles[lt];
    int tx = gt % c->tiles_x, ty = gt / c->tiles_x;
    for (int ly = 0; ly < c->tile_h; ly++)
      for (int lx = 0; lx < c->tile_w; lx++) {
        size_t li = (size_t)lt * tpx + (size_t)ly * c->tile_w + lx;
        float* h;
        if (layout == RT_LAYOUT_LOCAL_TILES) {
          h = host + 3 * li;
        } else {
          int px = tx * c->tile_w + lx, py = ty * c->tile_h + ly;
          if (px >= c->W || py >= c->H) continue;
          h = host + 3 * ((size_t)py * c->W + px);
        }
        if (to_host) { h[0] = buf[li].x; h[1] = buf[li].y; h[2] = buf[li].z; }
        else buf[li] = make_float4(h[0], h[1], h[2], 0.0f);
      }
  }
  if (!to_host) HIPCHK(c, hipMemcpy(c->d_accum, buf.data(), buf.size() * sizeof(float4), hipMemcpyHostToDevice));
  return RT_OK;
}

int rt_read_accum(rt_ctx* c, float* rgb_out, int32_t layout) { return accum_transfer(c, rgb_out, layout, true); }
int rt_write_accum(rt_ctx* c, const float* rgb_in, int32_t layout) {
  return accum_transfer(c, const_cast<float*>(rgb_in), layout, false);
}

int rt_accum_device(const rt_ctx* c, void** ptr, size_t* bytes, int32_t* local_tiles, int32_t* max_local_tiles) {
  if (!c || !ptr || !bytes) return RT_ERR_ARG;
  if (!c->frame_set) return RT_ERR_STATE;
  *ptr = c->d_accum;
  *bytes = (size_t)std::max(1, c->max_local_tiles) * c->tile_w * c->tile_h * sizeof(float4);
  if (local_tiles) *local_tiles = c->local_tiles;
  if (max_local_tiles) *max_local_tiles = c->max_local_tiles;
  return RT_OK;
}

int rt_copy_accum_device(rt_ctx* c, void* dst, size_t bytes) {
  if (!c || !dst) return RT_ERR_ARG;
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "rt_resize first");
  size_t have = (size_t)std::max(1, c->max_local_tiles) * c->tile_w * c->tile_h * sizeof(float4);
  if (bytes > have) return fail(c, RT_ERR_ARG, "copy larger than the accumulation buffer");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(dst, c->d_accum, bytes, hipMemcpyDeviceToDevice, c->stream));
  return RT_OK;
}

int rt_assemble_frame(rt_ctx* c, const void* gathered, int32_t world, void* frame) {
  if (!c || !gathered || !frame || world <= 0) return RT_ERR_ARG;
  if (!c->frame_set) return fail(c, RT_ERR_STATE, "rt_resize first");
  if (world != c->world) return fail(c, RT_ERR_ARG, "world differs from the tiling");
  HIPCHK(c, hipSetDevice(c->device));
  dim3 block(256), grid((c->W + 255) / 256, c->H);
  hipLaunchKernelGGL(rtd::rt_assemble_kernel, grid, block, 0, c->stream, (const float4*)gathered, (float*)frame, c->W,
                     c->H, c->tile_w, c->tile_h, c->tiles_x, (const int2*)c->d_tile_src, std::max(1, c->max_local_tiles));
  HIPCHK(c, hipGetLastError());
  return RT_OK;
}

int rt_gather(rt_ctx* const* ctxs, int32_t n, float* full_rgb) {
  return rt_gather_ex(ctxs, n, full_rgb, RT_GATHER_AUTO);
}

// RCCL form of the gather: one communicator per context's device (ncclCommInitAll,
// this thread drives every rank), each rank's tiles sent to rank 0 on its own stream after its
// queued work, rank 0 receiving all of them (its own included) into the rank-major buffer, in one
// group.  The communicators stay in ctxs[0] for the next gather over the same devices.
static int gather_rccl(rt_ctx* const* ctxs, int n, char* g, size_t part) {
  rt_ctx* c0 = ctxs[0];
  std::vector<int> devs(n);
  for (int r = 0; r < n; r++) devs[r] = ctxs[r]->device;
  auto nfail = [&](const char* what, ncclResult_t e) {
    return fail(c0, RT_ERR_HIP, std::string("rt_gather: ") + what + ": " + ncclGetErrorString(e));
  };
  if (c0->rccl_devs != devs) {
    for (auto& m : c0->rccl_comms) (void)ncclCommDestroy(m);
    c0->rccl_comms.assign(n, nullptr);
    c0->rccl_devs.clear();
    const ncclResult_t e = ncclCommInitAll(c0->rccl_comms.data(), n, devs.data());
    if (e != ncclSuccess) {
      c0->rccl_comms.clear();
      return nfail("ncclCommInitAll", e);
    }
    c0->rccl_devs = devs;
  }
  const size_t cnt = part / sizeof(float);
  ncclResult_t e = ncclGroupStart();
  if (e != ncclSuccess) return nfail("ncclGroupStart", e);
  for (int r = 0; r < n && e == ncclSuccess; r++) {
    (void)hipSetDevice(ctxs[r]->device);
    e = ncclSend(ctxs[r]->d_accum, cnt, ncclFloat32, 0, c0->rccl_comms[r], ctxs[r]->stream);
  }
  (void)hipSetDevice(c0->device);
  for (int r = 0; r < n && e == ncclSuccess; r++)
    e = ncclRecv(g + (size_t)r * part, cnt, ncclFloat32, r, c0->rccl_comms[0], c0->stream);
  const ncclResult_t eg = ncclGroupEnd();
  (void)hipSetDevice(c0->device);
  if (e != ncclSuccess) return nfail("ncclSend / ncclRecv", e);
  if (eg != ncclSuccess) return nfail("ncclGroupEnd", eg);
  return RT_OK;
}

int rt_gather_ex(rt_ctx* const* ctxs, int32_t n, float* full_rgb, int32_t transport) {
  if (!ctxs || n <= 0 || !full_rgb || !ctxs[0]) return RT_ERR_ARG;
  if (transport != RT_GATHER_AUTO && transport != RT_GATHER_RCCL && transport != RT_GATHER_PEER) return RT_ERR_ARG;
  rt_ctx* c0 = ctxs[0];
  for (int r = 0; r < n; r++) {
    const rt_ctx* c = ctxs[r];
    if (!c) return fail(c0, RT_ERR_ARG, "rt_gather: null context");
    if (!c->frame_set) return fail(c0, RT_ERR_STATE, "rt_gather: rt_resize every context first");
    if (c->rank != r || c->world != n) return fail(c0, RT_ERR_ARG, "rt_gather: ctxs[r] must render rank r of a world of n");
    if (c->W != c0->W || c->H != c0->H || c->tile_w != c0->tile_w || c->tile_h != c0->tile_h ||
        c->max_local_tiles != c0->max_local_tiles || c->owner != c0->owner)
      return fail(c0, RT_ERR_ARG, "rt_gather: contexts differ in frame size or tiling");
  }
  bool distinct = true;  // one device per context: what an RCCL communicator needs
  for (int r = 0; r < n; r++)
    for (int q = 0; q < r; q++) distinct &= ctxs[r]->device != ctxs[q]->device;
  if (transport == RT_GATHER_AUTO) transport = distinct ? RT_GATHER_RCCL : RT_GATHER_PEER;
  if (transport == RT_GATHER_RCCL && !distinct)
    return fail(c0, RT_ERR_ARG, "rt_gather: RCCL needs one device per context (use RT_GATHER_PEER)");
  const size_t part = (size_t)std::max(1, c0->max_local_tiles) * c0->tile_w * c0->tile_h * sizeof(float4);
  const size_t frame = (size_t)c0->W * c0->H * 3 * sizeof(float);
  HIPCHK(c0, hipSetDevice(c0->device));
  if (part * n + frame > c0->gather_bytes) {
    dfree(c0->d_gather);
    c0->gather_bytes = 0;
    HIPCHK(c0, hipMalloc(&c0->d_gather, part * n + frame));
    c0->gather_bytes = part * n + frame;
  }
  char* g = static_cast<char*>(c0->d_gather);
  std::vector<std::pair<int, hipEvent_t>> done;  // (device, event) per rank, destroyed after the copy
  auto cleanup = [&]() {
    for (auto& e : done) { (void)hipSetDevice(e.first); (void)hipEventDestroy(e.second); }
    (void)hipSetDevice(c0->device);
  };
  int rc = RT_OK;
  c0->gather_transport = transport;
  if (transport == RT_GATHER_RCCL) rc = gather_rccl(ctxs, n, g, part);
  for (int r = 0; r < n && rc == RT_OK && transport == RT_GATHER_PEER; r++) {
    const rt_ctx* c = ctxs[r];
    hipEvent_t e = nullptr;
    hipError_t he = hipSetDevice(c->device);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (he == hipSuccess) done.push_back({c->device, e});
    if (he == hipSuccess) he = hipEventRecord(e, c->stream);  // after everything queued on rank r
    if (he == hipSuccess) he = hipSetDevice(c0->device);
    if (he == hipSuccess && c->device != c0->device) {  // direct xGMI copies where the link allows
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, c0->device, c->device) == hipSuccess && can) {
        const hipError_t pe = hipDeviceEnablePeerAccess(c->device, 0);
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) he = pe;
        (void)hipGetLastError();
      }
    }
    if (he == hipSuccess) he = hipStreamWaitEvent(c0->stream, e, 0);
    if (he == hipSuccess)
      he = hipMemcpyPeerAsync(g + (size_t)r * part, c0->device, c->d_accum, c->device, part, c0->stream);
    if (he != hipSuccess) rc = fail(c0, RT_ERR_HIP, std::string("rt_gather: ") + hipGetErrorString(he));
  }
  if (rc == RT_OK) rc = rt_assemble_frame(c0, g, n, g + (size_t)n * part);
  if (rc == RT_OK) {
    hipError_t he = hipMemcpyAsync(full_rgb, g + (size_t)n * part, frame, hipMemcpyDeviceToHost, c0->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c0->stream);
    if (he != hipSuccess) rc = fail(c0, RT_ERR_HIP, std::string("rt_gather: ") + hipGetErrorString(he));
  } else {
    (void)hipStreamSynchronize(c0->stream);  // the events may still be waited on
  }
  cleanup();
  return rc;
}

}  // extern "C"

// ----------------------------------------------------------------------------- ray queries
namespace {

// Rays per chunk of a query: the buffers below take 108 B per ray (24 B ray records, 4 B queue
// entry, 8 B result words, 24 + 48 B staging of the host entry points), 432 MiB at 4 Mi rays.  A
// chunk is one wf_trace launch, whose end waits for its longest rays, so larger chunks trace
// faster: 16 Mi secondary rays on C3 at 2 / 4 / 8 / 16 Mi per chunk: 3.66 / 4.88 / 5.42 / 5.66
// Grays/s closest hit, 5.01 / 7.19 / 8.21 / 8.64 any hit (profiles/query_bench_C3.md); 4 Mi takes
// most of that for under half a GB.  RT_QUERY_CHUNK (development build) sets it, so a test can
// cross chunk boundaries with a few thousand rays.
constexpr size_t kQueryChunk = size_t(4) << 20;
size_t query_chunk() {
  if (const char* e = knob("RT_QUERY_CHUNK")) return (size_t)std::max(64, atoi(e));
  return kQueryChunk;
}

// The query buffers for `rays` rays at a time (they only grow, to at most one chunk) and the
// overflow stack of the query's trace grid
int reserve_query(rt_ctx* c, size_t rays) {
  rt_ctx::Query& q = c->q;
  if (rays > q.cap) {
    if (q.mem) {  // earlier queries on the stream may still use the old buffers
      HIPCHK(c, hipStreamSynchronize(c->stream));
      (void)hipFree(q.mem);
      q.mem = nullptr;
      q.cap = 0;
    }
    const dvl::Query L = dvl::query(rays);
    if (int rc = alloc_block(c, q.mem, L.total, "query buffers do not fit in device memory")) return rc;
    rtd::WFState& S = q.S;
    S = rtd::WFState{};
    place(S.ra, q.mem, L.ra);  // one kind of ray per chunk
    S.sa = S.cam = S.ra;
    place(S.rb, q.mem, L.rb);
    S.sb = S.rb;
    place(S.queue[0], q.mem, L.queue);
    S.queue_s[0] = S.queue[0];
    place(S.res, q.mem, L.res);
    place(q.d_in, q.mem, L.d_in);
    place(q.d_out, q.mem, L.d_out);
    place(S.cnt, q.mem, L.cnt);
    place(q.d_zero, q.mem, L.zero);
    HIPCHK(c, hipMemsetAsync(q.d_zero, 0, 4, c->stream));
    q.cap = L.rays;
  }
  const size_t lanes = (size_t)c->n_cus * std::max(c->trace_bpc, c->trace_bpc0) * 256;
  const size_t need = (size_t)std::max(0, std::max(c->stack_entries, c->qstack_entries) - c->trace_lds_entries) * lanes * sizeof(int2);
  if (need > q.ovf_bytes) {
    if (q.d_ovf) HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(q.d_ovf);
    q.ovf_bytes = 0;
    HIPCHK(c, hipMalloc(&q.d_ovf, need));
    q.ovf_bytes = need;
  }
  return RT_OK;
}

// Kernel parameters of a query's launches: the scene, the culling bound for origins within
// origin_R, and the trace's launch geometry with the query's own overflow stack
void fill_query_params(const rt_ctx* c, double origin_R, int32_t flags, rtd::WFParams& WP) {
  memset(&WP, 0, sizeof(WP));
  KParams& P = WP.K;
  fill_scene_kparams(c, origin_R, P);
  P.flags = (flags & RT_QUERY_NO_CULL) ? RT_FLAG_NO_CULL : 0;
  P.n_frames = 1;
  P.rand_origin = c->q.d_zero;
  P.lds_entries = c->trace_lds_entries;
  P.pool_chunk = c->pool_chunk;
  P.stack_ovf = c->q.d_ovf;
  P.ovf_lanes = (unsigned)(c->n_cus * std::max(c->trace_bpc, c->trace_bpc0)) * 256u;
  WP.S = c->q.S;
  WP.n_frames = 1;
}

dim3 query_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>(2048, (n + 255) / 256))); }

// One chunk of caller rays (device pointers, n <= the reserved size) on the ctx stream: setup,
// trace, resolve
int query_chunk_launch(rt_ctx* c, const rtd::WFParams& WP, const float* rays_dev, size_t n, int32_t kind,
                       float origin_bound, void* out_dev) {
  const bool any = kind == RT_QUERY_ANY;
  // the any-hit kernel of split queues exists for the 4-wide tree; the binary tree's kernel takes
  // both kinds from one queue
  const bool any_kernel = any && c->wide;
  HIPCHK(c, hipMemsetAsync(WP.S.cnt, 0, rtd::kCntWords * 4, c->stream));
  const dim3 setup_grid((unsigned)std::min<size_t>(2048, (n + 4 * rtd::kSetupSpan - 1) / (4 * rtd::kSetupSpan)));
  hipLaunchKernelGGL(rtd::wf_query_setup, setup_grid, dim3(256), 0, c->stream, WP.S, rays_dev, (unsigned)n,
                     origin_bound, any ? 1 : 0, any_kernel ? rtd::cqs(0) : rtd::cq(0));
  HIPCHK(c, hipGetLastError());
  const dim3 grid((unsigned)(c->n_cus * c->trace_bpc));
  launch_trace(c, any_kernel ? rpl::SHADOW : c->wide ? rpl::CONT : rpl::REG_B, grid, WP, c->stream);
  HIPCHK(c, hipGetLastError());
  if (any) hipLaunchKernelGGL(rtd::wf_query_resolve_any, query_grid(n), dim3(256), 0, c->stream, WP.S, (unsigned)n, (int*)out_dev);
  else hipLaunchKernelGGL(rtd::wf_query_resolve<false>, query_grid(n), dim3(256), 0, c->stream, WP, (unsigned)n, (float4*)out_dev);
  HIPCHK(c, hipGetLastError());
  return RT_OK;
}

int query_args(rt_ctx* c, const void* rays, int64_t n, int32_t kind, int32_t flags, const void* out) {
  if (!c) return RT_ERR_ARG;
  if (n < 0 || (kind != RT_QUERY_CLOSEST && kind != RT_QUERY_ANY) || (flags & ~RT_QUERY_NO_CULL))
    return fail(c, RT_ERR_ARG, "bad ray count, kind or flags");
  if (n > 0 && (!rays || !out)) return fail(c, RT_ERR_ARG, "null rays or output");
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "rt_set_scene first");
  return RT_OK;
}

// The camera of a first-hit / camera-ray / pick call: finite fields, a sized frame
int camera_args(rt_ctx* c, const rt_frame_params* fp, bool need_scene) {
  if (!c || !fp) return RT_ERR_ARG;
  if (!c->frame_set || (need_scene && !c->scene_set)) return fail(c, RT_ERR_STATE, need_scene ? "rt_set_scene and rt_resize first" : "rt_resize first");
  bool ok = std::isfinite(fp->half_w) && std::isfinite(fp->half_h);
  for (int a = 0; a < 3; a++)
    ok = ok && std::isfinite(fp->position[a]) && std::isfinite(fp->left_bottom_corner[a]) && std::isfinite(fp->right[a]) &&
         std::isfinite(fp->up[a]);
  return ok ? RT_OK : fail(c, RT_ERR_ARG, "non-finite camera");
}

void fill_camera(const rt_ctx* c, const rt_frame_params* fp, KParams& P) {
  memcpy(P.pos, fp->position, 12); memcpy(P.lbc, fp->left_bottom_corner, 12);
  memcpy(P.right, fp->right, 12); memcpy(P.up, fp->up, 12);
  P.half_w = fp->half_w; P.half_h = fp->half_h;
  P.W = c->W; P.H = c->H;
}

double camera_R(const rt_frame_params* fp) {
  double r = 0.0;
  for (int a = 0; a < 3; a++) r = std::max(r, std::fabs((double)fp->position[a]));
  return r;
}

// Records of `bytes` bytes each in local-tile order on the device -> the host buffer in `layout`
// (rt_read_accum's layouts; FRAME writes only this rank's pixels)
int tiles_to_host(rt_ctx* c, const void* tiles_dev, size_t bytes, void* host, int32_t layout) {
  const size_t tpx = (size_t)c->tile_w * c->tile_h, n = (size_t)c->local_tiles * tpx;
  if (layout == RT_LAYOUT_LOCAL_TILES) {
    if (n) HIPCHK(c, hipMemcpyAsync(host, tiles_dev, n * bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
  }
  std::vector<char> buf(std::max<size_t>(1, n * bytes));
  if (n) HIPCHK(c, hipMemcpyAsync(buf.data(), tiles_dev, n * bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int lt = 0; lt < c->local_tiles; lt++) {
    const int gt = c->my_tiles[lt], tx = gt % c->tiles_x, ty = gt / c->tiles_x;
    for (int ly = 0; ly < c->tile_h; ly++) {
      const int py = ty * c->tile_h + ly, px0 = tx * c->tile_w;
      if (py >= c->H || px0 >= c->W) continue;
      const size_t run = (size_t)std::min(c->tile_w, c->W - px0);
      memcpy(static_cast<char*>(host) + ((size_t)py * c->W + px0) * bytes,
             buf.data() + ((size_t)lt * tpx + (size_t)ly * c->tile_w) * bytes, run * bytes);
    }
  }
  return RT_OK;
}

// The first-hit frame of this rank into hits_dev (local-tile order), on the ctx stream: the
// implicit camera queue over wf_camera's table, a chunk of work items at a time
int first_hit_launch(rt_ctx* c, const rt_frame_params* fp, float4* hits_dev) {
  const size_t nv = (size_t)c->n_valid, chunk = query_chunk();
  if (int rc = reserve_query(c, std::min(nv, chunk))) return rc;
  rtd::WFParams WP;
  fill_query_params(c, camera_R(fp), (fp->flags & RT_FLAG_NO_CULL) ? RT_QUERY_NO_CULL : 0, WP);
  fill_camera(c, fp, WP.K);
  for (size_t w0 = 0; w0 < nv; w0 += chunk) {
    const unsigned int n = (unsigned)std::min(chunk, nv - w0);
    WP.K.n_work = n;
    WP.cam_n = n;
    WP.S.pix_xy = c->wf.pix_xy + w0;
    WP.S.pix_acc = c->wf.pix_acc + w0;
    rtd::GroupCounters Z;
    memset(&Z, 0, sizeof(Z));
    Z.n = 1;
    Z.cnt[0] = WP.S.cnt;
    hipLaunchKernelGGL(rtd::wf_camera, query_grid(n), dim3(256), 0, c->stream, WP, Z);
    HIPCHK(c, hipGetLastError());
    const dim3 grid((unsigned)(c->n_cus * c->trace_bpc0));
    launch_trace(c, c->wide ? rpl::CAM_W : rpl::CAM_B, grid, WP, c->stream);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(rtd::wf_query_resolve<true>, query_grid(n), dim3(256), 0, c->stream, WP, n, hits_dev);
    HIPCHK(c, hipGetLastError());
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_trace_rays_device(rt_ctx* c, const void* rays_dev, int64_t n, int32_t kind, int32_t flags, float origin_bound,
                         void* out_dev) {
  if (int rc = query_args(c, rays_dev, n, kind, flags, out_dev)) return rc;
  if (!(origin_bound >= 0.0f)) return fail(c, RT_ERR_ARG, "origin_bound must be >= 0");
  if (n == 0) return RT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t chunk = query_chunk();
  if (int rc = reserve_query(c, std::min((size_t)n, chunk))) return rc;
  rtd::WFParams WP;
  fill_query_params(c, (double)origin_bound, flags, WP);
  const size_t out_bytes = kind == RT_QUERY_ANY ? sizeof(int32_t) : sizeof(rt_hit);
  for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
    const size_t m = std::min(chunk, (size_t)n - i0);
    if (int rc = query_chunk_launch(c, WP, static_cast<const float*>(rays_dev) + 6 * i0, m, kind, origin_bound,
                                    static_cast<char*>(out_dev) + i0 * out_bytes))
      return rc;
  }
  return RT_OK;
}

int rt_trace_rays(rt_ctx* c, const rt_ray* rays, int64_t n, int32_t kind, int32_t flags, void* out) {
  if (int rc = query_args(c, rays, n, kind, flags, out)) return rc;
  if (n == 0) return RT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // the culling bound must cover the origins that are traced (a non-finite one never is)
  float bound = 0.0f;
  for (int64_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) {
      const float o = std::fabs(rays[i].origin[a]);
      if (std::isfinite(o)) bound = std::max(bound, o);
    }
  const size_t chunk = query_chunk();
  if (int rc = reserve_query(c, std::min((size_t)n, chunk))) return rc;
  rtd::WFParams WP;
  fill_query_params(c, (double)bound, flags, WP);
  const size_t out_bytes = kind == RT_QUERY_ANY ? sizeof(int32_t) : sizeof(rt_hit);
  for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
    const size_t m = std::min(chunk, (size_t)n - i0);
    HIPCHK(c, hipMemcpyAsync(c->q.d_in, rays + i0, m * sizeof(rt_ray), hipMemcpyHostToDevice, c->stream));
    if (int rc = query_chunk_launch(c, WP, c->q.d_in, m, kind, bound, c->q.d_out)) return rc;
    HIPCHK(c, hipMemcpyAsync(static_cast<char*>(out) + i0 * out_bytes, c->q.d_out, m * out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffers are reused by the next chunk
  }
  return RT_OK;
}

int rt_camera_rays(rt_ctx* c, const rt_frame_params* fp, rt_ray* rays, int32_t layout) {
  if (int rc = camera_args(c, fp, false)) return rc;
  if (!rays || (layout != RT_LAYOUT_FRAME && layout != RT_LAYOUT_LOCAL_TILES)) return fail(c, RT_ERR_ARG, "null rays or bad layout");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->local_tiles * c->tile_w * c->tile_h;
  float* d = nullptr;  // (a one-off table of the whole frame: not the chunked query buffers)
  HIPCHK(c, hipMalloc(&d, std::max<size_t>(1, n) * sizeof(rt_ray)));
  KParams P;
  memset(&P, 0, sizeof(P));
  fill_camera(c, fp, P);
  int rc = RT_OK;
  if (c->n_valid > 0) {
    hipLaunchKernelGGL(rtd::wf_query_camera, query_grid((size_t)c->n_valid), dim3(256), 0, c->stream, P, c->wf.pix_xy,
                       c->wf.pix_acc, (unsigned)c->n_valid, 0u, d);
    if (hipGetLastError() != hipSuccess) rc = fail(c, RT_ERR_HIP, "wf_query_camera launch failed");
  }
  if (!rc) rc = tiles_to_host(c, d, sizeof(rt_ray), rays, layout);
  (void)hipFree(d);
  return rc;
}

int rt_first_hit_device(rt_ctx* c, const rt_frame_params* fp, void* hits_dev) {
  if (int rc = camera_args(c, fp, true)) return rc;
  if (!hits_dev) return fail(c, RT_ERR_ARG, "null output");
  HIPCHK(c, hipSetDevice(c->device));
  return first_hit_launch(c, fp, static_cast<float4*>(hits_dev));
}

int rt_first_hit(rt_ctx* c, const rt_frame_params* fp, rt_hit* hits, int32_t layout) {
  if (int rc = camera_args(c, fp, true)) return rc;
  if (!hits || (layout != RT_LAYOUT_FRAME && layout != RT_LAYOUT_LOCAL_TILES)) return fail(c, RT_ERR_ARG, "null hits or bad layout");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->local_tiles * c->tile_w * c->tile_h;
  float4* d = nullptr;  // (the whole frame's records, tile pixels outside the frame zeroed)
  HIPCHK(c, hipMalloc(&d, std::max<size_t>(1, n) * sizeof(rt_hit)));
  int rc = RT_OK;
  if (hipMemsetAsync(d, 0, std::max<size_t>(1, n) * sizeof(rt_hit), c->stream) != hipSuccess) rc = fail(c, RT_ERR_HIP, "hipMemsetAsync failed");
  if (!rc) rc = first_hit_launch(c, fp, d);
  if (!rc) rc = tiles_to_host(c, d, sizeof(rt_hit), hits, layout);
  else (void)hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  return rc;
}

int rt_pick(rt_ctx* c, const rt_frame_params* fp, int32_t px, int32_t py, rt_hit* hit) {
  if (int rc = camera_args(c, fp, true)) return rc;
  if (!hit) return fail(c, RT_ERR_ARG, "null hit");
  if (px < 0 || py < 0 || px >= c->W || py >= c->H) return fail(c, RT_ERR_ARG, "pixel outside the frame");
  if (c->owner[(size_t)(py / c->tile_h) * c->tiles_x + px / c->tile_w] != c->rank)
    return fail(c, RT_ERR_ARG, "pixel not owned by this rank");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = reserve_query(c, 1)) return rc;
  // the pixel's camera ray as wf_camera computes it, then a closest-hit query of one ray
  const float bound = (float)camera_R(fp);  // (exact: a float's magnitude)
  rtd::WFParams WP;
  fill_query_params(c, (double)bound, (fp->flags & RT_FLAG_NO_CULL) ? RT_QUERY_NO_CULL : 0, WP);
  KParams PC;
  memset(&PC, 0, sizeof(PC));
  fill_camera(c, fp, PC);
  hipLaunchKernelGGL(rtd::wf_query_camera, dim3(1), dim3(256), 0, c->stream, PC, (const unsigned int*)nullptr,
                     (const unsigned int*)nullptr, 1u, (unsigned)px | ((unsigned)py << 16), c->q.d_in);
  HIPCHK(c, hipGetLastError());
  if (int rc = query_chunk_launch(c, WP, c->q.d_in, 1, RT_QUERY_CLOSEST, bound, c->q.d_out)) return rc;
  HIPCHK(c, hipMemcpyAsync(hit, c->q.d_out, sizeof(rt_hit), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_get_triangle_material(rt_ctx* c, int32_t triangle, rt_material* out, int32_t* material_id) {
  if (!c) return RT_ERR_ARG;
  if (!c->scene_set) return fail(c, RT_ERR_STATE, "rt_set_scene first");
  if (triangle < 0 || triangle >= c->n_tri) return fail(c, RT_ERR_ARG, "triangle outside the triangle list");
  const int id = c->tri_mat[(size_t)triangle];
  if (out) memcpy(out, &c->mat_table[32 * (size_t)id], sizeof(rt_material));  // pack_material keeps the 24 floats verbatim
  if (material_id) *material_id = id;
  return RT_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------- display denoiser
namespace {

// An iteration with s >= 4 runs the LDS kernel over one residue class per block (true) or direct
// global reads.  C3 1080p, us per launch, class / direct: s = 4 125 / 97, s = 8 83 / 104, s = 16
// 84 / 99 (Appendix A has the form rejected at each step).  RT_DN_FAR=lds|direct
// (development build) forces one form for every s >= 4, to repeat that measurement.
bool dn_far_lds(int s) {
  if (const char* e = knob("RT_DN_FAR")) return strcmp(e, "lds") == 0;
  return s >= 8;
}

// The denoiser's buffers for the current frame size (apply_tiling dropped those of another size)
int reserve_denoise(rt_ctx* c) {
  rt_ctx::Denoise& d = c->dn;
  if (d.mem) return RT_OK;
  const dvl::Denoise L = dvl::denoise((size_t)c->W * c->H, (size_t)std::max(1, c->local_tiles) * c->tile_w * c->tile_h);
  if (int rc = alloc_block(c, d.mem, L.total, "denoise buffers do not fit in device memory")) return rc;
  for (int k = 0; k < 2; k++) place(d.col[k], d.mem, L.col[k]);
  place(d.g0, d.mem, L.g0);
  place(d.g1, d.mem, L.g1);
  place(d.hits, d.mem, L.hits);
  place(d.out, d.mem, L.out);
  d.guides = false;
  return RT_OK;
}

bool dn_sigma_ok(float s) { return std::isfinite(s) && s > 0.0f; }

// The display history's buffers for the current frame size (after reserve_denoise: gp[0] is the
// denoiser's guide pair)
int reserve_temporal(rt_ctx* c) {
  rt_ctx::Temporal& t = c->tp;
  if (t.mem) return RT_OK;
  const dvl::History L = dvl::history((size_t)c->W * c->H);
  if (int rc = alloc_block(c, t.mem, L.total, "display history does not fit in device memory")) return rc;
  for (int k = 0; k < 2; k++) place(t.col[k], t.mem, L.col[k]);
  t.gp[0][0] = c->dn.g0;
  t.gp[0][1] = c->dn.g1;
  for (int k = 1; k < 3; k++)
    for (int j = 0; j < 2; j++) place(t.gp[k][j], t.mem, L.gp[k - 1][j]);
  place(t.out, t.mem, L.out);
  t.drop();
  return RT_OK;
}

// The motion mode's buffers (the mode is on): the triangle frames for the current frame size, the
// pose slots for the current scene
int reserve_tri_frames(rt_ctx* c) {
  rt_ctx::Motion& m = c->mo;
  if (m.tf_mem) return RT_OK;
  const dvl::TriFrames L = dvl::tri_frames((size_t)c->W * c->H);
  if (int rc = alloc_block(c, m.tf_mem, L.total, "triangle frames do not fit in device memory")) return rc;
  for (int k = 0; k < 3; k++) place(m.tf[k], m.tf_mem, L.tf[k]);
  for (bool& v : m.tf_valid) v = false;
  return RT_OK;
}
int reserve_poses(rt_ctx* c) {
  rt_ctx::Motion& m = c->mo;
  if (m.pose_mem) return RT_OK;
  const dvl::Poses L = dvl::poses((size_t)c->n_tri);
  if (int rc = alloc_block(c, m.pose_mem, std::max<size_t>(L.total, 256), "scene poses do not fit in device memory")) return rc;
  for (int k = 0; k < 2; k++) {
    place(m.tri[k], m.pose_mem, L.tri[k]);
    place(m.trin[k], m.pose_mem, L.trin[k]);
  }
  c->tp.pose_gen[0] = c->tp.pose_gen[1] = -1;
  return RT_OK;
}

// The variance mode's frames for the current frame size (the mode is on)
int reserve_variance(rt_ctx* c) {
  rt_ctx::Variance& v = c->vr;
  if (v.mem) return RT_OK;
  const dvl::Variance L = dvl::variance((size_t)c->W * c->H);
  if (int rc = alloc_block(c, v.mem, L.total, "variance frames do not fit in device memory")) return rc;
  for (int k = 0; k < 2; k++) place(v.st[k], v.mem, L.st[k]);
  place(v.tvar, v.mem, L.tvar);
  for (int k = 0; k < 2; k++) place(v.dvar[k], v.mem, L.dvar[k]);
  v.tvar_valid = false;
  v.last = nullptr;
  return RT_OK;
}

// The guide pair dn.g0 / dn.g1 point at (0, the denoiser's own, without a display history)
int tp_current_pair(const rt_ctx* c) {
  for (int k = 1; k < 3; k++)
    if (c->tp.mem && c->tp.gp[k][0] == c->dn.g0) return k;
  return 0;
}

// Before a fresh pack of the current guides: point dn.g0 / dn.g1 at a pair that the history does
// not hold, nor (keep_cand) the candidate; the pair they point at when that one is free.  Without a
// display history the denoiser's own pair stays.  Returns the pair's index.
int tp_guides_target(rt_ctx* c, bool keep_cand) {
  rt_ctx::Temporal& t = c->tp;
  if (!t.mem) return 0;
  int cur = tp_current_pair(c);
  auto taken = [&](int k) { return k == t.hist_g || (keep_cand && k == t.cand_g); };
  for (int k = 0; k < 3 && taken(cur); k++) cur = k;
  c->dn.g0 = t.gp[cur][0];
  c->dn.g1 = t.gp[cur][1];
  return cur;
}

// The state a display stage (rt_denoise_async, rt_temporal_async) needs, checked after its own
// arguments: a scene and a frame, one rank, guides to reuse, a camera where one is read
int display_state(rt_ctx* c, const rt_frame_params* fp, bool reuse, bool camera, const char* no_guides) {
  if (!c->scene_set || !c->frame_set) return fail(c, RT_ERR_STATE, "rt_set_scene and rt_resize first");
  if (c->world != 1) return fail(c, RT_ERR_STATE, "a multi-rank context has guides for its own pixels only");
  if (reuse && !(c->dn.mem && c->dn.guides)) return fail(c, RT_ERR_STATE, no_guides);
  if (camera)
    if (int rc = camera_args(c, fp, true)) return rc;
  return RT_OK;
}

// A display stage's input, after its reserve: the frame's colour in dn.col[0] and the current
// guides in dn.g0 / dn.g1 = guide pair `pair` (a fresh pack's: tp_guides_target), from the caller's
// hits or the library's own first-hit trace.
// The pack reads the accumulation on the ctx stream, after the render calls queued before it
// (the stream joins each of them); a render call queued afterwards blends only after it, as
// after rt_tonemap_async's pass (a pipelined call's blend waits for the ctx stream at its entry).
int display_pack(rt_ctx* c, const rt_frame_params* fp, bool reuse, const float* frame_in_device, const void* hits_dev,
                 bool keep_cand, int& pair) {
  rt_ctx::Denoise& d = c->dn;
  pair = reuse ? tp_current_pair(c) : tp_guides_target(c, keep_cand);
  if (!reuse && c->mo.on)
    if (int rc = reserve_tri_frames(c)) return rc;
  if (!reuse && !hits_dev) {
    d.guides = false;  // (they are being replaced: a failure below leaves none)
    if (int rc = first_hit_launch(c, fp, d.hits)) return rc;
  }
  const dim3 pgrid((c->W + 255) / 256, c->H);
  const float4* tiles = frame_in_device ? nullptr : c->d_accum;
  if (reuse)
    hipLaunchKernelGGL(rtd::dn_pack<false>, pgrid, dim3(256), 0, c->stream, tiles, frame_in_device, (const float4*)nullptr,
                       d.col[0], d.g0, d.g1, c->W, c->H, c->tile_w, c->tile_h, c->tiles_x);
  else
    hipLaunchKernelGGL(rtd::dn_pack<true>, pgrid, dim3(256), 0, c->stream, tiles, frame_in_device,
                       hits_dev ? (const float4*)hits_dev : d.hits, d.col[0], d.g0, d.g1, c->W, c->H, c->tile_w,
                       c->tile_h, c->tiles_x);
  HIPCHK(c, hipGetLastError());
  if (!reuse) {  // the pair's triangle frame: this pack's in motion mode, else none
    c->mo.tf_valid[pair] = c->mo.on;
    if (c->mo.on) {
      hipLaunchKernelGGL(rtd::tp_pack_tri, pgrid, dim3(256), 0, c->stream, hits_dev ? (const float4*)hits_dev : d.hits,
                         c->mo.tf[pair], c->W, c->H, c->tile_w, c->tile_h, c->tiles_x);
      HIPCHK(c, hipGetLastError());
    }
  }
  d.guides = true;
  return RT_OK;
}

// The blocking forms' tail: the stage's output frame (W*H*3 floats) to the host
int display_fetch(rt_ctx* c, const float* out, float* rgb_out_host) {
  HIPCHK(c, hipMemcpyAsync(rgb_out_host, out, (size_t)c->W * c->H * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise_default_params(rt_denoise_params* dp) {
  if (!dp) return RT_ERR_ARG;
  dp->iterations = 5;
  dp->sigma_color = 1.0f;
  dp->sigma_normal = 0.3f;
  dp->sigma_plane = 0.01f;
  dp->flags = 0;
  return RT_OK;
}

int rt_denoise_async(rt_ctx* c, const rt_frame_params* fp, const rt_denoise_params* dp, const float* frame_in_device,
                     const void* hits_dev, float** frame_out_device) {
  if (!c) return RT_ERR_ARG;
  if (!dp || !frame_out_device) return fail(c, RT_ERR_ARG, "null parameters or output");
  if (dp->iterations < 1 || dp->iterations > 5) return fail(c, RT_ERR_ARG, "iterations outside 1..5");
  if (!dn_sigma_ok(dp->sigma_color) || !dn_sigma_ok(dp->sigma_normal) || !dn_sigma_ok(dp->sigma_plane))
    return fail(c, RT_ERR_ARG, "a sigma is not finite and > 0");
  if (dp->flags & ~RT_DENOISE_REUSE_GUIDES) return fail(c, RT_ERR_ARG, "unknown flags");
  const bool reuse = (dp->flags & RT_DENOISE_REUSE_GUIDES) != 0;
  const bool trace = !reuse && !hits_dev;
  if (trace && !fp) return fail(c, RT_ERR_ARG, "null frame parameters");
  if (int rc = display_state(c, fp, reuse, trace, "no guides of an earlier denoise call for this size")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = reserve_denoise(c)) return rc;
  const bool var_mode = c->vr.p.on != 0;
  if (var_mode)
    if (int rc = reserve_variance(c)) return rc;
  rt_ctx::Denoise& d = c->dn;
  int pair;  // (a live candidate of the display history keeps its guides)
  if (int rc = display_pack(c, fp, reuse, frame_in_device, hits_dev, true, pair)) return rc;
  rtd::DnIter I;
  I.g0 = d.g0;
  I.g1 = d.g1;
  I.W = c->W;
  I.H = c->H;
  I.kn = 1.0f / (dp->sigma_normal * dp->sigma_normal);
  I.kp = 1.0f / (dp->sigma_plane * dp->sigma_plane);
  I.kc = 1.0f / (dp->sigma_color * dp->sigma_color);
  auto tiles_of = [](int n, int t) { return (unsigned)((n + t - 1) / t); };
  rt_ctx::Variance& vr = c->vr;
  rtd::DnVar V{};
  if (var_mode) {
    // The input's variance: the temporal stage's when the input is its output, else unknown; the
    // spatial estimate fills what is unknown
    const float* src = (frame_in_device && frame_in_device == c->tp.out && c->tp.cand >= 0 && vr.tvar_valid) ? vr.tvar : nullptr;
    I.cin = d.col[0];
    I.cout = nullptr;
    I.out3 = nullptr;
    I.s = 1;
    const dim3 grid(tiles_of(c->W, rtd::kDnTW), tiles_of(c->H, rtd::kDnTH), 1);
    hipLaunchKernelGGL(rtd::dn_var_spatial, grid, dim3(256), 0, c->stream, I, src, vr.dvar[0],
                       dp->sigma_normal * dp->sigma_normal, dp->sigma_plane);
    HIPCHK(c, hipGetLastError());
    V.sl = vr.p.sigma_lum;
  }
  for (int i = 0; i < dp->iterations; i++) {
    const bool last = i + 1 == dp->iterations;
    const int s = 1 << i;
    I.cin = d.col[i & 1];
    I.cout = last ? nullptr : d.col[(i + 1) & 1];
    I.out3 = last ? d.out : nullptr;
    I.s = s;
    if (var_mode) {  // the same forms for the same s, with the variance beside the colour
      V.vin = vr.dvar[i & 1];
      V.vout = vr.dvar[(i + 1) & 1];
      if (s <= 2) {
        const dim3 grid(tiles_of(c->W, rtd::kDnTW), tiles_of(c->H, rtd::kDnTH), 1);
        if (s == 1) hipLaunchKernelGGL(rtd::dn_atrous_lds_var<1>, grid, dim3(256), 0, c->stream, I, 1, V);
        else hipLaunchKernelGGL(rtd::dn_atrous_lds_var<2>, grid, dim3(256), 0, c->stream, I, 1, V);
      } else if (dn_far_lds(s)) {
        const dim3 grid(tiles_of((c->W + s - 1) / s, rtd::kDnTW), tiles_of((c->H + s - 1) / s, rtd::kDnTH), (unsigned)(s * s));
        hipLaunchKernelGGL(rtd::dn_atrous_lds_var<1>, grid, dim3(256), 0, c->stream, I, s, V);
      } else {
        const dim3 grid(tiles_of(c->W, rtd::kDnTW), tiles_of(c->H, rtd::kDnTH), 1);
        hipLaunchKernelGGL(rtd::dn_atrous_direct_var, grid, dim3(256), 0, c->stream, I, V);
      }
      vr.last = V.vout;
    } else if (s <= 2) {
      const dim3 grid(tiles_of(c->W, rtd::kDnTW), tiles_of(c->H, rtd::kDnTH), 1);
      if (s == 1) hipLaunchKernelGGL(rtd::dn_atrous_lds<1>, grid, dim3(256), 0, c->stream, I, 1);
      else hipLaunchKernelGGL(rtd::dn_atrous_lds<2>, grid, dim3(256), 0, c->stream, I, 1);
    } else if (dn_far_lds(s)) {  // class (0, 0) is the largest: ceil(W / s) x ceil(H / s)
      const dim3 grid(tiles_of((c->W + s - 1) / s, rtd::kDnTW), tiles_of((c->H + s - 1) / s, rtd::kDnTH), (unsigned)(s * s));
      hipLaunchKernelGGL(rtd::dn_atrous_lds<1>, grid, dim3(256), 0, c->stream, I, s);
    } else {
      const dim3 grid(tiles_of(c->W, rtd::kDnTW), tiles_of(c->H, rtd::kDnTH), 1);
      hipLaunchKernelGGL(rtd::dn_atrous_direct, grid, dim3(256), 0, c->stream, I);
    }
    HIPCHK(c, hipGetLastError());
    I.kc = I.kc * 4.0f;
  }
  *frame_out_device = d.out;
  return RT_OK;
}

int rt_denoise(rt_ctx* c, const rt_frame_params* fp, const rt_denoise_params* dp, float* rgb_out_host) {
  if (!c) return RT_ERR_ARG;
  if (!rgb_out_host) return fail(c, RT_ERR_ARG, "null output");
  float* out = nullptr;
  if (int rc = rt_denoise_async(c, fp, dp, nullptr, nullptr, &out)) return rc;
  return display_fetch(c, out, rgb_out_host);
}

// ----------------------------------------------------------------------------- display history
int rt_temporal_default_params(rt_temporal_params* tp) {
  if (!tp) return RT_ERR_ARG;
  tp->samples = 1;
  tp->max_history = 32;
  tp->sigma_normal = 0.3f;
  tp->sigma_plane = 0.01f;
  tp->flags = 0;
  return RT_OK;
}

int rt_temporal_async(rt_ctx* c, const rt_frame_params* fp, const rt_temporal_params* tp, const float* frame_in_device,
                      const void* hits_dev, float** frame_out_device) {
  if (!c) return RT_ERR_ARG;
  if (!tp || !frame_out_device) return fail(c, RT_ERR_ARG, "null parameters or output");
  if (!fp) return fail(c, RT_ERR_ARG, "null frame parameters");  // (never ignored: the output is stored with its camera)
  if (tp->samples < 1) return fail(c, RT_ERR_ARG, "samples < 1");
  if (tp->max_history < 1) return fail(c, RT_ERR_ARG, "max_history < 1");
  if (!dn_sigma_ok(tp->sigma_normal) || !dn_sigma_ok(tp->sigma_plane)) return fail(c, RT_ERR_ARG, "a sigma is not finite and > 0");
  if (tp->flags & ~(RT_TEMPORAL_ADVANCE | RT_TEMPORAL_REUSE_GUIDES | RT_TEMPORAL_RESET)) return fail(c, RT_ERR_ARG, "unknown flags");
  const bool reuse = (tp->flags & RT_TEMPORAL_REUSE_GUIDES) != 0;
  if (int rc = display_state(c, fp, reuse, true, "no guides of an earlier denoise or temporal call for this size")) return rc;
  if (reuse && c->mo.on && !c->mo.tf_valid[tp_current_pair(c)])
    return fail(c, RT_ERR_STATE, "the current guides were packed without their triangle frame (before rt_temporal_set_motion)");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(fp->front[a])) return fail(c, RT_ERR_ARG, "non-finite camera");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = reserve_denoise(c)) return rc;
  if (int rc = reserve_temporal(c)) return rc;
  if (c->mo.on)
    if (int rc = reserve_poses(c)) return rc;
  const bool var_mode = c->vr.p.on != 0;
  if (var_mode)
    if (int rc = reserve_variance(c)) return rc;
  rt_ctx::Denoise& d = c->dn;
  rt_ctx::Temporal& t = c->tp;
  // (variance mode) this call overwrites the previous call's candidate in place: the same view
  const bool own = t.cand >= 0 && !(tp->flags & (RT_TEMPORAL_RESET | RT_TEMPORAL_ADVANCE));
  // The previous output changes roles: the history (ADVANCE), or nothing (this call's replaces it)
  if (tp->flags & RT_TEMPORAL_RESET) {
    t.drop();
  } else if ((tp->flags & RT_TEMPORAL_ADVANCE) && t.cand >= 0) {
    t.hist = t.cand;
    t.hist_g = t.cand_g;
    t.hist_fp = t.cand_fp;
  }
  t.cand = t.cand_g = -1;
  int pair;  // (the old candidate's is free)
  if (int rc = display_pack(c, fp, reuse, frame_in_device, hits_dev, false, pair)) return rc;
  const int cand = t.hist == 0 ? 1 : 0;
  rtd::TpCall T;
  T.cur = d.col[0];
  T.g0 = d.g0;
  T.g1 = d.g1;
  T.hc = t.hist >= 0 ? t.col[t.hist] : nullptr;
  T.hg0 = t.hist >= 0 ? t.gp[t.hist_g][0] : nullptr;
  T.hg1 = t.hist >= 0 ? t.gp[t.hist_g][1] : nullptr;
  T.cand = t.col[cand];
  T.out3 = t.out;
  T.W = c->W;
  T.H = c->H;
  const rt_frame_params& h = t.hist_fp;  // (all zero without a history: not read)
  memcpy(T.pos, h.position, 12); memcpy(T.front, h.front, 12); memcpy(T.right, h.right, 12);
  memcpy(T.up, h.up, 12); memcpy(T.lbc, h.left_bottom_corner, 12);
  T.tw = 2.0f * h.half_w;
  T.th = 2.0f * h.half_h;
  T.S = (float)tp->samples;
  T.max_n = (float)tp->max_history;
  T.sn2 = tp->sigma_normal * tp->sigma_normal;
  T.sp = tp->sigma_plane;
  const dim3 grid((unsigned)((c->W + rtd::kDnTW - 1) / rtd::kDnTW), (unsigned)((c->H + rtd::kDnTH - 1) / rtd::kDnTH));
  rt_ctx::Motion& m = c->mo;
  rtd::TpVar V{};
  if (var_mode) {
    V.hst = t.hist >= 0 ? c->vr.st[t.hist] : nullptr;
    V.st = c->vr.st[cand];
    V.var = c->vr.tvar;
    V.own = own ? 1 : 0;
    V.max_m = (float)c->vr.p.max_estimates;
  }
  // The motion form only where the history was made from another pose than the current one
  if (m.on && t.hist >= 0 && t.pose_gen[t.hist] >= 0 && t.pose_gen[t.hist] != m.gen) {
    rtd::TpMotion Mo;
    Mo.tf = m.tf[pair];
    Mo.tri = c->d_tri;
    Mo.trin = c->d_trin;
    Mo.htri = m.tri[t.hist];
    Mo.htrin = m.trin[t.hist];
    Mo.n_tri = c->n_tri;
    if (var_mode) hipLaunchKernelGGL(rtd::tp_resolve_motion_var, grid, dim3(256), 0, c->stream, T, Mo, V);
    else hipLaunchKernelGGL(rtd::tp_resolve_motion, grid, dim3(256), 0, c->stream, T, Mo);
  } else if (var_mode) {
    hipLaunchKernelGGL(rtd::tp_resolve_var, grid, dim3(256), 0, c->stream, T, V);
  } else {
    hipLaunchKernelGGL(rtd::tp_resolve, grid, dim3(256), 0, c->stream, T);
  }
  HIPCHK(c, hipGetLastError());
  if (var_mode) {
    c->vr.tvar_valid = true;
    c->vr.last = c->vr.tvar;
  }
  // The candidate was made from the current pose: its slot holds it, copied once per generation
  if (m.on && t.pose_gen[cand] != m.gen) {
    const size_t bytes = (size_t)c->n_tri * dvl::kTriRecBytes;
    t.pose_gen[cand] = -1;
    if (bytes) {
      HIPCHK(c, hipMemcpyAsync(m.tri[cand], c->d_tri, bytes, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(m.trin[cand], c->d_trin, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    t.pose_gen[cand] = m.gen;
  }
  t.cand = cand;
  t.cand_g = pair;
  t.cand_fp = *fp;
  *frame_out_device = t.out;
  return RT_OK;
}

int rt_temporal(rt_ctx* c, const rt_frame_params* fp, const rt_temporal_params* tp, float* rgb_out_host) {
  if (!c) return RT_ERR_ARG;
  if (!rgb_out_host) return fail(c, RT_ERR_ARG, "null output");
  float* out = nullptr;
  if (int rc = rt_temporal_async(c, fp, tp, nullptr, nullptr, &out)) return rc;
  return display_fetch(c, out, rgb_out_host);
}

int rt_temporal_set_motion(rt_ctx* c, int32_t on) {
  if (!c) return RT_ERR_ARG;
  if (on != 0 && on != 1) return fail(c, RT_ERR_ARG, "on is 0 or 1");
  if (int rc = rt_synchronize(c)) return rc;  // (a temporal call in flight reads the buffers freed below)
  c->tp.drop();
  motion_free_poses(c);
  motion_free_frames(c);
  c->mo.on = on != 0;
  return RT_OK;
}

int rt_temporal_get_motion(const rt_ctx* c, int32_t* on) {
  if (!c || !on) return RT_ERR_ARG;
  *on = c->mo.on ? 1 : 0;
  return RT_OK;
}

int rt_temporal_history(rt_ctx* c, float* n_out_host) {
  if (!c) return RT_ERR_ARG;
  if (!n_out_host) return fail(c, RT_ERR_ARG, "null output");
  if (!c->tp.mem || c->tp.cand < 0) return fail(c, RT_ERR_STATE, "no temporal call for the current size and scene");
  const size_t npx = (size_t)c->W * c->H;
  std::vector<float> buf(4 * npx);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(buf.data(), c->tp.col[c->tp.cand], npx * 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < npx; i++) n_out_host[i] = buf[4 * i + 3];
  return RT_OK;
}

// ----------------------------------------------------------------------------- variance mode
int rt_variance_default_params(rt_variance_params* vp) {
  if (!vp) return RT_ERR_ARG;
  *vp = rt_ctx::Variance{}.p;
  return RT_OK;
}

int rt_variance_set(rt_ctx* c, const rt_variance_params* vp) {
  if (!c) return RT_ERR_ARG;
  if (!vp) return fail(c, RT_ERR_ARG, "null parameters");
  if (vp->on != 0 && vp->on != 1) return fail(c, RT_ERR_ARG, "on is 0 or 1");
  if (!dn_sigma_ok(vp->sigma_lum)) return fail(c, RT_ERR_ARG, "sigma_lum is not finite and > 0");
  if (vp->max_estimates < 1) return fail(c, RT_ERR_ARG, "max_estimates < 1");
  if (vp->flags != 0) return fail(c, RT_ERR_ARG, "unknown flags");
  if (int rc = rt_synchronize(c)) return rc;  // (a display stage in flight reads the buffers freed below)
  c->tp.drop();  // (a history made outside the mode has no state texels)
  c->vr.tvar_valid = false;
  c->vr.last = nullptr;
  if (!vp->on) variance_free(c);
  c->vr.p = *vp;
  return RT_OK;
}

int rt_variance_get(const rt_ctx* c, rt_variance_params* vp) {
  if (!c || !vp) return RT_ERR_ARG;
  *vp = c->vr.p;
  return RT_OK;
}

int rt_variance_frame(rt_ctx* c, float* var_out_host) {
  if (!c) return RT_ERR_ARG;
  if (!var_out_host) return fail(c, RT_ERR_ARG, "null output");
  if (!c->vr.p.on || !c->vr.mem || !c->vr.last) return fail(c, RT_ERR_STATE, "no temporal or denoise call in the variance mode for the current size");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(var_out_host, c->vr.last, (size_t)c->W * c->H * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RT_OK;
}

}  // extern "C"
