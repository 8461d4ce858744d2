/* rt_abi.h — C-ABI of the MI355X path tracer (librtamd.so, HIP for gfx950).
 *
 * Drop-in replacement for the reference's OpenGL program interface of the path-tracing
 * fragment shader (src/shaders/fragment_shader_ray_tracing.glsl, "RT:"), which the
 * reference drives from src/sources/main.cpp.  Entry point -> reference interface:
 *
 *   rt_create / rt_destroy   <- Shader RayTracerShader(...) + GL context (src/core/Shader.h:21-108,
 *                               main.cpp:93-95)
 *   rt_set_scene             <- EncodedBVHandTriangles() glBufferData/glTexBuffer uploads of the
 *                               triangle and BVH texture buffers (src/core/Scene.h:240-256) and the
 *                               nTriangles/nNodes uniforms (main.cpp:135-136); SoA instead of AoS
 *   rt_set_scene_encoded     <- the same upload taking the reference's AoS encodings verbatim
 *                               (Triangle_encoded src/core/Triangle.h:28-39, BVHNode_encoded
 *                               src/core/BVH.h:17-21)
 *   rt_update_materials      <- RefreshTriangleMaterial re-upload (src/core/Triangle.h:133-151),
 *                               with post-BVH triangle indices
 *   rt_set_env               <- InitHdrEnvMap() hdrMap/hdrCache RGB32F textures + hdrResolution
 *                               (src/core/Scene.h:164-184, main.cpp:138, :149-155)
 *   rt_resize                <- RenderBuffer::Init/Resize RGB32F ping-pong FBOs (src/core/Screen.h:110-122)
 *                               + this rank's pixel tiles (multi-GPU sharding, new)
 *   rt_reset / rt_set_loop_num <- camera.LoopNum = 0 (main.cpp:326, src/core/Camera.h:453)
 *   rt_render(_async)        <- per-frame loop body main.cpp:175-200: LoopIncrease, setCurrentBuffer,
 *                               the uniform list of main.cpp:181-199, DrawScreen
 *   rt_read_accum            <- reading the accumulation texture (Utility.h:19-30 SaveFrame reads it
 *                               after tone mapping; here the raw fp32 history)
 *   rt_accum_device / rt_assemble_frame <- (new) device-side tile gather for RCCL
 *   rt_trace_rays(_device)   <- hitBVH on caller rays (RT:338-392; any-hit: the isHit that RT:1389 consumes)
 *   rt_camera_rays / rt_first_hit(_device) / rt_pick <- the camera ray (RT:1520-1527) and its hitBVH
 *                               record (RT:1519), per pixel, without the bounce loop
 *
 * Conventions: every function returns RT_OK (0) or a negative rt_err_*; nothing aborts.
 * A context is bound to one HIP device and is not thread-safe (one host thread per ctx),
 * matching the single GL context of the reference (main.cpp:72).
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

/* ABI version of this header.
 * 4: rt_stats gained pass0_steps, pass1_steps, finish_steps and trace_busy_ms (round 4; round 3
 *    had added path_steps and p1_rays), and rt_stats_get_sized / rt_abi_version / RT_FLAG_SERIAL
 *    appeared.  path_steps changed meaning in 4: it counts wf_shade steps only; the finisher's shade
 *    steps, which it included before, are finish_steps (their sum is the old path_steps).
 * 5: rt_stats_get and rt_render write the ABI-3 struct only (the 104 bytes through p1_rays, what
 *    every binding of an ABI-3 header allocated; ABI 4 wrote past them), and the fields added in 4
 *    reach a caller only through rt_stats_get_sized with its own sizeof(rt_stats).  A binding
 *    written against the ABI-4 header (whose rt_stats_get filled the whole struct) must switch to
 *    rt_stats_get_sized(ctx, &s, sizeof s) to keep pass0_steps .. trace_busy_ms: the layout is
 *    unchanged, so that call with the ABI-4 size fills them (tests/c/abi_stats.c).
 *    RT_FLAG_SORTED_TRAVERSAL is accepted and has no effect (the octant-ordered traversal it
 *    switched off was removed).
 * 6: rt_gather moves the tiles with RCCL when the contexts sit on distinct devices;
 *    rt_gather_ex chooses the transport, rt_gather_last_transport reports it.  Nothing else changed.
 * 7: ray queries: rt_ray, rt_hit, RT_HIT_INVALID, RT_QUERY_*, rt_trace_rays, rt_trace_rays_device,
 *    rt_camera_rays, rt_first_hit, rt_first_hit_device, rt_pick, rt_get_triangle_material.  Additive:
 *    every ABI-6 entry point and struct is unchanged, and rendering computes what it did.
 *    The display denoiser (RT_HAS_DENOISE: rt_denoise_params, RT_DENOISE_*, rt_denoise_default_params,
 *    rt_denoise_async, rt_denoise) is an addition within ABI 7: nothing else changed, the version
 *    stays 7, and a binding finds it by symbol (a library built before it lacks rt_denoise).
 *    The temporal stage of the displayed frame (RT_HAS_TEMPORAL: rt_temporal_params, RT_TEMPORAL_*,
 *    rt_temporal_default_params, rt_temporal_async, rt_temporal, rt_temporal_history) is one more
 *    addition within ABI 7, found the same way, and so is its motion mode (RT_HAS_TEMPORAL_MOTION:
 *    rt_temporal_set_motion, rt_temporal_get_motion) and the variance mode of the two stages
 *    (RT_HAS_VARIANCE: rt_variance_params, rt_variance_default_params, rt_variance_set,
 *    rt_variance_get, rt_variance_frame).
 * A binding checks rt_abi_version() at load time. */
#define RT_ABI_VERSION 7
#define RT_HAS_DENOISE 1

#ifdef __cplusplus
extern "C" {
#endif

enum {
  RT_OK = 0,
  RT_ERR_ARG = -1,
  RT_ERR_HIP = -2,      /* a HIP runtime call failed; rt_last_error() has the text */
  RT_ERR_STATE = -3,    /* call order (e.g. render before set_scene/resize)          */
  RT_ERR_NOMEM = -4,
  RT_ERR_NODEVICE = -5, /* no HIP device / bad ordinal                               */
  RT_ERR_LIMIT = -6     /* scene exceeds a kernel limit (leaf > 16 tris, depth > 64) */
};

/* Frames per kernel batch; the path-state budget (184 B per pixel-frame; rt_set_max_paths or
 * RT_MAX_SLOTS, default 320 Mi slots = 64 GB) bounds it too: 161 frames at 1920x1080 with the
 * default budget; bench.py raises the budget to a whole 1024-frame step, which one GPU runs as two
 * launches of 512 frames (206 GB) and each of 8 tile-sharded GPUs as one launch (51 GB). */
enum { RT_MAX_FRAMES_PER_LAUNCH = 1024 };

/* Disney material (src/core/Material.h:25-46), 24 floats, same layout as rts_material. */
typedef struct rt_material {
  float emissive[3];
  float base_color[3];
  float subsurface, metallic, specular, specular_tint, roughness, anisotropic;
  float sheen, sheen_tint, clearcoat, clearcoat_gloss, ior, transmission;
  float medium_color[3];
  float medium_type, medium_density, medium_anisotropy;
} rt_material;

/* Scene in post-BVH triangle order (what buildBVHwithSAH leaves in `triangles`). */
typedef struct rt_scene_soa {
  int32_t n_triangles;
  const float *p1, *p2, *p3;      /* float[3*n_triangles], xyz interleaved */
  const float *n1, *n2, *n3;      /* vertex normals, float[3*n_triangles]  */
  const int32_t* material_id;     /* [n_triangles] index into materials    */
  const rt_material* materials;
  int32_t n_materials;
  int32_t n_nodes;                /* reference numbering: node 0 dummy, root 1, child 0 = none */
  const int32_t *node_left, *node_right, *node_n, *node_index;
  const float *node_aa, *node_bb; /* float[3*n_nodes] */
} rt_scene_soa;

/* Pixel tiling: the frame is cut into tile_w x tile_h tiles (multiples of 8), numbered
 * row-major from the bottom-left; this context renders tiles t with t % world == rank. */
typedef struct rt_tiling {
  int32_t tile_w, tile_h, rank, world;
} rt_tiling;

/* Per-call uniforms (main.cpp:181-199).  screen size comes from rt_resize. */
typedef struct rt_frame_params {
  float position[3], front[3], right[3], up[3], left_bottom_corner[3];
  float half_h, half_w;
  int32_t enable_mis, enable_env_map, enable_bsdf;
  float env_intensity, env_angle;
  int32_t max_bounce, max_iterations;
  int32_t flags;                  /* RT_FLAG_* */
} rt_frame_params;

enum {
  RT_FLAG_NO_CULL = 1,            /* disable closest-hit box culling (exhaustive RT:338 order)  */
  RT_FLAG_COUNT_VISITS = 2,       /* also count node/triangle visits (slower)                  */
  RT_FLAG_MEGAKERNEL = 4,         /* single persistent megakernel instead of the wavefront path */
  RT_FLAG_NO_FINISH = 8,          /* never end paths in the path-persistent finisher            */
  RT_FLAG_FINISH = 16,            /* use the finisher whatever the batch size (rt_set_finish)   */
  RT_FLAG_SERIAL = 32,            /* measurement: one frame group per batch (no two groups' kernels
                                     overlap), at most one group's path state of frames per batch */
  RT_FLAG_SORTED_TRAVERSAL = 64   /* ABI 4 (accepted, no effect since ABI 5): the trace always visits
                                     children by entry distance */
};

typedef struct rt_stats {
  uint64_t rays;            /* hitBVH invocations of the reference: camera + NEE shadow +
                               continuation, one camera ray per sample.  A group of several
                               frames answers a pixel's camera rays with one traversal (the
                               same ray in every frame), so rays / time is not a traversal
                               rate for the camera pass: compare builds on time per frame   */
  uint64_t samples;         /* pixel samples traced (frames x pixels, R12 copies excluded) */
  uint64_t internal_pops, leaf_pops, tri_tests;  /* only with RT_FLAG_COUNT_VISITS */
  uint64_t launches;        /* rt_render_async calls that launched work                  */
  double kernel_ms;         /* GPU time of those calls (HIP events on the ctx stream)     */
  uint64_t trace_launches;  /* traversal kernel launches (wavefront) / megakernel launches */
  double trace_ms;          /* summed duration of those launches (HIP events around each) */
  uint64_t trace_iters;     /* RT_FLAG_COUNT_VISITS: traversal loop iterations, all waves */
  uint64_t trace_iters_max; /* RT_FLAG_COUNT_VISITS: max loop iterations of one wave       */
  uint64_t path_steps;      /* wavefront path: wf_shade steps (one per path per bounce pass; since
                               ABI 4 without the finisher's, which are finish_steps)           */
  uint64_t p1_rays;         /* wavefront path: rays traced from pass 0's 16-B ray records  */
  /* ---- ABI 4: written only by rt_stats_get_sized */
  uint64_t pass0_steps;     /* of path_steps: pass 0 (implicit camera paths)                */
  uint64_t pass1_steps;     /* of path_steps: pass 1 (paths whose rays are 16-B records)    */
  uint64_t finish_steps;    /* shade steps run by the path-persistent finisher (wf_finish)  */
  double trace_busy_ms;     /* union of the traversal launches' intervals: the time during
                               which at least one of them ran (frame groups overlap, so
                               trace_ms can exceed it)                                       */
} rt_stats;

typedef struct rt_ctx rt_ctx;

int rt_create(int hip_device, rt_ctx** out);
int rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);
/* Device properties used for the launch geometry (CUs, clock). */
int rt_device_info(const rt_ctx* ctx, int32_t* n_cus, int32_t* blocks_per_cu, int32_t* lds_bytes_per_block);

/* A tree in which some child's box does not lie inside its parent's (aa >= and bb <= per axis; the root's
 * own box is not looked at) is traversed as the reference traverses it, on the binary tree with the
 * caller's boxes and without culling: the same results, more slowly. */
int rt_set_scene(rt_ctx* ctx, const rt_scene_soa* scene);
int rt_set_scene_encoded(rt_ctx* ctx, const float* tri_enc, int32_t n_triangles, const float* node_enc,
                         int32_t n_nodes);
int rt_update_materials(rt_ctx* ctx, int32_t first, int32_t count, const rt_material* material);
/* ---- Geometry update (RT_HAS_GEOMETRY_UPDATE, an addition within ABI 7: find it by symbol) -----------
 * New vertices for triangles of the scene set by rt_set_scene; the topology (triangle count and order,
 * leaves, both trees' structure, materials) stays.  Triangle t = first + i when tri_index is NULL, else
 * tri_index[i] (then first must be 0); p1..n3 hold 3 floats per updated triangle.  Everything derived
 * from the vertices is recomputed on the device (the geometric normals, the traversal records and their
 * edge filter, the shade's hit records) and every box of both trees is refitted as the exact min / max
 * union of what lies below it, so renders and queries return what a fresh rt_set_scene of the moved
 * triangles over the same tree returns, bit for bit.  The culling bound and the edge filter's margin only
 * grow under updates (more fallbacks to the reference's own test, never another answer); the tree is
 * not rebuilt for the new pose (rt_set_scene remains the way to a tree built for it).
 *   Like rt_update_materials, both calls wait for the render calls in flight, work on the context's
 * stream and return when the update is complete.  They leave LoopNum, the accumulation, rt_stats,
 * rt_order_work's order, the materials and the temporal history as they were (the caller resets what it
 * wants reset; with rt_temporal_set_motion the history follows the moved triangles) and forget the current denoise / temporal guides: RT_DENOISE_REUSE_GUIDES and
 * RT_TEMPORAL_REUSE_GUIDES return RT_ERR_STATE until a call packs fresh ones.  Every rank of a
 * multi-rank job makes the same call (each rank holds the whole scene).
 *   RT_ERR_STATE before rt_set_scene.  RT_ERR_ARG, with the scene untouched: count < 0, a null array with
 * count > 0, first != 0 with an index list, an index or range outside the triangle list, a duplicate
 * index (host form), a non-finite position or normal, |position| >= 2^30.  count == 0: RT_OK.
 *   rt_update_geometry_device takes device pointers (vertices produced on the GPU): it checks ranges and
 * values in a kernel that reads only its inputs, but cannot see duplicates: distinct indices are the
 * caller's contract there (a duplicate leaves one of the two triangles' data, never an invalid access).
 * The arrays must be complete on the context's stream, or the caller synchronises first.
 *   rt_scene_download copies one device array as it stands (bytes must be its size: 48 per triangle for
 * TRI / TRX / TRIN with at least one triangle's worth for TRX, 128 per triangle for HREC, 64 per binary
 * node, 128 per 4-wide node); rt_scene_bounds returns the scene's margins {cull_R, cull_K, cull_off,
 * tri_k1, tri_k0} and the number of triangles the edge filter leaves to the reference's test.  Both are
 * for tests and tooling.  Out of scope: topology changes, shrinking the margins, an asynchronous update
 * (the display history of a moved surface: rt_temporal_set_motion). */
#define RT_HAS_GEOMETRY_UPDATE 1
int rt_update_geometry(rt_ctx* ctx, const int32_t* tri_index, int32_t first, int32_t count, const float* p1,
                       const float* p2, const float* p3, const float* n1, const float* n2, const float* n3);
int rt_update_geometry_device(rt_ctx* ctx, const void* tri_index_dev, int32_t first, int32_t count, const void* p1_dev,
                              const void* p2_dev, const void* p3_dev, const void* n1_dev, const void* n2_dev,
                              const void* n3_dev);
enum { RT_SCENE_TRI = 0, RT_SCENE_TRX, RT_SCENE_TRIN, RT_SCENE_HREC, RT_SCENE_NODES, RT_SCENE_QNODES };
int rt_scene_download(rt_ctx* ctx, int32_t which, void* out, size_t bytes);
int rt_scene_array_bytes(rt_ctx* ctx, int32_t which, size_t* bytes);   /* the size rt_scene_download expects */
int rt_scene_bounds(rt_ctx* ctx, double out[5], int32_t* tri_flagged);
/* hdr_rgb / cache_rgb: w*h*3 floats, row 0 = first uploaded row (texture v = 0). */
int rt_set_env(rt_ctx* ctx, const float* hdr_rgb, const float* cache_rgb, int32_t w, int32_t h,
               int32_t hdr_resolution);
int rt_resize(rt_ctx* ctx, int32_t width, int32_t height, const rt_tiling* tiling /* NULL = whole frame */);
int rt_reset(rt_ctx* ctx);                       /* LoopNum = 0 (history kept, as the FBOs are) */
int rt_set_loop_num(rt_ctx* ctx, int32_t loop_num);
int rt_get_loop_num(const rt_ctx* ctx, int32_t* loop_num);
/* Clear this rank's accumulation to zero (fresh FBO contents). */
int rt_clear_accum(rt_ctx* ctx);
/* Tile ownership (SURVEY §8(e) "by a cost estimate from frame 1"): owner[t] = the rank that renders
 * global tile t (row-major from the bottom-left, n_tiles = tiles_x * tiles_y of the rt_resize
 * tiling).  rt_resize sets owner[t] = t % world; every rank of a job must set the same map.  Local
 * order = ascending tile id.  Re-sizes the accumulation (zeroed) and the pixel list, resets LoopNum. */
int rt_set_tile_owners(rt_ctx* ctx, const int32_t* owner, int32_t n_tiles);
int rt_get_tile_owners(const rt_ctx* ctx, int32_t* owner, int32_t n_tiles);
/* Cost probe for rt_set_tile_owners: renders n_frames and returns, per LOCAL tile of this ctx,
 * its rays' BVH node + triangle steps plus a per-ray share (deterministic integers).  LoopNum and
 * the accumulation are left as they were; the stats counters include the probe frames. */
int rt_tile_costs(rt_ctx* ctx, const rt_frame_params* params, const float* rand_origin, int32_t n_frames,
                  uint64_t* costs);
/* Longest-first work order (no GL counterpart: the rasteriser schedules fragments itself).  Traces
 * the camera pass of n_frames as a cost probe (the camera rays are the same in every frame, so the
 * costs do not depend on the frames; state left unchanged), then reorders this ctx's pixel
 * list by whole 64-pixel blocks (an 8x8 block stays one wave) in descending cost, so the blocks
 * whose rays cost most are queued first and a pass's tail is the cheap blocks; the costliest 5%
 * become a pixel group of their own in one-frame calls (their long bounce chains reach the
 * path-persistent finisher early, beside the rest's first passes).  Results are
 * unchanged (pixels are independent; the accumulation keeps its layout); rt_resize and
 * rt_set_tile_owners restore the natural order. */
int rt_order_work(rt_ctx* ctx, const rt_frame_params* params, const float* rand_origin, int32_t n_frames);
/* Path-state budget in pixel-frames (184 B each): frames in flight per launch = slots / pixels of
 * this rank, at most RT_MAX_FRAMES_PER_LAUNCH.  0 = RT_MAX_SLOTS from the environment or the
 * default 320 Mi slots.  A budget beyond free device memory runs fewer frames at a time.  No GL
 * counterpart: the fragment shader has one path per pixel in flight. */
int rt_set_max_paths(rt_ctx* ctx, uint64_t slots);
/* Path-persistent finisher (no GL counterpart: main.cpp:175-200 draws one frame per loop pass,
 * and each wavefront pass of such a small batch waits for its slowest ray).  A frame group of at
 * most max_slots path slots runs passes 0 .. pass-1 as wavefront passes and then ends every path
 * in one launch, one lane per path (results unchanged).  pass 0 disables it; defaults 2 and 8 Mi
 * slots (1080p: up to 8 frames per group).  RT_FLAG_NO_FINISH / RT_FLAG_FINISH override per call. */
int rt_set_finish(rt_ctx* ctx, int32_t pass, uint64_t max_slots);
/* Frames in flight across one-frame calls (the GL driver's own frame queue: main.cpp:175-251
 * issues a draw per loop pass and glfwSwapBuffers does not wait for it to finish).  With depth
 * 2 (the most; 1 = off), a one-frame rt_render_async call made while the previous call is
 * still running runs on the other of two internal streams with its own path state, so call k+1's
 * early passes overlap call k's latency-bound last bounces (a call with nothing in flight keeps
 * the lower-latency split into pixel groups).  Calls of one batch are pipelined the same way when
 * two sets of their path state fit the budget.  Only call k+1's blend waits for the ctx stream (call k's blend and
 * whatever the caller queued there since), and the ctx stream still joins every call at its end:
 * results and ordering are those of depth 1.  Default 1; synchronises the ctx. */
int rt_set_pipeline(rt_ctx* ctx, int32_t depth);

/* Enqueue n_frames progressive frames (one randOrigin per frame) on the ctx stream.  Each
 * frame first applies main.cpp:175 (LoopNum++ unless it reached max_iterations). */
int rt_render_async(rt_ctx* ctx, const rt_frame_params* params, const float* rand_origin, int32_t n_frames);
/* rt_render_async + synchronise + optional stats snapshot. */
int rt_render(rt_ctx* ctx, const rt_frame_params* params, const float* rand_origin, int32_t n_frames,
              rt_stats* stats /* ABI-3 fields only (see rt_stats_get) */);
int rt_synchronize(rt_ctx* ctx);
int rt_stats_get(rt_ctx* ctx, rt_stats* stats);  /* synchronises; writes the ABI-3 fields (104 bytes) */
/* The same, writing at most stats_bytes bytes (a caller's own, possibly older, sizeof(rt_stats)). */
int rt_stats_get_sized(rt_ctx* ctx, rt_stats* stats, size_t stats_bytes);
int rt_stats_reset(rt_ctx* ctx);
int rt_abi_version(void);                        /* RT_ABI_VERSION the library was built with */

/* The HIP stream (hipStream_t) the ctx launches on, for external events / collectives. */
int rt_get_stream(const rt_ctx* ctx, void** stream);
int rt_set_stream(rt_ctx* ctx, void* stream /* NULL = ctx-owned stream */);

enum { RT_LAYOUT_FRAME = 0, RT_LAYOUT_LOCAL_TILES = 1 };
/* FRAME: rgb_out = width*height*3 floats, row 0 = bottom row (GL framebuffer order); only this
 * rank's pixels are written.  LOCAL_TILES: local_tiles*tile_h*tile_w*3 floats. */
int rt_read_accum(rt_ctx* ctx, float* rgb_out, int32_t layout);
/* Upload a history (same layouts) — e.g. resume from a saved accumulation. */
int rt_write_accum(rt_ctx* ctx, const float* rgb_in, int32_t layout);
/* Device accumulation buffer: float4 (rgb + pad) per local tile pixel, padded to
 * max_local_tiles tiles so that every rank's buffer has the same size. */
int rt_accum_device(const rt_ctx* ctx, void** device_ptr, size_t* bytes, int32_t* local_tiles,
                    int32_t* max_local_tiles);
/* Device-to-device copy of the accumulation buffer (rt_accum_device bytes) into dst, enqueued
 * on the ctx stream (feeds the frame-end gather). */
int rt_copy_accum_device(rt_ctx* ctx, void* dst_device, size_t bytes);
/* Un-permute `world` gathered accumulation buffers (rank-major, each rt_accum_device bytes) on
 * this ctx's device into a width*height*3 float frame (device pointer). */
int rt_assemble_frame(rt_ctx* ctx, const void* gathered_device, int32_t world, void* frame_device);
/* Single-process form of the frame-end gather (SURVEY §8(b) rt_gather, §8(e)): ctxs[r] renders
 * rank r of a world of n (rt_resize tiling; one context per device, or several on one).  After
 * the work queued on each context, its accumulation tiles reach ctxs[0]'s device, are un-permuted
 * there (rt_assemble_frame) and read back: full_rgb = width*height*3 floats, row 0 = bottom
 * (RT_LAYOUT_FRAME).  Transport: with one device per context an RCCL gather over xGMI
 * (ncclCommInitAll over the contexts' devices, kept in ctxs[0]; ncclSend from every rank's stream,
 * ncclRecv on rank 0's, in one group), else peer copies (several contexts on one device).
 * Synchronous; errors land in rt_last_error(ctxs[0]).  One process per GPU uses
 * rt_copy_accum_device + a torch.distributed (RCCL) gather + rt_assemble_frame instead (bench.py). */
int rt_gather(rt_ctx* const* ctxs, int32_t n, float* full_rgb);
enum { RT_GATHER_AUTO = 0, RT_GATHER_RCCL = 1, RT_GATHER_PEER = 2 };
/* rt_gather with the transport chosen: RT_GATHER_AUTO (rt_gather's rule), RT_GATHER_RCCL
 * (RT_ERR_ARG unless every context has its own device), RT_GATHER_PEER (hipMemcpyPeerAsync). */
int rt_gather_ex(rt_ctx* const* ctxs, int32_t n, float* full_rgb, int32_t transport);
/* The transport ctx's last rt_gather / rt_gather_ex as ctxs[0] used (RT_GATHER_RCCL or
 * RT_GATHER_PEER; 0 before any). */
int rt_gather_last_transport(const rt_ctx* ctx);

/* Display / screenshot — replaces the tone-mapping pass
 * (src/shaders/fragment_shader_tone_mapping.glsl:66-93, main.cpp:215-227) or the screen blit
 * (fragment_shader_screen.glsl:6-9) plus the 8-bit read-back of SaveFrame (Utility.h:19-30).
 * flags: RT_DISPLAY_TONEMAP (enableToneMapping: simpleACES), RT_DISPLAY_GAMMA
 * (enableGammaCorrection: pow(c, 1/2.2), only with TONEMAP, as in main.cpp:216).
 * frame_device: an assembled width*height*3 float frame (rt_assemble_frame), or NULL for this
 * context's own accumulation (single rank only).  rgb8_host: width*height*3 bytes, row 0 = top
 * (PNG order).  Synchronous. */
enum { RT_DISPLAY_TONEMAP = 1, RT_DISPLAY_GAMMA = 2 };
int rt_tonemap(rt_ctx* ctx, const float* frame_device, int32_t flags, uint8_t* rgb8_host);
/* The same display pass without waiting for it (main.cpp:228-251: the blit and glfwSwapBuffers
 * queue the frame and the loop goes on): enqueues the pass and its read-back into internal pinned
 * slot `slot` (0..3) on the ctx stream, after the render calls queued before it, and returns.  A
 * render call queued afterwards blends only after this pass has read the accumulation.
 * rt_display_fetch waits for that slot's image and copies it out (width*height*3 bytes). */
int rt_tonemap_async(rt_ctx* ctx, const float* frame_device, int32_t flags, int32_t slot);
int rt_display_fetch(rt_ctx* ctx, int32_t slot, uint8_t* rgb8_host);

/* ---- Ray queries (ABI 7): the traversal of the render (hitBVH, RT:338-392) on rays of the caller's,
 * and the camera pass's hit record (RT:1519-1527) per pixel.  A query is queued on the ctx stream
 * after the render calls queued before it (pipelined ones included) and leaves LoopNum, the
 * accumulation, the path state, rt_order_work's order and every rt_stats field as they were.  Its
 * buffers are the context's own (allocated on first use, at most one chunk of 4 Mi rays, 432 MiB, freed by
 * rt_destroy); larger queries run as consecutive chunks.
 * Out of scope: a tmax for any-hit rays (the reference's shadow rays have none, RT:1389: use
 * RT_QUERY_CLOSEST and compare t), barycentrics / texture coordinates in rt_hit, and gathering
 * queries across ranks (each context answers for its own scene copy and its own pixels). */
typedef struct rt_ray {
  float origin[3];
  float dir[3];             /* any finite non-zero length (t is in units of it, RT:265) */
} rt_ray;                   /* 24 bytes */

/* The reference's HitRecord (RT:241-299, RT:330) of the closest hit, bit for bit.  A miss has
 * triangle = -1, t = -1.0f and every other byte 0; a ray that was not traced (below) has
 * triangle = RT_HIT_INVALID, t = -1.0f and every other byte 0. */
typedef struct rt_hit {
  float t;                  /* HitRecord.distance = t - 0.00001 (RT:284) */
  float point[3];           /* hitPoint = origin + dir * t (RT:270) */
  float normal[3];          /* the interpolated normal, negated when inside (RT:256-259, RT:290-297) */
  int32_t inside;           /* isInside: dot(N, dir) > 0 (RT:256) */
  int32_t triangle;         /* post-BVH triangle index (rt_update_materials' `first`) */
  int32_t material;         /* index into the context's material table (rt_get_triangle_material) */
  int32_t pad_[2];          /* 0 */
} rt_hit;                   /* 48 bytes */

enum { RT_HIT_INVALID = -2 };
enum { RT_QUERY_CLOSEST = 0, RT_QUERY_ANY = 1 };   /* kind */
enum { RT_QUERY_NO_CULL = 1 };                     /* flags: the exhaustive order of RT_FLAG_NO_CULL */

/* hitBVH (RT:338-392) for n rays in host memory; synchronous.  out: rt_hit[n] (RT_QUERY_CLOSEST) or
 * int32_t[n] (RT_QUERY_ANY: 1 occluded, 0 not -- the isHit of the reference's shadow ray, RT:1389;
 * which of several hits ends the ray is not defined, only that there is one).  A ray with a
 * non-finite component or an all-zero direction is not traced: RT_HIT_INVALID (in `triangle`, or
 * as the any-hit value); the call still returns RT_OK.  n == 0: RT_OK.  RT_ERR_STATE before
 * rt_set_scene; RT_ERR_ARG for a bad kind, unknown flags or null pointers. */
int rt_trace_rays(rt_ctx* ctx, const rt_ray* rays, int64_t n, int32_t kind, int32_t flags, void* out);
/* The same (hitBVH, RT:338-392) on device pointers: enqueued on the ctx stream, results valid after rt_synchronize or in
 * stream order.  origin_bound >= |every origin component| (finite, >= 0): the culling margin is derived
 * for origins within it (rt_trace_rays scans for it), and a ray outside it is not traced
 * (RT_HIT_INVALID).  rays_dev and out_dev need 4-byte alignment (out_dev 16 for rt_hit). */
int rt_trace_rays_device(rt_ctx* ctx, const void* rays_dev, int64_t n, int32_t kind, int32_t flags,
                         float origin_bound, void* out_dev);
/* The camera rays of this rank's pixels (RT:1520-1527, TexCoords of vertex_shader.glsl) as the render
 * computes them: origin = position, dir normalised.  Layouts as rt_read_accum (rt_ray instead of 3
 * floats; FRAME writes only this rank's pixels).  Only the camera fields of params are read. */
int rt_camera_rays(rt_ctx* ctx, const rt_frame_params* params, rt_ray* rays, int32_t layout);
/* First-hit frame: hitBVH's record (RT:1519) of every camera ray of this rank -- per-pixel depth,
 * normal, triangle and material for denoisers, outlines and debug views.  Same layouts; synchronous. */
int rt_first_hit(rt_ctx* ctx, const rt_frame_params* params, rt_hit* hits, int32_t layout);
/* The same (RT:1519) into device memory, RT_LAYOUT_LOCAL_TILES (rt_hit[local_tiles * tile_h * tile_w]; tile
 * pixels outside the frame are not written), enqueued on the ctx stream: the form a display or
 * denoise pass consumes. */
int rt_first_hit_device(rt_ctx* ctx, const rt_frame_params* params, void* hits_dev);
/* One pixel's camera ray (RT:1520-1527) and its hit: px, py in the accumulation's convention (row 0
 * = bottom).  RT_ERR_ARG for a pixel outside the frame or not owned by this rank.  Synchronous. */
int rt_pick(rt_ctx* ctx, const rt_frame_params* params, int32_t px, int32_t py, rt_hit* hit);
/* The material of a (post-BVH) triangle from the host copies (no device call): the 24 floats as
 * rt_set_scene / rt_update_materials received them (the device entry keeps them verbatim and adds
 * the derived ax, ay, RT:205-207, and the integer medium type), and its material-table index.
 * Triangles with equal materials share an index; rt_update_materials moves its range to the index
 * of the new material (a new one unless the table already holds it), so what a pick returns can
 * be edited and fed back to rt_update_materials(triangle, 1, ...).  Either output may be NULL. */
int rt_get_triangle_material(rt_ctx* ctx, int32_t triangle, rt_material* out, int32_t* material_id);

/* ---- Display denoiser (RT_HAS_DENOISE, within ABI 7; no counterpart in the reference, whose display
 * pass main.cpp:202-228 shows the raw accumulation): a guided edge-avoiding a-trous wavelet filter
 * (Dammertz et al. 2010) over the accumulation and the first-hit records, for a readable image after
 * one or a few samples per pixel.  It is a post-process between rendering and rt_tonemap(_async): it
 * leaves LoopNum, the accumulation, the path state, rt_order_work's order and every rt_stats field
 * as they were.  All arithmetic is fp32 in a fixed order (tests/denoise_model.py is
 * the same filter in numpy, and the two agree bit for bit).  Iteration i = 0 .. iterations-1 runs a
 * 5x5 B3-spline footprint with taps s = 2^i apart; a tap counts when it lies in the frame, hit
 * something, has the centre's material and a finite colour, weighted by
 * exp(-(|dN|^2 / sigma_normal^2 + (N . dP / t)^2 / sigma_plane^2 + |dG|^2 * 4^i / sigma_color^2)), G the
 * colour compressed by 1 / (1 + luminance).  Pixels whose camera ray misses pass through bit for
 * bit (they show the environment, which carries no noise); a non-finite pixel is never a source and
 * is filled from its neighbours by the geometric weights alone.
 * Out of scope: multi-rank contexts (a rank has guides for its own pixels only: RT_ERR_STATE when
 * world != 1), albedo demodulation (temporal reprojection: rt_temporal*, variance guidance:
 * rt_variance_*, both below). */
typedef struct rt_denoise_params {
  int32_t iterations;               /* 1..5 */
  float sigma_color, sigma_normal, sigma_plane;   /* each finite and > 0 */
  int32_t flags;                    /* RT_DENOISE_* */
} rt_denoise_params;                /* 20 bytes */
/* REUSE_GUIDES: use the guides (normal, position, depth, material per pixel) of this context's
 * previous denoise or temporal call; the caller asserts that the camera, scene, materials and size are
 * unchanged since.  fp and hits_dev are ignored. */
enum { RT_DENOISE_REUSE_GUIDES = 1 };
/* The defaults: 5 iterations, sigma_color 1.0, sigma_normal 0.3, sigma_plane 0.01, flags 0. */
int rt_denoise_default_params(rt_denoise_params* dp);
/* Enqueue the filter on the ctx stream, after the render calls queued before it (pipelined ones
 * included); a render call queued afterwards blends only after the filter has read the
 * accumulation.  frame_in_device: width*height*3 floats in RT_LAYOUT_FRAME order on the device, or
 * NULL for this context's accumulation.  hits_dev: the first-hit frame as rt_first_hit_device
 * writes it (the camera pass's hit record, RT:1519), or NULL: the library traces it for fp (only its
 * camera fields and RT_FLAG_NO_CULL are read) into a buffer of its own.  *frame_out_device
 * receives the context-owned output frame (width*height*3 floats, RT_LAYOUT_FRAME order), valid in
 * stream order until the next denoise call, rt_resize or rt_destroy; it can be passed to
 * rt_tonemap(_async) as frame_device.  The buffers (two colour frames, two guide frames, the rt_hit
 * frame, the output: 76 B per pixel + 48 B per tile pixel) are the context's own, allocated on first
 * use, dropped and re-sized by rt_resize, freed by rt_destroy.
 * RT_ERR_ARG: a null pointer (fp may be NULL when it is ignored), iterations outside 1..5, a sigma
 * that is not finite and > 0, unknown flags.  RT_ERR_STATE: before rt_set_scene or rt_resize; a
 * context with world != 1; RT_DENOISE_REUSE_GUIDES when no guides exist for the current size. */
int rt_denoise_async(rt_ctx* ctx, const rt_frame_params* fp, const rt_denoise_params* dp,
                     const float* frame_in_device, const void* hits_dev, float** frame_out_device);
/* The same on this context's accumulation with the library's own first-hit trace (RT:1519),
 * synchronous: rgb_out_host = width*height*3 floats, RT_LAYOUT_FRAME order (row 0 = bottom). */
int rt_denoise(rt_ctx* ctx, const rt_frame_params* fp, const rt_denoise_params* dp, float* rgb_out_host);

/* ---- Temporal accumulation of the displayed frame (RT_HAS_TEMPORAL, within ABI 7; no counterpart in
 * the reference, where LoopNum = 0 starts the image again from nothing, main.cpp:326).  The context
 * keeps a display history per pixel: colour, history length n, the two guide texels of the denoiser
 * ({N, material or -1 for a camera miss}, {P, 1/t}) and the camera they were seen from.  A call
 * reprojects that history into the current view through the current first-hit frame, rejects what
 * is not the same surface, and blends the input frame into it, weighted by sample counts.  Like the
 * denoiser it is a post-process of the displayed frame, between rendering and rt_denoise_async or
 * rt_tonemap(_async): LoopNum, the accumulation, the path state, rt_order_work's order and every
 * rt_stats field stay as they were.  All arithmetic is fp32 in a fixed order (DESIGN.md §4;
 * tests/temporal_model.py is the same stage in numpy, and the two agree bit for bit).
 * Per pixel, RT_LAYOUT_FRAME order, with input colour c, guides {N, M}, {P, 1/t}, S = samples:
 *   miss (M == -1)  out = c, n_out = 0 (the environment carries no noise); never a history source.
 *   hit             d = P - position', require d.front' > 0; k = (lbc'.front') / (d.front'),
 *                   a = k (d.right') - lbc'.right', b = k (d.up') - lbc'.up',
 *                   x = a / (2 half_w') * W - 0.5, y = b / (2 half_h') * H - 0.5 (primed: the history's
 *                   rt_frame_params).  This inverts the camera ray of RT:1520-1527 under the
 *                   assumption that front', right' and up' are unit length and orthogonal, as
 *                   Camera.h:160-174 produces them.  The four bilinear taps (floor x + i, floor y + j)
 *                   count when they lie in the frame, a history exists for this size, their n > 0,
 *                   their colour is finite, their material is M, |N - Nq|^2 <= sigma_normal^2 and
 *                   |N . (Pq - P)| / t <= sigma_plane.  With sw the counting taps' weight:
 *                   h = sum(w cq) / sw, n_h = sum(w nq) / sw when sw > 0, else no history.
 *   blend           history and finite c: n_out = min(n_h + S, max_history), alpha = min(S / n_out, 1),
 *                   out = h + alpha (c - h).  No history: out = c, n_out = min(S, max_history).
 *                   Non-finite c: out = h, n_out = n_h with history, else out = c, n_out = 0 (never a
 *                   source; the denoiser fills it).
 * RT_TEMPORAL_ADVANCE: the previous call's output (colours, lengths, guides, camera) becomes the
 * history before this call runs (buffers change roles, nothing is copied).  Without it the history
 * stays and this call's output replaces the previous call's as the candidate, so a still camera
 * does not count the accumulation's samples twice: while LoopNum grows the display is
 * (n H + k acc_k) / (n + k) against a frozen H.  Pass ADVANCE on the first display after the
 * accumulation restarted.  RT_TEMPORAL_RESET drops history and candidate before the call;
 * rt_resize and rt_set_scene drop them too.
 * A surface rt_update_geometry moved keeps its history only in the motion mode (below); without it
 * the caller resets (RT_TEMPORAL_RESET).  Out of scope: view-dependent (specular) reprojection,
 * multi-rank contexts (RT_ERR_STATE when world != 1); variance estimation: rt_variance_*, below. */
#define RT_HAS_TEMPORAL 1
typedef struct rt_temporal_params {
  int32_t samples;                  /* >= 1: samples per pixel in the input frame (LoopNum) */
  int32_t max_history;              /* >= 1: cap on a pixel's history length */
  float sigma_normal, sigma_plane;  /* each finite and > 0 */
  int32_t flags;                    /* RT_TEMPORAL_* */
} rt_temporal_params;               /* 20 bytes */
/* REUSE_GUIDES: the current guides are those of this context's previous denoise or temporal call (the
 * same assertion as RT_DENOISE_REUSE_GUIDES, which in turn accepts a temporal call's guides: the
 * chain temporal -> denoise -> tonemap traces the first-hit frame once per view); hits_dev is
 * ignored. */
enum { RT_TEMPORAL_ADVANCE = 1, RT_TEMPORAL_REUSE_GUIDES = 2, RT_TEMPORAL_RESET = 4 };
/* The defaults: samples 1, max_history 32, sigma_normal 0.3, sigma_plane 0.01, flags 0. */
int rt_temporal_default_params(rt_temporal_params* tp);
/* Enqueue the stage on the ctx stream, after the render calls queued before it (pipelined ones
 * included); a render call queued afterwards blends only after the stage has read the
 * accumulation.  frame_in_device, hits_dev: as for rt_denoise_async (NULL: this context's
 * accumulation; NULL: the library traces the first-hit frame for fp).  fp is never ignored: its
 * camera is kept with the output.  *frame_out_device receives the context-owned output frame
 * (width*height*3 floats, RT_LAYOUT_FRAME order), valid in stream order until the next temporal
 * call, rt_resize or rt_destroy; it can be passed to rt_denoise_async as frame_in_device or to
 * rt_tonemap(_async) as frame_device.  The first temporal call allocates the denoiser's buffers
 * (above) and, beside them, two {r, g, b, n} frames, two more guide pairs and the output: 108 B per
 * pixel; dropped and re-sized by rt_resize, freed by rt_destroy.
 * RT_ERR_ARG: a null pointer, samples < 1, max_history < 1, a sigma that is not finite and > 0,
 * unknown flags, a non-finite camera.  RT_ERR_STATE: before rt_set_scene or rt_resize; a context with
 * world != 1; RT_TEMPORAL_REUSE_GUIDES when no guides exist for the current size. */
int rt_temporal_async(rt_ctx* ctx, const rt_frame_params* fp, const rt_temporal_params* tp,
                      const float* frame_in_device, const void* hits_dev, float** frame_out_device);
/* The same on this context's accumulation (first-hit frame: the library's own trace, or the
 * previous call's guides with REUSE_GUIDES), synchronous: rgb_out_host = width*height*3 floats. */
int rt_temporal(rt_ctx* ctx, const rt_frame_params* fp, const rt_temporal_params* tp, float* rgb_out_host);
/* The history lengths n_out of the last temporal call's output: width*height floats,
 * RT_LAYOUT_FRAME order; synchronous.  RT_ERR_STATE when there is none (no call yet, or dropped). */
int rt_temporal_history(rt_ctx* ctx, float* n_out_host);

/* ---- Motion mode of the temporal stage (RT_HAS_TEMPORAL_MOTION, an addition within ABI 7: find it
 * by symbol).  Off (the default) the library does what is written above and nothing else: no
 * allocation, launch or kernel argument differs.  On, every output of the stage remembers the pose
 * of the scene it was made from (a copy of the vertex records RT_SCENE_TRI and RT_SCENE_TRIN, 96 B per
 * triangle and history frame, copied device to device once per geometry generation and frame: a
 * successful rt_update_geometry(_device) with count > 0 starts a generation), and a fresh pack of the
 * guides (by rt_temporal_async or rt_denoise_async) also stores each pixel's first-hit triangle, 4 B per
 * pixel and guide pair.  A hit pixel whose triangle T lies in [0, n_triangles) and has any of its 18
 * floats (three positions, three vertex normals; bitwise) differing between the history's pose
 * (q1..q3, m1..m3) and the current one (p1..p3, n1..n3) is reprojected through that triangle; every
 * other pixel runs the arithmetic above bit for bit.  fp32, one correctly rounded operation per
 * step, dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, vector lines per component:
 *   e1 = p2 - p1; e2 = p3 - p1; v = P - p1
 *   d11 = dot(e1,e1); d12 = dot(e1,e2); d22 = dot(e2,e2); v1 = dot(v,e1); v2 = dot(v,e2)
 *   den = d11 d22 - d12 d12                                              require den > 0
 *   b2 = (d22 v1 - d12 v2) / den; b3 = (d11 v2 - d12 v1) / den; b1 = (1 - b2) - b3   require all finite
 *   Pq = q1 + (b2 (q2 - q1) + b3 (q3 - q1))
 *   Nc = (b1 n1 + b2 n2) + b3 n3; flip = dot(N, Nc) < 0
 *   Nm = (b1 m1 + b2 m2) + b3 m3; l = sqrt(dot(Nm,Nm))                   require l > 0 and finite
 *   Nq = Nm / l, negated when flip
 * and the stage runs with Pq in place of P in the projection and the tap tests, Nq in place of N:
 * |Nq - N[q]|^2 <= sigma_normal^2, |dot(Nq, P[q] - Pq)| / t <= sigma_plane.  A failed `require`
 * means no history for that pixel.  (The barycentrics are the 3D ones: the reference's xy-projected
 * ones, RT:282-295, degenerate for a triangle edge-on to the xy plane.)  tests/temporal_motion_model.py
 * is the same in numpy.  Triangle indices in a caller's hits_dev outside the list take the static path.
 *   rt_temporal_set_motion waits for the work in flight (as rt_set_pipeline), drops history,
 * candidate and poses (as RT_TEMPORAL_RESET) and frees or forgets the mode's buffers; any time after
 * rt_create; RT_ERR_ARG unless on is 0 or 1.  The setting survives rt_set_scene and rt_resize, which
 * drop the poses with the history.  RT_TEMPORAL_REUSE_GUIDES in motion mode reads the stored triangle
 * frame and gives what fresh guides give; RT_ERR_STATE when the current guides were packed while the
 * mode was off.  Out of scope: topology changes, motion vectors as an output. */
#define RT_HAS_TEMPORAL_MOTION 1
int rt_temporal_set_motion(rt_ctx* ctx, int32_t on);   /* 0 / 1; default 0 */
int rt_temporal_get_motion(const rt_ctx* ctx, int32_t* on);

/* ---- Variance mode of the display chain (RT_HAS_VARIANCE, an addition within ABI 7: find it by
 * symbol).  Off (the default) the temporal stage and the denoiser do what is written above and
 * nothing else: no allocation, launch, kernel argument or output bit differs.  On, the temporal
 * stage estimates the per-sample variance of every pixel's luminance l = (0.2126 r + 0.7152 g) +
 * 0.0722 b from the inputs it sees, and the denoiser replaces its fixed colour term by a luminance
 * term scaled by the variance of what it filters (Schied et al. 2017, SVGF), so that a converged
 * view is no longer blurred.  fp32, one correctly rounded operation per step, in the order written;
 * tests/variance_model.py is the same in numpy and the kernels agree with it bit for bit.
 *   Temporal stage.  Beside each {r, g, b, n} texel of history and candidate lies one state texel
 * {l_prev, S_prev, v, m} (16 B): luminance and sample count of the last input seen for the view, the
 * running mean v of m variance estimates.  Per hit pixel with input luminance l_c, S = samples:
 *   a call without RT_TEMPORAL_ADVANCE / RESET after an earlier call (the same view, accumulated
 *   further) reads its own texel of the candidate before overwriting it; with a finite input and
 *   S > S_prev > 0:  dS = S - S_prev; s = (S l_c - S_prev l_prev) / dS; d = s - l_prev;
 *                    e = (d d) ((dS S_prev) / S)            (Welford's chunk-merge term)
 *   any other call takes v0 = sum(w vq) / sw, m0 = sum(w mq) / sw over the colour's counting taps
 *   (0, 0 without history); with history and a finite input, l_h the luminance of the history h:
 *                    d = l_c - l_h; e = (d d) / (1 / S + 1 / n_h)
 *   Either e is one squared difference of two independent means, unbiased for the per-sample
 *   variance.  With a finite e:  v = v0 + (e - v0) / (m0 + 1); m = min(m0 + 1, max_estimates); else
 *   v, m = v0, m0.  A finite input stores l_prev = l_c, S_prev = S; a non-finite one keeps both
 *   (0, 0 in the second case); a miss stores zeros.  The variance of the displayed luminance:
 *   var = v / max(n_out, S) when m > 0, else -1 (unknown).
 *   Denoiser.  The input's variance is the temporal stage's when frame_in_device is the pointer the
 * last rt_temporal_async returned, else unknown everywhere.  A hit pixel with var < 0 takes the
 * spatial estimate: over the 7 x 7 neighbours q (dy outer, dx inner, the centre included) with the
 * centre's material, a finite colour, |N - Nq|^2 <= sigma_normal^2 and |N . (Pq - P)| / t <=
 * sigma_plane, with d = l_q - (l_p, or 0 when p is not finite): s1 = sum d, s2 = sum d d, and
 * var = max((s2 - (s1 s1) / cnt) / (cnt - 1), 0) when cnt >= 2; a pixel that stays unknown keeps the
 * fixed sigma_color term.  Iteration i, for a pixel with var_p >= 0: g = sum(w3 var_q) / sum(w3) over
 * the 3 x 3 neighbours with p's material and var_q >= 0, w3 = {1/4, 1/2, 1/4}^2; kl = 1 / (sigma_lum
 * sqrt(g) + 1e-8); the colour term of a tap's exponent becomes |l_p - l_q| kl (0 for a non-finite p),
 * geometric terms, B3 weights, tap order and tap tests unchanged.  The iteration's output carries
 * var' = sum(w^2 var_q over counting taps with var_q >= 0) / (sum w)^2 where var_p >= 0 and a tap
 * counted, else var_p.  Miss pass-through, non-finite filling and the bit-identical return of
 * per-material constant frames hold as without the mode.
 *   rt_variance_set waits for the work in flight, drops history and candidate (as
 * RT_TEMPORAL_RESET) and, when on == 0, frees the mode's buffers (44 B per pixel: two state frames,
 * three variance frames; allocated by the first temporal or denoise call in the mode, re-sized by
 * rt_resize).  The setting survives rt_set_scene and rt_resize.  It composes with the motion mode: v
 * and m ride the colour's taps, moved triangles included.  RT_ERR_ARG: a null pointer, on outside
 * 0 / 1, sigma_lum not finite and > 0, max_estimates < 1, flags != 0.
 * Out of scope: a second-moment accumulation inside the renderer, specular reprojection, multi-rank
 * contexts. */
#define RT_HAS_VARIANCE 1
typedef struct rt_variance_params {
  int32_t on;                       /* 0 / 1; default 0 */
  float sigma_lum;                  /* finite and > 0: luminance differences in standard deviations */
  int32_t max_estimates;            /* >= 1: cap of m (from there on v is an exponential average) */
  int32_t flags;                    /* 0 */
} rt_variance_params;               /* 16 bytes */
/* The defaults: on 0, sigma_lum 1.5, max_estimates 64, flags 0. */
int rt_variance_default_params(rt_variance_params* vp);
int rt_variance_set(rt_ctx* ctx, const rt_variance_params* vp);
int rt_variance_get(const rt_ctx* ctx, rt_variance_params* vp);
/* The variance of the displayed luminance of the last temporal or denoise call's output in the mode:
 * width*height floats, RT_LAYOUT_FRAME order, -1 where it is unknown; synchronous.  RT_ERR_STATE when
 * there is none (mode off, no call yet, or dropped by rt_resize / rt_variance_set). */
int rt_variance_frame(rt_ctx* ctx, float* var_out_host);

#ifdef __cplusplus
}
#endif
#endif
