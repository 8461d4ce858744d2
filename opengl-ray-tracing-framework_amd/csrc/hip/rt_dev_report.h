// rt_dev_report.h — the RT_DEBUG_PASSES reports of the development library (-DRT_DEV): included
// by rt_render.hip only under RT_DEV, inside its anonymous namespace, after rt_ctx, knob(), HIPCHK,
// take_event and launch_finish.  The per-pass reports synchronise the group's stream after the
// launch they describe: measurement aids (tools/pass_counts.py, tools/gpu_run.sh read their text),
// never part of a timed render.

// RT_DEBUG_PASSES: per-pass report of the COUNT build (syncs after every pass)
inline bool dev_passes() {
  static const bool on = knob("RT_DEBUG_PASSES") != nullptr;
  return on;
}
// the kernels' per-wave records (KParams::wave_log): 8 words per wave of the trace grid (the
// trace's records use the first half)
inline size_t dev_wave_words(const rt_ctx* c) { return (size_t)c->n_cus * std::max(c->trace_bpc, c->trace_bpc0) * 4 * 8; }
int dev_wave_log(rt_ctx* c, unsigned long long*& log) {
  static unsigned long long* d_wave_log = nullptr;  // never freed
  if (dev_passes() && !d_wave_log) HIPCHK(c, hipMalloc(&d_wave_log, dev_wave_words(c) * sizeof(unsigned long long)));
  log = dev_passes() ? d_wave_log : nullptr;
  return RT_OK;
}

// development aid: what the planner (render_plan.h) was given for the batch and what it decided for
// group g, one line before the group's passes: the inputs, the batch, the group and its steps by
// name, in kInNames / kGroupNames / kStepNames order (a step's values joined by ',', steps by ';').
// tests/test_gpu_render_plan.py feeds the inputs back to rts_render_plan and compares.
void dev_plan_report(const rpl::In& in, const rpl::Batch& B, int g) {
  int64_t v[rpl::kInCount];
  static_assert(sizeof(v) == sizeof(in), "In is flat");
  memcpy(v, &in, sizeof(v));
  fprintf(stderr, "[rt] plan group %d:", g);
  for (int k = 0; k < rpl::kInCount; k++) fprintf(stderr, " %s=%lld", rpl::kInNames[k], (long long)v[k]);
  fprintf(stderr, " nf=%d G=%d pix_split=%d", B.nf, B.G, B.pix_split ? 1 : 0);
  int64_t gv[rpl::kGroupCount], sv[rpl::kStepCount];
  rpl::flatten(B.g[g], gv);
  for (int k = 0; k < rpl::kGroupCount; k++) fprintf(stderr, " %s=%lld", rpl::kGroupNames[k], (long long)gv[k]);
  fprintf(stderr, " steps=");
  for (int pass = 0; pass < B.g[g].n_steps; pass++) {
    rpl::flatten(rpl::step(in.f, in.s, in.c, B.g[g], pass), sv);
    for (int k = 0; k < rpl::kStepCount; k++) fprintf(stderr, "%s%lld", k ? "," : pass ? ";" : "", (long long)sv[k]);
  }
  fprintf(stderr, "\n");
}

// development aid: the finisher's launch of group g, then its waves (syncs!)
int dev_finish_report(rt_ctx* c, bool bsdf, dim3 grid, hipStream_t st, const rtd::WFParams& WP, int g, int pass) {
  std::vector<unsigned long long> wave_log(dev_wave_words(c));
  unsigned long long* const d_wave_log = WP.K.wave_log;
  HIPCHK(c, hipMemsetAsync(d_wave_log, 0, wave_log.size() * 8, st));
  hipEvent_t ft0 = take_event(c), ft1 = take_event(c);
  HIPCHK(c, hipEventRecord(ft0, st));
  launch_finish(c, bsdf, grid, st, WP);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(ft1, st));
  HIPCHK(c, hipStreamSynchronize(st));
  float ms = 0.0f;
  HIPCHK(c, hipEventElapsedTime(&ms, ft0, ft1));
  c->event_pool.push_back(ft0);
  c->event_pool.push_back(ft1);
  HIPCHK(c, hipMemcpy(wave_log.data(), d_wave_log, wave_log.size() * 8, hipMemcpyDeviceToHost));
  struct FW { double t0, t1, sh_us; unsigned long long it, sh, paths; double at[3]; unsigned long long it_at[3]; };
  std::vector<FW> fw;
  double tmin = 1e300;
  for (size_t w = 0; w < wave_log.size() / 8; w++) {
    const unsigned long long* e = &wave_log[8 * w];
    if (!e[1]) continue;
    FW f{e[0] / 100.0, e[1] / 100.0, e[3] / 100.0, e[2] & 0xfffffull, (e[2] >> 20) & 0xfffffull, e[2] >> 40, {}, {}};
    for (int q = 0; q < 3; q++) {
      f.at[q] = e[4 + q] ? (double)(e[4 + q] & 0xffffffffull) / 100.0 : -1.0;
      f.it_at[q] = e[4 + q] >> 32;
    }
    fw.push_back(f);
    tmin = std::min(tmin, e[0] / 100.0);
  }
  std::sort(fw.begin(), fw.end(), [](const FW& a, const FW& b) { return a.t1 > b.t1; });
  unsigned long long paths = 0;
  double life = 0.0, tail16 = 0.0, tail4 = 0.0;
  for (const FW& f : fw) {
    paths += f.paths;
    life += f.t1 - f.t0;
    if (f.at[0] >= 0) tail16 += f.t1 - f.t0 - f.at[0];
    if (f.at[1] >= 0) tail4 += f.t1 - f.t0 - f.at[1];
  }
  fprintf(stderr, "[rt] finisher wave time with <= 16 / <= 4 lanes holding a path (list drained): %.3f / %.3f of %.0f "
          "wave-us\n", tail16 / std::max(1.0, life), tail4 / std::max(1.0, life), life);
  fprintf(stderr, "[rt] group %d finisher from pass %d: %.3f ms, %zu waves, %llu paths; wave ends (us after the first "
          "start) 50%% %.1f 90%% %.1f 99%% %.1f 100%% %.1f\n", g, pass, ms, fw.size(), paths,
          fw.empty() ? 0.0 : fw[fw.size() / 2].t1 - tmin, fw.empty() ? 0.0 : fw[fw.size() / 10].t1 - tmin,
          fw.empty() ? 0.0 : fw[fw.size() / 100].t1 - tmin, fw.empty() ? 0.0 : fw[0].t1 - tmin);
  for (size_t k = 0; k < std::min<size_t>(6, fw.size()); k++) {
    const FW& f = fw[k];
    fprintf(stderr, "[rt]   wave: start %.1f end %.1f us, %llu paths, %llu trace iterations (%.2f us each outside "
            "shade), %llu shade steps %.1f us (%.2f us each); <=16 / 4 / 1 busy lanes from %.0f / %.0f / %.0f us "
            "(iteration %llu / %llu / %llu)\n", f.t0 - tmin, f.t1 - tmin, f.paths, f.it,
            (f.t1 - f.t0 - f.sh_us) / (double)std::max(1ull, f.it), f.sh, f.sh_us, f.sh_us / (double)std::max(1ull, f.sh),
            f.at[0], f.at[1], f.at[2], f.it_at[0], f.it_at[1], f.it_at[2]);
  }
  return RT_OK;
}

// development aid: per-pass rays / visits / duration of group g's trace launch (t0, t1) (syncs!)
int dev_pass_report(rt_ctx* c, hipStream_t st, const rtd::WFParams& WP, int g, int pass, hipEvent_t t0, hipEvent_t t1) {
  unsigned long long h[16];
  unsigned int q[8];
  HIPCHK(c, hipStreamSynchronize(st));
  float ms = 0.0f;
  HIPCHK(c, hipEventElapsedTime(&ms, t0, t1));
  HIPCHK(c, hipMemcpy(h, c->d_stats, sizeof(h), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(q, WP.S.cnt, sizeof(q), hipMemcpyDeviceToHost));
  const unsigned int n_cont = q[rtd::cq(pass & 1)], n_shadow = q[rtd::cqs(pass & 1)], n_kept = q[rtd::ca(pass & 1)];
  q[0] = q[rtd::cq(pass & 1)] + (WP.split ? q[rtd::cqs(pass & 1)] : 0u);  // (split queues: both kinds)
  const unsigned int traced = WP.cam_n ? (WP.cam_shared ? WP.K.n_work : WP.cam_n) : q[0];  // traversals of the launch
  fprintf(stderr, "[rt] group %d pass %d: %u rays %.3f ms  cum internal %llu leaf %llu tri %llu iters %llu "
          "wave-iters max %llu ray-steps max %llu\n", g, pass, traced, ms, h[2], h[3], h[4], h[5], h[6], h[7]);
  if (!WP.cam_n) {
    // the pass's lists as the shade before it counted them (with WFParams::p1_lean pass 1 has no
    // continuation queue or active list: its continuation trace and shade walk the hit-pixel list,
    // `items` entries, and these are counts alone)
    unsigned int hits = 0;
    HIPCHK(c, hipMemcpy(&hits, WP.S.cnt + rtd::kCntHit, sizeof(hits), hipMemcpyDeviceToHost));
    const bool lean1 = WP.p1_lean && pass == 1;
    fprintf(stderr, "[rt]   lists: continuations %u shadow rays %u kept paths %u  p1_lean %d items %u\n",
            WP.split ? n_cont : 0u, WP.split ? n_shadow : 0u, n_kept, lean1 ? 1 : 0,
            lean1 ? hits * (unsigned)WP.n_frames : n_kept);
  }
  unsigned long long hq[6];
  HIPCHK(c, hipMemcpy(hq, c->d_stats + 22, sizeof(hq), hipMemcpyDeviceToHost));
  fprintf(stderr, "[rt]   4-wide node visits with BFS index < 1 / 5 / 21 / 64 / 85 / 341: %llu %llu %llu %llu %llu %llu\n",
          hq[0], hq[1], hq[2], hq[3], hq[4], hq[5]);
  HIPCHK(c, hipMemset(c->d_stats + 22, 0, sizeof(hq)));
  fprintf(stderr, "[rt]   lane utilisation: node phase %.3f (%llu iters)  tri phase %.3f (%llu iters)  busy at "
          "refill %.3f (%llu outer)\n", h[9] / (64.0 * (double)(h[8] + !h[8])), h[8],
          h[11] / (64.0 * (double)(h[10] + !h[10])), h[10], h[13] / (64.0 * (double)(h[12] + !h[12])), h[12]);
  fprintf(stderr, "[rt]   overflow-column pushes %llu (%.3f per ray)\n", h[14],
          (double)h[14] / (double)std::max(1u, traced));
  HIPCHK(c, hipMemset(c->d_stats + 6, 0, 10 * sizeof(unsigned long long)));
  {  // steps-per-ray histogram (16-step buckets) by ray kind
    unsigned long long hh[64];
    HIPCHK(c, hipMemcpy(hh, c->d_stats + 32, sizeof(hh), hipMemcpyDeviceToHost));
    static const char* kinds[4] = {"cont miss", "cont hit ", "shad miss", "shad hit "};
    for (int kd = 0; kd < 4; kd++) {
      fprintf(stderr, "[rt]   steps/ray %s:", kinds[kd]);
      for (int b = 0; b < 16; b++) fprintf(stderr, " %llu", hh[kd * 16 + b]);
      fprintf(stderr, "\n");
    }
    HIPCHK(c, hipMemset(c->d_stats + 32, 0, sizeof(hh)));
  }
  if (!WP.K.wave_log) return RT_OK;
  std::vector<unsigned long long> wave_log(dev_wave_words(c));
  HIPCHK(c, hipMemcpy(wave_log.data(), WP.K.wave_log, wave_log.size() * 8, hipMemcpyDeviceToHost));
  unsigned long long t0min = ~0ull, t1max = 0, t0max = 0, dmax = 0, itmax = 0, rmax = 0, cmax = 0;
  std::vector<unsigned long long> ends;
  double clk_sum = 0.0, wt_sum = 0.0;
  for (size_t w = 0; w < wave_log.size() / 8; w++) {  // (trace_grid * 4 waves, 4 words each)
    const unsigned long long* e = &wave_log[4 * w];
    const unsigned long long its = e[2] & 0xfffffull, cyc = e[2] >> 20;
    t0min = std::min(t0min, e[0]); t0max = std::max(t0max, e[0]); t1max = std::max(t1max, e[1]);
    if (e[1] - e[0] > dmax) { dmax = e[1] - e[0]; itmax = its; rmax = e[3]; cmax = cyc; }
    if (e[1] > e[0]) { clk_sum += (double)cyc; wt_sum += (double)(e[1] - e[0]); }
    ends.push_back(e[1]);
  }
  fprintf(stderr, "[rt]   shader clock: mean over waves %.0f MHz, longest wave %.0f MHz\n",
          wt_sum > 0 ? 100.0 * clk_sum / wt_sum : 0.0, dmax ? 100.0 * (double)cmax / (double)dmax : 0.0);
  std::sort(ends.begin(), ends.end());
  auto us = [](unsigned long long t) { return t / 100.0; };  // wall_clock64 = 100 MHz
  fprintf(stderr, "[rt]   waves: start spread %.1f us, span %.1f us; 50%% done at %.1f us, 90%% at %.1f, "
          "99%% at %.1f; longest wave %.1f us (%llu iters, %llu rays)\n", us(t0max - t0min),
          us(t1max - t0min), us(ends[ends.size() / 2] - t0min), us(ends[ends.size() * 9 / 10] - t0min),
          us(ends[ends.size() * 99 / 100] - t0min), us(dmax), itmax, rmax);
  return RT_OK;
}

// development aid: after pass 1's shade, whether the group moved to the row arena
// (WFParams::row_compact): pass 1's continuation hits as wf_p1_count counted them (4294967295: its
// sample of a long list put them far above the capacity and the list was not counted), the rows the
// arena holds for the group, the rows pass 1's shade claimed, and the decision of rtd::rows_on (syncs!)
int dev_rows_report(rt_ctx* c, hipStream_t st, const rtd::WFParams& WP) {
  unsigned int q[rtd::kCntRows + 1];
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipMemcpy(q, WP.S.cnt, sizeof(q), hipMemcpyDeviceToHost));
  const unsigned int hits = q[rtd::kCntP1Hits], claimed = q[rtd::kCntRows];
  fprintf(stderr, "[rt]   rows: enabled %d hits %u cap %u claimed %u compact %d\n", WP.row_compact, hits, WP.row_cap,
          claimed, (RT_ROW_COMPACT && WP.row_compact && hits <= WP.row_cap) ? 1 : 0);
  return RT_OK;
}
