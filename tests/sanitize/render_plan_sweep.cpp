// render_plan_sweep.cpp — csrc/common/render_plan.h under AddressSanitizer and UBSan, stand-alone
// (`make -C tests/sanitize`: g++ -fsanitize=address,undefined, no GPU, no Python).
//
// Sweeps the call shapes of tests/test_gpu_launch_structure.py and a slice of the grid of
// tests/test_render_plan.py through plan_batch, step and the two flatten()s into buffers of
// exactly the advertised sizes on the heap, so an index past a fixed-size array or a name table
// that has lost step with its struct is an error here.  The values themselves are
// tests/test_render_plan.py's business; this only asserts what keeps the executor in bounds.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "render_plan.h"

#define REQUIRE(x)                                                        \
  do {                                                                    \
    if (!(x)) {                                                           \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #x);   \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

static rpl::In base() {
  rpl::In in{};
  in.f = rpl::Facts{2, 96 * 72, 1024, 64 << 20, 2, -1, 8 << 20, 1, 5, 1, 0, 0, (1 << 20) + 64, 16 << 20, 0, 1, INT64_MAX,
                    256, 8, 7, 3, 2, 3, 8, 8, 16};
  in.c = rpl::Call{0, 1, 8, 1, 0, 0, 0};
  in.s = rpl::Switches();
  return in;
}

static long checked = 0;

// one call: every batch of it, every group, every pass
static void run(rpl::In in) {
  for (int64_t left = in.c.n_left; left > 0;) {
    in.c.n_left = left;
    in.c.pipe = rpl::admit_pipe(in.f, in.s, in.c);
    const rpl::Batch B = rpl::plan_batch(in.f, in.s, in.c);
    REQUIRE(B.nf >= 1 && B.nf <= left && B.nf <= rpl::batch_cap(in.f, in.c));
    REQUIRE(B.G >= 1 && B.G <= rpl::kMaxGroups && B.G <= in.f.n_groups);
    for (int g = 0; g < B.G; g++) {
      const rpl::Group& G = B.g[g];
      REQUIRE(G.set >= 0 && G.set < rpl::kMaxGroups && G.stream >= 0 && G.stream < rpl::kMaxGroups);
      REQUIRE(G.f0 >= 0 && G.f0 < G.f1 && G.f1 <= B.nf && G.w0 <= G.w1 && G.w1 <= (unsigned)in.f.n_valid);
      REQUIRE(G.w0 < G.w1 || in.s.group_head >= 0);  // (RT_GROUP_SPLIT=1 leaves the other groups empty)
      REQUIRE(G.n_steps >= 1 && G.n_steps <= std::max<int64_t>(0, in.c.max_bounce) + 1);
      std::unique_ptr<int64_t[]> gv(new int64_t[rpl::kGroupCount]);
      rpl::flatten(G, gv.get());
      for (int pass = 0; pass < G.n_steps; pass++) {
        const rpl::Step s = rpl::step(in.f, in.s, in.c, G, pass);
        std::unique_ptr<int64_t[]> sv(new int64_t[rpl::kStepCount]);
        rpl::flatten(s, sv.get());
        REQUIRE(s.finisher == (G.finish && pass == G.n_steps - 1));
        if (s.finisher) continue;
        REQUIRE(s.n_trace == 1 || s.n_trace == 2);
        for (int k = 0; k < s.n_trace; k++) REQUIRE(s.trace[k] >= 0 && s.trace[k] < rpl::kTraceCount);
        REQUIRE(s.shade >= 0 && s.shade < rpl::kShadeCount);
        REQUIRE(s.trace_grid > 0 && s.shade_grid > 0);
        checked++;
      }
    }
    left -= B.nf;
  }
}

int main() {
  // the named cases
  rpl::In in = base();
  run(in);
  for (int64_t f : {RT_FLAG_NO_FINISH, RT_FLAG_COUNT_VISITS, RT_FLAG_FINISH, RT_FLAG_SERIAL, RT_FLAG_MEGAKERNEL}) {
    in = base();
    in.c.flags = f;
    run(in);
  }
  in = base(), in.f.frames_cap = 4, in.c.n_left = 6;
  run(in);
  in.f.wf_paths = 2 * 6912, in.c.flags = RT_FLAG_SERIAL;
  run(in);
  in = base(), in.f.n_valid = 24 * 16, in.f.finish_slots = 1, in.c.n_left = 128;
  run(in);
  // a slice of the grid: every group count and frame count against the sizes where the rules
  // branch, pipelined or not, with the overrides at their ends
  for (int64_t ng = 1; ng <= rpl::kMaxGroups; ng++)
    for (int64_t nf : {1, 2, 3, 4, 5, 63, 64, 128, 512, 1025})
      for (int64_t nv : {63, 64, 255, 256, 384, 6912, 2073600})
        for (int64_t depth : {1, 2, 4})
          for (int64_t mb : {-1, 0, 1, 8, 40})
            for (int64_t fs : {int64_t(1), int64_t(8) << 20})
              for (int v = 0; v < 4; v++) {
                in = base();
                in.f.n_groups = ng, in.f.n_valid = nv, in.f.pipe_depth = depth, in.f.finish_slots = fs;
                in.c.n_left = nf, in.c.max_bounce = mb, in.c.pset = std::min<int64_t>(depth, ng) - 1 > 0 ? 1 : 0;
                if (v == 1) in.f.order_head = 64, in.f.split_passes = 40, in.c.idle = 1;
                if (v == 2) in.s.group_head = nv / 64 * 64, in.s.row_cap = 0, in.s.finish_pass_g[ng - 1] = 1;
                if (v == 3) in.f.finish_pass = 40, in.f.pipe_finish_pass = 0, in.f.wf_rows = 0, in.f.wf_hit_cap = 0;
                run(in);
              }
  printf("render_plan_sweep: %ld passes planned, clean\n", checked);
  return 0;
}
