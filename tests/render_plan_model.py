"""Which kernels a wavefront batch of rt_render_async launches: the rules of DESIGN.md §4's decision
table in Python, the model csrc/common/render_plan.h is compared with field by field
(tests/test_render_plan.py).  It calls no C++.

    p = plan(inputs)        inputs: a dict with every name of rtamd.scene_lib.PLAN_INPUTS

returns what rtamd.scene_lib.render_plan returns (the batch's head values, its groups, each group's
steps), except that a step names its kernels: "trace0" / "trace1" are names of PLAN_TRACE or None,
"shade" a name of PLAN_SHADE or None.

The rules are stated per question (who may run pipelined, how a batch is cut, which protocol a
group runs, what one pass launches), each from the facts alone, not in the order the host code
happens to ask them.
"""
from types import SimpleNamespace

COUNT_VISITS, MEGAKERNEL, NO_FINISH, FINISH, SERIAL = 2, 4, 8, 16, 32
MAX_FRAMES_PER_LAUNCH = 1024
U32 = 0xFFFFFFFF


def arena_rows(slots):
    """dvl::arena_rows: a quarter of the slots, in whole groups of 4 rows"""
    return slots // 4 // 4 * 4


def _ceil_div(a, b):
    return -(-a // b)


def _grid(blocks, most):
    return max(1, min(most, blocks))


def call_rules(inputs):
    """The call's part of the plan: the batch size and whether the call may run pipelined"""
    i = SimpleNamespace(**inputs)
    mega = bool(i.flags & MEGAKERNEL)
    serial = bool(i.flags & SERIAL) and not mega
    pixels = max(1, i.n_valid)
    if mega:
        batch_cap = MAX_FRAMES_PER_LAUNCH
    elif serial:  # what one group's path state holds
        batch_cap = max(1, min(i.frames_cap, i.wf_paths // pixels))
    else:
        batch_cap = i.frames_cap
    pipe_sets = min(i.pipe_depth, i.n_groups)
    fits_a_set = i.n_left < i.n_groups or (i.n_left <= i.frames_cap and i.n_left * pixels < i.pipe_nomem_slots)
    candidate = pipe_sets >= 2 and not mega and not serial and i.n_left > 0 and _groups_possible(i) and fits_a_set
    idle_matters = candidate and _may_split_pixels(i, i.n_left)
    admit = candidate and not (idle_matters and i.idle)
    return dict(batch_cap=batch_cap, serial=int(serial), pipe_sets=pipe_sets, idle_matters=int(idle_matters),
                admit_pipe=int(admit))


def _groups_possible(i):
    """every group gets whole 64-item blocks, and a tile-cost probe keeps one wavefront"""
    return i.n_valid >= 64 * i.n_groups and not i.tile_cost_on


def _may_split_pixels(i, frames):
    return bool(i.sw_pix_split) and frames < i.n_groups and _groups_possible(i)


def plan(inputs):
    i = SimpleNamespace(**inputs)
    call = call_rules(inputs)
    count = bool(i.flags & COUNT_VISITS)
    serial = bool(call["serial"])
    probe = bool(i.tile_cost_on)

    # ---- the batch: frame groups, pixel groups or one group
    nf = min(call["batch_cap"], i.n_left)
    pipe = bool(i.pipe)
    one_group = pipe or serial
    pix_split = not one_group and _may_split_pixels(i, nf)
    G = 1 if one_group else i.n_groups if pix_split else min(i.n_groups, nf)
    head = i.sw_group_head if i.sw_group_head >= 0 else min(i.order_head, i.n_valid)
    if pix_split:
        if head > 0 and G > 1:  # the costly head alone, the rest in even shares
            cuts = [0] + [head + (i.n_valid - head) * k // (G - 1) for k in range(G - 1)] + [i.n_valid]
        else:
            cuts = [i.n_valid * k // G for k in range(G)] + [i.n_valid]
        ranges = [(0, nf, cuts[k], cuts[k + 1]) for k in range(G)]
    else:
        ranges = [(k * nf // G, (k + 1) * nf // G, 0, i.n_valid) for k in range(G)]

    last_pass = max(0, i.max_bounce)
    groups = []
    for k, (f0, f1, w0, w1) in enumerate(ranges):
        frames, work = f1 - f0, w1 - w0
        slots = frames * work & U32
        # ---- which protocol the group runs
        fused = not pipe and frames == 1 and (pix_split or G == 1) and not count
        small = slots <= i.finish_slots  # within the finisher's budget
        bulk = not small and not fused
        measuring = count or probe       # counting runs and tile-cost probes keep the plain protocol
        split = bool(i.split_kinds) and bool(i.wide) and bulk and not measuring
        fin_pass = i.pipe_finish_pass if pipe and i.pipe_finish_pass >= 0 else i.finish_pass
        if inputs[f"sw_finish_pass_g{k}"] >= 0:
            fin_pass = inputs[f"sw_finish_pass_g{k}"]
        finish = (not measuring and not i.flags & NO_FINISH and 1 <= fin_pass <= last_pass
                  and (bool(i.flags & FINISH) or small))
        p1_compact = not (finish and fin_pass == 1)  # the finisher reads full rays
        cam_shared = bool(i.sw_cam_shared) and frames > 1 and not measuring
        cam_shade = bool(i.sw_cam_shade) and bulk and slots > 0 and frames >= 64
        miss_once = bool(i.sw_cam_miss_once) and cam_shared and cam_shade and work <= i.wf_hit_cap
        lean = (bool(i.sw_p1_lean) and miss_once and p1_compact and last_pass >= 1 and split and i.split_passes >= 1
                and not i.mats_emissive)
        rows = bool(i.sw_row_compact) and lean and not finish
        row_cap = min(arena_rows(slots), i.wf_rows)
        if i.sw_row_cap >= 0:
            row_cap = min(row_cap, i.sw_row_cap)
        n_steps = fin_pass + 1 if finish else last_pass + 1

        # ---- what each pass launches
        steps = []
        for p in range(n_steps):
            s = dict(finisher=0, fgrid=0, split=int(split and 1 <= p <= i.split_passes),
                     split_out=int(split and p + 1 <= i.split_passes), cam_n=0, cam_shared=0, n_trace=0, trace0=None,
                     trace1=None, trace_grid=0, classify=0, classify_grid=0, p1_count=0, p1_grid0=0, p1_grid1=0,
                     shade=None, shade_grid=0)
            steps.append(s)
            if finish and p == fin_pass:
                s.update(finisher=1, fgrid=i.n_cus * (i.pipe_finish_bpc if pipe else i.finish_bpc))
                continue
            camera = p == 0 and slots > 0
            rays16 = p == 1 and p1_compact  # pass 1 reads the 16-B rays pass 0 queued
            which = "CAM" if camera else "P1" if rays16 else "REG"
            shared = p == 0 and cam_shared
            s.update(cam_n=slots if p == 0 else 0, cam_shared=int(shared),
                     trace_grid=i.n_cus * (i.trace_bpc0 if p == 0 else i.trace_bpc))
            if count or not i.wide:  # one queue of both kinds: counting / 4-wide / binary
                traces = [which + "_" + ("C" if count else "") + ("W" if i.wide else "B")]
            elif small or (shared and i.sw_cam_shared_static):
                traces = [which + "_SMALL"]
            elif s["split"] and not camera:
                cont = ("P1_CONT_LEAN" if lean else "P1_CONT") if rays16 else "CONT"
                shadow = "P1_SHADOW" if rays16 else "SHADOW"
                traces = [cont, shadow] if i.sw_split_cont_first else [shadow, cont]
            else:
                traces = [which + "_W"]
            s.update(n_trace=len(traces), trace0=traces[0], trace1=traces[1] if len(traces) > 1 else None)
            if p == 0 and miss_once:
                s.update(classify=1, classify_grid=_grid(_ceil_div(work, 256), 2 * i.n_cus))
            if p == 1 and lean and rows:
                runs = _ceil_div(min(slots, work * frames), 256)
                s.update(p1_count=1, p1_grid0=_grid(runs // i.p1_sample_every + 1, 8 * i.n_cus),
                         p1_grid1=_grid(runs, 8 * i.n_cus))
            if fused:
                shade = "FUSED"
            elif p == 0 and lean:
                shade = "CAM_LEAN"
            elif p == 0 and cam_shade:
                shade = "CAM"
            elif p == 1 and lean:
                shade = "BULK_LEAN"
            else:
                shade = "BULK" if bulk else "PLAIN"
            per_block = 256 * {"CAM": i.sh_sub_cam, "CAM_LEAN": i.sh_sub_cam, "BULK": i.sh_sub_bulk,
                               "BULK_LEAN": i.sh_sub_bulk}.get(shade, i.sh_sub)
            s.update(shade=shade, shade_grid=_grid(_ceil_div(slots, per_block), 4096))
        groups.append(dict(f0=f0, f1=f1, w0=w0, w1=w1, slots=slots, set=i.pset if pipe else k,
                           stream=1 + i.pset if pipe else k, fuse_blend=int(fused), split_g=int(split), finish=int(finish),
                           fin_pass=fin_pass, p1_compact=int(p1_compact), cam_shared=int(cam_shared),
                           cam_miss_once=int(miss_once), p1_lean=int(lean), row_compact=int(rows), row_cap=row_cap & U32,
                           blend=int(not fused), n_steps=n_steps, steps=steps))
    return dict(call, nf=nf, G=G, pix_split=int(pix_split), groups=groups)
