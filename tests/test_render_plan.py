"""CPU: which kernels a wavefront batch runs (csrc/common/render_plan.h through rts_render_plan).

rt_render.hip launches what rpl::plan_batch and rpl::step decide from the context's facts, the
call and the switches.  This test compares that decision field by field with a second statement of
the rules (tests/render_plan_model.py) over a grid of call shapes, restates the launch counts of
tests/test_gpu_launch_structure.py as literal cases, and checks the invariants of DESIGN.md §4
directly on the C++ plans.
"""
import copy
import itertools

import pytest

import render_plan_model as model
from rtamd import scene_lib as sl

MI = 1 << 20
COUNT_VISITS, NO_FINISH, FINISH, SERIAL = model.COUNT_VISITS, model.NO_FINISH, model.FINISH, model.SERIAL
B = 8  # max_bounce of the named cases: passes 0 .. B

# a context as rt_create + rt_resize(96, 72) leave it on a 256-CU device, one call of one frame
BASE = dict(n_groups=2, n_valid=96 * 72, frames_cap=1024, wf_paths=64 * MI, finish_pass=2, pipe_finish_pass=-1,
            finish_slots=8 * MI, split_kinds=1, split_passes=5, wide=1, mats_emissive=0, tile_cost_on=0,
            wf_hit_cap=MI + 64, wf_rows=16 * MI, order_head=0, pipe_depth=1, pipe_nomem_slots=(1 << 63) - 1,
            n_cus=256, trace_bpc0=8, trace_bpc=7, finish_bpc=3, pipe_finish_bpc=2, sh_sub=3, sh_sub_cam=8, sh_sub_bulk=8,
            p1_sample_every=16,
            flags=0, enable_bsdf=1, max_bounce=B, n_left=1, idle=0, pipe=0, pset=0,
            sw_cam_shade=1, sw_cam_shared=1, sw_cam_shared_static=0, sw_cam_miss_once=1, sw_p1_lean=1, sw_row_compact=1,
            sw_split_cont_first=0, sw_pix_split=1, sw_group_head=-1, sw_finish_pass_g0=-1, sw_finish_pass_g1=-1,
            sw_finish_pass_g2=-1, sw_finish_pass_g3=-1, sw_row_cap=-1)
assert tuple(BASE) == sl.PLAN_INPUTS


def named(plan):
    """rts_render_plan's plan with its enumerators by name, as the model states them"""
    for g in plan["groups"]:  # (in place: the plan is this call's own)
        for s in g["steps"]:
            for k in ("trace0", "trace1"):
                s[k] = None if s[k] < 0 else sl.PLAN_TRACE[s[k]]
            s["shade"] = None if s["shade"] < 0 else sl.PLAN_SHADE[s["shade"]]
    return plan


def differences(a, b):
    """The fields in which two plans differ, as (group, step, field) with -1 for "not in one"."""
    out = [(-1, -1, k) for k in sl.PLAN_HEAD if a[k] != b[k]]
    if len(a["groups"]) != len(b["groups"]):
        return out + [(-1, -1, "groups")]
    for gi, (ga, gb) in enumerate(zip(a["groups"], b["groups"])):
        out += [(gi, -1, k) for k in sl.PLAN_GROUP if ga[k] != gb[k]]
        if len(ga["steps"]) != len(gb["steps"]):
            out.append((gi, -1, "steps"))
            continue
        for si, (sa, sb) in enumerate(zip(ga["steps"], gb["steps"])):
            out += [(gi, si, k) for k in sl.PLAN_STEP if sa[k] != sb[k]]
    return out


def both(inputs):
    """(the C++ plan, named; the model's plan) for one set of inputs; pipelined inputs (pipe_depth
    2) run pipelined when the model's admission, the streams found busy, lets them"""
    if inputs["pipe_depth"] >= 2:
        inputs = dict(inputs, pipe=model.call_rules(inputs)["admit_pipe"])
    return named(sl.render_plan(inputs)), model.plan(inputs), inputs


# ---- the grid ------------------------------------------------------------------------------------
FRAMES = (1, 2, 3, 63, 64, 128, 512)
N_VALID = (63, 64, 127, 128, 384, 6912, 2073600)
N_GROUPS = (1, 2, 3, 4)
FLAGS = (0, COUNT_VISITS, NO_FINISH, FINISH, SERIAL)
PIPELINED = (0, 1)
FINISH_SLOTS = (1, 8 * MI)
FINISH_PASS = (0, 1, 2, 9)
MAX_BOUNCE = (0, 1, 2, 8)


def first_sweep(frames=FRAMES, n_valid=N_VALID, n_groups=N_GROUPS, flags=FLAGS, pipelined=PIPELINED,
                finish_slots=FINISH_SLOTS, finish_pass=FINISH_PASS, max_bounce=MAX_BOUNCE):
    for nf, nv, ng, fl, pp, fs, fpass, mb in itertools.product(frames, n_valid, n_groups, flags, pipelined, finish_slots,
                                                               finish_pass, max_bounce):
        yield dict(BASE, n_left=nf, n_valid=nv, n_groups=ng, flags=fl, pipe_depth=2 if pp else 1, pset=pp, finish_slots=fs,
                   finish_pass=fpass, max_bounce=mb)


def _group0(inputs):
    """(work items, slots) of the model's first group"""
    g = model.plan(inputs)["groups"][0]
    return g["w1"] - g["w0"], g["slots"]


# the second sweep: one change each to a point of the first
VARIANTS = [
    ("base", lambda i: {}),
    ("binary tree", lambda i: dict(wide=0)),
    ("emissive", lambda i: dict(mats_emissive=1)),
    ("tile-cost probe", lambda i: dict(tile_cost_on=1)),
    ("no split queues", lambda i: dict(split_kinds=0)),
    ("split_passes 0", lambda i: dict(split_passes=0)),
    ("split_passes 1", lambda i: dict(split_passes=1)),
    ("split_passes 8", lambda i: dict(split_passes=8)),
    ("ordered head", lambda i: dict(order_head=64)),
    ("hit list one short", lambda i: dict(wf_hit_cap=_group0(i)[0] - 1)),
    ("hit list exact", lambda i: dict(wf_hit_cap=_group0(i)[0])),
    ("arena four short", lambda i: dict(wf_rows=max(0, model.arena_rows(_group0(i)[1]) - 4))),
    ("arena exact", lambda i: dict(wf_rows=model.arena_rows(_group0(i)[1]))),
    ("pipelined finisher pass", lambda i: dict(pipe_finish_pass=1)),
    ("streams idle", lambda i: dict(idle=1)),
    # (RT_GROUP_SPLIT: whole 64-item blocks, here at most half of the work items)
    ("sw_group_head", lambda i: dict(sw_group_head=min(128, i["n_valid"] // 128 * 64))),
] + [(f"{k}={v}", lambda i, k=k, v=v: {k: v}) for k, v in (
    ("sw_cam_shade", 0), ("sw_cam_shared", 0), ("sw_cam_shared_static", 1), ("sw_cam_miss_once", 0), ("sw_p1_lean", 0),
    ("sw_row_compact", 0), ("sw_split_cont_first", 1), ("sw_pix_split", 0),
    ("sw_finish_pass_g0", 1), ("sw_finish_pass_g1", 3), ("sw_row_cap", 1))]


def check(inputs, tag):
    got, want, inputs = both(inputs)
    d = differences(got, want)
    assert not d, (tag, d[:8], inputs)
    invariants(got, inputs)
    return got


def test_model_agrees_over_the_grid():
    """The full first sweep, every point with one variant of the second in rotation (each variant
    meets about 2300 points) ..."""
    n = 0
    for n, inputs in enumerate(first_sweep()):
        tag, change = VARIANTS[n % len(VARIANTS)]
        inputs.update(change(inputs))
        check(inputs, tag)
    assert n + 1 == 7 * 7 * 4 * 5 * 2 * 2 * 4 * 4


@pytest.mark.parametrize("variant", range(len(VARIANTS)), ids=[v[0] for v in VARIANTS])
def test_model_agrees_for_every_variant(variant):
    """... and every variant of the second sweep on the shapes where the rules branch: one frame,
    fewer frames than groups, bulk groups of 64 and 256 frames, small and large images."""
    tag, change = VARIANTS[variant]
    for inputs in first_sweep(frames=(1, 3, 128, 512), n_valid=(384, 6912), n_groups=(2, 4), flags=(0, COUNT_VISITS, FINISH),
                              finish_pass=(1, 2), max_bounce=(8,)):
        inputs.update(change(inputs))
        check(inputs, tag)


# ---- invariants, stated on the C++ plan itself ---------------------------------------------------
SMALL = {"CAM_SMALL", "P1_SMALL", "REG_SMALL"}
SPLIT = {"P1_SHADOW", "P1_CONT_LEAN", "P1_CONT", "SHADOW", "CONT"}
COUNTING = {"CAM_CW", "P1_CW", "REG_CW", "CAM_CB", "P1_CB", "REG_CB"}


def invariants(p, i):
    G, groups = p["G"], p["groups"]
    assert 1 <= G <= i["n_groups"] and len(groups) == G
    # the groups tile the batch's frames or the work items exactly, without overlap
    if p["pix_split"]:
        assert all((g["f0"], g["f1"]) == (0, p["nf"]) for g in groups)
        assert groups[0]["w0"] == 0 and groups[-1]["w1"] == i["n_valid"]
        assert all(a["w1"] == b["w0"] for a, b in zip(groups, groups[1:]))
    else:
        assert all((g["w0"], g["w1"]) == (0, i["n_valid"]) for g in groups)
        assert groups[0]["f0"] == 0 and groups[-1]["f1"] == p["nf"]
        assert all(a["f1"] == b["f0"] for a, b in zip(groups, groups[1:]))
    assert all(g["f0"] < g["f1"] and g["w0"] < g["w1"] for g in groups)
    trace_grid_max = i["n_cus"] * max(i["trace_bpc"], i["trace_bpc0"])
    measuring = bool(i["flags"] & COUNT_VISITS) or bool(i["tile_cost_on"])
    for g in groups:
        steps = g["steps"]
        frames = g["f1"] - g["f0"]
        # fused blends: one-frame groups that do not blend in frame order
        if g["fuse_blend"]:
            assert frames == 1 and (p["pix_split"] or G == 1) and not i["pipe"]
        assert g["blend"] == 1 - g["fuse_blend"]
        # lean => miss-once => shared camera trace and CAM shade
        if g["p1_lean"]:
            assert g["cam_miss_once"]
            assert g["p1_compact"] and steps[0]["split_out"] and not i["mats_emissive"]
            assert steps[0]["shade"] == "CAM_LEAN" and steps[1]["shade"] == "BULK_LEAN"
        if g["cam_miss_once"]:
            assert g["cam_shared"] and steps[0]["cam_shared"] and steps[0]["classify"]
            assert steps[0]["shade"] in ("CAM", "CAM_LEAN")
        if g["row_compact"]:
            assert g["p1_lean"] and not g["finish"]
        assert all(s["p1_count"] == (g["row_compact"] and k == 1) for k, s in enumerate(steps))
        assert all(not s["classify"] and not s["cam_shared"] for s in steps[1:])
        # the finisher is the last step and nothing follows it
        assert [k for k, s in enumerate(steps) if s["finisher"]] == ([len(steps) - 1] if g["finish"] else [])
        assert len(steps) == g["n_steps"] <= max(0, i["max_bounce"]) + 1
        if not g["finish"]:
            assert len(steps) == max(0, i["max_bounce"]) + 1
        for s in steps:
            if s["finisher"]:
                assert 0 < s["fgrid"] <= trace_grid_max  # (ovf_layout_error's third condition)
                assert s["n_trace"] == 0 and s["shade"] is None
                continue
            # no grid is zero
            assert s["trace_grid"] > 0 and s["shade_grid"] > 0
            assert not s["classify"] or s["classify_grid"] > 0
            assert not s["p1_count"] or (s["p1_grid0"] > 0 and s["p1_grid1"] > 0)
            assert s["n_trace"] == (2 if s["trace1"] is not None else 1) and s["trace0"] is not None
            assert (s["n_trace"] == 2) == (s["trace0"] in SPLIT) and (s["n_trace"] == 2) <= bool(s["split"])
        # counting runs and tile-cost probes: none of the protocols
        if measuring:
            assert not (g["finish"] or g["split_g"] or g["cam_shared"] or g["cam_miss_once"] or g["p1_lean"])
            assert not any(s["split"] or s["split_out"] or s["cam_shared"] for s in steps)
        if i["flags"] & COUNT_VISITS:
            assert all(s["trace0"] in COUNTING and s["trace1"] is None for s in steps)


# ---- named cases: tests/test_gpu_launch_structure.py on the CPU -----------------------------------
def traces(p):
    """regular passes of the batch (rt_stats.trace_launches counts one per pass and group)"""
    return sum(1 for g in p["groups"] for s in g["steps"] if not s["finisher"])


def test_one_frame_runs_two_pixel_groups_into_the_finisher():
    p = check(dict(BASE), "one frame")
    assert (p["G"], p["pix_split"], traces(p)) == (2, 1, 4)
    assert [(g["w0"], g["w1"]) for g in p["groups"]] == [(0, 3456), (3456, 6912)]
    for g in p["groups"]:
        assert g["fuse_blend"] and g["finish"] and g["fin_pass"] == 2
        assert [s["finisher"] for s in g["steps"]] == [0, 0, 1]
        assert [s["trace0"] for s in g["steps"][:2]] == ["CAM_SMALL", "P1_SMALL"]
        assert [s["shade"] for s in g["steps"][:2]] == ["FUSED", "FUSED"]


@pytest.mark.parametrize("flag", [NO_FINISH, COUNT_VISITS])
def test_one_frame_without_the_finisher_runs_every_pass(flag):
    p = check(dict(BASE, flags=flag), "no finisher")
    assert (p["G"], p["pix_split"], traces(p)) == (2, 1, 2 * (B + 1))
    assert not any(s["finisher"] for g in p["groups"] for s in g["steps"])
    if flag == COUNT_VISITS:  # no split, small or lean enumerator
        assert {s["trace0"] for g in p["groups"] for s in g["steps"]} == {"CAM_CW", "P1_CW", "REG_CW"}
        assert all(s["trace1"] is None for g in p["groups"] for s in g["steps"])


def batches(inputs, n):
    out = []
    while n > 0:
        out.append(check(dict(inputs, n_left=n), "batches"))
        n -= out[-1]["nf"]
    return out


def test_frame_groups_over_two_batches():
    bs = batches(dict(BASE, frames_cap=4), 6)
    assert [b["nf"] for b in bs] == [4, 2] and [b["G"] for b in bs] == [2, 2]
    assert not any(b["pix_split"] for b in bs) and sum(traces(b) for b in bs) == 8
    assert [(g["f0"], g["f1"]) for g in bs[0]["groups"]] == [(0, 2), (2, 4)]


def test_serial_runs_one_group_per_batch():
    bs = batches(dict(BASE, frames_cap=4, wf_paths=2 * 6912, flags=SERIAL), 6)
    assert [b["nf"] for b in bs] == [2, 2, 2] and [b["G"] for b in bs] == [1, 1, 1]
    assert sum(traces(b) for b in bs) == 6


def test_bulk_groups_run_every_pass():
    rows = 4096
    p = check(dict(BASE, n_valid=24 * 16, n_left=128, finish_slots=1, wf_rows=rows), "bulk")
    assert (p["G"], p["pix_split"], traces(p)) == (2, 0, 2 * (B + 1))
    assert [(g["f0"], g["f1"]) for g in p["groups"]] == [(0, 64), (64, 128)]
    for g in p["groups"]:
        steps = g["steps"]
        assert g["slots"] == 64 * 384 and g["split_g"] and not g["finish"] and not g["fuse_blend"] and g["blend"]
        assert g["cam_shared"] and g["cam_miss_once"] and g["p1_lean"] and g["row_compact"]
        assert g["row_cap"] == min(model.arena_rows(g["slots"]), rows) == rows
        assert steps[0]["cam_shared"] and steps[0]["classify"] and steps[0]["shade"] == "CAM_LEAN"
        assert (steps[0]["trace0"], steps[0]["trace1"]) == ("CAM_W", None)
        assert (steps[1]["trace0"], steps[1]["trace1"]) == ("P1_SHADOW", "P1_CONT_LEAN")  # shadow first
        assert steps[1]["p1_count"] and steps[1]["shade"] == "BULK_LEAN"
        assert [s["split"] for s in steps] == [0, 1, 1, 1, 1, 1, 0, 0, 0]
        assert all((s["trace0"], s["trace1"]) == ("SHADOW", "CONT") for s in steps[2:6])
        assert all((s["trace0"], s["trace1"]) == ("REG_W", None) for s in steps[6:])
        assert all(s["shade"] == "BULK" for s in steps[2:])
    # the arena, not the context, bounds the rows of a smaller group
    p = check(dict(BASE, n_valid=24 * 16, n_left=128, finish_slots=1, wf_rows=16 * MI), "bulk")
    assert p["groups"][0]["row_cap"] == model.arena_rows(64 * 384) == 6144


def test_pipelined_calls():
    """One-frame calls run pipelined as one group on their set's stream unless the streams are
    idle; a batch that fits a set runs pipelined whatever the streams do."""
    busy = dict(BASE, pipe_depth=2, pset=1)
    p = check(busy, "pipelined")
    assert (p["idle_matters"], p["admit_pipe"], p["G"], p["pix_split"]) == (1, 1, 1, 0)
    g = p["groups"][0]
    assert (g["set"], g["stream"], g["fuse_blend"], g["finish"]) == (1, 2, 0, 1)
    assert g["steps"][-1]["fgrid"] == BASE["n_cus"] * BASE["pipe_finish_bpc"]
    p = check(dict(busy, idle=1), "pipelined, idle")
    assert (p["admit_pipe"], p["G"], p["pix_split"]) == (0, 2, 1)
    p = check(dict(busy, idle=1, n_left=8), "pipelined batch")
    assert (p["idle_matters"], p["admit_pipe"], p["G"]) == (0, 1, 1)


# ---- the comparison catches a fault --------------------------------------------------------------
@pytest.mark.parametrize("where, field, value", [
    ((0, None), "p1_lean", 0), ((1, None), "row_compact", 0), ((0, 1), "split", 0), ((0, 1), "trace1", "P1_CONT"),
    ((1, 0), "trace0", "CAM_SMALL"), ((0, 2), "shade", "PLAIN"), ((0, 0), "classify_grid", 1), ((None, None), "G", 1)])
def test_comparison_catches_a_changed_field(where, field, value):
    """As tests/test_dev_layout.py shows its checker catching an overlap: one field of a returned
    plan changed in a copy, and `differences` names exactly that field."""
    got, want, _ = both(dict(BASE, n_valid=24 * 16, n_left=128, finish_slots=1))
    assert differences(got, want) == []
    bad = copy.deepcopy(got)
    g, s = where
    target = bad if g is None else bad["groups"][g] if s is None else bad["groups"][g]["steps"][s]
    assert target[field] != value
    target[field] = value
    assert differences(bad, want) == [(-1 if g is None else g, -1 if s is None else s, field)]


def test_plan_rejects_inputs_outside_its_domain():
    for bad in (dict(n_groups=0), dict(n_groups=5), dict(n_left=0), dict(p1_sample_every=0), dict(sh_sub=0), dict(pset=3)):
        with pytest.raises(Exception):
            sl.render_plan(dict(BASE, **bad))
    with pytest.raises(Exception):  # a plan longer than the caller's buffer
        sl.render_plan(dict(BASE, flags=NO_FINISH, max_bounce=100000))
    assert len(sl.render_plan(dict(BASE, flags=NO_FINISH, max_bounce=100))["groups"][0]["steps"]) == 101
