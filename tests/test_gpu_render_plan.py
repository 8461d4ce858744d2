"""The plan the library runs is the plan the CPU tests check.

Under RT_DEBUG_PASSES the development library prints, before each group's passes, one line
`[rt] plan group <g>: ...` with the planner's inputs as it copied them from the real context
(occupancy, CU count, path-state sizes, finisher limits), the batch, the group and its steps
(csrc/hip/rt_dev_report.h dev_plan_report).  For two call shapes, bulk frame groups (lean, split
queues, dense rows) and one frame split by pixels into the finisher, every printed line's inputs go
through rts_render_plan (the planner tests/test_render_plan.py compares with its model) and must
give the printed plan; the images equal the oracle bit for bit.  One child process renders both
(RT_DEBUG_PASSES is read once per process; the test is about that report).
"""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import bit_mismatch, frames_for, oracle_render
from rtamd import configs as cf
from rtamd import scene_lib as sl

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SHAPES = {"bulk": (24, 16, 128, (2, 1)), "single": (96, 72, 1, None)}  # width, height, frames, set_finish

_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1] + "/opengl-ray-tracing-framework_amd"]
import numpy as np
from rtamd import configs as cf
from rtamd.renderer import Renderer, dev_lib_path
sd, env = cf.config_scene("C3"), cf.load_env()
r = Renderer(0, lib_path=dev_lib_path())
for tag, w, h, n, finish in (("bulk", 24, 16, 128, (2, 1)), ("single", 96, 72, 1, None)):
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env)
    r.resize(w, h)
    if finish:
        r.set_finish(*finish)
    r.clear_accum()
    r.set_loop_num(0)
    print("==== " + tag, file=sys.stderr, flush=True)
    r.render(cf.frame_params(w, h), cf.rand_origins(n))
    np.save(sys.argv[2] + "/" + tag + ".npy", r.read_accum())
    if finish:
        r.set_finish(2, 8 << 20)
r.close()
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """{shape: [printed plan line as a dict of strings, ...]} and the directory of the images"""
    out = tmp_path_factory.mktemp("render_plan")
    env = dict(os.environ, RT_DEBUG_PASSES="1")
    for k in [k for k in env if k.startswith("RT_") and k != "RT_DEBUG_PASSES"]:
        del env[k]
    p = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, tag = {}, None
    for ln in p.stderr.splitlines():
        if ln.startswith("==== "):
            tag = ln[5:].strip()
        m = re.match(r"\[rt\] plan group (\d+): (.*)", ln)
        if m:
            kv = dict(f.split("=", 1) for f in m.group(2).split())
            lines.setdefault(tag, []).append(dict(kv, group=m.group(1)))
    assert set(lines) == set(SHAPES), p.stderr[-2000:]
    return lines, out


def _printed_matches_planner(line):
    """The line's plan, after requiring that rts_render_plan gives the same from the line's inputs"""
    inputs = {k: int(line[k]) for k in sl.PLAN_INPUTS}
    plan = sl.render_plan(inputs)
    g = int(line["group"])
    assert (plan["nf"], plan["G"], plan["pix_split"]) == (int(line["nf"]), int(line["G"]), int(line["pix_split"])), line
    want = plan["groups"][g]
    assert {k: int(line[k]) for k in sl.PLAN_GROUP} == {k: want[k] for k in sl.PLAN_GROUP}, line
    steps = [dict(zip(sl.PLAN_STEP, (int(v) for v in s.split(",")))) for s in line["steps"].split(";")]
    assert steps == want["steps"], (steps, want["steps"])
    return plan, want


def test_bulk_groups_run_the_checked_plan(report, env_maps):
    lines, out = report
    w, h, n, _ = SHAPES["bulk"]
    assert [ln["group"] for ln in lines["bulk"]] == ["0", "1"]
    for ln in lines["bulk"]:
        plan, g = _printed_matches_planner(ln)
        assert (plan["G"], plan["pix_split"], g["f1"] - g["f0"], g["slots"]) == (2, 0, 64, 64 * w * h)
        assert g["split_g"] and g["cam_miss_once"] and g["p1_lean"] and g["row_compact"] and not g["finish"]
        assert g["row_cap"] == min((g["slots"] // 4) & ~3, int(ln["wf_rows"]))
        assert [sl.PLAN_TRACE[s["trace0"]] for s in g["steps"][:3]] == ["CAM_W", "P1_SHADOW", "SHADOW"]
        assert g["steps"][1]["p1_count"] and len(g["steps"]) == int(ln["max_bounce"]) + 1
    sd = cf.config_scene("C3")
    ref, _ = oracle_render(sd, env_maps, w, h, frames_for(cf.frame_params(w, h), 1, n)[1])
    assert bit_mismatch(np.load(out / "bulk.npy"), ref)[0] == 0.0


def test_one_frame_runs_the_checked_plan(report, env_maps):
    lines, out = report
    w, h, n, _ = SHAPES["single"]
    assert [ln["group"] for ln in lines["single"]] == ["0", "1"]
    for ln in lines["single"]:
        plan, g = _printed_matches_planner(ln)
        assert (plan["G"], plan["pix_split"], g["fuse_blend"], g["finish"], g["fin_pass"]) == (2, 1, 1, 1, 2)
        assert [s["finisher"] for s in g["steps"]] == [0, 0, 1]
        # the finisher's lanes index the overflow column of the trace grid
        assert g["steps"][2]["fgrid"] <= max(s["trace_grid"] for s in g["steps"][:2])
    assert (int(lines["single"][0]["w0"]), int(lines["single"][1]["w1"])) == (0, w * h)
    sd = cf.config_scene("C3")
    ref, _ = oracle_render(sd, env_maps, w, h, frames_for(cf.frame_params(w, h), 1, n)[1])
    assert bit_mismatch(np.load(out / "single.npy"), ref)[0] == 0.0
