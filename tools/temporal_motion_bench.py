#!/usr/bin/env python3
"""Cost and benefit of the temporal stage's motion mode (rt_temporal_set_motion) on C3 with the loong
turning (development aid, the sibling of tools/temporal_bench.py; bench.py is not touched).

  --part stage    ms per rt_temporal_async call, HIP events on the ctx stream around --reps enqueued
                  calls after a warm-up, still camera, with REUSE_GUIDES (colour pack + resolve) and
                  with fresh guides (first-hit trace + packs + resolve):
                    off            mode off
                    on_still       mode on, nothing moved (the host launches the mode-off kernel)
                    on_moved       mode on, the history's pose one update behind: the loong's pixels on
                                   the moved path (no ADVANCE: every call reprojects the same history)
                  and the pose copy: the first fresh call after an update (copies 2 x 48 B per
                  triangle) minus the same call repeated, over --reps updates.
  --part quality  the loong turns --degrees per tick for --ticks ticks at 1 spp per tick; per tick the
                  RMS error of the linear displayed frame over the pixels whose first hit is a loong
                  triangle, against a --ref-spp render of the same pose (non-finite pixels masked and
                  counted), for: no temporal stage, mode off (ADVANCE each tick), RT_TEMPORAL_RESET
                  with each update, mode on; and the share of those pixels that found no history.

Prints one JSON line per part and appends it to profiles/temporal_motion_bench_C3.jsonl (--out).
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "opengl-ray-tracing-framework_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["stage", "quality"], default="stage")
ap.add_argument("--config", default="C3")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ticks", type=int, default=16)
ap.add_argument("--degrees", type=float, default=3.0)
ap.add_argument("--ref-spp", type=int, default=256)
ap.add_argument("--out", default=str(ROOT / "profiles" / "temporal_motion_bench_C3.jsonl"), help="'' = do not write")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rtamd import configs as cf  # noqa: E402
from rtamd import geometry as geo  # noqa: E402
from rtamd.renderer import Renderer, TemporalParams  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("temporal_motion_bench: no HIP device (times and images come from the GPU only)")

W, H = a.width, a.height
sd = cf.config_scene(a.config)
spun = len(sd.objects) - 1
obj = sd.objects[spun]


def turned(degrees):
    return geo.moved_object(sd, spun, (obj.rotate[0], obj.rotate[1] + degrees, obj.rotate[2]), obj.translate, obj.scale)


r = Renderer(0)
r.set_scene_soa(sd.soa, sd.nodes)
r.set_env(*cf.load_env())
r.resize(W, H)
fp = cf.frame_params(W, H)
stream = torch.cuda.ExternalStream(r.stream)
res = {"part": a.part, "config": a.config, "width": W, "height": H, "triangles_moved": int(len(turned(0.0)[0]))}


def timed(call, reps):
    call()
    r.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        call()
    e1.record(stream)
    r.synchronize()
    return round(e0.elapsed_time(e1) / reps, 4)


def part_stage():
    res["reps"] = a.reps
    ro = cf.rand_origins(4)
    poses = [turned(a.degrees * k) for k in range(3)]
    for mode in ("off", "on_still", "on_moved"):
        r.set_temporal_motion(mode != "off")
        r.update_geometry(*poses[0])
        r.reset()
        r.render(fp, ro[:1])
        r.temporal_async(fp, advance=True, reset=True)
        r.temporal_async(fp, advance=True)  # the history: this pose's
        if mode == "on_moved":
            r.update_geometry(*poses[1])
            r.reset()
            r.render(fp, ro[1:2])
        res[f"{mode}_fresh_ms"] = timed(lambda: r.temporal_async(fp), a.reps)
        res[f"{mode}_reuse_ms"] = timed(lambda: r.temporal_async(fp, reuse_guides=True), a.reps)
        n = r.temporal_history()
        res[f"{mode}_history_share"] = round(float((n > 1).mean()), 4)
    # the pose copy: a fresh call right after an update against the same call again
    first, again = [], []
    for k in range(a.reps):
        r.update_geometry(*poses[1 + (k & 1)])
        for into in (first, again):
            r.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r.temporal_async(fp)
            e1.record(stream)
            r.synchronize()
            into.append(e0.elapsed_time(e1))
    res["fresh_call_with_pose_copy_ms"] = round(float(np.median(first)), 4)
    res["fresh_call_again_ms"] = round(float(np.median(again)), 4)
    res["pose_copy_ms"] = round(float(np.median(first) - np.median(again)), 4)
    res["pose_copy_bytes"] = 2 * 48 * int(r.scene_download("tri").shape[0] // 3)
    r.set_pipeline(1)
    res["render_1frame_ms"] = timed(lambda: r.render_async(fp, ro[:1]), a.reps)
    res["denoise_fresh_ms"] = timed(lambda: r.denoise_async(fp), a.reps)  # (for scale: trace + packs + five filter passes)


def part_quality():
    ticks = a.ticks
    poses = [turned(a.degrees * (k + 1)) for k in range(ticks)]
    loong = np.zeros(int(r.scene_download("tri").shape[0] // 3), bool)
    loong[poses[0][0]] = True
    ro = cf.rand_origins(ticks + a.ref_spp)
    refs, masks = [], []
    r.set_temporal_motion(False)
    for k in range(ticks):  # the references, and the first-hit masks
        r.update_geometry(*poses[k])
        r.reset()
        r.clear_accum()
        r.render(fp, ro[ticks:ticks + a.ref_spp])
        refs.append(r.read_accum().astype(np.float64))
        t = r.first_hit(fp)["triangle"]
        masks.append((t >= 0) & loong[np.maximum(t, 0)])
    cols = {"none": [], "off": [], "reset": [], "on": []}
    nonfinite = {k: 0 for k in cols}
    no_history = {"off": [], "on": []}
    for col in cols:
        r.set_temporal_motion(col == "on")
        r.update_geometry(*turned(0.0))
        r.reset()
        r.clear_accum()
        r.render(fp, ro[:1])
        if col != "none":
            r.temporal(fp, TemporalParams(samples=1), advance=True, reset=True)  # tick 0: the loong at rest
        for k in range(ticks):
            r.update_geometry(*poses[k])
            r.reset()
            r.clear_accum()
            r.render(fp, ro[k:k + 1])
            if col == "none":
                img = r.read_accum()
            else:
                img = r.temporal(fp, TemporalParams(samples=1), advance=True, reset=col == "reset")
            m = masks[k]
            d = img[m].astype(np.float64) - refs[k][m]
            ok = np.isfinite(d).all(-1)
            nonfinite[col] += int((~ok).sum())
            cols[col].append(round(float(np.sqrt((d[ok] ** 2).mean())), 5))
            if col in no_history:
                no_history[col].append(round(float((r.temporal_history()[m] <= 1).mean()), 4))
    res.update(ticks=ticks, degrees_per_tick=a.degrees, ref_spp=a.ref_spp, loong_pixels=[int(m.sum()) for m in masks],
               rms=cols, nonfinite_masked=nonfinite, no_history_share=no_history)


{"stage": part_stage, "quality": part_quality}[a.part]()
r.set_temporal_motion(False)
r.close()
line = json.dumps(res)
print(line)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
