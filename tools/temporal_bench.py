#!/usr/bin/env python3
"""Cost of the temporal stage of the displayed frame on C3 (development aid, the sibling of
tools/denoise_bench.py; bench.py is the project's benchmark and is not touched):

  (a) rt_temporal_async with ADVANCE and REUSE_GUIDES: colour pack + the resolve kernel, every call
      reprojecting the previous call's output (still camera);
  (b) the same without ADVANCE (the ticks of a still view: a frozen history);
  (c) ADVANCE with a fresh first-hit trace, the camera alternating between two views a strafe
      apart (a moving camera: every call reprojects across the move);
  (d) the chain (c) -> rt_denoise_async(REUSE_GUIDES) on its output, and the still chain (b) -> the
      same: what a tick of the interactive loop queues with both settings on;
  (e) rt_denoise_async alone (fresh and reused guides) and one-frame rt_render_async calls
      (pipeline depth 1 and 2) in the same process, for scale.

Each is timed with HIP events on the ctx stream around `--reps` enqueued calls after a warm-up
call.  Prints one JSON line and appends it to profiles/temporal_bench_C3.jsonl (--out).

    python tools/temporal_bench.py [--reps 20]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "opengl-ray-tracing-framework_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--variance", action="store_true", help="the variance mode (rt_variance_set) for every stage timed")
ap.add_argument("--out", default=str(ROOT / "profiles" / "temporal_bench_C3.jsonl"), help="'' = do not write")
a = ap.parse_args()

import torch  # noqa: E402

from rtamd import configs as cf  # noqa: E402
from rtamd import interactive as ia  # noqa: E402
from rtamd.renderer import FrameParams, Renderer  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("temporal_bench: no HIP device (times are measured on the GPU only)")

W, H = a.width, a.height
sd = cf.config_scene(a.config)
r = Renderer(0)
r.set_scene_soa(sd.soa, sd.nodes)
r.set_env(*cf.load_env())
r.resize(W, H)
if a.variance:
    r.set_variance(True)
cam = ia.Camera(W / H)


def view():
    return FrameParams(position=cam.position, front=cam.front, right=cam.right, up=cam.up,
                       left_bottom_corner=cam.left_bottom_corner, half_h=float(cam.half_h), half_w=float(cam.half_w))


fp = view()
cam.process_keyboard(ia.RIGHT, 0.02)  # 0.05 units to the right
views = (fp, view())
ro = cf.rand_origins(2 * a.reps + 8)
stream = torch.cuda.ExternalStream(r.stream)
r.render(fp, ro[:1])  # a 1-spp accumulation: what the stage is for


def timed(call):
    """ms per call of `call` enqueued --reps times on the ctx stream, after one warm-up."""
    call(0)
    r.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for k in range(a.reps):
        call(1 + k)
    e1.record(stream)
    r.synchronize()
    return round(e0.elapsed_time(e1) / a.reps, 4)


def chain(k, moving):
    if moving:
        out = r.temporal_async(views[k & 1], advance=True)
    else:
        out = r.temporal_async(fp, reuse_guides=True)
    r.denoise_async(views[k & 1] if moving else fp, frame_ptr=out, reuse_guides=True)


res = {"config": a.config, "width": W, "height": H, "reps": a.reps, "variance": a.variance}
r.temporal_async(fp, advance=True)  # guides and a first output
res["temporal_advance_reuse_ms"] = timed(lambda k: r.temporal_async(fp, advance=True, reuse_guides=True))
res["temporal_reuse_ms"] = timed(lambda k: r.temporal_async(fp, reuse_guides=True))
res["temporal_advance_fresh_moving_ms"] = timed(lambda k: r.temporal_async(views[k & 1], advance=True))
res["chain_moving_ms"] = timed(lambda k: chain(k, True))
r.temporal_async(fp, advance=True)
res["chain_still_ms"] = timed(lambda k: chain(k, False))
res["history_share"] = round(float((r.temporal_history() > 1).mean()), 3)  # pixels that found a history
res["denoise_fresh_ms"] = timed(lambda k: r.denoise_async(fp))
res["denoise_reuse_ms"] = timed(lambda k: r.denoise_async(fp, reuse_guides=True))
for depth in (1, 2):
    r.set_pipeline(depth)
    res[f"render_1frame_depth{depth}_ms"] = timed(lambda k: r.render_async(fp, ro[1 + k:2 + k]))
r.set_pipeline(1)
# the resolve's algorithmic traffic per pixel: 48 B of the current colour and guides, up to 4 x 48 B
# of history taps (neighbouring lanes share them: 48 B when served from cache), 28 B written
res["resolve_algorithmic_bytes"] = W * H * (48 + 48 + 28)
r.close()
line = json.dumps(res)
print(line)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
