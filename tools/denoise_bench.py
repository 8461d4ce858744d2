#!/usr/bin/env python3
"""Cost of the display denoiser on C3 (development aid; bench.py is the project's benchmark and is
not touched):

  (a) rt_denoise_async, 5 iterations, fresh guides (the library traces the first-hit frame);
  (b) the same with RT_DENOISE_REUSE_GUIDES (a still camera: pack + 5 a-trous launches);
  (c) the same with 2 iterations (s = 1, 2: the LDS-staged launches alone, so (b) - (c) is the
      three launches with s >= 4);
  (d) one-frame rt_render_async calls in the same process, for scale (pipeline depth 1 and 2).

Each is timed with HIP events on the ctx stream around `--reps` enqueued calls after a warm-up
call.  Prints one JSON line and appends it to profiles/denoise_bench.jsonl (--out).  Per-kernel
times (dn_pack / dn_atrous_* / the first-hit trace) come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/denoise_bench.py --reps 2 --out ''`.

    python tools/denoise_bench.py [--reps 20]
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
ap.add_argument("--variance", action="store_true",
                help="the variance mode (rt_variance_set): no temporal stage runs here, so every call pays the 7 x 7 "
                     "spatial estimate (tools/temporal_bench.py --variance times the chain that does not)")
ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise_bench.jsonl"), help="'' = do not write")
a = ap.parse_args()

import torch  # noqa: E402

from rtamd import configs as cf  # noqa: E402
from rtamd.renderer import DenoiseParams, Renderer  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("denoise_bench: no HIP device (times are measured on the GPU only)")

W, H = a.width, a.height
sd = cf.config_scene(a.config)
r = Renderer(0)
r.set_scene_soa(sd.soa, sd.nodes)
r.set_env(*cf.load_env())
r.resize(W, H)
if a.variance:
    r.set_variance(True)
fp = cf.frame_params(W, H)
ro = cf.rand_origins(2 * a.reps + 8)
stream = torch.cuda.ExternalStream(r.stream)
r.render(fp, ro[:1])  # a 1-spp accumulation: what the denoiser is for


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


res = {"config": a.config, "width": W, "height": H, "reps": a.reps, "variance": a.variance}
res["denoise_fresh_ms"] = timed(lambda k: r.denoise_async(fp))
res["denoise_reuse_ms"] = timed(lambda k: r.denoise_async(fp, reuse_guides=True))
res["denoise_reuse_2it_ms"] = timed(lambda k: r.denoise_async(fp, DenoiseParams(iterations=2), reuse_guides=True))
res["first_hit_share"] = round(1.0 - res["denoise_reuse_ms"] / res["denoise_fresh_ms"], 3)
for depth in (1, 2):
    r.set_pipeline(depth)
    res[f"render_1frame_depth{depth}_ms"] = timed(lambda k: r.render_async(fp, ro[1 + k:2 + k]))
r.set_pipeline(1)
res["reuse_over_render"] = round(res["denoise_reuse_ms"] / res["render_1frame_depth2_ms"], 3)
# dn_atrous' algorithmic traffic: 48 B read + 16 B written per pixel and iteration, 12 B on the last
px = W * H
res["atrous_algorithmic_bytes"] = px * (5 * 48 + 4 * 16 + 12)
r.close()
line = json.dumps(res)
print(line)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
