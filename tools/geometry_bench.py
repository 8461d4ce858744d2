#!/usr/bin/env python3
"""Cost of moving an object: rt_update_geometry (host form and device form) against the only way
before it, a host BVH build + rt_set_scene, in one process; and what a render call costs on the
refitted tree, which is no longer SAH-built for the new pose.

C3: every loong triangle under a new transform (rtamd.geometry.moved_object), a different one per
call.  Prints one JSON line; --out appends it to a .jsonl file.

    python tools/geometry_bench.py --config C3 --calls 20 --out out/geometry_bench_C3.jsonl
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "opengl-ray-tracing-framework_amd"))

from rtamd import configs as cf  # noqa: E402
from rtamd import geometry as geo  # noqa: E402
from rtamd.renderer import Renderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--object", type=int, default=1, help="which object of the config moves")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rebuilds", type=int, default=3, help="timed repetitions of the build + rt_set_scene path")
ap.add_argument("--width", type=int, default=0)
ap.add_argument("--height", type=int, default=0)
ap.add_argument("--render-calls", type=int, default=20)
ap.add_argument("--trace-only", action="store_true", help="a warm-up and 3 device-form calls (for a kernel trace)")
ap.add_argument("--out", default="")
a = ap.parse_args()

import torch  # noqa: E402

cfg = cf.CONFIGS[a.config]
W, H = a.width or cfg.width, a.height or cfg.height
sd = cf.config_scene(a.config)
o = sd.objects[a.object]


def pose(k):
    """The k-th pose: the object turned about the vertical axis, shifted and a little smaller."""
    return dict(rotate=(o.rotate[0], o.rotate[1] + 7.0 * (k + 1), o.rotate[2]),
                translate=(o.translate[0] + 0.01 * k, o.translate[1], o.translate[2]),
                scale=tuple(0.98 * s for s in o.scale))


def stats(ms):
    return {"mean": round(float(np.mean(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


r = Renderer(0)
r.set_scene_soa(sd.soa, sd.nodes)
r.set_env(*cf.load_env())
r.resize(W, H)
fp = cf.frame_params(W, H)
dev = torch.device("cuda", 0)
poses = [geo.moved_object(sd, a.object, **pose(k)) for k in range(a.calls + 1)]
dposes = [(torch.as_tensor(i, device=dev), torch.as_tensor(p, device=dev), torch.as_tensor(n, device=dev))
          for i, p, n in poses]
torch.cuda.synchronize()


def timed(fn, args_list):
    ms = []
    for args in args_list:
        r.synchronize()
        t0 = time.perf_counter()
        fn(*args)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def render_ms():
    ro = cf.rand_origins(1)
    r.render(fp, ro)  # warm-up
    ms = []
    for _ in range(a.render_calls):
        r.reset()
        r.synchronize()
        t0 = time.perf_counter()
        r.render(fp, ro)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


if a.trace_only:
    for d in dposes[:4]:
        r.update_geometry(*d)
    r.close()
    sys.exit(0)

res = {"config": a.config, "object": o.mesh, "triangles_moved": int(len(poses[0][0])),
       "triangles": sd.counts["n_triangles"], "width": W, "height": H, "calls": a.calls}
res["render_before_ms"] = stats(render_ms())
r.update_geometry(*poses[-1])      # warm-up: builds the refit schedule, allocates the staging
res["update_host_ms"] = stats(timed(r.update_geometry, poses[:a.calls]))
res["update_device_ms"] = stats(timed(r.update_geometry, dposes[:a.calls]))
res["render_after_refit_ms"] = stats(render_ms())
bounds = r.scene_bounds()
res["tri_flagged_after"] = bounds["tri_flagged"]

# the way before: the scene built again on the host with the object in its new pose, and set
objs = list(sd.objects)
build_ms, set_ms = [], []
for k in range(a.rebuilds + 1):
    objs[a.object] = cf.Obj(o.mesh, o.material, pose(a.calls - 1)["rotate"], pose(a.calls - 1)["translate"],
                            pose(a.calls - 1)["scale"], o.smooth)
    t0 = time.perf_counter()
    sd2 = cf.build_scene(objs)
    t1 = time.perf_counter()
    r.set_scene_soa(sd2.soa, sd2.nodes)
    r.synchronize()
    t2 = time.perf_counter()
    if k:  # (the first is the warm-up)
        build_ms.append((t1 - t0) * 1e3)
        set_ms.append((t2 - t1) * 1e3)
res["rebuild_host_scene_ms"] = stats(build_ms)
res["rebuild_set_scene_ms"] = stats(set_ms)
res["render_after_rebuild_ms"] = stats(render_ms())
r.close()
line = json.dumps(res)
print(line)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
