#!/usr/bin/env python3
"""Pick-and-edit demo (needs a GPU): render C3, pick the centre pixel (or the nearest one that
sees the scene) through the interactive loop, recolour the picked triangle's material range,
render again and save both images.

    python tools/pick_demo.py [--width 640 --height 360 --frames 32 --out /tmp/pick]
"""
import argparse
import dataclasses
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "opengl-ray-tracing-framework_amd"))

from rtamd import configs as cf  # noqa: E402
from rtamd.interactive import Input, Session  # noqa: E402
from rtamd.renderer import Renderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--height", type=int, default=360)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--out", default="pick_demo")
a = ap.parse_args()

sd = cf.config_scene("C3")
r = Renderer(0)
r.set_scene_soa(sd.soa, sd.nodes)
r.set_env(*cf.load_env())
s = Session(r, a.width, a.height)


def save(name, img):
    try:
        from PIL import Image
        Image.fromarray(img).save(f"{a.out}_{name}.png")
    except ImportError:
        np.save(f"{a.out}_{name}.npy", img)


for _ in range(a.frames - 1):
    s.tick(display=False)
# the centre pixel, or the pixel nearest to it that sees the scene (first-hit frame, row 0 = bottom)
fh = r.first_hit(s.frame_params())
ys, xs = np.nonzero(fh["triangle"] >= 0)
if not len(xs):
    sys.exit("no pixel sees the scene")
k = np.argmin((xs - a.width // 2) ** 2 + (ys - (a.height - 1 - a.height // 2)) ** 2)
out = s.tick(Input(pick=(xs[k] + 0.5, a.height - 1 - ys[k] + 0.5)))  # window coordinates: origin top-left
save("before", out["image"])
p = out["pick"]
print(f"pixel {p['pixel']}: triangle {p['triangle']}, material {p['material_id']}, t {p['t']:.4f}, point {p['point']}")
# the contiguous range of (post-BVH) triangles around the picked one that share its material
lo = hi = p["triangle"]
while lo > 0 and r.triangle_material(lo - 1)[1] == p["material_id"]:
    lo -= 1
while hi + 1 < len(sd.tri_enc) and r.triangle_material(hi + 1)[1] == p["material_id"]:
    hi += 1
red = dataclasses.replace(p["material"], base_color=(0.9, 0.1, 0.1))
print(f"recolouring triangles [{lo}, {hi}]")
out = s.tick(Input(materials=[(lo, hi - lo + 1, red)]))
for _ in range(a.frames - 1):
    out = s.tick(display=False)
save("after", s.tick()["image"])
r.close()
