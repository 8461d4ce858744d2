"""The ray-query boundary of include/rt_abi.h (ABI 7) without a GPU: record layouts and constants
against the header itself, and the interactive loop's cursor-to-pixel mapping."""
import ctypes as C
import re
import subprocess

import numpy as np

from conftest import ROOT
from rtamd import renderer
from rtamd import scene_lib as sl
from rtamd.interactive import Input, Session

HEADER = ROOT / "include" / "rt_abi.h"


def test_query_records_match_header(tmp_path):
    """rt_ray is 24 bytes and rt_hit 48, every field sits where the ctypes structs and the numpy
    dtypes put it (sizes and offsets from gcc on the header), and the header's ABI version is 7,
    the binding's."""
    structs = [("rt_ray", renderer.RtRay, renderer.RAY_DTYPE), ("rt_hit", renderer.RtHit, renderer.HIT_DTYPE)]
    lines = ['printf("%d\\n", RT_ABI_VERSION);']
    for name, ct, _ in structs:
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        lines += [f'printf("%zu\\n", offsetof({name}, {f}));' for f, _ in ct._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void) {\n  ' +
                   "\n  ".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out.pop(0) == 7 == renderer.RT_ABI_VERSION
    for (name, ct, dt), size in zip(structs, (24, 48)):
        assert out.pop(0) == size == C.sizeof(ct) == dt.itemsize, name
        for f, _ in ct._fields_:
            assert out.pop(0) == getattr(ct, f).offset == dt.fields[f][1], (name, f)
    assert not out


def test_query_constants_match_header():
    """RT_HIT_INVALID, RT_QUERY_CLOSEST / ANY and RT_QUERY_NO_CULL have the header's values."""
    text = HEADER.read_text()
    header = {k: int(v) for k, v in re.findall(r"\b(RT_HIT_INVALID|RT_QUERY_\w+)\s*=\s*(-?\d+)", text)}
    assert header == {"RT_HIT_INVALID": -2, "RT_QUERY_CLOSEST": 0, "RT_QUERY_ANY": 1, "RT_QUERY_NO_CULL": 1}
    assert header == {k: getattr(renderer, k) for k in dir(renderer) if k.startswith(("RT_HIT_", "RT_QUERY_"))}


def test_header_documents_every_query_entry_point():
    """Each new entry point is declared under a comment that names the reference lines it stands for."""
    text = HEADER.read_text()
    for fn in ("rt_trace_rays", "rt_trace_rays_device", "rt_camera_rays", "rt_first_hit", "rt_first_hit_device",
               "rt_pick", "rt_get_triangle_material"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + fn + r"\(", text, re.S)
        assert m and re.search(r"RT:\d+", m.group(1)), fn


def test_material_round_trips_through_its_texels():
    """sl.Material.from_texels inverts texels(): what rt_get_triangle_material returns becomes the
    Material an editor shows and feeds back to rt_update_materials."""
    m = sl.Material(emissive=(0.25, 0.55, 1.05), base_color=(0.1, 0.2, 0.3), subsurface=0.4, metallic=0.5, specular=0.6,
                    specular_tint=0.7, roughness=0.8, anisotropic=0.9, sheen=1.0, sheen_tint=1.1, clearcoat=1.2,
                    clearcoat_gloss=1.3, ior=1.4, transmission=1.5, medium_color=(1.6, 1.7, 1.8), medium_type=2.0,
                    medium_density=1.9, medium_anisotropy=-0.5)
    t = m.texels()
    assert len(set(t.tolist())) == 24
    assert np.array_equal(sl.Material.from_texels(t).texels(), t)


class PickRenderer:
    """Records what the loop asks of a renderer, in order (no device)."""

    def __init__(self):
        self.calls = []

    def resize(self, w, h, **_):
        self.calls.append(("resize", w, h))

    def reset(self):
        self.calls.append(("reset",))

    def render(self, fp, ro):
        self.calls.append(("render", fp))
        return {}

    loop_num = 1

    def tonemap(self, flags):
        return np.zeros((1, 1, 3), np.uint8)

    def pick(self, fp, px, py):
        self.calls.append(("pick", fp, px, py))
        h = np.zeros((), renderer.HIT_DTYPE)
        h["t"], h["point"], h["normal"], h["triangle"], h["material"] = 2.5, (1, 2, 3), (0, 1, 0), 7, 1
        return h

    def triangle_material(self, tri):
        self.calls.append(("triangle_material", tri))
        return sl.Material(base_color=(0.25, 0.5, 0.75), roughness=0.125).texels(), 1


def test_input_has_pick():
    assert Input().pick is None
    assert Input(pick=(3.0, 4.0)).pick == (3.0, 4.0)


def test_session_maps_the_cursor_to_the_accumulations_pixel():
    """Window coordinates have their origin top-left (GLFW), the accumulation row 0 at the bottom:
    px = floor(x), py = height - 1 - floor(y).  The pick uses the frame's own uniforms and comes
    before the frame is queued; a tick without `pick` asks the renderer for none."""
    W, H = 64, 36
    r = PickRenderer()
    s = Session(r, W, H)
    for (x, y), pixel in (((0, 0), (0, H - 1)), ((W - 0.5, H - 0.5), (W - 1, 0)), ((10.75, 3.25), (10, H - 4))):
        r.calls.clear()
        out = s.tick(Input(pick=(x, y)))
        names = [c[0] for c in r.calls]
        assert names.index("pick") < names.index("render")
        pick = next(c for c in r.calls if c[0] == "pick")
        assert pick[2:] == pixel
        assert pick[1] is out["params"] is next(c for c in r.calls if c[0] == "render")[1]
        p = out["pick"]
        assert p["pixel"] == pixel and p["triangle"] == 7 and p["material_id"] == 1 and p["t"] == 2.5
        assert np.array_equal(p["point"], np.array((1, 2, 3), np.float32)) and np.array_equal(p["normal"], (0, 1, 0))
        assert p["material"] == sl.Material.from_texels(sl.Material(base_color=(0.25, 0.5, 0.75), roughness=0.125).texels())
    r.calls.clear()
    out = s.tick(Input())
    assert "pick" not in out and [c[0] for c in r.calls] == ["render"]
