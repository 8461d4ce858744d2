"""The display denoiser without a GPU: the numpy model of tests/denoise_model.py (its exp_ against the
oracle's, the exactness properties of the filter, non-finite input, and that it denoises the
oracle's own 1-spp frame), and the boundary of include/rt_abi.h (struct layout, constants, the
interactive loop's calls)."""
import ctypes as C
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import denoise_model as dm
import oracle as orc
import query_cases as qc
from conftest import ROOT
from helpers import frames_for
from rtamd import configs as cf
from rtamd import renderer
from rtamd.interactive import Input, Session, Settings
from rtamd.renderer import HIT_DTYPE, DenoiseParams
from test_gpu_query import _camera_rays_numpy

F = np.float32
HEADER = ROOT / "include" / "rt_abi.h"
W, H = 70, 37


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------ exp_
def test_numpy_exp_is_the_oracles():
    """denoise_model.exp_ equals gm::exp_ (orc_math(4, x)) bit for bit over -110 .. 5 and at the
    branch points of its range reduction."""
    xs = np.concatenate([np.linspace(-110.0, 5.0, 4501), [0.0, -0.0, -87.3, -88.0, -95.0, -103.9, -104.0, 88.8]]).astype(F)
    L = orc.lib()
    ref = np.array([L.orc_math(4, float(x), 0.0) for x in xs], F)
    got = dm.exp_(xs)
    bad = np.flatnonzero(bits(got) != bits(ref))
    assert len(xs) >= 4000 and bad.size == 0, (bad.size, xs[bad[:8]], got[bad[:8]], ref[bad[:8]])


# ------------------------------------------------------------------ C3's guides and frames
@pytest.fixture(scope="module")
def c3(env_maps):
    """C3 at 70 x 37: the first-hit frame from orc_trace on the numpy camera rays (materials: the
    floor's id on the floor's plane, the mesh's elsewhere), the oracle's 1-spp frame and its
    128-spp frame (rand origins offset by 1).  Read-only."""
    sd = cf.config_scene("C3")
    sc = orc.OracleScene(sd.tri_enc, sd.node_enc, *env_maps)
    fp = cf.frame_params(W, H)
    d = _camera_rays_numpy(fp, W, H).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(fp.position, F), d.shape)
    hits = qc.oracle_hits(sc, o, d).reshape(H, W)
    mid = np.asarray(sd.soa["material_id"])
    plane = (sd.tri_enc[:, 6:14].reshape(len(sd.tri_enc), 24) == cf.MATERIALS["plane"].texels()[None]).all(axis=1)
    floor_y = sd.tri_enc[plane, 0:3, 1]
    assert plane.any() and not plane.all() and floor_y.min() == floor_y.max()
    on_floor = np.abs(hits["point"][..., 1] - floor_y.flat[0]) <= 1e-4
    hits["material"] = np.where(hits["triangle"] >= 0, np.where(on_floor, mid[plane][0], mid[~plane][0]), 0)
    ro, frames = frames_for(fp, 1, 1)
    noisy, _ = orc.render(sc, frames, W, H)
    ro, frames = frames_for(fp, 1, 128, ro_offset=1)
    clean, _ = orc.render(sc, frames, W, H)
    for a in (hits, noisy, clean):
        a.flags.writeable = False
    return SimpleNamespace(hits=hits, hit=hits["triangle"] >= 0, noisy=noisy, clean=clean)


def test_c3_guides_have_both_materials_and_misses(c3):
    m = c3.hits["material"][c3.hit]
    assert len(np.unique(m)) == 2 and 0.3 < c3.hit.mean() < 1.0


def test_constant_frames_come_back_bit_identical(c3):
    """An all-1.0 frame, and 2.0 on one material and 0.5 on the other: every weight sum is an
    exact multiple of the value, so sum / sw is the value itself."""
    ones = np.ones((H, W, 3), F)
    assert np.array_equal(bits(dm.denoise(ones, c3.hits, DenoiseParams())), bits(ones))
    first = c3.hits["material"] == c3.hits["material"][c3.hit][0]
    two = np.where(first[..., None], F(2.0), F(0.5)) * np.ones((H, W, 3), F)
    assert np.array_equal(bits(dm.denoise(two, c3.hits, DenoiseParams())), bits(two))


def test_miss_pixels_pass_through(c3):
    rng = np.random.default_rng(11)
    img = rng.uniform(0.0, 4.0, (H, W, 3)).astype(F)
    out = dm.denoise(img, c3.hits, DenoiseParams())
    assert np.array_equal(bits(out)[~c3.hit], bits(img)[~c3.hit])
    assert not np.array_equal(bits(out)[c3.hit], bits(img)[c3.hit])


@pytest.mark.parametrize("iterations", [1, 5])
def test_nonfinite_pixels_are_filled(c3, iterations):
    """12 planted NaN / inf pixels are never a source and are filled from their neighbours."""
    img, yx = dm.plant_nonfinite(c3.noisy, c3.hit)
    assert (~np.isfinite(img).all(-1)).sum() == 12
    out = dm.denoise(img, c3.hits, DenoiseParams(iterations=iterations))
    assert np.isfinite(out[c3.hit]).all()


def test_it_denoises(c3):
    """mse(x / (1 + x)) over the hit pixels against the 128-spp frame: the filtered 1-spp frame's is
    at most half the noisy frame's (measured with the prototype: ratio 0.36)."""
    out = dm.denoise(c3.noisy, c3.hits, DenoiseParams())

    def err(img):
        a, b = img[c3.hit].astype(np.float64), c3.clean[c3.hit].astype(np.float64)
        return float(np.mean((a / (1 + a) - b / (1 + b)) ** 2))

    e_noisy, e_out = err(c3.noisy), err(out)
    print(f"mse noisy {e_noisy:.5f} filtered {e_out:.5f} ratio {e_out / e_noisy:.3f}")
    assert e_out <= 0.5 * e_noisy, (e_out, e_noisy)


# ------------------------------------------------------------------ ABI
def test_denoise_params_match_header(tmp_path):
    """rt_denoise_params: size and offsets from gcc on the header equal the ctypes struct's."""
    ct = renderer.RtDenoiseParams
    lines = ['printf("%zu\\n", sizeof(rt_denoise_params));']
    lines += [f'printf("%zu\\n", offsetof(rt_denoise_params, {f}));' for f, _ in ct._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void) {\n  ' +
                   "\n  ".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out.pop(0) == 20 == C.sizeof(ct)
    assert out == [getattr(ct, f).offset for f, _ in ct._fields_]
    assert [f for f, _ in ct._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_plane", "flags"]
    d = DenoiseParams()
    assert (d.iterations, d.sigma_color, d.sigma_normal, d.sigma_plane, d.flags) == (5, 1.0, 0.3, 0.01, 0)
    c = DenoiseParams(iterations=3).to_c(renderer.RT_DENOISE_REUSE_GUIDES)
    assert (c.iterations, c.flags) == (3, 1)


def test_denoise_constants_match_header():
    text = HEADER.read_text()
    enums = {k: int(v) for k, v in re.findall(r"\b(RT_DENOISE_\w+)\s*=\s*(-?\d+)", text)}
    assert enums == {"RT_DENOISE_REUSE_GUIDES": 1}
    assert enums == {k: getattr(renderer, k) for k in dir(renderer) if k.startswith("RT_DENOISE_")}
    assert re.search(r"^#define RT_HAS_DENOISE 1$", text, re.M) and renderer.RT_HAS_DENOISE == 1
    assert re.search(r"^#define RT_ABI_VERSION 7$", text, re.M)
    for name in ("rt_denoise_default_params", "rt_denoise_async", "rt_denoise"):
        assert name in renderer.ABI_SYMBOLS


class StubRenderer:
    """Records what the loop asks of a renderer, in order (no device)."""

    loop_num = 1

    def __init__(self):
        self.calls = []

    def resize(self, w, h, **_):
        self.calls.append(("resize", w, h))

    def reset(self):
        self.calls.append(("reset",))

    def render(self, fp, ro):
        self.calls.append(("render", fp))
        return {}

    def denoise_async(self, fp, dp=None, frame_ptr=None, hits_ptr=None, reuse_guides=False):
        self.calls.append(("denoise_async", fp, reuse_guides))
        return 0xD000

    def tonemap(self, flags, frame_ptr=None):
        self.calls.append(("tonemap", flags, frame_ptr))
        return np.zeros((1, 1, 3), np.uint8)


def test_session_denoises_before_the_display_pass():
    """enable_denoise: render, denoise_async, tonemap(flags, frame_ptr=<the returned pointer>);
    the guides are reused exactly while nothing has reset the accumulation."""
    r = StubRenderer()
    s = Session(r, 64, 36, settings=Settings(enable_denoise=True))
    reuse = []
    for inp in (Input(), Input(), Input(keys=["w"]), Input(), Input(resize=(48, 40)), Input()):
        r.calls.clear()
        out = s.tick(inp, delta_time=0.05)
        names = [c[0] for c in r.calls if c[0] not in ("reset", "resize")]
        assert names == ["render", "denoise_async", "tonemap"]
        dn = next(c for c in r.calls if c[0] == "denoise_async")
        assert dn[1] is out["params"]
        assert r.calls[-1] == ("tonemap", out["display_flags"], 0xD000)
        reuse.append(dn[2])
    assert reuse == [False, True, False, True, False, True]
    # not displayed: no denoise either; the setting off: today's calls
    r.calls.clear()
    s.tick(Input(), delta_time=0.05, display=False)
    assert [c[0] for c in r.calls] == ["render"]
    assert "enable_denoise" not in __import__("rtamd.interactive").interactive.RESETTING
    r.calls.clear()
    s.tick(Input(gui={"enable_denoise": False}), delta_time=0.05)
    assert [c[:1] + c[2:] if c[0] == "render" else c for c in r.calls] == [("render",), ("tonemap", 3, None)]
