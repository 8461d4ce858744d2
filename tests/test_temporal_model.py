"""The temporal stage of the displayed frame without a GPU: the numpy model of tests/temporal_model.py
against float64 analytic answers on the synthetic first-hit frames of tests/temporal_cases.py, and the
boundary of include/rt_abi.h (struct layout, constants, the interactive loop's calls)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import temporal_cases as tc
import temporal_model as tm
from conftest import ROOT
from rtamd import interactive, renderer
from rtamd.interactive import Input, Session, Settings
from rtamd.renderer import TemporalParams

HEADER = ROOT / "include" / "rt_abi.h"
SIZES = list(tc.SIZES)


@pytest.fixture
def run():
    return tm.Temporal().call


@pytest.mark.parametrize("basis", ["axis", "turned"])
@pytest.mark.parametrize("size", SIZES)
def test_world_linear_colour_on_a_camera_parallel_plane(run, size, basis):
    tc.case_linear_plane(size, run, basis)


@pytest.mark.parametrize("variant", ["material", "plane"])
@pytest.mark.parametrize("size", SIZES)
def test_exactly_the_revealed_pixels_start_again(run, size, variant):
    tc.case_disocclusion(size, run, variant)


@pytest.mark.parametrize("size", SIZES)
def test_a_tilted_neighbour_is_rejected_by_its_normal(run, size):
    tc.case_tilted_neighbour(size, run)


@pytest.mark.parametrize("size", SIZES)
def test_sample_count_bookkeeping(run, size):
    tc.case_bookkeeping(size, run)


@pytest.mark.parametrize("size", SIZES)
def test_pass_through_and_fallback(run, size):
    tc.case_passthrough(size, run)


def test_another_size_or_a_drop_leaves_no_history():
    t = tm.Temporal()
    W, H, fp, hits, hit = tc._still_scene("64x36")
    c = np.random.default_rng(1).uniform(0, 2, (H, W, 3)).astype(np.float32)
    t.call(c, hits, fp, tc.TP(), advance=True)
    t.drop()
    out, n = t.call(c * 2, hits, fp, tc.TP(), advance=True)
    assert np.array_equal(out, c * 2) and (n[hit] == 1).all() and not t.has.any()
    out, n = t.call(c, hits, fp, tc.TP(), advance=True)
    assert t.has[hit].all() and (n[hit] == 2).all()


# ------------------------------------------------------------------ ABI
def test_temporal_params_match_header(tmp_path):
    """rt_temporal_params: size and offsets from gcc on the header equal the ctypes struct's."""
    ct = renderer.RtTemporalParams
    lines = ['printf("%zu\\n", sizeof(rt_temporal_params));']
    lines += [f'printf("%zu\\n", offsetof(rt_temporal_params, {f}));' for f, _ in ct._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void) {\n  ' +
                   "\n  ".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out.pop(0) == 20 == C.sizeof(ct)
    assert out == [getattr(ct, f).offset for f, _ in ct._fields_]
    assert [f for f, _ in ct._fields_] == ["samples", "max_history", "sigma_normal", "sigma_plane", "flags"]
    d = TemporalParams()
    assert (d.samples, d.max_history, d.sigma_normal, d.sigma_plane, d.flags) == (1, 32, 0.3, 0.01, 0)
    c = TemporalParams(samples=3).to_c(renderer.RT_TEMPORAL_ADVANCE | renderer.RT_TEMPORAL_RESET)
    assert (c.samples, c.flags) == (3, 5)


def test_temporal_constants_match_header():
    text = HEADER.read_text()
    enums = {k: int(v) for k, v in re.findall(r"\b(RT_TEMPORAL_\w+)\s*=\s*(-?\d+)", text)}
    assert enums == {"RT_TEMPORAL_ADVANCE": 1, "RT_TEMPORAL_REUSE_GUIDES": 2, "RT_TEMPORAL_RESET": 4}
    assert enums == {k: getattr(renderer, k) for k in dir(renderer) if k.startswith("RT_TEMPORAL_")}
    assert re.search(r"^#define RT_HAS_TEMPORAL 1$", text, re.M) and renderer.RT_HAS_TEMPORAL == 1
    assert re.search(r"^#define RT_ABI_VERSION 7$", text, re.M)
    for name in ("rt_temporal_default_params", "rt_temporal_async", "rt_temporal", "rt_temporal_history"):
        assert name in renderer.ABI_SYMBOLS
    lib = C.CDLL(str(ROOT / "opengl-ray-tracing-framework_amd" / "lib" / "librtamd.so"))
    d = renderer.RtTemporalParams()
    lib.rt_temporal_default_params.argtypes = [C.POINTER(renderer.RtTemporalParams)]
    assert lib.rt_temporal_default_params(C.byref(d)) == 0 and lib.rt_temporal_default_params(None) == renderer.RT_ERR_ARG
    assert (d.samples, d.max_history, d.sigma_normal, d.sigma_plane, d.flags) == (1, 32, np.float32(0.3), np.float32(0.01), 0)


class StubRenderer:
    """Records what the loop asks of a renderer, in order (no device)."""

    def __init__(self):
        self.calls = []
        self.loop_num = 0

    def resize(self, w, h, **_):
        self.calls.append(("resize", w, h))

    def reset(self):
        self.loop_num = 0
        self.calls.append(("reset",))

    def render(self, fp, ro):
        self.loop_num += 1
        self.calls.append(("render", fp))
        return {}

    def temporal_async(self, fp, tp=None, frame_ptr=None, hits_ptr=None, advance=False, reuse_guides=False, reset=False):
        self.calls.append(("temporal_async", fp, tp.samples, advance, reuse_guides, reset, frame_ptr))
        return 0x7000

    def denoise_async(self, fp, dp=None, frame_ptr=None, hits_ptr=None, reuse_guides=False):
        self.calls.append(("denoise_async", fp, reuse_guides, frame_ptr))
        return 0xD000

    def tonemap(self, flags, frame_ptr=None):
        self.calls.append(("tonemap", flags, frame_ptr))
        return np.zeros((1, 1, 3), np.uint8)


@pytest.mark.parametrize("denoise", [False, True])
def test_session_runs_the_temporal_stage_before_the_display(denoise):
    """enable_temporal: render, temporal_async(samples = LoopNum, ADVANCE on the first display after a
    reset, the guides reused while nothing reset the accumulation), then the denoiser on its output
    with REUSE_GUIDES when both are on, then the display pass on the last output."""
    r = StubRenderer()
    s = Session(r, 64, 36, settings=Settings(enable_temporal=True, enable_denoise=denoise))
    seen = []
    for inp in (Input(), Input(), Input(keys=["w"]), Input(), Input(resize=(48, 40)), Input()):
        r.calls.clear()
        out = s.tick(inp, delta_time=0.05)
        names = [c[0] for c in r.calls if c[0] not in ("reset", "resize")]
        assert names == ["render", "temporal_async"] + (["denoise_async"] if denoise else []) + ["tonemap"]
        t = next(c for c in r.calls if c[0] == "temporal_async")
        assert t[1] is out["params"] and t[2] == out["loop_num"] and t[5] is False and t[6] is None
        seen.append((t[2], t[3], t[4]))
        if denoise:
            d = next(c for c in r.calls if c[0] == "denoise_async")
            assert d[1] is out["params"] and d[2] is True and d[3] == 0x7000
        assert r.calls[-1] == ("tonemap", out["display_flags"], 0xD000 if denoise else 0x7000)
    #               samples, advance, reuse_guides
    assert seen == [(1, True, False), (2, False, True), (1, True, False), (2, False, True), (1, True, False),
                    (2, False, True)]
    # a tick that is not displayed makes no temporal call, and the next displayed one still advances
    r.calls.clear()
    s.tick(Input(keys=["a"]), delta_time=0.05, display=False)
    assert [c[0] for c in r.calls] == ["reset", "render"]
    r.calls.clear()
    s.tick(Input(), delta_time=0.05)
    t = next(c for c in r.calls if c[0] == "temporal_async")
    assert (t[2], t[3], t[4]) == (2, True, False)
    assert "enable_temporal" not in interactive.RESETTING
    # the setting off: today's calls
    r.calls.clear()
    s.tick(Input(gui={"enable_temporal": False, "enable_denoise": False}), delta_time=0.05)
    assert [c[:1] + c[2:] if c[0] == "render" else c for c in r.calls] == [("render",), ("tonemap", 3, None)]
