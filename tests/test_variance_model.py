"""The variance mode of the display chain without a GPU: the numpy model of tests/variance_model.py (its
estimators' bias, what it leaves exactly as it was, and that it stops blurring a converged view of the
oracle's own C3 frames) and the boundary of include/rt_abi.h (struct layout, constants, the interactive
loop's calls)."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import denoise_model as dm
import oracle as orc
import temporal_cases as tc
import temporal_model as tm
import variance_model as vm
from conftest import ROOT
from helpers import frames_for
from rtamd import configs as cf
from rtamd import renderer
from rtamd.interactive import Input, Session, Settings
from rtamd.renderer import DenoiseParams, TemporalParams, VarianceParams
from test_denoise_model import H, W, c3  # noqa: F401  (the C3 fixture of the denoiser's tests: 70 x 37)

F = np.float32
D = np.float64
HEADER = ROOT / "include" / "rt_abi.h"
VP = VarianceParams(on=True)
bits = tc.bits


# ------------------------------------------------------------------ estimator bias
# A wall perpendicular to the view, one material: every pixel is a hit with the same guides.  The
# colour is grey, so the luminance is the value (the three weights sum to 1); each sample is
# N(MU, SIGMA^2), independent per pixel and sample.
BW, BH, MU, SIGMA = 64, 48, 2.0, 0.25


def _wall(fp):
    front = np.asarray(fp.front, D)
    return tc.plane("wall", np.asarray(fp.position, D) + 5.0 * front, -front, 3)


def _grey(x):
    return np.repeat(np.asarray(x, F)[..., None], 3, axis=-1)


def test_still_estimator_is_unbiased():
    """A still view seen at S = 1, 2, 3, 5, 9 (uneven chunks): four estimates per pixel, each
    sigma^2 chi^2_1 and independent of the others (Welford's chunk-merge terms of Gaussian samples), so
    the frame mean of v has the standard error sigma^2 sqrt(2 / (pixels x 4)) = 1.28 % of sigma^2 at
    64 x 48; the bound is four of them, 5.1 %."""
    fp = tc.camera(BW, BH, (0.0, 0.0, 1.0))
    hits, which = tc.trace(fp, BW, BH, [_wall(fp)])
    assert (which == 0).all()
    rng = np.random.default_rng(101)
    x = rng.normal(MU, SIGMA, (9, BH, BW))
    t = vm.VarianceTemporal(VP)
    for k, S in enumerate((1, 2, 3, 5, 9)):
        out, n, var = t.call(_grey(x[:S].mean(axis=0)), hits, fp, TemporalParams(samples=S), advance=k == 0)
    st = t.cand.st
    assert (st[..., 3] == 4).all() and (st[..., 1] == 9).all()
    se = np.sqrt(2.0 / (BW * BH * 4))
    rel = float(st[..., 2].astype(D).mean()) / SIGMA ** 2 - 1.0
    print(f"still: mean(v) / sigma^2 - 1 = {rel:+.4f}, bound {4 * se:.4f}")
    assert abs(rel) <= 4 * se
    assert np.array_equal(bits(var), bits(st[..., 2] / np.fmax(n, F(9))))   # the displayed luminance's: v / 9


def test_moving_estimator_is_unbiased():
    """ADVANCE with S = 1 across K = 9 views, each one whole pixel further along right (the taps
    then fetch single texels: a bilinear mix of neighbours would correlate the history's mean with
    nothing but lower its variance below sigma^2 / n_h, and bias e down).  A surface point seen in
    every view gathers K - 1 independent estimates, again Welford's terms; over those pixels the
    standard error of the frame mean of v is sigma^2 sqrt(2 / (pixels x (K - 1))), the bound four of
    them (printed; 3.9 % for the 2688 points seen from all 9 views)."""
    K = 9
    fp0 = tc.camera(BW, BH, (0.0, 0.0, 1.0))
    wall = _wall(fp0)
    px = tc.pixel_size(fp0, BW, 5.0)
    rng = np.random.default_rng(202)
    t = vm.VarianceTemporal(VP)
    for k in range(K):
        fp = tc.moved(fp0, BW, BH, right=k * px)
        hits, which = tc.trace(fp, BW, BH, [wall])
        assert (which == 0).all()
        t.call(_grey(rng.normal(MU, SIGMA, (BH, BW))), hits, fp, TemporalParams(samples=1, max_history=32), advance=True)
    st = t.cand.st
    full = st[..., 3] > K - 1.5
    assert full.sum() >= (BW - K) * BH * 0.95 and np.allclose(st[..., 3][full], K - 1, atol=1e-3)
    se = np.sqrt(2.0 / (full.sum() * (K - 1)))
    rel = float(st[..., 2][full].astype(D).mean()) / SIGMA ** 2 - 1.0
    print(f"moving: mean(v) / sigma^2 - 1 = {rel:+.4f} over {full.sum()} pixels, bound {4 * se:.4f}")
    assert abs(rel) <= 4 * se


# ------------------------------------------------------------------ what the mode leaves as it was
def test_temporal_colours_and_lengths_are_todays(c3):
    """The variance state rides beside the colour: outputs and history lengths of the stage in the mode
    equal tests/temporal_model.py bit for bit, across a camera move, a still second frame and planted
    non-finite pixels."""
    fp1 = cf.frame_params(W, H)
    fp2 = cf.frame_params(W, H, position=tuple(np.asarray(fp1.position, F) + np.asarray(fp1.right, F) * F(0.05)))
    a, b = tm.Temporal(), vm.VarianceTemporal(VP)
    rng = np.random.default_rng(5)
    img = [dm.plant_nonfinite(rng.uniform(0.0, 4.0, (H, W, 3)).astype(F), c3.hit, seed=k)[0] for k in range(3)]
    for k, (fp, S, adv) in enumerate(((fp1, 1, True), (fp2, 1, True), (fp2, 2, False))):
        wo, wn = a.call(img[k], c3.hits, fp, TemporalParams(samples=S), advance=adv)
        go, gn, _ = b.call(img[k], c3.hits, fp, TemporalParams(samples=S), advance=adv)
        assert np.array_equal(bits(go), bits(wo)) and np.array_equal(bits(gn), bits(wn))
    assert b.has.any()


def test_pixels_without_a_variance_keep_the_fixed_filter(c3):
    """With the spatial estimate out of reach every pixel keeps today's colour term: denoise_model bit
    for bit.  The materials are renumbered in an 8 x 8 pattern, so no 7 x 7 neighbourhood holds the
    centre's material twice (cnt = 1: unknown), while the taps of s = 8 and 16 do find it."""
    hits = c3.hits.copy()
    y, x = np.mgrid[0:H, 0:W]
    hits["material"] = (x % 8) + 8 * (y % 8)
    dp = DenoiseParams()
    got, var = vm.denoise(c3.noisy, hits, dp, VP)
    assert (var == -1).all()
    want = dm.denoise(c3.noisy, hits, dp)
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(want), bits(c3.noisy))


def test_constant_frames_come_back_bit_identical(c3):
    ones = np.ones((H, W, 3), F)
    first = c3.hits["material"] == c3.hits["material"][c3.hit][0]
    two = np.where(first[..., None], F(2.0), F(0.5)) * ones
    for img in (ones, two):
        out, var = vm.denoise(img, c3.hits, DenoiseParams(), VP)                       # the spatial estimate: 0
        known = var[c3.hit] >= 0   # (all but the mesh pixels with no second pixel of their surface around them)
        assert np.array_equal(bits(out), bits(img)) and (var[c3.hit][known] == 0).all() and known.mean() > 0.9
        out, _ = vm.denoise(img, c3.hits, DenoiseParams(), VP, np.where(c3.hit, F(0.3), F(-1.0)))   # a temporal one
        assert np.array_equal(bits(out), bits(img))


def test_miss_pass_through_and_nonfinite_filling(c3):
    img, yx = dm.plant_nonfinite(c3.noisy, c3.hit)
    for it in (1, 5):
        out, var = vm.denoise(img, c3.hits, DenoiseParams(iterations=it), VP)
        assert np.array_equal(bits(out)[~c3.hit], bits(img)[~c3.hit]) and (var[~c3.hit] == -1).all()
        assert np.isfinite(out[c3.hit]).all() and (var[c3.hit] >= 0).mean() > 0.9
        assert (var[yx[:, 0], yx[:, 1]] >= 0).sum() >= 10   # (a filled pixel carries its neighbours' variance)


# ------------------------------------------------------------------ the converged view stays sharp
@pytest.fixture(scope="module")
def c3_frames(env_maps):
    """The oracle's C3 at 70 x 37: the still view's accumulations acc_1 .. acc_256 (rand origins from 0),
    the 2048-spp reference (offset 3000) and acc_k at k = 16, 64, 256 from four more offsets."""
    sd = cf.config_scene("C3")
    sc = orc.OracleScene(sd.tri_enc, sd.node_enc, *env_maps)
    fp = cf.frame_params(W, H)
    th = min(16, os.cpu_count() or 1)   # (a frame this small gains nothing from more threads; the results do not depend on it)
    ref, _ = orc.render(sc, frames_for(fp, 1, 2048, ro_offset=3000)[1], W, H, threads=th)
    acc, seq = None, []
    for f in frames_for(fp, 1, 256)[1]:
        acc, _ = orc.render(sc, [f], W, H, accum=acc, threads=min(4, th))
        seq.append(acc)
    others = {k: [orc.render(sc, frames_for(fp, 1, k, ro_offset=off)[1], W, H, threads=th)[0] for off in (6000, 7000, 8000, 9000)]
              for k in (16, 64, 256)}
    return SimpleNamespace(fp=fp, ref=ref, seq=seq, others=others)


def test_a_converged_view_is_not_blurred(c3, c3_frames):
    """A still view from an empty history, acc_1, acc_2, ... fed tick by tick through
    temporal(variance) -> denoise(variance), both at their defaults; mse(x / (1 + x)) over the hit
    pixels against the 2048-spp reference, as test_it_denoises measures it.

    At k = 16, 64, 256 the filtered error may exceed the input's by no more than the run-to-run spread
    of the input error, the standard deviation (n - 1) of that error over four other rand-origin
    offsets; at k = 1, where only the spatial estimate exists, filtered <= 0.5 x input.  Measured:

        k     input mse   spread     variance mode  ratio    fixed sigma_color  ratio
        1     0.025826    -          0.010247       0.397    0.009083           0.352
        4     0.008273    -          0.004937       0.597    0.005164           0.624
        16    0.002404    0.000122   0.001812       0.754    0.003355           1.396
        64    0.000602    0.000045   0.000555       0.922    0.002938           4.881
        256   0.000193    0.000006   0.000189       0.981    0.002941           15.26
    """
    f = c3_frames

    def err(img):
        a, b = img[c3.hit].astype(D), f.ref[c3.hit].astype(D)
        return float(np.mean((a / (1 + a) - b / (1 + b)) ** 2))

    t = vm.VarianceTemporal(VP)
    rows = {}
    for k in range(1, 257):
        out, n, var = t.call(f.seq[k - 1], c3.hits, f.fp, TemporalParams(samples=k), advance=k == 1)
        if k in (1, 4, 16, 64, 256):
            assert np.array_equal(bits(out), bits(f.seq[k - 1]))   # (no history: the display is the accumulation)
            got, _ = vm.denoise(out, c3.hits, DenoiseParams(), VP, var)
            fixed = dm.denoise(out, c3.hits, DenoiseParams())
            spread = float(np.std([err(o) for o in f.others[k]], ddof=1)) if k in f.others else float("nan")
            rows[k] = (err(out), spread, err(got), err(fixed))
            e_in, sp, e_var, e_fix = rows[k]
            print(f"k {k:3d}  input {e_in:.6f}  spread {sp:.6f}  variance mode {e_var:.6f} ratio {e_var / e_in:.3f}"
                  f"  fixed {e_fix:.6f} ratio {e_fix / e_in:.3f}")
    assert (var[c3.hit] >= 0).all()
    assert rows[1][2] <= 0.5 * rows[1][0], rows[1]
    for k in (16, 64, 256):
        e_in, sp, e_var, _ = rows[k]
        assert e_var <= e_in + sp, (k, rows[k])


# ------------------------------------------------------------------ ABI
def test_variance_params_match_header(tmp_path):
    """rt_variance_params: size and offsets from gcc on the header equal the ctypes struct's; the
    structs beside it keep their 20 bytes."""
    ct = renderer.RtVarianceParams
    lines = ['printf("%zu %zu %zu\\n", sizeof(rt_variance_params), sizeof(rt_denoise_params), sizeof(rt_temporal_params));']
    lines += [f'printf("%zu\\n", offsetof(rt_variance_params, {f}));' for f, _ in ct._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void) {\n  ' +
                   "\n  ".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [16, 20, 20] and C.sizeof(ct) == 16
    assert out[3:] == [getattr(ct, f).offset for f, _ in ct._fields_]
    assert [f for f, _ in ct._fields_] == ["on", "sigma_lum", "max_estimates", "flags"]
    d = VarianceParams()
    assert (d.on, d.sigma_lum, d.max_estimates, d.flags) == (False, 1.5, 64, 0)
    c = VarianceParams(on=True, sigma_lum=2.0).to_c()
    assert (c.on, c.sigma_lum, c.max_estimates, c.flags) == (1, 2.0, 64, 0)


def test_variance_constants_match_header():
    text = HEADER.read_text()
    assert re.search(r"^#define RT_HAS_VARIANCE 1$", text, re.M) and renderer.RT_HAS_VARIANCE == 1
    assert re.search(r"^#define RT_ABI_VERSION 7$", text, re.M)
    for name in ("rt_variance_default_params", "rt_variance_set", "rt_variance_get", "rt_variance_frame"):
        assert name in renderer.ABI_SYMBOLS and re.search(rf"^int {name}\(", text, re.M)
    # no enumerator joined the two stages' sets, none was made for the mode
    assert set(re.findall(r"\b(RT_(?:DENOISE|TEMPORAL|VARIANCE)_[A-Z_]+)\s*=", text)) == {
        "RT_DENOISE_REUSE_GUIDES", "RT_TEMPORAL_ADVANCE", "RT_TEMPORAL_REUSE_GUIDES", "RT_TEMPORAL_RESET"}
    assert "variance estimation," not in text   # (no longer out of scope)


def test_variance_layout():
    """dvl::Variance through rts_dev_layout: two 16-byte state frames and three float frames, each on
    a 256-byte boundary, none overlapping, 44 bytes per pixel before the rounding."""
    from rtamd import scene_lib as sl
    for npx in (1, 33 * 17, 70 * 37, 1920 * 1080):
        scalars, spans = sl.dev_layout("variance", npx)
        assert [s["name"] for s in spans] == ["st0", "st1", "tvar", "dvar0", "dvar1"]
        assert [s["bytes"] for s in spans] == [16 * npx, 16 * npx, 4 * npx, 4 * npx, 4 * npx]
        at = 0
        for s in spans:
            assert s["off"] % 256 == 0 and s["off"] >= at and s["host"] == -1
            at = s["off"] + s["bytes"]
        assert at <= scalars[0] <= 44 * npx + 5 * 255


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
        self.calls.append(("render",))
        return {}

    def set_variance(self, on):
        self.calls.append(("set_variance", on))

    def temporal_async(self, fp, tp=None, frame_ptr=None, hits_ptr=None, advance=False, reuse_guides=False, reset=False):
        self.calls.append(("temporal_async", advance, reuse_guides))
        return 0x7000

    def denoise_async(self, fp, dp=None, frame_ptr=None, hits_ptr=None, reuse_guides=False):
        self.calls.append(("denoise_async", frame_ptr, reuse_guides))
        return 0xD000

    def tonemap(self, flags, frame_ptr=None):
        self.calls.append(("tonemap", frame_ptr))
        return np.zeros((1, 1, 3), np.uint8)


class StubWithoutTheMode(StubRenderer):
    set_variance = None   # (a renderer of before the mode: calling it would raise)


def test_session_sets_the_mode_once_and_keeps_todays_calls_without_it():
    chain = [("render",), ("temporal_async", False, True), ("denoise_async", 0x7000, True), ("tonemap", 0xD000)]
    first = [("render",), ("temporal_async", True, False), ("denoise_async", 0x7000, True), ("tonemap", 0xD000)]
    # off (the default): today's calls, and nothing of the mode is asked of the renderer
    r = StubWithoutTheMode()
    s = Session(r, 64, 36, settings=Settings(enable_temporal=True, enable_denoise=True))
    assert Settings().enable_variance is False
    seen = []
    for _ in range(2):
        r.calls.clear()
        s.tick(Input(), delta_time=0.05)
        seen.append(list(r.calls))
    assert seen == [first, chain]
    # on: one set_variance(True) before the frame, the history starts again (ADVANCE), the guides stay
    r = StubRenderer()
    s = Session(r, 64, 36, settings=Settings(enable_temporal=True, enable_denoise=True, enable_variance=True))
    seen = []
    for inp in (Input(), Input(), Input(gui={"enable_variance": False}), Input()):
        r.calls.clear()
        s.tick(inp, delta_time=0.05)
        seen.append(list(r.calls))
    assert seen[0] == [("set_variance", True)] + first and seen[1] == chain
    assert seen[2] == [("set_variance", False), ("render",), ("temporal_async", True, True)] + chain[2:] and seen[3] == chain
    assert "enable_variance" not in __import__("rtamd.interactive").interactive.RESETTING
