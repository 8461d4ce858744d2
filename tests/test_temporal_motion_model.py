"""The motion mode of the temporal stage without a GPU: the numpy model of
tests/temporal_motion_model.py on the triangle scenes of tests/temporal_motion_cases.py against their
float64 analytic answers, the layouts of the mode's device buffers (csrc/common/dev_layout.h) and the
boundary of include/rt_abi.h."""
import re

import numpy as np
import pytest

import temporal_motion_cases as mc
from conftest import ROOT
from rtamd import interactive, renderer
from rtamd import scene_lib as sl

SIZES = list(mc.SIZES)


@pytest.mark.parametrize("case", list(mc.CASES))
@pytest.mark.parametrize("size", SIZES)
def test_cases_on_the_model(size, case):
    mc.CASES[case](size, mc.ModelStage(True), mc.ModelStage(False))


def test_translation_bound_is_twice_the_measured_worst():
    """The worst error of the fp32 model against the float64 geometry over the translation case's
    inputs is what temporal_motion_cases.py states (rounded up to two digits), and the bound twice it."""
    worst = max(mc.case_translation(s, mc.ModelStage(True), mc.ModelStage(False), moves) for s in SIZES for moves in (False, True))
    assert 0.5 * mc.TRANSLATION_WORST < worst <= mc.TRANSLATION_WORST
    assert mc.TRANSLATION_BOUND == 2.0 * mc.TRANSLATION_WORST


def test_a_failed_require_means_no_history():
    """A degenerate current triangle (den = 0) and a history pose whose normals are zero (l = 0): the moved
    pixels start again, out == c and n = min(S, max_history)."""
    W, H, _ = mc.SIZES["64x36"]
    scene = mc.CaseScene()
    fp = mc.still_camera(W, H)
    for what in ("den", "l"):
        st = mc.ModelStage(True)
        st.load(scene)
        h = st.first_hit(fp, W, H)
        card = mc.on_card(scene, h)
        p, n = scene.p[scene.card].copy(), scene.n[scene.card].copy()
        if what == "l":
            st.update(scene.card, p, np.zeros_like(n))   # the history's pose: vertex normals that interpolate to zero
        st.call(mc.colours(H, W, 1), h, fp, mc.TP(), advance=True, reset=True)
        if what == "den":
            p[:, 2] = p[:, 1]                    # p3 = p2: e1 = e2, den = 0
            st.update(scene.card, p, n)
        else:
            st.update(scene.card, *scene.card_moved((0.01, 0.0, 0.0)))
        c = mc.colours(H, W, 2)
        out, cnt = st.call(c, h, fp, mc.TP(samples=3), advance=True)
        assert st.model.moved[card].all() and st.model.failed[card].all() and not st.model.moved[~card].any()
        assert np.array_equal(mc.bits(out)[card], mc.bits(c)[card]) and (cnt[card] == 3).all()
        assert (cnt[~card] == 4).all()


# ------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("n_tri", [0, 1, 4, 100000, 5_000_001])
def test_pose_layout(n_tri):
    sc, spans = sl.dev_layout("poses", n_tri)
    assert [s["name"] for s in spans] == ["tri0", "trin0", "tri1", "trin1"]
    check_spans(sc, spans, 48 * n_tri)


@pytest.mark.parametrize("npx", [1, 70 * 37, 64 * 36, 1920 * 1080])
def test_triangle_frame_layout(npx):
    sc, spans = sl.dev_layout("tri_frames", npx)
    assert [s["name"] for s in spans] == ["tf0", "tf1", "tf2"]
    check_spans(sc, spans, 4 * npx)


def check_spans(sc, spans, size):
    """Every span holds `size` bytes of its own, starts on a 16-byte boundary, overlaps no other and
    ends inside the total"""
    at = 0
    for s in sorted(spans, key=lambda s: s["off"]):
        assert s["bytes"] == size and s["host"] == -1 and s["live"] == 1
        assert s["off"] % 16 == 0 and s["off"] >= at
        at = s["off"] + s["bytes"]
    assert at <= sc[0] and sc[0] % 256 == 0


def test_the_existing_layouts_are_as_they_were():
    assert sl.LAYOUT_KINDS[:6] == ("path_state", "query", "denoise", "history", "frame_table", "camera_table")
    sc, spans = sl.dev_layout("history", 64 * 36)
    assert len(spans) == 7 and sc[0] == sum((s["bytes"] + 255) // 256 * 256 for s in spans)


# ------------------------------------------------------------------------------------ boundary
def test_header_and_binding():
    text = (ROOT / "include" / "rt_abi.h").read_text()
    assert re.search(r"#define RT_HAS_TEMPORAL_MOTION 1", text)
    assert re.search(r"int rt_temporal_set_motion\(rt_ctx\* ctx, int32_t on\);", text)
    assert re.search(r"int rt_temporal_get_motion\(const rt_ctx\* ctx, int32_t\* on\);", text)
    assert "#define RT_ABI_VERSION 7" in text
    assert "caller resets it" not in text
    assert hasattr(renderer.Renderer, "set_temporal_motion") and hasattr(renderer.Renderer, "get_temporal_motion")
    assert interactive.Settings().enable_temporal_motion is False


class FakeRenderer:
    """Records the calls of a Session (no device)"""

    def __init__(self):
        self.calls, self.loop_num = [], 0

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            if name == "reset":
                self.loop_num = 0
            if name == "render":
                self.loop_num += 1
            return 0
        return call


def test_session_switches_the_mode_like_a_resize():
    r = FakeRenderer()
    s = interactive.Session(r, 64, 36, settings=interactive.Settings(enable_temporal=True))
    s.tick(delta_time=0.05)
    s.tick(delta_time=0.05)
    assert not any(c[0] == "set_temporal_motion" for c in r.calls)
    r.calls.clear()
    s.tick(interactive.Input(gui={"enable_temporal_motion": True}), delta_time=0.05)
    names = [c[0] for c in r.calls]
    assert names.index("set_temporal_motion") < names.index("temporal_async")
    assert [c for c in r.calls if c[0] == "set_temporal_motion"][0][1] == (True,)
    t = [c for c in r.calls if c[0] == "temporal_async"][0][2]
    assert t["advance"] is True and t["reuse_guides"] is False
    r.calls.clear()
    geo = (np.zeros(1, np.int32), np.zeros((1, 3, 3), np.float32), np.zeros((1, 3, 3), np.float32))
    s.tick(interactive.Input(geometry=[geo]), delta_time=0.05)   # (reset, ADVANCE, fresh guides: the library does the rest)
    names = [c[0] for c in r.calls]
    assert "set_temporal_motion" not in names and names.index("update_geometry") < names.index("reset")
    t = [c for c in r.calls if c[0] == "temporal_async"][0][2]
    assert t["advance"] is True and t["reuse_guides"] is False
    r.calls.clear()
    s.tick(delta_time=0.05)
    t = [c for c in r.calls if c[0] == "temporal_async"][0][2]
    assert t["advance"] is False and t["reuse_guides"] is True
