"""How rt_render_async schedules each call shape, read off rt_stats: `launches` counts the batches
with work, `trace_launches` the traversal launches (one per wavefront pass of a group, one per
megakernel launch) and `finish_steps` is non-zero only when wf_finish ran.  Every case also
equals the oracle bit for bit, with the oracle's ray count.

The renderer is this module's own: the path-state size (it only grows) and the finisher settings
of the session's shared renderer depend on the tests that ran before.  Pipelined calls are not
here: whether a one-frame call finds the streams idle depends on timing, so its group count is
not fixed (tests/test_gpu_api.py covers their result)."""
import pytest

from helpers import bit_mismatch, frames_for, oracle_render
from rtamd import configs as cf
from rtamd.renderer import (RT_FLAG_COUNT_VISITS, RT_FLAG_MEGAKERNEL, RT_FLAG_NO_FINISH, RT_FLAG_SERIAL,
                            Renderer)

pytestmark = pytest.mark.gpu

W, H = 96, 72
B = cf.frame_params(W, H).max_bounce  # passes 0 .. B


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def refs(env_maps):
    """Oracle image and counters after 1, 3 and 6 progressive frames of C3 at W x H (computed once:
    each continues the previous one's accumulation)."""
    sd = cf.config_scene("C3")
    ro, frames = frames_for(cf.frame_params(W, H), 1, 6)
    out, acc, rays, k0 = {}, None, 0, 0
    for n in (1, 3, 6):
        acc, cnt = oracle_render(sd, env_maps, W, H, frames[k0:n], accum=acc)
        rays += cnt["rays"]
        out[n] = (acc, rays)
        k0 = n
    return out


def _render(r, env_maps, w, h, fp, ro):
    sd = cf.config_scene("C3")
    r.set_scene_soa(sd.soa, sd.nodes)
    r.set_env(*env_maps)
    r.resize(w, h)
    r.reset_stats()
    st = r.render(fp, ro)
    return r.read_accum(), st


def _check(img, st, ref, rays, launches, trace_launches):
    assert bit_mismatch(img, ref)[0] == 0.0
    assert st["rays"] == rays, st
    assert st["launches"] == launches, st
    assert st["trace_launches"] == trace_launches, st


def test_one_frame_runs_two_pixel_groups_into_the_finisher(renderer, env_maps, refs):
    """Two pixel groups trace passes 0 and 1; wf_finish takes over from pass 2."""
    fp = cf.frame_params(W, H)
    img, st = _render(renderer, env_maps, W, H, fp, cf.rand_origins(1))
    _check(img, st, *refs[1], launches=1, trace_launches=4)
    assert st["finish_steps"] > 0, st


def test_one_frame_without_the_finisher_runs_every_pass(renderer, env_maps, refs):
    fp = cf.frame_params(W, H, flags=RT_FLAG_NO_FINISH)
    img, st = _render(renderer, env_maps, W, H, fp, cf.rand_origins(1))
    _check(img, st, *refs[1], launches=1, trace_launches=2 * (B + 1))
    assert st["finish_steps"] == 0, st


def test_visit_counting_runs_every_pass(renderer, env_maps, refs):
    """RT_FLAG_COUNT_VISITS: the counting trace in every pass of both pixel groups, no finisher."""
    fp = cf.frame_params(W, H, flags=RT_FLAG_COUNT_VISITS)
    img, st = _render(renderer, env_maps, W, H, fp, cf.rand_origins(1))
    _check(img, st, *refs[1], launches=1, trace_launches=2 * (B + 1))
    assert st["finish_steps"] == 0, st
    assert st["tri_tests"] > 0, st


def test_frame_groups_over_two_batches(renderer, env_maps, refs):
    """6 frames with room for 4: batches of 4 and 2 frames, two frame groups each, each group
    tracing passes 0 and 1 before its finisher."""
    fp = cf.frame_params(W, H)
    renderer.set_max_paths(4 * W * H)
    try:
        img, st = _render(renderer, env_maps, W, H, fp, cf.rand_origins(6))
    finally:
        renderer.set_max_paths(0)
    _check(img, st, *refs[6], launches=2, trace_launches=8)


def test_serial_runs_one_group_per_batch(env_maps, refs):
    """RT_FLAG_SERIAL on a fresh renderer: its path state is sized for two frames per group
    (a budget of 4 frames over two groups), so 6 frames run as 3 batches of one group."""
    fp = cf.frame_params(W, H, flags=RT_FLAG_SERIAL)
    r = Renderer(0)
    try:
        r.set_max_paths(4 * W * H)
        img, st = _render(r, env_maps, W, H, fp, cf.rand_origins(6))
    finally:
        r.close()
    _check(img, st, *refs[6], launches=3, trace_launches=6)


def test_bulk_groups_run_every_pass(renderer, env_maps):
    """Two frame groups of 64 frames above the finisher's size limit: the bulk kernels (split
    queues, camera-hit records, SH_SUB_BULK shade) in every pass."""
    w, h, n = 24, 16, 128
    sd = cf.config_scene("C3")
    fp = cf.frame_params(w, h)
    ro, frames = frames_for(fp, 1, n)
    ref, cnt = oracle_render(sd, env_maps, w, h, frames)
    renderer.set_finish(2, 1)
    try:
        img, st = _render(renderer, env_maps, w, h, fp, ro)
    finally:
        renderer.set_finish(2, 8 << 20)
    _check(img, st, ref, cnt["rays"], launches=1, trace_launches=2 * (B + 1))
    assert st["finish_steps"] == 0, st


def test_megakernel_is_one_launch(renderer, env_maps, refs):
    fp = cf.frame_params(W, H, flags=RT_FLAG_MEGAKERNEL)
    img, st = _render(renderer, env_maps, W, H, fp, cf.rand_origins(3))
    _check(img, st, *refs[3], launches=1, trace_launches=1)
