"""CPU: the carved device allocations of rt_render.hip (csrc/common/dev_layout.h).

rt_render.hip places the arrays of the path state, the row arena, the query buffers, the display
denoiser's and display history's frames, the frame table and the camera table at the offsets
dvl:: computes and allocates dvl's total.  rts_dev_layout (rt_scene.h) returns the same layouts as
spans {off, bytes, host, live}; this test checks that no two arrays share memory they must not
share, that every array ends inside the allocation and inside the array it aliases, the alignment
the kernels' vector accesses need, and that no allocation is larger than the hand-written sums
these layouts replaced.
"""
import pytest

from rtamd import scene_lib as sl

MI = 1 << 20
CNT_WORDS = 416 + 32 * 8  # rtd::kCntWords (rt_render.hip asserts dvl's copy equals it)
PATHS = (1, 64, 65, 100, 1000, 4099, 6912, 24576, MI, 160 * MI)


def pad(b):
    return (b + 255) & ~255


def faults(spans, total):
    """What is wrong with a layout, as a set of (kind, name, name): spans with memory of their own
    (host -1) that overlap, hosted spans that overlap each other, a span that runs past the
    allocation or past its host.  Empty spans occupy nothing."""
    out = set()
    for s in spans:
        if s["off"] + s["bytes"] > total:
            out.add(("past_total", s["name"], ""))
        if s["host"] >= 0:
            h = spans[s["host"]]
            if s["off"] < h["off"] or s["off"] + s["bytes"] > h["off"] + h["bytes"]:
                out.add(("outside_host", s["name"], h["name"]))
    for hosted in (False, True):
        group = sorted((s for s in spans if (s["host"] >= 0) == hosted and s["bytes"]), key=lambda s: s["off"])
        reach = None  # the span that ends last so far
        for s in group:
            if reach is not None and s["off"] < reach["off"] + reach["bytes"]:
                out.add(("overlap", reach["name"], s["name"]))
            if reach is None or s["off"] + s["bytes"] > reach["off"] + reach["bytes"]:
                reach = s
    return out


def by_name(spans):
    return {s["name"]: s for s in spans}


def test_checker_reports_overlap_and_overrun():
    """The helper itself: one overlapping pair and one array past its host, both reported, and a
    sound layout reported clean."""
    def span(name, off, size, host=-1):
        return dict(name=name, off=off, bytes=size, host=host, live=1)
    good = [span("a", 0, 256), span("b", 256, 512), span("a.x", 0, 128, 0), span("a.y", 128, 128, 0)]
    assert faults(good, 768) == set()
    bad = [span("a", 0, 256), span("b", 192, 512), span("c", 1024, 256), span("c.x", 1152, 256, 2)]
    assert faults(bad, 2048) == {("overlap", "a", "b"), ("outside_host", "c.x", "c")}
    assert faults(good, 767) == {("past_total", "b", "")}
    assert faults([span("a", 0, 256), span("a.x", 0, 128, 0), span("a.y", 64, 128, 0)], 256) == {("overlap", "a.x", "a.y")}


@pytest.mark.parametrize("groups", [1, 2, 3, 4])
@pytest.mark.parametrize("paths", PATHS)
def test_path_state(paths, groups):
    sc, spans = sl.dev_layout("path_state", paths, groups)
    total, set_bytes, P, hit_cap, rows, slot_bytes, row_bytes = sc[:7]
    assert P == max(paths, 64) and hit_cap == P // 64 + 64
    assert slot_bytes == 184 and row_bytes == 148  # the figures DESIGN.md §3 quotes
    assert faults(spans, total) == set()
    assert groups * 184 * P <= total == groups * set_bytes
    # never more than the sum this layout replaced: 184 P + the hit list + 32768 B of padding per set
    assert total <= groups * (184 * P + 4 * (P // 64 + 64) + 32768)
    N = by_name(spans)
    for g in range(groups):
        own = [s for s in spans if s["name"].startswith(f"{g}.") and s["host"] < 0]
        assert len(own) == 18 and all(s["off"] % 256 == 0 for s in own)
        assert all(g * set_bytes <= s["off"] and s["off"] + s["bytes"] <= (g + 1) * set_bytes for s in own)
        assert sum(s["bytes"] for s in own) == 184 * P + 4 * hit_cap + 4 * CNT_WORDS
        assert N[f"{g}.hit"]["bytes"] == 4 * hit_cap and N[f"{g}.cnt"]["bytes"] == 4 * CNT_WORDS
        for k in range(2):  # the split queues' shadow half is the upper half of the queue
            q, qs = N[f"{g}.queue{k}"], N[f"{g}.queue_s{k}"]
            assert spans[qs["host"]] is q and q["bytes"] == 8 * P
            assert qs["off"] == q["off"] + 4 * P and qs["bytes"] == 4 * P


# where the row arena's arrays live, and the slot arrays a lean group still uses
ARENA_HOST = {"s0": "s1", "s1": "s1", "s2": "s1", "s3": "s1", "s4": "s5", "ra": "s5", "sa": "rb", "s5": "rb",
              "rb": "rb", "sb": "sb", "res": "sb", "rpath": "sb"}
ROW_BYTES = {"s0": 16, "s1": 16, "s2": 16, "s3": 16, "s4": 16, "s5": 8, "ra": 16, "rb": 8, "sa": 16, "sb": 8,
             "res": 8, "rpath": 4}
DEAD_IN_LEAN = {"s1", "s5", "rb", "sb"}


@pytest.mark.parametrize("groups", [1, 2, 3, 4])
@pytest.mark.parametrize("paths", PATHS)
def test_row_arena(paths, groups):
    sc, spans = sl.dev_layout("path_state", paths, groups)
    total, P, rows = sc[0], sc[2], sc[4]
    assert rows == (P // 4) & ~3
    assert faults(spans, total) == set()  # inside their hosts, disjoint from each other
    for g in range(groups):
        slots = [s for s in spans if s["name"].startswith(f"{g}.") and "arena" not in s["name"]]
        assert {s["name"].split(".")[1] for s in slots if not s["live"]} == DEAD_IN_LEAN
        arena = [s for s in spans if s["name"].startswith(f"{g}.arena.")]
        assert len(arena) == 12 and sum(s["bytes"] for s in arena) == 148 * rows
        for s in arena:
            name = s["name"].split(".")[2]
            host = spans[s["host"]]
            assert host["name"] == f"{g}.{ARENA_HOST[name]}" and not host["live"]
            assert s["bytes"] == ROW_BYTES[name] * rows and s["off"] % 16 == 0
            # it touches no array a lean group still uses
            for o in slots:
                if o["live"] and o["host"] < 0:
                    assert s["off"] + s["bytes"] <= o["off"] or o["off"] + o["bytes"] <= s["off"], (s, o)


@pytest.mark.parametrize("n", [1, 1024, 1025, 4 * MI])
def test_query(n):
    sc, spans = sl.dev_layout("query", n)
    total, rays = sc[:2]
    assert rays == max(n, 1024)
    assert faults(spans, total) == set()
    assert all(s["off"] % 256 == 0 and s["host"] < 0 for s in spans)
    N = by_name(spans)
    per_ray = {"ra": 16, "rb": 8, "queue": 4, "res": 8, "d_in": 24, "d_out": 48}
    assert all(N[k]["bytes"] == v * rays for k, v in per_ray.items())
    assert N["cnt"]["bytes"] == 4 * CNT_WORDS and N["zero"]["bytes"] == 4
    assert 108 * rays + 4 * CNT_WORDS + 4 <= total <= 108 * rays + 4 * CNT_WORDS + 2048


# W, H, tile size, local tiles; the last: 4 x 2 tiles of 32 x 32 cover more than the 100 x 50 frame
FRAMES = [(1, 1, 32, 1), (17, 9, 8, 6), (1920, 1080, 32, 60 * 34), (100, 50, 32, 8)]


@pytest.mark.parametrize("W,H,tile,local_tiles", FRAMES)
def test_denoise_and_history(W, H, tile, local_tiles):
    npx, hit_px = W * H, local_tiles * tile * tile
    sc, spans = sl.dev_layout("denoise", npx, hit_px)
    assert faults(spans, sc[0]) == set()
    assert all(s["off"] % 256 == 0 for s in spans)
    assert [s["bytes"] for s in spans] == [16 * npx] * 4 + [48 * hit_px, 12 * npx]
    assert sc[0] == 4 * pad(16 * npx) + pad(48 * hit_px) + pad(12 * npx)
    sc, spans = sl.dev_layout("history", npx)
    assert faults(spans, sc[0]) == set()
    assert all(s["off"] % 256 == 0 for s in spans)
    assert [s["bytes"] for s in spans] == [16 * npx] * 6 + [12 * npx]
    assert sc[0] == 6 * pad(16 * npx) + pad(12 * npx)


@pytest.mark.parametrize("cap", [1, 16, 1024, 1500])
def test_frame_table(cap):
    sc, spans = sl.dev_layout("frame_table", cap)
    assert sc[0] == 12 * cap and sc[1] == 2 * cap  # ints: the device table, the host copy
    assert [s["off"] for s in spans] == [0, cap, 2 * cap, 10 * cap]
    assert [s["name"] for s in spans] == ["loop_num", "rand_origin", "sobol", "blend_w"]
    at = 0  # the sub-tables tile the allocation
    for s in spans:
        assert s["off"] == at
        at += s["bytes"]
    assert at == sc[0]


@pytest.mark.parametrize("sets", [1, 2, 3])
@pytest.mark.parametrize("n_valid", [0, 1, 5000, 1920 * 1080])
def test_camera_table(n_valid, sets):
    sc, spans = sl.dev_layout("camera_table", n_valid, sets)
    total = sc[0]
    assert total == 2 * sets * max(1, n_valid)  # float4: what apply_tiling and a deeper pipeline allocate
    assert faults(spans, total) == set()
    N = by_name(spans)
    for p in range(sets):
        assert N[f"dir{p}"]["off"] == p * n_valid and N[f"dir{p}"]["bytes"] == n_valid
        assert N[f"org{p}"]["off"] == sets * max(1, n_valid) + p * n_valid and N[f"org{p}"]["bytes"] == n_valid


def test_rejects_bad_arguments():
    for kind, n, m in (("path_state", 64, 0), ("path_state", 64, 5), ("camera_table", 64, 9)):
        with pytest.raises(RuntimeError):
            sl.dev_layout(kind, n, m)
