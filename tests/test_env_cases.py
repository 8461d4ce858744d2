"""The .hdr decoder, the sampling cache and the oracle's texel lookup on other inputs than the one
asset (tests/env_cases.py): every scanline encoding the decoder reads, malformed files, maps of
odd shapes and contents, and an independent float64 statement of which texel a camera ray fetches.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import env_cases as ec
from conftest import ROOT
from rtamd import scene_lib as sl

RTS_OK, RTS_ERR_FORMAT = 0, -3
WIDTHS = (1, 7, 8, 9, 100, 300)
ENCODINGS = ("rle", "flat", "old_rle", "flat_22x", "flat_2x")
HEADERS = ((), ("FORMAT=32-bit_rle_rgbe", "EXPOSURE=1.0"), ("# written by tests/env_cases.py", "FORMAT=32-bit_rle_rgbe"))
SPECIAL_E = (0, 1, 127, 128, 129, 255)
REF_EXE = ROOT / "oracle" / "_ref" / "ref_hdr_dump"


def _pixels(w, h, seed, enc):
    """Random RGBE bytes with the exponent bytes 0, 1, 127, 128, 129, 255 and the mantissas 0 and
    255 planted, stretches of repeated pixels (the first scanline of an image of more than two is
    one pixel throughout: runs at the 127 limit, and a repeat count above 255), made expressible in
    `enc`: no literal 1,1,1,x pixel outside new-style RLE, no scanline starting 2,2,x<128."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    sel = rng.random((h, w)) < 0.5
    px[..., 3][sel] = rng.choice(SPECIAL_E, (h, w))[sel]
    m = rng.random((h, w, 3))
    px[..., :3][m < 0.1] = 0
    px[..., :3][m > 0.9] = 255
    for y in range(h):
        for _ in range(int(rng.integers(0, 3))):  # stretches of one pixel
            a = int(rng.integers(0, w))
            px[y, a:a + int(rng.integers(2, 12))] = px[y, a]
    if h > 2:
        px[0] = px[0, 0]
    if enc == "old_rle" and h > 1:
        px[h - 1, :min(w, 3)] = 0  # leading zero pixels: a marker as the first pixel of a scanline
    if enc != "rle":
        lit = np.all(px[..., :3] == 1, axis=-1)
        px[..., 0][lit] = 3
        if enc == "flat_22x":
            px[:, 0, 0], px[:, 0, 1] = 2, 2
            px[:, 0, 2] |= 128
        elif enc == "flat_2x":
            px[:, 0, 0] = 2
            px[:, 0, 1][px[:, 0, 1] == 2] = 7
        else:
            start = (px[:, 0, 0] == 2) & (px[:, 0, 1] == 2) & (px[:, 0, 2] < 128)
            px[:, 0, 2][start] |= 128
    return px


def _cases():
    """(id, rgbe, mode, header lines) of every well-formed file: widths x encodings (where legal) x
    heights 1..5, the three header variants in turn."""
    for wi, w in enumerate(WIDTHS):
        for ei, enc in enumerate(ENCODINGS):
            if enc == "rle" and w < 8:
                continue
            for h in range(1, 6):
                hl = HEADERS[(h + wi + ei) % 3]
                yield f"{enc}-{w}x{h}", _pixels(w, h, 1000 * wi + 10 * ei + h, enc), "rle" if enc == "rle" else (
                    "old_rle" if enc == "old_rle" else "flat"), hl


def _load(path):
    """rts_hdr_load's return code, (w, h) and the image (None when no image was returned)."""
    L = sl.lib()
    w, h = C.c_int32(-7), C.c_int32(-7)
    p = C.POINTER(C.c_float)()
    rc = L.rts_hdr_load(str(path).encode(), C.byref(w), C.byref(h), C.byref(p))
    img = None
    if p:
        img = np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
        L.rts_free(C.cast(p, C.c_void_p))
    return rc, (w.value, h.value), img


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------- decoder
def test_decode_model_values():
    """decode_rgbe at the format's corners: exact in float32, denormals and the top exponent too."""
    px = np.array([[[255, 128, 1, 0], [255, 0, 1, 255], [128, 64, 0, 128], [0, 0, 0, 200], [3, 2, 1, 129]]], np.uint8)
    d = ec.decode_rgbe(px)[0].astype(np.float64)
    assert np.array_equal(d[0], np.array([255, 128, 1]) * 2.0 ** -136)
    assert np.array_equal(d[1], np.array([255, 0, 1]) * 2.0 ** 119) and np.all(np.isfinite(d))
    assert np.array_equal(d[2], [0.5, 0.25, 0.0]) and np.array_equal(d[3], [0, 0, 0])
    assert np.array_equal(d[4], np.array([3, 2, 1]) / 128.0)


@pytest.mark.parametrize("w,enc", [(w, e) for w in WIDTHS for e in ENCODINGS if e != "rle" or w >= 8])
def test_decoder_equals_model_bitwise(tmp_path, w, enc):
    """sl.load_hdr of every encoding the decoder reads equals decode_rgbe bit for bit: new-style RLE
    (runs and literals), flat pixels, old-style repeat markers (single, chained, and first in a
    scanline), flat scanlines starting 2,2,x>=128 and 2,x (which decrunch first takes for RLE),
    widths on both sides of the new-style minimum of 8 (below it there is no new-style RLE), under
    three headers."""
    seen = dict(runs=0, literals=0, max_run=0, max_literal=0, markers=0, chained=0, first_markers=0)
    n = 0
    for cid, px, mode, hl in _cases():
        if not cid.startswith(f"{enc}-{w}x"):
            continue
        st = ec.write_hdr(tmp_path / "a.hdr", px, mode, hl)
        img = sl.load_hdr(tmp_path / "a.hdr")
        assert _same_bits(img, ec.decode_rgbe(px)), (cid, hl)
        for k in seen:
            seen[k] = max(seen[k], st[k]) if k.startswith("max") else seen[k] + st[k]
        n += 1
    assert n == 5
    # the writer did emit what the case is about
    if enc == "rle":
        assert seen["runs"] > 0 and seen["literals"] > 0
        if w == 300:
            assert seen["max_run"] == 127 and seen["max_literal"] == 128
    if enc == "old_rle" and w > 1:
        assert seen["markers"] > 0 and seen["first_markers"] > 0
        if w == 300:
            assert seen["chained"] > 0


def test_decoder_cases_cover_the_byte_values():
    es, ms = set(), set()
    for _, px, _, _ in _cases():
        es |= set(np.unique(px[..., 3]).tolist())
        ms |= set(np.unique(px[..., :3]).tolist())
    assert set(SPECIAL_E) <= es and {0, 255} <= ms


def test_decoder_equals_reference_build_live(tmp_path):
    """The same well-formed files through the reference's own decoder (oracle/_ref/ref_hdr_dump),
    where it is built.  Two kinds stay away from it, because it reads or writes outside its buffers
    on them and decodes them by accident if at all: a header of the magic line alone (it looks for
    the header's empty line from the pixels on, into a 200-byte array), and a repeat marker as the
    first pixel of a scanline (it copies the four bytes in front of its scanline allocation)."""
    if not REF_EXE.exists():
        pytest.skip("oracle/_ref not built (reference absent)")
    n = 0
    for cid, px, mode, hl in _cases():
        data, st = ec.encode_hdr(px, mode, hl)
        if not hl or st["first_markers"]:
            continue
        (tmp_path / "a.hdr").write_bytes(data)
        subprocess.run([str(REF_EXE), str(tmp_path / "a.hdr"), str(tmp_path / "o.bin")], check=True)
        raw = (tmp_path / "o.bin").read_bytes()
        w, h = np.frombuffer(raw[:8], np.int32)
        ref = np.frombuffer(raw[8:], np.float32).reshape(h, w, 3)
        assert _same_bits(sl.load_hdr(tmp_path / "a.hdr"), ref), cid
        n += 1
    assert n >= 60


def test_writer_refuses_what_a_mode_cannot_express():
    px = np.full((1, 9, 4), 9, np.uint8)
    px[0, 4] = (1, 1, 1, 5)
    for mode in ("flat", "old_rle"):
        with pytest.raises(ValueError):
            ec.encode_hdr(px, mode)
    ec.encode_hdr(px, "rle")
    px[0, 4] = 9
    px[0, 0] = (2, 2, 100, 9)
    with pytest.raises(ValueError):
        ec.encode_hdr(px, "flat")
    with pytest.raises(ValueError):
        ec.encode_hdr(px[:, :7], "rle")


# ------------------------------------------------------------------------ malformed files
@pytest.mark.parametrize("w,mode", [(9, "rle"), (9, "flat"), (9, "old_rle"), (5, "flat"), (5, "old_rle")])
def test_truncated_file_keeps_the_rows_before(tmp_path, w, mode):
    """A file that ends inside scanline 2 of 4: RTS_OK, scanlines 0 and 1 decoded, the rest 0 (the
    reference's behaviour: its loop breaks at the first scanline that hits the end of the file)."""
    px = _pixels(w, 4, 77, mode)
    px[2] = np.arange(3, 3 + 4 * w, dtype=np.uint8).reshape(w, 4)  # no repeats: at least 4 bytes per pixel or component
    data, st = ec.encode_hdr(px, mode, HEADERS[1])
    want = ec.decode_rgbe(px)
    want[2:] = 0
    for cut in (st["row_offsets"][2] + 1, st["row_offsets"][2] + 6, st["row_offsets"][3] - 1):
        (tmp_path / "t.hdr").write_bytes(data[:cut])
        rc, size, img = _load(tmp_path / "t.hdr")
        assert rc == RTS_OK and size == (w, 4), (cut, rc)
        assert _same_bits(img, want), cut


def test_file_ending_at_a_scanline_boundary(tmp_path):
    px = _pixels(9, 3, 5, "rle")
    data, st = ec.encode_hdr(px, "rle", HEADERS[1])
    (tmp_path / "t.hdr").write_bytes(data[:st["row_offsets"][1]])
    rc, _, img = _load(tmp_path / "t.hdr")
    want = ec.decode_rgbe(px)
    want[1:] = 0
    assert rc == RTS_OK and _same_bits(img, want)


@pytest.mark.parametrize("name,data", [
    ("no-magic", b"#?RADIANCX\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\n\x01\x02\x03\x80"),
    ("short", b"#?RADIAN"),
    ("no-blank-line", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n-Y 1 +X 1\n\x01\x02\x03\x80"),
    ("no-resolution-line", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1"),
    ("x-first", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+X 1 -Y 1\n\x01\x02\x03\x80"),
    ("plus-y", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+Y 1 +X 1\n\x01\x02\x03\x80"),
    ("one-number", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1\n\x01\x02\x03\x80"),
    ("zero-width", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 0\n\x01\x02\x03\x80"),
    ("zero-height", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 0 +X 1\n\x01\x02\x03\x80"),
    ("negative-width", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X -4\n\x01\x02\x03\x80"),
    ("negative-height", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y -1 +X 1\n\x01\x02\x03\x80"),
])
def test_bad_headers_are_format_errors(tmp_path, name, data):
    (tmp_path / "t.hdr").write_bytes(data)
    rc, _, img = _load(tmp_path / "t.hdr")
    assert rc == RTS_ERR_FORMAT and img is None


def _old_file(w, h, pixel_bytes):
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode() + bytes(pixel_bytes)


P, Q = (9, 8, 7, 128), (30, 20, 10, 129)
M = lambda n: (1, 1, 1, n)  # noqa: E731


def _flat(*pixels):
    return [b for p in pixels for b in p]


@pytest.mark.parametrize("name,w,h,body", [
    ("first-marker", 4, 1, _flat(P, M(255))),              # the issue's file: 255 repeats into 3 pixels
    ("one-too-many", 4, 1, _flat(P, M(4))),
    ("marker-opens-the-scanline", 4, 1, _flat(M(5))),
    ("second-scanline", 4, 2, _flat(P, M(3), Q, Q, M(3))),
    ("chained", 300, 1, _flat(P, M(40), M(2))),            # 40 + (2 << 8) = 552 repeats into 299
    ("chained-second-alone", 100, 1, _flat(P, M(1), M(1))),  # 1 fits, 1 << 8 does not
    ("chain-of-three", 300, 1, _flat(P, M(0), M(0), M(1))),  # 1 << 16
    ("shift-past-32-bits", 4, 1, _flat(P, M(0), M(0), M(0), M(0), M(0), M(0), M(1))),
    ("after-2x-start", 9, 1, _flat((2, 5, 5, 128), M(9))),  # decrunch's flat fallback: 8 pixels left
    ("wider-than-rle", 40000, 1, _flat(P, M(255), M(255))),  # 255 + 65280 repeats into 39999
])
def test_old_rle_run_past_the_scanline_is_a_format_error(tmp_path, name, w, h, body):
    """The overrun the reference's oldDecrunch writes past its scanline buffer with: a repeat count
    (shifted 8 bits per marker directly before it) above what is left of the scanline.  rts_hdr_load
    returns RTS_ERR_FORMAT and no image (tests/sanitize/hdr_load_sweep.cpp runs the same files under
    AddressSanitizer, which also reports a leak)."""
    (tmp_path / "t.hdr").write_bytes(_old_file(w, h, body))
    rc, _, img = _load(tmp_path / "t.hdr")
    assert rc == RTS_ERR_FORMAT and img is None


def test_old_rle_runs_that_just_fit(tmp_path):
    """The same shapes one repeat shorter decode: a run to the scanline's last pixel, a chain to it,
    zero counts (which repeat nothing at any shift), and a run after decrunch's flat fallback."""
    def load(w, h, body):
        (tmp_path / "t.hdr").write_bytes(_old_file(w, h, body))
        rc, size, img = _load(tmp_path / "t.hdr")
        assert rc == RTS_OK and size == (w, h)
        return img

    def rows(*pixels):
        return ec.decode_rgbe(np.array(pixels, np.uint8).reshape(1, -1, 4))

    assert _same_bits(load(4, 1, _flat(P, M(3))), rows(P, P, P, P))
    assert _same_bits(load(4, 1, _flat(M(4))), rows(*[(0, 0, 0, 0)] * 4))
    assert _same_bits(load(300, 1, _flat(P, M(43), M(1))), rows(*[P] * 300))
    assert _same_bits(load(4, 1, _flat(P, M(0), M(0), M(0), M(0), M(0), M(0), Q, M(2))), rows(P, Q, Q, Q))
    assert _same_bits(load(9, 1, _flat((2, 5, 5, 128), M(8))), rows(*[(2, 5, 5, 128)] * 9))
    assert _same_bits(load(40000, 1, _flat(P, M(63), M(156))), rows(*[P] * 40000))


# ------------------------------------------------------------------------- sampling cache
@pytest.mark.parametrize("name", ec.NAMES)
def test_hdr_cache_equals_model_bitwise(name):
    """rts_hdr_cache against calculateHdrCache restated in numpy, bit for bit, NaN included (black
    columns divide 0 by 0; the halving search is defined on them)."""
    img, cache = ec.env_pair(name)
    model = ec.hdr_cache_model(img)
    assert _same_bits(cache, model)
    if name == "black":
        assert int(np.isnan(cache).sum()) == 128
    if name == "black_cols":
        assert np.all(cache[..., 2][:, 1::2] == 0) and np.all(cache[..., 2][:, 0::2] > 0)


@pytest.mark.parametrize("name", ec.POSITIVE)
def test_hdr_cache_properties_on_positive_maps(name):
    """x and y lie in [0, 1] and do not decrease along their search axis (x is found from xi_1 =
    row / h, y from xi_2 = column / w), the pdf sums to 1, and the share of cache rows that point at
    column x follows the marginal.  The bound of the last: the rows with x are those whose i / h
    lies in (cdf[x-1], cdf[x]], one more or fewer than h times that interval; the interval is the
    column's sum m[x] of the pdf channel (taken here in float64) up to the fp32 rounding of the h
    adds of the marginal and the w adds of the cdf, at both ends: 2 (h + w) 2^-24; the last column
    also takes the rows past the cdf's end, |1 - sum m|."""
    img, cache = ec.env_pair(name)
    h, w, _ = img.shape
    x, y, pdf = cache[..., 0], cache[..., 1], cache[..., 2].astype(np.float64)
    assert x.min() >= 0 and x.max() <= 1 and y.min() >= 0 and y.max() <= 1
    assert np.all(np.diff(x, axis=0) >= 0) and np.all(np.diff(y, axis=1) >= 0)
    assert abs(pdf.sum() - 1.0) < 1e-3
    xs = np.rint(x.astype(np.float64) * w).astype(np.int64)
    assert np.all(xs == xs[:, :1])  # a row's texels share one x
    share = np.bincount(xs[:, 0], minlength=w) / h
    m = pdf.sum(axis=0)
    tol = np.full(w, 1.0 / h + 2.0 * (h + w) * 2.0 ** -24)
    tol[-1] += abs(1.0 - m.sum())
    assert np.all(np.abs(share - m) <= tol), float(np.max(np.abs(share - m) - tol))
    if name.endswith("_sun"):  # most of a sun map's cache points at the sun's column
        sy, sx = np.argwhere(img[..., 0] == ec.SUN[0])[0]
        assert share[sx] == share.max() and (name == "big_sun" or share[sx] > 0.5)


# ---------------------------------------------------------------------------- lookup
@pytest.mark.parametrize("angle", ec.IDENTITY_ANGLES)
@pytest.mark.parametrize("w,h", ec.IDENTITY_SIZES)
def test_oracle_lookup_names_the_float64_texel(w, h, angle):
    """The oracle's empty-scene frame under the texel-identity map (R = column + 1, G = row + 1):
    every pixel is one texel's colour, and it is the texel a float64 evaluation of the camera ray's
    spherical coordinates names (camera vectors promoted from fp32; normalize, atan2, asin, +
    envAngle, floor, clamp), except where float64 u*w or v*h lies within 1e-3 of an integer (the
    fp32 builtins are stated at <= 3 ulp, about 4e-7 in u, times w <= 100).  Measured share of
    excluded pixels at 96 x 54 (the cap is 2 %): 64 x 32: 0.39 % at every angle but 0.6 (0.21 %);
    100 x 37: 0.44 % at every angle.  The frame sees columns 7..25 / 11..39 at angle 0 and rows
    13..23 / 15..27; the angles move the columns, -0.25 and 0.75 clamp part of the frame to the
    first / last column, -1.25 and 3.0 all of it."""
    W, H = ec.IDENTITY_FRAME
    out = ec.identity_oracle_render(w, h, angle)
    col, row = out[..., 0] - 1.0, out[..., 1] - 1.0
    assert np.all(out[..., 2] == 1.0)
    assert np.all(col == np.floor(col)) and np.all((col >= 0) & (col <= w - 1))
    assert np.all(row == np.floor(row)) and np.all((row >= 0) & (row <= h - 1))
    c64, r64, dist = ec.camera_texels_f64(ec.identity_frame_params(angle), W, H, w, h, angle)
    keep = dist > 1e-3
    excluded = 1.0 - keep.mean()
    print(f"identity {w}x{h} angle {angle}: excluded {excluded:.4%}, "
          f"columns {int(c64.min())}..{int(c64.max())}, rows {int(r64.min())}..{int(r64.max())}")
    assert excluded < 0.02
    assert np.array_equal(col[keep].astype(np.int64), c64[keep])
    assert np.array_equal(row[keep].astype(np.int64), r64[keep])
    if angle in (-1.25, 3.0):  # clamped throughout
        assert np.all(c64 == (0 if angle < 0 else w - 1))
    if angle in (-0.25, 0.75):  # clamped in part
        edge = 0 if angle < 0 else w - 1
        assert 0.05 < np.mean(c64 == edge) < 0.95
