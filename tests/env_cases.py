"""Environment maps of other shapes than the one asset, a Radiance .hdr writer, and numpy models of
the decoder, the sampling cache and the texel lookup (plain numpy, seeded; nothing read from disk).

The maps (env_map / env_pair): width x height, contents uniform in [0.1, 1.0) unless stated.
    one           1 x 1      (hdrResolution^2 / 2 == 0: every light pdf is 0)
    two           2 x 1
    tall          3 x 5      h > w
    narrow_sun    7 x 4      one texel (5e4, 4e4, 3e4)
    odd_sun     100 x 37     one sun texel; neither side a power of two, w*h no multiple of 256
    odd, odd_b  257 x 129    two seeds of one shape
    black_cols   64 x 32     every other column 0 (columns of pdf 0; their cdf rows are NaN)
    black_texels 64 x 32     half the texels 0 at random
    black        16 x 8      all 0 (the cache is NaN throughout)
    big_sun    2048 x 1024   one sun texel; rows >= 512 uniform in [1.0, 3.0) instead: 2^21 texels,
                             twice the threads rt_light_table_kernel launches at most, so rows >= 512
                             are written by the second turn of its grid-stride loop
"""
from functools import lru_cache

import numpy as np

SUN = (5e4, 4e4, 3e4)
_SPECS = {  # name: (w, h, seed)
    "one": (1, 1, 11), "two": (2, 1, 12), "tall": (3, 5, 13), "narrow_sun": (7, 4, 14), "odd_sun": (100, 37, 15),
    "odd": (257, 129, 16), "odd_b": (257, 129, 17), "black_cols": (64, 32, 18), "black_texels": (64, 32, 19),
    "black": (16, 8, 20), "big_sun": (2048, 1024, 21),
}
NAMES = tuple(_SPECS)
POSITIVE = ("one", "two", "tall", "narrow_sun", "odd_sun", "odd", "odd_b", "big_sun")


@lru_cache(maxsize=None)
def env_map(name: str) -> np.ndarray:
    """float32 (h, w, 3); read-only (shared between tests)."""
    w, h, seed = _SPECS[name]
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.1, 1.0, (h, w, 3)).astype(np.float32)
    if name == "big_sun":
        img[512:] = rng.uniform(1.0, 3.0, (h - 512, w, 3)).astype(np.float32)
    if name.endswith("_sun"):
        img[int(rng.integers(h)), int(rng.integers(w))] = SUN
    if name == "black_cols":
        img[:, 1::2] = 0.0
    if name == "black_texels":
        img[rng.permutation(w * h).reshape(h, w) < w * h // 2] = 0.0
    if name == "black":
        img[:] = 0.0
    img.setflags(write=False)
    return img


@lru_cache(maxsize=None)
def env_pair(name: str):
    """(map, rts_hdr_cache of it): what rt_set_env and the oracle take."""
    from rtamd import scene_lib as sl
    img = env_map(name)
    cache = sl.hdr_cache(img)
    cache.setflags(write=False)
    return img, cache


@lru_cache(maxsize=None)
def identity_map(w: int, h: int) -> np.ndarray:
    """R = column + 1, G = row + 1, B = 1: a fetched colour names its texel."""
    img = np.ones((h, w, 3), np.float32)
    img[..., 0] = np.arange(1, w + 1, dtype=np.float32)[None, :]
    img[..., 1] = np.arange(1, h + 1, dtype=np.float32)[:, None]
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------- .hdr files
def decode_rgbe(rgbe: np.ndarray) -> np.ndarray:
    """uint8 (h, w, 4) -> float32 (h, w, 3): val / 256 * 2^(e - 128) in float64, then cast.  Every
    value is val * 2^(e - 136), at least 2^-136 (a float32 denormal) and below 2^127: exact."""
    rgbe = np.asarray(rgbe, np.uint8)
    d = np.exp2(rgbe[..., 3].astype(np.float64) - 128.0)[..., None]
    return (rgbe[..., :3].astype(np.float64) / 256.0 * d).astype(np.float32)


def _is_marker(px) -> bool:
    return px[0] == 1 and px[1] == 1 and px[2] == 1


def _rle_component(row: np.ndarray, out: bytearray, st: dict) -> None:
    """New-style RLE of one component of a scanline: runs of 3 to 127 equal bytes as (128 + n,
    value), everything else as literals of 1 to 128 bytes (count, bytes)."""
    n, j, lit = len(row), 0, bytearray()

    def flush():
        if lit:
            out.append(len(lit))
            out.extend(lit)
            st["literals"] += 1
            st["max_literal"] = max(st["max_literal"], len(lit))
            lit.clear()

    while j < n:
        k = j + 1
        while k < n and k - j < 127 and row[k] == row[j]:
            k += 1
        if k - j >= 3:
            flush()
            out.extend((128 + (k - j), int(row[j])))
            st["runs"] += 1
            st["max_run"] = max(st["max_run"], k - j)
            j = k
        else:
            lit.append(int(row[j]))
            j += 1
            if len(lit) == 128:
                flush()
    flush()


def _old_rle_row(row: np.ndarray, out: bytearray, st: dict) -> None:
    """Old-style run-length scanline: a pixel, then its n repeats as 1,1,1,d markers with n's
    base-256 digits, lowest first (the decoder shifts each consecutive marker 8 bits further).
    Leading (0,0,0,0) pixels are written as markers alone: the decoder repeats the zero pixel in
    front of its scanline buffer."""
    w, j = len(row), 0

    def px(k):
        return tuple(int(v) for v in row[k])

    prev = (0, 0, 0, 0)  # what a marker repeats at the start of a scanline
    st["first_markers"] += px(0) == prev
    while j < w:
        if j > 0 or px(0) != prev:
            prev = px(j)
            if _is_marker(prev):
                raise ValueError("a 1,1,1,x pixel cannot be written literally in old_rle / flat mode")
            out.extend(prev)
            j += 1
        k = j
        while k < w and px(k) == prev:
            k += 1
        n, digits = k - j, []
        while n:
            digits.append(n & 255)
            n >>= 8
        for d in digits:
            out.extend((1, 1, 1, d))
        st["markers"] += len(digits)
        st["chained"] += len(digits) > 1
        j = k


def encode_hdr(rgbe: np.ndarray, mode: str, header_lines=()) -> tuple:
    """(file bytes, stats) of write_hdr."""
    rgbe = np.asarray(rgbe)
    if rgbe.dtype != np.uint8 or rgbe.ndim != 3 or rgbe.shape[2] != 4:
        raise ValueError("rgbe: uint8 (h, w, 4)")
    h, w, _ = rgbe.shape
    st = dict(runs=0, literals=0, max_run=0, max_literal=0, markers=0, chained=0, first_markers=0, row_offsets=[])
    out = bytearray(b"#?RADIANCE\n")
    for line in header_lines:
        out.extend(line.encode() + b"\n")
    out.extend(b"\n" + f"-Y {h} +X {w}\n".encode())
    new_style = 8 <= w <= 0x7FFF  # else the decoder reads every scanline the old way
    for y in range(h):
        st["row_offsets"].append(len(out))
        row = rgbe[y]
        if mode == "rle":
            if not new_style:
                raise ValueError("new-style RLE needs 8 <= w <= 32767")
            out.extend((2, 2, w >> 8, w & 255))
            for c in range(4):
                _rle_component(row[:, c], out, st)
            continue
        if new_style and row[0, 0] == 2 and row[0, 1] == 2 and not row[0, 2] & 128:
            raise ValueError("a scanline starting 2,2,x with x < 128 reads as new-style RLE")
        if mode == "flat":
            if np.any(np.all(row[:, :3] == 1, axis=1)):
                raise ValueError("a 1,1,1,x pixel cannot be written literally in old_rle / flat mode")
            out.extend(row.tobytes())
        elif mode == "old_rle":
            _old_rle_row(row, out, st)
        else:
            raise ValueError(f"mode {mode!r}")
    st["row_offsets"].append(len(out))
    return bytes(out), st


def write_hdr(path, rgbe: np.ndarray, mode: str, header_lines=()) -> dict:
    """Write uint8 (h, w, 4) RGBE pixels as a Radiance .hdr.  mode: "rle" (new-style scanlines:
    runs up to 127 and literals up to 128 per component), "flat" (raw pixels) or "old_rle" (1,1,1,n
    repeat markers, chained for runs of 256 and more, and alone at the start of a scanline for
    leading zero pixels).  Raises ValueError for pixels the mode cannot express.  Returns what it
    emitted: counts of runs / literals / markers, the longest run and literal, chained and
    first-pixel markers, and the file offset of each scanline (and of the end)."""
    data, st = encode_hdr(rgbe, mode, header_lines)
    with open(path, "wb") as f:
        f.write(data)
    return st


# ------------------------------------------------------------------------- sampling cache
def _lower_bound(a: np.ndarray, first: np.ndarray, length: int, val: np.ndarray) -> np.ndarray:
    """std::lower_bound's halving search, literally, on flat `a` over [first, first + length) for
    many (first, val) at once: defined for NaN too (NaN < x and x < NaN are false)."""
    first = first.astype(np.int64).copy()
    ln = np.full(first.shape, length, np.int64)
    start = first.copy()
    while np.any(ln > 0):
        half = ln >> 1
        mid = first + half
        act = ln > 0
        with np.errstate(invalid="ignore"):
            less = act & (a[np.where(act, mid, 0)] < val)
        first = np.where(less, mid + 1, first)
        ln = np.where(less, ln - half - 1, np.where(act, half, ln))
    return first - start


def hdr_cache_model(img: np.ndarray) -> np.ndarray:
    """calculateHdrCache (src/core/Utility.h:33-131) in its fp32 evaluation order: luminance in
    double then rounded, the sums sequential in fp32 (cumsum), two lower_bound searches per texel."""
    f = np.float32
    img = np.asarray(img, f)
    h, w, _ = img.shape
    d = img.astype(np.float64)
    lum = ((0.2 * d[..., 0] + 0.7 * d[..., 1]) + 0.1 * d[..., 2]).astype(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        lum_sum = np.cumsum(lum.ravel(), dtype=f)[-1]  # row-major, one add per texel
        pdf = lum / lum_sum
        marg = np.cumsum(pdf, axis=0, dtype=f)[-1]
        cdf_x = np.cumsum(marg, dtype=f)
        cdf_y = np.cumsum(pdf / marg[None, :], axis=0, dtype=f).T.copy()  # [column, row]
    xi_1 = np.arange(h, dtype=f) / f(h)
    xi_2 = np.arange(w, dtype=f) / f(w)
    x = np.minimum(_lower_bound(cdf_x, np.zeros(h, np.int64), w, xi_1), w - 1)
    xs = np.repeat(x[:, None], w, axis=1)
    y = _lower_bound(cdf_y.ravel(), xs * h, h, np.repeat(xi_2[None, :], h, axis=0))
    out = np.empty((h, w, 3), f)
    out[..., 0] = xs.astype(f) / f(w)
    out[..., 1] = y.astype(f) / f(h)
    out[..., 2] = pdf
    return out


# -------------------------------------------------------------------------- texel lookup
def camera_texels_f64(fp, W: int, H: int, w: int, h: int, env_angle: float):
    """The texel each camera ray of a W x H frame fetches from a w x h map (RT:1527, 625-631, and
    NEAREST + CLAMP_TO_EDGE), in float64 from the frame's fp32 camera vectors.  Returns (column,
    row, distance): integer (H, W) arrays, frame row 0 = bottom, and each pixel's distance in texels
    from the nearest texel border along either axis."""
    f8 = np.float64
    lbc, right, up = (np.asarray(v, np.float32).astype(f8) for v in (fp.left_bottom_corner, fp.right, fp.up))
    hw, hh = f8(np.float32(fp.half_w)), f8(np.float32(fp.half_h))
    px, py = np.meshgrid(np.arange(W, dtype=f8), np.arange(H, dtype=f8))
    u, v = (px + 0.5) / W, (py + 0.5) / H
    d = lbc + (u * 2.0 * hw)[..., None] * right + (v * 2.0 * hh)[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    tu = (np.arctan2(d[..., 2], d[..., 0]) / (2.0 * np.pi) + 0.5 + f8(np.float32(env_angle))) * w
    tv = (1.0 - (np.arcsin(d[..., 1]) / np.pi + 0.5)) * h
    col = np.clip(np.floor(tu), 0, w - 1).astype(np.int64)
    row = np.clip(np.floor(tv), 0, h - 1).astype(np.int64)
    dist = np.minimum(np.abs(tu - np.round(tu)), np.abs(tv - np.round(tv)))
    return col, row, dist


# ------------------------------------------------------------------- shared oracle renders
IDENTITY_SIZES = ((64, 32), (100, 37))
# u = ux + envAngle with ux in about [0.13, 0.38] for the default camera: no clamp, none, part of
# the frame clamped to column 0, part to the last column, then all of it to either side
IDENTITY_ANGLES = (0.0, 0.6, -0.25, 0.75, -1.25, 3.0)
IDENTITY_FRAME = (96, 54)


@lru_cache(maxsize=None)
def empty_scene():
    from rtamd import configs as cf
    from rtamd import scene_lib as sl
    s = sl.Scene()
    s.build_bvh(8)
    tri, nodes = s.encode()
    return cf.SceneData("empty", s.counts(), tri, nodes, s.export_soa(), s.nodes(), [])


@lru_cache(maxsize=None)
def identity_pair(w: int, h: int):
    from rtamd import scene_lib as sl
    img = identity_map(w, h)
    cache = sl.hdr_cache(img)
    cache.setflags(write=False)
    return img, cache


def identity_frame_params(angle: float):
    from rtamd import configs as cf
    W, H = IDENTITY_FRAME
    return cf.frame_params(W, H, env_angle=angle, env_intensity=1.0)


@lru_cache(maxsize=None)
def identity_oracle_render(w: int, h: int, angle: float) -> np.ndarray:
    """The oracle's one frame of the empty scene under the w x h texel-identity map over a cleared
    history: tests/test_env_cases.py checks it against the float64 lookup, tests/test_gpu_env.py
    the GPU against it."""
    import oracle as orc
    from rtamd import configs as cf
    W, H = IDENTITY_FRAME
    fp = identity_frame_params(angle)
    sd = empty_scene()
    img, cache = identity_pair(w, h)
    frames = [cf.oracle_frame_params(fp, 1, cf.rand_origins(1)[0])]
    out, _ = orc.render(orc.OracleScene(sd.tri_enc, sd.node_enc, img, cache), frames, W, H)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def oracle_case(name: str, scene: str, bsdf: bool, mis: bool, angle: float = 0.6, res=None, W: int = 48, H: int = 27,
                n: int = 2):
    """(image, counters) of the oracle for map `name` on `scene` ("C2" or "empty"), shared by the
    modes that must agree with it (the wavefront path and the megakernel)."""
    import oracle as orc
    from rtamd import configs as cf
    sd = empty_scene() if scene == "empty" else cf.config_scene(scene)
    img, cache = env_pair(name)
    fp = cf.frame_params(W, H, env_angle=angle, enable_bsdf=bsdf, enable_mis=mis)
    ro = cf.rand_origins(n)
    frames = [cf.oracle_frame_params(fp, k + 1, ro[k]) for k in range(n)]
    out, cnt = orc.render(orc.OracleScene(sd.tri_enc, sd.node_enc, img, cache, res), frames, W, H)
    out.setflags(write=False)
    return out, cnt
