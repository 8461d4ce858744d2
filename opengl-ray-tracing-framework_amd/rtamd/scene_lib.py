"""ctypes bindings of librtscene.so (include/rt_scene.h): the reference's host pipeline.

Python mirror of the reference's scene-assembly calls (src/core/Scene.h:35-257):
``Mesh.load`` ~ ``Model(path)``, ``Scene.add_mesh`` ~ ``getTriangle(...)``,
``Scene.build_bvh`` ~ ``buildBVHwithSAH(...)``, ``Scene.encode`` ~
``EncodedBVHandTriangles()``, ``load_hdr``/``hdr_cache`` ~ ``InitHdrEnvMap()``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional, Sequence

import numpy as np

from ._paths import lib_path

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)


class RtsMaterial(C.Structure):
    _fields_ = [
        ("emissive", C.c_float * 3),
        ("base_color", C.c_float * 3),
        ("subsurface", C.c_float), ("metallic", C.c_float), ("specular", C.c_float),
        ("specular_tint", C.c_float), ("roughness", C.c_float), ("anisotropic", C.c_float),
        ("sheen", C.c_float), ("sheen_tint", C.c_float), ("clearcoat", C.c_float),
        ("clearcoat_gloss", C.c_float), ("ior", C.c_float), ("transmission", C.c_float),
        ("medium_color", C.c_float * 3),
        ("medium_type", C.c_float), ("medium_density", C.c_float), ("medium_anisotropy", C.c_float),
    ]


@dataclasses.dataclass
class Material:
    """src/core/Material.h:25-46 with the reference defaults."""
    emissive: Sequence[float] = (0.0, 0.0, 0.0)
    base_color: Sequence[float] = (1.0, 1.0, 1.0)
    subsurface: float = 0.0
    metallic: float = 0.0
    specular: float = 0.0
    specular_tint: float = 0.0
    roughness: float = 0.0
    anisotropic: float = 0.0
    sheen: float = 0.0
    sheen_tint: float = 0.0
    clearcoat: float = 0.0
    clearcoat_gloss: float = 0.0
    ior: float = 1.0
    transmission: float = 0.0
    medium_color: Sequence[float] = (1.0, 1.0, 1.0)
    medium_type: float = 0.0
    medium_density: float = 0.0
    medium_anisotropy: float = 0.0

    def to_c(self) -> RtsMaterial:
        m = RtsMaterial()
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if isinstance(v, (tuple, list)):
                arr = getattr(m, f.name)
                for i in range(3):
                    arr[i] = float(np.float32(v[i]))
            else:
                setattr(m, f.name, float(np.float32(v)))
        return m

    def texels(self) -> np.ndarray:
        """The 24 material floats of Triangle_encoded texels 6..13 (src/core/Triangle.h:31-38)."""
        return np.array(list(self.emissive) + list(self.base_color) + [
            self.subsurface, self.metallic, self.specular, self.specular_tint, self.roughness,
            self.anisotropic, self.sheen, self.sheen_tint, self.clearcoat, self.clearcoat_gloss,
            self.ior, self.transmission] + list(self.medium_color) + [
            self.medium_type, self.medium_density, self.medium_anisotropy], dtype=np.float32)

    @classmethod
    def from_texels(cls, t) -> "Material":
        """The inverse of texels(): a Material from its 24 floats (rt_get_triangle_material)."""
        t = [float(x) for x in np.asarray(t, np.float32).reshape(24)]
        return cls(tuple(t[0:3]), tuple(t[3:6]), *t[6:18], tuple(t[18:21]), *t[21:24])


class RtsCompiledView(C.Structure):
    _fields_ = ([(k, _f32p) for k in ("tri", "trx", "trin", "hrec", "mats")]
                + [("nodes", C.c_void_p), ("qnodes", C.c_void_p), ("tri_mat", _i32p)]
                + [(k, C.c_int64) for k in ("n_tri_f", "n_trx_f", "n_trin_f", "n_hrec_f", "n_mats_f", "n_nodes",
                                            "n_qnodes", "n_tri_mat")]
                + [(k, C.c_double) for k in ("cull_R", "cull_K", "cull_off", "tri_k1", "tri_k0")]
                + [(k, C.c_int32) for k in ("n_tri", "n_mats", "root", "has_scene", "depth", "qroot", "qdepth",
                                            "wide", "tri_flagged")]
                + [("err", C.c_char_p)])


class RtsRefitPlanView(C.Structure):
    _fields_ = ([(k, _i32p) for k in ("leaves", "blist", "boff", "qlist", "qoff")]
                + [(k, C.c_int32) for k in ("n_leaves", "n_blist", "n_boff", "n_qlist", "n_qoff")])


# the scene compiler's records (csrc/common/scene_compile.h scn::BNode, scn::WNode)
BNODE_DTYPE = np.dtype([("box", np.float32, 12), ("ref", np.int32, 4)])
WNODE_DTYPE = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("ref", np.int32, 4),
                        ("pad", np.int32, 4)])
Q_EMPTY = 0x7fffffff
LEAF_BIT = 0x80000000


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        L = C.CDLL(str(lib_path("librtscene.so")))
        vp = C.c_void_p
        L.rts_obj_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
        L.rts_obj_parse_raw.argtypes = [C.c_char_p, C.c_int, _i32p, _i32p, _i32p, _i32p, _f32p, _f32p, _i32p,
                                        _i32p, _i32p]
        L.rts_mesh_from_raw.argtypes = [_f32p, C.c_int, _f32p, C.c_int, _i32p, C.c_int, _i32p, _i32p,
                                        C.POINTER(vp)]
        L.rts_mesh_counts.argtypes = [vp, _i32p, _i32p]
        L.rts_mesh_data.argtypes = [vp, _f32p, _f32p, _i32p]
        L.rts_mesh_free.argtypes = [vp]
        L.rts_mesh_free.restype = None
        L.rts_scene_create.argtypes = [C.POINTER(vp)]
        L.rts_scene_free.argtypes = [vp]
        L.rts_scene_free.restype = None
        L.rts_scene_add_mesh.argtypes = [vp, vp, C.POINTER(RtsMaterial), _f32p, _f32p, _f32p, C.c_int, _i32p]
        L.rts_scene_add_triangles.argtypes = [vp, _f32p, C.c_int, C.POINTER(RtsMaterial), _i32p]
        L.rts_scene_build_bvh.argtypes = [vp, C.c_int]
        L.rts_scene_counts.argtypes = [vp, _i32p, _i32p, _i32p, _i32p]
        L.rts_scene_encode.argtypes = [vp, _f32p, _f32p]
        L.rts_scene_nodes.argtypes = [vp, _i32p, _i32p, _i32p, _i32p, _f32p, _f32p]
        L.rts_scene_export_soa.argtypes = [vp, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _i32p,
                                           C.POINTER(RtsMaterial), _i32p]
        L.rts_scene_set_material.argtypes = [vp, C.c_int, C.c_int, C.POINTER(RtsMaterial)]
        L.rts_scene_post_bvh_index.argtypes = [vp, _i32p]
        L.rts_hdr_load.argtypes = [C.c_char_p, _i32p, _i32p, C.POINTER(_f32p)]
        L.rts_hdr_cache.argtypes = [_f32p, C.c_int, C.c_int, _f32p]
        L.rts_free.argtypes = [vp]
        L.rts_free.restype = None
        L.rts_camera.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, _f32p]
        L.rts_cpu_rand_origins.argtypes = [C.c_uint, C.c_int, _f32p]
        L.rts_glibc_rand.argtypes = [C.c_uint, C.c_int, C.POINTER(C.c_int)]
        L.rts_write_png.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
        L.rts_tri_filter.argtypes = [_f32p, C.c_int, _f32p, C.POINTER(C.c_double), _i32p]
        L.rts_dev_layout.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), vp, C.c_int32, _i32p]
        L.rts_render_plan.argtypes = [C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int64), C.c_int32, _i32p]
        L.rts_compile_scene.argtypes = [vp, _i32p, C.POINTER(vp)]
        L.rts_compile_scene_encoded.argtypes = [_f32p, C.c_int32, _f32p, C.c_int32, _i32p, C.POINTER(vp)]
        L.rts_compiled_get.argtypes = [vp, C.POINTER(RtsCompiledView)]
        L.rts_compiled_free.argtypes = [vp]
        L.rts_compiled_free.restype = None
        L.rts_compiled_update_geometry.argtypes = [vp, _i32p, C.c_int32, C.c_int32] + [_f32p] * 6
        L.rts_compiled_filter_state.argtypes = [vp, C.POINTER(C.c_double)]
        L.rts_refit_plan.argtypes = [vp, C.POINTER(RtsRefitPlanView)]
        _lib = L
    return _lib


def _fp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_f32p)


def _ip(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_i32p)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with rts error {rc}")


@dataclasses.dataclass
class RawObj:
    """OBJ data as parsed: positions, file normals, polygon faces (0-based indices)."""
    positions: np.ndarray
    normals: np.ndarray
    face_sizes: np.ndarray
    pos_index: np.ndarray
    nrm_index: np.ndarray


def parse_obj_raw(path: str, parse_mode: int = 0) -> RawObj:
    L = lib()
    n = [C.c_int32() for _ in range(4)]
    _check(L.rts_obj_parse_raw(str(path).encode(), parse_mode, *[C.byref(x) for x in n],
                               None, None, None, None, None), "rts_obj_parse_raw(sizes)")
    npos, nnrm, nf, ni = (x.value for x in n)
    raw = RawObj(np.zeros((npos, 3), np.float32), np.zeros((nnrm, 3), np.float32),
                 np.zeros(nf, np.int32), np.zeros(ni, np.int32), np.zeros(ni, np.int32))
    _check(L.rts_obj_parse_raw(str(path).encode(), parse_mode, *[C.byref(x) for x in n],
                               _fp(raw.positions), _fp(raw.normals), _ip(raw.face_sizes), _ip(raw.pos_index),
                               _ip(raw.nrm_index)), "rts_obj_parse_raw")
    return raw


class Mesh:
    """A post-processed model (assimp Triangulate | GenSmoothNormals semantics)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    @classmethod
    def load(cls, path: str, parse_mode: int = 0) -> "Mesh":
        h = C.c_void_p()
        _check(lib().rts_obj_load(str(path).encode(), parse_mode, C.byref(h)), f"rts_obj_load({path})")
        return cls(h.value)

    @classmethod
    def from_raw(cls, raw: RawObj) -> "Mesh":
        h = C.c_void_p()
        pos = np.ascontiguousarray(raw.positions, np.float32)
        nrm = np.ascontiguousarray(raw.normals, np.float32)
        fs = np.ascontiguousarray(raw.face_sizes, np.int32)
        pi = np.ascontiguousarray(raw.pos_index, np.int32)
        ni = np.ascontiguousarray(raw.nrm_index, np.int32)
        _check(lib().rts_mesh_from_raw(_fp(pos), len(pos), _fp(nrm) if len(nrm) else None, len(nrm), _ip(fs), len(fs),
                                       _ip(pi), _ip(ni), C.byref(h)), "rts_mesh_from_raw")
        return cls(h.value)

    def data(self):
        nv, ni = C.c_int32(), C.c_int32()
        _check(lib().rts_mesh_counts(self._h, C.byref(nv), C.byref(ni)), "rts_mesh_counts")
        pos = np.zeros((nv.value, 3), np.float32)
        nrm = np.zeros((nv.value, 3), np.float32)
        idx = np.zeros(ni.value, np.int32)
        _check(lib().rts_mesh_data(self._h, _fp(pos), _fp(nrm), _ip(idx)), "rts_mesh_data")
        return pos, nrm, idx

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None and self._h.value:
            _lib.rts_mesh_free(self._h)
            self._h = C.c_void_p()


class Scene:
    """Triangle list + SAH BVH (src/core/RenderSettings.h:502 ``triangles`` + BVH.h)."""

    def __init__(self):
        h = C.c_void_p()
        _check(lib().rts_scene_create(C.byref(h)), "rts_scene_create")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None and self._h.value:
            _lib.rts_scene_free(self._h)
            self._h = C.c_void_p()

    def add_mesh(self, mesh: Mesh, material: Material, rotate=(0, 0, 0), translate=(0, 0, 0), scale=(1, 1, 1),
                 smooth: bool = False):
        r = np.asarray(rotate, np.float32)
        t = np.asarray(translate, np.float32)
        s = np.asarray(np.broadcast_to(np.asarray(scale, np.float32), (3,)), np.float32).copy()
        rng = np.zeros(2, np.int32)
        m = material.to_c()
        _check(lib().rts_scene_add_mesh(self._h, mesh._h, C.byref(m), _fp(r), _fp(t), _fp(s), int(smooth), _ip(rng)),
               "rts_scene_add_mesh")
        return int(rng[0]), int(rng[1])

    def add_triangles(self, positions: np.ndarray, material: Material):
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
        rng = np.zeros(2, np.int32)
        m = material.to_c()
        _check(lib().rts_scene_add_triangles(self._h, _fp(p), len(p), C.byref(m), _ip(rng)), "rts_scene_add_triangles")
        return int(rng[0]), int(rng[1])

    def build_bvh(self, leaf_size: int = 8) -> None:
        _check(lib().rts_scene_build_bvh(self._h, leaf_size), "rts_scene_build_bvh")

    def counts(self):
        v = [C.c_int32() for _ in range(4)]
        _check(lib().rts_scene_counts(self._h, *[C.byref(x) for x in v]), "rts_scene_counts")
        return dict(zip(("n_triangles", "n_nodes", "max_depth", "n_leaves"), (x.value for x in v)))

    def encode(self):
        c = self.counts()
        tri = np.zeros((c["n_triangles"], 14, 3), np.float32)
        nodes = np.zeros((c["n_nodes"], 4, 3), np.float32)
        _check(lib().rts_scene_encode(self._h, _fp(tri), _fp(nodes) if c["n_nodes"] else None), "rts_scene_encode")
        return tri, nodes

    def nodes(self):
        nn = self.counts()["n_nodes"]
        out = {k: np.zeros(nn, np.int32) for k in ("left", "right", "n", "index")}
        aa = np.zeros((nn, 3), np.float32)
        bb = np.zeros((nn, 3), np.float32)
        _check(lib().rts_scene_nodes(self._h, _ip(out["left"]), _ip(out["right"]), _ip(out["n"]), _ip(out["index"]),
                                     _fp(aa), _fp(bb)), "rts_scene_nodes")
        out["aa"], out["bb"] = aa, bb
        return out

    def export_soa(self):
        nt = self.counts()["n_triangles"]
        arr = {k: np.zeros((nt, 3), np.float32) for k in ("p1", "p2", "p3", "n1", "n2", "n3")}
        mid = np.zeros(nt, np.int32)
        nm = C.c_int32()
        _check(lib().rts_scene_export_soa(self._h, *(None for _ in range(7)), None, C.byref(nm)), "export_soa(count)")
        mats = (RtsMaterial * max(nm.value, 1))()
        _check(lib().rts_scene_export_soa(self._h, *(_fp(arr[k]) for k in ("p1", "p2", "p3", "n1", "n2", "n3")),
                                          _ip(mid), mats, C.byref(nm)), "rts_scene_export_soa")
        arr["material_id"] = mid
        arr["materials"] = np.ctypeslib.as_array(
            C.cast(mats, C.POINTER(C.c_float)), shape=(max(nm.value, 1), 24))[: nm.value].copy()
        return arr

    def set_material(self, first: int, count: int, material: Material) -> None:
        m = material.to_c()
        _check(lib().rts_scene_set_material(self._h, first, count, C.byref(m)), "rts_scene_set_material")

    def post_bvh_index(self) -> np.ndarray:
        out = np.zeros(self.counts()["n_triangles"], np.int32)
        _check(lib().rts_scene_post_bvh_index(self._h, _ip(out)), "rts_scene_post_bvh_index")
        return out


def load_hdr(path: str) -> np.ndarray:
    """Radiance .hdr -> float32 (H, W, 3), row 0 = file's first scanline (HDRLoader order)."""
    L = lib()
    w, h = C.c_int32(), C.c_int32()
    p = _f32p()
    _check(L.rts_hdr_load(str(path).encode(), C.byref(w), C.byref(h), C.byref(p)), f"rts_hdr_load({path})")
    try:
        img = np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        L.rts_free(C.cast(p, C.c_void_p))
    return img


def hdr_cache(img: np.ndarray) -> np.ndarray:
    img = np.ascontiguousarray(img, np.float32)
    h, w, _ = img.shape
    out = np.zeros_like(img)
    _check(lib().rts_hdr_cache(_fp(img), w, h, _fp(out)), "rts_hdr_cache")
    return out


def camera(yaw: float, pitch: float, zoom: float, ratio: float) -> dict:
    out = np.zeros(17, np.float32)
    _check(lib().rts_camera(yaw, pitch, zoom, ratio, _fp(out)), "rts_camera")
    return {"front": out[0:3].copy(), "right": out[3:6].copy(), "up": out[6:9].copy(),
            "left_bottom_corner": out[9:12].copy(), "half_h": float(out[12]), "half_w": float(out[13])}


def cpu_rand_origins(seed: int, n: int) -> np.ndarray:
    """randOrigin_1..n after srand(seed) (main.cpp:190; glibc rand restated in librtscene)."""
    out = np.zeros(n, np.float32)
    _check(lib().rts_cpu_rand_origins(seed, n, _fp(out)), "rts_cpu_rand_origins")
    return out


def glibc_rand(seed: int, n: int) -> np.ndarray:
    """The first n glibc rand() values after srand(seed) (rts_glibc_rand)."""
    out = np.zeros(n, np.int32)
    _check(lib().rts_glibc_rand(seed, n, out.ctypes.data_as(C.POINTER(C.c_int))), "rts_glibc_rand")
    return out


def tri_filter(tri: np.ndarray):
    """Traversal records {p1, N.x} {R2, N.y} {R3, N.z} and the edge-filter margin (k1, k0) of the
    HIP path (csrc/common/tri_filter.h) for tri = (n, 3, 4) float32 {p1, N.x} {p2, N.y} {p3, N.z}."""
    tri = np.ascontiguousarray(tri, np.float32)
    n = tri.shape[0]
    out = np.zeros_like(tri)
    k = (C.c_double * 2)()
    fl = np.zeros(1, np.int32)
    _check(lib().rts_tri_filter(_fp(tri), n, _fp(out), k, _ip(fl)), "rts_tri_filter")
    return out, float(k[0]), float(k[1]), int(fl[0])


# rts_dev_layout's kinds and the names of their spans (one set's, for the path state), in order
LAYOUT_KINDS = ("path_state", "query", "denoise", "history", "frame_table", "camera_table", "poses",
                "tri_frames", "variance")
_SLOT_NAMES = ("s0", "s1", "s2", "s3", "s4", "s5", "ra", "rb", "sa", "sb", "res", "fin", "queue0", "queue1",
               "active0", "active1", "queue_s0", "queue_s1", "hit", "cnt")
_ROW_NAMES = ("s0", "s1", "s2", "s3", "s4", "s5", "ra", "rb", "sa", "sb", "res", "rpath")
LAYOUT_SPANS = {
    "path_state": _SLOT_NAMES + tuple("arena." + r for r in _ROW_NAMES),
    "query": ("ra", "rb", "queue", "res", "d_in", "d_out", "cnt", "zero"),
    "denoise": ("col0", "col1", "g0", "g1", "hits", "out"),
    "history": ("col0", "col1", "gp1.g0", "gp1.g1", "gp2.g0", "gp2.g1", "out"),
    "frame_table": ("loop_num", "rand_origin", "sobol", "blend_w"),
    "poses": ("tri0", "trin0", "tri1", "trin1"),
    "tri_frames": ("tf0", "tf1", "tf2"),
    "variance": ("st0", "st1", "tvar", "dvar0", "dvar1"),
}


class RtsDevSpan(C.Structure):
    _fields_ = [("off", C.c_uint64), ("bytes", C.c_uint64), ("host", C.c_int32), ("live", C.c_int32)]


def dev_layout(kind: str, n: int, m: int = 1):
    """A carved device allocation of the HIP path (csrc/common/dev_layout.h) for sizes n, m:
    (scalars, spans), the 8 scalars of rts_dev_layout (rt_scene.h; the total first) and its spans
    as dicts {name, off, bytes, host, live}.  Units are bytes, ints in the frame table and float4
    in the camera table; host is the index of the span this one lies in, or -1.  Path-state names
    carry their set ("1.s0", "1.arena.s0"), camera-table names are "dir<p>" and "org<p>"."""
    cap = 256
    scalars = (C.c_uint64 * 8)()
    spans = (RtsDevSpan * cap)()
    cnt = C.c_int32()
    _check(lib().rts_dev_layout(LAYOUT_KINDS.index(kind), n, m, scalars, spans, cap, C.byref(cnt)), "rts_dev_layout")
    if kind == "path_state":
        names = [f"{g}.{s}" for g in range(m) for s in LAYOUT_SPANS[kind]]
    elif kind == "camera_table":
        names = [f"{t}{p}" for t in ("dir", "org") for p in range(m)]
    else:
        names = list(LAYOUT_SPANS[kind])
    assert len(names) == cnt.value, (kind, len(names), cnt.value)
    return list(scalars), [dict(name=nm, off=s.off, bytes=s.bytes, host=s.host, live=s.live)
                           for nm, s in zip(names, spans)]


# rts_render_plan (csrc/common/render_plan.h): the names of its inputs (rpl::kInNames), of a group's
# and a step's values (kGroupNames, kStepNames) and of its enumerators (rpl::Trace, rpl::Shade)
PLAN_INPUTS = (
    "n_groups", "n_valid", "frames_cap", "wf_paths", "finish_pass", "pipe_finish_pass", "finish_slots", "split_kinds",
    "split_passes", "wide", "mats_emissive", "tile_cost_on", "wf_hit_cap", "wf_rows", "order_head", "pipe_depth",
    "pipe_nomem_slots", "n_cus", "trace_bpc0", "trace_bpc", "finish_bpc", "pipe_finish_bpc", "sh_sub", "sh_sub_cam",
    "sh_sub_bulk", "p1_sample_every",
    "flags", "enable_bsdf", "max_bounce", "n_left", "idle", "pipe", "pset",
    "sw_cam_shade", "sw_cam_shared", "sw_cam_shared_static", "sw_cam_miss_once", "sw_p1_lean", "sw_row_compact",
    "sw_split_cont_first", "sw_pix_split", "sw_group_head", "sw_finish_pass_g0", "sw_finish_pass_g1", "sw_finish_pass_g2",
    "sw_finish_pass_g3", "sw_row_cap")
PLAN_HEAD = ("batch_cap", "serial", "pipe_sets", "idle_matters", "admit_pipe", "nf", "G", "pix_split")
PLAN_GROUP = ("f0", "f1", "w0", "w1", "slots", "set", "stream", "fuse_blend", "split_g", "finish", "fin_pass",
              "p1_compact", "cam_shared", "cam_miss_once", "p1_lean", "row_compact", "row_cap", "blend", "n_steps")
PLAN_STEP = ("finisher", "fgrid", "split", "split_out", "cam_n", "cam_shared", "n_trace", "trace0", "trace1",
             "trace_grid", "classify", "classify_grid", "p1_count", "p1_grid0", "p1_grid1", "shade", "shade_grid")
PLAN_TRACE = ("CAM_SMALL", "P1_SMALL", "REG_SMALL", "P1_SHADOW", "P1_CONT_LEAN", "P1_CONT", "SHADOW", "CONT",
              "CAM_CW", "P1_CW", "REG_CW", "CAM_CB", "P1_CB", "REG_CB", "CAM_W", "P1_W", "REG_W", "CAM_B", "P1_B",
              "REG_B")
PLAN_SHADE = ("PLAIN", "BULK", "CAM", "FUSED", "CAM_LEAN", "BULK_LEAN")


def render_plan_values(inputs: dict, max_values: int = 4096) -> list:
    """rts_render_plan's output values (rt_scene.h) for `inputs`, a dict with every name of
    PLAN_INPUTS."""
    assert len(inputs) == len(PLAN_INPUTS), sorted(set(inputs) ^ set(PLAN_INPUTS))
    vin = (C.c_int64 * len(PLAN_INPUTS))(*[int(inputs[k]) for k in PLAN_INPUTS])
    out = (C.c_int64 * max_values)()
    cnt = C.c_int32()
    _check(lib().rts_render_plan(vin, len(PLAN_INPUTS), out, max_values, C.byref(cnt)), "rts_render_plan")
    return out[:cnt.value]


def render_plan(inputs: dict, max_values: int = 4096) -> dict:
    """What one wavefront batch launches for `inputs` (render_plan_values, by name): the PLAN_HEAD
    values and "groups", a list of dicts with the PLAN_GROUP values and "steps", a list of dicts of
    PLAN_STEP values (all ints)."""
    return decode_plan(render_plan_values(inputs, max_values))


def decode_plan(v: list) -> dict:
    plan = dict(zip(PLAN_HEAD, v), groups=[])
    at = len(PLAN_HEAD)
    for _ in range(plan["G"]):
        g = dict(zip(PLAN_GROUP, v[at:at + len(PLAN_GROUP)]), steps=[])
        at += len(PLAN_GROUP)
        for _ in range(g["n_steps"]):
            g["steps"].append(dict(zip(PLAN_STEP, v[at:at + len(PLAN_STEP)])))
            at += len(PLAN_STEP)
        plan["groups"].append(g)
    assert at == len(v), (at, len(v))
    return plan


@dataclasses.dataclass
class CompiledScene:
    """What rt_set_scene uploads and commits for a scene (scn::Compiled), or why it refuses it."""
    rc: int                 # rt_set_scene's code: 0, RT_ERR_ARG (-1) or RT_ERR_LIMIT (-6)
    err: str
    arrays: dict            # tri, trx, trin, hrec (n, 4) float32; mats (n, 32); nodes, qnodes; tri_mat
    scalars: dict


def _compiled(rc: int, h, keep: bool = False) -> CompiledScene:
    L = lib()
    try:
        v = RtsCompiledView()
        _check(L.rts_compiled_get(h, C.byref(v)), "rts_compiled_get")

        def take(ptr, n, dtype, ctype):
            if n == 0:
                return np.zeros(0, dtype)
            buf = C.cast(ptr, C.POINTER(ctype * (n * np.dtype(dtype).itemsize // C.sizeof(ctype)))).contents
            return np.frombuffer(buf, dtype=dtype, count=n).copy()
        a = {k: take(getattr(v, k), getattr(v, f"n_{k}_f"), np.float32, C.c_float).reshape(-1, 32 if k == "mats" else 4)
             for k in ("tri", "trx", "trin", "hrec", "mats")}
        a["nodes"] = take(v.nodes, v.n_nodes, BNODE_DTYPE, C.c_float)
        a["qnodes"] = take(v.qnodes, v.n_qnodes, WNODE_DTYPE, C.c_float)
        a["tri_mat"] = take(v.tri_mat, v.n_tri_mat, np.int32, C.c_int32)
        sc = {k: getattr(v, k) for k in ("cull_R", "cull_K", "cull_off", "tri_k1", "tri_k0", "n_tri", "n_mats", "root",
                                         "has_scene", "depth", "qroot", "qdepth", "tri_flagged")}
        sc["wide"] = bool(v.wide)
        return CompiledScene(rc, (v.err or b"").decode(), a, sc)
    finally:
        if not keep:
            L.rts_compiled_free(h)


def split_vertices(p, n, count=None):
    """(count, 3, 3) positions and normals [triangle, vertex, xyz] -> the six float[3 * count] arrays
    p1, p2, p3, n1, n2, n3 of the geometry update calls."""
    p = np.asarray(p, np.float32).reshape(-1, 3, 3)
    n = np.asarray(n, np.float32).reshape(-1, 3, 3)
    if p.shape != n.shape or (count is not None and p.shape[0] != count):
        raise ValueError("positions and normals must be (count, 3, 3)")
    return [np.ascontiguousarray(a[:, k]) for a in (p, n) for k in range(3)]


class CompiledHandle:
    """A compiled scene that stays alive, for the geometry update's CPU model
    (rts_compiled_update_geometry = scn::update_geometry, the definition the device follows)."""

    def __init__(self, tri_enc: np.ndarray, node_enc: np.ndarray, *, rebuild=True, greedy=False, bfs=True, wide=True):
        t = np.ascontiguousarray(tri_enc, np.float32)
        n = np.ascontiguousarray(node_enc, np.float32)
        self._h = C.c_void_p()
        self.rc = lib().rts_compile_scene_encoded(_fp(t), t.shape[0], _fp(n), n.shape[0],
                                                  _ip(_options(rebuild, greedy, bfs, wide)), C.byref(self._h))
        if not self._h.value:
            raise RuntimeError(f"rts_compile_scene_encoded failed with {self.rc}")

    def __del__(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().rts_compiled_free(self._h)
            self._h = None

    def snapshot(self) -> CompiledScene:
        """Copies of the arrays and scalars as they stand."""
        return _compiled(self.rc, self._h, keep=True)

    def update_geometry(self, tri_index, p, n, first: int = 0, count: Optional[int] = None) -> int:
        """tri_index: int array or None (then triangles first .. first + count); p, n: (count, 3, 3).
        Returns the code (0 or RT_ERR_ARG); the reason is snapshot().err."""
        idx = None if tri_index is None else np.ascontiguousarray(tri_index, np.int32)
        if count is None:
            count = len(idx) if idx is not None else np.asarray(p).reshape(-1, 3, 3).shape[0]
        arrs = split_vertices(p, n) if p is not None else [None] * 6
        return lib().rts_compiled_update_geometry(self._h, _ip(idx), int(first), int(count), *[_fp(a) for a in arrs])

    def filter_state(self) -> dict:
        out = (C.c_double * 5)()
        _check(lib().rts_compiled_filter_state(self._h, out), "rts_compiled_filter_state")
        return dict(zip(("s_cap", "sc_cap", "s_max", "sc_max", "c_min"), list(out)))

    def refit_plan(self) -> dict:
        """leaves (n, 4) int32 {ref, binary parent * 2 + side, 4-wide parent * 4 + slot, 0}; blist / qlist
        the internal nodes by height with offsets boff / qoff (height h: list[off[h - 1]:off[h]])."""
        v = RtsRefitPlanView()
        _check(lib().rts_refit_plan(self._h, C.byref(v)), "rts_refit_plan")

        def take(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        return {"leaves": take(v.leaves, 4 * v.n_leaves).reshape(-1, 4), "blist": take(v.blist, v.n_blist),
                "boff": take(v.boff, v.n_boff), "qlist": take(v.qlist, v.n_qlist), "qoff": take(v.qoff, v.n_qoff)}


def _options(rebuild, greedy, bfs, wide):
    return np.array([rebuild, greedy, bfs, wide], np.int32)


def compile_scene(soa, nodes: Optional[dict] = None, *, rebuild=True, greedy=False, bfs=True, wide=True) -> CompiledScene:
    """The HIP path's scene compiler (csrc/common/scene_compile.h, the code rt_set_scene runs) on
    soa / nodes as Renderer.set_scene_soa takes them, or on a ready RtSceneSoa."""
    from .renderer import marshal_scene_soa
    s, _keep = (soa, None) if nodes is None else marshal_scene_soa(soa, nodes)
    h = C.c_void_p()
    rc = lib().rts_compile_scene(C.byref(s), _ip(_options(rebuild, greedy, bfs, wide)), C.byref(h))
    if not h.value:
        raise RuntimeError(f"rts_compile_scene failed with {rc}")
    return _compiled(rc, h)


def compile_scene_encoded(tri_enc: np.ndarray, node_enc: np.ndarray, *, rebuild=True, greedy=False, bfs=True,
                          wide=True) -> CompiledScene:
    """The same from the reference's encodings, as Renderer.set_scene_encoded takes them."""
    t = np.ascontiguousarray(tri_enc, np.float32)
    n = np.ascontiguousarray(node_enc, np.float32)
    h = C.c_void_p()
    rc = lib().rts_compile_scene_encoded(_fp(t), t.shape[0], _fp(n), n.shape[0],
                                         _ip(_options(rebuild, greedy, bfs, wide)), C.byref(h))
    if not h.value:
        raise RuntimeError(f"rts_compile_scene_encoded failed with {rc}")
    return _compiled(rc, h)


def write_png(path: str, rgb: np.ndarray) -> None:
    """8-bit RGB (H, W, 3), row 0 = top -> PNG (rts_write_png, SaveFrame's stbi_write_png)."""
    a = np.ascontiguousarray(rgb, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected an (H, W, 3) uint8 image")
    _check(lib().rts_write_png(str(path).encode(), a.shape[1], a.shape[0], a.ctypes.data_as(C.POINTER(C.c_uint8))),
           "rts_write_png")
