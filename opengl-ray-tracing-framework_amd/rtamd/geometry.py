"""Vertex data for Renderer.update_geometry: one object of a scene under a new transform."""
from __future__ import annotations

import numpy as np

from . import configs as cf
from . import scene_lib as sl


def moved_object(sd: "cf.SceneData", obj: int, rotate, translate, scale):
    """Object number `obj` of sd (a cf.SceneData built by cf.build_scene / cf.config_scene) under
    the transform (rotate in degrees, translate, scale) instead of its own.

    Returns (tri_index, p, n): the post-BVH indices of its triangles (int32) and their positions and
    normals, (count, 3, 3) float32 [triangle, vertex, xyz], ready for Renderer.update_geometry.
    The triangles come from the host code of a fresh scene build: rts_scene_add_mesh on a scratch
    scene, read back before any BVH build (so in pre-BVH order), mapped through the scene's
    post-BVH index."""
    if not sd.objects or sd.pre_to_post is None:
        raise ValueError("the scene does not record its objects (build it with configs.build_scene)")
    o = sd.objects[obj]
    mat = o.material if isinstance(o.material, sl.Material) else cf.MATERIALS[o.material]
    s = sl.Scene()
    first, end = s.add_mesh(cf.load_mesh(o.mesh), mat, rotate, translate, scale, o.smooth)
    soa = s.export_soa()
    lo, hi = sd.ranges[obj]
    if hi - lo != end - first:
        raise ValueError("the object's triangle count changed")
    p = np.stack([soa[k][first:end] for k in ("p1", "p2", "p3")], axis=1)
    n = np.stack([soa[k][first:end] for k in ("n1", "n2", "n3")], axis=1)
    return np.ascontiguousarray(sd.pre_to_post[lo:hi], np.int32), np.ascontiguousarray(p), np.ascontiguousarray(n)
