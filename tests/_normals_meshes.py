"""Meshes and the small scene of the tests of the recomputed normals' derivative (tests/test_normals_adjoint.py,
tests/test_gpu_normals_adjoint.py): float64 vertices, int64 faces."""
import contextlib
import ctypes

import numpy as np


@contextlib.contextmanager
def one_thread():
    """The host build of the tracer sums its float atomics in thread order: with one OpenMP thread two calls give the same bits."""
    omp = ctypes.CDLL("libgomp.so.1")
    omp.omp_get_max_threads.restype = ctypes.c_int
    n = omp.omp_get_max_threads()
    omp.omp_set_num_threads(1)
    try:
        yield
    finally:
        omp.omp_set_num_threads(n)


def icosphere(subdivisions, radius=1.0, center=(0.0, 0.0, 0.0)):
    """V = 10 * 4^s + 2: 42, 162, 642."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(x, float) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = g
    return np.asarray(v) * radius + np.asarray(center, float), np.asarray(f, np.int64)


def bump_grid(n, height=0.25):
    """An open n x n grid over the unit square with a smooth bump: boundary vertices of valence 1, 2 and 3."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x, y = i.ravel() / (n - 1), j.ravel() / (n - 1)
    v = np.stack([x, y, height * np.exp(-((x - 0.4) ** 2 + (y - 0.6) ** 2) / 0.08)], 1)
    f = []
    for a in range(n - 1):
        for b in range(n - 1):
            k = a * n + b
            f += [[k, k + n, k + 1], [k + 1, k + n, k + n + 1]]
    return v, np.asarray(f, np.int64)


def fan(valence=100):
    """A hub of the given (even) valence: the rim zigzags by +-h so that every triangle is close to equilateral -- the hub's
    angles sum to valence * 60 degrees, a ruffle."""
    h = 3.0 ** -0.5
    ph = 2 * np.pi * np.arange(valence) / valence
    rim = np.stack([np.cos(ph), np.sin(ph), h * (1 - 2 * (np.arange(valence) % 2))], 1)
    v = np.concatenate([np.zeros((1, 3)), rim])
    f = [[0, 1 + k, 1 + (k + 1) % valence] for k in range(valence)]
    return v, np.asarray(f, np.int64)


def corner_angles(v, f):
    p = v[f]
    out = []
    for i in range(3):
        d0, d1 = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        out.append(np.degrees(np.arccos((d0 * d1).sum(1) / np.linalg.norm(d0, axis=1) / np.linalg.norm(d1, axis=1))))
    return np.stack(out, 1)


def cut_mesh():
    """Next to the valid triangles of a small grid: a triangle that repeats a vertex, a zero-area sliver of three collinear
    points, an isolated vertex, a vertex whose only triangle is degenerate.  Returns (v, f, isolated, only_degenerate)."""
    v, f = bump_grid(4)
    n = v.shape[0]
    extra = np.array([[2.0, 0.0, 0.0],                 # n: isolated
                      [3.0, 0.0, 0.0],                 # n + 1: its only triangle repeats a vertex
                      [0.0, 2.0, 0.0], [0.5, 2.0, 0.0], [1.0, 2.0, 0.0]])   # n + 2 .. n + 4: collinear
    more = [[0, 5, 5],                                 # repeats a vertex, at two vertices that have valid triangles too
            [n + 1, 1, 1],                             # the only triangle of n + 1
            [n + 2, n + 3, n + 4],                     # the sliver: the only triangle of its three vertices
            [2, n + 3, n + 4]]                         # a valid triangle at two of the sliver's vertices
    return np.concatenate([v, extra]), np.concatenate([f, np.asarray(more, np.int64)]), n, n + 1


GLOSSY = {"type": "roughconductor", "alpha": 0.05}      # prb_reparam carries no normal gradient through a delta lobe: a glossy mirror


def mirror_scene(res=16, spp=8, device="cpu", bsdf=GLOSSY, subdivisions=2, border=True, **scene_kw):
    """A smoothly shaded mirror (or glass) sphere in front of a lit diffuse plane; the sphere's normals are computed, not given.
    ``bsdf``: the glossy mirror for ``prb_reparam``, ``{"type": "conductor"}`` / ``{"type": "dielectric"}`` for the manifold
    integrators."""
    from _reparam_scenes import rect
    from _scenes import sensor
    from epsm_mitsuba3_amd import scene as S
    d = {"type": "scene", "cam": sensor([0, 0, 4], [0, 0, 0], up=(0, 1, 0), fov=28.8415, res=res, spp=spp, rfilter="gaussian", sample_border=border)}
    v, f = rect(3.0, (0, 0, -1.0))
    d["plane"] = {"type": "mesh", "vertices": v, "faces": f, "face_normals": True,
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.6, 0.5]}}}
    v, f = icosphere(subdivisions, 0.6, (0.1, 0.05, 0.2))
    d["sphere"] = {"type": "mesh", "vertices": v, "faces": f, "bsdf": dict(bsdf)}
    v, f = rect(0.7, (1.5, 2.0, 3.0))
    d["light"] = {"type": "mesh", "vertices": v, "faces": f[:, ::-1], "face_normals": True,
                  "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [20.0, 20.0, 20.0]}}}
    sc = S.Scene.from_dict(d, device=device, **scene_kw)
    if str(device) == "cpu":
        from _forward_host import on_host_forward
        on_host_forward(sc)
    sc.tracer = "mega"
    return sc


def bump_scene(res=32, spp=64, device="cpu"):
    """No discontinuity in view: a smoothly shaded glossy sheet with a bump, larger than the image, under a small area light (the
    `receiver_along_normal` configuration of tests/_reparam_scenes.py with the plane made a curved glossy mirror)."""
    from _reparam_scenes import rect
    from _scenes import sensor
    from epsm_mitsuba3_amd import scene as S
    d = {"type": "scene", "cam": sensor([0, 0, 4], [0, 0, 0], up=(0, 1, 0), fov=28.8415, res=res, spp=spp, rfilter="gaussian", sample_border=True)}
    v, f = bump_grid(17, height=0.05)
    v = (v - np.array([0.5, 0.5, 0.0])) * np.array([6.0, 6.0, 6.0])
    d["mirror"] = {"type": "mesh", "vertices": v, "faces": f, "bsdf": {"type": "roughconductor", "alpha": 0.3}}
    v, f = rect(0.5, (0.8, 0.3, 2.0))
    d["light"] = {"type": "mesh", "vertices": v, "faces": f[:, ::-1], "face_normals": True,
                  "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [40.0, 40.0, 40.0]}}}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        from _forward_host import on_host_forward
        on_host_forward(sc)
    sc.tracer = "mega"
    return sc


def bump_motion(sc):
    """d position / d theta of the one-parameter bulge: every vertex of the sheet moves along z by a smooth bump of its (x, y) --
    no rigid motion."""
    import torch
    x = sc.vertex_positions("mirror")
    dz = torch.exp(-((x[:, 0] - 0.3) ** 2 + (x[:, 1] + 0.2) ** 2) / 0.5)
    return torch.stack([torch.zeros_like(dz), torch.zeros_like(dz), dz], 1)
