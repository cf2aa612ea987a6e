"""Scenes with per-vertex colours (`mesh_attribute` reflectances; test infrastructure of tests/test_vertex_color.py and
tests/test_gpu_vertex_color.py): A, a tessellated floor without texture coordinates under test_texture_adjoint.texture_scene's wall
and area light; B, test_envpose_adjoint's ball scene with a diffuse per-vertex ball; the reparameterised pass's plane with
per-vertex colours in the place of its bitmap."""
import numpy as np

from _scenes import quad, sensor
from _texture_host import on_host_texture
from epsm_mitsuba3_amd import scene as S


def grid(n=3, half=2.0, z=0.0):
    """An n x n vertex grid over [-half, half]^2 at height z (normal +z): (n - 1)^2 cells of two triangles, rows along y."""
    t = np.linspace(-half, half, n)
    v = np.array([[x, y, z] for y in t for x in t], float)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
    return v, np.array(f)


def vertex_colours(n, seed=0):
    return (0.2 + 0.7 * np.random.default_rng(seed).random((n, 3))).astype(np.float32)


def attribute(scale=None):
    r = {"type": "mesh_attribute", "name": "vertex_color"}
    if scale is not None:
        r["scale"] = scale
    return r


def scene_a(device="cpu", res=12, spp=32, colours=None, n=3, reflectance=None, scale=None, wall_colour=(0.2, 0.5, 0.7), cam=None,
            wall_reflectance=None):
    """Scene A: the floor of texture_scene as an n x n vertex grid without texture coordinates, its reflectance the grid's
    vertex_color (or ``reflectance``, any other one); the same wall and area light."""
    fv, ff = grid(n, 2.0)
    wv = np.array([[-2, 2, 0], [2, 2, 0], [2, 2, 2.5], [-2, 2, 2.5]], float)
    wf = np.array([[0, 2, 1], [0, 3, 2]])
    lv, lf = quad(2.2, 0.4, up=False)
    floor = {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True,
             "bsdf": {"type": "diffuse", "reflectance": attribute(scale) if reflectance is None else reflectance}}
    if reflectance is None:
        floor["vertex_color"] = vertex_colours(n * n) if colours is None else colours
    d = {"type": "scene",
         "cam": cam or sensor([0.0, -3.5, 1.6], [0, 0.5, 0.5], up=(0, 0, 1), res=res, spp=spp, rfilter="gaussian"),
         "floor": floor,
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [30.0, 25.0, 20.0]}}}}
    d["wall"] = {"type": "mesh", "vertices": wv, "faces": wf, "face_normals": True,
                 "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": wall_reflectance or {"type": "rgb", "value": list(wall_colour)}}}}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_texture(sc)
    sc.tracer = "mega"
    return sc


def ball_mesh():
    from epsm_mitsuba3_amd.exp.clutter import icosphere
    bv, bf = icosphere(1)
    return bv * 0.7 + np.array([0.0, 0.0, 0.7]), bf, bv


def scene_b(device="cpu", res=16, spp=4, colours=None, tracer="mega", tilt=0.0):
    """Scene B: test_envpose_adjoint.env_scene("ball") -- 80 triangles of a ball on a 2-triangle floor under its envmap -- with a
    diffuse ball whose reflectance is its vertex_color (smooth normals: curved shading).  ``tilt``: the ball turned by so many
    degrees about an oblique axis through its centre -- as it stands, eight of its triangles have a geometric normal whose z is
    exactly zero, the value whose sign coordinate_system() branches on (cross_rounded, epsm_trace_core.h)."""
    from test_envpose_adjoint import env_scene
    v, f, _ = ball_mesh()
    if tilt:
        c = np.array([0.0, 0.0, 0.7])
        v = (v - c) @ S.rotate([0.3, 1.0, 0.2], tilt)[:3, :3].T + c
    ball = {"type": "mesh", "vertices": v, "faces": f, "face_normals": False, "vertex_color": vertex_colours(v.shape[0], 3) if colours is None else colours,
            "bsdf": {"type": "diffuse", "reflectance": attribute()}}
    sc = env_scene("ball", "16x8", device=device, res=res, spp=spp, extra={"ball": ball})
    if str(device) == "cpu":
        on_host_texture(sc)
    sc.tracer = tracer
    return sc


def plane_colours(v):
    """Colours with structure over the plane: a smooth function of the vertex position (one per channel)."""
    x, y = v[:, 0], v[:, 1]
    return np.stack([0.5 + 0.35 * np.sin(2.0 * x + 0.3), 0.45 + 0.3 * np.cos(1.5 * y) * np.sin(1.2 * x), 0.5 + 0.3 * np.cos(1.7 * x - 0.4)], 1).astype(np.float32)


def vertex_plane(theta=0.0, res=16, spp=16, device="cpu", half=2.0, n=5, bump=0.0):
    """_reparam_scenes' textured_plane_constant (half 2: its silhouette is in view) or textured_plane_fills_the_view (half 4: only
    the colours slide) with an n x n vertex grid and per-vertex colours in the place of the bitmap; ``theta`` translates the plane
    along x, in its own plane, colours and all; ``bump`` moves the grid's centre vertex alone along x (the plane stays flat: only
    the colours inside the centre's six triangles slide)."""
    v, f = grid(n, half)
    colours = plane_colours(v)
    v[(n * n) // 2, 0] += bump
    cam = sensor([0, 0, 4], [0, 0, 0], up=(0, 1, 0), fov=28.8415, res=res, spp=spp, rfilter="gaussian", sample_border=True)
    d = {"type": "scene", "cam": cam,
         "plane": {"type": "mesh", "vertices": v + np.array([theta, 0.0, 0.0]), "faces": f, "face_normals": True, "vertex_color": colours,
                   "bsdf": {"type": "diffuse", "reflectance": attribute()}},
         "light": {"type": "constant"}}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_texture(sc)
    sc.tracer = "mega"
    return sc

