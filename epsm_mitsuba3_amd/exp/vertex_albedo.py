"""Per-vertex albedo experiment (``prb`` / ``prb_reparam``): recover the ``vertex_color`` attribute of a lit, tessellated ball
without texture coordinates -- the ``mesh_attribute`` reflectance of its diffuse BSDF (``'ball.vertex_color'``) -- from one target
image, with the texel adjoint (Scene.attach_vertex_color, epsm_trace_paths_texture_backward: a footprint of three vertices) and the
L2 image loss of the reference's non-EPSM branch:

    python -m epsm_mitsuba3_amd.optim prb vertex_albedo
"""
import numpy as np
import torch

from ..scene import Scene, look_at
from .clutter import icosphere

it = 40
spp = 32
resolution = 48
thres = 3
max_depth = 3
match_res = 16
lr = 0.05

_EYE = np.array([0.0, -1.0, 4.0])
_V, _F = icosphere(2)                            # 162 vertices, 320 triangles, radius 1 about the origin


def _target():
    """A smooth pattern of three phases over the ball: something each vertex colour must move towards."""
    x, y, z = _V[:, 0], _V[:, 1], _V[:, 2]
    c = np.stack([0.5 + 0.35 * np.sin(3.0 * x + 1.0), 0.5 + 0.35 * np.sin(3.0 * y - 0.5), 0.5 + 0.35 * np.cos(2.5 * (x + z))], 1)
    return c.astype(np.float32)


_START = np.full((_V.shape[0], 3), 0.5, np.float32)


def visible():
    """The vertices the sensor sees well: the ball is convex, so those whose normal points at the eye (cosine > 0.3)."""
    d = _EYE[None] - _V
    cos = (d * _V).sum(1) / np.linalg.norm(d, axis=1)          # (the vertex normal of the unit ball is the vertex)
    return torch.from_numpy(cos > 0.3)


def _sensor(res, n):
    return {"type": "perspective", "fov": 35, "near_clip": 0.01, "far_clip": 100.0,
            "to_world": look_at(list(_EYE), [0, 0, 0], [0, 1, 0]),
            "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "gaussian"}},
            "sampler": {"type": "independent", "sample_count": n}}


def load_scene(device="cuda", colours=None):
    lv = np.array([[1.5, -2.5, 3.5], [2.5, -2.5, 3.5], [2.5, -1.5, 3.5], [1.5, -1.5, 3.5]], float)       # (out of view)
    lf = np.array([[0, 2, 1], [0, 3, 2]])
    d = {"type": "scene", "sensor0": _sensor(resolution, spp), "sensor1": _sensor(resolution, spp), "sensor2": _sensor(match_res, 8),
         "ball": {"type": "mesh", "vertices": _V, "normals": _V, "faces": _F, "vertex_color": _START if colours is None else colours,
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "mesh_attribute", "name": "vertex_color"}}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 20.0}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.5}}}
    sc = Scene.from_dict(d, device=device)
    sc.tracer = "mega"
    return sc


def gt_scene(device="cuda"):
    return load_scene(device, _target())


def optim_settings(scene):
    slot = scene.attach_vertex_color("ball")
    opt = {"ball": torch.tensor(_START, device=scene.device, requires_grad=True)}
    target, seen = torch.from_numpy(_target()), visible()

    def apply_transformation(scene_, opt_):
        scene_.set_texture(slot, opt_["ball"].detach().clamp(0.0, 1.0))

    def backward(opt_, params):
        opt_["ball"].grad = params.texture(slot)[:, 0].clone()

    def output(opt_):
        """Mean absolute colour error over the vertices visible in the target."""
        return float((opt_["ball"].detach().cpu() - target)[seen].abs().mean())

    return opt, apply_transformation, backward, output
