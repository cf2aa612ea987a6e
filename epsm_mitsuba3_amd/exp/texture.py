"""Texture experiment for the second phase of the hybrid scheme (``prb`` / ``prb_reparam``): recover the 16 x 16 bilinear
``bitmap`` reflectance of a diffuse floor (``'floor.bsdf.reflectance.data'``) from a target image, with the texel adjoint
(Scene.attach_texture, epsm_trace_paths_texture_backward) and the L2 image loss of the reference's non-EPSM branch:

    python -m epsm_mitsuba3_amd.optim prb texture
"""
import numpy as np
import torch

from ..scene import Scene, look_at

it = 40
spp = 32
resolution = 48
thres = 3
max_depth = 3
match_res = 16
lr = 0.05

_N = 16


def _target():
    """A checker of two colours with a smooth ramp: something the floor's texels must each move towards."""
    j, i = np.meshgrid(np.arange(_N), np.arange(_N), indexing="ij")
    chk = ((i // 4 + j // 4) % 2)[..., None].astype(np.float32)
    a, b = np.array([0.8, 0.3, 0.2], np.float32), np.array([0.2, 0.5, 0.8], np.float32)
    return (chk * a + (1 - chk) * b) * (0.7 + 0.3 * i[..., None] / (_N - 1))


_START = np.full((_N, _N, 3), 0.5, np.float32)


def _sensor(res, n):
    return {"type": "perspective", "fov": 45, "near_clip": 0.01, "far_clip": 100.0,
            "to_world": look_at([0.0, -1.0, 4.0], [0, 0, 0], [0, 1, 0]),
            "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "gaussian"}},
            "sampler": {"type": "independent", "sample_count": n}}


def load_scene(device="cuda", texels=None):
    fv = np.array([[-1.5, -1.5, 0], [1.5, -1.5, 0], [1.5, 1.5, 0], [-1.5, 1.5, 0]], float)
    ff = np.array([[0, 1, 2], [0, 2, 3]])
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    lv = np.array([[1.5, -0.5, 2.5], [2.5, -0.5, 2.5], [2.5, 0.5, 2.5], [1.5, 0.5, 2.5]], float)       # (out of view)
    d = {"type": "scene", "sensor0": _sensor(resolution, spp), "sensor1": _sensor(resolution, spp), "sensor2": _sensor(match_res, 8),
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "texcoords": uv, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "bitmap", "bitmap": _START if texels is None else texels}}},
         "light": {"type": "mesh", "vertices": lv, "faces": ff[:, ::-1], "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 20.0}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.3}}}
    sc = Scene.from_dict(d, device=device)
    sc.tracer = "mega"
    return sc


def gt_scene(device="cuda"):
    return load_scene(device, _target())


def optim_settings(scene):
    slot = scene.attach_texture("floor.bsdf.reflectance.data")
    opt = {"floor": torch.tensor(_START, device=scene.device, requires_grad=True)}
    target = torch.from_numpy(_target())

    def apply_transformation(scene_, opt_):
        scene_.set_texture(slot, opt_["floor"].detach().clamp(0.02, 0.98))

    def backward(opt_, params):
        opt_["floor"].grad = params.texture(slot).clone()

    def output(opt_):
        """Mean absolute texel error of the floor."""
        return float((opt_["floor"].detach().cpu() - target).abs().mean())

    return opt, apply_transformation, backward, output
