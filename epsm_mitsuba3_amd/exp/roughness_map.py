"""Roughness-map experiment for the colour adjoint (``prb`` / ``prb_reparam`` without attached geometry): a flat rough plate under
an area light and a dim sky whose ``alpha`` is an 8 x 8 ``nearest`` bitmap (``'plate.bsdf.alpha.data'``).  The target is rendered
with a two-level checker, the optimisation starts from a uniform map in between; Adam on the 64 texels, clamped to 0.02 ... 0.7,
with the L2 image loss of the reference's non-EPSM branch.  The blur of the light's reflection is fitted texel by texel from the
image alone -- the roughness-map adjoint, Scene.attach_texture('<bsdf>.alpha.data') + epsm_trace_paths_alpha_texture_backward:

    python -m epsm_mitsuba3_amd.optim prb roughness_map
"""
import numpy as np
import torch

from ..scene import Scene, look_at

it = 40
spp = 32
resolution = 48
thres = 10000
max_depth = 2
match_res = 16
lr = 0.01

_N = 8
ALPHA_LOW, ALPHA_HIGH, ALPHA_START = 0.1, 0.3, 0.2
ALPHA_MIN, ALPHA_MAX = 0.02, 0.7


def _target():
    j, i = np.meshgrid(np.arange(_N), np.arange(_N), indexing="ij")
    return np.where((i + j) % 2 == 0, ALPHA_LOW, ALPHA_HIGH).astype(np.float32)


_START = np.full((_N, _N), ALPHA_START, np.float32)


def _sensor(res, n):
    return {"type": "perspective", "fov": 45, "near_clip": 0.01, "far_clip": 100.0,
            "to_world": look_at([0.0, -1.5, 2.0], [0, 0, 0], [0, 0, 1]),
            "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "gaussian"}},
            "sampler": {"type": "independent", "sample_count": n}}


def load_scene(device="cuda", texels=None):
    pv = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], float)
    pf = np.array([[0, 1, 2], [0, 2, 3]])
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    # (above the camera, out of its view: where the plate mirrors most of the camera's rays to)
    lv = np.array([[-1.6, 0.3, 2.5], [1.6, 0.3, 2.5], [1.6, 3.4, 2.5], [-1.6, 3.4, 2.5]], float)
    alpha = {"type": "bitmap", "bitmap": _START if texels is None else texels, "filter_type": "nearest"}
    d = {"type": "scene", "sensor0": _sensor(resolution, spp), "sensor1": _sensor(resolution, spp), "sensor2": _sensor(match_res, 8),
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "texcoords": uv, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": alpha, "sample_visible": False}},
         "light": {"type": "mesh", "vertices": lv, "faces": pf[:, ::-1], "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 6.0}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.2}}}
    sc = Scene.from_dict(d, device=device)
    sc.tracer = "mega"
    return sc


def gt_scene(device="cuda"):
    return load_scene(device, _target())


def optim_settings(scene):
    slot = scene.attach_texture("plate.bsdf.alpha.data")
    opt = {"alpha": torch.tensor(_START, device=scene.device, requires_grad=True)}
    target = torch.from_numpy(_target())

    def apply_transformation(scene_, opt_):
        with torch.no_grad():
            opt_["alpha"].clamp_(ALPHA_MIN, ALPHA_MAX)
        scene_.set_texture(slot, opt_["alpha"].detach())

    def backward(opt_, params):
        opt_["alpha"].grad = params.texture(slot).clone()

    def output(opt_):
        """Mean absolute texel error of the roughness map."""
        return float((opt_["alpha"].detach().cpu() - target).abs().mean())

    return opt, apply_transformation, backward, output
