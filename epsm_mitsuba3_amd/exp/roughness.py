"""Roughness experiment for the colour adjoint (``prb`` / ``prb_reparam`` / the second phase of the hybrid scheme): the plate of
``exp/plate.py`` under its light, the target rendered at one roughness, the optimisation started at another; Adam on ``alpha`` with
the clamp of EPSM/exp/glossyball.py:264 (0.001 ... 0.5) and the L2 image loss of the reference's non-EPSM branch.  The size of a
highlight is fitted from the image alone -- the roughness adjoint, Scene.attach_alpha + epsm_trace_paths_bsdf_backward:

    python -m epsm_mitsuba3_amd.optim prb roughness
    python -m epsm_mitsuba3_amd.optim manifold_hybrid roughness      # `thres` iterations of manifold, then prb_reparam

``alpha_grads`` keeps d loss / d alpha of every iteration of the last run (after ``thres`` they come from the colour adjoint).
"""
import torch

from . import plate as _plate

it = 40
spp = 16
resolution = 64
thres = 2
max_depth = 3
match_res = 32
lr = 0.01

ALPHA_TARGET = 0.08
ALPHA_START = 0.2
ALPHA_MIN, ALPHA_MAX = 0.001, 0.5

alpha_grads = []


def load_scene(device="cuda", alpha=ALPHA_START, **scene_kw):
    sc = _plate.load_scene(device, **scene_kw)
    sc.set_alpha("plate.bsdf", alpha)
    sc.tracer = "mega"
    return sc


def gt_scene(device="cuda"):
    return load_scene(device, ALPHA_TARGET)


def optim_settings(scene):
    slot = scene.attach_alpha("plate.bsdf")
    opt = {"alpha": torch.tensor(ALPHA_START, device=scene.device, requires_grad=True)}
    del alpha_grads[:]

    def apply_transformation(scene_, opt_):
        with torch.no_grad():
            opt_["alpha"].clamp_(ALPHA_MIN, ALPHA_MAX)
        scene_.set_alpha("plate.bsdf", float(opt_["alpha"].detach()))

    def backward(opt_, params):
        alpha_grads.append(float(params.alpha[slot]))
        opt_["alpha"].grad = params.alpha[slot].clone().reshape(())

    def output(opt_):
        return abs(float(opt_["alpha"].detach()) - ALPHA_TARGET)

    return opt, apply_transformation, backward, output
