"""Recover the index of refraction of the glass from its caustic: the `caustic_sphere` configuration (an open diffuse box, a
smoothly shaded glass sphere above the floor, a small area light above it) with the light fixed and the sphere's ``int_ior``
unknown.  The focus of the caustic on the floor moves with the IOR; `manifold_caustic` carries the matcher's pixel motion through
the two refractions to d / d eta_k of both (epsm_cp_core.h, ``geta``), the tracer logs d eta / d int_ior with each of them, and the
sum arrives in ``ParamGrads.alpha[slot]`` of ``Scene.attach_ior`` (EPSM_OPT_IOR_GRADS).  The reference has no such
gradient: ``eta`` enters its ``calc_grad`` as a constant."""
import torch

from . import caustic_sphere as _cs

it = 60
spp = 32
resolution = 64
thres = 10000
max_depth = 5
match_res = 32
lr = 0.01
# samples per pixel of the backward pass (optim.run; the integrators' default is the reference's 8): a focusing sphere puts single
# paths close to the +-0.1 clamp of the per-vertex terms, and at 8 spp a handful of them outweighs the rest of the wavefront
# (MEASUREMENTS.md 32)
backward_spp = 512

GLASS = "ball.bsdf"
START_IOR, TARGET_IOR = 1.45, 1.6
_MIN_IOR = 1.05                       # (the surrounding medium has 1.0: int_ior == ext_ior is no refraction at all)


def load_scene(device="cuda", int_ior=START_IOR):
    scene = _cs.load_scene(device)
    scene.set_ior(GLASS, int_ior)
    return scene


def gt_scene(device="cuda"):
    return load_scene(device, TARGET_IOR)


def optim_settings(scene):
    slot = scene.attach_ior(GLASS)
    opt = {"int_ior": torch.tensor([float(scene.ior_values()[scene.ior_slots.index(slot)])], device=scene.device, requires_grad=True)}

    def apply_transformation(scene_, opt_):
        scene_.set_ior(GLASS, max(_MIN_IOR, float(opt_["int_ior"].detach())))

    def backward(opt_, params):
        opt_["int_ior"].grad = params.alpha[slot:slot + 1].detach().clone()

    def output(opt_):
        return abs(float(opt_["int_ior"].detach()) - TARGET_IOR)

    return opt, apply_transformation, backward, output
