"""Lighting experiment for the colour adjoint: the composition of ``exp/glossyball.py`` restated synthetically -- a
``roughconductor`` ball on a diffuse floor under a smooth analytic envmap.  The target is the same scene with the map turned by a
known rotation, about an axis that is neither the map's polar axis nor perpendicular to it, and with another ``scale``; the
optimisation starts at the unturned map.  Adam on ``omega`` (the rotation of ``to_world <- Rot(omega) to_world``: every step is
applied through the exponential map and the result re-orthonormalised, so the leaf is the step from the current pose and
returns to zero) and on ``ln scale``, with the L2 image loss of the reference's non-EPSM branch and de-correlated seeds.  The
orientation and the brightness of the environment are fitted from the image alone -- the envmap pose adjoint,
Scene.attach_envmap_pose + epsm_trace_paths_envpose_backward:

    python -m epsm_mitsuba3_amd.optim prb lighting

The reported error is the angle (radians) between the current and the target rotation; ``pose_errors`` keeps
(angle, |ln(scale / target)|) of every iteration of the last run and ``pose_grads`` the four gradients.
"""
import numpy as np
import torch

from .. import scene as S
from .clutter import icosphere

it = 40
spp = 16
resolution = 32
thres = 10000
max_depth = 3
match_res = 32
lr = 0.03

MAP_W, MAP_H = 32, 16
POLAR = np.array([0.0, 0.0, 1.0])                  # the map's polar axis in the world: z up
TURN_AXIS = np.array([0.5, 0.3, 0.8])              # 36 degrees off the polar axis
TURN_ANGLE = 0.6
SCALE_START, SCALE_TARGET = 1.0, 1.6

pose_grads = []
pose_errors = []


def rot(w) -> np.ndarray:
    """Rot(w): the right-handed rotation about w by |w| (the exponential map), float64."""
    w = np.asarray(w, np.float64)
    a = float(np.linalg.norm(w))
    if a == 0.0:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def orthonormalised(R: np.ndarray) -> np.ndarray:
    """The rotation nearest to R (polar decomposition)."""
    u, _, vt = np.linalg.svd(R)
    return u @ np.diag([1.0, 1.0, np.linalg.det(u @ vt)]) @ vt


def rotation_angle(A: np.ndarray, B: np.ndarray) -> float:
    return float(np.arccos(np.clip((np.trace(A @ B.T) - 1.0) / 2.0, -1.0, 1.0)))


R_START = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])      # the map's y (its pole) -> the world's z
R_TARGET = rot(TURN_AXIS / np.linalg.norm(TURN_AXIS) * TURN_ANGLE) @ R_START


def sky_bitmap() -> np.ndarray:
    """(MAP_H, MAP_W, 3): a dim blue sky, a broad warm lobe 50 degrees above the horizon and a cooler one opposite -- smooth in
    the direction, so the pole rows are constant and the bilinear map has no sharp feature to snap to."""
    phi = 2 * np.pi * (np.arange(MAP_W) + 0.5) / MAP_W
    theta = np.pi * np.arange(MAP_H) / (MAP_H - 1)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    l = np.stack([np.sin(phi)[None] * st, ct * np.ones((1, MAP_W)), -np.cos(phi)[None] * st], -1)      # the emitter's frame
    lobe = lambda d, sharp: np.exp(sharp * (l @ (np.array(d) / np.linalg.norm(d)) - 1.0))[..., None]
    sky = np.array([0.25, 0.35, 0.5]) * (0.6 + 0.4 * l[..., 1:2])
    return (sky + np.array([6.0, 4.5, 3.0]) * lobe([0.5, 0.75, -0.4], 6.0)
            + np.array([1.0, 1.5, 2.5]) * lobe([-0.6, 0.3, 0.7], 3.0)).astype(np.float32)


def load_scene(device="cuda", rotation=R_START, scale=SCALE_START, **scene_kw):
    bv, bf = icosphere(3)
    half = 3.0
    fv = np.array([[-half, -half, 0.0], [half, -half, 0.0], [half, half, 0.0], [-half, half, 0.0]])
    tw = np.eye(4)
    tw[:3, :3] = rotation
    d = {"type": "scene",
         "cam": {"type": "perspective", "fov": 40, "near_clip": 0.01, "far_clip": 100.0,
                 "to_world": S.look_at([0.0, -4.0, 2.2], [0.0, 0.0, 0.7], (0, 0, 1)),
                 "film": {"type": "hdrfilm", "width": resolution, "height": resolution, "rfilter": {"type": "gaussian"}},
                 "sampler": {"type": "independent", "sample_count": spp}},
         "sky": {"type": "envmap", "bitmap": sky_bitmap(), "scale": float(scale), "to_world": tw},
         "floor": {"type": "mesh", "vertices": fv, "faces": np.array([[0, 1, 2], [0, 2, 3]]), "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.55, 0.5, 0.45]}}},
         "ball": {"type": "mesh", "vertices": bv * 0.8 + np.array([0.0, 0.0, 0.8]), "faces": bf, "face_normals": False,
                  "bsdf": {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": 0.25}}}
    sc = S.Scene.from_dict(d, device=device, **scene_kw)
    sc.tracer = "mega"
    return sc


def gt_scene(device="cuda"):
    return load_scene(device, R_TARGET, SCALE_TARGET)


def optim_settings(scene):
    scene.attach_envmap_pose()
    opt = {"omega": torch.zeros(3, device=scene.device, requires_grad=True),
           "ln_scale": torch.tensor([float(np.log(SCALE_START))], device=scene.device, requires_grad=True)}
    del pose_grads[:], pose_errors[:]

    def apply_transformation(scene_, opt_):
        R, _ = scene_.envmap_pose()
        step = opt_["omega"].detach().cpu().double().numpy()
        with torch.no_grad():
            opt_["omega"].zero_()                                   # the leaf is the step from the current pose
        scene_.set_envmap_pose(rotation=orthonormalised(rot(step) @ R), scale=float(torch.exp(opt_["ln_scale"].detach())[0]))

    def backward(opt_, params):
        pose_grads.append(params.env_pose.detach().cpu().clone())
        opt_["omega"].grad = params.env_rotation.detach().clone().to(opt_["omega"].device)
        opt_["ln_scale"].grad = (params.env_scale.detach() * scene.envmap_pose()[1]).to(opt_["ln_scale"].device)

    def output(opt_):
        R, _ = scene.envmap_pose()
        R = orthonormalised(rot(opt_["omega"].detach().cpu().double().numpy()) @ R)      # (the step Adam just took included)
        err = (rotation_angle(R, R_TARGET), abs(float(opt_["ln_scale"].detach()[0]) - float(np.log(SCALE_TARGET))))
        pose_errors.append(err)
        return err[0]

    return opt, apply_transformation, backward, output
