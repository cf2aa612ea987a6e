"""Free-form geometry from the per-vertex gradient rows (``prb_reparam``): every one of the 642 vertices of a diffuse icosphere
is free, and the target is the same sphere pushed into an ellipsoid with a low-frequency bump field.  The vertices are not
optimised directly: the leaf is ``u = (I + LAMBDA L) x`` (smooth.MeshLaplacian, the "large steps" re-parameterisation of Nicolet,
Jakob and Jacobson 2021), its gradient the solve ``(I + LAMBDA L)^-1 g_x`` of the Monte Carlo gradient, its optimiser AdamUniform:

    python -m epsm_mitsuba3_amd.optim prb_reparam relief

``LAMBDA = 0`` with ``optimizer = "Adam"`` is plain Adam on the vertices -- what the sparse, noisy gradient crumples within a few
iterations (tests/test_gpu_smooth.py runs both)."""
import numpy as np
import torch

from ..scene import Scene, look_at
from .clutter import icosphere

it = 20
spp = 16
resolution = 64
thres = 10000
max_depth = 3
match_res = 32
lr = 0.1                                          # MEASUREMENTS 33: where plain Adam on the vertices is reliably the worse
LAMBDA = 19.0
optimizer = "AdamUniform"                         # optim.run: smooth.AdamUniform in place of torch's Adam

_CENTRE = np.array([0.0, 0.0, 1.0])
_V, _F = icosphere(3)                             # 642 vertices, 1 280 triangles, radius 1 about the origin
_RADIUS = 0.8


def start_vertices() -> np.ndarray:
    return _V * _RADIUS + _CENTRE


def target_vertices() -> np.ndarray:
    """The sphere as an ellipsoid, each vertex pushed along its normal by a bump field of about one period over the ball."""
    x, y, z = _V[:, 0], _V[:, 1], _V[:, 2]
    bump = 0.10 * np.sin(2.5 * x + 0.5) * np.cos(2.0 * y - 0.3) + 0.06 * np.sin(3.0 * z)
    return _V * (np.array([1.25, 0.85, 1.0]) * _RADIUS) + _V * bump[:, None] + _CENTRE


def _quad(z, half):
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], float)
    return v, np.array([[0, 1, 2], [0, 2, 3]])


def _sensor(res, spp_):
    return {"type": "perspective", "fov": 40, "near_clip": 0.01, "far_clip": 100.0,
            "to_world": look_at([0.6, -4.2, 2.6], [0.0, 0.0, 0.85], [0, 0, 1]),
            "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "gaussian"}},
            "sampler": {"type": "independent", "sample_count": spp_}}


def load_scene(device="cuda", vertices=None):
    fv, ff = _quad(0.0, 5.0)
    lv, lf = _quad(6.0, 0.6)
    lv = lv + np.array([-1.5, -2.0, 0.0])
    d = {"type": "scene", "sensor0": _sensor(resolution, spp), "sensor1": _sensor(resolution, spp), "sensor2": _sensor(match_res, 8),
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.5]}}},
         "relief": {"type": "mesh", "vertices": start_vertices() if vertices is None else vertices, "faces": _F,
                    "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.55, 0.4]}}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf[:, ::-1], "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 120.0}}}}
    return Scene.from_dict(d, device=device)


def gt_scene(device="cuda"):
    return load_scene(device, target_vertices())


def optim_settings(scene):
    """``u`` is the one leaf.  ``apply_transformation``: x = (I + LAMBDA L)^-1 u, the mesh's vertices; ``backward``: the rows of
    ``ParamGrads.pos`` chained through that solve (optim.chain_vertex_grads).  ``output``: the mean distance of the vertices
    from the target's."""
    from ..optim import chain_vertex_grads
    lap = scene.mesh_laplacian("relief", LAMBDA)
    with torch.no_grad():
        u0 = lap.to_differential(scene.vertex_positions("relief").clone())
    opt = {"u": u0.clone().requires_grad_(True)}
    scene.attach("relief", positions=True)
    target = torch.tensor(target_vertices(), dtype=torch.float32)
    state = {"lap": lap}

    def apply_transformation(scene_, opt_):
        state["x"] = lap.from_differential(opt_["u"])
        scene_.set_vertex_positions("relief", state["x"].detach())

    def backward(opt_, params):
        g = torch.nan_to_num(params.mesh_pos("relief"), nan=0.0)
        opt_["u"].grad = None
        chain_vertex_grads(state["x"], g)

    def output(opt_):
        with torch.no_grad():
            x = lap.solve(opt_["u"].detach())
        return float((x.cpu() - target).norm(dim=1).mean())

    return opt, apply_transformation, backward, output


def vertices_of(scene, opt) -> torch.Tensor:
    """The vertex positions a run's leaf stands for (a fresh Laplacian of ``scene``'s mesh at the module's LAMBDA)."""
    with torch.no_grad():
        return scene.mesh_laplacian("relief", LAMBDA).solve(opt["u"].detach())


def inverted_triangles(start: torch.Tensor, end: torch.Tensor) -> int:
    """How many triangles' face normals flipped against their start (negative dot product)."""
    f = torch.as_tensor(_F, dtype=torch.int64)
    n = lambda v: torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    return int(((n(start.double().cpu()) * n(end.double().cpu())).sum(1) < 0).sum())
