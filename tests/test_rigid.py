"""Rigid-motion gradients on the host build of the tracer: the ``rigid`` / ``cam_rotation`` sections of ParamGrads, the refusals,
the transpose identity over rigid twists and the sensor's full pose, the sensor's rotation against finite differences of the
primal image, and a mesh's twist against a float64 chain rule on its own ``pos`` / ``nrm`` rows.  The HIP kernels
(csrc/epsm_trace_rigid.hip) are checked in tests/test_gpu_rigid.py; here ``rigid.reduce`` / ``rigid.expand`` run their torch forms."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _forward_host import on_host_forward
from _reparam_scenes import CONFIGS, build
from epsm_mitsuba3_amd import ParamGrads, rigid
from epsm_mitsuba3_amd import scene as S


# -- layout -------------------------------------------------------------------------------------------------------------------
def test_a_buffer_without_the_new_sections_is_laid_out_as_before():
    V, B, C, tex = 7, 2, 3, [(4, 5), (2, 3)]
    p = ParamGrads(V, B, device="cpu", n_colors=C, tex_shapes=tex)
    n0 = 6 * V + B + 3 + 3 * C
    assert p.flat.numel() == n0 + 3 * 4 * 5 + 3 * 2 * 3
    assert p.rigid is None and p.cam_rotation is None
    off = lambda t: (t.data_ptr() - p.flat.data_ptr()) // 4
    assert [off(t) for t in (p.pos, p.nrm, p.alpha, p.cam_origin, p.color, p.texture(0), p.texture(1))] == \
        [0, 3 * V, 6 * V, 6 * V + B, 6 * V + B + 3, n0, n0 + 60]
    assert p.scratch().flat.numel() == p.flat.numel()


def test_the_new_sections_follow_the_textures():
    V, B, C, tex = 7, 2, 3, [(4, 5), (2, 3)]
    old = ParamGrads(V, B, device="cpu", n_colors=C, tex_shapes=tex)
    p = ParamGrads(V, B, device="cpu", n_colors=C, tex_shapes=tex, n_rigid=2, cam_rotation=True)
    n1 = old.flat.numel()
    off = lambda q, t: (t.data_ptr() - q.flat.data_ptr()) // 4
    assert p.flat.numel() == n1 + 12 + 3 and tuple(p.rigid.shape) == (2, 6) and tuple(p.cam_rotation.shape) == (3,)
    assert off(p, p.rigid) == n1 and off(p, p.cam_rotation) == n1 + 12
    for a, b in ((p.pos, old.pos), (p.nrm, old.nrm), (p.alpha, old.alpha), (p.cam_origin, old.cam_origin), (p.color, old.color),
                 (p.texture(1), old.texture(1))):
        assert off(p, a) == off(old, b) and a.shape == b.shape
    s = p.scratch()
    assert s.flat.numel() == p.flat.numel() and tuple(s.rigid.shape) == (2, 6) and s.cam_rotation is not None
    only_rot = ParamGrads(V, B, device="cpu", cam_rotation=True)
    assert only_rot.rigid is None and off(only_rot, only_rot.cam_rotation) == 6 * V + B + 3


def test_scene_param_grads_carries_the_attached_sections():
    sc = build("translate_camera_lit", 0.0, 8, 2)
    assert sc.param_grads().rigid is None and sc.param_grads().cam_rotation is None
    sc.attach_sensor()
    assert sc.param_grads().cam_rotation is None                       # today's call: today's buffer
    sc.attach_sensor(rotation=True)
    slot = sc.attach_rigid("sphere", pivot=[0.5, 0.25, 0.125])
    assert slot == 0 and sc.attach_rigid("sphere") == 0 and sc.rigid_slots[0]["pivot"] == [0.5, 0.25, 0.125]   # attached again: it stays
    lo, hi = sc.mesh_slices["sphere"]
    sc.set_rigid_pivot(0, sc.positions[lo:hi].double().mean(0))
    p = sc.param_grads()
    assert tuple(p.rigid.shape) == (1, 6) and tuple(p.cam_rotation.shape) == (3,)
    m = sc.mesh("sphere")
    assert m.pos_attached and m.nrm_attached                            # a vertex-normal mesh: its normals turn with it
    assert sc.attach_rigid("floor") == 1 and sc.mesh("floor").pos_attached and not sc.mesh("floor").nrm_attached
    lo, hi = sc.mesh_slices["sphere"]
    assert np.allclose(sc.rigid_slots[0]["pivot"], sc.positions[lo:hi].double().mean(0).numpy())
    sc.set_vertex_positions("sphere", sc.vertex_positions("sphere") + 1.0)
    assert np.allclose(sc.rigid_slots[0]["pivot"], (sc.positions[lo:hi].double().mean(0) - 1.0).numpy(), atol=1e-6)   # it stays put
    sc.set_rigid_pivot(0, [1.0, 2.0, 3.0])
    assert sc.rigid_slots[0]["pivot"] == [1.0, 2.0, 3.0]
    sc.attach_sensor(False)
    assert sc.param_grads().cam_rotation is None


# -- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 2, "reparam_rays": 4})
    g = torch.ones((8, 8, 3))
    # an envmap would have to turn with the shapes
    sc = on_host_forward(build("diffuse_sphere_envmap", 0.0, 8, 2))
    sc.attach_sensor(rotation=True)
    sc.attach_color(sc.bsdf_names[sc.mesh("sphere").bsdf])
    p = sc.param_grads()
    with pytest.raises(NotImplementedError, match="envmap"):
        integ.render_backward(sc, p, g, sensor=0, seed=0, spp=2)
    assert float(p.flat.abs().max()) == 0.0                              # refused before the colour pass: nothing left behind
    with pytest.raises(NotImplementedError, match="envmap"):
        integ.render_forward(sc, sc.param_grads(), sensor=0, seed=0, spp=2)
    sc.attach_sensor()                                                   # its translation alone is served as before
    integ.render_backward(sc, sc.param_grads(), g, sensor=0, seed=0, spp=2)
    # a point emitter
    sc = on_host_forward(build("receiver_point_light", 0.0, 8, 2))
    sc.attach_sensor(rotation=True)
    with pytest.raises(NotImplementedError, match="point"):
        integ.render_backward(sc, sc.param_grads(), g, sensor=0, seed=0, spp=2)
    with pytest.raises(NotImplementedError, match="point"):
        integ.render_forward(sc, sc.param_grads(), sensor=0, seed=0, spp=2)
    # the 5-channel branch transports ray.o alone: no zeros left behind
    sc = on_host_forward(build("translate_camera_lit", 0.0, 8, 2))
    sc.attach_sensor(rotation=True)
    for kind in ("manifold", "manifold_caustic"):
        with pytest.raises(NotImplementedError, match="5-channel"):
            epsm.load_dict({"type": kind, "max_depth": 3}).render_backward(sc, sc.param_grads(), torch.ones((8, 8, 5)), seed=0)
    # an unknown mesh
    with pytest.raises(ValueError, match="no mesh named 'teapot'"):
        sc.attach_rigid("teapot")
    # a buffer from before the slots were attached
    stale = sc.param_grads()
    sc.attach_rigid("sphere")
    with pytest.raises(ValueError, match="attach_rigid"):
        integ.render_backward(sc, stale, g, sensor=0, seed=0, spp=2)
    # the kernels have no CPU form outside the host build
    r, c = torch.tensor([[0, 2]]), torch.zeros((1, 3))
    with pytest.raises(epsm._lib.EpsmError, match="GPU only"):
        rigid.reduce(torch.zeros((2, 3)), torch.zeros((2, 3)), torch.zeros((2, 3)), None, r, c, torch.zeros((1, 6)))


# -- the transpose ------------------------------------------------------------------------------------------------------------
def pose_scene(name, res, spp, device="cpu", rigid_meshes=(), rotation=True, own_rows=()):
    sc = build(name, 0.0, res, spp, device)
    if str(device) == "cpu":
        on_host_forward(sc)
    for m in own_rows:
        sc.attach(m, positions=True, normals=sc.mesh(m).has_normals)
    for m in rigid_meshes:
        sc.attach_rigid(m)
    if rotation is not None:
        sc.attach_sensor(rotation=rotation)
    return sc


def pose_tangent(sc, gen):
    """A random tangent over ``rigid``, ``cam_origin`` and ``cam_rotation`` together, and over the rows of the attached meshes."""
    t = sc.param_grads()
    for m in sc.meshes:
        lo, hi = t.mesh_slices[m.name]
        if m.pos_attached:
            t.pos[lo:hi] = 0.3 * torch.randn((hi - lo, 3), generator=gen).to(sc.device)
        if m.nrm_attached:
            t.nrm[lo:hi] = 0.3 * torch.randn((hi - lo, 3), generator=gen).to(sc.device)
    if t.rigid is not None:
        t.rigid[:] = torch.randn(tuple(t.rigid.shape), generator=gen).to(sc.device)
    if getattr(sc, "sensor_attached", False):
        t.cam_origin[:] = torch.randn(3, generator=gen).to(sc.device)
    if t.cam_rotation is not None:
        t.cam_rotation[:] = torch.randn(3, generator=gen).to(sc.device)
    return t


def pose_transpose_gap(integ, sc, seed, spp, gen):
    """tests/test_render_forward.py::transpose_gap with the tangent drawn over the new sections too."""
    s = sc.sensors[0]
    params = sc.param_grads()
    t = pose_tangent(sc, gen)
    g = torch.randn((s.height, s.width, 3), generator=gen).to(sc.device)
    fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp)
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    a = (g.double() * fwd.double()).sum()
    prod = params.flat.double() * t.flat.double()
    S_ = float((g.double() * fwd.double()).abs().sum() + prod.abs().sum())
    new = sum(float(x.abs().max()) for x in (params.rigid, params.cam_rotation) if x is not None)
    return abs(float(a - prod.sum())), S_, float(fwd.abs().max()), new


@pytest.mark.parametrize("name,rigid_meshes,rotation,own_rows", [
    ("translate_camera_lit", ("sphere", "floor"), True, ()),           # twists + the sensor's full pose
    ("translate_camera_lit", ("sphere",), True, ("sphere", "light")),  # + per-vertex rows on the rigid mesh and on another
    ("translate_camera", (), True, ()),                                # the sensor alone under the constant environment
    ("diffuse_sphere_area_light", ("sphere", "wall"), None, ()),       # twists without the sensor
    ("translate_camera_lit", ("sphere",), False, ()),                  # twists + the sensor's translation (today's call)
])
def test_forward_is_the_transpose_of_the_backward_pass(name, rigid_meshes, rotation, own_rows):
    """sum g . (J t) = sum (J^T g) . t at the relative bound tests/test_render_forward.py uses on the host (1e-4 of the sum of
    the absolute terms)."""
    cfg = CONFIGS[name]
    sc = pose_scene(name, 12, 4, rigid_meshes=rigid_meshes, rotation=rotation, own_rows=own_rows)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": 8, "reparam_kappa": cfg.get("kappa", 1e5)})
    gap, S_, big, new = pose_transpose_gap(integ, sc, 7, 4, torch.Generator().manual_seed(21))
    assert big > 0 and S_ > 0 and new > 0
    assert gap <= 1e-4 * S_, (gap, S_)


# -- the sensor's rotation against finite differences -----------------------------------------------------------------------------
def turn_sensor(sc, omega):
    """to_world <- Rot(omega) to_world about the sensor's own position, world axes."""
    for s in sc.sensors:
        w = np.asarray(s.to_world, float).copy()
        ang = float(np.linalg.norm(omega))
        if ang > 0:
            w[:3, :3] = S.rotate(np.asarray(omega) / ang, np.degrees(ang))[:3, :3] @ w[:3, :3]
        s.to_world = w


# The sensor-translation row of tests/test_reparam.py (test_sensor_translation_gradient_on_the_host): this config, spp, rays, FD
# sample multiplier and threshold.  Its FD step is fd_eps = 2e-3 scene units across the view.  A point at depth d moves by
# h f / d pixels under a translation h and by phi f pixels (at the image centre) under a rotation phi: the sensor looks at the origin
# from 4 units away and the scene lies at depths 3.3 .. 4.6 about it, so the angle step of the same mean pixel motion is h / 4.
ROW = dict(name="translate_camera_lit", spp=96, rays=16, fd_spp_mult=2, tol=0.6)
ANGLE_STEP = CONFIGS[ROW["name"]]["fd_eps"] / 4.0


def rotation_fd_check(device="cpu", spp=ROW["spp"], rays=ROW["rays"], seeds=1, fd_spp_mult=ROW["fd_spp_mult"], axis=None):
    """fd_check's recipe (tests/_reparam_scenes.py) for the sensor turning about its own y axis: ``cam_rotation . axis`` against
    central differences of the primal image under common random numbers."""
    name = ROW["name"]
    cfg = CONFIGS[name]
    res = cfg.get("res", 32)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": rays, "reparam_kappa": cfg.get("kappa", 1e5)})
    sc = build(name, 0.0, res, spp, device)
    sc.attach_sensor(rotation=True)
    ax = np.asarray(sc.sensors[0].to_world, float)[:3, 1] if axis is None else np.asarray(axis, float)
    g = torch.ones((res, res, 3), device=sc.device) * (0.5 + torch.arange(res, device=sc.device, dtype=torch.float32) / res)[None, :, None]
    got, fd = [], []
    for seed in range(seeds):
        params = sc.param_grads()
        integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
        got.append(float((params.cam_rotation.double().cpu() * torch.tensor(ax)).sum()))
        assert float(params.pos.abs().max()) == 0.0 and float(params.nrm.abs().max()) == 0.0      # no mesh was attached by the caller
        v = []
        for sgn in (1, -1):
            s2 = build(name, 0.0, res, spp * fd_spp_mult, device)
            turn_sensor(s2, sgn * ANGLE_STEP * ax)
            v.append(float((integ.render(s2, sensor=0, seed=100 + seed, spp=spp * fd_spp_mult) * g).sum()))
        fd.append((v[0] - v[1]) / (2 * ANGLE_STEP))
    return got, fd


def test_sensor_rotation_gradient_matches_finite_differences_on_the_host():
    """At the row's sample counts and its threshold (sign, and 60 % of the finite difference).  The rotation's FD noise at this spp
    stays inside the row's threshold (MEASUREMENTS.md 16.1: the FD-to-FD spread over five seeds), so the row's number holds."""
    got, fd = rotation_fd_check()
    g, f = float(np.mean(got)), float(np.mean(fd))
    print(f"cam_rotation . y: {g:+.3f}, FD {f:+.3f}")
    assert g * f > 0 and abs(g - f) / max(abs(f), 1e-3) < ROW["tol"], (g, f)


# -- a mesh's twist against the chain rule ------------------------------------------------------------------------------------
def _chain_rule(sc, p, mesh, pivot, normal_term=True):
    """[F, T] by torch autograd in float64: x(tw) = x + dt + dw x (x - c), n(tw) = n + dw x n, loss = sum g_pos . x + g_nrm . n."""
    lo, hi = sc.mesh_slices[mesh]
    x, n = sc.positions[lo:hi].double(), sc.normals[lo:hi].double()
    tw = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    w = tw[3:].expand(hi - lo, 3)
    loss = (p.pos[lo:hi].double() * (x + tw[:3] + torch.linalg.cross(w, x - torch.tensor(pivot, dtype=torch.float64), dim=1))).sum()
    if normal_term:
        loss = loss + (p.nrm[lo:hi].double() * (n + torch.linalg.cross(w, n, dim=1))).sum()
    loss.backward()
    return tw.grad


def test_a_mesh_twist_is_the_chain_rule_of_its_own_rows():
    """``rigid[slot]`` against float64 autograd on the ``pos`` / ``nrm`` rows of the same call, on a vertex-normal mesh whose
    normal gradients matter: without the n x g_nrm term the torque is off by far more than the tolerance.  The bound: the twist
    is a float64 sum rounded to float32 once (2^-24 relative) of float32 rows that are exact inputs to both sides, so a few
    float32 ulps of sum |terms| -- 4 * 2^-24 of it.  (The manifold integrators' twists: tests/test_gpu_rigid.py, their backward
    pass has no host build.)"""
    sc = pose_scene("diffuse_sphere_area_light", 12, 8, rigid_meshes=(), rotation=None)
    mesh, pivot = "sphere", [0.4, -0.2, 0.1]                                       # off the centroid: the force's arm counts
    slot = sc.attach_rigid(mesh, pivot=pivot)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    g = torch.randn((12, 12, 3), generator=torch.Generator().manual_seed(2))
    p = sc.param_grads()
    integ.render_backward(sc, p, g, sensor=0, seed=3, spp=8)
    lo, hi = sc.mesh_slices[mesh]
    assert float(p.pos[lo:hi].abs().max()) > 0 and float(p.nrm[lo:hi].abs().max()) > 0
    want = _chain_rule(sc, p, mesh, pivot)
    x = (sc.positions[lo:hi].double() - torch.tensor(pivot, dtype=torch.float64)).abs()
    gp, gn, n = p.pos[lo:hi].double().abs(), p.nrm[lo:hi].double().abs(), sc.normals[lo:hi].double().abs()
    acr = lambda a, b: torch.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
    terms = torch.cat([gp.sum(0), (acr(x, gp) + acr(n, gn)).sum(0)])
    assert torch.all((p.rigid[slot].double() - want).abs() <= 4 * 2.0 ** -24 * terms), (p.rigid[slot], want)
    without = _chain_rule(sc, p, mesh, pivot, normal_term=False)
    assert float((without[3:] - want[3:]).abs().max()) > 1e3 * float((4 * 2.0 ** -24 * terms[3:]).max()), (without, want)
    integ.render_backward(sc, p, g, sensor=0, seed=3, spp=8)
    assert torch.allclose(p.rigid[slot].double(), 2 * want, rtol=1e-5, atol=1e-6 * float(want.abs().max()))       # it accumulates
