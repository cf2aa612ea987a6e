"""render_forward on the GPU (epsm_trace_paths_reparam_forward, epsm_film_splat_tangent): the transpose identity against the
device backward pass, the device forward pass against the host build of the same per-path code, the film kernel against its
torch form, and finite differences at the sample counts tests/test_gpu_reparam.py gives the backward pass."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _forward_host import on_host_forward
from _reparam_scenes import CONFIGS, build, fd_check
from _scenes import floor_and_light
from epsm_mitsuba3_amd.integrators import film_splat_tangent, film_splat_tangent_torch
from test_render_forward import GEOMETRY, transpose_gap

pytestmark = pytest.mark.gpu


def _scene(name, res, spp, device, normals=False):
    cfg = CONFIGS[name]
    sc = build(name, 0.0, res, spp, device)
    if device == "cpu":
        on_host_forward(sc)
    for m in cfg["moving"]:
        sc.attach(m, positions=True, normals=normals)
    if cfg.get("camera"):
        sc.attach_sensor()
    return sc


@pytest.mark.parametrize("name,normals", GEOMETRY)
@pytest.mark.parametrize("rays,antithetic", [(5, False), (16, False), (16, True)])
def test_device_forward_is_the_transpose_of_the_device_backward_pass(name, normals, rays, antithetic):
    cfg = CONFIGS[name]
    sc = _scene(name, 16, 8, "cuda", normals=normals)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": rays,
                            "reparam_kappa": cfg.get("kappa", 1e5), "reparam_antithetic": antithetic})
    gap, S, big = transpose_gap(integ, sc, 7, 8, torch.Generator().manual_seed(rays + 100 * antithetic))
    assert big > 0 and S > 0
    assert gap <= 2e-3 * S, (gap, S)


@pytest.mark.parametrize("kind", ["prb", "prb_reparam", "manifold"])
def test_device_colour_forward_is_the_transpose_of_the_backward_pass(kind):
    sc = floor_and_light(res=16, device="cuda")
    sc.attach_color(sc.bsdf_names[sc.meshes[0].bsdf])
    sc.attach_radiance("light")
    integ = epsm.load_dict({"type": kind, "max_depth": 3})
    gap, S, big = transpose_gap(integ, sc, 3, 8, torch.Generator().manual_seed(5))
    assert big > 0 and gap <= 2e-3 * S, (gap, S)


@pytest.mark.parametrize("name,rays,antithetic", [
    ("diffuse_sphere_area_light", 16, False), ("sphere_on_glossy_floor", 16, False), ("occluder_area_light", 16, False),
    ("diffuse_sphere_area_light", 5, False), ("sphere_on_glossy_floor", 64, False), ("diffuse_sphere_envmap", 24, False),
    ("diffuse_sphere_area_light", 16, True)])
def test_device_forward_equals_the_host_build(name, rays, antithetic):
    """Per path d_radiance / d_film, and the image, against the host build's inline warps under the bound of
    test_gpu_reparam.py::test_device_pass_equals_the_host_build (fma contraction may flip a grazing auxiliary hit)."""
    res, spp = 16, 32
    cfg = CONFIGS[name]
    kw = dict(reparam_max_depth=cfg["max_depth"], reparam_rays=rays, kappa=cfg.get("kappa", 1e5), exponent=3.0, antithetic=antithetic)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": rays,
                            "reparam_kappa": cfg.get("kappa", 1e5), "reparam_antithetic": antithetic})
    out = []
    radiance = None
    for dev in ("cpu", "cuda"):
        sc = _scene(name, res, spp, dev, normals=True)
        t = sc.param_grads()
        t.flat.copy_(torch.randn(t.flat.shape, generator=torch.Generator().manual_seed(4)).to(sc.device))
        n = sc.sensors[0].wavefront_size(spp)
        if radiance is None:
            radiance = sc._trace(0, 5, spp, cfg["max_depth"], 0, 0, n).radiance.contiguous()
        d_rad, d_film = sc.trace_reparam_forward(0, 5, spp, cfg["max_depth"], 0, n, radiance.to(sc.device), t.pos.contiguous(),
                                                 t.nrm.contiguous(), **kw)
        img = integ.render_forward(sc, t, sensor=0, seed=5, spp=spp)
        out.append((d_rad.cpu(), d_film.cpu(), img.cpu()))
    for k, what in enumerate(("d_radiance", "d_film", "image")):
        a, b = out[0][k], out[1][k]
        scale = float(a.abs().max())
        if what == "d_film" and name == "occluder_area_light":       # the camera does not see the occluder: nothing moves on the film
            assert scale == 0 and float(b.abs().max()) == 0
            continue
        assert scale > 0, what
        bad = ((a - b).abs() > 2e-2 * scale).float().mean()
        assert float(bad) < 0.02, (name, what, float(bad), scale)
        assert abs(float(a.sum() - b.sum())) < 2e-2 * float(a.abs().sum()), (name, what)


@pytest.mark.parametrize("rfilter,moving", [(1, True), (1, False), (0, False)])
def test_film_splat_tangent_kernel_equals_its_torch_form(rfilter, moving):
    gen = torch.Generator().manual_seed(8)
    H, W, n = 37, 53, 20000
    pos = torch.rand((n, 2), generator=gen) * torch.tensor([W + 4.0, H + 4.0]) - 2.0
    L, dL = torch.rand((n, 3), generator=gen), torch.randn((n, 3), generator=gen)
    dpos = torch.randn((n, 3), generator=gen) if moving else None
    ref = film_splat_tangent_torch(pos, L, dL, dpos, H, W, rfilter)
    got = torch.zeros((H, W, 4), device="cuda")
    film_splat_tangent(got, pos.cuda(), L.cuda(), dL.cuda(), None if dpos is None else dpos.cuda(), rfilter)
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    assert scale > 0
    assert float((got.cpu() - ref).abs().max()) <= 1e-4 * scale


@pytest.mark.parametrize("name,spp,tol", [
    ("diffuse_sphere_area_light", 4096, 0.15),
    ("textured_plane_constant", 800, 0.1),
    ("translate_camera_lit", 2048, 0.2),
])
def test_forward_matches_finite_differences(name, spp, tol):
    """fd_check's central differences (two seeds) against sum g * render_forward under the same seeds, at the sample counts and
    thresholds of test_gpu_reparam.py::test_backward_gradient_matches_finite_differences."""
    cfg = CONFIGS[name]
    res = cfg.get("res", 32)
    fd_eps = 5e-3 if name == "diffuse_sphere_area_light" else 0.0        # as test_backward_gradient_matches_finite_differences picks it
    _, fd, _ = fd_check(name, device="cuda", spp=spp, rays=64, seeds=2, fd_eps=fd_eps, fd_spp_mult=2)
    sc = _scene(name, res, spp, "cuda")
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": 64,
                            "reparam_kappa": cfg.get("kappa", 1e5)})
    t = sc.param_grads()
    if cfg.get("camera"):
        t.cam_origin[:] = torch.tensor(np.asarray(sc.sensors[0].to_world, float)[:3, 0], dtype=torch.float32)
    u = torch.tensor(cfg.get("dir", (1.0, 0.0, 0.0)), device="cuda")
    for m in cfg["moving"]:
        t.mesh_pos(m)[:] = u
    g = torch.ones((res, res, 3), device="cuda") * (0.5 + torch.arange(res, device="cuda", dtype=torch.float32) / res)[None, :, None]
    got = [float((integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp) * g).sum()) for seed in range(2)]
    gm, fm = float(np.mean(got)), float(np.mean(fd))
    print(f"{name}: forward {gm:+.3f} per seed {[round(x, 2) for x in got]}, FD {fm:+.3f}")
    assert abs(gm - fm) / max(abs(fm), 1e-3) < tol, (name, gm, fm)
