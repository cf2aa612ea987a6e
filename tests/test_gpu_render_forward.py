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


def _pixel_major(res, spp, n_cut, gen):
    """Film positions of a pixel-major wavefront without its last ``n_cut`` samples: pixel + uniform jitter."""
    n = res * res * spp - n_cut
    pix = torch.arange(res * res * spp)[:n] // spp
    return torch.stack([(pix % res).float(), (pix // res).float()], dim=1) + torch.rand((n, 2), generator=gen)


@pytest.mark.parametrize("rfilter,res,spp,n_cut,moving", [
    (1, 9, 64, 0, True), (1, 9, 128, 0, True), (1, 12, 16, 0, True), (1, 12, 8, 0, True), (1, 11, 5, 0, True), (1, 9, 64, 37, True),
    (1, 9, 64, 0, False), (1, 9, 128, 0, False), (1, 12, 16, 0, False), (1, 12, 8, 0, False), (1, 11, 5, 0, False), (1, 9, 64, 37, False),
    (0, 12, 16, 0, False)])
def test_film_splat_tangent_kernel_through_every_group_size(rfilter, res, spp, n_cut, moving):
    """epsm_film_splat_tangent against its torch form on pixel-major wavefronts: 64 / 128, 16 and 8 spp take the sums over
    groups of 64, 16 and 8 lanes, 5 spp the lane-by-lane form; a ragged tail puts lanes past the end (weight 0) into a
    group of 64.  Films of 9 to 12 pixels: most 5 x 5 windows are clipped at an edge.  The bound is the one of
    test_film_splat_tangent_kernel_equals_its_torch_form (the same kernel against the same reference): on these cases the
    worst error of the build before the film unit was 9.6e-7 of max|ref| (MEASUREMENTS.md 24), far below a third of it."""
    gen = torch.Generator().manual_seed(res * 1000 + spp + n_cut)
    pos = _pixel_major(res, spp, n_cut, gen)
    n = pos.shape[0]
    L, dL = torch.rand((n, 3), generator=gen), torch.randn((n, 3), generator=gen)
    dpos = torch.randn((n, 3), generator=gen) if moving else None
    ref = film_splat_tangent_torch(pos, L, dL, dpos, res, res, rfilter)
    got = torch.zeros((res, res, 4), device="cuda")
    film_splat_tangent(got, pos.cuda(), L.cuda(), dL.cuda(), None if dpos is None else dpos.cuda(), rfilter)
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    err = float((got.cpu() - ref).abs().max())
    print("film_splat_tangent", (rfilter, res, spp, n_cut, moving), "err / max|ref| = %.3g" % (err / scale))
    assert scale > 0
    assert err <= 1e-4 * scale


def _one_wave(name, gen):
    """64 film positions -- one wave -- whose 5 x 5 windows overlap only inside an aligned group of lanes in one pixel, so that
    every word of the film receives one atomic add at the most: -> (W, H, pos (n,2))."""
    jitter = torch.rand((64, 2), generator=gen)
    if name in ("64 lanes in one pixel", "40 lanes in one pixel"):
        W = H = 14
        px = torch.tensor([[1.0, 12.0]]).expand(64, 2)                      # (clipped at two edges)
    elif name == "four pixels":                                             # four groups of 16 lanes, 7 pixels apart
        W = H = 14
        g = torch.arange(64) // 16
        px = torch.stack([3.0 + 7 * (g % 2), 3.0 + 7 * (g // 2)], dim=1)
    elif name == "eight pixels":                                            # eight groups of 8 lanes, 6 pixels apart
        W, H = 23, 11
        g = torch.arange(64) // 8
        px = torch.stack([2.0 + 6 * (g % 4), 2.0 + 6 * (g // 4)], dim=1)
    else:                                                                   # 64 pixels 5 apart, row 0 and column 0 among them
        W = H = 40
        g = torch.arange(64)
        px = torch.stack([5.0 * (g % 8), 5.0 * (g // 8)], dim=1)
    pos = (px + jitter)[:40 if name.startswith("40") else 64].contiguous()
    return W, H, pos


ONE_WAVE = ["64 lanes in one pixel", "four pixels", "eight pixels", "64 pixels", "40 lanes in one pixel"]


@pytest.mark.parametrize("name", ONE_WAVE)
@pytest.mark.parametrize("which", ["splat", "tangent"])
def test_film_splats_one_group_size_at_a_time(which, name):
    """Each group size of the two splats -- 64, 16, 8 lanes and lane by lane -- alone in one wave, and lanes past the end in a
    group of 64.  No word of the film gets a second add, so the result does not depend on the order of the atomics: two calls
    into zeroed films agree bit for bit, and the result meets the host twin (test_gpu_tracer.py::test_film_splat_matches_host's
    bound) / the torch form (test_film_splat_tangent_kernel_equals_its_torch_form's)."""
    import ctypes as C
    from _scenes import host_tracer
    from epsm_mitsuba3_amd import _lib
    gen = torch.Generator().manual_seed(ONE_WAVE.index(name))
    W, H, pos = _one_wave(name, gen)
    n = pos.shape[0]
    L, dL, dpos = torch.rand((n, 3), generator=gen) * 3.0, torch.randn((n, 3), generator=gen), torch.randn((n, 3), generator=gen)
    pd, Ld, dLd, dposd = pos.cuda(), L.cuda(), dL.cuda(), dpos.cuda()
    out = []
    for _ in range(2):
        got = torch.zeros((H, W, 4), device="cuda")
        if which == "splat":
            assert _lib.lib().epsm_film_splat(C.c_int64(n), C.c_void_p(pd.data_ptr()), C.c_void_p(Ld.data_ptr()), W, H, 1,
                                              C.c_void_p(got.data_ptr()), C.c_void_p(_lib.stream(got.device))) == 0
        else:
            film_splat_tangent(got, pd, Ld, dLd, dposd, 1)
        torch.cuda.synchronize()
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])
    if which == "splat":
        want = torch.zeros((H, W, 4))
        assert host_tracer().epsm_film_splat(C.c_int64(n), C.c_void_p(pos.data_ptr()), C.c_void_p(L.data_ptr()), W, H, 1,
                                             C.c_void_p(want.data_ptr()), None) == 0
        assert float(want.abs().max()) > 0
        assert torch.allclose(out[0], want, rtol=2e-4, atol=2e-4 * float(want.abs().max()))
    else:
        ref = film_splat_tangent_torch(pos, L, dL, dpos, H, W, 1)
        scale = float(ref.abs().max())
        assert scale > 0
        assert float((out[0] - ref).abs().max()) <= 1e-4 * scale


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
