"""render_forward (common.py:118-197) on the host build of the tracer: the exact transpose of render_backward (the dot-product
test under the same random numbers), against finite differences of the primal image, the film's forward mode against the
adjoint it transposes, the refusals it shares with the backward pass, and two ranks."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _forward_host import on_host_forward
from _reparam_scenes import CONFIGS, build, fd_check
from _scenes import floor_and_light, furnace
from epsm_mitsuba3_amd.integrators import film_adjoint_reparam_torch, film_splat_tangent_torch

# (config, normals attached too)
GEOMETRY = [("diffuse_sphere_area_light", True), ("occluder_area_light", False), ("sphere_on_glossy_floor", False),
            ("textured_plane_constant", False), ("diffuse_sphere_envmap", False), ("translate_camera_lit", False)]


def _scene(name, res, spp, device="cpu", normals=False):
    cfg = CONFIGS[name]
    sc = build(name, 0.0, res, spp, device)
    if str(device) == "cpu":
        on_host_forward(sc)
    for m in cfg["moving"]:
        sc.attach(m, positions=True, normals=normals)
    if cfg.get("camera"):
        sc.attach_sensor()
    return sc


def _random_tangent(sc, params, gen, colour=False):
    """A random tangent on the attached rows of ``params`` (and the sensor / colour slots when attached)."""
    t = sc.param_grads()
    dev = sc.device
    for m in sc.meshes:
        lo, hi = params.mesh_slices[m.name]
        if getattr(m, "pos_attached", False):
            t.pos[lo:hi] = torch.randn((hi - lo, 3), generator=gen).to(dev)
        if getattr(m, "nrm_attached", False):
            t.nrm[lo:hi] = torch.randn((hi - lo, 3), generator=gen).to(dev)
    if getattr(sc, "sensor_attached", False):
        t.cam_origin[:] = torch.randn(3, generator=gen).to(dev)
    if colour and t.C:
        t.color[:] = torch.randn((t.C, 3), generator=gen).to(dev)
    return t


def transpose_gap(integ, sc, seed, spp, gen):
    """(|a - b|, S): a = sum g * J t, b = sum J^T g * t, S = sum |g * J t| + sum |J^T g * t|."""
    s = sc.sensors[0]
    params = sc.param_grads()
    t = _random_tangent(sc, params, gen, colour=True)
    g = torch.randn((s.height, s.width, 3), generator=gen).to(sc.device)
    fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp)
    assert tuple(fwd.shape) == (s.height, s.width, 3)
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    a = (g.double() * fwd.double()).sum()
    prod = params.flat.double() * t.flat.double()
    b = prod.sum()
    S = float((g.double() * fwd.double()).abs().sum() + prod.abs().sum())
    return abs(float(a - b)), S, float(fwd.abs().max())


@pytest.mark.parametrize("name,normals", GEOMETRY)
@pytest.mark.parametrize("rays,antithetic", [(5, False), (16, False), (16, True)])
def test_geometry_forward_is_the_transpose_of_the_backward_pass(name, normals, rays, antithetic):
    cfg = CONFIGS[name]
    sc = _scene(name, 12, 4, normals=normals)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": rays,
                            "reparam_kappa": cfg.get("kappa", 1e5), "reparam_antithetic": antithetic})
    gap, S, big = transpose_gap(integ, sc, 7, 4, torch.Generator().manual_seed(rays + 100 * antithetic))
    assert big > 0 and S > 0
    assert gap <= 1e-4 * S, (gap, S)


def _colour_scene(kind):
    sc = floor_and_light(res=10, device="cpu")
    on_host_forward(sc)
    sc.sensors[0].spp = 4
    sc.attach_color(sc.bsdf_names[sc.meshes[0].bsdf])
    sc.attach_radiance("light")
    return sc


@pytest.mark.parametrize("kind", ["prb", "prb_reparam", "manifold"])
def test_colour_forward_is_the_transpose_of_the_backward_pass(kind):
    sc = _colour_scene(kind)
    integ = epsm.load_dict({"type": kind, "max_depth": 3})
    gap, S, big = transpose_gap(integ, sc, 3, 4, torch.Generator().manual_seed(5))
    assert big > 0 and gap <= 1e-4 * S, (gap, S)


def test_colour_and_geometry_together_are_the_transpose_of_the_backward_pass():
    sc = _scene("diffuse_sphere_area_light", 12, 4)
    sc.attach_color(sc.bsdf_names[sc.mesh("sphere").bsdf])
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    gap, S, big = transpose_gap(integ, sc, 1, 4, torch.Generator().manual_seed(9))
    assert big > 0 and gap <= 1e-4 * S, (gap, S)


def test_colour_forward_matches_finite_differences():
    """test02_rendering_forward's metric (test_ad_integrators.py:768-830) for a diffuse reflectance, with max_depth <= rr_depth:
    no Russian roulette, so the samples do not depend on the parameter and the central difference under the same seed is exact
    up to rounding."""
    furn = dict(radiance=1.0, reflectance=(0.5, 0.3, 0.8), res=8, spp=16)
    sc = on_host_forward(furnace(**furn))
    slot = sc.attach_color(sc.bsdf_names[sc.meshes[0].bsdf])
    integ = epsm.load_dict({"type": "prb", "max_depth": 4, "rr_depth": 5})
    t = sc.param_grads()
    t.color[slot] = torch.tensor([1.0, -0.5, 0.7])
    fwd = integ.render_forward(sc, t, sensor=0, seed=4, spp=16)
    h = 1e-3
    imgs = []
    for sgn in (1, -1):
        refl = [r + sgn * h * float(d) for r, d in zip(furn["reflectance"], t.color[slot])]
        s2 = on_host_forward(furnace(**{**furn, "reflectance": tuple(refl)}))
        imgs.append(integ.render(s2, sensor=0, seed=4, spp=16).double())
    fd = (imgs[0] - imgs[1]) / (2 * h)
    err = ((fwd.double() - fd).abs() / fd.abs().clamp_min(0.2)).mean()
    assert float(fd.abs().max()) > 0.1
    assert float(err) <= 1e-3, float(err)


@pytest.mark.parametrize("name,rays,spp,kw,tol", [
    ("textured_plane_constant", 32, 128, dict(fd_spp_mult=4), 0.1),        # test_smooth_and_silhouette_configs_match_finite_differences
    ("occluder_area_light", 64, 256, dict(fd_eps=5e-3, fd_spp_mult=4), 0.35),   # test_shadow_and_indirect_configs_have_the_sign_...
    ("translate_camera_lit", 16, 96, dict(fd_spp_mult=2), 0.6),             # test_sensor_translation_gradient_on_the_host
])
def test_geometry_forward_matches_finite_differences(name, rays, spp, kw, tol):
    """Sum g * render_forward against fd_check's central differences, at the sample counts and thresholds test_reparam.py gives
    the backward pass on the same configs."""
    cfg = CONFIGS[name]
    res = cfg.get("res", 32)
    _, fd, _ = fd_check(name, spp=spp, rays=rays, seeds=1, **kw)
    sc = _scene(name, res, spp)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": rays,
                            "reparam_kappa": cfg.get("kappa", 1e5)})
    t = sc.param_grads()
    if cfg.get("camera"):          # d / d theta of to_world @ translate(theta, 0, 0): the sensor's x axis in the world
        t.cam_origin[:] = torch.tensor(np.asarray(sc.sensors[0].to_world, float)[:3, 0], dtype=torch.float32)
    u = torch.tensor(cfg.get("dir", (1.0, 0.0, 0.0)))
    for m in cfg["moving"]:
        t.mesh_pos(m)[:] = u
    g = torch.ones((res, res, 3)) * (0.5 + torch.arange(res, dtype=torch.float32) / res)[None, :, None]
    got = float((integ.render_forward(sc, t, sensor=0, seed=0, spp=spp) * g).sum())
    assert got * fd[0] > 0 and abs(got - fd[0]) <= tol * abs(fd[0]), (got, fd[0])


def test_film_forward_is_the_transpose_of_the_film_adjoint():
    gen = torch.Generator().manual_seed(2)
    H, W, n = 9, 11, 400
    pos = torch.rand((n, 2), generator=gen) * torch.tensor([W + 2.0, H + 2.0]) - 1.0
    L = torch.rand((n, 3), generator=gen)
    accum = torch.rand((H, W, 4), generator=gen) + 0.1
    g = torch.randn((H, W, 3), generator=gen)
    dL, dpos = torch.randn((n, 3), generator=gen), torch.randn((n, 3), generator=gen)
    adj_L, adj_f = film_adjoint_reparam_torch(pos, L, g, accum)
    d_accum = film_splat_tangent_torch(pos, L, dL, dpos, H, W, 1)
    img_t = epsm.integrators.develop_tangent(accum, d_accum)
    a = float((g.double() * img_t.double()).sum())
    b = float((adj_L.double() * dL.double()).sum() + (adj_f.double() * dpos.double()).sum())
    S = float((g * img_t).abs().sum() + (adj_L * dL).abs().sum() + (adj_f * dpos).abs().sum())
    assert abs(a - b) <= 1e-5 * S, (a, b)


def test_refusals_are_those_of_the_backward_pass():
    # a box filter with a geometry tangent
    sc = on_host_forward(floor_and_light(res=8, device="cpu"))
    sc.attach("floor")
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 2, "reparam_rays": 4})
    with pytest.raises(Exception, match="box reconstruction filter"):
        integ.render_forward(sc, sc.param_grads(), spp=2)
    # prb with only geometry attached
    with pytest.raises(NotImplementedError, match="geometry is attached but no colour"):
        epsm.load_dict({"type": "prb", "max_depth": 2}).render_forward(sc, sc.param_grads(), spp=2)
    # a point emitter with a sensor tangent
    sc = build("receiver_point_light", 0.0, 8, 2, "cpu")
    on_host_forward(sc)
    sc.attach_sensor()
    with pytest.raises(NotImplementedError, match="point"):
        integ.render_forward(sc, sc.param_grads(), spp=2)


def test_host_twins_refuse_what_the_device_refuses():
    """Both reparameterised host entry points fill their ``cfg`` through the device library's own rule
    (csrc/epsm_trace_reparam.h, reparam_cfg_fill), as the tracer's twins do with trace_args_fill
    (tests/test_tracer_wavefront_host.py::test_host_twin_refuses_what_the_device_refuses): a ray count outside 1..64, a kappa
    or exponent that is not positive, a negative reparam_max_depth and an unknown flag bit are refused and nothing is written;
    N == 0 with a scene and a sensor is fine whatever else is passed; the same call without the fault runs."""
    import ctypes as C
    res, spp, depth = 8, 2, 3
    sc = _scene("diffuse_sphere_area_light", res, spp)
    lib, n = sc._backend, sc.sensors[0].wavefront_size(spp)
    radiance = sc._trace(0, 1, spp, depth, 0, 0, n).radiance.contiguous()
    gen = torch.Generator().manual_seed(1)
    adj, adj_film = torch.randn((n, 3), generator=gen), torch.randn((n, 3), generator=gen)
    tan_pos, tan_nrm = torch.randn((sc.V, 3), generator=gen), torch.randn((sc.V, 3), generator=gen)
    grad_pos, grad_nrm = torch.zeros((sc.V, 3)), torch.zeros((sc.V, 3))
    d_radiance, d_film = torch.full((n, 3), float("nan")), torch.full((n, 3), float("nan"))
    cs = sc.sensors[0].c_struct()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    good = dict(rmd=depth, rays=4, kappa=1e5, exponent=3.0, flags=0)

    def call(forward, N=n, spp_=spp, **kw):
        c = dict(good, **kw)
        head = [C.byref(sc.c_scene), C.byref(cs), C.c_uint32(1), spp_, depth, int(sc.rr_depth), C.c_int64(0), C.c_int64(N)]
        cfg = [c["rmd"], c["rays"], C.c_float(c["kappa"]), C.c_float(c["exponent"]), C.c_uint32(c["flags"])]
        if N == 0:                                                                       # garbage beside scene and sensor
            return getattr(lib, "epsm_trace_paths_reparam_forward" if forward else "epsm_trace_paths_reparam")(
                *head, None, None, None, *cfg, None, None, None, C.c_size_t(0), None)
        if forward:
            return lib.epsm_trace_paths_reparam_forward(*head, ptr(radiance), ptr(tan_pos), ptr(tan_nrm), *cfg, ptr(d_radiance), ptr(d_film),
                                                        None, C.c_size_t(0), None)
        return lib.epsm_trace_paths_reparam(*head, ptr(radiance), ptr(adj), ptr(adj_film), *cfg, ptr(grad_pos), ptr(grad_nrm), None,
                                            C.c_size_t(0), None)

    for forward in (False, True):
        for bad in (dict(rays=0), dict(rays=65), dict(kappa=0.0), dict(exponent=0.0), dict(rmd=-1), dict(flags=2)):
            assert call(forward, **bad) != 0, (forward, bad)
        assert call(forward, N=0, spp_=-3, rays=0, kappa=-1.0, exponent=0.0, rmd=-7, flags=0xF0) == 0
        if forward:                                                                      # nothing ran
            assert bool(torch.isnan(d_radiance).all()) and bool(torch.isnan(d_film).all())
        else:
            assert float(grad_pos.abs().max()) == 0
        assert call(forward) == 0
    assert float(grad_pos.abs().max()) > 0 and bool(torch.isfinite(d_radiance).all()) and float(d_radiance.abs().max()) > 0


def test_unattached_slots_do_not_change_the_image():
    sc = _scene("diffuse_sphere_area_light", 10, 4)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    gen = torch.Generator().manual_seed(3)
    t = _random_tangent(sc, sc.param_grads(), gen)
    ref = integ.render_forward(sc, t, seed=2, spp=4)
    assert float(ref.abs().max()) > 0
    noisy = sc.param_grads()
    noisy.flat.copy_(t.flat)
    for m in sc.meshes:
        lo, hi = noisy.mesh_slices[m.name]
        if not m.pos_attached:
            noisy.pos[lo:hi] = torch.randn((hi - lo, 3), generator=gen)
        noisy.nrm[lo:hi] = torch.randn((hi - lo, 3), generator=gen)      # no normals attached anywhere
    noisy.cam_origin[:] = torch.randn(3, generator=gen)                   # the sensor is not attached
    assert torch.equal(integ.render_forward(sc, noisy, seed=2, spp=4), ref)


# -- two ranks (tests/test_dist_gloo.py::_reparam_single) ---------------------------------------------------------------
def _forward_single(tile_paths):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import epsm_mitsuba3_amd as epsm_
    from _forward_host import on_host_forward as on_host_fwd
    from _reparam_scenes import build as build_
    sc = build_("diffuse_sphere_area_light", 0.0, 12, 8, "cpu")
    on_host_fwd(sc)
    sc.tile_paths = tile_paths
    sc.attach("sphere", positions=True, normals=True)
    sc.attach_color(sc.bsdf_names[sc.mesh("sphere").bsdf])
    integ = epsm_.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    t = sc.param_grads()
    gen = torch.Generator().manual_seed(12)
    t.flat.copy_(torch.randn(t.flat.shape, generator=gen))
    return integ.render_forward(sc, t, sensor=0, seed=3, spp=8)


def _forward_worker(rank, world, port, q):
    import torch.distributed as dist
    from epsm_mitsuba3_amd import dist as edist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    edist.init_from_env("gloo")
    img = _forward_single(512)
    q.put((rank, img.numpy().tobytes(), tuple(img.shape)))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_forward_matches_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_forward_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    single = _forward_single(512)
    m = float(single.abs().max())
    assert m > 0
    for rank, buf, shape in got:
        img = torch.from_numpy(np.frombuffer(buf, dtype=np.float32).reshape(shape).copy())
        assert torch.allclose(img, single, rtol=1e-4, atol=1e-5 * m), rank
