"""`prb_reparam` on the GPU (csrc/epsm_trace_reparam.hip through the C ABI): the device pass against the host build of the
same per-path code, and the reference's recipe -- backward gradient against finite differences of the primal image
(src/integrators/tests/test_ad_integrators.py:833-871) -- at sample counts of the order of the reference's (its configs:
1024 .. 12 000 spp, 64 auxiliary rays) with ITS thresholds for the configs restated in tests/_reparam_scenes.py."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _reparam_scenes import CONFIGS, build, fd_check, fd_check_normals

pytestmark = pytest.mark.gpu


def rel(got, fd):
    g, f = float(np.mean(got)), float(np.mean(fd))
    return abs(g - f) / max(abs(f), 1e-3), g, f


@pytest.mark.parametrize("name,rays,antithetic", [
    ("diffuse_sphere_area_light", 16, False), ("sphere_on_glossy_floor", 16, False), ("occluder_area_light", 16, False),
    ("diffuse_sphere_area_light", 24, False), ("diffuse_sphere_area_light", 5, False), ("sphere_on_glossy_floor", 64, False),
    ("diffuse_sphere_area_light", 16, True), ("occluder_area_light", 5, True)])
def test_device_pass_equals_the_host_build(name, rays, antithetic):
    """Same seed, same auxiliary rays (every ray has its own stream): the device's two stages -- requests, then one lane per
    auxiliary ray in groups of 16 / 32 / 64, partly filled for 5 and 24 rays -- against the host build's inline warps; per-vertex
    gradients agree up to what fma contraction flips (a hit that becomes a miss moves one auxiliary ray's share).  With
    ``reparam_antithetic`` the lanes 2m and 2m + 1 of a group draw the same sample (an odd count leaves the last one alone)."""
    res, spp = 16, 32
    cfg = CONFIGS[name]
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": rays, "reparam_kappa": cfg.get("kappa", 1e5),
                            "reparam_antithetic": antithetic})
    g = torch.ones((res, res, 3)) * (0.5 + torch.arange(res, dtype=torch.float32) / res)[None, :, None]
    out = []
    for dev in ("cpu", "cuda"):
        sc = build(name, 0.0, res, spp, dev)
        for m in cfg["moving"]:
            sc.attach(m, positions=True, normals=True)
        p = sc.param_grads()
        integ.render_backward(sc, p, g.to(sc.device), sensor=0, seed=5, spp=spp)
        out.append((p.pos.cpu().clone(), p.nrm.cpu().clone()))
    for a, b, what in ((out[0][0], out[1][0], "pos"), (out[0][1], out[1][1], "nrm")):
        scale = float(a.abs().max())
        if what == "nrm" and name == "occluder_area_light":          # never shaded: the camera does not see it, depth 2
            assert scale == 0 and float(b.abs().max()) == 0
            continue
        assert scale > 0, what
        bad = ((a - b).abs() > 2e-2 * scale).float().mean()
        assert float(bad) < 0.02, (name, what, float(bad), scale)
        assert abs(float(a.sum() - b.sum())) < 2e-2 * float(a.abs().sum()), (name, what)


_MAX_REQ, _REQ_WORDS = 13, 16            # rp::kMaxReq requests per path of sizeof(rp::WarpReq) / 4 words (csrc/epsm_trace_reparam.h)


def _attached(name, res, spp, device="cuda"):
    sc = build(name, 0.0, res, spp, device)
    for m in CONFIGS[name]["moving"]:
        sc.attach(m, positions=True, normals=True)
    return sc


def _cfg_kw(name, rays=16):
    return dict(reparam_max_depth=CONFIGS[name]["max_depth"], reparam_rays=rays, kappa=CONFIGS[name].get("kappa", 1e5), exponent=3.0)


def _workspace_tables(sc, n):
    """The workspace a reparameterised pass left for n paths, as (kMaxReq, n, 16) request words and n counts: the requests,
    rounded up to 256 bytes, then the counts (epsm_trace_reparam_workspace_bytes)."""
    import ctypes as C
    req_bytes = (n * _MAX_REQ * _REQ_WORDS * 4 + 255) & ~255
    assert int(sc._runtime()[0].epsm_trace_reparam_workspace_bytes(C.c_int64(n))) == req_bytes + 4 * n
    ws = sc._reparam_ws.clone()
    req = ws[: n * _MAX_REQ * _REQ_WORDS * 4].view(torch.int32).view(_MAX_REQ, n, _REQ_WORDS)
    count = ws[req_bytes: req_bytes + 4 * n].view(torch.int32)
    return req.cpu(), count.cpu()


@pytest.mark.parametrize("name", ["sphere_on_glossy_floor", "diffuse_sphere_envmap"])
def test_both_passes_number_their_requests_alike(name):
    """Request n of path i is the same warp in the backward and in the forward pass -- the forward pass draws the backward's
    auxiliary rays only because of that.  Both passes leave their requests in the same workspace layout: the counts are equal
    and, below a path's count, the ray (o, d), em_inv_dist and the glued origin (ftri, fb1, fb2) are the same bits; gdir / gdiv
    hold adjoints in one and tangents in the other, and slots at or past the count are not written.  The glossy floor has warps
    of the ray into a vertex and of emitter rays at several depths, the envmap escaped rays and camera rays that hit nothing."""
    res, spp, seed = 16, 4, 3
    sc = _attached(name, res, spp)
    depth, n = CONFIGS[name]["max_depth"], sc.sensors[0].wavefront_size(spp)
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *shape: torch.randn(shape, generator=gen).to(sc.device)
    radiance = sc._trace(0, seed, spp, depth, 0, 0, n).radiance.contiguous()
    p = sc.param_grads()
    sc.trace_reparam(0, seed, spp, depth, 0, n, radiance, rnd(n, 3), rnd(n, 3), p.pos, p.nrm, **_cfg_kw(name))
    torch.cuda.synchronize()
    req_b, count_b = _workspace_tables(sc, n)
    sc.trace_reparam_forward(0, seed, spp, depth, 0, n, radiance, rnd(sc.V, 3), rnd(sc.V, 3), **_cfg_kw(name))
    torch.cuda.synchronize()
    req_f, count_f = _workspace_tables(sc, n)
    assert torch.equal(count_b, count_f)
    assert int(count_b.min()) >= 1 and int(count_b.max()) <= min(_MAX_REQ, 1 + 2 * depth)
    live = torch.arange(_MAX_REQ)[:, None] < count_b[None, :]                       # (kMaxReq, n)
    for what, words in (("o", [0, 1, 2]), ("d", [4, 5, 6]), ("em_inv_dist", [7]), ("fb1", [11]), ("ftri", [12]), ("fb2", [13])):
        assert torch.equal(req_b[:, :, words][live], req_f[:, :, words][live]), what
    # not vacuous: paths with the camera ray's warp alone, paths with three and more, three different counts at least
    hist = torch.bincount(count_b, minlength=_MAX_REQ + 1)
    print(f"{name}: {n} paths, requests per path {hist.tolist()}")
    assert int(hist[1]) > 0 and int(hist[3:].sum()) > 0 and int((hist > 0).sum()) >= 3, hist


_RAGGED = [(37, 1037), (1000, 1001)]      # 1 000 paths -- no multiple of 64 or 256 -- from a non-zero offset, and a single path


def test_forward_pass_on_ragged_ranges_gives_the_rows_of_the_whole_call():
    """``trace_reparam_forward`` on a tile that starts off a workgroup's boundary and ends off another: the rows of the call on
    [0, 2048), bit for bit -- no atomics, a path's streams are keyed by its wavefront index, and the wave-packet walk of stage 2
    gives every ray its own closest hit whoever its neighbours are (measured on the library before the passes shared their
    frame: MEASUREMENTS.md 26)."""
    name, res, spp, seed = "diffuse_sphere_area_light", 16, 8, 5
    sc = _attached(name, res, spp)
    depth = CONFIGS[name]["max_depth"]
    assert sc.sensors[0].wavefront_size(spp) >= 2048
    gen = torch.Generator().manual_seed(2)
    tan_pos, tan_nrm = (torch.randn((sc.V, 3), generator=gen).to(sc.device) for _ in range(2))
    radiance = sc._trace(0, seed, spp, depth, 0, 0, 2048).radiance.contiguous()
    whole = sc.trace_reparam_forward(0, seed, spp, depth, 0, 2048, radiance, tan_pos, tan_nrm, **_cfg_kw(name))
    assert float(whole[0].abs().max()) > 0 and float(whole[1].abs().max()) > 0
    for lo, hi in _RAGGED:
        part = sc.trace_reparam_forward(0, seed, spp, depth, lo, hi, radiance[lo:hi].contiguous(), tan_pos, tan_nrm, **_cfg_kw(name))
        for a, b, what in zip(part, whole, ("d_radiance", "d_film")):
            differ = int((a != b[lo:hi]).any(dim=1).sum())
            print(f"[{lo}, {hi}) {what}: {differ} of {hi - lo} rows differ")
            assert torch.equal(a, b[lo:hi]), (lo, hi, what, differ)


def test_backward_pass_on_ragged_ranges_equals_the_host_build():
    """The same ranges through ``trace_reparam`` against the host build's inline warps, under the bound of
    test_device_pass_equals_the_host_build."""
    name, res, spp, seed = "diffuse_sphere_area_light", 16, 8, 5
    depth = CONFIGS[name]["max_depth"]
    gen = torch.Generator().manual_seed(6)
    adj_radiance, adj_film = torch.randn((2048, 3), generator=gen), torch.randn((2048, 3), generator=gen)
    radiance, out = None, []
    for dev in ("cpu", "cuda"):
        sc = _attached(name, res, spp, dev)
        if radiance is None:
            radiance = sc._trace(0, seed, spp, depth, 0, 0, 2048).radiance.contiguous()
        grads = []
        for lo, hi in _RAGGED:
            p = sc.param_grads()
            sc.trace_reparam(0, seed, spp, depth, lo, hi, *(t[lo:hi].contiguous().to(sc.device) for t in (radiance, adj_radiance, adj_film)),
                             p.pos, p.nrm, **_cfg_kw(name))
            grads.append((p.pos.cpu().clone(), p.nrm.cpu().clone()))
        out.append(grads)
    for k, (lo, hi) in enumerate(_RAGGED):
        for a, b, what in zip(out[0][k], out[1][k], ("pos", "nrm")):
            scale = float(a.abs().max())
            bad = float(((a - b).abs() > 2e-2 * scale).float().mean())
            print(f"[{lo}, {hi}) {what}: scale {scale:.3e}, share beyond 2e-2 of it {bad:.4f}, sums {float(a.sum()):.4e} {float(b.sum()):.4e}")
            if hi - lo > 1:
                assert scale > 0, what
            assert bad < 0.02, (lo, hi, what, bad, scale)
            assert abs(float(a.sum() - b.sum())) <= 2e-2 * float(a.abs().sum()), (lo, hi, what)


@pytest.mark.parametrize("name,spp,tol", [
    ("scale_sphere_emitter_on_black", 2048, 0.1),    # :438-460
    ("self_shadow_point_light", 4096, 0.35),         # :551-596 (all-ones weights, as there: the ramp's answer is ~0)
    ("receiver_point_light", 256, 0.01),
    ("receiver_along_normal", 1024, 0.06),
    ("corner_along_normal", 1024, 0.06),
    ("rectangle_emitter_on_black", 2048, 0.2),       # error_mean_threshold_bwd of the config it restates (:383-410)
    ("sphere_emitter_on_black", 2048, 0.15),         # :413-435
    ("occluder_area_light", 4096, 0.25),             # :463-500
    ("sphere_on_glossy_floor", 4096, 0.2),           # :601-640
    ("diffuse_sphere_area_light", 4096, 0.15),
    # the reference's configs under its `constant` environment emitter, as it states them, at its thresholds and sample counts
    ("diffuse_sphere_constant", 1024, 0.25),         # :317-338
    ("diffuse_rectangle_constant", 1024, 0.25),      # :341-363
    ("shadow_receiver_constant", 4096, 0.25),        # :482-520
    ("sphere_on_glossy_floor_constant", 2048, 0.2),  # :600-637
    # the first of them under an `envmap` that varies with direction (no counterpart in the reference's list)
    ("textured_plane_constant", 800, 0.1),           # :523-550 (spp 800, error_mean_threshold 0.1 there)
    ("textured_plane_fills_the_view", 1024, 0.05),
    ("diffuse_sphere_envmap", 1024, 0.1),
    ("glossy_sphere_envmap", 1024, 0.1),
    # the sensor's own translation (ParamGrads.cam_origin): TranslateCameraConfig as stated (:639-674: res 16, spp 1024, 64 rays,
    # kappa 1e4; its thresholds are 0.3 / 1.6 forward and 1.3 backward under all-ones weights, where the answer is ~0 -- the ramp
    # makes the motion of the silhouette count) and a lit scene where shading and shadows move in the image too
    ("translate_camera", 1024, 0.3),
    ("translate_camera_lit", 2048, 0.2),
])
def test_backward_gradient_matches_finite_differences(name, spp, tol):
    got, fd, dt = fd_check(name, device="cuda", spp=spp, rays=64, seeds=2, fd_eps=0.0 if ("emitter" in name or "constant" in name or "envmap" in name or "textured" in name or "camera" in name) else 5e-3, fd_spp_mult=2,
                           weights="ones" if name == "self_shadow_point_light" else "ramp")
    r, g, f = rel(got, fd)
    print(f"{name}: grad {g:+.3f} per seed {[round(x, 2) for x in got]}, FD {f:+.3f} per seed {[round(x, 2) for x in fd]}, rel {r:.3f}, "
          f"{dt:.2f} s for the backward passes")
    assert r < tol, (name, g, f)


def test_vertex_normals_on_the_device():
    got, fd = fd_check_normals("diffuse_sphere_area_light", device="cuda", spp=1024, rays=16, fd_spp_mult=1)
    assert got * fd > 0 and abs(got - fd) < 0.12 * abs(fd), (got, fd)


def test_hybrid_second_phase_moves_geometry():
    """manifold_hybrid on the shadow experiment (EPSM/optim.py:87-119): the manifold phase brings the occluder's shadow
    near the target, then ``prb_reparam`` on sensor 0 with the L2 loss keeps moving the GEOMETRY (round 2: it stood still
    there) and ends closer."""
    from epsm_mitsuba3_amd.exp import shadow
    from epsm_mitsuba3_amd.optim import run
    old = shadow.thres
    shadow.thres = 25
    try:
        lines = []
        hist, opt = run("manifold_hybrid", "shadow", iterations=60, lr=0.02, log=lines.append)
    finally:
        shadow.thres = old
    assert "phase 2 = PRBReparamIntegrator" in lines[0]
    moved = abs(hist[-1] - hist[26])
    print("error at the switch", hist[25], "at the end", hist[-1], "history", [round(h, 3) for h in hist])
    assert moved > 1e-4                                       # the second phase moves the occluder
    assert np.mean(hist[-8:]) < 0.6 * hist[25] or np.mean(hist[-8:]) < 0.05 * hist[0], hist


def test_hybrid_on_the_mirror_experiment():
    """The shape of BASELINE.json's configs[3] (`manifold_hybrid` on objects seen in a mirror): after the manifold phase the
    reparameterised phase takes the three tiles from ~0.19 to ~0.035 of the target at 128 x 128 @ 64 spp (at the experiment
    file's 64 x 64 @ 16 spp it wanders in its noise: profiles/r03_g_hybrid_experiments.txt)."""
    from epsm_mitsuba3_amd.exp import bathroom
    from epsm_mitsuba3_amd.optim import run
    old = bathroom.thres, bathroom.spp, bathroom.resolution
    bathroom.thres, bathroom.spp, bathroom.resolution = 40, 64, 128
    try:
        hist, opt = run("manifold_hybrid", "bathroom", iterations=100, lr=0.02, log=lambda s: None)
    finally:
        bathroom.thres, bathroom.spp, bathroom.resolution = old
    print("at the switch", hist[40], "end", np.mean(hist[-10:]))
    assert np.mean(hist[-10:]) < 0.5 * hist[40] and np.mean(hist[-10:]) < 0.1 * hist[0], hist[36::4]


def test_prb_reparam_alone_refines_a_nearby_start():
    """``python -m epsm_mitsuba3_amd.optim prb_reparam shadow`` from a start whose shadow overlaps the target's (the regime
    the L2 loss works in, the reason for the hybrid scheme)."""
    from epsm_mitsuba3_amd.exp import shadow
    from epsm_mitsuba3_amd.optim import run
    old = shadow._TARGET_SHIFT.copy()
    shadow._TARGET_SHIFT[:] = [0.12, -0.08, 0.0]
    try:
        hist, opt = run("prb_reparam", "shadow", iterations=40, lr=0.01, log=lambda s: None)
    finally:
        shadow._TARGET_SHIFT[:] = old
    print([round(h, 4) for h in hist])
    assert np.mean(hist[-8:]) < 0.4 * hist[0], hist


def test_film_adjoint_kernel_matches_the_torch_form():
    """``epsm_film_adjoint_reparam`` (one HIP kernel; include/epsm_trace.h) against the dense torch form it replaced
    (integrators.film_adjoint_reparam_torch, itself checked against autograd of the splat in tests/test_reparam.py): samples
    inside the film, in its two-pixel border and beyond it, pixels without weight."""
    from epsm_mitsuba3_amd.integrators import film_adjoint_reparam, film_adjoint_reparam_torch
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(4)
    H, W, n = 37, 53, 20000
    pos = torch.stack([torch.rand(n, generator=g) * (W + 6) - 3, torch.rand(n, generator=g) * (H + 6) - 3], dim=1)
    pos[:50] = torch.tensor([10.5, 7.5])                              # exactly on a pixel centre
    rad = torch.rand((n, 3), generator=g) * 2
    grad = torch.randn((H, W, 3), generator=g)
    accum = torch.rand((H, W, 4), generator=g) + 0.2
    accum[5:8, 9:12] = 0.0                                             # pixels no sample reached
    a = film_adjoint_reparam(pos.to(dev), rad.to(dev), grad.to(dev), accum.to(dev))
    b = film_adjoint_reparam_torch(pos.to(dev), rad.to(dev), grad.to(dev), accum.to(dev))
    torch.cuda.synchronize()
    for x, y, name in zip(a, b, ("dL", "adj")):
        m = float(y.abs().max())
        assert m > 0 and float((x - y).abs().max()) <= 2e-5 * m, (name, float((x - y).abs().max()) / m)
    # a gradient image with more channels than three (the caller's (H,W,5) crop): the first three are read
    grad5 = torch.cat([grad, torch.randn((H, W, 2), generator=g)], dim=2).to(dev)
    c = film_adjoint_reparam(pos.to(dev), rad.to(dev), grad5, accum.to(dev))
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])
