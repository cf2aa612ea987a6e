"""The conductor material adjoint on the GPU (epsm_trace_paths_material_backward / _forward): the device passes against the host
build of the same per-path code, the transpose identity on the device, the bit-for-bit repeatability of the atomic-free reduction,
one tile against its two halves, the closed forms through the device probe, the 5-channel branch, and the metal experiment of
exp/metal.py.  The shape is the two-plate scene at 11 x 11 @ 32 spp: 11 * 11 * 32 = 3872 paths (this sensor has no sample
border), 30 workgroups and a tail of 32 lanes -- the ride-along lanes and the partial last row are exercised."""
import ctypes as C

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd import optim
from test_material_adjoint import (PROBE_FRESNEL_CONDUCTOR_GRAD, TRANSPOSE, attach_two, check_fresnel_probe, transpose_gap,
                                   two_metal_scene)

pytestmark = pytest.mark.gpu

RES, SPP, PATHS = 11, 32, 3872


def _replay(sc, seed, spp, depth, adj, tangent, lo=0, hi=None):
    """Both passes over the paths [lo, hi) of sensor 0, by default all of them: (d loss / d material (M,3,3), d radiance for
    `tangent`, the primal radiance)."""
    if hi is None:
        hi = sc.sensors[0].wavefront_size(spp)
        assert hi == PATHS and hi % 128 == 32
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, lo, hi)
    radiance = radiance.contiguous()
    grad = torch.zeros((len(sc.material_slots), 3, 3), device=sc.device)
    sc.trace_material_backward(0, seed, spp, depth, lo, hi, radiance, adj.to(sc.device), grad)
    d_rad = sc.trace_material_forward(0, seed, spp, depth, lo, hi, radiance, tangent.to(sc.device))
    return grad.cpu(), d_rad.cpu(), radiance.cpu()


@pytest.mark.parametrize("integ_name", list(TRANSPOSE))
@pytest.mark.parametrize("depth", [2, 4])
def test_device_passes_match_the_host_twin(integ_name, depth):
    seed = 11
    dev, host = two_metal_scene("cuda", RES, SPP), two_metal_scene("cpu", RES, SPP)
    TRANSPOSE[integ_name](dev); TRANSPOSE[integ_name](host)
    gen = torch.Generator().manual_seed(depth)
    adj = torch.randn((PATHS, 3), generator=gen)
    tangent = torch.randn((2, 3, 3), generator=gen)
    gd, fd_, rd = _replay(dev, seed, SPP, depth, adj, tangent)
    gh, fh, rh = _replay(host, seed, SPP, depth, adj, tangent)
    print(f"{integ_name} depth {depth}: radiance gap {float((rd - rh).abs().sum()) / float(rh.abs().sum()):.3e}, backward gap "
          f"{float((gd - gh).abs().sum()) / float(gh.abs().sum()):.3e}, forward gap {float((fd_ - fh).abs().sum()) / float(fh.abs().sum()):.3e}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    assert float(gh.abs().min()) > 0
    assert float((gd - gh).abs().sum()) <= 2e-3 * float(gh.abs().sum()), (gd, gh)
    assert float(fh.abs().sum()) > 0
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())
    # through the integrator too: render_backward on the device against the twin
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    g = torch.randn((RES, RES, 3), generator=torch.Generator().manual_seed(7))
    pd, ph = dev.param_grads(), host.param_grads()
    integ.render_backward(dev, pd, g.to(dev.device), sensor=0, seed=seed, spp=SPP)
    integ.render_backward(host, ph, g, sensor=0, seed=seed, spp=SPP)
    gap = float((pd.conductor.cpu() - ph.conductor).abs().sum()) / float(ph.conductor.abs().sum())
    print(f"{integ_name} depth {depth}: ParamGrads.conductor gap {gap:.3e}")
    assert gap <= 2e-3, (pd.conductor, ph.conductor)


@pytest.mark.parametrize("integ_name", list(TRANSPOSE))
@pytest.mark.parametrize("depth", [2, 4])
def test_device_forward_is_the_transpose_of_the_device_backward(integ_name, depth):
    sc = two_metal_scene("cuda", RES, SPP)
    TRANSPOSE[integ_name](sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params = transpose_gap(integ, sc, 5, SPP, torch.Generator().manual_seed(2 + depth))
    print(f"{integ_name} depth {depth}: transpose gap {gap / S_:.3e}")
    assert S_ > 0 and abs(a) > 0 and float(params.conductor.abs().min()) > 0
    assert gap <= 2e-3 * S_, (gap, S_)


def test_two_backward_calls_give_identical_bits():
    sc = two_metal_scene("cuda", RES, SPP)
    attach_two(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 4})
    g = torch.randn((RES, RES, 3), generator=torch.Generator().manual_seed(3)).to(sc.device)
    p1, p2 = sc.param_grads(), sc.param_grads()
    integ.render_backward(sc, p1, g, sensor=0, seed=4, spp=SPP)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=SPP)
    assert float(p1.conductor.abs().min()) > 0
    assert torch.equal(p1.conductor, p2.conductor)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=SPP)
    assert torch.equal(p2.conductor, 2 * p1.conductor)                  # gradients accumulate


def test_one_tile_equals_the_sum_of_its_halves():
    """Split at path 1500, no multiple of 128: the halves' rows hold other groups of 128 paths than the whole tile's.  The adjoint
    is positive (0.5 + uniform), so that every one of the 18 sums is a sum of terms of one sign by and large and its relative gap
    measures the order of the additions, not a cancellation."""
    depth, seed, cut = 3, 9, 1500
    sc = two_metal_scene("cuda", RES, SPP)
    attach_two(sc)
    n = sc.sensors[0].wavefront_size(SPP)
    assert n == PATHS and cut % 128 != 0
    _, radiance, _ = sc.trace_color(0, seed, SPP, depth, 0, n)
    radiance = radiance.contiguous()
    adj = (0.5 + torch.rand((n, 3), generator=torch.Generator().manual_seed(1))).to(sc.device)
    whole = torch.zeros((2, 3, 3), device=sc.device)
    sc.trace_material_backward(0, seed, SPP, depth, 0, n, radiance, adj, whole)
    halves = torch.zeros((2, 3, 3), device=sc.device, dtype=torch.float64)
    for lo, hi in ((0, cut), (cut, n)):
        part = torch.zeros((2, 3, 3), device=sc.device)
        sc.trace_material_backward(0, seed, SPP, depth, lo, hi, radiance[lo:hi].contiguous(), adj[lo:hi].contiguous(), part)
        halves += part.double()
    rel = ((whole.double() - halves).abs() / halves.abs()).cpu()
    print(f"whole tile vs halves: relative gap {rel.flatten().tolist()}")
    assert float(halves.abs().min()) > 0
    assert float(rel.max()) <= 1e-6, (whole, halves)


def _ragged_pair(lo, hi):
    """The two-metal scene at 16 x 16 @ 8 spp (2048 paths), both passes over [lo, hi) on the device and on the host twin."""
    spp, seed, depth = 8, 7, 3
    dev, host = two_metal_scene("cuda", 16, spp), two_metal_scene("cpu", 16, spp)
    attach_two(dev); attach_two(host)
    assert dev.sensors[0].wavefront_size(spp) >= hi
    gen = torch.Generator().manual_seed(lo)
    adj = torch.randn((hi - lo, 3), generator=gen)
    tangent = torch.randn((2, 3, 3), generator=gen)
    return _replay(dev, seed, spp, depth, adj, tangent, lo, hi), _replay(host, seed, spp, depth, adj, tangent, lo, hi)


@pytest.mark.parametrize("lo,hi", [(1000, 1040), (960, 1025), (960, 1089), (960, 1153), (900, 1901)])
def test_ragged_path_counts(lo, hi):
    """Path counts that leave lanes and whole waves of the reducing kernel without a path: 40 paths that start inside a wave of
    the full launch (the workgroup's second wave is idle), 65 (one lane in the second wave), 129 (the second workgroup has one
    lane: its second wave is idle and still owes the reduction its zeros), 193, and a ragged tile of eight workgroups."""
    (gd, fd_, rd), (gh, fh, rh) = _ragged_pair(lo, hi)
    print(f"[{lo}, {hi}): radiance gap {float((rd - rh).abs().sum()) / float(rh.abs().sum()):.3e}, backward gap "
          f"{float((gd - gh).abs().sum()) / float(gh.abs().sum()):.3e}, forward gap {float((fd_ - fh).abs().sum()) / float(fh.abs().sum()):.3e}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    assert float(gh.abs().min()) > 0
    assert float((gd - gh).abs().sum()) <= 2e-3 * float(gh.abs().sum()), (gd, gh)
    assert float(fh.abs().sum()) > 0
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())


def test_one_path_that_misses_the_plates_gives_zeros():
    """[1000, 1001): 127 of the workgroup's 128 lanes ride along; the one path sees no plate, and zero is the answer."""
    (gd, fd_, rd), (gh, fh, rh) = _ragged_pair(1000, 1001)
    print(f"[1000, 1001): radiance {rd.tolist()} / {rh.tolist()}, backward {gd.flatten().tolist()} / {gh.flatten().tolist()}, "
          f"forward {fd_.tolist()} / {fh.tolist()}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    assert float(gh.abs().sum()) == 0 and torch.equal(gd, gh)
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())      # (exact where the twin gives zeros)


def test_fresnel_derivatives_on_the_device():
    """The closed forms as the kernels run them: the assertions of the CPU test (test_material_adjoint.check_fresnel_probe)."""
    from epsm_mitsuba3_amd import _lib
    lib = _lib.lib()
    lib.epsm_probe.restype = C.c_int
    dev = torch.device("cuda", 0)

    def probe(rows):
        inp = torch.zeros((rows.shape[0], 8), device=dev)
        inp[:, : rows.shape[1]] = torch.from_numpy(rows).to(dev)
        out = torch.zeros((rows.shape[0], 16), device=dev)
        with torch.cuda.device(dev):
            rc = lib.epsm_probe(C.c_int(PROBE_FRESNEL_CONDUCTOR_GRAD), C.c_int64(rows.shape[0]), C.c_void_p(inp.data_ptr()),
                                C.c_void_p(out.data_ptr()), None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _lib.check(rc, "epsm_probe")
        torch.cuda.synchronize()
        return out.cpu().numpy().astype(np.float32)
    check_fresnel_probe(probe)


def test_five_channel_branch_leaves_conductor_zero():
    """The half-vector constraint does not depend on eta, k or the tint: the manifold integrators' 5-channel pass (which runs on
    the device only) gives the material slots nothing, and zero is the answer."""
    sc = two_metal_scene("cuda", RES, SPP)
    attach_two(sc)
    sc.attach("plate2")
    integ = epsm.load_dict({"type": "manifold", "max_depth": 3})
    p = sc.param_grads()
    g = (torch.randn((RES, RES, 5), generator=torch.Generator().manual_seed(1)) * 1e-3).to(sc.device)
    img = integ.render(sc, sensor=0, seed=2, spp=SPP)
    integ.render_backward(sc, p, g, sensor=0, seed=2, spp=SPP)
    print(f"5-channel pass: |image| {float(img.abs().sum()):.3e}, |params.flat| {float(p.flat.abs().sum()):.3e}")
    assert img.shape[-1] == 5 and float(img.abs().sum()) > 0
    assert float(p.conductor.abs().sum()) == 0


def test_metal_experiment_recovers_the_reflectance():
    from epsm_mitsuba3_amd.exp import metal
    hist, opt = optim.run("prb", "metal", iterations=40, log=lambda s: None)
    first, last = metal.param_errors[0], metal.param_errors[-1]
    print(f"metal experiment: |F(1) R - target| {hist[0]:.4f} -> {hist[-1]:.4f}; |specular_reflectance - target| {first[0]:.4f} -> "
          f"{last[0]:.4f}, |k - target| {first[1]:.4f} -> {last[1]:.4f}")
    assert all(bool(torch.isfinite(g).all()) and float(g[1:].abs().sum()) > 0 for g in metal.material_grads)
    # measured on the MI355X: 0.1691 -> 0.0064 (26 x), specular_reflectance 0.1667 -> 0.0730, k 0.5333 -> 0.1687; asserted with a
    # margin of 3 x on the product the image pins down and of 1.5 x on the two factors, which it separates only through the angles
    assert hist[-1] < hist[0] / 8, hist
    assert last[0] < first[0] / 1.5 and last[1] < first[1] / 2, metal.param_errors
