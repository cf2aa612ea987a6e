"""The roughness adjoint on the GPU (epsm_trace_paths_bsdf_backward / _forward): the device passes against the host build of the
same per-path code, the transpose identity on the device, the bit-for-bit repeatability of the atomic-free reduction, one large
tile against its two halves, and the roughness experiment of exp/roughness.py."""
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd import optim
from test_alpha_adjoint import TRANSPOSE, attach_two, transpose_gap, two_plate_scene

pytestmark = pytest.mark.gpu


def _replay(sc, seed, spp, depth, adj, tangent, lo=0, hi=None):
    """Both passes over the paths [lo, hi) of sensor 0, by default all of them: (d loss / d alpha per slot, d radiance for
    `tangent`, the primal radiance)."""
    hi = sc.sensors[0].wavefront_size(spp) if hi is None else hi
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, lo, hi)
    radiance = radiance.contiguous()
    grad = torch.zeros(len(sc.alpha_slots), device=sc.device)
    sc.trace_alpha_backward(0, seed, spp, depth, lo, hi, radiance, adj.to(sc.device), grad)
    d_rad = sc.trace_alpha_forward(0, seed, spp, depth, lo, hi, radiance, tangent.to(sc.device))
    return grad.cpu(), d_rad.cpu(), radiance.cpu()


@pytest.mark.parametrize("integ_name", list(TRANSPOSE))
@pytest.mark.parametrize("depth", [2, 4])
def test_device_passes_match_the_host_twin(integ_name, depth):
    spp, seed = 64, 11
    dev, host = two_plate_scene("cuda", 16, spp), two_plate_scene("cpu", 16, spp)
    TRANSPOSE[integ_name](dev); TRANSPOSE[integ_name](host)
    n = dev.sensors[0].wavefront_size(spp)
    adj = torch.randn((n, 3), generator=torch.Generator().manual_seed(depth))
    tangent = torch.tensor([0.7, -1.3])
    gd, fd_, rd = _replay(dev, seed, spp, depth, adj, tangent)
    gh, fh, rh = _replay(host, seed, spp, depth, adj, tangent)
    print(f"{integ_name} depth {depth}: radiance gap {float((rd - rh).abs().sum()) / float(rh.abs().sum()):.3e}, backward gap "
          f"{float((gd - gh).abs().sum()) / float(gh.abs().sum()):.3e}, forward gap {float((fd_ - fh).abs().sum()) / float(fh.abs().sum()):.3e}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    assert float(gh.abs().min()) > 0
    assert float((gd - gh).abs().sum()) <= 2e-3 * float(gh.abs().sum()), (gd, gh)
    assert float(fh.abs().sum()) > 0
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())
    # through the integrator too: render_backward / render_forward on the device against the twin
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    g = torch.randn((16, 16, 3), generator=torch.Generator().manual_seed(7))
    pd, ph = dev.param_grads(), host.param_grads()
    integ.render_backward(dev, pd, g.to(dev.device), sensor=0, seed=seed, spp=spp)
    integ.render_backward(host, ph, g, sensor=0, seed=seed, spp=spp)
    assert float((pd.alpha.cpu() - ph.alpha).abs().sum()) <= 2e-3 * float(ph.alpha.abs().sum()), (pd.alpha, ph.alpha)


@pytest.mark.parametrize("integ_name", list(TRANSPOSE))
@pytest.mark.parametrize("depth", [2, 4])
def test_device_forward_is_the_transpose_of_the_device_backward(integ_name, depth):
    sc = two_plate_scene("cuda")
    TRANSPOSE[integ_name](sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params = transpose_gap(integ, sc, 5, 32, torch.Generator().manual_seed(2 + depth))
    print(f"{integ_name} depth {depth}: transpose gap {gap / S_:.3e}")
    assert S_ > 0 and abs(a) > 0 and float(params.alpha.abs().min()) > 0
    assert gap <= 2e-3 * S_, (gap, S_)


def test_two_backward_calls_give_identical_bits():
    sc = two_plate_scene("cuda", 32, 64)
    attach_two(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 4})
    g = torch.randn((32, 32, 3), generator=torch.Generator().manual_seed(3)).to(sc.device)
    p1, p2 = sc.param_grads(), sc.param_grads()
    integ.render_backward(sc, p1, g, sensor=0, seed=4, spp=64)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=64)
    assert float(p1.alpha.abs().min()) > 0
    assert torch.equal(p1.alpha, p2.alpha)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=64)
    assert torch.equal(p2.alpha, 2 * p1.alpha)                           # gradients accumulate


def test_one_large_tile_equals_the_sum_of_its_halves():
    res, spp, depth, seed = 128, 64, 3, 9
    sc = two_plate_scene("cuda", res, spp)
    attach_two(sc)
    n = sc.sensors[0].wavefront_size(spp)
    assert n >= 2 ** 20 and n % 256 == 0
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, 0, n)
    radiance = radiance.contiguous()
    adj = torch.randn((n, 3), generator=torch.Generator().manual_seed(1)).to(sc.device)
    whole = torch.zeros(2, device=sc.device)
    sc.trace_alpha_backward(0, seed, spp, depth, 0, n, radiance, adj, whole)
    halves = torch.zeros(2, device=sc.device, dtype=torch.float64)
    for lo, hi in ((0, n // 2), (n // 2, n)):
        part = torch.zeros(2, device=sc.device)
        sc.trace_alpha_backward(0, seed, spp, depth, lo, hi, radiance[lo:hi].contiguous(), adj[lo:hi].contiguous(), part)
        halves += part.double()
    rel = ((whole.double() - halves).abs() / halves.abs()).cpu()
    print(f"whole tile vs halves: relative gap {rel.tolist()}")
    assert float(halves.abs().min()) > 0
    assert float(rel.max()) <= 1e-6, (whole, halves)


def _ragged_pair(lo, hi):
    """The two-plate scene at 16 x 16 @ 8 spp (2048 paths), both passes over [lo, hi) on the device and on the host twin."""
    spp, seed, depth = 8, 7, 3
    dev, host = two_plate_scene("cuda", 16, spp), two_plate_scene("cpu", 16, spp)
    attach_two(dev); attach_two(host)
    assert dev.sensors[0].wavefront_size(spp) >= hi
    adj = torch.randn((hi - lo, 3), generator=torch.Generator().manual_seed(lo))
    tangent = torch.tensor([0.7, -1.3])
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
    print(f"[1000, 1001): radiance {rd.tolist()} / {rh.tolist()}, backward {gd.tolist()} / {gh.tolist()}, forward {fd_.tolist()} / {fh.tolist()}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    assert float(gh.abs().sum()) == 0 and torch.equal(gd, gh)
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())      # (exact where the twin gives zeros)


def test_roughness_experiment_recovers_alpha():
    hist, opt = optim.run("prb", "roughness", iterations=40, log=lambda s: None)
    print(f"roughness experiment: |alpha - target| {hist[0]:.4f} -> {hist[-1]:.4f}")
    assert hist[-1] < hist[0] / 3, hist


def test_hybrid_scheme_keeps_differentiating_alpha_after_the_switch():
    from epsm_mitsuba3_amd.exp import roughness
    optim.run("manifold_hybrid", "roughness", iterations=roughness.thres + 2, log=lambda s: None)
    after = roughness.alpha_grads[roughness.thres:]
    print(f"hybrid: d loss / d alpha per iteration {roughness.alpha_grads}")
    assert len(after) == 2 and all(g != 0 and g == g for g in after), roughness.alpha_grads
