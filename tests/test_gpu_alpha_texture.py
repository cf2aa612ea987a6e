"""Roughness maps on the GPU (epsm_trace_paths_alpha_texture_backward / _forward): the device passes against the host build of the
same per-path code -- with the wave-level merge taken and not taken, footprints across the map's borders, fewer paths than a
workgroup and a tile that starts inside a wave --, the transpose identity on the device, and exp/roughness_map.py.  The pass uses
float atomics: nothing here asks for repeatable bits."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd import optim
from test_alpha_texture import (TRANSPOSE, UV, _both_maps, alpha_bitmap, attach_maps, checker, filling_plate_map, map_scene,
                                transpose_gap)

pytestmark = pytest.mark.gpu


def _replay(sc, seed, spp, depth, lo, hi, adj, tangents):
    """Both passes over paths [lo, hi) of sensor 0: (texel gradients per slot, d radiance for `tangents`, the primal radiance)."""
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, lo, hi)
    radiance = radiance.contiguous()
    grads = [torch.zeros(tuple(t.shape), device=sc.device) for t in tangents]
    sc.trace_alpha_texture_backward(0, seed, spp, depth, lo, hi, radiance, adj.to(sc.device), grads)
    d_rad = sc.trace_alpha_texture_forward(0, seed, spp, depth, lo, hi, radiance, [t.to(sc.device) for t in tangents])
    return [g.cpu() for g in grads], d_rad.cpu(), radiance.cpu()


def _check_against_twin(what, dev, host, seed, spp, depth, lo=0, hi=None):
    """The device's passes over [lo, hi) against the host twin's: 1e-3 for the radiance and 2e-3 for the rest as a sum norm (those
    of test_gpu_alpha_adjoint), and no single texel further off than 2e-3 of the largest."""
    attach_maps(dev); attach_maps(host)
    n = dev.sensors[0].wavefront_size(spp)
    hi = n if hi is None else hi
    gen = torch.Generator().manual_seed(depth + lo)
    adj = torch.randn((hi - lo, 3), generator=gen)
    tangents = [torch.randn(tuple(t.shape), generator=gen) for t in host.param_grads()._tex]
    gd, fd_, rd = _replay(dev, seed, spp, depth, lo, hi, adj, tangents)
    gh, fh, rh = _replay(host, seed, spp, depth, lo, hi, adj, tangents)
    gd, gh = torch.cat([g.reshape(-1) for g in gd]), torch.cat([g.reshape(-1) for g in gh])
    print(f"{what}: {hi - lo} paths; radiance gap {float((rd - rh).abs().sum()) / float(rh.abs().sum()):.3e}, backward gap "
          f"{float((gd - gh).abs().sum()) / float(gh.abs().sum()):.3e} (max norm {float((gd - gh).abs().max()) / float(gh.abs().max()):.3e}, "
          f"{int((gh != 0).sum())} of {gh.numel()} texels touched), forward gap {float((fd_ - fh).abs().sum()) / float(fh.abs().sum()):.3e}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    assert float(gh.abs().sum()) > 0 and float(fh.abs().sum()) > 0
    assert float((gd - gh).abs().sum()) <= 2e-3 * float(gh.abs().sum())
    assert float((gd - gh).abs().max()) <= 2e-3 * float(gh.abs().max())
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())
    return gh


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("depth", [2, 4])
def test_device_passes_match_the_host_twin(nearest, depth):
    spp, seed = 64, 11
    dev, host = _both_maps(nearest, "cuda", res=16, spp=spp), _both_maps(nearest, "cpu", res=16, spp=spp)
    _check_against_twin(f"two plates nearest={nearest} depth {depth}", dev, host, seed, spp, depth)
    # through the integrator too: render_backward on the device against the twin
    integ = epsm.load_dict({"type": "prb", "max_depth": depth})
    g = torch.randn((16, 16, 3), generator=torch.Generator().manual_seed(7))
    pd, ph = dev.param_grads(), host.param_grads()
    integ.render_backward(dev, pd, g.to(dev.device), sensor=0, seed=seed, spp=spp)
    integ.render_backward(host, ph, g, sensor=0, seed=seed, spp=spp)
    for k in range(2):
        d, h = pd.texture(k).cpu(), ph.texture(k)
        assert float(h.abs().sum()) > 0
        assert float((d - h).abs().sum()) <= 2e-3 * float(h.abs().sum()), (d, h)
        assert float((d - h).abs().max()) <= 2e-3 * float(h.abs().max()), (d, h)


def test_every_wave_shares_footprints():
    """A film-filling plate under a 2 x 2 bilinear map: 64 samples of a pixel are one wave, and all of them sit between the same
    four texels -- the merge branch is taken by every wave."""
    values = np.array([[0.25, 0.32], [0.3, 0.27]], np.float32)
    mk = lambda device: filling_plate_map("ggx", "area", values, res=8, spp=64, device=device, nearest=False)
    gh = _check_against_twin("shared footprints", mk("cuda"), mk("cpu"), 3, 64, 2)
    assert int((gh != 0).sum()) == 4


def test_adjacent_lanes_on_different_texels():
    """The same plate under a 64 x 64 `nearest` map repeated 8 times across it: a pixel spans some 40 texels each way, so the
    samples of a pixel -- adjacent lanes -- land on different texels and most waves have no footprint to merge."""
    values = checker(64, 64, seed=3)
    mk = lambda device: filling_plate_map("beckmann", "area", values, res=8, spp=64, device=device, nearest=True, uv=8.0 * UV)
    gh = _check_against_twin("distinct footprints", mk("cuda"), mk("cpu"), 3, 64, 2)
    assert int((gh != 0).sum()) > 1000


def test_footprints_across_the_borders_wrap():
    """Texture coordinates over [-0.5, 1.5]^2 on a 4 x 4 bilinear map: footprints straddle both borders and wrap around."""
    uv = 2.0 * UV - 0.5
    mk = lambda device: map_scene(device, res=16, spp=64, alpha=alpha_bitmap(checker(), False), uv=uv)
    gh = _check_against_twin("wrap", mk("cuda"), mk("cpu"), 5, 64, 3)
    assert int((gh != 0).sum()) == 16


@pytest.mark.parametrize("res,spp,lo,hi", [(5, 5, 0, 125), (9, 3, 0, 243), (16, 8, 100, 1001)])
def test_ragged_path_counts(res, spp, lo, hi):
    """125 paths: less than one workgroup; 243: a workgroup and a ragged second; a tile that starts at path 100 -- inside a wave of
    the full launch -- and ends at 1001."""
    mk = lambda device: map_scene(device, res=res, spp=spp, alpha=alpha_bitmap(checker(), False))
    dev = mk("cuda")
    assert dev.sensors[0].wavefront_size(spp) >= hi and (lo == 0 or lo % 64 != 0)
    _check_against_twin(f"{res}x{res} @ {spp} [{lo}, {hi})", dev, mk("cpu"), 7, spp, 3, lo, hi)


@pytest.mark.parametrize("name,depth", [("bilinear", 2), ("nearest", 4), ("with_colour_and_bitmap", 3), ("prb_reparam_no_geometry", 3)])
def test_device_forward_is_the_transpose_of_the_device_backward(name, depth):
    make, integ_name, attach = TRANSPOSE[name]
    sc = make(device="cuda")
    attach(sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params = transpose_gap(integ, sc, 5, 32, torch.Generator().manual_seed(2 + depth))
    print(f"{name} depth {depth}: transpose gap {gap / S_:.3e}")
    assert S_ > 0 and abs(a) > 0
    assert all(float(params.texture(k).abs().sum()) > 0 for k in sc.alpha_map_slots())
    assert gap <= 2e-3 * S_, (gap, S_)


def test_roughness_map_experiment_recovers_the_checker():
    hist, opt = optim.run("prb", "roughness_map", iterations=40, log=lambda s: None)
    print(f"roughness map experiment: mean |alpha - target| {hist[0]:.4f} -> {hist[-1]:.4f} ({hist[-1] / hist[0]:.3f}); history {hist}")
    assert hist[-1] < hist[0] / 3, hist
