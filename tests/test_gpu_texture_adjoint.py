"""The texel adjoint on the GPU (epsm_trace_paths_texture_backward / _forward): the device passes against the host build of the
same per-path code -- on a scene where the lanes of a wave share one footprint (a 2 x 2 texture magnified over the floor, an
envmap seen directly: the merge before the atomics) and on one of mostly distinct footprints (a 1024^2 texture) -- the transpose
identity on the device, and the texture experiment of exp/texture.py."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd import optim
from test_texture_adjoint import env_bitmap, floor_texture, texture_scene, transpose_gap

pytestmark = pytest.mark.gpu

SCENES = {
    # every lane of a primary-ray wave (64 samples of one pixel) on the same 2 x 2 footprint, and the sky above the wall
    "shared_footprints": dict(tex=floor_texture(2, 2), env=env_bitmap(), env_scale=0.8),
    "nearest": dict(tex=floor_texture(2, 2), nearest=True, env=env_bitmap()),
    # a 1024^2 texture over the floor: neighbouring samples mostly on distinct texels
    "distinct_footprints": dict(tex=floor_texture(1024, 1024)),
}


def _pair(name, res=16, spp=64):
    return texture_scene("cuda", res, spp, **SCENES[name]), texture_scene("cpu", res, spp, **SCENES[name])


def _attach(sc):
    slots = [sc.attach_texture("floor.bsdf")]
    if "sky" in sc.emitter_names:
        slots.append(sc.attach_texture("sky"))
    return slots


def _replay(sc, seed, spp, depth, adj, lo=0, hi=None):
    """Both texel passes over the paths [lo, hi) of sensor 0, by default all of them: (texel gradients per slot, d radiance for
    the tangent 1 + texel index)."""
    hi = sc.sensors[0].wavefront_size(spp) if hi is None else hi
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, lo, hi)
    radiance = radiance.contiguous()
    shapes = sc.texture_shapes()
    grads = [torch.zeros((h, w, 3), device=sc.device) for h, w in shapes]
    sc.trace_texture_backward(0, seed, spp, depth, lo, hi, radiance, adj.to(sc.device), grads)
    tans = [torch.from_numpy(np.cos(np.arange(h * w * 3, dtype=np.float32) * 0.37).reshape(h, w, 3)).to(sc.device) for h, w in shapes]
    d_rad = sc.trace_texture_forward(0, seed, spp, depth, lo, hi, radiance, tans)
    return [g.cpu() for g in grads], d_rad.cpu(), radiance.cpu()


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("depth", [2, 4])
def test_device_passes_match_the_host_twin(name, depth):
    spp, seed = 64, 11
    dev, host = _pair(name, spp=spp)
    _attach(dev); _attach(host)
    n = dev.sensors[0].wavefront_size(spp)
    adj = torch.randn((n, 3), generator=torch.Generator().manual_seed(depth))
    gd, fd_, rd = _replay(dev, seed, spp, depth, adj)
    gh, fh, rh = _replay(host, seed, spp, depth, adj)
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    for a, b in zip(gd, gh):
        assert float(b.abs().sum()) > 0
        assert float((a - b).abs().sum()) <= 2e-3 * float(b.abs().sum()), (float((a - b).abs().sum()), float(b.abs().sum()))
    assert float(fh.abs().sum()) > 0
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())


@pytest.mark.parametrize("res,spp,lo,hi", [(5, 5, 0, 125), (9, 3, 0, 243), (16, 8, 100, 1001)])
def test_ragged_path_counts(res, spp, lo, hi):
    """The count shapes of test_gpu_alpha_texture.py: 125 paths, less than one workgroup; 243, a workgroup and a ragged second;
    a tile that starts at path 100 -- inside a wave of the full launch -- and ends at 1001.  Floor texture and envmap attached."""
    dev, host = _pair("shared_footprints", res, spp)
    _attach(dev); _attach(host)
    assert dev.sensors[0].wavefront_size(spp) >= hi and (lo == 0 or lo % 64 != 0)
    adj = torch.randn((hi - lo, 3), generator=torch.Generator().manual_seed(3 + lo))
    gd, fd_, rd = _replay(dev, 7, spp, 3, adj, lo, hi)
    gh, fh, rh = _replay(host, 7, spp, 3, adj, lo, hi)
    print(f"{res}x{res} @ {spp} [{lo}, {hi}): radiance gap {float((rd - rh).abs().sum()) / float(rh.abs().sum()):.3e}, backward gaps "
          f"{[float((a - b).abs().sum()) / float(b.abs().sum()) for a, b in zip(gd, gh)]}, forward gap "
          f"{float((fd_ - fh).abs().sum()) / float(fh.abs().sum()):.3e}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    for a, b in zip(gd, gh):
        assert float(b.abs().sum()) > 0
        assert float((a - b).abs().sum()) <= 2e-3 * float(b.abs().sum()), (float((a - b).abs().sum()), float(b.abs().sum()))
    assert float(fh.abs().sum()) > 0
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())


def test_merge_sees_shared_footprints():
    """The 2 x 2 texture is seen by every sample of a pixel: the per-texel sums are those of ~N items each (no add lost)."""
    spp, seed = 64, 3
    dev, host = _pair("shared_footprints", res=32, spp=spp)
    dev.attach_texture("floor.bsdf"); host.attach_texture("floor.bsdf")
    n = dev.sensors[0].wavefront_size(spp)
    adj = torch.ones((n, 3))
    gd, _, _ = _replay(dev, seed, spp, 2, adj)
    gh, _, _ = _replay(host, seed, spp, 2, adj)
    torch.testing.assert_close(gd[0], gh[0], rtol=1e-3, atol=1e-3 * float(gh[0].abs().max()))


@pytest.mark.parametrize("name", ["with_colour_slot", "bitmap_and_envmap", "envmap"])
def test_device_forward_is_the_transpose_of_the_device_backward(name):
    from test_texture_adjoint import TRANSPOSE
    make, integ_name, attach = TRANSPOSE[name]
    import test_texture_adjoint as T
    kw = {"with_colour_slot": dict(env=env_bitmap()), "bitmap_and_envmap": dict(env=env_bitmap()),
          "envmap": dict(env=env_bitmap(), env_scale=0.7, light=False)}[name]
    sc = T.texture_scene("cuda", **kw)
    attach(sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": 3})
    gap, S_, a = transpose_gap(integ, sc, 5, 32, torch.Generator().manual_seed(2))
    assert S_ > 0 and abs(a) > 0
    assert gap <= 2e-3 * S_, (gap, S_)


def test_texture_experiment_lowers_the_texel_error():
    hist, opt = optim.run("prb", "texture", iterations=40, log=lambda s: None)
    assert hist[-1] < hist[0] / 3, hist
