"""Per-vertex colours on the GPU (an EpsmTexture of kind EPSM_TEXTURE_VERTEX_RGB through epsm_trace_paths_texture_backward /
_forward): the device passes against the host build of the same per-path code on the flat floor (A) and the ball (B) of
tests/_vertex_scenes.py, ragged path counts, the merge before the atomics -- on a 2-triangle floor, where the lanes of a wave share a
footprint, and on a 65 x 65 vertex grid, where they share vertices but not footprints --, both tracer forms, the transpose identity
on the device, and the experiment of exp/vertex_albedo.py."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _scenes import sensor
from _vertex_scenes import scene_a, scene_b, vertex_plane
from epsm_mitsuba3_amd import optim
from test_texture_adjoint import transpose_gap

pytestmark = pytest.mark.gpu

SCENES = {"A": (scene_a, "floor"), "B": (scene_b, "ball"),
          # B with the ball turned by 10 degrees: no triangle's geometric normal has a zero component
          "B_tilted": (lambda *a, **kw: scene_b(*a, tilt=10.0, **kw), "ball")}


def _pair(name, res=16, spp=64, **kw):
    make, mesh = SCENES[name]
    dev, host = make("cuda", res, spp, **kw), make("cpu", res, spp, **kw)
    assert dev.attach_vertex_color(mesh) == 0 and host.attach_vertex_color(mesh) == 0
    return dev, host


def _replay(sc, seed, spp, depth, adj, lo=0, hi=None):
    """Both texel passes over the paths [lo, hi) of sensor 0, by default all of them: (colour gradients per slot, d radiance for
    the tangent cos(0.37 x element index), the radiance)."""
    hi = sc.sensors[0].wavefront_size(spp) if hi is None else hi
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, lo, hi)
    radiance = radiance.contiguous()
    shapes = [sc._texture_shape(k) for k in range(len(sc.texture_slots))]          # (V_mesh, 1, 3)
    grads = [torch.zeros(s, device=sc.device) for s in shapes]
    sc.trace_texture_backward(0, seed, spp, depth, lo, hi, radiance, adj.to(sc.device), grads)
    tans = [torch.from_numpy(np.cos(np.arange(int(np.prod(s)), dtype=np.float32) * 0.37).reshape(s)).to(sc.device) for s in shapes]
    d_rad = sc.trace_texture_forward(0, seed, spp, depth, lo, hi, radiance, tans)
    return [g.cpu() for g in grads], d_rad.cpu(), radiance.cpu()


def _check(dev, host, seed, spp, depth, adj, lo=0, hi=None, what=""):
    """test_gpu_texture_adjoint.py's bounds for this kernel: radiance 1e-3, gradients and forward 2e-3 of the L1 norm."""
    gd, fd_, rd = _replay(dev, seed, spp, depth, adj, lo, hi)
    gh, fh, rh = _replay(host, seed, spp, depth, adj, lo, hi)
    print(f"{what}: radiance gap {float((rd - rh).abs().sum()) / float(rh.abs().sum()):.3e}, backward gaps "
          f"{[float((a - b).abs().sum()) / float(b.abs().sum()) for a, b in zip(gd, gh)]}, forward gap "
          f"{float((fd_ - fh).abs().sum()) / float(fh.abs().sum()):.3e}")
    assert float((rd - rh).abs().sum()) <= 1e-3 * float(rh.abs().sum())
    for a, b in zip(gd, gh):
        assert float(b.abs().sum()) > 0
        assert float((a - b).abs().sum()) <= 2e-3 * float(b.abs().sum()), (float((a - b).abs().sum()), float(b.abs().sum()))
    assert float(fh.abs().sum()) > 0
    assert float((fd_ - fh).abs().sum()) <= 2e-3 * float(fh.abs().sum())


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("depth", [2, 4])
def test_device_passes_match_the_host_twin(name, depth):
    """A, B and B with the ball turned by 10 degrees, under the texel kernel's bounds.

    B is the case that needs surface_interaction's geometric normal formed without a fused multiply-add (cross_rounded,
    epsm_trace_core.h): eight of the ball's 80 triangles have a normal whose z is exactly zero, coordinate_system() branches on its
    sign, and with one fma in the cross product the device's shading frames on those triangles were turned about the normal
    against the host's -- 94 (depth 2) and 178 (depth 4) of the 25 600 paths took other sample directions: radiance gap 1.563e-3 /
    1.205e-3, backward 7.45e-2 / 3.83e-2, forward 1.26e-2 / 7.36e-3, with per-vertex colours and with a constant `rgb` alike.  With
    the rounded products: 7.5e-8 / 8.2e-8, 1.7e-6 / 2.5e-6, 9.5e-7 / 1.1e-6.  The turned ball has no such triangle."""
    spp, seed = 64, 11
    dev, host = _pair(name, spp=spp)
    n = dev.sensors[0].wavefront_size(spp)
    adj = torch.randn((n, 3), generator=torch.Generator().manual_seed(depth))
    _check(dev, host, seed, spp, depth, adj, what=f"{name} depth {depth}")


@pytest.mark.parametrize("res,spp,lo,hi", [(5, 5, 0, 125), (9, 3, 0, 243), (16, 8, 100, 1001)])
def test_ragged_path_counts(res, spp, lo, hi):
    """The count shapes of test_gpu_texture_adjoint.py: 125 paths, less than one workgroup; 243, a workgroup and a ragged second; a
    tile that starts at path 100 -- inside a wave of the full launch -- and ends at 1001."""
    dev, host = _pair("A", res, spp)
    assert dev.sensors[0].wavefront_size(spp) >= hi and (lo == 0 or lo % 64 != 0)
    adj = torch.randn((hi - lo, 3), generator=torch.Generator().manual_seed(3 + lo))
    _check(dev, host, 7, spp, 3, adj, lo, hi, what=f"{res}x{res} @ {spp} [{lo}, {hi})")


def test_merge_sees_shared_footprints():
    """A 2-triangle floor filling the frame: every sample of a pixel -- the 64 lanes of a wave -- lies in one of two triangles, and
    the per-vertex sums are those of ~N items each (no add lost), as test_gpu_texture_adjoint.test_merge_sees_shared_footprints."""
    spp, seed, res = 64, 3, 32
    cam = sensor([0.3, 0.2, 2.0], [0.3, 0.2, 0.0], up=(0, 1, 0), res=res, spp=spp, rfilter="gaussian")      # (below the light, looking down)
    dev, host = _pair("A", res, spp, n=2, cam=cam)
    n = dev.sensors[0].wavefront_size(spp)
    adj = torch.ones((n, 3))
    gd, _, _ = _replay(dev, seed, spp, 2, adj)
    gh, _, _ = _replay(host, seed, spp, 2, adj)
    assert float(gh[0].abs().min()) > 0                              # all four vertices
    torch.testing.assert_close(gd[0], gh[0], rtol=1e-3, atol=1e-3 * float(gh[0].abs().max()))


def test_merge_keeps_distinct_footprints_apart():
    """A 65 x 65 vertex grid: a pixel's samples straddle triangles that share vertices but not footprints.  Lanes merged by
    anything less than the triangle -- a vertex row, say -- would add one lane's weights to another's rows."""
    spp, seed = 64, 3
    dev, host = _pair("A", 16, spp, n=65)
    n = dev.sensors[0].wavefront_size(spp)
    adj = torch.ones((n, 3))
    gd, _, _ = _replay(dev, seed, spp, 2, adj)
    gh, _, _ = _replay(host, seed, spp, 2, adj)
    assert int((gh[0].abs().sum(dim=(1, 2)) > 0).sum()) > 1000       # (most of the 4225 vertices are reached)
    torch.testing.assert_close(gd[0], gh[0], rtol=1e-3, atol=1e-3 * float(gh[0].abs().max()))
    _check(dev, host, seed, spp, 3, torch.randn((n, 3), generator=torch.Generator().manual_seed(1)), what="65 x 65 grid")


def test_both_tracer_forms_render_the_ball():
    """Both forms go through path_bounce: one against the other on scene B within the bound of
    test_gpu_environment.test_device_image_and_log_equal_the_host_build (a bitmap-lit scene in both forms): fewer than 3 % of the
    pixels off by more than 1e-3 (1 + |value|) -- and each against the host build, on B and on the turned ball."""
    res, spp = 16, 8
    close = lambda a, b: float(((a - b).abs() > 1e-3 * (1 + a.abs())).float().mean())
    for tilt in (0.0, 10.0):
        dev = scene_b("cuda", res, spp, tilt=tilt)
        imgs = {}
        for tracer in ("mega", "wavefront"):
            dev.tracer = tracer
            imgs[tracer] = dev.render_primal(sensor=0, seed=4, spp=spp, max_depth=4).cpu()
        a, b = imgs["mega"], imgs["wavefront"]
        print(f"tilt {tilt}: pixels off between the forms {close(a, b):.4f}")
        assert float(a.abs().sum()) > 0
        assert close(a, b) < 0.03
        host = scene_b("cpu", res, spp, tilt=tilt).render_primal(sensor=0, seed=4, spp=spp, max_depth=4)
        print(f"          against the host: mega {close(host, a):.4f}, wavefront {close(host, b):.4f}")
        assert close(host, a) < 0.03 and close(host, b) < 0.03
    # the colours are seen in both: a grey ball renders another image
    grey = scene_b("cuda", res, spp, colours=np.full((42, 3), 0.5, np.float32), tracer="wavefront", tilt=10.0)
    assert float((grey.render_primal(sensor=0, seed=4, spp=spp, max_depth=4).cpu() - b).abs().max()) > 1e-2


@pytest.mark.parametrize("name", ["scene_a_with_colour_slot", "prb_reparam_plane"])
def test_device_forward_is_the_transpose_of_the_device_backward(name):
    if name == "prb_reparam_plane":
        sc, integ_name = vertex_plane(0.0, 16, 16, device="cuda"), "prb_reparam"
        sc.attach("plane"); sc.attach_vertex_color("plane")
    else:
        sc, integ_name = scene_a("cuda"), "prb"
        sc.attach_color("wall.bsdf"); sc.attach_vertex_color("floor"); sc.attach_radiance("light")
    integ = epsm.load_dict({"type": integ_name, "max_depth": 3})
    gap, S_, a = transpose_gap(integ, sc, 5, sc.sensors[0].spp, torch.Generator().manual_seed(2))
    assert S_ > 0 and abs(a) > 0
    assert gap <= 2e-3 * S_, (gap, S_)


def test_vertex_albedo_experiment_lowers_the_colour_error():
    """The bar of test_texture_experiment_lowers_the_texel_error for the same problem in bitmap form: a third of the start."""
    hist, opt = optim.run("prb", "vertex_albedo", iterations=40, log=lambda s: None)
    print("history:", [round(h, 4) for h in hist])
    assert hist[-1] < hist[0] / 3, hist
