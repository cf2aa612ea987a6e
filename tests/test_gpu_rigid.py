"""The rigid-motion kernels on the GPU (csrc/epsm_trace_rigid.hip): epsm_rigid_reduce and epsm_rigid_expand against their float64
torch forms, the transpose pair, the device passes against the host build of the tracer, the device transpose identity and the
recovery of the camera's angle by exp/camera_pose.py."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _reparam_scenes import CONFIGS
from epsm_mitsuba3_amd import rigid
from test_rigid import pose_scene, pose_transpose_gap

pytestmark = pytest.mark.gpu

# slots of 1, 63, 64, 65, 1024, 1025 and 3 * 1024 + 7 vertices back to back -- boundaries inside a wave, at a chunk and across
# several chunks -- an empty slot and two that overlap each other and the others
SIZES = [1, 63, 64, 65, 1024, 1025, 3 * 1024 + 7]
V = sum(SIZES) + 79                                        # 5400: the tail belongs to no back-to-back slot
U = 2.0 ** -24                                             # float32 unit roundoff
SLACK = 1.0 + 1e-4                                         # 5400 float64 adds at 2^-53 each, twice: 1e-12 of sum |terms|, far inside


def _slots():
    r, lo = [], 0
    for n in SIZES:
        r.append([lo, lo + n]); lo += n
    r += [[700, 700], [10, 2000], [1500, V - 40]]              # (the last 40 vertices lie in no slot at all)
    return torch.tensor(r, dtype=torch.int64)


@pytest.fixture(scope="module")
def rows():
    gen = torch.Generator().manual_seed(17)
    ranges = _slots()
    n = ranges.shape[0]
    d = dict(ranges=ranges, pivots=torch.randn((n, 3), generator=gen), positions=2.0 * torch.randn((V, 3), generator=gen),
             normals=torch.nn.functional.normalize(torch.randn((V, 3), generator=gen), dim=1),
             g_pos=torch.randn((V, 3), generator=gen), g_nrm=torch.randn((V, 3), generator=gen),
             twists=torch.randn((n, 6), generator=gen), start=torch.randn((n, 6), generator=gen))
    d["cuda"] = {k: v.cuda() for k, v in d.items()}
    # sum |terms| of every output of the reduce, (n, 6) float64: what the rounding bounds are relative to
    acr = lambda a, b: torch.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
    terms = torch.zeros((n, 6), dtype=torch.float64)
    for s, (lo, hi) in enumerate(ranges.tolist()):
        g, h = d["g_pos"][lo:hi].double().abs(), d["g_nrm"][lo:hi].double().abs()
        terms[s, :3] = g.sum(0)
        terms[s, 3:] = acr((d["positions"][lo:hi].double() - d["pivots"][s].double()).abs(), g).sum(0) + acr(d["normals"][lo:hi].double().abs(), h).sum(0)
    d["terms"] = terms
    d["want"] = rigid.reduce_torch(d["positions"], d["normals"], d["g_pos"], d["g_nrm"], ranges, d["pivots"])
    return d


def _reduce(c, out, normals=True):
    rigid.reduce(c["positions"], c["normals"], c["g_pos"], c["g_nrm"] if normals else None, c["ranges"], c["pivots"], out)
    torch.cuda.synchronize()
    return out


def test_reduce_equals_float64_torch_adds_to_its_output_and_repeats_bit_for_bit(rows):
    """The kernel sums in float64 (every product of two float32 numbers is exact in it; the sums carry 2^-53 per add, nothing at
    these counts) and rounds twice on the way out: the sum S to float32, u |S|, and the add out + S, u |out + S|, u = 2^-24.  Both
    are below u (2 sum |terms| + |out|): the bound, per number (SLACK covers the float64 adds of the kernel and of the reference)."""
    c = rows["cuda"]
    got = _reduce(c, c["start"].clone()).cpu().double()
    want = rows["start"].double() + rows["want"]
    bound = SLACK * U * (2 * rows["terms"] + rows["start"].double().abs())
    assert torch.all((got - want).abs() <= bound), ((got - want).abs() / bound).max()
    assert torch.equal(got[7], rows["start"][7].double())                                    # the empty slot adds nothing
    assert torch.equal(_reduce(c, c["start"].clone()).cpu().double(), got)                    # two calls: the same bits
    zero = _reduce(c, torch.zeros_like(c["start"])).cpu()
    assert torch.equal(_reduce(c, torch.zeros_like(c["start"])).cpu(), zero)
    assert torch.all((zero.double() - rows["want"]).abs() <= SLACK * U * rows["terms"])       # from zero: the one rounding of S
    # without the normal rows: the torque of the positions alone
    no_n = _reduce(c, torch.zeros_like(c["start"]), normals=False).cpu().double()
    want_n = rigid.reduce_torch(rows["positions"], rows["normals"], rows["g_pos"], None, rows["ranges"], rows["pivots"])
    assert torch.all((no_n - want_n).abs() <= SLACK * U * rows["terms"])
    assert float((no_n - zero.double())[:, 3:].abs().max()) > 1.0 and torch.equal(no_n[:, :3], zero.double()[:, :3])


def _expand_terms(rows):
    """sum |terms| of every output of the expand, (V, 3) float64 each."""
    acr = lambda a, b: torch.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
    tp, tn = torch.zeros((V, 3), dtype=torch.float64), torch.zeros((V, 3), dtype=torch.float64)
    for s, (lo, hi) in enumerate(rows["ranges"].tolist()):
        t, w = rows["twists"][s, :3].double().abs(), rows["twists"][s, 3:].double().abs().expand(hi - lo, 3)
        x, c = rows["positions"][lo:hi].double().abs(), rows["pivots"][s].double().abs()
        tp[lo:hi] += t + acr(w, x + c)
        tn[lo:hi] += acr(w, rows["normals"][lo:hi].double().abs())
    return tp, tn


def test_expand_equals_torch_and_adds_to_its_output(rows):
    """float32 arithmetic.  Per slot term four roundings, each u of that slot's |terms|: the difference x - c, the product, the
    difference of the two products of a cross component, the add to dt.  A vertex lies in at most three of these slots: three adds
    over the slots, each u of a partial sum; and the add into the output, u (sum |terms| + |d|).  Together 8 u (sum |terms| + |d|)."""
    c = rows["cuda"]
    gen = torch.Generator().manual_seed(5)
    d0p, d0n = torch.randn((V, 3), generator=gen), torch.randn((V, 3), generator=gen)
    dp, dn = d0p.cuda(), d0n.cuda()
    rigid.expand(c["positions"], c["normals"], c["ranges"], c["pivots"], c["twists"], dp, dn)
    torch.cuda.synchronize()
    wp, wn = rigid.expand_torch(rows["positions"], rows["normals"], rows["ranges"], rows["pivots"], rows["twists"])
    tp, tn = _expand_terms(rows)
    assert torch.all((dp.cpu().double() - (d0p.double() + wp)).abs() <= 8 * U * (tp + d0p.double().abs()))
    assert torch.all((dn.cpu().double() - (d0n.double() + wn)).abs() <= 8 * U * (tn + d0n.double().abs()))
    covered = torch.zeros(V, dtype=torch.bool)
    for lo, hi in rows["ranges"].tolist():
        covered[lo:hi] = True
    assert not bool(covered.all()) and torch.equal(dp.cpu()[~covered], d0p[~covered])           # vertices in no slot are not written
    only = d0p.cuda()
    rigid.expand(c["positions"], None, c["ranges"], c["pivots"], c["twists"], only, None)          # positions alone
    assert torch.equal(only, dp)


def test_reduce_and_expand_are_a_transpose_pair(rows):
    """<reduce(g), tau> = <g, expand(tau)> to float32 rounding: both sides are sums of the same products |tau_k| |term|, the left
    rounded once per output (u), the right at most eight times per slot term (above): 9 u sum |tau| |terms|."""
    c = rows["cuda"]
    F = _reduce(c, torch.zeros_like(c["start"])).cpu().double()
    dp, dn = torch.zeros((V, 3), device="cuda"), torch.zeros((V, 3), device="cuda")
    rigid.expand(c["positions"], c["normals"], c["ranges"], c["pivots"], c["twists"], dp, dn)
    lhs = float((F * rows["twists"].double()).sum())
    rhs = float((dp.cpu().double() * rows["g_pos"].double()).sum() + (dn.cpu().double() * rows["g_nrm"].double()).sum())
    S = float((rows["terms"] * rows["twists"].double().abs()).sum())
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= 9 * U * S, (lhs, rhs, S)


def test_invalid_arguments_are_refused_on_the_host(rows):
    import ctypes as C
    from epsm_mitsuba3_amd import _lib
    c, lib = rows["cuda"], _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    out, ws = torch.zeros((10, 6), device="cuda"), torch.zeros(64, device="cuda", dtype=torch.uint8)
    args = [p(c["positions"]), p(c["normals"]), p(c["g_pos"]), p(c["g_nrm"]), V, p(c["ranges"]), p(c["pivots"]), 10, p(out)]
    assert lib.epsm_rigid_workspace_bytes(V, 10) == 48 * 10 * 6 and lib.epsm_rigid_workspace_bytes(1025, 1) == 96
    assert lib.epsm_rigid_reduce(*args, p(ws), 64, None) == -22 and b"workspace" in lib.epsm_last_error()
    assert lib.epsm_rigid_reduce(*args[:5], None, *args[6:], p(ws), 64, None) == -22 and b"ranges" in lib.epsm_last_error()
    assert lib.epsm_rigid_reduce(*args[:7], 70000, p(out), p(ws), 64, None) == -22 and b"n_slots" in lib.epsm_last_error()
    assert lib.epsm_rigid_expand(p(c["positions"]), None, V, p(c["ranges"]), p(c["pivots"]), p(c["twists"]), 10, p(out), p(out), None) == -22
    assert lib.epsm_rigid_expand(p(c["positions"]), None, V, p(c["ranges"]), p(c["pivots"]), None, 10, p(out), None, None) == -22
    assert lib.epsm_rigid_reduce(*args[:4], 1 << 30, *args[5:7], 10, p(out), p(ws), 64, None) == -22 and b"2^23" in lib.epsm_last_error()
    with pytest.raises(ValueError, match="lives on cpu"):                                         # a host pointer never reaches a kernel
        rigid.reduce(c["positions"], c["normals"], c["g_pos"], c["g_nrm"], rows["ranges"], c["pivots"], torch.zeros((10, 6), device="cuda"))
    with pytest.raises(ValueError, match="lives on cpu"):
        rigid.expand(c["positions"], c["normals"], c["ranges"], c["pivots"], rows["twists"], torch.zeros((V, 3), device="cuda"), None)
    assert lib.epsm_rigid_reduce(*args[:7], 0, None, None, 0, None) == 0                           # nothing to do is not an error
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# -- the passes ---------------------------------------------------------------------------------------------------------------
def test_device_pose_gradients_equal_the_host_build():
    """`cam_rotation`, `cam_origin` and a mesh's twist under prb_reparam on the smallest reparam config (translate_camera, 16 x 16
    film) against the host build under the same seed, at the agreement bound of
    tests/test_gpu_reparam.py::test_device_pass_equals_the_host_build: 2e-2 of the largest entry, per entry."""
    name, res, spp = "translate_camera", 16, 32
    cfg = CONFIGS[name]
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": 16, "reparam_kappa": cfg.get("kappa", 1e5)})
    g = torch.ones((res, res, 3)) * (0.5 + torch.arange(res, dtype=torch.float32) / res)[None, :, None]
    out = []
    for dev in ("cpu", "cuda"):
        sc = pose_scene(name, res, spp, dev, rotation=True)
        sc.attach_rigid("sphere", pivot=[0.3, -0.2, 0.5])
        p = sc.param_grads()
        integ.render_backward(sc, p, g.to(sc.device), sensor=0, seed=5, spp=spp)
        out.append([x.cpu().clone() for x in (p.cam_rotation, p.cam_origin, p.rigid[0])])
    for a, b, what in zip(out[0], out[1], ("cam_rotation", "cam_origin", "rigid")):
        scale = float(a.abs().max())
        print(what, a.tolist(), b.tolist())
        assert scale > 0, what
        assert float((a - b).abs().max()) <= 2e-2 * scale, (what, a, b)


@pytest.mark.parametrize("name,rigid_meshes,rotation", [("translate_camera_lit", ("sphere", "floor"), True),
                                                         ("translate_camera", ("sphere",), True),
                                                         ("diffuse_sphere_area_light", ("sphere",), None)])
def test_device_forward_is_the_transpose_of_the_device_backward_pass(name, rigid_meshes, rotation):
    """The bound tests/test_gpu_render_forward.py uses on the device: 2e-3 of the sum of the absolute terms."""
    cfg = CONFIGS[name]
    sc = pose_scene(name, 16, 8, "cuda", rigid_meshes=rigid_meshes, rotation=rotation)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": cfg["max_depth"], "reparam_rays": 16, "reparam_kappa": cfg.get("kappa", 1e5)})
    gap, S, big, new = pose_transpose_gap(integ, sc, 7, 8, torch.Generator().manual_seed(31))
    assert big > 0 and S > 0 and new > 0
    assert gap <= 2e-3 * S, (gap, S)


@pytest.mark.parametrize("kind", ["manifold", "manifold_caustic"])
def test_rigid_twists_under_the_manifold_integrators_repeat_the_reduce_of_their_rows(kind):
    """The 5-channel branch on the device (the scene of exp/camera.py, every mesh a rigid slot): `rigid` is the reduce of this
    call's `pos` / `nrm` contribution, to the float32 rounding of the kernel's output."""
    from epsm_mitsuba3_amd.exp import camera
    sc = camera.load_scene("cuda")
    slots = {m.name: sc.attach_rigid(m.name) for m in sc.meshes}
    integ = epsm.load_dict({"type": kind, "max_depth": camera.max_depth})
    g = 1e-3 * torch.randn((camera.resolution, camera.resolution, 5), generator=torch.Generator().manual_seed(1)).cuda()
    p = sc.param_grads()
    integ.render_backward(sc, p, g, seed=2)
    assert float(p.pos.abs().max()) > 0 and float(p.rigid.abs().max()) > 0
    ranges, pivots = sc.rigid_tables()
    want = rigid.reduce_torch(sc.positions.cpu(), sc.normals.cpu(), p.pos.cpu(), p.nrm.cpu(), ranges.cpu(), pivots.cpu())
    for name, slot in slots.items():
        assert torch.allclose(p.rigid[slot].cpu().double(), want[slot], rtol=1e-5, atol=1e-6 * float(want.abs().max())), name


def test_the_camera_angle_is_recovered():
    """exp/camera_pose.py -- bedroom's one angle about the sensors' local y axis -- under prb_reparam, 100 Adam steps from 10
    degrees: the angle error ends below where it started, at what the device measured plus 5 % (MEASUREMENTS.md 16.2: the run ends
    at 0.00633 of the start, twice, which is also the largest of its last ten iterations; the host build ends at 0.0064)."""
    from epsm_mitsuba3_amd.exp import camera_pose
    from epsm_mitsuba3_amd.optim import run
    hist, opt = run("prb_reparam", "camera_pose", log=lambda s: None)
    print("camera_pose: start", hist[0], "end", hist[-1], "min of the last 10", min(hist[-10:]), "max of the last 10", max(hist[-10:]))
    assert abs(hist[0] - camera_pose._START) < 1e-6
    assert hist[-1] < hist[0], hist[::10]
    assert max(hist[-10:]) < CAMERA_POSE_END * 1.05 * hist[0], hist[::10]


CAMERA_POSE_END = 0.00633       # measured: max of the last ten iterations / start
