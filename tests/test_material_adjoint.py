"""The conductor material adjoint of the colour pass (Scene.attach_conductor with prb / prb_reparam / a 3-channel gradient image;
epsm_trace_paths_material_backward / _forward) on the host build of the tracer (tests/host_harness/trace_material_host.cpp): the
closed forms of d F / d eta and d F / d k against float64 autograd of the formula, the transpose identity, EXACT finite differences
of the rendered image (sampling does not depend on eta, k or the tint), and the bookkeeping.  The GPU twin is
tests/test_gpu_material_adjoint.py."""
import ctypes as C
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _material_host import host_material_tracer, on_host_material
from _scenes import quad, sensor
from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd.params import ParamGrads

PROBE_FRESNEL_CONDUCTOR_GRAD = 13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the closed forms: fresnel_conductor (fresnel.h:92-117) restated in float64 torch and differentiated by autograd
# ---------------------------------------------------------------------------------------------------------------------
def fresnel_conductor64(cos_i, eta, k):
    c2 = cos_i * cos_i
    s2 = 1.0 - c2
    s4 = s2 * s2
    t1 = eta * eta - k * k - s2
    p = torch.sqrt(t1 * t1 + 4.0 * k * k * eta * eta)
    a = torch.sqrt(0.5 * (p + t1))
    term_1, term_2 = p + c2, 2.0 * cos_i * a
    r_s = (term_1 - term_2) / (term_1 + term_2)
    term_3, term_4 = p * c2 + s4, term_2 * s2
    r_p = r_s * (term_3 - term_4) / (term_3 + term_4)
    return 0.5 * (r_s + r_p)


def fresnel_grid():
    """cos in linspace(0.02, 1, 50) x eta in {0.05 ... 4} x k in {0.1 ... 7}: 2400 rows of (cos, eta, k), none excluded."""
    cos = np.linspace(0.02, 1.0, 50)
    eta = np.array([0.05, 0.14, 0.2, 0.5, 1.0, 1.5, 2.5, 4.0])
    k = np.array([0.1, 0.5, 1.0, 2.0, 3.98, 7.0])
    g = np.stack(np.meshgrid(cos, eta, k, indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def fresnel_reference(rows):
    """(F, d F / d eta, d F / d k) in float64 on the float32 numbers the probe saw."""
    x = torch.tensor(rows.astype(np.float64))
    eta, k = x[:, 1].clone().requires_grad_(True), x[:, 2].clone().requires_grad_(True)
    F = fresnel_conductor64(x[:, 0], eta, k)
    de, dk = torch.autograd.grad(F.sum(), [eta, k])
    return F.detach().numpy(), de.numpy(), dk.numpy()


# the asserted bounds: 4 x the worst absolute error the host build shows on the grid (measured: d F / d eta 6.68e-07 against a
# largest value of 3.256, d F / d k 6.58e-07 against 2.687 -- 2e-07 of their scale, where float32 autograd of the naive formula
# reaches 4e-05), far under the hard cap of 1e-3 of the largest value
FRESNEL_BOUND = {"eta": 4 * 6.68e-07, "k": 4 * 6.58e-07}


def check_fresnel_probe(probe):
    """The assertions of the closed-form test for `probe(rows) -> (n,16)`: the host harness here, the device in the GPU twin."""
    rows = fresnel_grid()
    out = probe(rows)
    F, de, dk = fresnel_reference(rows)
    assert len(rows) == 50 * 8 * 6
    print(f"F: worst relative error {float(np.max(np.abs(out[:, 0] - F) / F)):.3e}")
    for name, got, want in (("eta", out[:, 1], de), ("k", out[:, 2], dk)):
        err, scale = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
        print(f"d F / d {name}: worst abs error {err:.3e}, largest value {scale:.3f}, ratio {err / scale:.3e} (bound {FRESNEL_BOUND[name]:.3e})")
        assert FRESNEL_BOUND[name] <= 1e-3 * scale                      # the hard cap is a condition on the bound itself
        assert err <= FRESNEL_BOUND[name], (name, err)
    # the `eta = 0, k = 1` mirror: F = 1 and derivatives exactly 0 (autograd of the formula gives NaN there)
    mirror = np.stack([np.linspace(0.02, 1.0, 50), np.zeros(50), np.ones(50)], -1).astype(np.float32)
    m = probe(mirror)
    assert np.all(m[:, 0] == 1.0) and np.all(m[:, 1] == 0.0) and np.all(m[:, 2] == 0.0)
    x = torch.tensor([0.0, 1.0], dtype=torch.float64, requires_grad=True)
    fresnel_conductor64(torch.tensor(0.5, dtype=torch.float64), x[0], x[1]).backward()
    assert bool(torch.isnan(x.grad).any())


def _host_probe(rows, what=PROBE_FRESNEL_CONDUCTOR_GRAD):
    lib = host_material_tracer()
    lib.epsm_probe.restype = C.c_int
    inp = np.zeros((rows.shape[0], 8), np.float32)
    inp[:, : rows.shape[1]] = rows
    out = np.zeros((rows.shape[0], 16), np.float32)
    assert lib.epsm_probe(C.c_int(what), C.c_int64(rows.shape[0]), inp.ctypes.data_as(C.c_void_p),
                          out.ctypes.data_as(C.c_void_p), None, None) == 0
    return out


def test_fresnel_derivatives_match_float64_autograd():
    """d F / d eta and d F / d k through the host probe against autograd of the float64 restatement on the whole grid, no point
    excluded; the bound is 4 x the worst error measured on the host build (FRESNEL_BOUND: 6.68e-07 and 6.58e-07 absolute), itself
    under the cap of 1e-3 of the largest derivative (3.256 and 2.687).  The F it returns is fresnel_conductor's, bit for bit."""
    check_fresnel_probe(_host_probe)
    rows = fresnel_grid()
    assert np.array_equal(_host_probe(rows)[:, 0], _host_probe(rows, what=6)[:, 0])        # EPSM_PROBE_FRESNEL_CONDUCTOR


def test_header_and_python_agree():
    text = open(os.path.join(ROOT, "include", "epsm_trace.h")).read()
    for name in ("epsm_trace_paths_material_backward", "epsm_trace_paths_material_forward", "epsm_trace_material_workspace_bytes",
                 f"EPSM_MAX_MATERIAL_GRADS {S.MAX_MATERIAL_GRADS}", "EPSM_PROBE_FRESNEL_CONDUCTOR_GRAD = 13", "EPSM_PROBE_COUNT = 16"):
        assert name in text, name
    assert S.MAX_MATERIAL_GRADS == 4 and C.sizeof(S.EpsmBsdf) == 80
    from epsm_mitsuba3_amd import _lib
    lib = _lib.lib()
    assert lib.epsm_abi_version() == _lib.ABI_VERSION == 7
    assert lib.epsm_trace_material_workspace_bytes(C.c_int64(0)) == 0
    assert lib.epsm_trace_material_workspace_bytes(C.c_int64(129)) == 2 * 9 * 4 * 4     # one row of 9 x 4 floats per 128 paths


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def two_metal_scene(device="cpu", res=12, spp=32):
    """The two-plate scene of test_alpha_adjoint.py with one plate a `conductor` (a copper mirror) and one a twosided
    `roughconductor`, over a diffuse floor under an area light and a constant sky."""
    pv, pf = quad(0.3, 0.9, up=True)
    qv = pv + np.array([1.2, 0.6, 0.4]); pv = pv + np.array([-0.7, 0.0, 0.0])
    fv, ff = quad(0.0, 4.0, up=True)
    lv, lf = quad(3.0, 0.6, up=False)
    ggx = {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": 0.25,
           "specular_reflectance": {"type": "rgb", "value": [0.9, 0.8, 0.7]}}
    d = {"type": "scene", "cam": sensor([0.0, -3.5, 2.5], [0.2, 0.2, 0.3], up=(0, 0, 1), res=res, spp=spp, rfilter="gaussian"),
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "face_normals": True,
                   "bsdf": {"type": "conductor", "material": "Cu"}},
         "plate2": {"type": "mesh", "vertices": qv, "faces": pf, "face_normals": True, "bsdf": {"type": "twosided", "bsdf": ggx}},
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.4, 0.3]}}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [12.0, 10.0, 8.0]}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.4}}}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_material(sc)
    sc.tracer = "mega"
    return sc


def attach_two(sc):
    return [sc.attach_conductor("plate.bsdf"), sc.attach_conductor("plate2.bsdf")]


def transpose_gap(integ, sc, seed, spp, gen, geometry=True):
    """(|a - b|, S, a, params): a = sum g * J t, b = sum J^T g * t, S = sum |g * J t| + sum |J^T g * t|."""
    s = sc.sensors[0]
    t = sc.param_grads()
    t.conductor[:] = torch.randn(tuple(t.conductor.shape), generator=gen).to(sc.device)
    if geometry:
        for m in sc.meshes:
            if getattr(m, "pos_attached", False):
                lo, hi = t.mesh_slices[m.name]
                t.pos[lo:hi] = torch.randn((hi - lo, 3), generator=gen).to(sc.device)
    g = torch.randn((s.height, s.width, 3), generator=gen).to(sc.device)
    fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp)
    params = sc.param_grads()
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    a = float((g * fwd).double().sum())
    b = float((params.flat * t.flat).double().sum())
    S_ = float((g * fwd).abs().double().sum()) + float((params.flat * t.flat).abs().double().sum())
    return abs(a - b), S_, a, params


TRANSPOSE = {"prb": lambda sc: attach_two(sc),
             "prb_reparam": lambda sc: attach_two(sc) + [sc.attach("plate2")],
             "manifold": lambda sc: attach_two(sc)}


@pytest.mark.parametrize("integ_name", list(TRANSPOSE))
@pytest.mark.parametrize("depth", [2, 4])
def test_forward_is_the_transpose_of_backward(integ_name, depth):
    sc = two_metal_scene()
    TRANSPOSE[integ_name](sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params = transpose_gap(integ, sc, seed=5, spp=32, gen=torch.Generator().manual_seed(2 + depth))
    assert float(params.conductor[0].abs().min()) > 0 and float(params.conductor[1].abs().min()) > 0      # all 18 numbers live
    assert S_ > 0 and abs(a) > 0
    print(f"{integ_name} depth {depth}: transpose gap {gap / S_:.3e}")
    assert gap <= 1e-4 * S_, (gap, S_)


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact finite differences of the rendered image
# ---------------------------------------------------------------------------------------------------------------------
def filling_metal(kind, light, res=8, spp=64, device="cpu"):
    """A metal plate that fills the film under an area light or a constant environment; a second, tilted plate of the same BSDF
    stands on it so that paths meet the BSDF more than once."""
    pv, pf = quad(0.0, 3.0, up=True)
    wv = np.array([[-3.0, 1.2, 0.0], [3.0, 1.2, 0.0], [3.0, 2.2, 2.5], [-3.0, 2.2, 2.5]])
    bsdf = {"type": kind, "material": "Cu", "specular_reflectance": {"type": "rgb", "value": [0.9, 0.75, 0.6]}}
    if kind == "roughconductor":
        bsdf.update(distribution="ggx", alpha=0.3)
    d = {"type": "scene", "cam": sensor([0.0, -1.2, 2.0], [0.0, 0.0, 0.0], up=(0, 0, 1), fov=30, res=res, spp=spp, rfilter="gaussian"),
         "metal": bsdf,
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "face_normals": True, "bsdf": {"type": "ref", "id": "metal"}},
         "wall": {"type": "mesh", "vertices": wv, "faces": np.array([[0, 2, 1], [0, 3, 2]]), "face_normals": True,
                  "bsdf": {"type": "ref", "id": "metal"}}}
    if light == "area":
        lv, lf = quad(4.0, 1.5, up=False)
        d["light"] = {"type": "mesh", "vertices": lv + np.array([0.0, 0.5, 0.0]), "faces": lf, "face_normals": True,
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6.0, 5.0, 4.0]}}}
    else:
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [0.8, 1.0, 1.2]}}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_material(sc)
    sc.tracer = "mega"
    return sc


@pytest.mark.parametrize("kind", ["conductor", "roughconductor"])
@pytest.mark.parametrize("light", ["area", "constant"])
def test_forward_equals_finite_differences_of_the_image(kind, light):
    """max_depth 4 < rr_depth 5: no roulette decision, sampling free of the parameters -- render_forward along each of the 9 unit
    tangents against central differences of render at h and h / 2 (h = 2 % of the value), same seed:
    |fwd - FD(h/2)|_1 <= |FD(h) - FD(h/2)|_1 (Richardson's own estimate of FD(h/2)'s error, 3 x it) + 1e-4 |fwd|_1.
    Measured on the host twin, worst of the 9 tangents of each case, relative to |fwd|_1: gap 4.0e-4 ... 4.9e-4, Richardson term
    4.5e-4 ... 5.1e-4, gap / bound at most 0.85 (conductor, area light, eta_r = 0.2: the smallest step).  Both are the float32
    rounding of the renders over 2 h -- they fall as 1 / h up to h = 10 % (MEASUREMENTS.md 21) -- and the host build repeats bit
    for bit."""
    sc = filling_metal(kind, light)
    name = "metal"
    assert name in sc.bsdf_names
    slot = sc.attach_conductor(name)
    integ = epsm.load_dict({"type": "prb", "max_depth": 4})
    assert sc.rr_depth == 5
    seed, spp = 3, 64
    base = sc.conductor_values()[slot].clone()
    keys = ("eta", "k", "specular_reflectance")
    for p in range(3):
        for c in range(3):
            t = sc.param_grads()
            t.conductor[slot, p, c] = 1.0
            fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp).double()
            fds = []
            h = 0.02 * float(base[p, c])
            for step in (h, h / 2):
                out = []
                for sgn in (+1, -1):
                    v = base[p].clone()
                    v[c] += sgn * step
                    sc.set_conductor(name, **{keys[p]: v})
                    out.append(integ.render(sc, sensor=0, seed=seed, spp=spp).double())
                fds.append((out[0] - out[1]) / (2 * step))
            sc.set_conductor(name, **{keys[p]: base[p]})
            gap = float((fwd - fds[1]).abs().sum())
            rich = float((fds[0] - fds[1]).abs().sum())
            scale = float(fwd.abs().sum())
            print(f"{kind} {light} d/d {keys[p]}[{c}]: |fwd - FD(h/2)| {gap:.3e}  |FD(h) - FD(h/2)| {rich:.3e}  |fwd| {scale:.3e}")
            assert scale > 0
            assert float(fwd[..., [j for j in range(3) if j != c]].abs().sum()) == 0       # nothing crosses channels
            assert gap <= rich + 1e-4 * scale, (keys[p], c, gap, rich, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 4. bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def _grad_image(res=12):
    return 0.5 + torch.rand((res, res, 3), generator=torch.Generator().manual_seed(3))


def test_gradients_accumulate_bit_for_bit():
    sc = two_metal_scene()
    attach_two(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = _grad_image()
    p1, p2 = sc.param_grads(), sc.param_grads()
    integ.render_backward(sc, p1, g, sensor=0, seed=4, spp=32)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=32)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=32)
    assert float(p1.conductor.abs().min()) > 0
    assert torch.equal(p2.conductor, 2 * p1.conductor)


def _five_plates():
    pv, pf = quad(0.0, 0.3, up=True)
    d = {"type": "scene", "cam": sensor([0, 0, 6], [0, 0, 0], res=8, spp=4), "sky": {"type": "constant"}}
    for k in range(5):
        d[f"p{k}"] = {"type": "mesh", "vertices": pv + np.array([0.7 * (k % 3 - 1), 0.7 * (k // 3 - 1), 0.0]), "faces": pf,
                      "bsdf": {"type": "roughconductor", "material": "Au", "alpha": 0.1 + 0.02 * k}}
    return on_host_material(S.Scene.from_dict(d, device="cpu"))


def test_fifth_slot_is_refused_by_scene_and_entry_point():
    sc = _five_plates()
    for k in range(4):
        assert sc.attach_conductor(f"p{k}.bsdf") == k
    assert sc.attach_conductor("p2.bsdf") == 2                                              # attached already: its slot
    with pytest.raises(ValueError, match="at most 4"):
        sc.attach_conductor("p4.bsdf")
    assert len(sc.material_slots) == 4
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((8, 8, 3)), seed=1, spp=4)
    assert tuple(p.conductor.shape) == (4, 3, 3) and int((p.conductor.abs().sum(dim=(1, 2)) != 0).sum()) == 4
    # the entry point itself: M = 5 is EPSM_EINVAL, M = 4 is fine
    n = 64
    z = lambda *s: torch.zeros(s, dtype=torch.float32)
    rad, adj, grad, out = z(n, 3), z(n, 3), z(5, 3, 3), z(n, 3)
    lib = sc._backend
    work = z(int(lib.epsm_trace_material_workspace_bytes(C.c_int64(n))) // 4)
    cs = sc.sensors[0].c_struct()
    head = [C.byref(sc.c_scene), C.byref(cs), C.c_uint32(1), 4, 2, 5, C.c_int64(0), C.c_int64(n)]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    bwd = lambda M: lib.epsm_trace_paths_material_backward(*head, ptr(rad), ptr(adj), ptr(grad), M, ptr(work), C.c_size_t(work.numel() * 4), None)
    fwd = lambda M: lib.epsm_trace_paths_material_forward(*head, ptr(rad), ptr(grad), M, ptr(out), None)
    assert bwd(4) == 0 and fwd(4) == 0
    assert bwd(5) == -22 and fwd(5) == -22 and bwd(-1) == -22


def test_wrong_type_and_the_mirror_default_are_refused():
    sc = two_metal_scene()
    with pytest.raises(ValueError, match="neither a conductor nor a roughconductor"):
        sc.attach_conductor("floor.bsdf")
    pv, pf = quad(0.0, 1.0, up=True)
    d = {"type": "scene", "cam": sensor([0, 0, 6], [0, 0, 0], res=8, spp=4), "sky": {"type": "constant"},
         "mirror": {"type": "mesh", "vertices": pv, "faces": pf, "bsdf": {"type": "conductor", "eta": 0.0, "k": 1.0}},
         "black": {"type": "mesh", "vertices": pv + 2.0, "faces": pf,
                   "bsdf": {"type": "conductor", "material": "Cu", "specular_reflectance": {"type": "rgb", "value": [0.5, 0.0, 0.5]}}}}
    sc = on_host_material(S.Scene.from_dict(d, device="cpu"))
    for name in ("mirror.bsdf", "black.bsdf"):
        with pytest.raises(ValueError, match="100 % mirror"):
            sc.attach_conductor(name)
    assert not sc.material_slots


def test_material_alone_counts_as_attached():
    sc = two_metal_scene()
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    sc.attach("plate")
    with pytest.raises(NotImplementedError, match="prb: geometry is attached but no colour parameter is"):
        integ.render_backward(sc, sc.param_grads(), torch.ones((12, 12, 3)), seed=1, spp=4)
    sc.attach_conductor("plate.bsdf")
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((12, 12, 3)), seed=1, spp=4)
    assert float(p.conductor.abs().sum()) > 0
    assert float(p.color.abs().sum()) == 0 and float(p.pos.abs().sum()) == 0 and float(p.nrm.abs().sum()) == 0
    assert float(p.alpha.abs().sum()) == 0
    with pytest.raises(ValueError, match="after attach_conductor"):                         # a buffer laid out before the slot
        integ.render_backward(sc, ParamGrads(sc.V, device="cpu", mesh_slices=sc.mesh_slices), torch.ones((12, 12, 3)), seed=1, spp=4)


def test_set_conductor_is_seen_by_the_next_backward():
    sc, ref = two_metal_scene(), two_metal_scene()
    attach_two(sc); attach_two(ref)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = _grad_image()
    p0 = sc.param_grads()
    integ.render_backward(sc, p0, g, sensor=0, seed=4, spp=32)
    new = dict(eta=[0.3, 0.9, 1.2], k=[3.0, 2.5, 2.2], specular_reflectance=[0.8, 0.9, 1.0])
    sc.set_conductor("plate.bsdf", **new)
    assert torch.equal(sc.conductor_values()[0], torch.tensor([new["eta"], new["k"], new["specular_reflectance"]]))
    p1 = sc.param_grads()
    integ.render_backward(sc, p1, g, sensor=0, seed=4, spp=32)
    b = ref.bsdf_desc[ref.bsdf_names.index("plate.bsdf")]
    b["eta"], b["k"], b["reflectance"] = (np.array(new[x], np.float32) for x in ("eta", "k", "specular_reflectance"))
    ref._upload()
    p2 = ref.param_grads()
    integ.render_backward(ref, p2, g, sensor=0, seed=4, spp=32)
    assert not torch.equal(p0.conductor, p1.conductor)
    assert torch.equal(p1.conductor, p2.conductor)


def test_param_grads_without_conductors_keeps_its_layout():
    old = ParamGrads(10, 2, device="cpu", n_colors=1, tex_shapes=[(2, 3)], n_rigid=1, cam_rotation=True)
    assert old.conductor is None and old.flat.numel() == 60 + 2 + 3 + 3 + 18 + 6 + 3
    new = ParamGrads(10, 2, device="cpu", n_colors=1, tex_shapes=[(2, 3)], n_rigid=1, cam_rotation=True, n_conductors=2)
    assert new.flat.numel() == old.flat.numel() + 18 and tuple(new.conductor.shape) == (2, 3, 3)
    new.flat[:] = torch.arange(new.flat.numel(), dtype=torch.float32)
    assert float(new.conductor[0, 0, 0]) == old.flat.numel() and float(new.cam_rotation[2]) == old.flat.numel() - 1   # at the very end
    for a, b in ((old.pos, new.pos), (old.alpha, new.alpha), (old.color, new.color), (old.texture(0), new.texture(0)),
                 (old.rigid, new.rigid), (old.cam_rotation, new.cam_rotation)):
        assert a.storage_offset() == b.storage_offset() and a.shape == b.shape
    assert tuple(new.scratch().conductor.shape) == (2, 3, 3)
    assert ParamGrads(10, device="cpu").flat.numel() == 63
    sc = two_metal_scene()
    assert sc.param_grads().conductor is None
    attach_two(sc)
    assert tuple(sc.param_grads().conductor.shape) == (2, 3, 3) and tuple(sc.conductor_values().shape) == (2, 3, 3)


def _free_port():
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc = two_metal_scene()
        sc.tile_paths = 1000                                           # several tiles, dealt over the ranks
        attach_two(sc)
        integ = epsm.load_dict({"type": "prb", "max_depth": 3})
        p = sc.param_grads()
        integ.render_backward(sc, p, _grad_image(), sensor=0, seed=4, spp=32)
        q.put((rank, p.flat.clone().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_material_gradients_match_single_process():
    sc = two_metal_scene()
    sc.tile_paths = 1000
    attach_two(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    p = sc.param_grads()
    integ.render_backward(sc, p, _grad_image(), sensor=0, seed=4, spp=32)
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=300) for _ in procs)
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    want = p.flat.numpy()
    assert float(np.abs(want).sum()) > 0
    for r in range(2):
        np.testing.assert_allclose(got[r], want, rtol=1e-4, atol=1e-6 * float(np.abs(want).max()))
