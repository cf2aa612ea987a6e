"""The roughness adjoint of the colour pass (Scene.attach_alpha with prb / prb_reparam / a 3-channel gradient image;
epsm_trace_paths_bsdf_backward / _forward) on the host build of the tracer (tests/host_harness/trace_bsdf_host.cpp): the closed
forms of the microfacet terms' alpha derivatives against a float64 restatement differentiated by autograd, the transpose
identity, finite differences of the rendered image, and the bookkeeping.  The GPU twin is tests/test_gpu_alpha_adjoint.py."""
import ctypes as C
import math
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _bsdf_host import host_bsdf_tracer, on_host_bsdf
from _reparam_scenes import gradient_map
from _scenes import quad, sensor
from epsm_mitsuba3_amd import scene as S

PROBE_BSDF_EVAL, PROBE_MICROFACET_DALPHA, PROBE_BSDF_DALPHA = 10, 11, 12


# ---------------------------------------------------------------------------------------------------------------------
# 1. the closed forms: D, G1 and D G / (4 cos_i) restated in float64 torch (microfacet.h, roughconductor.cpp:302-400)
# ---------------------------------------------------------------------------------------------------------------------
def _D(distr, a, m):
    ct2 = m[:, 2] ** 2
    s = (m[:, 0] ** 2 + m[:, 1] ** 2) / a ** 2
    if distr == "beckmann":
        return torch.exp(-s / ct2) / (math.pi * a ** 2 * ct2 ** 2)
    return 1.0 / (math.pi * a ** 2 * (s + ct2) ** 2)


def _G1(distr, a, v):
    tan2 = a ** 2 * (v[:, 0] ** 2 + v[:, 1] ** 2) / v[:, 2] ** 2
    if distr == "beckmann":
        x = 1.0 / torch.sqrt(tan2)
        fit = (3.535 * x + 2.181 * x * x) / (1.0 + 2.276 * x + 2.577 * x * x)
        return torch.where(x >= 1.6, torch.ones_like(x), fit), x
    return 2.0 / (1.0 + torch.sqrt(1.0 + tan2)), None


def _unit(theta, phi):
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)


def _grid():
    """(alpha, wi, wo): twelve roughnesses over [0.01, 0.5], both directions from near the normal to grazing (89 degrees), six
    azimuth differences from the mirror configuration to nearly back-scattering.  (The derivative's zero crossing -- half-vector
    slope about alpha -- is an excluded boundary and the exclusions may take 2 % of the grid: it is met by the rougher lobes in the
    near-mirror azimuths, about 1 in 9 points at alpha = 0.5, hence the spacing that thins out towards 0.5 and the wide azimuths.)"""
    alphas = np.array([0.01, 0.015, 0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5])
    th = np.radians([1.0, 10.0, 25.0, 40.0, 55.0, 70.0, 80.0, 86.0, 89.0])
    dphi = np.radians([180.0, 170.0, 135.0, 90.0, 60.0, 30.0])
    rows = [(a, ti, to, p) for a in alphas for ti in th for to in th for p in dphi]
    a, ti, to, p = (np.array(x) for x in zip(*rows))
    return a, _unit(ti, np.zeros_like(ti)), _unit(to, p)


def _probe(what, rows, bsdf):
    lib = host_bsdf_tracer()
    lib.epsm_probe.restype = C.c_int
    inp = np.zeros((rows.shape[0], 8), np.float32)
    inp[:, : rows.shape[1]] = rows
    out = np.zeros((rows.shape[0], 16), np.float32)
    assert lib.epsm_probe(C.c_int(what), C.c_int64(rows.shape[0]), inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                          C.byref(bsdf), None) == 0
    return out


def _bsdf_struct(distr, alpha):
    b = S.EpsmBsdf()
    b.type, b.twosided, b.distr, b.sample_visible = S.BSDF_TYPES["roughconductor"], 0, {"beckmann": 0, "ggx": 1}[distr], 0
    b.reflectance[:] = [1.0, 1.0, 1.0]
    b.alpha = float(alpha)
    b.eta[:] = [0.0, 0.0, 0.0]; b.k[:] = [1.0, 1.0, 1.0]           # (Fresnel = 1: the value is D G / (4 cos_i))
    b.int_ior, b.ext_ior, b.alpha_slot, b.color_slot, b.texture = 1.5, 1.0, 0, -1, -1
    return b


@pytest.mark.parametrize("distr", ["beckmann", "ggx"])
def test_microfacet_alpha_derivatives_match_float64_autograd(distr):
    """d/d alpha of D, G1 and of the value D G / (4 cos_i), through the probe, against autograd on the float64 restatement.  The
    bound is 4 x the relative error of the EXISTING float32 value (bsdf_eval_pdf through its probe) on the same points, measured
    here; the error of the derivative is relative to the derivative itself.  Measured on the host twin (max over the kept points of
    the 5832): beckmann value 1.35e-05, derivative 1.32e-05 (bound 5.39e-05), 0.48 % of the grid excluded (all of it the
    derivative's zero crossing), 53.5 % below the 1e-20 cut (value and derivative exactly 0 there); ggx value 7.90e-07, derivative
    2.87e-06 (bound 3.16e-06), 1.56 % excluded (zero crossing), nothing cut."""
    alphas, wi, wo = _grid()
    H = wi + wo
    H /= np.linalg.norm(H, axis=1, keepdims=True)
    value32 = np.zeros(len(alphas)); dvalue32 = np.zeros(len(alphas)); parts32 = np.zeros((len(alphas), 3))
    for a in np.unique(alphas):                                     # (one cfg per alpha)
        sel = alphas == a
        b = _bsdf_struct(distr, a)
        rows = np.concatenate([wi[sel], wo[sel]], 1)
        value32[sel] = _probe(PROBE_BSDF_EVAL, rows, b)[:, 0]
        dvalue32[sel] = _probe(PROBE_BSDF_DALPHA, rows, b)[:, 0]
        o1 = _probe(PROBE_MICROFACET_DALPHA, np.concatenate([H[sel], wi[sel]], 1), b)
        o2 = _probe(PROBE_MICROFACET_DALPHA, np.concatenate([H[sel], wo[sel]], 1), b)
        parts32[sel] = np.stack([o1[:, 0], o1[:, 1], o2[:, 1]], 1)
    # float64 on the float32 inputs the probe saw
    a64 = torch.tensor(alphas.astype(np.float32).astype(np.float64), requires_grad=True)
    twi, two = (torch.tensor(x.astype(np.float32).astype(np.float64)) for x in (wi, wo))
    tH = twi + two
    tH = tH / tH.norm(dim=1, keepdim=True)
    D = _D(distr, a64, tH)
    Gi, xi = _G1(distr, a64, twi)
    Go, xo = _G1(distr, a64, two)
    value = D * Gi * Go / (4.0 * twi[:, 2])
    dvalue, = torch.autograd.grad(value.sum(), a64, retain_graph=True)
    # (the microfacet probe is GIVEN the half vector: its yardstick starts from the same float32 numbers)
    tH32 = torch.tensor(H.astype(np.float32).astype(np.float64))
    dlogs = [torch.autograd.grad(torch.log(t).sum(), a64, retain_graph=True)[0].numpy() for t in (_D(distr, a64, tH32), Gi, Go)]
    value, dvalue, D = value.detach().numpy(), dvalue.numpy(), D.detach().numpy()
    # excluded: within 2 % of a branch boundary -- the fit's a = 1.6, the 1e-20 cut of D cos -- and the derivative's own zero crossing:
    # d value = value x d ln f, and d ln D is the difference of two terms of size up to 2 / alpha (the normalisation's -2 / alpha
    # against the exponent's or the denominator's) that cancel where the lobe's slope equals alpha; a number that passes through
    # zero has no relative error there, so points with |d ln f| below 5 % of 2 / alpha count as on that boundary.  All of it
    # together may take 2 % of the grid.
    near = np.zeros(len(alphas), bool)
    for x in (xi, xo):
        if x is not None:
            near |= np.abs(x.detach().numpy() / 1.6 - 1.0) < 0.02
    dcos = D * tH[:, 2].numpy()
    near |= np.abs(dcos / 1e-20 - 1.0) < 0.02
    cut = dcos <= 1e-20
    assert np.all(value32[cut & ~near] == 0) and np.all(dvalue32[cut & ~near] == 0)      # derivative 0 where the value is cut
    live = ~cut & (value > 1e-30)
    zero = np.zeros(len(alphas), bool)
    zero[live] = np.abs(dvalue[live] / value[live]) < 0.05 * 2.0 / alphas[live]
    zero_D = live & (np.abs(dlogs[0]) < 0.05 * 2.0 / alphas)                                # (the same crossing, of d ln D alone)
    excluded = near | (zero & live)
    print(f"{distr}: excluded {excluded.mean():.2%} of the grid (branch boundaries {near.mean():.2%}, zero crossing of d ln f "
          f"{(zero & live).mean():.2%}); d ln D alone crosses zero on {zero_D.mean():.2%}; below the cut {cut.mean():.2%}")
    assert excluded.mean() <= 0.02, excluded.mean()
    assert (near | zero_D).mean() <= 0.02, (near | zero_D).mean()
    keep = ~excluded & live
    # (a narrow Beckmann lobe is below the cut for most of the grid: alpha = 0.01 keeps 22 of its 486 points; what matters is that
    # every roughness is represented and the maximum is taken over thousands of points)
    assert keep.sum() >= 2000 and min(int(keep[alphas == a].sum()) for a in np.unique(alphas)) >= 10
    err_value = float(np.max(np.abs(value32[keep] - value[keep]) / np.abs(value[keep])))
    err_d = float(np.max(np.abs(dvalue32[keep] - dvalue[keep]) / np.abs(dvalue[keep])))
    keep_D = live & ~near & ~zero_D
    err_parts = [float(np.max(np.abs(parts32[keep_D, 0] - dlogs[0][keep_D]) / np.abs(dlogs[0][keep_D])))]
    for j in (1, 2):                                                 # G1: no crossing; exactly 0 where the value is constant
        nz = live & ~near & (dlogs[j] != 0)
        assert np.all(parts32[live & ~near & (dlogs[j] == 0), j] == 0)
        err_parts.append(float(np.max(np.abs(parts32[nz, j] - dlogs[j][nz]) / np.abs(dlogs[j][nz]))))
    print(f"{distr}: value rel err {err_value:.3e}, derivative rel err {err_d:.3e} (bound {4 * err_value:.3e}), "
          f"d ln D / G1(wi) / G1(wo) rel err {err_parts}")
    assert err_value > 0
    assert err_d <= 4 * err_value, (err_d, err_value)
    assert max(err_parts) <= 4 * err_value, (err_parts, err_value)
    # the a >= 1.6 side of the Beckmann fit is in the grid, and its G1 derivative is exactly 0 there
    if distr == "beckmann":
        flat = (xi.detach().numpy() >= 1.6 * 1.02)
        assert flat.sum() > 100 and np.all(parts32[flat, 1] == 0)


def test_smith_g1_derivative_is_zero_at_normal_incidence():
    b = _bsdf_struct("ggx", 0.3)
    out = _probe(PROBE_MICROFACET_DALPHA, np.array([[0, 0, 1, 0, 0, 1]], np.float32), b)        # xy_alpha_2 == 0
    assert out[0, 1] == 0 and out[0, 3] == 1 and np.isfinite(out[0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def two_plate_scene(device="cpu", res=12, spp=32, twosided=True):
    """Two rough plates (Beckmann and GGX, one of them `twosided`) over a diffuse floor under an area light and a constant sky."""
    pv, pf = quad(0.3, 0.9, up=True)
    qv = pv + np.array([1.2, 0.6, 0.4]); pv = pv + np.array([-0.7, 0.0, 0.0])
    fv, ff = quad(0.0, 4.0, up=True)
    lv, lf = quad(3.0, 0.6, up=False)
    ggx = {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": 0.25}
    d = {"type": "scene", "cam": sensor([0.0, -3.5, 2.5], [0.2, 0.2, 0.3], up=(0, 0, 1), res=res, spp=spp, rfilter="gaussian"),
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "distribution": "beckmann", "alpha": 0.15, "sample_visible": False}},
         "plate2": {"type": "mesh", "vertices": qv, "faces": pf, "face_normals": True,
                    "bsdf": {"type": "twosided", "bsdf": ggx} if twosided else ggx},
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.4, 0.3]}}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [12.0, 10.0, 8.0]}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.4}}}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_bsdf(sc)
    sc.tracer = "mega"
    return sc


def attach_two(sc):
    return [sc.attach_alpha("plate.bsdf"), sc.attach_alpha("plate2.bsdf")]


def transpose_gap(integ, sc, seed, spp, gen, geometry=True):
    """(|a - b|, S, a, params): a = sum g * J t, b = sum J^T g * t, S = sum |g * J t| + sum |J^T g * t|."""
    s = sc.sensors[0]
    t = sc.param_grads()
    t.alpha[:] = torch.randn((t.B,), generator=gen).to(sc.device)
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
    sc = two_plate_scene()
    TRANSPOSE[integ_name](sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params = transpose_gap(integ, sc, seed=5, spp=32, gen=torch.Generator().manual_seed(2 + depth))
    assert float(params.alpha[0]) != 0 and float(params.alpha[1]) != 0
    assert S_ > 0 and abs(a) > 0
    assert gap <= 1e-4 * S_, (gap, S_)


# ---------------------------------------------------------------------------------------------------------------------
# 3 / 4. finite differences of the rendered image
# ---------------------------------------------------------------------------------------------------------------------
def filling_plate(distr, light, sample_visible, res=8, spp=4096, alpha=0.3, device="cpu"):
    """A rough plate that fills the film: no silhouette and no occluder, so that every sample is smooth in alpha."""
    pv, pf = quad(0.0, 3.0, up=True)
    d = {"type": "scene", "cam": sensor([0.0, -1.2, 2.0], [0.0, 0.0, 0.0], up=(0, 0, 1), fov=30, res=res, spp=spp, rfilter="gaussian"),
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "material": "Cu", "distribution": distr, "alpha": alpha,
                            "sample_visible": sample_visible}}}
    if light == "area":
        lv, lf = quad(4.0, 1.5, up=False)
        d["light"] = {"type": "mesh", "vertices": lv + np.array([0.0, 1.5, 0.0]), "faces": lf, "face_normals": True,
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6.0, 5.0, 4.0]}}}
    else:
        d["sky"] = {"type": "envmap", "bitmap": gradient_map(), "to_world": S.rotate([1.0, 0.0, 0.0], 90.0)}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_bsdf(sc)
    sc.tracer = "mega"
    return sc


def image_derivatives(sc, depth, seed, spp, h):
    """(forward-mode derivative image, central finite difference at step h, at step h / 2), same seed."""
    integ = epsm.load_dict({"type": "prb", "max_depth": depth})
    slot = sc.attach_alpha("plate.bsdf")
    t = sc.param_grads()
    t.alpha[slot] = 1.0
    fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp).double().cpu()
    a0 = float(sc.bsdf_desc[sc.bsdf_names.index("plate.bsdf")]["alpha"])
    fds = []
    for step in (h, h / 2):
        out = []
        for sgn in (+1, -1):
            sc.set_alpha("plate.bsdf", a0 + sgn * step)
            out.append(integ.render(sc, sensor=0, seed=seed, spp=spp).double().cpu())
        fds.append((out[0] - out[1]) / (2 * step))
    sc.set_alpha("plate.bsdf", a0)
    return fwd, fds[0], fds[1]


def _stats(img):
    """Per-channel mean of the image and the means of its 4 x 4 blocks."""
    H, W, _ = img.shape
    blocks = img.reshape(H // 4, 4, W // 4, 4, 3).mean(dim=(1, 3)).reshape(-1)
    return torch.cat([img.mean(dim=(0, 1)), blocks])


def _rel(a, b):
    """The reference's error image, |a - b| / max(|b|, floor) (test_ad_integrators.py:862-866, floor 0.2 for images of order 1):
    the floor here is 0.2 of the mean magnitude of b."""
    return (a - b).abs() / b.abs().clamp_min(0.2 * float(b.abs().mean()))


FD_CASES = [(d, l, k) for d in ("beckmann", "ggx") for l in ("area", "envmap") for k in (2, 3)]


@pytest.mark.parametrize("distr,light,depth", FD_CASES)
def test_forward_matches_finite_differences_of_the_image(distr, light, depth):
    """sample_visible = False: sampler, pdf and value agree, the rule is the derivative of the image's expectation.  The sampled
    directions move with alpha under a fixed seed, so the two estimators agree in expectation only: 4096 spp, block means."""
    sc = filling_plate(distr, light, False)
    fwd, fd1, fd2 = image_derivatives(sc, depth, seed=3, spp=4096, h=2e-2)
    s_fwd, s1, s2 = _stats(fwd), _stats(fd1), _stats(fd2)
    yard = _rel(s1, s2)
    rel = _rel(s_fwd, s2)
    print(f"{distr} {light} depth {depth}: channel means fwd {s_fwd[:3].tolist()} fd {s2[:3].tolist()}; rel mean {float(rel.mean()):.4f} "
          f"max {float(rel.max()):.4f}; FD(h) vs FD(h/2) mean {float(yard.mean()):.4f} max {float(yard.max()):.4f}")
    assert float(s2.abs().min()) > 0
    assert float(yard.mean()) < 0.05 / 4 and float(yard.max()) < 0.5 / 4, "not a valid yardstick"
    assert float(rel.mean()) < 0.05 and float(rel.max()) < 0.5, (s_fwd, s2)


@pytest.mark.parametrize("distr", ["beckmann", "ggx"])
def test_sample_visible_gap_is_measured_not_asserted(distr):
    """sample_visible = True: the fork samples D cos while weight and pdf follow the visible-normal formulas, so weight x pdf is not
    the value and the rule (applied unchanged, as prb.py's eval-based replay does) is not the derivative of what is rendered.  Only
    sign and finiteness are asserted; the gap is printed (MEASUREMENTS 15)."""
    sc = filling_plate(distr, "area", True)
    fwd, _, fd = image_derivatives(sc, 2, seed=3, spp=4096, h=2e-2)
    a, b = fwd.mean(dim=(0, 1)), fd.mean(dim=(0, 1))
    print(f"{distr} sample_visible: channel means fwd {a.tolist()} fd {b.tolist()} ratio {(a / b).tolist()}")
    assert bool(torch.isfinite(fwd).all())
    assert bool((torch.sign(a) == torch.sign(b)).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def test_gradients_accumulate_bit_for_bit():
    sc = two_plate_scene()
    attach_two(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
    p1, p2 = sc.param_grads(), sc.param_grads()
    integ.render_backward(sc, p1, g, sensor=0, seed=4, spp=32)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=32)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=32)
    assert float(p1.alpha.abs().min()) > 0
    assert torch.equal(p2.alpha, 2 * p1.alpha)


def test_nine_slots_are_refused():
    pv, pf = quad(0.0, 0.3, up=True)
    d = {"type": "scene", "cam": sensor([0, 0, 6], [0, 0, 0], res=8, spp=4), "sky": {"type": "constant"}}
    for k in range(9):
        d[f"p{k}"] = {"type": "mesh", "vertices": pv + np.array([0.7 * (k % 3 - 1), 0.7 * (k // 3 - 1), 0.0]), "faces": pf,
                      "bsdf": {"type": "roughconductor", "alpha": 0.1 + 0.02 * k}}
    sc = on_host_bsdf(S.Scene.from_dict(d, device="cpu"))
    for k in range(8):
        sc.attach_alpha(f"p{k}.bsdf")
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((8, 8, 3)), seed=1, spp=4)
    assert int((p.alpha != 0).sum()) == 8
    assert sc.attach_alpha("p8.bsdf") == 8                                                    # attaching is not refused (5 channels)
    with pytest.raises(ValueError, match="at most 8"):
        integ.render_backward(sc, sc.param_grads(), torch.ones((8, 8, 3)), seed=1, spp=4)
    with pytest.raises(ValueError, match="at most 8"):
        integ.render_forward(sc, sc.param_grads(), seed=1, spp=4)


def test_alpha_alone_counts_as_attached():
    sc = two_plate_scene()
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    sc.attach("plate")
    with pytest.raises(NotImplementedError, match="prb: geometry is attached but no colour parameter is"):
        integ.render_backward(sc, sc.param_grads(), torch.ones((12, 12, 3)), seed=1, spp=4)
    sc.attach_alpha("plate.bsdf")
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((12, 12, 3)), seed=1, spp=4)
    assert float(p.alpha.abs().sum()) > 0
    assert float(p.color.abs().sum()) == 0 and float(p.pos.abs().sum()) == 0 and float(p.nrm.abs().sum()) == 0


def test_set_alpha_is_seen_by_the_next_backward():
    sc, ref = two_plate_scene(), two_plate_scene()
    attach_two(sc); attach_two(ref)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
    p0 = sc.param_grads()
    integ.render_backward(sc, p0, g, sensor=0, seed=4, spp=32)
    sc.set_alpha("plate.bsdf", 0.3)
    p1 = sc.param_grads()
    integ.render_backward(sc, p1, g, sensor=0, seed=4, spp=32)
    ref.bsdf_desc[ref.bsdf_names.index("plate.bsdf")]["alpha"] = 0.3
    ref._upload()
    p2 = ref.param_grads()
    integ.render_backward(ref, p2, g, sensor=0, seed=4, spp=32)
    assert not torch.equal(p0.alpha, p1.alpha)
    assert torch.equal(p1.alpha, p2.alpha)


def _free_port():
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc = two_plate_scene()
        sc.tile_paths = 1000                                           # several tiles, dealt over the ranks
        attach_two(sc)
        integ = epsm.load_dict({"type": "prb", "max_depth": 3})
        p = sc.param_grads()
        g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
        integ.render_backward(sc, p, g, sensor=0, seed=4, spp=32)
        q.put((rank, p.flat.clone().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_alpha_gradients_match_single_process():
    sc = two_plate_scene()
    sc.tile_paths = 1000
    attach_two(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    p = sc.param_grads()
    g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
    integ.render_backward(sc, p, g, sensor=0, seed=4, spp=32)
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
