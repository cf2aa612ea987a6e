"""Roughness maps (a `roughconductor` whose alpha is a 1-channel bitmap; Scene.attach_texture('<bsdf>.alpha.data'),
epsm_trace_paths_alpha_texture_backward / _forward) on the host build of the tracer (tests/host_harness/trace_alphamap_host.cpp):
the primal lookup against a scalar alpha, the texel gradients pinned to the scalar roughness adjoint, the transpose identity,
finite differences of the rendered image, the refusals and the gradient buffer's layout, and two ranks.  The GPU twin is
tests/test_gpu_alpha_texture.py."""
import ctypes as C
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _alphamap_host import host_alphamap_tracer, on_host_alphamap
from _reparam_scenes import gradient_map
from _scenes import quad, sensor
from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd.params import ParamGrads
from test_alpha_adjoint import _rel, _stats

UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)


def alpha_bitmap(values, nearest):
    return {"type": "bitmap", "bitmap": np.asarray(values, np.float32), "filter_type": "nearest" if nearest else "bilinear"}


def checker(h=4, w=4, lo=0.1, hi=0.3, seed=0):
    """(h, w) roughnesses: a two-level checker with a little noise, so that no two texels are alike."""
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (np.where((i + j) % 2 == 0, lo, hi) + 0.03 * np.random.default_rng(seed).random((h, w))).astype(np.float32)


def map_scene(device="cpu", res=12, spp=32, alpha=None, alpha2=0.25, uv=UV, floor_tex=None):
    """test_alpha_adjoint.two_plate_scene's geometry -- two rough plates (Beckmann and GGX, the second `twosided`) over a diffuse
    floor under an area light and a constant sky -- with texture coordinates on the plates, so that either alpha may be a bitmap
    (a dict) or a scalar; the floor's reflectance may be a bitmap too."""
    pv, pf = quad(0.3, 0.9, up=True)
    qv = pv + np.array([1.2, 0.6, 0.4]); pv = pv + np.array([-0.7, 0.0, 0.0])
    fv, ff = quad(0.0, 4.0, up=True)
    lv, lf = quad(3.0, 0.6, up=False)
    refl = {"type": "rgb", "value": [0.5, 0.4, 0.3]} if floor_tex is None else {"type": "bitmap", "bitmap": floor_tex}
    ggx = {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": alpha2}
    d = {"type": "scene", "cam": sensor([0.0, -3.5, 2.5], [0.2, 0.2, 0.3], up=(0, 0, 1), res=res, spp=spp, rfilter="gaussian"),
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "texcoords": uv, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "distribution": "beckmann", "alpha": 0.15 if alpha is None else alpha,
                            "sample_visible": False}},
         "plate2": {"type": "mesh", "vertices": qv, "faces": pf, "texcoords": uv, "face_normals": True,
                    "bsdf": {"type": "twosided", "bsdf": ggx}},
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "texcoords": UV, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": refl}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [12.0, 10.0, 8.0]}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.4}}}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_alphamap(sc)
    sc.tracer = "mega"
    return sc


def attach_maps(sc):
    """Attaches every roughness map of the scene; the slots."""
    return [sc.attach_texture(f"{n}.alpha.data") for n, b in zip(sc.bsdf_names, sc.bsdf_desc) if "alpha_texture" in b]


# ---------------------------------------------------------------------------------------------------------------------
# 1. primal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ_name", ["prb", "manifold"])
def test_constant_map_renders_like_the_scalar(integ_name):
    """A constant `nearest` map reads back the very float the scalar holds: the same bits.  Bilinear weights sum to 1 within an ulp
    or two, so alpha differs by ~1e-7 relative and the image within 1e-5 of its mean."""
    a = 0.2
    integ = epsm.load_dict({"type": integ_name, "max_depth": 3})
    want = integ.render(map_scene(alpha=a), sensor=0, seed=3, spp=32)
    assert want.shape[-1] == (3 if integ_name == "prb" else 5) and float(want.abs().sum()) > 0
    got = integ.render(map_scene(alpha=alpha_bitmap(np.full((4, 4), a), True)), sensor=0, seed=3, spp=32)
    assert torch.equal(got, want)
    got = integ.render(map_scene(alpha=alpha_bitmap(np.full((4, 4), a), False)), sensor=0, seed=3, spp=32)
    gap = float((got - want).abs().max())
    print(f"{integ_name}: bilinear constant map against the scalar: max gap {gap:.3e}, image mean {float(want[..., :3].mean()):.3e}")
    assert gap <= 1e-5 * float(want[..., :3].mean())


def test_the_map_is_looked_up_where_the_plate_is_seen():
    """Not a constant: the image differs from every scalar's, and the wavefront tracer agrees with the one-launch tracer."""
    sc = map_scene(alpha=alpha_bitmap(checker(), True))
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    img = integ.render(sc, sensor=0, seed=3, spp=32)
    flat = integ.render(map_scene(alpha=float(checker().mean())), sensor=0, seed=3, spp=32)
    assert float((img - flat).abs().max()) > 1e-3 * float(flat.mean())
    sc.tracer = "wavefront"
    wf = integ.render(sc, sensor=0, seed=3, spp=32)
    assert float((wf - img).abs().max()) <= 1e-5 * float(img.mean())


@pytest.mark.parametrize("nearest", [True, False])
def test_set_texture_then_render_equals_a_scene_built_from_the_array(nearest):
    new = checker(seed=5)
    sc = map_scene(alpha=alpha_bitmap(checker(), nearest))
    slot = sc.attach_texture("plate.bsdf.alpha.data")
    assert tuple(sc.texture_values(slot).shape) == (4, 4)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    before = integ.render(sc, sensor=0, seed=3, spp=32)
    sc.set_texture(slot, torch.from_numpy(new))
    after = integ.render(sc, sensor=0, seed=3, spp=32)
    want = integ.render(map_scene(alpha=alpha_bitmap(new, nearest)), sensor=0, seed=3, spp=32)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)
    assert torch.equal(sc.texture_values(slot), torch.from_numpy(new))
    assert sc.bsdf_desc[sc.bsdf_names.index("plate.bsdf")]["alpha"] == pytest.approx(float(new.mean()))


# ---------------------------------------------------------------------------------------------------------------------
# 2. pinned to the scalar roughness adjoint
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nearest", [True, False])
def test_texel_gradients_of_a_constant_map_sum_to_the_scalar_gradient(nearest):
    """Every texel of a constant map is the same alpha: the sum of the texel gradients is d loss / d alpha of the scalar twin, path
    term by path term (the footprint's weights sum to 1); only the order of the summation differs -- 1e-4 relative, the project's
    transpose bound."""
    a = 0.2
    g = 0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3))
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    twin = map_scene(alpha=a)
    slot_s = twin.attach_alpha("plate.bsdf")
    ps = twin.param_grads()
    integ.render_backward(twin, ps, g, sensor=0, seed=4, spp=32)
    sc = map_scene(alpha=alpha_bitmap(np.full((4, 4), a), nearest))
    slot = sc.attach_texture("plate.bsdf.alpha.data")
    p = sc.param_grads()
    integ.render_backward(sc, p, g, sensor=0, seed=4, spp=32)
    want, got = float(ps.alpha[slot_s]), float(p.texture(slot).double().sum())
    print(f"nearest={nearest}: sum of texel gradients {got:.6e}, scalar gradient {want:.6e}")
    assert tuple(p.texture(slot).shape) == (4, 4) and int((p.texture(slot) != 0).sum()) > 4
    assert want != 0 and abs(got - want) <= 1e-4 * abs(want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. transpose
# ---------------------------------------------------------------------------------------------------------------------
def transpose_gap(integ, sc, seed, spp, gen):
    """(|a - b|, S, a, params): a = sum g * J t, b = sum J^T g * t, S = sum |g * J t| + sum |J^T g * t|."""
    s = sc.sensors[0]
    t = sc.param_grads()
    for k in range(len(sc.texture_slots)):
        t.texture(k)[:] = torch.randn(tuple(t.texture(k).shape), generator=gen).to(sc.device)
    if t.C:
        t.color[:] = torch.randn((t.C, 3), generator=gen).to(sc.device)
    g = torch.randn((s.height, s.width, 3), generator=gen).to(sc.device)
    fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp)
    params = sc.param_grads()
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    a = float((g * fwd).double().sum())
    b = float((params.flat * t.flat).double().sum())
    S_ = float((g * fwd).abs().double().sum()) + float((params.flat * t.flat).abs().double().sum())
    return abs(a - b), S_, a, params


def _both_maps(nearest, device="cpu", **kw):
    return map_scene(device, alpha=alpha_bitmap(checker(), nearest), alpha2=alpha_bitmap(checker(4, 4, 0.15, 0.35, seed=2), nearest), **kw)


def _with_colour_and_bitmap(device="cpu", **kw):
    tex = (0.2 + 0.7 * np.random.default_rng(0).random((4, 4, 3))).astype(np.float32)
    return map_scene(device, alpha=alpha_bitmap(checker(), False), floor_tex=tex, **kw)


TRANSPOSE = {
    "bilinear": (lambda **kw: _both_maps(False, **kw), "prb", attach_maps),
    "nearest": (lambda **kw: _both_maps(True, **kw), "prb", attach_maps),
    "with_colour_and_bitmap": (_with_colour_and_bitmap, "prb",
                               lambda sc: [sc.attach_radiance("light"), sc.attach_texture("floor.bsdf.reflectance.data")] + attach_maps(sc)),
    "prb_reparam_no_geometry": (lambda **kw: _both_maps(False, **kw), "prb_reparam", attach_maps),
}
TRANSPOSE_CASES = [(n, d) for n in TRANSPOSE for d in ((2, 4) if n in ("bilinear", "nearest") else (3,))]


@pytest.mark.parametrize("name,depth", TRANSPOSE_CASES)
def test_forward_is_the_transpose_of_backward(name, depth):
    make, integ_name, attach = TRANSPOSE[name]
    sc = make()
    slots = attach(sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params = transpose_gap(integ, sc, seed=5, spp=32, gen=torch.Generator().manual_seed(2 + depth))
    for k in sc.alpha_map_slots():
        assert tuple(params.texture(k).shape) == (4, 4) and float(params.texture(k).abs().sum()) > 0
    assert len(slots) == len(sc.texture_slots) + params.C
    assert S_ > 0 and abs(a) > 0
    assert gap <= 1e-4 * S_, (gap, S_)


# ---------------------------------------------------------------------------------------------------------------------
# 4. finite differences of the rendered image, one texel at a time
# ---------------------------------------------------------------------------------------------------------------------
def filling_plate_map(distr, light, values, res=8, spp=4096, device="cpu", nearest=True, uv=UV):
    """test_alpha_adjoint.filling_plate with sample_visible = False and the roughness a map over the plate (the finite differences'
    is 2 x 2 `nearest`)."""
    pv, pf = quad(0.0, 3.0, up=True)
    d = {"type": "scene", "cam": sensor([0.0, -1.2, 2.0], [0.0, 0.0, 0.0], up=(0, 0, 1), fov=30, res=res, spp=spp, rfilter="gaussian"),
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "texcoords": uv, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "material": "Cu", "distribution": distr, "alpha": alpha_bitmap(values, nearest),
                            "sample_visible": False}}}
    if light == "area":
        lv, lf = quad(4.0, 1.5, up=False)
        d["light"] = {"type": "mesh", "vertices": lv + np.array([0.0, 1.5, 0.0]), "faces": lf, "face_normals": True,
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6.0, 5.0, 4.0]}}}
    else:
        d["sky"] = {"type": "envmap", "bitmap": gradient_map(), "to_world": S.rotate([1.0, 0.0, 0.0], 90.0)}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_alphamap(sc)
    sc.tracer = "mega"
    return sc


@pytest.mark.parametrize("distr,light", [("beckmann", "area"), ("ggx", "envmap")])
def test_forward_matches_finite_differences_texel_by_texel(distr, light):
    """One distribution per light type, depth 2.  The plate fills the film and the 2 x 2 map covers the plate, so each texel owns
    a quadrant of the image and reaches the others through the reconstruction filter; the statistics of test_alpha_adjoint
    (_stats: channel means and 4 x 4 block means; _rel: the reference's error image, floored at 0.2 of the mean magnitude).
    Thresholds: the reference's (mean < 0.05, max < 0.5); the yardstick FD(h) against FD(h / 2) a quarter of them."""
    base = np.array([[0.25, 0.32], [0.3, 0.27]], np.float32)
    seed, spp, h = 3, 4096, 2e-2
    sc = filling_plate_map(distr, light, base)
    slot = sc.attach_texture("plate.bsdf.alpha.data")
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    seen = 0
    for r in range(2):
        for c in range(2):
            t = sc.param_grads()
            t.texture(slot)[r, c] = 1.0
            fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp).double().cpu()
            fds = []
            for step in (h, h / 2):
                out = []
                for sgn in (+1, -1):
                    v = base.copy(); v[r, c] += sgn * step
                    sc.set_texture(slot, v)
                    out.append(integ.render(sc, sensor=0, seed=seed, spp=spp).double().cpu())
                fds.append((out[0] - out[1]) / (2 * step))
            sc.set_texture(slot, base)
            s_fwd, s1, s2 = _stats(fwd), _stats(fds[0]), _stats(fds[1])
            yard, rel = _rel(s1, s2), _rel(s_fwd, s2)
            print(f"{distr} {light} texel ({r},{c}): channel means fwd {s_fwd[:3].tolist()} fd {s2[:3].tolist()}; block means fd "
                  f"{s2[3:].tolist()}; rel mean {float(rel.mean()):.4f} max {float(rel.max()):.4f}; FD(h) vs FD(h/2) mean "
                  f"{float(yard.mean()):.4f} max {float(yard.max()):.4f}")
            assert float(s2.abs().min()) > 0
            assert float(yard.mean()) < 0.05 / 4 and float(yard.max()) < 0.5 / 4, "not a valid yardstick"
            assert float(rel.mean()) < 0.05 and float(rel.max()) < 0.5, (s_fwd, s2)
            seen += 1
    assert seen == 4


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals and layout
# ---------------------------------------------------------------------------------------------------------------------
def test_loader_refusals():
    with pytest.raises(ValueError, match="ONE channel.*luminance"):
        map_scene(alpha=alpha_bitmap(np.full((4, 4, 3), 0.2), True))
    with pytest.raises(ValueError, match="must be > 0"):
        map_scene(alpha=alpha_bitmap(np.array([[0.2, 0.0], [0.1, 0.3]]), True))
    with pytest.raises(ValueError, match="must be > 0"):
        map_scene(alpha=alpha_bitmap(np.array([[0.2, -0.1], [0.1, 0.3]]), True))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            map_scene(alpha=alpha_bitmap(np.array([[0.2, bad], [0.1, 0.3]]), True))
    with pytest.raises(ValueError, match="wrap_mode"):
        map_scene(alpha=dict(alpha_bitmap(checker(), True), wrap_mode="clamp"))
    with pytest.raises(ValueError, match="to_uv"):
        map_scene(alpha=dict(alpha_bitmap(checker(), True), to_uv=np.eye(3)))
    sc = map_scene(alpha={"type": "bitmap", "data": checker()[:, :, None]})            # `data`, (H, W, 1): one channel
    b = sc.bsdf_desc[sc.bsdf_names.index("plate.bsdf")]
    assert b["alpha"] == pytest.approx(float(checker().mean())) and b["alpha_texture"]["nearest"] == 0


def test_attach_and_set_refusals():
    sc = map_scene(alpha=alpha_bitmap(checker(), True))
    for call in (lambda: sc.attach_alpha("plate.bsdf"), lambda: sc.set_alpha("plate.bsdf", 0.2)):
        with pytest.raises(ValueError, match=r"attach_texture\('plate\.bsdf\.alpha\.data'\)"):
            call()
    with pytest.raises(ValueError, match="roughness of 'plate2.bsdf' is not a bitmap"):
        sc.attach_texture("plate2.bsdf.alpha.data")
    with pytest.raises(ValueError, match="not a roughconductor"):
        sc.attach_texture("floor.bsdf.alpha.data")
    slot = sc.attach_texture("plate.bsdf.alpha.data")
    assert sc.attach_texture("plate.bsdf.alpha.data") == slot and sc.texture_slots[slot][0] == "alpha"
    with pytest.raises(ValueError, match="must be > 0"):
        sc.set_texture(slot, np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        sc.set_texture(slot, np.full((2, 2), 0.2, np.float32))
    with pytest.raises(ValueError, match="ONE channel"):
        sc.set_texture(slot, np.full((4, 4, 3), 0.2, np.float32))
    assert sc.attach_alpha("plate2.bsdf") == 0                       # (the scalar neighbour is untouched by all this)
    bs = sc._bsdf_structs()
    i = sc.bsdf_names.index("plate.bsdf")
    assert bs[i].alpha_slot == -1 and bs[i].texture == 0 and bs[sc.bsdf_names.index("plate2.bsdf")].texture == -1


def test_integrator_refusals():
    sc = map_scene(alpha=alpha_bitmap(checker(), True))
    g3, g5 = torch.ones((12, 12, 3)), torch.ones((12, 12, 5))
    sc.attach_texture("plate.bsdf.alpha.data")
    with pytest.raises(NotImplementedError, match="5-channel manifold branch has no gradient for a roughness map"):
        epsm.load_dict({"type": "manifold", "max_depth": 3}).render_backward(sc, sc.param_grads(), g5, seed=1, spp=4)
    reparam = epsm.load_dict({"type": "prb_reparam", "max_depth": 3})
    p = sc.param_grads()
    reparam.render_backward(sc, p, g3, seed=1, spp=4)                  # nothing geometric attached: fine
    assert float(p.texture(0).abs().sum()) > 0
    sc.attach("plate2")
    for call in (lambda: reparam.render_backward(sc, sc.param_grads(), g3, seed=1, spp=4),
                 lambda: reparam.render_forward(sc, sc.param_grads(), seed=1, spp=4)):
        with pytest.raises(NotImplementedError, match="prb_reparam: the scene has a roughness map"):
            call()
    cam = map_scene(alpha=alpha_bitmap(checker(), True))
    cam.attach_sensor()
    with pytest.raises(NotImplementedError, match="prb_reparam: the scene has a roughness map"):
        reparam.render_backward(cam, cam.param_grads(), g3, seed=1, spp=4)


def test_map_slot_alone_counts_as_attached():
    sc = map_scene(alpha=alpha_bitmap(checker(), False))
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    sc.attach("plate2")
    with pytest.raises(NotImplementedError, match="prb: geometry is attached but no colour parameter is"):
        integ.render_backward(sc, sc.param_grads(), torch.ones((12, 12, 3)), seed=1, spp=4)
    slot = sc.attach_texture("plate.bsdf.alpha.data")
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((12, 12, 3)), seed=1, spp=4)
    assert float(p.texture(slot).abs().sum()) > 0
    assert float(p.color.abs().sum()) == 0 and float(p.pos.abs().sum()) == 0 and float(p.alpha.abs().sum()) == 0


def test_the_ninth_texture_slot_is_refused():
    pv, pf = quad(0.0, 0.3, up=True)
    d = {"type": "scene", "cam": sensor([0, 0, 6], [0, 0, 0], res=8, spp=4), "sky": {"type": "constant"}}
    for k in range(9):
        d[f"p{k}"] = {"type": "mesh", "vertices": pv + np.array([0.7 * (k % 3 - 1), 0.7 * (k // 3 - 1), 0.0]), "faces": pf, "texcoords": UV,
                      "bsdf": {"type": "roughconductor", "alpha": alpha_bitmap(checker(2, 2, seed=k), True)}}
    sc = on_host_alphamap(S.Scene.from_dict(d, device="cpu"))
    for k in range(8):
        assert sc.attach_texture(f"p{k}.bsdf.alpha.data") == k
    p = sc.param_grads()
    epsm.load_dict({"type": "prb", "max_depth": 2}).render_backward(sc, p, torch.ones((8, 8, 3)), seed=1, spp=4)
    assert all(float(p.texture(k).abs().sum()) > 0 for k in range(8))
    with pytest.raises(ValueError, match="at most 8 texture parameters"):
        sc.attach_texture("p8.bsdf.alpha.data")


def test_param_grads_layout_with_and_without_a_roughness_map():
    off = lambda p, t: (t.data_ptr() - p.flat.data_ptr()) // 4
    old = ParamGrads(5, 2, device="cpu", n_colors=1, tex_shapes=[(4, 6), (2, 3)], n_rigid=1, cam_rotation=True, n_conductors=1)
    n0 = 6 * 5 + 2 + 3 + 3
    assert [off(old, t) for t in (old.texture(0), old.texture(1), old.rigid, old.cam_rotation, old.conductor)] == \
        [n0, n0 + 72, n0 + 90, n0 + 96, n0 + 99] and old.flat.numel() == n0 + 108
    assert old.tex_shapes == [(4, 6), (2, 3)] and tuple(old.texture(1).shape) == (2, 3, 3)
    new = ParamGrads(5, 2, device="cpu", n_colors=1, tex_shapes=[(4, 6), (3, 5, 1), (2, 3)], n_rigid=1, cam_rotation=True, n_conductors=1)
    assert [off(new, t) for t in (new.texture(0), new.texture(1), new.texture(2), new.rigid, new.cam_rotation, new.conductor)] == \
        [n0, n0 + 72, n0 + 87, n0 + 105, n0 + 111, n0 + 114] and new.flat.numel() == n0 + 123
    assert tuple(new.texture(1).shape) == (3, 5) and tuple(new.texture(2).shape) == (2, 3, 3)
    assert tuple(new.scratch().texture(1).shape) == (3, 5)
    for a, b in ((old.pos, new.pos), (old.nrm, new.nrm), (old.alpha, new.alpha), (old.cam_origin, new.cam_origin), (old.color, new.color),
                 (old.texture(0), new.texture(0))):
        assert off(old, a) == off(new, b) and a.shape == b.shape
    with pytest.raises(ValueError, match="tex_shapes"):
        ParamGrads(5, tex_shapes=[(4, 6, 3)], device="cpu")
    tex = (0.2 + 0.7 * np.random.default_rng(0).random((4, 4, 3))).astype(np.float32)
    sc = map_scene(alpha=alpha_bitmap(checker(3, 5), True), floor_tex=tex)
    sc.attach_texture("floor.bsdf.reflectance.data"); sc.attach_texture("plate.bsdf.alpha.data")
    assert sc.texture_shapes() == [(4, 4), (3, 5, 1)]
    p = sc.param_grads()
    assert tuple(p.texture(0).shape) == (4, 4, 3) and tuple(p.texture(1).shape) == (3, 5)
    stale = ParamGrads(sc.V, 0, device="cpu", tex_shapes=[(4, 4), (3, 5)])
    with pytest.raises(ValueError, match="texture slots are attached"):
        epsm.load_dict({"type": "prb", "max_depth": 2}).render_backward(sc, stale, torch.ones((12, 12, 3)), seed=1, spp=4)


def test_abi_is_unchanged_and_the_entry_points_are_exported():
    assert C.sizeof(S.EpsmTexture) == 24 and S.EpsmTexture.channels.offset == 20 and S.EpsmTexture.channels.size == 4
    assert C.sizeof(S.EpsmBsdf) == 76 + 4 and S.EpsmBsdf.texture.offset == 72
    lib = host_alphamap_tracer()
    for name in ("epsm_trace_paths_alpha_texture_backward", "epsm_trace_paths_alpha_texture_forward"):
        assert hasattr(lib, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "epsm_trace.h")).read()
    assert "uint32_t channels;" in header and "int epsm_trace_paths_alpha_texture_backward(" in header
    assert "int epsm_trace_paths_alpha_texture_forward(" in header
    from epsm_mitsuba3_amd import _lib
    assert _lib.ABI_VERSION == 7
    so = os.path.join(root, "epsm_mitsuba3_amd", "libepsm_hip.so")
    if os.path.isfile(so):                                             # (the product library, where it is built: a symbol table needs no GPU)
        product = C.CDLL(so)
        assert product.epsm_abi_version() == 7
        for name in ("epsm_trace_paths_alpha_texture_backward", "epsm_trace_paths_alpha_texture_forward"):
            assert hasattr(product, name), name


def test_entry_points_check_their_arguments():
    sc = map_scene(alpha=alpha_bitmap(checker(), True))
    slot = sc.attach_texture("plate.bsdf.alpha.data")
    n = sc.sensors[0].wavefront_size(4)
    _, radiance, _ = sc.trace_color(0, 1, 4, 3, 0, n)
    radiance = radiance.contiguous()
    adj = torch.ones((n, 3))
    g = [torch.zeros((4, 4))]
    sc.trace_alpha_texture_backward(0, 1, 4, 3, 0, n, radiance, adj, g)
    assert float(g[0].abs().sum()) > 0
    # N == 0 is fine, and with no buffer backward is a no-op
    lib = host_alphamap_tracer()
    cs = sc.sensors[0].c_struct()
    head = (C.byref(sc.c_scene), C.byref(cs), C.c_uint32(1), 4, 3, 5, C.c_int64(0))
    assert lib.epsm_trace_paths_alpha_texture_backward(*head, C.c_int64(0), None, None, None, None) == 0
    assert lib.epsm_trace_paths_alpha_texture_forward(*head, C.c_int64(0), None, None, None, None) == 0
    assert lib.epsm_trace_paths_alpha_texture_backward(*head, C.c_int64(n), C.c_void_p(radiance.data_ptr()), C.c_void_p(adj.data_ptr()),
                                                       None, None) == 0
    assert lib.epsm_trace_paths_alpha_texture_backward(*head, C.c_int64(n), None, C.c_void_p(adj.data_ptr()), None, None) != 0
    # a buffer handed to the RGB texel adjoint for the roughness map's texture is never written: (H, W) is not (H, W, 3)
    arr = (C.c_void_p * 1)(g[0].data_ptr())
    before = g[0].clone()
    assert lib.epsm_trace_paths_texture_backward(*head, C.c_int64(n), C.c_void_p(radiance.data_ptr()), C.c_void_p(adj.data_ptr()),
                                                 C.cast(arr, C.c_void_p), None, None) == 0
    assert torch.equal(g[0], before) and slot == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. two ranks
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def _two_rank_backward():
    sc = _with_colour_and_bitmap()
    sc.tile_paths = 1000                                               # several tiles, dealt over the ranks
    sc.attach_texture("floor.bsdf.reflectance.data"); attach_maps(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    p = sc.param_grads()
    g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
    integ.render_backward(sc, p, g, sensor=0, seed=4, spp=32)
    return sc, p


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _two_rank_backward()[1].flat.clone().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_roughness_map_gradients_match_single_process():
    sc, p = _two_rank_backward()
    assert float(p.texture(1).abs().sum()) > 0 and float(p.texture(0).abs().sum()) > 0
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
    for r in range(2):
        np.testing.assert_allclose(got[r], want, rtol=1e-4, atol=1e-6 * float(np.abs(want).max()))
