"""Scene.attach_ior on the device, traced: a glass slab and a rough metal plate over a lit floor, 32 x 32 at 4 spp, seen from above
(pixels through the slab: camera -> two refractions -> floor, `manifold`'s chains; pixels beside it: floor -> two refractions ->
light, `manifold_caustic`'s).  ``params.alpha[slot]`` of the 5-channel branch against the sum over the device's own trace records,
formed with the oracle's first-vertex tangent and the float64 host core (tests/_ior_host.py), by test_gpu_pipeline.py's yardstick
for ``alpha``: 2e-3 of the buffer's magnitude plus the allowance (components within 2 % of the clamp, twice the float32 core's
distance from the float64 one), the allowance below a tenth of the magnitude.  With the default flags (first-hit fusion, path list,
native log) and with them off; a tile against its halves; a scene with both kinds of slot; the option after a call on a scene
without an IOR slot; exp/ior.py for a handful of iterations."""
import numpy as np
import pytest
import torch

from _scenes import quad, sensor
from epsm_mitsuba3_amd import scene as S

pytestmark = pytest.mark.gpu

RES, SPP, SEED = 32, 4, 5
FLAGS = {"default": {}, "flags off": {"fuse_first_hit": False, "packed_log": False, "gradient_only": False}}


def _scene(dev, glass=True, metal=True):
    fv, ff = quad(0.0, 5.0, up=True)
    tv, tf = quad(1.0, 1.0, up=True)
    bv, bf = quad(0.8, 1.0, up=False)
    lv, lf = quad(2.5, 0.5, up=False)
    mv, mf = quad(0.3, 0.6, up=True)
    g = {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0}
    d = {"type": "scene", "cam": sensor([0.0, -3.2, 2.2], [0.3, 0.0, 0.4], up=(0, 0, 1), fov=50, res=RES, spp=SPP, rfilter="gaussian"),
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.7, 0.7]}}},
         "top": {"type": "mesh", "vertices": tv, "faces": tf, "face_normals": True, "bsdf": g},
         "bottom": {"type": "mesh", "vertices": bv, "faces": bf, "face_normals": True, "bsdf": dict(g)},
         "plate": {"type": "mesh", "vertices": mv + np.array([1.9, 0.2, 0.0]), "faces": mf, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": 0.15}},
         "wall": {"type": "mesh", "vertices": np.array([[-5, 3.0, 0], [5, 3.0, 0], [5, 3.0, 8], [-5, 3.0, 8]], float),      # what the plate mirrors
                  "faces": np.array([[0, 2, 1], [0, 3, 2]]), "face_normals": True,
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.6]}}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 30.0}}}}
    sc = S.Scene.from_dict(d, device=dev)
    slots = {}
    if metal:
        slots["plate"] = sc.attach_alpha("plate.bsdf")
    if glass:
        slots["top"], slots["bottom"] = sc.attach_ior("top.bsdf"), sc.attach_ior("bottom.bsdf")
    return sc, slots


def _grad_in(dev, scale=2e-5):
    g = torch.Generator().manual_seed(23)
    return (torch.randn((RES, RES, 5), generator=g) * scale).to(dev)


def _integrator(kind, flags):
    import epsm_mitsuba3_amd as epsm
    integ = epsm.load_dict({"type": kind, "max_depth": 6, **flags})
    integ.backward_spp = SPP
    return integ


def _backward(sc, kind, flags, grad_in):
    p = sc.param_grads()
    _integrator(kind, flags).render_backward(sc, p, grad_in, seed=SEED)
    torch.cuda.synchronize()
    return p


def _reference(sc, kind, grad_in):
    """-> (alpha (B,), allowance (B,), refracted (B,)) from the device's own per-field trace of the backward wavefront"""
    from _ior_host import ior_alpha_buffer
    from epsm_mitsuba3_amd.synth import path_info_to
    from oracle.binding import oracle_first_vertex_tangent
    integ = _integrator(kind, {})
    B = len(sc.alpha_slots)
    out = [torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.bool)]
    for tr in sc.trace_paths(sensor=integ.backward_sensor, seed=SEED, spp=SPP, max_depth=integ.tracer_depth(), max_log_depth=integ.max_log_depth):
        pi = path_info_to(tr.path_info, device="cpu")
        si = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()} for r in tr.scatter_info]
        first = pi[1]
        dlduv, dldp, _ = oracle_first_vertex_tangent(tr.ray_o, tr.ray_d, tr.ray_dx, tr.ray_dy, grad_in.cpu(), tr.spp, tr.res, first["points"][0],
                                                     first["points"][1], first["points"][2], first["active"], 2, tr.path_offset)
        run = lambda clip, dtype: ior_alpha_buffer(kind, pi, si, dlduv.double(), dldp.double(), B, clip=clip, dtype=dtype)
        a, refr = run(0.1, torch.float64)
        out[0] += a
        out[1] += (run(0.098, torch.float64)[0] - run(0.102, torch.float64)[0]).abs() + 2 * (run(0.1, torch.float32)[0] - a).abs()
        out[2] |= refr
    return out


def _repeats(a, b):
    """Two launches of one arithmetic on these 4 096 paths: an entry is the float32 sum of at most 32 workgroup sums (windows of
    128 paths) added by float atomics in any order -- each addition rounds by half an ulp of a running sum that stays below the
    entry's own magnitude here (one sign per slot, checked by the caller's reference), so two orders part by at most 32 x 2^-24 =
    2^-19 of the entry -- and every path's term may take the 2^-44 fixed-point row or not (rounding 2^-45 each)."""
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a - b).abs() <= 2.0 ** -19 * b.abs() + RES * RES * SPP * 2.0 ** -45).all())


def _assert_yardstick(mine, ref, allow, what):
    m = float(ref.abs().max())
    err = (mine.double().cpu() - ref).abs()
    print(*what, "alpha", mine.tolist(), "reference", ref.tolist(), "allowance / m", float(allow.max()) / max(m, 1e-300),
          "worst (|diff| - allowance) / m", float((err - allow).max()) / max(m, 1e-300))
    assert m > 0, what
    assert float(allow.max()) < 0.1 * m, what
    assert bool((err <= 2e-3 * m + allow).all()), what


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("kind", ["manifold", "manifold_caustic"])
def test_traced_ior_slots_match_the_sum_over_the_trace_records(kind, flags):
    dev = torch.device("cuda", 0)
    sc, slots = _scene(dev)
    grad_in = _grad_in(dev)
    ref, allow, refracted = _reference(sc, kind, grad_in)
    assert bool(refracted[slots["top"]]) and bool(refracted[slots["bottom"]])
    assert sc.ior_slots == sorted([slots["top"], slots["bottom"]])
    p = _backward(sc, kind, FLAGS[flags], grad_in)
    _assert_yardstick(p.alpha, ref, allow, (kind, flags))
    assert float(ref[slots["top"]]) != 0.0 and float(ref[slots["bottom"]]) != 0.0
    # two calls repeat -- the order of the float atomics aside, which no two launches of the accumulating kernel share
    # (test_gpu_ior_backward.py): _REPEAT below
    q = _backward(sc, kind, FLAGS[flags], grad_in)
    print(kind, flags, "two calls", p.alpha.tolist(), q.alpha.tolist())
    assert _repeats(p.alpha, q.alpha), (p.alpha.tolist(), q.alpha.tolist())
    # a tile equals the sum of its halves
    sc.tile_paths = RES * RES * SPP // 2
    halves = _backward(sc, kind, FLAGS[flags], grad_in)
    _assert_yardstick(halves.alpha, ref, allow, (kind, flags, "two tiles"))
    m = float(ref.abs().max())
    assert bool(((halves.alpha - p.alpha).double().cpu().abs() <= 2e-3 * m + allow).all())


@pytest.mark.parametrize("kind", ["manifold", "manifold_caustic"])
def test_a_scene_with_both_kinds_of_slot_fills_both(kind):
    """The rough metal's alpha slot next to the glass: what it holds is what it holds in the run without attach_ior (the order of
    the float additions aside: ``_repeats``)."""
    dev = torch.device("cuda", 0)
    grad_in = _grad_in(dev)
    both, slots = _scene(dev)
    metal_only, slots_m = _scene(dev, glass=False)
    assert slots_m["plate"] == slots["plate"] == 0 and metal_only.ior_slots == []
    p, q = _backward(both, kind, {}, grad_in), _backward(metal_only, kind, {}, grad_in)
    a, b = float(p.alpha[slots["plate"]]), float(q.alpha[0])
    print(kind, "plate alpha with / without attach_ior", a, b, "glass", float(p.alpha[slots["top"]]), float(p.alpha[slots["bottom"]]))
    if kind == "manifold":
        assert b != 0.0
    assert _repeats(torch.tensor([a]), torch.tensor([b])), (a, b)
    assert float(p.alpha[slots["top"]]) != 0.0 and float(p.alpha[slots["bottom"]]) != 0.0
    # the 3-channel colour branch leaves the IOR slots at zero (detached sampling cannot see the refraction direction)
    c = both.param_grads()
    _integrator(kind, {}).render_backward(both, c, torch.ones((RES, RES, 3), device=dev) * 1e-3, seed=SEED)
    torch.cuda.synchronize()
    assert float(c.alpha[slots["top"]]) == 0.0 and float(c.alpha[slots["bottom"]]) == 0.0


def test_without_an_ior_slot_the_integrator_leaves_the_option_at_zero():
    from epsm_mitsuba3_amd import _lib
    dev = torch.device("cuda", 0)
    sc, _ = _scene(dev, glass=False)
    lib = _lib.lib()
    before = lib.epsm_get_option(_lib.OPT_IOR_GRADS)
    try:
        assert lib.epsm_set_option(_lib.OPT_IOR_GRADS, 1) == 0
        _backward(sc, "manifold", {}, _grad_in(dev))
        assert lib.epsm_get_option(_lib.OPT_IOR_GRADS) == 0
        glass, _ = _scene(dev)
        _backward(glass, "manifold", {}, _grad_in(dev))
        assert lib.epsm_get_option(_lib.OPT_IOR_GRADS) == 0              # (1 for the call's launches, the default behind it)
        assert lib.epsm_set_option(_lib.OPT_IOR_GRADS, 2) == -22
        _backward(sc, "manifold_caustic", {}, _grad_in(dev))
        assert lib.epsm_get_option(_lib.OPT_IOR_GRADS) == 0
    finally:
        lib.epsm_set_option(_lib.OPT_IOR_GRADS, before)


def test_exp_ior_moves_towards_the_target(monkeypatch):
    """exp/ior.py at a 32 x 32 film for a handful of iterations: the fitted IOR ends strictly closer to the target than it began
    -- the sign of the gradient and the plumbing attach_ior -> render_backward -> set_ior; the gradient's size is pinned by
    test_ior_snell.py and the tests above."""
    from epsm_mitsuba3_amd import _lib, optim
    from epsm_mitsuba3_amd.exp import caustic_sphere, ior
    for mod in (caustic_sphere, ior):
        monkeypatch.setattr(mod, "resolution", 32)
        monkeypatch.setattr(mod, "match_res", 16)
        monkeypatch.setattr(mod, "spp", 32)
    history, opt = optim.run("manifold_caustic", "ior", device="cuda", iterations=8, log=lambda s: None)
    print("exp/ior.py |int_ior - target| per iteration", [round(h, 4) for h in history])
    assert _lib.lib().epsm_get_option(_lib.OPT_IOR_GRADS) == 0
    assert len(history) == 9 and history[-1] < history[0]
