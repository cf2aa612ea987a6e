"""Scene.attach_ior through the host twin of the tracer (tests/_scenes.py): what a dielectric with a slot logs, and what it leaves alone.

A glass slab (int_ior 1.5 in a medium of 1.1) over a rough metal floor whose alpha is attached in both runs, so that both logs
carry ``aux``.  The attached run against the unattached one: every word of the log is the same except the ``aux`` words of the
dielectric vertices -- slot in aux[0]; aux[1] = d eta / d int_ior = 1 / ext_ior on a refraction into the glass, -eta / int_ior on
one out of it, 0 on a reflection (csrc/epsm_trace_core.h, bsdf_sample).  attach_ior's refusals, and the NotImplementedError of the
integrator routes that cannot fill the slot."""
import numpy as np
import pytest
import torch

from _scenes import on_host, quad, sensor
from epsm_mitsuba3_amd import scene as S

INT, EXT = 1.5, 1.1
N = 8 * 8 * 16


def _slab(int_ior=INT, ext_ior=EXT):
    top_v, top_f = quad(1.0, 4.0, up=True)
    bot_v, bot_f = quad(0.0, 4.0, up=False)
    flo_v, flo_f = quad(-1.0, 6.0, up=True)
    lv, lf = quad(4.0, 1.0, up=False)
    glass = {"type": "dielectric", "int_ior": int_ior, "ext_ior": ext_ior}
    d = {"type": "scene", "cam": sensor([0, -2.0, 3.0], [0, 0, 1.0], up=(0, 0, 1), res=8, spp=16),
         "top": {"type": "mesh", "vertices": top_v, "faces": top_f, "face_normals": True, "bsdf": glass},
         "bottom": {"type": "mesh", "vertices": bot_v, "faces": bot_f, "face_normals": True, "bsdf": dict(glass)},
         "floor": {"type": "mesh", "vertices": flo_v, "faces": flo_f, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": 0.2}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0, 0, 0]}},
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 10.0}}}}
    sc = on_host(S.Scene.from_dict(d, device="cpu"))
    sc.attach_alpha("floor.bsdf")
    return sc


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_an_attached_ior_changes_the_aux_words_of_dielectric_vertices_only():
    plain, glass = _slab(), _slab()
    slots = {glass.attach_ior("top.bsdf"), glass.attach_ior("bottom.bsdf")}
    assert slots == {1, 2} and glass.ior_slots == [1, 2] and glass.alpha_slots[glass.bsdf_names.index("floor.bsdf")] == 0
    assert glass.attach_ior("top.bsdf") in slots and glass.ior_slots == [1, 2]                  # attaching twice: the same slot
    assert torch.equal(glass.ior_values(), torch.tensor([INT, INT]))
    K = 4
    a = plain._trace(0, seed=4, spp=16, max_depth=6, K=K, lo=0, hi=N)
    b = glass._trace(0, seed=4, spp=16, max_depth=6, K=K, lo=0, hi=N)
    assert _same([a.ray_o, a.ray_d, a.ray_dx, a.ray_dy], [b.ray_o, b.ray_d, b.ray_dx, b.ray_dy])
    seen = {"in": 0, "out": 0, "reflected": 0}
    top_bsdf, bot_bsdf = glass.bsdf_names.index("top.bsdf"), glass.bsdf_names.index("bottom.bsdf")
    for k in range(1, K + 1):
        ra, rb = a.path_info[k], b.path_info[k]
        assert set(ra) == set(rb) and all(_same(ra[f], rb[f]) for f in ra), k
        sa, sb = a.scatter_info[k - 1], b.scatter_info[k - 1]
        for f in ("tri", "emit", "shadow"):
            assert _same(sa.get(f), sb.get(f)), (k, f)
        glassy = (rb["active"] > 0) & ((rb["bsdf"] & 0x40) != 0)
        assert torch.equal(sa["aux"][~glassy], sb["aux"][~glassy])                              # everybody else: word for word
        assert bool((sa["aux"][glassy][:, 0] == -1).all()) and bool((sa["aux"][glassy][:, 1:] == 0).all())
        aux = sb["aux"][glassy]
        tri = sb["tri"][glassy].long()
        on_top = (tri >= glass.mesh_tri_slices["top"][0]) & (tri < glass.mesh_tri_slices["top"][1])
        want_slot = torch.where(on_top, glass.alpha_slots[top_bsdf], glass.alpha_slots[bot_bsdf]).to(aux.dtype)
        assert torch.equal(aux[:, 0], want_slot)
        d = aux[:, 1:4].contiguous().view(torch.float32)
        eta = rb["eta"][glassy]
        assert bool((d[:, 1:] == 0).all())
        refl, into, out = eta == 1.0, eta > 1.0, eta < 1.0
        assert bool((d[refl, 0] == 0).all())
        assert torch.allclose(eta[into], torch.tensor(INT / EXT), rtol=1e-6) and torch.allclose(eta[out], torch.tensor(EXT / INT), rtol=1e-6)
        assert torch.allclose(d[into, 0], torch.tensor(1.0 / EXT), rtol=1e-6)
        assert torch.allclose(d[out, 0], -eta[out] / INT, rtol=1e-6)
        seen["in"] += int(into.sum()); seen["out"] += int(out.sum()); seen["reflected"] += int(refl.sum())
    assert min(seen.values()) > 20, seen


def test_without_a_slot_a_dielectric_logs_what_it_always_did():
    """No attach_ior: the dielectric vertices' aux words are [no slot, 0, 0, 0], whatever the IOR."""
    sc = _slab()
    tr = sc._trace(0, seed=4, spp=16, max_depth=6, K=3, lo=0, hi=N)
    n = 0
    for k in range(1, 4):
        glassy = (tr.path_info[k]["active"] > 0) & ((tr.path_info[k]["bsdf"] & 0x40) != 0)
        aux = tr.scatter_info[k - 1]["aux"][glassy]
        assert bool((aux[:, 0] == -1).all()) and bool((aux[:, 1:] == 0).all())
        n += int(glassy.sum())
    assert n > 100


def test_set_ior_rewrites_the_table_in_place():
    sc = _slab()
    sc.attach_ior("top.bsdf")
    buf = sc._bsdf_buf.data_ptr()
    sc.set_ior("top.bsdf", 1.7)
    assert sc._bsdf_buf.data_ptr() == buf and torch.equal(sc.ior_values(), torch.tensor([1.7]))
    tr = sc._trace(0, seed=4, spp=16, max_depth=6, K=1, lo=0, hi=N)
    into = (tr.path_info[1]["active"] > 0) & (tr.path_info[1]["eta"] > 1.0)
    assert int(into.sum()) > 100 and torch.allclose(tr.path_info[1]["eta"][into], torch.tensor(1.7 / EXT), rtol=1e-6)
    with pytest.raises(ValueError, match="int_ior == ext_ior"):
        sc.set_ior("top.bsdf", EXT)
    with pytest.raises(ValueError, match="not a dielectric"):
        sc.set_ior("floor.bsdf", 1.3)


def test_attach_ior_refusals():
    sc = _slab()
    with pytest.raises(ValueError, match="not a dielectric"):
        sc.attach_ior("floor.bsdf")
    with pytest.raises(ValueError):
        sc.attach_ior("nobody.bsdf")
    matched = _slab(int_ior=1.25, ext_ior=1.25)
    with pytest.raises(ValueError, match="int_ior == ext_ior"):
        matched.attach_ior("top.bsdf")
    assert sc.ior_slots == [] and matched.ior_slots == [] and sc.ior_values().numel() == 0


@pytest.mark.parametrize("kind", ["manifold", "manifold_caustic"])
@pytest.mark.parametrize("props", [{"fused": False}, {"fused": True, "fuse_tangent": False}], ids=["unfused stages", "precomputed tangents"])
def test_routes_that_cannot_fill_the_slot_refuse(kind, props):
    import epsm_mitsuba3_amd as epsm
    sc = _slab()
    sc.attach_ior("top.bsdf")
    integ = epsm.load_dict({"type": kind, "max_depth": 6, **props})
    params = sc.param_grads()
    grad_in = torch.zeros((8, 8, 5))
    with pytest.raises(NotImplementedError, match="attach_ior"):
        integ.render_backward(sc, params, grad_in, seed=1)
    assert float(params.flat.abs().max()) == 0.0


def test_the_option_round_trips_without_a_device():
    """include/epsm.h, EPSM_OPT_IOR_GRADS: option 5 of epsm_set_option / epsm_get_option, default 0, no environment variable;
    ``_lib.options(ior_grads=...)`` sets it for a block.  Option 4 stays unassigned."""
    from epsm_mitsuba3_amd import _lib
    lib = _lib.lib()
    assert _lib.OPT_IOR_GRADS == 5 and lib.epsm_get_option(_lib.OPT_IOR_GRADS) == 0
    with _lib.options(ior_grads=True):
        assert lib.epsm_get_option(_lib.OPT_IOR_GRADS) == 1
    assert lib.epsm_get_option(_lib.OPT_IOR_GRADS) == 0
    assert lib.epsm_set_option(_lib.OPT_IOR_GRADS, -1) == -22
    assert lib.epsm_set_option(4, 1) == -22 and lib.epsm_get_option(4) == -1 and lib.epsm_get_option(6) == -1


def test_attach_alpha_on_a_dielectric_keeps_its_slot_out_of_the_log():
    """attach_alpha takes any BSDF; a dielectric's slot must not reach the tracer, which would take it for an IOR slot and log
    d eta / d int_ior into a launch that reads it as d hf / d alpha.  The slot exists, the log names none, the words are zero."""
    sc = _slab()
    slot = sc.attach_alpha("top.bsdf")
    assert slot == 1 and sc.ior_slots == [] and sc.param_grads().alpha.numel() == 2
    tr = sc._trace(0, seed=4, spp=16, max_depth=6, K=2, lo=0, hi=N)
    n = 0
    for k in (1, 2):
        glassy = (tr.path_info[k]["active"] > 0) & ((tr.path_info[k]["bsdf"] & 0x40) != 0)
        aux = tr.scatter_info[k - 1]["aux"][glassy]
        assert bool((aux[:, 0] == -1).all()) and bool((aux[:, 1:] == 0).all())
        n += int(glassy.sum())
    assert n > 100 and not tr.ior_grads
    with pytest.raises(ValueError, match="attach_alpha"):
        sc.attach_ior("top.bsdf")
