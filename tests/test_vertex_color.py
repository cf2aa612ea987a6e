"""Per-vertex colours -- `mesh_attribute` reflectances reading a mesh's `vertex_color` (Scene.attach_vertex_color; an EpsmTexture of
kind EPSM_TEXTURE_VERTEX_RGB; a footprint of three vertices in epsm_trace_paths_texture_backward / _forward) -- on the host build
of the tracer (tests/host_harness/trace_tex_host.cpp): the loader and its refusals, the primal image, the exact transpose, finite
differences of the primal image per vertex and along a random direction, the reparameterised pass's sliding-colour term, the
gradient buffer's layout and two ranks.  The scenes: tests/_vertex_scenes.py.  The GPU twin is tests/test_gpu_vertex_color.py."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _scenes import quad, sensor
from _texture_host import on_host_texture
from _vertex_scenes import attribute, ball_mesh, grid, scene_a, scene_b, vertex_colours, vertex_plane
from epsm_mitsuba3_amd import replays
from epsm_mitsuba3_amd import scene as S
from test_texture_adjoint import floor_texture, random_tangent, transpose_gap


# ---------------------------------------------------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------------------------------------------------
def _write_ply(path, v, f, colours, names, ctype, alpha=False):
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n")
        for nm in names:
            fh.write(f"property {ctype} {nm}\n")
        if alpha:
            fh.write(f"property {ctype} alpha\n")
        fh.write(f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        for p, c in zip(v, colours):
            fh.write(" ".join(repr(float(x)) for x in p) + " " + " ".join(str(x) for x in c) + (" 255" if alpha else "") + "\n")
        for t in f:
            fh.write("3 " + " ".join(str(int(i)) for i in t) + "\n")


def test_dict_mesh_with_vertex_color_renders():
    sc = scene_a()
    assert sc.mesh("floor").vertex_color.shape == (9, 3) and sc.mesh("floor").vertex_color.dtype == np.float32
    assert sc.mesh("wall").vertex_color is None
    img = sc.render_primal(sensor=0, seed=1, spp=8, max_depth=3)
    assert bool(torch.isfinite(img).all()) and float(img.abs().sum()) > 0
    i = sc.bsdf_names.index("floor.bsdf")
    np.testing.assert_allclose(sc.bsdf_desc[i]["reflectance"], vertex_colours(9).mean(0), rtol=1e-6)    # the stand-in, as a bitmap's
    # the colours are seen: another set renders another image
    other = scene_a(colours=vertex_colours(9, seed=5)).render_primal(sensor=0, seed=1, spp=8, max_depth=3)
    assert not torch.equal(img, other)


def test_ply_vertex_colours_float_and_uchar(tmp_path):
    v, f = grid(3, 2.0)
    cf = vertex_colours(9, seed=2)
    _write_ply(tmp_path / "f.ply", v, f, [[repr(float(x)) for x in c] for c in cf], ("r", "g", "b"), "float")
    out = S.load_ply(str(tmp_path / "f.ply"), with_color=True)
    assert len(out) == 4 and out[3].dtype == np.float32
    np.testing.assert_array_equal(out[3], cf)                          # float properties as they are
    cu = np.random.default_rng(3).integers(0, 256, (9, 3))
    cu[0] = [0, 255, 10]                                               # both ends and the linear toe of the sRGB curve
    _write_ply(tmp_path / "u.ply", v, f, cu, ("red", "green", "blue"), "uchar", alpha=True)
    got = S.load_ply(str(tmp_path / "u.ply"), with_color=True)[3]
    # the inverse of optim.to_ldr's curve (linear -> sRGB: 12.92 x below 0.0031308, 1.055 x^(1/2.4) - 0.055 above), in float64
    s = cu.astype(np.float64) / 255.0
    want = np.where(s <= 12.92 * 0.0031308, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)        # (float32 of the float64 value)
    assert got[0, 0] == 0.0 and got[0, 1] == 1.0
    # the three-value return is unchanged, and a file without colours gives None
    assert len(S.load_ply(str(tmp_path / "u.ply"))) == 3
    _write_ply(tmp_path / "n.ply", v, f, [[] for _ in v], (), "float")
    assert S.load_ply(str(tmp_path / "n.ply"), with_color=True)[3] is None
    # a `ply` shape keeps the attribute
    d = {"type": "scene", "cam": sensor([0.0, -3.5, 1.6], [0, 0.5, 0.5], up=(0, 0, 1), res=8, spp=4),
         "floor": {"type": "ply", "filename": "u.ply", "face_normals": True, "bsdf": {"type": "diffuse", "reflectance": attribute()}},
         "sky": {"type": "constant"}}
    sc = on_host_texture(S.Scene.from_dict(d, device="cpu", base_dir=str(tmp_path)))
    np.testing.assert_array_equal(sc.mesh("floor").vertex_color, got)
    assert sc.attach_vertex_color("floor") == 0
    np.testing.assert_array_equal(sc.texture_values(0).numpy(), got)


def _scene_dict(**floor):
    v, f = quad(0.0, 1.0)
    base = {"type": "mesh", "vertices": v, "faces": f, "face_normals": True, "vertex_color": vertex_colours(4),
            "bsdf": {"type": "diffuse", "reflectance": attribute()}}
    base.update(floor)
    return {"type": "scene", "cam": sensor([0, 0, 4], [0, 0, 0], res=8, spp=4), "floor": base, "sky": {"type": "constant"}}


def test_refusals():
    build = lambda d: S.Scene.from_dict(d, device="cpu")
    v, f = quad(0.0, 1.0)
    # any other attribute name, face_* included
    for name in ("face_color", "vertex_albedo", "vertex_normal"):
        with pytest.raises(ValueError, match="only the attribute 'vertex_color'"):
            build(_scene_dict(bsdf={"type": "diffuse", "reflectance": {"type": "mesh_attribute", "name": name}}))
    # a shape that uses such a BSDF and has no vertex_color
    d = _scene_dict(); del d["floor"]["vertex_color"]
    with pytest.raises(ValueError, match="has no 'vertex_color' attribute"):
        build(d)
    # values that are negative or not finite, or not one colour per vertex
    bad = vertex_colours(4); bad[2, 1] = -0.1
    with pytest.raises(ValueError, match="negative"):
        build(_scene_dict(vertex_color=bad))
    bad = vertex_colours(4); bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        build(_scene_dict(vertex_color=bad))
    bad = vertex_colours(4); bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        build(_scene_dict(vertex_color=bad))
    with pytest.raises(ValueError, match=r"is not \(4, 3\)"):
        build(_scene_dict(vertex_color=vertex_colours(5)))
    with pytest.raises(ValueError, match="scale"):
        build(_scene_dict(bsdf={"type": "diffuse", "reflectance": attribute(scale=-1.0)}))
    # such a BSDF used by more than one shape
    d = _scene_dict()
    d["shared"] = {"type": "diffuse", "reflectance": attribute()}
    d["floor"]["bsdf"] = {"type": "ref", "id": "shared"}
    d["other"] = {"type": "mesh", "vertices": v + np.array([0, 0, 1.0]), "faces": f, "face_normals": True, "vertex_color": vertex_colours(4),
                  "bsdf": {"type": "ref", "id": "shared"}}
    with pytest.raises(ValueError, match="more than one shape"):
        build(d)
    # mesh_attribute anywhere but a diffuse reflectance
    with pytest.raises(ValueError, match="only the reflectance of a diffuse BSDF"):
        build(_scene_dict(bsdf={"type": "roughconductor", "alpha": attribute()}))
    with pytest.raises(ValueError, match="only the reflectance of a diffuse BSDF"):
        build(_scene_dict(bsdf={"type": "conductor", "specular_reflectance": attribute()}))
    with pytest.raises(ValueError, match="only the reflectance of a diffuse BSDF"):
        build(_scene_dict(emitter={"type": "area", "radiance": attribute()}))
    # the attach entry points
    sc = scene_a()
    with pytest.raises(ValueError, match="not a bitmap"):
        sc.attach_texture("floor.bsdf")
    with pytest.raises(ValueError, match="only the CONSTANT"):
        sc.attach_color("floor.bsdf")
    with pytest.raises(ValueError, match="does not read its vertex_color"):
        sc.attach_vertex_color("wall")
    with pytest.raises(ValueError, match="not a shape"):
        sc.attach_vertex_color("nothing")
    slot = sc.attach_vertex_color("floor")
    for bad in (np.zeros((8, 3), np.float32), np.zeros((9, 2, 3), np.float32), np.zeros((3, 3, 3), np.float32)):
        with pytest.raises(ValueError, match="shape"):
            sc.set_texture(slot, bad)
    neg = vertex_colours(9); neg[4, 0] = -1e-3
    with pytest.raises(ValueError, match="negative"):
        sc.set_texture(slot, neg)
    nan = vertex_colours(9); nan[4, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        sc.set_texture(slot, nan)


def test_twosided_and_scale():
    """Inside `twosided`, and with a scale: the table holds scale x colour, texture_values the colours before it."""
    d = _scene_dict(bsdf={"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": attribute(scale=0.5)}})
    sc = on_host_texture(S.Scene.from_dict(d, device="cpu"))
    slot = sc.attach_vertex_color("floor")
    assert sc.texture_scale(slot) == 0.5
    np.testing.assert_array_equal(sc.texture_values(slot).numpy(), vertex_colours(4))
    a = sc.render_primal(sensor=0, seed=1, spp=8, max_depth=2)
    ref = on_host_texture(S.Scene.from_dict(_scene_dict(vertex_color=vertex_colours(4) * np.float32(0.5)), device="cpu"))
    assert torch.equal(a, ref.render_primal(sensor=0, seed=1, spp=8, max_depth=2))


# ---------------------------------------------------------------------------------------------------------------------
# primal
# ---------------------------------------------------------------------------------------------------------------------
def test_equal_colours_render_as_the_constant_reflectance():
    """Nine equal colours against the same constant `rgb` reflectance.  NOT bit for bit: the kernel forms b0 = 1 - b1 - b2 and
    b0 c + b1 c + b2 c in fp32, which rounds to c only up to an ulp -- measured on the host twin: a largest difference of 2 ulp
    in a pixel -- so, as the issue allows, the assertion is 2 ulp per pixel."""
    rgb = [0.3, 0.6, 0.8]
    a = scene_a(colours=np.tile(np.array([rgb], np.float32), (9, 1))).render_primal(sensor=0, seed=2, spp=32, max_depth=3)
    b = scene_a(reflectance={"type": "rgb", "value": rgb}).render_primal(sensor=0, seed=2, spp=32, max_depth=3)
    assert float(b.abs().sum()) > 0
    ulp = (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()
    print("largest difference in ulp:", int(ulp.max()))
    assert int(ulp.max()) <= 2


def test_set_texture_renders_as_a_scene_built_from_the_array():
    new = vertex_colours(9, seed=9)
    for arr in (new, torch.from_numpy(new).reshape(9, 1, 3)):
        sc = scene_a()
        slot = sc.attach_vertex_color("floor")
        sc.set_texture(slot, arr)
        a = sc.render_primal(sensor=0, seed=2, spp=16, max_depth=3)
        b = scene_a(colours=new).render_primal(sensor=0, seed=2, spp=16, max_depth=3)
        assert torch.equal(a, b)
        assert torch.equal(sc.texture_values(slot), torch.from_numpy(new)) and tuple(sc.texture_values(slot).shape) == (9, 3)


# ---------------------------------------------------------------------------------------------------------------------
# transpose
# ---------------------------------------------------------------------------------------------------------------------
def _a(sc):
    return sc.attach_vertex_color("floor")


TRANSPOSE = {
    "scene_a": (lambda: scene_a(), "prb", lambda sc: [_a(sc)]),
    "scene_a_with_colour_slot": (lambda: scene_a(), "prb", lambda sc: [sc.attach_color("wall.bsdf"), _a(sc), sc.attach_radiance("light")]),
    "scene_b": (lambda: scene_b(), "prb", lambda sc: [sc.attach_vertex_color("ball")]),
    "prb_reparam_plane": (lambda: vertex_plane(0.0, 16, 16), "prb_reparam", lambda sc: [sc.attach("plane"), sc.attach_vertex_color("plane")]),
}


@pytest.mark.parametrize("name", list(TRANSPOSE))
def test_forward_is_the_transpose_of_backward(name):
    make, integ_name, attach = TRANSPOSE[name]
    sc = make()
    attach(sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": 3})
    gap, S_, a = transpose_gap(integ, sc, seed=5, spp=sc.sensors[0].spp, gen=torch.Generator().manual_seed(2))
    assert S_ > 0 and abs(a) > 0
    assert gap <= 1e-4 * S_, (gap, S_)                                # the texel adjoint's bound on this twin (test_texture_adjoint.py)


# ---------------------------------------------------------------------------------------------------------------------
# finite differences
# ---------------------------------------------------------------------------------------------------------------------
def _loss(integ, sc, g, seed, spp):
    return float((integ.render(sc, sensor=0, seed=seed, spp=spp) * g).double().sum())


def _fd_per_vertex(sc, slot, rows, integ, g, seed, spp, h):
    params = sc.param_grads()
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    base = sc.texture_values(slot).clone()
    rel = []
    for r in rows:
        for ch in range(3):
            out = []
            for sgn in (+1, -1):
                v = base.clone(); v[r, ch] += sgn * h
                sc.set_texture(slot, v)
                out.append(_loss(integ, sc, g, seed, spp))
            want = (out[0] - out[1]) / (2 * h)
            got = float(params.texture(slot)[r, 0, ch])
            assert abs(want) > 1e-6, (r, ch)
            rel.append(abs(got - want) / abs(want))
    sc.set_texture(slot, base)
    return np.array(rel)


def test_backward_matches_finite_differences_for_every_vertex_of_the_flat_floor():
    """Scene A's floor is flat: it never lights itself, and the radiance is a polynomial of low degree in each vertex colour
    (linear but for the paths floor - wall - floor), of which the central difference at h = 2e-2 is exact up to fp32.  All nine
    vertices and their channels: each has a triangle in view."""
    res, spp, seed, h = 12, 32, 7, 2e-2
    sc = scene_a(res=res, spp=spp)
    slot = _a(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = (0.5 + torch.rand((res, res, 3), generator=torch.Generator().manual_seed(5))).to(sc.device)
    rel = _fd_per_vertex(sc, slot, range(9), integ, g, seed, spp, h)
    print("relative errors:", rel)
    assert rel.max() < 0.02, rel                                     # test_backward_matches_finite_differences_per_texel's bound


def test_backward_matches_finite_differences_on_the_ball():
    """Scene B is curved: a colour can enter a path twice.  Ten vertices of the ball's side towards the sensor (the envmap lights
    all of it), the reference's thresholds as test_texture_adjoint.py uses them."""
    res, spp, seed, h = 16, 16, 3, 2e-2
    sc = scene_b(res=res, spp=spp)
    slot = sc.attach_vertex_color("ball")
    _, _, n = ball_mesh()
    eye = np.array([0.0, -3.5, 2.5]) - np.array([0.0, 0.0, 0.7])
    rows = np.argsort(-(n @ (eye / np.linalg.norm(eye))))[:10]
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    s = sc.sensors[0]
    g = (0.5 + torch.rand((s.height, s.width, 3), generator=torch.Generator().manual_seed(5))).to(sc.device)
    rel = _fd_per_vertex(sc, slot, [int(r) for r in rows], integ, g, seed, spp, h)
    print("relative errors:", rel)
    assert rel.mean() < 0.05 and rel.max() < 0.5, rel


def test_forward_matches_finite_differences_along_a_random_direction():
    res, spp, seed, h = 12, 32, 3, 1e-2
    sc = scene_a(res=res, spp=spp)
    slot = _a(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    gen = torch.Generator().manual_seed(4)
    t = random_tangent(sc, gen)
    g = (0.5 + torch.rand((res, res, 3), generator=gen)).to(sc.device)
    got = float((integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp) * g).double().sum())
    base = sc.texture_values(slot).clone()
    out = []
    for sgn in (+1, -1):
        sc.set_texture(slot, base + sgn * h * t.texture(slot)[:, 0])
        out.append(_loss(integ, sc, g, seed, spp))
    want = (out[0] - out[1]) / (2 * h)
    assert abs(want) > 0
    assert abs(got - want) / abs(want) < 0.02, (got, want)


# ---------------------------------------------------------------------------------------------------------------------
# the reparameterised pass: the colours slide with the plane
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half,rays,spp,tol,reparam_depth", [
    (2.0, 32, 128, 0.1, -1),    # textured_plane_constant's numbers: tests/test_render_forward.py:129 (tests/test_reparam.py:148)
    (4.0, 16, 256, 0.08, -1),   # textured_plane_fills_the_view's: tests/test_reparam.py:149 -- no silhouette in view
    # the same with the warp switched off (reparam_max_depth 0): nothing in view is discontinuous, so the derivative stays exact,
    # the rays stand still, and ALL of it is the per-vertex factor of eval_lo -- measured 182.83 against 182.88 by central
    # differences, and 0 with the factor taken out.  With the warp on, the reparameterised ray follows the plane, the barycentrics
    # it sees hardly move and the factor carries under 1 % of the two cases above (measured with a build without it: -412.866
    # against -412.872, 182.683 against 182.684): only this case fails when the factor is removed
    (4.0, 16, 256, 0.08, 0),
])
def test_reparam_forward_along_an_in_plane_translation_matches_finite_differences(half, rays, spp, tol, reparam_depth):
    res, h = 32, 1e-3 if half == 2.0 else 2e-3                        # (fd_eps of the two configs, _reparam_scenes.CONFIGS)
    props = {"type": "prb_reparam", "max_depth": 2, "reparam_rays": rays, "reparam_kappa": 1e5}
    if reparam_depth >= 0:
        props["reparam_max_depth"] = reparam_depth
    integ = epsm.load_dict(props)
    g = torch.ones((res, res, 3)) * (0.5 + torch.arange(res, dtype=torch.float32) / res)[None, :, None]
    sc = vertex_plane(0.0, res, spp, half=half)
    sc.attach("plane")
    t = sc.param_grads()
    t.mesh_pos("plane")[:] = torch.tensor([1.0, 0.0, 0.0])
    got = float((integ.render_forward(sc, t, sensor=0, seed=0, spp=spp) * g).sum())
    v = []
    for sgn in (1, -1):                                               # fd_check's recipe: 4 x the samples, common random numbers
        s2 = vertex_plane(sgn * h, res, 4 * spp, half=half)
        v.append(float((integ.render(s2, sensor=0, seed=100, spp=4 * spp) * g).double().sum()))
    fd = (v[0] - v[1]) / (2 * h)
    print("forward", got, "central differences", fd)
    assert got * fd > 0 and abs(got - fd) <= tol * abs(fd), (got, fd)


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
def test_param_grads_layout_without_and_with_a_vertex_slot():
    sc = scene_a()
    sc.attach_color("wall.bsdf")
    before = sc.param_grads()
    n0 = 6 * before.V + before.B + 3 + 3 * before.C
    assert before.flat.numel() == n0 and before.tex_shapes == []
    assert _a(sc) == 0 and _a(sc) == 0
    assert before.flat.numel() == n0                                  # a buffer built before the attach keeps its size
    after = sc.param_grads()
    assert after.tex_shapes == [(9, 1)] and sc.texture_shapes() == [(9, 1)]
    assert after.flat.numel() == n0 + 27
    assert after.color.data_ptr() - after.flat.data_ptr() == before.color.data_ptr() - before.flat.data_ptr()
    assert after.texture(0).data_ptr() == after.flat[n0:].data_ptr() and tuple(after.texture(0).shape) == (9, 1, 3)
    assert after.scratch().tex_shapes == after.tex_shapes
    assert replays.TEXTURE.attached(sc) and not replays.ALPHA_TEXTURE.attached(sc)


def test_a_bitmap_slot_and_a_vertex_slot_fill_together():
    """A bitmap wall behind the per-vertex floor: one call fills both sections, each as it fills alone."""
    make = lambda: scene_a(wall_reflectance={"type": "bitmap", "bitmap": floor_texture(seed=4)})      # (no uv on the wall: (b1, b2))
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
    both = make()
    assert both.attach_texture("wall.bsdf") == 0 and both.attach_vertex_color("floor") == 1
    p = both.param_grads()
    assert p.tex_shapes == [(4, 4), (9, 1)]
    integ.render_backward(both, p, g, sensor=0, seed=4, spp=32)
    assert float(p.texture(0).abs().sum()) > 0 and float(p.texture(1).abs().sum()) > 0
    for k, attach in ((0, lambda sc: sc.attach_texture("wall.bsdf")), (1, lambda sc: sc.attach_vertex_color("floor"))):
        alone = make()
        attach(alone)
        q = alone.param_grads()
        integ.render_backward(alone, q, g, sensor=0, seed=4, spp=32)
        want = p.texture(k).numpy()                                  # (the adds of a section come in any order: the two-rank bound)
        np.testing.assert_allclose(q.texture(0).numpy(), want, rtol=1e-4, atol=1e-6 * float(np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def _two_rank_case():
    sc = scene_a()
    sc.tile_paths = 1000                                               # several tiles, dealt over the ranks
    sc.attach_color("wall.bsdf"); _a(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    p = sc.param_grads()
    g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
    integ.render_backward(sc, p, g, sensor=0, seed=4, spp=32)
    return p


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _two_rank_case().flat.clone().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_vertex_gradients_match_single_process():
    p = _two_rank_case()
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
    assert float(np.abs(p.texture(0).numpy()).sum()) > 0
    for r in range(2):                                                # test_two_rank_texel_gradients_match_single_process's bound
        np.testing.assert_allclose(got[r], want, rtol=1e-4, atol=1e-6 * float(np.abs(want).max()))
