"""The texel adjoint (Scene.attach_texture, epsm_trace_paths_texture_backward / _forward) on the host build of the tracer
(tests/host_harness/trace_tex_host.cpp): the exact transpose of the backward pass (dot-product test under the same random
numbers), finite differences of the primal image for individual texels and along a random texel direction, the refusals,
the gradient buffer's layout, set_texture, and two ranks.  The GPU twin is tests/test_gpu_texture_adjoint.py."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _reparam_scenes import build as build_reparam
from _scenes import quad, sensor
from _texture_host import on_host_texture
from epsm_mitsuba3_amd import scene as S


def floor_texture(h=4, w=4, seed=0):
    return (0.2 + 0.7 * np.random.default_rng(seed).random((h, w, 3))).astype(np.float32)


def env_bitmap(h=8, w=16, seed=1):
    rng = np.random.default_rng(seed)
    sky = 0.3 + 1.5 * rng.random((h, w, 3))
    sky[: h // 3] *= 3.0                                               # a brighter band: something for the emitter samples
    return sky.astype(np.float32)


def texture_scene(device="cpu", res=12, spp=32, tex=None, nearest=False, env=None, env_scale=1.0, light=True, wall_colour=(0.2, 0.5, 0.7)):
    """A floor whose reflectance is a bitmap (uv over [0, 1]^2), a wall behind it, an area light and / or an envmap."""
    fv, ff = quad(0.0, 2.0, up=True)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    wv = np.array([[-2, 2, 0], [2, 2, 0], [2, 2, 2.5], [-2, 2, 2.5]], float)
    wf = np.array([[0, 2, 1], [0, 3, 2]])
    refl = {"type": "bitmap", "bitmap": floor_texture() if tex is None else tex, "filter_type": "nearest" if nearest else "bilinear"}
    d = {"type": "scene", "cam": sensor([0.0, -3.5, 1.6], [0, 0.5, 0.5], up=(0, 0, 1), res=res, spp=spp, rfilter="gaussian"),
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "texcoords": uv, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": refl}},
         "wall": {"type": "mesh", "vertices": wv, "faces": wf, "face_normals": True,
                  "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": list(wall_colour)}}}}}
    if light:
        lv, lf = quad(2.2, 0.4, up=False)
        d["light"] = {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [30.0, 25.0, 20.0]}}}
    if env is not None:
        d["sky"] = {"type": "envmap", "bitmap": env, "scale": env_scale, "to_world": S.rotate([0.3, 1.0, 0.2], 40.0)}
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_texture(sc)
    sc.tracer = "mega"
    return sc


def random_tangent(sc, gen, colour=True, geometry=True):
    t = sc.param_grads()
    for k in range(len(sc.texture_slots)):
        t.texture(k)[:] = torch.randn(tuple(t.texture(k).shape), generator=gen).to(sc.device)
    if colour and t.C:
        t.color[:] = torch.randn((t.C, 3), generator=gen).to(sc.device)
    if geometry:
        for m in sc.meshes:
            if getattr(m, "pos_attached", False):
                lo, hi = t.mesh_slices[m.name]
                t.pos[lo:hi] = torch.randn((hi - lo, 3), generator=gen).to(sc.device)
    return t


def transpose_gap(integ, sc, seed, spp, gen):
    """(|a - b|, S, a): a = sum g * J t, b = sum J^T g * t, S = sum |g * J t| + sum |J^T g * t|."""
    s = sc.sensors[0]
    t = random_tangent(sc, gen)
    g = torch.randn((s.height, s.width, 3), generator=gen).to(sc.device)
    fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp)
    params = sc.param_grads()
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    a = float((g * fwd).double().sum())
    b = float((params.flat * t.flat).double().sum())
    S_ = float((g * fwd).abs().double().sum()) + float((params.flat * t.flat).abs().double().sum())
    return abs(a - b), S_, a


def _floor(sc):
    return sc.attach_texture("floor.bsdf.reflectance.data")


def _env(sc):
    return sc.attach_texture("sky.data")


TRANSPOSE = {
    "bilinear": (lambda: texture_scene(), "prb", lambda sc: [_floor(sc)]),
    "nearest": (lambda: texture_scene(nearest=True), "prb", lambda sc: [_floor(sc)]),
    "envmap": (lambda: texture_scene(env=env_bitmap(), env_scale=0.7, light=False), "prb", lambda sc: [_env(sc)]),
    "bitmap_and_envmap": (lambda: texture_scene(env=env_bitmap()), "prb", lambda sc: [_floor(sc), _env(sc)]),
    "with_colour_slot": (lambda: texture_scene(env=env_bitmap()), "prb",
                         lambda sc: [sc.attach_color("wall.bsdf"), _floor(sc), sc.attach_radiance("light"), _env(sc)]),
    "prb_reparam_geometry": (lambda: on_host_texture(build_reparam("textured_plane_constant", 0.0, 16, 16)), "prb_reparam",
                             lambda sc: [sc.attach("plane"), sc.attach_texture("plane.bsdf")]),
    "prb_reparam_envmap": (lambda: on_host_texture(build_reparam("diffuse_sphere_envmap", 0.0, 16, 16)), "prb_reparam",
                           lambda sc: [sc.attach("sphere"), sc.attach_texture("light")]),
}


@pytest.mark.parametrize("name", list(TRANSPOSE))
def test_forward_is_the_transpose_of_backward(name):
    make, integ_name, attach = TRANSPOSE[name]
    sc = make()
    attach(sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": 3})
    gap, S_, a = transpose_gap(integ, sc, seed=5, spp=sc.sensors[0].spp, gen=torch.Generator().manual_seed(2))
    assert S_ > 0 and abs(a) > 0
    assert gap <= 1e-4 * S_, (gap, S_)


def _set_detached(sc, slot, arr):
    """set_texture with the envmap's sampling tables kept as they were: the derivative detaches them (envmap.cpp builds its warp
    from detached data), so the finite differences that check it must not move the samples either."""
    tables = [t.clone() for t in sc._env_buf[1:]] if sc.texture_slots[slot][0] == "envmap" else []
    sc.set_texture(slot, arr)
    for dst, src in zip(sc._env_buf[1:], tables):
        dst.copy_(src)


def _loss(integ, sc, g, seed, spp):
    return float((integ.render(sc, sensor=0, seed=seed, spp=spp) * g).double().sum())


def test_forward_matches_finite_differences_along_a_random_texel_direction():
    res, spp, seed, h = 10, 32, 3, 1e-2
    sc = texture_scene(res=res, spp=spp, env=env_bitmap())
    slots = [_floor(sc), _env(sc)]
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    gen = torch.Generator().manual_seed(4)
    t = random_tangent(sc, gen)
    g = (0.5 + torch.rand((res, res, 3), generator=gen)).to(sc.device)
    got = float((integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp) * g).double().sum())
    base = [sc.texture_values(k).clone() for k in slots]
    out = []
    for sgn in (+1, -1):
        for k in slots:
            _set_detached(sc, k, base[k] + sgn * h * t.texture(k))
        out.append(_loss(integ, sc, g, seed, spp))
    for k in slots:
        sc.set_texture(k, base[k])
    want = (out[0] - out[1]) / (2 * h)
    assert abs(want) > 0
    assert abs(got - want) / abs(want) < 0.02, (got, want)


# (slot, (row, column) of the texel): the floor's, and the envmap's in its wrap columns 0 and W - 1
FD_TEXELS = [(0, (1, 2)), (0, (3, 0)), (1, (2, 0)), (1, (2, 15)), (1, (1, 7))]


def test_backward_matches_finite_differences_per_texel():
    res, spp, seed, h = 10, 64, 7, 2e-2
    sc = texture_scene(res=res, spp=spp, env=env_bitmap(), env_scale=0.8)
    slots = [_floor(sc), _env(sc)]
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = (0.5 + torch.rand((res, res, 3), generator=torch.Generator().manual_seed(5))).to(sc.device)
    params = sc.param_grads()
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    rel = []
    for k, (r, c) in FD_TEXELS:
        base = sc.texture_values(slots[k]).clone()
        for ch in range(3):
            out = []
            for sgn in (+1, -1):
                v = base.clone(); v[r, c, ch] += sgn * h
                _set_detached(sc, slots[k], v)
                out.append(_loss(integ, sc, g, seed, spp))
            want = (out[0] - out[1]) / (2 * h)
            got = float(params.texture(slots[k])[r, c, ch])
            assert abs(want) > 1e-6, (k, r, c, ch)
            rel.append(abs(got - want) / abs(want))
        sc.set_texture(slots[k], base)
    rel = np.array(rel)
    assert rel.mean() < 0.05 and rel.max() < 0.5, rel               # the reference's thresholds (test_color_adjoint.py)
    assert rel.max() < 0.02, rel                                     # the radiance is linear in each texel: FD is exact up to fp32


def test_refusals():
    sc = texture_scene(env=None)
    with pytest.raises(ValueError, match="not a bitmap"):
        sc.attach_texture("wall.bsdf")
    with pytest.raises(ValueError, match="neither a BSDF nor an emitter"):
        sc.attach_texture("sky.data")                                 # no envmap in this scene
    with pytest.raises(ValueError, match="not an envmap"):
        sc.attach_texture("light")                                    # an area light
    with pytest.raises(ValueError, match="only the CONSTANT"):
        sc.attach_color("floor.bsdf")                                 # unchanged
    v, f = quad(0.0, 1.0)
    d = {"type": "scene", "cam": sensor([0, 0, 4], [0, 0, 0], res=8, spp=4),
         "plate": {"type": "mesh", "vertices": v, "faces": f, "texcoords": v[:, :2],
                   "bsdf": {"type": "roughconductor", "alpha": 0.2}},
         "sky": {"type": "constant"}}
    sc2 = on_host_texture(S.Scene.from_dict(d, device="cpu"))
    with pytest.raises(ValueError, match="not a diffuse BSDF"):
        sc2.attach_texture("plate.bsdf")
    with pytest.raises(ValueError, match="`constant` environment"):
        sc2.attach_texture("sky")
    sc3 = texture_scene(env=env_bitmap(), light=False)
    with pytest.raises(ValueError, match="envmap's radiance is its bitmap"):
        sc3.attach_radiance(0)                                        # unchanged
    slot = _env(sc3)
    with pytest.raises(ValueError, match="shape"):
        sc3.set_texture(slot, np.zeros((4, 4, 3), np.float32))


def test_param_grads_layout_without_and_with_textures():
    sc = texture_scene(env=env_bitmap())
    sc.attach_color("wall.bsdf")
    before = sc.param_grads()
    n0 = 6 * before.V + before.B + 3 + 3 * before.C
    assert before.flat.numel() == n0 and before.tex_shapes == []
    assert before.color.data_ptr() == before.flat[6 * before.V + before.B + 3:].data_ptr()
    assert _floor(sc) == 0 and _env(sc) == 1 and _floor(sc) == 0
    after = sc.param_grads()
    assert after.tex_shapes == [(4, 4), (8, 16)]
    assert after.flat.numel() == n0 + 3 * (16 + 128)
    assert after.color.shape == before.color.shape
    assert after.color.data_ptr() - after.flat.data_ptr() == before.color.data_ptr() - before.flat.data_ptr()
    assert after.texture(0).data_ptr() == after.flat[n0:].data_ptr() and tuple(after.texture(1).shape) == (8, 16, 3)
    assert after.scratch().tex_shapes == after.tex_shapes


def test_set_texture_renders_as_a_scene_built_from_the_array():
    new_tex, new_env = floor_texture(seed=9), env_bitmap(seed=11)
    sc = texture_scene(env=env_bitmap(), env_scale=0.6)
    sc.set_texture(_floor(sc), new_tex)
    sc.set_texture(_env(sc), new_env)
    ref = texture_scene(tex=new_tex, env=new_env, env_scale=0.6)
    a = sc.render_primal(sensor=0, seed=2, spp=16, max_depth=3)
    b = ref.render_primal(sensor=0, seed=2, spp=16, max_depth=3)
    assert torch.equal(a, b)
    assert torch.allclose(sc.texture_values(1).cpu(), torch.from_numpy(new_env), rtol=1e-6)      # (before the scale, up to its rounding)


def test_textures_alone_count_as_attached_and_prb_still_refuses_bare_geometry():
    sc = texture_scene()
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    sc.attach("floor")
    with pytest.raises(NotImplementedError, match="prb: geometry is attached but no colour parameter is"):
        integ.render_backward(sc, sc.param_grads(), torch.ones((12, 12, 3)), seed=1, spp=4)
    _floor(sc)
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((12, 12, 3)), seed=1, spp=4)
    assert float(p.texture(0).abs().sum()) > 0 and float(p.pos.abs().sum()) == 0


def _free_port():
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc = texture_scene(env=env_bitmap())
        sc.tile_paths = 1000                                           # several tiles, dealt over the ranks
        _floor(sc); _env(sc)
        integ = epsm.load_dict({"type": "prb", "max_depth": 3})
        p = sc.param_grads()
        g = (0.5 + torch.rand((12, 12, 3), generator=torch.Generator().manual_seed(3)))
        integ.render_backward(sc, p, g, sensor=0, seed=4, spp=32)
        q.put((rank, p.flat.clone().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_texel_gradients_match_single_process():
    sc = texture_scene(env=env_bitmap())
    sc.tile_paths = 1000
    _floor(sc); _env(sc)
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
