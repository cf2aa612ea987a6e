"""The envmap pose adjoint of the colour pass (Scene.attach_envmap_pose with prb / prb_reparam / a 3-channel gradient image;
epsm_trace_paths_envpose_backward / _forward) on the host build of the tracer (tests/host_harness/trace_envpose_host.cpp).
The yardstick is independent of the per-path code: the items (coefficient, world direction) the observer forms are exported by
the host twin, and the envmap lookup is restated here in float64 numpy from the header comment of EpsmEnvironment
(include/epsm_trace.h) -- F(R', s') = sum_items coef L64(R' d) s' / s.  The GPU twin is tests/test_gpu_envpose_adjoint.py."""
import ctypes as C
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _envpose_host import host_envpose_tracer, on_host_envpose
from _scenes import quad, sensor
from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd.film import develop_tangent, film_splat_tangent_torch
from epsm_mitsuba3_amd.params import ParamGrads

RES, SPP = 16, 4
N_PATHS = (RES + 4) * (RES + 4) * SPP            # gaussian filter with border: 1600 paths
MAPS = {"4x3": (4, 3), "16x8": (16, 8)}          # (W, H); 4 x 3 is the smallest with both pole rows and the seam
ITEM_CAP = 16                                    # at most 2 items per bounce, 6 bounces


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def rot(w):
    """Rot(w): the right-handed rotation about w by |w| (Rodrigues), float64."""
    w = np.asarray(w, np.float64)
    a = float(np.linalg.norm(w))
    if a == 0.0:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


R0 = rot([0.3, -0.5, 0.4])                       # the envmaps' to_world: no axis of the map along a world axis
SCALE0 = 1.7


def local_dirs(W, H):
    """(H, W, 3) directions of the texels in the emitter's frame (EpsmEnvironment's header comment)."""
    phi = 2 * np.pi * (np.arange(W) + 0.5) / W
    theta = np.pi * np.arange(H) / (H - 1)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    return np.stack([np.sin(phi)[None] * st, ct * np.ones((1, W)), -np.cos(phi)[None] * st], -1)


def smooth_map(W, H):
    """(H, W, 3) float32: a smooth positive function of the direction (so the pole rows are constant), one per channel."""
    l = local_dirs(W, H)
    out = []
    for a, b in (([0.6, 0.3, -0.2], [0.2, 0.7, 0.5]), ([-0.3, 0.5, 0.4], [0.6, -0.2, 0.6]), ([0.1, -0.4, 0.7], [-0.5, 0.5, 0.3])):
        out.append(1.0 + 0.6 * (l @ np.array(a)) + 0.5 * (l @ np.array(b)) ** 2)
    return np.stack(out, -1).astype(np.float32)


def env_scene(kind, size="4x3", device="cpu", res=RES, spp=SPP, to_world=None, bitmap=None, scale=SCALE0, cam=None, extra=None):
    """Envmap-only-lit scenes: "floor" a diffuse floor under an occluder, "ball" a roughconductor ball on a diffuse floor,
    "mirror" a `conductor` quad and the background (nothing smooth), "pole" the floor seen by a sensor that looks along the
    map's polar axis.  16 x 16 @ 4 spp, gaussian filter with border.  ``extra``: further entries of the scene dict."""
    W, H = MAPS[size]
    R = R0 if to_world is None else to_world
    tw = np.eye(4); tw[:3, :3] = R
    d = {"type": "scene",
         "sky": {"type": "envmap", "bitmap": smooth_map(W, H) if bitmap is None else bitmap, "scale": scale, "to_world": tw}}
    origin, target = [0.0, -3.5, 2.5], [0.0, 0.0, 0.3]
    fv, ff = quad(0.0, 2.0, up=True)
    diffuse = lambda rgb: {"type": "diffuse", "reflectance": {"type": "rgb", "value": rgb}}
    if kind in ("floor", "pole"):
        ov, of = quad(0.7, 0.5, up=True)
        d["floor"] = {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True, "bsdf": diffuse([0.6, 0.5, 0.4])}
        d["occluder"] = {"type": "mesh", "vertices": ov + np.array([0.3, 0.2, 0.0]), "faces": of, "face_normals": True,
                         "bsdf": {"type": "twosided", "bsdf": diffuse([0.3, 0.5, 0.7])}}
        if kind == "pole":
            axis = R @ np.array([0.0, 1.0, 0.0])
            origin = np.array([0.0, 0.0, 1.5])
            target = origin + axis
    elif kind == "ball":
        from epsm_mitsuba3_amd.exp.clutter import icosphere
        bv, bf = icosphere(1)
        d["floor"] = {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True, "bsdf": diffuse([0.6, 0.5, 0.4])}
        d["ball"] = {"type": "mesh", "vertices": bv * 0.7 + np.array([0.0, 0.0, 0.7]), "faces": bf, "face_normals": False,
                     "bsdf": {"type": "roughconductor", "material": "Cu", "distribution": "ggx", "alpha": 0.3}}
    elif kind == "mirror":
        mv, mf = quad(0.0, 1.5, up=True)
        d["plate"] = {"type": "mesh", "vertices": mv, "faces": mf, "face_normals": True, "bsdf": {"type": "conductor", "material": "Cu"}}
    else:
        raise ValueError(kind)
    up = (0, 0, 1) if kind != "pole" else (1, 0, 0)
    d["cam"] = cam or sensor(origin, target, up=up, res=res, spp=spp, rfilter="gaussian", sample_border=True)
    d.update(extra or {})
    sc = S.Scene.from_dict(d, device=device)
    if str(device) == "cpu":
        on_host_envpose(sc)
    sc.tracer = "mega"
    return sc


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick: the envmap lookup in float64, from the header comment of EpsmEnvironment
# ---------------------------------------------------------------------------------------------------------------------
def lookup64(texels, v, grad=False):
    """texels (H, W, 3) (bitmap x scale, the float32 numbers the device holds) along the unit directions v (n,3) of the emitter's
    frame: texel (i, j) sits at phi = 2 pi (i + 1/2) / W, theta = pi j / (H - 1), direction (sin phi sin theta, cos theta,
    -cos phi sin theta); bilinear in between, column W = column 0.  Returns L (n,3) and, with ``grad``, d L / d v (n,3 channels,3)."""
    t = np.asarray(texels, np.float64)
    H, W = t.shape[:2]
    v = np.asarray(v, np.float64)
    x = (np.arctan2(v[:, 0], -v[:, 2]) / (2 * np.pi) - 0.5 / W) % 1.0 * W
    y = np.arccos(np.clip(v[:, 1], -1.0, 1.0)) / np.pi * (H - 1)
    i = np.minimum(np.floor(x).astype(int), W - 1)
    j = np.minimum(np.floor(y).astype(int), H - 2)
    fx, fy = (x - i)[:, None], (y - j)[:, None]
    i1 = (i + 1) % W
    a, b, c, e = t[j, i], t[j, i1], t[j + 1, i], t[j + 1, i1]
    L = a * (1 - fx) * (1 - fy) + b * fx * (1 - fy) + c * (1 - fx) * fy + e * fx * fy
    if not grad:
        return L
    Lx = (b - a) * (1 - fy) + (e - c) * fy
    Ly = (c - a) * (1 - fx) + (e - b) * fx
    r2 = v[:, 0] ** 2 + v[:, 2] ** 2
    dx = np.stack([-v[:, 2] / r2, np.zeros_like(r2), v[:, 0] / r2], -1) * (W / (2 * np.pi))          # d x / d v
    dy = np.stack([np.zeros_like(r2), -1.0 / np.sqrt(r2), np.zeros_like(r2)], -1) * ((H - 1) / np.pi)
    return L, Lx[:, :, None] * dx[:, None, :] + Ly[:, :, None] * dy[:, None, :]


class Items:
    """The items of a tile of paths (the host twin's test-only export) and the yardstick on them."""

    def __init__(self, sc, depth, seed, lo=0, hi=N_PATHS, spp=SPP):
        self.sc, n = sc, hi - lo
        self.film_pos, self.radiance, _ = sc.trace_color(0, seed, spp, depth, lo, hi)
        lib = host_envpose_tracer()
        items = np.zeros((n, ITEM_CAP, 6), np.float32)
        count = np.zeros(n, np.int32)
        cs = sc.sensors[0].c_struct()
        lib.epsm_test_envpose_items.restype = C.c_int
        rc = lib.epsm_test_envpose_items(C.byref(sc.c_scene), C.byref(cs), C.c_uint32(seed), spp, depth, sc.rr_depth, C.c_int64(lo),
                                         C.c_int64(n), C.c_void_p(self.radiance.data_ptr()), ITEM_CAP,
                                         items.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p))
        assert rc == 0 and int(count.max()) <= ITEM_CAP
        self.n = n
        live = np.arange(ITEM_CAP)[None, :] < count[:, None]
        self.path = np.nonzero(live)[0]                                  # the path of every item
        self.coef = items[live][:, :3].astype(np.float64)
        self.d = items[live][:, 3:].astype(np.float64)
        self.d /= np.linalg.norm(self.d, axis=1, keepdims=True)
        self.R, self.scale = sc.envmap_pose()
        e = sc.emitter_desc[sc._envmap_index("test")]
        self.texels = np.asarray(e["bitmap"], np.float32)                # bitmap x scale

    def _sum(self, per_item):
        out = np.zeros((self.n, 3))
        np.add.at(out, self.path, per_item)
        return out

    def F(self, omega=(0, 0, 0), lnscale=0.0):
        """(n,3): sum_items coef L64(to_local' d) s' / s at to_world' = Rot(omega) to_world, s' = s exp(lnscale)."""
        Rw = rot(omega) @ self.R
        return self._sum(self.coef * lookup64(self.texels, self.d @ Rw) * np.exp(lnscale))

    def dF(self, tangent):
        """(n,3): the analytic derivative of F along tangent = [omega, ln(scale)] at the scene's own pose."""
        L, g = lookup64(self.texels, self.d @ self.R, grad=True)
        gw = g @ self.R.T                                                # world-direction gradient, (m, 3 channels, 3)
        torque = np.cross(gw, self.d[:, None, :])                        # g_c x d
        t = np.asarray(tangent, np.float64)
        return self._sum(self.coef * (torque @ t[:3] + L * t[3]))

    def fd(self, tangent, h):
        t = np.asarray(tangent, np.float64)
        return (self.F(h * t[:3], h * t[3]) - self.F(-h * t[:3], -h * t[3])) / (2 * h)

    def sin_theta(self):
        """|sin theta| of every item's direction in the emitter's frame, float64."""
        v = self.d @ self.R
        return np.sqrt(v[:, 0] ** 2 + v[:, 2] ** 2)


def l1_rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).sum() / np.abs(want).sum())


def forward(sc, it, depth, seed, tangent, lo=0, hi=N_PATHS):
    t = torch.tensor(np.asarray(tangent, np.float32), device=sc.device)
    return sc.trace_envpose_forward(0, seed, SPP, depth, lo, hi, it.radiance.contiguous(), t).cpu().numpy()


TANGENTS = {"e_x": [1, 0, 0, 0], "e_y": [0, 1, 0, 0], "e_z": [0, 0, 1, 0], "ln s": [0, 0, 0, 1], "oblique": [0.4, -0.7, 0.5, 0.8]}
KINDS = ["floor", "ball", "mirror"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. completeness, 2. closed form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sorted(MAPS))
@pytest.mark.parametrize("kind", KINDS)
def test_items_reproduce_the_path_radiance(kind, size):
    """The scenes are lit by the envmap alone, so F at the scene's own pose IS the path radiance: float32 sums of at most 12
    positive terms -- a missing item fails by orders of magnitude.  L1-relative <= 1e-4."""
    sc = env_scene(kind, size)
    sc.attach_envmap_pose()
    it = Items(sc, 4, seed=3)
    want = it.radiance.numpy().astype(np.float64)
    gap = l1_rel(it.F(), want)
    print(f"{kind} {size}: {len(it.path)} items on {it.n} paths, |F - radiance|_1 / |radiance|_1 = {gap:.3e}")
    assert np.abs(want).sum() > 0 and len(it.path) >= it.n // 2
    assert gap <= 1e-4


@pytest.mark.parametrize("size", sorted(MAPS))
@pytest.mark.parametrize("kind", KINDS)
def test_forward_matches_float64_differences_of_the_yardstick(kind, size):
    """d_radiance for the unit tangents and an oblique one against central differences of F in float64 at step 1e-6 (kinks and
    truncation negligible), every path counted: L1-relative <= 1e-3, the bound of this project's twin comparisons -- float32
    closed forms sit two orders inside."""
    sc = env_scene(kind, size)
    sc.attach_envmap_pose()
    it = Items(sc, 4, seed=3)
    for name, t in TANGENTS.items():
        got = forward(sc, it, 4, 3, t)
        want = it.fd(t, 1e-6)
        assert got.shape == want.shape == (N_PATHS, 3) and np.isfinite(got).all()
        gap = l1_rel(got, want)
        print(f"{kind} {size} {name}: |fwd - FD64|_1 / |FD64|_1 = {gap:.3e}  (analytic64: {l1_rel(it.dF(t), want):.3e})")
        assert np.abs(want).sum() > 0
        assert gap <= 1e-3, (name, gap)


# ---------------------------------------------------------------------------------------------------------------------
# 3. transpose
# ---------------------------------------------------------------------------------------------------------------------
def transpose_gap(integ, sc, seed, spp, gen):
    """(|a - b|, S, a, params): a = sum g * J t, b = sum J^T g * t, S = sum |g * J t| + sum |J^T g * t|."""
    s = sc.sensors[0]
    t = sc.param_grads()
    t.env_pose[:] = torch.randn(4, generator=gen).to(sc.device)
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


TRANSPOSE = {"prb": lambda sc: None, "prb_reparam": lambda sc: sc.attach("occluder"), "manifold": lambda sc: None}


@pytest.mark.parametrize("integ_name", list(TRANSPOSE))
@pytest.mark.parametrize("depth", [2, 4])
def test_forward_is_the_transpose_of_backward(integ_name, depth):
    sc = env_scene("floor", "16x8")
    sc.attach_envmap_pose()
    TRANSPOSE[integ_name](sc)
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params = transpose_gap(integ, sc, seed=5, spp=SPP, gen=torch.Generator().manual_seed(2 + depth))
    assert float(params.env_pose.abs().min()) > 0                       # all four numbers live
    assert S_ > 0 and abs(a) > 0
    print(f"{integ_name} depth {depth}: transpose gap {gap / S_:.3e}")
    assert gap <= 1e-4 * S_, (gap, S_)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the mirror scene through the public API
# ---------------------------------------------------------------------------------------------------------------------
def _image_of(sc, it, values):
    """The image of per-path values under the primal film weights: sum_i w_ip v_i / W_p (the film's tangent map)."""
    s = sc.sensors[0]
    accum = torch.zeros((s.height, s.width, 4), dtype=torch.float32)
    sc.film_splat(accum, s, it.film_pos, it.radiance)
    d = film_splat_tangent_torch(it.film_pos, it.radiance, torch.tensor(values, dtype=torch.float32), None, s.height, s.width, s.rfilter)
    return develop_tangent(accum, d.view(s.height, s.width, 4)).double().numpy()


def test_mirror_scene_forward_equals_finite_differences_of_render():
    """`conductor` quad + background: prev_bsdf_delta makes mis = 1 and no emitter sample contributes, so nothing samples the
    map and a one-seed central difference of render() at h = 1e-2 rad differentiates the very estimator render_forward does.
    Bound: 1e-3 + g64, g64 the same difference's own error on the float64 yardstick (its gap to F's analytic derivative, both
    carried through the primal film weights): the bilinear map's kinks and the h^2 term.  Measured here in numpy on the 4 x 3
    map: g64 = 1.3e-3 (e_x), 3.3e-3 (e_y), 3.2e-3 (e_z), 1.7e-5 (ln s), 5.3e-4 (oblique) of |d image|_1, printed below (MEASUREMENTS.md); float32 noise,
    2^-23 / h ~ 1e-5, is inside the 1e-3."""
    h, seed = 1e-2, 7
    sc = env_scene("mirror", "4x3")
    sc.attach_envmap_pose()
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    it = Items(sc, 3, seed=seed)
    R, s0 = sc.envmap_pose()
    for name, tan in TANGENTS.items():
        tan = np.asarray(tan, np.float64)
        g64 = float(np.abs(_image_of(sc, it, it.fd(tan, h)) - _image_of(sc, it, it.dF(tan))).sum()
                    / np.abs(_image_of(sc, it, it.dF(tan))).sum())
        t = sc.param_grads()
        t.env_rotation[:] = torch.tensor(tan[:3], dtype=torch.float32)
        t.env_scale[0] = float(tan[3] * s0)                               # d scale = scale d ln(scale)
        fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=SPP).double().numpy()
        out = []
        for sgn in (+1, -1):
            sc.set_envmap_pose(rotation=rot(sgn * h * tan[:3]) @ R, scale=s0 * np.exp(sgn * h * tan[3]))
            out.append(integ.render(sc, sensor=0, seed=seed, spp=SPP).double().numpy())
        sc.set_envmap_pose(rotation=R, scale=s0)
        fd = (out[0] - out[1]) / (2 * h)
        gap = float(np.abs(fwd - fd).sum() / np.abs(fd).sum())
        print(f"mirror {name}: |fwd - FD|_1 / |FD|_1 = {gap:.3e}, g64 = {g64:.3e}")
        assert np.abs(fd).sum() > 0
        assert gap <= 1e-3 + g64, (name, gap, g64)
    # render_backward on the same scene is that forward's transpose
    gap, S_, a, _ = transpose_gap(integ, sc, seed=seed, spp=SPP, gen=torch.Generator().manual_seed(1))
    assert S_ > 0 and abs(a) > 0 and gap <= 1e-4 * S_, (gap, S_)


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 9. bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def _grad_image(res=RES):
    return 0.5 + torch.rand((res, res, 3), generator=torch.Generator().manual_seed(3))


@pytest.mark.parametrize("kind", ["floor", "ball"])
def test_scale_gradient_equals_the_texel_gradient_summed(kind):
    """The same coefficients along two routes: d / d scale = sum_texels d / d bitmap x bitmap / scale.  1e-4 relative."""
    sc = env_scene(kind, "16x8")
    slot = sc.attach_texture("sky")
    sc.attach_envmap_pose()
    integ = epsm.load_dict({"type": "prb", "max_depth": 4})
    p = sc.param_grads()
    integ.render_backward(sc, p, _grad_image(), sensor=0, seed=4, spp=SPP)
    scale = sc.envmap_pose()[1]
    want = float((p.texture(slot).double() * sc.texture_values(slot).double()).sum()) / scale
    got = float(p.env_scale[0])
    print(f"{kind}: env_scale {got:.6e}, texel route {want:.6e}")
    assert want != 0 and abs(got - want) <= 1e-4 * abs(want)


def test_param_grads_without_env_pose_keeps_its_layout():
    old = ParamGrads(10, 2, device="cpu", n_colors=1, tex_shapes=[(2, 3)], n_rigid=1, cam_rotation=True, n_conductors=2)
    assert old.env_pose is None and old.env_rotation is None and old.env_scale is None
    assert old.flat.numel() == 60 + 2 + 3 + 3 + 18 + 6 + 3 + 18
    new = ParamGrads(10, 2, device="cpu", n_colors=1, tex_shapes=[(2, 3)], n_rigid=1, cam_rotation=True, n_conductors=2, env_pose=True)
    assert new.flat.numel() == old.flat.numel() + 4
    assert tuple(new.env_rotation.shape) == (3,) and tuple(new.env_scale.shape) == (1,)
    new.flat[:] = torch.arange(new.flat.numel(), dtype=torch.float32)
    assert float(new.env_rotation[0]) == old.flat.numel() and float(new.env_scale[0]) == new.flat.numel() - 1      # the very end
    assert float(new.conductor[1, 2, 2]) == old.flat.numel() - 1
    for a, b in ((old.pos, new.pos), (old.nrm, new.nrm), (old.alpha, new.alpha), (old.cam_origin, new.cam_origin), (old.color, new.color),
                 (old.texture(0), new.texture(0)), (old.rigid, new.rigid), (old.cam_rotation, new.cam_rotation),
                 (old.conductor, new.conductor)):
        assert a.storage_offset() == b.storage_offset() and a.shape == b.shape
    assert new.scratch().env_pose is not None and new.scratch().flat.numel() == new.flat.numel()
    assert old.scratch().env_pose is None
    assert ParamGrads(10, device="cpu").flat.numel() == 63 and ParamGrads(10, device="cpu", env_pose=True).flat.numel() == 67
    sc = env_scene("mirror")
    assert sc.param_grads().env_pose is None
    sc.attach_envmap_pose()
    assert tuple(sc.param_grads().env_pose.shape) == (4,)


def test_scenes_without_an_envmap_and_stale_buffers_are_refused():
    fv, ff = quad(0.0, 1.0, up=True)
    plain = {"type": "scene", "cam": sensor([0, 0, 6], [0, 0, 0], res=8, spp=4),
             "floor": {"type": "mesh", "vertices": fv, "faces": ff, "bsdf": {"type": "diffuse"},
                       "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 1.0}}}}
    sc = on_host_envpose(S.Scene.from_dict(plain, device="cpu"))
    with pytest.raises(ValueError, match="no envmap"):
        sc.attach_envmap_pose()
    sc = on_host_envpose(S.Scene.from_dict(dict(plain, sky={"type": "constant"}), device="cpu"))
    with pytest.raises(ValueError, match="`constant` environment has no pose"):
        sc.attach_envmap_pose()
    with pytest.raises(ValueError, match="`constant` environment has no pose"):
        sc.set_envmap_pose(scale=2.0)
    assert not sc.env_pose_attached
    with pytest.raises(ValueError, match="scale 0"):
        env_scene("mirror", scale=0.0).attach_envmap_pose()
    sc = env_scene("mirror")
    stale = sc.param_grads()                                             # laid out before the attach
    sc.attach_envmap_pose()
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    with pytest.raises(ValueError, match="after attach_envmap_pose"):
        integ.render_backward(sc, stale, torch.ones((RES, RES, 3)), seed=1, spp=SPP)
    with pytest.raises(ValueError, match="after attach_envmap_pose"):
        integ.render_forward(sc, stale, seed=1, spp=SPP)
    with pytest.raises(ValueError, match="rotation matrix"):
        sc.set_envmap_pose(rotation=np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="positive"):
        sc.set_envmap_pose(scale=-1.0)
    # the pose alone counts as something attached
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((RES, RES, 3)), seed=1, spp=SPP)
    assert float(p.env_pose.abs().sum()) > 0 and float(p.flat[:-4].abs().sum()) == 0


FAKE = 0x1000                # a non-NULL, 16-byte aligned device address: validation must fail before anything dereferences it


def test_entry_points_refuse_invalid_arguments_with_a_message():
    """The product library's own checks, without a device: EPSM_EINVAL before any launch, the reason in epsm_last_error."""
    from epsm_mitsuba3_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "epsm_trace.h")).read()
    assert "#define EPSM_ENV_POSE_GRADS 4" in text and lib.epsm_abi_version() == _lib.ABI_VERSION == 7
    n = 300
    need = lib.epsm_trace_envpose_workspace_bytes(C.c_int64(n))
    assert need == 3 * 4 * 4 and lib.epsm_trace_envpose_workspace_bytes(C.c_int64(0)) == 0      # one row of 4 floats per 128 paths
    sc = S.EpsmSceneC()
    sc.n_emitters, sc.emitters = 1, FAKE
    sc.env.kind, sc.env.emitter, sc.env.width, sc.env.height = 2, 0, 4, 3
    sc.env.texels = sc.env.row_cdf = sc.env.col_cdf = sc.env.cell_pdf = FAKE
    cs = S.EpsmSensor()
    cs.width = cs.height = 16
    cs.border = 2
    p = lambda ok: C.c_void_p(FAKE if ok else None)

    def bwd(scene=sc, N=n, rad=True, adj=True, grad=True, ws=FAKE, ws_bytes=need):
        return lib.epsm_trace_paths_envpose_backward(C.byref(scene), C.byref(cs), C.c_uint32(1), SPP, 4, 5, C.c_int64(0), C.c_int64(N),
                                                     p(rad), p(adj), p(grad), C.c_void_p(ws), C.c_size_t(ws_bytes), None)

    def fwd(scene=sc, N=n, rad=True, tan=True, out=True):
        return lib.epsm_trace_paths_envpose_forward(C.byref(scene), C.byref(cs), C.c_uint32(1), SPP, 4, 5, C.c_int64(0), C.c_int64(N),
                                                    p(rad), p(tan), p(out), None)

    const = S.EpsmSceneC()
    const.n_emitters, const.emitters = 1, FAKE
    const.env.kind, const.env.emitter = 1, 0
    none = S.EpsmSceneC()
    cases = [(bwd, dict(scene=const), b"not an envmap"), (bwd, dict(scene=none), b"not an envmap"), (bwd, dict(rad=False), b"NULL radiance"),
             (bwd, dict(adj=False), b"NULL adj_radiance"), (bwd, dict(grad=False), b"NULL grad_pose"), (bwd, dict(ws=None), b"workspace"),
             (bwd, dict(ws=FAKE + 4), b"workspace"), (bwd, dict(ws_bytes=need - 1), b"workspace"), (bwd, dict(N=-1), b"bad N"),
             (fwd, dict(scene=const), b"not an envmap"), (fwd, dict(rad=False), b"NULL radiance"), (fwd, dict(tan=False), b"NULL tangent_pose"),
             (fwd, dict(out=False), b"NULL d_radiance"), (fwd, dict(N=10 ** 9), b"path range")]
    for fn, kw, msg in cases:
        assert fn(**kw) == -22, kw
        err = lib.epsm_last_error()
        assert msg in err and err.startswith(b"epsm_trace_paths_envpose_" + (b"backward" if fn is bwd else b"forward")), (kw, err)
    assert bwd(N=0) == 0 and fwd(N=0) == 0 and bwd(scene=const, N=0, rad=False, ws=None) == 0
    # the host twin refuses the same calls
    hs = env_scene("mirror")
    host = hs._backend
    hc = hs.sensors[0].c_struct()
    z = lambda *s: torch.zeros(s, dtype=torch.float32)
    rad, out, grad, work = z(n, 3), z(n, 3), z(4), z(need // 4)
    q = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    head = [C.byref(hs.c_scene), C.byref(hc), C.c_uint32(1), SPP, 4, 5, C.c_int64(0), C.c_int64(n)]
    assert host.epsm_trace_paths_envpose_backward(*head, q(rad), q(rad), q(grad), q(work), C.c_size_t(need), None) == 0
    assert host.epsm_trace_paths_envpose_backward(*head, q(rad), q(rad), q(grad), q(work), C.c_size_t(need - 1), None) == -22
    assert host.epsm_trace_paths_envpose_backward(*head, q(rad), q(rad), q(None), q(work), C.c_size_t(need), None) == -22
    assert host.epsm_trace_paths_envpose_forward(*head, q(rad), q(grad), q(out), None) == 0
    assert host.epsm_trace_paths_envpose_forward(*head, q(rad), q(None), q(out), None) == -22


def test_set_envmap_pose_is_seen_by_the_next_render_without_a_rebuild():
    """Turning a W-column map by exactly 2 pi / W about its polar axis renders the image of the column-rolled bitmap, to 1e-5
    relative: the handedness of to_world <- Rot(omega) to_world, pinned independently of the gradient.  The local direction is
    to_local Rot(-omega) d: its phi grows by 2 pi / W, so column i shows what column i + 1 held.  (The mirror scene: nothing
    samples the map, so both renders draw the same paths.)"""
    W, H = MAPS["4x3"]
    bitmap = smooth_map(W, H)
    bitmap[1] *= np.array([1.0, 1.6, 0.7, 1.2], np.float32)[:, None]     # (columns that differ by more than the smooth function's)
    sc = env_scene("mirror", bitmap=bitmap)
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    before = integ.render(sc, sensor=0, seed=2, spp=SPP).clone()
    ptrs = [t.data_ptr() for t in sc._env_buf]
    R, s0 = sc.envmap_pose()
    assert np.allclose(R, R0) and s0 == SCALE0
    axis = R @ np.array([0.0, 1.0, 0.0])
    sc.set_envmap_pose(rotation=rot(axis * 2 * np.pi / W) @ R, scale=2.5)
    assert [t.data_ptr() for t in sc._env_buf] == ptrs
    assert np.allclose(sc.envmap_pose()[0], rot(axis * 2 * np.pi / W) @ R) and sc.envmap_pose()[1] == 2.5
    got = integ.render(sc, sensor=0, seed=2, spp=SPP).double()
    rel = lambda a, b: float((a - b).abs().sum() / b.abs().sum())
    want = {k: integ.render(env_scene("mirror", bitmap=np.roll(bitmap, k, axis=1), scale=2.5), sensor=0, seed=2, spp=SPP).double()
            for k in (-1, +1)}
    print(f"rolled by -1: {rel(got, want[-1]):.3e}, by +1: {rel(got, want[+1]):.3e}, unchanged: {rel(got, before.double()):.3e}")
    assert rel(got, want[-1]) <= 1e-5
    assert rel(got, want[+1]) > 1e-2 and rel(got, before.double()) > 1e-2
    # and the scale alone: the image is linear in it
    sc.set_envmap_pose(scale=5.0)
    assert rel(integ.render(sc, sensor=0, seed=2, spp=SPP).double(), 2 * got) <= 1e-5


def test_gradients_accumulate_bit_for_bit():
    sc = env_scene("ball", "16x8")
    sc.attach_envmap_pose()
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    g = _grad_image()
    p1, p2 = sc.param_grads(), sc.param_grads()
    integ.render_backward(sc, p1, g, sensor=0, seed=4, spp=SPP)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=SPP)
    integ.render_backward(sc, p2, g, sensor=0, seed=4, spp=SPP)
    assert float(p1.env_pose.abs().min()) > 0
    assert torch.equal(p2.env_pose, 2 * p1.env_pose)


# ---------------------------------------------------------------------------------------------------------------------
# 10. two ranks
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc = env_scene("ball", "16x8")
        sc.tile_paths = 500                                            # several tiles, dealt over the ranks
        sc.attach_envmap_pose()
        integ = epsm.load_dict({"type": "prb", "max_depth": 3})
        p = sc.param_grads()
        integ.render_backward(sc, p, _grad_image(), sensor=0, seed=4, spp=SPP)
        q.put((rank, p.flat.clone().numpy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_pose_gradients_match_single_process():
    sc = env_scene("ball", "16x8")
    sc.tile_paths = 500
    sc.attach_envmap_pose()
    integ = epsm.load_dict({"type": "prb", "max_depth": 3})
    p = sc.param_grads()
    integ.render_backward(sc, p, _grad_image(), sensor=0, seed=4, spp=SPP)
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
    assert float(np.abs(want[-4:]).min()) > 0
    for r in range(2):
        np.testing.assert_allclose(got[r], want, rtol=1e-4, atol=1e-6 * float(np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------------
# 11. the pole
# ---------------------------------------------------------------------------------------------------------------------
POLE_CUT = 1e-3                                  # |sin theta| below which a path is left out of the comparison
POLE_SHARE = 0.01                                # ... which may be at most this share of the paths


def pole_kept(it):
    """(n) bool: the paths none of whose items lies within POLE_CUT of a pole (by the yardstick's own float64 sin theta)."""
    near = np.zeros(it.n, bool)
    near[it.path[it.sin_theta() <= POLE_CUT]] = True
    return ~near


@pytest.mark.parametrize("size", sorted(MAPS))
def test_sensor_along_the_polar_axis(size):
    """The film's centre looks at the map's pole, where d phi / d d grows as 1 / sin theta: every output is finite, and on the
    paths whose |sin theta| > 1e-3 the gradients equal the yardstick.  The cut is a disc of 1e-3 rad in a film 0.7 rad wide:
    measured share of the paths left out 0 of 1600 (bound: 1 %), by the yardstick's own float64 sin theta."""
    sc = env_scene("pole", size)
    sc.attach_envmap_pose()
    it = Items(sc, 4, seed=3)
    keep = pole_kept(it)
    share = 1.0 - float(keep.mean())
    print(f"pole {size}: smallest |sin theta| {float(it.sin_theta().min()):.3e}, share of the paths cut {share:.4%}")
    assert float(it.sin_theta().min()) < 0.05                            # the pole is in view
    assert share <= POLE_SHARE
    for name, t in TANGENTS.items():
        got = forward(sc, it, 4, 3, t)
        want = it.fd(t, 1e-6)
        assert np.isfinite(got).all() and np.isfinite(want[keep]).all()
        gap = l1_rel(got[keep], want[keep])
        print(f"pole {size} {name}: |fwd - FD64|_1 / |FD64|_1 = {gap:.3e}")
        assert gap <= 1e-3, (name, gap)
    adj = torch.rand((N_PATHS, 3), generator=torch.Generator().manual_seed(1))
    grad = torch.zeros(4)
    sc.trace_envpose_backward(0, 3, SPP, 4, 0, N_PATHS, it.radiance.contiguous(), adj, grad)
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().min()) > 0
    p = sc.param_grads()
    epsm.load_dict({"type": "prb", "max_depth": 4}).render_backward(sc, p, _grad_image(), sensor=0, seed=3, spp=SPP)
    assert bool(torch.isfinite(p.flat).all())
