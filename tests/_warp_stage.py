"""What tests/test_warp_stage.py (host twin) and tests/test_gpu_warp_stage.py (device) share: the scene, the hand-written warp
requests, the reference of tests/_warp_oracle.py computed once per case, and the assertions.

Scene (370 triangles): a lat-long sphere with vertex normals (attached), a flat-shaded 2 x 2 grid of quads (attached), a
`rectangle` shape (not attached), open background.  Requests: N = 605 paths (two workgroups and a ragged third with a partial
wave), per-path counts cycling through 0 .. 13 with the whole second 256-path block at 0, max_depth = 3 so that n_max = 7 and the
counts above it leave poisoned slots, path_offset = 1000.  Origins on a shell in free space; rays aimed at the sphere's silhouette,
the occluder's and the rectangle's border (offset by up to two widths 1 / sqrt(kappa) of the cone to either side), at their
interiors and at the background; origins glued to nothing (camera-like), to attached and to non-attached triangles, with and
without em_inv_dist.

Two conditions on the fixture, both from the reference alone:
  * a request with an UNDECIDED auxiliary ray (tests/_ray_query.py's rule and EPS) is left out of the per-request comparisons and
    zeroed in both backward sums; at most 2 % of a case's requests may be such (they are re-aimed four times like the requests
    of the second condition, so what remains is 0 .. 0.11 %);
  * a request is kept away from a boundary until none of its rays has a weight denominator inv_vmf - 1 + B below 1e-2 (it is
    re-aimed, at most four times, then sent to the background): below that float32 loses the weight's digits by conditioning alone
    (ISSUE: `tol` must come out <= 1e-3), and the jump of the weight at 1e-4 is not something a reference can pin.

Tolerance, per case and pass, computed at run time: e32 = the worst |ref32 - ref64| / A over the case's outputs, ref32 the float32
run of the oracle; tol = 8 e32, floor 32 u, and tol <= 1e-3 is asserted.  Measured (MEASUREMENTS.md 29, with the errors of both builds):

  rays, kappa, antithetic    e32 fwd   tol fwd   e32 bwd   tol bwd
   5, 1e3, yes               1.05e-5   8.42e-5   4.91e-6   3.92e-5
  16, 1e3, no                1.91e-5   1.52e-4   2.56e-5   2.05e-4
  24, 1e5, no                2.12e-5   1.70e-4   7.53e-5   6.02e-4
  32, 1e3, yes               1.53e-5   1.22e-4   9.77e-6   7.82e-5
  33, 1e5, yes               2.53e-5   2.03e-4   3.27e-5   2.61e-4
  64, 1e3, no                1.14e-5   9.10e-5   9.99e-6   7.99e-5
  64, 1e5, no                1.22e-4   9.73e-4   3.35e-5   2.68e-4"""
import functools

import numpy as np
import torch

import _warp_oracle as O
from _reparam_scenes import sphere
from _scenes import on_host, sensor
from epsm_mitsuba3_amd import scene as S

N_PATHS, PATH_OFFSET, MAX_DEPTH, SEED = 605, 1000, 3, 7
# (rays, kappa, antithetic): all three G partly and exactly filled, an odd count under EPSM_REPARAM_ANTITHETIC, both kappa
CASES = [(5, 1e3, True), (16, 1e3, False), (24, 1e5, False), (32, 1e3, True), (33, 1e5, True), (64, 1e3, False), (64, 1e5, False)]
CASE_IDS = [f"rays{r}-kappa{k:g}{'-anti' if a else ''}" for r, k, a in CASES]
UNDECIDED_CAP, W_DENOM_MIN, TOL_CAP, TOL_FLOOR = 0.02, 1e-2, 1e-3, 32 * O.U32
SPHERE_R, OCC_C, OCC_H, RECT_C, RECT_H = 0.5, np.array([1.3, 0.2, 0.1]), 0.35, np.array([-1.4, -0.1, 0.0]), 0.5


def scene_dict():
    v, n, f = sphere(SPHERE_R, (0, 0, 0), 10, 20)
    g = np.linspace(-OCC_H, OCC_H, 3)
    ov = np.array([[x, y, 0.0] for y in g for x in g]) + OCC_C
    of = np.array([t for j in range(2) for i in range(2) for t in ([3 * j + i, 3 * j + i + 1, 3 * j + i + 4], [3 * j + i, 3 * j + i + 4, 3 * j + i + 3])])
    tw = np.eye(4)
    tw[:3, :3] *= RECT_H
    tw[:3, 3] = RECT_C
    return {"type": "scene", "cam": sensor([0, 0, 4], [0, 0, 0], res=8, spp=1),
            "sphere": {"type": "mesh", "vertices": v, "normals": n, "faces": f},
            "occluder": {"type": "mesh", "vertices": ov, "faces": of, "face_normals": True},
            "border": {"type": "rectangle", "to_world": tw}}


def build_scene(device="cpu"):
    sc = S.Scene.from_dict(scene_dict(), device=device)
    if str(device) == "cpu":
        on_host(sc)
    sc.attach("sphere", positions=True)
    sc.attach("occluder", positions=True)
    return sc


@functools.lru_cache(maxsize=None)
def scene_arrays():
    sc = S.Scene.from_dict(scene_dict(), device="cpu")
    sc.attach("sphere", positions=True)
    sc.attach("occluder", positions=True)
    sa = O.SceneArrays.of(sc)
    sa.slices = dict(sc.mesh_tri_slices)
    return sa


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(a):
    h = np.where(np.abs(a[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    e1 = _unit(np.cross(a, h))
    return e1, np.cross(a, e1)


def _aim(rng, o, cat, sigma):
    """directions of rays from o by target category: 0 sphere silhouette, 1 sphere interior, 2 / 3 occluder border / interior,
    4 / 5 rectangle border / interior, 6 background"""
    n = o.shape[0]
    d = np.empty((n, 3))
    delta = rng.uniform(-2 * sigma, 2 * sigma, size=n)
    L = np.linalg.norm(o, axis=1)
    a = -o / L[:, None]
    e1, e2 = _frame(a)
    phi = rng.uniform(0, 2 * np.pi, size=n)
    alpha = np.arcsin(SPHERE_R / L)
    ang = np.where(cat == 0, alpha + delta, alpha * 0.8 * np.sqrt(rng.uniform(size=n)))
    cone = np.cos(ang)[:, None] * a + np.sin(ang)[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    side, s = rng.integers(0, 4, size=n), rng.uniform(-1, 1, size=n)
    out = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0]])[side]
    along = np.array([[0, 1.0, 0], [0, 1.0, 0], [1.0, 0, 0], [1.0, 0, 0]])[side]
    inner = np.concatenate([rng.uniform(-0.8, 0.8, size=(n, 2)), np.zeros((n, 1))], axis=1)
    for border, interior, c, h in ((2, 3, OCC_C, OCC_H), (4, 5, RECT_C, RECT_H)):
        p = c + h * (out + along * s[:, None])
        p = p + out * (delta * np.linalg.norm(p - o, axis=1))[:, None]
        d[cat == border] = _unit(p - o)[cat == border]
        d[cat == interior] = _unit(c + h * inner - o)[cat == interior]
    d[cat <= 1] = cone[cat <= 1]
    away = _unit(-a + 0.3 * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2))
    d[cat == 6] = away[cat == 6]
    return d.astype(np.float32)


def counts():
    c = (np.arange(N_PATHS) * 5 + 3) % 14                                  # every value 0 .. 13, many times
    c[256:512] = 0                                                         # a whole workgroup without a request
    c[N_PATHS - 1], c[0], c[255], c[512] = 13, 13, 7, 1                     # the last path of the ragged wave, slot n_max - 1 at a block's edge
    return c.astype(np.int32)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(rays, kappa, antithetic):
    sa = scene_arrays()
    cfg = O.Cfg(rays, kappa, 3.0, antithetic, SEED, PATH_OFFSET, MAX_DEPTH)
    rng = np.random.default_rng(1000 + rays + int(antithetic))
    cnt = counts()
    live_n = np.minimum(cnt, cfg.n_max)
    path = np.repeat(np.arange(N_PATHS), live_n)
    n = np.concatenate([np.arange(k) for k in live_n])
    R = path.shape[0]
    # origins on a shell above the scene: every plane is seen from its front
    o = _unit(rng.normal(size=(R, 3)) * [1.0, 1.0, 0.3] + [0, 0, 1.2]) * rng.uniform(2.5, 3.5, size=(R, 1))
    o[:, 2] = np.abs(o[:, 2]) + 1.0
    o = o.astype(np.float32)
    sigma = 1.0 / np.sqrt(kappa)
    cat = rng.choice(7, size=R, p=[0.30, 0.15, 0.15, 0.10, 0.12, 0.06, 0.12])
    d = _aim(rng, o.astype(np.float64), cat, sigma)
    # what the origin is glued to: 0 nothing, 1 attached, 2 not attached, 3 / 4 the same as an emitter ray, 5 emitter ray glued to nothing
    kind = rng.choice(6, size=R, p=[0.35, 0.25, 0.10, 0.20, 0.05, 0.05])
    att = np.nonzero(sa.attached_tri)[0]
    non = np.nonzero(~sa.attached_tri)[0]
    ftri = np.full(R, O.NO_TRI, dtype=np.int64)
    ftri[(kind == 1) | (kind == 3)] = rng.choice(att, size=R)[(kind == 1) | (kind == 3)]
    ftri[(kind == 2) | (kind == 4)] = rng.choice(non, size=R)[(kind == 2) | (kind == 4)]
    fb = rng.uniform(size=(R, 2))
    fb = np.where((fb.sum(axis=1) > 1)[:, None], 1 - fb, fb)
    em = np.where(kind >= 3, 1.0 / rng.uniform(1.0, 4.0, size=R), 0.0)
    req = O.Requests(path, n, o, d, rng.normal(size=(R, 3)), rng.normal(size=R), em, ftri, fb[:, 0], fb[:, 1])
    # keep the requests decided and away from where float32 cannot hold the weight: re-aim those that are not
    W = O.collect(sa, cfg, req)
    reaimed = 0
    for attempt in range(5):
        with np.errstate(invalid="ignore"):
            bad = np.nonzero(((W.tri >= 0) & (W.w_denom < W_DENOM_MIN)).any(axis=1) | ~W.decided)[0]
        if attempt == 4:
            bad = np.nonzero(((W.tri >= 0) & (W.w_denom < W_DENOM_MIN)).any(axis=1))[0]
        if bad.size == 0:
            break
        reaimed += bad.size
        c = np.full(bad.size, 6) if attempt == 4 else cat[bad]
        req.d[bad] = _aim(rng, o[bad].astype(np.float64), c, sigma)
        cat[bad] = c
        Wb = O.collect(sa, cfg, req.take(bad))
        for k, v in vars(Wb).items():
            getattr(W, k)[bad] = v
    K = Case()
    K.sa, K.cfg, K.req, K.count, K.cat, K.kind, K.reaimed = sa, cfg, req, cnt, cat, kind, reaimed
    K.W64 = W
    K.W32 = O.collect(sa, cfg, req, np.float32, hits=(W.tri, W.ray_decided))
    K.decided = W.decided
    K.tan = np.random.default_rng(5).normal(size=(sa.V, 3)).astype(np.float32)
    K.alone = np.random.default_rng(6).choice(np.nonzero(K.decided)[0], size=64, replace=False)
    # ---- the reference, and its own float32 error in units of A
    K.fwd64 = O.forward(sa, W, req, K.tan)
    f32 = O.forward(sa, K.W32, req, K.tan, np.float32)
    dec = K.decided
    K.e32_fwd = max(_units(f32[0][dec], K.fwd64[0][dec], K.fwd64[2][dec]), _units(f32[1][dec], K.fwd64[1][dec], K.fwd64[3][dec]))
    K.bwd64 = O.backward(sa, W, req, keep=dec)
    b32 = O.backward(sa, K.W32, req, np.float32, keep=dec)
    e = _units(b32[0], K.bwd64[0], K.bwd64[1])
    K.alone64 = []
    for r in K.alone:
        one = np.zeros(req.R, dtype=bool)
        one[r] = True
        K.alone64.append(O.backward(sa, W, req, keep=one))
        e = max(e, _units(O.backward(sa, K.W32, req, np.float32, keep=one)[0], *K.alone64[-1]))
    K.e32_bwd = e
    K.tol_fwd, K.tol_bwd = max(8 * K.e32_fwd, TOL_FLOOR), max(8 * K.e32_bwd, TOL_FLOOR)
    return K


def _units(got, ref, A):
    """the worst |got - ref| / A; where A is zero both must be"""
    got, ref, A = (np.asarray(x, dtype=np.float64) for x in (got, ref, A))
    zero = A == 0
    assert (got[zero] == 0).all() and (ref[zero] == 0).all(), "a non-zero output where the scale A is zero"
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / A[~zero]).max())


def describe(K):
    three = float((K.W64.distinct[K.decided] >= 3).mean())
    return (f"live requests {K.req.R}, undecided {1 - K.decided.mean():.4f}, re-aimed {K.reaimed}, >= 3 triangles {three:.3f}, all miss "
            f"{float((K.W64.tri < 0).all(axis=1).mean()):.3f}, e32 fwd {K.e32_fwd:.3g} bwd {K.e32_bwd:.3g}, tol fwd {K.tol_fwd:.3g} bwd {K.tol_bwd:.3g}")


def check_fixture(K):
    """Conditions on the fixture alone, before any kernel is looked at."""
    print(describe(K))
    assert 1 - K.decided.mean() <= UNDECIDED_CAP
    assert K.tol_fwd <= TOL_CAP and K.tol_bwd <= TOL_CAP, (K.tol_fwd, K.tol_bwd)
    assert set(K.count.tolist()) == set(range(14)) and (K.count[256:512] == 0).all() and (K.count > K.cfg.n_max).any()
    assert K.req.R >= 1500
    hit_any = (K.W64.tri >= 0).any(axis=1)
    miss_any = (K.W64.tri < 0).any(axis=1)
    assert (~hit_any).sum() >= 50, "requests whose rays all miss"
    assert (hit_any & miss_any).sum() >= 200, "requests that straddle a boundary"
    assert ((K.req.em != 0) & (K.req.ftri != O.NO_TRI) & hit_any & miss_any).sum() >= 30, "emitter rays past a silhouette"
    for k in range(6):
        assert (K.kind == k).sum() >= 30, k
    for name in ("sphere", "occluder", "border"):                          # every shape is hit, its boundary branch runs
        lo, hi = K.sa.slices[name]
        assert ((K.W64.tri >= lo) & (K.W64.tri < hi)).any(axis=1).sum() >= 100, name
    if K.cfg.kappa <= 1e3 and K.cfg.rays >= 16:                            # the group_min rounds: three and more triangles per warp
        assert (K.W64.distinct[K.decided] >= 3).mean() >= 0.2


# ---------------------------------------------------------------------------- the build under test
class Runner:
    """Stage 2 alone on a Scene (device, or host twin on the CPU) through Scene.probe_reparam_warps"""

    def __init__(self, device):
        self.sc = build_scene(device)
        self.dev = self.sc.device

    def _sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def call(self, cfg, n_paths, words, grad=None, tan=None, path_offset=None):
        ws = torch.from_numpy(words.copy()).to(self.dev)
        rc = self.sc.probe_reparam_warps(cfg.seed, cfg.path_offset if path_offset is None else path_offset, n_paths, cfg.max_depth,
                                         ws.view(torch.uint8), cfg.rays, cfg.kappa, cfg.exponent, cfg.antithetic, grad_pos=grad, tan_pos=tan)
        assert rc == 0, rc
        self._sync()
        return ws.cpu().numpy()

    def backward(self, cfg, n_paths, words, path_offset=None):
        grad = torch.zeros((self.sc.V, 3), dtype=torch.float32, device=self.dev)
        after = self.call(cfg, n_paths, words, grad=grad, path_offset=path_offset)
        assert np.array_equal(after, words), "the backward kernel wrote into its workspace"
        return grad.cpu().numpy()

    def forward(self, cfg, n_paths, words, tan):
        return self.call(cfg, n_paths, words, tan=torch.from_numpy(tan).to(self.dev))


def _worst(got, ref, A, tol, extra=0.0):
    """asserts |got - ref| <= tol A + extra |ref| everywhere, returns the worst error in units of A"""
    got, ref, A = (np.asarray(x, dtype=np.float64) for x in (got, ref, A))
    err = np.abs(got - ref)
    bad = err > tol * A + extra * np.abs(ref)
    units = float((err[A > 0] / A[A > 0]).max()) if (A > 0).any() else 0.0
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} outputs beyond tol = {tol:.3g}; worst {units:.3g} A; first at "
                           f"{np.argwhere(bad)[:4].tolist()}: got {got[bad][:4]}, reference {ref[bad][:4]}, A {A[bad][:4]}")
    return units


def forward_outputs(K, after):
    slots = O.unpack_slots(after, N_PATHS).view(np.float32)
    k = (K.req.n, K.req.path)
    return np.stack([slots[k + (8 + j,)] for j in range(3)], axis=1), slots[k + (3,)]


def check_forward(run, K, label):
    """d', div' of every decided request against float64; the poison, the requests' other words, two calls bit for bit."""
    before = O.pack_workspace(N_PATHS, K.req, K.count)
    after = run.forward(K.cfg, N_PATHS, before, K.tan)
    again = run.forward(K.cfg, N_PATHS, before, K.tan)
    assert np.array_equal(after, again), "two calls of the forward stage differ"
    sb, sa_ = O.unpack_slots(before, N_PATHS), O.unpack_slots(after, N_PATHS)
    live = np.arange(O.MAX_REQ)[:, None] < np.minimum(K.count, K.cfg.n_max)[None, :]
    assert np.array_equal(sb[~live], sa_[~live]) and (sa_[~live] == O.POISON).all(), "a slot at or past a path's clipped count was written"
    assert np.array_equal(after[O.request_bytes(N_PATHS) // 4:], before[O.request_bytes(N_PATHS) // 4:]), "the counts were written"
    kept = [0, 1, 2, 4, 5, 6, 7, 11, 12, 13, 14, 15]
    assert np.array_equal(sb[live][:, kept], sa_[live][:, kept]), "o, d, em_inv_dist, ftri, fb1, fb2 of a live request changed"
    ddir, div = forward_outputs(K, after)
    assert np.isfinite(ddir).all() and np.isfinite(div).all(), "poison reached a result"
    dec = K.decided
    wd = _worst(ddir[dec], K.fwd64[0][dec], K.fwd64[2][dec], K.tol_fwd)
    wv = _worst(div[dec], K.fwd64[1][dec], K.fwd64[3][dec], K.tol_fwd)
    assert float(np.abs(K.fwd64[0][dec]).max()) > 0 and float(np.abs(K.fwd64[1][dec]).max()) > 0
    print(f"{label} forward: worst error d' {wd:.3g} A, div' {wv:.3g} A (tol {K.tol_fwd:.3g})")
    return ddir, div


def zeroed(K):
    """the requests with an undecided ray carry no adjoint: they add nothing to either backward sum"""
    gdir, gdiv = K.req.gdir.copy(), K.req.gdiv.copy()
    gdir[~K.decided], gdiv[~K.decided] = 0.0, 0.0
    return gdir, gdiv


def check_backward(run, K, label):
    """grad_pos row by row against the float64 sums; rows of meshes that are not attached exactly zero."""
    words = O.pack_workspace(N_PATHS, K.req, K.count, *zeroed(K))
    grad = run.backward(K.cfg, N_PATHS, words)
    assert np.isfinite(grad).all(), "poison reached a result"
    assert (grad[~K.sa.attached_row] == 0).all(), "a row of a mesh that is not attached was written"
    assert float(np.abs(K.bwd64[0]).max()) > 0
    w = _worst(grad, K.bwd64[0], K.bwd64[1], K.tol_bwd, O.U32)
    print(f"{label} backward: worst row error {w:.3g} A (tol {K.tol_bwd:.3g})")
    return grad


def check_backward_alone(run, K, label):
    """64 requests each on its own: path path_offset + i alone in a tile of one path, the slots before its own carrying no
    adjoint -- no cancellation across requests can hide a wrong share."""
    worst, grads = 0.0, []
    for r, (rows, A) in zip(K.alone, K.alone64):
        n = int(K.req.n[r])
        ids = np.full(n + 1, r)
        one = K.req.take(ids)
        one.path[:], one.n[:] = 0, np.arange(n + 1)
        gdir, gdiv = one.gdir.copy(), one.gdiv.copy()
        gdir[:n], gdiv[:n] = 0.0, 0.0
        words = O.pack_workspace(1, one, [n + 1], gdir, gdiv)
        grad = run.backward(K.cfg, 1, words, path_offset=K.cfg.path_offset + int(K.req.path[r]))
        worst = max(worst, _worst(grad, rows, A, K.tol_bwd, O.U32))
        grads.append(grad)
    print(f"{label} backward, 64 requests alone: worst row error {worst:.3g} A (tol {K.tol_bwd:.3g})")
    return grads


def check_transpose(run, K, label):
    """<g, forward(u)> = <backward(g), u> for the random tangent u = K.tan and the requests' adjoints g: over all requests at
    once, and for each of the 64 requests that run alone -- there no sum over requests widens the bound."""
    gdir, gdiv = zeroed(K)
    ddir, div = forward_outputs(K, run.forward(K.cfg, N_PATHS, O.pack_workspace(N_PATHS, K.req, K.count), K.tan))
    grad = run.backward(K.cfg, N_PATHS, O.pack_workspace(N_PATHS, K.req, K.count, gdir, gdiv))
    lhs = float((gdir.astype(np.float64) * ddir).sum() + (gdiv.astype(np.float64) * div).sum())
    rhs = float((grad.astype(np.float64) * K.tan).sum())
    scale = float((np.abs(gdir) * K.fwd64[2]).sum() + (np.abs(gdiv) * K.fwd64[3]).sum()) * K.tol_fwd + \
        float((K.bwd64[1] * np.abs(K.tan)).sum()) * K.tol_bwd
    print(f"{label} transpose: <g, Ju> = {lhs:.9g}, <J^T g, u> = {rhs:.9g}, difference {abs(lhs - rhs):.3g}, bound {scale:.3g}")
    assert abs(lhs) > 0 and abs(lhs - rhs) <= scale
    worst = 0.0
    for r, grad, (_, A) in zip(K.alone, check_backward_alone(run, K, label), K.alone64):
        g3, g1 = K.req.gdir[r].astype(np.float64), float(K.req.gdiv[r])
        lhs, rhs = float((g3 * ddir[r]).sum() + g1 * div[r]), float((grad.astype(np.float64) * K.tan).sum())
        bound = K.tol_fwd * float((np.abs(g3) * K.fwd64[2][r]).sum() + abs(g1) * K.fwd64[3][r]) + K.tol_bwd * float((A * np.abs(K.tan)).sum())
        assert abs(lhs - rhs) <= bound, (int(r), lhs, rhs, bound)
        worst = max(worst, abs(lhs - rhs) / bound if bound > 0 else 0.0)
    print(f"{label} transpose, 64 requests alone: worst difference {worst:.3g} of its bound")
