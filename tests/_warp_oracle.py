"""A float64 restatement of what STAGE 2 of the reparameterised passes computes from one warp request
(csrc/epsm_trace_reparam.hip: epsm_reparam_warp_kernel<G>, epsm_reparam_fwd_warp_kernel<G>, run alone through
epsm_probe_reparam_warps, include/epsm_trace.h).  Test infrastructure; it shares no code with csrc/.  In numpy, from the scene's
float32 arrays, the pass's cfg and a list of requests, per request:

  draws     key = (0xffffffff ^ seed) ^ (0x9E3779B9 (64 n + rs + 1) mod 2^32), stream = PCG32 seeded with tea(key, path_offset + i),
            sx, sy_ its first two next_1d(); rs = r & ~1 under EPSM_REPARAM_ANTITHETIC with the even ray mirrored (reparam.py:82-84,
            189-196); the von Mises-Fisher direction of warp.h:559-566 in the Duff frame of d (vector.h coordinate_system)
  hits      every auxiliary ray against every triangle in float64 (mesh.h:343-365), DECIDED by tests/_ray_query.py's rule and EPS
  B         the boundary term: rectangle shapes (rectangle.cpp:320-321), flat-shaded meshes (the equilateral parameterisation,
            mesh.cpp:832-887), meshes with vertex normals (dot(n, ray_d)^2)
  weights   inv_vmf, w, dw = tangent clamp(..) (reparam.py:104-118), Z, dZ
  backward  g_V, per ray g_v, g_p and the shares of the hit triangle's vertices (POS_ATTACHED meshes), misses to g_d, the origin's
            adjoint through em_inv_dist to the glued triangle (reparam.py:269-327) -> (V,3) float64
  forward   d' = P(sum w_i v_i') / Z, div' = sum (dw_i - w_i dZ / Z) . v_i' / Z (reparam.py:155-221)
  A         beside every output the same expression with every product replaced by its absolute value (no cancellation): the unit
            errors are measured in, as tests/test_gpu_rigid.py measures its reductions in units of sum |terms|.  One factor is
            not taken by its own size: a hit's barycentric weights b_j count as 1.  They are the intersector's outputs, quotients
            of determinants whose float32 error is ABSOLUTE (about 20 u at these distances; tests/_ray_query.py bounds it by an
            absolute UV_TOL): next to an edge a weight of 2e-4 carries no digits, and a vertex row that receives nothing else
            would have an error of its whole size.  The glued origin's weights are given exactly; their 1 - b1 - b2 counts as
            1 + |b1| + |b2|.  A dropped or doubled lane still moves a row by about a third of that lane's A.

Every function takes ``dt``: with np.float32 the same statements run in float32 on the float64 run's hit triangles -- the
reference's OWN rounding error, from which the tests derive their tolerance (tol = 8 e32, floor 32 u)."""
import numpy as np

from _ray_query import EPS, _moeller_trumbore_pairs, zero_area

NO_TRI = 0xFFFFFFFF
MAX_REQ, REQ_WORDS = 13, 16              # rp::kMaxReq requests per path of sizeof(rp::WarpReq) / 4 words
MESH_VERTEX_NORMALS, MESH_POS_ATTACHED, MESH_IS_MESH = 1, 4, 16
U32 = 2.0 ** -24
W_DENOM_FLOOR = 1e-4                     # reparam.py:113: the weight is zero below it


# ---------------------------------------------------------------------------- random streams (python-int restatements: _refvec.py)
def tea(v0, v1):
    """sample_tea_32 (4 rounds) on uint32 arrays -> (v0, v1)"""
    v0, v1 = np.asarray(v0, dtype=np.uint64) & 0xFFFFFFFF, np.asarray(v1, dtype=np.uint64) & 0xFFFFFFFF
    M = np.uint64(0xFFFFFFFF)
    s = np.uint64(0)
    for _ in range(4):
        s = (s + np.uint64(0x9E3779B9)) & M
        v0 = (v0 + ((((v1 << np.uint64(4)) & M) + np.uint64(0xA341316C)) ^ (v1 + s) ^ ((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)))) & M
        v1 = (v1 + ((((v0 << np.uint64(4)) & M) + np.uint64(0xAD90777D)) ^ (v0 + s) ^ ((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)))) & M
    return v0.astype(np.uint32), v1.astype(np.uint32)


class Pcg32Vec:
    """_refvec.Pcg32Py side by side for arrays of (initstate, initseq)"""
    MULT = np.uint64(0x5851F42D4C957F2D)

    def __init__(self, initstate, initseq):
        self.inc = (np.asarray(initseq, dtype=np.uint64) << np.uint64(1)) | np.uint64(1)
        self.state = np.zeros_like(self.inc)
        self.next_u32()
        self.state = self.state + np.asarray(initstate, dtype=np.uint64)
        self.next_u32()

    def next_u32(self):
        old = self.state
        with np.errstate(over="ignore"):
            self.state = old * self.MULT + self.inc
        x = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)) & np.uint64(0xFFFFFFFF)
        r = old >> np.uint64(59)
        return (((x >> r) | (x << ((np.uint64(32) - r) & np.uint64(31)))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)

    def next_1d(self):
        return ((self.next_u32() >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


class Cfg:
    def __init__(self, rays, kappa, exponent=3.0, antithetic=False, seed=0, path_offset=0, max_depth=3):
        self.rays, self.kappa, self.exponent, self.antithetic = int(rays), float(kappa), float(exponent), bool(antithetic)
        self.seed, self.path_offset, self.max_depth = int(seed), int(path_offset), int(max_depth)

    @property
    def n_max(self):
        return min(1 + 2 * min(self.max_depth, 6), MAX_REQ)


def draws(cfg, path, n):
    """(sx, sy_, mirror) of every auxiliary ray: (R, rays) float32, float32, float64 (+-1)"""
    r = np.arange(cfg.rays)
    rs = (r & ~1) if cfg.antithetic else r
    mult = (np.uint64(0x9E3779B9) * (np.asarray(n, dtype=np.uint64)[:, None] * np.uint64(64) + rs[None, :].astype(np.uint64) + np.uint64(1))) \
        & np.uint64(0xFFFFFFFF)
    key = np.uint64(0xFFFFFFFF ^ (cfg.seed & 0xFFFFFFFF)) ^ mult
    widx = (np.asarray(path, dtype=np.uint64) + np.uint64(cfg.path_offset))[:, None] + np.zeros_like(key)
    v0, v1 = tea(key, widx)
    rng = Pcg32Vec(v0, v1)
    sx = rng.next_1d()
    sy_ = rng.next_1d()
    mirror = np.where(cfg.antithetic & ((r & 1) == 0), -1.0, 1.0)[None, :] + np.zeros(sx.shape)
    return sx, sy_, mirror


# ---------------------------------------------------------------------------- the scene's arrays
class SceneArrays:
    """pos, nrm (V,3) float32; tri (T,3), tri_mesh (T) int64; mesh_flags, mesh_tri_begin (M) int64"""

    def __init__(self, pos, nrm, tri, tri_mesh, mesh_flags, mesh_tri_begin):
        self.pos, self.nrm = np.ascontiguousarray(pos, dtype=np.float32), np.ascontiguousarray(nrm, dtype=np.float32)
        self.tri, self.tri_mesh = np.asarray(tri, dtype=np.int64), np.asarray(tri_mesh, dtype=np.int64)
        self.mesh_flags, self.mesh_tri_begin = np.asarray(mesh_flags, dtype=np.int64), np.asarray(mesh_tri_begin, dtype=np.int64)
        self.V, self.T = self.pos.shape[0], self.tri.shape[0]
        self.tri_flags = self.mesh_flags[self.tri_mesh]
        self.attached_tri = (self.tri_flags & MESH_POS_ATTACHED) != 0
        self.attached_row = np.zeros(self.V, dtype=bool)
        self.attached_row[self.tri[self.attached_tri].reshape(-1)] = True

    @staticmethod
    def of(scene):
        return SceneArrays(scene.positions.cpu().numpy(), scene.normals.cpu().numpy(), scene.tri.cpu().numpy(), scene.tri_mesh.cpu().numpy(),
                           [m.flags() for m in scene.meshes], [scene.mesh_tri_slices[m.name][0] for m in scene.meshes])


class Requests:
    """R requests: path, n (R) int; o, d, gdir (R,3), gdiv, em, fb1, fb2 (R) float32; ftri (R) int64 (NO_TRI: glued to nothing)"""

    def __init__(self, path, n, o, d, gdir, gdiv, em, ftri, fb1, fb2):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.path, self.n = np.asarray(path, dtype=np.int64), np.asarray(n, dtype=np.int64)
        self.o, self.d, self.gdir, self.gdiv, self.em, self.fb1, self.fb2 = f(o), f(d), f(gdir), f(gdiv), f(em), f(fb1), f(fb2)
        self.ftri = np.asarray(ftri, dtype=np.int64)
        self.R = self.path.shape[0]

    def take(self, ids):
        ids = np.asarray(ids)
        return Requests(self.path[ids], self.n[ids], self.o[ids], self.d[ids], self.gdir[ids], self.gdiv[ids], self.em[ids], self.ftri[ids],
                        self.fb1[ids], self.fb2[ids])


# ---------------------------------------------------------------------------- small vector helpers on (.., 3) arrays
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _proj(x, axis, absolute=False):
    """x - axis (axis . x); with `absolute` the same with |.| of every product and a plus"""
    if absolute:
        return np.abs(x) + np.abs(axis) * _dot(np.abs(axis), np.abs(x))[..., None]
    return x - axis * _dot(axis, x)[..., None]


def duff_frame(n, dt):
    """vector.h coordinate_system (Duff et al.)"""
    one = dt(1.0)
    sign = np.where(n[..., 2] >= 0, one, -one).astype(dt)
    a = -one / (sign + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    ms = lambda x: np.where(n[..., 2] < 0, -x, x)
    s = np.stack([ms(n[..., 0] * n[..., 0] * a) + one, ms(b), ms(-n[..., 0])], axis=-1)
    t = np.stack([b, n[..., 1] * n[..., 1] * a + sign, -n[..., 1]], axis=-1)
    return s.astype(dt), t.astype(dt)


# ---------------------------------------------------------------------------- the auxiliary rays
def aux_rays(cfg, req, dt=np.float64):
    """-> dict(sy_, tangent (R,rays,3), ray_d (R,rays,3)) in dt"""
    sx, sy_, mirror = draws(cfg, req.path, req.n)
    sx, sy_, mirror = sx.astype(dt), sy_.astype(dt), mirror.astype(dt)
    kappa, one = dt(cfg.kappa), dt(1.0)
    sy = np.maximum(one - sy_, dt(1e-6))
    with np.errstate(under="ignore"):
        e = np.log(sy + (one - sy) * np.exp(dt(-2.0) * kappa)) / kappa          # cos_theta - 1 <= 0
    cos_theta = one + e
    sin_theta = np.sqrt(np.maximum(-e * (dt(2.0) + e), dt(0.0)))
    phi = dt(2.0) * dt(np.pi) * sx
    olx, oly = mirror * np.cos(phi) * sin_theta, mirror * np.sin(phi) * sin_theta
    d = req.d.astype(dt)
    fs, ft = duff_frame(d, dt)
    tangent = fs[:, None, :] * olx[..., None] + ft[:, None, :] * oly[..., None]
    ray_d = tangent + d[:, None, :] * cos_theta[..., None]
    return dict(sy_=sy_, tangent=tangent.astype(dt), ray_d=ray_d.astype(dt))


def closest_hits(sa, o, ray_d, chunk=2048):
    """o (R,3), ray_d (R,rays,3) float64 -> tri (R,rays) int64 (-1: miss), decided (R,rays) bool by _ray_query's rule: the tightened
    and the widened test name the same closest triangle and no other widened candidate lies within t (1 + EPS) of it, or neither
    finds anything."""
    R, rays = ray_d.shape[:2]
    verts = sa.pos.astype(np.float64)[sa.tri]
    live = ~zero_area(verts)
    oo = np.repeat(o.astype(np.float64), rays, axis=0)
    dd = ray_d.reshape(-1, 3).astype(np.float64)
    tri = np.full(R * rays, -1, dtype=np.int64)
    decided = np.zeros(R * rays, dtype=bool)
    for a in range(0, R * rays, chunk):
        t, u, v = _moeller_trumbore_pairs(oo[a:a + chunk], dd[a:a + chunk], verts)
        with np.errstate(invalid="ignore"):
            wide = live[None] & (u >= -EPS) & (v >= -EPS) & (u + v <= 1 + EPS) & (t > 0)
            tight = wide & (u >= EPS) & (v >= EPS) & (u + v <= 1 - EPS)
        tw = np.where(wide, t, np.inf)
        tt = np.where(tight, t, np.inf)
        k = np.argmin(tt, axis=1)
        tk = tt[np.arange(tt.shape[0]), k]
        none = ~wide.any(axis=1)
        near = (tw <= (tk * (1 + EPS))[:, None]).sum(axis=1)
        ok = np.isfinite(tk) & (np.argmin(tw, axis=1) == k) & (near == 1)
        decided[a:a + chunk] = none | ok
        tri[a:a + chunk] = np.where(ok, k, -1)
    return tri.reshape(R, rays), decided.reshape(R, rays)


def _boundary(sa, tri, u, v, ray_d, dt):
    """boundary_test on hits (flat arrays): the three branches"""
    one, half = dt(1.0), dt(0.5)
    w = one - u - v
    flags = sa.tri_flags[tri]
    pos, nrm = sa.pos.astype(dt), sa.nrm.astype(dt)
    iv = sa.tri[tri]
    B = np.ones(tri.shape[0], dtype=dt)
    # rectangle = its first two triangles (v0 v1 v2), (v0 v2 v3): uv in [0,1]^2 along v1 - v0 and v2 - v1
    m = (flags & MESH_IS_MESH) == 0
    if m.any():
        i0 = sa.tri[sa.mesh_tri_begin[sa.tri_mesh[tri[m]]]]
        q0, q1, q2 = pos[i0[:, 0]], pos[i0[:, 1]], pos[i0[:, 2]]
        p = pos[iv[m, 0]] * w[m, None] + pos[iv[m, 1]] * u[m, None] + pos[iv[m, 2]] * v[m, None]
        eu, ev, r = q1 - q0, q2 - q1, p - q0
        uu, vv = _dot(r, eu) / _dot(eu, eu), _dot(r, ev) / _dot(ev, ev)
        B[m] = np.minimum(half - np.abs(uu - half), half - np.abs(vv - half))
    # flat shading: distance to the nearest edge in an equilateral parameterisation, 1 at the barycentre
    m = ((flags & MESH_IS_MESH) != 0) & ((flags & MESH_VERTEX_NORMALS) == 0)
    if m.any():
        s3 = dt(1.7320508075688772)
        px, py = u[m] + half * v[m], half * s3 * v[m]
        best = np.full(px.shape, np.inf, dtype=dt)
        for ex, ey, ax, ay in ((one, dt(0.0), dt(0.0), dt(0.0)), (-half, half * s3, one, dt(0.0)), (-half, -half * s3, half, half * s3)):
            vx, vy = px - ax, py - ay
            h = np.minimum(np.maximum((vx * ex + vy * ey) / (ex * ex + ey * ey), dt(0.0)), one)
            qx, qy = vx - ex * h, vy - ey * h
            best = np.minimum(best, qx * qx + qy * qy)
        B[m] = np.sqrt(best) / (s3 / dt(6.0))
    m = ((flags & MESH_IS_MESH) != 0) & ((flags & MESH_VERTEX_NORMALS) != 0)
    if m.any():
        n = nrm[iv[m, 0]] * w[m, None] + nrm[iv[m, 1]] * u[m, None] + nrm[iv[m, 2]] * v[m, None]
        dp = -_dot(n, ray_d[m])
        B[m] = dp * dp
    return B.astype(dt)


class Warps:
    """What stage 2 holds of R requests once their rays are walked: per ray w, dw (3), v (3), inv_dist, tri (-1: miss), b (3) the
    weights of the hit triangle's vertices, w_denom; per request Z, dZ, iZ, sum |dw| and `decided` (every ray is)."""


def collect(sa, cfg, req, dt=np.float64, hits=None):
    """warp_collect of every request.  `hits` = (tri, decided) of an earlier float64 run (the float32 run is given them)."""
    A = aux_rays(cfg, req, dt)
    if hits is None:
        hits = closest_hits(sa, req.o, A["ray_d"])
    tri, decided = hits
    R, rays = tri.shape
    W = Warps()
    W.tri, W.ray_decided, W.decided = tri, decided, decided.all(axis=1)
    one = dt(1.0)
    o = np.repeat(req.o.astype(dt), rays, axis=0)
    d = np.repeat(req.d.astype(dt), rays, axis=0)
    ray_d = A["ray_d"].reshape(-1, 3)
    flat = tri.reshape(-1)
    hit = np.nonzero(flat >= 0)[0]
    B = np.ones(R * rays, dtype=dt)
    vdir = d.copy()
    inv_dist = np.zeros(R * rays, dtype=dt)
    b = np.zeros((R * rays, 3), dtype=dt)
    if hit.size:
        iv = sa.tri[flat[hit]]
        pos = sa.pos.astype(dt)
        p0, p1, p2 = pos[iv[:, 0]], pos[iv[:, 1]], pos[iv[:, 2]]
        e1, e2 = p1 - p0, p2 - p0                                          # mesh.h:343-365 in dt
        pvec = _cross(ray_d[hit], e2)
        inv_det = one / _dot(e1, pvec)
        tvec = o[hit] - p0
        u = _dot(tvec, pvec) * inv_det
        v = _dot(ray_d[hit], _cross(tvec, e1)) * inv_det
        p = p0 * (one - u - v)[:, None] + p1 * u[:, None] + p2 * v[:, None]
        r3 = p - o[hit]
        dist = np.sqrt(_dot(r3, r3))
        inv_dist[hit] = one / dist
        vdir[hit] = r3 * inv_dist[hit][:, None]
        b[hit] = np.stack([one - u - v, u, v], axis=-1)
        B[hit] = _boundary(sa, flat[hit], u, v, ray_d[hit], dt)
    sy_ = A["sy_"].reshape(-1)
    kappa, expo = dt(cfg.kappa), dt(cfg.exponent)
    with np.errstate(under="ignore"):
        inv_vmf = one / (sy_ * np.exp(dt(-2.0) * kappa) + (one - sy_))      # reparam.py:111
    w_denom = inv_vmf - one + B
    with np.errstate(divide="ignore"):
        rcp = np.where(w_denom > dt(W_DENOM_FLOOR), one / w_denom, dt(0.0)).astype(dt)
    w = np.power(rcp, expo) * inv_vmf
    tmp1 = np.clip(inv_vmf * w * rcp * kappa * expo, dt(-1e10), dt(1e10))
    dw = A["tangent"].reshape(-1, 3) * tmp1[:, None]
    sh = lambda a: a.reshape((R, rays) + a.shape[1:]).astype(dt)
    W.w, W.dw, W.v, W.inv_dist, W.b, W.w_denom = sh(w), sh(dw), sh(vdir), sh(inv_dist), sh(b), sh(w_denom)
    W.Z = W.w.sum(axis=1, dtype=dt)
    W.dZ = W.dw.sum(axis=1, dtype=dt)
    W.dZ_abs = np.abs(W.dw).sum(axis=1, dtype=dt)
    W.iZ = one / np.maximum(W.Z, dt(1e-8))
    W.distinct = np.array([np.unique(t[t >= 0]).size for t in tri])
    return W


def _follow_weights(req, dt, absolute=False):
    b1, b2 = req.fb1.astype(dt), req.fb2.astype(dt)
    if absolute:
        return np.stack([dt(1.0) + np.abs(b1) + np.abs(b2), np.abs(b1), np.abs(b2)], axis=-1)
    return np.stack([dt(1.0) - b1 - b2, b1, b2], axis=-1)


# ---------------------------------------------------------------------------- backward
def backward(sa, W, req, dt=np.float64, keep=None):
    """The adjoint of every request with keep[r] (default: all) summed into (V,3) rows -> (rows, A) in dt; A = the same sums of
    absolute values."""
    R, rays = W.tri.shape
    keep = np.ones(R, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    d, g_dir, g_div = req.d.astype(dt), req.gdir.astype(dt), req.gdiv.astype(dt)
    iZ = W.iZ
    g_V = _proj(g_dir, d) * iZ[:, None] - W.dZ * (g_div * iZ * iZ)[:, None]
    g_V_abs = _proj(g_dir, d, True) * iZ[:, None] + W.dZ_abs * np.abs(g_div * iZ * iZ)[:, None]
    g_v = g_V[:, None, :] * W.w[..., None] + W.dw * (g_div * iZ)[:, None, None]
    g_v_abs = g_V_abs[:, None, :] * W.w[..., None] + np.abs(W.dw) * np.abs(g_div * iZ)[:, None, None]
    hit = W.tri >= 0
    g_p = np.where(hit[..., None], _proj(g_v, W.v) * W.inv_dist[..., None], dt(0.0))
    g_p_abs = np.where(hit[..., None], _proj(g_v_abs, W.v, True) * W.inv_dist[..., None], dt(0.0))
    g_d = np.where(hit[..., None], dt(0.0), g_v).sum(axis=1, dtype=dt)
    g_d_abs = np.where(hit[..., None], dt(0.0), g_v_abs).sum(axis=1, dtype=dt)
    g_o = -g_p.sum(axis=1, dtype=dt)
    g_o_abs = g_p_abs.sum(axis=1, dtype=dt)
    em = req.em.astype(dt)
    g_o = g_o - np.where((em != 0)[:, None], _proj(g_d, d) * em[:, None], dt(0.0))
    g_o_abs = g_o_abs + np.where((em != 0)[:, None], _proj(g_d_abs, d, True) * np.abs(em)[:, None], dt(0.0))
    rows, rows_abs = np.zeros((sa.V, 3), dtype=dt), np.zeros((sa.V, 3), dtype=dt)
    # the hit triangles' vertices
    sel = hit & keep[:, None]
    sel &= sa.attached_tri[np.where(hit, W.tri, 0)]
    iv = sa.tri[W.tri[sel]]
    for j in range(3):
        np.add.at(rows, iv[:, j], g_p[sel] * W.b[sel][:, j, None])
        np.add.at(rows_abs, iv[:, j], g_p_abs[sel])                        # (a barycentric weight counts as 1: module docstring)
    # the glued origin
    glued = keep & (req.ftri != NO_TRI)
    glued &= sa.attached_tri[np.where(req.ftri != NO_TRI, req.ftri, 0)]
    iv = sa.tri[req.ftri[glued]]
    fb, fb_abs = _follow_weights(req, dt)[glued], _follow_weights(req, dt, True)[glued]
    for j in range(3):
        np.add.at(rows, iv[:, j], g_o[glued] * fb[:, j, None])
        np.add.at(rows_abs, iv[:, j], g_o_abs[glued] * fb_abs[:, j, None])
    return rows, rows_abs


# ---------------------------------------------------------------------------- forward
def forward(sa, W, req, tan_pos, dt=np.float64):
    """-> d' (R,3), div' (R), A of d' (R,3), A of div' (R) in dt for the vertex tangents tan_pos (V,3)"""
    R, rays = W.tri.shape
    tan = np.asarray(tan_pos).astype(dt)
    d, em = req.d.astype(dt), req.em.astype(dt)
    # the motion of the glued origin (zero on meshes that are not attached, or glued to nothing)
    glued = (req.ftri != NO_TRI) & sa.attached_tri[np.where(req.ftri != NO_TRI, req.ftri, 0)]
    iv = sa.tri[np.where(glued, req.ftri, 0)]
    fb, fb_abs = _follow_weights(req, dt), _follow_weights(req, dt, True)
    t_o = np.where(glued[:, None], sum(tan[iv[:, j]] * fb[:, j, None] for j in range(3)), dt(0.0)).astype(dt)
    t_o_abs = np.where(glued[:, None], sum(np.abs(tan[iv[:, j]]) * fb_abs[:, j, None] for j in range(3)), dt(0.0)).astype(dt)
    hit = W.tri >= 0
    att = hit & sa.attached_tri[np.where(hit, W.tri, 0)]
    ih = sa.tri[np.where(hit, W.tri, 0)]                                   # (R,rays,3)
    t_hit = np.where(att[..., None], sum(tan[ih[..., j]] * W.b[..., j, None] for j in range(3)), dt(0.0)).astype(dt)
    t_hit_abs = np.where(att[..., None], sum(np.abs(tan[ih[..., j]]) for j in range(3)), dt(0.0)).astype(dt)
    dp, dp_abs = t_hit - t_o[:, None, :], t_hit_abs + t_o_abs[:, None, :]
    tv_hit = _proj(dp, W.v) * W.inv_dist[..., None]
    tv_hit_abs = _proj(dp_abs, W.v, True) * W.inv_dist[..., None]
    # a miss follows ray.d, which moves only for an emitter ray
    tv_miss = np.where((em != 0)[:, None], _proj(t_o, d) * (-em)[:, None], dt(0.0))[:, None, :]
    tv_miss_abs = np.where((em != 0)[:, None], _proj(t_o_abs, d, True) * np.abs(em)[:, None], dt(0.0))[:, None, :]
    tv = np.where(hit[..., None], tv_hit, tv_miss).astype(dt)
    tv_abs = np.where(hit[..., None], tv_hit_abs, tv_miss_abs).astype(dt)
    iZ = W.iZ
    S = (tv * W.w[..., None]).sum(axis=1, dtype=dt)
    S_abs = (tv_abs * W.w[..., None]).sum(axis=1, dtype=dt)
    ddir = _proj(S, d) * iZ[:, None]
    ddir_abs = _proj(S_abs, d, True) * iZ[:, None]
    c = W.dw - W.dZ[:, None, :] * (iZ[:, None] * W.w)[..., None]
    c_abs = np.abs(W.dw) + W.dZ_abs[:, None, :] * (iZ[:, None] * W.w)[..., None]
    div = _dot(c, tv).sum(axis=1, dtype=dt) * iZ
    div_abs = _dot(c_abs, tv_abs).sum(axis=1, dtype=dt) * iZ
    return ddir.astype(dt), div.astype(dt), ddir_abs.astype(dt), div_abs.astype(dt)


# ---------------------------------------------------------------------------- the workspace (epsm_trace_reparam_workspace_bytes)
def request_bytes(n):
    return (n * MAX_REQ * REQ_WORDS * 4 + 255) & ~255


def workspace_bytes(n):
    return request_bytes(n) + 4 * n if n > 0 else 0


POISON = 0x7FC00BAD                      # a NaN: a slot nothing may read into a result or write


def pack_workspace(n_paths, req, count, gdir=None, gdiv=None):
    """The workspace as int32 words: every slot poisoned, then the requests (word layout of rp::WarpReq) and the counts.
    gdir / gdiv override the requests' own (None: theirs)."""
    words = np.full(workspace_bytes(n_paths) // 4, POISON, dtype=np.int32)
    slots = words[: n_paths * MAX_REQ * REQ_WORDS].reshape(MAX_REQ, n_paths, REQ_WORDS)
    f = slots.view(np.float32)
    gdir = req.gdir if gdir is None else np.asarray(gdir, dtype=np.float32)
    gdiv = req.gdiv if gdiv is None else np.asarray(gdiv, dtype=np.float32)
    k = (req.n, req.path)
    for j in range(3):
        f[k + (j,)], f[k + (4 + j,)], f[k + (8 + j,)] = req.o[:, j], req.d[:, j], gdir[:, j]
    f[k + (3,)], f[k + (7,)], f[k + (11,)], f[k + (13,)] = gdiv, req.em, req.fb1, req.fb2
    slots[k + (12,)] = req.ftri.astype(np.uint32).view(np.int32)
    slots[k + (14,)] = 0
    slots[k + (15,)] = 0
    words[request_bytes(n_paths) // 4:] = np.asarray(count, dtype=np.int32)
    return words


def unpack_slots(words, n_paths):
    return words[: n_paths * MAX_REQ * REQ_WORDS].reshape(MAX_REQ, n_paths, REQ_WORDS)
