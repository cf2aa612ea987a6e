"""Ray queries against the tracer's own BVH traversal (epsm_probe_rays, include/epsm_trace.h): adversarial trees, ray families
no sensor produces, a brute-force float64 checker that accounts for EVERY ray, and a restatement of the ordered walk's stack
bookkeeping that measures how deep the traversal stack gets.  Test infrastructure (tests/test_ray_query.py on the host build
of the traversal, tests/test_gpu_ray_query.py on the device); nothing here shares code with csrc/epsm_trace_core.h.

The checker.  Every ray is tested against every triangle with mesh.h:343-365's formulas in float64, twice: TIGHTENED by a
relative margin EPS (u, v >= EPS, u + v <= 1 - EPS, 0 < t <= maxt (1 - EPS)) and WIDENED by it (u, v >= -EPS, u + v <= 1 + EPS,
0 < t <= maxt (1 + EPS)).  A closest-hit ray is DECIDED when both name the same closest triangle and no other widened candidate
lies within t (1 + EPS) of it, or when neither finds anything; the traversal must then report exactly that.  On an undecided
ray it must still report one of the widened candidates no farther than the tightened winner's t (1 + EPS) (or, when the
tightened test finds nothing, one of the widened candidates or a miss).  Any-hit rays are decided `occluded` when a triangle
passes the tightened test and `free` when none passes the widened one.  Zero-area triangles are never candidates.  The share
of undecided rays is a property of the fixture alone and is capped (UNDECIDED_CAP) before any traversal is looked at."""
import ctypes as C
import functools

import numpy as np
import torch

from epsm_mitsuba3_amd import scene as S
from test_bvh_build import _soup

EPS = 2e-4                  # relative margin of the two tests and the tolerance of t: the tie tolerance of _trace_replay.replay
UV_TOL = 5e-3               # _trace_replay.replay's tolerance of the barycentrics
UNDECIDED_CAP = 0.10
MISS = 0xffffffff
ABSENT = 0x7fffffff
K_INF = np.float32(3.402823466e+38)      # the tracer's kInf
LANE, LANE_ANY, WAVEFRONT, WAVEFRONT_ANY, PACKET = range(5)
ANY_HIT = {LANE: False, LANE_ANY: True, WAVEFRONT: False, WAVEFRONT_ANY: True, PACKET: False}
SIZES = (1, 63, 64, 65, 200)             # and the whole family: partial waves, partial workgroups
K_BVH_STACK, K_WF_STACK_LDS, K_LANE_STACK_LDS = 48, 16, 32     # csrc: kBvhStack, kWfStackLds, kLaneStackLds


# ---------------------------------------------------------------------------- geometry: (pos (V,3) float64 holding float32 values, tri (T,3))
def _f32(pos):
    return np.ascontiguousarray(pos, dtype=np.float32).astype(np.float64)


CHAIN_SCALE = 2.0 ** 36


def chain():
    """test_bvh_build's geometric chain: 1 500 triangles of size 2^-i/25 at distance 2^-i/25 from the corner (0, 0, 0) --
    SCALED by 2^36 (exact; the same tree, the same walk).  From the corner Moeller-Trumbore's numerators are products of three
    lengths, about 0.009 s^3 for the triangle of scale s: unscaled (2^0 .. 2^-60) they leave float32's normal range below
    s = 2^-32, t underflows to 0 and every such triangle the ray crosses is a `hit at t = 0` -- in mesh.h's float32 formula
    itself, which is not what these tests are about.  Scaled, the chain spans 2^36 .. 2^-24 and 0.009 s^3 stays inside
    [2^-79, 2^102]."""
    rng = np.random.default_rng(1)
    t = 1500
    s = 2.0 ** (-np.arange(t) / 25.0)
    pos, tri = _soup(np.stack([s * 3.0, s * 2.0, s], axis=1), 0.05 * s, rng)
    return _f32(pos * CHAIN_SCALE), tri


def uniform():
    """test_bvh_build's uniform soup: 4 000 triangles of size 0.02 in [-1, 1]^3."""
    rng = np.random.default_rng(3)
    t = 4000
    pos, tri = _soup(rng.uniform(-1, 1, size=(t, 3)), np.full(t, 0.02), rng)
    return _f32(pos), tri


def one_centroid(t=20000):
    """test_gpu_bvh_device's one-centroid soup (every box centred on the origin exactly), at 20 000 triangles."""
    rng = np.random.default_rng(9)
    e = rng.integers(1, 1000, size=(t, 3))
    d = np.empty((t, 3, 3), dtype=np.int64)
    d[:, 0], d[:, 1] = -e, e
    d[:, 2] = rng.integers(-e, e + 1)
    return _f32((d * 1e-3).reshape(-1, 3)), np.arange(3 * t, dtype=np.int64).reshape(t, 3)


def small(t):
    """test_gpu_bvh_device's T = 1..7: a single node."""
    rng = np.random.default_rng(100 + t)
    pos, tri = _soup(rng.uniform(-1, 1, size=(t, 3)), np.full(t, 0.1), rng)
    return _f32(pos), tri


def degenerate():
    """The uniform soup with 50 zero-area triangles mixed in, on small integer coordinates (exact in float32): 25 with two
    equal corners, 25 with three collinear corners."""
    pos, tri = uniform()
    rng = np.random.default_rng(17)
    a = rng.integers(-1, 2, size=(50, 3))
    e = rng.integers(-1, 2, size=(50, 3))
    e[(e == 0).all(axis=1)] = (1, 0, 0)
    corners = np.stack([a - e, a, a + e], axis=1).astype(np.float64)        # collinear ...
    corners[:25, 1] = corners[:25, 0]                                       # ... or two equal corners
    t0 = tri.shape[0]
    where = np.sort(rng.choice(t0 + 50, size=50, replace=False))            # their places in the triangle list
    verts = np.empty((t0 + 50, 3, 3))
    keep = np.ones(t0 + 50, dtype=bool); keep[where] = False
    verts[keep] = pos[tri]; verts[where] = corners
    return verts.reshape(-1, 3), np.arange(3 * (t0 + 50), dtype=np.int64).reshape(-1, 3)


GEOMETRY = {"chain": chain, "uniform": uniform, "one_centroid": one_centroid, "degenerate": degenerate,
            **{f"T{t}": functools.partial(small, t) for t in range(1, 8)}}


@functools.lru_cache(maxsize=None)
def geometry(name):
    pos, tri = GEOMETRY[name]()
    pos.setflags(write=False); tri.setflags(write=False)
    return pos, tri


def triangle_verts(name):
    pos, tri = geometry(name)
    return pos[tri]                                                        # (T,3,3) float64 of the float32 corners


def zero_area(verts):
    e1, e2 = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    return (np.cross(e1, e2) == 0.0).all(axis=1)


# ---------------------------------------------------------------------------- trees and the scene struct the probe reads
class Tree:
    """nodes (n,32) float32, prim_index (T) int32 and tri_verts (T,9) float32 on ``device`` + the EpsmScene naming them."""

    def __init__(self, bvh, device):
        self.bvh, self.device = bvh, torch.device(device)
        self.struct = S.EpsmSceneC()
        self.refresh()

    def refresh(self):
        b = self.bvh
        self.struct.bvh, self.struct.n_nodes = b.nodes.data_ptr(), int(b.nodes.shape[0])
        self.struct.prim_index, self.struct.tri_verts = b.prim_index.data_ptr(), b.tri_verts.data_ptr()
        self.struct.n_triangles = int(b.prim_index.shape[0])

    def host_nodes(self):
        return self.bvh.nodes.detach().cpu().numpy().copy()

    def host_tri_verts(self):
        return self.bvh.tri_verts.detach().cpu().numpy().astype(np.float64).reshape(-1, 3, 3)

    def refit(self, pos, tri):
        p = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).to(self.device)
        t = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32)).to(self.device)
        self.bvh.refit(p, t)
        self.refresh()


class EmptyTree:
    """A scene without triangles: n_nodes == 0, every table NULL."""
    device = None

    def __init__(self, device):
        self.device = torch.device(device)
        self.struct = S.EpsmSceneC()


def build_tree(name, builder="host", device="cpu"):
    pos, tri = geometry(name)
    p = torch.from_numpy(pos.astype(np.float32)).to(device)
    t = torch.from_numpy(tri.astype(np.int32)).to(device)
    if builder == "device":
        from epsm_mitsuba3_amd.bvh import NativeBvh
        return Tree(NativeBvh(p, t), device)
    bvh = S.DeviceBvh(S.build_bvh(pos, tri), device)
    bvh.refit(p, t)
    return Tree(bvh, device)


# ---------------------------------------------------------------------------- the probe
def declare(lib):
    lib.epsm_probe_rays.restype = C.c_int
    lib.epsm_probe_rays.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.epsm_probe_rays_workspace_bytes.restype = C.c_size_t
    lib.epsm_probe_rays_workspace_bytes.argtypes = [C.c_int, C.c_int64]
    return lib


def probe(lib, tree, form, rays):
    """rays (n,8) float32 numpy -> (n,4) uint32 numpy: triangle id or MISS, then the bits of t, u, v."""
    from epsm_mitsuba3_amd import _lib
    dev = tree.device
    n = rays.shape[0]
    r = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).to(dev)
    out = torch.full((max(n, 1), 4), 0x55555555, dtype=torch.int32, device=dev)
    need = int(lib.epsm_probe_rays_workspace_bytes(form, n))
    ws = torch.full((max(need, 4) // 4,), 0x7f7f7f7f, dtype=torch.int32, device=dev)      # junk, never a valid reference by luck
    rc = lib.epsm_probe_rays(C.byref(tree.struct), form, n, r.data_ptr(), out.data_ptr(), ws.data_ptr(), need, _lib.stream(dev))
    assert rc == 0, rc
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return out[:n].cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------- ray families: (n,8) float32 rows o, d, maxt, mask
def _rows(o, d, maxt=None):
    n = o.shape[0]
    r = np.empty((n, 8), dtype=np.float32)
    r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6] = K_INF if maxt is None else maxt
    r[:, 7] = 1.0
    return r


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _inside_points(verts, n, rng, ids=None):
    """a barycentric point in [0.05, 0.9]^3 (normalised) of n random triangles with an area (or of triangles `ids`)"""
    if ids is None:
        ids = rng.choice(np.nonzero(~zero_area(verts))[0], size=n)
    w = rng.uniform(0.05, 0.9, size=(n, 3))
    w /= w.sum(axis=1, keepdims=True)
    return (verts[ids] * w[:, :, None]).sum(axis=1)


def _well_conditioned(verts, reach):
    """triangles whose shortest edge AND shortest altitude are >= reach / 10^3: float32's own error in u, v (2^-24 x distance /
    that length) then stays an order of magnitude under the margin for any origin within `reach`"""
    e = np.stack([verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 1], verts[:, 0] - verts[:, 2]], axis=1)
    length = np.linalg.norm(e, axis=2)
    area2 = np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        altitude = np.where(length.max(axis=1) > 0, area2 / length.max(axis=1), 0.0)
    return np.nonzero((length.min(axis=1) >= reach * 1e-3) & (altitude >= reach * 1e-3))[0]


def interior_rays(name, n=2048, radius=3.0):
    """Origins on a shell of radius 3 around the soup (which lies in [-1, 1]^3, or [-2, 2]^3 with the zero-area triangles),
    aimed at an inside point of a random triangle.  Conditioning: the aimed triangle's shortest edge and altitude are >= 2 radius
    / 10^3 and the ray meets its plane at cos >= 0.3 (at grazing incidence float32's error in t, u, v grows as 1 / cos).
    Undecided share, from the oracle alone: uniform soup 0.0 %, one-centroid soup 1.9 %, uniform soup with zero-area
    triangles 0.0 %, T = 1..7 0.0 % (any-hit rule: 0.0 % everywhere)."""
    rng = np.random.default_rng(41)
    verts = triangle_verts(name)
    ids = rng.choice(_well_conditioned(verts, 2 * radius), size=n)
    target = _inside_points(verts, n, rng, ids)
    normal = _unit(np.cross(verts[ids, 1] - verts[ids, 0], verts[ids, 2] - verts[ids, 0])) * rng.choice([-1.0, 1.0], size=(n, 1))
    helper = np.where(np.abs(normal[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    a = _unit(np.cross(normal, helper)); b = np.cross(normal, a)
    cos, phi = rng.uniform(0.3, 1.0, size=(n, 1)), rng.uniform(0, 2 * np.pi, size=(n, 1))
    away = normal * cos + np.sqrt(1 - cos * cos) * (np.cos(phi) * a + np.sin(phi) * b)       # from the target to the origin
    along = (target * away).sum(axis=1)
    s = -along + np.sqrt(along * along - (target * target).sum(axis=1) + radius * radius)    # |target + s away| = radius
    o = (target + s[:, None] * away).astype(np.float32).astype(np.float64)
    return _rows(o, _unit(target - o))


def deep_rays(n=2048):
    """The geometric chain seen from its corner: origin EXACTLY (0, 0, 0); half the rays in a cone of 0.02 rad about (3, 2, 1),
    half aimed at inside points of random chain triangles.  Only from the corner is the chain (2^0 .. 2^-60) scale-free, which
    keeps float32 Moeller-Trumbore well conditioned.
    Undecided share, from the oracle alone: 0.3 % (cone: 0.3 %, aimed: 0.3 %); 99.7 % of the rays have a decided hit."""
    rng = np.random.default_rng(42)
    verts = triangle_verts("chain")
    a = np.array([3.0, 2.0, 1.0]) / np.sqrt(14.0)
    u = _unit(np.cross(a, [0.0, 0.0, 1.0])); v = np.cross(a, u)
    h = n // 2
    rad, phi = 0.02 * np.sqrt(rng.uniform(size=h)), rng.uniform(0, 2 * np.pi, size=h)
    cone = _unit(a + np.tan(rad)[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v))
    aimed = _unit(_inside_points(verts, n - h, rng))
    return _rows(np.zeros((n, 3)), np.concatenate([cone, aimed]))


def _axis_directions():
    out = []
    for k in range(3):
        for sign in (1.0, -1.0):
            for za in (0.0, -0.0):
                for zb in (0.0, -0.0):
                    d = np.empty(3, dtype=np.float32)
                    d[k], d[(k + 1) % 3], d[(k + 2) % 3] = sign, za, zb
                    out.append((k, sign, d))
    return out                                                              # 24: +-e_k with every sign of the two zeros


def axis_rays(nodes):
    """Directions exactly +-e_x, +-e_y, +-e_z with +0.0 and -0.0 in the other two components.  First set: origins on a 9 x 9
    lattice on the face x_k = -+3 outside the soup's box.  Second set: one coordinate along a zero-direction axis is the bits of
    a lo / hi plane of a node of the tree under test, so that the ray lies IN a slab plane.  2 x 1 944 rows.
    Undecided share, from the oracle alone (uniform soup, host builder's tree): lattice 0.0 %, in-plane 0.3 %; a third of
    the rays hit something."""
    rng = np.random.default_rng(43)
    lat = np.linspace(-0.95, 0.95, 9).astype(np.float32)
    boxes = np.asarray(nodes, dtype=np.float32)[:, 0:24].reshape(-1, 2, 3, 4)      # (node, lo / hi, axis, slot)
    refs = np.asarray(nodes, dtype=np.float32).view(np.int32)[:, 24:28]
    first, second = [], []
    for k, sign, d in _axis_directions():
        a, b = (k + 1) % 3, (k + 2) % 3
        o = np.empty((81, 3), dtype=np.float32)
        o[:, k] = -3.0 * sign
        o[:, a], o[:, b] = np.repeat(lat, 9), np.tile(lat, 9)
        first.append(_rows(o, np.broadcast_to(d, (81, 3))))
        o = o.copy()
        node = rng.integers(0, boxes.shape[0], size=81)
        slot = rng.integers(0, 4, size=81)
        ok = refs[node, slot] != ABSENT                                    # (an absent child's box is +-inf: keep the lattice value)
        plane = boxes[node, rng.integers(0, 2, size=81), a, slot]
        o[ok, a] = plane[ok]
        o[:, b] = rng.uniform(-1, 1, size=81).astype(np.float32)
        second.append(_rows(o, np.broadcast_to(d, (81, 3))))
    return np.concatenate(first), np.concatenate(second)


def limit_rays(rays, oracle, n=1024):
    """The first 1 024 interior rays with a decided first hit, each twice: maxt = 1/2 and 2 x the float64 distance of that hit
    (cut in front of it: a miss; behind it: the hit).  Run under the any-hit forms as well.
    Undecided share, from the oracle alone: uniform soup 0.0 %, one-centroid soup 0.0 %."""
    c = oracle.classify(False)
    ids = np.nonzero(c.decided & (c.tri >= 0))[0][:n]
    half, twice = rays[ids].copy(), rays[ids].copy()
    half[:, 6] = (0.5 * c.t[ids]).astype(np.float32)
    twice[:, 6] = (2.0 * c.t[ids]).astype(np.float32)
    return np.concatenate([half, twice]), np.concatenate([ids, ids])


# ---------------------------------------------------------------------------- the oracle: every ray x every triangle, float64
def moeller_trumbore(o, d, p0, p1, p2):
    """mesh.h:343-365 in float64 on broadcastable (.., 3) arrays -> t, u, v (inf / NaN where the determinant vanishes)."""
    e1, e2 = p1 - p0, p2 - p0
    pvec = np.cross(d, e2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_det = 1.0 / (e1 * pvec).sum(axis=-1)
        tvec = o - p0
        u = (tvec * pvec).sum(axis=-1) * inv_det
        qvec = np.cross(tvec, e1)
        v = (d * qvec).sum(axis=-1) * inv_det
        t = (e2 * qvec).sum(axis=-1) * inv_det
    return t, u, v


def _moeller_trumbore_pairs(o, d, verts):
    """the same for every pair of c rays and T triangles, component by component (no (c, T, 3) temporaries) -> (c, T) each"""
    p0 = [verts[None, :, 0, k] for k in range(3)]
    e1 = [verts[None, :, 1, k] - p0[k] for k in range(3)]
    e2 = [verts[None, :, 2, k] - p0[k] for k in range(3)]
    dd = [d[:, k, None] for k in range(3)]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pvec = cross(dd, e2)
        inv_det = 1.0 / dot(e1, pvec)
        tvec = [o[:, k, None] - p0[k] for k in range(3)]
        u = dot(tvec, pvec) * inv_det
        qvec = cross(tvec, e1)
        return dot(e2, qvec) * inv_det, u, dot(dd, qvec) * inv_det


class Verdict:
    """Per ray: decided (n) bool; the decided answer tri (n) (-1 = miss / free; for any-hit -2 = occluded), t, u, v; and for
    every ray the list `allowed` of triangles an undecided ray may still report, with allow_miss (n)."""


class Oracle:
    """The widened candidates of n rays against T triangles (maxt not yet applied) and their float64 (t, u, v)."""

    def __init__(self, rays, verts, chunk=64):
        rays = np.asarray(rays, dtype=np.float32)
        self.n = rays.shape[0]
        self.maxt = rays[:, 6].astype(np.float64)
        o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
        live = ~zero_area(verts)
        self.cand = []                                                     # per ray: (tri, t, u, v, tight) sorted by t
        for a in range(0, self.n, chunk):
            t, u, v = _moeller_trumbore_pairs(o[a:a + chunk], d[a:a + chunk], verts)
            with np.errstate(invalid="ignore"):
                wide = live[None] & (u >= -EPS) & (v >= -EPS) & (u + v <= 1 + EPS) & (t > 0)
                tight = (u >= EPS) & (v >= EPS) & (u + v <= 1 - EPS)
            for r in range(wide.shape[0]):
                ids = np.nonzero(wide[r])[0]
                ids = ids[np.argsort(t[r, ids], kind="stable")]
                self.cand.append((ids, t[r, ids], u[r, ids], v[r, ids], tight[r, ids]))

    def with_maxt(self, maxt, ids=None):
        """The same rays (or rows `ids` of them) under other limits: no new arithmetic."""
        o = object.__new__(Oracle)
        ids = np.arange(self.n) if ids is None else np.asarray(ids)
        o.n, o.maxt, o.cand = ids.shape[0], np.asarray(maxt, dtype=np.float32).astype(np.float64), [self.cand[i] for i in ids]
        return o

    def take(self, ids, mask=None):
        """Rows `ids`; a row whose mask is False carries no ray: it has no candidates and must report a miss."""
        o = self.with_maxt(self.maxt[np.asarray(ids)], ids)
        if mask is not None:
            none = (np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, bool))
            o.cand = [c if m else none for c, m in zip(o.cand, mask)]
        return o

    @staticmethod
    def concat(parts):
        o = object.__new__(Oracle)
        o.n, o.maxt, o.cand = sum(p.n for p in parts), np.concatenate([p.maxt for p in parts]), sum((p.cand for p in parts), [])
        return o

    def classify(self, any_hit):
        cache = self.__dict__.setdefault("_verdicts", {})
        if any_hit not in cache:
            cache[any_hit] = self._classify(any_hit)
        return cache[any_hit]

    def _classify(self, any_hit):
        c = Verdict()
        n = self.n
        c.decided = np.zeros(n, dtype=bool); c.tri = np.full(n, -1, dtype=np.int64)
        c.t, c.u, c.v = np.zeros(n), np.zeros(n), np.zeros(n)
        c.allowed, c.allow_miss = [None] * n, np.zeros(n, dtype=bool)
        for r, (ids, t, u, v, tight) in enumerate(self.cand):
            w = t <= self.maxt[r] * (1 + EPS)
            ti = tight & (t <= self.maxt[r] * (1 - EPS))
            ids_w, t_w = ids[w], t[w]
            if not w.any():                                                # neither test finds anything
                c.decided[r] = True
            elif any_hit:
                c.decided[r] = bool(ti.any())
                c.tri[r] = -2 if ti.any() else -1
                c.allowed[r] = (ids_w, t_w); c.allow_miss[r] = not ti.any()
            elif not ti.any():
                c.allowed[r] = (ids_w, t_w); c.allow_miss[r] = True
            else:
                k = int(np.argmax(ti))                                     # the tightened winner (sorted by t)
                near = w & (t <= t[k] * (1 + EPS))
                if ids_w[0] == ids[k] and near.sum() == 1:
                    c.decided[r] = True
                    c.tri[r], c.t[r], c.u[r], c.v[r] = ids[k], t[k], u[k], v[k]
                else:
                    c.allowed[r] = (ids[near], t[near])
        return c

    def undecided_share(self, any_hit=False):
        return float(1.0 - self.classify(any_hit).decided.mean()) if self.n else 0.0


def check(oracle, out, any_hit, n=None):
    """out (n,4) uint32 of the probe against the oracle's first n rays.  Returns dict(unexplained = [(ray, why)], rel_t, du, dv =
    the worst deviations on decided hits, decided, undecided).  The caller asserts that `unexplained` is empty."""
    c = oracle.classify(any_hit)
    n = oracle.n if n is None else n
    assert out.shape == (n, 4)
    tri = out[:, 0].astype(np.int64); tri[out[:, 0] == MISS] = -1
    t, u, v = (out[:, j].copy().view(np.float32).astype(np.float64) for j in (1, 2, 3))
    bad = []
    worst = {"rel_t": 0.0, "du": 0.0, "dv": 0.0}
    for r in range(n):
        if c.decided[r] and c.tri[r] == -1:
            if tri[r] != -1:
                bad.append((r, f"reports triangle {tri[r]} at t = {t[r]:.9g}; the oracle: nothing even with the margin"))
        elif c.decided[r] and not any_hit:
            rel = abs(t[r] - c.t[r]) / c.t[r]
            if tri[r] != c.tri[r]:
                bad.append((r, f"reports {tri[r]} (t = {t[r]:.9g}); the oracle: {c.tri[r]} at {c.t[r]:.9g}, no tie"))
            elif not (rel <= EPS and abs(u[r] - c.u[r]) <= UV_TOL and abs(v[r] - c.v[r]) <= UV_TOL):
                bad.append((r, f"triangle {tri[r]}: t, u, v = {t[r]:.9g}, {u[r]:.6g}, {v[r]:.6g}; the oracle: {c.t[r]:.9g}, {c.u[r]:.6g}, {c.v[r]:.6g}"))
            else:
                worst["rel_t"] = max(worst["rel_t"], rel)
                worst["du"] = max(worst["du"], abs(u[r] - c.u[r])); worst["dv"] = max(worst["dv"], abs(v[r] - c.v[r]))
        else:                                                              # undecided, or any-hit `occluded`
            ids, ts = c.allowed[r]
            if tri[r] == -1:
                if not c.allow_miss[r]:
                    bad.append((r, f"reports a miss; the oracle: triangle {ids[0]} at t = {ts[0]:.9g} inside the margin"))
            elif tri[r] not in ids:
                bad.append((r, f"reports {tri[r]} (t = {t[r]:.9g}): not among the candidates {ids.tolist()[:8]}"))
            elif any_hit and not abs(t[r] - ts[list(ids).index(tri[r])]) <= EPS * ts[list(ids).index(tri[r])]:
                bad.append((r, f"occluder {tri[r]}: t = {t[r]:.9g}; the oracle: {ts[list(ids).index(tri[r])]:.9g}"))
    return {"unexplained": bad, **worst, "decided": int(c.decided[:n].sum()), "undecided": int(n - c.decided[:n].sum())}


# ---------------------------------------------------------------------------- reach: how deep the ordered walk's stack gets
def peak_stack_depth(nodes, tri_verts, rays):
    """trav_round's push / pop bookkeeping (csrc/epsm_trace_core.h) restated for all rays side by side: float32 slab distances
    (the fma as a float64 product-sum rounded once), children entered nearest first, the others pushed farthest first, maxt cut
    by the hits of the float64 test.  Returns the peak number of stack entries per ray."""
    f = np.float32
    nodes = np.asarray(nodes, dtype=f); refs = nodes.view(np.int32)[:, 24:28].astype(np.int64)
    tv = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 3, 3)
    n = rays.shape[0]
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    with np.errstate(divide="ignore"):
        inv = np.clip(f(1) / rays[:, 3:6].astype(f), f(-1e18), f(1e18)).astype(np.float64)
    noid = (-(rays[:, 0:3].astype(f)) * inv.astype(f)).astype(f).astype(np.float64)
    maxt = rays[:, 6].astype(f)
    cur = np.where(rays[:, 7] != 0, 0 if nodes.shape[0] else ABSENT, ABSENT).astype(np.int64)
    stack = np.zeros((n, K_BVH_STACK), dtype=np.int64); sp = np.zeros(n, dtype=np.int64); peak = np.zeros(n, dtype=np.int64)

    def pop(idx):
        has = sp[idx] > 0
        sp[idx] -= has
        cur[idx] = np.where(has, stack[idx, sp[idx]], ABSENT)

    while True:
        inner = np.nonzero((cur >= 0) & (cur != ABSENT))[0]
        leaf = np.nonzero(cur < 0)[0]
        if inner.size == 0 and leaf.size == 0:
            return peak
        if inner.size:
            nd = nodes[cur[inner]].astype(np.float64)
            lo = (nd[:, 0:12].reshape(-1, 3, 4) * inv[inner, :, None] + noid[inner, :, None]).astype(f)     # (k, axis, slot)
            hi = (nd[:, 12:24].reshape(-1, 3, 4) * inv[inner, :, None] + noid[inner, :, None]).astype(f)
            t0 = np.maximum(np.fmin(lo, hi).max(axis=1), f(0))
            t1 = np.minimum((np.fmax(lo, hi).min(axis=1) * f(1.0000004)).astype(f), maxt[inner, None])
            c = refs[cur[inner]]
            hit = (t0 <= t1) & (c != ABSENT)
            order = np.argsort(np.where(hit, t0, K_INF), axis=1, kind="stable")
            c = np.take_along_axis(np.where(hit, c, ABSENT), order, axis=1)
            for j in (3, 2, 1):
                push = (c[:, j] != ABSENT) & (sp[inner] < K_BVH_STACK)
                stack[inner[push], sp[inner[push]]] = c[push, j]
                sp[inner[push]] += 1
            peak[inner] = np.maximum(peak[inner], sp[inner])
            down = c[:, 0] != ABSENT
            cur[inner[down]] = c[down, 0]
            pop(inner[~down])
        if leaf.size:
            ref = ~cur[leaf]
            first, count = ref >> 3, ref & 7
            for j in range(7):
                m = j < count
                if not m.any():
                    break
                ids, e = leaf[m], first[m] + j
                t, u, v = moeller_trumbore(o[ids], d[ids], tv[e, 0], tv[e, 1], tv[e, 2])
                with np.errstate(invalid="ignore"):
                    h = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= maxt[ids])
                maxt[ids[h]] = t[h].astype(f)
            pop(leaf)


# ---------------------------------------------------------------------------- what the two test files share, computed once
@functools.lru_cache(maxsize=None)
def interior_family(name, n=2048):
    rays = interior_rays(name, n)
    return rays, Oracle(rays, triangle_verts(name))


@functools.lru_cache(maxsize=None)
def deep_family():
    rays = deep_rays()
    return rays, Oracle(rays, triangle_verts("chain"))


@functools.lru_cache(maxsize=None)
def limit_family(name):
    rays, oracle = interior_family(name)
    lim, ids = limit_rays(rays, oracle)
    return lim, oracle.with_maxt(lim[:, 6], ids)


def axis_family(name, nodes):
    """(rays, oracle) of the lattice set and of the in-plane set for the tree whose nodes these are"""
    verts = triangle_verts(name)
    return [(r, Oracle(r, verts)) for r in axis_rays(nodes)]


def packet_rows(families, n=2048, seed=5):
    """Rows of several families of ONE tree, shuffled so that the 64 lanes of a wave are incoherent: (rays, oracle)."""
    rays = np.concatenate([r for r, _ in families])
    oracle = Oracle.concat([o for _, o in families])
    ids = np.random.default_rng(seed).permutation(rays.shape[0])[:n]
    return rays[ids], oracle.take(ids)


def masked(rays, oracle, mask):
    r = rays.copy()
    r[:, 7] = mask
    return r, oracle.take(np.arange(oracle.n), mask)


def families(name, nodes):
    """The ray families of the tree `name` whose nodes these are: {family: (rays, oracle)}."""
    if name == "chain":
        return {"deep": deep_family()}
    if name.startswith("T"):
        return {"interior": interior_family(name, 256)}
    out = {"interior": interior_family(name)}
    if name in ("uniform", "one_centroid"):
        out["limits"] = limit_family(name)
    if name in ("uniform", "degenerate"):
        out["axis_lattice"], out["axis_in_plane"] = axis_family(name, nodes)
    return out


def empty_family(n=200):
    rays = interior_rays("uniform", n)
    return rays, Oracle(rays, np.zeros((0, 3, 3)))


def account(lib, tree, rays, oracle, forms, sizes=SIZES, label=""):
    """Runs the family at every size under every form and returns the worst deviations; raises when a ray is unexplained."""
    worst = {"rel_t": 0.0, "du": 0.0, "dv": 0.0}
    outs = {}
    for form in forms:
        for n in sorted(set(min(s, rays.shape[0]) for s in sizes) | {rays.shape[0]}):
            out = probe(lib, tree, form, rays[:n])
            res = check(oracle, out, ANY_HIT[form], n)
            assert not res["unexplained"], (f"{label} form {form} n = {n}: {len(res['unexplained'])} unexplained rays of {n}, "
                                            f"first: {res['unexplained'][:4]}")
            for k in worst:
                worst[k] = max(worst[k], float(res[k]))
        outs[form] = out
    print(f"{label}: forms {list(forms)}, {rays.shape[0]} rays, {res['undecided']} undecided; worst |dt|/t = {worst['rel_t']:.3g}, "
          f"|du| = {worst['du']:.3g}, |dv| = {worst['dv']:.3g}")
    return worst, outs
