"""d / d eta of the manifold constraint against Snell's law itself -- a check that shares nothing with the code under test.

One hand-built path through a flat slab: camera, a vertex on each face (flat triangles; eta = n entering, 1 / n leaving), a
diffuse end point; variant `manifold`, K = 3.  The barycentrics that satisfy the half-vector constraint
C_k = [normalize(T(n_k)(wi + eta_k wo))]_xy = 0 -- Snell's law -- are found by Newton in float64 numpy, and the expected gradients are
finite differences of that solution with camera and end point fixed:

    g_eta_k = dlduv . (uv(eta_k + h) - uv(eta_k - h)) / 2h,  h = 1e-5
    g_ior   = g_eta_1 (1 / ext) + g_eta_2 (-ext / int^2)          (eta_1 = int / ext, eta_2 = ext / int)

The float64 host build of epsm_cp_core.h (tests/host_harness/cp_ior_host.cpp) must match to 1e-6 relative: the truncation of the
central difference is ~h^2 = 1e-10 relative, Newton converges to ~1e-13, round-off is ~eps / h = 2e-11 -- all far below it.
dlduv is small enough that no term reaches the 0.1 clamp.  The same for a tilted slab (normals along no axis) and for a path
with a reflection vertex in the chain, whose row must be exactly 0 after the chain factor d eta / d int_ior = 0."""
import numpy as np
import pytest
import torch

from _ior_host import host_ior_calc_grad, ior_row_values
from epsm_mitsuba3_amd.synth import FLAGS_DIELECTRIC, FLAGS_DIFFUSE

H = 1e-5


def _unit(v):
    return v / np.linalg.norm(v)


def _constraint(xp, x, xn, n, eta):
    """[normalize(T(n)(wi + eta wo))]_xy with the frame t = (0, -n_z, n_y) / |.|, bt = n x t of a unit normal n."""
    nn = _unit(n)
    t = _unit(np.array([0.0, -nn[2], nn[1]]))
    bt = np.cross(nn, t)
    u = _unit(_unit(xp - x) + eta * _unit(xn - x))
    return np.array([t @ u, bt @ u])


class Chain:
    """camera, `len(tris)` specular vertices on flat triangles, a fixed end point"""

    def __init__(self, cam, tris, normals, end):
        self.cam, self.tris, self.normals, self.end = np.asarray(cam, float), [np.asarray(t, float) for t in tris], normals, np.asarray(end, float)
        self.m = len(tris)

    def point(self, k, uv):
        p0, p1, p2 = self.tris[k]
        return p0 * uv[0] + p1 * uv[1] + p2 * (1.0 - uv[0] - uv[1])

    def residual(self, uv, etas):
        uv = uv.reshape(self.m, 2)
        xs = [self.cam] + [self.point(k, uv[k]) for k in range(self.m)] + [self.end]
        return np.concatenate([_constraint(xs[k], xs[k + 1], xs[k + 2], self.normals[k], etas[k]) for k in range(self.m)])

    def barycentrics(self, k, x):
        p0, p1, p2 = self.tris[k]
        return np.linalg.lstsq(np.stack([p0 - p2, p1 - p2], axis=1), np.asarray(x, float) - p2, rcond=None)[0]

    def solve(self, etas, uv0):
        uv = np.array(uv0, float).reshape(-1)
        for _ in range(60):
            r = self.residual(uv, etas)
            if np.abs(r).max() < 1e-15:
                break
            J = np.empty((uv.size, uv.size))
            for j in range(uv.size):
                d = np.zeros_like(uv); d[j] = 1e-7
                J[:, j] = (self.residual(uv + d, etas) - self.residual(uv - d, etas)) / 2e-7
            step, t = np.linalg.solve(J, r), 1.0
            while t > 1e-4 and not np.abs(self.residual(uv - t * step, etas)).max() < np.abs(r).max():      # (damped: a NaN counts as worse)
                t *= 0.5
            uv = uv - t * step
        assert np.abs(self.residual(uv, etas)).max() < 1e-13
        return uv


def _path_info(chain, uv, etas, end_tri):
    """The path as calc_grad's records: m specular vertices, then the diffuse end point (N = 1, float64)."""
    f = lambda a: torch.tensor(np.asarray(a, float), dtype=torch.float64).reshape(1, -1)
    s = lambda a: torch.tensor([float(a)], dtype=torch.float64)
    info = [{"cam": f(chain.cam)}]
    uv = uv.reshape(chain.m, 2)
    verts = [(chain.tris[k], uv[k], chain.normals[k], etas[k], FLAGS_DIELECTRIC) for k in range(chain.m)]
    b = np.linalg.lstsq(np.stack([end_tri[0] - end_tri[2], end_tri[1] - end_tri[2]], axis=1), chain.end - end_tri[2], rcond=None)[0]
    verts.append((end_tri, b, np.array([0.0, 0.0, 1.0]), 1.0, FLAGS_DIFFUSE))
    for k, (tri, bc, n, eta, flags) in enumerate(verts):
        p = tri[0] * bc[0] + tri[1] * bc[1] + tri[2] * (1 - bc[0] - bc[1])
        info.append({"it": k, "active": torch.tensor([True]), "bsdf": torch.tensor([flags], dtype=torch.int32), "ismesh": s(1.0),
                     "light": f([0.0, 9.0, 9.0]), "active_em": torch.tensor([False]),
                     "points": [f(tri[0]), f(tri[1]), f(tri[2]), f(p)], "uv": [s(bc[0]), s(bc[1])], "normal": f(_unit(n)),
                     "normals": [f(_unit(n))] * 3, "eta": s(eta), "hf": f([0.0, 0.0, 0.0])})
    return info


def _slab(tilt):
    """Two parallel faces one unit apart, big flat triangles on each; `tilt`: the slab's rotation (normals along no axis)."""
    c, s_ = np.cos(0.4), np.sin(0.4)
    R = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]]) if tilt else np.eye(3)
    face = lambda z: [R @ np.array([-4.0, -4.0, z]), R @ np.array([4.0, -4.0, z]), R @ np.array([0.0, 4.0, z])]
    return R, face


def _check(chain, etas, chain_factor, end_tri, dlduv_row, start, int_ior=None, ext_ior=1.0):
    """`start`: where the straight (unfolded) line from the camera to the end point meets the faces -- Newton's first guess"""
    m = chain.m
    uv = chain.solve(etas, [chain.barycentrics(k, start[k]) for k in range(m)])
    assert (uv > 0.02).all() and (uv.reshape(m, 2).sum(1) < 0.98).all()       # inside their triangles
    want = np.zeros(m)
    for k in range(m):
        if etas[k] == 1.0:
            continue
        ep, em = list(etas), list(etas)
        ep[k] += H; em[k] -= H
        want[k] = dlduv_row @ (chain.solve(ep, uv) - chain.solve(em, uv)) / (2 * H)
    K = m + 1
    info = _path_info(chain, uv, etas, end_tri)
    dlduv = torch.zeros((1, 1, 2 * (K + 1)), dtype=torch.float64)
    dlduv[0, 0, :2 * m] = torch.tensor(dlduv_row)
    dldp = torch.zeros((1, 3), dtype=torch.float64)
    fp, _, _, geta = host_ior_calc_grad("manifold", info, dlduv, dldp, dtype=torch.float64, dlduv_cols=2 * m)
    got = geta[:m, 0].numpy()
    assert np.abs(want).max() < 0.05 and np.abs(want[np.asarray(etas) != 1.0]).min() > 1e-6       # away from the clamp, and not trivially 0
    for k in range(m):
        if etas[k] != 1.0:
            assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got[k], want[k])
    # the chain factor d eta_k / d int_ior per vertex (0 on a reflection), through the row rule of the backward kernel
    dhf = torch.zeros((K, 1, 3), dtype=torch.float64)
    dhf[:m, 0, 0] = torch.tensor(chain_factor)
    eta_t = torch.tensor(list(etas) + [1.0], dtype=torch.float64).reshape(K, 1)
    gm = torch.stack([fp[5 * k + 4] for k in range(m)] + [torch.zeros((1, 3), dtype=torch.float64)])
    rows = ior_row_values(eta_t, geta, gm, dhf)[:, 0].numpy()
    for k in range(m):
        if etas[k] == 1.0:
            assert rows[k] == 0.0                                  # a reflection: exactly nothing
    g_ior = float(want @ np.asarray(chain_factor))
    assert abs(rows.sum() - g_ior) <= 1e-6 * abs(g_ior), (rows, g_ior)
    if int_ior is not None:
        # ... and the same number straight from a finite difference in int_ior
        def uv_at(i):
            return chain.solve([1.0 if e == 1.0 else (i / ext_ior if e > 1.0 else ext_ior / i) for e in etas], uv)
        fd = dlduv_row @ (uv_at(int_ior + H) - uv_at(int_ior - H)) / (2 * H)
        assert abs(rows.sum() - fd) <= 1e-6 * abs(fd), (rows.sum(), fd)


@pytest.mark.parametrize("n", [1.5, 1.33])
@pytest.mark.parametrize("tilt", [False, True], ids=["axis", "tilted"])
def test_geta_of_a_slab_is_the_derivative_of_snells_law(n, tilt):
    R, face = _slab(tilt)
    nz = R @ np.array([0.0, 0.0, 1.0])
    chain = Chain(R @ np.array([-0.5, 0.2, 3.0]), [face(1.0), face(0.0)], [nz, nz], R @ np.array([0.8, -0.1, -1.5]))
    end_tri = [R @ np.array([-4.0, -4.0, -1.5]), R @ np.array([4.0, -4.0, -1.5]), R @ np.array([0.0, 4.0, -1.5])]
    ext = 1.0
    cam, end = np.array([-0.5, 0.2, 3.0]), np.array([0.8, -0.1, -1.5])
    start = [R @ (cam + (end - cam) * (cam[2] - z) / (cam[2] - end[2])) for z in (1.0, 0.0)]
    _check(chain, [n / ext, ext / n], [1.0 / ext, -ext / n ** 2], end_tri, np.array([3e-3, -2e-3, 1.5e-3, 2.5e-3]), start, int_ior=n)


@pytest.mark.parametrize("n", [1.5, 1.33])
def test_a_reflection_vertex_in_the_chain_contributes_nothing(n):
    """camera -> into the slab (eta = n) -> mirror reflection off the lower face from inside (eta = 1) -> out of the upper face
    (eta = 1 / n) -> a diffuse end point above the slab."""
    R, face = _slab(True)
    nz = R @ np.array([0.0, 0.0, 1.0])
    chain = Chain(R @ np.array([-0.9, 0.2, 3.0]), [face(1.0), face(0.0), face(1.0)], [nz, nz, nz], R @ np.array([1.1, -0.3, 2.5]))
    end_tri = [R @ np.array([-4.0, -4.0, 2.5]), R @ np.array([4.0, -4.0, 2.5]), R @ np.array([0.0, 4.0, 2.5])]
    cam, end = np.array([-0.9, 0.2, 3.0]), np.array([1.1, -0.3, -2.5])             # (the end point mirrored in the lower face)
    on_line = [cam + (end - cam) * (cam[2] - z) / (cam[2] - end[2]) for z in (1.0, 0.0, -1.0)]
    start = [R @ (x * np.array([1.0, 1.0, -1.0 if j == 2 else 1.0])) for j, x in enumerate(on_line)]
    _check(chain, [n, 1.0, 1.0 / n], [1.0, 0.0, -1.0 / n ** 2], end_tri, np.array([2e-3, -1e-3, 1e-3, 2e-3, -1.5e-3, 1e-3]), start, int_ior=n)
