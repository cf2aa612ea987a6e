"""Large-steps vertex updates without a GPU: the entry points of include/epsm_trace.h are exported and refuse bad arguments before
anything touches a device; the torch forms of epsm_mitsuba3_amd.smooth (what ``host=True`` runs) against the dense float64
Laplacian of tests/_smooth_meshes.py; ``from_differential``'s derivative; AdamUniform's step; Scene.mesh_laplacian's indices.
The HIP kernels (csrc/epsm_trace_smooth.hip) are checked in tests/test_gpu_smooth.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _smooth_meshes as M
from _scenes import floor_and_light, on_host
from epsm_mitsuba3_amd import _lib, smooth

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _host_lap(name, lam):
    tri, V = M.MESHES[name]
    return smooth.MeshLaplacian(torch.from_numpy(tri), V, lam, host=True)


# -- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported(lib):
    for s in ("epsm_mesh_laplacian_bytes", "epsm_mesh_laplacian", "epsm_laplacian_apply", "epsm_laplacian_solve_bytes",
              "epsm_laplacian_solve"):
        assert hasattr(lib, s), s
    assert lib.epsm_abi_version() == 7                       # additions only


def test_the_bytes_queries_grow_with_V_and_T(lib):
    assert 0 < lib.epsm_mesh_laplacian_bytes(100, 200) < lib.epsm_mesh_laplacian_bytes(100000, 200) < lib.epsm_mesh_laplacian_bytes(100000, 200000)
    assert 0 < lib.epsm_laplacian_solve_bytes(100) < lib.epsm_laplacian_solve_bytes(100000) < lib.epsm_laplacian_solve_bytes(10 ** 7)
    assert lib.epsm_mesh_laplacian_bytes(642, 1280) >= 256 + 4 * 643 + 4 * 642 + 24 * 1280       # head, offsets, degrees, two slots per corner
    assert lib.epsm_laplacian_solve_bytes(642) >= 4 * 12 * 642                                   # r, two p, q


class _Args:
    """Host memory standing in for the device arrays: a refused call never reads it."""

    def __init__(self, lib, V=64, T=100):
        self.V, self.T = V, T
        self.bufs = {k: (C.c_char * (n + 32))() for k, n in dict(
            tri=12 * T, topology=8 * V + 12 * T + 1024, table=lib.epsm_mesh_laplacian_bytes(V, T), b=12 * V, x=12 * V, info=48,
            ws=lib.epsm_laplacian_solve_bytes(V)).items()}
        self.table_bytes, self.ws_bytes = lib.epsm_mesh_laplacian_bytes(V, T), lib.epsm_laplacian_solve_bytes(V)

    def p(self, k, off=0):
        a = C.addressof(self.bufs[k])
        return (a + 15) // 16 * 16 + off


def _refused(lib, rc, word=None):
    assert rc == EINVAL
    msg = lib.epsm_last_error()
    assert msg and (word is None or word.encode() in msg), msg


def test_mesh_laplacian_refuses_bad_arguments_without_a_device(lib):
    a = _Args(lib)
    ok = lambda **kw: dict(dict(tri=a.p("tri"), V=a.V, T=a.T, top=a.p("topology"), table=a.p("table"), n=a.table_bytes), **kw)
    call = lambda d: lib.epsm_mesh_laplacian(d["tri"], d["V"], d["T"], d["top"], d["table"], d["n"], None)
    _refused(lib, call(ok(tri=None)), "NULL")
    _refused(lib, call(ok(top=None)), "NULL")
    _refused(lib, call(ok(table=None)), "NULL")
    _refused(lib, call(ok(V=-1)), "V must")
    _refused(lib, call(ok(T=-5)), "T must")
    _refused(lib, call(ok(n=a.table_bytes - 1)), "smaller")
    _refused(lib, call(ok(table=a.p("table", 8))), "aligned")


def test_apply_refuses_bad_arguments_without_a_device(lib):
    a = _Args(lib)
    call = lambda table, V, lam, x, y: lib.epsm_laplacian_apply(table, V, lam, x, y, None)
    _refused(lib, call(None, a.V, 1.0, a.p("b"), a.p("x")), "NULL")
    _refused(lib, call(a.p("table"), a.V, 1.0, None, a.p("x")), "NULL")
    _refused(lib, call(a.p("table"), a.V, 1.0, a.p("b"), None), "NULL")
    _refused(lib, call(a.p("table"), -3, 1.0, a.p("b"), a.p("x")), "V outside")
    for lam in (-1.0, math.nan, math.inf, -math.inf):
        _refused(lib, call(a.p("table"), a.V, lam, a.p("b"), a.p("x")), "lambda")
    _refused(lib, call(a.p("table", 4), a.V, 1.0, a.p("b"), a.p("x")), "aligned")


def test_solve_refuses_bad_arguments_without_a_device(lib):
    a = _Args(lib)
    base = dict(table=a.p("table"), V=a.V, lam=10.0, b=a.p("b"), x=a.p("x"), iters=50, tol=1e-6, form=0, info=a.p("info"), ws=a.p("ws"),
                n=a.ws_bytes)
    call = lambda **kw: (lambda d: lib.epsm_laplacian_solve(d["table"], d["V"], d["lam"], d["b"], d["x"], d["iters"], d["tol"], d["form"],
                                                            d["info"], d["ws"], d["n"], None))(dict(base, **kw))
    for k in ("table", "b", "x", "info"):
        _refused(lib, call(**{k: None}), "NULL")
    _refused(lib, call(ws=None), "workspace")
    _refused(lib, call(V=-1), "V outside")
    for lam in (-0.5, math.nan, math.inf):
        _refused(lib, call(lam=lam), "lambda")
    for iters in (0, -4):
        _refused(lib, call(iters=iters), "max_iters")
    for tol in (0.0, 1.0, -1e-3, 2.0, math.nan):
        _refused(lib, call(tol=tol), "rel_tol")
    _refused(lib, call(form=3), "form")
    _refused(lib, call(n=a.ws_bytes - 1), "workspace")
    _refused(lib, call(ws=a.p("ws", 8)), "workspace")
    _refused(lib, call(x=a.p("b")), "overlap")
    _refused(lib, call(V=smooth.ONE_GROUP_MAX_V + 1, form=smooth.FORMS["one_group"]), "ONE_GROUP")


def test_a_cpu_tensor_is_refused_without_host():
    tri, V = M.octahedron()
    with pytest.raises(_lib.EpsmError, match="no CPU fallback"):
        smooth.MeshLaplacian(torch.from_numpy(tri), V, 1.0)


# -- the torch forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.MESHES))
def test_the_torch_laplacian_is_the_definition(name):
    tri, V = M.MESHES[name]
    want = M.dense_laplacian(tri, V)
    assert np.array_equal(smooth.laplacian_dense(torch.from_numpy(tri), V).numpy(), want)
    lap = _host_lap(name, 3.0)
    assert lap.max_degree == M.max_degree(tri, V)
    assert lap.neighbours() == M.neighbour_sets(tri, V)
    x = torch.from_numpy(M.rows(V, 1)).double()
    assert np.allclose(lap.apply(x).numpy(), M.dense_matrix(tri, V, 3.0) @ x.numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name", ("octahedron", "grid_31x33", "unnamed_vertex"))
def test_the_torch_solve_meets_the_dense_solve(name):
    tri, V = M.MESHES[name]
    lap = _host_lap(name, 10.0)
    b = torch.from_numpy(M.rows(V, 2)).double()
    b[:, 1] = 0.0                                             # a zero column: zeros, and the others still converge
    x = lap.solve(b, rel_tol=1e-12, max_iters=4 * V)
    want = M.dense_solve(tri, V, 10.0, b.numpy())
    assert np.abs(x.numpy() - want).max() <= 1e-9 * np.abs(want).max()
    assert not x[:, 1].any()
    info = lap.info()
    assert all(c for _, c, _ in info) and info[1] == (0, True, 0.0)


def test_from_differential_passes_gradcheck_on_the_octahedron():
    lap = _host_lap("octahedron", 2.5)
    u = torch.from_numpy(M.rows(6, 3)).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: lap.from_differential(t, rel_tol=1e-14, max_iters=100), (u,), eps=1e-6, atol=1e-8)


def test_to_differential_undoes_from_differential():
    lap = _host_lap("grid_25x41", 19.0)
    u = torch.from_numpy(M.rows(1025, 4)).double()
    back = lap.to_differential(lap.from_differential(u, rel_tol=1e-13, max_iters=5000))
    assert float((back - u).abs().max()) <= 1e-10 * float(u.abs().max())
    assert lap.to_differential is not None and torch.equal(lap.to_differential(u), lap.apply(u))


def test_default_max_iters_is_the_textbook_bound():
    lap = _host_lap("grid_32x32", 50.0)
    kappa = 1 + 2 * 50.0 * lap.max_degree
    assert lap.default_max_iters(1e-6) == math.ceil(0.5 * math.sqrt(kappa) * math.log(2 / 1e-6))


# -- the optimiser --------------------------------------------------------------------------------------------------------------
def test_adam_uniform_takes_the_closed_form_step():
    # first step: m_hat = g, v_hat = g^2, one maximum for the tensor: 16 -> every element moves by lr g / 4
    p = torch.nn.Parameter(torch.tensor([1.0, 2.0], dtype=torch.float64))
    opt = smooth.AdamUniform([p], lr=0.5, betas=(0.9, 0.999))
    p.grad = torch.tensor([3.0, -4.0], dtype=torch.float64)
    opt.step()
    assert torch.allclose(p.detach(), torch.tensor([1.0 - 0.5 * 3 / 4, 2.0 + 0.5 * 4 / 4], dtype=torch.float64), rtol=1e-12, atol=0)
    # second step with g = (0, 2): m = .9 (.1 g1) + .1 g2, v = .999 (.001 g1^2) + .001 g2^2, bias-corrected, max over the tensor
    p.grad = torch.tensor([0.0, 2.0], dtype=torch.float64)
    before = p.detach().clone()
    opt.step()
    m = np.array([0.9 * 0.3, 0.9 * -0.4 + 0.1 * 2.0]) / (1 - 0.9 ** 2)
    v = np.array([0.999 * 0.009, 0.999 * 0.016 + 0.001 * 4.0]) / (1 - 0.999 ** 2)
    want = before.numpy() - 0.5 * m / math.sqrt(v.max())
    assert np.allclose(p.detach().numpy(), want, rtol=1e-12, atol=0)


def test_adam_uniform_leaves_a_tensor_without_gradient_signal_alone():
    p = torch.nn.Parameter(torch.ones(3))
    opt = smooth.AdamUniform([p], lr=0.1)
    p.grad = torch.zeros(3)
    opt.step()
    assert torch.equal(p.detach(), torch.ones(3))


# -- the scene ------------------------------------------------------------------------------------------------------------------
def test_scene_mesh_laplacian_uses_the_meshs_local_indices():
    sc = on_host(floor_and_light())
    lo, hi = sc.mesh_slices["light"]
    assert lo > 0                                              # not the first mesh: its triangles are stored with an offset
    lap = sc.mesh_laplacian("light", 7.0)
    t0, t1 = sc.mesh_tri_slices["light"]
    local = sc.tri[t0:t1].numpy() - lo
    assert lap.V == hi - lo and lap.lam == 7.0
    assert lap.neighbours() == M.neighbour_sets(local, hi - lo) and lap.max_degree == 3
    x = torch.from_numpy(M.rows(hi - lo, 5)).double()
    assert np.allclose(lap.apply(x).numpy(), M.dense_matrix(local, hi - lo, 7.0) @ x.numpy(), rtol=1e-13, atol=1e-13)
    with pytest.raises(ValueError, match="no mesh named"):
        sc.mesh_laplacian("nothing", 1.0)
