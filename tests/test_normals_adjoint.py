"""The derivative of the recomputed vertex normals with respect to the positions (scene_tables.vertex_normals_backward /
_forward, Scene.attach(recomputed_normals=True)) without a device: the float64 twin against finite differences of the numpy
rule, against autograd of the torch rule, as a transpose pair, under rigid motions and at the primal's cuts; the chain through
``prb_reparam`` on the host build of the tracer, with one and with two ranks.  The HIP kernels: tests/test_gpu_normals_adjoint.py
(where the manifold integrators run too: their backward pass has no host build)."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _normals_meshes import bump_grid, bump_motion, bump_scene, cut_mesh, icosphere, mirror_scene, one_thread
from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd import scene_tables as st

MESHES = {"icosphere": lambda: icosphere(2), "grid": lambda: bump_grid(9)}


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)


@pytest.fixture(scope="module", params=sorted(MESHES))
def mesh(request):
    v, f = MESHES[request.param]()
    gen = torch.Generator().manual_seed(len(v))
    return dict(name=request.param, v=v, f=f, vt=_t(v), ft=_t(f, torch.int64), g=torch.randn(v.shape, generator=gen, dtype=torch.float64),
                t=torch.randn(v.shape, generator=gen, dtype=torch.float64))


def test_the_meshes_are_what_the_tests_say(mesh):
    assert mesh["v"].shape[0] == {"icosphere": 162, "grid": 81}[mesh["name"]]
    if mesh["name"] == "grid":
        valence = np.bincount(mesh["f"].ravel(), minlength=81)
        assert {1, 2, 3} <= set(valence.tolist())


def test_twin_against_finite_differences(mesh):
    """Central differences of the numpy rule with step h = 1e-6 along a direction t of unit largest entry.  n is homogeneous of
    degree 0 in the edge vectors, so its k-th derivative along t is at most C_k / L^k with L the shortest edge; the truncation
    error h^2 / 6 |n'''| is then below h^2 / 6 * C_3 / L^3, and with C_3 = 100 (generous: measured below) that is 1.7e-11 / L^3.  The
    rounding of the difference quotient adds 2^-52 / h = 2.2e-10 per entry.
    Measured |twin - FD|, largest entry: icosphere (L = 0.276) 1.9e-10, grid (L = 0.125, derivatives up to 7.3) 5.0e-10, against
    bounds of 1.0e-9 and 8.8e-9: the rounding term and a fraction of the truncation term; no excess over the bound on either."""
    v, f, h = mesh["v"], mesh["f"], 1e-6
    t = (mesh["t"] / mesh["t"].abs().max()).numpy()
    fd = (S.vertex_normals(v + h * t, f) - S.vertex_normals(v - h * t, f)) / (2 * h)
    jvp = st.vertex_normals_jvp_torch(mesh["vt"], mesh["ft"], _t(t)).numpy()
    p = v[f]
    L = min(float(np.linalg.norm(p[:, i] - p[:, (i + 1) % 3], axis=1).min()) for i in range(3))
    err = float(np.abs(fd - jvp).max())
    print(f"{mesh['name']}: L = {L:.3f}, |twin - FD| = {err:.2e}, largest derivative {np.abs(jvp).max():.2f}")
    assert np.abs(jvp).max() > 0.1
    assert err <= h * h / 6 * 100 / L ** 3 + 2.0 ** -52 / h, (err, L)
    # and the vjp, one coordinate at a time on a few vertices: row w of J^T g by differences of g . n
    g = mesh["g"].numpy()
    vjp = st.vertex_normals_vjp_torch(mesh["vt"], mesh["ft"], mesh["g"]).numpy()
    for w in (0, 7, v.shape[0] - 1):
        for k in range(3):
            e = np.zeros_like(v); e[w, k] = 1.0
            d = float(((S.vertex_normals(v + h * e, f) - S.vertex_normals(v - h * e, f)) * g).sum()) / (2 * h)
            assert abs(d - vjp[w, k]) <= (h * h / 6 * 100 / L ** 3 + 2.0 ** -52 / h) * np.abs(g).sum(), (w, k, d, vjp[w, k])


def test_twin_against_autograd(mesh):
    v = mesh["vt"].clone().requires_grad_(True)
    n = S.vertex_normals_torch(v, mesh["ft"])
    (auto,) = torch.autograd.grad((n * mesh["g"]).sum(), v)
    vjp = st.vertex_normals_vjp_torch(mesh["vt"], mesh["ft"], mesh["g"])
    assert float((vjp - auto).abs().max()) <= 1e-12 * float(auto.abs().max())
    _, auto_jvp = torch.autograd.functional.jvp(lambda x: S.vertex_normals_torch(x, mesh["ft"]), mesh["vt"], mesh["t"])
    jvp = st.vertex_normals_jvp_torch(mesh["vt"], mesh["ft"], mesh["t"])
    assert float((jvp - auto_jvp).abs().max()) <= 1e-12 * float(auto_jvp.abs().max())


def test_twin_forward_is_the_transpose_of_twin_backward(mesh):
    jvp = st.vertex_normals_jvp_torch(mesh["vt"], mesh["ft"], mesh["t"])
    vjp = st.vertex_normals_vjp_torch(mesh["vt"], mesh["ft"], mesh["g"])
    a, b = (mesh["g"] * jvp), (vjp * mesh["t"])
    assert abs(float(a.sum() - b.sum())) <= 1e-12 * float(a.abs().sum() + b.abs().sum())


def test_translation_invariance_and_rotation_equivariance(mesh):
    """n(x + c) = n(x) and n(R x) = R n(x): sum_w (J^T g)_w = 0 and sum_w x_w x (J^T g)_w = sum_v n_v x g_v -- the second is why
    the chain and the rigid reduction's n x g_nrm term are the same torque."""
    x, g = mesh["vt"] + torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64), mesh["g"]
    vjp = st.vertex_normals_vjp_torch(x, mesh["ft"], g)
    n = _t(S.vertex_normals(x.numpy(), mesh["f"]))
    rhs = torch.linalg.cross(n, g, dim=1)
    scale = float(rhs.abs().sum())
    assert float(vjp.sum(0).abs().max()) <= 1e-10 * scale
    assert float((torch.linalg.cross(x, vjp, dim=1).sum(0) - rhs.sum(0)).abs().max()) <= 1e-10 * scale


def test_cut_rules():
    v, f, isolated, only_degenerate = cut_mesh()
    vt, ft = _t(v), _t(f, torch.int64)
    n = S.vertex_normals(v, f)
    assert np.array_equal(n[isolated], [0, 0, 1]) and np.array_equal(n[only_degenerate], [0, 0, 1]) and np.array_equal(n[only_degenerate + 1], [0, 0, 1])
    gen = torch.Generator().manual_seed(4)
    g, t = torch.randn(v.shape, generator=gen, dtype=torch.float64), torch.randn(v.shape, generator=gen, dtype=torch.float64)
    vjp, jvp = st.vertex_normals_vjp_torch(vt, ft, g), st.vertex_normals_jvp_torch(vt, ft, t)
    assert bool(torch.isfinite(vjp).all()) and bool(torch.isfinite(jvp).all())
    assert float(vjp[:16].abs().max()) > 0 and float(jvp[:16].abs().max()) > 0
    for w in (isolated, only_degenerate, only_degenerate + 1):          # constants: nothing flows in either direction
        assert float(vjp[w].abs().max()) == 0.0 and float(jvp[w].abs().max()) == 0.0
    a, b = g * jvp, vjp * t
    assert abs(float(a.sum() - b.sum())) <= 1e-12 * float(a.abs().sum() + b.abs().sum())


def test_refusals():
    z = torch.zeros((4, 3))
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    table = (S.EpsmMesh * 1)()
    table[0].tri_count, table[0].flags = 1, 1
    with pytest.raises(epsm._lib.EpsmError, match="GPU only"):
        st.vertex_normals_backward(z, tri, table, [0, 4], z.clone(), z.clone())
    with pytest.raises(epsm._lib.EpsmError, match="GPU only"):
        st.vertex_normals_forward(z, tri, table, [0, 4], z.clone(), z.clone())
    with pytest.raises(ValueError, match="float32"):
        st.vertex_normals_backward(z, tri, table, [0, 4], z.double(), z.clone(), host=True)
    with pytest.raises(ValueError, match="float32"):
        st.vertex_normals_forward(z, tri, table, [0, 4], z.clone(), torch.zeros((3, 3)), host=True)
    from _reparam_scenes import build
    sc = build("diffuse_sphere_area_light", 0.0, 8, 2)
    with pytest.raises(ValueError, match="came with the geometry"):
        sc.attach("sphere", recomputed_normals=True)
    with pytest.raises(ValueError, match="face normals"):
        sc.attach("wall", recomputed_normals=True)
    assert not sc.has_recomputed_normals() and not sc.mesh("sphere").pos_attached
    sc.set_vertex_positions("sphere", sc.vertex_positions("sphere") * 1.01)      # recomputed: now a function of the positions
    sc.attach("sphere", recomputed_normals=True)
    m = sc.mesh("sphere")
    assert m.pos_attached and m.nrm_attached and sc.has_recomputed_normals()
    sc.attach("sphere", positions=True, normals=True)                          # the default is off
    assert not sc.has_recomputed_normals()


# -- through the integrator, on the host build ------------------------------------------------------------------------------------
RES, SPP = 16, 8


def _backward(sc, flagged, seed=3, twice=False):
    sc.attach("sphere", positions=True, normals=True, recomputed_normals=flagged)
    sc.attach("plane", positions=True)                                         # a second mesh, never flagged
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    g = torch.ones((RES, RES, 3)) * (0.5 + torch.arange(RES, dtype=torch.float32) / RES)[None, :, None]
    p = sc.param_grads()
    integ.render_backward(sc, p, g, sensor=0, seed=seed, spp=SPP)
    if twice:
        integ.render_backward(sc, p, g, sensor=0, seed=seed + 1, spp=SPP)
    return p


def _twin_chain(sc, nrm):
    lo, hi = sc.mesh_slices["sphere"]
    m = sc.mesh("sphere")
    return st.vertex_normals_vjp_torch(sc.positions[lo:hi].double(), _t(m.f, torch.int64), nrm[lo:hi].double())


def test_chain_through_prb_reparam_on_the_host():
    """Flag on against flag off under one seed: the same ``nrm``, ``pos_on - pos_off`` = twin(nrm_off) at float32 rounding -- the
    twin's float64 result is rounded to float32 once and added to a float32 row, 2^-24 of each, SLACK for the float64 sums -- and
    the rows of the unflagged mesh bit for bit.  (One OpenMP thread: the host build then repeats a call bit for bit.)"""
    sc = mirror_scene(RES, SPP)
    with one_thread():
        off, on = _backward(sc, False), _backward(sc, True)
    lo, hi = sc.mesh_slices["sphere"]
    assert float(off.nrm[lo:hi].abs().max()) > 0 and float(off.pos[lo:hi].abs().max()) > 0
    assert torch.equal(on.nrm, off.nrm)
    plo, phi = sc.mesh_slices["plane"]
    assert torch.equal(on.pos[plo:phi], off.pos[plo:phi]) and float(off.pos[plo:phi].abs().max()) > 0
    want = _twin_chain(sc, off.nrm)
    assert float(want.abs().max()) > 0.1 * float(off.pos[lo:hi].abs().max())       # the chain is no small correction here
    got = on.pos[lo:hi].double() - off.pos[lo:hi].double()
    bound = 2.0 ** -24 * (1 + 1e-4) * (want.abs() + on.pos[lo:hi].double().abs())
    assert torch.all((got - want).abs() <= bound), float(((got - want).abs() - bound).max())


def test_forward_is_the_transpose_of_the_chained_backward_pass():
    """The dot-product test at the bound tests/test_render_forward.py uses on the host: 1e-4 of the sum of the absolute terms."""
    from test_render_forward import transpose_gap
    sc = mirror_scene(12, 4)
    sc.attach("sphere", recomputed_normals=True)
    sc.attach("plane", positions=True)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    gap, S_, big = transpose_gap(integ, sc, 7, 4, torch.Generator().manual_seed(5))
    assert big > 0 and S_ > 0
    assert gap <= 1e-4 * S_, (gap, S_)
    # the chain is part of both sides: without it on one side the identity fails by far more
    params, t = sc.param_grads(), sc.param_grads()
    lo, hi = sc.mesh_slices["sphere"]
    t.pos[lo:hi] = torch.randn((hi - lo, 3), generator=torch.Generator().manual_seed(6))
    g = torch.randn((12, 12, 3), generator=torch.Generator().manual_seed(7))
    fwd = integ.render_forward(sc, t, sensor=0, seed=7, spp=4)
    sc.attach("sphere", positions=True, normals=True)
    integ.render_backward(sc, params, g, sensor=0, seed=7, spp=4)
    a, b = float((g.double() * fwd.double()).sum()), float((params.flat.double() * t.flat.double()).sum())
    assert abs(a - b) > 1e-2 * (abs(a) + abs(b)), (a, b)


# -- end to end ---------------------------------------------------------------------------------------------------------------
def test_a_bulge_matches_finite_differences_only_with_the_chain():
    """A one-parameter non-rigid bulge of a glossy sheet (``set_vertex_positions`` recomputes the normals) by the recipe of
    tests/test_reparam.py's smooth configs -- tests/_reparam_scenes.py::fd_check: d sum(image * ramp) / d theta against central
    differences under common random numbers, 32 rays, 128 samples, 4 x the samples in the differences -- at the threshold of its
    configs without a discontinuity in view, 8 %.  The chained gradient meets it; ``pos . dp/dtheta`` alone does not.
    Measured (two seeds): chained -6857 / -6843, finite differences -6785 / -6806 (1.1 % / 0.6 % apart), unchained +1420 (121 %
    off, the other sign): on a mirror the normals carry most of the derivative."""
    res, spp, rays, mult, h, tol = 32, 128, 32, 4, 5e-3, 0.08
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 2, "reparam_rays": rays})
    g = torch.ones((res, res, 3)) * (0.5 + torch.arange(res, dtype=torch.float32) / res)[None, :, None]
    sc = bump_scene(res, spp)
    dp = bump_motion(sc)
    lo, hi = sc.mesh_slices["mirror"]
    got = {}
    for flagged in (True, False):
        sc.attach("mirror", positions=True, normals=True, recomputed_normals=flagged)
        p = sc.param_grads()
        integ.render_backward(sc, p, g, sensor=0, seed=0, spp=spp)
        got[flagged] = float((p.pos[lo:hi] * dp).sum())
    v = []
    for sgn in (1, -1):
        s2 = bump_scene(res, spp * mult)
        s2.set_vertex_positions("mirror", s2.vertex_positions("mirror") + sgn * h * bump_motion(s2))
        v.append(float((integ.render(s2, sensor=0, seed=100, spp=spp * mult) * g).sum()))
    fd = (v[0] - v[1]) / (2 * h)
    print(f"chained {got[True]:.1f}, unchained {got[False]:.1f}, finite differences {fd:.1f}")
    rel = lambda x: abs(x - fd) / max(abs(fd), 1e-3)
    assert rel(got[True]) < tol, (got, fd)
    assert not rel(got[False]) < tol, (got, fd)


# -- two ranks ----------------------------------------------------------------------------------------------------------------
def _chain_single(tile_paths):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sc = mirror_scene(12, 8)
    sc.tile_paths = tile_paths
    sc.attach_rigid("sphere")
    p = _backward(sc, True, twice=True)                  # a second call accumulates: its contribution alone is summed and chained
    lo, hi = sc.mesh_slices["sphere"]
    return torch.cat([p.pos[lo:hi].reshape(-1), p.nrm[lo:hi].reshape(-1), p.rigid.reshape(-1)])


def _chain_worker(rank, world, port, q):
    import torch.distributed as dist
    from epsm_mitsuba3_amd import dist as edist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    edist.init_from_env("gloo")
    out = _chain_single(512)
    q.put((rank, out.numpy().tobytes()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_match_a_single_process():
    """The pattern and the bound of tests/test_dist_gloo_rigid.py: both ranks chain the ALL-REDUCED rows and hold the same bits."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_chain_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[0] == got[1]
    single = _chain_single(512)
    both = torch.from_numpy(np.frombuffer(got[0], dtype=np.float32).copy())
    n = (single.numel() - 6) // 2
    for part in (slice(0, n), slice(n, 2 * n), slice(2 * n, 2 * n + 6)):
        m = float(single[part].abs().max())
        assert m > 0 and torch.allclose(both[part], single[part], rtol=1e-4, atol=1e-5 * m), float((both[part] - single[part]).abs().max())
