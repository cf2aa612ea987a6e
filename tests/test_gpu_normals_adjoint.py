"""The derivative of the recomputed vertex normals on the GPU (csrc/epsm_trace_scene.hip: epsm_vertex_normals_backward /
_forward) against the float64 twin of scene_tables.py, and the chain through ``render_backward`` / ``render_forward`` of the
manifold integrators and ``prb_reparam`` on the device."""

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _normals_meshes import bump_grid, corner_angles, cut_mesh, fan, icosphere, mirror_scene
from _util import assert_two_routes_agree
from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd import scene_tables as st

pytestmark = pytest.mark.gpu


def _two_meshes():
    """Only the second mesh is flagged: its vertex range does not start at 0."""
    (v0, f0), (v1, f1) = bump_grid(9), icosphere(2)
    return [(v0, f0, False), (v1, f1, True)]


CASES = {"icosphere": lambda: [icosphere(3) + (True,)], "grid": lambda: [bump_grid(33) + (True,)], "fan": lambda: [fan(100) + (True,)],
         "two_meshes": _two_meshes}


class Table:
    """Meshes [(v, f, flagged)] back to back on the device with their topology, and the twin's inputs (float64 of the SAME
    float32 positions)."""

    def __init__(self, meshes, seed=0):
        gen = torch.Generator().manual_seed(seed)
        self.meshes = meshes
        self.table = (S.EpsmMesh * len(meshes))()
        self.vb, pos, tri, t0 = [0], [], [], 0
        for c, (v, f, flagged) in zip(self.table, meshes):
            c.tri_begin, c.tri_count, c.flags = t0, len(f), 1 if flagged else 0
            tri.append(f + self.vb[-1]); pos.append(v)
            t0 += len(f); self.vb.append(self.vb[-1] + len(v))
        self.pos = torch.tensor(np.concatenate(pos), dtype=torch.float32)
        self.tri = torch.tensor(np.concatenate(tri), dtype=torch.int32)
        self.V = self.pos.shape[0]
        self.g = torch.randn((self.V, 3), generator=gen)
        self.t = torch.randn((self.V, 3), generator=gen)
        self.d_pos, self.d_tri = self.pos.cuda(), self.tri.cuda()
        self.top = st.SceneTopology(self.d_tri, self.V)

    def twin(self, rows, forward):
        out = torch.zeros((self.V, 3), dtype=torch.float64)
        for (v, f, flagged), lo, hi in zip(self.meshes, self.vb, self.vb[1:]):
            if flagged:
                fn = st.vertex_normals_jvp_torch if forward else st.vertex_normals_vjp_torch
                out[lo:hi] = fn(self.pos[lo:hi].double(), torch.tensor(f), rows[lo:hi].double())
        return out

    def device(self, rows, forward, out=None):
        out = torch.zeros((self.V, 3), device="cuda") if out is None else out
        fn = st.vertex_normals_forward if forward else st.vertex_normals_backward
        fn(self.d_pos, self.d_tri, self.table, self.vb, rows.cuda(), out, topology=self.top)
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module", params=sorted(CASES))
def table(request):
    tb = Table(CASES[request.param](), seed=len(request.param))
    tb.name = request.param
    tb.want = {False: tb.twin(tb.g, False), True: tb.twin(tb.t, True)}       # computed once, shared, left unchanged
    return tb


def test_the_meshes_are_what_the_tests_say(table):
    """V = 642 is no multiple of the block; the fan's hub has valence 100; every angle lies between 20 and 140 degrees."""
    sizes = {"icosphere": 642, "grid": 33 * 33, "fan": 101, "two_meshes": 81 + 162}
    assert table.V == sizes[table.name] and table.V % 256 != 0
    for v, f, _ in table.meshes:
        a = corner_angles(v, f)
        assert 20.0 < a.min() and a.max() < 140.0, (table.name, a.min(), a.max())
    if table.name == "fan":
        assert np.bincount(table.meshes[0][1].ravel())[0] == 100


@pytest.mark.parametrize("forward", [False, True], ids=["backward", "forward"])
def test_device_equals_the_float64_twin(table, forward):
    """Both sides compute in float64 from the same float32 inputs and round once: per element 2^-23 |twin| + 2^-40 max |twin|."""
    want = table.want[forward]
    got = table.device(table.t if forward else table.g, forward).cpu().double()
    bound = 2.0 ** -23 * want.abs() + 2.0 ** -40 * float(want.abs().max())
    excess = (got - want).abs() - bound
    print(f"{table.name} {'forward' if forward else 'backward'}: max |device - twin| / max |twin| = "
          f"{float((got - want).abs().max() / want.abs().max()):.3e}, largest (error - bound) = {float(excess.max()):.3e}")
    assert float(want.abs().max()) > 0.1
    assert bool((excess <= 0).all()), float(excess.max())


def test_rows_of_unflagged_meshes_come_back_bit_for_bit():
    tb = Table(_two_meshes(), seed=2)
    lo = tb.vb[1]
    pattern = (torch.arange(tb.V * 3, dtype=torch.float32).reshape(-1, 3) * 0.37 - 11.0)
    for forward in (False, True):
        out = tb.device(tb.t if forward else tb.g, forward, out=pattern.cuda()).cpu()
        assert torch.equal(out[:lo], pattern[:lo])
        assert not torch.equal(out[lo:], pattern[lo:])


@pytest.mark.parametrize("forward", [False, True], ids=["backward", "forward"])
def test_two_calls_give_identical_bits_and_the_output_is_added_to(table, forward):
    rows = table.t if forward else table.g
    once = table.device(rows, forward)
    assert torch.equal(table.device(rows, forward), once)
    start = torch.randn((table.V, 3), generator=torch.Generator().manual_seed(9))
    got = table.device(rows, forward, out=start.cuda()).cpu()
    assert torch.equal(got, start + once.cpu())                 # ONE float32 add of the rounded sum


def test_device_forward_is_the_transpose_of_device_backward(table):
    """|sum g . (J t) - sum (J^T g) . t| <= 2^-22 sum |g| |J t|."""
    Jt = table.device(table.t, True).cpu().double()
    JTg = table.device(table.g, False).cpu().double()
    a, b = table.g.double() * Jt, JTg * table.t.double()
    assert abs(float(a.sum() - b.sum())) <= 2.0 ** -22 * float(a.abs().sum()), (float(a.sum()), float(b.sum()))


def test_cut_rules_on_the_device():
    v, f, isolated, only_degenerate = cut_mesh()
    tb = Table([(v, f, True)], seed=4)
    for forward in (False, True):
        rows = tb.t if forward else tb.g
        got, want = tb.device(rows, forward).cpu().double(), tb.twin(rows, forward)
        assert bool(torch.isfinite(got).all())
        for w in (isolated, only_degenerate, only_degenerate + 1):
            assert float(got[w].abs().max()) == 0.0
        assert float(got[:16].abs().max()) > 0
        assert bool(((got - want).abs() <= 2.0 ** -23 * want.abs() + 2.0 ** -40 * float(want.abs().max())).all())


def test_tensors_of_another_device_are_refused(table):
    z = torch.zeros((table.V, 3))
    with pytest.raises(ValueError, match="lives on cpu"):
        st.vertex_normals_backward(table.d_pos, table.d_tri, table.table, table.vb, z, z.cuda(), topology=table.top)
    with pytest.raises(ValueError, match="lives on cpu"):
        st.vertex_normals_forward(table.d_pos, table.d_tri, table.table, table.vb, z.cuda(), z, topology=table.top)
    with pytest.raises(ValueError, match="SceneTopology"):
        st.vertex_normals_backward(table.d_pos, table.d_tri, table.table, table.vb, z.cuda(), z.cuda())


# -- through the integrators --------------------------------------------------------------------------------------------------
RES = 16
FORMS = [("manifold", "wavefront", {"type": "dielectric"}), ("manifold", "mega", {"type": "conductor"}), ("prb_reparam", "mega", None)]


def _pass(kind, tracer, bsdf, flagged, scene_tables="host", clip=None, seed=3):
    # (the manifold integrators map path -> pixel without a sample border)
    sc = mirror_scene(RES, 8, "cuda", scene_tables=scene_tables, border=kind != "manifold", **({} if bsdf is None else {"bsdf": bsdf}))
    sc.tracer = tracer
    sc.attach("sphere", positions=True, normals=True, recomputed_normals=flagged)
    sc.attach("plane", positions=True)
    gen = torch.Generator().manual_seed(1)
    if kind == "manifold":
        props = {"type": kind, "max_depth": 4, "backward_sensor": 0, "backward_spp": 8}
        if clip is not None:
            props["outlier_clip"] = clip
        g = (1e-3 * torch.randn((RES, RES, 5), generator=gen)).cuda()
    else:
        props = {"type": kind, "max_depth": 3, "reparam_rays": 8}
        g = torch.randn((RES, RES, 3), generator=gen).cuda()
    integ = epsm.load_dict(props)
    p = sc.param_grads()
    integ.render_backward(sc, p, g, sensor=0, seed=seed, spp=8)
    torch.cuda.synchronize()
    return sc, integ, p


def _chain(sc, nrm):
    out = torch.zeros_like(nrm)
    sc.normals_backward(nrm.contiguous(), out)
    return out


@pytest.mark.parametrize("kind,tracer,bsdf", FORMS, ids=[f"{k}-{t}" for k, t, _ in FORMS])
def test_chain_through_render_backward(kind, tracer, bsdf):
    """``pos_on - chain(nrm_on)`` against ``pos_off`` and ``nrm_on`` against ``nrm_off``: two calls of a pass whose float atomics
    differ in the last bits, at the tolerance of tests/_util.py's two-routes helper (its band: the outlier threshold moved by
    -+2 % where the integrator has one)."""
    from epsm_mitsuba3_amd.integrators import OUTLIER_CLIP
    sc, _, on = _pass(kind, tracer, bsdf, True)
    _, _, off = _pass(kind, tracer, bsdf, False)
    if kind == "manifold":
        lo, hi = (_pass(kind, tracer, bsdf, False, clip=OUTLIER_CLIP * s)[2] for s in (0.98, 1.02))
    else:
        lo = hi = off
    a, b = sc.mesh_slices["sphere"]
    assert float(on.nrm[a:b].abs().max()) > 0
    chain = _chain(sc, on.nrm)
    assert float(chain[a:b].abs().max()) > 1e-3 * float(on.pos[a:b].abs().max()) and float(chain[:a].abs().max()) == 0.0
    assert_two_routes_agree(on.nrm, off.nrm, lo.nrm, hi.nrm, name=f"{kind} nrm")
    assert_two_routes_agree(on.pos - chain, off.pos, lo.pos, hi.pos, name=f"{kind} pos")


def test_render_forward_is_the_transpose_on_the_device():
    """The bound tests/test_gpu_render_forward.py uses: 2e-3 of the sum of the absolute terms."""
    from test_render_forward import transpose_gap
    sc = mirror_scene(RES, 8, "cuda")
    sc.attach("sphere", recomputed_normals=True)
    sc.attach("plane", positions=True)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    gap, S_, big = transpose_gap(integ, sc, 7, 8, torch.Generator().manual_seed(5))
    assert big > 0 and S_ > 0
    assert gap <= 2e-3 * S_, (gap, S_)


def test_device_and_host_tables_give_the_same_chained_rows():
    """``scene_tables="device"`` reads the topology the scene built for its normals, the host tables build one on first use: the
    same kernels over the same triangles -- the chain of the same rows is the same bits."""
    sc_h, _, p = _pass("prb_reparam", "mega", None, True)
    sc_d = mirror_scene(RES, 8, "cuda", scene_tables="device")
    sc_d.attach("sphere", recomputed_normals=True)
    assert sc_h.scene_tables == "host" and sc_d.scene_tables == "device" and torch.equal(sc_h.tri, sc_d.tri)
    assert torch.equal(sc_h.positions, sc_d.positions)
    assert torch.equal(_chain(sc_h, p.nrm), _chain(sc_d, p.nrm))
    a, b = sc_h.mesh_slices["sphere"]
    assert float(_chain(sc_h, p.nrm)[a:b].abs().max()) > 0
