"""The scene tables built on the device (scene_tables.py: epsm_scene_topology, epsm_vertex_normals, epsm_emitter_tables,
epsm_environment_tables) against the host rules of scene.py: vertex normals against the fp64 ``vertex_normals``, CDFs and
areas against numpy fed the same float32 positions, envmap tables against ``environment_tables``; determinism, the in-place
``EpsmMesh.area``, and the rows the normals must leave alone."""
import numpy as np
import pytest
import torch

from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd import scene_tables as st

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _grid(n, rng, z=0.0):
    x, y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    v = np.stack([x.ravel(), y.ravel(), z + 0.05 * rng.normal(size=n * n)], axis=1)
    a = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).ravel()
    f = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)])
    return v, f


def _meshes():
    """(v, f, flagged): a small mesh with degenerate triangles (a repeated index, three collinear points, a zero-length edge)
    and two unreferenced vertices; an unflagged mesh; a flagged mesh of >= 10^6 triangles; a flagged sphere-like blob."""
    rng = np.random.default_rng(11)
    v0 = rng.normal(size=(40, 3))
    v0[30] = v0[31] = v0[32]                       # a zero-length edge
    v0[33] = 0.5 * (v0[34] + v0[35])               # collinear
    f0 = rng.integers(0, 30, size=(60, 3))
    f0 = np.concatenate([f0, [[0, 0, 5], [33, 34, 35], [30, 31, 36], [32, 37, 38]]])
    f0[f0 == 39] = 0                               # vertex 39 and 29 stay unreferenced
    f0[f0 == 29] = 1
    v1, f1 = _grid(30, rng, z=1.0)
    v2, f2 = _grid(710, rng, z=-1.0)               # 2 * 709^2 = 1 005 362 triangles
    v3 = rng.normal(size=(500, 3)); v3 /= np.linalg.norm(v3, axis=1, keepdims=True)
    f3 = rng.integers(0, 500, size=(900, 3))
    return [(v0, f0, True), (v1, f1, False), (v2, f2, True), (v3, f3, True)]


def _setup():
    ms = _meshes()
    V = sum(m[0].shape[0] for m in ms)
    pos = np.concatenate([m[0] for m in ms]).astype(np.float32)
    tri, table, vb = [], (S.EpsmMesh * len(ms))(), [0]
    toff = 0
    for i, (v, f, flagged) in enumerate(ms):
        tri.append(f + vb[-1])
        c = table[i]
        c.tri_begin, c.tri_count, c.cdf_begin = toff, f.shape[0], toff
        c.flags = S.MESH_IS_MESH | (S.MESH_VERTEX_NORMALS if flagged else 0)
        c.emitter, c.area = -1, -7.0
        toff += f.shape[0]
        vb.append(vb[-1] + v.shape[0])
    tri = np.concatenate(tri).astype(np.int32)
    assert V == vb[-1]
    return ms, pos, tri, table, vb


@pytest.fixture(scope="module")
def tables():
    ms, pos, tri, table, vb = _setup()
    P = torch.from_numpy(pos).to(DEV)
    TRI = torch.from_numpy(tri).to(DEV)
    top = st.SceneTopology(TRI, P.shape[0])
    runs = []
    for _ in range(2):
        nrm = torch.full_like(P, 7.0)
        mesh_buf = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
        cdf = torch.full((tri.shape[0],), -1.0, dtype=torch.float32, device=DEV)
        st.vertex_normals(P, top, table, vb, nrm)
        st.emitter_tables(P, TRI, table, mesh_buf, cdf)
        torch.cuda.synchronize()
        runs.append((nrm.cpu().numpy(), cdf.cpu().numpy(), mesh_buf.cpu().numpy()))
    return ms, pos, tri, table, vb, runs


def test_topology_is_a_stable_csr_of_the_corners():
    rng = np.random.default_rng(2)
    V, T = 3000, 5000
    tri = rng.integers(0, V - 10, size=(T, 3)).astype(np.int32)     # the last ten vertices unreferenced
    tri[7] = [4, 4, 4]
    top = st.SceneTopology(torch.from_numpy(tri).to(DEV), V)
    torch.cuda.synchronize()
    raw = top.buf.cpu().numpy().view(np.uint32)
    row = raw[:V + 1]
    adj_at = -(-4 * (V + 1) // 256) * 256 // 4
    adj = raw[adj_at:adj_at + 3 * T]
    order = np.argsort(tri.reshape(-1), kind="stable")
    counts = np.bincount(tri.reshape(-1), minlength=V)
    assert row[0] == 0 and np.array_equal(np.diff(row.astype(np.int64)), counts)
    assert np.array_equal(adj, order.astype(np.uint32))


def test_vertex_normals_match_the_fp64_rule(tables):
    ms, pos, tri, table, vb, runs = tables
    nrm = runs[0][0]
    for i, (v, f, flagged) in enumerate(ms):
        got = nrm[vb[i]:vb[i + 1]]
        if not flagged:
            assert np.all(got == 7.0), "an unflagged mesh's rows must be left alone"
            continue
        want = S.vertex_normals(pos[vb[i]:vb[i + 1]].astype(np.float64), f)
        err = np.abs(got.astype(np.float64) - want).max()
        assert err <= 2e-6, (i, err)
    # unreferenced vertices of a flagged mesh: (0, 0, 1)
    assert np.array_equal(nrm[29], [0, 0, 1]) and np.array_equal(nrm[39], [0, 0, 1])


def test_cdfs_and_areas_match_numpy_on_the_same_float32_positions(tables):
    ms, pos, tri, table, vb, runs = tables
    _, cdf, mesh_buf = runs[0]
    area = mesh_buf.view(np.float32).reshape(-1, 8)[:, 5]
    for i, c in enumerate(table):
        p = pos.astype(np.float64)[tri[c.tri_begin:c.tri_begin + c.tri_count]]
        a = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
        want = (np.cumsum(a) / max(a.sum(), 1e-30)).astype(np.float32)
        got = cdf[c.cdf_begin:c.cdf_begin + c.tri_count]
        ulp = np.spacing(np.abs(want))
        assert np.all(np.abs(got - want) <= 2 * ulp), (i, np.abs(got - want).max())
        assert got[-1] == 1.0
        wa = np.float32(a.sum())
        assert abs(area[i] - wa) <= 2 * np.spacing(wa), (i, area[i], wa)
    # nothing but `area` changed in the device table
    before = np.frombuffer(bytes(table), dtype=np.uint8).view(np.int32).reshape(-1, 8)
    after = mesh_buf.view(np.int32).reshape(-1, 8)
    assert np.array_equal(np.delete(after, 5, axis=1), np.delete(before, 5, axis=1))
    assert not np.array_equal(after[:, 5], before[:, 5])


def test_two_calls_are_bitwise_equal(tables):
    runs = tables[-1]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_a_sub_range_of_the_table_updates_only_those_meshes(tables):
    ms, pos, tri, table, vb, runs = tables
    P = torch.from_numpy(pos).to(DEV)
    TRI = torch.from_numpy(tri).to(DEV)
    mesh_buf = torch.from_numpy(runs[0][2].copy()).to(DEV)
    cdf = torch.from_numpy(runs[0][1].copy()).to(DEV)
    P[vb[3]:vb[4]] *= 2.0                                   # mesh 3 grows: area x 4, same CDF
    st.emitter_tables(P, TRI, table, mesh_buf, cdf, first=3, count=1)
    torch.cuda.synchronize()
    area = mesh_buf.cpu().numpy().view(np.float32).reshape(-1, 8)[:, 5]
    old = runs[0][2].view(np.float32).reshape(-1, 8)[:, 5]
    assert np.array_equal(area[:3], old[:3])
    assert abs(area[3] / old[3] - 4.0) < 1e-6
    assert np.allclose(cdf.cpu().numpy(), runs[0][1], rtol=0, atol=2e-7)


def test_cdf_layout_independent_of_the_triangle_layout(tables):
    """cdf_begin need not equal tri_begin: the same meshes with their CDFs laid out in reverse order."""
    ms, pos, tri, table, vb, runs = tables
    P = torch.from_numpy(pos).to(DEV)
    TRI = torch.from_numpy(tri).to(DEV)
    moved = (S.EpsmMesh * len(table))()
    C = __import__("ctypes")
    C.memmove(moved, table, C.sizeof(moved))
    off = 5                                                  # and an offset in front of the first
    for c in reversed(moved):
        c.cdf_begin, off = off, off + c.tri_count
    cdf = torch.full((off,), -1.0, dtype=torch.float32, device=DEV)
    buf = torch.frombuffer(bytearray(bytes(moved)), dtype=torch.uint8).to(DEV)
    st.emitter_tables(P, TRI, moved, buf, cdf)
    torch.cuda.synchronize()
    got, want = cdf.cpu().numpy(), runs[0][1]
    assert np.all(got[:5] == -1.0)
    for a, b in zip(moved, table):
        assert np.array_equal(got[a.cdf_begin:a.cdf_begin + a.tri_count], want[b.cdf_begin:b.cdf_begin + b.tri_count])
    assert np.array_equal(buf.cpu().numpy().view(np.float32).reshape(-1, 8)[:, 5], runs[0][2].view(np.float32).reshape(-1, 8)[:, 5])


def _env_cases():
    rng = np.random.default_rng(5)
    m = rng.uniform(0, 3, size=(33, 64, 3))
    z = m.copy(); z[5] = 0; z[6] = 0                       # zero cells (two zero texel rows: one zero cell row)
    wide = rng.uniform(0, 1, size=(9, 1500, 3)) ** 4
    return {"random": m, "zero rows": z, "all zero": np.zeros((16, 32, 3)), "smallest": rng.uniform(size=(2, 2, 3)), "wide": wide}


@pytest.mark.parametrize("name", list(_env_cases()))
def test_environment_tables_match_the_host_rule(name):
    bm = _env_cases()[name].astype(np.float32)
    want = S.environment_tables(bm.astype(np.float64))
    got = [t.cpu().numpy() for t in st.environment_tables(torch.from_numpy(bm).to(DEV))]
    again = [t.cpu().numpy() for t in st.environment_tables(torch.from_numpy(bm).to(DEV))]
    for label, g, w, g2 in zip(("texels", "row_cdf", "col_cdf", "cell_pdf"), got, want, again):
        assert g.shape == w.shape, (label, g.shape, w.shape)
        assert np.allclose(g, w, rtol=1e-6, atol=1e-12), (name, label, np.abs(g - w).max())
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)), (name, label)
    assert got[1][-1] == 1.0 and np.all(got[2][:, -1] == 1.0)
