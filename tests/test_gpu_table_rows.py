"""The rows of the scene table the backward kernel's emission names (csrc/epsm_backward_cp.hip, table_rows): the hit triangle
of a lane's vertex, the next vertex's -- a neighbour lane's id, or the end-point record's -- the emitter sample's and the
occluder's.  The kernel requests the four together and without a guard, from a substitute row where an id names nothing, and
picks the "no triangle" row afterwards; an id beyond the table must therefore still give exactly what epsm::table_row() gives:
no row at all, and no other row a different value.

Every (path, vertex) has PRIVATE rows (tests/_per_path.py) and every path a private occluder triangle behind them; triangle 0 of
the table -- the substitute row -- is named by no record.  The launch runs once clean and once with a seeded third of the hit,
emitter and occluder ids replaced by T, T + 5 and 0xFFFFFFFF: the private rows of a replaced id must be exactly 0, every other
row must be what the clean run gave (up to the order of float atomics), triangle 0's rows must stay 0.

2 048 paths, K = 3: the smallest shape with rounds of every class 0..3, so that a lane takes the next vertex's id from its
neighbour (k < c) and from the end-point record (k == c), with emitter samples and occluder records, in both window forms."""
import pytest
import torch

from _per_path import private_addressing

pytestmark = pytest.mark.gpu

RES, SPP, K = 16, 8, 3
N = RES * RES * SPP                              # 2 048 paths
NK = N * K
T = 1 + 2 * NK + N                               # substitute row, hit rows, emitter rows, occluder rows
V = 3 * T                                        # every triangle has its own three vertices: triangle t -> 3t, 3t + 1, 3t + 2
BEYOND = (T, T + 5, -1)                          # ids that name no row (-1: 0xFFFFFFFF)


def _addressing(dev, gen):
    """private_addressing() moved up by one triangle -- row 0 is the substitute row, attached like any other and named by nobody --
    with one private occluder triangle per path behind the emitter rows."""
    table, si = private_addressing(N, K, dev, gen)
    table = table.cpu().to(torch.int64)
    table[:, :3] += 3
    p = torch.arange(N, dtype=torch.int64)
    to = 1 + 2 * NK + p
    occ = torch.stack([3 * to, 3 * to + 1, 3 * to + 2, torch.full_like(p, 4)], dim=1)
    table = torch.cat([torch.tensor([[0, 1, 2, 4 | 8 | 1]]), table, occ]).to(torch.int32).to(dev)
    assert table.shape[0] == T
    bits = lambda x: x.to(torch.float32).contiguous().view(torch.int32)
    for k in range(K):
        si[k]["tri"] = si[k]["tri"] + 1
        si[k]["emit"][:, 0] += 1
        si[k]["table"] = table
    sb0, sb1 = torch.rand(N, generator=gen) * 0.5, torch.rand(N, generator=gen) * 0.5
    dis = 0.5 + torch.rand(N, generator=gen)
    si[0]["shadow"] = torch.stack([to.to(torch.int32), bits(sb0), bits(sb1), bits(dis)], dim=1).to(dev)
    return table, si


def _replaced(si, gen, dev):
    """A copy of the records with a seeded third of each kind of id replaced; the masks (K, N), (K, N), (N)."""
    out, masks = [], []
    bad = torch.tensor(BEYOND, dtype=torch.int32)

    def pick(n):
        m = torch.rand(n, generator=gen) < 1.0 / 3.0
        return m, bad[torch.randint(0, 3, (n,), generator=gen)]

    m_tri, m_emit = torch.zeros((K, N), dtype=torch.bool), torch.zeros((K, N), dtype=torch.bool)
    m_occ = torch.zeros(N, dtype=torch.bool)
    for k in range(K):
        r = dict(si[k])
        m_tri[k], v = pick(N)
        r["tri"] = torch.where(m_tri[k].to(dev), v.to(dev), si[k]["tri"])
        m_emit[k], v = pick(N)
        r["emit"] = si[k]["emit"].clone()
        r["emit"][:, 0] = torch.where(m_emit[k].to(dev), v.to(dev), si[k]["emit"][:, 0])
        if k == 0 and si[0].get("shadow") is not None:
            m_occ, v = pick(N)
            r["shadow"] = si[0]["shadow"].clone()
            r["shadow"][:, 0] = torch.where(m_occ.to(dev), v.to(dev), si[0]["shadow"][:, 0])
        out.append(r)
    return out, (m_tri, m_emit, m_occ)


@pytest.mark.usefixtures("window_form")
@pytest.mark.parametrize("records", ["occluders and alpha", "no occluder records", "no alpha gradients"])
@pytest.mark.parametrize("layout", ["packed log", "per-field records"])
@pytest.mark.parametrize("kind,profile", [("manifold", "mixed"), ("manifold_caustic", "pool")])
def test_ids_beyond_the_table_name_no_row(kind, profile, layout, records):
    import epsm_mitsuba3_amd as epsm
    from epsm_mitsuba3_amd.records import PackedLog
    dev = torch.device("cuda", 0)
    scene = epsm.SyntheticScene(res=RES, n_vertices=K, n_scene_vertices=3000, n_bsdfs=4, profile=profile, device=dev, tile_paths=N)
    trace = scene.tile(0, 0, N, seed=17 + K, spp=SPP, K=K)
    gen = torch.Generator().manual_seed(21)
    table, si = _addressing(dev, gen)
    if records == "no occluder records":
        si[0]["shadow"] = None
    B = 0 if records == "no alpha gradients" else NK
    grad_in = (torch.randn((RES, RES, 5), generator=gen) * 1e-3).to(dev)
    integ = epsm.load_dict({"type": kind, "max_depth": 8})

    def run(recs):
        packed = None
        if layout == "packed log":
            # the log is built from the CLEAN records -- from_trace looks the alpha slot up in the table by the triangle id, on the
            # host side of the ABI, where an id beyond the table has no business -- and the ids are then written into its words:
            # word 11 of a record the hit triangle, word 24 the emitter sample's, word 0 of the occluder record the occluder's
            trace.scatter_info = si
            log = PackedLog.from_trace(trace)
            verts = log.verts.clone()
            iv = verts.view(torch.int32)
            for k in range(K):
                iv[:, k, 11] = recs[k]["tri"]
                iv[:, k, 24] = recs[k]["emit"][:, 0]
            shadow = recs[0]["shadow"].clone() if recs[0].get("shadow") is not None else None
            packed = PackedLog(log.rays, log.flags, verts, shadow, log.table, K)
        trace.scatter_info = recs
        params = epsm.ParamGrads(V, B, device=dev)
        integ.backward_from_trace(trace, params, grad_in, packed=packed)
        torch.cuda.synchronize()
        return params

    def rows(p):
        """[hit (K, N, 9) | emitter (K, N, 9) | occluder (N, 9)] of a (V, 3) buffer, and triangle 0's three rows"""
        b = p.cpu()
        return b[3:3 + 3 * NK].view(K, N, 9), b[3 + 3 * NK:3 + 6 * NK].view(K, N, 9), b[3 + 6 * NK:].view(N, 9), b[:3]

    clean = run(si)
    bad_si, (m_tri, m_emit, m_occ) = _replaced(si, gen, dev)
    bad = run(bad_si)
    assert bool(torch.isfinite(clean.flat).all()) and bool(torch.isfinite(bad.flat).all())
    c_hit, c_emit, c_occ, c_sub = rows(clean.pos)
    b_hit, b_emit, b_occ, b_sub = rows(bad.pos)
    cn_hit, cn_emit, cn_occ, cn_sub = rows(clean.nrm)
    bn_hit, bn_emit, bn_occ, bn_sub = rows(bad.nrm)
    nz = lambda x, m: int((x[m].abs().amax(dim=-1) > 0).sum())
    print(kind, profile, layout, records, "clean rows that a replaced id takes away: hit", nz(c_hit, m_tri), "normal", nz(cn_hit, m_tri),
          "emitter", nz(c_emit, m_emit), "occluder", nz(c_occ, m_occ), "of", int(m_tri.sum()), int(m_emit.sum()), int(m_occ.sum()))
    # the clean run has the rows whose ids are replaced: the test bites
    assert nz(c_hit, m_tri) > 0 and nz(cn_hit, m_tri) > 0
    if kind == "manifold":                                           # (caustic: light_grad == 0, no emitter rows)
        assert nz(c_emit, m_emit) > 0
        if records != "no occluder records":
            assert nz(c_occ, m_occ) > 0
    if records == "no occluder records":
        assert float(c_occ.abs().max()) == 0.0 and float(b_occ.abs().max()) == 0.0
    # the substitute row is nobody's: triangle 0's vertices stay 0 in both runs
    for sub in (c_sub, b_sub, cn_sub, bn_sub):
        assert float(sub.abs().max()) == 0.0
    # every private row of a replaced id: exactly 0
    assert float(b_hit[m_tri].abs().max()) == 0.0 and float(bn_hit[m_tri].abs().max()) == 0.0
    assert float(b_emit[m_emit].abs().max()) == 0.0
    if m_occ.any():
        assert float(b_occ[m_occ].abs().max()) == 0.0
    # every other row: the clean run's (the order of the float atomics of a crowded table)
    same = lambda x, y: torch.allclose(x, y, rtol=1e-5, atol=1e-7 * float(y.abs().max()))
    assert same(b_hit[~m_tri], c_hit[~m_tri]) and same(bn_hit[~m_tri], cn_hit[~m_tri])
    assert same(b_emit[~m_emit], c_emit[~m_emit]) and same(b_occ[~m_occ], c_occ[~m_occ])
    assert float(cn_emit.abs().max()) == 0.0 and float(bn_emit.abs().max()) == 0.0 and float(bn_occ.abs().max()) == 0.0
    if B:
        # the alpha slot: the packed log takes it from the hit triangle's row of the table (gone with the row), the per-field
        # records from the BSDF record (untouched)
        ca, ba = clean.alpha.cpu().view(K, N), bad.alpha.cpu().view(K, N)
        assert float(ca.abs().max()) > 0
        if layout == "packed log":
            assert float(ba[m_tri].abs().max()) == 0.0 and same(ba[~m_tri], ca[~m_tri])
        else:
            assert same(ba, ca)
