"""The tracer's BVH traversal ray by ray on the device (epsm_probe_rays, csrc/epsm_trace_probe.hip): intersect on the
one-launch kernels' stack (32 entries in LDS + a private array) and on the wavefront kernels' (16 entries in LDS + the
workspace, strided), closest hit and any hit, and the wave-packet walk -- on the host builder's and the device builder's
trees.  Every ray of every family is accounted for by the brute-force float64 oracle of tests/_ray_query.py.

Measured on an MI355X.  Peak stack depth of the walk as tests/_ray_query.py restates it: chain 47 of 48 entries on the host
builder's tree and 47 on the device builder's (all 2 048 deep rays above 32); one-centroid soup 24 and 23.  Worst deviations on
decided rays over all trees, families and forms: |dt| / t 4.2e-5, |du| 5.1e-5, |dv| 4.1e-5 (allowed: 2e-4, 5e-3, 5e-3)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _ray_query as Q

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FORMS = (Q.LANE, Q.LANE_ANY, Q.WAVEFRONT, Q.WAVEFRONT_ANY, Q.PACKET)
BUILDERS = ("host", "device")
TREES = ["chain", "uniform", "degenerate", "one_centroid"] + [f"T{t}" for t in range(1, 8)]


@pytest.fixture(scope="module")
def lib():
    from epsm_mitsuba3_amd import _lib
    return Q.declare(_lib.lib())


@pytest.fixture(scope="module")
def trees():
    cache = {}

    def get(name, builder):
        if (name, builder) not in cache:
            cache[name, builder] = Q.build_tree(name, builder, DEV)
            torch.cuda.synchronize()
        return cache[name, builder]
    return get


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", TREES)
def test_every_ray_is_accounted_for(name, builder, lib, trees):
    """Forms 0-4 at n = 1, 63, 64, 65, 200 and the whole family; the undecided share is asserted first, from the oracle alone
    (the in-plane axis rays depend on the tree's own boxes)."""
    tree = trees(name, builder)
    for family, (rays, oracle) in Q.families(name, tree.host_nodes()).items():
        for any_hit in (False, True):
            assert oracle.undecided_share(any_hit) <= Q.UNDECIDED_CAP, (name, builder, family, any_hit)
        Q.account(lib, tree, rays, oracle, FORMS, label=f"device, {builder} builder, {name}, {family}")


@pytest.mark.parametrize("builder", BUILDERS)
def test_stack_reach_on_the_device_trees(builder, trees):
    """The deep family must keep testing what it is for, on the nodes the DEVICE holds: at least 64 rays above the 32 entries
    of the one-launch kernels' LDS share, the family's peak within [40, 48]; the one-centroid family above the wavefront
    kernels' 16."""
    tree = trees("chain", builder)
    peak = Q.peak_stack_depth(tree.host_nodes(), tree.host_tri_verts(), Q.deep_family()[0])
    print(f"chain, {builder} builder: peak stack depth {int(peak.max())}, rays above 32: {int((peak > Q.K_LANE_STACK_LDS).sum())}")
    assert (peak > Q.K_LANE_STACK_LDS).sum() >= 64
    assert 40 <= peak.max() <= Q.K_BVH_STACK
    tree = trees("one_centroid", builder)
    peak = Q.peak_stack_depth(tree.host_nodes(), tree.host_tri_verts(), Q.interior_family("one_centroid")[0][:64])
    print(f"one centroid, {builder} builder: peak stack depth {int(peak.max())}")
    assert Q.K_WF_STACK_LDS < peak.max() <= Q.K_BVH_STACK


@pytest.mark.parametrize("builder", BUILDERS)
def test_stack_homes_and_the_packet_agree_on_the_deep_family(builder, lib, trees):
    """Forms 0 / 2 and 1 / 3 run intersect on the same code path, only the stack's home differs: the same triangle and the same
    bits of t, u, v on every decided ray.  The packet walk differs from the per-lane walk only in the order among hits at
    exactly the same distance, which are undecided by construction: the same triangle on every decided ray."""
    tree = trees("chain", builder)
    rays, oracle = Q.deep_family()
    out = {f: Q.probe(lib, tree, f, rays) for f in FORMS}
    for a, b in ((Q.LANE, Q.WAVEFRONT), (Q.LANE_ANY, Q.WAVEFRONT_ANY)):
        decided = oracle.classify(Q.ANY_HIT[a]).decided
        assert decided.sum() > 1900
        assert np.array_equal(out[a][decided], out[b][decided]), (a, b)
    decided = oracle.classify(False).decided
    assert np.array_equal(out[Q.PACKET][decided, 0], out[Q.LANE][decided, 0])


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["uniform", "one_centroid", "chain"])
def test_packets_of_incoherent_and_masked_lanes(name, builder, lib, trees):
    """The wave-packet walk with the rows of a tree's families shuffled, so that the 64 lanes of a wave share nothing and the
    wave's stack holds the union of their pushes -- all lanes, a random half, only lane 0, only lane 63, none (which must
    report misses and terminate) -- and, on the chain, one wave whose 64 lanes are all deep rays: what holds
    kPacketStack = 64 >= 3 x 16 (csrc/epsm_trace_packet.h).  The per-lane forms take the same rows: a masked row is a miss."""
    tree = trees(name, builder)
    rays, oracle = Q.packet_rows(list(Q.families(name, tree.host_nodes()).values()))
    n = rays.shape[0]
    lane = np.arange(n) % 64
    masks = {"all": np.ones(n, bool), "random": np.random.default_rng(8).uniform(size=n) < 0.5, "lane 0": lane == 0,
             "lane 63": lane == 63, "none": np.zeros(n, bool)}
    for what, mask in masks.items():
        r, o = Q.masked(rays, oracle, mask)
        _, outs = Q.account(lib, tree, r, o, FORMS, sizes=(65,), label=f"device, {builder} builder, {name}, shuffled rows, mask: {what}")
        for form in FORMS:
            assert (outs[form][~mask, 0] == Q.MISS).all(), (what, form)
    if name == "chain":
        Q.account(lib, tree, rays[:64], oracle.take(np.arange(64)), (Q.PACKET,), sizes=(64,), label=f"device, {builder} builder, one wave of deep rays")


@pytest.mark.parametrize("builder", BUILDERS)
def test_empty_scene_misses_and_terminates(builder, lib):
    rays, oracle = Q.empty_family()
    _, outs = Q.account(lib, Q.EmptyTree(DEV), rays, oracle, FORMS, label="device, empty scene")
    for form in FORMS:
        assert (outs[form][:, 0] == Q.MISS).all()


@pytest.mark.parametrize("builder", BUILDERS)
def test_zero_area_triangles_are_never_reported(builder, lib, trees):
    tree = trees("degenerate", builder)
    flat = np.nonzero(Q.zero_area(Q.triangle_verts("degenerate")))[0]
    for family, (rays, _) in Q.families("degenerate", tree.host_nodes()).items():
        for form in FORMS:
            assert not np.isin(Q.probe(lib, tree, form, rays)[:, 0], flat).any(), (family, form)


@pytest.mark.parametrize("builder", BUILDERS)
def test_second_call_after_a_refit_that_moved_the_soup(builder, lib):
    """The tree is refitted in place (same pointers) after every vertex of the uniform soup moved; the moved soup's own oracle
    accounts for every ray again."""
    tree = Q.build_tree("uniform", builder, DEV)
    rays, oracle = Q.interior_family("uniform")
    Q.account(lib, tree, rays, oracle, FORMS, sizes=(), label=f"device, {builder} builder, uniform, before the refit")
    pos, tri = Q.geometry("uniform")
    rng = np.random.default_rng(12)
    moved = (pos * 1.25 + np.array([0.3, -0.2, 0.1]) + rng.normal(size=pos.shape) * 0.01).astype(np.float32).astype(np.float64)
    ptr = tree.bvh.nodes.data_ptr()
    tree.refit(moved, tri)
    torch.cuda.synchronize()
    assert tree.bvh.nodes.data_ptr() == ptr
    after = Q.Oracle(rays, moved[tri])
    assert after.undecided_share() <= Q.UNDECIDED_CAP
    c0, c1 = oracle.classify(False), after.classify(False)
    assert ((c0.tri != c1.tri) & c0.decided & c1.decided).mean() > 0.5          # the answers did change
    Q.account(lib, tree, rays, after, FORMS, sizes=(), label=f"device, {builder} builder, uniform, after the refit")


def test_argument_refusals_on_the_device(lib, trees):
    tree = trees("T3", "host")
    rays = torch.from_numpy(Q.interior_family("T3", 256)[0]).to(DEV)
    out = torch.zeros((256, 4), dtype=torch.int32, device=DEV)
    need = lib.epsm_probe_rays_workspace_bytes(Q.WAVEFRONT, 256)
    ws = torch.zeros(need // 4, dtype=torch.int32, device=DEV)
    sc, r, o, w = C.byref(tree.struct), rays.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert lib.epsm_probe_rays(sc, Q.LANE, 0, None, None, None, 0, None) == 0
    assert lib.epsm_probe_rays(sc, 5, 256, r, o, w, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.WAVEFRONT, 256, r, o, None, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.WAVEFRONT, 256, r, o, w, need - 1, None) == -22
    assert lib.epsm_probe_rays(sc, Q.PACKET, 256, None, o, None, 0, None) == -22
    torch.cuda.synchronize()
    assert not bool(out.any())                                                  # nothing was launched
    assert lib.epsm_probe_rays(sc, Q.PACKET, 256, r, o, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool(out.any())
