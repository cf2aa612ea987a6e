"""The tracer's BVH traversal ray by ray, on the host build of it (epsm_probe_rays of tests/host_harness/trace_host.cpp: the
tracer's intersect on the stacks epsm_trace_paths and epsm_trace_paths_wavefront give a path): every ray of every family is
accounted for by the brute-force float64 oracle of tests/_ray_query.py, on trees whose walk overflows both stack caps."""
import ctypes as C

import numpy as np
import pytest

import _ray_query as Q
from _scenes import host_tracer

HOST_FORMS = (Q.LANE, Q.LANE_ANY, Q.WAVEFRONT, Q.WAVEFRONT_ANY)
TREES = ["chain", "uniform", "degenerate", "one_centroid"] + [f"T{t}" for t in range(1, 8)]


@pytest.fixture(scope="module")
def lib():
    return Q.declare(host_tracer())


@pytest.fixture(scope="module")
def trees():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Q.build_tree(name, "host", "cpu")
        return cache[name]
    return get


def test_the_probe_is_exported_by_the_product_library_and_the_host_harness(lib):
    from epsm_mitsuba3_amd import _lib
    for l in (lib, _lib.lib()):
        assert hasattr(l, "epsm_probe_rays") and hasattr(l, "epsm_probe_rays_workspace_bytes")
    for l in (lib, Q.declare(_lib.lib())):
        assert l.epsm_probe_rays_workspace_bytes(Q.LANE, 1000) == 0 and l.epsm_probe_rays_workspace_bytes(Q.PACKET, 1000) == 0
        assert l.epsm_probe_rays_workspace_bytes(Q.WAVEFRONT, 1000) == 1000 * 4 * (Q.K_BVH_STACK - Q.K_WF_STACK_LDS)
        assert l.epsm_probe_rays_workspace_bytes(Q.WAVEFRONT_ANY, 0) == 0


@pytest.mark.parametrize("name", TREES)
def test_undecided_share_of_every_family_is_capped(name, trees):
    """From the oracle alone, before any traversal is looked at: at most 10 % of a family's rays may be undecided, under the
    closest-hit and under the any-hit rule (measured shares: the families' docstrings in tests/_ray_query.py)."""
    for family, (rays, oracle) in Q.families(name, trees(name).host_nodes()).items():
        assert rays.shape[0] <= 2048 and oracle.n == rays.shape[0]
        for any_hit in (False, True):
            share = oracle.undecided_share(any_hit)
            print(f"{name} {family} ({'any' if any_hit else 'closest'} hit): {rays.shape[0]} rays, undecided {share:.4f}")
            assert share <= Q.UNDECIDED_CAP, (name, family, any_hit, share)
        if not family.startswith("axis"):
            assert (oracle.classify(False).tri >= 0).mean() >= 0.4, "the family hardly hits anything"


def test_deep_family_overflows_both_stack_caps(trees):
    """The walk of the host builder's chain from its corner: measured peak 47 entries of kBvhStack = 48, every one of the 2 048
    rays above the 32 entries the one-launch kernels keep in LDS (and above the wavefront kernels' 16)."""
    tree = trees("chain")
    rays, _ = Q.deep_family()
    peak = Q.peak_stack_depth(tree.host_nodes(), tree.host_tri_verts(), rays)
    print("chain, host builder: peak stack depth", int(peak.max()), "rays above 32:", int((peak > Q.K_LANE_STACK_LDS).sum()))
    assert (peak > Q.K_LANE_STACK_LDS).sum() >= 64
    assert 40 <= peak.max() <= Q.K_BVH_STACK


def test_one_centroid_family_overflows_the_wavefront_cap(trees):
    """Measured on the host builder's tree: peak 24 entries, past the 16 the wavefront kernels keep in LDS."""
    tree = trees("one_centroid")
    rays, _ = Q.interior_family("one_centroid")
    peak = Q.peak_stack_depth(tree.host_nodes(), tree.host_tri_verts(), rays[:64])
    print("one centroid, host builder: peak stack depth", int(peak.max()))
    assert Q.K_WF_STACK_LDS < peak.max() <= Q.K_BVH_STACK


@pytest.mark.parametrize("name", TREES)
def test_every_ray_is_accounted_for(name, lib, trees):
    tree = trees(name)
    for family, (rays, oracle) in Q.families(name, tree.host_nodes()).items():
        Q.account(lib, tree, rays, oracle, HOST_FORMS, label=f"host twin, {name}, {family}")


def test_two_stack_homes_give_the_same_bits_on_the_deep_family(lib, trees):
    """intersect on kBvhStack words of its own against intersect on 16 words + the strided overflow: only the stack's home differs."""
    tree = trees("chain")
    rays, _ = Q.deep_family()
    for a, b in ((Q.LANE, Q.WAVEFRONT), (Q.LANE_ANY, Q.WAVEFRONT_ANY)):
        assert np.array_equal(Q.probe(lib, tree, a, rays), Q.probe(lib, tree, b, rays))


def test_masked_rows_report_a_miss(lib, trees):
    tree = trees("uniform")
    rays, oracle = Q.interior_family("uniform")
    mask = np.random.default_rng(3).uniform(size=rays.shape[0]) < 0.5
    r, o = Q.masked(rays, oracle, mask)
    _, outs = Q.account(lib, tree, r, o, HOST_FORMS, label="host twin, uniform, interior with a random mask")
    assert (outs[Q.LANE][~mask, 0] == Q.MISS).all() and (outs[Q.LANE][mask, 0] != Q.MISS).mean() > 0.9


def test_empty_scene_misses_and_terminates(lib):
    rays, oracle = Q.empty_family()
    _, outs = Q.account(lib, Q.EmptyTree("cpu"), rays, oracle, HOST_FORMS, label="host twin, empty scene")
    assert (outs[Q.WAVEFRONT][:, 0] == Q.MISS).all()


def test_zero_area_triangles_are_never_reported(lib, trees):
    tree = trees("degenerate")
    flat = np.nonzero(Q.zero_area(Q.triangle_verts("degenerate")))[0]
    assert flat.size == 50
    for family, (rays, _) in Q.families("degenerate", tree.host_nodes()).items():
        for form in HOST_FORMS:
            assert not np.isin(Q.probe(lib, tree, form, rays)[:, 0], flat).any(), (family, form)


def test_argument_refusals(lib, trees):
    import torch
    tree = trees("T3")
    rays = torch.from_numpy(Q.interior_family("T3", 256)[0])
    out = torch.zeros((256, 4), dtype=torch.int32)
    ws = torch.zeros(256 * 32, dtype=torch.int32)
    sc, r, o, w = C.byref(tree.struct), rays.data_ptr(), out.data_ptr(), ws.data_ptr()
    need = lib.epsm_probe_rays_workspace_bytes(Q.WAVEFRONT, 256)
    assert lib.epsm_probe_rays(sc, Q.WAVEFRONT, 256, r, o, w, need, None) == 0
    assert lib.epsm_probe_rays(sc, Q.LANE, 0, None, None, None, 0, None) == 0              # n == 0
    assert lib.epsm_probe_rays(sc, Q.LANE, 256, r, o, None, 0, None) == 0                  # no workspace needed
    assert lib.epsm_probe_rays(sc, 5, 256, r, o, w, need, None) == -22                     # unknown form
    assert lib.epsm_probe_rays(sc, -1, 256, r, o, w, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.PACKET, 256, r, o, w, need, None) == -22              # device only
    assert lib.epsm_probe_rays(None, Q.LANE, 256, r, o, w, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.LANE, 256, None, o, w, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.LANE, 256, r, None, w, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.LANE, -1, r, o, w, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.WAVEFRONT, 256, r, o, None, need, None) == -22
    assert lib.epsm_probe_rays(sc, Q.WAVEFRONT_ANY, 256, r, o, w, need - 1, None) == -22
    assert (out.numpy() != 0).any()


def test_the_product_library_refuses_before_any_launch():
    """The same refusals by libepsm_hip.so, on a machine with or without a GPU: nothing touches a device."""
    from epsm_mitsuba3_amd import _lib
    from epsm_mitsuba3_amd import scene as S
    lib = Q.declare(_lib.lib())
    sc = S.EpsmSceneC()
    one = C.c_void_p(16)                                                                   # never dereferenced
    assert lib.epsm_probe_rays(C.byref(sc), Q.LANE, 0, None, None, None, 0, None) == 0
    assert lib.epsm_probe_rays(C.byref(sc), 5, 4, one, one, None, 0, None) == -22 and b"unknown form" in lib.epsm_last_error()
    assert lib.epsm_probe_rays(None, Q.LANE, 4, one, one, None, 0, None) == -22
    assert lib.epsm_probe_rays(C.byref(sc), Q.PACKET, 4, None, one, None, 0, None) == -22
    assert lib.epsm_probe_rays(C.byref(sc), Q.LANE, 4, one, None, None, 0, None) == -22
    assert lib.epsm_probe_rays(C.byref(sc), Q.WAVEFRONT, 4, one, one, None, 512, None) == -22
    assert lib.epsm_probe_rays(C.byref(sc), Q.WAVEFRONT, 4, one, one, one, 511, None) == -22 and b"workspace" in lib.epsm_last_error()
    sc.n_nodes = 3                                                                         # nodes but no tables
    assert lib.epsm_probe_rays(C.byref(sc), Q.LANE, 4, one, one, None, 0, None) == -22
