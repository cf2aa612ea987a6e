"""The device BVH's C ABI (include/epsm_trace.h: epsm_bvh_max_nodes / _workspace_bytes / _build / _refit) without a device:
the symbols are exported, every invalid argument is refused with EPSM_EINVAL and a message before anything touches the
device, the capacities are consistent."""
import ctypes as C

import pytest

EINVAL = -22
SYMBOLS = ["epsm_bvh_max_nodes", "epsm_bvh_workspace_bytes", "epsm_bvh_build", "epsm_bvh_refit"]
FAKE = 0x1000                # a non-NULL device address: validation must fail before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    import os
    from epsm_mitsuba3_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_are_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_capacities(lib):
    for T in (1, 2, 6, 7, 100, 128004, 1 << 20):
        assert lib.epsm_bvh_max_nodes(T) >= max(1, T - 1)
    sizes = [lib.epsm_bvh_workspace_bytes(T) for T in (1, 2, 7, 100, 1000, 128004, 1 << 20, 1 << 24)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    per_tri = (lib.epsm_bvh_workspace_bytes(1 << 24) - lib.epsm_bvh_workspace_bytes(1 << 20)) / ((1 << 24) - (1 << 20))
    assert per_tri < 256                                  # linear in T (the header documents the bytes per triangle)


def _build(lib, T=100, V=300, pos=FAKE, tri=FAKE, nodes=FAKE, prim=FAKE, tv=FAKE, nn=True, lb=True, nl=True, ws=FAKE, ws_bytes=None):
    n_nodes, n_levels = C.c_int32(0), C.c_int32(0)
    level_begin = (C.c_int32 * 17)()
    if ws_bytes is None:
        ws_bytes = lib.epsm_bvh_workspace_bytes(max(T, 1))
    return lib.epsm_bvh_build(pos, V, tri, T, nodes, prim, tv, C.byref(n_nodes) if nn else None, level_begin if lb else None,
                              C.byref(n_levels) if nl else None, ws, ws_bytes, None)


@pytest.mark.parametrize("case,kw,msg", [
    ("T < 1", dict(T=0), b"T must be >= 1"),
    ("T negative", dict(T=-5), b"T must be >= 1"),
    ("T >= 2^28", dict(T=1 << 28, ws_bytes=1 << 62), b"2^28"),
    ("positions NULL", dict(pos=None), b"NULL"),
    ("tri NULL", dict(tri=None), b"NULL"),
    ("nodes NULL", dict(nodes=None), b"NULL"),
    ("prim_index NULL", dict(prim=None), b"NULL"),
    ("tri_verts NULL", dict(tv=None), b"NULL"),
    ("n_nodes NULL", dict(nn=False), b"NULL"),
    ("level_begin NULL", dict(lb=False), b"NULL"),
    ("n_levels NULL", dict(nl=False), b"NULL"),
    ("workspace NULL", dict(ws=None), b"NULL"),
    ("workspace too small", dict(ws_bytes=1024), b"workspace"),
])
def test_build_refuses_invalid_arguments(lib, case, kw, msg):
    assert _build(lib, **kw) == EINVAL, case
    assert msg in lib.epsm_last_error(), (case, lib.epsm_last_error())


def test_build_refuses_a_workspace_one_byte_short(lib):
    assert _build(lib, T=1000, ws_bytes=lib.epsm_bvh_workspace_bytes(1000) - 1) == EINVAL
    assert b"workspace" in lib.epsm_last_error()


def _refit(lib, T=100, V=300, pos=FAKE, tri=FAKE, prim=FAKE, nodes=FAKE, n_nodes=5, levels=(0, 1, 5), tv=FAKE, lb=True):
    n_levels = len(levels) - 1
    level_begin = (C.c_int32 * max(1, len(levels)))(*levels)
    return lib.epsm_bvh_refit(pos, V, tri, prim, T, nodes, n_nodes, level_begin if lb else None, n_levels, tv, None)


@pytest.mark.parametrize("case,kw,msg", [
    ("T < 1", dict(T=0), b"T must be >= 1"),
    ("T >= 2^28", dict(T=1 << 28), b"2^28"),
    ("positions NULL", dict(pos=None), b"NULL"),
    ("tri NULL", dict(tri=None), b"NULL"),
    ("prim_index NULL", dict(prim=None), b"NULL"),
    ("nodes NULL", dict(nodes=None), b"NULL"),
    ("tri_verts NULL", dict(tv=None), b"NULL"),
    ("level_begin NULL", dict(lb=False), b"NULL"),
    ("n_levels > 16", dict(levels=tuple(range(18)), n_nodes=17), b"n_levels"),
    ("n_levels < 1", dict(levels=(0,), n_nodes=1), b"n_levels"),
    ("level table does not end at n_nodes", dict(levels=(0, 1, 4), n_nodes=5), b"level_begin"),
    ("level table decreases", dict(levels=(0, 3, 2, 5), n_nodes=5), b"level_begin"),
])
def test_refit_refuses_invalid_arguments(lib, case, kw, msg):
    assert _refit(lib, **kw) == EINVAL, case
    assert msg in lib.epsm_last_error(), (case, lib.epsm_last_error())


def test_level_table_of_a_host_built_tree():
    """The refit takes the host builder's tree too: its level table is derived from the breadth-first node order."""
    import numpy as np
    from epsm_mitsuba3_amd import scene as S
    from epsm_mitsuba3_amd.bvh import level_table
    rng = np.random.default_rng(5)
    t = 3000
    pos = rng.uniform(-1, 1, size=(3 * t, 3))
    tri = np.arange(3 * t, dtype=np.int64).reshape(t, 3)
    plan = S.build_bvh(pos, tri)
    lb = level_table(plan["nodes"])
    assert lb[0] == 0 and lb[-1] == plan["nodes"].shape[0] and 1 < len(lb) - 1 <= 16
    assert len(lb) - 1 == len(plan["levels"]) + 1                    # one level of inner-slot updates per level above the deepest
    small = S.build_bvh(pos[:15], tri[:5])                           # T <= 6: one node, one leaf
    assert level_table(small["nodes"]) == [0, 1]
