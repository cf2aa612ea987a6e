"""The C ABI of the recomputed normals' derivative (include/epsm_trace.h: epsm_vertex_normals_backward_bytes,
epsm_vertex_normals_backward, epsm_vertex_normals_forward) without a device: the symbols are exported, every invalid argument is
refused with EPSM_EINVAL and a message before anything touches the device (the device pointers are fake), and a call with nothing
to do is not an error."""
import ctypes as C

import pytest

EINVAL = -22
FAKE = 0x1000                # a non-NULL, aligned device address: validation must fail before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    import os
    from epsm_mitsuba3_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _meshes(ranges, flags=1):
    from epsm_mitsuba3_amd.scene import EpsmMesh
    a = (EpsmMesh * max(1, len(ranges)))()
    for c, (t0, n, c0) in zip(a, ranges):
        c.tri_begin, c.tri_count, c.cdf_begin, c.flags = t0, n, c0, flags
    return a


def _call(lib, entry, V=300, T=100, pos=FAKE, tri=FAKE, top=FAKE, meshes=True, ranges=((0, 60, 0), (60, 40, 60)), vb=(0, 150, 300),
          n=None, src=FAKE, dst=FAKE, ws=FAKE, ws_bytes=None):
    m = _meshes(ranges) if meshes else None
    vba = (C.c_int64 * len(vb))(*vb) if vb is not None else None
    n = len(ranges) if n is None else n
    if entry == "forward":
        return lib.epsm_vertex_normals_forward(pos, V, tri, T, top, m, vba, n, src, dst, None)
    ws_bytes = lib.epsm_vertex_normals_backward_bytes(max(V, 1)) if ws_bytes is None else ws_bytes
    return lib.epsm_vertex_normals_backward(pos, V, tri, T, top, m, vba, n, src, dst, ws, ws_bytes, None)


def test_symbols_are_exported(lib):
    for s in ("epsm_vertex_normals_backward_bytes", "epsm_vertex_normals_backward", "epsm_vertex_normals_forward"):
        assert hasattr(lib, s), s


def test_the_workspace_is_three_doubles_per_vertex(lib):
    sizes = [lib.epsm_vertex_normals_backward_bytes(V) for V in (0, 1, 2, 100, 642, 1 << 20, 1 << 30)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s >= 24 * V for s, V in zip(sizes, (0, 1, 2, 100, 642, 1 << 20, 1 << 30)))


BOTH = [
    ("T negative", dict(T=-1), b"T must be"),
    ("T >= 2^28", dict(T=1 << 28), b"2^28"),
    ("V negative", dict(V=-1), b"V must be"),
    ("V >= 2^31", dict(V=1 << 31), b"2^31"),
    ("n_meshes negative", dict(n=-1), b"n_meshes"),
    ("positions NULL", dict(pos=None), b"NULL"),
    ("tri NULL", dict(tri=None), b"NULL"),
    ("topology NULL", dict(top=None), b"NULL"),
    ("input rows NULL", dict(src=None), b"NULL"),
    ("output rows NULL", dict(dst=None), b"NULL"),
    ("meshes NULL", dict(meshes=False), b"NULL"),
    ("vertex_begin NULL", dict(vb=None), b"NULL"),
    ("topology misaligned", dict(top=FAKE + 4), b"aligned"),
    ("mesh beyond T", dict(ranges=((0, 60, 0), (60, 41, 60))), b"beyond T"),
    ("meshes overlap", dict(ranges=((0, 60, 0), (30, 60, 60))), b"overlap"),
    ("vertex range beyond V", dict(vb=(0, 150, 301)), b"vertex_begin"),
    ("vertex ranges decrease", dict(vb=(0, 200, 150)), b"vertex_begin"),
    ("vertex range negative", dict(vb=(-1, 150, 300)), b"vertex_begin"),
]
BACKWARD_ONLY = [
    ("workspace NULL", dict(ws=None), b"NULL"),
    ("workspace too small", dict(ws_bytes=64), b"workspace smaller"),
    ("workspace one byte short", dict(ws_bytes=24 * 300 - 1), b"workspace smaller"),
    ("workspace misaligned", dict(ws=FAKE + 8), b"aligned"),
]


@pytest.mark.parametrize("entry", ["backward", "forward"])
@pytest.mark.parametrize("case,kw,msg", BOTH)
def test_invalid_arguments_are_refused(lib, entry, case, kw, msg):
    assert _call(lib, entry, **kw) == EINVAL, case
    assert msg in lib.epsm_last_error(), (case, lib.epsm_last_error())
    assert (b"backward" if entry == "backward" else b"forward") in lib.epsm_last_error()


@pytest.mark.parametrize("case,kw,msg", BACKWARD_ONLY)
def test_backward_refuses_a_bad_workspace(lib, case, kw, msg):
    assert _call(lib, "backward", **kw) == EINVAL, case
    assert msg in lib.epsm_last_error(), (case, lib.epsm_last_error())


@pytest.mark.parametrize("entry", ["backward", "forward"])
def test_nothing_to_do_is_not_an_error(lib, entry):
    """V == 0, no triangle or an empty table: EPSM_OK without a launch (so also without a device)."""
    assert _call(lib, entry, V=0, vb=(0, 0, 0)) == 0
    assert _call(lib, entry, ranges=(), vb=(0,), n=0) == 0
    assert _call(lib, entry, T=0, ranges=((0, 0, 0),), vb=(0, 300)) == 0
    assert _call(lib, entry, V=0, T=0, n=0, pos=None, tri=None, top=None, meshes=False, vb=None, src=None, dst=None, ws=None, ws_bytes=0) == 0
