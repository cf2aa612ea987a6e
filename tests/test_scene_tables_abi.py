"""The device scene tables' C ABI (include/epsm_trace.h: epsm_scene_topology, epsm_vertex_normals, epsm_emitter_tables,
epsm_environment_tables and their *_bytes queries) without a device: the symbols are exported, every invalid argument is
refused with EPSM_EINVAL and a message before anything touches the device (the device pointers are fake), the sizes are
positive and monotone; and the Scene keyword is checked."""
import ctypes as C

import pytest

EINVAL = -22
SYMBOLS = ["epsm_scene_topology_bytes", "epsm_scene_topology_workspace_bytes", "epsm_scene_topology", "epsm_vertex_normals",
           "epsm_emitter_tables_bytes", "epsm_emitter_tables", "epsm_environment_tables_bytes", "epsm_environment_tables"]
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


def _refused(lib, rc, msg, case):
    assert rc == EINVAL, case
    assert msg in lib.epsm_last_error(), (case, lib.epsm_last_error())


def test_symbols_are_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_sizes_are_positive_and_monotone(lib):
    Ts = (1, 2, 7, 100, 1000, 128004, 1 << 20, 1 << 24)
    for f in (lambda T: lib.epsm_scene_topology_bytes(T, T), lambda T: lib.epsm_scene_topology_bytes(3 * T, T),
              lib.epsm_scene_topology_workspace_bytes, lambda T: lib.epsm_emitter_tables_bytes(T, 1),
              lambda T: lib.epsm_emitter_tables_bytes(T, 40)):
        sizes = [f(T) for T in Ts]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert lib.epsm_scene_topology_bytes(1000, 10) < lib.epsm_scene_topology_bytes(2000, 10)
    assert lib.epsm_emitter_tables_bytes(1000, 1) < lib.epsm_emitter_tables_bytes(1000, 1000)
    assert lib.epsm_scene_topology_bytes(3 * 10 ** 6, 10 ** 6) >= 4 * (3 * 10 ** 6 + 1 + 3 * 10 ** 6)
    env = [lib.epsm_environment_tables_bytes(w, h) for w, h in ((2, 2), (8, 4), (64, 32), (1024, 512), (4096, 2048))]
    assert env[0] > 0 and all(a <= b for a, b in zip(env, env[1:])), env


def _topology(lib, V=300, T=100, tri=FAKE, top=FAKE, top_bytes=None, ws=FAKE, ws_bytes=None):
    top_bytes = lib.epsm_scene_topology_bytes(max(V, 1), max(T, 1)) if top_bytes is None else top_bytes
    ws_bytes = lib.epsm_scene_topology_workspace_bytes(max(T, 1)) if ws_bytes is None else ws_bytes
    return lib.epsm_scene_topology(tri, V, T, top, top_bytes, ws, ws_bytes, None)


@pytest.mark.parametrize("case,kw,msg", [
    ("T < 1", dict(T=0), b"T must be"),
    ("T negative", dict(T=-3), b"T must be"),
    ("T >= 2^28", dict(T=1 << 28, ws_bytes=1 << 62, top_bytes=1 << 62), b"2^28"),
    ("V < 1", dict(V=0), b"V must be"),
    ("V negative", dict(V=-1), b"V must be"),
    ("tri NULL", dict(tri=None), b"NULL"),
    ("topology NULL", dict(top=None), b"NULL"),
    ("workspace NULL", dict(ws=None), b"NULL"),
    ("topology too small", dict(top_bytes=64), b"topology smaller"),
    ("workspace too small", dict(ws_bytes=64), b"workspace smaller"),
    ("topology misaligned", dict(top=FAKE + 4), b"aligned"),
])
def test_topology_refuses_invalid_arguments(lib, case, kw, msg):
    _refused(lib, _topology(lib, **kw), msg, case)


def test_topology_refuses_a_buffer_one_byte_short(lib):
    _refused(lib, _topology(lib, V=5000, T=1000, top_bytes=lib.epsm_scene_topology_bytes(5000, 1000) - 1), b"topology", "short")
    _refused(lib, _topology(lib, V=5000, T=1000, ws_bytes=lib.epsm_scene_topology_workspace_bytes(1000) - 1), b"workspace", "short")


def _normals(lib, V=300, T=100, pos=FAKE, tri=FAKE, top=FAKE, meshes=True, ranges=((0, 60, 0), (60, 40, 60)), vb=(0, 150, 300),
             n=None, nrm=FAKE):
    m = _meshes(ranges) if meshes else None
    vba = (C.c_int64 * len(vb))(*vb) if vb is not None else None
    return lib.epsm_vertex_normals(pos, V, tri, T, top, m, vba, len(ranges) if n is None else n, nrm, None)


@pytest.mark.parametrize("case,kw,msg", [
    ("T < 1", dict(T=0), b"T must be"),
    ("V < 1", dict(V=0), b"V must be"),
    ("n_meshes negative", dict(n=-1), b"n_meshes"),
    ("positions NULL", dict(pos=None), b"NULL"),
    ("tri NULL", dict(tri=None), b"NULL"),
    ("topology NULL", dict(top=None), b"NULL"),
    ("normals NULL", dict(nrm=None), b"NULL"),
    ("meshes NULL", dict(meshes=False), b"NULL"),
    ("vertex_begin NULL", dict(vb=None), b"NULL"),
    ("mesh beyond T", dict(ranges=((0, 60, 0), (60, 41, 60))), b"beyond T"),
    ("meshes overlap", dict(ranges=((0, 60, 0), (30, 60, 60))), b"overlap"),
    ("meshes overlap, counts fit", dict(ranges=((0, 10, 0), (5, 10, 10))), b"overlap"),
    ("vertex range beyond V", dict(vb=(0, 150, 301)), b"vertex_begin"),
    ("vertex ranges decrease", dict(vb=(0, 200, 150)), b"vertex_begin"),
    ("vertex range negative", dict(vb=(-1, 150, 300)), b"vertex_begin"),
])
def test_vertex_normals_refuse_invalid_arguments(lib, case, kw, msg):
    _refused(lib, _normals(lib, **kw), msg, case)


def _emitter(lib, V=300, T=100, pos=FAKE, tri=FAKE, meshes=True, dev=FAKE, ranges=((0, 60, 0), (60, 40, 60)), n=None, cdf=FAKE,
             cdf_len=100, ws=FAKE, ws_bytes=None):
    n = len(ranges) if n is None else n
    ws_bytes = lib.epsm_emitter_tables_bytes(max(T, 1), max(n, 1)) if ws_bytes is None else ws_bytes
    return lib.epsm_emitter_tables(pos, V, tri, T, _meshes(ranges) if meshes else None, dev, n, cdf, cdf_len, ws, ws_bytes, None)


@pytest.mark.parametrize("case,kw,msg", [
    ("T < 1", dict(T=0), b"T must be"),
    ("T >= 2^28", dict(T=1 << 28, ws_bytes=1 << 62), b"2^28"),
    ("V < 1", dict(V=0), b"V must be"),
    ("n_meshes negative", dict(n=-2), b"n_meshes"),
    ("cdf_len negative", dict(cdf_len=-1), b"cdf_len"),
    ("positions NULL", dict(pos=None), b"NULL"),
    ("tri NULL", dict(tri=None), b"NULL"),
    ("meshes NULL", dict(meshes=False), b"NULL"),
    ("device meshes NULL", dict(dev=None), b"NULL"),
    ("emitter_cdf NULL", dict(cdf=None), b"NULL"),
    ("workspace NULL", dict(ws=None), b"NULL"),
    ("workspace too small", dict(ws_bytes=64), b"workspace"),
    ("workspace misaligned", dict(ws=FAKE + 8), b"aligned"),
    ("mesh beyond T", dict(ranges=((0, 60, 0), (61, 40, 60))), b"beyond T"),
    ("meshes overlap", dict(ranges=((0, 60, 0), (30, 60, 60))), b"overlap"),
    ("CDF beyond cdf_len", dict(ranges=((0, 60, 0), (60, 40, 61))), b"cdf_len"),
    ("meshes overlap, counts fit", dict(ranges=((0, 10, 0), (5, 10, 20))), b"overlap"),
    ("CDF ranges overlap", dict(ranges=((0, 60, 0), (60, 40, 30))), b"CDF ranges overlap"),
])
def test_emitter_tables_refuse_invalid_arguments(lib, case, kw, msg):
    _refused(lib, _emitter(lib, **kw), msg, case)


def test_emitter_tables_refuse_a_workspace_one_byte_short(lib):
    _refused(lib, _emitter(lib, T=5000, V=9000, ranges=((0, 5000, 0),), cdf_len=5000,
                           ws_bytes=lib.epsm_emitter_tables_bytes(5000, 1) - 1), b"workspace", "short")


def _env(lib, W=16, H=8, bm=FAKE, tex=FAKE, row=FAKE, col=FAKE, pdf=FAKE, ws=FAKE, ws_bytes=None):
    ws_bytes = lib.epsm_environment_tables_bytes(max(W, 2), max(H, 2)) if ws_bytes is None else ws_bytes
    return lib.epsm_environment_tables(bm, W, H, tex, row, col, pdf, ws, ws_bytes, None)


@pytest.mark.parametrize("case,kw,msg", [
    ("width < 2", dict(W=1), b"width and height"),
    ("height < 2", dict(H=1), b"width and height"),
    ("width negative", dict(W=-4), b"width and height"),
    ("too many texels", dict(W=1 << 14, H=1 << 13, ws_bytes=1 << 62), b"2^26"),
    ("bitmap NULL", dict(bm=None), b"NULL"),
    ("texels NULL", dict(tex=None), b"NULL"),
    ("row_cdf NULL", dict(row=None), b"NULL"),
    ("col_cdf NULL", dict(col=None), b"NULL"),
    ("cell_pdf NULL", dict(pdf=None), b"NULL"),
    ("workspace NULL", dict(ws=None), b"NULL"),
    ("workspace too small", dict(ws_bytes=64), b"workspace"),
    ("workspace misaligned", dict(ws=FAKE + 8), b"aligned"),
])
def test_environment_tables_refuse_invalid_arguments(lib, case, kw, msg):
    _refused(lib, _env(lib, **kw), msg, case)


def test_environment_tables_refuse_a_workspace_one_byte_short(lib):
    _refused(lib, _env(lib, W=512, H=256, ws_bytes=lib.epsm_environment_tables_bytes(512, 256) - 1), b"workspace", "short")


def test_nothing_to_do_is_not_an_error(lib):
    """No mesh in the table: both per-mesh entries return 0 without a launch (so also without a device)."""
    assert _normals(lib, ranges=(), vb=(0,), n=0) == 0
    assert _emitter(lib, ranges=(), n=0) == 0


def test_scene_keyword_is_checked():
    from epsm_mitsuba3_amd import scene as S
    with pytest.raises(ValueError, match="scene_tables"):
        S.Scene([], [], [], [], device="cpu", scene_tables="gpu")
