"""Stage 2 of the reparameterised passes, request by request, on the HOST TWIN of epsm_probe_reparam_warps
(tests/host_harness/trace_host.cpp: warp_collect + warp_backward / warp_forward per live request) against the float64
restatement of tests/_warp_oracle.py -- the assertions tests/test_gpu_warp_stage.py makes of the device kernels, shared through
tests/_warp_stage.py (fixture, conditions on it and the tolerance rule: its docstring; measured e32 / tol: MEASUREMENTS.md 29)."""
import ctypes as C

import numpy as np
import pytest

import _warp_oracle as O
import _warp_stage as WS
from _refvec import Pcg32Py, check_tea_python


@pytest.fixture(scope="module")
def run():
    return WS.Runner("cpu")


def test_the_oracle_draws_from_the_pinned_streams():
    """tea against the reference's vectors, the side-by-side PCG32 against the python-int one of tests/_refvec.py."""
    check_tea_python(lambda a, b: tuple(int(x[0]) for x in O.tea(np.array([a]), np.array([b]))))
    seeds = [(1, 2), (0xDEADBEEF, 0x1234567), (0xFFFFFFFF, 0)]
    rng = O.Pcg32Vec(np.array([s for s, _ in seeds], dtype=np.uint64), np.array([q for _, q in seeds], dtype=np.uint64))
    ref = [Pcg32Py(s, q) for s, q in seeds]
    for _ in range(4):
        assert [float(x) for x in rng.next_1d()] == [p.next_f32() for p in ref]


@pytest.mark.parametrize("rays,kappa,antithetic", WS.CASES, ids=WS.CASE_IDS)
def test_fixture_conditions_hold_by_the_reference_alone(rays, kappa, antithetic):
    WS.check_fixture(WS.case(rays, kappa, antithetic))


@pytest.mark.parametrize("rays,kappa,antithetic", WS.CASES, ids=WS.CASE_IDS)
def test_forward_stage_per_request(run, rays, kappa, antithetic):
    WS.check_forward(run, WS.case(rays, kappa, antithetic), "host twin")


@pytest.mark.parametrize("rays,kappa,antithetic", WS.CASES, ids=WS.CASE_IDS)
def test_backward_stage_per_vertex_row(run, rays, kappa, antithetic):
    K = WS.case(rays, kappa, antithetic)
    WS.check_backward(run, K, "host twin")
    WS.check_backward_alone(run, K, "host twin")


def _refusals(lib, scene_struct, good):
    """the return codes of the calls section `EPSM_EINVAL` of the entry point's comment lists, in a fixed order"""
    def call(**kw):
        a = dict(good, **kw)
        return int(lib.epsm_probe_reparam_warps(a["scene"], C.c_uint32(7), C.c_int64(a["offset"]), C.c_int64(a["n"]), a["depth"], a["rays"],
                                                C.c_float(a["kappa"]), C.c_float(a["exponent"]), C.c_uint32(a["flags"]), a["forward"],
                                                C.c_void_p(a["grad"]), C.c_void_p(a["tan"]), C.c_void_p(a["ws"]), C.c_size_t(a["bytes"]), None))
    codes = [call(n=0, grad=None, tan=None, ws=None, bytes=0),               # N = 0: fine, nothing is touched
             call(scene=None), call(n=-1), call(depth=0), call(offset=-1), call(offset=2 ** 32 - 2),
             call(grad=None), call(forward=1, tan=None), call(ws=None), call(bytes=good["bytes"] - 1), call(ws=good["ws"] + 4),
             call(rays=0), call(rays=65), call(kappa=0.0), call(exponent=-1.0), call(flags=2)]
    empty = type(scene_struct)()
    codes.append(call(scene=C.addressof(empty)))                            # a scene without triangles
    return codes


def test_both_builds_refuse_alike_before_anything_is_touched(run):
    """The product library (no device is touched: every call is refused before a launch, or N = 0) and the host twin return the
    same codes for the same bad calls."""
    from epsm_mitsuba3_amd import _lib
    n = 3
    ws = np.zeros(O.workspace_bytes(n) // 4 + 8, dtype=np.int32)              # counts 0: the one good call has nothing to do
    base = ws.ctypes.data + (-ws.ctypes.data) % 16
    rows = np.zeros((run.sc.V, 3), dtype=np.float32)
    good = dict(scene=C.addressof(run.sc.c_scene), offset=0, n=n, depth=3, rays=16, kappa=1e3, exponent=3.0, flags=1, forward=0,
                grad=rows.ctypes.data, tan=rows.ctypes.data, ws=base, bytes=O.workspace_bytes(n))
    host = _refusals(run.sc._backend, run.sc.c_scene, good)
    device = _refusals(_lib.lib(), run.sc.c_scene, good)
    assert host == device == [0] + [-22] * 16, (host, device)
    assert b"epsm_probe_reparam_warps" in _lib.lib().epsm_last_error()
    lib = run.sc._backend                                                  # the good call itself, on the host twin: counts 0, nothing written
    assert lib.epsm_probe_reparam_warps(good["scene"], C.c_uint32(7), C.c_int64(0), C.c_int64(n), 3, 16, C.c_float(1e3), C.c_float(3.0),
                                        C.c_uint32(1), 0, C.c_void_p(good["grad"]), None, C.c_void_p(base), C.c_size_t(good["bytes"]), None) == 0
    assert not rows.any() and not ws.any()
