"""Stage 2 of the reparameterised passes on the DEVICE, request by request: the production kernels epsm_reparam_warp_kernel<G> and
epsm_reparam_fwd_warp_kernel<G> (csrc/epsm_trace_reparam.hip), run alone on hand-written requests through
epsm_probe_reparam_warps, against the float64 restatement of tests/_warp_oracle.py.  The assertions are those of
tests/test_warp_stage.py (the host twin), shared through tests/_warp_stage.py: its docstring has the fixture, the conditions on it
and the tolerance rule (tol = 8 e32 of the reference's own float32 run, floor 32 u, asserted <= 1e-3), MEASUREMENTS.md 29 the
measured e32, tol and device errors per case.  Beyond the host file: the transpose identity on the device and host twin against
device."""
import numpy as np
import pytest

import _warp_oracle as O
import _warp_stage as WS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    return WS.Runner("cuda")


@pytest.fixture(scope="module")
def host():
    return WS.Runner("cpu")


@pytest.mark.parametrize("rays,kappa,antithetic", WS.CASES, ids=WS.CASE_IDS)
def test_forward_stage_per_request(run, rays, kappa, antithetic):
    K = WS.case(rays, kappa, antithetic)
    WS.check_fixture(K)
    WS.check_forward(run, K, "device")


@pytest.mark.parametrize("rays,kappa,antithetic", WS.CASES, ids=WS.CASE_IDS)
def test_backward_stage_per_vertex_row(run, rays, kappa, antithetic):
    K = WS.case(rays, kappa, antithetic)
    WS.check_backward(run, K, "device")
    WS.check_backward_alone(run, K, "device")


@pytest.mark.parametrize("rays,kappa,antithetic", WS.CASES, ids=WS.CASE_IDS)
def test_forward_stage_is_the_transpose_of_the_backward_stage(run, rays, kappa, antithetic):
    WS.check_transpose(run, WS.case(rays, kappa, antithetic), "device")


@pytest.mark.parametrize("rays,kappa,antithetic", WS.CASES, ids=WS.CASE_IDS)
def test_host_twin_agrees_with_the_device(run, host, rays, kappa, antithetic):
    """On decided requests the forward outputs of the two builds agree within 2 tol A (each is within tol A of the reference).  The
    host twin's own error is printed, never used for a bound."""
    K = WS.case(rays, kappa, antithetic)
    words = O.pack_workspace(WS.N_PATHS, K.req, K.count)
    dev = WS.forward_outputs(K, run.forward(K.cfg, WS.N_PATHS, words, K.tan))
    hst = WS.forward_outputs(K, host.forward(K.cfg, WS.N_PATHS, words, K.tan))
    dec = K.decided
    for a, b, ref, A, what in ((dev[0], hst[0], K.fwd64[0], K.fwd64[2], "d'"), (dev[1], hst[1], K.fwd64[1], K.fwd64[3], "div'")):
        print(f"{what}: host twin {WS._units(b[dec], ref[dec], A[dec]):.3g} A, device {WS._units(a[dec], ref[dec], A[dec]):.3g} A from the reference")
        WS._worst(a[dec], b[dec].astype(np.float64), A[dec], 2 * K.tol_fwd)
