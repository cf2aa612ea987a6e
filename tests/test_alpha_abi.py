"""The C ABI of the roughness adjoint: the symbols and the ABI version of the product library (no GPU needed to look them up),
and the argument refusals of the entry points, on the host twin and -- marked gpu -- on the device library."""
import ctypes as C
import os

import pytest
import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd import _lib
from test_alpha_adjoint import attach_two, two_plate_scene

SYMBOLS = ["epsm_trace_paths_bsdf_backward", "epsm_trace_paths_bsdf_forward", "epsm_trace_bsdf_workspace_bytes"]


def test_product_library_exports_the_entry_points_and_keeps_abi_7():
    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.epsm_abi_version() == _lib.ABI_VERSION == 7
    lib.epsm_trace_bsdf_workspace_bytes.restype = C.c_size_t
    assert lib.epsm_trace_bsdf_workspace_bytes(C.c_int64(0)) == 0
    assert lib.epsm_trace_bsdf_workspace_bytes(C.c_int64(129)) == 2 * 8 * 4      # one row of EPSM_MAX_ALPHA_GRADS floats per 128 paths


def test_header_declares_them():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "epsm_trace.h")).read()
    from epsm_mitsuba3_amd import scene as S
    for name in SYMBOLS + [f"EPSM_MAX_ALPHA_GRADS {S.MAX_ALPHA_GRADS}", "EPSM_PROBE_MICROFACET_DALPHA = 11", "EPSM_PROBE_BSDF_DALPHA = 12"]:
        assert name in text, name


def _refusals(sc, lib, stream=None):
    n = 64
    dev = sc.device
    z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)
    rad, adj, grad, work, out = z(n, 3), z(n, 3), z(2), z(64), z(n, 3)
    cs = sc.sensors[0].c_struct()
    head = lambda N=n, spp=4: [C.byref(sc.c_scene), C.byref(cs), C.c_uint32(1), spp, 2, 5, C.c_int64(0), C.c_int64(N)]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    bwd = lambda h, r=rad, a=adj, g=grad, B=2, w=work, wb=256: lib.epsm_trace_paths_bsdf_backward(
        *h, p(r), p(a), p(g), B, p(w), C.c_size_t(wb), stream)
    fwd = lambda h, r=rad, t=grad, B=2, o=out: lib.epsm_trace_paths_bsdf_forward(*h, p(r), p(t), B, p(o), stream)
    assert bwd(head()) == 0 and fwd(head()) == 0
    assert bwd(head(), B=9) == -22 and fwd(head(), B=9) == -22                      # more than EPSM_MAX_ALPHA_GRADS
    assert bwd(head(), B=-1) == -22
    assert bwd(head(), r=None) == -22 and bwd(head(), a=None) == -22 and bwd(head(), g=None) == -22
    assert bwd(head(), w=None) == -22 and bwd(head(), wb=8) == -22                  # no or too small a workspace
    assert fwd(head(), r=None) == -22 and fwd(head(), t=None) == -22 and fwd(head(), o=None) == -22
    assert bwd(head(spp=0)) == -22 and bwd(head(N=-1)) == -22 and bwd(head(N=10 ** 9)) == -22      # beyond the sensor's paths
    assert bwd(head(N=0)) == 0 and fwd(head(N=0)) == 0
    assert bwd([None] + head()[1:]) == -22 and fwd([head()[0], None] + head()[2:]) == -22


def test_refusals_on_the_host_twin():
    sc = two_plate_scene()
    attach_two(sc)
    _refusals(sc, sc._backend)


@pytest.mark.gpu
def test_refusals_on_the_device():
    sc = two_plate_scene("cuda")
    attach_two(sc)
    lib, stream = sc._runtime()
    _refusals(sc, lib, C.c_void_p(stream))
    torch.cuda.synchronize()


def test_scene_refuses_a_tracer_without_the_entry_points():
    """A missing kernel is an error, not a fall-back: a backend that lacks the roughness adjoint cannot serve an attached alpha."""
    from _scenes import on_host
    sc = on_host(two_plate_scene())
    attach_two(sc)
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    with pytest.raises(AttributeError, match="epsm_trace"):
        integ.render_backward(sc, sc.param_grads(), torch.ones((12, 12, 3)), seed=1, spp=4)
