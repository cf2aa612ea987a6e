"""The arguments every replay entry point of the tracer starts with -- scene, sensor, seed, spp, max_depth, rr_depth, path_offset,
N -- are checked by one function (csrc/epsm_trace_replay.h, replay_args_fill): one table of calls over the six replay entry points
and epsm_trace_paths_color, on the host twins and -- marked gpu -- on the device library.  Every refused call is refused by that
check, before anything is launched."""
import ctypes as C

import pytest
import torch

from _bsdf_host import on_host_bsdf
from _reparam_scenes import build as build_reparam
from test_alpha_adjoint import attach_two, two_plate_scene
from test_texture_adjoint import texture_scene

RES, SPP, N = 12, 4, 64
ENTRY_POINTS = ["epsm_trace_paths_color", "epsm_trace_paths_texture_backward", "epsm_trace_paths_texture_forward",
                "epsm_trace_paths_bsdf_backward", "epsm_trace_paths_bsdf_forward", "epsm_trace_paths_reparam",
                "epsm_trace_paths_reparam_forward"]


def _two_plates(device):
    sc = two_plate_scene(device, res=RES, spp=SPP)
    attach_two(sc)
    return sc


def _textured(device):
    sc = texture_scene(device, res=RES, spp=SPP)
    sc.attach_texture("floor.bsdf")
    return sc


def _smallest_reparam(device):
    return build_reparam("rectangle_emitter_on_black", res=RES, spp=SPP, device=device)


SCENES = {"two_plates": _two_plates, "textured": _textured, "reparam": _smallest_reparam}


def _tails(sc, lib):
    """Per entry point, the arguments behind the common eight (valid ones), the stream left out."""
    dev = sc.device
    z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)
    p = lambda t: C.c_void_p(t.data_ptr())
    B = len(sc.alpha_slots)
    rad, adj, film, out, out2 = z(N, 3), z(N, 3), z(N, 3), z(N, 3), z(N, 3)
    pos2, valid, sums = z(N, 2), torch.zeros(N, device=dev, dtype=torch.uint8), z(N, 1, 3)
    alpha, work = z(max(B, 1)), z(64)
    texels = [z(*sc._texture_shape(k)) for k in range(len(sc.texture_slots))]
    arr, env = sc._texture_pointers(texels)
    vpos, vnrm = z(sc.V, 3), z(sc.V, 3)
    lib.epsm_trace_reparam_workspace_bytes.restype = C.c_size_t
    ws = torch.zeros(max(int(lib.epsm_trace_reparam_workspace_bytes(C.c_int64(N))), 16), device=dev, dtype=torch.uint8)
    reparam = [1, 4, C.c_float(1e5), C.c_float(3.0), C.c_uint32(0)]        # reparam_max_depth, rays, kappa, exponent, flags
    keep = [rad, adj, film, out, out2, pos2, valid, sums, alpha, work, texels, arr, vpos, vnrm, ws]
    return keep, {
        "epsm_trace_paths_color": [p(pos2), p(rad), p(valid), p(sums), 1],
        "epsm_trace_paths_texture_backward": [p(rad), p(adj), arr, env],
        "epsm_trace_paths_texture_forward": [p(rad), arr, env, p(out)],
        "epsm_trace_paths_bsdf_backward": [p(rad), p(adj), p(alpha), B, p(work), C.c_size_t(256)],
        "epsm_trace_paths_bsdf_forward": [p(rad), p(alpha), B, p(out)],
        "epsm_trace_paths_reparam": [p(rad), p(adj), p(film)] + reparam + [p(vpos), p(vnrm), p(ws), C.c_size_t(ws.numel())],
        "epsm_trace_paths_reparam_forward": [p(rad), p(vpos), p(vnrm)] + reparam + [p(out), p(out2), p(ws), C.c_size_t(ws.numel())],
    }


def _table(sc, lib, stream=None, last_error=None):
    cs = sc.sensors[0].c_struct()
    keep, tails = _tails(sc, lib)

    def head(scene=True, sensor=True, spp=SPP, rr_depth=5, offset=0, n=N):
        return [C.byref(sc.c_scene) if scene else None, C.byref(cs) if sensor else None, C.c_uint32(1), spp, 2, rr_depth,
                C.c_int64(offset), C.c_int64(n)]

    refused = {"NULL scene": dict(scene=False), "NULL sensor": dict(sensor=False), "spp = 0": dict(spp=0), "N = -1": dict(n=-1),
               "path_offset = -1": dict(offset=-1), "N = 10**9": dict(n=10 ** 9), "rr_depth = 0": dict(rr_depth=0)}
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        fn.restype = C.c_int
        call = lambda **kw: fn(*head(**kw), *tails[name], stream)
        assert call() == 0, name
        assert call(n=0) == 0, name
        for what, kw in refused.items():
            assert call(**kw) == -22, (name, what)
            if last_error is not None:
                assert last_error().startswith(name + ": "), (name, what, last_error())
    del keep


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_common_arguments_on_the_host_twins(scene):
    sc = on_host_bsdf(SCENES[scene]("cpu"))                  # (the host library that holds all seven entry points)
    _table(sc, sc._backend)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_common_arguments_on_the_device(scene):
    sc = SCENES[scene]("cuda")
    lib, stream = sc._runtime()
    lib.epsm_last_error.restype = C.c_char_p
    _table(sc, lib, C.c_void_p(stream), last_error=lambda: lib.epsm_last_error().decode())
    torch.cuda.synchronize()
