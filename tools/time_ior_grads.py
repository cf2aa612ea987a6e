"""Launch time of the backward kernel's IOR instantiation (EPSM_OPT_IOR_GRADS = 1) against the default one, on one resident slab
of the headline configuration and of the pool-caustic configuration (bench.py CONFIGS[0] and [3]): native packed log, the
one-launch backward pass, HIP events on the launch stream around ten launches after two warm-up launches, three rounds with the
two settings alternating (MEASUREMENTS.md 32).  A library without the option (EPSM_LIB_NAME names an older build) is timed with
the default instantiation alone.

    python tools/time_ior_grads.py [--default-only]            # one JSON line per (configuration, option)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    import epsm_mitsuba3_amd as epsm
    from epsm_mitsuba3_amd import _lib
    from epsm_mitsuba3_amd.records import PackedLog
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    have = lib.epsm_get_option(_lib.OPT_IOR_GRADS) >= 0 and "--default-only" not in sys.argv      # (--default-only: the protocol an older library gets)
    for index in (0, 3):
        label, variant, profile, res, spp, K, V = bench.CONFIGS[index]
        n = min(res * res * spp, bench.SLAB_PATHS)
        scene = epsm.SyntheticScene(res=res, n_vertices=K, n_scene_vertices=V, n_bsdfs=4, profile=profile, device=dev, tile_paths=n)
        integ = epsm.load_dict({"type": variant, "max_depth": 8})
        trace = scene.tile(0, 0, n, seed=0, spp=spp, K=K, lean=True)
        log = PackedLog.from_trace(trace, device=dev, table=scene.triangle_table(), free=True)
        trace = epsm.PathTrace(res=trace.res, spp=trace.spp, ray_o=None, ray_d=None, ray_dx=None, ray_dy=None, path_info=None,
                               scatter_info=None, path_offset=trace.path_offset, n_paths_total=trace.n_paths_total)
        g = torch.Generator(device=dev).manual_seed(1)
        grad_in = torch.randn((res, res, 5), generator=g, device=dev) * 1e-3
        params = epsm.ParamGrads(V, 4, device=dev)
        times = {0: [], 1: []}
        for _ in range(3):
            for option in ((0, 1) if have else (0,)):
                if have:
                    _lib.check(lib.epsm_set_option(_lib.OPT_IOR_GRADS, option), "epsm_set_option")
                trace.ior_grads = bool(option)          # (backward_from_trace takes the option from the trace)
                try:
                    for _ in range(2):
                        integ.backward_from_trace(trace, params, grad_in, packed=log)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        integ.backward_from_trace(trace, params, grad_in, packed=log)
                    e1.record()
                    torch.cuda.synchronize()
                    times[option].append(e0.elapsed_time(e1) / 10)
                finally:
                    if have:
                        lib.epsm_set_option(_lib.OPT_IOR_GRADS, 0)
        for option, ms in times.items():
            if ms:
                print(json.dumps({"workload": f"{label}: one slab of {n} paths", "library": os.path.basename(_lib.LIB_PATH), "ior_grads": option,
                                  "kernel_ms": [round(x, 4) for x in ms]}), flush=True)
        del log, params, scene


if __name__ == "__main__":
    main()
