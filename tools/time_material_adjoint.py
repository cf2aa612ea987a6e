"""Times the conductor material replays (epsm_trace_paths_material_backward / _forward) on one tile of exp/metal.py at depth 4
(64 x 64 pixels x 1024 samples), the roughness replays of the same BSDF on the same tile beside them, and the primal
epsm_trace_paths_color (MEASUREMENTS 16).  Device events around each call, best of `reps` after one warm-up."""
import json
import sys

import torch

from epsm_mitsuba3_amd.exp import metal


def best(fn, reps=5):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return min(out)


def main():
    depth, seed, spp = 4, 3, 1024
    res = {}
    sc = metal.load_scene("cuda")
    sc.attach_alpha("plate.bsdf")
    sc.attach_conductor("plate.bsdf")
    n = sc.sensors[0].wavefront_size(spp)
    res["paths"] = n
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, 0, n)
    radiance = radiance.contiguous()
    adj = torch.randn((n, 3), device="cuda")
    grad_a, tan_a = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    grad_m, tan_m = torch.zeros((1, 3, 3), device="cuda"), torch.ones((1, 3, 3), device="cuda")
    res["trace_color_ms"] = best(lambda: sc.trace_color(0, seed, spp, depth, 0, n))
    res["alpha_backward_ms"] = best(lambda: sc.trace_alpha_backward(0, seed, spp, depth, 0, n, radiance, adj, grad_a))
    res["alpha_forward_ms"] = best(lambda: sc.trace_alpha_forward(0, seed, spp, depth, 0, n, radiance, tan_a))
    res["material_backward_ms"] = best(lambda: sc.trace_material_backward(0, seed, spp, depth, 0, n, radiance, adj, grad_m))
    res["material_forward_ms"] = best(lambda: sc.trace_material_forward(0, seed, spp, depth, 0, n, radiance, tan_m))
    print(json.dumps(res))
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
