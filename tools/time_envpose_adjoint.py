"""Times the envmap pose replays (epsm_trace_paths_envpose_backward / _forward) on one tile of exp/lighting.py at depth 3
(32 x 32 pixels x 1024 samples), the conductor material replays of the ball and the texel replays of the envmap on the same tile
beside them, and the primal epsm_trace_paths_color (MEASUREMENTS 28).  Device events around each call, best of `reps` after one
warm-up."""
import json
import sys

import torch

from epsm_mitsuba3_amd.exp import lighting


def best(fn, reps=5):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return min(out)


def main():
    depth, seed, spp = lighting.max_depth, 3, 1024
    res = {}
    sc = lighting.load_scene("cuda")
    sc.attach_envmap_pose()
    sc.attach_conductor("ball.bsdf")
    slot = sc.attach_texture("sky")
    n = sc.sensors[0].wavefront_size(spp)
    res["paths"] = n
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, 0, n)
    radiance = radiance.contiguous()
    adj = torch.randn((n, 3), device="cuda")
    grad_p, tan_p = torch.zeros(4, device="cuda"), torch.ones(4, device="cuda")
    grad_m, tan_m = torch.zeros((1, 3, 3), device="cuda"), torch.ones((1, 3, 3), device="cuda")
    texels = [torch.zeros(sc._texture_shape(slot), device="cuda")]
    res["trace_color_ms"] = best(lambda: sc.trace_color(0, seed, spp, depth, 0, n))
    res["envpose_backward_ms"] = best(lambda: sc.trace_envpose_backward(0, seed, spp, depth, 0, n, radiance, adj, grad_p))
    res["envpose_forward_ms"] = best(lambda: sc.trace_envpose_forward(0, seed, spp, depth, 0, n, radiance, tan_p))
    res["material_backward_ms"] = best(lambda: sc.trace_material_backward(0, seed, spp, depth, 0, n, radiance, adj, grad_m))
    res["material_forward_ms"] = best(lambda: sc.trace_material_forward(0, seed, spp, depth, 0, n, radiance, tan_m))
    res["texture_backward_ms"] = best(lambda: sc.trace_texture_backward(0, seed, spp, depth, 0, n, radiance, adj, texels))
    res["texture_forward_ms"] = best(lambda: sc.trace_texture_forward(0, seed, spp, depth, 0, n, radiance, texels))
    print(json.dumps(res))
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
