"""Times the roughness replays (epsm_trace_paths_bsdf_backward / _forward) on one 2^22-path tile of exp/plate.py at depth 4, the
texel replay on exp/texture.py's tile of the same size beside them, and prb's render_backward on the plate with and without the
alpha slot (MEASUREMENTS 15).  Device events around each call, best of `reps` after one warm-up."""
import json
import sys

import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd.exp import plate, texture


def best(fn, reps=5):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return min(out)


def main():
    depth, seed, spp, n = 4, 3, 1024, 1 << 22                      # 64 x 64 pixels x 1024 samples
    res = {}
    sc = plate.load_scene("cuda"); sc.tracer = "mega"
    sc.set_alpha("plate.bsdf", 0.1)
    sc.attach_alpha("plate.bsdf")
    assert sc.sensors[0].wavefront_size(spp) == n
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, 0, n)
    radiance = radiance.contiguous()
    adj = torch.randn((n, 3), device="cuda")
    grad, tan = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    res["trace_color_ms"] = best(lambda: sc.trace_color(0, seed, spp, depth, 0, n))
    res["alpha_backward_ms"] = best(lambda: sc.trace_alpha_backward(0, seed, spp, depth, 0, n, radiance, adj, grad))
    res["alpha_forward_ms"] = best(lambda: sc.trace_alpha_forward(0, seed, spp, depth, 0, n, radiance, tan))
    integ = epsm.load_dict({"type": "prb", "max_depth": depth})
    g = torch.randn((64, 64, 3), device="cuda")
    sc.attach_radiance("light")
    res["render_backward_with_alpha_ms"] = best(lambda: integ.render_backward(sc, sc.param_grads(), g, seed=seed, spp=256), 3)
    sc2 = plate.load_scene("cuda"); sc2.tracer = "mega"
    sc2.set_alpha("plate.bsdf", 0.1)
    sc2.attach_radiance("light")
    res["render_backward_without_alpha_ms"] = best(lambda: integ.render_backward(sc2, sc2.param_grads(), g, seed=seed, spp=256), 3)
    tx = texture.load_scene("cuda")
    tx.attach_texture("floor.bsdf.reflectance.data")
    spp_t = n // (texture.resolution ** 2)
    nt = tx.sensors[0].wavefront_size(spp_t)
    _, rad_t, _ = tx.trace_color(0, seed, spp_t, depth, 0, nt)
    rad_t = rad_t.contiguous()
    adj_t = torch.randn((nt, 3), device="cuda")
    bufs = [torch.zeros((h, w, 3), device="cuda") for h, w in tx.texture_shapes()]
    res["texel_paths"] = nt
    res["texel_backward_ms"] = best(lambda: tx.trace_texture_backward(0, seed, spp_t, depth, 0, nt, rad_t, adj_t, bufs))
    res["texel_forward_ms"] = best(lambda: tx.trace_texture_forward(0, seed, spp_t, depth, 0, nt, rad_t, bufs))
    res["texel_trace_color_ms"] = best(lambda: tx.trace_color(0, seed, spp_t, depth, 0, nt))
    print(json.dumps(res))
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
