"""Times the roughness-map replays (epsm_trace_paths_alpha_texture_backward / _forward) on one 2^22-path tile (64 x 64 pixels x
1024 samples, depth 3) of exp/roughness_map.py's plate, with the roughness replay (epsm_trace_paths_bsdf_backward) of the same
plate under a scalar alpha beside them (MEASUREMENTS 17).  Two maps bracket the merge branch: the experiment's 8 x 8 `nearest`
map -- a pixel is a fraction of a texel, so every wave (64 samples of one pixel) shares footprints -- and a 1024 x 1024 map
repeated 8 times across the plate -- a pixel spans some hundred texels each way, so next to no two adjacent lanes meet.  Device
events around each call, best of `reps` after one warm-up."""
import json
import sys

import numpy as np
import torch

from epsm_mitsuba3_amd.exp import roughness_map as exp
from epsm_mitsuba3_amd.scene import Scene, look_at


def best(fn, reps=5):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return min(out)


def plate(alpha, uv_scale=1.0, res=64):
    """exp/roughness_map.py's plate, light and sky with `alpha` (a scalar or a bitmap dict) and a res x res film."""
    pv = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], float)
    pf = np.array([[0, 1, 2], [0, 2, 3]])
    uv = uv_scale * np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    lv = np.array([[-1.6, 0.3, 2.5], [1.6, 0.3, 2.5], [1.6, 3.4, 2.5], [-1.6, 3.4, 2.5]], float)
    cam = {"type": "perspective", "fov": 45, "near_clip": 0.01, "far_clip": 100.0, "to_world": look_at([0.0, -1.5, 2.0], [0, 0, 0], [0, 0, 1]),
           "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "gaussian"}},
           "sampler": {"type": "independent", "sample_count": 1024}}
    d = {"type": "scene", "cam": cam,
         "plate": {"type": "mesh", "vertices": pv, "faces": pf, "texcoords": uv, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": alpha, "sample_visible": False}},
         "light": {"type": "mesh", "vertices": lv, "faces": pf[:, ::-1], "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 6.0}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.2}}}
    sc = Scene.from_dict(d, device="cuda")
    sc.tracer = "mega"
    return sc


def main():
    depth, seed, spp, n = 3, 3, 1024, 1 << 22
    res = {"paths": n, "depth": depth}
    adj = torch.randn((n, 3), device="cuda")
    sc = plate(exp.ALPHA_START)
    sc.attach_alpha("plate.bsdf")
    assert sc.sensors[0].wavefront_size(spp) == n
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, 0, n)
    radiance = radiance.contiguous()
    grad, tan = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    res["trace_color_ms"] = best(lambda: sc.trace_color(0, seed, spp, depth, 0, n))
    res["scalar_alpha_backward_ms"] = best(lambda: sc.trace_alpha_backward(0, seed, spp, depth, 0, n, radiance, adj, grad))
    res["scalar_alpha_forward_ms"] = best(lambda: sc.trace_alpha_forward(0, seed, spp, depth, 0, n, radiance, tan))
    big = (exp.ALPHA_START + 0.1 * np.random.default_rng(0).random((1024, 1024))).astype(np.float32)
    for name, values, scale, nearest in (("map8_nearest", np.full((8, 8), exp.ALPHA_START, np.float32), 1.0, True),
                                         ("map8_bilinear", np.full((8, 8), exp.ALPHA_START, np.float32), 1.0, False),
                                         ("map1024x8_nearest", big, 8.0, True)):
        m = plate({"type": "bitmap", "bitmap": values, "filter_type": "nearest" if nearest else "bilinear"}, scale)
        m.attach_texture("plate.bsdf.alpha.data")
        _, rad, _ = m.trace_color(0, seed, spp, depth, 0, n)
        rad = rad.contiguous()
        bufs = [torch.zeros(values.shape, device="cuda")]
        tans = [torch.randn(values.shape, device="cuda")]
        res[name + "_trace_color_ms"] = best(lambda: m.trace_color(0, seed, spp, depth, 0, n))
        res[name + "_backward_ms"] = best(lambda: m.trace_alpha_texture_backward(0, seed, spp, depth, 0, n, rad, adj, bufs))
        res[name + "_forward_ms"] = best(lambda: m.trace_alpha_texture_forward(0, seed, spp, depth, 0, n, rad, tans))
        res[name + "_texels_touched"] = int((bufs[0] != 0).sum())
    print(json.dumps(res))
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
