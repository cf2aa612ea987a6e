"""Time of the texel adjoint's replay (epsm_trace_paths_texture_backward / _forward) for one tile of 2^22 paths (256 x 256 @ 64
spp, max_depth 4) against epsm_trace_paths_color on the same tile, on three scenes: a 1024^2 floor texture, a 4 x 4 floor texture
(every lane of a wave on one footprint: the worst contention), a 512 x 256 envmap.
    python tools/time_texture_adjoint.py [REPEATS] [SCENE ...]
Prints one line per scene and pass (median ms of REPEATS launches after one warm-up)."""
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from epsm_mitsuba3_amd.scene import Scene, look_at

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
RES, SPP, DEPTH = 256, 64, 4


def scene(kind):
    rng = np.random.default_rng(0)
    fv = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], float)
    ff = np.array([[0, 1, 2], [0, 2, 3]])
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    n = {"tex1024": 1024, "tex4": 4}.get(kind)
    refl = ({"type": "bitmap", "bitmap": (0.2 + 0.6 * rng.random((n, n, 3))).astype(np.float32)} if n
            else {"type": "rgb", "value": [0.5, 0.5, 0.5]})
    d = {"type": "scene",
         "cam": {"type": "perspective", "fov": 50, "to_world": look_at([0, -3.5, 1.6], [0, 0.5, 0.3], [0, 0, 1]),
                 "film": {"type": "hdrfilm", "width": RES, "height": RES, "rfilter": {"type": "gaussian"}},
                 "sampler": {"type": "independent", "sample_count": SPP}},
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "texcoords": uv, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": refl}}}
    if kind == "env512x256":
        d["sky"] = {"type": "envmap", "bitmap": (0.2 + rng.random((256, 512, 3))).astype(np.float32)}
    else:
        lv = np.array([[-0.4, -0.4, 2.2], [0.4, -0.4, 2.2], [0.4, 0.4, 2.2], [-0.4, 0.4, 2.2]], float)
        d["light"] = {"type": "mesh", "vertices": lv, "faces": ff[:, ::-1], "face_normals": True,
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 20.0}}}
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": 0.2}}
    sc = Scene.from_dict(d, device="cuda")
    sc.tracer = "mega"
    sc.attach_texture("sky" if kind == "env512x256" else "floor.bsdf")
    return sc


def median_ms(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


for kind in sys.argv[2:] or ["tex1024", "tex4", "env512x256"]:
    sc = scene(kind)
    n = sc.sensors[0].wavefront_size(SPP)
    _, radiance, _ = sc.trace_color(0, 1, SPP, DEPTH, 0, n)
    radiance = radiance.contiguous()
    adj = torch.randn((n, 3), device="cuda") * 1e-3
    grads = [torch.zeros((h, w, 3), device="cuda") for h, w in sc.texture_shapes()]
    tans = [torch.randn((h, w, 3), device="cuda") for h, w in sc.texture_shapes()]
    tc = median_ms(lambda: sc.trace_color(0, 1, SPP, DEPTH, 0, n))
    tb = median_ms(lambda: sc.trace_texture_backward(0, 1, SPP, DEPTH, 0, n, radiance, adj, grads))
    tf = median_ms(lambda: sc.trace_texture_forward(0, 1, SPP, DEPTH, 0, n, radiance, tans))
    print(f"{kind}: {n} paths, max_depth {DEPTH}: trace_color {tc:.2f} ms, texture backward {tb:.2f} ms "
          f"({tb / tc:.2f}x), texture forward {tf:.2f} ms ({tf / tc:.2f}x)", flush=True)
