"""Times the colour adjoint's replays through their table (epsm_mitsuba3_amd/replays.py):
    python tools/time_color_adjoint.py CONFIG|all [OUT.json]
A configuration is a list of scenes with something attached; on each, one tile is timed: epsm_trace_paths_color
(``<prefix>trace_color_ms``) and both directions of every attached kind (``<prefix><kind>_backward_ms`` / ``_forward_ms``).
Device events around each call, best of five after one warm-up; one JSON object per configuration.  The configurations:
  texture        2^22 paths (256 x 256 @ 64 spp, depth 4): a 1024^2 floor texture, a 4 x 4 one (every lane of a wave on one
                 footprint: the worst contention), a 512 x 256 envmap
  alpha          exp/plate.py's plate under a scalar alpha, 2^22 paths (64 x 64 @ 1024 spp, depth 4); exp/texture.py's texels
                 on a tile of the same size beside it (``texel_``)
  material       exp/metal.py at depth 4 (64 x 64 @ 1024 spp): alpha and conductor material of the same BSDF
  alpha_texture  exp/roughness_map.py's plate, 2^22 paths at depth 3: a scalar alpha (``scalar_alpha_``), the experiment's 8 x 8
                 map `nearest` and `bilinear` (a pixel is a fraction of a texel: every wave shares footprints), a 1024^2 map
                 repeated 8 times across the plate (next to no two adjacent lanes meet)
  envpose        exp/lighting.py at its depth (32 x 32 @ 1024 spp): the envmap's pose, the ball's material, the envmap's texels"""
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from epsm_mitsuba3_amd import replays
from epsm_mitsuba3_amd.scene import Scene, look_at

QUAD_F = np.array([[0, 1, 2], [0, 2, 3]])
UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)


def best(fn, reps=5):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return min(out)


def _film(res, spp):
    return {"film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "gaussian"}},
            "sampler": {"type": "independent", "sample_count": spp}}


def textured_floor(kind):
    """A floor under a light and a constant sky with a `kind` = "tex1024" / "tex4" reflectance bitmap, or ("env512x256") a plain
    floor under an envmap; the bitmap attached."""
    rng = np.random.default_rng(0)
    fv = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], float)
    n = {"tex1024": 1024, "tex4": 4}.get(kind)
    refl = ({"type": "bitmap", "bitmap": (0.2 + 0.6 * rng.random((n, n, 3))).astype(np.float32)} if n
            else {"type": "rgb", "value": [0.5, 0.5, 0.5]})
    d = {"type": "scene",
         "cam": {"type": "perspective", "fov": 50, "to_world": look_at([0, -3.5, 1.6], [0, 0.5, 0.3], [0, 0, 1]), **_film(256, 64)},
         "floor": {"type": "mesh", "vertices": fv, "faces": QUAD_F, "texcoords": UV, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": refl}}}
    if n:
        lv = np.array([[-0.4, -0.4, 2.2], [0.4, -0.4, 2.2], [0.4, 0.4, 2.2], [-0.4, 0.4, 2.2]], float)
        d["light"] = {"type": "mesh", "vertices": lv, "faces": QUAD_F[:, ::-1], "face_normals": True,
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 20.0}}}
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": 0.2}}
    else:
        d["sky"] = {"type": "envmap", "bitmap": (0.2 + rng.random((256, 512, 3))).astype(np.float32)}
    sc = Scene.from_dict(d, device="cuda")
    sc.attach_texture("floor.bsdf" if n else "sky")
    return sc, 4, 1, 64


def rough_plate(alpha, uv_scale=1.0):
    """exp/roughness_map.py's plate, light and sky with `alpha` (a scalar or a bitmap dict) and a 64 x 64 film; it attached."""
    pv = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], float)
    lv = np.array([[-1.6, 0.3, 2.5], [1.6, 0.3, 2.5], [1.6, 3.4, 2.5], [-1.6, 3.4, 2.5]], float)
    d = {"type": "scene",
         "cam": {"type": "perspective", "fov": 45, "near_clip": 0.01, "far_clip": 100.0,
                 "to_world": look_at([0.0, -1.5, 2.0], [0, 0, 0], [0, 0, 1]), **_film(64, 1024)},
         "plate": {"type": "mesh", "vertices": pv, "faces": QUAD_F, "texcoords": uv_scale * UV, "face_normals": True,
                   "bsdf": {"type": "roughconductor", "material": "Al", "distribution": "ggx", "alpha": alpha, "sample_visible": False}},
         "light": {"type": "mesh", "vertices": lv, "faces": QUAD_F[:, ::-1], "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": 6.0}}},
         "sky": {"type": "constant", "radiance": {"type": "rgb", "value": 0.2}}}
    sc = Scene.from_dict(d, device="cuda")
    if isinstance(alpha, dict):
        sc.attach_texture("plate.bsdf.alpha.data")
    else:
        sc.attach_alpha("plate.bsdf")
    return sc, 3, 3, 1024


def alpha_map(values, nearest):
    return {"type": "bitmap", "bitmap": values, "filter_type": "nearest" if nearest else "bilinear"}


def exp_plate():
    from epsm_mitsuba3_amd.exp import plate
    sc = plate.load_scene("cuda")
    sc.set_alpha("plate.bsdf", 0.1)
    sc.attach_alpha("plate.bsdf")
    return sc, 4, 3, 1024


def exp_texture():
    from epsm_mitsuba3_amd.exp import texture
    sc = texture.load_scene("cuda")
    sc.attach_texture("floor.bsdf.reflectance.data")
    return sc, 4, 3, (1 << 22) // texture.resolution ** 2


def exp_metal():
    from epsm_mitsuba3_amd.exp import metal
    sc = metal.load_scene("cuda")
    sc.attach_alpha("plate.bsdf")
    sc.attach_conductor("plate.bsdf")
    return sc, 4, 3, 1024


def exp_lighting():
    from epsm_mitsuba3_amd.exp import lighting
    sc = lighting.load_scene("cuda")
    sc.attach_envmap_pose()
    sc.attach_conductor("ball.bsdf")
    sc.attach_texture("sky")
    return sc, lighting.max_depth, 3, 1024


def _maps():
    from epsm_mitsuba3_amd.exp.roughness_map import ALPHA_START
    small = np.full((8, 8), ALPHA_START, np.float32)
    big = (ALPHA_START + 0.1 * np.random.default_rng(0).random((1024, 1024))).astype(np.float32)
    return [("", lambda: rough_plate(ALPHA_START), {"alpha": "scalar_alpha_"}),
            ("map8_nearest_", lambda: rough_plate(alpha_map(small, True)), {"alpha_texture": ""}),
            ("map8_bilinear_", lambda: rough_plate(alpha_map(small, False)), {"alpha_texture": ""}),
            ("map1024x8_nearest_", lambda: rough_plate(alpha_map(big, True), 8.0), {"alpha_texture": ""})]


# configuration -> its scenes: (key prefix, () -> (scene, depth, seed, spp), {kind: its key stem where not "<kind>_"})
CONFIGS = {"texture": lambda: [(k + "_", lambda k=k: textured_floor(k), {}) for k in ("tex1024", "tex4", "env512x256")],
           "alpha": lambda: [("", exp_plate, {}), ("texel_", exp_texture, {"texture": ""})],
           "material": lambda: [("", exp_metal, {})],
           "alpha_texture": _maps,
           "envpose": lambda: [("", exp_lighting, {})]}


def time_scene(res, prefix, build, stems):
    sc, depth, seed, spp = build()
    sc.tracer = "mega"
    n = sc.sensors[0].wavefront_size(spp)
    res[prefix + "paths"] = n
    _, radiance, _ = sc.trace_color(0, seed, spp, depth, 0, n)
    radiance = radiance.contiguous()
    adj = torch.randn((n, 3), device="cuda")
    res[prefix + "trace_color_ms"] = best(lambda: sc.trace_color(0, seed, spp, depth, 0, n))
    tangent = sc.param_grads()
    tangent.flat.normal_()
    for r in replays.attached(sc):
        key = prefix + stems.get(r.name, r.name + "_")
        grads, tan = r.section.zeros(sc, tangent)[1], r.section.tangent(sc, tangent)
        res[key + "backward_ms"] = best(lambda: sc.replay_backward(r, 0, seed, spp, depth, 0, n, radiance, adj, grads))
        res[key + "forward_ms"] = best(lambda: sc.replay_forward(r, 0, seed, spp, depth, 0, n, radiance, tan))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    out = {}
    for name in (CONFIGS if which == "all" else [which]):
        res = out[name] = {}
        for prefix, build, stems in CONFIGS[name]():
            time_scene(res, prefix, build, stems)
        print(json.dumps({name: res}), flush=True)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
