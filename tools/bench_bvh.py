"""The BVH builders side by side on one MI355X; prints ONE JSON line.
  build   host (scene.build_bvh, numpy on one core) against device (epsm_bvh_build) on clutter (128 004 triangles) and on a
          soup of 2^20 triangles of mixed scales
  refit   DeviceBvh.refit (torch gathers) against epsm_bvh_refit, both on the host builder's clutter tree
  sah     SAH cost of both trees (bvh.sah_cost)
  trace   render_backward (manifold) and render_primal on clutter, 512 x 512 @ 16 spp, with each tree (wavefront tracer)
python tools/bench_bvh.py [--reps 7] [--skip-host-soup]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from epsm_mitsuba3_amd import bvh as B
from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd.exp import clutter


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def clutter_geometry():
    d = clutter.scene_dict(n_spheres=100, res=16, spp=1)
    pos, tri, off = [], [], 0
    for v in d.values():
        if isinstance(v, dict) and v.get("type") == "mesh":
            pos.append(np.asarray(v["vertices"], np.float64)); tri.append(np.asarray(v["faces"], np.int64) + off)
            off += pos[-1].shape[0]
    return np.concatenate(pos), np.concatenate(tri)


def soup_geometry(t, seed=7):
    """teapot in a stadium (tests/test_bvh_build.py) at t triangles"""
    rng = np.random.default_rng(seed)
    sizes = 10.0 ** rng.uniform(-5, 1, size=t)
    cl = rng.normal(size=(12, 3)) * 10.0 ** rng.uniform(-2, 2, size=(12, 1))
    centres = cl[rng.integers(0, 12, size=t)] + rng.normal(size=(t, 3)) * 10.0 ** rng.uniform(-4, 1, size=(t, 1))
    pos = (centres[:, None, :] + rng.normal(size=(t, 3, 3)) * sizes[:, None, None]).reshape(-1, 3)
    return pos, np.arange(3 * t, dtype=np.int64).reshape(t, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-host-soup", action="store_true", help="do not time the host build of the 2^20 soup (~minutes)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"tool": "bench_bvh", "device": torch.cuda.get_device_name(0)}
    for name, (pos, tri) in (("clutter", clutter_geometry()), ("soup_2p20", soup_geometry(1 << 20))):
        p = torch.from_numpy(pos.astype(np.float32)).to(dev)
        t = torch.from_numpy(tri.astype(np.int32)).to(dev)
        r = {"triangles": int(tri.shape[0])}
        r["device_build_ms"] = median_ms(lambda: B.NativeBvh(p, t), args.reps)
        nb = B.NativeBvh(p, t)
        r["device_nodes"], r["device_levels"] = int(nb.nodes.shape[0]), nb.n_levels
        r["sah_device"] = B.sah_cost(nb.nodes)
        if name == "clutter" or not args.skip_host_soup:
            t0 = time.perf_counter()
            plan = S.build_bvh(pos, tri)
            r["host_build_ms"] = (time.perf_counter() - t0) * 1e3
            host = S.DeviceBvh(plan, dev)
            host.refit(p, t)
            r["host_nodes"], r["host_levels"] = int(host.nodes.shape[0]), len(B.level_table(plan["nodes"])) - 1
            r["sah_host"] = B.sah_cost(host.nodes)
            r["sah_ratio_device_over_host"] = r["sah_device"] / r["sah_host"]
            r["build_speedup"] = r["host_build_ms"] / r["device_build_ms"]
            if name == "clutter":                  # refit: both on the host builder's tree
                lb = B.level_table(plan["nodes"])
                r["refit_torch_ms"] = event_ms(lambda: host.refit(p, t), args.reps * 3)
                r["refit_kernel_ms"] = event_ms(lambda: B.refit(host.nodes, host.prim_index, host.tri_verts, lb, p, t), args.reps * 3)
                r["refit_speedup"] = r["refit_torch_ms"] / r["refit_kernel_ms"]
                r["refit_device_tree_kernel_ms"] = event_ms(lambda: nb.refit(p, t), args.reps * 3)
        out[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)

    import epsm_mitsuba3_amd as epsm
    res, spp = 512, 16
    g = torch.Generator().manual_seed(4)
    grad_in = (torch.randn((res, res, 5), generator=g) * 1e-3).to(dev)
    trace = {}
    for builder in ("host", "device"):
        sc = S.Scene.from_dict(clutter.scene_dict(n_spheres=100, res=res, spp=spp), device=dev, bvh_builder=builder)
        for i in range(0, 100, 7):
            sc.attach(f"s{i}", positions=True, normals=True)
        sc.tracer = "wavefront"
        integ = epsm.load_dict({"type": "manifold", "max_depth": clutter.max_depth})
        integ.backward_spp = spp
        params = sc.param_grads()
        trace[builder] = {
            "render_backward_ms": median_ms(lambda: integ.render_backward(sc, params, grad_in, seed=3), args.reps),
            "render_ms": median_ms(lambda: sc.render_primal(sensor=0, seed=0, spp=spp, max_depth=clutter.max_depth), args.reps)}
        print(builder, json.dumps(trace[builder]), file=sys.stderr, flush=True)
        del sc, params
        torch.cuda.empty_cache()
    for k in ("render_backward_ms", "render_ms"):
        trace["device_over_host_" + k[:-3]] = trace["device"][k] / trace["host"][k]
    out["clutter_512x512_16spp"] = trace
    print(json.dumps(out))


if __name__ == "__main__":
    main()
