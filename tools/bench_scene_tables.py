"""The scene tables side by side on one MI355X; prints ONE JSON line.
  tables  vertex normals and emitter CDFs / areas of every mesh: numpy (scene.vertex_normals + the area loop of Scene._upload)
          against the device entries (epsm_vertex_normals, epsm_emitter_tables), on clutter (128 004 triangles) and on one
          mesh of 1 048 352 triangles; the topology build (once per triangle set) on its own
  envmap  scene.environment_tables against epsm_environment_tables on a 1024 x 2048 map
  move    Scene.set_vertex_positions of clutter's area light, scene_tables="host" (a full _upload with the host BVH builder:
          the fingerprint cache misses on every move) against "device"
python tools/bench_scene_tables.py [--reps 7] [--host-moves 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd import scene_tables as st
from epsm_mitsuba3_amd.exp import clutter

DEV = torch.device("cuda", 0)


def wall_ms(fn, reps, warm=1):
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


def meshes_of(d):
    return [(np.asarray(v["vertices"], np.float64), np.asarray(v["faces"], np.int64), not v.get("face_normals", False))
            for v in d.values() if isinstance(v, dict) and v.get("type") == "mesh"]


def grid_mesh(n=725):
    x, y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    v = np.stack([x.ravel(), y.ravel(), 0.1 * np.sin(5 * x.ravel()) * np.cos(3 * y.ravel())], axis=1)
    a = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).ravel()
    f = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)])
    return [(v, f, True)]


def tables_case(ms, reps):
    table, vb, pos, tri, toff = (S.EpsmMesh * len(ms))(), [0], [], [], 0
    for i, (v, f, flagged) in enumerate(ms):
        c = table[i]
        c.tri_begin, c.tri_count, c.cdf_begin, c.flags = toff, f.shape[0], toff, S.MESH_VERTEX_NORMALS if flagged else 0
        pos.append(v); tri.append(f + vb[-1])
        toff += f.shape[0]
        vb.append(vb[-1] + v.shape[0])
    P = torch.from_numpy(np.concatenate(pos).astype(np.float32)).to(DEV)
    TRI = torch.from_numpy(np.concatenate(tri).astype(np.int32)).to(DEV)
    nrm = torch.zeros_like(P)
    buf = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    cdf = torch.empty(TRI.shape[0], dtype=torch.float32, device=DEV)
    top = st.SceneTopology(TRI, P.shape[0])

    def host():
        for v, f, flagged in ms:
            if flagged:
                S.vertex_normals(v, f)
            p = v[f]
            a = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
            np.cumsum(a) / max(a.sum(), 1e-30)

    return {"triangles": int(TRI.shape[0]), "meshes": len(ms),
            "host_numpy_ms": wall_ms(host, max(1, reps // 3)),
            "device_topology_ms": event_ms(lambda: st.SceneTopology(TRI, P.shape[0]), reps),
            "device_normals_ms": event_ms(lambda: st.vertex_normals(P, top, table, vb, nrm), reps),
            "device_emitter_tables_ms": event_ms(lambda: st.emitter_tables(P, TRI, table, buf, cdf), reps)}


def envmap_case(reps):
    rng = np.random.default_rng(0)
    bm = rng.uniform(0, 4, size=(1024, 2048, 3)).astype(np.float32)
    t = torch.from_numpy(bm).to(DEV)
    return {"size": [1024, 2048], "host_numpy_ms": wall_ms(lambda: S.environment_tables(bm.astype(np.float64)), max(1, reps // 3)),
            "device_ms": event_ms(lambda: st.environment_tables(t), reps)}


def move_case(tables, moves):
    sc = S.Scene.from_dict(clutter.scene_dict(n_spheres=100, res=64, spp=1), device=DEV, scene_tables=tables)
    base = sc.vertex_positions("light").clone()
    out = []
    for k in range(moves + 1):
        v = base + torch.tensor([0.01 * (k + 1), 0.0, 0.0], device=DEV)
        torch.cuda.synchronize()
        t = time.perf_counter()
        sc.set_vertex_positions("light", v)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out[1:]))                   # the first move pays one-time costs (kernel loading, allocator)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-moves", type=int, default=3)
    a = ap.parse_args()
    res = {"clutter": tables_case(meshes_of(clutter.scene_dict(n_spheres=100, res=16, spp=1)), a.reps),
           "grid_2^20": tables_case(grid_mesh(), a.reps),
           "envmap": envmap_case(a.reps),
           "move_emitter_ms": {"host": move_case("host", a.host_moves), "device": move_case("device", max(a.reps, 5))},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
