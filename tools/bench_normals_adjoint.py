"""The derivative of the recomputed vertex normals on one MI355X, next to the primal and to what a user had before; ONE JSON line.
Per case (clutter: 128 004 triangles over its meshes; one mesh of 1 048 352 triangles), median HIP-event time of
  normals        epsm_vertex_normals
  backward       epsm_vertex_normals_backward (two launches)
  forward        epsm_vertex_normals_forward
  autograd_vjp   float32 torch autograd of scene.vertex_normals_torch on the device, forward + backward of one vjp per mesh that
                 has vertex normals -- the chain a user had to write by hand, index_add_ atomics and all
and the largest |backward - autograd_vjp| relative to the largest entry (float32 autograd against the fp64 kernel).
python tools/bench_normals_adjoint.py [--reps 15]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bench_scene_tables import DEV, event_ms, grid_mesh, meshes_of
from epsm_mitsuba3_amd import scene as S
from epsm_mitsuba3_amd import scene_tables as st
from epsm_mitsuba3_amd.exp import clutter


def case(ms, reps):
    table, vb, pos, tri, toff = (S.EpsmMesh * len(ms))(), [0], [], [], 0
    for i, (v, f, flagged) in enumerate(ms):
        c = table[i]
        c.tri_begin, c.tri_count, c.flags = toff, f.shape[0], S.MESH_VERTEX_NORMALS if flagged else 0
        pos.append(v); tri.append(f + vb[-1])
        toff += f.shape[0]
        vb.append(vb[-1] + v.shape[0])
    P = torch.from_numpy(np.concatenate(pos).astype(np.float32)).to(DEV)
    TRI = torch.from_numpy(np.concatenate(tri).astype(np.int32)).to(DEV)
    top = st.SceneTopology(TRI, P.shape[0])
    gen = torch.Generator().manual_seed(0)
    g = torch.randn(tuple(P.shape), generator=gen).to(DEV)
    nrm, out = torch.zeros_like(P), torch.zeros_like(P)
    faces = [(lo, hi, torch.from_numpy(f).to(DEV)) for (v, f, flagged), lo, hi in zip(ms, vb, vb[1:]) if flagged]

    def autograd(into=None):
        for lo, hi, f in faces:
            x = P[lo:hi].detach().requires_grad_(True)
            (gx,) = torch.autograd.grad((S.vertex_normals_torch(x, f) * g[lo:hi]).sum(), x)
            if into is not None:
                into[lo:hi] = gx

    ref, mine = torch.zeros_like(P), torch.zeros_like(P)
    autograd(ref)
    st.vertex_normals_backward(P, TRI, table, vb, g, mine, topology=top)
    return {"triangles": int(TRI.shape[0]), "vertices": int(P.shape[0]), "meshes_with_normals": len(faces),
            "normals_ms": event_ms(lambda: st.vertex_normals(P, top, table, vb, nrm), reps),
            "backward_ms": event_ms(lambda: st.vertex_normals_backward(P, TRI, table, vb, g, out, topology=top), reps),
            "forward_ms": event_ms(lambda: st.vertex_normals_forward(P, TRI, table, vb, g, out, topology=top), reps),
            "autograd_vjp_ms": event_ms(autograd, reps),
            "backward_vs_autograd_rel": float((mine - ref).abs().max() / ref.abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    print(json.dumps({"clutter": case(meshes_of(clutter.scene_dict(n_spheres=100, res=16, spp=1)), a.reps),
                      "grid_2^20": case(grid_mesh(), a.reps), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
