"""The large-steps solve on one MI355X (smooth.MeshLaplacian.solve, csrc/epsm_trace_smooth.hip); ONE JSON line.
Per mesh -- the icosphere of exp/relief.py (642 vertices) and open grids of 6 890 (SMPL's count), 65 536 and 1 048 576 vertices --
at lambda = 19, rel_tol = 1e-6, from x0 = 0, the median HIP-event time of
  grid_ms / one_group_ms    the solve in each form (one_group up to its 13 312 vertices), with the iterations it took
  apply_ms                  one product (I + lambda L) x
  torch_sparse_ms           what a user could do without the kernels: the same conjugate gradients written with a torch.sparse
                            CSR matrix on the device, float32, its convergence test read on the host every iteration
and, beside them, one render_backward of exp/human.py's scene (``manifold``), the pass two solves per iteration follow.
--crossover adds grids between 2 048 and 13 312 vertices in both forms: the curves EPSM_SMOOTH_AUTO's constant is read from.
python tools/time_smooth.py [--reps 15] [--crossover] [--no-human]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bench_scene_tables import DEV, event_ms
from epsm_mitsuba3_amd import load_dict, smooth
from epsm_mitsuba3_amd.exp.clutter import icosphere

LAMBDA, REL_TOL = 19.0, 1e-6


def grid_faces(nx, ny):
    idx = np.arange(nx * ny).reshape(ny, nx)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    return np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32), nx * ny


def sparse_cg(A, b, max_iters):
    """Conjugate gradients with torch.sparse products, three columns at once, stopping when every column is inside REL_TOL."""
    x = torch.zeros_like(b)
    r = b.clone()
    p = r.clone()
    rr, bb = (r * r).sum(0), (b * b).sum(0)
    for k in range(max_iters):
        q = A @ p
        alpha = rr / (p * q).sum(0)
        x += alpha * p
        r -= alpha * q
        rr_new = (r * r).sum(0)
        if bool((rr_new <= REL_TOL * REL_TOL * bb).all()):
            return x, k + 1
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x, max_iters


def sparse_matrix(tri, V):
    e = smooth.unique_edges(torch.from_numpy(tri), V)
    deg = torch.zeros(V).index_add_(0, e.reshape(-1), torch.ones(e.numel()))
    i = torch.cat([e[:, 0], e[:, 1], torch.arange(V)])
    j = torch.cat([e[:, 1], e[:, 0], torch.arange(V)])
    w = torch.cat([torch.full((2 * e.shape[0],), -LAMBDA), 1.0 + LAMBDA * deg])
    return torch.sparse_coo_tensor(torch.stack([i, j]), w, (V, V)).coalesce().to_sparse_csr().to(DEV)


def case(tri, V, reps, forms=("grid", "one_group"), baseline=True):
    lap = smooth.MeshLaplacian(torch.from_numpy(tri), V, LAMBDA, device=DEV)
    b = torch.randn((V, 3), generator=torch.Generator().manual_seed(1)).to(DEV)
    out = {"vertices": V, "triangles": int(tri.shape[0]), "max_degree": lap.max_degree, "max_iters": lap.default_max_iters(REL_TOL)}
    out["apply_ms"] = event_ms(lambda: lap.apply(b), reps)
    for form in forms:
        if form == "one_group" and V > smooth.ONE_GROUP_MAX_V:
            continue
        out[form + "_ms"] = event_ms(lambda: lap.solve(b, rel_tol=REL_TOL, form=form), reps)
        out[form + "_iterations"] = max(i for i, _, _ in lap.info())
    if baseline:
        A = sparse_matrix(tri, V)
        x, its = sparse_cg(A, b, out["max_iters"])
        out["torch_sparse_iterations"] = its
        out["torch_sparse_ms"] = event_ms(lambda: sparse_cg(A, b, out["max_iters"]), max(3, reps // 3), warm=1)
        out["torch_sparse_vs_grid_rel"] = float((x - lap.solve(b, rel_tol=REL_TOL, form="grid")).norm() / x.norm())
    return out


def human_backward_ms(reps):
    from epsm_mitsuba3_amd.exp import human
    scene = human.load_scene(DEV)
    scene.attach("human", positions=True)
    integ = load_dict({"type": "manifold", "max_depth": human.max_depth})
    integ.render(scene, sensor=1, seed=0, spp=human.spp)
    params = scene.param_grads()
    grad = (torch.randn((human.resolution, human.resolution, 5), generator=torch.Generator().manual_seed(2)) * 1e-5).to(DEV)
    return {"vertices": scene.V, "triangles": scene.T, "resolution": human.resolution, "spp": human.spp,
            "render_backward_ms": event_ms(lambda: integ.render_backward(scene, params, grad, sensor=1, seed=1, spp=human.spp), reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--no-human", action="store_true")
    a = ap.parse_args()
    sv, sf = icosphere(3)
    result = {"lambda": LAMBDA, "rel_tol": REL_TOL,
              "icosphere_642": case(sf.astype(np.int32), sv.shape[0], a.reps),
              "grid_6890": case(*grid_faces(65, 106), a.reps),
              "grid_65536": case(*grid_faces(256, 256), a.reps),
              "grid_1048576": case(*grid_faces(1024, 1024), a.reps)}
    if a.crossover:
        result["crossover"] = [case(*grid_faces(64, n), a.reps, baseline=False) for n in (32, 48, 64, 96, 112, 128, 160, 208)]
    if not a.no_human:
        result["human"] = human_backward_ms(a.reps)
    result["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
