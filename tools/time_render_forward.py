"""Wall-clock of prb_reparam's render_forward against its render_backward at the same size: the 128 k-triangle clutter scene of
tools/bench_reparam.py, every tenth sphere attached (positions and normals), a 512 x 512 film at 16 spp with its sample
border (4.26 M paths), 16 auxiliary rays, max_depth 3.
    python tools/time_render_forward.py [RES] [SPP] [RAYS] [MAX_DEPTH] [REPEATS]
Prints one line per pass (median ms of REPEATS calls after one warm-up) and the transpose gap of the two passes."""
import sys
import time

sys.path.insert(0, ".")
import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd.exp import clutter
from epsm_mitsuba3_amd.scene import Scene

res = int(sys.argv[1]) if len(sys.argv) > 1 else 512
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 16
rays = int(sys.argv[3]) if len(sys.argv) > 3 else 16
depth = int(sys.argv[4]) if len(sys.argv) > 4 else 3
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
d = clutter.scene_dict(100, res, spp)
d["sensor0"]["film"]["sample_border"] = True
scene = Scene.from_dict(d, device="cuda")
for i in range(0, 100, 10):
    scene.attach(f"s{i}", positions=True, normals=True)
integ = epsm.load_dict({"type": "prb_reparam", "max_depth": depth, "reparam_rays": rays})
torch.manual_seed(0)
g = torch.randn((res, res, 3), device="cuda") * 1e-2
tan = scene.param_grads()
for i in range(0, 100, 10):
    tan.mesh_pos(f"s{i}")[:] = torch.randn_like(tan.mesh_pos(f"s{i}"))
    tan.mesh_nrm(f"s{i}")[:] = torch.randn_like(tan.mesh_nrm(f"s{i}"))
params = scene.param_grads()
out = {}


def backward():
    params.zero_()
    integ.render_backward(scene, params, g, sensor=0, seed=1, spp=spp)


def forward():
    out["img"] = integ.render_forward(scene, tan, sensor=0, seed=1, spp=spp)


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


n = scene.sensors[0].wavefront_size(spp)
tb = median_ms(backward)
tf = median_ms(forward)
a = float((g.double() * out["img"].double()).sum())
b = float((params.flat.double() * tan.flat.double()).sum())
S = float((g.double() * out["img"].double()).abs().sum() + (params.flat.double() * tan.flat.double()).abs().sum())
print(f"paths {n} ({res}x{res} @ {spp} spp + border), {rays} rays, max_depth {depth}, {scene.T} triangles")
print(f"render_backward {tb:.1f} ms")
print(f"render_forward  {tf:.1f} ms  (forward / backward {tf / tb:.2f})")
print(f"transpose gap |a - b| / S = {abs(a - b) / S:.2e}")
