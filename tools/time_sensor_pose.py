"""Times one prb_reparam render_backward on the scene of exp/camera.py with the sensor attached: `translation` = attach_sensor(),
`rotation` = attach_sensor(rotation=True) (MEASUREMENTS 16.3).  The sums over all vertex rows are epsm_rigid_reduce in both; the
rotation's pass attaches the normals of the vertex-normal meshes too.  Device events around each call, warm, best and median of `reps`.

    python tools/time_sensor_pose.py translation|rotation [res] [spp] [out.json]
"""
import json
import statistics
import sys

import torch

import epsm_mitsuba3_amd as epsm
from epsm_mitsuba3_amd.exp import camera


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "rotation"
    res, spp = (int(sys.argv[2]) if len(sys.argv) > 2 else 256), (int(sys.argv[3]) if len(sys.argv) > 3 else 16)
    camera.resolution = res
    sc = camera.load_scene("cuda")
    if mode == "rotation":
        sc.attach_sensor(rotation=True)
    else:
        sc.attach_sensor()
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": camera.max_depth})
    g = torch.randn((res, res, 3), generator=torch.Generator().manual_seed(1)).cuda()
    params = sc.param_grads()
    call = lambda: integ.render_backward(sc, params, g, sensor=0, seed=3, spp=spp)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(15):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    out = {"mode": mode, "res": res, "spp": spp, "vertices": sc.V, "best_ms": min(ms), "median_ms": statistics.median(ms)}
    print(json.dumps(out))
    if len(sys.argv) > 4:
        open(sys.argv[4], "w").write(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
