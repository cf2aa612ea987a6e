"""World size 2 (gloo) on the host build of the tracer: the rigid twists and the sensor's rotation of a sharded prb_reparam pass
are reduced from the ALL-REDUCED vertex rows, so both ranks hold the same bits and they agree with one process."""
import multiprocessing as mp
import os
import socket

import numpy as np
import torch


def _pose_single(tile_paths):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import epsm_mitsuba3_amd as epsm_
    from test_rigid import pose_scene
    sc = pose_scene("translate_camera_lit", 12, 8, rigid_meshes=("sphere", "floor"), rotation=True)
    sc.tile_paths = tile_paths
    integ = epsm_.load_dict({"type": "prb_reparam", "max_depth": 3, "reparam_rays": 8})
    g = torch.randn((12, 12, 3), generator=torch.Generator().manual_seed(12))
    p = sc.param_grads()
    integ.render_backward(sc, p, g, sensor=0, seed=3, spp=8)
    integ.render_backward(sc, p, g, sensor=0, seed=4, spp=8)          # a second call accumulates: its contribution alone is summed
    return torch.cat([p.rigid.reshape(-1), p.cam_rotation, p.cam_origin])


def _pose_worker(rank, world, port, q):
    import torch.distributed as dist
    from epsm_mitsuba3_amd import dist as edist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    edist.init_from_env("gloo")
    out = _pose_single(512)
    q.put((rank, out.numpy().tobytes()))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_twists_and_sensor_rotation_match_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_pose_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[0] == got[1]                                              # both ranks hold identical bits
    single = _pose_single(512)
    both = torch.from_numpy(np.frombuffer(got[0], dtype=np.float32).copy())
    assert float(single[:12].abs().max()) > 0 and float(single[12:15].abs().max()) > 0
    # the bound of tests/test_render_forward.py::test_two_rank_forward_matches_single_process: the ranks sum the film and the rows
    # in another order
    for part in (slice(0, 12), slice(12, 15), slice(15, 18)):
        m = float(single[part].abs().max())
        assert torch.allclose(both[part], single[part], rtol=1e-4, atol=1e-5 * m), (both[part], single[part])
