"""The four-wide BVH built and refitted on the device (epsm_bvh_build / epsm_bvh_refit, bvh.NativeBvh, Scene(bvh_builder=
"device")): the structure of tests/test_bvh_build.py, determinism, bit-identical refit against DeviceBvh.refit, SAH quality
against the host builder, closest hits against the float64 oracle of tests/_trace_replay.py, gradients against the host
tree, and the C++ host driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

from epsm_mitsuba3_amd import scene as S
from test_bvh_build import _check, _soup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


def _teapot():
    rng = np.random.default_rng(7)
    t = 20000
    sizes = 10.0 ** rng.uniform(-5, 1, size=t)
    cl = rng.normal(size=(12, 3)) * 10.0 ** rng.uniform(-2, 2, size=(12, 1))
    centres = cl[rng.integers(0, 12, size=t)] + rng.normal(size=(t, 3)) * 10.0 ** rng.uniform(-4, 1, size=(t, 1))
    return _soup(centres, sizes, rng)


def _chain():
    rng = np.random.default_rng(1)
    t = 1500
    s = 2.0 ** (-np.arange(t) / 25.0)
    return _soup(np.stack([s * 3.0, s * 2.0, s], axis=1), 0.05 * s, rng)


def _uniform():
    rng = np.random.default_rng(3)
    t = 4000
    return _soup(rng.uniform(-1, 1, size=(t, 3)), np.full(t, 0.02), rng)


def _clutter():
    """The 128 004 triangles of exp/clutter.py, concatenated in the scene's mesh order."""
    from epsm_mitsuba3_amd.exp import clutter
    d = clutter.scene_dict(n_spheres=100, res=16, spp=1)
    pos, tri, off = [], [], 0
    for v in d.values():
        if isinstance(v, dict) and v.get("type") == "mesh":
            pos.append(np.asarray(v["vertices"], np.float64)); tri.append(np.asarray(v["faces"], np.int64) + off)
            off += pos[-1].shape[0]
    return np.concatenate(pos), np.concatenate(tri)


def _small(t):
    rng = np.random.default_rng(100 + t)
    return _soup(rng.uniform(-1, 1, size=(t, 3)), np.full(t, 0.1), rng)


def _one_centroid():
    """10^5 triangles with one common centroid (every box centred on the origin, exactly: integer corners): no SAH plane
    anywhere, every split is the middle of the range."""
    rng = np.random.default_rng(9)
    t = 100000
    e = rng.integers(1, 1000, size=(t, 3))                       # half extents of the box
    d = np.empty((t, 3, 3), dtype=np.int64)
    d[:, 0], d[:, 1] = -e, e                                     # two corners span the box ...
    d[:, 2] = rng.integers(-e, e + 1)                            # ... the third lies inside it
    pos = (d * 1e-3).reshape(-1, 3)
    return pos, np.arange(3 * t, dtype=np.int64).reshape(t, 3)


def _device_tree(pos, tri):
    from epsm_mitsuba3_amd.bvh import NativeBvh
    p = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32)).to(DEV)
    b = NativeBvh(p, t)
    torch.cuda.synchronize()
    return b, p, t


def _plan_of(b):
    return {"nodes": b.nodes.cpu().numpy(), "order": b.prim_index.cpu().numpy().astype(np.int64)}


GEOMETRIES = {"teapot_in_a_stadium": _teapot, "geometric_chain": _chain, "uniform_soup": _uniform, "clutter": _clutter,
              "one_centroid": _one_centroid, **{f"T{t}": (lambda t=t: _small(t)) for t in range(1, 8)}}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_device_tree_structure(name):
    pos, tri = GEOMETRIES[name]()
    b, _, _ = _device_tree(pos, tri)
    T = tri.shape[0]
    nodes = b.nodes.cpu().numpy()
    levels = _check(_plan_of(b), pos.astype(np.float32).astype(np.float64), tri)
    assert levels <= S.kMaxWideDepth and b.n_levels == levels
    assert b.level_begin[0] == 0 and b.level_begin[-1] == nodes.shape[0]
    from epsm_mitsuba3_amd.bvh import level_table
    assert level_table(nodes) == b.level_begin                              # breadth first, levels contiguous
    tv = b.tri_verts.cpu().numpy()
    assert np.array_equal(tv, pos.astype(np.float32)[tri[b.prim_index.cpu().numpy().astype(np.int64)]].reshape(T, 9))
    if T <= S.LEAF_SIZE:
        c = nodes.view(np.int32)[0, 24:28]
        assert nodes.shape[0] == 1 and c[0] == ~T and (c[1:] == 0x7fffffff).all()


def test_two_builds_are_bit_identical():
    pos, tri = _clutter()
    a, _, _ = _device_tree(pos, tri)
    b, _, _ = _device_tree(pos, tri)
    for x, y in ((a.nodes, b.nodes), (a.prim_index, b.prim_index), (a.tri_verts, b.tri_verts)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert a.level_begin == b.level_begin


def test_refit_of_the_host_tree_is_bit_identical_to_the_torch_refit():
    from epsm_mitsuba3_amd import bvh
    pos, tri = _clutter()
    plan = S.build_bvh(pos, tri)
    rng = np.random.default_rng(2)
    moved = (pos + rng.normal(size=pos.shape) * 0.01).astype(np.float32)
    p = torch.from_numpy(moved).to(DEV)
    t = torch.from_numpy(tri.astype(np.int32)).to(DEV)
    ref = S.DeviceBvh(plan, DEV)
    ref.refit(p, t)
    mine = S.DeviceBvh(plan, DEV)
    mine.tri_verts = torch.zeros_like(ref.tri_verts)
    mine.nodes.view(torch.int32)[:, 0:24] = 0x7fc00000                     # boxes: NaN until the refit writes them
    bvh.refit(mine.nodes, mine.prim_index, mine.tri_verts, bvh.level_table(plan["nodes"]), p, t)
    torch.cuda.synchronize()
    assert torch.equal(mine.nodes.view(torch.int32), ref.nodes.view(torch.int32))
    assert torch.equal(mine.tri_verts.view(torch.int32), ref.tri_verts.view(torch.int32))


@pytest.mark.parametrize("name", ["clutter", "uniform_soup"])
def test_sah_cost_against_the_host_tree(name):
    from epsm_mitsuba3_amd.bvh import sah_cost
    pos, tri = GEOMETRIES[name]()
    b, p, t = _device_tree(pos, tri)
    host = S.DeviceBvh(S.build_bvh(pos, tri), DEV)
    host.refit(p, t)
    c_dev, c_host = sah_cost(b.nodes), sah_cost(host.nodes)
    print(name, "SAH cost device / host", c_dev, c_host, c_dev / c_host)
    assert c_dev <= 1.05 * c_host, (c_dev, c_host)


def _move_some_spheres(sc, step):
    for i in range(0, 100, 9):
        v = sc.vertex_positions(f"s{i}").clone()
        v[:, 2] += 0.15 * step
        v[:, 0] -= 0.1 * step
        sc.set_vertex_positions(f"s{i}", v)


@pytest.mark.parametrize("tracer", ["mega", "wavefront"])
def test_device_tree_hits_replay_against_brute_force(tracer):
    """The thresholds of test_gpu_tracer_oracle.py, on the device tree, before and after a refit moved some spheres."""
    from _trace_replay import replay
    from epsm_mitsuba3_amd.exp import clutter
    res, spp, K = 128, 8, 4
    sc = S.Scene.from_dict(clutter.scene_dict(n_spheres=100, res=res, spp=spp), device=DEV, bvh_builder="device")
    assert sc.T == 128004 and type(sc.bvh).__name__ == "NativeBvh"
    sc.tracer = tracer
    nodes_ptr = sc.bvh.nodes.data_ptr()
    for step in (0, 1):
        if step:
            _move_some_spheres(sc, step)
            assert sc.bvh.nodes.data_ptr() == nodes_ptr                        # refit in place
        n = res * res * spp
        tr = sc._trace(2, seed=7, spp=spp, max_depth=clutter.max_depth, K=K, lo=0, hi=n)
        torch.cuda.synchronize()
        rep = replay(sc, tr, K)
        print(tracer, step, rep)
        assert rep["primary_rays"] > 100000
        for name in ["primary", "bounce1", "bounce2", "bounce3"]:
            assert rep[name + "_hit_found"] >= 0.9999, (step, name, rep)
            assert rep[name + "_same_primitive"] >= 0.999, (step, name, rep)
            assert rep[name + "_exact_primitive"] >= 0.995, (step, name, rep)
            assert rep[name + "_t_agrees"] >= 0.999, (step, name, rep)
            assert rep[name + "_uv_agrees"] >= 0.995, (step, name, rep)
        assert rep["primary_miss_confirmed"] >= 0.999, rep
        assert rep["shadow_rays"] > 100000, rep
        assert rep["occluded_have_zero_weight"] >= 0.998, rep
        assert rep["emitter_point_rebuilt"] >= 0.999, rep


def test_gradients_with_the_device_tree_agree_with_the_host_tree():
    import epsm_mitsuba3_amd as epsm
    from _util import assert_two_routes_agree
    from epsm_mitsuba3_amd.exp import clutter
    res, spp = 128, 8
    g = torch.Generator().manual_seed(4)
    grad_in = (torch.randn((res, res, 5), generator=g) * 1e-3).to(DEV)
    bufs = []
    for builder, clip in (("device", None), ("host", None), ("host", 0.098), ("host", 0.102)):
        sc = S.Scene.from_dict(clutter.scene_dict(n_spheres=100, res=res, spp=spp), device=DEV, bvh_builder=builder)
        for i in range(0, 100, 7):
            sc.attach(f"s{i}", positions=True, normals=True)
        props = {"type": "manifold", "max_depth": clutter.max_depth}
        if clip is not None:
            props["outlier_clip"] = clip
        integ = epsm.load_dict(props)
        integ.backward_spp = spp
        p = sc.param_grads()
        integ.render_backward(sc, p, grad_in, seed=3)
        torch.cuda.synchronize()
        bufs.append(p.flat.double().cpu())
    assert float(bufs[0].abs().max()) > 0
    print(assert_two_routes_agree(*bufs, name="device tree vs host tree"))


def test_cpp_host_driver_builds_and_refits_a_tree():
    exe = os.path.join(ROOT, "examples", "build", "epsm_bvh_driver")
    if not os.path.isfile(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "-s"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().endswith("OK")
