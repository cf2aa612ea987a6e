"""Scene.tile_plan: this rank's tiles of every pass that cuts a wavefront -- the backward trace (iter_traces), render_primal,
prb's colour pass and prb_reparam -- for both tracer forms, one to three ranks, a default or an assigned tile_paths and a
WAVEFRONT_TILE_PATHS lowered to test sizes.  The expected tiles are written out from the policies the passes had while each
cut its own; the passes are run on the host build of the tracer (tests/host_harness) and their tiles observed too."""
import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _scenes import on_host, quad, sensor
from epsm_mitsuba3_amd import dist as edist
from epsm_mitsuba3_amd import scene as S

RES, SPP = 8, 4
N_PATHS = RES * RES * SPP                                  # 256
TILE, WAVEFRONT_TILE = 48, 100

# world size -> [rank 0's tiles, rank 1's, ...]
BY_TILE = {1: [[(0, 48), (48, 96), (96, 144), (144, 192), (192, 240), (240, 256)]],
           2: [[(0, 48), (96, 144), (192, 240)], [(48, 96), (144, 192), (240, 256)]],
           3: [[(0, 48), (144, 192)], [(48, 96), (192, 240)], [(96, 144), (240, 256)]]}
# tile_paths widened to the share of a rank (256, 128, 86 paths) up to WAVEFRONT_TILE_PATHS = 100
WIDE = {1: [[(0, 100), (100, 200), (200, 256)]],
        2: [[(0, 100), (200, 256)], [(100, 200)]],
        3: [[(0, 86)], [(86, 172)], [(172, 256)]]}
# the share of a rank (up to REPARAM_TILE_PATHS = 2^23)
SHARE = {1: [[(0, 256)]],
         2: [[(0, 128)], [(128, 256)]],
         3: [[(0, 86)], [(86, 172)], [(172, 256)]]}

GRID = [(tracer, assigned, world, rank) for tracer in ("mega", "wavefront") for assigned in (False, True)
        for world in (1, 2, 3) for rank in range(world)]


def expected(pass_, tracer, assigned):
    if pass_ == "trace":
        return WIDE if tracer == "wavefront" else BY_TILE        # an assigned tile_paths does not bound the wavefront form
    if pass_ == "color":
        return BY_TILE
    return BY_TILE if assigned else SHARE


def make_scene(tracer, assigned):
    fv, ff = quad(0.0, 2.0, up=True)
    lv, lf = quad(2.0, 0.4, up=False)
    d = {"type": "scene", "cam": sensor([0.0, -3.0, 1.5], [0, 0, 0], up=(0, 0, 1), res=RES, spp=SPP, rfilter="gaussian"),
         "floor": {"type": "mesh", "vertices": fv, "faces": ff, "face_normals": True,
                   "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.4, 0.3]}}},
         "light": {"type": "mesh", "vertices": lv, "faces": lf, "face_normals": True,
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [20.0, 20.0, 20.0]}}}}
    sc = on_host(S.Scene.from_dict(d, device="cpu"))
    sc.tracer = tracer
    sc.tile_paths = TILE
    sc.tile_paths_explicit = assigned                            # False: TILE stands for the default
    sc.WAVEFRONT_TILE_PATHS = WAVEFRONT_TILE
    return sc


def spy(monkeypatch, sc, name, calls, lo_at):
    """Records (lo, hi) of every call of the Scene method ``name`` (its positional arguments lo_at, lo_at + 1)."""
    real = getattr(sc, name)

    def wrapper(*a, **kw):
        calls.append((a[lo_at], a[lo_at + 1]))
        return real(*a, **kw)
    monkeypatch.setattr(sc, name, wrapper)


@pytest.mark.parametrize("pass_", ["trace", "color", "reparam"])
def test_tile_plan_of_every_pass(pass_):
    for tracer in ("mega", "wavefront"):
        for assigned in (False, True):
            sc = make_scene(tracer, assigned)
            for world in (1, 2, 3):
                got = [sc.tile_plan(N_PATHS, pass_, rank, world) for rank in range(world)]
                assert got == expected(pass_, tracer, assigned)[world], (tracer, assigned, world)


def test_reparam_tiles_stop_at_their_cap():
    sc = make_scene("mega", False)
    sc.REPARAM_TILE_PATHS = 64
    assert sc.tile_plan(N_PATHS, "reparam", 0, 1) == [(0, 64), (64, 128), (128, 192), (192, 256)]
    assert sc.tile_plan(N_PATHS, "reparam", 1, 3) == [(64, 128)]
    sc.tile_paths_explicit = True
    assert sc.tile_plan(N_PATHS, "reparam", 0, 1) == BY_TILE[1][0]
    with pytest.raises(ValueError):
        sc.tile_plan(N_PATHS, "primal", 0, 1)


@pytest.mark.parametrize("tracer,assigned,world,rank", GRID)
def test_backward_trace_runs_its_tiles(tracer, assigned, world, rank):
    sc = make_scene(tracer, assigned)
    for packed_log in (False, True):
        got = [(t.path_offset, t.path_offset + t.ray_o.shape[0])
               for t in sc.iter_traces(sensor=0, seed=1, spp=SPP, max_depth=2, rank=rank, world_size=world, packed_log=packed_log)]
        assert got == expected("trace", tracer, assigned)[world][rank]


@pytest.mark.parametrize("tracer,assigned,world,rank", GRID)
def test_render_primal_runs_its_tiles(monkeypatch, tracer, assigned, world, rank):
    sc = make_scene(tracer, assigned)
    calls = []
    spy(monkeypatch, sc, "_trace", calls, 5)
    img = sc.render_primal(sensor=0, seed=1, spp=SPP, max_depth=2, rank=rank, world_size=world)
    assert calls == expected("trace", tracer, assigned)[world][rank]
    assert tuple(img.shape) == (RES, RES, 3) and bool(np.isfinite(img.numpy()).all())


@pytest.mark.parametrize("tracer,assigned,world,rank", GRID)
def test_prb_color_pass_runs_its_tiles(monkeypatch, tracer, assigned, world, rank):
    sc = make_scene(tracer, assigned)
    sc.attach_color("floor.bsdf")
    monkeypatch.setattr(edist, "world", lambda: (rank, world))
    calls = []
    spy(monkeypatch, sc, "trace_color", calls, 4)
    integ = epsm.load_dict({"type": "prb", "max_depth": 2})
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((RES, RES, 3)), sensor=0, seed=1, spp=SPP)
    assert calls == expected("color", tracer, assigned)[world][rank]


@pytest.mark.parametrize("tracer,assigned,world,rank", GRID)
def test_prb_reparam_runs_its_tiles(monkeypatch, tracer, assigned, world, rank):
    sc = make_scene(tracer, assigned)
    sc.attach("light", positions=True)
    monkeypatch.setattr(edist, "world", lambda: (rank, world))
    primal, replay = [], []
    spy(monkeypatch, sc, "_trace", primal, 5)
    spy(monkeypatch, sc, "trace_reparam", replay, 4)
    integ = epsm.load_dict({"type": "prb_reparam", "max_depth": 2, "reparam_rays": 4})
    p = sc.param_grads()
    integ.render_backward(sc, p, torch.ones((RES, RES, 3)), sensor=0, seed=1, spp=SPP)
    want = expected("reparam", tracer, assigned)[world][rank]
    assert primal == want and replay == want
