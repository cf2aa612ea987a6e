"""The colour adjoint with every replay kind attached at once (epsm_mitsuba3_amd/replays.py: the table PRBIntegrator loops over),
on the host build that holds four of the five kinds (tests/host_harness/trace_envpose_host.cpp: texture, alpha, material,
envpose).  The scene is test_envpose_adjoint's ball: 82 triangles under a 4 x 3 envmap, 16 x 16 @ 4 spp with the gaussian
filter's border -- 1600 paths, 12.5 workgroups of 128.  The GPU twin, with a roughness map for the fifth kind, is
tests/test_gpu_color_replays.py."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import epsm_mitsuba3_amd as epsm
from _scenes import quad
from test_envpose_adjoint import N_PATHS, SPP, _grad_image, env_scene

DEPTH, SEED = 4, 7
TILINGS = [None, 512]                            # one tile of 1600 paths; four tiles, the last one of 64 paths
ATTACH = {"color": lambda sc: sc.attach_color("floor.bsdf"),
          "texture": lambda sc: sc.attach_texture("sky"),
          "alpha_texture": lambda sc: sc.attach_texture("plate.bsdf.alpha.data"),          # (a scene with the plate)
          "alpha": lambda sc: sc.attach_alpha("ball.bsdf"),
          "conductor": lambda sc: sc.attach_conductor("ball.bsdf"),
          "env_pose": lambda sc: sc.attach_envmap_pose()}
HOST_KINDS = ("color", "texture", "alpha", "conductor", "env_pose")
BITWISE = ("color", "alpha", "conductor", "env_pose")          # sections of ParamGrads no float atomic adds to
# The texel section is summed by float atomics: it differs from run to run and between the combined call and a kind's own.
# Measured on the parent commit on the host twin, as a share of the section's largest element, over both tilings
# (MEASUREMENTS.md 30): two identical calls 1.14e-6, combined against alone 1.04e-6.  The bound is 8 times the larger.
TEXEL_SPREAD_HOST = 8 * 1.14e-6


def plate():
    """A small GGX plate beside the ball whose alpha is a 4 x 4 bilinear bitmap: the scene entry of the roughness-map replay."""
    pv, pf = quad(0.02, 0.4, up=True)
    alpha = (0.15 + 0.1 * np.random.default_rng(4).random((4, 4))).astype(np.float32)
    return {"plate": {"type": "mesh", "vertices": pv + np.array([0.85, -1.0, 0.0]), "faces": pf, "face_normals": True,
                      "texcoords": np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float),
                      "bsdf": {"type": "roughconductor", "material": "Al", "distribution": "ggx",
                               "alpha": {"type": "bitmap", "bitmap": alpha, "filter_type": "bilinear"}}}}


def all_scene(kinds, device="cpu", tile=None, with_plate=False):
    sc = env_scene("ball", "4x3", device=device, extra=plate() if with_plate else None)
    assert sc.sensors[0].wavefront_size(SPP) == N_PATHS == 1600
    if tile is not None:
        sc.tile_paths = tile
    for k in kinds:
        ATTACH[k](sc)
    return sc


@functools.lru_cache(maxsize=None)
def backward(kinds, tile, device="cpu", with_plate=False, run=0):
    """(scene, ParamGrads) of one prb.render_backward with ``kinds`` attached; computed once per argument tuple (``run`` tells
    two identical calls apart) and shared, never written to."""
    sc = all_scene(kinds, device, tile, with_plate)
    p = sc.param_grads()
    epsm.load_dict({"type": "prb", "max_depth": DEPTH}).render_backward(sc, p, _grad_image().to(sc.device), sensor=0, seed=SEED, spp=SPP)
    return sc, p


def texel_spreads(kinds, tile, device="cpu", with_plate=False):
    """Per texel kind of ``kinds``: (|combined - the kind alone|, |combined - the same call again|), each the largest element's
    difference as a share of the section's largest element."""
    _, both = backward(kinds, tile, device, with_plate)
    _, again = backward(kinds, tile, device, with_plate, run=1)
    out = {}
    for slot, k in enumerate(k for k in kinds if k in ("texture", "alpha_texture")):
        alone = backward((k,), tile, device, with_plate)[1].texture(0)
        top = float(alone.abs().max())
        assert top > 0 and both.texture(slot).shape == alone.shape
        out[k] = (float((both.texture(slot) - alone).abs().max()) / top, float((both.texture(slot) - again.texture(slot)).abs().max()) / top)
    return out


def check_combined_equals_separate(kinds, tile, bound, device="cpu", with_plate=False, bitwise=BITWISE):
    """Test 2 on either platform: every section of the combined call against the call with that kind alone."""
    _, both = backward(kinds, tile, device, with_plate)
    _, again = backward(kinds, tile, device, with_plate, run=1)
    want = {k: backward((k,), tile, device, with_plate)[1] for k in ("alpha", "conductor", "env_pose")}
    want["color"] = backward(("color", "env_pose"), tile, device, with_plate)[1]      # (colour alone: float film weights, ~2e-7 off)
    for k in BITWISE:
        got = getattr(both, k)
        assert float(got.abs().min()) > 0, k
        same, repeats = torch.equal(got, getattr(want[k], k)), torch.equal(got, getattr(again, k))
        print(f"{device} tile {tile} {k}: equal to its own call {same}, two combined calls equal {repeats}")
        if k in bitwise:
            assert same and repeats, k
    for k, (alone, repeat) in texel_spreads(kinds, tile, device, with_plate).items():
        print(f"{device} tile {tile} {k}: combined against alone {alone:.3e}, two combined calls {repeat:.3e} of the largest element")
        assert alone <= bound and repeat <= bound, (k, alone, repeat)


def combined_gap(integ, sc, seed, spp, gen):
    """test_envpose_adjoint.transpose_gap with a random tangent in EVERY attached section: (|a - b|, S, a, params, image
    tangent), a = sum g * J t, b = sum J^T g * t, S = sum |g * J t| + sum |J^T g * t|."""
    s = sc.sensors[0]
    t = sc.param_grads()
    rand = lambda v: v.copy_(torch.randn(tuple(v.shape), generator=gen).to(sc.device))
    for v in [t.color, t.alpha, t.conductor, t.env_pose] + [t.texture(k) for k in range(len(t.tex_shapes))]:
        rand(v)
    for m in sc.meshes:
        if m.pos_attached:
            lo, hi = t.mesh_slices[m.name]
            rand(t.pos[lo:hi])
    g = torch.randn((s.height, s.width, 3), generator=gen).to(sc.device)
    fwd = integ.render_forward(sc, t, sensor=0, seed=seed, spp=spp)
    params = sc.param_grads()
    integ.render_backward(sc, params, g, sensor=0, seed=seed, spp=spp)
    a = float((g * fwd).double().sum())
    b = float((params.flat * t.flat).double().sum())
    S_ = float((g * fwd).abs().double().sum()) + float((params.flat * t.flat).abs().double().sum())
    return abs(a - b), S_, a, params, fwd


TRANSPOSE = ["prb", "manifold", "prb_reparam"]


def check_combined_transpose(integ_name, depth, kinds, device="cpu", with_plate=False):
    """Test 3 on either platform."""
    sc = all_scene(kinds, device, with_plate=with_plate)
    if integ_name == "prb_reparam":
        sc.attach("ball")
    integ = epsm.load_dict({"type": integ_name, "max_depth": depth})
    gap, S_, a, params, _ = combined_gap(integ, sc, SEED, SPP, torch.Generator().manual_seed(2 + depth))
    print(f"{device} {integ_name} depth {depth}: transpose gap {gap / S_:.3e}")
    for k in BITWISE:
        assert float(getattr(params, k).abs().min()) > 0, k                        # every section is live
    sky = params.texture(0)                                                        # ("texture" is attached before "alpha_texture")
    assert sky.numel() == 36 and int((sky != 0).sum()) == 36                       # all 4 x 3 x 3 texels of the envmap
    if "alpha_texture" in kinds:
        assert float(params.texture(1).abs().max()) > 0                            # the roughness map's replay ran
    assert S_ > 0 and abs(a) > 0
    assert gap <= 1e-4 * S_, (gap, S_)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the table against the header
# ---------------------------------------------------------------------------------------------------------------------
def test_table_names_the_header_s_replay_entry_points():
    from _envpose_host import host_envpose_tracer
    from epsm_mitsuba3_amd import _lib, replays
    assert [r.name for r in replays.REPLAYS] == ["texture", "alpha_texture", "alpha", "material", "envpose"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "epsm_trace.h")).read()
    declared = {f"epsm_trace_paths_{stem}_{d}" for stem, d in re.findall(r"\bint epsm_trace_paths_(\w+)_(backward|forward)\(", header)}
    declared |= {f"epsm_trace_paths_{stem}" for stem in re.findall(r"\bint epsm_trace_paths_(\w+ward)\(", header)}
    declared = {e for e in declared if "reparam" not in e}
    entries = [r.entry(d) for r in replays.REPLAYS for d in ("backward", "forward")]
    assert len(set(entries)) == 10 and set(entries) == declared
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    for lib, n_expected in ((_lib.lib(), 10), (host_envpose_tracer(), 8)):
        exported = [e for e in entries if hasattr(lib, e)]
        assert len(exported) == n_expected                                         # (the host twin has no roughness-map replay)
        for r in replays.REPLAYS:
            for d in ("backward", "forward"):
                if r.entry(d) in exported:
                    fn = getattr(lib, r.entry(d))
                    assert fn.argtypes is not None and len(fn.argtypes) == 9 + len(r.tail(d)), r.entry(d)
            if r.workspace and hasattr(lib, r.workspace):
                assert getattr(lib, r.workspace).argtypes is not None, r.workspace


# ---------------------------------------------------------------------------------------------------------------------
# 2. the combined call equals the separate calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILINGS)
def test_combined_call_equals_the_separate_calls(tile):
    """alpha, conductor and env_pose are torch.equal to the call with that kind alone, colour to a call with colour and pose
    (colour alone divides by the float film weights), and two combined calls are torch.equal in all four.  The texels, summed by
    float atomics, stay within TEXEL_SPREAD_HOST of their own call and of a second combined call."""
    check_combined_equals_separate(HOST_KINDS, tile, TEXEL_SPREAD_HOST)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the combined transpose
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ_name", TRANSPOSE)
@pytest.mark.parametrize("depth", [2, 4])
def test_combined_forward_is_the_transpose_of_backward(integ_name, depth):
    """|<g, render_forward(t)> - <render_backward(g), t>| <= 1e-4 S for a random tangent in every attached section, the bound of
    every per-kind transpose test.  Measured on the parent commit: at most 8.3e-8 S in the six cases."""
    check_combined_transpose(integ_name, depth, HOST_KINDS)
