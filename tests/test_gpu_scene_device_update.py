"""Moving an emitting mesh with ``scene_tables="device"`` (Scene.set_vertex_positions: position rows, epsm_vertex_normals,
epsm_emitter_tables, a refit) against the host tables' route (a full _upload) on the plate and slab experiments: the same
primal image and the same gradients after the light moved, and the device move never calls _upload."""
import numpy as np
import pytest
import torch

from epsm_mitsuba3_amd import scene as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHIFT = torch.tensor([0.3, -0.2, 0.0])


def _run(exp, integrator, tables, monkeypatch, clip=None):
    import epsm_mitsuba3_amd as epsm
    sc = exp.load_scene(DEV, scene_tables=tables)
    sc.attach("light", positions=True)
    calls = []
    real = S.Scene._upload
    monkeypatch.setattr(S.Scene, "_upload", lambda self: (calls.append(1), real(self))[1])
    sc.set_vertex_positions("light", sc.vertex_positions("light").clone() + SHIFT.to(DEV))
    moved_uploads = len(calls)
    monkeypatch.setattr(S.Scene, "_upload", real)
    img = sc.render_primal(sensor=1, seed=5, spp=64, max_depth=exp.max_depth).cpu().double()
    props = {"type": integrator, "max_depth": exp.max_depth}
    if clip is not None:
        props["outlier_clip"] = clip
    integ = epsm.load_dict(props)
    integ.backward_spp = 16
    res = sc.sensors[integ.backward_sensor].width
    g = torch.Generator().manual_seed(9)
    grad_in = (torch.randn((res, res, 5), generator=g) * 1e-2).to(DEV)
    p = sc.param_grads()
    integ.render_backward(sc, p, grad_in, seed=2)
    torch.cuda.synchronize()
    return img, p.flat.double().cpu(), moved_uploads, sc


@pytest.mark.parametrize("name,integrator", [("plate", "manifold"), ("slab", "manifold_caustic")])
def test_device_move_of_the_light_agrees_with_the_host_route(name, integrator, monkeypatch):
    from _util import assert_two_routes_agree
    import importlib
    exp = importlib.import_module(f"epsm_mitsuba3_amd.exp.{name}")
    img_h, grad_h, up_h, sc_h = _run(exp, integrator, "host", monkeypatch)
    img_d, grad_d, up_d, sc_d = _run(exp, integrator, "device", monkeypatch)
    lo = _run(exp, integrator, "host", monkeypatch, clip=0.098)[1]      # the allowance of the outlier clamp's threshold
    hi = _run(exp, integrator, "host", monkeypatch, clip=0.102)[1]
    assert up_h == 1, "the host tables' route moves an emitting mesh with a full upload"
    assert up_d == 0, "the device move must not call _upload"
    assert float(img_h.abs().max()) > 0 and float(grad_h.abs().max()) > 0
    img_h = img_h.reshape(-1)
    print(assert_two_routes_agree(img_d.reshape(-1), img_h, img_h, img_h, name=f"{name} image"))
    print(assert_two_routes_agree(grad_d, grad_h, lo, hi, name=f"{name} gradients"))
    # the moved light's table entries: area and CDF as the host computes them from the new positions
    i = [m.name for m in sc_d.meshes].index("light")
    area_d = sc_d._mesh_buf.cpu().numpy().view(np.float32).reshape(-1, 8)[i, 5]
    assert abs(area_d - sc_h._mesh_structs[i].area) <= 1e-6 * sc_h._mesh_structs[i].area
    t0, t1 = sc_d.mesh_tri_slices["light"]
    assert torch.allclose(sc_d.emitter_cdf[t0:t1].cpu(), sc_h.emitter_cdf[t0:t1].cpu(), rtol=0, atol=1e-6)
    assert torch.equal(sc_d.vertex_positions("light").cpu(), sc_h.vertex_positions("light").cpu())


def _device_areas(sc):
    return sc._mesh_buf.cpu().numpy().view(np.float32).reshape(-1, 8)[:len(sc.meshes), 5].copy()


def test_attach_on_a_fresh_device_scene_keeps_the_device_areas():
    """_refresh_attach_flags rewrites only the flags words of the device mesh table: an attach() on a scene built with
    scene_tables="device" (no move, so no re-upload) must not put the host copy's areas -- which the device tables leave at 0 --
    over the ones the device computed."""
    from epsm_mitsuba3_amd.exp import plate
    sc = plate.load_scene(DEV, scene_tables="device")
    light = [m.name for m in sc.meshes].index("light")
    before = _device_areas(sc)
    assert before[light] > 0
    sc.attach("plate", positions=True)
    after = sc._mesh_buf.cpu().numpy().view(np.int32).reshape(-1, 8)
    assert np.array_equal(after.view(np.float32)[:len(sc.meshes), 5], before)
    assert after[[m.name for m in sc.meshes].index("plate"), 2] & S.MESH_POS_ATTACHED


def test_flag_refresh_without_host_sync_keeps_the_device_areas():
    """The sync_host=False form (prb_reparam's) after a device move: no upload can hide an overwrite."""
    from epsm_mitsuba3_amd.exp import plate
    sc = plate.load_scene(DEV, scene_tables="device")
    sc.set_vertex_positions("light", sc.vertex_positions("light").clone() * torch.tensor([2.0, 2.0, 1.0], device=DEV))
    before = _device_areas(sc)
    sc.mesh("plate").pos_attached = True
    sc._refresh_attach_flags(sync_host=False)
    assert np.array_equal(_device_areas(sc), before)
    assert before[[m.name for m in sc.meshes].index("light")] > 0


def test_envmap_tables_of_a_device_tables_scene_match_the_host_scene():
    """The _upload branch of scene_tables="device" for an envmap emitter: the same four tables as the host scene's."""
    rng = np.random.default_rng(4)
    bitmap = rng.uniform(0.0, 2.0, size=(16, 32, 3))
    bitmap[3] = 0.0

    def scene(tables):
        d = {"type": "scene", "sensor0": {"type": "perspective", "fov": 45, "to_world": S.look_at([0, -3, 1], [0, 0, 0], [0, 0, 1]),
                                          "film": {"type": "hdrfilm", "width": 8, "height": 8}},
             "floor": {"type": "mesh", "vertices": np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], float),
                       "faces": np.array([[0, 1, 2], [0, 2, 3]]), "bsdf": {"type": "diffuse"}},
             "sky": {"type": "envmap", "bitmap": bitmap}}
        return S.Scene.from_dict(d, device=DEV, scene_tables=tables)

    host, dev = scene("host"), scene("device")
    assert dev.c_scene.env.kind == 2 and (dev.c_scene.env.width, dev.c_scene.env.height) == (32, 16)
    for h, d in zip(host._env_buf, dev._env_buf):
        assert h.shape == d.shape
        assert torch.allclose(d.cpu(), h.cpu(), rtol=1e-6, atol=1e-12)
