"""EPSM_OPT_IOR_GRADS on the device: synthetic records through epsm_backward_pass (per-field records) and epsm_backward_pass_packed
(the native log) with the option on, in every launch form -- one ragged small window, the small form with replicas (summed by a
second kernel, and inside the launch), the large form, and a list of an eighth of the paths, small and large.

Expected ``alpha``: the float64 sum over the host core's outputs of the per-vertex rule
``eta != 1 ? fin(geta) * dhf.x : dot(fin(gm), dhf)`` (tests/_ior_cases.py), judged by test_gpu_pipeline.py's yardstick for ``alpha``:
2e-3 of the buffer's magnitude plus the allowance (components within 2 % of the clamp, twice the float32 core's distance from the
float64 one), which test_ior_synthetic.py keeps below a tenth of the magnitude for these seeds.

``pos`` and ``nrm`` with the option on equal the same launch with the option off, and so does every ``alpha`` entry whose slot
receives no vertex with eta != 1 -- as far as two launches of this kernel can be equal.  Bit for bit they are not, and neither
are two launches with the SAME option (the parent's kernel included): a term reaches its buffer either through a fixed-point row
of the LDS table, rounded to 2^-44 (epsm_wave_scatter.h, AccFixed64), or, where the table is full, as a float atomic of its own,
and which of the two is a race between the waves of a workgroup; rows that several paths share are moreover summed in an order no
two launches repeat.  So the comparison runs on the same records with PRIVATE addressing (tests/_per_path.py: its own rows and its
own slot for every (path, vertex) -- at most three terms per entry: the vertex's own row, the end-point row of the vertex before
it, diffuse_grad[0]) and allows what the number formats allow: 2^-45 per term and one float32 rounding of the entry,
``4 * 2^-45 + 2^-23 |entry|``.  Measured on an MI355X, `manifold` / `pool`, K = 1, 4 396 paths, large form: 637 of 39 564 entries
of ``pos`` differ between option on and off, 999 between two launches with the option off, none by more than 2^-45 = 2.84e-14.
Options come back in a ``finally`` (``_lib.options``)."""
import pytest
import torch

from _ior_cases import B, KS, N_LARGE, N_RAGGED, N_REPLICAS, PROFILES, RES, SPP, V, case, list_keep, private_case, reference

pytestmark = pytest.mark.gpu

DEFAULT = dict(small_wavefront_paths=1 << 20, replicas=True, one_launch=False)
FORMS = [("ragged window", N_RAGGED, {}, False), ("replicas", N_REPLICAS, {}, False), ("replicas, one launch", N_REPLICAS, {"one_launch": True}, False),
         ("large form", N_LARGE, {"small_wavefront_paths": 0}, False),
         ("list, small", N_REPLICAS, {}, True), ("list, large", N_LARGE, {"small_wavefront_paths": 0}, True)]


def _launch(variant, c, dev, packed, opts, ior, listed):
    import epsm_mitsuba3_amd as epsm
    from epsm_mitsuba3_amd import _lib
    from epsm_mitsuba3_amd.records import PackedLog, PackedRecords, PackedScatter
    from epsm_mitsuba3_amd.synth import path_info_to
    from epsm_mitsuba3_amd.tangent_scatter import backward_pass, backward_pass_packed
    tr, N = c["trace"], c["N"]
    grad_in = c["grad_in"].to(dev)
    p = epsm.ParamGrads(c.get("V", V), c.get("B", B), device=dev)
    with _lib.options(**{**DEFAULT, **opts, "ior_grads": ior}):          # (restores what it found, whatever happens inside)
        if packed:
            log = PackedLog.from_trace(tr, device=dev)
            if listed:
                ids = torch.nonzero(list_keep(N)).flatten()
                cap = torch.zeros(N, dtype=torch.int32)
                cap[:ids.numel()] = ids.to(torch.int32)
                log.set_path_list(cap.to(dev), torch.tensor([ids.numel()], dtype=torch.int32, device=dev))
            backward_pass_packed(variant, log, grad_in, SPP, RES, p.pos, p.nrm, p.alpha, None if listed else p.cam_origin, clip=0.1, path_offset=0)
        else:
            pi = path_info_to(tr.path_info, device=dev)
            si = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in r.items()} for r in tr.scatter_info]
            mv = lambda t: t.to(dev)
            backward_pass(variant, PackedRecords(pi, device=dev), PackedScatter(si, device=dev), mv(tr.ray_o), mv(tr.ray_d), mv(tr.ray_dx),
                          mv(tr.ray_dy), grad_in, SPP, RES, p.pos, p.nrm, p.alpha, p.cam_origin, clip=0.1, path_offset=0)
        torch.cuda.synchronize()
        assert _lib.lib().epsm_get_option(_lib.OPT_IOR_GRADS) == int(ior)
    return p


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("variant,profile", PROFILES)
def test_alpha_rows_of_refraction_vertices_are_ior_gradients(variant, profile, K):
    from epsm_mitsuba3_amd import _lib
    dev = torch.device("cuda", 0)
    before = _lib.lib().epsm_get_option(_lib.OPT_IOR_GRADS)
    seen = 0
    for form, N, opts, listed in FORMS:
        c = case(variant, profile, K, N)
        ref, allow, refracted, plain = reference(variant, profile, K, N, listed)
        m = float(ref.abs().max())
        for packed in ((True,) if listed else (False, True)):       # (a path list exists on the native log only)
            on = _launch(variant, c, dev, packed, opts, True, listed)
            off = _launch(variant, c, dev, packed, opts, False, listed)
            what = (variant, profile, K, form, "packed" if packed else "per-field")
            mine = on.alpha.double().cpu()
            err = (mine - ref).abs()
            print(*what, "max |alpha|", m, "worst (|diff| - allowance) / m", float((err - allow).max()) / max(m, 1e-300),
                  "allowance / m", float(allow.max()) / max(m, 1e-300), "|on - off| / m", float((mine - off.alpha.double().cpu()).abs().max()) / max(m, 1e-300))
            assert bool(torch.isfinite(on.flat).all()), what
            assert bool((err <= 2e-3 * m + allow).all()), (what, mine, ref)
            assert float(allow.max()) <= 0.1 * m, what
            if m > 0 and bool(refracted.any()):                 # the option has an effect where a refraction meets a slot
                seen += 1
                assert not torch.equal(on.alpha, off.alpha), what
            # a handful of terms per entry: equal up to the table's fixed-point rounding (module docstring)
            pc = private_case(variant, profile, K, N)
            on, off = _launch(variant, pc, dev, packed, opts, True, listed), _launch(variant, pc, dev, packed, opts, False, listed)
            quiet = pc["reflections"].to(dev)
            for name, x, y in (("pos", on.pos, off.pos), ("nrm", on.nrm, off.nrm), ("alpha", on.alpha[quiet], off.alpha[quiet])):
                x, y = x.double(), y.double()
                assert bool(((x - y).abs() <= 4 * 2.0 ** -45 + 2.0 ** -23 * y.abs()).all()), (what, name, float((x - y).abs().max()))
            assert float(off.pos.abs().max()) > 0 or m == 0, what
            if m > 0:
                assert bool((on.alpha[~quiet] != off.alpha[~quiet]).any()), what
    assert _lib.lib().epsm_get_option(_lib.OPT_IOR_GRADS) == before
    if (variant, profile) != ("manifold", "pool") and K >= 3:       # (`manifold` on `pool`: a diffuse first hit ends every chain)
        assert seen >= 6, seen


def test_precomputed_tangents_refuse_the_option():
    """include/epsm.h: with EPSM_OPT_IOR_GRADS = 1 the entry point that takes the caller's tangents returns -EINVAL and says why."""
    from epsm_mitsuba3_amd import _lib
    from epsm_mitsuba3_amd.records import PackedRecords, PackedScatter
    from epsm_mitsuba3_amd.synth import path_info_to
    from epsm_mitsuba3_amd.tangent_scatter import manifold_grad_scatter
    dev = torch.device("cuda", 0)
    c = case("manifold", "mixed", 3, N_RAGGED)
    tr = c["trace"]
    pi = path_info_to(tr.path_info, device=dev)
    si = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in r.items()} for r in tr.scatter_info]
    gp, gn, ga = torch.zeros((V, 3), device=dev), torch.zeros((V, 3), device=dev), torch.zeros(B, device=dev)
    args = ("manifold", PackedRecords(pi, device=dev), PackedScatter(si, device=dev), c["dlduv"].float().to(dev), c["dldp"].float().to(dev), gp, gn, ga)
    with _lib.options(ior_grads=True):
        with pytest.raises(_lib.EpsmError, match="EPSM_OPT_IOR_GRADS"):
            manifold_grad_scatter(*args)
    torch.cuda.synchronize()
    assert float(gp.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0
    manifold_grad_scatter(*args)                                   # ... and runs as ever without it
    torch.cuda.synchronize()
    assert float(gp.abs().max()) > 0.0
