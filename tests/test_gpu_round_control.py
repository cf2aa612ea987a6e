"""Round control and substitute loads of the accumulating backward kernel (csrc/epsm_backward_cp.hip).

The round loop keeps its control -- round index, class, lanes per path, the class bounds -- in scalar registers, and the
lanes of a round that have nothing to read load from an address that is always valid (the window's first record, its
first rays, the pixel of its first path) instead of branching around the load.  What can go wrong with that shows at
small sizes: windows with fewer rounds than waves, waves with unequal numbers of rounds, empty classes, a last window of
one path, a first round with nothing behind it -- and a substitute word that leaks into a result.

Every case gives each (path, vertex) PRIVATE parameter rows (tests/_per_path.py) and is judged by ``check_private_rows`` at
the tolerance of test_gpu_backward_per_path.py.  The wavefronts of N paths are the first N paths of ONE trace of 2 049 paths
per (integrator, profile, K): the rows of the other paths must stay exactly 0, and the rows of the first N must agree with
those of the launch over all 2 049 (the bound of test_path_list_per_path: 1e-5 of the row + 1e-7 of the buffer's magnitude),
which prices every path by itself where a statistic over one or 63 paths says little."""
import pytest
import torch

from _per_path import check_private_rows, private_addressing

pytestmark = pytest.mark.gpu

N_FULL = 2049
SIZES = [1, 63, 64, 65, 255, 257, 2049]
_cache = {}


def _setup(kind, profile, K, N=N_FULL, res=50, spp=8, seed=None):
    """One trace with private addressing, its native log and image gradient (made once per key, never modified)."""
    key = (kind, profile, K, N, res, spp)
    if key not in _cache:
        import epsm_mitsuba3_amd as epsm
        from epsm_mitsuba3_amd.records import PackedLog
        dev = torch.device("cuda", 0)
        scene = epsm.SyntheticScene(res=res, n_vertices=K, n_scene_vertices=3000, n_bsdfs=4, profile=profile, device=dev, tile_paths=N)
        trace = scene.tile(0, 0, N, seed=(17 + K) if seed is None else seed, spp=spp, K=K)
        gen = torch.Generator().manual_seed(3)
        table, si = private_addressing(N, K, dev, gen)
        trace.scatter_info = si
        grad_in = (torch.randn((res, res, 5), generator=gen) * 2e-5).to(dev)      # small tangents: few components near the +-0.1 clamp
        _cache[key] = (trace, si, grad_in, PackedLog.from_trace(trace))
    return _cache[key]


def _head(log, n):
    """The native log of the first n paths (views of the same storage)."""
    from epsm_mitsuba3_amd.records import PackedLog
    return PackedLog(log.rays[:n], log.flags[:n], log.verts[:n], log.shadow[:n] if log.shadow is not None else None, log.table, log.K)


def _run(kind, log, grad_in, spp, res, N, K, origin=True, path_offset=0):
    import epsm_mitsuba3_amd as epsm
    from epsm_mitsuba3_amd.tangent_scatter import backward_pass_packed
    p = epsm.ParamGrads(6 * N * K, N * K, device=log.device)
    backward_pass_packed(kind, log, grad_in, spp, res, p.pos, p.nrm, p.alpha, p.cam_origin if origin else None, clip=0.1,
                         path_offset=path_offset)
    torch.cuda.synchronize()
    return p


def _rows(p, N, K):
    """(N, every private row of the path)"""
    return torch.cat([p.pos.view(2, K, N, 9).permute(2, 0, 1, 3).reshape(N, -1), p.nrm.view(2, K, N, 9).permute(2, 0, 1, 3).reshape(N, -1),
                      p.alpha.view(K, N).t()], dim=1).double().cpu()


def _same_as_whole(got, whole, keep):
    m = float(whole.abs().max())
    assert m > 0
    assert float(got[~keep].abs().max()) == 0.0 if bool((~keep).any()) else True
    bad = ((got - whole).abs() > 1e-5 * whole.abs() + 1e-7 * m) & keep[:, None]
    assert not bool(bad.any()), ("paths off the launch over the whole log", torch.nonzero(bad.any(dim=1)).flatten()[:8].tolist())


@pytest.mark.usefixtures("window_form")
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("kind,profile", [("manifold", "bathroom"), ("manifold_caustic", "pool")])
def test_rounds_against_waves(kind, profile, K, N):
    """Small form: windows of 128 paths (N = 1 .. 257: one to three windows, the last one of 1, 63, 64 or 127 paths; 2 049: 17 windows);
    large form: ONE window of 2 048 paths and, at N = 2 049, a second one that holds a single path."""
    trace, si, grad_in, log = _setup(kind, profile, K)
    whole = _run(kind, log, grad_in, trace.spp, trace.res, N_FULL, K)
    if N == N_FULL:
        check_private_rows(kind, trace, si, whole, grad_in, K, label=f"{profile} N={N}")
        return
    keep = torch.arange(N_FULL) < N
    p = _run(kind, _head(log, N), grad_in, trace.spp, trace.res, N_FULL, K)
    _same_as_whole(_rows(p, N_FULL, K), _rows(whole, N_FULL, K), keep)
    # (the origin sum of the first N paths alone has no oracle here: the one of the whole trace is checked at N = 2 049)
    if float(_rows(whole, N_FULL, K)[:N].abs().max()) > 0:       # (a single path may carry no term at all: then all there is to see is zeros)
        check_private_rows(kind, trace, si, p, grad_in, K, label=f"{profile} N={N}", keep=keep, origin=False)


@pytest.mark.usefixtures("window_form")
def test_rounds_of_chains_of_five():
    """``specular`` at K = 5: every round is a chain of five, 12 paths on 60 lanes -- 130 paths are eleven rounds, the last with ten paths."""
    trace, si, grad_in, log = _setup("manifold", "specular", 5, N=130)
    p = _run("manifold", log, grad_in, trace.spp, trace.res, 130, 5)
    check_private_rows("manifold", trace, si, p, grad_in, 5, label="specular N=130")


@pytest.mark.usefixtures("window_form")
@pytest.mark.parametrize("kind,profile", [("manifold", "bathroom"), ("manifold_caustic", "pool")])
def test_rounds_over_a_path_list(kind, profile):
    """The windows over a list of 100 survivors of 257 paths (capacity 257, the tail repeats kept paths: a read past the count counts one twice)."""
    K, N = 5, 257
    trace, si, grad_in, full = _setup(kind, profile, K)
    whole = _rows(_run(kind, full, grad_in, trace.spp, trace.res, N_FULL, K, origin=False), N_FULL, K)
    from epsm_mitsuba3_amd.records import PackedLog
    flags = full.flags[:N].clone()                                   # (the shared log is not written to)
    gen = torch.Generator().manual_seed(5)
    ids = torch.randperm(N, generator=gen)[:100]
    keep = torch.zeros(N_FULL, dtype=torch.bool)
    keep[ids] = True
    flags[~keep[:N].to(flags.device)] = 0
    log = PackedLog(full.rays[:N], flags, full.verts[:N], None, full.table, K)
    lst = torch.cat([ids, ids.repeat(2)[:N - 100]]).to(torch.int32).to(flags.device)
    log.set_path_list(lst, torch.tensor([100], dtype=torch.int32, device=flags.device))
    p = _run(kind, log, grad_in, trace.spp, trace.res, N_FULL, K, origin=False)
    _same_as_whole(_rows(p, N_FULL, K), whole, keep)
    check_private_rows(kind, trace, si, p, grad_in, K, label=f"{profile} list of 100", keep=keep, origin=False)


@pytest.mark.parametrize("N", [300, 257])
@pytest.mark.parametrize("origin", [False, True], ids=["no origin sum", "origin sum"])
@pytest.mark.parametrize("kind,profile", [("manifold", "bathroom"), ("manifold_caustic", "pool")])
def test_substitute_record_is_never_used(kind, profile, origin, N, window_form):
    """The first path of every window -- paths 0, 128 and 256 in the small form, path 0 in the large one -- is what a lane without a
    need of its own loads: its flag word is 0 and its records, its rays, its occluder record and the image gradient at its pixel
    (spp = 1: the pixel is its own) are NaN.  Nothing of that may reach a row: the buffers must equal those of the same log with
    zeros in place of the NaNs.  At N = 257 path 256 is the only path of the small form's last window.
    With the camera-origin sum a path without a term still owes its share of it (epsm.py:260-261) and takes a lane that reads its
    rays and its pixel: there those two keep their values -- they ARE used -- and the records and the occluder record alone are NaN.

    `Equal`: a row's terms meet either in the 64-bit fixed-point table (resolution 2^-44) or, when the table is crowded, as float
    atomics, and which of the two is a matter of timing -- so two launches on the SAME log agree to one float rounding (2^-23
    relative) plus two table quanta (2^-43), not in every last bit.  That is the bound used; a leaked NaN or a leaked word of a
    foreign record misses it by orders of magnitude.
    The camera-origin sum is no such row: every workgroup adds its window's part to it with one float atomic per component, in
    whatever order the workgroups finish.  W parts summed in two different orders differ by at most 2 (W - 1) roundings of at most
    2^-24 sum |part| each; the parts are measured by launching every window by itself.  One window (the large form): no difference at all."""
    from _util import launch_form
    from epsm_mitsuba3_amd.records import PackedLog
    K, res = 3, 18                                                   # 324 pixels, one path each
    trace, si, grad_in, log0 = _setup(kind, profile, K, N=300, res=res, spp=1, seed=23)
    dev = log0.device
    bits = lambda x: x.to(torch.float32).contiguous().view(torch.int32)
    first = torch.arange(0, 300, 128)

    def make(fill, dis_on):
        # occluder record of the first vertex [triangle, b0, b1, dis]: the path's own emitter triangle of vertex 1 (private rows)
        dis = torch.rand(300, generator=torch.Generator().manual_seed(11)) if dis_on else torch.zeros(300)
        sb = torch.rand(300, 2, generator=torch.Generator().manual_seed(12)) * 0.5
        shadow = torch.stack([(300 * K + torch.arange(300)).to(torch.int32), bits(sb[:, 0]), bits(sb[:, 1]), bits(dis)], dim=1).to(dev)
        rays, verts, flags, g = log0.rays.clone(), log0.verts.clone(), log0.flags.clone(), grad_in.clone()
        flags[first] = 0
        verts[first] = fill
        shadow[first] = bits(torch.full((4,), fill)).to(dev)
        if not origin:
            rays[first] = fill
            g[first // res, first % res] = fill
        return _head(PackedLog(rays, flags, verts, shadow, log0.table, K), N), g

    window = launch_form(N, 6 * 300 * K, 300 * K, small_wavefront_paths=(1 << 20) if window_form == "windows of 256" else 0)[0]

    def origin_parts(log, g):
        """sum over the windows of |that window's part of the origin sum| (3,), and the number of windows"""
        tot = torch.zeros(3, dtype=torch.float64)
        for lo in range(0, N, window):
            hi = min(lo + window, N)
            sub = PackedLog(log.rays[lo:hi], log.flags[lo:hi], log.verts[lo:hi], log.shadow[lo:hi], log.table, K)
            tot += _run(kind, sub, g, 1, res, 300, K, path_offset=lo).cam_origin.double().abs().cpu()
        return tot, -(-N // window)

    keep = torch.ones(300, dtype=torch.bool)
    keep[first] = False
    keep[N:] = False
    emitter_rows = {}
    for dis_on in (True, False):
        (lz, gz), (ln, gn) = make(0.0, dis_on), make(float("nan"), dis_on)
        pz = _run(kind, lz, gz, 1, res, 300, K, origin=origin)
        pn = _run(kind, ln, gn, 1, res, 300, K, origin=origin)
        assert bool(torch.isfinite(pn.flat).all())
        assert float(pz.pos.abs().max()) > 0
        for a, b in ((pn.pos, pz.pos), (pn.nrm, pz.nrm), (pn.alpha, pz.alpha)):
            assert bool(((a - b).abs() <= 2.0 ** -23 * b.abs() + 2.0 ** -43).all())
        if origin:
            parts, W = origin_parts(lz, gz)
            diff = (pn.cam_origin.double() - pz.cam_origin.double()).abs().cpu()
            print("origin sum: |difference|", diff.tolist(), "sum |part|", parts.tolist(), "windows", W)
            assert float(pz.cam_origin.abs().max()) > 0
            assert bool((diff <= 2 * (W - 1) * 2.0 ** -24 * parts).all())
        emitter_rows[dis_on] = pz.pos.view(2, K, 300, 3, 3)[1, 0].clone()
    if profile == "bathroom":                                        # (its first hits are diffuse: there ARE occluder rows)
        assert not torch.equal(emitter_rows[True], emitter_rows[False])
    # without occluder rows (dis = 0) the buffers hold what check_private_rows knows: the poisoned log against the oracle
    check_private_rows(kind, trace, si, pn, grad_in, K, label=f"{profile} poisoned N={N}", keep=keep, origin=False)
