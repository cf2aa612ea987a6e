"""The tapered window schedule and the slot word of the accumulating backward kernel (csrc/epsm_backward_cp.hip,
cp::window_schedule / cp::slot_word in csrc/epsm_cp_core.h) on the device.

Under EPSM_OPT_WORKGROUP_SLOTS = S > 0 a large wavefront ends in windows of half and a quarter of the bulk window, sized by
the S workgroup slots (off by default: MEASUREMENTS.md 27).  With TWO slots a few thousand paths meet every window size and
every segment boundary (tests/test_window_schedule.py pins the schedules themselves on the host):

    N = 1 025   512, 512, 1                                   taper only
    N = 3 071   512 x 5, 511                                   one path short of a half segment
    N = 3 072   1024, 1024, 512, 512                           both tapers, nothing ragged
    N = 3 073   1024, 1024, 512, 512, 1                        ... and a last window of one path
    N = 6 145   2048, 1024, 1024, 512 x 4, 1                   bulk + both tapers + a last window of one path

Every case gives each (path, vertex) PRIVATE parameter rows (tests/_per_path.py) and is judged by ``check_private_rows``; the
wavefronts of N paths are the first N paths of ONE trace of 6 145 paths per (integrator, profile): the rows of the other paths
must stay exactly 0, and the rows of the first N must agree with those of ONE launch over the whole trace in the default form
(a small wavefront: windows of 128 paths, no schedule) to 1e-5 of the row + 1e-7 of the buffer's magnitude."""
import pytest
import torch

from _per_path import check_private_rows, private_addressing

pytestmark = pytest.mark.gpu

K = 5
N_FULL = 6145
SIZES = [1025, 3071, 3072, 3073, 6145]
CASES = [("manifold", "bathroom"), ("manifold_caustic", "pool")]
_cache = {}


def _setup(kind, profile, res=50, spp=8):
    """One trace with private addressing, its native log, its image gradient and the rows of the launch over all of it in the
    default form (made once per key, never modified)."""
    key = (kind, profile)
    if key not in _cache:
        import epsm_mitsuba3_amd as epsm
        from epsm_mitsuba3_amd.records import PackedLog
        dev = torch.device("cuda", 0)
        scene = epsm.SyntheticScene(res=res, n_vertices=K, n_scene_vertices=3000, n_bsdfs=4, profile=profile, device=dev, tile_paths=N_FULL)
        trace = scene.tile(0, 0, N_FULL, seed=17 + K, spp=spp, K=K)
        gen = torch.Generator().manual_seed(3)
        table, si = private_addressing(N_FULL, K, dev, gen)
        trace.scatter_info = si
        grad_in = (torch.randn((res, res, 5), generator=gen) * 2e-5).to(dev)      # small tangents: few components near the +-0.1 clamp
        log = PackedLog.from_trace(trace)
        whole = _rows(_run(kind, log, grad_in, trace.spp, trace.res))
        _cache[key] = (trace, si, grad_in, log, whole)
    return _cache[key]


def _head(log, n):
    """The native log of the first n paths (views of the same storage)."""
    from epsm_mitsuba3_amd.records import PackedLog
    return PackedLog(log.rays[:n], log.flags[:n], log.verts[:n], log.shadow[:n] if log.shadow is not None else None, log.table, log.K)


def _run(kind, log, grad_in, spp, res, origin=True, **opts):
    import epsm_mitsuba3_amd as epsm
    from epsm_mitsuba3_amd import _lib
    from epsm_mitsuba3_amd.tangent_scatter import backward_pass_packed
    p = epsm.ParamGrads(6 * N_FULL * K, N_FULL * K, device=log.device)
    with _lib.options(**opts):
        backward_pass_packed(kind, log, grad_in, spp, res, p.pos, p.nrm, p.alpha, p.cam_origin if origin else None, clip=0.1)
        torch.cuda.synchronize()
    return p


def _rows(p):
    """(N_FULL, every private row of the path)"""
    N = N_FULL
    return torch.cat([p.pos.view(2, K, N, 9).permute(2, 0, 1, 3).reshape(N, -1), p.nrm.view(2, K, N, 9).permute(2, 0, 1, 3).reshape(N, -1),
                      p.alpha.view(K, N).t()], dim=1).double().cpu()


def _same_as_whole(got, whole, keep):
    m = float(whole.abs().max())
    assert m > 0
    if bool((~keep).any()):
        assert float(got[~keep].abs().max()) == 0.0
    bad = ((got - whole).abs() > 1e-5 * whole.abs() + 1e-7 * m) & keep[:, None]
    assert not bool(bad.any()), ("paths off the launch over the whole log", torch.nonzero(bad.any(dim=1)).flatten()[:8].tolist())


TAPER = dict(small_wavefront_paths=0, workgroup_slots=2)              # the large form on two workgroup slots


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind,profile", CASES)
def test_tapered_windows(kind, profile, N):
    trace, si, grad_in, log, whole = _setup(kind, profile)
    keep = torch.arange(N_FULL) < N
    p = _run(kind, _head(log, N), grad_in, trace.spp, trace.res, **TAPER)
    _same_as_whole(_rows(p), whole, keep)
    # (the origin sum of the first N paths alone has no oracle here: the one of the whole trace is checked at N = 6 145)
    check_private_rows(kind, trace, si, p, grad_in, K, label=f"{profile} N={N}", keep=None if N == N_FULL else keep, origin=N == N_FULL)


@pytest.mark.parametrize("kind,profile", CASES)
def test_tapered_windows_over_a_path_list(kind, profile):
    """The windows over a list of 1 500 survivors of 6 145 paths -- 512, 512, 476 on two slots, where the grid was sized for the
    eight windows of all 6 145 -- with capacity 6 145: the tail repeats kept paths, so a read past the count counts one twice."""
    from epsm_mitsuba3_amd.records import PackedLog
    trace, si, grad_in, full, whole = _setup(kind, profile)
    flags = full.flags.clone()                                       # (the shared log is not written to)
    gen = torch.Generator().manual_seed(5)
    ids = torch.randperm(N_FULL, generator=gen)[:1500]
    keep = torch.zeros(N_FULL, dtype=torch.bool)
    keep[ids] = True
    flags[~keep.to(flags.device)] = 0
    log = PackedLog(full.rays, flags, full.verts, None, full.table, K)
    lst = torch.cat([ids, ids.repeat(4)[:N_FULL - 1500]]).to(torch.int32).to(flags.device)
    log.set_path_list(lst, torch.tensor([1500], dtype=torch.int32, device=flags.device))
    p = _run(kind, log, grad_in, trace.spp, trace.res, origin=False, **TAPER)
    _same_as_whole(_rows(p), whole, keep)
    check_private_rows(kind, trace, si, p, grad_in, K, label=f"{profile} list of 1500", keep=keep, origin=False)


@pytest.mark.parametrize("kind,profile", CASES)
def test_default_slots_at_2049_paths(kind, profile):
    """EPSM_OPT_WORKGROUP_SLOTS left at 0, its default, in the large form at 2 049 paths: no taper -- one window of 2 048 paths
    and one that holds a single path (tests/test_window_schedule.py).  Same rows as the whole trace's launch."""
    from epsm_mitsuba3_amd import _lib
    assert _lib.lib().epsm_get_option(_lib.OPT_WORKGROUP_SLOTS) == 0
    N = 2049
    trace, si, grad_in, log, whole = _setup(kind, profile)
    keep = torch.arange(N_FULL) < N
    p = _run(kind, _head(log, N), grad_in, trace.spp, trace.res, small_wavefront_paths=0)
    _same_as_whole(_rows(p), whole, keep)
    check_private_rows(kind, trace, si, p, grad_in, K, label=f"{profile} N={N}, default slots", keep=keep, origin=False)
