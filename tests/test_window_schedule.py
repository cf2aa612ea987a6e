"""The window bookkeeping of the accumulating backward kernel on the host (csrc/epsm_cp_core.h through
tests/host_harness/cp_window_host.cpp: the functions the gfx950 kernel and its launcher call).

Slot word: the ONE 32-bit word a window keeps per sorted path -- the plan's bits 0..15, diffuse1, active1, in-range and the
path's slot in the window.  Every accessor the rounds use must read from it what it reads from the plan word.

Window schedule: a large launch of n paths on S > 0 workgroup slots (EPSM_OPT_WORKGROUP_SLOTS; 0, the default: no taper) with
bulk windows of W puts its last min(n, S W / 4) paths into windows of W / 4, the min(rest, S W / 2) before them into windows
of W / 2 and everything before that into windows of W; segments start on multiples of W, only the launch's last window is
ragged."""
import numpy as np
import pytest

from _window_host import FIELDS, host_window, slot_words, windows


@pytest.mark.parametrize("slot", [0, 1, 4095, 8191])
@pytest.mark.parametrize("variant", [0, 1], ids=["manifold", "manifold_caustic"])
def test_slot_word_round_trips_every_field(variant, slot):
    """A seeded million of the 2^25 flag words of K = 5 (plus the all-zero and the all-one word), one in sixteen of them outside
    the wavefront: nv, id*, a[1..5], b[1..5], diffuse1, active1, in-range and the slot come back from the slot word as the plan
    word (and the slot handed in) give them; an occupied entry is never 0, an entry outside the wavefront always."""
    rng = np.random.default_rng(1234 + variant)
    fw = rng.integers(0, 1 << 25, size=1_000_000, dtype=np.uint32)
    fw[0], fw[1] = 0, (1 << 25) - 1
    in_range = rng.integers(0, 16, size=fw.shape[0]) != 0
    in_range[:2] = True
    plan, word, fp, fs = slot_words(variant, 5, fw, in_range, slot)
    for j, name in enumerate(FIELDS):
        keep = in_range if name != "in_range" else np.ones_like(in_range)
        bad = np.nonzero((fp[:, j] != fs[:, j]) & keep)[0]
        assert bad.size == 0, (name, [hex(int(fw[i])) for i in bad[:4]])
    assert bool((word[in_range] != 0).all()) and bool((word[~in_range] == 0).all())
    assert bool((fs[in_range, FIELDS.index("slot")] == slot).all())
    assert bool(((word & 0xffff) == (plan & 0xffff))[in_range].all())
    # the fields are not trivially constant on this sample
    for name in ("nv", "a1", "b1", "diffuse1", "active1"):
        assert np.unique(fp[in_range, FIELDS.index(name)]).size > 1, name


def test_slot_word_at_fewer_vertices():
    """K < 5: the planning masks the flag word to 5 K bits first; the round trip holds there too."""
    rng = np.random.default_rng(7)
    fw = rng.integers(0, 1 << 25, size=100_000, dtype=np.uint32)
    for K in (1, 2, 3, 4):
        _, _, fp, fs = slot_words(0, K, fw, np.ones(fw.shape[0], bool), 2047)
        assert np.array_equal(fp, fs), K
        assert int(fp[:, FIELDS.index("nv")].max()) <= K


def _sizes_of_the_issue(n, S, W):
    """The closed form, restated: (start of the W / 2 segment, start of the W / 4 segment)."""
    tail_q = min(n, S * W // 4)
    start_q = (n - tail_q) // W * W
    tail_h = min(start_q, S * W // 2)
    start_h = (start_q - tail_h) // W * W
    return start_h, start_q


def _cases():
    out = []
    for W in (2048, 3072):
        for S in (1, 2, 768):
            ns = {0, 1, 63, 64, 65, W - 1, W, W + 1, S * W // 4 - 1, S * W // 4 + 1, 3 * S * W // 4 - 1, 3 * S * W // 4 + 1, 1 << 24, (1 << 31) + 7}
            out += [(n, S, W) for n in sorted(ns)]
    return out


@pytest.mark.parametrize("n,S,W", _cases())
def test_schedule_tiles_the_launch(n, S, W):
    first, size, count = windows(n, S, W)
    assert first.shape[0] == count == host_window().epsm_host_window_count(n, S, W)      # what the launcher sizes the grid with
    if n == 0:
        assert count == 0
        return
    # the windows tile [0, n) exactly once, in order
    assert int(first[0]) == 0 and bool((size > 0).all())
    assert np.array_equal(first[1:], first[:-1] + size[:-1]) and int(first[-1]) + int(size[-1]) == n
    # every start a multiple of 64; sizes W, W / 2, W / 4 -- except a ragged last window
    assert bool((first % 64 == 0).all())
    assert bool(np.isin(size[:-1], [W, W // 2, W // 4]).all())
    assert bool((np.diff(size[:-1]) <= 0).all())                     # bulk, then half, then quarter windows
    # the segments of the closed form: each starts on a multiple of W
    start_h, start_q = _sizes_of_the_issue(n, S, W)
    assert start_h % W == 0 and start_q % W == 0 and 0 <= start_h <= start_q <= n
    nominal = np.where(first < start_h, W, np.where(first < start_q, W // 2, W // 4))
    assert np.array_equal(size[:-1], nominal[:-1]) and int(size[-1]) == min(int(nominal[-1]), n - int(first[-1]))
    # ... and the taper holds what the closed form says, rounded up by less than a bulk window
    assert min(n, S * W // 4) <= n - start_q < min(n, S * W // 4) + W
    assert min(start_q, S * W // 2) <= start_q - start_h < min(start_q, S * W // 2) + W
    # the workgroups of a grid of any size walk all of them
    for grid in (1, 7, count, count + 1, 1 << 20):
        per = host_window().epsm_host_windows_per_workgroup(count, grid)
        assert per >= 1 and per * grid >= count and (per == 1 or (per - 1) * grid < count)


@pytest.mark.parametrize("n,W", [(0, 128), (1, 128), (257, 128), (2049, 1024), (1 << 20, 1024), ((1 << 31) + 7, 2048)])
def test_no_slots_no_taper(n, W):
    """S = 0 -- the small form, and the large one by default: windows of W, the last one ragged."""
    first, size, count = windows(n, 0, W)
    assert count == -(-n // W)
    assert np.array_equal(first, np.arange(count, dtype=np.int64) * W)
    if count:
        assert bool((size[:-1] == W).all()) and int(size[-1]) == n - (count - 1) * W


def test_workgroup_slots_option_round_trips_without_a_device():
    """include/epsm.h, EPSM_OPT_WORKGROUP_SLOTS: option 3 of epsm_set_option / epsm_get_option, default 0 = no taper;
    `_lib.options(workgroup_slots=...)` sets it for a block.  Option 4 is still unknown."""
    from epsm_mitsuba3_amd import _lib
    lib = _lib.lib()
    before = lib.epsm_get_option(_lib.OPT_WORKGROUP_SLOTS)
    assert _lib.OPT_WORKGROUP_SLOTS == 3 and before >= 0
    with _lib.options(workgroup_slots=2):
        assert lib.epsm_get_option(_lib.OPT_WORKGROUP_SLOTS) == 2
    assert lib.epsm_get_option(_lib.OPT_WORKGROUP_SLOTS) == before
    assert lib.epsm_set_option(_lib.OPT_WORKGROUP_SLOTS, -1) == -22
    assert lib.epsm_set_option(4, 1) == -22 and lib.epsm_get_option(4) == -1


def test_the_cases_of_the_device_test():
    """What tests/test_gpu_window_schedule.py runs on two workgroup slots, and 2 049 paths by default (no taper: one window of
    2 048 paths and one of a single path) and on the 768 slots of an MI355X (the whole launch is shorter than the taper)."""
    sizes = lambda n, S: windows(n, S, 2048)[1].tolist()
    assert sizes(1025, 2) == [512, 512, 1]
    assert sizes(3071, 2) == [512] * 5 + [511]
    assert sizes(3072, 2) == [1024, 1024, 512, 512]
    assert sizes(3073, 2) == [1024, 1024, 512, 512, 1]
    assert sizes(6145, 2) == [2048, 1024, 1024, 512, 512, 512, 512, 1]
    assert sizes(1500, 2) == [512, 512, 476]
    assert sizes(2049, 0) == [2048, 1]
    assert sizes(2049, 768) == [512] * 4 + [1]
