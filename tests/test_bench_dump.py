"""bench.py --dump-outputs: the parameter-gradient buffer as float32 .npy files, whole when small, a fixed seeded sample of
rows under the 64 MB cap when large (CPU: the helper alone; the GPU run of the flag is bench.py's own)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from epsm_mitsuba3_amd.params import ParamGrads  # noqa: E402


def _params(V):
    p = ParamGrads(V, 4, device="cpu")
    p.flat.copy_(torch.arange(p.flat.numel(), dtype=torch.float32))
    return p


def test_small_buffer_is_written_whole(tmp_path):
    p = _params(1000)
    names = bench.dump_outputs(p, str(tmp_path))
    assert names == ["alpha", "cam_origin", "nrm", "pos"]
    for n in names:
        a = np.load(tmp_path / f"{n}.npy")
        assert a.dtype == np.float32
        assert np.array_equal(a, getattr(p, n).numpy())


def test_large_buffer_is_sampled_under_the_cap_and_repeatably(tmp_path):
    p = _params(3_000_000)                                  # 72 MB of pos + nrm
    bench.dump_outputs(p, str(tmp_path / "a"))
    bench.dump_outputs(p, str(tmp_path / "b"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    pos = np.load(tmp_path / "a" / "pos.npy")
    assert pos.shape[0] > 2_000_000 and pos.shape[1] == 3
    rows = pos[:, 0].astype(np.int64) // 3                  # arange content: row r starts at 3 r
    assert np.all(np.diff(rows) > 0)                        # sorted rows of the original buffer
    assert np.array_equal(pos, p.pos.numpy()[rows])
