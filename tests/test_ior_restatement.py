"""d / d eta_k of epsm_cp_core.h against a float64 restatement of the reference's linear systems with eta as a parameter column
(tests/_ior_oracle.py), on the 16 goldens of tests/golden/.

The reference has no eta gradient, so the restatement is a yardstick only after it reproduces what the reference DOES compute:
its normal and hf columns against ``ref64_param`` to the bound test_oracle_golden.py applies to the float64 oracle (1e-7 of the
path's scale, the same zero pattern) -- the first test.  Then the float64 host core's ``geta`` (tests/host_harness/cp_ior_host.cpp)
against the restatement's eta column to that same bound, and the float32 host core to the bound test_kernel_core_host.py applies
to the core's lists: inside the conditioning gate cond_2 < 1e4 at most max(1, 0.5 % of the paths) may leave
scale * max(2e-4, 4 eps cond)."""
import functools

import pytest
import torch

from _ior_host import host_ior_calc_grad
from _ior_oracle import calc_grad_with_eta
from _util import gated_parity_report, golden_files, golden_id, load_golden
from oracle.binding import oracle_cond

FILES = golden_files()


@functools.lru_cache(maxsize=None)
def _restated(path):
    variant, pi, dlduv, dldp, ref = load_golden(path, dtype=torch.float64)
    return calc_grad_with_eta(variant, pi, dlduv, dldp)


def _scale(ref):
    truth = torch.cat([ref["ref64_param"], ref["ref64_light"], ref["ref64_diffuse"]]).double()
    return truth.abs().amax(dim=(0, 2)).clamp_min(1e-12)


def test_goldens_present():
    assert len(FILES) >= 16


@pytest.mark.parametrize("path", FILES, ids=golden_id)
def test_restatement_reproduces_the_reference_normal_and_hf_rows(path):
    variant, pi, dlduv, dldp, ref = load_golden(path, dtype=torch.float64)
    gn, gm, _ = _restated(path)
    truth = ref["ref64_param"].double()
    K = len(pi) - 1
    scale = _scale(ref)
    rows = 0
    for k in range(1, K + 1):
        for col, mine in ((3, gn[k - 1]), (4, gm[k - 1])):
            r = 5 * (k - 1) + col
            if r >= truth.shape[0]:                       # manifold_caustic: the last vertex has no n, m entries
                assert float(mine.abs().max()) == 0.0
                continue
            rel = (mine - truth[r]).abs().amax(dim=1) / scale
            assert float(rel.max()) < 1e-7, (k, col, float(rel.max()))
            assert torch.equal(mine == 0, truth[r] == 0), (k, col)
            rows += 1
    assert rows >= 2 * (K - 1)


@pytest.mark.parametrize("path", FILES, ids=golden_id)
def test_core_f64_eta_column_matches_the_restatement(path):
    variant, pi, dlduv, dldp, ref = load_golden(path, dtype=torch.float64)
    _, _, geta = _restated(path)
    want = torch.stack(geta)                                                   # (K,N)
    fp, _, _, got = host_ior_calc_grad(variant, pi, dlduv, dldp, dtype=torch.float64)
    assert not torch.isnan(got).any()
    scale = _scale(ref)
    rel = (got - want).abs().amax(dim=0) / scale
    print(golden_id(path), "max |geta|", float(want.abs().max()), "max rel", float(rel.max()), "paths with an eta term", int((want != 0).any(dim=0).sum()))
    assert float(rel.max()) < 1e-7, float(rel.max())
    assert torch.equal(got == 0, want == 0)
    # ... and on the eta column's own scale, where a path has one
    own = want.abs().amax(dim=0)
    has = own > 0
    if bool(has.any()):
        assert float(((got - want).abs().amax(dim=0)[has] / own[has]).max()) < 1e-6


@pytest.mark.parametrize("path", FILES, ids=golden_id)
def test_core_f32_eta_column_inside_the_conditioning_gate(path):
    variant, pi, dlduv, dldp, ref = load_golden(path, dtype=torch.float32)
    _, _, geta = _restated(path)
    want = torch.stack(geta)
    _, _, _, got = host_ior_calc_grad(variant, pi, dlduv, dldp, dtype=torch.float32)
    cond = oracle_cond(variant, pi, dlduv, dldp)
    three = lambda t: torch.stack([t.double(), torch.zeros_like(t, dtype=torch.float64), torch.zeros_like(t, dtype=torch.float64)], dim=-1)
    rep = gated_parity_report(three(got), three(want), cond)
    print(golden_id(path), rep)
    assert rep["n_bad_inside"] <= max(1, int(0.005 * want.shape[1])), rep
