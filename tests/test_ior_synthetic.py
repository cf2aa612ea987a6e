"""The synthetic cases of test_gpu_ior_backward.py, looked at on the CPU: the reference ``alpha`` buffer under EPSM_OPT_IOR_GRADS
is not trivial, differs from the buffer without the option exactly on the slots that receive a refraction, and the allowance of
the GPU test's yardstick -- components within 2 % of the clamp, twice the float32 core's distance from the float64 core -- stays
below a tenth of the reference's magnitude for the seeds chosen in tests/_ior_cases.py."""
import pytest
import torch

from _ior_cases import B, KS, N_LARGE, N_RAGGED, N_REPLICAS, PROFILES, QUIET_SLOT, case, reference


@pytest.mark.parametrize("N,listed", [(N_RAGGED, False), (N_REPLICAS, False), (N_LARGE, False), (N_REPLICAS, True), (N_LARGE, True)])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("variant,profile", PROFILES)
def test_the_allowance_of_the_synthetic_cases_stays_small(variant, profile, K, N, listed):
    alpha, allow, refracted, plain = reference(variant, profile, K, N, listed)
    m = float(alpha.abs().max())
    print(variant, profile, K, N, listed, "max |alpha|", m, "allowance / m", float(allow.max()) / max(m, 1e-300), "refracted", refracted.tolist())
    assert bool(torch.isfinite(alpha).all())
    assert not bool(refracted[QUIET_SLOT])
    # a slot without a refraction is what it is without the option, to the last bit of the float64 sum
    assert torch.equal(alpha[~refracted], plain[~refracted])
    # `manifold` on `pool` paths: a diffuse first hit ends every chain; `manifold_caustic` needs a vertex behind the first refraction
    if (variant, profile) == ("manifold", "pool") or (variant == "manifold_caustic" and K < 3):
        assert m == 0.0 and float(allow.max()) == 0.0
        return
    assert m > 0
    assert float(allow.max()) < 0.1 * m, (float(allow.max()), m)
    # the option matters: on the slots with refractions the two buffers are far apart
    if N >= N_LARGE and not listed and K >= 3:
        assert float((alpha - plain).abs().max()) > 1e-2 * m


def test_the_quiet_slot_holds_reflections_only():
    c = case("manifold_caustic", "pool", 5, N_LARGE)
    tr = c["trace"]
    for k in range(1, 6):
        on_slot = tr.scatter_info[k - 1]["aux"][:, 0] == QUIET_SLOT
        assert int(on_slot.sum()) > 0 and bool((tr.path_info[k]["eta"][on_slot] == 1.0).all())
    assert any(bool((tr.path_info[k]["eta"] != 1.0).any()) for k in range(1, 6)) and B > 1
