"""tests/test_color_replays.py on the GPU, with all five replay kinds: the ball scene plus a small `roughconductor` plate whose
alpha is a 4 x 4 bitmap (Scene.attach_texture('plate.bsdf.alpha.data')).  1600 paths: 12.5 workgroups of 128, and with
tile_paths = 512 four tiles, the last one of 64 paths."""
import pytest

from test_color_replays import HOST_KINDS, TILINGS, TRANSPOSE, check_combined_equals_separate, check_combined_transpose

pytestmark = pytest.mark.gpu

ALL_KINDS = HOST_KINDS + ("alpha_texture",)
# Measured on the parent commit on the MI355X, as a share of the section's largest element, over both tilings and both texel
# kinds (MEASUREMENTS.md 30): two identical calls 6.05e-7, combined against alone 2.02e-7.  8 times the larger.
TEXEL_SPREAD_DEVICE = 8 * 6.05e-7


@pytest.mark.parametrize("tile", TILINGS)
def test_combined_call_equals_the_separate_calls(tile):
    """As on the host: alpha, conductor, env_pose and colour bit for bit (the parent commit does on the device too), the envmap's
    and the roughness map's texels within TEXEL_SPREAD_DEVICE."""
    check_combined_equals_separate(ALL_KINDS, tile, TEXEL_SPREAD_DEVICE, device="cuda", with_plate=True)


@pytest.mark.parametrize("integ_name", TRANSPOSE)
@pytest.mark.parametrize("depth", [2, 4])
def test_combined_forward_is_the_transpose_of_backward(integ_name, depth):
    """`prb_reparam` with geometry attached refuses a scene that has a roughness map (the term through the map's uv derivative is
    not differentiated), so its two cases run the four kinds of the host test on the scene without the plate."""
    plate = integ_name != "prb_reparam"
    check_combined_transpose(integ_name, depth, ALL_KINDS if plate else HOST_KINDS, device="cuda", with_plate=plate)
