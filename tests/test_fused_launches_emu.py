"""Options shift_fuse and loss_fuse on the host emulation: off against on the same gradient bits, whole and staged backward, and the merged
loss kernel against the two it replaces (tests/fused_launch_cases.py); GPU twin: tests/test_gpu_fused_launches.py."""
import pytest

from tests.fused_launch_cases import LOSS_SHAPES, OPTIONS, SHAPES, merged_loss_case, option_case


@pytest.mark.parametrize("staged", [False, True], ids=["whole", "staged"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_L%d_T%d" % s)
@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_option_off_equals_on(emu, name, shape, staged):
    option_case(emu, name, shape, staged)


@pytest.mark.parametrize("B,T,G", LOSS_SHAPES)
def test_merged_loss_kernel(emu, B, T, G):
    merged_loss_case(emu, B, T, G)
