"""The catalogue-ranking kernels (csrc/p5_rank.h, p5_cand.h, p5_prune.h, p5_bound.h and the p5_tree_attn_row body of p5_verify.h) on the host
emulation against exact restatements and float64 references (rank_kernel_cases.rank_ref_case): every row of tests/rank_matrix.py the emulator
can afford."""
import pytest

from tests import rank_kernel_cases
from tests.rank_matrix import ROWS


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS if not r["gpu_only"]])
def test_rank_against_reference(emu, row):
    rank_kernel_cases.rank_ref_case(emu, row)
