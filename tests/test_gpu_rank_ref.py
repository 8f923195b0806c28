"""The catalogue-ranking kernels (csrc/p5_rank.h, p5_cand.h, p5_prune.h, p5_bound.h and the p5_tree_attn_row body of p5_verify.h) on the MI355X
against exact restatements and float64 references: every row of tests/rank_matrix.py, the selection over a million items included."""
import pytest

from tests import rank_kernel_cases
from tests.rank_matrix import ROWS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS])
def test_gpu_rank_against_reference(hip, row):
    rank_kernel_cases.rank_ref_case(hip, row)
