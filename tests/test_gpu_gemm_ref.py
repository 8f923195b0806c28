"""GEMM family on the MI355X against a float64 reference (cases.gemm_ref_case): every row of tests/gemm_matrix.py, and training-scale shapes
of the T5-small benchmark step at default options.  Each call is bracketed by p5_profile_begin / p5_profile_end and must reach the launch
site and tag its row names, so a moved threshold fails here instead of silently testing another kernel."""
import pytest

from tests import cases
from tests.gemm_matrix import ROWS, TRAINING

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS if not r["checked_by"]])
def test_gpu_gemm_against_fp64(hip, row):
    cases.gemm_ref_case(hip, row)


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in TRAINING])
def test_gpu_gemm_training_scale(hip, row):
    cases.gemm_ref_case(hip, row, seed=1)
