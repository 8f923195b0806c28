"""The decode-step kernels (csrc/p5_decode2.h and the row-scoring kernels of csrc/p5_decode.h) on the MI355X against float64 references:
every row of tests/decode_matrix.py, the headline head shape (200 rows x 32100 tokens) included."""
import pytest

from tests import decode_cases
from tests.decode_matrix import ROWS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS])
def test_gpu_decode_against_fp64(hip, row):
    decode_cases.decode_ref_case(hip, row)
