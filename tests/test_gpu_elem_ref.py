"""Row kernels (csrc/p5_elem.h) and the embedding gradient (csrc/p5_embed.h) on the MI355X against float64 references: every row of
tests/elem_matrix.py, the shapes the emulator cannot afford included (32768 x 1024 norm rows, the 60.8 M element arena of T5-small, the
benchmark step's 8704 + 8192 lookups)."""
import pytest

from tests import cases
from tests.elem_matrix import ROWS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS])
def test_gpu_elem_against_fp64(hip, row):
    cases.elem_ref_case(hip, row)
