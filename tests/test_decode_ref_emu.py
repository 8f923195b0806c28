"""The decode-step kernels (csrc/p5_decode2.h: skinny GEMM, T5LayerNorm of the fp32 stream, self- and cross-attention, streaming head; the two
row-scoring kernels of csrc/p5_decode.h) on the host emulation against float64 references (decode_cases.decode_ref_case): every row of
tests/decode_matrix.py the emulator can afford."""
import pytest

from tests import decode_cases
from tests.decode_matrix import ROWS


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS if not r["gpu_only"]])
def test_decode_against_fp64(emu, row):
    decode_cases.decode_ref_case(emu, row)
