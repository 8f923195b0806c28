"""GEMM family (csrc/p5_gemm*.h, the decode step's skinny kernels in p5_decode2.h) on the host emulation against a float64 reference
(cases.gemm_ref_case): every row of tests/gemm_matrix.py -- each launch route at the edges of its conditions, under options that lower the
routes' size thresholds -- with NaN operand padding, sentinel guard bands around C, dropout's keep set and exact zeros.  The emulation keeps
the in-run profiler's launch record, so every row also checks which launch site and tag it reached."""
import pytest

from tests import cases
from tests.gemm_matrix import ROWS


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS if not r["gpu_only"] and not r["checked_by"]])
def test_gemm_against_fp64(emu, row):
    cases.gemm_ref_case(emu, row)


def test_gemm_k_tail_padding_is_not_read(emu):
    """K % 8 (bf16) / K % 4 (fp32) != 0 with lda, ldb padded to the next 16 bytes (the contract of p5_op_gemm, include/p5hip.h): the
    padding elements hold 1.0 instead of NaN and must not be multiplied in either."""
    import torch
    for dtype, K in ((1, 50), (0, 50), (2, 50), (1, 3), (0, 7)):
        tt = torch.bfloat16 if dtype == 1 else torch.float32
        epf = 8 if dtype == 1 else 4
        ld = (K + epf - 1) // epf * epf
        g = torch.Generator().manual_seed(K)
        A = torch.ones(70, ld, dtype=tt)
        B = torch.ones(40, ld, dtype=tt)
        A[:, :K] = torch.randn(70, K, generator=g).to(tt)
        B[:, :K] = torch.randn(40, K, generator=g).to(tt)
        ref = A[:, :K].double() @ B[:, :K].double().t()
        C = torch.zeros(70, 40, dtype=torch.float32 if dtype != 1 else tt)
        emu.check(emu.lib.p5_op_gemm(dtype, cases.P(A), cases.P(B), cases.P(C), None, 70, 40, K, ld, ld, 40, 0, 0, 0, 0, 0, 1, 1.0, None, 0, 0.0,
                                     emu.stream_ptr()), "gemm")
        S = A[:, :K].double().abs() @ B[:, :K].double().abs().t()
        bound = cases.GEMM_R[dtype == 1] * ref.abs() + cases.GEMM_S * S
        assert bool(((C.double() - ref).abs() <= bound).all()), f"dtype {dtype} K {K}: the padding of the last 16 bytes was multiplied in"
