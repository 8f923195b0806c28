"""Attention kernels (csrc/p5_attn.h) on the MI355X against a float64 reference (cases.attn_ref_case): the whole shape matrix of
tests/attn_matrix.py (every kernel and template instance at both of its boundaries) crossed with the key-mask patterns and dropout, and
two cases at training scale (many workgroups, large keep indices)."""
import pytest

from oracle import t5_oracle as O
from tests import cases
from tests.attn_matrix import BF16, FP32, case_id, drop_variants, masks_of

pytestmark = pytest.mark.gpu


def _params():
    out = []
    for dtype, table in ((1, BF16), (0, FP32)):
        for mode, Lq, Lk, _fwd, _bwd in table:
            for mask in masks_of(mode):
                for drop_p, op_bits in drop_variants(dtype, Lk):
                    out.append((dtype, mode, Lq, Lk, mask, drop_p, op_bits))
    return [pytest.param(*p, id=case_id(*p)) for p in out]


@pytest.mark.parametrize("dtype,mode,Lq,Lk,mask,drop_p,op_bits", _params())
def test_gpu_attention_against_fp64(hip, dtype, mode, Lq, Lk, mask, drop_p, op_bits):
    cases.attn_ref_case(hip, dtype, 2, 3, Lq, Lk, mode, mask=mask, drop_p=drop_p, op_bits=op_bits)


@pytest.mark.parametrize("op_bits", [False, True])
def test_gpu_attention_training_scale_long(hip, op_bits):
    """B = 8, H = 16, L = 512 (the C5 encoder shape): 128 workgroups of the head-resident kernels, keep indices up to 2^25"""
    cases.attn_ref_case(hip, 1, 8, 16, 512, 512, "enc", mask="holes", drop_p=0.1, op_bits=op_bits, seed=2)


def test_gpu_attention_training_scale_short(hip):
    """B = 64, H = 8, L = 128 (the benchmark's encoder shape), dropout on, sample 0 dead: 512 workgroups of the fused kernels"""
    cases.attn_ref_case(hip, 1, 64, 8, 128, 128, "enc", mask="dead", drop_p=0.1, seed=1)


@pytest.mark.parametrize("mask,drop_p,L", [("dead", 0.1, 40), ("dead", 0.0, 128), ("one", 0.1, 17)])
def test_gpu_attention_row_sums_against_fp64(hip, mask, drop_p, L):
    cases.attn_ref_case(hip, 1, 2, 3, L, L, "enc", mask=mask, drop_p=drop_p, rowdot=True)
    cases.attn_rowdot_case(hip, 2, 3, L, mode="enc", mask=mask, drop_p=drop_p)


@pytest.mark.parametrize("dtype,L", [("fp32", 40), ("bf16", 40), ("fp32", 150), ("bf16", 150)])
def test_gpu_model_dead_sample(hip, dtype, L):
    tol = dict(loss_tol=2e-5, grad_tol=2e-4, drop_tol=1e-5) if dtype == "fp32" else dict(loss_tol=0.08, grad_tol=0.5, drop_tol=2.0 ** -6)
    cases.model_dead_sample_case(hip, O.T5Cfg.named("tiny"), 2, L, 5, dtype, **tol)
