"""Attention kernels (csrc/p5_attn.h) on the host emulation against a float64 reference (cases.attn_ref_case): every forward and backward
kernel and template instance with every key-mask pattern (full, suffix, one valid key, holes, one dead sample), dropout off and on, the
long-sequence kernels with and without the forward's stored keep masks.  A subset of the GPU matrix (test_gpu_attention_ref.py) sized for
the emulator; tests/attn_matrix.py lists which kernels each shape takes."""
import pytest

from oracle import t5_oracle as O
from tests import cases
from tests.attn_matrix import MASKS, case_id

# (dtype, mode, Lq, Lk): at least one shape per (forward kernel, backward kernel) pair of attn_matrix, the cheaper end of each range
SHAPES = [
    (1, "enc", 17, 17),        # fwd_wg<4>, bwd_fused
    (1, "cross", 128, 17),     # fwd_wg<8>, bwd_fused
    (1, "cross", 1, 1),        # fwd_wg<4>, bwd_small
    (1, "enc", 16, 16),        # fwd_wg<4>, bwd_small (relative bias)
    (1, "cross", 8, 300),      # fwd_head<32>, bwd_small
    (1, "cross", 40, 8),       # fwd_wg<4>, bf16 bwd_dq + bwd_dkv
    (1, "cross", 128, 1),      # fwd_wg<8>, bf16 bwd_dq + bwd_dkv
    (1, "enc", 129, 129),      # fwd_head<16>, bwd_head dq<16> dkv<16>
    (1, "enc", 257, 257),      # fwd_head<32>, bwd_head dq<32> dkv<32>
    (1, "cross", 17, 512),     # fwd_head<32>, bwd_head dq<32> dkv<16>
    (1, "cross", 300, 70),     # fwd_blocked<8>, bwd_head dq<16> dkv<32>
    (1, "cross", 300, 1),      # fwd_blocked<4>, bwd_head dq<16> dkv<32>
    (0, "enc", 17, 17),        # fp32 fwd<4>, bwd_dq + bwd_dkv
    (0, "enc", 65, 65),        # fp32 fwd<8>
    (0, "cross", 16, 512),     # fp32 fwd<32>, bwd_small
    (0, "enc", 129, 129),      # fp32 fwd<16>
]
DEC = [(1, 1), (1, 16), (1, 33), (1, 65), (1, 200), (1, 257), (0, 16), (0, 100)]      # (dtype, L), causal: no key mask


def _params():
    out = []
    for dtype, mode, Lq, Lk in SHAPES:
        for mask in MASKS:
            out.append((dtype, mode, Lq, Lk, mask, 0.1, False))
        out.append((dtype, mode, Lq, Lk, "suffix", 0.0, False))
        out.append((dtype, mode, Lq, Lk, "dead", 0.0, False))
        if dtype == 1 and Lk > 128:
            out.append((dtype, mode, Lq, Lk, "holes", 0.1, True))
            out.append((dtype, mode, Lq, Lk, "dead", 0.1, True))
    for dtype, L in DEC:
        out.append((dtype, "dec", L, L, "none", 0.0, False))
        out.append((dtype, "dec", L, L, "none", 0.1, False))
        if dtype == 1 and L > 128:
            out.append((dtype, "dec", L, L, "none", 0.1, True))
    return [pytest.param(*p, id=case_id(*p)) for p in out]


@pytest.mark.parametrize("dtype,mode,Lq,Lk,mask,drop_p,op_bits", _params())
def test_attention_against_fp64(emu, dtype, mode, Lq, Lk, mask, drop_p, op_bits):
    cases.attn_ref_case(emu, dtype, 2, 2, Lq, Lk, mode, mask=mask, drop_p=drop_p, op_bits=op_bits)


@pytest.mark.parametrize("mask,drop_p", [("dead", 0.1), ("dead", 0.0), ("one", 0.1)])
def test_attention_row_sums_against_fp64(emu, mask, drop_p):
    """dot_out of the fused backward (the T5LayerNorm-backward epilogue's input) with dead rows: finite, exactly 0 on the dead sample"""
    cases.attn_ref_case(emu, 1, 2, 2, 40, 40, "enc", mask=mask, drop_p=drop_p, rowdot=True)
    cases.attn_rowdot_case(emu, 2, 2, 40, mode="enc", mask=mask, drop_p=drop_p)


@pytest.mark.parametrize("dtype,L", [("fp32", 20), ("bf16", 20), ("fp32", 130), ("bf16", 150)])
def test_model_dead_sample(emu, dtype, L):
    """a sample with an all-zero attention_mask and no label weight: loss and gradients finite, equal to the oracle's and to those of
    the batch without it"""
    tol = dict(loss_tol=2e-5, grad_tol=2e-4, drop_tol=1e-5) if dtype == "fp32" else dict(loss_tol=0.08, grad_tol=0.5, drop_tol=2.0 ** -6)
    cases.model_dead_sample_case(emu, O.T5Cfg.named("tiny"), 3, L, 5, dtype, **tol)
