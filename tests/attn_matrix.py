"""Shape matrix of the attention kernels (openp5_amd/csrc/p5_attn.h, selected by p5_attn_tu.hip): every kernel and template instance at
both of its boundaries, as (mode, Lq, Lk) with the forward and backward kernel each shape takes.  Shared by the emulator and the GPU
tests of cases.attn_ref_case."""

# bf16: (mode, Lq, Lk, forward kernel, backward kernel)
BF16 = [
    # forward whole-head p5_attn_fwd_wg_kernel (<4> for Lq <= 64, <8> above), Lq, Lk <= 128
    ("enc", 17, 17, "fwd_wg<4>", "bwd_fused"),
    ("enc", 64, 64, "fwd_wg<4>", "bwd_fused"),
    ("enc", 65, 65, "fwd_wg<8>", "bwd_fused"),
    ("enc", 128, 128, "fwd_wg<8>", "bwd_fused"),
    ("cross", 1, 1, "fwd_wg<4>", "bwd_small"),
    ("cross", 64, 128, "fwd_wg<4>", "bwd_fused"),
    ("cross", 128, 1, "fwd_wg<8>", "bwd_dq+dkv"),
    ("dec", 33, 33, "fwd_wg<4>", "bwd_fused"),
    ("dec", 100, 100, "fwd_wg<8>", "bwd_fused"),
    # forward head-resident p5_attn_fwd_head_kernel (<16> for Lk <= 256, <32> above), Lk > 128
    ("enc", 129, 129, "fwd_head<16>", "bwd_head dq<16> dkv<16>"),
    ("enc", 256, 256, "fwd_head<16>", "bwd_head dq<16> dkv<16>"),
    ("enc", 257, 257, "fwd_head<32>", "bwd_head dq<32> dkv<32>"),
    ("enc", 512, 512, "fwd_head<32>", "bwd_head dq<32> dkv<32>"),
    ("cross", 1, 129, "fwd_head<16>", "bwd_small"),
    ("cross", 16, 512, "fwd_head<32>", "bwd_small"),
    ("cross", 300, 200, "fwd_head<16>", "bwd_head dq<16> dkv<32>"),
    ("dec", 200, 200, "fwd_head<16>", "bwd_head dq<16> dkv<16>"),
    ("dec", 300, 300, "fwd_head<32>", "bwd_head dq<32> dkv<32>"),
    ("dec", 257, 257, "fwd_head<32>", "bwd_head dq<32> dkv<32>"),
    # forward 64-query-block p5_attn_fwd_kernel in bf16: Lq > 128, Lk <= 128
    ("cross", 129, 128, "fwd_blocked<8>", "bwd_head dq<16> dkv<16>"),
    ("cross", 300, 70, "fwd_blocked<8>", "bwd_head dq<16> dkv<32>"),
    ("cross", 512, 1, "fwd_blocked<4>", "bwd_head dq<16> dkv<32>"),
    ("cross", 300, 1, "fwd_blocked<4>", "bwd_head dq<16> dkv<32>"),
    ("cross", 512, 128, "fwd_blocked<8>", "bwd_head dq<16> dkv<32>"),
    # backward p5_attn_bwd_small_kernel: Lq <= 16
    ("dec", 1, 1, "fwd_wg<4>", "bwd_small"),
    ("dec", 16, 16, "fwd_wg<4>", "bwd_small"),
    ("enc", 16, 16, "fwd_wg<4>", "bwd_small"),
    ("cross", 8, 300, "fwd_head<32>", "bwd_small"),
    # backward p5_attn_bwd_fused_kernel: 16 < Lq, Lk <= 128
    ("dec", 64, 64, "fwd_wg<4>", "bwd_fused"),
    ("dec", 65, 65, "fwd_wg<8>", "bwd_fused"),
    ("cross", 17, 128, "fwd_wg<4>", "bwd_fused"),
    ("cross", 128, 17, "fwd_wg<8>", "bwd_fused"),
    # backward p5_attn_bwd_dq_kernel + p5_attn_bwd_dkv_kernel in bf16: 16 < Lq <= 128, Lk <= 16
    ("cross", 40, 8, "fwd_wg<4>", "bwd_dq+dkv"),
    # backward head-resident, asymmetric template choices (dq by Lk, dkv by Lq)
    ("cross", 17, 512, "fwd_head<32>", "bwd_head dq<32> dkv<16>"),
    ("cross", 200, 300, "fwd_head<32>", "bwd_head dq<32> dkv<16>"),
]

# fp32: every NKT instance of p5_attn_fwd_kernel (Lk <= 64, 128, 256, 512), the small backward and the dq + dkv pair
FP32 = [
    ("enc", 17, 17, "fwd_blocked<4>", "bwd_dq+dkv"),
    ("enc", 65, 65, "fwd_blocked<8>", "bwd_dq+dkv"),
    ("cross", 1, 1, "fwd_blocked<4>", "bwd_small"),
    ("cross", 128, 1, "fwd_blocked<4>", "bwd_dq+dkv"),
    ("enc", 129, 129, "fwd_blocked<16>", "bwd_dq+dkv"),
    ("enc", 257, 257, "fwd_blocked<32>", "bwd_dq+dkv"),
    ("cross", 16, 512, "fwd_blocked<32>", "bwd_small"),
    ("cross", 300, 70, "fwd_blocked<8>", "bwd_dq+dkv"),
    ("dec", 16, 16, "fwd_blocked<4>", "bwd_small"),
    ("dec", 100, 100, "fwd_blocked<8>", "bwd_dq+dkv"),
    ("dec", 300, 300, "fwd_blocked<32>", "bwd_dq+dkv"),
]

MASKS = ("full", "suffix", "one", "holes", "dead")


def masks_of(mode):
    return ("none",) if mode == "dec" else MASKS


def drop_variants(dtype, Lk):
    """(drop_p, op_bits): off, on, and for the bf16 long-sequence kernels on with the forward's stored keep masks"""
    v = [(0.0, False), (0.1, False)]
    if dtype == 1 and Lk > 128:
        v.append((0.1, True))
    return v


def case_id(dtype, mode, Lq, Lk, mask, drop_p, op_bits):
    return f"{'bf16' if dtype else 'fp32'}-{mode}-{Lq}x{Lk}-{mask}-p{drop_p}{'-bits' if op_bits else ''}"
