"""Table of the HBM-bound row kernels (openp5_amd/csrc/p5_elem.h) and the embedding gradient (openp5_amd/csrc/p5_embed.h): one row per kernel
and edge, shared by the emulator tests (tests/test_elem_ref_emu.py) and the GPU tests (tests/test_gpu_elem_ref.py) of cases.rmsnorm_ref_case,
cases.ce_ref_case, cases.masked_mean_ref_case, cases.embed_fwd_ref_case, cases.embed_ref_case and cases.adamw_ref_case.  tests/test_static.py
checks that every launch in p5_lib.hip of a kernel these two headers define is named in KERNELS.

Bounds (cases.py): |got - ref| <= r |ref| + s S per element, S = the float64 expression with every term replaced by its absolute value.
  r   unit roundoff of the stored type, once per rounding the kernel's comments name: cases.GEMM_R (2^-8, bf16), ELEM_R32 = 2^-24 (fp32)
  s   the accumulation constant.  None was chosen from a kernel's error: each is a constant cases.py already holds for the same arithmetic,
      taken as it is (no margin on top).  For the record, the reference-side measurement -- a plain fp32 torch implementation of the same
      formula against float64, worst err / S over the table's rows -- is given with each:
        rmsnorm   cases.GEMM_S = 2^-16 (1.5e-5): fp32 sums of squares / of products over a row (d <= 1024) and over rows (dw), a GEMM's K
                  loop.  Measured: y 3.0e-7 of |ref|, dx 3.1e-7, dw 1.9e-7 of S (x 4 = 1.2e-6: GEMM_S is 12 x that)
        ce        cases.ATTN_TAU[0] = 1e-5: fp32 max / sum of exp / log, the attention kernels' softmax arithmetic.  Measured: lse 1.1e-7 of S
                  = |max| + |log sum| (x 4 = 4.4e-7); the bf16 mode's fast exponential adds |x| 2^-24 <= 5.2e-6 for x in [-87, 0]
        masked    cases.GEMM_S: fp32 sums over T and B
        embed fwd no accumulation: five fp32 roundings (p, 1 - p, its reciprocal, the add, the multiply), 5 ELEM_R32 S; the row's sums of
                  squares per 64 columns cases.GEMM_S
        embed bwd cases.GEMM_S: fp32 sums over the rows of a key, both modes.  Measured: 8704 rows of one key added one by one, 1.1e-7 of S
        adamw     2e-6 of each tensor's largest |ref| (cases.adamw_golden_case's bound against its fp64 fixture); sum of squares cases.GEMM_S
  results whose float64 value lies below the smallest normal fp32 number may flush to zero: ELEM_TINY = 2^-126 (times |g|) is added to the
  bound of the cross-entropy gradient, whose softmax terms reach exp(-200).

A row is a dict with `id`, `fam`, `gpu_only` (too large for the emulator) and the family's own fields (see the builders below).
"""

ELEM_R32 = 2.0 ** -24
ELEM_TINY = 2.0 ** -126

# kernel -> the family of rows that runs it here, or `checked_by`: the existing test that reaches it (None: no test does)
KERNELS = {
    "p5_rmsnorm_fwd_kernel": dict(fam="rmsnorm"),
    "p5_rmsnorm_bwd_kernel": dict(fam="rmsnorm"),
    "p5_reduce_rows_kernel": dict(fam="rmsnorm"),            # the partial-sum mode of the norm-weight gradient
    "p5_ce_fwd_kernel": dict(fam="ce"),                      # <float> and <bf16> (the fast exponential) through p5_op_ce_fwd_t
    "p5_ce_bwd_kernel": dict(fam="ce"),
    "p5_ce_gscale_kernel": dict(fam="ce"),
    "p5_masked_mean_kernel": dict(fam="masked"),
    "p5_embed_fwd_kernel": dict(fam="embed_fwd"),
    "p5_embed_bwd_kernel": dict(fam="embed"),
    "p5_embed_sortchunk_kernel": dict(fam="embed"),
    "p5_embed_rank_kernel": dict(fam="embed"),
    "p5_embed_seg_kernel": dict(fam="embed"),
    "p5_embed_fix_kernel": dict(fam="embed"),
    "p5_sumsq_kernel": dict(fam="adamw"),
    "p5_adamw_kernel": dict(fam="adamw"),
    # no row here
    "p5_cast_mask_kernel": dict(checked_by="tests/test_emu_kernels.py::test_model_fp32_dropout (whole-model gradients only)"),
    "p5_reduce_splits_kernel": dict(checked_by="tests/test_emu_kernels.py::test_model_bf16 (whole-model gradients only)"),
    "p5_reduce_rows_multi_kernel": dict(checked_by="tests/test_emu_kernels.py::test_model_bf16 (whole-model gradients only)"),
    "p5_reduce_copies_kernel": dict(checked_by=None),        # not launched by p5_lib.hip
    "p5_cast_kernel": dict(checked_by="tests/test_emu_kernels.py::test_model_bf16 (p5_refresh_shadow; whole model only)"),
    "p5_gated_gelu_fwd_kernel": dict(checked_by="tests/test_emu_kernels.py::test_model_gated (whole model only)"),
    "p5_gated_gelu_bwd_kernel": dict(checked_by="tests/test_emu_kernels.py::test_model_gated (whole model only)"),
    "p5_ce_finish_kernel": dict(checked_by="cases.ce_free_case (tests/test_emu_kernels.py, against the materialised-logits path)"),
}


def _r(fam, id, gpu_only=False, **kw):
    return dict(fam=fam, id=id, gpu_only=gpu_only, **kw)


# ---- T5LayerNorm ---------------------------------------------------------------------------------------------------------------------
# dtype 0 fp32 / 1 bf16; rows, d; dres (incoming residual gradient given); drop_y / drop_in / drop_next (p, 0 = off); ssq (the backward takes
# the statistic as d / 64 partial sums per row and writes n_out); edge (row 0 all zero, 1 of magnitude 1e4, 2 of magnitude 1e-4, 3 a single
# non-zero element, where the row count allows); error (the launcher must refuse and write nothing); opts (p5_set_option values, restored
# afterwards).  Every row runs the forward, and the backward with dw by atomics and by per-workgroup partials.
# The backward's grid is capped at 1024 workgroups of 4 rows, so its grid-stride loop and the second row a wave keeps in flight (RU = 2 of
# the NCH <= 2 instances) start at 4097 rows, 1 - 2 s per row in the emulator; LOW_BLOCKS lowers the cap to 64 workgroups (256 rows per
# pass) so that the emulator reaches both at 257 and 513 rows.  The rows of 4096 and more run at the default cap on the GPU.
LOW_BLOCKS = {"norm_bwd_blocks": 64}


def _rmsnorm_rows():
    R = []
    for dtype, nm in ((0, "fp32"), (1, "bf16")):
        epf = 8 if dtype else 4

        def row(rows, d, tag="", **kw):
            base = dict(dtype=dtype, rows=rows, d=d, dres=True, drop_y=0.0, drop_in=0.0, drop_next=0.0, ssq=False, edge=rows >= 5, error=False, opts={})
            base.update(kw)
            go = base.pop("gpu_only", False)
            return _r("rmsnorm", f"rmsnorm-{nm}-{rows}x{d}{tag}", gpu_only=go, **base)
        for d in (epf, 64, 128, 320, 512, 768, 1000, 1024):        # 768: fp32 NCH = 4 with three pieces, bf16 NCH = 2 with half-idle lanes
            R.append(row(5, d))
        for rows in (1, 3, 4, 4096, 4097, 8193):                    # above 4096 rows the grid (capped at 1024 workgroups) strides
            R.append(row(rows, 512, gpu_only=rows > 4))
        R.append(row(4097, 768, gpu_only=True))
        R.append(row(4097, 128, "-nodres", dres=False, gpu_only=True))
        for rows, d in ((256, 512), (257, 512), (513, 768), (600, 128)):        # one pass exactly; a second row in flight; a second loop iteration (RU = 1: a third)
            R.append(row(rows, d, "-blocks64", opts=LOW_BLOCKS, gpu_only=rows == 600))
        R.append(row(5, 512, "-nodres", dres=False))
        R.append(row(37, 512, "-dropy", drop_y=0.1))
        R.append(row(37, 512, "-dropin", drop_in=0.1))
        R.append(row(37, 512, "-dropnext", drop_next=0.1))
        R.append(row(37, 768, "-dropall", drop_y=0.1, drop_in=0.1, drop_next=0.1))
        for nt in (2, 4, 5, 12):                                    # (d / 64) & 3 == 0: the vector branch of the partial sums
            R.append(row(9, nt * 64, "-ssq", ssq=True))
        R.append(row(4097, 256, "-ssq-dropnext", ssq=True, drop_next=0.1, gpu_only=True))
        R.append(row(3, 1032, "-refused", error=True))
        if dtype:
            R.append(row(3, 12, "-refused", error=True))
        R.append(row(8193, 1024, gpu_only=True))
        R.append(row(32768, 1024, "-dropnext", drop_next=0.1, gpu_only=True))     # T5-large at L = 512
    return R


# ---- cross-entropy --------------------------------------------------------------------------------------------------------------------
# V, pad (ldl = V rounded up to 64, plus pad).  Every row is one [18, ldl] logit matrix: six kinds of rows (N(0, 1); N(0, 1) + 1e4; constant;
# one dominant logit, gap 200; some entries -inf; the first min(1024, V - 1) entries -inf) x three labels (-100, first finite column, V - 1),
# padding columns NaN.  Forward <float> and <bf16>; backward fp32 and bf16 x g from dnll / from the mask x gridDim.y 1, 4, 8.
CE = [_r("ce", f"ce-V{V}-pad{pad}", V=V, pad=pad, gpu_only=(V, pad) == (32100, 64))
      for V, pad in ((1, 0), (3, 64), (4, 0), (5, 64), (255, 0), (1027, 64), (1027, 0), (32100, 0), (32100, 64))]
MASKED = [_r("masked", f"masked-mean-{B}x{T}", B=B, T=T) for B, T in ((1, 1), (1, 64), (255, 5), (256, 64), (257, 5), (600, 1), (600, 64))]


# ---- embedding lookup -----------------------------------------------------------------------------------------------------------------
def _embed_fwd_rows():
    R = []
    for dtype, nm in ((0, "fp32"), (1, "bf16")):
        for rows, d, ww, drop, ssq in ((1, 64, True, 0.1, True), (5, 512, False, 0.0, True), (1027, 768, True, 0.1, True), (1027, 1024, True, 0.0, False),
                                       (5, 1024, False, 0.1, True), (1027, 64, False, 0.1, False), (1, 768, False, 0.0, False), (5, 64, True, 0.0, True),
                                       (1027, 512, True, 0.1, True)):
            R.append(_r("embed_fwd", f"embed-fwd-{nm}-{rows}x{d}{'-ww' if ww else ''}{'-drop' if drop else ''}{'-ssq' if ssq else ''}", dtype=dtype,
                        rows=rows, d=d, ww=ww, drop=drop, ssq=ssq))
    return R


# ---- embedding gradient ---------------------------------------------------------------------------------------------------------------
# sets: one or two of (n, n0, pattern, drop0, drop1): n lookups of which the first n0 come from the first key array (n0 = n: one array,
# n0 = 0: only the second), patterns:
#   equal     one key (one segment through every block of 32 sorted positions)
#   distinct  every key once
#   pad70     70 % key 0, the rest random with repeats
#   blocks    segments laid out on the 32-position blocks: one ending exactly on a block boundary, then segments that start on the last
#             position of a block and span exactly 4, 5 and 9 blocks (3, 4 and 8 pieces for the fix-up kernel's four-at-a-time loop and its
#             remainder), distinct keys between them, the last key = the largest table row
# The table is pre-filled with random values; both modes (atomic scatter, fixed-order chain run twice) on every row.
def _embed_rows():
    R = []

    def row(id, d, sets, gpu_only=False):
        R.append(_r("embed", f"embed-bwd-{id}-d{d}", gpu_only=gpu_only, d=d, sets=sets))
    for n, pat in ((1, "equal"), (31, "distinct"), (32, "equal"), (33, "pad70"), (255, "distinct"), (256, "pad70"), (257, "equal")):
        row(f"{n}-{pat}", 64, [(n, n, pat, 0.0, 0.0)])
    row("33-equal", 768, [(33, 33, "equal", 0.0, 0.0)])
    row("257-distinct", 1024, [(257, 100, "distinct", 0.1, 0.0)])
    row("1027-blocks", 64, [(1027, 1027, "blocks", 0.0, 0.0)])
    row("1027-blocks-two-arrays", 768, [(1027, 500, "blocks", 0.1, 0.1)])
    row("1027-blocks-second-array", 512, [(1027, 0, "blocks", 0.0, 0.1)])
    row("4097-pad70", 512, [(4097, 4000, "pad70", 0.1, 0.1)])            # a 17th chunk: second LDS batch of the rank kernel
    row("4097-distinct", 64, [(4097, 4097, "distinct", 0.0, 0.0)])
    row("4097-equal", 64, [(4097, 1, "equal", 0.0, 0.0)])
    row("8704-pad70-two-sets", 768, [(8704, 8192, "pad70", 0.1, 0.1), (8192, 8192, "pad70", 0.1, 0.0)], gpu_only=True)      # the benchmark step's shape
    row("8704-equal", 1024, [(8704, 8192, "equal", 0.0, 0.0)], gpu_only=True)
    row("8704-pad70", 64, [(8704, 8192, "pad70", 0.0, 0.1)], gpu_only=True)
    row("two-sets-300-17", 512, [(300, 200, "pad70", 0.1, 0.1), (17, 17, "pad70", 0.1, 0.0)])      # the second shorter than one block
    row("two-sets-1027-31", 1024, [(1027, 1027, "blocks", 0.0, 0.0), (31, 0, "equal", 0.0, 0.0)])
    row("two-sets-257-257", 64, [(257, 1, "distinct", 0.0, 0.1), (257, 256, "blocks", 0.1, 0.0)])
    return R


# ---- clip + AdamW ---------------------------------------------------------------------------------------------------------------------
# n; factor (the gradient is scaled so that norm * grad_scale = max_norm * factor in float64: clip factor below / at / above 1); sumsq /
# shadow (False = NULL); grad_scale; zero (all-zero gradients); steps (consecutive step_t values, the moments carried).  The launches have a
# fixed grid (1024 / 2048 workgroups with barriers), 0.5 s per step in the emulator whatever n: it keeps n = 3.
def _adamw_rows():
    R = []

    def row(n, factor, tag="", sumsq=True, shadow=True, grad_scale=1.0, zero=False, steps=(1, 2, 3), gpu_only=False):
        R.append(_r("adamw", f"adamw-n{n}-f{factor:.7g}{tag}", gpu_only=gpu_only, n=n, factor=factor, sumsq=sumsq, shadow=shadow, grad_scale=grad_scale,
                    zero=zero, steps=steps))
    row(1, 0.5, steps=(1,), gpu_only=True)
    row(3, 1.0 - 2.0 ** -20, steps=(2,))
    row(4, 1.0 + 2.0 ** -20, steps=(1,), gpu_only=True)
    row(5, 40.0, gpu_only=True)
    row(1023, 40.0, "-gs128", grad_scale=1.0 / 128, gpu_only=True)
    row(1023, 0.5, "-gs128", grad_scale=1.0 / 128, gpu_only=True)
    row(1023, 40.0, "-nosumsq", sumsq=False, gpu_only=True)
    row(1023, 40.0, "-noshadow", shadow=False, gpu_only=True)
    row(1023, 1.0, "-zero", zero=True, gpu_only=True)
    row(4099, 1.0 + 2.0 ** -20, "-t100000", steps=(100000, 100001), gpu_only=True)
    row(2048 * 256 + 1, 40.0, gpu_only=True)                       # beyond one sweep of the update's grid
    row(60754432, 40.0, "-t5small", steps=(1,), gpu_only=True)     # the T5-small arena
    return R


RMSNORM = _rmsnorm_rows()
EMBED_FWD = _embed_fwd_rows()
EMBED = _embed_rows()
ADAMW = _adamw_rows()
ROWS = RMSNORM + CE + MASKED + EMBED_FWD + EMBED + ADAMW
# embedding rows whose chain is also run with the emulator's workgroups last-to-first (bit-identical table gradient)
EMBED_ORDER = ("embed-bwd-1027-blocks-two-arrays-d768", "embed-bwd-two-sets-300-17-d512", "embed-bwd-257-equal-d64")
