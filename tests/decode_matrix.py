"""Table of the decode-step kernels (openp5_amd/csrc/p5_decode2.h and the two row-scoring kernels of p5_decode.h): one row per kernel
instance and edge, shared by the emulator tests (tests/test_decode_ref_emu.py) and the GPU tests (tests/test_gpu_decode_ref.py) of
decode_cases.decode_ref_case.  Every kernel is reached through the launcher the engine itself uses (p5_op_skinny_gemm,
p5_op_rmsnorm_f32in, p5_op_dec_self_attn, p5_op_dec_cross_attn_ex, p5_op_head_lse, p5_op_dec_score).  tests/test_static.py checks that
every kernel of p5_decode.h, p5_decode2.h, p5_decode_wide.h and p5_verify.h that p5_lib.hip launches is named in KERNELS.

Every case builds its inputs on the CPU in the stored types, runs the op with its outputs inside NaN-pattern guards (cases.GEMM_SENT) and
compares with a float64 evaluation of the same formula on the same stored inputs, reproducing the roundings the kernels' comments name (the
normalised row is rounded to T before the weight multiply and the product again; the fused cross-attention rounds q to T).

Bounds: |got - ref| <= r |ref| + s S per element, S = the float64 expression with every term replaced by its absolute value.  No constant
was chosen from a kernel's error; each is one cases.py / elem_matrix.py already holds for the same arithmetic, with no margin on top:
  r        cases.GEMM_R = 2^-8 once per bf16 rounding the kernel's comments name, ELEM_R32 = 2^-24 per fp32 rounding
  GEMM_S   2^-16: fp32 dot products and sums of squares
  TAU      cases.ATTN_TAU[0] = 1e-5: fp32 max / sum of exp / log / divide, relative to |max| + |log sum| (log-sum-exp) or to S (softmax P V)
per family:
  skinny     T out: r |ref| + GEMM_S S; fp32 out: ELEM_R32 |ref| + GEMM_S S; S = |alpha| sum_k |a_k w_k| (+ |C0| for the += epilogues).
             amode 1 (a = T(ln * T(x rstd))): + (2 r + GEMM_S) S -- the two named roundings of a may each fall the other way than the float64
             reference's (rstd is fp32), and rstd carries a sum of squares.  An all-zero x row gives exactly 0 (exactly C0 for +=).
  rmsnorm    (2 r + GEMM_S) |ref|, the bound cases.rmsnorm_ref_case holds p5_rmsnorm_fwd_kernel's y to (same formula, same roundings)
  self_attn  scores s_j = q . k_j + bias_j are off by at most e = GEMM_S max_j (sum_d |q_d k_jd| + |bias_j|); scores moved by <= e move every
  cross_attn probability by a factor within exp(+-2 e), so O = sum_j p_j v_j by at most 2 e S with S = sum_j p_j |v_j|; the fp32 softmax arithmetic
             adds TAU S and the fp32 P V sum GEMM_S S; the stored output r |ref|:   r |ref| + (2 e + TAU + GEMM_S) S.  The matrix-core
             kernel keeps P in bf16 as hi + lo (16 mantissa bits, its comment): one more GEMM_S S.  A dead item (no valid key) gives O = 0
             exactly (cases.attn_ref64's convention).  Fused q: q is rounded to bf16 from an fp32 accumulator, so an element may round the
             other way than the reference's; that moves a score by at most e_q = GEMM_R sum_d |q_d k_jd| and O by at most
             2 max_j e_q max |V| (|p'_j - p_j| summed over j is at most exp(2 e_q) - 1), added to the bound.  The rows scale Wq so that
             this bound stays below a tenth of the largest |ref| of the row; the case asserts that condition on its inputs.  It asserts
             too, on the CPU and from float64 references alone, that what only the fused kernels do shows in O: with q = 0, with the
             T5LayerNorm weight left out, with the second half of the projection's K range left out and with the next head's slice of
             Wq, O moves by more than 2 bounds (beyond which a kernel with that mistake fails for certain: its own error is within one)
             on every row of x that is not zero and has two valid keys or more, and by 8 on some row.  For that the fused rows' K is
             sparse (+-1 in four dimensions), their keys repeat 16 (K, sign of V) pairs per (item, head), |V| is in [0.75, 1] and |ln|
             in [0.5, 2] with either sign (decode_cases.cross_attn_ref_case); measured there: 9.6 bounds at the least, 39 at the most.
  head_lse   logits l = alpha h . e are off by at most e_l = GEMM_S alpha sum |h e| + ELEM_R32 |l| (largest over the tile's columns):
             part_m: e_l; part_m + log(part_s): e_l + TAU (|max| + |log sum|), in bf16 + 2^-24 max_j min(|l_j - max|, 88) for the fast exponential
             (elem_matrix.py records the same term for the bf16 cross-entropy)
  score      score = (logit - lse) + run_score: the logit's e_l (streaming; the materialised logits are inputs), TAU (|max| + |log sum|) for
             the log-sum-exp, 3 ELEM_R32 (|logit| + |lse| + |run_score|) for the three fp32 operations.  Checked per decode row: n_top ==
             min(K2, finite candidates); every returned (score, child) within the bound of ref[child]; the list in (own score desc, child
             asc) order; every finite child left out has ref <= min(returned ref) + 2 bound; rows of bit-equal scores (`ties`): the child
             list exactly.  -inf logits are out of scope for p5_dec_score_kernel (its online sum would give NaN for a leading -inf; decode
             logits are GEMM outputs and cannot be -inf): no such row.

For the record only, not a source of tolerances: the reference-side measurement -- a plain fp32 torch implementation of the same formula
against float64 on the CPU, N(0, 1) fp32 inputs at the largest shape of each family, worst error as a fraction of the family's scale:
  skinny 6.0e-8 of S (200 x 40 x 2048), amode 1 1.2e-7 of S (K = 1024); rmsnorm 2.5e-7 of |ref| (200 x 1024); self_attn 3.9e-6 of S (480
  (row, head) pairs x 128 keys), cross_attn 4.9e-6 of S (612 x 512 keys) -- both include the fp32 scores; head_lse 4.3e-7 of |max| + |log sum|
  (200 x 1024, tiles of 64); score 2.7e-7 of |logit| + |lse| + |run_score|.

A row is a dict with `id`, `fam`, `gpu_only` (the emulator needs more than about 2 s) and the family's own fields (see the builders).
"""

ELEM_R32 = 2.0 ** -24

_BEAM = "tests/test_emu_kernels.py::test_generate, ::test_generate_forced_prefix_fast_forward (cases.generate_case: token-exact against the oracle; tests/test_gpu_parity.py::test_generate on the GPU)"
_WIDE = "tests/test_wide_beams_emu.py::test_wide_oracle_parity, tests/test_gpu_wide_beams.py::test_gpu_wide_oracle_parity (wide_cases: token-exact against the oracle)"
_VERIFY = "tests/test_emu_kernels.py::test_generate_verified, tests/test_gpu_parity.py::test_generate_verified (token-exact against the oracle)"

# kernel -> the family of rows that runs it here, or `checked_by`: the existing test that reaches it (None: no test does)
KERNELS = {
    "p5_skinny_gemm_kernel": dict(fam="skinny"),
    "p5_rmsnorm_f32in_kernel": dict(fam="rmsnorm"),
    "p5_dec_self_attn2_kernel": dict(fam="self_attn"),
    "p5_dec_cross_attn2_kernel": dict(fam="cross_attn"),
    "p5_dec_cross_attn3_kernel": dict(fam="cross_attn"),
    "p5_head_lse_kernel": dict(fam="head_lse"),
    "p5_dec_score2_kernel": dict(fam="score"),
    "p5_dec_score_kernel": dict(fam="score"),
    # beam bookkeeping: integer state machines, compared token by token with the oracle's beam search
    "p5_beam_step_kernel": dict(checked_by=_BEAM),
    "p5_beam_init_kernel": dict(checked_by=_BEAM),
    "p5_beam_forced_kernel": dict(checked_by=_BEAM),
    "p5_beam_finalize_kernel": dict(checked_by=_BEAM),
    "p5_ff_labels_kernel": dict(checked_by=_BEAM),
    "p5_ff_cache_kernel": dict(checked_by=_BEAM),
    "p5_wide_score_kernel": dict(checked_by=_WIDE),
    "p5_wide_score2_kernel": dict(checked_by=_WIDE),
    "p5_wide_select_kernel": dict(checked_by=_WIDE),
    "p5_wide_scorer_kernel": dict(checked_by=_WIDE),
    "p5_wide_commit_kernel": dict(checked_by=_WIDE),
    "p5_verify_plan_kernel": dict(checked_by=_VERIFY),
    "p5_verify_rows_kernel": dict(checked_by=_VERIFY),
    "p5_verify_forced_kernel": dict(checked_by=_VERIFY),
    "p5_verify_range_kernel": dict(checked_by=_VERIFY),
    "p5_verify_step_kernel": dict(checked_by=_VERIFY),
    # its per-row body (p5_tree_attn_row) is shared with exhaustive ranking: the rows of both against float64 are in the ranking table
    "p5_tree_attn_kernel": dict(checked_by="tests/rank_matrix.py, family tree_attn, variant 2 (tests/test_rank_ref_emu.py, tests/test_gpu_rank_ref.py); " + _VERIFY),
}


def _r(fam, id, gpu_only=False, **kw):
    return dict(fam=fam, id=id, gpu_only=gpu_only, **kw)


_NM = {0: "fp32", 1: "bf16"}
_EPS = {0: 32, 1: 64}        # K elements per 128-byte step (SkT<T>::EPS)


# ---- skinny GEMM ------------------------------------------------------------------------------------------------------------------------
# dtype, amode, M, N, K, epi (0 store T * alpha, 1 ReLU, 2 fp32 += by atomics over K splits, 3 store fp32 * alpha, 4 fp32 += by one writer
# over K passes), alpha, pad (elements added to the least lda, ldw, ldc; padding NaN), opts (p5_set_option, restored), inst = the
# <NB, AMODE, LDSKB> instance the profiler report must name, edge (amode 1, M >= 5: row 0 all zero, 1 of magnitude 1e4, 2 of magnitude 1e-4,
# 3 a single non-zero), error (the launcher must refuse and write nothing; word: what its message must say).
# LDS a tile needs: steps * (2048 + NB * 128) (+ 3072 below NB = 64), steps = K range / EPS; instances of 44 / 52 / 80 / 100 / 140 KiB.
_SK_LDS = (44, 52, 80, 100, 140)


def _sk_steps(nb, kb):
    """largest number of 128-byte K steps whose tile fits kb KiB at column width nb"""
    return (kb * 1024 - (3072 if nb < 64 else 0)) // (2048 + nb * 128)


def _skinny_rows():
    R = []

    def row(dtype, amode, M, N, K, epi, inst, tag="", alpha=1.0, pad=(0, 0, 0), opts=None, edge=False, error=False, word="skinny"):
        R.append(_r("skinny", f"skinny-{_NM[dtype]}-a{amode}-{M}x{N}x{K}-e{epi}{tag}", dtype=dtype, amode=amode, M=M, N=N, K=K, epi=epi, alpha=alpha,
                    pad=pad, opts=opts or {}, inst=inst, edge=edge and M >= 5, error=error, word=word))

    Ms = (1, 15, 16, 17, 200)
    for dtype in (0, 1):
        eps = _EPS[dtype]
        i = 0
        # every <NB, AMODE, LDSKB> at the largest K range that still fits it (odd i: the smallest that no longer fits the size below)
        for amode in (0, 1):
            for nb in (64, 32, 16):
                lo = 0
                for kb in _SK_LDS:
                    hi = _sk_steps(nb, kb)
                    steps = hi if i % 2 == 0 else lo + 1
                    lo = hi
                    if amode == 1 and steps * eps > 1024:
                        steps = 1024 // eps
                        if steps <= _sk_steps(nb, _SK_LDS[_SK_LDS.index(kb) - 1]):
                            continue                   # (bf16 rows of 1024 columns are 16 steps: NB 32 / 140 and NB 16 / 100, 140 cannot be reached)
                    M = Ms[i % 5]
                    N = (nb, nb * 2 + 1, max(nb // 4, 8), nb + 1)[i % 4]          # one tile; NB k + 1; N < NB (clamped W rows); NB + 1
                    epi = (0, 1, 3)[i % 3]
                    alpha = 0.75 if epi in (0, 3) and i % 2 else 1.0
                    pad = ((0, 0, 0), (8, 16, 8))[(i // 2) % 2]
                    row(dtype, amode, M, N, steps * eps, epi, (nb, amode, kb), tag=f"-nb{nb}-lds{kb}", alpha=alpha, pad=pad, opts={"dec_nb": nb},
                        edge=amode == 1)
                    i += 1
        # automatic selection.  amode 1: NB 64 while its tile fits 80 KiB, then 32 up to 100 KiB, then 16; d = EPS, 512, 768, 1024
        a1 = {0: ((32, (64, 1, 44)), (512, (32, 1, 100)), (768, (16, 1, 100)), (1024, (16, 1, 140))),
              1: ((64, (64, 1, 44)), (512, (64, 1, 80)), (768, (32, 1, 80)), (1024, (32, 1, 100)))}[dtype]
        for j, (d, inst) in enumerate(a1):
            row(dtype, 1, (17, 5, 200, 16)[j], (65, 16, 40, 129)[j], d, (0, 1, 0, 3)[j], inst, tag="-auto", pad=(0, 8, 8), edge=True)
        # amode 0, store: NB 64, the whole K up front.  K = EPS (one step: three of the four waves of an NB = 16 tile have no K part),
        # 2 EPS, 5 EPS (not a multiple of sk_mma's 4-step block), 512
        for K, kb in ((eps, 44), (2 * eps, 44), (5 * eps, 52), (512, 80 if dtype else 140)):
            if dtype == 0 and K == 512:
                continue          # (fp32: 16 steps x 10 KiB = 160 KiB, the refused row below)
            row(dtype, 0, 17, 65, K, 0, (64, 0, kb), tag="-auto", alpha=0.75, pad=(8, 8, 8))
        row(dtype, 0, 16, 16, eps, 1, (16, 0, 44), tag="-nb16-onestep", opts={"dec_nb": 16})
        row(dtype, 0, 15, 33, 5 * eps, 3, (16, 0, 44), tag="-nb16", alpha=0.75, opts={"dec_nb": 16})
        # += by one writer (epi 4): NB 32 while its tile fits 52 KiB, else 16; K walked in passes of at most 80 KiB
        row(dtype, 0, 17, 33, 8 * eps, 4, (32, 0, 52), tag="-onepass")
        row(dtype, 0, 200, 40, 2048, 4, (16, 0, 80), tag="-passes-even", pad=(8, 0, 8))       # d_ff: bf16 2 passes of 1024, fp32 4 of 512
        row(dtype, 0, 17, 17, 21 * eps, 4, (16, 0, 52), tag="-passes-short")                   # 21 steps halve to 11: passes of 11 and 10 steps
        row(dtype, 0, 5, 16, 1024, 4, (16, 0, 80) if dtype else (16, 0, 80), tag="-passes-1024")
        # += by atomics (epi 2): NB 64, K split over workgroups; few tiles: the range per workgroup halves down to 2 EPS
        row(dtype, 0, 17, 65, 512, 2, (64, 0, 44), tag="-splits")
        row(dtype, 0, 16, 64, 5 * eps, 2, (64, 0, 44), tag="-splits-short")                    # splits of 2, 2 and 1 steps
        row(dtype, 0, 1, 8, 2048, 2, (64, 0, 44), tag="-splits-2048", pad=(0, 8, 0))
        row(dtype, 0, 15, 129, 7 * eps, 2, (32, 0, 44), tag="-kw3-short", opts={"dec_nb": 32, "dec_kw": 3 * eps})      # splits of 3, 3 and 1 steps
        # refused, nothing written
        row(dtype, 0, 5, 16, eps + 8, 0, None, tag="-refused-K", error=True)
        row(dtype, 1, 5, 16, 1032, 0, None, tag="-refused-norm1032", error=True)                # (no multiple of EPS either: refused as the row above is)
        row(dtype, 1, 5, 16, 2048, 0, None, tag="-refused-norm2048", error=True, word="1024 columns")      # a multiple of EPS: only the norm's width refuses it
        row(dtype, 0, 5, 16, 1024 if dtype else 512, 0, None, tag="-refused-lds", error=True)  # NB 64, 16 steps: 160 KiB > 140 KiB
    return R


# ---- rmsnorm_f32in ------------------------------------------------------------------------------------------------------------------------
# dtype, rows, d, edge (rows >= 5), error, done (the flag is set: nothing may be written)
def _rmsnorm_rows():
    R = []
    for dtype in (0, 1):
        def row(rows, d, tag="", **kw):
            R.append(_r("rmsnorm", f"rmsnorm-f32in-{_NM[dtype]}-{rows}x{d}{tag}", dtype=dtype, rows=rows, d=d, edge=rows >= 5, error=kw.get("error", False),
                        done=kw.get("done", False)))
        for d in (8, 64, 512, 768, 1000, 1024):
            row(5, d)
        for rows in (1, 3, 4, 201):
            row(rows, 512)
        row(201, 1024)
        row(3, 1032, "-refused", error=True)
        row(3, 12, "-refused", error=True)
        row(5, 64, "-done", done=True)
    return R


# ---- self-attention over the ancestry-indexed cache ----------------------------------------------------------------------------------------
# dtype, R, H, cur_len, max_len (<= 64: NP = 8, else NP = 16), anc (identity / perm: a random permutation per step / one: every beam descends
# from beam 0; the table of the other parity always holds a different valid map), bias (plain: rel_table ~ N(0, 1) / big: one bucket of
# magnitude 30 / gap: one key dominates by a score gap of 200), done
def _self_attn_rows():
    R = []
    for dtype in (0, 1):
        def row(Rr, H, cur, mx, anc, bias="plain", done=False):
            R.append(_r("self_attn", f"self-attn-{_NM[dtype]}-R{Rr}-H{H}-len{cur}of{mx}-{anc}-{bias}{'-done' if done else ''}", dtype=dtype, R=Rr, H=H,
                        cur_len=cur, max_len=mx, anc=anc, bias=bias, done=done, inst=8 if mx <= 64 else 16))
        row(3, 1, 1, 64, "identity")
        row(5, 2, 2, 64, "perm")
        row(4, 8, 8, 64, "one")
        row(5, 2, 9, 64, "perm", "big")
        row(3, 1, 63, 64, "perm", "gap")
        row(40, 12, 64, 64, "perm")
        row(4, 8, 64, 64, "identity")
        row(5, 2, 65, 128, "perm")
        row(3, 1, 127, 128, "one", "big")
        row(40, 12, 128, 128, "perm", "gap")
        row(4, 8, 128, 128, "identity")
        row(5, 2, 9, 64, "perm", done=True)
    return R


# ---- cross-attention ----------------------------------------------------------------------------------------------------------------------
# dtype, variant (2 scalar / 3 matrix-core), fused (bf16: the kernel normalises x and projects q itself; d = d_model), B, H, Kb, L, mask
# (attn_matrix.MASKS; prefix: the first 128-key chunk -- or the first half of a shorter sequence -- wholly masked; late-one: the only valid key
# is the last of the last chunk), ldkv (1: 2 * inner; 3: three layers' blocks per row, this layer's in the middle, the others NaN), gap (one key
# dominates by a score gap of 200; q given: a fused row's condition on its bound rules such scores out), wq_scale (fused: standard deviation of q's elements, see the bound), edge (fused: the x rows of skinny amode 1), error
CROSS_MASKS = ("full", "suffix", "one", "holes", "dead", "prefix", "late-one")


def _cross_rows():
    R = []

    def row(dtype, variant, fused, B, H, Kb, L, mask, ldkv=1, d=0, gap=False, tag="", error=False, done=False, wq_scale=0.0):
        mode = "fused" if fused else _NM[dtype]
        R.append(_r("cross_attn", f"cross-attn{variant}-{mode}-B{B}-H{H}-Kb{Kb}-L{L}-{mask}-ld{ldkv}{f'-d{d}' if fused else ''}{'-gap' if gap else ''}{tag}",
                    dtype=dtype, variant=variant, fused=fused, B=B, H=H, Kb=Kb, L=L, mask=mask, ldkv=ldkv, d=d, gap=gap, error=error, done=done,
                    wq_scale=wq_scale, edge=fused and B * Kb >= 5, inst=mode if not fused else "bf16 fuseq"))
    shapes = ((1, 1, 1, 1, "full", 1), (3, 2, 5, 37, "holes", 3), (1, 12, 16, 127, "suffix", 3), (3, 1, 17, 128, "one", 1), (1, 2, 20, 129, "prefix", 3),
              (3, 2, 33, 300, "dead", 3), (1, 1, 5, 512, "late-one", 1), (3, 2, 5, 300, "prefix", 3), (1, 2, 16, 129, "late-one", 1),
              (3, 12, 17, 512, "holes", 3), (1, 1, 5, 300, "full", 3))
    for variant in (2, 3):
        for dtype in (0, 1):
            for B, H, Kb, L, mask, ld in shapes:
                row(dtype, variant, False, B, H, Kb, L, mask, ld)
            row(dtype, variant, False, 3, 2, 5, 300, "suffix", 3, gap=True)
            row(dtype, variant, False, 3, 2, 5, 37, "holes", 3, tag="-done", done=True)
        # fused: every d_model gets at least two shapes with many valid keys (i % 3 alone would leave d = 64 with one), and the last shape
        # twelve heads: five rows of one head are too few softmaxes for one of them to be peaked, which the condition on the bound needs
        for i, (B, H, Kb, L, mask, ld) in enumerate(shapes[:-1] + ((1, 12, 5, 300, "full", 3),)):
            row(1, variant, True, B, H, Kb, L, mask, ld, d=(64, 256, 512)[(i + i // 3) % 3], wq_scale=0.7)
        row(1, variant, True, 3, 2, 5, 37, "holes", 3, d=256, tag="-done", done=True, wq_scale=0.7)      # the early return ahead of the staging of x and Wq
        row(1, variant, True, 3, 2, 5, 37, "holes", 1, d=768, tag="-refused", error=True)
        row(0, variant, True, 3, 2, 5, 37, "holes", 1, d=64, tag="-refused-fp32", error=True)
    return R


# ---- streaming head -------------------------------------------------------------------------------------------------------------------------
# dtype, nv, R, d, V, inst = the <NV, LDSKB> instance, kind (normal / peaked: logits reaching +-80 and one dominant column), error.
# A wave walks its m-tiles (wave, wave + 4, ...) in units of eight 64-byte chunks through a ring of four register buffers: nunits =
# m-tiles of the wave x d / (256 bf16 | 128 fp32); the (R, d) pairs give nunits = 1, 2, 3, 4, 5, 7, 8, 9 (and more on other waves).
def _head_rows():
    R = []

    def row(dtype, nv, Rr, d, V, inst, kind="normal", gpu_only=False, error=False, done=False, tag=""):
        R.append(_r("head_lse", f"head-lse-{_NM[dtype]}-nv{nv}-R{Rr}-d{d}-V{V}{'' if kind == 'normal' else '-' + kind}{tag}", gpu_only=gpu_only, dtype=dtype,
                    nv=nv, R=Rr, d=d, V=V, inst=inst, kind=kind, error=error, done=done))
    # bf16: units per m-tile d / 256
    row(1, 128, 1, 256, 1, (128, 128))               # nunits 1
    row(1, 128, 16, 512, 128, (128, 128))            # 2; V = nv
    row(1, 128, 17, 512, 129, (128, 128), "peaked")  # V = nv + 1
    row(1, 64, 17, 256, 5, (64, 64))
    row(1, 64, 15, 512, 65, (64, 64))
    row(1, 64, 200, 768, 199, (64, 128))             # 3 m-tiles x 3 = 9 on waves 1 - 3, 12 on wave 0; V = 3 nv + 7
    row(1, 64, 65, 1024, 64, (64, 128))              # 2 x 4 = 8 on wave 0, 4 on the others
    row(1, 32, 16, 1024, 33, (32, 64))               # 4
    row(1, 32, 1, 768, 103, (32, 64))                # 3
    row(1, 32, 1, 1280, 103, (32, 128))              # 5
    row(1, 16, 65, 768, 17, (16, 64))
    row(1, 16, 17, 1792, 55, (16, 64))               # 7
    row(1, 128, 200, 512, 32100, (128, 128), gpu_only=True)      # the headline shape: 251 tiles, the last of 100 rows (1.6e9 MACs in the emulator)
    # fp32: units per m-tile d / 128
    row(0, 128, 1, 128, 129, (128, 128))             # 1
    row(0, 128, 17, 256, 5, (128, 128))              # 2
    row(0, 64, 16, 256, 64, (64, 64))
    row(0, 64, 15, 384, 65, (64, 128))               # 3
    row(0, 64, 65, 512, 199, (64, 128), "peaked")    # 2 x 4 = 8
    row(0, 32, 200, 384, 103, (32, 64))              # 3 x 3 = 9, 12
    row(0, 32, 1, 640, 1, (32, 128))                 # 5
    row(0, 32, 15, 896, 33, (32, 128))               # 7
    row(0, 32, 16, 1024, 32, (32, 128))              # 8
    row(0, 16, 17, 1024, 55, (16, 64))
    row(0, 16, 1, 512, 17, (16, 64))                 # 4
    for dtype in (0, 1):
        row(dtype, 64, 5, 512 if dtype else 256, 65, None, done=True, tag="-done")
        row(dtype, 48, 5, 512, 65, None, error=True, tag="-refused-nv")
        row(dtype, 16, 5, 320, 65, None, error=True, tag="-refused-d")
        row(dtype, 128, 5, 1024, 65, None, error=True, tag="-refused-lds")        # 128 rows of 1024: 256 / 512 KiB
    return R


# ---- row scoring ----------------------------------------------------------------------------------------------------------------------------
# dtype (of hn / E; the materialised kernel has none), streaming, K2, max_c, Kb, d, fans (fan-out of the trie node of each decode row; -1 = a
# dead row), ntiles (streaming) or V (materialised; ldl = V rounded up to 64, padding NaN), neginf_tile (one tile (-inf, 0)), excl (None / "some"
# / "all": of the children of every second row; the bitmap of user r / Kb), ties (None / "dup": the children cycle over three tokens, so their
# scores are bit-equal in threes / "dead": run_score = -1e9, every finite child rounds to the same fp32 value), done, error
def _score_rows():
    R = []

    def row(streaming, dtype, K2, fans, tag, max_c=2049, Kb=2, d=128, ntiles=3, V=255, neginf_tile=False, excl=None, ties=None, done=False, error=False,
            gpu_only=False):
        nm = f"score-{'stream-' + _NM[dtype] if streaming else 'logits'}-K2_{K2}-{tag}"
        R.append(_r("score", nm, gpu_only=gpu_only, streaming=streaming, dtype=dtype, K2=K2, fans=fans, max_c=max_c, Kb=Kb, d=d, ntiles=ntiles, V=V,
                    neginf_tile=neginf_tile, excl=excl, ties=ties, done=done, error=error))
    for streaming, dtype in ((1, 0), (1, 1), (0, 0)):
        kw = lambda i: dict(ntiles=(1, 3, 256, 257, 502)[i % 5], V=(3, 5, 255, 1027)[i % 4], d=(128, 256, 1024, 128)[i % 4] if dtype == 0 else (64, 256, 1024, 512)[i % 4])      # noqa: E731
        row(streaming, dtype, 40, (0, 1, 2, 39, 40, 41, -1, 255, 256, 257), "fans-small", excl="some", Kb=3, **kw(0))
        row(streaming, dtype, 40, (2048, -1, 2049, 257), "fans-pool", excl="some", **kw(1))
        row(streaming, dtype, 2, (0, 1, 2, 3, 255, 256, 257, 2049), "fans", excl="all", Kb=1, neginf_tile=True, **kw(2))
        row(streaming, dtype, 128, (127, 128, 129, 256, 257, 2048, 2049), "fans", excl="some", Kb=4, **kw(3))
        row(streaming, dtype, 40, (2048, 300, 41, 5), "maxc300", max_c=300, **kw(4))          # fan-outs above max_c: the first 300 children only
        row(streaming, dtype, 40, (5, 300, 2049), "ties-dup", ties="dup", excl="some", Kb=1, **kw(1))
        row(streaming, dtype, 128, (5, 300, 2049), "ties-dup", ties="dup", Kb=1, **kw(5))
        row(streaming, dtype, 40, (1100, 1100), "ties-dead", ties="dead", excl="some", Kb=1, **kw(6))
        row(streaming, dtype, 40, (5, 257), "done", done=True, **kw(0))
        row(streaming, dtype, 40, (5, 2049), "refused-scratch", error=True, **kw(0))           # fan-outs above 2048 without cand_scratch
    row(1, 1, 40, (5,), "refused-d", d=72, error=True)
    row(0, 0, 40, (5,), "refused-ldl", V=255, error=True)
    return R


SKINNY = _skinny_rows()
RMSNORM = _rmsnorm_rows()
SELF_ATTN = _self_attn_rows()
CROSS = _cross_rows()
HEAD = _head_rows()
SCORE = _score_rows()
ROWS = SKINNY + RMSNORM + SELF_ATTN + CROSS + HEAD + SCORE
assert len({r["id"] for r in ROWS}) == len(ROWS)
