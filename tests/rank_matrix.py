"""Table of the catalogue-ranking kernels (openp5_amd/csrc/p5_rank.h, p5_cand.h, p5_prune.h, p5_bound.h, p5_sample.h and the p5_tree_attn_row
body of p5_verify.h): one row per kernel and edge, shared by the emulator tests (tests/test_rank_ref_emu.py) and the GPU tests
(tests/test_gpu_rank_ref.py) of rank_kernel_cases.rank_ref_case.  Every kernel is reached through the launch helper the engine itself uses
(p5_op_rank_select, p5_op_rank_edges, p5_op_cand_row_lse, p5_op_tree_attn, p5_op_cand_plan / _rows / _score, p5_op_prune_fill / _propose /
_mask / _certify, p5_op_bound_seed / _expand).  tests/test_static.py checks that every kernel of the five headers that p5_lib.hip launches is
named in KERNELS.

Every case builds its inputs on the CPU in the stored types, runs the op with its outputs inside NaN-pattern guards (cases.GEMM_SENT; integer
outputs: the value -7), checks that nothing outside the output was written and that slots the kernel does not own keep their prior bits, and
finds the kernels it expects in the profiler report.

Exact families (the kernels are pure functions of integers and fp32 values; the reference restates them in numpy float32 / Python integers
and the comparison is bit for bit): items (the depth-ordered fp32 sum and one fp32 divide; no multiply, nothing to contract), select (sort by
(score desc, index asc) over the non-excluded items; a zero of either sign is one score: p5_wkey gives both +0.0's key and a returned zero is
+0.0), cand plan / hdr / rows / order, prune, bound.

Bounded families: |got - ref| <= bound per element against float64 on the same stored inputs.  No constant was chosen from a kernel's error;
each is one tests/decode_matrix.py already holds for the same arithmetic, with no margin on top (GEMM_S = 2^-16 fp32 dot products, TAU =
cases.ATTN_TAU[0] = 1e-5 fp32 max / sum of exp / log / divide, ELEM_R32 = 2^-24 per fp32 rounding, GEMM_R = 2^-8 per bf16 rounding):
  edges      lp = alpha h . e - lse: decode_matrix's `score` bound with run_score = 0: the logit's e_l = GEMM_S alpha sum |h e| + ELEM_R32 |l| on the
             streaming route only (the other route's logits come from the throughput GEMM, whose table is tests/gemm_matrix.py), TAU (|max| +
             |log sum|) for the log-sum-exp, 3 ELEM_R32 (|logit| + |lse|) for the fp32 operations.  An edge of a row that is not in the pass
             keeps the bits it had.
  row_lse    the log-sum-exp alone (p5_cand_lse*_kernel): max_j e_l (streaming) + TAU (|max| + |log sum|) + ELEM_R32 |lse|
  tree_attn  decode_matrix's `self_attn` bound: r |ref| + (2 e + TAU + GEMM_S) S, e = GEMM_S max_j (sum_d |q_d k_jd| + |bias_j|), S = sum_j p_j
             |v_j|, r the rounding of the stored output.  A padding row attends to itself alone: its output is its own V, bit for bit.
  cand score the mean over the path of alpha h . e - row_lse (row_lse given): the edges' e_l and 2 ELEM_R32 (|logit| + |lse|) per edge, summed
             along the path, and ELEM_R32 per fp32 addition and the divide on the sum of the |terms|: (sum_t (e_l + 2 ELEM_R32 (|l_t| +
             |lse_t|)) + (n + 1) ELEM_R32 sum_t |l_t - lse_t|) / n.  The order is then checked exactly on the scores the kernel stored.

Which head route a width takes is the engine's rule (head_nv): the streaming head needs d_model % 256 == 0 (bf16) / % 128 == 0 (fp32), every
other width takes materialised logits.  So p5_rank_score_kernel<T> sees np = d / (8 EPF) in multiples of four only: the partial group of eight
pieces is np = 4 and 12 (bf16 d = 256, 768; fp32 d = 128, 384), the full register file np = 16 (bf16 d = 1024) and 32 (fp32 d = 1024).  d = 64 and
320 run p5_rank_score_logits_kernel in both types, and p5_cand_score_kernel's own loop (np = 10 / 5 at d = 320).  No head tile exists for d =
64; the least V with more than 256 tiles per row is taken at the least streaming widths (tile 128: V = 32769).

A row is a dict with `id`, `fam`, `gpu_only` (the emulator needs more than about 2 s) and the family's own fields (see the builders).
"""

_SAMPLE = "tests/sample_cases.py::sample_case -> replay_check (tests/test_sample_items_emu.py, tests/test_gpu_sample_items.py): every draw replayed against float64"

# kernel -> the family of rows that runs it here, or `checked_by`: the existing test that reaches it
KERNELS = {
    "p5_rank_score_kernel": dict(fam="edges"),
    "p5_rank_score_logits_kernel": dict(fam="edges"),
    "p5_cand_lse_kernel": dict(fam="row_lse"),
    "p5_cand_lse_logits_kernel": dict(fam="row_lse"),
    "p5_rank_items_kernel": dict(fam="items"),
    "p5_rank_select_part_kernel": dict(fam="select"),
    "p5_rank_select_kernel": dict(fam="select"),
    "p5_rank_tree_attn_kernel": dict(fam="tree_attn"),
    "p5_cand_tree_attn_kernel": dict(fam="tree_attn"),
    "p5_cand_plan_kernel": dict(fam="cand_plan"),
    "p5_cand_hdr_kernel": dict(fam="cand_plan"),
    "p5_cand_rows_kernel": dict(fam="cand_rows"),
    "p5_cand_score_kernel": dict(fam="cand_score"),
    "p5_cand_order_kernel": dict(fam="cand_score"),
    "p5_prune_fill_kernel": dict(fam="fill"),
    "p5_prune_propose_kernel": dict(fam="propose"),
    "p5_prune_mask_kernel": dict(fam="mask"),
    "p5_prune_certify_kernel": dict(fam="certify"),
    "p5_bound_seed_kernel": dict(fam="seed"),
    "p5_bound_union_kernel": dict(fam="seed"),
    "p5_bound_expand_kernel": dict(fam="expand"),
    "p5_bound_hdr_kernel": dict(fam="expand"),
    # integer bookkeeping of the pass (token ids, a range test): compared item by item with the oracle through model.rank_items
    "p5_rank_rows_kernel": dict(checked_by="tests/rank_cases.py::rank_case (tests/test_rank_items_emu.py, tests/test_gpu_rank_items.py)"),
    "p5_rank_range_kernel": dict(checked_by="tests/rank_cases.py::range_guard_case (tests/test_rank_items_emu.py, tests/test_gpu_rank_items.py)"),
    "p5_sample_init_kernel": dict(checked_by=_SAMPLE),
    "p5_sample_step_kernel": dict(checked_by=_SAMPLE),
    "p5_sample_finish_kernel": dict(checked_by=_SAMPLE),
}
# (p5_verify.h's p5_tree_attn_kernel runs the same per-row body: variant 2 of the tree_attn rows; tests/decode_matrix.py names them)


def _r(fam, id, gpu_only=False, **kw):
    return dict(fam=fam, id=id, gpu_only=gpu_only, **kw)


_NM = {0: "fp32", 1: "bf16"}
FANS = (1, 31, 32, 33, 64, 65, 257)          # children per node


def head_nv(dtype, d):
    """the streaming head's tile as the engine picks it (p5_lib.hip: head_nv); 0 = materialised logits.  The rows carry it in their ids; every
    edges / row_lse case asserts it against the engine's own answer (p5_op_head_nv) before it runs"""
    if d % (256 if dtype == 1 else 128):
        return 0
    row = d * (2 if dtype == 1 else 4)
    for nv in (128, 64, 32, 16):
        if nv * row <= 128 * 1024:
            return nv
    return 0


# ---- edges, row_lse -------------------------------------------------------------------------------------------------------------------------
# dtype, d, V, B, CQ, nchunk, rows (plan rows per user; the rest of a user's CQ * nchunk rows is padding), HC (rows per head chunk), sel (None /
# "ragged": user 0 takes every second plan row, the last user one row), peak (row 0 of user 0: one child's logit leads by 120)
def _edges_rows():
    R = []
    for dtype in (0, 1):
        def row(d, V, tag="", B=2, CQ=16, nchunk=2, rows=27, HC=16, sel=None, peak=False, gpu_only=False):
            nv = head_nv(dtype, d)
            for fam in ("edges", "row_lse"):
                if fam == "row_lse" and (sel or peak):
                    continue
                R.append(_r(fam, f"{fam}-{_NM[dtype]}-d{d}-V{V}-{'nv%d' % nv if nv else 'logits'}{tag}", gpu_only=gpu_only, dtype=dtype, d=d, V=V, nv=nv, B=B,
                            CQ=CQ, nchunk=nchunk, rows=rows, HC=HC, sel=sel, peak=peak))
        for d in (64, 320, 512, 1024) + ((256, 768) if dtype else (128, 384)):
            row(d, 203)                                   # V % 4 = 3; 203 = 128 + 75 = 3 * 64 + 11 = 6 * 32 + 11
        row(64, 203, "-sel", sel="ragged", peak=True)
        row(512, 203, "-sel", sel="ragged", peak=True)
        row(1024, 77, "-onechunk", HC=64)                 # one head chunk (g0 = 0 only), V below every tile
        row(320, 1030, "-peak", peak=True, rows=32)       # no padding rows
        row(256 if dtype else 128, 32769, "-257tiles", B=1, CQ=16, nchunk=1, rows=13, HC=8)
    return R


# ---- items ------------------------------------------------------------------------------------------------------------------------------------
def _items_rows():
    return [_r("items", f"items-n{n}-path{pl}", n_items=n, path_len=pl, B=2) for n in (1, 255, 256, 257) for pl in (1, 6)]


# ---- select -----------------------------------------------------------------------------------------------------------------------------------
# n_items, top_n, B, pattern, excl (None: no bitmap / "some": a fifth of the items, and every bit past n_items of the last word / "all" / "few":
# all but top_n - 3 / "slice0": all but top_n / 2 items of the first slice), G the first stage's grid the row expects
SELECT_PATTERNS = ("random", "equal", "two", "oneslice", "mixed", "zeros")


def select_grid(n_items, top_n):
    slice_ = max(top_n * 4, 1024)
    G = min(max((n_items + slice_ - 1) // slice_, 1), 64)
    return G, (n_items + G - 1) // G


def _select_rows():
    R = []

    def row(n, N, pattern="random", excl="some", B=2, gpu_only=False):
        G, S = select_grid(n, N)
        R.append(_r("select", f"select-n{n}-top{N}-{pattern}-excl_{excl}", gpu_only=gpu_only, n_items=n, top_n=N, pattern=pattern, excl=excl, B=B, G=G, S=S))
    for n, N in ((1, 1), (1023, 10), (1024, 10), (1025, 10), (65537, 1), (16385, 4096)):
        row(n, N)
    row(1032193, 4096, B=1, gpu_only=True)                # G = 63 slices of 16384: 258048 keys in the second stage
    for N in (255, 256, 257):
        row(3001, N)
    for pattern in SELECT_PATTERNS[1:]:
        row(1025, 10, pattern)
        row(3001, 256, pattern, excl=None if pattern in ("equal", "zeros") else "some")
    row(16385, 4096, "equal", excl=None)
    row(16385, 4096, "two")
    for excl in ("few", "all", "slice0", None):
        row(1025, 10, excl=excl)
        row(3001, 257, excl=excl)
    row(1, 1, excl="all")
    return R


# ---- tree attention -----------------------------------------------------------------------------------------------------------------------------
# dtype, variant (0 p5_rank_tree_attn_kernel / 1 p5_cand_tree_attn_kernel through a ragged sel / 2 p5_tree_attn_kernel), H, depth (of the chain: the
# plan holds a chain of rows of depth 0 .. depth, each with a side row, so every depth up to it occurs; 128 is the deepest the bucket LUT of
# half-width 128 allows), bias (plain / rising: scores grow by 0.5 per depth, so every 8-key trip raises the running maximum / big: one bucket 30)
def _tree_rows():
    R = []
    for dtype in (0, 1):
        for variant in (0, 1, 2):
            def row(H, depth, bias="plain", B=2):
                R.append(_r("tree_attn", f"tree-attn{variant}-{_NM[dtype]}-H{H}-depth{depth}-{bias}", dtype=dtype, variant=variant, H=H, depth=depth, bias=bias, B=B))
            row(1, 0)
            row(3, 17)             # depths 0 .. 17: 7, 8, 9, 16, 17 among them
            row(1, 128, "rising")
            row(3, 128, "big")
    return R


# ---- candidates ---------------------------------------------------------------------------------------------------------------------------------
# plan: B, C, path_len (the trie's levels), kind ("mixed": random items with duplicates, -1 and ids >= n_items / "prefix": items of one subtree)
def _cand_rows():
    R = []
    for B, C, pl in ((1, 85, 3), (2, 64, 4), (2, 257, 1), (3, 33, 6), (2, 4096, 3), (2, 1, 5)):      # C * path_len: 255, 256, 257, 198, 12288, 5
        R.append(_r("cand_plan", f"cand-plan-B{B}-C{C}-path{pl}", B=B, C=C, path_len=pl))
    for B in (1, 64, 65, 130):
        R.append(_r("cand_plan", f"cand-plan-hdr-B{B}", B=B, C=3, path_len=3))
    for B, CQ, nchunk in ((1, 16, 1), (2, 16, 2), (3, 272, 1)):
        R.append(_r("cand_rows", f"cand-rows-B{B}-CQ{CQ}x{nchunk}", B=B, CQ=CQ, nchunk=nchunk))
    for dtype in (0, 1):
        def row(C, top_n, d, tag="", ties=False, B=2, pl=4):
            R.append(_r("cand_score", f"cand-score-{_NM[dtype]}-C{C}-top{top_n}-d{d}{tag}", dtype=dtype, C=C, top_n=top_n, d=d, ties=ties, B=B, path_len=pl))
        row(1, 1, 64)
        row(33, 33, 320)
        row(33, 10, 1024)
        row(65, 65, 512, "-ties", ties=True)
        row(4096, 4096, 64, pl=3)
        row(4096, 255, 64, "-ties", ties=True, pl=3)
    return R


# ---- prune --------------------------------------------------------------------------------------------------------------------------------------
def _prune_rows():
    R = [_r("fill", "prune-fill-gridstride", n=4096 * 256 * 2 + 77), _r("fill", "prune-fill-1", n=1), _r("fill", "prune-fill-257", n=257)]
    for rows in (1, 255, 256, 257, 1000):
        R.append(_r("propose", f"prune-propose-rows{rows}", rows=rows, B=4))
    for n, pl, excl in ((8219, 3, True), (8219, 3, False), (33, 6, True), (1, 1, False)):      # 8219 items: 257 bitmap words
        R.append(_r("mask", f"prune-mask-n{n}-path{pl}-{'excl' if excl else 'noexcl'}", n_items=n, path_len=pl, excl=excl, B=2))
    R.append(_r("certify", "prune-certify-causes", near=False))
    R.append(_r("certify", "prune-certify-near-misses", near=True))
    return R


# ---- bound --------------------------------------------------------------------------------------------------------------------------------------
# seed: S, T (0: the longest item + 2), short_depth (max_depth given one less than the plan's: the deepest items are "too long"), error (fewer
# key slots than n_seeds * max_depth + 1: p5_op_bound_seed refuses, nothing is written; the engine's layout always holds them).  expand: kind
# (pc_positive: rows admitted through the `Pc > 0` arm of the bound alone)
def _bound_rows():
    R = []
    for S, T, sd in ((1, 0, False), (256, 0, False), (257, 0, False), (5, 1, False), (40, 0, True), (40, 3, False)):
        R.append(_r("seed", f"bound-seed-S{S}-T{T or 'full'}{'-shortdepth' if sd else ''}", S=S, T=T, short_depth=sd, B=3))
    R.append(_r("seed", "bound-seed-S600-refused-kp", S=600, T=0, short_depth=False, B=3, error=True))      # 600 seeds x 4 levels need 4096 key slots: 2048 given
    for kind in ("none", "nan", "pc_positive", "wide", "cross256", "cross512", "beyond_kp", "empty"):
        R.append(_r("expand", f"bound-expand-{kind}", kind=kind, B=3))
    return R


EDGES = _edges_rows()
ITEMS = _items_rows()
SELECT = _select_rows()
TREE = _tree_rows()
CAND = _cand_rows()
PRUNE = _prune_rows()
BOUND = _bound_rows()
ROWS = EDGES + ITEMS + SELECT + TREE + CAND + PRUNE + BOUND
assert len({r["id"] for r in ROWS}) == len(ROWS)
