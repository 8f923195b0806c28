"""not-gpu: source-level guards.

The training step is bit-reproducible because no gradient is a sum of fp32 atomics any more.  A float `atomicAdd` that
creeps back into a training kernel would not fail any tolerance-based parity test -- it would only make two runs differ in their last
bits, which AdamW then amplifies -- and the GPU reproducibility tests would catch it a round later.  This test catches it at once: every
float atomic in the kernel sources must be on the short list of known, non-default or generation-only sites."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openp5_amd", "csrc")

# file -> substrings identifying the lines that MAY hold an fp32 / LDS float atomic, with the reason
ALLOWED = {
    "p5_elem.h": ["atomicAdd(dE + ", "atomicAdd(dWW + ",      # p5_embed_bwd_kernel: the atomic scatter of rounds 1-3, only with p5_set_option("embed_det", 0)
                  "atomicAdd(dw + j, v)"],                     # p5_rmsnorm_bwd_kernel without a partial buffer: the stand-alone op entry's legacy mode
    "p5_gemm.h": ["atomicAdd(essq + row, ss)", "atomicAdd(crow + col, v)", "atomicAdd(g.ssq_out + row, w * w)", "atomicAdd(((float*)g.C) + ci, v)"],
    "p5_gemm4.h": ["atomicAdd(cp + r, v[r])", "atomicAdd((float*)g.C + ci + r, v[r])", "atomicAdd(cp + e, v[e])", "atomicAdd(g.ssq_out + row, ss)"],
    "p5_gemm5.h": ["atomicAdd(cp + r, v[r])", "atomicAdd((float*)g.C + ci + r, v[r])", "atomicAdd(cp + e, v[e])", "atomicAdd(g.ssq_out + row, ss)"],
    # (GEMM epilogues: P5_EPI_ATOMIC is issued by the engine with ONE split only -- each element receives a single add per backward --
    #  or with c_split_stride > 0, which stores; the scalar ssq form is reachable through p5_op_gemm only)
    "p5_decode2.h": ["atomicAdd((float*)g.C + ci, v)"],        # decode step of rounds 2-4 (K-split workgroups adding into the residual stream): only with p5_set_option("dec_atomic", 1)
}


def test_no_new_float_atomics_in_kernel_sources():
    found = {}
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".h", ".hip")):
            continue
        for i, line in enumerate(open(os.path.join(CSRC, fn)), 1):
            code = line.split("//")[0]
            if "atomicAdd(" not in code:
                continue
            if re.search(r"atomicAdd\(&?(s_nothit|st\.flags|hist|s_sel|pl\.hdr)", code):       # integer counters of the beam search / verification plan
                continue
            if not any(tok in code for tok in ALLOWED.get(fn, [])):
                found.setdefault(fn, []).append((i, code.strip()))
    assert not found, f"float atomics outside the allowed sites (DESIGN.md 3.5): {found}"


def test_decode_step_updates_the_residual_stream_with_one_writer_per_element():
    src = open(os.path.join(CSRC, "p5_lib.hip")).read()
    assert "g_opt_dec_atomic ? P5_SK_ATOMIC : P5_SK_RESID" in src and 'P5_DEC_ATOMIC") ? atoi(getenv("P5_DEC_ATOMIC")) : 0' in src
    assert "P5_SK_ATOMIC, 1.f, 0.f, done" not in src         # no projection of the decode step asks for the atomic epilogue directly


def test_engine_issues_atomic_gemms_with_one_split():
    src = open(os.path.join(CSRC, "p5_lib.hip")).read()
    # the only P5_EPI_ATOMIC problems the engine builds: the ungrouped weight gradient (one split unless P5_WGRAD_SPLIT_ATOMIC) and the tied
    # head's input gradient (c_split_stride > 0: partial products are stored and summed in order)
    sites = [m.start() for m in re.finditer(r"g\.epi = P5_EPI_ATOMIC", src)]
    assert len(sites) == 2, sites
    assert "g.splitk = g_opt_wgrad_split_atomic ? 0 : 1" in src
    assert "g.c_split_stride = (long long)Md * d" in src


def _gemm_launch_sites():
    """first argument of every P5_LAUNCH in p5_gemm_tu.hip, outside the P5_GEMM5_ABL lab build"""
    src = open(os.path.join(CSRC, "p5_gemm_tu.hip")).read()
    src = re.sub(r"#ifdef P5_GEMM5_ABL.*?#else", "", src, flags=re.S)
    sites = []
    for m in re.finditer(r"P5_LAUNCH\(\(", src):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        sites.append("".join(src[m.end():i - 1].split()))
    return sites


def test_every_gemm_launch_site_has_a_route_row():
    """tests/gemm_matrix.py names every launch site of the GEMM dispatcher (cases.gemm_ref_case checks the rows against float64 and, in
    the profiler's report, that they reach their site): a new kernel instance or launch branch needs a row there."""
    from tests.gemm_matrix import launch_sites
    sites = _gemm_launch_sites()
    assert len(sites) >= 25, sites
    named = {"".join(s.split()) for s in launch_sites()}
    missing = [s for s in sites if s not in named]
    assert not missing, f"GEMM launch sites without a row in tests/gemm_matrix.py: {missing}"
    stale = sorted(named - set(sites))
    assert not stale, f"rows of tests/gemm_matrix.py name launch sites that no longer exist: {stale}"


def _launch_sites(fn):
    """first argument of every P5_LAUNCH in a source file, whitespace removed"""
    src = open(os.path.join(CSRC, fn)).read()
    sites = []
    for m in re.finditer(r"P5_LAUNCH\(", src):
        i, depth = m.end(), 0
        while depth or src[i] != ",":
            depth += {"(": 1, ")": -1, "<": 1, ">": -1}.get(src[i], 0)
            i += 1
        sites.append("".join(src[m.end():i].split()))
    return sites


def test_every_row_kernel_launch_is_named_in_the_elem_table():
    """tests/elem_matrix.py names every kernel of p5_elem.h / p5_embed.h that p5_lib.hip launches: with rows checked against float64
    (cases.*_ref_case) or with the existing test that reaches it (`checked_by`), so a new row kernel cannot arrive without either."""
    from tests.elem_matrix import KERNELS, ROWS
    defined = set()
    for fn in ("p5_elem.h", "p5_embed.h"):
        defined |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(p5_\w+)\s*\(", open(os.path.join(CSRC, fn)).read()))
    assert len(defined) >= 23, sorted(defined)
    launched = set()
    for site in _launch_sites("p5_lib.hip"):
        name = re.match(r"\(*(\w+)", site).group(1)
        if name in defined:
            launched.add(name)
    assert len(launched) >= 20, sorted(launched)
    missing = sorted(launched - set(KERNELS))
    assert not missing, f"kernels launched by p5_lib.hip without an entry in tests/elem_matrix.py: {missing}"
    stale = sorted(set(KERNELS) - defined)
    assert not stale, f"tests/elem_matrix.py names kernels that p5_elem.h / p5_embed.h no longer define: {stale}"
    fams = {r["fam"] for r in ROWS}
    for k, v in KERNELS.items():
        assert ("fam" in v) != ("checked_by" in v), k
        assert "fam" not in v or v["fam"] in fams, f"{k}: no row of family {v.get('fam')}"


def test_every_decode_kernel_launch_is_named_in_the_decode_table():
    """tests/decode_matrix.py names every kernel of p5_decode.h / p5_decode2.h / p5_decode_wide.h / p5_verify.h that p5_lib.hip launches: with
    rows checked against float64 (decode_cases.*_ref_case) or with the existing token-exact test that reaches it (`checked_by`), so a new
    decode kernel cannot arrive without either."""
    from tests.decode_matrix import KERNELS, ROWS
    defined = set()
    for fn in ("p5_decode.h", "p5_decode2.h", "p5_decode_wide.h", "p5_verify.h"):
        defined |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(p5_\w+)\s*\(", open(os.path.join(CSRC, fn)).read()))
    assert len(defined) >= 25, sorted(defined)
    launched = set()
    for site in _launch_sites("p5_lib.hip"):
        name = re.match(r"\(*(\w+)", site).group(1)
        if name in defined:
            launched.add(name)
    assert len(launched) >= 25, sorted(launched)
    missing = sorted(launched - set(KERNELS))
    assert not missing, f"kernels launched by p5_lib.hip without an entry in tests/decode_matrix.py: {missing}"
    stale = sorted(set(KERNELS) - launched)
    assert not stale, f"tests/decode_matrix.py names kernels that the four headers no longer define or p5_lib.hip no longer launches: {stale}"
    fams = {r["fam"] for r in ROWS}
    for k, v in KERNELS.items():
        assert ("fam" in v) != ("checked_by" in v), k
        assert "fam" not in v or v["fam"] in fams, f"{k}: no row of family {v.get('fam')}"


def test_every_rank_kernel_launch_is_named_in_the_rank_table():
    """tests/rank_matrix.py names every kernel of p5_rank.h / p5_cand.h / p5_prune.h / p5_bound.h / p5_sample.h that p5_lib.hip launches: with rows
    checked against an exact restatement or float64 (rank_kernel_cases.*_case) or with the existing test that reaches it (`checked_by`), so a
    new ranking kernel cannot arrive without either."""
    from tests.rank_matrix import KERNELS, ROWS
    defined = set()
    for fn in ("p5_rank.h", "p5_cand.h", "p5_prune.h", "p5_bound.h", "p5_sample.h"):
        defined |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(p5_\w+)\s*\(", open(os.path.join(CSRC, fn)).read()))
    assert len(defined) >= 27, sorted(defined)
    launched = set()
    for site in _launch_sites("p5_lib.hip"):
        name = re.match(r"\(*(\w+)", site).group(1)
        if name in defined:
            launched.add(name)
    assert len(launched) >= 27, sorted(launched)
    missing = sorted(launched - set(KERNELS))
    assert not missing, f"kernels launched by p5_lib.hip without an entry in tests/rank_matrix.py: {missing}"
    stale = sorted(set(KERNELS) - launched)
    assert not stale, f"tests/rank_matrix.py names kernels that the five headers no longer define or p5_lib.hip no longer launches: {stale}"
    fams = {r["fam"] for r in ROWS}
    for k, v in KERNELS.items():
        assert ("fam" in v) != ("checked_by" in v), k
        assert "fam" not in v or v["fam"] in fams, f"{k}: no row of family {v.get('fam')}"
