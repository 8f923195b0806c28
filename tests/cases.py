"""Parity cases shared by the not-gpu suite (host emulation backend) and the -m gpu suite (libp5hip.so on the MI355X).
Every case drives the C ABI of include/p5hip.h and checks against plain torch math or the oracle / golden fixtures."""
import ctypes
import os
import math
import random

import torch

from oracle import t5_oracle as O
from openp5_amd.model import P5ModelConfig, P5T5Native, relative_position_bucket_lut
from openp5_amd.trie import Trie, prefix_allowed_tokens_fn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TT = {0: torch.float32, 1: torch.bfloat16}


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def sync(be):
    if not be.is_emulator:
        torch.cuda.synchronize()


def dev(be, t):
    return t.to(be.device).contiguous()


# ---------------------------------------------------------------------------------------------------------
def tr_probe(be):
    """ds_read_b64_tr_b16: lane i of a 16-lane group must receive column i of the group's [4][16] block."""
    x = torch.arange(256, dtype=torch.int16)
    out = torch.zeros(256, dtype=torch.int16)
    xd, od = dev(be, x), dev(be, out)
    be.check(be.lib.p5_op_tr_probe(P(od), P(xd), be.stream_ptr()), "tr_probe")
    sync(be)
    got = od.cpu().view(64, 4)
    exp = torch.zeros(64, 4, dtype=torch.int16)
    for l in range(64):
        for j in range(4):
            exp[l, j] = (l >> 4) * 64 + j * 16 + (l & 15)
    assert torch.equal(got, exp), f"tr16 semantics differ:\n{got[:20]}\nexpected\n{exp[:20]}"


def gemm_case(be, dtype, M, N, K, a_ks, b_ks, epi=0, c_f32=0, splitk=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    tt = TT[dtype]
    A = torch.randn(M, K, generator=g).to(tt)
    Bm = torch.randn(N, K, generator=g).to(tt)
    ref = A.float() @ Bm.float().t()
    A_ = A.t().contiguous() if a_ks else A
    B_ = Bm.t().contiguous() if b_ks else Bm
    out_f32 = bool(c_f32) or dtype == 0
    C = torch.zeros(M, N, dtype=torch.float32 if out_f32 else tt)
    aux = None
    if epi == 1:
        ref = torch.relu(ref)
    elif epi == 2:
        aux = torch.randn(M, N, generator=g).to(tt)
        ref = ref + aux.float()
    elif epi == 3:
        aux = torch.randn(M, N, generator=g).to(tt)
        ref = torch.where(aux.float() > 0, ref, torch.zeros_like(ref))
    Ad, Bd, Cd = dev(be, A_), dev(be, B_), dev(be, C)
    auxd = dev(be, aux) if aux is not None else None
    be.check(be.lib.p5_op_gemm(dtype, P(Ad), P(Bd), P(Cd), P(auxd), M, N, K, A_.shape[1], B_.shape[1], N, N, a_ks, b_ks, epi, c_f32, splitk,
                               1.0, None, 0, 0.0, be.stream_ptr()), "gemm")
    sync(be)
    got = Cd.cpu().float()
    tol = 1e-4 * max(1.0, K ** 0.5) if out_f32 else 2e-2 * max(1.0, float(ref.abs().max()))
    if dtype == 1 and out_f32:
        tol = 1e-3 * max(1.0, K ** 0.5)
    err = (got - ref).abs().max().item()
    assert err <= tol, f"gemm dtype={dtype} M={M} N={N} K={K} aks={a_ks} bks={b_ks} epi={epi}: err {err} > {tol}"
    return err


# gemm_ref_case: |got - ref| <= GEMM_R[C is bf16] |ref| + GEMM_S S per element, S = sum_k |a_ik b_jk| (times the epilogue's scale) plus |aux| or
# |C0| where those are added.  GEMM_R: one bf16 rounding of the result (unit roundoff 2^-8); the bf16 epilogues also round the product P
# once before the residual add or the dropout rescale, so those get GEMM_R |P| more.  GEMM_S: fp32 accumulation (and the split-f16
# products' dropped lo x lo terms, ~2^-22 each) at any K.
GEMM_R = {True: 2.0 ** -8, False: 0.0}
GEMM_S = 2.0 ** -16
GEMM_SENT = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}     # NaN bit patterns outside the output
GEMM_STATE, GEMM_SITE = (4321, 9), 5


def _sentinel(shape, tt):
    it, v = GEMM_SENT[tt]
    return torch.full(shape, v, dtype=it).view(tt)


def _same_bits(a, b):
    it = GEMM_SENT[a.dtype][0]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _stored(g, rows, inner, ks, pad, tt, scale=1.0):
    """a logical [rows, inner] operand in dtype tt and its storage with the leading dimension padded by `pad` elements past the least legal
    one (a multiple of 16 bytes): K-contiguous [rows, ld], K-strided [inner, ld]; every padding element is NaN"""
    epf = 16 // torch.tensor([], dtype=tt).element_size()
    x = (torch.randn(rows, inner, generator=g) * scale).to(tt)
    used = rows if ks else inner
    ld = (used + epf - 1) // epf * epf + pad
    st = torch.full((inner, ld) if ks else (rows, ld), float("nan"), dtype=tt)
    if ks:
        st[:, :rows] = x.t()
    else:
        st[:, :inner] = x
    return x, st, ld


def _gemm_ref_out(A, B, epi, alpha, aux, C0, keep, drop_p, scale=None):
    """float64 reference of one problem: returns (ref, S, P) -- P the product term before aux is added (bf16 epilogues round it once)"""
    a, b = A.double(), B.double()
    sc = torch.full((a.shape[0], 1), float(alpha), dtype=torch.float64) if scale is None else scale[:, None] * float(alpha)
    prod = (a @ b.t()) * sc
    S = (a.abs() @ b.abs().t()) * sc.abs()
    zero = torch.zeros_like(prod, dtype=torch.bool)
    if epi == 1:
        zero = prod < -GEMM_S * S                  # clearly negative: ReLU gives an exact 0
        prod = prod.clamp(min=0)
    if epi in (1, 2) and keep is not None:
        prod = torch.where(keep, prod / (1.0 - drop_p), torch.zeros_like(prod))
        S = torch.where(keep, S / (1.0 - drop_p), torch.zeros_like(S))
    ref = prod
    if epi == 2:
        ref = prod + aux.double()
        S = S + aux.double().abs()
    elif epi == 3:
        ref = torch.where(aux.double() > 0, prod, torch.zeros_like(prod))
        zero = aux.double() <= 0
    elif epi in (4, 6):
        ref = prod + C0.double()
        S = S + C0.double().abs()
    if epi == 1 and keep is not None:
        zero = zero | ~keep
    return ref, S, prod, zero


def _gemm_check(tag, got_full, ref, S, P, zero, M, N, c_bf16, epi, aux, keep, extra=None):
    """one output: sentinel outside [0:M, 0:N] intact, finite, within the bound, exact zeros; returns err / bound at its worst"""
    it, v = GEMM_SENT[got_full.dtype]
    bits = got_full.view(it).clone()
    bits[:M, :N] = v
    assert bool((bits == v).all()), f"{tag}: {int((bits != v).sum())} elements outside C[0:M, 0:N] were written"
    got = got_full[:M, :N].double()
    assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} non-finite outputs (padding read, or unwritten)"
    r = GEMM_R[c_bf16]
    bound = r * ref.abs() + GEMM_S * S
    if c_bf16 and (epi == 2 or (epi == 1 and keep is not None)):
        bound = bound + r * P.abs()
    if extra is not None:
        bound = bound + extra
    err = (got - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        rr, cc = i // N, i % N
        raise AssertionError(f"{tag}: err {float(err.max()):.3e}; worst at ({rr}, {cc}): got {float(got[rr, cc]):.6e} ref {float(ref[rr, cc]):.6e} "
                             f"bound {float(bound[rr, cc]):.3e} ({int((ratio > 1).sum())} elements out of bound)")
    assert bool((got[zero] == 0).all()), f"{tag}: {int((got[zero] != 0).sum())} elements that must be exact zeros (ReLU of a negative, dropped, aux <= 0) are not"
    if epi == 2 and keep is not None:
        assert torch.equal(got[~keep], aux.double()[~keep]), f"{tag}: dropped elements are not the residual itself"
    return worst


def _set_opts(be, opts):
    """apply p5_set_option values; returns the (name, default) pairs to restore"""
    undo = []
    for k, v in opts.items():
        undo.append((k, GEMM_OPT_DEFAULTS[k]))
        be.check(be.lib.p5_set_option(k.encode(), v), f"p5_set_option {k}")
    return undo


GEMM_OPT_DEFAULTS = dict(gemm_v2=0, gemm_tile=0, gemm_ksdma=1, gemm_ring=1, gemm_small_ring=1, gemm_small_ring_tiles=256, gemm_ring32=128,
                         gemm_wide=1, gemm_ws=3, gemm_ws128=1, gemm_ws128_min_k=512, gemm_wide_min_tiles=160, gemm_ring128_min_k=1024,
                         gemm_ring128_min_tiles=128, gemm_ring_n512=1, g4_nst=3, g4_wgs=256, dec_nb=0, dec_kw=0)


def prof_kernels(report):
    """kernel keys of a p5_profile_end report"""
    import json
    return [e["kernel"] for e in json.loads(report)] if report else []


def route_matches(keys, site, tag):
    """True when a profiler key names the launch site (its P5_LAUNCH text, whitespace-insensitive) with the row's tag"""
    want = "".join(site.split())
    for k in keys:
        name = k.split(" [")[0].split(" grid=")[0]
        if "".join(name.split()).strip("()") != want:
            continue
        has = " [" in k.split(" grid=")[0]
        if (tag == "" and not has) or (tag and f" [{tag}]" in k):
            return True
    return False


def gemm_ref_case(be, row, seed=0, profile=True):
    """One row of tests/gemm_matrix.py against a float64 reference on the same rounded inputs (p5_op_gemm, p5_op_gemm_group,
    p5_op_skinny_gemm), with guard bands: operand padding is NaN, C is [M + 2, ldc] filled with a NaN sentinel that must survive outside
    [0:M, 0:N], aux is padded the same way.  Bound per element: GEMM_R |ref| + GEMM_S S (see above).  Exact: zeros of the ReLU and of the
    aux > 0 mask, dropout's keep set (O.dropout_keep_mask, row * N + col) with dropped elements exactly 0 (epilogue 1) or exactly the residual
    (epilogue 2).  With `profile`, the call is bracketed by p5_profile_begin / p5_profile_end and the report must name the row's launch
    site and tag.  Options set by the row are restored.  Returns the worst err / bound."""
    g = torch.Generator().manual_seed(seed)
    keepalive, checks = [], []
    op = row["op"]
    rng = None
    if row.get("drop", 0.0) > 0 and op != "skinny":
        rng = dev(be, torch.tensor(GEMM_STATE, dtype=torch.int32))
    sd = (GEMM_STATE[0] + GEMM_STATE[1] * 0x632BE5AB) & 0xFFFFFFFF

    def problem(M, N, K, a_ks, b_ks, epi, c_f32, dtype, pad, alpha, drop_p, stats_nt=0):
        tt = torch.bfloat16 if dtype == 1 else torch.float32
        A, Ast, lda = _stored(g, M, K, a_ks, pad[0], tt)
        B, Bst, ldb = _stored(g, N, K, b_ks, pad[1], tt)
        ct = torch.float32 if (c_f32 or dtype != 1) else torch.bfloat16
        ldc = (N + 7) // 8 * 8 + pad[2]
        Cst = _sentinel((M + 2, ldc), ct)
        C0 = None
        if epi in (4, 6):
            C0 = torch.randn(M, N, generator=g).to(ct)
            Cst[:M, :N] = C0
        aux = auxst = None
        ldaux = 0
        if epi in (2, 3):
            ldaux = (N + 7) // 8 * 8 + pad[3]
            aux = torch.randn(M, N, generator=g).to(tt)
            auxst = torch.full((M + 2, ldaux), float("nan"), dtype=tt)
            auxst[:M, :N] = aux
        keep = None
        if epi in (1, 2) and drop_p > 0:
            keep = O.dropout_keep_mask(sd, GEMM_SITE, M * N, drop_p).view(M, N)
        scale = rowss = ssq = None
        if stats_nt:
            part = (torch.rand(M, stats_nt, generator=g) * (2.0 * K / stats_nt)).float()
            ssum = torch.zeros(M, dtype=torch.float64)
            for t in range(stats_nt):
                ssum = ssum + part[:, t].double()
            scale = 1.0 / torch.sqrt(ssum / K + 1e-6)
            rowss = dev(be, part)
            ssq = dev(be, torch.full((M + 1, (N + 63) // 64), float("nan")))
        ref, S, Pt, zero = _gemm_ref_out(A, B, epi, alpha, aux, C0, keep, drop_p, scale)
        Ad, Bd, Cd = dev(be, Ast), dev(be, Bst), dev(be, Cst)
        auxd = dev(be, auxst) if auxst is not None else None
        keepalive.extend([Ad, Bd, Cd, auxd, rowss, ssq])
        checks.append(dict(Cd=Cd, ref=ref, S=S, P=Pt, zero=zero, M=M, N=N, c_bf16=ct == torch.bfloat16, epi=epi, aux=aux, keep=keep, ssq=ssq, alpha=alpha,
                           tag=f"{row['id']} ({M}x{N}x{K} epi {epi})"))
        return dict(A=Ad, B=Bd, C=Cd, aux=auxd, lda=lda, ldb=ldb, ldc=ldc, ldaux=ldaux, rowss=rowss, ssq=ssq)

    undo = _set_opts(be, row["opts"])
    report = None
    try:
        if profile:
            be.check(be.lib.p5_profile_begin(), "p5_profile_begin")
        if op == "gemm":
            d = problem(row["M"], row["N"], row["K"], row["a_ks"], row["b_ks"], row["epi"], row["c_f32"], row["dtype"], row["pad"], row["alpha"],
                        row["drop"])
            be.check(be.lib.p5_op_gemm(row["dtype"], P(d["A"]), P(d["B"]), P(d["C"]), P(d["aux"]), row["M"], row["N"], row["K"], d["lda"], d["ldb"],
                                       d["ldc"], d["ldaux"], row["a_ks"], row["b_ks"], row["epi"], row["c_f32"], row["splitk"], row["alpha"],
                                       P(rng), GEMM_SITE, row["drop"], be.stream_ptr()), f"gemm {row['id']}")
        elif op == "group":
            from openp5_amd._abi import P5GemmProblem
            arr = (P5GemmProblem * len(row["probs"]))()
            for i, (M, N, K, epi, c_f32, splitk, pad) in enumerate(row["probs"]):
                alpha = 0.75 if epi in (0, 3, 4, 6) else 1.0
                nt = row["stats_nt"] if (row["stats_nt"] and epi in (0, 1, 2, 3) and not c_f32) else 0
                d = problem(M, N, K, row["ks"], row["ks"], epi, c_f32, 1, pad, alpha, row["drop"], stats_nt=nt)
                _gemm_problem(arr, i, A=d["A"], B=d["B"], C=d["C"], M=M, N=N, K=K, lda=d["lda"], ldb=d["ldb"], ldc=d["ldc"], ldaux=d["ldaux"], epi=epi,
                              c_f32=c_f32, splitk=splitk, alpha=alpha)
                if d["aux"] is not None:
                    arr[i].aux = d["aux"].data_ptr()
                if nt:
                    q = arr[i]
                    q.rowss, q.rowss_eps, q.rowss_nt = d["rowss"].data_ptr(), 1e-6, nt
                    q.ssq_out, q.ssq_nt = d["ssq"].data_ptr(), (N + 63) // 64
            be.check(be.lib.p5_op_gemm_group(row["cfg"], row["ks"], len(row["probs"]), arr, P(rng), GEMM_SITE, row["drop"], be.stream_ptr()),
                     f"gemm_group {row['id']}")
        else:
            _skinny_problem(be, g, row, keepalive, checks)
        sync(be)
        if profile:
            buf = ctypes.create_string_buffer(1 << 16)
            be.check(be.lib.p5_profile_end(buf, len(buf)), "p5_profile_end")
            report = buf.value.decode()
            profile = False
    finally:
        if profile:
            be.lib.p5_profile_end(None, 0)
        for k, v in undo:
            be.lib.p5_set_option(k.encode(), v)
    if report is not None and row.get("site"):
        keys = prof_kernels(report)
        assert route_matches(keys, row["site"], row["tag"]), f"{row['id']}: expected {row['site']} [{row['tag']}], the profiler saw {keys}"
    worst = 0.0
    for c in checks:
        got = c["Cd"].cpu()
        worst = max(worst, _gemm_check(c["tag"], got, c["ref"], c["S"], c["P"], c["zero"], c["M"], c["N"], c["c_bf16"], c["epi"], c["aux"], c["keep"],
                                       c.get("extra")))
        if c.get("ssq") is not None:        # the output rows' partial sums per 64 columns: of the values as stored (MASK_POS: C * aux / alpha)
            M, N = c["M"], c["N"]
            s = c["ssq"].cpu().double()
            assert bool(torch.isnan(s[M:]).all()), f"{c['tag']}: ssq_out written past row M"
            v = got[:M, :N].double()
            w = v * (c["aux"].double() / c["alpha"]) if c["epi"] == 3 else v * v
            wa = w.abs()
            want = torch.stack([w[:, j:j + 64].sum(1) for j in range(0, N, 64)], 1)
            mag = torch.stack([wa[:, j:j + 64].sum(1) for j in range(0, N, 64)], 1)
            e = float(((s[:M] - want).abs() / (GEMM_S * mag).clamp(min=1e-30)).max())
            assert e <= 1.0, f"{c['tag']}: ssq_out off by {e:.3f} of its bound"
    return worst


def _skinny_problem(be, g, row, keepalive, checks):
    """p5_op_skinny_gemm (decode-step projections, p5_decode2.h): amode 0 A = T [M, lda]; amode 1 A = fp32 rows normalised by the kernel
    (T5LayerNorm with weight ln, the reference rounding order of p5_rmsnorm_fwd_kernel).  epi 0 store T * alpha, 1 ReLU store T, 2 fp32 +=
    (atomics over K splits), 3 store fp32 * alpha, 4 fp32 += with one writer per element."""
    dtype, amode, M, N, K, epi, alpha = row["dtype"], row["amode"], row["M"], row["N"], row["K"], row["epi"], row["alpha"]
    tt = TT[dtype]
    W, Wst, ldw = _stored(g, N, K, 0, row["pad"][1], tt, scale=K ** -0.5)
    extra = None
    if amode == 1:
        x = torch.randn(M, K, generator=g) * 3.0
        ln = (1.0 + 0.1 * torch.randn(K, generator=g)).float()
        rstd = torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + 1e-6)
        A = (ln.double() * (x.double() * rstd).to(tt).double()).to(tt)
        Ast, lda = x, K
        # the kernel's fp32 rstd may round an element of x rstd or of ln * that to the neighbouring T value: allow two such flips per row
        if dtype == 1:
            extra = 2.0 ** -6 * (A.double().abs()[:, None, :] * W.double().abs()[None, :, :]).amax(-1)
    else:
        A, Ast, lda = _stored(g, M, K, 0, row["pad"][0], tt)
    out_f32 = epi in (2, 3, 4)
    ct = torch.float32 if out_f32 else tt
    ldc = (N + 7) // 8 * 8 + row["pad"][2]
    Cst = _sentinel((M + 2, ldc), ct)
    C0 = None
    if epi in (2, 4):
        C0 = torch.randn(M, N, generator=g)
        Cst[:M, :N] = C0
    ref, S, Pt, zero = _gemm_ref_out(A, W, {2: 4, 4: 6}.get(epi, 0 if epi == 3 else epi), alpha, None, C0, None, 0.0)
    Ad, Wd, Cd = dev(be, Ast), dev(be, Wst), dev(be, Cst)
    lnd = dev(be, ln) if amode == 1 else None
    keepalive.extend([Ad, Wd, Cd, lnd])
    be.check(be.lib.p5_op_skinny_gemm(dtype, amode, P(Ad), lda, P(lnd), P(Wd), ldw, P(Cd), ldc, M, N, K, epi, alpha, 1e-6, be.stream_ptr()),
             f"skinny {row['id']}")
    checks.append(dict(Cd=Cd, ref=ref, S=S, P=Pt, zero=zero, M=M, N=N, c_bf16=ct == torch.bfloat16, epi=1 if epi == 1 else 0, aux=None, keep=None, ssq=None,
                       alpha=alpha, extra=extra, tag=f"{row['id']}"))


def gemm_split_case(be, M, N, K, epi=0, seed=0, scale_a=1.0, scale_b=0.05):
    """fp32 operands with the products on the f16 matrix cores (p5_gemm.h, two-term split; dtype code 2 of p5_op_gemm) against an fp64
    product: the error must be of the order of an fp32 GEMM's own (a few 2^-22 relative per product), nowhere near fp16's or bf16's."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g) * scale_a
    Bm = torch.randn(N, K, generator=g) * scale_b
    A[0, :4] = torch.tensor([3.0e-6, -7.0e-5, 1.0e3, -2.5e4][:min(4, K)])      # tiny (lo becomes subnormal) and large magnitudes
    ref = (A.double() @ Bm.double().t())
    aux = None
    if epi == 1:
        ref = torch.relu(ref)
    elif epi == 2:
        aux = torch.randn(M, N, generator=g)
        ref = ref + aux.double()
    Ad, Bd, Cd = dev(be, A), dev(be, Bm), dev(be, torch.zeros(M, N))
    auxd = dev(be, aux) if aux is not None else None
    out = {}
    for dtype in (0, 2):
        be.check(be.lib.p5_op_gemm(dtype, P(Ad), P(Bd), P(Cd), P(auxd), M, N, K, K, K, N, N, 0, 0, epi, 1, 1, 1.0, None, 0, 0.0, be.stream_ptr()), "gemm")
        sync(be)
        out[dtype] = Cd.cpu().double()
    scale = (A.double().abs() @ Bm.double().abs().t()).clamp(min=1e-30)          # sum of |products|: the natural error scale of a dot product
    e32 = ((out[0] - ref).abs() / scale).max().item()
    esp = ((out[2] - ref).abs() / scale).max().item()
    # (both accumulate in fp32: ~sqrt(K) 2^-24 of the sum of |products|; the split adds ~2^-22 per product for the dropped lo.lo term)
    assert esp <= 2 * e32 + 3e-7, f"split-f16 GEMM {M}x{N}x{K}: error {esp:.2e} of the sum of |products| (exact-fp32 kernel: {e32:.2e})"
    return e32, esp


def gemm_group_case(be, tile_cfg, ks, probs, nst=5, wgs=256, seed=0, drop_p=0.0, stats_nt=0):
    """persistent ring GEMM (p5_gemm4.h): a GROUP of bf16 problems in one launch.  probs: list of (M, N, K, epi, c_f32, splitk).
    Every epilogue against plain torch; accumulate epilogues (4 atomic, 6 C +=) start from a random C.
    stats_nt > 0 (K-contiguous, bf16 outputs): the training step's folded T5LayerNorm -- A rows are scaled by rsqrt(mean(x^2) + eps)
    from `stats_nt` partial sums of squares per row, and the output rows leave their own partial sums per 64 columns."""
    from openp5_amd._abi import P5GemmProblem
    g = torch.Generator().manual_seed(seed)
    tt = torch.bfloat16
    arr = (P5GemmProblem * len(probs))()
    keep, checks = [], []
    rng = dev(be, torch.tensor([77, 3], dtype=torch.int32)) if drop_p > 0 else None
    for i, (M, N, K, epi, c_f32, splitk) in enumerate(probs):
        A = torch.randn(M, K, generator=g).to(tt)
        Bm = torch.randn(N, K, generator=g).to(tt)
        ref = A.float() @ Bm.float().t()
        A_ = A.t().contiguous() if ks else A
        B_ = Bm.t().contiguous() if ks else Bm
        aux = None
        C0 = torch.zeros(M, N, dtype=torch.float32 if c_f32 else tt)
        alpha = 0.5 if epi in (0, 4, 6) else 1.0
        ref = ref * alpha
        if epi in (1, 2) and drop_p > 0:
            keepm = O.dropout_keep_mask((77 + 3 * 0x632BE5AB) & 0xFFFFFFFF, 5, M * N, drop_p).view(M, N)
        else:
            keepm = None
        if epi == 1:
            ref = torch.relu(ref)
            if keepm is not None:
                ref = torch.where(keepm, ref / (1 - drop_p), torch.zeros_like(ref))
        elif epi == 2:
            aux = torch.randn(M, N, generator=g).to(tt)
            if keepm is not None:
                ref = torch.where(keepm, ref / (1 - drop_p), torch.zeros_like(ref))
            ref = ref + aux.float()
        elif epi == 3:
            aux = torch.randn(M, N, generator=g).to(tt)
            ref = torch.where(aux.float() > 0, ref, torch.zeros_like(ref))
        elif epi in (4, 6):
            C0 = torch.randn(M, N, generator=g)
            ref = ref + C0
        Ad, Bd, Cd = dev(be, A_), dev(be, B_), dev(be, C0)
        auxd = dev(be, aux) if aux is not None else None
        keep += [Ad, Bd, Cd, auxd]
        q = arr[i]
        q.A, q.B, q.C, q.aux = Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr(), (auxd.data_ptr() if auxd is not None else None)
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc, q.ldaux = M, N, K, A_.shape[1], B_.shape[1], N, N
        q.epi, q.c_f32, q.splitk, q.alpha = epi, c_f32, splitk, alpha
        q.rowss, q.rowss_eps, q.ssq_out = None, 0.0, None
        q.rowss_nt = q.ssq_nt = 0
        ssq_d = None
        if stats_nt > 0 and not ks and not c_f32 and epi in (0, 1, 2, 3):
            part = (torch.rand(M, stats_nt, generator=g) * (2.0 * K / stats_nt)).float()
            eps = 1e-6
            ssum = torch.zeros(M)
            for t in range(stats_nt):            # index order, as the kernels sum them
                ssum = ssum + part[:, t]
            rstd = torch.rsqrt(ssum / K + eps)
            pre = (A.float() @ Bm.float().t()) * rstd[:, None] * alpha
            if epi == 1:
                pre = torch.relu(pre)
                if keepm is not None:
                    pre = torch.where(keepm, pre / (1 - drop_p), torch.zeros_like(pre))
            elif epi == 2:
                if keepm is not None:
                    pre = torch.where(keepm, pre / (1 - drop_p), torch.zeros_like(pre))
                pre = pre + aux.float()
            elif epi == 3:
                pre = torch.where(aux.float() > 0, pre, torch.zeros_like(pre))
            ref = pre
            partd = dev(be, part)
            nt_out = (N + 63) // 64
            ssq_d = dev(be, torch.full((M, nt_out), float("nan")))
            keep += [partd, ssq_d]
            q.rowss, q.rowss_eps, q.rowss_nt = partd.data_ptr(), eps, stats_nt
            q.ssq_out, q.ssq_nt = ssq_d.data_ptr(), nt_out
        checks.append((Cd, ref, c_f32, K, (M, N, K, epi), ssq_d, aux, alpha))
    lib = be.lib
    try:
        be.check(lib.p5_set_option(b"g4_nst", nst), "opt")
        be.check(lib.p5_set_option(b"g4_wgs", wgs), "opt")
        be.check(lib.p5_op_gemm_group(tile_cfg, ks, len(probs), arr, P(rng), 5, drop_p, be.stream_ptr()), "gemm_group")
        sync(be)
    finally:
        lib.p5_set_option(b"g4_nst", 3)
        lib.p5_set_option(b"g4_wgs", 256)
    worst = 0.0
    for Cd, ref, c_f32, K, tag, ssq_d, aux, alpha in checks:
        got = Cd.cpu().float()
        tol = 1e-3 * max(1.0, K ** 0.5) if c_f32 else 2e-2 * max(1.0, float(ref.abs().max()))
        err = (got - ref).abs().max().item()
        assert err <= tol, f"gemm_group cfg={tile_cfg} ks={ks} {tag}: err {err} > {tol}"
        worst = max(worst, err / tol)
        if ssq_d is not None:            # the output rows' partial sums of squares: of the bf16 values actually stored, per 64 columns
            N = got.shape[1]
            want = torch.stack([(got[:, c:c + 64] ** 2).sum(1) for c in range(0, N, 64)], 1)
            if tag[3] == 3:              # MASK_POS: the row sums of <d pre, pre> instead (C * aux / alpha, cases.gemm_rowdot_case)
                want = torch.stack([(got[:, c:c + 64] * aux.float()[:, c:c + 64]).sum(1) for c in range(0, N, 64)], 1) / alpha
            e2 = ((ssq_d.cpu() - want).abs() / want.abs().clamp(min=1.0)).max().item()
            assert e2 <= 1e-4, f"gemm_group {tag}: output row statistics off by {e2}"
    return worst


def _gemm_problem(arr, i, **kw):
    """one P5GemmProblem with everything optional nulled"""
    q = arr[i]
    for f in ("aux", "rowss", "ssq_out", "C2", "nb_dot", "nb_rin", "nb_rout", "nb_w", "nb_dw"):
        setattr(q, f, None)
    q.rowss_eps, q.rowss_nt, q.ssq_nt, q.ldc2, q.gate_F, q.nb_dot_nt, q.ldaux, q.c_f32, q.splitk, q.alpha = 0.0, 0, 0, 0, 0, 0, 0, 0, 1, 1.0
    for k, v in kw.items():
        setattr(q, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return q


def gemm_rowdot_case(be, M, N, K, alpha=1.0, seed=0, wgs=256):
    """P5_EPI_MASK_POS with ssq_out (p5_gemm5.h, 256x128 tiles): besides C = aux > 0 ? acc * alpha : 0 the epilogue leaves, per row and
    64-column group, sum(C * aux) / alpha with C as stored -- the row sums of <d pre, pre> that the T5LayerNorm-backward epilogue of the
    NEXT data-gradient GEMM consumes (HF modeling_t5.py:59-72, 83-94 under autograd)."""
    from openp5_amd._abi import P5GemmProblem
    g = torch.Generator().manual_seed(seed)
    tt = torch.bfloat16
    A = torch.randn(M, K, generator=g).to(tt)
    Bm = torch.randn(N, K, generator=g).to(tt)
    aux = (torch.randn(M, N, generator=g).clamp(min=0) * alpha).to(tt)       # a saved hidden: relu(pre) * alpha
    Ad, Bd, auxd = dev(be, A), dev(be, Bm), dev(be, aux)
    Cd = dev(be, torch.zeros(M, N, dtype=tt))
    nt = (N + 63) // 64
    dotd = dev(be, torch.full((M, nt), float("nan")))
    arr = (P5GemmProblem * 1)()
    _gemm_problem(arr, 0, A=Ad, B=Bd, C=Cd, aux=auxd, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldaux=N, epi=3, alpha=alpha, ssq_out=dotd, ssq_nt=nt)
    try:
        be.check(be.lib.p5_set_option(b"g4_wgs", wgs), "opt")
        be.check(be.lib.p5_op_gemm_group(3, 0, 1, arr, None, 0, 0.0, be.stream_ptr()), "gemm_group")
        sync(be)
    finally:
        be.lib.p5_set_option(b"g4_wgs", 256)
    ref = torch.where(aux.float() > 0, (A.float() @ Bm.float().t()) * alpha, torch.zeros(M, N))
    got = Cd.cpu().float()
    assert (got - ref).abs().max().item() <= 2e-2 * max(1.0, float(ref.abs().max()))
    want = torch.stack([(got[:, c:c + 64] * aux.float()[:, c:c + 64]).sum(1) for c in range(0, N, 64)], 1) / alpha
    err = ((dotd.cpu() - want).abs() / want.abs().clamp(min=1.0)).max().item()
    assert err <= 1e-4, f"row sums of <d pre, pre> off by {err}"
    return err


def gemm_norm_bwd_case(be, M, N, K, dot_nt, drop_p=0.0, seed=0, wgs=256, with_n=True):
    """P5_EPI_NORM_BWD (p5_gemm5.h, 128x128 tiles): the T5LayerNorm backward (HF modeling_t5.py:59-72 under autograd) in the epilogue of the
    data-gradient GEMM that produces the norm's input gradient.  Against the formulas of the stand-alone kernel in plain torch fp32:
    residual gradient out, the next dy with dropout, n = w * round(x rstd), partial rows of the norm-weight gradient."""
    from openp5_amd._abi import P5GemmProblem
    g = torch.Generator().manual_seed(seed)
    tt = torch.bfloat16
    eps = 1e-6
    A = torch.randn(M, K, generator=g).to(tt)
    Bm = (torch.randn(N, K, generator=g) / K ** 0.5).to(tt)
    x = (torch.randn(M, N, generator=g) * 2.0).to(tt)
    w = torch.rand(N, generator=g) + 0.5
    rin = torch.randn(M, N, generator=g)
    ssq = torch.stack([(x.float()[:, c:c + 64] ** 2).sum(1) for c in range(0, N, 64)], 1).contiguous()
    dotp = torch.randn(M, dot_nt, generator=g)
    Ad, Bd, xd, wd, rind, ssqd, dotd = (dev(be, t) for t in (A, Bm, x, w, rin, ssq, dotp))
    Cd = dev(be, torch.zeros(M, N, dtype=tt))
    C2d = dev(be, torch.zeros(M, N, dtype=tt)) if with_n else None
    routd = dev(be, torch.full((M, N), float("nan")))
    dwd = dev(be, torch.full((M // 64, N), float("nan")))
    rng = dev(be, torch.tensor([77, 3], dtype=torch.int32)) if drop_p > 0 else None
    arr = (P5GemmProblem * 1)()
    _gemm_problem(arr, 0, A=Ad, B=Bd, C=Cd, aux=xd, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ldaux=N, epi=10, rowss=ssqd, rowss_eps=eps, rowss_nt=N // 64,
                  C2=C2d, ldc2=N, nb_dot=dotd, nb_dot_nt=dot_nt, nb_rin=rind, nb_rout=routd, nb_w=wd, nb_dw=dwd)
    try:
        be.check(be.lib.p5_set_option(b"g4_wgs", wgs), "opt")
        be.check(be.lib.p5_op_gemm_group(4, 0, 1, arr, P(rng), 5, drop_p, be.stream_ptr()), "gemm_group")
        sync(be)
    finally:
        be.lib.p5_set_option(b"g4_wgs", 256)
    dn = A.float() @ Bm.float().t()
    ssum = torch.zeros(M)
    for t in range(N // 64):
        ssum = ssum + ssq[:, t]
    rstd = torch.rsqrt(ssum / N + eps)
    dsum = torch.zeros(M)
    for t in range(dot_nt):
        dsum = dsum + dotp[:, t]
    m = dsum / N
    xh = x.float() * rstd[:, None]
    v = rstd[:, None] * (dn * w[None, :] - xh * m[:, None]) + rin
    scale = float(v.abs().max())
    e_r = (routd.cpu() - v).abs().max().item() / scale
    assert e_r <= 2e-3, f"norm-backward epilogue: residual gradient off by {e_r}"
    out = routd.cpu()
    if drop_p > 0:
        keepm = O.dropout_keep_mask((77 + 3 * 0x632BE5AB) & 0xFFFFFFFF, 5, M * N, drop_p).view(M, N)
        dscale = torch.ones(()) / (torch.ones(()) - torch.tensor(drop_p, dtype=torch.float32))      # (the kernels multiply by the fp32 reciprocal)
        out = torch.where(keepm, out * dscale, torch.zeros_like(out))
    assert torch.equal(Cd.cpu(), out.to(tt)), "norm-backward epilogue: dy_next is not dropout(residual gradient) rounded once"
    if with_n:
        n_ref = (w[None, :] * xh.to(tt).float()).to(tt)
        e_n = (C2d.cpu().float() - n_ref.float()).abs().max().item() / float(n_ref.float().abs().max())
        assert e_n <= 1e-2, f"norm-backward epilogue: n off by {e_n}"
    dw_ref = (dn * xh).view(M // 64, 64, N).sum(1)
    e_w = (dwd.cpu() - dw_ref).abs().max().item() / float(dw_ref.abs().max())
    assert e_w <= 2e-3, f"norm-backward epilogue: norm-weight gradient partials off by {e_w}"
    return e_r, e_w


def attn_rowdot_case(be, B, H, L, mode="enc", drop_p=0.1, seed=3, mask="suffix"):
    """P5AttnArgs::dot_out of the fused attention backward (bf16, self-attention, 16 < L <= 128): <dQ, Q> + <dK, K> + <dV, V> per token and
    head from the gradients as stored; the gradients themselves are bit-identical to the call without it.  mask (enc): attn_key_mask's
    patterns; 'dead' (sample 0 without a valid key): its gradient rows and row sums are exactly 0."""
    g = torch.Generator().manual_seed(seed)
    tt = torch.bfloat16
    inner = H * 64
    qkv = (torch.randn(B * L, 3 * inner, generator=g) * 0.5).to(tt)
    qkvd = dev(be, qkv)
    Qd, Kd, Vd = qkvd, qkvd[:, inner:], qkvd[:, 2 * inner:]
    table_d = dev(be, torch.randn(32, H, generator=g) * 0.5)
    lut_half = 512
    lut_d = dev(be, relative_position_bucket_lut(lut_half, mode == "enc", 32, 128))
    kmask = attn_key_mask(B, L, mask, g) if mode == "enc" else None
    km_d = dev(be, kmask) if mode == "enc" else None
    causal = 1 if mode == "dec" else 0
    dOd = dev(be, torch.randn(B * L, inner, generator=g).to(tt))
    rng = dev(be, torch.tensor([1234, 7], dtype=torch.int32))
    Od = dev(be, torch.zeros(B * L, inner, dtype=tt))
    lse = dev(be, torch.zeros(B * H * L))
    be.check(be.lib.p5_op_attn_fwd(1, P(Qd), P(Kd), P(Vd), P(Od), P(lse), P(table_d), P(lut_d), lut_half, P(km_d), B, H, L, L, 3 * inner,
                                   3 * inner, 3 * inner, inner, causal, P(rng), 11, drop_p, be.stream_ptr()), "attn_fwd")
    res = []
    for want_dot in (True, False):
        dqkv = dev(be, torch.zeros(B * L, 3 * inner, dtype=tt))
        dtab = dev(be, torch.zeros(32, H))
        dscr = dev(be, torch.zeros(B * ((L + 63) // 64), 32 * H))
        Dv = dev(be, torch.zeros(B * H * L))
        dot = dev(be, torch.full((B * L, H), float("nan"))) if want_dot else None
        be.check(be.lib.p5_op_attn_bwd_dot(1, P(Qd), P(Kd), P(Vd), P(Od), P(dOd), P(lse), P(Dv), P(dqkv), P(dqkv[:, inner:]), P(dqkv[:, 2 * inner:]),
                                           P(table_d), P(dtab), P(dscr), 32, P(lut_d), lut_half, P(km_d), B, H, L, L, 3 * inner, 3 * inner, 3 * inner, inner,
                                           3 * inner, 3 * inner, 3 * inner, causal, P(rng), 11, drop_p, P(dot), be.stream_ptr()), "attn_bwd_dot")
        sync(be)
        res.append((dqkv.cpu(), dtab.cpu().clone(), dot.cpu() if want_dot else None))
    (ga, ta, dot), (gb, tb, _) = res
    assert torch.equal(ga, gb) and torch.equal(ta, tb), "attention backward changed by dot_out"
    prod = (ga.float() * qkv.float()).view(B * L, 3, H, 64).sum(3).sum(1)
    err = ((dot - prod).abs() / prod.abs().clamp(min=1.0)).max().item()
    assert err <= 1e-4 and bool(torch.isfinite(dot).all()), f"row sums of <d qkv, qkv> off by {err}"
    if mask == "dead":
        assert bool((ga[:L] == 0).all()) and bool((dot[:L] == 0).all()), "dead sample: gradient rows / row sums are not exactly 0"
    return err


def _gelu_new(a):
    return 0.5 * a * (1.0 + torch.tanh(0.7978845608028654 * (a + 0.044715 * a ** 3)))


def gemm_gate_case(be, M, F, K, drop_p=0.0, stats_nt=0, seed=0):
    """Gated-GELU FFN (T5 v1.1, HF modeling_t5.py:97-123) fused into the GEMMs around it (p5_gemm5.h whole-tile epilogues).
    Forward (epi 5): ONE GEMM over [wi_0; wi_1] writes u = [u0 | u1] and h = dropout(gelu_new(u0) * u1); backward (epi 7): the data-gradient
    GEMM dh = dy Wo writes du = [dh' u1 gelu'(u0) | dh' gelu(u0)] with dh' = dh under h's dropout mask.  Against plain torch."""
    from openp5_amd._abi import P5GemmProblem
    g = torch.Generator().manual_seed(seed)
    tt = torch.bfloat16
    rng = dev(be, torch.tensor([77, 3], dtype=torch.int32)) if drop_p > 0 else None
    keepm = O.dropout_keep_mask((77 + 3 * 0x632BE5AB) & 0xFFFFFFFF, 5, M * F, drop_p).view(M, F) if drop_p > 0 else None
    bf = lambda t: t.to(tt).float()      # noqa: E731
    # ---- forward
    A = torch.randn(M, K, generator=g).to(tt)
    W = (torch.randn(2 * F, K, generator=g) / K ** 0.5).to(tt)
    pre = A.float() @ W.float().t()
    arr = (P5GemmProblem * 1)()
    q = arr[0]
    Ad, Wd = dev(be, A), dev(be, W)
    hd = dev(be, torch.full((M, F), float("nan")).to(tt))
    ud = dev(be, torch.full((M, 2 * F), float("nan")).to(tt))
    keep = [Ad, Wd, hd, ud]
    q.A, q.B, q.C, q.aux, q.C2 = Ad.data_ptr(), Wd.data_ptr(), hd.data_ptr(), None, ud.data_ptr()
    q.M, q.N, q.K, q.lda, q.ldb, q.ldc, q.ldaux, q.ldc2, q.gate_F = M, 2 * F, K, K, K, F, 0, 2 * F, F
    q.epi, q.c_f32, q.splitk, q.alpha = 5, 0, 1, 1.0
    q.rowss, q.rowss_eps, q.ssq_out, q.rowss_nt, q.ssq_nt = None, 0.0, None, 0, 0
    if stats_nt > 0:
        part = (torch.rand(M, stats_nt, generator=g) * (2.0 * K / stats_nt)).float()
        ssum = torch.zeros(M)
        for t in range(stats_nt):
            ssum = ssum + part[:, t]
        pre = pre * torch.rsqrt(ssum / K + 1e-6)[:, None]
        partd = dev(be, part)
        keep.append(partd)
        q.rowss, q.rowss_eps, q.rowss_nt = partd.data_ptr(), 1e-6, stats_nt
    be.check(be.lib.p5_op_gemm_group(1, 0, 1, arr, P(rng), 5, drop_p, be.stream_ptr()), "gemm_group (gate fwd)")
    sync(be)
    u_got, h_got = ud.cpu().float(), hd.cpu().float()
    assert (u_got - pre).abs().max().item() <= 2e-2 * max(1.0, float(pre.abs().max())), "gate fwd: stored u"
    h_ref = _gelu_new(u_got[:, :F]) * u_got[:, F:]            # the gate of the STORED (rounded) u, as the stand-alone kernel computes it
    if keepm is not None:
        h_ref = torch.where(keepm, h_ref / (1 - drop_p), torch.zeros_like(h_ref))
    err_h = (h_got - bf(h_ref)).abs().max().item()
    assert err_h <= 1.6e-2 * max(1.0, float(h_ref.abs().max())), f"gate fwd: h off by {err_h}"      # (one bf16 rounding of a value near the max)
    assert torch.equal(h_got == 0, bf(h_ref) == 0) or keepm is None, "gate fwd: dropout mask"
    # ---- backward
    dy = torch.randn(M, K, generator=g).to(tt)
    WoT = (torch.randn(F, K, generator=g) / K ** 0.5).to(tt)
    u = torch.randn(M, 2 * F, generator=g).to(tt)
    dh = bf(dy.float() @ WoT.float().t())
    if keepm is not None:
        dh = torch.where(keepm, dh / (1 - drop_p), torch.zeros_like(dh))
    a, b = u[:, :F].float().requires_grad_(True), u[:, F:].float().requires_grad_(True)
    (_gelu_new(a) * b).backward(dh)
    du_ref = torch.cat([a.grad, b.grad], 1)
    dyd, Wod, uq = dev(be, dy), dev(be, WoT), dev(be, u)
    dud = dev(be, torch.full((M, 2 * F), float("nan")).to(tt))
    keep += [dyd, Wod, uq, dud]
    q.A, q.B, q.C, q.aux, q.C2 = dyd.data_ptr(), Wod.data_ptr(), dud.data_ptr(), uq.data_ptr(), None
    q.M, q.N, q.K, q.lda, q.ldb, q.ldc, q.ldaux, q.ldc2, q.gate_F = M, F, K, K, K, 2 * F, 2 * F, 0, 0
    q.epi = 7
    q.rowss, q.rowss_eps, q.rowss_nt = None, 0.0, 0
    be.check(be.lib.p5_op_gemm_group(1, 0, 1, arr, P(rng), 5, drop_p, be.stream_ptr()), "gemm_group (gate bwd)")
    sync(be)
    err_d = (dud.cpu().float() - du_ref).abs().max().item()
    assert err_d <= 2e-2 * max(1.0, float(du_ref.abs().max())), f"gate bwd: du off by {err_d}"
    return err_h, err_d


def gemm_v2_case(be, stages, M, N, K, epi, tile=128, ks=0):
    lib = be.lib
    try:
        be.check(lib.p5_set_option(b"gemm_v2", stages), "set_option")
        be.check(lib.p5_set_option(b"gemm_tile", tile), "set_option")
        return gemm_case(be, 1, M, N, K, ks, ks, epi=epi, c_f32=1 if epi == 4 else 0, splitk=2 if epi == 4 else 1)
    finally:
        lib.p5_set_option(b"gemm_v2", 0)
        lib.p5_set_option(b"gemm_tile", 0)


def rmsnorm_case(be, dtype, rows, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    tt = TT[dtype]
    x = torch.randn(rows, d, generator=g).to(tt)
    w = (1.0 + 0.1 * torch.randn(d, generator=g))
    dy = torch.randn(rows, d, generator=g).to(tt)
    dres = torch.randn(rows, d, generator=g)
    xr = x.float().clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    yr = O.rmsnorm(xr, wr, 1e-6)
    yr.backward(dy.float())
    y = torch.zeros(rows, d, dtype=tt)
    rstd = torch.zeros(rows)
    xd, wd, yd, rd = dev(be, x), dev(be, w), dev(be, y), dev(be, rstd)
    be.check(be.lib.p5_op_rmsnorm_fwd(dtype, P(yd), P(rd), P(xd), P(wd), rows, d, 1e-6, be.stream_ptr()), "rmsnorm_fwd")
    dyd, dresd = dev(be, dy), dev(be, dres)      # keep the device buffers alive across the launch
    tol = 1e-5 if dtype == 0 else 3e-2
    e_y = (yd.cpu().float() - yr.detach()).abs().max().item()
    assert e_y <= tol * 4, f"rmsnorm fwd dtype={dtype} rows={rows} d={d}: y {e_y:.3e}"
    for partial in (False, True):                # dw by atomics / by per-workgroup partials + reduction (the engine's mode)
        _rmsnorm_bwd_check(be, dtype, rows, d, tt, xr, wr, dres, xd, wd, rd, dyd, dresd, partial, tol)


def _rmsnorm_bwd_check(be, dtype, rows, d, tt, xr, wr, dres, xd, wd, rd, dyd, dresd, partial, tol):
    dres_out = dev(be, torch.zeros(rows, d))
    dy_next = dev(be, torch.zeros(rows, d, dtype=tt))
    dw = dev(be, torch.zeros(d))
    scratch = dev(be, torch.zeros(1024 * d)) if partial else None
    be.check(be.lib.p5_op_rmsnorm_bwd(dtype, P(dres_out), P(dy_next), P(dw), P(dyd), P(xd), P(wd), P(rd), P(dresd), rows, d,
                                      P(scratch) if partial else None, be.stream_ptr()), "rmsnorm_bwd")
    sync(be)
    e_dx = (dres_out.cpu() - (xr.grad + dres)).abs().max().item()
    e_dw = (dw.cpu() - wr.grad).abs().max().item()
    e_nx = (dy_next.cpu().float() - dres_out.cpu()).abs().max().item()
    msg = f"rmsnorm dtype={dtype} rows={rows} d={d} partial={partial}: dx {e_dx:.3e} dw {e_dw:.3e} next {e_nx:.3e}"
    assert e_dx <= tol * 8, msg
    assert e_dw <= tol * 8 * max(1.0, rows ** 0.5), msg
    assert e_nx <= (1e-6 if dtype == 0 else 5e-2), msg


# attn_ref_case: error bound relative to the reference's largest entry, independent of L ...
ATTN_TAU = {0: 1e-5, 1: 2.0 ** -6}
# ... or to this fraction of the same sums over |terms| where that is larger (O, dQ, dK, dV; relative-bias gradient dT): a result that
# cancels to (near) zero -- dQ, dK and dT of rows with one valid key, or at Lk = 1, are sums of P (dP - D) with P = 1 and dP = D -- keeps
# the rounding of its terms (fp32: ~2^-23 of them).  In bf16 dT needs the floor at long L too: at L = 512 a bucket sums ~10^5 dS values
# (bf16-rounded, as the MFMA sees them) that cancel to 4e-4 .. 1e-3 of their absolute sum.
ATTN_FLOOR = {0: (2e-2, 1e-2), 1: (1e-3, 1e-3)}


def attn_key_mask(B, Lk, pattern, g):
    """[B, Lk] key-padding mask (nonzero = attend).  full: no padding; suffix: a valid prefix of at least Lk // 2 keys; one: a single
    valid key inside the last 16-key chunk (the long-sequence kernels decide mask handling once per 16 / 64 keys); holes: Bernoulli(0.5)
    per key, at least one valid; dead: sample 0 has no valid key at all, the others are `suffix`."""
    km = torch.ones(B, Lk, dtype=torch.long)
    for b in range(B):
        if pattern == "full":
            continue
        if pattern == "suffix" or (pattern == "dead" and b > 0):
            km[b, int(torch.randint(max(1, Lk // 2), Lk + 1, (1,), generator=g)):] = 0
        elif pattern == "dead":
            km[b] = 0
        elif pattern == "one":
            c0 = (Lk - 1) // 16 * 16
            km[b] = 0
            km[b, c0 + int(torch.randint(0, Lk - c0, (1,), generator=g))] = 1
        elif pattern == "holes":
            km[b] = (torch.rand(Lk, generator=g) < 0.5).long()
            km[b, int(torch.randint(0, Lk, (1,), generator=g))] = 1
        else:
            raise ValueError(pattern)
    return km


def attn_ref64(q, k, v, dO, bias, valid, keep, drop_p, o_fwd=None):
    """float64 attention and its backward, written out.  q, dO [B,H,Lq,64], k, v [B,H,Lk,64], bias [H,Lq,Lk] or None, valid [B,1|H,Lq,Lk]
    bool (key mask and causal), keep [B,H,Lq,Lk] bool or None.  A DEAD row (no valid key) has P = 0: O = 0, lse = -inf, and it adds
    nothing to any gradient -- the engine's contract (HF's finfo.min mask would attend uniformly instead).  o_fwd: the forward output
    the backward is given (D = rowsum(dO o_fwd), as the kernels read it; default: the exact O).  Returns O, lse, dQ, dK, dV, dS (for
    the bias gradient) and `mag`: the same products over absolute values, the scale of the terms a result cancels."""
    s = q @ k.transpose(2, 3)
    if bias is not None:
        s = s + bias[None]
    s = s.masked_fill(~valid, float("-inf"))
    m = s.amax(-1, keepdim=True)
    dead = torch.isinf(m)
    e = torch.where(valid, torch.exp(s - torch.where(dead, torch.zeros_like(m), m)), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(dead, torch.ones_like(l), l)
    lse = torch.where(dead, torch.full_like(m, float("-inf")), m + torch.log(torch.where(dead, torch.ones_like(l), l))).squeeze(-1)
    ks = keep.double() / (1.0 - drop_p) if keep is not None else torch.ones_like(p)
    pd = p * ks
    o = pd @ v
    dp = (dO @ v.transpose(2, 3)) * ks
    D = (dO * (o if o_fwd is None else o_fwd)).sum(-1, keepdim=True)
    ds = p * (dp - D)
    out = dict(O=o, lse=lse, dQ=ds @ k, dK=ds.transpose(2, 3) @ q, dV=pd.transpose(2, 3) @ dO)
    dsa = p * ((dO.abs() @ v.abs().transpose(2, 3)) * ks + (dO.abs() * (pd @ v.abs())).sum(-1, keepdim=True))
    mag = dict(O=pd @ v.abs(), dQ=dsa @ k.abs(), dK=dsa.transpose(2, 3) @ q.abs(), dV=pd.transpose(2, 3) @ dO.abs())
    return out, ds, dsa, mag, dead.squeeze(-1)


def attn_ref_case(be, dtype, B, H, Lq, Lk, mode, mask="suffix", drop_p=0.0, op_bits=False, seed=0, tau=None, rowdot=False):
    """Every attention kernel against a float64 reference on the SAME (device-rounded) inputs.  mode: 'enc' (bidirectional bias + key
    mask, self), 'dec' (causal + unidirectional bias, self, no key mask), 'cross' (key mask only).  mask: attn_key_mask's patterns.
    Scores are q k^T + rel_bias (no 1/sqrt(d) scaling, as in T5) with -inf at masked keys.  Dropout (drop_p > 0) is the engine's counter
    hash replayed by the oracle (O.dropout_keep_mask), P keep / (1 - p) before PV, lse before dropout; op_bits: the long-sequence
    forward stores its keep decisions for the backward.  Per output (O, lse, dQ, dK, dV, d_rel_table): all finite, max |err| <=
    tau max |ref| and relative L2 error <= tau / 4 (tau = ATTN_TAU[dtype]; where a result cancels, ATTN_FLOOR).  Dead rows (mask
    'dead'): lse exactly -inf, O and the dead sample's dQ, dK, dV rows exactly 0, and no share in d_rel_table (the reference gives
    them none).  rowdot (bf16 self-attention, 16 < L <= 128): the fused backward's dot_out as well.  Returns the worst error per
    output as a fraction of its bound."""
    tau = ATTN_TAU[dtype] if tau is None else tau
    g = torch.Generator().manual_seed(seed)
    tt = TT[dtype]
    inner = H * 64
    self_attn = mode != "cross"
    if self_attn:
        assert Lq == Lk
        qkv = (0.5 * torch.randn(B * Lq, 3 * inner, generator=g)).to(tt)
        Qs, Ks, Vs = qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:]
        ldq = ldk = ldv = 3 * inner
    else:
        qb = (0.5 * torch.randn(B * Lq, inner, generator=g)).to(tt)
        kvb = (0.5 * torch.randn(B * Lk, 2 * inner, generator=g)).to(tt)
        Qs, Ks, Vs = qb, kvb[:, :inner], kvb[:, inner:]
        ldq, ldk, ldv = inner, 2 * inner, 2 * inner
    table = (0.5 * torch.randn(32, H, generator=g)) if self_attn else None
    kmask = attn_key_mask(B, Lk, mask, g) if mode != "dec" else None
    dO = torch.randn(B * Lq, inner, generator=g).to(tt)
    state = (1234 + seed, 7)
    site = 11

    def heads(x, Ln):
        return x.double().reshape(B, Ln, H, 64).transpose(1, 2)

    def unheads(x, Ln):
        return x.transpose(1, 2).reshape(B * Ln, inner)

    lut_half = 512
    lut = relative_position_bucket_lut(lut_half, mode == "enc", 32, 128) if self_attn else None
    rel = torch.arange(Lk)[None, :] - torch.arange(Lq)[:, None]
    bias = table.double()[lut[rel + lut_half].long()].permute(2, 0, 1) if self_attn else None
    valid = torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    if kmask is not None:
        valid = valid & (kmask[:, None, None, :] != 0)
    if mode == "dec":
        valid = valid & torch.ones(Lq, Lk, dtype=torch.bool).tril()
    keep = None
    if drop_p > 0:
        sd = (state[0] + state[1] * 0x632BE5AB) & 0xFFFFFFFF                  # p5_rng.h:p5_seed
        keep = O.dropout_keep_mask(sd, site, B * H * Lq * Lk, drop_p).view(B, H, Lq, Lk)

    Od = dev(be, torch.zeros(B * Lq, inner, dtype=tt))
    lse = dev(be, torch.full((B * H * Lq,), float("nan")))
    if self_attn:
        qkv_d = dev(be, qkv)
        Qd, Kd, Vd = qkv_d, qkv_d[:, inner:], qkv_d[:, 2 * inner:]
    else:
        q_d, kv_d = dev(be, qb), dev(be, kvb)
        Qd, Kd, Vd = q_d, kv_d, kv_d[:, inner:]
    table_d = dev(be, table) if self_attn else None
    lut_d = dev(be, lut) if self_attn else None
    km_d = dev(be, kmask) if kmask is not None else None
    causal = 1 if mode == "dec" else 0
    rng = dev(be, torch.tensor(state, dtype=torch.int32)) if drop_p > 0 else None
    if self_attn:
        dqkv = dev(be, torch.full((B * Lq, 3 * inner), float("nan"), dtype=tt))
        dQd, dKd, dVd = dqkv, dqkv[:, inner:], dqkv[:, 2 * inner:]
        lddq = lddk = lddv = 3 * inner
    else:
        dq_d = dev(be, torch.full((B * Lq, inner), float("nan"), dtype=tt))
        dkv_d = dev(be, torch.full((B * Lk, 2 * inner), float("nan"), dtype=tt))
        dQd, dKd, dVd = dq_d, dkv_d, dkv_d[:, inner:]
        lddq, lddk, lddv = inner, 2 * inner, 2 * inner
    dtab = dev(be, torch.zeros(32, H)) if self_attn else None
    dscr = dev(be, torch.full((B * ((Lq + 63) // 64), 32 * H), float("nan"))) if self_attn else None
    Dv = dev(be, torch.zeros(B * H * Lq))
    dOd = dev(be, dO)
    dot = dev(be, torch.full((B * Lq, H), float("nan"))) if rowdot else None
    be.check(be.lib.p5_set_option(b"attn_op_keep_bits", 1 if op_bits else 0), "set_option")
    try:
        be.check(be.lib.p5_op_attn_fwd(dtype, P(Qd), P(Kd), P(Vd), P(Od), P(lse), P(table_d), P(lut_d), lut_half, P(km_d), B, H, Lq, Lk, ldq,
                                       ldk, ldv, inner, causal, P(rng), site, drop_p, be.stream_ptr()), "attn_fwd")
        args = (dtype, P(Qd), P(Kd), P(Vd), P(Od), P(dOd), P(lse), P(Dv), P(dQd), P(dKd), P(dVd), P(table_d), P(dtab), P(dscr), 32, P(lut_d),
                lut_half, P(km_d), B, H, Lq, Lk, ldq, ldk, ldv, inner, lddq, lddk, lddv, causal, P(rng), site, drop_p)
        if rowdot:
            be.check(be.lib.p5_op_attn_bwd_dot(*args, P(dot), be.stream_ptr()), "attn_bwd_dot")
        else:
            be.check(be.lib.p5_op_attn_bwd(*args, be.stream_ptr()), "attn_bwd")
        sync(be)
    finally:
        be.check(be.lib.p5_set_option(b"attn_op_keep_bits", 0), "set_option")

    # (the backward reference takes D from the forward output as stored: the kernels do, and O itself is checked against the exact one)
    ref, ds, dsa, mag, dead = attn_ref64(heads(Qs, Lq), heads(Ks, Lk), heads(Vs, Lk), heads(dO, Lq), bias, valid, keep, drop_p,
                                         o_fwd=heads(Od.cpu(), Lq))
    if self_attn:      # d rel_table[bucket, h] = sum of dS over the (q, k) whose relative position falls in the bucket
        idx = lut[rel + lut_half].long().reshape(-1)
        ref["dT"] = torch.zeros(32, H, dtype=torch.float64).index_add_(0, idx, ds.sum(0).permute(1, 2, 0).reshape(-1, H))
        mag["dT"] = torch.zeros(32, H, dtype=torch.float64).index_add_(0, idx, dsa.sum(0).permute(1, 2, 0).reshape(-1, H))
    got = {"O": Od.cpu().double(), "lse": lse.cpu().double().view(B, H, Lq)}
    if self_attn:
        g_all = dqkv.cpu().double()
        got["dQ"], got["dK"], got["dV"] = g_all[:, :inner], g_all[:, inner:2 * inner], g_all[:, 2 * inner:]
        got["dT"] = dtab.cpu().double()
    else:
        got["dQ"] = dq_d.cpu().double()
        got["dK"], got["dV"] = dkv_d.cpu().double()[:, :inner], dkv_d.cpu().double()[:, inner:]
    want = {"O": unheads(ref["O"], Lq), "lse": ref["lse"], "dQ": unheads(ref["dQ"], Lq), "dK": unheads(ref["dK"], Lk),
            "dV": unheads(ref["dV"], Lk)}
    floor = {"O": unheads(mag["O"], Lq), "dQ": unheads(mag["dQ"], Lq), "dK": unheads(mag["dK"], Lk), "dV": unheads(mag["dV"], Lk)}
    if self_attn:
        want["dT"], floor["dT"] = ref["dT"], mag["dT"]
    tag = f"attention {mode} dtype={dtype} B={B} H={H} Lq={Lq} Lk={Lk} mask={mask} drop={drop_p} bits={int(op_bits)}"
    ratios = {}
    for name, w in want.items():
        x = got[name]
        if name == "lse":          # live rows against the reference, dead rows exactly -inf
            assert bool(torch.isneginf(x[dead]).all()), f"{tag}: lse of dead rows is not -inf: {x[dead][~torch.isneginf(x[dead])][:4]}"
            x, w = x[~dead], w[~dead]
            fl = torch.zeros(())
        else:
            fl = floor[name]
        assert bool(torch.isfinite(x).all()), f"{tag}: {name} has {int((~torch.isfinite(x)).sum())} non-finite entries"
        if x.numel() == 0:
            continue
        err = x - w
        c = ATTN_FLOOR[dtype][1 if name == "dT" else 0]
        smax = max(float(w.abs().max()), c * float(fl.abs().max()))
        sl2 = max(float(w.norm()), c * float(fl.norm()))
        r_max = float(err.abs().max()) / smax if smax > 0 else float(err.abs().max())
        r_l2 = float(err.norm()) / sl2 if sl2 > 0 else float(err.norm())
        ratios[name] = max(r_max, 4 * r_l2) / tau
        assert r_max <= tau and r_l2 <= tau / 4, f"{tag}: {name} max err {r_max:.3e} of max |ref|, L2 err {r_l2:.3e} (tau {tau:.3e})"
    if mask == "dead":
        assert not bool(dead[1:].any()) and bool(dead[0].all())
        for name, Ln in (("O", Lq), ("dQ", Lq), ("dK", Lk), ("dV", Lk)):
            rows = got[name][:Ln]
            assert bool((rows == 0).all()), f"{tag}: {name} rows of the dead sample are not exactly 0 (max {float(rows.abs().max())})"
    if rowdot:
        dg = dot.cpu().double()
        gq = torch.cat([got["dQ"], got["dK"], got["dV"]], 1)
        prod = (gq * qkv.double()).view(B * Lq, 3, H, 64).sum(3).sum(1)
        assert bool(torch.isfinite(dg).all()), f"{tag}: dot_out not finite"
        e = float(((dg - prod).abs() / prod.abs().clamp(min=1.0)).max())
        assert e <= 1e-4, f"{tag}: row sums of <d qkv, qkv> off by {e}"
        if mask == "dead":
            assert bool((dg[:Lq] == 0).all()), f"{tag}: dot_out rows of the dead sample are not 0"
    return ratios


def attn_case(be, dtype, B, H, Lq, Lk, mode, seed=0):
    """mode: 'enc' (bidirectional bias + key mask, self), 'dec' (causal + unidirectional bias, self), 'cross' (mask only); suffix key
    padding, no dropout: attn_ref_case's float64 reference and bounds."""
    return attn_ref_case(be, dtype, B, H, Lq, Lk, mode, mask="suffix", seed=seed)


def attn_fwd_wg_case(be, B, H, Lq, Lk, mode="enc", drop_p=0.1, seed=6, option=b"attn_fwd_wg", exact=True, op_bits=False):
    """bf16 attention forward with dropout ON: the one-workgroup-per-(batch, head) kernel (p5_attn_fwd_wg_kernel; for Lk > 128
    option b"attn_fwd_head": p5_attn_fwd_head_kernel) against the 64-query-block kernel on identical inputs and masks.  Same arithmetic
    in the same order per row: outputs and lse are equal (exact=False: the log-sum-exp is equal, the outputs agree to one bf16
    rounding -- the head-resident kernel feeds P to the MFMA in another key order)."""
    g = torch.Generator().manual_seed(seed)
    inner = H * 64
    tt = torch.bfloat16
    self_attn = mode != "cross"
    if self_attn:
        qkv = dev(be, (0.5 * torch.randn(B * Lq, 3 * inner, generator=g)).to(tt))
        Qd, Kd, Vd, ldq, ldk = qkv, qkv[:, inner:], qkv[:, 2 * inner:], 3 * inner, 3 * inner
    else:
        Qd = dev(be, (0.5 * torch.randn(B * Lq, inner, generator=g)).to(tt))
        kv = dev(be, (0.5 * torch.randn(B * Lk, 2 * inner, generator=g)).to(tt))
        Kd, Vd, ldq, ldk = kv, kv[:, inner:], inner, 2 * inner
    table_d = dev(be, 0.5 * torch.randn(32, H, generator=g)) if self_attn else None
    lut_half = 512
    lut_d = dev(be, relative_position_bucket_lut(lut_half, mode == "enc", 32, 128)) if self_attn else None
    kmask = torch.ones(B, Lk, dtype=torch.long)
    if mode != "dec":
        for b in range(B):
            kmask[b, int(torch.randint(max(1, Lk // 2), Lk + 1, (1,), generator=g)):] = 0
    km_d = dev(be, kmask) if mode != "dec" else None
    rng = dev(be, torch.tensor([4321, 3], dtype=torch.int32))
    res = []
    be.check(be.lib.p5_set_option(b"attn_op_keep_bits", 1 if op_bits else 0), "set_option")      # (the forward variant that also stores its keep masks)
    for wg in (1, 0):
        be.check(be.lib.p5_set_option(option, wg), "set_option")
        Od = dev(be, torch.zeros(B * Lq, inner, dtype=tt))
        lse = dev(be, torch.zeros(B * H * Lq))
        be.check(be.lib.p5_op_attn_fwd(1, P(Qd), P(Kd), P(Vd), P(Od), P(lse), P(table_d), P(lut_d), lut_half, P(km_d), B, H, Lq, Lk, ldq, ldk,
                                       ldk, inner, 1 if mode == "dec" else 0, P(rng), 9, drop_p, be.stream_ptr()), "attn_fwd")
        sync(be)
        res.append((Od.cpu().float(), lse.cpu().clone()))
    be.check(be.lib.p5_set_option(option, 1), "set_option")
    be.check(be.lib.p5_set_option(b"attn_op_keep_bits", 0), "set_option")
    (oa, la), (ob, lb) = res
    assert ob.abs().max() > 0.05 and bool(torch.isfinite(oa).all()) and bool(torch.isfinite(la).all())
    assert torch.equal(la, lb), float((la - lb).abs().max())
    if exact:
        assert torch.equal(oa, ob), float((oa - ob).abs().max())
    else:
        assert bool(((oa - ob).abs() <= ob.abs() * 2.0 ** -7 + 1e-6).all()), float((oa - ob).abs().max())


def attn_keep_masks_forward_case(be, shapes, reps):
    """bf16, dropout on, 128 < L <= 512: the forward variant that also stores its keep decisions as lane masks (p5_attn_fwd_head_kernel<.., true>;
    op hook b"attn_op_keep_bits") returns EXACTLY the output and log-sum-exp of the variant that does not, over repeated runs with fresh
    seeds and at grids of more workgroups than CUs.  (Regression test of a hardware-only failure: with partial lgkmcnt waits between the
    transposed V reads and the first P V MFMA the masks variant multiplied by stale register contents -- 1e38 / NaN in the first 16 output
    columns of some rows, different from run to run -- while the emulator and small grids passed: profiles/r05_call21_keep_mask_bisect.txt.)"""
    import ctypes
    tt = torch.bfloat16
    lut_d = dev(be, relative_position_bucket_lut(512, True, 32, 128))
    try:
        for (B, H, L) in shapes:
            inner = H * 64
            for rep in range(reps):
                g = torch.Generator().manual_seed(100 + rep)
                qkv = dev(be, (0.5 * torch.randn(B * L, 3 * inner, generator=g)).to(tt))
                table_d = dev(be, 0.5 * torch.randn(32, H, generator=g))
                km_d = dev(be, torch.ones(B, L, dtype=torch.long))
                rng = dev(be, torch.tensor([4321 + rep, 3], dtype=torch.int32))
                outs = []
                for ob in (0, 1, 1):
                    be.check(be.lib.p5_set_option(b"attn_op_keep_bits", ob), "set_option")
                    Od = dev(be, torch.zeros(B * L, inner, dtype=tt))
                    lse = dev(be, torch.zeros(B * H * L))
                    be.check(be.lib.p5_op_attn_fwd(1, P(qkv), P(qkv[:, inner:]), P(qkv[:, 2 * inner:]), P(Od), P(lse), P(table_d), P(lut_d), 512, P(km_d), B, H, L, L,
                                                   3 * inner, 3 * inner, 3 * inner, inner, 0, P(rng), 9, ctypes.c_float(0.1), be.stream_ptr()), "attn_fwd")
                    sync(be)
                    outs.append((Od.cpu(), lse.cpu()))
                assert bool(torch.isfinite(outs[0][0].float()).all())
                for o, l in outs[1:]:
                    assert torch.equal(o, outs[0][0]) and torch.equal(l, outs[0][1]), (B, H, L, rep, int((o != outs[0][0]).sum()))
    finally:
        be.check(be.lib.p5_set_option(b"attn_op_keep_bits", 0), "set_option")


def attn_fused_bwd_case(be, B, H, L, mode="enc", drop_p=0.1, seed=5, option=b"attn_fused", op_bits=False):
    """bf16 attention backward with dropout ON: the one-workgroup-per-(batch, head) kernel (p5_attn_bwd_fused_kernel) against the
    two-kernel path on identical inputs (same forward output, lse and counter-based masks).  Both round P and dS to bf16 at the
    same point, so they differ only by the order of fp32 accumulation."""
    g = torch.Generator().manual_seed(seed)
    inner = H * 64
    tt = torch.bfloat16
    qkv = dev(be, (0.5 * torch.randn(B * L, 3 * inner, generator=g)).to(tt))
    Qd, Kd, Vd = qkv, qkv[:, inner:], qkv[:, 2 * inner:]
    table_d = dev(be, 0.5 * torch.randn(32, H, generator=g))
    lut_half = 512
    lut_d = dev(be, relative_position_bucket_lut(lut_half, mode == "enc", 32, 128))
    kmask = torch.ones(B, L, dtype=torch.long)
    if mode == "enc":
        for b in range(B):
            kmask[b, int(torch.randint(max(1, L // 2), L + 1, (1,), generator=g)):] = 0
    km_d = dev(be, kmask) if mode == "enc" else None
    causal = 1 if mode == "dec" else 0
    dOd = dev(be, torch.randn(B * L, inner, generator=g).to(tt))
    rng = dev(be, torch.tensor([1234, 7], dtype=torch.int32))
    Od = dev(be, torch.zeros(B * L, inner, dtype=tt))
    lse = dev(be, torch.zeros(B * H * L))
    # op_bits: the forward stores its dropout decisions as lane masks and the head-resident backward reads them (the blocked one re-hashes)
    be.check(be.lib.p5_set_option(b"attn_op_keep_bits", 1 if op_bits else 0), "set_option")
    be.check(be.lib.p5_op_attn_fwd(1, P(Qd), P(Kd), P(Vd), P(Od), P(lse), P(table_d), P(lut_d), lut_half, P(km_d), B, H, L, L, 3 * inner,
                                   3 * inner, 3 * inner, inner, causal, P(rng), 11, drop_p, be.stream_ptr()), "attn_fwd")
    res = []
    for fused in (1, 0):
        be.check(be.lib.p5_set_option(option, fused), "set_option")
        dqkv = dev(be, torch.zeros(B * L, 3 * inner, dtype=tt))
        dtab = dev(be, torch.zeros(32, H))
        dscr = dev(be, torch.zeros(B * ((L + 63) // 64), 32 * H))
        Dv = dev(be, torch.zeros(B * H * L))
        be.check(be.lib.p5_op_attn_bwd(1, P(Qd), P(Kd), P(Vd), P(Od), P(dOd), P(lse), P(Dv), P(dqkv), P(dqkv[:, inner:]), P(dqkv[:, 2 * inner:]),
                                       P(table_d), P(dtab), P(dscr), 32, P(lut_d), lut_half, P(km_d), B, H, L, L, 3 * inner, 3 * inner, 3 * inner, inner,
                                       3 * inner, 3 * inner, 3 * inner, causal, P(rng), 11, drop_p, be.stream_ptr()), "attn_bwd")
        sync(be)
        res.append((dqkv.cpu().float(), dtab.cpu().clone()))
    be.check(be.lib.p5_set_option(option, 1), "set_option")
    be.check(be.lib.p5_set_option(b"attn_op_keep_bits", 0), "set_option")
    (ga, ta), (gb, tb) = res
    assert gb.abs().max() > 0.05 and bool(torch.isfinite(ga).all())
    e_g = (ga - gb).abs().max().item() / gb.abs().max().item()
    e_t = (ta - tb).abs().max().item() / max(1e-6, tb.abs().max().item())
    assert e_g <= 1e-2 and e_t <= 1e-3, f"fused vs two-kernel attention backward: grads {e_g}, rel-bias table {e_t}"
    return e_g, e_t


# ---------------------------------------------------------------------------------------------------------
def build_model(be, ocfg, params, dtype, dropout=0.0, seed=1):
    cfg = P5ModelConfig(vocab_size=ocfg.vocab_size, d_model=ocfg.d_model, d_ff=ocfg.d_ff, num_layers=ocfg.num_layers,
                        num_decoder_layers=ocfg.num_decoder_layers, num_heads=ocfg.num_heads, dropout_rate=dropout,
                        feed_forward_proj="relu" if ocfg.ff_act == "relu" else "gated-gelu")
    m = P5T5Native(cfg, dtype=dtype, backend=be, seed=seed)
    m.load_state_dict(params, strict=True)
    return m


def released_checkpoint_case(be, tmp, ocfg, dtype="fp32", nll_tol=3e-5):
    """A checkpoint in the layout of OpenP5's released `.pt` files -- `torch.save(model.state_dict())` of the HF-derived P5_T5
    (/root/reference/src/src_t5/utils/utils.py:119-121): stock `T5ForConditionalGeneration.state_dict()` keys INCLUDING the duplicated tied
    tables (`encoder.embed_tokens.weight`, `decoder.embed_tokens.weight`, `lm_head.weight`) plus `encoder.whole_word_embeddings.weight`
    (P5_T5.py:64-67), saved from a model whose vocabulary is larger than ours (main.py:193 resizes afterwards) -- goes through
    `utils.load_model` (utils.py:123-129) into the native model: per-token NLL must equal stock HF's on the same weights, and a save /
    load round trip of OUR state dict must reproduce the file's keys."""
    import os
    from oracle import hf_ref
    from openp5_amd.utils import utils as U
    big = O.T5Cfg(**{**ocfg.__dict__, "vocab_size": ocfg.vocab_size + 28})          # "32128 -> 32100"
    params = O.init_params(big, 11)
    hf, wwe = hf_ref.build_hf(big, params)
    sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    sd["encoder.whole_word_embeddings.weight"] = wwe.weight.detach().clone()
    assert {"shared.weight", "encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight"} <= set(sd)
    path = os.path.join(tmp, "released.pt")
    torch.save(sd, path)
    cfg = P5ModelConfig(vocab_size=big.vocab_size, d_model=ocfg.d_model, d_ff=ocfg.d_ff, num_layers=ocfg.num_layers,
                        num_decoder_layers=ocfg.num_decoder_layers, num_heads=ocfg.num_heads, dropout_rate=0.0,
                        feed_forward_proj="relu" if ocfg.ff_act == "relu" else "gated-gelu")
    m = P5T5Native(cfg, dtype=dtype, backend=be, seed=3)
    U.load_model(m, path)                                   # the file's vocabulary
    m.resize_token_embeddings(ocfg.vocab_size)              # main.py:193: keep the first rows
    m.eval()
    ids, ww, mask, labels, _ = synth_batch(ocfg, 3, 14, 5, 2)
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"].detach().cpu()
    with torch.no_grad():
        nll_hf, logits = hf_ref.hf_forward_nll(hf, wwe, ids, ww, mask, labels)
        # HF scored against its full table; the resized model sees the first `vocab_size` columns only
        lg = logits[..., :ocfg.vocab_size]
        nll_ref = torch.nn.functional.cross_entropy(lg.reshape(-1, ocfg.vocab_size), labels.view(-1), reduction="none")
    err = (nll - nll_ref).abs().max().item()
    assert err <= nll_tol, f"released-layout checkpoint: nll differs from stock HF by {err}"
    # our own save -> load round trip keeps the HF key set (tied duplicates included) and the values
    path2 = os.path.join(tmp, "ours.pt")
    U.save_model(m, path2)
    sd2 = torch.load(path2, map_location="cpu")
    assert set(sd) <= set(sd2) | {"decoder.block.0.layer.1.EncDecAttention.relative_attention_bias.weight"}, set(sd) - set(sd2)
    assert torch.equal(sd2["lm_head.weight"], sd2["shared.weight"]) and sd2["shared.weight"].shape[0] == ocfg.vocab_size
    m2 = P5T5Native(P5ModelConfig(**{**cfg.__dict__, "vocab_size": ocfg.vocab_size}), dtype=dtype, backend=be, seed=4)
    U.load_model(m2, path2)
    m2.eval()
    nll2 = m2(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"].detach().cpu()
    assert torch.equal(nll, nll2)
    return err


def synth_batch(cfg, B, L, T, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, cfg.vocab_size, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    for b in range(1, B):
        n = max(1, int(torch.randint(L // 2, L + 1, (1,), generator=g)))
        mask[b, n:] = 0
        ids[b, n:] = 0
    ww = torch.cumsum((torch.rand(B, L, generator=g) < 0.4).long(), 1) * mask
    labels = torch.randint(3, cfg.vocab_size, (B, T), generator=g)
    out_attn = torch.ones(B, T, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(2, T + 1, (1,), generator=g)) if T >= 2 else 1
        labels[b, n - 1] = cfg.eos_id
        labels[b, n:] = 0
        out_attn[b, n:] = 0
    return ids, ww, mask, labels, out_attn


def model_train_case(be, ocfg, B, L, T, dtype="fp32", dropout=0.0, seed=3, nll_tol=2e-5, grad_tol=2e-4):
    """forward NLL + every parameter gradient against the oracle (autograd on the CPU restatement)."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    m = build_model(be, ocfg, params, dtype, dropout)
    ids, ww, mask, labels, out_attn = synth_batch(ocfg, B, L, T, seed)
    dp = None
    if dropout > 0:
        m.train()
        m.set_dropout_seed(1234, 0)
        dp = O.DropoutPlan((1234 + 1 * 0x632BE5AB) & 0xFFFFFFFF, dropout)
    else:
        m.eval()
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, alpha=2, return_dict=True)["loss"]
    assert nll.shape == (B * T,)
    loss = O.runner_loss(nll, out_attn.to(nll.device))
    loss.backward()
    sync(be)
    Pq = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    nll_o = O.p5_forward_nll(Pq, ocfg, ids, ww, mask, labels, dp)
    O.runner_loss(nll_o, out_attn).backward()
    err = (nll.detach().cpu() - nll_o.detach()).abs().max().item()
    assert err <= nll_tol, f"nll err {err}"
    worst = (0.0, "")
    # error of each tensor relative to its own largest entry, with a floor of 1 % of the largest gradient entry overall
    # (tensors whose gradient is analytically zero -- e.g. q/k of a 1-token self-attention -- only carry rounding noise)
    gmax = max(float(v.grad.abs().max()) for v in Pq.values())
    for name, p in m.named_parameters():
        g_, go = p.grad.detach().cpu(), Pq[name].grad
        rel = (g_ - go).abs().max().item() / (go.abs().max().item() + 1e-2 * gmax + 1e-12)
        if rel > worst[0]:
            worst = (rel, name)
    assert worst[0] <= grad_tol, f"gradient mismatch {worst}"
    return err, worst


def model_dead_sample_case(be, ocfg, B, L, T, dtype="fp32", seed=3, loss_tol=2e-5, grad_tol=2e-4, drop_tol=1e-5):
    """A batch whose sample 0 has an all-zero attention_mask and no label weight: every encoder row and every decoder cross-attention
    row of that sample is dead (no valid key).  The engine gives those rows O = 0 and zero gradient; the oracle follows HF (finfo.min
    mask: the row attends uniformly) -- the two agree on everything the loss sees, because that sample carries no loss.  The loss and
    every parameter gradient are finite and match the oracle (relative to each tensor's largest entry, as model_train_case), and they
    equal the gradients of the same batch without sample 0 (scaled by (B - 1) / B: runner_loss averages over the samples) to drop_tol."""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = synth_batch(ocfg, B, L, T, seed)
    mask[0] = 0
    out_attn[0] = 0

    def engine(sl):
        m = build_model(be, ocfg, params, dtype)
        m.eval()
        nll = m(input_ids=ids[sl], whole_word_ids=ww[sl], attention_mask=mask[sl], labels=labels[sl], return_dict=True)["loss"]
        loss = O.runner_loss(nll, out_attn[sl].to(nll.device))
        loss.backward()
        sync(be)
        return float(loss), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}

    loss, grads = engine(slice(0, B))
    loss_r, grads_r = engine(slice(1, B))
    Pq = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    loss_o = O.runner_loss(O.p5_forward_nll(Pq, ocfg, ids, ww, mask, labels), out_attn)
    loss_o.backward()
    assert math.isfinite(loss) and abs(loss - float(loss_o)) <= loss_tol * max(1.0, abs(float(loss_o))), f"loss {loss} vs oracle {float(loss_o)}"
    assert abs(loss * B - loss_r * (B - 1)) <= drop_tol * max(1.0, abs(loss_r)) * B, f"loss {loss} vs {loss_r} without the dead sample"
    bad = [n for n, g_ in grads.items() if not bool(torch.isfinite(g_).all())]
    assert not bad, f"{len(bad)} of {len(grads)} parameter gradients are not finite: {bad[:6]}"
    gmax = max(float(v.grad.abs().max()) for v in Pq.values())
    worst, worst_r = (0.0, ""), (0.0, "")
    for name, g_ in grads.items():
        go = Pq[name].grad.double()
        rel = float((g_ - go).abs().max()) / (float(go.abs().max()) + 1e-2 * gmax + 1e-12)
        gr = grads_r[name] * ((B - 1) / B)
        rel_r = float((g_ - gr).abs().max()) / (float(gr.abs().max()) + 1e-2 * gmax + 1e-12)
        worst = max(worst, (rel, name))
        worst_r = max(worst_r, (rel_r, name))
    assert worst[0] <= grad_tol, f"gradient mismatch against the oracle {worst}"
    assert worst_r[0] <= drop_tol, f"gradients differ from the batch without the dead sample {worst_r}"
    return worst, worst_r


def golden_case(be, name, dtype="fp32", nll_tol=3e-5, grad_tol=3e-4, score_tol=2e-5):
    """HIP path vs fixtures produced by stock HF T5 (tests/golden/make_golden.py)."""
    fx = torch.load(os.path.join(GOLDEN, name + ".pt"), weights_only=False)
    ocfg = O.T5Cfg(**fx["cfg"])
    params = O.init_params(ocfg, fx["params_seed"])
    m = build_model(be, ocfg, params, dtype)
    m.eval()
    nll = m(input_ids=fx["input_ids"], whole_word_ids=fx["whole_word_ids"], attention_mask=fx["attention_mask"], labels=fx["labels"])["loss"]
    loss = O.runner_loss(nll, fx["output_attention"].to(nll.device))
    loss.backward()
    sync(be)
    assert (nll.detach().cpu() - fx["nll"]).abs().max().item() <= nll_tol
    assert abs(float(loss) - float(fx["loss"])) <= nll_tol
    tied = {"shared.weight"}
    for k, p in m.named_parameters():
        ref = fx["grad_norms"].get(k)
        if ref is None:
            continue
        got = float(p.grad.norm())
        assert abs(got - ref) <= grad_tol * max(1.0, ref) + 1e-7, f"grad norm {k}: {got} vs {ref}"
    assert (m.shared.weight.grad[:16].cpu() - fx["grad_shared"]).abs().max() <= grad_tol
    rel = dict(m.named_parameters())["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].grad.cpu()
    assert (rel - fx["grad_enc_rel"]).abs().max() <= grad_tol
    fn = prefix_allowed_tokens_fn(Trie(fx["items"]))
    out = m.generate(input_ids=fx["input_ids"], attention_mask=fx["attention_mask"], whole_word_ids=fx["whole_word_ids"],
                     max_length=fx["max_length"], prefix_allowed_tokens_fn=fn, num_beams=fx["num_beams"],
                     num_return_sequences=fx["num_beams"], output_scores=True, return_dict_in_generate=True)
    compare_generation(out["sequences"].cpu(), out["sequences_scores"].cpu(), fx["sequences"], fx["sequences_scores"], score_tol)


def compare_generation(seq, score, seq_ref, score_ref, score_tol, eos=1, tie_tol=0.0, K=None):
    """Token-exact up to and including the first EOS (HF 5.15 pads with eos, HF 4.26 / this path with pad=0).
    tie_tol > 0 (bf16 engine against the fp32 oracle; K = rows per batch item): a row may hold a different hypothesis if the
    reference ranks that hypothesis within tie_tol of this row's reference score (a swap between near-ties), or -- when the
    reference's top-K does not contain it -- if this row is within tie_tol of the reference's K-th score (a boundary item)."""
    assert seq.shape[0] == seq_ref.shape[0]
    if tie_tol <= 0:
        assert (score - score_ref).abs().max().item() <= score_tol, (score, score_ref)

    def cut(t):
        t = t.tolist()
        e_ = t.index(eos) if eos in t else len(t) - 1
        return t[:e_ + 1], t[e_ + 1:]
    for r in range(seq.shape[0]):
        (a, pad), (b, _) = cut(seq[r]), cut(seq_ref[r])
        assert all(t == 0 for t in pad), f"row {r} not pad-filled: {seq[r].tolist()}"
        if a == b:
            assert abs(float(score[r]) - float(score_ref[r])) <= score_tol, (r, score, score_ref)
            continue
        assert tie_tol > 0 and K, f"row {r}: {a} vs {b}"
        g0 = r // K * K
        group = [cut(seq_ref[q])[0] for q in range(g0, g0 + K)]
        if a in group:
            q = g0 + group.index(a)
            assert abs(float(score[r]) - float(score_ref[q])) <= score_tol, f"row {r}: score of a hypothesis both searches return differs"
        else:
            # a low-precision search prunes differently where an intermediate decision of the reference was a near-tie: it may keep a
            # hypothesis the reference dropped -- legitimate only if that hypothesis scores at least as well as the one it displaces
            assert float(score[r]) >= float(score_ref[r]) - tie_tol, f"row {r}: {a} is not in the reference's top-{K} and scores worse"


def make_items(n_items, seed, lo=7, hi=40, prefix=(0, 5, 6), minlen=2, maxlen=4):
    rnd = random.Random(seed)
    items = set()
    while len(items) < n_items:
        n = rnd.randint(minlen, maxlen)
        items.add(tuple(list(prefix) + [rnd.randint(lo, hi) for _ in range(n)] + [1]))
    return sorted(list(x) for x in items)


def generate_case(be, ocfg, B, L, K, max_len, n_items, dtype="fp32", seed=5, score_tol=2e-5, via="ours", id_len=(2, 4), mode=None, extra_beams=None,
                  sabotage=None, prefix=(0, 5, 6)):
    """mode (bf16 models): "verified" = the bf16 search proposes, the fp32 pass decides (csrc/p5_verify.h) -- held to the fp32 tolerances;
    "draft" = the plain bf16 search; None = the model's default.  sabotage(hist): test hook, edits the draft's recorded history before the
    verification pass reads it (to force the flagged-user fallback)."""
    params = O.init_params(ocfg, 7)
    m = build_model(be, ocfg, params, dtype)
    m.eval()
    if mode is not None:
        m.generation_mode = mode
    if extra_beams is not None:
        m.verify_extra_beams = extra_beams
    if sabotage is not None:
        plain = m._search
        def _search(engine, ws_attr, *a, hist=None):
            r = plain(engine, ws_attr, *a, hist=hist)
            if hist is not None:
                sabotage(hist, a[3], a[5])      # (B, K of the draft)
            return r
        m._search = _search
    verified = dtype == "bf16" and m.generation_mode == "verified"
    ids, ww, mask, _, _ = synth_batch(ocfg, B, L, 4, seed)
    items = make_items(n_items, seed, hi=min(60, ocfg.vocab_size - 1), minlen=id_len[0], maxlen=id_len[1], prefix=prefix)
    trie = Trie(items)
    if via == "append":             # generation_trie.py:19-21: a second trie takes over where the first one reaches `bos_token_id`
        bos = min(61, ocfg.vocab_size - 2)
        heads = sorted({tuple(it[:4]) for it in items})                      # the first four tokens of the item ids: several graft points ...
        trie = Trie([list(h) + [bos] for h in heads])
        trie.append(Trie([list(it[4:]) for it in items]), bos)               # ... sharing ONE appended trie of their tails (ending in </s>)
        fn = prefix_allowed_tokens_fn(trie)
    elif via == "ours":
        fn = prefix_allowed_tokens_fn(trie)
    elif via == "closure":          # the reference's closure style (generation_trie.py:91-97)
        def make(candidate_trie):
            def prefix_allowed_tokens(batch_id, sentence):
                return candidate_trie.get(sentence.tolist())
            return prefix_allowed_tokens
        fn = make(trie)
    else:                           # opaque callable -> host exploration path
        fn = lambda b, s: trie.get(s.tolist())   # noqa: E731
    out = m.generate(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=max_len, prefix_allowed_tokens_fn=fn,
                     num_beams=K, num_return_sequences=K, output_scores=True, return_dict_in_generate=True)
    with torch.no_grad():
        s_ref, sc_ref = O.beam_search(params, ocfg, ids, ww, mask, lambda b, s: trie.get(s.tolist()), K, max_len)
    compare_generation(out["sequences"].cpu(), out["sequences_scores"].cpu(), s_ref, sc_ref, score_tol,
                       tie_tol=0.05 if (dtype == "bf16" and not verified) else 0.0, K=K)
    out["verify_stats"] = dict(m.verify_stats)
    return out


def generate_excluded_case(be, ocfg, B, L, K, max_len, n_items, dtype="fp32", seed=5, score_tol=2e-5, frac=0.4, mode=None):
    """Per-user history exclusion (DistributedRunner.py:286-297): the shared device trie + one excluded-node bitmap per user
    must rank exactly like the reference protocol's per-user Trie(all_items - positive)."""
    from openp5_amd.trie import CompiledTrie
    params = O.init_params(ocfg, 7)
    m = build_model(be, ocfg, params, dtype)
    m.eval()
    if mode is not None:
        m.generation_mode = mode
    ids, ww, mask, _, _ = synth_batch(ocfg, B, L, 4, seed)
    items = make_items(n_items, seed, hi=min(60, ocfg.vocab_size - 1))
    ct = CompiledTrie.from_sequences(items)
    ct.index_items(items)
    rnd = random.Random(seed + 1)
    excluded = [sorted(rnd.sample(range(n_items), int(frac * n_items) if b else 0)) for b in range(B)]   # user 0: no history
    excluded[-1] = excluded[-1] + excluded[-1][:2]                                                   # duplicates are harmless
    out = m.generate(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=max_len, trie=ct,
                     excluded=ct.excluded_bitmap(excluded), num_beams=K, num_return_sequences=K, output_scores=True,
                     return_dict_in_generate=True)
    tries = [Trie([it for i, it in enumerate(items) if i not in set(ex)]) for ex in excluded]
    with torch.no_grad():
        s_ref, sc_ref = O.beam_search(params, ocfg, ids, ww, mask, lambda b, s: tries[b].get(s.tolist()), K, max_len)
    compare_generation(out["sequences"].cpu(), out["sequences_scores"].cpu(), s_ref, sc_ref, score_tol)
    gen = out["sequences"].view(B, K, -1).cpu().tolist()
    for b in range(B):
        banned = {tuple(items[i]) for i in excluded[b]}
        for k in range(K):
            row = gen[b][k]
            if 1 in row:
                assert tuple(row[:row.index(1) + 1]) not in banned
    return out


def generate_verified_collab_case(be, K, n_layers=2, B=3, L=40, n_items=400, with_excluded=True, seed=3, score_tol=2e-4, ocfg=None, tok_range=(32100, 32599)):
    """BASELINE.json configs[3] in the mode bench.py's `c4_t5base_beam20_b20` leg times: bf16 T5-base dims, vocabulary grown by 500 <CIk>
    tokens (collaborative indexing, main.py:190-193 -> V = 32600), item ids drawn from the added-token range, beam K, `generate()` in its
    default VERIFIED mode (bf16 search with extra beams proposes, one fp32 pass decides, csrc/p5_verify.h) -- token-exact ranked lists and
    scores within `score_tol` of the fp32 oracle's beam search (DistributedRunner.py:361-374), with and without per-user history
    exclusion (DistributedRunner.py:286-297).  K = 22 is the widest verified search; K = 23 must run the plain fp32 search, say so
    (RuntimeWarning, `last_generate_path`) and still return the oracle's lists."""
    import warnings
    from openp5_amd.trie import CompiledTrie
    if ocfg is None:
        ocfg = O.T5Cfg.named("t5-base", num_layers=n_layers, num_decoder_layers=n_layers, vocab_size=32600)
    rnd = random.Random(seed)
    items = set()
    while len(items) < n_items:
        items.add(tuple([0, 5] + [rnd.randint(*tok_range) for _ in range(rnd.randint(2, 4))] + [1]))
    items = sorted(list(x) for x in items)
    params = O.init_params(ocfg, 7)
    m = build_model(be, ocfg, params, "bf16")
    m.eval()
    assert m.generation_mode == "verified"
    ids, ww, mask, _, _ = synth_batch(ocfg, B, L, 4, 5)
    ct = CompiledTrie.from_sequences(items)
    ct.index_items(items)
    out = {}
    variants = [("plain", None)]
    if with_excluded:
        excluded = [sorted(rnd.sample(range(n_items), int(0.5 * n_items) if b else 0)) for b in range(B)]      # user 0: no history
        variants.append(("excluded", excluded))
    for name, excluded in variants:
        kw = {} if excluded is None else {"excluded": ct.excluded_bitmap(excluded)}
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = m.generate(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=30, trie=ct, num_beams=K, num_return_sequences=K,
                             output_scores=True, return_dict_in_generate=True, **kw)
        wide = [w for w in caught if issubclass(w.category, RuntimeWarning) and "verified generation covers" in str(w.message)]
        if K <= m.VERIFY_MAX_K:
            assert m.last_generate_path == "verified" and not wide, (m.last_generate_path, [str(w.message) for w in caught])
        else:
            assert m.last_generate_path == "fp32_search", m.last_generate_path
            assert wide or m._warned_wide_verified, "a verified call wider than VERIFY_MAX_K must say that it ran the fp32 search"
        if excluded is None:
            tries = [Trie(items)] * B
        else:
            tries = [Trie([it for i, it in enumerate(items) if i not in set(ex)]) for ex in excluded]
        with torch.no_grad():
            s_ref, sc_ref = O.beam_search(params, ocfg, ids, ww, mask, lambda b, s: tries[b].get(s.tolist()), K, 30)
        compare_generation(got["sequences"].cpu(), got["sequences_scores"].cpu(), s_ref, sc_ref, score_tol)
        out[name] = {"path": m.last_generate_path, "score_err": float((got["sequences_scores"].cpu() - sc_ref).abs().max())}
    out["verify_stats"] = dict(m.verify_stats)
    return out


def generate_verified_overflow_case(be, ocfg, B=3, L=20, K=5, max_len=12, n_items=40, scale=3.0e5, seed=5, score_tol=5e-5):
    """An FFN hidden layer far outside the range of the two-term fp16 split (|x| >= 2^15, csrc/p5_gemm.h): wi scaled up and wo down by
    the same factor leaves the function the same, the fp32 oracle does not care -- the verification pass must flag every user (range
    guard, csrc/p5_verify.h::p5_verify_range_kernel) and the host re-runs them on the exact-fp32 search: lists still the oracle's."""
    params = O.init_params(ocfg, 7)
    for k in list(params):
        if "DenseReluDense.wi" in k and ".decoder." in "." + k:
            params[k] = params[k] * scale
        if "DenseReluDense.wo" in k and ".decoder." in "." + k:
            params[k] = params[k] / scale
    m = build_model(be, ocfg, params, "bf16")
    m.eval()
    m.verify_escalation = ()          # (a wider draft cannot help an overflowing pass: go straight to the fp32 search)
    ids, ww, mask, _, _ = synth_batch(ocfg, B, L, 4, seed)
    items = make_items(n_items, seed, hi=min(60, ocfg.vocab_size - 1))
    trie = Trie(items)
    got = m.generate(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=max_len, prefix_allowed_tokens_fn=prefix_allowed_tokens_fn(trie),
                     num_beams=K, num_return_sequences=K, output_scores=True, return_dict_in_generate=True)
    with torch.no_grad():
        s_ref, sc_ref = O.beam_search(params, ocfg, ids, ww, mask, lambda b, s: trie.get(s.tolist()), K, max_len)
    compare_generation(got["sequences"].cpu(), got["sequences_scores"].cpu(), s_ref, sc_ref, score_tol)
    st = dict(m.verify_stats)
    assert st["fallback_users"] == B, st
    return st


def train_trajectory_case(be, ocfg, B, L, T, steps=3, dtype="fp32", lr=1e-2, tol=2e-4):
    """N fused steps (forward + backward + clip + HF-AdamW + linear warmup) against the oracle's restatement of the
    reference step (DistributedRunner.py:63-87, SingleRunner.py:178-219): parameter trajectories must coincide."""
    from openp5_amd.optim import FusedAdamW
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": 0.0})
    params = O.init_params(ocfg, 7)
    m = build_model(be, ocfg, params, dtype)
    m.eval()
    total, warm = 10, 2
    opt = FusedAdamW(m, lr=lr, eps=1e-6, weight_decay=0.01, max_grad_norm=1.0, warmup_steps=warm, total_steps=total)
    Pq = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    M1 = {k: torch.zeros_like(v) for k, v in params.items()}
    M2 = {k: torch.zeros_like(v) for k, v in params.items()}
    for step in range(1, steps + 1):
        ids, ww, mask, labels, out_attn = synth_batch(ocfg, B, L, T, 100 + step)
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
        O.runner_loss(nll, out_attn.to(nll.device)).backward()
        opt.step()
        m.zero_grad()
        loss_o = O.runner_loss(O.p5_forward_nll(Pq, ocfg, ids, ww, mask, labels), out_attn)
        grads = torch.autograd.grad(loss_o, list(Pq.values()))
        _, coef = O.clip_coef(grads, 1.0)
        lr_t = O.linear_schedule_lr(lr, step - 1, warm, total)       # lr in effect for this step (scheduler stepped after)
        with torch.no_grad():
            for (k, p), g in zip(Pq.items(), grads):
                O.adamw_hf_step(p, g * coef, M1[k], M2[k], step, lr_t)
    sync(be)
    worst = (0.0, "")
    for name, p in m.named_parameters():
        err = (p.detach().cpu() - Pq[name].detach()).abs().max().item()
        if err > worst[0]:
            worst = (err, name)
    assert worst[0] <= tol, f"parameter trajectory diverged: {worst}"
    return worst


def adamw_golden_case(be, tol=2e-6):
    """p5_grad_sumsq + p5_adamw_step (clip + HF-AdamW in one pass over a flat arena; DistributedRunner.py:81,85-86, SingleRunner.py:191-217)
    held to tests/golden/adamw_426.json -- the published transformers-4.26 AdamW.step / torch-1.8.1 clip_grad_norm_ / linear-warmup
    arithmetic run in fp64 Python (tests/golden/make_adamw_426.py).  fp32 kernel vs fp64 fixture: `tol` relative to each tensor's scale."""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_426.json")))
    h, names = gold["hyper"], list(gold["shapes"])
    flat = lambda d: torch.tensor([x for k in names for x in d[k]], dtype=torch.float64)     # noqa: E731
    p = dev(be, flat(gold["p0"]).float())
    n = p.numel()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sumsq = dev(be, torch.zeros(1024))
    shadow = dev(be, torch.zeros(n, dtype=torch.bfloat16))
    worst = 0.0
    for t, st in enumerate(gold["steps"], start=1):
        g = dev(be, flat(st["grad"]).float())
        be.check(be.lib.p5_grad_sumsq(P(g), n, P(sumsq), be.stream_ptr()), "p5_grad_sumsq")
        be.check(be.lib.p5_adamw_step(P(p), P(g), P(m), P(v), P(shadow), n, P(sumsq), h["max_norm"], 1.0, st["lr"], h["beta1"], h["beta2"], h["eps"],
                                      h["weight_decay"], t, be.stream_ptr()), "p5_adamw_step")
        sync(be)
        assert abs(math.sqrt(float(sumsq.double().sum())) - st["total_norm"]) <= 1e-5 * st["total_norm"]
        for name, got in (("p", p), ("m", m), ("v", v)):
            ref = flat(st[name])
            err = float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
            worst = max(worst, err)
            assert err <= tol, (t, name, err)
        assert torch.equal(shadow.cpu(), p.cpu().to(torch.bfloat16)), "the bf16 compute shadow is the updated master value rounded once"
    return worst


def ce_free_case(be, ocfg, B, L, T, dropout=0.0, min_tiles=None, seed=3):
    """Logit-free cross-entropy (csrc p5_gemm5.h P5_EPI_CE_STATS / _GRAD): the bf16 training step whose head never writes the
    [B*T, V] logits against the same step with the materialised logits (option ce_free 0): per-token NLL and every gradient agree to the
    rounding of the log-sum-exp's summation order.  min_tiles: lowers the wide kernel's tile threshold so that toy shapes take that path."""
    out = {}
    for free in (1, 0):
        be.check(be.lib.p5_set_option(b"ce_free", free), "opt")
        if min_tiles is not None:
            be.check(be.lib.p5_set_option(b"gemm_wide_min_tiles", min_tiles), "opt")
        try:
            m = build_model(be, ocfg, O.init_params(ocfg, 7), "bf16", dropout=dropout)
            m.train()
            ids, ww, mask, labels, out_attn = synth_batch(ocfg, B, L, T, seed)
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn)
            sync(be)
            out[free] = (float(loss), m._grads.detach().float().cpu().clone())
        finally:
            be.lib.p5_set_option(b"ce_free", 1)
            be.lib.p5_set_option(b"gemm_wide_min_tiles", 160)
    (l1, g1), (l0, g0) = out[1], out[0]
    assert abs(l1 - l0) <= 2e-5 * max(1.0, abs(l0)), (l1, l0)
    rel = float((g1 - g0).norm() / g0.norm().clamp(min=1e-30))
    assert rel <= 2e-3, f"logit-free vs materialised gradients differ by {rel}"
    return l1, l0, rel


def adamw_tiles_case(be, ocfg, steps=3, seed=11):
    """p5_engine_adamw_step's tile-wise update (the AdamW pass writes the transposed copy W^T and the norm-folded copy W diag(ln) itself,
    csrc p5_adamw_tiles_kernel) against the flat update followed by p5_refresh_transposed: parameters, both moments, the bf16 shadow and the
    whole transposed / folded buffer bit-identical after several steps (so the norm weights' moments are non-trivial when they are re-derived)."""
    from openp5_amd.optim import FusedAdamW
    out = {}
    for tiles in (1, 0):
        be.check(be.lib.p5_set_option(b"adam_tiles", tiles), "opt")
        try:
            m = build_model(be, ocfg, O.init_params(ocfg, 7), "bf16")
            opt = FusedAdamW(m, lr=1e-2, eps=1e-6, weight_decay=0.01, max_grad_norm=1.0, warmup_steps=1, total_steps=10)
            g = torch.Generator().manual_seed(seed)
            m._sync_shadow(); m._sync_transposed()
            for st in range(steps):
                m._grads.copy_(dev(be, torch.randn(m._grads.numel(), generator=g) * (0.05 if st % 2 else 2.0)))
                m._grads_dead = False
                opt.step()
                assert m._tr_dirty == (tiles == 0), "the tile-wise step leaves the copies fresh, the flat one does not"
                m._sync_shadow(); m._sync_transposed()
            sync(be)
            nb = 2 * int(m._n)
            fold_off = int(be.lib.p5_transposed_bytes(m._engine)) - nb - 256       # (the descriptor table in between has uninitialised padding bytes)
            out[tiles] = [t.detach().cpu().clone() for t in (m._flat, opt.m, opt.v, m._shadow.view(torch.int16), m._shadow_t[:nb],
                                                              m._shadow_t[fold_off:fold_off + nb])]
        finally:
            be.lib.p5_set_option(b"adam_tiles", 1)
    for name, a, b in zip(("params", "m", "v", "shadow", "transposed copy", "norm-folded copy"), out[1], out[0]):
        assert torch.equal(a, b), f"tile-wise AdamW differs from flat AdamW + refresh in {name}: {(a != b).sum().item()} elements"
    return True


def bf16_training_converges_case(be, steps=40):
    """fast mode sanity: fused bf16 training on one fixed batch drives the masked loss down (dropout on)."""
    from openp5_amd.optim import FusedAdamW
    ocfg = O.T5Cfg.named("tiny", dropout=0.1)
    params = O.init_params(ocfg, 3)
    m = build_model(be, ocfg, params, "bf16", dropout=0.1)
    m.train()
    m.set_dropout_seed(11, 0)
    opt = FusedAdamW(m, lr=3e-3, max_grad_norm=1.0)
    ids, ww, mask, labels, out_attn = synth_batch(ocfg, 8, 24, 6, 77)
    first = last = None
    for _ in range(steps):
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
        loss = O.runner_loss(nll, out_attn.to(nll.device))
        loss.backward()
        opt.step()
        m.zero_grad()
        v = float(loss.detach())
        first = v if first is None else first
        last = v
    assert last < 0.6 * first, (first, last)
    return first, last


def fused_loss_case(be, ocfg, B, L, T, dtype="fp32", dropout=0.0, seed=9, tol=1e-6):
    """`P5T5Native.loss_and_backward` (p5_forward_loss + mask-seeded backward, DistributedRunner.py:63-80 in one engine call)
    == forward() -> torch masked-mean -> autograd backward on the same inputs: same loss, same gradient arena."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = synth_batch(ocfg, B, L, T, seed)
    out_attn[0, :] = 0          # a row with an empty label mask exercises clamp(min=1)
    res = []
    for fused in (False, True):
        m = build_model(be, ocfg, params, dtype, dropout)
        if dropout > 0:
            m.train()
            m.set_dropout_seed(77, 0)
        else:
            m.eval()
        if fused:
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn)
        else:
            nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
            loss = O.runner_loss(nll, out_attn.to(nll.device))
            loss.backward()
        sync(be)
        res.append((float(loss.detach()), m._grads.detach().cpu().clone()))
    (l0, g0), (l1, g1) = res
    assert abs(l0 - l1) <= tol * max(1.0, abs(l0)), (l0, l1)
    err = (g0 - g1).abs().max().item() / max(1e-12, g0.abs().max().item())
    assert err <= (tol if dtype == "fp32" else 2e-2), f"fused-loss gradient differs: {err}"
    return l1, err


# ---------------------------------------------------------------------------------------------------------
# dataset-level evaluation parity (north_star: "ranked Hit@k identical")
# ---------------------------------------------------------------------------------------------------------
def make_pipeline(be, tmp, dtype, dataset="ML100K", n_users=120, n_items=150, n_inter=2400, flags=(), seed=2023, dropout=0.1, model_cfg=None,
                  vocab=None):
    """synthetic user sequences -> datasets -> sampler -> collator -> P5T5Native (T5-small dims) -> runner, as main.py wires it."""
    from torch.utils.data import ConcatDataset, DataLoader
    from openp5_amd.collator import Collator
    from openp5_amd.data import MultiTaskDataset
    from openp5_amd.runner import DistributedRunner, build_arg_parser
    from openp5_amd.sampler import SingleMultiDataTaskSampler
    from openp5_amd.synth import write_dataset, write_prompt_file
    from openp5_amd.tokenizer import build_offline_tokenizer
    from openp5_amd.utils.initialization import random_initialization
    write_dataset(os.path.join(tmp, "data"), dataset, n_users=n_users, n_items=n_items, n_inter=n_inter)
    prompt = write_prompt_file(os.path.join(tmp, "prompt.txt"))
    args = build_arg_parser().parse_args(["--data_path", os.path.join(tmp, "data"), "--datasets", dataset, "--tasks", "sequential,straightforward",
                                          "--item_indexing", "sequential", "--prompt_file", prompt, "--sample_prompt", "1", "--sample_num", "2,2",
                                          "--max_his", "10", "--distributed", "0", "--batch_size", "32", "--eval_batch_size", "10",
                                          "--test_before_train", "0", "--test_epoch", "0", "--compute_dtype", dtype] + list(flags))
    args.rank = 0
    args.model_path = os.path.join(tmp, "model.pt")
    # as main.py:61 does before it builds anything (utils.set_seed): `random_initialization` below draws from torch's DEVICE generator,
    # whose default seed differs from process to process -- without this the "same" pipeline starts from different embeddings in every
    # run (the five different trajectories of tests/test_gpu_dataset.py in round 4 were five different initialisations, not five
    # outcomes of one training: the training itself is bit-reproducible)
    from openp5_amd.utils.utils import set_seed
    set_seed(seed)
    random.seed(0)
    tok = build_offline_tokenizer(vocab) if vocab else build_offline_tokenizer()
    train = ConcatDataset([MultiTaskDataset(args, dataset, "train")])
    loader = DataLoader(train, sampler=SingleMultiDataTaskSampler(train, args.batch_size, args.seed), batch_size=args.batch_size,
                        collate_fn=Collator(tok))
    cfg = model_cfg or P5ModelConfig.from_backbone("t5-small", dropout_rate=dropout)
    model = P5T5Native(cfg, dtype=dtype, backend=be, seed=seed)
    model.resize_token_embeddings(len(tok))
    random_initialization(model, tok, "t5-small")
    return DistributedRunner(model, tok, loader, None, be.device, args, 0), model, tok, args


def collect_rankings(runner, gen_fn, K, max_length=50):
    """Per test loader, per user: (gold token tuple, K ranked item token tuples, K scores) -- the inputs of
    evaluate.rel_results (DistributedRunner.py:376-387) before they are collapsed into Hit/NDCG sums."""
    out = []
    for loader in runner.testloaders:
        ds = loader.dataset
        trie, ct, _ = runner._dataset_trie(ds)
        users = []
        for batch in loader:
            seq, score = gen_fn(batch, trie, ct, K, max_length)
            seq, score = seq.cpu(), score.cpu().float()
            B = batch[0].shape[0]
            seq = seq.view(B, K, -1)
            score = score.view(B, K)
            order = torch.sort(score, dim=1, descending=True, stable=True).indices
            for b in range(B):
                gold = tuple(t for t in batch[3][b].tolist() if t != 0)
                ranked = [tuple(t for t in seq[b, j].tolist()[1:] if t != 0) for j in order[b].tolist()]
                users.append((gold, ranked, score[b][order[b]].tolist()))
        out.append(users)
    return out


def _pack_sequences(chunk, K, which=1):
    T = 1 + max(len(it) for u in chunk for it in u[which])
    seqs = torch.zeros(len(chunk), K, T + 1, dtype=torch.long)
    for b, u in enumerate(chunk):
        for j, it in enumerate(u[which]):
            seqs[b, j, 1:1 + len(it)] = torch.tensor(it)
    return seqs


def dropped_gap(x, x_lp, ranked, ranked_lp):
    """How an item `x` that a beam search does NOT return can have been dropped, judged in the oracle's scores (`x_lp`, `ranked_lp`:
    oracle per-token log-probabilities of x and of the K returned items).  A beam search drops a path at the first step t at which its
    prefix is not among the kept ones, and every prefix it kept to the end scored at least as high there: so for SOME t from the first
    step at which x[:t] is no prefix of a returned item, the running sum of x must not exceed the smallest running sum of the returned
    items that are at least t tokens long -- or, at t = len(x), its final (per-token mean) score must not exceed theirs.  Returns the
    smallest violation over those t, per token (0.0 = the drop is consistent with an exact search; a lower-precision search is allowed
    its tie tolerance).  inf if x shares every prefix with a returned item (cannot happen for x not returned)."""
    best = float("inf")
    for t in range(1, len(x) + 1):
        if any(tuple(y[:t]) == tuple(x[:t]) for y in ranked):
            continue
        peers = [sum(lp[:t]) for y, lp in zip(ranked, ranked_lp) if len(y) >= t]
        if not peers:
            continue
        best = min(best, max(0.0, (sum(x_lp[:t]) - min(peers)) / t))
    return best


def list_difference(ranked, ref, r_lp, ro, so, o_lp):
    """What separates the list a search returned (`ranked`, oracle scores `ref`, oracle per-token log-probabilities `r_lp`) from the
    oracle's own list (`ro`, `so`, `o_lp`), all in ORACLE scores (per-token means):
      missed   -- how far an item only the oracle lists lies above the search's K-th item, and
      extra    -- how far an item only the search lists lies below the oracle's K-th item (both 0 on an exact ranking BY FINAL SCORE --
                  which a beam search is not: the K-th item can be one whose forced completion is poor and that both lists hold, e.g.
                  the gate's trie, where one five-token prefix is in every user's top 10 and its </s> costs -3.8: `missed` then says 0.6
                  for an exchange between two items that tie to 1e-3);
      exchange -- the best item only the oracle lists minus the worst item only the search lists: the final-score gap of what was
                  actually exchanged;
      dropped  -- the largest dropped_gap of the items only the oracle lists: whether the search was entitled to drop them."""
    kth, okth = min(ref), min(so)
    only_o = [i for i, it in enumerate(ro) if it not in ranked]
    only_s = [j for j, it in enumerate(ranked) if it not in ro]
    return {"missed": max([so[i] - kth for i in only_o] + [0.0]),
            "extra": max([okth - ref[j] for j in only_s] + [0.0]),
            "exchange": max(0.0, max(so[i] for i in only_o) - min(ref[j] for j in only_s)) if only_o and only_s else 0.0,
            "dropped": max([dropped_gap(ro[i], o_lp[i], ranked, r_lp) for i in only_o] + [0.0])}


_ORACLE_TOKEN_LP = {}


def teacher_forced_check(runner, params, ocfg, rankings, K, score_tol, order_tol, oracle_rankings=None):
    """Every hypothesis a search returned, scored by the ORACLE on the same token sequence (O.sequence_scores): per user
    (a) max |returned score - oracle score of that sequence|, (b) the largest inversion of the returned order under the oracle's
    scores, (c) what separates the returned list from the oracle's own (`list_difference`: missed / extra / exchange / dropped, one
    entry per user).  Unlike the margin-based robustness classes this check applies to EVERY user: it does not ask the two searches to
    have decided alike, only that what the search returns is correctly scored and ordered and that what it dropped could be dropped.
    `detail` keeps the per-token log-probabilities of both lists (for a dump)."""
    out = {"users": 0, "max_score_err": 0.0, "max_inversion": 0.0, "score_viol": 0, "order_viol": 0, "missed": [], "extra": [], "exchange": [],
           "dropped": [], "detail": []}
    li = 0
    for loader, users in zip(runner.testloaders, rankings):
        ui = 0
        for batch in loader:
            B = batch[0].shape[0]
            chunk = users[ui:ui + B]
            with torch.no_grad():
                ref, tok, _ = O.sequence_scores(params, ocfg, batch[0], batch[2], batch[1], _pack_sequences(chunk, K), True)
                if oracle_rankings is not None:
                    # (the oracle's token log-probabilities of its OWN lists do not depend on the engine under test: computed once per gate)
                    key = (id(oracle_rankings), li, ui)
                    if key not in _ORACLE_TOKEN_LP:
                        _ORACLE_TOKEN_LP[key] = O.sequence_scores(params, ocfg, batch[0], batch[2], batch[1],
                                                                   _pack_sequences(oracle_rankings[li][ui:ui + B], K), True)[1]
                    otok = _ORACLE_TOKEN_LP[key]
            for b, (_, ranked, sc) in enumerate(chunk):
                err = max(abs(float(ref[b, j]) - sc[j]) for j in range(K))
                if err > out["max_score_err"]:
                    jw = max(range(K), key=lambda j: abs(float(ref[b, j]) - sc[j]))
                    out["worst_score"] = {"oracle": float(ref[b, jw]), "returned": float(sc[jw]), "rank": jw, "token_lp_oracle": [round(x, 3) for x in tok[b, jw].tolist()]}
                inv = max([float(ref[b, j + 1] - ref[b, j]) for j in range(K - 1)] + [0.0])
                out["users"] += 1
                out["max_score_err"] = max(out["max_score_err"], err)
                out["max_inversion"] = max(out["max_inversion"], inv)
                out["score_viol"] += int(err > score_tol)
                out["order_viol"] += int(inv > order_tol)
                if oracle_rankings is not None:
                    _, ro, so = oracle_rankings[li][ui + b]
                    r_lp = [tok[b, j].tolist() for j in range(K)]
                    o_lp = [otok[b, j].tolist() for j in range(K)]
                    for k, v in list_difference(ranked, ref[b].tolist(), r_lp, ro, so, o_lp).items():
                        out[k].append(v)
                    out["detail"].append((r_lp, o_lp))
            ui += B
        li += 1
    return out


def rankings_metrics(rankings, metrics=("hit@5", "hit@10", "ndcg@5", "ndcg@10")):
    from openp5_amd import evaluate
    res = []
    for users in rankings:
        rel = [[1 if r == gold else 0 for r in ranked] for gold, ranked, _ in users]
        res.append(dict(zip(metrics, (evaluate.get_metrics_results(rel, list(metrics)) / max(1, len(rel))).tolist())))
    return res


def engine_gen_fn(model):
    def fn(batch, trie, ct, K, max_length):
        dev_ = model._be.device
        o = model.generate(input_ids=batch[0].to(dev_), attention_mask=batch[1].to(dev_), whole_word_ids=batch[2].to(dev_), max_length=max_length,
                           trie=ct, num_beams=K, num_return_sequences=K, output_scores=True, return_dict_in_generate=True)
        return o["sequences"], o["sequences_scores"]
    return fn


def oracle_gen_fn(params, ocfg, margins=None):
    """`margins` (optional list): receives, per user in evaluation order, (set_margin, [gaps between consecutive final scores])
    -- the smallest score margins by which the oracle's beam search took its decisions for that user (oracle/t5_oracle.py), all in
    the unit of the final scores (per-token means: comparisons of running sums are divided by the number of tokens summed)."""
    def fn(batch, trie, ct, K, max_length):
        dm = {} if margins is not None else None
        with torch.no_grad():
            out = O.beam_search(params, ocfg, batch[0], batch[2], batch[1], lambda b, s: trie.get(s.tolist()), K, max_length,
                                decision_margins=dm)
        if margins is not None:
            for b in range(batch[0].shape[0]):
                margins.append((float(dm["set_per_token"][b]), [float(x) for x in dm["order"][b]]))
        return out
    return fn


def robust_users(rankings_oracle, margins, tol):
    """Which users' results a lower-precision search MUST reproduce, given score errors below tol / 2.
    list-robust: every decision of the oracle's search for the user (candidate sets AND final order) had margin > tol;
    metric-robust: the candidate-set decisions had margin > tol and the gold item's final score is separated by > tol from its
    neighbours in the list (or the gold item is absent), so Hit@k / NDCG@k of the user cannot move."""
    flat = [u for users in rankings_oracle for u in users]
    assert len(flat) == len(margins)
    out = []
    for (gold, ranked, scores), (set_m, gaps) in zip(flat, margins):
        list_ok = set_m > tol and all(g > tol for g in gaps)
        if gold in ranked:
            k = ranked.index(gold)
            near = [gaps[j] for j in (k - 1, k) if 0 <= j < len(gaps)]
            metric_ok = set_m > tol and all(g > tol for g in near)
        else:
            metric_ok = set_m > tol
        out.append((list_ok, metric_ok))
    return out


def lists_equal_up_to_ties(ra, rb, sb, tol):
    """ranked list `ra` equals the reference list `rb` up to reordering items whose REFERENCE scores `sb` differ by <= tol:
    wherever the two lists disagree, the item `ra` puts there must sit in `rb` at a position whose score is within tol."""
    if len(ra) != len(rb):
        return False
    for i, (x, y) in enumerate(zip(ra, rb)):
        if x == y:
            continue
        if x not in rb or abs(sb[rb.index(x)] - sb[i]) > tol:
            return False
    return True


def compare_rankings(a, b, K_list=(5, 10), tie_tol=0.0):
    """users whose ranked lists / gold ranks differ between two evaluations of the same loaders (`b` = the reference)."""
    stats = {"users": 0, "identical_lists": 0, "identical_up_to_ties": 0, "same_topk_set": {k: 0 for k in K_list}, "same_gold_rank": 0,
             "max_score_diff": 0.0, "diff_users": []}
    for la, lb in zip(a, b):
        for i, ((ga, ra, sa), (gb, rb, sb)) in enumerate(zip(la, lb)):
            assert ga == gb
            stats["users"] += 1
            stats["identical_lists"] += int(ra == rb)
            stats["identical_up_to_ties"] += int(lists_equal_up_to_ties(list(ra), list(rb), list(sb), tie_tol))
            for k in K_list:
                stats["same_topk_set"][k] += int(set(ra[:k]) == set(rb[:k]))
            rka = ra.index(ga) if ga in ra else -1
            rkb = rb.index(gb) if gb in rb else -1
            stats["same_gold_rank"] += int(rka == rkb)
            if rka != rkb:
                stats["diff_users"].append((i, rka, rkb))
            # score accuracy on the items BOTH evaluations list (scores of different items say nothing about accuracy)
            common = [(sa[ra.index(it)], sb[rb.index(it)]) for it in ra if it in rb]
            if common:
                stats["max_score_diff"] = max(stats["max_score_diff"], max(abs(x - y) for x, y in common))
    return stats


def grad_agreement(m, Pq):
    """per-tensor relative L2 error and cosine of the engine's gradients against the oracle's, plus the whole-gradient figures."""
    rows = []
    for name, p in m.named_parameters():
        g, go = p.grad.detach().cpu().double().flatten(), Pq[name].grad.detach().double().flatten()
        rows.append((float((g - go).norm() / (go.norm() + 1e-30)), float((g @ go) / (g.norm() * go.norm() + 1e-30)), name))
    allg = torch.cat([p.grad.detach().cpu().double().flatten() for _, p in m.named_parameters()])
    allo = torch.cat([Pq[n].grad.detach().double().flatten() for n, _ in m.named_parameters()])
    whole = (float((allg - allo).norm() / allo.norm()), float((allg @ allo) / (allg.norm() * allo.norm())))
    return rows, whole


def bf16_gradient_case(be, ocfg, B, L, T, dropout=0.0, seed=3):
    """bf16 engine against the fp32 oracle at a given model size / shape: per-token NLL, every gradient tensor (relative L2 error +
    cosine), the whole gradient.  With dropout > 0 both sides draw the SAME masks (counter-based RNG restated in the oracle)."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = synth_batch(ocfg, B, L, T, seed)
    Pq = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    dp = O.DropoutPlan((1234 + 1 * 0x632BE5AB) & 0xFFFFFFFF, dropout) if dropout > 0 else None
    nll_o = O.p5_forward_nll(Pq, ocfg, ids, ww, mask, labels, dp)
    O.runner_loss(nll_o, out_attn).backward()
    m = build_model(be, ocfg, params, "bf16", dropout)
    if dropout > 0:
        m.train()
        m.set_dropout_seed(1234, 0)
    else:
        m.eval()
    loss = m.loss_and_backward(ids, ww, mask, labels, out_attn)
    sync(be)
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    if dropout > 0:
        m.set_dropout_seed(1234, 0)       # the same masks for the NLL read-back
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"].detach().cpu()
    for n, p in m.named_parameters():
        p.grad = grads[n]
    e = (nll - nll_o.detach()).abs()
    rows, whole = grad_agreement(m, Pq)
    return dict(nll_max=float(e.max()), nll_mean=float(e.mean()), loss_err=abs(float(loss) - float(O.runner_loss(nll_o, out_attn))),
                worst_rel=max(rows), worst_cos=min((r[1], r[2]) for r in rows), whole_rel=whole[0], whole_cos=whole[1])


def grad_arena_coverage_case(be, ocfg, B, L, T, dtype="bf16"):
    """zero_grad() leaves the gradient arena DEAD, not cleared: the next backward must write every parameter's gradient itself (store
    it, or clear it before accumulating into it).  Poison the arena with NaN behind zero_grad(): after the backward no parameter's
    gradient may contain a NaN, and all of them must equal the gradients of a fresh model's first backward."""
    params = O.init_params(ocfg, 7)
    a = synth_batch(ocfg, B, L, T, 3)
    b = synth_batch(ocfg, B, L, T, 4)
    ref = build_model(be, ocfg, params, dtype, 0.0)
    ref.eval()
    ref.loss_and_backward(*b)
    sync(be)
    want = ref._grads.detach().cpu().clone()
    m = build_model(be, ocfg, params, dtype, 0.0)
    m.eval()
    m.loss_and_backward(*a)
    m.zero_grad()
    sync(be)
    m._grads.fill_(float("nan"))
    m.begin_micro_batch(first=True, sync=False)
    m.loss_and_backward(*b)
    sync(be)
    got = m._grads.detach().cpu()
    for n, (o, k, _) in m._views.items():
        g = got[o:o + k]
        assert not bool(torch.isnan(g).any()), f"{n}: gradient not (fully) written by a backward that follows zero_grad()"
        assert torch.allclose(g, want[o:o + k], rtol=1e-5, atol=1e-7), (n, float((g - want[o:o + k]).abs().max()))


def backward_reproducible_case(be, ocfg, B, L, T, runs=4, dropout=0.0, dtype="bf16"):
    """The same step on fresh models: the loss and EVERY gradient must come out bit-identical.  Since round 4 no gradient of the engine
    is a sum of fp32 atomics (embedding lookups: fixed-order segmented sums, p5_embed.h; relative-bias tables: per-workgroup slots;
    T5LayerNorm weights: fixed-association partial sums; weight gradients: one writer per element), so there is no exception list --
    AdamW turns a last-bit difference of a near-zero gradient into an O(lr) parameter difference, which is how the run-to-run
    differences of round 3 arose (profiles/r04_repro_before_fix.txt)."""
    params = O.init_params(ocfg, 7)
    a = synth_batch(ocfg, B, L, T, 3)
    outs = []
    for r in range(runs):
        m = build_model(be, ocfg, params, dtype, dropout)
        if dropout > 0:
            m.train()
            m.set_dropout_seed(41, 5)
        else:
            m.eval()
        loss = m.loss_and_backward(*a)
        sync(be)
        outs.append((float(loss), m._grads.detach().cpu().clone()))
        views = dict(m._views)
    for r in range(1, runs):
        assert outs[r][0] == outs[0][0], (r, outs[r][0], outs[0][0])
        bad = [(n, float((outs[r][1][o:o + k] - outs[0][1][o:o + k]).abs().max())) for n, (o, k, _) in views.items()
               if not torch.equal(outs[r][1][o:o + k], outs[0][1][o:o + k])]
        assert not bad, (r, bad[:8], len(bad))


def attn_keep_bits_case(be, ocfg, B, L, T, dropout=0.1):
    """bf16, 128 < L <= 512, dropout on: the head-resident attention forward stores its keep decisions as lane masks and the two backward
    passes read them (P5AttnArgs::keep_bits; workspace laid out per encoder layer) instead of re-evaluating the counter-based hash --
    the SAME decisions, so the loss and every gradient are bit-identical to the hashed path (option attn_keep_bits 0) and to the blocked
    kernels' masks (the gradient gates against the oracle's mask run elsewhere)."""
    params = O.init_params(ocfg, 7)
    a = synth_batch(ocfg, B, L, T, 3)
    outs = []
    try:
        for bits in (1, 0, 1):
            be.check(be.lib.p5_set_option(b"attn_keep_bits", bits), "set_option")
            m = build_model(be, ocfg, params, "bf16", dropout)
            m.train()
            m.set_dropout_seed(41, 5)
            loss = m.loss_and_backward(*a)
            sync(be)
            outs.append((float(loss), m._grads.detach().cpu().clone()))
            views = dict(m._views)
    finally:
        be.check(be.lib.p5_set_option(b"attn_keep_bits", 1), "set_option")
    assert outs[0][1].abs().max() > 0
    for r in (1, 2):
        assert outs[r][0] == outs[0][0], (r, outs[r][0], outs[0][0])
        bad = [(n, float((outs[r][1][o:o + k] - outs[0][1][o:o + k]).abs().max())) for n, (o, k, _) in views.items()
               if not torch.equal(outs[r][1][o:o + k], outs[0][1][o:o + k])]
        assert not bad, (r, bad[:8], len(bad))


def staged_backward_case(be, ocfg, B, L, T, dtype="bf16", dropout=0.0):
    """The staged backward of the data-parallel path (p5_backward_staged = every p5_backward_stage + p5_backward_final_range in one call): the ranges it reports are
    contiguous, walk the arena from the back and tile it exactly; every gradient equals the whole backward's bit for bit -- with and
    without two-layer weight-gradient groups (p5_backward_stage_pairs)."""
    import ctypes
    params = O.init_params(ocfg, 7)
    a = synth_batch(ocfg, B, L, T, 3)

    def run(staged, pairs):
        m = build_model(be, ocfg, params, dtype, dropout)
        if dropout > 0:
            m.train()
            m.set_dropout_seed(41, 5)
        else:
            m.eval()
        m.staged_backward = staged
        be.check(be.lib.p5_backward_stage_pairs(m._engine, 1 if pairs else 0), "pairs")
        loss = m.loss_and_backward(*a)
        sync(be)
        # what the one-call staged backward (p5_backward_staged) reported: the gradient ranges in the order they became final
        ranges = [(int(m._staged_ranges[2 * k]), int(m._staged_ranges[2 * k + 1])) for k in range(m._staged_n)] if staged else []
        nst = int(be.lib.p5_backward_num_stages(m._engine))
        return float(loss), m._grads.detach().cpu().clone(), ranges, int(m._n), nst

    l0, g0, _, n, _ = run(False, True)
    for pairs in (True, False):
        l1, g1, ranges, _, nst = run(True, pairs)
        assert l1 == l0
        assert torch.equal(g1, g0), (pairs, float((g1 - g0).abs().max()))
        got = [r for r in ranges if r[1] > r[0]]
        assert got and got[-1][0] == 0 and got[0][1] == n, got
        for (b0, e0), (b1, e1) in zip(got, got[1:]):
            assert e1 == b0, ("ranges must tile the arena from the back", got)
        if pairs and ocfg.num_layers >= 2 and B * L % 64 == 0 and B * T % 64 == 0 and dtype == "bf16":
            assert len(got) < nst, "two-layer groups: some stages must report nothing"


def grad_store_first_case(be, ocfg, B, L, T, exact=True):
    """A backward that starts a new accumulation group STORES the Linear gradients over whatever the arena holds (no clear): its
    result must equal the clear-then-accumulate path's on the same batch, after an unrelated backward has left its gradients
    behind; and a second micro-batch (begin_micro_batch(first=False)) must add to it."""
    params = O.init_params(ocfg, 7)
    a = synth_batch(ocfg, B, L, T, 3)
    b = synth_batch(ocfg, B, L, T, 4)
    got = {}
    try:
        for mode in (1, 0):
            be.check(be.lib.p5_set_option(b"grad_store_first", mode), "opt")
            m = build_model(be, ocfg, params, "bf16", 0.0)
            m.eval()
            m.loss_and_backward(*a)                 # leaves gradients behind
            m.zero_grad()                           # (dead, not cleared)
            m.begin_micro_batch(first=True, sync=False)
            m.loss_and_backward(*b)
            sync(be)
            g1 = m._grads.detach().cpu().clone()
            m.begin_micro_batch(first=False, sync=False)
            m.loss_and_backward(*a)
            sync(be)
            got[mode] = (g1, m._grads.detach().cpu().clone())
            views = dict(m._views)
    finally:
        be.lib.p5_set_option(b"grad_store_first", 1)
    for i in (0, 1):
        if exact:
            assert torch.equal(got[1][i], got[0][i]), (i, float((got[1][i] - got[0][i]).abs().max()))
        else:       # (the embedding scatter's fp32 atomics land in a different order every run)
            scale = float(got[0][i].abs().max())
            bad = [(n, float((got[1][i][o:o + k] - got[0][i][o:o + k]).abs().max()), float(got[0][i][o:o + k].abs().max()))
                   for n, (o, k, _) in views.items() if float((got[1][i][o:o + k] - got[0][i][o:o + k]).abs().max()) > 1e-5 * scale]
            assert not bad, (i, scale, bad[:8])
    assert float((got[1][1] - got[1][0]).abs().max()) > 0


def bf16_c2_gradient_case(be, B=64, L=128, T=8):
    """The benchmarked mode at the benchmarked shape (BASELINE.json configs[1]: T5-small, B=64, L=128, T=8, bf16 engine)."""
    return bf16_gradient_case(be, O.T5Cfg.named("t5-small", dropout=0.0), B, L, T)


def relu_flip_audit(taps, eps):
    """{(stack, layer): set of hidden units f with some |ReLU pre-activation| < eps} from the fp64 oracle taps."""
    out = {}
    for k, pre in taps.items():
        if not k.endswith(".pre"):
            continue
        parts = k.split(".")            # encoder.block.i.layer.j.pre
        near = (pre.abs() < eps).reshape(-1, pre.shape[-1]).any(0)
        out[(parts[0], int(parts[2]))] = set(torch.nonzero(near).flatten().tolist())
    return out


def fp32_vs_fp64_case(be, ocfg, B, L, T, tol=1e-3, audit_eps=2e-6, seed=3):
    """fp32 engine against the oracle evaluated in fp64 (the ground truth both fp32 evaluations approximate).  An fp32 ReLU
    pre-activation within rounding noise of zero may land on either side of it -- a different, equally valid fp32 evaluation
    whose gradient differs by O(1) in that element.  Audit: hidden units with |fp64 pre-activation| < audit_eps at some token are
    listed per layer; a wi row of such a unit may exceed `tol` (an evidenced, explained flip).  A flip perturbs one token's
    gradient in everything it back-propagates into (the same sub-layer's norm weight, every earlier layer of the stack, the
    whole encoder for a decoder flip, the embeddings), so those tensors are held to a relative-L2 bound of 2 * tol (robust to
    a single token's contribution) and a max-abs bound of 20 * tol; every tensor that no evidenced flip reaches must meet the
    max-abs `tol` itself.  Without flips (T5-small/base dims in practice) the check is the plain max-abs one."""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = synth_batch(ocfg, B, L, T, seed)
    P64 = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    taps = {}
    O.runner_loss(O.p5_forward_nll(P64, ocfg, ids, ww, mask, labels, taps=taps), out_attn.double()).backward()
    m = build_model(be, ocfg, params, "fp32")
    m.eval()
    m.loss_and_backward(ids, ww, mask, labels, out_attn)
    sync(be)
    near = relu_flip_audit(taps, audit_eps)
    gmax = max(float(v.grad.abs().max()) for v in P64.values())
    errs, excused, flip = {}, [], {"encoder": -1, "decoder": -1}
    for name, p in m.named_parameters():
        g, g64 = p.grad.detach().cpu().double(), P64[name].grad
        err = (g - g64).abs() / (float(g64.abs().max()) + 1e-2 * gmax)
        if ".DenseReluDense.wi" in name:
            parts = name.split(".")
            units = sorted(near.get((parts[0], int(parts[2])), ()))
            if units and float(err[units, :].max()) > tol:
                excused.append((name, len(units), float(err[units, :].max())))
                flip[parts[0]] = max(flip[parts[0]], int(parts[2]))
                err[units, :] = 0
        errs[name] = (float(err.max()), float((g - g64).norm() / (g64.norm() + 1e-30)))

    def reached(name):      # can an evidenced flip have perturbed this tensor's gradient?
        parts = name.split(".")
        if name.startswith("encoder.block."):
            return int(parts[2]) <= flip["encoder"] or flip["decoder"] >= 0
        if name.startswith("decoder.block."):
            return int(parts[2]) <= flip["decoder"]
        if name == "decoder.final_layer_norm.weight":
            return False
        if name == "encoder.final_layer_norm.weight":
            return flip["decoder"] >= 0
        return flip["encoder"] >= 0 or flip["decoder"] >= 0

    worst = (0.0, "")
    for name, (emax, erel) in errs.items():
        if reached(name):
            assert erel <= 2 * tol and emax <= 20 * tol, f"{name}: relL2 {erel:.3e} max {emax:.3e} (reached by an audited ReLU flip; excused {excused})"
        else:
            assert emax <= tol, f"fp32 gradient mismatch {name}: {emax:.3e} > {tol} (no audited flip reaches it; excused {excused})"
        worst = max(worst, (emax, name))
    return worst, excused, {k: len(v) for k, v in near.items() if v}


def skinny_gemm_case(be, dtype, amode, M, N, K, epi, seed=0):
    """decode-step projection kernel (p5_decode2.h) against torch: plain / ReLU / fp32-atomic-accumulate epilogues, optional
    fused T5LayerNorm of the fp32 A rows."""
    g = torch.Generator().manual_seed(seed)
    tt = TT[dtype]
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(tt)
    if amode == 1:
        x = torch.randn(M, K, generator=g) * 3.0
        ln = 1.0 + 0.1 * torch.randn(K, generator=g)
        xn = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)).to(tt).float()
        A_ref = (ln * xn).to(tt).float()
        A_dev, lda = x, K
    else:
        A = torch.randn(M, K, generator=g).to(tt)
        A_ref, A_dev, lda, ln = A.float(), A, K, None
    ref = A_ref @ W.float().t()
    base = torch.randn(M, N, generator=g)
    if epi == 1:
        ref = torch.relu(ref)
    if epi in (2, 4):            # 2: fp32 atomics over K-split workgroups; 4: one writer per element, K walked in passes (bit-reproducible)
        ref = base + ref
    out_f32 = epi in (2, 3, 4)
    C = base.clone() if epi in (2, 4) else torch.zeros(M, N, dtype=torch.float32 if out_f32 else tt)
    Ad, Wd, Cd = dev(be, A_dev), dev(be, W), dev(be, C)
    lnd = dev(be, ln) if ln is not None else None
    be.check(be.lib.p5_op_skinny_gemm(dtype, amode, P(Ad), lda, P(lnd), P(Wd), K, P(Cd), N, M, N, K, epi, 1.0, 1e-6, be.stream_ptr()), "skinny")
    sync(be)
    err = (Cd.cpu().float() - ref).abs().max().item()
    tol = 2e-4 * max(1.0, K ** 0.5) if (dtype == 0 or out_f32) else 3e-2 * max(1.0, float(ref.abs().max()))
    if dtype == 1 and out_f32:
        tol = 2e-3 * max(1.0, K ** 0.5)
    assert err <= tol, f"skinny dtype={dtype} amode={amode} M={M} N={N} K={K} epi={epi}: err {err} > {tol}"
    return err


def dec_cross_attn_case(be, dtype, variant, B, H, Kb, L, seed=0):
    """decode-step cross-attention kernels (p5_decode2.h) against float64 softmax(q K^T + mask) V on the same rounded inputs."""
    import ctypes
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    g = torch.Generator().manual_seed(seed)
    td = torch.bfloat16 if dtype == 1 else torch.float32
    q = torch.randn(B * Kb, H * 64, generator=g).to(td)
    kv = torch.randn(B * L, 2 * H * 64, generator=g).to(td)
    lens = torch.randint(max(1, L // 2), L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None] < lens[:, None]).long()
    qd, kvd, md = q.to(be.device), kv.to(be.device), mask.to(be.device)
    out = torch.zeros(B * Kb, H * 64, dtype=td, device=be.device)
    be.check(be.lib.p5_op_dec_cross_attn(dtype, variant, P(out), P(qd), P(kvd), P(md), B, H, Kb, L, be.stream_ptr()), "dec_cross_attn")
    sync(be)
    q64 = q.double().view(B, Kb, H, 64)
    kv64 = kv.double().view(B, L, 2, H, 64)
    s = torch.einsum("bqhd,bkhd->bhqk", q64, kv64[:, :, 0]).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), kv64[:, :, 1]).reshape(B * Kb, H * 64)
    err = float((out.cpu().double() - ref).abs().max())
    tol = 2e-5 if dtype == 0 else 2.0 ** -8 * float(ref.abs().max())      # bf16: one rounding of the stored output
    assert err <= tol, f"dec_cross_attn dtype={dtype} variant={variant} B={B} H={H} Kb={Kb} L={L}: err {err} > {tol}"
    return err


def stepwise_decode_case(be, ocfg, B, L, K, max_len, n_items, dtype="fp32", seed=5):
    """p5_decode_begin + p5_decode_step x n + p5_decode_finish == p5_generate (same engine, same inputs); the done flag rises
    exactly when the search stops, and further steps change nothing."""
    import ctypes
    from openp5_amd.trie import CompiledTrie
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    params = O.init_params(ocfg, 7)
    m = build_model(be, ocfg, params, dtype)
    m.eval()
    ids, ww, mask, _, _ = synth_batch(ocfg, B, L, 4, seed)
    items = make_items(n_items, seed, hi=min(60, ocfg.vocab_size - 1))
    ct = CompiledTrie.from_sequences(items)
    ref = m.generate(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=max_len, trie=ct, num_beams=K, num_return_sequences=K,
                     output_scores=True, return_dict_in_generate=True)
    dev_ = be.device
    ml = max(2, min(max_len, ct.max_depth))
    off, tok, nxt = ct.device_arrays(dev_)
    i64 = lambda t: t.to(device=dev_, dtype=torch.int64).contiguous()      # noqa: E731
    ids_d, ww_d, mask_d = i64(ids), i64(ww), i64(mask)
    lib, eng = m._lib, m._engine
    m._sync_shadow()
    nb = lib.p5_generate_workspace_bytes(eng, B, L, K, ml, max(1, ct.max_children), 0)
    ws = m._workspace(nb, "_gen_ws")
    be.check(lib.p5_decode_begin(eng, P(ids_d), P(ww_d), P(mask_d), B, L, K, ml, P(off), P(tok), P(nxt), None, None, 0, max(1, ct.max_children),
                                 P(ws), ws.numel(), be.stream_ptr()), "p5_decode_begin")
    flag_ptr = lib.p5_decode_done_flag(eng)
    assert flag_ptr
    steps_to_done = None
    for i in range(ml + 2):                                   # two more than can ever do work: they must be no-ops
        be.check(lib.p5_decode_step(eng, be.stream_ptr()), "p5_decode_step")
        sync(be)
        done = ctypes.cast(flag_ptr, ctypes.POINTER(ctypes.c_int))[0] if be.is_emulator else _read_device_i32(flag_ptr)
        if done and steps_to_done is None:
            steps_to_done = i + 1
    seq = torch.zeros(B, K, ml, dtype=torch.int32, device=dev_)
    score = torch.zeros(B, K, dtype=torch.float32, device=dev_)
    ln = torch.zeros(B, K, dtype=torch.int32, device=dev_)
    be.check(lib.p5_decode_finish(eng, P(seq), P(score), P(ln), be.stream_ptr()), "p5_decode_finish")
    sync(be)
    assert not lib.p5_decode_done_flag(eng)                    # NULL outside begin..finish
    out_len = 1 + int(ln.max())
    got = seq[:, :, :out_len].reshape(B * K, out_len).to(torch.int64).cpu()
    assert torch.equal(got, ref["sequences"].cpu()), "step-wise sequences differ from p5_generate"
    assert torch.allclose(score.reshape(-1).cpu(), ref["sequences_scores"].cpu(), atol=1e-5 if dtype == "fp32" else 5e-3)
    assert steps_to_done is not None and steps_to_done <= ml - 1
    return steps_to_done


def _read_device_i32(ptr):
    """one int32 behind a raw device pointer (test helper; the stream has been synchronised by the caller)."""
    import ctypes
    host = ctypes.c_int(0)
    hip = ctypes.CDLL("libamdhip64.so")
    rc = hip.hipMemcpy(ctypes.byref(host), ctypes.c_void_p(ptr), ctypes.c_size_t(4), 2)      # hipMemcpyDeviceToHost
    assert rc == 0
    return int(host.value)


def generate_wide_fanout_case(be, ocfg, B, L, K, n_wide, dtype="fp32", seed=3, score_tol=5e-5):
    """A trie level with `n_wide` siblings (> 256: the radix-select path of p5_dec_score2_kernel, incl. the thousand-way score
    ties of the dead -1e9 beams that sit on the same node) followed by short tails: token-exact against the oracle."""
    rnd = random.Random(seed)
    lo = 10
    assert lo + n_wide < ocfg.vocab_size
    items = []
    for t in range(lo, lo + n_wide):
        tail = [rnd.randint(lo, lo + 40) for _ in range(rnd.choice((0, 1, 2)))]
        items.append([0, 5, 6, t] + tail + [1])
    params = O.init_params(ocfg, 7)
    m = build_model(be, ocfg, params, dtype)
    m.eval()
    ids, ww, mask, _, _ = synth_batch(ocfg, B, L, 4, seed)
    trie = Trie(items)
    out = m.generate(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=12, prefix_allowed_tokens_fn=prefix_allowed_tokens_fn(trie),
                     num_beams=K, num_return_sequences=K, output_scores=True, return_dict_in_generate=True)
    with torch.no_grad():
        s_ref, sc_ref = O.beam_search(params, ocfg, ids, ww, mask, lambda b, s: trie.get(s.tolist()), K, 12)
    compare_generation(out["sequences"].cpu(), out["sequences_scores"].cpu(), s_ref, sc_ref, score_tol)
    return out


# ---- the dataset-level gate (tests/test_gpu_dataset.py on the GPU; tests/test_runner_emu.py runs the same body on the host emulation)
FP32_TIE_TOL = 1e-4   # fp32 arithmetic vs the oracle: two items whose oracle scores differ by less than the fp32 score tolerance of the
                      # generation tests (1e-4) may swap places (measured: 2 of 240 users, score gaps <= 1.2e-5).  The HEADLINE generation
                      # mode (bf16 model, generation_mode "verified") and the fp32 engine are both held to this and to nothing looser.
# the plain bf16 search ("draft" mode: a leg of bench.py, and what proposes prefixes to the verification pass) -- round 5, tightened:
BF16_SCORE_TOL = 0.04    # ceiling on |returned score - oracle score of the same sequence|.  Round 5 set 0.016 with 13 % of headroom over the
                         # largest value seen until then (0.0141); round 6's trajectory -- a backward kernel's rounding changed, so the gate trains a
                         # different model -- has ONE of its 2,400 scores at 0.0300: two free tokens of log-probability -1.71 and -1.86 each off by
                         # 0.09 (length-normalised by 6), i.e. logits of magnitude ~12 at 8 mantissa bits.  The ceiling is now set from that
                         # arithmetic (0.1 per free token, two to three free tokens, length 6-7) instead of from the trajectories seen so far.
                         # The HEADLINE mode (verified) and the fp32 engine are held to 1e-4, not to this (measured 2e-6 / 6e-6).
TIE_TOL = 0.01           # oracle-score margin below which the bf16 search may decide differently: 4 x the largest gap observed between an
                         # item it dropped and the weakest it kept (0.0024 per token); was 0.04
BF16_SET_DIFF_MAX = 0.075  # share of users whose top-K SET may differ from the oracle's (measured 10 of 240 in round 4, 12 of 240 with the
                           # atomic-free decode step + forced-prefix pass of round 5: a bound AT the observed 5 % would be a coin flip)


def dropped_gap_first(x, x_lp, ranked, ranked_lp):
    """dropped_gap judged at ONE step only: the first step t at which x[:t] is no prefix of any returned item (the earliest step at which
    the search can have dropped x; it may have carried the prefix further -- then this is a lower bound of its excuse and the test says so
    in what it prints).  Per token; 0.0 = consistent with an exact search."""
    for t in range(1, len(x) + 1):
        if any(tuple(y[:t]) == tuple(x[:t]) for y in ranked):
            continue
        peers = [sum(lp[:t]) for y, lp in zip(ranked, ranked_lp) if len(y) >= t]
        if not peers:
            continue
        return max(0.0, (sum(x_lp[:t]) - min(peers)) / t)
    return float("inf")


def dataset_gate(be, tmp, ocfg_of, K=10, min_users=200, max_fallback_frac=0.05, loss_drop=0.7, bf16_set_diff_max=BF16_SET_DIFF_MAX, drop_rule="first",
                 **pipeline):
    """The dataset-level evaluation gate of tests/test_gpu_dataset.py: a model trained through the real pipeline (bf16 engine), then every
    test user of both tasks ranked FOUR ways with the same weights -- fp32 CPU oracle (HF beam search restated + Python trie callbacks), the
    bf16 model in its default "verified" mode (bf16 search with extra beams proposes, one fp32 pass decides: csrc/p5_verify.h), the fp32
    engine, and the plain bf16 search ("draft").  `be` is the backend (the HIP library on the GPU box; the host emulation runs the same
    body on a tiny model in tests/test_runner_emu.py), `pipeline` the make_pipeline arguments, `ocfg_of(vocab_size)` the oracle's
    configuration of the same model.  north_star: "ranked Hit@k identical" -- asserted for the verified mode and the fp32 engine."""
    runner, model, tok, args = make_pipeline(be, tmp, "bf16", **pipeline)
    losses = runner.train()
    assert min(losses[-2:]) < loss_drop * losses[0], losses        # (the gate needs a model that has learned something, not a converged one)
    model.eval()
    model.generation_mode = "verified"
    r_ver = collect_rankings(runner, engine_gen_fn(model), K)
    vstats = dict(model.verify_stats)
    model.generation_mode = "draft"
    r_bf16 = collect_rankings(runner, engine_gen_fn(model), K)
    model.generation_mode = "verified"
    sd = {k: v.detach().cpu().float().clone() for k, v in model.state_dict().items()}
    from openp5_amd.model import P5T5Native
    m32 = P5T5Native(model.config, dtype="fp32", backend=be, seed=1)
    m32.load_state_dict(sd, strict=False)
    m32.eval()
    r_fp32 = collect_rankings(runner, engine_gen_fn(m32), K)
    ocfg = ocfg_of(model.config.vocab_size)
    margins = []
    params_o = {k: sd[k] for k in O.param_shapes(ocfg)}
    r_or = collect_rankings(runner, oracle_gen_fn(params_o, ocfg, margins), K)
    m_ver, m_bf16, m_fp32, m_or = rankings_metrics(r_ver), rankings_metrics(r_bf16), rankings_metrics(r_fp32), rankings_metrics(r_or)
    cver = compare_rankings(r_ver, r_or, tie_tol=FP32_TIE_TOL)
    c32 = compare_rankings(r_fp32, r_or, tie_tol=FP32_TIE_TOL)
    c16 = compare_rankings(r_bf16, r_or, tie_tol=TIE_TOL)
    n_users = cver["users"]
    depth = sorted({len(it) for users in r_or for _, ranked, _ in users for it in ranked})
    # token positions at which the items of one user's oracle list differ: the steps at which the search had something to decide
    levels = sorted({p for users in r_or for _, ranked, _ in users for p in range(min(len(it) for it in ranked)) if len({it[p] for it in ranked}) > 1})
    print("[dataset] oracle metrics  ", m_or)
    print("[dataset] verified metrics", m_ver, "verification pass:", vstats)
    print("[dataset] plain bf16 metrics", m_bf16)
    print("[dataset] item lengths (tokens incl. </s>):", depth, "positions at which a user's top-K items differ:", levels)
    print("[dataset] verified vs oracle   ", {k: v for k, v in cver.items()})
    print("[dataset] fp32 engine vs oracle", {k: v for k, v in c32.items()})
    print("[dataset] plain bf16 vs oracle ", {k: v for k, v in c16.items()})
    assert sum(len(u) for u in r_or) >= min_users and any(v > 0 for m in m_or for v in m.values())
    # ---- headline mode and fp32 engine: every user's ranked list identical to the oracle's up to swaps of items the ORACLE scores within
    # 1e-4 of each other, the gold item at the same rank for every user, every Hit@k / NDCG@k EQUAL, scores within 1e-4; and every returned
    # hypothesis, re-scored by the oracle on the same token sequence (teacher-forced, O.sequence_scores), within 1e-4 and in order
    _ORACLE_TOKEN_LP.clear()
    for name, c, r, m in (("verified", cver, r_ver, m_ver), ("fp32 engine", c32, r_fp32, m_fp32)):
        assert c["identical_up_to_ties"] == c["users"] and c["max_score_diff"] <= 1e-4, (name, c)
        assert c["identical_lists"] >= 0.98 * c["users"], (name, c)
        assert c["same_gold_rank"] == c["users"] and m == m_or, (name, m, m_or)
        if name != "verified" and c["identical_lists"] == c["users"]:
            continue       # (identical lists with scores within 1e-4: the teacher-forced re-scoring would repeat the oracle's own numbers -- a minute of CPU)
        tf = teacher_forced_check(runner, params_o, ocfg, r, K, 1e-4, FP32_TIE_TOL, r_or)
        print(f"[dataset] teacher-forced, {name}:", {k: v for k, v in tf.items() if not isinstance(v, list)}, "max dropped", max(tf["dropped"]))
        assert tf["users"] == c["users"] and tf["score_viol"] == 0 and tf["order_viol"] == 0 and max(tf["dropped"]) <= FP32_TIE_TOL, (name, tf["max_score_err"])
    # (the verification pass may hand a user to the fp32 search when the draft dropped a prefix the fp32 search needs: correct either way,
    #  but it is the slow path -- it must stay the exception)
    assert vstats["fallback_users"] + vstats["escalated_users"] <= max_fallback_frac * max(1, vstats["users"]), vstats
    # ---- the plain bf16 search: (a) every returned score within BF16_SCORE_TOL of the oracle's score of that sequence, (b) the returned
    # order is the oracle's order of those sequences up to TIE_TOL, (c) the top-K set differs from the oracle's for at most 5 % of the
    # users, and (d) every item the oracle lists and the bf16 search does not was one it was entitled to drop AT THE FIRST STEP its prefix
    # is no prefix of a returned item: its running score there within TIE_TOL per token of -- or below -- the weakest kept prefix
    tf16 = teacher_forced_check(runner, params_o, ocfg, r_bf16, K, BF16_SCORE_TOL, TIE_TOL, r_or)
    flat16, flat_or = [u for us in r_bf16 for u in us], [u for us in r_or for u in us]
    dump = os.environ.get("P5_DATASET_DUMP")
    if dump:
        torch.save({"r_bf16": r_bf16, "r_ver": r_ver, "r_fp32": r_fp32, "r_or": r_or, "margins": margins, "tf16": tf16, "c16": c16, "c32": c32, "cver": cver,
                    "m": (m_bf16, m_fp32, m_or, m_ver), "losses": losses, "verify_stats": vstats}, dump)
    unexplained, set_diff, first_gaps = [], 0, []
    for i, ((_, ra, _), (_, ro, so)) in enumerate(zip(flat16, flat_or)):
        set_diff += int(set(ra) != set(ro))
        if list(ra) == list(ro) or lists_equal_up_to_ties(list(ra), list(ro), list(so), TIE_TOL):
            continue
        r_lp, o_lp = tf16["detail"][i]
        gaps = [dropped_gap_first(ro[j], o_lp[j], list(ra), r_lp) for j in range(len(ro)) if ro[j] not in ra]
        g = max(gaps + [0.0])
        first_gaps.append(g)
        # drop_rule "first": the item must have been droppable at the FIRST step its prefix is no prefix of a returned item -- exact when the
        # search decides once (dataset 1).  With several pruning steps the search may have carried the prefix further and dropped it later
        # (its siblings lost, not the prefix): "any" = droppable at SOME step from the first on (dropped_gap), the first-step figure is printed
        if (g if drop_rule == "first" else tf16["dropped"][i]) > TIE_TOL:
            unexplained.append((i, round(g, 4), round(tf16["dropped"][i], 4)))
    print(f"[dataset] plain bf16: teacher-forced", {k: v for k, v in tf16.items() if not isinstance(v, list)})
    print(f"[dataset] plain bf16: top-{K} set differs for {set_diff} of {n_users} users; largest first-step dropped gap {max(first_gaps + [0.0]):.4f} per token "
          f"(any-step {max(tf16['dropped']):.4f}); not explained at TIE_TOL {TIE_TOL}: {unexplained[:8]}; {c16['identical_lists']} bit-identical lists, "
          f"{c16['identical_up_to_ties']} identical up to oracle ties, same gold rank {c16['same_gold_rank']}")
    assert tf16["score_viol"] == 0 and tf16["order_viol"] == 0, {k: v for k, v in tf16.items() if not isinstance(v, list)}
    assert c16["max_score_diff"] <= BF16_SCORE_TOL, c16
    assert set_diff <= bf16_set_diff_max * n_users, (set_diff, n_users)
    assert len(unexplained) == 0, unexplained
    assert c16["same_gold_rank"] >= 0.95 * n_users and c16["same_topk_set"][5] >= 0.95 * n_users, c16
    return {"verify_stats": vstats, "cver": cver, "c16": c16, "set_diff": set_diff, "depth": depth, "levels": levels}


# ---------------------------------------------------------------------------------------------------------
# Row kernels (csrc/p5_elem.h) and the embedding gradient (csrc/p5_embed.h) against float64: the rows of tests/elem_matrix.py.
# Every case builds its inputs in the kernel's storage types, computes the operation in float64 from those stored values and holds each
# output element to  r |ref| + s S  (S: the same expression over absolute values; r, s: see the head of tests/elem_matrix.py), plus what is
# exact: dropped elements, ignored labels, padding columns, sentinels past the logical extent, untouched table rows, the bf16 shadow.
def _elem_seed():
    return (GEMM_STATE[0] + GEMM_STATE[1] * 0x632BE5AB) & 0xFFFFFFFF


def _elem_r(dtype):
    from tests.elem_matrix import ELEM_R32
    return GEMM_R[True] if dtype == 1 else ELEM_R32


def _guarded(t, extra_rows=1):
    """`t` ([n] or [rows, cols], bf16 / fp32) followed by `extra_rows` rows (or elements) of NaN sentinel"""
    shape = (t.shape[0] + extra_rows,) + tuple(t.shape[1:])
    out = _sentinel(shape, t.dtype)
    out[:t.shape[0]] = t
    return out


def _guard_intact(tag, full, n):
    it, v = GEMM_SENT[full.dtype]
    assert bool((full[n:].contiguous().view(it) == v).all()), f"{tag}: written past its logical extent"


def _elem_check(tag, got, ref, bound, zero=None):
    """every element of `got` within `bound` of the float64 `ref` (finite everywhere: nothing is left out); `zero`: exact zeros.
    Returns the worst err / bound."""
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{tag}: the float64 reference is not finite everywhere"
    got = got.double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{tag}: worst at flat index {i}: got {float(got.flatten()[i]):.9e} ref {float(ref.flatten()[i]):.9e} bound "
                             f"{float(bound.flatten()[i]):.3e} ({int((ratio > 1).sum())} of {ratio.numel()} elements out of bound, worst {worst:.3g} x)")
    if zero is not None:
        assert bool((got[zero] == 0).all()), f"{tag}: {int((got[zero] != 0).sum())} elements that must be exact zeros are not"
    return worst


def _keep(site, numel, p, shape):
    if p <= 0:
        return None
    return O.dropout_keep_mask(_elem_seed(), site, numel, p).view(shape)


def _dropped(x, keep, p):
    return x if keep is None else torch.where(keep, x / (1.0 - p), torch.zeros_like(x))


ELEM_OPT_DEFAULTS = dict(norm_bwd_blocks=1024)


def rmsnorm_ref_case(be, row, seed=0):
    """T5LayerNorm forward and backward (p5_rmsnorm_fwd_kernel, p5_rmsnorm_bwd_kernel<T, NCH>, p5_reduce_rows_kernel), one row of
    elem_matrix.RMSNORM.  The backward is given rstd (or the d / 64 partial sums of squares) as stored values and runs with dw by atomics and
    by per-workgroup partials; dw is pre-filled (+=).  Options set by the row are restored."""
    for k, v in row["opts"].items():
        be.check(be.lib.p5_set_option(k.encode(), v), f"p5_set_option {k}")
    try:
        return _rmsnorm_ref_run(be, row, seed)
    finally:
        for k in row["opts"]:
            be.lib.p5_set_option(k.encode(), ELEM_OPT_DEFAULTS[k])


def _rmsnorm_ref_run(be, row, seed):
    from tests.elem_matrix import ELEM_R32
    lib, st = be.lib, be.stream_ptr()
    dtype, rows, d, eps = row["dtype"], row["rows"], row["d"], 1e-6
    tt, r, tag = TT[dtype], _elem_r(dtype), row["id"]
    g = torch.Generator().manual_seed(seed + 17)
    x = torch.randn(rows, d, generator=g)
    if row["edge"]:
        x[0] = 0
        x[1] *= 1e4
        x[2] *= 1e-4
        x[3] = 0
        x[3, d // 2] = 1.5
    x = x.to(tt)
    w = (1.0 + 0.1 * torch.randn(d, generator=g)).float()
    dy = torch.randn(rows, d, generator=g).to(tt)
    dres = torch.randn(rows, d, generator=g).float() if row["dres"] else None
    dw0 = torch.randn(d, generator=g).float()
    rng = dev(be, torch.tensor(GEMM_STATE, dtype=torch.int32))
    S_Y, S_IN, S_NX = 21, 22, 23
    xd, wd, dyd = dev(be, x), dev(be, w), dev(be, dy)
    dresd = dev(be, dres) if dres is not None else None
    yd = dev(be, _sentinel((rows + 1, d), tt))
    rd = dev(be, _sentinel((rows + 1,), torch.float32))
    plain = not (row["drop_y"] or row["drop_in"] or row["drop_next"] or row["ssq"])

    def fwd():
        if plain:
            return lib.p5_op_rmsnorm_fwd(dtype, P(yd), P(rd), P(xd), P(wd), rows, d, eps, st)
        return lib.p5_op_rmsnorm_fwd_drop(dtype, P(yd), P(rd), P(xd), P(wd), rows, d, eps, P(rng), S_Y, row["drop_y"], st)

    outs = dict(dres_out=dev(be, _sentinel((rows + 1, d), torch.float32)), dy_next=dev(be, _sentinel((rows + 1, d), tt)),
                n_out=dev(be, _sentinel((rows + 1, d), tt)))
    dwd = dev(be, _guarded(dw0))
    rstd_in = ssq = None

    def bwd(partial):
        scratch = dev(be, torch.full((1024 * d,), float("nan"))) if partial else None      # (a partial row its workgroup did not write would show)
        if plain:
            return lib.p5_op_rmsnorm_bwd(dtype, P(outs["dres_out"]), P(outs["dy_next"]), P(dwd), P(dyd), P(xd), P(wd), P(rstd_in), P(dresd), rows, d,
                                         P(scratch), st)
        return lib.p5_op_rmsnorm_bwd_full(dtype, P(outs["dres_out"]), P(outs["dy_next"]), P(dwd), P(dyd), P(xd), P(wd), P(rstd_in), P(dresd), rows, d,
                                          P(scratch), P(rng), S_IN, row["drop_in"], S_NX, row["drop_next"], P(ssq), P(outs["n_out"]) if row["ssq"] else None,
                                          eps, st)

    if row["error"]:      # the launcher refuses (P5_REQUIRE): an error code, nothing launched, nothing written
        rstd_in = dev(be, torch.ones(rows))
        assert fwd() != 0 and b"rmsnorm" in lib.p5_last_error(), f"{tag}: forward accepted d = {d}"
        plain = False
        assert bwd(False) != 0 and b"rmsnorm" in lib.p5_last_error(), f"{tag}: backward accepted d = {d}"
        sync(be)
        for name, t in (("y", yd), ("rstd", rd), ("dw", dwd)) + tuple(outs.items()):
            _guard_intact(f"{tag} {name}", t.cpu(), d if name == "dw" else 0)
        assert torch.equal(dwd.cpu()[:d], dw0)
        return 0.0

    # ---- forward ----
    x64, w64 = x.double(), w.double()
    rstd64 = 1.0 / torch.sqrt((x64 * x64).mean(1) + eps)
    keep_y = _keep(S_Y, rows * d, row["drop_y"], (rows, d))
    yref = _dropped(w64 * (x64 * rstd64[:, None]), keep_y, row["drop_y"])
    be.check(fwd(), f"rmsnorm_fwd {tag}")
    sync(be)
    yh, rh = yd.cpu(), rd.cpu()
    _guard_intact(f"{tag} y", yh, rows)
    _guard_intact(f"{tag} rstd", rh, rows)
    worst = _elem_check(f"{tag} rstd", rh[:rows], rstd64, (ELEM_R32 + GEMM_S) * rstd64)
    # (x * rstd) is rounded to the activation type before * w, and the result once more: 2 r
    worst = max(worst, _elem_check(f"{tag} y", yh[:rows], yref, (2 * r + GEMM_S) * yref.abs(), zero=None if keep_y is None else ~keep_y))

    # ---- backward ----
    if row["ssq"]:
        part = torch.stack([(x64[:, j:j + 64] ** 2).sum(1) for j in range(0, d, 64)], 1).float()
        ssq = dev(be, part)
        rs = 1.0 / torch.sqrt(part.double().sum(1) / d + eps)
    else:
        rstd_in = dev(be, rstd64.float())
        rs = rstd64.float().double()
    keep_in = _keep(S_IN, rows * d, row["drop_in"], (rows, d))
    keep_nx = _keep(S_NX, rows * d, row["drop_next"], (rows, d))
    dyk = _dropped(dy.double(), keep_in, row["drop_in"])
    xh = x64 * rs[:, None]
    dwref, S_dw = dw0.double() + (dyk * xh).sum(0), dw0.double().abs() + (dyk * xh).abs().sum(0)
    gw = dyk * w64
    dot, S_dot = (gw * xh).mean(1, keepdim=True), (gw * xh).abs().mean(1, keepdim=True)
    rout, S_r = rs[:, None] * (gw - xh * dot), rs[:, None] * (gw.abs() + xh.abs() * S_dot)
    if dres is not None:
        rout, S_r = rout + dres.double(), S_r + dres.double().abs()
    nx, S_nx = _dropped(rout, keep_nx, row["drop_next"]), _dropped(S_r, keep_nx, row["drop_next"])
    nref = w64 * xh
    for partial in (False, True):
        md = f"{tag} ({'partials' if partial else 'atomics'})"
        for t in outs.values():
            t.copy_(_sentinel(tuple(t.shape), t.dtype))
        dwd.copy_(_guarded(dw0))
        be.check(bwd(partial), f"rmsnorm_bwd {md}")
        sync(be)
        o = {k: v.cpu() for k, v in outs.items()}
        for k, v in o.items():
            _guard_intact(f"{md} {k}", v, rows if (k != "n_out" or row["ssq"]) else 0)
        _guard_intact(f"{md} dw", dwd.cpu(), d)
        worst = max(worst, _elem_check(f"{md} dres_out", o["dres_out"][:rows], rout, ELEM_R32 * rout.abs() + GEMM_S * S_r))
        worst = max(worst, _elem_check(f"{md} dy_next", o["dy_next"][:rows], nx, r * nx.abs() + GEMM_S * S_nx, zero=None if keep_nx is None else ~keep_nx))
        worst = max(worst, _elem_check(f"{md} dw", dwd.cpu()[:d], dwref, ELEM_R32 * dwref.abs() + GEMM_S * S_dw))
        if row["ssq"]:
            worst = max(worst, _elem_check(f"{md} n_out", o["n_out"][:rows], nref, (2 * r + GEMM_S) * nref.abs()))
    return worst


CE_KINDS = ("normal", "shifted", "constant", "dominant", "neginf", "neginf-head")


def ce_ref_case(be, row, seed=0):
    """Token cross-entropy on materialised logits (p5_ce_fwd_kernel<float> / <bf16>, p5_ce_bwd_kernel, p5_ce_gscale_kernel), one row of
    elem_matrix.CE: 18 logit rows (six kinds x labels -100 / first finite column / V - 1) with NaN padding columns.  No label logit is -inf,
    so the float64 reference is finite for every row (asserted)."""
    from tests.elem_matrix import ELEM_R32, ELEM_TINY
    lib, st = be.lib, be.stream_ptr()
    V, tag = row["V"], row["id"]
    ldd = (V + 63) // 64 * 64
    ldl = ldd + row["pad"]
    tau = ATTN_TAU[0]
    g = torch.Generator().manual_seed(seed + 29)
    R = 3 * len(CE_KINDS)
    L = torch.full((R, ldl), float("nan"))
    labels = torch.zeros(R, dtype=torch.int64)
    ninf = float("-inf")
    for k, kind in enumerate(CE_KINDS):
        for j in range(3):
            i = 3 * k + j
            v = torch.randn(V, generator=g)
            first = 0
            if kind == "shifted":
                v = v + 1e4
            elif kind == "constant":
                v = torch.full((V,), 2.5)
            elif kind == "dominant":
                v[(7 * i) % V] += 200.0
            elif kind == "neginf" and V >= 3:
                m = torch.rand(V, generator=g) < 0.3
                m[1] = True
                m[0] = m[V - 1] = False
                v[m] = ninf
            elif kind == "neginf-head":
                first = min(1024, V - 1)
                v[:first] = ninf
            L[i, :V] = v
            labels[i] = (-100, first, V - 1)[j]
    x64 = L[:, :V].double()
    mx = x64.max(1).values
    lsum = torch.log(torch.exp(x64 - mx[:, None]).sum(1))
    lse = mx + lsum
    ign = labels == -100
    xl = x64.gather(1, labels.clamp(min=0)[:, None])[:, 0]
    nll = torch.where(ign, torch.zeros_like(lse), lse - xl)
    S_lse = mx.abs() + lsum.abs()
    S_nll = torch.where(ign, torch.zeros_like(lse), S_lse + xl.abs())
    Ld, labd = dev(be, L), dev(be, labels)
    worst = 0.0
    for dtype in (0, 1):
        nd, ld_ = dev(be, _sentinel((R + 1,), torch.float32)), dev(be, _sentinel((R + 1,), torch.float32))
        if dtype == 0:
            be.check(lib.p5_op_ce_fwd(P(nd), P(ld_), P(Ld), P(labd), R, V, ldl, st), f"ce_fwd {tag}")
        else:
            be.check(lib.p5_op_ce_fwd_t(dtype, P(nd), P(ld_), P(Ld), P(labd), R, V, ldl, st), f"ce_fwd_t {tag}")
        sync(be)
        nh, lh = nd.cpu(), ld_.cpu()
        md = f"{tag} fwd {'bf16 mode' if dtype else 'fp32'}"
        _guard_intact(f"{md} nll", nh, R)
        _guard_intact(f"{md} lse", lh, R)
        worst = max(worst, _elem_check(f"{md} lse", lh[:R], lse, ELEM_R32 * lse.abs() + tau * S_lse))
        worst = max(worst, _elem_check(f"{md} nll", nh[:R], nll, ELEM_R32 * nll.abs() + tau * S_nll, zero=ign))

    # ---- backward: lse as stored; g from dnll, or from the mask (rows = B x T) ----
    lse_in = lse.float()
    T = 3
    B = R // T
    attn = torch.tensor([0, 1, 1, 2, -1], dtype=torch.int64)[torch.randint(0, 5, (B, T), generator=g)]
    attn[2] = 0
    attn[0, 0] = 1
    gscale = float(torch.tensor(1.0 / B, dtype=torch.float32))
    dnll = torch.randn(R, generator=g).float()
    cnt = (attn != 0).sum(1).double().clamp(min=1.0)
    g_mask = torch.where(attn != 0, gscale / cnt[:, None].expand(B, T), torch.zeros(B, T, dtype=torch.float64)).reshape(R)
    p = torch.exp(x64 - lse_in.double()[:, None])
    onehot = torch.zeros_like(p)
    onehot[~ign, labels[~ign]] = 1.0
    lsed, attnd, dnlld = dev(be, lse_in), dev(be, attn), dev(be, dnll)
    for dtype in (0, 1):
        tt, r = TT[dtype], _elem_r(dtype)
        for seeding in ("dnll", "mask"):
            gref = torch.where(ign, torch.zeros(R, dtype=torch.float64), dnll.double() if seeding == "dnll" else g_mask)
            ref = (p - onehot) * gref[:, None]
            bound = r * ref.abs() + (tau * (p + onehot) + ELEM_TINY) * gref.abs()[:, None]
            for gy in (1, 4, 8):
                dl = dev(be, _sentinel((R + 1, ldd), tt))
                go = dev(be, _sentinel((R + 1,), torch.float32))
                be.check(lib.p5_op_ce_bwd(dtype, P(dl), P(Ld), P(lsed), P(labd), P(dnlld) if seeding == "dnll" else None, R, V, ldl, ldd, P(attnd), T,
                                          gscale, gy, P(go), st), f"ce_bwd {tag}")
                sync(be)
                dh, gh = dl.cpu(), go.cpu()
                md = f"{tag} bwd {'bf16' if dtype else 'fp32'} g from {seeding} gridDim.y {gy}"
                _guard_intact(f"{md} dlogits", dh, R)
                _guard_intact(f"{md} g", gh, R)
                assert bool((dh[:R, V:].float() == 0).all()), f"{md}: padding columns [V, ldd) are not zero"
                assert bool((dh[:R][ign].float() == 0).all()), f"{md}: rows with label -100 are not all zero"
                # (one fp32 division, up to 2.5 ulp where the compiler does not emit the correctly rounded sequence: 4 ELEM_R32)
                worst = max(worst, _elem_check(f"{md} g", gh[:R], gref, 4 * ELEM_R32 * gref.abs(), zero=ign))
                worst = max(worst, _elem_check(f"{md} dlogits", dh[:R, :V], ref, bound))
    return worst


def masked_mean_ref_case(be, row, seed=0):
    """The runner's loss (p5_masked_mean_kernel): mean over batch items of the masked mean of their tokens' NLL; items with an empty mask,
    mask values other than 0 / 1."""
    from tests.elem_matrix import ELEM_R32
    B, T, tag = row["B"], row["T"], row["id"]
    g = torch.Generator().manual_seed(seed + 31)
    nll = (torch.randn(B, T, generator=g) * 3.0).float()
    attn = torch.tensor([0, 1, 1, 2, -3], dtype=torch.int64)[torch.randint(0, 5, (B, T), generator=g)]
    attn[B // 2] = 0
    if B > 1:
        attn[0] = 1
    m = (attn != 0).double()
    cnt = m.sum(1).clamp(min=1.0)
    ref = ((nll.double() * m).sum(1) / cnt).mean().reshape(1)
    S = ((nll.double().abs() * m).sum(1) / cnt).mean().reshape(1)
    out = dev(be, _sentinel((2,), torch.float32))
    nd, ad = dev(be, nll), dev(be, attn)
    be.check(be.lib.p5_op_masked_mean(P(out), P(nd), P(ad), B, T, be.stream_ptr()), f"masked_mean {tag}")
    sync(be)
    oh = out.cpu()
    _guard_intact(tag, oh, 1)
    return _elem_check(tag, oh[:1], ref, ELEM_R32 * ref.abs() + GEMM_S * S)


def embed_fwd_ref_case(be, row, seed=0):
    """x = dropout(E[ids] (+ WW[ww])) in the activation type (p5_embed_fwd_kernel) and the rows' sums of squares per 64 columns; ids reach row 0
    and the last row of the table; rows past `rows` keep a sentinel."""
    from tests.elem_matrix import ELEM_R32
    dtype, rows, d, tag = row["dtype"], row["rows"], row["d"], row["id"]
    tt, r, p = TT[dtype], _elem_r(dtype), row["drop"]
    g = torch.Generator().manual_seed(seed + 37)
    Vt, Wt, SITE = 50, 20, 31
    E, WW = torch.randn(Vt, d, generator=g).to(tt), torch.randn(Wt, d, generator=g).to(tt)
    ids, ww = torch.randint(0, Vt, (rows,), generator=g), torch.randint(0, Wt, (rows,), generator=g)
    ids[0], ids[-1] = 0, Vt - 1
    ww[0], ww[-1] = Wt - 1, 0
    val = E.double()[ids] + (WW.double()[ww] if row["ww"] else 0.0)
    S = E.double().abs()[ids] + (WW.double().abs()[ww] if row["ww"] else 0.0)
    keep = _keep(SITE, rows * d, p, (rows, d))
    ref, S = _dropped(val, keep, p), _dropped(S, keep, p)
    out = dev(be, _sentinel((rows + 2, d), tt))
    ssq = dev(be, _sentinel((rows + 1, d // 64), torch.float32)) if row["ssq"] else None
    rng = dev(be, torch.tensor(GEMM_STATE, dtype=torch.int32))
    Ed, Wd, idd, wwd = dev(be, E), dev(be, WW), dev(be, ids), dev(be, ww)
    be.check(be.lib.p5_op_embed_fwd(dtype, P(out), P(Ed), P(Wd) if row["ww"] else None, P(idd), P(wwd) if row["ww"] else None, rows, d, P(rng), SITE, p,
                                    P(ssq), be.stream_ptr()), f"embed_fwd {tag}")
    sync(be)
    oh = out.cpu()
    _guard_intact(tag, oh, rows)
    # one rounding to the stored type; before it five fp32 roundings (p, 1 - p, its reciprocal, the add, the multiply)
    worst = _elem_check(tag, oh[:rows], ref, r * ref.abs() + 5 * ELEM_R32 * S, zero=None if keep is None else ~keep)
    if ssq is not None:
        sh = ssq.cpu()
        _guard_intact(f"{tag} ssq", sh, rows)
        want = torch.stack([(oh[:rows, j:j + 64].double() ** 2).sum(1) for j in range(0, d, 64)], 1)
        worst = max(worst, _elem_check(f"{tag} ssq_part", sh[:rows], want, (ELEM_R32 + GEMM_S) * want))
    return worst


def _embed_keys(pattern, n, g):
    """keys [n] int64 and the number of table rows for one pattern of elem_matrix.EMBED"""
    if pattern == "equal":
        return torch.full((n,), 7, dtype=torch.int64), 40
    if pattern == "distinct":
        return torch.randperm(n + 9, generator=g)[:n].clone(), n + 9
    if pattern == "pad70":
        Vt = max(50, n // 8)
        k = torch.randint(0, Vt, (n,), generator=g)
        k[torch.rand(n, generator=g) < 0.7] = 0
        return k, Vt
    assert pattern == "blocks"
    counts, pos = [], 0

    def seg(c):
        nonlocal pos
        counts.append(c)
        pos += c

    def fill_to_last_of_block():
        while pos % 32 != 31:
            seg(1)
    seg(min(32, n))                                   # ends exactly on a block boundary
    for blocks in (4, 5, 9):                          # starts on the last position of a block, ends on the first of the blocks-th
        c = 1 + 32 * (blocks - 2) + 1
        if pos + 31 + c > n:
            break
        fill_to_last_of_block()
        seg(c)
    while pos < n - 3:
        seg(1)
    if pos < n:
        seg(n - pos)                                  # the largest table row closes the array (a segment of up to 3)
    keys = torch.cat([torch.full((c,), i + 2, dtype=torch.int64) for i, c in enumerate(counts)])
    assert keys.numel() == n
    return keys[torch.randperm(n, generator=g)], len(counts) + 2


def embed_ref_case(be, row, seed=0, dump=None):
    """Gradient of the embedding lookups (p5_embed.h: sort chunks, rank, segmented sum, fix-up; p5_embed_bwd_kernel), one row of
    elem_matrix.EMBED.  The fixed-order chain must leave perm / skey / sstart / slen equal to a stable argsort of the concatenated keys, give
    the same bits on a second run (over scratch that still holds the first run's pieces; idx starts as zeros, so that a position a wrong
    rank leaves unwritten still names a row and a key inside the arrays), and stay within the bound of float64, as must the
    atomic scatter; table rows no key refers to keep their bits.  Returns (worst err / bound, sha256 of the chain's table gradients); `dump`
    (a dict) receives the sets' inputs as numpy arrays, for tests/emu/embed_chain_digest.py."""
    import hashlib
    import numpy as np
    from openp5_amd._abi import P5EmbedBwdSet
    from tests.elem_matrix import ELEM_R32
    d, tag = row["d"], row["id"]
    g = torch.Generator().manual_seed(seed + 41)
    rng = dev(be, torch.tensor(GEMM_STATE, dtype=torch.int32))
    sets = []
    for k, (n, n0, pat, p0, p1) in enumerate(row["sets"]):
        keys, Vt = _embed_keys(pat, n, g)
        n1 = n - n0
        dres = torch.randn(n, d, generator=g).float()
        table0 = torch.randn(Vt + 1, d, generator=g).float()
        s0, s1 = 41 + 2 * k, 42 + 2 * k
        vals = dres.double().clone()
        for lo, hi, site, p in ((0, n0, s0, p0), (n0, n, s1, p1)):
            if hi > lo and p > 0:
                keep = _keep(site, (hi - lo) * d, p, (hi - lo, d))
                vals[lo:hi] = _dropped(vals[lo:hi], keep, p)
        ref = table0.double().index_add(0, keys, vals)
        S = table0.double().abs().index_add(0, keys, vals.abs())
        kn = keys.numpy()
        perm = np.argsort(kn, kind="stable").astype(np.int32)
        skey = kn[perm].astype(np.int32)
        uniq, start, count = np.unique(skey, return_index=True, return_counts=True)
        which = np.searchsorted(uniq, skey)
        want_idx = torch.from_numpy(np.concatenate([perm, skey, start[which].astype(np.int32), count[which].astype(np.int32)]))
        q = dict(n=n, n0=n0, n1=n1, Vt=Vt, keys=keys, table0=table0, ref=ref, S=S, want_idx=want_idx, used=torch.zeros(Vt + 1, dtype=torch.bool),
                 key0=dev(be, keys[:n0].contiguous()) if n0 else None, key1=dev(be, keys[n0:].contiguous()) if n1 else None,
                 dres0=dev(be, dres[:n0].contiguous()) if n0 else None, dres1=dev(be, dres[n0:].contiguous()) if n1 else None,
                 s0=s0, s1=s1, p0=p0, p1=p1,
                 idx=dev(be, torch.cat([torch.zeros(4 * n, dtype=torch.int32), torch.full((4,), -7, dtype=torch.int32)])), csort=dev(be, torch.zeros((n + 255) // 256 * 256, dtype=torch.int64)),
                 part=dev(be, torch.full(((n + 31) // 32 * 2 * d,), float("nan"))))
        q["used"][keys] = True
        sets.append(q)
        if dump is not None:
            dump.setdefault(row["id"], []).append(dict(keys=kn, dres=dres.numpy(), table0=table0.numpy(), n0=n0, s0=s0, s1=s1, p0=p0, p1=p1))

    def run(mode):
        arr = (P5EmbedBwdSet * len(sets))()
        tabs = []
        for k, q in enumerate(sets):
            t = dev(be, q["table0"].clone())
            tabs.append(t)
            a = arr[k]
            for f in ("key0", "key1", "dres0", "dres1", "idx", "csort", "part"):
                setattr(a, f, q[f].data_ptr() if q[f] is not None else None)
            a.n0, a.n1, a.site0, a.site1, a.drop_p0, a.drop_p1, a.table = q["n0"], q["n1"], q["s0"], q["s1"], q["p0"], q["p1"], t.data_ptr()
        be.check(be.lib.p5_op_embed_bwd(0, mode, len(sets), d, arr, P(rng), be.stream_ptr()), f"embed_bwd {tag} mode {mode}")
        sync(be)
        return [t.cpu() for t in tabs]

    first, second, atomic = run(1), run(1), run(0)
    worst, h = 0.0, hashlib.sha256()
    for k, q in enumerate(sets):
        st = f"{tag} set {k}"
        idx = q["idx"].cpu()
        assert bool((idx[4 * q["n"]:] == -7).all()), f"{st}: idx written past 4 n"
        for j, name in enumerate(("perm", "skey", "sstart", "slen")):
            a, b = idx[j * q["n"]:(j + 1) * q["n"]], q["want_idx"][j * q["n"]:(j + 1) * q["n"]]
            assert torch.equal(a, b), f"{st}: {name} differs from the stable argsort at {int((a != b).nonzero()[0])} ({int((a != b).sum())} positions)"
        assert _same_bits(first[k], second[k]), f"{st}: the fixed-order chain gave different bits on its second run"
        h.update(first[k].numpy().tobytes())
        bound = ELEM_R32 * q["ref"].abs() + GEMM_S * q["S"]
        for name, got in (("chain", first[k]), ("atomic scatter", atomic[k])):
            assert _same_bits(got[~q["used"]], q["table0"][~q["used"]]), f"{st} {name}: table rows no key refers to were written"
            worst = max(worst, _elem_check(f"{st} {name}", got, q["ref"], bound))
    return worst, h.hexdigest()


ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01, max_norm=1.0)


def adamw_ref_case(be, row, seed=0, tol=2e-6):
    """p5_grad_sumsq + p5_adamw_step (p5_sumsq_kernel, p5_adamw_kernel) over consecutive steps against the same arithmetic in float64
    (transformers-4.26 AdamW.step after torch's clip_grad_norm_, as tests/golden/make_adamw_426.py writes it): p, m, v within `tol` of each
    tensor's largest |ref| (adamw_golden_case's bound), the sum of squares within cases.GEMM_S, the bf16 shadow == bf16(p) bit for bit,
    nothing written past n."""
    from tests.elem_matrix import ELEM_R32
    lib, st, h = be.lib, be.stream_ptr(), ADAMW_HYPER
    n, gs, tag = row["n"], row["grad_scale"], row["id"]
    g = torch.Generator().manual_seed(seed + 43)
    G = 8
    p0 = (torch.randn(n, generator=g) * 0.1).float()
    pd, md, vd = dev(be, _guarded(p0, G)), dev(be, _guarded(torch.zeros(n), G)), dev(be, _guarded(torch.zeros(n), G))
    sh = dev(be, _sentinel((n + G,), torch.bfloat16)) if row["shadow"] else None
    ssd = dev(be, _sentinel((1024 + G,), torch.float32))
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    worst = 0.0
    for t in row["steps"]:
        gr = torch.randn(n, generator=g)
        if row["zero"]:
            gr = torch.zeros(n)
        else:
            gr = (gr * (h["max_norm"] * row["factor"] / (gs * float(gr.double().norm())))).float()
        g64 = gr.double()
        gd = dev(be, gr)
        be.check(lib.p5_grad_sumsq(P(gd), n, P(ssd), st), "p5_grad_sumsq")
        be.check(lib.p5_adamw_step(P(pd), P(gd), P(md), P(vd), P(sh), n, P(ssd) if row["sumsq"] else None, h["max_norm"], gs, h["lr"], h["beta1"],
                                   h["beta2"], h["eps"], h["weight_decay"], t, st), "p5_adamw_step")
        sync(be)
        ssq = (g64 * g64).sum().reshape(1)
        ssh = ssd.cpu()
        _guard_intact(f"{tag} sumsq", ssh, 1024)
        worst = max(worst, _elem_check(f"{tag} step {t} sum of squares", ssh[:1024].double().sum().reshape(1), ssq, (ELEM_R32 + GEMM_S) * ssq))
        coef = gs
        if row["sumsq"]:
            coef = gs * min(1.0, h["max_norm"] / (math.sqrt(float(ssq)) * gs + 1e-6))
        gg = g64 * coef
        m = h["beta1"] * m + (1.0 - h["beta1"]) * gg
        v = h["beta2"] * v + (1.0 - h["beta2"]) * gg * gg
        step_size = h["lr"] * math.sqrt(1.0 - h["beta2"] ** t) / (1.0 - h["beta1"] ** t)
        p = p - step_size * (m / (v.sqrt() + h["eps"]))
        p = p - h["lr"] * h["weight_decay"] * p
        ph = pd.cpu()
        for name, got, ref in (("p", ph, p), ("m", md.cpu(), m), ("v", vd.cpu(), v)):
            _guard_intact(f"{tag} {name}", got, n)
            worst = max(worst, _elem_check(f"{tag} step {t} {name}", got[:n], ref, torch.full_like(ref, tol * float(ref.abs().max()))))
        if sh is not None:
            shh = sh.cpu()
            _guard_intact(f"{tag} shadow", shh, n)
            assert _same_bits(shh[:n], ph[:n].to(torch.bfloat16)), f"{tag} step {t}: the bf16 shadow is not the updated parameter rounded once"
    return worst


def elem_ref_case(be, row, seed=0):
    """dispatch one row of tests/elem_matrix.py to its family's case; returns the worst err / bound"""
    fam = row["fam"]
    if fam == "embed":
        return embed_ref_case(be, row, seed)[0]
    return {"rmsnorm": rmsnorm_ref_case, "ce": ce_ref_case, "masked": masked_mean_ref_case, "embed_fwd": embed_fwd_ref_case,
            "adamw": adamw_ref_case}[fam](be, row, seed)
