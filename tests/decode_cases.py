"""The decode-step kernels (csrc/p5_decode2.h and the row-scoring kernels of csrc/p5_decode.h) against float64: one *_ref_case per family of
tests/decode_matrix.py, shared by the emulator suite and the GPU suite.  Bounds and their constants: the head of tests/decode_matrix.py."""
import ctypes

import torch

from openp5_amd.model import relative_position_bucket_lut
from tests.cases import (ATTN_TAU, GEMM_R, GEMM_S, P, TT, _elem_check, _guard_intact, _guarded, _same_bits, _sentinel, _set_opts, attn_key_mask, dev,
                         prof_kernels, route_matches, sync)
from tests.decode_matrix import ELEM_R32

TAU = ATTN_TAU[0]
NM = {0: "fp32", 1: "bf16"}


def _rT(dtype):
    return GEMM_R[True] if dtype == 1 else ELEM_R32


def _round(x64, tt):
    """float64 values as the type tt stores them, back in float64"""
    return x64.to(tt).double()


def _off(t, elems):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def _flag(be, v):
    return dev(be, torch.tensor([v], dtype=torch.int32))


def _outside_intact(tag, full, M, N):
    """every element of the guarded [rows, ld] buffer outside [0:M, 0:N] still holds the sentinel"""
    probe = full.clone()
    probe[:M, :N] = _sentinel((M, N), full.dtype)
    assert _same_bits(probe, _sentinel(tuple(full.shape), full.dtype)), f"{tag}: written outside its {M} x {N} extent"


def _untouched(tag, t):
    assert _same_bits(t, _sentinel(tuple(t.shape), t.dtype)), f"{tag}: written although the call had to leave it alone"


def _profiled(be, row, call, site, tag):
    """run `call` with the row's options set and a profiler report taken; the report must name launch `site` with `tag`"""
    undo = _set_opts(be, row.get("opts", {}))
    open_ = False
    try:
        be.check(be.lib.p5_profile_begin(), "p5_profile_begin")
        open_ = True
        be.check(call(), row["id"])
        sync(be)
        buf = ctypes.create_string_buffer(1 << 16)
        be.check(be.lib.p5_profile_end(buf, len(buf)), "p5_profile_end")
        open_ = False
    finally:
        if open_:
            be.lib.p5_profile_end(None, 0)
        for k, v in undo:
            be.lib.p5_set_option(k.encode(), v)
    keys = prof_kernels(buf.value.decode())
    assert route_matches(keys, site, tag), f"{row['id']}: expected {site} [{tag}], the profiler saw {keys}"


def _refused(be, row, call, word):
    undo = _set_opts(be, row.get("opts", {}))
    try:
        rc = call()
    finally:
        for k, v in undo:
            be.lib.p5_set_option(k.encode(), v)
    assert rc != 0 and word in be.lib.p5_last_error(), f"{row['id']}: the launcher accepted it (rc {rc}, {be.lib.p5_last_error()})"
    sync(be)


def _edge_rows(x):
    """the edge rows of elem_matrix's T5LayerNorm rows: all zero; magnitude 1e4; magnitude 1e-4; a single non-zero"""
    d = x.shape[1]
    x[0] = 0
    x[1] *= 1e4
    x[2] *= 1e-4
    x[3] = 0
    x[3, d // 2] = 1.5
    return x


def _norm_rows64(x, ln, tt, eps):
    """T(ln * T(x rstd)) in float64 with the kernels' two roundings (sk_norm_rows, p5_rmsnorm_f32in_kernel)"""
    x64 = x.double()
    rstd = 1.0 / torch.sqrt((x64 * x64).mean(1, keepdim=True) + eps)
    return _round(ln.double() * _round(x64 * rstd, tt), tt)


# ---- skinny GEMM --------------------------------------------------------------------------------------------------------------------------
def skinny_ref_case(be, row, seed=0):
    dtype, amode, M, N, K, epi, alpha = row["dtype"], row["amode"], row["M"], row["N"], row["K"], row["epi"], row["alpha"]
    tt, tag, eps = TT[dtype], row["id"], 1e-6
    g = torch.Generator().manual_seed(seed + 31)
    lda, ldw = K + (row["pad"][0] if amode == 0 else 0), K + row["pad"][1]
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(tt)
    Wst = torch.full((N, ldw), float("nan"), dtype=tt)
    Wst[:, :K] = W
    ln = None
    if amode == 1:
        x = torch.randn(M, K, generator=g) * 3.0
        if row["edge"]:
            _edge_rows(x)
        ln = (1.0 + 0.1 * torch.randn(K, generator=g)).float()
        Ast = x
        a64 = _norm_rows64(x, ln, tt, eps) if not row["error"] else x.double()
    else:
        A = torch.randn(M, K, generator=g).to(tt)
        Ast = torch.full((M, lda), float("nan"), dtype=tt)
        Ast[:, :K] = A
        a64 = A.double()
    ct = torch.float32 if epi in (2, 3, 4) else tt
    ldc = (N + 7) // 8 * 8 + row["pad"][2]
    Cst = _sentinel((M + 2, ldc), ct)
    C0 = None
    if epi in (2, 4) and not row["error"]:
        C0 = torch.randn(M, N, generator=g)
        Cst[:M, :N] = C0
    Ad, Wd, Cd = dev(be, Ast), dev(be, Wst), dev(be, Cst)
    lnd = dev(be, ln) if ln is not None else None

    def call():
        return be.lib.p5_op_skinny_gemm(dtype, amode, P(Ad), lda, P(lnd), P(Wd), ldw, P(Cd), ldc, M, N, K, epi, alpha, eps, be.stream_ptr())

    if row["error"]:
        _refused(be, row, call, row["word"].encode())
        _untouched(f"{tag} C", Cd.cpu())
        return 0.0
    nb, am, kb = row["inst"]
    _profiled(be, row, call, f"p5_skinny_gemm_kernel<T, NB, AMODE, {kb}>", f"{NM[dtype]} NB={nb} AMODE={am} LDSKB={kb}")
    got = Cd.cpu()
    _outside_intact(f"{tag} C", got, M, N)
    w64 = W.double()
    acc, S = a64 @ w64.t(), a64.abs() @ w64.abs().t()
    if epi in (0, 3):
        al = float(torch.tensor(alpha, dtype=torch.float32))
        ref, S = acc * al, S * abs(al)
    elif epi == 1:
        ref = acc.clamp(min=0)
    else:
        ref, S = C0.double() + acc, S + C0.double().abs()
    r_out = ELEM_R32 if ct == torch.float32 else _rT(dtype)
    s = GEMM_S + ((2 * _rT(dtype) + GEMM_S) if amode == 1 else 0.0)
    worst = _elem_check(tag, got[:M, :N], ref, r_out * ref.abs() + s * S)
    if amode == 1 and row["edge"]:      # the all-zero row: a = 0 exactly
        want = C0[0] if C0 is not None else torch.zeros(N)
        assert torch.equal(got[0, :N].float(), want), f"{tag}: an all-zero row did not give exactly {'C0' if C0 is not None else '0'}"
    return worst


# ---- rmsnorm_f32in --------------------------------------------------------------------------------------------------------------------------
def rmsnorm_f32in_ref_case(be, row, seed=0):
    dtype, rows, d, eps = row["dtype"], row["rows"], row["d"], 1e-6
    tt, tag = TT[dtype], row["id"]
    g = torch.Generator().manual_seed(seed + 37)
    x = torch.randn(rows, d, generator=g)
    if row["edge"]:
        _edge_rows(x)
    w = (1.0 + 0.1 * torch.randn(d, generator=g)).float()
    xd, wd = dev(be, x), dev(be, w)
    yd = dev(be, _sentinel((rows + 1, d), tt))
    done = _flag(be, 1) if row["done"] else None

    def call():
        return be.lib.p5_op_rmsnorm_f32in(dtype, P(yd), P(xd), P(wd), rows, d, eps, P(done), be.stream_ptr())

    if row["error"]:
        _refused(be, row, call, b"rmsnorm_f32in")
        _untouched(f"{tag} y", yd.cpu())
        return 0.0
    be.check(call(), tag)
    sync(be)
    y = yd.cpu()
    if row["done"]:
        _untouched(f"{tag} y", y)
        return 0.0
    _guard_intact(f"{tag} y", y, rows)
    ref = _norm_rows64(x, w, tt, eps)
    worst = _elem_check(tag, y[:rows], ref, (2 * _rT(dtype) + GEMM_S) * ref.abs())
    if row["edge"]:
        assert bool((y[0] == 0).all()), f"{tag}: an all-zero row did not give exactly 0"
    return worst


# ---- softmax(scores) V with the bound of the attention families ---------------------------------------------------------------------------
def _softmax_pv(s, S_abs, v, valid, bias_abs=None):
    """s [.., n] float64 scores, S_abs the same dot products over absolute values, v [.., n, 64], valid [.., n] bool.  Returns O, S_o = P |V|, e =
    GEMM_S max_j (S_abs_j + |bias_j|) over the valid keys [.., 1], dead [..] (no valid key: O = 0)"""
    s = s.masked_fill(~valid, float("-inf"))
    m = s.amax(-1, keepdim=True)
    dead = torch.isinf(m)
    e_ = torch.where(valid, torch.exp(s - torch.where(dead, torch.zeros_like(m), m)), torch.zeros_like(s))
    l = e_.sum(-1, keepdim=True)
    p = e_ / torch.where(dead, torch.ones_like(l), l)
    mag = S_abs if bias_abs is None else S_abs + bias_abs
    e = GEMM_S * torch.where(valid, mag, torch.zeros_like(mag)).amax(-1, keepdim=True)
    return (p.unsqueeze(-2) @ v).squeeze(-2), (p.unsqueeze(-2) @ v.abs()).squeeze(-2), e, dead.squeeze(-1)


# ---- self-attention over the ancestry-indexed cache ---------------------------------------------------------------------------------------
LUT_HALF = 128


def self_attn_ref_case(be, row, seed=0):
    dtype, R, H, cur, mx = row["dtype"], row["R"], row["H"], row["cur_len"], row["max_len"]
    tt, tag, inner, pos = TT[dtype], row["id"], row["H"] * 64, row["cur_len"] - 1
    g = torch.Generator().manual_seed(seed + 41)
    qkv = torch.randn(R, 3 * inner, generator=g)
    if row["bias"] == "gap":      # this step's own key dominates: q . k = 200
        q = qkv[:, :inner].view(R, H, 64)
        qkv[:, inner:2 * inner] = (q * (200.0 / (q * q).sum(-1, keepdim=True))).reshape(R, inner)
    qkv = qkv.to(tt)
    cache0 = _sentinel((mx + 1, R, 2 * inner), tt)          # positions >= pos hold the sentinel; one guard position past max_len
    cache0[:pos] = torch.randn(pos, R, 2 * inner, generator=g).to(tt)
    anc = {}
    for par in (cur & 1, 1 - (cur & 1)):                    # the table this step reads first, then the other parity's: a different valid map
        if par == (cur & 1):
            if row["anc"] == "identity":
                a = torch.arange(R).repeat(mx, 1)
            elif row["anc"] == "one":
                a = torch.zeros(mx, R, dtype=torch.long)
            else:
                a = torch.stack([torch.randperm(R, generator=g) for _ in range(mx)])
            active = a
        else:
            a = (active + 1 + torch.randint(0, R - 1, (mx, 1), generator=g)) % R
        anc[par] = a.to(torch.int32)
    lut = relative_position_bucket_lut(LUT_HALF, False, 32, 128).to(torch.int32)
    rel = torch.randn(32, H, generator=g)
    if row["bias"] == "big" and pos >= 1:
        rel[int(lut[LUT_HALF - 1])] = 30.0 * torch.sign(torch.randn(H, generator=g))          # the bucket of the previous position
    outd = dev(be, _sentinel((R + 1, inner), tt))
    qkvd, cached, reld, lutd = dev(be, qkv), dev(be, cache0), dev(be, rel), dev(be, lut)
    oddd, evend, stepd = dev(be, anc[1]), dev(be, anc[0]), _flag(be, cur)
    done = _flag(be, 1) if row["done"] else None

    def call():
        return be.lib.p5_op_dec_self_attn(dtype, P(outd), P(qkvd), P(cached), P(oddd), P(evend), P(reld), P(lutd), LUT_HALF, R, H, P(stepd), mx, P(done),
                                          be.stream_ptr())

    if row["done"]:
        be.check(call(), tag)
        sync(be)
        _untouched(f"{tag} out", outd.cpu())
        assert _same_bits(cached.cpu(), cache0), f"{tag}: the cache changed although the done flag was set"
        return 0.0
    np_ = row["inst"]
    _profiled(be, row, call, "p5_dec_self_attn2_kernel<T, 8>" if np_ == 8 else "p5_dec_self_attn2_kernel<T, P5_MAX_LEN / 8>", f"{NM[dtype]} NP={np_}")
    out, cache1 = outd.cpu(), cached.cpu()
    _guard_intact(f"{tag} out", out, R)
    want = cache0.clone()
    want[pos] = qkv[:, inner:]                              # this step's K | V, bit for bit; every other byte unchanged
    assert _same_bits(cache1, want), f"{tag}: the cache does not hold exactly its old contents plus this step's K and V at position {pos}"
    # float64 reference
    src = active[:pos].long()                               # [pos, R]
    hist = cache0[:pos].double()[torch.arange(pos)[:, None], src]      # [pos, R, 2 inner]
    kv = torch.cat([hist, qkv[:, inner:].double()[None]], 0).view(cur, R, 2, H, 64)
    k, v = kv[:, :, 0].permute(1, 2, 0, 3), kv[:, :, 1].permute(1, 2, 0, 3)      # [R, H, cur, 64]
    q = qkv[:, :inner].double().view(R, H, 1, 64)
    bias = rel.double()[lut[torch.arange(cur) - pos + LUT_HALF].long()].t()[None]      # [1, H, cur]
    s = (q * k).sum(-1) + bias
    S_abs = (q.abs() * k.abs()).sum(-1)
    O, S_o, e, _ = _softmax_pv(s, S_abs, v, torch.ones_like(s, dtype=torch.bool), bias.abs().expand_as(s))
    ref, S_o = O.reshape(R, inner), S_o.reshape(R, inner)
    bound = _rT(dtype) * ref.abs() + ((2 * e + TAU + GEMM_S).expand(R, H, 64).reshape(R, inner)) * S_o
    return _elem_check(tag, out[:R], ref, bound)


# ---- cross-attention ------------------------------------------------------------------------------------------------------------------------
FUSED_CODES = 16      # distinct (K, sign of V) pairs among the keys of an (item, head) of a fused row
FUSED_MOVES = (2.0, 8.0)      # bounds by which each piece of the fused q projection must move O: on every row of x, on some row (see cross_attn_ref_case)


def _fused_q64(x, ln, Wq, eps, cols=None):
    """q of the fused kernels in float64: T(Wq T(ln * T(x rstd))), over the first `cols` columns of the projection only if given"""
    xn, w = _norm_rows64(x, ln, TT[1], eps), Wq.double()
    if cols is not None:
        xn, w = xn[:, :cols], w[:, :cols]
    return _round(xn @ w.t(), TT[1])


def _cross_mask(B, L, pattern, g):
    if pattern == "prefix":      # the first 128-key chunk (the first half of a shorter sequence) wholly masked; items after the first also lose a suffix
        km = torch.ones(B, L, dtype=torch.long)
        km[:, :128 if L > 128 else L // 2] = 0
        for b in range(1, B):
            if L > 130:
                km[b, 129 + int(torch.randint(1, L - 129, (1,), generator=g)):] = 0
        return km
    if pattern == "late-one":
        km = torch.zeros(B, L, dtype=torch.long)
        km[:, L - 1] = 1
        return km
    return attn_key_mask(B, L, pattern, g)


def cross_attn_ref_case(be, row, seed=0):
    dtype, variant, fused, B, H, Kb, L, d = row["dtype"], row["variant"], row["fused"], row["B"], row["H"], row["Kb"], row["L"], row["d"]
    tt, tag, inner, R, eps = TT[dtype], row["id"], row["H"] * 64, row["B"] * row["Kb"], 1e-6
    g = torch.Generator().manual_seed(seed + 43)
    mask = _cross_mask(B, L, row["mask"], g)
    kv = torch.randn(B * L, 2 * inner, generator=g)
    q = x = ln = Wq = None
    if fused:
        # the fused rows are about q.  The bound's q term, 2 GEMM_R max_j sum_d |q_d k_jd| max |V|, grows with all 64 products of a score and
        # with the largest |V|, whatever L is, while O shrinks as more keys share the weight.  So that q moves O by many bounds at every L:
        # a key is +-1 in four of its head's 64 dimensions and 0 elsewhere (a score is then as large as its sum of absolute products
        # allows), |V| lies in [0.75, 1], and the keys of an (item, head) are drawn from FUSED_CODES (K, sign of V) pairs, so that the weight
        # gathers on the keys of a few pairs, whose V agree in sign, however many keys there are.  Dense N(0, 1) K and V: the other rows.
        bi, hi = torch.arange(B)[:, None, None], torch.arange(H)[None, None, :]
        code = torch.randint(0, FUSED_CODES, (B, L, H), generator=g)
        dims = torch.rand(B, FUSED_CODES, H, 64, generator=g).argsort(-1)[..., :4]
        Kc = torch.zeros(B, FUSED_CODES, H, 64).scatter_(-1, dims, torch.randint(0, 2, (B, FUSED_CODES, H, 4), generator=g).float() * 2 - 1)
        Vc = torch.randint(0, 2, (B, FUSED_CODES, H, 64), generator=g).float() * 2 - 1
        kv[:, :inner] = Kc[bi, code, hi].reshape(B * L, inner)
        kv[:, inner:] = Vc[bi, code, hi].reshape(B * L, inner) * (0.75 + 0.25 * torch.rand(B * L, inner, generator=g))
        x = torch.randn(R, d, generator=g) * 3.0
        if row["edge"]:
            _edge_rows(x)
        ln = ((0.5 + 1.5 * torch.rand(d, generator=g)) * (torch.randint(0, 2, (d,), generator=g) * 2 - 1)).float()      # |ln| in [0.5, 2], either sign
        # q = Wq (ln * x / rms(x)): elements of standard deviation wq_scale
        ln[d // 2] = -1.75          # (all the row of x with a single non-zero reads of ln)
        Wq = (torch.randn(inner, d, generator=g) * (row["wq_scale"] / float(ln.double().pow(2).sum().sqrt()))).to(TT[1])
        if not row["error"]:
            q64 = _fused_q64(x, ln, Wq, eps)
    else:
        q = torch.randn(R, inner, generator=g).to(tt)
        q64 = q.double()
    if row["gap"]:      # the first valid key of every item dominates for the item's first beam: q . k = 200
        for b in range(B):
            j = int(mask[b].nonzero()[0])
            qb = q64[b * Kb].view(H, 64)
            kv[b * L + j, :inner] = (qb * (200.0 / (qb * qb).sum(-1, keepdim=True))).reshape(inner).float()
    kv = kv.to(tt if not fused else TT[1])
    nl = row["ldkv"]
    ldkv, off = nl * 2 * inner, (nl // 2) * 2 * inner
    kvst = torch.full((B * L, ldkv), float("nan"), dtype=kv.dtype)
    kvst[:, off:off + 2 * inner] = kv
    outd = dev(be, _sentinel((R + 1, inner), kv.dtype))
    kvd, md = dev(be, kvst), dev(be, mask)
    qd, xd, lnd, wqd = (dev(be, t) if t is not None else None for t in (q, x, ln, Wq))
    done = _flag(be, 1) if row["done"] else None

    def call():
        return be.lib.p5_op_dec_cross_attn_ex(dtype, variant, P(outd), P(qd), P(xd), P(lnd), P(wqd), _off(kvd, off), ldkv, P(md), B, H, Kb, L, d, eps,
                                              P(done), be.stream_ptr())

    if row["error"]:
        _refused(be, row, call, b"dec_cross_attn")
        _untouched(f"{tag} out", outd.cpu())
        return 0.0
    if row["done"]:
        be.check(call(), tag)
        sync(be)
        _untouched(f"{tag} out", outd.cpu())
        return 0.0
    if fused:
        site = "p5_dec_cross_attn3_kernel<T, true, 136>" if variant == 3 else "p5_dec_cross_attn2_kernel<T, true, 128>"
    elif variant == 3:
        site = "p5_dec_cross_attn3_kernel<T, false, sizeof(T) == 2 ? 52 : 96>"
    else:
        site = "p5_dec_cross_attn2_kernel<T, false, sizeof(T) == 2 ? 48 : 80>"
    _profiled(be, row, call, site, row["inst"])
    out = outd.cpu()
    _guard_intact(f"{tag} out", out, R)
    kv64 = kv.double().view(B, L, 2, H, 64)
    k, v = kv64[:, :, 0].permute(0, 2, 1, 3), kv64[:, :, 1].permute(0, 2, 1, 3)[:, None]               # k [B, H, L, 64], v [B, 1, H, L, 64]
    valid = (mask != 0)[:, None, None, :].expand(B, Kb, H, L)

    def attend(q64):
        qq = q64.view(B, Kb, H, 64)
        s, S_abs = torch.einsum("bqhd,bhld->bqhl", qq, k), torch.einsum("bqhd,bhld->bqhl", qq.abs(), k.abs())      # [B, Kb, H, L]
        O, S_o, e, dead = _softmax_pv(s, S_abs, v, valid)
        return O.reshape(R, inner), S_o.reshape(R, inner), e, dead, S_abs

    ref, S_o, e, dead, S_abs = attend(q64)
    r = _rT(1 if fused else dtype)
    coef = 2 * e + TAU + GEMM_S * (2 if (variant == 3 and kv.dtype == torch.bfloat16) else 1)
    bound = r * ref.abs() + coef.expand(B, Kb, H, 64).reshape(R, inner) * S_o
    if fused:      # q's rounding may fall the other way: a score moves by at most GEMM_R sum |q k|, O by at most 2 max_j of that x max |V|
        e_q = GEMM_R[True] * torch.where(valid, S_abs, torch.zeros_like(S_abs)).amax(-1, keepdim=True)
        vmax = (v.abs() * (mask != 0).double()[:, None, None, :, None]).amax(-1).amax(-1, keepdim=True)          # [B, 1, H, 1]: the largest |V| among an item's valid keys
        bound = bound + (2 * e_q * vmax).expand(B, Kb, H, 64).reshape(R, inner)
        live = ~dead.reshape(B, Kb, H)[:, :, :, None].expand(B, Kb, H, 64).reshape(R, inner)
        if bool(live.any()):
            print(f"{tag}: largest bound {float(bound[live].max()):.3g}, largest |ref| {float(ref.abs().max()):.3g}")
            assert float(bound[live].max()) < 0.1 * float(ref.abs().max()), \
                f"{tag}: the inputs leave a bound of {float(bound[live].max()):.3g} against a largest |ref| of {float(ref.abs().max()):.3g}: scale Wq down"
        # Conditions on the inputs, from the reference alone: what only the fused kernels do must show in O.  A kernel that got one piece
        # wrong returns about the `other` O below, and is caught for certain once that lies more than two bounds from ref (its own error
        # is within one).  FUSED_MOVES asks that of every row of x that is not zero and whose item has at least two valid keys (one valid
        # key gives O = its V, whatever q is) -- so the edge rows of x each check q -- and four times that of some row.
        rows = ((mask != 0).sum(1) >= 2).repeat_interleave(Kb) & (x != 0).any(1)
        others = dict(q_zero=torch.zeros_like(q64), ln_one=_fused_q64(x, torch.ones_like(ln), Wq, eps), half_K=_fused_q64(x, ln, Wq, eps, cols=d // 2))
        if H > 1:
            others["next_head_Wq"] = q64.view(R, H, 64).roll(1, 1).reshape(R, inner)
        for name, q_other in others.items():
            moved = ((attend(q_other)[0] - ref).abs() / bound).amax(1)
            print(f"{tag}: {name} moves O by at least {float(moved[rows].min()) if bool(rows.any()) else float('nan'):.3g} bounds on every row of x")
            assert not bool(rows.any()) or (float(moved[rows].min()) > FUSED_MOVES[0] and float(moved[rows].max()) >= FUSED_MOVES[1]), \
                f"{tag}: {name} moves O by only {float(moved[rows].min()):.3g} bounds on x row {int(moved.masked_fill(~rows, float('inf')).argmin())}, " \
                f"{float(moved[rows].max()):.3g} at the most: raise the score contrast"
    zero = dead[..., None].expand(B, Kb, H, 64).reshape(R, inner)
    return _elem_check(tag, out[:R], ref, bound, zero=zero if bool(zero.any()) else None)


# ---- streaming head -------------------------------------------------------------------------------------------------------------------------
def head_lse_ref_case(be, row, seed=0):
    dtype, nv, R, d, V = row["dtype"], row["nv"], row["R"], row["d"], row["V"]
    tt, tag = TT[dtype], row["id"]
    g = torch.Generator().manual_seed(seed + 47)
    nt = (V + nv - 1) // nv
    small = row["error"] or row["done"]
    hn = torch.randn(R, d, generator=g)
    E = torch.randn(V, d, generator=g)
    if row["kind"] == "peaked":      # logits ~ N(0, 25^2): beyond +-80; one column dominates row 0
        hn *= 25.0
        E[V // 2] = 4.0 * torch.sign(hn[0])
    hn, E = hn.to(tt), E.to(tt)
    alpha = float(torch.tensor(d ** -0.5, dtype=torch.float32))
    pm = dev(be, _sentinel((R + 1, nt), torch.float32))
    ps = dev(be, _sentinel((R + 1, nt), torch.float32))
    hd, Ed = dev(be, hn), dev(be, E)
    done = _flag(be, 1) if row["done"] else None

    def call():
        return be.lib.p5_op_head_lse(dtype, nv, P(pm), P(ps), P(hd), P(Ed), R, d, V, alpha, P(done), be.stream_ptr())

    if small:
        if row["error"]:
            _refused(be, row, call, b"head_lse")
        else:
            be.check(call(), tag)
            sync(be)
        _untouched(f"{tag} part_m", pm.cpu())
        _untouched(f"{tag} part_s", ps.cpu())
        return 0.0
    NV, KB = row["inst"]
    _profiled(be, row, call, f"p5_head_lse_kernel<T, {NV}, {KB}>", f"{NM[dtype]} NV={NV} LDSKB={KB}")
    m_got, s_got = pm.cpu(), ps.cpu()
    _guard_intact(f"{tag} part_m", m_got, R)
    _guard_intact(f"{tag} part_s", s_got, R)
    h64, e64 = hn.double(), E.double()
    lg = alpha * (h64 @ e64.t())
    e_l = GEMM_S * alpha * (h64.abs() @ e64.abs().t()) + ELEM_R32 * lg.abs()
    pad = nt * nv - V
    lg_t = torch.cat([lg, torch.full((R, pad), float("-inf"), dtype=torch.float64)], 1).view(R, nt, nv)
    el_t = torch.cat([e_l, torch.zeros(R, pad, dtype=torch.float64)], 1).view(R, nt, nv).amax(-1)
    m_ref = lg_t.amax(-1)
    logsum = torch.log(torch.exp(lg_t - m_ref[..., None]).sum(-1))
    worst = _elem_check(f"{tag} part_m", m_got[:R], m_ref, el_t)
    b_lse = el_t + TAU * (m_ref.abs() + logsum.abs())
    if dtype == 1:
        spread = torch.where(torch.isinf(lg_t), torch.zeros_like(lg_t), (lg_t - m_ref[..., None]).abs().clamp(max=88.0)).amax(-1)
        b_lse = b_lse + ELEM_R32 * spread
    assert bool((s_got[:R] > 0).all()), f"{tag}: a tile's sum of exponentials is not positive"
    return max(worst, _elem_check(f"{tag} lse", m_got[:R].double() + torch.log(s_got[:R].double()), m_ref + logsum, b_lse))


# ---- row scoring ----------------------------------------------------------------------------------------------------------------------------
def score_ref_case(be, row, seed=0):
    dtype, streaming, K2, max_c, Kb, d = row["dtype"], row["streaming"], row["K2"], row["max_c"], row["Kb"], row["d"]
    tt, tag, fans = TT[dtype], row["id"], row["fans"]
    g = torch.Generator().manual_seed(seed + 53)
    R = len(fans)
    # the trie: node i = the node of decode row i (no children for a dead row, which points at -1)
    off = [0]
    for f in fans:
        off.append(off[-1] + max(f, 0))
    total = off[-1]
    child_off = torch.tensor(off, dtype=torch.int32)
    node = torch.tensor([-1 if f < 0 else i for i, f in enumerate(fans)], dtype=torch.int32)
    child_node = (torch.randperm(max(total, 1), generator=g)[:total] + 1).to(torch.int32)      # distinct ids: the bits of the excluded bitmaps
    VE = 3001 if streaming else row["V"]
    if row["ties"] == "dup":
        three = torch.randperm(VE, generator=g)[:3]
        child_tok = torch.cat([three[torch.arange(max(f, 0)) % 3] for f in fans]).to(torch.int32) if total else torch.zeros(0, dtype=torch.int32)
    else:
        child_tok = torch.randint(0, VE, (total,), generator=g).to(torch.int32)
    run = -torch.randn(R, generator=g).abs() * 3.0
    if row["ties"] == "dead":
        run[:] = -1e9
    users = (R + Kb - 1) // Kb
    words = (total + 1 + 31) // 32 + 1
    excluded = None
    if row["excl"]:
        bits = torch.rand(users, words * 32, generator=g) < 0.3          # every user's own pattern over every child
        if row["excl"] == "all":
            for i in range(1, R, 2):
                bits[i // Kb, child_node[off[i]:off[i + 1]].long()] = True
        wgt = (2 ** torch.arange(32, dtype=torch.int64))
        excluded = (bits.view(users, words, 32).long() * wgt).sum(-1)
        excluded = torch.where(excluded >= 2 ** 31, excluded - 2 ** 32, excluded).to(torch.int32)
    # inputs of the kernel and the float64 score of every child
    if streaming:
        ntiles = row["ntiles"]
        part_m = (torch.randn(R, ntiles, generator=g) * 3.0).float()
        part_s = (1.0 + 127.0 * torch.rand(R, ntiles, generator=g)).float()
        if row["neginf_tile"]:
            part_m[:, ntiles // 2], part_s[:, ntiles // 2] = float("-inf"), 0.0
        pm64, ps64 = part_m.double(), part_s.double()
        mx = pm64.amax(-1)
        logsum = torch.log((ps64 * torch.exp(pm64 - mx[:, None])).sum(-1))
        hn = torch.randn(R, d, generator=g)
        E = torch.randn(VE, d, generator=g)
        if row["ties"] == "dup":      # every row the same h, the three tokens' logits apart by 2 alpha sum |h|: far more than the bound
            hn = hn[:1].expand(R, d).contiguous()
            for j in range(3):
                E[three[j]] = 2.0 * (j - 1) * torch.sign(hn[0])
        hn, E = hn.to(tt), E.to(tt)
        alpha = float(torch.tensor(d ** -0.5, dtype=torch.float32))
    else:
        V = row["V"]
        ldl = (V + 63) // 64 * 64 if not row["error"] else V
        logits = torch.full((R, ldl), float("nan"))
        logits[:, :V] = torch.randn(R, V, generator=g) * 3.0
        if row["ties"] == "dup":      # the three tokens' logits apart by 4
            for j in range(3):
                logits[:, three[j]] = 4.0 * (j - 1)
        l64 = logits[:, :V].double()
        mx = l64.amax(-1)
        logsum = torch.log(torch.exp(l64 - mx[:, None]).sum(-1))
    lse = mx + logsum
    ref, bound, finite = [], [], []
    for i, f in enumerate(fans):
        nc = min(max(f, 0), max_c)
        tok = child_tok[off[i]:off[i] + nc].long()
        if streaming:
            lg = alpha * (E[tok].double() @ hn[i].double())
            e_l = GEMM_S * alpha * (E[tok].double().abs() @ hn[i].double().abs()) + ELEM_R32 * lg.abs()
        else:
            lg, e_l = l64[i, tok], torch.zeros(nc, dtype=torch.float64)
        ref.append((lg - lse[i]) + float(run[i]))
        bound.append(e_l + TAU * (mx[i].abs() + logsum[i].abs()) + 3 * ELEM_R32 * (lg.abs() + lse[i].abs() + abs(float(run[i]))))
        fin = torch.ones(nc, dtype=torch.bool)
        if excluded is not None:
            cn = child_node[off[i]:off[i] + nc].long()
            fin = ~bits[i // Kb, cn]
        finite.append(fin)
    top_s = dev(be, _sentinel((R + 1, K2), torch.float32))
    top_c = dev(be, torch.full((R + 1, K2), -7, dtype=torch.int32))
    n_top = dev(be, torch.full((R + 1,), -7, dtype=torch.int32))
    scratch = None if row["error"] and max_c > 2048 else dev(be, _guarded(torch.full((R, max_c), float("nan"))))
    cod, ctd, cnd, nd, rd = dev(be, child_off), dev(be, child_tok if total else torch.zeros(1, dtype=torch.int32)), \
        dev(be, child_node if total else torch.zeros(1, dtype=torch.int32)), dev(be, node), dev(be, run)
    exd = dev(be, excluded) if excluded is not None else None
    done = _flag(be, 1) if row["done"] else None
    if streaming:
        pmd, psd, hd, Ed = dev(be, part_m), dev(be, part_s), dev(be, hn), dev(be, E)

        def call():
            return be.lib.p5_op_dec_score(dtype, 1, P(pmd), P(psd), ntiles, P(hd), P(Ed), d, alpha, None, 0, 0, P(nd), P(rd), P(cod), P(ctd), P(cnd), P(exd),
                                          words, R, Kb, max_c, K2, P(scratch), P(top_s), P(top_c), P(n_top), P(done), be.stream_ptr())
    else:
        ld_ = dev(be, logits)

        def call():
            return be.lib.p5_op_dec_score(0, 0, None, None, 0, None, None, 0, 0.0, P(ld_), ldl, V, P(nd), P(rd), P(cod), P(ctd), P(cnd), P(exd), words, R, Kb,
                                          max_c, K2, P(scratch), P(top_s), P(top_c), P(n_top), P(done), be.stream_ptr())

    def lists_untouched(rows):
        ts, tc, nt_ = top_s.cpu(), top_c.cpu(), n_top.cpu()
        for i in rows:
            _untouched(f"{tag} top_score[{i}]", ts[i])
            assert bool((tc[i] == -7).all()), f"{tag}: top_c[{i}] written"
        return ts, tc, nt_

    if row["error"] or row["done"]:
        if row["error"]:
            _refused(be, row, call, b"dec_score")
        else:
            be.check(call(), tag)
            sync(be)
        _, _, nt_ = lists_untouched(range(R + 1))
        assert bool((nt_ == -7).all()), f"{tag}: n_top written"
        return 0.0
    be.check(call(), tag)
    sync(be)
    ts, tc, nt_ = lists_untouched([R] + [i for i, f in enumerate(fans) if f < 0])
    assert int(nt_[R]) == -7, f"{tag}: n_top written past row R"
    if scratch is not None:
        _guard_intact(f"{tag} cand_scratch", scratch.cpu(), R)
    worst = 0.0
    for i, f in enumerate(fans):
        n = int(nt_[i])
        if f < 0:
            assert n == 0, f"{tag}: dead row {i} has n_top {n}"
            continue
        fin, rf, bd = finite[i], ref[i], bound[i]
        want_n = min(K2, int(fin.sum()))
        assert n == want_n, f"{tag}: row {i} (fan-out {f}) n_top {n}, expected {want_n}"
        _untouched(f"{tag} top_score[{i}] past n_top", ts[i, n:])
        assert bool((tc[i, n:] == -7).all()), f"{tag}: top_c[{i}] written past n_top"
        if n == 0:
            continue
        c, sc = tc[i, :n].long(), ts[i, :n].double()
        assert bool(((c >= 0) & (c < fin.numel())).all()) and len(set(c.tolist())) == n, f"{tag}: row {i} returned children {c.tolist()}"
        assert bool(fin[c].all()), f"{tag}: row {i} returned an excluded child"
        worst = max(worst, _elem_check(f"{tag} row {i} scores", sc, rf[c], bd[c]))
        order = [(-float(a), int(b)) for a, b in zip(sc, c)]
        assert order == sorted(order), f"{tag}: row {i} is not in (score desc, child asc) order"
        left = fin.clone()
        left[c] = False
        if bool(left.any()):
            assert bool((rf[left] <= float(rf[c].min()) + 2 * bd[left]).all()), f"{tag}: row {i} left out a child better than its last one by more than the bound"
        if row["ties"]:
            cand = fin.nonzero().flatten()
            if row["ties"] == "dup":      # three classes of bit-equal scores, apart by far more than the bound (a condition on the inputs)
                vals = sorted({float(rf[j]) for j in cand.tolist()})
                assert all(b - a > 4 * float(bd.max()) for a, b in zip(vals, vals[1:])), f"{tag}: row {i}: the three scores are too close for an exact order"
                exp = sorted(cand.tolist(), key=lambda j: (-float(rf[j]), j))[:n]
            else:                         # every finite child rounds to run_score itself: the order is the child order
                assert float((rf - float(run[i])).abs().max()) < 32.0, f"{tag}: row {i}: scores do not round to one fp32 value"
                exp = cand.tolist()[:n]
            assert c.tolist() == exp, f"{tag}: row {i} (fan-out {f}) tie order: got {c.tolist()[:12]}..., expected {exp[:12]}..."
    return worst


CASES = dict(skinny=skinny_ref_case, rmsnorm=rmsnorm_f32in_ref_case, self_attn=self_attn_ref_case, cross_attn=cross_attn_ref_case, head_lse=head_lse_ref_case,
             score=score_ref_case)


def decode_ref_case(be, row, seed=0):
    """one row of tests/decode_matrix.py; returns the worst err / bound"""
    return CASES[row["fam"]](be, row, seed)
