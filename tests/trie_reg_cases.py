"""Cases of the regularised item loss -- per-row entropy and KL to a frozen reference policy (`P5T5Native.forward(trie=..., item_entropy=,
ref_logits=)`, `loss_and_backward(entropy_coef=, kl_coef=, ref_logits=)`, `item_logits`, csrc/p5_trie_reg.h) -- shared by
tests/test_trie_reg_emu.py (host emulation) and tests/test_gpu_trie_reg.py (MI355X).

References: float64 sums over `trie_loss_cases.allowed_children` for the kernels one by one (`op_case`); for the model the oracle in float64
under autograd, `torch.log_softmax` over the children's columns of the policy's and of a second parameter set's logits (`oracle_item_terms`).

Definitions (a scored row at node n, A = the allowed children whose own logit is finite, z = logit / tau, zr = ref_logit / tau):
  H = -sum_A p log p,   KL = sum_A p (log p - log q),   p = softmax_A(z),  q = softmax_A(zr)
  dH/dz_j = -p_j (log p_j + H),   dKL/dz_j = p_j (log p_j - log q_j - KL)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases
from tests import multi_target_cases as mt
from tests import trie_head_cases as th
from tests import trie_loss_cases as tl
from tests.cases import ATTN_TAU, P, TT, _elem_check, _elem_r, _guard_intact, _same_bits, _sentinel, dev, sync
from tests.trie_loss_cases import BF16_BOUNDS, GRAD_TOL, NLL_TOL, SCORED

ALPHA, BETA = 0.01, 0.1          # entropy / KL coefficients of the model cases
REF_SEED = 11                    # O.init_params seed of the reference policy (the policy's is 7, as everywhere)
OP_TAUS = (0.5, 1.0, 2.0, 0.7)   # 0.7: the only one whose division logit / tau rounds


# ---------------------------------------------------------------------------------------------------------
# 1. the kernels one by one against float64
# ---------------------------------------------------------------------------------------------------------
def _tau32(tau):
    return float(np.float32(tau))


def _div_rounds(tau):
    """1 where fl(logit / tau) rounds (tau is no power of two), else 0: the division is exact and adds nothing to a bound"""
    return 0.0 if math.frexp(_tau32(tau))[0] == 0.5 else 1.0


def _ref_rows(pr, T, seed):
    """reference logits of trie_loss_cases._op_problem's rows: random, finite, from a second generator, in a row of another leading
    dimension (NaN in the padding columns); the "shifted" rows are shifted by another constant than the policy's"""
    g = torch.Generator().manual_seed(seed + 977)
    B, V = pr["B"], pr["V"]
    ldr = pr["ldl"] + 16
    Rf = torch.full((B * 3, ldr), float("nan"))
    for b, s in enumerate(pr["samples"]):
        for t in range(3):
            v = torch.randn(V, generator=g) * 1.5
            if t == 1 and s["kind"] == "shifted":
                v = v - 3e3
            Rf[b * 3 + t, :V] = v
    return Rf.view(B, 3, ldr)[:, :T].reshape(B * T, ldr).contiguous(), ldr


def _row_terms64(z, zr):
    """float64 H, KL, lse_ref of one row from z / zr over the allowed children (finite z only), each with the sum of absolute values of the
    max-shifted terms it adds"""
    keep = torch.isfinite(z)
    zk = z[keep]
    mx = zk.max()
    e = torch.exp(zk - mx)
    s = e.sum()
    ls = torch.log(s)
    p = e / s
    H = ls - (p * (zk - mx)).sum()
    S_H = ls.abs() + (p * (zk - mx).abs()).sum()
    n = float(zk.numel())
    out = dict(H=H, S_H=S_H, zmax=zk.abs().max(), keep=keep, tiny=n * (1 + (zk - mx).abs().max()))
    if zr is not None:
        zq = zr[keep]
        mr = zq.max()
        sr = torch.exp(zq - mr).sum()
        lsr = torch.log(sr)
        out.update(KL=(p * ((zk - mx) - (zq - mr))).sum() + (lsr - ls), S_KL=S_H + lsr.abs() + (p * (zq - mr).abs()).sum(), lser=mr + lsr,
                   S_lser=mr.abs() + lsr.abs(), zrmax=zq.abs().max(), tiny_kl=n * (1 + (zk - mx).abs().max() + (zq - mr).abs().max()))
    return out


def op_case(be, tau, T=3, seed=0, compact=False):
    """p5_op_trie_reg_fwd / p5_op_trie_reg_bwd in both dtypes' exponentials on trie_loss_cases._op_problem (fan-outs 1 .. 300, kinds shifted /
    dominant / neginf, the exclusion, </s>, -100 and stray samples), on the dense row or -- `compact` -- on the child_col row of the
    restricted head.
    Forward: nll, lse == p5_op_trie_ce_fwd[_cols] bit for bit; H, KL, lse_ref against float64 sums over the allowed children with
      |err| <= ELEM_R32 |x| + ATTN_TAU[0] S + D,
    S = the sum of absolute values of the max-shifted terms the reference adds (H: |log s| + sum p |z - m| -- which IS H, every term being
    non-negative; KL: that, plus |log s_ref| + sum p |zr - m_ref|; lse_ref: |m_ref| + |log s_ref|), the first two terms those of
    trie_loss_cases.op_case.  D is the rounding of the fp32 division that forms z (and zr) from the logit, e_z = ELEM_R32 max_A |z|
    per child, carried to first order through the derivatives: sum_j |dH/dz_j| <= sum p |log p| + H = 2 H = 2 S_H, sum_j |dKL/dz_j| <=
    sum p |log p| + sum p |log q| + |KL| <= 2 S_KL, sum_j |dKL/dzr_j| = sum |q - p| <= 2, so D_H = 2 e_z S_H and D_KL = 2 e_z S_KL + 2 e_zr.
    For tau a power of two the division is exact and D = 0 (_div_rounds); tau = 0.7 exercises it.  And the floor of fp32 itself: an
    exponential below the smallest normal number (ELEM_TINY = 2^-126) may come out as 0, an absolute error of at most ELEM_TINY per child in
    exp(z - m), which the sums multiply by at most 1 + max |z - m| (+ max |zr - m_ref| for KL): 2 n ELEM_TINY times that (the "dominant"
    rows, whose float64 entropy is 1e-173).
    Backward: with the forward's outputs as stored (fp32, the rule of trie_loss_cases.op_case for lse) against
      [g (p_j - [j = label]) - g_H p_j (lp_j + H) + g_KL p_j (lp_j - lq_j - KL)] / tau,  lp = z - lse, lq = zr - lse_ref, p = exp(lp)
    in float64, with three independent random per-row seeds and with the mask-derived ones; the elementwise bound is op_case's
    r |ref| + (ATTN_TAU[0] (p + [j = label]) + ELEM_TINY) |g| / tau extended by the new terms: p carries the relative error ATTN_TAU[0], so
    each bracket adds ATTN_TAU[0] p |bracket| times its seed; at most 8 fp32 roundings touch a term on its way to the store (z - lse,
    zr - lse_ref, their difference, - KL or + H, times p, times the seed, the accumulation, / tau): 8 ELEM_R32 times the sum of absolute values
    |g| (p + [label]) + |g_H| p (|lp| + |H|) + |g_KL| p (|lp| + |lq| + |KL|); and the division's e_z, e_zr through d/dz (p (lp + H)) =
    p (lp + H + 1), d/dz (p (lp - lq - KL)) = p (lp - lq - KL + 1), d/dzr = -p.
    Structure: guards intact, padding columns zero, zeros outside A, zero rows for states 1 / 2, EXACT zeros (H, KL, the whole row) where
    one child is allowed, and with g_H = g_KL = 0 (no reference) the row of p5_op_trie_ce_bwd[_cols] bit for bit.  Returns the worst
    err / bound."""
    from tests.elem_matrix import ELEM_R32, ELEM_TINY
    lib, st = be.lib, be.stream_ptr()
    pr = tl._op_problem(seed)
    off, tok, nxt, V, ldl, ldd, B = pr["off"], pr["tok"], pr["nxt"], pr["V"], pr["ldl"], pr["ldd"], pr["B"]
    labels = pr["labels"][:, :T].contiguous()
    logits = pr["logits"].view(B, 3, ldl)[:, :T].reshape(B * T, ldl).contiguous()
    ref, ldr = _ref_rows(pr, T, seed)
    excl = pr["excl"]
    R = B * T
    tau0, t32, div = ATTN_TAU[0], _tau32(tau), _div_rounds(tau)
    node_ref, state_ref = tl.walk(off, tok, nxt, labels.numpy(), excl, 0, 1)
    node_ref, state_ref = node_ref.reshape(R), state_ref.reshape(R)
    scored = torch.from_numpy(state_ref == SCORED)
    # ---- float64 reference over the allowed children ----
    z64 = lambda x: x.double() / t32        # noqa: E731
    H, KL, LR = (torch.zeros(R, dtype=torch.float64) for _ in range(3))
    bH, bKL, bLR = (torch.zeros(R, dtype=torch.float64) for _ in range(3))
    lse = torch.zeros(R, dtype=torch.float64)
    kids, zs, zrs, lab_at, ez, ezr = {}, {}, {}, {}, {}, {}
    for r in range(R):
        if state_ref[r] != SCORED:
            continue
        c = tl.allowed_children(off, tok, nxt, int(node_ref[r]), excl[r // T])
        z, zr = z64(logits[r, c]), z64(ref[r, c])
        q = _row_terms64(z, zr)
        e_z, e_zr = div * ELEM_R32 * q["zmax"], div * ELEM_R32 * q["zrmax"]
        H[r], KL[r], LR[r] = q["H"], q["KL"], q["lser"]
        bH[r] = ELEM_R32 * q["H"].abs() + tau0 * q["S_H"] + 2 * e_z * q["S_H"] + 2 * ELEM_TINY * q["tiny"]
        bKL[r] = ELEM_R32 * q["KL"].abs() + tau0 * q["S_KL"] + 2 * e_z * q["S_KL"] + 2 * e_zr + 2 * ELEM_TINY * q["tiny_kl"]
        bLR[r] = ELEM_R32 * q["lser"].abs() + tau0 * q["S_lser"] + e_zr
        zk = z[q["keep"]]
        lse[r] = zk.max() + torch.log(torch.exp(zk - zk.max()).sum())
        kids[r], zs[r], zrs[r], lab_at[r], ez[r], ezr[r] = c, z, zr, c.index(int(labels.view(-1)[r])), float(e_z), float(e_zr)
    single = torch.tensor([r in kids and int(torch.isfinite(zs[r]).sum()) == 1 for r in range(R)])
    assert int(single.sum()) >= (6 if T == 3 else 0)
    assert T != 3 or float(H.max()) > 3.0, "the case must hold rows of large entropy"
    # ---- device arrays: the dense row, or the compact row of the restricted head ----
    d_off, d_tok, d_nxt = (dev(be, torch.from_numpy(a)) for a in (off, tok, nxt))
    d_excl = dev(be, torch.from_numpy(excl.view(np.int32)))
    words = excl.shape[1]
    labd = dev(be, labels)
    nd_in, st_in = dev(be, torch.from_numpy(node_ref)), dev(be, torch.from_numpy(state_ref))
    if compact:
        U, col = th._columns(tok)
        Lx, Nu, Nup = th._compact(logits, U, V)
        Rx = th._compact(ref, U, V)[0]
        Rx = torch.cat([Rx, torch.full((R, 8), float("nan"))], 1).contiguous()        # (another leading dimension than the logits')
        d_col, out_ld, n_cols = dev(be, torch.from_numpy(col)), Nup, Nu
        cols_of = {int(t): i for i, t in enumerate(U)}
    else:
        Lx, Rx, d_col, out_ld, n_cols = logits, ref, None, ldd, V
        cols_of = None
    ldx, ldrx = Lx.shape[1], Rx.shape[1]
    Ld, Rd = dev(be, Lx), dev(be, Rx)
    cidx = lambda c: c if cols_of is None else [cols_of[t] for t in c]      # noqa: E731

    def ce_fwd(dtype, n_d, l_d):
        if compact:
            be.check(lib.p5_op_trie_ce_fwd_cols(dtype, P(n_d), P(l_d), P(Ld), P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt), P(d_col), P(d_excl),
                                                words, tau, R, T, ldx, st), "trie_ce_fwd_cols")
        else:
            be.check(lib.p5_op_trie_ce_fwd(dtype, P(n_d), P(l_d), P(Ld), P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt), P(d_excl), words, tau, R, T,
                                           ldx, st), "trie_ce_fwd")

    def ce_bwd(dtype, dl, lsed, dn, attnd, gscale):
        if compact:
            be.check(lib.p5_op_trie_ce_bwd_cols(dtype, P(dl), P(Ld), P(lsed), P(labd), P(nd_in), P(st_in), dn, P(d_off), P(d_tok), P(d_nxt), P(d_col), P(d_excl),
                                                words, tau, R, T, ldx, out_ld, P(attnd), gscale, st), "trie_ce_bwd_cols")
        else:
            be.check(lib.p5_op_trie_ce_bwd(dtype, P(dl), P(Ld), P(lsed), P(labd), P(nd_in), P(st_in), dn, P(d_off), P(d_tok), P(d_nxt), P(d_excl), words, tau, R,
                                           T, ldx, out_ld, P(attnd), gscale, st), "trie_ce_bwd")

    worst = 0.0
    # ---- forward ----
    for dtype in (0, 1):
        md = f"trie_reg fwd tau {tau} T {T} {'bf16 mode' if dtype else 'fp32'}{' compact' if compact else ''}"
        n0, l0 = dev(be, _sentinel((R + 1,), torch.float32)), dev(be, _sentinel((R + 1,), torch.float32))
        ce_fwd(dtype, n0, l0)
        for with_ref in (True, False):
            outs = [dev(be, _sentinel((R + 1,), torch.float32)) for _ in range(5)]
            n_d, l_d, h_d, k_d, r_d = outs
            be.check(lib.p5_op_trie_reg_fwd(dtype, P(n_d), P(l_d), P(h_d), P(k_d) if with_ref else None, P(r_d) if with_ref else None, P(Ld),
                                            P(Rd) if with_ref else None, P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt), P(d_col), P(d_excl), words,
                                            tau, R, T, ldx, ldrx, st), "trie_reg_fwd")
            sync(be)
            nh, lh, hh, kh, rh = (t.cpu() for t in outs)
            for nm, t in (("nll", nh), ("lse", lh), ("H", hh), ("KL", kh), ("lse_ref", rh)):
                _guard_intact(f"{md} {nm}", t, R)
            assert _same_bits(nh[:R], n0.cpu()[:R]) and _same_bits(lh[:R], l0.cpu()[:R]), f"{md}: nll / lse differ from p5_op_trie_ce_fwd's bits"
            worst = max(worst, _elem_check(f"{md} H", hh[:R], H, bH, zero=~scored))
            assert bool((hh[:R][single] == 0).all()), f"{md}: a row with one allowed child must have H exactly 0"
            if with_ref:
                worst = max(worst, _elem_check(f"{md} KL", kh[:R], KL, bKL, zero=~scored))
                worst = max(worst, _elem_check(f"{md} lse_ref", rh[:R], LR, bLR, zero=~scored))
                assert bool((kh[:R][single] == 0).all()), f"{md}: a row with one allowed child must have KL exactly 0"
            else:
                assert _same_bits(kh, _sentinel((R + 1,), torch.float32)) and _same_bits(rh, _sentinel((R + 1,), torch.float32)), f"{md}: KL written without a reference"
    # ---- backward: the forward's outputs as stored ----
    g = torch.Generator().manual_seed(seed + 29)
    lse_in, H_in, KL_in, LR_in = lse.float(), H.float(), KL.float(), LR.float()
    attn = torch.tensor([0, 1, 1, 2, -1], dtype=torch.int64)[torch.randint(0, 5, (B, T), generator=g)]
    attn[2] = 0
    attn[0, 0] = 1
    gscale = float(torch.tensor(1.0 / B, dtype=torch.float32))
    dnll, dH, dKL = (torch.randn(R, generator=g).float() for _ in range(3))
    ec, kc = 0.3, 0.7
    cnt = (attn != 0).sum(1).double().clamp(min=1.0)
    g_mask = torch.where(attn != 0, gscale / cnt[:, None].expand(B, T), torch.zeros(B, T, dtype=torch.float64)).reshape(R)
    z0 = lambda: torch.zeros(R, out_ld, dtype=torch.float64)      # noqa: E731
    p, onehot, lp, lq, e_z, e_zr = z0(), z0(), z0(), z0(), z0(), z0()
    inside = torch.zeros(R, out_ld, dtype=torch.bool)
    for r, c in kids.items():
        ci = cidx(c)
        fin = torch.isfinite(zs[r])
        lpr = torch.where(fin, zs[r] - lse_in[r].double(), torch.zeros_like(zs[r]))
        p[r, ci] = torch.where(fin, torch.exp(lpr), torch.zeros_like(lpr))
        lp[r, ci] = lpr
        lq[r, ci] = torch.where(fin, zrs[r] - LR_in[r].double(), torch.zeros_like(lpr))
        onehot[r, ci[lab_at[r]]] = 1.0
        inside[r, ci] = True
        e_z[r, ci], e_zr[r, ci] = ez[r], ezr[r]
    Hc, Kc = H_in.double()[:, None], KL_in.double()[:, None]
    tH, tK = p * (lp + Hc), p * (lp - lq - Kc)
    lsed, hd_, kd_, rd_ = dev(be, lse_in), dev(be, H_in), dev(be, KL_in), dev(be, LR_in)
    attnd, dnlld, dHd, dKLd = dev(be, attn), dev(be, dnll), dev(be, dH), dev(be, dKL)
    zero_r = torch.zeros(R, dtype=torch.float64)
    for dtype in (0, 1):
        tt, r_ = TT[dtype], _elem_r(dtype)
        for seeding in ("rows", "mask"):
            if seeding == "rows":
                gn, gh, gk = (torch.where(scored, x.double(), zero_r) for x in (dnll, dH, dKL))
            else:
                gn, gh, gk = (torch.where(scored, x, zero_r) for x in (g_mask, -ec * g_mask, kc * g_mask))
            gn, gh, gk = gn[:, None], gh[:, None], gk[:, None]
            want = (gn * (p - onehot) - gh * tH + gk * tK) / t32
            sum_abs = gn.abs() * (p + onehot) + gh.abs() * p * (lp.abs() + Hc.abs()) + gk.abs() * p * (lp.abs() + lq.abs() + Kc.abs())
            bound = r_ * want.abs() + (tau0 * (gn.abs() * (p + onehot) + gh.abs() * tH.abs() + gk.abs() * tK.abs()) + ELEM_TINY * gn.abs() + 8 * ELEM_R32 * sum_abs
                                       + e_z * p * (gn.abs() + gh.abs() * ((lp + Hc).abs() + 1) + gk.abs() * ((lp - lq - Kc).abs() + 1))
                                       + e_zr * p * gk.abs()) / t32
            dl = dev(be, _sentinel((R + 1, out_ld), tt))
            rows = seeding == "rows"
            be.check(lib.p5_op_trie_reg_bwd(dtype, P(dl), P(Ld), P(Rd), P(lsed), P(hd_), P(kd_), P(rd_), P(labd), P(nd_in), P(st_in), P(dnlld) if rows else None,
                                            P(dHd) if rows else None, P(dKLd) if rows else None, P(d_off), P(d_tok), P(d_nxt), P(d_col), P(d_excl), words, tau, R, T,
                                            ldx, ldrx, out_ld, P(attnd), gscale, ec, kc, st), "trie_reg_bwd")
            sync(be)
            dh = dl.cpu()
            md = f"trie_reg bwd tau {tau} T {T} {'bf16' if dtype else 'fp32'} seeds from {seeding}{' compact' if compact else ''}"
            _guard_intact(f"{md} dlogits", dh, R)
            got = dh[:R].float()
            assert bool((got[:, n_cols:] == 0).all()), f"{md}: padding columns are not zero"
            assert bool((got[~inside] == 0).all()), f"{md}: non-zero entries outside the allowed children"
            assert bool((got[~scored] == 0).all()), f"{md}: rows of state 1 / 2 are not all zero"
            assert bool((got[single] == 0).all()), f"{md}: a row with one allowed child must be a zero row"
            assert float(got.abs().max()) > 0
            worst = max(worst, _elem_check(f"{md} dlogits", dh[:R], want, bound))
            # g_H = g_KL = 0, no reference: the row of the plain kernel, bit for bit
            d0, d1 = dev(be, _sentinel((R + 1, out_ld), tt)), dev(be, _sentinel((R + 1, out_ld), tt))
            ce_bwd(dtype, d0, lsed, P(dnlld) if rows else None, attnd, gscale)
            be.check(lib.p5_op_trie_reg_bwd(dtype, P(d1), P(Ld), None, P(lsed), P(hd_), None, None, P(labd), P(nd_in), P(st_in), P(dnlld) if rows else None,
                                            None, None, P(d_off), P(d_tok), P(d_nxt), P(d_col), P(d_excl), words, tau, R, T, ldx, 0, out_ld, P(attnd), gscale, 0.0,
                                            0.0, st), "trie_reg_bwd")
            sync(be)
            assert _same_bits(d0.cpu(), d1.cpu()), f"{md}: with g_H = g_KL = 0 the row differs from p5_op_trie_ce_bwd's"
    print(f"[trie_reg op] tau {tau} T {T}{' compact' if compact else ''}: {R} rows, worst err / bound {worst:.3g}")
    return worst


# ---------------------------------------------------------------------------------------------------------
# 2. identities
# ---------------------------------------------------------------------------------------------------------
def self_reference_case(be, tau=0.7, seed=0):
    """the row's own logits (a copy, in another leading dimension) as the reference: lse_ref == lse and KL == 0.0 on every row bit for bit
    (lse and lse_ref come from one routine in one order, every bracket of the KL sum is then an exact zero), and the dlogits of g_KL = 1
    equal those of g_KL = 0 bit for bit, signs of zeros included (a KL term that is an exact zero is not added)"""
    lib, st = be.lib, be.stream_ptr()
    pr = tl._op_problem(seed)
    off, tok, nxt, V, ldl, ldd, B, T = pr["off"], pr["tok"], pr["nxt"], pr["V"], pr["ldl"], pr["ldd"], pr["B"], 3
    R = B * T
    logits = pr["logits"]
    ref = torch.full((R, ldl + 24), float("nan"))
    ref[:, :V] = logits[:, :V]          # (-inf where the policy has -inf: outside A)
    node_ref, state_ref = tl.walk(off, tok, nxt, pr["labels"].numpy(), pr["excl"], 0, 1)
    d_off, d_tok, d_nxt = (dev(be, torch.from_numpy(a)) for a in (off, tok, nxt))
    d_excl, words = dev(be, torch.from_numpy(pr["excl"].view(np.int32))), pr["excl"].shape[1]
    Ld, Rd, labd = dev(be, logits), dev(be, ref), dev(be, pr["labels"])
    nd_in, st_in = dev(be, torch.from_numpy(node_ref.reshape(R))), dev(be, torch.from_numpy(state_ref.reshape(R)))
    g = torch.Generator().manual_seed(seed + 3)
    dn, dh = dev(be, torch.randn(R, generator=g).float()), dev(be, torch.randn(R, generator=g).float())
    ones, zeros = dev(be, torch.ones(R)), dev(be, torch.zeros(R))
    for dtype in (0, 1):
        n_d, l_d, h_d, k_d, r_d = (dev(be, _sentinel((R,), torch.float32)) for _ in range(5))
        be.check(lib.p5_op_trie_reg_fwd(dtype, P(n_d), P(l_d), P(h_d), P(k_d), P(r_d), P(Ld), P(Rd), P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt),
                                        None, P(d_excl), words, tau, R, T, ldl, ref.shape[1], st), "trie_reg_fwd")
        sync(be)
        assert _same_bits(r_d.cpu(), l_d.cpu()), "lse_ref must equal lse bit for bit when the reference is the policy"
        assert bool((k_d.cpu() == 0).all()), ("KL must be exactly 0 when the reference is the policy", float(k_d.cpu().abs().max()))
        assert float(h_d.cpu().max()) > 1.0
        res = []
        for gk in (ones, zeros):
            dl = dev(be, _sentinel((R, ldd), TT[dtype]))
            be.check(lib.p5_op_trie_reg_bwd(dtype, P(dl), P(Ld), P(Rd), P(l_d), P(h_d), P(k_d), P(r_d), P(labd), P(nd_in), P(st_in), P(dn), P(dh), P(gk),
                                            P(d_off), P(d_tok), P(d_nxt), None, P(d_excl), words, tau, R, T, ldl, ref.shape[1], ldd, None, 0.0, 0.0, 0.0, st),
                     "trie_reg_bwd")
            sync(be)
            res.append(dl.cpu())
        assert bool(torch.isfinite(res[0].float()).all()) and float(res[0].float().abs().max()) > 0
        assert _same_bits(res[0], res[1]), "the KL gradient must vanish bit for bit when the reference is the policy"


def uniform_case(be, tau=2.0):
    """equal logits on the n allowed children of a node give H = log n (excluded children lower n), within op_case's bound for H:
    ELEM_R32 |H| + ATTN_TAU[0] S_H with S_H = H = log n (z - m = 0 on every child); KL to any reference that is uniform on the same
    children is 0 within the same bound with S_KL = 2 log n"""
    from tests.elem_matrix import ELEM_R32
    lib, st = be.lib, be.stream_ptr()
    pr = tl._op_problem(0)
    off, tok, nxt, V, ldl, B, T = pr["off"], pr["tok"], pr["nxt"], pr["V"], pr["ldl"], pr["B"], 3
    R = B * T
    node_ref, state_ref = tl.walk(off, tok, nxt, pr["labels"].numpy(), pr["excl"], 0, 1)
    node_ref, state_ref = node_ref.reshape(R), state_ref.reshape(R)
    logits = torch.full((R, ldl), float("nan"))
    logits[:, :V] = torch.linspace(-3.0, 5.0, R)[:, None]       # one value per row
    ref = torch.full((R, ldl), float("nan"))
    ref[:, :V] = -1.25
    want = torch.zeros(R, dtype=torch.float64)
    ns = set()
    for r in range(R):
        if state_ref[r] == SCORED:
            n = len(tl.allowed_children(off, tok, nxt, int(node_ref[r]), pr["excl"][r // T]))
            want[r] = math.log(n)
            ns.add(n)
    some = [b for b, s in enumerate(pr["samples"]) if s["excl"] == "some"][0]
    assert {1, 2, 33, 256, 257, 300} <= ns and want[some * T + 1] == math.log(33 - 11), sorted(ns)       # (33 children, every third from the second excluded)
    d_off, d_tok, d_nxt = (dev(be, torch.from_numpy(a)) for a in (off, tok, nxt))
    d_excl, words = dev(be, torch.from_numpy(pr["excl"].view(np.int32))), pr["excl"].shape[1]
    Ld, Rd, labd = dev(be, logits), dev(be, ref), dev(be, pr["labels"])
    nd_in, st_in = dev(be, torch.from_numpy(node_ref)), dev(be, torch.from_numpy(state_ref))
    for dtype in (0, 1):
        n_d, l_d, h_d, k_d, r_d = (dev(be, _sentinel((R,), torch.float32)) for _ in range(5))
        be.check(lib.p5_op_trie_reg_fwd(dtype, P(n_d), P(l_d), P(h_d), P(k_d), P(r_d), P(Ld), P(Rd), P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt),
                                        None, P(d_excl), words, tau, R, T, ldl, ldl, st), "trie_reg_fwd")
        sync(be)
        w = _elem_check(f"uniform H dtype {dtype}", h_d.cpu(), want, (ELEM_R32 + ATTN_TAU[0]) * want)
        wk = _elem_check(f"uniform KL dtype {dtype}", k_d.cpu(), torch.zeros_like(want), 2 * ATTN_TAU[0] * want)
        print(f"[trie_reg uniform] dtype {dtype}: worst err / bound H {w:.3g} KL {wk:.3g}")


# ---------------------------------------------------------------------------------------------------------
# 3. the model against the float64 oracle under autograd
# ---------------------------------------------------------------------------------------------------------
def oracle_item_terms(Pq, Pref, ocfg, ids, ww, mask, labels, ct, tau=1.0, excl=None, dp=None):
    """trie_loss_cases.oracle_item_nll's recipe, returning flat [B * T] NLL, entropy and KL rows (differentiable in Pq; the reference
    parameter set Pref, or None, never drops and is a constant), the oracle's logits [B * T, V] of both, and the states"""
    def head(Pm, d):
        enc = O.encoder_forward(Pm, ocfg, ids, ww, mask, d)
        return O.lm_logits(Pm, ocfg, O.decoder_forward(Pm, ocfg, O.shift_right(labels, ocfg), enc, mask, d))
    logits = head(Pq, dp)
    with torch.no_grad():
        rlog = None if Pref is None else head(Pref, None)
    B, T = labels.shape
    node, state = tl.walk(ct.child_off, ct.child_tok, ct.child_node, labels.numpy(), excl, ocfg.pad_id, ocfg.eos_id)
    nll, ent, kl = [], [], []
    for b in range(B):
        for t in range(T):
            if state[b, t] != SCORED:
                for x in (nll, ent, kl):
                    x.append(logits.new_zeros(()))
                continue
            c = tl.allowed_children(ct.child_off, ct.child_tok, ct.child_node, int(node[b, t]), None if excl is None else excl[b])
            lsm = torch.log_softmax(logits[b, t, c] / tau, 0)
            nll.append(-lsm[c.index(int(labels[b, t]))])
            ent.append(-(lsm.exp() * lsm).sum())
            kl.append(logits.new_zeros(()) if rlog is None else (lsm.exp() * (lsm - torch.log_softmax(rlog[b, t, c] / tau, 0))).sum())
    V = logits.shape[-1]
    return torch.stack(nll), torch.stack(ent), torch.stack(kl), logits.reshape(B * T, V), None if rlog is None else rlog.reshape(B * T, V), state


def _f64(params):
    return {k: v.double().clone().requires_grad_(True) for k, v in params.items()}


def _total(nll, ent, kl, out_attn, alpha, beta):
    loss = O.runner_loss(nll, out_attn)
    if beta:
        loss = loss + beta * O.runner_loss(kl, out_attn)
    if alpha:
        loss = loss - alpha * O.runner_loss(ent, out_attn)
    return loss


def model_case(be, ocfg, items, B=3, L=14, T=6, dtype="fp32", dropout=0.0, tau=1.0, excluded=False, item_head="dense", entropy=True, kl=True,
               seed=tl.MODEL_SEED):
    """forward(trie=, item_entropy=, ref_logits=) -> runner_loss(nll) + BETA masked_mean(KL) - ALPHA masked_mean(H) -> backward against the
    float64 oracle: per-row nll / H / KL within NLL_TOL and every parameter gradient within GRAD_TOL by trie_loss_cases.model_case's measure
    (fp32 engine), or cases.grad_agreement at BF16_BOUNDS (bf16 engine; nll_max then bounds all three rows).  The reference policy is a
    second O.init_params run through the same oracle functions; on the engine side its logits come from a second model's `item_logits`.
    The bf16 batch seed is trie_loss_cases.MODEL_SEED, chosen there on existing code alone (see model_case's docstring)."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params, params_ref = O.init_params(ocfg, 7), O.init_params(ocfg, REF_SEED)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, pick = tl.item_batch(ocfg, items, B, L, T, seed)
    excluded_items = tl._excluded_for(items, pick, B) if excluded else None
    excl = ct.excluded_bitmap(excluded_items) if excluded else None
    kw = dict(trie=ct, temperature=tau, excluded_items=excluded_items, item_head=item_head)
    ref_logits = None
    if kl:
        mref = cases.build_model(be, ocfg, params_ref, dtype, dropout)
        mref.train()          # (item_logits never drops)
        ref_logits = mref.item_logits(ids, ww, mask, labels, **kw)
    m = cases.build_model(be, ocfg, params, dtype, dropout)
    dp = tl._train_mode(m, dropout)
    out = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, item_entropy=entropy, ref_logits=ref_logits, **kw)
    assert ("item_entropy" in out) == entropy and ("item_kl" in out) == kl and all(v.shape == (B * T,) for v in out.values())
    zero = torch.zeros_like(out["loss"])
    oa = out_attn.to(out["loss"].device)
    _total(out["loss"], out.get("item_entropy", zero), out.get("item_kl", zero), oa, ALPHA if entropy else 0.0, BETA if kl else 0.0).backward()
    sync(be)
    Pq = _f64(params)
    nll_o, ent_o, kl_o, _, _, state = oracle_item_terms(Pq, _f64(params_ref) if kl else None, ocfg, ids, ww, mask, labels, ct, tau, excl, dp)
    _total(nll_o, ent_o, kl_o, out_attn, ALPHA if entropy else 0.0, BETA if kl else 0.0).backward()
    assert np.array_equal(m.last_item_loss_state.cpu().numpy(), state)
    unscored = torch.from_numpy(state.reshape(-1) != SCORED)
    errs = {}
    for name, want in (("loss", nll_o), ("item_entropy", ent_o), ("item_kl", kl_o)):
        if name in out:
            got = out[name].detach().cpu().double()
            assert bool((got[unscored] == 0).all()), f"{name}: rows that are not scored must be exactly 0"
            errs[name] = float((got - want.detach()).abs().max())
    assert not entropy or float(ent_o.detach().max()) > 0.5
    assert not kl or float(kl_o.detach().max()) > 1e-4, float(kl_o.detach().max())
    tag = f"dropout {dropout} tau {tau} excluded {excluded} head {item_head} entropy {entropy} kl {kl}"
    if dtype == "fp32":
        assert max(errs.values()) <= NLL_TOL, errs
        worst = (0.0, "")
        gmax = max(float(v.grad.abs().max()) for v in Pq.values())
        for name, p_ in m.named_parameters():
            g_, go = p_.grad.detach().cpu().double(), Pq[name].grad
            rel = (g_ - go).abs().max().item() / (go.abs().max().item() + 1e-2 * gmax + 1e-12)
            if rel > worst[0]:
                worst = (rel, name)
        print(f"[trie reg fp32] {tag}: row errors {errs}, worst gradient {worst[0]:.2e} ({worst[1]})")
        assert worst[0] <= GRAD_TOL, f"gradient mismatch {worst}"
        return errs, worst
    rows, whole = cases.grad_agreement(m, Pq)
    r = dict(nll_max=max(errs.values()), worst_rel=max(rows), whole_rel=whole[0], whole_cos=whole[1])
    print(f"[trie reg bf16] {tag}: {errs} {r}")
    assert (r["nll_max"] <= BF16_BOUNDS["nll_max"] and r["worst_rel"][0] <= BF16_BOUNDS["worst_rel"] and r["whole_rel"] <= BF16_BOUNDS["whole_rel"]
            and r["whole_cos"] >= BF16_BOUNDS["whole_cos"]), r
    return r


# ---------------------------------------------------------------------------------------------------------
# 4. the fused step against autograd
# ---------------------------------------------------------------------------------------------------------
def _ref_for(be, ocfg, dtype, batch, **kw):
    mref = cases.build_model(be, ocfg, O.init_params(ocfg, REF_SEED), dtype)
    mref.eval()
    ids, ww, mask, labels = batch[:4]
    return mref.item_logits(ids, ww, mask, labels, **kw)


def fused_case(be, ocfg, items, dtype="fp32", dropout=0.0, item_head="dense", B=3, L=14, T=6, tol=1e-6, staged=False):
    """loss_and_backward(trie=, entropy_coef=, kl_coef=, ref_logits=) == forward(trie=, item_entropy=True, ref_logits=) -> the torch
    expression -> backward on the same weights: loss within tol max(1, |loss|), gradients within trie_loss_cases.fused_case's tolerances;
    `last_item_loss_terms` == the three parts.  `staged`: both through the staged backward."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = tl.item_batch(ocfg, items, B, L, T, 9)
    out_attn[0, :] = 0          # a row with an empty label mask exercises clamp(min=1)
    kw = dict(trie=ct, temperature=0.7, item_head=item_head)
    ref_logits = _ref_for(be, ocfg, dtype, (ids, ww, mask, labels), **kw)
    res = []
    for fused in (False, True):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        tl._train_mode(m, dropout, 77)
        m.staged_backward = staged
        if fused:
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, entropy_coef=ALPHA, kl_coef=BETA, ref_logits=ref_logits, **kw)
            parts = m.last_item_loss_terms.detach().cpu()
        else:
            out = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, item_entropy=True, ref_logits=ref_logits, **kw)
            oa = out_attn.to(out["loss"].device)
            parts = torch.stack([O.runner_loss(out[k], oa).detach().cpu() for k in ("loss", "item_entropy", "item_kl")])
            loss = _total(out["loss"], out["item_entropy"], out["item_kl"], oa, ALPHA, BETA)
            loss.backward()
        sync(be)
        res.append((float(loss.detach()), m._grads.detach().cpu().clone(), parts))
    (l0, g0, p0), (l1, g1, p1) = res
    assert abs(l0 - l1) <= tol * max(1.0, abs(l0)), (l0, l1)
    assert p1.shape == (3,) and float((p0 - p1).abs().max()) <= tol * max(1.0, float(p0.abs().max())), (p0, p1)
    assert float(p1[1]) > 0.1 and float(p1[2]) > 1e-5, p1
    assert abs(l1 - float(p1[0] + BETA * p1[2] - ALPHA * p1[1])) <= tol * max(1.0, abs(l1))
    assert float(g0.abs().max()) > 0
    err = (g0 - g1).abs().max().item() / max(1e-12, g0.abs().max().item())
    print(f"[trie reg fused {dtype} head {item_head} dropout {dropout} staged {staged}] loss {l1:.6f} / {l0:.6f} parts {p1.tolist()}, gradients differ by {err:.2e}")
    assert err <= (tol if dtype == "fp32" else 2e-2), f"fused regularised gradient differs: {err}"
    return l1, err


def fused_targets_case(be, ocfg, items, B=3, L=14, T=6, G=3, dtype="fp32", item_head="dense", tau=0.7, tol=1e-6):
    """labels [B, G, T] with target_weights (zero and negative entries; user 1's targets ALL of weight 0) and per-user exclusion: the NLL
    part is weighted, the regulariser parts are not -- user 1 still contributes its entropy and KL -- against forward + torch + backward"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, picks = mt.item_batch(ocfg, items, B, L, T, G)
    excluded_items = mt._per_user_exclusion(items, labels, out_attn, picks, B)
    w = mt._weights(B, G)
    w[1, :] = 0.0
    assert float(w[0, 0]) == 0 and float(w[B - 1, G - 1]) < 0
    kw = dict(trie=ct, temperature=tau, excluded_items=excluded_items, item_head=item_head)
    ref_logits = _ref_for(be, ocfg, dtype, (ids, ww, mask, labels), **kw)
    assert ref_logits.shape[0] == B * G * T
    res = []
    for fused in (False, True):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        if fused:
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, entropy_coef=ALPHA, kl_coef=BETA, ref_logits=ref_logits, **kw)
            parts = m.last_item_loss_terms.detach().cpu()
        else:
            out = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, item_entropy=True, ref_logits=ref_logits, **kw)
            parts_t = [mt.weighted_loss(out["loss"], out_attn, w), mt.weighted_loss(out["item_entropy"], out_attn), mt.weighted_loss(out["item_kl"], out_attn)]
            loss = parts_t[0] + BETA * parts_t[2] - ALPHA * parts_t[1]
            loss.backward()
            parts = torch.stack([x.detach().cpu() for x in parts_t])
            ent_user1 = float(mt.weighted_loss(out["item_entropy"].detach().cpu().view(B, G, T)[1:2].reshape(-1), out_attn[1:2]))
            assert ent_user1 > 0.05, "the user whose targets all have weight 0 must have entropy to contribute"
            only_w = mt.weighted_loss(out["item_entropy"].detach().cpu(), out_attn, w)
            assert abs(float(only_w) - float(parts[1])) > 1e-3, "the case must tell a weighted entropy term from an unweighted one"
        sync(be)
        res.append((float(loss.detach()), m._grads.detach().cpu().clone(), parts))
    (l0, g0, p0), (l1, g1, p1) = res
    assert abs(l0 - l1) <= tol * max(1.0, abs(l0)), (l0, l1)
    assert float((p0 - p1).abs().max()) <= tol * max(1.0, float(p0.abs().max())), (p0, p1)
    err = float((g0 - g1).abs().max()) / max(1e-12, float(g0.abs().max()))
    print(f"[trie reg fused targets {dtype} head {item_head}] loss {l1:.6f} / {l0:.6f} parts {p1.tolist()}, gradients differ by {err:.2e}")
    assert err <= (tol if dtype == "fp32" else 2e-2), f"fused regularised gradient differs: {err}"


def accumulation_case(be, ocfg, items, dtype="fp32", B=3, L=14, T=6):
    """two regularised micro-batches (begin_micro_batch(first=False)) equal the sum of the two run alone: trie_loss_cases.accumulation_case's
    tolerance"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    a = tl.item_batch(ocfg, items, B, L, T, 3)[:5]
    b = tl.item_batch(ocfg, items, B, L, T, 4)[:5]
    kws = [dict(trie=ct, entropy_coef=ALPHA, kl_coef=BETA, ref_logits=_ref_for(be, ocfg, dtype, x, trie=ct)) for x in (a, b)]
    alone = []
    for batch, kw in zip((a, b), kws):
        m = cases.build_model(be, ocfg, params, dtype, 0.0)
        m.eval()
        m.loss_and_backward(*batch, **kw)
        sync(be)
        alone.append(m._grads.detach().cpu().clone())
    m = cases.build_model(be, ocfg, params, dtype, 0.0)
    m.eval()
    m.begin_micro_batch(first=True, sync=False)
    m.loss_and_backward(*a, **kws[0])
    m.begin_micro_batch(first=False, sync=False)
    m.loss_and_backward(*b, **kws[1])
    sync(be)
    got, want = m._grads.detach().cpu(), alone[0] + alone[1]
    scale = float(want.abs().max())
    assert scale > 0 and float((alone[0] - alone[1]).abs().max()) > 0
    err = float((got - want).abs().max())
    assert err <= 1e-5 * scale, (err, scale)


# ---------------------------------------------------------------------------------------------------------
# 6. item_logits
# ---------------------------------------------------------------------------------------------------------
def item_logits_case(be, ocfg, items, B=3, L=14, T=6, dropout=0.1):
    """item_logits == the oracle's logits at NLL_TOL (dense); the "trie" head's == the dense result's columns head_columns() within the two
    GEMM routes' rounding, by trie_head_cases._compare_routes' fp32 rule for route against route: each route is held to NLL_TOL against the
    oracle, so the two may differ by 2 NLL_TOL (absolute, on the logits as on the NLL there); equal bits in train() and eval();
    `.grad`, the dropout step and a following plain forward's bits untouched; labels [B, G, T] accepted"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = tl.item_batch(ocfg, items, B, L, T, tl.MODEL_SEED)
    m = cases.build_model(be, ocfg, params, "fp32", dropout)
    m.train()
    m.set_dropout_seed(5, 0)
    plain = lambda: m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct)["loss"]      # noqa: E731
    O.runner_loss(plain(), out_attn.to(m._be.device)).backward()
    sync(be)
    grads, step = m._grads.detach().cpu().clone(), list(m._rng_cpu)
    assert float(grads.abs().max()) > 0
    lg_train = m.item_logits(ids, ww, mask, labels, ct).cpu()
    m.eval()
    lg_eval = m.item_logits(ids, ww, mask, labels, ct).cpu()
    lg_trie = m.item_logits(ids, ww, mask, labels, ct, item_head="trie").cpu()
    m.train()
    sync(be)
    assert lg_train.shape == (B * T, ocfg.vocab_size) and lg_train.dtype == torch.float32 and not lg_train.requires_grad
    assert torch.equal(lg_train, lg_eval), "item_logits must not apply dropout in train() mode"
    assert torch.equal(m._grads.detach().cpu(), grads) and list(m._rng_cpu) == step, "item_logits changed .grad or the dropout step"
    _, _, _, lo, _, _ = oracle_item_terms(_f64(params), None, ocfg, ids, ww, mask, labels, ct)
    err = float((lg_eval.double() - lo.detach()).abs().max())
    U = torch.from_numpy(np.asarray(ct.head_columns()[0]).astype(np.int64))
    assert lg_trie.shape == (B * T, len(U))
    route = float((lg_trie - lg_eval[:, U]).abs().max())
    print(f"[item_logits] against the oracle {err:.2e} (tol {NLL_TOL:.0e}); trie head against dense columns {route:.2e} (tol {2 * NLL_TOL:.0e})")
    assert err <= NLL_TOL and route <= 2 * NLL_TOL
    # a following step is the step a model that never called item_logits takes
    m2 = cases.build_model(be, ocfg, params, "fp32", dropout)
    m2.train()
    m2.set_dropout_seed(5, 0)
    m2(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct)
    a, b = plain().detach().cpu(), m2(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct)["loss"].detach().cpu()
    assert torch.equal(a, b), "the forward after item_logits differs"
    ids3, ww3, mask3, lab3, _, _ = mt.item_batch(ocfg, items, B, L, T, 2)
    lg3 = m.item_logits(ids3, ww3, mask3, lab3, ct)
    assert lg3.shape == (B * 2 * T, ocfg.vocab_size) and bool(torch.isfinite(lg3).all())


# ---------------------------------------------------------------------------------------------------------
# 7. unchanged behaviour, errors, workspace
# ---------------------------------------------------------------------------------------------------------
def unchanged_case(be, ocfg, items, B=4, L=16, T=8):
    """a call without the new keywords launches the plain item-loss kernels and none of the regularised ones, and returns the same bits before
    and after a regularised call on the same engine (trie_loss_cases.plain_route_restored_case's method); the regularised call launches the
    twins INSTEAD of the plain kernels; coefficients 0 without ref_logits take the plain path"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    batch = tl.item_batch(ocfg, items, B, L, T, 3, stray=False)[:5]
    ref_logits = _ref_for(be, ocfg, "bf16", batch, trie=ct)
    m = cases.build_model(be, ocfg, params, "bf16", 0.0)
    m.eval()

    def step(**kw):
        m.zero_grad()
        loss = m.loss_and_backward(*batch, trie=ct, **kw)
        sync(be)
        return float(loss), m._grads.detach().cpu().clone()
    step()          # (the first step also refreshes the weight copies)
    (l0, g0), k0 = tl._profiled(be, step)
    (l1, g1), k1 = tl._profiled(be, lambda: step(entropy_coef=ALPHA, kl_coef=BETA, ref_logits=ref_logits))
    assert m.last_item_loss_terms is not None
    (l2, g2), k2 = tl._profiled(be, lambda: step(entropy_coef=0.0, kl_coef=0.0))
    assert m.last_item_loss_terms is None, "a step without regularisers must not leave the previous step's terms behind"
    has = lambda keys, name: any(name in k for k in keys)      # noqa: E731
    for keys in (k0, k2):
        assert has(keys, "p5_trie_ce_fwd_kernel") and has(keys, "p5_trie_ce_bwd_kernel") and has(keys, "p5_masked_mean_kernel") and not has(keys, "p5_trie_reg"), keys
    assert sorted(k0) == sorted(k2), (sorted(k0), sorted(k2))
    assert has(k1, "p5_trie_reg_fwd_kernel") and has(k1, "p5_trie_reg_bwd_kernel") and has(k1, "p5_trie_reg_loss_kernel"), k1
    assert not has(k1, "p5_trie_ce_fwd_kernel") and not has(k1, "p5_trie_ce_bwd_kernel") and not has(k1, "p5_masked_mean_kernel"), k1
    assert l0 == l2 and torch.equal(g0, g2), "the plain item-loss step changed after a regularised step"
    assert l1 != l0 and not torch.equal(g1, g0)
    # the autograd seam: "loss" keeps its bits with the keywords
    kw = dict(input_ids=batch[0], whole_word_ids=batch[1], attention_mask=batch[2], labels=batch[3], trie=ct)
    with torch.no_grad():
        a = m(**kw)["loss"].cpu()
        b = m(item_entropy=True, ref_logits=ref_logits, **kw)["loss"].cpu()
        c = m(**kw)["loss"].cpu()
    assert torch.equal(a, b) and torch.equal(a, c)


def errors_case(be, ocfg):
    """every keyword error is a ValueError that names the cause and leaves nothing armed; the C ABI refuses what it must"""
    from openp5_amd.model import _ptr
    items = cases.make_items(20, 5, hi=60)
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    B, T = 2, 6
    ids, ww, mask, labels, out_attn, _ = tl.item_batch(ocfg, items, B, 12, T, 5, stray=False)
    kw = dict(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)
    dv = m._be.device
    V, Nu = ocfg.vocab_size, len(ct.head_columns()[0])
    good = torch.zeros(B * T, V, device=dv)
    bad = [(dict(item_entropy=True), "trie"), (dict(ref_logits=good), "trie"),
           (dict(trie=ct, item_entropy=True, top_k=3), "truncated"), (dict(trie=ct, ref_logits=good, top_p=0.9), "truncated"),
           (dict(trie=ct, ref_logits=torch.zeros(B * T + 1, V, device=dv)), "ref_logits"), (dict(trie=ct, ref_logits=torch.zeros(B * T, V - 1, device=dv)), "ref_logits"),
           (dict(trie=ct, ref_logits=good, item_head="trie"), "ref_logits"), (dict(trie=ct, ref_logits=torch.zeros(B * T, Nu, device=dv)), "ref_logits"),
           (dict(trie=ct, ref_logits=good.double()), "float32"), (dict(trie=ct, ref_logits=good.cpu().numpy()), "float32")]
    if not be.is_emulator:
        bad.append((dict(trie=ct, ref_logits=good.cpu()), "is on"))
    with torch.no_grad():
        before = m(**kw)["loss"].cpu()
    for b, word in bad:
        with pytest.raises(ValueError, match=word):
            m(**b, **kw)
    fbad = [(dict(entropy_coef=0.1), "trie"), (dict(kl_coef=0.1, ref_logits=good), "trie"), (dict(trie=ct, kl_coef=0.1), "kl_coef"),
            (dict(trie=ct, entropy_coef=float("nan")), "finite"), (dict(trie=ct, entropy_coef=0.0, kl_coef=float("inf"), ref_logits=good), "finite"),
            (dict(trie=ct, entropy_coef=0.1, top_k=2), "truncated"), (dict(trie=ct, kl_coef=0.1, ref_logits=good[:, :5]), "ref_logits")]
    for b, word in fbad:
        with pytest.raises(ValueError, match=word):
            m.loss_and_backward(ids, ww, mask, labels, out_attn, **b)
    with pytest.raises(ValueError, match="trie"):
        m.item_logits(ids, ww, mask, labels, None)
    with torch.no_grad():
        after = m(**kw)["loss"].cpu()
    assert torch.equal(before, after), "a refused call left something armed"
    # ---- the C ABI ----
    lib, eng = be.lib, m._engine
    off, tok, nxt = ct.device_arrays(dv)
    rt = torch.zeros(3 * B * T, dtype=torch.float32, device=dv)
    cut = torch.zeros(B * T, dtype=torch.float32, device=dv)
    arm = lambda: be.check(lib.p5_train_set_item_loss(eng, _ptr(off), _ptr(tok), _ptr(nxt), ct.n_nodes, None, 0, 1.0, None), "arm")      # noqa: E731

    def refused(word, *args):
        assert lib.p5_train_set_item_regularizers(eng, *args) != 0, word
        assert word.encode() in lib.p5_last_error(), (word, lib.p5_last_error())
    with torch.no_grad():
        m(**kw)         # (consumes whatever is armed)
    refused("no item loss is armed", _ptr(good), V, _ptr(rt), 0.1, 0.1, None)
    be.check(lib.p5_train_set_item_loss_truncated(eng, _ptr(off), _ptr(tok), _ptr(nxt), ct.n_nodes, None, 0, 1.0, None, 3, 1.0, _ptr(cut)), "arm truncated")
    refused("truncated", _ptr(good), V, _ptr(rt), 0.1, 0.1, None)
    arm()
    refused("ld_ref", _ptr(good), V - 1, _ptr(rt), 0.1, 0.1, None)
    refused("row_terms", _ptr(good), V, None, 0.1, 0.1, None)
    refused("finite", _ptr(good), V, _ptr(rt), float("nan"), 0.1, None)
    refused("finite", _ptr(good), V, _ptr(rt), 0.1, float("inf"), None)
    assert lib.p5_train_set_item_regularizers(eng, None, 0, _ptr(rt), 0.1, 0.0, None) == 0        # entropy only
    arm()               # a new p5_train_set_item_loss disarms the regularisers: the forward below is the plain item loss
    with torch.no_grad():
        x = m(trie=ct, **kw)["loss"].cpu()
    assert lib.p5_backward_set_item_grads(eng, _ptr(rt), None) != 0 and b"without item regularizers" in lib.p5_last_error()
    with torch.no_grad():
        after = m(**kw)["loss"].cpu()
    assert torch.equal(before, after) and bool(torch.isfinite(x).all())
    ptr, rows, ld, cols = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.p5_train_last_item_logits(eng, ctypes.byref(ptr), ctypes.byref(rows), ctypes.byref(ld), ctypes.byref(cols)) != 0
    assert b"without an item loss" in lib.p5_last_error()


def workspace_case(be, ocfg, items, B=2, L=12, T=6):
    """p5_train_workspace_bytes is still exact with the regularisers armed (trie_loss_cases.workspace_case's method): a forward inside exactly
    that many bytes succeeds and writes nothing behind them; row_terms is written in its 3 * rows floats and not behind them"""
    from openp5_amd.model import _ptr
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, _, _ = tl.item_batch(ocfg, items, B, L, T, 3, stray=False)
    for dtype in ("fp32", "bf16"):
        ref_logits = _ref_for(be, ocfg, dtype, (ids, ww, mask, labels), trie=ct)
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        dv = m._be.device
        off, tok, nxt = ct.device_arrays(dv)
        ids_d, ww_d, mask_d, lab_d = (m._i64(t, dv) for t in (ids, ww, mask, labels))
        m._sync_shadow()
        m._sync_transposed()
        need = int(be.lib.p5_train_workspace_bytes(m._engine, B, L, T))
        raw = torch.zeros(need + 256, dtype=torch.uint8, device=dv)
        skew = (-raw.data_ptr()) % 256
        ws = raw[skew:skew + need]
        guard = raw[skew + need:].clone()
        nll = torch.zeros(B * T, dtype=torch.float32, device=dv)
        rt = _sentinel((3 * B * T + 1,), torch.float32).to(dv)

        def call(nbytes):
            be.check(be.lib.p5_train_set_item_loss(m._engine, _ptr(off), _ptr(tok), _ptr(nxt), ct.n_nodes, None, 0, 1.0, None), "set_item_loss")
            be.check(be.lib.p5_train_set_item_regularizers(m._engine, _ptr(ref_logits), ref_logits.shape[1], _ptr(rt), 0.0, 0.0, None), "set_item_regularizers")
            return be.lib.p5_forward(m._engine, _ptr(ids_d), _ptr(ww_d), _ptr(mask_d), _ptr(lab_d), B, L, T, 0, _ptr(nll), _ptr(ws), nbytes, m._be.stream_ptr())
        assert call(need - 1) != 0
        assert b"workspace" in be.lib.p5_last_error()
        assert call(need) == 0
        sync(be)
        assert torch.equal(raw[skew + need:], guard), "the regularised forward wrote behind the bytes p5_train_workspace_bytes asked for"
        _guard_intact("row_terms", rt.cpu(), 3 * B * T)
        out = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, item_entropy=True, ref_logits=ref_logits)
        assert torch.equal(nll.cpu(), out["loss"].detach().cpu())
        assert torch.equal(rt[:B * T].cpu(), out["item_entropy"].detach().cpu()) and torch.equal(rt[B * T:2 * B * T].cpu(), out["item_kl"].detach().cpu())


# ---------------------------------------------------------------------------------------------------------
# 8. runner
# ---------------------------------------------------------------------------------------------------------
def runner_case(be, tmp, steps=3):
    """--train_item_loss 1 --item_loss_entropy_coef 0.01 --item_loss_kl_coef 0.1 --item_loss_kl_ref init on the synthetic pipeline
    (trie_loss_cases.runner_case's): finite losses, KL exactly 0 at step 0 and for as long as the weights have not moved (the reference is
    the policy; the schedule's first step runs at learning rate 0), positive from then on, the
    reference's weights unchanged; the same flags with coefficient 0 reproduce the run without them bit for bit.  The model has no dropout:
    under dropout the policy of step 0 is not the reference, which never drops."""
    import os
    from openp5_amd.runner import training_step
    from openp5_amd.model import P5ModelConfig
    tiny = P5ModelConfig(d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=2, dropout_rate=0.0)
    base = ("--train_item_loss", "1")
    runs = {}
    for name, flags in (("reg", base + ("--item_loss_entropy_coef", "0.01", "--item_loss_kl_coef", "0.1", "--item_loss_kl_ref", "init")),
                        ("zero", base + ("--item_loss_entropy_coef", "0", "--item_loss_kl_coef", "0", "--item_loss_kl_ref", "init")), ("plain", base)):
        d = os.path.join(tmp, name)
        os.makedirs(d)
        runner, model, tok, args = cases.make_pipeline(be, d, "fp32", dataset="Toy", n_users=12, n_items=24, n_inter=90, flags=["--batch_size", "8"] + list(flags),
                                                       model_cfg=tiny, vocab=2400)
        model.train()
        kw = runner._item_loss_kw()
        assert kw is not None
        ref = kw.get("ref_model")
        assert (ref is not None) == (name == "reg")
        if ref is not None:
            assert ref is not model and not ref.training and ref.compute_dtype == model.compute_dtype
            ref_w = ref._flat.detach().cpu().clone()
            assert torch.equal(ref_w, model._flat.detach().cpu()), "the reference starts as a copy of the policy"
        losses, kls, moved = [], [], []
        for i, batch in enumerate(runner.train_loader):
            if i == steps:
                break
            input_ids, attn, whole_ids, output_ids, output_attention = runner._to_dev(batch)[:5]
            if name == "reg":
                moved.append(not torch.equal(model._flat.detach().cpu(), ref_w))
            loss = training_step(model, runner.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), args.alpha, item_loss=kw)
            losses.append(float(loss))
            if name == "reg":
                kls.append(float(model.last_item_loss_terms[2]))
                assert float(model.last_item_loss_terms[1]) > 0
        assert all(math.isfinite(x) for x in losses), losses
        if name == "reg":
            assert kls[0] == 0.0 and not moved[0] and moved[-1], (kls, moved)
            assert all((k > 0) if mv else (k == 0.0) for k, mv in zip(kls, moved)), (kls, moved)
            assert torch.equal(ref._flat.detach().cpu(), ref_w), "the reference's weights moved"
            assert not torch.equal(model._flat.detach().cpu(), ref_w)
        runs[name] = (losses, model._flat.detach().cpu().clone())
        model.eval()
    # a refused flag combination is refused on every call: nothing half-built is cached
    d = os.path.join(tmp, "bad")
    os.makedirs(d)
    runner = cases.make_pipeline(be, d, "fp32", dataset="Toy", n_users=12, n_items=24, n_inter=90, flags=["--batch_size", "8"] + list(base) + ["--item_loss_kl_coef", "0.1"],
                                 model_cfg=tiny, vocab=2400)[0]
    for _ in range(2):
        with pytest.raises(ValueError, match="item_loss_kl_ref"):
            runner._item_loss_kw()
    assert runs["zero"][0] == runs["plain"][0] and torch.equal(runs["zero"][1], runs["plain"][1]), (runs["zero"][0], runs["plain"][0])
    assert runs["reg"][0] != runs["plain"][0]
