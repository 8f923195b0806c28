"""Cases of the listwise preference objectives (csrc/p5_pref.h, p5_op_pref_objective, p5_train_set_pref_objective,
P5T5Native.loss_and_backward(preference=) / sequence_logprobs / preference_step), shared by tests/test_pref_emu.py (host emulation) and
tests/test_gpu_pref.py (MI355X).

1. the two kernels through the C ABI against `ref_objective`, torch autograd in float64: loss, every seed, exact zeros where promised, the
   eight statistics; twice, the same bits; `np32_objective`, an fp32 NumPy restatement in the kernel's order, inside the same bounds.
2. bits: a list of one with pref_sft_coef = c is the plain step with target_weights (c G, 0, ...), on every backward route; no pair and c = 0
   moves nothing.
3. meaning: loss and gradients against the objective restated on the oracle's item NLL under autograd.
4. composition: preference_step == sample_slates + policy_batch + sequence_logprobs + loss_and_backward by hand.
5. it does what it is for: repeated preference_steps raise the mean margin and the gold log-probability.
6. refusals name their cause and precede every launch.
7. the runner's flags: train, log, resume; defaults = the parent's calls."""
import math

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases
from tests import clip_cases as cc
from tests import multi_target_cases as mt
from tests import policy_cases as pc
from tests import trie_loss_cases as tl
from tests.cases import sync

KINDS = {"pl": 0, "ipo": 1}
U = 2.0 ** -24

# ---------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------
# one pair; no pair possible (SFT only); odd sizes; G * T = 512; two targets per thread and scans across all four waves; a partial last wave
KERNEL_SHAPES = ((1, 2, 1), (1, 1, 3), (3, 5, 7), (2, 64, 8), (2, 512, 1), (5, 300, 1))
# (kind, depth (0 = full), ref_lp given, length_normalize, pref_mask given): every value of every option, and PL's depths 1 / 2 / full / above n - 1
KERNEL_OPTIONS = (("pl", 1, True, False, True), ("pl", 1, False, True, False), ("pl", 2, True, True, True), ("pl", 2, False, False, False),
                  ("pl", 0, True, False, False), ("pl", 0, False, True, True), ("pl", 1000, True, False, True), ("ipo", 0, True, False, True),
                  ("ipo", 0, False, True, False), ("ipo", 0, True, True, False))
N_USER_KINDS = 9
BETA, SFT = 0.5, 0.25
GAP = 120.0
# sequential roundings of one block-level sum: 2 slots of a thread, block_reduce (6 + 3), the finish kernel's stride over users, its
# block_reduce (6 + 3), a divide and the final addition
SUM_OPS = 24
# one (max, sum) combine: two expf (2 ulp each; their arguments are exact differences of fp32 values up to a rounding u |x|, which exp turns
# into a relative u |x| e^-|x| <= 0.37 u of a term that carries weight e^-|x|), two multiplies and an addition -> 8 u relative in the sum;
# a slot's path through a scan: 1 in-thread + 6 shuffle steps + 1 exclusive + 3 waves + 2 own slots = 13 combines, taken as 16
LSE_ABS = 16 * 8 * U + 2 * U * math.log(512.0)          # ... and logf (2 ulp) of a sum <= 512: the absolute error of a log-sum-exp beside u |L|
TINY = 2.0 ** -126          # the number format's floor: fp32 has no normal value below it, and the device may flush what lies below to zero


def kernel_problem(B, G, T, shift=0, mask_null=False, seed=0, use_ref=True, ln=False):
    """User b is of kind (b + shift) % 9:
      0 all targets listed            1 the first target skipped            2 one target listed (not the first)      3 none listed
      4 a listed target with cnt = 0 in the middle (skipped by its count)   5 the tail labelled -100 under attention 1
      6 all h equal (identical rows)  7 the first h 120 above the rest      8 the first h 120 below the rest
    A skip is pref_mask = 0, or -- `mask_null`: the run passes no pref_mask -- attention 0.  ref is NaN wherever it must not be read: where the
    attention is 0 and, with a pref_mask, on every target it does not list.  Under the options of the run (`use_ref`, `ln`) no random target's h
    lies within 2e-3 of its user's first: such a target's first NLL is raised by 0.02 until it does not (the reference asserts the outcome)."""
    g = np.random.default_rng(1000 * seed + 100 * B + 10 * G + T + 7 * shift)
    n = B * G
    nll = g.uniform(0.05, 3.0, (n, T)).astype(np.float32)
    ref = (-g.uniform(0.05, 3.0, (n, T))).astype(np.float32)
    attn = np.zeros((n, T), np.int64)
    labels = g.integers(3, 50, (n, T)).astype(np.int64)
    pm = np.ones(n, np.int32)
    for tg in range(n):
        attn[tg, :int(g.integers(1, T + 1))] = 1
    kinds = []
    for b in range(B):
        kind = (b + shift) % N_USER_KINDS
        kinds.append(kind)
        u = slice(b * G, (b + 1) * G)
        if kind == 1:
            pm[b * G] = 0
        if kind == 2:
            pm[u] = 0
            pm[b * G + G // 2] = 1
        if kind == 3:
            pm[u] = 0
        if kind == 4:
            attn[b * G + G // 2] = 0
        if kind == 5:
            attn[u] = 1
            labels[u, max(T - 2, 0):] = -100
        if kind in (6, 7, 8):
            nll[u], ref[u], attn[u] = nll[b * G], ref[b * G], attn[b * G]
        if kind in (7, 8):
            # a gap of 120 in h whatever beta, the reference and the normalisation are: added to the first attended token
            who = slice(b * G + 1, (b + 1) * G) if kind == 7 else slice(b * G, b * G + 1)
            nll[who, 0] += np.float32(GAP / BETA * T)
    if mask_null:
        attn[pm == 0] = 0
    ref[attn == 0] = np.nan
    ref_mask = ref.copy()
    ref_mask[pm == 0] = np.nan
    for _ in range(8):
        md = (attn != 0).astype(np.float64)
        cp = np.maximum(md.sum(1), 1) if ln else 1.0
        h = BETA * (-(nll * md).sum(1) - (np.nan_to_num(ref) * md).sum(1) * use_ref) / cp
        for b, idx in enumerate(_lists(dict(attn=attn, pm=pm), B, G, mask_null)):
            if kinds[b] < 6:
                for j in idx[1:]:
                    if abs(h[idx[0]] - h[j]) < 2e-3:
                        nll[j, 0] += np.float32(0.02)
    return dict(nll=nll, ref=ref if mask_null else ref_mask, attn=attn, labels=labels, pm=pm, kinds=kinds)


def _lists(pr, B, G, mask_null):
    cnt = (pr["attn"] != 0).sum(1)
    listed = (cnt > 0) & (np.ones_like(pr["pm"], bool) if mask_null else pr["pm"] != 0)
    return [np.nonzero(listed[b * G:(b + 1) * G])[0] + b * G for b in range(B)]


def _depth(depth, n):
    return 0 if n < 2 else min(depth if depth > 0 else n - 1, n - 1)


def ref_objective(pr, B, G, T, kind, depth, use_ref, ln, mask_null, beta=BETA, sft=SFT):
    """float64 restatement under autograd (beta, sft_coef: the fp32 values the kernel gets).  Returns loss, seeds [n, T] (0 at labels -100),
    the statistics, and the derived bounds: `loss_tol`, `seed_tol` [n, T], `stat_tol` [8]."""
    n = B * G
    beta, sft = float(np.float32(beta)), float(np.float32(sft))
    nll = torch.from_numpy(pr["nll"]).double().requires_grad_(True)
    m = torch.from_numpy(pr["attn"] != 0)
    md = m.double()
    cnt = md.sum(1)
    c1 = cnt.clamp(min=1)
    cp = c1 if ln else torch.ones_like(c1)
    s = (nll * md).sum(1)
    r = torch.where(m, torch.from_numpy(np.nan_to_num(pr["ref"])).double(), torch.zeros((), dtype=torch.float64)).sum(1) if use_ref else torch.zeros_like(s)
    delta = (-s - r) / cp
    h = beta * delta
    lists = _lists(pr, B, G, mask_null)
    # the absolute error of every h: two sums of T terms, their difference (relative to |s| + |r|: it may cancel), a divide, a multiply
    eh = ((T + 4) * U * beta * (s.detach().abs() + r.abs()) / cp).numpy()
    hd, dd = h.detach().numpy(), delta.detach().numpy()
    pref, sfts, loss_tol = [], [], 0.0
    gtol = np.zeros(n)                                    # the absolute error of d l_b / d Delta of every target
    st = dict(users=0, pairs=0, wins=0, hf=0.0, sh=0.0, sm=0.0, nl=0, nn=0, eh=0.0)
    for idx in lists:
        nb = len(idx)
        if nb >= 1:
            sfts.append(sft * s[idx[0]] / c1[idx[0]])
            st["nl"] += 1
            st["nn"] += nb
        if nb < 2:
            continue
        ti = torch.from_numpy(idx)
        hb = h[ti]
        hbd, ehb = hd[idx], eh[idx]
        # the reference alone: statistic 1 is exact -- no pair's sign hangs on a rounding (rows of equal bits give a margin of exactly 0)
        marg = hbd[0] - hbd[1:]
        same = np.array([np.array_equal(pr["nll"][j], pr["nll"][idx[0]]) and np.array_equal(pr["attn"][j], pr["attn"][idx[0]]) for j in idx[1:]])
        assert ((np.abs(marg) > 1e-3) | (same & (marg == 0))).all(), marg
        st["users"] += 1; st["pairs"] += nb - 1; st["wins"] += int((marg > 0).sum()); st["hf"] += hbd[0]; st["sh"] += hbd[1:].sum(); st["sm"] += marg.sum()
        st["eh"] = max(st["eh"], float(ehb.max()))
        if kind == "pl":
            Db = _depth(depth, nb)
            L = torch.flip(torch.logcumsumexp(torch.flip(hb, [0]), 0), [0])
            terms = (L - hb)[:Db]
            pref.append(terms.sum())
            Ld = L.detach().numpy()
            eL = ehb.max() + LSE_ABS + U * np.abs(Ld)
            loss_tol += float((eL[:Db] + ehb[:Db] + U * np.abs(Ld - hbd)[:Db]).sum()) + SUM_OPS * U * float(terms.detach().abs().sum())
            negL = torch.from_numpy(-Ld[:Db])
            A = torch.logcumsumexp(negL, 0).numpy()
            A = np.concatenate([A, np.full(nb - Db, A[-1])])
            eA = eL.max() + LSE_ABS + U * np.abs(A)
            # an absolute error in an exponent is a relative one behind exp: e^x (e_x + 2 ulp of expf), then the subtraction and beta
            ex = np.exp(hbd + A)
            e_x = ehb + eA + U * np.maximum(1.0, np.abs(hbd) + np.abs(A))
            gtol[idx] = beta * (ex * (e_x + 4 * U) + 3 * U * np.abs(ex - (np.arange(nb) < Db)) + TINY)
        else:
            tau = 1.0 / (2.0 * beta)
            v = (delta[ti[0]] - delta[ti[1:]]) - tau
            pref.append((v * v).mean())
            vd = v.detach().numpy()
            ev = (ehb[0] + ehb[1:]) / beta + U * (np.abs(dd[idx[0]] - dd[idx[1:]]) + np.abs(vd) + tau)
            loss_tol += float((2 * np.abs(vd) * ev + 4 * U * vd * vd).sum()) / (nb - 1) + SUM_OPS * U * float((vd * vd).mean())
            gj = (2 * ev + 4 * U * 2 * np.abs(vd)) / (nb - 1)
            gtol[idx[1:]] = gj
            gtol[idx[0]] = gj.sum() + SUM_OPS * U * float(2 * np.abs(vd).sum()) / (nb - 1)
    zero = torch.zeros((), dtype=torch.float64)
    lp = (sum(pref) if pref else zero) / B
    ls = (sum(sfts) if sfts else zero) / B
    loss = lp + ls
    if loss.requires_grad:
        loss.backward()
    seeds = (nll.grad.numpy() if nll.grad is not None else np.zeros((n, T))) * (pr["labels"] != -100)
    sft_mag = float(sum(abs(float(x.detach())) for x in sfts)) / B
    lp_tol = 2 * (loss_tol / B + SUM_OPS * U * abs(float(lp.detach())))
    ls_tol = 2 * (T + 4 + SUM_OPS) * U * sft_mag
    # a seed: (d l / d Delta) / c' / B (two more roundings), plus the SFT part (a divide, two multiplies, the addition)
    cpn = cp.numpy()
    seed_tol = 2 * ((gtol / cpn / B)[:, None] + 6 * U * np.abs(seeds) + TINY)
    users, pairs = st["users"], st["pairs"]
    hs = max(1.0, abs(st["hf"]) / max(users, 1), abs(st["sh"]) / max(pairs, 1))
    mean_tol = 2 * (st["eh"] + SUM_OPS * U * hs)
    stats = np.array([users, st["wins"] / max(pairs, 1), st["hf"] / max(users, 1), st["sh"] / max(pairs, 1), st["sm"] / max(pairs, 1), float(lp.detach()), float(ls.detach()),
                      st["nn"] / max(st["nl"], 1)])
    stat_tol = np.array([0.0, 2.0 ** -22, mean_tol, mean_tol, 2 * mean_tol, lp_tol, ls_tol, 2 * U * stats[7]])
    listed = np.zeros(n, bool)
    for idx in lists:
        listed[idx] = True
    return dict(loss=float(loss.detach()), seeds=seeds, stats=stats, loss_tol=lp_tol + ls_tol, seed_tol=seed_tol, stat_tol=stat_tol, listed=listed, lists=lists)


# ---- the kernel's arithmetic in fp32 NumPy, in the kernel's order
_F = np.float32
_NINF = _F(-np.inf)


def _comb(a, b):
    """p5_pref_comb on arrays of (m, s, c)"""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.maximum(a[0], b[0])
        sm = a[1] * np.exp((a[0] - m).astype(_F)).astype(_F) + b[1] * np.exp((b[0] - m).astype(_F)).astype(_F)
        return m, np.where(m == _NINF, _F(0), sm).astype(_F), (a[2] + b[2]).astype(_F)


def _ident(shape):
    return np.full(shape, _NINF, _F), np.zeros(shape, _F), np.zeros(shape, _F)


def _scan(v, rev):
    """p5_pref_scan: v = (m, s, c) arrays [256]; the exclusive scan over threads, waves of 64"""
    v = tuple(x.reshape(4, 64).copy() for x in v)
    lane = np.arange(64)
    d = 1
    while d < 64:
        src = lane + d if rev else lane - d
        ok = (src >= 0) & (src < 64)
        o = tuple(x[:, src & 63] for x in v)
        nv = _comb(v, o) if rev else _comb(o, v)
        v = tuple(np.where(ok[None, :], a, b) for a, b in zip(nv, v))
        d *= 2
    nbr = lane + 1 if rev else lane - 1
    ok = (nbr >= 0) & (nbr < 64)
    ex = tuple(np.where(ok[None, :], x[:, nbr & 63], i) for x, i in zip(v, _ident((4, 64))))
    tot = tuple(x[:, 0 if rev else 63] for x in v)
    out = []
    for w in range(4):
        pre = _ident(())
        if rev:
            for k in range(3, w, -1):
                pre = _comb(tuple(t[k] for t in tot), pre)
            out.append(_comb(tuple(x[w] for x in ex), tuple(np.broadcast_to(p, (64,)) for p in pre)))
        else:
            for k in range(w):
                pre = _comb(pre, tuple(t[k] for t in tot))
            out.append(_comb(tuple(np.broadcast_to(p, (64,)) for p in pre), tuple(x[w] for x in ex)))
    return tuple(np.concatenate([o[i] for o in out]).astype(_F) for i in range(3)), float((tot[2][0] + tot[2][1]) + (tot[2][2] + tot[2][3]))


def _one(h):
    on = h != _NINF
    return h.astype(_F), on.astype(_F), on.astype(_F)


def np32_objective(pr, B, G, T, kind, depth, use_ref, ln, mask_null, beta=BETA, sft=SFT):
    """loss and seeds as p5_pref_objective_kernel / p5_pref_finish_kernel form them, in fp32 (block_reduce's order is restated as a sum in index
    order: its roundings are inside SUM_OPS either way)"""
    beta, sft, invb = _F(beta), _F(sft), _F(1) / _F(B)
    seeds = np.zeros((B * G, T), _F)
    lp = ls = _F(0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            h = np.full(512, _NINF, _F)
            dl = np.full(512, _NINF, _F)
            cn, cpr, sf = np.ones(512, _F), np.ones(512, _F), np.zeros(512, _F)
            for g in range(G):
                tg = b * G + g
                want = mask_null or pr["pm"][tg] != 0
                num = rs = cnt = _F(0)
                for t in range(T):
                    on = pr["attn"][tg, t] != 0
                    num = _F(num + pr["nll"][tg, t] * _F(on))
                    if want and use_ref and on:
                        rs = _F(rs + pr["ref"][tg, t])
                    cnt = _F(cnt + _F(on))
                cn[g] = max(cnt, _F(1))
                cpr[g] = cn[g] if ln else _F(1)
                sf[g] = _F(num / cn[g])
                if want and cnt > 0:
                    dl[g] = _F(_F(-num - rs) / cpr[g])
                    h[g] = _F(beta * dl[g])
            h0, h1, d0, d1 = h[0::2], h[1::2], dl[0::2], dl[1::2]
            x0, x1 = _one(h0), _one(h1)
            above, nb = _scan(_comb(x0, x1), True)
            suf1 = _comb(x1, above)
            suf0 = _comb(x0, suf1)
            pos = np.empty(512, _F)
            pos[0::2], pos[1::2] = nb - suf0[2], nb - suf1[2]
            on = h != _NINF
            Db = _depth(depth, int(nb))
            gd = np.zeros(512, _F)
            lpart = _F(0)
            first = int(np.nonzero(on & (pos == 0))[0][0]) if nb >= 1 else -1
            if kind == "pl":
                L = np.empty(512, _F)
                L[0::2], L[1::2] = suf0[0] + np.log(suf0[1]).astype(_F), suf1[0] + np.log(suf1[1]).astype(_F)
                act = on & (pos < Db)
                y = np.where(act, -L, _NINF).astype(_F)
                y0, y1 = _one(y[0::2]), _one(y[1::2])
                below, _ = _scan(_comb(y0, y1), False)
                pre0 = _comb(below, y0)
                pre1 = _comb(pre0, y1)
                A = np.empty(512, _F)
                A[0::2], A[1::2] = pre0[0] + np.log(pre0[1]).astype(_F), pre1[0] + np.log(pre1[1]).astype(_F)
                if nb >= 2:
                    gd = np.where(on, beta * (np.exp((h + A).astype(_F)).astype(_F) - act.astype(_F)), _F(0)).astype(_F)
                    for e in np.nonzero(act)[0]:
                        lpart = _F(lpart + _F(L[e] - h[e]))
            elif nb >= 2:
                tau, inv = _F(1) / _F(_F(2) * beta), _F(1) / _F(max(nb - 1, 1))
                gf = _F(0)
                for e in np.nonzero(on & (pos > 0))[0]:
                    v = _F(_F(dl[first] - dl[e]) - tau)
                    lpart = _F(lpart + _F(_F(v * v) * inv))
                    gd[e] = _F(_F(_F(-2) * v) * inv)
                    gf = _F(gf + _F(_F(_F(2) * v) * inv))
                gd[first] = gf
            if nb >= 2:
                lp = _F(lp + lpart)
            for g in range(G):
                if not on[g]:
                    continue
                gs = _F(_F(-gd[g] / cpr[g]) * invb) if nb >= 2 else _F(0)
                val = gs
                if g == first:
                    gf = _F(_F(invb / cn[g]) * sft)
                    val = _F(gs + gf) if nb >= 2 else gf
                    ls = _F(ls + _F(sft * sf[g]))
                tg = b * G + g
                seeds[tg] = np.where((pr["attn"][tg] != 0) & (pr["labels"][tg] != -100), val, _F(0))
    return dict(loss=float(_F(_F(lp / _F(B)) + _F(ls / _F(B)))), seeds=seeds.astype(np.float64))


def run_pref_op(be, pr, B, G, T, kind, depth, use_ref, ln, mask_null, beta=BETA, sft=SFT):
    from openp5_amd.model import _ptr
    dv = be.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dv)       # noqa: E731
    f = lambda k: torch.full((k,), float("nan"), dtype=torch.float32, device=dv)      # noqa: E731
    loss, seed, part, stats = f(1), f(B * G * T), f(16 * B), f(8)
    d_nll, d_ref, d_attn, d_lab, d_pm = t(pr["nll"]), t(pr["ref"]), t(pr["attn"]), t(pr["labels"]), t(pr["pm"])
    rc = be.lib.p5_op_pref_objective(_ptr(loss), _ptr(seed), _ptr(part), _ptr(stats), _ptr(d_nll), _ptr(d_ref) if use_ref else None, _ptr(d_attn), _ptr(d_lab),
                                     None if mask_null else _ptr(d_pm), KINDS[kind], beta, depth, 1 if ln else 0, sft, B, G, T, be.stream_ptr())
    be.check(rc, "p5_op_pref_objective")
    sync(be)
    return dict(loss=loss.cpu().numpy(), seed=seed.cpu().numpy(), stats=stats.cpu().numpy())


def _check_against(tag, ref, loss, seeds, stats=None):
    assert math.isfinite(loss) and abs(loss - ref["loss"]) <= ref["loss_tol"], (tag, loss, ref["loss"], ref["loss_tol"])
    assert np.isfinite(seeds).all(), tag
    err = np.abs(seeds - ref["seeds"])
    assert (err <= ref["seed_tol"]).all(), (tag, float((err - ref["seed_tol"]).max()), float(err.max()))
    if stats is not None:
        assert np.isfinite(stats).all() and (np.abs(stats - ref["stats"]) <= ref["stat_tol"]).all(), (tag, stats, ref["stats"], ref["stat_tol"])


def kernel_case(be, B, G, T, option):
    kind, depth, use_ref, ln, mask_null = option[0], option[1], option[2], option[3], not option[4]
    seen = set()
    for shift in range(0, N_USER_KINDS, B):
        pr = kernel_problem(B, G, T, shift, mask_null, use_ref=use_ref, ln=ln)
        seen.update(pr["kinds"])
        tag = f"B={B} G={G} T={T} {option} shift={shift}"
        ref = ref_objective(pr, B, G, T, kind, depth, use_ref, ln, mask_null)
        runs = [run_pref_op(be, pr, B, G, T, kind, depth, use_ref, ln, mask_null) for _ in range(2)]
        for k, v in runs[0].items():
            assert v.tobytes() == runs[1][k].tobytes(), f"{tag}: two runs differ in {k}"
        got = runs[0]
        n = B * G
        seeds = got["seed"].reshape(n, T).astype(np.float64)
        print(f"[pref kernel {tag}] loss {got['loss'][0]:.7f} ref {ref['loss']:.7f} (tol {ref['loss_tol']:.2e}), stats {got['stats'].tolist()}")
        _check_against(tag, ref, float(got["loss"][0]), seeds, got["stats"].astype(np.float64))
        # exact zeros where promised: skipped targets, rows not attended, labels -100; a user without a pair and sft_coef's first target aside
        assert (seeds[~ref["listed"]] == 0).all() and (seeds[pr["attn"] == 0] == 0).all() and (seeds[pr["labels"] == -100] == 0).all(), tag
        for idx in ref["lists"]:
            if len(idx) < 2:
                assert all((seeds[j] == 0).all() for j in idx[1:]), tag
                if len(idx) == 1:          # the SFT seed alone, with p5_masked_mean_g_kernel's bits
                    j = idx[0]
                    want = np.float32(np.float32(np.float32(1) / np.float32(B)) / np.float32(max(int((pr["attn"][j] != 0).sum()), 1))) * np.float32(SFT)
                    assert np.array_equal(got["seed"].reshape(n, T)[j], np.where((pr["attn"][j] != 0) & (pr["labels"][j] != -100), want, np.float32(0))), tag
        if shift == 0 and G * T <= 64:          # (the NumPy restatement walks every element in Python)
            cpu = np32_objective(pr, B, G, T, kind, depth, use_ref, ln, mask_null)
            _check_against(tag + " numpy fp32", ref, cpu["loss"], cpu["seeds"])
    assert seen == set(range(N_USER_KINDS)), seen
    # no listed target at all: the documented constants
    pr0 = kernel_problem(B, G, T, 0, False)
    pr0["pm"][:] = 0
    got = run_pref_op(be, pr0, B, G, T, kind, depth, False, ln, False)
    assert got["stats"].tolist() == [0] * 8 and float(got["loss"][0]) == 0 and (got["seed"] == 0).all(), got["stats"]


# ---------------------------------------------------------------------------------------------------------
# 2. bits
# ---------------------------------------------------------------------------------------------------------
def bits_case(be, ocfg, items, route, dtype, G, c=0.5, dropout=0.0):
    """pref_mask lists slot 0 only, pref_sft_coef = c: every .grad equals loss_and_backward(target_weights=[c G, 0, ...]) bit for bit (G a
    power of two: (1 / (B G)) (c G) and (1 / B) c round alike).  Route "ce_free" (bf16, dropout on): the logit-free head, where the plain
    call's loss kernel writes the seeds itself; the dropout seed is reset in front of every call."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn, _, ct = cc._route_batch(ocfg, items, route, G)
    B = labels.shape[0]
    kw = {} if ct is None else dict(trie=ct, temperature=0.8, item_head="trie" if route == "item_trie" else "dense")
    w = torch.zeros(B, G)
    w[:, 0] = c * G
    pm = torch.zeros(B, G, dtype=torch.int32)
    pm[:, 0] = 1

    def fresh():
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        tl._train_mode(m, dropout, 77)
        return m
    if route == "ce_free":
        be.check(be.lib.p5_set_option(b"gemm_wide_min_tiles", 1), "opt")
    try:
        p = fresh()
        loss_p = p.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, **kw)
        assert p.last_pref_stats is None
        q = fresh()
        loss_q = q.loss_and_backward(ids, ww, mask, labels, out_attn, preference="pl", pref_mask=pm, pref_sft_coef=c, ref_logprobs=torch.full(labels.shape, float("nan")),
                                     **kw)
        sync(be)
        st = q.last_pref_stats.cpu()
    finally:
        be.lib.p5_set_option(b"gemm_wide_min_tiles", 160)
    gp, gq = p._grads.detach().cpu(), q._grads.detach().cpu()
    assert float(gp.abs().max()) > 0
    assert torch.equal(gp, gq), (route, dtype, G, float((gp - gq).abs().max()))
    for (name, a), (_, b_) in zip(p.named_parameters(), q.named_parameters()):
        assert torch.equal(a.grad.cpu(), b_.grad.cpu()), name
    assert float(st[0]) == 0 and float(st[5]) == 0 and float(st[6]) == float(loss_q), st
    assert abs(float(loss_q) - float(loss_p)) <= cc.SUM_TOL(B, G, labels.shape[-1]) * max(1.0, abs(float(loss_p))), (float(loss_q), float(loss_p))


def no_pair_case(be, ocfg, items, dtype="fp32", G=3):
    """every user's list has fewer than two targets and pref_sft_coef = 0: loss 0, every gradient an exact zero"""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn, _, ct = cc._route_batch(ocfg, items, "item_dense", G)
    B = labels.shape[0]
    pm = torch.zeros(B, G, dtype=torch.int32)
    pm[0, 1] = 1
    pm[1, 0] = 1
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    for kind in ("pl", "ipo"):
        m.zero_grad()
        loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, trie=ct, temperature=0.8, preference=kind, pref_mask=pm)
        sync(be)
        assert float(loss) == 0 and bool((m._grads.detach().cpu() == 0).all()), (kind, float(loss))
        assert m.last_pref_stats.cpu().tolist()[:7] == [0] * 7


# ---------------------------------------------------------------------------------------------------------
# 3. meaning
# ---------------------------------------------------------------------------------------------------------
MEANING = {"pl1_ref": dict(preference="pl", pref_depth=1, ref=True), "pl_full": dict(preference="pl", pref_depth=None, pref_length_normalize=True),
           "ipo": dict(preference="ipo", ref=True, pref_sft_coef=0.3), "ragged": dict(preference="pl", pref_depth=2, ragged=True, pref_sft_coef=0.3)}


def meaning_case(be, ocfg, items, name, B=3, L=12, T=6, G=4, tau=0.8, beta=0.5):
    """fp32: loss and every gradient of loss_and_backward(preference=, trie=) against the objective restated in float64 on the oracle's item NLL
    (tl.oracle_item_nll of the replicated batch) under autograd -- the tolerances of clip_cases.meaning_case (mt.NLL_TOL / mt.GRAD_TOL)"""
    opt = dict(MEANING[name])
    use_ref, ragged = opt.pop("ref", False), opt.pop("ragged", False)
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn, _, ct = cc._route_batch(ocfg, items, "item_dense", G, B, L, T)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    ref_lp = None
    if use_ref:
        ref = m.frozen_copy()
        with torch.no_grad():
            ref._flat.mul_(1.02)
        ref.mark_params_updated()
        ref_lp = ref.sequence_logprobs(ids, ww, mask, labels, trie=ct, temperature=tau)
        assert ref_lp.shape == labels.shape and bool((ref_lp <= 0).all()) and float(ref_lp.abs().max()) > 0
    pm = None
    if ragged:
        pm = torch.ones(B, G, dtype=torch.int32)
        pm[0, 0] = 0
        pm[1, 1:] = 0
        pm[2, 2] = 0
    loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, trie=ct, temperature=tau, pref_beta=beta, ref_logprobs=ref_lp, pref_mask=pm, **opt)
    sync(be)
    st = m.last_pref_stats.cpu()
    Pq = mt._oracle_params(params, "bf16")          # (float64)
    nll_o, _, _ = tl.oracle_item_nll(Pq, ocfg, mt.rep(ids, G), mt.rep(ww, G), mt.rep(mask, G), labels.view(B * G, T), ct, tau, None)
    md = (out_attn != 0).double()
    cnt = md.sum(2)
    s = (nll_o.view(B, G, T) * md).sum(2)
    r = (ref_lp.cpu().double() * md).sum(2) if use_ref else torch.zeros_like(s)
    cp = cnt.clamp(min=1) if opt.get("pref_length_normalize") else torch.ones_like(cnt)
    delta = (-s - r) / cp
    h = float(np.float32(beta)) * delta
    total = torch.zeros((), dtype=torch.float64)
    depth, sc = opt.get("pref_depth"), float(np.float32(opt.get("pref_sft_coef", 0.0)))
    for b in range(B):
        idx = [g for g in range(G) if (pm is None or int(pm[b, g]) != 0) and float(cnt[b, g]) > 0]
        if idx:
            total = total + sc * s[b, idx[0]] / cnt[b, idx[0]].clamp(min=1)
        if len(idx) < 2:
            continue
        if opt["preference"] == "pl":
            hb = h[b, idx]
            for k in range(_depth(depth or 0, len(idx))):
                total = total + torch.logsumexp(hb[k:], 0) - hb[k]
        else:
            v = (delta[b, idx[0]] - delta[b, idx[1:]]) - 1.0 / (2.0 * float(np.float32(beta)))
            total = total + (v * v).mean()
    loss_o = total / B
    loss_o.backward()
    lo_ = float(loss_o.detach())
    _, worst = mt._fp32_errors(m, Pq, nll_o, nll_o)
    print(f"[pref meaning {name}] loss {float(loss):.6f} oracle {lo_:.6f}, worst gradient {worst[0]:.2e} ({worst[1]}), stats {st.tolist()}")
    assert float(st[0]) >= 2, st
    assert abs(float(loss) - lo_) <= mt.NLL_TOL * max(1.0, abs(lo_)), (float(loss), lo_)
    assert worst[0] <= mt.GRAD_TOL, worst


# ---------------------------------------------------------------------------------------------------------
# 4. composition
# ---------------------------------------------------------------------------------------------------------
def composition_case(be, ocfg, items, dtype="fp32", item_head="dense", negatives="slate", B=4, L=12, S=4, seed=11, with_ref=True, **kw):
    """preference_step(seed=s) against sample_slates / sample_items + policy_batch + sequence_logprobs + loss_and_backward by hand on a fresh
    model with the same weights: loss, gradient arena and statistics bit for bit; a draw that is the gold item is skipped"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    common = dict(temperature=0.8, item_head=item_head)
    pk = dict(preference="pl", pref_depth=1, pref_beta=0.5, pref_sft_coef=0.2)
    pk.update(kw)
    res = []
    for whole in (True, False):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        ref = None
        if with_ref:
            ref = m.frozen_copy()
            with torch.no_grad():
                ref._flat.mul_(1.01)
            ref.mark_params_updated()
        if whole:
            loss = m.preference_step(ids, ww, mask, labels, out_attn, ct, S, ref_model=ref, negatives=negatives, seed=seed, **pk, **common)
            pb = m.last_policy_batch
            hit, pmask = pb["rewards"].cpu(), pb["pref_mask"].cpu()
        else:
            if negatives == "slate":
                drawn = m.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=S, num_slates=1, temperature=0.8, seed=seed)
            else:
                drawn = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=0.8, seed=seed)
            pb = m.policy_batch(drawn["sequences"], labels, out_attn, S, baseline="none")
            pm = torch.cat([torch.ones(B, 1, dtype=torch.int32), (pb["rewards"].cpu() == 0).to(torch.int32)], 1)
            ref_lp = None if ref is None else ref.sequence_logprobs(ids, ww, mask, pb["labels"], trie=ct, **common)
            loss = m.loss_and_backward(ids, ww, mask, pb["labels"], pb["output_attention"], trie=ct, ref_logprobs=ref_lp, pref_mask=pm, **pk, **common)
        sync(be)
        res.append((loss.detach().cpu().clone(), m._grads.detach().cpu().clone(), m.last_pref_stats.cpu().clone()))
    (l0, g0, s0), (l1, g1, s1) = res
    assert math.isfinite(float(l0)) and float(g0.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(s0, s1), (float(l0), float(l1), float((g0 - g1).abs().max()))
    assert torch.equal(pmask[:, 0], torch.ones(B, dtype=torch.int32)) and torch.equal(pmask[:, 1:], (hit == 0).to(torch.int32))
    return hit, pmask, s0


def hit_skipped_case(be, ocfg, B=4, L=10, S=6):
    """a trie of 8 items and slates of 6 distinct ones: some user's slate holds the gold item; that slot is skipped -- the user's list is
    one shorter -- and the draw's rows get no gradient seed"""
    items = cases.make_items(8, 5, hi=60)
    hit, pmask, st = composition_case(be, ocfg, items, B=B, L=L, S=S, with_ref=False)
    assert float(hit.sum()) > 0, "the case needs a draw that hits the gold item"
    assert int(pmask.sum()) == B * (S + 1) - int(hit.sum())
    assert abs(float(st[7]) - float(pmask.sum()) / B) <= 1e-6 * (S + 1), (st, pmask)


# ---------------------------------------------------------------------------------------------------------
# 5. it does what it is for
# ---------------------------------------------------------------------------------------------------------
def learns_case(be, ocfg, steps=5, B=4, S=2, L=10, lr=1e-4, beta=0.5):
    """softmax-DPO against a frozen copy of the initial weights, negatives from slates of 2 on a trie of 8 items.  Returns the mean margin
    (statistic 4) of the first and the last step and the gold log-probability before and after."""
    from openp5_amd.optim import FusedAdamW
    items = cases.make_items(8, 5, hi=60)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    ref = m.frozen_copy()
    opt = FusedAdamW(m, lr=lr, weight_decay=0.0, max_grad_norm=1.0)
    before = pc._gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    margins = []
    for i in range(steps):
        m.preference_step(ids, ww, mask, labels, out_attn, ct, S, pref_beta=beta, ref_model=ref, seed=1000 + i)
        margins.append(m.last_pref_stats.clone())
        opt.step()
        m.zero_grad()
    sync(be)
    after = pc._gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    margins = [float(s.cpu()[4]) for s in margins]
    print(f"[pref learns] gold log-probability {before:.4f} -> {after:.4f} after {steps} steps; mean margin {margins[0]:.4f} -> {margins[-1]:.4f}")
    return margins[0], margins[-1], before, after


# ---------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------
def abi_errors_case(be, ocfg, items):
    from openp5_amd.model import _ptr
    lib, dv = be.lib, be.device
    B, G, T = 2, 2, 3
    buf = torch.zeros(256, dtype=torch.float32, device=dv)
    f, part_, stats_, loss_, nll_, ref_ = buf[0:64], buf[64:128], buf[128:136], buf[136:137], buf[144:176], buf[176:208]
    i64 = torch.ones(B * G * T, dtype=torch.int64, device=dv)

    def op(kind=0, beta=0.5, depth=0, sft=0.0, seed=f, G_=G, nll=nll_):
        return lib.p5_op_pref_objective(_ptr(loss_), _ptr(seed), _ptr(part_), _ptr(stats_), _ptr(nll), _ptr(ref_), _ptr(i64), _ptr(i64), None, kind, beta, depth,
                                        0, sft, B, G_, T, be.stream_ptr())
    assert op() == 0
    sync(be)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    eng = m._engine

    def arm(kind=0, beta=0.5, depth=0, sft=0.0, seed=f, part=part_, stats=stats_):
        return lib.p5_train_set_pref_objective(eng, _ptr(ref_), None, kind, beta, depth, 0, sft, _ptr(seed), _ptr(part), _ptr(stats))
    for call in (op, arm):
        for kw, msg in ((dict(beta=0.0), b"beta"), (dict(beta=-1.0), b"beta"), (dict(beta=float("nan")), b"beta"), (dict(beta=float("inf")), b"beta"),
                        (dict(kind=2), b"unknown kind"), (dict(kind=-1), b"unknown kind"), (dict(depth=-1), b"depth"), (dict(sft=float("nan")), b"sft_coef"),
                        (dict(sft=float("inf")), b"sft_coef"), (dict(seed=None), b"null pointer")):
            assert call(**kw) != 0, kw
            assert msg in lib.p5_last_error(), (kw, lib.p5_last_error())
    assert arm(stats=None) != 0 and b"null pointer" in lib.p5_last_error()
    assert arm(part=None) != 0 and b"null pointer" in lib.p5_last_error()
    assert op(nll=None) != 0 and b"null pointer" in lib.p5_last_error()
    assert op(G_=513) != 0 and b"shapes" in lib.p5_last_error()
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn = mt.grouped_batch(ocfg, B, 8, T, G)
    old = torch.zeros(B * G * T, dtype=torch.float32, device=dv)

    def plain_forward_runs():
        with torch.no_grad():
            nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
        sync(be)
        assert bool(torch.isfinite(nll).all())
    # the clip objective armed as well, in either order
    assert lib.p5_train_set_clip_objective(eng, _ptr(old), None, 0.2, 0.2, 0, _ptr(f), _ptr(part_), _ptr(stats_)) == 0
    assert arm() != 0 and b"clip objective is armed" in lib.p5_last_error()
    plain_forward_runs_after_refusal = pytest.raises(Exception, match="p5_train_set_clip_objective")
    with plain_forward_runs_after_refusal:          # (the clip objective itself is still armed: its own refusal disarms it)
        plain_forward_runs()
    plain_forward_runs()
    # armed behind the truncated item loss, and behind the regularisers
    q = m._item_loss_setup(ct, 1.0, None, B, top_k=2)
    m._arm_item_loss(q, B * G, T, G)
    assert arm() != 0 and b"truncated item loss" in lib.p5_last_error()
    assert lib.p5_train_set_item_loss(eng, None, None, None, 0, None, 0, 1.0, None) != 0          # (a refused call disarms the item loss armed above)
    q = m._item_regularizers(m._item_loss_setup(ct, 1.0, None, B), B * G * T, None, 0.1, 0.0, fused=True)
    m._arm_item_loss(q, B * G, T, G)
    assert arm() != 0 and b"item regularizers" in lib.p5_last_error()
    assert lib.p5_train_set_item_loss(eng, None, None, None, 0, None, 0, 1.0, None) != 0
    plain_forward_runs()
    # p5_forward while armed names the objective -- and disarms it: the next plain forward runs
    assert arm() == 0
    with pytest.raises(Exception, match="p5_train_set_pref_objective"):
        plain_forward_runs()
    plain_forward_runs()
    # target_weights in the armed forward
    assert arm() == 0
    with pytest.raises(Exception, match="target_weights must be NULL"):
        m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=torch.ones(B, G))
    plain_forward_runs()
    loss = m.loss_and_backward(ids, ww, mask, labels, out_attn)
    sync(be)
    assert math.isfinite(float(loss)) and m.last_pref_stats is None


def model_errors_case(be, ocfg, items):
    """every refusal is a ValueError raised before anything is sampled or launched"""
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    ct = rank_cases.compiled(items)
    calls = []
    for name in ("_workspace", "_lane_workspace", "sample_items", "sample_slates", "_sample", "_arm_item_loss", "_engine_forward", "policy_batch"):
        real = getattr(m, name)
        setattr(m, name, (lambda real_, name_: lambda *a, **k: calls.append(name_) or real_(*a, **k))(real, name))
    B, G, T, S = 2, 3, 6, 3
    ids, ww, mask, labels, out_attn, w, _ = cc._route_batch(ocfg, items, "item_dense", G, B, 8, T)
    ref = torch.zeros(B, G, T)

    def lb(match, labels_=labels, attn_=out_attn, **kw):
        with pytest.raises(ValueError, match=match):
            m.loss_and_backward(ids, ww, mask, labels_, attn_, trie=kw.pop("trie", ct), **kw)
    lb("preference", preference="dpo")
    lb("preference", ref_logprobs=ref)
    lb("preference", pref_mask=torch.ones(B, G, dtype=torch.int32))
    for bad in (0.0, -0.1, float("nan"), float("inf"), "big"):
        lb("pref_beta", preference="pl", pref_beta=bad)
    for bad in (0, -1, 1.5, True):
        lb("pref_depth", preference="pl", pref_depth=bad)
    lb("pref_sft_coef", preference="ipo", pref_sft_coef=float("nan"))
    lb("top_k / top_p", preference="pl", top_k=2)
    lb("top_k / top_p", preference="pl", top_p=0.9)
    lb("target_weights", preference="pl", target_weights=w)
    lb("one objective", preference="pl", old_logprobs=ref, clip_eps=0.2)
    lb("regularisers", preference="pl", entropy_coef=0.1)
    lb("regularisers", preference="pl", kl_coef=0.1, ref_logits=torch.zeros(B * G * T, ocfg.vocab_size))
    lb(r"labels \[B, G, T\]", labels_=labels[:, 0], attn_=out_attn[:, 0], preference="pl")
    lb("ref_logprobs.*shaped like labels", preference="pl", ref_logprobs=ref[:, :, :-1])
    lb("pref_mask", preference="pl", pref_mask=torch.ones(B, G + 1, dtype=torch.int32))
    lb("pref_mask", preference="pl", pref_mask=torch.ones(B * G, dtype=torch.int32))
    gl, ga = labels[:, 0], out_attn[:, 0]

    def ps(match, **kw):
        with pytest.raises(ValueError, match=match):
            m.preference_step(ids, ww, mask, gl, ga, kw.pop("trie", ct), kw.pop("S_", S), **kw)
    ps("trie", trie=None)
    ps("preference", preference="dpo")
    ps("preference", preference=None)
    ps("pref_beta", pref_beta=0.0)
    ps("pref_depth", pref_depth=0)
    ps("pref_sft_coef", pref_sft_coef=float("inf"))
    ps("negatives", negatives="beam")
    ps("num_negatives", S_=0)
    ps("num_negatives", S_=1.5)
    ps(r"G \* T <= 512", S_=102, negatives="sample")
    assert not calls, f"a refused call reached the sampler or the engine: {calls}"
    assert m.last_pref_stats is None


# ---------------------------------------------------------------------------------------------------------
# 7. the runner
# ---------------------------------------------------------------------------------------------------------
PREF_FLAGS = ("--train_item_loss", "1", "--train_preference", "pl", "--pref_negatives", "3", "--pref_beta", "0.5", "--pref_sft_coef", "0.1")


def _pipeline(be, tmp, name, flags, dropout=0.0, n_users=4):
    """policy_cases._pipeline on half its users (the emulator pays every training row): batches of 4, at least 4 of them per epoch"""
    import os
    from openp5_amd.model import P5ModelConfig
    tiny = P5ModelConfig(d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=2, dropout_rate=dropout)
    d = os.path.join(tmp, name)
    os.makedirs(d, exist_ok=True)
    return cases.make_pipeline(be, d, "fp32", dataset="Toy", n_users=n_users, n_items=16, n_inter=5 * n_users, flags=["--batch_size", "4", "--lr", "3e-3"] + list(flags),
                               model_cfg=tiny, vocab=2400)


def runner_case(be, tmp, caplog=None):
    """a short run with --train_preference pl completes, draws with a seed per step and logs the statistics; the flags are checked at
    construction"""
    import logging
    runner, model, _, _ = _pipeline(be, tmp, "on", PREF_FLAGS + ("--epochs", "1", "--logging_step", "2"))
    seen = []
    real = model.preference_step
    model.preference_step = lambda *a, **k: seen.append(k) or real(*a, **k)
    model.policy_step = lambda *a, **k: pytest.fail("policy_step called under --train_preference")
    if caplog is not None:
        caplog.set_level(logging.INFO)
    before = model._flat.detach().cpu().clone()
    losses = runner.train()
    assert len(losses) == 1 and math.isfinite(losses[0])
    assert len(seen) == len(runner.train_loader) and runner.optimizer.t == len(seen)
    assert all(k["num_negatives"] == 3 and k["preference"] == "pl" and k["pref_depth"] == 1 and k["pref_beta"] == 0.5 and k["pref_sft_coef"] == 0.1
               and k["negatives"] == "slate" and k["ref_model"] is not None and k["trie"] is not None for k in seen)
    assert len({k["seed"] for k in seen}) == len(seen), "every step draws with its own seed"
    assert not torch.equal(before, model._flat.detach().cpu())
    st = model.last_pref_stats.cpu()
    assert st.shape == (8,) and bool(torch.isfinite(st).all()) and float(st[7]) >= 1
    if caplog is not None:
        assert any("preference step" in r.getMessage() and "margin_mean" in r.getMessage() for r in caplog.records)
    runner, model, _, _ = _pipeline(be, tmp, "ipo", ("--train_item_loss", "1", "--train_preference", "ipo", "--pref_ref", "none", "--pref_negatives_mode",
                                                        "sample", "--pref_depth", "0", "--pref_length_normalize", "1", "--epochs", "1"))
    assert runner._pref == dict(num_negatives=4, preference="ipo", pref_depth=None, pref_beta=0.1, pref_sft_coef=0.0, pref_length_normalize=True,
                                ref_model=None, negatives="sample")
    for flags, match in ((("--train_preference", "pl"), "train_item_loss 1"),
                         (PREF_FLAGS + ("--train_policy_samples", "4"), "train_policy_samples"),
                         (PREF_FLAGS + ("--item_loss_top_k", "2"), "top_k / top_p"),
                         (PREF_FLAGS + ("--item_loss_top_p", "0.9"), "top_k / top_p"),
                         (PREF_FLAGS + ("--item_loss_entropy_coef", "0.1"), "item_loss_entropy_coef"),
                         (PREF_FLAGS[:4] + ("--pref_negatives", "0"), "pref_negatives"),
                         (PREF_FLAGS[:4] + ("--pref_beta", "0"), "pref_beta"),
                         (PREF_FLAGS[:4] + ("--pref_beta", "nan"), "pref_beta"),
                         (PREF_FLAGS[:4] + ("--pref_depth", "-1"), "pref_depth"),
                         (PREF_FLAGS[:4] + ("--pref_sft_coef", "inf"), "pref_sft_coef")):
        if flags[0] == "--train_preference" or "--train_policy_samples" in flags:          # through the constructor itself
            with pytest.raises(ValueError, match=match):
                _pipeline(be, tmp, "bad", flags)
            continue
        # the constructor's own check (`DistributedRunner.__init__` calls `_pref_flags`) on the parsed flags, without building a pipeline each
        from openp5_amd.runner import build_arg_parser
        bad = build_arg_parser().parse_args(list(flags))
        keep = runner.args
        runner.args = bad
        try:
            with pytest.raises(ValueError, match=match):
                runner._pref_flags()
        finally:
            runner.args = keep


def runner_resume_case(be, tmp):
    """a run interrupted at a --save_steps checkpoint and resumed ends with the weights of the uninterrupted one (dropout on: the draws, the
    dropout masks, the data order and the reference policy all come back)"""
    flags = PREF_FLAGS[:4] + ("--pref_negatives", "1", "--pref_beta", "0.5", "--epochs", "1")

    def build(name, extra=()):
        runner, model, _, _ = _pipeline(be, tmp, name, flags + tuple(extra), dropout=0.1)
        model.set_dropout_seed(77, 0)
        return runner
    straight = build("straight")
    straight.train()
    n = straight.optimizer.t
    assert n >= 4

    class Stop(Exception):
        pass
    part = build("part", ["--resume", "1", "--save_steps", "2"])
    orig = part.save_checkpoint

    def save_then_die(path, epoch, step, start, extra=None):
        orig(path, epoch, step, start, extra)
        if step == 2:
            raise Stop()
    part.save_checkpoint = save_then_die
    with pytest.raises(Stop):
        part.train()
    rest = build("part", ["--resume", "1", "--save_steps", "1000"])
    rest.train()
    assert rest.optimizer.t == n
    assert torch.equal(rest.model._flat.detach().cpu(), straight.model._flat.detach().cpu())


def runner_off_case(be, tmp):
    """with --train_preference absent (the other pref flags at any value) the calls that reach the model are those without the feature:
    loss_and_backward with the item loss's keywords alone, never preference_step or a sampler -- and the final weights are the same"""
    seen = {}
    for name, flags in (("absent", ("--train_item_loss", "1")),
                        ("unused", ("--train_item_loss", "1", "--pref_negatives", "7", "--pref_beta", "2.0", "--pref_depth", "3", "--pref_sft_coef", "1.0",
                                    "--pref_ref", "none", "--pref_negatives_mode", "sample", "--pref_length_normalize", "1"))):
        runner, model, _, _ = _pipeline(be, tmp, name, flags + ("--epochs", "1"))
        assert runner._pref is None
        calls = []
        real = model.loss_and_backward
        model.loss_and_backward = lambda *a, _r=real, _c=calls, **k: _c.append((len(a), sorted(k))) or _r(*a, **k)
        for fn in ("preference_step", "sequence_logprobs", "sample_items", "sample_slates", "frozen_copy"):
            setattr(model, fn, lambda *a, _n=fn, **k: pytest.fail(f"{_n} called with --train_preference absent"))
        runner.train()
        seen[name] = (calls, model._flat.detach().cpu().clone())
    assert seen["absent"][0] and all(c == (5, ["temperature", "trie"]) for c in seen["absent"][0]), seen["absent"][0][:2]
    assert seen["unused"][0] == seen["absent"][0] and torch.equal(seen["unused"][1], seen["absent"][1])
