"""Cases of the clipped-ratio policy objective (csrc/p5_clip.h, p5_op_clip_objective, p5_train_set_clip_objective, p5_policy_batch_clip,
P5T5Native.loss_and_backward(old_logprobs=, clip_eps=) / policy_collect / policy_update / policy_step(clip_eps=)), shared by
tests/test_clip_emu.py (host emulation) and tests/test_gpu_clip.py (MI355X).

1. the two kernels through the C ABI against `ref_objective`, torch autograd in float64 through torch.minimum / torch.clamp / exp: loss, every
   seed, the eight statistics; clipped and w == 0 seeds are exact zeros; twice, the same bits.
2. rho == 1 (old = -NLL of the same weights): every gradient carries the bits of the plain weighted step, on every backward route.
3. everything clipped: every gradient an exact zero; with a gold slot the SFT-only step's bits.
4. meaning: loss and gradients against the objective restated on the oracle's item NLL under autograd.
5. composition: policy_step(clip_eps) == policy_collect + policy_update, policy_batch's bits, the gather, old_logprobs="forward".
6. it does what it is for: several updates per rollout raise the gold log-probability, and the clip engages behind the first update.
7. refusals name their cause and precede every launch.
8. the runner's flags: batches x E optimizer steps, resume, defaults = the parent's calls."""
import math

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases
from tests import multi_target_cases as mt
from tests import policy_cases as pc
from tests import trie_loss_cases as tl
from tests.cases import sync

RATIOS = {"token": 0, "sequence": 1}
LOG2 = math.log(2.0)
FLT_MAX = float(np.finfo(np.float32).max)
# log-ratios of the random units: exp() of every one of them -- and, sequence mode, of their mean, which is the target's one value there -- stays
# clear of every threshold a case uses (0.8, 1, 1.2, 1.28), so no unit's side of the clip hangs on an fp32 rounding
DELTAS = (-0.5, -0.3, -0.1, -0.05, 0.05, 0.1, 0.15, 0.3, 0.5)


# ---------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------
KERNEL_SHAPES = ((1, 1, 1), (3, 5, 7), (2, 64, 8), (5, 300, 1))       # one unit; odd sizes; G * T = 512; G > 256: the thread stride
KERNEL_EPS = ((0.2, 0.2), (0.2, 0.28), (0.0, 0.0))
N_KINDS = 12


def SUM_TOL(B, G, T):
    """relative to the sum of the terms' magnitudes: a sum of T terms, one of the <= ceil(G / 256) targets of a thread, the two block reductions
    (6 additions each) and B users, with a handful of multiplies, one expf (2 ulp) and one divide per term -- 4 x (that count) x 2^-24, the
    rule of policy_cases.KERNEL_TOL"""
    return 4.0 * (T + (G + 255) // 256 + B + 12 + 8) * 2.0 ** -24


def UNIT_TOL(T):
    """relative, per seed / per rho: the log-ratio (a sum of <= T terms and a divide in sequence mode, one addition in token mode; |x| <= 1 in
    these cases, so its absolute error is rho's relative one), expf (2 ulp), base (one divide) and two multiplies -- twice that count x 2^-24"""
    return 2.0 * (T + 8) * 2.0 ** -24


def kernel_problem(B, G, T, ratio, seed=0):
    """Target tg = b * G + g is of kind tg % 12 (a shape with fewer targets has the first kinds only):
      0  mode 1, w > 0, random ratios          1  mode 1, w < 0, random ratios         2  mode 1, w = 0 (one unit with rho = +inf in fp32)
      3  mode 1, all-masked                    4  mode 1, w > 0, the tail labelled -100 under attention 1
      5  mode 0 (plain weighted NLL); old = NaN when target_mode is passed: never read
      6  rho = 1 exactly (old = -nll bitwise), w > 0 / < 0 alternating
      7  rho = 2, w > 0 (clipped)   8  rho = 2, w < 0 (active)   9  rho = 0.5, w < 0 (clipped)   10  rho = 0.5, w > 0 (active)
      11 w > 0, the first attended unit with -nll - old = 200: rho = +inf in fp32 (finite in float64), clipped
    old is NaN wherever the mask is 0: it is read only where attended."""
    g = np.random.default_rng(1000 * seed + 100 * B + 10 * G + T)
    n = B * G
    nll = g.uniform(0.05, 3.0, (n, T)).astype(np.float32)
    mask = np.zeros((n, T), np.int64)
    labels = g.integers(3, 50, (n, T)).astype(np.int64)
    w = g.uniform(0.3, 2.0, n).astype(np.float32)
    mode = np.ones(n, np.int32)
    old = np.zeros((n, T), np.float32)
    for tg in range(n):
        kind = tg % N_KINDS
        k = int(g.integers(1, T + 1))
        mask[tg, :k] = 1
        d = g.choice(DELTAS, T).astype(np.float32)
        if ratio == "sequence":
            d[:] = d[0]
        if kind in (1, 8, 9) or (kind == 6 and (tg // N_KINDS) % 2):
            w[tg] = -w[tg]
        if kind == 2:
            w[tg] = 0.0
            d[0] = 200.0
        if kind == 3:
            mask[tg] = 0
        if kind == 4:
            mask[tg] = 1
            labels[tg, max(T - 2, 0):] = -100
        if kind == 5:
            mode[tg] = 0
        if kind == 6:
            d[:] = 0.0
        if kind in (7, 8):
            d[:] = LOG2
        if kind in (9, 10):
            d[:] = -LOG2
        if kind == 11:
            d[0] = 200.0
            if ratio == "sequence":
                d[:] = 200.0
        old[tg] = (-nll[tg] - d) if kind not in (6,) else -nll[tg]
    old[mask == 0] = np.nan
    old_mode = old.copy()
    old_mode[mode == 0] = np.nan          # (what a run that passes target_mode gets: a mode-0 target's old is never read)
    return dict(nll=nll, old=old, old_mode=old_mode, mask=mask, labels=labels, w=w, mode=mode)


def ref_objective(pr, B, G, T, ratio, eps, mode_null=False, ent=None, kl=None, entropy_coef=0.0, kl_coef=0.0):
    """float64 restatement under autograd; lo / hi are the fp32 values the kernel forms.  Returns loss, terms, seeds [n, T] (0 at labels -100),
    the statistics, the clipped units' mask [n, T], the sum of the terms' magnitudes and the largest |log rho|."""
    n = B * G
    lo, hi = float(np.float32(1) - np.float32(eps[0])), float(np.float32(1) + np.float32(eps[1]))
    nll = torch.from_numpy(pr["nll"]).double().requires_grad_(True)
    m = torch.from_numpy(pr["mask"] != 0)
    md = m.double()
    old = torch.where(m, torch.from_numpy(pr["old"]).double(), torch.zeros((), dtype=torch.float64))
    w = torch.from_numpy(pr["w"]).double()
    mode1 = torch.ones(n, dtype=torch.bool) if mode_null else torch.from_numpy(pr["mode"] != 0)
    cnt = md.sum(1)
    c = cnt.clamp(min=1)
    if ratio == "token":
        x = -(old + nll)
        rho = torch.exp(x)
        sur = -torch.minimum(rho * w[:, None], torch.clamp(rho, lo, hi) * w[:, None])
        per1 = (sur * md).sum(1) / c
        unit = m & mode1[:, None] & (w != 0)[:, None]
        wu = w[:, None].expand(n, T)
    else:
        x = -((old + nll) * md).sum(1) / c
        rho = torch.exp(x)
        per1 = torch.where(cnt > 0, -torch.minimum(rho * w, torch.clamp(rho, lo, hi) * w), torch.zeros((), dtype=torch.float64))
        unit = mode1 & (w != 0) & (cnt > 0)
        wu = w
    per0 = w * (nll * md).sum(1) / c
    per = torch.where(mode1, per1, per0)
    l0 = per.sum() / n
    loss, terms = l0, None
    if ent is not None:
        rh = ((torch.from_numpy(ent).double() * md).sum(1) / c).sum() / n
        rk = ((torch.from_numpy(kl).double() * md).sum(1) / c).sum() / n if kl is not None else torch.zeros((), dtype=torch.float64)
        loss = (l0 + float(np.float32(kl_coef)) * rk) - float(np.float32(entropy_coef)) * rh
        terms = np.array([float(l0.detach()), float(rh), float(rk)])
    l0.backward()
    seeds = nll.grad.numpy() * (pr["labels"] != -100)
    rho_d, x_d = rho.detach(), x.detach()
    at_hi, at_lo = unit & (wu > 0) & (rho_d > hi), unit & (wu < 0) & (rho_d < lo)
    ru, xu = rho_d[unit], x_d[unit]
    nu = int(unit.sum())
    if nu:
        reg = (ru > 0) & (ru <= FLT_MAX)
        stats = [nu, float((at_hi | at_lo).sum()) / nu, float(at_hi.sum()) / nu, float(at_lo.sum()) / nu,
                 float(ru[reg].mean()) if bool(reg.any()) else 1.0, float(ru.max()) if float(ru.max()) <= FLT_MAX else math.inf, float(ru.min()),
                 float(((ru[reg] - 1) - xu[reg]).mean()) if bool(reg.any()) else 0.0]
        top = max(1.0, float(ru[reg].max()) if bool(reg.any()) else 1.0, float(xu[reg].abs().max()) if bool(reg.any()) else 0.0)
        # the reference alone: no unit's side of the clip hangs on a rounding (units at rho == 1 exactly are on the active side by definition)
        away = ru[(xu != 0)]
        for thr in (lo, hi):
            assert not bool(((away - thr).abs() < 1e-3).any()), (ratio, eps, thr)
    else:
        stats, top = [0, 0, 0, 0, 1, 1, 1, 0], 1.0
    clipped = (at_hi | at_lo) if ratio == "token" else ((at_hi | at_lo)[:, None] & m)
    return dict(loss=float(loss.detach()), terms=terms, seeds=seeds, stats=np.array(stats, np.float64), clipped=clipped.numpy(),
                mag=float(per.detach().abs().sum()) / n, top=top, base=(md / c[:, None] / n).numpy())


def run_clip_op(be, pr, B, G, T, ratio, eps, mode_null=False, ent=None, kl=None, entropy_coef=0.0, kl_coef=0.0, tw_null=False):
    from openp5_amd.model import _ptr
    dv = be.device
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dv)       # noqa: E731
    rows = B * G * T
    f = lambda k: torch.full((k,), float("nan"), dtype=torch.float32, device=dv)      # noqa: E731
    loss, terms, seed, part, stats = f(1), f(3), f((3 if ent is not None else 1) * rows), f(16 * B), f(8)
    d = [t(pr[k]) for k in ("nll", "old" if mode_null else "old_mode", "mask", "labels")]
    d_w, d_mode, d_ent, d_kl = None if tw_null else t(pr["w"]), None if mode_null else t(pr["mode"]), t(ent), t(kl)
    rc = be.lib.p5_op_clip_objective(_ptr(loss), _ptr(terms) if ent is not None else None, _ptr(seed), _ptr(part), _ptr(stats), _ptr(d[0]), _ptr(d[1]),
                                     _ptr(d[2]), _ptr(d[3]), _ptr(d_w), _ptr(d_mode), _ptr(d_ent), _ptr(d_kl), entropy_coef, kl_coef, eps[0], eps[1],
                                     RATIOS[ratio], B, G, T, be.stream_ptr())
    be.check(rc, "p5_op_clip_objective")
    sync(be)
    return dict(loss=loss.cpu().numpy(), terms=terms.cpu().numpy(), seed=seed.cpu().numpy(), stats=stats.cpu().numpy())


def kernel_case(be, B, G, T, ratio, eps):
    pr = kernel_problem(B, G, T, ratio)
    n, rows = B * G, B * G * T
    g = np.random.default_rng(7)
    ent, kl = g.uniform(0.0, 2.0, (n, T)).astype(np.float32), g.uniform(0.0, 1.0, (n, T)).astype(np.float32)
    for mode_null, reg in ((False, False), (True, False), (False, True)):
        tag = f"B={B} G={G} T={T} {ratio} eps={eps} mode_null={mode_null} reg={reg}"
        kw = dict(ent=ent, kl=kl, entropy_coef=0.05, kl_coef=0.2) if reg else {}
        ref = ref_objective(pr, B, G, T, ratio, eps, mode_null, **kw)
        runs = [run_clip_op(be, pr, B, G, T, ratio, eps, mode_null, **kw) for _ in range(2)]
        for k, v in runs[0].items():
            assert v.tobytes() == runs[1][k].tobytes(), f"{tag}: two runs differ in {k}"
        got = runs[0]
        stol, utol = SUM_TOL(B, G, T), UNIT_TOL(T)
        extra = 0.05 * abs(ref["terms"][1]) + 0.2 * abs(ref["terms"][2]) if reg else 0.0
        print(f"[clip kernel {tag}] loss {got['loss'][0]:.7f} ref {ref['loss']:.7f} (sum of magnitudes {ref['mag'] + extra:.3f}), stats {got['stats'].tolist()}")
        assert math.isfinite(got["loss"][0]) and abs(got["loss"][0] - ref["loss"]) <= stol * (ref["mag"] + extra), (tag, got["loss"], ref["loss"])
        seeds = got["seed"][:rows].reshape(n, T).astype(np.float64)
        assert np.isfinite(got["seed"]).all(), tag
        assert (np.abs(seeds - ref["seeds"]) <= utol * np.abs(ref["seeds"])).all(), (tag, float(np.abs(seeds - ref["seeds"]).max()))
        assert ref["clipped"].any() or n < 8, tag
        assert (seeds[ref["clipped"]] == 0).all(), f"{tag}: a clipped unit's seed is not an exact zero"
        zero_w = (pr["w"] == 0) & ((pr["mode"] != 0) | mode_null)
        assert (seeds[zero_w] == 0).all() and (seeds[pr["mask"] == 0] == 0).all() and (seeds[pr["labels"] == -100] == 0).all(), tag
        if reg:
            assert (np.abs(got["terms"] - ref["terms"]) <= stol * np.maximum(np.abs(ref["terms"]), ref["mag"])).all(), (tag, got["terms"], ref["terms"])
            gh, gk = got["seed"][rows:2 * rows].reshape(n, T), got["seed"][2 * rows:].reshape(n, T)
            for a, coef in ((gh, -0.05), (gk, 0.2)):
                want = float(np.float32(coef)) * ref["base"]
                assert (np.abs(a - want) <= 4 * 2.0 ** -24 * np.abs(want)).all(), tag
        st, rs = got["stats"].astype(np.float64), ref["stats"]
        assert st[0] == rs[0], (tag, st, rs)
        assert (np.abs(st[1:4] - rs[1:4]) <= 2.0 ** -22).all(), (tag, st, rs)
        assert abs(st[4] - rs[4]) <= stol * ref["top"] and abs(st[7] - rs[7]) <= stol * ref["top"], (tag, st, rs)
        assert (st[5] == rs[5] if math.isinf(rs[5]) else abs(st[5] - rs[5]) <= utol * rs[5]) and abs(st[6] - rs[6]) <= utol * rs[6], (tag, st, rs)
        assert np.isfinite(np.delete(st, 5)).all(), (tag, st)
        if n >= N_KINDS and not reg:
            assert math.isinf(rs[5]) and rs[2] > 0 and rs[3] > 0, (tag, rs)
    # no unit at all: the documented constants
    pr0 = dict(pr, w=np.zeros_like(pr["w"]))
    got = run_clip_op(be, pr0, B, G, T, ratio, eps, mode_null=True)
    assert got["stats"].tolist() == [0, 0, 0, 0, 1, 1, 1, 0] and float(got["loss"][0]) == 0 and (got["seed"] == 0).all(), got["stats"]
    if eps == (0.0, 0.0):
        # rho == 1 exactly under eps = 0 is ACTIVE for both signs: the seeds of kind-6 targets are base * w, bit for bit
        for tg in range(6, n, N_KINDS):
            c = max(int(pr["mask"][tg].sum()), 1)
            bw = np.float32(np.float32(1) / np.float32(n)) / np.float32(c) * pr["w"][tg]
            want = np.where((pr["mask"][tg] != 0) & (pr["labels"][tg] != -100), bw, np.float32(0))
            assert np.array_equal(runs[0]["seed"][:rows].reshape(n, T)[tg], want.astype(np.float32)), (tg, want)


# ---------------------------------------------------------------------------------------------------------
# 2. rho == 1 is the plain step, bit for bit
# ---------------------------------------------------------------------------------------------------------
ROUTES = ("ce", "ce_free", "item_dense", "item_trie", "reg")


def _route_batch(ocfg, items, route, G, B=3, L=12, T=6):
    """(ids, ww, mask, labels, out_attn, weights or None, trie or None) of a route; grouped batches carry a weight 0, a negative one, an
    all-masked target (plain routes) or one that leaves the trie (item routes)"""
    if route in ("ce", "ce_free"):
        if G is None:
            ids, ww, mask, labels, out_attn = cases.synth_batch(ocfg, B, L, T, 3)
        else:
            ids, ww, mask, labels, out_attn = mt.grouped_batch(ocfg, B, L, T, G)
        ct = None
    else:
        ct = rank_cases.compiled(items)
        if G is None:
            ids, ww, mask, labels, out_attn, _ = tl.item_batch(ocfg, items, B, L, T, tl.MODEL_SEED, stray=False)
        else:
            ids, ww, mask, labels, out_attn, _ = mt.item_batch(ocfg, items, B, L, T, G)
    return ids, ww, mask, labels, out_attn, (None if G is None else mt._weights(B, G)), ct


def rho1_case(be, ocfg, items, route, dtype, G, eps=0.2, ratio="token", dropout=0.0):
    """old_logprobs = -forward(...)["loss"] of the same weights: every .grad equals the plain weighted step's, bit for bit, and the loss is
    -sum w [mode 1, cnt > 0] / (B G) plus the plain terms.  Route "ce_free" (bf16): the logit-free head, with dropout on so that the step is a
    training step and the plain call's loss kernel writes the seeds itself (the ce_g_ready route the objective must not be short-circuited
    by); the dropout seed is reset in front of every call, so the three forwards draw the same masks."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn, w, ct = _route_batch(ocfg, items, route, G)
    B, T = labels.shape[0], labels.shape[-1]
    n = B * (G or 1)
    mode = None
    if G is not None:
        mode = torch.ones(B, G, dtype=torch.int32)
        mode[:, 0] = 0                # (a gold slot beside the draws)
    kw = {}
    if ct is not None:
        kw = dict(trie=ct, temperature=0.8, item_head="trie" if route == "item_trie" else "dense")

    def fresh():
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        tl._train_mode(m, dropout, 77)
        return m
    if route == "ce_free":
        be.check(be.lib.p5_set_option(b"gemm_wide_min_tiles", 1), "opt")
    try:
        m = fresh()
        regkw = {}
        if route == "reg":
            ref = m.frozen_copy()
            with torch.no_grad():
                ref._flat.mul_(1.01)
            ref.mark_params_updated()
            regkw = dict(entropy_coef=0.05, kl_coef=0.2, ref_logits=ref.item_logits(ids, ww, mask, labels, ct, temperature=0.8))
        with torch.no_grad():
            nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, **kw)["loss"]
        old = (-nll).view(labels.shape)
        p = fresh()
        loss_p = p.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, **kw, **regkw)
        assert p.last_clip_stats is None
        terms_p = None if p.last_item_loss_terms is None else p.last_item_loss_terms.cpu().double()
        q = fresh()
        loss_c = q.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, old_logprobs=old, target_mode=mode, clip_eps=eps, ratio=ratio,
                                     **kw, **regkw)
        sync(be)
        stats = q.last_clip_stats.cpu()
    finally:
        be.lib.p5_set_option(b"gemm_wide_min_tiles", 160)
    gp, gc = p._grads.detach().cpu(), q._grads.detach().cpu()
    assert float(gp.abs().max()) > 0
    assert torch.equal(gp, gc), (route, dtype, G, float((gp - gc).abs().max()))
    for (name, a), (_, b_) in zip(p.named_parameters(), q.named_parameters()):
        assert torch.equal(a.grad.cpu(), b_.grad.cpu()), name
    assert float(stats[4]) == 1 and float(stats[5]) == 1 and float(stats[6]) == 1 and float(stats[1]) == 0 and float(stats[7]) == 0, stats
    # the loss: -w per clipped target with an attended token, the plain term of the others, the regularisers' terms as the plain step has them
    md = (out_attn != 0).double().view(n, T)
    cnt = md.sum(1)
    wd = torch.ones(n, dtype=torch.float64) if w is None else w.double().view(n)
    m1 = torch.ones(n, dtype=torch.bool) if mode is None else (mode.view(n) != 0)
    plain = wd * (nll.detach().cpu().double().view(n, T) * md).sum(1) / cnt.clamp(min=1)
    want = (torch.where(m1, torch.where(cnt > 0, -wd, torch.zeros((), dtype=torch.float64)), plain)).sum() / n
    mag = (torch.where(m1, wd.abs(), plain.abs())).sum() / n
    if terms_p is not None:
        want = want + (float(loss_p) - float(terms_p[0]))
    tol = SUM_TOL(B, G or 1, T)        # (either dtype: the NLL is fp32, and the two forwards give the same bits)
    assert abs(float(loss_c) - float(want)) <= tol * max(1.0, float(mag)) + (abs(float(loss_p)) * 2.0 ** -22 if terms_p is not None else 0), \
        (float(loss_c), float(want))


# ---------------------------------------------------------------------------------------------------------
# 3. everything clipped
# ---------------------------------------------------------------------------------------------------------
def all_clipped_case(be, ocfg, items, dtype="fp32", G=3, ratio="token"):
    """old = -nll - log 2 (rho = 2) and every w > 0 under eps 0.2: nothing moves -- every gradient an exact zero, share clipped 1.  With a
    gold slot (mode 0) the gradients are the SFT-only step's (the draws' weights 0) bits."""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn, _, ct = _route_batch(ocfg, items, "item_dense", G)
    B = labels.shape[0]
    kw = dict(trie=ct, temperature=0.8)
    w = torch.full((B, G), 1.3)
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    with torch.no_grad():
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, **kw)["loss"]
    old = (-nll - LOG2).view(labels.shape)
    loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, old_logprobs=old, clip_eps=0.2, ratio=ratio, **kw)
    sync(be)
    assert math.isfinite(float(loss))
    assert bool((m._grads.detach().cpu() == 0).all()), "a clipped batch moved a gradient"
    st = m.last_clip_stats.cpu()
    assert float(st[1]) == 1 and float(st[2]) == 1 and float(st[3]) == 0 and float(st[0]) > 0, st
    mode = torch.ones(B, G, dtype=torch.int32)
    mode[:, 0] = 0
    m.zero_grad()
    m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, old_logprobs=old, target_mode=mode, clip_eps=0.2, ratio=ratio, **kw)
    sync(be)
    g_clip = m._grads.detach().cpu().clone()
    s = cases.build_model(be, ocfg, params, dtype)
    s.eval()
    w_sft = w.clone()
    w_sft[:, 1:] = 0
    s.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w_sft, **kw)
    sync(be)
    g_sft = s._grads.detach().cpu()
    assert float(g_sft.abs().max()) > 0 and torch.equal(g_clip, g_sft), float((g_clip - g_sft).abs().max())


# ---------------------------------------------------------------------------------------------------------
# 4. meaning
# ---------------------------------------------------------------------------------------------------------
def meaning_case(be, ocfg, items, ratio, B=3, L=12, T=6, G=3, eps=(0.2, 0.28), tau=0.8):
    """fp32: loss and every gradient of loss_and_backward(old_logprobs=, clip_eps=) against the objective restated in float64 on the oracle's
    item NLL (tl.oracle_item_nll of the replicated batch) under autograd -- the tolerances of policy_cases.meaning_case (NLL 2e-5, gradients
    2e-4 with the 1 % floor).  old = -(the model's NLL) - delta: mixed ratios, some clipped on either side."""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn, w, ct = _route_batch(ocfg, items, "item_dense", G, B, L, T)
    mode = torch.ones(B, G, dtype=torch.int32)
    mode[:, 0] = 0
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    with torch.no_grad():
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=tau)["loss"].cpu()
    # log-ratios by design, from the weights' signs: every third unit clipped (on the side its weight's sign decides), every third active away
    # from 1 on the other side, the rest active near 1 -- per token, or per target for the sequence ratio
    sg = torch.sign(w).double().numpy()[:, :, None]
    i = (np.arange(B * G * T).reshape(B, G, T) if ratio == "token" else np.arange(B * G).reshape(B, G, 1) + np.arange(B).reshape(B, 1, 1) + np.zeros((1, 1, T), np.int64))
    d = np.where(i % 3 == 0, 0.5 * sg, np.where(i % 3 == 1, -0.3 * sg, 0.1))
    old = (-nll.view(B, G, T).double() - torch.from_numpy(d)).float()
    loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, trie=ct, temperature=tau, target_weights=w, old_logprobs=old, target_mode=mode, clip_eps=eps,
                               ratio=ratio)
    sync(be)
    st = m.last_clip_stats.cpu()
    assert 0 < float(st[1]) < 1 and float(st[2]) > 0 and float(st[3]) > 0, f"the case must clip some units on either side, not all: {st}"
    Pq = mt._oracle_params(params, "bf16")          # (float64)
    nll_o, _, _ = tl.oracle_item_nll(Pq, ocfg, mt.rep(ids, G), mt.rep(ww, G), mt.rep(mask, G), labels.view(B * G, T), ct, tau, None)
    lo, hi = float(np.float32(1) - np.float32(eps[0])), float(np.float32(1) + np.float32(eps[1]))
    md = (out_attn != 0).double()
    c = md.sum(2).clamp(min=1)
    wd = w.double()
    x = -(old.double() + nll_o.view(B, G, T))
    if ratio == "token":
        rho = torch.exp(x)
        per1 = (-torch.minimum(rho * wd[..., None], torch.clamp(rho, lo, hi) * wd[..., None]) * md).sum(2) / c
    else:
        rho = torch.exp((x * md).sum(2) / c)
        per1 = torch.where(md.sum(2) > 0, -torch.minimum(rho * wd, torch.clamp(rho, lo, hi) * wd), torch.zeros((), dtype=torch.float64))
    per0 = wd * (nll_o.view(B, G, T) * md).sum(2) / c
    loss_o = torch.where(mode != 0, per1, per0).sum() / (B * G)
    loss_o.backward()
    lo_ = float(loss_o.detach())
    _, worst = mt._fp32_errors(m, Pq, nll_o, nll_o)
    print(f"[clip meaning {ratio}] loss {float(loss):.6f} oracle {lo_:.6f}, worst gradient {worst[0]:.2e} ({worst[1]}), stats {st.tolist()}")
    assert abs(float(loss) - lo_) <= mt.NLL_TOL * max(1.0, abs(lo_)), (float(loss), lo_)
    assert worst[0] <= mt.GRAD_TOL, worst


# ---------------------------------------------------------------------------------------------------------
# 5. composition
# ---------------------------------------------------------------------------------------------------------
def composition_case(be, ocfg, items, dtype="fp32", item_head="dense", reg=False, ratio="token", B=3, L=12, S=4, seed=11, old_logprobs="sampler", **kw):
    """policy_step(clip_eps=, seed=s) against policy_collect + policy_update on a fresh model with the same weights: loss, gradient arena and
    statistics bit for bit"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    common = dict(temperature=0.8, item_head=item_head)
    res = []
    for whole in (True, False):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        regkw, ref = {}, None
        if reg:
            ref = m.frozen_copy()
            with torch.no_grad():
                ref._flat.mul_(1.01)
            ref.mark_params_updated()
            regkw = dict(entropy_coef=0.05, kl_coef=0.2)
        if whole:
            loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, S, seed=seed, reward_fn=pc.index_reward, clip_eps=(0.2, 0.28), ratio=ratio,
                                 old_logprobs=old_logprobs, ref_model=ref, **regkw, **common, **kw)
        else:
            ro = m.policy_collect(ids, ww, mask, labels, out_attn, ct, S, seed=seed, reward_fn=pc.index_reward, old_logprobs=old_logprobs, ref_model=ref,
                                  kl_coef=regkw.get("kl_coef", 0.0), **common, **kw)
            assert ("ref_logits" in ro) == reg and ro["old_logprobs"].shape == ro["labels"].shape and ro["target_mode"].dtype == torch.int32
            loss = m.policy_update(ids, ww, mask, ro, ct, (0.2, 0.28), ratio=ratio, **regkw, **common)
        sync(be)
        res.append((loss.detach().cpu().clone(), m._grads.detach().cpu().clone(), m.last_clip_stats.cpu().clone()))
    (l0, g0, s0), (l1, g1, s1) = res
    assert math.isfinite(float(l0)) and float(g0.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(s0, s1), (float(l0), float(l1), float((g0 - g1).abs().max()))
    return s0


def batch_clip_case(be, ocfg, items, B=3, L=12, S=5, seed=11, with_gold=True):
    """policy_batch(token_logprobs=) returns policy_batch's bits, old_logprobs is the padded gather of the sampler's token_logprobs (exactly),
    target_mode is gold 0 / draws 1"""
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    drawn = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=0.8, seed=seed)
    kw = dict(rewards=pc.index_reward(drawn), baseline="grpo", sft_coef=1.0 if with_gold else 0.0)
    a = m.policy_batch(drawn["sequences"], labels, out_attn, S, **kw)
    b_ = m.policy_batch(drawn["sequences"], labels, out_attn, S, token_logprobs=drawn["token_logprobs"], **kw)
    sync(be)
    for k, v in a.items():
        assert torch.equal(v.cpu(), b_[k].cpu()), k
    seq, tlp = drawn["sequences"].cpu().numpy(), drawn["token_logprobs"].cpu().numpy()
    G, To = b_["labels"].shape[1:]
    want = np.zeros((B, G, To), np.float32)
    for r in range(B * S):
        k = pc.draw_length([int(t) for t in seq[r, 1:]])
        want[r // S, G - S + r % S, :k] = tlp[r, :k]
    got = b_["old_logprobs"].cpu().numpy()
    assert got.tobytes() == want.tobytes() or np.array_equal(got, want), float(np.abs(got - want).max())
    assert float(np.abs(want).max()) > 0
    mode = np.ones((B, G), np.int32)
    if with_gold:
        mode[:, 0] = 0
    assert np.array_equal(b_["target_mode"].cpu().numpy(), mode)


def forward_old_case(be, ocfg, items, dtype="fp32", item_head="dense"):
    """old_logprobs="forward", dropout off: the first update's ratio is exactly 1 -- mean rho == max rho == min rho == 1, nothing clipped"""
    for ratio in ("token", "sequence"):
        st = composition_case(be, ocfg, items, dtype=dtype, item_head=item_head, ratio=ratio, old_logprobs="forward")
        assert float(st[0]) > 0 and float(st[4]) == 1 and float(st[5]) == 1 and float(st[6]) == 1 and float(st[1]) == 0 and float(st[7]) == 0, (ratio, st)


# ---------------------------------------------------------------------------------------------------------
# 6. it does what it is for
# ---------------------------------------------------------------------------------------------------------
def learns_case(be, ocfg, collects=6, E=4, B=4, S=8, L=10, lr=3e-5, eps=0.2):
    """the setting of policy_cases.learns_case (REINFORCE alone: sft_coef 0, loo, the hit reward, 8 items) with E updates per rollout under
    old_logprobs="forward".  Returns (gold log-probability before, after, share clipped per (collect, update))."""
    from openp5_amd.optim import FusedAdamW
    items = cases.make_items(8, 5, hi=60)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    opt = FusedAdamW(m, lr=lr, weight_decay=0.0, max_grad_norm=1.0)
    before = pc._gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    clipped = []
    for c in range(collects):
        ro = m.policy_collect(ids, ww, mask, labels, out_attn, ct, S, baseline="loo", policy_coef=1.0, sft_coef=0.0, seed=1000 + c, old_logprobs="forward")
        row = []
        for _ in range(E):
            m.policy_update(ids, ww, mask, ro, ct, eps)
            row.append(m.last_clip_stats.clone())
            opt.step()
            m.zero_grad()
        clipped.append(row)
    sync(be)
    after = pc._gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    shares = [[float(s.cpu()[1]) for s in row] for row in clipped]
    print(f"[clip learns] gold log-probability {before:.4f} -> {after:.4f} after {collects} rollouts x {E} updates; share clipped {shares}")
    return before, after, shares


# ---------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------
def abi_errors_case(be, ocfg, items):
    from openp5_amd.model import _ptr
    lib, dv = be.lib, be.device
    B, G, T = 2, 2, 3
    buf = torch.zeros(256, dtype=torch.float32, device=dv)
    f, part_, stats_, loss_, nll_, old_ = buf[0:64], buf[64:128], buf[128:136], buf[136:137], buf[144:176], buf[176:208]
    i64 = torch.ones(B * G * T, dtype=torch.int64, device=dv)

    def op(eps=(0.2, 0.2), ratio=0, old=old_, seed=f, B_=B):
        return lib.p5_op_clip_objective(_ptr(loss_), None, _ptr(seed), _ptr(part_), _ptr(stats_), _ptr(nll_), _ptr(old), _ptr(i64), _ptr(i64), None, None, None,
                                        None, 0.0, 0.0, eps[0], eps[1], ratio, B_, G, T, be.stream_ptr())
    assert op() == 0
    sync(be)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    eng = m._engine

    def arm(eps=(0.2, 0.2), ratio=0, old=old_, seed=f, part=part_, stats=stats_):
        return lib.p5_train_set_clip_objective(eng, _ptr(old), None, eps[0], eps[1], ratio, _ptr(seed), _ptr(part), _ptr(stats))
    for call in (op, arm):
        for kw, msg in ((dict(eps=(-0.1, 0.2)), b"eps"), (dict(eps=(0.2, float("nan"))), b"eps"), (dict(eps=(float("inf"), 0.2)), b"eps"),
                        (dict(ratio=2), b"ratio mode"), (dict(ratio=-1), b"ratio mode"), (dict(old=None), b"null pointer"), (dict(seed=None), b"null pointer")):
            assert call(**kw) != 0, kw
            assert msg in lib.p5_last_error(), (kw, lib.p5_last_error())
    assert arm(stats=None) != 0 and b"null pointer" in lib.p5_last_error()
    assert arm(part=None) != 0 and b"null pointer" in lib.p5_last_error()
    assert op(B_=0) != 0 and b"shapes" in lib.p5_last_error()
    # armed behind the truncated item loss
    ct = rank_cases.compiled(items)
    q = m._item_loss_setup(ct, 1.0, None, B, top_k=2)
    m._arm_item_loss(q, B, T)
    assert arm() != 0 and b"truncated item loss" in lib.p5_last_error()
    assert lib.p5_train_set_item_loss(eng, None, None, None, 0, None, 0, 1.0, None) != 0          # (a refused call disarms the item loss armed above)
    # p5_forward while armed names the objective -- and disarms it: the next plain forward runs
    ids, ww, mask, labels, out_attn = cases.synth_batch(ocfg, B, 8, T, 3)
    assert arm() == 0
    with pytest.raises(Exception, match="p5_train_set_clip_objective"):
        with torch.no_grad():
            m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)
    with torch.no_grad():
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
    sync(be)
    assert bool(torch.isfinite(nll).all())


def model_errors_case(be, ocfg, items):
    """every refusal is a ValueError raised before anything is sampled or launched"""
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    ct = rank_cases.compiled(items)
    calls = []
    for name in ("_workspace", "_lane_workspace", "sample_items", "_sample", "_arm_item_loss", "_engine_forward", "policy_batch"):
        real = getattr(m, name)
        setattr(m, name, (lambda real_, name_: lambda *a, **k: calls.append(name_) or real_(*a, **k))(real, name))
    B, G, T, S = 2, 3, 6, 3
    ids, ww, mask, labels, out_attn, w, _ = _route_batch(ocfg, items, "item_dense", G, B, 8, T)
    old = torch.zeros(B, G, T)

    def lb(match, labels_=labels, attn_=out_attn, w_=w, **kw):
        with pytest.raises(ValueError, match=match):
            m.loss_and_backward(ids, ww, mask, labels_, attn_, trie=kw.pop("trie", ct), target_weights=w_, **kw)
    lb("clip_eps", old_logprobs=old)
    lb("old_logprobs", clip_eps=0.2)
    lb("old_logprobs", target_mode=torch.ones(B, G, dtype=torch.int32))
    lb("top_k / top_p", old_logprobs=old, clip_eps=0.2, top_k=2)
    lb("top_k / top_p", old_logprobs=old, clip_eps=0.2, top_p=0.9)
    lb("ratio", old_logprobs=old, clip_eps=0.2, ratio="item")
    lb("clip_eps", old_logprobs=old, clip_eps=-0.1)
    lb("clip_eps", old_logprobs=old, clip_eps=(0.2, float("nan")))
    lb("clip_eps", old_logprobs=old, clip_eps=(0.1, 0.2, 0.3))
    lb("clip_eps", old_logprobs=old, clip_eps="wide")
    lb("old_logprobs.*shaped like labels", old_logprobs=old[:, :, :-1], clip_eps=0.2)
    lb("old_logprobs.*shaped like labels", old_logprobs=old.view(B * G, T), clip_eps=0.2)
    lb("target_mode", old_logprobs=old, clip_eps=0.2, target_mode=torch.ones(B, G + 1, dtype=torch.int32))
    lb("old_logprobs.*shaped like labels", labels_=labels[:, 0], attn_=out_attn[:, 0], w_=None, old_logprobs=old, clip_eps=0.2)
    gl, ga = labels[:, 0], out_attn[:, 0]

    def pol(fn, match, **kw):
        with pytest.raises(ValueError, match=match):
            fn(ids, ww, mask, gl, ga, kw.pop("trie", ct), kw.pop("S_", S), **kw)
    for fn, extra in ((m.policy_collect, {}), (m.policy_step, dict(clip_eps=0.2))):
        pol(fn, "top_k / top_p", top_k=2, **extra)
        pol(fn, "ratio", ratio="item", **extra)
        pol(fn, "old_logprobs", old_logprobs="replay", **extra)
        pol(fn, "ref_model", kl_coef=0.1, **extra)
        pol(fn, "trie", trie=None, **extra)
        pol(fn, "num_samples", S_=0, **extra)
        pol(fn, r"G \* T <= 512", S_=102, **extra)
    pol(m.policy_collect, "clip_eps", clip_eps=-1.0)
    pol(m.policy_step, "clip_eps", clip_eps=(0.2, -1.0))
    with pytest.raises(ValueError, match="ref_logits"):
        m.policy_update(ids, ww, mask, dict(labels=labels, output_attention=out_attn, target_weights=w, old_logprobs=old,
                                            target_mode=torch.ones(B, G, dtype=torch.int32)), ct, 0.2, kl_coef=0.1)
    with pytest.raises(ValueError, match="clip_eps"):
        m.policy_update(ids, ww, mask, {}, ct, None)
    assert not calls, f"a refused call reached the sampler or the engine: {calls}"
    assert m.last_clip_stats is None


# ---------------------------------------------------------------------------------------------------------
# 8. the runner
# ---------------------------------------------------------------------------------------------------------
CLIP_FLAGS = pc.POLICY_FLAGS + ("--policy_clip_eps", "0.2", "--policy_clip_eps_high", "0.28", "--policy_epochs", "2", "--policy_old_logprobs", "forward")


def runner_case(be, tmp, caplog=None):
    """--policy_clip_eps / --policy_epochs 2 train: one collect per batch, E updates and optimizer steps behind it, the schedule over
    batches x E steps, the statistics logged; the flags are checked at construction"""
    import logging
    runner, model, _, _ = pc._pipeline(be, tmp, "on", CLIP_FLAGS + ("--epochs", "1", "--logging_step", "2", "--policy_ratio", "sequence"))
    seen = {"collect": [], "update": []}
    real_c, real_u = model.policy_collect, model.policy_update
    model.policy_collect = lambda *a, **k: seen["collect"].append(k) or real_c(*a, **k)
    model.policy_update = lambda *a, **k: seen["update"].append(k) or real_u(*a, **k)
    model.policy_step = lambda *a, **k: pytest.fail("policy_step called with --policy_epochs 2")
    if caplog is not None:
        caplog.set_level(logging.INFO)
    n_batches = len(runner.train_loader)
    assert runner.optimizer.total_steps == 2 * n_batches
    losses = runner.train()
    assert len(losses) == 1 and math.isfinite(losses[0])
    assert len(seen["collect"]) == n_batches and len(seen["update"]) == 2 * n_batches and runner.optimizer.t == 2 * n_batches
    assert all(k["num_samples"] == 4 and k["old_logprobs"] == "forward" and k["clip_eps"] == (0.2, 0.28) and k["ratio"] == "sequence" for k in seen["collect"])
    assert len({k["seed"] for k in seen["collect"]}) == n_batches, "every batch draws with its own seed"
    st = model.last_clip_stats.cpu()
    assert st.shape == (8,) and bool(torch.isfinite(st).all()) and float(st[0]) > 0
    if caplog is not None:
        assert any("policy clip step" in r.getMessage() and "ratio_mean" in r.getMessage() for r in caplog.records)
    for flags, match in ((pc.POLICY_FLAGS + ("--policy_epochs", "2"), "policy_clip_eps > 0"),
                         (CLIP_FLAGS + ("--gradient_accumulation_steps", "2"), "gradient_accumulation_steps"),
                         (pc.POLICY_FLAGS + ("--policy_clip_eps", "-0.1"), "policy_clip_eps"),
                         (pc.POLICY_FLAGS + ("--policy_clip_eps", "0.2", "--policy_epochs", "0"), "policy_epochs"),
                         (("--train_item_loss", "1", "--policy_clip_eps", "0.2"), "train_policy_samples"),
                         (CLIP_FLAGS + ("--item_loss_top_k", "2"), "top_k / top_p")):
        with pytest.raises(ValueError, match=match):
            pc._pipeline(be, tmp, "bad", flags)


def runner_accum_case(be, tmp):
    """one update per batch under gradient accumulation: policy_step(clip_eps=...) inside the accumulating step"""
    runner, model, _, _ = pc._pipeline(be, tmp, "accum", pc.POLICY_FLAGS + ("--policy_clip_eps", "0.2", "--gradient_accumulation_steps", "2", "--epochs", "1"))
    seen = []
    real = model.policy_step
    model.policy_step = lambda *a, **k: seen.append(k) or real(*a, **k)
    runner.train()
    n_batches = len(runner.train_loader)
    assert len(seen) == n_batches and runner.optimizer.t == math.ceil(n_batches / 2)
    assert all(k["clip_eps"] == (0.2, 0.2) and k["ratio"] == "token" and k["old_logprobs"] == "sampler" for k in seen)


def runner_resume_case(be, tmp):
    """a run with E = 2 interrupted at a --save_steps checkpoint (a batch boundary) and resumed ends with the weights of the uninterrupted one"""
    flags = CLIP_FLAGS + ("--epochs", "1")

    def build(name, extra=()):
        runner, model, _, _ = pc._pipeline(be, tmp, name, flags + tuple(extra), dropout=0.1)
        model.set_dropout_seed(77, 0)
        return runner
    straight = build("straight")
    straight.train()
    n = straight.optimizer.t
    assert n >= 8 and n % 2 == 0

    class Stop(Exception):
        pass
    part = build("part", ["--resume", "1", "--save_steps", "4"])
    orig = part.save_checkpoint

    def save_then_die(path, epoch, step, start, extra=None):
        orig(path, epoch, step, start, extra)
        if step == 2:
            raise Stop()
    part.save_checkpoint = save_then_die
    with pytest.raises(Stop):
        part.train()
    assert part.optimizer.t == 4
    rest = build("part", ["--resume", "1", "--save_steps", "1000"])
    rest.train()
    assert rest.optimizer.t == n
    assert torch.equal(rest.model._flat.detach().cpu(), straight.model._flat.detach().cpu())


def runner_off_case(be, tmp):
    """with the new flags absent or at their defaults the on-policy runner makes the calls it made before: policy_step with the same keywords,
    never policy_collect / policy_update, and ends with the same weights"""
    seen = {}
    for name, flags in (("absent", pc.POLICY_FLAGS), ("default", pc.POLICY_FLAGS + ("--policy_clip_eps", "0", "--policy_epochs", "1", "--policy_ratio", "sequence",
                                                                                  "--policy_old_logprobs", "forward"))):
        runner, model, _, _ = pc._pipeline(be, tmp, name, flags + ("--epochs", "1"))
        calls = []
        real = model.policy_step
        model.policy_step = lambda *a, _r=real, _c=calls, **k: _c.append((len(a), sorted(k))) or _r(*a, **k)
        model.policy_collect = lambda *a, **k: pytest.fail("policy_collect called with the flags off")
        model.policy_update = lambda *a, **k: pytest.fail("policy_update called with the flags off")
        lb = []
        real_lb = model.loss_and_backward
        model.loss_and_backward = lambda *a, _r=real_lb, _c=lb, **k: _c.append(sorted(k)) or _r(*a, **k)
        n_total = runner.optimizer.total_steps
        runner.train()
        seen[name] = (calls, lb, model._flat.detach().cpu().clone(), n_total)
    want = (5, sorted(["ref_model", "trie", "temperature", "num_samples", "baseline", "policy_coef", "sft_coef", "token_sum", "seed"]))
    assert seen["absent"][0] and all(c == want for c in seen["absent"][0]), seen["absent"][0][:2]
    assert all("clip_eps" not in k and "old_logprobs" not in k for k in seen["absent"][1])
    assert seen["default"][0] == seen["absent"][0] and seen["default"][1] == seen["absent"][1] and seen["default"][3] == seen["absent"][3]
    assert torch.equal(seen["default"][2], seen["absent"][2])
