"""Cases of the slate policy step (csrc/p5_slate_policy.h, p5_policy_slate_batch, P5T5Native.policy_slate_batch / policy_step(slate_size=...),
the runner's --policy_slate_size), shared by tests/test_slate_policy_emu.py (host emulation) and tests/test_gpu_slate_policy.py (MI355X).

1. the kernel through the C ABI against `ref_policy_slate_batch`, a numpy float64 restatement evaluated on the same fp32 inputs: integers and hit
   rewards exactly; omega, advantages, weights and slate_stats within KERNEL_TOL(K, X), relative to the user's largest reference magnitude;
   twice, the same bits; a slate's results do not depend on the other slates of the call.
   The bound, in units of u = 2^-24 (the unit roundoff of fp32), for a slot with x = phi - kappa, log q and y = phi - log q:
     x = fl(phi - kappa)                       absolute error |x| u
     e = expf(x), q = -expm1f(-e)              two transcendentals of <= 2 ulp = 4 u each; d log q / d log e = e exp(-e) / (1 - exp(-e)) <= 1, so
                                               log q inherits |x| u + 8 u
     logf(q)                                   2 u |log q| on top, |log q| <= 16 on this path (x > -16; for x <= -16 log q = x, no transcendental,
                                               and the neglected term e / 2 < 6e-8 < 1 u)
     y = fl(phi - log q), omega = expf(y)      |y| u + 4 u
   so omega is off by at most (|x| + |y| + 8 + 32 + 4) u = (X + 44) u relatively, X = the user's largest |x| + |y| over its existing slots.
   W, V and sum omega^2 are sums of K terms in slot order: K u each; the normalized advantage takes a second such sum (sum omega d), one
   divide, one subtract and two multiplies, the weights three more multiplies: 2 K u and a dozen u.  KERNEL_TOL(K, X) = (2 K + X + 64) 2^-24,
   and the test asserts that it stays <= 2^-14 for every combination it runs (a wrong q, q ~ u at u = 0.1, is off by 5 %).
   With the root noise (the sampler's values are conditioned on a maximum of 0; kappa = g - log1p((E - 1) exp(g)), E = -log u) kappa itself
   carries (|g| + 8 c) u, c = 1 / (1 + (E - 1) exp(g)) the amplification of the log1p: that term is added to X (`noise_kernel_case`).
   Largest error observed, as a share of the bound: KERNEL_OBSERVED.
2. the restatement against the distribution: unbiasedness of sum omega r and of W over 200 000 slates; the exact gradient when K1 > N.
3. the sampler's threshold is the kernel's: mean W = 1 and mean V = E_p[r] within 5 standard errors over 1024 slates of the engine's own
   sampler; the off-by-one threshold is more than 8 standard errors away.  This is the test that found the sampler's conditioning: with the
   sampler's value taken as the threshold as it is, mean W sat 4 standard errors below 1 for every user (printed as `conditioned threshold`).
4. meaning: the exact policy gradient when the catalogue fits in the slate; the formula of the loss on the oracle's item NLL.
5. composition: policy_step(slate_size=K) == sample_slates(K + 1) -> policy_slate_batch -> loss_and_backward, bit for bit.
6. refusals.  7. it learns.  8. the runner's flags."""
import itertools
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

PAD, EOS = pc.PAD, pc.EOS
ESTIMATORS = {"unbiased": 0, "normalized": 1}
KERNEL_OBSERVED = """largest error / bound over every combination of kernel_combos() (the printed `worst share of the bound`): host emulation 0.080
(S = 1, K1 = 4, normalized, given rewards); MI355X 0.080 (the same combination); with the root noise 0.044 on both"""


def KERNEL_TOL(K, X):
    return (2.0 * K + X + 64.0) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------
def ref_log_q(phi, kappa):
    """log of the inclusion probability q = 1 - exp(-exp(phi - kappa)) in float64; kappa = -inf: 0"""
    phi, kappa = np.asarray(phi, np.float64), np.asarray(kappa, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = phi - kappa
        lq = np.where(x < -30.0, x, np.log(-np.expm1(-np.exp(np.minimum(x, 50.0)))))
    return np.where(np.isneginf(kappa), 0.0, lq)


def ref_importance(phi, kappa):
    """omega = p / q in float64 (0 where phi = -inf)"""
    phi = np.asarray(phi, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(phi), 0.0, np.exp(phi - ref_log_q(np.where(np.isneginf(phi), 0.0, phi), kappa)))


def root_exp(seed, stream, slate):
    """E = exp(-Z) = -log u ~ Exp(1) of the root noise Z of one slate: the uniform of csrc/p5_rng.h at (seed, stream, slate, step 0, edge 2^32 - 1)"""
    from tests import sbs_cases
    return -math.log(float(sbs_cases.edge_uniforms(seed, stream, slate, 0, torch.tensor([0xFFFFFFFF], dtype=torch.int64))[0]))


def ref_kappa(g, e):
    """the un-conditioned threshold -log(exp(-g) - 1 + e) of a value g <= 0 conditioned on a maximum of 0, and 1 / (1 + (e - 1) exp(g)): how
    much the log1p amplifies the rounding of its argument"""
    if np.isneginf(g):
        return g, 0.0
    y = (e - 1.0) * math.exp(g)
    return g - math.log1p(y), 1.0 / (1.0 + y)


def condition_at_zero(pert):
    """perturbed values [.., K1] (descending) as a search whose root starts at G = 0 returns them: -log(exp(-g) - exp(-max) + 1)"""
    g = np.asarray(pert, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        out = -np.log1p(np.exp(-g) - np.exp(-g[..., :1]))
    return np.where(np.isneginf(g), -np.inf, out).astype(np.float32)


def ref_policy_slate_batch(seq, lp, pert, labels, attn, rewards, tok_lp, S, K1, estimator, policy_coef, sft_coef, token_sum, with_gold, noise=None):
    """numpy float64 restatement of p5_policy_slate_batch on the same fp32 inputs: seq int64 [B*S*K1, Ts], lp / pert [B, S, K1], rewards
    [B, S, K1] or None, tok_lp [B*S*K1, Ts-1] or None; noise = (seed, streams [B], slate_base) or None"""
    seq, labels, attn = np.asarray(seq), np.asarray(labels), np.asarray(attn)
    K = K1 - 1
    B, Ts, Tg = seq.shape[0] // (S * K1), seq.shape[1], labels.shape[1]
    G, To = S * K + with_gold, max(Tg, Ts - 1)
    lp, pert = np.asarray(lp, np.float64).reshape(B, S, K1), np.asarray(pert, np.float64).reshape(B, S, K1)
    lab_o, att_o = np.zeros((B, G, To), np.int64), np.zeros((B, G, To), np.int64)
    old = np.zeros((B, G, To), np.float64)
    mode = np.ones((B, G), np.int32)
    r, A, om = np.zeros((B, S, K)), np.zeros((B, S, K)), np.zeros((B, S, K))
    w = np.zeros((B, G))
    hits = np.zeros((B, S, K), bool)
    n = np.zeros((B, S, K), np.int64)
    st = np.zeros((B, S, 4))
    X = np.zeros(B)
    for b in range(B):
        attended = (attn[b] != 0) & (np.cumsum(labels[b] == -100) == 0)
        gold = [int(t) for t in labels[b][attended]]
        if with_gold:
            lab_o[b, 0, :Tg], att_o[b, 0, :Tg] = labels[b], attended
            w[b, 0] = np.float64(np.float32(sft_coef)) * G
            mode[b, 0] = 0
        for j in range(S):
            kappa, amp = pert[b, j, K], 0.0
            if noise is not None:
                kappa, amp = ref_kappa(kappa, root_exp(noise[0], int(noise[1][b]), noise[2] + j))
            for i in range(K):
                e = (b * S + j) * K1 + i
                row = [int(t) for t in seq[e, 1:]]
                k = pc.draw_length(row)
                g = with_gold + j * K + i
                n[b, j, i] = k
                lab_o[b, g, :k], att_o[b, g, :k] = row[:k], 1
                if tok_lp is not None:
                    old[b, g, :k] = tok_lp[e, :k]
                hits[b, j, i] = k > 0 and row[:k] == gold
                if k > 0:
                    r[b, j, i] = float(rewards[b, j, i]) if rewards is not None else float(hits[b, j, i])
                    lq = float(ref_log_q(lp[b, j, i], kappa))
                    om[b, j, i] = math.exp(lp[b, j, i] - lq)
                    X[b] = max(X[b], (abs(lp[b, j, i] - kappa) if np.isfinite(kappa) else 0.0) + abs(lp[b, j, i] - lq)
                               + (8.0 * amp + abs(pert[b, j, K]) if amp else 0.0))
            ex = n[b, j] > 0
            W, V, W2 = om[b, j][ex].sum(), (om[b, j] * r[b, j])[ex].sum(), (om[b, j][ex] ** 2).sum()
            st[b, j] = V, W, kappa, (W * W / W2 if W2 > 0 else 0.0)
            if not ex.any():
                continue
            if estimator == "unbiased":
                A[b, j][ex] = (om[b, j] * r[b, j])[ex]
            elif not bool((r[b, j][ex] == r[b, j][ex][0]).all()):
                A[b, j][ex] = (om[b, j][ex] / W) * (r[b, j][ex] - V / W)
        w[b, with_gold:] = (np.float64(np.float32(policy_coef)) * A[b] * G / S * (n[b] if token_sum else 1)).reshape(-1)
    exs = (n > 0).any(axis=2)
    ns, nslot = max(int(exs.sum()), 1), max(int((n > 0).sum()), 1)
    stats = np.array([st[..., 0][exs].sum() / ns, st[..., 1][exs].sum() / ns, np.mean((A != 0).any(axis=(1, 2))), np.abs(A).sum() / nslot,
                      hits.any(axis=2)[exs].sum() / ns, np.isneginf(st[..., 2])[exs].sum() / ns, float((~exs.any(axis=1)).sum()), st[..., 3][exs].sum() / ns])
    return dict(labels=lab_o, output_attention=att_o, rewards=r, advantages=A, importance=om, weights=w, slate_stats=st, stats=stats, hits=hits, n=n,
                old_logprobs=old, target_mode=mode, X=X)


# ---------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------
KERNEL_SK1 = ((1, 2), (1, 4), (3, 4), (5, 3), (16, 64), (2, 300))       # ... the limit S K1 = 1024; slots strided over the threads
KERNEL_SHAPES = ((3, 6), (8, 6))                                       # (Tg, Ts): Tg < Ts - 1, Tg > Ts - 1


def kernel_combos():
    """(S, K1, estimator, given rewards?) -- each runs every (Tg, Ts) x with_gold x token_logprobs x token_sum"""
    return [(S, K1, est, given) for (S, K1) in KERNEL_SK1 for est in ("unbiased", "normalized") if not (est == "normalized" and K1 < 3)
            for given in (False, True)]


def _item_row(i, room, short=False):
    """the token row of synthetic item i: two tokens that name it, up to two more, </s>"""
    extra = 0 if short else min(i % 3, room - 3)
    return [10 + i % 30, 50 + i // 30] + [90 + k for k in range(extra)] + [EOS]


def gumbel_slates(g, logp, S, K1):
    """S Gumbel top-K1 draws over the categorical distribution exp(logp): (item index [S, K1] with -1 behind the last item, perturbed [S, K1])"""
    N = logp.shape[0]
    pert = logp[None, :] - np.log(-np.log(g.random((S, N))))
    order = np.argsort(-pert, axis=1)[:, :K1]
    idx = np.full((S, K1), -1, np.int64)
    val = np.full((S, K1), -np.inf)
    idx[:, :order.shape[1]] = order
    val[:, :order.shape[1]] = np.take_along_axis(pert, order, axis=1)
    return idx, val


def kernel_problem(S, K1, Tg, Ts, given, seed):
    """B = 5 users.  Every slate is a Gumbel top-K1 draw in numpy over a known categorical distribution of N items whose token rows come from a
    small trie (`_item_row`).  User b:
      0  N = K1 + 5; the gold is the item in slot 0 of slate 0 (a hit); its LAST slate carries a slot with phi = -100 under kappa = -3
         (phi - kappa = -97: omega must be e^-3, not inf)
      1  all-pad rows only: nothing drawn (phi = g = -inf)
      2  N = min(K1 - 1, 3) < K1: every item is in the slate, the trailing slots are all-pad, kappa = -inf: omega = p and W = 1
      3  N = K1 + 5, no slot is the gold and the given rewards are all -1.7: equal rewards; the gold's tail is labelled -100 under attention 1
      4  as user 0 without a hit; slot 0 of slate 0 is a draw cut without </s> with phi = -0.5 under kappa = -12.5 (phi - kappa = +12: q = 1);
         the gold's tail is labelled -100
    Returns seq [B*S*K1, Ts], lp / pert fp32 [B, S, K1], labels / attn [B, Tg], rewards fp32 [B, S, K1] or None, tok_lp fp32 [B*S*K1, Ts-1]."""
    g = np.random.default_rng(seed)
    B, K, room = 5, K1 - 1, Ts - 1
    seq = np.zeros((B * S * K1, Ts), np.int64)
    lp = np.full((B, S, K1), -np.inf, np.float32)
    pert = np.full((B, S, K1), -np.inf, np.float32)
    labels, attn = np.zeros((B, Tg), np.int64), np.zeros((B, Tg), np.int64)
    rewards = (g.standard_normal((B, S, K1)) * 1.5).astype(np.float32) if given else None
    tok_lp = -g.random((B * S * K1, Ts - 1)).astype(np.float32)
    for b in range(B):
        if b == 1:
            gold = [20, 21, EOS]
        else:
            N = min(K1 - 1, 3) if b == 2 else K1 + 5
            logits = g.standard_normal(N) * 1.5
            logp = logits - np.log(np.exp(logits).sum())
            idx, val = gumbel_slates(g, logp, S, K1)
            head = int(idx[0, 0])
            rows = {i: _item_row(i, room, short=(i == head)) for i in range(N)}
            if b == 4:
                rows[head] = [10 + head % 30, 50 + head // 30] + [95] * (room - 2)          # no </s>: cut by the length limit
            for j in range(S):
                for i in range(K1):
                    if idx[j, i] >= 0:
                        e = (b * S + j) * K1 + i
                        seq[e, 1:1 + len(rows[int(idx[j, i])])] = rows[int(idx[j, i])]
                        lp[b, j, i], pert[b, j, i] = logp[idx[j, i]], val[j, i]
            gold = rows[head] if b in (0, 2) else [8, 9, EOS]
            if b == 0:
                lp[b, S - 1, K - 1], pert[b, S - 1, K] = -100.0, -3.0
                if K > 1:
                    pert[b, S - 1, K - 1] = -2.9
            if b == 4:
                lp[b, 0, 0], pert[b, 0, K] = -0.5, -12.5
        if b in (3, 4):
            if Tg > 3:
                labels[b, :3], labels[b, 3:] = gold, -100
                attn[b, :] = 1
            else:
                labels[b], attn[b] = [gold[0], -100, EOS], 1
        else:
            labels[b, :3], attn[b, :3] = gold, 1
        if given and b == 3:
            rewards[b] = -1.7
    return seq, lp, pert, labels, attn, rewards, tok_lp


def run_slate_abi(be, seq, lp, pert, labels, attn, rewards, tok_lp, S, K1, estimator, policy_coef, sft_coef, token_sum, with_gold, with_mode=True,
                  noise=None):
    from openp5_amd.model import _ptr
    dv = be.device
    K = K1 - 1
    B, Ts, Tg = seq.shape[0] // (S * K1), seq.shape[1], labels.shape[1]
    G, To = S * K + with_gold, max(Tg, Ts - 1)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dv)       # noqa: E731
    d_seq, d_lp, d_pert, d_lab, d_att, d_rew, d_tlp = t(seq), t(lp), t(pert), t(labels), t(attn), t(rewards), t(tok_lp)
    lab_o = torch.full((B, G, To), -7, dtype=torch.int64, device=dv)
    att_o = torch.full((B, G, To), -7, dtype=torch.int64, device=dv)
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dv)      # noqa: E731
    r_o, a_o, i_o, w_o, ss, us, st = f(B, S, K), f(B, S, K), f(B, S, K), f(B, G), f(B, S, 4), f(B, 8), f(8)
    old_o = f(B, G, To) if tok_lp is not None else None
    mode_o = torch.full((B, G), -7, dtype=torch.int32, device=dv) if tok_lp is not None and with_mode else None
    d_streams = None if noise is None else t(np.asarray(noise[1]).astype(np.int64).astype(np.uint32).view(np.int32))
    rc = be.lib.p5_policy_slate_batch(_ptr(d_seq), _ptr(d_lp), _ptr(d_pert), _ptr(d_lab), _ptr(d_att), _ptr(d_rew), _ptr(d_tlp), B, S, K1, Ts, Tg,
                                      ESTIMATORS[estimator], policy_coef, sft_coef, int(token_sum), with_gold, PAD, EOS, _ptr(lab_o), _ptr(att_o), _ptr(r_o),
                                      _ptr(a_o), _ptr(i_o), _ptr(w_o), _ptr(ss), _ptr(us), _ptr(st), _ptr(old_o), _ptr(mode_o), _ptr(d_streams),
                                      0 if noise is None else int(noise[0]) & 0xFFFFFFFF, 0 if noise is None else int(noise[2]) & 0xFFFFFFFF, be.stream_ptr())
    be.check(rc, "p5_policy_slate_batch")
    sync(be)
    out = dict(labels=lab_o, output_attention=att_o, rewards=r_o, advantages=a_o, importance=i_o, weights=w_o, slate_stats=ss, stats=st)
    if old_o is not None:
        out["old_logprobs"] = old_o
    if mode_o is not None:
        out["target_mode"] = mode_o
    return {k: v.cpu().numpy() for k, v in out.items()}


def _share(got, ref, tol, what):
    """per user (row): |got - ref| <= tol * the row's largest reference magnitude; returns the largest error as a share of the bound"""
    got, ref = np.asarray(got, np.float64).reshape(ref.shape[0], -1), np.asarray(ref).reshape(ref.shape[0], -1)
    assert np.isfinite(got).all(), what
    scale = np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(got - ref)
    tol = np.asarray(tol, np.float64).reshape(-1, 1)
    assert (err <= tol * scale).all(), (what, float((err / np.maximum(scale * tol, 1e-300)).max()))
    return float((err / np.maximum(scale * tol, 1e-300)).max())


def kernel_case(be, S, K1, estimator, given, seed=0):
    policy_coef, sft_coef = 0.7, 1.3
    K = K1 - 1
    worst = 0.0
    for (Tg, Ts), with_gold, with_tlp, token_sum in itertools.product(KERNEL_SHAPES, (0, 1), (False, True), (0, 1)):
        tag = f"S={S} K1={K1} {estimator} given={given} Tg={Tg} Ts={Ts} gold={with_gold} tlp={with_tlp} sum={token_sum}"
        seq, lp, pert, labels, attn, rewards, tok_lp = kernel_problem(S, K1, Tg, Ts, given, seed + 17 * Tg + 1000 * S + K1)
        tlp = tok_lp if with_tlp else None
        ref = ref_policy_slate_batch(seq, lp, pert, labels, attn, rewards, tlp, S, K1, estimator, policy_coef, sft_coef, token_sum, with_gold)
        B = 5
        tol = np.array([KERNEL_TOL(K, x) for x in ref["X"]])
        assert tol.max() <= 2.0 ** -14, (tag, tol.max())
        # the planted rows are there
        x0 = np.float64(lp[0, S - 1, K - 1]) - np.float64(pert[0, S - 1, K])
        assert x0 == -97.0 and ref["n"][0, S - 1, K - 1] > 0 and abs(ref["importance"][0, S - 1, K - 1] - math.exp(-3.0)) < 1e-12, tag
        assert (ref["n"][1] == 0).all() and ref["stats"][6] == 1, tag
        N2 = min(K1 - 1, 3)
        assert np.isneginf(pert[2, :, K]).all() and (ref["n"][2, :, N2:] == 0).all() and (ref["n"][2, :, :N2] > 0).all(), tag     # N < K1
        assert np.float64(lp[4, 0, 0]) - np.float64(pert[4, 0, K]) == 12.0 and abs(ref["importance"][4, 0, 0] - math.exp(-0.5)) < 1e-5, tag
        assert ref["n"][4, 0, 0] == Ts - 1 and EOS not in seq[(4 * S) * K1, 1:], tag                                   # a draw cut without </s>
        assert (labels[3] == -100).any() and (labels[4] == -100).any(), tag
        assert ref["hits"][0, 0, 0] and not ref["hits"][3].any(), tag
        ex3 = ref["n"][3] > 0
        assert ex3.all() and (ref["rewards"][3] == ref["rewards"][3, 0, 0]).all(), tag                                  # equal rewards
        runs = [run_slate_abi(be, seq, lp, pert, labels, attn, rewards, tlp, S, K1, estimator, policy_coef, sft_coef, token_sum, with_gold) for _ in range(2)]
        for k, v in runs[0].items():
            assert v.tobytes() == runs[1][k].tobytes(), f"{tag}: two runs differ in {k}"
        got = runs[0]
        assert np.array_equal(got["labels"], ref["labels"]), tag
        assert np.array_equal(got["output_attention"], ref["output_attention"]), tag
        assert np.array_equal(got["rewards"], (ref["hits"] if rewards is None else ref["rewards"]).astype(np.float32)), tag
        if with_tlp:
            assert np.array_equal(got["old_logprobs"], ref["old_logprobs"].astype(np.float32)) and np.array_equal(got["target_mode"], ref["target_mode"]), tag
        shares = [_share(got["importance"], ref["importance"], tol, tag + " importance"),
                  _share(got["advantages"], ref["advantages"], tol, tag + " advantages"),
                  _share(got["weights"], ref["weights"], tol, tag + " weights")]
        for c, name in ((0, "V"), (1, "W"), (3, "ESS")):
            shares.append(_share(got["slate_stats"][..., c], ref["slate_stats"][..., c], tol, f"{tag} slate_stats {name}"))
        assert np.array_equal(got["slate_stats"][..., 2], pert[..., K]), tag                                            # kappa: copied
        top = max(1.0, float(np.abs(ref["stats"]).max()))
        assert np.isfinite(got["stats"]).all() and (np.abs(got["stats"] - ref["stats"]) <= tol.max() * top).all(), (tag, got["stats"], ref["stats"])
        assert got["stats"][6] == 1
        # the planted rows' meaning
        assert np.isfinite(got["importance"]).all() and abs(got["importance"][0, S - 1, K - 1] - math.exp(-3.0)) <= tol[0] * math.exp(-3.0) * 2, tag
        e2 = ref["n"][2] > 0
        assert (np.abs(got["importance"][2][e2] - np.exp(lp[2, :, :K].astype(np.float64))[e2]) <= tol[2]).all(), tag     # kappa = -inf: omega = p
        assert (np.abs(got["slate_stats"][2, :, 1] - 1.0) <= tol[2] + 3 * 2.0 ** -24).all(), (tag, got["slate_stats"][2, :, 1])   # (log p rounded to fp32)
        assert (got["importance"][1] == 0).all() and (got["advantages"][1] == 0).all() and (got["weights"][1, with_gold:] == 0).all(), tag
        assert (got["output_attention"][1, with_gold:] == 0).all(), tag
        if estimator == "normalized":
            assert (got["advantages"][3] == 0.0).all() and (got["weights"][3, with_gold:] == 0.0).all(), (tag, got["advantages"][3])
        worst = max(worst, max(shares))
    print(f"[slate kernel] S={S} K1={K1} {estimator} given={given}: worst share of the bound {worst:.3f}")
    return worst


def independence_case(be, estimator="normalized", noise=None):
    """the advantages, importance and slate_stats of a slate are bit-equal whether the call holds S = 4 slates or the same slates in two calls
    of S = 2 (with the root noise: at slate_base + 2)"""
    S, K1, Tg, Ts = 4, 4, 3, 6
    seq, lp, pert, labels, attn, rewards, _ = kernel_problem(S, K1, Tg, Ts, True, 5)
    if noise is not None:
        pert = condition_at_zero(pert)
    whole = run_slate_abi(be, seq, lp, pert, labels, attn, rewards, None, S, K1, estimator, 0.7, 1.3, 0, 1, noise=noise)
    B = 5
    seq4 = seq.reshape(B, S, K1, Ts)
    for h in (0, 1):
        sl = slice(2 * h, 2 * h + 2)
        part = run_slate_abi(be, seq4[:, sl].reshape(-1, Ts), lp[:, sl], pert[:, sl], labels, attn, rewards[:, sl], None, 2, K1, estimator, 0.7, 1.3, 0, 1,
                             noise=None if noise is None else (noise[0], noise[1], noise[2] + 2 * h))
        for k in ("advantages", "importance", "slate_stats", "rewards"):
            assert whole[k][:, sl].tobytes() == part[k].tobytes(), (h, k)
    assert float(np.abs(whole["advantages"]).max()) > 0


NOISE = (0x5EED1234, np.array([7, 0, 2 ** 32 - 1, 12345, 3]), 2 ** 32 - 3)       # seed, stream ids, slate_base (the slate index wraps modulo 2^32)


def noise_kernel_case(be, S, K1, estimator):
    """the kernel with the root noise on (the values of a search whose root starts at 0) against the restatement: the threshold it reports and
    everything behind it within the bound, twice the same bits; and the threshold differs from the conditioned value it was given"""
    K, Tg, Ts = K1 - 1, 3, 6
    seq, lp, pert, labels, attn, rewards, _ = kernel_problem(S, K1, Tg, Ts, True, 31 + S)
    pert = condition_at_zero(pert)
    assert (pert[np.isfinite(pert)] <= 0).all() and (pert[0, :, 0] == 0).all()
    ref = ref_policy_slate_batch(seq, lp, pert, labels, attn, rewards, None, S, K1, estimator, 0.7, 1.3, 1, 1, noise=NOISE)
    tol = np.array([KERNEL_TOL(K, x) for x in ref["X"]])
    assert tol.max() <= 2.0 ** -14, tol.max()
    runs = [run_slate_abi(be, seq, lp, pert, labels, attn, rewards, None, S, K1, estimator, 0.7, 1.3, 1, 1, noise=NOISE) for _ in range(2)]
    for k, v in runs[0].items():
        assert v.tobytes() == runs[1][k].tobytes(), k
    got = runs[0]
    kap, kap_ref = got["slate_stats"][..., 2].astype(np.float64), ref["slate_stats"][..., 2]
    fin = np.isfinite(kap_ref)
    assert np.array_equal(np.isneginf(kap), ~fin) and fin[[0, 3, 4]].all() and not fin[[1, 2]].any()
    assert (np.abs(kap[fin] - kap_ref[fin]) <= (tol[:, None] * np.maximum(1.0, np.abs(kap_ref)))[fin]).all()
    assert (np.abs(kap_ref[fin] - pert[..., K][fin]) > 1e-3).any(), "the root noise moved no threshold"
    worst = 0.0
    for k in ("importance", "advantages", "weights"):
        worst = max(worst, _share(got[k], ref[k], tol, k))
    for c in (0, 1, 3):
        worst = max(worst, _share(got["slate_stats"][..., c], ref["slate_stats"][..., c], tol, f"slate_stats {c}"))
    print(f"[slate kernel, root noise] S={S} K1={K1} {estimator}: worst share of the bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------
# 2. the restatement against the distribution (numpy only)
# ---------------------------------------------------------------------------------------------------------
def distribution_case(K, N=7, M=200_000, seed=3):
    """|mean(sum omega r) - sum p r| and |mean W - 1| within 5 standard errors over M Gumbel top-(K + 1) slates"""
    g = np.random.default_rng(seed)
    logits = g.standard_normal(N) * 1.2
    logp = logits - np.log(np.exp(logits).sum())
    r = g.standard_normal(N) * 1.5 + 0.5
    idx, val = gumbel_slates(g, logp, M, K + 1)
    phi = logp[idx[:, :K]]
    om = ref_importance(phi, val[:, K:K + 1])
    V, W = (om * r[idx[:, :K]]).sum(1), om.sum(1)
    zV = (V.mean() - float(np.exp(logp) @ r)) / (V.std() / math.sqrt(M))
    zW = (W.mean() - 1.0) / (W.std() / math.sqrt(M))
    print(f"[slate distribution] K={K}: z(V) {zV:+.2f}, z(W) {zW:+.2f}")
    assert abs(zV) <= 5.0 and abs(zW) <= 5.0, (K, zV, zW)


def exact_gradient_case(N=7, seed=4):
    """K1 > N: kappa = -inf, omega = p, and the `unbiased` gradient w.r.t. the logits, sum_s A_s (e_s - p), equals p (r - E r) to 1e-12"""
    g = np.random.default_rng(seed)
    logits = g.standard_normal(N)
    logp = logits - np.log(np.exp(logits).sum())
    p, r = np.exp(logp), g.standard_normal(N)
    K1 = N + 1
    idx, val = gumbel_slates(g, logp, 1, K1)
    assert idx[0, N] == -1 and np.isneginf(val[0, N])
    Ts = 6
    seq = np.zeros((K1, Ts), np.int64)
    for i in range(N):
        row = _item_row(int(idx[0, i]), Ts - 1)
        seq[i, 1:1 + len(row)] = row
    lp = np.full((1, 1, K1), -np.inf)
    lp[0, 0, :N] = logp[idx[0, :N]]
    rew = np.zeros((1, 1, K1))
    rew[0, 0, :N] = r[idx[0, :N]]
    ref = ref_policy_slate_batch(seq, lp, val[None], np.array([[8, 9, EOS]]), np.ones((1, 3), np.int64), rew, None, 1, K1, "unbiased", 1.0, 0.0, 1, 0)
    A = ref["advantages"][0, 0]
    grad = np.zeros(N)
    for i in range(N):
        e = np.zeros(N)
        e[idx[0, i]] = 1.0
        grad += A[i] * (e - p)
    assert np.abs(grad - p * (r - p @ r)).max() <= 1e-12
    assert abs(ref["slate_stats"][0, 0, 1] - 1.0) <= 1e-12 and np.isneginf(ref["slate_stats"][0, 0, 2])


# ---------------------------------------------------------------------------------------------------------
# 3. the sampler and the kernel agree on the threshold
# ---------------------------------------------------------------------------------------------------------
def threshold_case(be, ocfg, B=3, L=12, K=3, M=1024, chunk=256, tau=1.0, seed=21):
    items = cases.make_items(8, 5, hi=60)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    K1 = K + 1
    full = m.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=9, num_slates=1, temperature=tau, seed=seed)
    fi, fl = full["item_index"].cpu().numpy().reshape(B, 9), full["sequences_logprob"].cpu().numpy().reshape(B, 9).astype(np.float64)
    assert (fi[:, :8] >= 0).all() and (fi[:, 8] == -1).all()
    r_item = (np.arange(8) * 7 % 5).astype(np.float64) - 1.5
    truth = np.array([(np.exp(fl[b, :8]) * r_item[fi[b, :8]]).sum() for b in range(B)])
    assert np.abs(np.exp(fl[:, :8]).sum(1) - 1.0).max() < 1e-4
    V, W, Wwrong, Wcond = [], [], [], []
    for s0 in range(0, M, chunk):
        d = m.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=K1, num_slates=chunk, temperature=tau, seed=seed,
                            slate_base=s0)
        seq = d["sequences"].cpu().numpy()
        lp = d["sequences_logprob"].cpu().numpy().reshape(B, chunk, K1)
        pert = d["perturbed"].cpu().numpy()
        rew = pc.index_reward(d).cpu().numpy().astype(np.float32)
        seed_, streams_, base_ = d["noise_key"]
        assert seed_ == seed and base_ == s0 and (pert[..., 0] == 0).all()                 # the sampler's root starts at G = 0
        noise = (seed_, streams_.cpu().numpy().view(np.uint32), base_)
        out = run_slate_abi(be, seq, lp, pert, labels.numpy(), out_attn.numpy(), rew, None, chunk, K1, "unbiased", 1.0, 0.0, 1, 0, noise=noise)
        V.append(out["slate_stats"][..., 0].astype(np.float64))
        W.append(out["slate_stats"][..., 1].astype(np.float64))
        kap = out["slate_stats"][..., 2].astype(np.float64)                                # the un-conditioned threshold the kernel used
        prev = np.array([[ref_kappa(float(pert[b, j, K - 1]), root_exp(seed_, int(noise[1][b]), base_ + j))[0] for j in range(chunk)] for b in range(B)])
        assert (kap <= prev + 1e-6).all()
        Wwrong.append(ref_importance(lp[..., :K], prev[..., None]).sum(2))                  # ... off by one: slot K - 1 as the threshold
        Wcond.append(ref_importance(lp[..., :K], pert[..., K:K + 1]).sum(2))                # ... the sampler's value as it is: conditioned on max = 0
    V, W, Wwrong, Wcond = np.concatenate(V, 1), np.concatenate(W, 1), np.concatenate(Wwrong, 1), np.concatenate(Wcond, 1)
    se = lambda a: a.std(axis=1) / math.sqrt(M)      # noqa: E731
    zW, zV, zX = (W.mean(1) - 1.0) / se(W), (V.mean(1) - truth) / se(V), (Wwrong.mean(1) - 1.0) / se(Wwrong)
    zC = (Wcond.mean(1) - 1.0) / se(Wcond)
    print(f"[slate threshold] z(W) {zW.round(2)}, z(V) {zV.round(2)}, off-by-one threshold z(W) {zX.round(2)}, conditioned threshold z(W) {zC.round(2)}")
    assert (np.abs(zW) <= 5.0).all() and (np.abs(zV) <= 5.0).all(), (zW, zV)
    assert (np.abs(zX) > 8.0).all(), zX


# ---------------------------------------------------------------------------------------------------------
# 4. meaning
# ---------------------------------------------------------------------------------------------------------
def _item_reward(n):
    return (torch.arange(n) * 7 % 5).double() - 1.5


def exact_meaning_case(be, ocfg, B=3, L=12, policy_coef=0.7, seed=5, tau=0.8):
    """the catalogue (6 items) fits in the slate: the gradient arena equals the autograd of -policy_coef mean_b sum_s p_b(s) r(s), p from the
    oracle's item NLL in float64 over all items; user 1 has excluded items, so its trailing slots are all-pad"""
    items = cases.make_items(6, 5, hi=60)
    N = len(items)
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    excluded = [[], [1, 4], []]
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, 1, temperature=tau, excluded_items=excluded, policy_coef=policy_coef, sft_coef=0.0,
                         token_sum=True, reward_fn=pc.index_reward, seed=seed, slate_size=N, slate_estimator="unbiased")
    sync(be)
    pb = m.last_policy_batch
    ss = pb["slate_stats"].cpu().numpy()
    assert np.isneginf(ss[:, 0, 2]).all() and np.abs(ss[:, 0, 1] - 1.0).max() < 1e-4                 # kappa = -inf, W = 1
    assert (pb["output_attention"][1].sum(1) == 0).sum() == 2, "user 1: two all-pad slots"
    To = pb["labels"].shape[2]
    lab = torch.zeros(B, N, To, dtype=torch.int64)
    for i, q in enumerate(items):
        lab[:, i, :len(q) - 1] = torch.tensor(q[1:])
    msk = (lab != 0).double()
    Pq = mt._oracle_params(params, "bf16")
    excl = np.repeat(ct.excluded_bitmap(excluded), N, axis=0)
    nll_o, _, _ = tl.oracle_item_nll(Pq, ocfg, mt.rep(ids, N), mt.rep(ww, N), mt.rep(mask, N), lab.view(B * N, To), ct, tau, excl)
    logp = -(nll_o.view(B, N, To) * msk).sum(2)
    allowed = torch.ones(B, N, dtype=torch.float64)
    allowed[1, excluded[1]] = 0.0
    p = torch.exp(logp) * allowed
    assert float((p.detach().sum(1) - 1.0).abs().max()) < 1e-9
    r = _item_reward(N)
    loss_o = -policy_coef * (p * r).sum(1).mean()
    loss_o.backward()
    surrogate = float(policy_coef * (p.detach() * r * -logp.detach() * allowed).sum(1).mean())
    _, worst = mt._fp32_errors(m, Pq, nll_o, nll_o)
    print(f"[slate exact gradient] loss {float(loss):.6f} surrogate {surrogate:.6f}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert abs(float(loss) - surrogate) <= mt.NLL_TOL * max(1.0, abs(surrogate)), (float(loss), surrogate)
    assert worst[0] <= mt.GRAD_TOL, worst


def meaning_case(be, ocfg, items, estimator, B=3, L=12, K=3, S=2, policy_coef=0.7, sft_coef=1.3, token_sum=True, seed=5, tau=0.8):
    """K = 3 < N with the gold: loss == sft_coef mean_b l(gold_b) + policy_coef mean_b (1/S) sum_j sum_i A_bji l_bji in float64 on the oracle's
    item NLL of the replicated batch, A from the float64 reference; gradients == its autograd"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, S, temperature=tau, policy_coef=policy_coef, sft_coef=sft_coef, token_sum=token_sum,
                         reward_fn=pc.index_reward, seed=seed, slate_size=K, slate_estimator=estimator)
    sync(be)
    pb = m.last_policy_batch
    m2 = cases.build_model(be, ocfg, params, "fp32")
    m2.eval()
    d = m2.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=K + 1, num_slates=S, temperature=tau, seed=seed)
    ref = ref_policy_slate_batch(d["sequences"].cpu().numpy(), d["sequences_logprob"].cpu().numpy(), d["perturbed"].cpu().numpy(), labels.numpy(),
                                 out_attn.numpy(), pc.index_reward(d).cpu().numpy(), None, S, K + 1, estimator, policy_coef, sft_coef, token_sum, 1,
                                 noise=(d["noise_key"][0], d["noise_key"][1].cpu().numpy().view(np.uint32), d["noise_key"][2]))
    assert np.array_equal(ref["labels"], pb["labels"].cpu().numpy()) and float(np.abs(ref["advantages"]).max()) > 0
    assert np.isfinite(ref["slate_stats"][..., 2]).all()
    G, To = S * K + 1, ref["labels"].shape[2]
    Pq = mt._oracle_params(params, "bf16")
    nll_o, _, _ = tl.oracle_item_nll(Pq, ocfg, mt.rep(ids, G), mt.rep(ww, G), mt.rep(mask, G), torch.from_numpy(ref["labels"]).view(B * G, To), ct, tau, None)
    msk = torch.from_numpy(ref["output_attention"]).double()
    tok = (nll_o.view(B, G, To) * msk).sum(2)
    per = tok if token_sum else tok / msk.sum(2).clamp(min=1)
    per_gold = tok[:, 0] / msk[:, 0].sum(1).clamp(min=1)
    A = torch.from_numpy(ref["advantages"]).view(B, S * K)
    loss_o = sft_coef * per_gold.mean() + policy_coef * ((A * per[:, 1:]).sum(1) / S).mean()
    loss_o.backward()
    lo = float(loss_o.detach())
    _, worst = mt._fp32_errors(m, Pq, nll_o, nll_o)
    print(f"[slate meaning {estimator}] loss {float(loss):.6f} oracle {lo:.6f}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert abs(float(loss) - lo) <= mt.NLL_TOL * max(1.0, abs(lo)), (float(loss), lo)
    assert worst[0] <= mt.GRAD_TOL, worst


# ---------------------------------------------------------------------------------------------------------
# 5. composition
# ---------------------------------------------------------------------------------------------------------
def composition_case(be, ocfg, items, dtype="fp32", item_head="dense", reg=False, B=3, L=12, S=2, K=2, estimator="normalized", seed=11, **kw):
    """policy_step(slate_size=K, seed=s) against its three parts on a fresh model with the same weights: loss and gradient arena bit for bit"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    excluded_items = [[i for i in range(b, len(items), 3)] if b != 1 else [] for b in range(B)]
    common = dict(temperature=0.8, excluded_items=excluded_items, item_head=item_head)
    regkw, ref, res = {}, None, []
    for whole in (True, False):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        if reg:
            ref = m.frozen_copy()
            with torch.no_grad():
                ref._flat.mul_(1.01)
            ref.mark_params_updated()
            regkw = dict(entropy_coef=0.05, kl_coef=0.2)
        if whole:
            loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, S, seed=seed, ref_model=ref, reward_fn=pc.index_reward, slate_size=K,
                                 slate_estimator=estimator, **regkw, **common, **kw)
            assert m.last_policy_stats.shape == (8,) and m.last_policy_batch["labels"].shape[:2] == (B, S * K + (kw.get("sft_coef", 1.0) != 0.0))
            assert m.last_policy_batch["importance"].shape == (B, S, K) and m.last_policy_batch["slate_stats"].shape == (B, S, 4)
        else:
            out = m.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=K + 1, num_slates=S, temperature=0.8,
                                  excluded_items=excluded_items, seed=seed)
            pb = m.policy_slate_batch(out, labels, out_attn, K, S, rewards=pc.index_reward(out), estimator=estimator, **kw)
            if reg:
                regkw["ref_logits"] = ref.item_logits(ids, ww, mask, pb["labels"], ct, temperature=0.8, excluded_items=excluded_items, item_head=item_head)
            loss = m.loss_and_backward(ids, ww, mask, pb["labels"], pb["output_attention"], trie=ct, target_weights=pb["target_weights"], **regkw, **common)
        sync(be)
        res.append((loss.detach().cpu().clone(), m._grads.detach().cpu().clone()))
    (l0, g0), (l1, g1) = res
    assert math.isfinite(float(l0)) and float(g0.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(g0, g1), (float(l0), float(l1), float((g0 - g1).abs().max()))


def clip_case(be, ocfg, items, B=3, L=12, S=2, K=2, seed=11):
    """policy_step(slate_size=K, clip_eps=...) == policy_collect(slate_size=K) + one policy_update, bit for bit; with one update the clip
    statistics report a ratio of 1 (fp32, old_logprobs="sampler": up to the last bits of the decode kernels against the training forward)"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    kw = dict(temperature=0.8, reward_fn=pc.index_reward, seed=seed, slate_size=K, slate_estimator="normalized", token_sum=True)
    res = []
    for whole in (True, False):
        m = cases.build_model(be, ocfg, params, "fp32")
        m.eval()
        if whole:
            loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, S, clip_eps=0.2, **kw)
        else:
            ro = m.policy_collect(ids, ww, mask, labels, out_attn, ct, S, clip_eps=0.2, **kw)
            assert ro["old_logprobs"].shape == ro["labels"].shape and ro["target_mode"].shape == ro["labels"].shape[:2]
            assert ro["target_mode"][:, 0].eq(0).all() and ro["target_mode"][:, 1:].eq(1).all() and "importance" in ro
            loss = m.policy_update(ids, ww, mask, ro, ct, 0.2, temperature=0.8)
        sync(be)
        cs = dict(zip(m.CLIP_STATS, m.last_clip_stats.cpu().tolist()))
        assert cs["units"] > 0 and cs["clipped"] == 0 and abs(cs["ratio_mean"] - 1.0) < 1e-4 and abs(cs["ratio_max"] - 1.0) < 1e-3, cs
        res.append((loss.detach().cpu().clone(), m._grads.detach().cpu().clone()))
    (l0, g0), (l1, g1) = res
    assert float(g0.abs().max()) > 0 and torch.equal(l0, l1) and torch.equal(g0, g1)


# ---------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------
def abi_errors_case(be):
    from openp5_amd.model import _ptr
    dv = be.device
    B, S, K1, Ts, Tg = 2, 2, 3, 5, 4
    seq = torch.zeros(B * S * K1, Ts, dtype=torch.int64, device=dv)
    lab = torch.zeros(B, Tg, dtype=torch.int64, device=dv)
    i64 = torch.zeros(B * (S * K1 + 1) * 4, dtype=torch.int64, device=dv)
    f32 = torch.zeros(2048, dtype=torch.float32, device=dv)
    i32 = torch.zeros(64, dtype=torch.int32, device=dv)
    lib = be.lib

    def call(S=S, K1=K1, Ts=Ts, est=1, seq_=seq, out=f32, tlp=None, old=None, pert=f32):
        return lib.p5_policy_slate_batch(_ptr(seq_), _ptr(f32), _ptr(pert), _ptr(lab), _ptr(lab), None, _ptr(tlp), B, S, K1, Ts, Tg, est, 1.0, 1.0, 0, 1, PAD,
                                         EOS, _ptr(i64), _ptr(i64), _ptr(out), _ptr(f32), _ptr(f32), _ptr(f32), _ptr(f32), _ptr(f32), _ptr(f32), _ptr(old),
                                         _ptr(i32) if old is not None else None, None, 0, 0, be.stream_ptr())
    assert call() == 0
    sync(be)
    for kw, msg in ((dict(K1=1), b"K1 >= 2"), (dict(S=512, K1=3), b"S * K1 <= 1024"), (dict(S=1, K1=1025), b"S * K1 <= 1024"), (dict(Ts=1), b"Ts >= 2"),
                    (dict(est=2), b"unknown estimator"), (dict(est=-1), b"unknown estimator"), (dict(K1=2, est=1), b"normalized estimator needs K >= 2"),
                    (dict(seq_=None), b"null input pointer"), (dict(pert=None), b"null input pointer"), (dict(out=None), b"null output pointer"),
                    (dict(tlp=f32), b"go together"), (dict(S=0), b"S >= 1")):
        assert call(**kw) != 0, kw
        assert msg in lib.p5_last_error(), (kw, lib.p5_last_error())
    assert call(K1=2, est=0) == 0 and call(tlp=f32, old=f32) == 0
    sync(be)


def model_errors_case(be, ocfg, items):
    """every refusal of policy_slate_batch / policy_step(slate_size=...) / policy_collect(slate_size=...) is a ValueError raised before anything
    is sampled or launched"""
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    ct = rank_cases.compiled(items)
    calls = []
    for name in ("_workspace", "_lane_workspace", "sample_items", "sample_slates", "_sample"):
        real = getattr(m, name)
        setattr(m, name, (lambda real_, name_: lambda *a, **k: calls.append(name_) or real_(*a, **k))(real, name))
    B, S, K, T = 2, 2, 2, 6
    ids, ww, mask, labels, out_attn = cases.synth_batch(ocfg, B, 8, T, 3)
    R = B * S * (K + 1)
    sampled = dict(sequences=torch.zeros(R, 7, dtype=torch.int64), sequences_logprob=torch.zeros(R), perturbed=torch.zeros(B, S, K + 1),
                   token_logprobs=torch.zeros(R, 6))

    def sb(match, sampled_=sampled, labels_=labels, attn_=out_attn, K_=K, S_=S, **kw):
        with pytest.raises(ValueError, match=match):
            m.policy_slate_batch(sampled_, labels_, attn_, K_, S_, **kw)

    def ps(match, labels_=labels, attn_=out_attn, S_=S, K_=K, fn="policy_step", **kw):
        with pytest.raises(ValueError, match=match):
            getattr(m, fn)(ids, ww, mask, labels_, attn_, kw.pop("trie", ct), S_, slate_size=K_, **kw)
    for f in (sb, ps):
        f("slate_size", K_=0)
        f("slate_size", K_=1.5)
        f("num_samples", S_=0)
        f("slate_estimator", **({"estimator": "median"} if f is sb else {"slate_estimator": "median"}))
        f("normalized.*slate_size >= 2", K_=1, **({"sampled_": {k: v[:B * S * 2] for k, v in sampled.items()}} if f is sb else {}))
        f("policy_coef", policy_coef=float("nan"))
        f("output_attention", attn_=out_attn[:, :-1])
        f(r"labels.*\[B, T\]", labels_=labels[:1], attn_=out_attn[:1])
        f("1024 slots", S_=400)
    sb("sampled", sampled_=None)
    sb("sequences", sampled_=dict(sampled, sequences=sampled["sequences"][:5]))
    sb("perturbed", sampled_=dict(sampled, perturbed=torch.zeros(B, S, K)))
    sb("rewards", rewards=torch.zeros(B, S, K))
    sb("token_logprobs", sampled_=dict(sampled, token_logprobs=torch.zeros(R, 5)), with_old_logprobs=True)
    sb(r"G \* T <= 512", sampled_=dict(sequences=torch.zeros(B * 37 * 3, 8, dtype=torch.int64), sequences_logprob=torch.zeros(B * 37 * 3),
                                       perturbed=torch.zeros(B, 37, 3)), S_=37)                    # G * To = 75 * 7
    for fn in ("policy_step", "policy_collect"):
        ps(r"G \* T <= 512", S_=37, fn=fn)                                                          # the trie's depth decides To
        trunc = "top_k / top_p" + (".*plain step" if fn == "policy_step" else "")          # (policy_collect: the clipped objective refuses it first)
        ps(trunc, top_k=2, fn=fn)
        ps(trunc, top_p=0.5, fn=fn)
        ps("baseline.*slate_estimator", baseline="mean", fn=fn)
        ps("baseline.*slate_estimator", baseline="none", fn=fn)
        ps("DAG.*plain step", trie=_grafted(items), fn=fn)
    ps("trie", trie=None)
    ps("ref_model", kl_coef=0.1)
    # (the kernel's 1024 slots are fewer than the sampler's SLATE_MAX_K today: both limits are lowered to be reached)
    wide, m.wide_max_rows = m.wide_max_rows, 2
    try:
        ps("wide_max_rows", K_=2)
    finally:
        m.wide_max_rows = wide
    m.SLATE_MAX_K = 2
    try:
        ps("SLATE_MAX_K", K_=2)
    finally:
        del m.SLATE_MAX_K
    assert not calls, f"a refused call reached the sampler or the engine: {calls}"


def _grafted(items):
    """a trie with an appended trie: a DAG, which the slate sampler refuses"""
    from openp5_amd.trie import Trie
    bos = 61
    t = Trie([list(it[:4]) + [bos] for it in items])
    t.append(Trie([list(it[4:]) for it in items]), bos)
    return t


# ---------------------------------------------------------------------------------------------------------
# 7. it learns
# ---------------------------------------------------------------------------------------------------------
LEARN_MARGIN = 0.5       # a third of the rise observed on the host emulation (see learns_case)


def learns_case(be, ocfg, steps=pc.LEARN_STEPS, B=4, S=2, K=4, L=10, lr=3e-5):
    """REINFORCE from slates alone (sft_coef 0, normalized, the hit reward, token_sum) on the 8-item trie: the mean trie-normalised
    log-probability of the gold items rises.  Observed on the host emulation (20 steps, B = 4, S = 2, K = 4, lr 3e-5): -2.9623 -> -1.4154, a
    rise of 1.55; LEARN_MARGIN asks for about a third of it, and the step is bit-reproducible.  Returns (before, after)."""
    from openp5_amd.optim import FusedAdamW
    items = cases.make_items(8, 5, hi=60)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = pc.policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    opt = FusedAdamW(m, lr=lr, weight_decay=0.0, max_grad_norm=1.0)
    before = pc._gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    for step in range(steps):
        m.policy_step(ids, ww, mask, labels, out_attn, ct, S, policy_coef=1.0, sft_coef=0.0, token_sum=True, seed=1000 + step, slate_size=K,
                      slate_estimator="normalized")
        opt.step()
        m.zero_grad()
    sync(be)
    after = pc._gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    print(f"[slate learns] gold log-probability {before:.4f} -> {after:.4f} after {steps} steps; last stats {m.last_policy_stats.cpu().tolist()}")
    return before, after


# ---------------------------------------------------------------------------------------------------------
# 8. the runner
# ---------------------------------------------------------------------------------------------------------
SLATE_FLAGS = ("--train_item_loss", "1", "--train_policy_samples", "2", "--policy_slate_size", "2")


def runner_case(be, tmp, caplog=None):
    """a short run with --policy_slate_size 2 completes and logs the slate statistics; the flags are checked at construction"""
    import logging
    runner, model, tok, args = pc._pipeline(be, tmp, "on", SLATE_FLAGS + ("--epochs", "1", "--logging_step", "2", "--policy_slate_estimator", "unbiased"))
    seen, drawn = [], []
    real, real_s = model.policy_step, model.sample_slates
    model.policy_step = lambda *a, **k: seen.append(k) or real(*a, **k)
    model.sample_slates = lambda *a, **k: drawn.append(k) or real_s(*a, **k)
    model.sample_items = lambda *a, **k: pytest.fail("sample_items called with --policy_slate_size on")
    if caplog is not None:
        caplog.set_level(logging.INFO)
    losses = runner.train()
    assert len(losses) == 1 and math.isfinite(losses[0])
    assert seen and all(k["num_samples"] == 2 and k["slate_size"] == 2 and k["slate_estimator"] == "unbiased" and k["trie"] is not None for k in seen)
    assert len({k["seed"] for k in seen}) == len(seen), "every step draws with its own seed"
    assert drawn and all(k["slate_size"] == 3 and k["num_slates"] == 2 for k in drawn)
    st = model.last_policy_stats.cpu()
    assert st.shape == (8,) and bool(torch.isfinite(st).all()) and float(st[6]) == 0 and float(st[7]) >= 1.0
    assert model.last_policy_batch["importance"].shape[1:] == (2, 2)
    if caplog is not None:
        assert any("policy slate step" in r.getMessage() and "ess_mean" in r.getMessage() and "weight_sum_mean" in r.getMessage() for r in caplog.records)
    S2 = ("--train_item_loss", "1", "--train_policy_samples", "2")
    for flags, match in ((("--policy_slate_size", "2"), "train_policy_samples > 0"),
                         (("--train_policy_samples", "2", "--policy_slate_size", "2"), "train_item_loss 1"),
                         (S2 + ("--policy_slate_size", "2", "--item_loss_top_k", "3"), "item_loss_top_k"),
                         (S2 + ("--policy_slate_size", "2", "--item_loss_top_p", "0.9"), "item_loss_top_p"),
                         (S2 + ("--policy_slate_size", "1"), "policy_slate_size >= 2"),
                         (S2 + ("--policy_slate_size", "2", "--policy_baseline", "grpo"), "policy_baseline"),
                         (S2 + ("--policy_slate_size", "-1"), "policy_slate_size")):
        with pytest.raises(ValueError, match=match):
            pc._pipeline(be, tmp, "bad", flags)
    # one slate per user is enough (no leave-one-out over draws), and slates of one item take the unbiased estimator
    pc._pipeline(be, tmp, "one", ("--train_item_loss", "1", "--train_policy_samples", "1", "--policy_slate_size", "1", "--policy_slate_estimator", "unbiased"))


def runner_resume_case(be, tmp):
    """a run interrupted at a --save_steps checkpoint and resumed ends with the weights of the uninterrupted one: the slates come back"""
    flags = SLATE_FLAGS + ("--epochs", "1")

    def build(name, extra=()):
        runner, model, _, _ = pc._pipeline(be, tmp, name, flags + tuple(extra), dropout=0.1)
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
    """with --policy_slate_size 0 (or absent) the calls that reach the model are the parent's: policy_step without a slate keyword, never
    sample_slates"""
    seen = {}
    for name, flags in (("absent", pc.POLICY_FLAGS), ("zero", pc.POLICY_FLAGS + ("--policy_slate_size", "0", "--policy_slate_estimator", "unbiased"))):
        runner, model, _, _ = pc._pipeline(be, tmp, name, flags + ("--epochs", "1"))
        calls = []
        real = model.policy_step
        model.policy_step = lambda *a, **k: calls.append((len(a), sorted(k), k["num_samples"], k["baseline"])) or real(*a, **k)
        model.sample_slates = lambda *a, **k: pytest.fail("sample_slates called with the flag off")
        model.policy_slate_batch = lambda *a, **k: pytest.fail("policy_slate_batch called with the flag off")
        runner.train()
        seen[name] = (calls, model._flat.detach().cpu().clone())
    assert seen["absent"][0] and all("slate_size" not in c[1] and "slate_estimator" not in c[1] for c in seen["absent"][0])
    assert seen["zero"][0] == seen["absent"][0] and torch.equal(seen["zero"][1], seen["absent"][1])
