"""Cases of the on-policy fine-tuning step (csrc/p5_policy.h, p5_policy_batch, P5T5Native.policy_batch / policy_step, the runner's
--train_policy_samples), shared by tests/test_policy_emu.py (host emulation) and tests/test_gpu_policy.py (MI355X).

1. the kernel through the C ABI against `ref_policy_batch`, a numpy float64 restatement: labels, masks and hit rewards exactly; advantages,
   weights and stats within KERNEL_TOL(S) = 4 (S + 8) 2^-24 of the reference, relative to the user's largest reference magnitude (the fp32
   rounding of a sum of S terms, a handful of multiplies and one divide); twice, the same bits.
2. errors: the C entry's refusals name their cause; the model's are ValueErrors raised before anything is sampled or launched.
3. composition: policy_step(seed=s) == sample_items(seed=s) -> policy_batch -> loss_and_backward on a fresh model, bit for bit.
4. meaning: the loss and the gradients against the formula evaluated in float64 on the oracle's item NLL of the replicated batch.
5. it learns: a few dozen steps raise the trie-normalised log-probability of the gold items; both coefficients 0 leave the weights alone.
6. the runner's flags."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases
from tests import multi_target_cases as mt
from tests import trie_loss_cases as tl
from tests.cases import sync

PAD, EOS = 0, 1
BASELINES = {"none": 0, "mean": 1, "loo": 2, "grpo": 3}


def KERNEL_TOL(S):
    return 4.0 * (S + 8) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------
def draw_length(row):
    """tokens of a drawn row (without the decoder start): through the first </s>; without one, in front of the first pad"""
    for i, t in enumerate(row):
        if t == EOS:
            return i + 1
        if t == PAD:
            return i
    return len(row)


def ref_policy_batch(seq, labels, attn, rewards, S, baseline, policy_coef, sft_coef, token_sum, adv_eps, with_gold):
    """numpy float64 restatement of p5_policy_batch: dict of labels / output_attention int64 [B, G, To], rewards / advantages [B, S], weights
    [B, G], hits bool [B, S], stats [8] (all float64)"""
    seq, labels, attn = np.asarray(seq), np.asarray(labels), np.asarray(attn)
    B, Ts, Tg = seq.shape[0] // S, seq.shape[1], labels.shape[1]
    G, To = S + with_gold, max(Tg, Ts - 1)
    lab_o = np.zeros((B, G, To), np.int64)
    att_o = np.zeros((B, G, To), np.int64)
    r = np.zeros((B, S), np.float64)
    A = np.zeros((B, S), np.float64)
    w = np.zeros((B, G), np.float64)
    hits = np.zeros((B, S), bool)
    n = np.zeros((B, S), np.int64)
    for b in range(B):
        attended = (attn[b] != 0) & (np.cumsum(labels[b] == -100) == 0)          # a -100 ends the gold: the engine scores nothing at it and behind it
        gold = [int(t) for t in labels[b][attended]]
        if with_gold:
            lab_o[b, 0, :Tg] = labels[b]
            att_o[b, 0, :Tg] = attended
            w[b, 0] = np.float64(np.float32(sft_coef)) * G
        for s in range(S):
            row = [int(t) for t in seq[b * S + s, 1:]]
            k = draw_length(row)
            n[b, s] = k
            lab_o[b, with_gold + s, :k] = row[:k]
            att_o[b, with_gold + s, :k] = 1
            hits[b, s] = k > 0 and row[:k] == gold
            if k > 0:
                r[b, s] = float(rewards[b, s]) if rewards is not None else float(hits[b, s])
        ex = n[b] > 0
        Se = int(ex.sum())
        if Se == 0:
            continue
        re = r[b][ex]
        if baseline == "none":
            a = re.copy()
        elif bool((re == re[0]).all()) or Se == 1:       # equal rewards (and a lone draw under mean / loo / grpo): exactly 0
            a = np.zeros(Se)
        elif baseline == "mean":
            a = re - re.mean()
        elif baseline == "loo":
            a = re - (re.sum() - re) / (Se - 1)
        else:
            a = (re - re.mean()) / (re.std() + np.float64(np.float32(adv_eps)))
        A[b][ex] = a
        w[b, with_gold:] = np.float64(np.float32(policy_coef)) * A[b] * G / S * (n[b] if token_sum else 1)
    N = max(int((n > 0).sum()), 1)
    signal = [(n[b] > 0).any() and not bool((r[b][n[b] > 0] == r[b][n[b] > 0][0]).all()) for b in range(B)]
    stats = np.array([r.sum() / N, np.mean(signal), np.abs(A).sum() / N, hits.sum() / N, np.mean(hits.any(axis=1)), float(((n > 0).sum(axis=1) == 0).sum()),
                      0.0, 0.0])
    return dict(labels=lab_o, output_attention=att_o, rewards=r, advantages=A, weights=w, hits=hits, stats=stats, n=n)


# ---------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------
KERNEL_S = (1, 2, 3, 16, 65)                     # one draw, loo's edge, a few, more than a thread's first pass needs ... 65: past one wave
KERNEL_SHAPES = ((3, 6), (5, 6), (8, 6))         # (Tg, Ts): Tg < Ts - 1, Tg == Ts - 1, Tg > Ts - 1


def kernel_combos():
    """(S, baseline, given rewards?) -- each runs every (Tg, Ts) x with_gold x token_sum x B in {1, 5}"""
    out = []
    for S in KERNEL_S:
        for baseline in ("none", "mean", "loo", "grpo"):
            if baseline == "loo" and S < 2 or baseline == "grpo" and S < 2:
                continue
            for given in (False, True):
                out.append((S, baseline, given))
    return out


def kernel_problem(B, S, Tg, Ts, given, seed):
    """sequences [B*S, Ts], labels / attn [B, Tg], rewards [B, S] or None.  Every user's gold has 3 attended tokens (a, b, </s>); when Tg == 3
    and the user's gold carries -100 labels it is [a, -100, </s>] under attention 1, whose one attended token is a: the -100 ends it.  User b:
      b % 5 == 0  draw 0 IS the gold, draw 1 the gold's prefix but longer, draw 2 shorter, draw 4 (if any) an empty slot, the rest random
                  (one of them without </s>: cut by the length limit)
      b % 5 == 1  all-pad sequences: nothing drawn
      b % 5 == 2  no draw hits and the given rewards are all 0.3: equal rewards
      b % 5 == 3  every draw is the gold: equal rewards of 1 (given: all -1.7); the gold's tail is labelled -100 under attention 1
      b % 5 == 4  as user 0 with the gold's unattended tail labelled -100
    With B == 1 the user is of kind 0."""
    g = np.random.default_rng(seed)
    seq = np.zeros((B * S, Ts), np.int64)
    labels = np.zeros((B, Tg), np.int64)
    attn = np.zeros((B, Tg), np.int64)
    rewards = (g.standard_normal((B, S)) * 1.5).astype(np.float32) if given else None
    if given and S >= 2:
        rewards[:, 0], rewards[:, 1] = 2.0, -2.0                       # (a spread grpo can divide by)
    room = Ts - 1
    for b in range(B):
        kind = b % 5
        a_, b_ = int(g.integers(3, 50)), int(g.integers(3, 50))
        gold = [a_, b_, EOS]
        if kind in (3, 4):
            if Tg > 3:
                labels[b, :3], labels[b, 3:] = gold, -100
                attn[b, :] = 1
            else:
                labels[b], attn[b] = [a_, -100, EOS], 1                 # attended tokens: (a) -- the -100 and what is behind it are not
                gold = [a_]
        else:
            labels[b, :3], attn[b, :3] = gold, 1
        for s in range(S):
            row = seq[b * S + s]
            if kind == 1:
                continue
            if kind == 3 or (kind in (0, 4) and s == 0):
                d = gold
            elif kind in (0, 4) and s == 1:
                d = gold[:-1] + [int(g.integers(3, 50)), EOS]
            elif kind in (0, 4) and s == 2:
                d = gold[:1] + [EOS]
            elif kind in (0, 4) and s == 4:
                continue
            elif kind in (0, 4) and s == 5:
                d = [int(t) for t in g.integers(50, 60, room)]          # no </s>
            else:
                d = [int(t) for t in g.integers(50, 60, int(g.integers(0, room)))] + [EOS]       # (tokens the golds do not use: no hit)
            row[1:1 + len(d)] = d
        if given and kind == 2:
            rewards[b] = 0.3
        if given and kind == 3:
            rewards[b] = -1.7
    return seq, labels, attn, rewards


def run_policy_abi(be, seq, labels, attn, rewards, S, baseline, policy_coef, sft_coef, token_sum, adv_eps, with_gold):
    from openp5_amd.model import _ptr
    dv = be.device
    B, Ts, Tg = seq.shape[0] // S, seq.shape[1], labels.shape[1]
    G, To = S + with_gold, max(Tg, Ts - 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dv)       # noqa: E731
    d_seq, d_lab, d_att = t(seq), t(labels), t(attn)
    d_rew = None if rewards is None else t(rewards)
    lab_o = torch.full((B, G, To), -7, dtype=torch.int64, device=dv)
    att_o = torch.full((B, G, To), -7, dtype=torch.int64, device=dv)
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dv)      # noqa: E731
    r_o, a_o, w_o, us, st = f(B, S), f(B, S), f(B, G), f(B, 4), f(8)
    rc = be.lib.p5_policy_batch(_ptr(d_seq), _ptr(d_lab), _ptr(d_att), _ptr(d_rew), B, S, Ts, Tg, BASELINES[baseline], policy_coef, sft_coef, int(token_sum),
                                adv_eps, with_gold, PAD, EOS, _ptr(lab_o), _ptr(att_o), _ptr(r_o), _ptr(a_o), _ptr(w_o), _ptr(us), _ptr(st), be.stream_ptr())
    be.check(rc, "p5_policy_batch")
    sync(be)
    return dict(labels=lab_o.cpu().numpy(), output_attention=att_o.cpu().numpy(), rewards=r_o.cpu().numpy(), advantages=a_o.cpu().numpy(),
                weights=w_o.cpu().numpy(), stats=st.cpu().numpy())


def _assert_close(got, ref, tol, what):
    """per user (row): |got - ref| <= tol * the row's largest reference magnitude"""
    got, ref = np.asarray(got, np.float64).reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    assert np.isfinite(got).all(), what
    scale = np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(got - ref)
    assert (err <= tol * scale).all(), (what, float((err / np.maximum(scale, 1e-300)).max()), tol)


def kernel_case(be, S, baseline, given, seed=0):
    policy_coef, sft_coef = 0.7, 1.3
    tol = KERNEL_TOL(S)
    seen_hit = seen_equal = False
    # grpo also at adv_eps = 0: equal rewards must still give exact zeros (0 / 0 is not formed), never NaN
    for (Tg, Ts), with_gold, token_sum, B, adv_eps in itertools.product(KERNEL_SHAPES, (0, 1), (0, 1), (1, 5), (1e-6, 0.0) if baseline == "grpo" else (1e-6,)):
        tag = f"S={S} {baseline} given={given} Tg={Tg} Ts={Ts} gold={with_gold} sum={token_sum} B={B} eps={adv_eps}"
        seq, labels, attn, rewards = kernel_problem(B, S, Tg, Ts, given, seed + 17 * Tg + B)
        ref = ref_policy_batch(seq, labels, attn, rewards, S, baseline, policy_coef, sft_coef, token_sum, adv_eps, with_gold)
        if baseline == "grpo":          # the reference alone: the division must not amplify beyond the bound
            for b in range(B):
                ex = ref["n"][b] > 0
                if ex.any():
                    sd, top = ref["rewards"][b][ex].std(), np.abs(ref["rewards"][b][ex]).max()
                    assert sd == 0.0 or sd >= 0.1 * top, (tag, b, sd, top)
        runs = [run_policy_abi(be, seq, labels, attn, rewards, S, baseline, policy_coef, sft_coef, token_sum, adv_eps, with_gold) for _ in range(2)]
        for k, v in runs[0].items():
            assert v.tobytes() == runs[1][k].tobytes(), f"{tag}: two runs differ in {k}"
        got = runs[0]
        assert np.array_equal(got["labels"], ref["labels"]), tag
        assert np.array_equal(got["output_attention"], ref["output_attention"]), tag
        if rewards is None:
            assert np.array_equal(got["rewards"], ref["hits"].astype(np.float32)), tag
        else:
            assert np.array_equal(got["rewards"], ref["rewards"].astype(np.float32)), tag
        _assert_close(got["advantages"], ref["advantages"], tol, tag + " advantages")
        _assert_close(got["weights"], ref["weights"], tol, tag + " weights")
        top = max(1.0, float(np.abs(ref["rewards"]).max()), float(np.abs(ref["advantages"]).max()))
        assert np.isfinite(got["stats"]).all() and (np.abs(got["stats"] - ref["stats"]) <= tol * top).all(), (tag, got["stats"], ref["stats"])
        assert got["stats"][5] == ref["stats"][5] and got["stats"][6] == 0 and got["stats"][7] == 0
        if baseline != "none":
            for b in range(B):
                ex = ref["n"][b] > 0
                if ex.any() and bool((ref["rewards"][b][ex] == ref["rewards"][b][ex][0]).all()):
                    seen_equal = True
                    assert (got["advantages"][b] == 0.0).all() and (got["weights"][b, with_gold:] == 0.0).all(), (tag, b, got["advantages"][b])
        seen_hit = seen_hit or bool(ref["hits"].any())
        if B == 5:
            assert ref["stats"][5] == 1 and (ref["output_attention"][1, with_gold:] == 0).all()
            if S >= 3 and Ts - 1 >= 4:
                assert ref["hits"][0, 0] and not ref["hits"][0, 1] and not ref["hits"][0, 2], tag       # the gold; its prefix but longer; shorter
    assert seen_hit and (seen_equal or baseline == "none")


# ---------------------------------------------------------------------------------------------------------
# 2. errors
# ---------------------------------------------------------------------------------------------------------
def abi_errors_case(be):
    from openp5_amd.model import _ptr
    dv = be.device
    B, S, Ts, Tg = 2, 2, 5, 4
    seq = torch.zeros(B * S, Ts, dtype=torch.int64, device=dv)
    lab = torch.zeros(B, Tg, dtype=torch.int64, device=dv)
    i64 = torch.zeros(B * (S + 1) * 4, dtype=torch.int64, device=dv)
    f32 = torch.zeros(64, dtype=torch.float32, device=dv)
    lib = be.lib

    def call(S=S, baseline=2, pc=1.0, sc=1.0, eps=1e-6, seq_=seq, out=f32):
        return lib.p5_policy_batch(_ptr(seq_), _ptr(lab), _ptr(lab), None, B, S, Ts, Tg, baseline, pc, sc, 0, eps, 1, PAD, EOS, _ptr(i64), _ptr(i64), _ptr(out),
                                   _ptr(f32), _ptr(f32), _ptr(f32), _ptr(f32), be.stream_ptr())
    assert call() == 0
    sync(be)
    for kw, msg in ((dict(S=0), b"S >= 1"), (dict(S=1), b"loo"), (dict(baseline=4), b"unknown baseline"), (dict(baseline=-1), b"unknown baseline"),
                    (dict(pc=float("nan")), b"non-finite"), (dict(sc=float("inf")), b"non-finite"), (dict(seq_=None), b"null input pointer"),
                    (dict(out=None), b"null output pointer"), (dict(S=1025, baseline=0), b"S <= 1024")):
        assert call(**kw) != 0, kw
        assert msg in lib.p5_last_error(), (kw, lib.p5_last_error())
    assert call(S=1, baseline=1) == 0
    sync(be)


def model_errors_case(be, ocfg, items):
    """every refusal of policy_batch / policy_step is a ValueError raised before anything is sampled or launched"""
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    ct = rank_cases.compiled(items)
    calls = []
    for name in ("_workspace", "_lane_workspace", "sample_items", "_sample"):
        real = getattr(m, name)
        setattr(m, name, (lambda real_, name_: lambda *a, **k: calls.append(name_) or real_(*a, **k))(real, name))
    real_pb = be.lib.p5_policy_batch
    B, S, T = 2, 3, 6
    ids, ww, mask, labels, out_attn = cases.synth_batch(ocfg, B, 8, T, 3)
    seq = torch.zeros(B * S, 7, dtype=torch.int64)

    def pb(match, seq_=seq, labels_=labels, attn_=out_attn, S_=S, **kw):
        with pytest.raises(ValueError, match=match):
            m.policy_batch(seq_, labels_, attn_, S_, **kw)

    def ps(match, labels_=labels, attn_=out_attn, S_=S, **kw):
        with pytest.raises(ValueError, match=match):
            m.policy_step(ids, ww, mask, labels_, attn_, kw.pop("trie", ct), S_, **kw)
    for f in (pb, ps):
        f("num_samples", S_=0)
        f("num_samples", S_=2.5)
        f("baseline", baseline="median")
        f("loo", S_=1, **({"seq_": seq[:2]} if f is pb else {}))
        f("policy_coef", policy_coef=float("nan"))
        f("sft_coef", sft_coef=float("inf"))
        f("output_attention", attn_=out_attn[:, :-1])
        f(r"labels.*\[B, T\]", labels_=labels[:1], attn_=out_attn[:1])
    pb("adv_eps", adv_eps=-1.0)
    pb("sequences", seq_=seq[:5])
    pb("sequences", seq_=seq.view(-1))
    pb("rewards", rewards=torch.zeros(B, S + 1))
    pb(r"G \* T <= 512", seq_=torch.zeros(B * 73, 8, dtype=torch.int64), S_=73)                 # G * To = 74 * 7 = 518
    ps(r"G \* T <= 512", S_=102)                                                                  # the trie's depth decides To: 103 * 6 > 512
    ps("trie", trie=None)
    ps("top_k", top_k=-1)
    ps("top_p", top_p=0.0)
    ps("item_head", item_head="sparse")
    ps("top_k / top_p", entropy_coef=0.1, top_k=2)
    ps("ref_model", kl_coef=0.1)
    ps("finite", entropy_coef=float("nan"))
    assert not calls, f"a refused call reached the sampler or the engine: {calls}"
    assert be.lib.p5_policy_batch is real_pb


# ---------------------------------------------------------------------------------------------------------
# 3. composition
# ---------------------------------------------------------------------------------------------------------
def policy_inputs(ocfg, items, B, L, seed=tl.MODEL_SEED):
    """inputs of cases.synth_batch and every user's gold: an item of the trie behind the decoder start, pad-filled"""
    T = max(len(q) for q in items) - 1
    ids, ww, mask, labels, out_attn, pick = tl.item_batch(ocfg, items, B, L, T, seed, stray=False)
    return ids, ww, mask, labels, out_attn, pick


def index_reward(drawn):
    """a reward with signal whatever was drawn: a fixed function of the drawn item's index"""
    return (drawn["item_index"] * 7 % 5).to(torch.float32) - 1.5


def composition_case(be, ocfg, items, dtype="fp32", item_head="dense", dropout=0.0, reg=False, B=3, L=12, S=4, baseline="loo", seed=11, reward_fn=None,
                     **kw):
    """policy_step(seed=s) against its three parts on a fresh model with the same weights: loss and gradient arena bit for bit"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = policy_inputs(ocfg, items, B, L)
    excluded_items = [[i for i in range(b, len(items), 3)] if b != 1 else [] for b in range(B)]
    common = dict(temperature=0.8, excluded_items=excluded_items, item_head=item_head)
    regkw, ref = {}, None
    res = []
    for whole in (True, False):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        tl._train_mode(m, dropout, 77)
        if reg:
            ref = m.frozen_copy()
            with torch.no_grad():
                ref._flat.mul_(1.01)          # (a reference that is not the policy: KL > 0)
            ref.mark_params_updated()
            regkw = dict(entropy_coef=0.05, kl_coef=0.2)
        if whole:
            loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, S, baseline=baseline, seed=seed, ref_model=ref, reward_fn=reward_fn, **regkw, **common,
                                     **kw)
            assert m.last_policy_stats.shape == (8,) and m.last_policy_batch["labels"].shape[:2] == (B, S + (kw.get("sft_coef", 1.0) != 0.0))
        else:
            out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=0.8, excluded_items=excluded_items,
                                 seed=seed)
            pb = m.policy_batch(out["sequences"], labels, out_attn, S, rewards=None if reward_fn is None else reward_fn(out), baseline=baseline, **kw)
            if reg:
                regkw["ref_logits"] = ref.item_logits(ids, ww, mask, pb["labels"], ct, temperature=0.8, excluded_items=excluded_items, item_head=item_head)
            loss = m.loss_and_backward(ids, ww, mask, pb["labels"], pb["output_attention"], trie=ct, target_weights=pb["target_weights"], **regkw, **common)
        sync(be)
        res.append((loss.detach().cpu().clone(), m._grads.detach().cpu().clone()))
    (l0, g0), (l1, g1) = res
    assert math.isfinite(float(l0)) and float(g0.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(g0, g1), (float(l0), float(l1), float((g0 - g1).abs().max()))


# ---------------------------------------------------------------------------------------------------------
# 4. meaning
# ---------------------------------------------------------------------------------------------------------
def meaning_case(be, ocfg, items, B=3, L=12, S=3, policy_coef=0.7, sft_coef=1.3, token_sum=False, seed=5):
    """fp32, baseline "mean": loss == sft_coef mean_b l(gold_b) + policy_coef mean_b (1/S) sum_s A_bs l_bs in float64 from the oracle's item NLL
    of the replicated batch, with A from the float64 reference of the kernel; gradients == its autograd (the tolerances of
    multi_target_cases._check: NLL 2e-5, gradients 2e-4 with the 1 % floor)"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    tau = 0.8
    loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, S, temperature=tau, baseline="mean", policy_coef=policy_coef, sft_coef=sft_coef,
                         token_sum=token_sum, reward_fn=index_reward, seed=seed)
    sync(be)
    pb = m.last_policy_batch
    # the reference's inputs do not pass through the kernel: the same draws from a second model with the same weights, rewarded here
    m2 = cases.build_model(be, ocfg, params, "fp32")
    m2.eval()
    drawn = m2.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=tau, seed=seed)
    seq, rew = drawn["sequences"].cpu().numpy(), index_reward(drawn).cpu().numpy()
    ref = ref_policy_batch(seq, labels.numpy(), out_attn.numpy(), rew, S, "mean", policy_coef, sft_coef, token_sum, 1e-6, 1)
    assert np.array_equal(ref["labels"], pb["labels"].cpu().numpy()) and float(np.abs(ref["advantages"]).max()) > 0
    G, To = S + 1, ref["labels"].shape[2]
    Pq = mt._oracle_params(params, "bf16")          # (float64)
    glab = torch.from_numpy(ref["labels"])
    nll_o, _, _ = tl.oracle_item_nll(Pq, ocfg, mt.rep(ids, G), mt.rep(ww, G), mt.rep(mask, G), glab.view(B * G, To), ct, tau, None)
    msk = torch.from_numpy(ref["output_attention"]).double()
    tok = (nll_o.view(B, G, To) * msk).sum(2)
    per = tok if token_sum else tok / msk.sum(2).clamp(min=1)
    per_gold = tok[:, 0] / msk[:, 0].sum(1).clamp(min=1)
    A = torch.from_numpy(ref["advantages"])
    loss_o = sft_coef * per_gold.mean() + policy_coef * ((A * per[:, 1:]).sum(1) / S).mean()
    loss_o.backward()
    lo = float(loss_o.detach())
    _, worst = mt._fp32_errors(m, Pq, nll_o, nll_o)
    print(f"[policy meaning token_sum={token_sum}] loss {float(loss):.6f} oracle {lo:.6f}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert abs(float(loss) - lo) <= mt.NLL_TOL * max(1.0, abs(lo)), (float(loss), lo)
    assert worst[0] <= mt.GRAD_TOL, worst


# ---------------------------------------------------------------------------------------------------------
# 5. it learns
# ---------------------------------------------------------------------------------------------------------
LEARN_STEPS = 20


def _gold_logprob(m, ids, ww, mask, labels, out_attn, ct):
    m.eval()
    with torch.no_grad():
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct)["loss"]
    B, T = labels.shape
    return -float((nll.view(B, T).cpu() * (out_attn != 0)).sum(1).mean())


def learns_case(be, ocfg, steps=LEARN_STEPS, B=4, S=8, L=10, lr=3e-5):
    """REINFORCE alone (sft_coef 0, policy_coef 1, loo, the hit reward) on a trie of 8 items: the mean trie-normalised log-probability of the
    gold items rises.  The learning rate is small because AdamW moves every parameter of this tiny model by lr per step whatever the
    gradient's size: at 3e-4 the two users that hit first are learnt within three steps and drag the other two users' gold items down
    with them (-2.96 -> -4.49 after 40 steps; 3e-3: -5.91), at 3e-5 all four users find their item.  Returns (before, after)."""
    from openp5_amd.optim import FusedAdamW
    items = cases.make_items(8, 5, hi=60)
    ct = rank_cases.compiled(items)
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn, _ = policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, params, "fp32")
    opt = FusedAdamW(m, lr=lr, weight_decay=0.0, max_grad_norm=1.0)
    before = _gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    for step in range(steps):
        m.policy_step(ids, ww, mask, labels, out_attn, ct, S, baseline="loo", policy_coef=1.0, sft_coef=0.0, seed=1000 + step)
        opt.step()
        m.zero_grad()
    sync(be)
    after = _gold_logprob(m, ids, ww, mask, labels, out_attn, ct)
    print(f"[policy learns] gold log-probability {before:.4f} -> {after:.4f} after {steps} steps; last stats {m.last_policy_stats.cpu().tolist()}")
    return before, after


def zero_coef_case(be, ocfg, steps=3, B=4, S=8, L=10):
    """policy_coef = sft_coef = 0 and weight decay 0: the weights do not move"""
    from openp5_amd.optim import FusedAdamW
    items = cases.make_items(8, 5, hi=60)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = policy_inputs(ocfg, items, B, L)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    opt = FusedAdamW(m, lr=3e-3, weight_decay=0.0, max_grad_norm=1.0)
    w0 = m._flat.detach().cpu().clone()
    for step in range(steps):
        loss = m.policy_step(ids, ww, mask, labels, out_attn, ct, S, baseline="loo", policy_coef=0.0, sft_coef=0.0, seed=1000 + step)
        assert float(loss) == 0.0 and float(m._grads.abs().max()) == 0.0
        opt.step()
        m.zero_grad()
    sync(be)
    assert torch.equal(m._flat.detach().cpu(), w0)


# ---------------------------------------------------------------------------------------------------------
# 6. the runner
# ---------------------------------------------------------------------------------------------------------
def _pipeline(be, tmp, name, flags, dropout=0.0):
    from openp5_amd.model import P5ModelConfig
    tiny = P5ModelConfig(d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=2, dropout_rate=dropout)
    d = os.path.join(tmp, name)
    os.makedirs(d, exist_ok=True)
    return cases.make_pipeline(be, d, "fp32", dataset="Toy", n_users=8, n_items=16, n_inter=40, flags=["--batch_size", "8", "--lr", "3e-3"] + list(flags),
                               model_cfg=tiny, vocab=2400)


POLICY_FLAGS = ("--train_item_loss", "1", "--train_policy_samples", "4")


def runner_case(be, tmp, caplog=None):
    """a short run with --train_policy_samples 4 completes and logs the statistics; the flags are checked at construction"""
    import logging
    runner, model, tok, args = _pipeline(be, tmp, "on", POLICY_FLAGS + ("--epochs", "1", "--logging_step", "2", "--policy_baseline", "grpo"))
    seen = []
    real = model.policy_step
    model.policy_step = lambda *a, **k: seen.append(k) or real(*a, **k)
    if caplog is not None:
        caplog.set_level(logging.INFO)
    losses = runner.train()
    assert len(losses) == 1 and math.isfinite(losses[0])
    assert seen and all(k["num_samples"] == 4 and k["baseline"] == "grpo" and k["trie"] is not None for k in seen)
    assert len({k["seed"] for k in seen}) == len(seen), "every step draws with its own seed"
    st = model.last_policy_stats.cpu()
    assert st.shape == (8,) and bool(torch.isfinite(st).all()) and float(st[5]) == 0
    if caplog is not None:
        assert any("policy step" in r.getMessage() and "hit_rate" in r.getMessage() for r in caplog.records)
    for flags, match in ((("--train_policy_samples", "4"), "train_item_loss 1"), (POLICY_FLAGS[:3] + ("1",), "loo"),
                         (POLICY_FLAGS[:3] + ("-2",), "train_policy_samples")):
        with pytest.raises(ValueError, match=match):
            _pipeline(be, tmp, "bad", flags)


def runner_resume_case(be, tmp):
    """a run interrupted at a --save_steps checkpoint and resumed ends with the weights of the uninterrupted one (dropout on: the draws,
    the dropout masks and the data order all come back)"""
    flags = POLICY_FLAGS + ("--epochs", "1")

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
    """with --train_policy_samples 0 (or absent) the calls that reach the model are those without the feature: loss_and_backward with the
    item loss's keywords alone, never policy_step"""
    seen = {}
    for name, flags in (("absent", ("--train_item_loss", "1")), ("zero", ("--train_item_loss", "1", "--train_policy_samples", "0", "--policy_coef", "3"))):
        runner, model, _, _ = _pipeline(be, tmp, name, flags + ("--epochs", "1"))
        calls = []
        real = model.loss_and_backward
        model.loss_and_backward = lambda *a, **k: calls.append((len(a), sorted(k))) or real(*a, **k)
        model.policy_step = lambda *a, **k: pytest.fail("policy_step called with the flag off")
        model.sample_items = lambda *a, **k: pytest.fail("sample_items called with the flag off")
        runner.train()
        seen[name] = (calls, model._flat.detach().cpu().clone())
    assert seen["absent"][0] and all(c == (5, ["temperature", "trie"]) for c in seen["absent"][0]), seen["absent"][0][:2]
    assert seen["zero"][0] == seen["absent"][0] and torch.equal(seen["zero"][1], seen["absent"][1])
