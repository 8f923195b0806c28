"""Cases of training on several targets per user with one encoder pass (`labels [B, G, T]`, p5_forward_targets / p5_forward_loss_targets),
shared by tests/test_multi_target_emu.py (host emulation) and tests/test_gpu_multi_target.py (MI355X).

The reference is the oracle on the REPLICATED batch: user b's inputs repeated G times, sample b * G + g carrying labels[b, g]
(`O.p5_forward_nll` / `trie_loss_cases.oracle_item_nll` + autograd), compared as `cases.model_train_case` compares (fp32: NLL 2e-5, every
gradient 2e-4 of the tensor's largest entry with the 1 % floor) or, for the bf16 engine, to `trie_loss_cases.BF16_BOUNDS`.  With dropout on
the replicated batch draws other masks than the tensors the engine forms, so the reference is `grouped_nll`: the decoder restated from the
oracle's own blocks on those tensors."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases, sample_cases
from tests import trie_loss_cases as tl
from tests.cases import sync

NLL_TOL, GRAD_TOL = tl.NLL_TOL, tl.GRAD_TOL

# (B, L, T, G), bf16 too?  -- the selection edges of csrc/p5_attn_tu.hip for Lq = G * T
SHAPES = [((3, 14, 5, 1), False),       # G = 1
          ((3, 14, 5, 3), True),        # G * T = 15 <= 16: the one-launch backward
          ((2, 14, 3, 6), True),        # 18
          ((2, 14, 5, 13), True),       # 65: the 8-wave forward
          ((2, 14, 5, 26), True),       # 130: past 128
          ((1, 130, 4, 33), True),      # 132: Lk > 128 and Lq > 128
          ((1, 14, 8, 64), False),      # 512: the query limit
          ((2, 32, 8, 4), True)]        # M = Md = 64: the deferred weight-gradient plan and the fused-norm route


def rep(t, G):
    return t.repeat_interleave(G, dim=0)


def grouped_batch(ocfg, B, L, T, G, seed=3):
    """inputs of cases.synth_batch (part of the encoder input of users >= 1 is masked) and labels / output_attention [B, G, T]: the targets
    of one user have different lengths, and one target (the last of user 0 when G > 1, else of the last user) is all-masked"""
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, T, seed)
    g = torch.Generator().manual_seed(seed + 101)
    labels = torch.randint(3, ocfg.vocab_size, (B, G, T), generator=g)
    out_attn = torch.ones(B, G, T, dtype=torch.long)
    for b in range(B):
        for k in range(G):
            n = 1 + (b + k) % T if T >= 2 else 1          # lengths cycle through 1 .. T within a user
            n = max(n, min(2, T))
            labels[b, k, n - 1] = ocfg.eos_id
            labels[b, k, n:] = 0
            out_attn[b, k, n:] = 0
    dead = (0, G - 1) if G > 1 else (B - 1, 0)
    if B * G > 1:
        out_attn[dead] = 0
    return ids, ww, mask, labels, out_attn


def _d(dp, x, site):
    return x if dp is None else dp.apply(x, site)


def grouped_nll(P, cfg, ids, ww, mask, labels, dp=None):
    """The grouped step restated from the oracle's blocks: the encoder on B users; the decoder's row sites on the flat [B*G*T, d] tensor,
    self-attention on [B*G, T, d] (probabilities [B*G, H, T, T]), cross-attention on [B, G*T, d] against the user's encoder output
    (probabilities [B, H, G*T, L]).  Returns the flat [B*G*T] NLL."""
    B, G, T = labels.shape
    enc = O.encoder_forward(P, cfg, ids, ww, mask, dp)
    x = _d(dp, P["shared.weight"][O.shift_right(labels.reshape(B * G, T), cfg)], O.site_id(1, 0, 0))
    neg = torch.finfo(x.dtype).min
    cmask = torch.where(torch.ones(T, T, dtype=torch.bool).tril(), torch.zeros((), dtype=x.dtype), torch.full((), neg, dtype=x.dtype))[None, None]
    sbias = O.compute_bias(P["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], T, T, False, cfg) + cmask
    xbias = (1.0 - mask[:, None, None, :].to(x.dtype)) * neg
    for i in range(cfg.num_decoder_layers):
        p = f"decoder.block.{i}"
        n = O.rmsnorm(x, P[p + ".layer.0.layer_norm.weight"], cfg.eps)
        x = x + _d(dp, O.attention(n, n, P, p + ".layer.0.SelfAttention", sbias, cfg, dp, O.site_id(1, i, 1)), O.site_id(1, i, 2))
        n = O.rmsnorm(x, P[p + ".layer.1.layer_norm.weight"], cfg.eps).reshape(B, G * T, -1)
        a = O.attention(n, enc, P, p + ".layer.1.EncDecAttention", xbias, cfg, dp, O.site_id(1, i, 3)).reshape(B * G, T, -1)
        x = x + _d(dp, a, O.site_id(1, i, 4))
        n = O.rmsnorm(x, P[p + ".layer.2.layer_norm.weight"], cfg.eps)
        x = x + _d(dp, O.ffn(n, P, p + ".layer.2", cfg, dp, O.site_id(1, i, 5)), O.site_id(1, i, 6))
    x = _d(dp, O.rmsnorm(x, P["decoder.final_layer_norm.weight"], cfg.eps), O.site_id(1, 0, 7))
    logits = O.lm_logits(P, cfg, x)
    return torch.nn.functional.cross_entropy(logits.view(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100, reduction="none")


def weighted_loss(nll, out_attn, w=None):
    """sum_{b,g} w[b,g] * (sum_t nll*m / max(sum_t m, 1)) / (B*G): O.runner_loss over the replicated batch when w = 1"""
    B, G, T = out_attn.shape
    m = (out_attn != 0).to(nll.dtype).to(nll.device)
    per = (nll.view(B, G, T) * m).sum(2) / m.sum(2).clamp(min=1)
    if w is not None:
        per = per * w.to(device=nll.device, dtype=nll.dtype)
    return per.sum() / (B * G)


def _fp32_errors(m, Pq, nll, nll_o):
    err = float((nll.detach().cpu().double() - nll_o.detach().double()).abs().max())
    gmax = max(float(v.grad.abs().max()) for v in Pq.values())
    worst = (0.0, "")
    for name, p in m.named_parameters():
        g_, go = p.grad.detach().cpu().double(), Pq[name].grad.double()
        worst = max(worst, (float((g_ - go).abs().max()) / (float(go.abs().max()) + 1e-2 * gmax + 1e-12), name))
    return err, worst


def _check(m, Pq, nll, nll_o, dtype, tag):
    if dtype == "fp32":
        err, worst = _fp32_errors(m, Pq, nll, nll_o)
        print(f"[multi target fp32 {tag}] nll err {err:.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
        assert err <= NLL_TOL, f"{tag}: nll err {err}"
        assert worst[0] <= GRAD_TOL, f"{tag}: gradient mismatch {worst}"
        return err, worst
    err = float((nll.detach().cpu().double() - nll_o.detach().double()).abs().max())
    rows, whole = cases.grad_agreement(m, Pq)
    r = dict(nll_max=err, worst_rel=max(rows), whole_rel=whole[0], whole_cos=whole[1])
    print(f"[multi target bf16 {tag}] {r}")
    bb = tl.BF16_BOUNDS
    assert r["nll_max"] <= bb["nll_max"] and r["worst_rel"][0] <= bb["worst_rel"] and r["whole_rel"] <= bb["whole_rel"] and r["whole_cos"] >= bb["whole_cos"], (tag, r)
    return r


def _oracle_params(params, dtype):
    return {k: (v.double() if dtype == "bf16" else v).clone().requires_grad_(True) for k, v in params.items()}


def shape_case(be, ocfg, shape, dtype="fp32"):
    """1. NLL and every parameter gradient of a grouped call against the oracle on the replicated batch"""
    B, L, T, G = shape
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = grouped_batch(ocfg, B, L, T, G)
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
    assert nll.shape == (B * G * T,)
    weighted_loss(nll, out_attn).backward()
    sync(be)
    Pq = _oracle_params(params, dtype)
    nll_o = O.p5_forward_nll(Pq, ocfg, rep(ids, G), rep(ww, G), rep(mask, G), labels.view(B * G, T))
    O.runner_loss(nll_o, out_attn.view(B * G, T)).backward()
    return _check(m, Pq, nll, nll_o, dtype, f"{shape}")


# ---------------------------------------------------------------------------------------------------------
# 2. G = 1 returns the existing bits
# ---------------------------------------------------------------------------------------------------------
def g1_python_case(be, ocfg, B=3, L=14, T=5, dtype="fp32"):
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = cases.synth_batch(ocfg, B, L, T, 3)
    res = []
    for lab in (labels, labels[:, None, :]):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=lab)["loss"]
        O.runner_loss(nll, out_attn.to(nll.device)).backward()
        sync(be)
        res.append((nll.detach().cpu().clone(), m._grads.detach().cpu().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0


def g1_abi_case(be, ocfg, dtype, dropout, B=3, L=14, T=5):
    """the old C entry points against the new ones with G = 1 and NULL weights: NLL, loss and the gradient arena, bit for bit"""
    from openp5_amd.model import _ptr
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = cases.synth_batch(ocfg, B, L, T, 3)
    res = []
    for new in (False, True):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        tl._train_mode(m, dropout, 77)
        if dropout > 0:
            m._advance_dropout_step()
        dv, lib, eng = m._be.device, be.lib, m._engine
        a = [m._i64(t, dv) for t in (ids, ww, mask, labels, out_attn)]
        m._sync_shadow()
        m._sync_transposed()
        need = int(lib.p5_train_workspace_bytes(eng, B, L, T))
        assert need == int(lib.p5_train_workspace_bytes_targets(eng, B, L, T, 1))
        ws = m._workspace(need)
        out = torch.zeros(B * T + 1, dtype=torch.float32, device=dv)
        loss_p = torch.zeros(1, dtype=torch.float32, device=dv)
        tr = 1 if dropout > 0 else 0
        if new:
            rc = lib.p5_forward_loss_targets(eng, *[_ptr(t) for t in a], B, L, T, 1, None, tr, _ptr(out), _ptr(loss_p), _ptr(ws), ws.numel(), m._be.stream_ptr())
        else:
            rc = lib.p5_forward_loss(eng, *[_ptr(t) for t in a], B, L, T, tr, _ptr(out), _ptr(loss_p), _ptr(ws), ws.numel(), m._be.stream_ptr())
        be.check(rc, "forward_loss")
        be.check(lib.p5_backward(eng, None, m._be.stream_ptr()), "backward")
        sync(be)
        fused = (out[:B * T].cpu().clone(), loss_p.cpu().clone(), m._grads.detach().cpu().clone())
        nll = torch.zeros(B * T, dtype=torch.float32, device=dv)
        if new:
            rc = lib.p5_forward_targets(eng, *[_ptr(t) for t in a[:4]], B, L, T, 1, tr, _ptr(nll), _ptr(ws), ws.numel(), m._be.stream_ptr())
        else:
            rc = lib.p5_forward(eng, *[_ptr(t) for t in a[:4]], B, L, T, tr, _ptr(nll), _ptr(ws), ws.numel(), m._be.stream_ptr())
        be.check(rc, "forward")
        sync(be)
        res.append(fused + (nll.cpu().clone(),))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert float(res[0][2].abs().max()) > 0 and torch.equal(res[0][0], res[0][3])


# ---------------------------------------------------------------------------------------------------------
# 3. the fused loss
# ---------------------------------------------------------------------------------------------------------
def _weights(B, G, seed=5):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(B, G, generator=g)
    w.view(-1)[0] = 0.0
    w.view(-1)[-1] = -abs(float(w.view(-1)[-1])) - 0.25
    return w


def fused_case(be, ocfg, B=3, L=11, T=5, G=3, dtype="fp32", dropout=0.0, tol=1e-6):
    """loss_and_backward(labels [B, G, T], target_weights) == forward -> the torch expression of the weighted masked mean -> backward
    (the rule of cases.fused_loss_case); target_weights=None == all ones, bit for bit"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = grouped_batch(ocfg, B, L, T, G, 9)
    w = _weights(B, G)
    res = {}
    for mode in ("autograd", "fused", "autograd_w", "fused_w", "fused_ones"):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        tl._train_mode(m, dropout, 77)
        tw = {"fused_w": w, "autograd_w": w, "fused_ones": torch.ones(B, G)}.get(mode)
        if mode.startswith("fused"):
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=tw)
        else:
            nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
            loss = weighted_loss(nll, out_attn, tw)
            loss.backward()
        sync(be)
        res[mode] = (float(loss.detach()), m._grads.detach().cpu().clone())
    for a, b in (("autograd", "fused"), ("autograd_w", "fused_w")):
        (l0, g0), (l1, g1) = res[a], res[b]
        assert abs(l0 - l1) <= tol * max(1.0, abs(l0)), (a, l0, l1)
        assert float(g0.abs().max()) > 0
        err = float((g0 - g1).abs().max()) / max(1e-12, float(g0.abs().max()))
        assert err <= (tol if dtype == "fp32" else 2e-2), f"{b}: fused-loss gradient differs: {err}"
    assert res["fused"][0] == res["fused_ones"][0] and torch.equal(res["fused"][1], res["fused_ones"][1])
    assert float((res["fused"][1] - res["fused_w"][1]).abs().max()) > 0


def weights_oracle_case(be, ocfg, B=3, L=14, T=5, G=3):
    """weights with 0 and negative entries: loss and every gradient against the oracle on the replicated batch"""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = grouped_batch(ocfg, B, L, T, G)
    w = _weights(B, G)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w)
    sync(be)
    Pq = _oracle_params(params, "fp32")
    nll_o = O.p5_forward_nll(Pq, ocfg, rep(ids, G), rep(ww, G), rep(mask, G), labels.view(B * G, T))
    loss_o = weighted_loss(nll_o, out_attn, w)
    loss_o.backward()
    loss_o = loss_o.detach()
    assert abs(float(loss) - float(loss_o)) <= NLL_TOL * max(1.0, abs(float(loss_o))), (float(loss), float(loss_o))
    _, worst = _fp32_errors(m, Pq, nll_o, nll_o)
    print(f"[multi target weights] loss {float(loss):.6f} oracle {float(loss_o):.6f}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= GRAD_TOL, f"gradient mismatch {worst}"


def dead_user_case(be, ocfg, B=3, L=14, T=5, G=3, drop_tol=1e-5):
    """a user whose weights are all 0: the gradients of the batch without that user, scaled by (B - 1) / B
    (drop_tol of cases.model_dead_sample_case)"""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = grouped_batch(ocfg, B, L, T, G)
    w = _weights(B, G, 6).abs() + 0.5
    w[1] = 0.0
    w[0, 0] = -0.75
    keep = [b for b in range(B) if b != 1]
    res = []
    for sl in (list(range(B)), keep):
        m = cases.build_model(be, ocfg, params, "fp32")
        m.eval()
        loss = m.loss_and_backward(ids[sl], ww[sl], mask[sl], labels[sl], out_attn[sl], target_weights=w[sl])
        sync(be)
        res.append((float(loss), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = res
    assert abs(l0 * B - l1 * (B - 1)) <= drop_tol * max(1.0, abs(l1)) * B, (l0, l1)
    gmax = max(float(v.abs().max()) for v in g1.values()) * (B - 1) / B
    worst = (0.0, "")
    for n, g_ in g0.items():
        gr = g1[n] * ((B - 1) / B)
        worst = max(worst, (float((g_ - gr).abs().max()) / (float(gr.abs().max()) + 1e-2 * gmax + 1e-12), n))
    assert gmax > 0 and worst[0] <= drop_tol, f"gradients differ from the batch without the zero-weight user {worst}"


def zero_target_exact_case(be, ocfg, B=2, L=14, T=5, G=3):
    """a target with weight 0 or an all-zero mask gives exact-zero contributions: replacing its labels changes neither loss nor gradient bits"""
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = grouped_batch(ocfg, B, L, T, G)
    w = torch.ones(B, G)
    w[1, 1] = 0.0
    other = labels.clone()
    other[1, 1, 0] = 5 if int(labels[1, 1, 0]) != 5 else 6          # the zero-weight target
    other[0, G - 1, 0] = 5 if int(labels[0, G - 1, 0]) != 5 else 6      # the all-masked target
    res = []
    for lab in (labels, other):
        m = cases.build_model(be, ocfg, params, "fp32")
        m.eval()
        loss = m.loss_and_backward(ids, ww, mask, lab, out_attn, target_weights=w)
        sync(be)
        res.append((float(loss), m._grads.detach().cpu().clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------------
# 4. dropout
# ---------------------------------------------------------------------------------------------------------
def dropout_case(be, ocfg, shape=(2, 14, 5, 3), p=0.1):
    B, L, T, G = shape
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": p})
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = grouped_batch(ocfg, B, L, T, G)
    runs = []
    for _ in range(2):
        m = cases.build_model(be, ocfg, params, "fp32", p)
        dp = tl._train_mode(m, p)
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"]
        weighted_loss(nll, out_attn).backward()
        sync(be)
        runs.append((nll.detach().cpu().clone(), m._grads.detach().cpu().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs with the same seed and step differ"
    Pq = _oracle_params(params, "fp32")
    nll_o = grouped_nll(Pq, ocfg, ids, ww, mask, labels, dp)
    weighted_loss(nll_o, out_attn).backward()
    return _check(m, Pq, nll, nll_o, "fp32", f"dropout {shape}")


def restatement_case(ocfg, shape=(2, 14, 5, 3)):
    """without dropout the grouped restatement IS the oracle on the replicated batch (float64: to rounding)"""
    B, L, T, G = shape
    P = {k: v.double() for k, v in O.init_params(ocfg, 7).items()}
    ids, ww, mask, labels, _ = grouped_batch(ocfg, B, L, T, G)
    a = grouped_nll(P, ocfg, ids, ww, mask, labels)
    b = O.p5_forward_nll(P, ocfg, rep(ids, G), rep(ww, G), rep(mask, G), labels.view(B * G, T))
    assert float((a - b).abs().max()) <= 1e-10


# ---------------------------------------------------------------------------------------------------------
# 5. the item loss
# ---------------------------------------------------------------------------------------------------------
def item_batch(ocfg, items, B, L, T, G, seed=tl.MODEL_SEED):
    """labels [B, G, T]: G distinct items of the trie per user (cut at T, pad-filled behind </s>); the last target of the last user
    leaves the trie at position 2.  Returns (ids, ww, mask, labels, out_attn, picks [B][G])."""
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, T, seed)
    g = torch.Generator().manual_seed(seed + 17)
    labels = torch.zeros(B, G, T, dtype=torch.int64)
    out_attn = torch.zeros(B, G, T, dtype=torch.int64)
    picks = []
    for b in range(B):
        pick = torch.randperm(len(items), generator=g)[:G].tolist()
        picks.append(pick)
        for k, i in enumerate(pick):
            q = items[i][1:1 + T]
            labels[b, k, :len(q)] = torch.tensor(q)
            out_attn[b, k, :len(q)] = 1
    labels[B - 1, G - 1, 2] = ocfg.vocab_size - 1
    return ids, ww, mask, labels, out_attn, picks


def item_case(be, ocfg, items, B=3, L=14, T=6, G=3, dtype="fp32", tau=0.7, excluded=True):
    """forward(trie=..., labels [B, G, T]) against oracle_item_nll on the replicated batch.  excluded_items differs per USER: user 0
    excludes the item of its own target 1 (that target goes off the trie, the same item as a target of another user stays scored),
    user 1 nothing, the others every third item that is none of their targets; states against the Python walk."""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, picks = item_batch(ocfg, items, B, L, T, G)
    excluded_items, excl = None, None
    if excluded:
        excluded_items = _per_user_exclusion(items, labels, out_attn, picks, B)
        excl = ct.excluded_bitmap(excluded_items)
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=tau, excluded_items=excluded_items)["loss"]
    assert nll.shape == (B * G * T,)
    weighted_loss(nll, out_attn).backward()
    sync(be)
    Pq = _oracle_params(params, "bf16")         # (float64, as trie_loss_cases.model_case)
    excl_rep = None if excl is None else np.repeat(excl, G, axis=0)
    nll_o, node, state = tl.oracle_item_nll(Pq, ocfg, rep(ids, G), rep(ww, G), rep(mask, G), labels.view(B * G, T), ct, tau, excl_rep)
    O.runner_loss(nll_o, out_attn.view(B * G, T)).backward()
    got = m.last_item_loss_state.cpu()
    assert got.shape == (B, G, T) and got.dtype == torch.int32
    state = state.reshape(B, G, T)
    assert np.array_equal(got.numpy(), state), (got.tolist(), state.tolist())
    assert (state[B - 1, G - 1, 2:] == tl.OFF).all()
    if excluded:
        assert state[0, 1, 0] == tl.SCORED and (state[0, 1] == tl.OFF).any(), "user 0's exclusion must hit its own target"
        assert not (state[1, 0] == tl.OFF).any(), "... and nobody else's"
        assert not (state[0, 0] == tl.OFF).any() and not (state[0, 2:] == tl.OFF).any()
    assert bool((nll.detach().cpu()[torch.from_numpy(state.reshape(-1) != tl.SCORED)] == 0).all())
    return _check(m, Pq, nll, nll_o, dtype, f"item loss G={G} excluded={excluded}")


def _per_user_exclusion(items, labels, out_attn, picks, B):
    """excluded_items that differ per USER (in place on labels / out_attn / picks): user 0 excludes the item of its own target 1 and every
    second item that is none of its other targets, user 1 -- whose target 0 becomes that same item -- nothing, the others every third item
    that is none of their targets"""
    hit = picks[0][1]
    labels[1, 0] = labels[0, 1]
    out_attn[1, 0] = out_attn[0, 1]
    picks[1][0] = hit
    excluded_items = [[hit] + [i for i in range(0, len(items), 2) if i not in picks[0]], []]
    excluded_items += [[i for i in range(b % 3, len(items), 3) if i not in picks[b]] for b in range(2, B)]
    return excluded_items


def _rel_grad_diff(g0, g1):
    """worst per-tensor difference of two {name: gradient} sets, relative to the tensor's largest entry with the 1 % floor"""
    gmax = max(float(g.abs().max()) for g in g0.values())
    worst = (0.0, "")
    for n, a in g0.items():
        worst = max(worst, (float((g1[n].double() - a.double()).abs().max()) / (float(a.abs().max()) + 1e-2 * gmax + 1e-12), n))
    return worst


def fused_item_case(be, ocfg, items, B=3, L=14, T=6, G=3, dtype="fp32", item_head="dense", tau=0.7, tol=1e-6, **trunc):
    """loss_and_backward(labels [B, G, T], trie=, excluded_items per user, target_weights with 0 and negative entries[, top_k / top_p],
    item_head) -- the engine seeds the item-loss backward kernels itself: 1 / (B*G), the target's weight, the user's bitmap row -- against
    forward + the torch expression of the weighted masked mean + backward (the rule of cases.fused_loss_case) and, without truncation,
    loss and gradients against oracle_item_nll on the replicated batch."""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, picks = item_batch(ocfg, items, B, L, T, G)
    excluded_items = _per_user_exclusion(items, labels, out_attn, picks, B)
    w = _weights(B, G)
    w[0, 1] = 1.5           # (the target its own user's exclusion takes off the trie)
    assert float(w[0, 0]) == 0 and float(w[B - 1, G - 1]) < 0
    kw = dict(trie=ct, temperature=tau, excluded_items=excluded_items, item_head=item_head, **trunc)
    res = []
    for fused in (False, True):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        if fused:
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, **kw)
        else:
            nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, **kw)["loss"]
            loss = weighted_loss(nll, out_attn, w)
            loss.backward()
        sync(be)
        res.append((float(loss.detach()), m._grads.detach().cpu().clone(), m.last_item_loss_state.cpu().clone()))
    (l0, g0, s0), (l1, g1, s1) = res
    assert s1.shape == (B, G, T) and torch.equal(s0, s1)
    assert bool((s1[0, 1] == tl.OFF).any()) and not bool((s1[1, 0] == tl.OFF).any()), "user 0's exclusion must hit its own target only"
    if trunc:
        assert bool((s1 == 3).any()), "the case must truncate a label away"
    assert abs(l0 - l1) <= tol * max(1.0, abs(l0)), (l0, l1)
    assert float(g0.abs().max()) > 0
    err = float((g0 - g1).abs().max()) / max(1e-12, float(g0.abs().max()))
    print(f"[multi target fused item loss {dtype} head {item_head} {trunc}] loss {l1:.6f} / {l0:.6f}, gradients differ by {err:.2e} of the largest entry")
    assert err <= (tol if dtype == "fp32" else 2e-2), f"fused item-loss gradient differs: {err}"
    if not trunc:
        Pq = _oracle_params(params, "bf16")
        excl_rep = np.repeat(ct.excluded_bitmap(excluded_items), G, axis=0)
        nll_o, _, state = tl.oracle_item_nll(Pq, ocfg, rep(ids, G), rep(ww, G), rep(mask, G), labels.view(B * G, T), ct, tau, excl_rep)
        loss_o = weighted_loss(nll_o, out_attn, w)
        loss_o.backward()
        assert np.array_equal(s1.numpy().reshape(B * G, T), state)
        lerr = abs(l1 - float(loss_o.detach()))
        assert lerr <= (NLL_TOL if dtype == "fp32" else tl.BF16_BOUNDS["nll_max"]) * max(1.0, abs(float(loss_o.detach()))), (l1, float(loss_o.detach()))
        _check(m, Pq, nll_o, nll_o, dtype, f"fused item loss head {item_head}")       # (gradients; the NLL itself is item_case's)


def item_trunc_case(be, ocfg, items, B=3, L=14, T=6, G=3, dtype="fp32", **trunc):
    """top_k / top_p with per-user exclusion and target weights: the grouped step against the engine's own replicated-batch run, row for
    row -- states (3 = truncated away included) exactly; NLL, the weighted loss and every gradient (fused grouped backward against
    forward + autograd on the replicated batch, so p5_trunc_ce_bwd_kernel's seed, weight and bitmap row are held) to the sum of the two
    runs' fp32 tolerances.  Bit equality cannot be expected: cross-attention runs a user's G * T queries in one launch (another kernel
    of csrc/p5_attn_tu.hip, and dK / dV summed in another order), and the encoder's GEMMs see B * L rows where the replicated batch's
    see B * G * L, which may take another tile route."""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, picks = item_batch(ocfg, items, B, L, T, G)
    excluded_items = _per_user_exclusion(items, labels, out_attn, picks, B)
    w = _weights(B, G)
    w[0, 1] = 1.5
    kw = dict(trie=ct, temperature=0.7, **trunc)
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    with torch.no_grad():
        a = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, excluded_items=excluded_items, **kw)["loss"].cpu()
    la = float(m.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w, excluded_items=excluded_items, **kw))
    sync(be)
    sa = m.last_item_loss_state.cpu()
    ga = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    m2 = cases.build_model(be, ocfg, params, dtype)
    m2.eval()
    b = m2(input_ids=rep(ids, G), whole_word_ids=rep(ww, G), attention_mask=rep(mask, G), labels=labels.view(B * G, T),
           excluded_items=[excluded_items[u] for u in range(B) for _ in range(G)], **kw)["loss"]
    lb = weighted_loss(b, out_attn, w)
    lb.backward()
    sync(be)
    sb = m2.last_item_loss_state.cpu()
    gb = {n: p.grad.detach().cpu().clone() for n, p in m2.named_parameters()}
    assert sa.shape == (B, G, T) and torch.equal(sa.view(B * G, T), sb), (sa.tolist(), sb.tolist())
    assert bool((sa == 3).any()), "the case must truncate a label away"
    assert bool((sa[0, 1] == tl.OFF).any()) and not bool((sa[1, 0] == tl.OFF).any())
    err = float((a - b.detach().cpu()).abs().max())
    worst = _rel_grad_diff(gb, ga)
    print(f"[multi target trunc {trunc}] grouped against replicated: nll {err:.2e}, loss {abs(la - float(lb.detach())):.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
    assert err <= 2 * NLL_TOL, err
    assert abs(la - float(lb.detach())) <= 2 * NLL_TOL * max(1.0, abs(la)), (la, float(lb.detach()))
    assert max(float(g.abs().max()) for g in gb.values()) > 0 and worst[0] <= 2 * GRAD_TOL, worst
    assert bool((a[sa.view(-1) != 0] == 0).all())


def item_head_case(be, ocfg, items, B=3, L=14, T=6, G=3, dtype="fp32"):
    """item_head="trie" against "dense" on a grouped call: the rule of trie_head_cases.routes_case"""
    from tests import trie_head_cases as th
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = item_batch(ocfg, items, B, L, T, G)
    out = {}
    for head in ("dense", "trie"):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=0.7, item_head=head)["loss"]
        weighted_loss(nll, out_attn).backward()
        sync(be)
        out[head] = (nll.detach().cpu().clone(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}, m._grads.detach().cpu().clone(),
                     m.last_item_loss_state.cpu().clone())
    assert torch.equal(out["dense"][3], out["trie"][3])
    th._compare_routes(ocfg, ct, ids, labels.view(B * G, T), out["dense"], out["trie"], dtype, f" grouped G={G}")


# ---------------------------------------------------------------------------------------------------------
# sampler to trainer
# ---------------------------------------------------------------------------------------------------------
def sampler_case(be, ocfg, items, B=3, L=14, dtype="fp32", tau=0.7):
    """sample_items(num_samples=4) and sample_slates(slate_size=3, num_slates=2) feed `labels` as they are: nll == -token_logprobs within
    trie_loss_cases.SAMPLER_TOL; an empty slate slot (the all-pad sequence) has NLL 0 and no gradient"""
    m, _ = sample_cases.make_model(be, ocfg, dtype)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    tol = tl.SAMPLER_TOL[dtype]
    excluded_items = [list(range(b % 2, len(items), 2)) if b != 1 else [] for b in range(B)]
    out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=4, temperature=tau, excluded_items=excluded_items, seed=3)
    labels = out["sequences"].view(B, 4, -1)[:, :, 1:]
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=tau, excluded_items=excluded_items)["loss"]
    tlp = out["token_logprobs"]
    d = float((nll.detach().view_as(tlp) + tlp).abs().max())
    st = m.last_item_loss_state
    assert st.shape == labels.shape and not bool((st == tl.OFF).any())
    print(f"[multi target == sampler {dtype}] items: max |nll + token log-prob| = {d:.3e} (tol {tol:.1e})")
    assert d <= tol, d
    return d


def slates_case(be, ocfg, n_items=4, B=2, L=12, dtype="fp32", tau=1.0):
    """slates of 3 from a catalogue of n_items with 2 of them excluded for user 0: that user's slates have an empty slot"""
    items = cases.make_items(n_items, 5, hi=60)
    m, _ = sample_cases.make_model(be, ocfg, dtype)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    tol = tl.SAMPLER_TOL[dtype]
    excluded_items = [[0, 1]] + [[] for _ in range(B - 1)]
    out = m.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=3, num_slates=2, temperature=tau,
                          excluded_items=excluded_items, seed=3)
    seq = out["sequences"]
    labels = seq.view(B, 6, -1)[:, :, 1:]
    empty = (labels == 0).all(dim=2)
    assert bool(empty[0].any()) and not bool(empty[1:].any()), "user 0 has two items left: its slates of 3 must hold an empty slot"
    m.zero_grad()
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=tau, excluded_items=excluded_items)["loss"]
    tlp = out["token_logprobs"]
    d = float((nll.detach().view_as(tlp) + tlp).abs().max())
    print(f"[multi target == sampler {dtype}] slates: max |nll + token log-prob| = {d:.3e} (tol {tol:.1e})")
    assert d <= tol, d
    T = labels.shape[2]
    assert bool((nll.detach().view(B, 6, T)[empty.to(nll.device)] == 0).all()), "an empty slot has NLL exactly 0"
    # no gradient: the backward seeded on the empty slots alone leaves an all-zero arena
    nll.backward(empty.to(nll.device)[:, :, None].expand(B, 6, T).reshape(-1).to(nll.dtype))
    sync(be)
    assert float(m._grads.abs().max()) == 0.0, "an empty slot must not reach the gradients"
    return d


# ---------------------------------------------------------------------------------------------------------
# 6. accumulation and the staged backward
# ---------------------------------------------------------------------------------------------------------
def accumulation_case(be, ocfg, dtype="fp32", B=3, L=14, T=5, G=3):
    """two grouped micro-batches through begin_micro_batch == the sum of their separate gradients (the rule of
    trie_loss_cases.accumulation_case / cases.grad_store_first_case: 1e-5 of the largest gradient entry)"""
    params = O.init_params(ocfg, 7)
    a = grouped_batch(ocfg, B, L, T, G, 3)
    b = grouped_batch(ocfg, B, L, T, G, 4)
    w = _weights(B, G)
    alone = []
    for batch in (a, b):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        m.loss_and_backward(*batch, target_weights=w)
        sync(be)
        alone.append(m._grads.detach().cpu().clone())
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    m.begin_micro_batch(first=True, sync=False)
    m.loss_and_backward(*a, target_weights=w)
    m.begin_micro_batch(first=False, sync=False)
    m.loss_and_backward(*b, target_weights=w)
    sync(be)
    got, want = m._grads.detach().cpu(), alone[0] + alone[1]
    scale = float(want.abs().max())
    assert scale > 0 and float((alone[0] - alone[1]).abs().max()) > 0
    err = float((got - want).abs().max())
    assert err <= 1e-5 * scale, (err, scale)


def staged_case(be, ocfg, B, L, T, G, dtype="bf16", dropout=0.0):
    """the staged backward of a grouped step: the whole backward's gradients bit for bit, ranges tiling the arena from the back (the rule
    of cases.staged_backward_case)"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    a = grouped_batch(ocfg, B, L, T, G)
    w = _weights(B, G)

    def run(staged, pairs):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        tl._train_mode(m, dropout, 41)
        m.staged_backward = staged
        be.check(be.lib.p5_backward_stage_pairs(m._engine, 1 if pairs else 0), "pairs")
        loss = m.loss_and_backward(*a, target_weights=w)
        sync(be)
        ranges = [(int(m._staged_ranges[2 * k]), int(m._staged_ranges[2 * k + 1])) for k in range(m._staged_n)] if staged else []
        return float(loss), m._grads.detach().cpu().clone(), ranges, int(m._n)

    l0, g0, _, n = run(False, True)
    assert float(g0.abs().max()) > 0
    for pairs in (True, False):
        l1, g1, ranges, _ = run(True, pairs)
        assert l1 == l0
        assert torch.equal(g1, g0), (pairs, float((g1 - g0).abs().max()))
        got = [r for r in ranges if r[1] > r[0]]
        assert got and got[-1][0] == 0 and got[0][1] == n, got
        for (b0, e0), (b1, e1) in zip(got, got[1:]):
            assert e1 == b0, ("ranges must tile the arena from the back", got)


# ---------------------------------------------------------------------------------------------------------
# 7. errors and the workspace
# ---------------------------------------------------------------------------------------------------------
def errors_case(be, ocfg):
    """limits are ValueErrors that name the limit, raised before the engine is called (the engine's last error stays what it was)"""
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    calls = []
    real_ws = m._workspace          # (both paths size the workspace right before they call the engine)
    m._workspace = lambda *a, **k: calls.append(a) or real_ws(*a, **k)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, 2, 8, 4, 3)

    def both(labels, out_attn, match, **kw):
        with pytest.raises(ValueError, match=match):
            m.loss_and_backward(ids, ww, mask, labels, out_attn, **kw)
        if not kw and labels.shape == out_attn.shape:
            with pytest.raises(ValueError, match=match):
                m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)

    z = lambda *s: torch.zeros(*s, dtype=torch.int64)      # noqa: E731
    both(z(2, 27, 19), z(2, 27, 19), r"G \* T <= 512")                       # G * T = 513
    rows = m.MAX_DECODER_ROWS
    idsb = torch.zeros(rows // 512 + 1, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"B \* G \* T <= 65536"):
        m(input_ids=idsb, labels=z(rows // 512 + 1, 64, 8))
    with pytest.raises(ValueError, match=r"B \* G \* T <= 65536"):
        m.loss_and_backward(idsb, None, None, z(rows // 512 + 1, 64, 8), z(rows // 512 + 1, 64, 8))
    nb = m.MAX_GRID_Y // (512 * ocfg.num_heads) + 1          # B * G * num_heads past a launch grid's y extent, inside the other two limits
    assert nb * 512 <= rows
    with pytest.raises(ValueError, match=r"B \* G \* num_heads <= 65535"):
        m(input_ids=torch.zeros(nb, 8, dtype=torch.int64), labels=z(nb, 512, 1))
    with pytest.raises(ValueError, match=r"B \* G \* num_heads <= 65535"):
        m.loss_and_backward(torch.zeros(nb, 8, dtype=torch.int64), None, None, z(nb, 512, 1), z(nb, 512, 1))
    both(z(2, 3, 4), z(2, 3, 5), "output_attention")
    both(z(2, 3, 4), z(6, 4), "output_attention")
    both(z(2, 4), z(2, 1, 4), "output_attention")
    both(z(2, 3, 4), z(2, 3, 4), r"target_weights.*\[B, G\]", target_weights=torch.ones(2, 4))
    both(z(2, 3, 4), z(2, 3, 4), r"target_weights.*\[B, G\]", target_weights=torch.ones(6))
    both(z(2, 4), z(2, 4), "target_weights", target_weights=torch.ones(2, 1))
    both(z(3, 3, 4), z(3, 3, 4), "first dimension")
    both(z(2, 0, 4), z(2, 0, 4), "G >= 1")
    both(z(2, 1, 2, 4), z(2, 1, 2, 4), "labels")
    assert not calls, "a refused call reached the engine"
    m._workspace = real_ws
    # the engine itself refuses the same shapes (a C caller has no Python in front of it)
    from openp5_amd.model import _ptr
    dv = m._be.device
    t = [m._i64(x, dv) for x in (ids, ww, mask, z(2, 27, 19))]
    nll = torch.zeros(2 * 513, dtype=torch.float32, device=dv)
    ws = m._workspace(1 << 20)
    assert be.lib.p5_forward_targets(m._engine, *[_ptr(x) for x in t], 2, 8, 19, 27, 0, _ptr(nll), _ptr(ws), ws.numel(), m._be.stream_ptr()) != 0
    assert b"G * T <= 512" in be.lib.p5_last_error()
    assert be.lib.p5_forward_targets(m._engine, *[_ptr(x) for x in t], 2, 8, 19, 0, 0, _ptr(nll), _ptr(ws), ws.numel(), m._be.stream_ptr()) != 0


def workspace_case(be, ocfg, B=2, L=12, T=5, G=3):
    """p5_train_workspace_bytes_targets: equals the plain function at G = 1; a forward + backward inside exactly that many bytes succeeds and
    writes nothing behind them (nor behind nll_out: cases._guard_intact), one byte fewer fails with a message"""
    from openp5_amd.model import _ptr
    params = O.init_params(ocfg, 7)
    ids, ww, mask, labels, out_attn = grouped_batch(ocfg, B, L, T, G)
    for dtype in ("fp32", "bf16"):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        dv, lib, eng = m._be.device, be.lib, m._engine
        for b_, l_, t_ in ((B, L, T), (64, 128, 8), (3, 7, 1)):
            assert int(lib.p5_train_workspace_bytes_targets(eng, b_, l_, t_, 1)) == int(lib.p5_train_workspace_bytes(eng, b_, l_, t_))
        a = [m._i64(t, dv) for t in (ids, ww, mask, labels, out_attn)]
        w = _weights(B, G).to(dv)
        m._sync_shadow()
        m._sync_transposed()
        need = int(lib.p5_train_workspace_bytes_targets(eng, B, L, T, G))
        assert need % 256 == 0 and need > int(lib.p5_train_workspace_bytes(eng, B, L, T))
        raw = torch.zeros(need + 256, dtype=torch.uint8, device=dv)
        skew = (-raw.data_ptr()) % 256
        ws = raw[skew:skew + need]
        raw[skew + need:] = 0xA5
        guard = raw[skew + need:].clone()
        n = B * G * T
        out = cases._sentinel((n + 1 + 8,), torch.float32).to(dv)

        def call(nbytes):
            return lib.p5_forward_loss_targets(eng, *[_ptr(t) for t in a], B, L, T, G, _ptr(w), 0, _ptr(out), ctypes.c_void_p(out.data_ptr() + 4 * n),
                                               _ptr(ws), nbytes, m._be.stream_ptr())
        assert call(need - 1) != 0
        assert b"workspace" in lib.p5_last_error()
        assert call(need) == 0
        be.check(lib.p5_backward(eng, None, m._be.stream_ptr()), "backward")
        sync(be)
        assert torch.equal(raw[skew + need:], guard), "the grouped step wrote behind the bytes p5_train_workspace_bytes_targets asked for"
        cases._guard_intact("nll_out / loss_out", out.cpu(), n + 1)
        grads = m._grads.detach().cpu().clone()
        m2 = cases.build_model(be, ocfg, params, dtype)
        m2.eval()
        loss = m2.loss_and_backward(ids, ww, mask, labels, out_attn, target_weights=w)
        sync(be)
        assert torch.equal(out[:n].cpu(), m2(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)["loss"].detach().cpu())
        assert float(out[n]) == float(loss) and torch.equal(grads, m2._grads.detach().cpu())
