"""Cases of trie-constrained sampling (`P5T5Native.sample_items`, csrc/p5_sample.h) shared by tests/test_sample_items_emu.py (host
emulation) and tests/test_gpu_sample_items.py (MI355X).

The reference is the oracle in float64 (`O.encoder_forward`, `O.decoder_forward`, the tied head restated as a product with the children's
rows of the table -- `O.lm_logits` restricted to the columns that are read) plus a Python restatement of the uniforms of csrc/p5_rng.h
built on `O._mix32`.  The device's own numbers are a reference only where a check says so (the bf16 frequency test)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases

FP32_TOL = 1e-4          # the project's fp32 score tolerance
BF16_TOL = 0.1           # per free token: the figure behind cases.BF16_SCORE_TOL
M32 = 0xFFFFFFFF
KEYS = ("sequences", "sequences_logprob", "token_logprobs", "item_index")


def uniforms(seed, stream, draw, step, n):
    """csrc/p5_rng.h::p5_sample_row_key / p5_sample_uniform restated: the uniforms of the n children of a node, float64 (each value is
    (j + 0.5) / 2^23, exact in fp32 as well)"""
    t = lambda v: torch.tensor([v & M32], dtype=torch.int64)      # noqa: E731
    k = O._mix32(t(seed) ^ O._mix32(t(((stream & M32) * 0x9E3779B1 + 0x7F4A7C15))))
    k = O._mix32(k ^ t(draw))
    k = O._mix32((k + t(0x9E3779B9 * (step + 1))) & M32)
    h = O._mix32(k ^ torch.arange(n, dtype=torch.int64))
    return ((h >> 9).double() + 0.5) / 8388608.0


def uniforms_range_case():
    """the restated uniforms stay in the open interval and look uniform"""
    u = torch.cat([uniforms(s, 3, d, 2, 1000) for s in (0, 1, M32) for d in (0, 7)])
    assert float(u.min()) >= 2.0 ** -24 and float(u.max()) <= 1.0 - 2.0 ** -24
    assert abs(float(u.mean()) - 0.5) < 0.02


class Reference:
    """float64 logits of the children of every trie node a user's sequences pass through, computed once per (user, node)"""

    def __init__(self, params, ocfg, ids, ww, mask, ct):
        self.P = {k: v.double() for k, v in params.items()}
        self.cfg, self.ct, self.mask = ocfg, ct, mask
        with torch.no_grad():
            self.enc = O.encoder_forward(self.P, ocfg, ids, ww, mask)
        self.z = {}
        self.edge = {}
        for n in range(ct.n_nodes):
            for e in range(int(ct.child_off[n]), int(ct.child_off[n + 1])):
                self.edge[(n, int(ct.child_tok[e]))] = e

    def children(self, node):
        lo, hi = int(self.ct.child_off[node]), int(self.ct.child_off[node + 1])
        return self.ct.child_tok[lo:hi], self.ct.child_node[lo:hi]

    def walk(self, seq):
        """nodes behind seq[0], seq[:2], ...; raises KeyError when the sequence leaves the trie"""
        nodes, n = [], 0
        for tok in seq:
            n = int(self.ct.child_node[self.edge[(n, int(tok))]])
            nodes.append(n)
        return nodes

    def add(self, b, seqs):
        """teacher-forced float64 decoder over the sequences (token lists, decoder start first) of user b"""
        todo = []
        for q in {tuple(int(t) for t in q) for q in seqs}:
            if any((b, n) not in self.z and self.children(n)[0].size for n in self.walk(q)):
                todo.append(q)
        E, scale = self.P["shared.weight"], self.cfg.d_model ** -0.5
        for a in range(0, len(todo), 64):
            part = todo[a:a + 64]
            T = max(len(q) for q in part)
            dec_ids = torch.zeros(len(part), T, dtype=torch.int64)
            for i, q in enumerate(part):
                dec_ids[i, :len(q)] = torch.tensor(q)
            with torch.no_grad():
                out = O.decoder_forward(self.P, self.cfg, dec_ids, self.enc[b:b + 1].expand(len(part), -1, -1), self.mask[b:b + 1].expand(len(part), -1))
                for i, q in enumerate(part):
                    for t, n in enumerate(self.walk(q)):
                        toks, _ = self.children(n)
                        if toks.size and (b, n) not in self.z:
                            # O.lm_logits (dec_out * d^-0.5 @ E^T), the columns of the node's children only
                            self.z[(b, n)] = (out[i, t] * scale) @ E[torch.from_numpy(toks.astype(np.int64))].T

    def allowed(self, node, excl_row):
        _, kids = self.children(node)
        if excl_row is None:
            return torch.ones(len(kids), dtype=torch.bool)
        return torch.tensor([not ((int(excl_row[int(k) >> 5]) >> (int(k) & 31)) & 1) for k in kids], dtype=torch.bool)

    def item_probs(self, b, items, tau, excl_row=None):
        """exact probability of every item for user b: products of the renormalised child softmaxes along its path"""
        self.add(b, items)
        p = torch.zeros(len(items), dtype=torch.float64)
        for i, q in enumerate(items):
            nodes, lp = self.walk(q), 0.0
            for t in range(len(q) - 1):
                toks, _ = self.children(nodes[t])
                ok = self.allowed(nodes[t], excl_row)
                z = torch.where(ok, self.z[(b, nodes[t])] / tau, torch.full((), -math.inf, dtype=torch.float64))
                c = int(np.nonzero(toks == q[t + 1])[0][0])
                lp = lp + (float(z[c] - torch.logsumexp(z, 0)) if bool(ok[c]) else -math.inf)
            p[i] = math.exp(lp)
        return p


def replay_check(out, ref, items, B, S, seed, streams, draw_base, tau, tol, excl=None, eos=1, tag=""):
    """tests 1 and 2 on every draw and every step: the chosen child is allowed and its perturbed value is within 2 tol / tau of the
    maximum; the sequence ends in </s> at a leaf and item_index names it; token log-probabilities are the reference's renormalised
    log_softmax(z / tau) (exactly 0 where one child is allowed: the forced prefix among them); sequences_logprob is their sum."""
    seq = out["sequences"].cpu()
    lp = out["sequences_logprob"].cpu()
    tlp = out["token_logprobs"].cpu()
    idx = out["item_index"].cpu() if out["item_index"] is not None else None
    T = seq.shape[1]
    assert seq.shape == (B * S, T) and seq.dtype == torch.int64 and lp.shape == (B * S,) and tlp.shape == (B * S, T - 1)
    assert idx is None or (idx.shape == (B, S) and idx.dtype == torch.int64)
    index_of = {tuple(q): i for i, q in enumerate(items)}
    worst_gap, worst_lp = 0.0, 0.0
    for b in range(B):
        rows = [seq[b * S + s].tolist() for s in range(S)]
        lens = [q.index(eos) if eos in q else None for q in rows]
        assert all(n is not None for n in lens), f"user {b}: a draw without </s>"
        ref.add(b, [q[:n + 1] for q, n in zip(rows, lens)])
        ex = None if excl is None else excl[b]
        for s in range(S):
            q, n = rows[s], lens[s]
            assert q[0] == 0 and all(t == 0 for t in q[n + 1:]), "decoder start first, pad-filled behind </s>"
            nodes = ref.walk(q[:n + 1])
            assert ref.children(nodes[-1])[0].size == 0, "the sequence must end at a leaf"
            if idx is not None:
                assert int(idx[b, s]) == index_of[tuple(q[:n + 1])], (b, s, int(idx[b, s]))
            for t in range(1, n + 1):
                node = nodes[t - 1]
                toks, _ = ref.children(node)
                ok = ref.allowed(node, ex)
                c = int(np.nonzero(toks == q[t])[0][0])
                assert bool(ok[c]), f"user {b} draw {s} step {t}: an excluded child was drawn"
                z = torch.where(ok, ref.z[(b, node)] / tau, torch.full((), -math.inf, dtype=torch.float64))
                g = -torch.log(-torch.log(uniforms(seed, int(streams[b]), draw_base + s, t, len(toks))))
                pert = z + g
                gap = float(pert.max() - pert[c])
                worst_gap = max(worst_gap, gap)
                assert gap <= 2 * tol / tau, f"user {b} draw {s} step {t}: perturbed value {gap:.3e} below the maximum (bound {2 * tol / tau:.1e})"
                want = float(z[c] - torch.logsumexp(z, 0))
                got = float(tlp[b * S + s, t - 1])
                if int(ok.sum()) == 1:
                    assert got == 0.0, f"user {b} draw {s} step {t}: one allowed child, log-probability {got!r} instead of exactly 0"
                worst_lp = max(worst_lp, abs(got - want))
                assert abs(got - want) <= tol, f"user {b} draw {s} step {t}: token log-probability {got} vs {want}"
            assert bool((tlp[b * S + s, n:] == 0).all())
            assert abs(float(lp[b * S + s]) - float(tlp[b * S + s].double().sum())) <= 1e-5 * max(1, n)
    print(f"[sample{tag}] B={B} S={S} tau={tau}: largest shortfall of a chosen child's perturbed value {worst_gap:.3e} (bound {2 * tol / tau:.1e}); "
          f"max |token log-prob - reference| = {worst_lp:.3e} (tol {tol:.1e})")
    return worst_gap, worst_lp


def make_model(be, ocfg, dtype="fp32", params=None):
    params = params if params is not None else O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    return m, params


def sample_case(be, ocfg, B, L, items, S, dtype="fp32", tau=1.0, seed=1, streams=None, draw_base=0, excluded_items=None, batch_seed=5, ct=None, tag=""):
    """sample_items on a synthetic batch; replay and log-prob checks on everything returned"""
    m, params = make_model(be, ocfg, dtype)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, batch_seed)
    ct = ct if ct is not None else rank_cases.compiled(items)
    out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=tau, seed=seed, streams=streams,
                         draw_base=draw_base, excluded_items=excluded_items)
    assert m.last_generate_path == "sample"
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    excl = None if excluded_items is None else ct.excluded_bitmap(excluded_items)
    replay_check(out, ref, items, B, S, seed, streams if streams is not None else list(range(B)), draw_base, tau, FP32_TOL if dtype == "fp32" else BF16_TOL,
                 excl=excl, tag=f"{tag} {dtype}")
    return out, m, ref, (ids, ww, mask, ct)


# ---- 3. frequencies ----
def freq_items():
    """40 items of unequal lengths (1 to 4 tokens behind the shared prefix)"""
    items = cases.make_items(40, 13, hi=60, minlen=1, maxlen=4)
    assert len({len(q) for q in items}) >= 3
    return items


def bins_ok(counts, p, S):
    """every item with expected count e = S p >= 5 is a bin, all others are pooled into one: |count - e| <= 5 sqrt(e (1 - p)) + 1"""
    counts, p = np.asarray(counts, dtype=np.float64), np.asarray(p, dtype=np.float64)
    big = S * p >= 5
    pc = np.concatenate([p[big], [max(0.0, 1.0 - p[big].sum())]])
    cc = np.concatenate([counts[big], [S - counts[big].sum()]])
    e = S * pc
    bad = np.abs(cc - e) > 5 * np.sqrt(e * (1 - pc)) + 1
    return not bool(bad.any()), int(bad.sum()), len(pc)


def frequency_case(be, ocfg, S, dtype="fp32", seeds=(1, 2, 3), B=2, L=12):
    items = freq_items()
    m, params = make_model(be, ocfg, dtype)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    for seed in seeds:
        out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=seed)
        idx, lp = out["item_index"].cpu(), out["sequences_logprob"].cpu().view(B, S)
        assert int(idx.min()) >= 0
        for b in range(B):
            counts = np.bincount(idx[b].numpy(), minlength=len(items))
            if dtype == "fp32":
                p = ref.item_probs(b, items, 1.0).numpy()
                assert abs(p.sum() - 1.0) < 1e-9
            else:
                # the probabilities the device itself reported for the drawn items (held to the reference by the log-prob check); items
                # never drawn fall into the rest bin, whose probability is 1 - sum over the distinct drawn items
                p = np.zeros(len(items))
                for s in range(S):
                    p[int(idx[b, s])] = math.exp(float(lp[b, s]))
            ok, n_bad, n_bins = bins_ok(counts, p, S)
            print(f"[sample freq {dtype}] seed {seed} user {b}: {n_bins} bins, {n_bad} outside 5 sigma + 1")
            assert ok, f"seed {seed} user {b}: {n_bad} of {n_bins} bins outside the bound"
    return ref, items


def bound_is_not_vacuous_case(ocfg, S, B=2, L=12):
    """CPU only: a NumPy multinomial from the reference probabilities passes the bins; a sampler that ignores the model and draws
    children uniformly violates them on this trie"""
    items = freq_items()
    params = O.init_params(ocfg, 7)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    rng = np.random.default_rng(0)
    for b in range(B):
        p = ref.item_probs(b, items, 1.0).numpy()
        for _ in range(3):
            assert bins_ok(rng.multinomial(S, p / p.sum()), p, S)[0]
        unif = np.zeros(len(items))
        for i, q in enumerate(items):
            nodes, pr = ref.walk(q), 1.0
            for t in range(len(q) - 1):
                pr /= len(ref.children(nodes[t])[0])
            unif[i] = pr
        assert abs(unif.sum() - 1.0) < 1e-9
        assert not bins_ok(rng.multinomial(S, unif), p, S)[0], "the bound does not tell the model's distribution from uniform children"


# ---- 5. exclusion ----
def exclusion_case(be, ocfg, S, prefix, S_freq=None, L=12):
    """user 0: half the catalogue excluded; user 1: everything; user 2: nothing.  `prefix` (0, 5, 6): a forced chain (the all-excluded
    user touches it); (0,): none (that user reaches the kernel and has no allowed child at the first step)."""
    items = cases.make_items(40, 13, hi=60, minlen=1, maxlen=4, prefix=prefix)
    n = len(items)
    half = list(range(0, n, 2))
    excluded = [half, list(range(n)), []]
    m, params = make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, 3, L, 4, 5)
    ct = rank_cases.compiled(items)
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=4)
    out = m.sample_items(excluded_items=excluded, **kw)
    idx, lp, seq = out["item_index"].cpu(), out["sequences_logprob"].cpu().view(3, S), out["sequences"].cpu().view(3, S, -1)
    assert bool((idx[1] == -1).all()) and bool((lp[1] == -math.inf).all()) and int(seq[1].abs().max()) == 0
    assert not (set(idx[0].tolist()) & set(half)), "an excluded item was drawn"
    excl = ct.excluded_bitmap(excluded)
    live = {"item_index": out["item_index"][[0, 2]], "sequences_logprob": out["sequences_logprob"].view(3, S)[[0, 2]].reshape(2 * S)}
    for k in ("sequences", "token_logprobs"):
        live[k] = out[k].view(3, S, -1)[[0, 2]].reshape(2 * S, -1)
    replay_check(live, ReferenceView(ref, [0, 2]), items, 2, S, 4, [0, 2], 0, 1.0, FP32_TOL, excl=excl[[0, 2]], tag=f" exclusion prefix={prefix}")
    # the others are unaffected, bit for bit, by that user's exclusion
    other = m.sample_items(excluded_items=[half, [], []], **kw)
    for k in KEYS:
        a, o = out[k].cpu(), other[k].cpu()
        a, o = (a, o) if k == "item_index" else (a.view(3, S, -1), o.view(3, S, -1))
        assert torch.equal(a[[0, 2]], o[[0, 2]]), f"{k} of the other users changed with user 1's exclusion"
    if S_freq:
        big = m.sample_items(input_ids=ids[:1], attention_mask=mask[:1], whole_word_ids=ww[:1], trie=ct, num_samples=S_freq, seed=2, excluded_items=[half])
        p = ref.item_probs(0, items, 1.0, excl_row=excl[0]).numpy()
        assert abs(p.sum() - 1.0) < 1e-9 and float(p[half].max()) == 0.0
        counts = np.bincount(big["item_index"].cpu()[0].numpy(), minlength=n)
        ok, n_bad, n_bins = bins_ok(counts, p, S_freq)
        print(f"[sample exclusion] {n_bins} bins, {n_bad} outside 5 sigma + 1")
        assert ok and int(counts[half].sum()) == 0


class ReferenceView:
    """a Reference seen through a list of users (row i of a sub-batch = user users[i])"""

    def __init__(self, ref, users):
        self.ref, self.users = ref, users
        self.children, self.walk, self.allowed = ref.children, ref.walk, ref.allowed
        self.z = _ZView(ref, users)

    def add(self, b, seqs):
        self.ref.add(self.users[b], seqs)


class _ZView:
    def __init__(self, ref, users):
        self.ref, self.users = ref, users

    def __getitem__(self, key):
        return self.ref.z[(self.users[key[0]], key[1])]


# ---- 6. determinism and plumbing ----
def same_bits(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k].cpu(), b[k].cpu()), f"{k}: {what}"


def determinism_case(be, ocfg, B=3, L=14, S=10):
    items = cases.make_items(40, 5, hi=60)
    m, _ = make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct)
    a = m.sample_items(num_samples=S, seed=9, **kw)
    same_bits(a, m.sample_items(num_samples=S, seed=9, **kw), "two calls with one seed")
    c = m.sample_items(num_samples=S, seed=10, **kw)
    assert not torch.equal(a["item_index"].cpu(), c["item_index"].cpu()), "another seed must draw differently"
    # seed=None: fresh seeds from the per-model counter, reproducible from the model's seed
    d1, d2 = m.sample_items(num_samples=S, **kw), m.sample_items(num_samples=S, **kw)
    assert not torch.equal(d1["item_index"].cpu(), d2["item_index"].cpu())
    m2, _ = make_model(be, ocfg, "fp32")
    same_bits(d1, m2.sample_items(num_samples=S, **kw), "the first seedless call of two models built with one seed")
    # user chunks and draw ranges of at most wide_max_rows rows
    calls = m.sample_stats["engine_calls"]
    m.wide_max_rows = 8
    same_bits(a, m.sample_items(num_samples=S, seed=9, **kw), "wide_max_rows = 8")
    assert m.sample_stats["engine_calls"] - calls == 2 * B, "10 draws in ranges of 8 and 2, one user per call"
    m.wide_max_rows = 2 * S
    same_bits(a, m.sample_items(num_samples=S, seed=9, **kw), "two users per call")
    m.wide_max_rows = type(m).wide_max_rows
    # num_samples split by hand
    lo = m.sample_items(num_samples=4, seed=9, **kw)
    hi = m.sample_items(num_samples=S - 4, seed=9, draw_base=4, **kw)
    for k in KEYS:
        v = (lambda t: t.cpu()) if k == "item_index" else (lambda t: t.cpu().view(B, -1, t.shape[-1]) if t.dim() == 2 else t.cpu().view(B, -1))
        assert torch.equal(torch.cat([v(lo[k]), v(hi[k])], 1), v(a[k])), f"{k}: draws 0-3 and 4-9 in two calls"
    # the coordinates reach the kernel: other ids, replayed with those ids
    sample_case(be, ocfg, 1, L, items, 6, seed=9, streams=[7], draw_base=5, tag=" streams=[7] draw_base=5")
    # streams: a user's draws do not depend on the batch they are made in
    one = m.sample_items(input_ids=ids[1:2], attention_mask=mask[1:2], whole_word_ids=ww[1:2], trie=ct, num_samples=S, seed=9, streams=[1])
    for k in KEYS:
        v = (lambda t: t.cpu()) if k == "item_index" else (lambda t: t.cpu().view(-1, S, t.shape[-1]) if t.dim() == 2 else t.cpu().view(-1, S))
        assert torch.equal(v(one[k])[0], v(a[k])[1]), f"{k}: user 1 alone with streams=[1]"


def lanes_case(be, ocfg, lanes):
    """map_lanes over batches of different B and S returns the bits of one-at-a-time calls"""
    items = cases.make_items(40, 5, hi=60)
    ct = rank_cases.compiled(items)
    m, _ = make_model(be, ocfg, "bf16")
    batches = []
    for i, (B, S) in enumerate([(3, 5), (1, 20), (4, 3), (2, 17), (3, 8), (2, 1)]):
        ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, 12 + i, 4, 30 + i)
        batches.append(dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, num_samples=S, seed=40 + i))

    def one(kw):
        out = m.sample_items(trie=ct, **kw)
        return {k: out[k].cpu() for k in KEYS}
    want = [one(kw) for kw in batches]
    got = list(m.map_lanes(one, batches, lanes=lanes))
    for w, g in zip(want, got):
        same_bits(w, g, "map_lanes")


# ---- 7. forced prefix ----
def forced_prefix_case(be, ocfg, dtype="fp32", B=2, L=12, S=12):
    items = cases.make_items(40, 5, hi=60)
    tol = FP32_TOL if dtype == "fp32" else BF16_TOL
    outs = []
    for ff in (1, 0):
        be.lib.p5_set_option(b"gen_ff", ff)
        try:
            out, m, _, _ = sample_case(be, ocfg, B, L, items, S, dtype=dtype, seed=6, tag=f" gen_ff={ff}")
        finally:
            be.lib.p5_set_option(b"gen_ff", 1)
        assert m.sample_stats["forced_prefix_steps"] == 2
        outs.append(out)
    a, b = outs
    if torch.equal(a["sequences"].cpu(), b["sequences"].cpu()):
        d = float((a["token_logprobs"].cpu() - b["token_logprobs"].cpu()).abs().max())
        assert d <= 2 * tol
    else:       # a draw decided differently within the tolerance: compare the draws that agree
        eq = (a["sequences"].cpu() == b["sequences"].cpu()).all(1)
        assert float(eq.float().mean()) >= 0.5
        d = float((a["token_logprobs"].cpu() - b["token_logprobs"].cpu())[eq].abs().max())
        assert d <= 2 * tol
    print(f"[sample forced prefix {dtype}] fast-forward on / off: max |token log-prob difference| = {d:.3e}")
    # the model's own switch: every step a decode step
    m, _ = make_model(be, ocfg, dtype)
    m.prefix_fast_forward = False
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    c = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=rank_cases.compiled(items), num_samples=S, seed=6)
    assert m.sample_stats["forced_prefix_steps"] == 0
    same_bits(b, c, "gen_ff = 0 and prefix_fast_forward = False run the same steps")


# ---- 8. generate ----
def generate_case(be, ocfg, B=2, L=12, S=6):
    from openp5_amd.trie import Trie, prefix_allowed_tokens_fn
    items = cases.make_items(40, 5, hi=60)
    m, _ = make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    trie = Trie(items)
    ct = m._compiled_trie(trie)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww)
    beam = dict(max_length=12, num_beams=5, num_return_sequences=5, output_scores=True, return_dict_in_generate=True, trie=trie, **kw)
    g1 = m.generate(**beam)
    path = m.last_generate_path
    want = m.sample_items(trie=ct, num_samples=S, temperature=0.7, seed=3, **kw)
    got = m.generate(do_sample=True, num_beams=1, num_return_sequences=S, temperature=0.7, seed=3, max_length=30,
                     prefix_allowed_tokens_fn=prefix_allowed_tokens_fn(trie), output_scores=True, return_dict_in_generate=True, **kw)
    assert m.last_generate_path == "sample"
    assert torch.equal(got["sequences"].cpu(), want["sequences"].cpu()) and torch.equal(got["sequences_scores"].cpu(), want["sequences_logprob"].cpu())
    plain = m.generate(do_sample=True, num_return_sequences=S, temperature=0.7, seed=3, trie=trie, **kw)
    assert torch.equal(plain.cpu(), want["sequences"].cpu())
    for bad, word in ((dict(num_beams=2), "num_beams"), (dict(top_k=50), "top_k"), (dict(top_p=0.9), "top_p"), (dict(roots=[0] * B), "roots")):
        with pytest.raises(ValueError, match=word) as ei:
            m.generate(do_sample=True, trie=trie, **{**dict(num_beams=1), **bad}, **kw)
        assert "supports" in str(ei.value)
    # the beam search is what it was: same bits with its decode-step graph kept ...
    g2 = m.generate(**beam)
    assert m.last_generate_path == path
    for k in ("sequences", "sequences_scores"):
        assert torch.equal(g1[k].cpu(), g2[k].cpu()), f"generate() {k} changed after a sampling call"
    # ... and rebuilt (another shape in between), with a sampling call in between as well
    m.generate(**{**beam, "num_beams": 3, "num_return_sequences": 3})
    m.sample_items(trie=ct, num_samples=S, seed=3, **kw)
    g3 = m.generate(**beam)
    for k in ("sequences", "sequences_scores"):
        assert torch.equal(g1[k].cpu(), g3[k].cpu()), f"generate() {k} changed after its graph was rebuilt"
    # do_sample=False: nothing changes
    g4 = m.generate(do_sample=False, **beam)
    assert torch.equal(g1["sequences"].cpu(), g4["sequences"].cpu())


# ---- 9. ABI ----
def workspace_case(be, ocfg, B=2, L=12, S=5):
    """p5_sample_workspace_bytes is exact: a call inside exactly that many bytes succeeds, one byte fewer fails with a message"""
    from openp5_amd import _abi
    from openp5_amd.model import _ptr
    assert len(_abi.PROTOTYPES["p5_sample_workspace_bytes"][1]) == 7 and len(_abi.PROTOTYPES["p5_sample_items"][1]) == 25
    items = cases.make_items(40, 5, hi=60)
    m, params = make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    dev = m._be.device
    off, tok, nxt = ct.device_arrays(dev)
    ids_d, ww_d, mask_d = (m._i64(t, dev) for t in (ids, ww, mask))
    m._sync_shadow()
    m._sync_transposed()
    eng, T = m._cur_lane().engine, int(ct.max_depth)
    need = int(be.lib.p5_sample_workspace_bytes(eng, B, L, S, T, ct.max_children, 0))
    assert need > 0 and need % 256 == 0
    assert need == int(be.lib.p5_sample_workspace_bytes(eng, B, L, S, T, 7 * ct.max_children, 3)), "no buffer follows the fan-out or the bitmap"
    raw = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    skew = (-raw.data_ptr()) % 256
    ws = raw[skew:skew + need]
    guard = raw[skew + need:].clone()
    streams = torch.arange(B, dtype=torch.int32, device=dev)
    seq = torch.zeros(B, S, T, dtype=torch.int32, device=dev)
    lp = torch.zeros(B, S, dtype=torch.float32, device=dev)
    tlp = torch.zeros(B, S, T, dtype=torch.float32, device=dev)
    ln = torch.zeros(B, S, dtype=torch.int32, device=dev)

    def call(nbytes):
        return be.lib.p5_sample_items(eng, _ptr(ids_d), _ptr(ww_d), _ptr(mask_d), B, L, S, T, _ptr(off), _ptr(tok), _ptr(nxt), None, 0, ct.max_children, 5,
                                      _ptr(streams), 0, 1.0, _ptr(seq), _ptr(lp), _ptr(tlp), _ptr(ln), _ptr(ws), nbytes, m._be.stream_ptr())
    assert call(need - 1) != 0
    assert b"workspace" in be.lib.p5_last_error()
    assert call(need) == 0
    if torch.cuda.is_available() and raw.is_cuda:
        torch.cuda.synchronize()
    assert torch.equal(raw[skew + need:], guard), "the call wrote behind the bytes it asked for"
    m.prefix_fast_forward = False          # (the raw call above set no forced prefix)
    want = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=5)
    assert torch.equal(seq.view(B * S, T).cpu().to(torch.int64), want["sequences"].cpu()) and torch.equal(lp.view(-1).cpu(), want["sequences_logprob"].cpu())
    assert bool((ln > 0).all())
    for bad in (dict(S=0), dict(S=4097), dict(T=1), dict(T=129), dict(tau=0.0), dict(tau=-1.0)):
        a = dict(S=S, T=T, tau=1.0, **{})
        a.update(bad)
        rc = be.lib.p5_sample_items(eng, _ptr(ids_d), _ptr(ww_d), _ptr(mask_d), B, L, a["S"], a["T"], _ptr(off), _ptr(tok), _ptr(nxt), None, 0, ct.max_children,
                                    5, _ptr(streams), 0, ctypes.c_float(a["tau"]), _ptr(seq), _ptr(lp), _ptr(tlp), _ptr(ln), _ptr(ws), need, m._be.stream_ptr())
        assert rc != 0, bad


def errors_case(be, ocfg):
    from openp5_amd.trie import Trie
    items = cases.make_items(20, 5, hi=60)
    m, _ = make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, 2, 12, 4, 5)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww)
    with pytest.raises(ValueError, match="trie"):
        m.sample_items(**kw)
    for bad in (dict(num_samples=0), dict(temperature=0.0), dict(temperature=float("nan")), dict(streams=[1, 2, 3]), dict(excluded_items=[[0]]),
                dict(excluded_items=[[0], [20]]), dict(draw_base=-1)):
        with pytest.raises(ValueError):
            m.sample_items(trie=Trie(items), **bad, **kw)
    # a trie with an appended trie is sampled like any other, but cannot be indexed
    bos = 61
    grafted = Trie([list(it[:4]) + [bos] for it in items])
    grafted.append(Trie([list(it[4:]) for it in items]), bos)
    out = m.sample_items(trie=grafted, num_samples=3, seed=1, **kw)
    assert out["item_index"] is None and bool((out["sequences_logprob"].cpu() <= 0).all())
    # a plain Trie is compiled and indexed on demand, items in lexicographic order (make_items returns them sorted)
    out = m.sample_items(trie=Trie(items), num_samples=3, seed=1, **kw)
    seq, idx = out["sequences"].cpu(), out["item_index"].cpu().view(-1)
    for r in range(seq.shape[0]):
        q = seq[r].tolist()
        assert q[:q.index(1) + 1] == items[int(idx[r])]
