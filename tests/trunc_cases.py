"""Cases of top-k / nucleus truncation (csrc/p5_trunc.h: `sample_items(top_k=, top_p=)`, `forward(trie=, top_k=, top_p=)`) shared by
tests/test_trunc_emu.py (host emulation) and tests/test_gpu_trunc.py (MI355X).

The reference is float64: `kept_ref` restates the semantics (HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on the
allowed children, the nucleus by VALUE), `classify` says which children a logit error within the tolerance could move across the cut, and
the model's logits come from `sample_cases.Reference` / the oracle under autograd."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases, sample_cases, trie_loss_cases
from tests.cases import ATTN_TAU, P, TT, _elem_check, _elem_r, _guard_intact, _sentinel, dev, sync
from tests.sample_cases import BF16_TOL, FP32_TOL, KEYS, Reference, uniforms

SCORED, TRUNCATED = 0, 3
NEG = -math.inf
UNDECIDED_CAP = 0.10          # of the visited (user, node) pairs: the slates tests' figure
P_MARGIN = 1e-5               # the top-p cut is exact where every boundary mass is farther than this (relative) from top_p
STAGE = 2048                  # P5_TRUNC_STAGE of csrc/p5_trunc.h: wider nodes are not staged in LDS


def p32(top_p):
    """top_p as the engine receives it (a C float)"""
    return float(np.float32(top_p))


# ---------------------------------------------------------------------------------------------------------
# the semantics, float64
# ---------------------------------------------------------------------------------------------------------
def kept_ref(z, top_k=0, top_p=1.0):
    """z: float64 [n], -inf = not allowed (excluded or a masked logit).  Returns (kept bool [n], cut = min z over the kept set or +inf,
    margin = the least relative distance of a boundary mass from top_p, inf without top-p)."""
    z = z.double()
    keep = torch.isfinite(z)
    if top_k > 0 and int(keep.sum()) > top_k:
        kth = torch.topk(z[keep], top_k).values[-1]
        keep = keep & (z >= kth)
    margin = math.inf
    p = p32(top_p)
    if p < 1.0 and bool(keep.any()):
        zz = torch.where(keep, z, torch.full_like(z, NEG))
        w = torch.exp(zz - zz.max())
        vals, inv = torch.unique(zz, return_inverse=True)                    # ascending
        mass = torch.zeros_like(vals).index_add_(0, inv, w)
        above = (mass.flip(0).cumsum(0).flip(0) - mass)[inv]                 # mass of the values strictly above each child's
        M = w.sum()
        margin = float(((above[keep] / M - p).abs() / p).min())
        keep = keep & (above < p * M)
    cut = float(z[keep].min()) if bool(keep.any()) else math.inf
    return keep, cut, margin


def classify(z, top_k, top_p, eps):
    """three-way under perturbations |dz_i| <= eps of every allowed child: (surely kept, surely removed) bool [n]; the rest of the allowed
    children is undecided.  Conservative: whatever it calls sure is sure."""
    z = z.double()
    ok = torch.isfinite(z)
    n = z.numel()
    gt_hi = (z[None, :] + eps > z[:, None] - eps) & ok[None, :] & ~torch.eye(n, dtype=torch.bool)      # j may lie above i
    gt_lo = (z[None, :] - eps > z[:, None] + eps) & ok[None, :]                                        # j surely lies above i
    sure_in, sure_out = ok.clone(), ~ok
    if top_k > 0:
        sure_in = ok & (gt_hi.sum(1) < top_k)
        sure_out = sure_out | (ok & (gt_lo.sum(1) >= top_k))
    p = p32(top_p)
    if p < 1.0 and bool(ok.any()):
        w = torch.where(ok, torch.exp(z - z[ok].max()), torch.zeros_like(z))
        maybe = ok & ~sure_out
        M_lo, M_hi = (w * sure_in).sum(), (w * maybe).sum()
        U = (gt_hi & maybe[None, :]).double() @ w
        Lo = (gt_lo & sure_in[None, :]).double() @ w
        e = math.exp(eps)
        sure_out = sure_out | (ok & (Lo / e >= p * M_hi * e))
        sure_in = sure_in & (U * e < p * M_lo / e)
    return sure_in, sure_out


def hf_pin_case(trials=60):
    """kept_ref against the installed transformers' TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on random float64 rows
    without ties: the sets of finite entries are equal"""
    tf = pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(3)
    n_checked = 0
    for t in range(trials):
        n = int(torch.randint(1, 300, (1,), generator=g))
        tau = (0.5, 1.0, 2.0, 0.7)[t % 4]
        k = (0, 1, 2, max(1, n - 1), n, n + 1, 7)[t % 7]
        p = (1.0, 1e-6, 0.3, 0.9, 1 - 1e-6, 0.5)[t % 6]
        logits = torch.randn(1, n, generator=g, dtype=torch.float64) * 2
        assert len(torch.unique(logits)) == n
        s = tf.TemperatureLogitsWarper(tau)(None, logits.clone())
        if k > 0:
            s = tf.TopKLogitsWarper(top_k=k)(None, s)
        if p < 1.0:
            s = tf.TopPLogitsWarper(top_p=p)(None, s)
        keep, _, margin = kept_ref(logits[0] / tau, k, p)
        if margin < 1e-9:
            continue          # (HF sums in another order: a boundary mass on top_p itself is not a difference of semantics)
        assert torch.equal(torch.isfinite(s[0]), keep), (n, tau, k, p)
        n_checked += 1
    assert n_checked >= trials - 3


# ---------------------------------------------------------------------------------------------------------
# the kernels one by one: p5_op_trunc_cut, p5_op_trunc_ce_fwd, p5_op_trunc_ce_bwd
# ---------------------------------------------------------------------------------------------------------
OP_FANS = (1, 2, 3, 32, 33, 255, 256, 257, 1025, STAGE + 1)
OP_KINDS = ("normal", "neginf", "excluded", "equal", "triples")
OP_TOP_P = (1e-6, 0.3, 0.9, 1 - 1e-6)
OP_V = 4096


def _op_params(nc):
    ks = sorted({k for k in (1, 2, nc - 1, nc, nc + 1) if k >= 1})
    out = [(k, 1.0) for k in ks] + [(0, p) for p in OP_TOP_P]
    out += [(2, 0.3), (max(1, nc - 1), 0.9), (max(1, nc // 2), 0.3), (nc + 1, 1 - 1e-6)]
    return out


def _op_rows(fan, tau, seed):
    """One node of `fan` leaf children and one row of logits per kind.  The values are tau * y with y drawn at a spread of 0.5: z = y for
    tau in {0.5, 1, 2} exactly (powers of two), and no child's probability falls below 1.1e-5 at these fan-outs, so top_p = 1 - 1e-6 keeps a
    row whole by a margin the assertion of op_case can see.  `triples`: every value three times (ties at most k-th places and across most
    nucleus boundaries); `equal`: one value."""
    g = torch.Generator().manual_seed(seed)
    toks = torch.sort(torch.randperm(OP_V - 2, generator=g)[:fan] + 2).values
    rows, excl = [], []
    for kind in OP_KINDS:
        y = torch.randn(fan, generator=g) * 0.5
        ex = torch.zeros(fan, dtype=torch.bool)
        if kind == "equal":
            y = torch.full((fan,), 0.25)
        elif kind == "triples":
            y = (torch.randn((fan + 2) // 3, generator=g) * 0.5).repeat_interleave(3)[torch.randperm(((fan + 2) // 3) * 3, generator=g)][:fan]
        elif kind == "neginf":
            y[torch.rand(fan, generator=g) < 0.3] = NEG
            y[int(torch.randint(0, fan, (1,), generator=g))] = 0.1          # (at least one finite child)
        elif kind == "excluded":
            ex[1::3] = True
        v = torch.full((OP_V,), float("nan"))
        v[:] = torch.randn(OP_V, generator=g) * 3          # (columns that are no children must not matter)
        v[toks] = (y * tau).float()
        rows.append(v)
        excl.append(ex)
    return toks, torch.stack(rows), torch.stack(excl)


def op_case(be, tau, fans=OP_FANS, seed=0):
    """Every fan-out x (top_k, top_p) x row kind at temperature tau, logits given.  The top-k cut and the kept count are exact; so is the
    top-p cut, every row being asserted farther than P_MARGIN from a boundary (a condition on the inputs).  lse / nll / dlogits are held to
    the bounds of trie_loss_cases.op_case (ELEM_R32 |x| + ATTN_TAU[0] S), dlogits are exactly 0 outside the kept set, state 3 sits exactly
    where the reference puts the label below the cut."""
    from tests.elem_matrix import ELEM_R32, ELEM_TINY
    lib, st = be.lib, be.stream_ptr()
    tau0 = ATTN_TAU[0]
    R = len(OP_KINDS)
    ldd = (OP_V + 63) // 64 * 64
    ldl = ldd + 8
    worst, n_tie_k, n_tie_p, n_state3, n_cases = 0.0, 0, 0, 0, 0
    for fan in fans:
        # the inputs are CHOSEN so that every row lies farther than P_MARGIN from every nucleus boundary (judged by the float64 reference
        # alone): the first seed of seed + fan, + 1000, + 2000, ... whose rows do; the assertion below then holds by construction
        for attempt in range(200):
            toks, logit_rows, ex = _op_rows(fan, tau, seed + fan + 1000 * attempt)
            z_try = torch.where(ex, torch.full((len(OP_KINDS), fan), NEG, dtype=torch.float64),
                                (logit_rows[:, toks] / torch.tensor(tau, dtype=torch.float32)).double())
            if all(kept_ref(z_try[r], k, p)[2] > 2 * P_MARGIN for k, p in _op_params(fan) for r in range(len(OP_KINDS))):
                break
        # CSR: node 0 = root with one edge to node 1; node 1 has the `fan` children (leaves 2 .. fan + 1)
        off = np.asarray([0, 1, 1 + fan] + [1 + fan] * fan, dtype=np.int32)
        tok = np.concatenate([[0], toks.numpy()]).astype(np.int32)
        nxt = np.concatenate([[1], np.arange(2, fan + 2)]).astype(np.int32)
        n_nodes = fan + 2
        words = (n_nodes + 31) // 32
        excl = np.zeros((R, words), dtype=np.uint32)
        for r in range(R):
            for i in np.nonzero(ex[r].numpy())[0]:
                excl[r, (i + 2) >> 5] |= np.uint32(1) << np.uint32((i + 2) & 31)
        L = torch.full((R, ldl), float("nan"))
        L[:, :OP_V] = logit_rows
        z = torch.where(ex, torch.full((R, fan), NEG, dtype=torch.float64), (L[:, toks] / torch.tensor(tau, dtype=torch.float32)).double())
        d_off, d_tok, d_nxt = (dev(be, torch.from_numpy(a)) for a in (off, tok, nxt))
        d_excl = dev(be, torch.from_numpy(excl.view(np.int32)))
        Ld = dev(be, L)
        node = dev(be, torch.ones(R, dtype=torch.int32))
        g = torch.Generator().manual_seed(seed + 7 * fan)
        dnll = torch.randn(R, generator=g).float()
        attn = torch.ones(R, 1, dtype=torch.int64)
        attn[1] = 0
        dnlld, attnd = dev(be, dnll), dev(be, attn)
        gscale = float(torch.tensor(1.0 / R, dtype=torch.float32))
        for ci, (k, p) in enumerate(_op_params(fan)):
            n_cases += 1
            ref = [kept_ref(z[r], k, p) for r in range(R)]
            for r in range(R):
                assert ref[r][2] > P_MARGIN, f"fan {fan} row {OP_KINDS[r]} top_p {p}: a boundary mass lies {ref[r][2]:.2e} (relative) from top_p: choose other inputs"
            keep = torch.stack([q[0] for q in ref])
            cut_ref = torch.tensor([q[1] for q in ref], dtype=torch.float64)
            md = f"trunc fan {fan} tau {tau} top_k {k} top_p {p}"
            # ---- the cut ----
            c_d, n_d = dev(be, _sentinel((R + 1,), torch.float32)), dev(be, torch.full((R + 1,), trie_loss_cases.I32_SENT, dtype=torch.int32))
            be.check(lib.p5_op_trunc_cut(P(c_d), P(n_d), P(Ld), P(node), P(d_off), P(d_tok), P(d_nxt), P(d_excl), words, tau, k, p, R, 1, ldl, st), "trunc_cut")
            sync(be)
            ch, nh = c_d.cpu(), n_d.cpu()
            _guard_intact(f"{md} cut", ch, R)
            assert int(nh[R]) == trie_loss_cases.I32_SENT
            assert np.array_equal(nh[:R].numpy(), keep.sum(1).to(torch.int32).numpy()), (md, nh[:R].tolist(), keep.sum(1).tolist())
            assert torch.equal(ch[:R].double(), cut_ref), (md, ch[:R].tolist(), cut_ref.tolist())
            if k > 0 and p == 1.0:
                n_tie_k += int((keep.sum(1) > k).sum())
            if p < 1.0:
                for r in range(R):          # a tie group that HF's positional rule would cut inside
                    grp = keep[r] & (z[r] == cut_ref[r])
                    if int(grp.sum()) >= 2:
                        w = torch.where(keep[r] | (z[r] < cut_ref[r]), torch.exp(z[r] - z[r][torch.isfinite(z[r])].max()), torch.zeros(fan, dtype=torch.float64))
                        kk = kept_ref(z[r], k, 1.0)[0]
                        w = w * kk
                        above = float(w[z[r] > cut_ref[r]].sum())
                        one = float(w[grp][0])
                        n_tie_p += int(above + (int(grp.sum()) - 1) * one >= p32(p) * float(w.sum()))
            # ---- labels: the largest child (always kept) on even cases, the median allowed child on odd ones ----
            lab_pos = []
            for r in range(R):
                fin = torch.nonzero(torch.isfinite(z[r])).flatten()
                order = fin[torch.argsort(z[r][fin], descending=True, stable=True)]
                lab_pos.append(int(order[0] if ci % 2 == 0 else order[len(order) // 2]))
            labels = toks[lab_pos].to(torch.int64).view(R, 1)
            away = torch.tensor([not bool(keep[r, lab_pos[r]]) for r in range(R)])
            n_state3 += int(away.sum())
            labd = dev(be, labels)
            zk = torch.where(keep, z, torch.full_like(z, NEG))
            mx = zk.max(1).values
            lsum = torch.log(torch.exp(zk - mx[:, None]).sum(1))
            lse = mx + lsum
            zl = z[torch.arange(R), lab_pos]
            nll = torch.where(away, torch.zeros(R, dtype=torch.float64), lse - zl)
            S_lse = mx.abs() + lsum.abs()
            S_nll = S_lse + zl.abs()
            single = keep.sum(1) == 1
            for dtype in (0, 1):
                o_n, o_l, o_c = (dev(be, _sentinel((R + 1,), torch.float32)) for _ in range(3))
                st_d = dev(be, torch.cat([torch.zeros(R, dtype=torch.int32), torch.tensor([trie_loss_cases.I32_SENT], dtype=torch.int32)]))
                be.check(lib.p5_op_trunc_ce_fwd(dtype, P(o_n), P(o_l), P(o_c), P(st_d), P(Ld), P(labd), P(node), P(d_off), P(d_tok), P(d_nxt), P(d_excl), words,
                                                tau, k, p, R, 1, ldl, st), "trunc_ce_fwd")
                sync(be)
                hn, hl, hc, hs = o_n.cpu(), o_l.cpu(), o_c.cpu(), st_d.cpu()
                for t_, nm in ((hn, "nll"), (hl, "lse"), (hc, "row_cut")):
                    _guard_intact(f"{md} {nm}", t_, R)
                assert int(hs[R]) == trie_loss_cases.I32_SENT
                assert torch.equal(hc[:R].double(), cut_ref), (md, "row_cut")
                assert torch.equal(hs[:R] == TRUNCATED, away) and bool(((hs[:R] == SCORED) | (hs[:R] == TRUNCATED)).all()), (md, hs[:R].tolist(), away.tolist())
                worst = max(worst, _elem_check(f"{md} dtype {dtype} lse", hl[:R], lse, ELEM_R32 * lse.abs() + tau0 * S_lse))
                worst = max(worst, _elem_check(f"{md} dtype {dtype} nll", hn[:R], nll, ELEM_R32 * nll.abs() + tau0 * S_nll, zero=away))
                assert bool((hn[:R][single & ~away] == 0).all()), f"{md}: one kept child: nll exactly 0"
            # ---- backward: lse and cut as stored, the states of the forward ----
            state_in = dev(be, torch.where(away, TRUNCATED, SCORED).to(torch.int32))
            lse_in = lse.float()
            lsed, cutd = dev(be, lse_in), dev(be, cut_ref.float())
            prob = torch.zeros(R, ldd, dtype=torch.float64)
            onehot = torch.zeros(R, ldd, dtype=torch.float64)
            inside = torch.zeros(R, ldd, dtype=torch.bool)
            for r in range(R):
                kt = toks[keep[r]]
                prob[r, kt] = torch.exp(z[r][keep[r]] - lse_in[r].double())
                inside[r, kt] = True
                onehot[r, toks[lab_pos[r]]] = 1.0
            for dtype in (0, 1):
                tt, r_ = TT[dtype], _elem_r(dtype)
                for seeding in ("dnll", "mask"):
                    gref = dnll.double() if seeding == "dnll" else torch.where(attn.view(R) != 0, torch.full((R,), gscale, dtype=torch.float64), torch.zeros(R, dtype=torch.float64))
                    gref = torch.where(away, torch.zeros(R, dtype=torch.float64), gref)
                    want = (prob - onehot) * gref[:, None] / tau
                    bound = r_ * want.abs() + (tau0 * (prob + onehot) + ELEM_TINY) * gref.abs()[:, None] / tau
                    dl = dev(be, _sentinel((R + 1, ldd), tt))
                    be.check(lib.p5_op_trunc_ce_bwd(dtype, P(dl), P(Ld), P(lsed), P(cutd), P(labd), P(node), P(state_in), P(dnlld) if seeding == "dnll" else None,
                                                    P(d_off), P(d_tok), P(d_nxt), P(d_excl), words, tau, R, 1, ldl, ldd, P(attnd), gscale, st), "trunc_ce_bwd")
                    sync(be)
                    dh = dl.cpu()
                    _guard_intact(f"{md} dlogits", dh, R)
                    got = dh[:R].float()
                    assert bool((got[~inside] == 0).all()), f"{md}: non-zero dlogits outside the kept set"
                    assert bool((got[away] == 0).all()), f"{md}: a row whose label was truncated away must be a zero row"
                    worst = max(worst, _elem_check(f"{md} {seeding} dtype {dtype} dlogits", dh[:R], want, bound))
    print(f"[trunc op] tau {tau}: {n_cases} (fan-out, top_k, top_p) cases x {R} rows, worst err / bound {worst:.3g}; ties across the k-th place {n_tie_k}, "
          f"tie groups across the nucleus boundary {n_tie_p}, labels truncated away {n_state3}")
    if len(fans) >= 5:
        assert n_tie_k >= 5 and n_tie_p >= 3 and n_state3 >= 10, (n_tie_k, n_tie_p, n_state3)
    return worst


def op_errors_case(be):
    lib, st = be.lib, be.stream_ptr()
    t = dev(be, torch.zeros(64, dtype=torch.float32))
    i = dev(be, torch.zeros(64, dtype=torch.int32))
    for k, p in ((-1, 1.0), (0, 0.0), (0, 1.5), (0, float("nan"))):
        assert lib.p5_op_trunc_cut(P(t), P(i), P(t), P(i), P(i), P(i), P(i), None, 0, 1.0, k, ctypes.c_float(p), 1, 1, 8, st) != 0, (k, p)
        assert b"top_" in lib.p5_last_error()


# ---------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------
def _z(ref, b, node, tau, ex):
    ok = ref.allowed(node, ex)
    return torch.where(ok, ref.z[(b, node)] / tau, torch.full((), NEG, dtype=torch.float64))


def trunc_replay_check(out, ref, items, B, S, seed, streams, draw_base, tau, tol, top_k, top_p, excl=None, eos=1, cap=UNDECIDED_CAP, tag=""):
    """Every draw and step against the three-way classification of the node's children under logit errors within tol: no drawn child is
    surely removed; its perturbed value is within 2 tol / tau of the maximum over the surely-kept children; its log-probability lies in
    [z_c - lse(surely kept + undecided) - tol, z_c - lse(surely kept) + tol] -- at a DECIDED node (no undecided child) that is: the child
    is in the reference's kept set, within 2 tol / tau of the maximum over it, its log-probability within tol of log-softmax over it, and
    exactly 0.0 where one child is kept.  cap: at most that share of the visited (user, node) pairs may be undecided (None: no cap).
    Returns (visited pairs, undecided pairs, users with a surely-removed child on their paths)."""
    seq, lp, tlp = out["sequences"].cpu(), out["sequences_logprob"].cpu(), out["token_logprobs"].cpu()
    T = seq.shape[1]
    assert seq.shape == (B * S, T) and tlp.shape == (B * S, T - 1)
    eps = tol / tau
    visited, undecided, bites = set(), set(), set()
    cls = {}
    worst_gap, worst_lp = 0.0, 0.0
    for b in range(B):
        rows = [seq[b * S + s].tolist() for s in range(S)]
        lens = [q.index(eos) if eos in q else None for q in rows]
        assert all(n is not None for n in lens), f"user {b}: a draw without </s>"
        ref.add(b, [q[:n + 1] for q, n in zip(rows, lens)])
        ex = None if excl is None else excl[b]
        for s in range(S):
            q, n = rows[s], lens[s]
            nodes = ref.walk(q[:n + 1])
            assert ref.children(nodes[-1])[0].size == 0, "the sequence must end at a leaf"
            for t in range(1, n + 1):
                node = nodes[t - 1]
                toks, _ = ref.children(node)
                z = _z(ref, b, node, tau, ex)
                if (b, node) not in cls:
                    cls[(b, node)] = classify(z, top_k, top_p, eps) + (kept_ref(z, top_k, top_p)[0],)
                sure_in, sure_out, keep = cls[(b, node)]
                und = torch.isfinite(z) & ~sure_in & ~sure_out
                visited.add((b, node))
                if bool(und.any()):
                    undecided.add((b, node))
                else:
                    assert torch.equal(sure_in, keep)
                if bool((sure_out & torch.isfinite(z)).any()):
                    bites.add(b)
                c = int(np.nonzero(toks == q[t])[0][0])
                where = f"user {b} draw {s} step {t}"
                assert not bool(sure_out[c]), f"{where}: a child that is surely truncated away (or excluded) was drawn"
                g = -torch.log(-torch.log(uniforms(seed, int(streams[b]), draw_base + s, t, len(toks))))
                pert = z + g
                if bool(sure_in.any()):
                    gap = float(pert[sure_in].max() - pert[c])
                    worst_gap = max(worst_gap, gap)
                    assert gap <= 2 * tol / tau, f"{where}: perturbed value {gap:.3e} below the maximum over the kept set (bound {2 * tol / tau:.1e})"
                got = float(tlp[b * S + s, t - 1])
                hi = float(z[c] - torch.logsumexp(z[sure_in], 0)) if bool(sure_in.any()) else 0.0
                lo = float(z[c] - torch.logsumexp(z[sure_in | und], 0))
                assert lo - tol <= got <= min(hi, 0.0) + tol, f"{where}: token log-probability {got} outside [{lo}, {hi}] +- {tol}"
                if not bool(und.any()):
                    worst_lp = max(worst_lp, abs(got - hi))
                    if int(keep.sum()) == 1:
                        assert got == 0.0, f"{where}: one kept child, log-probability {got!r} instead of exactly 0"
            assert bool((tlp[b * S + s, n:] == 0).all())
            assert abs(float(lp[b * S + s]) - float(tlp[b * S + s].double().sum())) <= 1e-5 * max(1, n)
    print(f"[trunc sample{tag}] B={B} S={S} tau={tau} top_k={top_k} top_p={top_p}: {len(undecided)} of {len(visited)} (user, node) pairs undecided at {tol:.0e}; "
          f"largest shortfall {worst_gap:.3e} (bound {2 * tol / tau:.1e}); max |token log-prob - reference| at decided nodes {worst_lp:.3e}")
    if cap is not None:
        assert len(undecided) <= cap * len(visited), f"{len(undecided)} of {len(visited)} visited (user, node) pairs are undecided: more than {cap:.0%}"
    return len(visited), len(undecided), bites


def sample_case(be, ocfg, B, L, items, S, top_k=0, top_p=1.0, dtype="fp32", tau=1.0, seed=1, streams=None, draw_base=0, excluded_items=None, batch_seed=5,
                capped=True, tag=""):
    """sample_items(top_k=, top_p=) on a synthetic batch: fp32 the replay check with the cap, bf16 (and fp32 with capped=False) the three-way
    check, which must bite"""
    m, params = sample_cases.make_model(be, ocfg, dtype)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, batch_seed)
    ct = rank_cases.compiled(items)
    out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=tau, seed=seed, streams=streams,
                         draw_base=draw_base, excluded_items=excluded_items, top_k=top_k, top_p=top_p)
    assert m.last_generate_path == "sample"
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    excl = None if excluded_items is None else ct.excluded_bitmap(excluded_items)
    fp32 = dtype == "fp32"
    _, _, bites = trunc_replay_check(out, ref, items, B, S, seed, streams if streams is not None else list(range(B)), draw_base, tau,
                                     FP32_TOL if fp32 else BF16_TOL, top_k, top_p, excl=excl, cap=UNDECIDED_CAP if fp32 and capped else None,
                                     tag=f"{tag} {dtype}")
    if not (fp32 and capped):
        assert bites == set(range(B)), f"the three-way check is vacuous for users {sorted(set(range(B)) - bites)}: no visited node has a surely-removed child"
    return out, m, ref, (ids, ww, mask, ct)


def crn_case(be, ocfg, items, B=2, L=12, S=12, top_k=0, top_p=1.0, tau=1.0, seed=3):
    """common random numbers: a draw whose UNTRUNCATED path stays inside the reference's kept sets at decided nodes is the same draw under
    truncation, bit for bit, with token log-probabilities >= the untruncated ones - 1e-6"""
    m, params = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=tau, seed=seed)
    plain = m.sample_items(**kw)
    trunc = m.sample_items(top_k=top_k, top_p=top_p, **kw)
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    seq, tlp, seq_t, tlp_t = plain["sequences"].cpu(), plain["token_logprobs"].cpu(), trunc["sequences"].cpu(), trunc["token_logprobs"].cpu()
    same = 0
    for b in range(B):
        rows = [seq[b * S + s].tolist() for s in range(S)]
        ref.add(b, [q[:q.index(1) + 1] for q in rows])
        for s in range(S):
            q = rows[s]
            n = q.index(1)
            nodes = ref.walk(q[:n + 1])
            inside = True
            for t in range(1, n + 1):
                toks, _ = ref.children(nodes[t - 1])
                z = _z(ref, b, nodes[t - 1], tau, None)
                sure_in, sure_out = classify(z, top_k, top_p, FP32_TOL / tau)
                c = int(np.nonzero(toks == q[t])[0][0])
                inside = inside and bool((sure_in | sure_out).all()) and bool(sure_in[c])
            if inside:
                same += 1
                assert torch.equal(seq_t[b * S + s], seq[b * S + s]), f"user {b} draw {s}: the truncated draw left a path that lies inside the kept sets"
                assert bool((tlp_t[b * S + s] >= tlp[b * S + s] - 1e-6).all()), f"user {b} draw {s}: a truncated log-probability below the untruncated one"
    print(f"[trunc crn] top_k={top_k} top_p={top_p}: {same} of {B * S} untruncated draws lie inside the kept sets")
    assert same >= max(2, B * S // 6), same
    assert not torch.equal(seq, seq_t) or same == B * S


def greedy_case(be, ocfg, items, B=3, L=14, S=3):
    """top_k = 1 is the float64 greedy descent wherever the top gap exceeds 2 tol; every log-probability is exactly 0"""
    m, params = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=8, top_k=1)
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    seq = out["sequences"].cpu()
    assert bool((out["token_logprobs"].cpu() == 0).all()) and bool((out["sequences_logprob"].cpu() == 0).all())
    checked = 0
    for b in range(B):
        q, node = [0], ref.walk([0])[0]
        while ref.children(node)[0].size:
            ref.add(b, [q + [int(ref.children(node)[0][0])]])          # (any child: the logits of `node` are those of the prefix q)
            toks, kids = ref.children(node)
            z = ref.z[(b, node)]
            top = torch.topk(z, min(2, len(toks)))
            if len(toks) > 1 and float(top.values[0] - top.values[1]) <= 2 * FP32_TOL:
                break
            c = int(top.indices[0])
            q.append(int(toks[c]))
            node = int(kids[c])
            for s in range(S):
                assert int(seq[b * S + s, len(q) - 1]) == q[-1], f"user {b} draw {s} position {len(q) - 1}: not the greedy child"
            checked += 1
    assert checked >= 3 * B


def item_probs(ref, b, items, tau, top_k, top_p, excl_row=None):
    """exact probability of every item under truncation: the product of the truncated conditionals along its path (0 behind a removed child)"""
    ref.add(b, items)
    p = torch.zeros(len(items), dtype=torch.float64)
    for i, q in enumerate(items):
        nodes, lp = ref.walk(q), 0.0
        for t in range(len(q) - 1):
            toks, _ = ref.children(nodes[t])
            z = _z(ref, b, nodes[t], tau, excl_row)
            keep = kept_ref(z, top_k, top_p)[0]
            c = int(np.nonzero(toks == q[t + 1])[0][0])
            lp = lp + (float(z[c] - torch.logsumexp(z[keep], 0)) if bool(keep[c]) else NEG)
        p[i] = math.exp(lp)
    return p


def frequency_case(be, ocfg, S, top_k=0, top_p=1.0, seeds=(1, 2), B=2, L=12):
    items = sample_cases.freq_items()
    m, params = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    for seed in seeds:
        out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=seed, top_k=top_k, top_p=top_p)
        idx = out["item_index"].cpu()
        for b in range(B):
            counts = np.bincount(idx[b].numpy(), minlength=len(items))
            p = item_probs(ref, b, items, 1.0, top_k, top_p).numpy()
            assert abs(p.sum() - 1.0) < 1e-9 and int((p == 0).sum()) >= 5, "the truncation must remove items"
            # an item behind an undecided child may carry the other side's probability: leave the users out whose catalogue has one
            und = 0
            for node in {n for q in items for n in ref.walk(q)[:-1]}:
                z = _z(ref, b, node, 1.0, None)
                si, so = classify(z, top_k, top_p, FP32_TOL)
                und += int((torch.isfinite(z) & ~si & ~so).sum())
            assert und == 0, f"user {b}: {und} undecided children in the catalogue: choose another top_k / top_p"
            ok, n_bad, n_bins = sample_cases.bins_ok(counts, p, S)
            print(f"[trunc freq] top_k={top_k} top_p={top_p} seed {seed} user {b}: {n_bins} bins, {n_bad} outside 5 sigma + 1, {int((p == 0).sum())} items of probability 0")
            assert ok, f"seed {seed} user {b}: {n_bad} of {n_bins} bins outside the bound"
            assert int(counts[p == 0].sum()) == 0, "an item of probability 0 was drawn"


def determinism_case(be, ocfg, B=3, L=14, S=10, top_k=3, top_p=0.8):
    """user chunks, draw ranges, streams and lanes return the same bits under truncation"""
    items = cases.make_items(40, 5, hi=60)
    m, _ = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, top_k=top_k, top_p=top_p)
    a = m.sample_items(num_samples=S, seed=9, **kw)
    sample_cases.same_bits(a, m.sample_items(num_samples=S, seed=9, **kw), "two calls with one seed")
    assert not torch.equal(a["item_index"].cpu(), m.sample_items(num_samples=S, seed=10, **kw)["item_index"].cpu())
    calls = m.sample_stats["engine_calls"]
    m.wide_max_rows = 8
    sample_cases.same_bits(a, m.sample_items(num_samples=S, seed=9, **kw), "wide_max_rows = 8")
    assert m.sample_stats["engine_calls"] - calls == 2 * B
    m.wide_max_rows = type(m).wide_max_rows
    lo = m.sample_items(num_samples=4, seed=9, **kw)
    hi = m.sample_items(num_samples=S - 4, seed=9, draw_base=4, **kw)
    for k in KEYS:
        v = (lambda t: t.cpu()) if k == "item_index" else (lambda t: t.cpu().view(B, -1, t.shape[-1]) if t.dim() == 2 else t.cpu().view(B, -1))
        assert torch.equal(torch.cat([v(lo[k]), v(hi[k])], 1), v(a[k])), f"{k}: draws 0-3 and 4-9 in two calls"
    one = m.sample_items(input_ids=ids[1:2], attention_mask=mask[1:2], whole_word_ids=ww[1:2], trie=ct, num_samples=S, seed=9, streams=[1], top_k=top_k,
                         top_p=top_p)
    for k in KEYS:
        v = (lambda t: t.cpu()) if k == "item_index" else (lambda t: t.cpu().view(-1, S, t.shape[-1]) if t.dim() == 2 else t.cpu().view(-1, S))
        assert torch.equal(v(one[k])[0], v(a[k])[1]), f"{k}: user 1 alone with streams=[1]"
    # forced prefix on and off: the same draws (the prefix is forced under any truncation)
    m.prefix_fast_forward = False
    b = m.sample_items(num_samples=S, seed=9, **kw)
    assert torch.equal(a["sequences"].cpu(), b["sequences"].cpu()) or float((a["sequences"].cpu() == b["sequences"].cpu()).all(1).float().mean()) >= 0.5
    m.prefix_fast_forward = True
    # lanes
    batches = [dict(num_samples=S, seed=40 + i) for i in range(3)]

    def one_call(bkw):
        out = m.sample_items(**bkw, **kw)
        return {k: out[k].cpu() for k in KEYS}
    want = [one_call(x) for x in batches]
    for w, g in zip(want, m.map_lanes(one_call, batches, lanes=2)):
        sample_cases.same_bits(w, g, "map_lanes")


def off_case(be, ocfg, B=2, L=12, S=5):
    """top_k = 0 / top_k >= max_children with top_p = 1 is a call without the arguments, bit for bit -- through the model and through the
    truncated C entry point; p5_sample_truncated_workspace_bytes is exact"""
    from openp5_amd import _abi
    from openp5_amd.model import _ptr
    assert len(_abi.PROTOTYPES["p5_sample_truncated_workspace_bytes"][1]) == 7 and len(_abi.PROTOTYPES["p5_sample_items_truncated"][1]) == 27
    items = cases.make_items(40, 5, hi=60)
    m, _ = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=5)
    m.prefix_fast_forward = False          # (the raw calls below set no forced prefix)
    want = m.sample_items(**kw)
    sample_cases.same_bits(want, m.sample_items(top_k=0, top_p=1.0, **kw), "top_k=0, top_p=1.0")
    sample_cases.same_bits(want, m.sample_items(top_k=ct.max_children, **kw), "top_k = max_children")
    sample_cases.same_bits(want, m.sample_items(top_k=10 ** 6, top_p=1, **kw), "top_k > max_children")
    dv = m._be.device
    off, tok, nxt = ct.device_arrays(dv)
    ids_d, ww_d, mask_d = (m._i64(t, dv) for t in (ids, ww, mask))
    eng, T = m._cur_lane().engine, int(ct.max_depth)
    plain = int(be.lib.p5_sample_workspace_bytes(eng, B, L, S, T, ct.max_children, 0))
    need = int(be.lib.p5_sample_truncated_workspace_bytes(eng, B, L, S, T, ct.max_children, 0))
    assert need == plain + (B * S * ct.max_children * 4 + 255) // 256 * 256
    assert int(be.lib.p5_sample_truncated_workspace_bytes(eng, B, L, 4097, T, ct.max_children, 0)) == -1
    assert int(be.lib.p5_sample_truncated_workspace_bytes(eng, B, L, S, 1, ct.max_children, 0)) == -1
    raw = torch.zeros(need + 256, dtype=torch.uint8, device=dv)
    skew = (-raw.data_ptr()) % 256
    ws = raw[skew:skew + need]
    guard = raw[skew + need:].clone()
    streams = torch.arange(B, dtype=torch.int32, device=dv)
    seq = torch.zeros(B, S, T, dtype=torch.int32, device=dv)
    lp = torch.zeros(B, S, dtype=torch.float32, device=dv)
    tlp = torch.zeros(B, S, T, dtype=torch.float32, device=dv)
    ln = torch.zeros(B, S, dtype=torch.int32, device=dv)

    def call(nbytes, k, p):
        return be.lib.p5_sample_items_truncated(eng, _ptr(ids_d), _ptr(ww_d), _ptr(mask_d), B, L, S, T, _ptr(off), _ptr(tok), _ptr(nxt), None, 0, ct.max_children,
                                                5, _ptr(streams), 0, 1.0, k, ctypes.c_float(p), _ptr(seq), _ptr(lp), _ptr(tlp), _ptr(ln), _ptr(ws), nbytes,
                                                m._be.stream_ptr())
    assert call(need - 1, 2, 0.9) != 0
    assert b"workspace" in be.lib.p5_last_error()
    assert call(need, 0, 1.0) == 0
    sync(be)
    assert torch.equal(seq.view(B * S, T).cpu().to(torch.int64), want["sequences"].cpu()) and torch.equal(lp.view(-1).cpu(), want["sequences_logprob"].cpu())
    assert torch.equal(tlp.view(B * S, T)[:, 1:].cpu(), want["token_logprobs"].cpu())
    assert call(need, 2, 0.9) == 0
    sync(be)
    assert torch.equal(raw[skew + need:], guard), "the call wrote behind the bytes it asked for"
    tr = m.sample_items(top_k=2, top_p=0.9, **kw)
    assert torch.equal(seq.view(B * S, T).cpu().to(torch.int64), tr["sequences"].cpu()) and torch.equal(lp.view(-1).cpu(), tr["sequences_logprob"].cpu())
    for k, p in ((-1, 1.0), (0, 0.0), (0, 1.5)):
        assert call(need, k, p) != 0, (k, p)
        assert b"top_" in be.lib.p5_last_error()


def errors_case(be, ocfg):
    from openp5_amd.trie import Trie
    items = cases.make_items(20, 5, hi=60)
    m, _ = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, labels, out_attn, _ = trie_loss_cases.item_batch(ocfg, items, 2, 12, 6, 5, stray=False)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww)
    for bad in (dict(top_k=-1), dict(top_p=0), dict(top_p=1.5), dict(top_p=float("nan")), dict(top_k=1.5)):
        with pytest.raises(ValueError, match="top_"):
            m.sample_items(trie=Trie(items), **bad, **kw)
        with pytest.raises(ValueError, match="top_"):
            m(labels=labels, trie=Trie(items), **bad, **kw)
        with pytest.raises(ValueError, match="top_"):
            m.loss_and_backward(ids, ww, mask, labels, out_attn, trie=Trie(items), **bad)
    with pytest.raises(ValueError, match="top_k") as ei:
        m.generate(do_sample=True, trie=Trie(items), num_beams=1, top_k=5, **kw)
    assert "supports" in str(ei.value) and "sample_items(top_k=, top_p=)" in str(ei.value)
    # a failed setup leaves nothing armed
    with torch.no_grad():
        a = m(labels=labels, **kw)["loss"].cpu()
        with pytest.raises(ValueError):
            m(labels=labels, trie=Trie(items), top_p=0.0, **kw)
        assert torch.equal(a, m(labels=labels, **kw)["loss"].cpu())


# ---------------------------------------------------------------------------------------------------------
# the item loss
# ---------------------------------------------------------------------------------------------------------
def oracle_trunc_nll(Pq, ocfg, ids, ww, mask, labels, ct, tau, excl, dp, top_k, top_p, tol=FP32_TOL):
    """trie_loss_cases.oracle_item_nll with the children outside the kept set masked to -inf, the set taken from the detached float64
    logits.  Returns (nll [B * T], states with 3 where the label is truncated away, scored rows with an undecided child)."""
    enc = O.encoder_forward(Pq, ocfg, ids, ww, mask, dp)
    dec = O.decoder_forward(Pq, ocfg, O.shift_right(labels, ocfg), enc, mask, dp)
    logits = O.lm_logits(Pq, ocfg, dec)
    B, T = labels.shape
    node, state = trie_loss_cases.walk(ct.child_off, ct.child_tok, ct.child_node, labels.numpy(), excl, ocfg.pad_id, ocfg.eos_id)
    state = state.copy()
    rows, undecided = [], []
    oracle_trunc_nll.live = 0          # scored rows with a kept label and at least two kept children: the rows that carry a gradient
    for b in range(B):
        for t in range(T):
            if state[b, t] != SCORED:
                rows.append(logits.new_zeros(()))
                continue
            c = trie_loss_cases.allowed_children(ct.child_off, ct.child_tok, ct.child_node, int(node[b, t]), None if excl is None else excl[b])
            z = logits[b, t, c] / tau
            keep = kept_ref(z.detach(), top_k, top_p)[0]
            si, so = classify(z.detach(), top_k, top_p, tol / tau)
            if not bool((si | so).all()):
                undecided.append((b, t))
            j = c.index(int(labels[b, t]))
            if not bool(keep[j]):
                state[b, t] = TRUNCATED
                rows.append(logits.new_zeros(()))
                continue
            oracle_trunc_nll.live += int(keep.sum()) >= 2
            rows.append(-torch.log_softmax(z[keep], 0)[int(keep[:j].sum())])
    return torch.stack(rows), state, undecided


def model_case(be, ocfg, items, top_k=0, top_p=1.0, B=4, L=14, T=6, dropout=0.0, tau=1.0, excluded=False, seed=trie_loss_cases.MODEL_SEED):
    """forward(trie=, top_k=, top_p=) + runner loss + backward against float64 autograd on the oracle with the non-kept children masked and
    the set detached: trie_loss_cases.model_case's tolerances (nll 2e-5, gradients 2e-4); the states (3 included) are the reference's.
    The labels of the first B - 2 samples are DRAWN under the same truncation (a random item is truncated away at the first branching
    node, and the nodes behind it have one child: nothing would carry a gradient); sample B - 2 keeps its random item (state 3), the last
    one leaves the trie.  The case asserts that no scored row has an undecided child -- the kept sets are then the same on both sides --
    and that rows with a gradient exist."""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, pick = trie_loss_cases.item_batch(ocfg, items, B, L, T, seed)
    excluded_items = trie_loss_cases._excluded_for(items, pick, B) if excluded else None
    excl = ct.excluded_bitmap(excluded_items) if excluded else None
    m0 = cases.build_model(be, ocfg, params, "fp32", 0.0)
    m0.eval()
    drawn = m0.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=1, temperature=tau, seed=11,
                            excluded_items=excluded_items, top_k=top_k, top_p=top_p)["sequences"].cpu()
    for b in range(B - 2):
        q = drawn[b, 1:].tolist()
        n = min(T, q.index(ocfg.eos_id) + 1)
        labels[b], out_attn[b] = 0, 0
        labels[b, :n], out_attn[b, :n] = torch.tensor(q[:n]), 1
    m = cases.build_model(be, ocfg, params, "fp32", dropout)
    dp = trie_loss_cases._train_mode(m, dropout)
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=tau, excluded_items=excluded_items, top_k=top_k,
            top_p=top_p)["loss"]
    O.runner_loss(nll, out_attn.to(nll.device)).backward()
    sync(be)
    Pq = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    nll_o, state, undecided = oracle_trunc_nll(Pq, ocfg, ids, ww, mask, labels, ct, tau, excl, dp, top_k, top_p)
    assert not undecided, f"rows {undecided} have an undecided child: choose another top_k / top_p / seed"
    O.runner_loss(nll_o, out_attn).backward()
    got_state = m.last_item_loss_state.cpu()
    assert np.array_equal(got_state.numpy(), state), (got_state.tolist(), state.tolist())
    nll_h = nll.detach().cpu().double()
    assert bool((nll_h[torch.from_numpy(state.reshape(-1) != SCORED)] == 0).all())
    err = float((nll_h - nll_o.detach()).abs().max())
    assert err <= trie_loss_cases.NLL_TOL, f"nll err {err}"
    worst = (0.0, "")
    gmax = max(float(v.grad.abs().max()) for v in Pq.values())
    for name, p in m.named_parameters():
        g_, go = p.grad.detach().cpu().double(), Pq[name].grad
        rel = (g_ - go).abs().max().item() / (go.abs().max().item() + 1e-2 * gmax + 1e-12)
        if rel > worst[0]:
            worst = (rel, name)
    n3 = int((state == TRUNCATED).sum())
    assert oracle_trunc_nll.live >= 1 and gmax > 0 and n3 >= 1, (oracle_trunc_nll.live, gmax, n3)
    print(f"[trunc loss fp32] top_k {top_k} top_p {top_p} dropout {dropout} tau {tau} excluded {excluded}: nll err {err:.2e}, worst gradient {worst[0]:.2e} "
          f"({worst[1]}), {n3} rows truncated away, {oracle_trunc_nll.live} rows with a gradient")
    assert worst[0] <= trie_loss_cases.GRAD_TOL, f"gradient mismatch {worst}"
    return err, worst, n3


def sampler_case(be, ocfg, items, B, L, S, top_k=0, top_p=1.0, tau=1.0, excluded=False, tag=""):
    """sample_items(top_k, top_p) draws fed back as labels: nll == -token_logprobs within the sum of both tolerances; state 3 only at rows
    the reference calls undecided, under the cap"""
    m, params = sample_cases.make_model(be, ocfg, "fp32")
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    excluded_items = [list(range(b % 2, len(items), 2)) if b != 1 else [] for b in range(B)] if excluded else None
    out = m.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, temperature=tau, excluded_items=excluded_items, seed=3,
                         top_k=top_k, top_p=top_p)
    seq, tlp = out["sequences"], out["token_logprobs"].cpu()
    R, T = seq.shape
    r = lambda t: t.repeat_interleave(S, dim=0)      # noqa: E731
    rep_ex = None if excluded_items is None else [excluded_items[b] for b in range(B) for _ in range(S)]
    nll = m(input_ids=r(ids), whole_word_ids=r(ww), attention_mask=r(mask), labels=seq[:, 1:], trie=ct, temperature=tau, excluded_items=rep_ex, top_k=top_k,
            top_p=top_p)["loss"].detach().cpu().view(R, T - 1)
    state = m.last_item_loss_state.cpu()
    assert not bool((state == trie_loss_cases.OFF).any()), "a drawn sequence left the trie"
    ref = Reference(params, ocfg, ids, ww, mask, ct)
    excl = None if excluded_items is None else ct.excluded_bitmap(excluded_items)
    visited, undecided = set(), set()
    seq_h = seq.cpu()
    for row in range(R):
        b, q = row // S, seq_h[row].tolist()
        n = q.index(1)
        ref.add(b, [q[:n + 1]])
        nodes = ref.walk(q[:n + 1])
        for t in range(1, n + 1):
            z = _z(ref, b, nodes[t - 1], tau, None if excl is None else excl[b])
            si, so = classify(z, top_k, top_p, FP32_TOL / tau)
            visited.add((b, nodes[t - 1]))
            if not bool((si | so | ~torch.isfinite(z)).all()):
                undecided.add((b, nodes[t - 1]))
            elif int(state[row, t - 1]) == TRUNCATED:
                raise AssertionError(f"draw {row} step {t}: the trainer truncated away a label the sampler drew at a decided node")
    assert len(undecided) <= UNDECIDED_CAP * len(visited), (len(undecided), len(visited))
    sc = state == SCORED
    tol = trie_loss_cases.SAMPLER_TOL["fp32"]
    d = float((nll + tlp)[sc].abs().max())
    print(f"[trunc loss == sampler{tag}] top_k {top_k} top_p {top_p} tau {tau}: {R} draws, max |nll + token log-prob| = {d:.3e} (tol {tol:.1e}); "
          f"{int((state == TRUNCATED).sum())} rows truncated away at undecided nodes")
    assert d <= tol
    assert bool((nll[~sc] == 0).all())


def fused_case(be, ocfg, items, dtype="fp32", dropout=0.0, top_k=0, top_p=0.995, B=3, L=14, T=6, tol=1e-6):
    """loss_and_backward(trie=, top_k=, top_p=) == forward(...) -> O.runner_loss -> autograd.  (The labels are random items, not the
    model's favourites, and these items branch at one node only: a tight truncation removes every label there, which leaves no gradient
    to compare; at top_p = 0.995 the labels stay while the tail of the node is cut.)"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = trie_loss_cases.item_batch(ocfg, items, B, L, T, 9)
    out_attn[B - 1, :] = 0          # a row with an empty label mask exercises clamp(min=1)
    res = []
    for fused in (False, True):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        trie_loss_cases._train_mode(m, dropout, 77)
        if fused:
            loss = m.loss_and_backward(ids, ww, mask, labels, out_attn, trie=ct, temperature=0.7, top_k=top_k, top_p=top_p)
        else:
            nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, temperature=0.7, top_k=top_k, top_p=top_p)["loss"]
            loss = O.runner_loss(nll, out_attn.to(nll.device))
            loss.backward()
        sync(be)
        res.append((float(loss.detach()), m._grads.detach().cpu().clone(), m.last_item_loss_state.cpu().clone()))
    (l0, g0, s0), (l1, g1, s1) = res
    assert torch.equal(s0, s1) and bool((s0 == SCORED).any())
    assert abs(l0 - l1) <= tol * max(1.0, abs(l0)), (l0, l1)
    assert float(g0.abs().max()) > 0
    err = (g0 - g1).abs().max().item() / max(1e-12, g0.abs().max().item())
    assert err <= (tol if dtype == "fp32" else 2e-2), f"fused truncated item-loss gradient differs: {err}"


def reproducible_case(be, ocfg, items, dtype="bf16", runs=3, dropout=0.1, top_k=0, top_p=0.995, B=3, L=14, T=6):
    """the same truncated item-loss step on fresh models, and two micro-batches accumulated: bit-identical losses and gradients"""
    ocfg = O.T5Cfg(**{**ocfg.__dict__, "dropout": dropout})
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    a = trie_loss_cases.item_batch(ocfg, items, B, L, T, 3)[:5]
    b = trie_loss_cases.item_batch(ocfg, items, B, L, T, 9)[:5]          # (seed 4's labels are all truncated away at the first branching node)
    outs = []
    for _ in range(runs):
        m = cases.build_model(be, ocfg, params, dtype, dropout)
        trie_loss_cases._train_mode(m, dropout, 41)
        m.begin_micro_batch(first=True, sync=False)
        l0 = m.loss_and_backward(*a, trie=ct, temperature=0.7, top_k=top_k, top_p=top_p)
        g0 = m._grads.detach().cpu().clone()
        m.begin_micro_batch(first=False, sync=False)
        l1 = m.loss_and_backward(*b, trie=ct, temperature=0.7, top_k=top_k, top_p=top_p)
        sync(be)
        outs.append((float(l0), float(l1), g0, m._grads.detach().cpu().clone()))
    assert float(outs[0][2].abs().max()) > 0 and not torch.equal(outs[0][2], outs[0][3]), "the second micro-batch must add to the arena"
    for r in range(1, runs):
        assert outs[r][:2] == outs[0][:2] and torch.equal(outs[r][2], outs[0][2]) and torch.equal(outs[r][3], outs[0][3]), r


def plain_route_restored_case(be, ocfg, items, B=3, L=14, T=6):
    """a plain step, an item-loss step, a truncated item-loss step, then the first two again: the same bits, and the truncated step runs
    the kernels of p5_trunc.h"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    batch = trie_loss_cases.item_batch(ocfg, items, B, L, T, 3, stray=False)[:5]
    m = cases.build_model(be, ocfg, params, "bf16", 0.0)
    m.eval()

    def step(**kw):
        m.zero_grad()
        loss = m.loss_and_backward(*batch, **kw)
        sync(be)
        return float(loss), m._grads.detach().cpu().clone()
    l0, g0 = step()
    l1, g1 = step(trie=ct)
    (l2, g2), k2 = trie_loss_cases._profiled(be, lambda: step(trie=ct, top_k=2))
    (l3, g3), k3 = trie_loss_cases._profiled(be, lambda: step(trie=ct, top_k=0, top_p=1.0))
    l4, g4 = step()
    has = lambda keys, name: any(name in k for k in keys)      # noqa: E731
    assert has(k2, "p5_trunc_ce_fwd_kernel") and has(k2, "p5_trunc_ce_bwd_kernel") and not has(k2, "p5_trie_ce_fwd_kernel"), k2
    assert has(k3, "p5_trie_ce_fwd_kernel") and not has(k3, "p5_trunc_ce"), k3
    assert l1 == l3 and torch.equal(g1, g3), "top_k=0, top_p=1.0 must be the untruncated item loss, bit for bit"
    assert l0 == l4 and torch.equal(g0, g4), "the plain step changed after a truncated item-loss step"
    assert l2 != l1 and not torch.equal(g2, g1)


def runner_case(be, tmp):
    """--item_loss_top_k / --item_loss_top_p reach the model; the defaults leave the keyword arguments of the untruncated loss"""
    import os
    from openp5_amd.runner import training_step
    from openp5_amd.model import P5ModelConfig
    tiny = P5ModelConfig(d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=2, dropout_rate=0.1)
    for name, flags in (("trunc", ("--item_loss_top_k", "3", "--item_loss_top_p", "0.9")), ("plain", ())):
        d = os.path.join(tmp, name)
        os.makedirs(d)
        runner, model, tok, args = cases.make_pipeline(be, d, "fp32", dataset="Toy", n_users=12, n_items=24, n_inter=90,
                                                       flags=["--batch_size", "8", "--train_item_loss", "1"] + list(flags), model_cfg=tiny, vocab=2400)
        model.train()
        kw = runner._item_loss_kw()
        if name == "plain":
            assert set(kw) == {"trie", "temperature"} and args.item_loss_top_k == 0 and args.item_loss_top_p == 1.0
            continue
        assert kw["top_k"] == 3 and kw["top_p"] == 0.9
        batch = next(iter(runner.train_loader))
        input_ids, attn, whole_ids, output_ids, output_attention = runner._to_dev(batch)[:5]
        loss = training_step(model, runner.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), args.alpha, item_loss=kw)
        assert math.isfinite(float(loss))
        st = model.last_item_loss_state.cpu()
        assert not bool((st == trie_loss_cases.OFF).any()) and bool(((st == SCORED) | (st == TRUNCATED)).eq(output_attention.cpu() != 0).all())
