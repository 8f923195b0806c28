"""Cases of the item loss on a head restricted to the trie's tokens (`forward(trie=..., item_head="trie")`, csrc/p5_item_head.h) shared by
tests/test_trie_head_emu.py (host emulation) and tests/test_gpu_trie_head.py (MI355X).

The oracle of the compact cross-entropy kernels is bit-equality with the dense kernels on the same logits (those are held to float64 by
tests/trie_loss_cases.py / tests/trunc_cases.py); the gather and the scatter are copies and single fp32 adds, exact by construction.  At
model level the existing cases of trie_loss_cases / trunc_cases run unchanged under `P5T5Native.item_head = "trie"` (the test files switch
the class attribute), and the two routes are compared with each other: each is held to the oracle, so they may differ by the sum of
their bounds."""

import numpy as np
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases, trie_loss_cases as tl, trunc_cases
from tests.cases import P, TT, _guard_intact, _same_bits, _sentinel, dev, sync

GS_V = 300                       # not a multiple of 64
GS_D = (8, 128, 512)


def _token_sets(V, seed=0):
    rnd = np.random.default_rng(seed)
    sets = {"first": [0], "last": [V - 1], "all": list(range(V))}
    for n in (63, 64, 65):
        sets[f"n{n}"] = sorted(rnd.choice(V, size=n, replace=False).tolist())
    return sets


def gather_scatter_case(be):
    """p5_op_item_gather (both dtypes) and p5_op_item_scatter (store and add mode): V = 300, d in {8, 128, 512}, U = {0}, {V - 1},
    63 / 64 / 65 random tokens, all 300 -- copies and single fp32 adds, compared bit for bit, with guards behind every output"""
    lib, st = be.lib, be.stream_ptr()
    V = GS_V
    g = torch.Generator().manual_seed(11)
    for d in GS_D:
        for name, U in _token_sets(V).items():
            Nu = len(U)
            Nup = (Nu + 63) // 64 * 64
            Ut = torch.tensor(U, dtype=torch.int64)
            tok_d = dev(be, Ut.to(torch.int32))
            md = f"item head d {d} U {name}"
            for dtype in (0, 1):
                tt = TT[dtype]
                E = torch.randn(V + 1, d, generator=g).to(tt)          # (one row behind V: never read)
                out = dev(be, _sentinel((Nup + 1, d), tt))
                be.check(lib.p5_op_item_gather(dtype, P(out), P(dev(be, E)), P(tok_d), Nu, d, st), "item_gather")
                sync(be)
                oh = out.cpu()
                _guard_intact(f"{md} gather dtype {dtype}", oh, Nup)
                assert _same_bits(oh[:Nu], E[Ut]), f"{md}: gathered rows differ from the source"
                assert bool((oh[Nu:Nup].float() == 0).all()) and not bool(torch.signbit(oh[Nu:Nup].float()).any()), f"{md}: pad rows are not +0"
            dEU = torch.randn(Nup, d, generator=g)
            dEU[Nu:] = float("nan")                                     # (pad rows are never read)
            dEU_d = dev(be, dEU)
            inU = torch.zeros(V, dtype=torch.bool)
            inU[Ut] = True
            # store mode: every row of [V, d] is written, nothing behind it
            tgt = dev(be, _sentinel((V + 1, d), torch.float32))
            be.check(lib.p5_op_item_scatter(P(tgt), P(dEU_d), P(tok_d), Nu, V, d, 1, st), "item_scatter store")
            sync(be)
            th = tgt.cpu()
            _guard_intact(f"{md} scatter store", th, V)
            assert _same_bits(th[:V][inU], dEU[:Nu]), f"{md}: stored rows of U differ from dE_U"
            assert bool((th[:V][~inU] == 0).all()), f"{md}: rows outside U are not zero"
            # add mode: rows of U = target + dE_U in fp32, every other row untouched
            base = torch.randn(V + 1, d, generator=g)
            base[V] = _sentinel((d,), torch.float32)
            tgt = dev(be, base.clone())
            be.check(lib.p5_op_item_scatter(P(tgt), P(dEU_d), P(tok_d), Nu, V, d, 0, st), "item_scatter add")
            sync(be)
            th = tgt.cpu()
            _guard_intact(f"{md} scatter add", th, V)
            assert _same_bits(th[:V][inU], base[:V][inU] + dEU[:Nu]), f"{md}: added rows differ from target + dE_U"
            assert _same_bits(th[:V][~inU], base[:V][~inU]), f"{md}: rows outside U were touched"


def _columns(tok):
    """(U int32 ascending, child_col int32 [n_edges]) of a CSR token array: CompiledTrie.head_columns()'s rule"""
    U, col = np.unique(tok, return_inverse=True)
    return U.astype(np.int32), col.reshape(-1).astype(np.int32)


def _compact(logits, U, V_cols):
    """logits[:, U] in a row of Nup columns plus 8 of padding, NaN in every column from Nu on"""
    Nu = len(U)
    Nup = (Nu + 63) // 64 * 64
    Lc = torch.full((logits.shape[0], Nup + 8), float("nan"))
    Lc[:, :Nu] = logits[:, torch.from_numpy(U.astype(np.int64))]
    return Lc, Nu, Nup


def ce_case(be, tau, T=3, seed=0):
    """p5_op_trie_ce_fwd_cols / _bwd_cols on logits_U = logits[:, U] against p5_op_trie_ce_fwd / _bwd on the dense row of
    trie_loss_cases._op_problem: nll, lse and dlogits_U[:, :Nu] == dlogits[:, U] bit for bit; pad columns and rows of state 1 / 2 zero"""
    lib, st = be.lib, be.stream_ptr()
    pr = tl._op_problem(seed)
    off, tok, nxt, ldl, ldd, B = pr["off"], pr["tok"], pr["nxt"], pr["ldl"], pr["ldd"], pr["B"]
    labels = pr["labels"][:, :T].contiguous()
    logits = pr["logits"].view(B, 3, ldl)[:, :T].reshape(B * T, ldl).contiguous()
    excl = pr["excl"]
    R = B * T
    U, col = _columns(tok)
    Lc, Nu, Nup = _compact(logits, U, pr["V"])
    ldc = Lc.shape[1]
    Ui = torch.from_numpy(U.astype(np.int64))
    node_ref, state_ref = tl.walk(off, tok, nxt, labels.numpy(), excl, 0, 1)
    scored = torch.from_numpy(state_ref.reshape(R) == tl.SCORED)
    assert 0 < int(scored.sum()) and (T == 1 or int(scored.sum()) < R)      # (T = 1: every row sits at the start node and is scored)
    d_off, d_tok, d_nxt, d_col = (dev(be, torch.from_numpy(a)) for a in (off, tok, nxt, col))
    d_excl = dev(be, torch.from_numpy(excl.view(np.int32)))
    words = excl.shape[1]
    Ld, Lcd, labd = dev(be, logits), dev(be, Lc), dev(be, labels)
    nd_in, st_in = dev(be, torch.from_numpy(node_ref.reshape(R))), dev(be, torch.from_numpy(state_ref.reshape(R)))
    g = torch.Generator().manual_seed(seed + 29)
    attn = torch.tensor([0, 1, 1, 2, -1], dtype=torch.int64)[torch.randint(0, 5, (B, T), generator=g)]
    attn[0, 0] = 1
    gscale = float(torch.tensor(1.0 / B, dtype=torch.float32))
    dnlld, attnd = dev(be, torch.randn(R, generator=g).float()), dev(be, attn)
    for dtype in (0, 1):
        md = f"compact trie_ce tau {tau} T {T} dtype {dtype}"
        outs = []
        for compact in (False, True):
            n_d, l_d = dev(be, _sentinel((R + 1,), torch.float32)), dev(be, _sentinel((R + 1,), torch.float32))
            if compact:
                be.check(lib.p5_op_trie_ce_fwd_cols(dtype, P(n_d), P(l_d), P(Lcd), P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt), P(d_col), P(d_excl),
                                                    words, tau, R, T, ldc, st), "trie_ce_fwd_cols")
            else:
                be.check(lib.p5_op_trie_ce_fwd(dtype, P(n_d), P(l_d), P(Ld), P(labd), P(nd_in), P(st_in), P(d_off), P(d_tok), P(d_nxt), P(d_excl), words, tau, R,
                                               T, ldl, st), "trie_ce_fwd")
            sync(be)
            outs.append((n_d.cpu(), l_d.cpu()))
        for k, nm in ((0, "nll"), (1, "lse")):
            _guard_intact(f"{md} {nm}", outs[1][k], R)
            assert _same_bits(outs[0][k][:R], outs[1][k][:R]), f"{md}: {nm} differs from the dense kernel's"
        assert bool(torch.isfinite(outs[1][0][:R]).all()), f"{md}: a pad column (NaN) was read"
        lsed = dev(be, outs[0][1][:R].clone())
        for seeding in ("dnll", "mask"):
            dn = P(dnlld) if seeding == "dnll" else None
            dl = dev(be, _sentinel((R + 1, ldd), TT[dtype]))
            be.check(lib.p5_op_trie_ce_bwd(dtype, P(dl), P(Ld), P(lsed), P(labd), P(nd_in), P(st_in), dn, P(d_off), P(d_tok), P(d_nxt), P(d_excl), words, tau, R, T,
                                           ldl, ldd, P(attnd), gscale, st), "trie_ce_bwd")
            dc = dev(be, _sentinel((R + 1, Nup), TT[dtype]))
            be.check(lib.p5_op_trie_ce_bwd_cols(dtype, P(dc), P(Lcd), P(lsed), P(labd), P(nd_in), P(st_in), dn, P(d_off), P(d_tok), P(d_nxt), P(d_col), P(d_excl),
                                                words, tau, R, T, ldc, Nup, P(attnd), gscale, st), "trie_ce_bwd_cols")
            sync(be)
            dh, ch = dl.cpu(), dc.cpu()
            _guard_intact(f"{md} dlogits_U", ch, R)
            assert _same_bits(ch[:R, :Nu], dh[:R][:, Ui]), f"{md} {seeding}: dlogits_U differs from dlogits[:, U]"
            assert bool((ch[:R, Nu:].float() == 0).all()), f"{md}: pad columns [Nu, Nup) are not zero"
            assert bool((ch[:R][~scored].float() == 0).all()), f"{md}: rows of state 1 / 2 are not zero"
            assert float(ch[:R].float().abs().max()) > 0


TRUNC_FANS = trunc_cases.OP_FANS


def trunc_ce_case(be, tau, fans=TRUNC_FANS, seed=0):
    """the truncated pair on the rows of trunc_cases (fan-outs up to 2,049, V = 4096): nll, lse, row_cut, the states and
    dlogits_U[:, :Nu] == dlogits[:, U] of the dense kernels, bit for bit"""
    lib, st = be.lib, be.stream_ptr()
    V = trunc_cases.OP_V
    R = len(trunc_cases.OP_KINDS)
    ldd = (V + 63) // 64 * 64
    ldl = ldd + 8
    n3 = 0
    for fan in fans:
        toks, logit_rows, ex = trunc_cases._op_rows(fan, tau, seed + fan)
        off = np.asarray([0, 1, 1 + fan] + [1 + fan] * fan, dtype=np.int32)
        tok = np.concatenate([[0], toks.numpy()]).astype(np.int32)
        nxt = np.concatenate([[1], np.arange(2, fan + 2)]).astype(np.int32)
        words = (fan + 2 + 31) // 32
        excl = np.zeros((R, words), dtype=np.uint32)
        for r in range(R):
            for i in np.nonzero(ex[r].numpy())[0]:
                excl[r, (i + 2) >> 5] |= np.uint32(1) << np.uint32((i + 2) & 31)
        L = torch.full((R, ldl), float("nan"))
        L[:, :V] = logit_rows
        U, col = _columns(tok)
        Lc, Nu, Nup = _compact(L, U, V)
        ldc = Lc.shape[1]
        Ui = torch.from_numpy(U.astype(np.int64))
        d_off, d_tok, d_nxt, d_col = (dev(be, torch.from_numpy(a)) for a in (off, tok, nxt, col))
        d_excl = dev(be, torch.from_numpy(excl.view(np.int32)))
        Ld, Lcd = dev(be, L), dev(be, Lc)
        node = dev(be, torch.ones(R, dtype=torch.int32))
        g = torch.Generator().manual_seed(seed + 7 * fan)
        dnlld = dev(be, torch.randn(R, generator=g).float())
        attnd = dev(be, torch.ones(R, 1, dtype=torch.int64))
        gscale = float(torch.tensor(1.0 / R, dtype=torch.float32))
        z = torch.where(ex, torch.full((R, fan), -np.inf, dtype=torch.float64), L[:, toks].double())
        for ci, (k, p) in enumerate(trunc_cases._op_params(fan)):
            # labels as in trunc_cases.op_case: the largest child on even cases, the median allowed child on odd ones
            lab_pos = []
            for r in range(R):
                fin = torch.nonzero(torch.isfinite(z[r])).flatten()
                order = fin[torch.argsort(z[r][fin], descending=True, stable=True)]
                lab_pos.append(int(order[0] if ci % 2 == 0 else order[len(order) // 2]))
            labd = dev(be, toks[lab_pos].to(torch.int64).view(R, 1))
            for dtype in (0, 1):
                md = f"compact trunc_ce fan {fan} tau {tau} top_k {k} top_p {p} dtype {dtype}"
                outs = []
                for compact in (False, True):
                    o_n, o_l, o_c = (dev(be, _sentinel((R + 1,), torch.float32)) for _ in range(3))
                    st_d = dev(be, torch.cat([torch.zeros(R, dtype=torch.int32), torch.tensor([tl.I32_SENT], dtype=torch.int32)]))
                    if compact:
                        be.check(lib.p5_op_trunc_ce_fwd_cols(dtype, P(o_n), P(o_l), P(o_c), P(st_d), P(Lcd), P(labd), P(node), P(d_off), P(d_tok), P(d_nxt), P(d_col),
                                                             P(d_excl), words, tau, k, p, R, 1, ldc, st), "trunc_ce_fwd_cols")
                    else:
                        be.check(lib.p5_op_trunc_ce_fwd(dtype, P(o_n), P(o_l), P(o_c), P(st_d), P(Ld), P(labd), P(node), P(d_off), P(d_tok), P(d_nxt), P(d_excl), words,
                                                        tau, k, p, R, 1, ldl, st), "trunc_ce_fwd")
                    sync(be)
                    outs.append((o_n.cpu(), o_l.cpu(), o_c.cpu(), st_d.cpu()))
                for j, nm in enumerate(("nll", "lse", "row_cut")):
                    _guard_intact(f"{md} {nm}", outs[1][j], R)
                    assert _same_bits(outs[0][j][:R], outs[1][j][:R]), f"{md}: {nm} differs from the dense kernel's"
                assert torch.equal(outs[0][3], outs[1][3]), f"{md}: states differ"
                n3 += int((outs[1][3][:R] == trunc_cases.TRUNCATED).sum())
                lsed, cutd, state_in = dev(be, outs[0][1][:R].clone()), dev(be, outs[0][2][:R].clone()), dev(be, outs[0][3][:R].clone())
                dl = dev(be, _sentinel((R + 1, ldd), TT[dtype]))
                be.check(lib.p5_op_trunc_ce_bwd(dtype, P(dl), P(Ld), P(lsed), P(cutd), P(labd), P(node), P(state_in), P(dnlld), P(d_off), P(d_tok), P(d_nxt),
                                                P(d_excl), words, tau, R, 1, ldl, ldd, P(attnd), gscale, st), "trunc_ce_bwd")
                dc = dev(be, _sentinel((R + 1, Nup), TT[dtype]))
                be.check(lib.p5_op_trunc_ce_bwd_cols(dtype, P(dc), P(Lcd), P(lsed), P(cutd), P(labd), P(node), P(state_in), P(dnlld), P(d_off), P(d_tok), P(d_nxt),
                                                     P(d_col), P(d_excl), words, tau, R, 1, ldc, Nup, P(attnd), gscale, st), "trunc_ce_bwd_cols")
                sync(be)
                dh, ch = dl.cpu(), dc.cpu()
                _guard_intact(f"{md} dlogits_U", ch, R)
                assert _same_bits(ch[:R, :Nu], dh[:R][:, Ui]), f"{md}: dlogits_U differs from dlogits[:, U]"
                assert bool((ch[:R, Nu:].float() == 0).all()), f"{md}: pad columns are not zero"
                away = outs[1][3][:R] == trunc_cases.TRUNCATED
                assert bool((ch[:R][away].float() == 0).all()), f"{md}: a truncated row is not zero"
    if len(fans) >= 5:
        assert n3 >= 10, n3


def abi_errors_case(be, ocfg):
    """p5_train_set_item_head: no item loss armed, n_tokens outside [1, vocab_size], a workspace that is too small -- each with a message;
    the Python keyword: anything but "dense" / "trie", and "trie" without a trie"""
    import pytest
    from openp5_amd.model import _ptr
    items = cases.make_items(20, 5, hi=60)
    ct = rank_cases.compiled(items)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    dv = m._be.device
    off, tok, nxt = ct.device_arrays(dv)
    htok, hcol = ct.head_columns_device(dv)
    Nu = int(htok.numel())
    lib = be.lib
    need = int(lib.p5_item_head_workspace_bytes(m._engine, 2, 6, Nu))
    assert need > 0 and int(lib.p5_item_head_workspace_bytes(m._engine, 4, 6, Nu)) > need
    raw = torch.zeros(need + 256, dtype=torch.uint8, device=dv)
    ws = raw[(-raw.data_ptr()) % 256:]
    arm = lambda: be.check(lib.p5_train_set_item_loss(m._engine, _ptr(off), _ptr(tok), _ptr(nxt), ct.n_nodes, None, 0, 1.0, None), "set_item_loss")  # noqa: E731
    assert lib.p5_train_set_item_head(m._engine, _ptr(htok), Nu, _ptr(hcol), _ptr(ws), need) != 0
    assert b"no item loss is armed" in lib.p5_last_error()
    for n in (0, -1, ocfg.vocab_size + 1):
        arm()
        assert lib.p5_train_set_item_head(m._engine, _ptr(htok), n, _ptr(hcol), _ptr(ws), need) != 0, n
        assert b"n_tokens" in lib.p5_last_error()
    arm()
    assert lib.p5_train_set_item_head(m._engine, _ptr(htok), Nu, _ptr(hcol), _ptr(ws), 16) != 0
    assert b"workspace too small" in lib.p5_last_error()
    arm()
    assert lib.p5_train_set_item_head(m._engine, _ptr(htok), Nu, _ptr(hcol), _ptr(ws), need) == 0
    arm()           # a new p5_train_set_item_loss disarms the head: the dense item loss, bit for bit
    ids, ww, mask, labels, out_attn, _ = tl.item_batch(ocfg, items, 2, 12, 6, 5, stray=False)
    kw = dict(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels)
    ids_d, ww_d, mask_d, lab_d = (m._i64(t, dv) for t in (ids, ww, mask, labels))
    m._sync_shadow()
    tws = m._workspace(lib.p5_train_workspace_bytes(m._engine, 2, 12, 6))
    nll = torch.zeros(12, dtype=torch.float32, device=dv)
    be.check(lib.p5_forward(m._engine, _ptr(ids_d), _ptr(ww_d), _ptr(mask_d), _ptr(lab_d), 2, 12, 6, 0, _ptr(nll), _ptr(tws), tws.numel(), m._be.stream_ptr()), "fwd")
    sync(be)
    with torch.no_grad():
        dense = m(trie=ct, item_head="dense", **kw)["loss"].cpu()
        assert torch.equal(nll.cpu(), dense)
        for bad in (dict(trie=ct, item_head="sparse"), dict(item_head="trie"), dict(item_head=1)):
            with pytest.raises(ValueError):
                m(**bad, **kw)
            with pytest.raises(ValueError):
                m.loss_and_backward(ids, ww, mask, labels, out_attn, **bad)
        # a failed call leaves nothing armed, and the attribute alone (no trie) is the plain loss
        a = m(**kw)["loss"].cpu()
        type(m).item_head, keep = "trie", type(m).item_head
        try:
            b = m(**kw)["loss"].cpu()
        finally:
            type(m).item_head = keep
        assert torch.equal(a, b)


def head_columns_case():
    from openp5_amd.trie import CompiledTrie, Trie
    items = cases.make_items(40, 5, hi=60)
    ct = CompiledTrie.from_trie(Trie(items))
    U, col = ct.head_columns()
    assert U.dtype == np.int32 and col.dtype == np.int32 and col.shape == ct.child_tok.shape
    assert np.array_equal(U, np.unique(ct.child_tok)) and np.array_equal(U[col], ct.child_tok)
    assert ct.head_columns()[0] is U, "cached"
    a = ct.head_columns_device(torch.device("cpu"))
    assert ct.head_columns_device(torch.device("cpu"))[0] is a[0] and np.array_equal(a[1].numpy(), col)
    assert ct.device_arrays(torch.device("cpu"))[1].dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------
# route against route
# ---------------------------------------------------------------------------------------------------------
def _untouched_rows(ocfg, ct, ids, labels):
    """rows of shared.weight whose token is neither in U nor looked up by the encoder's or the decoder's inputs"""
    seen = torch.zeros(ocfg.vocab_size, dtype=torch.bool)
    seen[torch.from_numpy(ct.head_columns()[0].astype(np.int64))] = True
    seen[ids.reshape(-1)] = True
    seen[O.shift_right(labels, ocfg).reshape(-1).clamp(min=0)] = True
    seen[labels.reshape(-1).clamp(min=0)] = True
    return ~seen


def _compare_routes(ocfg, ct, ids, labels, dense, trie, dtype, tag):
    """dense / trie: (nll [B*T] cpu, {name: grad cpu}, whole arena cpu)"""
    nerr = float((dense[0].double() - trie[0].double()).abs().max())
    if dtype == "fp32":
        assert nerr <= 2 * tl.NLL_TOL, f"{tag}: nll differs by {nerr}"
        gmax = max(float(g.abs().max()) for g in dense[1].values())
        worst = (0.0, "")
        for name, go in dense[1].items():
            rel = float((trie[1][name].double() - go.double()).abs().max()) / (float(go.abs().max()) + 1e-2 * gmax + 1e-12)
            worst = max(worst, (rel, name))
        assert worst[0] <= 2 * tl.GRAD_TOL, f"{tag}: gradients differ {worst}"
        gerr = worst[0]
    else:
        assert nerr <= 2 * tl.BF16_BOUNDS["nll_max"], f"{tag}: nll differs by {nerr}"
        gerr = float((dense[2] - trie[2]).abs().max()) / max(1e-12, float(dense[2].abs().max()))
        assert gerr <= 2e-2, f"{tag}: gradients differ by {gerr} of the largest entry"
    free = _untouched_rows(ocfg, ct, ids, labels)
    assert int(free.sum()) > 0
    gE = trie[1]["shared.weight"]
    assert bool((gE[free] == 0).all()), f"{tag}: rows of shared.weight.grad outside U and the batch's lookups are not exactly 0"
    assert float(gE.abs().max()) > 0
    print(f"[item head, route against route{tag}] {dtype}: nll {nerr:.2e}, gradients {gerr:.2e}; {int(free.sum())} rows of shared.weight.grad exactly 0")


def _autograd_step(be, ocfg, params, dtype, batch, ct, head, **kw):
    ids, ww, mask, labels, out_attn = batch
    m = cases.build_model(be, ocfg, params, dtype, 0.0)
    m.eval()
    nll = m(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, item_head=head, **kw)["loss"]
    O.runner_loss(nll, out_attn.to(nll.device)).backward()
    sync(be)
    return nll.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}, m._grads.detach().cpu().clone()


def routes_case(be, ocfg, items, dtype="fp32", B=3, L=14, T=6, ct=None, params=None, tag="", **kw):
    """one batch, fresh models: the restricted head against the dense one"""
    params = params if params is not None else O.init_params(ocfg, 7)
    ct = ct if ct is not None else rank_cases.compiled(items)
    batch = tl.item_batch(ocfg, items, B, L, T, 3, stray=False)[:5]
    dense = _autograd_step(be, ocfg, params, dtype, batch, ct, "dense", **kw)
    trie = _autograd_step(be, ocfg, params, dtype, batch, ct, "trie", **kw)
    _compare_routes(ocfg, ct, batch[0], batch[3], dense, trie, dtype, tag)


# ---------------------------------------------------------------------------------------------------------
# the grouped, storing path (bf16, M = Md = 64: wg_all_deferred holds and the weight-gradient plan runs)
# ---------------------------------------------------------------------------------------------------------
def _fused(be, m, batch, ct, **kw):
    loss = m.loss_and_backward(*batch, trie=ct, **kw)
    sync(be)
    return float(loss), m._grads.detach().cpu().clone()


def storing_case(be, ocfg, items, B=8, L=8, T=8, staged=False, dtype="bf16", ct=None, params=None):
    """A plain step on another batch fills the arena, zero_grad() leaves it as it is (the next backward STORES), then the restricted step:
    bit-identical to the restricted step of a fresh model, and again when repeated; as two accumulated micro-batches the arena is the sum
    of the two alone (accumulation_case's 1e-5); and the restricted route agrees with the dense one"""
    assert (B * L) % 64 == 0 and (B * T) % 64 == 0
    params = params if params is not None else O.init_params(ocfg, 7)
    ct = ct if ct is not None else rank_cases.compiled(items)
    a = tl.item_batch(ocfg, items, B, L, T, 3, stray=False)[:5]
    b = tl.item_batch(ocfg, items, B, L, T, 4, stray=False)[:5]

    def model():
        m = cases.build_model(be, ocfg, params, dtype, 0.0)
        m.eval()
        m.staged_backward = staged
        return m
    fresh = _fused(be, model(), a, ct, item_head="trie")
    assert float(fresh[1].abs().max()) > 0
    m = model()
    m.loss_and_backward(*b)
    sync(be)
    dirty = m._grads.detach().cpu().clone()
    assert not torch.equal(dirty, fresh[1])
    for rep in range(2):
        m.zero_grad()
        got = _fused(be, m, a, ct, item_head="trie")
        assert got[0] == fresh[0] and torch.equal(got[1], fresh[1]), (rep, float((got[1] - fresh[1]).abs().max()))
    # accumulation: first micro-batch stores, the second adds at the rows U
    alone_b = _fused(be, model(), b, ct, item_head="trie")
    m = model()
    m.loss_and_backward(*b)          # (stale gradients in the arena)
    m.zero_grad()
    m.begin_micro_batch(first=True, sync=False)
    m.loss_and_backward(*a, trie=ct, item_head="trie")
    m.begin_micro_batch(first=False, sync=False)
    m.loss_and_backward(*b, trie=ct, item_head="trie")
    sync(be)
    want = fresh[1] + alone_b[1]
    err, scale = float((m._grads.detach().cpu() - want).abs().max()), float(want.abs().max())
    assert err <= 1e-5 * scale, (err, scale)
    # route against route
    md = model()
    dense = _fused(be, md, a, ct, item_head="dense")
    gerr = float((dense[1] - fresh[1]).abs().max()) / float(dense[1].abs().max())
    assert abs(dense[0] - fresh[0]) <= 2 * tl.BF16_BOUNDS["nll_max"] and gerr <= (2e-2 if dtype == "bf16" else 2 * tl.GRAD_TOL), (dense[0], fresh[0], gerr)
    off, n, shape = md._views["shared.weight"]
    gE = fresh[1][off:off + n].view(shape)
    free = _untouched_rows(ocfg, ct, a[0], a[3])
    assert int(free.sum()) > 0 and bool((gE[free] == 0).all()), "stale rows of shared.weight.grad survived the storing scatter"


# ---------------------------------------------------------------------------------------------------------
# which kernels run
# ---------------------------------------------------------------------------------------------------------
def profile_case(be, ocfg, items, B=4, L=16, T=8):
    """plain, dense item loss, restricted item loss, dense item loss, plain (tl.plain_route_restored_case's set-up): the dense steps and
    the plain steps are bit-identical pairs; the gather and scatter kernels run in the restricted step only, which runs none of the
    full-vocabulary cross-entropy kernels"""
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    batch = tl.item_batch(ocfg, items, B, L, T, 3, stray=False)[:5]
    be.check(be.lib.p5_set_option(b"gemm_wide_min_tiles", 1), "opt")
    try:
        m = cases.build_model(be, ocfg, params, "bf16", 0.0)
        m.eval()

        def step(**kw):
            m.zero_grad()
            loss = m.loss_and_backward(*batch, **kw)
            sync(be)
            return float(loss), m._grads.detach().cpu().clone()
        (lp0, gp0), kp0 = tl._profiled(be, step)
        (ld0, gd0), kd0 = tl._profiled(be, lambda: step(trie=ct, item_head="dense"))
        (lt, gt), kt = tl._profiled(be, lambda: step(trie=ct, item_head="trie"))
        (ld1, gd1), kd1 = tl._profiled(be, lambda: step(trie=ct, item_head="dense"))
        (lp1, gp1), kp1 = tl._profiled(be, step)
    finally:
        be.lib.p5_set_option(b"gemm_wide_min_tiles", 160)
    has = lambda keys, name: any(name in k for k in keys)      # noqa: E731
    assert ld0 == ld1 and torch.equal(gd0, gd1), "the dense item-loss step changed after a restricted one"
    assert lp0 == lp1 and torch.equal(gp0, gp1), "the plain step changed after the item-loss steps"
    for keys in (kp0, kd0, kd1, kp1):
        assert not has(keys, "p5_item_gather_kernel") and not has(keys, "p5_item_scatter_kernel"), keys
    assert has(kt, "p5_item_gather_kernel") and has(kt, "p5_item_scatter_kernel"), kt
    assert has(kt, "p5_trie_walk_kernel") and has(kt, "p5_trie_ce_fwd_kernel") and has(kt, "p5_trie_ce_bwd_kernel"), kt
    assert not has(kt, "p5_ce_fwd_kernel") and not has(kt, "p5_ce_finish_kernel") and not has(kt, "p5_ce_bwd_kernel<"), kt
    assert has(kp0, "p5_ce_finish_kernel") and has(kp1, "p5_ce_finish_kernel")
    assert abs(lt - ld0) <= 2 * tl.BF16_BOUNDS["nll_max"] and lt != lp0


# ---------------------------------------------------------------------------------------------------------
# workspace
# ---------------------------------------------------------------------------------------------------------
def workspace_case(be, ocfg, items, B=2, L=12, T=6):
    """the restricted forward and backward inside exactly p5_item_head_workspace_bytes, a guard behind it; one byte fewer fails with a
    message.  p5_train_workspace_bytes: the unchanged tl.workspace_case still holds (the test files run it)."""
    from openp5_amd.model import _ptr
    params = O.init_params(ocfg, 7)
    ct = rank_cases.compiled(items)
    ids, ww, mask, labels, out_attn, _ = tl.item_batch(ocfg, items, B, L, T, 3, stray=False)
    lib = be.lib
    for dtype in ("fp32", "bf16"):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        dv = m._be.device
        off, tok, nxt = ct.device_arrays(dv)
        htok, hcol = ct.head_columns_device(dv)
        Nu = int(htok.numel())
        ids_d, ww_d, mask_d, lab_d = (m._i64(t, dv) for t in (ids, ww, mask, labels))
        m._sync_shadow()
        m._sync_transposed()
        tws = m._workspace(lib.p5_train_workspace_bytes(m._engine, B, L, T))
        need = int(lib.p5_item_head_workspace_bytes(m._engine, B, T, Nu))
        assert need > 0
        raw = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=dv)
        skew = (-raw.data_ptr()) % 256
        ws = raw[skew:skew + need]
        guard = raw[skew + need:].clone()
        nll = torch.zeros(B * T, dtype=torch.float32, device=dv)
        dnll = torch.full((B * T,), 1.0 / (B * T), dtype=torch.float32, device=dv)

        def call(nbytes):
            be.check(lib.p5_train_set_item_loss(m._engine, _ptr(off), _ptr(tok), _ptr(nxt), ct.n_nodes, None, 0, 1.0, None), "set_item_loss")
            be.check(lib.p5_train_set_item_head(m._engine, _ptr(htok), Nu, _ptr(hcol), _ptr(ws), nbytes), "set_item_head")
            return lib.p5_forward(m._engine, _ptr(ids_d), _ptr(ww_d), _ptr(mask_d), _ptr(lab_d), B, L, T, 0, _ptr(nll), _ptr(tws), tws.numel(), m._be.stream_ptr())
        assert call(need - 1) != 0
        assert b"workspace too small" in lib.p5_last_error()
        assert call(need) == 0
        be.check(lib.p5_backward(m._engine, _ptr(dnll), m._be.stream_ptr()), "p5_backward")
        sync(be)
        assert torch.equal(raw[skew + need:], guard), "the restricted head wrote behind the bytes p5_item_head_workspace_bytes asked for"
        got_g = m._grads.detach().cpu().clone()
        m2 = cases.build_model(be, ocfg, params, dtype)
        m2.eval()
        want = m2(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=labels, trie=ct, item_head="trie")["loss"]
        want.backward(dnll.to(want.device))
        sync(be)
        assert torch.equal(nll.cpu(), want.detach().cpu()) and torch.equal(got_g, m2._grads.detach().cpu())


def runner_case(be, tmp):
    """--item_loss_head: trie trains (finite losses, every target row on the union trie); dense gives the first-step loss of the run
    without the flag, bit for bit"""
    import math
    import os
    from openp5_amd.model import P5ModelConfig, P5T5Native
    from openp5_amd.runner import training_step
    tiny = P5ModelConfig(d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=2, dropout_rate=0.1)
    first = {}
    keep = P5T5Native.item_head
    P5T5Native.item_head = "dense"          # (the flag decides, whatever the class says)
    try:
        # (the first pipeline of a process starts from other initial weights than the later ones, whatever its flags: the two runs that are
        #  compared bit for bit come second and third, and the trie run is compared with the dense head on its own model)
        for name, flags in (("trie", ("--item_loss_head", "trie")), ("dense", ("--item_loss_head", "dense")), ("absent", ())):
            d = os.path.join(tmp, "head_" + name)
            os.makedirs(d)
            runner, model, tok, args = cases.make_pipeline(be, d, "fp32", dataset="Toy", n_users=12, n_items=24, n_inter=90,
                                                           flags=["--batch_size", "8", "--train_item_loss", "1"] + list(flags), model_cfg=tiny, vocab=2400)
            model.train()
            kw = runner._item_loss_kw()
            assert kw.get("item_head", "dense") == ("trie" if name == "trie" else "dense") and args.item_loss_head == kw.get("item_head", "dense")
            losses = []
            for i, batch in enumerate(runner.train_loader):
                if i == (3 if name == "trie" else 1):
                    break
                input_ids, attn, whole_ids, output_ids, output_attention = runner._to_dev(batch)[:5]
                if name == "trie" and i == 0:
                    model.eval()          # (no dropout: the dropout step is not advanced, the training below is undisturbed)
                    with torch.no_grad():
                        fk = dict(input_ids=input_ids, whole_word_ids=whole_ids, attention_mask=attn, labels=output_ids)
                        n_t = model(**fk, **kw)["loss"].cpu()
                        n_d = model(**fk, **{**kw, "item_head": "dense"})["loss"].cpu()
                    assert float(n_d.abs().max()) > 0 and float((n_t - n_d).abs().max()) <= 2 * tl.NLL_TOL, float((n_t - n_d).abs().max())
                    model.train()
                losses.append(float(training_step(model, runner.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), args.alpha, item_loss=kw)))
                st = model.last_item_loss_state.cpu()
                assert not bool((st == tl.OFF).any()) and bool(((st == tl.SCORED) == (output_attention.cpu() != 0)).all())
            assert all(math.isfinite(x) for x in losses), losses
            first[name] = losses[0]
            model.eval()
    finally:
        P5T5Native.item_head = keep
    assert first["dense"] == first["absent"], first
