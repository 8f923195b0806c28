"""Cases of certified pruned ranking (`P5T5Native.rank_items(pruned=True)`, csrc/p5_prune.h) shared by tests/test_rank_pruned_emu.py
(host emulation) and tests/test_gpu_rank_pruned.py (MI355X).  The reference for every score and every order is the oracle over EVERY item
(`rank_cases.oracle_scores` / `oracle_order`); never `rank_items` and never the code under test.  The fixture is a toy model trained to put
real mass on the trie's tokens (tests/golden/make_peaked_tiny.py): only such a model prunes."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "peaked_tiny.pt")
FP32_TOL = 2e-5            # what rank_cases holds a bf16 model's verified (fp32-engine) scores to at toy width
STAT_KEYS = ("pruned_calls", "certified_users", "fallback_users", "declined_users")


@functools.lru_cache(maxsize=None)
def fixture():
    """(oracle config, trained parameters, items) of tests/golden/peaked_tiny.pt"""
    fx = torch.load(GOLDEN, map_location="cpu")
    ocfg = O.T5Cfg(**fx["cfg"])
    items = cases.make_items(fx["n_items"], fx["item_seed"], hi=fx["item_hi"])
    return ocfg, fx["params"], items, int(fx["L"])


_REF = {}


def oracle_reference(key, params, ocfg, ids, ww, mask, items):
    """(scores [B, n_items], per-token log-probabilities [B, n_items, T - 1]) by O.sequence_scores, computed once per `key`"""
    if key not in _REF:
        seqs = rank_cases.items_tensor(items)
        with torch.no_grad():
            sc, lp, _ = O.sequence_scores(params, ocfg, ids, ww, mask, seqs[None].expand(ids.shape[0], -1, -1).contiguous(), return_token_logprobs=True)
        _REF[key] = (sc, lp)
    return _REF[key]


def oracle_kept_rows(ct, items, lp_b, tau, s):
    """the oracle's kept-row count of one user at slack s: plan rows r with P(r) / Lmax(r) >= tau - s, P the oracle's log-probability of
    the prefix, Lmax the largest token count of an item below it -- both by brute force over the items"""
    item_rows = ct.item_rows(0)
    rows = ct.rank_plan(0)["rows"]
    P = np.zeros(rows, dtype=np.float64)
    lmax = np.zeros(rows, dtype=np.int64)
    lp_b = lp_b.double().numpy()
    for i, q in enumerate(items):
        n = len(q) - 1
        cum = np.concatenate(([0.0], np.cumsum(lp_b[i, :n])))
        for t in range(item_rows.shape[1]):
            r = int(item_rows[i, t])
            if r < 0:
                break
            P[r] = cum[t]
            lmax[r] = max(lmax[r], n)
    assert int(lmax.min()) >= 1
    return int((P / lmax >= tau - s).sum())


def check_lists(out, ref, items, B, N, excluded, order, score_tol):
    """the returned lists against the oracle's scores `ref` [B, n_items]: self-consistent (rank_cases.rank_case's checks on what is
    returned), every returned score within score_tol of the oracle's score of that item, and the order as rank_case judges it"""
    n_items = len(items)
    idx = out["item_index"].cpu()
    seq = out["sequences"].cpu().view(B, N, -1)
    sc = out["sequences_scores"].cpu().view(B, N)
    assert out["scores"] is None and idx.shape == (B, N) and int(seq[:, :, 0].abs().max()) == 0
    orders = rank_cases.oracle_order(ref, excluded)
    toks = rank_cases.items_tensor(items)
    worst = 0.0
    for b in range(B):
        n_live = min(N, len(orders[b]))
        assert bool((idx[b, n_live:] == -1).all()) and bool((sc[b, n_live:] == -1e9).all()) and int(seq[b, n_live:].abs().max() if n_live < N else 0) == 0
        for k in range(n_live):
            i = int(idx[b, k])
            assert 0 <= i < n_items and (excluded is None or i not in set(excluded[b]))
            assert seq[b, k, :toks.shape[1]].tolist() == toks[i].tolist() and int(seq[b, k, toks.shape[1]:].abs().sum()) == 0
            worst = max(worst, abs(float(sc[b, k]) - float(ref[b, i])))
            if k:
                assert float(sc[b, k]) <= float(sc[b, k - 1])
        assert len(set(idx[b, :n_live].tolist())) == n_live
    print(f"[pruned] max |returned score - oracle| = {worst:.3e} (tol {score_tol:.1e})")
    assert worst <= score_tol, worst
    if order == "near":
        for b in range(B):
            for k in range(min(N, len(orders[b]))):
                assert abs(float(ref[b, int(idx[b, k])]) - float(ref[b, orders[b][k]])) <= 2 * score_tol, (b, k, int(idx[b, k]), orders[b][k])
    elif order == "exact":
        # (gaps that can change the returned list: among the oracle's first N + 1 items, the one between ranks N and N + 1 included)
        gaps = torch.cat([ref[b][torch.tensor(orders[b][:N + 1], dtype=torch.int64)].diff().abs() for b in range(B) if len(orders[b]) > 1])
        assert float(gaps.min()) >= 4 * score_tol, f"oracle gap {float(gaps.min()):.2e} too small for a token-exact check at tolerance {score_tol}"
        for b in range(B):
            n_live = min(N, len(orders[b]))
            assert idx[b, :n_live].tolist() == orders[b][:n_live], (b, idx[b, :n_live].tolist(), orders[b][:n_live])
    else:
        raise ValueError(order)


def delta(m, before):
    return {k: m.rank_stats[k] - before[k] for k in STAT_KEYS}


def call(m, ids, ww, mask, ct, N, excluded=None, **opts):
    """one rank_items(pruned=True) call with the model's prune options set to `opts`; returns (out, the call's stat counts)"""
    for k, v in opts.items():
        setattr(m, "rank_prune_" + k, v)
    before = dict(m.rank_stats)
    out = m.rank_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, top_n=N, excluded_items=excluded, pruned=True)
    return out, delta(m, before)


class Peaked:
    """the fixture on a backend: bf16 model, B users (tests.cases.synth_batch, the distribution the fixture was trained on), the oracle's numbers"""

    def __init__(self, be, B=3, seed=5):
        self.ocfg, self.params, self.items, self.L = fixture()
        self.B = B
        self.m = cases.build_model(be, self.ocfg, self.params, "bf16")
        self.m.eval()
        self.ids, self.ww, self.mask, _, _ = cases.synth_batch(self.ocfg, B, self.L, 4, seed)
        self.ct = rank_cases.compiled(self.items)
        self.ref, self.lp = oracle_reference(("peaked", B, seed), self.params, self.ocfg, self.ids, self.ww, self.mask, self.items)
        self.rows = self.ct.rank_plan(0)["rows"]

    def kept(self, N, s, excluded=None):
        """the largest oracle kept-row count over the users at slack s"""
        orders = rank_cases.oracle_order(self.ref, excluded)
        return max(oracle_kept_rows(self.ct, self.items, self.lp[b], float(self.ref[b, orders[b][N - 1]]), s) for b in range(self.B))

    def run(self, N=10, excluded=None, **opts):
        return call(self.m, self.ids, self.ww, self.mask, self.ct, N, excluded, **opts)


def certified_case(be, N=10):
    """1. certified equals the oracle: every user certified, the list token-exact, and the number of rows that got fp32 numbers between
    the oracle's counts at slack -/+ two bf16 tolerances (one on the threshold, one on the bound)"""
    p = Peaked(be)
    slack = p.m.rank_prune_slack
    assert slack == pytest.approx(3 * cases.BF16_SCORE_TOL) and p.m.rank_prune_margin == 1e-4 and p.m.rank_prune_max_fraction == 0.6
    out, st = p.run(N, max_fraction=1.0)
    assert p.m.last_generate_path == "rank_pruned", p.m.last_generate_path
    assert st == {"pruned_calls": 1, "certified_users": p.B, "fallback_users": 0, "declined_users": 0}, st
    check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)
    lo, hi, got = p.kept(N, slack - 2 * cases.BF16_SCORE_TOL), p.kept(N, slack + 2 * cases.BF16_SCORE_TOL), p.m.rank_stats["kept_rows_per_user"]
    print(f"[pruned certified] rows kept {got} of {p.rows}; oracle at slack -/+ 2 tol: {lo} .. {hi}")
    assert lo <= got <= hi < p.rows, (lo, got, hi, p.rows)
    return out


def slack_case(be, N=10):
    """2. slack changes cost and the fallback share, never a list"""
    p = Peaked(be)
    seen = {}
    for slack in (0.0, 0.12, 10.0):
        out, st = p.run(N, slack=slack, max_fraction=1.0)
        check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)
        assert st["declined_users"] == 0 and st["certified_users"] + st["fallback_users"] == p.B, st
        seen[slack] = (st, p.m.rank_stats["kept_rows_per_user"])
        print(f"[pruned slack {slack}] {st} kept {seen[slack][1]} of {p.rows}")
    assert seen[10.0][1] == p.rows > 512 and seen[10.0][0]["certified_users"] == p.B        # everything kept: two cross-attention chunks, no frontier
    assert seen[0.0][1] < seen[0.12][1] < p.rows and seen[0.12][0]["certified_users"] == p.B
    return seen


def sabotage_case(be, N=10, victim=1):
    """3. a prefix the proposal lacks is detected: the deepest row of the oracle-best item's path removed from one user's sel"""
    p = Peaked(be)
    best = rank_cases.oracle_order(p.ref)[victim][0]
    path = [int(r) for r in p.ct.item_rows(0)[best] if r >= 0]
    gone = path[-1]
    hit = []

    def sabotage(sel, n_rows):
        n = int(n_rows[victim])
        row = sel[victim, :n].tolist()
        assert gone in row
        row.remove(gone)
        sel[victim, :n - 1] = torch.tensor(row, dtype=sel.dtype, device=sel.device)
        n_rows[victim] = n - 1
        hit.append(n)
    p.m._prune_sabotage = sabotage
    try:
        out, st = p.run(N, max_fraction=1.0)
    finally:
        p.m._prune_sabotage = None
    assert hit and st == {"pruned_calls": 1, "certified_users": p.B - 1, "fallback_users": 1, "declined_users": 0}, (hit, st)
    assert p.m.last_generate_path == "rank_pruned"
    check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)
    return out


def structure_case(be, ocfg, B, L, items, N, order, score_tol=FP32_TOL, seed=5):
    """4. random-init model, slack 10 and fraction 1: every row kept, every user certified (no frontier), the lists held to the oracle as
    the matching rank_items test holds them"""
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, "bf16")
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, seed)
    ct = rank_cases.compiled(items)
    out, st = call(m, ids, ww, mask, ct, N, slack=10.0, max_fraction=1.0)
    assert st == {"pruned_calls": 1, "certified_users": B, "fallback_users": 0, "declined_users": 0}, st
    assert m.last_generate_path == "rank_pruned" and m.rank_stats["kept_rows_per_user"] == ct.rank_plan(0)["rows"]
    ref = rank_cases.oracle_scores(params, ocfg, ids, ww, mask, items)
    check_lists(out, ref, items, B, N, None, order, score_tol)
    return out


def exclusion_case(be, N=10):
    """5. user 0 without the oracle's top 3 (certified), user 1 with fewer than N items left (falls back: filler beyond them), user 2 with
    everything excluded"""
    p = Peaked(be)
    n_items = len(p.items)
    orders = rank_cases.oracle_order(p.ref)
    rnd = random.Random(6)
    excluded = [orders[0][:3], sorted(rnd.sample(range(n_items), n_items - N // 2)), list(range(n_items))]
    out, st = p.run(N, excluded=excluded, max_fraction=1.0)
    assert st == {"pruned_calls": 1, "certified_users": 1, "fallback_users": 2, "declined_users": 0}, st
    check_lists(out, p.ref, p.items, p.B, N, excluded, "exact", FP32_TOL)
    idx, sc = out["item_index"].cpu(), out["sequences_scores"].cpu().view(p.B, N)
    assert int((idx[1] >= 0).sum()) == N // 2 and bool((idx[1, N // 2:] == -1).all()) and bool((sc[1, N // 2:] == -1e9).all())
    assert bool((idx[2] == -1).all()) and bool((sc[2] == -1e9).all()) and int(out["sequences"].cpu().view(p.B, N, -1)[2].abs().max()) == 0
    return out


def declines_case(be, ocfg, B=3, L=20, n_items=40, N=10):
    """6. a random-init model keeps (nearly) every row: with the default options the proposal is declined and the full fp32 pass answers"""
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, "bf16")
    m.eval()
    items = cases.make_items(n_items, 5, hi=min(60, ocfg.vocab_size - 1))
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    out, st = call(m, ids, ww, mask, rank_cases.compiled(items), N)
    assert m.last_generate_path == "rank_fp32" and st == {"pruned_calls": 1, "certified_users": 0, "fallback_users": 0, "declined_users": B}, (m.last_generate_path, st)
    check_lists(out, rank_cases.oracle_scores(params, ocfg, ids, ww, mask, items), items, B, N, None, "near", FP32_TOL)
    return out


def determinism_case(be, N=10):
    """7. two calls bit-identical in every output; one user per pass (a small rank_max_bytes): the same lists, scores within tolerance"""
    p = Peaked(be)
    a, st = p.run(N, max_fraction=1.0)
    b, _ = p.run(N, max_fraction=1.0)
    assert st["certified_users"] == p.B
    for k in ("sequences", "sequences_scores", "item_index"):
        assert torch.equal(a[k].cpu(), b[k].cpu()), f"{k} differs between two identical calls"
    lane, lib = p.m._cur_lane(), be.lib
    n_edges, n_items = len(p.ct.child_tok), len(p.items)
    need = lambda nb: max(int(lib.p5_rank_workspace_bytes(lane.engine_v, nb, p.L, p.rows, n_edges, n_items, N)),      # noqa: E731
                          int(lib.p5_rank_workspace_bytes(lane.engine, nb, p.L, p.rows, n_edges, n_items, N)),
                          int(lib.p5_prune_workspace_bytes(lane.engine_v, nb, p.L, p.rows, p.rows, n_edges, n_items, N)))
    assert need(2) > need(1)
    p.m.rank_max_bytes = need(2) - 1
    c, st = p.run(N, max_fraction=1.0)
    assert p.m.rank_stats["users_per_pass"] == 1 and st["certified_users"] == p.B, (p.m.rank_stats, st)
    assert torch.equal(a["item_index"].cpu(), c["item_index"].cpu()) and torch.equal(a["sequences"].cpu(), c["sequences"].cpu())
    assert float((a["sequences_scores"].cpu() - c["sequences_scores"].cpu()).abs().max()) <= FP32_TOL
    p.m.rank_max_bytes = need(1) - 1
    with pytest.raises(ValueError, match="rank_max_bytes"):
        p.run(N, max_fraction=1.0)
    return a


def errors_case(be, ocfg):
    """8. return_all_scores with pruning raises; on an fp32 model (and in draft mode) `pruned` has no effect"""
    items = cases.make_items(20, 5, hi=min(60, ocfg.vocab_size - 1))
    params = O.init_params(ocfg, 7)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, 2, 12, 4, 5)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=rank_cases.compiled(items), top_n=5)
    m = cases.build_model(be, ocfg, params, "bf16")
    m.eval()
    with pytest.raises(ValueError, match="return_all_scores"):
        m.rank_items(pruned=True, return_all_scores=True, **kw)
    before = dict(m.rank_stats)
    m.rank_items(pruned=True, generation_mode="draft", return_all_scores=True, **kw)
    assert m.last_generate_path == "rank_bf16" and delta(m, before)["pruned_calls"] == 0
    f = cases.build_model(be, ocfg, params, "fp32")
    f.eval()
    plain = f.rank_items(return_all_scores=True, **kw)
    before = dict(f.rank_stats)
    same = f.rank_items(pruned=True, return_all_scores=True, **kw)
    assert f.last_generate_path == "rank_fp32" and delta(f, before) == dict.fromkeys(STAT_KEYS, 0)
    for k in ("sequences", "sequences_scores", "item_index", "scores"):
        assert torch.equal(plain[k].cpu(), same[k].cpu()), k


def runner_case(be, tmp_path):
    """9. --test_exhaustive 2 on the toy dataset of rank_cases.runner_exhaustive_case (bf16 model): the metrics of --test_exhaustive 1, and
    rank_items is called with pruned=True (under 1: without the argument, as before)"""
    import random as _random
    from torch.utils.data import ConcatDataset, DataLoader
    from openp5_amd.collator import Collator
    from openp5_amd.data import MultiTaskDataset
    from openp5_amd.runner import DistributedRunner
    from openp5_amd.sampler import SingleMultiDataTaskSampler
    from openp5_amd.tokenizer import build_offline_tokenizer
    from tests.test_host import make_args
    tok = build_offline_tokenizer(2400)
    ocfg = O.T5Cfg(vocab_size=len(tok), d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=1)
    model = cases.build_model(be, ocfg, O.init_params(ocfg, 11), "bf16")
    got, seen = {}, {}
    plain = model.rank_items
    for flag in ("1", "2"):
        tmp = tmp_path / flag
        tmp.mkdir(parents=True, exist_ok=True)
        flags = ["--epochs", "1", "--test_before_train", "0", "--test_epoch", "0", "--metrics", "hit@1,hit@5,ndcg@5", "--batch_size", "8",
                 "--sample_num", "1,1", "--max_his", "8", "--eval_batch_size", "3", "--id_metrics", "1", "--test_exhaustive", flag,
                 "--test_filtered", "1", "--test_filtered_batch", "1"]
        args = make_args(str(tmp), flags, toy=dict(n_users=4, n_items=90, n_inter=4 * 75))
        _random.seed(0)
        train = ConcatDataset([MultiTaskDataset(args, "Toy", "train")])
        loader = DataLoader(train, sampler=SingleMultiDataTaskSampler(train, args.batch_size, args.seed), batch_size=args.batch_size, collate_fn=Collator(tok))
        r = DistributedRunner(model, tok, loader, None, torch.device("cpu") if be.is_emulator else be.device, args, 0)
        kws = []

        def counted(*a, _kws=kws, **kw):
            _kws.append(dict(kw))
            return plain(*a, **kw)
        model.rank_items = counted
        try:
            got[flag] = r.test()
        finally:
            model.rank_items = plain
        seen[flag] = kws
    assert seen["1"] and all("pruned" not in kw for kw in seen["1"])
    assert seen["2"] and all(kw.get("pruned") is True for kw in seen["2"])
    assert model.rank_stats["pruned_calls"] == len(seen["2"])
    assert len(got["1"]) == len(got["2"]) > 0
    for a, b in zip(got["1"], got["2"]):
        assert b == pytest.approx(a, abs=1e-12), (a, b)
    return got


def large_trie_declines_case(be, ocfg, trie, B=2, L=32, N=20, n_sample=40, score_tol=1e-4, seed=9):
    """10. T5-small width, the benchmark's trie, random init: the propose kernel over thousands of rows, then a decline; the returned top N
    and a seeded sample of items against O.sequence_scores (the checks of rank_cases.sampled_case on what a pruned call returns)"""
    from openp5_amd.trie import CompiledTrie
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, "bf16")
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = CompiledTrie.from_trie(trie)
    items = ct.enumerate_items()
    ct.index_items(items)
    out, st = call(m, ids, ww, mask, ct, N)
    assert m.last_generate_path == "rank_fp32" and st == {"pruned_calls": 1, "certified_users": 0, "fallback_users": 0, "declined_users": B}, (m.last_generate_path, st)
    rows, kept = ct.rank_plan(0)["rows"], m.rank_stats["kept_rows_per_user"]
    assert m.rank_prune_max_fraction * rows < kept <= rows
    idx, sc = out["item_index"].cpu(), out["sequences_scores"].cpu().view(B, N)
    sample = sorted(random.Random(seed).sample(range(len(items)), n_sample))
    worst = 0.0
    for b in range(B):
        top = [int(i) for i in idx[b].tolist()]
        assert min(top) >= 0 and len(set(top)) == N and bool((sc[b, 1:] <= sc[b, :-1]).all())
        ref = rank_cases.oracle_scores(params, ocfg, ids[b:b + 1], ww[b:b + 1], mask[b:b + 1], [items[i] for i in sample + top])[0]
        worst = max(worst, float((sc[b] - ref[n_sample:]).abs().max()))
        others = [float(s) for s, i in zip(ref[:n_sample].tolist(), sample) if i not in set(top)]
        assert all(s <= float(sc[b, -1]) + score_tol for s in others), "a sampled item outside the returned top scores above its last entry"
    print(f"[pruned large] items={len(items)} rows/user={rows} kept={kept}: max |score - oracle| over the returned top {N} = {worst:.3e} (tol {score_tol:.1e})")
    assert worst <= score_tol, worst
    return out
