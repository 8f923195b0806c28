"""Cases of bounded trie search (`P5T5Native.rank_items(pruned="search")`, csrc/p5_bound.h) shared by tests/test_rank_search_emu.py (host
emulation) and tests/test_gpu_rank_search.py (MI355X).  They follow tests/prune_cases.py and reuse its fixture, its oracle numbers and its
list check: the reference for every score and every order is the oracle over EVERY item, never `rank_items` and never the code under test.
Score tolerance prune_cases.FP32_TOL, certificate margin 1e-4."""
import random

import numpy as np
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, prune_cases, rank_cases
from tests.prune_cases import FP32_TOL, Peaked, check_lists

MARGIN = 1e-4
SEARCH_KEYS = ("search_calls", "search_certified_users", "search_fallback_users", "search_declined_users")


def counts(calls=1, certified=0, fallback=0, declined=0):
    return dict(zip(SEARCH_KEYS, (calls, certified, fallback, declined)))


def call(m, ids, ww, mask, ct, N, excluded=None, seed_items=None, **opts):
    """one rank_items(pruned="search") call with the model's search options set to `opts`; returns (out, the call's search counts)"""
    for k, v in opts.items():
        setattr(m, "rank_search_" + k, v)
    before = dict(m.rank_stats)
    out = m.rank_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, top_n=N, excluded_items=excluded, pruned="search",
                       seed_items=seed_items)
    assert {k: m.rank_stats[k] - before[k] for k in prune_cases.STAT_KEYS} == dict.fromkeys(prune_cases.STAT_KEYS, 0)
    assert m.rank_stats["kept_rows_per_user"] == before["kept_rows_per_user"]
    return out, {k: m.rank_stats[k] - before[k] for k in SEARCH_KEYS}


class Fixture(Peaked):
    """prune_cases.Peaked (tests/golden/peaked_tiny.pt: 300 items, 646 plan rows, 7 levels) with a bf16 or an fp32 model"""

    def __init__(self, be, dtype="bf16", B=3, seed=5):
        super().__init__(be, B, seed)
        if dtype != "bf16":
            self.m = cases.build_model(be, self.ocfg, self.params, dtype)
            self.m.eval()
        plan = self.ct.rank_plan(0)
        self.levels, self.parent = int(plan["levels"]), plan["row_parent"]
        self.orders = rank_cases.oracle_order(self.ref)

    def search(self, N=10, excluded=None, seed_items=None, **opts):
        opts.setdefault("max_fraction", 1.0)
        return call(self.m, self.ids, self.ww, self.mask, self.ct, N, excluded, seed_items, **opts)

    def ranks(self, lo, hi):
        """seed_items: every user's oracle ranks lo .. hi - 1"""
        return torch.tensor([o[lo:hi] for o in self.orders], dtype=torch.int64)

    def bounds(self, b):
        """the oracle's UB(r) = P(r) / Lmax(r) of every plan row of user b, by brute force over the items (as prune_cases.oracle_kept_rows)"""
        item_rows = self.ct.item_rows(0)
        P, lmax = np.zeros(self.rows, dtype=np.float64), np.zeros(self.rows, dtype=np.int64)
        lp_b = self.lp[b].double().numpy()
        for i, q in enumerate(self.items):
            n = len(q) - 1
            cum = np.concatenate(([0.0], np.cumsum(lp_b[i, :n])))
            for t in range(item_rows.shape[1]):
                r = int(item_rows[i, t])
                if r < 0:
                    break
                P[r] = cum[t]
                lmax[r] = max(lmax[r], n)
        return P / lmax


def certified_case(be, dtype, N=10):
    """1 / 2. certified equals the oracle with the default seeds (the model's own beam search), bf16-verified and fp32"""
    p = Fixture(be, dtype)
    assert p.m.rank_prune_margin == MARGIN and p.m.rank_search_max_fraction == 0.1 and p.m.rank_search_seed_beams is None
    out, st = p.search(N)
    assert p.m.last_generate_path == "rank_search", p.m.last_generate_path
    assert st == counts(certified=p.B), st
    check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)
    got, rounds = p.m.rank_stats["search_rows_per_user"], p.m.rank_stats["search_rounds"]
    print(f"[search certified {dtype}] rows reached {got} of {p.rows} in {rounds} rounds")
    assert got < p.rows == 646 and 1 <= rounds <= p.levels + 1, (got, rounds)
    return out


def seeds_bound_cost_case(be, N=10):
    """3. with the oracle's ranks 11-20 as seeds the rows reached lie between the oracle's count at tau_true (slack margin - 2 tol: every
    such row must be reached) and its count at the seeds' tau, the oracle's 20th score (slack margin + 2 tol: no other row can be)"""
    p = Fixture(be)
    out, st = p.search(N, seed_items=p.ranks(N, 2 * N))
    assert st == counts(certified=p.B), st
    check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)
    lo, hi, got = p.kept(N, MARGIN - 2 * FP32_TOL), p.kept(2 * N, MARGIN + 2 * FP32_TOL), p.m.rank_stats["search_rows_per_user"]
    print(f"[search seeds 11-20] rows reached {got} of {p.rows}; oracle counts {lo} .. {hi}")
    assert lo <= got <= hi < p.rows, (lo, got, hi)


def seeds_never_change_a_list_case(be, N=10):
    """4. seeds change cost, never a list"""
    p = Fixture(be)
    worst = torch.tensor([o[-N:] for o in p.orders], dtype=torch.int64)
    dup = p.ranks(0, N).clone()
    dup[:, 1::2] = dup[:, 0::2]                      # every seed twice
    seen = {}

    def junk(seeds):             # user 0: sequences that leave the trie; user 1: sequences cut short of their leaf; user 2: duplicates only
        seeds[0, :, 2] = p.ocfg.vocab_size - 1
        seeds[1, :, 2:] = 0
    for name, seeds, hook in (("top", p.ranks(0, N), None), ("next", p.ranks(N, 2 * N), None), ("worst", worst, None),
                              ("none", torch.full((p.B, N), -1, dtype=torch.int64), None), ("junk", dup, junk)):
        p.m._search_seed_hook = hook
        try:
            out, st = p.search(N, seed_items=seeds)
        finally:
            p.m._search_seed_hook = None
        check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)
        assert st["search_declined_users"] == 0 and st["search_certified_users"] + st["search_fallback_users"] == p.B, (name, st)
        seen[name] = (p.m.rank_stats["search_rows_per_user"], p.m.rank_stats["search_rounds"])
        print(f"[search seeds {name}] {st} rows {seen[name][0]} of {p.rows}, rounds {seen[name][1]}")
        assert seen[name][1] <= p.levels + 1
    assert seen["top"][0] <= seen["next"][0] <= seen["worst"][0] < p.rows, seen
    assert seen["none"][0] < p.rows and seen["junk"][0] < p.rows, seen
    return seen


def invariants_case(be, N=10):
    """5. every round: sel ascending, distinct, with row 0, closed under "parent of", a superset of the round before; at convergence it
    holds every row whose oracle bound reaches tau_true + 2 tol"""
    p = Fixture(be)
    log = []

    def hook(rnd, sel, n_rows):
        cur = [sel[b, :int(n_rows[b])].tolist() for b in range(p.B)]
        for b, rows in enumerate(cur):
            assert rows and rows[0] == 0 and all(x < y for x, y in zip(rows, rows[1:])) and rows[-1] < p.rows, (rnd, b)
            have = set(rows)
            assert all(int(p.parent[r]) in have for r in rows[1:]), (rnd, b)
            if log:
                assert set(log[-1][b]) <= have, (rnd, b)
        assert rnd == len(log) + 1
        log.append(cur)
    p.m._search_hook = hook
    try:
        out, st = p.search(N)
    finally:
        p.m._search_hook = None
    assert st == counts(certified=p.B) and len(log) == p.m.rank_stats["search_rounds"] >= 2, (st, len(log))
    assert log[-1] == log[-2]           # (the last round admitted nothing)
    for b in range(p.B):
        tau = float(p.ref[b, p.orders[b][N - 1]])
        must = set(np.nonzero(p.bounds(b) >= tau + 2 * FP32_TOL)[0].tolist())
        assert must <= set(log[-1][b]), (b, sorted(must - set(log[-1][b])))
    assert max(len(r) for r in log[-1]) == p.m.rank_stats["search_rows_per_user"]
    check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)


def removed_prefix_case(be, N=10, victim=1):
    """6. the deepest row of the oracle-best item's path taken out of one user's sel after round 2: healed or flagged, never a wrong list"""
    p = Fixture(be)
    best = p.orders[victim][0]
    gone = [int(r) for r in p.ct.item_rows(0)[best] if r >= 0][-1]
    hit = []

    def hook(rnd, sel, n_rows):
        if rnd != 2:
            return
        n = int(n_rows[victim])
        row = sel[victim, :n].tolist()
        assert gone in row
        row.remove(gone)
        sel[victim, :n - 1] = torch.tensor(row, dtype=sel.dtype, device=sel.device)
        n_rows[victim] = n - 1
        hit.append(n)
    p.m._search_hook = hook
    try:
        out, st = p.search(N)
    finally:
        p.m._search_hook = None
    print(f"[search removed prefix] {st} rounds {p.m.rank_stats['search_rounds']}")
    assert hit and p.m.rank_stats["search_rounds"] > 2
    assert st["search_declined_users"] == 0 and st["search_certified_users"] + st["search_fallback_users"] == p.B, st
    check_lists(out, p.ref, p.items, p.B, N, None, "exact", FP32_TOL)


def structure_case(be, ocfg, B, L, items, N, order, score_tol=FP32_TOL, seed=5, dtype="bf16"):
    """7. prune_cases.structure_case's inputs: a random-init model keeps every row (fraction 1), every user certified without a frontier"""
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, seed)
    ct = rank_cases.compiled(items)
    out, st = call(m, ids, ww, mask, ct, N, max_fraction=1.0)
    rows, levels = ct.rank_plan(0)["rows"], ct.rank_plan(0)["levels"]
    print(f"[search structure] {st} rows {m.rank_stats['search_rows_per_user']} of {rows}, rounds {m.rank_stats['search_rounds']}")
    assert st == counts(certified=B), st
    assert m.last_generate_path == "rank_search" and m.rank_stats["search_rows_per_user"] == rows and m.rank_stats["search_rounds"] <= levels + 1
    ref = rank_cases.oracle_scores(params, ocfg, ids, ww, mask, items)
    check_lists(out, ref, items, B, N, None, order, score_tol)
    return out


def exclusion_case(be, N=10):
    """8. prune_cases.exclusion_case's users: the oracle's top 3 excluded (certified), fewer than N items left (falls back: filler beyond
    them), everything excluded"""
    p = Fixture(be)
    n_items = len(p.items)
    rnd = random.Random(6)
    excluded = [p.orders[0][:3], sorted(rnd.sample(range(n_items), n_items - N // 2)), list(range(n_items))]
    out, st = p.search(N, excluded=excluded)
    assert st == counts(certified=1, fallback=2), st
    check_lists(out, p.ref, p.items, p.B, N, excluded, "exact", FP32_TOL)
    idx, sc = out["item_index"].cpu(), out["sequences_scores"].cpu().view(p.B, N)
    assert int((idx[1] >= 0).sum()) == N // 2 and bool((idx[1, N // 2:] == -1).all()) and bool((sc[1, N // 2:] == -1e9).all())
    assert bool((idx[2] == -1).all()) and bool((sc[2] == -1e9).all()) and int(out["sequences"].cpu().view(p.B, N, -1)[2].abs().max()) == 0


def declines_case(be, ocfg, B=3, L=20, n_items=40, N=10):
    """9. a random-init model keeps every row: with the default options the chunk is declined and the full pass answers"""
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, "bf16")
    m.eval()
    items = cases.make_items(n_items, 5, hi=min(60, ocfg.vocab_size - 1))
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = rank_cases.compiled(items)
    out, st = call(m, ids, ww, mask, ct, N)
    assert m.last_generate_path == "rank_fp32" and st == counts(declined=B), (m.last_generate_path, st)
    assert m.rank_search_max_fraction == 0.1 and m.rank_stats["search_rows_per_user"] > 0.1 * ct.rank_plan(0)["rows"]
    check_lists(out, rank_cases.oracle_scores(params, ocfg, ids, ww, mask, items), items, B, N, None, "near", FP32_TOL)


def determinism_case(be, N=10):
    """10. two calls bit-identical in every output; one user per pass (a small rank_max_bytes): the same lists, scores within tolerance;
    below one user's need: ValueError"""
    p = Fixture(be)
    a, st = p.search(N)
    b, _ = p.search(N)
    assert st["search_certified_users"] == p.B
    for k in ("sequences", "sequences_scores", "item_index"):
        assert torch.equal(a[k].cpu(), b[k].cpu()), f"{k} differs between two identical calls"
    lane, lib = p.m._cur_lane(), be.lib
    n_edges, n_items = len(p.ct.child_tok), len(p.items)
    need = lambda nb: max(int(lib.p5_rank_workspace_bytes(lane.engine_v, nb, p.L, p.rows, n_edges, n_items, N)),      # noqa: E731
                          int(lib.p5_bound_workspace_bytes(lane.engine_v, nb, p.L, p.rows, p.rows, n_edges, n_items, N, N, p.levels)))
    assert need(2) > need(1)
    keep = p.m.rank_max_bytes
    try:
        p.m.rank_max_bytes = need(2) - 1
        c, st = p.search(N)
        assert p.m.rank_stats["users_per_pass"] == 1 and st["search_certified_users"] == p.B, (p.m.rank_stats, st)
        assert torch.equal(a["item_index"].cpu(), c["item_index"].cpu()) and torch.equal(a["sequences"].cpu(), c["sequences"].cpu())
        assert float((a["sequences_scores"].cpu() - c["sequences_scores"].cpu()).abs().max()) <= FP32_TOL
        p.m.rank_max_bytes = need(1) - 1
        with pytest.raises(ValueError, match="rank_max_bytes"):
            p.search(N)
    finally:
        p.m.rank_max_bytes = keep


def errors_case(be, ocfg):
    """11. return_all_scores raises, an unknown `pruned` value raises, seed_items without the search raises; draft mode: the plain bf16 pass"""
    items = cases.make_items(20, 5, hi=min(60, ocfg.vocab_size - 1))
    params = O.init_params(ocfg, 7)
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, 2, 12, 4, 5)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=rank_cases.compiled(items), top_n=5)
    for dtype in ("bf16", "fp32"):
        m = cases.build_model(be, ocfg, params, dtype)
        m.eval()
        with pytest.raises(ValueError, match="return_all_scores"):
            m.rank_items(pruned="search", return_all_scores=True, **kw)
        for bad in ("Search", "yes", 2, None):
            with pytest.raises(ValueError, match="pruned"):
                m.rank_items(pruned=bad, **kw)
        with pytest.raises(ValueError, match="seed_items"):
            m.rank_items(seed_items=[[0], [1]], **kw)
        with pytest.raises(ValueError, match="seed_items"):
            m.rank_items(pruned="search", seed_items=[[0], [len(items)]], **kw)
    m = cases.build_model(be, ocfg, params, "bf16")
    m.eval()
    plain = m.rank_items(generation_mode="draft", return_all_scores=True, **kw)
    before = dict(m.rank_stats)
    same = m.rank_items(pruned="search", generation_mode="draft", return_all_scores=True, **kw)
    assert m.last_generate_path == "rank_bf16" and {k: m.rank_stats[k] - before[k] for k in SEARCH_KEYS} == dict.fromkeys(SEARCH_KEYS, 0)
    for k in ("sequences", "sequences_scores", "item_index", "scores"):
        assert torch.equal(plain[k].cpu(), same[k].cpu()), k


def runner_case(be, tmp_path):
    """12. --test_exhaustive 3 on the toy dataset of prune_cases.runner_case: the metrics of --test_exhaustive 1, and every rank_items call
    carries pruned="search" (under 1: no such argument, as before)"""
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
    for flag in ("1", "3"):
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
    assert seen["3"] and all(kw.get("pruned") == "search" for kw in seen["3"])
    assert model.rank_stats["search_calls"] == len(seen["3"]) and model.rank_stats["pruned_calls"] == 0
    assert len(got["1"]) == len(got["3"]) > 0
    for a, b in zip(got["1"], got["3"]):
        assert b == pytest.approx(a, abs=1e-12), (a, b)
    return got


def large_trie_declines_case(be, ocfg, trie, B=2, L=32, N=20, n_sample=40, score_tol=1e-4, seed=9):
    """13. T5-small width, the benchmark's trie, random init: the seed and expand kernels over ~1000-way levels, then a decline; the returned
    top N and a seeded sample of items against O.sequence_scores (the checks of prune_cases.large_trie_declines_case)"""
    from openp5_amd.trie import CompiledTrie
    params = O.init_params(ocfg, 7)
    m = cases.build_model(be, ocfg, params, "bf16")
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
    ct = CompiledTrie.from_trie(trie)
    items = ct.enumerate_items()
    ct.index_items(items)
    out, st = call(m, ids, ww, mask, ct, N)
    assert m.last_generate_path == "rank_fp32" and st == counts(declined=B), (m.last_generate_path, st)
    rows, kept = ct.rank_plan(0)["rows"], m.rank_stats["search_rows_per_user"]
    assert m.rank_search_max_fraction * rows < kept <= rows
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
    print(f"[search large] items={len(items)} rows/user={rows} reached={kept} in {m.rank_stats['search_rounds']} rounds: "
          f"max |score - oracle| over the returned top {N} = {worst:.3e} (tol {score_tol:.1e})")
    assert worst <= score_tol, worst
    return out
