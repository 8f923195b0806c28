"""Cases of per-user candidate scoring (`P5T5Native.score_candidates`, csrc/p5_cand.h) shared by tests/test_score_candidates_emu.py
(host emulation) and tests/test_gpu_score_candidates.py (MI355X).  The reference is always the oracle: `O.sequence_scores` on the
candidates' own token sequences; never `rank_items`, never the code under test."""
import random

import pytest
import torch

from oracle import t5_oracle as O
from tests import cases, rank_cases

EMPTY = -1.0e9


def pad_lists(lists):
    """ragged per-user lists -> LongTensor [B, C], -1 = empty slot"""
    C = max(len(c) for c in lists)
    out = torch.full((len(lists), C), -1, dtype=torch.int64)
    for b, c in enumerate(lists):
        out[b, :len(c)] = torch.tensor(c, dtype=torch.int64)
    return out


def seeded_lists(n_items, sizes, seed):
    rnd = random.Random(seed)
    return [rnd.sample(range(n_items), k) for k in sizes]


def oracle_scores(params, ocfg, ids, ww, mask, items, cand, toks=None):
    """O.sequence_scores of every user's own candidates: [B, C], -1e9 in the empty slots"""
    toks = rank_cases.items_tensor(items) if toks is None else toks
    with torch.no_grad():
        ref = O.sequence_scores(params, ocfg, ids, ww, mask, toks[cand.clamp(min=0)].contiguous())
    return torch.where(cand >= 0, ref, torch.full_like(ref, EMPTY))


def oracle_order(ref, cand):
    """per user: the live slots by (oracle score desc, item index asc)"""
    return [sorted((j for j in range(cand.shape[1]) if int(cand[b, j]) >= 0), key=lambda j: (-float(ref[b, j]), int(cand[b, j])))
            for b in range(cand.shape[0])]


def check_against_oracle(out, ref, cand, toks, N, score_tol, order, tag=""):
    """EVERY score elementwise; what is returned is consistent with itself; the order token-exact (`order` "exact": the oracle's smallest
    gap between ANY two candidates of a user is asserted >= 4 x score_tol first), rank by rank (`order` "near": the oracle's score of
    the returned item within 2 x score_tol of the oracle's score at that rank) or not judged (None: the bf16 engine)."""
    B, C = cand.shape
    got = out["scores"].cpu()
    assert got.shape == (B, C) and got.dtype == torch.float32
    live = cand >= 0
    assert bool((got[~live] == EMPTY).all()), "an empty slot must score -1e9"
    err = float((got - ref)[live].abs().max())
    print(f"[cand{tag}] B={B} C={C}: max |score - oracle| = {err:.3e} (tol {score_tol:.1e})")
    assert err <= score_tol, f"scores differ from O.sequence_scores by {err}"
    slot = out["order"].cpu()
    idx = out["item_index"].cpu()
    seq = out["sequences"].cpu().view(B, N, -1)
    sc = out["sequences_scores"].cpu().view(B, N)
    assert slot.shape == (B, N) and slot.dtype == torch.int64 and idx.shape == (B, N) and int(seq[:, :, 0].abs().max()) == 0
    orders = oracle_order(ref, cand)
    for b in range(B):
        n_live = min(N, len(orders[b]))
        assert bool((slot[b, n_live:] == -1).all()) and bool((idx[b, n_live:] == -1).all()) and bool((sc[b, n_live:] == EMPTY).all())
        assert int(seq[b, n_live:].abs().max() if n_live < N else 0) == 0, "ranks beyond the user's candidates: the all-pad sequence"
        for k in range(n_live):
            j = int(slot[b, k])
            assert 0 <= j < C and int(cand[b, j]) == int(idx[b, k]) >= 0
            assert seq[b, k, :toks.shape[1]].tolist() == toks[int(idx[b, k])].tolist() and int(seq[b, k, toks.shape[1]:].abs().sum()) == 0
            assert float(sc[b, k]) == float(got[b, j])
            if k:
                assert (float(sc[b, k]), -int(idx[b, k])) < (float(sc[b, k - 1]), -int(idx[b, k - 1])), "order: score desc, item index asc"
        assert len(set(slot[b, :n_live].tolist())) == n_live
    if order is None:
        return
    if order == "near":
        for b in range(B):
            for k in range(min(N, len(orders[b]))):
                assert abs(float(ref[b, int(slot[b, k])]) - float(ref[b, orders[b][k]])) <= 2 * score_tol, (b, k, int(slot[b, k]), orders[b][k])
        return
    assert order == "exact"
    gaps = torch.cat([ref[b][torch.tensor(orders[b])].diff().abs() for b in range(B) if len(orders[b]) > 1])
    assert float(gaps.min()) >= 4 * score_tol, f"oracle gap {float(gaps.min()):.2e} too small for a token-exact check at tolerance {score_tol}"
    for b in range(B):
        n_live = min(N, len(orders[b]))
        assert slot[b, :n_live].tolist() == orders[b][:n_live], (b, slot[b, :n_live].tolist(), orders[b][:n_live])


def cand_case(be, ocfg, B, L, items, lists, dtype="fp32", mode=None, score_tol=2e-5, top_n=None, order="exact", params=None, seed=5,
              params_fn=None, tag="", ct=None, toks=None):
    """score_candidates on per-user lists (`lists`: B lists of item indices, ragged allowed, or a [B, C] tensor) against the oracle"""
    params = params if params is not None else O.init_params(ocfg, 7)
    if params_fn is not None:
        params = params_fn(params, ocfg)
    m = cases.build_model(be, ocfg, params, dtype)
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, seed)
    cand = lists if torch.is_tensor(lists) else pad_lists(lists)
    N = int(top_n or cand.shape[1])
    ct = ct if ct is not None else rank_cases.compiled(items)
    out = m.score_candidates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, candidates=lists, top_n=top_n, generation_mode=mode)
    want_path = "cand_bf16" if (dtype == "bf16" and (mode or m.generation_mode) == "draft") else "cand_fp32"
    assert m.last_generate_path == want_path, m.last_generate_path
    toks = rank_cases.items_tensor(items) if toks is None else toks
    ref = oracle_scores(params, ocfg, ids, ww, mask, items, cand, toks)
    check_against_oracle(out, ref, cand, toks, N, score_tol, order, tag=f"{tag} {dtype}/{mode} rows/user={m.cand_stats['rows_per_user']}")
    return out, m, ref


def host_rows_per_user(ct, cand):
    """the largest per-user number of distinct non-leaf prefixes of the candidates, from item_paths with Python sets"""
    leaf = ct.child_off[1:] == ct.child_off[:-1]
    worst = 0
    for b in range(cand.shape[0]):
        nodes = set()
        for i in cand[b].tolist():
            if i >= 0:
                nodes.update(int(n) for n in ct.item_paths[i] if n >= 0 and not leaf[n])
        worst = max(worst, len(nodes))
    return worst


def every_score_case(be, ocfg, n_items):
    """case 1: lists of different content per user (seeded samples of 10 and n - 5 items, one user with all n); token-exact order"""
    items = cases.make_items(n_items, 11, hi=60)
    lists = seeded_lists(n_items, [10, n_items - 5], 21) + [list(range(n_items))]
    out, m, _ = cand_case(be, ocfg, 3, 12, items, lists, seed=11, tag=f" every n={n_items}")
    assert m.cand_stats["rows_per_user"] == host_rows_per_user(rank_cases.compiled(items), pad_lists(lists))
    return out


def ragged_case(be, ocfg):
    """case 2: lists of length 1, C and in between in one batch; -1 slots in the middle of a tensor"""
    items = cases.make_items(40, 11, hi=60)
    lists = seeded_lists(40, [1, 17, 6], 22)
    out, _, _ = cand_case(be, ocfg, 3, 12, items, lists, seed=11, tag=" ragged")
    assert bool((out["scores"].cpu()[0, 1:] == EMPTY).all()) and bool((out["item_index"].cpu()[0, 1:] == -1).all())
    cand = pad_lists(seeded_lists(40, [9, 9, 9], 23))
    cand[0, 3] = -1
    cand[1, 0] = -1
    cand[2, :8] = -1
    cand_case(be, ocfg, 3, 12, items, cand, seed=11, top_n=5, tag=" holes")


def over_512_rows_case(be, ocfg):
    """case 4: 300 items, all of them candidates: every row of the trie's plan (646 > 512), two chunks of cross-attention queries"""
    items = cases.make_items(300, 5, hi=min(60, ocfg.vocab_size - 1))
    out, m, _ = cand_case(be, ocfg, 2, 16, items, [list(range(300)), list(range(299, -1, -1))], order="near", tag=" 300")
    rows = rank_cases.compiled(items).rank_plan(0)["rows"]
    assert m.cand_stats["rows_per_user"] == rows == host_rows_per_user(rank_cases.compiled(items), torch.arange(300)[None]) and rows > 512
    return out


def rank_items_agreement_case(be, ocfg, B, L, items, lists, dtype="fp32", mode=None, score_tol=2e-5, seed=5, ct=None, tag=""):
    """case 6: the same model and inputs through rank_items(return_all_scores=True): the candidates' scores agree within the tolerance"""
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), dtype)
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, seed)
    ct = ct if ct is not None else rank_cases.compiled(items)
    cand = pad_lists(lists)
    a = m.score_candidates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, candidates=cand, generation_mode=mode)["scores"].cpu()
    r = m.rank_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, top_n=1, return_all_scores=True, generation_mode=mode)["scores"].cpu()
    want = torch.where(cand >= 0, torch.gather(r, 1, cand.clamp(min=0)), torch.full_like(a, EMPTY))
    err = float((a - want).abs().max())
    print(f"[cand vs rank_items{tag}] {dtype}/{mode} C={cand.shape[1]} of {len(items) if items is not None else r.shape[1]} items: "
          f"max |difference| = {err:.3e}; bit-equal: {bool(torch.equal(a, want))}")
    assert err <= score_tol
    return err


def determinism_case(be, ocfg, B, L, n_items, sizes, score_tol=2e-5, seed=5, params_fn=None):
    """case 7: two calls bit-identical in every returned tensor; tied slots in ascending item index; one user per pass (the smallest
    rank_max_bytes that holds one user) within the tolerance; one byte less raises ValueError naming rank_max_bytes"""
    items = cases.make_items(n_items, seed, hi=min(60, ocfg.vocab_size - 1))
    params = O.init_params(ocfg, 7)
    if params_fn is not None:
        params = params_fn(params, ocfg)
    m = cases.build_model(be, ocfg, params, "fp32")
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, seed)
    ct = rank_cases.compiled(items)
    cand = pad_lists(seeded_lists(n_items, sizes, seed + 2))
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, candidates=cand)
    a = m.score_candidates(**kw)
    b = m.score_candidates(**kw)
    keys = ("scores", "order", "item_index", "sequences", "sequences_scores")
    for k in keys:
        assert torch.equal(a[k].cpu(), b[k].cpu()), f"{k} differs between two identical calls"
    C = cand.shape[1]
    sc, idx = a["sequences_scores"].cpu().view(B, C), a["item_index"].cpu()
    ties = 0
    for u in range(B):
        for k in range(1, C):
            if int(idx[u, k]) < 0:
                break
            assert float(sc[u, k]) <= float(sc[u, k - 1])
            if float(sc[u, k]) == float(sc[u, k - 1]):
                ties += 1
                assert int(idx[u, k]) > int(idx[u, k - 1]), "tied slots must come in ascending item index"
    assert m.cand_stats["users_per_pass"] == B
    rows, path_len = m.cand_stats["rows_per_user"], ct.item_rows(0).shape[1]
    one = int(be.lib.p5_cand_workspace_bytes(m._cur_lane().engine, 1, L, C, path_len, rows))
    m.rank_max_bytes = one
    c = m.score_candidates(**kw)
    assert m.cand_stats["users_per_pass"] == 1
    chunk_bits = all(torch.equal(a[k].cpu(), c[k].cpu()) for k in keys)
    assert float((a["scores"].cpu() - c["scores"].cpu()).abs().max()) <= score_tol
    print(f"[cand determinism] ties among returned neighbours: {ties}; one user per pass bit-identical to the whole batch: {chunk_bits}")
    m.rank_max_bytes = one - 1
    with pytest.raises(ValueError, match="rank_max_bytes"):
        m.score_candidates(**kw)
    return ties, chunk_bits


def permutation_case(be, ocfg):
    """case 8: permuting a user's list permutes `scores` bit for bit and leaves item_index / sequences_scores bit-identical"""
    items = cases.make_items(60, 11, hi=60)
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, 3, 12, 4, 11)
    ct = rank_cases.compiled(items)
    cand = pad_lists(seeded_lists(60, [25, 25, 12], 31))
    g = torch.Generator().manual_seed(3)
    perm = torch.stack([torch.randperm(cand.shape[1], generator=g) for _ in range(3)])
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct)
    a = m.score_candidates(candidates=cand, **kw)
    b = m.score_candidates(candidates=torch.gather(cand, 1, perm), **kw)
    assert torch.equal(torch.gather(a["scores"].cpu(), 1, perm), b["scores"].cpu())
    for k in ("item_index", "sequences", "sequences_scores"):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    sa, sb = a["order"].cpu(), b["order"].cpu()
    live = sb >= 0
    assert torch.equal(live, sa >= 0) and torch.equal(torch.gather(perm, 1, sb.clamp(min=0))[live], sa[live])


def range_guard_case(be, ocfg, B=3, L=20, n_items=40, scale=3.0e5, seed=5, score_tol=5e-5):
    """case 9: the out-of-range decoder FFN of rank_cases.range_guard_case: every user flagged by the split-product pass, rescored with
    exact fp32 products, scores the oracle's"""
    params = O.init_params(ocfg, 7)
    for k in list(params):
        if "DenseReluDense.wi" in k and ".decoder." in "." + k:
            params[k] = params[k] * scale
        if "DenseReluDense.wo" in k and ".decoder." in "." + k:
            params[k] = params[k] / scale
    items = cases.make_items(n_items, seed, hi=min(60, ocfg.vocab_size - 1))
    out, m, _ = cand_case(be, ocfg, B, L, items, seeded_lists(n_items, [20] * B, 41), dtype="bf16", mode="verified", score_tol=score_tol, top_n=10,
                          order="near", params=params, seed=seed, tag=" guard")
    assert m.cand_stats["rescored_users"] == B, m.cand_stats
    return out


def errors_case(be, ocfg):
    """case 10"""
    from openp5_amd.trie import Trie
    items = cases.make_items(20, 5, hi=min(60, ocfg.vocab_size - 1))
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    m.eval()
    ids, ww, mask, _, _ = cases.synth_batch(ocfg, 2, 12, 4, 5)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww)
    ok = [[0, 3, 5], [7, 2]]
    with pytest.raises(ValueError, match="trie"):
        m.score_candidates(candidates=ok, **kw)
    bos = min(61, ocfg.vocab_size - 2)
    grafted = Trie([list(it[:4]) + [bos] for it in items])
    grafted.append(Trie([list(it[4:]) for it in items]), bos)
    with pytest.raises(ValueError, match="appended trie"):
        m.score_candidates(trie=grafted, candidates=ok, **kw)
    for bad in ([[0, 20], [1]], [[0, 1], [-2]]):
        with pytest.raises(ValueError, match="item indices"):
            m.score_candidates(trie=Trie(items), candidates=bad, **kw)
    with pytest.raises(ValueError, match="twice"):
        m.score_candidates(trie=Trie(items), candidates=[[4, 1, 4], [2]], **kw)
    with pytest.raises(ValueError, match="4096"):
        m.score_candidates(trie=Trie(items), candidates=torch.full((2, 4097), -1, dtype=torch.int64), **kw)
    for n in (0, 4):
        with pytest.raises(ValueError, match="top_n"):
            m.score_candidates(trie=Trie(items), candidates=ok, top_n=n, **kw)
    long_items = [[0] + [7 + (i % 50) for i in range(m.LUT_HALF + 1)] + [1], [0, 8, 1]]
    with pytest.raises(ValueError, match="longer than"):
        m.score_candidates(trie=Trie(long_items), candidates=[[0], [1]], **kw)
    m.rank_max_bytes = 1024
    with pytest.raises(ValueError, match="rank_max_bytes"):
        m.score_candidates(trie=Trie(items), candidates=ok, **kw)
    m.rank_max_bytes = type(m).rank_max_bytes
    # a plain Trie is compiled and indexed on demand: items numbered in lexicographic order (make_items returns them sorted); -1 is an empty slot
    out = m.score_candidates(trie=Trie(items), candidates=[[0, 3, -1, 5], [7, 2]], **kw)
    cand = torch.tensor([[0, 3, -1, 5], [7, 2, -1, -1]])
    ref = oracle_scores(O.init_params(ocfg, 7), ocfg, ids, ww, mask, items, cand)
    assert float((out["scores"].cpu() - ref).abs().max()) <= 2e-5


def workspace_case(be):
    """case 11, host-only part: the prototype carries no catalogue size, and 100 candidates need less than the 3,416-item catalogue"""
    import bench
    from openp5_amd import _abi
    from openp5_amd.trie import CompiledTrie
    res, args = _abi.PROTOTYPES["p5_cand_workspace_bytes"]
    assert len(args) == 6, "p5_cand_workspace_bytes(engine, B, L, C, path_len, rows_per_user): no n_items / n_edges"
    ocfg = O.T5Cfg.named("t5-small")
    m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "fp32")
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    ct.index_items(ct.enumerate_items())
    plan = ct.rank_plan(0)
    eng = m._cur_lane().engine
    cand = int(be.lib.p5_cand_workspace_bytes(eng, 8, 128, 100, ct.item_rows(0).shape[1], 304))
    rank = int(be.lib.p5_rank_workspace_bytes(eng, 8, 128, plan["rows"], len(ct.child_tok), 3416, 10))
    head = int(be.lib.p5_cand_workspace_bytes(eng, 8, 128, 100, ct.item_rows(0).shape[1], 0))
    print(f"[cand workspace] B=8 L=128: 100 candidates / 304 rows {cand} bytes (plan part {head}); rank_items of 3416 items / {plan['rows']} rows {rank} bytes")
    assert 0 < head < cand < rank


def runner_args(tmp_path, id_metrics, extra=()):
    from tests.test_host import make_args
    tmp_path.mkdir(parents=True, exist_ok=True)
    flags = ["--epochs", "1", "--test_before_train", "0", "--test_epoch", "0", "--metrics", "hit@1,hit@5,ndcg@5", "--batch_size", "8",
             "--sample_num", "1,1", "--max_his", "8", "--eval_batch_size", "3", "--id_metrics", id_metrics] + list(extra)
    return make_args(str(tmp_path), flags, toy=dict(n_users=4, n_items=90, n_inter=4 * 75))


def make_runner(be, args, ocfg_seed=11, model=None):
    import random as _random
    from torch.utils.data import ConcatDataset, DataLoader
    from openp5_amd.collator import Collator
    from openp5_amd.data import MultiTaskDataset
    from openp5_amd.runner import DistributedRunner
    from openp5_amd.sampler import SingleMultiDataTaskSampler
    from openp5_amd.tokenizer import build_offline_tokenizer
    tok = build_offline_tokenizer(2400)
    _random.seed(0)
    train = ConcatDataset([MultiTaskDataset(args, "Toy", "train")])
    loader = DataLoader(train, sampler=SingleMultiDataTaskSampler(train, args.batch_size, args.seed), batch_size=args.batch_size, collate_fn=Collator(tok))
    ocfg = O.T5Cfg(vocab_size=len(tok), d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=1)
    params = O.init_params(ocfg, ocfg_seed)
    model = model if model is not None else cases.build_model(be, ocfg, params, "fp32")
    r = DistributedRunner(model, tok, loader, None, torch.device("cpu") if be.is_emulator else be.device, args, 0)
    return r, tok, ocfg, params, model


def runner_candidates_case(be, tmp_path, id_metrics, n_neg=20):
    """case 12: the toy dataset of rank_cases.runner_exhaustive_case under --test_candidates 20.  First the sampler on its own, then the
    runner's metrics against the metrics computed from O.sequence_scores over the same lists."""
    from openp5_amd import evaluate
    from openp5_amd.runner import DistributedRunner
    args = runner_args(tmp_path, id_metrics, ["--test_candidates", str(n_neg)])
    r, tok, ocfg, params, model = make_runner(be, args)
    args1 = runner_args(tmp_path, id_metrics, ["--test_candidates", str(n_neg), "--eval_batch_size", "1"])
    r1 = DistributedRunner(model, tok, r.train_loader, None, r.device, args1, 0)
    assert len(r.testloaders) == len(r1.testloaders) >= 1
    for tl, tl1 in zip(r.testloaders, r1.testloaders):
        ds = tl.dataset
        by_user = {}
        for batch in tl:
            users = batch[5].tolist()
            for u, items in zip(users, r.candidate_lists(ds, users)):
                by_user[u] = items
        again = {}
        for batch in tl1:
            assert len(batch[5]) == 1
            again[int(batch[5][0])] = r1.candidate_lists(tl1.dataset, batch[5].tolist())[0]
        assert by_user == again, "the lists must not depend on the construction or on eval_batch_size"
        assert len(by_user) == len(ds) == 4
        for u, items in by_user.items():
            user = ds.id2user[u]
            gold = ds.reindex_user_seq_dict[user][-1]
            pool = set(ds.all_items) - set(ds.positive[user]) - {gold}
            assert items[0] == gold and items.count(gold) == 1 and len(items) == min(n_neg, len(pool)) + 1 == len(set(items))
            assert set(items[1:]) <= pool
            # (the toy's users have 6, 0, 74 and 31 unseen items: two of them take all they have; a draw of 5 samples for three of them)
            few = [evaluate.sample_candidates(ds.all_items, ds.positive[user], gold, 5, s, ds.dataset, user) for s in (args.seed, args.seed, args.seed + 1)]
            assert few[0] == few[1] and few[0][0] == gold and len(set(few[0])) == min(5, len(pool)) + 1 and set(few[0][1:]) <= pool
            assert len(pool) <= 5 or few[0] != few[2], "another seed draws another list"
        assert sorted(len(v) for v in by_user.values()) == [1, 7, 21, 21]
        assert len({tuple(v) for v in by_user.values()}) == len(by_user), "users must draw different lists"
        drawn = [tuple(evaluate.sample_candidates(ds.all_items, set(), "none", 5, args.seed, ds.dataset, ds.id2user[u])) for u in by_user]
        assert len(set(drawn)) == len(drawn), "the same pool, different users: different draws"
    calls = {"n": 0}
    plain = model.score_candidates

    def counted(*a, **kw):
        calls["n"] += 1
        return plain(*a, **kw)
    model.score_candidates = counted
    got = r.test()
    assert calls["n"] > 0 and model.last_generate_path == "cand_fp32"
    k = min(r.generate_num, n_neg + 1)
    for li, tl in enumerate(r.testloaders):
        ds = tl.dataset
        _, ct, index = r._dataset_trie(ds)
        toks = torch.from_numpy(ct.item_tokens)
        res, total = 0, 0
        for batch in tl:
            lists = r.candidate_lists(ds, batch[5].tolist())
            gold = tok.batch_decode(batch[3], skip_special_tokens=True)
            gen, scores = [], []
            for b, items in enumerate(lists):       # (ragged lists: every user scored on its own, ranks beyond its list never hit)
                cand = torch.tensor([index[i] for i in items])
                with torch.no_grad():
                    ref = O.sequence_scores(params, ocfg, batch[0][b:b + 1], batch[2][b:b + 1], batch[1][b:b + 1], toks[cand][None].contiguous())[0]
                order = sorted(range(len(items)), key=lambda j: (-float(ref[j]), int(cand[j])))[:k]
                gen += tok.batch_decode(toks[cand[order]], skip_special_tokens=True) + [""] * (k - len(order))
                scores += [float(ref[j]) for j in order] + [EMPTY] * (k - len(order))
            rel = evaluate.rel_results(gen, gold, scores, k)
            total += len(rel)
            res = res + evaluate.get_metrics_results(rel, r.metrics)
        want = dict(zip(r.metrics, (torch.as_tensor(res, dtype=torch.float64) / total).tolist()))
        assert got[li] == pytest.approx(want, abs=1e-12), (li, got[li], want)
    return got


def runner_flag_errors_case(be, tmp_path):
    args = runner_args(tmp_path, "1", ["--test_candidates", "5", "--test_exhaustive", "1"])
    with pytest.raises(ValueError, match="test_candidates"):
        make_runner(be, args)


def runner_filtered_precedence_case(be, tmp_path, caplog):
    """--test_filtered 1 with --test_candidates: the candidates protocol runs (same metrics as without --test_filtered up to the
    collator's whole-word rule) and the log says so once"""
    import logging
    args = runner_args(tmp_path, "1", ["--test_candidates", "20", "--test_filtered", "1"])
    r, *_ = make_runner(be, args)
    model = r.model
    model.rank_items = model.generate = None          # (neither may be reached)
    with caplog.at_level(logging.INFO):
        r.test()
        r.test()
    said = [rec for rec in caplog.records if "takes precedence" in rec.getMessage()]
    assert len(said) == 1 and model.last_generate_path == "cand_fp32"
