"""gpu: per-user candidate scoring (`P5T5Native.score_candidates`, csrc/p5_cand.h) on the MI355X against the oracle's score of every
candidate (tests/cand_cases.py), at toy sizes, on the benchmark's ML-1M-shaped catalogue and on a Yelp-sized one."""
import random

import pytest
import torch

from oracle import t5_oracle as O
from tests import cand_cases, cases, rank_cases
from tests.wide_cases import tie_heavy_params

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")


def _items(n, **kw):
    return cases.make_items(n, 5, hi=min(60, TINY.vocab_size - 1), **kw)


def _halves(n, B, seed):
    return cand_cases.seeded_lists(n, [n // 2] * B, seed)


@pytest.mark.parametrize("n_items", [40, 90])
def test_every_score_and_the_order_fp32(hip, n_items):
    cand_cases.every_score_case(hip, TINY, n_items)


def test_ragged_lists_and_empty_slots(hip):
    cand_cases.ragged_case(hip, TINY)


def test_every_score_bf16_verified(hip):
    cand_cases.cand_case(hip, TINY, 3, 20, _items(40), _halves(40, 3, 51), dtype="bf16", mode="verified", top_n=10, order="near")


def test_every_score_bf16_draft(hip):
    cand_cases.cand_case(hip, TINY, 3, 20, _items(40), _halves(40, 3, 51), dtype="bf16", mode="draft", score_tol=cases.BF16_SCORE_TOL, top_n=10, order=None)


def test_300_candidates_cross_the_512_query_limit(hip):
    cand_cases.over_512_rows_case(hip, TINY)


def test_wide_level_of_250_siblings(hip):
    cand_cases.cand_case(hip, TINY, 2, 12, rank_cases.fanout_items(250), _halves(250, 2, 52), score_tol=5e-5, top_n=65, order="near", seed=3, tag=" fanout")


def test_items_of_unequal_length_and_a_padded_input_row(hip):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    cand_cases.cand_case(hip, TINY, 3, 14, items, _halves(30, 3, 53), order="near", seed=11, tag=" unequal")


def test_gated_gelu(hip):
    cand_cases.cand_case(hip, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), _halves(30, 2, 54), order="near", seed=11,
                         tag=" gated")


def test_agrees_with_rank_items(hip):
    cand_cases.rank_items_agreement_case(hip, TINY, 3, 12, cases.make_items(90, 11, hi=60), cand_cases.seeded_lists(90, [30, 12, 45], 55), seed=11)


def test_deterministic_and_user_chunks(hip):
    cand_cases.determinism_case(hip, TINY, 3, 20, 40, [20, 20, 9])


def test_deterministic_with_ties(hip):
    ties, _ = cand_cases.determinism_case(hip, TINY, 2, 12, 40, [40, 25], params_fn=tie_heavy_params)
    assert ties > 0


def test_permuting_a_list_permutes_its_scores(hip):
    cand_cases.permutation_case(hip, TINY)


def test_range_guard_rescores_flagged_users(hip):
    cand_cases.range_guard_case(hip, TINY)


def test_errors_and_on_demand_indexing(hip):
    cand_cases.errors_case(hip, TINY)


def test_workspace_does_not_grow_with_the_catalogue(hip):
    cand_cases.workspace_case(hip)


@pytest.mark.parametrize("id_metrics", ["1", "0"])
def test_runner_sampled_candidates(hip, tmp_path, id_metrics):
    cand_cases.runner_candidates_case(hip, tmp_path / "c", id_metrics)


def _catalogue(trie):
    from openp5_amd.trie import CompiledTrie
    ct = CompiledTrie.from_trie(trie)
    items = ct.enumerate_items()
    ct.index_items(items)
    return ct, items, torch.from_numpy(ct.item_tokens)


@pytest.mark.parametrize("dtype,mode", [("fp32", None), ("bf16", "verified")])
def test_ml1m_shaped_catalogue_t5_small(hip, dtype, mode):
    """T5-small dims, the benchmark's 3416-item trie, 100 seeded candidates per user; and the same scores through rank_items"""
    import bench
    ct, items, toks = _catalogue(bench.synth_item_trie(3416, 7))
    lists = cand_cases.seeded_lists(3416, [100, 100], 61)
    ocfg = O.T5Cfg.named("t5-small")
    cand_cases.cand_case(hip, ocfg, 2, 32, items, lists, dtype=dtype, mode=mode, score_tol=1e-4, order="near", ct=ct, toks=toks, tag=" ml1m")
    cand_cases.rank_items_agreement_case(hip, ocfg, 2, 32, None, lists, dtype=dtype, mode=mode, score_tol=1e-4, ct=ct, tag=" ml1m")


def test_yelp_sized_catalogue(hip):
    """112,394 items, tiny width: C = 100 (about 300 rows per user) in ONE pass inside exactly the bytes p5_cand_workspace_bytes names,
    and C = 1000 (about 2,630 rows per user: six cross-attention chunks); every candidate against the oracle"""
    import bench
    ocfg = O.T5Cfg(vocab_size=4096, d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=1)
    ct, items, toks = _catalogue(bench.synth_item_trie(112394, 7, pieces=(3, 3, 3)))
    B, L = 2, 16
    for C in (100, 1000):
        lists = cand_cases.seeded_lists(112394, [C] * B, 70 + C)
        rows = cand_cases.host_rows_per_user(ct, cand_cases.pad_lists(lists))
        params = O.init_params(ocfg, 7)
        m = cases.build_model(hip, ocfg, params, "fp32")
        m.eval()
        need = int(hip.lib.p5_cand_workspace_bytes(m._cur_lane().engine, B, L, C, ct.item_rows(0).shape[1], rows))
        m.rank_max_bytes = need
        ids, ww, mask, _, _ = cases.synth_batch(ocfg, B, L, 4, 5)
        cand = cand_cases.pad_lists(lists)
        out = m.score_candidates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, candidates=cand)
        assert m.cand_stats["rows_per_user"] == rows and m.cand_stats["users_per_pass"] == B, (m.cand_stats, rows)
        ref = cand_cases.oracle_scores(params, ocfg, ids, ww, mask, None, cand, toks)
        cand_cases.check_against_oracle(out, ref, cand, toks, C, 2e-5, "near", tag=f" yelp rows/user={rows} workspace={need}")
    assert rows > 5 * 512 > 0


def test_collab_dims_t5_base_width(hip):
    """T5-base width (2 + 2 layers, the vocabulary of collaborative indexing), the config and items of the rank_items test"""
    ocfg = O.T5Cfg.named("t5-base", num_layers=2, num_decoder_layers=2, vocab_size=32600)
    rnd = random.Random(3)
    items = set()
    while len(items) < 120:
        items.add(tuple([0, 5] + [rnd.randint(32100, 32599) for _ in range(rnd.randint(2, 4))] + [1]))
    cand_cases.cand_case(hip, ocfg, 2, 40, sorted(list(x) for x in items), _halves(120, 2, 81), dtype="bf16", mode="verified", score_tol=2e-4, top_n=20,
                         order="near", tag=" collab")


@pytest.mark.parametrize("lanes", [2, 3])
def test_lanes_match_one_at_a_time(hip, lanes):
    """map_lanes over batches of different B and C returns the bits of one-at-a-time calls"""
    items = cases.make_items(90, 11, hi=60)
    ct = rank_cases.compiled(items)
    m = cases.build_model(hip, TINY, O.init_params(TINY, 7), "bf16")
    m.eval()
    batches = []
    for i, (B, C) in enumerate([(3, 20), (1, 45), (4, 7), (2, 90), (3, 33), (2, 12)]):
        ids, ww, mask, _, _ = cases.synth_batch(TINY, B, 12 + i, 4, 30 + i)
        batches.append(dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, candidates=cand_cases.pad_lists(cand_cases.seeded_lists(90, [C] * B, 90 + i))))
    keys = ("scores", "order", "item_index", "sequences", "sequences_scores")

    def one(kw):
        out = m.score_candidates(trie=ct, **kw)
        return {k: out[k].cpu() for k in keys}
    want = [one(kw) for kw in batches]
    got = list(m.map_lanes(one, batches, lanes=lanes))
    for w, g in zip(want, got):
        for k in keys:
            assert torch.equal(w[k], g[k]), k
