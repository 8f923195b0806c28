"""gpu: exhaustive catalogue ranking (`P5T5Native.rank_items`, csrc/p5_rank.h) on the MI355X against the oracle's score of every item
(tests/rank_cases.py), at toy sizes and at the benchmark's ML-1M-shaped and a Yelp-sized catalogue."""
import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases
from tests.wide_cases import tie_heavy_params

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")


def _items(n, **kw):
    return cases.make_items(n, 5, hi=min(60, TINY.vocab_size - 1), **kw)


@pytest.mark.parametrize("n_items", [40, 90])
def test_every_score_and_the_order_fp32(hip, n_items):
    """token-exact order: inputs (seed 11, L = 12) whose oracle scores are at least 1.07e-4 apart at both sizes (4 x tolerance = 8e-5)"""
    rank_cases.rank_case(hip, TINY, 3, 12, cases.make_items(n_items, 11, hi=60), top_n=n_items, seed=11)


def test_every_score_bf16_verified(hip):
    rank_cases.rank_case(hip, TINY, 3, 20, _items(40), dtype="bf16", mode="verified", top_n=10)


def test_every_score_bf16_draft(hip):
    rank_cases.rank_case(hip, TINY, 3, 20, _items(40), dtype="bf16", mode="draft", score_tol=cases.BF16_SCORE_TOL, top_n=10, order=None)


def test_300_items_cross_the_512_query_limit(hip):
    out, m, _ = rank_cases.rank_case(hip, TINY, 2, 16, _items(300), top_n=300, order="ties")
    assert m.rank_stats["rows_per_user"] > 512


def test_wide_level_of_250_siblings(hip):
    rank_cases.rank_case(hip, TINY, 2, 12, rank_cases.fanout_items(250), score_tol=5e-5, top_n=65, order="near", seed=3)


def test_items_of_unequal_length_and_a_padded_input_row(hip):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    rank_cases.rank_case(hip, TINY, 3, 14, items, top_n=30, order="ties", seed=11)


def test_gated_gelu(hip):
    rank_cases.rank_case(hip, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), top_n=30, order="ties", seed=11)


@pytest.mark.parametrize("n_items", [40, 90])
def test_equals_the_widened_beam_protocol_in_its_limit(hip, n_items):
    rank_cases.protocol_link_case(hip, TINY, 3, 12, n_items, seed=11)


def test_exclusion(hip):
    rank_cases.exclusion_case(hip, TINY, 3, 20, 40, 10)


def test_deterministic_and_user_chunks(hip):
    rank_cases.determinism_case(hip, TINY, 3, 20, 40, 10)


def test_deterministic_with_ties(hip):
    ties, _ = rank_cases.determinism_case(hip, TINY, 2, 12, 40, 40, params_fn=tie_heavy_params)
    assert ties > 0


def test_range_guard_rescores_flagged_users(hip):
    rank_cases.range_guard_case(hip, TINY)


def test_collab_dims_t5_base_width(hip):
    """T5-base width (2 + 2 layers, the vocabulary of collaborative indexing), the dims of cases.generate_verified_collab_case"""
    import random
    ocfg = O.T5Cfg.named("t5-base", num_layers=2, num_decoder_layers=2, vocab_size=32600)
    rnd = random.Random(3)
    items = set()
    while len(items) < 120:
        items.add(tuple([0, 5] + [rnd.randint(32100, 32599) for _ in range(rnd.randint(2, 4))] + [1]))
    rank_cases.rank_case(hip, ocfg, 2, 40, sorted(list(x) for x in items), dtype="bf16", mode="verified", score_tol=2e-4, top_n=20, order="near")


@pytest.mark.parametrize("id_metrics", ["1", "0"])
def test_runner_exhaustive_filtered(hip, tmp_path, id_metrics):
    rank_cases.runner_exhaustive_case(hip, tmp_path / "x", id_metrics, True, "1")


def test_runner_exhaustive_unfiltered(hip, tmp_path):
    rank_cases.runner_exhaustive_case(hip, tmp_path / "x", "1", False)


@pytest.mark.parametrize("dtype,mode", [("fp32", None), ("bf16", "verified")])
def test_ml1m_shaped_catalogue_t5_small(hip, dtype, mode):
    """T5-small dims, the benchmark's 3416-item trie (5499 rows per user)"""
    import bench
    rank_cases.sampled_case(hip, O.T5Cfg.named("t5-small"), bench.synth_item_trie(3416, 7), 2, 32, dtype, mode, 1e-4, tag=" ml1m")


def test_yelp_sized_catalogue(hip):
    """112,394 items, 219,666 rows per user, d_model 64: the catalogue size no beam width reaches"""
    import bench
    ocfg = O.T5Cfg(vocab_size=4096, d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=1)
    out = rank_cases.sampled_case(hip, ocfg, bench.synth_item_trie(112394, 7, pieces=(3, 3, 3)), 2, 16, "fp32", None, 2e-5, tag=" yelp")
    assert out["scores"].shape[1] == 112394
