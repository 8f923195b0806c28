"""gpu: bounded trie search (`P5T5Native.rank_items(pruned="search")`, csrc/p5_bound.h) on the MI355X against
the oracle's score of every item (tests/search_cases.py), and the seed and expand kernels at the benchmark's catalogue."""
import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases, search_cases

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")


def test_certified_equals_the_oracle(hip):
    search_cases.certified_case(hip, "bf16")


def test_certified_equals_the_oracle_fp32_model(hip):
    search_cases.certified_case(hip, "fp32")


def test_given_seeds_bound_the_cost(hip):
    search_cases.seeds_bound_cost_case(hip)


def test_seeds_change_cost_never_a_list(hip):
    search_cases.seeds_never_change_a_list_case(hip)


def test_invariants_of_every_round(hip):
    search_cases.invariants_case(hip)


def test_a_removed_prefix_is_healed_or_flagged(hip):
    search_cases.removed_prefix_case(hip)


def test_wide_level_of_250_siblings(hip):
    search_cases.structure_case(hip, TINY, 2, 12, rank_cases.fanout_items(250), 65, "near", score_tol=5e-5, seed=3)


def test_items_of_unequal_length_and_a_padded_input_row(hip):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    search_cases.structure_case(hip, TINY, 3, 14, items, 30, "near", seed=11)


def test_gated_gelu(hip):
    search_cases.structure_case(hip, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), 30, "near", seed=11)


def test_one_user(hip):
    search_cases.structure_case(hip, TINY, 1, 12, cases.make_items(40, 11, hi=60), 10, "near", seed=11)


def test_top_n_equal_to_the_item_count(hip):
    """token-exact: the inputs of test_rank_items_emu.test_every_score_and_the_order_fp32, whose oracle scores are >= 1.07e-4 apart"""
    search_cases.structure_case(hip, TINY, 3, 12, cases.make_items(40, 11, hi=60), 40, "exact", seed=11)


def test_exclusion(hip):
    search_cases.exclusion_case(hip)


def test_declines_on_a_random_init_model(hip):
    search_cases.declines_case(hip, TINY)


def test_deterministic_and_user_chunks(hip):
    search_cases.determinism_case(hip)


def test_errors_and_no_effect_in_draft_mode(hip):
    search_cases.errors_case(hip, TINY)


def test_runner_exhaustive_3(hip, tmp_path):
    search_cases.runner_case(hip, tmp_path)


def test_ml1m_shaped_catalogue_t5_small_declines(hip):
    """T5-small dims, the benchmark's 3416-item trie (5499 rows per user, about 1000-way levels), random init"""
    import bench
    search_cases.large_trie_declines_case(hip, O.T5Cfg.named("t5-small"), bench.synth_item_trie(3416, 7))
