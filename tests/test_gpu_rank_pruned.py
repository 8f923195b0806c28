"""gpu: certified pruned ranking (`P5T5Native.rank_items(pruned=True)`, csrc/p5_prune.h) on the MI355X against the oracle's score of every
item (tests/prune_cases.py), and the propose kernel at the benchmark's catalogue."""
import pytest

from oracle import t5_oracle as O
from tests import cases, prune_cases, rank_cases

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")


def test_certified_equals_the_oracle(hip):
    prune_cases.certified_case(hip)


def test_slack_never_changes_the_answer(hip):
    prune_cases.slack_case(hip)


def test_a_missing_prefix_is_detected(hip):
    prune_cases.sabotage_case(hip)


def test_wide_level_of_250_siblings(hip):
    prune_cases.structure_case(hip, TINY, 2, 12, rank_cases.fanout_items(250), 65, "near", score_tol=5e-5, seed=3)


def test_items_of_unequal_length_and_a_padded_input_row(hip):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    prune_cases.structure_case(hip, TINY, 3, 14, items, 30, "near", seed=11)


def test_gated_gelu(hip):
    prune_cases.structure_case(hip, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), 30, "near", seed=11)


def test_one_user(hip):
    prune_cases.structure_case(hip, TINY, 1, 12, cases.make_items(40, 11, hi=60), 10, "near", seed=11)


def test_top_n_equal_to_the_item_count(hip):
    prune_cases.structure_case(hip, TINY, 3, 12, cases.make_items(40, 11, hi=60), 40, "exact", seed=11)


def test_exclusion(hip):
    prune_cases.exclusion_case(hip)


def test_declines_on_a_random_init_model(hip):
    prune_cases.declines_case(hip, TINY)


def test_deterministic_and_user_chunks(hip):
    prune_cases.determinism_case(hip)


def test_errors_and_no_effect_without_a_bf16_verified_model(hip):
    prune_cases.errors_case(hip, TINY)


def test_runner_exhaustive_2(hip, tmp_path):
    prune_cases.runner_case(hip, tmp_path)


def test_ml1m_shaped_catalogue_t5_small_declines(hip):
    """T5-small dims, the benchmark's 3416-item trie (5499 rows per user, about 9k edges), random init"""
    import bench
    prune_cases.large_trie_declines_case(hip, O.T5Cfg.named("t5-small"), bench.synth_item_trie(3416, 7))
