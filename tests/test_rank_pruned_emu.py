"""not-gpu: certified pruned ranking (`P5T5Native.rank_items(pruned=True)`, csrc/p5_prune.h) on the host emulation of the kernels, against
the oracle's score of every item (tests/prune_cases.py)."""
import pytest

from oracle import t5_oracle as O
from tests import cases, prune_cases, rank_cases

TINY = O.T5Cfg.named("tiny")


def test_certified_equals_the_oracle(emu):
    prune_cases.certified_case(emu)


def test_slack_never_changes_the_answer(emu):
    prune_cases.slack_case(emu)


def test_a_missing_prefix_is_detected(emu):
    prune_cases.sabotage_case(emu)


def test_wide_level_of_250_siblings(emu):
    prune_cases.structure_case(emu, TINY, 2, 12, rank_cases.fanout_items(250), 65, "near", score_tol=5e-5, seed=3)


def test_items_of_unequal_length_and_a_padded_input_row(emu):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    assert len({len(q) for q in items}) >= 5
    _, _, mask, _, _ = cases.synth_batch(TINY, 3, 14, 4, 11)
    assert int(mask.sum(1).min()) < 14          # (a padded input row)
    prune_cases.structure_case(emu, TINY, 3, 14, items, 30, "near", seed=11)


def test_gated_gelu(emu):
    prune_cases.structure_case(emu, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), 30, "near", seed=11)


def test_one_user(emu):
    prune_cases.structure_case(emu, TINY, 1, 12, cases.make_items(40, 11, hi=60), 10, "near", seed=11)


def test_top_n_equal_to_the_item_count(emu):
    """token-exact: the inputs of test_rank_items_emu.test_every_score_and_the_order_fp32, whose oracle scores are >= 1.07e-4 apart"""
    prune_cases.structure_case(emu, TINY, 3, 12, cases.make_items(40, 11, hi=60), 40, "exact", seed=11)


def test_exclusion(emu):
    prune_cases.exclusion_case(emu)


def test_declines_on_a_random_init_model(emu):
    prune_cases.declines_case(emu, TINY)


def test_deterministic_and_user_chunks(emu):
    prune_cases.determinism_case(emu)


def test_errors_and_no_effect_without_a_bf16_verified_model(emu):
    prune_cases.errors_case(emu, TINY)


def test_runner_exhaustive_2(emu, tmp_path):
    prune_cases.runner_case(emu, tmp_path)
