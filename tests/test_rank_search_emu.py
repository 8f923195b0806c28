"""not-gpu: bounded trie search (`P5T5Native.rank_items(pruned="search")`, csrc/p5_bound.h) on the host emulation of the kernels, against
the oracle's score of every item (tests/search_cases.py)."""
import os
import subprocess
import sys

import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases, search_cases

TINY = O.T5Cfg.named("tiny")


def test_certified_equals_the_oracle(emu):
    search_cases.certified_case(emu, "bf16")


def test_certified_equals_the_oracle_fp32_model(emu):
    search_cases.certified_case(emu, "fp32")


def test_given_seeds_bound_the_cost(emu):
    search_cases.seeds_bound_cost_case(emu)


def test_seeds_change_cost_never_a_list(emu):
    search_cases.seeds_never_change_a_list_case(emu)


def test_invariants_of_every_round(emu):
    search_cases.invariants_case(emu)


def test_a_removed_prefix_is_healed_or_flagged(emu):
    search_cases.removed_prefix_case(emu)


def test_wide_level_of_250_siblings(emu):
    search_cases.structure_case(emu, TINY, 2, 12, rank_cases.fanout_items(250), 65, "near", score_tol=5e-5, seed=3)


def test_items_of_unequal_length_and_a_padded_input_row(emu):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    assert len({len(q) for q in items}) >= 5
    _, _, mask, _, _ = cases.synth_batch(TINY, 3, 14, 4, 11)
    assert int(mask.sum(1).min()) < 14          # (a padded input row)
    search_cases.structure_case(emu, TINY, 3, 14, items, 30, "near", seed=11)


def test_gated_gelu(emu):
    search_cases.structure_case(emu, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), 30, "near", seed=11)


def test_one_user(emu):
    search_cases.structure_case(emu, TINY, 1, 12, cases.make_items(40, 11, hi=60), 10, "near", seed=11)


def test_top_n_equal_to_the_item_count(emu):
    """token-exact: the inputs of test_rank_items_emu.test_every_score_and_the_order_fp32, whose oracle scores are >= 1.07e-4 apart"""
    search_cases.structure_case(emu, TINY, 3, 12, cases.make_items(40, 11, hi=60), 40, "exact", seed=11)


def test_exclusion(emu):
    search_cases.exclusion_case(emu)


def test_declines_on_a_random_init_model(emu):
    search_cases.declines_case(emu, TINY)


def test_deterministic_and_user_chunks(emu):
    search_cases.determinism_case(emu)


def test_errors_and_no_effect_in_draft_mode(emu):
    search_cases.errors_case(emu, TINY)


def test_runner_exhaustive_3(emu, tmp_path):
    search_cases.runner_case(emu, tmp_path)


@pytest.mark.parametrize("env", [{"P5_EMU_POISON_LDS": "1"}, {"P5_EMU_FIBER_ORDER": "reverse"}, {"P5_EMU_BLOCK_ORDER": "reverse"}],
                         ids=["poison_lds", "fiber_reverse", "block_reverse"])
def test_search_kernels_under_adversarial_emulation(env):
    """case 3 (given seeds: the seed, union and expand kernels, a row count pinned between two oracle counts) under the emulator's
    adversarial modes, each in a fresh process (the modes are read once per process): sel may not depend on thread or workgroup order,
    and no kernel may read LDS it has not written"""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_given_seeds_bound_the_cost", "-p", "no:cacheprovider"],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
