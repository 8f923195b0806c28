"""not-gpu: per-user candidate scoring (`P5T5Native.score_candidates`, csrc/p5_cand.h) on the host emulation of the kernels, against
the oracle's score of every candidate (tests/cand_cases.py)."""
import os
import subprocess
import sys

import pytest

from oracle import t5_oracle as O
from tests import cand_cases, cases, rank_cases
from tests.wide_cases import runner_widened_case, tie_heavy_params

TINY = O.T5Cfg.named("tiny")


def _items(n, **kw):
    return cases.make_items(n, 5, hi=min(60, TINY.vocab_size - 1), **kw)


def _halves(n, B, seed):
    return cand_cases.seeded_lists(n, [n // 2] * B, seed)


@pytest.mark.parametrize("n_items", [40, 90])
def test_every_score_and_the_order_fp32(emu, n_items):
    """token-exact order: inputs (seed 11, L = 12) whose oracle scores are at least 1.07e-4 apart between ANY two items of a user"""
    cand_cases.every_score_case(emu, TINY, n_items)


def test_ragged_lists_and_empty_slots(emu):
    cand_cases.ragged_case(emu, TINY)


def test_every_score_bf16_verified(emu):
    """a bf16 model in its default mode scores with the fp32 verification engine: held to the fp32 tolerance"""
    cand_cases.cand_case(emu, TINY, 3, 20, _items(40), _halves(40, 3, 51), dtype="bf16", mode="verified", top_n=10, order="near")


def test_every_score_bf16_draft(emu):
    cand_cases.cand_case(emu, TINY, 3, 20, _items(40), _halves(40, 3, 51), dtype="bf16", mode="draft", score_tol=cases.BF16_SCORE_TOL, top_n=10, order=None)


def test_300_candidates_cross_the_512_query_limit(emu):
    cand_cases.over_512_rows_case(emu, TINY)


def test_wide_level_of_250_siblings(emu):
    cand_cases.cand_case(emu, TINY, 2, 12, rank_cases.fanout_items(250), _halves(250, 2, 52), score_tol=5e-5, top_n=65, order="near", seed=3, tag=" fanout")


def test_items_of_unequal_length_and_a_padded_input_row(emu):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    assert len({len(q) for q in items}) >= 5
    cand_cases.cand_case(emu, TINY, 3, 14, items, _halves(30, 3, 53), order="near", seed=11, tag=" unequal")


def test_gated_gelu(emu):
    cand_cases.cand_case(emu, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), _halves(30, 2, 54), order="near", seed=11,
                         tag=" gated")


def test_agrees_with_rank_items(emu):
    cand_cases.rank_items_agreement_case(emu, TINY, 3, 12, cases.make_items(90, 11, hi=60), cand_cases.seeded_lists(90, [30, 12, 45], 55), seed=11)


def test_deterministic_and_user_chunks(emu):
    cand_cases.determinism_case(emu, TINY, 3, 20, 40, [20, 20, 9])


def test_deterministic_with_ties(emu):
    ties, _ = cand_cases.determinism_case(emu, TINY, 2, 12, 40, [40, 25], params_fn=tie_heavy_params)
    assert ties > 0


def test_permuting_a_list_permutes_its_scores(emu):
    cand_cases.permutation_case(emu, TINY)


def test_range_guard_rescores_flagged_users(emu):
    cand_cases.range_guard_case(emu, TINY)


def test_errors_and_on_demand_indexing(emu):
    cand_cases.errors_case(emu, TINY)


def test_workspace_does_not_grow_with_the_catalogue(emu):
    cand_cases.workspace_case(emu)


@pytest.mark.parametrize("id_metrics", ["1", "0"])
def test_runner_sampled_candidates(emu, tmp_path, id_metrics):
    cand_cases.runner_candidates_case(emu, tmp_path / "c", id_metrics)


def test_runner_flag_off_never_scores_candidates(emu, tmp_path, monkeypatch):
    from openp5_amd.model import P5T5Native

    def boom(*a, **kw):
        raise AssertionError("score_candidates called without --test_candidates")
    monkeypatch.setattr(P5T5Native, "score_candidates", boom)
    runner_widened_case(emu, tmp_path / "w", "1")


def test_runner_candidates_with_exhaustive_is_refused_at_construction(emu, tmp_path):
    cand_cases.runner_flag_errors_case(emu, tmp_path / "e")


def test_runner_candidates_take_precedence_over_filtered(emu, tmp_path, caplog):
    cand_cases.runner_filtered_precedence_case(emu, tmp_path / "f", caplog)


@pytest.mark.parametrize("env", [{"P5_EMU_POISON_LDS": "1"}, {"P5_EMU_FIBER_ORDER": "reverse"}, {"P5_EMU_BLOCK_ORDER": "reverse"}],
                         ids=["poison_lds", "fiber_reverse", "block_reverse"])
def test_candidate_kernels_under_adversarial_emulation(env):
    """cases 1, 4 and 7 under the emulator's adversarial modes, each in a fresh process (the modes are read once per process): the plan
    may not depend on thread or workgroup order, and no kernel may read LDS it has not written"""
    sel = "test_every_score_and_the_order_fp32 or test_300_candidates or test_deterministic"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", sel, "-p", "no:cacheprovider"],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
