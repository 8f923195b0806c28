"""not-gpu: exhaustive catalogue ranking (`P5T5Native.rank_items`, csrc/p5_rank.h) on the host emulation of the kernels, against the
oracle's score of every item (tests/rank_cases.py)."""
import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases
from tests.wide_cases import runner_widened_case, tie_heavy_params

TINY = O.T5Cfg.named("tiny")


def _items(n, **kw):
    return cases.make_items(n, 5, hi=min(60, TINY.vocab_size - 1), **kw)


@pytest.mark.parametrize("n_items", [40, 90])
def test_every_score_and_the_order_fp32(emu, n_items):
    """token-exact order: inputs (seed 11, L = 12) whose oracle scores are at least 1.07e-4 apart at both sizes (4 x tolerance = 8e-5)"""
    rank_cases.rank_case(emu, TINY, 3, 12, cases.make_items(n_items, 11, hi=60), top_n=n_items, seed=11)


def test_every_score_bf16_verified(emu):
    """a bf16 model in its default mode ranks with the fp32 verification engine: held to the fp32 tolerance"""
    rank_cases.rank_case(emu, TINY, 3, 20, _items(40), dtype="bf16", mode="verified", top_n=10)


def test_every_score_bf16_draft(emu):
    rank_cases.rank_case(emu, TINY, 3, 20, _items(40), dtype="bf16", mode="draft", score_tol=cases.BF16_SCORE_TOL, top_n=10, order=None)


def test_300_items_cross_the_512_query_limit(emu):
    """583 rows per user: two chunks of cross-attention queries; near-ties among 300 items judged by the tie rule"""
    out, m, _ = rank_cases.rank_case(emu, TINY, 2, 16, _items(300), top_n=300, order="ties")
    assert m.rank_stats["rows_per_user"] > 512


def test_wide_level_of_250_siblings(emu):
    rank_cases.rank_case(emu, TINY, 2, 12, rank_cases.fanout_items(250), score_tol=5e-5, top_n=65, order="near", seed=3)


def test_items_of_unequal_length_and_a_padded_input_row(emu):
    items = cases.make_items(30, 11, hi=min(60, TINY.vocab_size - 1), minlen=1, maxlen=6)
    assert len({len(q) for q in items}) >= 5
    ids, ww, mask, _, _ = cases.synth_batch(TINY, 3, 14, 4, 11)
    assert int(mask.sum(1).min()) < 14          # (a padded input row)
    rank_cases.rank_case(emu, TINY, 3, 14, items, top_n=30, order="ties", seed=11)


def test_gated_gelu(emu):
    rank_cases.rank_case(emu, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, cases.make_items(30, 11, hi=60), top_n=30, order="ties", seed=11)


@pytest.mark.parametrize("n_items", [40, 90])
def test_equals_the_widened_beam_protocol_in_its_limit(emu, n_items):
    rank_cases.protocol_link_case(emu, TINY, 3, 12, n_items, seed=11)


def test_exclusion(emu):
    rank_cases.exclusion_case(emu, TINY, 3, 20, 40, 10)


def test_deterministic_and_user_chunks(emu):
    rank_cases.determinism_case(emu, TINY, 3, 20, 40, 10)


def test_deterministic_with_ties(emu):
    ties, _ = rank_cases.determinism_case(emu, TINY, 2, 12, 40, 40, params_fn=tie_heavy_params)
    assert ties > 0


def test_range_guard_rescores_flagged_users(emu):
    rank_cases.range_guard_case(emu, TINY)


def test_errors_and_on_demand_indexing(emu):
    rank_cases.errors_case(emu, TINY)


@pytest.mark.parametrize("id_metrics", ["1", "0"])
@pytest.mark.parametrize("filtered_batch", ["1", "0"])
def test_runner_exhaustive_filtered(emu, tmp_path, id_metrics, filtered_batch):
    rank_cases.runner_exhaustive_case(emu, tmp_path / "x", id_metrics, True, filtered_batch)


@pytest.mark.parametrize("id_metrics", ["1", "0"])
def test_runner_exhaustive_unfiltered(emu, tmp_path, id_metrics):
    rank_cases.runner_exhaustive_case(emu, tmp_path / "x", id_metrics, False)


def test_runner_flag_off_never_ranks(emu, tmp_path, monkeypatch):
    from openp5_amd.model import P5T5Native

    def boom(*a, **kw):
        raise AssertionError("rank_items called without --test_exhaustive 1")
    monkeypatch.setattr(P5T5Native, "rank_items", boom)
    runner_widened_case(emu, tmp_path / "w", "1")
