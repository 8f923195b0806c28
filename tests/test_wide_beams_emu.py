"""Wide constrained beam search (65 .. 4096 beams, csrc/p5_decode_wide.h) on the host emulation of the kernels: oracle parity, equality
with the narrow step where both run, forced prefix, user chunking and the widened-beam filtered protocol of the runner."""
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases
from tests.wide_cases import gen_pair, narrow_vs_wide_case, runner_widened_case, tie_heavy_params, wide_leaves_case


def _set(be, name, value):
    be.check(be.lib.p5_set_option(name, value), "p5_set_option")


@pytest.mark.parametrize("K", [65, 80, 130])
def test_wide_oracle_parity(emu, K):
    cases.generate_case(emu, O.T5Cfg.named("tiny"), 2, 12, K, 12, 300)


def test_wide_oracle_parity_excluded(emu):
    cases.generate_excluded_case(emu, O.T5Cfg.named("tiny"), 2, 12, 80, 12, 300, frac=0.4)


def test_wide_fanout_beyond_2k(emu):
    """a trie level with 250 siblings > 2K = 130: the row-level radix select of the wide scoring kernel (dead -1e9 beams tie there)."""
    cases.generate_wide_fanout_case(emu, O.T5Cfg.named("tiny"), 2, 12, 65, 250)


def test_wide_fewer_items_than_beams(emu):
    """40 items, 65 beams: live candidates run out, dead beams (node -1) fill the rest as in the narrow step.  The real hypotheses are
    the oracle's; the narrow step at 64 beams and the wide step at 64 (gen_wide) return the same bits."""
    wide_leaves_case(emu, O.T5Cfg.named("tiny"), 2, 12, 65, 8, 40)
    narrow_vs_wide_case(emu, O.T5Cfg.named("tiny"), 2, 12, 64, 8, 40)


@pytest.mark.parametrize("K", [1, 10, 64])
def test_narrow_equals_wide(emu, K):
    narrow_vs_wide_case(emu, O.T5Cfg.named("tiny"), 2, 12, K, 12, 120)


def test_narrow_equals_wide_ties(emu):
    """identical embedding rows: many candidates with equal scores, ranked by the flat index (beam * max_c + child) on both paths."""
    narrow_vs_wide_case(emu, O.T5Cfg.named("tiny"), 2, 12, 10, 12, 120, params_fn=tie_heavy_params)


def test_wide_forced_prefix(emu):
    kw = dict(prefix=(0, 5, 6, 7, 8), seed=4)
    a = cases.generate_case(emu, O.T5Cfg.named("tiny"), 2, 12, 130, 14, 300, **kw)
    try:
        _set(emu, b"gen_ff", 0)
        b = cases.generate_case(emu, O.T5Cfg.named("tiny"), 2, 12, 130, 14, 300, **kw)
    finally:
        _set(emu, b"gen_ff", 1)
    assert torch.equal(a["sequences"].cpu(), b["sequences"].cpu())
    assert (a["sequences_scores"].cpu() - b["sequences_scores"].cpu()).abs().max() <= 2e-6


def test_wide_user_chunks_are_bit_identical(emu):
    whole, _ = gen_pair(emu, O.T5Cfg.named("tiny"), 3, 12, 70, 12, 200)
    chunked, m = gen_pair(emu, O.T5Cfg.named("tiny"), 3, 12, 70, 12, 200, wide_max_rows=70)
    assert m.wide_max_rows == 70
    assert torch.equal(whole["sequences"].cpu(), chunked["sequences"].cpu())
    assert torch.equal(whole["sequences_scores"].cpu(), chunked["sequences_scores"].cpu())


def test_wide_beam_limit(emu):
    m = cases.build_model(emu, O.T5Cfg.named("tiny"), O.init_params(O.T5Cfg.named("tiny"), 7), "fp32")
    ids = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="num_beams <= 4096"):
        m.generate(input_ids=ids, trie=_tiny_trie(), num_beams=4097)


def _tiny_trie():
    from openp5_amd.trie import CompiledTrie
    return CompiledTrie.from_sequences(cases.make_items(10, 1))


def test_runner_widened_beam_protocol_beyond_64(emu, tmp_path):
    """--test_filtered 1 --test_filtered_batch 1 with generate_num + longest history > 64 runs on the device, and its metrics equal the
    protocol restated literally (the oracle's beam search at that width, then evaluate.rel_results_filtered)."""
    for id_metrics in ("0", "1"):
        runner_widened_case(emu, tmp_path / id_metrics, id_metrics)
