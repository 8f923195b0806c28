"""Wide constrained beam search (65 .. 4096 beams, csrc/p5_decode_wide.h) on the MI355X."""
import pytest
import torch

from oracle import t5_oracle as O
from tests import cases
from tests.wide_cases import check_leaves, gen_pair, narrow_vs_wide_case, oracle_case, tie_heavy_params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [65, 80, 130, 256, 1024])
def test_gpu_wide_oracle_parity(hip, K):
    oracle_case(hip, O.T5Cfg.named("tiny"), 2, 12, K, 12, max(300, 2 * K))


def test_gpu_wide_oracle_parity_excluded(hip):
    cases.generate_excluded_case(hip, O.T5Cfg.named("tiny"), 2, 12, 80, 12, 300, frac=0.4)


def test_gpu_wide_fanout_beyond_2k(hip):
    cases.generate_wide_fanout_case(hip, O.T5Cfg.named("tiny"), 2, 12, 65, 250)


def test_gpu_wide_fewer_items_than_beams(hip):
    out, _ = gen_pair(hip, O.T5Cfg.named("tiny"), 2, 12, 130, 8, 40)
    check_leaves(out["sequences"], out["sequences_scores"], 130, out["items"])


@pytest.mark.parametrize("K", [1, 10, 64])
def test_gpu_narrow_equals_wide(hip, K):
    narrow_vs_wide_case(hip, O.T5Cfg.named("tiny"), 2, 12, K, 12, 120)


def test_gpu_narrow_equals_wide_ties(hip):
    narrow_vs_wide_case(hip, O.T5Cfg.named("tiny"), 2, 12, 10, 12, 120, params_fn=tie_heavy_params)


def test_gpu_narrow_equals_wide_t5_small_bf16(hip):
    """bf16 T5-small dims: the streaming head's scoring kernel on both paths (plain bf16 search)."""
    cfg = O.T5Cfg.named("t5-small")
    params = O.init_params(cfg, 7)
    m = cases.build_model(hip, cfg, params, "bf16")
    m.generation_mode = "draft"
    a, _ = gen_pair(hip, cfg, 2, 24, 20, 12, 300, model=m)
    hip.check(hip.lib.p5_set_option(b"gen_wide", 1), "p5_set_option")
    try:
        b, _ = gen_pair(hip, cfg, 2, 24, 20, 12, 300, model=m)
    finally:
        hip.lib.p5_set_option(b"gen_wide", 0)
    assert torch.equal(a["sequences"].cpu(), b["sequences"].cpu())
    assert torch.equal(a["sequences_scores"].cpu(), b["sequences_scores"].cpu())


def test_gpu_wide_forced_prefix(hip):
    kw = dict(prefix=(0, 5, 6, 7, 8), seed=4)
    a = cases.generate_case(hip, O.T5Cfg.named("tiny"), 2, 12, 130, 14, 300, **kw)
    try:
        hip.check(hip.lib.p5_set_option(b"gen_ff", 0), "p5_set_option")
        b = cases.generate_case(hip, O.T5Cfg.named("tiny"), 2, 12, 130, 14, 300, **kw)
    finally:
        hip.lib.p5_set_option(b"gen_ff", 1)
    assert torch.equal(a["sequences"].cpu(), b["sequences"].cpu())
    assert (a["sequences_scores"].cpu() - b["sequences_scores"].cpu()).abs().max() <= 2e-6


def test_gpu_wide_user_chunks_are_bit_identical(hip):
    whole, _ = gen_pair(hip, O.T5Cfg.named("tiny"), 4, 12, 300, 12, 600)
    chunked, _ = gen_pair(hip, O.T5Cfg.named("tiny"), 4, 12, 300, 12, 600, wide_max_rows=600)
    assert torch.equal(whole["sequences"].cpu(), chunked["sequences"].cpu())
    assert torch.equal(whole["sequences_scores"].cpu(), chunked["sequences_scores"].cpu())


def test_gpu_wide_ml1m_width(hip):
    """K = 2354 (an ML-1M-shaped width: generate_num + longest history), B = 2, tiny dims: the oracle's lists -- token-exact except where
    two hypotheses' oracle scores are within cases.FP32_TIE_TOL (fp32 device vs fp32 CPU arithmetic; at 2354 ranked items per user near-ties
    are dense), scores within 2e-5; the K finished hypotheses are sorted, complete trie items and distinct."""
    K = 2354
    out = oracle_case(hip, O.T5Cfg.named("tiny"), 2, 12, K, 12, 6000, tie_tol=cases.FP32_TIE_TOL)
    check_leaves(out["sequences"], out["sequences_scores"], K, out["items"])
    assert bool((out["sequences_scores"] > -1e8).all())          # 6000 items: every beam holds a real hypothesis


def test_gpu_wide_bf16_draft(hip):
    """the plain bf16 search at K = 256: ranked-set agreement with the fp32 oracle under the bf16 generation tests' tie tolerance."""
    oracle_case(hip, O.T5Cfg.named("tiny"), 2, 12, 256, 12, 600, score_tol=0.05, dtype="bf16", mode="draft", tie_tol=0.05)
