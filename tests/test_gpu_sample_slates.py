"""gpu: stochastic beam search on the item trie (`P5T5Native.sample_slates`, csrc/p5_sbs.h) on the MI355X against the float64 oracle, the
restated uniforms and the exhaustive top-down reference of tests/sbs_cases.py, at toy sizes and at T5-small width on the benchmark's
catalogue."""
import pytest

from oracle import t5_oracle as O
from tests import sbs_cases

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")


def test_replay_fp32(hip):
    sbs_cases.replay_case(hip, "replay")


def test_structure_and_logprobs_bf16(hip):
    sbs_cases.replay_case(hip, "replay", dtype="bf16")


@pytest.mark.parametrize("name", [n for n in sbs_cases.REPLAY_CASES if n not in ("replay", "chain", "no_chain")])
def test_edges_of_the_dispatch(hip, name):
    """slate sizes, fan-outs (a row with more children than K selects), items of 1 - 6 tokens (finished beams carried), 5 items in a slate
    of 8 (empty slots), gated GELU, temperatures, exclusion (half / everything / nothing)"""
    out, _, _, _ = sbs_cases.replay_case(hip, name)
    if name == "five":
        assert bool((out["item_index"].cpu()[:, :, 5:] == -1).all()) and bool((out["item_index"].cpu()[:, :, :5] >= 0).all())
    if name == "exclusion":
        assert bool((out["item_index"].cpu()[1] == -1).all())


def test_forced_chain_and_fast_forward(hip):
    sbs_cases.forced_prefix_case(hip)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ml1m_shaped_catalogue_t5_small(hip, dtype):
    """T5-small dims (d = 512, V = 32100), the benchmark's 3,416-item trie, B = 2, S = 2, K = 10.  The float64 pass over 3,416 items per
    user is too slow for a test: only the returned items' perturbed values and log-probabilities are compared (no order comparison)."""
    import bench
    from openp5_amd.trie import CompiledTrie
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    items = ct.enumerate_items()
    ct.index_items(items)
    sbs_cases.slate_case(hip, O.T5Cfg.named("t5-small"), 2, 32, items, 10, S=2, dtype=dtype, ct=ct, tag=" ml1m", full=False)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pure_function_properties(hip, dtype):
    sbs_cases.pure_function_case(hip, TINY, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("lanes", [2, 3])
def test_lanes_match_one_at_a_time(hip, lanes, dtype):
    sbs_cases.lanes_case(hip, TINY, lanes, dtype)


@pytest.mark.parametrize("dtype,tau", [("fp32", 1.0), ("fp32", 0.5), ("bf16", 1.0)])
def test_frequencies(hip, dtype, tau):
    """2048 slates of 3: position 0 against p, position 1 against the without-replacement law, with and without half the catalogue
    excluded.  At temperature 0.5 the distribution is peaked enough for the second law to tell sampling with replacement from without
    (tests/test_sample_slates_emu.py::test_frequency_bound_is_not_vacuous)."""
    sbs_cases.frequency_case(hip, TINY, 2048, dtype=dtype, tau=tau)


def test_workspace_bytes_are_exact_and_limits(hip):
    sbs_cases.workspace_case(hip, TINY)


def test_errors(hip):
    sbs_cases.errors_case(hip, TINY)
