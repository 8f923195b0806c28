"""gpu: trie-constrained sampling (`P5T5Native.sample_items`, csrc/p5_sample.h) on the MI355X against the float64 oracle and the restated
uniforms (tests/sample_cases.py), at toy sizes, at T5-small width on the benchmark's catalogue and at T5-base width."""
import random

import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases, sample_cases

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")


def _items(n=40, **kw):
    return cases.make_items(n, 5, hi=60, **kw)


def test_replay_and_logprobs_fp32(hip):
    sample_cases.sample_case(hip, TINY, 3, 20, _items(), 8)


def test_replay_and_logprobs_bf16(hip):
    sample_cases.sample_case(hip, TINY, 3, 20, _items(), 8, dtype="bf16")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frequencies(hip, dtype):
    sample_cases.frequency_case(hip, TINY, 2048, dtype=dtype)


@pytest.mark.parametrize("S", [1, 16, 17, 64, 65])
def test_rows_per_user(hip, S):
    sample_cases.sample_case(hip, TINY, 2, 12, _items(), S, tag=f" S={S}")


def _fan(n):
    return [[0, 5, 6, 10 + i] + ([40 + (i % 7)] if i % 3 == 0 else []) + [1] for i in range(n)]


@pytest.mark.parametrize("fan", [1, 2, 32, 33])
def test_fan_out(hip, fan):
    sample_cases.sample_case(hip, TINY, 2, 12, _fan(fan), 6, tag=f" fan-out {fan}")


def test_fan_out_250(hip):
    sample_cases.sample_case(hip, TINY, 2, 12, rank_cases.fanout_items(250), 12, seed=2, tag=" fan-out 250")


def test_items_of_length_1_to_6_and_a_padded_input_row(hip):
    sample_cases.sample_case(hip, TINY, 3, 14, cases.make_items(30, 11, hi=60, minlen=1, maxlen=6), 8, batch_seed=11, tag=" unequal")


def test_gated_gelu(hip):
    sample_cases.sample_case(hip, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, _items(30), 6, tag=" gated")


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_temperature(hip, tau):
    sample_cases.sample_case(hip, TINY, 2, 12, _items(), 8, tau=tau)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ml1m_shaped_catalogue_t5_small(hip, dtype):
    """T5-small dims (d = 512, V = 32100), the benchmark's 3,416-item trie, B = 2, S = 10"""
    import bench
    from openp5_amd.trie import CompiledTrie
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    items = ct.enumerate_items()
    ct.index_items(items)
    sample_cases.sample_case(hip, O.T5Cfg.named("t5-small"), 2, 32, items, 10, dtype=dtype, ct=ct, tag=" ml1m")


def test_collab_dims_t5_base_width(hip):
    """T5-base width (2 + 2 layers, the vocabulary of collaborative indexing), the config and items of the score_candidates test"""
    ocfg = O.T5Cfg.named("t5-base", num_layers=2, num_decoder_layers=2, vocab_size=32600)
    rnd = random.Random(3)
    items = set()
    while len(items) < 120:
        items.add(tuple([0, 5] + [rnd.randint(32100, 32599) for _ in range(rnd.randint(2, 4))] + [1]))
    sample_cases.sample_case(hip, ocfg, 2, 40, sorted(list(x) for x in items), 10, dtype="bf16", tag=" collab")


@pytest.mark.parametrize("prefix", [(0, 5, 6), (0,)], ids=["forced_chain", "no_chain"])
def test_exclusion(hip, prefix):
    sample_cases.exclusion_case(hip, TINY, 8, prefix, S_freq=2048 if prefix == (0,) else None)


def test_determinism_chunks_draw_ranges_and_streams(hip):
    sample_cases.determinism_case(hip, TINY)


@pytest.mark.parametrize("lanes", [2, 3])
def test_lanes_match_one_at_a_time(hip, lanes):
    sample_cases.lanes_case(hip, TINY, lanes)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forced_prefix_on_and_off(hip, dtype):
    sample_cases.forced_prefix_case(hip, TINY, dtype=dtype)


def test_generate_do_sample(hip):
    sample_cases.generate_case(hip, TINY)


def test_workspace_bytes_are_exact(hip):
    sample_cases.workspace_case(hip, TINY)


def test_errors_grafted_trie_and_on_demand_indexing(hip):
    sample_cases.errors_case(hip, TINY)
