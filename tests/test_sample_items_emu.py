"""not-gpu: trie-constrained sampling (`P5T5Native.sample_items`, csrc/p5_sample.h) on the host emulation of the kernels, against the
float64 oracle and the restated uniforms (tests/sample_cases.py)."""
import os
import subprocess
import sys

import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases, sample_cases

TINY = O.T5Cfg.named("tiny")
EMU_FREQ_S = 80          # draws per user of the frequency test on the emulator: three seeds in about 20 s (the GPU test draws 2048)


def _items(n=40, **kw):
    return cases.make_items(n, 5, hi=60, **kw)


def test_uniforms_restatement():
    sample_cases.uniforms_range_case()


def test_replay_and_logprobs_fp32(emu):
    sample_cases.sample_case(emu, TINY, 3, 20, _items(), 8)


def test_replay_and_logprobs_bf16(emu):
    sample_cases.sample_case(emu, TINY, 3, 20, _items(), 8, dtype="bf16")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frequencies(emu, dtype):
    sample_cases.frequency_case(emu, TINY, EMU_FREQ_S, dtype=dtype)


def test_frequency_bound_is_not_vacuous():
    for S in (EMU_FREQ_S, 2048):
        sample_cases.bound_is_not_vacuous_case(TINY, S)


@pytest.mark.parametrize("S", [1, 16, 17, 64, 65])
def test_rows_per_user(emu, S):
    sample_cases.sample_case(emu, TINY, 2, 12, _items(), S, tag=f" S={S}")


def _fan(n):
    """one level of n siblings behind the shared prefix, short tails"""
    return [[0, 5, 6, 10 + i] + ([40 + (i % 7)] if i % 3 == 0 else []) + [1] for i in range(n)]


@pytest.mark.parametrize("fan", [1, 2, 32, 33])
def test_fan_out(emu, fan):
    sample_cases.sample_case(emu, TINY, 2, 12, _fan(fan), 6, tag=f" fan-out {fan}")


def test_fan_out_250(emu):
    sample_cases.sample_case(emu, TINY, 2, 12, rank_cases.fanout_items(250), 12, seed=2, tag=" fan-out 250")


def test_items_of_length_1_to_6_and_a_padded_input_row(emu):
    items = cases.make_items(30, 11, hi=60, minlen=1, maxlen=6)
    assert len({len(q) for q in items}) >= 5
    sample_cases.sample_case(emu, TINY, 3, 14, items, 8, batch_seed=11, tag=" unequal")


def test_gated_gelu(emu):
    sample_cases.sample_case(emu, O.T5Cfg.named("tiny", ff_act="gated-gelu"), 2, 12, _items(30), 6, tag=" gated")


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_temperature(emu, tau):
    sample_cases.sample_case(emu, TINY, 2, 12, _items(), 8, tau=tau)


@pytest.mark.parametrize("prefix", [(0, 5, 6), (0,)], ids=["forced_chain", "no_chain"])
def test_exclusion(emu, prefix):
    sample_cases.exclusion_case(emu, TINY, 8, prefix, S_freq=EMU_FREQ_S if prefix == (0,) else None)


def test_determinism_chunks_draw_ranges_and_streams(emu):
    sample_cases.determinism_case(emu, TINY)


def test_map_lanes(emu):
    sample_cases.lanes_case(emu, TINY, 2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forced_prefix_on_and_off(emu, dtype):
    sample_cases.forced_prefix_case(emu, TINY, dtype=dtype)


def test_generate_do_sample(emu):
    sample_cases.generate_case(emu, TINY)


def test_workspace_bytes_are_exact(emu):
    sample_cases.workspace_case(emu, TINY)


def test_errors_grafted_trie_and_on_demand_indexing(emu):
    sample_cases.errors_case(emu, TINY)


@pytest.mark.parametrize("env", [{"P5_EMU_POISON_LDS": "1"}, {"P5_EMU_FIBER_ORDER": "reverse"}, {"P5_EMU_BLOCK_ORDER": "reverse"}],
                         ids=["poison_lds", "fiber_reverse", "block_reverse"])
def test_sampling_kernels_under_adversarial_emulation(env):
    """replay, fan-out 250 and exclusion under the emulator's adversarial modes, each in a fresh process (the modes are read once per
    process): no kernel may read LDS it has not written or depend on thread / workgroup order"""
    sel = "test_replay_and_logprobs_fp32 or test_fan_out_250 or no_chain"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", sel, "-p", "no:cacheprovider"],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
