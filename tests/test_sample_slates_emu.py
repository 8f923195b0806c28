"""not-gpu: stochastic beam search on the item trie (`P5T5Native.sample_slates`, csrc/p5_sbs.h) on the host emulation of the kernels,
against the float64 oracle, the restated uniforms and the exhaustive top-down reference of tests/sbs_cases.py."""
import os
import subprocess
import sys

import pytest

from oracle import t5_oracle as O
from tests import sbs_cases

TINY = O.T5Cfg.named("tiny")
EMU_FREQ_S = 40          # slates per user of the frequency test on the emulator: about 20 s (the GPU test draws 2048)


def test_replay_cases_are_mostly_separated():
    sbs_cases.separation_case()


def test_replay_fp32(emu):
    sbs_cases.replay_case(emu, "replay")


def test_structure_and_logprobs_bf16(emu):
    sbs_cases.replay_case(emu, "replay", dtype="bf16")


@pytest.mark.parametrize("name", [n for n in sbs_cases.REPLAY_CASES if n not in ("replay", "chain", "no_chain")])
def test_edges_of_the_dispatch(emu, name):
    """slate sizes, fan-outs (a row with more children than K selects), items of 1 - 6 tokens (finished beams carried), 5 items in a slate
    of 8 (empty slots), gated GELU, temperatures, exclusion (half / everything / nothing)"""
    out, _, _, _ = sbs_cases.replay_case(emu, name)
    if name == "five":
        assert bool((out["item_index"].cpu()[:, :, 5:] == -1).all()) and bool((out["item_index"].cpu()[:, :, :5] >= 0).all())
    if name == "exclusion":
        assert bool((out["item_index"].cpu()[1] == -1).all())


def test_forced_chain_and_fast_forward(emu):
    sbs_cases.forced_prefix_case(emu)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pure_function_properties(emu, dtype):
    sbs_cases.pure_function_case(emu, TINY, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_map_lanes(emu, dtype):
    sbs_cases.lanes_case(emu, TINY, 2, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frequencies(emu, dtype):
    sbs_cases.frequency_case(emu, TINY, EMU_FREQ_S, dtype=dtype)


def test_frequency_bound_is_not_vacuous():
    """A float64 Gumbel-top-K passes both laws on the frequency test's catalogue at both sizes and both temperatures.  A second position
    drawn WITH replacement does not fail clearly at temperature 1 (TINY's random weights give a nearly flat distribution over the 40
    items: 0 or 1 bin of about 35 outside the bound at S = 2048), and the peaked weights of tests/golden/make_peaked_tiny.py do not help
    (300 items, no item above a few percent: 0 of about 130 bins).  At temperature 0.5 the same model and catalogue put 0.88 / 0.49 on
    one item and the with-replacement sampler misses 14 of 26 / 3 of 19 bins: the GPU frequency test therefore runs at both temperatures."""
    for S in (EMU_FREQ_S, 2048):
        sbs_cases.frequency_bound_case(TINY, S)
    assert sbs_cases.frequency_bound_case(TINY, 2048, tau=0.5) == 2, "sampling with replacement passes the second law"


def test_workspace_bytes_are_exact_and_limits(emu):
    sbs_cases.workspace_case(emu, TINY)


def test_errors(emu):
    sbs_cases.errors_case(emu, TINY)


@pytest.mark.parametrize("env", [{"P5_EMU_POISON_LDS": "1"}, {"P5_EMU_FIBER_ORDER": "reverse"}, {"P5_EMU_BLOCK_ORDER": "reverse"}],
                         ids=["poison_lds", "fiber_reverse", "block_reverse"])
def test_slate_kernels_under_adversarial_emulation(env):
    """replay, fan-out 250 and carried finished beams under the emulator's adversarial modes, each in a fresh process (the modes are read
    once per process): no kernel may read LDS it has not written or depend on thread / workgroup order"""
    sel = "test_replay_fp32 or fan250 or unequal"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", sel, "-p", "no:cacheprovider"],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
