"""not-gpu: the trie-normalised training loss (`P5T5Native.forward(trie=...)`, csrc/p5_trie_ce.h) on the host emulation of the kernels: the
kernels one by one against float64, the model against the float64 oracle under autograd, the sampler's log-probabilities against the
trainer's NLL (tests/trie_loss_cases.py)."""
import os
import subprocess
import sys

import pytest

from oracle import t5_oracle as O
from tests import trie_loss_cases as tl

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_kernels_against_float64(emu, tau):
    tl.op_case(emu, tau)


def test_kernels_one_position_per_sample(emu):
    tl.op_case(emu, 1.0, T=1)


@pytest.mark.parametrize("name", sorted(ITEMS))
def test_model_fp32(emu, name):
    tl.model_case(emu, TINY, ITEMS[name])


def test_model_fp32_dropout(emu):
    tl.model_case(emu, TINY, ITEMS["plain"], dropout=0.1)


def test_model_fp32_temperature(emu):
    tl.model_case(emu, TINY, ITEMS["plain"], tau=0.7)


def test_model_fp32_excluded_items(emu):
    tl.model_case(emu, TINY, ITEMS["plain"], excluded=True, tau=0.7)


@pytest.mark.parametrize("kw", [dict(), dict(tau=0.7, excluded=True)], ids=["plain", "tau_excluded"])
def test_model_bf16(emu, kw):
    tl.model_case(emu, TINY, ITEMS["plain"], dtype="bf16", **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampler_logprobs_are_the_trainer_nll(emu, dtype):
    tl.sampler_case(emu, TINY, ITEMS["plain"], 3, 14, 4, dtype=dtype, tau=0.7, excluded=True)


def test_sampler_logprobs_unequal_items(emu):
    tl.sampler_case(emu, TINY, ITEMS["unequal"], 2, 12, 4, batch_seed=11, tag=" unequal")


def test_slate_logprobs_are_the_trainer_nll(emu):
    tl.slates_case(emu, TINY, ITEMS["plain"])


def test_subset_normalisation_and_single_children(emu):
    tl.subset_case(emu, TINY, ITEMS["plain"])


@pytest.mark.parametrize("dtype,dropout", [("fp32", 0.0), ("fp32", 0.1), ("bf16", 0.0)])
def test_loss_and_backward_equals_forward_and_autograd(emu, dtype, dropout):
    tl.fused_case(emu, TINY, ITEMS["plain"], dtype=dtype, dropout=dropout)


def test_second_micro_batch_accumulates(emu):
    tl.accumulation_case(emu, TINY, ITEMS["plain"])


def test_backward_is_bit_reproducible(emu):
    tl.reproducible_case(emu, TINY, ITEMS["plain"])


def test_plain_step_unchanged_around_an_item_loss_step(emu):
    tl.plain_route_restored_case(emu, TINY, ITEMS["plain"])


def test_train_workspace_bytes_are_exact(emu):
    tl.workspace_case(emu, TINY, ITEMS["plain"])


def test_errors(emu):
    tl.errors_case(emu, TINY)


def test_runner_trains_on_the_union_trie(emu, tmp_path):
    tl.runner_case(emu, str(tmp_path))


@pytest.mark.parametrize("env", [{"P5_EMU_POISON_LDS": "1"}, {"P5_EMU_FIBER_ORDER": "reverse"}, {"P5_EMU_BLOCK_ORDER": "reverse"}],
                         ids=["poison_lds", "fiber_reverse", "block_reverse"])
def test_kernels_under_adversarial_emulation(env):
    """the kernels one by one and the model under the emulator's adversarial modes, each in a fresh process (the modes are read once per
    process): no kernel may read LDS it has not written or depend on thread / workgroup order"""
    sel = "test_kernels_against_float64 or test_model_fp32_excluded_items"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", sel, "-p", "no:cacheprovider"],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
