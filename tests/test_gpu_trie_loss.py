"""gpu: the trie-normalised training loss (`P5T5Native.forward(trie=...)`, csrc/p5_trie_ce.h) on the MI355X: the cases of
tests/test_trie_loss_emu.py (tests/trie_loss_cases.py), plus the sampler's log-probabilities against the trainer's NLL at T5-small width
on the benchmark's catalogue."""
import pytest

from oracle import t5_oracle as O
from tests import trie_loss_cases as tl

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_kernels_against_float64(hip, tau):
    tl.op_case(hip, tau)


def test_kernels_one_position_per_sample(hip):
    tl.op_case(hip, 1.0, T=1)


@pytest.mark.parametrize("name", sorted(ITEMS))
def test_model_fp32(hip, name):
    tl.model_case(hip, TINY, ITEMS[name])


def test_model_fp32_dropout(hip):
    tl.model_case(hip, TINY, ITEMS["plain"], dropout=0.1)


def test_model_fp32_temperature(hip):
    tl.model_case(hip, TINY, ITEMS["plain"], tau=0.7)


def test_model_fp32_excluded_items(hip):
    tl.model_case(hip, TINY, ITEMS["plain"], excluded=True, tau=0.7)


@pytest.mark.parametrize("kw", [dict(), dict(tau=0.7, excluded=True)], ids=["plain", "tau_excluded"])
def test_model_bf16(hip, kw):
    tl.model_case(hip, TINY, ITEMS["plain"], dtype="bf16", **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampler_logprobs_are_the_trainer_nll(hip, dtype):
    tl.sampler_case(hip, TINY, ITEMS["plain"], 3, 14, 4, dtype=dtype, tau=0.7, excluded=True)


def test_sampler_logprobs_unequal_items(hip):
    tl.sampler_case(hip, TINY, ITEMS["unequal"], 2, 12, 4, batch_seed=11, tag=" unequal")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampler_logprobs_ml1m_shaped_catalogue_t5_small(hip, dtype):
    """T5-small dims (d = 512, V = 32100), the benchmark's 3,416-item trie, B = 2, S = 2, L = 32"""
    import bench
    from openp5_amd.trie import CompiledTrie
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    items = ct.enumerate_items()
    ct.index_items(items)
    tl.sampler_case(hip, O.T5Cfg.named("t5-small"), items, 2, 32, 2, dtype=dtype, ct=ct, tag=" ml1m")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_slate_logprobs_are_the_trainer_nll(hip, dtype):
    tl.slates_case(hip, TINY, ITEMS["plain"], dtype=dtype)


def test_subset_normalisation_and_single_children(hip):
    tl.subset_case(hip, TINY, ITEMS["plain"])


@pytest.mark.parametrize("dtype,dropout", [("fp32", 0.0), ("fp32", 0.1), ("bf16", 0.0)])
def test_loss_and_backward_equals_forward_and_autograd(hip, dtype, dropout):
    tl.fused_case(hip, TINY, ITEMS["plain"], dtype=dtype, dropout=dropout)


def test_second_micro_batch_accumulates(hip):
    tl.accumulation_case(hip, TINY, ITEMS["plain"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_is_bit_reproducible(hip, dtype):
    tl.reproducible_case(hip, TINY, ITEMS["plain"], dtype=dtype)


def test_plain_step_unchanged_around_an_item_loss_step(hip):
    tl.plain_route_restored_case(hip, TINY, ITEMS["plain"])


def test_train_workspace_bytes_are_exact(hip):
    tl.workspace_case(hip, TINY, ITEMS["plain"])


def test_errors(hip):
    tl.errors_case(hip, TINY)
