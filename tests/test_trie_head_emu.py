"""not-gpu: the item loss on a head restricted to the trie's tokens (`forward(trie=..., item_head="trie")`, csrc/p5_item_head.h) on the host
emulation of the kernels: the gather, the scatter and the compact cross-entropy kernels bit for bit against the source / the dense
kernels, the existing item-loss cases under `P5T5Native.item_head = "trie"`, and the restricted route against the dense one
(tests/trie_head_cases.py)."""
import os
import subprocess
import sys

import pytest

from oracle import t5_oracle as O
from openp5_amd.model import P5T5Native
from tests import trie_head_cases as th, trie_loss_cases as tl, trunc_cases as tc

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


@pytest.fixture
def trie_head(monkeypatch):
    monkeypatch.setattr(P5T5Native, "item_head", "trie")


# ---- op level ----
def test_gather_and_scatter(emu):
    th.gather_scatter_case(emu)


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_compact_cross_entropy_equals_dense(emu, tau):
    th.ce_case(emu, tau)


def test_compact_cross_entropy_one_position_per_sample(emu):
    th.ce_case(emu, 1.0, T=1)


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_compact_truncated_cross_entropy_equals_dense(emu, tau):
    th.trunc_ce_case(emu, tau)


def test_errors_of_the_abi_and_the_keyword(emu):
    th.abi_errors_case(emu, TINY)


def test_head_columns():
    th.head_columns_case()


# ---- the existing cases under the class attribute ----
@pytest.mark.parametrize("name", sorted(ITEMS))
def test_model_fp32(emu, trie_head, name):
    tl.model_case(emu, TINY, ITEMS[name])


def test_model_fp32_dropout(emu, trie_head):
    tl.model_case(emu, TINY, ITEMS["plain"], dropout=0.1)


def test_model_fp32_temperature(emu, trie_head):
    tl.model_case(emu, TINY, ITEMS["plain"], tau=0.7)


def test_model_fp32_excluded_items(emu, trie_head):
    tl.model_case(emu, TINY, ITEMS["plain"], excluded=True, tau=0.7)


@pytest.mark.parametrize("kw", [dict(), dict(tau=0.7, excluded=True)], ids=["plain", "tau_excluded"])
def test_model_bf16(emu, trie_head, kw):
    tl.model_case(emu, TINY, ITEMS["plain"], dtype="bf16", **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampler_logprobs_are_the_trainer_nll(emu, trie_head, dtype):
    tl.sampler_case(emu, TINY, ITEMS["plain"], 3, 14, 4, dtype=dtype, tau=0.7, excluded=True)


def test_sampler_logprobs_unequal_items(emu, trie_head):
    tl.sampler_case(emu, TINY, ITEMS["unequal"], 2, 12, 4, batch_seed=11, tag=" unequal")


def test_slate_logprobs_are_the_trainer_nll(emu, trie_head):
    tl.slates_case(emu, TINY, ITEMS["plain"])


def test_subset_normalisation_and_single_children(emu, trie_head):
    tl.subset_case(emu, TINY, ITEMS["plain"])


@pytest.mark.parametrize("dtype,dropout", [("fp32", 0.0), ("fp32", 0.1), ("bf16", 0.0)])
def test_loss_and_backward_equals_forward_and_autograd(emu, trie_head, dtype, dropout):
    tl.fused_case(emu, TINY, ITEMS["plain"], dtype=dtype, dropout=dropout)


def test_second_micro_batch_accumulates(emu, trie_head):
    tl.accumulation_case(emu, TINY, ITEMS["plain"])


def test_backward_is_bit_reproducible(emu, trie_head):
    tl.reproducible_case(emu, TINY, ITEMS["plain"])


def test_errors(emu, trie_head):
    tl.errors_case(emu, TINY)


def test_runner_under_the_class_attribute(emu, trie_head, tmp_path):
    tl.runner_case(emu, str(tmp_path))


def test_runner_item_loss_head_flag(emu, tmp_path):
    th.runner_case(emu, str(tmp_path))


@pytest.mark.parametrize("top_k,top_p,dropout,tau,excluded", [(2, 1.0, 0.0, 1.0, False), (0, 0.5, 0.0, 1.0, False), (3, 0.8, 0.1, 0.7, True)],
                         ids=["top_k", "top_p", "both_dropout_tau_excluded"])
def test_truncated_model(emu, trie_head, top_k, top_p, dropout, tau, excluded):
    tc.model_case(emu, TINY, ITEMS["plain"], top_k=top_k, top_p=top_p, dropout=dropout, tau=tau, excluded=excluded)


def test_truncated_loss_and_backward_equals_forward_and_autograd(emu, trie_head):
    tc.fused_case(emu, TINY, ITEMS["plain"])


def test_truncated_backward_is_bit_reproducible(emu, trie_head):
    tc.reproducible_case(emu, TINY, ITEMS["plain"])


# ---- route against route ----
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_restricted_route_against_dense(emu, dtype):
    th.routes_case(emu, TINY, ITEMS["plain"], dtype=dtype)


def test_restricted_route_against_dense_truncated(emu):
    th.routes_case(emu, TINY, ITEMS["plain"], dtype="fp32", temperature=0.7, top_p=0.995, tag=" truncated")


@pytest.mark.parametrize("staged", [False, True], ids=["whole", "staged"])
def test_grouped_storing_path(emu, staged):
    th.storing_case(emu, TINY, ITEMS["plain"], staged=staged)


def test_kernels_of_the_restricted_step(emu):
    th.profile_case(emu, TINY, ITEMS["plain"])


def test_item_head_workspace_bytes_are_exact(emu):
    th.workspace_case(emu, TINY, ITEMS["plain"])


def test_train_workspace_bytes_unchanged(emu, trie_head):
    tl.workspace_case(emu, TINY, ITEMS["plain"])


@pytest.mark.parametrize("env", [{"P5_EMU_POISON_LDS": "1"}, {"P5_EMU_FIBER_ORDER": "reverse"}, {"P5_EMU_BLOCK_ORDER": "reverse"}],
                         ids=["poison_lds", "fiber_reverse", "block_reverse"])
def test_kernels_under_adversarial_emulation(env):
    """the op-level cases and one model case under the emulator's adversarial modes, each in a fresh process (the modes are read once per
    process)"""
    sel = ("test_gather_and_scatter or test_compact_cross_entropy_equals_dense or test_compact_cross_entropy_one_position_per_sample or "
           "test_compact_truncated_cross_entropy_equals_dense or test_model_fp32_excluded_items")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", sel, "-p", "no:cacheprovider"],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
