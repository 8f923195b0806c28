"""not-gpu: the regularised item loss -- per-row entropy and KL to a frozen reference policy (`forward(trie=..., item_entropy=, ref_logits=)`,
`loss_and_backward(entropy_coef=, kl_coef=, ref_logits=)`, `item_logits`, csrc/p5_trie_reg.h) -- on the host emulation of the kernels: the
kernels one by one against float64, the identities, the model against the float64 oracle under autograd, the fused step against autograd
(tests/trie_reg_cases.py)."""
import pytest

from oracle import t5_oracle as O
from tests import trie_loss_cases as tl
from tests import trie_reg_cases as tr

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "child_col"])
@pytest.mark.parametrize("tau", tr.OP_TAUS)
def test_kernels_against_float64(emu, tau, compact):
    assert tr.op_case(emu, tau, compact=compact) <= 1.0


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "child_col"])
def test_kernels_one_position_per_sample(emu, compact):
    tr.op_case(emu, 1.0, T=1, compact=compact)


def test_reference_equal_to_the_policy_gives_zero_kl(emu):
    tr.self_reference_case(emu)


def test_uniform_logits_give_log_n(emu):
    tr.uniform_case(emu)


MODEL_VARIANTS = {"plain": dict(), "tau_excluded": dict(tau=0.7, excluded=True), "dropout": dict(dropout=0.1), "trie_head": dict(item_head="trie"),
                  "entropy_only": dict(kl=False), "kl_only": dict(entropy=False)}


@pytest.mark.parametrize("name", sorted(MODEL_VARIANTS))
def test_model_fp32(emu, name):
    tr.model_case(emu, TINY, ITEMS["plain"], **MODEL_VARIANTS[name])


@pytest.mark.parametrize("name", ["fan33", "unequal"])
def test_model_fp32_item_sets(emu, name):
    tr.model_case(emu, TINY, ITEMS[name])


@pytest.mark.parametrize("kw", [dict(), dict(tau=0.7, excluded=True, item_head="trie")], ids=["plain", "tau_excluded_trie_head"])
def test_model_bf16(emu, kw):
    tr.model_case(emu, TINY, ITEMS["plain"], dtype="bf16", **kw)


@pytest.mark.parametrize("dtype,dropout,head", [("fp32", 0.0, "dense"), ("fp32", 0.1, "trie"), ("bf16", 0.0, "dense"), ("bf16", 0.1, "trie")])
def test_loss_and_backward_equals_forward_and_autograd(emu, dtype, dropout, head):
    tr.fused_case(emu, TINY, ITEMS["plain"], dtype=dtype, dropout=dropout, item_head=head)


def test_loss_and_backward_staged(emu):
    tr.fused_case(emu, TINY, ITEMS["plain"], staged=True)


@pytest.mark.parametrize("dtype,head", [("fp32", "dense"), ("bf16", "trie")])
def test_target_weights_do_not_weight_the_regularisers(emu, dtype, head):
    tr.fused_targets_case(emu, TINY, ITEMS["plain"], dtype=dtype, item_head=head)


def test_second_micro_batch_accumulates(emu):
    tr.accumulation_case(emu, TINY, ITEMS["plain"])


def test_item_logits(emu):
    tr.item_logits_case(emu, TINY, ITEMS["plain"])


def test_plain_item_loss_unchanged_around_a_regularised_step(emu):
    tr.unchanged_case(emu, TINY, ITEMS["plain"])


def test_errors(emu):
    tr.errors_case(emu, TINY)


def test_train_workspace_bytes_are_exact(emu):
    tr.workspace_case(emu, TINY, ITEMS["plain"])


def test_runner_regularised_item_loss(emu, tmp_path):
    tr.runner_case(emu, str(tmp_path))
