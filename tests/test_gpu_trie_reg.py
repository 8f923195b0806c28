"""gpu: the regularised item loss -- per-row entropy and KL to a frozen reference policy (csrc/p5_trie_reg.h) -- on the MI355X: the cases of
tests/test_trie_reg_emu.py (tests/trie_reg_cases.py)."""
import pytest

from oracle import t5_oracle as O
from tests import trie_loss_cases as tl
from tests import trie_reg_cases as tr
from tests.test_trie_reg_emu import MODEL_VARIANTS

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "child_col"])
@pytest.mark.parametrize("tau", tr.OP_TAUS)
def test_kernels_against_float64(hip, tau, compact):
    assert tr.op_case(hip, tau, compact=compact) <= 1.0


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "child_col"])
def test_kernels_one_position_per_sample(hip, compact):
    tr.op_case(hip, 1.0, T=1, compact=compact)


def test_reference_equal_to_the_policy_gives_zero_kl(hip):
    tr.self_reference_case(hip)


def test_uniform_logits_give_log_n(hip):
    tr.uniform_case(hip)


@pytest.mark.parametrize("name", sorted(MODEL_VARIANTS))
def test_model_fp32(hip, name):
    tr.model_case(hip, TINY, ITEMS["plain"], **MODEL_VARIANTS[name])


@pytest.mark.parametrize("name", ["fan33", "unequal"])
def test_model_fp32_item_sets(hip, name):
    tr.model_case(hip, TINY, ITEMS[name])


@pytest.mark.parametrize("kw", [dict(), dict(tau=0.7, excluded=True, item_head="trie")], ids=["plain", "tau_excluded_trie_head"])
def test_model_bf16(hip, kw):
    tr.model_case(hip, TINY, ITEMS["plain"], dtype="bf16", **kw)


@pytest.mark.parametrize("dtype,dropout,head", [("fp32", 0.0, "dense"), ("fp32", 0.1, "trie"), ("bf16", 0.0, "dense"), ("bf16", 0.1, "trie")])
def test_loss_and_backward_equals_forward_and_autograd(hip, dtype, dropout, head):
    tr.fused_case(hip, TINY, ITEMS["plain"], dtype=dtype, dropout=dropout, item_head=head)


def test_loss_and_backward_staged(hip):
    tr.fused_case(hip, TINY, ITEMS["plain"], staged=True)


@pytest.mark.parametrize("dtype,head", [("fp32", "dense"), ("bf16", "trie")])
def test_target_weights_do_not_weight_the_regularisers(hip, dtype, head):
    tr.fused_targets_case(hip, TINY, ITEMS["plain"], dtype=dtype, item_head=head)


def test_second_micro_batch_accumulates(hip):
    tr.accumulation_case(hip, TINY, ITEMS["plain"])


def test_item_logits(hip):
    tr.item_logits_case(hip, TINY, ITEMS["plain"])


def test_plain_item_loss_unchanged_around_a_regularised_step(hip):
    tr.unchanged_case(hip, TINY, ITEMS["plain"])


def test_errors(hip):
    tr.errors_case(hip, TINY)


def test_train_workspace_bytes_are_exact(hip):
    tr.workspace_case(hip, TINY, ITEMS["plain"])


def test_runner_regularised_item_loss(hip, tmp_path):
    tr.runner_case(hip, str(tmp_path))
