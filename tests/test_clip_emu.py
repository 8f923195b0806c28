"""not-gpu: the clipped-ratio policy objective (csrc/p5_clip.h, loss_and_backward(old_logprobs=, clip_eps=), policy_collect / policy_update)
on the host emulation of the kernels: the cases of tests/clip_cases.py."""
import pytest

from oracle import t5_oracle as O
from tests import clip_cases as cc
from tests import trie_loss_cases as tl

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


# ---- 1. the kernels against the float64 restatement
@pytest.mark.parametrize("eps", cc.KERNEL_EPS, ids=lambda e: f"eps{e[0]}-{e[1]}")
@pytest.mark.parametrize("ratio", ["token", "sequence"])
@pytest.mark.parametrize("shape", cc.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_fp64(emu, shape, ratio, eps):
    cc.kernel_case(emu, *shape, ratio, eps)


# ---- 2. rho == 1 is the plain step, bit for bit
@pytest.mark.parametrize("G", [None, 3])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("route", ["ce", "item_dense", "item_trie", "reg"])
def test_unit_ratio_is_the_plain_step(emu, route, dtype, G):
    cc.rho1_case(emu, TINY, ITEMS["plain"], route, dtype, G)


@pytest.mark.parametrize("G", [None, 3])
def test_unit_ratio_is_the_plain_step_logit_free_head(emu, G):
    cc.rho1_case(emu, TINY, ITEMS["plain"], "ce_free", "bf16", G, dropout=0.1)


@pytest.mark.parametrize("route", ["ce", "item_trie"])
def test_unit_ratio_is_the_plain_step_sequence_ratio(emu, route):
    cc.rho1_case(emu, TINY, ITEMS["plain"], route, "fp32", 3, eps=0.0, ratio="sequence")


# ---- 3. everything clipped
@pytest.mark.parametrize("ratio", ["token", "sequence"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_all_clipped_moves_nothing(emu, dtype, ratio):
    cc.all_clipped_case(emu, TINY, ITEMS["plain"], dtype=dtype, ratio=ratio)


# ---- 4. meaning
@pytest.mark.parametrize("ratio", ["token", "sequence"])
def test_loss_and_gradients_against_oracle(emu, ratio):
    cc.meaning_case(emu, TINY, ITEMS["plain"], ratio)


# ---- 5. composition
@pytest.mark.parametrize("item_head", ["dense", "trie"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_policy_step_is_collect_then_update(emu, dtype, item_head):
    cc.composition_case(emu, TINY, ITEMS["plain"], dtype=dtype, item_head=item_head)


def test_policy_step_is_collect_then_update_regularised(emu):
    cc.composition_case(emu, TINY, ITEMS["plain"], reg=True, ratio="sequence", baseline="grpo", sft_coef=0.5)


@pytest.mark.parametrize("with_gold", [True, False])
def test_policy_batch_clip_keeps_the_bits_and_gathers(emu, with_gold):
    cc.batch_clip_case(emu, TINY, ITEMS["plain"], with_gold=with_gold)


@pytest.mark.parametrize("item_head", ["dense", "trie"])
def test_forward_old_logprobs_give_unit_ratio(emu, item_head):
    cc.forward_old_case(emu, TINY, ITEMS["plain"], item_head=item_head)


# ---- 6. it does what it is for
def test_several_updates_per_rollout_learn_and_clip(emu):
    """observed on the host emulation (6 rollouts x 4 updates, B = 4, S = 8, 8 items, lr 3e-5, eps 0.2, old_logprobs="forward"): gold
    log-probability -2.9623 -> -2.0476; share clipped 0 on every first update (and on the second from the second rollout on), 0.035 .. 0.068 on
    the third, 0.063 .. 0.122 on the fourth.  Half a nat is asked for, well inside what was observed; the step is bit-reproducible."""
    before, after, shares = cc.learns_case(emu, TINY)
    assert after > before + 0.5, (before, after)
    assert all(row[0] == 0.0 for row in shares), shares
    assert any(s > 0.0 for row in shares for s in row[1:]), shares


# ---- 7. refusals
def test_abi_refusals_name_their_cause(emu):
    cc.abi_errors_case(emu, TINY, ITEMS["plain"])


def test_model_refusals_precede_sampling_and_engine(emu):
    cc.model_errors_case(emu, TINY, ITEMS["plain"])


# ---- 8. the runner
def test_runner_clip_flags(emu, tmp_path, caplog):
    cc.runner_case(emu, str(tmp_path), caplog)


def test_runner_clip_under_accumulation(emu, tmp_path):
    cc.runner_accum_case(emu, str(tmp_path))


def test_runner_resume_between_rollouts(emu, tmp_path):
    cc.runner_resume_case(emu, str(tmp_path))


def test_runner_flags_at_defaults_issue_the_parents_calls(emu, tmp_path):
    cc.runner_off_case(emu, str(tmp_path))
