"""not-gpu: the on-policy fine-tuning step (csrc/p5_policy.h, P5T5Native.policy_batch / policy_step, --train_policy_samples) on the host
emulation of the kernels: the cases of tests/policy_cases.py."""
import pytest

from oracle import t5_oracle as O
from tests import policy_cases as pc
from tests import trie_loss_cases as tl

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()
COMBOS = pc.kernel_combos()


# ---- 1. the kernel against the float64 restatement
@pytest.mark.parametrize("S,baseline,given", COMBOS, ids=[f"S{s}-{b}-{'given' if g else 'hit'}" for s, b, g in COMBOS])
def test_kernel_against_fp64(emu, S, baseline, given):
    pc.kernel_case(emu, S, baseline, given)


# ---- 2. errors
def test_abi_refusals_name_their_cause(emu):
    pc.abi_errors_case(emu)


def test_model_refusals_precede_sampling_and_engine(emu):
    pc.model_errors_case(emu, TINY, ITEMS["plain"])


# ---- 3. composition, bit for bit
@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("item_head", ["dense", "trie"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_policy_step_is_its_parts(emu, dtype, item_head, dropout):
    pc.composition_case(emu, TINY, ITEMS["plain"], dtype=dtype, item_head=item_head, dropout=dropout)


def test_policy_step_is_its_parts_regularised(emu):
    pc.composition_case(emu, TINY, ITEMS["plain"], reg=True, baseline="grpo", token_sum=True, sft_coef=0.5, reward_fn=pc.index_reward)


def test_policy_step_is_its_parts_without_gold(emu):
    pc.composition_case(emu, TINY, ITEMS["plain"], baseline="mean", sft_coef=0.0, policy_coef=2.0, reward_fn=pc.index_reward)


# ---- 4. meaning
@pytest.mark.parametrize("token_sum", [False, True])
def test_loss_and_gradients_against_oracle(emu, token_sum):
    pc.meaning_case(emu, TINY, ITEMS["plain"], token_sum=token_sum)


# ---- 5. it learns
def test_reinforce_raises_gold_logprob(emu):
    """observed on the host emulation (20 steps, B = 4, S = 8, 8 items, lr 3e-5): -2.9623 -> -1.6505, hit rate 0.06 -> 0.41; half a nat is
    asked for, well inside what was observed, and there is no run-to-run noise: the step is bit-reproducible"""
    before, after = pc.learns_case(emu, TINY)
    assert after > before + 0.5, (before, after)


def test_zero_coefficients_leave_the_weights(emu):
    pc.zero_coef_case(emu, TINY)


# ---- 6. the runner
def test_runner_policy_flags(emu, tmp_path, caplog):
    pc.runner_case(emu, str(tmp_path), caplog)


def test_runner_resume_draws_what_the_straight_run_drew(emu, tmp_path):
    pc.runner_resume_case(emu, str(tmp_path))


def test_runner_flag_off_issues_the_parents_calls(emu, tmp_path):
    pc.runner_off_case(emu, str(tmp_path))
