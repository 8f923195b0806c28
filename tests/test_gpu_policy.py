"""gpu: the on-policy fine-tuning step (csrc/p5_policy.h, P5T5Native.policy_batch / policy_step, --train_policy_samples) on the MI355X: the
cases of tests/test_policy_emu.py (tests/policy_cases.py)."""
import pytest

from oracle import t5_oracle as O
from tests import policy_cases as pc
from tests import trie_loss_cases as tl

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()
COMBOS = pc.kernel_combos()


# ---- 1. the kernel against the float64 restatement
@pytest.mark.parametrize("S,baseline,given", COMBOS, ids=[f"S{s}-{b}-{'given' if g else 'hit'}" for s, b, g in COMBOS])
def test_kernel_against_fp64(hip, S, baseline, given):
    pc.kernel_case(hip, S, baseline, given)


# ---- 2. errors
def test_abi_refusals_name_their_cause(hip):
    pc.abi_errors_case(hip)


def test_model_refusals_precede_sampling_and_engine(hip):
    pc.model_errors_case(hip, TINY, ITEMS["plain"])


# ---- 3. composition, bit for bit
@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("item_head", ["dense", "trie"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_policy_step_is_its_parts(hip, dtype, item_head, dropout):
    pc.composition_case(hip, TINY, ITEMS["plain"], dtype=dtype, item_head=item_head, dropout=dropout)


def test_policy_step_is_its_parts_regularised(hip):
    pc.composition_case(hip, TINY, ITEMS["plain"], reg=True, baseline="grpo", token_sum=True, sft_coef=0.5, reward_fn=pc.index_reward)


def test_policy_step_is_its_parts_without_gold(hip):
    pc.composition_case(hip, TINY, ITEMS["plain"], baseline="mean", sft_coef=0.0, policy_coef=2.0, reward_fn=pc.index_reward)


# ---- 4. meaning
@pytest.mark.parametrize("token_sum", [False, True])
def test_loss_and_gradients_against_oracle(hip, token_sum):
    pc.meaning_case(hip, TINY, ITEMS["plain"], token_sum=token_sum)


# ---- 5. it learns
def test_reinforce_raises_gold_logprob(hip):
    """the margin of tests/test_policy_emu.py: the draws are the engine's own, so the trajectory is the device's, not the emulation's"""
    before, after = pc.learns_case(hip, TINY)
    assert after > before + 0.5, (before, after)


def test_zero_coefficients_leave_the_weights(hip):
    pc.zero_coef_case(hip, TINY)


# ---- 6. the runner (the tiny pipeline of tests/test_gpu_runner.py::test_resume_on_device: seconds)
def test_runner_policy_flags(hip, tmp_path, caplog):
    pc.runner_case(hip, str(tmp_path), caplog)


def test_runner_resume_draws_what_the_straight_run_drew(hip, tmp_path):
    pc.runner_resume_case(hip, str(tmp_path))
