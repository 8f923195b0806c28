"""gpu: the slate policy step (csrc/p5_slate_policy.h, P5T5Native.policy_slate_batch / policy_step(slate_size=...), --policy_slate_size) on
the MI355X: the cases of tests/test_slate_policy_emu.py (tests/slate_policy_cases.py) that run kernels."""
import pytest

from oracle import t5_oracle as O
from tests import cases
from tests import slate_policy_cases as sp
from tests import trie_loss_cases as tl

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()
ITEMS8 = cases.make_items(8, 5, hi=60)
COMBOS = sp.kernel_combos()


# ---- 1. the kernel against the float64 restatement
@pytest.mark.parametrize("S,K1,estimator,given", COMBOS, ids=[f"S{s}-K1_{k}-{e}-{'given' if g else 'hit'}" for s, k, e, g in COMBOS])
def test_kernel_against_fp64(hip, S, K1, estimator, given):
    sp.kernel_case(hip, S, K1, estimator, given)


@pytest.mark.parametrize("estimator", ["unbiased", "normalized"])
def test_slates_are_independent(hip, estimator):
    sp.independence_case(hip, estimator)


def test_slates_are_independent_with_root_noise(hip):
    sp.independence_case(hip, "normalized", noise=sp.NOISE)


@pytest.mark.parametrize("estimator", ["unbiased", "normalized"])
@pytest.mark.parametrize("S,K1", [(3, 4), (5, 3)])
def test_kernel_with_root_noise_against_fp64(hip, S, K1, estimator):
    sp.noise_kernel_case(hip, S, K1, estimator)


# ---- 3. the sampler's threshold is the kernel's
def test_sampler_and_kernel_agree_on_threshold(hip):
    sp.threshold_case(hip, TINY)


# ---- 4. meaning
def test_exact_gradient_when_catalogue_fits(hip):
    sp.exact_meaning_case(hip, TINY)


@pytest.mark.parametrize("estimator", ["unbiased", "normalized"])
def test_loss_and_gradients_against_oracle(hip, estimator):
    sp.meaning_case(hip, TINY, ITEMS8, estimator)


# ---- 5. composition, bit for bit
@pytest.mark.parametrize("item_head", ["dense", "trie"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_slate_step_is_its_parts(hip, dtype, item_head):
    sp.composition_case(hip, TINY, ITEMS["plain"], dtype=dtype, item_head=item_head)


def test_slate_step_is_its_parts_regularised(hip):
    sp.composition_case(hip, TINY, ITEMS["plain"], reg=True, estimator="unbiased", token_sum=True, sft_coef=0.5)


def test_slate_step_clipped_is_collect_and_update(hip):
    sp.clip_case(hip, TINY, ITEMS["plain"])


# ---- 6. refusals
def test_abi_refusals_name_their_cause(hip):
    sp.abi_errors_case(hip)


def test_model_refusals_precede_sampling_and_engine(hip):
    sp.model_errors_case(hip, TINY, ITEMS["plain"])


# ---- 7. it learns
def test_reinforce_from_slates_raises_gold_logprob(hip):
    """the margin of tests/test_slate_policy_emu.py; observed on the MI355X: -2.9623 -> -1.4154, the emulation's trajectory to four digits"""
    before, after = sp.learns_case(hip, TINY)
    assert after > before + sp.LEARN_MARGIN, (before, after)


# ---- 8. the runner
def test_runner_slate_flags(hip, tmp_path, caplog):
    sp.runner_case(hip, str(tmp_path), caplog)


def test_runner_resume_draws_what_the_straight_run_drew(hip, tmp_path):
    sp.runner_resume_case(hip, str(tmp_path))


def test_runner_flag_off_issues_the_parents_calls(hip, tmp_path):
    sp.runner_off_case(hip, str(tmp_path))
