"""not-gpu: the slate policy step (csrc/p5_slate_policy.h, P5T5Native.policy_slate_batch / policy_step(slate_size=...), --policy_slate_size) on
the host emulation of the kernels: the cases of tests/slate_policy_cases.py."""
import pytest

from oracle import t5_oracle as O
from tests import cases
from tests import slate_policy_cases as sp
from tests import trie_loss_cases as tl

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()
ITEMS8 = cases.make_items(8, 5, hi=60)
COMBOS = sp.kernel_combos()


# ---- 1. the kernel against the float64 restatement
@pytest.mark.parametrize("S,K1,estimator,given", COMBOS, ids=[f"S{s}-K1_{k}-{e}-{'given' if g else 'hit'}" for s, k, e, g in COMBOS])
def test_kernel_against_fp64(emu, S, K1, estimator, given):
    sp.kernel_case(emu, S, K1, estimator, given)


@pytest.mark.parametrize("estimator", ["unbiased", "normalized"])
def test_slates_are_independent(emu, estimator):
    sp.independence_case(emu, estimator)


def test_slates_are_independent_with_root_noise(emu):
    sp.independence_case(emu, "normalized", noise=sp.NOISE)


@pytest.mark.parametrize("estimator", ["unbiased", "normalized"])
@pytest.mark.parametrize("S,K1", [(3, 4), (5, 3)])
def test_kernel_with_root_noise_against_fp64(emu, S, K1, estimator):
    sp.noise_kernel_case(emu, S, K1, estimator)


# ---- 2. the restatement against the distribution (numpy only)
@pytest.mark.parametrize("K", [1, 3, 6])
def test_restatement_is_unbiased(K):
    sp.distribution_case(K)


def test_restatement_exact_gradient_when_catalogue_fits():
    sp.exact_gradient_case()


# ---- 3. the sampler's threshold is the kernel's
def test_sampler_and_kernel_agree_on_threshold(emu):
    """ONE user here (its 1024 slates are two minutes of emulated decode rows, the costliest case of this file); the MI355X test runs the
    three users of the case in a second.  A user's draws do not depend on the batch, so this is user 0 of that test: the same margins."""
    sp.threshold_case(emu, TINY, B=1)


# ---- 4. meaning
def test_exact_gradient_when_catalogue_fits(emu):
    sp.exact_meaning_case(emu, TINY)


@pytest.mark.parametrize("estimator", ["unbiased", "normalized"])
def test_loss_and_gradients_against_oracle(emu, estimator):
    sp.meaning_case(emu, TINY, ITEMS8, estimator)


# ---- 5. composition, bit for bit
@pytest.mark.parametrize("item_head", ["dense", "trie"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_slate_step_is_its_parts(emu, dtype, item_head):
    sp.composition_case(emu, TINY, ITEMS["plain"], dtype=dtype, item_head=item_head)


def test_slate_step_is_its_parts_regularised(emu):
    sp.composition_case(emu, TINY, ITEMS["plain"], reg=True, estimator="unbiased", token_sum=True, sft_coef=0.5)


def test_slate_step_clipped_is_collect_and_update(emu):
    sp.clip_case(emu, TINY, ITEMS["plain"])


# ---- 6. refusals
def test_abi_refusals_name_their_cause(emu):
    sp.abi_errors_case(emu)


def test_model_refusals_precede_sampling_and_engine(emu):
    sp.model_errors_case(emu, TINY, ITEMS["plain"])


# ---- 7. it learns
def test_reinforce_from_slates_raises_gold_logprob(emu):
    """observed on the host emulation (20 steps, B = 4, S = 2 slates of K = 4, 8 items, lr 3e-5): -2.9623 -> -1.4154; half a nat is asked
    for, a third of the observed rise, and there is no run-to-run noise: the step is bit-reproducible"""
    before, after = sp.learns_case(emu, TINY)
    assert after > before + sp.LEARN_MARGIN, (before, after)


# ---- 8. the runner
def test_runner_slate_flags(emu, tmp_path, caplog):
    sp.runner_case(emu, str(tmp_path), caplog)


def test_runner_resume_draws_what_the_straight_run_drew(emu, tmp_path):
    sp.runner_resume_case(emu, str(tmp_path))


def test_runner_flag_off_issues_the_parents_calls(emu, tmp_path):
    sp.runner_off_case(emu, str(tmp_path))
