"""gpu: the clipped-ratio policy objective (csrc/p5_clip.h, loss_and_backward(old_logprobs=, clip_eps=), policy_collect / policy_update) on the
MI355X: the cases of tests/test_clip_emu.py (tests/clip_cases.py) through the product library."""
import pytest

from oracle import t5_oracle as O
from tests import clip_cases as cc
from tests import trie_loss_cases as tl

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


# ---- 1. the kernels against the float64 restatement
@pytest.mark.parametrize("eps", cc.KERNEL_EPS, ids=lambda e: f"eps{e[0]}-{e[1]}")
@pytest.mark.parametrize("ratio", ["token", "sequence"])
@pytest.mark.parametrize("shape", cc.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_fp64(hip, shape, ratio, eps):
    cc.kernel_case(hip, *shape, ratio, eps)


# ---- 2. rho == 1 is the plain step, bit for bit
@pytest.mark.parametrize("G", [None, 3])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("route", ["ce", "item_dense", "item_trie", "reg"])
def test_unit_ratio_is_the_plain_step(hip, route, dtype, G):
    cc.rho1_case(hip, TINY, ITEMS["plain"], route, dtype, G)


@pytest.mark.parametrize("G", [None, 3])
def test_unit_ratio_is_the_plain_step_logit_free_head(hip, G):
    cc.rho1_case(hip, TINY, ITEMS["plain"], "ce_free", "bf16", G, dropout=0.1)


@pytest.mark.parametrize("route", ["ce", "item_trie"])
def test_unit_ratio_is_the_plain_step_sequence_ratio(hip, route):
    cc.rho1_case(hip, TINY, ITEMS["plain"], route, "fp32", 3, eps=0.0, ratio="sequence")


# ---- 3. everything clipped
@pytest.mark.parametrize("ratio", ["token", "sequence"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_all_clipped_moves_nothing(hip, dtype, ratio):
    cc.all_clipped_case(hip, TINY, ITEMS["plain"], dtype=dtype, ratio=ratio)


# ---- 4. meaning
@pytest.mark.parametrize("ratio", ["token", "sequence"])
def test_loss_and_gradients_against_oracle(hip, ratio):
    cc.meaning_case(hip, TINY, ITEMS["plain"], ratio)


# ---- 5. composition
@pytest.mark.parametrize("item_head", ["dense", "trie"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_policy_step_is_collect_then_update(hip, dtype, item_head):
    cc.composition_case(hip, TINY, ITEMS["plain"], dtype=dtype, item_head=item_head)


def test_policy_step_is_collect_then_update_regularised(hip):
    cc.composition_case(hip, TINY, ITEMS["plain"], reg=True, ratio="sequence", baseline="grpo", sft_coef=0.5)


@pytest.mark.parametrize("with_gold", [True, False])
def test_policy_batch_clip_keeps_the_bits_and_gathers(hip, with_gold):
    cc.batch_clip_case(hip, TINY, ITEMS["plain"], with_gold=with_gold)


@pytest.mark.parametrize("item_head", ["dense", "trie"])
def test_forward_old_logprobs_give_unit_ratio(hip, item_head):
    cc.forward_old_case(hip, TINY, ITEMS["plain"], item_head=item_head)


# ---- 7. refusals
def test_abi_refusals_name_their_cause(hip):
    cc.abi_errors_case(hip, TINY, ITEMS["plain"])


def test_model_refusals_precede_sampling_and_engine(hip):
    cc.model_errors_case(hip, TINY, ITEMS["plain"])


# ---- 8. the runner
def test_runner_clip_flags(hip, tmp_path, caplog):
    cc.runner_case(hip, str(tmp_path), caplog)


def test_runner_clip_under_accumulation(hip, tmp_path):
    cc.runner_accum_case(hip, str(tmp_path))


def test_runner_resume_between_rollouts(hip, tmp_path):
    cc.runner_resume_case(hip, str(tmp_path))
