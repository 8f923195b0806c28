"""not-gpu: training on several targets per user with one encoder pass (`labels [B, G, T]`, p5_forward_targets / p5_forward_loss_targets) on
the host emulation of the kernels: the cases of tests/multi_target_cases.py against the oracle on the replicated batch."""
import pytest

from oracle import t5_oracle as O
from tests import multi_target_cases as mt
from tests import trie_loss_cases as tl

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()
SHAPE_IDS = ["x".join(map(str, s)) for s, _ in mt.SHAPES]


# ---- 1. shapes
@pytest.mark.parametrize("shape", [s for s, _ in mt.SHAPES], ids=SHAPE_IDS)
def test_shapes_fp32(emu, shape):
    mt.shape_case(emu, TINY, shape, "fp32")


@pytest.mark.parametrize("shape", [s for s, b in mt.SHAPES if b], ids=[i for i, (_, b) in zip(SHAPE_IDS, mt.SHAPES) if b])
def test_shapes_bf16(emu, shape):
    mt.shape_case(emu, TINY, shape, "bf16")


# ---- 2. G = 1 bits
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_g1_labels_view_returns_the_2d_bits(emu, dtype):
    mt.g1_python_case(emu, TINY, dtype=dtype)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_g1_old_entry_points_are_the_new_ones(emu, dtype, dropout):
    mt.g1_abi_case(emu, TINY, dtype, dropout)


# ---- 3. fused loss
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_fused_loss_and_weights(emu, dropout):
    mt.fused_case(emu, TINY, dropout=dropout)


def test_fused_loss_bf16_grouped_plan(emu):
    mt.fused_case(emu, TINY, B=2, L=32, T=8, G=4, dtype="bf16")


def test_weights_zero_and_negative_against_oracle(emu):
    mt.weights_oracle_case(emu, TINY)


def test_zero_weight_user_drops_out(emu):
    mt.dead_user_case(emu, TINY)


def test_zero_weight_and_masked_targets_contribute_exact_zeros(emu):
    mt.zero_target_exact_case(emu, TINY)


# ---- 4. dropout
def test_dropout_masks_of_the_formed_tensors(emu):
    mt.restatement_case(TINY)       # (the reference itself: without dropout it is the oracle on the replicated batch)
    mt.dropout_case(emu, TINY)


# ---- 5. item loss
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_item_loss_excluded_per_user(emu, dtype):
    mt.item_case(emu, TINY, ITEMS["plain"], dtype=dtype)


def test_item_loss_plain(emu):
    mt.item_case(emu, TINY, ITEMS["fan33"], tau=1.0, excluded=False)


@pytest.mark.parametrize("trunc", [dict(top_k=2), dict(top_p=0.7)], ids=["top_k2", "top_p0.7"])
def test_item_loss_truncated_equals_replicated(emu, trunc):
    mt.item_trunc_case(emu, TINY, ITEMS["plain"], **trunc)


@pytest.mark.parametrize("head", ["dense", "trie"])
@pytest.mark.parametrize("trunc", [dict(), dict(top_k=2), dict(top_p=0.7)], ids=["plain", "top_k2", "top_p0.7"])
def test_fused_item_loss_weights_exclusion(emu, trunc, head):
    mt.fused_item_case(emu, TINY, ITEMS["plain"], item_head=head, **trunc)


@pytest.mark.parametrize("head", ["dense", "trie"])
def test_fused_item_loss_weights_exclusion_bf16(emu, head):
    mt.fused_item_case(emu, TINY, ITEMS["plain"], dtype="bf16", item_head=head)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_item_head_trie_against_dense(emu, dtype):
    mt.item_head_case(emu, TINY, ITEMS["plain"], dtype=dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampler_draws_are_labels(emu, dtype):
    mt.sampler_case(emu, TINY, ITEMS["plain"], dtype=dtype)


def test_slates_are_labels_and_empty_slots_score_nothing(emu):
    mt.slates_case(emu, TINY)


# ---- 6. accumulation and staging
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_micro_batches_accumulate(emu, dtype):
    mt.accumulation_case(emu, TINY, dtype=dtype)


def test_micro_batches_accumulate_bf16_grouped_plan(emu):
    mt.accumulation_case(emu, TINY, dtype="bf16", B=2, L=32, T=8, G=4)


def test_staged_backward(emu):
    mt.staged_case(emu, TINY, 2, 32, 8, 4)
    mt.staged_case(emu, TINY, 3, 10, 5, 3, dtype="fp32")
    mt.staged_case(emu, O.T5Cfg.named("tiny", num_layers=3, num_decoder_layers=2), 4, 16, 4, 4, dropout=0.1)


# ---- 7. errors and workspace
def test_limits_raise_before_the_engine(emu):
    mt.errors_case(emu, TINY)


def test_workspace_exact_and_guards(emu):
    mt.workspace_case(emu, TINY)
