"""not-gpu: the listwise preference objectives (csrc/p5_pref.h, loss_and_backward(preference=), sequence_logprobs, preference_step) on the
host emulation of the kernels: the cases of tests/pref_cases.py."""
import pytest

from oracle import t5_oracle as O
from tests import pref_cases as pf
from tests import trie_loss_cases as tl

TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


# ---- 1. the kernels against the float64 restatement
@pytest.mark.parametrize("option", pf.KERNEL_OPTIONS, ids=lambda o: "-".join(map(str, o)))
@pytest.mark.parametrize("shape", pf.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_fp64(emu, shape, option):
    pf.kernel_case(emu, *shape, option)


# ---- 2. bits
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("route", ["ce", "item_dense", "item_trie"])
def test_list_of_one_is_the_plain_weighted_step(emu, route, dtype, G):
    pf.bits_case(emu, TINY, ITEMS["plain"], route, dtype, G)


@pytest.mark.parametrize("G", [2, 4])
def test_list_of_one_is_the_plain_weighted_step_logit_free_head(emu, G):
    pf.bits_case(emu, TINY, ITEMS["plain"], "ce_free", "bf16", G, dropout=0.1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_pair_moves_nothing(emu, dtype):
    pf.no_pair_case(emu, TINY, ITEMS["plain"], dtype=dtype)


# ---- 3. meaning
@pytest.mark.parametrize("name", sorted(pf.MEANING))
def test_loss_and_gradients_against_oracle(emu, name):
    pf.meaning_case(emu, TINY, ITEMS["plain"], name)


# ---- 4. composition
@pytest.mark.parametrize("negatives", ["slate", "sample"])
@pytest.mark.parametrize("item_head", ["dense", "trie"])
def test_preference_step_is_its_parts(emu, item_head, negatives):
    pf.composition_case(emu, TINY, ITEMS["plain"], item_head=item_head, negatives=negatives)


def test_preference_step_is_its_parts_bf16_ipo(emu):
    pf.composition_case(emu, TINY, ITEMS["plain"], dtype="bf16", preference="ipo", pref_depth=None)


def test_a_draw_that_hit_the_gold_item_is_skipped(emu):
    pf.hit_skipped_case(emu, TINY)


# ---- 5. it does what it is for
def test_preference_steps_raise_margin_and_gold_logprob(emu):
    """observed on the host emulation (5 steps of softmax-DPO, beta 0.5, B = 4, S = 2 distinct negatives, 8 items, lr 1e-4, reference = the
    initial weights): mean margin 0.0000 -> 1.1012, gold log-probability -2.9623 -> -0.8746.  Half of either gain is asked for; the step is
    bit-reproducible."""
    m0, m1, before, after = pf.learns_case(emu, TINY)
    assert m1 > m0 + 0.55, (m0, m1)
    assert after > before + 1.04, (before, after)


# ---- 6. refusals
def test_abi_refusals_name_their_cause(emu):
    pf.abi_errors_case(emu, TINY, ITEMS["plain"])


def test_model_refusals_precede_sampling_and_engine(emu):
    pf.model_errors_case(emu, TINY, ITEMS["plain"])


# ---- 7. the runner
def test_runner_preference_flags(emu, tmp_path, caplog):
    pf.runner_case(emu, str(tmp_path), caplog)


def test_runner_resume(emu, tmp_path):
    pf.runner_resume_case(emu, str(tmp_path))


def test_runner_flags_absent_issue_the_parents_calls(emu, tmp_path):
    pf.runner_off_case(emu, str(tmp_path))
