"""not-gpu: top-k / nucleus truncation of trie sampling and of the item loss (csrc/p5_trunc.h) on the host emulation of the kernels, against
the float64 semantics of tests/trunc_cases.py."""
import os
import subprocess
import sys

import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases, trunc_cases

TINY = O.T5Cfg.named("tiny")
EMU_FREQ_S = 80          # draws per user of the frequency test on the emulator (the GPU test draws 2048)


def _items(n=40, **kw):
    return cases.make_items(n, 5, hi=60, **kw)


def _fan(n):
    """one level of n siblings behind the shared prefix, short tails (tests/test_sample_items_emu.py)"""
    return [[0, 5, 6, 10 + i] + ([40 + (i % 7)] if i % 3 == 0 else []) + [1] for i in range(n)]


def test_semantics_are_hf_warpers():
    trunc_cases.hf_pin_case()


def test_reference_edges():
    """the float64 reference on hand-made rows: ties at the k-th place stay, a tie group across the nucleus boundary stays whole, the
    largest value always stays, -inf is never kept"""
    import torch
    z = torch.tensor([1.0, 3.0, 2.0, 2.0, float("-inf"), 0.0], dtype=torch.float64)
    assert trunc_cases.kept_ref(z, 2, 1.0)[0].tolist() == [False, True, True, True, False, False]
    assert trunc_cases.kept_ref(z, 9, 1.0)[0].tolist() == [True, True, True, True, False, True]
    assert trunc_cases.kept_ref(z, 0, 1e-6)[0].tolist() == [False, True, False, False, False, False]
    p3 = float(torch.softmax(z, 0)[1])
    keep, cut, _ = trunc_cases.kept_ref(z, 0, p3 + 0.01)          # the boundary falls inside the pair of 2.0s: both stay
    assert keep.tolist() == [False, True, True, True, False, False] and cut == 2.0
    assert trunc_cases.kept_ref(torch.full((4,), float("-inf"), dtype=torch.float64), 1, 0.5)[1] == float("inf")
    si, so = trunc_cases.classify(z, 2, 1.0, 1e-4)
    assert si.tolist() == [False, True, False, False, False, False] and so.tolist() == [True, False, False, False, True, True]


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_kernels_one_by_one(emu, tau):
    trunc_cases.op_case(emu, tau)


def test_kernel_entry_points_reject_bad_truncation(emu):
    trunc_cases.op_errors_case(emu)


@pytest.mark.parametrize("top_k,top_p", [(2, 1.0), (0, 0.5), (3, 0.8), (5, 0.95)])
def test_replay_and_logprobs_fp32(emu, top_k, top_p):
    trunc_cases.sample_case(emu, TINY, 3, 20, _items(), 8, top_k=top_k, top_p=top_p)


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_temperature_and_exclusion(emu, tau):
    n = len(_items())
    trunc_cases.sample_case(emu, TINY, 3, 12, _items(), 8, top_k=3, top_p=0.8, tau=tau, excluded_items=[list(range(0, n, 2)), [], list(range(1, n, 3))])


@pytest.mark.parametrize("fan", [1, 2, 32, 33])
def test_fan_out(emu, fan):
    trunc_cases.sample_case(emu, TINY, 2, 12, _fan(fan), 6, top_k=5, top_p=0.8, tag=f" fan-out {fan}")


def test_fan_out_250(emu):
    trunc_cases.sample_case(emu, TINY, 2, 12, rank_cases.fanout_items(250), 12, top_k=5, top_p=0.95, seed=2, tag=" fan-out 250")


@pytest.mark.parametrize("top_k,top_p", [(40, 1.0), (0, 0.9)])
def test_fan_out_above_the_lds_stage(emu, top_k, top_p):
    """one node of 2049 children (a vocabulary of 2200): the z row of the step lives in the workspace's scratch, not in LDS.  Under top-p
    the node cannot be decided at 1e-4: a child holds about 5e-4 of the mass and a logit error of 1e-4 moves the boundary by 2e-4 of it, so
    some child always lies across -- the three-way check, which must bite, without the cap (the node is one of four on a path)."""
    wide = O.T5Cfg.named("tiny", vocab_size=2200)
    items = [[0, 5, 6, 10 + i, 1] for i in range(trunc_cases.STAGE + 1)]
    trunc_cases.sample_case(emu, wide, 2, 12, items, 4, top_k=top_k, top_p=top_p, capped=top_p == 1.0, tag=" fan-out 2049")


@pytest.mark.parametrize("top_k,top_p", [(5, 1.0), (0, 0.95)])
def test_common_random_numbers(emu, top_k, top_p):
    trunc_cases.crn_case(emu, TINY, _items(), top_k=top_k, top_p=top_p)


def test_top_k_1_is_greedy(emu):
    trunc_cases.greedy_case(emu, TINY, _items())


@pytest.mark.parametrize("top_k,top_p", [(2, 1.0), (0, 0.5)])
def test_frequencies(emu, top_k, top_p):
    trunc_cases.frequency_case(emu, TINY, EMU_FREQ_S, top_k=top_k, top_p=top_p)


def test_determinism_chunks_draw_ranges_streams_and_lanes(emu):
    trunc_cases.determinism_case(emu, TINY)


def test_off_is_off_and_workspace_bytes_are_exact(emu):
    trunc_cases.off_case(emu, TINY)


def test_errors(emu):
    trunc_cases.errors_case(emu, TINY)


@pytest.mark.parametrize("top_k,top_p", [(2, 1.0), (0, 0.5)], ids=["top_k", "top_p"])
def test_three_way_bf16(emu, top_k, top_p):
    trunc_cases.sample_case(emu, TINY, 3, 20, _items(), 8, top_k=top_k, top_p=top_p, dtype="bf16")


# ---- item loss ----
@pytest.mark.parametrize("top_k,top_p,dropout,tau,excluded", [(2, 1.0, 0.0, 1.0, False), (0, 0.5, 0.0, 1.0, False), (3, 0.8, 0.1, 0.7, True)],
                         ids=["top_k", "top_p", "both_dropout_tau_excluded"])
def test_item_loss_against_float64_autograd(emu, top_k, top_p, dropout, tau, excluded):
    trunc_cases.model_case(emu, TINY, _items(), top_k=top_k, top_p=top_p, dropout=dropout, tau=tau, excluded=excluded)


@pytest.mark.parametrize("top_k,top_p,tau,excluded", [(3, 0.8, 1.0, False), (0, 0.5, 0.7, True)])
def test_item_loss_is_the_samplers_logprob(emu, top_k, top_p, tau, excluded):
    trunc_cases.sampler_case(emu, TINY, _items(), 3, 12, 6, top_k=top_k, top_p=top_p, tau=tau, excluded=excluded)


def test_item_loss_fan_out_250(emu):
    trunc_cases.sampler_case(emu, TINY, rank_cases.fanout_items(250), 2, 12, 6, top_k=5, top_p=0.95, tag=" fan-out 250")


@pytest.mark.parametrize("dtype,dropout", [("fp32", 0.0), ("bf16", 0.1)])
def test_fused_loss_and_backward(emu, dtype, dropout):
    trunc_cases.fused_case(emu, TINY, _items(), dtype=dtype, dropout=dropout)


def test_accumulation_and_reproducibility_bf16(emu):
    trunc_cases.reproducible_case(emu, TINY, _items())


def test_plain_route_restored(emu):
    trunc_cases.plain_route_restored_case(emu, TINY, _items())


def test_runner_flags(emu, tmp_path):
    trunc_cases.runner_case(emu, str(tmp_path))


@pytest.mark.parametrize("env", [{"P5_EMU_POISON_LDS": "1"}, {"P5_EMU_FIBER_ORDER": "reverse"}, {"P5_EMU_BLOCK_ORDER": "reverse"}],
                         ids=["poison_lds", "fiber_reverse", "block_reverse"])
def test_truncation_kernels_under_adversarial_emulation(env):
    """replay, fan-out 250 and an item-loss test under the emulator's adversarial modes, each in a fresh process (the modes are read once per
    process): no kernel may read LDS it has not written or depend on thread / workgroup order"""
    sel = "test_replay_and_logprobs_fp32 or test_fan_out_250 or test_item_loss_is_the_samplers_logprob"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", sel, "-p", "no:cacheprovider"],
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
