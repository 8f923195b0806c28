"""gpu: top-k / nucleus truncation of trie sampling and of the item loss (csrc/p5_trunc.h) on the MI355X through the C ABI, against the
float64 semantics of tests/trunc_cases.py -- the cases of tests/test_trunc_emu.py at the same small shapes, and the frequencies at 2048 draws."""
import ctypes
import os

import pytest

from oracle import t5_oracle as O
from tests import cases, rank_cases, trunc_cases

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")


def _items(n=40, **kw):
    return cases.make_items(n, 5, hi=60, **kw)


def _fan(n):
    return [[0, 5, 6, 10 + i] + ([40 + (i % 7)] if i % 3 == 0 else []) + [1] for i in range(n)]


def test_abi_symbols(hip):
    from openp5_amd import _abi
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openp5_amd", "libp5hip.so"))
    for name in ("p5_sample_items_truncated", "p5_sample_truncated_workspace_bytes", "p5_train_set_item_loss_truncated", "p5_op_trunc_cut",
                 "p5_op_trunc_ce_fwd", "p5_op_trunc_ce_bwd"):
        assert hasattr(lib, name) and name in _abi.PROTOTYPES, name
    assert len(_abi.PROTOTYPES["p5_train_set_item_loss_truncated"][1]) == 12
    assert hip.lib.p5_abi_version() == 6 and hip.lib.p5_is_emulator() == 0


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_kernels_one_by_one(hip, tau):
    trunc_cases.op_case(hip, tau)


def test_kernel_entry_points_reject_bad_truncation(hip):
    trunc_cases.op_errors_case(hip)


@pytest.mark.parametrize("top_k,top_p", [(2, 1.0), (0, 0.5), (3, 0.8), (5, 0.95)])
def test_replay_and_logprobs_fp32(hip, top_k, top_p):
    trunc_cases.sample_case(hip, TINY, 3, 20, _items(), 8, top_k=top_k, top_p=top_p)


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_temperature_and_exclusion(hip, tau):
    n = len(_items())
    trunc_cases.sample_case(hip, TINY, 3, 12, _items(), 8, top_k=3, top_p=0.8, tau=tau, excluded_items=[list(range(0, n, 2)), [], list(range(1, n, 3))])


@pytest.mark.parametrize("fan", [1, 2, 32, 33])
def test_fan_out(hip, fan):
    trunc_cases.sample_case(hip, TINY, 2, 12, _fan(fan), 6, top_k=5, top_p=0.8, tag=f" fan-out {fan}")


def test_fan_out_250(hip):
    trunc_cases.sample_case(hip, TINY, 2, 12, rank_cases.fanout_items(250), 12, top_k=5, top_p=0.95, seed=2, tag=" fan-out 250")


@pytest.mark.parametrize("top_k,top_p", [(40, 1.0), (0, 0.9)])
def test_fan_out_above_the_lds_stage(hip, top_k, top_p):
    """one node of 2049 children (a vocabulary of 2200): the z row of the step lives in the workspace's scratch, not in LDS.  Under top-p
    the node cannot be decided at 1e-4: a child holds about 5e-4 of the mass and a logit error of 1e-4 moves the boundary by 2e-4 of it, so
    some child always lies across -- the three-way check, which must bite, without the cap (the node is one of four on a path)."""
    wide = O.T5Cfg.named("tiny", vocab_size=2200)
    items = [[0, 5, 6, 10 + i, 1] for i in range(trunc_cases.STAGE + 1)]
    trunc_cases.sample_case(hip, wide, 2, 12, items, 4, top_k=top_k, top_p=top_p, capped=top_p == 1.0, tag=" fan-out 2049")


@pytest.mark.parametrize("top_k,top_p", [(5, 1.0), (0, 0.95)])
def test_common_random_numbers(hip, top_k, top_p):
    trunc_cases.crn_case(hip, TINY, _items(), top_k=top_k, top_p=top_p)


def test_top_k_1_is_greedy(hip):
    trunc_cases.greedy_case(hip, TINY, _items())


@pytest.mark.parametrize("top_k,top_p", [(2, 1.0), (0, 0.5)])
def test_frequencies(hip, top_k, top_p):
    trunc_cases.frequency_case(hip, TINY, 2048, top_k=top_k, top_p=top_p)


def test_determinism_chunks_draw_ranges_streams_and_lanes(hip):
    trunc_cases.determinism_case(hip, TINY)


def test_off_is_off_and_workspace_bytes_are_exact(hip):
    trunc_cases.off_case(hip, TINY)


def test_errors(hip):
    trunc_cases.errors_case(hip, TINY)


@pytest.mark.parametrize("top_k,top_p", [(2, 1.0), (0, 0.5)], ids=["top_k", "top_p"])
def test_three_way_bf16(hip, top_k, top_p):
    trunc_cases.sample_case(hip, TINY, 3, 20, _items(), 8, top_k=top_k, top_p=top_p, dtype="bf16")


@pytest.mark.parametrize("top_k,top_p,dropout,tau,excluded", [(2, 1.0, 0.0, 1.0, False), (0, 0.5, 0.0, 1.0, False), (3, 0.8, 0.1, 0.7, True)],
                         ids=["top_k", "top_p", "both_dropout_tau_excluded"])
def test_item_loss_against_float64_autograd(hip, top_k, top_p, dropout, tau, excluded):
    trunc_cases.model_case(hip, TINY, _items(), top_k=top_k, top_p=top_p, dropout=dropout, tau=tau, excluded=excluded)


@pytest.mark.parametrize("top_k,top_p,tau,excluded", [(3, 0.8, 1.0, False), (0, 0.5, 0.7, True)])
def test_item_loss_is_the_samplers_logprob(hip, top_k, top_p, tau, excluded):
    trunc_cases.sampler_case(hip, TINY, _items(), 3, 12, 6, top_k=top_k, top_p=top_p, tau=tau, excluded=excluded)


def test_item_loss_fan_out_250(hip):
    trunc_cases.sampler_case(hip, TINY, rank_cases.fanout_items(250), 2, 12, 6, top_k=5, top_p=0.95, tag=" fan-out 250")


@pytest.mark.parametrize("dtype,dropout", [("fp32", 0.0), ("bf16", 0.1)])
def test_fused_loss_and_backward(hip, dtype, dropout):
    trunc_cases.fused_case(hip, TINY, _items(), dtype=dtype, dropout=dropout)


def test_accumulation_and_reproducibility_bf16(hip):
    trunc_cases.reproducible_case(hip, TINY, _items())


def test_plain_route_restored(hip):
    trunc_cases.plain_route_restored_case(hip, TINY, _items())
