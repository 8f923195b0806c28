"""gpu: the item loss on a head restricted to the trie's tokens (`forward(trie=..., item_head="trie")`, csrc/p5_item_head.h) on the MI355X: the
cases of tests/test_trie_head_emu.py (tests/trie_head_cases.py), plus the two routes against each other at T5-small width on the
benchmark's catalogue."""
import pytest
import torch

from oracle import t5_oracle as O
from openp5_amd.model import P5T5Native
from tests import trie_head_cases as th, trie_loss_cases as tl, trunc_cases as tc

pytestmark = pytest.mark.gpu
TINY = O.T5Cfg.named("tiny")
ITEMS = tl.item_sets()


@pytest.fixture
def trie_head(monkeypatch):
    monkeypatch.setattr(P5T5Native, "item_head", "trie")


# ---- op level ----
def test_gather_and_scatter(hip):
    th.gather_scatter_case(hip)


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_compact_cross_entropy_equals_dense(hip, tau):
    th.ce_case(hip, tau)


def test_compact_cross_entropy_one_position_per_sample(hip):
    th.ce_case(hip, 1.0, T=1)


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_compact_truncated_cross_entropy_equals_dense(hip, tau):
    th.trunc_ce_case(hip, tau)


def test_errors_of_the_abi_and_the_keyword(hip):
    th.abi_errors_case(hip, TINY)


# ---- the existing cases under the class attribute ----
@pytest.mark.parametrize("name", sorted(ITEMS))
def test_model_fp32(hip, trie_head, name):
    tl.model_case(hip, TINY, ITEMS[name])


def test_model_fp32_dropout(hip, trie_head):
    tl.model_case(hip, TINY, ITEMS["plain"], dropout=0.1)


def test_model_fp32_temperature(hip, trie_head):
    tl.model_case(hip, TINY, ITEMS["plain"], tau=0.7)


def test_model_fp32_excluded_items(hip, trie_head):
    tl.model_case(hip, TINY, ITEMS["plain"], excluded=True, tau=0.7)


@pytest.mark.parametrize("kw", [dict(), dict(tau=0.7, excluded=True)], ids=["plain", "tau_excluded"])
def test_model_bf16(hip, trie_head, kw):
    tl.model_case(hip, TINY, ITEMS["plain"], dtype="bf16", **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampler_logprobs_are_the_trainer_nll(hip, trie_head, dtype):
    tl.sampler_case(hip, TINY, ITEMS["plain"], 3, 14, 4, dtype=dtype, tau=0.7, excluded=True)


def test_sampler_logprobs_unequal_items(hip, trie_head):
    tl.sampler_case(hip, TINY, ITEMS["unequal"], 2, 12, 4, batch_seed=11, tag=" unequal")


def test_slate_logprobs_are_the_trainer_nll(hip, trie_head):
    tl.slates_case(hip, TINY, ITEMS["plain"])


def test_subset_normalisation_and_single_children(hip, trie_head):
    tl.subset_case(hip, TINY, ITEMS["plain"])


@pytest.mark.parametrize("dtype,dropout", [("fp32", 0.0), ("fp32", 0.1), ("bf16", 0.0)])
def test_loss_and_backward_equals_forward_and_autograd(hip, trie_head, dtype, dropout):
    tl.fused_case(hip, TINY, ITEMS["plain"], dtype=dtype, dropout=dropout)


def test_second_micro_batch_accumulates(hip, trie_head):
    tl.accumulation_case(hip, TINY, ITEMS["plain"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_is_bit_reproducible(hip, trie_head, dtype):
    tl.reproducible_case(hip, TINY, ITEMS["plain"], dtype=dtype)


def test_errors(hip, trie_head):
    tl.errors_case(hip, TINY)


def test_runner_item_loss_head_flag(hip, tmp_path):
    th.runner_case(hip, str(tmp_path))


@pytest.mark.parametrize("top_k,top_p,dropout,tau,excluded", [(2, 1.0, 0.0, 1.0, False), (0, 0.5, 0.0, 1.0, False), (3, 0.8, 0.1, 0.7, True)],
                         ids=["top_k", "top_p", "both_dropout_tau_excluded"])
def test_truncated_model(hip, trie_head, top_k, top_p, dropout, tau, excluded):
    tc.model_case(hip, TINY, ITEMS["plain"], top_k=top_k, top_p=top_p, dropout=dropout, tau=tau, excluded=excluded)


def test_truncated_loss_and_backward_equals_forward_and_autograd(hip, trie_head):
    tc.fused_case(hip, TINY, ITEMS["plain"])


def test_truncated_backward_is_bit_reproducible(hip, trie_head):
    tc.reproducible_case(hip, TINY, ITEMS["plain"])


# ---- route against route ----
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_restricted_route_against_dense(hip, dtype):
    th.routes_case(hip, TINY, ITEMS["plain"], dtype=dtype)


def test_restricted_route_against_dense_truncated(hip):
    th.routes_case(hip, TINY, ITEMS["plain"], dtype="fp32", temperature=0.7, top_p=0.995, tag=" truncated")


@pytest.mark.parametrize("staged", [False, True], ids=["whole", "staged"])
def test_grouped_storing_path(hip, staged):
    th.storing_case(hip, TINY, ITEMS["plain"], staged=staged)


def test_kernels_of_the_restricted_step(hip):
    th.profile_case(hip, TINY, ITEMS["plain"])


def test_item_head_workspace_bytes_are_exact(hip):
    th.workspace_case(hip, TINY, ITEMS["plain"])


def test_train_workspace_bytes_unchanged(hip, trie_head):
    tl.workspace_case(hip, TINY, ITEMS["plain"])


# ---- T5-small width: d = 512, V = 32100, the benchmark's 3,416-item trie (Nu = 1,006); B = 8, L = 64, T = 8: Md = 64, the plan runs ----
@pytest.fixture(scope="module")
def ml1m():
    import bench
    from openp5_amd.trie import CompiledTrie
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    items = ct.enumerate_items()
    ct.index_items(items)
    assert len(ct.head_columns()[0]) == 1006
    ocfg = O.T5Cfg.named("t5-small")
    return ct, items, ocfg, O.init_params(ocfg, 7)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_routes_t5_small(hip, ml1m, dtype):
    ct, items, ocfg, params = ml1m
    th.routes_case(hip, ocfg, items, dtype=dtype, B=8, L=64, T=8, ct=ct, params=params, tag=" t5-small")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_reproducible_t5_small(hip, ml1m, dtype):
    """three restricted steps on fresh models (the first backward of a model stores): the loss and every gradient bit-identical"""
    ct, items, ocfg, params = ml1m
    batch = tl.item_batch(ocfg, items, 8, 64, 8, 3, stray=False)[:5]
    outs = []
    for _ in range(3):
        m = th.cases.build_model(hip, ocfg, params, dtype, 0.1)
        tl._train_mode(m, 0.1, 41)
        outs.append(th._fused(hip, m, batch, ct, temperature=0.7, item_head="trie"))
        del m
    assert float(outs[0][1].abs().max()) > 0
    for r in (1, 2):
        assert outs[r][0] == outs[0][0] and torch.equal(outs[r][1], outs[0][1]), (r, float((outs[r][1] - outs[0][1]).abs().max()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampler_logprobs_ml1m_shaped_catalogue_t5_small(hip, trie_head, ml1m, dtype):
    ct, items, ocfg, _ = ml1m
    tl.sampler_case(hip, ocfg, items, 2, 32, 2, dtype=dtype, ct=ct, tag=" ml1m")
