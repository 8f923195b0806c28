"""The weight-gradient plan of the whole backward (option wgrad_fill, p5_lib.hip wgrad_plan_flush): the tied head's, the decoder layers'
and the cross-attention K/V block's weight gradients ride as FILLER units in the short workgroups of the encoder's two-layer launches
(p5_gemm5_kernel<true>, P5GemmGroupFill in p5_gemm4.h).  Only which problems share a launch changes -- every tile keeps its whole K range
and its one writer -- so every gradient must equal the unplanned backward's (wgrad_fill 0).

Token counts are tiny (B=8, L=64 -> M=512; T=8 -> Md=64, one K-step per decoder filler): the unit counts come from the weight shapes."""
import ctypes
import json
import os

import pytest
import torch

from oracle import t5_oracle as O
from tests import cases

SHAPE = (8, 64, 8)      # B, L, T
SMALL = dict(d_model=512, d_ff=2048, num_heads=8)
BASE = dict(d_model=768, d_ff=3072, num_heads=12)
FILL_TAG = "KS: grouped weight gradients + fillers"


def _cfg(dims, n_enc, n_dec, **kw):
    return O.T5Cfg(**{**dims, "num_layers": n_enc, "num_decoder_layers": n_dec, "vocab_size": 1000, **kw})


def _set(be, opts):
    for k, v in opts.items():
        be.check(be.lib.p5_set_option(k.encode(), v), f"p5_set_option {k}")


# what the library starts with (p5_lib.hip: the environment variable, else the built-in default) -- the values in force outside these tests
_START = {"wgrad_fill": ("P5_WGRAD_FILL", 1), "wgrad_wgs": ("P5_WGRAD_WGS", 0), "wgrad_wide_min": ("P5_WGRAD_WIDE_MIN", 160),
          "embed_det": ("P5_EMBED_DET", 1)}


def _in_force(names):
    return {k: int(os.environ.get(_START[k][0], _START[k][1])) for k in names}


def _backward(be, ocfg, fill, opts=None, dropout=0.1, passes=1, poison=False, profile=False, shape=SHAPE, batches=None):
    """`passes` backward passes of one accumulation group on a fresh model under wgrad_fill = `fill`; -> (loss, gradient arena, views,
    profiler keys).  Every option it sets goes back to the value that was in force, whatever happens."""
    params = O.init_params(ocfg, 7)
    if batches is None:
        batches = [cases.synth_batch(ocfg, *shape, 3 + k) for k in range(passes)]
    keys, profiling = [], False
    opts = {"wgrad_fill": fill, **(opts or {})}
    try:
        _set(be, opts)
        m = cases.build_model(be, ocfg, params, "bf16", dropout)
        if dropout > 0:
            m.train()
            m.set_dropout_seed(41, 5)
        else:
            m.eval()
        if poison:      # the arena is dead after zero_grad(): NaN in every element the backward does not write itself
            m.zero_grad()
            cases.sync(be)
            m._grads.fill_(float("nan"))
        if profile:
            be.check(be.lib.p5_profile_begin(), "p5_profile_begin")
            profiling = True
        for k, b in enumerate(batches):
            m.begin_micro_batch(first=k == 0, sync=False)
            loss = m.loss_and_backward(*b)
        cases.sync(be)
        if profile:
            buf = ctypes.create_string_buffer(1 << 16)
            be.check(be.lib.p5_profile_end(buf, len(buf)), "p5_profile_end")
            profiling = False
            keys = [e["kernel"] for e in json.loads(buf.value.decode())]
        return float(loss), m._grads.detach().cpu().clone(), dict(m._views), keys
    finally:
        if profiling:
            be.lib.p5_profile_end(None, 0)
        _set(be, _in_force(opts))


def _assert_same(got, want, views, what):
    bad = [(n, float((got[o:o + k] - want[o:o + k]).abs().max())) for n, (o, k, _) in views.items() if not torch.equal(got[o:o + k], want[o:o + k])]
    assert not bad, (what, bad[:8], len(bad))


def _filled(keys):
    return [k for k in keys if f"[{FILL_TAG}]" in k]


def plan_equals_no_plan_case(be, ocfg, passes=1, expect_fill=True, opts=None, **kw):
    """Every gradient tensor under the plan is bit-identical to the unplanned backward's: the tensors that stay on the same kernel
    instance and tile shape (encoder layers grouped in pairs either way, the K/V block) by construction, and the ones that move from
    128x128 tiles to filler units of 256x128 (decoder layers, head, a bottom encoder layer that now leaves in a pair) because both kernels
    walk K upward in 64-steps through the same MFMA, one accumulator per element -- torch.equal holds for all of them, so no bound is needed.
    (Measured on MI355X: equal everywhere on a first micro-batch; on an accumulating one the tied head's gradient, the only one with
    alpha != 1, first differed by one ulp, 7.5e-9 -- "c + acc * alpha" was an FMA in one kernel and a multiply and an add in the other.  The
    epilogues now round acc * alpha before the add (p5_mul_rn), and the accumulating case is equal too.)"""
    l1, g1, views, keys = _backward(be, ocfg, 1, passes=passes, profile=True, opts=opts, **kw)
    l0, g0, _, keys0 = _backward(be, ocfg, 0, passes=passes, profile=True, opts=opts, **kw)
    assert not _filled(keys0), keys0
    assert bool(_filled(keys)) == expect_fill, keys
    assert l1 == l0
    assert float(g0.abs().max()) > 0
    _assert_same(g1, g0, views, "wgrad_fill 1 vs 0")


def fully_written_case(be, ocfg, opts, **kw):
    l1, g1, views, keys = _backward(be, ocfg, 1, opts=opts, poison=True, profile=True, **kw)
    assert _filled(keys), keys
    for n, (o, k, _) in views.items():
        assert not bool(torch.isnan(g1[o:o + k]).any()), f"{n}: gradient not (fully) written under the weight-gradient plan"
    l0, g0, _, _ = _backward(be, ocfg, 0, opts=opts, poison=True, **kw)
    assert l1 == l0
    _assert_same(g1, g0, views, "wgrad_fill 1 vs 0 over a poisoned arena")


# (encoder layers, decoder layers, a filled launch is expected): 2 + 2 = one pair carrying everything; 3 + 1 = a pair, then the bottom layer
# alone on its own route with the pool's rest behind it; 1 + 1 = no pair at all, the pool leaves as ordinary launches
LAYERS = [(2, 2, True), (3, 1, True), (1, 1, False)]
# T5-base dims, 2 + 1 layers: 432 primary units = the 80 workgroups that sit out the second round are the short ones; d_ff = 2944 makes it
# 426 units (ragged XCD ranges: 54 x 7 + 48); 8 workgroups = every one loops over many primaries, then fillers
BASE_CASES = [(3072, 0), (2944, 0), (2944, 8), (3072, 8)]


# ---- the emulator runs the same kernel and the same plan, but a T5-small-sized step takes it a minute: the not-gpu suite checks the dealing
# on d_model = 128 weights (9 units per encoder layer; wgrad_wide_min 1 puts the pair on the 256x128 instance), where 18 primary units on 24
# workgroups leave XCDs 6 and 7 without primaries (ragged ranges, every workgroup of those XCDs short) and 8 workgroups make every one loop
# over primaries and fillers.  The model-sized cases below run on the GPU.
TINY = dict(d_model=128, d_ff=512, num_heads=2)


@pytest.mark.parametrize("n_enc,n_dec,wgs,passes", [(2, 2, 0, 1), (3, 1, 8, 1), (2, 1, 0, 2)])
def test_plan_equals_no_plan_tiny_weights(emu, n_enc, n_dec, wgs, passes):
    ocfg = _cfg(TINY, n_enc, n_dec, vocab_size=300)
    plan_equals_no_plan_case(emu, ocfg, passes=passes, opts={"wgrad_wide_min": 1, "wgrad_wgs": wgs}, shape=(2, 32, 32))
    fully_written_case(emu, ocfg, {"wgrad_wide_min": 1, "wgrad_wgs": wgs}, shape=(2, 32, 32))


# ---- embed_det 0: the atomic embedding scatter adds the decoder's rows into shared.weight's gradient in the stage behind the decoder --
# before the encoder's launches, where the plan would store the tied head's gradient over them.  The plan must stand back: wgrad_fill 1
# launches what wgrad_fill 0 launches, and every tensor is equal.
# Atomic adds land in no fixed order, so the comparison is exact only where the order cannot matter: one sequence whose encoder and
# decoder token ids and whole-word ids are all different (the decoder's start token 0 included) -- every row of the two embedding tables
# then receives at most ONE atomic add on top of what was stored or cleared there, a sum of two terms.
def _unique_id_batch(ocfg, L, T, seed):
    g = torch.Generator().manual_seed(seed)
    perm = 3 + torch.randperm(ocfg.vocab_size - 3, generator=g)[:L + T]
    ids, labels = perm[:L].reshape(1, L), perm[L:].reshape(1, T).clone()
    labels[0, T - 1] = ocfg.eos_id
    assert len(set(ids.flatten().tolist()) | set(labels.flatten().tolist()) | {0}) == L + T + 1
    ww = torch.arange(1, L + 1).reshape(1, L)
    return ids, ww, torch.ones(1, L, dtype=torch.long), labels, torch.ones(1, T, dtype=torch.long)


def atomic_scatter_case(be, ocfg, opts=None):
    L = T = 64      # M = Md = 64: every weight gradient on the grouped path
    batches = [_unique_id_batch(ocfg, L, T, 11)]
    opts = {"embed_det": 0, **(opts or {})}
    l1, g1, views, keys1 = _backward(be, ocfg, 1, opts=opts, profile=True, shape=(1, L, T), batches=batches)
    l0, g0, _, keys0 = _backward(be, ocfg, 0, opts=opts, profile=True, shape=(1, L, T), batches=batches)
    assert not _filled(keys1), keys1
    assert keys1 == keys0
    assert l1 == l0
    _assert_same(g1, g0, views, "wgrad_fill 1 vs 0 under embed_det 0")
    # and the same gradients as the segmented sums (no plan either way: the same launches but the embedding kernels; two-term sums)
    ld, gd, _, _ = _backward(be, ocfg, 0, opts={**opts, "embed_det": 1}, shape=(1, L, T), batches=batches)
    assert ld == l0
    _assert_same(g0, gd, views, "embed_det 0 vs 1, wgrad_fill 0")


def test_plan_stands_back_for_the_atomic_scatter_tiny_weights(emu):
    atomic_scatter_case(emu, _cfg(TINY, 2, 2, vocab_size=300), {"wgrad_wide_min": 1})


@pytest.mark.gpu
def test_gpu_plan_stands_back_for_the_atomic_scatter(hip):
    atomic_scatter_case(hip, _cfg(SMALL, 2, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("n_enc,n_dec,filled", LAYERS)
def test_gpu_plan_equals_no_plan_per_tensor(hip, n_enc, n_dec, filled):
    plan_equals_no_plan_case(hip, _cfg(SMALL, n_enc, n_dec), expect_fill=filled)


@pytest.mark.gpu
@pytest.mark.parametrize("d_ff,wgs", BASE_CASES)
def test_gpu_no_short_workgroups_and_ragged_xcd_ranges(hip, d_ff, wgs):
    fully_written_case(hip, _cfg({**BASE, "d_ff": d_ff}, 2, 1), {"wgrad_wgs": wgs})


@pytest.mark.gpu
def test_gpu_accumulation_micro_batch(hip):
    plan_equals_no_plan_case(hip, _cfg(SMALL, 2, 2), passes=2)


@pytest.mark.gpu
def test_gpu_twice_the_same_bits(hip):
    ocfg = _cfg(SMALL, 2, 2)
    la, ga, views, keys = _backward(hip, ocfg, 1, profile=True)
    lb, gb, _, _ = _backward(hip, ocfg, 1)
    assert _filled(keys), keys
    assert la == lb
    _assert_same(ga, gb, views, "two runs of the same step")
