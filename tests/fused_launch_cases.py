"""Launches the training step no longer needs, each behind one p5_set_option switch (default on):
  shift_fuse   the decoder's embedding lookup shifts the labels itself (no p5_shift_right_kernel launch; e->dec_ids is still written)
  loss_fuse    the loss kernel of p5_forward_loss* also writes the NLL gradients (no p5_ce_gscale_kernel launch in the backward)
Off against on, every gradient tensor of one backward -- the whole one and the staged one -- must be the same bits (the helper pattern of
tests/test_wgrad_fill.py), and the merged loss kernel by itself must give the bits of the loss kernel plus the stand-alone scale kernel."""
import ctypes
import json
import os

import torch

from oracle import t5_oracle as O
from tests import cases
from tests.cases import P, dev, sync

TINY = dict(d_model=128, d_ff=512, num_heads=2)
# option -> (environment variable the library starts from, built-in default, kernel whose launch the option removes)
OPTIONS = {"shift_fuse": ("P5_SHIFT_FUSE", 1, "p5_shift_right_kernel"), "loss_fuse": ("P5_LOSS_FUSE", 1, "p5_ce_gscale_kernel")}
_START = {**{k: v[:2] for k, v in OPTIONS.items()}, "gemm_wide_min_tiles": ("P5_GEMM_WIDE_MIN_TILES", 160)}
SHAPES = [(2, 17, 3), (2, 64, 3)]      # B, L, T


def _set(be, opts):
    for k, v in opts.items():
        be.check(be.lib.p5_set_option(k.encode(), v), f"p5_set_option {k}")


def _batch(ocfg, B, L, T):
    ids, ww, mask, labels, out_attn = cases.synth_batch(ocfg, B, L, T, 3)
    labels = labels.clone()
    labels[0][out_attn[0] == 0] = -100      # ignored labels: the start token on their right, no gradient
    if not bool((labels == -100).any()):
        labels[0, T - 1], out_attn[0, T - 1] = -100, 0
    return ids, ww, mask, labels, out_attn


def _backward(be, ocfg, opts, shape, staged, dropout=0.1):
    """one backward on a fresh model under `opts`; -> (loss, gradient arena, views, launched kernels).  gemm_wide_min_tiles 1 puts the toy
    head on the logit-free route, the one whose backward takes its NLL gradients from ce_g."""
    opts = {**opts, "gemm_wide_min_tiles": 1}
    profiling = False
    try:
        _set(be, opts)
        m = cases.build_model(be, ocfg, O.init_params(ocfg, 7), "bf16", dropout)
        m.train()
        m.set_dropout_seed(41, 5)
        m.staged_backward = staged
        be.check(be.lib.p5_profile_begin(), "p5_profile_begin")
        profiling = True
        m.begin_micro_batch(first=True, sync=False)
        loss = m.loss_and_backward(*_batch(ocfg, *shape))
        sync(be)
        buf = ctypes.create_string_buffer(1 << 16)
        be.check(be.lib.p5_profile_end(buf, len(buf)), "p5_profile_end")
        profiling = False
        keys = [e["kernel"] for e in json.loads(buf.value.decode())]
        return float(loss), m._grads.detach().cpu().clone(), dict(m._views), keys
    finally:
        if profiling:
            be.lib.p5_profile_end(None, 0)
        _set(be, {k: int(os.environ.get(_START[k][0], _START[k][1])) for k in opts})


def option_case(be, name, shape, staged):
    ocfg = O.T5Cfg(**{**TINY, "num_layers": 1, "num_decoder_layers": 1, "vocab_size": 300})
    kernel = OPTIONS[name][2]
    l1, g1, views, keys1 = _backward(be, ocfg, {name: 1}, shape, staged)
    l0, g0, _, keys0 = _backward(be, ocfg, {name: 0}, shape, staged)
    assert any(kernel in k for k in keys0), (name, "off: the launch it removes must be there", keys0)
    assert not any(kernel in k for k in keys1), (name, "on: the launch is still there", keys1)
    assert l1 == l0
    assert float(g0.abs().max()) > 0
    bad = [(n, float((g1[o:o + k] - g0[o:o + k]).abs().max())) for n, (o, k, _) in views.items() if not torch.equal(g1[o:o + k], g0[o:o + k])]
    assert not bad, (f"{name} 1 vs 0", bad[:8], len(bad))


# B, T, groups per user (tw has B entries: the B x G samples of p5_forward_loss_targets are its batch rows)
LOSS_SHAPES = [(1, 1, 1), (3, 5, 1), (64, 8, 1), (6, 5, 2)]


def merged_loss_case(be, B, T, G, seed=0):
    """p5_masked_mean_g_kernel (merged 1) against p5_masked_mean_kernel + p5_ce_gscale_kernel (merged 0): loss and g the same bits.  One
    mask row is all zero (count 0 -> divided by 1), one label is ignored; G = 2 carries a zero and a negative weight."""
    g = torch.Generator().manual_seed(seed + 5 * B + T)
    nll = (torch.rand(B, T, generator=g) * 9).float()
    mask = (torch.rand(B, T, generator=g) < 0.7).long()
    mask[:, 0] = 1
    mask[B // 2] = 0
    labels = torch.randint(3, 300, (B, T), generator=g)
    labels[B - 1, T - 1] = -100
    tw = None
    if G > 1:
        tw = torch.rand(B, generator=g).float() + 0.25
        tw[0], tw[1] = 0.0, -1.5
    nd, ad, ld, twd = dev(be, nll), dev(be, mask), dev(be, labels), dev(be, tw) if tw is not None else None
    out = {}
    for merged in (1, 0):
        loss = dev(be, torch.full((1,), float("nan")))
        gout = dev(be, torch.full((B * T + 4,), float("nan")))
        be.check(be.lib.p5_op_masked_mean_g(merged, P(loss), P(gout), P(nd), P(ad), P(ld), P(twd), B, T, 1.0 / B, be.stream_ptr()), f"masked_mean_g {merged}")
        sync(be)
        out[merged] = (loss.cpu(), gout.cpu())
    (l1, g1), (l0, g0) = out[1], out[0]
    assert bool(torch.isnan(g1[B * T:]).all()), "g written past B * T"
    assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(g0[:B * T]).all())
    assert cases._same_bits(l1, l0), (float(l1), float(l0))
    assert cases._same_bits(g1[:B * T], g0[:B * T]), int((g1[:B * T] != g0[:B * T]).sum())
    gg = g0[:B * T].view(B, T)
    assert float(gg[B // 2].abs().max()) == 0 and float(gg[B - 1, T - 1]) == 0
    if B > 1:
        assert float(gg.abs().max()) > 0
