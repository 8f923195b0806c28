"""`P5T5Native` -- drop-in for OpenP5's `P5_T5` model object (/root/reference/src/src_t5/model/P5_T5.py:207)
backed by the HIP engine in libp5hip.so.

It satisfies exactly the uses the reference's launcher/runner make of the model:
  * `forward(input_ids, whole_word_ids, attention_mask, labels, alpha=..., return_dict=True)["loss"]` is the flat
    [B*T] fp32 per-token NLL (P5_T5.py:368-369, consumed at DistributedRunner.py:63-77), differentiable;
  * `generate(input_ids, attention_mask, whole_word_ids, max_length, prefix_allowed_tokens_fn, num_beams,
    num_return_sequences, output_scores, return_dict_in_generate)` -> {"sequences", "sequences_scores"}
    (DistributedRunner.py:361-374);
  * `nn.Module` protocol with HF T5 state-dict keys incl. the duplicated tied keys;
    `shared.weight` is the single tied [V, d] tensor, writable in place (utils/initialization.py:27-29);
  * `resize_token_embeddings(n)` (main.py:193), `.train()/.eval()/.zero_grad()/.parameters()`.

All parameters are views into ONE flat fp32 arena (and all gradients views into a second arena of the same
layout), which is what lets clip + AdamW be two flat kernels and the data-parallel all-reduce a handful of
contiguous buckets issued while the backward is still running.
"""
from __future__ import annotations

import contextlib
import warnings
import os
import copy
import ctypes
import threading
import math
import types
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _abi
from .trie import CompiledTrie, Trie, find_trie


@dataclass
class P5ModelConfig:
    """The T5Config fields the path reads (HF configuration_t5.py:44-62 defaults = t5-small)."""
    vocab_size: int = 32128
    d_model: int = 512
    d_kv: int = 64
    d_ff: int = 2048
    num_layers: int = 6
    num_decoder_layers: Optional[int] = None
    num_heads: int = 8
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    dropout_rate: float = 0.1
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "relu"
    whole_word_size: int = 512           # P5_T5.py:64
    pad_token_id: int = 0
    eos_token_id: int = 1
    decoder_start_token_id: int = 0

    @staticmethod
    def from_backbone(name: str, **kw) -> "P5ModelConfig":
        presets = {
            "t5-small": dict(d_model=512, d_ff=2048, num_heads=8, num_layers=6),
            "t5-base": dict(d_model=768, d_ff=3072, num_heads=12, num_layers=12),
            "t5-large": dict(d_model=1024, d_ff=4096, num_heads=16, num_layers=24),
        }
        key = name.split("/")[-1]
        if key not in presets:
            raise ValueError(f"unknown backbone {name!r} (known: {sorted(presets)})")
        d = dict(presets[key])
        d.update(kw)
        return P5ModelConfig(**d)

    @staticmethod
    def from_hf(cfg) -> "P5ModelConfig":
        g = lambda k, dflt=None: getattr(cfg, k, dflt)
        return P5ModelConfig(
            vocab_size=g("vocab_size"), d_model=g("d_model"), d_kv=g("d_kv"), d_ff=g("d_ff"), num_layers=g("num_layers"),
            num_decoder_layers=g("num_decoder_layers"), num_heads=g("num_heads"),
            relative_attention_num_buckets=g("relative_attention_num_buckets", 32),
            relative_attention_max_distance=g("relative_attention_max_distance", 128),
            dropout_rate=g("dropout_rate", 0.1), layer_norm_epsilon=g("layer_norm_epsilon", 1e-6),
            feed_forward_proj=g("feed_forward_proj", "relu"), pad_token_id=g("pad_token_id", 0) or 0,
            eos_token_id=g("eos_token_id", 1), decoder_start_token_id=g("decoder_start_token_id", 0) or 0)


def relative_position_bucket_lut(half: int, bidirectional: bool, num_buckets: int, max_distance: int) -> torch.Tensor:
    """bucket(rel) for rel = key_pos - query_pos in [-half, half]; same op sequence (fp32 log, truncation) as
    HF modeling_t5.py:217-262 so the table is bit-identical to what T5Attention.compute_bias indexes with."""
    rel = torch.arange(-half, half + 1, dtype=torch.long)
    ret = torch.zeros_like(rel)
    nb = num_buckets
    if bidirectional:
        nb //= 2
        ret = ret + (rel > 0).to(torch.long) * nb
        rel = torch.abs(rel)
    else:
        rel = -torch.min(rel, torch.zeros_like(rel))
    max_exact = nb // 2
    is_small = rel < max_exact
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return (ret + torch.where(is_small, rel, large)).to(torch.int32)


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _P5LossFn(torch.autograd.Function):
    """autograd seam: forward = p5_forward (activations stay in the engine workspace), backward = p5_backward
    writing straight into the gradient arena."""

    @staticmethod
    def forward(ctx, anchor, model, input_ids, whole_word_ids, attention_mask, labels, item_loss=None):
        ctx.model = model
        ctx.item_loss = item_loss       # (the engine keeps the setting of its last forward for the backward; this keeps the device arrays alive)
        return model._engine_forward(input_ids, whole_word_ids, attention_mask, labels, item_loss)

    @staticmethod
    def backward(ctx, dnll):
        ctx.model._engine_backward(dnll)
        return None, None, None, None, None, None, None


class _P5RegLossFn(torch.autograd.Function):
    """The seam of the regularised item loss (csrc/p5_trie_reg.h): three per-row outputs -- NLL, entropy, KL to the reference -- and ONE engine
    backward that receives the three per-row gradients.  Without reference logits the third output is zeros and carries no gradient."""

    @staticmethod
    def forward(ctx, anchor, model, input_ids, whole_word_ids, attention_mask, labels, item_loss):
        ctx.model = model
        ctx.item_loss = item_loss
        nll = model._engine_forward(input_ids, whole_word_ids, attention_mask, labels, item_loss)
        rows = nll.numel()
        ent = item_loss.row_terms[:rows]
        if item_loss.ref is None:
            kl = torch.zeros_like(nll)
            ctx.mark_non_differentiable(kl)
        else:
            kl = item_loss.row_terms[rows:2 * rows]
        return nll, ent, kl

    @staticmethod
    def backward(ctx, dnll, dent, dkl):
        ctx.model._engine_backward(dnll, dent, dkl if ctx.item_loss.ref is not None else None)
        return None, None, None, None, None, None, None


class _GenLane:
    """What ONE in-flight generate() call owns: its engines (the bf16 / fp32 search engine and, for verified generation, the fp32 verification
    engine -- all bound to the model's ONE set of parameter arenas), its workspaces, its pinned read-back buffer, its HIP stream.  Lane 0 is
    the model's own engine on the caller's stream; further lanes let several batches be in flight at once (`P5T5Native.map_lanes`)."""
    __slots__ = ("idx", "engine", "engine_v", "ws", "ver_hdr", "forced", "stream")

    def __init__(self, idx, engine, stream=None):
        self.idx, self.engine, self.stream = idx, engine, stream
        self.engine_v, self.ver_hdr = None, None
        self.ws, self.forced = {}, ([], [])


class P5T5Native(nn.Module):
    LUT_HALF = 512
    # Engine-internal second HIP stream (weight gradients, K/V projections, clears off the main stream).  OFF since round 3: with
    # the layer-grouped weight-gradient launches every phase of the encoder backward fills the GPU from ONE stream, and the ~50
    # cross-stream event waits per step cost more than the overlap returns (MI355X, C2 step: 4.74 ms without, 5.07-5.4 ms with).
    # Data-parallel gradient exchange uses its own communication stream either way (`_engine_backward`).
    use_side_stream = False
    use_transposed_weights = True     # bf16: keep W^T of the layer weights for the data gradients (p5_engine_bind_transposed)
    # generate() of a bf16 model: "verified" = the bf16 search (with `verify_extra_beams` more beams) proposes, one fp32 pass decides -- the
    # returned lists and scores are the fp32 search's (include/p5hip.h, csrc/p5_verify.h); "draft" = the plain bf16 search.  An fp32 model
    # always runs the plain (fp32) search.
    generation_mode = "verified"
    verify_extra_beams = 6
    VERIFY_MAX_K = 22             # the replay's candidate pool (K x 2K <= 1024 entries of LDS, csrc/p5_verify.h)
    VERIFY_MAX_ROWS = 512         # rows per user of the fp32 pass = queries per (user, head) of its cross-attention launch
    verify_escalation = (22,)     # extra beams of the wider draft a FLAGGED user gets before the plain fp32 search is the last resort
    verify_share_encoder = True   # verified mode: the draft starts from the verification pass's fp32 encoder output (one encoder pass per batch)
    gen_lanes = 3                 # batches in flight in `map_lanes` (the runner's evaluation loops, bench.py): lanes overlap each other's latency-bound chains
    prefix_fast_forward = True    # the steps every item shares ("<dataset> item _") as one teacher-forced pass (p5_generate_set_forced_prefix)
    NARROW_MAX_K = 64             # widest search of the narrow beam step (csrc/p5_decode.h); up to WIDE_MAX_K beams run the wide one (p5_decode_wide.h)
    WIDE_MAX_K = 4096
    rank_max_bytes = 4 << 30      # rank_items(): users per pass are as many as fit a workspace of this many bytes (p5_rank_workspace_bytes)
    wide_max_rows = 4096          # a wide search (K > 64) runs over at most this many decode rows (users x beams) per call: larger batches go in user
                                  # chunks (the step KV cache alone is n_dec_layers x max_len x rows x 2 x inner x sizeof(T): ~3 GiB for fp32
                                  # T5-small at max_len 30)
    # head of the trie-normalised item loss (forward(trie=...)): "dense" = over the whole vocabulary; "trie" = over the distinct tokens of the
    # trie's edges only (csrc/p5_item_head.h: no [B*T, V] logits, the tied head's three GEMMs shrink to the trie's token set)
    item_head = "dense"

    def __init__(self, config, dtype: str = "bf16", device=None, backend=None, seed: int = 2023):
        super().__init__()
        if not isinstance(config, P5ModelConfig):
            config = P5ModelConfig.from_hf(config)
        if config.num_decoder_layers is None:
            config.num_decoder_layers = config.num_layers
        self.config = config
        if backend is None:
            from ._lib import hip_backend
            backend = hip_backend(device)
        self._be = backend
        self._lib = backend.lib
        self.compute_dtype = {"bf16": 1, "bfloat16": 1, "fp32": 0, "float32": 0}[str(dtype).replace("torch.", "")]
        self._engine = ctypes.c_void_p()
        self._ws = None
        self._gen_ws = None
        self._anchor = torch.zeros(1, device=backend.device, requires_grad=True)
        self.ddp_world = 1          # set by the runner: gradient all-reduce across ranks during backward
        self.ddp_group = None
        self._ddp_sync = True       # False on all but the last micro-batch of a gradient-accumulation group
        self.ddp_bucket_dtype = "fp32"   # "bf16": gradient buckets travel as bf16 (half the bytes on the xGMI links)
        self.staged_backward = False     # run the stage-by-stage backward (the data-parallel code path) even at world size 1, without collectives
        self.ddp_lazy_wait = True        # gradient buckets are waited for at their first use (the optimizer step), not at the end of the backward
        self._pending_half = False
        self.ddp_timing = False          # record device time the main stream spends waiting for the gradient exchange (bench.py)
        self.ddp_wait_ms = []
        self._pending = []
        self._staged_ranges, self._bucket16 = None, None
        self._side = None
        self._comm = None
        self._lanes = []            # generation lanes (lane 0 = this model's engine on the caller's stream)
        self._tls = threading.local()
        self._stats_lock = threading.Lock()
        self.verify_stats = {"calls": 0, "users": 0, "escalated_users": 0, "fallback_users": 0, "rows": 0, "rows_per_user_max": 0, "draft_beams": 0,
                             "wide_fp32_users": 0}
        self.last_item_loss_terms = None    # fp32 [3] device tensor (L_nll, R_H, R_KL) of the last loss_and_backward if it was regularised, else None
        self.last_item_loss_state = None    # int32 [B, T] device tensor of the last item-loss forward (forward(trie=...)): 0 scored, 1 past the end, 2 off the trie, 3 truncated away
        self.last_generate_path = None      # "verified" | "fp32_search" | "draft_bf16": which search the most recent generate() call ran ("sample": sample_items() / generate(do_sample=True); "slates": sample_slates(); "rank_fp32" | "rank_bf16": rank_items(); "cand_fp32" | "cand_bf16": score_candidates())
        self.rank_stats = {"calls": 0, "users": 0, "rescored_users": 0, "users_per_pass": 0, "rows_per_user": 0,
                           "pruned_calls": 0, "certified_users": 0, "fallback_users": 0, "declined_users": 0, "kept_rows_per_user": 0,
                           "search_calls": 0, "search_certified_users": 0, "search_fallback_users": 0, "search_declined_users": 0,
                           "search_rounds": 0, "search_rows_per_user": 0}
        # rank_items(pruned=True), csrc/p5_prune.h.  slack: how far below the bf16 N-th score a prefix's bound may lie and still get fp32
        # numbers (3 x the bf16 score tolerance 0.04: one on the threshold, one on the bound, one of headroom); margin: the certificate's
        # (the tolerance fp32 scores are held to at T5-small width); max_fraction: above this share of the trie's rows the proposal is
        # declined and the full fp32 pass runs instead.  0.6 is the measured break-even (profiles/rank_pruned.jsonl, T5-small, 3416 items,
        # 8 users: bf16 pass 1.19 ms per user, full fp32 pass 3.86, pruned call 2.73 at a kept share of 0.36 and 4.70 at 0.81): up to a
        # share of 0.62 the whole pruned call, bf16 pass included, costs less than the full fp32 pass alone, and the fp32 work still to do
        # at 0.6 (2.6 ms) leaves room for a third of the users falling back before declining would have been cheaper.
        # slack and max_fraction change cost and the fallback share, never a returned list.
        self.rank_prune_slack = 0.12
        self.rank_prune_margin = 1e-4
        self.rank_prune_max_fraction = 0.6
        self._prune_sabotage = None         # test hook: called as _prune_sabotage(sel [nb, rows], n_rows [nb]) between propose and decide
        # rank_items(pruned="search"), csrc/p5_bound.h.  The certificate's margin is rank_prune_margin.  max_fraction: when a user's set of
        # scored rows outgrows this share of the trie's rows the chunk is declined and the full pass runs instead.  0.1 is the largest share
        # at which the search was still measured faster than the full fp32 pass, rounded down to one decimal (profiles/rank_search.jsonl,
        # T5-small, 8 users: at a share of 0.13 of the 12101-item trie's rows 6.71 ms per user against 11.3 for the full pass; at 0.30 of the
        # 3416-item trie's 5.32 against 3.84 -- every round re-runs the cumulative row set).
        # seed_beams: width of the beam search that proposes the seeds (None: top_n).  Both change cost and the fallback share, never a list.
        self.rank_search_max_fraction = 0.1
        self.rank_search_seed_beams = None
        self._search_hook = None            # test hook: _search_hook(round, sel [nb, rows], n_rows [nb]) after each round's header read; may edit sel in place
        self._search_seed_hook = None       # test hook: _search_seed_hook(seeds int64 [B, S, T]) before the search begins; may edit the sequences in place
        self.cand_stats = {"calls": 0, "users": 0, "rescored_users": 0, "users_per_pass": 0, "rows_per_user": 0}      # score_candidates()
        self.sample_stats = {"calls": 0, "users": 0, "engine_calls": 0, "rows_per_call": 0, "forced_prefix_steps": 0}      # sample_items()
        self.slate_stats = {"calls": 0, "users": 0, "engine_calls": 0, "rows_per_call": 0, "forced_prefix_steps": 0}       # sample_slates()
        self._sample_seed0 = int(seed) & 0xFFFFFFFF      # sample_items(seed=None): call n of this model draws with seed mix32(seed0 + golden * (n + 1))
        self._sample_calls = 0
        self._warned_wide_verified = False
        self._shadow_t = None       # transposed bf16 copy of the layer weights (data gradients run on the forward GEMM kernel)
        self._grads_dead = False    # zero_grad(set_to_none=True) was called and no backward has run since: `.grad` holds stale values
        self._tr_dirty = True
        self._build(seed)

    # ------------------------------------------------------------------ engine / arena plumbing
    def _cfg_struct(self):
        c = self.config
        ff = c.feed_forward_proj
        if ff not in ("relu", "gated-gelu"):
            raise ValueError(f"feed_forward_proj={ff!r} not supported (relu | gated-gelu)")
        return _abi.P5Config(
            vocab_size=c.vocab_size, d_model=c.d_model, d_kv=c.d_kv, d_ff=c.d_ff, n_enc_layers=c.num_layers,
            n_dec_layers=c.num_decoder_layers, n_heads=c.num_heads, rel_buckets=c.relative_attention_num_buckets,
            rel_max_distance=c.relative_attention_max_distance, whole_word_size=c.whole_word_size,
            gated_gelu=1 if ff == "gated-gelu" else 0, dtype=self.compute_dtype, eps=c.layer_norm_epsilon,
            dropout=c.dropout_rate, pad_id=c.pad_token_id, eos_id=c.eos_token_id)

    def _create_engine(self):
        if self._engine:
            self._lib.p5_engine_destroy(self._engine)
        self._engine = ctypes.c_void_p()
        self._drop_lanes()          # lane engines (verification engines, extra search engines) are bound to the old arena: rebuilt on demand
        cfg = self._cfg_struct()
        self._be.check(self._lib.p5_engine_create(ctypes.byref(cfg), ctypes.byref(self._engine)), "p5_engine_create")
        table = []
        name = ctypes.create_string_buffer(256)
        off, rows, cols = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
        i = 0
        while self._lib.p5_param_table(self._engine, i, name, 256, ctypes.byref(off), ctypes.byref(rows), ctypes.byref(cols)) == 0:
            table.append((name.value.decode(), off.value, rows.value, cols.value))
            i += 1
        self._table = table
        self._n = int(self._lib.p5_param_count(self._engine))

    def _build(self, seed, old_state: Optional[Dict[str, torch.Tensor]] = None):
        dev = self._be.device
        self._create_engine()
        self._flat = torch.zeros(self._n, dtype=torch.float32, device=dev)
        self._grads = torch.zeros(self._n, dtype=torch.float32, device=dev)
        self._shadow = torch.zeros(self._n, dtype=torch.bfloat16, device=dev) if self.compute_dtype == 1 else None
        c = self.config
        self._lut_enc = relative_position_bucket_lut(self.LUT_HALF, True, c.relative_attention_num_buckets, c.relative_attention_max_distance).to(dev)
        self._lut_dec = relative_position_bucket_lut(self.LUT_HALF, False, c.relative_attention_num_buckets, c.relative_attention_max_distance).to(dev)
        self._rng_cpu = [int(seed) & 0xFFFFFFFF, 0]
        self._rng = torch.tensor(self._rng_cpu, dtype=torch.int64, device=dev).to(torch.int32)
        # drop any previous parameter modules, then (re)register views with HF names
        for k in list(self._modules.keys()):
            del self._modules[k]
        self._views = {}
        for name, off, rows, cols in self._table:
            shape = (cols,) if name.endswith("layer_norm.weight") else (rows, cols)
            view = self._flat[off:off + rows * cols].view(shape)
            p = nn.Parameter(view, requires_grad=True)
            self._register_dotted(name, p)
            self._views[name] = (off, rows * cols, shape)
        self._init_weights(seed)
        if old_state is not None:
            self._copy_in(old_state, strict=False)
        self._bind()
        self._shadow_dirty = True

    def _register_dotted(self, name, p):
        parts = name.split(".")
        mod = self
        for part in parts[:-1]:
            if part not in mod._modules:
                mod.add_module(part, nn.Module())
            mod = mod._modules[part]
        mod.register_parameter(parts[-1], p)

    def _bind(self):
        self._be.check(self._lib.p5_engine_bind(self._engine, _ptr(self._flat), _ptr(self._grads), _ptr(self._shadow), _ptr(self._lut_enc),
                                                 _ptr(self._lut_dec), self.LUT_HALF, _ptr(self._rng)), "p5_engine_bind")
        if not self._be.is_emulator and self.use_side_stream:
            # weight-gradient GEMMs run on a second HIP stream, off the dgrad critical path
            if self._side is None:
                self._side = torch.cuda.Stream(device=self._be.device)
            self._lib.p5_engine_set_side_stream(self._engine, ctypes.c_void_p(self._side.cuda_stream))
        if self.compute_dtype == 1 and self.use_transposed_weights:
            nbytes = int(self._lib.p5_transposed_bytes(self._engine))
            self._shadow_t = torch.zeros(nbytes, dtype=torch.uint8, device=self._be.device)
            self._be.check(self._lib.p5_engine_bind_transposed(self._engine, _ptr(self._shadow_t), self._be.stream_ptr()), "p5_engine_bind_transposed")
            self._tr_dirty = True

    @torch.no_grad()
    def _init_weights(self, seed):
        """HF `_init_weights` std's (modeling_t5.py:563-616, factor 1.0); whole-word table N(0,1) (P5_T5.py:64-67)."""
        g = torch.Generator().manual_seed(int(seed))
        c = self.config
        d, dk, H, F = c.d_model, c.d_kv, c.num_heads, c.d_ff
        for name, p in self.named_parameters():
            if name.endswith("layer_norm.weight"):
                p.fill_(1.0)
                continue
            if name in ("shared.weight", "encoder.whole_word_embeddings.weight"):
                std = 1.0
            elif name.endswith(".q.weight"):
                std = (d * dk) ** -0.5
            elif name.endswith(".k.weight") or name.endswith(".v.weight"):
                std = d ** -0.5
            elif name.endswith(".o.weight"):
                std = (H * dk) ** -0.5
            elif ".wi" in name:
                std = d ** -0.5
            elif name.endswith(".wo.weight"):
                std = F ** -0.5
            else:
                std = d ** -0.5
            p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device))

    def _sync_shadow(self):
        if self.compute_dtype == 1 and self._shadow_dirty:
            self._be.check(self._lib.p5_refresh_shadow(self._engine, self._be.stream_ptr()), "p5_refresh_shadow")
        self._shadow_dirty = False

    def mark_params_updated(self, shadow_fresh: bool = False, copies_fresh: bool = False):
        """Call after writing parameters outside the fused optimizer (which refreshes the bf16 shadow -- and, `copies_fresh`, the transposed
        and norm-folded copies -- itself)."""
        self._shadow_dirty = not shadow_fresh
        self._tr_dirty = not (copies_fresh and shadow_fresh)

    def _sync_transposed(self):
        """W^T of the layer weights for the next backward, and W diag(ln) of the projections behind a T5LayerNorm for the next forward
        (both live in the buffer bound with p5_engine_bind_transposed; one refresh call after every parameter change)."""
        if self._shadow_t is not None and self._tr_dirty:
            self._be.check(self._lib.p5_refresh_transposed(self._engine, self._be.stream_ptr()), "p5_refresh_transposed")
            self._tr_dirty = False

    # ------------------------------------------------------------------ nn.Module protocol
    def _apply(self, fn, recurse=True):
        probe = fn(torch.zeros(1, device=self._flat.device))
        if probe.device != self._flat.device:
            if not self._be.is_emulator and probe.device.type != "cuda":
                raise RuntimeError("P5T5Native lives on the HIP device; there is no CPU path")
            if probe.device != self._be.device:
                raise RuntimeError(f"P5T5Native was built for {self._be.device}; build it with device={probe.device} instead")
        if probe.dtype != torch.float32:
            raise RuntimeError("master parameters are fp32; choose the compute dtype with dtype='bf16'|'fp32'")
        return self

    TIED = ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight")

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = super().state_dict(*args, destination=destination, prefix=prefix, keep_vars=keep_vars)
        shared = sd[prefix + "shared.weight"]
        for k in self.TIED:
            sd[prefix + k] = shared
        return sd

    @torch.no_grad()
    def _copy_in(self, state_dict, strict):
        own = dict(self.named_parameters())
        missing = [k for k in own if k not in state_dict]
        unexpected = []
        for k, v in state_dict.items():
            if k in own:
                if tuple(own[k].shape) != tuple(v.shape):
                    if k in ("shared.weight",) and v.shape[1] == own[k].shape[1]:
                        n = min(v.shape[0], own[k].shape[0])
                        own[k][:n].copy_(v[:n].to(own[k].device, torch.float32))
                        continue
                    raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)} vs {tuple(own[k].shape)}")
                own[k].copy_(v.to(own[k].device, torch.float32))
            elif k in self.TIED or k == "decoder.block.0.layer.1.EncDecAttention.relative_attention_bias.weight":
                continue   # tied duplicates / key ignored on load (P5_T5.py:213-215)
            else:
                unexpected.append(k)
        if "shared.weight" not in state_dict:
            for k in self.TIED:
                if k in state_dict:
                    own["shared.weight"].copy_(state_dict[k].to(own["shared.weight"].device, torch.float32))
                    missing = [m for m in missing if m != "shared.weight"]
                    break
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing={missing} unexpected={unexpected}")
        self._shadow_dirty = True
        self._tr_dirty = True
        return missing, unexpected

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        missing, unexpected = self._copy_in(state_dict, strict)
        from torch.nn.modules.module import _IncompatibleKeys
        return _IncompatibleKeys(missing, unexpected)

    @classmethod
    def from_pretrained(cls, backbone, config=None, state_dict=None, **kw):
        """`P5_T5.from_pretrained(args.backbone, config=config)` (main.py:176,184).  Weights come from `state_dict`
        or from a local HF checkpoint directory/file (`pytorch_model.bin` / `model.safetensors`); with neither (no
        network in this environment) the HF `_init_weights` distribution is used.  A missing
        `encoder.whole_word_embeddings.weight` keeps its fresh N(0,1) init, as in the reference."""
        import os
        if config is None:
            config = P5ModelConfig.from_backbone(str(backbone))
        model = cls(config, **kw)
        sd = state_dict
        if sd is None and isinstance(backbone, str) and os.path.exists(backbone):
            path = backbone
            if os.path.isdir(path):
                for cand in ("model.safetensors", "pytorch_model.bin"):
                    if os.path.exists(os.path.join(path, cand)):
                        path = os.path.join(path, cand)
                        break
            if path.endswith(".safetensors"):
                from safetensors.torch import load_file
                sd = load_file(path)
            elif os.path.isfile(path):
                sd = torch.load(path, map_location="cpu")
        if sd is not None:
            model.load_state_dict(sd, strict=False)
        return model

    @torch.no_grad()
    def resize_token_embeddings(self, new_num_tokens: int):
        """main.py:193: keep the old rows, new rows ~ N(0, 1) (HF `_init_weights` for the shared table)."""
        old = self.config.vocab_size
        if new_num_tokens == old:
            return self.shared
        state = {k: v.detach().clone() for k, v in super().state_dict().items()}
        old_E = state.pop("shared.weight")
        self.config.vocab_size = int(new_num_tokens)
        seed = self._rng_cpu[0]
        self._build(seed)
        self._copy_in(state, strict=False)
        n = min(old, new_num_tokens)
        self.shared.weight[:n].copy_(old_E[:n])
        self._shadow_dirty = True
        return self.shared

    def get_input_embeddings(self):
        return self.shared

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def zero_grad(self, set_to_none: bool = True):
        """set_to_none=True (torch's default, what the reference loop's optimizer.zero_grad() does, DistributedRunner.py:93): the
        gradients are DEAD until the next backward, which overwrites them -- a first micro-batch STORES every Linear gradient and
        clears only the ~1 MB of atomically accumulated ones -- so there is no 242 MB fill and no read-modify-write of zeros.  The
        `.grad` views stay attached (re-attaching ~130 of them every step is host time); their contents are undefined until that
        backward, where torch would show None.  set_to_none=False: the arena is cleared now."""
        if set_to_none:
            self._be.check(self._lib.p5_engine_discard_grads(self._engine), "discard_grads")
            self._grads_dead = True         # (FusedAdamW.step skips the update until a backward has rewritten them, as torch skips grad=None)
        else:
            self._be.check(self._lib.p5_engine_clear_grads(self._engine, self._be.stream_ptr()), "clear_grads")
            self._grads_dead = False        # real zeros: a step would apply them (weight decay only), as torch does

    def tie_weights(self):
        return None

    def begin_micro_batch(self, first: bool, sync: bool):
        """Gradient accumulation (--gradient_accumulation_steps > 1): every gradient kernel of the engine ADDS into the
        arena (split-K atomics, partial-sum reductions, `+=`), the only overwrite is the clear at the start of a backward --
        so a micro-batch other than the first tells the engine to skip that clear; `sync` = exchange gradients across ranks
        in this backward (only the last micro-batch of a group does)."""
        if not first:
            self._lib.p5_engine_grads_zeroed(self._engine)
        self._ddp_sync = bool(sync)

    # ------------------------------------------------------------------ RNG for dropout
    def set_dropout_seed(self, seed: int, step: int = 0):
        self._rng_cpu = [int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF]
        self._rng.copy_(torch.tensor(self._rng_cpu, dtype=torch.int64).to(torch.int32))

    # ------------------------------------------------------------------ forward / backward
    def _workspace(self, nbytes, which="_ws"):
        cur = getattr(self, which)
        if cur is None or cur.numel() < nbytes:
            raw = torch.empty(int(nbytes * 1.05) + 512, dtype=torch.uint8, device=self._be.device)
            if os.environ.get("P5_POISON_WS"):      # debugging aid: NaN patterns in every byte the engine has not written yet
                raw.fill_(0xFF)
            skew = (-raw.data_ptr()) % 256          # the engine wants a 256-byte aligned base
            cur = raw[skew:skew + int(nbytes * 1.05) + 255]
            setattr(self, which, cur)
        return cur

    @staticmethod
    def _i64(t, device):
        return t.to(device=device, dtype=torch.int64).contiguous()

    @staticmethod
    def _truncation(top_k, top_p):
        """checked (top_k, top_p) of `sample_items` / the item loss: top_k an integer >= 0 (0 = off), 0 < top_p <= 1 (1 = off)"""
        if top_k is None:
            top_k = 0
        if top_p is None:
            top_p = 1.0
        if isinstance(top_k, bool) or int(top_k) != top_k or int(top_k) < 0:
            raise ValueError(f"top_k={top_k!r}: an integer >= 0 (0 = no top-k truncation)")
        p = float(top_p)
        if not (0.0 < p <= 1.0):
            raise ValueError(f"top_p={top_p!r}: 0 < top_p <= 1 (1 = no nucleus truncation)")
        return min(int(top_k), 2 ** 31 - 1), p

    def _item_head_mode(self, item_head, trie):
        """`item_head` of forward / loss_and_backward: None = the model's `item_head` attribute (which a call without a trie ignores)."""
        if item_head is not None and trie is None and item_head == "trie":
            raise ValueError('item_head="trie" needs trie=...: the restricted head belongs to the trie-normalised item loss')
        mode = self.item_head if item_head is None else item_head
        if mode not in ("dense", "trie"):
            raise ValueError(f'item_head={mode!r}: "dense" (the head over the vocabulary) or "trie" (over the tokens of the trie)')
        return mode

    def _item_loss_setup(self, trie, temperature, excluded_items, B, top_k=0, top_p=1.0, item_head="dense"):
        """The checked setting of the trie-normalised item loss (csrc/p5_trie_ce.h) for a batch of B users: the trie on the device, the
        temperature (the check of `_sampling_setup`), the excluded-node bitmap (the rule of `sample_items`), the truncation and the head
        ("trie": the sorted token set of the trie and every edge's column in it, csrc/p5_item_head.h)."""
        dev = self._be.device
        top_k, top_p = self._truncation(top_k, top_p)
        tau = float(temperature)
        if not (tau > 0.0 and math.isfinite(tau)):
            raise ValueError(f"temperature={temperature!r}: a finite value > 0")
        trie = self._compiled_trie(trie)
        start = int(self.config.decoder_start_token_id)
        lo, hi = int(trie.child_off[0]), int(trie.child_off[1])
        if trie.n_nodes < 1 or start not in [int(t) for t in trie.child_tok[lo:hi]]:
            raise ValueError(f"item loss: the trie has no edge for the decoder start token ({start}) at its root")
        if trie.child_tok.size and int(trie.child_tok.max()) >= self.config.vocab_size:
            raise ValueError(f"item loss: the trie holds token {int(trie.child_tok.max())}, the vocabulary has {self.config.vocab_size}")
        excl_t, excl_words = None, 0
        if excluded_items is not None:
            if trie.grafted:
                raise ValueError("item loss (excluded_items=...): a trie with an appended trie (Trie.append) cannot be indexed")
            if getattr(trie, "item_edges", None) is None:
                trie.index_items(trie.enumerate_items())
            excl_np = self._excluded_items_bitmap(trie, excluded_items, B)
            excl_words = int(excl_np.shape[1])
            excl_t = torch.from_numpy(np.ascontiguousarray(excl_np).view(np.int32)).to(dev)
        off, tok, nxt = trie.device_arrays(dev)
        head_tok, head_col = trie.head_columns_device(dev) if item_head == "trie" else (None, None)
        return types.SimpleNamespace(tau=tau, off=off, tok=tok, nxt=nxt, n_nodes=int(trie.n_nodes), excl_t=excl_t, excl_words=excl_words, top_k=top_k,
                                     top_p=top_p, row_cut=None, head_tok=head_tok, head_col=head_col, head_ws=None, reg=False, ref=None,
                                     entropy_coef=0.0, kl_coef=0.0, row_terms=None, terms=None)

    def _item_regularizers(self, q, rows, ref_logits, entropy_coef=0.0, kl_coef=0.0, fused=False):
        """The checked setting of the item loss's regularisers (csrc/p5_trie_reg.h) on the item-loss setting q of a call with `rows` decoder
        rows: per-row entropy and, with `ref_logits`, KL(policy || reference).  Returns q."""
        if q is None:
            raise ValueError("item_entropy / ref_logits / entropy_coef / kl_coef need trie=...: they regularise the trie-normalised item loss")
        if q.top_k > 0 or q.top_p < 1.0:
            raise ValueError("item_entropy / ref_logits / entropy_coef / kl_coef are not built for the truncated item loss (top_k / top_p)")
        ec, kc = float(entropy_coef), float(kl_coef)
        if not (math.isfinite(ec) and math.isfinite(kc)):
            raise ValueError(f"entropy_coef={entropy_coef!r}, kl_coef={kl_coef!r}: finite values")
        if kc != 0.0 and ref_logits is None:
            raise ValueError(f"kl_coef={kl_coef!r} needs ref_logits (a frozen reference model's `item_logits` of this batch)")
        if ref_logits is not None:
            cols = int(q.head_tok.numel()) if q.head_tok is not None else int(self.config.vocab_size)
            head = "trie" if q.head_tok is not None else "dense"
            if not isinstance(ref_logits, torch.Tensor) or ref_logits.dtype != torch.float32:
                raise ValueError(f"ref_logits must be a float32 tensor (got {getattr(ref_logits, 'dtype', type(ref_logits))})")
            if tuple(ref_logits.shape) != (rows, cols):
                raise ValueError(f"ref_logits {tuple(ref_logits.shape)}: [rows, columns] = {(rows, cols)} for this call (item_head={head!r}: "
                                 f"{'the tokens of trie.head_columns()' if head == 'trie' else 'the vocabulary'})")
            if ref_logits.device != self._flat.device:
                raise ValueError(f"ref_logits is on {ref_logits.device}, the model on {self._flat.device}")
            q.ref = ref_logits.detach().contiguous()
        q.reg, q.entropy_coef, q.kl_coef = True, ec, kc
        if fused:
            q.terms = torch.empty(3, dtype=torch.float32, device=self._be.device)
        return q

    def _arm_item_loss(self, q, B, T, G=None):
        """p5_train_set_item_loss (or its truncated sibling) for the engine's next forward; the rows' states land in `last_item_loss_state`
        (no host sync).  Truncated: the rows' cuts live in q.row_cut, which the saved inputs keep alive until the backward has run.
        B: the decoder's batch (users x targets per user, G); the states are [users, G, T] then."""
        state = torch.empty(B, T, dtype=torch.int32, device=self._be.device)
        if q.top_k > 0 or q.top_p < 1.0:
            q.row_cut = torch.empty(B, T, dtype=torch.float32, device=self._be.device)
            self._be.check(self._lib.p5_train_set_item_loss_truncated(self._engine, _ptr(q.off), _ptr(q.tok), _ptr(q.nxt), q.n_nodes, _ptr(q.excl_t),
                                                                      q.excl_words, q.tau, _ptr(state), q.top_k, q.top_p, _ptr(q.row_cut)),
                           "p5_train_set_item_loss_truncated")
        else:
            self._be.check(self._lib.p5_train_set_item_loss(self._engine, _ptr(q.off), _ptr(q.tok), _ptr(q.nxt), q.n_nodes, _ptr(q.excl_t), q.excl_words,
                                                            q.tau, _ptr(state)), "p5_train_set_item_loss")
        if q.head_tok is not None:
            # the restricted head's compact buffers: the caller's, like row_cut -- the saved inputs keep them alive until the backward has run
            n_tok = int(q.head_tok.numel())
            need = int(self._lib.p5_item_head_workspace_bytes(self._engine, B, T, n_tok))
            raw = self.__dict__.get("_item_head_raw")       # (one buffer per model, grown on demand: the engine holds one forward at a time)
            if raw is None or raw.numel() < need + 256:
                raw = self.__dict__["_item_head_raw"] = torch.empty(need + 256, dtype=torch.uint8, device=self._be.device)
            skew = (-raw.data_ptr()) % 256
            q.head_ws = raw[skew:skew + need]
            self._be.check(self._lib.p5_train_set_item_head(self._engine, _ptr(q.head_tok), n_tok, _ptr(q.head_col), _ptr(q.head_ws), need),
                           "p5_train_set_item_head")
        if q.reg:
            # the rows' entropy | KL | reference log-sum-exp: the caller's, like row_cut (the forward writes them, the backward reads them)
            q.row_terms = torch.empty(3 * B * T, dtype=torch.float32, device=self._be.device)
            self._be.check(self._lib.p5_train_set_item_regularizers(self._engine, _ptr(q.ref), 0 if q.ref is None else int(q.ref.shape[1]),
                                                                    _ptr(q.row_terms), q.entropy_coef, q.kl_coef, _ptr(q.terms)),
                           "p5_train_set_item_regularizers")
        self.last_item_loss_state = state if G is None else state.view(B // G, G, T)

    MAX_TARGET_QUERIES = 512        # G * T: the training attention kernels' query limit (cross-attention runs a user's G * T queries)
    MAX_DECODER_ROWS = 1024 * 64    # B * G * T: the norm-backward epilogue's partial table holds 1024 blocks of 64 rows
    MAX_GRID_Y = 65535              # B * G * num_heads: decoder self-attention launches one grid-y entry per (sequence, head)

    def _check_targets(self, B, labels, output_attention=None, target_weights=None, fused=False):
        """The limits of a call with several targets per user (labels [B, G, T]), checked before the engine is called; returns G, or None
        for the plain labels [B, T]."""
        if labels.dim() == 2:
            if fused and output_attention.dim() != 2:
                raise ValueError(f"output_attention {tuple(output_attention.shape)} must match labels {tuple(labels.shape)}")
            if target_weights is not None:
                raise ValueError("target_weights needs labels [B, G, T] (one weight per target); labels [B, T] has none")
            return None
        if labels.dim() != 3:
            raise ValueError(f"labels {tuple(labels.shape)}: [B, T], or [B, G, T] for G targets per user")
        Bl, G, T = labels.shape
        if Bl != B:
            raise ValueError(f"labels {tuple(labels.shape)}: the first dimension must be the batch of input_ids ({B})")
        if G < 1 or T < 1:
            raise ValueError(f"labels {tuple(labels.shape)}: G >= 1 targets per user of T >= 1 tokens")
        if G * T > self.MAX_TARGET_QUERIES:
            raise ValueError(f"labels {tuple(labels.shape)}: G * T = {G * T} exceeds the limit G * T <= {self.MAX_TARGET_QUERIES} "
                             "(the attention kernels' query limit; split the targets over several calls)")
        if B * G * T > self.MAX_DECODER_ROWS:
            raise ValueError(f"labels {tuple(labels.shape)}: B * G * T = {B * G * T} decoder rows exceed the limit B * G * T <= {self.MAX_DECODER_ROWS} "
                             "(the engine's row limit: 1024 blocks of 64 rows in the norm backward's partial table)")
        if G > 1 and B * G * self.config.num_heads > self.MAX_GRID_Y:
            raise ValueError(f"labels {tuple(labels.shape)}: B * G * num_heads = {B * G * self.config.num_heads} exceeds the limit "
                             f"B * G * num_heads <= {self.MAX_GRID_Y} (the y extent of the self-attention launch grids)")
        if fused and tuple(output_attention.shape) != tuple(labels.shape):
            raise ValueError(f"output_attention {tuple(output_attention.shape)} must match labels {tuple(labels.shape)} ([B, G, T])")
        if target_weights is not None and tuple(target_weights.shape) != (B, G):
            raise ValueError(f"target_weights {tuple(target_weights.shape)} must have shape [B, G] = {(B, G)}")
        return int(G)

    def _engine_forward(self, input_ids, whole_word_ids, attention_mask, labels, item_loss=None, inference=False):
        """`inference`: no dropout whatever `self.training` says, and the dropout step stays where it is (`item_logits`)."""
        dev = self._be.device
        B, L = input_ids.shape
        G = int(labels.shape[1]) if labels.dim() == 3 else None      # several targets per user (checked by the caller: _check_targets)
        T = labels.shape[-1]
        Bd = B * (G or 1)
        self._sync_shadow()
        self._sync_transposed()     # (no-op unless the parameters changed; a backward may follow this forward)
        if G is None:
            ws = self._workspace(self._lib.p5_train_workspace_bytes(self._engine, B, L, T))
        else:
            ws = self._workspace(self._lib.p5_train_workspace_bytes_targets(self._engine, B, L, T, G))
        nll = torch.empty(Bd * T, dtype=torch.float32, device=dev)
        training = 1 if (self.training and self.config.dropout_rate > 0 and not inference) else 0
        if training:
            self._advance_dropout_step()
        self._saved_inputs = (input_ids, whole_word_ids, attention_mask, labels, item_loss)   # keep device buffers alive
        if item_loss is not None:
            self._arm_item_loss(item_loss, Bd, T, G)
        if G is None:
            self._be.check(self._lib.p5_forward(self._engine, _ptr(input_ids), _ptr(whole_word_ids), _ptr(attention_mask), _ptr(labels), B, L, T,
                                                training, _ptr(nll), _ptr(ws), ws.numel(), self._be.stream_ptr()), "p5_forward")
        else:
            self._be.check(self._lib.p5_forward_targets(self._engine, _ptr(input_ids), _ptr(whole_word_ids), _ptr(attention_mask), _ptr(labels), B, L, T,
                                                        G, training, _ptr(nll), _ptr(ws), ws.numel(), self._be.stream_ptr()), "p5_forward_targets")
        return nll

    def _engine_backward(self, dnll, d_entropy=None, d_kl=None):
        """dnll = gradient of the per-token NLL (autograd path), or None after `p5_forward_loss`: the engine then seeds
        the backward with the gradient of the runner's masked-mean loss itself.
        d_entropy / d_kl: per-row gradients of the regularised item loss's entropy / KL rows (autograd path; None = zeros)."""
        if dnll is not None:
            dnll = dnll.to(torch.float32).contiguous()
        self.finish_exchange()          # (an exchange nobody consumed: its buckets must land before this backward rewrites the arena)
        lib, eng, sp = self._lib, self._engine, self._be.stream_ptr()
        if d_entropy is not None or d_kl is not None:
            d_entropy = None if d_entropy is None else d_entropy.to(torch.float32).contiguous()
            d_kl = None if d_kl is None else d_kl.to(torch.float32).contiguous()
            self._be.check(lib.p5_backward_set_item_grads(eng, _ptr(d_entropy), _ptr(d_kl)), "p5_backward_set_item_grads")
        exchange = self.ddp_world > 1 and self._ddp_sync
        if exchange or self.staged_backward:
            import torch.distributed as dist
            # ONE library call enqueues every stage and records an event behind each gradient range that became final (the staged backward
            # issues the same grouped weight-gradient launches as the single-GPU step, so ranges leave in two-layer groups); the exchange
            # of range k goes to a communication stream that waits for event k -- it overlaps the rest of the backward on the device, and
            # the host makes one call per step instead of one per stage
            nst = lib.p5_backward_num_stages(eng)
            if self._staged_ranges is None or len(self._staged_ranges) < 2 * nst:
                self._staged_ranges = (ctypes.c_int64 * (2 * nst))()
            nr = ctypes.c_int(0)
            self._be.check(lib.p5_backward_staged(eng, _ptr(dnll), sp, self._staged_ranges, nst, ctypes.byref(nr)), "p5_backward_staged")
            self._staged_n = nr.value
            self._pending = []
            half = str(self.ddp_bucket_dtype).replace("torch.", "") in ("bf16", "bfloat16")
            if exchange:
                comm = self._side
                if comm is None and self._flat.is_cuda:
                    if self._comm is None:
                        self._comm = torch.cuda.Stream(device=self._be.device)
                    comm = self._comm
                if half and (self._bucket16 is None or self._bucket16.numel() != self._grads.numel()):
                    self._bucket16 = torch.empty(self._grads.numel(), dtype=torch.bfloat16, device=self._grads.device)      # allocated once, not per step
                ctx = torch.cuda.stream(comm) if comm is not None else contextlib.nullcontext()
                with ctx:
                    for k in range(nr.value):
                        b0, e0 = int(self._staged_ranges[2 * k]), int(self._staged_ranges[2 * k + 1])
                        if comm is not None:
                            self._be.check(lib.p5_backward_staged_wait(eng, k, ctypes.c_void_p(comm.cuda_stream)), "p5_backward_staged_wait")
                        seg = self._grads[b0:e0]
                        if half:                     # bf16 bucket: cast, reduce, cast back (below)
                            buf = self._bucket16[b0:e0]
                            buf.copy_(seg)
                        else:
                            buf = seg
                        self._pending.append((dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.ddp_group, async_op=True), buf, seg))
            self._pending_half = half
            # the buckets are waited for where the gradients are first READ (FusedAdamW.step -> finish_exchange), bucket by bucket, not here:
            # with a host-blocking backend (gloo) the host goes on to the next batch's collation while the last buckets travel, and nothing
            # between the end of the backward and the optimizer step touches the gradient arena.  `ddp_lazy_wait = False` restores the wait
            # at the end of the backward (a caller that reads .grad before stepping must call finish_exchange() itself).
            if not (exchange and self.ddp_lazy_wait):
                self.finish_exchange()
        else:
            self._be.check(lib.p5_backward(eng, _ptr(dnll), sp), "p5_backward")
        self._grads_dead = False
        for name, p in self.named_parameters():
            if p.grad is None:
                off, n, shape = self._views[name]
                p.grad = self._grads[off:off + n].view(shape)

    def finish_exchange(self):
        """Wait (bucket by bucket, in issue order) for the gradient all-reduces the last backward enqueued; a no-op when none is pending.
        Called by FusedAdamW.step before the gradient norm is taken; call it yourself before reading `.grad` of a data-parallel model."""
        if not self._pending:
            return
        exchange = True
        timing = self.ddp_timing and self._flat.is_cuda
        if timing:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        for w, buf, seg in self._pending:
            w.wait()
            if self._pending_half:
                seg.copy_(buf)      # every rank holds the same bf16 sums -> identical fp32 gradients -> identical updates
        self._pending = []
        for cs in (self._side, self._comm):
            if cs is not None and exchange and self._flat.is_cuda:
                # NCCL/RCCL's wait() already orders the CURRENT stream after the collective; backends that complete on the
                # stream they were issued from (gloo on device tensors) need the explicit edge comm -> main
                torch.cuda.current_stream().wait_stream(cs)
        if timing:
            ev1.record()
            self.ddp_wait_ms.append((ev0, ev1))     # (read by bench.py after a synchronize: main-stream time spent waiting for the buckets)

    def loss_and_backward(self, input_ids, whole_word_ids, attention_mask, labels, output_attention, trie=None, temperature=1.0, excluded_items=None,
                          top_k=0, top_p=1.0, item_head=None, target_weights=None, entropy_coef=0.0, kl_coef=0.0, ref_logits=None, old_logprobs=None,
                          target_mode=None, clip_eps=None, ratio="token", preference=None, pref_beta=0.1, ref_logprobs=None, pref_mask=None,
                          pref_depth=None, pref_length_normalize=False, pref_sft_coef=0.0):
        """Fused form of the reference loop body DistributedRunner.py:63-80: forward, masked-mean loss
        (`(nll.view(B,T) * m).sum(1) / m.sum(1).clamp(min=1)).mean()`) and backward, all inside the engine -- the loss is
        reduced behind the cross-entropy kernel and the backward is seeded from the label mask, so no torch autograd graph and
        none of the ~10 elementwise launches of the generic path.  Returns the loss as a 0-dim tensor; gradients are in `.grad`.
        `trie`, `temperature`, `excluded_items`, `top_k`, `top_p`: the trie-normalised item loss, as in `forward` (the masked mean then runs
        over its NLL); `item_head`: "dense" | "trie" | None = `self.item_head`, as in `forward`.
        Several targets per user: `labels` and `output_attention` [B, G, T] (see `forward`: one encoder pass per user) and optionally
        `target_weights` [B, G] (float; None = ones; may be negative or zero, as advantages are) -- the loss is
        sum_{b,g} w[b,g] * (sum_t nll*m / max(sum_t m, 1)) / (B*G), the runner's masked mean over the replicated batch when w = 1; a target
        with weight 0 or an all-zero mask contributes exactly nothing to the loss and the gradients.
        `entropy_coef`, `kl_coef`, `ref_logits` (item loss only, not under top_k / top_p; csrc/p5_trie_reg.h): the returned loss is
        L_nll + kl_coef * R_KL - entropy_coef * R_H, with L_nll the loss above and R_H / R_KL the same masked mean (NOT weighted by
        `target_weights`: a target of weight 0 still contributes) of the rows' exact entropy over the allowed children and of their exact
        KL(policy || reference); `ref_logits` fp32 [rows, V] ("dense") or [rows, Nu] ("trie") is a frozen reference model's `item_logits` of the
        same batch, finite at the allowed children, a constant of the gradient.  `last_item_loss_terms` is the device tensor
        (L_nll, R_H, R_KL), no host sync (None behind a call without regularisers).  With both coefficients 0 and no `ref_logits` the call is the one above, bit for bit.
        `old_logprobs`, `clip_eps`, `target_mode`, `ratio`: the clipped-ratio (PPO / GRPO style) objective (csrc/p5_clip.h), for several updates
        on one sampled batch; `old_logprobs` and `clip_eps` come together.  `old_logprobs` fp32, shaped like `labels`: the BEHAVIOUR policy's
        log-probability of every label (read where `output_attention != 0`); `clip_eps` a float or a (low, high) pair, lo = 1 - low, hi = 1 + high;
        `target_mode` int [B, G] ([B] without G): 1 = clipped surrogate, 0 = the plain weighted NLL above (a gold target); None = all 1.  With
        rho = exp(-nll - old), w the target's weight and cnt its attended tokens, a mode-1 target's term is
          ratio="token"     (1 / max(cnt, 1)) sum_t m_t max(-rho_t w, -clamp(rho_t, lo, hi) w)
          ratio="sequence"  max(-rho w, -clamp(rho, lo, hi) w), rho = exp(-(sum_t m_t (old_t + nll_t)) / max(cnt, 1)) (GSPO's length-normalised
                            ratio; a target without an attended token contributes nothing)
        in the place of w * (masked mean of nll); the regularisers keep their terms.  A unit (token, or target) is clipped -- no gradient, an
        exact zero -- iff (w > 0 and rho > hi) or (w < 0 and rho < lo).  With rho == 1 everywhere (old = -nll of these weights) every gradient
        carries the bits of the call without the objective.  Rows are taken as they come: the item loss gives NLL 0 to a row it did not score
        (`last_item_loss_state`), so clipped targets should be fully scored -- `policy_batch`'s draws are.  Not under top_k / top_p (the kept set
        may differ between the two policies).  `last_clip_stats` is the device tensor fp32 [8] named by `CLIP_STATS`, no host sync (None behind
        a call without the objective).  Without these keywords the call issues the engine calls it always did.
        `preference` ("pl" | "ipo"; None = off) and `pref_*`, `ref_logprobs`: a listwise preference objective over the G targets of every user
        (csrc/p5_pref.h; needs `labels` [B, G, T], no `target_weights`, not beside the clipped objective, the regularisers or top_k / top_p).
        Per target, with m = output_attention != 0: Delta = (log p(target) - log p_ref(target)) / c', log p = -sum_t m nll, log p_ref =
        sum_t m ref_logprobs (`ref_logprobs` fp32 shaped like `labels`, e.g. `ref.sequence_logprobs(...)` of a `frozen_copy()`; None =
        reference-free), c' = max(sum_t m, 1) under `pref_length_normalize`, else 1; h = pref_beta * Delta.  A user's LIST is its targets with
        `pref_mask` [B, G] != 0 (None = all) and at least one attended token, in index order, the preferred one first; anything else is
        skipped: no contribution, exact-zero gradients, its `ref_logprobs` never read.  "pl" (Plackett-Luce) with `pref_depth` D (None = full):
        sum_{k < min(D, n - 1)} (logsumexp_{j >= k} h_j - h_k) -- a list of two is DPO, D = 1 softmax-DPO (one positive against the listed
        negatives), full depth the likelihood of the whole order; "ipo": mean_{j >= 1} ((Delta_0 - Delta_j) - 1 / (2 pref_beta))^2.  A list of
        fewer than two gives 0; `pref_sft_coef` times the first listed target's masked-mean NLL is added.  The loss is the mean over the B
        users.  `last_pref_stats` is the device tensor fp32 [8] named by `PREF_STATS`, no host sync (None behind a call without the objective)."""
        item_head = self._item_head_mode(item_head, trie)
        clip = self._clip_args(old_logprobs, target_mode, clip_eps, ratio, top_k, top_p)
        pref = self._pref_args(preference, pref_beta, pref_depth, pref_sft_coef, ref_logprobs, pref_mask, top_k, top_p)
        if pref is not None:
            if clip is not None:
                raise ValueError("preference and the clipped objective (old_logprobs / clip_eps) exclude each other: one objective per call")
            if target_weights is not None:
                raise ValueError("preference: target_weights must be None (the objective forms every target's weight itself; list targets with pref_mask)")
            if entropy_coef != 0.0 or kl_coef != 0.0 or ref_logits is not None:
                raise ValueError("preference is not built beside the item regularisers (entropy_coef / kl_coef / ref_logits)")
        dev = self._be.device
        input_ids = self._i64(input_ids, dev)
        B, L = input_ids.shape
        whole_word_ids = self._i64(whole_word_ids if whole_word_ids is not None else torch.zeros_like(input_ids), dev)
        attention_mask = self._i64(attention_mask if attention_mask is not None else (input_ids != self.config.pad_token_id).long(), dev)
        labels = self._i64(labels, dev)
        output_attention = self._i64(output_attention, dev)
        if target_weights is not None:
            target_weights = torch.as_tensor(target_weights).to(device=dev, dtype=torch.float32).contiguous()
        G = self._check_targets(B, labels, output_attention, target_weights, fused=True)
        T = labels.shape[-1]
        Bd = B * (G or 1)
        if clip is not None:
            if not torch.is_tensor(old_logprobs) or tuple(old_logprobs.shape) != tuple(labels.shape):
                raise ValueError(f"old_logprobs {tuple(getattr(old_logprobs, 'shape', ()))} must be a tensor shaped like labels {tuple(labels.shape)}")
            if target_mode is not None and (not torch.is_tensor(target_mode) or tuple(target_mode.shape) != tuple(labels.shape[:-1])):
                raise ValueError(f"target_mode {tuple(getattr(target_mode, 'shape', ()))} must be a tensor of shape {tuple(labels.shape[:-1])} (one per target)")
        if pref is not None:
            if G is None:
                raise ValueError(f"preference needs labels [B, G, T] (the G targets of every user); labels {tuple(labels.shape)} has one")
            if G > self.PREF_MAX_TARGETS:
                raise ValueError(f"preference: G = {G} targets per user exceed the limit G <= {self.PREF_MAX_TARGETS}")
            if ref_logprobs is not None and (not torch.is_tensor(ref_logprobs) or tuple(ref_logprobs.shape) != tuple(labels.shape)):
                raise ValueError(f"ref_logprobs {tuple(getattr(ref_logprobs, 'shape', ()))} must be a tensor shaped like labels {tuple(labels.shape)}")
            if pref_mask is not None and (not torch.is_tensor(pref_mask) or tuple(pref_mask.shape) != (B, G)):
                raise ValueError(f"pref_mask {tuple(getattr(pref_mask, 'shape', ()))} must be a tensor of shape [B, G] = {(B, G)}")
        item_loss = None if trie is None else self._item_loss_setup(trie, temperature, excluded_items, B, top_k, top_p, item_head)
        if entropy_coef != 0.0 or kl_coef != 0.0 or ref_logits is not None:
            item_loss = self._item_regularizers(item_loss, Bd * T, ref_logits, entropy_coef, kl_coef, fused=True)
        self.last_item_loss_terms = item_loss.terms if item_loss is not None else None      # (None behind a call without regularisers: never a stale step's)
        self._sync_shadow()
        self._sync_transposed()
        if G is None:
            ws = self._workspace(self._lib.p5_train_workspace_bytes(self._engine, B, L, T))
        else:
            ws = self._workspace(self._lib.p5_train_workspace_bytes_targets(self._engine, B, L, T, G))
        out = torch.empty(Bd * T + 1, dtype=torch.float32, device=dev)
        training = 1 if (self.training and self.config.dropout_rate > 0) else 0
        if training:
            self._advance_dropout_step()
        self._saved_inputs = (input_ids, whole_word_ids, attention_mask, labels, output_attention, item_loss, target_weights)
        if item_loss is not None:
            self._arm_item_loss(item_loss, Bd, T, G)
        self.last_clip_stats = None            # (None behind a call without the objective: never a stale step's)
        if clip is not None:
            # the seeds (and, regularised, the entropy / KL seeds behind them), the users' partials and the statistics: the caller's, like row_cut
            old = old_logprobs.detach().to(device=dev, dtype=torch.float32).contiguous()
            mode = None if target_mode is None else target_mode.to(device=dev, dtype=torch.int32).contiguous()
            reg = item_loss is not None and item_loss.reg
            buf = torch.empty((3 if reg else 1) * Bd * T + 16 * B + 8, dtype=torch.float32, device=dev)
            seed, partials, stats = torch.split(buf, [buf.numel() - 16 * B - 8, 16 * B, 8])
            self._saved_inputs += (old, mode, buf)
            self._be.check(self._lib.p5_train_set_clip_objective(self._engine, _ptr(old), _ptr(mode), clip[0], clip[1], clip[2], _ptr(seed), _ptr(partials),
                                                                 _ptr(stats)), "p5_train_set_clip_objective")
            self.last_clip_stats = stats
        self.last_pref_stats = None
        if pref is not None:
            # the seeds, the users' partials and the statistics: the caller's, until the backward has run
            ref_lp = None if ref_logprobs is None else ref_logprobs.detach().to(device=dev, dtype=torch.float32).contiguous()
            pmask = None
            if pref_mask is not None:          # (int32 as it is: the kernel tests != 0)
                pmask = (pref_mask if pref_mask.dtype == torch.int32 else (pref_mask != 0)).to(device=dev, dtype=torch.int32).contiguous()
            buf = torch.empty(Bd * T + 16 * B + 8, dtype=torch.float32, device=dev)
            seed, partials, stats = torch.split(buf, [Bd * T, 16 * B, 8])
            self._saved_inputs += (ref_lp, pmask, buf)
            self._be.check(self._lib.p5_train_set_pref_objective(self._engine, _ptr(ref_lp), _ptr(pmask), pref[0], pref[1], pref[2],
                                                                 1 if pref_length_normalize else 0, pref[3], _ptr(seed), _ptr(partials), _ptr(stats)),
                           "p5_train_set_pref_objective")
            self.last_pref_stats = stats
        if G is None:
            self._be.check(self._lib.p5_forward_loss(self._engine, _ptr(input_ids), _ptr(whole_word_ids), _ptr(attention_mask), _ptr(labels),
                                                     _ptr(output_attention), B, L, T, training, _ptr(out), ctypes.c_void_p(out.data_ptr() + 4 * B * T),
                                                     _ptr(ws), ws.numel(), self._be.stream_ptr()), "p5_forward_loss")
        else:
            self._be.check(self._lib.p5_forward_loss_targets(self._engine, _ptr(input_ids), _ptr(whole_word_ids), _ptr(attention_mask), _ptr(labels),
                                                             _ptr(output_attention), B, L, T, G, _ptr(target_weights), training, _ptr(out),
                                                             ctypes.c_void_p(out.data_ptr() + 4 * Bd * T), _ptr(ws), ws.numel(),
                                                             self._be.stream_ptr()), "p5_forward_loss_targets")
        self._engine_backward(None)
        return out[Bd * T]

    # ------------------------------------------------------------------ on-policy fine-tuning (csrc/p5_policy.h)
    POLICY_BASELINES = {"none": 0, "mean": 1, "loo": 2, "grpo": 3}
    POLICY_STATS = ("reward_mean", "users_with_signal", "abs_advantage_mean", "hit_rate", "users_with_hit", "users_without_draw")
    last_policy_batch = None      # of the last policy_step: the dict of policy_batch / its "stats", on the device
    last_policy_stats = None

    CLIP_STATS = ("units", "clipped", "clipped_high", "clipped_low", "ratio_mean", "ratio_max", "ratio_min", "kl_old_new_k3")
    CLIP_RATIOS = {"token": 0, "sequence": 1}
    last_clip_stats = None        # of the last loss_and_backward with the clipped objective: fp32 [8] on the device (CLIP_STATS); else None

    def _clip_args(self, old_logprobs, target_mode, clip_eps, ratio, top_k=0, top_p=1.0):
        """the checked scalars of the clipped objective, (eps_low, eps_high, ratio code), or None when the call does not ask for it"""
        if old_logprobs is None and clip_eps is None:
            if target_mode is not None:
                raise ValueError("target_mode belongs to the clipped objective: it needs old_logprobs and clip_eps")
            if ratio not in self.CLIP_RATIOS:
                raise ValueError(f"ratio={ratio!r}: one of {sorted(self.CLIP_RATIOS)}")
            return None
        if clip_eps is None:
            raise ValueError("old_logprobs needs clip_eps (a float, or a (low, high) pair): the clipped objective takes both")
        if old_logprobs is None:
            raise ValueError("clip_eps needs old_logprobs (the behaviour policy's log-probabilities of the labels): the clipped objective takes both")
        if ratio not in self.CLIP_RATIOS:
            raise ValueError(f"ratio={ratio!r}: one of {sorted(self.CLIP_RATIOS)}")
        try:
            lo, hi = (float(clip_eps),) * 2 if not isinstance(clip_eps, (tuple, list)) else (float(clip_eps[0]), float(clip_eps[1]))
            if isinstance(clip_eps, (tuple, list)) and len(clip_eps) != 2:
                raise TypeError
        except (TypeError, ValueError, IndexError):
            raise ValueError(f"clip_eps={clip_eps!r}: a float, or a (low, high) pair") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo >= 0.0 and hi >= 0.0):
            raise ValueError(f"clip_eps={clip_eps!r}: finite values >= 0")
        tk, tp = self._truncation(top_k, top_p)
        if tk > 0 or tp < 1.0:
            raise ValueError("the clipped objective (clip_eps) is not built for the truncated item loss (top_k / top_p): the kept set may differ "
                             "between the two policies")
        return lo, hi, self.CLIP_RATIOS[ratio]

    PREF_KINDS = {"pl": 0, "ipo": 1}
    PREF_STATS = ("users_with_pair", "pairs_won", "h_first_mean", "h_others_mean", "margin_mean", "preference_loss", "sft_loss", "list_length_mean")
    PREF_MAX_TARGETS = 512
    last_pref_stats = None        # of the last loss_and_backward with a preference objective: fp32 [8] on the device (PREF_STATS); else None

    def _pref_args(self, preference, pref_beta, pref_depth, pref_sft_coef, ref_logprobs=None, pref_mask=None, top_k=0, top_p=1.0):
        """the checked scalars of a preference objective, (kind code, beta, depth (0 = full), sft_coef), or None when the call does not ask for it"""
        if preference is None:
            if ref_logprobs is not None or pref_mask is not None:
                raise ValueError("ref_logprobs / pref_mask belong to a preference objective: they need preference=\"pl\" | \"ipo\"")
            return None
        if preference not in self.PREF_KINDS:
            raise ValueError(f"preference={preference!r}: one of {sorted(self.PREF_KINDS)}, or None")
        try:
            beta, sc = float(pref_beta), float(pref_sft_coef)
        except (TypeError, ValueError):
            raise ValueError(f"pref_beta={pref_beta!r}, pref_sft_coef={pref_sft_coef!r}: numbers") from None
        if not (math.isfinite(beta) and beta > 0.0):
            raise ValueError(f"pref_beta={pref_beta!r}: a finite value > 0")
        if not math.isfinite(sc):
            raise ValueError(f"pref_sft_coef={pref_sft_coef!r}: a finite value")
        if pref_depth is None:
            depth = 0
        else:
            if isinstance(pref_depth, bool) or not isinstance(pref_depth, int) or pref_depth < 1:
                raise ValueError(f"pref_depth={pref_depth!r}: an integer >= 1, or None for the full depth")
            depth = int(pref_depth)
        tk, tp = self._truncation(top_k, top_p)
        if tk > 0 or tp < 1.0:
            raise ValueError("preference is not built for the truncated item loss (top_k / top_p): the kept set may differ between the two policies")
        return self.PREF_KINDS[preference], beta, depth, sc

    @torch.no_grad()
    def sequence_logprobs(self, input_ids, whole_word_ids, attention_mask, labels, trie=None, temperature=1.0, excluded_items=None, item_head=None):
        """log p(label) of every position, -nll shaped like `labels` ([B, T] or [B, G, T]): the full-vocabulary log-softmax, or with `trie` the
        trie-normalised one of the item loss (`temperature`, `excluded_items`, `item_head`: those of `forward`).  No gradient is recorded,
        dropout is never applied whatever `self.training` says, `.grad` and the dropout step stay as they are.  On a `frozen_copy()` it is
        the `ref_logprobs` of `loss_and_backward(preference=...)`.  Positions the loss does not score (label -100, off the trie, behind the
        end) give 0.  Not between a forward of THIS model and its backward: the engine holds one forward at a time."""
        item_head = self._item_head_mode(item_head, trie)
        dev = self._be.device
        input_ids = self._i64(input_ids, dev)
        whole_word_ids = self._i64(whole_word_ids if whole_word_ids is not None else torch.zeros_like(input_ids), dev)
        attention_mask = self._i64(attention_mask if attention_mask is not None else (input_ids != self.config.pad_token_id).long(), dev)
        labels = self._i64(labels, dev)
        self._check_targets(input_ids.shape[0], labels)
        q = None if trie is None else self._item_loss_setup(trie, temperature, excluded_items, input_ids.shape[0], 0, 1.0, item_head)
        nll = self._engine_forward(input_ids, whole_word_ids, attention_mask, labels, q, inference=True)
        return (-nll).view(labels.shape)

    def preference_step(self, input_ids, whole_word_ids, attention_mask, labels, output_attention, trie, num_negatives, preference="pl", pref_depth=1,
                        pref_beta=0.1, pref_sft_coef=0.0, pref_length_normalize=False, ref_model=None, negatives="slate", temperature=1.0,
                        excluded_items=None, item_head=None, seed=None, streams=None):
        """One preference step on negatives drawn from the model itself: (1) `num_negatives` = S items per user from the trie --
        `negatives="slate"`: `sample_slates(slate_size=S)`, S DISTINCT items; "sample": `sample_items(num_samples=S)`, i.i.d. draws; (2)
        `policy_batch` builds the grouped batch [B, S + 1, To], slot 0 = the gold target `labels` [B, T], and the hit reward; (3) the list of
        every user is the gold target and the draws that are NOT the gold item (`pref_mask` = [1, hit == 0], formed on the device); (4)
        `ref_model.sequence_logprobs` of the grouped labels (a `frozen_copy()`; None = reference-free); (5)
        `loss_and_backward(preference=...)`.  The defaults are softmax-DPO (Plackett-Luce, depth 1): the gold against the listed negatives.
        Returns the loss; `last_policy_batch` (the dict of `policy_batch` plus "pref_mask" and "sampled") and `last_pref_stats` stay on the
        device, no host sync.  Every refusal is raised before anything is drawn.  Not built: reward-ordered draws (order `labels` yourself and
        call `loss_and_backward`), per-user weights, a SimPO margin, entropy / KL regularisers beside the objective."""
        if trie is None:
            raise ValueError("preference_step needs trie=...: the draws and the item loss share it")
        if preference is None:
            raise ValueError('preference_step needs preference="pl" | "ipo"')
        self._pref_args(preference, pref_beta, pref_depth, pref_sft_coef)
        if negatives not in ("slate", "sample"):
            raise ValueError(f'negatives={negatives!r}: "slate" (distinct items, sample_slates) or "sample" (i.i.d. draws, sample_items)')
        if isinstance(num_negatives, bool) or not isinstance(num_negatives, int) or num_negatives < 1:
            raise ValueError(f"num_negatives={num_negatives!r}: an integer >= 1 (draws per user)")
        S = int(num_negatives)
        trie = self._compiled_trie(trie)
        item_head = self._item_head_mode(item_head, trie)
        if negatives == "slate":
            if trie.grafted:
                raise ValueError('negatives="slate": a trie with an appended trie (Trie.append) is a DAG, which sample_slates refuses; use negatives="sample"')
            if S > self.SLATE_MAX_K or S > int(self.wide_max_rows):
                raise ValueError(f'negatives="slate": num_negatives={S} exceeds min(SLATE_MAX_K, wide_max_rows) = '
                                 f'{min(self.SLATE_MAX_K, int(self.wide_max_rows))}; use negatives="sample"')
        input_ids = torch.as_tensor(input_ids)
        B = int(input_ids.shape[0])
        Ts = max(2, int(trie.max_depth))
        labels, output_attention = torch.as_tensor(labels), torch.as_tensor(output_attention)
        G, _ = self._check_policy_shapes(B, S, Ts, labels, output_attention, 1)
        if G > self.PREF_MAX_TARGETS:
            raise ValueError(f"num_negatives={S}: G = {G} targets per user exceed the limit G <= {self.PREF_MAX_TARGETS}")
        if negatives == "slate":
            drawn = self.sample_slates(input_ids=input_ids, attention_mask=attention_mask, whole_word_ids=whole_word_ids, trie=trie, slate_size=S,
                                       num_slates=1, temperature=temperature, excluded_items=excluded_items, seed=seed, streams=streams)
        else:
            drawn = self.sample_items(input_ids=input_ids, attention_mask=attention_mask, whole_word_ids=whole_word_ids, trie=trie, num_samples=S,
                                      temperature=temperature, excluded_items=excluded_items, seed=seed, streams=streams)
        pb = self.policy_batch(drawn["sequences"], labels, output_attention, S, rewards=None, baseline="none", policy_coef=1.0, sft_coef=1.0)
        pmask = torch.cat([torch.ones(B, 1, dtype=torch.int32, device=pb["rewards"].device), (pb["rewards"] == 0).to(torch.int32)], dim=1)
        ref_lp = None
        if ref_model is not None:
            ref_lp = ref_model.sequence_logprobs(input_ids, whole_word_ids, attention_mask, pb["labels"], trie=trie, temperature=temperature,
                                                 excluded_items=excluded_items, item_head=item_head)
        loss = self.loss_and_backward(input_ids, whole_word_ids, attention_mask, pb["labels"], pb["output_attention"], trie=trie, temperature=temperature,
                                      excluded_items=excluded_items, item_head=item_head, preference=preference, pref_beta=pref_beta,
                                      ref_logprobs=ref_lp, pref_mask=pmask, pref_depth=pref_depth, pref_length_normalize=pref_length_normalize,
                                      pref_sft_coef=pref_sft_coef)
        pb["pref_mask"], pb["sampled"] = pmask, drawn
        self.last_policy_batch, self.last_policy_stats = pb, pb["stats"]
        return loss

    def _policy_args(self, num_samples, baseline, policy_coef, sft_coef, token_sum, adv_eps):
        """the checked scalars of policy_batch / policy_step: (S, baseline code, policy_coef, sft_coef, token_sum, adv_eps, with_gold)"""
        if isinstance(num_samples, bool) or int(num_samples) != num_samples or int(num_samples) < 1:
            raise ValueError(f"num_samples={num_samples!r}: an integer >= 1 (draws per user)")
        S = int(num_samples)
        if baseline not in self.POLICY_BASELINES:
            raise ValueError(f"baseline={baseline!r}: one of {sorted(self.POLICY_BASELINES)}")
        if baseline == "loo" and S < 2:
            raise ValueError(f'baseline="loo" needs num_samples >= 2 (got {S}): a draw\'s baseline is the mean of the OTHER draws')
        pc, sc, eps = float(policy_coef), float(sft_coef), float(adv_eps)
        if not (math.isfinite(pc) and math.isfinite(sc)):
            raise ValueError(f"policy_coef={policy_coef!r}, sft_coef={sft_coef!r}: finite values")
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"adv_eps={adv_eps!r}: a finite value >= 0")
        return S, self.POLICY_BASELINES[baseline], pc, sc, 1 if token_sum else 0, eps, 0 if sc == 0.0 else 1

    def _check_policy_shapes(self, B, S, Ts, labels, output_attention, with_gold):
        """the grouped call a policy batch of these shapes becomes, held to `_check_targets` before anything is sampled or launched"""
        if labels.dim() != 2 or labels.shape[0] != B:
            raise ValueError(f"labels {tuple(labels.shape)}: the gold target of every user, [B, T] with B = {B}")
        if tuple(output_attention.shape) != tuple(labels.shape):
            raise ValueError(f"output_attention {tuple(output_attention.shape)} must match labels {tuple(labels.shape)}")
        G, To = S + with_gold, max(int(labels.shape[1]), Ts - 1)
        self._check_targets(B, torch.empty(B, G, To, dtype=torch.int64, device="meta"))
        return G, To

    @torch.no_grad()
    def policy_batch(self, sequences, labels, output_attention, num_samples, rewards=None, baseline="loo", policy_coef=1.0, sft_coef=1.0,
                     token_sum=False, adv_eps=1e-6, token_logprobs=None):
        """The batch of one on-policy (REINFORCE-style) step from drawn sequences, built on the device in two launches (csrc/p5_policy.h), no
        host sync: for callers who bring their own sequences (`sample_slates` with num_samples = num_slates * slate_size) or rewards.
        `sequences` int64 [B * S, Ts] as `sample_items` / `sample_slates` return them (an all-pad row: nothing drawn); `labels` /
        `output_attention` [B, T]: every user's gold target (a label of -100 ends it: that position and everything behind it count as not
        attended, as the engine scores nothing there); `rewards` fp32 [B, S] or None = the hit
        reward (1 where the draw is the gold item, else 0).  `baseline`: "none" A = r; "mean" A = r - mean(r); "loo" A_s = r_s - mean of the
        other draws' r (num_samples >= 2; a user with ONE existing draw gets A = 0); "grpo" A = (r - mean) / (population std + adv_eps) -- over
        the draws that exist; a user whose rewards are all equal has A exactly 0.
        Returns device tensors {"labels", "output_attention" [B, G, To], "target_weights" [B, G], "rewards", "advantages" [B, S], "stats" [8]}
        with G = S + 1 (slot 0 = the gold) or G = S when sft_coef == 0, To = max(T, Ts - 1).  `loss_and_backward(labels, output_attention,
        target_weights=...)` on them is sft_coef * mean_b nll(gold_b) + policy_coef * mean_b (1/S) sum_s A_bs nll(draw_bs), nll the token mean
        or -- `token_sum` -- the token sum, whose gradient is REINFORCE's.  `stats`: the values named by `POLICY_STATS`, then two zeros.
        `token_logprobs` fp32 [B * S, Ts - 1] (the sampler's): the dict gains the clipped objective's inputs, "old_logprobs" fp32 [B, G, To] (the
        draws' token log-probabilities at their label positions; the gold slot and positions behind a draw's end: 0) and "target_mode" int32
        [B, G] (gold 0, draws 1); everything else keeps its bits."""
        S, base, pc, sc, tsum, eps, with_gold = self._policy_args(num_samples, baseline, policy_coef, sft_coef, token_sum, adv_eps)
        dev = self._be.device
        if not torch.is_tensor(sequences) or sequences.dim() != 2 or sequences.shape[0] % S != 0 or sequences.shape[0] == 0 or sequences.shape[1] < 2:
            raise ValueError(f"sequences {tuple(getattr(sequences, 'shape', ()))}: [B * num_samples, Ts] with num_samples = {S}, Ts >= 2")
        B, Ts = sequences.shape[0] // S, int(sequences.shape[1])
        labels, output_attention = torch.as_tensor(labels), torch.as_tensor(output_attention)
        G, To = self._check_policy_shapes(B, S, Ts, labels, output_attention, with_gold)
        if rewards is not None:
            if not torch.is_tensor(rewards) or tuple(rewards.shape) != (B, S):
                raise ValueError(f"rewards {tuple(getattr(rewards, 'shape', ()))}: a tensor [B, S] = {(B, S)}")
            rewards = rewards.to(device=dev, dtype=torch.float32).contiguous()
        if token_logprobs is not None:
            if not torch.is_tensor(token_logprobs) or tuple(token_logprobs.shape) != (B * S, Ts - 1):
                raise ValueError(f"token_logprobs {tuple(getattr(token_logprobs, 'shape', ()))}: a tensor [B * S, Ts - 1] = {(B * S, Ts - 1)}")
            token_logprobs = token_logprobs.to(device=dev, dtype=torch.float32).contiguous()
        sequences, labels, output_attention = self._i64(sequences, dev), self._i64(labels, dev), self._i64(output_attention, dev)
        lab_o = torch.empty(B, G, To, dtype=torch.int64, device=dev)
        att_o = torch.empty(B, G, To, dtype=torch.int64, device=dev)
        f = torch.empty(2 * B * S + B * G + 4 * B + 8, dtype=torch.float32, device=dev)       # rewards | advantages | weights | user stats | stats
        r_o, a_o, w_o, us, st = torch.split(f, [B * S, B * S, B * G, 4 * B, 8])
        if token_logprobs is not None:
            old_o = torch.empty(B, G, To, dtype=torch.float32, device=dev)
            mode_o = torch.empty(B, G, dtype=torch.int32, device=dev)
            self._be.check(self._lib.p5_policy_batch_clip(_ptr(sequences), _ptr(labels), _ptr(output_attention), _ptr(rewards), _ptr(token_logprobs), B, S, Ts,
                                                          int(labels.shape[1]), base, pc, sc, tsum, eps, with_gold, int(self.config.pad_token_id),
                                                          int(self.config.eos_token_id), _ptr(lab_o), _ptr(att_o), _ptr(r_o), _ptr(a_o), _ptr(w_o), _ptr(us),
                                                          _ptr(st), _ptr(old_o), _ptr(mode_o), self._be.stream_ptr()), "p5_policy_batch_clip")
            return {"labels": lab_o, "output_attention": att_o, "target_weights": w_o.view(B, G), "rewards": r_o.view(B, S), "advantages": a_o.view(B, S),
                    "stats": st, "old_logprobs": old_o, "target_mode": mode_o}
        self._be.check(self._lib.p5_policy_batch(_ptr(sequences), _ptr(labels), _ptr(output_attention), _ptr(rewards), B, S, Ts, int(labels.shape[1]), base,
                                                 pc, sc, tsum, eps, with_gold, int(self.config.pad_token_id), int(self.config.eos_token_id), _ptr(lab_o),
                                                 _ptr(att_o), _ptr(r_o), _ptr(a_o), _ptr(w_o), _ptr(us), _ptr(st), self._be.stream_ptr()), "p5_policy_batch")
        return {"labels": lab_o, "output_attention": att_o, "target_weights": w_o.view(B, G), "rewards": r_o.view(B, S), "advantages": a_o.view(B, S),
                "stats": st}

    SLATE_ESTIMATORS = {"unbiased": 0, "normalized": 1}
    SLATE_POLICY_STATS = ("value_mean", "weight_sum_mean", "users_with_signal", "abs_advantage_mean", "slates_with_hit", "slates_exhausted",
                          "users_without_draw", "ess_mean")
    SLATE_POLICY_MAX_SLOTS = 1024          # num_slates * (slate_size + 1) per user (csrc/p5_slate_policy.h)

    def _slate_policy_args(self, slate_size, num_slates, estimator, policy_coef, sft_coef, token_sum):
        """the checked scalars of policy_slate_batch / policy_step(slate_size=...): (K, S, estimator code, policy_coef, sft_coef, token_sum,
        with_gold)"""
        if isinstance(slate_size, bool) or int(slate_size) != slate_size or int(slate_size) < 1:
            raise ValueError(f"slate_size={slate_size!r}: an integer >= 1 (items per slate; the sampler draws slate_size + 1, the last one is the threshold)")
        if isinstance(num_slates, bool) or int(num_slates) != num_slates or int(num_slates) < 1:
            raise ValueError(f"num_samples={num_slates!r}: an integer >= 1 (slates per user)")
        K, S = int(slate_size), int(num_slates)
        if estimator not in self.SLATE_ESTIMATORS:
            raise ValueError(f"slate_estimator={estimator!r}: one of {sorted(self.SLATE_ESTIMATORS)}")
        if estimator == "normalized" and K < 2:
            raise ValueError(f'slate_estimator="normalized" needs slate_size >= 2 (got {K}): its baseline is the slate\'s own weighted mean reward; '
                             'use "unbiased"')
        if S * (K + 1) > self.SLATE_POLICY_MAX_SLOTS:
            raise ValueError(f"num_samples * (slate_size + 1) = {S * (K + 1)}: at most {self.SLATE_POLICY_MAX_SLOTS} slots per user")
        pc, sc = float(policy_coef), float(sft_coef)
        if not (math.isfinite(pc) and math.isfinite(sc)):
            raise ValueError(f"policy_coef={policy_coef!r}, sft_coef={sft_coef!r}: finite values")
        return K, S, self.SLATE_ESTIMATORS[estimator], pc, sc, 1 if token_sum else 0, 0 if sc == 0.0 else 1

    @torch.no_grad()
    def policy_slate_batch(self, sampled, labels, output_attention, slate_size, num_slates, rewards=None, estimator="normalized", policy_coef=1.0,
                           sft_coef=1.0, token_sum=False, with_old_logprobs=False):
        """The batch of one on-policy step from SLATES: the importance-weighted without-replacement estimator of Kool, van Hoof and Welling
        (2019, 2020), built on the device in two launches (csrc/p5_slate_policy.h), no host sync.  `sampled` is the dict of
        `sample_slates(slate_size=slate_size + 1, num_slates=num_slates)`: the extra slot's perturbed value is the threshold kappa, an item s
        enters the slate with probability q(s) = 1 - exp(-exp(log p(s) - kappa)), and sum_{s in slate} p(s) / q(s) f(s) estimates E_p[f] without
        bias; the threshold slot becomes no training row.  A user whose allowed items all fit in the slate has kappa = -inf and weights p: the
        exact expectation.  q is the inclusion probability under UNCONDITIONED perturbed values; the sampler's are conditioned on a maximum of
        0, so with sampled["noise_key"] (which `sample_slates` returns) the kernel un-conditions kappa with one Exp(1) draw per slate keyed
        by the slate's own (seed, stream, index) -- without it the estimator is biased (mean W 0.94 instead of 1 at 8 items, K = 3).  A dict
        without "noise_key" is taken to hold unconditioned values log p + Gumbel.
        `rewards` fp32 [B, S, K + 1] (the last slot is never read) or None = the hit reward.  `estimator`: "unbiased"
        A = omega r; "normalized" A = (omega / W)(r - V / W) with W = sum omega, V = sum omega r over the slate (slate_size >= 2): biased,
        consistent, lower in variance; a slate whose rewards are all equal gets A exactly 0.
        Returns the dict of `policy_batch` -- "labels" / "output_attention" [B, G, To], "target_weights" [B, G] with G = S K + 1 (slot 0 = the
        gold; G = S K when sft_coef == 0), "rewards" / "advantages" [B, S, K] -- plus "importance" [B, S, K] (omega), "slate_stats" [B, S, 4] =
        (V, W, kappa, effective sample size W^2 / sum omega^2) and "stats" fp32 [8] named by `SLATE_POLICY_STATS`.  `loss_and_backward` on them
        is sft_coef * mean_b nll(gold_b) + policy_coef * mean_b (1/S) sum_j sum_i A_bji nll_bji.  The estimator's unbiasedness is that of
        `token_sum=True`: the weights refer to log p(item), the SUM of the item's token log-probabilities; `token_sum=False` is the
        length-normalised variant the plain step also offers.  `with_old_logprobs`: the dict gains "old_logprobs" fp32 [B, G, To] and
        "target_mode" int32 [B, G], the clipped objective's inputs, as `policy_batch(token_logprobs=...)` returns them."""
        K, S, est, pc, sc, tsum, with_gold = self._slate_policy_args(slate_size, num_slates, estimator, policy_coef, sft_coef, token_sum)
        K1, dev = K + 1, self._be.device
        try:
            seq, lp, pert = sampled["sequences"], sampled["sequences_logprob"], sampled["perturbed"]
            tok_lp = sampled["token_logprobs"] if with_old_logprobs else None
        except (TypeError, KeyError):
            raise ValueError('sampled: the dict of sample_slates ("sequences", "sequences_logprob", "perturbed", "token_logprobs")') from None
        if not torch.is_tensor(seq) or seq.dim() != 2 or seq.shape[0] == 0 or seq.shape[0] % (S * K1) != 0 or seq.shape[1] < 2:
            raise ValueError(f"sampled['sequences'] {tuple(getattr(seq, 'shape', ()))}: [B * num_slates * (slate_size + 1), Ts] with num_slates = {S}, "
                             f"slate_size + 1 = {K1}, Ts >= 2 -- draw with sample_slates(slate_size={K1})")
        B, Ts = seq.shape[0] // (S * K1), int(seq.shape[1])
        if not torch.is_tensor(lp) or lp.numel() != B * S * K1 or not torch.is_tensor(pert) or pert.numel() != B * S * K1:
            raise ValueError(f"sampled['sequences_logprob'] / ['perturbed']: {B * S * K1} values each, one per slot")
        labels, output_attention = torch.as_tensor(labels), torch.as_tensor(output_attention)
        G, To = self._check_policy_shapes(B, S * K, Ts, labels, output_attention, with_gold)
        if rewards is not None:
            if not torch.is_tensor(rewards) or tuple(rewards.shape) != (B, S, K1):
                raise ValueError(f"rewards {tuple(getattr(rewards, 'shape', ()))}: a tensor [B, S, slate_size + 1] = {(B, S, K1)}")
            rewards = rewards.to(device=dev, dtype=torch.float32).contiguous()
        if tok_lp is not None:
            if not torch.is_tensor(tok_lp) or tuple(tok_lp.shape) != (B * S * K1, Ts - 1):
                raise ValueError(f"sampled['token_logprobs'] {tuple(getattr(tok_lp, 'shape', ()))}: a tensor {(B * S * K1, Ts - 1)}")
            tok_lp = tok_lp.to(device=dev, dtype=torch.float32).contiguous()
        seq, labels, output_attention = self._i64(seq, dev), self._i64(labels, dev), self._i64(output_attention, dev)
        lp, pert = lp.to(device=dev, dtype=torch.float32).contiguous(), pert.to(device=dev, dtype=torch.float32).contiguous()
        lab_o = torch.empty(B, G, To, dtype=torch.int64, device=dev)
        att_o = torch.empty(B, G, To, dtype=torch.int64, device=dev)
        n = B * S * K
        f = torch.empty(3 * n + B * G + 4 * B * S + 8 * B + 8, dtype=torch.float32, device=dev)   # rewards | advantages | importance | weights | slate stats | user stats | stats
        r_o, a_o, i_o, w_o, ss, us, st = torch.split(f, [n, n, n, B * G, 4 * B * S, 8 * B, 8])
        old_o = mode_o = None
        if tok_lp is not None:
            old_o = torch.empty(B, G, To, dtype=torch.float32, device=dev)
            mode_o = torch.empty(B, G, dtype=torch.int32, device=dev)
        r_seed, r_streams, r_base = 0, None, 0
        if sampled.get("noise_key") is not None:
            r_seed, r_streams, r_base = sampled["noise_key"]
            if not torch.is_tensor(r_streams) or r_streams.numel() != B:
                raise ValueError(f"sampled['noise_key']: (seed, stream ids [B = {B}], slate_base) as sample_slates returns it")
            r_streams = r_streams.to(device=dev, dtype=torch.int32).contiguous()
            r_seed, r_base = int(r_seed) & 0xFFFFFFFF, int(r_base) & 0xFFFFFFFF
        self._be.check(self._lib.p5_policy_slate_batch(_ptr(seq), _ptr(lp), _ptr(pert), _ptr(labels), _ptr(output_attention), _ptr(rewards), _ptr(tok_lp), B, S,
                                                       K1, Ts, int(labels.shape[1]), est, pc, sc, tsum, with_gold, int(self.config.pad_token_id),
                                                       int(self.config.eos_token_id), _ptr(lab_o), _ptr(att_o), _ptr(r_o), _ptr(a_o), _ptr(i_o), _ptr(w_o),
                                                       _ptr(ss), _ptr(us), _ptr(st), _ptr(old_o), _ptr(mode_o), _ptr(r_streams), r_seed, r_base,
                                                       self._be.stream_ptr()),
                       "p5_policy_slate_batch")
        out = {"labels": lab_o, "output_attention": att_o, "target_weights": w_o.view(B, G), "rewards": r_o.view(B, S, K), "advantages": a_o.view(B, S, K),
               "importance": i_o.view(B, S, K), "slate_stats": ss.view(B, S, 4), "stats": st}
        if tok_lp is not None:
            out.update(old_logprobs=old_o, target_mode=mode_o)
        return out

    def _check_slate_step(self, trie, slate_size, num_samples, slate_estimator, baseline, top_k, top_p, policy_coef, sft_coef, token_sum):
        """the refusals of policy_step / policy_collect with `slate_size` set, raised before anything is sampled; returns the checked scalars of
        `_slate_policy_args`"""
        q = self._slate_policy_args(slate_size, num_samples, slate_estimator, policy_coef, sft_coef, token_sum)
        tk, tp = self._truncation(top_k, top_p)
        if tk > 0 or tp < 1.0:
            raise ValueError("slate_size: the slate sampler has no truncation (top_k / top_p); use the plain step (slate_size=None) for truncated draws")
        if baseline != "loo":
            raise ValueError(f'slate_size: baseline={baseline!r} belongs to the plain step; a slate\'s baseline is chosen by slate_estimator '
                             '("normalized" = the slate\'s own weighted mean, "unbiased" = none)')
        if trie.grafted:
            raise ValueError("slate_size: a trie with an appended trie (Trie.append) is a DAG, which sample_slates refuses; use the plain step "
                             "(slate_size=None)")
        K1 = q[0] + 1
        if K1 > self.SLATE_MAX_K or K1 > int(self.wide_max_rows):
            raise ValueError(f"slate_size={q[0]}: the sampler draws slate_size + 1 = {K1} items per slate, at most min(SLATE_MAX_K, wide_max_rows) = "
                             f"{min(self.SLATE_MAX_K, int(self.wide_max_rows))}; use a smaller slate and more slates (num_samples)")
        return q

    def policy_step(self, input_ids, whole_word_ids, attention_mask, labels, output_attention, trie, num_samples, temperature=1.0, excluded_items=None,
                    top_k=0, top_p=1.0, item_head=None, baseline="loo", policy_coef=1.0, sft_coef=1.0, token_sum=False, reward_fn=None, seed=None,
                    streams=None, entropy_coef=0.0, kl_coef=0.0, ref_model=None, clip_eps=None, ratio="token", old_logprobs="sampler", slate_size=None,
                    slate_estimator="normalized"):
        """One on-policy fine-tuning step: (1) `sample_items(num_samples=...)` with the trie, temperature, exclusion and truncation the loss
        uses -- that sameness is what on-policy means here; (2) `policy_batch` on the draws (`reward_fn`, if given, is called with the
        sampler's dict and returns fp32 [B, S] on the device; else the hit reward against `labels`); (3) `loss_and_backward` on the grouped
        batch [B, G, To] with the advantages as `target_weights`.  With `kl_coef != 0`, `ref_model` (a `frozen_copy()`) supplies `ref_logits`
        of the grouped labels; entropy and KL keep the meaning and the limits of `loss_and_backward` (not under top_k / top_p).
        Returns the loss as a 0-dim tensor, gradients in `.grad`; `last_policy_batch` (the dict of `policy_batch`) and `last_policy_stats`
        (fp32 [8], `POLICY_STATS`) stay on the device, no host sync.  The limits of a grouped call (G * To <= 512, ...) are checked before
        anything is sampled.  Sampling ignores `self.training` (no dropout in the draw, as in `sample_items`); the training forward applies
        dropout as usual, so under dropout the draws come from the dropout-free policy.  `seed` / `streams`: those of `sample_items`.
        `clip_eps` (None = off: the step above, bit for bit): `policy_collect` and then ONE `policy_update` with the clipped-ratio objective
        (`ratio`, `old_logprobs`: theirs) -- call the two yourself for several updates per sampled batch.
        `slate_size=K` (None = off: the step above, bit for bit): the draws are `num_samples` SLATES of K distinct items per user,
        `sample_slates(slate_size=K + 1, num_slates=num_samples)` (the extra slot is the threshold), `reward_fn` returns fp32 [B, S, K + 1], and
        the batch comes from `policy_slate_batch(estimator=slate_estimator)`: the importance-weighted without-replacement estimator, G = S K + 1
        training rows.  Its unbiasedness ("unbiased") is that of `token_sum=True`: the weights refer to log p(item); `token_sum=False` is the
        length-normalised variant the plain step also offers.  With `slate_size` set, `top_k` / `top_p` (the slate sampler has no truncation), a
        `baseline` other than its default (the slate's baseline is `slate_estimator`'s), a grafted trie and K + 1 above `SLATE_MAX_K` /
        `wide_max_rows` are ValueErrors raised before anything is sampled.  `last_policy_stats` are then named by `SLATE_POLICY_STATS`."""
        if clip_eps is not None:
            rollout = self.policy_collect(input_ids, whole_word_ids, attention_mask, labels, output_attention, trie, num_samples, temperature=temperature,
                                          excluded_items=excluded_items, top_k=top_k, top_p=top_p, item_head=item_head, baseline=baseline,
                                          policy_coef=policy_coef, sft_coef=sft_coef, token_sum=token_sum, reward_fn=reward_fn, seed=seed, streams=streams,
                                          entropy_coef=entropy_coef, kl_coef=kl_coef, ref_model=ref_model, old_logprobs=old_logprobs, clip_eps=clip_eps,
                                          ratio=ratio, **({} if slate_size is None else dict(slate_size=slate_size, slate_estimator=slate_estimator)))
            return self.policy_update(input_ids, whole_word_ids, attention_mask, rollout, trie, clip_eps, ratio=ratio, temperature=temperature,
                                      excluded_items=excluded_items, item_head=item_head, entropy_coef=entropy_coef, kl_coef=kl_coef)
        if trie is None:
            raise ValueError("policy_step needs trie=...: the draws and the item loss share it")
        K = None
        if slate_size is not None:
            trie = self._compiled_trie(trie)
            K, S, _, _, _, _, with_gold = self._check_slate_step(trie, slate_size, num_samples, slate_estimator, baseline, top_k, top_p, policy_coef,
                                                                 sft_coef, token_sum)
        else:
            S, _, _, _, _, _, with_gold = self._policy_args(num_samples, baseline, policy_coef, sft_coef, token_sum, 1e-6)
        item_head = self._item_head_mode(item_head, trie)
        top_k, top_p = self._truncation(top_k, top_p)
        ec, kc = float(entropy_coef), float(kl_coef)
        if ec != 0.0 or kc != 0.0:
            if top_k > 0 or top_p < 1.0:
                raise ValueError("entropy_coef / kl_coef are not built for the truncated item loss (top_k / top_p)")
            if not (math.isfinite(ec) and math.isfinite(kc)):
                raise ValueError(f"entropy_coef={entropy_coef!r}, kl_coef={kl_coef!r}: finite values")
            if kc != 0.0 and ref_model is None:
                raise ValueError(f"kl_coef={kl_coef!r} needs ref_model (a frozen_copy() of the reference policy)")
        trie = self._compiled_trie(trie)
        input_ids = torch.as_tensor(input_ids)
        B = int(input_ids.shape[0])
        depth = int(trie.max_depth)
        Ts = max(2, depth)
        labels, output_attention = torch.as_tensor(labels), torch.as_tensor(output_attention)
        self._check_policy_shapes(B, S if K is None else S * K, Ts, labels, output_attention, with_gold)
        if K is None:
            drawn = self.sample_items(input_ids=input_ids, attention_mask=attention_mask, whole_word_ids=whole_word_ids, trie=trie, num_samples=S,
                                      temperature=temperature, excluded_items=excluded_items, seed=seed, streams=streams, top_k=top_k, top_p=top_p)
            rewards = None if reward_fn is None else reward_fn(drawn)
            pb = self.policy_batch(drawn["sequences"], labels, output_attention, S, rewards=rewards, baseline=baseline, policy_coef=policy_coef,
                                   sft_coef=sft_coef, token_sum=token_sum)
        else:
            drawn = self.sample_slates(input_ids=input_ids, attention_mask=attention_mask, whole_word_ids=whole_word_ids, trie=trie, slate_size=K + 1,
                                       num_slates=S, temperature=temperature, excluded_items=excluded_items, seed=seed, streams=streams)
            rewards = None if reward_fn is None else reward_fn(drawn)
            pb = self.policy_slate_batch(drawn, labels, output_attention, K, S, rewards=rewards, estimator=slate_estimator, policy_coef=policy_coef,
                                         sft_coef=sft_coef, token_sum=token_sum)
        kw = {}
        if ec != 0.0 or kc != 0.0:
            kw.update(entropy_coef=ec, kl_coef=kc)
            if kc != 0.0:
                kw["ref_logits"] = ref_model.item_logits(input_ids, whole_word_ids, attention_mask, pb["labels"], trie, temperature=temperature,
                                                         excluded_items=excluded_items, item_head=item_head)
        loss = self.loss_and_backward(input_ids, whole_word_ids, attention_mask, pb["labels"], pb["output_attention"], trie=trie, temperature=temperature,
                                      excluded_items=excluded_items, top_k=top_k, top_p=top_p, item_head=item_head, target_weights=pb["target_weights"],
                                      **kw)
        self.last_policy_batch, self.last_policy_stats = pb, pb["stats"]
        return loss

    def policy_collect(self, input_ids, whole_word_ids, attention_mask, labels, output_attention, trie, num_samples, temperature=1.0,
                       excluded_items=None, top_k=0, top_p=1.0, item_head=None, baseline="loo", policy_coef=1.0, sft_coef=1.0, token_sum=False,
                       reward_fn=None, seed=None, streams=None, entropy_coef=0.0, kl_coef=0.0, ref_model=None, old_logprobs="sampler", clip_eps=0.2,
                       ratio="token", slate_size=None, slate_estimator="normalized"):
        """The rollout of a clipped-ratio (PPO / GRPO style) step: `sample_items` and `policy_batch` as in `policy_step`, ONCE, for several
        `policy_update` calls.  Returns the dict of `policy_batch` plus "old_logprobs" fp32 [B, G, To] (the behaviour policy's log-probability
        of every label), "target_mode" int32 [B, G] (gold 0, draws 1), "sampled" (the sampler's dict) and -- with `kl_coef != 0` -- "ref_logits"
        (`ref_model.item_logits` of the grouped labels: they depend on the labels only, so the updates share them).
        `old_logprobs`: "sampler" = the sampler's `token_logprobs`, which cost nothing (the decode kernels and the training forward differ in
        their last bits: the first update's ratio is 1 up to those); "forward" = recomputed with one grouped item-loss forward of this model,
        no gradient, no dropout: the first update's ratio is then exactly 1 when dropout is off.  `clip_eps` / `ratio` / `entropy_coef` are only
        checked here (every refusal of the update is raised before anything is sampled).  Not under top_k / top_p.
        `slate_size` / `slate_estimator`: those of `policy_step` -- slates and `policy_slate_batch(with_old_logprobs=True)` in place of draws
        and `policy_batch`."""
        if trie is None:
            raise ValueError("policy_collect needs trie=...: the draws and the item loss share it")
        if old_logprobs not in ("sampler", "forward"):
            raise ValueError(f'old_logprobs={old_logprobs!r}: "sampler" (the sampler\'s token_logprobs) or "forward" (recomputed by a training-path forward)')
        self._clip_args(True, None, clip_eps, ratio, top_k, top_p)
        K = None
        if slate_size is not None:
            trie = self._compiled_trie(trie)
            K, S, _, _, _, _, with_gold = self._check_slate_step(trie, slate_size, num_samples, slate_estimator, baseline, top_k, top_p, policy_coef,
                                                                 sft_coef, token_sum)
        else:
            S, _, _, _, _, _, with_gold = self._policy_args(num_samples, baseline, policy_coef, sft_coef, token_sum, 1e-6)
        item_head = self._item_head_mode(item_head, trie)
        ec, kc = float(entropy_coef), float(kl_coef)
        if not (math.isfinite(ec) and math.isfinite(kc)):
            raise ValueError(f"entropy_coef={entropy_coef!r}, kl_coef={kl_coef!r}: finite values")
        if kc != 0.0 and ref_model is None:
            raise ValueError(f"kl_coef={kl_coef!r} needs ref_model (a frozen_copy() of the reference policy)")
        trie = self._compiled_trie(trie)
        input_ids = torch.as_tensor(input_ids)
        B = int(input_ids.shape[0])
        Ts = max(2, int(trie.max_depth))
        labels, output_attention = torch.as_tensor(labels), torch.as_tensor(output_attention)
        self._check_policy_shapes(B, S if K is None else S * K, Ts, labels, output_attention, with_gold)
        if K is None:
            drawn = self.sample_items(input_ids=input_ids, attention_mask=attention_mask, whole_word_ids=whole_word_ids, trie=trie, num_samples=S,
                                      temperature=temperature, excluded_items=excluded_items, seed=seed, streams=streams)
            rewards = None if reward_fn is None else reward_fn(drawn)
            rollout = self.policy_batch(drawn["sequences"], labels, output_attention, S, rewards=rewards, baseline=baseline, policy_coef=policy_coef,
                                        sft_coef=sft_coef, token_sum=token_sum, token_logprobs=drawn["token_logprobs"])
        else:
            drawn = self.sample_slates(input_ids=input_ids, attention_mask=attention_mask, whole_word_ids=whole_word_ids, trie=trie, slate_size=K + 1,
                                       num_slates=S, temperature=temperature, excluded_items=excluded_items, seed=seed, streams=streams)
            rewards = None if reward_fn is None else reward_fn(drawn)
            rollout = self.policy_slate_batch(drawn, labels, output_attention, K, S, rewards=rewards, estimator=slate_estimator, policy_coef=policy_coef,
                                              sft_coef=sft_coef, token_sum=token_sum, with_old_logprobs=True)
        rollout["sampled"] = drawn
        if old_logprobs == "forward":
            dev = self._be.device
            ids = self._i64(input_ids, dev)
            ww = self._i64(whole_word_ids if whole_word_ids is not None else torch.zeros_like(ids), dev)
            am = self._i64(attention_mask if attention_mask is not None else (ids != self.config.pad_token_id).long(), dev)
            q = self._item_loss_setup(trie, temperature, excluded_items, B, 0, 1.0, item_head)
            with torch.no_grad():
                nll = self._engine_forward(ids, ww, am, rollout["labels"], q, inference=True)
            rollout["old_logprobs"] = (-nll).view_as(rollout["old_logprobs"])
        if kc != 0.0:
            rollout["ref_logits"] = ref_model.item_logits(input_ids, whole_word_ids, attention_mask, rollout["labels"], trie, temperature=temperature,
                                                          excluded_items=excluded_items, item_head=item_head)
        self.last_policy_batch, self.last_policy_stats = rollout, rollout["stats"]
        return rollout

    def policy_update(self, input_ids, whole_word_ids, attention_mask, rollout, trie, clip_eps, ratio="token", temperature=1.0, excluded_items=None,
                      item_head=None, entropy_coef=0.0, kl_coef=0.0):
        """One update on a rollout of `policy_collect`: `loss_and_backward` on its grouped batch with the clipped-ratio objective (the gold
        slot keeps its plain weighted NLL).  Callable several times per rollout: optimizer step and `zero_grad` in between are the caller's.
        Trie, temperature, exclusion and head must be those of the collect.  With `kl_coef != 0` the rollout's "ref_logits" are used.
        Returns the loss; `last_clip_stats` says how much was clipped."""
        if trie is None:
            raise ValueError("policy_update needs trie=...: the item loss of the rollout's draws")
        if clip_eps is None:
            raise ValueError("policy_update needs clip_eps (a float, or a (low, high) pair)")
        kw = {}
        if float(entropy_coef) != 0.0 or float(kl_coef) != 0.0:
            kw.update(entropy_coef=float(entropy_coef), kl_coef=float(kl_coef))
            if float(kl_coef) != 0.0:
                if "ref_logits" not in rollout:
                    raise ValueError(f"kl_coef={kl_coef!r}: the rollout holds no ref_logits (policy_collect(kl_coef=..., ref_model=...) computes them once)")
                kw["ref_logits"] = rollout["ref_logits"]
        return self.loss_and_backward(input_ids, whole_word_ids, attention_mask, rollout["labels"], rollout["output_attention"], trie=trie,
                                      temperature=temperature, excluded_items=excluded_items, item_head=item_head,
                                      target_weights=rollout["target_weights"], old_logprobs=rollout["old_logprobs"], target_mode=rollout["target_mode"],
                                      clip_eps=clip_eps, ratio=ratio, **kw)

    def _advance_dropout_step(self):
        self._rng_cpu[1] = (self._rng_cpu[1] + 1) & 0xFFFFFFFF
        self._rng[1] = self._rng_cpu[1] if self._rng_cpu[1] < 2 ** 31 else self._rng_cpu[1] - 2 ** 32

    def forward(self, input_ids=None, whole_word_ids=None, attention_mask=None, labels=None, alpha=None, return_dict=True, trie=None,
                temperature=1.0, excluded_items=None, top_k=0, top_p=1.0, item_head=None, item_entropy=False, ref_logits=None, **unused):
        """P5_T5.forward (P5_T5.py:275-386): returns {"loss": flat [B*T] per-token NLL}; `alpha` is accepted and ignored
        exactly as in the reference (P5_T5.py:294).
        `trie` (Trie / CompiledTrie; None = the full-vocabulary cross-entropy, unchanged): the trie-normalised item loss (csrc/p5_trie_ce.h),
        the NLL of the distribution `sample_items` / `sample_slates` draw from -- at every position softmax(logits / `temperature`)
        renormalised over the allowed children of the trie node behind labels[b, :t]; `excluded_items` (per-user lists of item indices, as
        for `sample_items`; not for a trie with an appended trie) are taken out of the normalisation.  With the sampler's trie, temperature
        and exclusion, forward(labels=drawn[:, 1:]) returns -token_logprobs of the draw and its backward is the score function of what was
        drawn.  Positions behind </s>, at label -100 and behind it, and every position from the first label that is not an allowed child
        on, have NLL 0 and no gradient; `last_item_loss_state` (int32 [B, T] on the device, no host sync) says which: 0 scored, 1 past the
        end, 2 off the trie.
        `top_k` (0 = off) / `top_p` (1 = off): the loss of the TRUNCATED distribution `sample_items(top_k=, top_p=)` draws from
        (csrc/p5_trunc.h) -- the normalisation runs over the kept children only and the kept set is a constant of the gradient (HF's
        masked_fill under autograd); a label that is allowed but below the row's cut has NLL 0, no gradient and state 3 (truncated away),
        for that row only.
        `item_head` ("dense" | "trie"; None = `self.item_head`, "dense" unless changed): "dense" runs the tied head over the whole vocabulary
        and writes a dense logits gradient; "trie" (csrc/p5_item_head.h) runs it over the distinct tokens of the trie's edges only -- no
        [B*T, V] array is written or read, the loss is the same function of the logits, and rows of shared.weight's gradient whose token is
        neither on the trie nor looked up by the batch are exact zeros.  Gradient accumulation (`begin_micro_batch`), DDP and the staged
        backward work with either head as for the plain loss.
        Several targets per user: `labels` [B, G, T] returns the flat [B*G*T] NLL, in (b, g, t) order, of the replicated batch (user b's
        inputs repeated G times, sample b*G + g carrying labels[b, g]) -- but the encoder and the cross-attention K/V projections run ONCE per
        user, and the gradients into them are the sums over the user's G targets.  G * T <= 512, B * G * T <= 65536, B * G * num_heads <= 65535.  Every keyword
        keeps its meaning; `excluded_items` stays per USER and applies to all G targets, `last_item_loss_state` is [B, G, T].
        `sample_items(...)["sequences"].view(B, S, -1)[:, :, 1:]` and the [B, S*K, .] view of a slate are valid `labels` as they are.
        With dropout on, the masks are those of the tensors the engine forms (decoder rows [B*G*T, .], self-attention [B*G, H, T, T],
        cross-attention [B, H, G*T, L]), not those of the replicated batch.  labels[:, None, :] (G = 1) returns the bits of the 2-D call.
        `item_entropy=True` / `ref_logits` (item loss only, not under top_k / top_p; csrc/p5_trie_reg.h): the dict gains "item_entropy" and /
        or "item_kl", flat fp32 like "loss" and differentiable -- per scored row the exact entropy of the row's distribution over its allowed
        children, and its exact KL(policy || reference) from the distribution `ref_logits` give over the same children at the same
        temperature (rows that are not scored, and rows with one allowed child: exactly 0).  `ref_logits`: fp32 [rows, V] ("dense") or
        [rows, Nu] ("trie"), a frozen reference model's `item_logits` of the same batch; finite at the allowed children (not checked); a
        constant of the gradient.  One engine backward serves the three outputs.  "loss" keeps the bits it has without the keywords."""
        if labels is None:
            raise ValueError("P5T5Native.forward needs labels (the runner always passes them)")
        item_head = self._item_head_mode(item_head, trie)
        dev = self._be.device
        input_ids = self._i64(input_ids, dev)
        if whole_word_ids is None:
            whole_word_ids = torch.zeros_like(input_ids)
        whole_word_ids = self._i64(whole_word_ids, dev)
        if attention_mask is None:
            attention_mask = (input_ids != self.config.pad_token_id).long()
        attention_mask = self._i64(attention_mask, dev)
        labels = self._i64(labels, dev)
        self._check_targets(input_ids.shape[0], labels)
        item_loss = None if trie is None else self._item_loss_setup(trie, temperature, excluded_items, input_ids.shape[0], top_k, top_p, item_head)
        if item_entropy or ref_logits is not None:
            item_loss = self._item_regularizers(item_loss, labels.numel(), ref_logits)
            nll, ent, kl = _P5RegLossFn.apply(self._anchor, self, input_ids, whole_word_ids, attention_mask, labels, item_loss)
            out = {"loss": nll}
            if item_entropy:
                out["item_entropy"] = ent
            if ref_logits is not None:
                out["item_kl"] = kl
            return out if return_dict else (nll,)
        nll = _P5LossFn.apply(self._anchor, self, input_ids, whole_word_ids, attention_mask, labels, item_loss)
        out = {"loss": nll}
        return out if return_dict else (nll,)

    def frozen_copy(self):
        """A second model on the same backend with a copy of this model's weights as they are now, in eval mode, same dtype, tied to no
        optimizer and to no data-parallel group: the frozen reference policy whose `item_logits` are another call's `ref_logits`."""
        ref = P5T5Native(copy.copy(self.config), dtype="bf16" if self.compute_dtype == 1 else "fp32", backend=self._be)
        ref.load_state_dict(self.state_dict(), strict=True)
        ref.item_head = self.item_head
        ref.eval()
        return ref

    @torch.no_grad()
    def item_logits(self, input_ids, whole_word_ids, attention_mask, labels, trie, temperature=1.0, excluded_items=None, item_head=None):
        """The head's fp32 logits of an item-loss forward, as a frozen REFERENCE model hands them to another model's `ref_logits`:
        [rows, V] ("dense") or [rows, Nu] ("trie": the columns of `trie.head_columns()`), rows = B*T or B*G*T in the order of "loss".
        No gradient is recorded, dropout is never applied whatever `self.training` says, `.grad` and the dropout step stay as they are.
        The result is a fresh tensor copied on the current stream: the engine's buffers may be reused at once.  (The logits do not depend
        on `temperature` / `excluded_items`; they are accepted so that the call takes the arguments of the forward it mirrors.)
        Not between a forward of THIS model and its backward: the engine holds one forward at a time."""
        if trie is None:
            raise ValueError("item_logits needs trie=...")
        item_head = self._item_head_mode(item_head, trie)
        dev = self._be.device
        input_ids = self._i64(input_ids, dev)
        whole_word_ids = self._i64(whole_word_ids if whole_word_ids is not None else torch.zeros_like(input_ids), dev)
        attention_mask = self._i64(attention_mask if attention_mask is not None else (input_ids != self.config.pad_token_id).long(), dev)
        labels = self._i64(labels, dev)
        self._check_targets(input_ids.shape[0], labels)
        q = self._item_loss_setup(trie, temperature, excluded_items, input_ids.shape[0], 0, 1.0, item_head)
        self._engine_forward(input_ids, whole_word_ids, attention_mask, labels, q, inference=True)
        ptr, rows, ld, cols = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._be.check(self._lib.p5_train_last_item_logits(self._engine, ctypes.byref(ptr), ctypes.byref(rows), ctypes.byref(ld), ctypes.byref(cols)),
                       "p5_train_last_item_logits")
        base = q.head_ws if q.head_ws is not None else self._ws       # (the array lives in the buffer this call handed to the engine)
        off, nbytes = int(ptr.value) - base.data_ptr(), rows.value * ld.value * 4
        if off < 0 or off + nbytes > base.numel():
            raise RuntimeError("item_logits: the engine's logits lie outside the workspace of this call")
        return base[off:off + nbytes].view(torch.float32).view(rows.value, ld.value)[:, :cols.value].clone()

    # ------------------------------------------------------------------ generation lanes
    def _drop_lanes(self):
        for ln in getattr(self, "_lanes", []):
            if ln.engine_v:
                self._lib.p5_engine_destroy(ln.engine_v)
            if ln.idx > 0 and ln.engine:
                self._lib.p5_engine_destroy(ln.engine)
        self._lanes = []

    def _lane(self, i):
        """lane i, created on demand: lane 0 = the model's own engine; lane i > 0 = a second search engine over the SAME parameter arenas,
        bf16 shadow and transposed / norm-folded copies (read-only during generation) with its own HIP stream."""
        while len(self._lanes) <= i:
            k = len(self._lanes)
            if k == 0:
                self._lanes.append(_GenLane(0, self._engine))
                continue
            cfg = self._cfg_struct()
            eng = ctypes.c_void_p()
            self._be.check(self._lib.p5_engine_create(ctypes.byref(cfg), ctypes.byref(eng)), "p5_engine_create (lane)")
            self._be.check(self._lib.p5_engine_bind(eng, _ptr(self._flat), _ptr(self._grads), _ptr(self._shadow), _ptr(self._lut_enc), _ptr(self._lut_dec),
                                                     self.LUT_HALF, _ptr(self._rng)), "p5_engine_bind (lane)")
            if self._shadow_t is not None:
                self._be.check(self._lib.p5_engine_bind_transposed(eng, _ptr(self._shadow_t), self._be.stream_ptr()), "p5_engine_bind_transposed (lane)")
            self._lanes.append(_GenLane(k, eng, torch.cuda.Stream(device=self._be.device) if self._flat.is_cuda else None))
        return self._lanes[i]

    def _cur_lane(self):
        return getattr(self._tls, "lane", None) or self._lane(0)

    def _lane_workspace(self, lane, nbytes, key):
        cur = lane.ws.get(key)
        if cur is None or cur.numel() < nbytes:
            raw = torch.empty(int(nbytes * 1.05) + 512, dtype=torch.uint8, device=self._be.device)
            skew = (-raw.data_ptr()) % 256
            cur = raw[skew:skew + int(nbytes * 1.05) + 255]
            lane.ws[key] = cur
        return cur

    def map_lanes(self, fn, items, lanes=None):
        """`fn(item)` for every item, IN ORDER, with up to `lanes` calls in flight: each worker thread owns a generation lane (its own search /
        verification engines, workspaces and HIP stream over the model's one set of weights), so the latency-bound kernel chain of one
        batch's beam search overlaps the next batch's -- on one MI355X two lanes run beam-10 generation at 1.5-1.6 x the items/s of one
        (DESIGN.md 3.8).  `fn` typically calls `model.generate(...)` and post-processes its result; results come back as a generator."""
        lanes = int(self.gen_lanes if lanes is None else lanes)
        if lanes <= 1 or not self._flat.is_cuda:
            for it in items:
                yield fn(it)
            return
        import collections
        import concurrent.futures
        # parameter copies the searches read are refreshed HERE, once, on the caller's stream: no lane does it under another lane's feet
        self._sync_shadow()
        self._sync_transposed()
        pool = [self._lane(i + 1) for i in range(lanes)]          # lanes 1 .. n; lane 0 stays with the calling thread's own generate() calls
        main = torch.cuda.current_stream()
        for ln in pool:
            ln.stream.wait_stream(main)
        q, lock, tls = collections.deque(pool), threading.Lock(), self._tls

        dev = self._be.device

        def init():
            torch.cuda.set_device(dev)          # (the current device is per host thread; rank r of a multi-GPU job is not on device 0)
            with lock:
                tls.lane = q.popleft()

        def run(it):
            ln = tls.lane
            with torch.cuda.stream(ln.stream), torch.no_grad():
                out = fn(it)
                ln.stream.synchronize()
            return out

        with concurrent.futures.ThreadPoolExecutor(max_workers=lanes, initializer=init) as ex:
            pending = collections.deque()
            for it in items:
                pending.append(ex.submit(run, it))
                while len(pending) >= 2 * lanes:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()
        for ln in pool:
            main.wait_stream(ln.stream)

    # ------------------------------------------------------------------ generation
    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, whole_word_ids=None, max_length: int = 20,
                 prefix_allowed_tokens_fn: Optional[Callable] = None, num_beams: int = 1, num_return_sequences: Optional[int] = None,
                 output_scores: bool = False, return_dict_in_generate: bool = False, trie=None, roots=None, excluded=None, **unused):
        """Constrained beam search (DistributedRunner.py:361-371).  `prefix_allowed_tokens_fn` made by
        `openp5_amd.trie.prefix_allowed_tokens_fn` -- or by the reference's own generation_trie.prefix_allowed_tokens_fn,
        whose closure holds the Trie -- runs fully on the device.  `trie` may be passed directly (Trie / CompiledTrie).
        `excluded`: optional uint32 [B, words] bitmap from `CompiledTrie.excluded_bitmap` -- per-user history exclusion.
        `do_sample=True` (with num_beams=1; `num_return_sequences` draws per user, `temperature`, optional `seed` / `streams` / `draw_base`)
        draws items instead of searching: see `sample_items`, whose sequences and log-probabilities ("sequences_scores") it returns."""
        if unused.get("do_sample"):
            return self._generate_sampled(input_ids, attention_mask, whole_word_ids, max_length, prefix_allowed_tokens_fn, num_beams, num_return_sequences,
                                          output_scores, return_dict_in_generate, trie, roots, excluded, unused)
        dev = self._be.device
        K = int(num_beams)
        nret = int(num_return_sequences or K)
        if trie is None and prefix_allowed_tokens_fn is not None:
            trie = find_trie(prefix_allowed_tokens_fn)
            if trie is None:
                trie = self._explore_callable(prefix_allowed_tokens_fn, input_ids.shape[0], max_length)
                roots = trie._roots
        if trie is None:
            raise ValueError("generate() needs a trie / prefix_allowed_tokens_fn (OpenP5 always decodes under the item trie)")
        trie = self._compiled_trie(trie)
        off, tok, nxt = trie.device_arrays(dev)
        input_ids = self._i64(input_ids, dev)
        B, L = input_ids.shape
        if whole_word_ids is None:
            whole_word_ids = torch.zeros_like(input_ids)
        whole_word_ids = self._i64(whole_word_ids, dev)
        if attention_mask is None:
            attention_mask = (input_ids != self.config.pad_token_id).long()
        attention_mask = self._i64(attention_mask, dev)
        roots_t = None
        if roots is not None:
            roots_t = torch.as_tensor(roots, dtype=torch.int32, device=dev).contiguous()
        self._sync_shadow()
        self._sync_transposed()     # (also refreshes the folded copy W diag(ln) the encoder pass multiplies the raw residual stream with)
        maxc = max(1, trie.max_children)
        excl_t, excl_words = None, 0
        if excluded is not None:
            excl_np = np.ascontiguousarray(excluded.cpu().numpy() if torch.is_tensor(excluded) else excluded, dtype=np.uint32)
            if excl_np.ndim != 2 or excl_np.shape[0] != B or excl_np.shape[1] * 32 < trie.n_nodes:
                raise ValueError(f"excluded bitmap must be [B={B}, >= {(trie.n_nodes + 31) // 32}] uint32, got {excl_np.shape}")
            excl_words = int(excl_np.shape[1])
            excl_t = torch.from_numpy(excl_np.view(np.int32)).to(dev)
        # no hypothesis is longer than the deepest trie path, and the search stops on the device (no per-step read-back):
        # enqueue exactly as many decode steps as can do work.  (With max_length == depth the forced finish at max_length
        # coincides with the leaves' </s>, so results are those of the unbounded call.)
        max_length = max(2, min(int(max_length), int(trie.max_depth)))
        # forced-prefix fast-forward (include/p5hip.h): the chain every item shares behind the start token, as long as no user's history
        # exclusion touches it (an excluded node on the chain would leave that user without candidates: the plain search handles that)
        lane = self._cur_lane()
        lane.forced = ([], [])
        if self.prefix_fast_forward and roots_t is None:
            ftok, fnode = trie.forced_prefix(self.config.decoder_start_token_id, self.config.eos_token_id)
            n = min(len(ftok), max_length - 2)
            if n >= 2 and excluded is not None:
                words = excl_np[:, [x >> 5 for x in fnode[:n]]]
                bits = np.asarray([x & 31 for x in fnode[:n]], dtype=np.uint32)
                if bool(((words >> bits[None, :]) & 1).any()):
                    n = 0
            if n >= 2:
                lane.forced = (ftok[:n], fnode[:n])
        mode = unused.get("generation_mode", self.generation_mode)
        if mode not in ("verified", "draft"):
            raise ValueError(f"generation_mode={mode!r} (verified | draft)")
        if not 1 <= K <= self.WIDE_MAX_K:
            raise ValueError(f"generate(num_beams={K}): 1 <= num_beams <= {self.WIDE_MAX_K}")
        args = (input_ids, whole_word_ids, attention_mask, B, L, K, max_length, off, tok, nxt, roots_t, excl_t, excl_words, maxc)
        if self.compute_dtype == 1 and mode == "verified" and K <= self.VERIFY_MAX_K:
            seq, score, ln = self._generate_verified(*args)
            path = "verified"
        elif self.compute_dtype == 1 and mode == "verified":
            # the replay's candidate pool (K x 2K entries in LDS, csrc/p5_verify.h P5_VERIFY_POOL) ends at K = 22: wider searches run as the
            # plain fp32 search on the verification engine -- still the fp32 search's lists, at its speed -- and say so
            if not self._warned_wide_verified:
                warnings.warn(f"generate(num_beams={K}): verified generation covers num_beams <= {self.VERIFY_MAX_K}; running the plain fp32 beam search "
                              f"instead (same ranked lists, slower).  generation_mode='draft' selects the plain bf16 search.", RuntimeWarning, stacklevel=2)
                self._warned_wide_verified = True
            seq, score, ln = self._in_user_chunks(self._search_fp32, args)
            with self._stats_lock:
                self.verify_stats["wide_fp32_users"] += B
            path = "fp32_search"
        else:
            seq, score, ln = self._in_user_chunks(lambda *a: self._search(lane.engine, "gen", *a), args)
            path = "draft_bf16" if self.compute_dtype == 1 else "fp32_search"
        self.last_generate_path = path
        out_len = 1 + int(ln[:, :nret].max().item())
        sequences = seq[:, :nret, :out_len].reshape(B * nret, out_len).to(torch.int64)
        scores = score[:, :nret].reshape(B * nret)
        if return_dict_in_generate:
            return {"sequences": sequences, "sequences_scores": scores if output_scores else None}
        return sequences

    @staticmethod
    def _compiled_trie(trie):
        """The CompiledTrie of a `Trie` (ours or the reference's), compiled once and cached on it; a CompiledTrie passes through."""
        if isinstance(trie, Trie) or (hasattr(trie, "trie_dict") and not isinstance(trie, CompiledTrie)):
            app = getattr(trie, "append_trie", None)
            key = (getattr(trie, "len", None), id(app), getattr(app, "len", None), getattr(trie, "bos_token_id", None))
            cache = getattr(trie, "_p5_compiled", None)
            if cache is None or cache[0] != key:
                cache = (key, CompiledTrie.from_trie(trie))        # (grafts an appended trie, trie.py)
                try:
                    trie._p5_compiled = cache
                except Exception:
                    pass
            trie = cache[1]
        return trie

    # ------------------------------------------------------------------ exhaustive catalogue ranking (csrc/p5_rank.h)
    @torch.no_grad()
    def rank_items(self, input_ids=None, attention_mask=None, whole_word_ids=None, trie=None, top_n: int = 10, excluded_items=None,
                   return_all_scores: bool = False, generation_mode: Optional[str] = None, roots=None, pruned=False, seed_items=None):
        """Rank the WHOLE catalogue for every user, exactly: one teacher-forced decoder pass over every prefix of the item trie gives each
        item the score HF's beam search would assign it (sum of its tokens' log-probabilities up to and including </s>, divided by their
        number), then an exact top-`top_n` per user -- what `generate(num_beams = number of items + 1)` returns, without a search.
        `trie`: Trie / CompiledTrie; items are indexed on demand (`CompiledTrie.index_items`; an unindexed trie's items are numbered in
        lexicographic order).  `excluded_items`: per-user lists of item indices that are not ranked (their scores are still computed).
        Arithmetic follows `generation_mode` as generate() does: a bf16 model in "verified" mode ranks with the fp32 verification engine,
        in "draft" mode with the bf16 engine; an fp32 model ranks in fp32.  fp32 passes multiply with split products; a user whose pass
        leaves their range is rescored with exact fp32 products.  Users go through in chunks whose workspace fits `rank_max_bytes`.
        `pruned=True` (a bf16 model in "verified" mode; no effect on an fp32 model or in "draft" mode): certified pruned ranking
        (csrc/p5_prune.h).  The bf16 pass over the whole trie proposes the prefixes whose score bound is within `rank_prune_slack` of its
        N-th score, the fp32 engine scores those prefixes alone, and a certificate (margin `rank_prune_margin`) proves that no item
        outside them reaches the fp32 N-th score: the returned lists are the fp32 lists.  A user without a certificate is ranked by the
        full fp32 pass (`rank_stats["fallback_users"]`); when the proposal keeps more than `rank_prune_max_fraction` of the rows the
        chunk's users are (`"declined_users"`).  `last_generate_path` is "rank_pruned" when at least one user of the call was certified.
        Only survivors have fp32 scores, so `return_all_scores` cannot be combined with it.
        `pruned="search"` (a bf16 model in "verified" mode AND an fp32 model; no effect in "draft" mode): bounded trie search
        (csrc/p5_bound.h), no pass over the whole trie at all.  The deciding engine scores the prefixes of a few seed items -- the model's
        own constrained beam search with `rank_search_seed_beams` (default `top_n`) beams, or `seed_items` [B, S] item indices, -1 = empty
        slot -- and round by round exactly the frontier prefixes whose score bound still reaches the N-th score, until none does: that is
        the certificate of `pruned=True`, so the returned lists are the fp32 lists.  The two integers read per round are the only host
        synchronisation.  Users without a certificate fall back to the full pass (`rank_stats["search_fallback_users"]`); a chunk whose
        users outgrow `rank_search_max_fraction` of the rows is declined (`"search_declined_users"`); `"search_rounds"` is the last chunk's
        round count, `"search_rows_per_user"` the largest final row count.  `last_generate_path` is "rank_search" when at least one user was
        certified.  Not with `return_all_scores`.
        Returns {"sequences" int64 [B * top_n, S] (decoder start first, pad-filled), "sequences_scores" [B * top_n], "item_index"
        [B, top_n] (-1 and score -1e9 where a user has fewer than top_n candidates), "scores" [B, n_items] or None}."""
        lib, dev = self._lib, self._be.device
        if roots is not None:
            raise ValueError("rank_items: per-user roots are not supported (one trie, shared by all users)")
        if trie is None:
            raise ValueError("rank_items() needs the item trie (Trie / CompiledTrie)")
        N = int(top_n)
        if not 1 <= N <= self.WIDE_MAX_K:
            raise ValueError(f"rank_items(top_n={N}): 1 <= top_n <= {self.WIDE_MAX_K}")
        trie = self._compiled_trie(trie)
        if trie.grafted:
            raise ValueError("rank_items: a trie with an appended trie (Trie.append) is a DAG; exhaustive ranking needs a tree of items")
        if getattr(trie, "item_edges", None) is None:
            trie.index_items(trie.enumerate_items())
        mode = self.generation_mode if generation_mode is None else generation_mode
        if mode not in ("verified", "draft"):
            raise ValueError(f"generation_mode={mode!r} (verified | draft)")
        start = self.config.decoder_start_token_id
        plan = trie.rank_plan(start)
        if plan["levels"] > self.LUT_HALF:
            raise ValueError(f"rank_items: items longer than {self.LUT_HALF} tokens")
        off, tok, _ = trie.device_arrays(dev)
        row_tok, row_depth, row_node, row_anc, item_edges, item_tokens = trie.rank_device_arrays(dev, start)
        n_items, n_edges, rows = int(item_edges.shape[0]), int(tok.numel()), int(plan["rows"])
        input_ids = self._i64(input_ids, dev)
        B, L = input_ids.shape
        if whole_word_ids is None:
            whole_word_ids = torch.zeros_like(input_ids)
        whole_word_ids = self._i64(whole_word_ids, dev)
        if attention_mask is None:
            attention_mask = (input_ids != self.config.pad_token_id).long()
        attention_mask = self._i64(attention_mask, dev)
        excl_t = None
        if excluded_items is not None:
            if len(excluded_items) != B:
                raise ValueError(f"excluded_items: one list of item indices per user ({B}), got {len(excluded_items)}")
            bm = np.zeros((B, (n_items + 31) // 32), dtype=np.uint32)
            for b, items in enumerate(excluded_items):
                it = np.unique(np.asarray(list(items), dtype=np.int64))
                if it.size and (it[0] < 0 or it[-1] >= n_items):
                    raise ValueError(f"excluded_items[{b}]: item indices must be in 0 .. {n_items - 1}")
                np.bitwise_or.at(bm[b], it >> 5, (np.uint32(1) << (it & 31).astype(np.uint32)))
            excl_t = torch.from_numpy(bm.view(np.int32)).to(dev)
        self._sync_shadow()
        self._sync_transposed()
        lane = self._cur_lane()
        if self.compute_dtype == 1 and mode == "draft":
            engine, path = lane.engine, "rank_bf16"
        elif self.compute_dtype == 1:
            engine, path = self._verify_engine(lane), "rank_fp32"
        else:
            engine, path = lane.engine, "rank_fp32"
        if isinstance(pruned, str):
            if pruned != "search":
                raise ValueError(f"rank_items(pruned={pruned!r}): False | True | \"search\"")
        elif pruned is None or pruned not in (True, False):
            raise ValueError(f"rank_items(pruned={pruned!r}): False | True | \"search\"")
        search = isinstance(pruned, str) and not (self.compute_dtype == 1 and mode == "draft")
        prune = not isinstance(pruned, str) and bool(pruned) and self.compute_dtype == 1 and mode == "verified"
        if prune and return_all_scores:
            raise ValueError("rank_items(pruned=True, return_all_scores=True): only the prefixes that survive pruning get fp32 scores")
        if search and return_all_scores:
            raise ValueError("rank_items(pruned=\"search\", return_all_scores=True): only the prefixes the search reaches get fp32 scores")
        if seed_items is not None and not isinstance(pruned, str):
            raise ValueError("rank_items: seed_items goes with pruned=\"search\"")
        need_full = lambda nb: int(lib.p5_rank_workspace_bytes(engine, nb, L, rows, n_edges, n_items, N))      # noqa: E731
        need = need_full
        if prune:
            frac = float(self.rank_prune_max_fraction)
            slack, margin = float(self.rank_prune_slack), float(self.rank_prune_margin)
            if not (slack >= 0.0 and margin >= 0.0 and 0.0 < frac <= 1.0):
                raise ValueError("rank_prune_slack >= 0, rank_prune_margin >= 0, 0 < rank_prune_max_fraction <= 1")
            max_keep = max(1, min(rows, int(frac * rows)))          # a proposal that keeps more rows per user is declined
            row_lmax, row_edge, edge_row = trie.prune_device_arrays(dev, start)
            need_prune = lambda nb, kept: int(lib.p5_prune_workspace_bytes(engine, nb, L, rows, kept, n_edges, n_items, N))      # noqa: E731
            need_draft = lambda nb: int(lib.p5_rank_workspace_bytes(lane.engine, nb, L, rows, n_edges, n_items, N))      # noqa: E731
            need = lambda nb: max(need_full(nb), need_draft(nb), need_prune(nb, max_keep))      # noqa: E731
        if search:
            frac, margin = float(self.rank_search_max_fraction), float(self.rank_prune_margin)
            if not (margin >= 0.0 and 0.0 < frac <= 1.0):
                raise ValueError("rank_prune_margin >= 0, 0 < rank_search_max_fraction <= 1")
            max_keep = max(1, min(rows, int(frac * rows)))          # a user whose set of scored rows outgrows this declines the chunk
            row_lmax, row_edge, edge_row = trie.prune_device_arrays(dev, start)
            levels = int(row_anc.shape[1])
            if seed_items is not None:
                seed_idx = torch.as_tensor(seed_items, dtype=torch.int64, device=dev)
                if seed_idx.dim() != 2 or seed_idx.shape[0] != B or not 1 <= seed_idx.shape[1] <= self.WIDE_MAX_K:
                    raise ValueError(f"seed_items: item indices [B={B}, 1 .. {self.WIDE_MAX_K}] (-1 = empty slot), got {tuple(seed_idx.shape)}")
                if int(seed_idx.max()) >= n_items or int(seed_idx.min()) < -1:
                    raise ValueError(f"seed_items: item indices must be in -1 .. {n_items - 1}")
                seeds = (item_tokens[seed_idx.clamp(min=0)] * (seed_idx >= 0).unsqueeze(-1)).contiguous()
            else:
                # the model's own constrained beam search proposes: the draft search of a bf16 model, the fp32 search of an fp32 model
                n_beams = max(1, min(int(self.rank_search_seed_beams or N), self.WIDE_MAX_K))
                bm = None if excluded_items is None else trie.excluded_bitmap(excluded_items)
                seeds = self.generate(input_ids=input_ids, attention_mask=attention_mask, whole_word_ids=whole_word_ids, max_length=trie.max_depth,
                                      num_beams=n_beams, trie=trie, excluded=bm, generation_mode="draft")
                seeds = seeds.view(B, n_beams, -1).contiguous()
            if self._search_seed_hook is not None:
                self._search_seed_hook(seeds)
            n_seeds, seed_len = int(seeds.shape[1]), int(seeds.shape[2])
            need_search = lambda nb, kept: int(lib.p5_bound_workspace_bytes(engine, nb, L, rows, kept, n_edges, n_items, N, n_seeds, levels))      # noqa: E731
            need = lambda nb: max(need_full(nb), need_search(nb, max_keep))      # noqa: E731
        budget = int(self.rank_max_bytes)
        if need(1) > budget:
            raise ValueError(f"rank_items: one user of this catalogue needs a workspace of {need(1)} bytes, rank_max_bytes is {budget}")
        per = B
        while need(per) > budget:
            per = max(1, min(per - 1, per * budget // need(per)))
        index = torch.empty(B, N, dtype=torch.int32, device=dev)
        score = torch.empty(B, N, dtype=torch.float32, device=dev)
        scores_all = torch.empty(B, n_items, dtype=torch.float32, device=dev) if return_all_scores else None
        sp = self._be.stream_ptr()

        def run(users, exact):
            nb = int(users.numel())
            whole = nb == B and bool((users == torch.arange(B, device=users.device)).all())
            cut = lambda t: None if t is None else (t if whole else t[users].contiguous())      # noqa: E731
            ids_c, ww_c, mask_c, ex_c = cut(input_ids), cut(whole_word_ids), cut(attention_mask), cut(excl_t)
            o_idx = torch.empty(nb, N, dtype=torch.int32, device=dev)
            o_sc = torch.empty(nb, N, dtype=torch.float32, device=dev)
            o_all = torch.empty(nb, n_items, dtype=torch.float32, device=dev) if return_all_scores else None
            flagged = torch.zeros(nb, dtype=torch.int32, device=dev)
            ws = self._lane_workspace(lane, need_full(nb), "rank")
            self._be.check(lib.p5_rank_items(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, _ptr(off), _ptr(tok), n_edges, _ptr(row_tok),
                                             _ptr(row_depth), _ptr(row_node), _ptr(row_anc), rows, int(row_anc.shape[1]), _ptr(item_edges), n_items,
                                             int(item_edges.shape[1]), _ptr(ex_c), N, 1 if exact else 0, _ptr(o_all), _ptr(o_idx), _ptr(o_sc),
                                             _ptr(flagged), _ptr(ws), ws.numel(), sp), "p5_rank_items")
            return o_idx, o_sc, o_all, flagged

        def run_pruned(users):
            """PROPOSE on the bf16 engine, DECIDE on the fp32 engine: (index, score, flagged) of the users, or the largest kept-row count
            alone when the proposal is declined"""
            nb = int(users.numel())
            whole = nb == B
            cut = lambda t: None if t is None else (t if whole else t[users].contiguous())      # noqa: E731
            ids_c, ww_c, mask_c, ex_c = cut(input_ids), cut(whole_word_ids), cut(attention_mask), cut(excl_t)
            o_idx = torch.empty(nb, N, dtype=torch.int32, device=dev)
            o_sc = torch.empty(nb, N, dtype=torch.float32, device=dev)
            flagged = torch.zeros(nb, dtype=torch.int32, device=dev)
            ws_r = self._lane_workspace(lane, need_draft(nb), "rank")
            ws_p = self._lane_workspace(lane, need_prune(nb, max_keep), "prune")         # (sized for the largest pass that is not declined: the head stays put)
            trie_args = (_ptr(off), _ptr(tok), n_edges, _ptr(row_tok), _ptr(row_depth), _ptr(row_node), _ptr(row_anc), rows, int(row_anc.shape[1]))
            self._be.check(lib.p5_prune_propose(lane.engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, *trie_args, _ptr(row_edge), _ptr(row_lmax),
                                                _ptr(item_edges), n_items, int(item_edges.shape[1]), _ptr(ex_c), N, slack, _ptr(o_idx), _ptr(o_sc), _ptr(flagged),
                                                _ptr(ws_r), ws_r.numel(), _ptr(ws_p), ws_p.numel(), sp), "p5_prune_propose")
            off_sel = 256 + (nb * 4 + 255) // 256 * 256
            n_rows_t = ws_p[256:256 + nb * 4].view(torch.int32)
            sel_t = ws_p[off_sel:off_sel + nb * rows * 4].view(torch.int32).view(nb, rows)
            if self._prune_sabotage is not None:
                self._prune_sabotage(sel_t, n_rows_t)
                ws_p[:4].view(torch.int32).copy_(n_rows_t.max().reshape(1))
            kept = int(ws_p[:4].view(torch.int32).item())        # the one integer the host reads: it sizes the pass
            if kept > max_keep:
                return kept, None
            kept = max(kept, 1)
            self._be.check(lib.p5_prune_decide(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, *trie_args, _ptr(row_edge), _ptr(row_lmax), _ptr(edge_row),
                                               _ptr(item_edges), n_items, int(item_edges.shape[1]), _ptr(ex_c), N, kept, margin, _ptr(o_idx), _ptr(o_sc),
                                               _ptr(flagged), _ptr(ws_p), ws_p.numel(), sp), "p5_prune_decide")
            return kept, (o_idx, o_sc, flagged)

        def run_search(users):
            """BEGIN + ROUNDs on the deciding engine: (largest row count, rounds, (index, score, flagged) of the users or None when the
            chunk is declined)"""
            nb = int(users.numel())
            whole = nb == B
            cut = lambda t: None if t is None else (t if whole else t[users].contiguous())      # noqa: E731
            ids_c, ww_c, mask_c, ex_c, seeds_c = cut(input_ids), cut(whole_word_ids), cut(attention_mask), cut(excl_t), cut(seeds)
            o_idx = torch.empty(nb, N, dtype=torch.int32, device=dev)
            o_sc = torch.empty(nb, N, dtype=torch.float32, device=dev)
            flagged = torch.zeros(nb, dtype=torch.int32, device=dev)
            ws = self._lane_workspace(lane, need_search(nb, max_keep), "search")          # (sized for the largest pass that is not declined: the head stays put)
            self._be.check(lib.p5_bound_begin(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, _ptr(off), _ptr(tok), n_edges, _ptr(row_tok), _ptr(row_node),
                                              rows, levels, _ptr(edge_row), _ptr(seeds_c), n_seeds, seed_len, n_items, N, _ptr(ws), ws.numel(), sp),
                           "p5_bound_begin")
            off_sel = 256 + (nb * 4 + 255) // 256 * 256
            hdr_t = ws[:8].view(torch.int32)
            n_rows_t = ws[256:256 + nb * 4].view(torch.int32)
            sel_t = ws[off_sel:off_sel + nb * rows * 4].view(torch.int32).view(nb, rows)
            kept, rounds = int(hdr_t[0].item()), 0
            while True:
                if kept > max_keep:
                    return kept, rounds, None
                if rounds == levels + 1:
                    # (not reached in exact arithmetic: new rows get strictly deeper.)  No certificate for anybody
                    flagged.fill_(1)
                    break
                kept = max(kept, 1)
                self._be.check(lib.p5_bound_round(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, _ptr(off), _ptr(tok), n_edges, _ptr(row_tok),
                                                  _ptr(row_depth), _ptr(row_node), _ptr(row_anc), rows, levels, _ptr(row_edge), _ptr(row_lmax), _ptr(edge_row),
                                                  _ptr(item_edges), n_items, int(item_edges.shape[1]), _ptr(ex_c), N, n_seeds, kept, margin, _ptr(o_idx),
                                                  _ptr(o_sc), _ptr(flagged), _ptr(ws), ws.numel(), sp), "p5_bound_round")
                rounds += 1
                kept, grew = hdr_t.tolist()          # the two integers the host reads per round
                if self._search_hook is not None:
                    self._search_hook(rounds, sel_t, n_rows_t)
                    kept = int(n_rows_t.max().item())
                    hdr_t[0] = kept
                if grew == 0:
                    break
            return kept, rounds, (o_idx, o_sc, flagged)

        rescored = certified = fallback = declined = kept_max = 0
        s_rounds = 0
        for a in range(0, B, per):
            users = torch.arange(a, min(B, a + per), device=dev)
            todo = users
            if search:
                kept, s_rounds, res = run_search(users)
                kept_max = max(kept_max, kept)
                if res is None:
                    declined += int(users.numel())
                else:
                    o_idx, o_sc, flagged = res
                    index[users], score[users] = o_idx, o_sc
                    # no certificate: these users through the full pass (their search results are overwritten, never returned)
                    todo = users[flagged.nonzero().flatten()]
                    fallback += int(todo.numel())
                    certified += int(users.numel()) - int(todo.numel())
                if not todo.numel():
                    continue
            if prune:
                kept, res = run_pruned(users)
                kept_max = max(kept_max, kept)
                if res is None:
                    declined += int(users.numel())
                else:
                    o_idx, o_sc, flagged = res
                    index[users], score[users] = o_idx, o_sc
                    # no certificate: these users through the full fp32 pass (their pruned results are overwritten, never returned)
                    todo = users[flagged.nonzero().flatten()]
                    fallback += int(todo.numel())
                    certified += int(users.numel()) - int(todo.numel())
                if not todo.numel():
                    continue
            o_idx, o_sc, o_all, flagged = run(todo, False)
            index[todo], score[todo] = o_idx, o_sc
            if scores_all is not None:
                scores_all[todo] = o_all
            bad = todo[flagged.nonzero().flatten()]
            if bad.numel():
                # a value of the split-product pass left the range of the two-term fp16 split: these users again, with exact fp32 products
                rescored += int(bad.numel())
                o_idx, o_sc, o_all, flagged = run(bad, True)
                index[bad], score[bad] = o_idx, o_sc
                if scores_all is not None:
                    scores_all[bad] = o_all
        with self._stats_lock:
            st = self.rank_stats
            st["calls"] += 1; st["users"] += B; st["rescored_users"] += rescored; st["users_per_pass"] = per; st["rows_per_user"] = rows
            if prune:
                st["pruned_calls"] += 1; st["certified_users"] += certified; st["fallback_users"] += fallback; st["declined_users"] += declined
                st["kept_rows_per_user"] = kept_max
            if search:
                st["search_calls"] += 1; st["search_certified_users"] += certified; st["search_fallback_users"] += fallback
                st["search_declined_users"] += declined; st["search_rounds"] = s_rounds; st["search_rows_per_user"] = kept_max
        if prune and certified:
            path = "rank_pruned"
        if search and certified:
            path = "rank_search"
        self.last_generate_path = path
        item_index = index.to(torch.int64)
        sequences = item_tokens[item_index.clamp(min=0)] * (item_index >= 0).unsqueeze(-1)       # (a missing candidate: the all-pad sequence)
        return {"sequences": sequences.reshape(B * N, -1), "sequences_scores": score.reshape(B * N), "item_index": item_index, "scores": scores_all}

    # ------------------------------------------------------------------ per-user candidate lists (csrc/p5_cand.h)
    @torch.no_grad()
    def score_candidates(self, input_ids=None, attention_mask=None, whole_word_ids=None, trie=None, candidates=None, top_n: Optional[int] = None,
                         generation_mode: Optional[str] = None):
        """The exact score and order of C chosen items per user (sampled-candidates evaluation, re-ranking a first stage's short list):
        one teacher-forced decoder pass over the prefixes of each user's OWN candidates -- the numbers `rank_items` gives those items,
        at a cost that follows the candidates, with no buffer that grows with the catalogue.
        `candidates`: LongTensor [B, C] or a list of B lists (ragged lists are padded with -1 = empty slot) of item indices in the order
        given to `CompiledTrie.index_items` (an unindexed trie is indexed on demand in lexicographic order); a user's items are distinct.
        Engine choice, split products and the exact rescoring of flagged users follow `rank_items`; users go through in chunks whose
        workspace fits `rank_max_bytes`.  `top_n` defaults to C.
        Returns {"scores" fp32 [B, C] in slot order (-1e9 for an empty slot), "order" int64 [B, top_n] slots by (score desc, item index
        asc) with -1 beyond the user's candidates, "item_index" [B, top_n], "sequences" int64 [B * top_n, S], "sequences_scores"
        [B * top_n] (as rank_items returns them)}."""
        lib, dev = self._lib, self._be.device
        if trie is None:
            raise ValueError("score_candidates() needs the item trie (Trie / CompiledTrie)")
        if candidates is None:
            raise ValueError("score_candidates() needs `candidates`: item indices per user")
        trie = self._compiled_trie(trie)
        if trie.grafted:
            raise ValueError("score_candidates: a trie with an appended trie (Trie.append) is a DAG; candidate scoring needs a tree of items")
        if getattr(trie, "item_edges", None) is None:
            trie.index_items(trie.enumerate_items())
        mode = self.generation_mode if generation_mode is None else generation_mode
        if mode not in ("verified", "draft"):
            raise ValueError(f"generation_mode={mode!r} (verified | draft)")
        input_ids = self._i64(input_ids, dev)
        B, L = input_ids.shape
        if torch.is_tensor(candidates):
            cand = candidates.detach().cpu().numpy().astype(np.int64)
        else:
            rows_ = [list(map(int, c)) for c in candidates]
            width = max((len(c) for c in rows_), default=0)
            cand = np.full((len(rows_), max(width, 1)), -1, dtype=np.int64)
            for b, c in enumerate(rows_):
                cand[b, :len(c)] = c
        if cand.ndim != 2 or cand.shape[0] != B or cand.shape[1] < 1:
            raise ValueError(f"candidates: one list of item indices per user ([B={B}, C]), got shape {tuple(cand.shape)}")
        C = int(cand.shape[1])
        if C > self.WIDE_MAX_K:
            raise ValueError(f"score_candidates: C = {C} candidates per user, at most {self.WIDE_MAX_K}")
        N = C if top_n is None else int(top_n)
        if not 1 <= N <= C:
            raise ValueError(f"score_candidates(top_n={N}): 1 <= top_n <= C = {C}")
        n_items = int(trie.item_edges.shape[0])
        if bool(((cand < -1) | (cand >= n_items)).any()):
            raise ValueError(f"candidates: item indices must be in 0 .. {n_items - 1} (-1 = empty slot)")
        srt = np.sort(cand, axis=1)
        if bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()):
            raise ValueError("candidates: the same item twice in one user's list")
        start = self.config.decoder_start_token_id
        plan = trie.rank_plan(start)
        if plan["levels"] > self.LUT_HALF:
            raise ValueError(f"score_candidates: items longer than {self.LUT_HALF} tokens")
        row_tok, row_depth, row_anc, item_rows, item_tokens = trie.cand_device_arrays(dev, start)
        path_len, ldt = int(item_rows.shape[1]), int(item_tokens.shape[1])
        cand_t = torch.from_numpy(cand.astype(np.int32)).to(dev)
        if whole_word_ids is None:
            whole_word_ids = torch.zeros_like(input_ids)
        whole_word_ids = self._i64(whole_word_ids, dev)
        if attention_mask is None:
            attention_mask = (input_ids != self.config.pad_token_id).long()
        attention_mask = self._i64(attention_mask, dev)
        self._sync_shadow()
        self._sync_transposed()
        lane = self._cur_lane()
        if self.compute_dtype == 1 and mode == "draft":
            engine, path = lane.engine, "cand_bf16"
        elif self.compute_dtype == 1:
            engine, path = self._verify_engine(lane), "cand_fp32"
        else:
            engine, path = lane.engine, "cand_fp32"
        need = lambda nb, rows: int(lib.p5_cand_workspace_bytes(engine, nb, L, C, path_len, rows))      # noqa: E731
        budget = int(self.rank_max_bytes)
        sp = self._be.stream_ptr()

        def fit(rows):          # users per pass
            if need(1, rows) > budget:
                what = f"one user's {rows} rows need" if rows else "the plan of one user's candidates needs"
                raise ValueError(f"score_candidates: {what} a workspace of {need(1, rows)} bytes, rank_max_bytes is {budget}")
            per = B
            while need(per, rows) > budget:
                per = max(1, min(per - 1, per * budget // need(per, rows)))
            return per

        def plan_users(cand_c, nb, nbytes):
            ws = self._lane_workspace(lane, nbytes, "cand")
            self._be.check(lib.p5_cand_plan(engine, _ptr(cand_c), nb, C, _ptr(item_rows), n_items, path_len, _ptr(ws), ws.numel(), sp), "p5_cand_plan")
            return ws

        # PLAN on the device; the one integer the host reads is the largest row count (it sizes the pass)
        per0, rows, ws = fit(0), 0, None
        for a in range(0, B, per0):
            nb = min(B, a + per0) - a
            ws = plan_users(cand_t[a:a + nb].contiguous(), nb, need(nb, 0))
            rows = max(rows, int(ws[:4].view(torch.int32).item()))
        rows = max(rows, 1)
        per = fit(rows)
        scores = torch.empty(B, C, dtype=torch.float32, device=dev)
        order = torch.empty(B, N, dtype=torch.int32, device=dev)
        index = torch.empty(B, N, dtype=torch.int32, device=dev)
        score = torch.empty(B, N, dtype=torch.float32, device=dev)

        def run(users, exact, planned=None):
            nb = int(users.numel())
            whole = nb == B and bool((users == torch.arange(B, device=users.device)).all())
            cut = lambda t: t if whole else t[users].contiguous()      # noqa: E731
            ids_c, ww_c, mask_c, cand_c = cut(input_ids), cut(whole_word_ids), cut(attention_mask), cut(cand_t)
            o_all = torch.empty(nb, C, dtype=torch.float32, device=dev)
            o_ord = torch.empty(nb, N, dtype=torch.int32, device=dev)
            o_idx = torch.empty(nb, N, dtype=torch.int32, device=dev)
            o_sc = torch.empty(nb, N, dtype=torch.float32, device=dev)
            flagged = torch.zeros(nb, dtype=torch.int32, device=dev)
            if planned is None:
                ws = plan_users(cand_c, nb, need(nb, rows))
            else:               # the plan made above leads the workspace: kept, or carried to the head of the larger one
                ws = self._lane_workspace(lane, need(nb, rows), "cand")
                if ws.data_ptr() != planned.data_ptr():
                    head = need(nb, 0)
                    ws[:head].copy_(planned[:head])
            self._be.check(lib.p5_cand_score(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, _ptr(row_tok), _ptr(row_depth), _ptr(row_anc),
                                             int(row_anc.shape[1]), _ptr(cand_c), C, _ptr(item_rows), _ptr(item_tokens), n_items, path_len, ldt, rows, N,
                                             1 if exact else 0, _ptr(o_all), _ptr(o_ord), _ptr(o_idx), _ptr(o_sc), _ptr(flagged), _ptr(ws), ws.numel(), sp),
                           "p5_cand_score")
            return o_all, o_ord, o_idx, o_sc, flagged

        rescored = 0
        for a in range(0, B, per):
            users = torch.arange(a, min(B, a + per), device=dev)
            o_all, o_ord, o_idx, o_sc, flagged = run(users, False, ws if (per == B and per0 >= B) else None)
            scores[users], order[users], index[users], score[users] = o_all, o_ord, o_idx, o_sc
            bad = users[flagged.nonzero().flatten()]
            if bad.numel():
                # a value of the split-product pass left the range of the two-term fp16 split: these users again, with exact fp32 products
                rescored += int(bad.numel())
                o_all, o_ord, o_idx, o_sc, flagged = run(bad, True)
                scores[bad], order[bad], index[bad], score[bad] = o_all, o_ord, o_idx, o_sc
        with self._stats_lock:
            st = self.cand_stats
            st["calls"] += 1; st["users"] += B; st["rescored_users"] += rescored; st["users_per_pass"] = per; st["rows_per_user"] = rows
        self.last_generate_path = path
        item_index = index.to(torch.int64)
        sequences = item_tokens[item_index.clamp(min=0)] * (item_index >= 0).unsqueeze(-1)       # (no candidate at this rank: the all-pad sequence)
        return {"scores": scores, "order": order.to(torch.int64), "item_index": item_index, "sequences": sequences.reshape(B * N, -1),
                "sequences_scores": score.reshape(B * N)}

    # ------------------------------------------------------------------ trie-constrained sampling (csrc/p5_sample.h)
    SAMPLE_MAX_S = 4096           # draws per user of one engine call (the decode step's rows-per-user limit); more go in draw ranges

    @staticmethod
    def _mix32(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    def _generate_sampled(self, input_ids, attention_mask, whole_word_ids, max_length, prefix_allowed_tokens_fn, num_beams, num_return_sequences,
                          output_scores, return_dict_in_generate, trie, roots, excluded, kw):
        """generate(do_sample=True, ...): the arguments HF users pass, checked against what is built, then `_sample`."""
        supported = "generate(do_sample=True) supports num_beams=1, num_return_sequences, temperature, excluded, seed, streams, draw_base"
        if int(num_beams) != 1:
            raise ValueError(f"generate(do_sample=True, num_beams={num_beams}): beam sampling is not built; {supported}")
        if kw.get("top_k") not in (None, 0):
            raise ValueError(f"generate(do_sample=True, top_k={kw.get('top_k')}): truncation is not wired into generate(), call "
                             f"sample_items(top_k=, top_p=); {supported}")
        if kw.get("top_p") not in (None, 1, 1.0):
            raise ValueError(f"generate(do_sample=True, top_p={kw.get('top_p')}): truncation is not wired into generate(), call "
                             f"sample_items(top_k=, top_p=); {supported}")
        if roots is not None:
            raise ValueError(f"generate(do_sample=True, roots=...): per-user roots are not built; {supported}")
        if trie is None and prefix_allowed_tokens_fn is not None:
            trie = find_trie(prefix_allowed_tokens_fn)
            if trie is None:
                raise ValueError(f"generate(do_sample=True): the prefix_allowed_tokens_fn must be made from a Trie (per-user roots are not built); {supported}")
        if trie is None:
            raise ValueError("generate() needs a trie / prefix_allowed_tokens_fn (OpenP5 always decodes under the item trie)")
        trie = self._compiled_trie(trie)
        excl_np = None
        if excluded is not None:
            excl_np = np.ascontiguousarray(excluded.cpu().numpy() if torch.is_tensor(excluded) else excluded, dtype=np.uint32)
        S = int(num_return_sequences or 1)
        seq, lp, _, _ = self._sample(input_ids, attention_mask, whole_word_ids, trie, S, float(kw.get("temperature") or 1.0), excl_np, kw.get("seed"),
                                     kw.get("streams"), int(kw.get("draw_base") or 0), max_length=max_length)
        B = seq.shape[0]
        sequences = seq.reshape(B * S, -1).to(torch.int64)
        if return_dict_in_generate:
            return {"sequences": sequences, "sequences_scores": lp.reshape(B * S) if output_scores else None}
        return sequences

    @torch.no_grad()
    def sample_items(self, input_ids=None, attention_mask=None, whole_word_ids=None, trie=None, num_samples: int = 1, temperature: float = 1.0,
                     excluded_items=None, seed: Optional[int] = None, streams=None, draw_base: int = 0, top_k: int = 0, top_p: float = 1.0):
        """Draw `num_samples` items per user from the model's distribution over the catalogue (on-policy samples for preference / policy-
        gradient fine-tuning, exploration, Monte-Carlo estimates).  What HF's sampling path computes under the item trie: at every step
        softmax(logits / temperature) renormalised over the allowed children of the prefix, one child drawn (Gumbel-max on the device,
        csrc/p5_sample.h), until </s>.  The draw runs on the model's own engine and dtype -- `generation_mode` does not apply -- and the
        returned log-probabilities are those of the distribution that was sampled.
        `excluded_items`: per-user lists of item indices (the order given to `CompiledTrie.index_items`; an unindexed trie is indexed on
        demand in lexicographic order) that have probability 0; the rest is renormalised.
        `seed` (None: a fresh one from a per-model counter seeded by the model's seed), `streams` (one uint32 id per user, default
        arange(B): pass dataset user ids to make a user's draws independent of batch composition) and `draw_base` (index of the first
        draw) are the coordinates of the counter-based uniforms (csrc/p5_rng.h): a draw is a pure function of (weights, the user's input,
        seed, stream, draw index), so user chunks (at most `wide_max_rows` decode rows per engine call) and draw ranges (`num_samples` >
        4096, or split by hand with `draw_base`) do not change a bit of the result.
        `top_k` (0 = off) / `top_p` (1 = off): HF's TopKLogitsWarper then TopPLogitsWarper on the allowed children, behind the temperature
        (csrc/p5_trunc.h): the k largest stay (ties at the k-th value all stay), then child i stays iff the probability mass strictly above
        it is < top_p -- by value, so equal logits stay or leave together (HF cuts inside such a group by sort position).  The returned
        log-probabilities are those of the truncated distribution (exactly 0 where one child is kept: top_k=1 is the greedy descent); a
        child's noise does not depend on the truncation, so a draw whose untruncated path stays inside the kept sets is the same draw.
        With both off the untruncated kernels run.  `forward(trie=, top_k=, top_p=)` is the loss of this distribution.
        Returns {"sequences" int64 [B * S, T] (decoder start first, pad-filled; T = depth of the trie), "sequences_logprob" fp32 [B * S]
        (-inf for a user with nothing to draw), "token_logprobs" fp32 [B * S, T - 1] (0 at forced-prefix positions and behind </s>),
        "item_index" int64 [B, S] (-1 for a user with nothing to draw; None for a trie with an appended trie, which cannot be indexed)}."""
        if trie is None:
            raise ValueError("sample_items() needs the item trie (Trie / CompiledTrie)")
        trie = self._compiled_trie(trie)
        S = int(num_samples)
        if S < 1:
            raise ValueError(f"sample_items(num_samples={num_samples}): at least one draw per user")
        if not trie.grafted and getattr(trie, "item_edges", None) is None:
            trie.index_items(trie.enumerate_items())
        excl_np = None
        if excluded_items is not None:
            if trie.grafted:
                raise ValueError("sample_items(excluded_items=...): a trie with an appended trie (Trie.append) cannot be indexed")
            excl_np = self._excluded_items_bitmap(trie, excluded_items, input_ids.shape[0])
        top_k, top_p = self._truncation(top_k, top_p)
        seq, lp, tok_lp, ln = self._sample(input_ids, attention_mask, whole_word_ids, trie, S, temperature, excl_np, seed, streams, draw_base, top_k=top_k,
                                           top_p=top_p)
        B, _, T = seq.shape
        item_index = None
        if not trie.grafted:
            item_index = self._sampled_item_index(trie, seq.reshape(B * S, T), ln.reshape(B * S)).view(B, S)
        return {"sequences": seq.reshape(B * S, T).to(torch.int64), "sequences_logprob": lp.reshape(B * S),
                "token_logprobs": tok_lp.reshape(B * S, T)[:, 1:].contiguous(), "item_index": item_index}

    def _sampled_item_index(self, trie, seq, ln):
        """item index of every drawn sequence [R, T] (ln [R] generated tokens): the trie walked on the device, one sorted lookup of
        (node, token) per position, then the item of the leaf reached; -1 where the draw did not reach a leaf"""
        dev = seq.device
        key = (str(dev), "sample")
        if key not in trie._dev_items:
            V = int(trie.child_tok.max()) + 1 if trie.child_tok.size else 1
            nodes = np.repeat(np.arange(trie.n_nodes, dtype=np.int64), np.diff(trie.child_off.astype(np.int64)))
            keys = nodes * V + trie.child_tok.astype(np.int64)
            order = np.argsort(keys, kind="stable")
            paths = trie.item_paths
            last = np.maximum((paths >= 0).sum(axis=1) - 1, 0)
            leaf_item = np.full(trie.n_nodes, -1, dtype=np.int64)
            leaf_item[paths[np.arange(paths.shape[0]), last]] = np.arange(paths.shape[0], dtype=np.int64)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
            trie._dev_items[key] = (V, t(keys[order]), t(trie.child_node.astype(np.int64)[order]), t(leaf_item))
        V, keys, edge_node, leaf_item = trie._dev_items[key]
        R, T = seq.shape
        node = torch.zeros(R, dtype=torch.int64, device=dev)
        ok = ln > 0
        tok = seq.to(torch.int64)
        for t in range(T):
            active = ok & (ln >= t)
            q = node * V + tok[:, t].clamp(max=V - 1)
            pos = torch.searchsorted(keys, q).clamp(max=keys.numel() - 1)
            hit = (keys[pos] == q) & (tok[:, t] < V)
            node = torch.where(active & hit, edge_node[pos], node)
            ok = ok & (hit | ~active)
        return torch.where(ok, leaf_item[node], torch.full_like(node, -1))

    @staticmethod
    def _excluded_items_bitmap(trie, excluded_items, B):
        """the excluded-node bitmap of per-user lists of item indices, checked"""
        if len(excluded_items) != B:
            raise ValueError(f"excluded_items: one list of item indices per user ({B}), got {len(excluded_items)}")
        n_items = int(trie.item_edges.shape[0])
        for b, items in enumerate(excluded_items):
            it = np.asarray(list(items), dtype=np.int64)
            if it.size and (it.min() < 0 or it.max() >= n_items):
                raise ValueError(f"excluded_items[{b}]: item indices must be in 0 .. {n_items - 1}")
        return trie.excluded_bitmap(excluded_items)

    def _sampling_setup(self, input_ids, attention_mask, whole_word_ids, trie, S, temperature, excl_np, seed, streams, base, base_name, max_length=None):
        """What sample_items and sample_slates share before their engine calls: the checked temperature, the inputs and the trie on the
        device, T, the stream ids, the index of the first draw / slate (`base`, S of them), the seed (None: the next of the per-model
        counter), the excluded-node bitmap and the forced-prefix rule with the users it leaves to the engine."""
        dev = self._be.device
        tau = float(temperature)
        if not (tau > 0.0 and math.isfinite(tau)):
            raise ValueError(f"temperature={temperature!r}: a finite value > 0")
        off, tok, nxt = trie.device_arrays(dev)
        input_ids = self._i64(input_ids, dev)
        B, L = input_ids.shape
        if whole_word_ids is None:
            whole_word_ids = torch.zeros_like(input_ids)
        whole_word_ids = self._i64(whole_word_ids, dev)
        if attention_mask is None:
            attention_mask = (input_ids != self.config.pad_token_id).long()
        attention_mask = self._i64(attention_mask, dev)
        depth = int(trie.max_depth)
        T = max(2, depth if max_length is None else min(int(max_length), depth))
        if T > 128:
            raise ValueError(f"sampling: items of {T} tokens, at most 128")
        if streams is None:
            st_np = np.arange(B, dtype=np.uint32)
        else:
            st_np = np.asarray(streams.cpu().numpy() if torch.is_tensor(streams) else streams).astype(np.int64).reshape(-1)
            if st_np.shape[0] != B:
                raise ValueError(f"streams: one id per user ({B}), got {st_np.shape[0]}")
            st_np = (st_np & 0xFFFFFFFF).astype(np.uint32)
        streams_t = torch.from_numpy(st_np.view(np.int32).copy()).to(dev)
        base = int(base)
        if base < 0 or base + S > 2 ** 32:
            raise ValueError(f"{base_name}={base}: {base_name.split('_')[0]} indices are uint32")
        if seed is None:
            with self._stats_lock:
                n = self._sample_calls
                self._sample_calls += 1
            seed = self._mix32(self._sample_seed0 + 0x9E3779B9 * (n + 1))
        seed = int(seed) & 0xFFFFFFFF
        excl_t, excl_words = None, 0
        if excl_np is not None:
            if excl_np.ndim != 2 or excl_np.shape[0] != B or excl_np.shape[1] * 32 < trie.n_nodes:
                raise ValueError(f"excluded bitmap must be [B={B}, >= {(trie.n_nodes + 31) // 32}] uint32, got {excl_np.shape}")
            excl_words = int(excl_np.shape[1])
            excl_t = torch.from_numpy(np.ascontiguousarray(excl_np).view(np.int32)).to(dev)
        self._sync_shadow()
        self._sync_transposed()
        # forced-prefix fast-forward, under generate()'s rule -- no user is fast-forwarded through an excluded node -- applied per user: every
        # item lies behind the chain, so a user whose exclusion touches it has nothing to draw and is answered here (-inf, the all-pad
        # sequence: what the kernel answers a user without an allowed child); the others keep the fast-forward, and their bits do not
        # depend on that user being in the batch
        ftok, fnode = [], []
        alive = np.arange(B)
        if self.prefix_fast_forward:
            ftok, fnode = trie.forced_prefix(self.config.decoder_start_token_id, self.config.eos_token_id)
            n = min(len(ftok), T - 2)
            ftok, fnode = (ftok[:n], fnode[:n]) if n >= 2 else ([], [])
            if ftok and excl_np is not None:
                words = excl_np[:, [x >> 5 for x in fnode]]
                bits = np.asarray([x & 31 for x in fnode], dtype=np.uint32)
                alive = np.nonzero(~((words >> bits[None, :]) & 1).any(axis=1))[0]
        return types.SimpleNamespace(tau=tau, off=off, tok=tok, nxt=nxt, input_ids=input_ids, whole_word_ids=whole_word_ids, attention_mask=attention_mask,
                                     B=B, L=L, T=T, streams_t=streams_t, base=base, seed=seed, excl_t=excl_t, excl_words=excl_words, ftok=ftok, fnode=fnode,
                                     alive=alive)

    def _sample(self, input_ids, attention_mask, whole_word_ids, trie, S, temperature, excl_np, seed, streams, draw_base, max_length=None, top_k=0,
                top_p=1.0):
        """The engine calls of sample_items / generate(do_sample=True): (sequences int32 [B, S, T], log-probability [B, S], per-position
        log-probabilities [B, S, T], generated tokens [B, S]).  `excl_np`: uint32 [B, words] excluded-node bitmap or None."""
        lib, dev = self._lib, self._be.device
        q = self._sampling_setup(input_ids, attention_mask, whole_word_ids, trie, S, temperature, excl_np, seed, streams, draw_base, "draw_base", max_length)
        tau, off, tok, nxt, input_ids, whole_word_ids, attention_mask = q.tau, q.off, q.tok, q.nxt, q.input_ids, q.whole_word_ids, q.attention_mask
        B, L, T, streams_t, draw_base, seed, excl_t, excl_words, ftok, fnode, alive = (q.B, q.L, q.T, q.streams_t, q.base, q.seed, q.excl_t, q.excl_words,
                                                                                       q.ftok, q.fnode, q.alive)
        lane = self._cur_lane()
        engine, sp = lane.engine, self._be.stream_ptr()
        maxc = max(1, trie.max_children)
        truncated = (0 < top_k < maxc) or top_p < 1.0        # (off: the untruncated entry point, the same bits)
        seq = torch.empty(B, S, T, dtype=torch.int32, device=dev)
        lp = torch.empty(B, S, dtype=torch.float32, device=dev)
        tok_lp = torch.empty(B, S, T, dtype=torch.float32, device=dev)
        ln = torch.empty(B, S, dtype=torch.int32, device=dev)
        nA = int(alive.size)
        if nA < B:
            seq.fill_(self.config.pad_token_id)
            seq[:, :, 0] = self.config.decoder_start_token_id
            lp.fill_(-math.inf)
            tok_lp.zero_()
            ln.zero_()
            alive_t = torch.from_numpy(alive).to(dev)
        # at most `wide_max_rows` decode rows per engine call: draw ranges of a user first, then users
        s_per = max(1, min(S, self.SAMPLE_MAX_S, int(self.wide_max_rows)))
        u_per = max(1, int(self.wide_max_rows) // s_per)
        calls = 0
        for s0 in range(0, S, s_per):
            sc = min(s_per, S - s0)
            for a in range(0, nA, u_per):
                b = min(nA, a + u_per)
                nb = b - a
                whole = nb == B and sc == S
                users = slice(a, b) if nA == B else alive_t[a:b]
                cut = lambda t: None if t is None else (t if nb == B else t[users].contiguous())      # noqa: E731
                o_seq = seq if whole else torch.empty(nb, sc, T, dtype=torch.int32, device=dev)
                o_lp = lp if whole else torch.empty(nb, sc, dtype=torch.float32, device=dev)
                o_tok = tok_lp if whole else torch.empty(nb, sc, T, dtype=torch.float32, device=dev)
                o_ln = ln if whole else torch.empty(nb, sc, dtype=torch.int32, device=dev)
                if ftok:
                    arr = (ctypes.c_int * len(ftok))
                    self._be.check(lib.p5_generate_set_forced_prefix(engine, arr(*ftok), arr(*fnode), len(ftok)), "p5_generate_set_forced_prefix")
                need = (lib.p5_sample_truncated_workspace_bytes if truncated else lib.p5_sample_workspace_bytes)(engine, nb, L, sc, T, maxc, excl_words)
                if need < 0:
                    self._be.check(-1, "p5_sample_truncated_workspace_bytes")
                ws = self._lane_workspace(lane, need, "sample")
                ids_c, ww_c, mask_c, ex_c, st_c = cut(input_ids), cut(whole_word_ids), cut(attention_mask), cut(excl_t), cut(streams_t)
                if truncated:
                    self._be.check(lib.p5_sample_items_truncated(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, sc, T, _ptr(off), _ptr(tok), _ptr(nxt),
                                                                 _ptr(ex_c), excl_words, maxc, seed, _ptr(st_c), (draw_base + s0) & 0xFFFFFFFF, tau, top_k,
                                                                 top_p, _ptr(o_seq), _ptr(o_lp), _ptr(o_tok), _ptr(o_ln), _ptr(ws), ws.numel(), sp),
                                   "p5_sample_items_truncated")
                else:
                    self._be.check(lib.p5_sample_items(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, sc, T, _ptr(off), _ptr(tok), _ptr(nxt), _ptr(ex_c),
                                                       excl_words, maxc, seed, _ptr(st_c), (draw_base + s0) & 0xFFFFFFFF, tau, _ptr(o_seq), _ptr(o_lp),
                                                       _ptr(o_tok), _ptr(o_ln), _ptr(ws), ws.numel(), sp), "p5_sample_items")
                if not whole:
                    seq[users, s0:s0 + sc], lp[users, s0:s0 + sc], tok_lp[users, s0:s0 + sc], ln[users, s0:s0 + sc] = o_seq, o_lp, o_tok, o_ln
                calls += 1
        with self._stats_lock:
            st = self.sample_stats
            st["calls"] += 1; st["users"] += B; st["engine_calls"] += calls; st["rows_per_call"] = min(nA, u_per) * s_per
            st["forced_prefix_steps"] = len(ftok)
        self.last_generate_path = "sample"
        return seq, lp, tok_lp, ln

    # ------------------------------------------------------------------ stochastic beam search (csrc/p5_sbs.h)
    SLATE_MAX_K = 4096            # beams of one slate, and decode rows per user of one engine call (slates x slate size)

    @torch.no_grad()
    def sample_slates(self, input_ids=None, attention_mask=None, whole_word_ids=None, trie=None, slate_size: int = 1, num_slates: int = 1,
                      temperature: float = 1.0, excluded_items=None, seed: Optional[int] = None, streams=None, slate_base: int = 0):
        """Draw `num_slates` slates of `slate_size` DISTINCT items per user: each slate is a sample without replacement from the
        distribution `sample_items` draws from, in sequential-sampling (Plackett-Luce) order -- exploration slates, on-policy lists for
        listwise / policy-gradient fine-tuning, without-replacement estimators.  Stochastic beam search (Kool, van Hoof, Welling 2019) on
        the item trie (csrc/p5_sbs.h): the slate is the top `slate_size` of log p(item) + Gumbel noise, found with `slate_size` decode rows.
        `excluded_items`, `seed`, `streams`, `temperature`: as `sample_items`; `slate_base` is the index of the first slate.  The perturbed
        value of an item is a pure function of (weights, the user's input, seed, stream, slate index): the slate of K' < K is the first K'
        entries of the slate of K, and user chunks (at most `wide_max_rows` decode rows per engine call; users first, then slate ranges, a
        slate is never split) or slate ranges split by hand with `slate_base` do not change a bit.  Tree-shaped tries only.
        Returns {"sequences" int64 [B * S * K, T], "sequences_logprob" fp32 [B * S * K] (log p(item)), "perturbed" fp32 [B, S, K]
        (descending, <= 0), "token_logprobs" fp32 [B * S * K, T - 1], "item_index" int64 [B, S, K]}.  A user with fewer than K allowed items
        gets trailing slots with the all-pad sequence, log-probability -inf, perturbed -inf and item_index -1.
        The search starts its root at G = 0, so `perturbed` are the values of a draw whose MAXIMUM is conditioned to be 0 (the first slot
        holds 0): the slate's distribution does not depend on that, a threshold taken from the values does.  "noise_key" = (seed, stream ids
        int32 [B] on the device, slate_base) is what `policy_slate_batch` un-conditions its threshold with."""
        if trie is None:
            raise ValueError("sample_slates() needs the item trie (Trie / CompiledTrie)")
        trie = self._compiled_trie(trie)
        if trie.grafted:
            raise ValueError("sample_slates(): a trie with an appended trie (Trie.append) is a DAG -- an edge reached by two prefixes would share "
                             "its noise between them; tree-shaped tries only")
        K, S = int(slate_size), int(num_slates)
        if K < 1 or K > self.SLATE_MAX_K:
            raise ValueError(f"sample_slates(slate_size={slate_size}): 1 <= slate_size <= {self.SLATE_MAX_K}")
        if S < 1:
            raise ValueError(f"sample_slates(num_slates={num_slates}): at least one slate per user")
        if K > int(self.wide_max_rows):
            raise ValueError(f"sample_slates(slate_size={K}): one slate needs {K} decode rows, more than wide_max_rows = {self.wide_max_rows}; a slate "
                             "cannot be split")
        if getattr(trie, "item_edges", None) is None:
            trie.index_items(trie.enumerate_items())
        excl_np = None
        if excluded_items is not None:
            excl_np = self._excluded_items_bitmap(trie, excluded_items, input_ids.shape[0])
        lib, dev = self._lib, self._be.device
        q = self._sampling_setup(input_ids, attention_mask, whole_word_ids, trie, S, temperature, excl_np, seed, streams, slate_base, "slate_base")
        tau, off, tok, nxt, input_ids, whole_word_ids, attention_mask = q.tau, q.off, q.tok, q.nxt, q.input_ids, q.whole_word_ids, q.attention_mask
        B, L, T, streams_t, slate_base, seed, excl_t, excl_words, ftok, fnode, alive = (q.B, q.L, q.T, q.streams_t, q.base, q.seed, q.excl_t, q.excl_words,
                                                                                        q.ftok, q.fnode, q.alive)
        lane = self._cur_lane()
        engine, sp = lane.engine, self._be.stream_ptr()
        maxc = max(1, trie.max_children)
        seq = torch.empty(B, S, K, T, dtype=torch.int32, device=dev)
        lp = torch.empty(B, S, K, dtype=torch.float32, device=dev)
        pert = torch.empty(B, S, K, dtype=torch.float32, device=dev)
        tok_lp = torch.empty(B, S, K, T, dtype=torch.float32, device=dev)
        ln = torch.empty(B, S, K, dtype=torch.int32, device=dev)
        nA = int(alive.size)
        if nA < B:
            seq.fill_(self.config.pad_token_id)
            seq[..., 0] = self.config.decoder_start_token_id
            lp.fill_(-math.inf)
            pert.fill_(-math.inf)
            tok_lp.zero_()
            ln.zero_()
            alive_t = torch.from_numpy(alive).to(dev)
        # at most `wide_max_rows` decode rows per engine call: users first, then slate ranges; a slate is never split
        s_per = max(1, min(S, self.SLATE_MAX_K // K, int(self.wide_max_rows) // K))
        u_per = max(1, int(self.wide_max_rows) // (s_per * K))
        calls = 0
        for s0 in range(0, S, s_per):
            sc = min(s_per, S - s0)
            for a in range(0, nA, u_per):
                b = min(nA, a + u_per)
                nb = b - a
                whole = nb == B and sc == S
                users = slice(a, b) if nA == B else alive_t[a:b]
                cut = lambda t: None if t is None else (t if nb == B else t[users].contiguous())      # noqa: E731
                o_seq = seq if whole else torch.empty(nb, sc, K, T, dtype=torch.int32, device=dev)
                o_lp = lp if whole else torch.empty(nb, sc, K, dtype=torch.float32, device=dev)
                o_pert = pert if whole else torch.empty(nb, sc, K, dtype=torch.float32, device=dev)
                o_tok = tok_lp if whole else torch.empty(nb, sc, K, T, dtype=torch.float32, device=dev)
                o_ln = ln if whole else torch.empty(nb, sc, K, dtype=torch.int32, device=dev)
                if ftok:
                    arr = (ctypes.c_int * len(ftok))
                    self._be.check(lib.p5_generate_set_forced_prefix(engine, arr(*ftok), arr(*fnode), len(ftok)), "p5_generate_set_forced_prefix")
                ws = self._lane_workspace(lane, lib.p5_sample_slates_workspace_bytes(engine, nb, L, sc, K, T, maxc, excl_words), "slates")
                ids_c, ww_c, mask_c, ex_c, st_c = cut(input_ids), cut(whole_word_ids), cut(attention_mask), cut(excl_t), cut(streams_t)
                self._be.check(lib.p5_sample_slates(engine, _ptr(ids_c), _ptr(ww_c), _ptr(mask_c), nb, L, sc, K, T, _ptr(off), _ptr(tok), _ptr(nxt),
                                                    _ptr(ex_c), excl_words, maxc, seed, _ptr(st_c), (slate_base + s0) & 0xFFFFFFFF, tau, _ptr(o_seq),
                                                    _ptr(o_lp), _ptr(o_pert), _ptr(o_tok), _ptr(o_ln), _ptr(ws), ws.numel(), sp), "p5_sample_slates")
                if not whole:
                    seq[users, s0:s0 + sc], lp[users, s0:s0 + sc], pert[users, s0:s0 + sc] = o_seq, o_lp, o_pert
                    tok_lp[users, s0:s0 + sc], ln[users, s0:s0 + sc] = o_tok, o_ln
                calls += 1
        with self._stats_lock:
            st = self.slate_stats
            st["calls"] += 1; st["users"] += B; st["engine_calls"] += calls; st["rows_per_call"] = min(nA, u_per) * s_per * K
            st["forced_prefix_steps"] = len(ftok)
        self.last_generate_path = "slates"
        R = B * S * K
        item_index = self._sampled_item_index(trie, seq.reshape(R, T), ln.reshape(R)).view(B, S, K)
        return {"sequences": seq.reshape(R, T).to(torch.int64), "sequences_logprob": lp.reshape(R), "perturbed": pert,
                "token_logprobs": tok_lp.reshape(R, T)[:, 1:].contiguous(), "item_index": item_index, "noise_key": (seed, streams_t, slate_base)}

    def _in_user_chunks(self, fn, args):
        """fn(*args) for a search wider than the narrow step, over consecutive chunks of users of at most `wide_max_rows` decode rows each,
        results concatenated.  The beam search of a user depends on that user alone and the decode step has one writer per output element,
        so the results are those of one call, bit for bit."""
        B, K = args[3], args[5]
        per = max(1, int(self.wide_max_rows) // K)
        if K <= self.NARROW_MAX_K or per >= B:
            return fn(*args)
        cut = lambda t, a, b: None if t is None else t[a:b].contiguous()     # noqa: E731
        outs = []
        for a in range(0, B, per):
            b = min(B, a + per)
            sub = list(args)
            sub[0], sub[1], sub[2], sub[3] = cut(args[0], a, b), cut(args[1], a, b), cut(args[2], a, b), b - a
            sub[10], sub[11] = cut(args[10], a, b), cut(args[11], a, b)        # per-user roots / excluded-node bitmap
            outs.append(fn(*sub))
        return tuple(torch.cat([o[i] for o in outs], 0) for i in range(3))

    def _search(self, engine, ws_attr, input_ids, whole_word_ids, attention_mask, B, L, K, max_length, off, tok, nxt, roots_t, excl_t, excl_words,
                maxc, hist=None):
        """One device beam search on `engine` (p5_generate; with `hist`, p5_generate_draft records what the search kept alive)."""
        dev = self._be.device
        lane = self._cur_lane()
        ftok, fnode = lane.forced
        if ftok:
            arr = (ctypes.c_int * len(ftok))
            self._be.check(self._lib.p5_generate_set_forced_prefix(engine, arr(*ftok), arr(*fnode), len(ftok)), "p5_generate_set_forced_prefix")
        ws = self._lane_workspace(lane, self._lib.p5_generate_workspace_bytes(engine, B, L, K, max_length, maxc, excl_words), ws_attr)
        seq = torch.zeros(B, K, max_length, dtype=torch.int32, device=dev)
        score = torch.zeros(B, K, dtype=torch.float32, device=dev)
        ln = torch.zeros(B, K, dtype=torch.int32, device=dev)
        if hist is None:
            self._be.check(self._lib.p5_generate(engine, _ptr(input_ids), _ptr(whole_word_ids), _ptr(attention_mask), B, L, K, max_length,
                                                 _ptr(off), _ptr(tok), _ptr(nxt), _ptr(roots_t), _ptr(excl_t), excl_words, maxc, _ptr(seq), _ptr(score), _ptr(ln),
                                                 _ptr(ws), ws.numel(), self._be.stream_ptr()), "p5_generate")
        else:
            self._be.check(self._lib.p5_generate_draft(engine, _ptr(input_ids), _ptr(whole_word_ids), _ptr(attention_mask), B, L, K, max_length,
                                                       _ptr(off), _ptr(tok), _ptr(nxt), _ptr(roots_t), _ptr(excl_t), excl_words, maxc, _ptr(seq), _ptr(score),
                                                       _ptr(ln), _ptr(hist), _ptr(ws), ws.numel(), self._be.stream_ptr()), "p5_generate_draft")
        return seq, score, ln

    # ------------------------------------------------------------------ verified generation (bf16 drafts, fp32 decides)
    def _verify_engine(self, lane):
        """fp32 engine over the SAME master parameter arena (no copy of the weights; its kernels read `_flat` directly), one per lane."""
        if not lane.engine_v:
            cfg = self._cfg_struct()
            cfg.dtype = 0
            lane.engine_v = ctypes.c_void_p()
            self._be.check(self._lib.p5_engine_create(ctypes.byref(cfg), ctypes.byref(lane.engine_v)), "p5_engine_create (verify)")
            self._be.check(self._lib.p5_engine_bind(lane.engine_v, _ptr(self._flat), _ptr(self._grads), None, _ptr(self._lut_enc), _ptr(self._lut_dec),
                                                     self.LUT_HALF, _ptr(self._rng)), "p5_engine_bind (verify)")
        return lane.engine_v

    def _generate_verified(self, input_ids, whole_word_ids, attention_mask, B, L, K, max_length, off, tok, nxt, roots_t, excl_t, excl_words, maxc, level=0):
        """include/p5hip.h "verified generation": the bf16 search with `verify_extra_beams` more beams proposes, ONE teacher-forced fp32
        pass over the distinct prefixes it kept alive scores them, and HF's beam search of the real width is replayed on those fp32 numbers.
        Users whose replay needed a prefix the draft had dropped are re-run through the plain fp32 search (counted in `verify_stats`)."""
        lib, dev, sp = self._lib, self._be.device, self._be.stream_ptr()
        extra = (int(self.verify_extra_beams),) + tuple(int(x) for x in self.verify_escalation)
        Kw = min(64, K + max(0, extra[min(level, len(extra) - 1)]))
        lane = self._cur_lane()
        ev = self._verify_engine(lane)
        common = (input_ids, whole_word_ids, attention_mask, B, L)
        trie_args = (off, tok, nxt, roots_t, excl_t, excl_words, maxc)
        ftok, fnode = lane.forced
        if ftok:      # (the replay skips the forced steps as the draft does)
            arr = (ctypes.c_int * len(ftok))
            self._be.check(lib.p5_generate_set_forced_prefix(ev, arr(*ftok), arr(*fnode), len(ftok)), "p5_generate_set_forced_prefix (verify)")
        ws = self._lane_workspace(lane, lib.p5_verify_workspace_bytes(ev, B, L, K, Kw, max_length, maxc, excl_words), "ver")
        self._be.check(lib.p5_verify_begin(ev, B, L, K, Kw, max_length, _ptr(off), _ptr(tok), _ptr(nxt), _ptr(roots_t), maxc, excl_words, _ptr(ws), ws.numel()),
                       "p5_verify_begin")
        # ONE encoder pass per batch: the fp32 one; the draft starts from its output
        self._be.check(lib.p5_verify_encode(ev, _ptr(input_ids), _ptr(whole_word_ids), _ptr(attention_mask), sp), "p5_verify_encode")
        if self.verify_share_encoder:
            self._be.check(lib.p5_generate_set_encoder_output(lane.engine, ctypes.c_void_p(lib.p5_verify_encoder_output(ev))), "p5_generate_set_encoder_output")
        # (carved out of the lane's workspace: its address is part of the decode-step graph's key, a fresh tensor per call would re-capture it)
        nh = int(lib.p5_generate_history_count(B, Kw, max_length))
        hist = self._lane_workspace(lane, nh * 4, "hist")[:nh * 4].view(torch.int32)
        hist.zero_()
        self._search(lane.engine, "gen", *common, Kw, max_length, *trie_args, hist=hist)
        self._be.check(lib.p5_verify_plan(ev, _ptr(hist), sp), "p5_verify_plan")
        hdr_off = int(lib.p5_verify_plan_header(ev)) - ws.data_ptr()
        hdr_dev = ws[hdr_off:hdr_off + 16].view(torch.int32)
        if ws.is_cuda:
            if lane.ver_hdr is None:
                lane.ver_hdr = torch.zeros(4, dtype=torch.int32).pin_memory()
            lane.ver_hdr.copy_(hdr_dev, non_blocking=True)      # the ONE number the host needs: rows per user of this batch
            torch.cuda.current_stream().synchronize()
            hdr = lane.ver_hdr.tolist()
        else:
            hdr = hdr_dev.cpu().tolist()
        if hdr[3]:
            raise RuntimeError("p5_verify_plan: row capacity exceeded")
        cap = int(lib.p5_verify_row_capacity(Kw, max_length))
        PU = min(cap, (max(1, int(hdr[0])) + 15) // 16 * 16)      # rows per user of the fp32 pass: the largest row count of the batch, in whole 16-row tiles
        st = self.verify_stats
        if PU > self.VERIFY_MAX_ROWS:
            # the users' rows are the queries of ONE cross-attention launch per layer (<= 512 queries per user): a deep, wide draft beyond that
            # goes to the plain fp32 search as a whole
            with self._stats_lock:
                st["calls"] += 1; st["users"] += B if level == 0 else 0; st["fallback_users"] += B
            return self._search_fp32(input_ids, whole_word_ids, attention_mask, B, L, K, max_length, *trie_args)
        seq = torch.zeros(B, K, max_length, dtype=torch.int32, device=dev)
        score = torch.zeros(B, K, dtype=torch.float32, device=dev)
        ln = torch.zeros(B, K, dtype=torch.int32, device=dev)
        missing = torch.zeros(B, dtype=torch.int32, device=dev)
        self._be.check(lib.p5_verify_run(ev, PU, _ptr(excl_t), _ptr(seq), _ptr(score), _ptr(ln), _ptr(missing), sp), "p5_verify_run")
        with self._stats_lock:
            st["calls"] += 1; st["users"] += B if level == 0 else 0; st["rows"] += int(hdr[2]); st["rows_per_user_max"] = max(st["rows_per_user_max"], int(hdr[0]))
            if level == 0:
                st["draft_beams"] = Kw
        miss = missing.nonzero().flatten()
        if miss.numel():
            sub = lambda t: None if t is None else t[miss].contiguous()     # noqa: E731
            nb = int(miss.numel())
            sub_args = (sub(input_ids), sub(whole_word_ids), sub(attention_mask), nb, L, K, max_length, off, tok, nxt, sub(roots_t), sub(excl_t), excl_words, maxc)
            if level + 1 < len(extra) and K + extra[level + 1] > Kw:
                # a flagged user first gets a WIDER draft (cheap: a sub-batch, ~2 ms) -- only what that cannot settle goes to the fp32 search
                with self._stats_lock:
                    st["escalated_users"] += nb
                s2, sc2, l2 = self._generate_verified(*sub_args, level=level + 1)
            else:
                # the fp32 search itself for these users (a prefix the fp32 search ranks among its K was not among the draft's Kw, or a
                # row of the split-product pass left the range the two-term fp16 split covers)
                with self._stats_lock:
                    st["fallback_users"] += nb
                s2, sc2, l2 = self._search_fp32(*sub_args)
            seq[miss] = s2; score[miss] = sc2; ln[miss] = l2
        return seq, score, ln

    def _search_fp32(self, *args):
        """The plain fp32 beam search on this lane's verification engine (exact fp32 MFMAs over the master arena): the last resort of the
        verified mode and what a verified call wider than VERIFY_MAX_K beams runs."""
        ev = self._verify_engine(self._cur_lane())
        return self._search(ev, "gen_v", *args)

    def time_generate(self, enable: bool = True):
        """Benchmark aid: arm (or disarm) the engine's device-time brackets around the next `generate` calls (two event records per
        call, nothing is waited for until `last_generate_timing` is read)."""
        self._be.check(self._lib.p5_generate_timing(self._engine, 1 if enable else 0, None, None), "p5_generate_timing")
        self._gen_timed = bool(enable)

    def last_generate_timing(self):
        """{"encode_ms", "decode_ms", "forced_prefix_steps"} of the calling thread's most recent `generate` call made while `time_generate()`
        was armed: device time of the encoder pass + cross-attention K/V projections (+ the forced-prefix pass), and of the decode loop
        alone (waits for that call to finish); the number of steps the forced-prefix pass covered.  None if not armed."""
        if not getattr(self, "_gen_timed", False):
            return None
        a, b = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._be.check(self._lib.p5_generate_timing(self._engine, 1, ctypes.byref(a), ctypes.byref(b)), "p5_generate_timing")
        return {"encode_ms": float(a.value), "decode_ms": float(b.value), "forced_prefix_steps": len(self._cur_lane().forced[0])}

    def _explore_callable(self, fn, B, max_length):
        """Compat path for an arbitrary prefix_allowed_tokens_fn(batch_id, prefix): enumerate it breadth-first into one
        CSR trie per batch item (as many Python calls as trie nodes, once per generate call)."""
        off, tok, nxt, roots = [0], [], [], []
        queue = []
        for b in range(B):
            roots.append(len(queue) + 0)
            queue.append((b, []))
        next_id = len(queue)
        qi = 0
        while qi < len(queue):
            b, prefix = queue[qi]
            qi += 1
            kids = [] if (len(prefix) >= max_length or (prefix and prefix[-1] == self.config.eos_token_id)) else \
                (sorted(set(int(t) for t in fn(b, torch.tensor(prefix, dtype=torch.long)))) if prefix else [self.config.decoder_start_token_id])
            for t in kids:
                tok.append(t)
                nxt.append(next_id)
                next_id += 1
                queue.append((b, prefix + [t]))
            off.append(len(tok))
        ct = CompiledTrie(np.asarray(off), np.asarray(tok), np.asarray(nxt))
        ct._roots = roots
        return ct

    def __del__(self):
        try:
            if self._engine:
                self._lib.p5_engine_destroy(self._engine)
            self._drop_lanes()
        except Exception:
            pass
