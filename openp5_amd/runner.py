"""Trainer / evaluator for the T5 path -- the same contract as the reference's `DistributedRunner`
(/root/reference/src/src_t5/runner/DistributedRunner.py:21-400 on top of SingleRunner.py:13-233), with its flags.

Differences, all deliberate:
  * world_size == 1 works (the reference's SingleRunner is broken as shipped);
  * gradients ARE averaged across ranks: the reference wraps the model in DDP but calls `.module(...)`, so its reducer
    never fires; here the backward all-reduces contiguous buckets of the flat gradient arena while it is still running;
  * clip + AdamW + schedule is the fused arena optimizer (same arithmetic: HF AdamW, wd on every parameter, linear warmup);
  * no per-step barriers / loss all-reduce (loss is all-reduced once per logging interval);
  * the trie constraint runs on the device (the model recognises our and the reference's prefix_allowed_tokens_fn).
"""
import logging
import math
import time

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from . import evaluate
from .collator import Collator, TestCollator
from .data import TestDataset
from .optim import FusedAdamW
from .trie import CompiledTrie, Trie, prefix_allowed_tokens_fn


def parse_runner_args(parser):
    parser.add_argument("--optim", type=str, default="AdamW", help="The name of the optimizer")
    parser.add_argument("--epochs", type=int, default=10)
    parser.add_argument("--lr", type=float, default=1e-3)
    parser.add_argument("--clip", type=float, default=1)
    parser.add_argument("--logging_step", type=int, default=100)
    parser.add_argument("--warmup_prop", type=float, default=0.05)
    parser.add_argument("--gradient_accumulation_steps", type=int, default=1)
    parser.add_argument("--weight_decay", type=float, default=0.01)
    parser.add_argument("--adam_eps", type=float, default=1e-6)
    parser.add_argument("--dropout", type=float, default=0.1)
    parser.add_argument("--alpha", type=float, default=2)
    parser.add_argument("--train", type=int, default=1, help="train or not")
    parser.add_argument("--backbone", type=str, default="t5-small", help="backbone model name")
    parser.add_argument("--metrics", type=str, default="hit@5,hit@10,ndcg@5,ndcg@10", help="Metrics used for evaluation")
    parser.add_argument("--load", type=int, default=0, help="load model from model path or not.")
    parser.add_argument("--random_initialize", type=int, default=1, help="Randomly initialize number-related tokens.")
    parser.add_argument("--test_epoch", type=int, default=1, help="test once for how many epochs, 0 for no test during training.")
    parser.add_argument("--valid_select", type=int, default=0, help="use validation loss to select models")
    parser.add_argument("--test_before_train", type=int, default=1, help="whether test before training")
    parser.add_argument("--test_filtered", type=int, default=0, help="whether filter out the items in the training data.")
    parser.add_argument("--test_filtered_batch", type=int, default=1, help="whether testing with filtered data in batch (1 = the reference's widened beam, "
                        "up to 4096 beams; 2 = history excluded inside the search, any history length; 0 = per-user protocol).")
    parser.add_argument("--test_exhaustive", type=int, default=0, help="1 = rank the whole catalogue exactly instead of searching it "
                        "(P5T5Native.rank_items: one pass scores every item of the trie, then an exact top generate_num; with --test_filtered "
                        "the user's history is left out of the ranking, whichever --test_filtered_batch is set): the limit the widened-beam "
                        "protocol approaches, at any catalogue size and history length.  2 = the same ranking with rank_items(pruned=True): on a bf16 "
                        "model the bf16 pass proposes the prefixes worth fp32 numbers and a certificate proves the fp32 list complete "
                        "(users without one are ranked as under 1).  3 = the same ranking with rank_items(pruned=\"search\"): bounded trie search, for bf16 "
                        "and fp32 models, which scores the prefixes within reach of the last returned item instead of the catalogue and certifies "
                        "the list in the same way.  0 = the beam-search protocols, untouched.")
    parser.add_argument("--test_candidates", type=int, default=0, help="N > 0 = the sampled-candidates protocol: every test user is ranked on the gold "
                        "item + N negatives drawn uniformly, without replacement, from the items outside the user's history (all of them if fewer "
                        "exist) by a generator seeded from (--seed, dataset, user) alone, scored exactly in one pass (P5T5Native.score_candidates), "
                        "metrics over the top min(generate_num, N + 1).  Takes precedence over --test_filtered; not with --test_exhaustive 1.  "
                        "0 = off, nothing changes.")
    parser.add_argument("--gen_lanes", type=int, default=3, help="evaluation batches in flight (P5T5Native.map_lanes): each lane has its own search / "
                        "verification engines, workspaces and HIP stream over the one set of weights, so one batch's latency-bound beam search overlaps "
                        "the next one's; 1 = one batch at a time")
    parser.add_argument("--id_metrics", type=int, default=1, help="compare generated token ids with the gold ids on the device "
                        "instead of decoding to strings (same Hit/NDCG; 0 = the reference's string path).")
    parser.add_argument("--compute_dtype", type=str, default="bf16", help="bf16 (fast) or fp32 (parity) engine arithmetic")
    parser.add_argument("--ddp_bucket_dtype", type=str, default="fp32", help="fp32 | bf16: dtype of the gradient buckets the ranks exchange "
                        "(bf16 halves the bytes on the xGMI links; the sums are identical on every rank either way).")
    parser.add_argument("--train_item_loss", type=int, default=0, choices=[0, 1], help="1 = train (and validate) on the trie-normalised item loss: "
                        "at every target position the softmax is renormalised over the continuations that are items (one union trie over the "
                        "items of all training datasets), the likelihood of the distribution P5T5Native.sample_items / sample_slates draw from.  "
                        "0 = the full-vocabulary cross-entropy, untouched.")
    parser.add_argument("--item_loss_temperature", type=float, default=1.0, help="temperature of --train_item_loss 1 (logits / temperature)")
    parser.add_argument("--item_loss_top_k", type=int, default=0, help="top-k truncation of --train_item_loss 1: the loss of the distribution "
                        "sample_items(top_k=...) draws from (0 = off)")
    parser.add_argument("--item_loss_top_p", type=float, default=1.0, help="nucleus truncation of --train_item_loss 1 (sample_items(top_p=...)); "
                        "1.0 = off")
    parser.add_argument("--item_loss_head", type=str, default="dense", choices=["dense", "trie"], help="head of --train_item_loss 1: dense = the "
                        "tied head over the whole vocabulary; trie = over the distinct tokens of the item trie only (the same loss, no [B*T, V] "
                        "logits; P5T5Native.forward(item_head=...))")
    parser.add_argument("--item_loss_entropy_coef", type=float, default=0.0, help="--train_item_loss 1: the loss gains -coef * (masked mean of the exact "
                        "entropy of every target row's distribution over the allowed children of its trie node); 0 = off")
    parser.add_argument("--item_loss_kl_coef", type=float, default=0.0, help="--train_item_loss 1: the loss gains +coef * (masked mean of the exact "
                        "KL(policy || reference) over the same children); needs --item_loss_kl_ref; 0 = off")
    parser.add_argument("--item_loss_kl_ref", type=str, default="", choices=["", "init"], help="reference policy of --item_loss_kl_coef: init = a frozen "
                        "copy of the model's weights at the start of training (eval mode, same dtype, no optimizer, not data-parallel)")
    parser.add_argument("--train_policy_samples", type=int, default=0, help="S > 0 = on-policy fine-tuning (P5T5Native.policy_step; needs "
                        "--train_item_loss 1 and the native model): every step draws S items per user from the model's own distribution on the "
                        "item trie, rewards a draw that is the gold item with 1, and trains on the gold (--policy_sft_coef) and on the draws weighted "
                        "by their advantages (--policy_coef).  0 = off, nothing changes.")
    parser.add_argument("--policy_baseline", type=str, default="loo", choices=["loo", "mean", "grpo", "none"], help="advantage of a draw: its reward "
                        "minus the mean of the user's OTHER draws (loo, S >= 2), minus the user's mean (mean), that divided by the user's standard "
                        "deviation (grpo), or the reward itself (none)")
    parser.add_argument("--policy_coef", type=float, default=1.0, help="weight of the policy-gradient term")
    parser.add_argument("--policy_sft_coef", type=float, default=1.0, help="weight of the likelihood of the gold item (0 = the draws alone)")
    parser.add_argument("--policy_clip_eps", type=float, default=0.0, help="eps > 0 = the clipped-ratio (PPO / GRPO style) objective on the draws "
                        "(P5T5Native.policy_collect / policy_update): a draw whose probability ratio to the sampled policy left [1 - eps, 1 + eps_high] "
                        "on the side its advantage pushes to gets no gradient.  0 = off, nothing changes.")
    parser.add_argument("--policy_clip_eps_high", type=float, default=-1.0, help="upper clip range (negative = --policy_clip_eps)")
    parser.add_argument("--policy_ratio", type=str, default="token", choices=["token", "sequence"], help="per-token ratios, or one length-normalised "
                        "ratio per draw")
    parser.add_argument("--policy_epochs", type=int, default=1, help="E optimizer steps per sampled batch (E > 1 needs --policy_clip_eps > 0 and "
                        "--gradient_accumulation_steps 1); the schedule runs over batches x E steps")
    parser.add_argument("--policy_old_logprobs", type=str, default="sampler", choices=["sampler", "forward"], help="the sampled policy's "
                        "log-probabilities: the sampler's own (free), or recomputed by one training-path forward (the first update's ratio is then "
                        "exactly 1 without dropout)")
    parser.add_argument("--policy_token_sum", type=int, default=0, choices=[0, 1], help="1 = a draw's term is the SUM of its tokens' NLL (REINFORCE "
                        "proper) instead of their mean")
    parser.add_argument("--policy_slate_size", type=int, default=0, help="K > 0 = the on-policy step draws SLATES of K distinct items per user "
                        "(stochastic beam search; --train_policy_samples then counts slates) and weights them with the importance-weighted "
                        "without-replacement estimator (P5T5Native.policy_slate_batch).  Not with --item_loss_top_k / --item_loss_top_p or a "
                        "non-default --policy_baseline.  0 = off, nothing changes.")
    parser.add_argument("--policy_slate_estimator", type=str, default="normalized", choices=["normalized", "unbiased"], help="normalized = weights "
                        "and baseline normalised by the slate's own weight sum (biased, consistent, lower variance; K >= 2); unbiased = p / q alone")
    parser.add_argument("--train_preference", type=str, default="", choices=["", "pl", "ipo"], help="pl | ipo = preference fine-tuning "
                        "(P5T5Native.preference_step; needs --train_item_loss 1 and the native model): every step draws --pref_negatives items per user "
                        "from the model's own distribution on the item trie and trains the gold item against the draws that are not the gold item.  pl = "
                        "Plackett-Luce with --pref_depth (1 = softmax-DPO; one negative = DPO), ipo = IPO.  Not with --train_policy_samples, "
                        "--item_loss_top_k / --item_loss_top_p or the item-loss regularisers.  Empty = off, nothing changes.")
    parser.add_argument("--pref_negatives", type=int, default=4, help="S sampled negatives per user")
    parser.add_argument("--pref_beta", type=float, default=0.1, help="beta: the scale of the log-probability ratios (> 0)")
    parser.add_argument("--pref_depth", type=int, default=1, help="Plackett-Luce depth (1 = softmax-DPO; 0 = the full order)")
    parser.add_argument("--pref_sft_coef", type=float, default=0.0, help="weight of the gold item's masked-mean NLL beside the preference loss")
    parser.add_argument("--pref_length_normalize", type=int, default=0, choices=[0, 1], help="1 = sequence log-probabilities are divided by their "
                        "number of tokens")
    parser.add_argument("--pref_ref", type=str, default="init", choices=["init", "none"], help="reference policy: init = a frozen copy of the model's "
                        "weights when the runner is built; none = reference-free")
    parser.add_argument("--pref_negatives_mode", type=str, default="slate", choices=["slate", "sample"], help="slate = S distinct items per user "
                        "(stochastic beam search); sample = S i.i.d. draws")
    parser.add_argument("--resume", type=int, default=0, help="continue from <model_path>.resume when it exists (weights + optimizer "
                        "moments + schedule position + epoch/step + dropout and data-order state; the reference saves weights only).")
    parser.add_argument("--save_steps", type=int, default=0, help="with --resume: also write the resume file every N optimizer steps "
                        "(0 = at epoch ends only).")
    return parser


def build_arg_parser(description="OpenP5 (MI355X-native T5 path)"):
    """The reference's four flag groups merged (main.py:24-232: global, dataset, sampler, runner)."""
    import argparse
    from .data import MultiTaskDataset
    from .sampler import parse_sampler_args
    from .utils import utils
    parser = argparse.ArgumentParser(description=description)
    utils.parse_global_args(parser)
    MultiTaskDataset.parse_dataset_args(parser)
    parse_sampler_args(parser)
    parse_runner_args(parser)
    return parser


def masked_mean_loss(nll, output_attention):
    """DistributedRunner.py:72-77."""
    B, T = output_attention.shape
    m = (output_attention != 0).float()
    loss = nll.view(B, T) * m
    return (loss.sum(dim=1) / m.sum(dim=1).clamp(min=1)).mean()


def policy_seed(seed, step, micro, rank):
    """The sampling seed of an on-policy step: a pure function of (--seed, optimizer step index, micro-batch index, rank), so that a resumed
    run draws what the uninterrupted run would have drawn (no state of its own in the resume file)."""
    from .model import P5T5Native
    mix = P5T5Native._mix32
    return mix(mix(mix(mix(int(seed) + 0x9E3779B9) ^ (int(step) & 0xFFFFFFFF)) ^ (int(micro) & 0xFFFFFFFF)) ^ (int(rank) & 0xFFFFFFFF))


def training_step(model, optimizer, batch, alpha=2, micro=0, accum=1, item_loss=None, policy=None, preference=None):
    """One pass of the reference loop body (DistributedRunner.py:63-87): forward, masked-mean loss, backward, clip + AdamW +
    scheduler (fused), zero_grad.  `batch` = (input_ids, whole_word_ids, attention_mask, labels, output_attention) on the
    device.  With the native model the loss and its gradient seed are computed by the engine
    (`P5T5Native.loss_and_backward`: masked mean folded behind the CE kernel, no torch autograd graph); any other model
    goes through the generic torch path.

    `accum` > 1 = --gradient_accumulation_steps: micro-batch `micro` (0-based, within a group of `accum`) adds its gradients
    to the arena (every gradient kernel accumulates; the arena clear at the start of a backward is skipped), ranks exchange
    gradients on the LAST micro-batch only, and the optimizer steps once per group on the group mean (1/accum folded into the
    AdamW gradient scale).  The reference only divides total_steps by this flag and still steps every batch
    (SingleRunner.py:182), which drives its schedule to lr = 0 after 1/accum of the run; this is the intended behaviour.

    `item_loss` (None = the full-vocabulary cross-entropy): keyword arguments of the native model's trie-normalised item loss --
    {"trie": ..., "temperature": ...[, "top_k": ..., "top_p": ...]} (`P5T5Native.forward`); with "entropy_coef" / "kl_coef" (native model
    only) the loss gains the regularisers of `P5T5Native.loss_and_backward`, and "ref_model" (a frozen `P5T5Native`) supplies the
    reference's `item_logits` of the batch when kl_coef != 0.

    `policy` (None = off): keyword arguments of `P5T5Native.policy_step` on top of `item_loss` -- {"num_samples", "baseline", "policy_coef",
    "sft_coef", "token_sum", "seed"} and, for slates, {"slate_size", "slate_estimator"}: the step samples, rewards, weights and trains in
    one call.

    `preference` (None = off): keyword arguments of `P5T5Native.preference_step` on top of `item_loss` -- {"num_negatives", "preference",
    "pref_depth", "pref_beta", "pref_sft_coef", "pref_length_normalize", "ref_model", "negatives", "seed"}."""
    kw = dict(item_loss or {})
    input_ids, whole_ids, attn, output_ids, output_attention = batch[:5]
    fused = getattr(model, "loss_and_backward", None)
    ref_model = kw.pop("ref_model", None)
    if fused is None and [kw.pop(k, 0.0) for k in ("entropy_coef", "kl_coef")] != [0.0, 0.0]:
        raise ValueError("item-loss regularisers (entropy_coef / kl_coef) need the native model")
    if ref_model is not None and kw.get("kl_coef", 0.0) != 0.0 and policy is None:
        kw["ref_logits"] = ref_model.item_logits(input_ids, whole_ids, attn, output_ids, kw["trie"], temperature=kw.get("temperature", 1.0),
                                                 item_head=kw.get("item_head"))
    last = micro == accum - 1
    if fused is not None and hasattr(model, "begin_micro_batch"):
        model.begin_micro_batch(first=micro == 0, sync=last)
    if policy is not None:
        if not hasattr(model, "policy_step") or "trie" not in kw:
            raise ValueError("the on-policy step needs the native model and the item loss's keywords (trie=...)")
        kw.pop("ref_logits", None)         # (policy_step takes the reference's logits on the grouped labels itself)
        loss = model.policy_step(input_ids, whole_ids, attn, output_ids, output_attention, ref_model=ref_model, **kw, **policy)
    elif preference is not None:
        if not hasattr(model, "preference_step") or "trie" not in kw:
            raise ValueError("the preference step needs the native model and the item loss's keywords (trie=...)")
        loss = model.preference_step(input_ids, whole_ids, attn, output_ids, output_attention, **kw, **preference)
    elif fused is not None:
        loss = fused(input_ids, whole_ids, attn, output_ids, output_attention, **kw)
    else:
        out = model(input_ids=input_ids, whole_word_ids=whole_ids, attention_mask=attn, labels=output_ids, alpha=alpha, return_dict=True, **kw)
        loss = masked_mean_loss(out["loss"], output_attention)
        (loss / accum if accum > 1 else loss).backward()
    if last:
        if accum > 1 and fused is not None:
            optimizer.step(grad_accum=accum)
        else:
            optimizer.step()          # clip_grad_norm_ + AdamW + scheduler.step, fused
        model.zero_grad()
    return loss.detach()


def policy_clip_steps(model, optimizer, batch, item_loss, policy, clip):
    """One sampled batch of the clipped-ratio objective with E = clip["epochs"] optimizer steps: `P5T5Native.policy_collect` once, then E x
    (`policy_update`, clip + AdamW + scheduler, zero_grad).  `policy`: the keywords of `training_step`'s `policy` (with "seed"); `clip`:
    {"clip_eps", "ratio", "old_logprobs", "epochs"}.  Returns (mean loss of the E updates, their `last_clip_stats` stacked [E, 8]), on the
    device, no host sync."""
    kw = dict(item_loss or {})
    if not hasattr(model, "policy_collect") or "trie" not in kw:
        raise ValueError("the clipped policy objective needs the native model and the item loss's keywords (trie=...)")
    input_ids, whole_ids, attn, output_ids, output_attention = batch[:5]
    ref_model = kw.pop("ref_model", None)
    kw.pop("ref_logits", None)
    rollout = model.policy_collect(input_ids, whole_ids, attn, output_ids, output_attention, ref_model=ref_model, clip_eps=clip["clip_eps"],
                                   ratio=clip["ratio"], old_logprobs=clip["old_logprobs"], **kw, **policy)
    upd = {k: v for k, v in kw.items() if k in ("temperature", "excluded_items", "item_head", "entropy_coef", "kl_coef")}
    losses, stats = [], []
    for _ in range(int(clip["epochs"])):
        model.begin_micro_batch(first=True, sync=True)
        losses.append(model.policy_update(input_ids, whole_ids, attn, rollout, kw["trie"], clip["clip_eps"], ratio=clip["ratio"], **upd).detach())
        stats.append(model.last_clip_stats)
        optimizer.step()
        model.zero_grad()
    return torch.stack(losses).mean(), torch.stack(stats)


class Prefetcher:
    """Background collation: the DataLoader (tokenisation + whole-word ids, num_workers=0 as in main.py:61) runs in a thread
    and stays `depth` batches ahead, so host-side batch preparation overlaps the asynchronously issued GPU step instead of
    serialising with it (the reference collates in the training loop)."""

    def __init__(self, loader, depth=3, pin=False):
        import queue
        import threading
        self.q = queue.Queue(maxsize=depth)
        self.pin = pin
        self._done = object()
        self.err = None

        def work():
            try:
                for batch in loader:
                    if self.pin:
                        batch = [t.pin_memory() if torch.is_tensor(t) else t for t in batch]
                    self.q.put(batch)
            except BaseException as e:   # surfaced in the consumer
                self.err = e
            self.q.put(self._done)

        self.t = threading.Thread(target=work, daemon=True)
        self.t.start()

    def __iter__(self):
        while True:
            item = self.q.get()
            if item is self._done:
                if self.err is not None:
                    raise self.err
                return
            yield item


MAX_DEVICE_BEAMS = 4096    # include/p5hip.h: p5_generate keeps <= 4096 beams per batch item (the wide search beyond 64)


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class DistributedRunner:
    parse_runner_args = staticmethod(parse_runner_args)

    def __init__(self, model, tokenizer, train_loader, valid_loader, device, args, rank=0):
        self.model, self.tokenizer = model, tokenizer
        self.train_loader, self.valid_loader = train_loader, valid_loader
        self.device, self.args, self.rank = device, args, rank
        self.world = _world()
        self.model.ddp_world = self.world          # gradient all-reduce inside the staged backward
        self.model.ddp_bucket_dtype = getattr(args, "ddp_bucket_dtype", "fp32")
        ds0 = self.train_loader.dataset.datasets[0] if train_loader is not None else None
        self.regenerate_candidate = ds0 is not None and "candidate_items" in ds0.info
        self.reconstruct_data = args.sample_prompt
        self.test_epoch, self.valid_select = args.test_epoch, args.valid_select
        self.test_before_train = args.test_before_train
        self.test_filtered, self.test_filtered_batch = args.test_filtered, args.test_filtered_batch
        self.test_exhaustive = int(getattr(args, "test_exhaustive", 0))
        self.test_candidates = int(getattr(args, "test_candidates", 0))
        if self.test_candidates < 0:
            raise ValueError(f"--test_candidates {self.test_candidates}: the number of sampled negatives per user (0 = off)")
        if self.test_candidates > 0 and self.test_exhaustive:
            raise ValueError("--test_candidates N ranks the gold item among N sampled negatives, --test_exhaustive 1 ranks the whole catalogue: "
                             "choose one of the two protocols")
        self.id_metrics = int(getattr(args, "id_metrics", 1))
        self.gen_lanes = int(getattr(args, "gen_lanes", 3))
        self.metrics = args.metrics.split(",")
        self.generate_num = max(int(m.split("@")[1]) for m in self.metrics)
        self.get_testloader()
        self._policy = self._policy_flags()          # (raises now, not at the first step)
        self._pref = self._pref_flags()
        if args.train:
            self.optimizer, self.scheduler = self.create_optimizer_and_scheduler()
        self.samples_per_sec = None
        self.items_per_sec = None

    # ------------------------------------------------------------------ setup
    def create_optimizer_and_scheduler(self):
        batch_per_epoch = len(self.train_loader)
        # one optimizer step per group of `accum` batches, the trailing (shorter) group of an epoch included
        total_steps = math.ceil(batch_per_epoch / max(1, self.args.gradient_accumulation_steps)) * self.args.epochs
        if getattr(self, "_policy_clip", None) is not None:
            total_steps *= self._policy_clip["epochs"]          # (E optimizer steps per sampled batch)
        warmup_steps = int(total_steps * self.args.warmup_prop)
        if self.rank == 0:
            logging.info(f"Batch per epoch: {batch_per_epoch}; total steps: {total_steps}; warm up steps: {warmup_steps}")
        if self.args.optim.lower() != "adamw":
            raise NotImplementedError(self.args.optim)
        opt = FusedAdamW(self.model, lr=self.args.lr, eps=self.args.adam_eps, weight_decay=self.args.weight_decay,
                         max_grad_norm=self.args.clip, warmup_steps=warmup_steps, total_steps=total_steps)
        return opt, opt      # the fused optimizer advances its own linear-warmup schedule

    def get_testloader(self):
        self.testloaders = []
        collator = (TestCollator(self.tokenizer, solo_rows=(self.test_filtered_batch == 0)) if self.test_filtered > 0
                    else TestCollator(self.tokenizer) if self.test_candidates > 0 else Collator(self.tokenizer))
        for dataset in self.args.datasets.split(","):
            for task in self.args.tasks.split(","):
                testdata = TestDataset(self.args, dataset, task)
                sampler = DistributedSampler(testdata, num_replicas=self.world, rank=self.rank) if self.world > 1 else None
                self.testloaders.append(DataLoader(dataset=testdata, sampler=sampler, batch_size=self.args.eval_batch_size,
                                                   collate_fn=collator, shuffle=False))

    def _to_dev(self, batch):
        return [t.to(self.device, non_blocking=True) if torch.is_tensor(t) else t for t in batch]

    # ------------------------------------------------------------------ resume state
    def _resume_path(self):
        return str(self.args.model_path) + ".resume"

    def _epoch_start_state(self):
        """Everything the data order of an epoch is derived from, captured BEFORE the epoch's prompt re-sampling and in-place
        cumulative shuffle (MultiTaskDataset.py:189-195): restoring it and replaying the epoch's setup reproduces the batch
        stream exactly, so a mid-epoch resume only has to skip the batches already consumed."""
        import random
        # (plain containers + tensors only, so that the resume file loads with torch.load(weights_only=True))
        pv, pk, pg = random.getstate()
        nn, nk, npos, nhas, ncached = np.random.get_state()
        state = {"py_random": [int(pv), [int(x) for x in pk], pg], "np_random": [str(nn), torch.from_numpy(nk.astype(np.int64)), int(npos), int(nhas), float(ncached)],
                 "torch_rng": torch.get_rng_state()}
        if self.train_loader is not None:
            state["task_data"] = [{t: list(v) for t, v in ds.task_data.items()} for ds in self.train_loader.dataset.datasets]
        return state

    def _restore_epoch_start(self, state):
        import random
        pv, pk, pg = state["py_random"]
        random.setstate((pv, tuple(pk), pg))
        nn, nk, npos, nhas, ncached = state["np_random"]
        np.random.set_state((nn, nk.numpy().astype(np.uint32), npos, nhas, ncached))
        torch.set_rng_state(state["torch_rng"])
        for ds, td in zip(self.train_loader.dataset.datasets, state.get("task_data", [])):
            ds.task_data = {t: list(v) for t, v in td.items()}

    def save_checkpoint(self, path, epoch, step_in_epoch, epoch_start, extra=None):
        """Weights (HF key layout, as utils.save_model) + optimizer moments / step / schedule position + epoch, step inside
        the epoch, dropout counter and the epoch-start data state.  Written by rank 0: parameters and optimizer state are
        identical on every rank (all-reduced gradients, deterministic clip factor), the Python / NumPy / torch RNG states that
        drive the data order are identical by construction (every rank seeds them alike and draws the same sequence; the
        samplers shard AFTER shuffling, DistMultiDataTaskSampler.py:30-33).  The dropout counter is the one piece of state a
        launcher may seed per rank (bench.py, tests/test_gpu_ddp.py do): it is gathered from all ranks and restored per rank."""
        rng = [int(x) for x in getattr(self.model, "_rng_cpu", [0, 0])]
        rng_ranks = [rng]
        if self.world > 1:
            parts = [None] * self.world          # (through the object channel: no device-tensor collective, works on every backend)
            dist.all_gather_object(parts, rng)
            rng_ranks = [[int(v) for v in p] for p in parts]
        if self.rank != 0:
            return
        ck = {"model": {k: v.detach().cpu() for k, v in self.model.state_dict().items()},
              "optimizer": {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in self.optimizer.state_dict().items()},
              "epoch": int(epoch), "step_in_epoch": int(step_in_epoch), "epoch_start": epoch_start,
              "dropout_rng": rng, "dropout_rng_ranks": rng_ranks, "world": self.world}
        ck.update(extra or {})
        tmp = str(path) + ".tmp"
        torch.save(ck, tmp)
        import os
        os.replace(tmp, path)

    def load_checkpoint(self, path):
        ck = torch.load(path, map_location="cpu", weights_only=True)     # tensors and plain containers only: nothing is unpickled
        self.model.load_state_dict(ck["model"], strict=False)
        self.optimizer.load_state_dict(ck["optimizer"])
        if hasattr(self.model, "set_dropout_seed"):
            ranks = ck.get("dropout_rng_ranks") or [ck["dropout_rng"]]
            self.model.set_dropout_seed(*(ranks[self.rank] if self.rank < len(ranks) and ck.get("world") == self.world else ck["dropout_rng"]))
        return ck

    # ------------------------------------------------------------------ training
    def train(self):
        import os
        self.model.zero_grad()
        train_losses, valid_losses, best_epoch = [], [], -1
        accum = max(1, int(self.args.gradient_accumulation_steps))
        resume = int(getattr(self.args, "resume", 0)) > 0
        save_steps = int(getattr(self.args, "save_steps", 0))
        start_epoch, skip_batches, pending_start = 0, 0, None
        carry_sum, carry_cnt = 0.0, 0          # loss of the batches of a resumed epoch that ran before the checkpoint was written
        if resume and os.path.exists(self._resume_path()):
            ck = self.load_checkpoint(self._resume_path())
            start_epoch, skip_batches, pending_start = ck["epoch"], ck["step_in_epoch"], ck["epoch_start"]
            carry_sum, carry_cnt = float(ck.get("loss_sum", 0.0)), int(ck.get("loss_cnt", 0))
            train_losses, valid_losses, best_epoch = ck.get("train_losses", []), ck.get("valid_losses", []), ck.get("best_epoch", -1)
            if self.rank == 0:
                logging.info(f"Resume from {self._resume_path()}: epoch {start_epoch + 1}, batch {skip_batches}, optimizer step {self.optimizer.t}")
        elif self.test_before_train > 0:
            self.test()
        for epoch in range(start_epoch, self.args.epochs):
            if self.rank == 0:
                logging.info(f"Start training for epoch {epoch + 1}")
            if pending_start is not None:
                self._restore_epoch_start(pending_start)
            epoch_start = self._epoch_start_state() if resume else None
            pending_start = None
            if self.regenerate_candidate or self.reconstruct_data:
                for ds in self.train_loader.dataset.datasets:
                    if self.regenerate_candidate and hasattr(ds, "generate_candidates"):
                        ds.generate_candidates()
                    ds.construct_sentence()
            if hasattr(self.train_loader.sampler, "set_epoch"):
                self.train_loader.sampler.set_epoch(epoch)
            self.model.train()
            losses, n_samples, n_batches = [], 0, 0
            n_total = len(self.train_loader)
            t0 = time.perf_counter()
            for batch in Prefetcher(self.train_loader, pin=torch.cuda.is_available()):
                n_batches += 1
                if n_batches <= skip_batches:         # already consumed before the checkpoint was written
                    continue
                input_ids, attn, whole_ids, output_ids, output_attention = self._to_dev(batch)[:5]
                # groups of `accum` batches; the LAST group of the epoch may be shorter -- its last batch is still the one that
                # exchanges gradients across ranks and steps (on the mean over the group's actual size), so every rank applies the
                # same update (a partial group stepped on rank-local sums would let the replicas drift apart for good)
                g0 = (n_batches - 1) // accum * accum
                gsize = min(accum, n_total - g0)
                micro = n_batches - 1 - g0
                if self._pref is not None:
                    prf = dict(self._pref, seed=policy_seed(getattr(self.args, "seed", 0), self.optimizer.t, micro, self.rank))
                    loss = training_step(self.model, self.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), self.args.alpha,
                                         micro=micro, accum=gsize, item_loss=self._item_loss_kw(), preference=prf)
                    # (the one host read, once per --logging_step batches, as for the on-policy step)
                    if self.rank == 0 and n_batches % max(1, int(self.args.logging_step)) == 0:
                        st = [float(x) for x in self.model.last_pref_stats.cpu()]
                        logging.info(f"preference step {self.optimizer.t} batch {n_batches}: loss {float(loss):.6f} "
                                     + " ".join(f"{k} {v:.4f}" for k, v in zip(self.model.PREF_STATS, st)))
                elif self._policy is None:
                    loss = training_step(self.model, self.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), self.args.alpha,
                                         micro=micro, accum=gsize, item_loss=self._item_loss_kw())
                else:
                    pol = dict(self._policy, seed=policy_seed(getattr(self.args, "seed", 0), self.optimizer.t, micro, self.rank))
                    clip_stats = None
                    if self._policy_clip is None:
                        loss = training_step(self.model, self.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), self.args.alpha,
                                             micro=micro, accum=gsize, item_loss=self._item_loss_kw(), policy=pol)
                    elif accum > 1:           # (one update per batch: the accumulating step with the clipped objective inside policy_step)
                        cl = {k: v for k, v in self._policy_clip.items() if k != "epochs"}
                        loss = training_step(self.model, self.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention), self.args.alpha,
                                             micro=micro, accum=gsize, item_loss=self._item_loss_kw(), policy=dict(pol, **cl))
                        clip_stats = self.model.last_clip_stats[None]
                    else:
                        loss, clip_stats = policy_clip_steps(self.model, self.optimizer, (input_ids, whole_ids, attn, output_ids, output_attention),
                                                             self._item_loss_kw(), pol, self._policy_clip)
                    # the one host read of the statistics -- and of this batch's loss: this runner logs no per-batch loss elsewhere, so with the
                    # flag on rank 0 synchronises with the device once per --logging_step batches; with the flag off nothing is read
                    if self.rank == 0 and n_batches % max(1, int(self.args.logging_step)) == 0:
                        if "slate_size" in pol:
                            st = [float(x) for x in self.model.last_policy_stats.cpu()]
                            logging.info(f"policy slate step {self.optimizer.t} batch {n_batches}: loss {float(loss):.6f} "
                                         + " ".join(f"{k} {v:.4f}" for k, v in zip(self.model.SLATE_POLICY_STATS, st)))
                        else:
                            st = [float(x) for x in self.model.last_policy_stats[:6].cpu()]
                            logging.info(f"policy step {self.optimizer.t} batch {n_batches}: loss {float(loss):.6f} "
                                         + " ".join(f"{k} {v:.4f}" for k, v in zip(self.model.POLICY_STATS, st)))
                        if clip_stats is not None:
                            cs = [float(x) for x in clip_stats.mean(0).cpu()]
                            logging.info(f"policy clip step {self.optimizer.t} batch {n_batches} (mean of {clip_stats.shape[0]} updates): "
                                         + " ".join(f"{k} {v:.4f}" for k, v in zip(self.model.CLIP_STATS, cs)))
                losses.append(loss)
                n_samples += input_ids.shape[0]
                if resume and save_steps > 0 and micro == gsize - 1 and self.optimizer.t % save_steps == 0:
                    self.save_checkpoint(self._resume_path(), epoch, n_batches, epoch_start,
                                         {"train_losses": train_losses, "valid_losses": valid_losses, "best_epoch": best_epoch,
                                          "loss_sum": carry_sum + float(torch.stack(losses).sum()), "loss_cnt": carry_cnt + len(losses)})
            skip_batches = 0
            assert n_batches == n_total, (n_batches, n_total)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            self.samples_per_sec = self.world * n_samples / max(dt, 1e-9)
            epoch_loss = ((torch.stack(losses).sum() + carry_sum) / (len(losses) + carry_cnt) if losses
                          else torch.full((), carry_sum / max(1, carry_cnt), device=self.device))
            carry_sum, carry_cnt = 0.0, 0
            if self.world > 1:
                dist.all_reduce(epoch_loss, op=dist.ReduceOp.SUM)
                epoch_loss /= self.world
            if self.rank == 0:
                train_losses.append(float(epoch_loss))
                logging.info(f"The average training loss for epoch {epoch + 1} is {float(epoch_loss):.6f} ({self.samples_per_sec:.1f} samples/s)")
            if self.valid_select > 0:
                v = self.validate()
                if self.rank == 0:
                    valid_losses.append(v)
                    logging.info(f"The average valid loss for epoch {epoch + 1} is {v}")
                    if v == min(valid_losses):
                        best_epoch = epoch + 1
                        torch.save(self.model.state_dict(), self.args.model_path)
                        logging.info(f"Save the current model to {self.args.model_path}")
            if self.test_epoch > 0 and (epoch + 1) % self.test_epoch == 0:
                self.model.eval()
                self.test()
            if resume:
                # the next epoch starts from the data state as it is NOW (prompts re-sampled, lists permuted cumulatively)
                self.save_checkpoint(self._resume_path(), epoch + 1, 0, self._epoch_start_state(),
                                     {"train_losses": train_losses, "valid_losses": valid_losses, "best_epoch": best_epoch})
            if self.world > 1:
                dist.barrier()
        if self.rank == 0:
            if self.valid_select > 0:
                logging.info(f"The best validation at Epoch {best_epoch}")
            elif getattr(self.args, "model_path", None):
                torch.save(self.model.state_dict(), self.args.model_path)
                logging.info(f"Save the current model to {self.args.model_path}")
        return train_losses

    def _policy_flags(self):
        """--train_policy_samples S: the keyword arguments of `P5T5Native.policy_step` (None with the flag at 0), every flag checked here."""
        S = int(getattr(self.args, "train_policy_samples", 0))
        self._policy_clip = None
        eps = float(getattr(self.args, "policy_clip_eps", 0.0))
        eps_high = float(getattr(self.args, "policy_clip_eps_high", -1.0))
        E = int(getattr(self.args, "policy_epochs", 1))
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"--policy_clip_eps {eps}: a finite value >= 0 (0 = off)")
        if E < 1:
            raise ValueError(f"--policy_epochs {E}: at least one update per sampled batch")
        if E > 1 and eps == 0.0:
            raise ValueError(f"--policy_epochs {E} requires --policy_clip_eps > 0: updates behind the first are off-policy without the clipped ratio")
        if E > 1 and int(getattr(self.args, "gradient_accumulation_steps", 1)) > 1:
            raise ValueError(f"--policy_epochs {E} cannot be combined with --gradient_accumulation_steps > 1")
        if eps > 0.0 and S == 0:
            raise ValueError("--policy_clip_eps requires --train_policy_samples > 0")
        K = int(getattr(self.args, "policy_slate_size", 0))
        estimator = str(getattr(self.args, "policy_slate_estimator", "normalized"))
        if K < 0:
            raise ValueError(f"--policy_slate_size {K}: the number of items per slate (0 = off)")
        if K > 0 and S <= 0:
            raise ValueError("--policy_slate_size requires --train_policy_samples > 0 (the number of slates per user) and --train_item_loss 1")
        if K > 0 and estimator not in ("normalized", "unbiased"):
            raise ValueError(f"--policy_slate_estimator {estimator}: normalized or unbiased")
        if K == 1 and estimator == "normalized":
            raise ValueError("--policy_slate_estimator normalized needs --policy_slate_size >= 2 (use unbiased for slates of one item)")
        if S == 0:
            return None
        if eps > 0.0:
            if eps_high >= 0.0 and not math.isfinite(eps_high):
                raise ValueError(f"--policy_clip_eps_high {eps_high}: a finite value (negative = --policy_clip_eps)")
            if not hasattr(self.model, "policy_collect"):
                raise ValueError("--policy_clip_eps needs the native model (P5T5Native)")
            if int(getattr(self.args, "item_loss_top_k", 0) or 0) > 0 or float(getattr(self.args, "item_loss_top_p", 1.0) or 1.0) < 1.0:
                raise ValueError("--policy_clip_eps is not built for the truncated item loss (top_k / top_p)")
            self._policy_clip = {"clip_eps": (eps, eps_high if eps_high >= 0.0 else eps), "ratio": str(getattr(self.args, "policy_ratio", "token")),
                                 "old_logprobs": str(getattr(self.args, "policy_old_logprobs", "sampler")), "epochs": E}
        if S < 0:
            raise ValueError(f"--train_policy_samples {S}: the number of draws per user (0 = off)")
        if not int(getattr(self.args, "train_item_loss", 0)):
            raise ValueError("--train_policy_samples requires --train_item_loss 1 (the draws and the loss share the union item trie)")
        if not hasattr(self.model, "policy_step"):
            raise ValueError("--train_policy_samples needs the native model (P5T5Native)")
        baseline = str(getattr(self.args, "policy_baseline", "loo"))
        if baseline not in ("loo", "mean", "grpo", "none"):
            raise ValueError(f"--policy_baseline {baseline}: loo, mean, grpo or none")
        if K > 0:
            if baseline != "loo":
                raise ValueError(f"--policy_baseline {baseline} belongs to the plain draws: with --policy_slate_size the baseline is "
                                 "--policy_slate_estimator's (normalized = the slate's own weighted mean, unbiased = none)")
            if int(getattr(self.args, "item_loss_top_k", 0) or 0) > 0 or float(getattr(self.args, "item_loss_top_p", 1.0) or 1.0) < 1.0:
                raise ValueError("--policy_slate_size cannot be combined with --item_loss_top_k / --item_loss_top_p: the slate sampler has no "
                                 "truncation (use the plain draws, --policy_slate_size 0)")
            if not hasattr(self.model, "policy_slate_batch"):
                raise ValueError("--policy_slate_size needs the native model (P5T5Native)")
        elif baseline == "loo" and S < 2:
            raise ValueError("--policy_baseline loo needs --train_policy_samples >= 2")
        pc, sc = float(getattr(self.args, "policy_coef", 1.0)), float(getattr(self.args, "policy_sft_coef", 1.0))
        if not (math.isfinite(pc) and math.isfinite(sc)):
            raise ValueError(f"--policy_coef {pc} / --policy_sft_coef {sc}: finite values")
        pol = {"num_samples": S, "baseline": baseline, "policy_coef": pc, "sft_coef": sc, "token_sum": bool(int(getattr(self.args, "policy_token_sum", 0)))}
        if K > 0:
            pol.update(slate_size=K, slate_estimator=estimator)
        return pol

    def _pref_flags(self):
        """--train_preference pl | ipo: the keyword arguments of `P5T5Native.preference_step` (None with the flag absent), every flag checked
        here.  The reference policy (--pref_ref init) is a frozen copy of the weights the runner is built with: a --resume'd run is built
        with the same weights as the run it continues, so both train against the same reference."""
        kind = str(getattr(self.args, "train_preference", "") or "")
        if not kind:
            return None
        if kind not in ("pl", "ipo"):
            raise ValueError(f"--train_preference {kind}: pl or ipo")
        if not int(getattr(self.args, "train_item_loss", 0)):
            raise ValueError("--train_preference requires --train_item_loss 1 (the draws and the loss share the union item trie)")
        if not hasattr(self.model, "preference_step"):
            raise ValueError("--train_preference needs the native model (P5T5Native)")
        if int(getattr(self.args, "train_policy_samples", 0)) != 0:
            raise ValueError("--train_preference cannot be combined with --train_policy_samples: one objective per run")
        if int(getattr(self.args, "item_loss_top_k", 0)) != 0 or float(getattr(self.args, "item_loss_top_p", 1.0)) != 1.0:
            raise ValueError("--train_preference is not built for the truncated item loss (top_k / top_p): --item_loss_top_k / --item_loss_top_p")
        if float(getattr(self.args, "item_loss_entropy_coef", 0.0)) != 0.0 or float(getattr(self.args, "item_loss_kl_coef", 0.0)) != 0.0:
            raise ValueError("--train_preference is not built beside --item_loss_entropy_coef / --item_loss_kl_coef")
        S, depth = int(getattr(self.args, "pref_negatives", 4)), int(getattr(self.args, "pref_depth", 1))
        beta, sc = float(getattr(self.args, "pref_beta", 0.1)), float(getattr(self.args, "pref_sft_coef", 0.0))
        if S < 1:
            raise ValueError(f"--pref_negatives {S}: at least one sampled negative per user")
        if not (math.isfinite(beta) and beta > 0.0):
            raise ValueError(f"--pref_beta {beta}: a finite value > 0")
        if depth < 0:
            raise ValueError(f"--pref_depth {depth}: the Plackett-Luce depth (0 = the full order)")
        if not math.isfinite(sc):
            raise ValueError(f"--pref_sft_coef {sc}: a finite value")
        ref, mode = str(getattr(self.args, "pref_ref", "init")), str(getattr(self.args, "pref_negatives_mode", "slate"))
        if ref not in ("init", "none"):
            raise ValueError(f"--pref_ref {ref}: init or none")
        if mode not in ("slate", "sample"):
            raise ValueError(f"--pref_negatives_mode {mode}: slate or sample")
        return {"num_negatives": S, "preference": kind, "pref_depth": depth if depth > 0 else None, "pref_beta": beta, "pref_sft_coef": sc,
                "pref_length_normalize": bool(int(getattr(self.args, "pref_length_normalize", 0))),
                "ref_model": self.model.frozen_copy() if ref == "init" else None, "negatives": mode}

    def _item_loss_kw(self):
        """--train_item_loss 1: the keyword arguments of the trie-normalised item loss -- ONE union trie over the items of all training
        datasets (item ids carry their dataset's name, so the union is a tree), built once; None with the flag at 0."""
        if not int(getattr(self.args, "train_item_loss", 0)):
            if float(getattr(self.args, "item_loss_entropy_coef", 0.0)) != 0.0 or float(getattr(self.args, "item_loss_kl_coef", 0.0)) != 0.0:
                raise ValueError("--item_loss_entropy_coef / --item_loss_kl_coef require --train_item_loss 1")
            return None
        kw = self.__dict__.get("_item_loss")
        if kw is None:
            # (every flag is checked before anything is built, and the dict is cached only when it is complete: a caller that catches an
            #  error never meets a half-built setting on its next call)
            top_k, top_p = int(getattr(self.args, "item_loss_top_k", 0)), float(getattr(self.args, "item_loss_top_p", 1.0))
            ec, kc = float(getattr(self.args, "item_loss_entropy_coef", 0.0)), float(getattr(self.args, "item_loss_kl_coef", 0.0))
            if ec != 0.0 or kc != 0.0:
                if top_k != 0 or top_p != 1.0:
                    raise ValueError("--item_loss_entropy_coef / --item_loss_kl_coef are not built for --item_loss_top_k / --item_loss_top_p")
                if kc != 0.0 and str(getattr(self.args, "item_loss_kl_ref", "")) != "init":
                    raise ValueError("--item_loss_kl_coef needs a reference policy: --item_loss_kl_ref init")
                if not (hasattr(self.model, "loss_and_backward") and hasattr(self.model, "frozen_copy")):
                    raise ValueError("--item_loss_entropy_coef / --item_loss_kl_coef need the native model (P5T5Native)")
            loader = self.train_loader if self.train_loader is not None else self.valid_loader
            seqs, seen = [], set()
            for ds in loader.dataset.datasets:
                if ds.dataset not in seen:
                    seen.add(ds.dataset)
                    seqs += self._item_sequences(ds, list(ds.all_items))
            kw = {"trie": CompiledTrie.from_trie(Trie(seqs)), "temperature": float(getattr(self.args, "item_loss_temperature", 1.0))}
            if top_k != 0 or top_p != 1.0:          # (off: the keyword arguments of the untruncated loss, as before)
                kw.update(top_k=top_k, top_p=top_p)
            if str(getattr(self.args, "item_loss_head", "dense")) == "trie":      # (dense: the keyword arguments of the run without the flag)
                kw["item_head"] = "trie"
            if ec != 0.0 or kc != 0.0:           # (both 0: the keyword arguments of the run without the flags)
                kw.update(entropy_coef=ec, kl_coef=kc)
                if kc != 0.0:
                    # the frozen reference: this model's weights as they are NOW (the first call precedes the first step)
                    kw["ref_model"] = self.model.frozen_copy()
            self._item_loss = kw
        return kw

    TRAIN_ONLY_ITEM_LOSS_KEYS = ("entropy_coef", "kl_coef", "ref_model")      # of training_step; `forward` (validation) does not take them

    @torch.no_grad()
    def validate(self):
        self.model.eval()
        if self.args.valid_prompt_sample > 0:
            for ds in self.valid_loader.dataset.datasets:
                ds.construct_sentence()
        losses = []
        for batch in self.valid_loader:
            input_ids, attn, whole_ids, output_ids, output_attention = self._to_dev(batch)[:5]
            out = self.model(input_ids=input_ids, whole_word_ids=whole_ids, attention_mask=attn, labels=output_ids,
                             alpha=self.args.alpha, return_dict=True,
                             **{k: v for k, v in (self._item_loss_kw() or {}).items() if k not in self.TRAIN_ONLY_ITEM_LOSS_KEYS})
            losses.append(masked_mean_loss(out["loss"], output_attention))
        v = torch.stack(losses).mean()
        if self.world > 1:
            dist.all_reduce(v, op=dist.ReduceOp.SUM)
            v /= self.world
        return float(v)

    # ------------------------------------------------------------------ evaluation
    def test(self, path=None):
        self.model.eval()
        if path:
            self.model.load_state_dict(torch.load(path, map_location="cpu"), strict=False)
        results = []
        if self.test_candidates > 0 and self.test_filtered > 0 and self.rank == 0 and not self.__dict__.get("_cand_said"):
            self._cand_said = True
            logging.info(f"--test_candidates {self.test_candidates} takes precedence over --test_filtered {self.test_filtered}: "
                         "the sampled negatives never contain the user's history")
        for loader in self.testloaders:
            if self.test_candidates > 0:
                results.append(self.test_dataset_task_candidates(loader))
            elif self.test_filtered > 0:
                if self.test_filtered_batch > 0:
                    results.append(self.test_dataset_task_filtered_batch(loader))
                else:
                    results.append(self.test_dataset_task_filtered(loader))
            else:
                results.append(self.test_dataset_task(loader))
        return results

    def _item_sequences(self, ds, candidates):
        """[decoder start] + token ids of "<dataset> item_<id>" per candidate (DistributedRunner.py:344-350); tokenised once per
        item and cached -- the per-user filtered protocol (:286-297) would otherwise re-tokenise every item for every user."""
        cache = self.__dict__.setdefault("_item_tok_cache", {})
        out = []
        for c in candidates:
            key = (ds.dataset, c)
            seq = cache.get(key)
            if seq is None:
                seq = [0] + self.tokenizer.encode(f"{ds.dataset} item_{c}")
                cache[key] = seq
            out.append(seq)
        return out

    def _generate(self, batch, fn, num_beams, max_length):
        input_ids, attn, whole_ids, output_ids = batch[0], batch[1], batch[2], batch[3]
        pred = self.model.generate(input_ids=input_ids, attention_mask=attn, whole_word_ids=whole_ids, max_length=max_length,
                                   prefix_allowed_tokens_fn=fn, num_beams=num_beams, num_return_sequences=num_beams,
                                   output_scores=True, return_dict_in_generate=True)
        gold = self.tokenizer.batch_decode(output_ids, skip_special_tokens=True)
        gen = self.tokenizer.batch_decode(pred["sequences"], skip_special_tokens=True)
        return gold, gen, pred["sequences_scores"].detach().cpu().tolist()

    def _generate_ids(self, batch, num_beams, max_length, **kw):
        """ID-level evaluation of one batch: bool relevance [B, K] on the device (no decode to strings)."""
        pred = self.model.generate(input_ids=batch[0], attention_mask=batch[1], whole_word_ids=batch[2], max_length=max_length,
                                   num_beams=num_beams, num_return_sequences=num_beams, output_scores=True,
                                   return_dict_in_generate=True, **kw)
        return evaluate.rel_results_ids(pred["sequences"], pred["sequences_scores"], batch[3].to(pred["sequences"].device), num_beams)

    def _rank_metrics(self, batch, ct, excluded_items=None):
        """--test_exhaustive 1: the batch's metric sums from an exact ranking of the whole catalogue (top generate_num, the items of
        `excluded_items` left out), in either metric form."""
        pred = self.model.rank_items(input_ids=batch[0], attention_mask=batch[1], whole_word_ids=batch[2], trie=ct, top_n=self.generate_num,
                                     excluded_items=excluded_items, **({"pruned": True} if self.test_exhaustive == 2 else {"pruned": "search"} if self.test_exhaustive == 3 else {}))
        if self.id_metrics:
            rel = evaluate.rel_results_ids(pred["sequences"], pred["sequences_scores"], batch[3].to(pred["sequences"].device), self.generate_num)
            return evaluate.get_metrics_results_ids(rel, self.metrics), len(rel)
        gold = self.tokenizer.batch_decode(batch[3], skip_special_tokens=True)
        gen = self.tokenizer.batch_decode(pred["sequences"], skip_special_tokens=True)
        rel = evaluate.rel_results(gen, gold, pred["sequences_scores"].detach().cpu().tolist(), self.generate_num)
        return evaluate.get_metrics_results(rel, self.metrics), len(rel)

    def _lanes_map(self, fn, batches):
        """fn(batch) for every batch in order, several batches in flight when the model offers generation lanes (P5T5Native.map_lanes)."""
        ml = getattr(self.model, "map_lanes", None)
        if ml is None or self.gen_lanes <= 1:
            return (fn(b) for b in batches)
        return ml(fn, batches, lanes=self.gen_lanes)

    def _dataset_trie(self, ds):
        """Item trie of a dataset, compiled once, with the item -> path index used for per-user exclusion."""
        cache = self.__dict__.setdefault("_trie_cache", {})
        ent = cache.get(ds.dataset)
        if ent is None:
            items = list(ds.all_items)
            seqs = self._item_sequences(ds, items)
            trie = Trie(seqs)
            ct = CompiledTrie.from_trie(trie)
            ct.index_items(seqs)
            ent = cache[ds.dataset] = (trie, ct, {it: i for i, it in enumerate(items)})
        return ent

    def _finish(self, metrics_res, test_total, testloader, t0):
        metrics_res = torch.as_tensor(metrics_res, dtype=torch.float64).to(self.device)
        total = torch.tensor(float(test_total), dtype=torch.float64, device=self.device)
        if self.world > 1:
            dist.all_reduce(metrics_res, op=dist.ReduceOp.SUM)
            dist.all_reduce(total, op=dist.ReduceOp.SUM)
        dt = time.perf_counter() - t0
        self.items_per_sec = float(total) * self.generate_num / max(dt, 1e-9)
        metrics_res = (metrics_res / total).cpu().numpy()
        if self.rank == 0:
            for name, val in zip(self.metrics, metrics_res):
                logging.info(f"{name}: {val}")
            logging.info(f"{testloader.dataset.dataset}/{testloader.dataset.task}: {self.items_per_sec:.1f} items/s")
        return dict(zip(self.metrics, metrics_res.tolist()))

    @torch.no_grad()
    def test_dataset_task(self, testloader):
        """DistributedRunner.py:339-399 (max_length 50 there)."""
        ds = testloader.dataset
        trie, ct, _ = self._dataset_trie(ds)
        fn = prefix_allowed_tokens_fn(trie)
        metrics_res, test_total, t0 = 0, 0, time.perf_counter()

        def one(batch):          # runs on a generation lane (its own stream): everything up to the batch's metric sums
            batch = self._to_dev(batch)
            if self.test_exhaustive:
                return self._rank_metrics(batch, ct)
            if self.id_metrics:
                rel = self._generate_ids(batch, self.generate_num, 50, trie=ct)
                return evaluate.get_metrics_results_ids(rel, self.metrics), len(rel)
            gold, gen, scores = self._generate(batch, fn, self.generate_num, 50)
            rel = evaluate.rel_results(gen, gold, scores, self.generate_num)
            return evaluate.get_metrics_results(rel, self.metrics), len(rel)

        # (collation overlaps the previous generate(); up to --gen_lanes batches are in flight on the device, results come back in order)
        for m, n in self._lanes_map(one, Prefetcher(testloader, pin=self.device.type == "cuda")):
            if torch.is_tensor(m) and m.is_cuda:
                m.record_stream(torch.cuda.current_stream())      # (allocated on the lane's stream, read here)
            metrics_res = metrics_res + (m.to(self.device) if torch.is_tensor(m) else m)
            test_total += n
        return self._finish(metrics_res, test_total, testloader, t0)

    def candidate_lists(self, ds, user_idx):
        """--test_candidates N: per user of the batch the item ids [gold, N sampled negatives] (evaluate.sample_candidates: the same
        list on every rank, every run and at every batch size)."""
        out = []
        for u in user_idx:
            user = ds.id2user[int(u)]
            out.append(evaluate.sample_candidates(ds.all_items, ds.positive[user], ds.reindex_user_seq_dict[user][-1], self.test_candidates,
                                                  self.args.seed, ds.dataset, user))
        return out

    @torch.no_grad()
    def test_dataset_task_candidates(self, testloader):
        """The sampled-candidates protocol ("1 + N"): the gold item among N negatives from outside the user's history, every list scored
        exactly in one pass over its own prefixes (P5T5Native.score_candidates), metrics over the top min(generate_num, N + 1)."""
        ds = testloader.dataset
        _, ct, index = self._dataset_trie(ds)
        width = self.test_candidates + 1
        top_n = min(self.generate_num, width)
        metrics_res, test_total, t0 = 0, 0, time.perf_counter()

        def one(batch):
            batch = self._to_dev(batch)
            lists = self.candidate_lists(ds, batch[5].detach().cpu().tolist())
            cand = torch.full((len(lists), width), -1, dtype=torch.int64)
            for b, items in enumerate(lists):
                cand[b, :len(items)] = torch.tensor([index[i] for i in items], dtype=torch.int64)
            pred = self.model.score_candidates(input_ids=batch[0], attention_mask=batch[1], whole_word_ids=batch[2], trie=ct, candidates=cand,
                                               top_n=top_n)
            if self.id_metrics:
                rel = evaluate.rel_results_ids(pred["sequences"], pred["sequences_scores"], batch[3].to(pred["sequences"].device), top_n)
                return evaluate.get_metrics_results_ids(rel, self.metrics), len(rel)
            gold = self.tokenizer.batch_decode(batch[3], skip_special_tokens=True)
            gen = self.tokenizer.batch_decode(pred["sequences"], skip_special_tokens=True)
            rel = evaluate.rel_results(gen, gold, pred["sequences_scores"].detach().cpu().tolist(), top_n)
            return evaluate.get_metrics_results(rel, self.metrics), len(rel)

        for m, n in self._lanes_map(one, Prefetcher(testloader, pin=self.device.type == "cuda")):
            if torch.is_tensor(m) and m.is_cuda:
                m.record_stream(torch.cuda.current_stream())      # (allocated on the lane's stream, read here)
            metrics_res = metrics_res + (m.to(self.device) if torch.is_tensor(m) else m)
            test_total += n
        return self._finish(metrics_res, test_total, testloader, t0)

    @torch.no_grad()
    def test_dataset_task_filtered(self, testloader):
        """DistributedRunner.py:271-337: one trie per user = all items minus the user's history."""
        ds = testloader.dataset
        _, ct, index = self._dataset_trie(ds)
        metrics_res, test_total, t0 = 0, 0, time.perf_counter()

        def one(batch):
            batch = self._to_dev(batch)
            # the reference rebuilds Trie(all_items - positive) per user (hence its eval_batch_size == 1); here the shared
            # device trie is used with one excluded-node bitmap per user, so any batch size works
            users = [ds.id2user[int(u)] for u in batch[5].detach().cpu().tolist()]
            history = [[index[i] for i in ds.positive[u] if i in index] for u in users]
            if self.test_exhaustive:
                return self._rank_metrics(batch, ct, excluded_items=history)
            excluded = ct.excluded_bitmap(history)
            if self.id_metrics:
                rel = self._generate_ids(batch, self.generate_num, 30, trie=ct, excluded=excluded)
                return evaluate.get_metrics_results_ids(rel, self.metrics), len(rel)
            else:
                input_ids, attn, whole_ids, output_ids = batch[0], batch[1], batch[2], batch[3]
                pred = self.model.generate(input_ids=input_ids, attention_mask=attn, whole_word_ids=whole_ids, max_length=30, trie=ct,
                                           excluded=excluded, num_beams=self.generate_num, num_return_sequences=self.generate_num,
                                           output_scores=True, return_dict_in_generate=True)
                gold = self.tokenizer.batch_decode(output_ids, skip_special_tokens=True)
                gen = self.tokenizer.batch_decode(pred["sequences"], skip_special_tokens=True)
                rel = evaluate.rel_results(gen, gold, pred["sequences_scores"].detach().cpu().tolist(), self.generate_num)
                return evaluate.get_metrics_results(rel, self.metrics), len(rel)

        for m, n in self._lanes_map(one, Prefetcher(testloader, pin=self.device.type == "cuda")):
            if torch.is_tensor(m) and m.is_cuda:
                m.record_stream(torch.cuda.current_stream())      # (allocated on the lane's stream, read here)
            metrics_res = metrics_res + (m.to(self.device) if torch.is_tensor(m) else m)
            test_total += n
        return self._finish(metrics_res, test_total, testloader, t0)

    @torch.no_grad()
    def test_dataset_task_filtered_batch(self, testloader):
        """DistributedRunner.py:204-269: widen the beam by max_positive, filter the history afterwards."""
        ds = testloader.dataset
        trie, ct, index = self._dataset_trie(ds)
        fn = prefix_allowed_tokens_fn(trie)
        width = self.generate_num + ds.max_positive
        if self.test_exhaustive:
            # the widened beam ranks the catalogue and drops the history afterwards; an exact ranking without the history is its limit
            return self.test_dataset_task_filtered(testloader)
        if self.test_filtered_batch >= 2:
            # OPT-IN (--test_filtered_batch 2): exclude each user's history INSIDE the constrained search (shared device trie + per-user
            # excluded-node bitmap, batched) instead of widening the beam -- history never appears, the top generate_num are kept.  This is
            # the --test_filtered_batch 0 protocol's result, not the widened-beam protocol's: a beam of generate_num + max_history can
            # keep items an excluded search prunes, so the two may differ.
            return self.test_dataset_task_filtered(testloader)
        if width > MAX_DEVICE_BEAMS:
            # the literal protocol of the reference's DEFAULT flag (SingleRunner.py:39, DistributedRunner.py:235-236) needs
            # num_beams = generate_num + max history; never silently substitute another protocol for it
            raise ValueError(f"--test_filtered_batch 1 needs num_beams = {self.generate_num} + max history {ds.max_positive} = {width} > "
                             f"{MAX_DEVICE_BEAMS} (device beam limit).  Use --test_filtered_batch 2 (history excluded inside the search, batched: "
                             "the results of --test_filtered_batch 0) or --test_filtered_batch 0 (the released test protocol).")
        seq2idx = None
        if self.id_metrics:     # item token tuple (without the decoder start) -> item index: no batch_decode, no string sets
            seq2idx = self.__dict__.setdefault("_seq2idx_cache", {}).get(ds.dataset)
            if seq2idx is None:
                items = list(ds.all_items)
                seq2idx = {tuple(q[1:]): i for i, q in enumerate(self._item_sequences(ds, items))}
                self._seq2idx_cache[ds.dataset] = seq2idx
        metrics_res, test_total, t0 = 0, 0, time.perf_counter()
        for batch in Prefetcher(testloader, pin=self.device.type == "cuda"):      # collation overlaps the previous generate()
            batch = self._to_dev(batch)
            if self.id_metrics:
                pred = self.model.generate(input_ids=batch[0], attention_mask=batch[1], whole_word_ids=batch[2], max_length=30, trie=ct,
                                           num_beams=width, num_return_sequences=width, output_scores=True, return_dict_in_generate=True)
                B = batch[0].shape[0]
                seqs = pred["sequences"].detach().cpu().numpy().reshape(B, width, -1)
                sc = pred["sequences_scores"].detach().cpu().numpy().reshape(B, width)
                users = [ds.id2user[int(u)] for u in batch[5].detach().cpu().tolist()]
                pos = [{index[i] for i in ds.positive[u] if i in index} for u in users]
                rel = evaluate.rel_results_filtered_ids(seqs, sc, batch[3].detach().cpu().numpy(), pos, seq2idx, self.generate_num)
            else:
                gold, gen, scores = self._generate(batch, fn, width, 30)
                rel = evaluate.rel_results_filtered(ds.positive_text, ds.id2user, batch[5].detach().cpu().numpy(), width, gen, gold, scores,
                                                    self.generate_num)
            test_total += len(rel)
            metrics_res = metrics_res + evaluate.get_metrics_results(rel, self.metrics)
        return self._finish(metrics_res, test_total, testloader, t0)


SingleRunner = DistributedRunner
