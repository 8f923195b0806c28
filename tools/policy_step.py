"""On-policy fine-tuning step, timing: at the benchmark shape (bf16 T5-small, B = 64, L = 128, dropout 0.1, the 3,416-item trie) with S in
--samples (default 4, 8, 16) draws per user, three steps alternated window by window in one process so that a drift of the machine lands on
all of them:
  (a) fused   model.policy_step: sample_items, the batch built on the device by p5_policy_batch (two launches), the grouped fused step;
  (b) torch   the same parts with the glue in torch: sample_items, `torch_policy_batch` (lengths, labels, masks, hits, leave-one-out
              advantages, weights -- a restatement of csrc/p5_policy.h in torch ops), loss_and_backward;
  (c) loss    the grouped loss_and_backward alone on prebuilt tensors;
and (s) sample_items alone.  (a), (b) and (c) end in the optimizer step, (s) does not: (a) - (c) - (s) counts it once.  The model is trained
by the steps that are timed, so late windows run on a policy that has collapsed onto the gold items (the recorded `stats` show it); the
launches do not depend on the weights' values.  One JSON line per S: ms per step of each (median and spread over the
rounds), (a) / (b), and the glue's cost (a) - (c) - (s).  No figure is gated.
python tools/policy_step.py [--batch 64] [--samples 4,8,16] [--rounds 5] [--min_seconds 0.3] [--item_head dense] [--out profiles/policy_step.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--samples", default="4,8,16")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--min_seconds", type=float, default=0.3)
ap.add_argument("--item_head", default="dense", choices=["dense", "trie"])
ap.add_argument("--baseline", default="loo")
ap.add_argument("--tag", default="this")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args() if __name__ == "__main__" else None
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from openp5_amd._lib import hip_backend  # noqa: E402
from openp5_amd.trie import CompiledTrie  # noqa: E402


def window(fn, min_seconds):
    """seconds per call over one timed window that ends in a device synchronise"""
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < min_seconds:
        fn()
        reps += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def torch_policy_batch(seq, labels, out_attn, S, policy_coef=1.0, sft_coef=1.0, eos=1, pad=0):
    """what p5_policy_batch computes (hit reward, leave-one-out baseline, token mean, gold in slot 0), in torch ops without a host sync"""
    B, Tg = labels.shape
    d = seq.view(B, S, -1)[:, :, 1:]
    Ts1 = d.shape[2]
    To = max(Tg, Ts1)
    pos = torch.arange(Ts1, device=seq.device)
    is_eos = d == eos
    first = torch.where(is_eos.any(2), is_eos.long().argmax(2) + 1, (d != pad).long().cumprod(2).sum(2))       # tokens through </s>
    m = (pos[None, None, :] < first[:, :, None]).long()
    gold_m = ((out_attn != 0) & (labels != -100)).long()
    lab = torch.zeros(B, S + 1, To, dtype=torch.int64, device=seq.device)
    att = torch.zeros_like(lab)
    lab[:, 0, :Tg], att[:, 0, :Tg] = labels, gold_m
    lab[:, 1:, :Ts1], att[:, 1:, :Ts1] = d * m, m
    # hit: the draw's tokens equal the gold's attended tokens (a prefix here) and the lengths agree
    T = min(Tg, Ts1)
    same = ((lab[:, 1:, :T] * att[:, 1:, :T]) == (labels * gold_m)[:, None, :T]).all(2) & (first == gold_m.sum(1)[:, None]) & (first > 0)
    r = same.float()
    ex = (first > 0).float()
    se = ex.sum(1, keepdim=True)
    dlt = (r - r[:, :1]) * ex
    A = (dlt - (dlt.sum(1, keepdim=True) - dlt) / (se - 1).clamp(min=1)) * ex
    G = S + 1
    w = torch.cat([torch.full((B, 1), sft_coef * G, device=seq.device), policy_coef * A * (G / S)], 1)
    return lab, att, w


def main(a):
    be = hip_backend()
    B, L, T = a.batch, 128, 8
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    items = bench.synth_items(3416, 7)
    _, model, opt = bench.build_model("t5-small", a.dtype, be.device, be, 1, 0, total_steps=100000)
    model.train()
    ids, ww, mask, _, _ = bench.synth_batch(B, L, T, be.device, 500)
    g = torch.Generator().manual_seed(11)
    pick = torch.randint(0, len(items), (B,), generator=g).tolist()
    Tg = max(len(q) for q in items) - 1
    labels = torch.zeros(B, Tg, dtype=torch.int64)
    out_attn = torch.zeros(B, Tg, dtype=torch.int64)
    for b, i in enumerate(pick):
        q = list(items[i][1:])
        labels[b, :len(q)] = torch.tensor(q)
        out_attn[b, :len(q)] = 1
    labels, out_attn = labels.to(be.device), out_attn.to(be.device)
    kw = dict(trie=ct, temperature=1.0, item_head=a.item_head)
    lines = []
    for S in [int(s) for s in a.samples.split(",")]:
        seed = [0]

        def finish():
            opt.step()
            model.zero_grad()

        def sample():
            seed[0] += 1
            return model.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=seed[0])

        def fused():
            seed[0] += 1
            model.policy_step(ids, ww, mask, labels, out_attn, ct, S, baseline=a.baseline, seed=seed[0], item_head=a.item_head)
            finish()

        def torch_glue():
            lab, att, w = torch_policy_batch(sample()["sequences"], labels, out_attn, S)
            model.loss_and_backward(ids, ww, mask, lab, att, target_weights=w, **kw)
            finish()

        pre = torch_policy_batch(sample()["sequences"], labels, out_attn, S)

        def loss_only():
            model.loss_and_backward(ids, ww, mask, pre[0], pre[1], target_weights=pre[2], **kw)
            finish()

        # the two ways of building the batch agree on the same draws
        pb = model.policy_batch(sample()["sequences"], labels, out_attn, S, baseline="loo")
        seed[0] -= 1
        lab, att, w = torch_policy_batch(sample()["sequences"], labels, out_attn, S)
        assert torch.equal(pb["labels"], lab) and torch.equal(pb["output_attention"], att), "torch restatement differs from the kernel"
        assert float((pb["target_weights"] - w).abs().max()) <= 1e-5
        steps = {"fused": fused, "torch": torch_glue, "loss": loss_only, "sample": sample}
        for _ in range(3):
            for fn in steps.values():
                fn()
        t = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, fn in steps.items():
                t[k].append(window(fn, a.min_seconds) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        line = {"tag": a.tag, "what": "policy_step", "dtype": a.dtype, "backbone": "t5-small", "B": B, "L": L, "S": S, "G": S + 1,
                "To": int(pre[0].shape[2]), "item_head": a.item_head, "baseline": a.baseline, "dropout": 0.1, "n_items": 3416, "rounds": a.rounds}
        for k in steps:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        line["fused_over_torch"] = round(med["fused"] / med["torch"], 4)
        line["glue_ms_fused"] = round(med["fused"] - med["loss"] - med["sample"], 4)
        line["glue_ms_torch"] = round(med["torch"] - med["loss"] - med["sample"], 4)
        line["stats"] = [round(float(x), 5) for x in model.last_policy_stats.tolist()[:6]]
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
