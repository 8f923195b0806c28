"""Clipped-ratio policy objective, timing: at the benchmark shape (bf16 T5-small, B = 64, L = 128, dropout 0.1, the 3,416-item trie) with S in
--samples (default 4, 8, 16) draws per user, alternated window by window in one process so that a drift of the machine lands on all of them:
  (a) plain    the grouped loss_and_backward(target_weights=...) on a FIXED rollout (one policy_collect in front of the timing) + optimizer step:
               the code of the step without the objective;
  (b) clip     policy_update on the same rollout (the two kernels of csrc/p5_clip.h in the loss kernel's place, the seeds through the
               backward's per-row route) + optimizer step;
  (k) kernels  the two clip kernels alone (p5_op_clip_objective) on arrays of the rollout's shape;
  (c) for E in --epochs (default 1, 2, 4): one policy_collect + E x (policy_update + optimizer step) against E fresh policy_step + optimizer
      step -- both per E optimizer steps.
The model is trained by the steps that are timed and the rollout stays what it was, so the ratios drift and late windows clip most units (the
recorded `clip_stats` show it); the launches do not depend on the values.  One JSON line per S: ms of each (median and spread over the rounds),
(b) - (a) beside (a)'s own spread and (k).  No figure is gated.
python tools/policy_clip.py [--batch 64] [--samples 4,8,16] [--epochs 1,2,4] [--rounds 5] [--min_seconds 0.3] [--out profiles/policy_clip.jsonl]"""
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
ap.add_argument("--epochs", default="1,2,4")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--min_seconds", type=float, default=0.3)
ap.add_argument("--item_head", default="dense", choices=["dense", "trie"])
ap.add_argument("--baseline", default="loo")
ap.add_argument("--clip_eps", type=float, default=0.2)
ap.add_argument("--ratio", default="token", choices=["token", "sequence"])
ap.add_argument("--tag", default="this")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args() if __name__ == "__main__" else None
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from openp5_amd._lib import hip_backend  # noqa: E402
from openp5_amd.model import _ptr  # noqa: E402
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
    epochs = [int(e) for e in a.epochs.split(",")]
    lines = []
    for S in [int(s) for s in a.samples.split(",")]:
        seed = [0]

        def finish():
            opt.step()
            model.zero_grad()

        def reward(drawn):
            # a reward with signal whatever was drawn (the untrained model hits no gold item: the hit reward would give every draw weight 0 and
            # the objective no unit to work on)
            return (drawn["item_index"] * 7 % 5).to(torch.float32) - 1.5

        def collect():
            seed[0] += 1
            return model.policy_collect(ids, ww, mask, labels, out_attn, ct, S, baseline=a.baseline, seed=seed[0], item_head=a.item_head,
                                        clip_eps=a.clip_eps, ratio=a.ratio, reward_fn=reward)

        ro = collect()
        Bq, G, To = ro["labels"].shape

        def plain():
            model.loss_and_backward(ids, ww, mask, ro["labels"], ro["output_attention"], target_weights=ro["target_weights"], **kw)
            finish()

        def clip():
            model.policy_update(ids, ww, mask, ro, ct, a.clip_eps, ratio=a.ratio, item_head=a.item_head)
            finish()

        rows = Bq * G * To
        f = torch.zeros(2 * rows + 16 * Bq + 16, dtype=torch.float32, device=be.device)
        nll = (-ro["old_logprobs"]).contiguous()
        ratio_code = model.CLIP_RATIOS[a.ratio]

        def kernels():
            be.check(be.lib.p5_op_clip_objective(_ptr(f[2 * rows + 16 * Bq:]), None, _ptr(f), _ptr(f[2 * rows:]), _ptr(f[2 * rows + 16 * Bq + 8:]), _ptr(nll),
                                                 _ptr(ro["old_logprobs"]), _ptr(ro["output_attention"]), _ptr(ro["labels"]), _ptr(ro["target_weights"]),
                                                 _ptr(ro["target_mode"]), None, None, 0.0, 0.0, a.clip_eps, a.clip_eps, ratio_code, Bq, G, To,
                                                 be.stream_ptr()), "p5_op_clip_objective")

        def updates(E):
            def fn():
                r = collect()
                for _ in range(E):
                    model.policy_update(ids, ww, mask, r, ct, a.clip_eps, ratio=a.ratio, item_head=a.item_head)
                    finish()
            return fn

        def fresh(E):
            def fn():
                for _ in range(E):
                    seed[0] += 1
                    model.policy_step(ids, ww, mask, labels, out_attn, ct, S, baseline=a.baseline, seed=seed[0], item_head=a.item_head, reward_fn=reward)
                    finish()
            return fn

        steps = {"plain": plain, "clip": clip, "kernels": kernels}
        for E in epochs:
            steps[f"collect_update_E{E}"] = updates(E)
            steps[f"fresh_steps_E{E}"] = fresh(E)
        for _ in range(2):
            for fn in steps.values():
                fn()
        t = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, fn in steps.items():
                t[k].append(window(fn, a.min_seconds) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        clip()
        line = {"tag": a.tag, "what": "policy_clip", "dtype": a.dtype, "backbone": "t5-small", "B": B, "L": L, "S": S, "G": int(G), "To": int(To),
                "item_head": a.item_head, "baseline": a.baseline, "clip_eps": a.clip_eps, "ratio": a.ratio, "dropout": 0.1, "n_items": 3416,
                "rounds": a.rounds}
        for k in steps:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        line["clip_minus_plain_ms"] = round(med["clip"] - med["plain"], 4)
        line["plain_spread_ms"] = round(max(t["plain"]) - min(t["plain"]), 4)
        for E in epochs:
            line[f"updates_over_fresh_E{E}"] = round(med[f"collect_update_E{E}"] / med[f"fresh_steps_E{E}"], 4)
        line["clip_stats"] = [round(float(x), 5) for x in model.last_clip_stats.tolist()]
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as fo:
            for line in lines:
                fo.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
