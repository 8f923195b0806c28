"""Several targets per user, step timing: the training step on `labels [B, G, T]` (one encoder pass per user, p5_forward_loss_targets) against
the replicated-batch step of the same content (user b's inputs repeated G times, `labels [B*G, T]`: the existing step), alternated window by
window in one process so that a drift of the machine lands on both.  bf16 T5-small, B = 64, L = 128, T = 8, dropout 0.1, G in --groups
(default 2, 8, 16); three losses: the plain cross-entropy, and the item loss on the benchmark's 3,416-item trie with `item_head` "dense" and
"trie".  One JSON line per (loss, G): ms per step of both steps (median and spread over the rounds), their ratio, the ms per target
sequence, and the device ms of one step of each by kernel family (in-run profiler, p5_profile_begin / end: each launch's time includes its
dispatch gap).  No ratio is gated.  `--only replicated` times the replicated step alone: that is existing code, so the tool can run against
another build of the library (--root: a checkout of it) to put the yardstick on record there as well.
python tools/multi_target.py [--batch 64] [--groups 2,8,16] [--losses plain,item_dense,item_trie] [--rounds 5] [--min_seconds 0.3]
                             [--only both|grouped|replicated] [--tag NAME] [--out profiles/multi_target.jsonl]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--groups", default="2,8,16")
ap.add_argument("--losses", default="plain,item_dense,item_trie")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--min_seconds", type=float, default=0.3)
ap.add_argument("--only", default="both", choices=["both", "grouped", "replicated"])
ap.add_argument("--tag", default="this")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ARGS = ap.parse_args() if __name__ == "__main__" else None
if ARGS is not None:
    sys.path.insert(0, os.path.abspath(ARGS.root))
import torch  # noqa: E402

import bench  # noqa: E402
from openp5_amd._lib import hip_backend  # noqa: E402
from openp5_amd.runner import training_step  # noqa: E402
from openp5_amd.trie import CompiledTrie  # noqa: E402

# family <- kernel name prefixes
PARTS = (("loss", ("p5_trie_", "p5_ce_", "p5_masked_mean", "p5_item_", "p5_trunc_")), ("attention", ("p5_attn",)), ("gemm", ("p5_gemm", "p5_g4", "p5_g5")),
         ("optimizer", ("p5_adamw", "p5_sumsq")), ("embedding", ("p5_embed",)))
LOSSES = {"plain": None, "item_dense": "dense", "item_trie": "trie"}


def profile_split(lib, run):
    lib.p5_profile_begin()
    run()
    buf = ctypes.create_string_buffer(1 << 22)
    lib.p5_profile_end(buf, len(buf))
    out = {name: 0.0 for name, _ in PARTS}
    out["other"] = 0.0
    for r in json.loads(buf.value.decode() or "[]"):
        kname = re.match(r"\(*(\w+)", r["kernel"]).group(1)
        for name, keys in PARTS:
            if any(kname.startswith(k) for k in keys):
                out[name] += r["total_us"] / 1e3
                break
        else:
            out["other"] += r["total_us"] / 1e3
    return {k: round(v, 3) for k, v in out.items()}


def window(fn, min_seconds):
    """seconds per call over one timed window that ends in a device synchronise"""
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < min_seconds:
        fn()
        reps += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def item_labels(items, B, G, T, seed):
    """labels [B, G, T] and their mask: G items of the catalogue per user behind the decoder start, pad-filled behind </s>"""
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(items), (B, G), generator=g).tolist()
    labels = torch.zeros(B, G, T, dtype=torch.int64)
    out_attn = torch.zeros(B, G, T, dtype=torch.int64)
    for b in range(B):
        for k in range(G):
            q = list(items[pick[b][k]][1:1 + T])
            labels[b, k, :len(q)] = torch.tensor(q)
            out_attn[b, k, :len(q)] = 1
    return labels, out_attn


def main(a):
    be = hip_backend()
    lib = be.lib
    B, L, T = a.batch, 128, 8
    items = bench.synth_items(3416, 7)
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    _, model, opt = bench.build_model("t5-small", a.dtype, be.device, be, 1, 0, total_steps=100000)
    model.train()
    ids, ww, mask, _, _ = bench.synth_batch(B, L, T, be.device, 500)
    lines = []
    for G in [int(g) for g in a.groups.split(",")]:
        labels, out_attn = (t.to(be.device) for t in item_labels(items, B, G, T, 501 + G))
        r = lambda t: t.repeat_interleave(G, dim=0)      # noqa: E731
        grouped = (ids, ww, mask, labels, out_attn)
        replicated = (r(ids), r(ww), r(mask), labels.view(B * G, T), out_attn.view(B * G, T))
        for name in a.losses.split(","):
            head = LOSSES[name]
            kw = None if head is None else {"trie": ct, "temperature": 1.0, "item_head": head}
            steps = {}
            if a.only in ("both", "grouped"):
                steps["grouped"] = lambda: training_step(model, opt, grouped, alpha=2, item_loss=kw)
            if a.only in ("both", "replicated"):
                steps["replicated"] = lambda: training_step(model, opt, replicated, alpha=2, item_loss=kw)
            for _ in range(3):          # warm-up: workspaces, code objects, the trie on the device
                for fn in steps.values():
                    fn()
            torch.cuda.synchronize()
            loss = {k: float(fn()) for k, fn in steps.items()}
            t = {k: [] for k in steps}
            for _ in range(a.rounds):
                for k, fn in steps.items():
                    t[k].append(window(fn, a.min_seconds) * 1e3)
            med = {k: statistics.median(v) for k, v in t.items()}
            line = {"tag": a.tag, "what": "multi_target", "loss": name, "item_head": head, "dtype": a.dtype, "backbone": "t5-small", "B": B, "L": L, "T": T,
                    "G": G, "dropout": 0.1, "n_items": 3416, "rounds": a.rounds}
            for k, fn in steps.items():
                line[k + "_ms"] = round(med[k], 4)
                line[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
                line[k + "_us_per_target"] = round(med[k] * 1e3 / (B * G), 3)
                line[k + "_loss"] = round(loss[k], 5)
                line[k + "_ms_by_family"] = profile_split(lib, lambda: (fn(), torch.cuda.synchronize()))
            if len(steps) == 2:
                line["replicated_over_grouped"] = round(med["replicated"] / med["grouped"], 4)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
