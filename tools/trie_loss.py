"""Item-loss training step timing (csrc/p5_trie_ce.h): the C2 training step (T5-small, bf16, B = 64, L = 128, T = 8, dropout 0.1; labels are
items of the benchmark's 3,416-item trie) three ways in one process --
  plain          the default step: full-vocabulary cross-entropy on the logit-free head
  plain_ce_free0 the same loss with option "ce_free" 0: materialised fp32 logits, p5_ce_fwd_kernel / p5_ce_bwd_kernel
  item_loss      training_step(..., item_loss={"trie": ...}): materialised logits, p5_trie_walk / p5_trie_ce_fwd / p5_trie_ce_bwd
  item_loss_trie_head   (with --item_head trie or both) the same loss on the head restricted to the trie's tokens (csrc/p5_item_head.h): the
                 rows U of the head weight gathered, logits_U [B*T, Nup], one scatter of dE_U into shared.weight's gradient
With --entropy_coef / --kl_coef (csrc/p5_trie_reg.h) every selected item-loss step is followed by its regularised forms:
  <step>_entropy          the same step with the entropy term (entropy_coef, no reference)
  <step>_entropy_kl       with entropy + KL, the reference's logits of the batch prepared OUTSIDE the timed region (`ref_logits`, in the
                          column layout of the step's own head)
  <step>_entropy_kl_ref   the same with the frozen reference's `item_logits` call INSIDE the timed region ("ref_model": what the runner does)
the reference being a frozen copy of the model's initial weights (`P5T5Native.frozen_copy`).
alternated window by window, so that a drift of the machine lands on all three; one JSON line per variant: ms per step (median and spread
over the rounds), its ratio to the plain step of the same run, and the device ms of one step by kernel family (in-run profiler,
p5_profile_begin / end: each launch's time includes its dispatch gap).
Nothing is gated on the item-loss step.  The yardstick of the restricted head is the dense item-loss step of the same call
(`over_item_loss`, with that step's own spread in `step_ms_min_max`).
python tools/trie_loss.py [--batch 64] [--dtype bf16] [--rounds 7] [--min_seconds 0.5] [--temperature 1.0] [--item_head dense|trie|both] [--entropy_coef 0.01] [--kl_coef 0.1] [--tag NAME]
                          [--out profiles/trie_loss.jsonl]"""
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
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--min_seconds", type=float, default=0.5)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--item_head", default="both", choices=["dense", "trie", "both"], help="which item-loss steps run beside the plain ones")
ap.add_argument("--entropy_coef", type=float, default=0.0, help="non-zero (or --kl_coef): also time the regularised item-loss steps")
ap.add_argument("--kl_coef", type=float, default=0.0)
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
REG = ("_entropy", "_entropy_kl", "_entropy_kl_ref")
PARTS = (("loss", ("p5_trie_", "p5_ce_", "p5_masked_mean", "p5_item_")), ("attention", ("p5_attn",)), ("gemm", ("p5_gemm", "p5_g4", "p5_g5")),
         ("optimizer", ("p5_adamw", "p5_sumsq")), ("embedding", ("p5_embed",)))


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


def item_labels(items, B, T, seed):
    """labels [B, T] and their mask: B items of the catalogue behind the decoder start, pad-filled behind </s>"""
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(items), (B,), generator=g).tolist()
    labels = torch.zeros(B, T, dtype=torch.int64)
    out_attn = torch.zeros(B, T, dtype=torch.int64)
    for b, i in enumerate(pick):
        q = list(items[i][1:1 + T])
        labels[b, :len(q)] = torch.tensor(q)
        out_attn[b, :len(q)] = 1
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
    labels, out_attn = item_labels(items, B, T, 501)
    batch = (ids, ww, mask, labels.to(be.device), out_attn.to(be.device))
    kw = {"trie": ct, "temperature": a.temperature}

    def variant(ce_free, item_loss):
        def step():
            lib.p5_set_option(b"ce_free", ce_free)
            try:
                return training_step(model, opt, batch, alpha=2, item_loss=item_loss)
            finally:
                lib.p5_set_option(b"ce_free", 1)
        return step
    steps = {"plain": variant(1, None), "plain_ce_free0": variant(0, None)}
    if a.item_head in ("dense", "both"):
        steps["item_loss"] = variant(1, {**kw, "item_head": "dense"})
    if a.item_head in ("trie", "both"):
        steps["item_loss_trie_head"] = variant(1, {**kw, "item_head": "trie"})
    if a.entropy_coef != 0.0 or a.kl_coef != 0.0:
        ref = model.frozen_copy()
        for name, head in (("item_loss", "dense"), ("item_loss_trie_head", "trie")):
            if name not in steps:
                continue
            hk = {**kw, "item_head": head}
            ref_logits = ref.item_logits(ids, ww, mask, batch[3], ct, temperature=a.temperature, item_head=head)      # the step's own head's columns
            steps[name + REG[0]] = variant(1, {**hk, "entropy_coef": a.entropy_coef})
            steps[name + REG[1]] = variant(1, {**hk, "entropy_coef": a.entropy_coef, "kl_coef": a.kl_coef, "ref_logits": ref_logits})
            steps[name + REG[2]] = variant(1, {**hk, "entropy_coef": a.entropy_coef, "kl_coef": a.kl_coef, "ref_model": ref})
    for _ in range(5):          # warm-up: workspaces, code objects, the trie on the device
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    loss = {k: float(fn()) for k, fn in steps.items()}
    off = int((model.last_item_loss_state == 2).sum())
    assert off == 0, f"{off} label rows off the trie"
    t = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            t[k].append(window(fn, a.min_seconds) * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = []
    for k, fn in steps.items():
        base = next((k[:-len(sfx)] for sfx in sorted(REG, key=len, reverse=True) if k.endswith(sfx)), k)        # the un-regularised step of the same head
        line = {"tag": a.tag, "what": "trie_loss", "variant": k, "dtype": a.dtype, "backbone": "t5-small", "B": B, "L": L, "T": T, "dropout": 0.1,
                "n_items": 3416, "temperature": a.temperature if k.startswith("item_loss") else None,
                "item_head": {"item_loss": "dense", "item_loss_trie_head": "trie"}.get(base), "head_columns": len(ct.head_columns()[0]) if base == "item_loss_trie_head" else None,
                "entropy_coef": a.entropy_coef if base != k else None, "kl_coef": a.kl_coef if k.endswith(REG[1:]) else None,
                "over_unregularised": round(med[k] / med[base], 4) if base != k else None,
                "added_ms_min_max": [round(min(x - y for x, y in zip(t[k], t[base])), 4), round(max(x - y for x, y in zip(t[k], t[base])), 4)] if base != k else None, "rounds": a.rounds, "loss": round(loss[k], 5),
                "step_ms": round(med[k], 4), "step_ms_min_max": [round(min(t[k]), 4), round(max(t[k]), 4)],
                "over_plain": round(med[k] / med["plain"], 4), "over_item_loss": round(med[k] / med["item_loss"], 4) if "item_loss" in med else None, "step_ms_by_family": profile_split(lib, lambda: (fn(), torch.cuda.synchronize()))}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
