"""Policy gradients from slates, cost and variance, at the benchmark shape (bf16 T5-small, B = 64, L = 128, dropout 0.1, the 3,416-item
trie), in the manner of tools/policy_step.py: steps alternated window by window in one process, five rounds.
  (a) time      ms per step of policy_step(slate_size=K, num_samples=S) next to policy_step(num_samples=S * K) of the same build, at the
                (S, K) of --shapes (default S * K = 4 / 8 / 16 training rows per user); both end in the optimizer step.  The expectation from
                the code is the same grouped step plus one more decode row per slate in the sampler.
  (b) variance  over --seeds R sampling seeds on a FIXED model (no optimizer step, dropout off) and batch: the plain `loo` step at S * K draws
                next to both slate estimators at equal training rows (token_sum, the hit reward, sft_coef 0).  Per method: the per-parameter
                variance of the gradient arena summed over the parameters, and the squared distance of its mean from the mean over all
                methods' seeds that are unbiased by construction (plain `loo` and slates `unbiased`).
One JSON line per shape and part.  No figure is gated.
python tools/policy_slates.py [--batch 64] [--shapes 2x2,2x4,4x4] [--rounds 5] [--min_seconds 0.3] [--seeds 64] [--out profiles/policy_slates.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--shapes", default="2x2,2x4,4x4", help="SxK: slates per user x items per slate")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--min_seconds", type=float, default=0.3)
ap.add_argument("--seeds", type=int, default=64)
ap.add_argument("--item_head", default="dense", choices=["dense", "trie"])
ap.add_argument("--tag", default="this")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args() if __name__ == "__main__" else None
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from openp5_amd._lib import hip_backend  # noqa: E402
from openp5_amd.trie import CompiledTrie  # noqa: E402
from tools.policy_step import window  # noqa: E402


def main(a):
    be = hip_backend()
    B, L, T = a.batch, 128, 8
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    items = bench.synth_items(3416, 7)
    _, model, opt = bench.build_model("t5-small", a.dtype, be.device, be, 1, 0, total_steps=100000)
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
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    lines = []
    base = {"tag": a.tag, "dtype": a.dtype, "backbone": "t5-small", "B": B, "L": L, "item_head": a.item_head, "n_items": 3416}

    # (b) first: the model is still the one it was built as
    model.eval()
    w0 = model._flat.detach().clone()
    for S, K in shapes:
        kw = dict(policy_coef=1.0, sft_coef=0.0, token_sum=True, item_head=a.item_head)
        methods = {"plain_loo": lambda s: model.policy_step(ids, ww, mask, labels, out_attn, ct, S * K, baseline="loo", seed=s, **kw),
                   "slates_unbiased": lambda s: model.policy_step(ids, ww, mask, labels, out_attn, ct, S, seed=s, slate_size=K, slate_estimator="unbiased", **kw)}
        if K >= 2:
            methods["slates_normalized"] = lambda s: model.policy_step(ids, ww, mask, labels, out_attn, ct, S, seed=s, slate_size=K,
                                                                       slate_estimator="normalized", **kw)
        mean, m2 = {}, {}
        for name, fn in methods.items():
            mu = torch.zeros_like(model._grads, dtype=torch.float64)
            sq = torch.zeros_like(mu)
            for s in range(a.seeds):
                model.zero_grad()
                fn(1000 + s)
                gr = model._grads.detach().double()
                mu += gr
                sq += gr * gr
            mean[name], m2[name] = mu / a.seeds, sq / a.seeds
        assert torch.equal(model._flat.detach(), w0)
        centre = (mean["plain_loo"] + mean["slates_unbiased"]) / 2
        line = dict(base, what="policy_slates_variance", S=S, K=K, rows=S * K, seeds=a.seeds, dropout=0.0)
        for name in methods:
            var = (m2[name] - mean[name] ** 2).clamp(min=0) * a.seeds / max(a.seeds - 1, 1)
            line[name + "_var_sum"] = float(var.sum())
            line[name + "_mean_dist2"] = float(((mean[name] - centre) ** 2).sum())
        line["centre_norm2"] = float((centre ** 2).sum())
        lines.append(line)
        print(json.dumps(line), flush=True)
    model.zero_grad()

    # (a) time
    model.train()
    for S, K in shapes:
        seed = [0]

        def finish():
            opt.step()
            model.zero_grad()

        def slates():
            seed[0] += 1
            model.policy_step(ids, ww, mask, labels, out_attn, ct, S, seed=seed[0], item_head=a.item_head, slate_size=K,
                              slate_estimator="normalized" if K >= 2 else "unbiased")
            finish()

        def plain():
            seed[0] += 1
            model.policy_step(ids, ww, mask, labels, out_attn, ct, S * K, baseline="loo", seed=seed[0], item_head=a.item_head)
            finish()

        steps = {"slates": slates, "plain": plain}
        for _ in range(3):
            for fn in steps.values():
                fn()
        t = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, fn in steps.items():
                t[k].append(window(fn, a.min_seconds) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        line = dict(base, what="policy_slates_time", S=S, K=K, rows=S * K, G=S * K + 1, dropout=0.1, rounds=a.rounds)
        for k in steps:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        line["slates_over_plain"] = round(med["slates"] / med["plain"], 4)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
