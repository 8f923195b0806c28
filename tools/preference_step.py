"""Preference objectives, timing: at the benchmark shape (bf16 T5-small, B = 64, L = 128, dropout 0.1, the 3,416-item trie) with S in
--negatives (default 1, 4, 8, 16) sampled negatives per user, alternated window by window in one process so that a drift of the machine lands
on all of them.  On a FIXED grouped batch [B, S + 1, To] (one draw in front of the timing), each + optimizer step:
  (a) plain       loss_and_backward(target_weights=...): the grouped step without the objective;
  (b) fused       loss_and_backward(preference=...): the two kernels of csrc/p5_pref.h in the loss kernel's place, the seeds through the
                  backward's per-row route;
  (c) torch       the same objective written in torch on forward()'s autograd seam (masked sums, logsumexp, backward through _P5LossFn);
  (k) kernels     the two kernels alone (p5_op_pref_objective) on arrays of the batch's shape;
and the whole step, drawing included:
  (s) step        preference_step (sample_slates, policy_batch, the reference's sequence_logprobs, the fused objective);
  (t) torch_step  the same draws and reference, the objective in torch.
One JSON line per S: ms of each (median and spread over the rounds), (b) - (a) beside (a)'s own spread, (c) / (b), (t) / (s).  No figure is gated.
python tools/preference_step.py [--batch 64] [--negatives 1,4,8,16] [--rounds 5] [--min_seconds 0.3] [--out profiles/preference_step.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--negatives", default="1,4,8,16")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--min_seconds", type=float, default=0.3)
ap.add_argument("--item_head", default="dense", choices=["dense", "trie"])
ap.add_argument("--preference", default="pl", choices=["pl", "ipo"])
ap.add_argument("--depth", type=int, default=1)
ap.add_argument("--beta", type=float, default=0.1)
ap.add_argument("--mode", default="slate", choices=["slate", "sample"])
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


def torch_objective(nll, out_attn, ref_lp, pmask, kind, depth, beta):
    """the objective of csrc/p5_pref.h in torch ops on the device (no length normalisation, no SFT term): nll [B, G, T] with a graph"""
    m = (out_attn != 0).to(nll.dtype)
    cnt = m.sum(2)
    delta = -(nll * m).sum(2) - (ref_lp * m).sum(2)
    listed = (pmask != 0) & (cnt > 0)
    h = torch.where(listed, beta * delta, torch.full_like(delta, float("-inf")))
    nb = listed.sum(1)
    has = (nb >= 2) & listed[:, 0]
    if kind == "pl" and depth == 1:          # (slot 0 is the first listed target in a preference_step batch: softmax-DPO)
        l = torch.logsumexp(h, 1) - h[:, 0]
    elif kind == "ipo":
        v = (delta[:, :1] - delta[:, 1:]) - 1.0 / (2.0 * beta)
        lm = listed[:, 1:].to(nll.dtype)
        l = (v * v * lm).sum(1) / lm.sum(1).clamp(min=1)
    else:
        raise SystemExit("torch restatement: --preference pl --depth 1, or ipo")
    return torch.where(has, l, torch.zeros_like(l)).sum() / nll.shape[0]


def main(a):
    be = hip_backend()
    B, L, T = a.batch, 128, 8
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    items = bench.synth_items(3416, 7)
    _, model, opt = bench.build_model("t5-small", a.dtype, be.device, be, 1, 0, total_steps=100000)
    model.train()
    ref = model.frozen_copy()
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
    pk = dict(preference=a.preference, pref_depth=a.depth if a.preference == "pl" else None, pref_beta=a.beta)
    lines = []
    for S in [int(s) for s in a.negatives.split(",")]:
        seed = [0]

        def finish():
            opt.step()
            model.zero_grad()

        def step():
            seed[0] += 1
            model.preference_step(ids, ww, mask, labels, out_attn, num_negatives=S, ref_model=ref, negatives=a.mode, seed=seed[0], **pk, **kw)
            finish()

        step()
        pb = model.last_policy_batch
        Bq, G, To = pb["labels"].shape
        ref_lp = ref.sequence_logprobs(ids, ww, mask, pb["labels"], **kw)

        def plain():
            model.loss_and_backward(ids, ww, mask, pb["labels"], pb["output_attention"], target_weights=pb["target_weights"], **kw)
            finish()

        def fused():
            model.loss_and_backward(ids, ww, mask, pb["labels"], pb["output_attention"], ref_logprobs=ref_lp, pref_mask=pb["pref_mask"], **pk, **kw)
            finish()

        def torch_loss(batch, rlp, pmask):
            nll = model(input_ids=ids, whole_word_ids=ww, attention_mask=mask, labels=batch["labels"], **kw)["loss"].view(Bq, G, To)
            torch_objective(nll, batch["output_attention"], rlp, pmask, a.preference, a.depth, a.beta).backward()

        def torch_fixed():
            torch_loss(pb, ref_lp, pb["pref_mask"])
            finish()

        def torch_step():
            seed[0] += 1
            if a.mode == "slate":
                drawn = model.sample_slates(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, slate_size=S, num_slates=1, seed=seed[0])
            else:
                drawn = model.sample_items(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, num_samples=S, seed=seed[0])
            q = model.policy_batch(drawn["sequences"], labels, out_attn, S, baseline="none")
            pmask = torch.cat([torch.ones(Bq, 1, dtype=torch.int32, device=be.device), (q["rewards"] == 0).to(torch.int32)], 1)
            torch_loss(q, ref.sequence_logprobs(ids, ww, mask, q["labels"], **kw), pmask)
            finish()

        rows = Bq * G * To
        f = torch.zeros(rows + 16 * Bq + 16, dtype=torch.float32, device=be.device)
        nll0 = (-ref_lp).reshape(-1).contiguous()
        rl0 = ref_lp.reshape(-1).contiguous()

        def kernels():
            be.check(be.lib.p5_op_pref_objective(_ptr(f[rows + 16 * Bq:]), _ptr(f), _ptr(f[rows:]), _ptr(f[rows + 16 * Bq + 8:]), _ptr(nll0), _ptr(rl0),
                                                 _ptr(pb["output_attention"]), _ptr(pb["labels"]), _ptr(pb["pref_mask"]), model.PREF_KINDS[a.preference], a.beta,
                                                 a.depth if a.preference == "pl" else 0, 0, 0.0, Bq, G, To, be.stream_ptr()), "p5_op_pref_objective")

        steps = {"plain": plain, "fused": fused, "torch": torch_fixed, "kernels": kernels, "step": step, "torch_step": torch_step}
        for _ in range(2):
            for fn in steps.values():
                fn()
        t = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, fn in steps.items():
                t[k].append(window(fn, a.min_seconds) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        fused()
        line = {"tag": a.tag, "what": "preference_step", "dtype": a.dtype, "backbone": "t5-small", "B": B, "L": L, "S": S, "G": int(G), "To": int(To),
                "item_head": a.item_head, "preference": a.preference, "depth": a.depth, "beta": a.beta, "negatives": a.mode, "dropout": 0.1,
                "n_items": 3416, "rounds": a.rounds}
        for k in steps:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        line["fused_minus_plain_ms"] = round(med["fused"] - med["plain"], 4)
        line["plain_spread_ms"] = round(max(t["plain"]) - min(t["plain"]), 4)
        line["torch_over_fused"] = round(med["torch"] / med["fused"], 4)
        line["torch_step_over_step"] = round(med["torch_step"] / med["step"], 4)
        line["pref_stats"] = [round(float(x), 5) for x in model.last_pref_stats.tolist()]
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as fo:
            for line in lines:
                fo.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
