"""Certified pruned ranking timing (csrc/p5_prune.h): rank_items(pruned=True) next to generation_mode "verified" (the full fp32 pass) and
"draft" (the bf16 pass) on the SAME trained bf16 model and the SAME users, over the 3416-item synthetic trie of bench.py.

Pruning only happens on a model that puts real mass on the trie's tokens, so a fresh T5-small is first trained for `--steps` native steps
with the benchmarked training step on the learnable task of bench.trained_generation_leg (the first input token names a user cluster,
the target is drawn from the cluster's own Zipf popularity over items of the trie) -- synthetic data in the spirit of openp5_amd/synth.py
without the dataset pipeline -- and the weights are written to `--weights`, so that another process (another build, see --root) times
exactly the same model: the file is loaded when it exists.

Every `what` is warmed up once, then timed in windows of at least `--min_seconds` that ALTERNATE between the whats for `--rounds`
rounds; a line reports the median window.  `--root DIR` imports the package from another tree (a checkout of the parent commit built in
a second directory; it has no `pruned`, so give it `--what verified`): alternate the two builds in one session by alternating commands.
Appends one JSON line per (what, slack) to `--out`:
  ms per user, rows kept per user (largest), the certified / fallback / declined shares, slack, and with --check whether the pruned lists
  equal the verified lists of this build token for token.
python tools/rank_pruned.py [--steps 300] [--users 8] [--what pruned,verified,draft] [--slacks 0.12] [--fraction 1.0] [--rounds 3]
                            [--min_seconds 1.0] [--weights FILE] [--root DIR] [--tag NAME] [--check] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--users", type=int, default=8)
ap.add_argument("--L", type=int, default=128)
ap.add_argument("--top_n", type=int, default=10)
ap.add_argument("--what", default="pruned,verified,draft")
ap.add_argument("--slacks", default="0.12")
ap.add_argument("--fraction", type=float, default=1.0, help="rank_prune_max_fraction during the timing (1.0: never decline, so that the cost at every kept share is seen)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--min_seconds", type=float, default=1.0)
ap.add_argument("--weights", default=None)
ap.add_argument("--tag", default="this")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--check", action="store_true")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args() if __name__ == "__main__" else None
if ARGS is not None:
    sys.path.insert(0, os.path.abspath(ARGS.root))
import torch  # noqa: E402

import bench  # noqa: E402
from openp5_amd._lib import hip_backend  # noqa: E402
from openp5_amd.trie import CompiledTrie  # noqa: E402

N_ITEMS, CLUSTERS, HEAD = 3416, 8, 100


def task(L, device):
    """the learnable task of bench.trained_generation_leg: batch(B, seed) -> (ids, ww, mask, labels, out_attn)"""
    items = bench.synth_items(N_ITEMS, 7)
    T = max(len(it) for it in items) - 1
    g = torch.Generator().manual_seed(4242)
    perms = [torch.randperm(N_ITEMS, generator=g)[:HEAD] for _ in range(CLUSTERS)]
    w = 1.0 / torch.arange(1, HEAD + 1, dtype=torch.float64) ** 1.2
    item_tok = torch.zeros(N_ITEMS, T, dtype=torch.long)
    for i, it in enumerate(items):
        item_tok[i, :len(it) - 1] = torch.tensor(it[1:])

    def batch(B, seed):
        ids, ww, mask, _, _ = bench.synth_batch(B, L, T, "cpu", seed)
        gg = torch.Generator().manual_seed(seed)
        cl = torch.randint(0, CLUSTERS, (B,), generator=gg)
        ids[:, 0] = 100 + cl
        tgt = torch.stack([perms[int(c)][int(r)] for c, r in zip(cl, torch.multinomial(w, B, replacement=True, generator=gg))])
        labels = item_tok[tgt]
        return [t.to(device) for t in (ids, ww, mask, labels, (labels != 0).long())]
    return items, batch


def window(fn, min_seconds):
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < min_seconds:
        fn()
        reps += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main(a):
    be = hip_backend()
    device = be.device
    cfg, model, opt = bench.build_model("t5-small", "bf16", device, be, 1, 0, total_steps=max(a.steps, 1))
    items, batch = task(a.L, device)
    final_loss = None
    if a.weights and os.path.exists(a.weights):
        model.load_state_dict(torch.load(a.weights, map_location="cpu"))
    else:
        model.train()
        pool = [batch(64, 9000 + i) for i in range(32)]
        loss = None
        for st in range(a.steps):
            loss = bench.train_step(model, opt, pool[st % len(pool)])
        final_loss = float(loss.detach()) if loss is not None else None
        if a.weights:
            os.makedirs(os.path.dirname(os.path.abspath(a.weights)), exist_ok=True)
            torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, a.weights)
    model.eval()
    ct = CompiledTrie.from_sequences([list(it) for it in items])
    ct.index_items([list(it) for it in items])
    rows = ct.rank_plan(cfg.decoder_start_token_id)["rows"]
    ids, ww, mask, _, _ = batch(a.users, 777)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, top_n=a.top_n)
    runs = {}
    for what in a.what.split(","):
        if what == "pruned":
            for s in (float(x) for x in a.slacks.split(",")):
                def run(s=s):
                    model.rank_prune_slack, model.rank_prune_max_fraction = s, a.fraction
                    return model.rank_items(generation_mode="verified", pruned=True, **kw)
                runs[("pruned", s)] = run
        else:
            runs[(what, None)] = lambda what=what: model.rank_items(generation_mode=what, **kw)
    for run in runs.values():              # warm-up: plan upload, workspaces, code objects
        run()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, run in runs.items():
            times[k].append(window(run, a.min_seconds))
    verified = runs[("verified", None)]()["item_index"].cpu() if a.check and ("verified", None) in runs else None
    lines = []
    for (what, s), run in runs.items():
        before = dict(model.rank_stats)
        out = run()
        st = {k: model.rank_stats[k] - before[k] for k in ("certified_users", "fallback_users", "declined_users") if k in before}
        dt = statistics.median(times[(what, s)])
        line = {"tag": a.tag, "what": what, "path": model.last_generate_path, "n_items": N_ITEMS, "rows_per_user": rows, "B": a.users, "L": a.L, "top_n": a.top_n,
                "train_steps": a.steps, "final_train_loss": final_loss, "ms_per_user": round(dt * 1e3 / a.users, 4),
                "ms_per_user_windows": [round(t * 1e3 / a.users, 4) for t in times[(what, s)]]}
        if what == "pruned":
            line.update({"slack": s, "max_fraction": a.fraction, "kept_rows_per_user": model.rank_stats["kept_rows_per_user"],
                         "kept_share": round(model.rank_stats["kept_rows_per_user"] / rows, 4), **{k: v / a.users for k, v in st.items()}})
            if verified is not None:
                line["lists_equal_verified"] = bool(torch.equal(out["item_index"].cpu(), verified))
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
