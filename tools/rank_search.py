"""Bounded trie search timing (csrc/p5_bound.h): rank_items(pruned="search") next to pruned=True (certified pruned ranking) and the full
pass ("verified") on the SAME trained weights and the SAME users, for a bf16 model (its fp32 verification engine decides) and an fp32
model, over the synthetic tries of bench.py with 3416 and 12101 items, at top_n 1, 10 and 100.

The recipe is that of tools/rank_pruned.py: a fresh T5-small is trained for `--steps` native steps on the learnable task of
bench.trained_generation_leg over the trie's items (only a model that puts real mass on the trie's tokens prunes), the weights go to
`--weights` (one file per trie; loaded when it exists, so another process -- another build, see --root -- times exactly the same model,
and the fp32 model loads what the bf16 model trained).  Every (what, top_n) is warmed up once, then timed in windows of at least
`--min_seconds` that ALTERNATE between them for `--rounds` rounds; a line reports the median window.  `--root DIR` imports the package
from another tree (a checkout of the parent commit built in a second directory; it has no search, so give it `--what verified,pruned`):
alternate the two builds in one session by alternating commands.
Appends one JSON line per (dtype, what, top_n) to `--out`: ms per user, the rounds and the rows reached (search) or kept (pruned), the
certified / fallback / declined shares, and with --check whether the lists equal the full pass's lists of this build token for token.
python tools/rank_search.py [--n_items 3416] [--dtype bf16] [--top_n 1,10,100] [--what search,pruned,verified] [--fraction 1.0]
                            [--steps 300] [--users 8] [--rounds 3] [--min_seconds 1.0] [--weights FILE] [--root DIR] [--tag NAME] [--check]
                            [--out profiles/rank_search.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--n_items", type=int, default=3416, help="3416 (5499 plan rows) | 12101")
ap.add_argument("--dtype", default="bf16", help="bf16 | fp32: the model that ranks (training is always bf16)")
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--users", type=int, default=8)
ap.add_argument("--L", type=int, default=128)
ap.add_argument("--top_n", default="1,10,100")
ap.add_argument("--what", default="search,pruned,verified")
ap.add_argument("--fraction", type=float, default=1.0, help="rank_search_max_fraction / rank_prune_max_fraction during the timing (1.0: never decline, "
                "so that the cost at every share of rows is seen)")
ap.add_argument("--seed_beams", type=int, default=0, help="rank_search_seed_beams (0: top_n)")
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

CLUSTERS, HEAD = 8, 100
SEARCH_STATS = ("search_certified_users", "search_fallback_users", "search_declined_users")
PRUNE_STATS = ("certified_users", "fallback_users", "declined_users")


def task(n_items, L, device):
    """the learnable task of bench.trained_generation_leg over n_items items: batch(B, seed) -> (ids, ww, mask, labels, out_attn)"""
    items = bench.synth_items(n_items, 7)
    T = max(len(it) for it in items) - 1
    g = torch.Generator().manual_seed(4242)
    perms = [torch.randperm(n_items, generator=g)[:HEAD] for _ in range(CLUSTERS)]
    w = 1.0 / torch.arange(1, HEAD + 1, dtype=torch.float64) ** 1.2
    item_tok = torch.zeros(n_items, T, dtype=torch.long)
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
    items, batch = task(a.n_items, a.L, device)
    final_loss = None
    if not (a.weights and os.path.exists(a.weights)):
        cfg, trainer, opt = bench.build_model("t5-small", "bf16", device, be, 1, 0, total_steps=max(a.steps, 1))
        trainer.train()
        pool = [batch(64, 9000 + i) for i in range(32)]
        loss = None
        for st in range(a.steps):
            loss = bench.train_step(trainer, opt, pool[st % len(pool)])
        final_loss = float(loss.detach()) if loss is not None else None
        state = {k: v.detach().cpu() for k, v in trainer.state_dict().items()}
        if a.weights:
            os.makedirs(os.path.dirname(os.path.abspath(a.weights)), exist_ok=True)
            torch.save(state, a.weights)
        del trainer, opt
    else:
        state = torch.load(a.weights, map_location="cpu")
    cfg, model, _ = bench.build_model("t5-small", a.dtype, device, be, 1, 0, total_steps=1)
    model.load_state_dict(state)
    model.eval()
    ct = CompiledTrie.from_sequences([list(it) for it in items])
    ct.index_items([list(it) for it in items])
    rows = ct.rank_plan(cfg.decoder_start_token_id)["rows"]
    ids, ww, mask, _, _ = batch(a.users, 777)
    runs = {}
    for n in (int(x) for x in a.top_n.split(",")):
        kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, top_n=n, generation_mode="verified")
        for what in a.what.split(","):
            if what == "search":
                def run(kw=kw):
                    model.rank_search_max_fraction, model.rank_search_seed_beams = a.fraction, (a.seed_beams or None)
                    return model.rank_items(pruned="search", **kw)
            elif what == "pruned":
                def run(kw=kw):
                    model.rank_prune_max_fraction = a.fraction
                    return model.rank_items(pruned=True, **kw)
            else:
                def run(kw=kw):
                    return model.rank_items(**kw)
            runs[(what, n)] = run
    for run in runs.values():              # warm-up: plan upload, workspaces, code objects
        run()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, run in runs.items():
            times[k].append(window(run, a.min_seconds))
    lines = []
    for (what, n), run in runs.items():
        before = dict(model.rank_stats)
        out = run()
        dt = statistics.median(times[(what, n)])
        line = {"tag": a.tag, "dtype": a.dtype, "what": what, "path": model.last_generate_path, "n_items": a.n_items, "rows_per_user": rows, "B": a.users,
                "L": a.L, "top_n": n, "train_steps": a.steps, "final_train_loss": final_loss, "ms_per_user": round(dt * 1e3 / a.users, 4),
                "ms_per_user_windows": [round(t * 1e3 / a.users, 4) for t in times[(what, n)]]}
        if what == "search":
            line.update({"max_fraction": a.fraction, "rounds": model.rank_stats["search_rounds"], "rows_reached": model.rank_stats["search_rows_per_user"],
                         "rows_share": round(model.rank_stats["search_rows_per_user"] / rows, 4),
                         **{k[len("search_"):]: (model.rank_stats[k] - before[k]) / a.users for k in SEARCH_STATS}})
        elif what == "pruned":
            line.update({"max_fraction": a.fraction, "rows_kept": model.rank_stats["kept_rows_per_user"],
                         "rows_share": round(model.rank_stats["kept_rows_per_user"] / rows, 4),
                         **{k: (model.rank_stats[k] - before[k]) / a.users for k in PRUNE_STATS}})
        if a.check and what != "verified" and ("verified", n) in runs:
            line["lists_equal_verified"] = bool(torch.equal(out["item_index"].cpu(), runs[("verified", n)]()["item_index"].cpu()))
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
