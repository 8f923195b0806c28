"""Per-user candidate scoring timing (csrc/p5_cand.h): score_candidates() at C candidates per user next to rank_items() of the whole
catalogue on the same trie and users.  Two settings: T5-small dims over the 3416-item synthetic trie of bench.py (the ML-1M shape), and
a tiny-width model (d_model 64, one layer) over a 112,394-item trie (pieces 3, 3, 3: a Yelp-sized catalogue).  fp32 (split products)
and bf16 (generation_mode "draft": the bf16 engine).  Prints one JSON line per (setting, dtype, what):
  ms per user, users per second, rows per user, and the device ms of one call split by phase (in-run profiler, p5_profile_begin / end:
  each launch's time includes its dispatch gap).
`--root DIR` imports the package from another tree (a checkout of an earlier commit built in a second directory) and `--what rank`
times rank_items alone, so that the two builds can be alternated in one session; `--check` also records the largest difference between
score_candidates and rank_items scores of the same candidates.
python tools/cand_score.py [--settings ml1m,yelp] [--dtypes fp32,bf16] [--cands 20,100,1000] [--what cand,rank] [--users 8]
                           [--min_seconds 1.0] [--tag NAME] [--root DIR] [--check] [--out FILE]"""
import argparse
import ctypes
import json
import os
import random
import re
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--settings", default="ml1m,yelp")
ap.add_argument("--dtypes", default="fp32,bf16")
ap.add_argument("--cands", default="20,100,1000")
ap.add_argument("--what", default="cand,rank")
ap.add_argument("--users", type=int, default=8)
ap.add_argument("--min_seconds", type=float, default=1.0)
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
from openp5_amd.model import P5ModelConfig, P5T5Native  # noqa: E402
from openp5_amd.trie import CompiledTrie  # noqa: E402

# phase <- kernel name prefixes
PARTS = (("plan", ("p5_cand_plan", "p5_cand_hdr")), ("tree_attention", ("p5_cand_tree_attn", "p5_rank_tree_attn")),
         ("cross_and_encoder_attention", ("p5_attn_fwd",)),
         ("head_and_scoring", ("p5_head_lse", "p5_cand_lse", "p5_cand_score", "p5_rank_score", "p5_rank_items")),
         ("order", ("p5_cand_order", "p5_rank_select")), ("gemm", ("p5_gemm", "p5_g4", "p5_g5", "p5_skinny")))


def profile_split(lib, run):
    lib.p5_profile_begin()
    run()
    buf = ctypes.create_string_buffer(1 << 22)
    lib.p5_profile_end(buf, len(buf))
    rows = json.loads(buf.value.decode() or "[]")
    out = {name: 0.0 for name, _ in PARTS}
    out["other"] = 0.0
    for r in rows:
        kname = re.match(r"\(?(\w+)", r["kernel"]).group(1)
        for name, keys in PARTS:
            if any(kname.startswith(k) for k in keys):
                out[name] += r["total_us"] / 1e3
                break
        else:
            out["other"] += r["total_us"] / 1e3
    return {k: round(v, 3) for k, v in out.items()}


def timed(fn, min_seconds):
    fn()                                # warm-up (plan upload, workspace, code objects)
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < min_seconds:
        fn()
        reps += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, reps


def main(a):
    be = hip_backend()
    lines = []
    for setting in a.settings.split(","):
        if setting == "ml1m":
            cfg = P5ModelConfig.from_backbone("t5-small", vocab_size=bench.V, dropout_rate=0.1)
            trie, n_items = bench.synth_item_trie(3416, 7), 3416
        else:
            cfg = P5ModelConfig(vocab_size=bench.V, d_model=64, d_ff=128, num_layers=1, num_decoder_layers=1, num_heads=1, dropout_rate=0.1)
            trie, n_items = bench.synth_item_trie(112394, 7, pieces=(3, 3, 3)), 112394
        ct = CompiledTrie.from_trie(trie)
        ct.index_items(ct.enumerate_items())
        plan = ct.rank_plan(cfg.decoder_start_token_id)
        B, L = a.users, 128
        for dtype in a.dtypes.split(","):
            model = P5T5Native(cfg, dtype=dtype, backend=be, seed=2023)
            model.eval()
            model.generation_mode = "draft"
            ids, ww, mask, _, _ = bench.synth_batch(B, L, 8, be.device, 500)
            kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct)
            base = {"tag": a.tag, "setting": setting, "dtype": dtype, "n_items": n_items, "B": B, "L": L}
            if "rank" in a.what.split(","):
                run = lambda: model.rank_items(top_n=10, **kw)      # noqa: E731
                dt, reps = timed(run, a.min_seconds)
                lines.append({**base, "what": "rank_items", "path": model.last_generate_path, "rows_per_user": plan["rows"],
                              "users_per_pass": model.rank_stats["users_per_pass"], "reps": reps, "ms_per_user": round(dt * 1e3 / B, 4),
                              "users_per_s": round(B / dt, 2), "ms_per_call_by_phase": profile_split(model._lib, lambda: (run(), torch.cuda.synchronize()))})
                print(json.dumps(lines[-1]), flush=True)
            if "cand" in a.what.split(","):
                for C in (int(x) for x in a.cands.split(",")):
                    if setting != "ml1m" and C != 100:
                        continue
                    rnd = random.Random(1000 + C)
                    cand = torch.tensor([rnd.sample(range(n_items), C) for _ in range(B)], dtype=torch.int64)
                    run = lambda: model.score_candidates(candidates=cand, top_n=min(10, C), **kw)      # noqa: E731
                    dt, reps = timed(run, a.min_seconds)
                    line = {**base, "what": "score_candidates", "C": C, "path": model.last_generate_path, "rows_per_user": model.cand_stats["rows_per_user"],
                            "users_per_pass": model.cand_stats["users_per_pass"], "reps": reps, "ms_per_user": round(dt * 1e3 / B, 4),
                            "users_per_s": round(B / dt, 2), "ms_per_call_by_phase": profile_split(model._lib, lambda: (run(), torch.cuda.synchronize()))}
                    if a.check:
                        got = run()["scores"]
                        ref = torch.gather(model.rank_items(top_n=1, return_all_scores=True, **kw)["scores"], 1, cand.to(got.device))
                        line["max_abs_diff_vs_rank_items"] = float((got - ref).abs().max())
                        line["bit_equal_to_rank_items"] = bool(torch.equal(got, ref))
                    lines.append(line)
                    print(json.dumps(line), flush=True)
            del model
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
