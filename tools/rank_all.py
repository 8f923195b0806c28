"""Exhaustive catalogue ranking timing (csrc/p5_rank.h): rank_items() for T5-small dims over the 3416-item synthetic trie of bench.py (the
ML-1M shape) and a 12,101-item one, fp32 (split products) and bf16 (generation_mode "draft": the bf16 engine).  Prints one JSON line per
(dtype, catalogue):
  users per second, ranked items per second (users x catalogue size: every item gets its exact score), ms per user,
  achieved FLOP/s of the pass from its row count (decoder projections + feed-forward + cross-attention + tied head per row),
  device ms per call split by kernel family (in-run profiler, p5_profile_begin / end: each launch's time includes its dispatch gap).
python tools/rank_all.py [--items 3416,12101] [--dtypes fp32,bf16] [--users 8] [--top_n 10] [--min_seconds 1.0] [--out FILE]"""
import argparse
import ctypes
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from openp5_amd._lib import hip_backend  # noqa: E402
from openp5_amd.model import P5ModelConfig, P5T5Native  # noqa: E402
from openp5_amd.trie import CompiledTrie  # noqa: E402

# kernel family <- kernel name prefixes (the GEMMs of the encoder, the decoder rows and a materialised-logits head are one family)
PARTS = (("tree_attention", ("p5_rank_tree_attn",)), ("cross_and_encoder_attention", ("p5_attn_fwd",)), ("head_and_edge_scores", ("p5_head_lse", "p5_rank_score")),
         ("item_scores_and_selection", ("p5_rank_items", "p5_rank_select")), ("gemm", ("p5_gemm", "p5_g4", "p5_g5", "p5_skinny")))


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
    return out


def pass_flops(cfg, rows, L):
    d, inner, F, V, NL, H = cfg.d_model, cfg.num_heads * cfg.d_kv, cfg.d_ff, cfg.vocab_size, cfg.num_decoder_layers, cfg.num_heads
    per_row = NL * 2 * (d * 3 * inner + 3 * inner * d + 2 * d * F) + NL * 4 * H * L * 64 + 2 * d * V
    return float(rows) * per_row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="3416,12101")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--users", type=int, default=8)
    ap.add_argument("--top_n", type=int, default=10)
    ap.add_argument("--min_seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = hip_backend()
    lines = []
    for dtype in a.dtypes.split(","):
        cfg = P5ModelConfig.from_backbone("t5-small", vocab_size=bench.V, dropout_rate=0.1)
        model = P5T5Native(cfg, dtype=dtype, backend=be, seed=2023)
        model.eval()
        model.generation_mode = "draft"
        for n_items in (int(x) for x in a.items.split(",")):
            t0 = time.perf_counter()
            ct = CompiledTrie.from_trie(bench.synth_item_trie(n_items, 7))
            ct.index_items(ct.enumerate_items())
            plan = ct.rank_plan(cfg.decoder_start_token_id)
            plan_s = time.perf_counter() - t0
            B, L = a.users, 128
            ids, ww, mask, _, _ = bench.synth_batch(B, L, 8, be.device, 500)
            kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, trie=ct, top_n=a.top_n)
            model.rank_items(**kw)                      # warm-up (plan upload, workspace, code objects)
            torch.cuda.synchronize()
            reps, t0 = 0, time.perf_counter()
            while reps < 3 or time.perf_counter() - t0 < a.min_seconds:
                model.rank_items(**kw)
                reps += 1
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            split = profile_split(model._lib, lambda: (model.rank_items(**kw), torch.cuda.synchronize()))
            flops = pass_flops(cfg, plan["rows"], L) * B
            line = {"dtype": dtype, "path": model.last_generate_path, "n_items": n_items, "rows_per_user": plan["rows"], "B": B,
                    "users_per_pass": model.rank_stats["users_per_pass"], "reps": reps, "ms_per_call": round(dt * 1e3, 3), "ms_per_user": round(dt * 1e3 / B, 3),
                    "users_per_s": round(B / dt, 2), "ranked_items_per_s": round(B * n_items / dt, 1), "pass_tflop_per_user": round(flops / B / 1e12, 4),
                    "achieved_tflops": round(flops / dt / 1e12, 2), "plan_build_s": round(plan_s, 3),
                    "ms_per_call_by_family": {k: round(v, 3) for k, v in split.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del model
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
