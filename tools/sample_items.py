"""Trie-constrained sampling timing (csrc/p5_sample.h): sample_items() at S draws per user next to the plain bf16 beam search
(generate(), generation_mode "draft") at K = S beams -- the same number of decode rows -- in the same process, on the benchmark's
3,416-item trie (the ML-1M shape), T5-small, B = 20 users, L = 128.  The two are alternated round by round, so that a drift of the machine
lands on both; one JSON line per configuration:
  ms per call (median and spread over the rounds), the draft search's ms from the same run, their ratio, the decode steps either runs,
  and the device ms of one sampling call split by phase (in-run profiler, p5_profile_begin / end: each launch's time includes its
  dispatch gap).
With --top_k / --top_p (csrc/p5_trunc.h) the truncated call is timed instead of the search, alternating with the untruncated call at the same
shape: "what": "sample_items_truncated", the two medians and their ratio.
python tools/sample_items.py [--rows 10,64] [--users 20] [--dtype bf16] [--rounds 7] [--min_seconds 0.5] [--top_k K] [--top_p P] [--tag NAME]
                             [--out FILE]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="10,64")
ap.add_argument("--users", type=int, default=20)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--min_seconds", type=float, default=0.5)
ap.add_argument("--top_k", type=int, default=0)
ap.add_argument("--top_p", type=float, default=1.0)
ap.add_argument("--tag", default="this")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
PARTS = (("selection", ("p5_sample_", "p5_trunc_sample_")), ("step_attention", ("p5_dec_self_attn", "p5_dec_cross_attn")), ("step_gemm", ("p5_skinny",)),
         ("step_norm_gelu", ("p5_rmsnorm_f32in", "p5_gated_gelu")), ("encoder_and_prefix_attention", ("p5_attn_fwd",)),
         ("encoder_and_prefix_gemm", ("p5_gemm", "p5_g4", "p5_g5")))


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
    cfg = P5ModelConfig.from_backbone("t5-small", vocab_size=bench.V, dropout_rate=0.1)
    ct = CompiledTrie.from_trie(bench.synth_item_trie(3416, 7))
    ct.index_items(ct.enumerate_items())
    B, L = a.users, 128
    model = P5T5Native(cfg, dtype=a.dtype, backend=be, seed=2023)
    model.eval()
    model.generation_mode = "draft"
    ids, ww, mask, _, _ = bench.synth_batch(B, L, 8, be.device, 500)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww)
    depth = int(ct.max_depth)
    lines = []
    for R in (int(x) for x in a.rows.split(",")):
        draw = lambda: model.sample_items(trie=ct, num_samples=R, seed=1, **kw)      # noqa: E731
        if a.top_k != 0 or a.top_p != 1.0:
            trunc = lambda: model.sample_items(trie=ct, num_samples=R, seed=1, top_k=a.top_k, top_p=a.top_p, **kw)      # noqa: E731
            for fn in (draw, trunc, draw, trunc):
                fn()
            torch.cuda.synchronize()
            t_draw, t_trunc = [], []
            for _ in range(a.rounds):
                t_draw.append(window(draw, a.min_seconds) * 1e3)
                t_trunc.append(window(trunc, a.min_seconds) * 1e3)
            md, mt = statistics.median(t_draw), statistics.median(t_trunc)
            line = {"tag": a.tag, "what": "sample_items_truncated", "dtype": a.dtype, "n_items": 3416, "max_children": int(ct.max_children), "B": B, "L": L,
                    "rows_per_user": R, "rounds": a.rounds, "top_k": a.top_k, "top_p": a.top_p, "sample_ms": round(md, 4),
                    "sample_ms_min_max": [round(min(t_draw), 4), round(max(t_draw), 4)], "truncated_ms": round(mt, 4),
                    "truncated_ms_min_max": [round(min(t_trunc), 4), round(max(t_trunc), 4)], "truncated_over_untruncated": round(mt / md, 4),
                    "truncated_ms_by_phase": profile_split(model._lib, lambda: (trunc(), torch.cuda.synchronize()))}
            lines.append(line)
            print(json.dumps(line), flush=True)
            continue
        search = lambda: model.generate(trie=ct, max_length=depth, num_beams=R, num_return_sequences=R, **kw)      # noqa: E731
        for fn in (draw, search, draw, search):          # warm-up: workspaces, code objects, the search's decode-step graph
            fn()
        torch.cuda.synchronize()
        path = model.last_generate_path
        t_draw, t_search = [], []
        for _ in range(a.rounds):
            t_draw.append(window(draw, a.min_seconds) * 1e3)
            t_search.append(window(search, a.min_seconds) * 1e3)
        md, ms = statistics.median(t_draw), statistics.median(t_search)
        forced = model.sample_stats["forced_prefix_steps"]
        line = {"tag": a.tag, "what": "sample_items", "dtype": a.dtype, "n_items": 3416, "B": B, "L": L, "rows_per_user": R, "rounds": a.rounds,
                "sample_ms": round(md, 4), "sample_ms_min_max": [round(min(t_draw), 4), round(max(t_draw), 4)],
                "draft_search_ms": round(ms, 4), "draft_search_ms_min_max": [round(min(t_search), 4), round(max(t_search), 4)],
                "draft_search_path": path, "sample_over_search": round(md / ms, 4), "within_5_percent": bool(md <= 1.05 * ms),
                "decode_steps": depth - 1 - forced, "forced_prefix_steps": forced,
                "sample_ms_by_phase": profile_split(model._lib, lambda: (draw(), torch.cuda.synchronize())),
                "draft_search_ms_by_phase": profile_split(model._lib, lambda: (search(), torch.cuda.synchronize()))}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
