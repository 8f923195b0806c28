"""Stochastic beam search timing (csrc/p5_sbs.h): sample_slates() at S slates of K distinct items per user next to sample_items() at
S x K independent draws per user -- the same number of decode rows -- in the same process, on the benchmark's 3,416-item trie (the ML-1M
shape), T5-small, B = 20 users, L = 128.  The two are alternated round by round, so that a drift of the machine lands on both; one JSON
line per configuration:
  ms per call (median and spread over the rounds), sample_items' ms from the same run, their ratio, the decode steps either runs, and the
  device ms of one slate call split by phase (in-run profiler, p5_profile_begin / end: each launch's time includes its dispatch gap).
Nothing is gated: there is no time to beat, the numbers are recorded.
python tools/sample_slates.py [--sizes 10,100] [--slates 1,8] [--users 20] [--dtype bf16] [--rounds 7] [--min_seconds 0.5] [--tag NAME] [--out FILE]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10,100")
ap.add_argument("--slates", default="1,8")
ap.add_argument("--users", type=int, default=20)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--min_seconds", type=float, default=0.5)
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
PARTS = (("selection", ("p5_sbs_", "p5_sample_")), ("step_attention", ("p5_dec_self_attn", "p5_dec_cross_attn")), ("step_gemm", ("p5_skinny",)),
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
    ids, ww, mask, _, _ = bench.synth_batch(B, L, 8, be.device, 500)
    kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww)
    depth = int(ct.max_depth)
    lines = []
    for K in (int(x) for x in a.sizes.split(",")):
        for S in (int(x) for x in a.slates.split(",")):
            slates = lambda: model.sample_slates(trie=ct, slate_size=K, num_slates=S, seed=1, **kw)      # noqa: E731
            draws = lambda: model.sample_items(trie=ct, num_samples=S * K, seed=1, **kw)      # noqa: E731
            for fn in (slates, draws, slates, draws):          # warm-up: workspaces, code objects
                fn()
            torch.cuda.synchronize()
            calls0 = model.slate_stats["engine_calls"]
            out = slates()
            engine_calls = model.slate_stats["engine_calls"] - calls0
            distinct = float(sum(len(set(r.tolist())) for r in out["item_index"].cpu().view(B * S, K)) / (B * S))
            t_sl, t_dr = [], []
            for _ in range(a.rounds):
                t_sl.append(window(slates, a.min_seconds) * 1e3)
                t_dr.append(window(draws, a.min_seconds) * 1e3)
            msl, mdr = statistics.median(t_sl), statistics.median(t_dr)
            forced = model.slate_stats["forced_prefix_steps"]
            line = {"tag": a.tag, "what": "sample_slates", "dtype": a.dtype, "n_items": 3416, "B": B, "L": L, "slate_size": K, "num_slates": S,
                    "rows_per_user": S * K, "engine_calls": engine_calls, "rounds": a.rounds, "distinct_items_per_slate": distinct,
                    "slates_ms": round(msl, 4), "slates_ms_min_max": [round(min(t_sl), 4), round(max(t_sl), 4)],
                    "sample_items_ms": round(mdr, 4), "sample_items_ms_min_max": [round(min(t_dr), 4), round(max(t_dr), 4)],
                    "slates_over_sample_items": round(msl / mdr, 4), "decode_steps": depth - 1 - forced, "forced_prefix_steps": forced,
                    "slates_ms_by_phase": profile_split(model._lib, lambda: (slates(), torch.cuda.synchronize())),
                    "sample_items_ms_by_phase": profile_split(model._lib, lambda: (draws(), torch.cuda.synchronize()))}
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(ARGS)
