"""Wide beam search timing (csrc/p5_decode_wide.h): generate() at widths 64 (narrow step), 65, 256, 1024 and 2354 (an ML-1M-shaped
width: generate_num + longest history) for T5-small dims, fp32 and bf16 (plain bf16 search, generation_mode "draft"), over the
3416-item synthetic trie of bench.py.  Prints one JSON line per (dtype, width):
  users / items per second (items = users x beams: every beam is a returned ranked item),
  device ms per decode step split into decoder / scoring / selection / scorer (in-run profiler, p5_profile_begin / end; hipGraph
  replay is off so that every launch is bracketed -- each launch's time includes its dispatch gap, see include/p5hip.h).
python tools/gen_wide.py [--widths 64,65,256,1024,2354] [--dtypes fp32,bf16] [--reps 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import re
import sys
import time

os.environ.setdefault("P5_NO_GRAPH", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from openp5_amd._lib import hip_backend  # noqa: E402
from openp5_amd.model import P5ModelConfig, P5T5Native  # noqa: E402
from openp5_amd.trie import prefix_allowed_tokens_fn  # noqa: E402

PARTS = (("scoring", ("p5_wide_score", "p5_dec_score")), ("selection", ("p5_wide_select",)),
         ("scorer", ("p5_wide_scorer", "p5_wide_commit")), ("select+scorer (narrow, one kernel)", ("p5_beam_step",)))   # kernel name prefixes


def profile_split(lib, run):
    lib.p5_profile_begin()
    run()
    buf = ctypes.create_string_buffer(1 << 22)
    lib.p5_profile_end(buf, len(buf))
    rows = json.loads(buf.value.decode() or "[]")
    out = {name: 0.0 for name, _ in PARTS}
    steps = 0
    for r in rows:
        kname = re.match(r"\(?(\w+)", r["kernel"]).group(1)          # "(p5_wide_score2_kernel<T>) ..." -> p5_wide_score2_kernel
        for name, keys in PARTS:
            if any(kname.startswith(k + "_kernel") or kname.startswith(k + "2_kernel") for k in keys):
                out[name] += r["total_us"] / 1e3
        if kname in ("p5_wide_score_kernel", "p5_wide_score2_kernel", "p5_dec_score_kernel", "p5_dec_score2_kernel"):
            steps += r["launches"]
    return out, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="64,65,256,1024,2354")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = hip_backend()
    fn = prefix_allowed_tokens_fn(bench.synth_item_trie(3416, 7))
    lines = []
    for dtype in a.dtypes.split(","):
        cfg = P5ModelConfig.from_backbone("t5-small", vocab_size=bench.V, dropout_rate=0.1)
        model = P5T5Native(cfg, dtype=dtype, backend=be, seed=2023)
        model.eval()
        model.generation_mode = "draft"
        for K in (int(x) for x in a.widths.split(",")):
            B = min(20, max(1, model.wide_max_rows // K))
            ids, ww, mask, _, _ = bench.synth_batch(B, 128, 8, be.device, 500)
            kw = dict(input_ids=ids, attention_mask=mask, whole_word_ids=ww, max_length=30, prefix_allowed_tokens_fn=fn, num_beams=K,
                      num_return_sequences=K, output_scores=True, return_dict_in_generate=True)
            model.generate(**kw)                       # warm-up (trie upload, workspaces, code objects)
            torch.cuda.synchronize()
            model.time_generate(True)
            t0 = time.perf_counter()
            dec = []
            for _ in range(a.reps):
                model.generate(**kw)
                dec.append(model.last_generate_timing()["decode_ms"])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.reps
            model.time_generate(False)
            split, steps = profile_split(model._lib, lambda: model.generate(**kw))
            steps = max(1, steps)
            dec_ms = sorted(dec)[len(dec) // 2]
            per = {k: v / steps for k, v in split.items()}
            per["decoder"] = max(0.0, dec_ms / steps - sum(per.values()))
            line = {"dtype": dtype, "K": K, "B": B, "path": "wide" if K > model.NARROW_MAX_K else "narrow", "ms_per_call": round(dt * 1e3, 3),
                    "users_per_s": round(B / dt, 2), "items_per_s": round(B * K / dt, 1), "decode_ms": round(dec_ms, 3), "steps": steps,
                    "ms_per_step": {k: round(v, 4) for k, v in per.items() if v > 0 or k == "decoder"}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del model
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
