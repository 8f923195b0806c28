"""Row kernels (csrc/p5_elem.h: T5LayerNorm, cross-entropy, masked mean, embedding lookup, clip + AdamW) and the embedding gradient
(csrc/p5_embed.h) on the host emulation against float64 references (cases.rmsnorm_ref_case, ce_ref_case, masked_mean_ref_case,
embed_fwd_ref_case, embed_ref_case, adamw_ref_case): every row of tests/elem_matrix.py the emulator can afford."""
import json
import os
import subprocess
import sys

import pytest

from tests import cases
from tests.elem_matrix import EMBED, EMBED_ORDER, ROWS


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS if not r["gpu_only"]])
def test_elem_against_fp64(emu, row):
    cases.elem_ref_case(emu, row)


def test_embed_chain_is_independent_of_workgroup_order(emu, tmp_path):
    """The fixed-order embedding gradient gives the same bits with the emulator's workgroups run last-to-first.  P5_EMU_BLOCK_ORDER is read
    once per process: one fresh process (tests/emu/embed_chain_digest.py) runs the chain on the inputs of the rows of
    elem_matrix.EMBED_ORDER and prints the digests of their table gradients."""
    import numpy as np
    rows = [r for r in EMBED if r["id"] in EMBED_ORDER]
    assert len(rows) == len(EMBED_ORDER)
    dump = {}
    here = {r["id"]: cases.embed_ref_case(emu, r, dump=dump)[1] for r in rows}
    arrays, meta = {}, []
    for r in rows:
        meta.append([r["id"], r["d"], [{k: v for k, v in q.items() if k not in ("keys", "dres", "table0")} for q in dump[r["id"]]]])
        for k, q in enumerate(dump[r["id"]]):
            for f in ("keys", "dres", "table0"):
                arrays[f"{r['id']}/{k}/{f}"] = q[f]
    path = str(tmp_path / "embed_inputs.npz")
    np.savez(path, meta=json.dumps(meta), rng=json.dumps(list(cases.GEMM_STATE)), **arrays)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "embed_chain_digest.py")
    r = subprocess.run([sys.executable, child, path], env={**os.environ, "P5_EMU_BLOCK_ORDER": "reverse"}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    there = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DIGESTS ")][-1][8:])
    assert there == here, "the table gradient depends on the order the workgroups run in"
