"""TEST-ONLY child process of tests/test_elem_ref_emu.py::test_embed_chain_is_independent_of_workgroup_order: runs the fixed-order embedding
gradient (p5_op_embed_bwd, mode 1) of libp5emu.so on the inputs cases.embed_ref_case dumped and prints the sha256 of the table gradients per
row.  The emulator reads P5_EMU_BLOCK_ORDER once per process, hence a process of its own; ctypes and numpy only, so it starts quickly."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from openp5_amd import _abi  # noqa: E402


def main(path):
    lib = _abi.bind(ctypes.CDLL(os.path.join(HERE, "libp5emu.so")))
    z = np.load(path)
    rng = np.array(json.loads(str(z["rng"])), dtype=np.int32)
    out = {}
    for rid, d, sets in json.loads(str(z["meta"])):
        arr = (_abi.P5EmbedBwdSet * len(sets))()
        keep, tabs = [], []
        for k, q in enumerate(sets):
            keys, dres, table = (np.ascontiguousarray(z[f"{rid}/{k}/{f}"]) for f in ("keys", "dres", "table0"))
            n, n0 = keys.shape[0], q["n0"]
            table = table.copy()
            bufs = dict(key0=keys[:n0].copy(), key1=keys[n0:].copy(), dres0=dres[:n0].copy(), dres1=dres[n0:].copy(), idx=np.zeros(4 * n, np.int32),
                        csort=np.zeros((n + 255) // 256 * 256, np.uint64), part=np.full((n + 31) // 32 * 2 * d, np.nan, np.float32))
            keep.append(bufs)
            tabs.append(table)
            a = arr[k]
            for f, b in bufs.items():
                setattr(a, f, b.ctypes.data if b.size else None)
            a.n0, a.n1, a.site0, a.site1, a.drop_p0, a.drop_p1, a.table = n0, n - n0, q["s0"], q["s1"], q["p0"], q["p1"], table.ctypes.data
        rc = lib.p5_op_embed_bwd(0, 1, len(sets), d, arr, rng.ctypes.data, None)
        assert rc == 0, lib.p5_last_error()
        h = hashlib.sha256()
        for t in tabs:
            h.update(t.tobytes())
        out[rid] = h.hexdigest()
    print("DIGESTS " + json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
