"""The fixed-order embedding gradient (csrc/p5_embed.h, p5_op_embed_bwd mode 1) against a NumPy float32 REPLAY of its association, written
here from the header's description and never calling the library:
  * rows are ranked by a stable sort of (key, row);
  * inside a block of 32 sorted positions the rows of one key are added in sorted order, starting from 0;
  * a segment (all rows of one key) that lies inside one block writes table_old + a;
  * a piece of a segment that crosses a block boundary goes to part[block][0] (the segment began before the block) or part[block][1];
  * the block in which a crossing segment starts adds its own piece and then the later blocks' pieces in block order: table += a.
Every float32 operation above is one rounded addition, so the table must come out bit for bit.  Shapes are the smallest at which the
chain can go wrong (the ends of a block, of a half block and of the set; a key over several blocks; one or two key arrays, one or two sets);
each case runs twice over the same scratch, the second run over what the first left there."""
import numpy as np
import torch

from tests import cases
from tests.cases import GEMM_S, GEMM_STATE, P, dev, sync
from tests.elem_matrix import ELEM_R32

SEG = 32


def replay(keys, rows, table0):
    """float32 replay of the chain: keys int64 [n], rows float32 [n, d] (dropout already applied), table0 float32 [V, d]."""
    n, d = rows.shape
    table = table0.copy()
    perm = np.argsort(keys, kind="stable")
    skey = keys[perm]
    uniq, start, count = np.unique(skey, return_index=True, return_counts=True)
    which = np.searchsorted(uniq, skey)
    sstart, send = start[which], start[which] + count[which]
    nblk = (n + SEG - 1) // SEG
    part = np.full((nblk, 2, d), np.nan, dtype=np.float32)
    for b in range(nblk):
        p0, p1 = b * SEG, min(n, b * SEG + SEG)
        a = np.zeros(d, dtype=np.float32)
        for p in range(p0, p1):
            a = a + rows[perm[p]]
            if p == p1 - 1 or skey[p + 1] != skey[p]:
                head, tail = sstart[p] < p0, send[p] > p0 + SEG
                if not head and not tail:
                    table[skey[p]] = table0[skey[p]] + a
                else:
                    part[b, 0 if head else 1] = a
                a = np.zeros(d, dtype=np.float32)
    for b in range(nblk - 1):
        last = b * SEG + SEG - 1
        if send[last] <= b * SEG + SEG or sstart[last] < b * SEG:
            continue
        a = part[b, 1].copy()
        for bb in range(b + 1, (send[last] - 1) // SEG + 1):
            a = a + part[bb, 0]
        table[skey[last]] = table[skey[last]] + a
    assert table.dtype == np.float32
    return table


def _keys(kind, n, g):
    if kind == "random":              # a small vocabulary: repeats, segments of every length
        return torch.randint(0, max(2, n // 3), (n,), generator=g)
    if kind == "distinct":
        return torch.randperm(n, generator=g) + 1
    if kind == "long":                # 100 rows of key 0 (more than three blocks), the rest distinct, shuffled
        k = torch.cat([torch.zeros(100, dtype=torch.int64), torch.arange(1, n - 100 + 1)])
        return k[torch.randperm(n, generator=g)]
    if kind == "edge":
        # sorted: 20 x key 1, 12 x key 2 (ends exactly on the first block boundary), 16 x key 3 (ends on the middle of the second block),
        # 48 x key 4 (crosses into the third block and ends exactly on its end, position 96), the rest key 5
        k = torch.cat([torch.full((c,), v, dtype=torch.int64) for v, c in ((1, 20), (2, 12), (3, 16), (4, 48), (5, n - 96))])
        return k[torch.randperm(n, generator=g)]
    raise ValueError(kind)


# id, [(n, n0, key pattern, p0, p1) per set]
_SINGLE = [(1, 1), (1, 0), (31, 15), (32, 32), (32, 0), (33, 16), (65, 40)]
CASES = [(f"n{n}_n0_{n0}", [(n, n0, "random", 0.0, 0.0)]) for n, n0 in _SINGLE] + [
    ("long_key_130", [(130, 70, "long", 0.0, 0.0)]),
    ("distinct_65", [(65, 33, "distinct", 0.0, 0.0)]),
    ("block_edge_100", [(100, 50, "edge", 0.0, 0.0)]),
    ("two_sets_65_33", [(65, 40, "random", 0.0, 0.0), (33, 33, "random", 0.0, 0.0)]),
    ("two_sets_130_31", [(130, 0, "long", 0.0, 0.0), (31, 10, "distinct", 0.0, 0.0)]),
    ("dropout_130", [(130, 70, "long", 0.1, 0.25), (65, 65, "random", 0.5, 0.0)]),
]
DIMS = (64, 512)


def chain_case(be, d, sets_spec, seed=0):
    from openp5_amd._abi import P5EmbedBwdSet
    g = torch.Generator().manual_seed(seed + 977)
    rng = dev(be, torch.tensor(GEMM_STATE, dtype=torch.int32))
    sets = []
    for k, (n, n0, pat, p0, p1) in enumerate(sets_spec):
        keys = _keys(pat, n, g)
        dres = torch.randn(n, d, generator=g).float()
        table0 = torch.randn(int(keys.max()) + 2, d, generator=g).float()
        s0, s1 = 41 + 2 * k, 42 + 2 * k
        q = dict(n=n, n0=n0, n1=n - n0, keys=keys, dres=dres, table0=table0, s0=s0, s1=s1, p0=p0, p1=p1, exact=(p0 == 0.0 and p1 == 0.0),
                 key0=dev(be, keys[:n0].contiguous()) if n0 else None, key1=dev(be, keys[n0:].contiguous()) if n - n0 else None,
                 dres0=dev(be, dres[:n0].contiguous()) if n0 else None, dres1=dev(be, dres[n0:].contiguous()) if n - n0 else None,
                 idx=dev(be, torch.full((4 * n,), 0, dtype=torch.int32)), csort=dev(be, torch.full(((n + 255) // 256 * 256,), -1, dtype=torch.int64)),
                 part=dev(be, torch.full(((n + 31) // 32 * 2 * d,), float("nan"))))
        if q["exact"]:
            q["want"] = torch.from_numpy(replay(keys.numpy(), dres.numpy(), table0.numpy()))
        else:
            vals = dres.double().clone()
            for lo, hi, site, p in ((0, n0, s0, p0), (n0, n, s1, p1)):
                if hi > lo and p > 0:
                    vals[lo:hi] = cases._dropped(vals[lo:hi], cases._keep(site, (hi - lo) * d, p, (hi - lo, d)), p)
            q["ref"] = table0.double().index_add(0, keys, vals)
            q["bound"] = ELEM_R32 * q["ref"].abs() + GEMM_S * table0.double().abs().index_add(0, keys, vals.abs())
        sets.append(q)

    def run():
        arr = (P5EmbedBwdSet * len(sets))()
        tabs = []
        for k, q in enumerate(sets):
            t = dev(be, q["table0"].clone())
            tabs.append(t)
            a = arr[k]
            for f in ("key0", "key1", "dres0", "dres1", "idx", "csort", "part"):
                setattr(a, f, q[f].data_ptr() if q[f] is not None else None)
            a.n0, a.n1, a.site0, a.site1, a.drop_p0, a.drop_p1, a.table = q["n0"], q["n1"], q["s0"], q["s1"], q["p0"], q["p1"], t.data_ptr()
        be.check(be.lib.p5_op_embed_bwd(0, 1, len(sets), d, arr, P(rng), be.stream_ptr()), "embed_bwd")
        sync(be)
        return [t.cpu() for t in tabs]

    first, second = run(), run()          # the second run finds the first one's idx / csort / part
    for k, q in enumerate(sets):
        assert cases._same_bits(first[k], second[k]), f"set {k}: the second run over used scratch gave other bits"
        if q["exact"]:
            bad = (first[k].view(torch.int32) != q["want"].view(torch.int32)).nonzero()
            assert bad.numel() == 0, f"set {k}: {bad.shape[0]} elements differ from the float32 replay, first at (row, col) {bad[0].tolist()}"
        else:
            cases._elem_check(f"set {k} (dropout)", first[k], q["ref"], q["bound"])
