"""The catalogue-ranking kernels (csrc/p5_rank.h, p5_cand.h, p5_prune.h, p5_bound.h, p5_tree_attn_row) against exact restatements and float64:
one *_case per family of tests/rank_matrix.py, shared by the emulator suite and the GPU suite.  Bounds and their constants: the head of
tests/rank_matrix.py."""
import ctypes

import numpy as np
import torch

from openp5_amd.model import relative_position_bucket_lut
from tests.cases import ATTN_TAU, GEMM_R, GEMM_S, P, TT, _elem_check, _same_bits, _sentinel, dev, prof_kernels, route_matches, sync
from tests.decode_cases import _softmax_pv
from tests.decode_matrix import ELEM_R32
from tests.rank_matrix import FANS, select_grid

TAU = ATTN_TAU[0]
NM = {0: "fp32", 1: "bf16"}
IS = -7                    # sentinel of integer outputs
F32 = np.float32


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32)


def _isent(*shape):
    return torch.full(shape, IS, dtype=torch.int32)


def _alpha(d):
    return float(F32(1.0) / np.sqrt(F32(d)))


def _run(be, row, call, sites):
    """run `call` with a profiler report taken; the report must name every (launch site, tag) of `sites`"""
    open_ = False
    try:
        be.check(be.lib.p5_profile_begin(), "p5_profile_begin")
        open_ = True
        be.check(call(), row["id"])
        sync(be)
        buf = ctypes.create_string_buffer(1 << 16)
        be.check(be.lib.p5_profile_end(buf, len(buf)), "p5_profile_end")
        open_ = False
    finally:
        if open_:
            be.lib.p5_profile_end(None, 0)
    keys = prof_kernels(buf.value.decode())
    for site, tag in sites:
        assert route_matches(keys, site, tag), f"{row['id']}: expected {site} [{tag}], the profiler saw {keys}"


def _flat_guard(n, tt, extra=64):
    """a flat sentinel buffer of n elements plus `extra` guard elements"""
    return _sentinel((n + extra,), tt)


def _tail_intact(tag, full, n):
    assert _same_bits(full[n:], _sentinel((full.numel() - n,), full.dtype)), f"{tag}: written past its {n} elements"


def _itail_intact(tag, full, n):
    assert bool((full.flatten()[n:] == IS).all()), f"{tag}: written past its {n} elements"


# ---- a synthetic trie and its plans, restated in plain Python ---------------------------------------------------------------------------------
class Trie:
    """parents[r]: parent row of plan row r (-1 for row 0), non-decreasing, so rows are numbered level by level; leaves[r]: leaf children of row
    r (each an item).  Node ids are a permutation of the rows (inner nodes) followed by the leaves; tokens of a node's children are distinct."""

    def __init__(self, parents, leaves, V, g, start=0):
        rows = len(parents)
        self.rows, self.parents = rows, list(parents)
        depth = [0] * rows
        for r in range(1, rows):
            assert 0 <= parents[r] < r and parents[r] >= parents[r - 1]
            depth[r] = depth[parents[r]] + 1
        self.depth = depth
        self.levels = max(depth) + 1
        kids = [[] for _ in range(rows)]
        for r in range(1, rows):
            kids[parents[r]].append(r)
        for r in range(rows):
            assert kids[r] or leaves[r] >= 1, "an inner node needs a child"
        perm = torch.randperm(rows, generator=g).tolist()
        n_items = int(sum(leaves))
        self.n_nodes = rows + n_items
        self.row_node = perm
        node_row = {perm[r]: r for r in range(rows)}
        child_off, child_tok, edge_row, edge_item = [0], [], [], []
        self.row_edge, self.row_tok = [-1] * rows, [start] * rows
        item_parent, item_edge, it = [], [], 0
        for node in range(self.n_nodes):
            if node in node_row:
                r = node_row[node]
                ch = [("row", c) for c in kids[r]] + [("leaf", None)] * leaves[r]
                order = torch.randperm(len(ch), generator=g).tolist()
                toks = (torch.randperm(V - 1, generator=g)[:len(ch)] + 1).tolist()
                for j, o in enumerate(order):
                    kind, c = ch[o]
                    e = len(child_tok)
                    child_tok.append(toks[j])
                    if kind == "row":
                        edge_row.append(c)
                        edge_item.append(-1)
                        self.row_edge[c], self.row_tok[c] = e, toks[j]
                    else:
                        edge_row.append(-1)
                        edge_item.append(it)
                        item_parent.append(r)
                        item_edge.append(e)
                        it += 1
            child_off.append(len(child_tok))
        self.child_off, self.child_tok, self.edge_row = child_off, child_tok, edge_row
        self.n_edges, self.n_items = len(child_tok), n_items
        md = self.levels
        self.anc = np.zeros((rows, md), dtype=np.int32)
        for r in range(1, rows):
            p, d = parents[r], depth[r]
            self.anc[r, :d - 1] = self.anc[p, :d - 1]
            self.anc[r, d - 1] = p
        # items: the edges and rows of the path, the tokens (column 0 = the start token)
        self.path_len = md
        self.item_edges = np.full((n_items, md), -1, dtype=np.int32)
        self.item_rows = np.full((n_items, md), -1, dtype=np.int32)
        self.item_tok = np.zeros((n_items, md + 2), dtype=np.int64)
        self.item_len = np.zeros(n_items, dtype=np.int32)
        self.item_tok[:, 0] = start
        for i in range(n_items):
            r = item_parent[i]
            chain = [int(a) for a in self.anc[r, :depth[r]]] + [r]            # rows of the prefixes at depth 0 .. depth[r]
            edges = [self.row_edge[c] for c in chain[1:]] + [item_edge[i]]
            n = len(edges)
            self.item_len[i] = n
            self.item_edges[i, :n] = edges
            self.item_rows[i, :n] = chain
            self.item_tok[i, 1:n + 1] = [child_tok[e] for e in edges]
        self.row_lmax = [d + 1 for d in depth]
        for i in range(n_items):
            for c in self.item_rows[i, :self.item_len[i]]:
                self.row_lmax[c] = max(self.row_lmax[c], int(self.item_len[i]))

    def chain(self, r):
        """rows on the path from depth 1 to r itself"""
        return [int(a) for a in self.anc[r, 1:self.depth[r]]] + ([r] if r else [])

    def closure(self, rows):
        out = {0}
        for r in rows:
            out.update(int(a) for a in self.anc[r, :self.depth[r]])
            out.add(r)
        return sorted(out)


def random_trie(rows, g, V=5000, step=0.45, max_leaves=2):
    parents = [-1]
    for r in range(1, rows):
        nxt = parents[-1] + (1 if float(torch.rand(1, generator=g)) < step else 0) if r > 1 else 0
        parents.append(min(max(nxt, 0), r - 1))
    has_kid = set(parents[1:])
    leaves = [int(torch.randint(0 if r in has_kid else 1, max_leaves + 1, (1,), generator=g)) for r in range(rows)]
    return Trie(parents, leaves, V, g)


def _path_sum32(lp, t, r):
    """P32(r): the edge log-probabilities on the path to row r summed in depth order in fp32"""
    Pv = F32(0.0)
    for a in t.chain(r):
        Pv = F32(Pv + lp[t.row_edge[a]])
    return Pv


# ---- edges, row_lse -----------------------------------------------------------------------------------------------------------------------------
def _edges_inputs(row, g):
    dtype, d, V, B, CQ, nchunk, rows = row["dtype"], row["d"], row["V"], row["B"], row["CQ"], row["nchunk"], row["rows"]
    tt = TT[dtype]
    R = B * CQ * nchunk
    hn = torch.randn(R, d, generator=g)
    E = torch.randn(V, d, generator=g)
    return tt, R, hn, E


def _logits64(hn, E, alpha):
    h64, e64 = hn.double(), E.double()
    lg = alpha * (h64 @ e64.t())
    e_l = GEMM_S * alpha * (h64.abs() @ e64.abs().t()) + ELEM_R32 * lg.abs()
    mx = lg.amax(-1)
    logsum = torch.log(torch.exp(lg - mx[:, None]).sum(-1))
    return lg, e_l, mx, logsum


def _engine_tile(be, row):
    nv = be.lib.p5_op_head_nv(row["dtype"], row["d"])
    assert nv == row["nv"], f"{row['id']}: the engine picks the head tile {nv} for this type and width, the table says {row['nv']}"


def _head_buf(row, tt):
    V, nv, HC = row["V"], row["nv"], row["HC"]
    n = 2 * HC * ((V + nv - 1) // nv) if nv else HC * ((V + 63) // 64 * 64)
    return _flat_guard(n, torch.float32), n


def edges_case(be, row, seed=0):
    dtype, d, V, B, CQ, nchunk, rows, HC, nv = (row[k] for k in ("dtype", "d", "V", "B", "CQ", "nchunk", "rows", "HC", "nv"))
    tag = row["id"]
    _engine_tile(be, row)
    g = torch.Generator().manual_seed(seed + 61)
    tt, R, hn, E = _edges_inputs(row, g)
    n_nodes = rows + 3
    row_node = torch.randperm(n_nodes, generator=g)[:rows].tolist()
    fans = [0] * n_nodes
    for r in range(rows):
        fans[row_node[r]] = FANS[r % len(FANS)]
    child_off = np.concatenate(([0], np.cumsum(fans))).astype(np.int32)
    n_edges = int(child_off[-1])
    child_tok = torch.randint(0, V, (n_edges,), generator=g).to(torch.int32)
    cap = rows
    if row["sel"]:
        n_rows = [0] * B
        sel = np.full((B, cap), -1, dtype=np.int32)
        for b in range(B):
            mine = list(range(0, rows, 2)) if b == 0 else ([rows - 1] if b == B - 1 else list(range(1, rows, 3)))
            n_rows[b] = len(mine)
            sel[b, :len(mine)] = mine
        plan_row = lambda b, ru: int(sel[b, ru]) if ru < n_rows[b] else -1      # noqa: E731
    else:
        plan_row = lambda b, ru: ru if ru < rows else -1      # noqa: E731
    pass_rows = []          # (g, b, plan row)
    for gi in range(R):
        b, ru = (gi // CQ) % B, (gi // (B * CQ)) * CQ + gi % CQ
        pr = plan_row(b, ru)
        if pr >= 0:
            pass_rows.append((gi, b, pr))
        else:
            hn[gi] = float("nan")          # a padding row: nothing of it may reach an edge
    alpha = _alpha(d)
    hn, E = hn.to(tt), E.to(tt)
    child_tok[int(child_off[row_node[pass_rows[1][2]]])] = V - 1          # the last row of E, which the NaN guard follows
    if row["peak"]:          # the first child of the first pass row leads by 120
        gi, b, pr = pass_rows[0]
        c0 = int(child_off[row_node[pr]])
        h = hn[gi].double()
        E[int(child_tok[c0])] = (h * (120.0 / (alpha * float((h * h).sum())))).to(tt)
    edge0 = _flat_guard(B * n_edges, torch.float32)
    head0, _ = _head_buf(row, tt)
    ed, hd, Ed, headd = dev(be, edge0), dev(be, hn), dev(be, torch.cat([E, _sentinel((1, d), tt)])), dev(be, head0)
    rnd, cod, ctd = dev(be, _i32(row_node)), dev(be, _i32(child_off)), dev(be, child_tok)
    seld = dev(be, _i32(sel)) if row["sel"] else None
    nrd = dev(be, _i32(n_rows)) if row["sel"] else None

    def call():
        return be.lib.p5_op_rank_edges(dtype, nv, P(ed), n_edges, P(hd), P(Ed), d, V, P(headd), HC, P(rnd), rows, B, CQ, nchunk, P(seld), P(nrd), cap, P(cod),
                                       P(ctd), be.stream_ptr())

    _run(be, row, call, [("p5_rank_score_kernel<T>", NM[dtype])] if nv else [("p5_rank_score_logits_kernel", "")])
    got = ed.cpu()
    _tail_intact(f"{tag} edge_lp", got, B * n_edges)
    got = got[:B * n_edges].view(B, n_edges)
    live = [i for i in range(R) if not bool(torch.isnan(hn[i].float()).any())]
    lg, e_l, mx, logsum = _logits64(hn[live], E, alpha)
    at = {gi: k for k, gi in enumerate(live)}
    owned = torch.zeros(B, n_edges, dtype=torch.bool)
    ref = torch.zeros(B, n_edges, dtype=torch.float64)
    bound = torch.ones(B, n_edges, dtype=torch.float64)
    for gi, b, pr in pass_rows:
        k, nd = at[gi], row_node[pr]
        c0, c1 = int(child_off[nd]), int(child_off[nd + 1])
        tok = child_tok[c0:c1].long()
        l, lse = lg[k, tok], mx[k] + logsum[k]
        ref[b, c0:c1] = l - lse
        bound[b, c0:c1] = (e_l[k, tok] if nv else 0.0) + TAU * (mx[k].abs() + logsum[k].abs()) + 3 * ELEM_R32 * (l.abs() + lse.abs())
        owned[b, c0:c1] = True
    assert _same_bits(got[~owned], _sentinel((int((~owned).sum()),), torch.float32)), f"{tag}: an edge of a row that is not in the pass was written"
    if row["peak"]:
        gi, b, pr = pass_rows[0]
        c0 = int(child_off[row_node[pr]])
        assert float(ref[b, c0]) > -1e-3 and (FANS[pr % len(FANS)] == 1 or float(ref[b, c0 + 1]) < -100.0), f"{tag}: the inputs do not hold the peaked row"
    return _elem_check(tag, got[owned], ref[owned], bound[owned])


def row_lse_case(be, row, seed=0):
    dtype, d, V, HC, nv = (row[k] for k in ("dtype", "d", "V", "HC", "nv"))
    tag = row["id"]
    _engine_tile(be, row)
    g = torch.Generator().manual_seed(seed + 67)
    tt, R, hn, E = _edges_inputs(row, g)
    hn[1] *= 25.0          # logits beyond +-80
    hn, E = hn.to(tt), E.to(tt)
    alpha = _alpha(d)
    out0 = _flat_guard(R, torch.float32)
    head0, _ = _head_buf(row, tt)
    od, hd, Ed, headd = dev(be, out0), dev(be, hn), dev(be, E), dev(be, head0)

    def call():
        return be.lib.p5_op_cand_row_lse(dtype, nv, P(od), P(hd), P(Ed), d, V, P(headd), HC, R, be.stream_ptr())

    _run(be, row, call, [("p5_cand_lse_kernel" if nv else "p5_cand_lse_logits_kernel", "")])
    got = od.cpu()
    _tail_intact(f"{tag} row_lse", got, R)
    lg, e_l, mx, logsum = _logits64(hn, E, alpha)
    ref = mx + logsum
    bound = TAU * (mx.abs() + logsum.abs()) + ELEM_R32 * ref.abs()
    if nv:
        bound = bound + e_l.amax(-1)
        if dtype == 1:      # the streaming head's fast exponential in bf16 (decode_matrix: head_lse)
            bound = bound + ELEM_R32 * (lg - mx[:, None]).abs().clamp(max=88.0).amax(-1)
    return _elem_check(tag, got[:R], ref, bound)


# ---- items ----------------------------------------------------------------------------------------------------------------------------------------
def items_case(be, row, seed=0):
    n_items, path_len, B = row["n_items"], row["path_len"], row["B"]
    tag = row["id"]
    g = torch.Generator().manual_seed(seed + 71)
    n_edges = 3 * n_items + 5
    lp = (-torch.rand(B, n_edges, generator=g) * 12.0).float()
    lp[:, ::7] *= 1e-3
    ie = torch.randint(0, n_edges, (n_items, path_len), generator=g).to(torch.int32)
    ln = torch.randint(1, path_len + 1, (n_items,), generator=g)
    if n_items >= 3:
        ln[n_items // 2] = 0          # -1 in column 0: no edge at all
        ln[0] = path_len
    for i in range(n_items):
        ie[i, int(ln[i]):] = -1
    out0 = _flat_guard(B * n_items, torch.float32)
    od, lpd, ied = dev(be, out0), dev(be, lp), dev(be, ie)

    def call():
        return be.lib.p5_op_rank_select(2, P(od), P(lpd), n_edges, P(ied), n_items, path_len, None, None, B, 1, None, None, None, be.stream_ptr())

    _run(be, row, call, [("p5_rank_items_kernel", "")])
    got = od.cpu()
    _tail_intact(f"{tag} scores", got, B * n_items)
    lpn, ien = lp.numpy(), ie.numpy()
    ref = np.zeros((B, n_items), dtype=F32)
    for b in range(B):
        for i in range(n_items):
            s, n = F32(0.0), 0
            for e in ien[i]:
                if e < 0:
                    break
                s = F32(s + lpn[b, e])
                n += 1
            ref[b, i] = F32(s / F32(n)) if n else F32(-1.0e9)
    assert _same_bits(got[:B * n_items].view(B, n_items), torch.from_numpy(ref)), f"{tag}: item scores differ from the fp32 restatement"
    return 0.0


# ---- select ---------------------------------------------------------------------------------------------------------------------------------------
def _select_scores(row, g):
    n, N, B, S, pattern = row["n_items"], row["top_n"], row["B"], row["S"], row["pattern"]
    sc = torch.randn(B, n, generator=g)
    if pattern == "equal":
        sc[:] = 1.5
    elif pattern == "two":          # the cut falls inside the run of the lower value
        sc[:] = 1.0
        for b in range(B):
            sc[b, torch.randperm(n, generator=g)[:max(N // 2, 0)]] = 2.0
    elif pattern == "oneslice":     # the whole top N lies in the second slice
        k = min(N, n - S)
        for b in range(B):
            sc[b, S + torch.randperm(min(S, n - S), generator=g)[:k]] += 100.0
    elif pattern == "mixed":
        vals = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, float("-inf"), 3.0e38, -3.0e38, 1.0, -1.0, 1.0000001])
        sc = vals[torch.randint(0, len(vals), (B, n), generator=g)]
    elif pattern == "zeros":        # both zeros on top, in both index orders; everything else below
        sc = -sc.abs() - 1.0
        for b in range(B):
            idx = torch.randperm(n, generator=g)[:min(max(2, 2 * N // 3), n)]
            sc[b, idx] = torch.where(torch.rand(idx.numel(), generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
            lo = idx.sort().values
            sc[b, lo[0]], sc[b, lo[1]] = -0.0, 0.0
    return sc.float().contiguous()


def _select_excl(row, g):
    n, N, B, S, excl = row["n_items"], row["top_n"], row["B"], row["S"], row["excl"]
    if excl is None:
        return None, torch.zeros(B, n, dtype=torch.bool)
    words = (n + 31) // 32
    bits = torch.zeros(B, words * 32, dtype=torch.bool)
    if excl == "some":
        bits[:, :n] = torch.rand(B, n, generator=g) < 0.2
    elif excl == "all":
        bits[:, :n] = True
    elif excl == "few":             # fewer live items than top_n
        bits[:, :n] = True
        for b in range(B):
            bits[b, torch.randperm(n, generator=g)[:max(N - 3, 0)]] = False
    elif excl == "slice0":          # the first slice holds fewer live items than top_n
        bits[:, :n] = torch.rand(B, n, generator=g) < 0.2
        bits[:, :min(S, n)] = True
        for b in range(B):
            bits[b, torch.randperm(min(S, n), generator=g)[:N // 2]] = False
    bits[:, n:] = True              # bits past n_items in the last word
    wgt = 2 ** torch.arange(32, dtype=torch.int64)
    wd = (bits.view(B, words, 32).long() * wgt).sum(-1)
    wd = torch.where(wd >= 2 ** 31, wd - 2 ** 32, wd).to(torch.int32)
    return wd, bits[:, :n]


def select_case(be, row, seed=0):
    n, N, B, G = row["n_items"], row["top_n"], row["B"], row["G"]
    tag = row["id"]
    assert (G, row["S"]) == select_grid(n, N)
    g = torch.Generator().manual_seed(seed + 73)
    sc = _select_scores(row, g)
    wd, dead = _select_excl(row, g)
    part0 = torch.full((B * G * N + 16,), IS, dtype=torch.int64)
    oi0, os0 = _isent(B + 1, N), _sentinel((B + 1, N), torch.float32)
    scd, wdd, partd, oid, osd = dev(be, sc), (dev(be, wd) if wd is not None else None), dev(be, part0), dev(be, oi0), dev(be, os0)
    grid = (ctypes.c_int * 2)(0, 0)

    def call():
        return be.lib.p5_op_rank_select(0, P(scd), None, 0, None, n, 1, P(wdd), P(partd), B, N, P(oid), P(osd), ctypes.cast(grid, ctypes.c_void_p),
                                        be.stream_ptr())

    _run(be, row, call, [("p5_rank_select_part_kernel", ""), ("p5_rank_select_kernel", "")])
    assert (grid[0], grid[1]) == (G, row["S"]), f"{tag}: the launcher's grid is {grid[0]} x {grid[1]}, the row expects {G} x {row['S']}"
    assert _same_bits(scd.cpu(), sc), f"{tag}: the scores changed"
    assert bool((partd.cpu()[B * G * N:] == IS).all()), f"{tag}: written past the first stage's scratch"
    oi, os_ = oid.cpu(), osd.cpu()
    assert bool((oi[B] == IS).all()) and _same_bits(os_[B], os0[B]), f"{tag}: written past the last user"
    scn = sc.numpy()
    canon = np.where(scn == 0, F32(0.0), scn)          # a zero of either sign is one score
    for b in range(B):
        live = np.nonzero(~dead[b].numpy())[0]
        order = live[np.lexsort((live, -canon[b, live].astype(np.float64)))][:N]
        L = len(order)
        want_i = np.full(N, -1, dtype=np.int32)
        want_s = np.full(N, -1.0e9, dtype=F32)
        want_i[:L], want_s[:L] = order, canon[b, order]
        gi, gs = oi[b].numpy(), os_[b].numpy()
        if not np.array_equal(gi, want_i):
            k = int(np.nonzero(gi != want_i)[0][0])
            raise AssertionError(f"{tag}: user {b} rank {k}: item {gi[k]} (score {gs[k]!r}), expected item {want_i[k]} (score {want_s[k]!r}); {L} live of {n}")
        assert np.array_equal(gs.view(np.int32), want_s.view(np.int32)), f"{tag}: user {b}: returned scores differ in their bits"
    return 0.0


# ---- tree attention ---------------------------------------------------------------------------------------------------------------------------------
LUT_HALF = 128


def tree_attn_case(be, row, seed=0):
    dtype, variant, H, D, B = row["dtype"], row["variant"], row["H"], row["depth"], row["B"]
    tt, tag, inner = TT[dtype], row["id"], row["H"] * 64
    g = torch.Generator().manual_seed(seed + 79)
    # the plan: a chain of depth 0 .. D; every chain row also has a side row (leaves only), so chain rows and side rows alternate in level order
    parents = [-1]
    chain = [0]
    for dd in range(1, D + 1):
        parents += [chain[-1], chain[-1]]
        chain.append(len(parents) - 2)
    rows = len(parents)
    has_kid = set(parents[1:])
    t = Trie(parents, [0 if r in has_kid else 1 for r in range(rows)], 5000, g)
    md = t.levels
    depth = t.depth
    if variant == 1:          # ragged sel: user 0 the chain alone (positions differ from rows), the last user its first rows, others every row
        sels = [chain if b == 0 else (chain[:min(10, len(chain))] if b == B - 1 else list(range(rows))) for b in range(B)]
    else:
        sels = [list(range(rows)) for _ in range(B)]
    per_user = max(len(s) for s in sels)
    nchunk = 2 if per_user > 1 else 1
    CQ = ((per_user + 3 + nchunk - 1) // nchunk + 15) // 16 * 16          # at least three padding rows; with two chunks, ancestors lie in the other chunk
    if variant == 2:
        nchunk, CQ = 1, per_user + 3
    R = B * CQ * nchunk
    pass_row = lambda b, ru: ((ru // CQ) * B + b) * CQ + ru % CQ      # noqa: E731
    qkv = torch.randn(R, 3 * inner, generator=g)
    if row["bias"] == "rising":          # one q for all; the key of a row of depth t gives q . k = 0.5 t
        q = torch.randn(inner, generator=g)
        qkv[:, :inner] = q
        for b in range(B):
            for ru, pr in enumerate(sels[b]):
                qh = q.view(H, 64)
                qkv[pass_row(b, ru), inner:2 * inner] = (qh * (0.5 * depth[pr] / (qh * qh).sum(-1, keepdim=True))).reshape(inner)
    qkv = qkv.to(tt)
    lut = relative_position_bucket_lut(LUT_HALF, False, 32, 128).to(torch.int32)
    rel = torch.randn(32, H, generator=g)
    if row["bias"] == "big":
        rel[int(lut[LUT_HALF - 1])] = 30.0 * torch.sign(torch.randn(H, generator=g))
    # keys of every pass row: the pass rows of its ancestors by depth, then itself; padding rows: themselves alone
    keys = [[gi] for gi in range(R)]
    for b in range(B):
        pos = {pr: ru for ru, pr in enumerate(sels[b])}
        for ru, pr in enumerate(sels[b]):
            keys[pass_row(b, ru)] = [pass_row(b, pos[int(a)]) for a in t.anc[pr, :depth[pr]]] + [pass_row(b, ru)]
    out0 = _sentinel((R + 1, inner), tt)
    outd, qd, reld, lutd = dev(be, out0), dev(be, qkv), dev(be, rel), dev(be, lut)
    cap = rows
    if variant == 2:          # per-user plans: depth per pass row, anc [B][cap][md] over the user's own row numbers
        cap = CQ
        dflat = np.zeros(B * CQ, dtype=np.int32)
        anc = np.full((B, cap, md), 0, dtype=np.int32)
        for b in range(B):
            for ru, pr in enumerate(sels[b]):
                dflat[b * CQ + ru] = depth[pr]
                anc[b, ru] = t.anc[pr]
        depd, ancd, seld, nrd = dev(be, _i32(dflat)), dev(be, _i32(anc)), None, None
    else:
        depd, ancd = dev(be, _i32(depth)), dev(be, _i32(t.anc))
        sel = np.full((B, cap), -1, dtype=np.int32)
        for b in range(B):
            sel[b, :len(sels[b])] = sels[b]
        seld, nrd = (dev(be, _i32(sel)), dev(be, _i32([len(s) for s in sels]))) if variant == 1 else (None, None)

    def call():
        return be.lib.p5_op_tree_attn(dtype, variant, P(outd), P(qd), P(depd), P(ancd), rows, md, B, CQ, nchunk, P(seld), P(nrd), cap, P(reld), P(lutd),
                                      LUT_HALF, H, be.stream_ptr())

    site = ("p5_rank_tree_attn_kernel<T>", "p5_cand_tree_attn_kernel<T>", "p5_tree_attn_kernel<T>")[variant]
    _run(be, row, call, [(site, NM[dtype])])
    out = outd.cpu()
    assert _same_bits(out[R:], out0[R:]), f"{tag}: written past the pass"
    n = max(len(k) for k in keys)
    idx = torch.zeros(R, n, dtype=torch.long)
    valid = torch.zeros(R, n, dtype=torch.bool)
    bias_i = torch.zeros(R, n, dtype=torch.long)
    for gi, k in enumerate(keys):
        idx[gi, :len(k)] = torch.tensor(k)
        valid[gi, :len(k)] = True
        bias_i[gi, :len(k)] = lut[torch.arange(len(k)) - (len(k) - 1) + LUT_HALF].long()
    q64 = qkv[:, :inner].double().view(R, H, 1, 64)
    k64 = qkv[:, inner:2 * inner].double().view(R, H, 64)[idx].permute(0, 2, 1, 3)          # [R, H, n, 64]
    v64 = qkv[:, 2 * inner:].double().view(R, H, 64)[idx].permute(0, 2, 1, 3)
    bias = rel.double()[bias_i].permute(0, 2, 1)                                           # [R, H, n]
    s = (q64 * k64).sum(-1) + bias
    S_abs = (q64.abs() * k64.abs()).sum(-1)
    vm = valid[:, None, :].expand(R, H, n)
    O, S_o, e, _ = _softmax_pv(s, S_abs, v64, vm, bias.abs())
    ref, S_o = O.reshape(R, inner), S_o.reshape(R, inner)
    r_out = GEMM_R[True] if dtype == 1 else ELEM_R32
    bound = r_out * ref.abs() + ((2 * e + TAU + GEMM_S).expand(R, H, 64).reshape(R, inner)) * S_o
    pad = torch.tensor([len(k) == 1 for k in keys])
    assert int(pad.sum()) >= 3 * B
    assert _same_bits(out[:R][pad], qkv[:, 2 * inner:][pad]), f"{tag}: a row without ancestors (padding rows among them) must return its own V"
    return _elem_check(tag, out[:R], ref, bound)


# ---- candidates -------------------------------------------------------------------------------------------------------------------------------------
def _trie_of_levels(levels, g, n_items=40, width=9):
    """a trie of exactly `levels` levels of rows (`width` rows on every level behind the first) and at least n_items items"""
    parents, first = [-1], 0
    for lv in range(1, levels):
        lo, hi = (0, 1) if lv == 1 else (first, len(parents))
        first = len(parents)
        parents += sorted(torch.randint(lo, hi, (width,), generator=g).tolist())
    rows = len(parents)
    has_kid = set(parents[1:])
    leaves = [0 if r in has_kid and float(torch.rand(1, generator=g)) < 0.5 else 1 for r in range(rows)]
    while sum(leaves) < n_items:
        for r in range(rows):
            leaves[r] += 1 if leaves[r] or r not in has_kid else 0
        if not any(leaves):
            leaves[0] = 1
    t = Trie(parents, leaves, 5000, g)
    assert t.levels == levels and t.n_items >= n_items
    return t


def cand_plan_case(be, row, seed=0):
    B, C, pl = row["B"], row["C"], row["path_len"]
    tag = row["id"]
    g = torch.Generator().manual_seed(seed + 83)
    t = _trie_of_levels(pl, g)
    assert t.path_len == pl
    cand = torch.randint(0, t.n_items, (B, C), generator=g)
    kinds = torch.rand(B, C, generator=g)
    cand[kinds < 0.1] = -1
    cand[(kinds >= 0.1) & (kinds < 0.2)] = t.n_items + 3
    if C >= 4:
        cand[:, 1] = cand[:, 0]          # a duplicate
        cand[B - 1, :] = cand[B - 1, 0]  # one user names one item C times: shared prefixes only
    if "hdr" in tag:                     # every user a different row count: the largest sits at a user of the last wave-stride trip
        for b in range(B):
            cand[b] = -1
        cand[B - 1, 0] = int(np.argmax(t.item_len))
        cand[0, 0] = int(np.argmin(t.item_len))
    cand = cand.to(torch.int32)
    cap = C * pl
    Pk = 256
    while Pk < cap:
        Pk <<= 1
    sel0, nr0, hdr0 = _isent(B + 1, cap), _isent(B + 4), _isent(8)
    keys0 = torch.full((B * Pk + 16,), IS, dtype=torch.int64)
    seld, nrd, hdrd, keyd, cd, ird = dev(be, sel0), dev(be, nr0), dev(be, hdr0), dev(be, keys0), dev(be, cand), dev(be, _i32(t.item_rows))

    def call():
        return be.lib.p5_op_cand_plan(P(seld), P(nrd), P(hdrd), P(keyd), P(cd), P(ird), B, C, t.n_items, pl, cap, Pk, be.stream_ptr())

    _run(be, row, call, [("p5_cand_plan_kernel", ""), ("p5_cand_hdr_kernel", "")])
    sel, nr, hdr = seld.cpu(), nrd.cpu(), hdrd.cpu()
    assert bool((keyd.cpu()[B * Pk:] == IS).all()), f"{tag}: written past the sort keys"
    _itail_intact(f"{tag} n_rows", nr, B)
    _itail_intact(f"{tag} hdr", hdr, 1)
    assert bool((sel[B] == IS).all()), f"{tag}: sel written past the last user"
    most = 0
    for b in range(B):
        want = sorted({int(r) for c in cand[b].tolist() if 0 <= c < t.n_items for r in t.item_rows[c] if r >= 0})
        assert int(nr[b]) == len(want) and sel[b, :len(want)].tolist() == want, f"{tag}: user {b}: sel {sel[b, :int(nr[b])].tolist()[:12]}, expected {want[:12]}"
        assert bool((sel[b, len(want):] == IS).all()), f"{tag}: user {b}: sel written past its rows"
        most = max(most, len(want))
    assert int(hdr[0]) == most, f"{tag}: header {int(hdr[0])}, the largest row count is {most}"
    return 0.0


def _ragged_sel(t, B, per_user, g):
    """ancestor-closed row sets: user 0 everything that fits, the last user row 0 alone, others random"""
    sels = []
    for b in range(B):
        if b == 0:
            s = list(range(min(t.rows, per_user)))
        elif b == B - 1:
            s = [0]
        else:
            s = t.closure(torch.randperm(t.rows, generator=g)[:max(per_user // 4, 1)].tolist())[:per_user]
            s = [r for r in s if all(int(a) in s for a in t.anc[r, :t.depth[r]])]
        sels.append(s)
    return sels


def cand_rows_case(be, row, seed=0):
    B, CQ, nchunk = row["B"], row["CQ"], row["nchunk"]
    tag = row["id"]
    g = torch.Generator().manual_seed(seed + 89)
    t = random_trie(min(CQ * nchunk - 3, 300), g)
    sels = _ragged_sel(t, B, CQ * nchunk - 3, g)
    cap = t.rows + 2
    sel = np.full((B, cap), 10 ** 6, dtype=np.int32)          # (an entry past n_rows must not be followed)
    for b in range(B):
        sel[b, :len(sels[b])] = sels[b]
    R = B * CQ * nchunk
    ids0 = torch.full((R + 8,), IS, dtype=torch.int64)
    idd, rtd, seld, nrd = dev(be, ids0), dev(be, _i32(t.row_tok)), dev(be, _i32(sel)), dev(be, _i32([len(s) for s in sels]))
    pad_id = 4999

    def call():
        return be.lib.p5_op_cand_rows(P(idd), P(rtd), B, CQ, nchunk, P(seld), P(nrd), cap, pad_id, be.stream_ptr())

    _run(be, row, call, [("p5_cand_rows_kernel", "")])
    ids = idd.cpu()
    assert bool((ids[R:] == IS).all()), f"{tag}: written past the pass"
    want = torch.full((R,), pad_id, dtype=torch.int64)
    for b in range(B):
        for ru, pr in enumerate(sels[b]):
            want[((ru // CQ) * B + b) * CQ + ru % CQ] = t.row_tok[pr]
    assert torch.equal(ids[:R], want), f"{tag}: decoder input ids differ"
    return 0.0


def cand_score_case(be, row, seed=0):
    dtype, C, N, d, B, pl = row["dtype"], row["C"], row["top_n"], row["d"], row["B"], row["path_len"]
    tt, tag = TT[dtype], row["id"]
    g = torch.Generator().manual_seed(seed + 97)
    t = _trie_of_levels(pl, g, n_items=C + 7)
    V = 5000
    cand = torch.stack([torch.randperm(t.n_items, generator=g)[:C] for _ in range(B)])          # a user's items are distinct (p5_cand_order_kernel)
    kinds = torch.rand(B, C, generator=g)
    cand[kinds < 0.1] = -1
    cand[(kinds >= 0.1) & (kinds < 0.15)] = t.n_items + 1
    cand = cand.to(torch.int32)
    sels = [sorted({int(r) for c in cand[b].tolist() if 0 <= c < t.n_items for r in t.item_rows[c] if r >= 0}) or [0] for b in range(B)]
    per_user = max(len(s) for s in sels)
    nchunk = 2 if per_user > 16 else 1
    CQ = ((per_user + nchunk - 1) // nchunk + 15) // 16 * 16
    R = B * CQ * nchunk
    cap = t.rows
    sel = np.full((B, cap), -1, dtype=np.int32)
    for b in range(B):
        sel[b, :len(sels[b])] = sels[b]
    hn = torch.randn(R, d, generator=g)
    E = torch.randn(V, d, generator=g)
    lse = (torch.randn(R, generator=g) * 2.0 + 6.0).float()
    if row["ties"]:          # one h, one e, one lse: items of equal length score the same bits
        hn[:] = hn[0]
        E[:] = E[0]
        lse[:] = lse[0]
    hn, E = hn.to(tt), E.to(tt)
    alpha = _alpha(d)
    for c in cand[0].tolist():          # the first live candidate ends on the last row of E, which the NaN guard follows
        if 0 <= c < t.n_items:
            t.item_tok[c, int(t.item_len[c])] = V - 1
            break
    sc0 = _flat_guard(B * C, torch.float32)
    oo0, oi0, os0 = _isent(B + 1, N), _isent(B + 1, N), _sentinel((B + 1, N), torch.float32)
    scd, hd, Ed, lsed = dev(be, sc0), dev(be, hn), dev(be, torch.cat([E, _sentinel((1, d), tt)])), dev(be, lse)
    seld, nrd, cd = dev(be, _i32(sel)), dev(be, _i32([len(s) for s in sels])), dev(be, cand)
    ird, itd = dev(be, _i32(t.item_rows)), dev(be, torch.from_numpy(t.item_tok))
    ood, oid, osd = dev(be, oo0), dev(be, oi0), dev(be, os0)

    def call():
        return be.lib.p5_op_cand_score(dtype, P(scd), P(hd), P(Ed), d, P(lsed), B, CQ, nchunk, P(seld), P(nrd), cap, P(cd), C, P(ird), P(itd),
                                       t.item_tok.shape[1], t.n_items, pl, P(ood), P(oid), P(osd), N, be.stream_ptr())

    _run(be, row, call, [("p5_cand_score_kernel<T>", NM[dtype]), ("p5_cand_order_kernel", "")])
    sc = scd.cpu()
    _tail_intact(f"{tag} scores", sc, B * C)
    sc = sc[:B * C].view(B, C)
    oo, oi, os_ = ood.cpu(), oid.cpu(), osd.cpu()
    assert bool((oo[B] == IS).all()) and bool((oi[B] == IS).all()) and _same_bits(os_[B], os0[B]), f"{tag}: written past the last user"
    h64, e64, l64 = hn.double(), E.double(), lse.double()
    ref = torch.full((B, C), -1.0e9, dtype=torch.float64)
    bound = torch.zeros(B, C, dtype=torch.float64)
    for b in range(B):
        pos = {pr: ru for ru, pr in enumerate(sels[b])}
        for j, c in enumerate(cand[b].tolist()):
            if not 0 <= c < t.n_items:
                continue
            n = int(t.item_len[c])
            gs = [((pos[int(r)] // CQ) * B + b) * CQ + pos[int(r)] % CQ for r in t.item_rows[c, :n]]
            toks = t.item_tok[c, 1:n + 1]
            hh, ee = h64[gs], e64[toks]
            lg = alpha * (hh * ee).sum(-1)
            e_l = GEMM_S * alpha * (hh.abs() * ee.abs()).sum(-1) + ELEM_R32 * lg.abs()
            term = lg - l64[gs]
            ref[b, j] = term.sum() / n
            bound[b, j] = ((e_l + 2 * ELEM_R32 * (lg.abs() + l64[gs].abs())).sum() + (n + 1) * ELEM_R32 * term.abs().sum()) / n
    live = ref > -1.0e8
    assert bool((sc[~live] == -1.0e9).all()), f"{tag}: an empty slot must score -1e9"
    worst = _elem_check(tag, sc[live], ref[live], bound[live]) if bool(live.any()) else 0.0
    # the order, exactly, on the scores the kernel stored: (score desc, item asc) over the live slots
    for b in range(B):
        slots = [j for j in range(C) if live[b, j]]
        ranked = sorted(slots, key=lambda j: (-float(sc[b, j]), int(cand[b, j]), j))
        L = min(N, len(ranked))
        want_i = [int(cand[b, j]) for j in ranked[:L]] + [-1] * (N - L)
        want_s = [float(sc[b, j]) for j in ranked[:L]] + [-1.0e9] * (N - L)
        assert oi[b].tolist() == want_i, f"{tag}: user {b}: out_index {oi[b].tolist()[:10]}, expected {want_i[:10]}"
        assert os_[b].tolist() == want_s, f"{tag}: user {b}: out_score differs"
        got_o = oo[b].tolist()
        assert all(x == -1 for x in got_o[L:]), f"{tag}: user {b}: out_order beyond the live slots"
        assert got_o[:L] == ranked[:L], f"{tag}: user {b}: out_order {got_o[:10]}, expected {ranked[:10]}"
        if row["ties"]:
            assert len({float(sc[b, j]) for j in slots}) <= pl, f"{tag}: user {b}: the inputs do not tie items of equal length"
    return worst


# ---- prune ------------------------------------------------------------------------------------------------------------------------------------------
def fill_case(be, row, seed=0):
    n, tag = row["n"], row["id"]
    buf = dev(be, _flat_guard(n, torch.float32))

    def call():
        return be.lib.p5_op_prune_fill(P(buf), n, -1.0e30, be.stream_ptr())

    _run(be, row, call, [("p5_prune_fill_kernel", "")])
    got = buf.cpu()
    _tail_intact(tag, got, n)
    assert bool((got[:n] == -1.0e30).all()), f"{tag}: {int((got[:n] != -1.0e30).sum())} elements not filled"
    return 0.0


def propose_case(be, row, seed=0):
    rows, B = row["rows"], row["B"]
    tag, N, slack = row["id"], 5, 0.25
    g = torch.Generator().manual_seed(seed + 101)
    t = random_trie(rows, g)
    lp = (-torch.rand(B, t.n_edges, generator=g) * 3.0).float()
    lmax = np.array(t.row_lmax, dtype=np.int32)
    if rows >= 255:          # an ancestor whose own test fails while its descendants' pass: a short lmax on one row of depth 1 with a subtree
        big = max((r for r in range(1, rows) if t.depth[r] == 1), key=lambda r: sum(1 for x in range(rows) if t.depth[x] > 1 and int(t.anc[x, 1]) == r))
        lmax[big] = 1
        lp[:, t.row_edge[big]] = -2.0
        inside = [x for x in range(rows) if t.depth[x] > 1 and int(t.anc[x, 1]) == big]
        for x in inside:
            lp[:, t.row_edge[x]] = -0.01
            lmax[x] = 40
    if rows >= 3:
        lp[2 % B, t.row_edge[rows // 2]] = float("nan")          # a NaN edge: the row and everything below it is dropped
    top = torch.zeros(B, N)
    for b in range(B):
        ub = sorted(float(_path_sum32(lp[b].numpy(), t, r) / F32(lmax[r])) for r in range(1, rows) if not np.isnan(_path_sum32(lp[b].numpy(), t, r)))
        top[b, N - 1] = (ub[len(ub) // 2] if ub else -1.0) + slack
        top[b, :N - 1] = top[b, N - 1] + 1.0
    top[B - 1] = -1.0e9          # fewer items than N: everything is kept
    if rows >= 255:
        top[0, N - 1] = -1.0 + slack          # thr = -1: the short-lmax row fails (-2 / 1), its subtree alone would pass (about -2.1 / 40)
    sel0, nr0, hdr0 = _isent(B + 1, rows), _isent(B + 4), _isent(8)
    seld, nrd, hdrd, lpd, topd = dev(be, sel0), dev(be, nr0), dev(be, hdr0), dev(be, lp), dev(be, top)
    depd, ancd, red, lmd = dev(be, _i32(t.depth)), dev(be, _i32(t.anc)), dev(be, _i32(t.row_edge)), dev(be, _i32(lmax))

    def call():
        return be.lib.p5_op_prune_propose(P(seld), P(nrd), P(hdrd), P(lpd), t.n_edges, P(topd), N, P(depd), P(ancd), rows, t.levels, P(red), P(lmd), slack,
                                          B, be.stream_ptr())

    _run(be, row, call, [("p5_prune_propose_kernel", ""), ("p5_cand_hdr_kernel", "")])
    sel, nr, hdr = seld.cpu(), nrd.cpu(), hdrd.cpu()
    _itail_intact(f"{tag} n_rows", nr, B)
    _itail_intact(f"{tag} hdr", hdr, 1)
    assert bool((sel[B] == IS).all()), f"{tag}: sel written past the last user"
    most, saw_closure_rule = 0, False
    for b in range(B):
        lpn = lp[b].numpy()
        thr = F32(top[b, N - 1].numpy() - F32(slack))
        own = [True] * rows
        for r in range(1, rows):
            own[r] = bool(F32(_path_sum32(lpn, t, r) / F32(lmax[r])) >= thr)
        want = [r for r in range(rows) if all(own[a] for a in t.chain(r))]
        saw_closure_rule |= any(own[r] and r not in set(want) for r in range(rows))
        got = sel[b, :int(nr[b])].tolist()
        assert got == want, f"{tag}: user {b}: {len(got)} rows {got[:12]}, expected {len(want)} rows {want[:12]}"
        assert bool((sel[b, len(want):] == IS).all()), f"{tag}: user {b}: sel written past its rows"
        keep = set(got)
        assert got == sorted(got) and all(int(a) in keep for r in got for a in t.anc[r, :t.depth[r]]), f"{tag}: user {b}: not ascending and ancestor-closed"
        most = max(most, len(want))
    assert int(nr[B - 1]) == rows, f"{tag}: a top score of -1e9 must keep every row"
    assert rows < 255 or saw_closure_rule, f"{tag}: the inputs hold no row that passes while an ancestor fails"
    assert int(hdr[0]) == most, f"{tag}: header {int(hdr[0])}, the largest row count is {most}"
    return 0.0


def mask_case(be, row, seed=0):
    n, pl, B = row["n_items"], row["path_len"], row["B"]
    tag = row["id"]
    g = torch.Generator().manual_seed(seed + 103)
    words, n_edges = (n + 31) // 32, 2 * n + 3
    lp = (-torch.rand(B, n_edges, generator=g) * 5.0).float()
    lp[torch.rand(B, n_edges, generator=g) < 0.15] = -1.0e30          # not scored
    lp[:, 1] = -1.0e29                                                # the sentinel test's own edge
    lp[:, 2] = -9.9e28
    ie = torch.randint(0, n_edges, (n, pl), generator=g).to(torch.int32)
    ln = torch.randint(1, pl + 1, (n,), generator=g)
    for i in range(n):
        ie[i, int(ln[i]):] = -1
    ex = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, words), generator=g).to(torch.int32) if row["excl"] else None
    out0 = _isent(B * words + 8)
    od, exd, lpd, ied = dev(be, out0), (dev(be, ex) if ex is not None else None), dev(be, lp), dev(be, ie)

    def call():
        return be.lib.p5_op_prune_mask(P(od), P(exd), P(lpd), n_edges, P(ied), n, pl, B, be.stream_ptr())

    _run(be, row, call, [("p5_prune_mask_kernel", "")])
    got = od.cpu()
    _itail_intact(tag, got, B * words)
    lpn, ien = lp.numpy(), ie.numpy()
    uns = lpn <= F32(-1.0e29)
    hit = np.zeros((B, words * 32), dtype=bool)
    for b in range(B):
        valid = ien >= 0
        hit[b, :n] = (uns[b][np.where(valid, ien, 0)] & valid).any(1)
    wgt = (2 ** np.arange(32, dtype=np.int64))
    want = (hit.reshape(B, words, 32) * wgt).sum(-1)
    if ex is not None:
        want |= ex.numpy().astype(np.int64) & 0xffffffff
    want = np.where(want >= 2 ** 31, want - 2 ** 32, want).astype(np.int32)
    assert np.array_equal(got[:B * words].view(B, words).numpy(), want), f"{tag}: bitmap differs"
    return 0.0


def _find(sel, n, row, lim):
    lo, hi = 0, min(n, lim) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if sel[mid] < row:
            lo = mid + 1
        else:
            hi = mid
    return lo


def _certify_ref(t, lmax, sel, n, lim, lp, out_index, out_score, N, margin, pc_branch=True):
    """p5_prune_certify_kernel restated; pc_branch False: what a kernel without the `Pc > 0` arm would answer (a condition on the inputs)"""
    flag = out_index[N - 1] < 0 or n > lim or n < 1
    tau = F32(out_score[N - 1])
    cut = F32(tau - F32(margin))
    for i in range(min(n, lim)):
        r = int(sel[i])
        dep = t.depth[r]
        if dep > 0:
            p = int(t.anc[r, dep - 1])
            flag |= int(sel[_find(sel, n, p, lim)]) != p
        else:
            flag |= r != 0
        Pv = _path_sum32(lp, t, r)
        nd = t.row_node[r]
        for e in range(t.child_off[nd], t.child_off[nd + 1]):
            l = lp[e]
            flag |= not (l <= F32(margin))
            c = t.edge_row[e]
            if c >= 0 and int(sel[_find(sel, n, c, lim)]) != c:
                Pc = F32(Pv + l)
                ub = Pc if (Pc > 0 and pc_branch) else F32(Pc / F32(lmax[c]))
                flag |= not (ub < cut)
    return int(bool(flag))


def certify_case(be, row, seed=0):
    near, tag = row["near"], row["id"]
    N, margin = 4, 1.0e-4
    CAUSES = ("clean", "frontier_at_cut", "pc_positive", "lp_above_margin", "lp_nan", "parent_missing", "short_list", "too_many_rows")
    B = len(CAUSES)
    g = torch.Generator().manual_seed(seed + 107)
    t = _trie_of_levels(5, g, width=60)
    lmax = np.array(t.row_lmax, dtype=np.int32)
    d1 = [r for r in range(t.rows) if t.depth[r] == 1]
    assert len(d1) >= 4
    front = d1[0]                                      # a frontier child of row 0 in every user
    lmax[front] = 2                                    # (its depth is 1: a kernel that divides by the depth is off by a factor of two)
    mid = next(r for r in d1[1:] if any(t.parents[x] == r for x in range(t.rows)))      # a row of depth 1 with a child row
    kid = next(x for x in range(t.rows) if t.parents[x] == mid)
    base = [r for r in t.closure([r for r in range(t.rows) if r % 5 == 0] + [kid]) if r != front and front not in t.anc[r, :t.depth[r]].tolist()]
    CQ, nchunk = 64, 2
    lim = CQ * nchunk
    assert len(base) + 1 <= lim
    cap = t.rows + 40
    sel = np.full((B, cap), 10 ** 6, dtype=np.int32)
    n_rows = []
    lp = np.zeros((B, t.n_edges), dtype=F32)
    out_index = np.tile(np.arange(N, dtype=np.int32), (B, 1))
    out_score = np.tile(np.array([-0.5, -0.7, -0.9, -1.0], dtype=F32), (B, 1))
    tau = F32(-1.0)
    cut = F32(tau - F32(margin))
    below = np.nextafter(cut, F32(-np.inf), dtype=F32)
    for b, cause in enumerate(CAUSES):
        mine = list(base)
        inset = set(mine)
        l = (-torch.rand(t.n_edges, generator=g) * 0.3 - 0.01).numpy().astype(F32)
        for e in range(t.n_edges):          # every frontier edge far out of reach
            c = t.edge_row[e]
            if c >= 0 and c not in inset:
                l[e] = F32(-60.0)
        l[t.row_edge[mid]] = F32(-60.0)     # (so that `mid` left out of sel is no frontier finding)
        inner_edge = t.row_edge[kid]        # an edge between two sel rows
        l[t.row_edge[front]] = F32(2.0) * below          # ub = lp / 2 = the largest value below the cut: clean
        if cause == "frontier_at_cut":
            l[t.row_edge[front]] = F32(2.0) * (below if near else cut)
        elif cause == "pc_positive":
            # Pc = lp > 0 is its own bound.  This user's N-th score is 1.4e-4, so the cut (about 4e-5) lies between Pc / row_lmax = 2.5e-5 and Pc =
            # 5e-5: only the `Pc > 0` arm flags.  lp stays below margin, so the lp test is silent.  near: Pc the largest value below the cut
            out_score[b] = F32(1.4e-4)
            cut_pc = F32(F32(1.4e-4) - F32(margin))
            pc = np.nextafter(cut_pc, F32(-np.inf), dtype=F32) if near else F32(5.0e-5)
            assert F32(pc / F32(2.0)) < cut_pc and (pc < cut_pc) == near and F32(0.0) < pc <= F32(margin)
            l[t.row_edge[front]] = pc
        elif cause == "lp_above_margin":
            l[inner_edge] = F32(margin) if near else np.nextafter(F32(margin), F32(1.0), dtype=F32)
        elif cause == "lp_nan":
            l[inner_edge] = F32(-0.0) if near else F32(np.nan)
        elif cause == "parent_missing":
            if not near:
                mine.remove(mid)
        elif cause == "short_list":
            out_index[b, N - 1] = 0 if near else -1
        elif cause == "too_many_rows":      # n = lim (near) / lim + 1
            extra = [r for r in range(t.rows) if r not in inset and r != front and front not in t.anc[r, :t.depth[r]].tolist()]
            mine = t.closure(mine + extra)
            mine = [r for r in mine if r != front]
            assert len(mine) >= lim + 1, (len(mine), lim)
            mine = mine[:lim if near else lim + 1]          # (ascending level order: a prefix of a closed set is closed)
            inset = set(mine)
            for e in range(t.n_edges):
                c = t.edge_row[e]
                if c >= 0:
                    l[e] = F32(-60.0) if c not in inset else (l[e] if l[e] > -50 else F32(-0.1))
            l[t.row_edge[front]] = F32(2.0) * below
        lp[b] = l
        sel[b, :len(mine)] = mine
        n_rows.append(len(mine))
    fl0 = torch.zeros(B + 4, dtype=torch.int32)
    fl0[B:] = IS
    fld, lpd = dev(be, fl0), dev(be, torch.from_numpy(lp))
    depd, rnd, ancd = dev(be, _i32(t.depth)), dev(be, _i32(t.row_node)), dev(be, _i32(t.anc))
    seld, nrd = dev(be, _i32(sel)), dev(be, _i32(n_rows))
    red, erd, lmd, cod = dev(be, _i32(t.row_edge)), dev(be, _i32(t.edge_row)), dev(be, _i32(lmax)), dev(be, _i32(t.child_off))
    oid, osd = dev(be, _i32(out_index)), dev(be, torch.from_numpy(out_score))

    def call():
        return be.lib.p5_op_prune_certify(P(fld), P(lpd), t.n_edges, P(depd), P(rnd), P(ancd), t.levels, B, CQ, nchunk, P(seld), P(nrd), cap, P(red), P(erd),
                                          P(lmd), P(cod), P(oid), P(osd), N, margin, be.stream_ptr())

    _run(be, row, call, [("p5_prune_certify_kernel", "")])
    fl = fld.cpu()
    _itail_intact(f"{tag} flagged", fl, B)
    want = [_certify_ref(t, lmax, sel[b], n_rows[b], lim, lp[b], out_index[b], out_score[b], N, margin) for b in range(B)]
    expect = [0] * B if near else [0] + [1] * (B - 1)
    assert want == expect, f"{tag}: the inputs do not present each cause alone: the restatement flags {dict(zip(CAUSES, want))}"
    b = CAUSES.index("pc_positive")
    assert _certify_ref(t, lmax, sel[b], n_rows[b], lim, lp[b], out_index[b], out_score[b], N, margin, pc_branch=False) == 0, \
        f"{tag}: the pc_positive user would be flagged without the Pc > 0 arm too"
    assert fl[:B].tolist() == want, f"{tag}: flags {dict(zip(CAUSES, fl[:B].tolist()))}, expected {dict(zip(CAUSES, want))}"
    return 0.0


# ---- bound ------------------------------------------------------------------------------------------------------------------------------------------
def seed_case(be, row, seed=0):
    S, T, B = row["S"], row["T"], row["B"]
    tag = row["id"]
    g = torch.Generator().manual_seed(seed + 109)
    t = _trie_of_levels(4, g, width=12)
    md = t.levels - 1 if row["short_depth"] else t.levels
    T = T or t.path_len + 2
    seeds = torch.zeros(B, S, T, dtype=torch.int64)
    for b in range(B):
        for j in range(S):
            k = int(torch.randint(0, 6, (1,), generator=g))
            it = int(torch.randint(0, t.n_items, (1,), generator=g)) if j > 1 else int((np.argmax, np.argmin)[j](t.item_len))
            seq = t.item_tok[it, :int(t.item_len[it]) + 1].tolist()
            if j < 2:
                pass                                # the longest and the shortest item, as they are
            elif k == 0 and len(seq) > 2:
                seq = seq[:-1]                      # stops on an inner node
            elif k == 1:
                seq[len(seq) // 2] = 4999           # leaves the trie (no child has this token)
            elif k == 2:
                seq[0] = 7                          # does not begin with the start token
            elif k == 3:
                seq = seeds[b, j - 1].tolist()      # a duplicate
            seq = (seq + [0] * T)[:T]
            seeds[b, j] = torch.tensor(seq)
    if B > 1:
        seeds[B - 1] = 4999                          # a user without a usable seed: row 0 alone
    cap = t.rows
    KP = 256
    while KP < S * md + 1:
        KP <<= 1
    if row.get("error"):
        KP >>= 1          # too few key slots for the seeds: the entry must refuse
    sel0, nr0, hdr0 = _isent(B + 1, cap), _isent(B + 4), _isent(8)
    keys0 = torch.full((B * KP + 16,), IS, dtype=torch.int64)
    seld, nrd, hdrd, keyd, sd = dev(be, sel0), dev(be, nr0), dev(be, hdr0), dev(be, keys0), dev(be, seeds)
    cod, ctd, erd, rtd, rnd = dev(be, _i32(t.child_off)), dev(be, _i32(t.child_tok)), dev(be, _i32(t.edge_row)), dev(be, _i32(t.row_tok)), dev(be, _i32(t.row_node))

    def call():
        return be.lib.p5_op_bound_seed(P(seld), P(nrd), P(hdrd), P(keyd), KP, cap, P(sd), S, T, P(cod), P(ctd), P(erd), P(rtd), P(rnd), md, B, be.stream_ptr())

    if row.get("error"):
        rc = call()
        assert rc != 0 and b"bound_seed" in be.lib.p5_last_error(), f"{tag}: the entry accepted it (rc {rc}, {be.lib.p5_last_error()})"
        sync(be)
        assert bool((seld.cpu() == IS).all()) and bool((nrd.cpu() == IS).all()) and bool((hdrd.cpu() == IS).all()) and bool((keyd.cpu() == IS).all()), \
            f"{tag}: written although the call was refused"
        return 0.0
    _run(be, row, call, [("p5_bound_seed_kernel", ""), ("p5_bound_union_kernel", ""), ("p5_bound_hdr_kernel", "")])
    sel, nr, hdr = seld.cpu(), nrd.cpu(), hdrd.cpu()
    assert bool((keyd.cpu()[B * KP:] == IS).all()), f"{tag}: written past the sort keys"
    _itail_intact(f"{tag} n_rows", nr, B)
    _itail_intact(f"{tag} hdr", hdr, 2)
    assert bool((sel[B] == IS).all()), f"{tag}: sel written past the last user"
    most, used = 0, 0
    for b in range(B):
        want = {0}
        for j in range(S):
            q = seeds[b, j].tolist()
            rows_, node, ok, leaf = [], t.row_node[0], T >= 2 and q[0] == t.row_tok[0], False
            k = 1
            while ok and not leaf and k < T:
                e = next((c for c in range(t.child_off[node], t.child_off[node + 1]) if t.child_tok[c] == q[k]), -1)
                if e < 0:
                    ok = False
                    break
                r = t.edge_row[e]
                if r < 0:
                    leaf = True
                elif len(rows_) < md:
                    rows_.append(r)
                    node = t.row_node[r]
                else:
                    ok = False
                k += 1
            if ok and leaf:
                want.update(rows_)
                used += 1
        want = sorted(want)
        assert int(nr[b]) == len(want) and sel[b, :len(want)].tolist() == want, f"{tag}: user {b}: sel {sel[b, :max(int(nr[b]), 0)].tolist()[:12]}, expected {want[:12]}"
        assert bool((sel[b, len(want):] == IS).all()), f"{tag}: user {b}: sel written past its rows"
        most = max(most, len(want))
    assert hdr[:2].tolist() == [most, 0], f"{tag}: header {hdr[:2].tolist()}, expected {[most, 0]}"
    assert T < 2 or S < 5 or used > 0, f"{tag}: no seed of the inputs is an item"
    return 0.0


def expand_case(be, row, seed=0):
    kind, B = row["kind"], row["B"]
    tag, N, margin = row["id"], 3, 1.0e-4
    g = torch.Generator().manual_seed(seed + 113)
    if kind == "wide":          # row 0 has 1000 child rows
        parents = [-1] + [0] * 1000 + [1 + i // 2 for i in range(200)]
        has_kid = set(parents[1:])
        t = Trie(parents, [0 if r in has_kid else 1 for r in range(len(parents))], 5000, g)
    elif kind == "pc_positive":          # row 0 has 30 child rows
        t = _trie_of_levels(3, g, width=30)
    elif kind in ("cross256", "cross512", "beyond_kp"):          # 300 rows on each of two levels: a prefix of the level order has a wide frontier
        t = _trie_of_levels(3, g, width=300)
    else:
        t = random_trie(420, g, step=0.3)
    lmax = np.array(t.row_lmax, dtype=np.int32)
    KP = 256
    while KP < t.rows:
        KP <<= 1
    if kind == "beyond_kp":
        KP = 256
    cap = t.rows
    CQ, nchunk = (t.rows + 1 + 15) // 16 * 16 // 2 // 16 * 16 + 16, 2
    lim = CQ * nchunk
    assert lim >= t.rows
    n_old = {"cross256": 200, "cross512": 380, "beyond_kp": 230, "empty": 0, "wide": 1}.get(kind, 120)
    # past n_rows sel holds what an earlier, larger plan left there: the very rows of the frontier (a search that looks one entry too far finds them)
    sel = np.tile(np.arange(cap, dtype=np.int32), (B, 1))
    n_rows, lp = [], (-torch.rand(B, t.n_edges, generator=g) * 2.0 - 0.05).numpy().astype(F32)
    pc_want = {}
    out_score = np.tile(np.array([-0.2, -0.4, -0.6], dtype=F32), (B, 1))
    for b in range(B):
        mine = list(range(min(n_old + 7 * b, t.rows))) if n_old else []          # a prefix of the level order is ancestor-closed
        if b == B - 1 and kind not in ("empty", "wide"):
            mine = [0]
        sel[b, :len(mine)] = mine
        n_rows.append(len(mine))
        if kind == "none":
            out_score[b, N - 1] = F32(3.0e38)
        if kind == "pc_positive":
            # sel = row 0 alone, P(0) = 0; the N-th score 1.4e-4 puts the cut (about 4e-5) between Pc / row_lmax and Pc of a child edge with lp = 5e-5 (a
            # child row has row_lmax >= 2): such a row is admitted through the `Pc > 0` arm alone; lp just below the cut or negative: not admitted
            mine = [0]
            sel[b, 0], n_rows[b] = 0, 1
            out_score[b] = F32(1.4e-4)
            cut_pc = F32(F32(1.4e-4) - F32(margin))
            nd = t.row_node[0]
            kids = [e for e in range(t.child_off[nd], t.child_off[nd + 1]) if t.edge_row[e] >= 0]
            assert len(kids) >= 3
            for j, e in enumerate(kids):
                lp[b, e] = (F32(5.0e-5), np.nextafter(cut_pc, F32(-np.inf), dtype=F32), F32(-1.0))[j % 3]
                assert lmax[t.edge_row[e]] >= 2
            pc_want[b] = sorted([0] + [t.edge_row[e] for j, e in enumerate(kids) if j % 3 == 0])
        if kind in ("wide", "cross256", "cross512", "beyond_kp") and b == 0:
            out_score[b, N - 1] = F32(-3.0e38)         # the whole frontier is within reach
        if kind == "nan" and mine:
            out_score[b, N - 1] = F32(3.0e38)          # nothing but the NaN edges is within reach
            inset = set(mine)
            fr = [e for e in range(t.n_edges) if t.edge_row[e] >= 0 and t.edge_row[e] not in inset and t.parents[t.edge_row[e]] in inset]
            for e in fr[::3]:
                lp[b, e] = np.nan
    sel0 = torch.from_numpy(sel.copy())
    nr0 = torch.cat([_i32(n_rows), _isent(4)])
    gr0, hdr0 = _isent(B + 4), _isent(8)
    keys0 = torch.full((B * KP + 16,), IS, dtype=torch.int64)
    seld, nrd, grd, hdrd, keyd, lpd = dev(be, sel0), dev(be, nr0), dev(be, gr0), dev(be, hdr0), dev(be, keys0), dev(be, torch.from_numpy(lp))
    depd, rnd, ancd = dev(be, _i32(t.depth)), dev(be, _i32(t.row_node)), dev(be, _i32(t.anc))
    red, erd, lmd, cod, osd = dev(be, _i32(t.row_edge)), dev(be, _i32(t.edge_row)), dev(be, _i32(lmax)), dev(be, _i32(t.child_off)), dev(be, torch.from_numpy(out_score))

    def call():
        return be.lib.p5_op_bound_expand(P(seld), P(nrd), P(grd), P(hdrd), P(keyd), KP, P(lpd), t.n_edges, P(depd), P(rnd), P(ancd), t.levels, B, CQ, nchunk, cap,
                                         P(red), P(erd), P(lmd), P(cod), P(osd), N, margin, be.stream_ptr())

    _run(be, row, call, [("p5_bound_expand_kernel", ""), ("p5_bound_hdr_kernel", "")])
    got_sel, nr, gr, hdr = seld.cpu(), nrd.cpu(), grd.cpu(), hdrd.cpu()
    assert bool((keyd.cpu()[B * KP:] == IS).all()), f"{tag}: written past the sort keys"
    _itail_intact(f"{tag} n_rows", nr, B)
    _itail_intact(f"{tag} grew", gr, B)
    _itail_intact(f"{tag} hdr", hdr, 2)
    most, grown, admitted_all = 0, 0, 0
    for b in range(B):
        n = max(min(n_rows[b], lim, cap, KP), 0)
        old = sel[b, :n].tolist()
        inset = set(old)
        cut = F32(out_score[b, N - 1] - F32(margin))
        keys = list(old)
        for r in old:
            Pv = _path_sum32(lp[b], t, r)
            nd = t.row_node[r]
            for e in range(t.child_off[nd], t.child_off[nd + 1]):
                c = t.edge_row[e]
                if c < 0 or c in inset:
                    continue
                Pc = F32(Pv + lp[b, e])
                ub = Pc if Pc > 0 else F32(Pc / F32(lmax[c]))
                if not (ub < cut):
                    keys.append(c)
        admitted_all += len(keys) - n
        want = sorted(set(keys[:KP]))[:cap]
        m = len(want)
        assert kind != "pc_positive" or (want == pc_want[b] and m > n), f"{tag}: the inputs do not admit exactly the rows with 0 < Pc / row_lmax < cut <= Pc"
        assert int(nr[b]) == m and got_sel[b, :m].tolist() == want, f"{tag}: user {b}: {int(nr[b])} rows {got_sel[b, :12].tolist()}, expected {m} rows {want[:12]}"
        assert torch.equal(got_sel[b, m:], sel0[b, m:]), f"{tag}: user {b}: sel changed past its rows"
        assert int(gr[b]) == int(m > n), f"{tag}: user {b}: grew {int(gr[b])}, expected {int(m > n)}"
        most, grown = max(most, m), grown + int(m > n)
        if kind == "cross256":
            assert b != 0 or n <= 256 < len(keys), (n, len(keys))
        if kind == "cross512":
            assert b != 0 or n <= 512 < len(keys), (n, len(keys))
        if kind == "beyond_kp":
            assert b != 0 or len(keys) > KP, (n, len(keys))
        if kind == "wide":
            assert b != 0 or len(keys) - n >= 900, (n, len(keys))
    assert hdr[:2].tolist() == [most, grown], f"{tag}: header {hdr[:2].tolist()}, expected {[most, grown]}"
    assert kind not in ("none", "empty") or grown == 0
    assert kind != "nan" or admitted_all > 0
    return 0.0


CASES = dict(edges=edges_case, row_lse=row_lse_case, items=items_case, select=select_case, tree_attn=tree_attn_case, cand_plan=cand_plan_case,
             cand_rows=cand_rows_case, cand_score=cand_score_case, fill=fill_case, propose=propose_case, mask=mask_case, certify=certify_case, seed=seed_case,
             expand=expand_case)


def rank_ref_case(be, row, seed=0):
    """one row of tests/rank_matrix.py; returns the worst err / bound (0 for the exact families)"""
    return CASES[row["fam"]](be, row, seed)
