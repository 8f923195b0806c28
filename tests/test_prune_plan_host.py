"""not-gpu, host only: `CompiledTrie.prune_plan` (what certified pruned ranking, csrc/p5_prune.h, adds to the rank plan) against brute
force over `enumerate_items()`."""
import numpy as np
import pytest

from openp5_amd.trie import CompiledTrie
from tests import cases, rank_cases


def _brute(ct, start=0):
    items = ct.enumerate_items()
    plan = ct.rank_plan(start)
    rows = plan["rows"]
    prefix_row = {}
    for r in range(rows):            # the prefix of a row: walk its ancestors' decoder input tokens
        d = int(plan["row_depth"][r])
        toks = [int(plan["row_tok"][int(plan["row_anc"][r, t])]) for t in range(d)] + [int(plan["row_tok"][r])]
        prefix_row[tuple(toks)] = r
    assert len(prefix_row) == rows
    edge_of = {}
    for n in range(ct.n_nodes):
        for e in range(int(ct.child_off[n]), int(ct.child_off[n + 1])):
            edge_of[(n, int(ct.child_tok[e]))] = e
    lmax = np.zeros(rows, dtype=np.int64)
    row_edge = np.full(rows, -1, dtype=np.int64)
    edge_row = np.full(len(ct.child_tok), -1, dtype=np.int64)
    for q in items:
        if q[0] != start:
            continue
        n_tok = len(q) - 1           # what p5_rank_items_kernel divides by: the tokens behind the decoder start
        node = 0
        for t in range(len(q)):
            e = edge_of[(node, q[t])]
            node = int(ct.child_node[e])
            r = prefix_row.get(tuple(q[:t + 1]), -1)
            if r >= 0:
                lmax[r] = max(lmax[r], n_tok)
                if t > 0:
                    row_edge[r] = e
                    edge_row[e] = r
    return lmax, row_edge, edge_row


@pytest.mark.parametrize("items", [cases.make_items(300, 5, hi=60), cases.make_items(30, 11, hi=60, minlen=1, maxlen=6), rank_cases.fanout_items(250),
                                   [[0, 1]], [[0, 7, 1], [0, 7, 8, 9, 1], [0, 9, 1], [3, 4, 1]]], ids=["300", "unequal", "fanout", "one", "other-start"])
def test_prune_plan_equals_brute_force(items):
    ct = CompiledTrie.from_sequences(items)
    pp = ct.prune_plan(0)
    lmax, row_edge, edge_row = _brute(ct)
    rows = ct.rank_plan(0)["rows"]
    assert pp["row_lmax"].dtype == pp["row_edge"].dtype == pp["edge_row"].dtype == np.int32
    assert pp["row_lmax"].shape == (rows,) and pp["row_edge"].shape == (rows,) and pp["edge_row"].shape == (len(ct.child_tok),)
    assert pp["row_lmax"].tolist() == lmax.tolist()
    assert pp["row_edge"].tolist() == row_edge.tolist() and int(pp["row_edge"][0]) == -1
    # (the edge of the start token itself leads to row 0: it is behind no scored row, both answers are accepted for it)
    start_edge = [e for e in range(int(ct.child_off[0]), int(ct.child_off[1])) if int(ct.child_tok[e]) == 0][0]
    got = pp["edge_row"].copy()
    assert int(got[start_edge]) in (0, -1)
    got[start_edge] = -1
    assert got.tolist() == edge_row.tolist()
    assert ct.prune_plan(0) is pp            # cached
    # Lmax and P only fall with depth: the bound of p5_prune.h is monotone along every path
    plan = ct.rank_plan(0)
    for r in range(1, rows):
        assert pp["row_lmax"][r] <= pp["row_lmax"][plan["row_parent"][r]] and pp["row_lmax"][r] >= plan["row_depth"][r] + 1
