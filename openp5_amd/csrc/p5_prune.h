// p5_prune.h -- certified exhaustive ranking: the bf16 pass over the whole trie PROPOSES which prefixes are worth fp32 numbers, an fp32
// pass over those prefixes alone DECIDES the top N, and a certificate proves that no item outside them could have entered the list.
//
// p5_rank.h gives a bf16 model two prices: the bf16 pass (lists that can differ at near-ties) or the whole pass again in fp32.  Here the
// fp32 pass runs over an ancestor-closed subset of the trie's plan rows per user -- the layout p5_cand.h already runs the decoder over
// (P5CandPlan::sel) -- so its cost follows the number of prefixes whose probability is within reach of the N-th item, not the catalogue.
//   PROPOSE  (bf16 engine, right after the unchanged p5_rank.h pass, on its edge_lp and its selected scores) p5_prune_propose_kernel: tau16
//            = the N-th best bf16 score of the user's non-excluded items; P16(r) = the edge log-probabilities on the path to row r summed in
//            depth order; row r is kept iff P16(a) / row_lmax[a] >= tau16 - slack for r AND every ancestor a of r (the test is monotone in
//            exact arithmetic -- P only falls with depth, row_lmax only falls with depth -- and taking it along the path makes the kept set
//            closed under "ancestor of" whatever the rounding).  Kept rows are compacted in ascending order by a block prefix scan over the
//            row index: sel[b][0 .. n_b), the header word = the largest n_b (p5_cand_hdr_kernel).  No atomics, the same bits every call.
//   DECIDE   (fp32 engine) the decoder over sel (p5_cand.h's rows / tree attention, the range guard), the fp32 log-probability of every
//            child edge of every sel row (p5_rank_score*_kernel fed the global row through sel; every other edge keeps a sentinel),
//            p5_prune_mask_kernel (an item with a sentinel edge joins the user's exclusion bitmap), then p5_rank.h's ITEMS and SELECT.
//   CERTIFY  p5_prune_certify_kernel, below.
//
// SOUNDNESS.  An item's score is s(i) = (lp(e_1) + ... + lp(e_n)) / n, the edges of its path in depth order, n its token count.  Let r be
// a sel row, e a child edge of r into a row c that is NOT in sel, P(c) = P(r) + lp(e), and i any item below c with n tokens.  The
// certificate has checked that every computed log-probability is <= margin, so s(i) <= (P(c) + (n - depth(c)) * margin) / n <= P(c) / n
// + margin.  n <= row_lmax[c], so for P(c) <= 0: P(c) / n <= P(c) / row_lmax[c] = UB(c); for P(c) > 0 (rounding residue only) P(c) / n
// <= P(c) = UB(c).  The kernel requires UB(c) < tau32 - margin, tau32 the N-th returned fp32 score: then s(i) < tau32 for every item
// below c.  sel is closed under "ancestor of" (the kernel checks that too: a row whose parent is missing flags the user), so an item is
// either scored in full -- all its prefixes in sel -- or lies below exactly one such frontier row c.  Hence every item that was not scored
// ranks below the N returned ones, and the returned list is the fp32 top N.  UB is formed with the division the item score uses (fp32
// divide of the depth-ordered fp32 sum by the count), so the two roundings are monotone in the same way.
// CAVEAT.  "the fp32 score" of an item that was not scored is the number the full fp32 pass WOULD give it.  A row of the decoder pass
// depends on its ancestors only, but the GEMM route (and with it the order of a dot product's partial sums) can depend on how many rows a
// pass has, and log p = logit - lse can carry a positive rounding residue.  Both are absorbed by `margin` (default 1e-4: the tolerance the
// project holds fp32 scores to at T5-small width) -- the certificate is exact up to that margin, and slack decides nothing: it changes how
// many rows are scored and how often the certificate fails, never a returned list.
// A user is FLAGGED (and re-run by the host through the full fp32 pass, never returned as is) when a frontier row's bound reaches
// tau32 - margin, when fewer than N items were returned, when a computed log-probability exceeds +margin or is not a number, when a sel
// row's parent is missing, or when the range guard of the split-product pass fired.
#pragma once
#include "p5_cand.h"

#define P5_PRUNE_SENTINEL (-1.0e30f)        // edge_lp of an edge whose parent row was not scored
#define P5_PRUNE_UNSCORED(x) ((x) <= -1.0e29f)

__global__ __launch_bounds__(256) void p5_prune_fill_kernel(float* __restrict__ p, size_t n, float v) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}

// ---- PROPOSE: one workgroup per user over the rows in 256-row steps.  top_score: [B][N] the bf16 pass's selected scores (-1e9 beyond the
// user's items: then every row is kept).  sel: [B][pl.rows].  pl: the trie's plan (rows, row_depth, anc, max_depth) ----
__global__ __launch_bounds__(256) void p5_prune_propose_kernel(int* __restrict__ sel, int* __restrict__ n_rows, const float* __restrict__ edge_lp,
                                                              long long n_edges, const float* __restrict__ top_score, int N, P5RankPlan pl,
                                                              const int* __restrict__ row_edge, const int* __restrict__ row_lmax, float slack) {
  __shared__ int s_w[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ lp = edge_lp + (size_t)b * n_edges;
  const float thr = top_score[(size_t)b * N + N - 1] - slack;
  int* __restrict__ out = sel + (size_t)b * pl.rows;
  int base = 0;
  for (int r0 = 0; r0 < pl.rows; r0 += 256) {
    const int r = r0 + tid;
    int keep = 0;
    if (r < pl.rows) {
      keep = 1;                                  // (row 0, the start prefix, is always kept)
      const int dep = pl.row_depth[r];
      const int* __restrict__ anc = pl.anc + (size_t)r * pl.max_depth;
      float P = 0.f;
      for (int t = 1; t <= dep; ++t) {
        const int a = t < dep ? anc[t] : r;
        P += lp[row_edge[a]];
        if (!(P / (float)row_lmax[a] >= thr)) keep = 0;
      }
    }
    int total;
    const int pos = p5_block_excl_scan(keep, s_w, total);
    if (keep) out[base + pos] = r;
    base += total;
  }
  if (tid == 0) n_rows[b] = base;
}

// ---- DECIDE: the exclusion bitmap of the selection = the user's own | items with an edge that has no fp32 number.  One thread per
// 32-item word: grid (ceil(words / 256), B) ----
__global__ __launch_bounds__(256) void p5_prune_mask_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ excluded, int words,
                                                           const float* __restrict__ edge_lp, long long n_edges, const int* __restrict__ item_edges,
                                                           int n_items, int path_len) {
  const int w = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (w >= words) return;
  const float* __restrict__ lp = edge_lp + (size_t)b * n_edges;
  uint32_t m = excluded ? excluded[(size_t)b * words + w] : 0u;
  for (int k = 0; k < 32; ++k) {
    const int i = w * 32 + k;
    if (i >= n_items) break;
    const int* __restrict__ pe = item_edges + (size_t)i * path_len;
    for (int n = 0; n < path_len; ++n) {
      const int e = pe[n];
      if (e < 0) break;
      if (P5_PRUNE_UNSCORED(lp[e])) { m |= 1u << k; break; }
    }
  }
  out[(size_t)b * words + w] = m;
}

// ---- CERTIFY: one thread per (user, sel row): grid (ceil(rows of the pass / 256), B).  pl.g: the trie's plan (row_depth, row_node, anc
// name GLOBAL rows) + the layout of the pass.  out_index / out_score: [B][N] the selection over the scored items.  flagged[b] = 1 unless
// the returned top N is proven complete (every writer stores the same value) ----
__global__ __launch_bounds__(256) void p5_prune_certify_kernel(int* __restrict__ flagged, const float* __restrict__ edge_lp, long long n_edges,
                                                              P5CandPlan pl, const int* __restrict__ row_edge, const int* __restrict__ edge_row,
                                                              const int* __restrict__ row_lmax, const int* __restrict__ child_off,
                                                              const int* __restrict__ out_index, const float* __restrict__ out_score, int N,
                                                              float margin) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int n = pl.n_rows[b], lim = pl.g.CQ * pl.g.nchunk;
  if (i == 0 && (out_index[(size_t)b * N + N - 1] < 0 || n > lim || n < 1)) flagged[b] = 1;        // fewer than N items (or a plan the pass does not hold)
  if (i >= n || i >= lim) return;
  const int* __restrict__ sel = pl.sel + (size_t)b * pl.cap;
  const float* __restrict__ lp = edge_lp + (size_t)b * n_edges;
  const float tau = out_score[(size_t)b * N + N - 1];
  const int r = sel[i];
  const int dep = pl.g.row_depth[r];
  const int* __restrict__ anc = pl.g.anc + (size_t)r * pl.g.max_depth;
  bool bad = false;
  if (dep > 0) {                                   // closed under "ancestor of": the parent is a sel row (then, by induction, every ancestor)
    const int p = anc[dep - 1];
    bad = sel[p5_cand_find(sel, n, p, lim)] != p;
  } else {
    bad = r != 0;
  }
  float P = 0.f;                                   // P32(r), summed as the item score sums it
  for (int t = 1; t <= dep; ++t) P += lp[row_edge[t < dep ? anc[t] : r]];
  const int nd = pl.g.row_node[r];
  for (int e = child_off[nd]; e < child_off[nd + 1]; ++e) {
    const float l = lp[e];
    bad |= !(l <= margin);                         // (a NaN fails too)
    const int c = edge_row[e];
    if (c >= 0 && sel[p5_cand_find(sel, n, c, lim)] != c) {
      const float Pc = P + l;
      const float ub = Pc > 0.f ? Pc : Pc / (float)row_lmax[c];
      bad |= !(ub < tau - margin);
    }
  }
  if (bad) flagged[b] = 1;
}
