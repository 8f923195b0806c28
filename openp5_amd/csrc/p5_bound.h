// p5_bound.h -- bounded trie search: the exact fp32 top N without a pass over the whole trie, in bf16 or fp32.
//
// p5_prune.h decides the top N on an ancestor-closed set of plan rows per user and certifies it, but the set comes from a bf16 pass over
// EVERY prefix.  Here the set is grown instead: start from the prefixes of a few good items (the seeds: the model's own beam search, or
// items the caller names), and let every round add exactly the frontier rows the certificate could not rule out.
//   BEGIN   (once per chunk of users, after the encoder + the cross-attention K/V) p5_bound_seed_kernel: one thread per (user, seed) walks
//           child_off / child_tok from the start node along the seed's tokens and notes the plan row behind every edge (edge_row) as a sort
//           key; a sequence that leaves the trie or does not end on a leaf notes nothing.  p5_bound_union_kernel: the keys of a user plus
//           row 0, sorted and made distinct as p5_cand_plan_kernel does it: sel[b][0 .. n_b) ascending.
//   ROUND   the DECIDE + CERTIFY of p5_prune.h over sel, unchanged, then p5_bound_expand_kernel: for every sel row r and every child edge e
//           of r into a row c that is NOT in sel, UB(c) = (P(r) + lp(e)) / row_lmax[c] as the certificate forms it, tau = the N-th score
//           of the round; c is admitted iff NOT UB(c) < tau - margin -- the complement of the certificate's test, so a NaN is admitted.  The
//           new sel is the sorted union of the old one and the admitted rows; grew[b] says whether it differs.
//           p5_bound_hdr_kernel: word 0 = the largest n_b, word 1 = the number of users that grew: the two integers the host reads.
//   STOP    when no user grew.  "Nothing admitted" is the certificate's frontier condition, evaluated in the same round on the same numbers:
//           the SOUNDNESS text of p5_prune.h applies as it stands, and out_flagged of that round says which users hold a certificate.
// tau never falls while the scored set grows, so a row admitted in round k + 1 is the child of a row admitted in round k: new rows get
// strictly deeper and the search ends within max_depth + 1 rounds.  Seeds change cost and the fallback share, never a returned list.
// Integer sort keys, block prefix scans, plain stores in a fixed order: no atomics, the same bits every call.  Neither kernel loops over
// the plan's rows or the items: the work follows sel and the children of its rows.
#pragma once
#include "p5_prune.h"

// sort key of plan row r: ~r, so the descending sort yields ascending rows; 0 = no row (sorted last), as p5_cand_plan_kernel
__device__ static __forceinline__ unsigned long long p5_bound_key(int r) { return (unsigned long long)(~(unsigned)r); }

// k[0 .. P) (P a multiple of 256, a power of two; the block synchronised before) sorted, its distinct rows ascending into out[0 .. cap):
// returns their number (uniform over the workgroup)
__device__ static int p5_bound_union(unsigned long long* k, int P, int* __restrict__ out, int cap, int* s_w) {
  const int tid = threadIdx.x;
  p5_wide_sort_desc(k, P);
  int base = 0;
  for (int i0 = 0; i0 < P; i0 += 256) {
    if (k[i0] == 0ull) break;                    // (uniform: the empty keys are sorted last)
    const int i = i0 + tid;
    const unsigned long long key = k[i];
    const int first = (key != 0ull && (i == 0 || k[i - 1] != key)) ? 1 : 0;
    int total;
    const int pos = p5_block_excl_scan(first, s_w, total);
    if (first && base + pos < cap) out[base + pos] = (int)(~(unsigned)(key & 0xffffffffull));
    base += total;
  }
  return base < cap ? base : cap;
}

// ---- BEGIN: grid (ceil(S / 256), B).  seeds: int64 [B][S][T], token 0 of a sequence = the decoder start (row_tok[0]).  keys: [B][KP];
// user b's slots: max_depth per seed, then row 0, then empty up to P (a power of two >= S * max_depth + 1, <= KP) ----
__global__ __launch_bounds__(256) void p5_bound_seed_kernel(unsigned long long* __restrict__ keys, int KP, int P, const int64_t* __restrict__ seeds, int S, int T,
                                                           const int* __restrict__ child_off, const int* __restrict__ child_tok,
                                                           const int* __restrict__ edge_row, const int* __restrict__ row_tok,
                                                           const int* __restrict__ row_node, int max_depth) {
  const int tid = threadIdx.x, j = blockIdx.x * 256 + tid, b = blockIdx.y;
  unsigned long long* k = keys + (size_t)b * KP;
  const int used = S * max_depth;
  if (blockIdx.x == 0)
    for (int i = used + tid; i < P; i += 256) k[i] = i == used ? p5_bound_key(0) : 0ull;
  if (j >= S) return;
  const int64_t* __restrict__ q = seeds + ((size_t)b * S + j) * T;
  unsigned long long* out = k + (size_t)j * max_depth;
  int n = 0, node = row_node[0];
  bool ok = T >= 2 && q[0] == (int64_t)row_tok[0], leaf = false;
  for (int t = 1; ok && !leaf && t < T; ++t) {
    const int64_t tk = q[t];
    int e = -1;
    for (int c = child_off[node]; c < child_off[node + 1]; ++c)
      if ((int64_t)child_tok[c] == tk) { e = c; break; }
    if (e < 0) { ok = false; break; }            // the sequence leaves the trie (a junk or filler beam, an empty slot)
    const int r = edge_row[e];
    if (r < 0) {
      leaf = true;
    } else if (n < max_depth) {
      out[n++] = p5_bound_key(r);
      node = row_node[r];
    } else {
      ok = false;
    }
  }
  if (!(ok && leaf)) n = 0;                      // not an item: none of its prefixes
  for (int i = n; i < max_depth; ++i) out[i] = 0ull;
}

// one workgroup per user: the seed kernel's keys into sel[b][0 .. n_b)
__global__ __launch_bounds__(256) void p5_bound_union_kernel(int* __restrict__ sel, int* __restrict__ n_rows, unsigned long long* __restrict__ keys, int KP,
                                                            int P, int cap) {
  __shared__ int s_w[4];
  const int b = blockIdx.x;
  const int m = p5_bound_union(keys + (size_t)b * KP, P, sel + (size_t)b * cap, cap, s_w);
  if (threadIdx.x == 0) n_rows[b] = m;
}

// ---- ROUND, after the certificate: one workgroup per user.  pl as p5_prune_certify_kernel takes it (sel and n_rows are read AND written:
// every read of the old sel precedes the sort's barriers, every write follows them).  keys: [B][KP], KP a power of two >= the plan's rows.
// grew[b] = 1 when rows were admitted ----
__global__ __launch_bounds__(256) void p5_bound_expand_kernel(int* __restrict__ sel_all, int* __restrict__ n_rows, int* __restrict__ grew,
                                                             unsigned long long* __restrict__ keys, int KP, const float* __restrict__ edge_lp,
                                                             long long n_edges, P5CandPlan pl, const int* __restrict__ row_edge,
                                                             const int* __restrict__ edge_row, const int* __restrict__ row_lmax,
                                                             const int* __restrict__ child_off, const float* __restrict__ out_score, int N, float margin) {
  __shared__ int s_w[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lim = pl.g.CQ * pl.g.nchunk;
  int n = n_rows[b];
  n = n < lim ? n : lim;
  n = n < pl.cap ? n : pl.cap;
  n = n < KP ? n : KP;
  n = n > 0 ? n : 0;
  int* sel = sel_all + (size_t)b * pl.cap;
  const float* __restrict__ lp = edge_lp + (size_t)b * n_edges;
  const float tau = out_score[(size_t)b * N + N - 1];
  unsigned long long* k = keys + (size_t)b * KP;
  // is the child row behind edge e, a row outside sel, within reach of tau?  P: the parent's sum
  auto admit = [&](int e, float P) -> int {
    const int c = edge_row[e];
    if (c < 0 || sel[p5_cand_find(sel, n, c, lim)] == c) return -1;
    const float Pc = P + lp[e];
    const float ub = Pc > 0.f ? Pc : Pc / (float)row_lmax[c];
    return !(ub < tau - margin) ? c : -1;         // (a NaN is admitted)
  };
  for (int i = tid; i < n; i += 256) k[i] = p5_bound_key(sel[i]);
  int base = n;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    int cnt = 0, e0 = 0, e1 = 0;
    float P = 0.f;                                 // P32(r), summed as the item score sums it
    if (i < n) {
      const int r = sel[i];
      const int dep = pl.g.row_depth[r];
      const int* __restrict__ anc = pl.g.anc + (size_t)r * pl.g.max_depth;
      for (int t = 1; t <= dep; ++t) P += lp[row_edge[t < dep ? anc[t] : r]];
      const int nd = pl.g.row_node[r];
      e0 = child_off[nd]; e1 = child_off[nd + 1];
      for (int e = e0; e < e1; ++e) cnt += admit(e, P) >= 0 ? 1 : 0;
    }
    int total;
    int at = base + p5_block_excl_scan(cnt, s_w, total);
    if (cnt)
      for (int e = e0; e < e1; ++e) {
        const int c = admit(e, P);
        if (c >= 0) {
          if (at < KP) k[at] = p5_bound_key(c);
          ++at;
        }
      }
    base += total;
  }
  base = base < KP ? base : KP;
  int P2 = 256;
  while (P2 < base) P2 <<= 1;                      // (<= KP: a power of two >= 256)
  for (int i = base + tid; i < P2; i += 256) k[i] = 0ull;
  __syncthreads();
  const int m = p5_bound_union(k, P2, sel, pl.cap, s_w);
  if (tid == 0) { n_rows[b] = m; grew[b] = m > n ? 1 : 0; }
}

// hdr[0] = the largest row count of the batch, hdr[1] = the number of users that grew (grew == nullptr: 0).  One wave; integer sums
__global__ __launch_bounds__(64) void p5_bound_hdr_kernel(int* __restrict__ hdr, const int* __restrict__ n_rows, const int* __restrict__ grew, int B) {
  int m = 0, g = 0;
  for (int b = threadIdx.x; b < B; b += 64) {
    m = n_rows[b] > m ? n_rows[b] : m;
    g += (grew && grew[b]) ? 1 : 0;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_xor(m, o);
    m = y > m ? y : m;
    g += __shfl_xor(g, o);
  }
  if (threadIdx.x == 0) { hdr[0] = m; hdr[1] = g; }
}
