// p5_rank.h -- exhaustive catalogue ranking: the exact beam-search score of EVERY item of the trie in one teacher-forced pass.
//
// Verified generation (p5_verify.h) scores the forest of prefixes a draft search kept alive.  Here the forest is the trie itself: one row
// per non-leaf node behind the decoder start token (the prefix that leads to it), so one decoder pass on the throughput GEMMs yields
// log p(token | prefix) for every edge of the trie, and the score HF's beam search assigns to an item -- the sum of its tokens'
// log-probabilities up to and including </s>, divided by their number -- is a sum along the item's path.  No search, no per-step
// selection, no beam-width limit.
//   PLAN    (host, once per trie: openp5_amd/trie.py::CompiledTrie.rank_plan)  per row: decoder input token, depth, trie node and the rows of
//           its ancestors.  ONE table for all users.
//   LAYOUT  the users' rows are the queries of the cross-attention kernels, which take up to 512 queries per user and launch: the pass lays
//           its rows out as [chunk][user][CQ] (CQ <= 512 rows of each user per chunk), so every chunk is one ordinary cross-attention
//           launch per layer and every other kernel sees one flat [rows, d] matrix.  Row `ru` of user b is row
//           ((ru / CQ) * B + b) * CQ + ru % CQ of the pass.
//   SCORE   p5_rank_score*_kernel: per row the log-sum-exp over the full vocabulary and the log-probability of EVERY child, stored per
//           (user, edge) -- edge = child_off[node] + i.
//   ITEMS   p5_rank_items_kernel: per (user, item) the edges of the item's path summed in depth order (the order the search adds them).
//   SELECT  p5_rank_select_part_kernel + p5_rank_select_kernel: per user the top N by (score desc, item index asc) without the items of a
//           per-user bitmap: G workgroups per user each keep the best N of their slice (radix select over integer histograms), one
//           workgroup per user selects among the G x N survivors and sorts them (p5_decode_wide.h's select + bitonic sort on 64-bit keys).
#pragma once
#include "p5_decode_wide.h"
#include "p5_verify.h"

struct P5RankPlan {
  const int* row_tok;     // [rows]  last token of the prefix (the decoder input of the row)
  const int* row_depth;   // [rows]  number of generated tokens in the prefix
  const int* row_node;    // [rows]  trie node the prefix leads to
  const int* anc;         // [rows][max_depth]  row of the ancestor at depth t < depth
  int rows, max_depth;    // rows per user; stride of anc
  int B, CQ, nchunk;      // layout of the pass: B * CQ * nchunk rows
};
__device__ static __forceinline__ int p5_rank_user_row(const P5RankPlan& pl, int g, int& b) {    // pass row -> (user, row of the plan)
  b = (g / pl.CQ) % pl.B;
  return (g / (pl.B * pl.CQ)) * pl.CQ + g % pl.CQ;
}
__device__ static __forceinline__ int p5_rank_pass_row(const P5RankPlan& pl, int b, int ru) {
  return ((ru / pl.CQ) * pl.B + b) * pl.CQ + ru % pl.CQ;
}

// a pass over a per-user subset of the plan's rows (p5_prune.h): row `ru` of user b of the pass is plan row sel[b][ru], ru < n_rows[b];
// sel == nullptr: the pass holds every plan row
struct P5RankSel { const int* sel; const int* n_rows; int cap; };
__device__ static __forceinline__ int p5_rank_plan_row(const P5RankPlan& pl, const P5RankSel& rs, int g, int& b) {    // pass row -> (user, plan row); -1: padding
  const int ru = p5_rank_user_row(pl, g, b);
  if (rs.sel == nullptr) return ru < pl.rows ? ru : -1;
  return ru < rs.n_rows[b] ? rs.sel[(size_t)b * rs.cap + ru] : -1;
}

// decoder input ids of the pass (padding rows: the pad token)
__global__ __launch_bounds__(256) void p5_rank_rows_kernel(int64_t* __restrict__ ids, P5RankPlan pl, int pad_id) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= pl.B * pl.CQ * pl.nchunk) return;
  int b;
  const int ru = p5_rank_user_row(pl, g, b);
  ids[g] = ru < pl.rows ? (int64_t)pl.row_tok[ru] : (int64_t)pad_id;
}

// self-attention of a row over its ancestors: p5_tree_attn_kernel's arithmetic on the shared plan (a padding row attends to itself)
template <class T>
__global__ __launch_bounds__(256) void p5_rank_tree_attn_kernel(T* __restrict__ out, const T* __restrict__ qkv, P5RankPlan pl,
                                                               const float* __restrict__ rel_table, const int* __restrict__ lut, int lut_half,
                                                               int H) {
  const long long rh = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rh >= (long long)pl.B * pl.CQ * pl.nchunk * H) return;
  const int g = (int)(rh / H), h = (int)(rh % H);
  int b;
  const int ru = p5_rank_user_row(pl, g, b);
  const bool ok = ru < pl.rows;
  const int* __restrict__ anc = pl.anc + (size_t)(ok ? ru : 0) * pl.max_depth;
  p5_tree_attn_row<T>(out, qkv, g, h, ok ? pl.row_depth[ru] : 0, anc, [=](int a) { return p5_rank_pass_row(pl, b, a); }, rel_table, lut, lut_half, H);
}

// range guard of the split-product pass (p5_verify_range_kernel's test) on the chunked layout: grid (B, nchunk)
template <class T>
__global__ __launch_bounds__(256) void p5_rank_range_kernel(int* __restrict__ flagged, const T* __restrict__ hn, int B, int CQ, int d) {
  const int b = blockIdx.x, ch = blockIdx.y;
  const T* __restrict__ p = hn + ((size_t)ch * B + b) * CQ * d;
  bool bad = false;
  for (int i = threadIdx.x; i < CQ * d; i += 256) bad |= !(fabsf(to_f<T>(p[i])) < 32768.f);
  if (bad) flagged[b] = 1;        // (every writer stores the same value)
}

// log-sum-exp of a row from the streaming head's per-tile (max, sum exp) partials, as p5_dec_score2_kernel / p5_wide_score2_kernel reduce them
__device__ static __forceinline__ float p5_rank_lse_from_partials(const float* __restrict__ pm_, const float* __restrict__ ps_, int ntiles,
                                                                 float* sm, float* ss) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float m = P5_NEG_INF, sum = 0.f;
  for (int t = tid; t < ntiles; t += 256) {
    const float pm = pm_[t], ps = ps_[t];
    if (pm > m) { sum = sum * expf(m - pm) + ps; m = pm; }
    else if (pm != P5_NEG_INF) sum += ps * expf(pm - m);
  }
  const float wm_ = wave_max(m);
  sum = wave_sum(m == P5_NEG_INF ? 0.f : sum * expf(m - wm_));
  if (lane == 0) { sm[wave] = wm_; ss[wave] = sum; }
  __syncthreads();
  m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  sum = 0.f;
  for (int w = 0; w < 4; ++w) sum += (sm[w] == P5_NEG_INF) ? 0.f : ss[w] * expf(sm[w] - m);
  return m + logf(sum);
}

// ---- SCORE, streaming head: rows g0 .. g0 + gridDim.x of the pass; partials are indexed by the row within this chunk of the head ----
// the children's logits are recomputed as hn . E (eight lanes per child, 16-byte loads), as p5_wide_score2_kernel does
template <class T>
__global__ __launch_bounds__(256) void p5_rank_score_kernel(float* __restrict__ edge_lp, long long n_edges, const float* __restrict__ part_m,
                                                           const float* __restrict__ part_s, int ntiles, const T* __restrict__ hn,
                                                           const T* __restrict__ E, int d, float alpha, P5RankPlan pl, int g0,
                                                           const int* __restrict__ child_off, const int* __restrict__ child_tok, P5RankSel rs) {
  constexpr int EPF = TT<T>::EPF;
  __shared__ float sm[4], ss[4];
  const int lr = blockIdx.x, g = g0 + lr, tid = threadIdx.x;
  int b;
  const int ru = p5_rank_plan_row(pl, rs, g, b);
  if (ru < 0) return;                          // padding row (uniform per block)
  const int nd = pl.row_node[ru];
  const int c0 = child_off[nd], nc = child_off[nd + 1] - c0;
  const float lse = p5_rank_lse_from_partials(part_m + (size_t)lr * ntiles, part_s + (size_t)lr * ntiles, ntiles, sm, ss);
  float* __restrict__ out = edge_lp + (size_t)b * n_edges + c0;
  constexpr int MAXP = 1024 / (8 * EPF);          // d_model <= 1024
  const int grp = tid >> 3, sub = tid & 7;
  const T* hp = hn + (size_t)g * d;
  const int np = d / (8 * EPF);
  u32x4 hx[MAXP];
#pragma unroll
  for (int k = 0; k < MAXP; ++k) hx[k] = k < np ? ld16(hp + sub * EPF + k * 8 * EPF) : zero16();
  int tok_next = grp < nc ? child_tok[c0 + grp] : 0;
  for (int i0 = 0; i0 < nc; i0 += 32) {
    const int i = i0 + grp;
    const int tok = tok_next;
    if (i + 32 < nc) tok_next = child_tok[c0 + i + 32];
    float acc = 0.f;
    if (i < nc) {
      const T* ep = E + (size_t)tok * d + sub * EPF;
#pragma unroll
      for (int k0 = 0; k0 < MAXP; k0 += 8) {
        if (k0 < np) {
          u32x4 wr[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) wr[k] = k0 + k < np ? ld16(ep + (k0 + k) * 8 * EPF) : zero16();
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float x[8], w[8];
            unpack16<T>(hx[k0 + k], x);
            unpack16<T>(wr[k], w);
#pragma unroll
            for (int e = 0; e < EPF; ++e) acc += x[e] * w[e];
          }
        }
      }
    }
    acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4);
    if (i < nc && sub == 0) out[i] = acc * alpha - lse;
  }
}

// log-sum-exp of one row of materialised logits, as p5_dec_score_kernel computes it (sm, ss: 4 floats of LDS each)
__device__ static __forceinline__ float p5_rank_lse_from_logits(const float* __restrict__ lr, int V, float* sm, float* ss) {
  const int tid = threadIdx.x;
  float m = P5_NEG_INF, sum = 0.f;
  const int V4 = V >> 2;
  for (int j = tid; j < V4; j += 256) {
    const f32x4 v = *(const f32x4*)(lr + 4 * j);
    const float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (mx > m) { sum *= expf(m - mx); m = mx; }
    sum += expf(v[0] - m) + expf(v[1] - m) + expf(v[2] - m) + expf(v[3] - m);
  }
  for (int j = (V4 << 2) + tid; j < V; j += 256) {
    const float v = lr[j];
    if (v > m) { sum *= expf(m - v); m = v; }
    sum += expf(v - m);
  }
  {
    const float wm_ = wave_max(m);
    sum = wave_sum(m == P5_NEG_INF ? 0.f : sum * expf(m - wm_));
    if ((tid & 63) == 0) { sm[tid >> 6] = wm_; ss[tid >> 6] = sum; }
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    sum = 0.f;
    for (int w = 0; w < 4; ++w) sum += ss[w] * expf(sm[w] - m);
  }
  return m + logf(sum);
}

// ---- SCORE over materialised logits (toy widths, and the split-product head): logits hold rows g0 .. of the pass; lse as
// p5_dec_score_kernel computes it ----
__global__ __launch_bounds__(256) void p5_rank_score_logits_kernel(float* __restrict__ edge_lp, long long n_edges, const float* __restrict__ logits,
                                                                  int ldl, int V, P5RankPlan pl, int g0, const int* __restrict__ child_off,
                                                                  const int* __restrict__ child_tok, P5RankSel rs) {
  __shared__ float sm[4], ss[4];
  const int g = g0 + blockIdx.x, tid = threadIdx.x;
  int b;
  const int ru = p5_rank_plan_row(pl, rs, g, b);
  if (ru < 0) return;
  const float* lr = logits + (size_t)blockIdx.x * ldl;
  const float lse = p5_rank_lse_from_logits(lr, V, sm, ss);
  const int nd = pl.row_node[ru];
  const int c0 = child_off[nd], nc = child_off[nd + 1] - c0;
  float* __restrict__ out = edge_lp + (size_t)b * n_edges + c0;
  for (int c = tid; c < nc; c += 256) out[c] = lr[child_tok[c0 + c]] - lse;
}

// ---- ITEMS: scores[b, i] = (sum of the edge log-probabilities of item i's path, in depth order) / (number of tokens).  item_edges:
// [n_items][path_len] edge ids behind the decoder start token, -1 beyond the item's </s>.  grid (ceil(n_items / 256), B) ----
__global__ __launch_bounds__(256) void p5_rank_items_kernel(float* __restrict__ scores, const float* __restrict__ edge_lp, long long n_edges,
                                                           const int* __restrict__ item_edges, int n_items, int path_len) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= n_items) return;
  const float* __restrict__ lp = edge_lp + (size_t)b * n_edges;
  const int* __restrict__ pe = item_edges + (size_t)i * path_len;
  float s = 0.f;
  int n = 0;
  for (; n < path_len; ++n) {
    const int e = pe[n];
    if (e < 0) break;
    s += lp[e];
  }
  scores[(size_t)b * n_items + i] = n > 0 ? s / (float)n : -1.0e9f;
}

// key of item i of a user: 0 = excluded (never selected); larger = better (score desc, then item index asc)
__device__ static __forceinline__ unsigned long long p5_rank_item_key(const float* __restrict__ sc, const uint32_t* __restrict__ ex, int i) {
  if (ex && ((ex[i >> 5] >> (i & 31)) & 1u)) return 0ull;
  return p5_wkey(sc[i], (unsigned)i);
}

// ---- SELECT, first stage: grid (G, B); workgroup (g, b) keeps the best min(N, slice) keys of items [g * S, (g + 1) * S) of user b in
// part[b][g][0 .. N) (unordered; 0 = empty slot) ----
__global__ __launch_bounds__(256) void p5_rank_select_part_kernel(unsigned long long* __restrict__ part, const float* __restrict__ scores,
                                                                 const uint32_t* __restrict__ excluded, int excl_words, int n_items, int S, int N) {
  __shared__ int hist[256];
  __shared__ int s_sel[4], s_w[4];
  const int g = blockIdx.x, b = blockIdx.y, G = gridDim.x, tid = threadIdx.x;
  const int lo = g * S;
  int n = n_items - lo;
  n = n < 0 ? 0 : (n < S ? n : S);
  const float* __restrict__ sc = scores + (size_t)b * n_items;
  const uint32_t* __restrict__ ex = excluded ? excluded + (size_t)b * excl_words : nullptr;
  unsigned long long* __restrict__ out = part + ((size_t)b * G + g) * N;
  auto key_at = [&](int i) -> unsigned long long { return p5_rank_item_key(sc, ex, lo + i); };
  const unsigned long long thr = p5_wide_radix_select(n, N, key_at, hist, s_sel, s_w);
  if (tid == 0) s_sel[2] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const unsigned long long k = key_at(i);
    if (k != 0ull && k >= thr) out[atomicAdd(&s_sel[2], 1)] = k;      // (integer LDS counter: which slot a key lands in is not part of any result)
  }
  __syncthreads();
  for (int i = s_sel[2] + tid; i < N; i += 256) out[i] = 0ull;
}

// ---- SELECT, second stage: one workgroup per user; the top N of the G x N survivors, sorted; fewer than N candidates: score -1e9,
// index -1 (as generate() fills dead beams) ----
__global__ __launch_bounds__(256) void p5_rank_select_kernel(int* __restrict__ out_index, float* __restrict__ out_score,
                                                            const unsigned long long* __restrict__ part, int G, int N) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[P5_WIDE_MAX_K];     // 32 KiB
  __shared__ int hist[256];
  __shared__ int s_sel[4], s_w[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* __restrict__ in = part + (size_t)b * G * N;
  const int n = G * N, P = p5_pow2_ceil(N);
  auto key_at = [&](int i) -> unsigned long long { return in[i]; };
  const unsigned long long thr = p5_wide_radix_select(n, N, key_at, hist, s_sel, s_w);
  for (int i = tid; i < P; i += 256) s_key[i] = 0ull;
  if (tid == 0) s_sel[2] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const unsigned long long k = in[i];
    if (k != 0ull && k >= thr) s_key[atomicAdd(&s_sel[2], 1)] = k;
  }
  __syncthreads();
  p5_wide_sort_desc(s_key, P);
  for (int i = tid; i < N; i += 256) {
    const unsigned long long k = s_key[i];
    out_index[(size_t)b * N + i] = k ? (int)(~(unsigned)(k & 0xffffffffull)) : -1;
    out_score[(size_t)b * N + i] = k ? p5_okey_inv((unsigned)(k >> 32)) : -1.0e9f;
  }
}
