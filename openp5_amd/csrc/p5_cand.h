// p5_cand.h -- per-user candidate lists: the exact beam-search score and order of C chosen items per user in one teacher-forced pass.
//
// p5_rank.h scores the whole trie: one row per non-leaf prefix, ONE plan for all users.  Here every user names C items (sampled-candidates
// evaluation, re-ranking a first stage's short list): the user's rows are the prefixes of those items only -- a subset of the trie's plan
// rows that is closed under "ancestor of" -- so the pass costs what the candidates cost, not what the catalogue costs, and no buffer
// grows with the catalogue.
//   PLAN    (device) p5_cand_plan_kernel: per user the global plan rows of the candidates' prefixes (item_rows, one table per trie),
//           sorted and made distinct: sel[b][0 .. n_b).  Global rows are numbered level by level, so in ascending order parents still
//           precede children.  A bitonic sort of integer keys and a prefix scan: no atomics, the same bits every call.
//           p5_cand_hdr_kernel: the largest n_b of the batch, the ONE integer the host reads to size the pass.
//   LAYOUT  as p5_rank.h: [chunk][user][CQ <= 512]; row i of user b is the prefix sel[b][i], rows beyond n_b are padding (pad token,
//           attend to themselves).  An ancestor (a global row) is found in sel[b] by binary search.
//   SCORE   per row the log-sum-exp over the vocabulary (p5_cand_lse*_kernel, the two head routes of p5_rank.h), then per (user, slot)
//           the candidate's path: hn[row of the prefix] . E[next token] * d_model^-0.5 - lse[row], summed in depth order, divided by the
//           number of tokens (p5_cand_score_kernel; the dot product in the arithmetic of p5_rank_score_kernel).  Only requested edges.
//   ORDER   p5_cand_order_kernel: per user the slots by (score desc, item index asc), empty slots last: bitonic sort of p5_wkey keys in
//           LDS; a slot finds its rank by binary search of its own key (a user's items are distinct, so keys are).
#pragma once
#include "p5_rank.h"

struct P5CandPlan {
  P5RankPlan g;           // the trie's plan (row_tok, row_depth, anc name GLOBAL rows) + the layout of the pass (g.rows: rows per user of the pass)
  const int* sel;         // [B][cap]  global rows of user b, ascending
  const int* n_rows;      // [B]
  int cap;                // stride of sel: C * path_len
};

// position of global row `row` in sel[0 .. n) (it is there: the row set is closed under "ancestor of"); never beyond lim - 1
__device__ static __forceinline__ int p5_cand_find(const int* __restrict__ sel, int n, int row, int lim) {
  int lo = 0, hi = (n < lim ? n : lim) - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sel[mid] < row) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- PLAN: one workgroup per user.  keys: [B][P] scratch, P = a power of two >= max(C * path_len, 256).  key of a row r: ~r (so the
// descending sort of p5_decode_wide.h yields ascending rows), 0 = no row (sorted last) ----
__global__ __launch_bounds__(256) void p5_cand_plan_kernel(int* __restrict__ sel, int* __restrict__ n_rows, unsigned long long* __restrict__ keys,
                                                          const int* __restrict__ cand, const int* __restrict__ item_rows, int C, int n_items,
                                                          int path_len, int cap, int P) {
  __shared__ int s_w[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long* k = keys + (size_t)b * P;
  for (int i = tid; i < P; i += 256) {
    unsigned long long key = 0ull;
    if (i < C * path_len) {
      const int c = cand[(size_t)b * C + i / path_len];
      if (c >= 0 && c < n_items) {
        const int r = item_rows[(size_t)c * path_len + i % path_len];
        if (r >= 0) key = (unsigned long long)(~(unsigned)r);
      }
    }
    k[i] = key;
  }
  __syncthreads();
  p5_wide_sort_desc(k, P);
  int* __restrict__ out = sel + (size_t)b * cap;
  int base = 0;
  for (int i0 = 0; i0 < P; i0 += 256) {
    if (k[i0] == 0ull) break;                  // (uniform: the empty keys are sorted last)
    const int i = i0 + tid;
    const unsigned long long key = k[i];
    const int first = (key != 0ull && (i == 0 || k[i - 1] != key)) ? 1 : 0;
    int total;
    const int pos = p5_block_excl_scan(first, s_w, total);
    if (first) out[base + pos] = (int)(~(unsigned)(key & 0xffffffffull));
    base += total;
  }
  if (tid == 0) n_rows[b] = base;
}
// hdr[0] = the largest row count of the batch (one wave)
__global__ __launch_bounds__(64) void p5_cand_hdr_kernel(int* __restrict__ hdr, const int* __restrict__ n_rows, int B) {
  int m = 0;
  for (int b = threadIdx.x; b < B; b += 64) m = n_rows[b] > m ? n_rows[b] : m;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_xor(m, o);
    m = y > m ? y : m;
  }
  if (threadIdx.x == 0) hdr[0] = m;
}

// decoder input ids of the pass (padding rows: the pad token)
__global__ __launch_bounds__(256) void p5_cand_rows_kernel(int64_t* __restrict__ ids, P5CandPlan pl, int pad_id) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= pl.g.B * pl.g.CQ * pl.g.nchunk) return;
  int b;
  const int ru = p5_rank_user_row(pl.g, g, b);
  ids[g] = ru < pl.n_rows[b] ? (int64_t)pl.g.row_tok[pl.sel[(size_t)b * pl.cap + ru]] : (int64_t)pad_id;
}

// self-attention of a row over its ancestors: p5_tree_attn_row on the trie's ancestor table, ancestors mapped through sel[b]
template <class T>
__global__ __launch_bounds__(256) void p5_cand_tree_attn_kernel(T* __restrict__ out, const T* __restrict__ qkv, P5CandPlan pl,
                                                               const float* __restrict__ rel_table, const int* __restrict__ lut, int lut_half,
                                                               int H) {
  const long long rh = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rh >= (long long)pl.g.B * pl.g.CQ * pl.g.nchunk * H) return;
  const int g = (int)(rh / H), h = (int)(rh % H);
  int b;
  const int ru = p5_rank_user_row(pl.g, g, b);
  const int n = pl.n_rows[b], lim = pl.g.CQ * pl.g.nchunk;
  const bool ok = ru < n;
  const int* __restrict__ sel = pl.sel + (size_t)b * pl.cap;
  const int gr = ok ? sel[ru] : 0;
  const int* __restrict__ anc = pl.g.anc + (size_t)gr * pl.g.max_depth;
  const P5RankPlan lay = pl.g;
  p5_tree_attn_row<T>(out, qkv, g, h, ok ? lay.row_depth[gr] : 0, anc, [=](int a) { return p5_rank_pass_row(lay, b, p5_cand_find(sel, n, a, lim)); },
                      rel_table, lut, lut_half, H);
}

// ---- SCORE, first half: log-sum-exp of rows g0 .. g0 + gridDim.x of the pass into row_lse ----
__global__ __launch_bounds__(256) void p5_cand_lse_kernel(float* __restrict__ row_lse, const float* __restrict__ part_m, const float* __restrict__ part_s,
                                                         int ntiles, int g0) {
  __shared__ float sm[4], ss[4];
  const int lr = blockIdx.x;
  const float lse = p5_rank_lse_from_partials(part_m + (size_t)lr * ntiles, part_s + (size_t)lr * ntiles, ntiles, sm, ss);
  if (threadIdx.x == 0) row_lse[g0 + lr] = lse;
}
__global__ __launch_bounds__(256) void p5_cand_lse_logits_kernel(float* __restrict__ row_lse, const float* __restrict__ logits, int ldl, int V, int g0) {
  __shared__ float sm[4], ss[4];
  const float lse = p5_rank_lse_from_logits(logits + (size_t)blockIdx.x * ldl, V, sm, ss);
  if (threadIdx.x == 0) row_lse[g0 + blockIdx.x] = lse;
}

// ---- SCORE, second half: grid (ceil(C / 32), B); eight lanes per (user, slot), the dot product as p5_rank_score_kernel forms it (16-byte
// loads, lane `sub` takes elements sub * EPF + k * 8 * EPF .., partial sums combined by xor-shuffles).  item_rows: [n_items][path_len]
// global row of the item's prefix at each depth, -1 beyond its last non-leaf prefix; item_tok: [n_items][ldt] int64, column 0 = the
// decoder start.  scores[b, j]: -1e9 for an empty slot ----
template <class T>
__global__ __launch_bounds__(256) void p5_cand_score_kernel(float* __restrict__ scores, const T* __restrict__ hn, const T* __restrict__ E, int d,
                                                           float alpha, const float* __restrict__ row_lse, P5CandPlan pl,
                                                           const int* __restrict__ cand, int C, const int* __restrict__ item_rows,
                                                           const int64_t* __restrict__ item_tok, int ldt, int n_items, int path_len) {
  constexpr int EPF = TT<T>::EPF;
  const int b = blockIdx.y, j = blockIdx.x * 32 + (threadIdx.x >> 3), sub = threadIdx.x & 7;
  const int c = j < C ? cand[(size_t)b * C + j] : -1;
  const int* __restrict__ sel = pl.sel + (size_t)b * pl.cap;
  const int nb = pl.n_rows[b], lim = pl.g.CQ * pl.g.nchunk;
  const int np = d / (8 * EPF);
  float s = 0.f;
  int n = 0;
  bool live = c >= 0 && c < n_items;
  for (int t = 0; t < path_len; ++t) {            // (every lane of the wave takes every trip: the shuffles below are wave-wide)
    const int r = live ? item_rows[(size_t)c * path_len + t] : -1;
    live = r >= 0;
    float acc = 0.f, lse = 0.f;
    if (live) {
      const int g = p5_rank_pass_row(pl.g, b, p5_cand_find(sel, nb, r, lim));
      const T* hp = hn + (size_t)g * d + sub * EPF;
      const T* ep = E + (size_t)item_tok[(size_t)c * ldt + t + 1] * d + sub * EPF;
      for (int k = 0; k < np; ++k) {
        float x[8], w[8];
        unpack16<T>(ld16(hp + k * 8 * EPF), x);
        unpack16<T>(ld16(ep + k * 8 * EPF), w);
#pragma unroll
        for (int e = 0; e < EPF; ++e) acc += x[e] * w[e];
      }
      lse = row_lse[g];
    }
    acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4);
    if (live) { s += acc * alpha - lse; ++n; }
  }
  if (sub == 0 && j < C) scores[(size_t)b * C + j] = n > 0 ? s / (float)n : -1.0e9f;
}

// ---- ORDER: one workgroup per user; C <= P5_WIDE_MAX_K.  out_order[b, k]: the slot at rank k, out_index its item, out_score its score;
// ranks beyond the user's candidates: -1, -1, -1e9 ----
__global__ __launch_bounds__(256) void p5_cand_order_kernel(int* __restrict__ out_order, int* __restrict__ out_index, float* __restrict__ out_score,
                                                           const float* __restrict__ scores, const int* __restrict__ cand, int C, int n_items, int N) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[P5_WIDE_MAX_K];     // 32 KiB
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P = p5_pow2_ceil(C);
  auto key_of = [&](int j) -> unsigned long long {
    const int c = j < C ? cand[(size_t)b * C + j] : -1;
    return (c >= 0 && c < n_items) ? p5_wkey(scores[(size_t)b * C + j], (unsigned)c) : 0ull;
  };
  for (int i = tid; i < P; i += 256) s_key[i] = key_of(i);
  __syncthreads();
  p5_wide_sort_desc(s_key, P);
  for (int i = tid; i < N; i += 256) {
    const unsigned long long k = s_key[i];
    out_index[(size_t)b * N + i] = k ? (int)(~(unsigned)(k & 0xffffffffull)) : -1;
    out_score[(size_t)b * N + i] = k ? p5_okey_inv((unsigned)(k >> 32)) : -1.0e9f;
    if (!k) out_order[(size_t)b * N + i] = -1;            // (a rank with a key is written by the slot that holds it, below)
  }
  for (int j = tid; j < C; j += 256) {
    const unsigned long long k = key_of(j);
    if (k == 0ull) continue;
    int lo = 0, hi = P - 1;                     // keys are distinct and sorted descending: the rank of k
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_key[mid] > k) lo = mid + 1; else hi = mid;
    }
    if (lo < N) out_order[(size_t)b * N + lo] = j;
  }
}
