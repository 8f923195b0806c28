// p5_decode_wide.h -- wide constrained beam search: 65 .. 4096 beams per batch item (and any width under p5_set_option("gen_wide", 1)).
//
// The narrow search (p5_decode.h) keeps an item's whole beam state and its K x 2K candidate pool in one workgroup's LDS, which ends at
// K = 64.  The widened-beam filtered evaluation (DistributedRunner.py:204-269: num_beams = generate_num + longest history) needs
// thousands of beams, so here the state lives in global memory and the step after the decoder is four launches:
//   p5_wide_score*_kernel   one workgroup per row: log-sum-exp, the trie children's scores, the row's best min(nc, 2K) candidates as
//                           64-bit keys (score desc, then flat index beam * max_c + child asc: the narrow path's order, HF's flat
//                           beam * V + token order)
//   p5_wide_select_kernel   one workgroup per item: exact top-2K of the item's pool (radix select over integer histograms, compaction,
//                           bitonic sort of the unique keys in LDS -- no result depends on the order atomics land in), the candidates'
//                           tokens / nodes, the K running beams (stable order of score - 1e9 * hit)
//   p5_wide_scorer_kernel   one workgroup per item: HF's finished-set update (utils.py:3008-3075 / p5_beam_tail) and early-stop test
//   p5_wide_commit_kernel   (items x beam chunks): next running / finished sequences, ancestry, next step's x32 rows; the last
//                           workgroup advances the step counter and raises the done flag (flags[0..4] protocol of P5BeamState)
// Every result equals the narrow path's bit for bit (tests/test_wide_beams_emu.py runs both at K <= 64).
#pragma once
#include "p5_decode.h"

#define P5_WIDE_MAX_K 4096
#define P5_WIDE_MAX_K2 (2 * P5_WIDE_MAX_K)
#define P5_WIDE_COMMIT_BEAMS 16        // beams per workgroup of p5_wide_commit_kernel

__device__ static __forceinline__ unsigned p5_okey(float v) {       // order-preserving float -> uint
  union { float f; unsigned u; } c; c.f = v;
  return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
__device__ static __forceinline__ float p5_okey_inv(unsigned o) {
  union { float f; unsigned u; } c;
  c.u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return c.f;
}
// candidate key: larger = better.  Finite scores only (0 marks "no candidate"; p5_okey of a finite float is never 0).  -0.0 and +0.0 tie as
// numbers but p5_okey orders their bits, so a zero of either sign takes +0.0's key: between them the index decides (score desc, index asc)
__device__ static __forceinline__ unsigned long long p5_wkey(float v, unsigned idx) {
  return ((unsigned long long)p5_okey(v == 0.f ? 0.f : v) << 32) | (unsigned long long)(~idx);
}

// exclusive prefix sum of one int per thread over the 256 threads; `total` = the block's sum (s_w: 4 ints of LDS)
__device__ static __forceinline__ int p5_block_excl_scan(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl(inc, lane >= o ? lane - o : 0);
    if (lane >= o) inc += y;
  }
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) { before += (w < wave) ? s_w[w] : 0; total += s_w[w]; }
  return before + inc - v;
}

// block-wide radix select over n unique 64-bit keys key_at(i) (0 = absent): returns T with #{present keys >= T} == want, or 1 when
// at most `want` keys are present (take them all).  Eight passes of an 8-bit integer histogram: counts, hence T, do not depend on
// the order the atomics land in.
template <class KeyAt>
__device__ static unsigned long long p5_wide_radix_select(int n, int want, KeyAt key_at, int* hist, int* s_sel, int* s_w) {
  const int tid = threadIdx.x;
  unsigned long long prefix = 0ull, mask = 0ull;
  int remaining = want;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const unsigned long long k = key_at(i);
      if (k != 0ull && (k & mask) == prefix) atomicAdd(&hist[(int)((k >> shift) & 255ull)], 1);
    }
    __syncthreads();
    const int own = hist[255 - tid];            // thread t owns bin 255 - t: `before` = keys in strictly higher bins
    int total;
    const int before = p5_block_excl_scan(own, s_w, total);
    if (pass == 0 && total <= want) return 1ull;          // (uniform: every thread sees the same total)
    if (before < remaining && before + own >= remaining) { s_sel[0] = 255 - tid; s_sel[1] = before; }
    __syncthreads();
    prefix |= (unsigned long long)s_sel[0] << shift;
    mask |= 255ull << shift;
    remaining -= s_sel[1];
    __syncthreads();
  }
  return prefix;                                 // the want-th largest key itself (keys are unique)
}

// descending bitonic sort of n (a power of two <= 8192) keys in LDS; the caller has synchronised the block before
__device__ static void p5_wide_sort_desc(unsigned long long* a, int n) {
  for (int k = 2; k <= n; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int i = threadIdx.x; i < n; i += 256) {
        const int l = i ^ jj;
        if (l > i) {
          const unsigned long long x = a[i], y = a[l];
          if ((i & k) == 0 ? (x < y) : (x > y)) { a[i] = y; a[l] = x; }
        }
      }
      __syncthreads();
    }
}
__device__ static __forceinline__ int p5_pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// the row's best min(nc, C) candidates from its scores sc[0 .. nc) (-inf = not allowed) into row_key[r, 0 .. C), row_n[r] = slots used.
// nc <= C: every child gets its slot (0 for an excluded one); otherwise radix select of the C-th key and compaction.
__device__ static void p5_wide_row_emit(unsigned long long* __restrict__ row_key, int* __restrict__ row_n, const float* sc, int r, int j, int nc,
                                        int C, int max_c, int* hist, int* s_sel, int* s_w) {
  const int tid = threadIdx.x;
  unsigned long long* out = row_key + (size_t)r * C;
  const unsigned base = (unsigned)j * (unsigned)max_c;
  auto key_at = [&](int i) -> unsigned long long {
    const float v = sc[i];
    return v == P5_NEG_INF ? 0ull : p5_wkey(v, base + (unsigned)i);
  };
  if (nc <= C) {
    for (int i = tid; i < nc; i += 256) out[i] = key_at(i);
    if (tid == 0) row_n[r] = nc;
    return;
  }
  const unsigned long long thr = p5_wide_radix_select(nc, C, key_at, hist, s_sel, s_w);
  if (tid == 0) s_sel[2] = 0;
  __syncthreads();
  for (int i = tid; i < nc; i += 256) {
    const unsigned long long k = key_at(i);
    if (k != 0ull && k >= thr) out[atomicAdd(&s_sel[2], 1)] = k;
  }
  __syncthreads();
  if (tid == 0) row_n[r] = s_sel[2];
}

// ---- a. row scoring, streaming head (per-tile (max, sum exp) partials; children's logits recomputed as hn . E) ----
// lse and the children's scores are computed exactly as p5_dec_score2_kernel computes them
template <class T>
__global__ __launch_bounds__(256) void p5_wide_score2_kernel(unsigned long long* __restrict__ row_key, int* __restrict__ row_n, float* __restrict__ cand,
                                                            const float* __restrict__ part_m, const float* __restrict__ part_s, int ntiles,
                                                            const T* __restrict__ hn, const T* __restrict__ E, int d, float alpha,
                                                            const int* __restrict__ node, const float* __restrict__ run_score,
                                                            const int* __restrict__ child_off, const int* __restrict__ child_tok,
                                                            const int* __restrict__ child_node, const uint32_t* __restrict__ excluded, int excl_words,
                                                            int Kb, int max_c, int C, const int* __restrict__ done) {
  constexpr int EPF = TT<T>::EPF;
  __shared__ float sm[4], ss[4];
  __shared__ int hist[256];
  __shared__ int s_sel[4], s_w[4];
  if (done && *done) return;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nd = node[r];
  if (nd < 0) {  // dead beam: no candidates (uniform per block)
    if (tid == 0) row_n[r] = 0;
    return;
  }
  const int c0 = child_off[nd];
  int nc = child_off[nd + 1] - c0;
  nc = nc < max_c ? nc : max_c;
  const float rs = run_score[r];
  float m = P5_NEG_INF, sum = 0.f;
  for (int t = tid; t < ntiles; t += 256) {
    const float pm = part_m[(size_t)r * ntiles + t], ps = part_s[(size_t)r * ntiles + t];
    if (pm > m) { sum = sum * expf(m - pm) + ps; m = pm; }
    else if (pm != P5_NEG_INF) sum += ps * expf(pm - m);
  }
  {
    const float wm_ = wave_max(m);
    sum = wave_sum(m == P5_NEG_INF ? 0.f : sum * expf(m - wm_));
    if (lane == 0) { sm[wave] = wm_; ss[wave] = sum; }
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    sum = 0.f;
    for (int w = 0; w < 4; ++w) sum += (sm[w] == P5_NEG_INF) ? 0.f : ss[w] * expf(sm[w] - m);
  }
  const float lse = m + logf(sum);
  float* pv = cand + (size_t)r * max_c;
  const uint32_t* ex = excluded ? excluded + (size_t)(r / Kb) * excl_words : nullptr;
  {
    constexpr int MAXP = 1024 / (8 * EPF);          // d_model <= 1024
    const int grp = tid >> 3, sub = tid & 7;
    const T* hp = hn + (size_t)r * d;
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
      if (i < nc && sub == 0) {
        float v = (acc * alpha - lse) + rs;
        if (ex) {
          const int cn = child_node[c0 + i];
          if ((ex[cn >> 5] >> (cn & 31)) & 1u) v = P5_NEG_INF;
        }
        pv[i] = v;
      }
    }
  }
  __syncthreads();
  p5_wide_row_emit(row_key, row_n, pv, r, r % Kb, nc, C, max_c, hist, s_sel, s_w);
}

// ---- a'. row scoring over materialised logits (toy widths: head_nv() == 0); lse as p5_dec_score_kernel computes it ----
__global__ __launch_bounds__(256) void p5_wide_score_kernel(unsigned long long* __restrict__ row_key, int* __restrict__ row_n, float* __restrict__ cand,
                                                           const float* __restrict__ logits, int ldl, int V, const int* __restrict__ node,
                                                           const float* __restrict__ run_score, const int* __restrict__ child_off,
                                                           const int* __restrict__ child_tok, const int* __restrict__ child_node,
                                                           const uint32_t* __restrict__ excluded, int excl_words, int Kb, int max_c, int C,
                                                           const int* __restrict__ done) {
  __shared__ float sm[4], ss[4];
  __shared__ int hist[256];
  __shared__ int s_sel[4], s_w[4];
  if (done && *done) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int nd = node[r];
  if (nd < 0) {
    if (tid == 0) row_n[r] = 0;
    return;
  }
  const float* lr = logits + (size_t)r * ldl;
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
  const float lse = m + logf(sum);
  const int c0 = child_off[nd];
  int nc = child_off[nd + 1] - c0;
  if (nc > max_c) nc = max_c;
  const float rs = run_score[r];
  float* cs = cand + (size_t)r * max_c;
  const uint32_t* ex = excluded ? excluded + (size_t)(r / Kb) * excl_words : nullptr;
  for (int c = tid; c < nc; c += 256) {
    float v = (lr[child_tok[c0 + c]] - lse) + rs;
    if (ex) {
      const int cn = child_node[c0 + c];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) v = P5_NEG_INF;
    }
    cs[c] = v;
  }
  __syncthreads();
  p5_wide_row_emit(row_key, row_n, cs, r, r % Kb, nc, C, max_c, hist, s_sel, s_w);
}

// scratch of the wide step in global memory: the item's top-2K candidates in rank order, the running selection, the finished set's sources
struct P5WideWs {
  unsigned long long* row_key;   // [R, C] per-row candidate keys (C = min(max_c, 2K))
  int* row_n;                    // [R] slots used
  float* top_lp;                 // [B, 2K] candidate scores in (score desc, flat index asc) order; -inf beyond the live candidates
  int *top_beam, *top_tok, *top_node;   // [B, 2K] (0, 0, -1 beyond the live candidates, as the narrow path)
  int* sel_run;                  // [B, K] position (in the top-2K list) of running beam j of the next step
  int* fin_src;                  // [B, K] finished hypothesis j of the next step: old finished index >= 0, or -(position + 1)
};

// ---- b. one workgroup per item: exact top-2K of the item's pool of K x C keys, the candidates' tokens / nodes, HF step d-e ----
__global__ __launch_bounds__(256) void p5_wide_select_kernel(P5BeamState st, P5WideWs ws, const int* __restrict__ child_off,
                                                            const int* __restrict__ child_tok, const int* __restrict__ child_node, int max_c, int Kb,
                                                            int C, int max_len, int eos_id) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[P5_WIDE_MAX_K2];     // 64 KiB
  __shared__ int hist[256];
  __shared__ int s_sel[4], s_w[4];
  __shared__ int s_nothit;
  if (st.flags[4]) return;       // the search stopped in an earlier step
  const int cur_len = st.flags[2];
  const bool at_max = (cur_len + 1 >= max_len);
  const int b = blockIdx.x, tid = threadIdx.x, K2 = 2 * Kb;
  const int n = Kb * C;
  auto key_at = [&](int t) -> unsigned long long {
    const int j = t / C, i = t - j * C;
    return i < ws.row_n[b * Kb + j] ? ws.row_key[(size_t)(b * Kb + j) * C + i] : 0ull;
  };
  const unsigned long long thr = p5_wide_radix_select(n, K2, key_at, hist, s_sel, s_w);
  if (tid == 0) { s_sel[2] = 0; s_nothit = 0; }
  __syncthreads();
  for (int t = tid; t < n; t += 256) {          // compaction: positions depend on the atomics' order, the sort below removes it
    const unsigned long long k = key_at(t);
    if (k != 0ull && k >= thr) s_key[atomicAdd(&s_sel[2], 1)] = k;
  }
  __syncthreads();
  const int cnt = s_sel[2];                      // == min(2K, live candidates)
  const int np = p5_pow2_ceil(cnt > 1 ? cnt : 1);
  for (int i = cnt + tid; i < np; i += 256) s_key[i] = 0ull;
  __syncthreads();
  p5_wide_sort_desc(s_key, np);
  // ---- the candidates in rank order (fewer than 2K live ones: the rest are -inf placeholders, as the narrow path's) ----
  float* top_lp = ws.top_lp + (size_t)b * K2;
  int* top_beam = ws.top_beam + (size_t)b * K2;
  int* top_tok = ws.top_tok + (size_t)b * K2;
  int* top_node = ws.top_node + (size_t)b * K2;
  for (int i = tid; i < K2; i += 256) {
    float v = P5_NEG_INF;
    int j = 0, tok = 0, nd = -1;
    if (i < cnt) {
      const unsigned long long k = s_key[i];
      v = p5_okey_inv((unsigned)(k >> 32));
      const unsigned idx = ~(unsigned)k;
      j = (int)(idx / (unsigned)max_c);
      const int c = (int)(idx - (unsigned)j * (unsigned)max_c);
      const int co = child_off[st.run_node[b * Kb + j]];
      tok = child_tok[co + c];
      nd = child_node[co + c];
    }
    top_lp[i] = v; top_beam[i] = j; top_tok[i] = tok; top_node[i] = nd;
    const int h = (tok == eos_id) || at_max;
    if (!h) atomicAdd(&s_nothit, 1);
  }
  __syncthreads();
  // ---- e: running beams = stable top-K of run_lp = score - 1e9 * hit (key: run_lp desc, position asc) ----
  for (int i = tid; i < K2; i += 256) {
    const int h = (top_tok[i] == eos_id) || at_max;
    const float rl = top_lp[i] + (h ? -1.0e9f : 0.f);
    s_key[i] = ((unsigned long long)p5_okey(rl) << 32) | (unsigned long long)(~(unsigned)i);
  }
  const int np2 = p5_pow2_ceil(K2);
  for (int i = K2 + tid; i < np2; i += 256) s_key[i] = 0ull;
  __syncthreads();
  p5_wide_sort_desc(s_key, np2);
  // run_node is read above (old nodes) and written here: the sorts' barriers separate the two
  for (int q = tid; q < Kb; q += 256) {
    const unsigned long long k = s_key[q];
    const int i = (int)(~(unsigned)k);
    ws.sel_run[b * Kb + q] = i;
    st.run_node[b * Kb + q] = top_node[i];
    st.last_tok[b * Kb + q] = (int64_t)top_tok[i];
    st.run_score[b * Kb + q] = p5_okey_inv((unsigned)(k >> 32));
  }
  if (tid == 0 && s_nothit > 0) atomicAdd(&st.flags[1], 1);
}

// ---- c. one workgroup per item: f (finished set = stable top-K over [old finished ; new EOS candidates ranked < K]) and g (early stop) ----
// The stored finished list is in rank order (non-increasing, written by rank) and so are the qualifying new candidates (positions of the
// top-2K list): the stable top-K of their union is a merge, old before new on equal scores.  A candidate that does not qualify (not a
// hit, ranked >= K, or the item already done) carries its score - 1e9 <= -1e9 and loses to each of the K old entries (>= -1e9, ties to
// the lower index): it never enters, as in p5_beam_tail.
__global__ __launch_bounds__(256) void p5_wide_scorer_kernel(P5BeamState st, P5WideWs ws, int Kb, int max_len, int eos_id) {
  __shared__ float s_old[P5_WIDE_MAX_K], s_nv[P5_WIDE_MAX_K], s_fsc[P5_WIDE_MAX_K];
  __shared__ int s_ofl[P5_WIDE_MAX_K], s_oln[P5_WIDE_MAX_K], s_ni[P5_WIDE_MAX_K], s_ffl[P5_WIDE_MAX_K];
  __shared__ int s_w[4];
  __shared__ float s_mn[4];
  __shared__ int s_any;
  if (st.flags[4]) return;
  const int cur_len = st.flags[2];
  const bool at_max = (cur_len + 1 >= max_len);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K2 = 2 * Kb;
  const bool uns = st.unsat[b] != 0;
  const float* top_lp = ws.top_lp + (size_t)b * K2;
  const int* top_tok = ws.top_tok + (size_t)b * K2;
  for (int j = tid; j < Kb; j += 256) {
    s_old[j] = st.fin_score[b * Kb + j]; s_ofl[j] = st.fin_flag[b * Kb + j]; s_oln[j] = st.fin_len[b * Kb + j];
  }
  // qualifying candidates (position i < K, a hit, item not done) in position order: each thread owns a contiguous run of positions
  const int per = (Kb + 255) / 256, i_lo = tid * per, i_hi = (i_lo + per < Kb) ? i_lo + per : Kb;
  int q = 0;
  if (uns)
    for (int i = i_lo; i < i_hi; ++i) q += ((top_tok[i] == eos_id) || at_max) ? 1 : 0;
  int nq;
  int at = p5_block_excl_scan(q, s_w, nq);
  if (uns)
    for (int i = i_lo; i < i_hi; ++i)
      if ((top_tok[i] == eos_id) || at_max) { s_nv[at] = top_lp[i] / (float)cur_len; s_ni[at] = i; ++at; }
  if (tid == 0) s_any = 0;
  __syncthreads();
  int* fin_src = ws.fin_src + (size_t)b * Kb;
  for (int j = tid; j < Kb; j += 256) {           // old entry j: rank = j + #{new strictly better}
    const float v = s_old[j];
    int lo = 0, hi = nq;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_nv[mid] > v) lo = mid + 1; else hi = mid; }
    const int rank = j + lo;
    if (rank < Kb) { s_fsc[rank] = v; fin_src[rank] = j; s_ffl[rank] = s_ofl[j]; st.fin_len[b * Kb + rank] = s_oln[j]; }
  }
  for (int t = tid; t < nq; t += 256) {           // new entry t: rank = t + #{old at least as good}
    const float v = s_nv[t];
    int lo = 0, hi = Kb;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_old[mid] >= v) lo = mid + 1; else hi = mid; }
    const int rank = t + lo;
    if (rank < Kb) { s_fsc[rank] = v; fin_src[rank] = -(s_ni[t] + 1); s_ffl[rank] = 1; st.fin_len[b * Kb + rank] = cur_len; }
  }
  __syncthreads();
  // ---- g: early-stop heuristic with the NEW running / finished sets ----
  float mn = INFINITY;
  for (int j = tid; j < Kb; j += 256) {
    st.fin_score[b * Kb + j] = s_fsc[j];
    st.fin_flag[b * Kb + j] = s_ffl[j];
    mn = fminf(mn, s_fsc[j]);
  }
  mn = -wave_max(-mn);
  if (lane == 0) s_mn[wave] = mn;
  __syncthreads();
  mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
  const float best_possible = st.run_score[b * Kb] / (float)cur_len;   // (cur_len+1) - prompt_len(1)
  for (int j = tid; j < Kb; j += 256)
    if (best_possible > (s_ffl[j] ? mn : -1.0e9f)) atomicMax(&s_any, 1);
  __syncthreads();
  if (tid == 0) {
    const int new_unsat = (uns && s_any) ? 1 : 0;
    st.unsat[b] = new_unsat;
    if (new_unsat) atomicAdd(&st.flags[0], 1);
  }
}

// ---- c'. grid (ceil(K / 16), B): materialise the next running / finished sequences, ancestry and x32 rows; step counter + stop flag ----
__global__ __launch_bounds__(256) void p5_wide_commit_kernel(P5BeamState st, P5WideWs ws, int Kb, int max_len, int R) {
  if (st.flags[4]) return;
  const int cur_len = st.flags[2];
  if ((cur_len & 1) == 0) {      // even step: the "next" buffers of the previous step are the current ones
    int* t;
    t = st.run_seq; st.run_seq = st.run_seq_next; st.run_seq_next = t;
    t = st.fin_seq; st.fin_seq = st.fin_seq_next; st.fin_seq_next = t;
    t = st.anc; st.anc = st.anc_next; st.anc_next = t;
  }
  const int b = blockIdx.y, j0 = blockIdx.x * P5_WIDE_COMMIT_BEAMS, tid = threadIdx.x, K2 = 2 * Kb;
  const int nb = (Kb - j0) < P5_WIDE_COMMIT_BEAMS ? (Kb - j0) : P5_WIDE_COMMIT_BEAMS;
  const int* top_beam = ws.top_beam + (size_t)b * K2;
  const int* top_tok = ws.top_tok + (size_t)b * K2;
  const int* sel_run = ws.sel_run + (size_t)b * Kb;
  const int* fin_src = ws.fin_src + (size_t)b * Kb;
  const size_t ib = (size_t)b * Kb;
  for (int t = tid; t < nb * max_len; t += 256) {
    const int j = j0 + t / max_len, p = t % max_len;
    const int fs = fin_src[j];
    int v;
    if (fs >= 0) v = st.fin_seq[(ib + fs) * max_len + p];
    else {
      const int i = -fs - 1;
      v = (p == cur_len) ? top_tok[i] : st.run_seq[(ib + top_beam[i]) * max_len + p];
    }
    st.fin_seq_next[(ib + j) * max_len + p] = v;
    const int i = sel_run[j];
    st.run_seq_next[(ib + j) * max_len + p] = (p == cur_len) ? top_tok[i] : st.run_seq[(ib + top_beam[i]) * max_len + p];
  }
  const int pos = cur_len - 1;   // K/V of this step were stored at `pos` by row (b*Kb + old beam)
  for (int t = tid; t < nb * (pos + 1); t += 256) {
    const int j = j0 + t / (pos + 1), p = t % (pos + 1);
    const int parent = top_beam[sel_run[j]];
    st.anc_next[(size_t)p * R + ib + j] = (p == pos) ? (int)ib + parent : st.anc[(size_t)p * R + ib + parent];
  }
  if (st.x32) {      // decoder input of the next step: x32[row, :] = E32[token, :]
    const int d4 = st.d >> 2, n4 = nb * d4;
    for (int t = tid; t < n4; t += 256) {
      const int j = j0 + t / d4, c4 = t % d4;
      *(f32x4*)(st.x32 + (ib + j) * st.d + c4 * 4) = *(const f32x4*)(st.E32 + (size_t)top_tok[sel_run[j]] * st.d + c4 * 4);
    }
  }
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    if (atomicAdd(&st.flags[3], 1) == (int)(gridDim.x * gridDim.y) - 1) {
      st.flags[3] = 0;
      st.flags[2] = cur_len + 1;
      const int any_unsat = atomicExch(&st.flags[0], 0), not_all_hits = atomicExch(&st.flags[1], 0);
      if (!(any_unsat > 0 && not_all_hits > 0)) st.flags[4] = 1;
    }
  }
}
