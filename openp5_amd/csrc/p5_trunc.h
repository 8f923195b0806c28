// p5_trunc.h -- top-k / nucleus TRUNCATION of the trie-constrained distribution: the sampler of p5_sample.h and the item loss of p5_trie_ce.h
// under HF's order of warpers (processors, temperature, TopKLogitsWarper, TopPLogitsWarper, softmax), restated on the allowed children.
//
// For a row at trie node n: A = the children that are not excluded and have a finite logit, z_i = logit_i / tau.
//   top-k   K1 = { i in A : z_i >= the k-th largest z of A }  (ties at the k-th value all stay: HF's `scores < kth`; |A| <= k: K1 = A)
//   top-p   over softmax(z | K1): child i stays iff mass{ j in K1 : z_j > z_i } < top_p * mass(K1).  HF's "remove while the ascending
//           cumulative probability <= 1 - top_p", by VALUE: children with equal z stay or leave together (HF cuts inside such a group by
//           sort position), so the result does not depend on the order of the children.  The largest value always stays.
// Both rules give ONE scalar per row, the cut c = min z over the kept set; kept <=> i in A and z_i >= c.  The step's distribution is
// softmax(z) over the kept set; gradients treat the kept set as a constant (what autograd gives HF's masked_fill).
//   p5_trunc_cut            workgroup-wide: the cut of nc values z_at(i).  Top-k is the radix select of the wide search (integer histograms
//                           over order-preserving keys: comparisons only, exact).  Top-p bisects the 32-bit key space: the smallest key t with
//                           mass{ key > t } < top_p * mass(K1); every mass is summed in ONE fixed association (per-thread strided partials,
//                           wave_sum, four waves in index order), and a fixed-order fp32 sum of non-negative terms is monotone in each term,
//                           so the masses are monotone in t and the bisection is well defined: the cut is a pure function of the row's
//                           values and their order.
//   p5_trunc_sample_step_kernel   p5_sample_step_kernel's twin: the children's z once (the same dot products), the cut, then log-sum-exp and
//                                 Gumbel-max over the kept set.  The uniform of child i is the same function of (row key, i): truncation never
//                                 changes a child's noise.
//   p5_trunc_ce_fwd_kernel / p5_trunc_ce_bwd_kernel   p5_trie_ce's twins; a label that is allowed but below the cut is state 3 (truncated
//                                 away): nll 0 and no gradient for that row only.
// Every value has one writer and every reduction a fixed order: no float atomics, two runs return the same bits.
#pragma once
#include "p5_sample.h"
#include "p5_trie_ce.h"
#include "p5_decode_wide.h"

#define P5_TRIE_TRUNCATED 3
// Values staged in LDS per row (z and its softmax weight: 2 x 8 KiB).  With the select's histogram a workgroup holds 17.1 KiB, so the 160 KiB
// of a CU admit 9 workgroups -- more than the 8 that its 32 waves do: LDS never limits occupancy.  Wider nodes are read where they lie (the
// sampler's scratch row, the loss's logits row) and their weights are recomputed per pass (the same bits: expf of the same arguments).
#define P5_TRUNC_STAGE 2048

struct P5TruncLds {
  float z[P5_TRUNC_STAGE], e[P5_TRUNC_STAGE];
  int hist[256];
  int s_sel[4], s_w[4];
  float s_f[4];
};

// the 256 threads' sum in a fixed association: wave_sum, then the four waves in index order
__device__ static __forceinline__ float p5_trunc_block_sum(float v, float* s_f) {
  v = wave_sum(v);
  __syncthreads();                       // (the readers of the previous sum are done with s_f)
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_f[0] + s_f[1]) + s_f[2]) + s_f[3];
}
__device__ static __forceinline__ float p5_trunc_block_max(float v, float* s_f) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
}
// +0.0 and -0.0 are one value: both take +0.0's key (p5_wkey's rule)
__device__ static __forceinline__ unsigned p5_trunc_key(float z) { return p5_okey(z == 0.f ? 0.f : z); }

// The cut of the row's nc values z_at(i) (-inf = not in A), called by all 256 threads with uniform arguments; z_at must return the same
// bits every time it is asked.  top_k 0 = off, top_p >= 1 = off.  Returns min z over the kept set (+inf when A is empty); *kept_out its size.
template <class ZAt>
__device__ static float p5_trunc_cut(int nc, ZAt z_at, int top_k, float top_p, P5TruncLds& L, int* kept_out) {
  const int tid = threadIdx.x;
  float c = P5_NEG_INF;
  if (top_k > 0 && top_k < nc) {
    auto key_at = [&](int i) -> unsigned long long {
      const float z = z_at(i);
      return z == P5_NEG_INF ? 0ull : p5_wkey(z, (unsigned)i);
    };
    const unsigned long long thr = p5_wide_radix_select(nc, top_k, key_at, L.hist, L.s_sel, L.s_w);
    if (thr != 1ull) c = p5_okey_inv((unsigned)(thr >> 32));        // the k-th largest value (1: at most k values, all stay)
  }
  if (top_p < 1.f) {
    float mx = P5_NEG_INF;
    for (int i = tid; i < nc; i += 256) mx = fmaxf(mx, z_at(i));
    mx = p5_trunc_block_max(mx, L.s_f);
    if (mx != P5_NEG_INF) {                  // (uniform)
      const bool staged = nc <= P5_TRUNC_STAGE;
      auto w_at = [&](int i) -> float {
        const float z = z_at(i);
        return (z != P5_NEG_INF && z >= c) ? expf(z - mx) : 0.f;
      };
      if (staged) {
        for (int i = tid; i < nc; i += 256) L.e[i] = w_at(i);        // (a thread reads back only what it wrote)
      }
      float part = 0.f;
      for (int i = tid; i < nc; i += 256) part += staged ? L.e[i] : w_at(i);
      const float thr = top_p * p5_trunc_block_sum(part, L.s_f);
      // the smallest key hi with mass{ key > hi } < thr: the key of the largest value qualifies (mass 0 < thr), key 0 does not
      unsigned lo = 0u, hi = p5_trunc_key(mx);
      while (lo < hi) {                      // (uniform: every thread reads the same sums) at most 32 passes
        const unsigned mid = lo + ((hi - lo) >> 1);
        part = 0.f;
        for (int i = tid; i < nc; i += 256) {
          const float z = z_at(i);
          if (z != P5_NEG_INF && p5_trunc_key(z) > mid) part += staged ? L.e[i] : w_at(i);
        }
        const float above = p5_trunc_block_sum(part, L.s_f);
        if (above < thr) hi = mid; else lo = mid + 1u;
      }
      c = fmaxf(c, p5_okey_inv(hi));
    }
  }
  // the cut as the issue states it: min z over the kept set, and the set's size
  float mn = P5_NEG_INF;                     // max of -z
  int cnt = 0;
  for (int i = tid; i < nc; i += 256) {
    const float z = z_at(i);
    if (z != P5_NEG_INF && z >= c) { mn = fmaxf(mn, -z); ++cnt; }
  }
  mn = p5_trunc_block_max(mn, L.s_f);
  int total;
  p5_block_excl_scan(cnt, L.s_w, total);
  __syncthreads();                           // (s_w / s_f may be rewritten by the caller's next reduction)
  if (kept_out) *kept_out = total;
  return -mn;
}

// ---- sampling ----
// the z of the children [0, nc) of one decode row into zrow: p5_sample_step_kernel's dot products hn[row] . E[token] (8 lanes per child, 32
// children per pass, the same order of additions), z = acc * alpha / tau, -inf for an excluded child; lane 0 of a child's group writes
template <class T>
__device__ static __forceinline__ void p5_trunc_row_z(float* zrow, const P5SampleArgs& a, int r, int c0, int nc, const uint32_t* ex) {
  constexpr int EPF = TT<T>::EPF;
  constexpr int MAXP = 1024 / (8 * EPF);          // d_model <= 1024
  const int tid = threadIdx.x, d = a.d;
  const int grp = tid >> 3, sub = tid & 7;
  const T* hp = (const T*)a.hn + (size_t)r * d;
  const T* E = (const T*)a.E;
  const int np = d / (8 * EPF);
  u32x4 hx[MAXP];
#pragma unroll
  for (int k = 0; k < MAXP; ++k) hx[k] = k < np ? ld16(hp + sub * EPF + k * 8 * EPF) : zero16();
  int tok_next = grp < nc ? a.child_tok[c0 + grp] : 0;
  for (int i0 = 0; i0 < nc; i0 += 32) {
    const int i = i0 + grp;
    const int tok = tok_next;
    if (i + 32 < nc) tok_next = a.child_tok[c0 + i + 32];
    float acc = 0.f;
    if (i < nc) {
      const T* ep = E + (size_t)tok * d + sub * EPF;
      // (the 4 + MAXP tests against the row length are taken per pass: hoisted out of the loop they would sit in up to 68 scalar
      //  registers -- one lane mask each -- for the whole kernel, more than the fp32 instance has)
      int npl = np;
#ifndef P5_EMU
      asm volatile("" : "+s"(npl));
#endif
#pragma unroll
      for (int k0 = 0; k0 < MAXP; k0 += 8) {          // 8 x 16 bytes of the E row in flight per lane
        if (k0 < npl) {
          u32x4 wr[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) wr[k] = k0 + k < npl ? ld16(ep + (k0 + k) * 8 * EPF) : zero16();
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
      bool allowed = true;
      if (ex) {
        const int cn = a.child_node[c0 + i];
        allowed = !((ex[cn >> 5] >> (cn & 31)) & 1u);
      }
      zrow[i] = allowed ? acc * a.alpha / a.tau : P5_NEG_INF;
    }
  }
}

// one workgroup per decode row, after the decoder of the step.  zs: [R, max_c] fp32 scratch, used by rows of more than P5_TRUNC_STAGE children
template <class T>
__global__ __launch_bounds__(256) void p5_trunc_sample_step_kernel(P5SampleState st, P5SampleArgs a, float* __restrict__ zs, int top_k, float top_p) {
  __shared__ P5TruncLds L;
  __shared__ float sm[4], ss[4];
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ float s_z;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nd = st.node[r];
  if (nd < 0) return;            // finished (or nothing to draw): the row's state and its x32 row stay as they are
  const int c0 = a.child_off[nd];
  int nc = a.child_off[nd + 1] - c0;
  nc = nc < a.max_c ? nc : a.max_c;
  const int b = r / a.S;
  const uint32_t key = p5_sample_row_key(a.seed, a.stream_ids[b], a.draw_base + (uint32_t)(r - b * a.S), (uint32_t)a.cur_len);
  const uint32_t* ex = a.excluded ? a.excluded + (size_t)b * a.excl_words : nullptr;
  // pass 1: the children's z, read from E once
  float* zrow = nc <= P5_TRUNC_STAGE ? L.z : zs + (size_t)r * a.max_c;
  p5_trunc_row_z<T>(zrow, a, r, c0, nc, ex);
  __syncthreads();
  const float* zr = zrow;
  const float cut = p5_trunc_cut(nc, [&](int i) -> float { return zr[i]; }, top_k, top_p, L, nullptr);
  // pass 2 over the stored z: online (max, sum exp) and the best perturbed value over the kept set (ascending positions: a tie keeps the lowest)
  float m = P5_NEG_INF, sum = 0.f, bv = P5_NEG_INF, bz = 0.f;
  int bi = 0x7fffffff;
  for (int i = tid; i < nc; i += 256) {
    const float z = zr[i];
    if (z != P5_NEG_INF && z >= cut) {
      if (z > m) { sum = sum * expf(m - z) + 1.f; m = z; }
      else sum += expf(z - m);
      const float pv = z - logf(-logf(p5_sample_uniform(key, (uint32_t)i)));
      if (pv > bv) { bv = pv; bi = i; bz = z; }
    }
  }
  {
    const float wm_ = wave_max(m);
    sum = wave_sum(m == P5_NEG_INF ? 0.f : sum * expf(m - wm_));
    if (lane == 0) { sm[wave] = wm_; ss[wave] = sum; }
  }
  const int my_i = bi;
  block_argmax(bv, bi, s_val, s_idx);        // (its barriers publish sm / ss as well)
  if (bi == 0x7fffffff) {
    // no allowed child: a user whose whole catalogue is excluded
    if (tid == 0) {
      st.tok_lp[(size_t)r * a.max_len + a.cur_len] = P5_NEG_INF;
      st.sum_lp[r] = P5_NEG_INF;
      st.node[r] = -1;
    }
    return;
  }
  if (my_i == bi) s_z = bz;                  // (one thread owns a child)
  __syncthreads();
  const int tok = a.child_tok[c0 + bi];
  if (tid == 0) {
    const float mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    float tot = 0.f;
    for (int w = 0; w < 4; ++w) tot += (sm[w] == P5_NEG_INF) ? 0.f : ss[w] * expf(sm[w] - mx);
    const float lp = s_z - (mx + logf(tot));      // (one kept child: tot = 1, mx = its z: exactly 0)
    st.seq[(size_t)r * a.max_len + a.cur_len] = tok;
    st.tok_lp[(size_t)r * a.max_len + a.cur_len] = lp;
    st.sum_lp[r] += lp;
    const bool fin = tok == a.eos_id;
    st.node[r] = fin ? -1 : a.child_node[c0 + bi];
    if (fin) st.len[r] = a.cur_len;
    st.anc[(size_t)(a.cur_len - 1) * a.R + r] = r;      // this step's K/V entered the cache at position cur_len - 1, row r
  }
  // decoder input of the next step: x32[row, :] = E32[token, :]  (fp32 master table)
  const int d4 = st.d >> 2;
  for (int t = tid; t < d4; t += 256) *(f32x4*)(st.x32 + (size_t)r * st.d + t * 4) = *(const f32x4*)(st.E32 + (size_t)tok * st.d + t * 4);
}

// ---- item loss ----
struct P5TruncCe { int top_k; float top_p; };

// the z of child i of a row of the materialised logits: -inf for an excluded child
struct P5TruncGather {
  const float* lr; const int* tok; const int* cnode; const uint32_t* ex; float tau;
  const int* col;      // P5TrieCe::col at the node's first edge, or nullptr: column = token
  __device__ __forceinline__ float operator()(int i) const {
    if (ex) {
      const int cn = cnode[i];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) return P5_NEG_INF;
    }
    return lr[col ? col[i] : tok[i]] / tau;
  }
};

// the cut of a logits row at a trie node: the children's z gathered into LDS when they fit, read in place otherwise
__device__ static float p5_trunc_row_cut(const P5TruncGather& g, int nc, int top_k, float top_p, P5TruncLds& L, int* kept_out) {
  if (nc <= P5_TRUNC_STAGE) {
    for (int i = threadIdx.x; i < nc; i += 256) L.z[i] = g(i);
    __syncthreads();
    const float* zr = L.z;
    return p5_trunc_cut(nc, [&](int i) -> float { return zr[i]; }, top_k, top_p, L, kept_out);
  }
  return p5_trunc_cut(nc, g, top_k, top_p, L, kept_out);
}

// one workgroup per row: cut[row] and kept[row] of the row's node (node < 0: +inf and 0); rows_per_user rows share a row of the bitmap
__global__ __launch_bounds__(256) void p5_trunc_cut_kernel(float* __restrict__ cut, int* __restrict__ kept, const float* __restrict__ logits,
                                                          const int* __restrict__ node, P5TrieCe tr, P5TruncCe tc, int rows_per_user, int ldl) {
  __shared__ P5TruncLds L;
  const int row = blockIdx.x;
  const int nd = node[row];
  if (nd < 0) {
    if (threadIdx.x == 0) { cut[row] = __builtin_huge_valf(); kept[row] = 0; }
    return;
  }
  const int c0 = tr.child_off[nd], nc = tr.child_off[nd + 1] - c0;
  const P5TruncGather g{logits + (size_t)row * ldl, tr.child_tok + c0, tr.child_node + c0,
                        tr.excluded ? tr.excluded + (size_t)(row / rows_per_user) * tr.excl_words : nullptr, tr.tau,
                        tr.col ? tr.col + c0 : nullptr};
  int n = 0;
  const float c = p5_trunc_row_cut(g, nc, tc.top_k, tc.top_p, L, &n);
  if (threadIdx.x == 0) { cut[row] = c; kept[row] = n; }
}

// one workgroup per decoder row behind p5_trie_walk_kernel: row_cut, lse over the kept set, nll = lse - z[label]; a label below the cut turns
// the row's state (and state2's, the caller's copy) into P5_TRIE_TRUNCATED with nll 0.  Rows that are not scored: nll = lse = 0, cut = +inf.
template <class T>
__global__ __launch_bounds__(256) void p5_trunc_ce_fwd_kernel(float* __restrict__ nll, float* __restrict__ lse_out, float* __restrict__ row_cut,
                                                             int* __restrict__ state, int* __restrict__ state2, const float* __restrict__ logits,
                                                             const int64_t* __restrict__ labels, const int* __restrict__ node, P5TrieCe tr,
                                                             P5TruncCe tc, int Tlen, int ldl) {
  __shared__ P5TruncLds L;
  __shared__ float sm[4], ss[4];
  __shared__ float s_zl;
  const int row = blockIdx.x, tid = threadIdx.x;
  if (state[row] != P5_TRIE_SCORED) {
    if (tid == 0) { nll[row] = 0.f; lse_out[row] = 0.f; row_cut[row] = __builtin_huge_valf(); }
    return;
  }
  const int nd = node[row];
  const int c0 = tr.child_off[nd], nc = tr.child_off[nd + 1] - c0;
  const P5TruncGather g{logits + (size_t)row * ldl, tr.child_tok + c0, tr.child_node + c0,
                        p5_trie_excl_row(tr, row / Tlen), tr.tau,
                        tr.col ? tr.col + c0 : nullptr};
  const float cut = p5_trunc_row_cut(g, nc, tc.top_k, tc.top_p, L, nullptr);
  const bool staged = nc <= P5_TRUNC_STAGE;
  const int64_t lab = labels[row];
  float m = P5_NEG_INF, s = 0.f;
  for (int i = tid; i < nc; i += 256) {
    const float z = staged ? L.z[i] : g(i);
    if ((int64_t)g.tok[i] == lab) s_zl = z;      // (the walk found the label among the allowed children: exactly one thread)
    if (z == P5_NEG_INF || !(z >= cut)) continue;
    if (z > m) { s *= p5_exp<T>(m - z); m = z; }
    s += p5_exp<T>(z - m);
  }
  {
    const float wm_ = wave_max(m);
    s = wave_sum(m == P5_NEG_INF ? 0.f : s * p5_exp<T>(m - wm_));
    if ((tid & 63) == 0) { sm[tid >> 6] = wm_; ss[tid >> 6] = s; }
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    s = 0.f;
    for (int w = 0; w < 4; ++w) s += sm[w] == P5_NEG_INF ? 0.f : ss[w] * p5_exp<T>(sm[w] - m);
  }
  if (tid == 0) {
    const float lse = m + logf(s);
    const bool away = !(s_zl >= cut);
    row_cut[row] = cut;
    lse_out[row] = lse;
    nll[row] = away ? 0.f : lse - s_zl;
    if (away) {
      state[row] = P5_TRIE_TRUNCATED;
      if (state2) state2[row] = P5_TRIE_TRUNCATED;
    }
  }
}

// p5_trie_ce_bwd_kernel with the kept set of the forward: zero-fill, drain, barrier, then g * (exp(z - lse) - [child == label]) / tau only
// where z >= row_cut[row]
template <class T>
__global__ __launch_bounds__(256) void p5_trunc_ce_bwd_kernel(T* __restrict__ dlogits, const float* __restrict__ logits, const float* __restrict__ lse,
                                                             const float* __restrict__ row_cut, const int64_t* __restrict__ labels,
                                                             const int* __restrict__ node, const int* __restrict__ state,
                                                             const float* __restrict__ dnll, P5TrieCe tr, int ldl, int ldd,
                                                             const int64_t* __restrict__ out_attn, int Tlen, float gscale) {
  constexpr int EPF = TT<T>::EPF;
  const int row = blockIdx.x, tid = threadIdx.x;
  T* dr = dlogits + (size_t)row * ldd;
  for (int j = tid * EPF; j < ldd; j += 256 * EPF) st16(dr + j, zero16());      // (ldd is a multiple of 16 bytes: the head GEMM pads V to 64)
  if (state[row] != P5_TRIE_SCORED) return;
  float g;
  if (dnll) {
    g = dnll[row];
  } else {
    const int b = row / Tlen;
    float cnt = 0.f;
    for (int t = 0; t < Tlen; ++t) cnt += out_attn[(size_t)b * Tlen + t] != 0 ? 1.f : 0.f;
    g = out_attn[row] != 0 ? gscale / fmaxf(cnt, 1.f) : 0.f;
    if (tr.tw) g *= tr.tw[b];
  }
  P5_WAIT_VM(0);      // this wave's zero stores are acknowledged before anybody's child store leaves
  __syncthreads();
  const int nd = node[row];
  const int c0 = tr.child_off[nd], nc = tr.child_off[nd + 1] - c0;
  const uint32_t* ex = p5_trie_excl_row(tr, row / Tlen);
  const float* lr = logits + (size_t)row * ldl;
  const int64_t lab = labels[row];
  const float l = lse[row], cut = row_cut[row];
  for (int i = tid; i < nc; i += 256) {
    if (ex) {
      const int cn = tr.child_node[c0 + i];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) continue;
    }
    const int tok = tr.child_tok[c0 + i];
    const int col = tr.col ? tr.col[c0 + i] : tok;
    const float z = lr[col] / tr.tau;
    if (z == P5_NEG_INF || !(z >= cut)) continue;
    dr[col] = from_f<T>(g * (p5_exp<T>(z - l) - ((int64_t)tok == lab ? 1.f : 0.f)) / tr.tau);
  }
}
