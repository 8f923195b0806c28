// p5_sbs.h -- stochastic beam search on the item trie: slates of K DISTINCT items, a sample WITHOUT replacement from the model's
// distribution over the catalogue (Kool, van Hoof, Welling 2019: "Stochastic Beams and Where to Find Them").
//
// The distribution is that of p5_sample.h: p(item) = product along the item's path of softmax(z / tau) renormalised over the allowed
// children.  A slate is the K items with the largest G(item) = log p(item) + Gumbel noise, largest first, which is a sample without
// replacement in sequential-sampling (Plackett-Luce) order.  It is computed top-down so that only K prefixes are alive per step: a live beam
// S with log-probability phi_S and perturbed value G_S gives its allowed children
//     phi_i = phi_S + (z_i / tau - lse),     g_i = phi_i - log(-log u_i),     Z = max_i g_i  (ties: the lowest edge),
//     G~_argmax = G_S exactly,               G~_i = G_S - max(v, 0) - log1p(exp(-|v|)),  v = G_S - g_i + log1p(-exp(g_i - Z))
// (the stable form of -log(exp(-G_S) - exp(-Z) + exp(-g_i)): the children's maximum is conditioned to be the parent's value), and the
// beams of the next step are the K best of {children of live beams} U {finished beams, carried with their G~}.  The root has (0, 0).
// u_i = p5_sample_uniform(p5_sample_row_key(seed, stream, slate, step), GLOBAL CSR edge index of the child) -- p5_rng.h -- so G~ of a trie
// node is a pure function of (weights, input, seed, stream, slate index): independent of K, of the batch and of the beam slot the node
// occupies.  Candidate keys are (G~ desc, global edge index asc): unique in a tree-shaped trie, where an edge is reached by one prefix.
//
// Rows: R = B x S x K (S slates per user, K beams per slate); the decoder of the step is that of the sampling path (decode_step2 without
// its head, cross-attention K/V shared by the S x K rows of a user).  Behind it, per step:
//   p5_sbs_row_kernel      one workgroup per row: children's logits hn . E[token] (8 lanes per child), log-sum-exp of the allowed ones,
//                          g_i, Z, G~_i into the [R, max_c] scratch (Z must be known before any G~_i), the row's best min(nc, K)
//                          candidates as 64-bit keys (p5_wide_row_emit); a finished row emits its own carried key, a dead row nothing
//   p5_sbs_select_kernel   one workgroup per slate: exact top-K of the slate's pool, sorted (radix select over integer histograms,
//                          compaction, bitonic sort: no result depends on the order atomics land in); the owner of each winning edge
//                          is found in a table of the rows' edge ranges sorted in LDS; writes parent, edge, token, node, phi, G~, log-prob
//   p5_sbs_commit_kernel   rows change places: gathers the parent's sequence and per-position log-probabilities, rebuilds the ancestry
//                          column of the step KV cache (two tables, as p5_wide_commit_kernel), writes the next step's x32 rows
// Dead rows (fewer candidates than K) hold the pad embedding in x32 from the init kernel on and run the decoder like any other row: their
// K/V are written and never referenced.  No early stop, nothing read back, one writer per value: two calls return the same bits.
#pragma once
#include "p5_decode_wide.h"
#include "p5_rng.h"

#define P5_SBS_MAX_K P5_WIDE_MAX_K
#define P5_SBS_COMMIT_ROWS 16          // rows per workgroup of p5_sbs_commit_kernel
#define P5_SBS_DEAD (-2)               // node of a beam slot without a candidate (-1: finished)

struct P5SbsState {
  int *seq, *seq_next;             // [R, max_len] pad-filled, decoder start first (the host swaps the pair after every step)
  float *tok_lp, *tok_lp_next;     // [R, max_len] log-probability of the token at each position
  float *phi, *G;                  // [R] log-probability and perturbed value of the beam (-inf: dead)
  int* node;                       // [R] trie node behind the beam's prefix; -1 finished, P5_SBS_DEAD no beam in this slot
  int* edge;                       // [R] global CSR edge that led to the beam: the low word of a carried beam's key
  int* len;                        // [R] generated tokens of a finished beam, </s> included
  int *anc, *anc_next;             // [max_len, R] x 2: a step with odd cur_len reads `anc`, one with even cur_len `anc_next`
  int* steps;                      // [max_len + 1] steps[i] = i
  int* flags;                      // [8] the decode kernels' done flag is flags[4]: stays 0
  float* x32;                      // [R, d]
  const float* E32;
  int d;
  // scratch of one step
  float* lp;                       // [R, max_c] z_i / tau of every child, then its token log-probability (-inf: not allowed)
  float* gt;                       // [R, max_c] g_i, then G~_i (-inf: not allowed)
  unsigned long long* row_key;     // [R, C] C = min(max_c, K)
  int* row_n;                      // [R]
  int *sel_parent, *sel_tok, *sel_node, *sel_edge, *sel_len;     // [R] the beams of the next step: parent row (-1: none), new token (-1:
  float *sel_phi, *sel_G, *sel_lp;                               //     carried or none), node, edge, length, phi, G~, token log-probability
};

struct P5SbsArgs {
  const void* hn; const void* E; int d; float alpha, tau;
  const int* child_off; const int* child_tok; const int* child_node;
  const uint32_t* excluded; int excl_words;
  int S, K, R, max_c, C, max_len, cur_len, eos_id, pad_id, start_id, F;
  uint32_t seed; const uint32_t* stream_ids; uint32_t slate_base;
};

// beam 0 of every slate at the start node (or at the end of the forced prefix f_1 .. f_F) with (phi, G) = (0, 0), the others dead; both
// ancestry tables: positions below F map to the user's first row, the others to the row itself
__global__ __launch_bounds__(256) void p5_sbs_init_kernel(P5SbsState st, P5Forced ff, const int* __restrict__ child_off,
                                                         const int* __restrict__ child_tok, const int* __restrict__ child_node, int B, int S, int K,
                                                         int max_len, int start_id, int pad_id) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int R = B * S * K, F = ff.n;
  if (i < R * max_len) {
    const int p = i % max_len, row = i / max_len;
    const bool first = (row % K) == 0;
    const int v = (p == 0) ? start_id : ((first && p <= F) ? ff.tok[p - 1] : pad_id);
    st.seq[i] = v; st.seq_next[i] = v;
    st.tok_lp[i] = 0.f; st.tok_lp_next[i] = 0.f;
    const int pp = i / R, r = i % R;           // the ancestry tables are [position][row]
    const int a = pp < F ? (r / (S * K)) * (S * K) : r;
    st.anc[i] = a; st.anc_next[i] = a;
  }
  if (i < R) {
    int nd = -1;
    if (F > 0) nd = ff.node[F - 1];
    else
      for (int c = child_off[0]; c < child_off[1]; ++c)
        if (child_tok[c] == start_id) nd = child_node[c];
    const bool live = (i % K) == 0 && nd >= 0;
    st.node[i] = live ? nd : P5_SBS_DEAD;
    st.phi[i] = live ? 0.f : P5_NEG_INF;
    st.G[i] = live ? 0.f : P5_NEG_INF;
    st.edge[i] = 0;
    st.len[i] = 0;
  }
  {
    const int last = F > 0 ? ff.tok[F - 1] : start_id;
    const int d4 = st.d >> 2;
    for (int t = i; t < R * d4; t += gridDim.x * 256) {
      const int row = t / d4;
      const int tok = (row % K) == 0 ? last : pad_id;
      *(f32x4*)(st.x32 + (size_t)t * 4) = *(const f32x4*)(st.E32 + (size_t)tok * st.d + (t % d4) * 4);
    }
  }
  if (i <= max_len) st.steps[i] = i;
  if (i < 8) st.flags[i] = 0;
}

// ---- a. one workgroup per decode row, after the decoder of the step (decode_step2 without its head) ----
template <class T>
__global__ __launch_bounds__(256) void p5_sbs_row_kernel(P5SbsState st, P5SbsArgs a) {
  constexpr int EPF = TT<T>::EPF;
  __shared__ float sm[4], ss[4];
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ int hist[256];
  __shared__ int s_sel[4], s_w[4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nd = st.node[r];
  if (nd == P5_SBS_DEAD) {            // (uniform per block)
    if (tid == 0) st.row_n[r] = 0;
    return;
  }
  if (nd < 0) {                       // finished: carried with its own key
    if (tid == 0) {
      st.row_key[(size_t)r * a.C] = p5_wkey(st.G[r], (unsigned)st.edge[r]);
      st.row_n[r] = 1;
    }
    return;
  }
  const int c0 = a.child_off[nd];
  int nc = a.child_off[nd + 1] - c0;
  nc = nc < a.max_c ? nc : a.max_c;
  const int rows_per_user = a.S * a.K;
  const int b = r / rows_per_user, d = a.d;
  const uint32_t key = p5_sample_row_key(a.seed, a.stream_ids[b], a.slate_base + (uint32_t)((r - b * rows_per_user) / a.K), (uint32_t)a.cur_len);
  const uint32_t* ex = a.excluded ? a.excluded + (size_t)b * a.excl_words : nullptr;
  float* lpz = st.lp + (size_t)r * a.max_c;
  float* gt = st.gt + (size_t)r * a.max_c;
  const float phi_s = st.phi[r], G_s = st.G[r];
  // pass 1: z_i / tau of every child into the scratch (-inf: excluded), online (max, sum exp) over the allowed ones
  float m = P5_NEG_INF, sum = 0.f;
  {
    // 8 lanes per child, 32 children per pass; the row's hn stays in registers (p5_sample_step_kernel's layout)
    constexpr int MAXP = 1024 / (8 * EPF);          // d_model <= 1024
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
#pragma unroll
        for (int k0 = 0; k0 < MAXP; k0 += 8) {          // 8 x 16 bytes of the E row in flight per lane
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
        bool allowed = true;
        if (ex) {
          const int cn = a.child_node[c0 + i];
          allowed = !((ex[cn >> 5] >> (cn & 31)) & 1u);
        }
        float z = P5_NEG_INF;
        if (allowed) {
          z = acc * a.alpha / a.tau;
          if (z > m) { sum = sum * expf(m - z) + 1.f; m = z; }
          else sum += expf(z - m);
        }
        lpz[i] = z;
      }
    }
  }
  {
    const float wm_ = wave_max(m);
    sum = wave_sum(m == P5_NEG_INF ? 0.f : sum * expf(m - wm_));
    if (lane == 0) { sm[wave] = wm_; ss[wave] = sum; }
  }
  __syncthreads();                     // (publishes sm / ss and the scratch row)
  const float mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  if (mx == P5_NEG_INF) {              // no allowed child (uniform): the beam ends here without a candidate
    if (tid == 0) st.row_n[r] = 0;
    return;
  }
  float tot = 0.f;
  for (int w = 0; w < 4; ++w) tot += (sm[w] == P5_NEG_INF) ? 0.f : ss[w] * expf(sm[w] - mx);
  const float lse = mx + logf(tot);
  // pass 2: token log-probability, phi_i, g_i; Z = max g_i with the lowest edge on a tie (a thread's children ascend)
  float bv = P5_NEG_INF;
  int bi = 0x7fffffff;
  for (int i = tid; i < nc; i += 256) {
    const float z = lpz[i];
    float g = P5_NEG_INF;
    if (z != P5_NEG_INF) {
      const float lp = z - lse;
      lpz[i] = lp;
      const float phi_i = phi_s + lp;
      g = phi_i - logf(-logf(p5_sample_uniform(key, (uint32_t)(c0 + i))));
      if (g > bv) { bv = g; bi = i; }
    }
    gt[i] = g;
  }
  block_argmax(bv, bi, s_val, s_idx);
  const float Z = bv;
  // pass 3: G~_i (the same thread owns child i in passes 2 and 3)
  for (int i = tid; i < nc; i += 256) {
    const float g = gt[i];
    if (i == bi) gt[i] = G_s;
    else if (g != P5_NEG_INF) {
      const float v = G_s - g + log1pf(-expf(g - Z));
      gt[i] = G_s - fmaxf(v, 0.f) - log1pf(expf(-fabsf(v)));
    }
  }
  __syncthreads();
  // keys (G~ desc, global edge c0 + i asc): p5_wide_row_emit forms the low word as j * max_c + i
  p5_wide_row_emit(st.row_key, st.row_n, gt, r, c0, nc, a.C, 1, hist, s_sel, s_w);
}

// ---- b. one workgroup per slate: exact top-K of the slate's pool, sorted; the beams of the next step ----
__global__ __launch_bounds__(256) void p5_sbs_select_kernel(P5SbsState st, P5SbsArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_key[P5_SBS_MAX_K];     // 32 KiB
  __shared__ __attribute__((aligned(16))) unsigned long long s_tab[P5_SBS_MAX_K];     // 32 KiB: (first edge + 1) << 32 | slot << 1 | finished
  __shared__ int hist[256];
  __shared__ int s_sel[4], s_w[4];
  const int sl = blockIdx.x, tid = threadIdx.x, K = a.K, C = a.C;
  const int r0 = sl * K;
  // the rows' edge ranges, descending by first edge: a live row owns [child_off[node], child_off[node + 1]), a finished one the edge that
  // led to it (never inside a live row's range: its parent is no longer a beam).  Root edges (first edge 0) belong to no beam.
  const int kp = p5_pow2_ceil(K);
  for (int j = tid; j < kp; j += 256) {
    unsigned long long t = 0ull;
    if (j < K) {
      const int nd = st.node[r0 + j];
      if (nd >= 0) t = ((unsigned long long)((unsigned)a.child_off[nd] + 1u) << 32) | ((unsigned long long)j << 1);
      else if (nd == -1) t = ((unsigned long long)((unsigned)st.edge[r0 + j] + 1u) << 32) | ((unsigned long long)j << 1) | 1ull;
    }
    s_tab[j] = t;
  }
  __syncthreads();
  p5_wide_sort_desc(s_tab, kp);
  const int n = K * C;
  auto key_at = [&](int t) -> unsigned long long {
    const int j = t / C, i = t - j * C;
    return i < st.row_n[r0 + j] ? st.row_key[(size_t)(r0 + j) * C + i] : 0ull;
  };
  const unsigned long long thr = p5_wide_radix_select(n, K, key_at, hist, s_sel, s_w);
  if (tid == 0) s_sel[2] = 0;
  __syncthreads();
  for (int t = tid; t < n; t += 256) {          // compaction: positions depend on the atomics' order, the sort below removes it
    const unsigned long long k = key_at(t);
    if (k != 0ull && k >= thr) s_key[atomicAdd(&s_sel[2], 1)] = k;
  }
  __syncthreads();
  const int cnt = s_sel[2];                      // == min(K, candidates)
  const int np = p5_pow2_ceil(cnt > 1 ? cnt : 1);
  for (int i = cnt + tid; i < np; i += 256) s_key[i] = 0ull;
  __syncthreads();
  p5_wide_sort_desc(s_key, np);
  for (int q = tid; q < K; q += 256) {
    int parent = -1, tok = -1, nd = P5_SBS_DEAD, edge = 0, len = 0;
    float phi = P5_NEG_INF, G = P5_NEG_INF, lp = 0.f;
    if (q < cnt) {
      const unsigned long long k = s_key[q];
      G = p5_okey_inv((unsigned)(k >> 32));
      const unsigned e = ~(unsigned)k;
      edge = (int)e;
      int lo = 0, hi = kp - 1;                   // first table entry with first edge <= e (one exists: the edge's owner)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)(s_tab[mid] >> 32) > e + 1u) lo = mid + 1; else hi = mid;
      }
      const unsigned long long t = s_tab[lo];
      const int j = (int)(((unsigned)t) >> 1);
      parent = r0 + j;
      const int i = (int)(e + 1u - (unsigned)(t >> 32));
      if (t & 1ull) {                            // a finished beam, carried
        nd = -1; phi = st.phi[parent]; len = st.len[parent];
      } else if ((unsigned)i >= (unsigned)a.max_c) {      // (cannot happen in a tree-shaped trie: an edge without an owner leaves the slot empty)
        parent = -1; G = P5_NEG_INF; edge = 0;
      } else {
        lp = st.lp[(size_t)parent * a.max_c + i];
        phi = st.phi[parent] + lp;
        tok = a.child_tok[e];
        const bool fin = tok == a.eos_id;
        nd = fin ? -1 : a.child_node[e];
        len = fin ? a.cur_len : 0;
      }
    }
    const int r = r0 + q;
    st.sel_parent[r] = parent; st.sel_tok[r] = tok; st.sel_node[r] = nd; st.sel_edge[r] = edge; st.sel_len[r] = len;
    st.sel_phi[r] = phi; st.sel_G[r] = G; st.sel_lp[r] = lp;
  }
}

// ---- c. P5_SBS_COMMIT_ROWS rows per workgroup: the next step's sequences, log-probabilities, ancestry, x32 rows and row state ----
// anc_src: the table the decoder of this step read; anc_dst: the one the next step reads
__global__ __launch_bounds__(256) void p5_sbs_commit_kernel(P5SbsState st, P5SbsArgs a, const int* __restrict__ anc_src, int* __restrict__ anc_dst) {
  const int tid = threadIdx.x, R = a.R, max_len = a.max_len, cur_len = a.cur_len;
  const int q0 = blockIdx.x * P5_SBS_COMMIT_ROWS;
  const int nb = (R - q0) < P5_SBS_COMMIT_ROWS ? (R - q0) : P5_SBS_COMMIT_ROWS;
  for (int t = tid; t < nb * max_len; t += 256) {
    const int r = q0 + t / max_len, p = t % max_len;
    const int parent = st.sel_parent[r], tok = st.sel_tok[r];
    int v = (p == 0) ? a.start_id : a.pad_id;
    float l = 0.f;
    if (parent >= 0) {
      v = st.seq[(size_t)parent * max_len + p];
      l = st.tok_lp[(size_t)parent * max_len + p];
      if (tok >= 0 && p == cur_len) { v = tok; l = st.sel_lp[r]; }
    }
    st.seq_next[(size_t)r * max_len + p] = v;
    st.tok_lp_next[(size_t)r * max_len + p] = l;
  }
  const int pos = cur_len - 1;   // K/V of this step were stored at `pos` by the parent's row; a slot without a beam keeps its own column
  for (int t = tid; t < nb * (pos + 1); t += 256) {
    const int r = q0 + t / (pos + 1), p = t % (pos + 1);
    int parent = st.sel_parent[r];
    if (parent < 0) parent = r;
    anc_dst[(size_t)p * R + r] = (p == pos) ? parent : anc_src[(size_t)p * R + parent];
  }
  {      // decoder input of the next step: x32[row, :] = E32[token, :]; </s> for a carried beam, pad for a slot without one (finite rows)
    const int d4 = st.d >> 2, n4 = nb * d4;
    for (int t = tid; t < n4; t += 256) {
      const int r = q0 + t / d4, c4 = t % d4;
      const int tok = st.sel_tok[r];
      const int in_tok = tok >= 0 ? tok : (st.sel_parent[r] >= 0 ? a.eos_id : a.pad_id);
      *(f32x4*)(st.x32 + (size_t)r * st.d + c4 * 4) = *(const f32x4*)(st.E32 + (size_t)in_tok * st.d + c4 * 4);
    }
  }
  for (int t = tid; t < nb; t += 256) {
    const int r = q0 + t;
    st.node[r] = st.sel_node[r]; st.edge[r] = st.sel_edge[r]; st.len[r] = st.sel_len[r];
    st.phi[r] = st.sel_phi[r]; st.G[r] = st.sel_G[r];
  }
}

__global__ __launch_bounds__(256) void p5_sbs_finish_kernel(int* __restrict__ out_seq, float* __restrict__ out_logprob, float* __restrict__ out_perturbed,
                                                           float* __restrict__ out_tok_logprob, int* __restrict__ out_len, P5SbsState st, int R,
                                                           int max_len) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < R * max_len) { out_seq[i] = st.seq[i]; out_tok_logprob[i] = st.tok_lp[i]; }
  if (i < R) {
    const bool fin = st.node[i] == -1;       // a beam that did not reach </s> within max_len is no item
    out_logprob[i] = st.phi[i]; out_perturbed[i] = st.G[i]; out_len[i] = fin ? st.len[i] : 0;
  }
}
