// p5_sample.h -- trie-constrained SAMPLING: draw items from the model's distribution over the catalogue.
//
// HF's sampling path applies the logits processors and then takes softmax, so under a PrefixConstrainedLogitsProcessor the distribution
// of a step is renormalised over the allowed children of the row's trie node (the beam path takes log_softmax over the full vocabulary
// first: that is what p5_head_lse_kernel is for).  A sampling step therefore needs no pass over the vocabulary: the decoder of
// p5_decode2.h runs for R = B x S independent rows (S draws per user), stops behind its final T5LayerNorm, and ONE launch per step
//   - recomputes the logits of the node's children as dot products hn[row] . E[token] (the layout of p5_dec_score2_kernel),
//   - draws one child by Gumbel-max over z_i / tau + g_i, g_i = -logf(-logf(u_i)), u_i from the counter-based hash of p5_rng.h,
//   - reduces log sum_allowed exp(z_i / tau) online in the same pass: the drawn token's log-probability is z_c / tau - lse,
//   - advances the row: token, log-probability, trie node, the next step's input embedding.
// Rows never change places, so the ancestry table of the step KV cache is the identity behind the forced prefix (whose K/V the
// teacher-forced pass of p5_decode.h left at the user's first row).  Every value has one writer: no atomics, results are a pure function
// of (weights, inputs, seed, stream id, draw index) -- the same whatever the batch a user is drawn in.
#pragma once
#include "p5_decode.h"
#include "p5_rng.h"

struct P5SampleState {
  int* seq;            // [R, max_len] pad-filled, decoder start first
  float* tok_lp;       // [R, max_len] log-probability of the token at each position (position 0 and forced positions: 0)
  float* sum_lp;       // [R] their running sum, in step order
  int* node;           // [R] trie node behind the row's prefix; -1 = finished (or nothing to draw)
  int* len;            // [R] generated tokens of a finished row, </s> included; 0 while the row runs
  int* anc;            // [max_len, R] ancestry of the step KV cache
  int* steps;          // [max_len + 1] steps[i] = i: the decoder kernels read cur_len through a device pointer
  int* flags;          // [8] the decode kernels' done flag is flags[4]: stays 0, every draw runs to its leaf
  float* x32;          // [R, d] fp32 residual stream: the step writes the next step's input embeddings E32[token]
  const float* E32;
  int d;
};

struct P5SampleArgs {
  const void* hn; const void* E; int d; float alpha, tau;
  const int* child_off; const int* child_tok; const int* child_node;
  const uint32_t* excluded; int excl_words;
  int S, R, max_c, max_len, cur_len, eos_id;
  uint32_t seed; const uint32_t* stream_ids; uint32_t draw_base;
};

// every row of a user at the start node (or at the end of the forced prefix f_1 .. f_F); ancestry: positions below F map to the user's
// first row, the others to the row itself
__global__ __launch_bounds__(256) void p5_sample_init_kernel(P5SampleState st, P5Forced ff, const int* __restrict__ child_off,
                                                            const int* __restrict__ child_tok, const int* __restrict__ child_node, int B, int S,
                                                            int max_len, int start_id, int pad_id) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int R = B * S, F = ff.n;
  if (i < R * max_len) {
    const int p = i % max_len;
    st.seq[i] = (p == 0) ? start_id : (p <= F ? ff.tok[p - 1] : pad_id);
    st.tok_lp[i] = 0.f;
    const int pp = i / R, r = i % R;           // the ancestry table is [position][row]
    st.anc[i] = pp < F ? (r / S) * S : r;
  }
  if (i < R) {
    int nd = -1;
    if (F > 0) nd = ff.node[F - 1];
    else
      for (int c = child_off[0]; c < child_off[1]; ++c)
        if (child_tok[c] == start_id) nd = child_node[c];
    st.node[i] = nd;
    st.sum_lp[i] = 0.f;
    st.len[i] = 0;
  }
  {
    const int last = F > 0 ? ff.tok[F - 1] : start_id;
    const int d4 = st.d >> 2;
    for (int t = i; t < R * d4; t += gridDim.x * 256)
      *(f32x4*)(st.x32 + (size_t)t * 4) = *(const f32x4*)(st.E32 + (size_t)last * st.d + (t % d4) * 4);
  }
  if (i <= max_len) st.steps[i] = i;
  if (i < 8) st.flags[i] = 0;
}

// one workgroup per decode row, after the decoder of the step (decode_step2 without its head)
template <class T>
__global__ __launch_bounds__(256) void p5_sample_step_kernel(P5SampleState st, P5SampleArgs a) {
  constexpr int EPF = TT<T>::EPF;
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
  const int b = r / a.S, d = a.d;
  const uint32_t key = p5_sample_row_key(a.seed, a.stream_ids[b], a.draw_base + (uint32_t)(r - b * a.S), (uint32_t)a.cur_len);
  const uint32_t* ex = a.excluded ? a.excluded + (size_t)b * a.excl_words : nullptr;
  // this lane's children: online (max, sum exp) of z / tau, and the best perturbed value with its child (ascending positions: a tie
  // keeps the lowest)
  float m = P5_NEG_INF, sum = 0.f, bv = P5_NEG_INF, bz = 0.f;
  int bi = 0x7fffffff;
  {
    // 8 lanes per child, 32 children per pass; the row's hn stays in registers (p5_dec_score2_kernel's layout)
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
        if (allowed) {
          const float z = acc * a.alpha / a.tau;
          if (z > m) { sum = sum * expf(m - z) + 1.f; m = z; }
          else sum += expf(z - m);
          const float pv = z - logf(-logf(p5_sample_uniform(key, (uint32_t)i)));
          if (pv > bv) { bv = pv; bi = i; bz = z; }
        }
      }
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
  if (my_i == bi) s_z = bz;                  // (one lane owns a child)
  __syncthreads();
  const int tok = a.child_tok[c0 + bi];
  if (tid == 0) {
    const float mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    float tot = 0.f;
    for (int w = 0; w < 4; ++w) tot += (sm[w] == P5_NEG_INF) ? 0.f : ss[w] * expf(sm[w] - mx);
    const float lp = s_z - (mx + logf(tot));
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

__global__ __launch_bounds__(256) void p5_sample_finish_kernel(int* __restrict__ out_seq, float* __restrict__ out_logprob,
                                                              float* __restrict__ out_tok_logprob, int* __restrict__ out_len, P5SampleState st,
                                                              int R, int max_len) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < R * max_len) { out_seq[i] = st.seq[i]; out_tok_logprob[i] = st.tok_lp[i]; }
  if (i < R) { out_logprob[i] = st.sum_lp[i]; out_len[i] = st.len[i]; }
}
