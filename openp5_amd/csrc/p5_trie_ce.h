// p5_trie_ce.h -- trie-normalised TRAINING loss: the negative log-likelihood (and its gradient) of the distribution that p5_sample.h draws from.
//
// p(item) = product over the item's path of softmax(z / tau) RENORMALISED over the allowed children of the prefix's trie node (a child whose
// node bit is set in the user's excluded-node bitmap is not allowed).  The full-vocabulary cross-entropy of p5_elem.h is the likelihood of a
// different distribution: its score function is not the gradient of the log-probabilities the samplers report.  Three kernels:
//   p5_trie_walk_kernel     labels [B, T] -> the trie node behind labels[b, :t] and a state per decoder row
//                             0 scored        the label is an allowed child of the node
//                             1 past the end  behind </s>, at a node without children, at label -100 and every row after it
//                             2 off the trie  the label is no child of the node or an excluded one; every later row of the sample as well
//   p5_trie_ce_fwd_kernel   per scored row: lse = log sum_allowed exp(z), nll = lse - z[label], z = logit / tau, from the node's children only
//                           (nc reads of the materialised fp32 logits row, not V); rows of state 1 / 2: nll = lse = 0
//   p5_trie_ce_bwd_kernel   the DENSE dlogits row: zero everywhere except g * (exp(z - lse) - [child == label]) / tau at the allowed children, so
//                           that the tied head's weight gradient and its split-K input gradient run unchanged behind it
// Every value has one writer and every reduction a fixed order: no atomics, two runs return the same bits.
// P5TrieCe::col (optional, one int per CSR edge): the head restricted to the trie's tokens (p5_item_head.h).  The logits row and the dlogits row
// are then COMPACT -- [rows, Nup] over the sorted distinct tokens of the trie -- and a child's logit / gradient sits at column col[edge] instead of
// column child_tok[edge].  Nothing else changes: labels, the walk and the exclusion bitmap stay on tokens and nodes, the arithmetic per child
// and the order of reduction are the same, so on equal logits nll, lse and the entries of dlogits are equal bit for bit.  nullptr = the dense row.
// Not there, either way: per-user roots; exclusion on a grafted trie (the Python layer raises).
#pragma once
#include "p5_elem.h"

#define P5_TRIE_SCORED 0
#define P5_TRIE_PAST_END 1
#define P5_TRIE_OFF 2

struct P5TrieCe {
  const int* child_off; const int* child_tok; const int* child_node;
  const uint32_t* excluded; int excl_words;      // [B, excl_words] bitmap over trie nodes, or nullptr
  float tau;
  const int* col;      // [n_edges] column of an edge's token in a compact logits row (p5_item_head.h), or nullptr: column = token
  int group;           // samples per user (several targets per user: p5_forward_targets); the bitmap row of sample s is s / group.  0 = 1
  const float* tw;     // [samples] weight of a sample in the seeded masked-mean loss (p5_forward_loss_targets), or nullptr = 1
};
// the excluded-node bitmap row of a sample
__device__ __forceinline__ const uint32_t* p5_trie_excl_row(const P5TrieCe& tr, int sample) {
  if (!tr.excluded) return nullptr;
  return tr.excluded + (size_t)(tr.group > 1 ? sample / tr.group : sample) * tr.excl_words;
}

// one workgroup per sample: the positions are walked in order, the 256 threads look the label up among the node's children.
// node[b * T + t]: the node whose children row (b, t) normalises over; -1 behind </s> and behind the row that ended the walk.
// state2: optional second copy of the states for the caller (each array has one writer per element: thread 0 of the sample's workgroup)
__global__ __launch_bounds__(256) void p5_trie_walk_kernel(int* __restrict__ node, int* __restrict__ state, int* __restrict__ state2,
                                                          const int64_t* __restrict__ labels, P5TrieCe tr, int T, int start_id, int eos_id) {
  __shared__ int s_hit[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* ex = p5_trie_excl_row(tr, b);
  int nd = -1;
  for (int c = tr.child_off[0]; c < tr.child_off[1]; ++c)      // p5_sample_init_kernel's start node
    if (tr.child_tok[c] == start_id) nd = tr.child_node[c];
  int dead = nd < 0 ? P5_TRIE_OFF : 0;      // (a trie without the decoder-start edge scores nothing)
  for (int t = 0; t < T; ++t) {
    const size_t row = (size_t)b * T + t;
    int st = dead, cur = nd;
    if (!dead) {
      const int64_t lab = labels[row];
      const int c0 = tr.child_off[nd], nc = tr.child_off[nd + 1] - c0;
      if (lab == -100 || nc <= 0) {
        st = dead = P5_TRIE_PAST_END;
        nd = -1;
      } else {
        // (child tokens of a node are distinct: at most one thread writes; the two slots alternate so that the reset of the next position
        //  cannot overtake a read of this one)
        int* hit = s_hit + (t & 1);
        if (tid == 0) *hit = -1;
        __syncthreads();
        for (int i = tid; i < nc; i += 256)
          if ((int64_t)tr.child_tok[c0 + i] == lab) *hit = i;
        __syncthreads();
        const int h = *hit;
        bool ok = h >= 0;
        int cn = -1;
        if (ok) {
          cn = tr.child_node[c0 + h];
          if (ex && ((ex[cn >> 5] >> (cn & 31)) & 1u)) ok = false;
        }
        if (!ok) {
          st = dead = P5_TRIE_OFF;
          nd = -1;
        } else if (lab == (int64_t)eos_id) {
          dead = P5_TRIE_PAST_END;        // this row is scored; the rows behind </s> are not
          nd = -1;
        } else {
          nd = cn;
        }
      }
    }
    if (tid == 0) {
      node[row] = cur;
      state[row] = st;
      if (state2) state2[row] = st;
    }
  }
}

// one workgroup per decoder row; the running (max, sum exp) merge of p5_ce_fwd_kernel over the allowed children
template <class T>
__global__ __launch_bounds__(256) void p5_trie_ce_fwd_kernel(float* __restrict__ nll, float* __restrict__ lse_out, const float* __restrict__ logits,
                                                            const int64_t* __restrict__ labels, const int* __restrict__ node,
                                                            const int* __restrict__ state, P5TrieCe tr, int Tlen, int ldl) {
  __shared__ float sm[4], ss[4];
  __shared__ float s_zl;
  const int row = blockIdx.x, tid = threadIdx.x;
  if (state[row] != P5_TRIE_SCORED) {
    if (tid == 0) { nll[row] = 0.f; lse_out[row] = 0.f; }
    return;
  }
  const int nd = node[row];
  const int c0 = tr.child_off[nd], nc = tr.child_off[nd + 1] - c0;
  const uint32_t* ex = p5_trie_excl_row(tr, row / Tlen);
  const float* lr = logits + (size_t)row * ldl;
  const int64_t lab = labels[row];
  float m = P5_NEG_INF, s = 0.f;
  for (int i = tid; i < nc; i += 256) {
    if (ex) {
      const int cn = tr.child_node[c0 + i];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) continue;
    }
    const int tok = tr.child_tok[c0 + i];
    const float z = lr[tr.col ? tr.col[c0 + i] : tok] / tr.tau;
    if ((int64_t)tok == lab) s_zl = z;      // (the walk found the label among the allowed children: exactly one thread)
    if (z == P5_NEG_INF) continue;          // a masked logit adds nothing; while m is still -inf, exp(-inf - m) would be NaN and stay in s
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
    lse_out[row] = lse;
    nll[row] = lse - s_zl;
  }
}

// one workgroup per decoder row: the row is zero-filled with 16-byte stores, then -- behind a drain of those stores and a workgroup barrier,
// the same addresses are written twice -- the allowed children get their entries (one 2- or 4-byte store each).
// g: p5_ce_bwd_kernel's two rules (dnll from autograd, or the masked-mean seed from the label mask), 0 for rows that are not scored.
template <class T>
__global__ __launch_bounds__(256) void p5_trie_ce_bwd_kernel(T* __restrict__ dlogits, const float* __restrict__ logits, const float* __restrict__ lse,
                                                            const int64_t* __restrict__ labels, const int* __restrict__ node,
                                                            const int* __restrict__ state, const float* __restrict__ dnll, P5TrieCe tr, int ldl, int ldd,
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
  const float l = lse[row];
  for (int i = tid; i < nc; i += 256) {
    if (ex) {
      const int cn = tr.child_node[c0 + i];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) continue;
    }
    const int tok = tr.child_tok[c0 + i];
    const int col = tr.col ? tr.col[c0 + i] : tok;
    const float z = lr[col] / tr.tau;
    dr[col] = from_f<T>(g * (p5_exp<T>(z - l) - ((int64_t)tok == lab ? 1.f : 0.f)) / tr.tau);
  }
}
