// p5_trie_reg.h -- the item loss of p5_trie_ce.h with two exact per-row regularisers of the policy: the ENTROPY of a row's child distribution
// and its KL divergence from a frozen reference model's child distribution over the same children.
//
// For a scored row at trie node n, A = the children of n that are not excluded for the row's user and whose own logit is finite (the set
// p5_trie_ce_fwd_kernel normalises over), z_i = logit_i / tau, zr_i = ref_logit_i / tau (the same tau), m = max_A z, s = sum_A exp(z_i - m),
// p_i = exp(z_i - m) / s, and m_ref, s_ref, q_i the same from zr over the SAME set A:
//   H  = -sum_A p_i log p_i        = log s - (sum_A exp(z_i - m) (z_i - m)) / s
//   KL =  sum_A p_i (log p_i - log q_i) = (sum_A exp(z_i - m) ((z_i - m) - (zr_i - m_ref))) / s + (log s_ref - log s)
// Only max-shifted values are added (z_i - m, zr_i - m_ref, log s, log s_ref): a constant added to a row's logits cancels before anything is
// summed.  With one allowed child s = s_ref = 1 and every shifted value is 0: H = KL = 0 exactly.  With zr == z bit for bit, (m_ref, s_ref) ==
// (m, s) bit for bit (one routine, one order: p5_trie_row_lse), every bracket of the KL sum is 0 and KL = 0 exactly.
// Two kernels, the twins of p5_trie_ce_fwd_kernel / p5_trie_ce_bwd_kernel:
//   p5_trie_reg_fwd_kernel   per scored row: nll, lse (the bits of p5_trie_ce_fwd_kernel), H and -- with reference logits -- KL, lse_ref.  The
//                            children are read TWICE: the running (max, sum exp) merge first, then the two sums against the finished m.  An
//                            online merge of (m, s, sum e (z - m)) would save that second read of at most ~1000 cached floats and pay for it with
//                            a rescale term (m_old - m_new) s per merge step in which the cancellation this header avoids comes back; and nll /
//                            lse could not keep the first kernel's arithmetic.  Rows of state 1 / 2: all outputs 0.
//   p5_trie_reg_bwd_kernel   the dense (or compact) dlogits row in ONE pass: zero-filled, then one store per allowed child of
//                              [g_nll (p_j - [j == label]) - g_H p_j (log p_j + H) + g_KL p_j (log p_j - log q_j - KL)] / tau
//                            with p_j = exp(z_j - lse), log p_j = z_j - lse, log q_j = zr_j - lse_ref (the reference is a constant).
//                            Seeds: per-row arrays from autograd (dnll, dH, dKL; a null dH / dKL is zeros), or -- dnll null -- the masked-mean
//                            rule of p5_trie_ce_bwd_kernel: base = [mask] gscale / max(count, 1), g_nll = base * tw, g_H = -entropy_coef * base,
//                            g_KL = kl_coef * base (the regularisers are not weighted by tw: they are properties of the policy).
//   p5_trie_reg_loss_kernel  the fused loss: L_nll (p5_masked_mean_kernel's sum), R_H, R_KL and L_nll + kl_coef R_KL - entropy_coef R_H.
// Every value has one writer and every reduction a fixed order: no atomics, two runs return the same bits.
// Reference logits must be finite on A (not checked): a -inf there gives KL = +inf, as the mathematics does.
#pragma once
#include "p5_trie_ce.h"

// block-wide (m, s) of the row `lr` over the allowed children whose logit in `gate` is finite: p5_trie_ce_fwd_kernel's loop and merge, statement
// by statement.  gate == lr for the policy row; the reference row is gated by the policy's logits, so both run over the same set.
// zl (shared, or nullptr): receives z of the label's child.  sm / ss: 4 shared floats each, owned by this call.
template <class T>
__device__ __forceinline__ void p5_trie_row_lse(float& m_out, float& s_out, const float* __restrict__ lr, const float* __restrict__ gate, const P5TrieCe& tr,
                                                const uint32_t* ex, int c0, int nc, int64_t lab, float* zl, float* sm, float* ss) {
  const int tid = threadIdx.x;
  float m = P5_NEG_INF, s = 0.f;
  for (int i = tid; i < nc; i += 256) {
    if (ex) {
      const int cn = tr.child_node[c0 + i];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) continue;
    }
    const int tok = tr.child_tok[c0 + i];
    const int col = tr.col ? tr.col[c0 + i] : tok;
    if (gate != lr && gate[col] / tr.tau == P5_NEG_INF) continue;
    const float z = lr[col] / tr.tau;
    if (zl && (int64_t)tok == lab) *zl = z;      // (the walk found the label among the allowed children: exactly one thread)
    if (z == P5_NEG_INF) continue;
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
  m_out = m;
  s_out = s;
}

// one workgroup per decoder row.  ent / kl / lse_ref: fp32 [rows]; ref (and with it kl, lse_ref) may be null.
template <class T>
__global__ __launch_bounds__(256) void p5_trie_reg_fwd_kernel(float* __restrict__ nll, float* __restrict__ lse_out, float* __restrict__ ent,
                                                             float* __restrict__ kl, float* __restrict__ lse_ref, const float* __restrict__ logits,
                                                             const float* __restrict__ ref, const int64_t* __restrict__ labels,
                                                             const int* __restrict__ node, const int* __restrict__ state, P5TrieCe tr, int Tlen, int ldl,
                                                             int ldr) {
  __shared__ float sm[4], ss[4], rm[4], rs[4], sa[4], sd[4];
  __shared__ float s_zl;
  const int row = blockIdx.x, tid = threadIdx.x;
  if (state[row] != P5_TRIE_SCORED) {
    if (tid == 0) {
      nll[row] = 0.f; lse_out[row] = 0.f; ent[row] = 0.f;
      if (ref) { kl[row] = 0.f; lse_ref[row] = 0.f; }
    }
    return;
  }
  const int nd = node[row];
  const int c0 = tr.child_off[nd], nc = tr.child_off[nd + 1] - c0;
  const uint32_t* ex = p5_trie_excl_row(tr, row / Tlen);
  const float* lr = logits + (size_t)row * ldl;
  const float* rr = ref ? ref + (size_t)row * ldr : nullptr;
  const int64_t lab = labels[row];
  float m, s, mr = 0.f, sr = 1.f;
  p5_trie_row_lse<T>(m, s, lr, lr, tr, ex, c0, nc, lab, &s_zl, sm, ss);
  if (rr) p5_trie_row_lse<T>(mr, sr, rr, lr, tr, ex, c0, nc, lab, nullptr, rm, rs);
  // second visit of the children: sum e (z - m) and sum e ((z - m) - (zr - m_ref)), e = exp(z - m)
  float a = 0.f, dsum = 0.f;
  for (int i = tid; i < nc; i += 256) {
    if (ex) {
      const int cn = tr.child_node[c0 + i];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) continue;
    }
    const int col = tr.col ? tr.col[c0 + i] : tr.child_tok[c0 + i];
    const float z = lr[col] / tr.tau;
    if (z == P5_NEG_INF) continue;
    const float zs = z - m, e = p5_exp<T>(zs);
    a += e * zs;
    if (rr) dsum += e * (zs - (rr[col] / tr.tau - mr));
  }
  a = wave_sum(a);
  dsum = wave_sum(dsum);
  if ((tid & 63) == 0) { sa[tid >> 6] = a; sd[tid >> 6] = dsum; }
  __syncthreads();
  if (tid == 0) {
    const float ls = logf(s);
    const float lse = m + ls;
    lse_out[row] = lse;
    nll[row] = lse - s_zl;
    ent[row] = ls - (((sa[0] + sa[1]) + sa[2]) + sa[3]) / s;
    if (rr) {
      const float lsr = logf(sr);
      lse_ref[row] = mr + lsr;
      kl[row] = (((sd[0] + sd[1]) + sd[2]) + sd[3]) / s + (lsr - ls);
    }
  }
}

// one workgroup per decoder row: p5_trie_ce_bwd_kernel's zero fill, drain and barrier (the same addresses are written twice), then one store per
// allowed child.  ent / kl / lse_ref: what the forward wrote; ref null: no KL term (kl, lse_ref, dKL are not read).
template <class T>
__global__ __launch_bounds__(256) void p5_trie_reg_bwd_kernel(T* __restrict__ dlogits, const float* __restrict__ logits, const float* __restrict__ ref,
                                                             const float* __restrict__ lse, const float* __restrict__ ent, const float* __restrict__ kl,
                                                             const float* __restrict__ lse_ref, const int64_t* __restrict__ labels,
                                                             const int* __restrict__ node, const int* __restrict__ state, const float* __restrict__ dnll,
                                                             const float* __restrict__ dH, const float* __restrict__ dKL, P5TrieCe tr, int ldl, int ldr,
                                                             int ldd, const int64_t* __restrict__ out_attn, int Tlen, float gscale, float entropy_coef,
                                                             float kl_coef) {
  constexpr int EPF = TT<T>::EPF;
  const int row = blockIdx.x, tid = threadIdx.x;
  T* dr = dlogits + (size_t)row * ldd;
  for (int j = tid * EPF; j < ldd; j += 256 * EPF) st16(dr + j, zero16());      // (ldd is a multiple of 16 bytes: the head GEMM pads V to 64)
  if (state[row] != P5_TRIE_SCORED) return;
  float g, gH, gK;
  if (dnll) {
    g = dnll[row];
    gH = dH ? dH[row] : 0.f;
    gK = ref && dKL ? dKL[row] : 0.f;
  } else {
    const int b = row / Tlen;
    float cnt = 0.f;
    for (int t = 0; t < Tlen; ++t) cnt += out_attn[(size_t)b * Tlen + t] != 0 ? 1.f : 0.f;
    g = out_attn[row] != 0 ? gscale / fmaxf(cnt, 1.f) : 0.f;
    gH = -entropy_coef * g;
    gK = ref ? kl_coef * g : 0.f;
    if (tr.tw) g *= tr.tw[b];
  }
  P5_WAIT_VM(0);      // this wave's zero stores are acknowledged before anybody's child store leaves
  __syncthreads();
  const int nd = node[row];
  const int c0 = tr.child_off[nd], nc = tr.child_off[nd + 1] - c0;
  const uint32_t* ex = p5_trie_excl_row(tr, row / Tlen);
  const float* lr = logits + (size_t)row * ldl;
  const float* rr = ref ? ref + (size_t)row * ldr : nullptr;
  const int64_t lab = labels[row];
  const float l = lse[row], H = ent[row];
  const float lq = rr ? lse_ref[row] : 0.f, K = rr ? kl[row] : 0.f;
  for (int i = tid; i < nc; i += 256) {
    if (ex) {
      const int cn = tr.child_node[c0 + i];
      if ((ex[cn >> 5] >> (cn & 31)) & 1u) continue;
    }
    const int tok = tr.child_tok[c0 + i];
    const int col = tr.col ? tr.col[c0 + i] : tok;
    const float z = lr[col] / tr.tau;
    const float lp = z - l, p = p5_exp<T>(lp);
    float v = g * (p - ((int64_t)tok == lab ? 1.f : 0.f));
    if (z != P5_NEG_INF) {          // (a masked logit is outside A: p = 0 and no regulariser term -- 0 * log 0 is not formed)
      // (a term that is zero adds nothing, not a signed zero that could turn a -0.0 entry into +0.0: with g_H = g_KL = 0 the entry is
      //  p5_trie_ce_bwd_kernel's bit for bit, and with the reference equal to the policy the entry is that of g_KL = 0 bit for bit)
      if (gH != 0.f) {
        const float t = gH * (p * (lp + H));
        if (t != 0.f) v -= t;
      }
      if (gK != 0.f) {
        const float t = gK * (p * ((lp - (rr[col] / tr.tau - lq)) - K));
        if (t != 0.f) v += t;
      }
    }
    dr[col] = from_f<T>(v / tr.tau);
  }
}

// the fused loss behind p5_trie_reg_fwd_kernel: one workgroup, p5_masked_mean_kernel's order of summation for each of the three masked means.
// terms (may be null) = (L_nll, R_H, R_KL); loss = L_nll + kl_coef R_KL - entropy_coef R_H.  kl null: R_KL = 0.
__global__ __launch_bounds__(256) void p5_trie_reg_loss_kernel(float* __restrict__ loss, float* __restrict__ terms, const float* __restrict__ nll,
                                                              const float* __restrict__ ent, const float* __restrict__ kl,
                                                              const int64_t* __restrict__ out_attn, int B, int T, const float* __restrict__ tw,
                                                              float entropy_coef, float kl_coef) {
  __shared__ float sred[4];
  float s = 0.f, sh = 0.f, sk = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    float num = 0.f, nh = 0.f, nk = 0.f, cnt = 0.f;
    for (int t = 0; t < T; ++t) {
      const float m = out_attn[(size_t)b * T + t] != 0 ? 1.f : 0.f;
      num += nll[(size_t)b * T + t] * m;
      nh += ent[(size_t)b * T + t] * m;
      if (kl) nk += kl[(size_t)b * T + t] * m;
      cnt += m;
    }
    const float c = fmaxf(cnt, 1.f);
    float r = num / c;
    if (tw) r *= tw[b];
    s += r;
    sh += nh / c;
    sk += nk / c;
  }
  s = block_reduce(s, false, sred);
  sh = block_reduce(sh, false, sred);
  sk = block_reduce(sk, false, sred);
  if (threadIdx.x == 0) {
    const float l0 = s / (float)B, rh = sh / (float)B, rk = sk / (float)B;
    if (terms) { terms[0] = l0; terms[1] = rh; terms[2] = rk; }
    loss[0] = (l0 + kl_coef * rk) - entropy_coef * rh;
  }
}
