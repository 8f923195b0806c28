// p5_clip.h -- the clipped-ratio (PPO / GRPO / GSPO style) policy objective behind the per-token NLL of p5_forward_loss*: what makes several
// optimizer steps on ONE sampled batch sound.  It takes the place of p5_masked_mean_kernel / p5_masked_mean_g_kernel / p5_trie_reg_loss_kernel
// behind the forward and hands the backward one seed per decoder row (the `dnll` route every loss kernel already has).
//
// A call carries B users x G targets x T positions.  Per target (b, g): nll[t] of the CURRENT weights, the mask m_t = (out_attn != 0),
// cnt = sum_t m_t, the weight w = tw[b, g] (coefficient x advantage x G / S, sign included; tw null = 1), old[t] = the BEHAVIOUR policy's
// log-probability of the label (read only where m_t) and mode[b, g] (0 = the plain weighted masked mean, 1 = the clipped surrogate; mode null = all 1).
// With lo = 1 - eps_low, hi = 1 + eps_high (formed in fp32), base = gscale / max(cnt, 1) and gscale = 1 / (B G):
//   token     rho_t = expf(-(old_t + nll_t))              (log p_new = -nll: rho = exp(log p_new - log p_old))
//             l = (1 / max(cnt, 1)) sum_t m_t max(-rho_t w, -clamp(rho_t, lo, hi) w)
//   sequence  rho = expf(-(sum_t m_t (old_t + nll_t)) / max(cnt, 1))      (length-normalised)
//             l = max(-rho w, -clamp(rho, lo, hi) w);  a target with cnt = 0 contributes nothing
//   loss = sum_{b,g} l_bg / (B G); a mode-0 target contributes w (sum_t nll m) / max(cnt, 1) as p5_masked_mean_kernel has it; with regularisers
//   (ent / kl rows given) terms = (that loss, R_H, R_KL) and loss = (L + kl_coef R_KL) - entropy_coef R_H, as p5_trie_reg_loss_kernel has them.
//   seed g_t = d loss / d nll_t = m_t ((base w) rho) [active], 0 where labels == -100.  A unit (a token, or -- sequence -- a target) is CLIPPED iff
//   (w > 0 and rho > hi) or (w < 0 and rho < lo), else active: at rho == lo or rho == hi it is active, as torch.minimum + torch.clamp differentiate.
//   A clipped unit's seed and the seeds of a w == 0 target are exact zeros by select (never 0 * rho: rho may be +inf).  base w is formed as
//   p5_masked_mean_g_kernel forms it (gscale / fmaxf(cnt, 1), then *= w), so with rho == 1.0f a seed carries the plain weighted step's bits;
//   mode-0 targets get that kernel's seeds.  With regularisers the H / KL seeds of every row (-entropy_coef base, +kl_coef base, masked, not
//   weighted) go to seed[rows + r] and seed[2 rows + r]: p5_trie_reg_bwd_kernel's masked-mean rule, as arrays.
// clip_stats fp32 [8] -- units = attended tokens of mode-1 targets with w != 0 (token), such targets with cnt > 0 (sequence):
//   0 number of units, 1 share clipped, 2 share clipped at hi, 3 share clipped at lo, 4 mean rho, 5 max rho, 6 min rho, 7 mean of (rho - 1) - log rho
//   (the k3 estimate of KL(old || new)).  4 and 7 run over the units with 0 < rho < +inf (an rho that left fp32's range has no finite mean; it is
//   still counted, clipped or not, and seen by 5 / 6).  No unit: (0, 0, 0, 0, 1, 1, 1, 0); units but none in range: 4 = 1 and 7 = 0.
//
//   p5_clip_objective_kernel   one workgroup (256 threads) per user; threads stride over the user's G targets, a thread walks its target's T
//                              positions in order.  Writes the seeds and the user's partials fp32 [16]: 0 loss part, 1 / 2 the H / KL parts,
//                              3 units, 4 clipped at hi, 5 clipped at lo, 6 sum rho, 7 max rho, 8 max -rho, 9 sum k3, 10 units in range.
//   p5_clip_finish_kernel      one workgroup: users strided over the threads, then block_reduce; writes loss[0], terms[3] if given, stats[8].
// No atomics; every value has one writer and every sum a fixed order (a thread's targets in index order, then block_reduce): two runs return the
// same bits.  Maxima are order-free.
#pragma once
#include "p5_elem.h"

enum { P5_RATIO_TOKEN = 0, P5_RATIO_SEQUENCE = 1 };
#define P5_CLIP_PARTIALS 16

struct P5ClipArgs {
  const float* nll; const float* old_lp; const int64_t* out_attn; const int64_t* labels; const float* tw; const int* mode;
  const float* ent; const float* kl;            // regularisers: the rows' entropy / KL (kl may be null), or ent null = none
  float* seed; float* partials;
  int G, T, ratio_mode, rows;                   // rows = B G T
  float lo, hi, gscale, entropy_coef, kl_coef;
};

// one unit's surrogate and whether it is active; its statistics go to the thread's accumulators
struct P5ClipAcc { float units, chi, clo, srho, mx, mn, sk3, nreg; };

__device__ static __forceinline__ float p5_clip_unit(float x /* log rho */, float w, float lo, float hi, bool* active, float* rho_out, P5ClipAcc& s) {
  const float rho = expf(x);
  *rho_out = rho;
  const bool at_hi = w > 0.f && rho > hi, at_lo = w < 0.f && rho < lo;
  *active = !(at_hi || at_lo);
  s.units += 1.f;
  s.chi += at_hi ? 1.f : 0.f;
  s.clo += at_lo ? 1.f : 0.f;
  s.mx = fmaxf(s.mx, rho);
  s.mn = fmaxf(s.mn, -rho);
  if (rho > 0.f && rho < __builtin_huge_valf()) { s.srho += rho; s.sk3 += (rho - 1.f) - x; s.nreg += 1.f; }
  return fmaxf(-(rho * w), -(fminf(fmaxf(rho, lo), hi) * w));
}

__global__ __launch_bounds__(256) void p5_clip_objective_kernel(P5ClipArgs a) {
  __shared__ float sred[4];
  const int b = blockIdx.x, tid = threadIdx.x, G = a.G, T = a.T;
  float s = 0.f, sh = 0.f, sk = 0.f;
  P5ClipAcc st = {0.f, 0.f, 0.f, 0.f, P5_NEG_INF, P5_NEG_INF, 0.f, 0.f};
  for (int g = tid; g < G; g += 256) {
    const size_t tg = (size_t)b * G + g, r0 = tg * T;
    float num = 0.f, nh = 0.f, nk = 0.f, cnt = 0.f;
    for (int t = 0; t < T; ++t) {
      const float m = a.out_attn[r0 + t] != 0 ? 1.f : 0.f;
      num += a.nll[r0 + t] * m;
      if (a.ent) nh += a.ent[r0 + t] * m;
      if (a.kl) nk += a.kl[r0 + t] * m;
      cnt += m;
    }
    const float c = fmaxf(cnt, 1.f);
    const float w = a.tw ? a.tw[tg] : 1.f;
    const bool clip = a.mode ? a.mode[tg] != 0 : true;
    sh += nh / c;
    sk += nk / c;
    float bw = a.gscale / c;          // (p5_masked_mean_g_kernel's operands in its order: with rho == 1.0f the seeds below are its bits)
    if (a.tw) bw *= w;
    if (!clip) {
      float r = num / c;
      if (a.tw) r *= w;
      s += r;
      for (int t = 0; t < T; ++t) {
        float gr = a.out_attn[r0 + t] != 0 ? a.gscale / c : 0.f;
        if (a.tw) gr *= w;
        if (a.labels[r0 + t] == -100) gr = 0.f;
        a.seed[r0 + t] = gr;
      }
    } else if (w == 0.f) {            // nothing by select: 0 * rho is not formed
      for (int t = 0; t < T; ++t) a.seed[r0 + t] = 0.f;
    } else if (a.ratio_mode == P5_RATIO_TOKEN) {
      float l = 0.f;
      for (int t = 0; t < T; ++t) {
        float gr = 0.f;
        if (a.out_attn[r0 + t] != 0) {
          bool active;
          float rho;
          l += p5_clip_unit(-(a.old_lp[r0 + t] + a.nll[r0 + t]), w, a.lo, a.hi, &active, &rho, st);
          if (active) gr = bw * rho;
        }
        if (a.labels[r0 + t] == -100) gr = 0.f;
        a.seed[r0 + t] = gr;
      }
      s += l / c;
    } else {
      float d = 0.f;
      for (int t = 0; t < T; ++t)
        if (a.out_attn[r0 + t] != 0) d += a.old_lp[r0 + t] + a.nll[r0 + t];
      bool active = false;
      float gs = 0.f;
      if (cnt > 0.f) {
        float rho;
        s += p5_clip_unit(-d / c, w, a.lo, a.hi, &active, &rho, st);
        if (active) gs = bw * rho;
      }
      for (int t = 0; t < T; ++t) {
        float gr = a.out_attn[r0 + t] != 0 ? gs : 0.f;
        if (a.labels[r0 + t] == -100) gr = 0.f;
        a.seed[r0 + t] = gr;
      }
    }
    if (a.ent) {                      // the regularisers' seeds: the masked-mean rule of p5_trie_reg_bwd_kernel, not weighted
      const float base = a.gscale / c;
      for (int t = 0; t < T; ++t) {
        const float gm = a.out_attn[r0 + t] != 0 ? base : 0.f;
        a.seed[(size_t)a.rows + r0 + t] = -a.entropy_coef * gm;
        a.seed[2 * (size_t)a.rows + r0 + t] = a.kl_coef * gm;
      }
    }
  }
  s = block_reduce(s, false, sred); sh = block_reduce(sh, false, sred); sk = block_reduce(sk, false, sred);
  st.units = block_reduce(st.units, false, sred); st.chi = block_reduce(st.chi, false, sred); st.clo = block_reduce(st.clo, false, sred);
  st.srho = block_reduce(st.srho, false, sred); st.sk3 = block_reduce(st.sk3, false, sred); st.nreg = block_reduce(st.nreg, false, sred);
  st.mx = block_reduce(st.mx, true, sred); st.mn = block_reduce(st.mn, true, sred);
  if (tid == 0) {
    float* p = a.partials + (size_t)b * P5_CLIP_PARTIALS;
    p[0] = s; p[1] = sh; p[2] = sk; p[3] = st.units; p[4] = st.chi; p[5] = st.clo; p[6] = st.srho; p[7] = st.mx; p[8] = st.mn; p[9] = st.sk3;
    p[10] = st.nreg;
    for (int i = 11; i < P5_CLIP_PARTIALS; ++i) p[i] = 0.f;
  }
}

// loss[0], terms[3] (null = none) and stats[8] from the users' partials [B, 16]; n = B * G targets
__global__ __launch_bounds__(256) void p5_clip_finish_kernel(float* __restrict__ loss, float* __restrict__ terms, float* __restrict__ stats,
                                                            const float* __restrict__ partials, int B, int n, int reg, float entropy_coef,
                                                            float kl_coef) {
  __shared__ float sred[4];
  float v[P5_CLIP_PARTIALS];
  for (int i = 0; i < 11; ++i) v[i] = (i == 7 || i == 8) ? P5_NEG_INF : 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* p = partials + (size_t)b * P5_CLIP_PARTIALS;
    for (int i = 0; i < 11; ++i) v[i] = (i == 7 || i == 8) ? fmaxf(v[i], p[i]) : v[i] + p[i];
  }
  for (int i = 0; i < 11; ++i) v[i] = block_reduce(v[i], i == 7 || i == 8, sred);
  if (threadIdx.x == 0) {
    const float l0 = v[0] / (float)n;
    if (reg) {
      const float rh = v[1] / (float)n, rk = v[2] / (float)n;
      if (terms) { terms[0] = l0; terms[1] = rh; terms[2] = rk; }
      loss[0] = (l0 + kl_coef * rk) - entropy_coef * rh;
    } else {
      loss[0] = l0;
    }
    const float u = v[3];
    if (u > 0.f) {
      stats[0] = u; stats[1] = (v[4] + v[5]) / u; stats[2] = v[4] / u; stats[3] = v[5] / u;
      stats[4] = v[10] > 0.f ? v[6] / v[10] : 1.f; stats[5] = v[7]; stats[6] = -v[8]; stats[7] = v[10] > 0.f ? v[9] / v[10] : 0.f;
    } else {
      stats[0] = 0.f; stats[1] = 0.f; stats[2] = 0.f; stats[3] = 0.f; stats[4] = 1.f; stats[5] = 1.f; stats[6] = 1.f; stats[7] = 0.f;
    }
  }
}
