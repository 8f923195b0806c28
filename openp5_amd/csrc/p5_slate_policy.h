// p5_slate_policy.h -- the batch of an on-policy step from SLATES: the importance-weighted without-replacement estimator of Kool, van Hoof
// and Welling (2019, 2020) on what p5_sample_slates returned, the slate counterpart of p5_policy.h (whose conventions -- length of a row, the
// -100 rule of the gold, the hit test by token match, the G / S scaling, token_sum -- it keeps).
//
//   p5_policy_slate_batch_kernel   one workgroup (256 threads) per user.  Reads the user's S slates of K1 = K + 1 slots: sequences int64
//                            [S, K1, Ts], log p(item) phi fp32 [S, K1], the perturbed values g fp32 [S, K1] (descending), optionally rewards fp32
//                            [S, K1] (the last slot is never read) and token_logprobs fp32 [S K1, Ts - 1], and the gold (labels / output_attention
//                            [Tg]).  Slot K of a slate is the THRESHOLD only, kappa = g[K] (behind p5_sample_slates: un-conditioned with the
//                            root noise, p5_slate_kappa): it becomes no training row.  A slot i < K exists iff
//                            its row has n > 0 tokens; a slot that does not exist has weight 0 and an all-zero mask.  For an existing slot, with
//                            x = phi_i - kappa:
//                              kappa = -inf (the allowed items ran out before slot K)   log q = 0: the slot is in the slate with certainty
//                              x <= -16                                                 log q = x   (q = 1 - exp(-u) = u - u^2 / 2 ..., u = e^x: the
//                                                                                       neglected relative term u / 2 < 6e-8; u itself may underflow)
//                              else                                                     log q = log(-expm1(-exp(x)))
//                              omega_i = exp(phi_i - log q)   (in the log domain: exp(phi) / q underflows for rare items)
//                            Per slate j, over its existing slots in SLOT ORDER by one thread (a slate's results do not depend on S or on the
//                            other slates): W = sum omega, V = sum omega r, ESS = W^2 / sum omega^2.  The advantage of a slot:
//                              unbiased (0)    A_i = omega_i r_i
//                              normalized (1)  A_i = (omega_i / W) (d_i - (sum omega d) / W), d_i = r_i - r of the slate's first existing slot: equal
//                                              rewards give d = 0 and A = 0 EXACTLY, before any division
//                            Reward: rewards[j, i] when given, else the hit reward of p5_policy.h.  With G = S K + with_gold and To = max(Tg, Ts - 1):
//                              labels_out / attention_out int64 [G, To]   slot 0 = the gold when with_gold, then the slates in (j, i) order
//                              rewards_out, advantages, importance (omega) fp32 [S, K], weights_out fp32 [G]: w[0] = sft_coef G, the others
//                              policy_coef A G / S (n if token_sum); slate_stats fp32 [S, 4] = (V, W, kappa, ESS); user_stats fp32 [8]
//                              old_lp_out fp32 [G, To] / mode_out int32 [G] (both optional) as p5_policy_batch_clip gathers them
//   p5_policy_slate_stats_kernel   one workgroup: stats fp32 [8] from user_stats [B, 8] -- mean V and mean W over the existing slates (those with
//                            an existing slot), share of users with a non-zero advantage, mean |A| over the existing slots, share of existing
//                            slates that contain the gold, share of existing slates with kappa = -inf, users without a draw, mean ESS.
// Every value has one writer and every sum a fixed order: no atomics, two runs return the same bits.
#pragma once
#include "p5_elem.h"
#include "p5_rng.h"

#define P5_SLATE_POLICY_MAX_SLOTS 1024      // S * K1 per user: what the LDS arrays hold
enum { P5_SLATE_UNBIASED = 0, P5_SLATE_NORMALIZED = 1 };

struct P5SlatePolicyArgs {
  const int64_t* seq; const float* logp; const float* pert; const int64_t* labels; const int64_t* out_attn; const float* rewards; const float* token_lp;
  int64_t* labels_out; int64_t* attn_out; float* rewards_out; float* adv; float* importance; float* weights; float* slate_stats; float* user_stats;
  float* old_lp_out; int* mode_out;
  int S, K1, Ts, Tg, To, estimator, token_sum, with_gold, pad_id, eos_id;
  float policy_coef, sft_coef;
  // the root noise (see p5_slate_kappa); streams null: the perturbed values are taken as they are
  const int* streams = nullptr; uint32_t seed = 0, slate_base = 0;
};

// The threshold of slate sl of user b.  The inclusion probability q = 1 - exp(-exp(phi - kappa)) is that of UNCONDITIONED perturbed values
// G_i = phi_i + Gumbel.  p5_sample_slates (p5_sbs.h) starts its root at G = 0: its values are those of a draw whose maximum is conditioned to
// be 0, G~_i = -log(exp(-G_i) - exp(-Z) + 1) with Z = max_i G_i.  The slate (the ORDER) does not depend on Z, but the threshold does, and
// with kappa = G~[K] the estimator is biased (mean W = 0.94 at N = 8, K = 3).  exp(-G_i) - exp(-Z) is the same for every Z, and Z is a
// standard Gumbel independent of it, so the unconditioned threshold is recovered with one more draw: E = exp(-Z) = -log(u) ~ Exp(1) and
//   kappa = -log(exp(-G~[K]) - 1 + E) = G~[K] - log1p((E - 1) exp(G~[K]))          (G~ <= 0; -inf stays -inf)
// u is the uniform of p5_rng.h at coordinates the sampler never uses: (seed, stream, slate, step 0, edge 2^32 - 1) -- a pure function of
// what the slate itself was drawn with, so a slate's threshold does not depend on the call that holds it.
__device__ static __forceinline__ float p5_slate_kappa(const P5SlatePolicyArgs& a, int b, int sl) {
  const float g = a.pert[((size_t)b * a.S + sl) * a.K1 + a.K1 - 1];
  if (!a.streams || g == P5_NEG_INF) return g;
  const float e = -logf(p5_sample_uniform(p5_sample_row_key(a.seed, (uint32_t)a.streams[b], a.slate_base + (uint32_t)sl, 0u), 0xFFFFFFFFu));
  return g - log1pf((e - 1.f) * expf(g));
}

__global__ __launch_bounds__(256) void p5_policy_slate_batch_kernel(P5SlatePolicyArgs a) {
  __shared__ int s_n[P5_SLATE_POLICY_MAX_SLOTS];        // tokens of slot e = j K1 + i (0: no draw; the threshold slot: 0)
  __shared__ float s_r[P5_SLATE_POLICY_MAX_SLOTS];      // its reward
  __shared__ float s_w[P5_SLATE_POLICY_MAX_SLOTS];      // its importance weight omega
  __shared__ int s_hit[P5_SLATE_POLICY_MAX_SLOTS];      // 1 iff it is the gold, token by token
  __shared__ float sred[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = a.S, K1 = a.K1, K = K1 - 1, Ts = a.Ts, Tg = a.Tg, To = a.To, R = S * K1, G = S * K + a.with_gold;
  const size_t gold = (size_t)b * Tg, slot0 = (size_t)b * R, used0 = (size_t)b * S * K;
  // 0. the gold's end: the index of its first -100 label, or Tg (p5_policy.h)
  float tail = 0.f;
  for (int j = tid; j < Tg; j += 256)
    if (a.labels[gold + j] == -100) { tail = (float)(Tg - j); break; }
  const int Te = Tg - (int)block_reduce(tail, true, sred);
  // 1. per slot: its length, its hit, its reward, its importance weight
  for (int e = tid; e < R; e += 256) {
    const int sl = e / K1, i = e - sl * K1;
    int n = 0;
    bool hit = false;
    float r = 0.f, w = 0.f;
    if (i < K) {
      const int64_t* row = a.seq + (slot0 + e) * Ts + 1;
      n = Ts - 1;
      for (int t = 0; t < Ts - 1; ++t) {
        const int64_t tk = row[t];
        if (tk == a.eos_id) { n = t + 1; break; }
        if (tk == a.pad_id) { n = t; break; }
      }
      hit = n > 0;
      int j = 0;
      for (int t = 0; t < n && hit; ++t) {
        while (j < Te && !(a.out_attn[gold + j] != 0)) ++j;
        hit = j < Te && a.labels[gold + j] == row[t];
        ++j;
      }
      while (hit && j < Te) {               // the gold must have no attended token left
        if (a.out_attn[gold + j] != 0) hit = false;
        ++j;
      }
      if (n > 0) {
        r = a.rewards ? a.rewards[slot0 + e] : (hit ? 1.f : 0.f);
        const float phi = a.logp[slot0 + e], kappa = p5_slate_kappa(a, b, sl);
        float logq = 0.f;
        if (kappa != P5_NEG_INF) {
          const float x = phi - kappa;
          logq = x <= -16.f ? x : logf(-expm1f(-expf(x)));
        }
        w = expf(phi - logq);
      }
    }
    s_n[e] = n; s_r[e] = r; s_w[e] = w; s_hit[e] = hit ? 1 : 0;
  }
  __syncthreads();
  // 2. labels, masks and the behaviour policy's token log-probabilities, one element per thread and pass
  for (int e = tid; e < G * To; e += 256) {
    const int g = e / To, t = e - g * To;
    int64_t lab = 0, m = 0;
    float old = 0.f;
    if (a.with_gold && g == 0) {
      if (t < Tg) { lab = a.labels[gold + t]; m = (t < Te && a.out_attn[gold + t] != 0) ? 1 : 0; }
    } else {
      const int u = g - a.with_gold, sl = u / K, src = sl * K1 + (u - sl * K);
      if (t < s_n[src]) {
        lab = a.seq[(slot0 + src) * Ts + 1 + t]; m = 1;
        if (a.old_lp_out) old = a.token_lp[(slot0 + src) * (Ts - 1) + t];
      }
    }
    a.labels_out[(size_t)b * G * To + e] = lab;
    a.attn_out[(size_t)b * G * To + e] = m;
    if (a.old_lp_out) a.old_lp_out[(size_t)b * G * To + e] = old;
  }
  if (a.mode_out)
    for (int g = tid; g < G; g += 256) a.mode_out[(size_t)b * G + g] = (a.with_gold && g == 0) ? 0 : 1;
  // 3. per slate, one thread, slot order: the sums, then the advantages and the weights
  float uV = 0.f, uW = 0.f, uA = 0.f, uE = 0.f, uHit = 0.f, uInf = 0.f, uSl = 0.f, uSlots = 0.f, uSig = 0.f;
  const float scale = (float)G / (float)S;
  for (int sl = tid; sl < S; sl += 256) {
    const int e0 = sl * K1;
    float W = 0.f, V = 0.f, W2 = 0.f, Vd = 0.f, r0 = 0.f, cnt = 0.f;
    int hit = 0;
    for (int i = 0; i < K; ++i)
      if (s_n[e0 + i] > 0) {
        const float w = s_w[e0 + i];
        if (cnt == 0.f) r0 = s_r[e0 + i];
        W += w; V += w * s_r[e0 + i]; W2 += w * w; Vd += w * (s_r[e0 + i] - r0);
        cnt += 1.f; hit |= s_hit[e0 + i];
      }
    const float kappa = p5_slate_kappa(a, b, sl);
    const float ess = W2 > 0.f ? W * W / W2 : 0.f;
    const float invW = W > 0.f ? 1.f / W : 0.f, dbar = Vd * invW;
    float* ss = a.slate_stats + ((size_t)b * S + sl) * 4;
    ss[0] = V; ss[1] = W; ss[2] = kappa; ss[3] = ess;
    for (int i = 0; i < K; ++i) {
      const int e = e0 + i;
      float A = 0.f, w = 0.f;
      if (s_n[e] > 0) {
        if (a.estimator == P5_SLATE_UNBIASED) A = s_w[e] * s_r[e];
        else { const float c = (s_r[e] - r0) - dbar; A = c == 0.f ? 0.f : (s_w[e] * invW) * c; }
        w = a.policy_coef * A * scale;
        if (a.token_sum) w *= (float)s_n[e];
      }
      const size_t o = used0 + (size_t)sl * K + i;
      a.rewards_out[o] = s_r[e]; a.adv[o] = A; a.importance[o] = s_w[e];
      a.weights[(size_t)b * G + a.with_gold + sl * K + i] = w;
      uA += fabsf(A);
      if (A != 0.f) uSig = 1.f;
    }
    if (cnt > 0.f) {
      uV += V; uW += W; uE += ess; uSl += 1.f; uSlots += cnt; uHit += (float)hit;
      uInf += kappa == P5_NEG_INF ? 1.f : 0.f;
    }
  }
  uV = block_reduce(uV, false, sred); uW = block_reduce(uW, false, sred); uA = block_reduce(uA, false, sred); uE = block_reduce(uE, false, sred);
  uHit = block_reduce(uHit, false, sred); uInf = block_reduce(uInf, false, sred); uSl = block_reduce(uSl, false, sred);
  uSlots = block_reduce(uSlots, false, sred); uSig = block_reduce(uSig, true, sred);
  if (tid == 0) {
    if (a.with_gold) a.weights[(size_t)b * G] = a.sft_coef * (float)G;
    float* us = a.user_stats + (size_t)b * 8;             // (the counts are small integers: exact in fp32)
    us[0] = uV; us[1] = uW; us[2] = uA; us[3] = uE; us[4] = uHit; us[5] = uInf; us[6] = 2.f * uSl + uSig; us[7] = uSlots;
  }
}

// stats[0..7] from user_stats [B, 8]; one workgroup of 256 threads, users strided over the threads, then block_reduce: a fixed order
__global__ __launch_bounds__(256) void p5_policy_slate_stats_kernel(float* __restrict__ stats, const float* __restrict__ user_stats, int B) {
  __shared__ float sred[4];
  float v = 0.f, w = 0.f, aa = 0.f, ess = 0.f, h = 0.f, inf = 0.f, nsl = 0.f, nslot = 0.f, sg = 0.f, empty = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* us = user_stats + (size_t)b * 8;
    const int code = (int)us[6];
    v += us[0]; w += us[1]; aa += us[2]; ess += us[3]; h += us[4]; inf += us[5]; nslot += us[7];
    nsl += (float)(code >> 1);
    sg += (float)(code & 1);
    empty += (code >> 1) == 0 ? 1.f : 0.f;
  }
  v = block_reduce(v, false, sred); w = block_reduce(w, false, sred); aa = block_reduce(aa, false, sred); ess = block_reduce(ess, false, sred);
  h = block_reduce(h, false, sred); inf = block_reduce(inf, false, sred); nsl = block_reduce(nsl, false, sred); nslot = block_reduce(nslot, false, sred);
  sg = block_reduce(sg, false, sred); empty = block_reduce(empty, false, sred);
  if (threadIdx.x == 0) {
    const float ns = fmaxf(nsl, 1.f);
    stats[0] = v / ns; stats[1] = w / ns; stats[2] = sg / (float)B; stats[3] = aa / fmaxf(nslot, 1.f); stats[4] = h / ns; stats[5] = inf / ns;
    stats[6] = empty; stats[7] = ess / ns;
  }
}
