// p5_policy.h -- the batch of an on-policy (REINFORCE-style) fine-tuning step, built on the device from what the sampler returned: the glue
// between p5_sample_items / p5_sample_slates and the grouped fused step (p5_forward_loss_targets), with no host synchronisation.
//
//   p5_policy_batch_kernel   one workgroup (256 threads) per user.  Reads the user's S drawn sequences int64 [S, Ts] (decoder start first, the
//                            drawn tokens through </s>, pad-filled; an all-pad row = nothing drawn) and the user's gold target (labels /
//                            output_attention int64 [Tg]; a position is ATTENDED iff output_attention != 0 and no label at or in front of it is -100:
//                            the engine scores nothing at a -100 and behind it, so a -100 ends the gold), and writes, with
//                            G = S + with_gold and To = max(Tg, Ts - 1):
//                              labels_out / attention_out int64 [G, To]   slot 0 = the gold as given (mask = attended) when with_gold, then the
//                                                                         draws in draw order; behind a draw's </s>: label 0, mask 0
//                              rewards_out, advantages fp32 [S], weights_out fp32 [G], user_stats fp32 [4]
//                            Length of a draw: n = index of the first </s> + 1; without a </s> (a draw cut by max_length) the tokens in front of
//                            the first pad.  n = 0: the draw does not exist (reward, advantage and weight 0, all-zero mask).
//                            Reward: rewards[s] when given, else the HIT reward: 1 iff the draw's n tokens equal the gold's attended tokens, in
//                            order and in number.  user_stats always counts hits by token match.
//                            Advantages over the Se existing draws.  The rewards are first taken relative to the first existing draw's,
//                            d_s = r_s - r_first (so equal rewards give d = 0 EXACTLY, before any division), sum = sum_s d_s:
//                              none  A_s = r_s
//                              mean  A_s = d_s - sum / Se
//                              loo   A_s = d_s - (sum - d_s) / max(Se - 1, 1)
//                              grpo  A_s = (d_s - sum / Se) / (sqrt(sum_s (d_s - sum / Se)^2 / Se) + adv_eps); a zero numerator gives 0 whatever
//                                    the denominator (adv_eps = 0 included)
//                            Weights: w[0] = sft_coef G (with_gold), w[g0 + s] = policy_coef A_s G / S (n_s if token_sum): the engine's
//                            sum_{b,g} w (token-mean NLL) / (B G) is then sft_coef mean_b l(gold) + policy_coef mean_b (1/S) sum_s A_s l_s.
//                            user_stats: (sum of existing rewards, sum |A|, hits, 2 Se + [some d_s != 0]) -- the last one an exact small integer.
//   p5_policy_stats_kernel   one workgroup: stats fp32 [8] from user_stats [B, 4] -- mean reward and mean |A| over the existing draws, share of
//                            users with signal, share of existing draws that hit, share of users with a hit, number of users without a draw, 0, 0.
// Every value has one writer and every sum a fixed order (a thread's draws in index order, then block_reduce): no atomics, two runs return the
// same bits.
#pragma once
#include "p5_elem.h"

#define P5_POLICY_MAX_S 1024
enum { P5_BASELINE_NONE = 0, P5_BASELINE_MEAN = 1, P5_BASELINE_LOO = 2, P5_BASELINE_GRPO = 3 };

struct P5PolicyArgs {
  const int64_t* seq; const int64_t* labels; const int64_t* out_attn; const float* rewards;
  int64_t* labels_out; int64_t* attn_out; float* rewards_out; float* adv; float* weights; float* user_stats;
  int S, Ts, Tg, To, baseline, token_sum, with_gold, pad_id, eos_id;
  float policy_coef, sft_coef, adv_eps;
  // the clipped-ratio objective's inputs (p5_clip.h), both optional: the behaviour policy's log-probabilities of the draws' labels, gathered from
  // the sampler's token_logprobs fp32 [B * S, Ts - 1] into old_lp_out fp32 [G, To] (the gold slot and positions behind a draw's end: 0), and
  // mode_out int32 [G] (gold 0 = plain weighted NLL, draws 1 = clipped surrogate).  Null: nothing is read or written.
  const float* token_lp = nullptr; float* old_lp_out = nullptr; int* mode_out = nullptr;
};

// position j of the gold is attended iff j lies in front of the gold's first -100 label (Te; the engine scores nothing at a -100 and behind
// it) and output_attention[j] != 0
__device__ static __forceinline__ bool p5_policy_attended(const P5PolicyArgs& a, size_t gold, int j, int Te) {
  return j < Te && a.out_attn[gold + j] != 0;
}

__global__ __launch_bounds__(256) void p5_policy_batch_kernel(P5PolicyArgs a) {
  __shared__ int s_n[P5_POLICY_MAX_S];        // tokens of draw s (0: no draw)
  __shared__ float s_r[P5_POLICY_MAX_S];      // reward of draw s (0: no draw)
  __shared__ float sred[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = a.S, Ts = a.Ts, Tg = a.Tg, To = a.To, G = S + a.with_gold;
  const size_t gold = (size_t)b * Tg;
  // 0. the gold's end: the index of its first -100 label, or Tg (a maximum of Tg - j: order-free; Tg <= 2^24 is exact in fp32)
  float tail = 0.f;
  for (int j = tid; j < Tg; j += 256)
    if (a.labels[gold + j] == -100) { tail = (float)(Tg - j); break; }
  const int Te = Tg - (int)block_reduce(tail, true, sred);
  // 1. per draw: its length, its hit, its reward
  float hits = 0.f;
  for (int s = tid; s < S; s += 256) {
    const int64_t* row = a.seq + ((size_t)b * S + s) * Ts + 1;
    int n = Ts - 1;
    for (int i = 0; i < Ts - 1; ++i) {
      const int64_t t = row[i];
      if (t == a.eos_id) { n = i + 1; break; }
      if (t == a.pad_id) { n = i; break; }
    }
    bool hit = n > 0;
    int j = 0;
    for (int i = 0; i < n && hit; ++i) {
      while (j < Te && !p5_policy_attended(a, gold, j, Te)) ++j;
      hit = j < Te && a.labels[gold + j] == row[i];
      ++j;
    }
    while (hit && j < Te) {               // the gold must have no attended token left
      if (p5_policy_attended(a, gold, j, Te)) hit = false;
      ++j;
    }
    s_n[s] = n;
    s_r[s] = n > 0 ? (a.rewards ? a.rewards[(size_t)b * S + s] : (hit ? 1.f : 0.f)) : 0.f;
    hits += hit ? 1.f : 0.f;
  }
  __syncthreads();
  // 2. labels and masks, one element per thread and pass (consecutive threads, consecutive addresses)
  for (int e = tid; e < G * To; e += 256) {
    const int g = e / To, t = e - g * To;
    int64_t lab = 0, m = 0;
    if (a.with_gold && g == 0) {
      if (t < Tg) { lab = a.labels[gold + t]; m = p5_policy_attended(a, gold, t, Te) ? 1 : 0; }
    } else {
      const int s = g - a.with_gold;
      if (t < s_n[s]) { lab = a.seq[((size_t)b * S + s) * Ts + 1 + t]; m = 1; }
    }
    a.labels_out[(size_t)b * G * To + e] = lab;
    a.attn_out[(size_t)b * G * To + e] = m;
    if (a.old_lp_out) {
      const int s = g - a.with_gold;
      a.old_lp_out[(size_t)b * G * To + e] = (s >= 0 && t < s_n[s]) ? a.token_lp[((size_t)b * S + s) * (Ts - 1) + t] : 0.f;
    }
  }
  if (a.mode_out)
    for (int g = tid; g < G; g += 256) a.mode_out[(size_t)b * G + g] = (a.with_gold && g == 0) ? 0 : 1;
  // 3. the first existing draw, the count, the sums.  A thread visits its draws in index order and block_reduce has a fixed order.
  float cnt = 0.f, rsum = 0.f, lead = 0.f;
  for (int s = tid; s < S; s += 256)
    if (s_n[s] > 0) { cnt += 1.f; rsum += s_r[s]; lead = fmaxf(lead, (float)(S - s)); }
  const float Se = block_reduce(cnt, false, sred);
  rsum = block_reduce(rsum, false, sred);
  hits = block_reduce(hits, false, sred);
  const int first = S - (int)block_reduce(lead, true, sred);          // (S <= 1024: exact in fp32)
  const float r0 = first < S ? s_r[first] : 0.f;
  float dsum = 0.f, sig = 0.f;
  for (int s = tid; s < S; s += 256) {
    if (a.rewards_out) a.rewards_out[(size_t)b * S + s] = s_r[s];
    if (s_n[s] > 0) {
      const float d = s_r[s] - r0;
      dsum += d;
      sig = fmaxf(sig, d != 0.f ? 1.f : 0.f);
    }
  }
  dsum = block_reduce(dsum, false, sred);
  sig = block_reduce(sig, true, sred);
  const float dmean = dsum / fmaxf(Se, 1.f);
  float inv = 1.f;
  if (a.baseline == P5_BASELINE_GRPO) {
    float v = 0.f;
    for (int s = tid; s < S; s += 256)
      if (s_n[s] > 0) { const float c = (s_r[s] - r0) - dmean; v += c * c; }
    v = block_reduce(v, false, sred);
    const float den = sqrtf(v / fmaxf(Se, 1.f)) + a.adv_eps;
    inv = den > 0.f ? 1.f / den : 0.f;          // (adv_eps = 0 and equal rewards: 0 * 0, not 0 * inf)
  }
  // 4. advantages and weights
  float asum = 0.f;
  const float scale = (float)G / (float)S;
  for (int s = tid; s < S; s += 256) {
    float A = 0.f, w = 0.f;
    if (s_n[s] > 0) {
      const float d = s_r[s] - r0;
      if (a.baseline == P5_BASELINE_NONE) A = s_r[s];
      else if (a.baseline == P5_BASELINE_MEAN) A = d - dmean;
      else if (a.baseline == P5_BASELINE_LOO) A = d - (dsum - d) / fmaxf(Se - 1.f, 1.f);
      else { const float c = d - dmean; A = c == 0.f ? 0.f : c * inv; }
      w = a.policy_coef * A * scale;
      if (a.token_sum) w *= (float)s_n[s];
    }
    a.adv[(size_t)b * S + s] = A;
    a.weights[(size_t)b * G + a.with_gold + s] = w;
    asum += fabsf(A);
  }
  asum = block_reduce(asum, false, sred);
  if (tid == 0) {
    if (a.with_gold) a.weights[(size_t)b * G] = a.sft_coef * (float)G;
    float* us = a.user_stats + (size_t)b * 4;
    us[0] = rsum; us[1] = asum; us[2] = hits; us[3] = 2.f * Se + sig;
  }
}

// stats[0..7] from user_stats [B, 4]; one workgroup of 256 threads, users strided over the threads, then block_reduce: a fixed order
__global__ __launch_bounds__(256) void p5_policy_stats_kernel(float* __restrict__ stats, const float* __restrict__ user_stats, int B) {
  __shared__ float sred[4];
  float r = 0.f, aa = 0.f, h = 0.f, n = 0.f, sg = 0.f, uh = 0.f, empty = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* us = user_stats + (size_t)b * 4;
    const int code = (int)us[3];
    r += us[0]; aa += us[1]; h += us[2];
    n += (float)(code >> 1);
    sg += (float)(code & 1);
    uh += us[2] > 0.f ? 1.f : 0.f;
    empty += (code >> 1) == 0 ? 1.f : 0.f;
  }
  r = block_reduce(r, false, sred); aa = block_reduce(aa, false, sred); h = block_reduce(h, false, sred); n = block_reduce(n, false, sred);
  sg = block_reduce(sg, false, sred); uh = block_reduce(uh, false, sred); empty = block_reduce(empty, false, sred);
  if (threadIdx.x == 0) {
    const float nd = fmaxf(n, 1.f);
    stats[0] = r / nd; stats[1] = sg / (float)B; stats[2] = aa / nd; stats[3] = h / nd; stats[4] = uh / (float)B; stats[5] = empty;
    stats[6] = 0.f; stats[7] = 0.f;
  }
}
