// p5_pref.h -- listwise preference objectives (Plackett-Luce with a depth: DPO, softmax-DPO and the full PL likelihood; IPO) behind the
// per-token NLL of p5_forward_loss_targets.  Like p5_clip.h it takes the place of the loss kernels behind the forward and hands the backward
// one seed per decoder row (the `dnll` route every loss kernel already has): a preference loss couples a user's G targets through their
// sequence log-probabilities, so its per-row weights exist only after the forward.
//
// A call carries B users x G targets x T positions (G <= 512).  Per target (b, g), with m_t = (out_attn != 0):
//   cnt = sum_t m_t,  s = sum_t m_t nll_t (the negative sequence log-probability),  r = sum_t m_t ref_t (0 when ref_lp is null),
//   Delta = (-s - r) / c',  c' = max(cnt, 1) under length_normalize, else 1;   h = beta Delta.
// The LIST of user b is its targets with pref_mask != 0 (null = all) and cnt > 0, in index order: the first listed target is the preferred
// one, the second the next, and so on.  Every other target is skipped: it contributes nothing, its seeds are exact zeros (by select) and its
// ref_lp is never read (ref_lp is read only where out_attn != 0, and only for targets with pref_mask != 0).  n_b = the list's length.
//   kind PL   depth D >= 1, or 0 = full.  For n_b >= 2: D_b = min(D or n_b - 1, n_b - 1),
//             l_b = sum_{k < D_b} (logsumexp_{j >= k} h_j - h_k) over list positions.  n_b = 2 is DPO's -log sigmoid(h_0 - h_1), D = 1 is
//             softmax-DPO's -log softmax_0(h), full depth is the Plackett-Luce likelihood of the order.
//             With L_k = logsumexp_{j >= k} h_j and A_j = logsumexp_{k <= min(j, D_b - 1)} (-L_k):  d l_b / d h_j = exp(h_j + A_j) - [j < D_b].
//   kind IPO  u_j = Delta_0 - Delta_j,  l_b = mean_{j = 1 .. n_b - 1} (u_j - 1 / (2 beta))^2.
//   Users with n_b < 2 have l_b = 0 exactly.  With n_b >= 1 the SFT term sft_b = sft_coef (sum_t m_t nll_t / max(cnt, 1)) of the FIRST listed
//   target is added.  loss = sum_b (l_b + sft_b) / B.
//   seed_t = d loss / d nll_t; 0 (by select) where labels == -100, where not attended, where the target is skipped.  The SFT part is formed as
//   p5_masked_mean_g_kernel forms its seed -- (1.0f / B) / max(cnt, 1), then *= sft_coef -- so a list of one target carries that kernel's bits.
// pref_stats fp32 [8]; "pairs" are the (first, j) pairs, j = 1 .. n_b - 1, of the users with n_b >= 2:
//   0 users with n_b >= 2, 1 share of pairs with h_first > h_j, 2 mean h_first over those users, 3 mean h_j over the pairs, 4 mean pair margin
//   h_first - h_j over the pairs, 5 the preference part of the loss (sum_b l_b / B), 6 the SFT part (sum_b sft_b / B), 7 mean n_b over the users
//   with n_b >= 1.  No user with a pair: 0 .. 4 are 0; no user with a listed target: 7 is 0.
//
//   p5_pref_objective_kernel   one workgroup (256 threads) per user.  (1) threads stride over the user's targets and walk their T positions in
//                              order: h and Delta go to LDS (512 floats each, -inf for skipped).  (2) thread i owns list slots 2 i, 2 i + 1:
//                              a SUFFIX scan over (max, sum, count) gives L_k, the list position of every slot and n_b; a PREFIX scan over
//                              (max, sum) of -L_k (k < D_b) gives A_j.  Both keep running maxima -- no global shift: a list whose head is 120
//                              nats above its tail keeps the tail (exp(-120) is 0 in fp32) -- and run as wave shuffles plus an LDS combine of
//                              the four waves, in index order.  d l_b / d Delta of every slot goes back to LDS.  (3) the strided threads write
//                              the seeds of their targets.  Writes the user's partials fp32 [16]: 0 l_b, 1 sft_b, 2 [n_b >= 2], 3 pairs,
//                              4 pairs with h_first > h_j, 5 h_first [n_b >= 2], 6 sum h_j, 7 sum margins, 8 [n_b >= 1], 9 n_b.
//   p5_pref_finish_kernel      one workgroup: users strided over the threads, then block_reduce; writes loss[0] and stats[8].
// No atomics; every value has one writer and every sum a fixed order: two runs return the same bits.
#pragma once
#include "p5_elem.h"

enum { P5_PREF_PL = 0, P5_PREF_IPO = 1 };
#define P5_PREF_PARTIALS 16
#define P5_PREF_MAX_G 512

struct P5PrefArgs {
  const float* nll; const float* ref_lp; const int64_t* out_attn; const int64_t* labels; const int* pref_mask;
  float* seed; float* partials;
  int G, T, kind, depth, length_normalize;
  float beta, sft_coef, inv_b;                  // inv_b = 1.0f / B
};

// a partial logsumexp (max, sum of exp relative to max) and a count; (-inf, 0, 0) is the identity
struct P5PrefAgg { float m, s, c; };

__device__ static __forceinline__ P5PrefAgg p5_pref_comb(P5PrefAgg a, P5PrefAgg b) {      // a: the lower indices
  P5PrefAgg r;
  r.m = fmaxf(a.m, b.m);
  r.c = a.c + b.c;
  r.s = r.m == P5_NEG_INF ? 0.f : a.s * expf(a.m - r.m) + b.s * expf(b.m - r.m);
  return r;
}
__device__ static __forceinline__ P5PrefAgg p5_pref_one(float h) { return P5PrefAgg{h, h == P5_NEG_INF ? 0.f : 1.f, h == P5_NEG_INF ? 0.f : 1.f}; }

// Exclusive scan over the workgroup's 256 threads of one aggregate per thread: the combination, in index order, of the aggregates of all
// threads below this one (rev: above).  Six shuffle steps inside a wave, then the four waves' totals through LDS (sw, 12 floats), which hold
// the block's total behind the call.  Called by all threads.
__device__ static __forceinline__ P5PrefAgg p5_pref_scan(P5PrefAgg v, bool rev, float* sw) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int src = rev ? lane + d : lane - d;
    P5PrefAgg o;
    o.m = __shfl(v.m, src & 63); o.s = __shfl(v.s, src & 63); o.c = __shfl(v.c, src & 63);
    if (src >= 0 && src < 64) v = rev ? p5_pref_comb(v, o) : p5_pref_comb(o, v);
  }
  const int nb = rev ? lane + 1 : lane - 1;
  P5PrefAgg ex;
  ex.m = __shfl(v.m, nb & 63); ex.s = __shfl(v.s, nb & 63); ex.c = __shfl(v.c, nb & 63);
  if (nb < 0 || nb > 63) ex = P5PrefAgg{P5_NEG_INF, 0.f, 0.f};
  __syncthreads();
  if (lane == (rev ? 0 : 63)) { sw[wave] = v.m; sw[4 + wave] = v.s; sw[8 + wave] = v.c; }
  __syncthreads();
  P5PrefAgg pre = {P5_NEG_INF, 0.f, 0.f};
  if (rev) {
    for (int w = 3; w > wave; --w) pre = p5_pref_comb(P5PrefAgg{sw[w], sw[4 + w], sw[8 + w]}, pre);
    return p5_pref_comb(ex, pre);
  }
  for (int w = 0; w < wave; ++w) pre = p5_pref_comb(pre, P5PrefAgg{sw[w], sw[4 + w], sw[8 + w]});
  return p5_pref_comb(pre, ex);
}

__global__ __launch_bounds__(256) void p5_pref_objective_kernel(P5PrefArgs a) {
  __shared__ float sh[P5_PREF_MAX_G], sd[P5_PREF_MAX_G], sw[12], sred[4], sfirst[2];
  const int b = blockIdx.x, tid = threadIdx.x, G = a.G, T = a.T;
  // (1) the target walk: thread tid has targets tid and tid + 256
  float cn[2] = {1.f, 1.f}, cp[2] = {1.f, 1.f}, sft[2] = {0.f, 0.f};
  if (tid == 0) { sfirst[0] = 0.f; sfirst[1] = 0.f; }      // (an empty list has no first)
  for (int i = 0; i < 2; ++i) {
    const int g = tid + 256 * i;
    float h = P5_NEG_INF, dl = P5_NEG_INF;
    if (g < G) {
      const size_t tg = (size_t)b * G + g, r0 = tg * T;
      const bool want = a.pref_mask ? a.pref_mask[tg] != 0 : true;
      const bool rd = want && a.ref_lp != nullptr;
      float num = 0.f, rs = 0.f, cnt = 0.f;
      int t = 0;
      for (; t + 4 <= T; t += 4) {                // four positions' loads in flight, then their use
        int64_t at[4]; float nl[4], rf[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { at[k] = a.out_attn[r0 + t + k]; nl[k] = a.nll[r0 + t + k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) rf[k] = (rd && at[k] != 0) ? a.ref_lp[r0 + t + k] : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float m = at[k] != 0 ? 1.f : 0.f;
          num += nl[k] * m; rs += rf[k]; cnt += m;
        }
      }
      for (; t < T; ++t) {
        const bool on = a.out_attn[r0 + t] != 0;
        const float m = on ? 1.f : 0.f;
        num += a.nll[r0 + t] * m;
        if (rd && on) rs += a.ref_lp[r0 + t];
        cnt += m;
      }
      cn[i] = fmaxf(cnt, 1.f);
      cp[i] = a.length_normalize ? cn[i] : 1.f;
      sft[i] = num / cn[i];
      if (want && cnt > 0.f) {
        dl = (-num - rs) / cp[i];
        h = a.beta * dl;
      }
    }
    sh[g] = h;
    sd[g] = dl;
  }
  __syncthreads();
  // (2) thread tid owns list slots 2 tid, 2 tid + 1
  const int e0 = 2 * tid;
  const float h0 = sh[e0], h1 = sh[e0 + 1], d0 = sd[e0], d1 = sd[e0 + 1];
  const bool on0 = h0 != P5_NEG_INF, on1 = h1 != P5_NEG_INF;
  const P5PrefAgg x0 = p5_pref_one(h0), x1 = p5_pref_one(h1);
  const P5PrefAgg above = p5_pref_scan(p5_pref_comb(x0, x1), true, sw);
  const P5PrefAgg suf1 = p5_pref_comb(x1, above), suf0 = p5_pref_comb(x0, suf1);      // slots >= e0 + 1, slots >= e0
  const float nb = (sw[8] + sw[9]) + (sw[10] + sw[11]);                                 // n_b (counts: exact)
  const float p0 = nb - suf0.c, p1 = nb - suf1.c;                                       // list positions
  const float Db = nb >= 2.f ? (a.depth > 0 ? fminf((float)a.depth, nb - 1.f) : nb - 1.f) : 0.f;
  if (on0 && p0 == 0.f) { sfirst[0] = h0; sfirst[1] = d0; }
  if (on1 && p1 == 0.f) { sfirst[0] = h1; sfirst[1] = d1; }
  float lpart = 0.f, g0 = 0.f, g1 = 0.f;      // l_b's terms of this thread, d l_b / d Delta of its two slots
  if (a.kind == P5_PREF_PL) {
    const float L0 = suf0.m + logf(suf0.s), L1 = suf1.m + logf(suf1.s);
    const bool act0 = on0 && p0 < Db, act1 = on1 && p1 < Db;
    const P5PrefAgg y0 = p5_pref_one(act0 ? -L0 : P5_NEG_INF), y1 = p5_pref_one(act1 ? -L1 : P5_NEG_INF);
    const P5PrefAgg below = p5_pref_scan(p5_pref_comb(y0, y1), false, sw);
    const P5PrefAgg pre0 = p5_pref_comb(below, y0), pre1 = p5_pref_comb(pre0, y1);
    if (nb >= 2.f) {
      if (on0) g0 = a.beta * (expf(h0 + (pre0.m + logf(pre0.s))) - (act0 ? 1.f : 0.f));
      if (on1) g1 = a.beta * (expf(h1 + (pre1.m + logf(pre1.s))) - (act1 ? 1.f : 0.f));
      if (act0) lpart += L0 - h0;
      if (act1) lpart += L1 - h1;
    }
  }
  __syncthreads();
  const float hf = sfirst[0], df = sfirst[1];
  float pairs = 0.f, wins = 0.f, sumh = 0.f, summ = 0.f, gfirst = 0.f;
  const bool pair0 = nb >= 2.f && on0 && p0 > 0.f, pair1 = nb >= 2.f && on1 && p1 > 0.f;
  if (pair0) { pairs += 1.f; wins += hf > h0 ? 1.f : 0.f; sumh += h0; summ += hf - h0; }
  if (pair1) { pairs += 1.f; wins += hf > h1 ? 1.f : 0.f; sumh += h1; summ += hf - h1; }
  if (a.kind == P5_PREF_IPO) {
    const float tau = 1.f / (2.f * a.beta), inv = 1.f / fmaxf(nb - 1.f, 1.f);
    if (pair0) { const float v = (df - d0) - tau; lpart += v * v * inv; g0 = -2.f * v * inv; gfirst += 2.f * v * inv; }
    if (pair1) { const float v = (df - d1) - tau; lpart += v * v * inv; g1 = -2.f * v * inv; gfirst += 2.f * v * inv; }
    gfirst = block_reduce(gfirst, false, sred);
    if (nb >= 2.f && on0 && p0 == 0.f) g0 = gfirst;
    if (nb >= 2.f && on1 && p1 == 0.f) g1 = gfirst;
  }
  lpart = block_reduce(lpart, false, sred);
  pairs = block_reduce(pairs, false, sred); wins = block_reduce(wins, false, sred);
  sumh = block_reduce(sumh, false, sred); summ = block_reduce(summ, false, sred);
  __syncthreads();
  // d l_b / d Delta of every slot, and the list position's two flags (listed, first), back through LDS to the threads that walk the targets
  sh[e0] = g0; sh[e0 + 1] = g1;
  sd[e0] = on0 ? (p0 == 0.f ? 2.f : 1.f) : 0.f; sd[e0 + 1] = on1 ? (p1 == 0.f ? 2.f : 1.f) : 0.f;
  __syncthreads();
  // (3) the seeds
  float sftb = 0.f;
  for (int i = 0; i < 2; ++i) {
    const int g = tid + 256 * i;
    if (g >= G) continue;
    const size_t r0 = ((size_t)b * G + g) * T;
    const float flag = sd[g];
    float gs = 0.f;
    if (flag != 0.f && nb >= 2.f) gs = (-sh[g] / cp[i]) * a.inv_b;        // d Delta / d nll_t = -1 / c'
    float gf = 0.f;
    if (flag == 2.f) {
      gf = a.inv_b / cn[i];
      gf *= a.sft_coef;
      sftb = a.sft_coef * sft[i];
    }
    const float on_seed = flag == 2.f ? (nb >= 2.f ? gs + gf : gf) : gs;
    for (int t = 0; t < T; ++t) {
      float gr = (flag != 0.f && a.out_attn[r0 + t] != 0) ? on_seed : 0.f;
      if (a.labels[r0 + t] == -100) gr = 0.f;
      a.seed[r0 + t] = gr;
    }
  }
  sftb = block_reduce(sftb, false, sred);       // (one thread's value, the others' zeros)
  if (tid == 0) {
    float* p = a.partials + (size_t)b * P5_PREF_PARTIALS;
    const bool two = nb >= 2.f;
    p[0] = two ? lpart : 0.f; p[1] = nb >= 1.f ? sftb : 0.f; p[2] = two ? 1.f : 0.f; p[3] = pairs; p[4] = wins; p[5] = two ? hf : 0.f;
    p[6] = sumh; p[7] = summ; p[8] = nb >= 1.f ? 1.f : 0.f; p[9] = nb;
    for (int i = 10; i < P5_PREF_PARTIALS; ++i) p[i] = 0.f;
  }
}

// loss[0] and stats[8] from the users' partials [B, 16]
__global__ __launch_bounds__(256) void p5_pref_finish_kernel(float* __restrict__ loss, float* __restrict__ stats, const float* __restrict__ partials, int B) {
  __shared__ float sred[4];
  float v[10];
  for (int i = 0; i < 10; ++i) v[i] = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* p = partials + (size_t)b * P5_PREF_PARTIALS;
    for (int i = 0; i < 10; ++i) v[i] += p[i];
  }
  for (int i = 0; i < 10; ++i) v[i] = block_reduce(v[i], false, sred);
  if (threadIdx.x == 0) {
    const float lp = v[0] / (float)B, ls = v[1] / (float)B;
    loss[0] = lp + ls;
    const float users = v[2], pairs = v[3];
    stats[0] = users;
    stats[1] = pairs > 0.f ? v[4] / pairs : 0.f;
    stats[2] = users > 0.f ? v[5] / users : 0.f;
    stats[3] = pairs > 0.f ? v[6] / pairs : 0.f;
    stats[4] = pairs > 0.f ? v[7] / pairs : 0.f;
    stats[5] = lp; stats[6] = ls;
    stats[7] = v[8] > 0.f ? v[9] / v[8] : 0.f;
  }
}
