// p5_rng.h -- counter-based dropout RNG.  keep(seed, site, idx) is a pure function, so forward and
// backward regenerate the same mask without storing it, and oracle/t5_oracle.py::dropout_keep_mask
// reproduces it bit-for-bit on the CPU for train-mode parity tests.
// The reference draws one Bernoulli mask per dropout site (P5_T5.py:125,180; HF modeling_t5.py:86,140,168,
// 400,431) from torch's Philox stream; bitwise parity with torch's stream is impossible,
// only the distribution (keep prob 1-p, scale 1/(1-p)) is matched.
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif

__host__ __device__ static inline uint32_t p5_mix32(uint32_t x) {  // "lowbias32"
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ static inline uint32_t p5_site_key(uint32_t site) { return site * 0x85EBCA6Bu + 0x27D4EB2Fu; }
// keep(seed, site, idx): ONE mixing round per element -- the (seed, site) part is mixed separately and is loop-invariant
// (wave-uniform, hoisted by the compiler), so an element costs an xor and lowbias32's two 32-bit multiplies.  32-bit integer
// multiplies are quarter-rate on CDNA; the first version (idx * odd + seed -> mix -> xor site -> mix: five of them per element)
// made the dropout epilogues of the GEMMs and the attention kernels VALU-bound.
__host__ __device__ static inline bool p5_keep(uint32_t seed, uint32_t site_key, uint32_t idx, uint32_t thr) {
  const uint32_t h = p5_mix32(idx ^ p5_mix32(seed + site_key));
  return (h >> 8) >= thr;
}
__host__ static inline uint32_t p5_drop_thr(float p) { return (uint32_t)(p * 16777216.0f); }

// dropout descriptor passed by value to kernels; seed comes from device memory so a captured hipGraph
// replays with a fresh seed every step (state[0] = base seed, state[1] = step counter).
struct P5Drop {
  const uint32_t* state;  // device pointer or nullptr (=> no dropout)
  uint32_t site_key;
  uint32_t thr;
  float scale;  // 1/(1-p)
};
__device__ static inline uint32_t p5_seed(const P5Drop& d) {
  return d.state ? (d.state[0] + d.state[1] * 0x632BE5ABu) : 0u;
}

// ---- uniforms of trie-constrained sampling (p5_sample.h).  This comment is the specification; tests restate it in Python. ----
// The uniform of one Gumbel is a pure function of five coordinates: the call's seed, the user's stream id, the draw index of the row
// (draw_base + row within the user), the step (position of the token being drawn in the sequence: 1 = the first token behind the decoder
// start) and the child's position in the node's CSR list.  One p5_mix32 round per coordinate, NESTED -- every coordinate enters the output
// of the previous round -- so that two distinct coordinate tuples cannot cancel the way a sum or xor of independent terms can:
//   k = mix32(seed ^ mix32(stream * 0x9E3779B1 + 0x7F4A7C15))
//   k = mix32(k ^ draw)
//   k = mix32(k + 0x9E3779B9 * (step + 1))          <- p5_sample_row_key: uniform over a decode row, computed once per row and step
//   h = mix32(k ^ child)
//   u = ((h >> 9) + 0.5) * 2^-23                    <- p5_sample_uniform
// All integer arithmetic is modulo 2^32.  u takes the 2^23 values (j + 0.5) / 2^23: each is exact in fp32 (24 significant bits), so
// 2^-24 <= u <= 1 - 2^-24 and u is never 0 or 1; with 24 hash bits, (h >> 8) + 0.5f would round to 2^24 for the largest j and give u = 1.
// The Gumbel of the child is g = -logf(-logf(u)).
// Stochastic beam search (p5_sbs.h) uses the same two functions with other coordinates: `draw` is the slate index (slate_base + slate
// within the user) and `child` is the GLOBAL CSR edge index of the child (child_off[node] + position).  The position alone is not enough
// there: two beams of one slate sit at different nodes in the same step and must not share noise.  In a tree-shaped trie an edge is
// reached by one prefix, so every (slate, step, edge) names one Gumbel, whatever the beam slot its parent occupies.
__host__ __device__ static inline uint32_t p5_sample_row_key(uint32_t seed, uint32_t stream, uint32_t draw, uint32_t step) {
  uint32_t k = p5_mix32(seed ^ p5_mix32(stream * 0x9E3779B1u + 0x7F4A7C15u));
  k = p5_mix32(k ^ draw);
  return p5_mix32(k + 0x9E3779B9u * (step + 1u));
}
__host__ __device__ static inline float p5_sample_uniform(uint32_t row_key, uint32_t child) {
  const uint32_t h = p5_mix32(row_key ^ child);
  return ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
}

// site numbering (shared with oracle.t5_oracle.site_id)
static inline uint32_t p5_site_id(int stack, int layer, int which) { return (uint32_t)((stack * 64 + layer) * 8 + which); }
