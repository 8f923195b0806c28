// p5_item_head.h -- the tied head of the trie-normalised item loss RESTRICTED to the trie's tokens (p5_train_set_item_head).
//
// U = the sorted set of distinct tokens on the trie's edges, Nu = |U|, Nup = Nu rounded up to 64.  The item loss reads a row's logits at the
// children of one trie node only, so the head need not run over the vocabulary:
//   p5_item_gather_kernel    E_U [Nup, d] = the rows U of the head weight (bf16 shadow or fp32 master), rows [Nu, Nup) exact zeros;
//                            the head GEMM then writes logits_U [Md, Nup] instead of [Md, Vp]
//   (cross-entropy)          p5_trie_ce.h / p5_trunc.h with P5TrieCe::col set: a child's logit is logits_U[row, col[edge]], its gradient lands in
//                            dlogits_U[row, col[edge]]; labels, the walk and the exclusion bitmap stay on tokens and nodes
//   p5_item_scatter_kernel   dE_U [Nup, d] fp32 (one un-split GEMM, stored) into shared.weight's gradient [V, d]:
//                              store mode (P5_EPI_STORE regime: the arena is not cleared)  every row v < V: dE_U[col(v)] or zeros
//                              add mode (cleared arena or a later micro-batch)             rows U only: += dE_U
// Memory-bound row kernels: 16-byte accesses, one writer per element, no atomics; nothing at or behind row V is touched.
#pragma once
#include "p5_elem.h"

// one thread per 16-byte piece of E_U
template <class T>
__global__ __launch_bounds__(256) void p5_item_gather_kernel(T* __restrict__ EU, const T* __restrict__ E, const int* __restrict__ tokens, int Nu, int Nup,
                                                            int d) {
  constexpr int EPF = TT<T>::EPF;
  const int pieces = d / EPF;
  const long long n = (long long)Nup * pieces;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int r = (int)(i / pieces), p = (int)(i - (long long)r * pieces);
    u32x4 v = zero16();
    if (r < Nu) v = ld16(E + (size_t)tokens[r] * d + (size_t)p * EPF);
    st16(EU + (size_t)r * d + (size_t)p * EPF, v);
  }
}

// the column of token v in the ascending list `tokens`, -1 when it is not there
__device__ static __forceinline__ int p5_item_col(const int* __restrict__ tokens, int Nu, int v) {
  int lo = 0, hi = Nu - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tokens[mid] < v) lo = mid + 1; else hi = mid;
  }
  return tokens[lo] == v ? lo : -1;
}

// one thread per 16-byte piece of a target row.  store != 0: rows [0, V) of dE, all of them; store == 0: the rows U, read-add-write
__global__ __launch_bounds__(256) void p5_item_scatter_kernel(float* __restrict__ dE, const float* __restrict__ dEU, const int* __restrict__ tokens, int Nu,
                                                             int V, int d, int store) {
  const int pieces = d / 4;
  const long long n = (long long)(store ? V : Nu) * pieces;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int r = (int)(i / pieces), p = (int)(i - (long long)r * pieces);
    if (store) {
      const int c = p5_item_col(tokens, Nu, r);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (c >= 0) v = *(const f32x4*)(dEU + (size_t)c * d + (size_t)p * 4);
      *(f32x4*)(dE + (size_t)r * d + (size_t)p * 4) = v;
    } else {
      float* q = dE + (size_t)tokens[r] * d + (size_t)p * 4;
      const f32x4 a = *(const f32x4*)q, b = *(const f32x4*)(dEU + (size_t)r * d + (size_t)p * 4);
      *(f32x4*)q = a + b;
    }
  }
}
