// p5_embed.h -- gradient of the embedding lookups (SURVEY.md App. C "Embedding lookups"; P5_T5.py:94-100 encoder: E[ids] + WW[ww],
// decoder: E[dec_ids]; the three contributions to the tied shared.weight are the head GEMM and these two lookups) WITHOUT fp32 atomics.
//
// Rounds 1-3 scattered every row of the residual-stream gradient into its table row with one fp32 atomic per element.  The order the
// atomics of a repeated token land in changes from run to run, the last bits of shared.weight's gradient with it, and AdamW turns a
// last-bit difference of a near-zero gradient into an O(lr) difference of the parameter (tools/diag_repro.py,
// profiles/r04_repro_before_fix.txt): two runs of the same training differed by up to 2 x lr.  Here the rows are summed in a FIXED order:
//   1. p5_embed_sortchunk_kernel + p5_embed_rank_kernel
//                               stable rank of every lookup row by (key, row): sorted position, start and length of its key's segment
//                               (chunks of 256 rows sorted in LDS, then binary searches per row and chunk -- integer comparisons only);
//   2. p5_embed_seg_kernel      one workgroup per block of 32 sorted positions: rows of one key are added in row order; a segment that
//                               lies inside the block is added to the table row by its only owner (plain read-modify-write), pieces of
//                               segments that cross block boundaries go to a partial buffer;
//   3. p5_embed_fix_kernel      the block in which a crossing segment starts adds its pieces in block order and updates the table row.
// The same association on every run -> bit-identical gradients.  A key set may be the concatenation of two index arrays (encoder ids
// followed by the decoder's shifted labels, both looking up the tied table): the tied table then has ONE owner per row.
#pragma once
#include "p5_device.h"
#include "p5_rng.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
#define P5_EMB_SEG 32          // sorted positions per workgroup of the segmented sum
#define P5_EMB_MAXSETS 2

struct P5EmbSet {
  const int64_t* key0; const int64_t* key1;     // virtual concatenation: row r < n0 looks up key0[r], else key1[r - n0]
  const float* dres0; const float* dres1;       // [n0, d] / [n1, d] fp32 gradients of the looked-up rows
  P5Drop drop0, drop1;                          // dropout applied to the looked-up rows in the forward (element index = local row * d + c)
  float* table;                                 // gradient of the table, += (row-major [*, d])
  int n0, n1;
  int* perm; int* sstart; int* slen;            // [n] sorted position -> row, start / length of the position's key segment
  int* skey;                                    // [n] sorted position -> key
  unsigned long long* csort;                    // [ceil(n / 256) * 256] scratch: (key << 32 | row), sorted inside each chunk of 256 rows
  float* part;                                  // [blocks][2][d] pieces of segments crossing block boundaries (0: continues from before, 1: continues after)
};
struct P5EmbArgs {
  P5EmbSet s[P5_EMB_MAXSETS];
  int nsets, d;
};

__device__ static __forceinline__ int emb_key(const P5EmbSet& s, int r) { return (int)(r < s.n0 ? s.key0[r] : s.key1[r - s.n0]); }

// Stable rank by (key, row) in two levels -- O(n (log c + (n / c) log c)) instead of the n^2 / 2 comparisons of a brute-force count
// (which took 98 us at n = 8704 and would take milliseconds at the 33k rows of a T5-large, L = 512 batch):
//   p5_embed_sortchunk_kernel   one workgroup per chunk of 256 rows: bitonic sort of the composite 64-bit values (key << 32 | row) in LDS
//                               -> `csort` (sorted chunks, back to back);
//   p5_embed_rank_kernel        one thread per row: its rank = sum over ALL chunks of the number of values below its own (a binary
//                               search per chunk, chunks staged through LDS), likewise the start and the end of its key's segment
//                               (values below key << 32 / below (key + 1) << 32); the three searches of two chunks run in lockstep.
// Integer comparisons only: the same permutation on every run.
#define P5_EMB_CHUNK 256
__global__ __launch_bounds__(256) void p5_embed_sortchunk_kernel(P5EmbArgs a) {
  __shared__ unsigned long long sv[P5_EMB_CHUNK];
  const P5EmbSet& s = a.s[blockIdx.y];
  const int n = s.n0 + s.n1;
  const int r = blockIdx.x * P5_EMB_CHUNK + threadIdx.x;
  if (blockIdx.x * P5_EMB_CHUNK >= n) return;
  sv[threadIdx.x] = r < n ? (((unsigned long long)(unsigned)emb_key(s, r)) << 32) | (unsigned)r : ~0ull;      // (padding sorts last)
  __syncthreads();
  for (int k = 2; k <= P5_EMB_CHUNK; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int i = threadIdx.x, l = i ^ j;
      if (l > i) {
        const unsigned long long x = sv[i], y = sv[l];
        const bool up = (i & k) == 0;
        if ((x > y) == up) { sv[i] = y; sv[l] = x; }
      }
      __syncthreads();
    }
  }
  s.csort[(size_t)blockIdx.x * P5_EMB_CHUNK + threadIdx.x] = sv[threadIdx.x];
}

// number of values of the sorted chunk v[0..256) that are < x: eight halving steps over v[0..255), then the last value.  No branch and no
// data-dependent trip count, so several searches written side by side advance in lockstep and their LDS reads overlap.
__device__ static __forceinline__ void emb_count_below(const unsigned long long* const (&v)[2], const unsigned long long (&x)[3], int (&cnt)[2][3]) {
  int p[2][3] = {};
#pragma unroll
  for (int s = P5_EMB_CHUNK / 2; s > 0; s >>= 1) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int q = 0; q < 3; ++q) p[h][q] += v[h][p[h][q] + s - 1] < x[q] ? s : 0;
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < 3; ++q) cnt[h][q] = p[h][q] + (v[h][p[h][q]] < x[q] ? 1 : 0);
  }
}

typedef unsigned long long emb_u64x2 __attribute__((ext_vector_type(2), aligned(8)));

// grid (ceil(max n / 64), nsets), 256 threads: lane = one of 64 rows, wave w searches the chunks c = w (mod 4) of every LDS batch
// (16 sorted chunks = 32 KiB at a time); the four waves' counts are added through LDS.
// A batch is fetched with eight 16-byte loads per thread that are all in flight together (clamped addresses: the tail of a short last batch
// re-reads the batch's first pair and lands in LDS nobody searches), and the next batch is requested before the current one is searched.
// A wave takes two chunks at a time and runs their six counts (values below key << 32, below (key + 1) << 32, below the row's own value) as
// one lockstep search of nine dependent LDS reads.  (Until round 7 the staging loop waited for each of its 8-byte loads before issuing
// the next -- 34 dependent round trips to L2 per workgroup at n = 8704 -- and the three counts of a chunk were three searches one after the
// other, about 17 dependent LDS reads per chunk; the counts, and with them perm / skey / sstart / slen, are the same integers.)
__global__ __launch_bounds__(256) void p5_embed_rank_kernel(P5EmbArgs a) {
  constexpr int CPB = 16;                 // chunks per LDS batch
  constexpr int NLD = CPB * P5_EMB_CHUNK / 2 / 256;      // 16-byte loads per thread and batch
  __shared__ __attribute__((aligned(16))) unsigned long long sc[CPB * P5_EMB_CHUNK];
  __shared__ int scnt[3][4][64];
  const P5EmbSet& s = a.s[blockIdx.y];
  const int n = s.n0 + s.n1;
  if (blockIdx.x * 64 >= n) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 64 + lane;
  const int k = r < n ? emb_key(s, r) : 0;
  const unsigned long long x[3] = {((unsigned long long)(unsigned)k) << 32, ((unsigned long long)(unsigned)k + 1ull) << 32,
                                   (((unsigned long long)(unsigned)k) << 32) | (unsigned)r};      // start, end, own position
  const int nchunks = (n + P5_EMB_CHUNK - 1) / P5_EMB_CHUNK;
  emb_u64x2 t[NLD];
  auto fetch = [&](int c0) {
    const int lim = (nchunks - c0 < CPB ? nchunks - c0 : CPB) * P5_EMB_CHUNK;
    const unsigned long long* src = s.csort + (size_t)c0 * P5_EMB_CHUNK;
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int i = (q * 256 + (int)threadIdx.x) * 2;
      t[q] = *(const emb_u64x2*)(src + (i < lim ? i : 0));
    }
  };
  fetch(0);
  int tot[3] = {0, 0, 0};
  for (int c0 = 0; c0 < nchunks; c0 += CPB) {
    const int nc = nchunks - c0 < CPB ? nchunks - c0 : CPB;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NLD; ++q) *(emb_u64x2*)(sc + (q * 256 + (int)threadIdx.x) * 2) = t[q];
    __syncthreads();
    if (c0 + CPB < nchunks) fetch(c0 + CPB);      // (uniform) lands while this batch is searched
    for (int c = wave; c < nc; c += 8) {
      const bool two = c + 4 < nc;                // (uniform)
      const unsigned long long* const v[2] = {sc + c * P5_EMB_CHUNK, sc + (two ? c + 4 : c) * P5_EMB_CHUNK};
      int cnt[2][3];
      emb_count_below(v, x, cnt);                 // (padding values ~0 are above every real value)
#pragma unroll
      for (int q = 0; q < 3; ++q) tot[q] += cnt[0][q] + (two ? cnt[1][q] : 0);
    }
  }
  scnt[0][wave][lane] = tot[2]; scnt[1][wave][lane] = tot[0]; scnt[2][wave][lane] = tot[1];
  __syncthreads();
  if (wave == 0 && r < n) {
    const int pos = scnt[0][0][lane] + scnt[0][1][lane] + scnt[0][2][lane] + scnt[0][3][lane];
    const int start = scnt[1][0][lane] + scnt[1][1][lane] + scnt[1][2][lane] + scnt[1][3][lane];
    const int end = scnt[2][0][lane] + scnt[2][1][lane] + scnt[2][2][lane] + scnt[2][3][lane];
    s.perm[pos] = r; s.skey[pos] = k; s.sstart[pos] = start; s.slen[pos] = end - start;
  }
}

typedef float emb_f4 __attribute__((ext_vector_type(4), aligned(4)));      // 16-byte access of four columns (rows are only known to be float-aligned)
// a pointer read back from LDS has lost its address space: say "global" again, or the loads are compiled as flat ones
#ifdef P5_EMU
#define EMB_GLOBAL
#else
#define EMB_GLOBAL __attribute__((address_space(1)))
#endif

// 0 in a vector register the compiler cannot see through: an LDS index `j + emb_vzero()` keeps what is read there in vector registers.
// (Read with a plain constant index, the 64 staged row pointers of a block are all moved to scalar registers, which do not hold them:
// the compiled kernel spilled several hundred of them into lanes of vector registers.)
__device__ static __forceinline__ int emb_vzero() {
  int z = 0;
#ifndef P5_EMU
  asm volatile("" : "+v"(z));
#endif
  return z;
}

// one half (positions H0 .. H0 + 15) of a block of p5_embed_seg_kernel, columns c..c+3: all loads, then dropout, then the adds
template <int H0>
__device__ static __forceinline__ void emb_seg_half(const P5EmbSet& s, const float* const* srow, const float* const* sown, const int* slr, const int* sk,
                                                    const int* sst, const int* sln, int p0, int cnt, int d, int c, int z, uint32_t seed0, uint32_t seed1,
                                                    bool use0, bool use1, float (&acc)[4]) {
  constexpr int S = P5_EMB_SEG, HB = S / 2;
  emb_f4 v[HB], o[HB];
#pragma unroll
  for (int i = 0; i < HB; ++i) v[i] = *(const EMB_GLOBAL emb_f4*)(srow[H0 + i + z] + c);
#pragma unroll
  for (int i = 0; i < HB; ++i) o[i] = *(const EMB_GLOBAL emb_f4*)(sown[H0 + i + z] + c);
  P5_SCHED_FENCE();                               // (the scalar work of the dropout and of the adds stays below the loads)
  if (use0 || use1) {                             // (uniform) the forward's dropout, same element index and scale
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      const int lr = slr[H0 + i];                 // local row; bit 31 set: a row of the second key array
      const bool first = lr >= 0;
      if (first ? use0 : use1) {                  // (uniform)
        const uint32_t seed = first ? seed0 : seed1, site_key = first ? s.drop0.site_key : s.drop1.site_key;
        const uint32_t thr = first ? s.drop0.thr : s.drop1.thr;
        const float scale = first ? s.drop0.scale : s.drop1.scale;
        const uint32_t i0 = (uint32_t)((lr & 0x7fffffff) * d + c);
        v[i].x = p5_keep(seed, site_key, i0, thr) ? v[i].x * scale : 0.f;
        v[i].y = p5_keep(seed, site_key, i0 + 1, thr) ? v[i].y * scale : 0.f;
        v[i].z = p5_keep(seed, site_key, i0 + 2, thr) ? v[i].z * scale : 0.f;
        v[i].w = p5_keep(seed, site_key, i0 + 3, thr) ? v[i].w * scale : 0.f;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < HB; ++i) {
    const int j = H0 + i;
    if (j < cnt) {                                // (uniform)
      acc[0] += v[i].x; acc[1] += v[i].y; acc[2] += v[i].z; acc[3] += v[i].w;
      if (sk[j + 1] != sk[j]) {                   // (uniform) the last row of its key in this block
        const int ss = sst[j], se = ss + sln[j];
        const bool head = ss < p0, tail = se > p0 + S;
        if (!head && !tail) {
          *(emb_f4*)(s.table + (size_t)sk[j] * d + c) = (emb_f4){o[i].x + acc[0], o[i].y + acc[1], o[i].z + acc[2], o[i].w + acc[3]};
        } else {
          *(emb_f4*)(s.part + ((size_t)blockIdx.x * 2 + (head ? 0 : 1)) * d + c) = (emb_f4){acc[0], acc[1], acc[2], acc[3]};
        }
        acc[0] = 0.f; acc[1] = 0.f; acc[2] = 0.f; acc[3] = 0.f;
      }
    }
  }
}

// grid (ceil(max n / 32), nsets), 256 threads = 1024 columns per pass (four per thread).
// The block's 32 positions are handled as two halves of 16.  A half first REQUESTS everything it reads -- its 16 gradient rows and the
// table rows of the segments that end in it and lie inside the block (distinct keys, this workgroup their only writer) -- and only then
// adds.  For that the loads carry no control flow: the first 32 threads work out one row pointer and one table-row pointer per position
// and stage them in LDS; a position past the end of the set repeats the set's last position, a position that owns no table row requests
// its own gradient row a second time (a cache hit), and dropout is applied to the registers after the loads.  (Until round 7 the loop
// read "every row is requested before the first add", but the guards `if (j < cnt)`, `if (last)` and the per-row choice of the dropout
// descriptor were branches, and the compiled kernel waited for every one of its 64 loads before issuing the next: 64 dependent round
// trips per workgroup, 48 us per launch at the C2 shape for 35 MB of reads.)
// The association is unchanged: rows of a key are added in sorted order starting from 0; a segment inside the block writes
// table_old + a; a piece of a segment that crosses a block boundary goes to part[block][0 (continues from before) | 1 (continues after)].
__global__ __launch_bounds__(256) void p5_embed_seg_kernel(P5EmbArgs a) {
  constexpr int S = P5_EMB_SEG;
  __shared__ const float* srow[S];
  __shared__ const float* sown[S];
  __shared__ int slr[S], sk[S + 1], sst[S], sln[S];
  const P5EmbSet& s = a.s[blockIdx.y];
  const int n = s.n0 + s.n1, d = a.d;
  const int p0 = blockIdx.x * S;
  if (p0 >= n) return;
  const int cnt = n - p0 < S ? n - p0 : S;
  if (threadIdx.x < S) {
    const int t = threadIdx.x;
    const bool ok = t < cnt;
    const int p = p0 + (ok ? t : cnt - 1);        // (clamped: a padding position names a row that exists)
    const int r = s.perm[p], key = s.skey[p], ss = s.sstart[p], ln = s.slen[p];
    const int next = t + 1 < cnt ? s.skey[p + 1] : -1;
    const bool first = r < s.n0;
    const int lr = first ? r : r - s.n0;
    const float* src = (first ? s.dres0 : s.dres1) + (size_t)lr * d;
    const bool own = ok && next != key && ss >= p0 && ss + ln <= p0 + S;
    srow[t] = src; sown[t] = own ? s.table + (size_t)key * d : src;
    slr[t] = first ? lr : (lr | (int)0x80000000);
    sk[t] = ok ? key : -1; sst[t] = ss; sln[t] = ln;
    if (t == 0) sk[S] = -1;
  }
  __syncthreads();
  const uint32_t seed0 = p5_seed(s.drop0), seed1 = p5_seed(s.drop1);
  const bool use0 = s.drop0.state != nullptr && s.drop0.thr != 0, use1 = s.drop1.state != nullptr && s.drop1.thr != 0;
  const int z = emb_vzero();
  for (int c = threadIdx.x * 4; c < d; c += 1024) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    emb_seg_half<0>(s, srow, sown, slr, sk, sst, sln, p0, cnt, d, c, z, seed0, seed1, use0, use1, acc);
    if (cnt > S / 2) emb_seg_half<S / 2>(s, srow, sown, slr, sk, sst, sln, p0, cnt, d, c, z, seed0, seed1, use0, use1, acc);      // (uniform)
  }
}

// grid (ceil(max n / 32), nsets): the block in which a boundary-crossing segment STARTS owns it
__global__ __launch_bounds__(256) void p5_embed_fix_kernel(P5EmbArgs a) {
  constexpr int S = P5_EMB_SEG;
  const P5EmbSet& s = a.s[blockIdx.y];
  const int n = s.n0 + s.n1, d = a.d;
  const int p0 = blockIdx.x * S;
  if (p0 + S >= n) return;                        // (the last block has no successor to cross into)
  const int last = p0 + S - 1;
  const int ss = s.sstart[last], se = ss + s.slen[last];
  if (se <= p0 + S || ss < p0) return;            // does not cross, or started in an earlier block (uniform)
  const int key = s.skey[last];
  const int b1 = (se - 1) / S;                    // last block holding a piece (its piece is a "continues from before" piece: slot 0)
  for (int c = threadIdx.x * 2; c < d; c += 512) {
    const float* p = s.part + ((size_t)blockIdx.x * 2 + 1) * d + c;
    float a0 = p[0], a1 = p[1];
    int b = blockIdx.x + 1;
    for (; b + 3 <= b1; b += 4) {                 // four pieces in flight, added in block order
      const float* q0 = s.part + (size_t)b * 2 * d + c;
      const float x00 = q0[0], x01 = q0[1], x10 = q0[2 * d], x11 = q0[2 * d + 1], x20 = q0[4 * d], x21 = q0[4 * d + 1], x30 = q0[6 * d], x31 = q0[6 * d + 1];
      a0 = (((a0 + x00) + x10) + x20) + x30;
      a1 = (((a1 + x01) + x11) + x21) + x31;
    }
    for (; b <= b1; ++b) {
      const float* q = s.part + (size_t)b * 2 * d + c;
      a0 += q[0]; a1 += q[1];
    }
    float* dst = s.table + (size_t)key * d + c;
    dst[0] += a0; dst[1] += a1;
  }
}
