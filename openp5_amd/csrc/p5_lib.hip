// p5_lib.hip -- host side of libp5hip.so: kernel launchers, the T5 engine (forward / backward / generate
// orchestration over one HIP stream) and the C ABI declared in include/p5hip.h.
//
// The engine replaces the Python object `P5_T5` (model/P5_T5.py:207) + HF T5ForConditionalGeneration + autograd:
// it owns no memory; parameters live in ONE flat fp32 arena (plus a bf16 shadow in fast mode), gradients in a
// second arena of the same layout (so clip + AdamW are two flat kernels and DDP buckets are contiguous
// ranges), activations in a caller-provided workspace.
#include <string>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#ifndef P5_EMU
#include <dlfcn.h>
#endif

#include "p5_host.h"
#include "p5_elem.h"
#include "p5_embed.h"
#include "p5_decode.h"
#include "p5_decode2.h"
#include "p5_decode_wide.h"
#include "p5_verify.h"
#include "p5_rank.h"
#include "p5_cand.h"
#include "p5_prune.h"
#include "p5_bound.h"
#include "p5_sample.h"
#include "p5_sbs.h"
#include "p5_trie_ce.h"
#include "p5_trie_reg.h"
#include "p5_item_head.h"
#include "p5_trunc.h"
#include "p5_policy.h"
#include "p5_slate_policy.h"
#include "p5_clip.h"
#include "p5_pref.h"
#include "../../include/p5hip.h"

thread_local std::string g_p5_err;

// =====================================================================================================
// launchers
// =====================================================================================================
// tuning knobs (p5_set_option / environment) of the engine and the decode step; the GEMM / attention families keep theirs in their own units
static int g_opt_wgrad_group = getenv("P5_WGRAD_GROUP") ? atoi(getenv("P5_WGRAD_GROUP")) : 1;   // layer-grouped deferred weight gradients (bf16)
static int g_opt_dec_nb = getenv("P5_DEC_NB") ? atoi(getenv("P5_DEC_NB")) : 0;           // skinny GEMM: forced column-tile width (0 = auto)
static int g_opt_dec_kw = getenv("P5_DEC_KW") ? atoi(getenv("P5_DEC_KW")) : 0;           // skinny GEMM: forced K range per workgroup (0 = auto)
static int g_opt_dec_fuseq = getenv("P5_DEC_FUSEQ") ? atoi(getenv("P5_DEC_FUSEQ")) : 1;   // cross-attention computes its own q projection
static int g_opt_dgrad_t = getenv("P5_DGRAD_T") ? atoi(getenv("P5_DGRAD_T")) : 1;       // data gradients on the transposed weight copy when one is bound
static int g_opt_dec_cross = getenv("P5_DEC_CROSS") ? atoi(getenv("P5_DEC_CROSS")) : 3;   // 3 = MFMA cross-attention, 2 = scalar score / PV loops
static int g_opt_dec_head = getenv("P5_DEC_HEAD") ? atoi(getenv("P5_DEC_HEAD")) : 1;      // 1 = streaming head (no [R, V] logits), 0 = GEMM + score kernel
static int g_opt_dec_atomic = getenv("P5_DEC_ATOMIC") ? atoi(getenv("P5_DEC_ATOMIC")) : 0;   // 1 = round-2..4 decode step: residual stream updated with fp32 atomics by K-split workgroups (not bit-reproducible)
static int g_opt_adam_tiles = getenv("P5_ADAM_TILES") ? atoi(getenv("P5_ADAM_TILES")) : 1;       // p5_engine_adamw_step: tile-wise update that also writes W^T and W diag(ln)
static int g_opt_gen_ff = getenv("P5_GEN_FF") ? atoi(getenv("P5_GEN_FF")) : 1;             // forced-prefix fast-forward (p5_decode.h): 0 = every step is a decode step
static int g_opt_dec_head_nv = getenv("P5_DEC_HEAD_NV") ? atoi(getenv("P5_DEC_HEAD_NV")) : 0;   // streaming head: forced E rows per workgroup (0 = auto)
static int g_opt_shift_fuse = getenv("P5_SHIFT_FUSE") ? atoi(getenv("P5_SHIFT_FUSE")) : 1;   // 1 = the decoder's embedding lookup shifts the labels itself (no p5_shift_right_kernel launch)
static int g_opt_loss_fuse = getenv("P5_LOSS_FUSE") ? atoi(getenv("P5_LOSS_FUSE")) : 1;      // 1 = the loss kernel of p5_forward_loss* also writes the NLL gradients (no p5_ce_gscale_kernel launch in the backward)
static int g_opt_gen_wide = getenv("P5_GEN_WIDE") ? atoi(getenv("P5_GEN_WIDE")) : 0;       // 1 = the wide search (p5_decode_wide.h) at every width, not only K > 64

__global__ __launch_bounds__(256) void p5_shift_right_kernel(int64_t* out, const int64_t* labels, int B, int T, int64_t start) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * T) return;
  const int t = i % T;
  int64_t v = (t == 0) ? start : labels[i - 1];
  if (v == -100) v = start;
  out[i] = v;
}

// p5_masked_mean_kernel that also writes g_out [B * T] = what p5_ce_gscale_kernel writes without dnll (the gradient of this loss with
// respect to the per-token NLL, gscale = 1 / B in the engine): the same expressions on the same operands, so the same bits, and the
// backward of p5_forward_loss* needs no launch of its own for them
__global__ __launch_bounds__(256) void p5_masked_mean_g_kernel(float* __restrict__ loss, float* __restrict__ g_out, const float* __restrict__ nll,
                                                              const int64_t* __restrict__ out_attn, const int64_t* __restrict__ labels, int B, int T,
                                                              float gscale, const float* __restrict__ tw = nullptr) {
  __shared__ float sred[4];
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    float num = 0.f, cnt = 0.f;
    for (int t = 0; t < T; ++t) {
      const float m = out_attn[(size_t)b * T + t] != 0 ? 1.f : 0.f;
      num += nll[(size_t)b * T + t] * m;
      cnt += m;
    }
    float r = num / fmaxf(cnt, 1.f);
    if (tw) r *= tw[b];
    s += r;
    for (int t = 0; t < T; ++t) {
      float g = out_attn[(size_t)b * T + t] != 0 ? gscale / fmaxf(cnt, 1.f) : 0.f;
      if (tw) g *= tw[b];
      if (labels[(size_t)b * T + t] == -100) g = 0.f;
      g_out[(size_t)b * T + t] = g;
    }
  }
  s = block_reduce(s, false, sred);
  if (threadIdx.x == 0) loss[0] = s / (float)B;
}

__global__ __launch_bounds__(64) void p5_tr_probe_kernel(unsigned short* out, const unsigned short* in) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[256];
  const int l = threadIdx.x;
  for (int i = l; i < 256; i += 64) lds[i] = in[i];
  __syncthreads();
  // 16-lane group g reads the [4][16] block starting at element g*64, lane i -> row i/4, cols (i%4)*4..
  const u32x2 r = lds_tr16_b64(&lds[(l >> 4) * 64 + (l & 15) * 4]);
  out[l * 4 + 0] = (unsigned short)(r[0] & 0xFFFF);
  out[l * 4 + 1] = (unsigned short)(r[0] >> 16);
  out[l * 4 + 2] = (unsigned short)(r[1] & 0xFFFF);
  out[l * 4 + 3] = (unsigned short)(r[1] >> 16);
}

// =====================================================================================================
// engine
// =====================================================================================================
static constexpr int P5_MAX_STAGED = 160;     // final gradient ranges of one staged backward (<= stages: n_dec + n_enc + 4)
static constexpr int P5_NSETS = 8;      // >= 2 x (sub-layers of a decoder layer), >= 2 x (sub-layers of the encoder layers grouped into one launch)
struct ParamInfo { std::string name; int64_t off; int rows, cols; };
struct AttnOff { int64_t q, k, v, o, ln; };
struct LayerOff { AttnOff sa, ca; int64_t wi, wo, ff_ln; int64_t begin, end; };

struct LayerSave {
  void *x_sa, *n_sa, *qkv, *o_sa; float *rstd_sa, *lse_sa;
  void *x_ca, *n_ca, *q_ca, *kv_ca, *o_ca; float *rstd_ca, *lse_ca;
  void *x_ff, *n_ff, *u_ff, *h_ff; float *rstd_ff;
  float *ssq_sa, *ssq_ca, *ssq_ff;     // [rows, d/64] partial sums of squares of x_sa / x_ca / x_ff (norm folded into the GEMMs)
  uint32_t* keep_sa;                   // dropout keep masks of the self-attention probabilities (P5AttnArgs::keep_bits) or nullptr
};

struct Bump {
  char* base; size_t off;
  void* take(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};

struct GraphKey { int B, L, K, max_len, max_c, excl_words; const void *ws, *trie, *trie_tok, *trie_node, *roots, *P, *S, *hist; int sz, fused, wide; };

struct GenWs {
  void* kv_cross[64];   // per decoder layer: T [B*L, ldkv] -- column slices of ONE [B*L, n_dec*2*inner] block
  int ldkv;             // (all layers' K/V projections are a single GEMM, as in training)
  void* cache[64];      // per decoder layer: T [max_len, R, 2*inner]
  void *qkv, *q, *o, *h, *hn;
  float* x32;             // [R, d] fp32 residual stream of the decode step (dec_atomic: updated in place with atomics)
  float *logits, *cand, *row_top_score; int *n_cand, *row_top_c;
  float *part_m, *part_s; int* cand_key;   // streaming head: per (row, vocabulary tile) max / sum exp; candidate keys of pools beyond the LDS budget
  int64_t* mask_copy;
  uint32_t* excluded;     // [B, excl_words] copy of the caller's per-item excluded-node bitmap (stable address for the graph)
  int64_t* ff_labels; float* ff_nll;     // forced-prefix pass: its labels [B, F] and per-token NLL
  P5BeamState st;
  P5WideWs wide;          // wide search (p5_decode_wide.h): null pointers unless the layout holds it
  int wide_c;             // its per-row candidate capacity min(max_c, 2K)
};

// state of the search between p5_decode_begin and p5_decode_finish (the workspace layout, the trie, the step counter)
struct GenCtx {
  bool active = false;
  GenWs w;
  int B = 0, L = 0, K = 0, max_len = 0, max_c = 0, excl_words = 0, steps = 0, steps0 = 0;     // steps0: steps covered by the forced-prefix pass
  bool wide = false;      // this search runs the wide step (p5_decode_wide.h)
  const int *child_off = nullptr, *child_tok = nullptr, *child_node = nullptr, *roots = nullptr;
  char* ws = nullptr;
};

struct P5Engine {
  P5Config c;
  int inner;
  int64_t off_E, off_WW, off_enc_rel, off_dec_rel, off_enc_fln, off_dec_fln, n_params, off_small_end;
  std::vector<LayerOff> enc, dec;
  std::vector<ParamInfo> table;
  float* P = nullptr; float* G = nullptr; void* S = nullptr;
  const int* lut_enc = nullptr; const int* lut_dec = nullptr; int lut_half = 0;
  uint32_t* rng = nullptr;
  // ---- saved state of the last forward ----
  int B = 0, L = 0, T = 0, training = 0, M = 0, Md = 0, Vp = 0;
  // several targets per user (p5_forward_targets): labels [B, G, T] -- the decoder is a batch of Bd = B * G sequences (Md = Bd * T rows), the encoder
  // and the cross-attention K/V a batch of B; cross-attention runs G * T queries of a user against that user's keys
  int Gt = 1, Bd = 0;                  // Gt: targets per user (G of the C ABI; `G` is the gradient arena)
  const float* tgt_w = nullptr;        // p5_forward_loss_targets: weight per target [Bd] of the seeded loss, or nullptr = 1
  const int64_t *ids = nullptr, *ww = nullptr, *mask = nullptr, *labels = nullptr, *out_attn = nullptr;
  std::vector<LayerSave> es, ds;
  void *enc_x0 = nullptr, *enc_xf = nullptr, *enc_out = nullptr; float* enc_rstd_f = nullptr;
  int64_t* dec_ids = nullptr; void *dec_x0 = nullptr, *dec_xf = nullptr, *dec_hn = nullptr; float* dec_rstd_f = nullptr;
  float *logits = nullptr, *lse_tok = nullptr, *ssq_scratch = nullptr;
  float *ce_part = nullptr, *ce_lab = nullptr, *ce_g = nullptr;      // logit-free cross-entropy: per-row partial (max, sum exp) pairs, label logits, NLL gradients
  bool ce_free_fwd = false;       // the last training forward took the logit-free head (the backward recomputes the logits tile by tile)
  bool ce_g_ready = false;        // ce_g already holds the NLL gradients of the last p5_forward_loss* (written by its loss kernel: option loss_fuse)
  // trie-normalised item loss (p5_trie_ce.h): il_next = p5_train_set_item_loss, armed for the NEXT forward (one-shot); il = what the last
  // forward ran under, read by the backward that follows it.  The rows' trie nodes and states live in ce_lab / ce_g (Md x 4 bytes each),
  // which only the logit-free route uses -- and an item-loss forward never takes it.
  // trunc: the truncated twins of p5_trunc.h (p5_train_set_item_loss_truncated); row_cut is the caller's [B * T] fp32 device array, written
  // by the forward and read by the backward
  struct ItemLoss {
    bool on = false; P5TrieCe tr = {nullptr, nullptr, nullptr, nullptr, 0, 1.f}; int* state_out = nullptr;
    bool trunc = false; P5TruncCe tc = {0, 1.f}; float* row_cut = nullptr;
    // head: the head restricted to the trie's tokens (p5_item_head.h, p5_train_set_item_head) -- tr.col is set, the caller's workspace holds
    // E_U [Nup, d] T | logits_U [Md, Nup] fp32 | dlogits_U [Md, Nup] T | dE_U [Nup, d] fp32, laid out by the forward, which knows Md
    // (item_head_layout)
    bool head = false; const int* head_tok = nullptr; int Nu = 0, Nup = 0;
    void* head_ws = nullptr; size_t head_ws_bytes = 0;
    void *EU = nullptr, *dlogitsU = nullptr; float *logitsU = nullptr, *dEU = nullptr;
    // reg: the regularised twins of p5_trie_reg.h (p5_train_set_item_regularizers) -- per-row entropy and, with reference logits, KL to the
    // reference.  row_terms is the caller's [3 * Md] fp32 device array (H | KL | lse_ref), written by the forward and read by the backward
    bool reg = false; const float* ref = nullptr; int ld_ref = 0; float* row_terms = nullptr; float ent_coef = 0.f, kl_coef = 0.f;
    float* terms_out = nullptr;
  };
  ItemLoss il_next, il;
  // clipped-ratio objective (p5_clip.h): clip_next = p5_train_set_clip_objective, armed for the NEXT p5_forward_loss* (one-shot); clip = what the
  // last forward ran under: the backward behind it (dnll == nullptr) takes its per-row seeds from clip.seed
  struct ClipObj {
    bool on = false; const float* old_lp = nullptr; const int* mode = nullptr; float eps_low = 0.f, eps_high = 0.f; int ratio_mode = 0;
    float *seed = nullptr, *partials = nullptr, *stats = nullptr;
  };
  ClipObj clip_next, clip;
  // preference objective (p5_pref.h): pref_next = p5_train_set_pref_objective, armed for the NEXT p5_forward_loss_targets (one-shot); pref = what
  // the last forward ran under: the backward behind it (dnll == nullptr) takes its per-row seeds from pref.seed
  struct PrefObj {
    bool on = false; const float* ref_lp = nullptr; const int* mask = nullptr; int kind = 0, depth = 0, length_normalize = 0;
    float beta = 0.f, sft_coef = 0.f; float *seed = nullptr, *partials = nullptr, *stats = nullptr;
  };
  PrefObj pref_next, pref;
  const float *bw_dH = nullptr, *bw_dKL = nullptr;      // p5_backward_set_item_grads: per-row gradients of H / KL for the NEXT backward (one-shot)
  void* Sf = nullptr;              // folded bf16 weight copy W diag(ln) for q/k/v, wi, cross-attention q (same arena offsets; behind St)
  float *dres_a = nullptr, *dres_b = nullptr, *d_enc = nullptr, *Dvec = nullptr, *dres_cur = nullptr, *rel_partial = nullptr;
  void *dy = nullptr, *dn = nullptr, *dqkv = nullptr, *dO = nullptr, *dh = nullptr, *du = nullptr, *dlogits = nullptr, *dkv = nullptr;
  // two sets of the temporaries the wgrad GEMMs read, alternated per sub-layer, so the side stream can run one
  // sub-layer behind the dgrad chain without a write-after-read hazard
  // (P5_NSETS sets: with the weight gradients of a whole layer deferred into ONE grouped launch at the end of the layer's backward --
  // p5_gemm4.h -- the temporaries of all its sub-layers, and of the next layer's that run meanwhile, must stay intact)
  void *dy2[P5_NSETS] = {}, *dh2[P5_NSETS] = {}, *du2[P5_NSETS] = {}, *dqkv2[P5_NSETS] = {}, *dkv2[P5_NSETS] = {};
  P5ReduceMulti nr_pending;               // norm-weight partial sums of the current backward stage, reduced by one launch at its end
  std::vector<P5GemmArgs> wg_pending;     // deferred weight-gradient problems (bf16, token count a multiple of 64)
  unsigned wg_sets = 0;                   // bit p: a pending problem reads temporaries of set p
  // weight-gradient plan of the whole backward (wgrad_plan_flush): the tied head's, the decoder layers' and the cross-attention K/V
  // block's problems wait in a pool and ride as FILLER units in the short workgroups of the encoder's two-layer launches (p5_gemm4.h)
  struct WgPoolItem { P5GemmArgs g; int kind, layer, rows_left, rows_all; };   // kind 0 head, 1 decoder layer, 2 K/V block; 256-row tile rows not yet taken
  std::vector<WgPoolItem> wg_pool;
  bool wg_plan = false;                   // this backward runs under the plan (decided in stage 0)
  int wg_pool_kind = -1, wg_pool_layer = 0;   // where linear_wgrad queues: -1 = wg_pending
  // ... whose decoder sub-layers therefore keep their temporaries (dy, dqkv, dh, du) in slots of their own, Md rows each, in backward order
  std::vector<void*> ds_dy, ds_dh, ds_du, ds_dqkv;
  bool whole_backward = false;            // inside p5_backward (as opposed to stage-by-stage calls of a data-parallel caller)
  bool stage_pairs = true;                // staged backward: the encoder's weight gradients still leave in two-layer groups (the benchmarked launch)
  int64_t fin_b = 0, fin_e = 0;           // staged backward: gradient range completed by the stages run since the last p5_backward_final_range
  int64_t rep_b = 0, rep_e = 0;           // ... and the range that call reports
  void* dy_next = nullptr;
  void *kv_all = nullptr, *dkv_all = nullptr;   // cross-attention K/V (and their gradients) of all decoder layers, [M, n_dec*2*inner]
  float* dw_scratch = nullptr;   // [norm slots][<=1024 workgroups][d] partial norm-weight gradients
  // deterministic embedding gradients (p5_embed.h): set 0 = tied table E over the encoder ids followed by the decoder ids, set 1 = whole-word table
  int* emb_idx[P5_EMB_MAXSETS] = {};     // perm | skey | sstart | slen, n ints each
  unsigned long long* emb_csort[P5_EMB_MAXSETS] = {};
  float* emb_part[P5_EMB_MAXSETS] = {};
  float* dres_dec0 = nullptr;            // [Md, d] gradient of the decoder's embedding rows (kept until the last stage)
  float* dres_out_override = nullptr;    // the next swap_norm_bwd writes its residual gradient here
  float* nb_dotbuf = nullptr;            // [rows, max(d_ff / 64, n_heads)] partial sums of <dOut, Out> per row: producer = the kernel that writes dOut, consumer = the P5_EPI_NORM_BWD GEMM that follows it
  bool nb_done = false;                  // the sub-layer's norm backward ran in the epilogue of its data-gradient GEMM: the caller skips swap_norm_bwd
  int norm_slot = 0;
  int sub = -1;
  bool d_enc_started = false;
  bool grads_zeroed = false;      // the gradient arena holds zeros (p5_engine_clear_grads): the next backward need not clear it
  bool grads_keep = false;        // p5_engine_grads_zeroed(): the next backward ADDS to the arena (2nd.. micro-batch of an accumulation group)
  int wg_epi = P5_EPI_ACCUM;      // how this backward's grouped weight-gradient GEMMs write: P5_EPI_STORE on a first micro-batch
  GenCtx gen;
  int* gen_hist_next = nullptr;    // p5_generate_draft: history buffer of the NEXT search (one-shot)
  const float* enc_ext_next = nullptr;   // p5_generate_set_encoder_output: fp32 encoder output the NEXT search starts from (one-shot)
  P5Forced ff_next = {0, {0}, {0}};  // p5_generate_set_forced_prefix: forced prefix of the NEXT search (one-shot)
  struct VerifyCtx* ver = nullptr;  // state of a verification pass between p5_verify_plan and p5_verify_run (p5_verify.h)
  // transposed bf16 copies of the 2-D layer weights (same arena offsets): the data gradients dx = dy W then read W^T as a
  // K-contiguous operand, i.e. run on the forward kernel (p5_engine_bind_transposed; optional)
  void* St = nullptr;
  struct TrDesc { int64_t off; int rows, cols, tile0; int64_t ln_off; };
  std::vector<TrDesc> tr_list;
  int tr_tiles = 0;
  int adam_tiles = 0;             // 64 x 256 tiles of p5_adamw_tiles_kernel over the same blocks
  bool tr_pending = false;
  bool zg_pending = false;        // p5_engine_clear_grads(): the clear runs on the side stream; the next backward waits for zg_ev
#ifndef P5_EMU
  hipEvent_t zg_ev = nullptr;
  hipEvent_t tr_ev = nullptr;
  hipEvent_t gen_ev[3] = {nullptr, nullptr, nullptr};   // p5_generate_timing: before the encoder pass / before the first / after the last decode step
  bool gen_timing = false;
  hipGraphExec_t gen_graph_exec = nullptr;
  bool gen_graph_failed = false;
  GraphKey gen_graph_key;
#endif
  bool st_side[P5_MAX_STAGED] = {};
  int64_t st_range[2 * P5_MAX_STAGED] = {};
  int st_n = 0;                   // p5_backward_staged: final ranges of the last call (events st_ev[0 .. st_n))
#ifndef P5_EMU
  hipEvent_t st_ev[P5_MAX_STAGED] = {};
  hipEvent_t st_ev_side[P5_MAX_STAGED] = {};      // the same point of the engine's side stream (weight gradients of the range may run there)
#endif
  // optional second stream for the weight-gradient GEMMs (off the critical dgrad chain)
  hipStream_t side = nullptr;
#ifndef P5_EMU
  bool side_events = false;               // the events below exist (created with the first side stream, destroyed with the engine)
  hipEvent_t ev_pool[32];
  hipEvent_t set_ev[P5_NSETS];            // recorded behind the last weight-gradient launch that reads set p
  hipEvent_t head_wg_ev;                  // ... behind the tied head's weight gradient (plain "+=" into shared.weight's gradient)
  hipEvent_t kv_ev[64];
  bool set_ev_valid[P5_NSETS] = {};
  bool head_wg_valid = false;
  int ev_next = 0;
#endif
};

static void begin_sublayer(P5Engine* e) {
  e->sub++;
  const int p = e->sub % P5_NSETS, pn = (e->sub + 1) % P5_NSETS;
  e->dy = e->dy2[p]; e->dy_next = e->dy2[pn];
  e->dh = e->dh2[p]; e->du = e->du2[p]; e->dqkv = e->dqkv2[p]; e->dkv = e->dkv2[p];
  if (e->wg_plan) {
    // decoder sub-layers (1 .. 3 n_dec of the backward) under the weight-gradient plan: what their weight gradients read must survive
    // until an encoder launch carries them -- slots of their own instead of the rotating sets
    const int n = (int)e->ds_dy.size(), k = e->sub - 1;
    if (k >= 0 && k < n) {
      e->dy = e->ds_dy[k];
      if (e->ds_dh[k]) e->dh = e->ds_dh[k];
      if (e->ds_du[k]) e->du = e->ds_du[k];
      if (e->ds_dqkv[k]) e->dqkv = e->ds_dqkv[k];
    }
    if (k + 1 >= 0 && k + 1 < n) e->dy_next = e->ds_dy[k + 1];
  }
}
// side stream waits for everything enqueued on `main` so far
static void fork_to_side(P5Engine* e, hipStream_t main) {
#ifndef P5_EMU
  if (!e->side) return;
  hipEvent_t ev = e->ev_pool[e->ev_next++ & 31];
  hipEventRecord(ev, main);
  hipStreamWaitEvent(e->side, ev, 0);
#endif
}
static void join_side(P5Engine* e, hipStream_t main) {
#ifndef P5_EMU
  if (!e->side) return;
  hipEvent_t ev = e->ev_pool[e->ev_next++ & 31];
  hipEventRecord(ev, e->side);
  hipStreamWaitEvent(main, ev, 0);
#endif
}
static int wgrad_flush(P5Engine* e, hipStream_t main, bool is_head, bool on_side);
// called right before the norm backward that ends sub-layer `sub`: it writes dy of the NEXT set, and the next sub-layer's data
// gradients write the rest of that set -- whatever weight-gradient launch still reads it (P5_NSETS sub-layers ago) must be done
static void end_sublayer_sync(P5Engine* e, hipStream_t main) {
  if ((e->wg_sets >> ((e->sub + 1) % P5_NSETS)) & 1) wgrad_flush(e, main, false, false);   // (cannot happen with one flush per layer; kept for safety)
#ifndef P5_EMU
  if (!e->side) return;
  const int p = e->sub % P5_NSETS, pn = (e->sub + 1) % P5_NSETS;
  if (!((e->wg_sets >> p) & 1)) {                      // this sub-layer's weight gradients were launched one by one: they are all enqueued
    hipEventRecord(e->set_ev[p], e->side);
    e->set_ev_valid[p] = true;
  }
  if (e->set_ev_valid[pn]) { hipStreamWaitEvent(main, e->set_ev[pn], 0); e->set_ev_valid[pn] = false; }
#endif
}
static hipStream_t wgrad_stream(P5Engine* e, hipStream_t main) {
  if (!e->side) return main;
  fork_to_side(e, main);
  return e->side;
}

static void add_param(P5Engine* e, const std::string& name, int rows, int cols, int64_t& off_out) {
  // every tensor starts on a 64-element boundary so 16-byte vector accesses stay aligned in both dtypes
  e->n_params = (e->n_params + 63) & ~(int64_t)63;
  off_out = e->n_params;
  e->table.push_back({name, e->n_params, rows, cols});
  e->n_params += (int64_t)rows * cols;
}

static void add_attn(P5Engine* e, const std::string& p, AttnOff& a) {
  const int d = e->c.d_model, in = e->inner;
  add_param(e, p + ".q.weight", in, d, a.q);
  // q,k,v must be back-to-back ([3*inner, d] fused projection): inner*d is a multiple of 64, so no padding appears
  add_param(e, p + ".k.weight", in, d, a.k);
  add_param(e, p + ".v.weight", in, d, a.v);
  add_param(e, p + ".o.weight", d, in, a.o);
}

static void build_layout(P5Engine* e) {
  const P5Config& c = e->c;
  const int d = c.d_model, F = c.d_ff;
  e->n_params = 0;
  add_param(e, "shared.weight", c.vocab_size, d, e->off_E);
  add_param(e, "encoder.whole_word_embeddings.weight", c.whole_word_size, d, e->off_WW);
  add_param(e, "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", c.rel_buckets, c.n_heads, e->off_enc_rel);
  add_param(e, "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", c.rel_buckets, c.n_heads, e->off_dec_rel);
  e->n_params = (e->n_params + 63) & ~(int64_t)63;
  e->off_small_end = e->n_params;
  auto add_ff = [&](const std::string& p, LayerOff& l) {
    if (c.gated_gelu) {
      int64_t t;
      add_param(e, p + ".DenseReluDense.wi_0.weight", F, d, l.wi);
      add_param(e, p + ".DenseReluDense.wi_1.weight", F, d, t);
    } else {
      add_param(e, p + ".DenseReluDense.wi.weight", F, d, l.wi);
    }
    add_param(e, p + ".DenseReluDense.wo.weight", d, F, l.wo);
  };
  e->enc.resize(c.n_enc_layers);
  for (int i = 0; i < c.n_enc_layers; ++i) {
    LayerOff& l = e->enc[i];
    const std::string p = "encoder.block." + std::to_string(i);
    e->n_params = (e->n_params + 63) & ~(int64_t)63;
    l.begin = e->n_params;
    add_attn(e, p + ".layer.0.SelfAttention", l.sa);
    add_param(e, p + ".layer.0.layer_norm.weight", 1, d, l.sa.ln);
    add_ff(p + ".layer.1", l);
    add_param(e, p + ".layer.1.layer_norm.weight", 1, d, l.ff_ln);
    l.end = e->n_params;
  }
  add_param(e, "encoder.final_layer_norm.weight", 1, d, e->off_enc_fln);
  e->dec.resize(c.n_dec_layers);
  // the cross-attention K/V projections of ALL decoder layers sit back to back ([n_dec * 2 * inner, d]): they all read the same
  // encoder output, so forward, weight gradient and d(enc_out) are one GEMM each instead of one per layer.  The block lies
  // between the encoder's final norm and the first decoder layer, i.e. inside the data-parallel bucket of the stage that
  // follows the decoder (p5_backward_stage_range), which is when its gradient is complete.
  for (int i = 0; i < c.n_dec_layers; ++i) {
    const std::string p = "decoder.block." + std::to_string(i) + ".layer.1.EncDecAttention";
    add_param(e, p + ".k.weight", e->inner, d, e->dec[i].ca.k);     // inner*d is a multiple of 64: no padding in between
    add_param(e, p + ".v.weight", e->inner, d, e->dec[i].ca.v);
  }
  for (int i = 0; i < c.n_dec_layers; ++i) {
    LayerOff& l = e->dec[i];
    const std::string p = "decoder.block." + std::to_string(i);
    e->n_params = (e->n_params + 63) & ~(int64_t)63;
    l.begin = e->n_params;
    add_attn(e, p + ".layer.0.SelfAttention", l.sa);
    add_param(e, p + ".layer.0.layer_norm.weight", 1, d, l.sa.ln);
    add_param(e, p + ".layer.1.EncDecAttention.q.weight", e->inner, d, l.ca.q);
    add_param(e, p + ".layer.1.EncDecAttention.o.weight", d, e->inner, l.ca.o);
    add_param(e, p + ".layer.1.layer_norm.weight", 1, d, l.ca.ln);
    add_ff(p + ".layer.2", l);
    add_param(e, p + ".layer.2.layer_norm.weight", 1, d, l.ff_ln);
    l.end = e->n_params;
  }
  add_param(e, "decoder.final_layer_norm.weight", 1, d, e->off_dec_fln);
  e->n_params = (e->n_params + 63) & ~(int64_t)63;
  // weights whose data gradient runs on the transposed copy: (offset, rows, cols) of each [rows, cols] block
  {
    e->tr_list.clear();
    int tiles = 0;
    // (ln: the T5LayerNorm weight whose output the projection consumes -- the blocks p5_refresh_transposed folds -- or -1)
    auto add = [&](int64_t off, int rows, int cols, int64_t ln = -1) {
      e->tr_list.push_back({off, rows, cols, tiles, ln});
      tiles += ((rows + 63) / 64) * ((cols + 63) / 64);
    };
    const int wi_rows = (c.gated_gelu ? 2 : 1) * F;
    for (int i = 0; i < c.n_enc_layers; ++i) {
      add(e->enc[i].sa.q, 3 * e->inner, d, e->enc[i].sa.ln); add(e->enc[i].sa.o, d, e->inner); add(e->enc[i].wi, wi_rows, d, e->enc[i].ff_ln); add(e->enc[i].wo, d, F);
    }
    add(e->dec[0].ca.k, c.n_dec_layers * 2 * e->inner, d);
    for (int i = 0; i < c.n_dec_layers; ++i) {
      add(e->dec[i].sa.q, 3 * e->inner, d, e->dec[i].sa.ln); add(e->dec[i].sa.o, d, e->inner); add(e->dec[i].ca.q, e->inner, d, e->dec[i].ca.ln);
      add(e->dec[i].ca.o, d, e->inner);
      add(e->dec[i].wi, wi_rows, d, e->dec[i].ff_ln); add(e->dec[i].wo, d, F);
    }
    e->tr_tiles = tiles;
  }
}

template <class T> static const T* Wc(const P5Engine* e, int64_t off) {
  if (sizeof(T) == 4) return (const T*)(e->P + off);
  return (const T*)((const bf16*)e->S + off);
}

static P5Drop mk_drop(const P5Engine* e, int stack, int layer, int which) {
  P5Drop d;
  d.state = nullptr; d.site_key = 0; d.thr = 0; d.scale = 1.f;
  if (e->training && e->c.dropout > 0.f) {
    d.state = e->rng;
    d.site_key = p5_site_key(p5_site_id(stack, layer, which));
    d.thr = p5_drop_thr(e->c.dropout);
    d.scale = 1.f / (1.f - e->c.dropout);
  }
  return d;
}
static P5Drop no_drop() { P5Drop d; d.state = nullptr; d.site_key = 0; d.thr = 0; d.scale = 1.f; return d; }

// fp32 engine: products of the K-contiguous forward GEMMs on the f16 matrix cores from a two-term split (p5_gemm.h); switched on by the
// verification pass for the duration of its calls (option "verify_split"), off everywhere else: the fp32 parity engine stays exact
static thread_local int g_f32_split = 0;
static int g_opt_verify_split = getenv("P5_VERIFY_SPLIT") ? atoi(getenv("P5_VERIFY_SPLIT")) : 1;
struct SplitScope { int prev; explicit SplitScope(int on) : prev(g_f32_split) { g_f32_split = on; } ~SplitScope() { g_f32_split = prev; } };

template <class T>
static int gemm(hipStream_t s, const void* A, int lda, int aks, const void* Bm, int ldb, int bks, void* C, int ldc, int M, int N,
                int K, int epi, const void* aux, int ldaux, float alpha, int c_f32, P5Drop drop) {
  P5GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = Bm; g.C = C; g.aux = aux; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux;
  g.a_ks = aks; g.b_ks = bks; g.epi = epi; g.c_f32 = c_f32; g.splitk = 0; g.ring = 0; g.alpha = alpha; g.drop = drop;
  g.g4_tiles_n = 0; g.g4_nk = 0; g.xcd_bm = g.xcd_bn = 0; g.c_split_stride = 0;
  g.mm_split = (sizeof(T) == 4 && !aks && !bks && epi != P5_EPI_ATOMIC && epi != P5_EPI_ACCUM) ? g_f32_split : 0;
  return launch_gemm<T>(g, s);
}
// TRAINING forward with T5LayerNorm folded in (bf16 engine): y = rstd(x) * (x Wf^T), Wf = W diag(ln) from the folded
// weight copy, rstd from the d/64 partial sums of squares per row that the PRODUCER of x left behind (`rowss`); `ssq_out`: this
// GEMM's own output is a residual-stream row whose partial sums the next folded GEMM needs.
template <class T>
static int gemm_nf(hipStream_t s, const void* A, int lda, const void* Bm, int ldb, void* C, int ldc, int M, int N, int K, int epi, const void* aux,
                   int ldaux, P5Drop drop, const float* rowss, float eps, float* ssq_out, int d_model) {
  P5GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = Bm; g.C = C; g.aux = aux; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux;
  g.epi = epi; g.alpha = 1.f; g.drop = drop;
  g.rowss = rowss; g.rowss_invd = 1.0f / (float)K; g.rowss_eps = eps; g.rowss_nt = rowss ? d_model / 64 : 0;
  g.ssq_out = ssq_out; g.ssq_nt = ssq_out ? d_model / 64 : 0;
  return launch_gemm<T>(g, s);
}
// y = x W^T
template <class T>
static int linear_fwd(hipStream_t s, const void* x, int ldx, const T* W, void* y, int ldy, int M, int N, int K, int epi = P5_EPI_STORE,
                      const void* aux = nullptr, int ldaux = 0, float alpha = 1.f, int c_f32 = 0, P5Drop drop = no_drop()) {
  return gemm<T>(s, x, ldx, 0, W, K, 0, y, ldy, M, N, K, epi, aux, ldaux, alpha, c_f32, drop);
}
// dx = dy W     (W is [N_out, K_in] row-major; reduction over N_out)
template <class T>
static int linear_dgrad(hipStream_t s, const void* dy, int lddy, const T* W, void* dx, int lddx, int M, int N_out, int K_in,
                        int epi = P5_EPI_STORE, const void* aux = nullptr, int ldaux = 0, float alpha = 1.f, int c_f32 = 0) {
  return gemm<T>(s, dy, lddy, 0, W, K_in, 1, dx, lddx, M, K_in, N_out, epi, aux, ldaux, alpha, c_f32, no_drop());
}
// dx = dy W with W given by its arena offset: when a transposed copy is bound (bf16), W^T [K_in, N_out] is a K-contiguous operand
// and the product runs on the forward kernel (direct-to-LDS copies of both operands) instead of the K-strided-B variant
template <class T>
static int dgrad_w(P5Engine* e, hipStream_t s, const void* dy, int lddy, int64_t w_off, void* dx, int lddx, int M, int N_out, int K_in,
                   int epi = P5_EPI_STORE, const void* aux = nullptr, int ldaux = 0, float alpha = 1.f, int c_f32 = 0) {
  if (sizeof(T) == 2 && e->St && g_opt_dgrad_t && (N_out % 64) == 0)
    return gemm<T>(s, dy, lddy, 0, (const T*)e->St + w_off, N_out, 0, dx, lddx, M, K_in, N_out, epi, aux, ldaux, alpha, c_f32, no_drop());
  return linear_dgrad<T>(s, dy, lddy, Wc<T>(e, w_off), dx, lddx, M, N_out, K_in, epi, aux, ldaux, alpha, c_f32);
}
static int g_opt_wgrad_split_atomic = getenv("P5_WGRAD_SPLIT_ATOMIC") ? atoi(getenv("P5_WGRAD_SPLIT_ATOMIC")) : 0;    // 1 = split-K atomics (not reproducible)
// dW += dy^T x   (into the grad arena)
template <class T>
static int linear_wgrad_on(hipStream_t s, const void* dy, int lddy, const void* x, int ldx, float* dW, int M, int N_out, int K_in,
                        float alpha = 1.f) {
  // ONE split: every element of dW then receives exactly one add per backward -- the same bits on every run.  (Split-K with fp32
  // atomics -- rounds 1-3 -- made the last bits depend on the order the splits landed in; the grouped bf16 path never splits.)
  P5GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = dy; g.B = x; g.C = dW; g.M = N_out; g.N = K_in; g.K = M; g.lda = lddy; g.ldb = ldx; g.ldc = K_in;
  g.a_ks = 1; g.b_ks = 1; g.epi = P5_EPI_ATOMIC; g.c_f32 = 1; g.splitk = g_opt_wgrad_split_atomic ? 0 : 1; g.alpha = alpha; g.drop = no_drop();
  g.rowss_invd = 1.0f / (float)M;
  return launch_gemm<T>(g, s);
}

// Weight gradients of the bf16 engine are DEFERRED: the problem is queued and the whole layer's queue goes out as one launch of the
// persistent ring kernel (p5_gemm4.h) -- every 128x128 tile of every weight of the layer reduces over ALL tokens (no split-K, no
// atomics, plain "dW += acc"; each weight has exactly one writer).  wgrad_flush is called at the end of every backward stage.
// which grouped weight-gradient launches go to the side stream: bit 0 = tied head + decoder layers (they run beside the decoder's chain of
// small, latency-bound kernels, which leaves most CUs idle), bit 1 = cross-attention K/V block + encoder layers (every main-stream
// kernel of the encoder backward fills the GPU by itself: beside it a 90 us weight-gradient workgroup only blocks CUs -- measured
// 5.07 ms per step with everything on the side stream, 4.74 ms with nothing on it)
static int g_opt_wgrad_side = getenv("P5_WGRAD_SIDE") ? atoi(getenv("P5_WGRAD_SIDE")) : 1;
static int g_opt_wgrad_wide = getenv("P5_WGRAD_WIDE") ? atoi(getenv("P5_WGRAD_WIDE")) : 1;
static int g_opt_wgrad_wide_min = getenv("P5_WGRAD_WIDE_MIN") ? atoi(getenv("P5_WGRAD_WIDE_MIN")) : 160;
static int g_opt_wgrad_wgs = getenv("P5_WGRAD_WGS") ? atoi(getenv("P5_WGRAD_WGS")) : 0;          // workgroups of a grouped weight-gradient launch (0 = one per unit, <= 256)
static int g_opt_wgrad_layers = getenv("P5_WGRAD_LAYERS") ? atoi(getenv("P5_WGRAD_LAYERS")) : 2;  // encoder layers per grouped launch (p5_backward only; staged backward: 1)
// 1 = the weight-gradient plan of the whole backward (wgrad_plan_flush below); 0 = the grouping and the launches of round 6
static int g_opt_wgrad_fill = getenv("P5_WGRAD_FILL") ? atoi(getenv("P5_WGRAD_FILL")) : 1;
// Cost model of the plan, in K-steps (one K-step of a 256x128 tile = 48 KiB copied, 64 MFMAs per compute wave): a unit costs its K-steps
// plus this constant for what does not shrink with K -- the cold first K-steps of a new problem and the 128 KB fp32 tile its epilogue
// stores (or reads, adds and stores).  Derivation: an encoder group runs 128 K-steps per unit in 122 us, 0.95 us per K-step; the tied
// head's own launch (504 units of 8 K-steps, two rounds on 256 workgroups, 41 us) spends ~20 us per unit, of which the K-steps explain
// 7.6 us -- the remaining ~12 us are 13 K-steps.  (The decoder layers' launches, 15.5 us for one round of 128x128 tiles of 8 K-steps, say
// the same: 7.6 us of K-steps, ~8 us of everything else.)
// Measured in the step (T5-small, B=64, L=128, T=8; profiles/r07_call1_wgrad_fill_epi_sweep.txt), constant -> ms per step / weight-gradient launches:
// 4 -> 3.95 / 4, 8 -> 3.92 / 4, 13 -> 3.95 / 5, 24 -> 3.96 / 6 (no plan: 4.11 / 11).  8: lower values overfill the short workgroups (the
// filled launches grow from 135 to 146 us), higher ones leave a second trailing launch.
static int g_opt_wgrad_fill_epi = getenv("P5_WGRAD_FILL_EPI") ? atoi(getenv("P5_WGRAD_FILL_EPI")) : 8;
static int wgrad_flush(P5Engine* e, hipStream_t main, bool is_head, bool on_side = true) {
  if (e->wg_pending.empty()) return 0;
  hipStream_t s = on_side ? wgrad_stream(e, main) : main;        // (side: it now waits for everything the main stream has been given)
  size_t i = 0;
  while (i < e->wg_pending.size()) {
    P5GemmGroup grp;
    memset(&grp, 0, sizeof(grp));
    long u256 = 0;
    while (i < e->wg_pending.size() && grp.nprob < P5_MAX_GROUP) {
      const P5GemmArgs& q = e->wg_pending[i];
      u256 += (long)((q.M + 255) / 256) * ((q.N + 127) / 128);
      grp.p[grp.nprob++] = e->wg_pending[i++];
    }
    const int keep = g_opt_g4_wgs;
    if (g_opt_wgrad_wgs > 0) g_opt_g4_wgs = g_opt_wgrad_wgs;
    // 256x128 tiles (eight waves) once the group has enough of them to occupy most CUs: 3/4 of the operand bytes per MAC copied
    // into LDS -- which is what bounds these launches (tools/lab: two encoder layers 130 us vs 163 us on 128x128 tiles; one
    // layer alone has only 96 such tiles and stays on 128x128: 85 vs 102 us)
    const int rc = launch_gemm4(g_opt_wgrad_wide && u256 >= g_opt_wgrad_wide_min ? P5_G4_256x128 : P5_G4_128x128, true, grp, s);
    g_opt_g4_wgs = keep;
    P5_TRY(rc);
  }
#ifndef P5_EMU
  if (e->side) {
    for (int p = 0; p < P5_NSETS; ++p)
      if ((e->wg_sets >> p) & 1) { hipEventRecord(e->set_ev[p], s); e->set_ev_valid[p] = true; }
    if (is_head) { hipEventRecord(e->head_wg_ev, s); e->head_wg_valid = true; }
  }
#endif
  e->wg_pending.clear();
  e->wg_sets = 0;
  return 0;
}

// ---- the weight-gradient plan of the whole backward ------------------------------------------------------------------------------
// An encoder group of two layers is 192 units of 256x128 on 256 workgroups: a quarter of the CUs idle for the whole launch, while the
// head's, the decoder's and the K/V block's weight gradients -- finished long before, not needed until the optimizer -- cost launches of
// their own that barely fill the GPU.  Under the plan they wait in e->wg_pool, and every encoder flush fills its launch's short workgroups
// from the pool: K/V block first (split by 256-row slices of its output, taken from the bottom rows up so that what is left keeps its
// base pointers), then decoder layers in the order they became ready, then the head (by slices too).  What the last encoder group could
// not take goes out as ordinary grouped launches.  Only which problems share a launch changes: every element keeps its one writer, every
// tile its whole K range.
// the pool as ordinary problems, appended to wg_pending (what nobody carried)
static void wgrad_pool_drain(P5Engine* e) {
  for (int kind : {2, 1, 0})
    for (const P5Engine::WgPoolItem& it : e->wg_pool) {
      if (it.kind != kind || it.rows_left <= 0) continue;
      P5GemmArgs g = it.g;
      if (it.rows_left < it.rows_all) g.M = it.rows_left * 256;      // (the upper slices were carried: rows [0, rows_left * 256) remain)
      e->wg_pending.push_back(g);
    }
  e->wg_pool.clear();
}
// the largest filler load (in cost units) the kernel's dealing puts on one short workgroup -- p5_gemm5.h, the same arithmetic
static long wgrad_fill_worst(int prim_units, int wcap, int nfill, int nheavy, int heavy_wgs, const int* units, const int* cost) {
  int fu = 0;
  for (int q = 0; q < nfill; ++q) fu += units[q];
  int nwg = ((prim_units + fu + 7) / 8) * 8;
  if (nwg > wcap) nwg = wcap;
  const int gx = nwg >> 3, upx = (prim_units + 7) >> 3;
  if (gx < 1) return -1;
  long worst = 0;
  std::vector<long> load((size_t)gx);
  for (int x = 0; x < 8; ++x) {
    int ulast = prim_units - x * upx;
    ulast = ulast < 0 ? 0 : (ulast > upx ? upx : ulast);
    const int rr = ulast % gx, ns = rr == 0 ? gx : gx - rr;
    const bool two = heavy_wgs > 0 && heavy_wgs < ns;
    for (int cls = 0; cls < (two ? 2 : 1); ++cls) {
      const int q0 = two && cls == 1 ? nheavy : 0, q1 = two && cls == 0 ? nheavy : nfill;
      const int n = two ? (cls == 0 ? heavy_wgs : ns - heavy_wgs) : ns;
      for (int w = 0; w < n; ++w) load[w] = 0;
      int pos = 0, first;
      for (int q = q0; q < q1; ++q) {
        const int sh = p5_fill_share(units[q], x, &first);
        for (int k = 0; k < sh; ++k) load[(pos + k) % n] += cost[q];
        pos += sh;
      }
      for (int w = 0; w < n; ++w) worst = load[w] > worst ? load[w] : worst;
    }
  }
  return worst;
}
static void wgrad_fill_entry(P5FillProb& f, const P5GemmArgs& g, int row0, int rows) {
  memset(&f, 0, sizeof(f));
  f.A = (const bf16*)g.A + row0; f.B = g.B; f.C = (float*)g.C + (size_t)row0 * g.ldc;
  f.M = rows; f.N = g.N; f.nk = g.K / 64; f.batch = 1; f.lda = g.lda; f.ldb = g.ldb; f.ldc = g.ldc; f.epi = g.epi; f.alpha = g.alpha;
  f.acap = g.lda - row0;
}
static int wgrad_plan_flush(P5Engine* e, hipStream_t s, bool last) {
  typedef P5Engine::WgPoolItem Item;
  std::vector<Item>& pool = e->wg_pool;
  const int nprim = (int)e->wg_pending.size();
  long prim_units = 0;
  int nkp = 0;
  for (const P5GemmArgs& q : e->wg_pending) {
    prim_units += (long)((q.M + 255) / 256) * ((q.N + 127) / 128);
    nkp = q.K / 64 > nkp ? q.K / 64 : nkp;
  }
  // fillers exist in the wave-specialised 256x128 K-strided instance only: a group that takes another route today keeps it
  const bool can_fill = !pool.empty() && nprim >= 1 && nprim <= P5_MAX_GROUP && g_opt_wgrad_wide && prim_units >= g_opt_wgrad_wide_min && p5l_gemm_fill_ok();
  P5GemmGroupFill grp;
  memset((void*)&grp, 0, sizeof(grp));
  if (can_fill) {
    const int wcap = g_opt_wgrad_wgs > 0 ? g_opt_wgrad_wgs : g_opt_g4_wgs;
    const int epi_c = g_opt_wgrad_fill_epi > 0 ? g_opt_wgrad_fill_epi : 0;
    const long allow = nkp + epi_c;          // a short workgroup may carry fillers worth ONE primary unit
    int units[P5_MAX_FILL], cost[P5_MAX_FILL], nf = 0, nheavy = 0, hw = 0;
    auto fits = [&](int n) { const long w = wgrad_fill_worst((int)prim_units, wcap, n, nheavy, hw, units, cost); return w >= 0 && w <= allow; };
    // 1. the K/V block: as many 256-row slices as fit, on workgroups of their own (its K is the encoder's: one tile fills a workgroup)
    for (Item& it : pool) {
      if (it.kind != 2 || it.rows_left <= 0 || nf > 0) continue;
      const int tn = (it.g.N + 127) / 128, c1 = it.g.K / 64 + epi_c, cap = (int)(allow / c1);
      if (cap < 1) continue;
      for (int t = it.rows_left; t >= 1; --t) {
        units[0] = t * tn; cost[0] = c1;
        nheavy = 1; hw = ((units[0] + 7) / 8 + cap - 1) / cap;
        if (!fits(1)) continue;
        const int r0 = (it.rows_left - t) * 256, r1 = it.rows_left * 256 < it.g.M ? it.rows_left * 256 : it.g.M;
        wgrad_fill_entry(grp.f[0], it.g, r0, r1 - r0);
        it.rows_left -= t;
        nf = 1;
        break;
      }
      if (nf == 0) { nheavy = 0; hw = 0; }
    }
    // 2. decoder layers, whole, in the order they became ready: one entry per weight, the layers as its batch
    {
      std::vector<int> idx;       // pool indices of decoder problems, in order
      for (size_t k = 0; k < pool.size(); ++k) if (pool[k].kind == 1) idx.push_back((int)k);
      int per = 0;                // problems per layer
      while (per < (int)idx.size() && pool[idx[per]].layer == pool[idx[0]].layer) ++per;
      const int nl = per ? (int)idx.size() / per : 0;
      int take = 0;
      P5FillProb ent[P5_MAX_FILL];
      for (int n = 1; n <= nl && per > 0 && nf + per <= P5_MAX_FILL; ++n) {
        bool ok = true;
        for (int k = 0; k < per && ok; ++k) {
          const P5GemmArgs& g0 = pool[idx[k]].g;
          P5FillProb f;
          wgrad_fill_entry(f, g0, 0, g0.M);
          f.batch = n;
          if (n > 1) {
            const P5GemmArgs& g1 = pool[idx[per + k]].g;
            const long long dA = (const char*)g1.A - (const char*)g0.A, dB = (const char*)g1.B - (const char*)g0.B, dC = (const char*)g1.C - (const char*)g0.C;
            ok = dA % 16 == 0 && dB % 16 == 0 && dC % 16 == 0;
            f.sA = dA / 2; f.sB = dB / 2; f.sC = dC / 4;
            for (int l = 1; l < n && ok; ++l) {
              const P5GemmArgs& gl = pool[idx[l * per + k]].g;
              ok = gl.M == g0.M && gl.N == g0.N && gl.K == g0.K && gl.lda == g0.lda && gl.ldb == g0.ldb && gl.ldc == g0.ldc && gl.alpha == g0.alpha && gl.epi == g0.epi &&
                   (const char*)gl.A - (const char*)g0.A == dA * l && (const char*)gl.B - (const char*)g0.B == dB * l && (const char*)gl.C - (const char*)g0.C == dC * l;
            }
          }
          units[nf + k] = ((g0.M + 255) / 256) * ((g0.N + 127) / 128) * n;
          cost[nf + k] = g0.K / 64 + epi_c;
          ent[k] = f;
        }
        if (!ok || !fits(nf + per)) break;
        take = n;
        for (int k = 0; k < per; ++k) grp.f[nf + k] = ent[k];
      }
      if (take > 0) {
        // (units[] holds the last layer count TRIED, one more than `take` when the loop broke: the head below is fitted against what was taken)
        for (int k = 0; k < per; ++k) units[nf + k] = grp.f[nf + k].batch * ((grp.f[nf + k].M + 255) / 256) * ((grp.f[nf + k].N + 127) / 128);
        nf += per;
        std::vector<Item> rest;
        int seen = 0;
        for (const Item& it : pool) {
          if (it.kind == 1 && seen < take * per) { ++seen; continue; }
          rest.push_back(it);
        }
        pool.swap(rest);
      }
    }
    // 3. the head: the most 256-row slices that still fit (bisection: the worst load grows with the slice count)
    for (Item& it : pool) {
      if (it.kind != 0 || it.rows_left <= 0 || nf >= P5_MAX_FILL) continue;
      const int tn = (it.g.N + 127) / 128;
      cost[nf] = it.g.K / 64 + epi_c;
      int lo = 0, hi = it.rows_left;
      while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        units[nf] = mid * tn;
        if (fits(nf + 1)) lo = mid; else hi = mid - 1;
      }
      if (lo > 0) {
        const int r0 = (it.rows_left - lo) * 256, r1 = it.rows_left * 256 < it.g.M ? it.rows_left * 256 : it.g.M;
        wgrad_fill_entry(grp.f[nf], it.g, r0, r1 - r0);
        it.rows_left -= lo;
        ++nf;
      }
      break;
    }
    grp.nfill = nf; grp.nheavy = nheavy; grp.heavy_wgs = hw;
  }
  if (grp.nfill > 0) {
    grp.nprob = nprim;
    for (int k = 0; k < nprim; ++k) grp.p[k] = e->wg_pending[k];
    const int keep = g_opt_g4_wgs;
    if (g_opt_wgrad_wgs > 0) g_opt_g4_wgs = g_opt_wgrad_wgs;
    const int rc = launch_gemm_fill(grp, s);
    g_opt_g4_wgs = keep;
    P5_TRY(rc);
    e->wg_pending.clear();
    e->wg_sets = 0;
  }
  if (last) wgrad_pool_drain(e);
  return wgrad_flush(e, s, false, false);
}
// ONE predicate for "every weight gradient of this step's backward takes the deferred, layer-grouped path" (token counts that are
// multiples of 64; the other conditions of linear_wgrad -- leading dimensions, 16-byte alignment -- hold by construction of the layout):
// the folded-norm forward, the storing backward and linear_wgrad itself all depend on it and must not drift apart.
template <class T> static bool wg_all_deferred(const P5Engine* e) {
  return sizeof(T) == 2 && g_opt_wgrad_group != 0 && (e->M % 64) == 0 && (e->Md % 64) == 0;
}
template <class T>
static int linear_wgrad(P5Engine* e, hipStream_t main, const void* dy, int lddy, const void* x, int ldx, float* dW, int M, int N_out, int K_in,
                        float alpha = 1.f) {
  if (sizeof(T) == 2 && g_opt_wgrad_group && (M % 64) == 0 && (lddy % 8) == 0 && (ldx % 8) == 0 && ((uintptr_t)dy % 16) == 0 &&
      ((uintptr_t)x % 16) == 0 && (K_in % 4) == 0) {
    P5GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = dy; g.B = x; g.C = dW; g.M = N_out; g.N = K_in; g.K = M; g.lda = lddy; g.ldb = ldx; g.ldc = K_in;
    g.a_ks = 1; g.b_ks = 1; g.epi = e->wg_epi; g.c_f32 = 1; g.splitk = 1; g.alpha = alpha; g.drop = no_drop();
    if (e->wg_plan && e->wg_pool_kind >= 0) {      // (reads no rotating set: nothing to note in wg_sets)
      P5Engine::WgPoolItem it;
      memset(&it, 0, sizeof(it));
      it.g = g; it.kind = e->wg_pool_kind; it.layer = e->wg_pool_layer; it.rows_left = it.rows_all = (g.M + 255) / 256;
      e->wg_pool.push_back(it);
      return 0;
    }
    e->wg_pending.push_back(g);
    if (e->sub >= 0) e->wg_sets |= 1u << (e->sub % P5_NSETS);
    return 0;
  }
  // an immediate weight gradient: under the folded-norm forward it would read the normalised rows before the norm backward has written
  // them, under a storing backward its target has not been cleared -- both modes require wg_all_deferred, which this problem contradicts
  P5_REQUIRE(!(e->Md > 0 && wg_all_deferred<T>(e)), "linear_wgrad: a weight gradient fell off the grouped path although wg_all_deferred holds (leading dimension / alignment)");
  if (e->wg_epi == P5_EPI_STORE) hipMemsetAsync(dW, 0, (size_t)N_out * K_in * 4, wgrad_stream(e, main));
  return linear_wgrad_on<T>(wgrad_stream(e, main), dy, lddy, x, ldx, dW, M, N_out, K_in, alpha);
}

template <class T>
static int rmsnorm_fwd(hipStream_t s, void* y, float* rstd, const void* x, const float* w, int rows, int d, float eps, P5Drop drop) {
  P5_REQUIRE(d % TT<T>::EPF == 0 && d <= 1024, "rmsnorm: d_model must be <= 1024 and a multiple of 8");
  P5_LAUNCH((p5_rmsnorm_fwd_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, (T*)y, rstd, (const T*)x, w, rows, d, eps, drop);
  return P5_KCHECK();
}
// workgroups of the norm backward (4 rows per workgroup and pass): with fewer than rows / 8 of them a wave makes several passes and its
// stores of one pass overlap its loads of the next
static int g_opt_norm_bwd_blocks = getenv("P5_NORM_BWD_BLOCKS") ? atoi(getenv("P5_NORM_BWD_BLOCKS")) : 1024;
template <class T>
static int rmsnorm_bwd(hipStream_t s, float* dres_out, void* dy_next, float* dw, const void* dy, const void* x, const float* w,
                       const float* rstd, const float* dres_in, int rows, int d, P5Drop din, P5Drop dnext, float* dw_partial = nullptr,
                       int* nblocks_out = nullptr, const float* ssq_part = nullptr, void* n_out = nullptr, float eps = 0.f) {
  P5_REQUIRE(d % TT<T>::EPF == 0 && d <= 1024, "rmsnorm: d_model must be <= 1024 and a multiple of 8");
  int blocks = (rows + 3) / 4;
  const int cap = g_opt_norm_bwd_blocks < 64 ? 64 : (g_opt_norm_bwd_blocks > 1024 ? 1024 : g_opt_norm_bwd_blocks);     // (the partial-sum scratch holds 1024 rows per norm)
  if (blocks > cap) blocks = cap;
  if (nblocks_out) *nblocks_out = blocks;
  const int nch = (d / TT<T>::EPF + 63) / 64;          // 16-byte pieces per lane
#define P5_NBWD(N) P5_LAUNCH((p5_rmsnorm_bwd_kernel<T, N>), dim3(blocks), dim3(256), 0, s, dres_out, (T*)dy_next, dw, (const T*)dy, (const T*)x, w, rstd, \
                             dres_in, rows, d, din, dnext, dw_partial, ssq_part, (T*)n_out, eps)
  if (nch <= 1) P5_NBWD(1);
  else if (nch == 2) P5_NBWD(2);
  else P5_NBWD(4);
#undef P5_NBWD
  return P5_KCHECK();
}

// relative-bias gradient: one slot of [rel_buckets, H] partial sums per attention-backward workgroup (layer x batch item x 64-query block),
// stored by that workgroup only and summed in slot order (p5_attn.h rel_bias_grad_flush)
static int rel_slots(int B, int Lq) { return B * ((Lq + 63) / 64); }
static constexpr int P5_HEAD_SPLITS = 32;      // most K-splits of the tied head's input-gradient GEMM (slices of its partial-product buffer)

// A backward that starts a new accumulation group does not clear the 4 B x n_params gradient arena and then add into it: every
// Linear weight's gradient is written by exactly one GEMM tile pass, which STORES on that first micro-batch (and `+=` on later ones);
// the head's gradient of the tied embedding is stored before the embedding scatter-adds land on it.  Only the parameters whose
// gradients are sums of atomics / partial reductions (whole-word embedding, relative-bias tables, T5LayerNorm weights: ~1 MB of
// T5-small's 242 MB) are cleared, by one table-driven launch.  Saves the fill and the read of the arena per step.
static int g_opt_grad_store_first = getenv("P5_GRAD_STORE_FIRST") ? atoi(getenv("P5_GRAD_STORE_FIRST")) : 1;
// embedding gradients as fixed-order segmented sums (p5_embed.h) instead of fp32 atomic scatters: bit-reproducible training (0 = the
// atomic scatter of rounds 1-3, kept for A/B timing)
static int g_opt_embed_det = getenv("P5_EMBED_DET") ? atoi(getenv("P5_EMBED_DET")) : 1;
struct P5ZeroTab {
  int n;
  struct D { long long off; int count, blk0; } e[200];
};
__global__ __launch_bounds__(256) void p5_zero_segments_kernel(float* __restrict__ G, P5ZeroTab tab) {
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;             // last segment with blk0 <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.e[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const int i0 = (b - tab.e[lo].blk0) * 8192, n = tab.e[lo].count;
  float* __restrict__ dst = G + tab.e[lo].off;
  for (int i = i0 + threadIdx.x; i < i0 + 8192 && i < n; i += 256) dst[i] = 0.f;
}
static int zero_small_grads(P5Engine* e, hipStream_t s) {
  const P5Config& c = e->c;
  P5ZeroTab tab;
  tab.n = 0;
  int blocks = 0;
  auto add = [&](int64_t off, int64_t count) {
    if (count <= 0 || tab.n >= 200) return;
    P5ZeroTab::D& q = tab.e[tab.n++];
    q.off = off; q.count = (int)count; q.blk0 = blocks;
    blocks += (int)((count + 8191) / 8192);
  };
  add(e->off_WW, (int64_t)c.whole_word_size * c.d_model);
  add(e->off_enc_rel, (int64_t)c.rel_buckets * c.n_heads);
  add(e->off_dec_rel, (int64_t)c.rel_buckets * c.n_heads);
  for (const LayerOff& l : e->enc) { add(l.sa.ln, c.d_model); add(l.ff_ln, c.d_model); }
  for (const LayerOff& l : e->dec) { add(l.sa.ln, c.d_model); add(l.ca.ln, c.d_model); add(l.ff_ln, c.d_model); }
  add(e->off_enc_fln, c.d_model);
  add(e->off_dec_fln, c.d_model);
  P5_REQUIRE(tab.n < 200, "zero_small_grads: too many segments");
  P5_LAUNCH(p5_zero_segments_kernel, dim3(blocks), dim3(256), 0, s, e->G, tab);
  return P5_KCHECK();
}

// the caller's workspace of the restricted item head (p5_item_head.h): E_U | logits_U | dlogits_U | dE_U.  The split-K partial products of
// its input gradient are [Md, d] slices like the dense head's and live in dres_b.
static size_t item_head_layout(const P5Engine* e, char* base, size_t Md, size_t Nup, P5Engine::ItemLoss* h) {
  const size_t sz = e->c.dtype == 1 ? 2 : 4, d = (size_t)e->c.d_model;
  Bump b{base, 0};
  void* EU = b.take(Nup * d * sz);
  float* lg = (float*)b.take(Md * Nup * 4);
  void* dl = b.take(Md * Nup * sz);
  float* dEU = (float*)b.take(Nup * d * 4);
  if (h) { h->EU = EU; h->logitsU = lg; h->dlogitsU = dl; h->dEU = dEU; }
  return b.off;
}
static unsigned item_head_blocks(long long pieces) {
  const long long b = (pieces + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

static int64_t layout_ws(P5Engine* e, char* base, int B, int L, int T, bool with_bwd, int G = 1) {
  const P5Config& c = e->c;
  const size_t sz = c.dtype == 1 ? 2 : 4;
  const int d = c.d_model, in = e->inner, F = c.d_ff, H = c.n_heads;
  const size_t M = (size_t)B * L, Bd = (size_t)B * G, Md = Bd * T;      // (G targets per user: the decoder's batch is B * G)
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  Bump b{base, 0};
  e->es.assign(c.n_enc_layers, LayerSave());
  e->ds.assign(c.n_dec_layers, LayerSave());
  e->enc_x0 = b.take(M * d * sz);
  void* xprev = e->enc_x0;
  for (auto& l : e->es) {
    l.x_sa = xprev;
    l.n_sa = b.take(M * d * sz); l.rstd_sa = (float*)b.take(M * 4);
    l.ssq_sa = (float*)b.take(M * (d / 64) * 4); l.ssq_ff = (float*)b.take(M * (d / 64) * 4); l.ssq_ca = nullptr;
    l.qkv = b.take(M * 3 * in * sz); l.o_sa = b.take(M * in * sz); l.lse_sa = (float*)b.take((size_t)B * H * L * 4);
    // long sequences (the head-resident attention kernels): the forward's dropout decisions as bit masks for the two backward passes
    l.keep_sa = (with_bwd && c.dtype == 1 && L > 128 && g_opt_attn_keep_bits) ? (uint32_t*)b.take((size_t)B * H * ((L + 15) / 16) * 1024) : nullptr;
    l.x_ff = b.take(M * d * sz);
    l.n_ff = b.take(M * d * sz); l.rstd_ff = (float*)b.take(M * 4);
    l.u_ff = c.gated_gelu ? b.take(M * 2 * F * sz) : nullptr;
    l.h_ff = b.take(M * F * sz);
    xprev = b.take(M * d * sz);
  }
  e->enc_xf = xprev;
  e->ssq_scratch = (float*)b.take((M > Md ? M : Md) * (d / 64) * 4);     // statistics of rows nobody normalises through a GEMM (stack outputs)
  e->enc_rstd_f = (float*)b.take(M * 4);
  e->enc_out = b.take(M * d * sz);
  if (T > 0) {
    e->dec_ids = (int64_t*)b.take(Md * 8);
    e->dec_x0 = b.take(Md * d * sz);
    xprev = e->dec_x0;
    for (auto& l : e->ds) {
      l.x_sa = xprev;
      l.n_sa = b.take(Md * d * sz); l.rstd_sa = (float*)b.take(Md * 4);
      l.ssq_sa = (float*)b.take(Md * (d / 64) * 4); l.ssq_ca = (float*)b.take(Md * (d / 64) * 4); l.ssq_ff = (float*)b.take(Md * (d / 64) * 4);
      l.qkv = b.take(Md * 3 * in * sz); l.o_sa = b.take(Md * in * sz); l.lse_sa = (float*)b.take(Bd * H * T * 4);
      l.keep_sa = nullptr;
      l.x_ca = b.take(Md * d * sz);
      l.n_ca = b.take(Md * d * sz); l.rstd_ca = (float*)b.take(Md * 4);
      l.q_ca = b.take(Md * in * sz); l.o_ca = b.take(Md * in * sz);
      l.lse_ca = (float*)b.take(Bd * H * T * 4);      // [B, H, G * T]
      l.x_ff = b.take(Md * d * sz);
      l.n_ff = b.take(Md * d * sz); l.rstd_ff = (float*)b.take(Md * 4);
      l.u_ff = c.gated_gelu ? b.take(Md * 2 * F * sz) : nullptr;
      l.h_ff = b.take(Md * F * sz);
      xprev = b.take(Md * d * sz);
    }
    e->dec_xf = xprev;
    // cross-attention K/V of all layers: [M, n_dec * 2 * inner]; layer i owns columns [i * 2 * inner, (i + 1) * 2 * inner)
    e->kv_all = b.take(M * (size_t)c.n_dec_layers * 2 * in * sz);
    for (size_t i = 0; i < e->ds.size(); ++i) e->ds[i].kv_ca = e->kv_all ? (char*)e->kv_all + i * 2 * in * sz : nullptr;
    e->dec_rstd_f = (float*)b.take(Md * 4);
    e->dec_hn = b.take(Md * d * sz);
    e->logits = (float*)b.take(Md * Vp * 4);
    e->lse_tok = (float*)b.take(Md * 4);
    e->ce_part = (float*)b.take(Md * (size_t)(Vp / 64) * 2 * 4);
    e->ce_lab = (float*)b.take(Md * 4);
    e->ce_g = (float*)b.take(Md * 4);
  }
  if (with_bwd) {
    const size_t Mx = M > Md ? M : Md;
    e->dres_a = (float*)b.take(Mx * d * 4);
    {   // (also the partial products of the tied head's deterministic split-K input gradient: up to P5_HEAD_SPLITS slices of [Md, d])
      const size_t need = Md * d * 4 * P5_HEAD_SPLITS;
      e->dres_b = (float*)b.take(need > Mx * d * 4 ? need : Mx * d * 4);
    }
    e->d_enc = (float*)b.take(M * d * 4);
    e->Dvec = (float*)b.take((size_t)H * ((size_t)B * L > Bd * T ? (size_t)B * L : Bd * T) * 4);
    e->rel_partial = (float*)b.take(((size_t)c.n_enc_layers * rel_slots(B, L) + (size_t)c.n_dec_layers * rel_slots((int)Bd, T > 0 ? T : 1)) * c.rel_buckets * H * 4);
    e->dw_scratch = (float*)b.take((size_t)(2 * c.n_enc_layers + 3 * c.n_dec_layers + 2) * 1024 * d * 4);
    e->nb_dotbuf = (float*)b.take(Mx * (size_t)((F / 64 > H ? F / 64 : H) + 4) * 4);
    {
      const size_t n0 = M + Md, n1 = M;
      e->emb_idx[0] = (int*)b.take(4 * n0 * 4); e->emb_idx[1] = (int*)b.take(4 * n1 * 4);
      e->emb_csort[0] = (unsigned long long*)b.take(((n0 + P5_EMB_CHUNK - 1) / P5_EMB_CHUNK) * P5_EMB_CHUNK * 8);
      e->emb_csort[1] = (unsigned long long*)b.take(((n1 + P5_EMB_CHUNK - 1) / P5_EMB_CHUNK) * P5_EMB_CHUNK * 8);
      e->emb_part[0] = (float*)b.take(((n0 + P5_EMB_SEG - 1) / P5_EMB_SEG) * 2 * d * 4);
      e->emb_part[1] = (float*)b.take(((n1 + P5_EMB_SEG - 1) / P5_EMB_SEG) * 2 * d * 4);
      e->dres_dec0 = (float*)b.take((Md > 0 ? Md : 1) * d * 4);
    }
    e->dn = b.take(Mx * d * sz);
    e->dO = b.take(Mx * in * sz);
    for (int p = 0; p < P5_NSETS; ++p) {
      e->dy2[p] = b.take(Mx * d * sz);
      e->dqkv2[p] = b.take(Mx * 3 * in * sz);
      e->dkv2[p] = nullptr;
      e->dh2[p] = b.take(Mx * F * sz);
      e->du2[p] = c.gated_gelu ? b.take(Mx * 2 * F * sz) : nullptr;
    }
    e->dy = e->dy2[0]; e->dqkv = e->dqkv2[0]; e->dkv = e->dkv2[0]; e->dh = e->dh2[0]; e->du = e->du2[0];
    e->dkv_all = T > 0 ? b.take(M * (size_t)c.n_dec_layers * 2 * in * sz) : nullptr;     // d(K/V) of all layers, same column layout
    e->dlogits = b.take(Md * Vp * sz);
    // the decoder sub-layers' own temporaries (weight-gradient plan, bf16 engine): [ffn | cross attention | self attention] per layer, in
    // the order the backward reaches them -- constant strides from layer to layer, so that one filler entry covers a weight of all layers
    e->ds_dy.clear(); e->ds_dh.clear(); e->ds_du.clear(); e->ds_dqkv.clear();
    if (T > 0 && c.dtype == 1) {
      for (int l = 0; l < c.n_dec_layers; ++l)
        for (int k = 0; k < 3; ++k) {
          e->ds_dy.push_back(b.take(Md * d * sz));
          e->ds_dh.push_back(k == 0 ? b.take(Md * F * sz) : nullptr);
          e->ds_du.push_back(k == 0 && c.gated_gelu ? b.take(Md * 2 * F * sz) : nullptr);
          e->ds_dqkv.push_back(k != 0 ? b.take(Md * (k == 1 ? 1 : 3) * in * sz) : nullptr);      // (cross attention: dQ only)
        }
    }
  }
  return (int64_t)((b.off + 255) & ~(size_t)255);
}

// ---- shared sub-layer forward helpers -----------------------------------------------------------------
// T5LayerNorm of the TRAINING forward folded into the GEMMs around it (bf16 engine with the folded weight copy bound): the producer of a
// residual-stream row leaves d/64 partial sums of squares behind, the consuming projection multiplies the raw row with W diag(ln) and
// scales its accumulator rows by rstd.  The normalised rows the weight gradients need are written by the norm BACKWARD kernel.
static int g_opt_norm_fuse = getenv("P5_NORM_FUSE") ? atoi(getenv("P5_NORM_FUSE")) : 1;
// (the weight gradients must be the deferred, layer-grouped ones: they run after the sub-layer's norm backward has written n)
template <class T> static bool norm_fused(const P5Engine* e) {
  return sizeof(T) == 2 && e->Sf != nullptr && g_opt_norm_fuse != 0 && (e->Md == 0 || wg_all_deferred<T>(e));
}
template <class T> static const T* Wnf(const P5Engine* e, int64_t off) { return (const T*)((const bf16*)e->Sf + off); }

// xout = x_ff + drop(wo(act(wi(norm(x_ff)))));  ssq_next: where to leave the statistics of xout (fused mode)
// gated-GELU FFN (T5 v1.1; HF modeling_t5.py:97-123): the gate runs in the epilogue of the wi GEMM (forward) / of the wo data-gradient GEMM
// (backward) wherever those GEMMs take the wide whole-tile path (p5_gemm5.h: bf16, rows % 256 == 0, >= 160 tiles); elsewhere -- the
// decoder's 512 rows, fp32 parity mode, ragged batches -- the stand-alone p5_gated_gelu_fwd / _bwd kernels.  Option "gate_fuse" 0 = never.
static int g_opt_gate_fuse = getenv("P5_GATE_FUSE") ? atoi(getenv("P5_GATE_FUSE")) : 1;
template <class T> static bool gate_fused(int rows, int N, int K) {
  return sizeof(T) == 2 && g_opt_gate_fuse != 0 && p5l_gemm_gate_ok(rows, N, K, K, K);
}
template <class T>
static int ffn_fwd(P5Engine* e, hipStream_t s, const LayerOff& lo, LayerSave& l, void* xout, int rows, int stack, int li, float* ssq_next) {
  const P5Config& c = e->c;
  const int d = c.d_model, F = c.d_ff;
  const bool nf = norm_fused<T>(e);
  if (!nf) P5_TRY(rmsnorm_fwd<T>(s, l.n_ff, l.rstd_ff, l.x_ff, e->P + lo.ff_ln, rows, d, c.eps, no_drop()));
  if (c.gated_gelu && gate_fused<T>(rows, 2 * F, d)) {
    // h = drop(gelu_new(u0) * u1) in the epilogue of ONE GEMM over [wi_0; wi_1] (rows read gate-interleaved), u kept for the backward
    P5GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = nf ? l.x_ff : l.n_ff; g.B = nf ? Wnf<T>(e, lo.wi) : Wc<T>(e, lo.wi); g.C = l.h_ff; g.C2 = l.u_ff;
    g.M = rows; g.N = 2 * F; g.K = d; g.lda = d; g.ldb = d; g.ldc = F; g.ldc2 = 2 * F; g.gate_F = F;
    g.epi = P5_EPI_GELU_GATE; g.alpha = 1.f; g.drop = mk_drop(e, stack, li, 5);
    if (nf) { g.rowss = l.ssq_ff; g.rowss_invd = 1.0f / (float)d; g.rowss_eps = c.eps; g.rowss_nt = d / 64; }
    P5_TRY(launch_gemm<T>(g, s));
  } else if (c.gated_gelu) {
    if (nf) P5_TRY(gemm_nf<T>(s, l.x_ff, d, Wnf<T>(e, lo.wi), d, l.u_ff, 2 * F, rows, 2 * F, d, P5_EPI_STORE, nullptr, 0, no_drop(), l.ssq_ff, c.eps, nullptr, d));
    else P5_TRY(linear_fwd<T>(s, l.n_ff, d, Wc<T>(e, lo.wi), l.u_ff, 2 * F, rows, 2 * F, d));
    const size_t n = (size_t)rows * F;
    P5_LAUNCH((p5_gated_gelu_fwd_kernel<T>), dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, s,
              (T*)l.h_ff, (const T*)l.u_ff, rows, F, mk_drop(e, stack, li, 5));
    P5_TRY(P5_KCHECK());
  } else if (nf) {
    P5_TRY(gemm_nf<T>(s, l.x_ff, d, Wnf<T>(e, lo.wi), d, l.h_ff, F, rows, F, d, P5_EPI_RELU_DROP, nullptr, 0, mk_drop(e, stack, li, 5), l.ssq_ff, c.eps, nullptr, d));
  } else {
    P5_TRY(linear_fwd<T>(s, l.n_ff, d, Wc<T>(e, lo.wi), l.h_ff, F, rows, F, d, P5_EPI_RELU_DROP, nullptr, 0, 1.f, 0, mk_drop(e, stack, li, 5)));
  }
  if (nf) return gemm_nf<T>(s, l.h_ff, F, Wc<T>(e, lo.wo), F, xout, d, rows, d, F, P5_EPI_RESID_DROP, l.x_ff, d, mk_drop(e, stack, li, 6), nullptr, 0.f, ssq_next, d);
  return linear_fwd<T>(s, l.h_ff, F, Wc<T>(e, lo.wo), xout, d, rows, d, F, P5_EPI_RESID_DROP, l.x_ff, d, 1.f, 0, mk_drop(e, stack, li, 6));
}

template <class T>
static int encoder_fwd(P5Engine* e, hipStream_t s) {
  const P5Config& c = e->c;
  const int d = c.d_model, in = e->inner, H = c.n_heads, M = e->M;
  const bool nf = norm_fused<T>(e);
  P5_LAUNCH((p5_embed_fwd_kernel<T>), dim3((M + 3) / 4), dim3(256), 0, s, (T*)e->enc_x0, Wc<T>(e, e->off_E), Wc<T>(e, e->off_WW), e->ids,
            e->ww, M, d, mk_drop(e, 0, 0, 0), nf ? e->es[0].ssq_sa : (float*)nullptr);
  P5_TRY(P5_KCHECK());
  for (int i = 0; i < c.n_enc_layers; ++i) {
    const LayerOff& lo = e->enc[i];
    LayerSave& l = e->es[i];
    void* xnext = (i + 1 < c.n_enc_layers) ? e->es[i + 1].x_sa : e->enc_xf;
    float* ssq_next = (i + 1 < c.n_enc_layers) ? e->es[i + 1].ssq_sa : e->ssq_scratch;
    if (nf) {
      P5_TRY(gemm_nf<T>(s, l.x_sa, d, Wnf<T>(e, lo.sa.q), d, l.qkv, 3 * in, M, 3 * in, d, P5_EPI_STORE, nullptr, 0, no_drop(), l.ssq_sa, c.eps, nullptr, d));
    } else {
      P5_TRY(rmsnorm_fwd<T>(s, l.n_sa, l.rstd_sa, l.x_sa, e->P + lo.sa.ln, M, d, c.eps, no_drop()));
      P5_TRY(linear_fwd<T>(s, l.n_sa, d, Wc<T>(e, lo.sa.q), l.qkv, 3 * in, M, 3 * in, d));
    }
    P5AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = l.qkv; a.K = (const T*)l.qkv + in; a.V = (const T*)l.qkv + 2 * in; a.O = l.o_sa; a.lse = l.lse_sa;
    a.rel_table = e->P + e->off_enc_rel; a.bucket_lut = e->lut_enc; a.lut_half = e->lut_half; a.kmask = e->mask;
    a.B = e->B; a.H = H; a.Lq = e->L; a.Lk = e->L; a.ldq = a.ldk = a.ldv = 3 * in; a.ldo = in; a.causal = 0;
    a.drop = mk_drop(e, 0, i, 1);
    a.keep_bits = (g_opt_attn_fwd_head && g_opt_attn_bwd_head && g_opt_attn_keep_bits) ? l.keep_sa : nullptr;      // (both passes on the head-resident kernels, or neither reads / writes the masks)
    P5_TRY(launch_attn_fwd<T>(a, s));
    if (nf) P5_TRY(gemm_nf<T>(s, l.o_sa, in, Wc<T>(e, lo.sa.o), in, l.x_ff, d, M, d, in, P5_EPI_RESID_DROP, l.x_sa, d, mk_drop(e, 0, i, 2), nullptr, 0.f, l.ssq_ff, d));
    else P5_TRY(linear_fwd<T>(s, l.o_sa, in, Wc<T>(e, lo.sa.o), l.x_ff, d, M, d, in, P5_EPI_RESID_DROP, l.x_sa, d, 1.f, 0, mk_drop(e, 0, i, 2)));
    P5_TRY(ffn_fwd<T>(e, s, lo, l, xnext, M, 0, i, ssq_next));
  }
  return rmsnorm_fwd<T>(s, e->enc_out, e->enc_rstd_f, e->enc_xf, e->P + e->off_enc_fln, M, d, c.eps, mk_drop(e, 0, 0, 7));
}

// Logit-free cross-entropy: in bf16 training the tied head's [B*T, V] logits (66 MB fp32 at C2) are never written -- the head
// GEMM's epilogue reduces every 64 columns of a row to (max, sum exp) and picks the label's logit, p5_ce_finish_kernel merges them into the
// row's log-sum-exp and NLL; the backward recomputes the same GEMM and its epilogue writes dlogits directly.  Option "ce_free" 0 = the
// materialised path (fp32 parity mode and shapes the wide kernel does not take always use it).
static int g_opt_ce_free = getenv("P5_CE_FREE") ? atoi(getenv("P5_CE_FREE")) : 1;
template <class T> static bool ce_free(const P5Engine* e) {
  return sizeof(T) == 2 && g_opt_ce_free != 0 && p5l_gemm_ce_ok(e->Md, e->c.vocab_size, e->c.d_model, e->c.d_model, e->c.d_model);
}
template <class T>
static int decoder_fwd(P5Engine* e, hipStream_t s, float* nll_out = nullptr) {
  const P5Config& c = e->c;
  const int d = c.d_model, in = e->inner, H = c.n_heads, M = e->M, Md = e->Md;
  const int nd_ = c.n_dec_layers, ldkv = nd_ * 2 * in;
  {
    // K/V projections of the encoder output for every layer: layer 0 on its own (the decoder needs it first), the rest as
    // ONE GEMM over the contiguous weight block; on the side stream when there is one (they only depend on enc_out)
    hipStream_t ks = e->side ? e->side : s;
    if (e->side) fork_to_side(e, s);      // enc_out is ready
    P5_TRY(linear_fwd<T>(ks, e->enc_out, d, Wc<T>(e, e->dec[0].ca.k), e->ds[0].kv_ca, ldkv, M, 2 * in, d));
#ifndef P5_EMU
    if (e->side) hipEventRecord(e->kv_ev[0], e->side);
#endif
    if (nd_ > 1) {
      P5_TRY(linear_fwd<T>(ks, e->enc_out, d, Wc<T>(e, e->dec[1].ca.k), e->ds[1].kv_ca, ldkv, M, (nd_ - 1) * 2 * in, d));
#ifndef P5_EMU
      if (e->side) hipEventRecord(e->kv_ev[1], e->side);
#endif
    }
  }
  const bool nf = norm_fused<T>(e);
  if (g_opt_shift_fuse) {      // the lookup shifts the labels itself and leaves e->dec_ids behind (the backward and the embedding gradient read it)
    P5_LAUNCH((p5_embed_fwd_kernel<T>), dim3((Md + 3) / 4), dim3(256), 0, s, (T*)e->dec_x0, Wc<T>(e, e->off_E), (const T*)nullptr,
              (const int64_t*)nullptr, (const int64_t*)nullptr, Md, d, mk_drop(e, 1, 0, 0), nf ? e->ds[0].ssq_sa : (float*)nullptr, e->labels, e->dec_ids,
              e->T, (int64_t)c.pad_id);
  } else {
    P5_LAUNCH(p5_shift_right_kernel, dim3((Md + 255) / 256), dim3(256), 0, s, e->dec_ids, e->labels, e->Bd, e->T, (int64_t)c.pad_id);
    P5_TRY(P5_KCHECK());
    P5_LAUNCH((p5_embed_fwd_kernel<T>), dim3((Md + 3) / 4), dim3(256), 0, s, (T*)e->dec_x0, Wc<T>(e, e->off_E), (const T*)nullptr,
              (const int64_t*)e->dec_ids, (const int64_t*)nullptr, Md, d, mk_drop(e, 1, 0, 0), nf ? e->ds[0].ssq_sa : (float*)nullptr);
  }
  P5_TRY(P5_KCHECK());
  for (int i = 0; i < c.n_dec_layers; ++i) {
    const LayerOff& lo = e->dec[i];
    LayerSave& l = e->ds[i];
    void* xnext = (i + 1 < c.n_dec_layers) ? e->ds[i + 1].x_sa : e->dec_xf;
    float* ssq_next = (i + 1 < c.n_dec_layers) ? e->ds[i + 1].ssq_sa : e->ssq_scratch;
    // self attention (causal, unidirectional buckets)
    if (nf) {
      P5_TRY(gemm_nf<T>(s, l.x_sa, d, Wnf<T>(e, lo.sa.q), d, l.qkv, 3 * in, Md, 3 * in, d, P5_EPI_STORE, nullptr, 0, no_drop(), l.ssq_sa, c.eps, nullptr, d));
    } else {
      P5_TRY(rmsnorm_fwd<T>(s, l.n_sa, l.rstd_sa, l.x_sa, e->P + lo.sa.ln, Md, d, c.eps, no_drop()));
      P5_TRY(linear_fwd<T>(s, l.n_sa, d, Wc<T>(e, lo.sa.q), l.qkv, 3 * in, Md, 3 * in, d));
    }
    P5AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = l.qkv; a.K = (const T*)l.qkv + in; a.V = (const T*)l.qkv + 2 * in; a.O = l.o_sa; a.lse = l.lse_sa;
    a.rel_table = e->P + e->off_dec_rel; a.bucket_lut = e->lut_dec; a.lut_half = e->lut_half; a.kmask = nullptr;
    a.B = e->Bd; a.H = H; a.Lq = e->T; a.Lk = e->T; a.ldq = a.ldk = a.ldv = 3 * in; a.ldo = in; a.causal = 1;
    a.drop = mk_drop(e, 1, i, 1);
    P5_TRY(launch_attn_fwd<T>(a, s));
    if (nf) {
      P5_TRY(gemm_nf<T>(s, l.o_sa, in, Wc<T>(e, lo.sa.o), in, l.x_ca, d, Md, d, in, P5_EPI_RESID_DROP, l.x_sa, d, mk_drop(e, 1, i, 2), nullptr, 0.f, l.ssq_ca, d));
      // cross attention (zero position bias + encoder padding mask)
      P5_TRY(gemm_nf<T>(s, l.x_ca, d, Wnf<T>(e, lo.ca.q), d, l.q_ca, in, Md, in, d, P5_EPI_STORE, nullptr, 0, no_drop(), l.ssq_ca, c.eps, nullptr, d));
    } else {
      P5_TRY(linear_fwd<T>(s, l.o_sa, in, Wc<T>(e, lo.sa.o), l.x_ca, d, Md, d, in, P5_EPI_RESID_DROP, l.x_sa, d, 1.f, 0, mk_drop(e, 1, i, 2)));
      P5_TRY(rmsnorm_fwd<T>(s, l.n_ca, l.rstd_ca, l.x_ca, e->P + lo.ca.ln, Md, d, c.eps, no_drop()));
      P5_TRY(linear_fwd<T>(s, l.n_ca, d, Wc<T>(e, lo.ca.q), l.q_ca, in, Md, in, d));
    }
#ifndef P5_EMU
    if (e->side && (i == 0 || (i == 1 && nd_ > 1))) hipStreamWaitEvent(s, e->kv_ev[i], 0);   // K/V projections were issued on the side stream up front
#endif
    memset(&a, 0, sizeof(a));
    a.Q = l.q_ca; a.K = l.kv_ca; a.V = (const T*)l.kv_ca + in; a.O = l.o_ca; a.lse = l.lse_ca;
    a.rel_table = nullptr; a.bucket_lut = nullptr; a.kmask = e->mask;
    a.B = e->B; a.H = H; a.Lq = e->Gt * e->T; a.Lk = e->L; a.ldq = in; a.ldk = a.ldv = ldkv; a.ldo = in; a.causal = 0;      // a user's G * T queries
    a.drop = mk_drop(e, 1, i, 3);
    P5_TRY(launch_attn_fwd<T>(a, s));
    if (nf) P5_TRY(gemm_nf<T>(s, l.o_ca, in, Wc<T>(e, lo.ca.o), in, l.x_ff, d, Md, d, in, P5_EPI_RESID_DROP, l.x_ca, d, mk_drop(e, 1, i, 4), nullptr, 0.f, l.ssq_ff, d));
    else P5_TRY(linear_fwd<T>(s, l.o_ca, in, Wc<T>(e, lo.ca.o), l.x_ff, d, Md, d, in, P5_EPI_RESID_DROP, l.x_ca, d, 1.f, 0, mk_drop(e, 1, i, 4)));
    P5_TRY(ffn_fwd<T>(e, s, lo, l, xnext, Md, 1, i, ssq_next));
  }
  P5_TRY(rmsnorm_fwd<T>(s, e->dec_hn, e->dec_rstd_f, e->dec_xf, e->P + e->off_dec_fln, Md, d, c.eps, mk_drop(e, 1, 0, 7)));
  // tied head, d^-0.5 rescale folded into alpha (P5_T5.py:352-361)
  const float alpha = 1.0f / sqrtf((float)d);
  e->ce_free_fwd = false;
  if (nll_out && !e->il.on && ce_free<T>(e)) {      // (the item loss reads the children's logits: materialised route)
    P5GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = e->dec_hn; g.B = Wc<T>(e, e->off_E); g.M = Md; g.N = c.vocab_size; g.K = d; g.lda = d; g.ldb = d;
    g.epi = P5_EPI_CE_STATS; g.alpha = alpha; g.drop = no_drop();
    g.ce_labels = e->labels; g.ce_part = e->ce_part; g.ce_lab = e->ce_lab; g.ce_np = (c.vocab_size + 63) / 64;
    P5_TRY(launch_gemm<T>(g, s));
    P5_LAUNCH((p5_ce_finish_kernel<T>), dim3((Md + 3) / 4), dim3(256), 0, s, nll_out, e->lse_tok, (const float*)e->ce_part, (const float*)e->ce_lab, e->labels, Md, g.ce_np);
    P5_TRY(P5_KCHECK());
    e->ce_free_fwd = true;
    return 0;
  }
  if (e->il.on && e->il.head) {
    // the head over the trie's tokens only: E_U = the rows U of the head weight, logits_U [Md, Nup] = alpha hn E_U^T
    P5Engine::ItemLoss& h = e->il;
    P5_REQUIRE(d % TT<T>::EPF == 0, "item head: d_model must be a multiple of 16 bytes");
    const size_t need = item_head_layout(e, (char*)h.head_ws, Md, h.Nup, &h);
    P5_REQUIRE(h.head_ws_bytes >= need, "item head: workspace too small for this batch (p5_item_head_workspace_bytes)");
    P5_LAUNCH((p5_item_gather_kernel<T>), dim3(item_head_blocks((long long)h.Nup * (d / TT<T>::EPF))), dim3(256), 0, s, (T*)h.EU, Wc<T>(e, e->off_E), h.head_tok,
              h.Nu, h.Nup, d);
    P5_TRY(P5_KCHECK());
    return linear_fwd<T>(s, e->dec_hn, d, (const T*)h.EU, h.logitsU, h.Nup, Md, h.Nup, d, P5_EPI_STORE, nullptr, 0, alpha, 1);
  }
  P5_TRY(linear_fwd<T>(s, e->dec_hn, d, Wc<T>(e, e->off_E), e->logits, e->Vp, Md, c.vocab_size, d, P5_EPI_STORE, nullptr, 0, alpha, 1));
  return 0;
}

template <class T>
static int forward_impl(P5Engine* e, float* nll_out, hipStream_t s) {
  P5_TRY(encoder_fwd<T>(e, s));
  P5_TRY(decoder_fwd<T>(e, s, nll_out));
  if (e->ce_free_fwd) return 0;       // (the head's epilogue + p5_ce_finish_kernel have written nll_out and the rows' log-sum-exp)
  if (e->il.on) {
    P5_LAUNCH(p5_trie_walk_kernel, dim3(e->Bd), dim3(256), 0, s, (int*)e->ce_lab, (int*)e->ce_g, e->il.state_out, e->labels, e->il.tr, e->T, e->c.pad_id,
              e->c.eos_id);
    P5_TRY(P5_KCHECK());
    // (restricted head: the compact row, columns through il.tr.col)
    const float* lg = e->il.head ? (const float*)e->il.logitsU : (const float*)e->logits;
    const int ldl = e->il.head ? e->il.Nup : e->Vp;
    if (e->il.trunc) {
      P5_LAUNCH((p5_trunc_ce_fwd_kernel<T>), dim3(e->Md), dim3(256), 0, s, nll_out, e->lse_tok, e->il.row_cut, (int*)e->ce_g, e->il.state_out,
                lg, e->labels, (const int*)e->ce_lab, e->il.tr, e->il.tc, e->T, ldl);
      return P5_KCHECK();
    }
    if (e->il.reg) {
      float* rt = e->il.row_terms;
      P5_LAUNCH((p5_trie_reg_fwd_kernel<T>), dim3(e->Md), dim3(256), 0, s, nll_out, e->lse_tok, rt, e->il.ref ? rt + e->Md : (float*)nullptr,
                e->il.ref ? rt + 2 * (size_t)e->Md : (float*)nullptr, lg, e->il.ref, e->labels, (const int*)e->ce_lab, (const int*)e->ce_g, e->il.tr,
                e->T, ldl, e->il.ld_ref);
      return P5_KCHECK();
    }
    P5_LAUNCH((p5_trie_ce_fwd_kernel<T>), dim3(e->Md), dim3(256), 0, s, nll_out, e->lse_tok, lg, e->labels, (const int*)e->ce_lab,
              (const int*)e->ce_g, e->il.tr, e->T, ldl);
    return P5_KCHECK();
  }
  P5_LAUNCH((p5_ce_fwd_kernel<T>), dim3(e->Md), dim3(256), 0, s, nll_out, e->lse_tok, (const float*)e->logits, e->labels, e->c.vocab_size, e->Vp);
  return P5_KCHECK();
}

// ---- backward ------------------------------------------------------------------------------------------
static int norm_flush(P5Engine* e, hipStream_t main);
// T5LayerNorm backward in the epilogue of the data-gradient GEMM that produces the norm's input gradient (P5_EPI_NORM_BWD, p5_gemm.h;
// round 6): no `dn` round trip, no stand-alone launch.  Needs the folded-norm forward (statistics as partial sums, n written by the
// backward), the transposed weight copy (K-contiguous operands), whole 128-row tiles, and a producer of dOut that leaves the row sums of
// <dOut, Out> in e->nb_dotbuf: the wide wo data-gradient GEMM (ReLU FFN) or the fused attention backward (encoder self-attention).
static int g_opt_norm_bwd_fuse = getenv("P5_NORM_BWD_FUSE") ? atoi(getenv("P5_NORM_BWD_FUSE")) : 1;
// (option 1: only where the N = d_model data gradient runs on 128-row tiles anyway -- at most one tile per CU, T5-small at the benchmark
//  batch; beyond that the 256x128 kernel's K loop is worth more than the saved pass: a T5-large FFN data gradient is 312 us there against 423.
//  2: wherever the shapes allow)
template <class T> static bool nb_fused(const P5Engine* e, int rows, int K) {
  const int d = e->c.d_model;
  return sizeof(T) == 2 && g_opt_norm_bwd_fuse != 0 && norm_fused<T>(e) && e->St != nullptr && g_opt_dgrad_t && e->nb_dotbuf != nullptr && (K % 64) == 0 &&
         p5l_gemm_normbwd_ok(rows, d, K, K, K) && (g_opt_norm_bwd_fuse >= 2 || (long)(rows / 128) * (d / 128) <= 256);
}
// dOut [rows, K] (T) x W^T copy -> residual gradient out (fp32), dy_next (T, dropout of the preceding sub-layer re-applied), n (T), norm-weight
// gradient partials; everything swap_norm_bwd does around its kernel, around the GEMM instead
template <class T>
static int norm_bwd_gemm(P5Engine* e, hipStream_t s, const void* dOut, int K, int64_t w_off, int rows, const void* x, const float* ssq, void* n_out,
                         int64_t ln_off, P5Drop dnext, int dot_nt) {
  const int d = e->c.d_model;
  float* out = (e->dres_cur == e->dres_a) ? e->dres_b : e->dres_a;
  if (e->dres_out_override) { out = e->dres_out_override; e->dres_out_override = nullptr; }
  end_sublayer_sync(e, s);             // (the epilogue writes dy_next and n: the set they live in must have been read out)
  float* part = e->dw_scratch + (size_t)(e->norm_slot++) * 1024 * d;
  P5_REQUIRE(rows / 64 <= 1024, "norm backward epilogue: more than 1024 partial rows of the norm-weight gradient");
  P5GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = dOut; g.B = (const T*)e->St + w_off; g.C = e->dy_next; g.C2 = n_out; g.aux = x;
  g.M = rows; g.N = d; g.K = K; g.lda = K; g.ldb = K; g.ldc = d; g.ldc2 = d; g.ldaux = d;
  g.epi = P5_EPI_NORM_BWD; g.alpha = 1.f; g.drop = dnext; g.splitk = 1;
  g.rowss = ssq; g.rowss_nt = d / 64; g.rowss_invd = 1.0f / (float)d; g.rowss_eps = e->c.eps;
  g.nb_dot = e->nb_dotbuf; g.nb_dot_nt = dot_nt; g.nb_rin = e->dres_cur; g.nb_rout = out; g.nb_w = e->P + ln_off; g.nb_dw = part;
  P5_TRY(launch_gemm<T>(g, s));
  {
    P5ReduceMulti& r = e->nr_pending;
    if (r.n == P5_REDUCE_MULTI_MAX) P5_TRY(norm_flush(e, s));
    r.d = d;
    r.nrows[r.n] = rows / 64;
    r.dst_off[r.n] = ln_off;
    r.part_off[r.n] = part - e->dw_scratch;
    r.n++;
  }
  e->dres_cur = out;
  e->nb_done = true;
  return 0;
}

// nb_*: the T5LayerNorm in front of the sub-layer (its input rows, their statistics, where n goes, the norm weight, the dropout of the
// sub-layer BEFORE it) -- used when the norm backward runs inside the wi data-gradient GEMM; e->nb_done then tells the caller
template <class T>
static int ffn_bwd(P5Engine* e, hipStream_t s, const LayerOff& lo, LayerSave& l, int rows, int stack, int li, P5Drop nb_dnext = no_drop()) {
  // in: e->dy = masked grad wrt the wo output (T), e->dres_cur = grad wrt the sub-layer output (fp32)
  const P5Config& c = e->c;
  const int d = c.d_model, F = c.d_ff;
  e->nb_done = false;
  const float hscale = (e->training && c.dropout > 0.f) ? 1.f / (1.f - c.dropout) : 1.f;
  P5_TRY(linear_wgrad<T>(e, s, e->dy, d, l.h_ff, F, e->G + lo.wo, rows, d, F));
  if (c.gated_gelu) {
    if (sizeof(T) == 2 && e->St && g_opt_dgrad_t && gate_fused<T>(rows, F, d)) {
      // dh = dy Wo never reaches memory: the epilogue of the data-gradient GEMM (on the transposed weight copy) writes du
      P5GemmArgs g;
      memset(&g, 0, sizeof(g));
      g.A = e->dy; g.B = (const T*)e->St + lo.wo; g.C = e->du; g.aux = l.u_ff;
      g.M = rows; g.N = F; g.K = d; g.lda = d; g.ldb = d; g.ldc = 2 * F; g.ldaux = 2 * F;
      g.epi = P5_EPI_GELU_GATE_BWD; g.alpha = 1.f; g.drop = mk_drop(e, stack, li, 5);
      P5_TRY(launch_gemm<T>(g, s));
    } else {
      P5_TRY(dgrad_w<T>(e, s, e->dy, d, lo.wo, e->dh, F, rows, d, F));
      const size_t n = (size_t)rows * F;
      P5_LAUNCH((p5_gated_gelu_bwd_kernel<T>), dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, s,
                (T*)e->du, (const T*)e->dh, (const T*)l.u_ff, rows, F, mk_drop(e, stack, li, 5));
      P5_TRY(P5_KCHECK());
    }
    P5_TRY(linear_wgrad<T>(e, s, e->du, 2 * F, l.n_ff, d, e->G + lo.wi, rows, 2 * F, d));
    P5_TRY(dgrad_w<T>(e, s, e->du, 2 * F, lo.wi, e->dn, d, rows, 2 * F, d));
  } else if (nb_fused<T>(e, rows, F) && p5l_gemm_gate_ok(rows, F, d, d, d) && l.ssq_ff && l.n_ff) {
    // dh = mask(dy Wo) leaves the row sums of <dh, pre> behind (32 partial sums per row at d_ff = 2048) ...
    P5GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = e->dy; g.B = (const T*)e->St + lo.wo; g.C = e->dh; g.aux = l.h_ff;
    g.M = rows; g.N = F; g.K = d; g.lda = d; g.ldb = d; g.ldc = F; g.ldaux = F;
    g.epi = P5_EPI_MASK_POS; g.alpha = hscale; g.drop = no_drop();
    g.ssq_out = e->nb_dotbuf; g.ssq_nt = F / 64;
    P5_TRY(launch_gemm<T>(g, s));
    P5_TRY(linear_wgrad<T>(e, s, e->dh, F, l.n_ff, d, e->G + lo.wi, rows, F, d));
    // ... and the wi data-gradient GEMM finishes the sub-layer: norm backward, residual add, next dy, n for the deferred weight gradient
    P5_TRY(norm_bwd_gemm<T>(e, s, e->dh, F, lo.wi, rows, l.x_ff, l.ssq_ff, l.n_ff, lo.ff_ln, nb_dnext, F / 64));
  } else {
    P5_TRY(dgrad_w<T>(e, s, e->dy, d, lo.wo, e->dh, F, rows, d, F, P5_EPI_MASK_POS, l.h_ff, F, hscale));
    P5_TRY(linear_wgrad<T>(e, s, e->dh, F, l.n_ff, d, e->G + lo.wi, rows, F, d));
    P5_TRY(dgrad_w<T>(e, s, e->dh, F, lo.wi, e->dn, d, rows, F, d));
  }
  return 0;
}

int norm_flush(P5Engine* e, hipStream_t main) {
  P5ReduceMulti& r = e->nr_pending;
  if (r.n == 0) return 0;
  P5_LAUNCH(p5_reduce_rows_multi_kernel, dim3((r.d + 15) / 16, r.n), dim3(256), 0, wgrad_stream(e, main), r, e->G, (const float*)e->dw_scratch);
  r.n = 0;
  return P5_KCHECK();
}

template <class T>
static int swap_norm_bwd(P5Engine* e, hipStream_t s, const void* x, int64_t ln_off, const float* rstd, int rows, P5Drop din, P5Drop dnext,
                         bool has_res_in = true, const float* ssq = nullptr, void* n_out = nullptr) {
  float* out = (e->dres_cur == e->dres_a) ? e->dres_b : e->dres_a;
  if (e->dres_out_override) { out = e->dres_out_override; e->dres_out_override = nullptr; }
  end_sublayer_sync(e, s);
  const int d = e->c.d_model;
  float* part = e->dw_scratch + (size_t)(e->norm_slot++) * 1024 * d;
  int nblk = 0;
  P5_TRY(rmsnorm_bwd<T>(s, out, e->dy_next, e->G + ln_off, e->dn, x, e->P + ln_off, rstd, has_res_in ? e->dres_cur : nullptr, rows, d, din,
                        dnext, part, &nblk, ssq, n_out, e->c.eps));
  // the per-workgroup partials are summed off the critical path, all norms of the stage in one launch (norm_flush)
  {
    P5ReduceMulti& r = e->nr_pending;
    if (r.n == P5_REDUCE_MULTI_MAX) P5_TRY(norm_flush(e, s));
    r.d = d;
    r.nrows[r.n] = nblk;
    r.dst_off[r.n] = ln_off;
    r.part_off[r.n] = part - e->dw_scratch;
    r.n++;
  }
  e->dres_cur = out;
  return 0;
}

template <class T>
static int self_attn_bwd(P5Engine* e, hipStream_t s, const LayerOff& lo, LayerSave& l, int rows, int Lq, bool is_dec, int li, P5Drop nb_dnext = no_drop()) {
  const P5Config& c = e->c;
  const int d = c.d_model, in = e->inner, H = c.n_heads;
  e->nb_done = false;
  P5_TRY(linear_wgrad<T>(e, s, e->dy, d, l.o_sa, in, e->G + lo.sa.o, rows, d, in));
  P5_TRY(dgrad_w<T>(e, s, e->dy, d, lo.sa.o, e->dO, in, rows, d, in));
  P5AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.Q = l.qkv; a.K = (const T*)l.qkv + in; a.V = (const T*)l.qkv + 2 * in; a.O = l.o_sa; a.lse = l.lse_sa; a.dO = e->dO;
  a.dQ = e->dqkv; a.dK = (T*)e->dqkv + in; a.dV = (T*)e->dqkv + 2 * in; a.Dvec = e->Dvec;
  a.rel_table = e->P + (is_dec ? e->off_dec_rel : e->off_enc_rel);
  a.rel_stride = c.rel_buckets * H;
  a.rel_copies = c.rel_buckets;
  // every layer's launch stores into its own block of slots (encoder layers first, then decoder layers): nothing to clear, nothing to add to
  // (blocks of exactly as many slots as the launch writes -- p5l_attn_bwd_slots -- so that a stack's blocks are contiguous rows for the reducer)
  const int sl_enc = p5l_attn_bwd_slots(sizeof(T) == 2, e->B, e->L, e->L), sl_dec = p5l_attn_bwd_slots(sizeof(T) == 2, e->Bd, e->T, e->T);
  a.d_rel_table = e->rel_partial + (is_dec ? ((size_t)c.n_enc_layers * rel_slots(e->B, e->L) + (size_t)li * sl_dec) * a.rel_stride
                                           : (size_t)li * sl_enc * a.rel_stride);
  a.bucket_lut = is_dec ? e->lut_dec : e->lut_enc; a.lut_half = e->lut_half; a.kmask = is_dec ? nullptr : e->mask;
  a.B = is_dec ? e->Bd : e->B; a.H = H; a.Lq = Lq; a.Lk = Lq; a.ldq = a.ldk = a.ldv = 3 * in; a.ldo = in; a.lddo = in;
  a.lddq = a.lddk = a.lddv = 3 * in; a.causal = is_dec ? 1 : 0;
  a.drop = mk_drop(e, is_dec ? 1 : 0, li, 1);
  a.keep_bits = (!is_dec && g_opt_attn_fwd_head && g_opt_attn_bwd_head && g_opt_attn_keep_bits) ? l.keep_sa : nullptr;
  // the attention backward leaves <dq, q> + <dk, k> + <dv, v> per token and head behind, and the qkv data-gradient GEMM runs the T5LayerNorm
  // backward of the sub-layer's input in its epilogue (norm_bwd_gemm above)
  const bool fuse = nb_fused<T>(e, rows, 3 * in) && p5l_attn_bwd_dot_ok(sizeof(T) == 2, a) && l.ssq_sa && l.n_sa;
  if (fuse) a.dot_out = e->nb_dotbuf;
  P5_TRY(launch_attn_bwd<T>(a, s));
  P5_TRY(linear_wgrad<T>(e, s, e->dqkv, 3 * in, l.n_sa, d, e->G + lo.sa.q, rows, 3 * in, d));
  if (fuse) return norm_bwd_gemm<T>(e, s, e->dqkv, 3 * in, lo.sa.q, rows, l.x_sa, l.ssq_sa, l.n_sa, lo.sa.ln, nb_dnext, H);
  P5_TRY(dgrad_w<T>(e, s, e->dqkv, 3 * in, lo.sa.q, e->dn, d, rows, 3 * in, d));
  return 0;
}

template <class T>
static int backward_stage_impl(P5Engine* e, const float* dnll, int stage, hipStream_t s) {
  const P5Config& c = e->c;
  const int d = c.d_model, in = e->inner, H = c.n_heads, M = e->M, Md = e->Md;
  const int nd = c.n_dec_layers, ne = c.n_enc_layers;
  if (stage == 0) {
    // the weight-gradient plan needs the whole backward in one call (gradient ranges become final in another order), one stream, every
    // weight gradient on the grouped path, and the decoder's own temporaries in the workspace.  It moves the tied head's weight gradient
    // from this stage to the encoder's launches, and on a storing micro-batch that store is what initialises shared.weight's gradient:
    // every embedding kernel that adds into it must run behind the last encoder group.  The segmented sums of the last stage do; the
    // atomic scatter of embed_det 0 adds the decoder's rows in stage nd + 1 -- no plan then.
    e->wg_plan = sizeof(T) == 2 && g_opt_wgrad_fill != 0 && g_opt_embed_det != 0 && e->whole_backward && !e->side && wg_all_deferred<T>(e) &&
                 (int)e->ds_dy.size() == 3 * nd;
    e->wg_pool.clear();
  }
  e->wg_pool_kind = !e->wg_plan ? -1 : stage == 0 ? 0 : stage <= nd ? 1 : stage == nd + 1 ? 2 : -1;
  e->wg_pool_layer = stage;
  if (stage == 0) {
    if (e->grads_keep) {
      e->wg_epi = P5_EPI_ACCUM;                 // a later micro-batch of an accumulation group: everything adds
    } else if (g_opt_grad_store_first && wg_all_deferred<T>(e)) {
      // (token counts that are multiples of 64 -- every batch of 64 sequences -- put ALL weight gradients on the grouped, storing
      //  path; ragged counts keep the clear-then-add form below: their split-K atomics need a cleared target anyway)
      if (!e->grads_zeroed) P5_TRY(zero_small_grads(e, s));
      e->wg_epi = P5_EPI_STORE;
    } else {
      if (!e->grads_zeroed) hipMemsetAsync(e->G, 0, (size_t)e->n_params * 4, s);     // (the caller may just have done it: zero_grad())
      e->wg_epi = P5_EPI_ACCUM;
    }
    e->grads_zeroed = false;
    e->grads_keep = false;
    e->d_enc_started = false;
    e->sub = -1;
    e->norm_slot = 0;
    e->nr_pending.n = 0;
#ifndef P5_EMU
    for (int i = 0; i < P5_NSETS; ++i) e->set_ev_valid[i] = false;
    e->head_wg_valid = false;
#endif
    begin_sublayer(e);
#ifndef P5_EMU
    if (e->tr_pending && e->tr_ev) { hipStreamWaitEvent(s, e->tr_ev, 0); hipStreamWaitEvent(e->side ? e->side : s, e->tr_ev, 0); }
#endif
    e->tr_pending = false;
#ifndef P5_EMU
    if (e->zg_pending && e->zg_ev) { hipStreamWaitEvent(s, e->zg_ev, 0); if (e->side) hipStreamWaitEvent(e->side, e->zg_ev, 0); }
#endif
    e->zg_pending = false;
    if (!dnll) P5_REQUIRE(e->out_attn, "backward without dnll needs p5_forward_loss (output_attention mask)");
    struct ItemGradsOnce { P5Engine* e; ~ItemGradsOnce() { e->bw_dH = e->bw_dKL = nullptr; } } item_grads_once{e};      // one-shot, whatever stage 0 returns
    if (!dnll && e->clip.on) {
      // the clipped objective's kernel has written this backward's seeds (and the regularisers'): every route below takes them as it takes autograd's
      dnll = e->clip.seed;
      if (e->il.on && e->il.reg) { e->bw_dH = e->clip.seed + Md; e->bw_dKL = e->clip.seed + 2 * (size_t)Md; }
    }
    if (!dnll && e->pref.on) dnll = e->pref.seed;      // the preference objective's kernel has written this backward's seeds
    const float alpha = 1.0f / sqrtf((float)d);
    // the head's logits, their gradient and their leading dimension: the vocabulary's, or -- item loss on the restricted head
    // (p5_item_head.h) -- the compact arrays of the caller's workspace
    const bool hd = e->il.on && e->il.head;
    const float* hd_lg = hd ? (const float*)e->il.logitsU : (const float*)e->logits;
    void* hd_dl = hd ? e->il.dlogitsU : e->dlogits;
    const int hd_ld = hd ? e->il.Nup : e->Vp;
    if (e->ce_free_fwd) {
      // dlogits = (softmax - onehot) * g straight out of the recomputed head GEMM (same operands, same accumulation order: the same logits)
      if (dnll || !e->ce_g_ready || !e->training) {      // (otherwise the loss kernel of p5_forward_loss* has written them)
        P5_LAUNCH(p5_ce_gscale_kernel, dim3((Md + 255) / 256), dim3(256), 0, s, e->ce_g, e->labels, dnll, e->out_attn, e->T, 1.0f / (float)e->Bd, Md, e->tgt_w);
        P5_TRY(P5_KCHECK());
        e->ce_g_ready = false;      // (dnll's values are not the masked-mean rule's)
      }
      P5GemmArgs g;
      memset(&g, 0, sizeof(g));
      g.A = e->dec_hn; g.B = Wc<T>(e, e->off_E); g.C = e->dlogits; g.M = Md; g.N = c.vocab_size; g.K = d; g.lda = d; g.ldb = d; g.ldc = e->Vp;
      g.epi = P5_EPI_CE_GRAD; g.alpha = alpha; g.drop = no_drop();
      g.ce_labels = e->labels; g.ce_lse = e->lse_tok; g.ce_g = e->ce_g; g.ce_np = (c.vocab_size + 63) / 64;
      P5_TRY(launch_gemm<T>(g, s));
    } else if (e->il.on && e->il.trunc) {
      P5_LAUNCH((p5_trunc_ce_bwd_kernel<T>), dim3(Md), dim3(256), 0, s, (T*)hd_dl, hd_lg, (const float*)e->lse_tok,
                (const float*)e->il.row_cut, e->labels, (const int*)e->ce_lab, (const int*)e->ce_g, dnll, e->il.tr, hd_ld, hd_ld, e->out_attn, e->T,
                1.0f / (float)e->Bd);
      P5_TRY(P5_KCHECK());
    } else if (e->il.on && e->il.reg) {
      const float* rt = e->il.row_terms;
      P5_LAUNCH((p5_trie_reg_bwd_kernel<T>), dim3(Md), dim3(256), 0, s, (T*)hd_dl, hd_lg, e->il.ref, (const float*)e->lse_tok, rt, rt + Md,
                rt + 2 * (size_t)Md, e->labels, (const int*)e->ce_lab, (const int*)e->ce_g, dnll, e->bw_dH, e->bw_dKL, e->il.tr, hd_ld, e->il.ld_ref,
                hd_ld, e->out_attn, e->T, 1.0f / (float)e->Bd, e->il.ent_coef, e->il.kl_coef);
      P5_TRY(P5_KCHECK());
    } else if (e->il.on) {
      P5_LAUNCH((p5_trie_ce_bwd_kernel<T>), dim3(Md), dim3(256), 0, s, (T*)hd_dl, hd_lg, (const float*)e->lse_tok, e->labels,
                (const int*)e->ce_lab, (const int*)e->ce_g, dnll, e->il.tr, hd_ld, hd_ld, e->out_attn, e->T, 1.0f / (float)e->Bd);
      P5_TRY(P5_KCHECK());
    } else {
      P5_LAUNCH((p5_ce_bwd_kernel<T>), dim3(Md, Md >= 2048 ? 1 : (Md >= 512 ? 4 : 8)), dim3(256), 0, s, (T*)e->dlogits, (const float*)e->logits, (const float*)e->lse_tok,
                e->labels, dnll, c.vocab_size, e->Vp, e->Vp, e->out_attn, e->T, 1.0f / (float)e->Bd, e->tgt_w);
      P5_TRY(P5_KCHECK());
    }
    // dE += alpha * dlogits^T hn ;  dhn = alpha * dlogits E
    if (hd) {
      // dE_U = alpha dlogits_U^T hn: ONE un-split GEMM that stores (one writer per element), then the scatter into shared.weight's gradient on
      // this stream -- ahead of the embedding sums of the last stage, which add into the same rows.  Nothing is queued: the weight-gradient
      // plan runs without head entries.  A storing backward writes ALL V rows (the arena was not cleared), the others add at the rows U.
      P5_TRY(gemm<T>(s, hd_dl, hd_ld, 1, e->dec_hn, d, 1, e->il.dEU, d, e->il.Nup, d, Md, P5_EPI_STORE, nullptr, 0, alpha, 1, no_drop()));
      const int store = e->wg_epi == P5_EPI_STORE ? 1 : 0;
      P5_LAUNCH(p5_item_scatter_kernel, dim3(item_head_blocks((long long)(store ? c.vocab_size : e->il.Nu) * (d / 4))), dim3(256), 0, s, e->G + e->off_E,
                (const float*)e->il.dEU, e->il.head_tok, e->il.Nu, c.vocab_size, d, store);
      P5_TRY(P5_KCHECK());
    } else {
      P5_TRY(linear_wgrad<T>(e, s, e->dlogits, e->Vp, e->dec_hn, d, e->G + e->off_E, Md, c.vocab_size, d, alpha));
      P5_TRY(wgrad_flush(e, s, true, (g_opt_wgrad_side & 1) != 0));
    }
    {
      // K = vocab is long and M*N small: split-K.  The splits STORE their partial products side by side and one pass sums them in index
      // order and casts -- not fp32 atomics into a cleared buffer: the order atomics land in changes from run to run, the bf16 rounding
      // of dhn then flips in a few elements, and that is the root of the whole backward (measured: two runs of the same step
      // differed by 1e-3 relative in every gradient tensor; with this, only the tensors that are themselves sums of atomics differ,
      // in their last bits).
      // (bf16: reduce over the padded vocabulary Vp = multiple of 64 so that both operands qualify for direct-to-LDS copies;
      //  dlogits columns V..Vp are exact zeros and the rows "E[V..Vp)" are the finite first rows of the next tensor in the arena)
      // (restricted head: the same block over K = Nup -- the rows [Nu, Nup) of E_U and the columns [Nu, Nup) of dlogits_U are exact zeros)
      const int Kv = hd ? e->il.Nup : sizeof(T) == 2 ? e->Vp : c.vocab_size;
      const void* hd_B = hd ? (const void*)e->il.EU : (const void*)Wc<T>(e, e->off_E);
      const bool big = Kv >= 16384 || (long)((Md + 127) / 128) * ((d + 127) / 128) >= 512;      // (launch_gemm's tile choice for this problem)
      const long tiles = big ? (long)((Md + 127) / 128) * ((d + 127) / 128) : (long)((Md + 63) / 64) * ((d + 63) / 64);
      const int nst = (Kv + 2 * TT<T>::KCH - 1) / (2 * TT<T>::KCH);         // K-steps of the 128x128 / 64x64 kernels (two K-chunks each)
      int want = (int)(((Kv >= 16384 ? 384 : 768) + tiles - 1) / tiles);
      want = want > P5_HEAD_SPLITS ? P5_HEAD_SPLITS : want;
      want = want > nst / 4 ? (nst / 4 > 0 ? nst / 4 : 1) : want;
      const int per = (nst + want - 1) / want, active = (nst + per - 1) / per;       // splits that have K-steps (the kernel's own arithmetic)
      {
        P5GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.A = hd_dl; g.B = hd_B; g.C = e->dres_b; g.M = Md; g.N = d; g.K = Kv; g.lda = hd_ld; g.ldb = d; g.ldc = d;
        g.a_ks = 0; g.b_ks = 1; g.epi = P5_EPI_ATOMIC; g.c_f32 = 1; g.splitk = want; g.alpha = alpha; g.drop = no_drop();
        g.rowss_invd = 1.0f / (float)Kv; g.c_split_stride = (long long)Md * d;
        P5_TRY(launch_gemm<T>(g, s));
      }
      const size_t n = (size_t)Md * d;
      P5_LAUNCH((p5_reduce_splits_kernel<T>), dim3((unsigned)((n / 8 + 255) / 256 > 4096 ? 4096 : (n / 8 + 255) / 256)), dim3(256), 0, s, (T*)e->dn,
                (const float*)e->dres_b, active, n, n);
      P5_TRY(P5_KCHECK());
    }
    e->dres_cur = e->dres_a;
    P5_TRY(swap_norm_bwd<T>(e, s, e->dec_xf, e->off_dec_fln, e->dec_rstd_f, Md, mk_drop(e, 1, 0, 7), mk_drop(e, 1, nd - 1, 6), false));
    return 0;
  }
  if (stage >= 1 && stage <= nd) {
    const int i = nd - stage;
    const LayerOff& lo = e->dec[i];
    LayerSave& l = e->ds[i];
    begin_sublayer(e);
    P5_TRY(ffn_bwd<T>(e, s, lo, l, Md, 1, i, mk_drop(e, 1, i, 4)));
    const bool nf = norm_fused<T>(e);
    if (!e->nb_done) P5_TRY(swap_norm_bwd<T>(e, s, l.x_ff, lo.ff_ln, l.rstd_ff, Md, no_drop(), mk_drop(e, 1, i, 4), true, nf ? l.ssq_ff : nullptr, nf ? l.n_ff : nullptr));
    e->nb_done = false;
    // cross attention
    begin_sublayer(e);
    P5_TRY(linear_wgrad<T>(e, s, e->dy, d, l.o_ca, in, e->G + lo.ca.o, Md, d, in));
    P5_TRY(dgrad_w<T>(e, s, e->dy, d, lo.ca.o, e->dO, in, Md, d, in));
    P5AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = l.q_ca; a.K = l.kv_ca; a.V = (const T*)l.kv_ca + in; a.O = l.o_ca; a.lse = l.lse_ca; a.dO = e->dO;
    const int ldkv = nd * 2 * in;
    T* dkv_i = (T*)e->dkv_all + (size_t)i * 2 * in;      // this layer's columns of d(K/V); consumed once, after the last layer
    a.dQ = e->dqkv; a.dK = dkv_i; a.dV = dkv_i + in; a.Dvec = e->Dvec;
    a.kmask = e->mask; a.B = e->B; a.H = H; a.Lq = e->Gt * e->T; a.Lk = e->L; a.ldq = in; a.ldk = a.ldv = ldkv; a.ldo = in; a.lddo = in;      // (dK / dV: summed over a user's G targets)
    a.lddq = in; a.lddk = a.lddv = ldkv; a.causal = 0; a.drop = mk_drop(e, 1, i, 3);
    P5_TRY(launch_attn_bwd<T>(a, s));
    P5_TRY(linear_wgrad<T>(e, s, e->dqkv, in, l.n_ca, d, e->G + lo.ca.q, Md, in, d));
    P5_TRY(dgrad_w<T>(e, s, e->dqkv, in, lo.ca.q, e->dn, d, Md, in, d));
    P5_TRY(swap_norm_bwd<T>(e, s, l.x_ca, lo.ca.ln, l.rstd_ca, Md, no_drop(), mk_drop(e, 1, i, 2), true, nf ? l.ssq_ca : nullptr, nf ? l.n_ca : nullptr));
    // self attention
    begin_sublayer(e);
    if (i == 0 && g_opt_embed_det) e->dres_out_override = e->dres_dec0;      // gradient of the decoder's embedding rows: consumed by the last stage
    P5_TRY(self_attn_bwd<T>(e, s, lo, l, Md, e->T, true, i, i > 0 ? mk_drop(e, 1, i - 1, 6) : no_drop()));
    if (!e->nb_done) P5_TRY(swap_norm_bwd<T>(e, s, l.x_sa, lo.sa.ln, l.rstd_sa, Md, no_drop(), i > 0 ? mk_drop(e, 1, i - 1, 6) : no_drop(), true, nf ? l.ssq_sa : nullptr,
                            nf ? l.n_sa : nullptr));
    e->nb_done = false;
    return wgrad_flush(e, s, false, (g_opt_wgrad_side & 1) != 0);     // the six weight gradients of the layer: one launch
  }
  if (stage == nd + 1) {
    {
      // every layer's d(K/V) is in place: ONE weight-gradient GEMM for the contiguous K/V block and ONE dgrad for d(enc_out)
      // (K = n_dec * 2 * inner), both off the critical path on the side stream; the encoder backward joins it (stage nd + 2)
      const int ldkv = nd * 2 * in;
      // weight gradient of the K/V block: with the side stream it goes out now; otherwise it stays queued and leaves with the top encoder
      // layer's group (one launch).  d(enc_out) is on the critical path of the encoder backward either way.
      P5_TRY(linear_wgrad<T>(e, s, e->dkv_all, ldkv, e->enc_out, d, e->G + e->dec[0].ca.k, M, ldkv, d));
      const bool side2 = e->side && (g_opt_wgrad_side & 2) != 0;
      if (side2 || !(e->whole_backward || e->stage_pairs)) P5_TRY(wgrad_flush(e, s, false, side2));
      P5_TRY(dgrad_w<T>(e, side2 ? e->side : s, e->dkv_all, ldkv, e->dec[0].ca.k, e->d_enc, d, M, ldkv, d, P5_EPI_STORE,
                             nullptr, 0, 1.f, 1));
    }
    P5_LAUNCH(p5_reduce_rows_kernel, dim3((c.rel_buckets * H + 15) / 16), dim3(256), 0, s, e->G + e->off_dec_rel,
              (const float*)(e->rel_partial + (size_t)c.n_enc_layers * rel_slots(e->B, e->L) * c.rel_buckets * H),
              c.n_dec_layers * p5l_attn_bwd_slots(sizeof(T) == 2, e->Bd, e->T, e->T), c.rel_buckets * H);
    P5_TRY(P5_KCHECK());
#ifndef P5_EMU
    // shared.weight's gradient: the tied head's weight gradient adds with plain read-modify-writes (side stream, stage 0); the
    // embedding scatters (atomics, from here on) must not run beside it
    if (e->side && e->head_wg_valid) { hipStreamWaitEvent(s, e->head_wg_ev, 0); e->head_wg_valid = false; }
#endif
    if (g_opt_embed_det) return 0;      // (the decoder's lookup rows join the encoder's in the last stage: one owner per row of the tied table)
    P5_LAUNCH((p5_embed_bwd_kernel<T>), dim3((Md + 3) / 4), dim3(256), 0, s, e->G + e->off_E, (float*)nullptr, (const float*)e->dres_cur,
              (const int64_t*)e->dec_ids, (const int64_t*)nullptr, Md, d, mk_drop(e, 1, 0, 0));
    return P5_KCHECK();
  }
  if (stage == nd + 2) {
    join_side(e, s);      // d_enc is accumulated on the side stream
    const size_t n = (size_t)M * d;
    P5_LAUNCH((p5_cast_mask_kernel<T>), dim3((unsigned)((n / 8 + 255) / 256 > 4096 ? 4096 : (n / 8 + 255) / 256)), dim3(256), 0, s, (T*)e->dn,
              (const float*)e->d_enc, n, no_drop());
    P5_TRY(P5_KCHECK());
    e->dres_cur = e->dres_a;
    begin_sublayer(e);
    P5_TRY(swap_norm_bwd<T>(e, s, e->enc_xf, e->off_enc_fln, e->enc_rstd_f, M, mk_drop(e, 0, 0, 7), mk_drop(e, 0, ne - 1, 6), false));
    return 0;
  }
  if (stage >= nd + 3 && stage <= nd + 2 + ne) {
    const int i = ne - (stage - (nd + 2));
    const LayerOff& lo = e->enc[i];
    LayerSave& l = e->es[i];
    begin_sublayer(e);
    P5_TRY(ffn_bwd<T>(e, s, lo, l, M, 0, i, mk_drop(e, 0, i, 2)));
    const bool nf = norm_fused<T>(e);
    if (!e->nb_done) P5_TRY(swap_norm_bwd<T>(e, s, l.x_ff, lo.ff_ln, l.rstd_ff, M, no_drop(), mk_drop(e, 0, i, 2), true, nf ? l.ssq_ff : nullptr, nf ? l.n_ff : nullptr));
    e->nb_done = false;
    begin_sublayer(e);
    P5_TRY(self_attn_bwd<T>(e, s, lo, l, M, e->L, false, i, i > 0 ? mk_drop(e, 0, i - 1, 6) : no_drop()));
    if (!e->nb_done) P5_TRY(swap_norm_bwd<T>(e, s, l.x_sa, lo.sa.ln, l.rstd_sa, M, no_drop(), i > 0 ? mk_drop(e, 0, i - 1, 6) : no_drop(), true, nf ? l.ssq_sa : nullptr,
                            nf ? l.n_sa : nullptr));
    e->nb_done = false;
    // the four weight gradients of the layer: one launch of 192 tiles over all 8192 tokens (or of 2 layers = 384 tiles when the
    // whole backward runs in one call and nobody waits for per-layer gradient ranges)
    // (the top layer's group also carries the cross-attention K/V block queued in the previous stage: 5 problems; then pairs of layers)
    const bool pairs = (e->whole_backward || e->stage_pairs) && g_opt_wgrad_layers > 1;
    if (e->wg_plan) {
      // pairs from the top ([L5,L4] [L3,L2] [L1,L0]; an odd bottom layer alone), each filled from the pool
      if (!pairs || i == 0 || ((ne - 1 - i) & 1)) return wgrad_plan_flush(e, s, i == 0);
      return 0;
    }
    if (!pairs || i == 0 || e->wg_pending.size() >= 5) return wgrad_flush(e, s, false, (g_opt_wgrad_side & 2) != 0);
    return 0;
  }
  if (stage == nd + ne + 3) {
    // the tail of the backward: nothing is left to overlap these with except each other -- the whole-word scatter and the
    // relative-bias reduction go to the side stream (p5_backward_stage joins it after this stage), the token scatter stays here
    hipStream_t s2 = s;
#ifndef P5_EMU
    if (e->side) { fork_to_side(e, s); s2 = e->side; }
#endif
    P5_LAUNCH(p5_reduce_rows_kernel, dim3((c.rel_buckets * H + 15) / 16), dim3(256), 0, s2, e->G + e->off_enc_rel,
              (const float*)e->rel_partial, c.n_enc_layers * p5l_attn_bwd_slots(sizeof(T) == 2, e->B, e->L, e->L), c.rel_buckets * H);
    P5_TRY(P5_KCHECK());
    if (g_opt_embed_det) {
      // embedding gradients without atomics (p5_embed.h): tied table over (encoder ids ++ decoder ids), whole-word table over the encoder's
      P5EmbArgs ea;
      memset(&ea, 0, sizeof(ea));
      ea.nsets = 2; ea.d = d;
      const int n[2] = {M + Md, M};
      for (int k = 0; k < 2; ++k) {
        P5EmbSet& q = ea.s[k];
        q.key0 = k == 0 ? e->ids : e->ww; q.dres0 = e->dres_cur; q.drop0 = mk_drop(e, 0, 0, 0); q.n0 = M;
        if (k == 0) { q.key1 = e->dec_ids; q.dres1 = e->dres_dec0; q.drop1 = mk_drop(e, 1, 0, 0); q.n1 = Md; }
        q.table = e->G + (k == 0 ? e->off_E : e->off_WW);
        q.perm = e->emb_idx[k]; q.skey = q.perm + n[k]; q.sstart = q.skey + n[k]; q.slen = q.sstart + n[k];
        q.part = e->emb_part[k];
        q.csort = e->emb_csort[k];
      }
      P5_LAUNCH(p5_embed_sortchunk_kernel, dim3((n[0] + P5_EMB_CHUNK - 1) / P5_EMB_CHUNK, 2), dim3(256), 0, s, ea);
      P5_TRY(P5_KCHECK());
      P5_LAUNCH(p5_embed_rank_kernel, dim3((n[0] + 63) / 64, 2), dim3(256), 0, s, ea);
      P5_TRY(P5_KCHECK());
      const int nblk = (n[0] + P5_EMB_SEG - 1) / P5_EMB_SEG;
      P5_LAUNCH(p5_embed_seg_kernel, dim3(nblk, 2), dim3(256), 0, s, ea);
      P5_TRY(P5_KCHECK());
      P5_LAUNCH(p5_embed_fix_kernel, dim3(nblk, 2), dim3(256), 0, s, ea);
      return P5_KCHECK();
    }
    // (a gather of the whole-word table's gradient -- one workgroup per (table row, 256-row slice), matching rows summed in
    //  registers, one atomic per column -- was measured: 4.545 vs 4.493 ms per step; index 0 (every pad) makes a few workgroups long)
    if (s2 != s) {
      P5_LAUNCH((p5_embed_bwd_kernel<T>), dim3((M + 3) / 4), dim3(256), 0, s2, (float*)nullptr, e->G + e->off_WW, (const float*)e->dres_cur,
                e->ids, e->ww, M, d, mk_drop(e, 0, 0, 0));
      P5_TRY(P5_KCHECK());
    }
    P5_LAUNCH((p5_embed_bwd_kernel<T>), dim3((M + 3) / 4), dim3(256), 0, s, e->G + e->off_E, s2 != s ? (float*)nullptr : e->G + e->off_WW,
              (const float*)e->dres_cur, e->ids, e->ww, M, d, mk_drop(e, 0, 0, 0));
    return P5_KCHECK();
  }
  return fail("backward: bad stage");
}

// ---- generation ------------------------------------------------------------------------------------------

static int head_nv(const P5Engine* e);
// which step a search of K beams runs: the narrow one (p5_decode.h, K <= 64) or the wide one (p5_decode_wide.h: K > 64, or any K under
// the gen_wide option -- except for p5_generate_draft, whose history recording only the narrow step does)
static bool gen_wide_layout(int K) { return K > P5_MAX_K || g_opt_gen_wide != 0; }
static bool gen_wide_run(int K, const int* hist) { return K > P5_MAX_K || (g_opt_gen_wide != 0 && hist == nullptr); }

static int64_t layout_gen(P5Engine* e, char* base, int B, int L, int K, int max_len, int max_c, int excl_words, GenWs* g) {
  const P5Config& c = e->c;
  const size_t sz = c.dtype == 1 ? 2 : 4;
  const int d = c.d_model, in = e->inner, F = c.d_ff;
  const size_t R = (size_t)B * K;
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  // (the encoder's buffers, and the training-layout decoder buffers of the forced-prefix pass: at most P5_FF_MAX positions per user)
  const int ffcap = g_opt_gen_ff ? (max_len - 2 < P5_FF_MAX ? (max_len - 2 > 0 ? max_len - 2 : 0) : P5_FF_MAX) : 0;
  const int64_t enc_bytes = layout_ws(e, base, B, L, ffcap, false);
  Bump b{base, (size_t)enc_bytes};
  GenWs tmp;
  GenWs& w = g ? *g : tmp;
  w.ff_labels = (int64_t*)b.take((size_t)B * (ffcap > 0 ? ffcap : 1) * 8);
  w.ff_nll = (float*)b.take((size_t)B * (ffcap > 0 ? ffcap : 1) * 4);
  {
    char* kv_all = (char*)b.take((size_t)B * L * c.n_dec_layers * 2 * in * sz);
    w.ldkv = c.n_dec_layers * 2 * in;
    for (int i = 0; i < c.n_dec_layers; ++i) {
      w.kv_cross[i] = base ? (void*)(kv_all + (size_t)i * 2 * in * sz) : nullptr;
      w.cache[i] = b.take((size_t)max_len * R * 2 * in * sz);
    }
  }
  w.qkv = b.take(R * 3 * in * sz); w.q = b.take(R * in * sz); w.o = b.take(R * in * sz);
  w.h = b.take(R * (c.gated_gelu ? 3 : 1) * F * sz); w.hn = b.take(R * d * sz);
  w.x32 = (float*)b.take(R * d * 4);
  // (beyond 64 beams only the wide step runs: no narrow candidate lists, and no [R, V] logits when the head streams)
  const bool narrow = K <= P5_MAX_K;
  w.logits = (float*)b.take(narrow || head_nv(e) == 0 ? R * Vp * 4 : 0);
  w.cand = (float*)b.take(R * (size_t)max_c * 4);
  w.cand_key = (int*)b.take(R * (size_t)max_c * 4);
  w.part_m = (float*)b.take(R * (size_t)((c.vocab_size + 15) / 16) * 4);
  w.part_s = (float*)b.take(R * (size_t)((c.vocab_size + 15) / 16) * 4);
  w.n_cand = (int*)b.take(R * 4);
  w.row_top_score = (float*)b.take(narrow ? R * (size_t)(2 * K) * 4 : 0);
  w.row_top_c = (int*)b.take(narrow ? R * (size_t)(2 * K) * 4 : 0);
  w.mask_copy = (int64_t*)b.take((size_t)B * L * 8);
  w.excluded = (uint32_t*)b.take((size_t)B * (excl_words > 0 ? excl_words : 0) * 4 + 16);
  P5BeamState& st = w.st;
  st.run_seq = (int*)b.take(R * max_len * 4); st.run_seq_next = (int*)b.take(R * max_len * 4);
  st.fin_seq = (int*)b.take(R * max_len * 4); st.fin_seq_next = (int*)b.take(R * max_len * 4);
  st.anc = (int*)b.take(R * max_len * 4); st.anc_next = (int*)b.take(R * max_len * 4);
  st.run_score = (float*)b.take(R * 4); st.run_node = (int*)b.take(R * 4);
  st.fin_score = (float*)b.take(R * 4); st.fin_flag = (int*)b.take(R * 4); st.fin_len = (int*)b.take(R * 4);
  st.unsat = (int*)b.take((size_t)B * 4);
  st.last_tok = (int64_t*)b.take(R * 8);
  st.flags = (int*)b.take(64);
  // latency-shaped decode step: the beam step itself writes the next step's input embeddings into the fp32 residual stream
  st.x32 = w.x32;
  st.E32 = e->P ? e->P + e->off_E : nullptr;
  st.d = d;
  st.hist = nullptr;
  // wide step (p5_decode_wide.h), behind everything above so that the narrow buffers keep their offsets under the gen_wide option
  memset(&w.wide, 0, sizeof(w.wide));
  w.wide_c = 0;
  if (gen_wide_layout(K)) {
    const int C = max_c < 2 * K ? max_c : 2 * K;
    w.wide_c = C;
    w.wide.row_key = (unsigned long long*)b.take(R * (size_t)C * 8);
    w.wide.row_n = (int*)b.take(R * 4);
    w.wide.top_lp = (float*)b.take(R * 2 * 4);
    w.wide.top_beam = (int*)b.take(R * 2 * 4);
    w.wide.top_tok = (int*)b.take(R * 2 * 4);
    w.wide.top_node = (int*)b.take(R * 2 * 4);
    w.wide.sel_run = (int*)b.take(R * 4);
    w.wide.fin_src = (int*)b.take(R * 4);
  }
  return (int64_t)((b.off + 255) & ~(size_t)255);
}

// ---- latency-shaped decode step (p5_decode2.h) ------------------------------------------------------------
// what the template parameters of a stringified decode-step kernel name stand for (the profiler's tag of the launch)
template <class T> static const char* dtype_name() { return sizeof(T) == 2 ? "bf16" : "fp32"; }
template <class T, int NB, int AMODE, int KB>
static const char* skinny_tag() {
  static const std::string t = std::string(dtype_name<T>()) + " NB=" + std::to_string(NB) + " AMODE=" + std::to_string(AMODE) + " LDSKB=" + std::to_string(KB);
  return t.c_str();
}
template <class T, int NB, int AMODE>
static int launch_skinny_nb(const P5SkinnyArgs& g, int splits, int need_bytes, hipStream_t s) {
  dim3 grid((g.N + NB - 1) / NB, (g.M + 15) / 16, splits), block(256);
  // (the static LDS size is what bounds the workgroups per CU: 52 KiB -> 3, 80 KiB -> 2 of the 160 KiB)
#define P5_SKINNY(KB) do { P5_PROF_TAG((skinny_tag<T, NB, AMODE, KB>())); P5_LAUNCH((p5_skinny_gemm_kernel<T, NB, AMODE, KB>), grid, block, 0, s, g); } while (0)
  if (need_bytes <= 44 * 1024) P5_SKINNY(44);
  else if (need_bytes <= 52 * 1024) P5_SKINNY(52);
  else if (need_bytes <= 80 * 1024) P5_SKINNY(80);
  else if (need_bytes <= 100 * 1024) P5_SKINNY(100);
  else if (need_bytes <= 140 * 1024) P5_SKINNY(140);
  else return fail("skinny gemm: tile does not fit the LDS");
#undef P5_SKINNY
  return P5_KCHECK();
}
// C = A W^T over M <= a few hundred rows.  amode 1: A is the fp32 residual stream, normalised (T5LayerNorm, weight `ln`) by the
// consumer itself (K = d_model, no split); amode 0: A is a T matrix, K may be split over workgroups (atomic epilogue only).
template <class T>
static int skinny(hipStream_t s, int amode, const void* A, int lda, const float* ln, const T* W, int ldw, void* C, int ldc, int M, int N, int K,
                  int epi, float alpha, float eps, const int* done) {
  constexpr int EPS = SkT<T>::EPS;
  P5_REQUIRE(M >= 1 && N >= 1 && K >= EPS && K % EPS == 0 && ldw % TT<T>::EPF == 0 && (amode == 1 || lda % TT<T>::EPF == 0), "skinny gemm: K / leading dims");
  P5_REQUIRE(amode != 1 || K <= 1024, "skinny gemm: the fused T5LayerNorm (sk_norm_rows) holds rows of at most 1024 columns");
  P5SkinnyArgs g;
  g.A = A; g.ln = ln; g.W = W; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.epi = epi; g.alpha = alpha; g.eps = eps;
  g.done = done;
  auto need = [&](int nb, int kw) { return (kw / EPS) * (2048 + nb * 128) + (nb < 64 ? 3072 : 0); };   // (+ cross-wave reduction buffer when waves split K)
  int nb = g_opt_dec_nb, kw = K, splits = 1;
  g.kpasses = 1;
  if (amode == 1) {
    if (!nb) nb = need(64, K) <= 80 * 1024 ? 64 : (need(32, K) <= 100 * 1024 ? 32 : 16);
  } else if (epi == P5_SK_RESID) {
    // one writer per output element (bit-reproducible residual update): no K split over workgroups -- narrow column tiles make the
    // workgroups (>= ~200 for 200 rows x 512 columns), and a long reduction is walked in passes of at most 80 KiB of operands
    if (!nb) nb = need(32, K) <= 52 * 1024 ? 32 : 16;
    kw = K;
    while (need(nb, kw) > 80 * 1024 && kw > 2 * EPS) kw = ((kw / 2 + EPS - 1) / EPS) * EPS;
    g.kpasses = (K + kw - 1) / kw;
  } else {
    if (!nb) nb = 64;
    // K range per workgroup: at most 512 (bf16) / 256 (fp32) elements -- one 80 KiB burst -- and enough splits for >= ~200 workgroups
    int cap = g_opt_dec_kw ? g_opt_dec_kw : (sizeof(T) == 2 ? 512 : 256);
    const int tiles = ((N + nb - 1) / nb) * ((M + 15) / 16);
    if (!g_opt_dec_kw && epi == P5_SK_ATOMIC)
      while (cap > 2 * EPS && tiles * ((K + cap - 1) / cap) < 192) cap /= 2;
    if (epi != P5_SK_ATOMIC) cap = K;
    kw = cap < K ? (cap / EPS) * EPS : K;
    splits = (K + kw - 1) / kw;
  }
  g.kw = kw;
  const int nbytes = need(nb, kw);
  if (amode == 1) {
    if (nb == 64) return launch_skinny_nb<T, 64, 1>(g, 1, nbytes, s);
    if (nb == 32) return launch_skinny_nb<T, 32, 1>(g, 1, nbytes, s);
    return launch_skinny_nb<T, 16, 1>(g, 1, nbytes, s);
  }
  if (nb == 64) return launch_skinny_nb<T, 64, 0>(g, splits, nbytes, s);
  if (nb == 32) return launch_skinny_nb<T, 32, 0>(g, splits, nbytes, s);
  return launch_skinny_nb<T, 16, 0>(g, splits, nbytes, s);
}

// streaming head: rows of E kept in LDS per workgroup (0 = materialised-logits path): the largest of 128/64/32/16 whose tile
// fits 128 KiB (bf16 d_model 512 -> 128, 768/1024 -> 64; fp32 512 -> 64, 768/1024 -> 32)
static int head_nv_of(int dtype, int d_model) {       // (p5_op_head_nv reports it: tests/rank_matrix.py)
  if (!g_opt_dec_head) return 0;
  // the kernel walks K in units of eight 64-byte chunks (p5_decode2.h): d_model % 256 (bf16) / % 128 (fp32) -- every T5 size;
  // other widths (toy models) take the materialised-logits head
  if (d_model % (dtype == 1 ? 256 : 128) != 0) return 0;
  const size_t row = (size_t)d_model * (dtype == 1 ? 2 : 4);
  if (g_opt_dec_head_nv) return (size_t)g_opt_dec_head_nv * row <= 128 * 1024 ? g_opt_dec_head_nv : 0;
  for (int nv = 128; nv >= 16; nv >>= 1)
    if ((size_t)nv * row <= 128 * 1024) return nv;
  return 0;
}
static int head_nv(const P5Engine* e) { return head_nv_of(e->c.dtype, e->c.d_model); }

// streaming tied head over R rows: per vocabulary tile (max, sum exp) only; the logits the search needs are recomputed by p5_dec_score2_kernel.
// nv = rows of E per workgroup, one of head_nv()'s values for (T, d); part_m / part_s: [R][ceil(V / nv)]
template <class T>
static int launch_head_lse_t(int nv, const T* E, int d, int V, float* part_m, float* part_s, const void* hn, int R, float alpha, const int* done,
                             hipStream_t s) {
  const size_t bytes = (size_t)nv * d * sizeof(T);
  P5_REQUIRE(R >= 1 && V >= 1 && d >= 1 && d % (sizeof(T) == 2 ? 256 : 128) == 0, "head_lse: d_model must be a multiple of 256 (bf16) / 128 (fp32)");
  P5_REQUIRE((nv == 128 || nv == 64 || nv == 32 || nv == 16) && bytes <= (nv == 16 ? 64 : 128) * 1024, "head_lse: nv rows of E must fit the kernel's LDS");
  const int nt = (V + nv - 1) / nv;
#define P5_HEAD(NV, KB) do { P5_PROF_TAG(sizeof(T) == 2 ? "bf16 NV=" #NV " LDSKB=" #KB : "fp32 NV=" #NV " LDSKB=" #KB); \
    P5_LAUNCH((p5_head_lse_kernel<T, NV, KB>), dim3(nt), dim3(256), 0, s, part_m, part_s, (const T*)hn, E, R, d, V, alpha, done); } while (0)
  if (nv == 128) P5_HEAD(128, 128);
  else if (nv == 64 && bytes <= 64 * 1024) P5_HEAD(64, 64);
  else if (nv == 64) P5_HEAD(64, 128);
  else if (nv == 32 && bytes <= 64 * 1024) P5_HEAD(32, 64);
  else if (nv == 32) P5_HEAD(32, 128);
  else P5_HEAD(16, 64);
#undef P5_HEAD
  return P5_KCHECK();
}
template <class T>
static int launch_head_lse(P5Engine* e, float* part_m, float* part_s, const void* hn, int R, const int* done, hipStream_t s) {
  const int d = e->c.d_model;
  return launch_head_lse_t<T>(head_nv(e), Wc<T>(e, e->off_E), d, e->c.vocab_size, part_m, part_s, hn, R, 1.0f / sqrtf((float)d), done, s);
}

// hn(T) = T5LayerNorm(x32): p5_rmsnorm_f32in_kernel holds a row of at most 2 x 64 x 8 columns per wave
template <class T>
static int launch_rmsnorm_f32in(void* y, const float* x, const float* w, int rows, int d, float eps, const int* done, hipStream_t s) {
  P5_REQUIRE(rows >= 1 && d >= 8 && d % 8 == 0 && d <= 1024, "rmsnorm_f32in: d must be a multiple of 8, <= 1024");
  P5_LAUNCH((p5_rmsnorm_f32in_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, (T*)y, x, w, rows, d, eps, done);
  return P5_KCHECK();
}

// single-token self-attention over the ancestry-indexed cache [max_len][R][2 * H * 64]; `step` holds cur_len (1 .. max_len) on the device
template <class T>
static int launch_dec_self_attn(void* out, const void* qkv, void* cache, const int* anc_odd, const int* anc_even, const float* rel_table,
                                const int* lut, int lut_half, int R, int H, const int* step, int max_len, const int* done, hipStream_t s) {
  P5_REQUIRE(R >= 1 && H >= 1 && max_len >= 1 && max_len <= P5_MAX_LEN && lut_half >= max_len - 1, "dec_self_attn: max_len <= P5_MAX_LEN, lut covers it");
  const dim3 grid((R * H + 3) / 4), block(256);
  if (max_len <= 64) {
    P5_PROF_TAG(sizeof(T) == 2 ? "bf16 NP=8" : "fp32 NP=8");
    P5_LAUNCH((p5_dec_self_attn2_kernel<T, 8>), grid, block, 0, s, (T*)out, (const T*)qkv, (T*)cache, anc_odd, anc_even, rel_table, lut, lut_half, R, H, step,
              max_len, done);
  } else {
    P5_PROF_TAG(sizeof(T) == 2 ? "bf16 NP=16" : "fp32 NP=16");
    P5_LAUNCH((p5_dec_self_attn2_kernel<T, P5_MAX_LEN / 8>), grid, block, 0, s, (T*)out, (const T*)qkv, (T*)cache, anc_odd, anc_even, rel_table, lut, lut_half,
              R, H, step, max_len, done);
  }
  return P5_KCHECK();
}

// LDS of the fused-q cross-attention: q image 2 KiB + scores 8.25 + probabilities 2 x 4.25 + stats + K/V chunk images 2 x 16 KiB + normalised
// rows + the head's Wq slice + reduction buffer
template <class T>
static bool cross_fuseq_fits(int d) {
  constexpr int EPS = SkT<T>::EPS;
  return sizeof(T) == 2 && d >= EPS && d % EPS == 0 && (d / EPS) * (2048 + 64 * 128) + 3072 + 19712 + 2 * 16384 <= 136 * 1024;
}
// single-token cross-attention of B x Kb beam rows (a.R = B * a.Kb): variant 3 = matrix-core kernel, 2 = scalar kernel; fuseq: the kernel
// normalises a.x and projects q itself (bf16, d_model within cross_fuseq_fits)
template <class T>
static int launch_dec_cross(const P5CrossArgs& a, int B, int variant, bool fuseq, hipStream_t s) {
  P5_REQUIRE(variant == 2 || variant == 3, "dec_cross_attn: variant 2 or 3");
  P5_REQUIRE(B >= 1 && a.H >= 1 && a.Kb >= 1 && a.L >= 1 && a.R == B * a.Kb && a.out && a.kv && a.mask, "dec_cross_attn: shape / null argument");
  P5_REQUIRE(a.ldkv >= 2 * a.H * 64 && a.ldkv % TT<T>::EPF == 0, "dec_cross_attn: ldkv >= 2 * inner, rows 16-byte aligned");
  const dim3 cgrid(B * ((a.Kb + 15) / 16), a.H), block(256);
  if (fuseq) {
    P5_REQUIRE(cross_fuseq_fits<T>(a.d) && a.x && a.ln && a.Wq, "dec_cross_attn: fused q needs bf16 and a d_model whose rows and Wq slice fit the LDS");
    if constexpr (sizeof(T) == 2) {
      if (variant == 3) { P5_PROF_TAG("bf16 fuseq"); P5_LAUNCH((p5_dec_cross_attn3_kernel<T, true, 136>), cgrid, block, 0, s, a); }
      else { P5_PROF_TAG("bf16 fuseq"); P5_LAUNCH((p5_dec_cross_attn2_kernel<T, true, 128>), cgrid, block, 0, s, a); }
    }
  } else {
    P5_REQUIRE(a.q != nullptr, "dec_cross_attn: q");
    P5_PROF_TAG(dtype_name<T>());
    if (variant == 3) P5_LAUNCH((p5_dec_cross_attn3_kernel<T, false, sizeof(T) == 2 ? 52 : 96>), cgrid, block, 0, s, a);
    else P5_LAUNCH((p5_dec_cross_attn2_kernel<T, false, sizeof(T) == 2 ? 48 : 80>), cgrid, block, 0, s, a);
  }
  return P5_KCHECK();
}

// the rows' best K2 trie children (score desc, child asc).  streaming: log-sum-exp from the head's per-tile partials, logits recomputed as dot
// products (p5_dec_score2_kernel); else from materialised logits [R, ldl] (p5_dec_score_kernel)
struct P5ScoreArgs {
  const float* part_m; const float* part_s; int ntiles; const void* hn; const void* E; int d; float alpha;      // streaming
  const float* logits; int ldl, V;                                                                              // materialised
  const int* node; const float* run_score; const int* child_off; const int* child_tok; const int* child_node;
  const uint32_t* excluded; int excl_words, Kb, max_c, K2;
  float* cand_scratch; float* top_score; int* top_c; int* n_top;
  const int* done;
};
template <class T>
static int launch_dec_score(bool streaming, int R, const P5ScoreArgs& a, hipStream_t s) {
  P5_REQUIRE(R >= 1 && a.Kb >= 1 && a.max_c >= 1 && a.K2 >= 1 && (a.excl_words >= 0) && (!a.excluded || a.excl_words > 0), "dec_score: shape");
  P5_REQUIRE(a.cand_scratch || a.max_c <= (streaming ? P5_POOL : P5_ROW_LDS_CAND), "dec_score: fan-outs beyond the LDS pool need cand_scratch [R, max_c]");
  if (streaming) {
    P5_REQUIRE(a.K2 <= P5_MAX_K2 || a.max_c <= 256, "dec_score: K2 <= P5_MAX_K2 when fan-outs above 256 take the radix select (its compacted list lives in LDS)");
    P5_REQUIRE(a.ntiles >= 1 && a.d >= 8 * TT<T>::EPF && a.d % (8 * TT<T>::EPF) == 0 && a.d <= 1024, "dec_score: d_model a multiple of 8 x 16 bytes, <= 1024");
    P5_LAUNCH((p5_dec_score2_kernel<T>), dim3(R), dim3(256), 0, s, a.top_score, a.top_c, a.n_top, a.cand_scratch, a.part_m, a.part_s, a.ntiles, (const T*)a.hn,
              (const T*)a.E, a.d, a.alpha, a.node, a.run_score, a.child_off, a.child_tok, a.child_node, a.excluded, a.excl_words, a.Kb, a.max_c, a.K2, a.done);
  } else {
    P5_REQUIRE(a.V >= 1 && a.ldl >= a.V && a.ldl % 4 == 0, "dec_score: ldl >= V, a multiple of 4");
    P5_LAUNCH(p5_dec_score_kernel, dim3(R), dim3(256), 0, s, a.cand_scratch, a.top_score, a.top_c, a.n_top, a.logits, a.ldl, a.V, a.node, a.run_score,
              a.child_off, a.child_tok, a.child_node, a.excluded, a.excl_words, a.Kb, a.max_c, a.K2, a.done);
  }
  return P5_KCHECK();
}

// `step`: device int holding cur_len (default: the beam state's counter flags[2]); head = false stops behind the final T5LayerNorm -- w.hn is
// what a caller that needs no full-vocabulary log-sum-exp reads (sampling, p5_sample.h)
template <class T>
static int decode_step2(P5Engine* e, GenWs& w, int B, int L, int K, int max_len, hipStream_t s, const int* step = nullptr, bool head = true) {
  const P5Config& c = e->c;
  const int d = c.d_model, in = e->inner, H = c.n_heads, F = c.d_ff, R = B * K;
  const int* done = w.st.flags + 4;
  if (!step) step = w.st.flags + 2;
  float* x = w.x32;       // holds E32[last token] of every row: written by the previous beam step (or the initial state)
  const int sk_resid = g_opt_dec_atomic ? P5_SK_ATOMIC : P5_SK_RESID;      // how the o / wo projections update the fp32 residual stream
  const bool fuseq = g_opt_dec_fuseq && cross_fuseq_fits<T>(d);
  for (int i = 0; i < c.n_dec_layers; ++i) {
    const LayerOff& lo = e->dec[i];
    // ---- self-attention: qkv = norm(x) Wqkv^T ; attention over the ancestry-indexed cache ; x += o Wo^T ----
    P5_TRY(skinny<T>(s, 1, x, d, e->P + lo.sa.ln, Wc<T>(e, lo.sa.q), d, w.qkv, 3 * in, R, 3 * in, d, P5_SK_STORE, 1.f, c.eps, done));
    P5_TRY(launch_dec_self_attn<T>(w.o, w.qkv, w.cache[i], (const int*)w.st.anc, (const int*)w.st.anc_next, (const float*)(e->P + e->off_dec_rel), e->lut_dec,
                                   e->lut_half, R, H, step, max_len, done, s));
    P5_TRY(skinny<T>(s, 0, w.o, in, nullptr, Wc<T>(e, lo.sa.o), in, x, d, R, d, in, sk_resid, 1.f, 0.f, done));
    // ---- cross-attention ----
    P5CrossArgs a;
    a.out = w.o; a.q = w.q; a.x = x; a.ln = e->P + lo.ca.ln; a.Wq = Wc<T>(e, lo.ca.q); a.kv = w.kv_cross[i]; a.mask = w.mask_copy;
    a.R = R; a.H = H; a.Kb = K; a.L = L; a.d = d; a.eps = c.eps; a.done = done; a.ldkv = w.ldkv;
    if (!fuseq) P5_TRY(skinny<T>(s, 1, x, d, e->P + lo.ca.ln, Wc<T>(e, lo.ca.q), d, w.q, in, R, in, d, P5_SK_STORE, 1.f, c.eps, done));
    P5_TRY(launch_dec_cross<T>(a, B, g_opt_dec_cross == 3 ? 3 : 2, fuseq, s));
    P5_TRY(skinny<T>(s, 0, w.o, in, nullptr, Wc<T>(e, lo.ca.o), in, x, d, R, d, in, sk_resid, 1.f, 0.f, done));
    // ---- feed-forward ----
    if (c.gated_gelu) {
      T* u = (T*)w.h + (size_t)R * F;
      P5_TRY(skinny<T>(s, 1, x, d, e->P + lo.ff_ln, Wc<T>(e, lo.wi), d, u, 2 * F, R, 2 * F, d, P5_SK_STORE, 1.f, c.eps, done));
      const size_t n = (size_t)R * F;
      P5_LAUNCH((p5_gated_gelu_fwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (T*)w.h, (const T*)u, R, F, no_drop());
      P5_TRY(P5_KCHECK());
    } else {
      P5_TRY(skinny<T>(s, 1, x, d, e->P + lo.ff_ln, Wc<T>(e, lo.wi), d, w.h, F, R, F, d, P5_SK_RELU, 1.f, c.eps, done));
    }
    P5_TRY(skinny<T>(s, 0, w.h, F, nullptr, Wc<T>(e, lo.wo), F, x, d, R, d, F, sk_resid, 1.f, 0.f, done));
  }
  // logits = (norm(x) * d^-0.5) E^T   (P5_T5.py:352-361)
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  P5_TRY(launch_rmsnorm_f32in<T>(w.hn, (const float*)x, (const float*)(e->P + e->off_dec_fln), R, d, c.eps, done, s));
  if (!head) return 0;
  const float alpha = 1.0f / sqrtf((float)d);
  if (head_nv(e) > 0) return launch_head_lse<T>(e, w.part_m, w.part_s, w.hn, R, done, s);
  return linear_fwd<T>(s, w.hn, d, Wc<T>(e, e->off_E), w.logits, Vp, R, c.vocab_size, d, P5_EPI_STORE, nullptr, 0, alpha, 1);
}

// ---- what every decode loop starts from (beam search and sampling): the encoder pass (or the encoder output handed in), the forced-prefix
// pass when one applies (*ff_out: the prefix taken, n = 0 for none) and the cross-attention K/V of every layer; `w` is laid out, K = rows per user ----
template <class T>
static int gen_prepare(P5Engine* e, GenWs& w, int B, int L, int K, int max_len, const int* roots, hipStream_t s, P5Forced* ff_out) {
  const P5Config& c = e->c;
  const int d = c.d_model, in = e->inner, R = B * K;
  e->B = B; e->Gt = 1; e->Bd = B; e->tgt_w = nullptr; e->L = L; e->T = 0; e->M = B * L; e->Md = 0; e->training = 0;
  if (e->enc_ext_next) {
    // the encoder output of the verification pass (fp32, same weights), rounded once to this engine's dtype: one encoder pass per batch
    // instead of two, and a draft that starts from the better numbers
    const size_t n = (size_t)B * L * d;
    if constexpr (sizeof(T) == 2) {
      P5_LAUNCH((p5_cast_kernel<T>), dim3((unsigned)((n / 8 + 255) / 256 > 2048 ? 2048 : (n / 8 + 255) / 256)), dim3(256), 0, s, (T*)e->enc_out, e->enc_ext_next, n);
      P5_TRY(P5_KCHECK());
    } else {
      hipMemcpyAsync(e->enc_out, e->enc_ext_next, n * 4, hipMemcpyDeviceToDevice, s);
    }
    e->enc_ext_next = nullptr;
  } else {
    P5_TRY(encoder_fwd<T>(e, s));
  }
  // forced-prefix fast-forward (p5_decode.h): the first F steps as one teacher-forced pass of the training-layout decoder over B x F rows
  P5Forced ff = e->ff_next;
  e->ff_next.n = 0;
  const int ffcap = g_opt_gen_ff ? (max_len - 2 < P5_FF_MAX ? max_len - 2 : P5_FF_MAX) : 0;
  if (ff.n > ffcap) ff.n = ffcap > 0 ? ffcap : 0;
  if (ff.n < 2 || roots != nullptr) ff.n = 0;          // (one forced step is what a decode step costs; per-user roots: not a shared prefix)
  const int F = ff.n;
  if (F > 0) {
    P5_LAUNCH(p5_ff_labels_kernel, dim3((B * F + 255) / 256), dim3(256), 0, s, w.ff_labels, ff, B);
    P5_TRY(P5_KCHECK());
    e->T = F; e->Md = B * F; e->labels = w.ff_labels; e->Vp = (c.vocab_size + 63) / 64 * 64;
    P5_TRY(decoder_fwd<T>(e, s));      // (also projects the encoder output to the cross-attention K/V of every layer: e->kv_all)
    P5_LAUNCH((p5_ce_fwd_kernel<T>), dim3(e->Md), dim3(256), 0, s, w.ff_nll, e->lse_tok, (const float*)e->logits, (const int64_t*)w.ff_labels, c.vocab_size, e->Vp);
    P5_TRY(P5_KCHECK());
    for (int i = 0; i < c.n_dec_layers; ++i) {
      w.kv_cross[i] = e->ds[i].kv_ca;                  // same [B*L, n_dec * 2 * inner] block layout as the decode step's own projection
      P5_LAUNCH((p5_ff_cache_kernel<T>), dim3(B * F), dim3(256), 0, s, (T*)w.cache[i], (const T*)e->ds[i].qkv, F, K, R, in);
      P5_TRY(P5_KCHECK());
    }
    e->T = 0; e->Md = 0; e->labels = nullptr;
  } else {     // K/V projections of every decoder layer in ONE GEMM over the contiguous weight block (build_layout)
    P5_TRY(linear_fwd<T>(s, e->enc_out, d, Wc<T>(e, e->dec[0].ca.k), w.kv_cross[0], w.ldkv, B * L, c.n_dec_layers * 2 * in, d));
  }
  *ff_out = ff;
  return 0;
}

// ---- the search as three calls (p5_decode_begin / p5_decode_step / p5_decode_finish); p5_generate strings them together ----
template <class T>
static int decode_begin_impl(P5Engine* e, int B, int L, int K, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                             const int* roots, const uint32_t* excluded, int excl_words, int max_c, char* ws, hipStream_t s) {
  const P5Config& c = e->c;
  const int R = B * K;
  GenCtx& g = e->gen;
  g.active = false;
  layout_gen(e, ws, B, L, K, max_len, max_c, excl_words, &g.w);
  GenWs& w = g.w;
  w.st.hist = e->gen_hist_next;       // (p5_generate_draft) one-shot
  e->gen_hist_next = nullptr;
  if (!excluded) excl_words = 0;
  P5Forced ff;
  P5_TRY(gen_prepare<T>(e, w, B, L, K, max_len, roots, s, &ff));
  const int F = ff.n;
  P5_LAUNCH(p5_beam_init_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, w.st, child_off, child_tok, child_node, roots, B, K, max_len,
            c.pad_id);
  P5_TRY(P5_KCHECK());
  if (F > 0) {
    P5_LAUNCH(p5_beam_forced_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, w.st, ff, (const float*)w.ff_nll, B, K, max_len, c.pad_id);
    P5_TRY(P5_KCHECK());
  }
  hipMemcpyAsync(w.mask_copy, e->mask, (size_t)B * L * 8, hipMemcpyDeviceToDevice, s);
  if (excl_words > 0) hipMemcpyAsync(w.excluded, excluded, (size_t)B * excl_words * 4, hipMemcpyDeviceToDevice, s);
  g.B = B; g.L = L; g.K = K; g.max_len = max_len; g.max_c = max_c; g.excl_words = excl_words; g.ws = ws;
  g.child_off = child_off; g.child_tok = child_tok; g.child_node = child_node; g.roots = roots;
  g.steps = F; g.steps0 = F;
  g.wide = gen_wide_run(K, w.st.hist);
  g.active = true;
  return 0;
}

template <class T>
static int decode_step_body(P5Engine* e, hipStream_t s) {
  const P5Config& c = e->c;
  GenCtx& g = e->gen;
  GenWs& w = g.w;
  const int d = c.d_model, B = g.B, L = g.L, K = g.K, R = B * K, max_len = g.max_len, max_c = g.max_c, excl_words = g.excl_words;
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  const uint32_t* excl = excl_words > 0 ? w.excluded : nullptr;
  const int* done = w.st.flags + 4;
  P5_TRY(decode_step2<T>(e, w, B, L, K, max_len, s));
  {
    const int nv = head_nv(e);
    P5ScoreArgs a;
    a.part_m = w.part_m; a.part_s = w.part_s; a.ntiles = nv > 0 ? (c.vocab_size + nv - 1) / nv : 0; a.hn = w.hn; a.E = Wc<T>(e, e->off_E); a.d = d;
    a.alpha = 1.0f / sqrtf((float)d); a.logits = w.logits; a.ldl = Vp; a.V = c.vocab_size;
    a.node = w.st.run_node; a.run_score = w.st.run_score; a.child_off = g.child_off; a.child_tok = g.child_tok; a.child_node = g.child_node;
    a.excluded = excl; a.excl_words = excl_words; a.Kb = K; a.max_c = max_c; a.K2 = 2 * K;
    a.cand_scratch = w.cand; a.top_score = w.row_top_score; a.top_c = w.row_top_c; a.n_top = w.n_cand; a.done = done;
    P5_TRY(launch_dec_score<T>(nv > 0, R, a, s));
  }
  P5_LAUNCH(p5_beam_step_kernel, dim3(B), dim3(256), 0, s, w.st, (const float*)w.row_top_score, (const int*)w.row_top_c,
            (const int*)w.n_cand, g.child_off, g.child_tok, g.child_node, max_c, K, max_len, c.eos_id, R);
  return P5_KCHECK();
}

// the wide step (p5_decode_wide.h): same decoder and head; scoring, selection and the scorer with their state in global memory
template <class T>
static int decode_step_wide(P5Engine* e, hipStream_t s) {
  const P5Config& c = e->c;
  GenCtx& g = e->gen;
  GenWs& w = g.w;
  const int d = c.d_model, B = g.B, L = g.L, K = g.K, R = B * K, max_len = g.max_len, max_c = g.max_c, excl_words = g.excl_words, C = w.wide_c;
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  const uint32_t* excl = excl_words > 0 ? w.excluded : nullptr;
  const int* done = w.st.flags + 4;
  P5_TRY(decode_step2<T>(e, w, B, L, K, max_len, s));
  if (head_nv(e) > 0) {
    const int nv = head_nv(e), nt = (c.vocab_size + nv - 1) / nv;
    P5_LAUNCH((p5_wide_score2_kernel<T>), dim3(R), dim3(256), 0, s, w.wide.row_key, w.wide.row_n, w.cand, (const float*)w.part_m,
              (const float*)w.part_s, nt, (const T*)w.hn, Wc<T>(e, e->off_E), d, 1.0f / sqrtf((float)d), (const int*)w.st.run_node,
              (const float*)w.st.run_score, g.child_off, g.child_tok, g.child_node, excl, excl_words, K, max_c, C, done);
  } else {
    P5_LAUNCH(p5_wide_score_kernel, dim3(R), dim3(256), 0, s, w.wide.row_key, w.wide.row_n, w.cand, (const float*)w.logits, Vp, c.vocab_size,
              (const int*)w.st.run_node, (const float*)w.st.run_score, g.child_off, g.child_tok, g.child_node, excl, excl_words, K, max_c, C, done);
  }
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_wide_select_kernel, dim3(B), dim3(256), 0, s, w.st, w.wide, g.child_off, g.child_tok, g.child_node, max_c, K, C, max_len, c.eos_id);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_wide_scorer_kernel, dim3(B), dim3(256), 0, s, w.st, w.wide, K, max_len, c.eos_id);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_wide_commit_kernel, dim3((K + P5_WIDE_COMMIT_BEAMS - 1) / P5_WIDE_COMMIT_BEAMS, B), dim3(256), 0, s, w.st, w.wide, K, max_len, R);
  return P5_KCHECK();
}

// One beam-search step: the whole decoder over R = B*K rows, the tied head, HF's candidate selection and bookkeeping.  Nothing
// is read back: HF's global stop test (utils.py:3055-3075) is taken on the device by the beam step, which raises flags[4]; a
// step enqueued after that returns at once in every kernel.  From the second step of a call on, the step is replayed from a
// hipGraph captured once per (shape, workspace, trie, option) key.
template <class T>
static int decode_step_impl(P5Engine* e, hipStream_t s) {
  GenCtx& g = e->gen;
  P5_REQUIRE(g.active, "p5_decode_step without p5_decode_begin");
  if (g.steps >= g.max_len - 1) return 0;          // no hypothesis can grow beyond max_len tokens
#ifndef P5_EMU
  static const bool use_graph = !(getenv("P5_NO_GRAPH") && atoi(getenv("P5_NO_GRAPH")));
  GraphKey key;
  memset(&key, 0, sizeof(key));
  key.B = g.B; key.L = g.L; key.K = g.K; key.max_len = g.max_len; key.max_c = g.max_c; key.excl_words = g.excl_words; key.ws = g.ws;
  key.trie = g.child_off; key.trie_tok = g.child_tok; key.trie_node = g.child_node; key.roots = g.roots;
  key.P = e->P; key.S = e->S; key.sz = (int)sizeof(T); key.hist = g.w.st.hist; key.wide = g.wide ? 1 : 0;
  key.fused = 4 * g_opt_dec_fuseq + 8 * g_opt_dec_nb + 4096 * g_opt_dec_kw + (g_opt_dec_cross << 20) +
              (g_opt_dec_head << 23) + (g_opt_dec_head_nv << 24) + ((g.steps0 > 0 ? 1 : 0) << 30) + (g_opt_dec_atomic << 29);     // (forced-prefix pass: the cross K/V live elsewhere)
  bool have_graph = use_graph && e->gen_graph_exec && memcmp(&key, &e->gen_graph_key, sizeof(key)) == 0;
  if (use_graph && !have_graph && g.steps > g.steps0 && !e->gen_graph_failed) {
    // (never during the very first step: the first launch of a kernel loads its code object, which is not allowed
    // while a stream is capturing)
    if (e->gen_graph_exec) { hipGraphExecDestroy(e->gen_graph_exec); e->gen_graph_exec = nullptr; }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
      const int rc = g.wide ? decode_step_wide<T>(e, s) : decode_step_body<T>(e, s);
      const hipError_t ec = hipStreamEndCapture(s, &graph);
      if (rc == 0 && ec == hipSuccess && graph && hipGraphInstantiate(&e->gen_graph_exec, graph, nullptr, nullptr, 0) == hipSuccess) {
        e->gen_graph_key = key;
        have_graph = true;
      } else {
        e->gen_graph_exec = nullptr;
      }
      if (graph) hipGraphDestroy(graph);
    }
    (void)hipGetLastError();
    if (!have_graph) e->gen_graph_failed = true;
  }
  if (have_graph) {
    if (hipGraphLaunch(e->gen_graph_exec, s) != hipSuccess) return fail("hipGraphLaunch failed");
    g.steps++;
    return 0;
  }
#endif
  P5_TRY(g.wide ? decode_step_wide<T>(e, s) : decode_step_body<T>(e, s));
  g.steps++;
  return 0;
}

static int decode_finish_impl(P5Engine* e, int* out_seq, float* out_score, int* out_len, hipStream_t s) {
  GenCtx& g = e->gen;
  P5_REQUIRE(g.active, "p5_decode_finish without p5_decode_begin");
  const int R = g.B * g.K;
  P5_LAUNCH(p5_beam_finalize_kernel, dim3((R * g.max_len + 255) / 256), dim3(256), 0, s, out_seq, out_score, out_len, g.w.st, R, g.max_len);
  P5_TRY(P5_KCHECK());
  g.active = false;
  return 0;
}

// ---- trie-constrained sampling (p5_sample.h): S independent draws per user, R = B * S decode rows ----
// The workspace holds what the decoder of the step reads and writes and the rows' state: no logits, no head partials, no candidate lists.
static int64_t layout_sample(P5Engine* e, char* base, int B, int L, int S, int max_len, GenWs* g, P5SampleState* ps) {
  const P5Config& c = e->c;
  const size_t sz = c.dtype == 1 ? 2 : 4;
  const int d = c.d_model, in = e->inner, F = c.d_ff;
  const size_t R = (size_t)B * S;
  const int ffcap = g_opt_gen_ff ? (max_len - 2 < P5_FF_MAX ? (max_len - 2 > 0 ? max_len - 2 : 0) : P5_FF_MAX) : 0;
  const int64_t enc_bytes = layout_ws(e, base, B, L, ffcap, false);
  Bump b{base, (size_t)enc_bytes};
  GenWs tmp;
  GenWs& w = g ? *g : tmp;
  memset(&w, 0, sizeof(w));
  w.ff_labels = (int64_t*)b.take((size_t)B * (ffcap > 0 ? ffcap : 1) * 8);
  w.ff_nll = (float*)b.take((size_t)B * (ffcap > 0 ? ffcap : 1) * 4);
  {
    char* kv_all = (char*)b.take((size_t)B * L * c.n_dec_layers * 2 * in * sz);
    w.ldkv = c.n_dec_layers * 2 * in;
    for (int i = 0; i < c.n_dec_layers; ++i) {
      w.kv_cross[i] = base ? (void*)(kv_all + (size_t)i * 2 * in * sz) : nullptr;
      w.cache[i] = b.take((size_t)max_len * R * 2 * in * sz);
    }
  }
  w.qkv = b.take(R * 3 * in * sz); w.q = b.take(R * in * sz); w.o = b.take(R * in * sz);
  w.h = b.take(R * (c.gated_gelu ? 3 : 1) * F * sz); w.hn = b.take(R * d * sz);
  w.x32 = (float*)b.take(R * d * 4);
  P5SampleState st;
  memset(&st, 0, sizeof(st));
  st.seq = (int*)b.take(R * max_len * 4);
  st.tok_lp = (float*)b.take(R * max_len * 4);
  st.anc = (int*)b.take(R * max_len * 4);
  st.sum_lp = (float*)b.take(R * 4); st.node = (int*)b.take(R * 4); st.len = (int*)b.take(R * 4);
  st.steps = (int*)b.take((size_t)(max_len + 1) * 4);
  st.flags = (int*)b.take(64);
  st.x32 = w.x32;
  st.E32 = e->P ? e->P + e->off_E : nullptr;
  st.d = d;
  // the decoder of the step finds the ancestry (one table: rows never change places) and its done flag where the beam state keeps them
  w.st.anc = st.anc; w.st.anc_next = st.anc; w.st.flags = st.flags;
  if (ps) *ps = st;
  return (int64_t)((b.off + 255) & ~(size_t)255);
}

template <class T>
static int sample_items_impl(P5Engine* e, int B, int L, int S, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                             const uint32_t* excluded, int excl_words, int max_c, uint32_t seed, const uint32_t* stream_ids, uint32_t draw_base,
                             float tau, int* out_seq, float* out_logprob, float* out_tok_logprob, int* out_len, char* ws, hipStream_t s,
                             bool trunc = false, int top_k = 0, float top_p = 1.f) {
  const P5Config& c = e->c;
  const int d = c.d_model, R = B * S;
  GenWs w;
  P5SampleState st;
  // (truncated: the [R, max_c] fp32 scratch of p5_trunc_sample_step_kernel lies behind the sampler's workspace)
  float* zs = (float*)(ws + layout_sample(e, ws, B, L, S, max_len, &w, &st));
  e->gen.active = false;              // (a search begun on this engine shared the encoder buffers: it cannot be continued)
  e->gen_hist_next = nullptr;
  if (!excluded) excl_words = 0;
  w.mask_copy = (int64_t*)e->mask;    // plain launches: the caller's arrays are read in place
  P5Forced ff;
  P5_TRY(gen_prepare<T>(e, w, B, L, S, max_len, nullptr, s, &ff));
  const int F = ff.n;
  P5_LAUNCH(p5_sample_init_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, st, ff, child_off, child_tok, child_node, B, S, max_len, c.pad_id,
            c.pad_id);
  P5_TRY(P5_KCHECK());
  P5SampleArgs a;
  a.hn = w.hn; a.E = Wc<T>(e, e->off_E); a.d = d; a.alpha = 1.0f / sqrtf((float)d); a.tau = tau;
  a.child_off = child_off; a.child_tok = child_tok; a.child_node = child_node;
  a.excluded = excl_words > 0 ? excluded : nullptr; a.excl_words = excl_words;
  a.S = S; a.R = R; a.max_c = max_c; a.max_len = max_len; a.eos_id = c.eos_id;
  a.seed = seed; a.stream_ids = stream_ids; a.draw_base = draw_base;
  // no early stop and nothing read back: every draw runs to its leaf, finished rows are no-ops of the selection
  for (int cur_len = F + 1; cur_len < max_len; ++cur_len) {
    P5_TRY(decode_step2<T>(e, w, B, L, S, max_len, s, (const int*)(st.steps + cur_len), false));
    a.cur_len = cur_len;
    if (trunc) P5_LAUNCH((p5_trunc_sample_step_kernel<T>), dim3(R), dim3(256), 0, s, st, a, zs, top_k, top_p);
    else P5_LAUNCH((p5_sample_step_kernel<T>), dim3(R), dim3(256), 0, s, st, a);
    P5_TRY(P5_KCHECK());
  }
  P5_LAUNCH(p5_sample_finish_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, out_seq, out_logprob, out_tok_logprob, out_len, st, R, max_len);
  return P5_KCHECK();
}

// ---- stochastic beam search (p5_sbs.h): S slates of K distinct items per user, R = B * S * K decode rows ----
// The workspace is layout_sample's for S * K rows per user plus the rows' second sequence / log-probability / ancestry buffers (rows change
// places) and the step's scratch, which DOES follow the fan-out: two [R, max_c] fp32 rows (token log-probabilities, perturbed values) and
// the [R, min(max_c, K)] key lists.
static int64_t layout_sbs(P5Engine* e, char* base, int B, int L, int S, int K, int max_len, int max_c, GenWs* g, P5SbsState* ps) {
  const P5Config& c = e->c;
  const size_t sz = c.dtype == 1 ? 2 : 4;
  const int d = c.d_model, in = e->inner, F = c.d_ff;
  const size_t R = (size_t)B * S * K;
  const size_t C = (size_t)(max_c < K ? max_c : K);
  const int ffcap = g_opt_gen_ff ? (max_len - 2 < P5_FF_MAX ? (max_len - 2 > 0 ? max_len - 2 : 0) : P5_FF_MAX) : 0;
  const int64_t enc_bytes = layout_ws(e, base, B, L, ffcap, false);
  Bump b{base, (size_t)enc_bytes};
  GenWs tmp;
  GenWs& w = g ? *g : tmp;
  memset(&w, 0, sizeof(w));
  w.ff_labels = (int64_t*)b.take((size_t)B * (ffcap > 0 ? ffcap : 1) * 8);
  w.ff_nll = (float*)b.take((size_t)B * (ffcap > 0 ? ffcap : 1) * 4);
  {
    char* kv_all = (char*)b.take((size_t)B * L * c.n_dec_layers * 2 * in * sz);
    w.ldkv = c.n_dec_layers * 2 * in;
    for (int i = 0; i < c.n_dec_layers; ++i) {
      w.kv_cross[i] = base ? (void*)(kv_all + (size_t)i * 2 * in * sz) : nullptr;
      w.cache[i] = b.take((size_t)max_len * R * 2 * in * sz);
    }
  }
  w.qkv = b.take(R * 3 * in * sz); w.q = b.take(R * in * sz); w.o = b.take(R * in * sz);
  w.h = b.take(R * (c.gated_gelu ? 3 : 1) * F * sz); w.hn = b.take(R * d * sz);
  w.x32 = (float*)b.take(R * d * 4);
  P5SbsState st;
  memset(&st, 0, sizeof(st));
  st.seq = (int*)b.take(R * max_len * 4); st.seq_next = (int*)b.take(R * max_len * 4);
  st.tok_lp = (float*)b.take(R * max_len * 4); st.tok_lp_next = (float*)b.take(R * max_len * 4);
  st.anc = (int*)b.take(R * max_len * 4); st.anc_next = (int*)b.take(R * max_len * 4);
  st.phi = (float*)b.take(R * 4); st.G = (float*)b.take(R * 4);
  st.node = (int*)b.take(R * 4); st.edge = (int*)b.take(R * 4); st.len = (int*)b.take(R * 4);
  st.steps = (int*)b.take((size_t)(max_len + 1) * 4);
  st.flags = (int*)b.take(64);
  st.lp = (float*)b.take(R * max_c * 4); st.gt = (float*)b.take(R * max_c * 4);
  st.row_key = (unsigned long long*)b.take(R * C * 8); st.row_n = (int*)b.take(R * 4);
  st.sel_parent = (int*)b.take(R * 4); st.sel_tok = (int*)b.take(R * 4); st.sel_node = (int*)b.take(R * 4);
  st.sel_edge = (int*)b.take(R * 4); st.sel_len = (int*)b.take(R * 4);
  st.sel_phi = (float*)b.take(R * 4); st.sel_G = (float*)b.take(R * 4); st.sel_lp = (float*)b.take(R * 4);
  st.x32 = w.x32;
  st.E32 = e->P ? e->P + e->off_E : nullptr;
  st.d = d;
  // the decoder of the step finds the two ancestry tables and its done flag where the beam state keeps them
  w.st.anc = st.anc; w.st.anc_next = st.anc_next; w.st.flags = st.flags;
  if (ps) *ps = st;
  return (int64_t)((b.off + 255) & ~(size_t)255);
}

template <class T>
static int sbs_impl(P5Engine* e, int B, int L, int S, int K, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                    const uint32_t* excluded, int excl_words, int max_c, uint32_t seed, const uint32_t* stream_ids, uint32_t slate_base, float tau,
                    int* out_seq, float* out_logprob, float* out_perturbed, float* out_tok_logprob, int* out_len, char* ws, hipStream_t s) {
  const P5Config& c = e->c;
  const int d = c.d_model, R = B * S * K;
  GenWs w;
  P5SbsState st;
  layout_sbs(e, ws, B, L, S, K, max_len, max_c, &w, &st);
  e->gen.active = false;              // (a search begun on this engine shared the encoder buffers: it cannot be continued)
  e->gen_hist_next = nullptr;
  if (!excluded) excl_words = 0;
  w.mask_copy = (int64_t*)e->mask;    // plain launches: the caller's arrays are read in place
  P5Forced ff;
  P5_TRY(gen_prepare<T>(e, w, B, L, S * K, max_len, nullptr, s, &ff));
  const int F = ff.n;
  P5_LAUNCH(p5_sbs_init_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, st, ff, child_off, child_tok, child_node, B, S, K, max_len, c.pad_id,
            c.pad_id);
  P5_TRY(P5_KCHECK());
  P5SbsArgs a;
  a.hn = w.hn; a.E = Wc<T>(e, e->off_E); a.d = d; a.alpha = 1.0f / sqrtf((float)d); a.tau = tau;
  a.child_off = child_off; a.child_tok = child_tok; a.child_node = child_node;
  a.excluded = excl_words > 0 ? excluded : nullptr; a.excl_words = excl_words;
  a.S = S; a.K = K; a.R = R; a.max_c = max_c; a.C = max_c < K ? max_c : K; a.max_len = max_len; a.eos_id = c.eos_id; a.pad_id = c.pad_id;
  a.start_id = c.pad_id; a.F = F;
  a.seed = seed; a.stream_ids = stream_ids; a.slate_base = slate_base;
  // no early stop and nothing read back: finished beams are carried, dead slots run the decoder on the pad embedding
  for (int cur_len = F + 1; cur_len < max_len; ++cur_len) {
    P5_TRY(decode_step2<T>(e, w, B, L, S * K, max_len, s, (const int*)(st.steps + cur_len), false));
    a.cur_len = cur_len;
    P5_LAUNCH((p5_sbs_row_kernel<T>), dim3(R), dim3(256), 0, s, st, a);
    P5_TRY(P5_KCHECK());
    P5_LAUNCH(p5_sbs_select_kernel, dim3(B * S), dim3(256), 0, s, st, a);
    P5_TRY(P5_KCHECK());
    const bool odd = (cur_len & 1) != 0;       // the decoder of this step read `anc` (odd cur_len) or `anc_next` (even)
    P5_LAUNCH(p5_sbs_commit_kernel, dim3((R + P5_SBS_COMMIT_ROWS - 1) / P5_SBS_COMMIT_ROWS), dim3(256), 0, s, st, a,
              (const int*)(odd ? st.anc : st.anc_next), odd ? st.anc_next : st.anc);
    P5_TRY(P5_KCHECK());
    { int* t = st.seq; st.seq = st.seq_next; st.seq_next = t; }
    { float* t = st.tok_lp; st.tok_lp = st.tok_lp_next; st.tok_lp_next = t; }
  }
  P5_LAUNCH(p5_sbs_finish_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, out_seq, out_logprob, out_perturbed, out_tok_logprob, out_len, st, R,
            max_len);
  return P5_KCHECK();
}

// ---- verified generation (p5_verify.h): plan -> encode -> run on an fp32 engine bound to the same master parameters ----
struct VerifyWs {
  P5VerifyPlan pl;
  int64_t* ids; int *node_flat, *depth_flat;
  void *x, *y, *n, *qkv, *q, *o, *h, *hn, *kv_all;
  float *lse, *part_m, *part_s, *logits, *cand, *row_top_score, *zeros;
  int *row_top_c, *n_top, *vrow_a, *vrow_b, *missing;
  P5BeamState st;
};
struct VerifyCtx {
  bool begun = false, encoded = false, planned = false;
  P5Forced ff = {0, {0}, {0}};     // forced prefix of the search being verified (p5_generate_set_forced_prefix on this engine before p5_verify_begin)
  VerifyWs w;
  int B = 0, L = 0, K = 0, Kw = 0, max_len = 0, max_c = 0, excl_words = 0;
  const int *child_off = nullptr, *child_tok = nullptr, *child_node = nullptr, *roots = nullptr;
  char* ws = nullptr;
};
static int verify_cap(int Kw, int max_len) { return (Kw * (max_len - 1) + 1 + 15) / 16 * 16; }

static int64_t layout_verify(P5Engine* e, char* base, int B, int L, int K, int Kw, int max_len, int max_c, int excl_words, VerifyWs* out) {
  const P5Config& c = e->c;
  const size_t sz = c.dtype == 1 ? 2 : 4;
  const int d = c.d_model, in = e->inner, F = c.d_ff, H = c.n_heads;
  const int cap = verify_cap(Kw, max_len);
  const size_t rows = (size_t)B * cap, R = (size_t)B * K;
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  const int64_t enc_bytes = layout_ws(e, base, B, L, 0, false);
  Bump b{base, (size_t)enc_bytes};
  VerifyWs tmp;
  VerifyWs& w = out ? *out : tmp;
  w.kv_all = b.take((size_t)B * L * c.n_dec_layers * 2 * in * sz);
  P5VerifyPlan& pl = w.pl;
  pl.cap = cap; pl.max_len = max_len;
  pl.hdr = (int*)b.take(64);
  pl.n_rows = (int*)b.take((size_t)B * 4);
  pl.row_tok = (int*)b.take(rows * 4); pl.row_parent = (int*)b.take(rows * 4); pl.row_depth = (int*)b.take(rows * 4); pl.row_node = (int*)b.take(rows * 4);
  pl.first = (int*)b.take((size_t)B * (max_len + 1) * 4);
  pl.anc = (int*)b.take(rows * max_len * 4);
  w.ids = (int64_t*)b.take(rows * 8); w.node_flat = (int*)b.take(rows * 4); w.depth_flat = (int*)b.take(rows * 4);
  w.x = b.take(rows * d * sz); w.y = b.take(rows * d * sz); w.n = b.take(rows * d * sz);
  w.qkv = b.take(rows * 3 * in * sz); w.q = b.take(rows * in * sz); w.o = b.take(rows * in * sz);
  w.h = b.take(rows * (c.gated_gelu ? 3 : 1) * F * sz); w.hn = b.take(rows * d * sz);
  w.lse = (float*)b.take((size_t)B * H * cap * 4);
  const int nv = head_nv(e);
  const size_t nt = nv > 0 ? (size_t)(c.vocab_size + nv - 1) / nv : 1;
  w.part_m = (float*)b.take(rows * nt * 4); w.part_s = (float*)b.take(rows * nt * 4);
  w.logits = (float*)b.take(rows * Vp * 4);        // (materialised logits: toy widths, and the split-product head -- one throughput GEMM)
  w.cand = (float*)b.take(rows * (size_t)max_c * 4);
  w.row_top_score = (float*)b.take(rows * (size_t)(2 * K) * 4); w.row_top_c = (int*)b.take(rows * (size_t)(2 * K) * 4);
  w.n_top = (int*)b.take(rows * 4); w.zeros = (float*)b.take(rows * 4);
  w.vrow_a = (int*)b.take(R * 4); w.vrow_b = (int*)b.take(R * 4); w.missing = (int*)b.take((size_t)B * 4);
  P5BeamState& st = w.st;
  st.run_seq = (int*)b.take(R * max_len * 4); st.run_seq_next = (int*)b.take(R * max_len * 4);
  st.fin_seq = (int*)b.take(R * max_len * 4); st.fin_seq_next = (int*)b.take(R * max_len * 4);
  st.anc = (int*)b.take(R * max_len * 4); st.anc_next = (int*)b.take(R * max_len * 4);
  st.run_score = (float*)b.take(R * 4); st.run_node = (int*)b.take(R * 4);
  st.fin_score = (float*)b.take(R * 4); st.fin_flag = (int*)b.take(R * 4); st.fin_len = (int*)b.take(R * 4);
  st.unsat = (int*)b.take((size_t)B * 4);
  st.last_tok = (int64_t*)b.take(R * 8);
  st.flags = (int*)b.take(64);
  st.x32 = nullptr; st.E32 = nullptr; st.d = d; st.hist = nullptr;
  (void)excl_words;
  return (int64_t)((b.off + 255) & ~(size_t)255);
}

static int verify_begin_impl(P5Engine* e, int B, int L, int K, int Kw, int max_len, const int* child_off, const int* child_tok,
                             const int* child_node, const int* roots, int max_c, int excl_words, char* ws) {
  if (!e->ver) e->ver = new VerifyCtx();
  VerifyCtx& v = *e->ver;
  v.begun = v.encoded = v.planned = false;
  layout_verify(e, ws, B, L, K, Kw, max_len, max_c, excl_words, &v.w);
  v.B = B; v.L = L; v.K = K; v.Kw = Kw; v.max_len = max_len; v.max_c = max_c; v.excl_words = excl_words; v.ws = ws;
  v.child_off = child_off; v.child_tok = child_tok; v.child_node = child_node; v.roots = roots;
  v.ff = e->ff_next;
  e->ff_next.n = 0;
  if (v.ff.n < 2 || roots != nullptr || !g_opt_gen_ff) v.ff.n = 0;
  if (v.ff.n > max_len - 2) v.ff.n = max_len - 2 > 0 ? max_len - 2 : 0;
  v.begun = true;
  return 0;
}
static int verify_plan_impl(P5Engine* e, const int* hist, hipStream_t s) {
  VerifyCtx& v = *e->ver;
  hipMemsetAsync(v.w.pl.hdr, 0, 64, s);
  P5_LAUNCH(p5_verify_plan_kernel, dim3(v.B), dim3(256), 0, s, v.w.pl, hist, v.child_off, v.child_tok, v.child_node, v.roots, v.B, v.Kw, e->c.pad_id);
  P5_TRY(P5_KCHECK());
  v.planned = true;
  return 0;
}

// the fp32 encoder pass + the cross-attention K/V of every decoder layer (one GEMM over the contiguous weight block); independent of the plan
template <class T>
static int verify_encode_impl(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, hipStream_t s) {
  VerifyCtx& v = *e->ver;
  const P5Config& c = e->c;
  SplitScope split(sizeof(T) == 4 ? g_opt_verify_split : 0);
  layout_ws(e, v.ws, v.B, v.L, 0, false);          // (the encoder's buffers: the head of the verification workspace)
  e->B = v.B; e->Gt = 1; e->Bd = v.B; e->tgt_w = nullptr; e->L = v.L; e->T = 0; e->M = v.B * v.L; e->Md = 0; e->training = 0;
  e->ids = input_ids; e->ww = whole_word_ids; e->mask = attention_mask; e->labels = nullptr;
  P5_TRY(encoder_fwd<T>(e, s));
  P5_TRY(linear_fwd<T>(s, e->enc_out, c.d_model, Wc<T>(e, e->dec[0].ca.k), v.w.kv_all, c.n_dec_layers * 2 * e->inner, v.B * v.L, c.n_dec_layers * 2 * e->inner, c.d_model));
  v.encoded = true;
  return 0;
}

// The teacher-forced decoder pass over a forest of prefixes, shared by verified generation (rows = what a draft kept alive) and exhaustive
// ranking (rows = the trie, p5_rank.h): rows are laid out [nchunk][B][CQ] -- self-attention sees B * CQ * nchunk single positions with
// ancestor lists (`tree_attn` launches the kernel that knows them), cross-attention sees, per chunk, B sequences of CQ <= 512 queries
// against the user's encoder keys.  Ends with the final T5LayerNorm of every row in w.hn.
struct RowsPassBufs {
  const int64_t* ids;       // decoder input token of every row
  void *x, *y, *n, *qkv, *q, *o, *h, *hn;
  float* lse;               // [B, H, CQ] scratch of the cross-attention kernels
  const void* kv_all;       // cross-attention K/V of every decoder layer, [B * L, n_dec_layers * 2 * inner]
};
template <class T, class TreeAttn>
static int decoder_rows_pass(P5Engine* e, const RowsPassBufs& w, int B, int CQ, int nchunk, int L, TreeAttn tree_attn, hipStream_t s) {
  const P5Config& c = e->c;
  const int d = c.d_model, in = e->inner, H = c.n_heads, F = c.d_ff;
  const int rows = B * CQ * nchunk, ldkv = c.n_dec_layers * 2 * in;
  void* x = w.x; void* y = w.y;
  P5_LAUNCH((p5_embed_fwd_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, (T*)x, Wc<T>(e, e->off_E), (const T*)nullptr, (const int64_t*)w.ids,
            (const int64_t*)nullptr, rows, d, no_drop(), (float*)nullptr);
  P5_TRY(P5_KCHECK());
  for (int i = 0; i < c.n_dec_layers; ++i) {
    const LayerOff& lo = e->dec[i];
    // self-attention over the row's own prefix
    P5_TRY(rmsnorm_fwd<T>(s, w.n, nullptr, x, e->P + lo.sa.ln, rows, d, c.eps, no_drop()));
    P5_TRY(linear_fwd<T>(s, w.n, d, Wc<T>(e, lo.sa.q), w.qkv, 3 * in, rows, 3 * in, d));
    P5_TRY(tree_attn((T*)w.o, (const T*)w.qkv));
    P5_TRY(linear_fwd<T>(s, w.o, in, Wc<T>(e, lo.sa.o), y, d, rows, d, in, P5_EPI_RESID_DROP, x, d));
    std::swap(x, y);
    // cross-attention: a user's CQ rows of a chunk are CQ queries against the user's encoder keys (zero position bias, padding mask)
    P5_TRY(rmsnorm_fwd<T>(s, w.n, nullptr, x, e->P + lo.ca.ln, rows, d, c.eps, no_drop()));
    P5_TRY(linear_fwd<T>(s, w.n, d, Wc<T>(e, lo.ca.q), w.q, in, rows, in, d));
    for (int ch = 0; ch < nchunk; ++ch) {
      P5AttnArgs a;
      memset(&a, 0, sizeof(a));
      a.Q = (const T*)w.q + (size_t)ch * B * CQ * in; a.K = (const T*)w.kv_all + (size_t)i * 2 * in; a.V = (const T*)w.kv_all + (size_t)i * 2 * in + in;
      a.O = (T*)w.o + (size_t)ch * B * CQ * in; a.lse = w.lse;
      a.rel_table = nullptr; a.bucket_lut = nullptr; a.kmask = e->mask;
      a.B = B; a.H = H; a.Lq = CQ; a.Lk = L; a.ldq = in; a.ldk = a.ldv = ldkv; a.ldo = in; a.causal = 0;
      a.drop = no_drop();
      P5_TRY(launch_attn_fwd<T>(a, s));
    }
    P5_TRY(linear_fwd<T>(s, w.o, in, Wc<T>(e, lo.ca.o), y, d, rows, d, in, P5_EPI_RESID_DROP, x, d));
    std::swap(x, y);
    // feed-forward
    P5_TRY(rmsnorm_fwd<T>(s, w.n, nullptr, x, e->P + lo.ff_ln, rows, d, c.eps, no_drop()));
    if (c.gated_gelu) {
      T* u = (T*)w.h + (size_t)rows * F;
      P5_TRY(linear_fwd<T>(s, w.n, d, Wc<T>(e, lo.wi), u, 2 * F, rows, 2 * F, d));
      const size_t n = (size_t)rows * F;
      P5_LAUNCH((p5_gated_gelu_fwd_kernel<T>), dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, s, (T*)w.h, (const T*)u, rows, F, no_drop());
      P5_TRY(P5_KCHECK());
    } else {
      P5_TRY(linear_fwd<T>(s, w.n, d, Wc<T>(e, lo.wi), w.h, F, rows, F, d, P5_EPI_RELU_DROP));
    }
    P5_TRY(linear_fwd<T>(s, w.h, F, Wc<T>(e, lo.wo), y, d, rows, d, F, P5_EPI_RESID_DROP, x, d));
    std::swap(x, y);
  }
  return rmsnorm_fwd<T>(s, w.hn, nullptr, x, e->P + e->off_dec_fln, rows, d, c.eps, no_drop());
}

// the three launches of p5_tree_attn_row with their operands as arguments (p5_op_tree_attn runs them too)
template <class T>
static int verify_tree_attn(T* o, const T* qkv, const P5VerifyPlan& pl, const int* depth_flat, const float* rel_table, const int* lut, int lut_half, int B, int PU,
                            int H, hipStream_t s) {
  P5_PROF_TAG(sizeof(T) == 2 ? "bf16" : "fp32");
  P5_LAUNCH((p5_tree_attn_kernel<T>), dim3((B * PU * H + 3) / 4), dim3(256), 0, s, o, qkv, pl, depth_flat, rel_table, lut, lut_half, B, PU, H);
  return P5_KCHECK();
}
template <class T>
static int rank_tree_attn(T* o, const T* qkv, const P5RankPlan& pl, const float* rel_table, const int* lut, int lut_half, int H, hipStream_t s) {
  const long long R = (long long)pl.B * pl.CQ * pl.nchunk;
  P5_PROF_TAG(sizeof(T) == 2 ? "bf16" : "fp32");
  P5_LAUNCH((p5_rank_tree_attn_kernel<T>), dim3((unsigned)((R * H + 3) / 4)), dim3(256), 0, s, o, qkv, pl, rel_table, lut, lut_half, H);
  return P5_KCHECK();
}
template <class T>
static int cand_tree_attn(T* o, const T* qkv, const P5CandPlan& pl, const float* rel_table, const int* lut, int lut_half, int H, hipStream_t s) {
  const long long R = (long long)pl.g.B * pl.g.CQ * pl.g.nchunk;
  P5_PROF_TAG(sizeof(T) == 2 ? "bf16" : "fp32");
  P5_LAUNCH((p5_cand_tree_attn_kernel<T>), dim3((unsigned)((R * H + 3) / 4)), dim3(256), 0, s, o, qkv, pl, rel_table, lut, lut_half, H);
  return P5_KCHECK();
}
// SCORE + REPLAY.  PU: rows per user of this pass (>= the plan's largest row count, a multiple of 16, <= cap): the decoder runs on
// [B x PU] rows (decoder_rows_pass, one chunk).
template <class T>
static int verify_run_impl(P5Engine* e, int PU, const uint32_t* excluded, int* out_seq, float* out_score, int* out_len, int* out_missing, hipStream_t s) {
  VerifyCtx& v = *e->ver;
  VerifyWs& w = v.w;
  const P5Config& c = e->c;
  SplitScope split(sizeof(T) == 4 ? g_opt_verify_split : 0);
  const int d = c.d_model, H = c.n_heads, B = v.B, K = v.K, max_len = v.max_len;
  const int rows = B * PU, R = B * K;
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  P5_LAUNCH(p5_verify_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, w.ids, w.node_flat, w.depth_flat, w.pl, B, PU, c.pad_id);
  P5_TRY(P5_KCHECK());
  RowsPassBufs pb;
  pb.ids = w.ids; pb.x = w.x; pb.y = w.y; pb.n = w.n; pb.qkv = w.qkv; pb.q = w.q; pb.o = w.o; pb.h = w.h; pb.hn = w.hn; pb.lse = w.lse; pb.kv_all = w.kv_all;
  auto tree_attn = [&](T* o, const T* qkv) -> int {
    return verify_tree_attn<T>(o, qkv, w.pl, (const int*)w.depth_flat, (const float*)(e->P + e->off_dec_rel), e->lut_dec, e->lut_half, B, PU, H, s);
  };
  P5_TRY((decoder_rows_pass<T>(e, pb, B, PU, 1, v.L, tree_attn, s)));
  // log-sum-exp over the full vocabulary per row + the log-probabilities of the row's trie children (running score 0)
  hipMemsetAsync(w.zeros, 0, (size_t)rows * 4, s);
  const float alpha = 1.0f / sqrtf((float)d);
  const uint32_t* excl = v.excl_words > 0 ? excluded : nullptr;
  // (with split products the tied head is one throughput GEMM into materialised logits: the streaming head multiplies on exact-fp32 MFMAs)
  if (head_nv(e) > 0 && !(sizeof(T) == 4 && g_opt_verify_split)) {
    P5_TRY(launch_head_lse<T>(e, w.part_m, w.part_s, w.hn, rows, nullptr, s));
  } else {
    P5_TRY(linear_fwd<T>(s, w.hn, d, Wc<T>(e, e->off_E), w.logits, Vp, rows, c.vocab_size, d, P5_EPI_STORE, nullptr, 0, alpha, 1));
  }
  {
    const bool streaming = head_nv(e) > 0 && !(sizeof(T) == 4 && g_opt_verify_split);
    const int nv = head_nv(e);
    P5ScoreArgs a;
    a.part_m = w.part_m; a.part_s = w.part_s; a.ntiles = nv > 0 ? (c.vocab_size + nv - 1) / nv : 0; a.hn = w.hn; a.E = Wc<T>(e, e->off_E); a.d = d; a.alpha = alpha;
    a.logits = w.logits; a.ldl = Vp; a.V = c.vocab_size;
    a.node = w.node_flat; a.run_score = w.zeros; a.child_off = v.child_off; a.child_tok = v.child_tok; a.child_node = v.child_node;
    a.excluded = excl; a.excl_words = v.excl_words; a.Kb = PU; a.max_c = v.max_c; a.K2 = 2 * K;
    a.cand_scratch = w.cand; a.top_score = w.row_top_score; a.top_c = w.row_top_c; a.n_top = w.n_top; a.done = nullptr;
    P5_TRY(launch_dec_score<T>(streaming, rows, a, s));
  }
  // REPLAY with the real beam width
  P5_LAUNCH(p5_beam_init_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, w.st, v.child_off, v.child_tok, v.child_node, v.roots, B, K, max_len,
            c.pad_id);
  P5_TRY(P5_KCHECK());
  hipMemsetAsync(w.vrow_a, 0, (size_t)R * 4, s);        // every beam starts on row 0 (the start prefix)
  hipMemsetAsync(w.vrow_b, 0, (size_t)R * 4, s);
  hipMemsetAsync(w.missing, 0, (size_t)B * 4, s);
  P5_LAUNCH((p5_verify_range_kernel<T>), dim3(B), dim3(256), 0, s, w.missing, (const T*)w.hn, PU, d);      // (ordered behind the clear on this stream)
  P5_TRY(P5_KCHECK());
  int first = 1;
  if (v.ff.n > 0) {
    // the forced steps of the replay (p5_decode.h): rows 0 .. F-1 are the forced chain (one live prefix per depth), each with ONE child
    P5_LAUNCH(p5_verify_forced_kernel, dim3((R + B * v.ff.n + 255) / 256), dim3(256), 0, s, w.zeros, w.vrow_a, w.vrow_b, (const float*)w.row_top_score, PU, 2 * K,
              B, K, v.ff.n);
    P5_TRY(P5_KCHECK());
    P5_LAUNCH(p5_beam_forced_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, w.st, v.ff, (const float*)w.zeros, B, K, max_len, c.pad_id);
    P5_TRY(P5_KCHECK());
    first = v.ff.n + 1;
  }
  for (int cur_len = first; cur_len < max_len; ++cur_len) {
    P5_LAUNCH(p5_verify_step_kernel, dim3(B), dim3(256), 0, s, w.st, w.pl, (const float*)w.row_top_score, (const int*)w.row_top_c, (const int*)w.n_top, PU,
              v.child_off, v.child_tok, v.child_node, excl, v.excl_words, v.max_c, K, max_len, c.eos_id, R, w.vrow_a, w.vrow_b, w.missing);
    P5_TRY(P5_KCHECK());
  }
  P5_LAUNCH(p5_beam_finalize_kernel, dim3((R * max_len + 255) / 256), dim3(256), 0, s, out_seq, out_score, out_len, w.st, R, max_len);
  P5_TRY(P5_KCHECK());
  hipMemcpyAsync(out_missing, w.missing, (size_t)B * 4, hipMemcpyDeviceToDevice, s);
  v.begun = v.encoded = v.planned = false;
  return 0;
}

// ---- exhaustive catalogue ranking (p5_rank.h): encoder -> decoder_rows_pass over the trie's rows -> edge log-probabilities -> item
// scores -> per-user top N.  One call, nothing kept between calls. ----
struct RankWs {
  void* kv_all;
  int64_t* ids;
  void *x, *y, *n, *qkv, *q, *o, *h, *hn;
  float *lse, *head, *edge_lp, *scores;
  unsigned long long* part;
  int CQ, nchunk;        // layout of the pass: [nchunk][B][CQ]
  int HC_stream, HC_logits;      // rows per launch of the head + score phase (streaming head / materialised logits)
  int G, S;              // first selection stage: G workgroups per user over slices of S items
};
#define P5_RANK_LOGITS_BYTES ((size_t)256 << 20)      // the [rows, V] logits of one head chunk never exceed this
static void rank_select_grid(int n_items, int top_n, int& G, int& S) {      // first selection stage: G workgroups per user over slices of S items
  const int slice = top_n * 4 > 1024 ? top_n * 4 : 1024;
  G = (n_items + slice - 1) / slice;
  G = G < 1 ? 1 : (G > 64 ? 64 : G);
  S = (n_items + G - 1) / G;
}
static int64_t layout_rank(P5Engine* e, char* base, int B, int L, int rows, int64_t n_edges, int n_items, int top_n, RankWs* out) {
  const P5Config& c = e->c;
  const size_t sz = c.dtype == 1 ? 2 : 4;
  const int d = c.d_model, in = e->inner, F = c.d_ff, H = c.n_heads;
  RankWs tmp;
  RankWs& w = out ? *out : tmp;
  // at most 512 rows of a user per chunk (the cross-attention kernels' query limit), chunks of equal size in whole 16-row tiles
  w.nchunk = (rows + 511) / 512;
  w.CQ = ((rows + w.nchunk - 1) / w.nchunk + 15) / 16 * 16;
  const size_t R = (size_t)B * w.CQ * w.nchunk;
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  const int64_t enc_bytes = layout_ws(e, base, B, L, 0, false);
  Bump b{base, (size_t)enc_bytes};
  w.kv_all = b.take((size_t)B * L * c.n_dec_layers * 2 * in * sz);
  w.ids = (int64_t*)b.take(R * 8);
  w.x = b.take(R * d * sz); w.y = b.take(R * d * sz); w.n = b.take(R * d * sz);
  w.qkv = b.take(R * 3 * in * sz); w.q = b.take(R * in * sz); w.o = b.take(R * in * sz);
  w.h = b.take(R * (c.gated_gelu ? 3 : 1) * F * sz); w.hn = b.take(R * d * sz);
  w.lse = (float*)b.take((size_t)B * H * w.CQ * 4);
  // head + score phase in row chunks: per-tile partials of the streaming head, or the logits of the materialised route
  const int nv = head_nv(e);
  const size_t nt = nv > 0 ? (size_t)(c.vocab_size + nv - 1) / nv : 0;
  size_t hl = P5_RANK_LOGITS_BYTES / ((size_t)Vp * 4) / 16 * 16;
  hl = hl < 16 ? 16 : hl;
  w.HC_logits = (int)(hl < R ? hl : R);
  w.HC_stream = (int)(R < 8192 ? R : 8192);
  const size_t head_bytes_l = (size_t)w.HC_logits * Vp * 4, head_bytes_s = 2 * (size_t)w.HC_stream * nt * 4;
  w.head = (float*)b.take(head_bytes_l > head_bytes_s ? head_bytes_l : head_bytes_s);
  w.edge_lp = (float*)b.take((size_t)B * n_edges * 4);
  w.scores = (float*)b.take((size_t)B * n_items * 4);
  rank_select_grid(n_items, top_n, w.G, w.S);
  w.part = (unsigned long long*)b.take((size_t)B * w.G * top_n * 8);
  return (int64_t)((b.off + 255) & ~(size_t)255);
}

// tied head + the log-probability of every child edge of every row of a pass, in row chunks (the buffers of this phase do not grow with
// the catalogue).  rs.sel == nullptr: the pass holds every plan row (rank_items_impl); else row i of user b is plan row sel[b][i]
// (prune_decide_impl).  head: the partials of the streaming head or the logits of one chunk.
// the part of rank_edges that takes its operands as arguments (p5_op_rank_edges runs it too): E [V][d] the tied embedding, nv the streaming
// head's tile (head_nv; 0: materialised logits, ld = V rounded up to 64), HC_stream / HC_logits the rows per head chunk
template <class T>
static int rank_edges_t(const T* E, int d, int V, int nv, float* edge_lp, int64_t n_edges, const void* hn_all, float* head, int HC_stream, int HC_logits, int R,
                        const P5RankPlan& pl, P5RankSel rs, const int* child_off, const int* child_tok, hipStream_t s) {
  const int Vp = (V + 63) / 64 * 64;
  const float alpha = 1.0f / sqrtf((float)d);
  const bool streaming = nv > 0;
  const int HC = streaming ? HC_stream : HC_logits;
  for (int g0 = 0; g0 < R; g0 += HC) {
    const int nr = R - g0 < HC ? R - g0 : HC;
    const T* hn = (const T*)hn_all + (size_t)g0 * d;
    if (streaming) {
      const int nt = (V + nv - 1) / nv;
      float* part_m = head; float* part_s = head + (size_t)HC_stream * nt;
      P5_TRY(launch_head_lse_t<T>(nv, E, d, V, part_m, part_s, hn, nr, alpha, nullptr, s));
      P5_PROF_TAG(sizeof(T) == 2 ? "bf16" : "fp32");
      P5_LAUNCH((p5_rank_score_kernel<T>), dim3(nr), dim3(256), 0, s, edge_lp, (long long)n_edges, (const float*)part_m, (const float*)part_s, nt,
                (const T*)hn_all, E, d, alpha, pl, g0, child_off, child_tok, rs);
    } else {
      P5_TRY(linear_fwd<T>(s, hn, d, E, head, Vp, nr, V, d, P5_EPI_STORE, nullptr, 0, alpha, 1));
      P5_LAUNCH(p5_rank_score_logits_kernel, dim3(nr), dim3(256), 0, s, edge_lp, (long long)n_edges, (const float*)head, Vp, V, pl, g0,
                child_off, child_tok, rs);
    }
    P5_TRY(P5_KCHECK());
  }
  return 0;
}
template <class T>
static int rank_edges(P5Engine* e, float* edge_lp, int64_t n_edges, const void* hn_all, float* head, int HC_stream, int HC_logits, int R, const P5RankPlan& pl,
                      P5RankSel rs, const int* child_off, const int* child_tok, int split_on, hipStream_t s) {
  const int nv = split_on ? 0 : head_nv(e);     // (with split products the head is a throughput GEMM into logits, as in verify_run_impl)
  return rank_edges_t<T>(Wc<T>(e, e->off_E), e->c.d_model, e->c.vocab_size, nv, edge_lp, n_edges, hn_all, head, HC_stream, HC_logits, R, pl, rs, child_off,
                         child_tok, s);
}
// item scores
static int rank_item_scores(float* scores, const float* edge_lp, int64_t n_edges, const int* item_edges, int n_items, int path_len, int B, hipStream_t s) {
  P5_LAUNCH(p5_rank_items_kernel, dim3((n_items + 255) / 256, B), dim3(256), 0, s, scores, edge_lp, (long long)n_edges, item_edges, n_items, path_len);
  return P5_KCHECK();
}
// the per-user top N of scores [B][n_items] (G, S: rank_select_grid)
static int rank_top_n(const float* scores, int n_items, const uint32_t* excluded, unsigned long long* part, int G, int S, int B, int top_n, int* out_index,
                      float* out_score, hipStream_t s) {
  P5_LAUNCH(p5_rank_select_part_kernel, dim3(G, B), dim3(256), 0, s, part, scores, excluded, (n_items + 31) / 32, n_items, S, top_n);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_rank_select_kernel, dim3(B), dim3(256), 0, s, out_index, out_score, (const unsigned long long*)part, G, top_n);
  return P5_KCHECK();
}
// item scores and the per-user top N
static int rank_select(float* scores, const float* edge_lp, int64_t n_edges, const int* item_edges, int n_items, int path_len, const uint32_t* excluded,
                       unsigned long long* part, int G, int S, int B, int top_n, int* out_index, float* out_score, hipStream_t s) {
  P5_TRY(rank_item_scores(scores, edge_lp, n_edges, item_edges, n_items, path_len, B, s));
  return rank_top_n(scores, n_items, excluded, part, G, S, B, top_n, out_index, out_score, s);
}

struct RankArgs {
  const int64_t *input_ids, *whole_word_ids, *attention_mask;
  int B, L;
  const int *child_off, *child_tok;
  int64_t n_edges;
  P5RankPlan pl;
  const int* item_edges;
  int n_items, path_len;
  const uint32_t* excluded;
  int top_n, exact;
  float* out_scores_all; int* out_index; float* out_score; int* out_flagged;
  char* ws;
};
template <class T>
static int rank_items_impl(P5Engine* e, RankArgs& r, hipStream_t s) {
  const P5Config& c = e->c;
  const int split_on = (sizeof(T) == 4 && !r.exact) ? g_opt_verify_split : 0;
  SplitScope split(split_on);
  RankWs w;
  layout_rank(e, r.ws, r.B, r.L, r.pl.rows, r.n_edges, r.n_items, r.top_n, &w);
  const int d = c.d_model, in = e->inner, H = c.n_heads, B = r.B;
  P5RankPlan pl = r.pl;
  pl.B = B; pl.CQ = w.CQ; pl.nchunk = w.nchunk;
  const int R = B * w.CQ * w.nchunk;
  // encoder + the cross-attention K/V of every decoder layer (as verify_encode_impl)
  layout_ws(e, r.ws, B, r.L, 0, false);
  e->B = B; e->Gt = 1; e->Bd = B; e->tgt_w = nullptr; e->L = r.L; e->T = 0; e->M = B * r.L; e->Md = 0; e->training = 0;
  e->ids = r.input_ids; e->ww = r.whole_word_ids; e->mask = r.attention_mask; e->labels = nullptr;
  P5_TRY(encoder_fwd<T>(e, s));
  P5_TRY(linear_fwd<T>(s, e->enc_out, c.d_model, Wc<T>(e, e->dec[0].ca.k), w.kv_all, c.n_dec_layers * 2 * in, B * r.L, c.n_dec_layers * 2 * in, c.d_model));
  // the decoder over every prefix of the trie
  P5_LAUNCH(p5_rank_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, s, w.ids, pl, c.pad_id);
  P5_TRY(P5_KCHECK());
  RowsPassBufs pb;
  pb.ids = w.ids; pb.x = w.x; pb.y = w.y; pb.n = w.n; pb.qkv = w.qkv; pb.q = w.q; pb.o = w.o; pb.h = w.h; pb.hn = w.hn; pb.lse = w.lse; pb.kv_all = w.kv_all;
  auto tree_attn = [&](T* o, const T* qkv) -> int {
    return rank_tree_attn<T>(o, qkv, pl, (const float*)(e->P + e->off_dec_rel), e->lut_dec, e->lut_half, H, s);
  };
  P5_TRY((decoder_rows_pass<T>(e, pb, B, w.CQ, w.nchunk, r.L, tree_attn, s)));
  hipMemsetAsync(r.out_flagged, 0, (size_t)B * 4, s);
  if (split_on) {     // (ordered behind the clear on this stream)
    P5_LAUNCH((p5_rank_range_kernel<T>), dim3(B, w.nchunk), dim3(256), 0, s, r.out_flagged, (const T*)w.hn, B, w.CQ, d);
    P5_TRY(P5_KCHECK());
  }
  // tied head + the log-probability of every edge
  hipMemsetAsync(w.edge_lp, 0, (size_t)B * r.n_edges * 4, s);
  P5_TRY((rank_edges<T>(e, w.edge_lp, r.n_edges, w.hn, w.head, w.HC_stream, w.HC_logits, R, pl, P5RankSel{nullptr, nullptr, 0}, r.child_off, r.child_tok,
                        split_on, s)));
  // item scores and the per-user top N
  P5_TRY(rank_select(w.scores, w.edge_lp, r.n_edges, r.item_edges, r.n_items, r.path_len, r.excluded, w.part, w.G, w.S, B, r.top_n, r.out_index, r.out_score, s));
  if (r.out_scores_all) hipMemcpyAsync(r.out_scores_all, w.scores, (size_t)B * r.n_items * 4, hipMemcpyDeviceToDevice, s);
  return 0;
}

// ---- per-user candidate lists (p5_cand.h): PLAN on the device (p5_cand_plan: the users' rows, the largest row count in the header word
// the host reads) -> encoder -> decoder_rows_pass over each user's own rows -> the requested edges only -> per-user order.  The plan's
// buffers lead the workspace and depend on B, C and path_len alone; nothing depends on the size of the catalogue. ----
struct CandWs {
  int *hdr, *n_rows, *sel;
  unsigned long long* keys;
  int cap, P;            // stride of sel; keys per user of the plan's sort (a power of two)
  size_t plan_bytes;
  void* kv_all;
  int64_t* ids;
  void *x, *y, *n, *qkv, *q, *o, *h, *hn;
  float *lse, *head, *row_lse, *scores;
  int CQ, nchunk, HC_stream, HC_logits;
};
static Bump layout_sel_pass(P5Engine* e, char* pass, int B, int L, int rows, CandWs& w);
static int64_t layout_cand(P5Engine* e, char* base, int B, int L, int C, int path_len, int rows, CandWs* out) {
  CandWs tmp;
  CandWs& w = out ? *out : tmp;
  Bump p{base, 0};
  w.cap = C * path_len;
  w.P = 256;
  while (w.P < w.cap) w.P <<= 1;
  w.hdr = (int*)p.take(64);
  w.n_rows = (int*)p.take((size_t)B * 4);
  w.sel = (int*)p.take((size_t)B * w.cap * 4);
  w.keys = (unsigned long long*)p.take((size_t)B * w.P * 8);
  w.plan_bytes = (p.off + 255) & ~(size_t)255;
  if (rows <= 0) return (int64_t)w.plan_bytes;
  Bump b = layout_sel_pass(e, base ? base + w.plan_bytes : nullptr, B, L, rows, w);
  const size_t R = (size_t)B * w.CQ * w.nchunk;
  w.row_lse = (float*)b.take(R * 4);
  w.scores = (float*)b.take((size_t)B * C * 4);
  return (int64_t)(w.plan_bytes + ((b.off + 255) & ~(size_t)255));
}
// the buffers of a pass over per-user subsets of the plan's rows (encoder, K/V, decoder_rows_pass, head chunk) behind a plan of
// w.plan_bytes: shared by layout_cand and layout_prune
static Bump layout_sel_pass(P5Engine* e, char* pass, int B, int L, int rows, CandWs& w) {
  const P5Config& c = e->c;
  const size_t sz = c.dtype == 1 ? 2 : 4;
  const int d = c.d_model, in = e->inner, F = c.d_ff, H = c.n_heads;
  w.nchunk = (rows + 511) / 512;
  w.CQ = ((rows + w.nchunk - 1) / w.nchunk + 15) / 16 * 16;
  const size_t R = (size_t)B * w.CQ * w.nchunk;
  const int Vp = (c.vocab_size + 63) / 64 * 64;
  const int64_t enc_bytes = layout_ws(e, pass, B, L, 0, false);
  Bump b{pass, (size_t)enc_bytes};
  w.kv_all = b.take((size_t)B * L * c.n_dec_layers * 2 * in * sz);
  w.ids = (int64_t*)b.take(R * 8);
  w.x = b.take(R * d * sz); w.y = b.take(R * d * sz); w.n = b.take(R * d * sz);
  w.qkv = b.take(R * 3 * in * sz); w.q = b.take(R * in * sz); w.o = b.take(R * in * sz);
  w.h = b.take(R * (c.gated_gelu ? 3 : 1) * F * sz); w.hn = b.take(R * d * sz);
  w.lse = (float*)b.take((size_t)B * H * w.CQ * 4);
  const int nv = head_nv(e);
  const size_t nt = nv > 0 ? (size_t)(c.vocab_size + nv - 1) / nv : 0;
  size_t hl = P5_RANK_LOGITS_BYTES / ((size_t)Vp * 4) / 16 * 16;
  hl = hl < 16 ? 16 : hl;
  w.HC_logits = (int)(hl < R ? hl : R);
  w.HC_stream = (int)(R < 8192 ? R : 8192);
  const size_t head_bytes_l = (size_t)w.HC_logits * Vp * 4, head_bytes_s = 2 * (size_t)w.HC_stream * nt * 4;
  w.head = (float*)b.take(head_bytes_l > head_bytes_s ? head_bytes_l : head_bytes_s);
  return b;
}

// the launches of p5_cand.h with their operands as arguments (the p5_op_cand_* entries run them too)
static int cand_plan_rows(int* sel, int* n_rows, int* hdr, unsigned long long* keys, const int* cand, const int* item_rows, int B, int C, int n_items, int path_len,
                          int cap, int P, hipStream_t s) {
  P5_LAUNCH(p5_cand_plan_kernel, dim3(B), dim3(256), 0, s, sel, n_rows, keys, cand, item_rows, C, n_items, path_len, cap, P);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_cand_hdr_kernel, dim3(1), dim3(64), 0, s, hdr, (const int*)n_rows, B);
  return P5_KCHECK();
}
static int cand_pass_ids(int64_t* ids, const P5CandPlan& pl, int pad_id, hipStream_t s) {
  const int R = pl.g.B * pl.g.CQ * pl.g.nchunk;
  P5_LAUNCH(p5_cand_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, s, ids, pl, pad_id);
  return P5_KCHECK();
}
template <class T>
static int cand_score_order(float* scores, const T* hn, const T* E, int d, const float* row_lse, const P5CandPlan& pl, const int* cand, int C, const int* item_rows,
                            const int64_t* item_tok, int ldt, int n_items, int path_len, int* out_order, int* out_index, float* out_score, int top_n,
                            hipStream_t s) {
  const float alpha = 1.0f / sqrtf((float)d);
  P5_PROF_TAG(sizeof(T) == 2 ? "bf16" : "fp32");
  P5_LAUNCH((p5_cand_score_kernel<T>), dim3((C + 31) / 32, pl.g.B), dim3(256), 0, s, scores, hn, E, d, alpha, row_lse, pl, cand, C, item_rows, item_tok, ldt, n_items,
            path_len);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_cand_order_kernel, dim3(pl.g.B), dim3(256), 0, s, out_order, out_index, out_score, (const float*)scores, cand, C, n_items, top_n);
  return P5_KCHECK();
}
static int cand_plan_impl(P5Engine* e, const int* cand, int B, int C, const int* item_rows, int n_items, int path_len, char* ws, hipStream_t s) {
  CandWs w;
  layout_cand(e, ws, B, 1, C, path_len, 0, &w);
  return cand_plan_rows(w.sel, w.n_rows, w.hdr, w.keys, cand, item_rows, B, C, n_items, path_len, w.cap, w.P, s);
}

// A pass over per-user subsets of the plan's rows, in two parts (`pass`: where its buffers start, behind the plan's).  layout_sel_pass puts
// the encoder's buffers and kv_all in front of everything that depends on the row count, so what the first part leaves stays where it is
// while the second runs again with more rows (bound_round_impl).
static void sel_pass_bind(P5Engine* e, char* pass, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L) {
  layout_ws(e, pass, B, L, 0, false);
  e->B = B; e->Gt = 1; e->Bd = B; e->tgt_w = nullptr; e->L = L; e->T = 0; e->M = B * L; e->Md = 0; e->training = 0;
  e->ids = input_ids; e->ww = whole_word_ids; e->mask = attention_mask; e->labels = nullptr;
}
// first part: encoder + the cross-attention K/V of every decoder layer (as verify_encode_impl)
template <class T>
static int sel_encode_pass(P5Engine* e, const CandWs& w, char* pass, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                           int B, int L, hipStream_t s) {
  const P5Config& c = e->c;
  const int in = e->inner;
  sel_pass_bind(e, pass, input_ids, whole_word_ids, attention_mask, B, L);
  P5_TRY(encoder_fwd<T>(e, s));
  return linear_fwd<T>(s, e->enc_out, c.d_model, Wc<T>(e, e->dec[0].ca.k), w.kv_all, c.n_dec_layers * 2 * in, B * L, c.n_dec_layers * 2 * in, c.d_model);
}
// second part: the decoder over every user's own rows pl.sel + the range guard of the split-product pass into out_flagged (cleared first)
template <class T>
static int sel_decode_pass(P5Engine* e, const CandWs& w, const P5CandPlan& pl, char* pass, const int64_t* input_ids, const int64_t* whole_word_ids,
                           const int64_t* attention_mask, int L, int split_on, int* out_flagged, hipStream_t s) {
  const P5Config& c = e->c;
  const int d = c.d_model, H = c.n_heads, B = pl.g.B;
  const int R = B * w.CQ * w.nchunk;
  sel_pass_bind(e, pass, input_ids, whole_word_ids, attention_mask, B, L);
  P5_TRY(cand_pass_ids(w.ids, pl, c.pad_id, s));
  RowsPassBufs pb;
  pb.ids = w.ids; pb.x = w.x; pb.y = w.y; pb.n = w.n; pb.qkv = w.qkv; pb.q = w.q; pb.o = w.o; pb.h = w.h; pb.hn = w.hn; pb.lse = w.lse; pb.kv_all = w.kv_all;
  auto tree_attn = [&](T* o, const T* qkv) -> int {
    return cand_tree_attn<T>(o, qkv, pl, (const float*)(e->P + e->off_dec_rel), e->lut_dec, e->lut_half, H, s);
  };
  P5_TRY((decoder_rows_pass<T>(e, pb, B, w.CQ, w.nchunk, L, tree_attn, s)));
  hipMemsetAsync(out_flagged, 0, (size_t)B * 4, s);
  if (split_on) {     // (ordered behind the clear on this stream)
    P5_LAUNCH((p5_rank_range_kernel<T>), dim3(B, w.nchunk), dim3(256), 0, s, out_flagged, (const T*)w.hn, B, w.CQ, d);
    P5_TRY(P5_KCHECK());
  }
  return 0;
}
// the two parts back to back: cand_score_impl and prune_decide_impl
template <class T>
static int sel_rows_pass(P5Engine* e, const CandWs& w, const P5CandPlan& pl, char* pass, const int64_t* input_ids, const int64_t* whole_word_ids,
                         const int64_t* attention_mask, int L, int split_on, int* out_flagged, hipStream_t s) {
  P5_TRY((sel_encode_pass<T>(e, w, pass, input_ids, whole_word_ids, attention_mask, pl.g.B, L, s)));
  return sel_decode_pass<T>(e, w, pl, pass, input_ids, whole_word_ids, attention_mask, L, split_on, out_flagged, s);
}

// the log-sum-exp over the vocabulary of every row of a pass, in row chunks: rank_edges_t's two head routes (p5_op_cand_row_lse runs it too)
template <class T>
static int cand_row_lse_t(const T* E, int d, int V, int nv, float* row_lse, const void* hn_all, float* head, int HC_stream, int HC_logits, int R, hipStream_t s) {
  const int Vp = (V + 63) / 64 * 64;
  const float alpha = 1.0f / sqrtf((float)d);
  const bool streaming = nv > 0;
  const int HC = streaming ? HC_stream : HC_logits;
  for (int g0 = 0; g0 < R; g0 += HC) {
    const int nr = R - g0 < HC ? R - g0 : HC;
    const T* hn = (const T*)hn_all + (size_t)g0 * d;
    if (streaming) {
      const int nt = (V + nv - 1) / nv;
      float* part_m = head; float* part_s = head + (size_t)HC_stream * nt;
      P5_TRY(launch_head_lse_t<T>(nv, E, d, V, part_m, part_s, hn, nr, alpha, nullptr, s));
      P5_LAUNCH(p5_cand_lse_kernel, dim3(nr), dim3(256), 0, s, row_lse, (const float*)part_m, (const float*)part_s, nt, g0);
    } else {
      P5_TRY(linear_fwd<T>(s, hn, d, E, head, Vp, nr, V, d, P5_EPI_STORE, nullptr, 0, alpha, 1));
      P5_LAUNCH(p5_cand_lse_logits_kernel, dim3(nr), dim3(256), 0, s, row_lse, (const float*)head, Vp, V, g0);
    }
    P5_TRY(P5_KCHECK());
  }
  return 0;
}

struct CandArgs {
  const int64_t *input_ids, *whole_word_ids, *attention_mask;
  int B, L;
  const int *row_tok, *row_depth, *row_anc;
  int max_depth;
  const int *cand, *item_rows;
  const int64_t* item_tokens;
  int C, n_items, path_len, ldt, rows, top_n, exact;
  float* out_scores; int* out_order; int* out_index; float* out_score; int* out_flagged;
  char* ws;
};
template <class T>
static int cand_score_impl(P5Engine* e, CandArgs& r, hipStream_t s) {
  const P5Config& c = e->c;
  const int split_on = (sizeof(T) == 4 && !r.exact) ? g_opt_verify_split : 0;
  SplitScope split(split_on);
  CandWs w;
  layout_cand(e, r.ws, r.B, r.L, r.C, r.path_len, r.rows, &w);
  const int d = c.d_model, B = r.B;
  P5CandPlan pl;
  pl.g.row_tok = r.row_tok; pl.g.row_depth = r.row_depth; pl.g.row_node = nullptr; pl.g.anc = r.row_anc;
  pl.g.rows = r.rows; pl.g.max_depth = r.max_depth; pl.g.B = B; pl.g.CQ = w.CQ; pl.g.nchunk = w.nchunk;
  pl.sel = w.sel; pl.n_rows = w.n_rows; pl.cap = w.cap;
  const int R = B * w.CQ * w.nchunk;
  P5_TRY((sel_rows_pass<T>(e, w, pl, r.ws + w.plan_bytes, r.input_ids, r.whole_word_ids, r.attention_mask, r.L, split_on, r.out_flagged, s)));
  // tied head: the log-sum-exp of every row, in row chunks (the two routes of rank_items_impl, chosen by the same condition)
  P5_TRY((cand_row_lse_t<T>(Wc<T>(e, e->off_E), d, c.vocab_size, split_on ? 0 : head_nv(e), w.row_lse, w.hn, w.head, w.HC_stream, w.HC_logits, R, s)));
  // the candidates' scores and the per-user order
  P5_TRY((cand_score_order<T>(w.scores, (const T*)w.hn, Wc<T>(e, e->off_E), d, w.row_lse, pl, r.cand, r.C, r.item_rows, r.item_tokens, r.ldt, r.n_items,
                              r.path_len, r.out_order, r.out_index, r.out_score, r.top_n, s)));
  hipMemcpyAsync(r.out_scores, w.scores, (size_t)B * r.C * 4, hipMemcpyDeviceToDevice, s);
  return 0;
}

// ---- certified pruned ranking (p5_prune.h).  PROPOSE on the bf16 engine: the unchanged rank_items_impl pass in its own workspace, then
// the rows worth fp32 numbers into the head of the prune workspace (hdr | n_rows [B] | sel [B][rows of the plan]: the plan protocol of
// p5_cand_plan, the head depends on B and the plan's row count alone, so the engine that decides finds it where this one left it).
// DECIDE on the fp32 engine: sel_rows_pass over sel -> rank_edges through sel -> mask -> rank_select -> certificate. ----
struct PruneWs : CandWs {
  float* edge_lp;
  uint32_t* excl;
  unsigned long long* part;
  int G, S;
};
// the pass behind a head of w.plan_bytes: shared by layout_prune and layout_bound
static int64_t layout_prune_pass(P5Engine* e, char* base, int B, int L, int rows, int64_t n_edges, int n_items, int top_n, PruneWs& w) {
  Bump b = layout_sel_pass(e, base ? base + w.plan_bytes : nullptr, B, L, rows, w);
  w.edge_lp = (float*)b.take((size_t)B * n_edges * 4);
  w.scores = (float*)b.take((size_t)B * n_items * 4);
  w.excl = (uint32_t*)b.take((size_t)B * ((n_items + 31) / 32) * 4);
  rank_select_grid(n_items, top_n, w.G, w.S);
  w.part = (unsigned long long*)b.take((size_t)B * w.G * top_n * 8);
  return (int64_t)(w.plan_bytes + ((b.off + 255) & ~(size_t)255));
}
static int64_t layout_prune(P5Engine* e, char* base, int B, int L, int rows_total, int rows, int64_t n_edges, int n_items, int top_n, PruneWs* out) {
  PruneWs tmp;
  PruneWs& w = out ? *out : tmp;
  Bump p{base, 0};
  w.cap = rows_total;
  w.P = 0; w.keys = nullptr; w.row_lse = nullptr;
  w.hdr = (int*)p.take(64);
  w.n_rows = (int*)p.take((size_t)B * 4);
  w.sel = (int*)p.take((size_t)B * w.cap * 4);
  w.plan_bytes = (p.off + 255) & ~(size_t)255;
  if (rows <= 0) return (int64_t)w.plan_bytes;
  return layout_prune_pass(e, base, B, L, rows, n_edges, n_items, top_n, w);
}

// the launches of p5_prune.h with their operands as arguments (the p5_op_prune_* entries run them too)
// PROPOSE: sel / n_rows from a pass's edge_lp and its selected scores, the largest row count into hdr[0]
static int prune_propose_rows(int* sel, int* n_rows, int* hdr, const float* edge_lp, int64_t n_edges, const float* top_score, int N, const P5RankPlan& pl,
                              const int* row_edge, const int* row_lmax, float slack, int B, hipStream_t s) {
  P5_LAUNCH(p5_prune_propose_kernel, dim3(B), dim3(256), 0, s, sel, n_rows, edge_lp, (long long)n_edges, top_score, N, pl, row_edge, row_lmax, slack);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_cand_hdr_kernel, dim3(1), dim3(64), 0, s, hdr, (const int*)n_rows, B);
  return P5_KCHECK();
}
static int prune_fill(float* p, size_t n, float v, hipStream_t s) {
  P5_LAUNCH(p5_prune_fill_kernel, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, s, p, n, v);
  return P5_KCHECK();
}
static int prune_mask(uint32_t* out, const uint32_t* excluded, const float* edge_lp, int64_t n_edges, const int* item_edges, int n_items, int path_len, int B,
                      hipStream_t s) {
  const int words = (n_items + 31) / 32;
  P5_LAUNCH(p5_prune_mask_kernel, dim3((words + 255) / 256, B), dim3(256), 0, s, out, excluded, words, edge_lp, (long long)n_edges, item_edges, n_items, path_len);
  return P5_KCHECK();
}
static int prune_certify(int* flagged, const float* edge_lp, int64_t n_edges, const P5CandPlan& pl, const int* row_edge, const int* edge_row, const int* row_lmax,
                         const int* child_off, const int* out_index, const float* out_score, int N, float margin, hipStream_t s) {
  P5_LAUNCH(p5_prune_certify_kernel, dim3((pl.g.CQ * pl.g.nchunk + 255) / 256, pl.g.B), dim3(256), 0, s, flagged, edge_lp, (long long)n_edges, pl, row_edge,
            edge_row, row_lmax, child_off, out_index, out_score, N, margin);
  return P5_KCHECK();
}

template <class T>
static int prune_propose_impl(P5Engine* e, RankArgs& r, const int* row_edge, const int* row_lmax, float slack, char* prune_ws, hipStream_t s) {
  P5_TRY(rank_items_impl<T>(e, r, s));
  RankWs w;
  layout_rank(e, r.ws, r.B, r.L, r.pl.rows, r.n_edges, r.n_items, r.top_n, &w);
  PruneWs p;
  layout_prune(e, prune_ws, r.B, 1, r.pl.rows, 0, r.n_edges, r.n_items, r.top_n, &p);
  return prune_propose_rows(p.sel, p.n_rows, p.hdr, w.edge_lp, r.n_edges, r.out_score, r.top_n, r.pl, row_edge, row_lmax, slack, r.B, s);
}

struct PruneArgs {
  RankArgs r;               // (r.pl: the trie's plan; r.ws: the prune workspace; r.exact unused: a user out of range falls back)
  const int *row_edge, *row_lmax, *edge_row;
  int rows;                 // rows per user of the pass (>= the header word)
  float margin;
};
// DECIDE + CERTIFY behind the encoder: the decoder over sel, the edges, the mask, the selection, the certificate.  Shared by
// prune_decide_impl (once) and bound_round_impl (every round, over a sel that grows).
template <class T>
static int prune_decide_rows(P5Engine* e, PruneArgs& a, const PruneWs& w, const P5CandPlan& pl, int split_on, hipStream_t s) {
  RankArgs& r = a.r;
  const int B = r.B;
  const int R = B * w.CQ * w.nchunk;
  P5_TRY((sel_decode_pass<T>(e, w, pl, r.ws + w.plan_bytes, r.input_ids, r.whole_word_ids, r.attention_mask, r.L, split_on, r.out_flagged, s)));
  // the log-probability of every child edge of every sel row; every other edge keeps the sentinel
  P5_TRY(prune_fill(w.edge_lp, (size_t)B * r.n_edges, P5_PRUNE_SENTINEL, s));
  P5_TRY((rank_edges<T>(e, w.edge_lp, r.n_edges, w.hn, w.head, w.HC_stream, w.HC_logits, R, pl.g, P5RankSel{w.sel, w.n_rows, w.cap}, r.child_off, r.child_tok,
                        split_on, s)));
  // items whose path was not scored in full join the user's exclusion bitmap; then the selection of rank_items_impl
  P5_TRY(prune_mask(w.excl, r.excluded, w.edge_lp, r.n_edges, r.item_edges, r.n_items, r.path_len, B, s));
  P5_TRY(rank_select(w.scores, w.edge_lp, r.n_edges, r.item_edges, r.n_items, r.path_len, w.excl, w.part, w.G, w.S, B, r.top_n, r.out_index, r.out_score, s));
  return prune_certify(r.out_flagged, w.edge_lp, r.n_edges, pl, a.row_edge, a.edge_row, a.row_lmax, r.child_off, r.out_index, r.out_score, r.top_n, a.margin, s);
}
static P5CandPlan prune_pass_plan(const PruneArgs& a, const PruneWs& w) {
  P5CandPlan pl;
  pl.g = a.r.pl;
  pl.g.rows = a.rows; pl.g.B = a.r.B; pl.g.CQ = w.CQ; pl.g.nchunk = w.nchunk;
  pl.sel = w.sel; pl.n_rows = w.n_rows; pl.cap = w.cap;
  return pl;
}
template <class T>
static int prune_decide_impl(P5Engine* e, PruneArgs& a, hipStream_t s) {
  RankArgs& r = a.r;
  const int split_on = sizeof(T) == 4 ? g_opt_verify_split : 0;
  SplitScope split(split_on);
  PruneWs w;
  layout_prune(e, r.ws, r.B, r.L, r.pl.rows, a.rows, r.n_edges, r.n_items, r.top_n, &w);
  const P5CandPlan pl = prune_pass_plan(a, w);
  P5_TRY((sel_encode_pass<T>(e, w, r.ws + w.plan_bytes, r.input_ids, r.whole_word_ids, r.attention_mask, r.B, r.L, s)));
  return prune_decide_rows<T>(e, a, w, pl, split_on, s);
}

// ---- bounded trie search (p5_bound.h).  The workspace: the head of the prune workspace (hdr | n_rows [B] | sel [B][rows of the plan]) +
// grew [B] + the sort keys [B][KP], then the pass of layout_prune.  BEGIN: encoder + K/V, the seeds' rows into sel.  ROUND: the rows part
// of the pass over sel, DECIDE + CERTIFY as prune_decide_impl, then the frontier rows within reach of tau join sel. ----
struct BoundWs : PruneWs {
  int* grew;
  int KP;                   // keys per user: a power of two >= max(the plan's rows, n_seeds * max_depth + 1, 256)
};
static int64_t layout_bound(P5Engine* e, char* base, int B, int L, int rows_total, int rows, int64_t n_edges, int n_items, int top_n, int n_seeds,
                            int max_depth, BoundWs* out) {
  BoundWs tmp;
  BoundWs& w = out ? *out : tmp;
  Bump p{base, 0};
  w.cap = rows_total;
  w.P = 0; w.row_lse = nullptr;
  w.hdr = (int*)p.take(64);
  w.n_rows = (int*)p.take((size_t)B * 4);
  w.sel = (int*)p.take((size_t)B * w.cap * 4);
  w.grew = (int*)p.take((size_t)B * 4);
  const int64_t slots = (int64_t)n_seeds * max_depth + 1;
  w.KP = 256;
  while (w.KP < rows_total || w.KP < slots) w.KP <<= 1;
  w.keys = (unsigned long long*)p.take((size_t)B * w.KP * 8);
  w.plan_bytes = (p.off + 255) & ~(size_t)255;
  if (rows <= 0) return (int64_t)w.plan_bytes;
  return layout_prune_pass(e, base, B, L, rows, n_edges, n_items, top_n, w);
}
struct BoundArgs {
  PruneArgs p;              // (p.r.ws: the bound workspace)
  const int64_t* seeds;     // [B][n_seeds][seed_len] (p5_bound_begin)
  int n_seeds, seed_len;
};
// the launches of p5_bound.h with their operands as arguments (the p5_op_bound_* entries run them too)
// BEGIN: the seeds' rows into sel / n_rows, the largest row count into hdr[0] (hdr[1] = 0).  keys: [B][KP], KP a power of two >= S * max_depth + 1
// (layout_bound sizes KP so; p5_op_bound_seed checks it)
static int bound_seed_rows(int* sel, int* n_rows, int* hdr, unsigned long long* keys, int KP, int cap, const int64_t* seeds, int S, int T, const int* child_off,
                           const int* child_tok, const int* edge_row, const int* row_tok, const int* row_node, int max_depth, int B, hipStream_t s) {
  int P = 256;
  while (P < S * max_depth + 1) P <<= 1;
  P5_LAUNCH(p5_bound_seed_kernel, dim3((S + 255) / 256, B), dim3(256), 0, s, keys, KP, P, seeds, S, T, child_off, child_tok, edge_row, row_tok, row_node, max_depth);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_bound_union_kernel, dim3(B), dim3(256), 0, s, sel, n_rows, keys, KP, P, cap);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_bound_hdr_kernel, dim3(1), dim3(64), 0, s, hdr, (const int*)n_rows, (const int*)nullptr, B);
  return P5_KCHECK();
}
// ROUND, after the certificate: the frontier rows within reach of tau join sel; hdr = (the largest row count, the users that grew)
static int bound_expand_rows(int* sel, int* n_rows, int* grew, int* hdr, unsigned long long* keys, int KP, const float* edge_lp, int64_t n_edges,
                             const P5CandPlan& pl, const int* row_edge, const int* edge_row, const int* row_lmax, const int* child_off, const float* out_score,
                             int N, float margin, hipStream_t s) {
  P5_LAUNCH(p5_bound_expand_kernel, dim3(pl.g.B), dim3(256), 0, s, sel, n_rows, grew, keys, KP, edge_lp, (long long)n_edges, pl, row_edge, edge_row, row_lmax,
            child_off, out_score, N, margin);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_bound_hdr_kernel, dim3(1), dim3(64), 0, s, hdr, (const int*)n_rows, (const int*)grew, pl.g.B);
  return P5_KCHECK();
}
template <class T>
static int bound_begin_impl(P5Engine* e, BoundArgs& a, hipStream_t s) {
  RankArgs& r = a.p.r;
  const int split_on = sizeof(T) == 4 ? g_opt_verify_split : 0;
  SplitScope split(split_on);
  BoundWs w;
  layout_bound(e, r.ws, r.B, r.L, r.pl.rows, 1, r.n_edges, r.n_items, r.top_n, a.n_seeds, r.pl.max_depth, &w);
  P5_TRY((sel_encode_pass<T>(e, w, r.ws + w.plan_bytes, r.input_ids, r.whole_word_ids, r.attention_mask, r.B, r.L, s)));
  return bound_seed_rows(w.sel, w.n_rows, w.hdr, w.keys, w.KP, w.cap, a.seeds, a.n_seeds, a.seed_len, r.child_off, r.child_tok, a.p.edge_row, r.pl.row_tok,
                         r.pl.row_node, r.pl.max_depth, r.B, s);
}
template <class T>
static int bound_round_impl(P5Engine* e, BoundArgs& a, hipStream_t s) {
  RankArgs& r = a.p.r;
  const int split_on = sizeof(T) == 4 ? g_opt_verify_split : 0;
  SplitScope split(split_on);
  BoundWs w;
  layout_bound(e, r.ws, r.B, r.L, r.pl.rows, a.p.rows, r.n_edges, r.n_items, r.top_n, a.n_seeds, r.pl.max_depth, &w);
  const P5CandPlan pl = prune_pass_plan(a.p, w);
  P5_TRY((prune_decide_rows<T>(e, a.p, w, pl, split_on, s)));
  return bound_expand_rows(w.sel, w.n_rows, w.grew, w.hdr, w.keys, w.KP, w.edge_lp, r.n_edges, pl, a.p.row_edge, a.p.edge_row, a.p.row_lmax, r.child_off,
                           r.out_score, r.top_n, a.p.margin, s);
}

// =====================================================================================================
// C ABI
// =====================================================================================================
// out[w_off + r*d + c] = bf16(P[w_off + r*d + c] * P[ln_off + c]) for every listed weight: 8 rows per workgroup, one launch for the model
struct P5FoldTab {
  int n, d;
  struct D { long long w_off, ln_off; int rows, blk0; } e[160];
};
__global__ __launch_bounds__(256) void p5_fold_rows_kernel(bf16* __restrict__ out, const float* __restrict__ P, P5FoldTab tab) {
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;             // last descriptor with blk0 <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.e[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const long long w_off = tab.e[lo].w_off, ln_off = tab.e[lo].ln_off;
  const int rows = tab.e[lo].rows, r0 = (b - tab.e[lo].blk0) * 8, d = tab.d;
  for (int i = threadIdx.x; i < 8 * (d / 8); i += 256) {
    const int r = r0 + i / (d / 8), c = (i % (d / 8)) * 8;
    if (r >= rows) continue;
    float w[8], l[8], o[8];
    ldf<8>(P + w_off + (size_t)r * d + c, w);
    ldf<8>(P + ln_off + c, l);
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = w[q] * l[q];
    st16(out + w_off + (size_t)r * d + c, pack16<bf16>(o));
  }
}

// out[c, r] = in[r, c] for every [rows, cols] block of the descriptor table (64 x 64 tiles through LDS, 16-byte row accesses)
struct P5TrDesc { int64_t off; int rows, cols, tile0; int64_t ln_off; int atile0, pad_; };      // ln_off >= 0: the T5LayerNorm weight folded into this block's copy (W diag(ln)), else -1; atile0: first 64 x 256 tile of p5_adamw_tiles_kernel
__global__ __launch_bounds__(256) void p5_transpose_blocks_kernel(bf16* __restrict__ out, const bf16* __restrict__ in, const P5TrDesc* __restrict__ tab,
                                                                 int ndesc) {
  __shared__ unsigned short tile[64][66];
  const int t = blockIdx.x;
  int lo = 0, hi = ndesc - 1;             // last descriptor with tile0 <= t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].tile0 <= t) lo = mid; else hi = mid - 1;
  }
  const P5TrDesc dsc = tab[lo];
  const int tc = (dsc.cols + 63) / 64;
  const int lt = t - dsc.tile0, r0 = (lt / tc) * 64, c0 = (lt % tc) * 64;
  const unsigned short* src = (const unsigned short*)in + dsc.off;
  unsigned short* dst = (unsigned short*)out + dsc.off;
  for (int i = threadIdx.x; i < 64 * 8; i += 256) {        // 64 rows x 8 pieces of 8 elements
    const int r = i >> 3, p = (i & 7) * 8;
    if (r0 + r < dsc.rows && c0 + p < dsc.cols) {           // (cols is a multiple of 8)
      const u32x4 v = ld16(src + (size_t)(r0 + r) * dsc.cols + c0 + p);
#pragma unroll
      for (int q = 0; q < 4; ++q) { tile[r][p + 2 * q] = (unsigned short)(v[q] & 0xFFFF); tile[r][p + 2 * q + 1] = (unsigned short)(v[q] >> 16); }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 8; i += 256) {        // 64 output rows (= input columns) x 8 pieces
    const int c = i >> 3, p = (i & 7) * 8;
    if (c0 + c < dsc.cols && r0 + p < dsc.rows) {           // (rows is a multiple of 8)
      u32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = (unsigned)tile[p + 2 * q][c] | ((unsigned)tile[p + 2 * q + 1][c] << 16);
      st16(dst + (size_t)(c0 + c) * dsc.rows + r0 + p, v);
    }
  }
}

// ---- clip + HF-AdamW over the arena that ALSO writes every bf16 copy the next step reads (round 6) --------------------------------------
// p5_adamw_kernel streams the flat arena and writes the bf16 shadow; the transposed copy W^T (data gradients) and the norm-folded copy
// W diag(ln) (training forward) were then rebuilt by two more launches that re-read what the update had just held in registers
// (p5_transpose_blocks_kernel + p5_fold_rows_kernel: 0.27 GB, ~80 us of the T5-small step).  Here the 2-D layer weights are updated tile by
// tile (the 64 x 64 tiles of the transpose table): a workgroup updates p / m / v of its tile, writes the shadow rows, transposes the bf16
// tile through LDS into W^T, and -- for a projection behind a T5LayerNorm -- multiplies by the NEW norm weight, which it derives itself from
// that weight's old state (64 columns: the same update formula on values nobody has overwritten yet; the norm weights themselves are
// updated by a second, tiny launch ordered behind this one).  Blocks past the tiles update the leading range of the arena (tied embedding,
// whole-word table, relative-bias tables) flat.  Same arithmetic per element as p5_adamw_kernel: bit-identical parameters and copies.
struct P5AdamTileArgs {
  P5AdamArgs a;
  const P5TrDesc* tab;
  int ndesc, ntiles;
  bf16* St; bf16* Sf;           // transposed / norm-folded copies (arena offsets), Sf may be null
  size_t flat_n;                // [0, flat_n): flat update by the blocks behind the tiles
};
__device__ static __forceinline__ float p5_adam_clip_coef(const P5AdamArgs& a, float* sp) {
  float coef = a.grad_scale;
  if (a.sumsq) {
    float t = 0.f;
    for (int i = threadIdx.x; i < P5_SUMSQ_PARTS; i += 256) t += a.sumsq[i];      // (the association of p5_adamw_kernel: same bits)
    sp[threadIdx.x] = t;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
      if ((int)threadIdx.x < st) sp[threadIdx.x] += sp[threadIdx.x + st];
      __syncthreads();
    }
    const float norm = sqrtf(sp[0]) * a.grad_scale;
    const float c = a.max_norm / (norm + 1e-6f);
    coef *= (c < 1.f ? c : 1.f);
  }
  return coef;
}
__device__ static __forceinline__ float p5_adam_update(const P5AdamArgs& a, float coef, float p, float g0, float& m, float& v) {
  const float g = g0 * coef;
  m = a.beta1 * m + a.omb1 * g;
  v = a.beta2 * v + a.omb2 * g * g;
  p = p - a.step_size * (m / (sqrtf(v) + a.eps));
  p = p - a.decay * p;
  return p;
}
#define P5_ADAM_TW 256        // columns of an AdamW tile: 64 rows x 256 columns = 1 KiB contiguous per row and fp32 array (64 x 64 tiles ran at
                              // 0.6 of the flat kernel's bandwidth: 256-byte pieces on a 2-8 KiB stride, profiles/r06_call2_*.txt)
__global__ __launch_bounds__(256) void p5_adamw_tiles_kernel(P5AdamTileArgs t) {
  __shared__ float sp[256];
  __shared__ unsigned short tile[64][P5_ADAM_TW + 2];
  const P5AdamArgs& a = t.a;
  const float coef = p5_adam_clip_coef(a, sp);
  const int b = blockIdx.x;
  if (b >= t.ntiles) {                       // ---- flat leading range
    const size_t nb = gridDim.x - t.ntiles;
    for (size_t i = (size_t)(b - t.ntiles) * 256 + threadIdx.x; i < t.flat_n; i += nb * 256) {
      float m = a.m[i], v = a.v[i];
      const float p = p5_adam_update(a, coef, a.p[i], a.g[i], m, v);
      a.m[i] = m; a.v[i] = v; a.p[i] = p;
      if (a.shadow) ((bf16*)a.shadow)[i] = from_f<bf16>(p);
    }
    return;
  }
  int lo = 0, hi = t.ndesc - 1;              // last descriptor with atile0 <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.tab[mid].atile0 <= b) lo = mid; else hi = mid - 1;
  }
  const P5TrDesc dsc = t.tab[lo];
  const int tc = (dsc.cols + P5_ADAM_TW - 1) / P5_ADAM_TW;
  const int lt = b - dsc.atile0, r0 = (lt / tc) * 64, c0 = (lt % tc) * P5_ADAM_TW;
  const int rq = threadIdx.x >> 5, cl = (threadIdx.x & 31) * 8;      // 32 threads x 8 columns = one 1-KiB row piece; 8 rows per pass
  const int c = c0 + cl;
  const bool col_ok = c < dsc.cols;                                    // (cols % 8 == 0)
  const bool fold = t.Sf != nullptr && dsc.ln_off >= 0 && col_ok;
  float ln_new[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) ln_new[e] = 0.f;
  if (fold) {
    // the norm weight AFTER this step, from its state before it (the launch that updates it runs behind this one)
    const size_t l0 = (size_t)dsc.ln_off + c;
    float lp[8], lg[8], lm[8], lv[8];
    ldf<8>(a.p + l0, lp); ldf<8>(a.g + l0, lg); ldf<8>(a.m + l0, lm); ldf<8>(a.v + l0, lv);
#pragma unroll
    for (int e = 0; e < 8; ++e) ln_new[e] = p5_adam_update(a, coef, lp[e], lg[e], lm[e], lv[e]);
  }
#pragma unroll 2
  for (int it = 0; it < 8; ++it) {
    const int r = it * 8 + rq;
    if (col_ok && r0 + r < dsc.rows) {
      const size_t i0 = (size_t)dsc.off + (size_t)(r0 + r) * dsc.cols + c;
      float p[8], g[8], m[8], v[8], o[8];
      ldf<8>(a.p + i0, p); ldf<8>(a.g + i0, g); ldf<8>(a.m + i0, m); ldf<8>(a.v + i0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = p5_adam_update(a, coef, p[e], g[e], m[e], v[e]);
      stf<8>(a.p + i0, o); stf<8>(a.m + i0, m); stf<8>(a.v + i0, v);
      const u32x4 pk = pack16<bf16>(o);
      if (a.shadow) st16((bf16*)a.shadow + i0, pk);
      if (fold) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = o[e] * ln_new[e];
        st16(t.Sf + i0, pack16<bf16>(f));
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) { tile[r][cl + 2 * q] = (unsigned short)(pk[q] & 0xFFFF); tile[r][cl + 2 * q + 1] = (unsigned short)(pk[q] >> 16); }
    }
  }
  __syncthreads();
  unsigned short* dst = (unsigned short*)t.St + dsc.off;
  for (int i = threadIdx.x; i < P5_ADAM_TW * 8; i += 256) {        // TW output rows (= input columns) x 8 pieces of 8 input rows
    const int cc = i >> 3, p8 = (i & 7) * 8;
    if (c0 + cc < dsc.cols && r0 + p8 < dsc.rows) {                  // (rows % 8 == 0)
      u32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = (unsigned)tile[p8 + 2 * q][cc] | ((unsigned)tile[p8 + 2 * q + 1][cc] << 16);
      st16(dst + (size_t)(c0 + cc) * dsc.rows + r0 + p8, v);
    }
  }
}
// the parameters the tiles and the leading range do not cover: the T5LayerNorm weights (one segment each), updated LAST
__global__ __launch_bounds__(256) void p5_adamw_segments_kernel(P5AdamArgs a, P5ZeroTab tab) {
  __shared__ float sp[256];
  const float coef = p5_adam_clip_coef(a, sp);
  const int b = blockIdx.x;
  int lo = 0, hi = tab.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.e[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const int i0 = (b - tab.e[lo].blk0) * 8192, n = tab.e[lo].count;
  for (int j = i0 + threadIdx.x; j < i0 + 8192 && j < n; j += 256) {
    const size_t i = (size_t)tab.e[lo].off + j;
    float m = a.m[i], v = a.v[i];
    const float p = p5_adam_update(a, coef, a.p[i], a.g[i], m, v);
    a.m[i] = m; a.v[i] = v; a.p[i] = p;
    if (a.shadow) ((bf16*)a.shadow)[i] = from_f<bf16>(p);
  }
}

extern "C" {

const char* p5_last_error(void) { return g_p5_err.c_str(); }
int p5_set_option(const char* name, int value) {
  if (!strcmp(name, "gemm_v2")) g_opt_gemm_v2 = value;
  else if (!strcmp(name, "gemm_tile")) g_opt_gemm_tile = value;
  else if (!strcmp(name, "gemm_ksdma")) g_opt_gemm_ksdma = value;
  else if (!strcmp(name, "gemm_ring")) g_opt_gemm_ring = value;
  else if (!strcmp(name, "gemm_small_ring")) g_opt_gemm_small_ring = value;
  else if (!strcmp(name, "gemm_small_ring_tiles")) g_opt_gemm_small_ring_tiles = value;
  else if (!strcmp(name, "attn_fused")) g_opt_attn_fused = value;
  else if (!strcmp(name, "attn_fwd_wg")) g_opt_attn_fwd_wg = value;
  else if (!strcmp(name, "attn_fwd_head")) g_opt_attn_fwd_head = value;
  else if (!strcmp(name, "attn_bwd_head")) g_opt_attn_bwd_head = value;
  else if (!strcmp(name, "attn_keep_bits")) g_opt_attn_keep_bits = value;
  else if (!strcmp(name, "attn_op_keep_bits")) g_opt_attn_op_keep_bits = value;
  else if (!strcmp(name, "attn_small")) g_opt_attn_small = value;
  else if (!strcmp(name, "gemm_ring32")) g_opt_gemm_ring32 = value;
  else if (!strcmp(name, "gemm_xcd_rect")) g_opt_gemm_xcd_rect = value;
  else if (!strcmp(name, "dec_nb")) g_opt_dec_nb = value;
  else if (!strcmp(name, "dec_kw")) g_opt_dec_kw = value;
  else if (!strcmp(name, "dec_fuseq")) g_opt_dec_fuseq = value;
  else if (!strcmp(name, "dgrad_t")) g_opt_dgrad_t = value;
  else if (!strcmp(name, "dec_cross")) g_opt_dec_cross = value;
  else if (!strcmp(name, "dec_head")) g_opt_dec_head = value;
  else if (!strcmp(name, "dec_head_nv")) g_opt_dec_head_nv = value;
  else if (!strcmp(name, "verify_split")) g_opt_verify_split = value;
  else if (!strcmp(name, "gen_ff")) g_opt_gen_ff = value;
  else if (!strcmp(name, "gen_wide")) g_opt_gen_wide = value;
  else if (!strcmp(name, "dec_atomic")) g_opt_dec_atomic = value;
  else if (!strcmp(name, "wgrad_group")) g_opt_wgrad_group = value;
  else if (!strcmp(name, "norm_fuse")) g_opt_norm_fuse = value;
  else if (!strcmp(name, "wgrad_wgs")) g_opt_wgrad_wgs = value;
  else if (!strcmp(name, "wgrad_wide")) g_opt_wgrad_wide = value;
  else if (!strcmp(name, "wgrad_side")) g_opt_wgrad_side = value;
  else if (!strcmp(name, "wgrad_layers")) g_opt_wgrad_layers = value;
  else if (!strcmp(name, "wgrad_fill")) g_opt_wgrad_fill = value;
  else if (!strcmp(name, "wgrad_fill_epi")) g_opt_wgrad_fill_epi = value;
  else if (!strcmp(name, "gemm_ring_n512")) g_opt_gemm_ring_n512 = value;
  else if (!strcmp(name, "gemm_wide")) g_opt_gemm_wide = value;
  else if (!strcmp(name, "gemm_ws")) g_opt_gemm_ws = value;
  else if (!strcmp(name, "gemm_ws128")) g_opt_gemm_ws128 = value;
  else if (!strcmp(name, "gemm_rect")) g_opt_gemm_rect = value;
  else if (!strcmp(name, "gemm_ws128_min_k")) g_opt_gemm_ws128_min_k = value;
  else if (!strcmp(name, "gate_fuse")) g_opt_gate_fuse = value;
  else if (!strcmp(name, "norm_bwd_blocks")) g_opt_norm_bwd_blocks = value;
  else if (!strcmp(name, "norm_bwd_fuse")) g_opt_norm_bwd_fuse = value;
  else if (!strcmp(name, "adam_tiles")) g_opt_adam_tiles = value;
  else if (!strcmp(name, "ce_free")) g_opt_ce_free = value;
  else if (!strcmp(name, "gemm_wide_min_tiles")) g_opt_gemm_wide_min_tiles = value;
  else if (!strcmp(name, "gemm_ring128_min_k")) g_opt_gemm_ring128_min_k = value;
  else if (!strcmp(name, "gemm_ring128_min_tiles")) g_opt_gemm_ring128_min_tiles = value;
  else if (!strcmp(name, "wgrad_wide_min")) g_opt_wgrad_wide_min = value;
  else if (!strcmp(name, "grad_store_first")) g_opt_grad_store_first = value;
  else if (!strcmp(name, "embed_det")) g_opt_embed_det = value;
  else if (!strcmp(name, "shift_fuse")) g_opt_shift_fuse = value;
  else if (!strcmp(name, "loss_fuse")) g_opt_loss_fuse = value;
  else if (!strcmp(name, "g4_nst")) g_opt_g4_nst = value;
  else if (!strcmp(name, "g4_wgs")) g_opt_g4_wgs = value;
  else return fail("p5_set_option: unknown option");
  return 0;
}
int p5_abi_version(void) { return 6; }    // 2: p5_op_attn_bwd gained d_rel_scratch / rel_buckets (round 4); 3: p5_generate_verified, p5_backward_staged (round 5); 4: p5_allreduce_range / _sum, p5_verify_row_capacity, range flag in p5_verify_run (round 6); 5: P5GemmProblem gained the T5LayerNorm-backward epilogue fields, p5_op_attn_bwd gained dot_out (round 6); 6: the decode-fold entries (count / bind / refresh of the folded decoder-weight buffer of the round-1 decode step) were removed
// ---- in-run kernel profiler (p5_device.h P5Prof) ----
int p5_profile_begin(void) {
#ifndef P5_EMU
  P5Prof& p = p5_prof();
  p.recs.clear(); p.used = 0; p.pending_flops = 0.0; p.on = 1;
#else
  p5_emu_prof().recs.clear();
  p5_emu_prof().on = 1;
#endif
  return 0;
}
int p5_profile_end(char* report, int cap) {
  if (report && cap > 0) report[0] = 0;
#ifdef P5_EMU
  {   // (host emulation: the launch record only -- which kernels ran, how often; no durations, no FLOPs)
    P5EmuProf& p = p5_emu_prof();
    p.on = 0;
    std::vector<std::pair<std::string, int>> agg;
    for (const std::string& k : p.recs) {
      size_t i = 0;
      for (; i < agg.size(); ++i) if (agg[i].first == k) break;
      if (i == agg.size()) agg.push_back({k, 0});
      agg[i].second++;
    }
    p.recs.clear();
    if (agg.empty()) return 0;
    std::string out = "[";
    for (size_t i = 0; i < agg.size(); ++i) {
      std::string key;
      for (char c : agg[i].first) { if (c == '"' || c == '\\') key += '\\'; key += c; }
      out += (i ? ", " : "") + std::string("{\"kernel\": \"") + key + "\", \"launches\": " + std::to_string(agg[i].second) + ", \"total_us\": 0, \"flops\": 0}";
    }
    out += "]";
    if (report && cap > 0) {
      if ((int)out.size() + 1 > cap) return fail("profile: report buffer too small");
      memcpy(report, out.c_str(), out.size() + 1);
    }
  }
#else
  P5Prof& p = p5_prof();
  p.on = 0;
  if (p.recs.empty()) return 0;
  // records are made on every stream the library launches on (main, side, weight-gradient): wait for all of them, and refuse to report
  // a table with holes in it
  if (hipDeviceSynchronize() != hipSuccess) return fail("profile: device sync failed");
  int dropped = 0;
  struct Agg { std::string key; int n; double us, flops; };
  std::vector<Agg> agg;
  for (const P5Prof::Rec& r : p.recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) { ++dropped; continue; }
    char k[512];
    char shp[64] = "";
    if (r.m > 0) snprintf(shp, sizeof(shp), " %dx%dx%d", r.m, r.n, r.k);
    snprintf(k, sizeof(k), "%s%s%s%s grid=(%u,%u,%u) block=%u%s", r.name, r.tag[0] ? " [" : "", r.tag, r.tag[0] ? "]" : "", r.gx, r.gy, r.gz, r.bx, shp);
    size_t i = 0;
    for (; i < agg.size(); ++i) if (agg[i].key == k) break;
    if (i == agg.size()) agg.push_back({k, 0, 0.0, 0.0});
    agg[i].n++; agg[i].us += ms * 1e3; agg[i].flops += r.flops;
  }
  std::string out = "[";
  for (size_t i = 0; i < agg.size(); ++i) {
    std::string key;
    for (char c : agg[i].key) { if (c == '"' || c == '\\') key += '\\'; key += c; }
    char b[768];
    snprintf(b, sizeof(b), "%s{\"kernel\": \"%s\", \"launches\": %d, \"total_us\": %.3f, \"flops\": %.6e}", i ? ", " : "", key.c_str(), agg[i].n, agg[i].us, agg[i].flops);
    out += b;
  }
  out += "]";
  if (dropped) { p.recs.clear(); (void)hipGetLastError(); return fail("profile: " + std::to_string(dropped) + " launch records could not be read"); }
  if (report && cap > 0) {
    if ((int)out.size() + 1 > cap) return fail("profile: report buffer too small");
    memcpy(report, out.c_str(), out.size() + 1);
  }
  p.recs.clear();
#endif
  return 0;
}
int p5_is_emulator(void) {
#ifdef P5_EMU
  return 1;
#else
  return 0;
#endif
}

int p5_engine_create(const P5Config* cfg, P5Engine** out) {
  P5_REQUIRE(cfg && out, "null argument");
  P5_REQUIRE(cfg->d_kv == 64, "d_kv must be 64 (every T5 checkpoint)");
  P5_REQUIRE(cfg->d_model % 64 == 0 && cfg->d_model <= 1024, "d_model must be a multiple of 64, <= 1024");
  P5_REQUIRE(cfg->d_ff % 64 == 0, "d_ff must be a multiple of 64");
  P5_REQUIRE(cfg->n_enc_layers >= 1 && cfg->n_enc_layers <= 64 && cfg->n_dec_layers >= 1 && cfg->n_dec_layers <= 64, "layer count");
  P5_REQUIRE(cfg->dtype == 0 || cfg->dtype == 1, "dtype must be 0 (fp32) or 1 (bf16)");
  P5_REQUIRE(cfg->rel_buckets >= 2 && cfg->rel_buckets <= 64, "relative_attention_num_buckets must be <= 64");
  P5Engine* e = new P5Engine();
  e->c = *cfg;
  e->inner = cfg->n_heads * cfg->d_kv;
  build_layout(e);
  *out = e;
  return 0;
}
int p5_engine_destroy(P5Engine* e) {
  if (!e) return 0;
#ifndef P5_EMU
  for (int i = 0; i < P5_MAX_STAGED; ++i) {
    if (e->st_ev[i]) hipEventDestroy(e->st_ev[i]);
    if (e->st_ev_side[i]) hipEventDestroy(e->st_ev_side[i]);
  }
  if (e->zg_ev) hipEventDestroy(e->zg_ev);
  if (e->tr_ev) hipEventDestroy(e->tr_ev);
  for (int i = 0; i < 3; ++i) if (e->gen_ev[i]) hipEventDestroy(e->gen_ev[i]);
  if (e->side_events) {
    for (int i = 0; i < 32; ++i) hipEventDestroy(e->ev_pool[i]);
    for (int i = 0; i < P5_NSETS; ++i) hipEventDestroy(e->set_ev[i]);
    hipEventDestroy(e->head_wg_ev);
    for (int i = 0; i < 64; ++i) hipEventDestroy(e->kv_ev[i]);
  }
#endif
  delete e->ver;
  delete e;
  return 0;
}
int64_t p5_param_count(const P5Engine* e) { return e->n_params; }
int p5_param_table(const P5Engine* e, int idx, char* name, int name_cap, int64_t* offset, int* rows, int* cols) {
  if (idx < 0 || idx >= (int)e->table.size()) return 1;
  const ParamInfo& p = e->table[idx];
  snprintf(name, name_cap, "%s", p.name.c_str());
  *offset = p.off; *rows = p.rows; *cols = p.cols;
  return 0;
}
int p5_engine_bind(P5Engine* e, float* params, float* grads, void* shadow, const int* lut_enc, const int* lut_dec, int lut_half,
                   uint32_t* rng_state) {
  P5_REQUIRE(params && lut_enc && lut_dec, "null argument");
  P5_REQUIRE(e->c.dtype == 0 || shadow, "bf16 mode needs a shadow arena");
  P5_REQUIRE(lut_half >= 511, "bucket LUT must cover |rel| <= 511");
  e->P = params; e->G = grads; e->S = shadow; e->lut_enc = lut_enc; e->lut_dec = lut_dec; e->lut_half = lut_half; e->rng = rng_state;
  return 0;
}

// buffer layout: [W^T copy: n_params bf16][256-byte aligned descriptor table][256-byte aligned folded copy W diag(ln): n_params bf16]
static size_t tr_table_off(const P5Engine* e) { return ((size_t)e->n_params * 2 + 255) & ~(size_t)255; }
static size_t tr_fold_off(const P5Engine* e) { return (tr_table_off(e) + e->tr_list.size() * sizeof(P5TrDesc) + 255) & ~(size_t)255; }
int64_t p5_transposed_bytes(const P5Engine* e) { return (int64_t)(tr_fold_off(e) + (size_t)e->n_params * 2 + 256); }
int p5_engine_bind_transposed(P5Engine* e, void* buf, void* stream) {
  e->St = buf;
  e->Sf = nullptr;
  if (!buf) return 0;
  P5_REQUIRE(e->c.dtype == 1, "the transposed weight copy serves the bf16 mode only");
  // the descriptor table lives behind the copy itself (the library allocates nothing)
  std::vector<P5TrDesc> tab;
  int at0 = 0;
  for (auto& t : e->tr_list) {
    P5TrDesc q;
    memset(&q, 0, sizeof(q));
    q.off = t.off; q.rows = t.rows; q.cols = t.cols; q.tile0 = t.tile0; q.ln_off = t.ln_off; q.atile0 = at0;
    at0 += ((t.rows + 63) / 64) * ((t.cols + 255) / 256);
    tab.push_back(q);
  }
  e->adam_tiles = at0;
  char* at = (char*)buf + tr_table_off(e);
  e->Sf = (char*)buf + tr_fold_off(e);
#ifndef P5_EMU
  P5_REQUIRE(hipMemcpyAsync(at, tab.data(), tab.size() * sizeof(P5TrDesc), hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess, "descriptor upload");
  hipStreamSynchronize((hipStream_t)stream);      // (tab is a host temporary; one-time set-up call)
  if (!e->tr_ev) hipEventCreateWithFlags(&e->tr_ev, hipEventDisableTiming);
#else
  memcpy(at, tab.data(), tab.size() * sizeof(P5TrDesc));
#endif
  return 0;
}
// clip + AdamW over the ENGINE's arenas; with the transposed / folded copies bound (bf16 training) the update writes them too and the
// caller need not call p5_refresh_transposed.  *copies_fresh = 1 when it did.  Otherwise identical to p5_adamw_step(P, G, m, v, S, n, ...).
int p5_engine_adamw_step(P5Engine* e, float* m, float* v, const float* sumsq, double max_norm, double grad_scale, double lr, double beta1,
                         double beta2, double eps, double weight_decay, int step_t, int* copies_fresh, void* stream) {
  P5_REQUIRE(e->P && e->G && m && v, "p5_engine_adamw_step: arenas not bound");
  if (copies_fresh) *copies_fresh = 0;
  const bool tiles = g_opt_adam_tiles != 0 && e->c.dtype == 1 && e->St && e->S && !e->side;
  if (!tiles) return p5_adamw_step(e->P, e->G, m, v, e->S, e->n_params, sumsq, max_norm, grad_scale, lr, beta1, beta2, eps, weight_decay, step_t, stream);
  P5AdamTileArgs t;
  P5AdamArgs& a = t.a;
  a.p = e->P; a.g = e->G; a.m = m; a.v = v; a.shadow = e->S; a.sumsq = sumsq; a.n = (size_t)e->n_params;
  a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps; a.max_norm = (float)max_norm; a.grad_scale = (float)grad_scale;
  const double bc1 = 1.0 - pow(beta1, (double)step_t), bc2 = 1.0 - pow(beta2, (double)step_t);
  a.step_size = (float)(lr * sqrt(bc2) / bc1);
  a.decay = (float)(lr * weight_decay);
  t.tab = (const P5TrDesc*)((char*)e->St + tr_table_off(e));
  t.ndesc = (int)e->tr_list.size(); t.ntiles = e->adam_tiles;
  t.St = (bf16*)e->St; t.Sf = (bf16*)e->Sf;
  t.flat_n = (size_t)e->off_small_end;
  hipStream_t s = (hipStream_t)stream;
  P5_LAUNCH(p5_adamw_tiles_kernel, dim3(e->adam_tiles + 1024), dim3(256), 0, s, t);
  P5_TRY(P5_KCHECK());
  {
    const P5Config& c = e->c;
    P5ZeroTab tab;
    tab.n = 0;
    int blocks = 0;
    auto add = [&](int64_t off, int64_t count) {
      P5ZeroTab::D& q = tab.e[tab.n++];
      q.off = off; q.count = (int)count; q.blk0 = blocks;
      blocks += (int)((count + 8191) / 8192);
    };
    P5_REQUIRE(2 * c.n_enc_layers + 3 * c.n_dec_layers + 2 < 200, "p5_engine_adamw_step: too many norm segments");
    for (const LayerOff& l : e->enc) { add(l.sa.ln, c.d_model); add(l.ff_ln, c.d_model); }
    for (const LayerOff& l : e->dec) { add(l.sa.ln, c.d_model); add(l.ca.ln, c.d_model); add(l.ff_ln, c.d_model); }
    add(e->off_enc_fln, c.d_model);
    add(e->off_dec_fln, c.d_model);
    P5_LAUNCH(p5_adamw_segments_kernel, dim3(blocks), dim3(256), 0, s, a, tab);
    P5_TRY(P5_KCHECK());
  }
  e->tr_pending = false;       // (same stream as the next forward / backward: nothing to wait for)
  if (copies_fresh) *copies_fresh = 1;
  return 0;
}
// Rebuild the transposed copy from the bf16 shadow (call after every parameter update, e.g. right after p5_adamw_step).  With a
// side stream bound it runs there, behind everything enqueued on `stream` so far; the next backward waits for it -- the
// forward in between does not, so the ~0.2 GB of copies overlap it.
int p5_refresh_transposed(P5Engine* e, void* stream) {
  P5_REQUIRE(e->St && e->S, "transposed copy / shadow not bound");
  hipStream_t main = (hipStream_t)stream;
  hipStream_t s = main;
#ifndef P5_EMU
  if (e->side) { fork_to_side(e, main); s = e->side; }
#endif
  const P5TrDesc* tab = (const P5TrDesc*)((char*)e->St + tr_table_off(e));
  P5_LAUNCH(p5_transpose_blocks_kernel, dim3(e->tr_tiles), dim3(256), 0, s, (bf16*)e->St, (const bf16*)e->S, tab, (int)e->tr_list.size());
  P5_TRY(P5_KCHECK());
#ifndef P5_EMU
  if (e->tr_ev) hipEventRecord(e->tr_ev, s);       // (W^T is first read by the backward; the folded copy below by the very next forward)
#endif
  s = main;          // the folded copy is read by the very next forward: always on the caller's stream
  if (e->Sf) {
    // W diag(ln) of every projection that consumes a T5LayerNorm output (q/k/v, wi, cross-attention q), from the fp32 masters, at the
    // weights' own arena offsets -- what the training forward multiplies the raw residual stream with (norm_fused)
    const P5Config& c = e->c;
    const int d = c.d_model, in = e->inner;
    const int wi_rows = (c.gated_gelu ? 2 : 1) * c.d_ff;
    P5FoldTab tab;
    tab.n = 0; tab.d = d;
    int blocks = 0;
    auto add = [&](int64_t w_off, int64_t ln_off, int rows) {
      P5FoldTab::D& q = tab.e[tab.n++];
      q.w_off = w_off; q.ln_off = ln_off; q.rows = rows; q.blk0 = blocks;
      blocks += (rows + 7) / 8;
    };
    P5_REQUIRE(2 * c.n_enc_layers + 3 * c.n_dec_layers <= 160, "fold table");
    for (int i = 0; i < c.n_enc_layers; ++i) { add(e->enc[i].sa.q, e->enc[i].sa.ln, 3 * in); add(e->enc[i].wi, e->enc[i].ff_ln, wi_rows); }
    for (int i = 0; i < c.n_dec_layers; ++i) {
      add(e->dec[i].sa.q, e->dec[i].sa.ln, 3 * in); add(e->dec[i].ca.q, e->dec[i].ca.ln, in); add(e->dec[i].wi, e->dec[i].ff_ln, wi_rows);
    }
    P5_LAUNCH(p5_fold_rows_kernel, dim3(blocks), dim3(256), 0, s, (bf16*)e->Sf, (const float*)e->P, tab);
    P5_TRY(P5_KCHECK());
  }
  e->tr_pending = true;
  return 0;
}

int p5_refresh_shadow(P5Engine* e, void* stream) {
  if (e->c.dtype != 1) return 0;
  const size_t n = (size_t)e->n_params;
  P5_LAUNCH((p5_cast_kernel<bf16>), dim3(2048), dim3(256), 0, (hipStream_t)stream, (bf16*)e->S, (const float*)e->P, n);
  return P5_KCHECK();
}

// ---- several targets per user: labels [B, G, T] against ONE encoder pass per user (p5_forward_targets, include/p5hip.h) ----
// the row limit of the decoder side: the norm-backward epilogue's partial table (dw_scratch) holds 1024 blocks of 64 rows per norm
static constexpr int64_t P5_MAX_DEC_ROWS = 1024 * 64;
int64_t p5_train_workspace_bytes_targets(const P5Engine* e, int B, int L, int T, int G) {
  if (G < 1) return 0;
  P5Engine tmp = *e;
  return layout_ws(&tmp, nullptr, B, L, T, true, G);
}
int64_t p5_train_workspace_bytes(const P5Engine* e, int B, int L, int T) { return p5_train_workspace_bytes_targets(e, B, L, T, 1); }

// both kernels of p5_clip.h behind a per-token NLL: the seeds, the users' partials, then loss / terms / stats
static int launch_clip(hipStream_t s, float* loss, float* terms, float* seed, float* partials, float* stats, const float* nll, const float* old_lp,
                       const int64_t* out_attn, const int64_t* labels, const float* tw, const int* mode, const float* ent, const float* kl,
                       float entropy_coef, float kl_coef, float eps_low, float eps_high, int ratio_mode, int B, int G, int T) {
  P5ClipArgs a;
  a.nll = nll; a.old_lp = old_lp; a.out_attn = out_attn; a.labels = labels; a.tw = tw; a.mode = mode; a.ent = ent; a.kl = ent ? kl : nullptr;
  a.seed = seed; a.partials = partials; a.G = G; a.T = T; a.ratio_mode = ratio_mode; a.rows = B * G * T;
  a.lo = 1.0f - eps_low; a.hi = 1.0f + eps_high; a.gscale = 1.0f / (float)(B * G); a.entropy_coef = entropy_coef; a.kl_coef = kl_coef;
  P5_LAUNCH(p5_clip_objective_kernel, dim3(B), dim3(256), 0, s, a);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_clip_finish_kernel, dim3(1), dim3(256), 0, s, loss, terms, stats, (const float*)partials, B, B * G, ent ? 1 : 0, entropy_coef, kl_coef);
  return P5_KCHECK();
}
static int clip_params_ok(float eps_low, float eps_high, int ratio_mode) {
  P5_REQUIRE(eps_low - eps_low == 0.f && eps_high - eps_high == 0.f && eps_low >= 0.f && eps_high >= 0.f,
             "clip objective: eps_low / eps_high must be finite and >= 0");
  P5_REQUIRE(ratio_mode == P5_RATIO_TOKEN || ratio_mode == P5_RATIO_SEQUENCE, "clip objective: unknown ratio mode (0 token, 1 sequence)");
  return 0;
}
// both kernels of p5_pref.h behind a per-token NLL: the seeds and the users' partials, then loss / stats
static int launch_pref(hipStream_t s, float* loss, float* seed, float* partials, float* stats, const float* nll, const float* ref_lp,
                       const int64_t* out_attn, const int64_t* labels, const int* pref_mask, int kind, float beta, int depth, int length_normalize,
                       float sft_coef, int B, int G, int T) {
  P5PrefArgs a;
  a.nll = nll; a.ref_lp = ref_lp; a.out_attn = out_attn; a.labels = labels; a.pref_mask = pref_mask; a.seed = seed; a.partials = partials;
  a.G = G; a.T = T; a.kind = kind; a.depth = depth; a.length_normalize = length_normalize ? 1 : 0;
  a.beta = beta; a.sft_coef = sft_coef; a.inv_b = 1.0f / (float)B;
  P5_LAUNCH(p5_pref_objective_kernel, dim3(B), dim3(256), 0, s, a);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_pref_finish_kernel, dim3(1), dim3(256), 0, s, loss, stats, (const float*)partials, B);
  return P5_KCHECK();
}
static int pref_params_ok(int kind, float beta, int depth, float sft_coef) {
  P5_REQUIRE(beta - beta == 0.f && beta > 0.f, "preference objective: beta must be finite and > 0");
  P5_REQUIRE(kind == P5_PREF_PL || kind == P5_PREF_IPO, "preference objective: unknown kind (0 Plackett-Luce, 1 IPO)");
  P5_REQUIRE(depth >= 0, "preference objective: depth >= 0 (0 = full depth)");
  P5_REQUIRE(sft_coef - sft_coef == 0.f, "preference objective: sft_coef must be finite");
  return 0;
}
static int forward_targets(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, const int64_t* labels,
                           int B, int L, int T, int G, int training, float* nll_out, void* ws, int64_t ws_bytes, void* stream, bool with_loss) {
  e->clip = e->clip_next;        // one-shot, whatever this call returns
  e->clip_next.on = false;
  if (e->clip.on && !with_loss) {
    e->clip.on = false;
    P5_REQUIRE(false, "p5_forward / p5_forward_targets: a clip objective is armed (p5_train_set_clip_objective): it needs p5_forward_loss / p5_forward_loss_targets");
  }
  e->pref = e->pref_next;        // one-shot, whatever this call returns
  e->pref_next.on = false;
  if (e->pref.on && !with_loss) {
    e->pref.on = false;
    P5_REQUIRE(false, "p5_forward / p5_forward_targets: a preference objective is armed (p5_train_set_pref_objective): it needs p5_forward_loss_targets");
  }
  if (e->pref.on && e->clip.on) {
    e->pref.on = e->clip.on = false;
    P5_REQUIRE(false, "preference objective: the clip objective is armed as well (p5_train_set_clip_objective): one objective per forward");
  }
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(B >= 1 && L >= 1 && L <= 512 && T >= 1 && T <= 512, "shape limits: 1 <= L,T <= 512");
  P5_REQUIRE(G >= 1, "targets per user: G >= 1");
  if (G > 1) {
    P5_REQUIRE((int64_t)G * T <= 512, "targets per user: G * T <= 512 (the cross-attention kernels' query limit)");
    P5_REQUIRE((int64_t)B * G * T <= P5_MAX_DEC_ROWS, "targets per user: B * G * T <= 65536 decoder rows");
    // (decoder self-attention launches put one entry per (sequence, head) in gridDim.y: p5_attn_tu.hip)
    P5_REQUIRE((int64_t)B * G * e->c.n_heads <= 65535, "targets per user: B * G * n_heads <= 65535 (a launch grid's y extent)");
  }
  const int64_t need = layout_ws(e, (char*)ws, B, L, T, true, G);
  P5_REQUIRE(ws_bytes >= need, "workspace too small");
  P5_REQUIRE(((uintptr_t)ws % 256) == 0, "workspace must be 256-byte aligned");
  e->B = B; e->Gt = G; e->Bd = B * G; e->L = L; e->T = T; e->M = B * L; e->Md = B * G * T; e->training = training;
  e->Vp = (e->c.vocab_size + 63) / 64 * 64;
  e->ids = input_ids; e->ww = whole_word_ids; e->mask = attention_mask; e->labels = labels; e->out_attn = nullptr; e->tgt_w = nullptr;
  e->ce_g_ready = false;
  if (training && e->c.dropout > 0.f) P5_REQUIRE(e->rng, "training with dropout needs rng_state");
  e->il = e->il_next;            // one-shot: this forward and the backward behind it
  e->il_next.on = false;
  e->il.tr.group = G;            // (the excluded-node bitmap is per USER: sample b * G + g reads row b)
  e->il.tr.tw = nullptr;
  if (e->il.on) P5_REQUIRE(nll_out, "item loss: nll_out");
  if (e->clip.on) {
    P5_REQUIRE(nll_out, "clip objective: nll_out");
    P5_REQUIRE(!(e->il.on && e->il.trunc), "clip objective: not built for the truncated item loss (top_k / top_p): the kept set may differ between the two policies");
  }
  if (e->pref.on) {
    P5_REQUIRE(nll_out, "preference objective: nll_out");
    P5_REQUIRE(G <= P5_PREF_MAX_G, "preference objective: G <= 512");
    P5_REQUIRE(!(e->il.on && e->il.trunc), "preference objective: not built for the truncated item loss (top_k / top_p): the kept set may differ between the two policies");
    P5_REQUIRE(!(e->il.on && e->il.reg), "preference objective: not built beside the item regularizers (p5_train_set_item_regularizers)");
  }
  return e->c.dtype == 1 ? forward_impl<bf16>(e, nll_out, (hipStream_t)stream) : forward_impl<float>(e, nll_out, (hipStream_t)stream);
}
int p5_forward_targets(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, const int64_t* labels,
                       int B, int L, int T, int G, int training, float* nll_out, void* ws, int64_t ws_bytes, void* stream) {
  return forward_targets(e, input_ids, whole_word_ids, attention_mask, labels, B, L, T, G, training, nll_out, ws, ws_bytes, stream, false);
}
int p5_forward(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, const int64_t* labels,
               int B, int L, int T, int training, float* nll_out, void* ws, int64_t ws_bytes, void* stream) {
  return p5_forward_targets(e, input_ids, whole_word_ids, attention_mask, labels, B, L, T, 1, training, nll_out, ws, ws_bytes, stream);
}
int p5_forward_loss_targets(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, const int64_t* labels,
                            const int64_t* output_attention, int B, int L, int T, int G, const float* target_weights, int training, float* nll_out,
                            float* loss_out, void* ws, int64_t ws_bytes, void* stream) {
  if (!(output_attention && loss_out)) e->clip_next.on = e->pref_next.on = false;     // (one-shot, refused calls included)
  P5_REQUIRE(output_attention && loss_out, "null argument");
  if (e->pref_next.on && target_weights) {
    e->pref_next.on = e->clip_next.on = false;
    P5_REQUIRE(false, "preference objective: target_weights must be NULL (the objective forms every target's weight itself)");
  }
  {
    const int rc = forward_targets(e, input_ids, whole_word_ids, attention_mask, labels, B, L, T, G, training, nll_out, ws, ws_bytes, stream, true);
    if (rc) { e->clip.on = e->pref.on = false; return rc; }
  }
  e->out_attn = output_attention;
  e->tgt_w = target_weights;
  e->il.tr.tw = target_weights;
  if (e->clip.on) {
    // the clipped objective in the loss kernels' place: it writes the seeds of the backward behind this call
    const bool reg = e->il.on && e->il.reg;
    const float* rt = reg ? e->il.row_terms : nullptr;
    return launch_clip((hipStream_t)stream, loss_out, reg ? e->il.terms_out : nullptr, e->clip.seed, e->clip.partials, e->clip.stats, (const float*)nll_out,
                       e->clip.old_lp, output_attention, e->labels, target_weights, e->clip.mode, rt, reg && e->il.ref ? rt + e->Md : nullptr,
                       reg ? e->il.ent_coef : 0.f, reg ? e->il.kl_coef : 0.f, e->clip.eps_low, e->clip.eps_high, e->clip.ratio_mode, B, G, T);
  }
  if (e->pref.on)      // the preference objective in the loss kernels' place: it writes the seeds of the backward behind this call
    return launch_pref((hipStream_t)stream, loss_out, e->pref.seed, e->pref.partials, e->pref.stats, (const float*)nll_out, e->pref.ref_lp, output_attention,
                       e->labels, e->pref.mask, e->pref.kind, e->pref.beta, e->pref.depth, e->pref.length_normalize, e->pref.sft_coef, B, G, T);
  if (e->il.on && e->il.reg) {
    const float* rt = e->il.row_terms;
    P5_LAUNCH(p5_trie_reg_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss_out, e->il.terms_out, (const float*)nll_out, rt,
              e->il.ref ? rt + e->Md : (const float*)nullptr, output_attention, B * G, T, target_weights, e->il.ent_coef, e->il.kl_coef);
    return P5_KCHECK();
  }
  if (g_opt_loss_fuse && training && e->ce_free_fwd && nll_out) {
    // the backward behind this call (dnll == nullptr) scales by exactly this mask and these weights: its NLL gradients are written here
    P5_LAUNCH(p5_masked_mean_g_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss_out, e->ce_g, (const float*)nll_out, output_attention, e->labels, B * G, T,
              1.0f / (float)e->Bd, target_weights);
    P5_TRY(P5_KCHECK());
    e->ce_g_ready = true;
    return 0;
  }
  P5_LAUNCH(p5_masked_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss_out, (const float*)nll_out, output_attention, B * G, T, target_weights);
  return P5_KCHECK();
}
int p5_forward_loss(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, const int64_t* labels,
                    const int64_t* output_attention, int B, int L, int T, int training, float* nll_out, float* loss_out, void* ws, int64_t ws_bytes,
                    void* stream) {
  return p5_forward_loss_targets(e, input_ids, whole_word_ids, attention_mask, labels, output_attention, B, L, T, 1, nullptr, training, nll_out, loss_out,
                                 ws, ws_bytes, stream);
}
int p5_train_set_item_loss(P5Engine* e, const int* child_off, const int* child_tok, const int* child_node, int n_nodes, const uint32_t* excluded_nodes,
                           int excluded_words, float temperature, int* row_state_out) {
  e->il_next.on = false;
  e->il_next.head = false;        // (the restricted head is armed behind this call, every time: p5_train_set_item_head)
  e->il_next.reg = false;         // (and so are the regularisers: p5_train_set_item_regularizers)
  P5_REQUIRE(child_off && child_tok && child_node && n_nodes >= 1, "item loss: trie (child_off / child_tok / child_node, n_nodes >= 1)");
  P5_REQUIRE(temperature > 0.f && temperature < __builtin_huge_valf(), "item loss: temperature > 0");
  P5_REQUIRE(excluded_words >= 0 && (excluded_nodes || excluded_words == 0), "item loss: excluded_nodes / excluded_words");
  P5_REQUIRE(!excluded_nodes || (int64_t)excluded_words * 32 >= n_nodes, "item loss: the excluded-node bitmap is shorter than the trie");
  e->il_next.tr = P5TrieCe{child_off, child_tok, child_node, excluded_words > 0 ? excluded_nodes : nullptr, excluded_words, temperature};
  e->il_next.state_out = row_state_out;
  e->il_next.trunc = false;
  e->il_next.on = true;
  return 0;
}
int p5_train_set_item_loss_truncated(P5Engine* e, const int* child_off, const int* child_tok, const int* child_node, int n_nodes,
                                     const uint32_t* excluded_nodes, int excluded_words, float temperature, int* row_state_out, int top_k, float top_p,
                                     float* row_cut) {
  e->il_next.on = false;
  P5_REQUIRE(top_k >= 0, "item loss: top_k >= 0 (0 = off)");
  P5_REQUIRE(top_p > 0.f && top_p <= 1.f, "item loss: 0 < top_p <= 1 (1 = off)");
  P5_REQUIRE(row_cut, "item loss: row_cut (device, one fp32 per decoder row)");
  P5_TRY(p5_train_set_item_loss(e, child_off, child_tok, child_node, n_nodes, excluded_nodes, excluded_words, temperature, row_state_out));
  e->il_next.trunc = top_k > 0 || top_p < 1.f;          // (off: the plain kernels, bit for bit; row_cut is not written then)
  e->il_next.tc = P5TruncCe{top_k, top_p};
  e->il_next.row_cut = row_cut;
  return 0;
}
size_t p5_item_head_workspace_bytes(const P5Engine* e, int B, int T, int n_tokens) {
  if (B < 1 || T < 1 || n_tokens < 1) return 0;
  return item_head_layout(e, nullptr, (size_t)B * T, ((size_t)n_tokens + 63) / 64 * 64, nullptr);
}
int p5_train_set_item_head(P5Engine* e, const int* head_tokens, int n_tokens, const int* child_col, void* ws, size_t ws_bytes) {
  e->il_next.head = false;
  e->il_next.tr.col = nullptr;
  P5_REQUIRE(e->il_next.on, "item head: no item loss is armed (call p5_train_set_item_loss / _truncated first)");
  P5_REQUIRE(n_tokens >= 1 && n_tokens <= e->c.vocab_size, "item head: n_tokens must lie in [1, vocab_size]");
  P5_REQUIRE(head_tokens && child_col && ws, "item head: head_tokens / child_col / ws");
  P5_REQUIRE(((uintptr_t)ws % 256) == 0, "item head: workspace must be 256-byte aligned");
  // (the forward knows the batch and checks the exact size; this is the part that does not depend on it)
  P5_REQUIRE(ws_bytes >= p5_item_head_workspace_bytes(e, 1, 1, n_tokens), "item head: workspace too small (p5_item_head_workspace_bytes)");
  P5Engine::ItemLoss& h = e->il_next;
  h.head_tok = head_tokens; h.Nu = n_tokens; h.Nup = (n_tokens + 63) / 64 * 64;
  h.head_ws = ws; h.head_ws_bytes = ws_bytes;
  h.tr.col = child_col;
  h.head = true;
  return 0;
}
int p5_train_set_item_regularizers(P5Engine* e, const float* ref_logits, int ld_ref, float* row_terms, float entropy_coef, float kl_coef,
                                   float* terms_out) {
  e->il_next.reg = false;
  P5_REQUIRE(e->il_next.on, "item regularizers: no item loss is armed (call p5_train_set_item_loss first)");
  P5_REQUIRE(!e->il_next.trunc, "item regularizers: not built for the truncated item loss (top_k / top_p)");
  P5_REQUIRE(row_terms, "item regularizers: row_terms (device, three fp32 per decoder row)");
  P5_REQUIRE(entropy_coef - entropy_coef == 0.f && kl_coef - kl_coef == 0.f, "item regularizers: entropy_coef / kl_coef must be finite");
  const int cols = e->il_next.head ? e->il_next.Nu : e->c.vocab_size;
  P5_REQUIRE(!ref_logits || ld_ref >= cols, "item regularizers: ld_ref is smaller than the head's columns (vocab_size, or the trie's tokens)");
  P5Engine::ItemLoss& h = e->il_next;
  h.ref = ref_logits; h.ld_ref = ref_logits ? ld_ref : 0; h.row_terms = row_terms; h.ent_coef = entropy_coef; h.kl_coef = kl_coef;
  h.terms_out = terms_out;
  h.reg = true;
  return 0;
}
int p5_train_set_clip_objective(P5Engine* e, const float* old_logprobs, const int* target_mode, float eps_low, float eps_high, int ratio_mode,
                                float* row_seed, float* user_partials, float* clip_stats) {
  e->clip_next.on = false;
  P5_TRY(clip_params_ok(eps_low, eps_high, ratio_mode));
  P5_REQUIRE(old_logprobs && row_seed && user_partials && clip_stats,
             "clip objective: null pointer (old_logprobs, row_seed, user_partials and clip_stats are required)");
  P5_REQUIRE(!(e->il_next.on && e->il_next.trunc),
             "clip objective: not built for the truncated item loss (top_k / top_p): the kept set may differ between the two policies");
  e->clip_next.old_lp = old_logprobs; e->clip_next.mode = target_mode; e->clip_next.eps_low = eps_low; e->clip_next.eps_high = eps_high;
  e->clip_next.ratio_mode = ratio_mode; e->clip_next.seed = row_seed; e->clip_next.partials = user_partials; e->clip_next.stats = clip_stats;
  e->clip_next.on = true;
  return 0;
}
int p5_train_set_pref_objective(P5Engine* e, const float* ref_logprobs, const int* pref_mask, int kind, float beta, int depth, int length_normalize,
                                float sft_coef, float* row_seed, float* user_partials, float* pref_stats) {
  e->pref_next.on = false;
  P5_TRY(pref_params_ok(kind, beta, depth, sft_coef));
  P5_REQUIRE(row_seed && user_partials && pref_stats, "preference objective: null pointer (row_seed, user_partials and pref_stats are required)");
  P5_REQUIRE(!e->clip_next.on, "preference objective: the clip objective is armed as well (p5_train_set_clip_objective): one objective per forward");
  P5_REQUIRE(!(e->il_next.on && e->il_next.reg), "preference objective: not built beside the item regularizers (p5_train_set_item_regularizers)");
  P5_REQUIRE(!(e->il_next.on && e->il_next.trunc),
             "preference objective: not built for the truncated item loss (top_k / top_p): the kept set may differ between the two policies");
  P5Engine::PrefObj& p = e->pref_next;
  p.ref_lp = ref_logprobs; p.mask = pref_mask; p.kind = kind; p.beta = beta; p.depth = depth; p.length_normalize = length_normalize ? 1 : 0;
  p.sft_coef = sft_coef; p.seed = row_seed; p.partials = user_partials; p.stats = pref_stats;
  p.on = true;
  return 0;
}
int p5_backward_set_item_grads(P5Engine* e, const float* d_entropy, const float* d_kl) {
  e->bw_dH = e->bw_dKL = nullptr;
  P5_REQUIRE(e->Md > 0 && e->il.on && e->il.reg, "item grads: the last forward ran without item regularizers (p5_train_set_item_regularizers)");
  e->bw_dH = d_entropy;
  e->bw_dKL = d_kl;
  return 0;
}
int p5_train_last_item_logits(const P5Engine* e, const float** ptr, int* rows, int* ld, int* cols) {
  P5_REQUIRE(ptr && rows && ld && cols, "last item logits: null argument");
  P5_REQUIRE(e->Md > 0 && e->il.on, "last item logits: the last forward ran without an item loss (p5_train_set_item_loss)");
  const bool hd = e->il.head;
  *ptr = hd ? (const float*)e->il.logitsU : (const float*)e->logits;
  *rows = e->Md; *ld = hd ? e->il.Nup : e->Vp; *cols = hd ? e->il.Nu : e->c.vocab_size;
  return 0;
}
int p5_backward_num_stages(const P5Engine* e) { return e->c.n_dec_layers + e->c.n_enc_layers + 4; }
int p5_backward_stage(P5Engine* e, const float* dnll, int stage, void* stream) {
  P5_REQUIRE(e->G, "no gradient arena bound");
  P5_REQUIRE(e->Md > 0, "p5_forward must run first");
  P5_TRY(e->c.dtype == 1 ? backward_stage_impl<bf16>(e, dnll, stage, (hipStream_t)stream)
                         : backward_stage_impl<float>(e, dnll, stage, (hipStream_t)stream));
  const bool last_stage = stage == p5_backward_num_stages(e) - 1;
  if (!e->whole_backward || last_stage) {
    // stage-by-stage callers: norm partials never stay pending; weight gradients only while a two-layer encoder group (or the
    // cross-attention K/V block that leaves with the top group) is still filling up -- p5_backward_final_range reports a range only
    // once everything inside it has been launched
    if (!e->stage_pairs || last_stage) P5_TRY(wgrad_flush(e, (hipStream_t)stream, false, (g_opt_wgrad_side & 2) != 0));
    P5_TRY(norm_flush(e, (hipStream_t)stream));
  }
  {
    int64_t b = 0, en = 0;
    p5_backward_stage_range(e, stage, &b, &en);
    if (stage == 0) { e->fin_b = e->fin_e = 0; }
    if (en > b) {
      if (e->fin_e <= e->fin_b) { e->fin_b = b; e->fin_e = en; }
      else { e->fin_b = b < e->fin_b ? b : e->fin_b; e->fin_e = en > e->fin_e ? en : e->fin_e; }
    }
    e->rep_b = e->rep_e = 0;
    if (e->wg_pending.empty() && e->fin_e > e->fin_b) { e->rep_b = e->fin_b; e->rep_e = e->fin_e; e->fin_b = e->fin_e = 0; }
  }
  // the side stream is now ordered after this stage's main-stream work (a bucket all-reduce enqueued behind the side
  // stream sees every gradient of the stage); after the last stage the main stream waits for the side stream
  fork_to_side(e, (hipStream_t)stream);
  if (stage == p5_backward_num_stages(e) - 1) join_side(e, (hipStream_t)stream);
  return 0;
}
// the gradient range that became FINAL with the most recent p5_backward_stage call (empty while a grouped weight-gradient launch is
// still collecting problems): contiguous, because the stages walk the arena from the back.  What a data-parallel caller all-reduces.
int p5_backward_final_range(const P5Engine* e, int64_t* begin, int64_t* end) { *begin = e->rep_b; *end = e->rep_e; return 0; }
// The whole staged backward in ONE call (round 5): every stage is enqueued back to back; whenever a gradient range becomes final an event is
// recorded behind it on `stream` and the range is noted.  A data-parallel caller then makes its communication stream wait for event k
// (p5_backward_staged_wait) and enqueues the all-reduce of range k -- the exchange still overlaps the rest of the backward on the device,
// and the host pays one library call per step instead of one per stage plus a range query each (16 + 16 at T5-small).
int p5_backward_staged(P5Engine* e, const float* dnll, void* stream, int64_t* ranges, int max_ranges, int* n_ranges) {
  P5_REQUIRE(ranges && n_ranges && max_ranges >= 1, "p5_backward_staged: ranges / n_ranges");
  const int nst = p5_backward_num_stages(e);
  int n = 0;
  for (int st = 0; st < nst; ++st) {
    P5_TRY(p5_backward_stage(e, dnll, st, stream));
    if (e->rep_e > e->rep_b) {
      P5_REQUIRE(n < max_ranges && n < P5_MAX_STAGED, "p5_backward_staged: more final ranges than the caller has room for");
#ifndef P5_EMU
      if (!e->st_ev[n]) P5_REQUIRE(hipEventCreateWithFlags(&e->st_ev[n], hipEventDisableTiming) == hipSuccess, "hipEventCreate");
      P5_REQUIRE(hipEventRecord(e->st_ev[n], (hipStream_t)stream) == hipSuccess, "hipEventRecord");
      if (e->side) {      // weight gradients of this range may have been launched on the side stream: the range is final behind BOTH events
        if (!e->st_ev_side[n]) P5_REQUIRE(hipEventCreateWithFlags(&e->st_ev_side[n], hipEventDisableTiming) == hipSuccess, "hipEventCreate");
        P5_REQUIRE(hipEventRecord(e->st_ev_side[n], e->side) == hipSuccess, "hipEventRecord");
      }
      e->st_side[n] = e->side != nullptr;
#endif
      ranges[2 * n] = e->rep_b; ranges[2 * n + 1] = e->rep_e;
      e->st_range[2 * n] = e->rep_b; e->st_range[2 * n + 1] = e->rep_e;
      ++n;
    }
  }
  e->st_n = n;
  *n_ranges = n;
  return 0;
}
int p5_backward_staged_wait(P5Engine* e, int k, void* comm_stream) {
  P5_REQUIRE(k >= 0 && k < e->st_n, "p5_backward_staged_wait: range index");
#ifndef P5_EMU
  P5_REQUIRE(hipStreamWaitEvent((hipStream_t)comm_stream, e->st_ev[k], 0) == hipSuccess, "hipStreamWaitEvent");
  if (e->st_side[k] && (hipStream_t)comm_stream != e->side)
    P5_REQUIRE(hipStreamWaitEvent((hipStream_t)comm_stream, e->st_ev_side[k], 0) == hipSuccess, "hipStreamWaitEvent");
#else
  (void)comm_stream;
#endif
  return 0;
}
// ---- the exchange itself for a caller without torch.distributed: RCCL through the ncclComm_t the caller created ----------------------
// No link-time dependency on a particular librccl: the symbols are taken from whatever RCCL the process has loaded (the one that made the
// communicator -- torch ships its own copy next to its HIP runtime, a C host links /opt/rocm/lib/librccl.so), else from librccl.so.1.
#ifndef P5_EMU
typedef int (*p5_nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*p5_nccl_errstr_fn)(int);
static p5_nccl_allreduce_fn g_nccl_allreduce = nullptr;
static p5_nccl_errstr_fn g_nccl_errstr = nullptr;
static int nccl_resolve() {
  if (g_nccl_allreduce) return 0;
  void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
  void* h = nullptr;
  if (!sym) {
    h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (h) sym = dlsym(h, "ncclAllReduce");
  }
  if (!sym) return fail("p5_allreduce: no RCCL in this process (ncclAllReduce not found; load librccl before creating the communicator)");
  g_nccl_errstr = (p5_nccl_errstr_fn)(h ? dlsym(h, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString"));
  g_nccl_allreduce = (p5_nccl_allreduce_fn)sym;
  return 0;
}
#endif
// rccl.h: ncclFloat32 = 7, ncclFloat64 = 8, ncclBfloat16 = 9, ncclInt64 = 4; ncclSum = 0
int p5_allreduce_sum(void* buf, int64_t count, int dtype, void* nccl_comm, void* stream) {
  P5_REQUIRE(buf && nccl_comm && count >= 0 && dtype >= 0 && dtype <= 3, "p5_allreduce_sum: arguments");
#ifndef P5_EMU
  P5_TRY(nccl_resolve());
  static const int kType[4] = {7, 9, 8, 4};
  const int rc = g_nccl_allreduce(buf, buf, (size_t)count, kType[dtype], 0, nccl_comm, (hipStream_t)stream);
  if (rc != 0) return fail(std::string("ncclAllReduce: ") + (g_nccl_errstr ? g_nccl_errstr(rc) : "error ") + " (" + std::to_string(rc) + ")");
  return 0;
#else
  (void)stream;
  return fail("p5_allreduce_sum: the host emulation has no RCCL");
#endif
}
// bf16 -> fp32 of an exchanged bucket
__global__ __launch_bounds__(256) void p5_widen_kernel(float* __restrict__ out, const bf16* __restrict__ in, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = to_f<bf16>(in[i]);
}
int p5_allreduce_range(P5Engine* e, int k, void* nccl_comm, void* bf16_scratch, void* comm_stream) {
  P5_REQUIRE(k >= 0 && k < e->st_n, "p5_allreduce_range: range index (call p5_backward_staged first)");
  P5_REQUIRE(e->G != nullptr, "p5_allreduce_range: no gradient arena bound");
  P5_TRY(p5_backward_staged_wait(e, k, comm_stream));
  const int64_t b = e->st_range[2 * k], n = e->st_range[2 * k + 1] - b;
  if (n <= 0) return 0;
  hipStream_t cs = (hipStream_t)comm_stream;
  if (!bf16_scratch) return p5_allreduce_sum(e->G + b, n, 0, nccl_comm, comm_stream);
  const unsigned blocks = (unsigned)((n / 8 + 255) / 256 > 4096 ? 4096 : (n / 8 + 255) / 256 + 1);
  P5_LAUNCH((p5_cast_kernel<bf16>), dim3(blocks), dim3(256), 0, cs, (bf16*)bf16_scratch, (const float*)(e->G + b), (size_t)n);
  P5_TRY(P5_KCHECK());
  P5_TRY(p5_allreduce_sum(bf16_scratch, n, 1, nccl_comm, comm_stream));
  P5_LAUNCH(p5_widen_kernel, dim3(blocks), dim3(256), 0, cs, e->G + b, (const bf16*)bf16_scratch, (size_t)n);
  return P5_KCHECK();
}
int p5_backward_stage_pairs(P5Engine* e, int on) { e->stage_pairs = on != 0; return 0; }
int p5_engine_grads_zeroed(P5Engine* e) { e->grads_keep = true; return 0; }
// zero_grad(set_to_none=True) of the reference loop: the gradients are dead until the next backward rewrites them -- nothing to do
// on the device (the next backward stores / clears what it needs); p5_engine_clear_grads is the eager form (set_to_none=False)
int p5_engine_discard_grads(P5Engine* e) { e->grads_zeroed = false; e->grads_keep = false; return 0; }

// zero_grad() of the reference loop (DistributedRunner.py:93): the 4 B x n_params fill is HBM-bound and nothing before the next
// backward needs its result, so it goes to the side stream (ordered after everything `stream` has been given so far, i.e. after
// the optimizer read the gradients) and overlaps the next forward; backward stage 0 waits for it.
int p5_engine_clear_grads(P5Engine* e, void* stream) {
  P5_REQUIRE(e->G, "engine not bound");
  hipStream_t main = (hipStream_t)stream, s = main;
#ifndef P5_EMU
  if (e->side) { fork_to_side(e, main); s = e->side; }
#endif
  if (hipMemsetAsync(e->G, 0, (size_t)e->n_params * 4, s) != 0) return fail("clear_grads: hipMemsetAsync failed");
#ifndef P5_EMU
  if (s != main) {
    if (!e->zg_ev) hipEventCreateWithFlags(&e->zg_ev, hipEventDisableTiming);
    hipEventRecord(e->zg_ev, s);
    e->zg_pending = true;
  }
#endif
  e->grads_zeroed = true;
  return 0;
}
int p5_engine_set_side_stream(P5Engine* e, void* side_stream) {
#ifndef P5_EMU
  if (side_stream && !e->side_events) {
    e->side_events = true;
    for (int i = 0; i < 32; ++i) hipEventCreateWithFlags(&e->ev_pool[i], hipEventDisableTiming);
    for (int i = 0; i < P5_NSETS; ++i) hipEventCreateWithFlags(&e->set_ev[i], hipEventDisableTiming);
    hipEventCreateWithFlags(&e->head_wg_ev, hipEventDisableTiming);
    for (int i = 0; i < 64; ++i) hipEventCreateWithFlags(&e->kv_ev[i], hipEventDisableTiming);
  }
  e->side = (hipStream_t)side_stream;
#else
  (void)e; (void)side_stream;
#endif
  return 0;
}
int p5_backward(P5Engine* e, const float* dnll, void* stream) {
  const int n = p5_backward_num_stages(e);
  e->whole_backward = true;       // nobody consumes per-stage gradient ranges: weight gradients may be grouped across stages
  int rc = 0;
  for (int s = 0; s < n && rc == 0; ++s) rc = p5_backward_stage(e, dnll, s, stream);
  e->whole_backward = false;
  return rc;
}
int p5_backward_stage_range(const P5Engine* e, int stage, int64_t* begin, int64_t* end) {
  const int nd = e->c.n_dec_layers, ne = e->c.n_enc_layers;
  *begin = *end = 0;
  if (stage == 0) { *begin = e->off_dec_fln; *end = e->n_params; }
  else if (stage >= 1 && stage <= nd) { *begin = e->dec[nd - stage].begin; *end = e->dec[nd - stage].end; }
  else if (stage == nd + 2) { *begin = e->off_enc_fln; *end = e->dec[0].begin; }
  else if (stage >= nd + 3 && stage <= nd + 2 + ne) { const int i = ne - (stage - (nd + 2)); *begin = e->enc[i].begin; *end = e->enc[i].end; }
  else if (stage == nd + ne + 3) { *begin = 0; *end = e->off_small_end; }
  return 0;
}

int p5_grad_sumsq(const float* grads, int64_t n, float* out_scalar, void* stream) {
  P5_LAUNCH(p5_sumsq_kernel, dim3(P5_SUMSQ_PARTS), dim3(256), 0, (hipStream_t)stream, out_scalar, grads, (size_t)n);
  return P5_KCHECK();
}
int p5_adamw_step(float* params, const float* grads, float* m, float* v, void* shadow_bf16, int64_t n, const float* sumsq, double max_norm,
                  double grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay, int step_t, void* stream) {
  // Hyper-parameters arrive as the doubles the reference holds them in (Python floats) and every derived scalar is formed in double and
  // rounded ONCE to fp32 -- as torch does with the Python scalars of transformers' AdamW.step (`alpha=1.0 - beta1`, `value=1.0 - beta2`,
  // `value=-step_size`, `alpha=-lr * weight_decay`): 1.f - 0.999f is 1.3e-5 off 0.001, which tests/golden/adamw_426.json sees in `v`.
  P5AdamArgs a;
  a.p = params; a.g = grads; a.m = m; a.v = v; a.shadow = shadow_bf16; a.sumsq = sumsq; a.n = (size_t)n;
  a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps; a.max_norm = (float)max_norm; a.grad_scale = (float)grad_scale;
  const double bc1 = 1.0 - pow(beta1, (double)step_t), bc2 = 1.0 - pow(beta2, (double)step_t);
  a.step_size = (float)(lr * sqrt(bc2) / bc1);
  a.decay = (float)(lr * weight_decay);
  P5_LAUNCH(p5_adamw_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, a);
  return P5_KCHECK();
}

int64_t p5_generate_workspace_bytes(const P5Engine* e, int B, int L, int K, int max_len, int max_children, int excluded_words) {
  P5Engine tmp = *e;
  return layout_gen(&tmp, nullptr, B, L, K, max_len, max_children, excluded_words, nullptr);
}
static void gen_mark_begin(P5Engine* e, void* stream) {
#ifndef P5_EMU
  if (e->gen_timing) {
    if (!e->gen_ev[0]) for (int i = 0; i < 3; ++i) hipEventCreate(&e->gen_ev[i]);
    hipEventRecord(e->gen_ev[0], (hipStream_t)stream);
  }
#endif
}
int p5_decode_begin(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int K,
                    int max_len, const int* child_off, const int* child_tok, const int* child_node, const int* roots,
                    const uint32_t* excluded_nodes, int excluded_words, int max_children, void* ws, int64_t ws_bytes, void* stream) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(K >= 1 && K <= P5_WIDE_MAX_K, "1 <= num_beams <= 4096");
  P5_REQUIRE(max_len >= 2 && max_len <= P5_MAX_LEN, "2 <= max_length <= 128 (P5_MAX_LEN)");
  P5_REQUIRE(L >= 1 && L <= 512, "1 <= L <= 512");
  P5_REQUIRE(max_children >= 1, "max_children");
  P5_REQUIRE(e->lut_half >= max_len, "bucket LUT too short");
  P5_REQUIRE(excluded_words >= 0 && (excluded_nodes || excluded_words == 0), "excluded_nodes / excluded_words");
  const int64_t need = layout_gen(e, nullptr, B, L, K, max_len, max_children, excluded_words, nullptr);
  P5_REQUIRE(ws_bytes >= need, "workspace too small");
  gen_mark_begin(e, stream);
  e->ids = input_ids; e->ww = whole_word_ids; e->mask = attention_mask; e->labels = nullptr;
  return e->c.dtype == 1
             ? decode_begin_impl<bf16>(e, B, L, K, max_len, child_off, child_tok, child_node, roots, excluded_nodes, excluded_words, max_children,
                                       (char*)ws, (hipStream_t)stream)
             : decode_begin_impl<float>(e, B, L, K, max_len, child_off, child_tok, child_node, roots, excluded_nodes, excluded_words, max_children,
                                        (char*)ws, (hipStream_t)stream);
}
int p5_decode_step(P5Engine* e, void* stream) {
  return e->c.dtype == 1 ? decode_step_impl<bf16>(e, (hipStream_t)stream) : decode_step_impl<float>(e, (hipStream_t)stream);
}
const int* p5_decode_done_flag(const P5Engine* e) { return e->gen.active ? e->gen.w.st.flags + 4 : nullptr; }
int p5_decode_finish(P5Engine* e, int* out_seq, float* out_score, int* out_len, void* stream) {
  return decode_finish_impl(e, out_seq, out_score, out_len, (hipStream_t)stream);
}
int p5_generate(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int K,
                int max_len, const int* child_off, const int* child_tok, const int* child_node, const int* roots,
                const uint32_t* excluded_nodes, int excluded_words, int max_children, int* out_seq, float* out_score, int* out_len, void* ws, int64_t ws_bytes, void* stream) {
  P5_TRY(p5_decode_begin(e, input_ids, whole_word_ids, attention_mask, B, L, K, max_len, child_off, child_tok, child_node, roots, excluded_nodes,
                         excluded_words, max_children, ws, ws_bytes, stream));
#ifndef P5_EMU
  if (e->gen_timing) {        // device-time brackets of the decode loop (p5_generate_timing): two event records, nothing is waited for
    if (!e->gen_ev[0]) for (int i = 0; i < 3; ++i) hipEventCreate(&e->gen_ev[i]);
    hipEventRecord(e->gen_ev[1], (hipStream_t)stream);
  }
#endif
  // every step is enqueued without reading anything back (the search stops on the device); the caller bounds max_len by the
  // depth of the trie, so at most a step or two are no-ops
  for (int cur_len = 1; cur_len < max_len; ++cur_len) P5_TRY(p5_decode_step(e, stream));
#ifndef P5_EMU
  if (e->gen_timing) hipEventRecord(e->gen_ev[2], (hipStream_t)stream);
#endif
  return p5_decode_finish(e, out_seq, out_score, out_len, stream);
}
int p5_generate_set_forced_prefix(P5Engine* e, const int* tokens, const int* nodes, int n) {
  P5_REQUIRE(n >= 0 && (n == 0 || (tokens && nodes)), "forced prefix: tokens / nodes");
  e->ff_next.n = n < P5_FF_MAX ? n : P5_FF_MAX;
  for (int i = 0; i < e->ff_next.n; ++i) { e->ff_next.tok[i] = tokens[i]; e->ff_next.node[i] = nodes[i]; }
  return 0;
}
int64_t p5_sample_workspace_bytes(const P5Engine* e, int B, int L, int S, int max_len, int max_children, int excluded_words) {
  (void)max_children; (void)excluded_words;       // (no buffer follows the fan-out, and the exclusion bitmap is read in place)
  P5Engine tmp = *e;
  return layout_sample(&tmp, nullptr, B, L, S, max_len, nullptr, nullptr);
}
// the scratch of the truncated step behind the sampler's workspace: [R, max_children] fp32
static int64_t trunc_scratch_bytes(int B, int S, int max_children) {
  return (int64_t)(((size_t)B * S * max_children * 4 + 255) & ~(size_t)255);
}
static int sample_items_checked(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int S,
                                int max_len, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded_nodes,
                                int excluded_words, int max_children, uint32_t seed, const uint32_t* stream_ids, uint32_t draw_base, float temperature,
                                int* out_seq, float* out_logprob, float* out_tok_logprob, int* out_len, void* ws, int64_t ws_bytes, void* stream,
                                bool truncated, int top_k, float top_p) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(B >= 1 && S >= 1 && S <= P5_WIDE_MAX_K, "sample_items: 1 <= samples per user <= 4096");
  P5_REQUIRE(max_len >= 2 && max_len <= P5_MAX_LEN, "sample_items: 2 <= max_length <= 128 (P5_MAX_LEN)");
  P5_REQUIRE(L >= 1 && L <= 512, "1 <= L <= 512");
  P5_REQUIRE(max_children >= 1, "max_children");
  P5_REQUIRE(e->lut_half >= max_len, "bucket LUT too short");
  P5_REQUIRE(temperature > 0.f && temperature < __builtin_huge_valf(), "sample_items: temperature > 0");
  P5_REQUIRE(excluded_words >= 0 && (excluded_nodes || excluded_words == 0), "excluded_nodes / excluded_words");
  P5_REQUIRE(stream_ids && out_seq && out_logprob && out_tok_logprob && out_len, "sample_items: stream_ids / outputs");
  P5_REQUIRE(e->c.d_model % (8 * (e->c.dtype == 1 ? 8 : 4)) == 0 && e->c.d_model <= 1024, "sample_items: d_model a multiple of 8 x 16 bytes, <= 1024");
  int64_t need = layout_sample(e, nullptr, B, L, S, max_len, nullptr, nullptr);
  if (truncated) {
    P5_REQUIRE(top_k >= 0, "sample_items_truncated: top_k >= 0 (0 = off)");
    P5_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_items_truncated: 0 < top_p <= 1 (1 = off)");
    need += trunc_scratch_bytes(B, S, max_children);
    P5_REQUIRE(ws_bytes >= need, "sample_items_truncated: workspace too small (p5_sample_truncated_workspace_bytes)");
  } else {
    P5_REQUIRE(ws_bytes >= need, "sample_items: workspace too small (p5_sample_workspace_bytes)");
  }
  // off (top_k 0 or >= the widest node, top_p 1): the untruncated kernels, bit for bit
  const bool trunc = truncated && ((top_k > 0 && top_k < max_children) || top_p < 1.f);
  e->ids = input_ids; e->ww = whole_word_ids; e->mask = attention_mask; e->labels = nullptr;
  return e->c.dtype == 1
             ? sample_items_impl<bf16>(e, B, L, S, max_len, child_off, child_tok, child_node, excluded_nodes, excluded_words, max_children, seed,
                                       stream_ids, draw_base, temperature, out_seq, out_logprob, out_tok_logprob, out_len, (char*)ws, (hipStream_t)stream,
                                       trunc, top_k, top_p)
             : sample_items_impl<float>(e, B, L, S, max_len, child_off, child_tok, child_node, excluded_nodes, excluded_words, max_children, seed,
                                        stream_ids, draw_base, temperature, out_seq, out_logprob, out_tok_logprob, out_len, (char*)ws, (hipStream_t)stream,
                                        trunc, top_k, top_p);
}
int p5_sample_items(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int S,
                    int max_len, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded_nodes,
                    int excluded_words, int max_children, uint32_t seed, const uint32_t* stream_ids, uint32_t draw_base, float temperature,
                    int* out_seq, float* out_logprob, float* out_tok_logprob, int* out_len, void* ws, int64_t ws_bytes, void* stream) {
  return sample_items_checked(e, input_ids, whole_word_ids, attention_mask, B, L, S, max_len, child_off, child_tok, child_node, excluded_nodes,
                              excluded_words, max_children, seed, stream_ids, draw_base, temperature, out_seq, out_logprob, out_tok_logprob, out_len, ws,
                              ws_bytes, stream, false, 0, 1.f);
}
int64_t p5_sample_truncated_workspace_bytes(const P5Engine* e, int B, int L, int S, int max_len, int max_children, int excluded_words) {
  (void)excluded_words;       // (the exclusion bitmap is read in place)
  if (B < 1 || S < 1 || S > P5_WIDE_MAX_K || max_len < 2 || max_len > P5_MAX_LEN || L < 1 || L > 512 || max_children < 1) {
    fail("sample_items_truncated: 1 <= samples per user <= 4096, 2 <= max_length <= 128, 1 <= L <= 512, max_children >= 1");
    return -1;
  }
  P5Engine tmp = *e;
  return layout_sample(&tmp, nullptr, B, L, S, max_len, nullptr, nullptr) + trunc_scratch_bytes(B, S, max_children);
}
int p5_sample_items_truncated(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int S,
                              int max_len, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded_nodes,
                              int excluded_words, int max_children, uint32_t seed, const uint32_t* stream_ids, uint32_t draw_base, float temperature,
                              int top_k, float top_p, int* out_seq, float* out_logprob, float* out_tok_logprob, int* out_len, void* ws,
                              int64_t ws_bytes, void* stream) {
  return sample_items_checked(e, input_ids, whole_word_ids, attention_mask, B, L, S, max_len, child_off, child_tok, child_node, excluded_nodes,
                              excluded_words, max_children, seed, stream_ids, draw_base, temperature, out_seq, out_logprob, out_tok_logprob, out_len, ws,
                              ws_bytes, stream, true, top_k, top_p);
}
static int sbs_limits(int B, int S, int K, int max_len) {
  P5_REQUIRE(B >= 1 && K >= 1 && K <= P5_SBS_MAX_K, "sample_slates: 1 <= slate size <= 4096");
  P5_REQUIRE(S >= 1 && (int64_t)S * K <= P5_WIDE_MAX_K, "sample_slates: 1 <= slates per user, slates x slate size <= 4096 rows per user and call");
  P5_REQUIRE(max_len >= 2 && max_len <= P5_MAX_LEN, "sample_slates: 2 <= max_length <= 128 (P5_MAX_LEN)");
  return 0;
}
int64_t p5_sample_slates_workspace_bytes(const P5Engine* e, int B, int L, int S, int K, int max_len, int max_children, int excluded_words) {
  (void)excluded_words;       // (the exclusion bitmap is read in place)
  if (sbs_limits(B, S, K, max_len) != 0) return -1;
  if (max_children < 1 || L < 1 || L > 512) { fail("sample_slates: max_children >= 1, 1 <= L <= 512"); return -1; }
  P5Engine tmp = *e;
  return layout_sbs(&tmp, nullptr, B, L, S, K, max_len, max_children, nullptr, nullptr);
}
int p5_sample_slates(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int S, int K,
                     int max_len, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded_nodes,
                     int excluded_words, int max_children, uint32_t seed, const uint32_t* stream_ids, uint32_t slate_base, float temperature,
                     int* out_seq, float* out_logprob, float* out_perturbed, float* out_tok_logprob, int* out_len, void* ws, int64_t ws_bytes,
                     void* stream) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_TRY(sbs_limits(B, S, K, max_len));
  P5_REQUIRE(L >= 1 && L <= 512, "1 <= L <= 512");
  P5_REQUIRE(max_children >= 1, "max_children");
  P5_REQUIRE(e->lut_half >= max_len, "bucket LUT too short");
  P5_REQUIRE(temperature > 0.f && temperature < __builtin_huge_valf(), "sample_slates: temperature > 0");
  P5_REQUIRE(excluded_words >= 0 && (excluded_nodes || excluded_words == 0), "excluded_nodes / excluded_words");
  P5_REQUIRE(stream_ids && out_seq && out_logprob && out_perturbed && out_tok_logprob && out_len, "sample_slates: stream_ids / outputs");
  P5_REQUIRE(e->c.d_model % (8 * (e->c.dtype == 1 ? 8 : 4)) == 0 && e->c.d_model <= 1024, "sample_slates: d_model a multiple of 8 x 16 bytes, <= 1024");
  const int64_t need = layout_sbs(e, nullptr, B, L, S, K, max_len, max_children, nullptr, nullptr);
  P5_REQUIRE(ws_bytes >= need, "sample_slates: workspace too small (p5_sample_slates_workspace_bytes)");
  e->ids = input_ids; e->ww = whole_word_ids; e->mask = attention_mask; e->labels = nullptr;
  return e->c.dtype == 1
             ? sbs_impl<bf16>(e, B, L, S, K, max_len, child_off, child_tok, child_node, excluded_nodes, excluded_words, max_children, seed, stream_ids,
                              slate_base, temperature, out_seq, out_logprob, out_perturbed, out_tok_logprob, out_len, (char*)ws, (hipStream_t)stream)
             : sbs_impl<float>(e, B, L, S, K, max_len, child_off, child_tok, child_node, excluded_nodes, excluded_words, max_children, seed, stream_ids,
                               slate_base, temperature, out_seq, out_logprob, out_perturbed, out_tok_logprob, out_len, (char*)ws, (hipStream_t)stream);
}
int64_t p5_generate_history_count(int B, int K, int max_len) { return 4 + (int64_t)max_len * P5_HIST_FIELDS * B * K; }
int p5_generate_draft(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int K,
                      int max_len, const int* child_off, const int* child_tok, const int* child_node, const int* roots,
                      const uint32_t* excluded_nodes, int excluded_words, int max_children, int* out_seq, float* out_score, int* out_len, int* hist,
                      void* ws, int64_t ws_bytes, void* stream) {
  P5_REQUIRE(hist, "p5_generate_draft: history buffer");
  P5_REQUIRE(K >= 1 && K <= P5_MAX_K, "p5_generate_draft: 1 <= num_beams <= 64");
  e->gen_hist_next = hist;
  const int rc = p5_generate(e, input_ids, whole_word_ids, attention_mask, B, L, K, max_len, child_off, child_tok, child_node, roots, excluded_nodes,
                             excluded_words, max_children, out_seq, out_score, out_len, ws, ws_bytes, stream);
  e->gen_hist_next = nullptr;
  return rc;
}
int64_t p5_verify_workspace_bytes(const P5Engine* e, int B, int L, int K, int Kw, int max_len, int max_children, int excluded_words) {
  return layout_verify(const_cast<P5Engine*>(e), nullptr, B, L, K, Kw, max_len, max_children, excluded_words, nullptr);
}
int p5_verify_begin(P5Engine* e, int B, int L, int K, int Kw, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                    const int* roots, int max_children, int excluded_words, void* ws, int64_t ws_bytes) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(K >= 1 && 2 * K * K <= P5_VERIFY_POOL, "verified generation: 1 <= num_beams <= 22");
  P5_REQUIRE(Kw >= K && Kw <= P5_MAX_K, "draft beam width: num_beams <= Kw <= 64");
  P5_REQUIRE(max_len >= 2 && max_len <= P5_MAX_LEN, "2 <= max_length <= 128 (P5_MAX_LEN)");
  P5_REQUIRE(L >= 1 && L <= 512, "1 <= L <= 512");
  P5_REQUIRE(max_children >= 1 && excluded_words >= 0, "max_children / excluded_words");
  P5_REQUIRE(e->lut_half >= max_len, "bucket LUT too short");
  const int64_t need = layout_verify(e, nullptr, B, L, K, Kw, max_len, max_children, excluded_words, nullptr);
  P5_REQUIRE(ws_bytes >= need, "workspace too small");
  return verify_begin_impl(e, B, L, K, Kw, max_len, child_off, child_tok, child_node, roots, max_children, excluded_words, (char*)ws);
}
int p5_verify_encode(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, void* stream) {
  P5_REQUIRE(e->ver && e->ver->begun, "p5_verify_encode without p5_verify_begin");
  return e->c.dtype == 1 ? verify_encode_impl<bf16>(e, input_ids, whole_word_ids, attention_mask, (hipStream_t)stream)
                         : verify_encode_impl<float>(e, input_ids, whole_word_ids, attention_mask, (hipStream_t)stream);
}
const void* p5_verify_encoder_output(const P5Engine* e) { return (e->ver && e->ver->encoded) ? e->enc_out : nullptr; }
int p5_verify_plan(P5Engine* e, const int* hist, void* stream) {
  P5_REQUIRE(e->ver && e->ver->begun, "p5_verify_plan without p5_verify_begin");
  P5_REQUIRE(hist, "p5_verify_plan: history of the draft search");
  return verify_plan_impl(e, hist, (hipStream_t)stream);
}
int p5_verify_row_capacity(int Kw, int max_len) { return verify_cap(Kw, max_len); }
const int* p5_verify_plan_header(const P5Engine* e) { return (e->ver && e->ver->begun) ? e->ver->w.pl.hdr : nullptr; }
int p5_verify_run(P5Engine* e, int rows_per_user, const uint32_t* excluded_nodes, int* out_seq, float* out_score, int* out_len, int* out_missing,
                  void* stream) {
  P5_REQUIRE(e->ver && e->ver->begun && e->ver->encoded && e->ver->planned, "p5_verify_run needs p5_verify_begin + p5_verify_encode + p5_verify_plan");
  P5_REQUIRE(rows_per_user >= 1 && rows_per_user <= e->ver->w.pl.cap, "rows_per_user: 1 .. capacity of the plan");
  P5_REQUIRE(e->ver->excl_words == 0 || excluded_nodes, "excluded_nodes");
  return e->c.dtype == 1 ? verify_run_impl<bf16>(e, rows_per_user, excluded_nodes, out_seq, out_score, out_len, out_missing, (hipStream_t)stream)
                         : verify_run_impl<float>(e, rows_per_user, excluded_nodes, out_seq, out_score, out_len, out_missing, (hipStream_t)stream);
}
int p5_generate_set_encoder_output(P5Engine* e, const float* enc_out_f32) { e->enc_ext_next = enc_out_f32; return 0; }
int64_t p5_rank_workspace_bytes(const P5Engine* e, int B, int L, int rows_per_user, int64_t n_edges, int n_items, int top_n) {
  return layout_rank(const_cast<P5Engine*>(e), nullptr, B, L, rows_per_user, n_edges, n_items, top_n, nullptr);
}
int p5_rank_items(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                  const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                  const int* row_anc, int rows_per_user, int max_depth, const int* item_edges, int n_items, int path_len,
                  const uint32_t* excluded_items, int top_n, int exact_products, float* out_scores_all, int* out_index, float* out_score,
                  int* out_flagged, void* ws, int64_t ws_bytes, void* stream) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(B >= 1 && L >= 1 && L <= 512, "rank_items: B >= 1, 1 <= L <= 512");
  P5_REQUIRE(child_off && child_tok && n_edges >= 1 && row_tok && row_depth && row_node && row_anc && item_edges, "rank_items: trie / plan / path arrays");
  P5_REQUIRE(rows_per_user >= 1 && max_depth >= 1 && max_depth <= e->lut_half, "rank_items: rows_per_user >= 1, 1 <= max_depth <= the bucket LUT's half length");
  P5_REQUIRE((int64_t)B * ((rows_per_user + 15) / 16 * 16 + 16 * ((rows_per_user + 511) / 512)) * e->c.n_heads < ((int64_t)1 << 31), "rank_items: B x rows_per_user x heads must stay below 2^31 (rank fewer users per call)");
  P5_REQUIRE(n_items >= 1 && path_len >= 1, "rank_items: n_items, path_len");
  P5_REQUIRE(top_n >= 1 && top_n <= P5_WIDE_MAX_K, "rank_items: 1 <= top_n <= 4096");
  P5_REQUIRE(out_index && out_score && out_flagged, "rank_items: out_index / out_score / out_flagged");
  const int64_t need = layout_rank(e, nullptr, B, L, rows_per_user, n_edges, n_items, top_n, nullptr);
  P5_REQUIRE(ws && ws_bytes >= need, "workspace too small");
  RankArgs r;
  r.input_ids = input_ids; r.whole_word_ids = whole_word_ids; r.attention_mask = attention_mask; r.B = B; r.L = L;
  r.child_off = child_off; r.child_tok = child_tok; r.n_edges = n_edges;
  r.pl.row_tok = row_tok; r.pl.row_depth = row_depth; r.pl.row_node = row_node; r.pl.anc = row_anc; r.pl.rows = rows_per_user; r.pl.max_depth = max_depth;
  r.pl.B = B; r.pl.CQ = 0; r.pl.nchunk = 0;
  r.item_edges = item_edges; r.n_items = n_items; r.path_len = path_len; r.excluded = excluded_items; r.top_n = top_n; r.exact = exact_products;
  r.out_scores_all = out_scores_all; r.out_index = out_index; r.out_score = out_score; r.out_flagged = out_flagged; r.ws = (char*)ws;
  return e->c.dtype == 1 ? rank_items_impl<bf16>(e, r, (hipStream_t)stream) : rank_items_impl<float>(e, r, (hipStream_t)stream);
}
int64_t p5_cand_workspace_bytes(const P5Engine* e, int B, int L, int C, int path_len, int rows_per_user) {
  return layout_cand(const_cast<P5Engine*>(e), nullptr, B, L, C, path_len, rows_per_user, nullptr);
}
int p5_cand_plan(P5Engine* e, const int* candidates, int B, int C, const int* item_rows, int n_items, int path_len, void* ws, int64_t ws_bytes,
                 void* stream) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(candidates && item_rows && B >= 1 && n_items >= 1 && path_len >= 1, "cand_plan: candidates / item_rows / B / n_items / path_len");
  P5_REQUIRE(C >= 1 && C <= P5_WIDE_MAX_K, "cand_plan: 1 <= C <= 4096");
  P5_REQUIRE(ws && ws_bytes >= layout_cand(e, nullptr, B, 1, C, path_len, 0, nullptr), "workspace too small");
  return cand_plan_impl(e, candidates, B, C, item_rows, n_items, path_len, (char*)ws, (hipStream_t)stream);
}
int p5_cand_score(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                  const int* row_tok, const int* row_depth, const int* row_anc, int max_depth, const int* candidates, int C, const int* item_rows,
                  const int64_t* item_tokens, int n_items, int path_len, int token_stride, int rows_per_user, int top_n, int exact_products,
                  float* out_scores, int* out_order, int* out_index, float* out_score, int* out_flagged, void* ws, int64_t ws_bytes, void* stream) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(B >= 1 && L >= 1 && L <= 512, "cand_score: B >= 1, 1 <= L <= 512");
  P5_REQUIRE(row_tok && row_depth && row_anc && candidates && item_rows && item_tokens, "cand_score: plan / candidate / item arrays");
  P5_REQUIRE(max_depth >= 1 && max_depth <= e->lut_half, "cand_score: 1 <= max_depth <= the bucket LUT's half length");
  P5_REQUIRE(C >= 1 && C <= P5_WIDE_MAX_K && top_n >= 1 && top_n <= C, "cand_score: 1 <= top_n <= C <= 4096");
  P5_REQUIRE(n_items >= 1 && path_len >= 1 && token_stride > path_len, "cand_score: n_items, path_len, token_stride > path_len");
  P5_REQUIRE(rows_per_user >= 1 && rows_per_user <= C * path_len, "cand_score: 1 <= rows_per_user <= C x path_len");
  P5_REQUIRE((int64_t)B * ((rows_per_user + 15) / 16 * 16 + 16 * ((rows_per_user + 511) / 512)) * e->c.n_heads < ((int64_t)1 << 31), "cand_score: B x rows_per_user x heads must stay below 2^31 (score fewer users per call)");
  P5_REQUIRE(out_scores && out_order && out_index && out_score && out_flagged, "cand_score: outputs");
  P5_REQUIRE(ws && ws_bytes >= layout_cand(e, nullptr, B, L, C, path_len, rows_per_user, nullptr), "workspace too small");
  CandArgs r;
  r.input_ids = input_ids; r.whole_word_ids = whole_word_ids; r.attention_mask = attention_mask; r.B = B; r.L = L;
  r.row_tok = row_tok; r.row_depth = row_depth; r.row_anc = row_anc; r.max_depth = max_depth;
  r.cand = candidates; r.item_rows = item_rows; r.item_tokens = item_tokens; r.C = C; r.n_items = n_items; r.path_len = path_len; r.ldt = token_stride;
  r.rows = rows_per_user; r.top_n = top_n; r.exact = exact_products;
  r.out_scores = out_scores; r.out_order = out_order; r.out_index = out_index; r.out_score = out_score; r.out_flagged = out_flagged; r.ws = (char*)ws;
  return e->c.dtype == 1 ? cand_score_impl<bf16>(e, r, (hipStream_t)stream) : cand_score_impl<float>(e, r, (hipStream_t)stream);
}
int64_t p5_prune_workspace_bytes(const P5Engine* e, int B, int L, int rows_total, int rows_per_user, int64_t n_edges, int n_items, int top_n) {
  return layout_prune(const_cast<P5Engine*>(e), nullptr, B, L, rows_total, rows_per_user, n_edges, n_items, top_n, nullptr);
}
static int prune_rank_args(P5Engine* e, RankArgs& r, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                           int B, int L, const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth,
                           const int* row_node, const int* row_anc, int rows_total, int max_depth, const int* item_edges, int n_items, int path_len,
                           const uint32_t* excluded_items, int top_n, int* out_index, float* out_score, int* out_flagged) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(B >= 1 && L >= 1 && L <= 512, "prune: B >= 1, 1 <= L <= 512");
  P5_REQUIRE(child_off && child_tok && n_edges >= 1 && row_tok && row_depth && row_node && row_anc && item_edges, "prune: trie / plan / path arrays");
  P5_REQUIRE(rows_total >= 1 && max_depth >= 1 && max_depth <= e->lut_half, "prune: rows_total >= 1, 1 <= max_depth <= the bucket LUT's half length");
  P5_REQUIRE((int64_t)B * ((rows_total + 15) / 16 * 16 + 16 * ((rows_total + 511) / 512)) * e->c.n_heads < ((int64_t)1 << 31), "prune: B x rows_total x heads must stay below 2^31 (rank fewer users per call)");
  P5_REQUIRE(n_items >= 1 && path_len >= 1, "prune: n_items, path_len");
  P5_REQUIRE(top_n >= 1 && top_n <= P5_WIDE_MAX_K, "prune: 1 <= top_n <= 4096");
  P5_REQUIRE(out_index && out_score && out_flagged, "prune: out_index / out_score / out_flagged");
  r.input_ids = input_ids; r.whole_word_ids = whole_word_ids; r.attention_mask = attention_mask; r.B = B; r.L = L;
  r.child_off = child_off; r.child_tok = child_tok; r.n_edges = n_edges;
  r.pl.row_tok = row_tok; r.pl.row_depth = row_depth; r.pl.row_node = row_node; r.pl.anc = row_anc; r.pl.rows = rows_total; r.pl.max_depth = max_depth;
  r.pl.B = B; r.pl.CQ = 0; r.pl.nchunk = 0;
  r.item_edges = item_edges; r.n_items = n_items; r.path_len = path_len; r.excluded = excluded_items; r.top_n = top_n; r.exact = 0;
  r.out_scores_all = nullptr; r.out_index = out_index; r.out_score = out_score; r.out_flagged = out_flagged; r.ws = nullptr;
  return 0;
}
int p5_prune_propose(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                     const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                     const int* row_anc, int rows_total, int max_depth, const int* row_edge, const int* row_lmax, const int* item_edges, int n_items,
                     int path_len, const uint32_t* excluded_items, int top_n, float slack, int* out_index, float* out_score, int* out_flagged,
                     void* rank_ws, int64_t rank_ws_bytes, void* prune_ws, int64_t prune_ws_bytes, void* stream) {
  RankArgs r;
  P5_TRY(prune_rank_args(e, r, input_ids, whole_word_ids, attention_mask, B, L, child_off, child_tok, n_edges, row_tok, row_depth, row_node, row_anc,
                         rows_total, max_depth, item_edges, n_items, path_len, excluded_items, top_n, out_index, out_score, out_flagged));
  P5_REQUIRE(row_edge && row_lmax && slack >= 0.f, "prune_propose: row_edge / row_lmax / slack >= 0");
  P5_REQUIRE(rank_ws && rank_ws_bytes >= layout_rank(e, nullptr, B, L, rows_total, n_edges, n_items, top_n, nullptr), "rank workspace too small");
  P5_REQUIRE(prune_ws && prune_ws_bytes >= layout_prune(e, nullptr, B, 1, rows_total, 0, n_edges, n_items, top_n, nullptr), "prune workspace too small");
  r.ws = (char*)rank_ws;
  return e->c.dtype == 1 ? prune_propose_impl<bf16>(e, r, row_edge, row_lmax, slack, (char*)prune_ws, (hipStream_t)stream)
                         : prune_propose_impl<float>(e, r, row_edge, row_lmax, slack, (char*)prune_ws, (hipStream_t)stream);
}
int p5_prune_decide(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                    const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                    const int* row_anc, int rows_total, int max_depth, const int* row_edge, const int* row_lmax, const int* edge_row,
                    const int* item_edges, int n_items, int path_len, const uint32_t* excluded_items, int top_n, int rows_per_user, float margin,
                    int* out_index, float* out_score, int* out_flagged, void* prune_ws, int64_t prune_ws_bytes, void* stream) {
  PruneArgs a;
  P5_TRY(prune_rank_args(e, a.r, input_ids, whole_word_ids, attention_mask, B, L, child_off, child_tok, n_edges, row_tok, row_depth, row_node, row_anc,
                         rows_total, max_depth, item_edges, n_items, path_len, excluded_items, top_n, out_index, out_score, out_flagged));
  P5_REQUIRE(row_edge && row_lmax && edge_row && margin >= 0.f, "prune_decide: row_edge / row_lmax / edge_row / margin >= 0");
  P5_REQUIRE(rows_per_user >= 1 && rows_per_user <= rows_total, "prune_decide: 1 <= rows_per_user <= rows_total");
  P5_REQUIRE(prune_ws && prune_ws_bytes >= layout_prune(e, nullptr, B, L, rows_total, rows_per_user, n_edges, n_items, top_n, nullptr), "prune workspace too small");
  a.r.ws = (char*)prune_ws;
  a.row_edge = row_edge; a.row_lmax = row_lmax; a.edge_row = edge_row; a.rows = rows_per_user; a.margin = margin;
  return e->c.dtype == 1 ? prune_decide_impl<bf16>(e, a, (hipStream_t)stream) : prune_decide_impl<float>(e, a, (hipStream_t)stream);
}
int64_t p5_bound_workspace_bytes(const P5Engine* e, int B, int L, int rows_total, int rows_per_user, int64_t n_edges, int n_items, int top_n, int n_seeds,
                                 int max_depth) {
  return layout_bound(const_cast<P5Engine*>(e), nullptr, B, L, rows_total, rows_per_user, n_edges, n_items, top_n, n_seeds, max_depth, nullptr);
}
int p5_bound_begin(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                   const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_node, int rows_total, int max_depth,
                   const int* edge_row, const int64_t* seeds, int n_seeds, int seed_len, int n_items, int top_n, void* ws, int64_t ws_bytes,
                   void* stream) {
  P5_REQUIRE(e->P, "engine not bound");
  P5_REQUIRE(B >= 1 && L >= 1 && L <= 512, "bound_begin: B >= 1, 1 <= L <= 512");
  P5_REQUIRE(child_off && child_tok && n_edges >= 1 && row_tok && row_node && edge_row, "bound_begin: trie / plan arrays");
  P5_REQUIRE(rows_total >= 1 && max_depth >= 1 && max_depth <= e->lut_half, "bound_begin: rows_total >= 1, 1 <= max_depth <= the bucket LUT's half length");
  P5_REQUIRE(seeds && n_seeds >= 1 && n_seeds <= P5_WIDE_MAX_K && seed_len >= 1, "bound_begin: seeds, 1 <= n_seeds <= 4096, seed_len >= 1");
  P5_REQUIRE(n_items >= 1 && top_n >= 1 && top_n <= P5_WIDE_MAX_K, "bound_begin: n_items, 1 <= top_n <= 4096");
  P5_REQUIRE(ws && ws_bytes >= layout_bound(e, nullptr, B, L, rows_total, 1, n_edges, n_items, top_n, n_seeds, max_depth, nullptr), "workspace too small");
  BoundArgs a;
  memset(&a, 0, sizeof(a));
  RankArgs& r = a.p.r;
  r.input_ids = input_ids; r.whole_word_ids = whole_word_ids; r.attention_mask = attention_mask; r.B = B; r.L = L;
  r.child_off = child_off; r.child_tok = child_tok; r.n_edges = n_edges;
  r.pl.row_tok = row_tok; r.pl.row_node = row_node; r.pl.rows = rows_total; r.pl.max_depth = max_depth; r.pl.B = B;
  r.n_items = n_items; r.top_n = top_n; r.ws = (char*)ws;
  a.p.edge_row = edge_row; a.p.rows = 1;
  a.seeds = seeds; a.n_seeds = n_seeds; a.seed_len = seed_len;
  return e->c.dtype == 1 ? bound_begin_impl<bf16>(e, a, (hipStream_t)stream) : bound_begin_impl<float>(e, a, (hipStream_t)stream);
}
int p5_bound_round(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                   const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                   const int* row_anc, int rows_total, int max_depth, const int* row_edge, const int* row_lmax, const int* edge_row,
                   const int* item_edges, int n_items, int path_len, const uint32_t* excluded_items, int top_n, int n_seeds, int rows_per_user,
                   float margin, int* out_index, float* out_score, int* out_flagged, void* ws, int64_t ws_bytes, void* stream) {
  BoundArgs a;
  P5_TRY(prune_rank_args(e, a.p.r, input_ids, whole_word_ids, attention_mask, B, L, child_off, child_tok, n_edges, row_tok, row_depth, row_node, row_anc,
                         rows_total, max_depth, item_edges, n_items, path_len, excluded_items, top_n, out_index, out_score, out_flagged));
  P5_REQUIRE(row_edge && row_lmax && edge_row && margin >= 0.f, "bound_round: row_edge / row_lmax / edge_row / margin >= 0");
  P5_REQUIRE(n_seeds >= 1 && n_seeds <= P5_WIDE_MAX_K, "bound_round: 1 <= n_seeds <= 4096 (as given to p5_bound_begin)");
  P5_REQUIRE(rows_per_user >= 1 && rows_per_user <= rows_total, "bound_round: 1 <= rows_per_user <= rows_total");
  P5_REQUIRE(ws && ws_bytes >= layout_bound(e, nullptr, B, L, rows_total, rows_per_user, n_edges, n_items, top_n, n_seeds, max_depth, nullptr), "workspace too small");
  a.p.r.ws = (char*)ws;
  a.p.row_edge = row_edge; a.p.row_lmax = row_lmax; a.p.edge_row = edge_row; a.p.rows = rows_per_user; a.p.margin = margin;
  a.seeds = nullptr; a.n_seeds = n_seeds; a.seed_len = 0;
  return e->c.dtype == 1 ? bound_round_impl<bf16>(e, a, (hipStream_t)stream) : bound_round_impl<float>(e, a, (hipStream_t)stream);
}
int p5_generate_timing(P5Engine* e, int enable, float* encode_ms, float* decode_ms) {
#ifndef P5_EMU
  if (encode_ms || decode_ms) {
    P5_REQUIRE(e->gen_timing && e->gen_ev[0], "generate_timing: enable it before the p5_generate call to be measured");
    P5_REQUIRE(hipEventSynchronize(e->gen_ev[2]) == hipSuccess, "generate_timing: event sync failed");
    float a = 0.f, b = 0.f;
    hipEventElapsedTime(&a, e->gen_ev[0], e->gen_ev[1]);
    hipEventElapsedTime(&b, e->gen_ev[1], e->gen_ev[2]);
    if (encode_ms) *encode_ms = a;
    if (decode_ms) *decode_ms = b;
  }
  e->gen_timing = enable != 0;
#else
  if (encode_ms) *encode_ms = 0.f;
  if (decode_ms) *decode_ms = 0.f;
  (void)enable;
#endif
  return 0;
}
int p5_encode(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
              void* enc_out, void* ws, int64_t ws_bytes, void* stream) {
  P5_REQUIRE(e->P, "engine not bound");
  const int64_t need = layout_ws(e, (char*)ws, B, L, 0, false);
  P5_REQUIRE(ws_bytes >= need, "workspace too small");
  e->B = B; e->Gt = 1; e->Bd = B; e->tgt_w = nullptr; e->L = L; e->T = 0; e->M = B * L; e->Md = 0; e->training = 0;
  e->ids = input_ids; e->ww = whole_word_ids; e->mask = attention_mask;
  P5_TRY(e->c.dtype == 1 ? encoder_fwd<bf16>(e, (hipStream_t)stream) : encoder_fwd<float>(e, (hipStream_t)stream));
  const size_t bytes = (size_t)B * L * e->c.d_model * (e->c.dtype == 1 ? 2 : 4);
  hipMemcpyAsync(enc_out, e->enc_out, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return 0;
}

// ---- per-kernel entry points ---------------------------------------------------------------------------
static P5Drop op_drop(const uint32_t* state, uint32_t site, float p) {
  P5Drop d = no_drop();
  if (state && p > 0.f) { d.state = state; d.site_key = p5_site_key(site); d.thr = p5_drop_thr(p); d.scale = 1.f / (1.f - p); }
  return d;
}
int p5_op_gemm(int dtype, const void* A, const void* Bm, void* C, const void* aux, int M, int N, int K, int lda, int ldb, int ldc, int ldaux,
               int a_ks, int b_ks, int epi, int c_f32, int splitk, float alpha, const uint32_t* rng_state, uint32_t site, float drop_p,
               void* stream) {
  P5GemmArgs g;
  g.A = A; g.B = Bm; g.C = C; g.aux = aux; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux;
  g.a_ks = a_ks; g.b_ks = b_ks; g.epi = epi; g.c_f32 = c_f32; g.splitk = splitk; g.ring = 0; g.alpha = alpha; g.drop = op_drop(rng_state, site, drop_p);
  g.mm_split = (dtype == 2) ? 1 : 0;      // dtype 2 (tests): fp32 operands, split-f16 products
  g.rowss = nullptr; g.rowss_invd = 0.f; g.rowss_eps = 0.f; g.ssq_out = nullptr; g.rowss_nt = 0; g.ssq_nt = 0; g.c_split_stride = 0;
  g.g4_tiles_n = 0; g.g4_nk = 0; g.xcd_bm = g.xcd_bn = 0;
  return dtype == 1 ? launch_gemm<bf16>(g, (hipStream_t)stream) : launch_gemm<float>(g, (hipStream_t)stream);
}
int p5_op_gemm_group(int tile_cfg, int ks, int nprob, const P5GemmProblem* probs, const uint32_t* rng_state, uint32_t site, float drop_p,
                     void* stream) {
  P5_REQUIRE(nprob >= 1 && nprob <= P5_MAX_GROUP && probs, "gemm_group: 1..8 problems");
  P5GemmGroup grp;
  memset(&grp, 0, sizeof(grp));
  grp.nprob = nprob;
  for (int i = 0; i < nprob; ++i) {
    const P5GemmProblem& q = probs[i];
    P5GemmArgs& g = grp.p[i];
    g.A = q.A; g.B = q.B; g.C = q.C; g.aux = q.aux; g.M = q.M; g.N = q.N; g.K = q.K; g.lda = q.lda; g.ldb = q.ldb; g.ldc = q.ldc; g.ldaux = q.ldaux;
    g.a_ks = ks; g.b_ks = ks; g.epi = q.epi; g.c_f32 = q.c_f32; g.splitk = q.splitk; g.alpha = q.alpha; g.drop = op_drop(rng_state, site, drop_p);
    g.rowss = q.rowss; g.rowss_invd = q.rowss ? 1.0f / (float)q.K : 0.f; g.rowss_eps = q.rowss_eps; g.ssq_out = q.ssq_out;
    g.rowss_nt = q.rowss_nt; g.ssq_nt = q.ssq_nt;
    g.C2 = q.C2; g.ldc2 = q.ldc2; g.gate_F = q.gate_F;
    g.nb_dot = q.nb_dot; g.nb_dot_nt = q.nb_dot_nt; g.nb_rin = q.nb_rin; g.nb_rout = q.nb_rout; g.nb_w = q.nb_w; g.nb_dw = q.nb_dw;
    if (q.epi == P5_EPI_NORM_BWD) {
      P5_REQUIRE(tile_cfg == P5_G5_128x128 && !ks, "gemm_group: the T5LayerNorm-backward epilogue runs on tile_cfg 4, ks 0");
      g.rowss_invd = 1.0f / (float)q.N;      // (the statistics are those of the d_model-wide rows of x = aux, not of the reduction dimension)
    }
    if (q.epi == P5_EPI_MASK_POS && q.ssq_out)
      P5_REQUIRE((tile_cfg == P5_G4_256x128 || tile_cfg == P5_G5_256x128 || tile_cfg == P5_G5_128x128) && !ks && (g_opt_gemm_ws & 1) && q.ssq_nt > 0 && !q.c_f32,
                 "gemm_group: row sums of <d pre, pre> (epi 3 + ssq_out) exist in the wave-specialised kernel only (tile_cfg 1, 3 or 4)");
    if (q.epi == P5_EPI_GELU_GATE || q.epi == P5_EPI_GELU_GATE_BWD)
      P5_REQUIRE(tile_cfg == P5_G4_256x128 && !ks && (g_opt_gemm_ws & 1) && (q.M % 256) == 0 && (q.N % 128) == 0 && !q.c_f32 &&
                 (q.epi == P5_EPI_GELU_GATE ? (q.C2 && q.gate_F * 2 == q.N) : (q.aux && q.gate_F == 0)),
                 "gemm_group: the gated-GELU epilogues run on whole 256x128 tiles of the wave-specialised kernel (tile_cfg 1, ks 0)");
  }
  return launch_gemm4(tile_cfg, ks != 0, grp, (hipStream_t)stream);
}
int p5_op_rmsnorm_fwd(int dtype, void* y, float* rstd, const void* x, const float* w, int rows, int d, float eps, void* stream) {
  return dtype == 1 ? rmsnorm_fwd<bf16>((hipStream_t)stream, y, rstd, x, w, rows, d, eps, no_drop())
                    : rmsnorm_fwd<float>((hipStream_t)stream, y, rstd, x, w, rows, d, eps, no_drop());
}
int p5_op_rmsnorm_bwd(int dtype, float* dres_out, void* dy_next, float* dw, const void* dy, const void* x, const float* w, const float* rstd,
                      const float* dres_in, int rows, int d, float* dw_partial, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int nblk = 0;
  P5_TRY(dtype == 1 ? rmsnorm_bwd<bf16>(s, dres_out, dy_next, dw, dy, x, w, rstd, dres_in, rows, d, no_drop(), no_drop(), dw_partial, &nblk)
                    : rmsnorm_bwd<float>(s, dres_out, dy_next, dw, dy, x, w, rstd, dres_in, rows, d, no_drop(), no_drop(), dw_partial, &nblk));
  if (dw_partial) {    // the engine's mode: per-workgroup partials + a separate reduction
    P5_LAUNCH(p5_reduce_rows_kernel, dim3((d + 15) / 16), dim3(256), 0, s, dw, (const float*)dw_partial, nblk, d);
    P5_TRY(P5_KCHECK());
  }
  return 0;
}
// test hook (p5_set_option "attn_op_keep_bits"): the standalone attention ops hand the long-sequence kernels a keep-mask buffer of their
// own (P5AttnArgs::keep_bits: written by p5_op_attn_fwd, read by the p5_op_attn_bwd that follows it), as the engine does per encoder layer
static uint32_t* op_keep_bits(int dtype, int B, int H, int Lq, int Lk, const P5Drop& d) {
  static uint32_t* buf = nullptr;
  static size_t cap = 0;
  if (!g_opt_attn_op_keep_bits || dtype != 1 || Lk <= 128 || d.state == nullptr || d.thr == 0 || !g_opt_attn_fwd_head || !g_opt_attn_bwd_head) return nullptr;
  const size_t need = (size_t)B * H * ((Lq + 15) / 16) * 1024;
  if (need > cap) {
#ifdef P5_EMU
    free(buf);
    buf = (uint32_t*)malloc(need);
    if (!buf) { cap = 0; return nullptr; }
#else
    if (buf) (void)hipFree(buf);
    buf = nullptr; cap = 0;
    if (hipMalloc((void**)&buf, need) != hipSuccess) return nullptr;      // (the only allocation of the library: a test hook, off by default)
#endif
    cap = need;
  }
  return buf;
}
int p5_op_attn_fwd(int dtype, const void* Q, const void* K, const void* V, void* O, float* lse, const float* rel_table, const int* lut,
                   int lut_half, const int64_t* kmask, int B, int H, int Lq, int Lk, int ldq, int ldk, int ldv, int ldo, int causal,
                   const uint32_t* rng_state, uint32_t site, float drop_p, void* stream) {
  P5AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.Q = Q; a.K = K; a.V = V; a.O = O; a.lse = lse; a.rel_table = rel_table; a.bucket_lut = lut; a.lut_half = lut_half; a.kmask = kmask;
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.causal = causal;
  a.drop = op_drop(rng_state, site, drop_p);
  a.keep_bits = op_keep_bits(dtype, B, H, Lq, Lk, a.drop);
  return dtype == 1 ? launch_attn_fwd<bf16>(a, (hipStream_t)stream) : launch_attn_fwd<float>(a, (hipStream_t)stream);
}
int p5_op_attn_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse, float* Dvec,
                   void* dQ, void* dK, void* dV, const float* rel_table, float* d_rel_table, float* d_rel_scratch, int rel_buckets, const int* lut,
                   int lut_half, const int64_t* kmask, int B, int H, int Lq, int Lk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                   int causal, const uint32_t* rng_state, uint32_t site, float drop_p, void* stream) {
  return p5_op_attn_bwd_dot(dtype, Q, K, V, O, dO, lse, Dvec, dQ, dK, dV, rel_table, d_rel_table, d_rel_scratch, rel_buckets, lut, lut_half, kmask, B, H, Lq, Lk,
                            ldq, ldk, ldv, ldo, lddq, lddk, lddv, causal, rng_state, site, drop_p, nullptr, stream);
}
int p5_op_attn_bwd_dot(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse, float* Dvec,
                       void* dQ, void* dK, void* dV, const float* rel_table, float* d_rel_table, float* d_rel_scratch, int rel_buckets, const int* lut,
                       int lut_half, const int64_t* kmask, int B, int H, int Lq, int Lk, int ldq, int ldk, int ldv, int ldo, int lddq, int lddk, int lddv,
                       int causal, const uint32_t* rng_state, uint32_t site, float drop_p, float* dot_out, void* stream) {
  P5AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.dot_out = dot_out;
  a.Q = Q; a.K = K; a.V = V; a.O = (void*)O; a.dO = dO; a.lse = (float*)lse; a.Dvec = Dvec; a.dQ = dQ; a.dK = dK; a.dV = dV;
  a.rel_table = rel_table; a.d_rel_table = nullptr; a.bucket_lut = lut; a.lut_half = lut_half; a.kmask = kmask;
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.lddo = ldo; a.lddq = lddq; a.lddk = lddk;
  a.lddv = lddv; a.causal = causal; a.rel_copies = rel_buckets; a.rel_stride = rel_buckets * H; a.drop = op_drop(rng_state, site, drop_p);
  a.keep_bits = op_keep_bits(dtype, B, H, Lq, Lk, a.drop);
  hipStream_t s = (hipStream_t)stream;
  if (dot_out) P5_REQUIRE(p5l_attn_bwd_dot_ok(dtype == 1, a), "attn_bwd: dot_out is written by the fused bf16 self-attention backward only (Lq == Lk in 17..128)");
  if (d_rel_table) {
    P5_REQUIRE(d_rel_scratch && rel_buckets >= 1 && rel_buckets <= 64, "attn_bwd: d_rel_table needs d_rel_scratch [B * ceil(Lq / 64)][rel_buckets * H] and rel_buckets <= 64");
    a.d_rel_table = d_rel_scratch;
  }
  P5_TRY(dtype == 1 ? launch_attn_bwd<bf16>(a, s) : launch_attn_bwd<float>(a, s));
  if (d_rel_table) {
    P5_LAUNCH(p5_reduce_rows_kernel, dim3((rel_buckets * H + 15) / 16), dim3(256), 0, s, d_rel_table, (const float*)d_rel_scratch,
              p5l_attn_bwd_slots(dtype == 1, B, Lq, Lk), rel_buckets * H);
    P5_TRY(P5_KCHECK());
  }
  return 0;
}
int p5_op_ce_fwd(float* nll, float* lse, const float* logits, const int64_t* labels, int rows, int V, int ldl, void* stream) {
  P5_LAUNCH((p5_ce_fwd_kernel<float>), dim3(rows), dim3(256), 0, (hipStream_t)stream, nll, lse, logits, labels, V, ldl);
  return P5_KCHECK();
}
// ---- row kernels of p5_elem.h / p5_embed.h with everything their launchers take (tests/elem_matrix.py); launch geometry = the engine's ----
int p5_op_rmsnorm_fwd_drop(int dtype, void* y, float* rstd, const void* x, const float* w, int rows, int d, float eps, const uint32_t* rng_state,
                           uint32_t site, float drop_p, void* stream) {
  P5_REQUIRE(rows >= 1, "rmsnorm: rows");
  const P5Drop dp = op_drop(rng_state, site, drop_p);
  return dtype == 1 ? rmsnorm_fwd<bf16>((hipStream_t)stream, y, rstd, x, w, rows, d, eps, dp) : rmsnorm_fwd<float>((hipStream_t)stream, y, rstd, x, w, rows, d, eps, dp);
}
int p5_op_rmsnorm_bwd_full(int dtype, float* dres_out, void* dy_next, float* dw, const void* dy, const void* x, const float* w, const float* rstd,
                           const float* dres_in, int rows, int d, float* dw_partial, const uint32_t* rng_state, uint32_t site_in, float drop_in_p,
                           uint32_t site_next, float drop_next_p, const float* ssq_part, void* n_out, float eps, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(rows >= 1 && (rstd || ssq_part), "rmsnorm_bwd: rows; rstd or ssq_part");
  P5_REQUIRE(!ssq_part || d % 64 == 0, "rmsnorm_bwd: ssq_part holds one partial sum per 64 columns");
  const P5Drop din = op_drop(rng_state, site_in, drop_in_p), dnx = op_drop(rng_state, site_next, drop_next_p);
  int nblk = 0;
  P5_TRY(dtype == 1 ? rmsnorm_bwd<bf16>(s, dres_out, dy_next, dw, dy, x, w, rstd, dres_in, rows, d, din, dnx, dw_partial, &nblk, ssq_part, n_out, eps)
                    : rmsnorm_bwd<float>(s, dres_out, dy_next, dw, dy, x, w, rstd, dres_in, rows, d, din, dnx, dw_partial, &nblk, ssq_part, n_out, eps));
  if (dw_partial) {
    P5_LAUNCH(p5_reduce_rows_kernel, dim3((d + 15) / 16), dim3(256), 0, s, dw, (const float*)dw_partial, nblk, d);
    P5_TRY(P5_KCHECK());
  }
  return 0;
}
int p5_op_embed_fwd(int dtype, void* out, const void* E, const void* WW, const int64_t* ids, const int64_t* ww, int rows, int d,
                    const uint32_t* rng_state, uint32_t site, float drop_p, float* ssq_part, void* stream) {
  P5_REQUIRE(rows >= 1 && d % 64 == 0 && d <= 1024, "embed_fwd: d_model must be a multiple of 64, <= 1024");
  P5_REQUIRE(out && E && ids && (!WW || ww), "embed_fwd: null argument");
  const P5Drop dp = op_drop(rng_state, site, drop_p);
  if (dtype == 1) P5_LAUNCH((p5_embed_fwd_kernel<bf16>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (bf16*)out, (const bf16*)E, (const bf16*)WW, ids, ww, rows, d, dp, ssq_part);
  else P5_LAUNCH((p5_embed_fwd_kernel<float>), dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (float*)out, (const float*)E, (const float*)WW, ids, ww, rows, d, dp, ssq_part);
  return P5_KCHECK();
}
int p5_op_embed_bwd(int dtype, int mode, int nsets, int d, const P5EmbedBwdSet* sets, const uint32_t* rng_state, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(sets && nsets >= 1 && nsets <= P5_EMB_MAXSETS && d % 64 == 0 && d >= 64 && d <= 1024, "embed_bwd: 1..2 sets, d_model a multiple of 64, <= 1024");
  P5_REQUIRE(mode == 0 || mode == 1, "embed_bwd: mode 0 (atomic scatter) or 1 (fixed-order chain)");
  int n[P5_EMB_MAXSETS] = {};
  for (int k = 0; k < nsets; ++k) {
    const P5EmbedBwdSet& q = sets[k];
    n[k] = q.n0 + q.n1;
    P5_REQUIRE(q.n0 >= 0 && q.n1 >= 0 && n[k] >= 1 && q.table && (q.n0 == 0 || (q.key0 && q.dres0)) && (q.n1 == 0 || (q.key1 && q.dres1)), "embed_bwd: keys / rows / table");
    P5_REQUIRE(n[k] <= n[0], "embed_bwd: the first set sizes the grids, a later one may not be longer");
    P5_REQUIRE(mode == 0 || (q.idx && q.csort && q.part), "embed_bwd: the fixed-order chain needs idx / csort / part");
  }
  if (mode == 0) {      // the scatter of p5_set_option("embed_det", 0): one launch per key array
    for (int k = 0; k < nsets; ++k) {
      const P5EmbedBwdSet& q = sets[k];
      for (int h = 0; h < 2; ++h) {
        const int rows = h ? q.n1 : q.n0;
        if (rows == 0) continue;
        const P5Drop dp = h ? op_drop(rng_state, q.site1, q.drop_p1) : op_drop(rng_state, q.site0, q.drop_p0);
        const float* dres = h ? q.dres1 : q.dres0;
        const int64_t* key = h ? q.key1 : q.key0;
        if (dtype == 1) P5_LAUNCH((p5_embed_bwd_kernel<bf16>), dim3((rows + 3) / 4), dim3(256), 0, s, q.table, (float*)nullptr, dres, key, (const int64_t*)nullptr, rows, d, dp);
        else P5_LAUNCH((p5_embed_bwd_kernel<float>), dim3((rows + 3) / 4), dim3(256), 0, s, q.table, (float*)nullptr, dres, key, (const int64_t*)nullptr, rows, d, dp);
        P5_TRY(P5_KCHECK());
      }
    }
    return 0;
  }
  P5EmbArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.nsets = nsets; ea.d = d;
  for (int k = 0; k < nsets; ++k) {
    const P5EmbedBwdSet& q = sets[k];
    P5EmbSet& o = ea.s[k];
    o.key0 = q.key0; o.key1 = q.key1; o.dres0 = q.dres0; o.dres1 = q.dres1; o.n0 = q.n0; o.n1 = q.n1;
    o.drop0 = op_drop(rng_state, q.site0, q.drop_p0); o.drop1 = op_drop(rng_state, q.site1, q.drop_p1);
    o.table = q.table;
    o.perm = q.idx; o.skey = o.perm + n[k]; o.sstart = o.skey + n[k]; o.slen = o.sstart + n[k];
    o.part = q.part; o.csort = q.csort;
  }
  P5_LAUNCH(p5_embed_sortchunk_kernel, dim3((n[0] + P5_EMB_CHUNK - 1) / P5_EMB_CHUNK, nsets), dim3(256), 0, s, ea);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_embed_rank_kernel, dim3((n[0] + 63) / 64, nsets), dim3(256), 0, s, ea);
  P5_TRY(P5_KCHECK());
  const int nblk = (n[0] + P5_EMB_SEG - 1) / P5_EMB_SEG;
  P5_LAUNCH(p5_embed_seg_kernel, dim3(nblk, nsets), dim3(256), 0, s, ea);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_embed_fix_kernel, dim3(nblk, nsets), dim3(256), 0, s, ea);
  return P5_KCHECK();
}
int p5_op_ce_fwd_t(int dtype, float* nll, float* lse, const float* logits, const int64_t* labels, int rows, int V, int ldl, void* stream) {
  P5_REQUIRE(rows >= 1 && V >= 1 && ldl >= V && ldl % 4 == 0, "ce_fwd: ldl >= V, a multiple of 4");
  if (dtype == 1) P5_LAUNCH((p5_ce_fwd_kernel<bf16>), dim3(rows), dim3(256), 0, (hipStream_t)stream, nll, lse, logits, labels, V, ldl);
  else P5_LAUNCH((p5_ce_fwd_kernel<float>), dim3(rows), dim3(256), 0, (hipStream_t)stream, nll, lse, logits, labels, V, ldl);
  return P5_KCHECK();
}
int p5_op_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const int64_t* labels, const float* dnll, int rows, int V, int ldl,
                 int ldd, const int64_t* out_attn, int T, float gscale, int grid_y, float* g_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(rows >= 1 && V >= 1 && ldd >= V && ldl >= ldd && ldl % 8 == 0 && ldd % 8 == 0, "ce_bwd: V <= ldd <= ldl, both multiples of 8");
  P5_REQUIRE(dnll || (out_attn && T >= 1 && rows % T == 0), "ce_bwd: dnll, or out_attn [rows / T, T]");
  P5_REQUIRE(grid_y >= 1 && grid_y <= 8, "ce_bwd: 1..8 column slices");
  if (g_out) {
    P5_LAUNCH(p5_ce_gscale_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, g_out, labels, dnll, out_attn, T, gscale, rows);
    P5_TRY(P5_KCHECK());
  }
  if (dtype == 1) P5_LAUNCH((p5_ce_bwd_kernel<bf16>), dim3(rows, grid_y), dim3(256), 0, s, (bf16*)dlogits, logits, lse, labels, dnll, V, ldl, ldd, out_attn, T, gscale);
  else P5_LAUNCH((p5_ce_bwd_kernel<float>), dim3(rows, grid_y), dim3(256), 0, s, (float*)dlogits, logits, lse, labels, dnll, V, ldl, ldd, out_attn, T, gscale);
  return P5_KCHECK();
}
static int trie_ce_args(P5TrieCe* tr, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words, float tau) {
  P5_REQUIRE(child_off && child_tok && child_node, "trie_ce: trie");
  P5_REQUIRE(tau > 0.f && tau < __builtin_huge_valf(), "trie_ce: temperature > 0");
  P5_REQUIRE(excl_words >= 0 && (excluded || excl_words == 0), "trie_ce: excluded / excl_words");
  *tr = P5TrieCe{child_off, child_tok, child_node, excl_words > 0 ? excluded : nullptr, excl_words, tau};
  return 0;
}
int p5_op_trie_walk(int* node, int* state, const int64_t* labels, const int* child_off, const int* child_tok, const int* child_node,
                    const uint32_t* excluded, int excl_words, int B, int T, int start_id, int eos_id, void* stream) {
  P5_REQUIRE(node && state && labels && B >= 1 && T >= 1, "trie_walk: arguments");
  P5TrieCe tr;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, 1.f));
  P5_LAUNCH(p5_trie_walk_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, node, state, (int*)nullptr, labels, tr, T, start_id, eos_id);
  return P5_KCHECK();
}
// (child_col: the compact row of the restricted item head, p5_op_*_cols below; nullptr = the dense row, column = token)
static int op_trie_ce_fwd(int dtype, float* nll, float* lse, const float* logits, const int64_t* labels, const int* node, const int* state,
                          const int* child_off, const int* child_tok, const int* child_node, const int* child_col, const uint32_t* excluded, int excl_words,
                          float temperature, int rows, int T, int ldl, void* stream) {
  P5_REQUIRE(nll && lse && logits && labels && node && state && rows >= 1 && T >= 1 && rows % T == 0 && ldl >= 1, "trie_ce_fwd: arguments");
  P5TrieCe tr;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, temperature));
  tr.col = child_col;
  if (dtype == 1) P5_LAUNCH((p5_trie_ce_fwd_kernel<bf16>), dim3(rows), dim3(256), 0, (hipStream_t)stream, nll, lse, logits, labels, node, state, tr, T, ldl);
  else P5_LAUNCH((p5_trie_ce_fwd_kernel<float>), dim3(rows), dim3(256), 0, (hipStream_t)stream, nll, lse, logits, labels, node, state, tr, T, ldl);
  return P5_KCHECK();
}
int p5_op_trie_ce_fwd(int dtype, float* nll, float* lse, const float* logits, const int64_t* labels, const int* node, const int* state,
                      const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words, float temperature,
                      int rows, int T, int ldl, void* stream) {
  return op_trie_ce_fwd(dtype, nll, lse, logits, labels, node, state, child_off, child_tok, child_node, nullptr, excluded, excl_words, temperature, rows, T,
                        ldl, stream);
}
static int op_trie_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const int64_t* labels, const int* node, const int* state,
                          const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                          const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn,
                          float gscale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(dlogits && logits && lse && labels && node && state && rows >= 1 && T >= 1 && rows % T == 0, "trie_ce_bwd: arguments");
  P5_REQUIRE(ldl >= 1 && ldd >= 1 && ldd % 8 == 0, "trie_ce_bwd: ldd a multiple of 8");
  P5_REQUIRE(dnll || out_attn, "trie_ce_bwd: dnll, or out_attn [rows / T, T]");
  P5TrieCe tr;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, temperature));
  tr.col = child_col;
  if (dtype == 1) P5_LAUNCH((p5_trie_ce_bwd_kernel<bf16>), dim3(rows), dim3(256), 0, s, (bf16*)dlogits, logits, lse, labels, node, state, dnll, tr, ldl, ldd, out_attn, T, gscale);
  else P5_LAUNCH((p5_trie_ce_bwd_kernel<float>), dim3(rows), dim3(256), 0, s, (float*)dlogits, logits, lse, labels, node, state, dnll, tr, ldl, ldd, out_attn, T, gscale);
  return P5_KCHECK();
}
int p5_op_trie_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const int64_t* labels, const int* node, const int* state,
                      const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words,
                      float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn, float gscale, void* stream) {
  return op_trie_ce_bwd(dtype, dlogits, logits, lse, labels, node, state, dnll, child_off, child_tok, child_node, nullptr, excluded, excl_words, temperature,
                        rows, T, ldl, ldd, out_attn, gscale, stream);
}
static int trunc_ce_args(P5TruncCe* tc, int top_k, float top_p) {
  P5_REQUIRE(top_k >= 0, "trunc: top_k >= 0 (0 = off)");
  P5_REQUIRE(top_p > 0.f && top_p <= 1.f, "trunc: 0 < top_p <= 1 (1 = off)");
  *tc = P5TruncCe{top_k, top_p};
  return 0;
}
int p5_op_trunc_cut(float* cut, int* kept, const float* logits, const int* node, const int* child_off, const int* child_tok, const int* child_node,
                    const uint32_t* excluded, int excl_words, float temperature, int top_k, float top_p, int rows, int rows_per_user, int ldl,
                    void* stream) {
  P5_REQUIRE(cut && kept && logits && node && rows >= 1 && rows_per_user >= 1 && rows % rows_per_user == 0 && ldl >= 1, "trunc_cut: arguments");
  P5TrieCe tr;
  P5TruncCe tc;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, temperature));
  P5_TRY(trunc_ce_args(&tc, top_k, top_p));
  P5_LAUNCH(p5_trunc_cut_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, cut, kept, logits, node, tr, tc, rows_per_user, ldl);
  return P5_KCHECK();
}
static int op_trunc_ce_fwd(int dtype, float* nll, float* lse, float* row_cut, int* state, const float* logits, const int64_t* labels, const int* node,
                           const int* child_off, const int* child_tok, const int* child_node, const int* child_col, const uint32_t* excluded,
                           int excl_words, float temperature, int top_k, float top_p, int rows, int T, int ldl, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(nll && lse && row_cut && state && logits && labels && node && rows >= 1 && T >= 1 && rows % T == 0 && ldl >= 1, "trunc_ce_fwd: arguments");
  P5TrieCe tr;
  P5TruncCe tc;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, temperature));
  tr.col = child_col;
  P5_TRY(trunc_ce_args(&tc, top_k, top_p));
  if (dtype == 1) P5_LAUNCH((p5_trunc_ce_fwd_kernel<bf16>), dim3(rows), dim3(256), 0, s, nll, lse, row_cut, state, (int*)nullptr, logits, labels, node, tr, tc, T, ldl);
  else P5_LAUNCH((p5_trunc_ce_fwd_kernel<float>), dim3(rows), dim3(256), 0, s, nll, lse, row_cut, state, (int*)nullptr, logits, labels, node, tr, tc, T, ldl);
  return P5_KCHECK();
}
int p5_op_trunc_ce_fwd(int dtype, float* nll, float* lse, float* row_cut, int* state, const float* logits, const int64_t* labels, const int* node,
                       const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words, float temperature,
                       int top_k, float top_p, int rows, int T, int ldl, void* stream) {
  return op_trunc_ce_fwd(dtype, nll, lse, row_cut, state, logits, labels, node, child_off, child_tok, child_node, nullptr, excluded, excl_words, temperature,
                         top_k, top_p, rows, T, ldl, stream);
}
static int op_trunc_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const float* row_cut, const int64_t* labels, const int* node,
                           const int* state, const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                           const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn,
                           float gscale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(dlogits && logits && lse && row_cut && labels && node && state && rows >= 1 && T >= 1 && rows % T == 0, "trunc_ce_bwd: arguments");
  P5_REQUIRE(ldl >= 1 && ldd >= 1 && ldd % 8 == 0, "trunc_ce_bwd: ldd a multiple of 8");
  P5_REQUIRE(dnll || out_attn, "trunc_ce_bwd: dnll, or out_attn [rows / T, T]");
  P5TrieCe tr;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, temperature));
  tr.col = child_col;
  if (dtype == 1) P5_LAUNCH((p5_trunc_ce_bwd_kernel<bf16>), dim3(rows), dim3(256), 0, s, (bf16*)dlogits, logits, lse, row_cut, labels, node, state, dnll, tr, ldl, ldd, out_attn, T, gscale);
  else P5_LAUNCH((p5_trunc_ce_bwd_kernel<float>), dim3(rows), dim3(256), 0, s, (float*)dlogits, logits, lse, row_cut, labels, node, state, dnll, tr, ldl, ldd, out_attn, T, gscale);
  return P5_KCHECK();
}
int p5_op_trunc_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const float* row_cut, const int64_t* labels, const int* node,
                       const int* state, const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded,
                       int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn, float gscale, void* stream) {
  return op_trunc_ce_bwd(dtype, dlogits, logits, lse, row_cut, labels, node, state, dnll, child_off, child_tok, child_node, nullptr, excluded, excl_words,
                         temperature, rows, T, ldl, ldd, out_attn, gscale, stream);
}
// ---- the restricted item head (p5_item_head.h), kernel by kernel ----
int p5_op_item_gather(int dtype, void* EU, const void* E, const int* tokens, int n_tokens, int d, void* stream) {
  P5_REQUIRE(EU && E && tokens && n_tokens >= 1 && d >= 1, "item_gather: arguments");
  P5_REQUIRE(d % (dtype == 1 ? 8 : 4) == 0 && ((uintptr_t)EU % 16) == 0 && ((uintptr_t)E % 16) == 0, "item_gather: rows of whole 16-byte pieces, 16-byte aligned");
  const int Nup = (n_tokens + 63) / 64 * 64;
  if (dtype == 1) P5_LAUNCH((p5_item_gather_kernel<bf16>), dim3(item_head_blocks((long long)Nup * (d / 8))), dim3(256), 0, (hipStream_t)stream, (bf16*)EU, (const bf16*)E, tokens, n_tokens, Nup, d);
  else P5_LAUNCH((p5_item_gather_kernel<float>), dim3(item_head_blocks((long long)Nup * (d / 4))), dim3(256), 0, (hipStream_t)stream, (float*)EU, (const float*)E, tokens, n_tokens, Nup, d);
  return P5_KCHECK();
}
int p5_op_item_scatter(float* dE, const float* dEU, const int* tokens, int n_tokens, int V, int d, int store, void* stream) {
  P5_REQUIRE(dE && dEU && tokens && n_tokens >= 1 && n_tokens <= V && d >= 1, "item_scatter: arguments");
  P5_REQUIRE(d % 4 == 0 && ((uintptr_t)dE % 16) == 0 && ((uintptr_t)dEU % 16) == 0, "item_scatter: rows of whole 16-byte pieces, 16-byte aligned");
  P5_LAUNCH(p5_item_scatter_kernel, dim3(item_head_blocks((long long)(store ? V : n_tokens) * (d / 4))), dim3(256), 0, (hipStream_t)stream, dE, dEU, tokens, n_tokens,
            V, d, store ? 1 : 0);
  return P5_KCHECK();
}
int p5_op_trie_ce_fwd_cols(int dtype, float* nll, float* lse, const float* logits, const int64_t* labels, const int* node, const int* state,
                           const int* child_off, const int* child_tok, const int* child_node, const int* child_col, const uint32_t* excluded, int excl_words,
                           float temperature, int rows, int T, int ldl, void* stream) {
  P5_REQUIRE(child_col, "trie_ce_fwd_cols: child_col");
  return op_trie_ce_fwd(dtype, nll, lse, logits, labels, node, state, child_off, child_tok, child_node, child_col, excluded, excl_words, temperature, rows, T,
                        ldl, stream);
}
int p5_op_trie_ce_bwd_cols(int dtype, void* dlogits, const float* logits, const float* lse, const int64_t* labels, const int* node, const int* state,
                           const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                           const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn,
                           float gscale, void* stream) {
  P5_REQUIRE(child_col, "trie_ce_bwd_cols: child_col");
  return op_trie_ce_bwd(dtype, dlogits, logits, lse, labels, node, state, dnll, child_off, child_tok, child_node, child_col, excluded, excl_words, temperature,
                        rows, T, ldl, ldd, out_attn, gscale, stream);
}
int p5_op_trie_reg_fwd(int dtype, float* nll, float* lse, float* entropy, float* kl, float* lse_ref, const float* logits, const float* ref_logits,
                       const int64_t* labels, const int* node, const int* state, const int* child_off, const int* child_tok, const int* child_node,
                       const int* child_col, const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ld_ref,
                       void* stream) {
  P5_REQUIRE(nll && lse && entropy && logits && labels && node && state && rows >= 1 && T >= 1 && rows % T == 0 && ldl >= 1, "trie_reg_fwd: arguments");
  P5_REQUIRE(!ref_logits || (kl && lse_ref && ld_ref >= 1), "trie_reg_fwd: ref_logits needs kl, lse_ref and ld_ref");
  P5TrieCe tr;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, temperature));
  tr.col = child_col;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 1) P5_LAUNCH((p5_trie_reg_fwd_kernel<bf16>), dim3(rows), dim3(256), 0, s, nll, lse, entropy, kl, lse_ref, logits, ref_logits, labels, node, state, tr, T, ldl, ld_ref);
  else P5_LAUNCH((p5_trie_reg_fwd_kernel<float>), dim3(rows), dim3(256), 0, s, nll, lse, entropy, kl, lse_ref, logits, ref_logits, labels, node, state, tr, T, ldl, ld_ref);
  return P5_KCHECK();
}
int p5_op_trie_reg_bwd(int dtype, void* dlogits, const float* logits, const float* ref_logits, const float* lse, const float* entropy, const float* kl,
                       const float* lse_ref, const int64_t* labels, const int* node, const int* state, const float* dnll, const float* d_entropy,
                       const float* d_kl, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                       const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ld_ref, int ldd,
                       const int64_t* out_attn, float gscale, float entropy_coef, float kl_coef, void* stream) {
  P5_REQUIRE(dlogits && logits && lse && entropy && labels && node && state && rows >= 1 && T >= 1 && rows % T == 0, "trie_reg_bwd: arguments");
  P5_REQUIRE(ldl >= 1 && ldd >= 1 && ldd % 8 == 0, "trie_reg_bwd: ldd a multiple of 8");
  P5_REQUIRE(dnll || out_attn, "trie_reg_bwd: dnll, or out_attn [rows / T, T]");
  P5_REQUIRE(!ref_logits || (kl && lse_ref && ld_ref >= 1), "trie_reg_bwd: ref_logits needs kl, lse_ref and ld_ref");
  P5TrieCe tr;
  P5_TRY(trie_ce_args(&tr, child_off, child_tok, child_node, excluded, excl_words, temperature));
  tr.col = child_col;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 1) P5_LAUNCH((p5_trie_reg_bwd_kernel<bf16>), dim3(rows), dim3(256), 0, s, (bf16*)dlogits, logits, ref_logits, lse, entropy, kl, lse_ref, labels, node, state, dnll, d_entropy, d_kl, tr, ldl, ld_ref, ldd, out_attn, T, gscale, entropy_coef, kl_coef);
  else P5_LAUNCH((p5_trie_reg_bwd_kernel<float>), dim3(rows), dim3(256), 0, s, (float*)dlogits, logits, ref_logits, lse, entropy, kl, lse_ref, labels, node, state, dnll, d_entropy, d_kl, tr, ldl, ld_ref, ldd, out_attn, T, gscale, entropy_coef, kl_coef);
  return P5_KCHECK();
}
int p5_op_trunc_ce_fwd_cols(int dtype, float* nll, float* lse, float* row_cut, int* state, const float* logits, const int64_t* labels, const int* node,
                            const int* child_off, const int* child_tok, const int* child_node, const int* child_col, const uint32_t* excluded,
                            int excl_words, float temperature, int top_k, float top_p, int rows, int T, int ldl, void* stream) {
  P5_REQUIRE(child_col, "trunc_ce_fwd_cols: child_col");
  return op_trunc_ce_fwd(dtype, nll, lse, row_cut, state, logits, labels, node, child_off, child_tok, child_node, child_col, excluded, excl_words, temperature,
                         top_k, top_p, rows, T, ldl, stream);
}
int p5_op_trunc_ce_bwd_cols(int dtype, void* dlogits, const float* logits, const float* lse, const float* row_cut, const int64_t* labels, const int* node,
                            const int* state, const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                            const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn,
                            float gscale, void* stream) {
  P5_REQUIRE(child_col, "trunc_ce_bwd_cols: child_col");
  return op_trunc_ce_bwd(dtype, dlogits, logits, lse, row_cut, labels, node, state, dnll, child_off, child_tok, child_node, child_col, excluded, excl_words,
                         temperature, rows, T, ldl, ldd, out_attn, gscale, stream);
}
int p5_op_masked_mean(float* loss, const float* nll, const int64_t* out_attn, int B, int T, void* stream) {
  P5_REQUIRE(loss && nll && out_attn && B >= 1 && T >= 1, "masked_mean: arguments");
  P5_LAUNCH(p5_masked_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss, nll, out_attn, B, T);
  return P5_KCHECK();
}
int p5_op_masked_mean_g(int merged, float* loss, float* g_out, const float* nll, const int64_t* out_attn, const int64_t* labels, const float* tw, int B, int T,
                        float gscale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(loss && g_out && nll && out_attn && labels && B >= 1 && T >= 1, "masked_mean_g: arguments");
  if (merged) {
    P5_LAUNCH(p5_masked_mean_g_kernel, dim3(1), dim3(256), 0, s, loss, g_out, nll, out_attn, labels, B, T, gscale, tw);
    return P5_KCHECK();
  }
  P5_LAUNCH(p5_masked_mean_kernel, dim3(1), dim3(256), 0, s, loss, nll, out_attn, B, T, tw);
  P5_TRY(P5_KCHECK());
  P5_LAUNCH(p5_ce_gscale_kernel, dim3((B * T + 255) / 256), dim3(256), 0, s, g_out, labels, (const float*)nullptr, out_attn, T, gscale, B * T, tw);
  return P5_KCHECK();
}
// the preference objective (p5_pref.h) behind a given per-token NLL: both launches, no engine
int p5_op_pref_objective(float* loss, float* row_seed, float* user_partials, float* pref_stats, const float* nll, const float* ref_logprobs,
                         const int64_t* out_attn, const int64_t* labels, const int* pref_mask, int kind, float beta, int depth, int length_normalize,
                         float sft_coef, int B, int G, int T, void* stream) {
  P5_TRY(pref_params_ok(kind, beta, depth, sft_coef));
  P5_REQUIRE(loss && row_seed && user_partials && pref_stats && nll && out_attn && labels, "preference objective: null pointer argument");
  P5_REQUIRE(B >= 1 && G >= 1 && G <= P5_PREF_MAX_G && T >= 1 && (int64_t)B * G * T <= ((int64_t)1 << 30),
             "preference objective: shapes B, G, T >= 1, G <= 512, B * G * T <= 2^30");
  return launch_pref((hipStream_t)stream, loss, row_seed, user_partials, pref_stats, nll, ref_logprobs, out_attn, labels, pref_mask, kind, beta, depth,
                     length_normalize, sft_coef, B, G, T);
}
// the clipped-ratio objective (p5_clip.h) behind a given per-token NLL: both launches, no engine
int p5_op_clip_objective(float* loss, float* terms, float* row_seed, float* user_partials, float* clip_stats, const float* nll, const float* old_logprobs,
                         const int64_t* out_attn, const int64_t* labels, const float* tw, const int* target_mode, const float* entropy_rows,
                         const float* kl_rows, float entropy_coef, float kl_coef, float eps_low, float eps_high, int ratio_mode, int B, int G, int T,
                         void* stream) {
  P5_TRY(clip_params_ok(eps_low, eps_high, ratio_mode));
  P5_REQUIRE(loss && row_seed && user_partials && clip_stats && nll && old_logprobs && out_attn && labels, "clip objective: null pointer argument");
  P5_REQUIRE(B >= 1 && G >= 1 && T >= 1 && (int64_t)B * G * T <= ((int64_t)1 << 30), "clip objective: shapes B, G, T >= 1, B * G * T <= 2^30");
  P5_REQUIRE(entropy_rows || !kl_rows, "clip objective: kl_rows needs entropy_rows");
  return launch_clip((hipStream_t)stream, loss, terms, row_seed, user_partials, clip_stats, nll, old_logprobs, out_attn, labels, tw, target_mode, entropy_rows,
                     kl_rows, entropy_coef, kl_coef, eps_low, eps_high, ratio_mode, B, G, T);
}
static int policy_batch_impl(const int64_t* sequences, const int64_t* labels, const int64_t* output_attention, const float* rewards, int B, int S, int Ts, int Tg,
                    int baseline, float policy_coef, float sft_coef, int token_sum, float adv_eps, int with_gold, int pad_id, int eos_id,
                    int64_t* labels_out, int64_t* attention_out, float* rewards_out, float* advantages, float* weights_out, float* user_stats,
                    float* stats, const float* token_lp, float* old_lp_out, int* mode_out, void* stream) {
  P5_REQUIRE(sequences && labels && output_attention, "policy_batch: null input pointer (sequences, labels, output_attention)");
  P5_REQUIRE(labels_out && attention_out && rewards_out && advantages && weights_out && user_stats && stats, "policy_batch: null output pointer");
  P5_REQUIRE(B >= 1 && Ts >= 2 && Tg >= 1 && Tg <= (1 << 24), "policy_batch: shapes B >= 1, Ts >= 2, 1 <= Tg <= 2^24");
  P5_REQUIRE(S >= 1, "policy_batch: S >= 1 draws per user");
  P5_REQUIRE(S <= P5_POLICY_MAX_S, "policy_batch: S <= 1024 draws per user");
  P5_REQUIRE(baseline >= P5_BASELINE_NONE && baseline <= P5_BASELINE_GRPO, "policy_batch: unknown baseline (0 none, 1 mean, 2 loo, 3 grpo)");
  P5_REQUIRE(baseline != P5_BASELINE_LOO || S >= 2, "policy_batch: the loo baseline needs S >= 2");
  P5_REQUIRE(std::isfinite(policy_coef) && std::isfinite(sft_coef) && std::isfinite(adv_eps) && adv_eps >= 0.f, "policy_batch: non-finite coefficient (policy_coef, sft_coef, adv_eps)");
  P5_REQUIRE((token_sum == 0 || token_sum == 1) && (with_gold == 0 || with_gold == 1), "policy_batch: token_sum and with_gold are 0 or 1");
  P5PolicyArgs a;
  a.seq = sequences; a.labels = labels; a.out_attn = output_attention; a.rewards = rewards;
  a.labels_out = labels_out; a.attn_out = attention_out; a.rewards_out = rewards_out; a.adv = advantages; a.weights = weights_out; a.user_stats = user_stats;
  a.S = S; a.Ts = Ts; a.Tg = Tg; a.To = Tg > Ts - 1 ? Tg : Ts - 1; a.baseline = baseline; a.token_sum = token_sum; a.with_gold = with_gold;
  a.pad_id = pad_id; a.eos_id = eos_id; a.policy_coef = policy_coef; a.sft_coef = sft_coef; a.adv_eps = adv_eps;
  a.token_lp = token_lp; a.old_lp_out = old_lp_out; a.mode_out = mode_out;
  P5_REQUIRE((int64_t)(S + with_gold) * a.To <= (int64_t)1 << 30, "policy_batch: G * To too large");
  hipStream_t s = (hipStream_t)stream;
  P5_LAUNCH(p5_policy_batch_kernel, dim3(B), dim3(256), 0, s, a);
  P5_LAUNCH(p5_policy_stats_kernel, dim3(1), dim3(256), 0, s, stats, user_stats, B);
  return P5_KCHECK();
}
// the batch of an on-policy step from the sampler's output (p5_policy.h): both launches, stateless
int p5_policy_batch(const int64_t* sequences, const int64_t* labels, const int64_t* output_attention, const float* rewards, int B, int S, int Ts, int Tg,
                    int baseline, float policy_coef, float sft_coef, int token_sum, float adv_eps, int with_gold, int pad_id, int eos_id,
                    int64_t* labels_out, int64_t* attention_out, float* rewards_out, float* advantages, float* weights_out, float* user_stats,
                    float* stats, void* stream) {
  return policy_batch_impl(sequences, labels, output_attention, rewards, B, S, Ts, Tg, baseline, policy_coef, sft_coef, token_sum, adv_eps, with_gold, pad_id,
                           eos_id, labels_out, attention_out, rewards_out, advantages, weights_out, user_stats, stats, nullptr, nullptr, nullptr, stream);
}
// ... and the clipped objective's two inputs: old_logprobs_out fp32 [B, G, To] gathered from the sampler's token_logprobs [B * S, Ts - 1], target_mode_out int32 [B, G]
int p5_policy_batch_clip(const int64_t* sequences, const int64_t* labels, const int64_t* output_attention, const float* rewards, const float* token_logprobs,
                         int B, int S, int Ts, int Tg, int baseline, float policy_coef, float sft_coef, int token_sum, float adv_eps, int with_gold, int pad_id,
                         int eos_id, int64_t* labels_out, int64_t* attention_out, float* rewards_out, float* advantages, float* weights_out, float* user_stats,
                         float* stats, float* old_logprobs_out, int* target_mode_out, void* stream) {
  P5_REQUIRE(token_logprobs && old_logprobs_out && target_mode_out, "policy_batch_clip: null pointer (token_logprobs, old_logprobs_out, target_mode_out)");
  return policy_batch_impl(sequences, labels, output_attention, rewards, B, S, Ts, Tg, baseline, policy_coef, sft_coef, token_sum, adv_eps, with_gold, pad_id,
                           eos_id, labels_out, attention_out, rewards_out, advantages, weights_out, user_stats, stats, token_logprobs, old_logprobs_out,
                           target_mode_out, stream);
}
// the batch of an on-policy step from slates (p5_slate_policy.h): the importance-weighted without-replacement estimator; both launches, stateless
int p5_policy_slate_batch(const int64_t* sequences, const float* sequences_logprob, const float* perturbed, const int64_t* labels,
                          const int64_t* output_attention, const float* rewards, const float* token_logprobs, int B, int S, int K1, int Ts, int Tg,
                          int estimator, float policy_coef, float sft_coef, int token_sum, int with_gold, int pad_id, int eos_id, int64_t* labels_out,
                          int64_t* attention_out, float* rewards_out, float* advantages, float* importance, float* weights_out, float* slate_stats,
                          float* user_stats, float* stats, float* old_logprobs_out, int* target_mode_out, const int* root_streams, uint32_t root_seed,
                          uint32_t slate_base, void* stream) {
  P5_REQUIRE(sequences && sequences_logprob && perturbed && labels && output_attention,
             "policy_slate_batch: null input pointer (sequences, sequences_logprob, perturbed, labels, output_attention)");
  P5_REQUIRE(labels_out && attention_out && rewards_out && advantages && importance && weights_out && slate_stats && user_stats && stats,
             "policy_slate_batch: null output pointer");
  P5_REQUIRE((token_logprobs != nullptr) == (old_logprobs_out != nullptr), "policy_slate_batch: token_logprobs and old_logprobs_out go together (both or neither)");
  P5_REQUIRE(B >= 1 && Tg >= 1 && Tg <= (1 << 24), "policy_slate_batch: shapes B >= 1, 1 <= Tg <= 2^24");
  P5_REQUIRE(Ts >= 2, "policy_slate_batch: Ts >= 2 (the decoder start and at least one token)");
  P5_REQUIRE(S >= 1, "policy_slate_batch: S >= 1 slates per user");
  P5_REQUIRE(K1 >= 2, "policy_slate_batch: K1 >= 2 (K >= 1 used slots and the threshold slot)");
  P5_REQUIRE((int64_t)S * K1 <= P5_SLATE_POLICY_MAX_SLOTS, "policy_slate_batch: S * K1 <= 1024 slots per user");
  P5_REQUIRE(estimator == P5_SLATE_UNBIASED || estimator == P5_SLATE_NORMALIZED, "policy_slate_batch: unknown estimator (0 unbiased, 1 normalized)");
  P5_REQUIRE(estimator != P5_SLATE_NORMALIZED || K1 >= 3, "policy_slate_batch: the normalized estimator needs K >= 2 (K1 >= 3)");
  P5_REQUIRE(std::isfinite(policy_coef) && std::isfinite(sft_coef), "policy_slate_batch: non-finite coefficient (policy_coef, sft_coef)");
  P5_REQUIRE((token_sum == 0 || token_sum == 1) && (with_gold == 0 || with_gold == 1), "policy_slate_batch: token_sum and with_gold are 0 or 1");
  P5SlatePolicyArgs a;
  a.seq = sequences; a.logp = sequences_logprob; a.pert = perturbed; a.labels = labels; a.out_attn = output_attention; a.rewards = rewards;
  a.token_lp = token_logprobs; a.labels_out = labels_out; a.attn_out = attention_out; a.rewards_out = rewards_out; a.adv = advantages;
  a.importance = importance; a.weights = weights_out; a.slate_stats = slate_stats; a.user_stats = user_stats; a.old_lp_out = old_logprobs_out;
  a.mode_out = target_mode_out; a.streams = root_streams; a.seed = root_seed; a.slate_base = slate_base;
  a.S = S; a.K1 = K1; a.Ts = Ts; a.Tg = Tg; a.To = Tg > Ts - 1 ? Tg : Ts - 1; a.estimator = estimator; a.token_sum = token_sum; a.with_gold = with_gold;
  a.pad_id = pad_id; a.eos_id = eos_id; a.policy_coef = policy_coef; a.sft_coef = sft_coef;
  P5_REQUIRE((int64_t)(S * (K1 - 1) + with_gold) * a.To <= (int64_t)1 << 30, "policy_slate_batch: G * To too large");
  hipStream_t s = (hipStream_t)stream;
  P5_LAUNCH(p5_policy_slate_batch_kernel, dim3(B), dim3(256), 0, s, a);
  P5_LAUNCH(p5_policy_slate_stats_kernel, dim3(1), dim3(256), 0, s, stats, user_stats, B);
  return P5_KCHECK();
}
int p5_op_skinny_gemm(int dtype, int amode, const void* A, int lda, const float* ln, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                      int epi, float alpha, float eps, void* stream) {
  return dtype == 1 ? skinny<bf16>((hipStream_t)stream, amode, A, lda, ln, (const bf16*)W, ldw, C, ldc, M, N, K, epi, alpha, eps, nullptr)
                    : skinny<float>((hipStream_t)stream, amode, A, lda, ln, (const float*)W, ldw, C, ldc, M, N, K, epi, alpha, eps, nullptr);
}
// single-token cross-attention of R = B * Kb beam rows (q given, not fused): variant 3 = MFMA kernel, 2 = scalar kernel
int p5_op_dec_cross_attn(int dtype, int variant, void* out, const void* q, const void* kv, const int64_t* mask, int B, int H, int Kb, int L,
                         void* stream) {
  return p5_op_dec_cross_attn_ex(dtype, variant, out, q, nullptr, nullptr, nullptr, kv, 2 * H * 64, mask, B, H, Kb, L, 0, 0.f, nullptr, stream);
}
// ---- kernels of the decode step (p5_decode2.h, p5_decode.h) through the launchers the engine uses (tests/decode_matrix.py) ----
int p5_op_dec_cross_attn_ex(int dtype, int variant, void* out, const void* q, const float* x, const float* ln, const void* Wq, const void* kv, int ldkv,
                            const int64_t* mask, int B, int H, int Kb, int L, int d, float eps, const int* done, void* stream) {
  P5CrossArgs a;
  memset(&a, 0, sizeof(a));
  a.out = out; a.q = q; a.x = x; a.ln = ln; a.Wq = Wq; a.kv = kv; a.ldkv = ldkv; a.mask = mask; a.R = B * Kb; a.H = H; a.Kb = Kb; a.L = L; a.d = d; a.eps = eps;
  a.done = done;
  const bool fuseq = x != nullptr;
  P5_REQUIRE(!fuseq || dtype == 1, "dec_cross_attn: the fused q projection exists in bf16 only");
  return dtype == 1 ? launch_dec_cross<bf16>(a, B, variant, fuseq, (hipStream_t)stream) : launch_dec_cross<float>(a, B, variant, fuseq, (hipStream_t)stream);
}
int p5_op_dec_self_attn(int dtype, void* out, const void* qkv, void* cache, const int* anc_odd, const int* anc_even, const float* rel_table, const int* lut,
                        int lut_half, int R, int H, const int* step, int max_len, const int* done, void* stream) {
  P5_REQUIRE(out && qkv && cache && anc_odd && anc_even && rel_table && lut && step, "dec_self_attn: null argument");
  hipStream_t s = (hipStream_t)stream;
  return dtype == 1 ? launch_dec_self_attn<bf16>(out, qkv, cache, anc_odd, anc_even, rel_table, lut, lut_half, R, H, step, max_len, done, s)
                    : launch_dec_self_attn<float>(out, qkv, cache, anc_odd, anc_even, rel_table, lut, lut_half, R, H, step, max_len, done, s);
}
int p5_op_rmsnorm_f32in(int dtype, void* y, const float* x, const float* w, int rows, int d, float eps, const int* done, void* stream) {
  P5_REQUIRE(y && x && w, "rmsnorm_f32in: null argument");
  return dtype == 1 ? launch_rmsnorm_f32in<bf16>(y, x, w, rows, d, eps, done, (hipStream_t)stream)
                    : launch_rmsnorm_f32in<float>(y, x, w, rows, d, eps, done, (hipStream_t)stream);
}
int p5_op_head_lse(int dtype, int nv, float* part_m, float* part_s, const void* hn, const void* E, int R, int d, int V, float alpha, const int* done,
                   void* stream) {
  P5_REQUIRE(part_m && part_s && hn && E, "head_lse: null argument");
  return dtype == 1 ? launch_head_lse_t<bf16>(nv, (const bf16*)E, d, V, part_m, part_s, hn, R, alpha, done, (hipStream_t)stream)
                    : launch_head_lse_t<float>(nv, (const float*)E, d, V, part_m, part_s, hn, R, alpha, done, (hipStream_t)stream);
}
int p5_op_dec_score(int dtype, int streaming, const float* part_m, const float* part_s, int ntiles, const void* hn, const void* E, int d, float alpha,
                    const float* logits, int ldl, int V, const int* node, const float* run_score, const int* child_off, const int* child_tok,
                    const int* child_node, const uint32_t* excluded, int excl_words, int R, int Kb, int max_c, int K2, float* cand_scratch,
                    float* top_score, int* top_c, int* n_top, const int* done, void* stream) {
  P5_REQUIRE(node && run_score && child_off && child_tok && child_node && top_score && top_c && n_top, "dec_score: null argument");
  P5_REQUIRE(streaming ? (part_m && part_s && hn && E) : logits != nullptr, "dec_score: the inputs of the chosen kernel");
  P5ScoreArgs a;
  a.part_m = part_m; a.part_s = part_s; a.ntiles = ntiles; a.hn = hn; a.E = E; a.d = d; a.alpha = alpha; a.logits = logits; a.ldl = ldl; a.V = V;
  a.node = node; a.run_score = run_score; a.child_off = child_off; a.child_tok = child_tok; a.child_node = child_node;
  a.excluded = excluded; a.excl_words = excluded ? excl_words : 0; a.Kb = Kb; a.max_c = max_c; a.K2 = K2;
  a.cand_scratch = cand_scratch; a.top_score = top_score; a.top_c = top_c; a.n_top = n_top; a.done = done;
  return dtype == 1 ? launch_dec_score<bf16>(streaming != 0, R, a, (hipStream_t)stream) : launch_dec_score<float>(streaming != 0, R, a, (hipStream_t)stream);
}
// ---- kernels of catalogue ranking (p5_rank.h, p5_cand.h, p5_prune.h, p5_bound.h, p5_tree_attn_row) through the launch helpers the engine
// uses (tests/rank_matrix.py) ----
static P5RankPlan op_rank_plan(const int* row_tok, const int* row_depth, const int* row_node, const int* anc, int rows, int max_depth, int B, int CQ, int nchunk) {
  P5RankPlan pl;
  pl.row_tok = row_tok; pl.row_depth = row_depth; pl.row_node = row_node; pl.anc = anc; pl.rows = rows; pl.max_depth = max_depth;
  pl.B = B; pl.CQ = CQ; pl.nchunk = nchunk;
  return pl;
}
int p5_op_head_nv(int dtype, int d_model) { return d_model >= 1 ? head_nv_of(dtype, d_model) : 0; }
int p5_op_rank_select(int items, float* scores, const float* edge_lp, int64_t n_edges, const int* item_edges, int n_items, int path_len,
                      const uint32_t* excluded, unsigned long long* part, int B, int top_n, int* out_index, float* out_score, int* grid, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(scores && B >= 1 && n_items >= 1 && (items == 2 || (part && out_index && out_score)), "rank_select: null argument");
  P5_REQUIRE(top_n >= 1 && top_n <= P5_WIDE_MAX_K, "rank_select: 1 <= top_n <= 4096");
  int G, S;
  rank_select_grid(n_items, top_n, G, S);
  if (grid) { grid[0] = G; grid[1] = S; }
  if (items) {
    P5_REQUIRE(edge_lp && item_edges && path_len >= 1, "rank_select: the item scores need edge_lp and item_edges");
    P5_TRY(rank_item_scores(scores, edge_lp, n_edges, item_edges, n_items, path_len, B, s));
    if (items == 2) return 0;
  }
  return rank_top_n(scores, n_items, excluded, part, G, S, B, top_n, out_index, out_score, s);
}
int p5_op_rank_edges(int dtype, int nv, float* edge_lp, int64_t n_edges, const void* hn, const void* E, int d, int V, float* head, int HC,
                     const int* row_node, int rows, int B, int CQ, int nchunk, const int* sel, const int* n_rows, int cap, const int* child_off,
                     const int* child_tok, void* stream) {
  P5_REQUIRE(edge_lp && hn && E && head && row_node && child_off && child_tok, "rank_edges: null argument");
  P5_REQUIRE(B >= 1 && CQ >= 1 && nchunk >= 1 && HC >= 1 && d >= 1 && V >= 1 && (sel == nullptr || n_rows != nullptr), "rank_edges: shape");
  P5_REQUIRE(d <= 1024 && d % (dtype == 1 ? 64 : 32) == 0, "rank_edges: d_model a multiple of 64 (bf16) / 32 (fp32), at most 1024");
  const P5RankPlan pl = op_rank_plan(nullptr, nullptr, row_node, nullptr, rows, 0, B, CQ, nchunk);
  const P5RankSel rs{sel, n_rows, cap};
  const int R = B * CQ * nchunk;
  return dtype == 1 ? rank_edges_t<bf16>((const bf16*)E, d, V, nv, edge_lp, n_edges, hn, head, HC, HC, R, pl, rs, child_off, child_tok, (hipStream_t)stream)
                    : rank_edges_t<float>((const float*)E, d, V, nv, edge_lp, n_edges, hn, head, HC, HC, R, pl, rs, child_off, child_tok, (hipStream_t)stream);
}
int p5_op_cand_row_lse(int dtype, int nv, float* row_lse, const void* hn, const void* E, int d, int V, float* head, int HC, int R, void* stream) {
  P5_REQUIRE(row_lse && hn && E && head && R >= 1 && HC >= 1 && d >= 1 && V >= 1, "cand_row_lse: null argument");
  return dtype == 1 ? cand_row_lse_t<bf16>((const bf16*)E, d, V, nv, row_lse, hn, head, HC, HC, R, (hipStream_t)stream)
                    : cand_row_lse_t<float>((const float*)E, d, V, nv, row_lse, hn, head, HC, HC, R, (hipStream_t)stream);
}
int p5_op_tree_attn(int dtype, int variant, void* out, const void* qkv, const int* row_depth, const int* anc, int rows, int max_depth, int B, int CQ, int nchunk,
                    const int* sel, const int* n_rows, int cap, const float* rel_table, const int* lut, int lut_half, int H, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(out && qkv && row_depth && anc && rel_table && lut && B >= 1 && CQ >= 1 && nchunk >= 1 && H >= 1, "tree_attn: null argument");
  P5_REQUIRE(variant >= 0 && variant <= 2 && (variant != 1 || (sel && n_rows)), "tree_attn: variant 0 rank, 1 cand (sel, n_rows), 2 verify");
  if (variant == 2) {         // the verification plan: [B][cap] rows, anc [B][cap][max_len]; row_depth = depth_flat [B * PU], PU = CQ
    P5_REQUIRE(nchunk == 1, "tree_attn: the verification pass has one chunk");
    P5VerifyPlan vp;
    memset(&vp, 0, sizeof(vp));
    vp.anc = const_cast<int*>(anc); vp.cap = cap; vp.max_len = max_depth;
    return dtype == 1 ? verify_tree_attn<bf16>((bf16*)out, (const bf16*)qkv, vp, row_depth, rel_table, lut, lut_half, B, CQ, H, s)
                      : verify_tree_attn<float>((float*)out, (const float*)qkv, vp, row_depth, rel_table, lut, lut_half, B, CQ, H, s);
  }
  P5CandPlan pl;
  pl.g = op_rank_plan(nullptr, row_depth, nullptr, anc, rows, max_depth, B, CQ, nchunk);
  pl.sel = sel; pl.n_rows = n_rows; pl.cap = cap;
  if (variant == 0)
    return dtype == 1 ? rank_tree_attn<bf16>((bf16*)out, (const bf16*)qkv, pl.g, rel_table, lut, lut_half, H, s)
                      : rank_tree_attn<float>((float*)out, (const float*)qkv, pl.g, rel_table, lut, lut_half, H, s);
  return dtype == 1 ? cand_tree_attn<bf16>((bf16*)out, (const bf16*)qkv, pl, rel_table, lut, lut_half, H, s)
                    : cand_tree_attn<float>((float*)out, (const float*)qkv, pl, rel_table, lut, lut_half, H, s);
}
int p5_op_cand_plan(int* sel, int* n_rows, int* hdr, unsigned long long* keys, const int* cand, const int* item_rows, int B, int C, int n_items, int path_len,
                    int cap, int P, void* stream) {
  P5_REQUIRE(sel && n_rows && hdr && keys && cand && item_rows && B >= 1 && n_items >= 1 && path_len >= 1, "cand_plan: null argument");
  P5_REQUIRE(C >= 1 && C <= P5_WIDE_MAX_K, "cand_plan: 1 <= C <= 4096");
  P5_REQUIRE(cap >= C * path_len && P >= 256 && P >= C * path_len && (P & (P - 1)) == 0, "cand_plan: cap >= C * path_len, P a power of two >= max(C * path_len, 256)");
  return cand_plan_rows(sel, n_rows, hdr, keys, cand, item_rows, B, C, n_items, path_len, cap, P, (hipStream_t)stream);
}
int p5_op_cand_rows(int64_t* ids, const int* row_tok, int B, int CQ, int nchunk, const int* sel, const int* n_rows, int cap, int pad_id, void* stream) {
  P5_REQUIRE(ids && row_tok && sel && n_rows && B >= 1 && CQ >= 1 && nchunk >= 1, "cand_rows: null argument");
  P5CandPlan pl;
  pl.g = op_rank_plan(row_tok, nullptr, nullptr, nullptr, 0, 0, B, CQ, nchunk);
  pl.sel = sel; pl.n_rows = n_rows; pl.cap = cap;
  return cand_pass_ids(ids, pl, pad_id, (hipStream_t)stream);
}
int p5_op_cand_score(int dtype, float* scores, const void* hn, const void* E, int d, const float* row_lse, int B, int CQ, int nchunk, const int* sel,
                     const int* n_rows, int cap, const int* cand, int C, const int* item_rows, const int64_t* item_tok, int ldt, int n_items, int path_len,
                     int* out_order, int* out_index, float* out_score, int top_n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  P5_REQUIRE(scores && hn && E && row_lse && sel && n_rows && cand && item_rows && item_tok && out_order && out_index && out_score, "cand_score: null argument");
  P5_REQUIRE(C >= 1 && C <= P5_WIDE_MAX_K && top_n >= 1 && top_n <= C, "cand_score: 1 <= top_n <= C <= 4096");
  P5_REQUIRE(d >= 1 && d % (dtype == 1 ? 64 : 32) == 0, "cand_score: d_model a multiple of 64 (bf16) / 32 (fp32)");
  P5CandPlan pl;
  pl.g = op_rank_plan(nullptr, nullptr, nullptr, nullptr, 0, 0, B, CQ, nchunk);
  pl.sel = sel; pl.n_rows = n_rows; pl.cap = cap;
  return dtype == 1 ? cand_score_order<bf16>(scores, (const bf16*)hn, (const bf16*)E, d, row_lse, pl, cand, C, item_rows, item_tok, ldt, n_items, path_len, out_order,
                                             out_index, out_score, top_n, s)
                    : cand_score_order<float>(scores, (const float*)hn, (const float*)E, d, row_lse, pl, cand, C, item_rows, item_tok, ldt, n_items, path_len, out_order,
                                              out_index, out_score, top_n, s);
}
int p5_op_prune_fill(float* p, int64_t n, float v, void* stream) {
  P5_REQUIRE(p && n >= 1, "prune_fill: null argument");
  return prune_fill(p, (size_t)n, v, (hipStream_t)stream);
}
int p5_op_prune_propose(int* sel, int* n_rows, int* hdr, const float* edge_lp, int64_t n_edges, const float* top_score, int N, const int* row_depth, const int* anc,
                        int rows, int max_depth, const int* row_edge, const int* row_lmax, float slack, int B, void* stream) {
  P5_REQUIRE(sel && n_rows && hdr && edge_lp && top_score && row_depth && anc && row_edge && row_lmax && N >= 1 && rows >= 1 && B >= 1, "prune_propose: null argument");
  const P5RankPlan pl = op_rank_plan(nullptr, row_depth, nullptr, anc, rows, max_depth, B, 0, 0);
  return prune_propose_rows(sel, n_rows, hdr, edge_lp, n_edges, top_score, N, pl, row_edge, row_lmax, slack, B, (hipStream_t)stream);
}
int p5_op_prune_mask(uint32_t* out, const uint32_t* excluded, const float* edge_lp, int64_t n_edges, const int* item_edges, int n_items, int path_len, int B,
                     void* stream) {
  P5_REQUIRE(out && edge_lp && item_edges && n_items >= 1 && path_len >= 1 && B >= 1, "prune_mask: null argument");
  return prune_mask(out, excluded, edge_lp, n_edges, item_edges, n_items, path_len, B, (hipStream_t)stream);
}
static P5CandPlan op_sel_plan(const int* row_depth, const int* row_node, const int* anc, int max_depth, int B, int CQ, int nchunk, const int* sel, const int* n_rows,
                              int cap) {
  P5CandPlan pl;
  pl.g = op_rank_plan(nullptr, row_depth, row_node, anc, CQ * nchunk, max_depth, B, CQ, nchunk);
  pl.sel = sel; pl.n_rows = n_rows; pl.cap = cap;
  return pl;
}
int p5_op_prune_certify(int* flagged, const float* edge_lp, int64_t n_edges, const int* row_depth, const int* row_node, const int* anc, int max_depth, int B, int CQ,
                        int nchunk, const int* sel, const int* n_rows, int cap, const int* row_edge, const int* edge_row, const int* row_lmax,
                        const int* child_off, const int* out_index, const float* out_score, int N, float margin, void* stream) {
  P5_REQUIRE(flagged && edge_lp && row_depth && row_node && anc && sel && n_rows && row_edge && edge_row && row_lmax && child_off && out_index && out_score,
             "prune_certify: null argument");
  P5_REQUIRE(B >= 1 && CQ >= 1 && nchunk >= 1 && N >= 1, "prune_certify: shape");
  return prune_certify(flagged, edge_lp, n_edges, op_sel_plan(row_depth, row_node, anc, max_depth, B, CQ, nchunk, sel, n_rows, cap), row_edge, edge_row, row_lmax,
                       child_off, out_index, out_score, N, margin, (hipStream_t)stream);
}
int p5_op_bound_seed(int* sel, int* n_rows, int* hdr, unsigned long long* keys, int KP, int cap, const int64_t* seeds, int S, int T, const int* child_off,
                     const int* child_tok, const int* edge_row, const int* row_tok, const int* row_node, int max_depth, int B, void* stream) {
  P5_REQUIRE(sel && n_rows && hdr && keys && seeds && child_off && child_tok && edge_row && row_tok && row_node, "bound_seed: null argument");
  P5_REQUIRE(S >= 1 && S <= P5_WIDE_MAX_K && T >= 1 && max_depth >= 1 && B >= 1 && cap >= 1, "bound_seed: 1 <= n_seeds <= 4096, seed_len >= 1");
  P5_REQUIRE(KP >= 256 && (KP & (KP - 1)) == 0 && (long long)KP >= (long long)S * max_depth + 1, "bound_seed: KP a power of two >= max(n_seeds * max_depth + 1, 256)");
  return bound_seed_rows(sel, n_rows, hdr, keys, KP, cap, seeds, S, T, child_off, child_tok, edge_row, row_tok, row_node, max_depth, B, (hipStream_t)stream);
}
int p5_op_bound_expand(int* sel, int* n_rows, int* grew, int* hdr, unsigned long long* keys, int KP, const float* edge_lp, int64_t n_edges, const int* row_depth,
                       const int* row_node, const int* anc, int max_depth, int B, int CQ, int nchunk, int cap, const int* row_edge, const int* edge_row,
                       const int* row_lmax, const int* child_off, const float* out_score, int N, float margin, void* stream) {
  P5_REQUIRE(sel && n_rows && grew && hdr && keys && edge_lp && row_depth && row_node && anc && row_edge && edge_row && row_lmax && child_off && out_score,
             "bound_expand: null argument");
  P5_REQUIRE(B >= 1 && CQ >= 1 && nchunk >= 1 && N >= 1 && KP >= 256 && (KP & (KP - 1)) == 0, "bound_expand: KP a power of two >= 256");
  return bound_expand_rows(sel, n_rows, grew, hdr, keys, KP, edge_lp, n_edges, op_sel_plan(row_depth, row_node, anc, max_depth, B, CQ, nchunk, sel, n_rows, cap),
                           row_edge, edge_row, row_lmax, child_off, out_score, N, margin, (hipStream_t)stream);
}
int p5_op_tr_probe(void* out, const void* in, void* stream) {
  P5_LAUNCH(p5_tr_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned short*)out, (const unsigned short*)in);
  return P5_KCHECK();
}

}  // extern "C"
