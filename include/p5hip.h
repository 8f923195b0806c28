/* p5hip.h -- C ABI of libp5hip.so: the MI355X-native T5 training + constrained-beam-search path that
 * replaces OpenP5's `P5_T5` model object (the seam is the Python `model` handed to the runner,
 * /root/reference/src/src_t5/main.py:184-206).
 *
 * The reference has no FFI of its own (pure Python over torch + HF transformers).  The entry points below are
 * therefore what a binding for this path needs, one per reference call it replaces:
 *
 *   p5_forward            <- P5_T5.forward(input_ids, whole_word_ids, attention_mask, labels) -> per-token NLL
 *                            (model/P5_T5.py:275-386, called at runner/DistributedRunner.py:63-70)
 *   p5_forward_loss       <- the same + the runner's masked-mean loss       (DistributedRunner.py:72-77)
 *   p5_backward           <- loss.backward()                               (DistributedRunner.py:80)
 *   p5_grad_sumsq +
 *   p5_adamw_step         <- clip_grad_norm_ + AdamW.step + scheduler      (DistributedRunner.py:81,85-86;
 *                                                                           SingleRunner.py:191-217)
 *   p5_generate           <- P5_T5.generate(..., prefix_allowed_tokens_fn, num_beams)  (DistributedRunner.py:361-371)
 *   p5_param_table        <- state_dict()/load_state_dict() key layout     (utils/utils.py:119-129)
 *
 * and, without a counterpart in the reference, what its users build on top of it: exact catalogue ranking and candidate scoring
 * (p5_rank_items, p5_cand_score, p5_prune_*, p5_bound_*), sampling under the item trie (p5_sample_items, p5_sample_slates) and the
 * training loss of that sampled distribution (p5_train_set_item_loss: the next p5_forward / p5_forward_loss and its backward normalise
 * every target position over the allowed children of the label prefix's trie node instead of the vocabulary),
 * plus per-kernel entry points (p5_op_*) used by the parity tests.
 *
 * Conventions: every pointer is a DEVICE pointer owned by the caller (torch's allocator); nothing is allocated,
 * freed or synchronised inside (graph-capturable); `stream` is a hipStream_t passed as void*; return value
 * 0 = ok, negative = error (message via p5_last_error()).  dtype: 0 = fp32 parity mode, 1 = bf16 fast mode.
 */
#ifndef P5HIP_H
#define P5HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct P5Config {
  int vocab_size, d_model, d_kv, d_ff, n_enc_layers, n_dec_layers, n_heads;
  int rel_buckets, rel_max_distance, whole_word_size;
  int gated_gelu;      /* 0: ReLU FFN (t5-small/base/large), 1: gated gelu_new (v1.1 / Flan) */
  int dtype;           /* 0 fp32, 1 bf16 */
  float eps, dropout;
  int pad_id, eos_id;
} P5Config;

typedef struct P5Engine P5Engine;

const char* p5_last_error(void);
/* process-wide tuning knobs (tests / benchmarks): "gemm_tile" = 0|64|128|256, "gemm_v2" = 0|2|3|4 (hand-pipelined loop for forced
 * 128x128 tiles), "gemm_ring", "gemm_small_ring", "gemm_ksdma", "gemm_xcd_rect" = 0|1 */
int p5_set_option(const char* name, int value);
int p5_abi_version(void);
/* In-run kernel profiler (measurement aid, bench.py): between p5_profile_begin() and p5_profile_end() every kernel launch of the library is
 * bracketed by two HIP events on its stream; p5_profile_end synchronises and writes a JSON array of {"kernel" (name + launch grid), "launches",
 * "total_us", "flops" (algorithmic FLOPs of the GEMM / attention launches, 0 elsewhere)} into `report` (NUL-terminated, `cap` bytes).
 * Durations include the dispatch gap of each launch (~1-2 us), i.e. they are upper bounds of the rocprofv3 kernel durations.  The test-only
 * host emulation reports the same kernel keys with zero times and FLOPs. */
int p5_profile_begin(void);
int p5_profile_end(char* report, int cap);
int p5_is_emulator(void);   /* 1 only for the test-only host emulation build under tests/emu */

/* ---- engine lifetime + parameter arena layout ---- */
int p5_engine_create(const P5Config* cfg, P5Engine** out);
int p5_engine_destroy(P5Engine* e);
int64_t p5_param_count(const P5Engine* e);
/* idx-th tensor of the arena in HF state-dict naming; returns 0, or 1 when idx is past the end */
int p5_param_table(const P5Engine* e, int idx, char* name, int name_cap, int64_t* offset, int* rows, int* cols);
/* params/grads: fp32 arenas of p5_param_count elements; shadow: bf16 arena (dtype=1) or NULL;
 * lut_enc/lut_dec: int32 [2*lut_half+1] bucket of rel=key-query (bidirectional / unidirectional);
 * rng_state: uint32[2] {seed, step} */
int p5_engine_bind(P5Engine* e, float* params, float* grads, void* shadow, const int* lut_enc, const int* lut_dec,
                   int lut_half, uint32_t* rng_state);
int p5_refresh_shadow(P5Engine* e, void* stream);
/* Optional (bf16 mode): a caller-owned buffer of p5_transposed_bytes(e) bytes that holds W^T of every 2-D layer weight at the
 * same arena offset.  When bound, the data gradients dx = dy W (the "autograd of nn.Linear" half of loss.backward(),
 * DistributedRunner.py:80) read W^T as a K-contiguous operand and run on the forward GEMM kernel instead of the
 * K-strided-operand variant.  p5_refresh_transposed after every parameter update (it runs on the side stream when one is bound
 * and the next backward waits for it). */
int64_t p5_transposed_bytes(const P5Engine* e);
int p5_engine_bind_transposed(P5Engine* e, void* buf, void* stream);
int p5_refresh_transposed(P5Engine* e, void* stream);
/* The next backward ADDS to what the gradient arena holds instead of starting a new sum: the 2nd.. micro-batch of a gradient-
 * accumulation group, or an arena the caller has just zero-filled itself on the stream that backward will use.  One-shot.
 * Without it a backward starts a new sum: it stores every Linear gradient and clears the atomically accumulated ones itself
 * (p5_engine_discard_grads), or clears the whole arena first where the storing path does not apply (fp32 engine). */
int p5_engine_grads_zeroed(P5Engine* e);
/* optimizer.zero_grad() (DistributedRunner.py:93) done by the engine: the fill is issued on the side stream when one is bound,
 * ordered after everything `stream` holds so far (the optimizer step that read the gradients), so that it overlaps the next
 * forward; the next backward waits for it.  Nothing else may read the gradient arena before that backward. */
int p5_engine_clear_grads(P5Engine* e, void* stream);
/* optimizer.zero_grad(set_to_none=True) (DistributedRunner.py:93): the gradients are dead until the next backward; no device work.
   (p5_engine_clear_grads is the eager, set_to_none=False form.) */
int p5_engine_discard_grads(P5Engine* e);
/* optional second stream: weight-gradient GEMMs run on it, one sub-layer behind the dgrad chain (NULL = single stream) */
int p5_engine_set_side_stream(P5Engine* e, void* side_stream);

/* ---- training step pieces ---- */
int64_t p5_train_workspace_bytes(const P5Engine* e, int B, int L, int T);
/* nll_out: fp32 [B*T]; keeps activations in ws for p5_backward */
int p5_forward(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
               const int64_t* labels, int B, int L, int T, int training, float* nll_out, void* ws, int64_t ws_bytes,
               void* stream);
/* p5_forward + the runner's masked-mean loss (DistributedRunner.py:72-77) in one call: loss_out[0] = mean_b(sum_t nll*m / max(sum_t m, 1)),
 * m = (output_attention != 0), computed behind the cross-entropy kernel.  A following p5_backward / p5_backward_stage with
 * dnll == NULL back-propagates d(loss) = 1 (the CE backward derives the per-token weights from the mask itself). */
int p5_forward_loss(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                    const int64_t* labels, const int64_t* output_attention /* [B,T] */, int B, int L, int T, int training,
                    float* nll_out /* [B*T] */, float* loss_out /* [1] */, void* ws, int64_t ws_bytes, void* stream);
/* ---- several targets per user with ONE encoder pass ----
 * labels [B, G, T] (flat [B*G*T], (b, g, t) order): what the three calls above compute for the replicated batch -- user b's inputs repeated G
 * times, sample b*G + g carrying labels[b, g] -- but the encoder and the projection of its output to every decoder layer's cross-attention K/V
 * run once per user; the decoder is a batch of B*G sequences, cross-attention runs a user's G*T queries against that user's keys, and the
 * gradients into the encoder output, the encoder and the K/V weights are the sums over a user's G targets.  nll_out: fp32 [B*G*T].  With dropout
 * on, the masks follow the engine's site / flat-index rule on the tensors actually formed (encoder: batch B; decoder rows: [B*G*T, .]; self
 * attention: [B*G, H, T, T]; cross attention: [B, H, G*T, L]).  G = 1 is the plain call, bit for bit (the plain calls ARE these with G = 1 and
 * NULL weights).  Limits: G >= 1; for G > 1, G*T <= 512 (the attention kernels' query limit) and B*G*T <= 65536 (the norm-backward
 * epilogue's partial table: 1024 blocks of 64 rows) and B*G*n_heads <= 65535 (the y extent of the self-attention launch grids).  p5_backward / p5_backward_stage / p5_backward_staged follow as usual.
 * The one-shot item-loss calls compose as with the plain calls: excluded_nodes stays [B, excluded_words] (per USER, applied to all G targets),
 * row_state_out / row_cut are [B*G*T], and p5_item_head_workspace_bytes(e, B, T, n) is called with B*G in the place of B.
 * p5_forward_loss_targets: output_attention [B, G, T]; target_weights DEVICE fp32 [B*G] or NULL (= all ones; may be negative or zero);
 *   loss_out[0] = sum_{b,g} w[b,g] * (sum_t nll*m / max(sum_t m, 1)) / (B*G),
 * and the backward with dnll == NULL is seeded with its gradient.  target_weights must stay valid until the backward has run. */
int64_t p5_train_workspace_bytes_targets(const P5Engine* e, int B, int L, int T, int G);
int p5_forward_targets(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                       const int64_t* labels /* [B,G,T] */, int B, int L, int T, int G, int training, float* nll_out /* [B*G*T] */, void* ws,
                       int64_t ws_bytes, void* stream);
int p5_forward_loss_targets(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                            const int64_t* labels /* [B,G,T] */, const int64_t* output_attention /* [B,G,T] */, int B, int L, int T, int G,
                            const float* target_weights /* DEVICE [B*G] or NULL */, int training, float* nll_out /* [B*G*T] */,
                            float* loss_out /* [1] */, void* ws, int64_t ws_bytes, void* stream);
/* stages: 0 = head + decoder-final, 1..n_dec = decoder layers (top first), then decoder embedding,
 * then encoder-final + encoder layers (top first), last = encoder embedding.  p5_backward runs them all. */
/* ---- trie-normalised item loss: the training loss of the distribution p5_sample_items / p5_sample_slates draw from (openp5_amd/csrc/p5_trie_ce.h) ----
 * One-shot: the NEXT p5_forward / p5_forward_loss on this engine, and the backward that follows it, replace the full-vocabulary cross-entropy by
 *   nll[b, t] = log sum_{allowed children c of node(labels[b, :t])} exp(z_c / temperature) - z_label / temperature,
 * z = the head's logits.  The trie is that of the samplers (CSR, DEVICE arrays, as p5_generate; the walk starts at the root's child whose
 * token is the decoder start id); excluded_nodes (DEVICE uint32 [B, excluded_words], excluded_words * 32 >= n_nodes, or NULL) takes the same
 * children out of the normalisation that the samplers never draw.  With the sampler's temperature and exclusion, nll is -out_tok_logprob of a
 * draw and the backward its exact score function.  Row states (row_state_out: DEVICE int32 [B * T] or NULL; written by the forward):
 *   0 scored; 1 past the end (behind </s>, at a node without children, at label -100 and behind it): nll = 0, no gradient;
 *   2 off the trie (the label is no child of the node, or an excluded one; every later row of the sample too): nll = 0, no gradient.
 * The forward takes the materialised-logits route (the head GEMM still runs over the whole vocabulary) and reads only the children's
 * logits; the backward writes the dense dlogits [B * T, Vp] (zeros outside the allowed children), so the tied head's gradients, the staged
 * backward, accumulation and data-parallel ranges are what they are for the plain loss, at the cost of the "ce_free" 0 route.  The workspace
 * is p5_train_workspace_bytes, unchanged.  The next forward without a new call is the plain one again, bit for bit.  All arrays must stay
 * valid until the backward has run. */
int p5_train_set_item_loss(P5Engine* e, const int* child_off, const int* child_tok, const int* child_node, int n_nodes,
                           const uint32_t* excluded_nodes, int excluded_words, float temperature, int* row_state_out);
/* The same under top-k / nucleus truncation (openp5_amd/csrc/p5_trunc.h; the semantics are stated at p5_sample_items_truncated): per
 * row the normalisation runs over the KEPT children only, nll = lse_kept - z_label / temperature, and the backward writes gradients only
 * there (the kept set is a constant of the gradient, as under HF's masked_fill).  With the sampler's top_k / top_p, nll is -out_tok_logprob
 * of a truncated draw.  A label that is allowed but below the row's cut is row state
 *   3 truncated away: nll = 0 and no gradient FOR THAT ROW ONLY (the walk knows nothing of logits: later rows are scored as usual).
 * row_cut (DEVICE fp32 [B * T], required): the forward writes every row's cut (min z over the kept set; +inf for rows that are not
 * scored), the backward reads it; it must stay valid until the backward has run.  top_k >= 0 (0 = off), 0 < top_p <= 1 (1 = off); with
 * both off the plain item-loss kernels run, bit for bit, and row_cut is not written.  One-shot like its sibling; p5_train_workspace_bytes
 * is unchanged. */
int p5_train_set_item_loss_truncated(P5Engine* e, const int* child_off, const int* child_tok, const int* child_node, int n_nodes,
                                     const uint32_t* excluded_nodes, int excluded_words, float temperature, int* row_state_out, int top_k,
                                     float top_p, float* row_cut /* DEVICE [B*T] */);
/* The item loss on a head RESTRICTED to the trie's tokens (openp5_amd/csrc/p5_item_head.h), opt-in.  U = the distinct tokens on the trie's edges,
 * ascending; Nu = |U|, Nup = Nu rounded up to 64.  The forward gathers the rows U of the head weight into E_U [Nup, d], the head GEMM writes
 * logits_U [B*T, Nup] instead of [B*T, Vp], the cross-entropy kernels read a child's logit at child_col[edge] (one int per CSR edge: the index of
 * child_tok[edge] in head_tokens), and the backward writes dlogits_U, takes dhn over K = Nup (the same ordered split-K partial sums) and
 * dE_U [Nup, d] with one un-split GEMM, which one kernel scatters into shared.weight's gradient: all V rows on a storing first micro-batch
 * (zeros outside U), the rows U added otherwise.  No [B*T, Vp] array is written or read.  The loss, the row states and row_cut are those of
 * the dense route on equal logits; the two heads' logits differ by the GEMMs' rounding only.
 * Call it BEHIND p5_train_set_item_loss[_truncated] and in front of the forward; one-shot like them (a new p5_train_set_item_loss disarms it).
 * ws: DEVICE, 256-byte aligned, at least p5_item_head_workspace_bytes(e, B, T, n_tokens) bytes for the batch of the forward (the forward
 * checks it); it holds E_U, logits_U, dlogits_U and dE_U and must stay valid, like head_tokens and child_col, until the backward has run.
 * p5_train_workspace_bytes is unchanged.  Errors: no item loss armed, n_tokens outside [1, vocab_size], null arguments, ws too small. */
size_t p5_item_head_workspace_bytes(const P5Engine* e, int B, int T, int n_tokens);
int p5_train_set_item_head(P5Engine* e, const int* head_tokens /* DEVICE [n_tokens], ascending, distinct */, int n_tokens,
                           const int* child_col /* DEVICE [n_edges] */, void* ws, size_t ws_bytes);
/* Two exact per-row regularisers of the item loss (openp5_amd/csrc/p5_trie_reg.h), opt-in: the ENTROPY H of a scored row's distribution over
 * the allowed children of its node, and its divergence KL(policy || reference) from the distribution that ref_logits give over the SAME
 * children at the same temperature.  Rows that are not scored and rows with one allowed child have H = KL = 0 exactly.
 * Call it BEHIND p5_train_set_item_loss and, if used, p5_train_set_item_head, in front of the forward; one-shot like them (a new
 * p5_train_set_item_loss disarms it).  The forward then runs the regularised twin of the item-loss kernel (nll and lse keep their bits) and the
 * backward the twin that adds the two terms' gradients to the same dlogits row in one pass.
 * ref_logits: DEVICE fp32 [rows, ld_ref] in the column layout of the call's own head -- token columns (ld_ref >= vocab_size) for the dense head,
 *   child_col columns (ld_ref >= n_tokens) for the restricted head -- or NULL: entropy only, KL is 0 and has no gradient.  It must be finite at
 *   the allowed children (not checked: a -inf there gives KL = +inf) and is a constant of the gradient.
 * row_terms: DEVICE fp32 [3 * rows], caller-owned like row_cut: H | KL | lse_ref, rows = B * G * T values each (the last two only with
 *   ref_logits); written by the forward, read by the backward.
 * The backward's seeds: called with dnll, it reads the per-row gradients of H and KL handed over by p5_backward_set_item_grads (zeros without
 *   that call).  Called without (behind p5_forward_loss / p5_forward_loss_targets) the loss is
 *     loss = L_nll + kl_coef * R_KL - entropy_coef * R_H,   R_X = sum_{b,g} (sum_t X * m / max(sum_t m, 1)) / (B * G),  m = output_attention != 0,
 *   L_nll what it is without this call (target_weights included); R_H and R_KL are NOT weighted by target_weights.  loss_out receives the loss
 *   and terms_out (DEVICE fp32 [3], or NULL) the parts (L_nll, R_H, R_KL).
 * Errors: no item loss armed, the truncated item loss armed (not built), ld_ref smaller than the head's columns, row_terms NULL, a
 * coefficient that is not finite. */
int p5_train_set_item_regularizers(P5Engine* e, const float* ref_logits, int ld_ref, float* row_terms, float entropy_coef, float kl_coef,
                                   float* terms_out);
/* The clipped-ratio (PPO / GRPO style) policy objective (p5_clip.h) for several updates on one sampled batch.  One-shot, like
 * p5_train_set_item_loss (call it behind that one): arms the NEXT p5_forward_loss / p5_forward_loss_targets and the backward behind it.  Two
 * launches take the place of the masked-mean loss kernels.  Per target (b, g) with mask m = output_attention != 0, cnt = sum_t m, w =
 * target_weights[b, g] (NULL = 1), lo = 1 - eps_low, hi = 1 + eps_high and rho = exp(log p_new - log p_old) = exp(-(old_logprobs + nll)):
 *   ratio_mode 0 (token)     l = (1 / max(cnt, 1)) sum_t m_t max(-rho_t w, -clamp(rho_t, lo, hi) w)
 *   ratio_mode 1 (sequence)  rho = exp(-(sum_t m_t (old_t + nll_t)) / max(cnt, 1)), l = max(-rho w, -clamp(rho, lo, hi) w); cnt = 0: l = 0
 * loss = sum l / (B G); a target with target_mode 0 keeps its plain weighted term (target_mode int32 DEVICE [B * G], NULL = all 1); armed
 * regularisers add their terms unchanged.  old_logprobs: DEVICE fp32 [rows], rows = B G T, read where m.  A unit (token, or target) with
 * (w > 0 and rho > hi) or (w < 0 and rho < lo) is clipped: its rows' seeds are exact zeros; w == 0 gives zeros too.  With rho == 1 the seeds
 * are the plain weighted step's bits.  Rows are taken as they come (nll 0 at rows the item loss did not score: clipped targets should be
 * fully scored).  row_seed: DEVICE fp32, caller-owned until the backward has run: [rows], or [3 * rows] with regularisers armed (then the
 * rows' entropy / KL seeds follow); user_partials DEVICE fp32 [B * 16] scratch; clip_stats DEVICE fp32 [8], no host sync: units, share clipped,
 * share clipped at hi, share clipped at lo, mean rho, max rho, min rho, mean of (rho - 1) - log rho -- the two means over units with
 * 0 < rho < inf; no unit: (0, 0, 0, 0, 1, 1, 1, 0).  The backward with dnll == NULL feeds row_seed through the per-row-seed path of every
 * route (p5_backward, p5_backward_stage, p5_backward_staged).  No atomics: equal inputs give equal bits.
 * Errors: eps not finite or negative, an unknown ratio mode, NULL required pointers, the truncated item loss armed (not built: the kept set
 * may differ between the two policies); p5_forward / p5_forward_targets called while it is armed refuse and disarm it. */
int p5_train_set_clip_objective(P5Engine* e, const float* old_logprobs, const int* target_mode, float eps_low, float eps_high, int ratio_mode,
                                float* row_seed, float* user_partials, float* clip_stats);
/* A listwise preference objective (p5_pref.h) over the G targets of every user.  One-shot, like p5_train_set_clip_objective (call it behind
 * p5_train_set_item_loss): arms the NEXT p5_forward_loss_targets and the backward behind it; two launches take the place of the masked-mean
 * loss kernels.  Per target (b, g) with m = output_attention != 0: cnt = sum_t m, s = sum_t m nll, r = sum_t m ref_logprobs (0 when NULL =
 * reference-free), Delta = (-s - r) / c' (c' = max(cnt, 1) with length_normalize, else 1), h = beta Delta.  The list of user b: its targets
 * with pref_mask != 0 (int32 DEVICE [B * G], NULL = all) and cnt > 0, in index order, the preferred one first; every other target is skipped
 * (no contribution, exact-zero seeds, ref_logprobs never read -- it is read only where m, and only at targets with pref_mask != 0).
 *   kind 0 (Plackett-Luce), depth D (0 = full): for a list of n >= 2, D_b = min(D or n - 1, n - 1) and
 *        l_b = sum_{k < D_b} (logsumexp_{j >= k} h_j - h_k): n = 2 is DPO, D = 1 softmax-DPO, full depth the PL likelihood of the order
 *   kind 1 (IPO): l_b = mean_{j = 1 .. n - 1} ((Delta_0 - Delta_j) - 1 / (2 beta))^2        (depth is ignored)
 * A list of fewer than two has l_b = 0; a list of at least one adds sft_coef * (sum_t m nll / max(cnt, 1)) of its first target.
 * loss = sum_b (l_b + sft_b) / B.  row_seed: DEVICE fp32 [B G T], caller-owned until the backward has run; user_partials DEVICE fp32 [B * 16]
 * scratch; pref_stats DEVICE fp32 [8], no host sync: users with a pair (n >= 2), share of pairs (first, j) with h_first > h_j, mean h_first
 * over those users, mean h_j over the pairs, mean margin h_first - h_j over the pairs, the preference part of the loss, the SFT part, mean n
 * over users with n >= 1; no pair: 0 .. 4 are 0, no list: 7 is 0.  With a list of one and sft_coef = c the seeds are the bits of the plain
 * step with target_weights (c G, 0, ...) when G is a power of two.  No atomics: equal inputs give equal bits.
 * Errors: beta not finite or <= 0, an unknown kind, depth < 0, sft_coef not finite, NULL required pointers, the clip objective armed as well,
 * item regularizers armed (not built), the truncated item loss armed (the kept set may differ between the two policies); the armed forward
 * refuses target_weights != NULL and G > 512; p5_forward / p5_forward_targets called while it is armed refuse and disarm it. */
int p5_train_set_pref_objective(P5Engine* e, const float* ref_logprobs, const int* pref_mask, int kind, float beta, int depth, int length_normalize,
                                float sft_coef, float* row_seed, float* user_partials, float* pref_stats);
/* One-shot, in front of p5_backward / p5_backward_stage (stage 0) / p5_backward_staged called WITH dnll: DEVICE fp32 [rows] gradients of the
 * rows' H and KL of the last forward (NULL = zeros).  Error: the last forward ran without p5_train_set_item_regularizers. */
int p5_backward_set_item_grads(P5Engine* e, const float* d_entropy, const float* d_kl);
/* The materialised fp32 logits of the last item-loss forward, for a frozen reference model: *ptr DEVICE [*rows, *ld], of which the first *cols
 * columns are logits (dense head: ld = vocab_size rounded up to 64, cols = vocab_size; restricted head: logits_U, ld = Nup, cols = n_tokens).
 * Valid until the engine's next forward.  Error: the last forward ran without an item loss. */
int p5_train_last_item_logits(const P5Engine* e, const float** ptr, int* rows, int* ld, int* cols);
int p5_backward_num_stages(const P5Engine* e);
int p5_backward_stage(P5Engine* e, const float* dnll, int stage, void* stream);
int p5_backward(P5Engine* e, const float* dnll, void* stream);
/* LAYOUT ONLY: the arena range [begin,end) of the parameters whose gradients `stage` computes.  It does NOT say when they are final:
 * with the default two-layer weight-gradient groups a stage's gradients may be written by a LATER stage's grouped launch.  A data-parallel
 * caller exchanges the range reported by p5_backward_final_range after each stage (below), never this one. */
int p5_backward_stage_range(const P5Engine* e, int stage, int64_t* begin, int64_t* end);
/* What a data-parallel caller exchanges after each p5_backward_stage call: the gradient range that became FINAL with that call -- the
 * union of the stage ranges whose kernels have all been launched (empty while a two-layer weight-gradient group of the encoder is still
 * filling up: the staged backward issues the same grouped launches as p5_backward; p5_backward_stage_pairs(e, 0) restores one launch per
 * layer and one range per stage).  Ranges are contiguous and walk the arena from the back. */
int p5_backward_final_range(const P5Engine* e, int64_t* begin, int64_t* end);
int p5_backward_stage_pairs(P5Engine* e, int on);
/* The staged backward as ONE call: all stages are enqueued on `stream`; ranges[2k], ranges[2k+1] = the k-th gradient range that became final
 * (arena offsets, in completion order), *n_ranges their number (<= max_ranges, <= p5_backward_num_stages).  Behind each one an event is
 * recorded on `stream` (and, when the engine has a side stream, a second one there: weight gradients of the range may have been launched
 * on it): p5_backward_staged_wait(e, k, comm_stream) makes `comm_stream` wait for both (hipStreamWaitEvent, no host wait), after
 * which the caller enqueues the exchange of range k there -- DDP's bucketed all-reduce overlapped with the rest of the backward
 * (/root/reference/src/src_t5/main.py:158-160 wraps the model in DDP) without one host round trip per stage. */
int p5_backward_staged(P5Engine* e, const float* dnll, void* stream, int64_t* ranges, int max_ranges, int* n_ranges);
int p5_backward_staged_wait(P5Engine* e, int k, void* comm_stream);
/* The exchange for a host without torch.distributed ("an p5_allreduce_* shim over RCCL taking an ncclComm_t created once per
 * process"; replaces what DDP's reducer would do at /root/reference/src/src_t5/runner/DistributedRunner.py:26).  `nccl_comm` is the
 * caller's ncclComm_t; the library has no link-time RCCL dependency and calls the ncclAllReduce already loaded in the process (the one
 * that created the communicator), else librccl.so.1.
 *   p5_allreduce_range(e, k, comm, bf16_scratch, comm_stream): waits on `comm_stream` for range k of the last p5_backward_staged (both of
 *     its events when weight gradients ran on the engine's side stream) and all-reduces (SUM) that slice of the gradient arena in place
 *     there; bf16_scratch != NULL (room for the range's elements as bf16): cast -> all-reduce in bf16 -> widen back (half the xGMI bytes).
 *     The mean over ranks is NOT taken here: pass grad_scale = 1 / world to p5_adamw_step.
 *   p5_allreduce_sum(buf, count, dtype, comm, stream): any device buffer in place; dtype 0 = f32, 1 = bf16, 2 = f64, 3 = i64 (the metric
 *     sums of DistributedRunner.py:389-395). */
int p5_allreduce_range(P5Engine* e, int k, void* nccl_comm, void* bf16_scratch, void* comm_stream);
int p5_allreduce_sum(void* buf, int64_t count, int dtype, void* nccl_comm, void* stream);

/* out_partials: float[1024], fully overwritten; p5_adamw_step sums them in a fixed order (bit-identical on every rank) */
int p5_grad_sumsq(const float* grads, int64_t n, float* out_partials, void* stream);
int p5_adamw_step(float* params, const float* grads, float* m, float* v, void* shadow_bf16, int64_t n,
                  const float* sumsq /* float[1024] from p5_grad_sumsq, or NULL = no clipping */, double max_norm, double grad_scale, double lr, double beta1,
                  double beta2, double eps, double weight_decay /* doubles, as the reference's Python floats: derived scalars are rounded once */, int step_t,
                  void* stream);
/* The same step over the ENGINE's bound arenas (params, grads, bf16 shadow).  With the transposed / norm-folded copies bound
 * (p5_engine_bind_transposed, bf16 training) the update ALSO writes W^T and W diag(ln) -- the 2-D layer weights are updated in 64 x 64
 * tiles that are transposed through LDS, a projection behind a T5LayerNorm is multiplied by the norm weight's NEW value -- so the
 * caller skips p5_refresh_transposed (*copies_fresh = 1; 0 when the flat path ran: fp32 engine, no copy bound, side stream, option
 * "adam_tiles" 0).  Per element the arithmetic is p5_adamw_step's: parameters, moments and all three copies are bit-identical. */
int p5_engine_adamw_step(P5Engine* e, float* m, float* v, const float* sumsq, double max_norm, double grad_scale, double lr, double beta1,
                         double beta2, double eps, double weight_decay, int step_t, int* copies_fresh, void* stream);

/* ---- generation ---- */
/* Exact workspace of p5_generate / p5_decode_begin (R = B*K rows, C = min(max_children, 2K), every block rounded up to 256 bytes):
 * the encoder / forced-prefix buffers, cross-attention K/V, the step KV cache (n_dec_layers x max_len x R x 2 x inner x sizeof(T)),
 * the decode-step activations, per-row head partials and candidate scratch (R x max_children fp32), the beam state, and
 *   K <= 64:                 the narrow candidate lists, 2 x R x 2K x 4 bytes, and the [R, V] fp32 logits;
 *   K > 64:                  no narrow lists; the [R, V] logits only where the head is not the streaming one (toy d_model);
 *   K > 64 or gen_wide = 1:  the wide step's buffers behind everything else: R x C x 8 (row candidate keys) + R x 4 (counts)
 *                            + 4 x R x 2 x 4 (the items' top-2K scores / beams / tokens / nodes) + 2 x R x 4 (running selection, finished sources).
 * The size depends on the gen_wide option at the time of the call: query it under the option the search runs with. */
int64_t p5_generate_workspace_bytes(const P5Engine* e, int B, int L, int K, int max_len, int max_children, int excluded_words);
/* trie in CSR: child_off[n_nodes+1], child_tok/child_node[n_edges]; node 0 = empty prefix.
 * out_seq int32 [B,K,max_len] (pad-filled, starts with pad=decoder start), out_score fp32 [B,K], out_len int32 [B,K].
 * excluded_nodes: optional uint32 bitmap [B, excluded_words] over trie node ids; bit n of row b set = node n does not
 * exist in item b's trie (the per-user history exclusion of the filtered protocol, DistributedRunner.py:286-297,
 * without building one trie per user).  NULL / 0 = nothing excluded.
 * Replaces P5_T5.generate(...) = HF beam search + PrefixConstrainedLogitsProcessor (DistributedRunner.py:361-371).
 * Enqueues the whole search and returns WITHOUT synchronising: HF's stop test is taken on the device, so no step reads
 * anything back.  max_len bounds the number of decode steps enqueued (max_len - 1): pass min(max_length, depth of the trie).
 * Limits: 1 <= K <= 4096 beams, 2 <= max_len <= 128; the trie may be any DAG in this CSR form (an appended trie, generation_trie.py:19-21,
 * is grafted by the caller -- openp5_amd/trie.py::CompiledTrie.from_trie).  K <= 64 runs the narrow beam step (openp5_amd/csrc/p5_decode.h:
 * an item's state and candidate pool in one workgroup's LDS); 65 <= K <= 4096 the wide one (p5_decode_wide.h: exact top-2K by radix select
 * + sort, beam state in global memory), which returns what the narrow step returns, bit for bit, where both run -- p5_set_option("gen_wide", 1)
 * selects it at any K (a test / benchmark hook; part of the decode-step hipGraph key).  p5_generate_draft and the p5_verify_* calls keep
 * K <= 64 (draft searches always take the narrow step). */
int p5_generate(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                int B, int L, int K, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                const int* roots /* [B] empty-prefix node per batch item, or NULL = node 0 */,
                const uint32_t* excluded_nodes, int excluded_words, int max_children, int* out_seq, float* out_score, int* out_len, void* ws, int64_t ws_bytes, void* stream);
/* Forced-prefix fast-forward (openp5_amd/csrc/p5_decode.h): when the first n tokens after the decoder start token are the same for EVERY
 * item of the trie (OpenP5 item ids all start with "<dataset> item _"), the first n beam-search steps have one allowed token each and
 * are computed as ONE teacher-forced decoder pass over n positions per user instead of n decode steps -- same numbers, n - 1 steps saved.
 * tokens[i] / nodes[i]: the i-th forced token and the trie node it leads to (HOST arrays, n <= 16).  One-shot: applies to the next
 * p5_decode_begin / p5_generate / p5_generate_draft on this engine; ignored with per-item roots, n < 2, or option "gen_ff" = 0.
 * The caller guarantees that the chain is really forced for every item of the batch (no excluded node on it). */
int p5_generate_set_forced_prefix(P5Engine* e, const int* tokens, const int* nodes, int n);
/* ---- trie-constrained sampling: S independent draws per user from the model's distribution over the trie's items (openp5_amd/csrc/p5_sample.h) ----
 * What HF's sampling path computes under a PrefixConstrainedLogitsProcessor: the logits processors run before softmax, so the distribution
 * of a step is softmax(z / temperature) RENORMALISED over the allowed children of the row's trie node (the beam search above normalises
 * over the full vocabulary first; these log-probabilities are therefore not the beam search's).  A step is the decoder of the beam search
 * over R = B x S rows without its vocabulary head, plus one launch that recomputes the children's logits, draws one child per row by
 * Gumbel-max (ties: the lowest child position) and reduces log sum_allowed exp(z / temperature) in the same pass.
 *   trie, excluded_nodes / excluded_words, max_children: as p5_generate (a child whose bit is set has probability 0; a user without any
 *     allowed child at the start gets log-probability -inf, length 0 and an all-pad sequence).  No per-item roots.
 *   seed, stream_ids (DEVICE uint32 [B]), draw_base: the uniform behind every Gumbel is a pure function of (seed, stream_ids[b],
 *     draw_base + s, step, child position) -- csrc/p5_rng.h::p5_sample_row_key / p5_sample_uniform is the specification -- so a draw does
 *     not depend on the batch it is made in: splitting users or draw ranges over several calls returns the same bits.
 *   out_seq int32 [B, S, max_len] (pad-filled, decoder start first), out_logprob fp32 [B, S] (sum of the tokens' log-probabilities),
 *     out_tok_logprob fp32 [B, S, max_len] by position (position 0, forced positions and positions behind </s>: 0), out_len int32 [B, S]
 *     generated tokens up to and including </s> (0: the draw did not reach a leaf within max_len).
 * A forced prefix (p5_generate_set_forced_prefix, option "gen_ff") is honoured as by p5_generate: its tokens have renormalised probability 1.
 * Enqueues max_len - 1 - (forced steps) steps with plain launches and returns without synchronising; there is no early stop (a finished
 * row is a no-op of the selection launch): pass max_len = min(max_length, depth of the trie).  The decode-step hipGraph of p5_generate is
 * neither used nor invalidated.  Every value has one writer: two calls return the same bits.
 * Limits: 1 <= S <= 4096, 2 <= max_len <= 128, L <= 512, temperature > 0, d_model <= 1024.
 * The workspace (exact; max_children / excluded_words do not enter it: no buffer follows the fan-out, the bitmap is read in place): the
 * encoder / forced-prefix buffers, cross-attention K/V, the step KV cache (n_dec_layers x max_len x R x 2 x inner x sizeof(T)), the
 * decode-step activations and the rows' state (3 x R x max_len x 4 bytes + a few words per row). */
int64_t p5_sample_workspace_bytes(const P5Engine* e, int B, int L, int S, int max_len, int max_children, int excluded_words);
int p5_sample_items(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int S,
                    int max_len, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded_nodes,
                    int excluded_words, int max_children, uint32_t seed, const uint32_t* stream_ids /* device uint32 [B] */, uint32_t draw_base,
                    float temperature, int* out_seq, float* out_logprob, float* out_tok_logprob, int* out_len, void* ws, int64_t ws_bytes, void* stream);
/* ---- p5_sample_items under top-k / nucleus truncation (openp5_amd/csrc/p5_trunc.h) ----
 * HF's order (processors, temperature, TopKLogitsWarper, TopPLogitsWarper, softmax) restated on the allowed children.  For a row at node n:
 * A = the children that are not excluded and have a finite logit, z_i = logit_i / temperature.
 *   top_k >= 1 (0 = off): K1 = { i in A : z_i >= the k-th largest z of A }; ties at the k-th value all stay; |A| <= k: K1 = A.
 *   0 < top_p <= 1 (1 = off), on softmax over K1: child i stays iff mass{ j in K1 : z_j > z_i } < top_p * mass(K1).  By VALUE: children
 *     with equal z stay or leave together (HF cuts inside such a group by sort position -- the one deviation), so the result does not
 *     depend on the order of the children.  The largest value always stays.
 * The step's distribution is softmax(z) over the kept set { i in A : z_i >= cut }; out_tok_logprob holds log-probabilities under it, exactly
 * 0 where one child is kept (top_k = 1 is the greedy descent).  The uniform of a child is the function of (seed, stream, draw, step,
 * child position) p5_sample_items uses: truncation never changes a child's noise, so a draw whose untruncated path stays inside the kept
 * sets is the same draw.  The cut is a pure function of the row's values (integer radix select for top-k; for top-p a bisection over
 * sums taken in one fixed order): two calls return the same bits.  Off = top_k in {0, >= max_children} and top_p = 1: the kernels of
 * p5_sample_items run and every output is its output, bit for bit.
 * The workspace (exact; -1 outside the limits of p5_sample_items): p5_sample_workspace_bytes plus the step's [B * S, max_children] fp32
 * scratch (rounded up to 256 bytes). */
int64_t p5_sample_truncated_workspace_bytes(const P5Engine* e, int B, int L, int S, int max_len, int max_children, int excluded_words);
int p5_sample_items_truncated(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                              int S, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                              const uint32_t* excluded_nodes, int excluded_words, int max_children, uint32_t seed,
                              const uint32_t* stream_ids /* device uint32 [B] */, uint32_t draw_base, float temperature, int top_k, float top_p,
                              int* out_seq, float* out_logprob, float* out_tok_logprob, int* out_len, void* ws, int64_t ws_bytes, void* stream);
/* ---- stochastic beam search: S slates of K DISTINCT items per user, a sample without replacement (openp5_amd/csrc/p5_sbs.h) ----
 * The distribution is that of p5_sample_items.  A slate is the K items with the largest G(item) = log p(item) + Gumbel noise, largest first:
 * a sample without replacement in sequential-sampling (Plackett-Luce) order (Kool, van Hoof, Welling 2019), computed top-down over the trie
 * with K beams per slate.  A live beam (phi_S, G_S) gives its allowed children phi_i = phi_S + token log-probability, g_i = phi_i -
 * log(-log u_i), Z = max g_i (ties: the lowest edge); the argmax child keeps G_S exactly, every other child gets
 * G_S - max(v, 0) - log1p(exp(-|v|)) with v = G_S - g_i + log1p(-exp(g_i - Z)).  The beams of the next step are the K best of the children
 * of the live beams and the finished beams (carried), by (perturbed value desc, global CSR edge index asc).  The root has (0, 0).
 *   trie, excluded_nodes / excluded_words, max_children, seed, stream_ids, temperature: as p5_sample_items.  The trie must be tree-shaped
 *     (every edge reached by one prefix): the uniform of a child is a pure function of (seed, stream_ids[b], slate_base + s, step, GLOBAL CSR
 *     edge index child_off[node] + i) -- csrc/p5_rng.h -- so the perturbed value of a trie node does not depend on K, on the batch or on
 *     the beam slot: the slate of K' < K is the first K' entries of the slate of K, and user chunks / slate ranges return the same bits.
 *   out_seq int32 [B, S, K, max_len], out_logprob fp32 [B, S, K] (phi: the item's log-probability), out_perturbed fp32 [B, S, K] (descending,
 *     <= 0), out_tok_logprob fp32 [B, S, K, max_len] by position, out_len int32 [B, S, K].  Fewer than K allowed items: the trailing slots
 *     hold the all-pad sequence behind the decoder start, log-probability -inf, perturbed -inf, length 0.
 * A forced prefix (p5_generate_set_forced_prefix, option "gen_ff") is honoured as by p5_sample_items: behind it beam 0 of every slate is live
 * with (0, 0).  Enqueues max_len - 1 - (forced steps) steps of plain launches (decoder without head, row / select / commit kernels) and
 * returns without synchronising; no early stop, no hipGraph.  Every value has one writer: two calls return the same bits.
 * Limits: 1 <= K <= 4096, 1 <= S, S x K <= 4096 rows per user and call, 2 <= max_len <= 128, L <= 512, temperature > 0, d_model <= 1024.
 * The workspace (exact; p5_sample_slates_workspace_bytes returns -1 outside the limits): that of p5_sample_items for S x K rows per user,
 * second sequence / log-probability / ancestry buffers (rows change places), and the step's scratch, which follows the fan-out: two
 * [R, max_children] fp32 rows and the [R, min(max_children, K)] 64-bit key lists. */
int64_t p5_sample_slates_workspace_bytes(const P5Engine* e, int B, int L, int S, int K, int max_len, int max_children, int excluded_words);
int p5_sample_slates(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L, int S, int K,
                     int max_len, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded_nodes,
                     int excluded_words, int max_children, uint32_t seed, const uint32_t* stream_ids /* device uint32 [B] */, uint32_t slate_base,
                     float temperature, int* out_seq, float* out_logprob, float* out_perturbed, float* out_tok_logprob, int* out_len, void* ws,
                     int64_t ws_bytes, void* stream);
/* ---- verified generation: the bf16 search proposes, an fp32 pass decides (openp5_amd/csrc/p5_verify.h) ----
 * The reference ranks by the fp32 scores of HF beam search (DistributedRunner.py:361-387, utils/evaluate.py:37-58).  Protocol, two engines
 * over the SAME master parameter arena (a bf16 one for the draft, an fp32 one -- dtype 0 -- for the verification), one stream:
 *   p5_verify_begin   (fp32 engine)   -> lays out the verification workspace for this batch shape (host only)
 *   p5_verify_encode  (fp32 engine)   -> fp32 encoder pass + cross-attention K/V; p5_verify_encoder_output() = its fp32 [B*L, d_model]
 *   p5_generate_set_encoder_output + p5_generate_draft (bf16 engine, beam width Kw = K + a few): the draft starts from THAT encoder
 *                                        output (rounded once) instead of running its own encoder; its results are ignored, `hist` = what
 *                                        the search kept alive at every step
 *   p5_verify_plan    (fp32 engine)   -> the distinct live prefixes of every user ("rows"); p5_verify_plan_header()[0] = the largest
 *                                        row count of any user -- the ONE number the host reads
 *   p5_verify_run     (fp32 engine, rows_per_user >= that number, multiple of 16 recommended)
 *                                     -> one teacher-forced fp32 decoder pass over all rows, full-vocabulary log-sum-exp and the trie
 *                                        children's log-probabilities per row, then HF's beam search of the REAL width K replayed on
 *                                        those numbers.  out_* as p5_generate; out_missing int32 [B]: 1 = the replay needed a prefix the
 *                                        draft had dropped, or a value of the pass left the range of the split products -- that user's
 *                                        result is NOT the fp32 search's and the caller must re-run the user through p5_generate on the
 *                                        fp32 engine (openp5_amd/model.py does).
 * A returned, unflagged list is the fp32 search's list: no bf16 number takes part in any decision or score.  The GEMMs of the fp32 passes
 * multiply on the f16 matrix cores from a two-term fp16 split of every fp32 operand (x = hi + lo / 4096: 22 mantissa bits, the lo x lo
 * term dropped, ~2^-22 relative per product, valid for |x| < 2^15 -- csrc/p5_gemm.h; option "verify_split" 0 = exact fp32 MFMAs).  A user
 * any of whose final hidden rows is non-finite or outside that range (an operand of the pass overflowed the split) is flagged through
 * out_missing exactly like a user with a missing prefix.  Limits: K <= 22, Kw <= 64, rows_per_user <= 512 and <= p5_verify_row_capacity.  A forced prefix set on the fp32 engine (p5_generate_set_forced_prefix) before p5_verify_begin
 * lets the replay skip the forced steps as the draft does. */
int64_t p5_generate_history_count(int B, int K, int max_len);      /* ints in `hist` for a draft of beam width K */
int p5_generate_draft(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                      int B, int L, int K, int max_len, const int* child_off, const int* child_tok, const int* child_node, const int* roots,
                      const uint32_t* excluded_nodes, int excluded_words, int max_children, int* out_seq, float* out_score, int* out_len,
                      int* hist, void* ws, int64_t ws_bytes, void* stream);
int64_t p5_verify_workspace_bytes(const P5Engine* e, int B, int L, int K, int Kw, int max_len, int max_children, int excluded_words);
int p5_verify_begin(P5Engine* e, int B, int L, int K, int Kw, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                    const int* roots, int max_children, int excluded_words, void* ws, int64_t ws_bytes);
int p5_verify_encode(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, void* stream);
const void* p5_verify_encoder_output(const P5Engine* e);     /* device fp32 [B*L, d_model], valid after p5_verify_encode until the next p5_verify_begin */
/* one-shot: the next p5_decode_begin / p5_generate / p5_generate_draft on `e` takes this fp32 encoder output [B*L, d_model] (cast to the
 * engine's dtype) instead of running its encoder */
int p5_generate_set_encoder_output(P5Engine* e, const float* enc_out_f32);
int p5_verify_plan(P5Engine* e, const int* hist, void* stream);
int p5_verify_row_capacity(int Kw, int max_len);           /* rows per user the workspace of a (Kw, max_len) verification holds (a multiple of 16) */
const int* p5_verify_plan_header(const P5Engine* e);     /* device int[4]: max rows per user, draft steps, total rows, overflow */
int p5_verify_run(P5Engine* e, int rows_per_user, const uint32_t* excluded_nodes, int* out_seq, float* out_score, int* out_len,
                  int* out_missing, void* stream);
/* ---- exhaustive catalogue ranking: the beam-search score of EVERY item of the trie in one pass (openp5_amd/csrc/p5_rank.h) ----
 * HF's beam search ranks an item by the sum of its tokens' log-probabilities up to and including </s>, divided by their number.  With one
 * decoder row per non-leaf trie node behind the decoder start token (the prefix that leads to it), ONE teacher-forced pass yields the
 * log-probability of every trie edge, an item's score is a sum along its path, and the ranked list is an exact top-N selection: what
 * p5_generate approaches as num_beams grows (DistributedRunner.py:204-269 widens the beam by the longest history), without a search.
 *   plan (host arrays on the device, ONE per trie, shared by all users -- openp5_amd/trie.py::CompiledTrie.rank_plan builds it):
 *     row_tok / row_depth / row_node [rows_per_user]: decoder input token, number of generated tokens, trie node of each prefix; parents
 *     precede children; row 0 = the decoder start token.  row_anc [rows_per_user][max_depth]: row of the ancestor at depth t < depth.
 *   item_edges [n_items][path_len]: edge ids (index into child_tok) of each item's path behind the start token, -1 beyond its </s>.
 *   excluded_items: optional uint32 [B, ceil(n_items / 32)]; bit i of row b set = item i is not ranked for user b (its score is still
 *     computed).  NULL = nothing excluded.
 *   out_index int32 / out_score fp32 [B, top_n]: the top_n items by (score desc, item index asc); fewer candidates: index -1, score -1e9.
 *   out_scores_all: optional fp32 [B, n_items], every item's score.  out_flagged int32 [B]: 1 = a value of the split-product pass left
 *     the range the two-term fp16 split covers (see verified generation above) -- that user's numbers are NOT to be used; call again for
 *     the user with exact_products = 1 (exact fp32 MFMAs; openp5_amd/model.py does).  Always 0 on a bf16 engine or with exact_products.
 * The pass lays its rows out [chunk][user][<= 512] so that each chunk is one cross-attention launch per layer; the tied head and the
 * scoring run in row chunks whose buffers do not grow with the catalogue.  Limits: top_n <= 4096, L <= 512, max_depth <= the half length of the bucket LUT bound to the engine, a tree-shaped
 * trie (no appended trie), B x rows_per_user x n_heads < 2^31.  Enqueues everything on `stream` and returns without synchronising. */
int64_t p5_rank_workspace_bytes(const P5Engine* e, int B, int L, int rows_per_user, int64_t n_edges, int n_items, int top_n);
int p5_rank_items(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                  const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                  const int* row_anc, int rows_per_user, int max_depth, const int* item_edges, int n_items, int path_len,
                  const uint32_t* excluded_items, int top_n, int exact_products, float* out_scores_all, int* out_index, float* out_score,
                  int* out_flagged, void* ws, int64_t ws_bytes, void* stream);
/* ---- per-user candidate lists: the exact score and order of C chosen items per user in one pass (openp5_amd/csrc/p5_cand.h) ----
 * The sampled-candidates evaluation protocol and re-ranking ask for the scores of a few items per user, not of the catalogue.  A user's
 * decoder rows are the non-leaf prefixes of that user's candidates only -- a subset of the rows of the exhaustive plan above that
 * contains every row's ancestors -- so the work and every buffer follow the candidates; none has a size that depends on the catalogue.
 *   candidates int32 [B, C]: item indices, -1 = empty slot; a user's items are distinct.
 *   item_rows int32 [n_items][path_len]: plan row (CompiledTrie.rank_plan numbering) of the item's prefix at each depth, -1 beyond its
 *     last non-leaf prefix.  item_tokens int64 [n_items][token_stride]: the sequences, column 0 = the decoder start token.
 *   row_tok / row_depth / row_anc: the trie's plan arrays, as above.
 * Protocol: (1) the plan call finds every user's rows on the device (sorted, distinct; integer sort and scan, no atomics) and writes
 * the largest row count of the batch into the first int32 of the workspace; (2) the host reads that ONE integer and makes sure the
 * workspace holds the workspace-bytes function's value for it -- the plan's part leads the workspace, is what that function returns
 * for rows_per_user = 0, and must be kept (or copied to the head of a larger workspace); (3) the score call runs encoder, decoder pass
 * ([chunk][user][<= 512] rows), head and scoring, and orders the slots.
 *   out_scores fp32 [B, C] in slot order (-1e9 for an empty slot); out_order int32 [B, top_n] slots by (score desc, item index asc),
 *   out_index / out_score their items and scores; ranks beyond a user's candidates: -1, -1, -1e9.  out_flagged / exact_products as above.
 * Limits: top_n <= C <= 4096, L <= 512, rows_per_user <= C x path_len, a tree-shaped trie.  Both calls enqueue on `stream` only. */
int64_t p5_cand_workspace_bytes(const P5Engine* e, int B, int L, int C, int path_len, int rows_per_user);
int p5_cand_plan(P5Engine* e, const int* candidates, int B, int C, const int* item_rows, int n_items, int path_len, void* ws, int64_t ws_bytes,
                 void* stream);
int p5_cand_score(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                  const int* row_tok, const int* row_depth, const int* row_anc, int max_depth, const int* candidates, int C, const int* item_rows,
                  const int64_t* item_tokens, int n_items, int path_len, int token_stride, int rows_per_user, int top_n, int exact_products,
                  float* out_scores, int* out_order, int* out_index, float* out_score, int* out_flagged, void* ws, int64_t ws_bytes, void* stream);
/* ---- certified pruned ranking: the bf16 pass proposes, an fp32 pass over the proposed prefixes decides (openp5_amd/csrc/p5_prune.h) ----
 * For a bf16 model: the top_n of p5_rank_items on the fp32 engine, at a cost that follows the prefixes within reach of the top_n-th item.
 * Besides p5_rank_items' trie / plan / path arrays (rows_total = its rows_per_user): row_edge int32 [rows_total] the edge leading into a
 * row (-1 for row 0), row_lmax int32 [rows_total] the largest token count of an item below the row, edge_row int32 [n_edges] the row of
 * an edge's child (-1 for a leaf) -- CompiledTrie.prune_plan.
 *   p5_prune_propose (the bf16 engine): p5_rank_items in `rank_ws` (out_index / out_score / out_flagged: its results), then per user the
 *     rows r with P(a) / row_lmax[a] >= out_score[top_n - 1] - slack for r and every ancestor a, ascending, into the head of `prune_ws`:
 *     int32 hdr[0] = the largest row count at byte 0 (the ONE integer the host reads), int32 n_rows[B] at byte 256, int32
 *     sel[B][rows_total] at byte 256 + (4 B rounded up to 256).  p5_prune_workspace_bytes(.., rows_per_user = 0, ..) = the head alone.
 *   p5_prune_decide (the fp32 engine; `prune_ws` sized for rows_per_user >= hdr[0], the head where propose left it): the decoder over
 *     sel, the log-probability of every child edge of every sel row, the top_n of the items scored in full (excluded_items applied), and
 *     the certificate: out_flagged[b] = 0 only when every item that was not scored is proven to score below out_score[b][top_n - 1] by
 *     more than `margin`.  A flagged user's outputs must not be used: rank that user with p5_rank_items.
 * Limits as p5_rank_items.  Both calls enqueue on `stream` only. */
int64_t p5_prune_workspace_bytes(const P5Engine* e, int B, int L, int rows_total, int rows_per_user, int64_t n_edges, int n_items, int top_n);
int p5_prune_propose(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                     const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                     const int* row_anc, int rows_total, int max_depth, const int* row_edge, const int* row_lmax, const int* item_edges, int n_items,
                     int path_len, const uint32_t* excluded_items, int top_n, float slack, int* out_index, float* out_score, int* out_flagged,
                     void* rank_ws, int64_t rank_ws_bytes, void* prune_ws, int64_t prune_ws_bytes, void* stream);
int p5_prune_decide(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                    const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                    const int* row_anc, int rows_total, int max_depth, const int* row_edge, const int* row_lmax, const int* edge_row,
                    const int* item_edges, int n_items, int path_len, const uint32_t* excluded_items, int top_n, int rows_per_user, float margin,
                    int* out_index, float* out_score, int* out_flagged, void* prune_ws, int64_t prune_ws_bytes, void* stream);
/* ---- bounded trie search: the exact top_n of p5_rank_items without a pass over the whole trie (openp5_amd/csrc/p5_bound.h) ----
 * For a bf16 model's fp32 engine and for an fp32 model.  The decoder runs over a per-user set of plan rows that starts from the prefixes
 * of a few seed sequences and grows, round by round, by exactly the frontier rows whose score bound still reaches the top_n-th score;
 * when nothing is admitted, the certificate of p5_prune_decide holds for the round that found it so.  Arrays as p5_prune_decide.
 * The head of the workspace: int32 hdr[0] = the largest row count at byte 0, int32 hdr[1] = the number of users whose set grew in the last
 * round at byte 4 (the TWO integers the host reads per round), int32 n_rows[B] at byte 256, int32 sel[B][rows_total] at byte 256 + (4 B
 * rounded up to 256), then the search's own scratch.  p5_bound_workspace_bytes(.., rows_per_user = 0, ..) = the head alone; the
 * workspace passed to every call must hold its value for the rows_per_user of that call, and its head must stay where it is.
 *   p5_bound_begin: the encoder and the cross-attention K/V of every decoder layer (they stay in the workspace for every round), then
 *     per user the plan rows of the prefixes of seeds int64 [B][n_seeds][seed_len] (token 0 = the decoder start; a sequence that leaves
 *     the trie or does not end on a leaf contributes nothing) plus row 0, sorted and distinct, into sel; hdr[0] set, hdr[1] = 0.
 *   p5_bound_round (rows_per_user >= hdr[0]): p5_prune_decide's pass over sel -- out_index / out_score / out_flagged as it leaves them --
 *     then sel grows by the child rows c outside it with NOT (UB(c) < out_score[top_n - 1] - margin); hdr[0], hdr[1] set.  Repeat while
 *     hdr[1] > 0, at most max_depth + 1 times; after a round with hdr[1] == 0 the outputs of that round are final, and a user with
 *     out_flagged set must be ranked with p5_rank_items.
 * Limits as p5_rank_items; 1 <= n_seeds <= 4096 and the same value in every call of a search.  All calls enqueue on `stream` only. */
int64_t p5_bound_workspace_bytes(const P5Engine* e, int B, int L, int rows_total, int rows_per_user, int64_t n_edges, int n_items, int top_n, int n_seeds,
                                 int max_depth);
int p5_bound_begin(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                   const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_node, int rows_total, int max_depth,
                   const int* edge_row, const int64_t* seeds, int n_seeds, int seed_len, int n_items, int top_n, void* ws, int64_t ws_bytes,
                   void* stream);
int p5_bound_round(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask, int B, int L,
                   const int* child_off, const int* child_tok, int64_t n_edges, const int* row_tok, const int* row_depth, const int* row_node,
                   const int* row_anc, int rows_total, int max_depth, const int* row_edge, const int* row_lmax, const int* edge_row,
                   const int* item_edges, int n_items, int path_len, const uint32_t* excluded_items, int top_n, int n_seeds, int rows_per_user,
                   float margin, int* out_index, float* out_score, int* out_flagged, void* ws, int64_t ws_bytes, void* stream);
/* Device-time brackets of p5_generate for benchmarks: p5_generate_timing(e, 1, NULL, NULL) arms it; after a p5_generate call,
 * p5_generate_timing(e, enable, &encode_ms, &decode_ms) WAITS for that call to finish and returns the time between its start and
 * its first decode step (encoder pass + cross-attention K/V projection + beam state) and the time of the decode loop itself. */
int p5_generate_timing(P5Engine* e, int enable, float* encode_ms, float* decode_ms);
/* The same search step by step (p5_generate = begin + (max_len - 1) x step + finish), for callers that interleave their own
 * work with the steps or want to stop early:
 *   p5_decode_begin   encoder, cross-attention K/V of every decoder layer, beam state (HF `_expand_inputs_for_generation`,
 *                     P5_T5.py:542-578, without physically repeating the encoder states num_beams times);
 *   p5_decode_step    one step: decoder over B*K rows with the KV cache, tied head, log-softmax over the full vocabulary,
 *                     trie mask, top-2K, BeamSearchScorer bookkeeping (HF generation/utils.py:3384-3483).  A no-op once the
 *                     search has stopped or max_len - 1 steps have run;
 *   p5_decode_done_flag  device pointer to an int that becomes 1 when the search has stopped (poll it asynchronously if
 *                     steps are enqueued one by one); NULL outside begin..finish;
 *   p5_decode_finish  writes the K best finished hypotheses per item (same outputs as p5_generate).
 * All arrays passed to p5_decode_begin must stay valid until p5_decode_finish; ws is p5_generate_workspace_bytes. */
int p5_decode_begin(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
                    int B, int L, int K, int max_len, const int* child_off, const int* child_tok, const int* child_node,
                    const int* roots, const uint32_t* excluded_nodes, int excluded_words, int max_children, void* ws, int64_t ws_bytes,
                    void* stream);
int p5_decode_step(P5Engine* e, void* stream);
const int* p5_decode_done_flag(const P5Engine* e);
int p5_decode_finish(P5Engine* e, int* out_seq, float* out_score, int* out_len, void* stream);
/* encoder only (JointEncoder.forward, P5_T5.py:74-204) */
int p5_encode(P5Engine* e, const int64_t* input_ids, const int64_t* whole_word_ids, const int64_t* attention_mask,
              int B, int L, void* enc_out /* T [B*L, d] */, void* ws, int64_t ws_bytes, void* stream);

/* ---- per-kernel entry points (parity tests) ---- */
/* C[M, N] = epi(alpha A B^T), C (ldc) written in [0:M, 0:N] only.  A K-contiguous operand may have K % 8 (bf16) / K % 4 (fp32) != 0 when
 * its leading dimension reaches the next multiple of 16 bytes: the elements in [K, round_up(K, 16 bytes)) of every row are padding, read but
 * never multiplied in, and may hold anything (NaN included); so may everything else past K, M or N in the operands and aux. */
int p5_op_gemm(int dtype, const void* A, const void* Bm, void* C, const void* aux, int M, int N, int K, int lda, int ldb,
               int ldc, int ldaux, int a_ks, int b_ks, int epi, int c_f32, int splitk, float alpha,
               const uint32_t* rng_state, uint32_t site, float drop_p, void* stream);
/* Persistent ring GEMM (openp5_amd/csrc/p5_gemm4.h), bf16 operands: up to 8 problems C[M,N] (+)= A B^T in ONE launch (the weight
 * gradients of a layer; nn.Linear autograd, DistributedRunner.py:80).  ks = 0: A [M, lda], B [N, ldb] (reduction dim contiguous);
 * ks = 1: A [K, lda], B [K, ldb] (reduction dim strided: dW = dy^T x).  epi as p5_op_gemm (0 store, 1 relu(+dropout), 2 residual +
 * dropout, 3 mask by aux > 0, 4 fp32 atomic add, 6 fp32 C += without split-K, 5 / 7 gated-GELU forward / backward, below).  tile_cfg 0 = 128x128, 1 = 256x128, 2 = 128x256, 3 = 256x128 loader / compute waves, 4 = 128x128 loader / compute waves.
 * rowss / ssq_out: optional T5LayerNorm statistics carried through the epilogue (row sum of squares in, sum of squares of the stored
 * row out), NULL = off.  `probs` is a HOST array. */
typedef struct P5GemmProblem {
  const void *A, *B; void* C; const void* aux;
  int M, N, K, lda, ldb, ldc, ldaux, epi, c_f32, splitk;
  float alpha;
  const float* rowss; float rowss_eps; float* ssq_out;
  int rowss_nt, ssq_nt;    /* > 0: the statistics are [rows, nt] partial sums (one per 64 columns), summed in index order / stored per tile; 0: one value per row */
  /* gated-GELU FFN (T5 v1.1, HF modeling_t5.py:97-123) fused into the GEMMs around it (tile_cfg 1, ks 0, whole 256x128 tiles):
   * epi 5 = forward: B = [wi_0; wi_1] ([2F, K], read gate-interleaved), N = 2F, C = h = dropout(gelu_new(u0) * u1) [M, F] (ldc), C2 = u =
   * [u0 | u1] [M, 2F] (ldc2) kept for the backward, gate_F = F;  epi 7 = backward: B = Wo^T [F, K], N = F, aux = u [M, 2F] (ldaux),
   * C = du = [dh u1 gelu'(u0) | dh gelu(u0)] [M, 2F] (ldc), dh = the product with the dropout mask of h re-applied; gate_F = 0 */
  void* C2; int ldc2, gate_F;
  /* epi 10 = T5LayerNorm backward (HF modeling_t5.py:59-72 under autograd) in the epilogue of the data-gradient GEMM that produces the
   * norm's input gradient (tile_cfg 4, ks 0, M % 128 == 0, N % 128 == 0, N = d_model): acc = dn = dOut W; aux = x [M, N] (ldaux) the
   * sub-layer's input rows, rowss / rowss_nt their partial sums of squares, nb_w [N] the norm weight, nb_dot [M, nb_dot_nt] partial sums
   * of <dOut, Out> per row (= sum_j (dn w)_j xh_j), nb_rin [M, N] fp32 incoming residual gradient.  Outputs: nb_rout [M, N] fp32 =
   * rstd (dn w - xh mean_j(dn w xh)) + nb_rin; C (ldc) = dropout(nb_rout) in bf16; C2 (ldc2, may be NULL) = w * round(x rstd);
   * nb_dw [M / 64, N] partial rows of the norm-weight gradient sum_rows dn xh.
   * epi 3 with ssq_out (tile_cfg 1): ssq_out[row][64-column group] = sum of C * aux / alpha (row sums of <d pre, pre>). */
  const float* nb_dot; int nb_dot_nt;
  const float* nb_rin; float* nb_rout;
  const float* nb_w; float* nb_dw;
} P5GemmProblem;
int p5_op_gemm_group(int tile_cfg, int ks, int nprob, const P5GemmProblem* probs, const uint32_t* rng_state, uint32_t site, float drop_p,
                     void* stream);
int p5_op_rmsnorm_fwd(int dtype, void* y, float* rstd, const void* x, const float* w, int rows, int d, float eps, void* stream);
int p5_op_rmsnorm_bwd(int dtype, float* dres_out, void* dy_next, float* dw, const void* dy, const void* x, const float* w,
                      const float* rstd, const float* dres_in, int rows, int d,
                      float* dw_partial /* scratch float[1024*d]: the engine's partial-sum mode; NULL = atomics */, void* stream);
int p5_op_attn_fwd(int dtype, const void* Q, const void* K, const void* V, void* O, float* lse, const float* rel_table,
                   const int* lut, int lut_half, const int64_t* kmask, int B, int H, int Lq, int Lk, int ldq, int ldk,
                   int ldv, int ldo, int causal, const uint32_t* rng_state, uint32_t site, float drop_p, void* stream);
/* d_rel_table [rel_buckets, H] (+=, may be NULL): the gradient of the relative-bias table is reduced WITHOUT fp32 atomics -- every
 * workgroup stores into its own slot of d_rel_scratch (caller-provided, room for float[B * ceil(Lq / 64)][rel_buckets * H]; the slots the launch uses are written in full, nothing is cleared) and the
 * slots are summed in index order, so the result is bit-reproducible. */
int p5_op_attn_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse,
                   float* Dvec, void* dQ, void* dK, void* dV, const float* rel_table, float* d_rel_table, float* d_rel_scratch,
                   int rel_buckets, const int* lut, int lut_half, const int64_t* kmask, int B, int H, int Lq, int Lk, int ldq, int ldk,
                   int ldv, int ldo, int lddq, int lddk, int lddv, int causal, const uint32_t* rng_state, uint32_t site, float drop_p,
                   void* stream);
/* the same, and dot_out [B * Lq, H] = <dQ, Q> + <dK, K> + <dV, V> per token and head from the values as stored: the row sums the
 * T5LayerNorm-backward epilogue of the qkv data-gradient GEMM consumes (P5GemmProblem epi 10).  bf16 self-attention with
 * 16 < Lq == Lk <= 128 (the fused backward kernel) only; NULL = p5_op_attn_bwd. */
int p5_op_attn_bwd_dot(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse,
                       float* Dvec, void* dQ, void* dK, void* dV, const float* rel_table, float* d_rel_table, float* d_rel_scratch,
                       int rel_buckets, const int* lut, int lut_half, const int64_t* kmask, int B, int H, int Lq, int Lk, int ldq, int ldk,
                       int ldv, int ldo, int lddq, int lddk, int lddv, int causal, const uint32_t* rng_state, uint32_t site, float drop_p,
                       float* dot_out, void* stream);
int p5_op_ce_fwd(float* nll, float* lse, const float* logits, const int64_t* labels, int rows, int V, int ldl, void* stream);
/* ---- the row kernels with every argument their launchers take, at the engine's launch geometry (tests/elem_matrix.py).  Dropout as in
 * p5_op_gemm: rng_state NULL or drop_p 0 = none; the element index is row * d + column. ---- */
/* T5LayerNorm forward with dropout on y (the final norms) */
int p5_op_rmsnorm_fwd_drop(int dtype, void* y, float* rstd, const void* x, const float* w, int rows, int d, float eps,
                           const uint32_t* rng_state, uint32_t site, float drop_p, void* stream);
/* T5LayerNorm backward: p5_op_rmsnorm_bwd plus dropout on the incoming dy (site_in) and on dy_next (site_next); ssq_part [rows, d / 64]
 * partial sums of squares of x instead of rstd (the folded-norm forward; rstd may then be NULL, eps is used), n_out T [rows, d] = the
 * forward norm's output recomputed (may be NULL) */
int p5_op_rmsnorm_bwd_full(int dtype, float* dres_out, void* dy_next, float* dw, const void* dy, const void* x, const float* w,
                           const float* rstd, const float* dres_in, int rows, int d, float* dw_partial, const uint32_t* rng_state,
                           uint32_t site_in, float drop_in_p, uint32_t site_next, float drop_next_p, const float* ssq_part, void* n_out,
                           float eps, void* stream);
/* out T [rows, d] = dropout(E[ids] (+ WW[ww] when WW != NULL)); ssq_part [rows, d / 64] (may be NULL) = sums of squares of the stored row
 * per 64 columns.  d a multiple of 64, <= 1024 */
int p5_op_embed_fwd(int dtype, void* out, const void* E, const void* WW, const int64_t* ids, const int64_t* ww, int rows, int d,
                    const uint32_t* rng_state, uint32_t site, float drop_p, float* ssq_part, void* stream);
/* Gradient of embedding lookups: table[key[r], :] += dropout(dres[r, :]) over one or two sets (HOST array), each the concatenation of up
 * to two key arrays with their own gradient rows and dropout sites.  mode 0: the fp32 atomic scatter (p5_set_option("embed_det", 0));
 * mode 1: the fixed-order chain of openp5_amd/csrc/p5_embed.h (sort chunks, rank, segmented sum, fix-up), whose grids the FIRST set sizes
 * (a later set may not be longer).  Scratch of mode 1, per set with n = n0 + n1, written by the chain and readable afterwards:
 * idx int[4 * n] = perm | skey | sstart | slen, csort uint64[ceil(n / 256) * 256], part float[ceil(n / 32) * 2 * d]. */
typedef struct P5EmbedBwdSet {
  const int64_t *key0, *key1;
  const float *dres0, *dres1;     /* fp32 [n0, d] / [n1, d] */
  int n0, n1;
  uint32_t site0, site1;
  float drop_p0, drop_p1;
  float* table;                   /* fp32 [*, d], += */
  int* idx;
  unsigned long long* csort;
  float* part;
} P5EmbedBwdSet;
int p5_op_embed_bwd(int dtype, int mode, int nsets, int d, const P5EmbedBwdSet* sets, const uint32_t* rng_state, void* stream);
/* p5_op_ce_fwd with the exponential of the mode (dtype 0: expf, 1: the fast exponential of the bf16 mode) */
int p5_op_ce_fwd_t(int dtype, float* nll, float* lse, const float* logits, const int64_t* labels, int rows, int V, int ldl, void* stream);
/* dlogits T [rows, ldd] = (softmax - onehot) * g, columns [V, ldd) zero; g = dnll[row], or with dnll NULL the masked-mean rule
 * out_attn[row] != 0 ? gscale / max(count of the row's batch item, 1) : 0 (out_attn [rows / T, T]); 0 where the label is -100.
 * grid_y = column slices per row (the engine: 1, 4 or 8 by row count).  g_out [rows] (may be NULL): the same g by p5_ce_gscale_kernel. */
int p5_op_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const int64_t* labels, const float* dnll, int rows,
                 int V, int ldl, int ldd, const int64_t* out_attn, int T, float gscale, int grid_y, float* g_out, void* stream);
/* the kernels of the trie-normalised item loss (p5_trie_ce.h; see p5_train_set_item_loss), one by one:
 * p5_op_trie_walk: labels int64 [B, T] -> node / state int32 [B * T] (node: whose children the row normalises over, -1 behind the end of the walk);
 * p5_op_trie_ce_fwd: nll / lse fp32 [rows] from fp32 logits [rows, ldl] (rows = B * T; dtype selects the exponential as in p5_op_ce_fwd_t);
 * p5_op_trie_ce_bwd: dlogits T [rows, ldd], zero outside the allowed children of scored rows, g * (exp(z - lse) - [child == label]) / temperature
 *   there; g by p5_op_ce_bwd's two rules, 0 for rows that are not scored. */
int p5_op_trie_walk(int* node, int* state, const int64_t* labels, const int* child_off, const int* child_tok, const int* child_node,
                    const uint32_t* excluded, int excl_words, int B, int T, int start_id, int eos_id, void* stream);
int p5_op_trie_ce_fwd(int dtype, float* nll, float* lse, const float* logits, const int64_t* labels, const int* node, const int* state,
                      const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words, float temperature,
                      int rows, int T, int ldl, void* stream);
int p5_op_trie_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const int64_t* labels, const int* node, const int* state,
                      const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words,
                      float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn, float gscale, void* stream);
/* the kernels of the truncated item loss (p5_trunc.h; see p5_train_set_item_loss_truncated), one by one:
 * p5_op_trunc_cut: fp32 logits [rows, ldl], node int32 [rows] (< 0: no node) -> cut fp32 [rows] (min z over the kept set, +inf where nothing is
 *   kept) and kept int32 [rows] (size of the kept set); rows_per_user consecutive rows share a row of the excluded bitmap;
 * p5_op_trunc_ce_fwd: p5_op_trie_ce_fwd over the kept set, plus row_cut fp32 [rows]; state int32 [rows] is read (the walk's) AND written (3
 *   where the label lies below the cut);
 * p5_op_trunc_ce_bwd: p5_op_trie_ce_bwd with entries only where z >= row_cut[row]. */
int p5_op_trunc_cut(float* cut, int* kept, const float* logits, const int* node, const int* child_off, const int* child_tok, const int* child_node,
                    const uint32_t* excluded, int excl_words, float temperature, int top_k, float top_p, int rows, int rows_per_user, int ldl,
                    void* stream);
int p5_op_trunc_ce_fwd(int dtype, float* nll, float* lse, float* row_cut, int* state, const float* logits, const int64_t* labels, const int* node,
                       const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words, float temperature,
                       int top_k, float top_p, int rows, int T, int ldl, void* stream);
int p5_op_trunc_ce_bwd(int dtype, void* dlogits, const float* logits, const float* lse, const float* row_cut, const int64_t* labels, const int* node,
                       const int* state, const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const uint32_t* excluded,
                       int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn, float gscale, void* stream);
/* the kernels of the restricted item head (p5_item_head.h; see p5_train_set_item_head), one by one:
 * p5_op_item_gather: EU T [Nup, d] = rows `tokens` of E T [*, d], rows [n_tokens, Nup) zeros (Nup = n_tokens rounded up to 64; d a multiple of 16 bytes);
 * p5_op_item_scatter: dEU fp32 [Nup, d] into dE fp32 [V, d].  store != 0: every row v < V is written, dEU[index of v in tokens] or zeros;
 *   store == 0: dE[tokens[r]] += dEU[r] for r < n_tokens, every other row untouched.  tokens ascending and distinct, all < V;
 * p5_op_*_cols: the four cross-entropy entries above on a COMPACT row -- child_col int32 [n_edges] gives the column of an edge's token in
 *   logits [rows, ldl] and dlogits [rows, ldd]; labels, nodes, states and the bitmap stay on tokens and nodes.  The arithmetic per child and
 *   the order of reduction are those of the dense entries: on equal logits nll, lse, row_cut and the entries of dlogits are equal bit for bit. */
int p5_op_item_gather(int dtype, void* EU, const void* E, const int* tokens, int n_tokens, int d, void* stream);
int p5_op_item_scatter(float* dE, const float* dEU, const int* tokens, int n_tokens, int V, int d, int store, void* stream);
int p5_op_trie_ce_fwd_cols(int dtype, float* nll, float* lse, const float* logits, const int64_t* labels, const int* node, const int* state,
                           const int* child_off, const int* child_tok, const int* child_node, const int* child_col, const uint32_t* excluded, int excl_words,
                           float temperature, int rows, int T, int ldl, void* stream);
int p5_op_trie_ce_bwd_cols(int dtype, void* dlogits, const float* logits, const float* lse, const int64_t* labels, const int* node, const int* state,
                           const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                           const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn,
                           float gscale, void* stream);
/* the kernels of the regularised item loss (p5_trie_reg.h; see p5_train_set_item_regularizers), one by one; child_col NULL = the dense row:
 * p5_op_trie_reg_fwd: p5_op_trie_ce_fwd[_cols] (the same bits in nll / lse) plus entropy fp32 [rows] and, with ref_logits fp32 [rows, ld_ref],
 *   kl and lse_ref fp32 [rows] (all three may be NULL together);
 * p5_op_trie_reg_bwd: p5_op_trie_ce_bwd[_cols]'s row with the two regularisers' gradients added in the same store; entropy / kl / lse_ref as the
 *   forward wrote them; seeds dnll / d_entropy / d_kl fp32 [rows] (the last two may be NULL = zeros), or -- dnll NULL -- from out_attn:
 *   base = [out_attn != 0] gscale / max(count, 1), g_nll = base, g_H = -entropy_coef * base, g_KL = kl_coef * base. */
int p5_op_trie_reg_fwd(int dtype, float* nll, float* lse, float* entropy, float* kl, float* lse_ref, const float* logits, const float* ref_logits,
                       const int64_t* labels, const int* node, const int* state, const int* child_off, const int* child_tok, const int* child_node,
                       const int* child_col, const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ld_ref,
                       void* stream);
int p5_op_trie_reg_bwd(int dtype, void* dlogits, const float* logits, const float* ref_logits, const float* lse, const float* entropy, const float* kl,
                       const float* lse_ref, const int64_t* labels, const int* node, const int* state, const float* dnll, const float* d_entropy,
                       const float* d_kl, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                       const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ld_ref, int ldd,
                       const int64_t* out_attn, float gscale, float entropy_coef, float kl_coef, void* stream);
int p5_op_trunc_ce_fwd_cols(int dtype, float* nll, float* lse, float* row_cut, int* state, const float* logits, const int64_t* labels, const int* node,
                            const int* child_off, const int* child_tok, const int* child_node, const int* child_col, const uint32_t* excluded,
                            int excl_words, float temperature, int top_k, float top_p, int rows, int T, int ldl, void* stream);
int p5_op_trunc_ce_bwd_cols(int dtype, void* dlogits, const float* logits, const float* lse, const float* row_cut, const int64_t* labels, const int* node,
                            const int* state, const float* dnll, const int* child_off, const int* child_tok, const int* child_node, const int* child_col,
                            const uint32_t* excluded, int excl_words, float temperature, int rows, int T, int ldl, int ldd, const int64_t* out_attn,
                            float gscale, void* stream);
/* loss[0] = mean_b(sum_t nll[b, t] m[b, t] / max(sum_t m[b, t], 1)), m = (out_attn != 0) */
int p5_op_masked_mean(float* loss, const float* nll, const int64_t* out_attn, int B, int T, void* stream);
/* The loss of p5_forward_loss_targets and its gradient with respect to the per-token NLL: loss[0] = mean_b(tw[b] * masked mean of nll[b, :]),
 * g_out [B * T] = out_attn != 0 ? gscale / max(count of the row's b, 1) * tw[b] : 0, and 0 where labels == -100 (tw may be NULL = 1).
 * merged 1: one launch (p5_masked_mean_g_kernel, the engine's route under p5_set_option("loss_fuse", 1)); merged 0: the loss kernel and the
 * stand-alone scale kernel.  Both give the same bits. */
int p5_op_masked_mean_g(int merged, float* loss, float* g_out, const float* nll, const int64_t* out_attn, const int64_t* labels, const float* tw, int B, int T,
                        float gscale, void* stream);
/* The batch of an on-policy fine-tuning step from what p5_sample_items / p5_sample_slates returned (p5_policy.h), two launches on `stream`,
 * no host synchronisation, no engine.  sequences int64 [B*S, Ts] (decoder start first, the drawn tokens through eos_id, pad_id behind; an
 * all-pad row = nothing drawn); labels / output_attention int64 [B, Tg]: every user's gold target (attended: output_attention != 0 in
 * front of the first -100 label, which ends the gold); rewards fp32 [B, S] or NULL = the hit reward (1 where the draw equals the gold's attended tokens, else 0).
 * baseline 0 none / 1 mean / 2 loo (S >= 2) / 3 grpo (adv_eps added to the population standard deviation).  With G = S + with_gold and
 * To = max(Tg, Ts - 1): labels_out / attention_out int64 [B, G, To] (slot 0 the gold when with_gold, then the draws), rewards_out /
 * advantages fp32 [B, S], weights_out fp32 [B, G] -- w[b, 0] = sft_coef G, w[b, s] = policy_coef A[b, s] G / S (times the draw's token count
 * when token_sum): the target_weights of p5_forward_loss_targets --, user_stats fp32 [B, 4] (scratch of the second launch), stats fp32 [8]:
 * mean reward of the existing draws, share of users whose draws differ in reward, mean |A|, share of draws equal to the gold, share of users
 * with such a draw, users without a draw, 0, 0.  No atomics: equal inputs give equal bits.  Non-zero (p5_last_error) for S < 1, S > 1024,
 * loo with S < 2, an unknown baseline, non-finite coefficients, NULL required pointers. */
int p5_policy_batch(const int64_t* sequences, const int64_t* labels, const int64_t* output_attention, const float* rewards, int B, int S, int Ts,
                    int Tg, int baseline, float policy_coef, float sft_coef, int token_sum, float adv_eps, int with_gold, int pad_id, int eos_id,
                    int64_t* labels_out, int64_t* attention_out, float* rewards_out, float* advantages, float* weights_out, float* user_stats,
                    float* stats, void* stream);
/* p5_policy_batch plus the clipped objective's inputs: token_logprobs fp32 [B*S, Ts-1] (the sampler's) in; old_logprobs_out fp32 [B, G, To]
 * (the draws' token log-probabilities at their label positions; the gold slot and positions behind a draw's end: 0) and target_mode_out
 * int32 [B, G] (gold 0, draws 1) out.  Every other output carries the bits of p5_policy_batch. */
int p5_policy_batch_clip(const int64_t* sequences, const int64_t* labels, const int64_t* output_attention, const float* rewards,
                         const float* token_logprobs, int B, int S, int Ts, int Tg, int baseline, float policy_coef, float sft_coef, int token_sum,
                         float adv_eps, int with_gold, int pad_id, int eos_id, int64_t* labels_out, int64_t* attention_out, float* rewards_out,
                         float* advantages, float* weights_out, float* user_stats, float* stats, float* old_logprobs_out, int* target_mode_out,
                         void* stream);
/* The batch of an on-policy step from SLATES (p5_slate_policy.h): the importance-weighted without-replacement estimator of Kool, van Hoof and
 * Welling on what p5_sample_slates(slate_size = K1 = K + 1) returned; two launches on `stream`, stateless.  Per user S slates of K1 slots:
 * sequences int64 [B*S*K1, Ts], sequences_logprob fp32 [B*S*K1] (log p(item)), perturbed fp32 [B, S, K1] (descending); slot K of a slate is the
 * threshold kappa only and becomes no training row (kappa = -inf: the allowed items ran out, every slot has inclusion probability 1).
 * rewards fp32 [B, S, K1] (the last slot is never read) or NULL = the hit reward; token_logprobs fp32 [B*S*K1, Ts-1] or NULL.
 * omega = p / q_kappa, q_kappa = 1 - exp(-exp(log p - kappa)); estimator 0 unbiased A = omega r, 1 normalized A = (omega / W)(r - V / W) with
 * W = sum omega, V = sum omega r over the slate's existing slots (K >= 2).  With G = S*K + with_gold, To = max(Tg, Ts - 1): labels_out /
 * attention_out int64 [B, G, To] (slot 0 = the gold when with_gold, then the slates in (slate, slot) order), rewards_out / advantages /
 * importance fp32 [B, S, K], weights_out fp32 [B, G] (w[b, 0] = sft_coef G, the others policy_coef A G / S, times the token count when
 * token_sum), slate_stats fp32 [B, S, 4] = (V, W, kappa, W^2 / sum omega^2), user_stats fp32 [B, 8] (scratch of the second launch), stats
 * fp32 [8]: mean V and mean W over the slates with an existing slot, share of users with a non-zero advantage, mean |A|, share of slates
 * that contain the gold, share of slates with kappa = -inf, users without a draw, mean effective sample size.  old_logprobs_out fp32
 * [B, G, To] (with token_logprobs, else NULL) and target_mode_out int32 [B, G] (nullable) as p5_policy_batch_clip writes them.  No atomics.
 * root_streams int32 [B] (nullable) with root_seed / slate_base: the stream ids, seed and slate_base the slates were drawn with by
 * p5_sample_slates, whose root starts at G = 0 (the maximum of the perturbed values is conditioned to be 0): kappa is then un-conditioned
 * with one Exp(1) draw per slate, E = -log u(seed, stream, slate, step 0, edge 2^32 - 1) of p5_rng.h, kappa = g[K] - log1p((E - 1) exp(g[K])).
 * NULL: perturbed holds unconditioned values log p + Gumbel and kappa = g[K] as it is.  slate_stats reports the kappa that was used.
 * Non-zero (p5_last_error) for NULL required pointers, K1 < 2, S * K1 > 1024, Ts < 2, an unknown estimator, normalized with K1 = 2. */
int p5_policy_slate_batch(const int64_t* sequences, const float* sequences_logprob, const float* perturbed, const int64_t* labels,
                          const int64_t* output_attention, const float* rewards, const float* token_logprobs, int B, int S, int K1, int Ts, int Tg,
                          int estimator, float policy_coef, float sft_coef, int token_sum, int with_gold, int pad_id, int eos_id, int64_t* labels_out,
                          int64_t* attention_out, float* rewards_out, float* advantages, float* importance, float* weights_out, float* slate_stats,
                          float* user_stats, float* stats, float* old_logprobs_out, int* target_mode_out, const int* root_streams, uint32_t root_seed,
                          uint32_t slate_base, void* stream);
/* The two kernels of p5_train_set_clip_objective behind a given per-token NLL, no engine: nll / old_logprobs fp32 [B*G*T], out_attn / labels
 * int64 [B*G*T], tw fp32 [B*G] or NULL, target_mode int32 [B*G] or NULL, entropy_rows / kl_rows fp32 [B*G*T] or NULL (the regularised loss:
 * terms fp32 [3] or NULL receives its parts, row_seed is [3*B*G*T] then, else [B*G*T]), user_partials fp32 [B*16], clip_stats fp32 [8]. */
int p5_op_clip_objective(float* loss, float* terms, float* row_seed, float* user_partials, float* clip_stats, const float* nll,
                         const float* old_logprobs, const int64_t* out_attn, const int64_t* labels, const float* tw, const int* target_mode,
                         const float* entropy_rows, const float* kl_rows, float entropy_coef, float kl_coef, float eps_low, float eps_high,
                         int ratio_mode, int B, int G, int T, void* stream);
/* The two kernels of p5_train_set_pref_objective behind a given per-token NLL, no engine: nll fp32 [B*G*T], ref_logprobs fp32 [B*G*T] or NULL,
 * out_attn / labels int64 [B*G*T], pref_mask int32 [B*G] or NULL; row_seed fp32 [B*G*T], user_partials fp32 [B*16], pref_stats fp32 [8].
 * 1 <= G <= 512. */
int p5_op_pref_objective(float* loss, float* row_seed, float* user_partials, float* pref_stats, const float* nll, const float* ref_logprobs,
                         const int64_t* out_attn, const int64_t* labels, const int* pref_mask, int kind, float beta, int depth, int length_normalize,
                         float sft_coef, int B, int G, int T, void* stream);
/* decode-step projection over a few hundred rows (p5_decode2.h): C = A W^T, W = T [N, ldw].  amode 0: A = T [M, lda];
 * amode 1: A = fp32 residual stream [M, K], normalised with T5LayerNorm weight `ln` by the kernel itself.
 * (K <= 1024 then).  epi: 0 store T (alpha), 1 relu store T, 2 fp32 atomic accumulate (split-K), 3 store fp32 (alpha), 4 fp32 += by one writer */
int p5_op_skinny_gemm(int dtype, int amode, const void* A, int lda, const float* ln, const void* W, int ldw, void* C, int ldc,
                      int M, int N, int K, int epi, float alpha, float eps, void* stream);
/* decode-step cross-attention of the Kb beams of each of B items (p5_decode2.h): q T [B*Kb, H*64], kv T [B*L, 2*H*64] (K then V),
 * mask int64 [B, L]; zero position bias (HF modeling_t5.py:336-343).  variant 3 = matrix-core kernel, 2 = scalar kernel */
int p5_op_dec_cross_attn(int dtype, int variant, void* out, const void* q, const void* kv, const int64_t* mask, int B, int H, int Kb,
                         int L, void* stream);
/* ---- the kernels of the decode step, each through the launcher the engine uses (tests/decode_matrix.py).  `done` (may be NULL): device
 * flag, != 0 -> the launch writes nothing.  Every entry refuses (error code, nothing launched) a shape its kernel cannot handle. ---- */
/* p5_op_dec_cross_attn with a free row stride of kv (ldkv >= 2*H*64 elements: the layer's K|V block inside a wider row) and, with x != NULL
 * (bf16 only; q ignored), the kernel's own q projection: q = T(T5LayerNorm(x fp32 [B*Kb, d], weight ln, eps) Wq^T), Wq T [H*64, d]; refused
 * when the rows and the Wq slice do not fit the LDS (d_model > 512) */
int p5_op_dec_cross_attn_ex(int dtype, int variant, void* out, const void* q, const float* x, const float* ln, const void* Wq, const void* kv,
                            int ldkv, const int64_t* mask, int B, int H, int Kb, int L, int d, float eps, const int* done, void* stream);
/* single-token self-attention over the ancestry-indexed cache: qkv T [R, 3*H*64] (this step's q | k | v), cache T [max_len][R][2*H*64];
 * step[0] = cur_len (1 .. max_len, on the device); this step's k, v are written at position cur_len - 1; position t < cur_len - 1 of row r is
 * read from row anc[t*R + r], anc = anc_odd for odd cur_len, else anc_even; bias rel_table[lut[t - pos + lut_half]*H + h]; out T [R, H*64] */
int p5_op_dec_self_attn(int dtype, void* out, const void* qkv, void* cache, const int* anc_odd, const int* anc_even, const float* rel_table,
                        const int* lut, int lut_half, int R, int H, const int* step, int max_len, const int* done, void* stream);
/* y T [rows, d] = w * T(x / rms(x)), x fp32 [rows, d]; d a multiple of 8, <= 1024 */
int p5_op_rmsnorm_f32in(int dtype, void* y, const float* x, const float* w, int rows, int d, float eps, const int* done, void* stream);
/* streaming tied head: per tile t of nv rows of E (T [V, d]) and row r of hn (T [R, d]): part_m[r*nt + t] = max, part_s = sum exp(. - max)
 * of alpha * hn[r] . E[v]; nt = ceil(V / nv); nv 16/32/64/128 with nv*d*sizeof(T) <= 128 KiB (64 KiB for 16), d % 256 (bf16) / 128 (fp32) == 0 */
int p5_op_head_lse(int dtype, int nv, float* part_m, float* part_s, const void* hn, const void* E, int R, int d, int V, float alpha,
                   const int* done, void* stream);
/* per decode row r (R rows): the best K2 children c of trie node node[r] (CSR child_off / child_tok / child_node; at most max_c), scored
 * log_softmax(logits[r])[child_tok] + run_score[r], in (score desc, child asc) order -> top_score / top_c [R, K2], n_top [R]; children whose
 * node's bit is set in excluded[(r / Kb) * excl_words ..] are dropped; node < 0: n_top = 0.  streaming 1: the log-sum-exp from part_m / part_s
 * [R, ntiles] and the logits as alpha * hn[r] . E[tok] (T, d <= 1024); streaming 0: fp32 logits [R, ldl], V columns.  cand_scratch fp32
 * [R, max_c]: needed for fan-outs above 2048 */
int p5_op_dec_score(int dtype, int streaming, const float* part_m, const float* part_s, int ntiles, const void* hn, const void* E, int d,
                    float alpha, const float* logits, int ldl, int V, const int* node, const float* run_score, const int* child_off,
                    const int* child_tok, const int* child_node, const uint32_t* excluded, int excl_words, int R, int Kb, int max_c, int K2,
                    float* cand_scratch, float* top_score, int* top_c, int* n_top, const int* done, void* stream);
/* ---- catalogue ranking (csrc/p5_rank.h, p5_cand.h, p5_prune.h, p5_bound.h and p5_tree_attn_row) through the launch helpers the engine uses;
 * tests/rank_matrix.py.  Layout of a pass: B * CQ * nchunk rows, row ru of user b at ((ru / CQ) * B + b) * CQ + ru % CQ. ---- */
/* the streaming head's tile (rows of E per workgroup) the engine picks for a model of this type and width; 0: materialised logits */
int p5_op_head_nv(int dtype, int d_model);
/* items 1: scores [B, n_items] = the depth-ordered sum of edge_lp [B, n_edges] over item_edges [n_items, path_len] (-1 ends a path) / the
 * number of edges (none: -1e9), then the selection; 2: the item scores only; 0: scores are given.  Selection: per user the top_n items by
 * (score desc, index asc) outside the bitmap excluded [B, ceil(n_items / 32)] -> out_index / out_score [B, top_n] (-1 / -1e9 beyond the live
 * items; with items 2 part, out_index and out_score may be null).  grid (host, may be null) receives G, S of the first stage; part: [B, G, top_n] 64-bit scratch, G <= 64 */
int p5_op_rank_select(int items, float* scores, const float* edge_lp, int64_t n_edges, const int* item_edges, int n_items, int path_len,
                      const uint32_t* excluded, unsigned long long* part, int B, int top_n, int* out_index, float* out_score, int* grid, void* stream);
/* edge_lp[b, child_off[nd] + i] = log_softmax(d^-0.5 hn[g] . E^T)[child_tok[..]] for every child i of node nd = row_node[plan row] of every pass
 * row g that is no padding; plan row = the user's row (< rows) or, with sel [B, cap] / n_rows [B], sel[b][row].  nv > 0: streaming head of
 * that tile (p5_op_head_lse's conditions), head fp32 [2, HC, ceil(V / nv)]; nv 0: materialised logits, head fp32 [HC, V rounded up to 64].
 * HC = rows per head chunk.  d a multiple of 64 (bf16) / 32 (fp32), <= 1024 */
int p5_op_rank_edges(int dtype, int nv, float* edge_lp, int64_t n_edges, const void* hn, const void* E, int d, int V, float* head, int HC,
                     const int* row_node, int rows, int B, int CQ, int nchunk, const int* sel, const int* n_rows, int cap, const int* child_off,
                     const int* child_tok, void* stream);
/* row_lse[g] = log sum exp(d^-0.5 hn[g] . E^T) for the R rows of a pass, by the two head routes of p5_op_rank_edges */
int p5_op_cand_row_lse(int dtype, int nv, float* row_lse, const void* hn, const void* E, int d, int V, float* head, int HC, int R, void* stream);
/* self-attention of every pass row over its ancestors and itself; qkv T [R, 3*H*64], out T [R, H*64], bias rel_table[lut[t - depth + lut_half]*H + h].
 * variant 0 (p5_rank_tree_attn_kernel): plan rows row_depth [rows], anc [rows, max_depth]; 1 (p5_cand_tree_attn_kernel): the same plan through
 * sel / n_rows; 2 (p5_tree_attn_kernel): row_depth = depth per pass row [B * CQ], anc [B, cap, max_depth], nchunk 1 */
int p5_op_tree_attn(int dtype, int variant, void* out, const void* qkv, const int* row_depth, const int* anc, int rows, int max_depth, int B, int CQ,
                    int nchunk, const int* sel, const int* n_rows, int cap, const float* rel_table, const int* lut, int lut_half, int H, void* stream);
/* p5_cand_plan_kernel + p5_cand_hdr_kernel: sel [B, cap], n_rows [B], hdr[0] = the largest n_rows; keys [B, P] scratch */
int p5_op_cand_plan(int* sel, int* n_rows, int* hdr, unsigned long long* keys, const int* cand, const int* item_rows, int B, int C, int n_items,
                    int path_len, int cap, int P, void* stream);
/* p5_cand_rows_kernel: decoder input ids [B * CQ * nchunk] of a pass over sel */
int p5_op_cand_rows(int64_t* ids, const int* row_tok, int B, int CQ, int nchunk, const int* sel, const int* n_rows, int cap, int pad_id, void* stream);
/* p5_cand_score_kernel + p5_cand_order_kernel: scores [B, C], out_order / out_index / out_score [B, top_n] */
int p5_op_cand_score(int dtype, float* scores, const void* hn, const void* E, int d, const float* row_lse, int B, int CQ, int nchunk, const int* sel,
                     const int* n_rows, int cap, const int* cand, int C, const int* item_rows, const int64_t* item_tok, int ldt, int n_items,
                     int path_len, int* out_order, int* out_index, float* out_score, int top_n, void* stream);
int p5_op_prune_fill(float* p, int64_t n, float v, void* stream);
/* p5_prune_propose_kernel + p5_cand_hdr_kernel: sel [B, rows], n_rows [B], hdr[0]; top_score [B, N] */
int p5_op_prune_propose(int* sel, int* n_rows, int* hdr, const float* edge_lp, int64_t n_edges, const float* top_score, int N, const int* row_depth,
                        const int* anc, int rows, int max_depth, const int* row_edge, const int* row_lmax, float slack, int B, void* stream);
int p5_op_prune_mask(uint32_t* out, const uint32_t* excluded, const float* edge_lp, int64_t n_edges, const int* item_edges, int n_items, int path_len,
                     int B, void* stream);
/* p5_prune_certify_kernel over sel [B, cap] / n_rows of a pass of CQ * nchunk rows per user: flagged[b] = 1 unless the list is proven complete */
int p5_op_prune_certify(int* flagged, const float* edge_lp, int64_t n_edges, const int* row_depth, const int* row_node, const int* anc, int max_depth,
                        int B, int CQ, int nchunk, const int* sel, const int* n_rows, int cap, const int* row_edge, const int* edge_row,
                        const int* row_lmax, const int* child_off, const int* out_index, const float* out_score, int N, float margin, void* stream);
/* p5_bound_seed_kernel + p5_bound_union_kernel + p5_bound_hdr_kernel: seeds int64 [B, S, T]; keys [B, KP], KP a power of two >= S * max_depth + 1 */
int p5_op_bound_seed(int* sel, int* n_rows, int* hdr, unsigned long long* keys, int KP, int cap, const int64_t* seeds, int S, int T,
                     const int* child_off, const int* child_tok, const int* edge_row, const int* row_tok, const int* row_node, int max_depth, int B,
                     void* stream);
/* p5_bound_expand_kernel + p5_bound_hdr_kernel: sel / n_rows read and written, grew [B], hdr = (largest n_rows, users that grew) */
int p5_op_bound_expand(int* sel, int* n_rows, int* grew, int* hdr, unsigned long long* keys, int KP, const float* edge_lp, int64_t n_edges,
                       const int* row_depth, const int* row_node, const int* anc, int max_depth, int B, int CQ, int nchunk, int cap,
                       const int* row_edge, const int* edge_row, const int* row_lmax, const int* child_off, const float* out_score, int N, float margin,
                       void* stream);
int p5_op_tr_probe(void* out64x4_u16, const void* in256_u16, void* stream);  /* ds_read_b64_tr_b16 semantics probe */

#ifdef __cplusplus
}
#endif
#endif
