"""ctypes prototypes for include/p5hip.h (one table, used by the product loader and by the test-only emulator
loader so both bind exactly the symbols the header declares)."""
import ctypes as C

c_i64p = C.POINTER(C.c_int64)
vp, i32, i64, f32, f64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_uint32


class P5Config(C.Structure):
    _fields_ = [
        ("vocab_size", i32), ("d_model", i32), ("d_kv", i32), ("d_ff", i32), ("n_enc_layers", i32),
        ("n_dec_layers", i32), ("n_heads", i32), ("rel_buckets", i32), ("rel_max_distance", i32),
        ("whole_word_size", i32), ("gated_gelu", i32), ("dtype", i32), ("eps", f32), ("dropout", f32),
        ("pad_id", i32), ("eos_id", i32),
    ]


class P5GemmProblem(C.Structure):
    _fields_ = [("A", vp), ("B", vp), ("C", vp), ("aux", vp), ("M", i32), ("N", i32), ("K", i32), ("lda", i32), ("ldb", i32), ("ldc", i32),
                ("ldaux", i32), ("epi", i32), ("c_f32", i32), ("splitk", i32), ("alpha", f32), ("rowss", vp), ("rowss_eps", f32), ("ssq_out", vp), ("rowss_nt", i32), ("ssq_nt", i32),
                ("C2", vp), ("ldc2", i32), ("gate_F", i32),
                ("nb_dot", vp), ("nb_dot_nt", i32), ("nb_rin", vp), ("nb_rout", vp), ("nb_w", vp), ("nb_dw", vp)]


class P5EmbedBwdSet(C.Structure):
    _fields_ = [("key0", vp), ("key1", vp), ("dres0", vp), ("dres1", vp), ("n0", i32), ("n1", i32), ("site0", u32), ("site1", u32),
                ("drop_p0", f32), ("drop_p1", f32), ("table", vp), ("idx", vp), ("csort", vp), ("part", vp)]


# name -> (restype, argtypes)
PROTOTYPES = {
    "p5_last_error": (C.c_char_p, []),
    "p5_set_option": (i32, [C.c_char_p, i32]),
    "p5_abi_version": (i32, []),
    "p5_is_emulator": (i32, []),
    "p5_engine_create": (i32, [C.POINTER(P5Config), C.POINTER(vp)]),
    "p5_engine_destroy": (i32, [vp]),
    "p5_param_count": (i64, [vp]),
    "p5_param_table": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]),
    "p5_engine_bind": (i32, [vp, vp, vp, vp, vp, vp, i32, vp]),
    "p5_refresh_shadow": (i32, [vp, vp]),
    "p5_transposed_bytes": (i64, [vp]),
    "p5_engine_bind_transposed": (i32, [vp, vp, vp]),
    "p5_refresh_transposed": (i32, [vp, vp]),
    "p5_engine_set_side_stream": (i32, [vp, vp]),
    "p5_train_workspace_bytes": (i64, [vp, i32, i32, i32]),
    "p5_forward": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i64, vp]),
    "p5_forward_loss": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i64, vp]),
    "p5_train_workspace_bytes_targets": (i64, [vp, i32, i32, i32, i32]),
    "p5_forward_targets": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i64, vp]),
    "p5_forward_loss_targets": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, i64, vp]),
    "p5_train_set_item_loss": (i32, [vp, vp, vp, vp, i32, vp, i32, f32, vp]),
    "p5_train_set_item_loss_truncated": (i32, [vp, vp, vp, vp, i32, vp, i32, f32, vp, i32, f32, vp]),
    "p5_item_head_workspace_bytes": (C.c_size_t, [vp, i32, i32, i32]),
    "p5_train_set_item_head": (i32, [vp, vp, i32, vp, vp, C.c_size_t]),
    "p5_train_set_item_regularizers": (i32, [vp, vp, i32, vp, f32, f32, vp]),
    "p5_backward_set_item_grads": (i32, [vp, vp, vp]),
    "p5_train_set_pref_objective": (i32, [vp, vp, vp, i32, f32, i32, i32, f32, vp, vp, vp]),
    "p5_train_set_clip_objective": (i32, [vp, vp, vp, f32, f32, i32, vp, vp, vp]),
    "p5_train_last_item_logits": (i32, [vp, vp, vp, vp, vp]),
    "p5_backward_num_stages": (i32, [vp]),
    "p5_backward_stage": (i32, [vp, vp, i32, vp]),
    "p5_backward": (i32, [vp, vp, vp]),
    "p5_backward_stage_range": (i32, [vp, i32, C.POINTER(i64), C.POINTER(i64)]),
    "p5_backward_final_range": (i32, [vp, C.POINTER(i64), C.POINTER(i64)]),
    "p5_backward_stage_pairs": (i32, [vp, i32]),
    "p5_backward_staged": (i32, [vp, vp, vp, C.POINTER(i64), i32, C.POINTER(i32)]),
    "p5_backward_staged_wait": (i32, [vp, i32, vp]),
    "p5_allreduce_range": (i32, [vp, i32, vp, vp, vp]),
    "p5_allreduce_sum": (i32, [vp, i64, i32, vp, vp]),
    "p5_grad_sumsq": (i32, [vp, i64, vp, vp]),
    "p5_adamw_step": (i32, [vp, vp, vp, vp, vp, i64, vp, f64, f64, f64, f64, f64, f64, f64, i32, vp]),
    "p5_engine_adamw_step": (i32, [vp, vp, vp, vp, f64, f64, f64, f64, f64, f64, f64, i32, C.POINTER(i32), vp]),
    "p5_engine_grads_zeroed": (i32, [vp]),
    "p5_engine_clear_grads": (i32, [vp, vp]),
    "p5_engine_discard_grads": (i32, [vp]),
    "p5_generate_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32, i32]),
    "p5_generate": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i64, vp]),
    "p5_generate_set_forced_prefix": (i32, [vp, vp, vp, i32]),
    "p5_sample_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32, i32]),
    "p5_sample_items": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, u32, vp, u32, f32, vp, vp, vp, vp, vp, i64, vp]),
    "p5_sample_truncated_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32, i32]),
    "p5_sample_items_truncated": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, u32, vp, u32, f32, i32, f32, vp, vp, vp, vp, vp, i64,
                                        vp]),
    "p5_sample_slates_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32, i32, i32]),
    "p5_sample_slates": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, u32, vp, u32, f32, vp, vp, vp, vp, vp, vp, i64, vp]),
    "p5_generate_history_count": (i64, [i32, i32, i32]),
    "p5_generate_draft": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
    "p5_verify_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32, i32, i32]),
    "p5_verify_begin": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, i64]),
    "p5_verify_encoder_output": (vp, [vp]),
    "p5_generate_set_encoder_output": (i32, [vp, vp]),
    "p5_verify_plan": (i32, [vp, vp, vp]),
    "p5_verify_plan_header": (vp, [vp]),
    "p5_verify_row_capacity": (i32, [i32, i32]),
    "p5_verify_encode": (i32, [vp, vp, vp, vp, vp]),
    "p5_verify_run": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    "p5_rank_workspace_bytes": (i64, [vp, i32, i32, i32, i64, i32, i32]),
    "p5_rank_items": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, i32, i32, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
    "p5_cand_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i32]),
    "p5_cand_plan": (i32, [vp, vp, i32, i32, vp, i32, i32, vp, i64, vp]),
    "p5_cand_score": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
    "p5_prune_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i64, i32, i32]),
    "p5_prune_propose": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, i32, f32, vp, vp, vp, vp, i64, vp, i64, vp]),
    "p5_prune_decide": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, i32, f32, vp, vp, vp, vp, i64, vp]),
    "p5_bound_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i64, i32, i32, i32, i32]),
    "p5_bound_begin": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, i64, vp]),
    "p5_bound_round": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, i32, i32, f32, vp, vp, vp, vp, i64, vp]),
    "p5_generate_timing": (i32, [vp, i32, C.POINTER(f32), C.POINTER(f32)]),
    "p5_decode_begin": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, i64, vp]),
    "p5_decode_step": (i32, [vp, vp]),
    "p5_decode_done_flag": (vp, [vp]),
    "p5_decode_finish": (i32, [vp, vp, vp, vp, vp]),
    "p5_encode": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, i64, vp]),
    "p5_op_gemm": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp, u32, f32, vp]),
    "p5_op_gemm_group": (i32, [i32, i32, i32, C.POINTER(P5GemmProblem), vp, u32, f32, vp]),
    "p5_op_rmsnorm_fwd": (i32, [i32, vp, vp, vp, vp, i32, i32, f32, vp]),
    "p5_op_rmsnorm_bwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]),
    "p5_op_attn_fwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, u32, f32, vp]),
    "p5_op_attn_bwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32,
                            i32, i32, i32, i32, vp, u32, f32, vp]),
    "p5_op_attn_bwd_dot": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32,
                                i32, i32, i32, i32, vp, u32, f32, vp, vp]),
    "p5_op_ce_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "p5_op_rmsnorm_fwd_drop": (i32, [i32, vp, vp, vp, vp, i32, i32, f32, vp, u32, f32, vp]),
    "p5_op_rmsnorm_bwd_full": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, u32, f32, u32, f32, vp, vp, f32, vp]),
    "p5_op_embed_fwd": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, vp, u32, f32, vp, vp]),
    "p5_op_embed_bwd": (i32, [i32, i32, i32, i32, C.POINTER(P5EmbedBwdSet), vp, vp]),
    "p5_op_ce_fwd_t": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, vp]),
    "p5_op_ce_bwd": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, f32, i32, vp, vp]),
    "p5_op_trie_walk": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "p5_op_trie_ce_fwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, vp]),
    "p5_op_trie_ce_bwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, vp, f32, vp]),
    "p5_op_trunc_cut": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, f32, i32, i32, i32, vp]),
    "p5_op_trunc_ce_fwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, f32, i32, i32, i32, vp]),
    "p5_op_trunc_ce_bwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, vp, f32, vp]),
    "p5_op_item_gather": (i32, [i32, vp, vp, vp, i32, i32, vp]),
    "p5_op_item_scatter": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "p5_op_trie_ce_fwd_cols": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, vp]),
    "p5_op_trie_ce_bwd_cols": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, vp, f32, vp]),
    "p5_op_trie_reg_fwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, vp]),
    "p5_op_trie_reg_bwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, i32, vp, f32,
                                 f32, f32, vp]),
    "p5_op_trunc_ce_fwd_cols": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, f32, i32, i32, i32, vp]),
    "p5_op_trunc_ce_bwd_cols": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, vp, f32, vp]),
    "p5_op_masked_mean": (i32, [vp, vp, vp, i32, i32, vp]),
    "p5_op_masked_mean_g": (i32, [i32, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]),
    "p5_policy_batch": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, i32, f32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "p5_policy_batch_clip": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, i32, f32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "p5_policy_slate_batch": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp]),
    "p5_op_pref_objective": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, f32, i32, i32, i32, vp]),
    "p5_op_clip_objective": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, f32, i32, i32, i32, i32, vp]),
    "p5_op_dec_cross_attn": (i32, [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "p5_op_skinny_gemm": (i32, [i32, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, f32, f32, vp]),
    "p5_op_dec_cross_attn_ex": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, f32, vp, vp]),
    "p5_op_dec_self_attn": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp]),
    "p5_op_rmsnorm_f32in": (i32, [i32, vp, vp, vp, i32, i32, f32, vp, vp]),
    "p5_op_head_lse": (i32, [i32, i32, vp, vp, vp, vp, i32, i32, i32, f32, vp, vp]),
    "p5_op_dec_score": (i32, [i32, i32, vp, vp, i32, vp, vp, i32, f32, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "p5_op_head_nv": (i32, [i32, i32]),
    "p5_op_rank_select": (i32, [i32, vp, vp, i64, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp]),
    "p5_op_rank_edges": (i32, [i32, i32, vp, i64, vp, vp, i32, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp]),
    "p5_op_cand_row_lse": (i32, [i32, i32, vp, vp, vp, i32, i32, vp, i32, i32, vp]),
    "p5_op_tree_attn": (i32, [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, vp]),
    "p5_op_cand_plan": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "p5_op_cand_rows": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, vp]),
    "p5_op_cand_score": (i32, [i32, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, i32, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp]),
    "p5_op_prune_fill": (i32, [vp, i64, f32, vp]),
    "p5_op_prune_propose": (i32, [vp, vp, vp, vp, i64, vp, i32, vp, vp, i32, i32, vp, vp, f32, i32, vp]),
    "p5_op_prune_mask": (i32, [vp, vp, vp, i64, vp, i32, i32, i32, vp]),
    "p5_op_prune_certify": (i32, [vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, f32, vp]),
    "p5_op_bound_seed": (i32, [vp, vp, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp]),
    "p5_op_bound_expand": (i32, [vp, vp, vp, vp, vp, i32, vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, f32, vp]),
    "p5_op_tr_probe": (i32, [vp, vp, vp]),
    "p5_profile_begin": (i32, []),
    "p5_profile_end": (i32, [C.c_char_p, i32]),
}


def bind(cdll):
    """Attach restype/argtypes for every symbol of include/p5hip.h; raises AttributeError if one is missing."""
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(cdll, name)
        fn.restype = res
        fn.argtypes = args
    return cdll


class P5Error(RuntimeError):
    pass


def check(lib, rc, what=""):
    if rc != 0:
        msg = lib.p5_last_error()
        raise P5Error(f"{what} failed: {msg.decode() if msg else rc}")
