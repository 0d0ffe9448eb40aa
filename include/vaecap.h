/* libvaecap C ABI -- MI355X (gfx950) kernels for the CVAE / AG-CVAE captioning trainer.
 *
 * The reference (yiyang92/vae_captioning) has NO native/FFI interface: its hot path is a
 * TensorFlow-1 static graph.  Each entry point below therefore names the reference GRAPH
 * CALL SITE (file:line under /root/reference) whose forward and/or tf.gradients-derived
 * backward it replaces; INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns 0 on success, else a
 *     hipError_t value or a VC_E* code (message: vc_last_error()).  No exceptions.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it.
 *   - All tensor pointers are DEVICE pointers owned by the caller; the library never
 *     allocates or frees caller-visible memory.  Scratch comes from caller workspaces.
 *   - fp32 everywhere (tf.float32 graph); token ids / lengths are int32.
 *   - Sequences are TIME-MAJOR [T, N, ...] (the reference feeds [N, T]; the transpose is
 *     host-side index plumbing).
 */
#ifndef VAECAP_H
#define VAECAP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (binders gate on vc_abi_version(); a mismatch is a LAYOUT break, not just a symbol break):
 *   4  precision and step-kernel choice are PER CALL: vc_gemm_f32 takes VC_GEMM_BF16X3 in `flags`; vc_lstm_seq_fwd_f32 / _bwd_f32 /
 *      _bwd_data_f32 / _bwd_weights_f32 gained a trailing `int flags` (VC_LSTM_BF16X3, VC_LSTM_KERNELS(k)): a v3 binder would pass one
 *      argument too few.  vc_gemm_set_precision / vc_lstm_set_mode remain as DEPRECATED process-wide defaults for calls that pass no
 *      choice of their own (the product path never calls them: two trainers of different precision coexist in one process).  Gone: the
 *      direct split-bf16 forward / data-gradient convolutions (vc_conv3x3_bx_* except the weight gradient, vc_conv3x3_bx2_*), which no
 *      product path called.  New: the F(4x4,3x3) convolution with a pre-transformed input (vc_conv3x3_wino4v_*), the decode-round
 *      entries vc_softmax_topk_rows_f32 / vc_beam_gather_f32 / vc_eos_track_i32 / vc_beam_init.
 *      Added within 4 (additive, no layout change): the diverse-captioning entries vc_diverse_latent_f32 / vc_decode_pick_f32 /
 *      vc_decode_round_end_i32 / vc_diverse_rank.
 *      Added within 4 (additive, no layout change): the consensus re-ranking entries vc_l2_normalize_rows_f32 / vc_topk_rows_wide_f32 /
 *      vc_topk_rows_wide_workspace_bytes / vc_ngram_vectors / vc_consensus_score.
 *      Added within 4 (additive, no layout change): the caption-scoring entries vc_logits_logprob_f32 /
 *      vc_logits_logprob_workspace_bytes / vc_score_reduce_f64.
 *      Added within 4 (additive, no layout change): the truncated-sampling entry vc_decode_pick_trunc_f32.
 *      Added within 4 (additive, no layout change): the caption-evaluation entry vc_ngram_overlap.
 *      Added within 4 (additive, no layout change): the posterior-bound entries vc_posterior_latent_f32 / vc_gauss_kl_rows_f64 /
 *      vc_bound_reduce_f64.
 *      Added within 4 (additive, no layout change): the marginal-decoding entries vc_mixture_topk_workspace_bytes / vc_mixture_topk_f32 /
 *      vc_mixture_advance_f32.
 *      Added within 4 (additive, no layout change): the constrained beam search entry vc_beam_update_constrained.
 *      Added within 4 (additive, no layout change): the decoding-controls entry vc_decode_controls_f32.
 *      Added within 4 (additive, no layout change): the stochastic beam search entries vc_sbs_init / vc_sbs_expand_f32 / vc_sbs_update.
 *      Added within 4 (additive, no layout change): the scheduled-sampling entry vc_sched_mix_f32.
 *      Added within 4 (additive, no layout change): the ROUGE-L entry vc_lcs_overlap.
 *      Added within 4 (additive, no layout change): the in-set CIDEr-D entry vc_cider_gram.
 *      Added within 4 (additive, no layout change): the mutual-information entry vc_gauss_mix_lse_f64.
 *      Added within 4 (additive, no layout change): the unlikelihood-training entries vc_softmax_xent_ul_f32, vc_ul_stats_f32.
 *      Added within 4 (additive, no layout change): the bag-of-words loss entries vc_bow_xent_f32, vc_bow_stats_f32.
 *      Added within 4 (additive, no layout change): the typical / min-p / eta sampling entry vc_decode_pick_typical_f32.
 *      Added within 4 (additive, no layout change): the contrastive-search entry vc_contrastive_pick_f32.
 *      Added within 4 (additive, no layout change): the DPP selection entry vc_dpp_select_f64.
 *   3  the 3x3-convolution family (vc_conv3x3_wino_*, vc_conv3x3_wino4_*, vc_conv3x3_wino_wgrad_*, vc_conv1_fwd* / vc_conv1_wgrad*,
 *      vc_maxpool2x2_bwd_bits_f32) takes and returns activations in the C4 layout [B][C/4][H][W][4] (v2: NHWC) and the pool routing
 *      codes / ReLU mask bits follow it; the vc_conv3x3_patch_*, vc_conv3x3_pack_f32, *_packed_f32 and wgrad_patch_* entries of v2 are
 *      gone.  A v2 binder would link and compute wrong numbers: it must refuse to run against a v3 library.  New in 3: the split-bf16
 *      products (vc_gemm_bf16x3_*), vc_vgg_preprocess_u8.
 *   2  round-3 surface (NHWC convolutions).  */
#define VC_ABI_VERSION 4
int vc_abi_version(void);
const char* vc_last_error(void);
/* 0 if a gfx950 device is usable from this process, else an error code. */
int vc_device_check(int device);
/* Tracing: named roctx ranges (`rocprofv3 --marker-trace --kernel-trace`); libroctx64 is bound at run time, without it push / pop are
 * no-ops.  trainer.Trainer brackets the phases of a step (VGG16 forward, caption forward / backward, VGG16 backward with its gradient
 * buckets, optimisers) when VC_TRACE=1. */
int vc_trace_available(void);
int vc_trace_push(const char* name);
int vc_trace_pop(void);

/* ------------------------------------------------------------------------------------
 * GEMM  C[M,N] = op(A)[M,K] . op(B)[K,N] (+ bias[N]) ; flags below.   fp32 MFMA.
 *   ta = 0: A stored [M,K] row-major (lda);  ta = 1: A stored [K,M] (computes A^T.B)
 *   tb = 0: B stored [K,N] row-major (ldb);  tb = 1: B stored [N,K] (computes A.B^T)
 * replaces tf.matmul / tf.layers.dense: main.py:94,108; vae_model/encoder.py:60-65,78-81,
 * 94-97; vae_model/decoder.py:111,127-129; utils/image_embeddings.py:223,234 and their
 * gradients (ops/optimizers.py:13,51).
 * Small outputs with long K are split along K into `ws` (vc_gemm_workspace_bytes) and
 * reduced in a fixed order (deterministic).
 * M == 0 or N == 0: nothing to do, returns 0.  K == 0 is the zero product (BLAS semantics): C = epilogue(0), i.e.
 * bias (or 0), + C with VC_GEMM_ACCUMULATE, ReLU'd with VC_GEMM_RELU; A and B are not read and may be NULL;
 * vc_gemm_workspace_bytes(M, N, 0) == 0.  Both precisions.
 * ---------------------------------------------------------------------------------- */
#define VC_GEMM_RELU 1
#define VC_GEMM_ACCUMULATE 2
#define VC_GEMM_BF16X3 4 /* this call on the bf16 matrix pipe with split operands (see vc_gemm_bf16x3_f32) */
size_t vc_gemm_workspace_bytes(int M, int N, int K);
int vc_gemm_f32(void* stream, int ta, int tb, int M, int N, int K, const float* A, long lda, const float* B,
                long ldb, float* C, long ldc, const float* bias, int flags, float* ws, size_t ws_bytes);
/* The same product on the bf16 matrix pipe ("bf16x3"): the f32 operands are split into (hi, lo) bf16 pairs while they are staged
 * into the LDS, three v_mfma_f32_32x32x16_bf16 products (hi.hi + hi.lo + lo.hi) accumulate in f32.  Same arguments, tile plan,
 * workspace and summation structure as vc_gemm_f32; |error| <= ~1e-5 of sum |a.b| (tests/test_gpu_bf16x3.py) instead of ~1e-7.
 * NOT the reference's arithmetic (tf.float32 matmul, main.py / vae_model/decoder.py:126-129): an opt-in mode, reported separately.
 * Per call: vc_gemm_f32 with VC_GEMM_BF16X3 in `flags` == this entry.  DEPRECATED: vc_gemm_set_precision(1) makes every vc_gemm_f32 /
 * vc_lstm_seq_* call of the process that carries no flag of its own take this path (0, the default = f32 MFMA); process-wide state,
 * not thread-safe, kept for ABI-3 callers only. */
int vc_gemm_bf16x3_f32(void* stream, int ta, int tb, int M, int N, int K, const float* A, long lda, const float* B,
                       long ldb, float* C, long ldc, const float* bias, int flags, float* ws, size_t ws_bytes);
int vc_gemm_set_precision(int mode);
int vc_gemm_get_precision(void);

/* ------------------------------------------------------------------------------------
 * Embedding lookup and its gradient.   tf.nn.embedding_lookup, vae_model/encoder.py:31-36,
 * vae_model/decoder.py:77-83 (pinned to /cpu:0 in the reference; on-device here).
 *   gather      out[r, :] = table[ids[r], :]
 *   scatter_add dtable[ids[r], :] += dX[r, :]      (IndexedSlices -> dense, TF-sem.)
 *   mark_rows   touched[ids[i]] = 1                 (rows a sparse Momentum update touches)
 * ---------------------------------------------------------------------------------- */
int vc_embedding_gather_f32(void* stream, const float* table, const int32_t* ids, long rows, int E, int vocab, float* out);
int vc_embedding_scatter_add_f32(void* stream, float* dtable, const int32_t* ids, long rows, int E, int vocab, const float* dX);
/* Deterministic form of scatter_add: out row v = sum of dX[order[j]] for j in seg_start[v] ..
 * seg_start[v+1] (nrows+1 entries), summed in that order; order = stable argsort of the ids (NULL =
 * identity).  Writes EVERY output row (zeros for empty segments), so repeated runs are
 * bit-identical.  Hot tokens are handled by calling it twice (sub-segments, then partial rows). */
int vc_embedding_grad_sorted_f32(void* stream, float* dtable, const int32_t* order, const int32_t* seg_start, int E,
                                 int nrows, const float* dX);
/* Inverted index of the token ids for the call pair above, built on device (stable counting sort, integer work, no
 * atomics): order [R] = stable argsort of clip(ids, 0, vocab-1); seg1 [max_subsegments + 1] = boundaries into `order` of
 * sub-segments of <= chunk positions that never cross an id boundary (entries past the real count are R: empty
 * sub-segments, so the first-level call may always run over max_subsegments rows -- no host read-back); seg2 [vocab + 1] =
 * for every id the range of its sub-segments.  ws: int32 scratch of vc_embedding_index_workspace_bytes. */
size_t vc_embedding_index_workspace_bytes(long R, int vocab);
size_t vc_embedding_index_max_subsegments(long R, int vocab, int chunk);
int vc_embedding_index_max_vocab(void); /* larger vocabularies: build the index on the host (engine.embedding_grad_index) */
int vc_embedding_grad_index(void* stream, const int32_t* ids, long R, int vocab, int chunk, int32_t* order, int32_t* seg1,
                            int32_t* seg2, int32_t* ws, size_t ws_bytes);
int vc_mark_rows_f32(void* stream, float* touched, const int32_t* ids, long n, int vocab);

/* ------------------------------------------------------------------------------------
 * LSTM.  utils/rnn_model.py:23-51 (make_rnn_cell), stepped at vae_model/encoder.py:46-55 and
 * vae_model/decoder.py:100-121.  W = [E+H, 4H] (rows 0..E-1 multiply x), gate order i,j,f,o,
 * forget_bias 1.0 (TF-sem.).  lens_eff[n]: step t of row n is active iff t < lens_eff[n]
 * (tf.nn.dynamic_rnn sequence_length semantics: state carried through when inactive).
 * H must be a multiple of 32.
 *   step_fwd: gact [N,4H] holds x.Wx+b on entry and the gate activations (i,j,f,o) on exit.
 *   step_bwd: one step of back-propagation through time (see lstm.hip for the recurrences).
 *   seq_fwd / seq_bwd: native loops over the T steps plus the batched input-projection and
 *   weight-gradient GEMMs.  cs / hs are [T+1,N,H] with index 0 = initial state.
 * ---------------------------------------------------------------------------------- */
int vc_lstm_step_fwd_f32(void* stream, int N, int H, int t, const float* h_prev, const float* c_prev, const float* Wh,
                         float* gact, const int32_t* lens_eff, float* c_out, float* h_out);
int vc_lstm_step_bwd_f32(void* stream, int N, int H, int t, int first, const float* dG_next, const float* Wh,
                         const int32_t* lens_eff, const float* dh_ext, float* dH_run, float* dC_run, const float* act,
                         const float* c_prev, const float* c_cur, float* dG);
/* Sequence drivers: `flags` of the vc_lstm_seq_* calls = VC_LSTM_KERNELS(k) | VC_LSTM_BF16X3.
 *   VC_LSTM_BF16X3   the call's products (input projection, recurrence, data / weight gradients) in the split-bf16 arithmetic of
 *                    vc_gemm_bf16x3_f32 (an opt-in mode, NOT the reference's tf.float32 LSTMCell)
 *   VC_LSTM_KERNELS(k), k = 0..3: which step kernels run (0 in the low bits = the default, auto); the numbering is vc_lstm_set_mode's.
 * vc_lstm_set_mode is the DEPRECATED process-wide default for calls whose flags choose nothing (identical arithmetic up to fp32 summation order and, in the
 * recurrence kernels, sigmoid / tanh built from v_exp_f32 + v_rcp_f32, |error| < 3e-7):
 * 2 (default) = auto: the register-operand recurrence step kernels (one workgroup per CU, four waves split K, Wh slice packed
 * in MFMA-operand order, 16x16x4 tiles, gate math in the epilogue; above 400 rows the forward uses eight waves on 16-unit slices)
 * when H == 512, otherwise 1; 1 = recurrent GEMM via vc_gemm_f32 (split-K) + element-wise gate kernels; 3 = recurrence kernels wherever
 * supported; 0 = the round-1 fused step kernels. */
#define VC_LSTM_BF16X3 0x10
#define VC_LSTM_KERNELS(k) ((k) + 1)
int vc_lstm_set_mode(int split);
/* Single steps on the recurrence kernel for callers that advance one token at a time with fixed weights (generation: greedy /
 * sampling / beam search, vae_model/decoder.py:145-320): pack Wh [H,4H] once into whp (2 * H * 4H floats: the operand orders of
 * both step kernels, chosen by N), then step with the same arguments as vc_lstm_step_fwd_f32.  H == 512 only: ask vc_lstm_step_packed_supported. */
int vc_lstm_step_packed_supported(int N, int H);
int vc_lstm_pack_wh_f32(void* stream, int H, const float* Wh, float* whp);
int vc_lstm_step_fwd_packed_f32(void* stream, int N, int H, int t, const float* h_prev, const float* c_prev, const float* whp,
                                float* gact, const int32_t* lens_eff, float* c_out, float* h_out);
size_t vc_lstm_seq_workspace_bytes(int T, int N, int E, int H);
int vc_lstm_seq_fwd_f32(void* stream, int T, int N, int E, int H, const float* X, const float* W, const float* b,
                        const int32_t* lens_eff, float* act, float* cs, float* hs, float* ws, size_t ws_bytes, int flags);
int vc_lstm_seq_bwd_f32(void* stream, int T, int N, int E, int H, const float* X, const float* W, const int32_t* lens_eff,
                        const float* act, const float* cs, const float* hs, const float* dhs_ext, float* dH_run,
                        float* dC_run, float* dG, float* dX, float* dW, float* db, float* ws, size_t ws_bytes, int flags);
/* The backward pass in two calls (vc_lstm_seq_bwd_f32 = the first followed by the second on one stream): the recurrence with
 * dX = dG.Wx^T, which is all the gradient chain below the LSTM waits for, and the weight gradients dWx = X^T.dG, dWh = hs[0:T]^T.dG,
 * db = colsum(dG) from the dG the first call left -- tf.gradients has no consumer for them before the optimiser
 * (ops/optimizers.py:13-16), so a caller may enqueue the second call on another stream with its own workspace. */
int vc_lstm_seq_bwd_data_f32(void* stream, int T, int N, int E, int H, const float* W, const int32_t* lens_eff, const float* act,
                             const float* cs, const float* dhs_ext, float* dH_run, float* dC_run, float* dG, float* dX, float* ws,
                             size_t ws_bytes, int flags);
int vc_lstm_seq_bwd_weights_f32(void* stream, int T, int N, int E, int H, const float* X, const float* hs, const float* dG, float* dW,
                                float* db, float* ws, size_t ws_bytes, int flags);

/* ------------------------------------------------------------------------------------
 * Masked sparse softmax cross-entropy, main.py:152-158.  In place: `logits` [rows, V] (ld)
 * is overwritten by d(loss)/d(logits) = (softmax - onehot) * (label != 0) * gscale / den[0]
 * when write_grad; row_loss[r] = (logsumexp - logit[label]) * (label != 0).
 * den is a DEVICE scalar (number of non-PAD labels, global over data-parallel ranks).
 * softmax_rows: gen-mode probabilities (vae_model/decoder.py:140,142).
 * ---------------------------------------------------------------------------------- */
int vc_softmax_xent_f32(void* stream, float* logits, const int32_t* labels, long rows, int V, long ld, const float* den,
                        float gscale, float* row_loss, int write_grad);
int vc_softmax_rows_f32(void* stream, const float* x, long rows, int V, long ld, float* y, long ldy);
int vc_argmax_rows_f32(void* stream, const float* x, long rows, int cols, long ld, int32_t* out);
/* The first k entries of each row under a STABLE descending sort (ties -> lower index first): the
 * candidate expansion of beam search, vae_model/decoder.py:273-276. */
int vc_topk_rows_f32(void* stream, const float* x, long rows, int cols, long ld, int k, float* out_val, int32_t* out_idx);
/* vc_softmax_rows_f32 followed by vc_topk_rows_f32 (k <= 8) in ONE read of the logits and no [rows, V] probability buffer: out_p / out_idx
 * [rows, k] equal the two-call sequence bit for bit (same expressions, same summation order, same tie rule).  One beam-search round,
 * vae_model/decoder.py:248-276. */
int vc_softmax_topk_rows_f32(void* stream, const float* logits, long rows, int V, long ld, int k, float* out_p, int32_t* out_idx);
int vc_fill_f32(void* stream, float* x, long n, float value);
/* tf.multinomial(logits / temperature, 1) (vae_model/decoder.py:137-138) by inverse CDF with injected
 * uniforms u[rows] in [0,1): out[r] = first index whose cumulative softmax exceeds u[r]. */
int vc_multinomial_rows_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature,
                            const float* u, int32_t* out);
/* Uniform [0,1) floats from the Philox stream (same counter convention as the other vc_philox_* calls). */
int vc_philox_uniform_f32(void* stream, float* out, long n, uint64_t seed, uint64_t offset, const int32_t* step);

/* ------------------------------------------------------------------------------------
 * Latent variable.  vae_model/encoder.py:59-109, main.py:118-145.
 *   latent_sample  z[s,n,l] = mean[n,l] + std[n,l]*eps[s,n,l]   (zs.Normal n_samples=S)
 *   kl_rows        mode 0: Normal/GMM KL per row (main.py:120-124,131-135); mode 1: AG
 *                  (main.py:140-145; mu_p = c_i.cluster_means [N,L])
 *   latent_bwd     dmean, dstd (or dlogstd = dstd*std when out_logstd) from dz [S,N,L] plus
 *                  ann[0]*kl_scale * dKL;  ann = device scalar (may be null = 1)
 *   heads_mix_*    GMM pick (idx != NULL, encoder.py:87-88) / AG mixture (c_i, :105-107) over
 *                  heads [N, 2*K*L] = [means | log-stds]
 * ---------------------------------------------------------------------------------- */
int vc_latent_sample_f32(void* stream, int S, int N, int L, const float* mean, const float* std_, const float* eps, float* z);
/* Data-parallel forms (the Q1 reshape mixes rows of the GLOBAL batch): this rank's z_rnn rows are the
 * flat range q in [q0, q0+nq) of the global [S, Ng, L] sample tensor, q = s*Ng + n; mean_g / std_g are the
 * all-gathered [Ng, L] statistics; sums_mixed returns the [Ng, L] partial sums to reduce-scatter.
 * vc_latent_bwd_f32 with S = 0 then adds the KL gradient to sums already stored in dmean / dstd. */
int vc_latent_sample_mixed_f32(void* stream, int Ng, int L, long q0, long nq, const float* mean_g, const float* std_g,
                               const float* eps, float* z);
int vc_latent_sums_mixed_f32(void* stream, int Ng, int L, long q0, long nq, const float* dz, const float* eps,
                             float* dmean_part, float* dstd_part);
int vc_kl_rows_f32(void* stream, int N, int L, int mode, const float* mean, const float* std_, const float* mu_p, float* row_kl);
int vc_latent_bwd_f32(void* stream, int S, int N, int L, int mode, int out_logstd, const float* dz, const float* eps,
                      const float* mean, const float* std_, const float* mu_p, const float* ann, float kl_scale,
                      float* dmean, float* dstd);
int vc_heads_mix_fwd_f32(void* stream, int N, int K, int L, const float* heads, const float* c_i, const int32_t* idx,
                         float* mean, float* std_);
int vc_heads_mix_bwd_f32(void* stream, int N, int K, int L, const float* heads, const float* c_i, const int32_t* idx,
                         const float* dmean, const float* dstd, float* dheads);
/* Step scalars, main.py:156-177: out4 = {rec_loss = ce_num/ce_den + reg_scale*reg_sumsq, mean KL =
 * kl_sum*inv_n, lower_bound = rec + ann*KL/10, ann}; every pointer is a device scalar (reg_sumsq,
 * kl_sum, ann may be NULL). */
int vc_loss_finalize_f32(void* stream, const float* ce_num, const float* ce_den, const float* reg_sumsq, float reg_scale,
                         const float* kl_sum, float inv_n, const float* ann, float* out4);

/* ------------------------------------------------------------------------------------
 * Training objective options (additive in ABI 4; DESIGN.md "Training objective options").  Each entry stands BESIDE its plain
 * form above and is called only when its option is on -- the plain entries and their kernels are unchanged.
 *   vc_softmax_xent_smooth_f32: label smoothing, target (1 - eps) * onehot + eps / V over the V real columns, eps in [0, 1):
 *     row_loss = mask * (lse - (1 - eps) * x[label] - (eps / V) * sum_{v<V} x[v]);  write_grad: logits[v] <- mask * (gscale / den) *
 *     (softmax[v] - (1 - eps) * [v == label] - eps / V) for v < V and exactly 0 for the pitch padding V <= v < ld (all of it).
 *     Same two kernels and dispatch rule as vc_softmax_xent_f32.
 *   vc_kl_rows_fb_f32: free bits, row_kl[n] = sum_l max(free_bits, kl[n,l]) with kl[n,l] the per-dimension summand of
 *     vc_kl_rows_f32 (its -0.5 included); row_kl_raw[n] = sum_l kl[n,l]; row_floored[n] = #{l: kl[n,l] <= free_bits}.
 *   vc_latent_bwd_fb_f32: vc_latent_bwd_f32 whose KL gradient is exactly 0 for the dimensions with kl[n,l] <= free_bits (the
 *     same f32 value and comparison as the forward entry's).
 *   vc_objective_stats_f32: out2 = {mean_n row_kl_raw, sum_n row_floored / (N * L)}.
 *   vc_loss_finalize_kl_f32: vc_loss_finalize_f32 with lower_bound = rec + ann * kl_coef * KL (kl_coef = beta / 10).
 * ---------------------------------------------------------------------------------- */
int vc_softmax_xent_smooth_f32(void* stream, float* logits, const int32_t* labels, long rows, int V, long ld, const float* den,
                               float gscale, float eps, float* row_loss, int write_grad);
int vc_kl_rows_fb_f32(void* stream, int N, int L, int mode, const float* mean, const float* std_, const float* mu_p,
                      float free_bits, float* row_kl, float* row_kl_raw, int32_t* row_floored);
int vc_latent_bwd_fb_f32(void* stream, int S, int N, int L, int mode, int out_logstd, const float* dz, const float* eps,
                         const float* mean, const float* std_, const float* mu_p, const float* ann, float kl_scale,
                         float free_bits, float* dmean, float* dstd);
int vc_objective_stats_f32(void* stream, int N, int L, const float* row_kl_raw, const int32_t* row_floored, float* out2);
int vc_loss_finalize_kl_f32(void* stream, const float* ce_num, const float* ce_den, const float* reg_sumsq, float reg_scale,
                            const float* kl_sum, float inv_n, const float* ann, float kl_coef, float* out4);

/* ------------------------------------------------------------------------------------
 * Self-critical training (additive in ABI 4; DESIGN.md "Self-critical training"): the policy-gradient loss of sampled captions.
 * Rows are time-major [T, N] (rows % N == 0): row r belongs to caption n = r % N with advantage adv[n] (device, [N]).  A row is
 * live when 0 < label < V.  With p = softmax(x) over the V real columns, lse = log sum exp x and H = lse - sum_v p_v x_v:
 *   row_lp[r]  = live ? x[label] - lse : 0                (log-probability of the token taken)
 *   row_ent[r] = live ? H : 0                              (beta > 0 only; may be NULL with beta == 0)
 *   write_grad: logits[r, v] <- live * scale * (adv[n] * (p_v - [v == label]) + beta * p_v * ((x_v - lse) + H)) for v < V and
 *   exactly 0 for the pitch padding V <= v < ld: the gradient of J = scale * sum_live (-adv[n] * log p(label) - beta * H).
 * H is computed from x (never as log p_v): an underflowed p_v contributes exactly 0.  Same two kernels and dispatch rule as
 * vc_softmax_xent_f32; beta == 0 runs them without the entropy arithmetic.
 * ---------------------------------------------------------------------------------- */
int vc_softmax_xent_policy_f32(void* stream, float* logits, const int32_t* labels, long rows, int V, long ld,
                               const float* adv, int N, float scale, float beta,
                               float* row_lp, float* row_ent, int write_grad);

/* ------------------------------------------------------------------------------------
 * Unlikelihood training (additive in ABI 4; csrc/loss.hip; DESIGN.md "Unlikelihood training"): vc_softmax_xent_smooth_f32 with the
 * token-level repetition penalty of Welleck et al. (2020) in the same pass over the row.  Rows are time-major [T, N] (rows % N == 0,
 * r = t * N + n, the layout of vc_softmax_xent_policy_f32); y = labels[r]; a row is live when 0 < y < V.
 *   candidates  C_r = the distinct values of labels[t' * N + n], max(0, t - window) <= t' < t, without values <= 0, values >= V and y
 *               itself; gathered by the kernel from `labels`.  t = 0 has none.
 *   terms       p = softmax(x) over the V real columns; om_c = 1 - p_c; a candidate with om_c <= 1e-5 is clamped: it adds -log(1e-5) to
 *               row_ul and nothing to the gradient (torch.clamp's autograd); otherwise r_c = p_c / om_c.  R = sum of r_c, unclamped c.
 *   row_loss[r] = what vc_softmax_xent_smooth_f32 writes (cross-entropy alone, smoothed by eps; eps = 0: the plain loss)
 *   row_ul[r]   = live * sum_c -log(max(om_c, 1e-5));  row_cand[r] = live * |C_r|;  row_mass[r] = live * sum_c p_c
 *   write_grad  logits[r, v] <- k * (p_v - (1 - eps) [v == y] - eps / V + alpha * (r_v [v in C_r, unclamped] - p_v * R)) for v < V,
 *               k = live * gscale / den[0], and exactly 0 for the pitch padding V <= v < ld; a row that is not live comes back all-zero.
 *               write_grad = 0 leaves the logits untouched.
 * Same dispatch rule as vc_softmax_xent_f32 (register kernel / generic kernel); per row at most 128 label reads, 128 scattered 4-byte
 * reads and 128 scattered 4-byte writes on top of the smoothed entry's traffic.  VC_EINVAL before any launch: window outside 1..128,
 * alpha not finite or <= 0, N < 1 or rows % N != 0, a null row_ul / row_cand / row_mass, and everything the smoothed entry rejects.
 *   vc_ul_stats_f32: out3 = {sum row_ul, sum row_cand, sum row_mass} / #{r: 0 < labels[r] < V}, sums in fixed order (zeros when no row
 *   is live): the unlikelihood loss per live row, the mean candidate count and the mean probability on already-said words.
 * ---------------------------------------------------------------------------------- */
int vc_softmax_xent_ul_f32(void* stream, float* logits, const int32_t* labels, long rows, int N, int V, long ld, const float* den,
                           float gscale, float eps, float alpha, int window, float* row_loss, float* row_ul, int32_t* row_cand,
                           float* row_mass, int write_grad);
int vc_ul_stats_f32(void* stream, long rows, int V, const int32_t* labels, const float* row_ul, const int32_t* row_cand,
                    const float* row_mass, float* out3);

/* ------------------------------------------------------------------------------------
 * Bag-of-words auxiliary loss (additive in ABI 4; csrc/loss.hip; DESIGN.md "Bag-of-words loss"; Zhao, Zhao & Eskenazi 2017): the
 * multi-label member of the logits-row family.  One row of logits per CAPTION (rows = N, pitch ld), one workgroup per row; labels is the
 * step's time-major [T, N] label buffer, ldl the stride between positions (N in the engine): position t of caption n is
 * labels[t * ldl + n].
 *   bag         of row n = the multiset { labels[t * ldl + n] : 0 <= t < T, 0 < label < V } (PAD and out-of-range ids are not in it);
 *               m = its size with multiplicity, c_w = the count of word w in it; p = softmax(x) over the V real columns
 *   row_loss[n] = m * lse(x) - sum_w c_w x_w       (= -sum over the bag of log p_w)
 *   row_mass[n] = sum over the DISTINCT bag words of p_w;  row_words[n] = the number of distinct bag words
 *   write_grad  logits[n, v] <- k * (m * p_v - c_v) for v < V, k = gscale / den[0], and exactly 0 for the pitch padding V <= v < ld;
 *               a row with m = 0 has loss 0, mass 0, words 0 and comes back all-zero.  write_grad = 0 leaves the logits untouched.
 * Same dispatch rule as vc_softmax_xent_f32 (register kernel / generic kernel); per row at most T label reads, T scattered 4-byte reads
 * and T scattered 4-byte writes on top of one read and one write of the row.  VC_EINVAL before any launch: T outside 1..256 (one
 * position per thread), ldl < rows, V < 1, ld < V, rows < 0, a null logits / labels / row_loss / row_mass / row_words, a null den with
 * write_grad.  rows = 0 is a successful no-op.
 *   vc_bow_stats_f32: out3 = {sum row_loss / sum m, sum row_words / #non-empty rows, sum row_mass / #non-empty rows} (zeros when every
 *   bag is empty), sums in fixed order, m counted from the labels as above: nats per bag word, mean distinct words and mean probability
 *   on the bag per non-empty caption.  One workgroup.
 * ---------------------------------------------------------------------------------- */
int vc_bow_xent_f32(void* stream, float* logits, long rows, int V, long ld, const int32_t* labels, int T, long ldl, const float* den,
                    float gscale, float* row_loss, float* row_mass, int32_t* row_words, int write_grad);
int vc_bow_stats_f32(void* stream, long rows, int V, const int32_t* labels, int T, long ldl, const float* row_loss,
                     const float* row_mass, const int32_t* row_words, float* out3);

/* ------------------------------------------------------------------------------------
 * Scheduled sampling, parallel form (additive in ABI 4; csrc/sched.hip; DESIGN.md "Scheduled sampling"): the mix between the two
 * decoder passes of a training step.  logits [T*N, V] (row pitch ld) are the teacher-forced pass's, time-major, so the model's
 * prediction for decoder input position (t, n) is row (t-1)*N + n.  cap_dec_t [T, N]: the gold decoder inputs; lens [N]: the caption
 * lengths as the batch carries them (labels per row -- not the LSTM lengths with the init steps).
 *   eligible  position (t, n) iff 1 <= t < lens[n]: <BOS>, PAD positions and rows of length 0 never are.
 *   selected  an eligible position iff coin[t, n] < rate (strict).  Every other position: dec_mix_t = cap_dec_t.
 *   the word  of a selected position: with u, the inverse-CDF draw of softmax(x / temperature) over the columns [0, V) with u[t, n]
 *             -- the token vc_multinomial_rows_f32 returns for that row and that uniform, bit for bit; with u == NULL the first
 *             maximum, as vc_argmax_rows_f32 returns it.  The eligibility and coin tests come before any read of the row: an
 *             unselected position touches no logits memory, a selected row is read from memory once (V <= 36864; wider rows are
 *             read in place).
 *   the rate  from the DEVICE step counter, s = max(step[0] - 1, 0) (the counter vc_step_update has already incremented: the
 *             first step of a run has s = 0).  schedule 0: rate_max.  1 (linear): rate_max * min(1, s / ramp_steps).
 *             2 (inverse sigmoid, Bengio et al. 2015 eq. 3 as a sampling rate): rate_max * (1 - k / (k + exp(s / k))), k = ramp_steps,
 *             evaluated as rate_max / (1 + k * exp(-s / k)).
 *   outputs   dec_mix_t [T, N]: EVERY element is written.  stats (may be NULL): stats[0] += eligible, stats[1] += selected
 *             positions (one thread's plain adds, in stream order).  rate_out (may be NULL): the rate of this call.
 * VC_EINVAL, nothing written: V < 1, ld < V, T < 1, N < 1; temperature <= 0 with u; rate_max outside [0, 1]; an unknown schedule;
 * ramp_steps <= 0 with schedule 1 or 2; a NULL logits / cap_dec_t / lens / coin / step / dec_mix_t.  T == 1 is valid (a copy).
 * ---------------------------------------------------------------------------------- */
int vc_sched_mix_f32(void* stream, const float* logits, long ld, int V, int T, int N, const int32_t* cap_dec_t, const int32_t* lens,
                     const float* coin, const float* u, float temperature, const int32_t* step, int schedule, float rate_max,
                     int ramp_steps, int32_t* dec_mix_t, int32_t* stats, float* rate_out);

/* ------------------------------------------------------------------------------------
 * Small data-movement ops.
 *   colsum       out[c] (+)= sum_r x[r,c]                (bias gradients)
 *   dropout      y = x*mask/keep                          (tf.nn.dropout, decoder.py:85-87, rnn_model.py:45-46)
 *   relu_bwd     dx = dy*(y>0) [*mask/keep]               (ReluGrad [+ dropout grad], image_embeddings.py:224-237)
 *   tile_rows    y[i*nc+j,:] = x[i,:]                     (main.py:84-89);  segment_sum_rows = its gradient
 * ---------------------------------------------------------------------------------- */
size_t vc_colsum_workspace_bytes(long rows, int cols);
int vc_colsum_f32(void* stream, const float* x, long rows, int cols, long ld, float* out, int accumulate, float* ws, size_t ws_bytes);
int vc_dropout_f32(void* stream, const float* x, const float* mask, float keep, long n, float* y);
int vc_relu_bwd_f32(void* stream, const float* dy, const float* y, const float* mask, float keep, long n, float* dx);
int vc_tile_rows_f32(void* stream, const float* x, long B, int nc, int E, float* y);
int vc_segment_sum_rows_f32(void* stream, const float* y, long B, int nc, int E, float* x, int accumulate);
int vc_exp_f32(void* stream, const float* x, long n, float* y);
int vc_axpy_f32(void* stream, float a, const float* x, long n, float* y);
/* a <-> b in place over n floats (16-byte aligned, not overlapping; n == 0 returns 0). */
int vc_swap_f32(void* stream, float* a, float* b, long n);
int vc_reduce_sum_f32(void* stream, const float* x, long n, float scale, float* out, int accumulate);
int vc_count_nonzero_i32(void* stream, const int32_t* x, long n, float* out);

/* ------------------------------------------------------------------------------------
 * Optimisers, ops/optimizers.py.
 *   sumsq_partial + clip_finalize = tf.clip_by_global_norm (:15-16): partial must hold
 *     vc_sumsq_blocks() floats per call; finalize sums n_partial of them in a fixed order and
 *     writes out[0] = global norm, out[1] = clip * min(1/norm, 1/clip).
 *   step_update: device-resident global_step, Adam lr_t, annealing coefficient
 *     (main.py:163-170), staircase lr decay (:24-31).  scalars[0..4], see optim.hip.
 *   adam / sgd / momentum: apply_gradients (:33-46, :68-81) over flat buffers; lr, scale are
 *     DEVICE scalars (scale may be NULL = 1); l2 adds l2*p to the gradient (main.py:69-74).
 * ---------------------------------------------------------------------------------- */
int vc_sumsq_blocks(void);
int vc_sumsq_partial_f32(void* stream, const float* x, long n, float* partial);
int vc_clip_finalize_f32(void* stream, const float* partial, int n_partial, float clip, float* out_norm_scale);
int vc_step_update(void* stream, int32_t* step, float* scalars, float lr, float cnn_lr, float beta1, float beta2,
                   float ann_param, int ann_on, int decay_steps);
/* vc_step_update with the cyclical KL schedule (additive in ABI 4) in scalars[1] instead of the tanh one:
 * min(1, (step mod cycle_steps) / (cycle_ramp * cycle_steps)) while step < cycles * cycle_steps or cycles == 0, 1 afterwards
 * (step = the counter before the increment); every other scalar and the counter as vc_step_update leaves them. */
int vc_step_update_cyclical(void* stream, int32_t* step, float* scalars, float lr, float cnn_lr, float beta1, float beta2,
                            int decay_steps, int cycle_steps, float cycle_ramp, int cycles);
int vc_adam_f32(void* stream, float* p, const float* g, float* m, float* v, long n, const float* lr_t, const float* scale,
                float beta1, float beta2, float eps, float l2);
/* The same update that also leaves sum(p_new^2) per workgroup in sumsq_partial[0 .. vc_adam_blocks(n)) (summed by vc_reduce_sum_f32):
 * the L2 regulariser's loss term of the NEXT step (main.py:69-74) without another pass over the 134 M VGG16 parameters. */
int vc_adam_blocks(long n);
int vc_adam_sumsq_f32(void* stream, float* p, const float* g, float* m, float* v, long n, const float* lr_t, const float* scale,
                      float beta1, float beta2, float eps, float l2, float* sumsq_partial);
/* Weight averaging (DESIGN.md "Weight averaging"): ema += w * (p_new - ema), w = max(omd, 9 / (10 + step[0])) -- the num_updates warm-up
 * of tf.train.ExponentialMovingAverage, step[0] = the device counter behind vc_step_update = updates including this one -- or w = omd
 * with step NULL.  omd = 1 - decay in (0, 1], computed by the caller in double.  vc_adam_ema_f32 / vc_adam_sumsq_ema_f32: the Adam
 * entries above with the average folded into the same pass (p, m, v and the sums equal theirs bit for bit; 36 B per parameter instead
 * of 28 + 12).  vc_ema_update_f32: the average alone, behind any other update; the same bits as the fused form.  Buffers 16-byte
 * aligned; ema must not overlap p, m or v; n == 0 returns 0 (the sumsq form needs n > 0 like vc_adam_sumsq_f32). */
int vc_adam_ema_f32(void* stream, float* p, const float* g, float* m, float* v, float* ema, long n, const float* lr_t, const float* scale,
                    float beta1, float beta2, float eps, float l2, float omd, const int32_t* step);
int vc_adam_sumsq_ema_f32(void* stream, float* p, const float* g, float* m, float* v, float* ema, long n, const float* lr_t, const float* scale,
                          float beta1, float beta2, float eps, float l2, float omd, const int32_t* step, float* sumsq_partial);
int vc_ema_update_f32(void* stream, float* ema, const float* p, long n, float omd, const int32_t* step);
int vc_sgd_f32(void* stream, float* p, const float* g, long n, const float* lr, const float* scale, float l2);
int vc_momentum_f32(void* stream, float* p, const float* g, float* accum, long n, const float* lr, const float* scale,
                    float momentum, float l2, const float* row_mask, int E);

/* ------------------------------------------------------------------------------------
 * Philox4x32-10 counter-based RNG (replaces TF's random_normal / dropout streams; the
 * streams cannot match TF's, parity tests inject noise instead).  Element i comes from
 * counter (i/4, offset) word i%4 under key (seed lo, seed hi + step); `step` (device int, may be
 * NULL) lives in the KEY so that graph replays draw fresh numbers and stream ids kept in
 * offset >> 32 never alias across steps.
 * ---------------------------------------------------------------------------------- */
int vc_philox_u32(void* stream, uint32_t* out, long n, uint64_t seed, uint64_t offset, const int32_t* step);
int vc_philox_normal_f32(void* stream, float* out, long n, uint64_t seed, uint64_t offset, const int32_t* step);
int vc_philox_bernoulli_f32(void* stream, float* out, long n, float keep, uint64_t seed, uint64_t offset, const int32_t* step);

/* ------------------------------------------------------------------------------------
 * VGG16 feature extractor, utils/image_embeddings.py:26-238.  NHWC activations, HWIO kernels,
 * channel counts powers of two >= 4 (conv1_1: RGB zero-padded to 4 channels).
 *   conv3x3_fwd    y = [relu](conv2d(x, w, stride 1, SAME) + bias)        (:40-44 ...)
 *   conv3x3_dgrad  dx = conv2d_backprop_input(dy, w) [* (relu_src > 0)]
 *   conv3x3_wgrad  dw (+)= conv2d_backprop_filter(x, dy)   (split-K, deterministic reduce); db != NULL also
 *                  returns the bias gradient db (+)= sum_pixels dy, summed from the dy tiles already staged in LDS
 *   maxpool2x2     tf.nn.max_pool 2x2/2 (:59-63 ...); bwd optionally fused with ReluGrad of x
 *   vgg_preprocess images [B,H,W,3] (0..255 RGB) - mean -> NHWC4            (:31-34)
 *   pad_dim        dst[o][c][i] = c < c_src ? src[o][c][i] : 0  (pad / strip a middle dim)
 * ---------------------------------------------------------------------------------- */
/* fwd / dgrad workspace (optional; NULL or too small -> single launch): lets the library run the last partial round of
 * tiles as a K-split second launch instead of a ragged round (csrc/conv.hip, launch_rounds); 0 when not needed. */
size_t vc_conv3x3_fwd_workspace_bytes(int B, int H, int W, int Cin, int Cout);
size_t vc_conv3x3_dgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int vc_conv3x3_fwd_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* w,
                       const float* bias, float* y, int relu, float* ws, size_t ws_bytes);
int vc_conv3x3_dgrad_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* dy, const float* w,
                         const float* relu_src, float* dx, float* ws, size_t ws_bytes);
size_t vc_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int vc_conv3x3_wgrad_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* dy, float* dw,
                         float* db, int accumulate, float* ws, size_t ws_bytes);
int vc_maxpool2x2_fwd_f32(void* stream, int B, int H, int W, int C, const float* x, float* y);
int vc_maxpool2x2_bwd_f32(void* stream, int B, int H, int W, int C, const float* x, const float* dy, float* dx, int relu_grad);
int vc_vgg_preprocess_f32(void* stream, const float* images, int B, int H, int W, float* out_nhwc4);
/* The same from uint8 RGB pixels [B,H,W,3] -- what the reference's HDF5 file holds (preprocess.py:27-28) and feeds (utils/image_utils.py:8;
 * the placeholder's float32 cast, utils/image_embeddings.py:31-34, is this kernel): a quarter of the host -> device bytes of the
 * float form (9.6 MB instead of 38.5 MB per 64 images), bit-identical output.  B*H*W % 4 == 0. */
int vc_vgg_preprocess_u8(void* stream, const void* images_u8, int B, int H, int W, float* out_nhwc4);
int vc_pad_dim_f32(void* stream, const float* src, long outer, int c_src, int c_dst, int inner, float* dst);

/* THE C4 ACTIVATION LAYOUT.  Every Winograd entry below (vc_conv3x3_wino_*, vc_conv3x3_wino4_*, vc_conv3x3_wino_wgrad_*) and conv1_1's
 * output / output gradient take their activation tensors channel-blocked: [B][C/4][H][W][4] -- per image C/4 planes, a plane = H x W
 * pixels, a pixel = 16 bytes = four consecutive channels (element (b, y, x, c) at float index (((b * C/4 + c/4) * H + y) * W + x) * 4 + c%4).
 * Why: the kernels gather 16-byte pieces (a pixel's four channels of one Winograd phase) for the pixels of a halo patch; in NHWC the
 * pixels of a patch row are 4 C bytes apart, one wave load touches 64 cache lines and the L1's tag rate bounds the kernel (measured:
 * HISTORY.md section 4g); in C4 a patch row is 288 consecutive bytes.  Images stay contiguous (image ranges, data-parallel shards and the
 * > 2 GiB cuts are slices of the leading dimension as before); C = 4 (conv1_1's zero-padded RGB input) is the same memory in both
 * layouts.  The reference's NHWC order (utils/image_embeddings.py:222: pool5 flattened as (h, w, c)) is restored at the fc1 boundary.
 * vc_maxpool2x2_fwd_f32 / vc_maxpool2x2_bwd_f32 work on C4 tensors when called with (B * C/4, H, W, 4). */
int vc_nhwc_to_c4_f32(void* stream, int B, int H, int W, int C, const float* nhwc, float* c4);
int vc_c4_to_nhwc_f32(void* stream, int B, int H, int W, int C, const float* c4, float* nhwc);

/* Winograd F(2x2, 3x3) forward / data gradient (csrc/conv_wino.hip): the same convolution in fp32 with 2.25x fewer multiplications.
 * Input transform, sixteen position products on MFMA (16x16x4 tiles) and output transform in one kernel; a wave owns up to 16 tiles
 * (2x2 output pixels each) x 32 output columns x all sixteen positions, two workgroups share a CU.  The weights are transformed and packed once per optimiser step
 * (wp: 16 * Cin * Cout floats; transpose 0 = forward, 1 = flipped taps + transposed channels for the data gradient).  Results agree
 * with conv3x3_fwd / conv3x3_dgrad to fp32 rounding of a different summation (tests/test_gpu_conv_wino.py: same fp64 oracle, same
 * tolerance class).  x, y, ypool, dy, dx, relu_src: C4 layout.  ypool != NULL also writes max_pool2x2(y) (a pooling window is one Winograd tile).  Shapes: H, W even, gathered
 * channels % 16 == 0, output channels % 32 == 0; ask vc_conv3x3_wino_supported. */
int vc_conv3x3_wino_supported(int B, int H, int W, int Cin, int Cout, int dgrad);
/* The kernels address a launch's tensors with 32-bit offsets: calls on more than 2 GiB per tensor are cut into launches over image
 * ranges inside the library; 1 if [B,H,W,max(Cin,Cout)] floats fit one launch (the mask-bit variants below require it). */
int vc_conv3x3_wino_single_launch_supported(int B, int H, int W, int Cin, int Cout);
int vc_conv3x3_wino_pack_f32(void* stream, int Cin, int Cout, const float* w, int transpose, float* wp);
int vc_conv3x3_wino_fwd_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                            const float* bias, float* y, float* ypool, int relu);
int vc_conv3x3_wino_dgrad_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* dy, const float* wpt,
                              const float* relu_src, float* dx);

/* MaxPoolGrad routing codes: a pooled forward (bias + ReLU applied) can also leave, per pooled element, four bits = the position of the
 * first maximum of its 2x2 window (row-major) | 4 if that maximum is > 0 -- vc_conv3x3_wino_pool_words(B, H, W, Cout) 32-bit words; a
 * 16-bit half-word = the four channels of one pooled pixel of one channel quad, layout [B][Cout/4][H/2][W/2] half-words --, and
 * vc_maxpool2x2_bwd_bits_f32 (dy, dx in the C4 layout) routes the pooled gradient with them: bit-identical to vc_maxpool2x2_bwd_f32(x = y,
 * dy, dx, relu_grad = 1) on the same planes without re-reading the pre-pool activation (H, W = the PRE-pool size in both calls). */
size_t vc_conv3x3_wino_pool_words(int B, int H, int W, int C);
int vc_conv3x3_wino_fwd_pool_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                                 const float* bias, float* y, float* ypool, uint32_t* pool_bits);
int vc_maxpool2x2_bwd_bits_f32(void* stream, int B, int H, int W, int C, const uint32_t* pool_bits, const float* dy, float* dx);

/* ReLU mask as bits: the forward of a layer can leave (y > 0) of every lane's 2x2 pixels x 8 columns as 32 bits (vc_conv3x3_wino_mask_words
 * (B, H, W, Cout) 32-bit words), and the data gradient of the NEXT 3x3 layer -- whose output has the same shape, hence the
 * same tiles and lanes -- reads those bits (one 4-byte load per lane) instead of relu_src (eight 16-byte loads + packing per lane:
 * 6-17 % of a data-gradient call).  Results are bit-identical to vc_conv3x3_wino_dgrad_f32 with relu_src = that y. */
size_t vc_conv3x3_wino_mask_words(int B, int H, int W, int C);
int vc_conv3x3_wino_fwd_mask_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                                 const float* bias, float* y, int relu, uint32_t* mask_out);
int vc_conv3x3_wino_dgrad_bits_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* dy, const float* wpt,
                                   const uint32_t* mask_bits, float* dx);

/* Winograd F(4x4,3x3) (csrc/conv_wino4.hip): the same convolution with 36 positions per 4 x 4 output tile -- 2.25 multiplications per
 * output where F(2x2,3x3) spends 4 -- for layers whose gathered channels are a multiple of 8 and produced channels a multiple of 32.
 * Every entry mirrors its vc_conv3x3_wino_* namesake argument for argument (same tensors, same routing-code format of the pooled
 * forward); what differs: the packed weights (36 * Cin * Cout floats, vc_conv3x3_wino4_pack_f32), the ReLU mask bits (64 per lane,
 * vc_conv3x3_wino4_mask_words words; bits written by this family's forward are read by this family's data gradient only), the
 * rounding (~1e-5 of the tensor maximum against ~1e-6).  vc_conv3x3_wino4_preferred: 1 where this kernel is the faster of the two
 * Winograd forms (the 224-, 112-, 28- and 14-wide layers of VGG16; the callers keep one family per block of layers between two
 * pools, since the mask bits pass from a layer's forward to the next layer's data gradient). */
int vc_conv3x3_wino4_supported(int B, int H, int W, int Cin, int Cout, int dgrad);
int vc_conv3x3_wino4_preferred(int B, int H, int W, int Cin, int Cout);
int vc_conv3x3_wino4_pack_f32(void* stream, int Cin, int Cout, const float* w, int transpose, float* wp);
int vc_conv3x3_wino4_fwd_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp, const float* bias,
                             float* y, float* ypool, int relu);
/* y == NULL (this entry, vc_conv3x3_wino4_fwd_f32 with ypool != NULL, and their vc_conv3x3_wino4v_* namesakes): the caller wants only
 * the pooled tensor (and, here, the routing codes).  The kernel then has no full-size output path at all -- no hand-over through the
 * LDS, no barrier in front of it, no stores -- and ypool / pool_bits are BIT-IDENTICAL to what the same call with a real y leaves (a
 * training step reads nothing else of a pooled layer: the next layer and its weight gradient read ypool, MaxPoolGrad + ReluGrad the
 * codes).  ypool (and pool_bits here) stay required; y == NULL without ypool is VC_EINVAL and launches nothing.  Calls over more
 * images than one launch addresses are cut into image ranges as before. */
int vc_conv3x3_wino4_fwd_pool_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                                  const float* bias, float* y, float* ypool, uint32_t* pool_bits);
size_t vc_conv3x3_wino4_mask_words(int B, int H, int W, int C);
int vc_conv3x3_wino4_fwd_mask_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp,
                                  const float* bias, float* y, int relu, uint32_t* mask_out);
int vc_conv3x3_wino4_dgrad_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* dy, const float* wpt,
                               const float* relu_src, float* dx);
int vc_conv3x3_wino4_dgrad_bits_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* dy, const float* wpt,
                                    const uint32_t* mask_bits, float* dx);
/* The F(4x4, 3x3) forward / data gradient with the input transformed ONCE per layer and pass (csrc/conv_wino4.hip, MODE 2): a first
 * kernel writes V = B^T d B of every (4 x 4 tile, gathered channel) into the workspace `vws` in the B-operand order of the MFMAs
 * (2.25 x the activation's bytes, HBM-bound), the main kernel then streams its B operands from V straight into registers -- no patch
 * staging, no patch LDS traffic and no transform arithmetic beside the MFMAs, where the fused kernel re-transforms every patch for
 * every 32-output-channel tile (16 x on the 512-channel layers).  Same packed weights (vc_conv3x3_wino4_pack_f32), same arithmetic in
 * the same order -- outputs, ReLU mask bits, pooled outputs and routing codes are BIT-IDENTICAL to the vc_conv3x3_wino4_* entry of the
 * same name, argument for argument + (vws, vws_bytes).  Shapes: those of vc_conv3x3_wino4_* whose launch puts the same tile in the same
 * lane (the linear-tile layers -- VGG16's 56- and 28-wide -- and 13..16 x 13..16 images), one launch (< 2 GiB): ask
 * vc_conv3x3_wino4v_supported.  vc_conv3x3_wino4v_workspace_bytes(B, H, W, C): C = the GATHERED channels (Cin forward, Cout data
 * gradient).  utils/image_embeddings.py:96-212 (conv3_1 .. conv5_3) and tf.gradients of them. */
int vc_conv3x3_wino4v_supported(int B, int H, int W, int Cin, int Cout, int dgrad);
int vc_conv3x3_wino4v_preferred(int B, int H, int W, int Cin, int Cout, int dgrad); /* 1: faster than the fused form for this launch (measured rule) */
size_t vc_conv3x3_wino4v_workspace_bytes(int B, int H, int W, int C);
int vc_conv3x3_wino4v_fwd_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp, const float* bias,
                              float* y, float* ypool, int relu, float* vws, size_t vws_bytes);
/* y == NULL: the pooled tensor and the routing codes only, as for vc_conv3x3_wino4_fwd_pool_f32 above (same contract, same bits). */
int vc_conv3x3_wino4v_fwd_pool_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp, const float* bias,
                                   float* y, float* ypool, uint32_t* pool_bits, float* vws, size_t vws_bytes);
int vc_conv3x3_wino4v_fwd_mask_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* wp, const float* bias,
                                   float* y, int relu, uint32_t* mask_out, float* vws, size_t vws_bytes);
int vc_conv3x3_wino4v_dgrad_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* dy, const float* wpt, const float* relu_src,
                                float* dx, float* vws, size_t vws_bytes);
int vc_conv3x3_wino4v_dgrad_bits_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* dy, const float* wpt,
                                     const uint32_t* mask_bits, float* dx, float* vws, size_t vws_bytes);
/* Winograd F(3x3, 2x2) weight gradient (csrc/conv_wino_wgrad.hip): both operands transformed in registers, the contraction runs over the
 * 2x2-pixel tiles; raw position sums per K split in the workspace, a reduce kernel sums the splits in fixed order and applies the
 * output transform.  Same contract as conv3x3_wgrad (db != NULL also returns the bias gradient, accumulate adds to dw / db); the
 * workspace is REQUIRED.  x, dy: C4 layout; dw: HWIO.  Shapes: H, W even, H >= 4, Cin % 64 == 0, Cout % 64 == 0; ask vc_conv3x3_wino_wgrad_supported. */
int vc_conv3x3_wino_wgrad_supported(int B, int H, int W, int Cin, int Cout);
size_t vc_conv3x3_wino_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int vc_conv3x3_wino_wgrad_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* dy, float* dw,
                              float* db, int accumulate, float* ws, size_t ws_bytes);

/* DIRECT 3x3 weight gradient on the bf16 matrix pipe (csrc/conv_wgrad_bx.hip; backward of tf.nn.conv2d w.r.t. the filter,
 * utils/image_embeddings.py:36-212, in the split-bf16 arithmetic of vc_gemm_bf16x3_f32 -- the opt-in mode of Trainer(precision="bf16x3")).
 * The contraction runs over the pixels; both operands are split in registers.  Same contract as vc_conv3x3_wino_wgrad_f32 (db != NULL also
 * returns the bias gradient -- summed in f32 --, accumulate adds to dw / db, the workspace is REQUIRED, results bit-reproducible).
 * x, dy: C4 layout, f32; dw: HWIO.  Shapes: Cin % 64 == 0, Cout % 64 == 0, any H, W >= 1; ask vc_conv3x3_bx_wgrad_supported. */
int vc_conv3x3_bx_wgrad_supported(int B, int H, int W, int Cin, int Cout);
size_t vc_conv3x3_bx_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int vc_conv3x3_bx_wgrad_f32(void* stream, int B, int H, int W, int Cin, int Cout, const float* x, const float* dy, float* dw,
                            float* db, int accumulate, float* ws, size_t ws_bytes);

/* conv1_1 (utils/image_embeddings.py:36-48: 3 -> 64 channels), csrc/conv_first.hip: the layer is HBM-bound (it writes / re-reads
 * the 64-channel activation, 822 MB at 64 images, for 0.6 % of the multiply-adds), so it has its own kernels: the forward makes
 * the 64 output channels the M dimension of the MFMA so that every lane stores 16-byte vectors of consecutive channels straight
 * from its accumulators (32 lanes = 32 consecutive pixels of one C4 plane); the weight gradient contracts 27 patch rows + one row of
 * ones (= the bias gradient) against dy and reduces per-workgroup partials in a fixed order.  y, dy: C4 layout ([B][16][H][W][4]);
 * x4: [B,H,W,4] from vc_vgg_preprocess_f32 (fourth channel ignored);
 * w / dw: [3,3,3,64] HWIO (no padding to 4 channels); W % 32 == 0 (ask vc_conv1_supported, else use vc_conv3x3_*_f32 on the
 * zero-padded weights).  There is no data gradient: the images are not trained. */
int vc_conv1_supported(int B, int H, int W);
size_t vc_conv1_wgrad_workspace_bytes(void);
int vc_conv1_fwd_f32(void* stream, int B, int H, int W, const float* x4, const float* w, const float* bias, float* y, int relu);
/* The forward with ReLU, also leaving (y > 0) as bits for the F(4x4,3x3) data gradient of the next layer (conv1_2): mask_out =
 * vc_conv3x3_wino4_mask_words(B, H, W, 64) words, to be passed to vc_conv3x3_wino4_dgrad_bits_f32(B, H, W, 64, Cout, ...); bit-identical
 * to that entry's float-mask form on y.  One launch (B images within 2 GiB), H % 16 == 0, W % 32 == 0. */
int vc_conv1_fwd_mask_f32(void* stream, int B, int H, int W, const float* x4, const float* w, const float* bias, float* y, uint32_t* mask_out);
int vc_conv1_wgrad_f32(void* stream, int B, int H, int W, const float* x4, const float* dy, float* dw, float* db, int accumulate,
                       float* ws, size_t ws_bytes);

/* ------------------------------------------------------------------------------------
 * Beam-search bookkeeping after one decoder step, on device, one wave per image: the loop body of
 * vae_model/decoder.py:254-293 with utils/top_n.py's TopN (heapq min-heap keyed by score; ties resolved by
 * heapq's sift order, reproduced exactly).  Rows are [B, beam]: row b*beam + i is the i-th live beam of
 * image b in heap-array order.
 *   in : top_p / top_i [B*beam, beam]  the beam_size most probable words of every row, descending, stable
 *        pcount [B] live beams; p_score / p_logprob (double) / p_len [B, beam]; sent_cur [B, beam, Lmax]
 *   out: the same for the new live beams (sent_next), the complete-caption heap c_* (captions in the pool
 *        c_sent [B, beam+1, Lmax], c_slot -> pool row, c_free = free-row bit mask, initially 2^(beam+1)-1),
 *        and for the next step parent [B*beam] (row whose LSTM state each new beam continues) and tok [B*beam].
 *   score of a completed caption = logprob / len^len_norm_f (len_norm_f <= 0: logprob); words with p < 1e-12 skipped.
 * ---------------------------------------------------------------------------------- */
int vc_beam_update(void* stream, int B, int beam, int Lmax, int eos, double len_norm_f, const float* top_p,
                   const int32_t* top_i, int32_t* pcount, int32_t* ccount, double* p_score, double* p_logprob,
                   int32_t* p_len, const int32_t* sent_cur, int32_t* sent_next, double* c_score, double* c_logprob,
                   int32_t* c_len, int32_t* c_slot, int32_t* c_free, int32_t* c_sent, int32_t* parent, int32_t* tok);

/* Group ("diverse") beam search bookkeeping after one decoder step (Diverse Beam Search, Vijayakumar et al. 2016, Hamming
 * dissimilarity): every image has `groups` beam searches of width w, one wave per image running its groups IN ORDER; a word that c live
 * beams of the round's earlier groups have just taken costs a candidate diversity * c of its heap key (rounded product, then rounded
 * difference; c == 0 leaves the key alone).  Per live beam the first w of its kc candidates under (key descending, raw rank ascending)
 * are walked like vc_beam_update walks a row.  The stored logprob stays the model's; <EOS> candidates are scored without the penalty.
 * The state is vc_beam_update's for B*groups "virtual images" v = b*groups + g of beam w (vc_beam_init with B*groups images):
 *   top_p / top_i [B*groups*w, kc], kc = min(groups*w, vocabulary) >= w; rows, heaps [B*groups, w]; pool c_sent [B*groups, w+1, Lmax];
 *   pcount / ccount / c_free [B*groups]; parent / tok [B*groups*w].  groups*w <= 16; diversity finite and >= 0.
 * groups == 1 is vc_beam_update(beam = w) move for move; diversity == 0 makes every group of an image the same search. */
int vc_beam_update_groups(void* stream, int B, int groups, int w, int kc, int Lmax, int eos, double len_norm_f, double diversity,
                          const float* top_p, const int32_t* top_i, int32_t* pcount, int32_t* ccount, double* p_score,
                          double* p_logprob, int32_t* p_len, const int32_t* sent_cur, int32_t* sent_next, double* c_score,
                          double* c_logprob, int32_t* c_len, int32_t* c_slot, int32_t* c_free, int32_t* c_sent, int32_t* parent,
                          int32_t* tok);

/* Constrained beam search bookkeeping after one decoder step (Anderson et al., EMNLP 2017): every image has C <= 3 constraints, each a
 * set of <= Wc <= 4 words that is satisfied once ANY of them has been emitted, and one beam search of width w per state s = the bit mask
 * of satisfied constraints (S = 2^C "banks", w * S <= 16).  One wave per image.  Per round every bank t is rebuilt from the OLD live beams
 * of bank t itself -- each row's first w of its kc listed words that belong to no set t lacks -- and then of the banks one constraint
 * short of t (missing bit ascending), which contribute every word of the missing set, forced, in table order; rows are walked in heap
 * array order like vc_beam_update walks them, p < 1e-12 skipped, <EOS> into the bank's complete heap.
 * The state is vc_beam_update's for B*S "virtual images" v = b*S + s of beam w (vc_beam_init with B*S images, then pcount of every bank
 * s > 0 set to 0): rows, heaps [B*S, w]; pool c_sent [B*S, w+1, Lmax]; pcount / ccount / c_free [B*S]; parent / tok [B*S*w], where parent
 * is the GLOBAL row (b*S + s)*w + i the new beam continues -- possibly a row of another bank of its image.
 *   cons [B, C, Wc]      the sets, padded with -1 (entries outside [0, V) count as absent; an all-absent set is never satisfied)
 *   top_p / top_i [B*S*w, kc]  vc_topk_rows_f32 of probs, kc = min(V, w + the largest number of constraint words of an image) <= w + C*Wc
 *   probs [B*S*w, ld >= V]     the softmax rows the lists were made from: the forced words' probabilities are read here
 * Rows of empty slots and banks are never read.  C == 0 is vc_beam_update(beam = w) move for move (cons and probs may be NULL). */
int vc_beam_update_constrained(void* stream, int B, int C, int Wc, int w, int kc, int Lmax, int eos, double len_norm_f,
                               const int32_t* cons, const float* top_p, const int32_t* top_i, const float* probs, long ld, int V,
                               int32_t* pcount, int32_t* ccount, double* p_score, double* p_logprob, int32_t* p_len,
                               const int32_t* sent_cur, int32_t* sent_next, double* c_score, double* c_logprob, int32_t* c_len,
                               int32_t* c_slot, int32_t* c_free, int32_t* c_sent, int32_t* parent, int32_t* tok);

/* The state vc_beam_update starts from, in ONE launch (vae_model/decoder.py:238-247: partial = [Beam([bos], state, 0.0, 0.0)], complete
 * empty): pcount = 1, ccount = 0, p_score = p_logprob = 0, p_len = 1, every sent_cur token = bos, sent_next / c_* / c_sent = 0,
 * c_free = 2^(beam+1)-1, parent[r] = r, tok[r] = bos, and the images' LSTM state expanded to the beam rows:
 * c_out[r] = c_in[r / beam], h_out[r] = h_in[r / beam] ([B, H] -> [B*beam, H]).  Same buffers and shapes as vc_beam_update. */
int vc_beam_init(void* stream, int B, int beam, int Lmax, int bos, int H, const float* c_in, const float* h_in, float* c_out, float* h_out,
                 int32_t* pcount, int32_t* ccount, double* p_score, double* p_logprob, int32_t* p_len, int32_t* sent_cur,
                 int32_t* sent_next, double* c_score, double* c_logprob, int32_t* c_len, int32_t* c_slot, int32_t* c_free,
                 int32_t* c_sent, int32_t* parent, int32_t* tok);

/* One beam-search round's row moves in ONE launch (vae_model/decoder.py:254-262): cg[r] = c[parent[r]], hg[r] = h[parent[r]] ([rows, H]
 * each) and, when xproj != NULL, gact[r] = xproj[tok[r]] ([vocab, G] -> [rows, G]: a word's LSTM input projection E.Wx + b looked up from a
 * table built once per generation call instead of multiplied every round).  H, G multiples of 4, 16-byte aligned pointers. */
int vc_beam_gather_f32(void* stream, const float* c, const float* h, const int32_t* parent, int rows, int H, float* cg, float* hg,
                       const float* xproj, const int32_t* tok, int vocab, int G, float* gact);

/* Stop-word bookkeeping of greedy / sampled decoding (vae_model/decoder.py:186-194), on device: done[b] |= (tok[b] == eos);
 * pending[0] = number of rows that have not emitted eos yet (a float, like the other device scalars). */
int vc_eos_track_i32(void* stream, const int32_t* tok, int B, int eos, int32_t* done, float* pending);

/* ------------------------------------------------------------------------------------
 * Diverse captioning (the AG-CVAE paper's use of z: K latent draws per image, each decoded, the candidates of an image merged by token
 * sequence and ranked).  Candidate rows are image-major: row r = b*K + k is draw k of image b.
 *   diverse_latent   z[r, s, l] = pm[r / K, l] + std * eps[r, s, l]  ([rows, S, L]; pm [rows / K, L] or NULL = zeros).  eps NULL: the
 *                    N(0,1) draws come from Philox, bit-identical to vc_philox_normal_f32(out, rows*S*L, seed, offset, step).
 *   decode_pick      one decoder round per row from one read of logits [rows, V] (ld): tok[r] = argmax (u NULL; first maximum, as
 *                    vc_argmax_rows_f32) or the inverse-CDF draw at `temperature` with u[round[0] * rows + r] (vc_multinomial_rows_f32's
 *                    partition and expressions: the same token); round NULL = 0, clamped to u_rounds - 1.  For rows with done[r] == 0 the
 *                    token is appended to seq [rows, Lmax] at len[r] (< Lmax), logprob[r] += its log-softmax at temperature 1 (f32 term,
 *                    f64 sum), len[r] += 1, and done[r] = (tok == eos).
 *   decode_pick_trunc decode_pick's sampled round with the distribution truncated before the draw (u is required).  y = fl32(x / temperature as
 *                    x * (1.0f / temperature)); order = y descending, equal y by lower index.  top_k > 0: only the first top_k words of
 *                    the order (0 or >= V: all).  top_p < 1: inside that set, the shortest prefix of the order whose mass
 *                    sum exp(y - max y) is >= top_p * the set's mass (at least one word; 1 = the whole set).  The draw is the inverse CDF
 *                    over the kept words in index order with target = u * their mass: the lowest-index kept word whose running kept
 *                    mass exceeds the target (else the last kept word).  Masses are summed as integers (multiples of 2^-32): the token
 *                    does not depend on rows, on the row's place in the launch or on the call.  logprob is decode_pick's: the
 *                    log-softmax at temperature 1 over the FULL vocabulary (the model's likelihood, not the sampler's).  kept (NULL or
 *                    [rows]): the number of words kept.  top_k 0 / >= V with top_p 1 is decode_pick itself, bit for bit.
 *   decode_pick_typical decode_pick's sampled round with cuts that follow the row's entropy or peak (u is required).  y as above, p =
 *                    softmax(y) over the FULL vocabulary, H = -sum p log p (nats; a word of zero mass adds 0).  typical_p = tau < 1: order by
 *                    d = |-log p - H| ascending, equal d by lower index, and keep the shortest prefix whose mass is >= tau (at least one
 *                    word; 1 = off).  min_p, eta: keep p >= max(min_p * p_max, min(eta, sqrt(eta) * exp(-H))) (0 = off; min_p = 1 keeps the
 *                    maxima of y).  Kept = typical set AND floor set, both taken on the full distribution (no cut renormalises for the
 *                    next); an empty intersection keeps the first maximum of y; a word of zero mass is never kept.  The draw, the integer
 *                    masses, logprob and kept are decode_pick_trunc's.  entropy (NULL or [rows]): H of every row.  All cuts off
 *                    (1, 0, 0) is decode_pick itself, bit for bit, with kept = V and entropy left UNTOUCHED.
 *   decode_round_end pending[0] = rows with done == 0 (float); round[0] += 1 when round is not NULL.  One workgroup.
 *   diverse_rank     per image (one workgroup, K <= 256, rows == B*K): score = logprob / (1 + len)^len_norm_f; candidates with equal token
 *                    sequences merged (best score kept, ties: lower draw); ranked <EOS>-ended first, then score descending, then lower
 *                    draw.  Writes n_distinct [B] and, per image, rep (draw index) / count / score [B, K] in rank order (slots past
 *                    n_distinct: rep -1, count 0, score 0). */
int vc_diverse_latent_f32(void* stream, long rows, int K, int S, int L, const float* pm, float std_, const float* eps, uint64_t seed,
                          uint64_t offset, const int32_t* step, float* z);
int vc_decode_pick_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature, const float* u, int u_rounds,
                       const int32_t* round, int eos, int32_t* tok, int32_t* done, int32_t* seq, int Lmax, int32_t* len, double* logprob);
int vc_decode_pick_trunc_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature, int top_k, float top_p,
                             const float* u, int u_rounds, const int32_t* round, int eos, int32_t* tok, int32_t* done, int32_t* seq, int Lmax,
                             int32_t* len, double* logprob, int32_t* kept);
int vc_decode_pick_typical_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature, float typical_p, float min_p,
                               float eta, const float* u, int u_rounds, const int32_t* round, int eos, int32_t* tok, int32_t* done,
                               int32_t* seq, int Lmax, int32_t* len, double* logprob, int32_t* kept, float* entropy);
int vc_decode_round_end_i32(void* stream, const int32_t* done, long rows, float* pending, int32_t* round);
int vc_diverse_rank(void* stream, long rows, int B, int K, int Lmax, const int32_t* seq, const int32_t* len, const int32_t* ended,
                    const double* logprob, double len_norm_f, int32_t* n_distinct, int32_t* rep, int32_t* count, double* score);

/* ------------------------------------------------------------------------------------
 * Decoding controls (csrc/decode_controls.hip; controls.py: DecodeControls): what a decoder may NOT say.  Before a round chooses words,
 * the logits [rows, V] (ld) are processed IN PLACE from every row's history, the W caption words it has emitted so far (no <BOS>):
 * hist[r*hist_ld + skip + i], i < W = clamp(len[r], skip, Lmax) - skip.  skip = 0: the candidate layout of vc_decode_pick_* (seq / len /
 * done); skip = 1: the beam layout (sent_cur / p_len, position 0 = <BOS>).  len outside [0, Lmax] is clamped (beam slots past pcount hold
 * stale lengths: nothing is read or written out of bounds for them).  Rows with done[r] != 0 (done may be NULL) are left alone; so are
 * the columns V..ld.  History entries outside [0, V) are ignored.  In this order:
 *   1. penalty     every DISTINCT history word w once: x[w] = x[w] > 0 ? x[w] * (1.0f / penalty) : x[w] * penalty  (f32)
 *   2. ngram = n   (n > 0, W >= n) for every p in [n-1, W) with h[p-n+1 .. p) == h[W-n+1 .. W): h[p] is banned (n = 1: every emitted
 *                  word; overlapping occurrences count: a a a with n = 2 bans a)
 *   3. banned      every id of the table (sorted ascending, unique, <= 256; NULL when n_banned == 0) is banned
 *   4. min_len     W < min_len: eos is banned
 * Banned: x[w] = -FLT_MAX (finite: probability exactly 0 in every consumer, and top-k still returns valid, distinct indices); a ban wins
 * over the penalty.  One wave per row; every touched logit has one owner lane and one store, so the result does not depend on rows, on
 * the row's place in the launch or on the call.  ngram 0..8, penalty finite >= 1, min_len >= 0, 0 <= eos < V, ld >= V,
 * 0 < Lmax <= 2048, hist_ld >= Lmax, 0 <= skip <= Lmax; ngram 0, min_len 0, penalty 1, n_banned 0 changes nothing.  rows == 0
 * launches nothing. */
int vc_decode_controls_f32(void* stream, float* logits, long rows, int V, long ld, const int32_t* hist, long hist_ld, int Lmax, int skip,
                           const int32_t* len, const int32_t* done, int ngram, int min_len, int eos, float penalty, const int32_t* banned,
                           int n_banned);

/* ------------------------------------------------------------------------------------
 * Contrastive search (csrc/contrastive.hip; generate.py: CaptionGenerator.contrastive_search; Su et al., NeurIPS 2022; DESIGN.md
 * "Contrastive search").  A deterministic decoder that scores a word by its probability AND by how unlike the caption's earlier
 * decoder states the state it leads to is.  Definition (normative): a row has emitted y_1..y_n (y_0 = <BOS>); g_j is the decoder
 * LSTM's output h after feeding y_j, j = 0..n (the vector decoder/rnn_logits reads; the z step's state is no part of the history), and
 * G_j = g_j / ||g_j||.  p = softmax (temperature 1) of the logits of g_n, after vc_decode_controls_f32 when controls are given.  The
 * candidates v_1..v_k are the first k words of p under vc_topk_rows_f32's stable descending order, k = min(contrastive_k, V), and h_i is
 * the LSTM output after feeding v_i from the row's state.
 *     sim_i = max_{j = 0..n} <h_i, G_j> / ||h_i||       (0 when ||h_i|| = 0, 0 over an empty history)
 *     s_i   = (1 - alpha) * p(v_i) - alpha * sim_i
 * The pick is the largest s_i, equal s going to the lower rank.  The row appends v_pick, adds (double)logf(p(v_pick)) to its
 * log-probability (f32 log of the f32 probability, f64 sum: vc_beam_update's), continues from the picked row's (c, h), appends
 * h_pick / ||h_pick|| to its history and is done once v_pick == eos.  alpha = 0 or k = 1 is greedy decoding; alpha = 1 ignores the
 * likelihood inside the top k.
 *   vc_contrastive_pick_f32  one round's pick, one workgroup per row.  h2 [rows * k, H]: the look-ahead outputs, row r * k + i for
 *     candidate i of row r; cand_tok / cand_p [rows, k]: the candidates' words and probabilities; hist [rows, Lmax + 1, H]: the unit
 *     vectors G_j, of which row r holds len[r] + (emit ? 1 : 0); seq [rows, Lmax], len, done [rows], logprob [rows] (float64): the rows'
 *     captions so far.  For a row with done == 0: hist[r, len + emit] = h_pick / ||h_pick|| (h_pick itself when its norm is 0),
 *     h_sel [rows, H] row r = h_pick (as it is: the operand of the next logits product), parent[r * k + i] = r * k + pick for every
 *     i < k (what vc_beam_gather_f32 takes to continue all k rows of the next round from the picked state), pick[r] = the rank and
 *     score[r, i] = s_i when those are not NULL; and with emit != 0: seq[r, len] = v_pick, len += 1, logprob += (double)logf(p_pick),
 *     done = (v_pick == eos).  emit == 0 leaves seq / len / logprob / done alone: the <BOS> round, which feeds <BOS> (k = 1, empty
 *     history) and only starts the history.  A row with done != 0, or one that already holds Lmax words under emit, writes nothing.
 *     Every history vector is read once per wave and multiplied into the wave's candidates, which stay in registers (H <= 1024);
 *     sums in a fixed order that depends on H alone, vector stores only, no atomics: a row's outputs do not depend on rows, on its
 *     place in the launch or on the call.  VC_EINVAL before any device work: a NULL pointer (pick, score may be NULL), k outside
 *     1..16, H no positive multiple of 4, Lmax < 1, h2 / hist / h_sel not 16-byte aligned, alpha outside [0, 1] or no number.
 *     rows == 0 launches nothing. */
int vc_contrastive_pick_f32(void* stream, long rows, int k, int H, int Lmax, const float* h2, const int32_t* cand_tok, const float* cand_p,
                            float* hist, int32_t* len, int32_t* done, int32_t* seq, double* logprob, float alpha, int eos, int emit,
                            float* h_sel, int32_t* parent, int32_t* pick, float* score);

/* ------------------------------------------------------------------------------------
 * Stochastic beam search (csrc/sbs.hip; generate.py: CaptionGenerator.stochastic_beam_search; Kool, van Hoof, Welling, ICML 2019): per
 * image n <= 32 DISTINCT captions, an exact sample without replacement from the model, by Gumbel top-k.  Beam rows are image-major: row
 * r = b*n + i is entry i of image b.  The state of an image: count [B] entries in rank order (best perturbed score first), each with
 * p_phi (float64 log-probability of its words), p_G (float64 perturbed score), p_len (words, <BOS> included), p_done (finished: its last
 * word is eos or it holds Lmax words; finished entries stay IN the beam and compete), its words in sent_cur [B, n, Lmax]; kappa [B]
 * (float64): the running maximum of the best perturbed score NOT taken, -inf while nothing was rejected.  Slots past count hold
 * p_phi = p_G = 0, p_len = 1, p_done = 1 (no round expands them), parent = their own row, tok = bos.
 *   sbs_init    count = 1, entry 0 = ([bos], 0, 0, not done), kappa = -inf, every sent_cur token = bos, sent_next = 0, parent[r] = r,
 *               tok[r] = bos, round[0] = 0 (round may be NULL), and the images' LSTM state expanded to the beam rows as vc_beam_init
 *               does: c_out[r] = c_in[r / n], h_out[r] = h_in[r / n] ([B, H] -> [B*n, H]).  VC_EINVAL: n outside 1..32, Lmax < 2, a NULL
 *               pointer.
 *   sbs_expand  one workgroup per row of logits [rows, V] (ld), rows = B*n; rows with r % n >= count[r / n] or done[r] != 0 are skipped
 *               (nothing read, nothing written).  lsm(v) = (x_v - M) - log S, M = max x, S = sum exp(x - M): f32, vc_decode_pick_f32's
 *               expressions and order (the same bits).  key(v) = (double)lsm(v) + g(v); the first kc words under (key descending, index
 *               ascending) go to cand_key [rows, kc] (float64, the key), cand_lsm [rows, kc] (f32) and cand_idx [rows, kc], always in
 *               [0, V) and distinct (a key that is no number ranks as -inf).  Noise: gumbel != NULL (float64 [g_rounds, rows, V]):
 *               g = gumbel[(rd * rows + r) * V + v], rd = round[0] (NULL: 0) clamped to g_rounds - 1.  gumbel == NULL: element
 *               i = r*V + v of the Philox stream (seed, offset) under the key step round[0] + step[0] (each NULL: 0), vc_philox_u32's
 *               counter convention, gives the word w; u = (w + 0.5) * 2^-32, g = -log(-log(u)), both float64.  The row is read from
 *               memory once (V <= 12288: staged in LDS; wider rows twice).  No atomics, every sum in a fixed order; a row's outputs
 *               depend on its own logits and noise only.  VC_EINVAL: rows no multiple of n, n outside 1..32, kc outside 1..33 or
 *               > V, ld < V, g_rounds < 1 with gumbel, a NULL pointer (gumbel, round, step may be NULL).
 *   sbs_update  one wave per image.  Candidates: the kc children of every live unfinished entry i,
 *               Gt = p_phi_i + key, Z = p_phi_i + key_0, t = G_i - Gt + log1mexp(Gt - Z), G' = G_i - max(0, t) - log1p(exp(-|t|))
 *               (the arg-max child: G' = G_i exactly), and every finished entry itself (G', p_phi unchanged).  The new beam is the best
 *               min(n, candidates) by (G' descending, parent ascending, word ascending), written IN PLACE in rank order: p_phi += the
 *               f32 lsm of the word, p_G = G', p_len + 1, p_done = (word == eos) or p_len == Lmax, sent_next = the parent's words of
 *               sent_cur plus the new one (sent_next != sent_cur), and for the next round parent [B*n] / tok [B*n] as vc_beam_gather_f32
 *               takes them (a carried finished entry: its own row before the update and eos).  kappa = max(kappa, G' of the best
 *               candidate not taken) when there is one; round[0] += 1 once per launch (round may be NULL).  kc is vc_sbs_expand_f32's
 *               (kappa is exact only with kc = min(n + 1, V)).  VC_EINVAL: n outside 1..32, kc outside 1..33, Lmax < 2,
 *               sent_cur == sent_next, a NULL pointer. */
int vc_sbs_init(void* stream, int B, int n, int Lmax, int bos, int H, const float* c_in, const float* h_in, float* c_out, float* h_out,
                int32_t* count, double* p_phi, double* p_G, int32_t* p_len, int32_t* p_done, int32_t* sent_cur, int32_t* sent_next,
                double* kappa, int32_t* parent, int32_t* tok, int32_t* round);
int vc_sbs_expand_f32(void* stream, const float* logits, long rows, int n, int V, long ld, const int32_t* count, const int32_t* done, int kc,
                      const double* gumbel, int g_rounds, const int32_t* round, uint64_t seed, uint64_t offset, const int32_t* step,
                      double* cand_key, float* cand_lsm, int32_t* cand_idx);
int vc_sbs_update(void* stream, int B, int n, int kc, int Lmax, int bos, int eos, const double* cand_key, const float* cand_lsm,
                  const int32_t* cand_idx, int32_t* count, double* p_phi, double* p_G, int32_t* p_len, int32_t* p_done,
                  const int32_t* sent_cur, int32_t* sent_next, double* kappa, int32_t* parent, int32_t* tok, int32_t* round);

/* ------------------------------------------------------------------------------------
 * Consensus re-ranking of diverse captions (consensus.py: ConsensusIndex; Devlin et al. 2015).  An index of D images (fc2 feature row,
 * one or more human captions); a query's k nearest index images by cosine, their captions pooled (neighbour order), every candidate
 * caption scored by the float64 mean of its m' = min(m, |pool|) largest CIDEr-D values against the pool.  Words: token ids without
 * <BOS>, <EOS> and PAD (0), at most 64, ids <= 65535.  n-gram keys (n = 1..4): the n ids packed 16 bits each, last word in the low bits.
 *   l2_normalize_rows   y[r] = x[r] / |x[r]| (f32 sum of squares; zero rows stay zero).  y == x allowed.
 *   topk_rows_wide      the first k (<= 256) entries of each row under (value descending, index ascending): with exclude NULL (or -1)
 *                       bit-identical to vc_topk_rows_f32 for non-NaN rows (+0 and -0 tie by index).  exclude[r] >= 0 drops column
 *                       exclude[r] of row r; slots past the row's eligible columns get index -1, value -inf.  One read of each row:
 *                       the best k of each 4096-column chunk (one workgroup) selected in LDS, the k-lists merged 4096 keys per
 *                       workgroup per launch.
 *                       ws: vc_topk_rows_wide_workspace_bytes(rows, cols, k) bytes (0 when cols <= 4096).
 *   ngram_vectors       per token row r of tok [n, ld] (the first len[r] entries): words[r] = its number of words L; the sorted distinct
 *                       n-gram keys of its words with weight count * idf in f32 (idf: the entry of the sorted df_keys [n_df] table, or
 *                       idf_unseen) at keys / w [off[r], off[r + 1]) (nnz[r] of them; the host sizes the range for L words:
 *                       sum_n max(0, L - n + 1)); norm[r, n-1] = |v_n| (sum of squares in f64, stored f32).  One wave per row.
 *   consensus_score     image b (< B) has candidates cand_img[b] .. cand_img[b+1] - 1 (at most max_cands <= 256) and neighbours
 *                       nbr [B, k] (k <= 256; -1 = none); index image i has the captions img_cap[i] .. img_cap[i+1] - 1 (pool <= 2048).
 *                       Captions (r_*) and candidates (c_*) are ngram_vectors outputs (off, nnz, keys, w, norm [.,4], words).  CIDEr-D(c, r)
 *                       = 10 exp(-(L(c) - L(r))^2 / 72) / 4 sum_n sum_g min(c_g, r_g) r_g / (|c_n| |r_n|) (0 when a norm is 0), in f32;
 *                       score[c] = f64 mean of the m' largest over the pool.  One workgroup per image and 4 candidates, ~53 KiB LDS. */
int vc_l2_normalize_rows_f32(void* stream, const float* x, long rows, int cols, long ld, float* y, long ldy);
size_t vc_topk_rows_wide_workspace_bytes(long rows, int cols, int k);
int vc_topk_rows_wide_f32(void* stream, const float* x, long rows, int cols, long ld, int k, const int32_t* exclude, float* out_val,
                          int32_t* out_idx, void* ws, size_t ws_bytes);
int vc_ngram_vectors(void* stream, const int32_t* tok, long n, long ld, const int32_t* len, int bos, int eos, const uint64_t* df_keys,
                     const float* idf, long n_df, float idf_unseen, const int32_t* off, uint64_t* keys, float* w, int32_t* nnz, float* norm,
                     int32_t* words);
int vc_consensus_score(void* stream, int B, int k, const int32_t* nbr, const int32_t* img_cap, const int32_t* r_off, const int32_t* r_nnz,
                       const uint64_t* r_keys, const float* r_w, const float* r_norm, const int32_t* r_len, const int32_t* cand_img,
                       int max_cands, const int32_t* c_off, const int32_t* c_nnz, const uint64_t* c_keys, const float* c_w,
                       const float* c_norm, const int32_t* c_len, int m, double* score);

/* ------------------------------------------------------------------------------------
 * In-set CIDEr-D (mbr.py: CiderGram; csrc/cider_gram.hip): every caption of an image against every caption of the same image.
 *   cider_gram   ONE ngram_vectors table (off, nnz, keys, w, norm [.,4], words); image b (< B) owns its rows cand_img[b] ..
 *                cand_img[b+1] - 1 (n_b <= max_cands <= 256).  For row i of image b and column j < n_b,
 *                  gram[i * ld + j] = CIDEr-D(hypothesis = caption i, reference = caption j of the image)     (ld >= max_cands)
 *                in f32 by consensus_score's pair function (csrc/cider_pair.h): the same bits for the same pair.  Columns j >= n_b of
 *                a row are not written.
 *                  mbr[i] = (sum_j weight[j] * (double)gram[i][j]) / sum_j weight[j]
 *                over ALL j of the image (i included), weight [C] per caption row (NULL: all 1), in float64 with a fixed order (one term
 *                per lane, an xor shuffle tree per wave, the wave sums in wave order; no atomics); 0.0 when the weight sum is 0.
 *                gram or mbr may be NULL (not both).  A row's bits depend on its image's captions (and weights) only: not on B, the
 *                other images or the row's place in its group.  One workgroup per image and 4 rows, 12 KiB LDS. */
int vc_cider_gram(void* stream, int B, const int32_t* cand_img, int max_cands, const int32_t* off, const int32_t* nnz, const uint64_t* keys,
                  const float* w, const float* norm, const int32_t* words, const double* weight, float* gram, long ld, double* mbr);

/* ------------------------------------------------------------------------------------
 * DPP selection (mbr.py: CiderGram.select; csrc/dpp.hip; DESIGN.md "DPP selection"): n of an image's m captions chosen jointly for
 * quality and for difference from each other -- the fast greedy MAP of a determinantal point process (Chen, Zhang & Zhou, NeurIPS
 * 2018) over the image's in-set CIDEr-D matrix.  Per image: m captions (0 <= m <= 256) in list order, their vc_cider_gram matrix G
 * (f32), a positive quality q_i per caption (float64), a count n (1 <= n <= 32).  Everything below is float64.
 *   similarity   S_ij = min(1, max(0, ((double)G_ij + (double)G_ji) / 20)) for i != j, S_ii = 1.  (CIDEr-D is scaled by 10 and is not
 *                symmetric; the diagonal is SET, not read: an empty caption's self-score is 0.)
 *   kernel       L_ij = q_i S_ij q_j.
 *   state        d_i = q_i^2; no caption is taken; vectors c_t[.] exist for the steps t done so far.
 *   step k = 0, 1, ... while fewer than min(n, m) captions are taken:
 *                a caption is LIVE if it is not taken and d_i > DPP_EPS * q_i^2.  No caption live: stop.  Otherwise
 *                j = argmax over the live i of d_i (equal values go to the lower index); sel[k] = j, gain[k] = d_j, j is taken.
 *                For every untaken i: acc = q_j S_ji q_i; for t = 0 .. k-1 in ascending order acc -= c_t[j] * c_t[i];
 *                e = acc / sqrt(d_j); c_k[i] = e; d_i -= e * e.
 *   after        n_dpp = the number of steps taken.  Fewer than min(n, m) taken: the remaining slots hold the untaken captions in
 *                ascending index with gain 0 (what is left are duplicates and numerically dependent captions; they go in rank order).
 *                Slots at or past min(n, m): sel = -1, gain = 0.
 * The steps maximise log det L_Y one element at a time; CIDEr-D's clipping means S need not be positive semidefinite, and the live
 * rule makes the procedure well defined anyway.  When the qualities differ, sel[0] is the caption with the largest q.
 *   dpp_select   cand_img [B + 1], gram and ld are vc_cider_gram's: table row i lives at gram + i * ld, image b owns the rows
 *                cand_img[b] .. cand_img[b+1] - 1 (n_b <= max_cands; a longer list is cut at max_cands as vc_cider_gram cuts it), so
 *                the selection runs on the block that call has just written.  q [C]: one quality per table row.  sel, gain [B, n],
 *                n_dpp [B]; sel holds indices WITHIN the image.  n_b == 0: sel = -1, gain = 0, n_dpp = 0.
 *                One workgroup per image, one lane per caption; d, q and the taken flags in registers, the c vectors in LDS (n x 256
 *                doubles: 16 KiB up to n = 8, 64 KiB above); row j and column j of G are read once per step; the argmax is an
 *                index-carrying xor shuffle tree per wave, then the four wave results through LDS in wave order.  No atomics; no
 *                product is contracted into a fused multiply-add.  An image's outputs depend on its own rows, q and n only: not on B,
 *                its place in the launch, max_cands or the call -- two calls give identical bits.
 *                q_i finite and > 0 is the caller's to check (mbr.py does): the kernel does not.
 *                VC_EINVAL before any device work: B < 0, max_cands outside 1..256, n outside 1..32, ld < max_cands, a NULL pointer
 *                with B > 0.  B == 0 launches nothing (no pointer is looked at). */
#define DPP_EPS 1e-9
int vc_dpp_select_f64(void* stream, int B, const int32_t* cand_img, int max_cands, const float* gram, long ld, const double* q, int n,
                      int32_t* sel, double* gain, int32_t* n_dpp);

/* ------------------------------------------------------------------------------------
 * Evaluation of caption sets (evaluate.py: CaptionEvaluator; csrc/evaluate.hip): BLEU-style clipped n-gram counts.
 *   ngram_overlap   Hypotheses (c_*, C rows) and references (r_*, n_ref rows) are ngram_vectors outputs (off, nnz, keys, w, words) built
 *                   with an EMPTY df table (n_df = 0, idf_unseen = 1.0f): w is then the n-gram's count as an exact float.  The two tables
 *                   may be the same one.  Hypothesis c is compared with the reference rows [lo[c], hi[c]) except row skip[c] (-1: none).
 *                   The range is clamped on the device: lo' = min(max(lo, 0), n_ref), hi' = min(max(hi, lo'), n_ref), so lo > hi and
 *                   ranges outside the table read nothing and give the results of an empty range; a skip outside the range drops
 *                   nothing.  (lo, hi and skip are device arrays: the host checks the scalars and the pointers only.)
 *                   With c_g the hypothesis's count of n-gram g and m_g the largest count of g over the range's rows, per order n = 1..4:
 *                     total[c, n-1]    = sum_g c_g             (= max(0, L - n + 1))
 *                     match[c, n-1]    = sum_g min(c_g, m_g)   (BLEU's clipped count)
 *                     distinct[c, n-1] = the number of distinct n-grams g
 *                     unseen[c, n-1]   = the number of those with m_g = 0
 *                     ref_len[c]       = the words of the range's row that minimises (|L_r - L_c|, L_r): a tie goes to the shorter
 *                   An empty range (also after the skip) gives match 0, unseen = distinct, ref_len 0.  All outputs are int32 sums and
 *                   maxima: a row's results depend on the row and its range only.  One wave per hypothesis, four per workgroup, 16 KiB LDS. */
int vc_ngram_overlap(void* stream, long C, const int32_t* c_off, const int32_t* c_nnz, const uint64_t* c_keys, const float* c_w,
                     const int32_t* c_len, long n_ref, const int32_t* r_off, const int32_t* r_nnz, const uint64_t* r_keys, const float* r_w,
                     const int32_t* r_len, const int32_t* lo, const int32_t* hi, const int32_t* skip, int32_t* total, int32_t* match,
                     int32_t* distinct, int32_t* unseen, int32_t* ref_len);

/* ------------------------------------------------------------------------------------
 * ROUGE-L counts (evaluate.py: lcs_overlap, CaptionEvaluator; scst.py: RougeReward; csrc/lcs.hip): longest common subsequences.
 *   lcs_overlap     c_tok [C, c_ld] and r_tok [n_ref, r_ld] are word rows (consensus.word_rows): left-aligned, len[r] valid words per row
 *                   (clamped to 0 .. min(64, ld)); entries at and past len are never read.  The two tables may be the same one.
 *                   Hypothesis c is compared with the reference rows [lo[c], hi[c]) except row skip[c] (-1: none); the range is clamped
 *                   on the device exactly as ngram_overlap's: lo' = min(max(lo, 0), n_ref), hi' = min(max(hi, lo'), n_ref), so lo > hi
 *                   and ranges outside the table give the results of an empty range; a skip outside the range drops nothing.
 *                   Only rows of the range with at least one word take part.  With LCS(c, r) the length of the longest common
 *                   subsequence of the two word sequences:
 *                     lcs_max[c]              = the largest LCS(c, r) over the range            (ROUGE-L precision = lcs_max / L_c)
 *                     rec_lcs[c], rec_len[c]  = (LCS(c, r), L_r) of the row that maximises LCS(c, r) / L_r, ratios compared by integer
 *                                               cross-multiplication; a tie in the ratio goes to the smaller L_r   (recall = rec_lcs / rec_len)
 *                   No row taking part (empty range, also after the skip, or zero-word rows only): all three are 0.  All outputs are
 *                   exact int32 values: a row's results depend on the row and its range only.  One wave per hypothesis, four per
 *                   workgroup: lane i holds hypothesis word i, the match mask of a reference word is one 64-bit ballot, the LCS row state
 *                   one 64-bit integer (bit-parallel recurrence V' = (V + (V & M)) | (V - (V & M)) modulo 2^64).  No LDS, no atomics.
 *                   C == 0 is a successful no-op (no pointer is looked at); C < 0, n_ref < 0 or >= 2^31, a pitch < 1, or a null pointer
 *                   with C > 0 are VC_EINVAL. */
int vc_lcs_overlap(void* stream, long C, const int32_t* c_tok, long c_ld, const int32_t* c_len, long n_ref, const int32_t* r_tok, long r_ld,
                   const int32_t* r_len, const int32_t* lo, const int32_t* hi, const int32_t* skip, int32_t* lcs_max, int32_t* rec_lcs,
                   int32_t* rec_len);

/* ------------------------------------------------------------------------------------
 * Scoring given captions (generate.py: CaptionGenerator.score; csrc/score.hip).  Forward only.
 *   logits_logprob   lp[r] = (hs[r] . W[:, labels[r]] + bias[labels[r]]) - log sum_{v < V} exp(hs[r] . W[:, v] + bias[v]) for every row of
 *                    hs [rows, H] (row pitch `pitch`), W [H, ldw] (columns >= V, the padding of the stored logits kernel, never enter the
 *                    sum), bias [V] or NULL.  labels[r] < 0 or >= V: row not scored, lp[r] = 0.  f32 MFMA products, f32 accumulate;
 *                    H % 32 == 0.  The [rows, V] logits are never written: every 128 x 128 tile of them is reduced on chip to one
 *                    (max, sum of exp) pair per row, and a second kernel merges a row's cdiv(V, 128) pairs in ascending tile order.
 *                    No atomics: two calls give identical bits, and a row's value does not depend on `rows`.
 *                    ws: vc_logits_logprob_workspace_bytes(rows, V, H) = rows * (2 * cdiv(V, 128) + 1) floats, 8-byte aligned; a smaller
 *                    one is VC_EWORKSPACE.
 *   score_reduce     lp [T, C*K] (time-major; column c*K + k = caption c under draw k), len [C] (tokens scored, clamped to 0..T):
 *                    logprob [C, K] = sum_{t < len[c]} lp (float64, ascending t); marginal [C] = log sum_k exp(logprob[c, k]) - log K
 *                    (float64, max-shifted).  One wave per caption, K <= 256.
 * ---------------------------------------------------------------------------------- */
size_t vc_logits_logprob_workspace_bytes(long rows, int V, int H);
int vc_logits_logprob_f32(void* stream, long rows, int V, int H, const float* hs, long pitch, const float* W, long ldw, const float* bias,
                          const int32_t* labels, float* lp, float* ws, size_t ws_bytes);
int vc_score_reduce_f64(void* stream, const float* lp, int T, int C, int K, const int32_t* len, double* logprob, double* marginal);

/* ------------------------------------------------------------------------------------
 * Posterior at inference: ELBO and importance-weighted bound of given captions (generate.py: CaptionGenerator.bound; csrc/bound.hip;
 * DESIGN.md "Bounds").  Rows are caption-major, draw-minor: r = c*K + k.  sigma_p = prior_std; pm [n_img, L] with img [rows / K] = the
 * pm row of every caption, or both NULL (a zero prior mean).  Every float64 sum is per-lane partials in a fixed stride order, then a fixed
 * shuffle tree: no atomics, and what a row gets depends on the row only (not on its index, nor on the other rows of the call).
 *   posterior_latent  z[r, s, l] = mean[r / K, l] + std_[r / K, l] * eps[r, s, l] (f32, vc_latent_sample_f32's expression) for mean, std_
 *                     [rows / K, L]; eps [rows, S, L], or NULL: N(0,1) draws from Philox, bit-identical to
 *                     vc_philox_normal_f32(out, rows*S*L, seed, offset, step) -- a draw is defined by its flat element index, so a row
 *                     whose S*L is no multiple of 4 may start inside a Philox quad.  logw[r] (float64) = sum_{s,l} [ -0.5 ((z - pm_l) /
 *                     sigma_p)^2 - log sigma_p + 0.5 eps^2 + log std_l ] = log p(z) - log q(z), the 2 pi terms cancelled, from the f32 z,
 *                     eps, std_, pm: one pass, z written and its term accumulated from the same registers.
 *   gauss_kl_rows     kl[c] = S * sum_l [ log(sigma_p / std_l) + (std_l^2 + (mean_l - pm_l)^2) / (2 sigma_p^2) - 0.5 ] (float64).
 *   bound_reduce      lp [T, C*K], len [C] as vc_score_reduce_f64; logw [C*K].  logprob [C, K] = vc_score_reduce_f64's sums (same bits;
 *                     len[c] == 0: zeros); with a_k = logprob[c, k] + logw[c, k]: out [C, 5] = elbo = mean_k a_k, iwae = log sum_k
 *                     exp(a_k - max a) + max a - log K, rec = mean_k logprob, kl_mc = -mean_k logw, ess = (sum_k v_k)^2 / sum_k v_k^2
 *                     with v_k = exp(a_k - max a).  One wave per caption, K <= 256.
 * K outside 1..256, S or L < 1, a negative size or a NULL output is VC_EINVAL.
 * ---------------------------------------------------------------------------------- */
int vc_posterior_latent_f32(void* stream, long rows, int K, int S, int L, const float* mean, const float* std_, const float* pm,
                            const int32_t* img, float prior_std, const float* eps, uint64_t seed, uint64_t offset, const int32_t* step,
                            float* z, double* logw);
int vc_gauss_kl_rows_f64(void* stream, long C, int S, int L, const float* mean, const float* std_, const float* pm, const int32_t* img,
                         float prior_std, double* kl);
int vc_bound_reduce_f64(void* stream, const float* lp, int T, int C, int K, const int32_t* len, const double* logw, double* logprob,
                        double* out);

/* ------------------------------------------------------------------------------------
 * Mutual information I(x; z) under the aggregated posterior (latent_mi.py: mutual_information; csrc/latent_mi.hip; DESIGN.md "Bounds",
 * "Mutual information"): the draws of N captions scored under a table of M Gaussian posteriors.  z [N, S, L], mean and std_ [M, L], all
 * f32; every operation is float64 on the f32 inputs converted to float64:
 *   gauss_mix_lse   t[n, s, m]      = sum_l [ -0.5 ((z[n,s,l] - mean[m,l]) / std_[m,l])^2 - log std_[m,l] ] - 0.5 L log(2 pi)
 *                   lse_block[n, s] = log sum_m exp(t[n, s, m])              [N, S]: one L-dimensional block under the mixture
 *                   lse_full[n]     = log sum_m exp(sum_s t[n, s, m])        [N]: the S*L-dimensional code the decoder is given
 *                   both max-subtracted: a table of sharp posteriors, whose far terms underflow, gives finite values.  The quotient is
 *                   formed as (z - mean) * (1 / std_) with one IEEE division per table element; sum_l log std_ is summed apart from the
 *                   squares.  std_ > 0 is the caller's to check (latent_mi.py does): the kernel does not.
 *                   A workgroup owns 128 / S whole captions (64 / S for S < 8) with all their draws and streams the table past them in
 *                   chunks of 64 posteriors by tiles of 32 dimensions (mean and 1 / std_ as float64 in LDS, ~129 KiB); a lane keeps the
 *                   running (max, sum) pair of every row it owns for the posteriors lane, lane + 64, ... in ascending order, rescaled
 *                   online; the 64 lanes' pairs are merged by xor shuffle trees.  sum_s runs in ascending s.  No atomics: two calls
 *                   give identical bits, and a caption's outputs depend on its own z rows and the table only -- not on N, on its index
 *                   or on the other captions.  No load runs past a row's end (any L >= 1).
 *                   N == 0 is a successful no-op (no pointer is looked at).  N < 0, M, S or L < 1, S > 128 (the rows a workgroup keeps
 *                   in registers), N or M >= 2^31, or a null pointer with N > 0 are VC_EINVAL, returned before any launch. */
int vc_gauss_mix_lse_f64(void* stream, long N, long M, int S, int L, const float* z, const float* mean, const float* std_,
                         double* lse_block, double* lse_full);

/* ------------------------------------------------------------------------------------
 * Marginal decoding: search under the K-draw mixture p(y | I) ~ 1/K sum_k p(y | z_k, I) (generate.py: CaptionGenerator.marginal_greedy /
 * marginal_beam_search; csrc/mixture.hip; DESIGN.md "Marginal decoding").  A hypothesis group g owns the K consecutive rows r = g*K + k
 * (draw-minor: vc_diverse_*'s image-major rows).  Per row, x = logits[r, :V] (row pitch ld; columns >= V are never read): M_r = max x,
 * S_r = sum_v exp(x_v - M_r), lsm_r(v) = (x_v - M_r) - log S_r, all f32 with vc_decode_pick_f32's expressions.  logw[r] (float64): the
 * log-likelihood of the group's prefix under draw k; w_r = exp(logw[r] - max_k logw) / sum_k exp(logw - max_k logw) (float64).
 *   mixture_topk      q_g(v) = sum_k w_r exp(x_rv - M_r) / S_r (f32, k ascending): top_p / top_i [G, kc] = the first kc (1..16, <= V) words
 *                     of q_g under (value descending, index ascending), top_p the f32 probabilities in the form vc_beam_update takes;
 *                     stat [G*K, 2] = (M_r, log S_r).  1 <= G <= 65535.  A group's outputs depend on its K rows only: no atomics, every
 *                     sum in a fixed order, the same bits in every call, for any G and any place of the group in the launch.  Rows of
 *                     dead beams may hold anything: words are selected by comparing (value, column) pairs, never through an offset
 *                     computed from a value, top_i is always in [0, V), and a q that is not a number is reported as -1.
 *                     Three launches: the row statistics (one workgroup per row), the best kc of every (group, 1024-column chunk), a
 *                     per-group merge.  ws: vc_mixture_topk_workspace_bytes(G, V, kc) = G * cdiv(V, 1024) * kc * 8 bytes, 4-byte
 *                     aligned; a smaller one is VC_EWORKSPACE.
 *   mixture_advance   for every new group g < Gn and draw k, with src = (parent ? parent[g] : g) * K + k (parent[g]: a group of the round
 *                     that stat / logits describe, clamped to [0, Gn)) and w = tok[g]: logw_out[g*K + k] = logw_in[src] + (double)
 *                     lsm_src(w) (f32 term from stat, f64 sum; logw_in != logw_out), parent_rows[g*K + k] = src (NULL: not wanted),
 *                     tok_rows[g*K + k] = w: what vc_beam_gather_f32 and the embedding gather take for the expanded rows.
 *                     Greedy form (done [Gn], seq [Gn, Lmax], len [Gn] given, parent NULL): a group with done[g] == 0 and len[g] < Lmax
 *                     appends w to seq[g, len[g]], len[g] += 1, and its logw advances; then done[g] = (w == eos).  A group with
 *                     done[g] != 0 changes nothing and its logw is copied through, as is that of a group whose seq row is full.
 *                     Beam form: done, seq and len all NULL.  One workgroup per group.
 * K outside 1..256, kc outside 1..min(16, V), ld < V, a NULL required pointer or a mixed greedy / beam form is VC_EINVAL.
 * ---------------------------------------------------------------------------------- */
size_t vc_mixture_topk_workspace_bytes(long G, int V, int kc);
int vc_mixture_topk_f32(void* stream, const float* logits, long G, int K, int V, long ld, const double* logw, int kc, float* top_p,
                        int32_t* top_i, float* stat, void* ws, size_t ws_bytes);
int vc_mixture_advance_f32(void* stream, const float* logits, int V, long ld, const float* stat, long Gn, int K, const int32_t* parent,
                           const int32_t* tok, const double* logw_in, double* logw_out, int32_t* parent_rows, int32_t* tok_rows, int eos,
                           int32_t* done, int32_t* seq, int Lmax, int32_t* len);

/* ------------------------------------------------------------------------------------
 * Host-side helper (the only entry point that takes HOST pointers): CRC-32C (Castagnoli) of a byte
 * range, continuing from *crc_inout (start with 0).  Used by the TensorFlow V2 checkpoint
 * ("tensor bundle") reader / writer for the per-tensor and per-block checksums
 * (main.py:189-190,286-288 tf.train.Saver; gen_caption.py:113-115 saver.restore).
 * ---------------------------------------------------------------------------------- */
int vc_host_crc32c(const void* data, size_t nbytes, uint32_t* crc_inout);

/* ------------------------------------------------------------------------------------
 * Collectives of the data-parallel step (RCCL over xGMI; csrc/comm.hip).  The reference is single-GPU
 * (utils/parameters.py:163-164 picks one device): these have no counterpart there.  One process per GPU; rank 0 calls
 * vc_comm_unique_id and hands the 128 bytes to every rank out of band (a file, the launcher's store, MPI ...); every rank then calls
 * vc_comm_init_rank (collective: returns when all `world` ranks have joined).  RCCL is bound at run time (the process's
 * already-loaded librccl.so.1 if there is one -- PyTorch bundles its own --, else the ROCm install; VC_RCCL_LIB overrides), so a
 * single-GPU user needs none.  All calls are stream-ordered on `stream` and in place / out of place as declared; any RCCL failure
 * (incl. an asynchronous error an earlier collective left on the communicator) is a non-zero return with the RCCL message in
 * vc_last_error(), and a destroyed / aborted communicator is refused instead of dereferenced.
 *   vc_allreduce_sum_f32      buf[n] <- sum over ranks, in place: the gradient buffer (or one bucket of it), the CE denominator,
 *                             the loss scalars (trainer.py, engine.py: fw_loss)
 *   vc_allgather_f32          out[world * n_per_rank] <- rank-ordered concatenation of in[n_per_rank]: mean / std of the global batch
 *                             before the Q1-mixed latent sample (vae_model/decoder.py:109-110 reshapes across rows)
 *   vc_reducescatter_sum_f32  out[n_per_rank] <- this rank's slice of the sum of in[world * n_per_rank]: the gradients of that mix */
int vc_comm_available(void);                                   /* 1: an RCCL library can be loaded */
int vc_comm_unique_id(void* id128);                            /* rank 0: 128 bytes to distribute */
int vc_comm_init_rank(int world, int rank, const void* id128, int device, void** comm_out);
int vc_comm_info(void* comm, int* world, int* rank, int* rccl_version);
int vc_comm_destroy(void* comm);
int vc_comm_abort(void* comm);
int vc_allreduce_sum_f32(void* comm, void* stream, float* buf, size_t n);
int vc_allgather_f32(void* comm, void* stream, const float* in, float* out, size_t n_per_rank);
int vc_reducescatter_sum_f32(void* comm, void* stream, const float* in, float* out, size_t n_per_rank);

#ifdef __cplusplus
}
#endif
#endif
