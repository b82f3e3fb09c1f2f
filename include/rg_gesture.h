/*
 * rg_gesture.h -- C ABI of the MI355X (gfx950) HIP extension for the RAG-Gesture
 * inference hot path.
 *
 * The reference (m-hamza-mughal/RAG-Gesture) is 100% Python on PyTorch eager ops; it has
 * no FFI of its own.  Each entry point below therefore cites the reference Python
 * function whose arithmetic it replaces (path:line under the reference tree), and
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the name
 *     ends in _host.  Buffers are owned by the caller (torch tensors in the host code).
 *   - every launch goes to `stream` (a hipStream_t passed as void*); no entry point
 *     synchronises, allocates or reads back, so all of them are hipGraph-capturable.
 *   - return 0 on success, negative rg_status otherwise; rg_last_error() gives the text.
 *   - fp32 activations are row-major; "token rows" M = batch_rows * T (T = 43 latent tokens).
 */
#ifndef RG_GESTURE_H
#define RG_GESTURE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rg_handle rg_handle;

enum rg_status {
  RG_OK = 0,
  RG_ERR_INVALID = -1,   /* bad argument (null pointer, unsupported shape) */
  RG_ERR_HIP = -2,       /* a HIP runtime call or launch failed */
  RG_ERR_NO_DEVICE = -3
};

/* ABI version of THIS header: bumped whenever an argument block (rg_seq_args, ...) or an entry point changes shape.  A caller
 * compares it with rg_version() of the library it loaded (rag-gesture_amd/capi.py load_library does and refuses a mismatch).
 * 110 (round 6): rg_seq_args gains `form`; the two entry points of the device-chosen launch form (removed in 131).  100 -> 105
 * were the unversioned states of rounds 1-5 (round 5 changed rg_seq_args -- gbuf in, l0 / l1 out -- and the afrag layout
 * without a bump: ADVICE r05).
 * 111: rg_seq_args gains `glue_ctr` and `glue` (the loop step's update at the end of the forward, csrc/rg_tail.h).
 * 112: rg_fgd_layer_args, rg_fgd_encoder_layer, rg_latent_moments (FGD evaluation).
 * 113: rg_smplx_joints_args, rg_smplx_joints, rg_joint_stats_args, rg_joint_clip_stats, rg_pair_dist_args,
 *      rg_pair_distance_sums (SMPL-X joint metrics).
 * 114: rg_mesh_transforms_args, rg_mesh_transforms, rg_mesh_blend_args, rg_mesh_blend_skin, rg_mesh_face_sums_args,
 *      rg_mesh_face_sums (SMPL-X mesh vertices and the face metrics).
 * 115: rg_render_project_args, rg_render_project, rg_render_bin_args, rg_render_bin, rg_render_raster_args, rg_render_raster
 *      (SMPL-X clip rendering).
 * 116: rg_srgr_args, rg_srgr_clip_sums (SRGR).
 * 117: rg_venc_args gains the posterior-only store (post_rows, post_mu, post_logvar, post_nrows); rg_vae_reparam_cached.
 * 118: rg_smplx_joints_expr_args, rg_smplx_joints_expr, rg_clip_prepare_args, rg_clip_prepare, rg_joint_speed_args,
 *      rg_joint_speed_sums (model inputs and the mean-velocity file from raw SMPL-X recordings).
 * 119: rg_onset_mel_args, rg_onset_mel_db, rg_onset_pick_args, rg_onset_pick (audio onsets for beat alignment).
 * 120: rg_seq_args gains `twin` (rg_seq2_forward: a clip's conditional and classifier-free sequences in one workgroup).
 * 121: rg_wave_normalize, rg_time_groupnorm_gelu_batched, rg_im2col_grouped_batched, rg_embed_sum3_ragged, rg_mha_bf16_ragged
 *      (conditioning features of many windows per call).
 * 122: rg_resample_poly and RG_RESAMPLE_* (recorded audio of any rate, channel count and sample format to 16 kHz mono).
 * 123: rg_decode_outputs (the output conversions behind the four body-part decoders in one launch); rg_vdec_args gains
 *      latent / table / frames (rg_vdec_step builds its input rows and compacts its output rows itself).
 * 124: rg_seq_forward_many and RG_SEQ_MANY_MAX (the forwards of several sessions in one launch).
 * 125: rg_jpeg_dct_quant, rg_jpeg_entropy_count, rg_jpeg_entropy_write and RG_JPEG_* (baseline JPEG of rendered frames).
 * 126: rg_ctc_log_softmax, rg_ctc_align, rg_word_frames and RG_CTC_* (word timings from CTC emissions; word vectors on frames).
 * 127: rg_prosody_frames, rg_prosody_signal, rg_prosody_cwt, rg_prosody_words and RG_PROSODY_* (word prominence from audio).
 * 128: rg_seq2_forward_many (the twin-form forwards of several sessions in one launch).
 * 129: rg_text_diag_sim_many, rg_discourse_search_batch, rg_retrieval_pack_rows (a batch's exemplar search in one call).
 * 130: rg_rank_survivors_batch (the ranking half of that call, for any sweep); rg_discourse_scores and rg_text_diag_sim removed.
 * 131: rg_seqx_forward, rg_lane_form, RG_LANE_STRIDE and rg_seq_args.form removed (the device-chosen launch form of 110: slower
 *      on the headline and unreachable from the twin and grouped launches; the fields behind `form` move up by 8 bytes).
 * 132: rg_prosody_scores_batched (the sweep of the `prosody` retrieval method: exemplars by word prominence).
 * 133: rg_motion_scores_batched (the sweep of the `motion` retrieval method: exemplars by a motion example).
 * 134: rg_foot_skate_sums, rg_foot_plant and RG_FOOT_SUMS (foot skating measured, contact feet planted).
 * 135: rg_foot_lock_targets, rg_foot_lock_ik and RG_FOOT_LOCK_STATS (contact ankles locked by analytic leg IK). */
#define RG_VERSION 135
int rg_version(void);
int rg_create(rg_handle** out, int device);
void rg_destroy(rg_handle* h);
const char* rg_last_error(rg_handle* h);
/* Compute units of the handle's device (tile-shape policies: one workgroup per CU while a launch fits). */
int rg_num_cus(rg_handle* h);

/* ---------------------------------------------------------------- sampler (elementwise)
 * DDIM update with x0-prediction, eta = 0:
 *   eps = (c_recip * x - x0) / c_recipm1 ;  x_out = x0 * c_a + c_b * eps
 * Forward step: c_a = sqrt(abar_prev), c_b = sqrt(1 - abar_prev)
 *   (gaussian_diffusion.py:693-697 `_predict_eps_from_xstart`, :981-1001 `ddim_sample`).
 * Inversion step: c_a = sqrt(abar_next), c_b = sqrt(1 - abar_next)
 *   (gaussian_diffusion.py:1003-1040 `ddim_reverse_sample`).
 * Coefficients are the reference's fp64 tables cast to fp32 by the host.
 * x_out may alias x.  n = number of floats. */
int rg_ddim_update(rg_handle* h, const float* x, const float* x0, float* x_out, int64_t n,
                   float c_recip, float c_recipm1, float c_a, float c_b, void* stream);

/* Classifier-free mix of the denoiser head output followed by the DDIM update, fused:
 *   x0[b,t,:] = js[t]*w_c*out[b,t,:] + (1/js[t])*w_u*out[B+b,t,:]
 *   (raggesture.py:1086-1111 `forward_test` CFG mix; w_c = both+text, w_u = retr+none)
 * then rg_ddim_update on x0.  out is [2B,T,D] (cond rows first), x/x_out [B,T,D],
 * js = per_joint_scale mask [T].  x0_out may be NULL. */
int rg_cfg_ddim_update(rg_handle* h, const float* out, const float* x, float* x_out, float* x0_out,
                       const float* js, int B, int T, int D, float w_c, float w_u,
                       float c_recip, float c_recipm1, float c_a, float c_b, void* stream);
/* The same on a sub-range of a batch: out_cond / out_uncond point at the conditional and the classifier-free rows of the
 * same B clips (they are not B*T*D apart when the denoiser batch holds more sequences); x_out2 (may be NULL) receives a
 * second copy of the updated latent (the inversion stores every level and keeps the working rows in place). */
int rg_cfg_ddim_update_rows(rg_handle* h, const float* out_cond, const float* out_uncond, const float* x, float* x_out,
                            float* x_out2, const float* js, int B, int T, int D, float w_c, float w_u,
                            float c_recip, float c_recipm1, float c_a, float c_b, void* stream);

/* The same CFG mix followed by one ancestral (DDPM) step, `inference_type="ddpm"`:
 *   x_out = (c1 * x0 + c2 * x) + sigma * noise
 *   (gaussian_diffusion.py:479-501 `q_posterior_mean_variance` with model_mean_type START_X, :560-570 fixed_large
 *   variance, :795-803 `p_sample`: sigma = exp(0.5 * log_variance), 0 at the last step).  x_out may alias x. */
int rg_cfg_ddpm_update(rg_handle* h, const float* out, const float* x, const float* noise, float* x_out,
                       const float* js, int B, int T, int D, float w_c, float w_u, float c1, float c2, float sigma,
                       void* stream);

/* Everything between two denoiser forwards of a chain that advances a sampling loop (group a: n_a clips) and an inversion
 * loop (group b: n_b clips) in the same launches, in ONE launch: group a: rg_cfg_ddim_update_rows of this step, then -- for the
 * NEXT step, on the rows in_seq_next marks -- rg_guidance_update (g_iter_next iterations, numel = n_a * T * D) and
 * rg_inseq_replace; group b: rg_cfg_ddim_update_rows with its own coefficients and a second copy of the result.  The same
 * arithmetic as those entry points, operation for operation (gaussian_diffusion.py:910-1001 `ddim_sample`, :1003-1040
 * `ddim_reverse_sample`, :1263-1273, :1351-1378 guidance). */
typedef struct rg_glue_args {
  const float* out_c_a;    /* denoiser output, conditional rows of group a [n_a][T][D] */
  const float* out_u_a;    /* ... classifier-free rows of group a */
  float* x_a;              /* latent of group a, updated in place */
  const float* out_c_b;
  const float* out_u_b;
  float* x_b;              /* latent of group b, updated in place */
  float* x_b_copy;         /* or NULL: second copy of group b's result (the inversion level kept) */
  const float* in_seq_next;   /* or NULL: the next step's in_seq of group a [n_a][T][D] */
  const float* noise_next;    /* its randn_like(in_seq) draw */
  const float* js;         /* per_joint_scale [T] */
  int n_a, n_b, T, D;
  int g_iter_next;         /* insertion-guidance iterations of the next step (0: none) */
  float wc_a, wu_a, c_recip_a, c_recipm1_a, ca_a, cb_a;   /* CFG weights and DDIM coefficients of group a's step */
  float wc_b, wu_b, c_recip_b, c_recipm1_b, ca_b, cb_b;   /* ... of group b's */
  float lr, s_ab_next, s_1mab_next;
} rg_glue_args;
int rg_cobatch_glue(rg_handle* h, const rg_glue_args* args_host, void* stream);

/* In-sequence replacement (outpainting / exemplar insertion / prev-latent chaining):
 *   m[r] = any(in_seq[r,:] != 0);  x[r,:] = m ? s_ab*in_seq[r,:] + s_1mab*noise[r,:] : x[r,:]
 *   (gaussian_diffusion.py:934-947 in `ddim_sample`, :459-477 `q_sample`).  rows = B*T. */
int rg_inseq_replace(rg_handle* h, float* x, const float* in_seq, const float* noise,
                     int rows, int dim, float s_ab, float s_1mab, void* stream);

/* Insertion-guidance update: g_iter gradient steps on mse(x*m, in_seq) w.r.t. x,
 *   x <- x - lr * (2/numel) * ((x*m - in_seq) * m),  m as above, numel = rows*dim
 *   (gaussian_diffusion.py:1263-1273 `retrieval_guidance`, :1351-1378 the autograd loop). */
int rg_guidance_update(rg_handle* h, float* x, const float* in_seq, int rows, int dim,
                       int g_iter, float lr, void* stream);

/* All exemplar splices of a batch in one launch: for entry i, rows [r0, r0 + nrows) of exemplar e (upper block and hands
 * block, row offset n_lat + 1) of inv [S][Ep][T][D] go into rows [q0, q0 + nrows) of clip b -- level `lvl` into start_noise
 * [B][T][D] (rg_splice_rows) and, when invl [S][B][T][D] is given, every level into it (rg_splice_rows_rep)
 * (diffusion_architecture.py:386-407).  The entries' destinations do not overlap (raggesture.py:703-731 de-overlaps them). */
#define RG_SPLICE_MAX 64
typedef struct rg_splice_table {
  int n;
  int e[RG_SPLICE_MAX], b[RG_SPLICE_MAX], r0[RG_SPLICE_MAX], q0[RG_SPLICE_MAX], nrows[RG_SPLICE_MAX];
} rg_splice_table;
int rg_splice_many(rg_handle* h, const rg_splice_table* tab_host, const float* inv, float* start_noise, float* invl,
                   int T, int D, int n_lat, int lvl, int S, int Ep, int B, void* stream);

/* Exemplar splice: copy token rows [r0,r1) of src[b_src] into rows [q0,q1) of dst[b_dst]
 * for the upper block and the hands block (row offset n_lat+1)
 *   (diffusion_architecture.py:386-407).  src/dst are [*,T,D]. */
int rg_splice_rows(rg_handle* h, const float* src, float* dst, int T, int D, int n_lat,
                   int b_src, int b_dst, int r0, int r1, int q0, int q1, void* stream);
/* The same splice repeated for nrep (diffusion level) slabs: slab s reads batch item
 * b_src + s*src_rep_stride and writes b_dst + s*dst_rep_stride (the 50 per-timestep inverted
 * latents, diffusion_architecture.py:399-407). */
int rg_splice_rows_rep(rg_handle* h, const float* src, float* dst, int T, int D, int n_lat,
                       int b_src, int b_dst, int r0, int r1, int q0, int q1, int nrep,
                       int src_rep_stride, int dst_rep_stride, void* stream);

/* ---------------------------------------------------------------- fused bf16-MFMA GEMM
 * out[M,N] = epilogue( A'[M,K] * W[N,K]^T ), bf16 operands, fp32 accumulate (MFMA 16x16x32).
 * It replaces every nn.Linear on the hot path together with the elementwise ops around it:
 *   A' can be built on the fly from fp32 sources: identity cast, LayerNorm
 *   (efficient_attention.py:29,31,36,72-74 `self.norm(x)`), or the StylizationBlock front half
 *   LN -> *(1+scale)+shift -> SiLU (stylization_block.py:36-39);
 *   the epilogue adds bias / a token-periodic table (positional embeddings,
 *   diffusion_transformer.py:646-659) / a residual (efficient_attention.py:44,100;
 *   diffusion_transformer.py:86), applies GELU (diffusion_transformer.py:85) or the per-head
 *   softmax over head_dim=32 of the queries (efficient_attention.py:32,78), and can emit
 *   per-row partial (sum, sumsq) so the consumer's LayerNorm needs no extra pass.
 * The descriptor is a HOST struct read at call time. */

#define RG_MAX_SEG 4

// A-operand transforms applied while an fp32 source tile is staged into LDS as bf16
enum { RG_A_IDENT = 0, RG_A_LN = 1, RG_A_STYL = 2 };

typedef struct rg_a_segment {
  const float* src;    // fp32 source, row-major
  int ld;              // row stride of src (floats)
  int mode;            // RG_A_IDENT / RG_A_LN / RG_A_STYL
  const float* stats;  // [rows][nparts][2] partial (sum, sumsq) over the segment's seg_len columns
  int nparts;
  int pad_;
  const float* gamma;  // [seg_len] LayerNorm weight (LN, STYL)
  const float* beta;   // [seg_len] LayerNorm bias
  const float* scale_shift;  // STYL: [2*seg_len] = AdaLN scale | shift for this (step, layer, block)
} rg_a_segment;

typedef struct rg_gemm_desc {
  int M, N, K;
  int a_is_bf16;          // 1: A is bf16 [M, lda] (nseg = 0; or nseg = 1 with seg[0].mode = RG_A_STYL: the rows are the
                          //    bf16 copy of a block output y and the operand is SiLU((y - mean) * rstd * gain + offset):
                          //    the StylizationBlock front half with gain = gamma (1 + scale), offset = beta (1 + scale)
                          //    + shift folded by the caller into seg[0].gamma / .beta (16-byte aligned, K floats each;
                          //    .scale_shift NULL, .src unused) and mean / rstd from seg[0].stats; applied once per
                          //    element in LDS by the LDS-DMA kernel: K <= 512, K % 64 == 0); 0: fp32 segments
  const void* A;          // bf16 A (a_is_bf16): lda % 8 == 0 and K % 8 == 0 (staged in 16-byte chunks of 8 columns)
  int lda;
  int a_row_mod;          // >0: A row index = row % a_row_mod (row-duplicating GEMMs)
  int seg_len;            // K columns per fp32 segment (K = nseg * seg_len, last may be short)
  int nseg;
  rg_a_segment seg[RG_MAX_SEG];
  int gb_group;           // >0: column tiles [g*gb_group, (g+1)*gb_group) form group g: gamma/beta of every fp32
  int gb_stride;          //     segment, or the bf16 A pointer, are offset by g * gb_stride elements (several
                          //     projections of differently normalised copies of the same rows in one launch)
  const void* W;          // bf16 [Np, ldw]  (rows = output features, K contiguous, zero padded)
  int ldw;
  int act;                // 0 none, 1 GELU(erf), 2 ReLU
  const float* bias;      // [N] or null
  const float* tbias;     // [tb_period, N] or null: + tbias[(row % tb_period) * N + col]
  int tb_period;          //   required > 0 with tbias
  int softmax_cols;       // columns [0, softmax_cols) get a softmax over each group of 32 columns; a multiple of 32, <= N
  const float* residual;  // fp32 [M, ldr] or null
  int ldr;
  int out_bf16;           // 1: out is bf16, 0: fp32
  void* out;
  int ldo;
  int ldo2;               // row stride (elements) of out2
  float* stats_out;       // null, or [M][ceil(N / tile)][2] partial (sum, sumsq) of the final fp32 output, one pair per
                          // column tile: tile = 128 columns, or 64 with tile_n = 64 (a ragged last tile sums its columns < N)
  const void* W_lo;       // null, or bf16 [Np, ldw] = bf16(W - float(bf16(W))): selects the precise
                          // "bf16x3" mode (hi*hi + hi*lo + lo*hi), fp32 A segments only
  void* out2;             // null, or bf16 [M, ldo2]: a second, bf16-rounded copy of the output (the next
                          // GEMM's A operand, written by the producer instead of converted by every consumer tile)
  const float* ln_stats;  // null, or [M][ln_nparts][2] partial (sum, sumsq) of the fp32 rows whose bf16 copy is A:
  const float* ln_c1;     //   LayerNorm folded into the epilogue.  With W' = W diag(gamma) packed as the weight,
  int ln_nparts;          //   c1[n] = sum_k W'[n][k] and bias[n] = b[n] + sum_k W[n][k] beta[k]:
  int split_col;          //   out = rstd * (A W'^T - mean * c1) + bias  ==  LN(x) W^T + b   (mean/rstd over K columns)
                          //   ln_stats requires ln_c1 ([N]) and ln_nparts > 0 (more than 8 partials take a scalar loop)
                          // split_col > 0: output columns >= split_col go ONLY to out2 (bf16, column index - split_col),
                          // columns below it only to out: a GEMM with an fp32 and a bf16 consumer.  Requires out2,
                          // split_col % 128 == 0 and 0 < split_col < N; 0 = no split (negative values are rejected)
  int tile_n;             // 0 / 128: default tile width; 64: 64x64 tiles (bf16 A, aligned shapes only): more, smaller
  int pad4_;              //   workgroups for single-round GEMMs; stats_out then holds N/64 partials per row
} rg_gemm_desc;

int rg_gemm(rg_handle* h, const rg_gemm_desc* desc_host, void* stream);
/* n GEMMs that share a shape signature (M, N, K, operand kinds, epilogue features) in one launch: descriptor i belongs to
 * the workgroups with blockIdx.y = i (the four body-part VAEs run the same layer on different weights: 4x fewer dependent
 * launches in the front end, which is what it costs beside running denoiser chains).  descs_host: array of n descriptors;
 * groups that do not share a signature, or n > 4, are launched one by one.  Same result bits as n rg_gemm calls. */
int rg_gemm_grouped(rg_handle* h, const rg_gemm_desc* descs_host, int n, void* stream);

/* The A-operand prologue of rg_gemm as a standalone pass: out[row, s*seg_len + k] =
 * bf16(f_s(src_s[row,k])) for nseg fp32 segments (identity / LayerNorm / stylization front half,
 * same rg_a_segment descriptors, HOST array).  Used in front of the K = 4*512 ca_mix GEMM so the
 * SiLU prologue runs once per element instead of once per column tile.
 * Rows [m_cond, M) are the classifier-free rows: for the first unc_nseg segments they copy
 * unc_tab[flag][s*seg_len + k] (bf16; flag = 1 where qmask[s][row] == 0) instead of reading the source:
 * with cond_type 0 the cross-attention output is the value bias for every token
 * (efficient_attention.py:83-90), so its stylized form depends on the weights and the
 * timestep only and is tabulated at load time.  m_cond = M disables this. */
int rg_stylize(rg_handle* h, const rg_a_segment* segs_host, int nseg, int seg_len, int M, void* out_bf16, int ldo,
               int m_cond, int unc_nseg, const void* unc_tab_bf16, const float* qmask, void* stream);
/* rg_stylize for a batch whose sequences sit at TWO diffusion steps (the sampling rows of one batch of clips and the
 * inversion rows of the next batch's exemplars in the same launches): rows are [2 CFG halves][nseq sequences][T tokens];
 * sequences >= split of either half take their (scale | shift) from scale_shift_b_host[s] (HOST array of nseg device
 * pointers) instead of segs[s].scale_shift.  split >= nseq: one group, as rg_stylize. */
int rg_stylize_groups(rg_handle* h, const rg_a_segment* segs_host, int nseg, int seg_len, int M, void* out_bf16, int ldo,
                      int m_cond, int unc_nseg, const void* unc_tab_bf16, const float* qmask,
                      const float* const* scale_shift_b_host, int T, int nseq, int split, void* stream);

/* Kernel selection hook for tests / tuning: 0 = auto, 1 = generic register-staged kernel only (any
 * shape), 2 = prefer the LDS-DMA ring kernel, 3 = prefer the depth-4 register-staged kernel, 4 = prefer the
 * 128-row big-tile kernel (bf16 A; 128 x 256 tiles), 5 = never use it, 6 = prefer it with 128 x 128 tiles,
 * 7 = 128 x 128 tiles on a ring of 2 at two workgroups per CU. */
int rg_set_gemm_path(rg_handle* h, int path);
/* Tuning knob of this handle: waves per workgroup of the LDS-DMA GEMM kernel (0 = auto by shape, 4 or 8; default 0). */
int rg_set_gemm_waves(rg_handle* h, int waves);

/* Measurement aid (bench.py roofline): between begin and end every rg_gemm launch is bracketed by
 * HIP events on its stream; end synchronises and returns launch count, summed kernel time and summed
 * algorithmic FLOPs (2*M*N*K) for one kernel variant (0: fp32-source A, 1: bf16 A, 2: bf16x3; 3: rg_seq_forward
 * launches, FLOPs = the unit GEMMs and attention products of the T token rows of every sequence). */
int rg_profile_begin(rg_handle* h);
int rg_profile_end(rg_handle* h, int variant, int64_t* launches_host, double* total_ms_host,
                   double* total_flops_host);

/* out[i,:] = table[idx[i],:]  (nn.Embedding lookup of speaker ids, diffusion_transformer.py:544-548).
 * idx is int64 on device; dim % 4 == 0. */
int rg_gather_rows(rg_handle* h, const float* table, const int64_t* idx, float* out, int n, int dim,
                   void* stream);

/* ---------------------------------------------------------------- linear attention
 * Self-attention core of EfficientSelfAttention (efficient_attention.py:32-41) for R batch rows
 * of T tokens: qkv is [R*T, ldqkv] fp32 with q (already softmaxed over head_dim by the GEMM
 * epilogue) in columns [0,D), k in [D,2D), v in [2D,3D); src_mask [R,T] (0 = masked token:
 * `key + (1-mask)*-1e6` and `value*mask`).  Writes y [R*T, ldy] fp32 and per-row partial
 * LayerNorm statistics stats[R*T][D/128][2] (sum, sumsq over each 128-column head group).
 * perm (device, nperm ints, or NULL): launch order -> work item (row * D/128 + head group, -1 = idle
 * block); lets the caller place a row group on the XCD whose L2 already holds its rows.
 * mode 1: P^T V and Q A on the matrix cores (bf16 hi + lo operand pairs, fp32 accumulate: the bf16
 * production path); 0: exact fp32 VALU products (precision = "fp32"); 2: as 1 and y leaves as bf16 [R*T, ldy]
 * (T <= 48): the A operand of the SA-out GEMM, which applies the stylization in LDS (rg_gemm_desc.seg). */
int rg_sa_attention(rg_handle* h, const float* qkv, int ldqkv, const float* src_mask, void* y, int ldy,
                    float* stats, int R, int T, int D, const int* perm, int nperm, int mode, void* stream);

/* Cross-attention core of EfficientCrossAttention for ncond parallel conditions
 * (efficient_attention.py:90-98; diffusion_transformer.py:105-118): y3[:, c*D:(c+1)*D] = Q_c A_c
 * with Q_c = q3[:, c*D:(c+1)*D] (softmaxed), A_c = Apre[c][row] ([H][32][32], from rg_kv_reduce) for
 * rows < Rc and Aunc[c] for the classifier-free rows [Rc,R) (cond_type 0: V = value(0) = bias, so
 * A[d][l] = b_v[l]; efficient_attention.py:83-90).
 * qmask [ncond][R][T] or NULL: where 0, y is rounded exactly as the reference's fp32
 * `y + (1-query_mask)*-1e6` rounds it (grid 1/16) so that the following LayerNorm sees the
 * same values up to the shift.  stats layout [ncond][R*T][D/128][2].
 * perm as for rg_sa_attention; work item = (row * ncond + cond) * D/128 + head group. */
int rg_ca_attention(rg_handle* h, const float* q3, const float* Apre, const float* Aunc, const float* qmask,
                    float* y3, float* stats, int R, int Rc, int T, int D, int ncond, const int* perm, int nperm,
                    void* stream);

/* rg_ca_attention + the stylization front half (StylizationBlock: LN, *(1+scale)+shift, SiLU;
 * stylization_block.py:30-47) of the three cross-attention outputs in one launch, one workgroup per
 * (conditional row group, condition): out[b*T+n][c*D + col] (bf16, row stride ldo) for the Rc conditional
 * row groups (y = Q A on the matrix cores, Q and A as bf16 hi + lo pairs: At_bf16 = rg_split_transpose_bf16 of
 * the rg_kv_reduce output, [ncond][Rc][H][2][32][32]); the Ru classifier-free row groups [Rc, Rc+Ru) receive unc_tab[flag][0 .. ncond*D) (flag = 1
 * where qmask == 0), see rg_stylize.  q3 holds the conditional rows only ([Rc*T][ncond*D]);
 * qmask is [ncond][Rc+Ru][T] or NULL; gamma/beta [ncond][D]; scale_shift [ncond][2*D]. */
int rg_ca_stylize(rg_handle* h, const float* q3, const void* At_bf16, const float* qmask, const float* gamma,
                  const float* beta, const float* scale_shift, const void* unc_tab_bf16, void* out_bf16, int ldo,
                  int Rc, int Ru, int T, int D, int ncond, void* stream);
/* The same for two groups of sequences at different diffusion steps: row groups >= split of the conditional rows take
 * scale_shift_b, those >= split of the classifier-free rows unc_tab_b (see rg_stylize_groups). */
int rg_ca_stylize_groups(rg_handle* h, const float* q3, const void* At_bf16, const float* qmask, const float* gamma,
                         const float* beta, const float* scale_shift, const void* unc_tab_bf16, void* out_bf16, int ldo,
                         int Rc, int Ru, int T, int D, int ncond, const float* scale_shift_b, const void* unc_tab_b_bf16,
                         int split, void* stream);

/* At[m] = (bf16(A[m]^T), bf16(A[m]^T - hi)) for n_mat fp32 32x32 matrices: the B-operand layout rg_ca_stylize reads. */
int rg_split_transpose_bf16(rg_handle* h, const float* A, void* At_bf16, int n_mat, void* stream);

/* A[b][h] = softmax_over_tokens(K[b,:,h,:])^T V[b,:,h,:]  (efficient_attention.py:82-90) for B rows
 * of N conditioning tokens; kv is [B*N, ldkv] fp32 with k in columns [0,D) and v in [D,2D).
 * A is [B][H][32][32].  Loop invariant over the 50 DDIM steps: run once per clip. */
int rg_kv_reduce(rg_handle* h, const float* kv, int ldkv, float* A, int B, int N, int D, void* stream);

/* Partial LayerNorm statistics of fp32 rows that no GEMM produced (the gathered speaker
 * embeddings): stats[row][dim/64][2] = (sum, sumsq) over each 64-column part. */
int rg_row_stats(rg_handle* h, const float* x, float* stats, int rows, int dim, void* stream);

/* Guard of the folded LayerNorm (rg_gemm_desc.ln_stats): *max_ratio = max(*max_ratio, max over rows of mean^2 / var)
 * from the partial (sum, sumsq) statistics [rows][nparts][2] of K-wide rows.  *max_ratio must hold a non-negative
 * float (zero it first).  The folded form multiplies bf16(x) with x un-normalised: its error grows with |mean| / std
 * (efficient_attention.py:29,72-74 normalise first); the host reads the figure once per session and uses the
 * LayerNorm pre-pass instead when it is large. */
int rg_ln_guard(rg_handle* h, const float* stats, int rows, int nparts, int K, float* max_ratio, void* stream);

/* Exact fp32 linear for load-time tables: out[M,N] = f_out( f_in(a)[M,K] w[N,K]^T + bias ),
 * f = SiLU if the flag is set (time_embed MLP, diffusion_transformer.py:404-408, and the 40
 * StylizationBlock emb_layers, stylization_block.py:35, which depend only on the timestep). */
int rg_linear_f32(rg_handle* h, const float* a, const float* w, const float* bias, float* out, int M,
                  int N, int K, int silu_in, int silu_out, void* stream);

/* Condition side of the efficient cross attention, one launch per condition (csrc/rg_condkv.hip): for every clip b, layer l and
 * head h,  A[l][b][h] = softmax_tokens(K_h)^T V_h  with  [K | V] = xhat_b W_l^T + bias_l
 * (mogen/models/attentions/efficient_attention.py:74-90; xhat = the condition rows after the LayerNorm WITHOUT its affine,
 * which is folded into W / bias: LN_l(x) W_l^T + b_l = xhat (W_l diag(gamma_l))^T + (b_l + W_l beta_l)).
 * xhat bf16 [B][n_tok][512], w bf16 [L][1024 = key 512 | value 512][512], bias fp32 [L][1024]; out fp32: the A matrices of
 * (layer 0, clip 0), [16 heads][32][32] per clip, layer l at out + l * layer_stride.  n_tok <= 512, 16 heads of 32.
 * afrag_bf16 (or NULL): the same matrices once more as rg_seq_args.afrag of (layer 0, this condition, clip 0) -- bf16 MFMA
 * A-operand fragments [8][2 heads][2 column blocks][64 lanes][8] per clip, layer l at + l * afrag_layer_stride elements.
 * Replaces rg_gemm (K | V of two layers as fp32 [rows][2048]) + rg_kv_reduce per layer: nothing but A is written. */
int rg_cond_kv(rg_handle* h, const void* xhat_bf16, const void* w_bf16, const float* bias, float* out, long long layer_stride,
               void* afrag_bf16, long long afrag_layer_stride, int B, int n_tok, int L, void* stream);

/* ---------------------------------------------------------------- one denoiser forward, sequence-stationary
 * ReGestureTransformer.forward at inference (raggesture.py:1041-1085 `forward_test` up to the CFG mix,
 * diffusion_transformer.py:620-668, :105-127 `DecoderLayer`, :74-87 `FFN`, efficient_attention.py:23-45, 62-102,
 * stylization_block.py:29-40) in ONE launch of 2B workgroups: workgroup s owns sequence s (T <= 48 token rows; the B
 * conditional sequences first, then the B classifier-free ones) from the joint embedding to the output head.  The fp32
 * residual stream stays in registers, the bf16 MFMA operand panels in LDS; the only memory traffic is the weight stream,
 * which every wave fetches for itself by LDS-DMA in the order it consumes it (csrc/rg_seq.hip).  D = 512, 16 heads x 32,
 * FF = 1024, L <= 8, bf16 operands / fp32 accumulate, LayerNorm statistics exact in fp32.
 * Streams (DEVICE, built once per model / per clip batch by the host, rag-gesture_amd/seqfwd.py):
 *   wstream  bf16  [NU][8 waves][64][1 KiB]   NU = 16 L + 2 unit GEMMs of 512 x 512 (embed; per layer k, v, q, sa_out,
 *            mix_x, (q3_c, mix_c) x 3, ff1_0, ff2_0, ff1_1, ff2_1, ffn_out; head).  Fragment (wave w, step s, block j) is
 *            the MFMA operand image of W[64 w + 16 j + (lane & 15)][32 s + 8 (lane >> 4) + e], e = 0..7.  LayerNorm gains
 *            are folded into the k / v / q / q3 weights (W diag(gamma)), their betas into the biases.
 *   pstream  fp32  [S][NU][8][4][64]          per step and unit, for the wave's 64 features: vector 0 = bias, 1 / 2 =
 *            stylization gain gamma (1 + scale) / offset beta (1 + scale) + shift of the block the unit feeds
 *            (mix_x: vector 1 = row sums of the bf16 weight, for the un-normalised x segment).
 *   ustream  fp32  [S][L][8][2 KiB]           classifier-free sequences: sum_k W_mix_c[n][k] * unc_tab[flag][c][k] for
 *            (c, flag) = (0,0) (0,1) (1,0) (1,1) | (2,0) (2,1): their cross-attention output is a constant of (step, layer).
 *   afrag    bf16  [L][3][B][8][2 heads][2 column blocks][64 lanes][8]   A = softmax_N(K)^T V of every clip,
 *            condition and head (rg_kv_reduce) as MFMA A-operand fragments: element e of lane (jj, g) is
 *            A[i][16 jb + jj], i = e < 4 ? 4 g + e : 16 + 4 g + e - 4.
 * Clips >= split run at step index step_b (two diffusion loops sharing the launch: sampler.cobatched_loop).
 * dump / dump_stage: diagnostics (stage 1: after the embedding; 2 / 3 / 4: after the self-attention / cross-attention /
 * FFN block of layer dump_layer; 10: self-attention output y; 11-13: cross-attention y of condition 0-2), the T-layout
 * registers go to dump [2B][48][512] and the workgroup exits.
 * Unit slots of a layer in wstream / pstream: layer l's unit u is unit 1 + RG_SEQ_UPL l + u of the stream (unit 0 = the
 * embedding, the last = the head).  The ONE definition: the kernels walk the streams by these, rag-gesture_amd/seqfwd.py packs
 * them by these.  KV is a double unit (key | value: slots KV and KV2), its parameter fragment carries both biases. */
#define RG_SEQ_UPL 16
#define RG_SEQ_U_KV 0
#define RG_SEQ_U_KV2 1
#define RG_SEQ_U_Q 2
#define RG_SEQ_U_SAO 3
#define RG_SEQ_U_MIXX 4
#define RG_SEQ_U_Q3_0 5
#define RG_SEQ_U_MIX_0 6
#define RG_SEQ_U_Q3_1 7
#define RG_SEQ_U_MIX_1 8
#define RG_SEQ_U_Q3_2 9
#define RG_SEQ_U_MIX_2 10
#define RG_SEQ_U_FF1_0 11
#define RG_SEQ_U_FF2_0 12
#define RG_SEQ_U_FF1_1 13
#define RG_SEQ_U_FF2_1 14
#define RG_SEQ_U_FFO 15
typedef struct rg_seq_args {
  const void* wstream;
  const void* pstream;
  const void* ustream;
  const void* afrag;
  const float* x;          /* fp32 [B][T][512] latent at this step */
  const float* tbias;      /* fp32 [T][512] positional tables */
  const float* src_mask;   /* fp32 [2B][T] */
  const float* qmask;      /* fp32 [3][2B][T] */
  float* head;             /* fp32 [2B][T][512] result */
  float* dump;
  float* xbuf;             /* rg_seq2_forward: fp32 [workgroups][2][8][12][64][4] round trips of the two sequences' tiles; rg_seq_forward: unused */
  void* gbuf;              /* rg_seq2_forward: bf16 [workgroups][4][2][48 KiB] panel images; rg_seq_forward: unused */
  int L, B, T, S;          /* layers, clips, tokens, steps in pstream / ustream */
  int step, step_b, split; /* clips [0, split) at step, clips [split, B) at step_b */
  int dump_stage, dump_layer;
  int pairs;               /* 0: one workgroup per sequence (2 B workgroups); 1: one workgroup per clip runs the conditional
                              sequence, then its classifier-free twin (B workgroups, 1.7x as long: less CU time per forward,
                              for callers that run several narrow launches side by side) -- same results bit for bit */
  int twin;                /* rg_seq2_forward only, 0 or 1, not together with pairs.  1: workgroup b runs clip b -- its conditional
                              sequence and its classifier-free twin TOGETHER (B workgroups): the units both kinds run feed both
                              sequences from one weight fragment, the cross-attention units the conditional one alone, so all
                              workgroups of a launch do the same work and end together; with glue_ctr the workgroup updates
                              its clip itself and leaves the counters alone -- same results bit for bit.  rg_seq_forward
                              ignores it */
  int* glue_ctr;           /* or NULL.  DEVICE int [B], zero-initialised once by the caller and then left to the launches: with
                              it, the forward ends with what rg_cobatch_glue does between two forwards of a loop (`glue` below;
                              n_a + n_b == B, n_b may be 0; its out_* pointers are rows of `head`, its x_* rows of `x`) -- the
                              workgroup that finishes the second of a clip's two sequences updates that clip's rows, so a loop
                              step is ONE launch (csrc/rg_tail.h).  Same arithmetic, operation for operation. */
  rg_glue_args glue;
} rg_seq_args;

int rg_seq_forward(rg_handle* h, const rg_seq_args* args_host, void* stream);
int rg_seq2_forward(rg_handle* h, const rg_seq_args* args_host, void* stream);

/* rg_seq_forward for n sessions (1 <= n <= RG_SEQ_MANY_MAX) in ONE launch of sum(2 B_i) workgroups: workgroups [first_i,
 * first_i + 2 B_i) run session i's sequences exactly as rg_seq_forward(args[i]) would -- same bits, tail (glue_ctr) included,
 * every session with its own B, split, step, step_b, x, afrag, head, masks, glue_ctr and glue.  For independent chains that
 * are ready at the same moment (a pipeline's pending sampling loops when it drains): a launch of this kernel takes about
 * the same time for any number of workgroups up to one per compute unit, so n loops advance in the time of one.  L, T, S
 * and wstream / pstream / ustream must be the same for all sessions; only the one-workgroup-per-sequence form is accepted
 * (pairs == 0, twin == 0, dump_stage == 0).  The sessions' buffers must not overlap. */
#define RG_SEQ_MANY_MAX 8
int rg_seq_forward_many(rg_handle* h, const rg_seq_args* const* args_host, int n, void* stream);

/* rg_seq2_forward in its twin form for n sessions (1 <= n <= RG_SEQ_MANY_MAX) in ONE launch of sum(B_i) workgroups: workgroup
 * first_i + c runs clip c of session i -- its conditional sequence and its classifier-free twin -- exactly as
 * rg_seq2_forward(args[i]) with twin == 1 would: same bits, tail (glue_ctr) included, the counters left alone; every session
 * with its own B, split, step, step_b, x, afrag, head, masks, xbuf, gbuf and glue.  For the co-batched chains of a pipeline's
 * lanes, which are ready together once per rotation: four chains of 64 workgroups fill the chip from one stream.  Every
 * session must have twin == 1, pairs == 0 and dump_stage == 0; L, T, S and wstream / pstream / ustream must be the same for
 * all.  n == 1 is rg_seq2_forward.  The sessions' buffers must not overlap. */
int rg_seq2_forward_many(rg_handle* h, const rg_seq_args* const* args_host, int n, void* stream);

/* Sequence-stationary body-part VAE encoder: the whole skip-transformer stack of `TransformerVAE.encode_to_dist`
 * (mogen/models/transformers/gesture_vae.py:111-193: chunk sequences of frame_chunk_size frames + the two distribution
 * tokens; mogen/models/utils/detr_utils.py:101-152 SkipTransformerEncoder, :335-393 TransformerEncoderLayer.forward_post with
 * torch.nn.MultiheadAttention) in ONE launch, one workgroup per two chunk sequences; replaces the per-op launch chain
 * (rg_gemm / rg_mha_bf16 / rg_layernorm) for the shape it is specialised for: latent_dim 512, 4 heads, ff_size 1024, GELU,
 * post-norm, S <= 24 tokens, bf16 operands with fp32 accumulation, fp32 residual stream / LayerNorm / softmax.
 *   x       fp32 [nseq][S][512]   the embedded sequences (skel_embedding + the distribution tokens + positional table)
 *   out     fp32 [nseq][S][512]   encoder output behind the final LayerNorm (rows 0 / 1 = mu / logvar: rg_vae_reparam)
 *   wstream bf16 [NU][8 waves][64 fragments][64 lanes][8]   unit GEMMs (512 x 512) in consumption order, per block:
 *           [skip W[:, :D], skip W[:, D:]] (output blocks only), Q (x 1/sqrt(128)), K, V, out_proj, linear1[:512],
 *           linear2[:, :512], linear1[512:], linear2[:, 512:];  NU = 8 (2 nb + 1) + 2 nb
 *   pstream fp32 [NU + 1][8 waves][4][64]   per unit: vector 0 = bias (zero for the second half of a split unit), vectors
 *           1 / 2 = gamma / beta of the LayerNorm that follows the unit (out_proj: norm1, linear2 first half: norm2);
 *           slot NU: vectors 0 / 1 = gamma / beta of the encoder's final norm
 *   xbuf    fp32 [ceil(nseq / 2)][nb][8][12][64][4]   the skip stack (states behind the input blocks)
 *   nb      input blocks = output blocks ((num_layers - 1) / 2 for odd num_layers, num_layers / 2 for even: detr_utils.py:108)
 *   dump / dump_block: diagnostics (state behind block dump_block as fp32 [workgroup][48][512]); dump_block < 0: off.
 * Posterior-only store (post_rows != NULL; `out` is then not written and may be NULL): of every sequence only token rows 0 / 1
 * (mu / logvar) are stored, the same bits `out` would hold, straight into the rows of an exemplar posterior cache:
 *   post_rows   int32 [nseq] (device)   destination row of sequence i; < 0 (or >= post_nrows): store nothing (padding)
 *   post_mu / post_logvar   fp32 [post_nrows][512]   row post_rows[i] receives token row 0 / 1 of sequence i. */
typedef struct rg_venc_args {
  const void* wstream;
  const void* pstream;
  const float* x;
  float* out;
  float* xbuf;
  float* dump;
  int nseq, S, nb, dump_block;
  const int* post_rows;
  float* post_mu;
  float* post_logvar;
  int post_nrows, pad_;
} rg_venc_args;

int rg_venc_forward(rg_handle* h, const rg_venc_args* args_host, void* stream);
/* n <= 4 independent stacks (the four body-part VAEs: different weights, inputs and widths of nothing -- the stacks share D = 512)
 * in ONE launch: args_host[n], gridDim.y = n. */
int rg_venc_forward_grouped(rg_handle* h, const rg_venc_args* args_host, int n, void* stream);

/* Block-fused body-part VAE decoder of the "all_encoder" architecture (mogen/models/transformers/gesture_vae.py:195-239
 * `decode`: the skip-transformer ENCODER stack over cat(z [10], zero queries [150]) = 160 tokens with pos = query_pos, i.e.
 * q = k = x + pos, v = x (detr_utils.py:335-393), num_heads * 8 = 32 heads of 16): one launch per block instead of nine,
 * a sequence cut into four tiles of 40 rows (one workgroup each), the tiles' keys / values exchanged through L2 between the
 * launches.  Launch `step` (0 .. 2 nb + 1) runs [attention, out_proj + norm1, FFN + norm2 of block step - 1] -> [skip push or
 * skip linear of block step] -> [Q, K, V of block step]; launch 0 only projects, the last one ends with the stack's final norm.
 * Same weight / parameter streams as rg_venc_forward (Q pre-scaled by 1/sqrt(16)); specialised for latent_dim 512, 4 x 8
 * heads, ff_size 1024, GELU, post-norm, 160 tokens, bf16 operands with fp32 accumulation.
 *   x    fp32 [nseq][160][512]   residual stream: the stack's input before step 0, its output (behind the final norm) after the
 *                                last step, updated in place by every launch
 *   pos  fp32 [nseq][160][512]   query_pos (constant over the blocks)
 *   qimg bf16 [4 nseq][48 KiB]   a tile's Q operand panel as it lies in LDS (handed from launch to launch): tile 4 seq + quarter as
 *                                [3 tb][16 s][4 gq][16 l][8 e] = Q[token 40 quarter + 16 tb + l][feature 32 s + 8 gq + e]; rows
 *                                16 tb + l >= 40 are padding (tests/test_vdec_stages_gpu.py decodes it)
 *   kbuf bf16 [2][nseq][160][512]   keys, row-major;   vt bf16 [2][nseq][512][160]   values, feature-major; both double-buffered
 *                                by launch parity (a launch's faster tiles write block `step`'s while slower ones still read
 *                                block step - 1's)
 *   xbuf fp32 [4 nseq][nb][8][12][64][4]   the skip stack;   dump: diagnostics (fp32 [4 nseq][48][512]: the state a launch starts
 *                                its projection part from) or NULL
 * The stack's own ends (each pointer may be NULL: x / pos are then read and x written as described above):
 *   latent fp32 [nseq][lat_T][512]   launch 0 builds its x rows itself: token t < n_lat = latent row lat_row0 + t of the clip,
 *                                the 160 - n_lat frame queries = 0 (instead of reading x, which it still writes)
 *   table  fp32 [160][512]       launch 0 computes pos = x + table and WRITES it to pos for the later launches
 *   frames fp32 [nseq][160 - n_lat][512]   the last launch stores the frame rows (tokens >= n_lat) here, compactly, instead of
 *                                writing x */
typedef struct rg_vdec_args {
  const void* wstream;
  const void* pstream;
  float* x;
  const float* pos;
  void* qimg;
  void* kbuf;
  void* vt;
  float* xbuf;
  float* dump;
  int nseq, nb, step, pad_;
  const float* latent;
  const float* table;
  float* frames;
  int lat_T, lat_row0, n_lat, pad2_;
} rg_vdec_args;

int rg_vdec_step(rg_handle* h, const rg_vdec_args* args_host, void* stream);
int rg_vdec_step_grouped(rg_handle* h, const rg_vdec_args* args_host, int n, void* stream);

/* ---------------------------------------------------------------- body-part VAEs + rotations
 * Softmax multi-head attention core of torch.nn.MultiheadAttention for short sequences
 * (detr_utils.py:364-366, 427-433): o[b,i,h,:] = softmax_j(q[b,i,h,:].k[b,j,h,:]/sqrt(hd)) v[b,j,h,:].
 * q [B*Sq, ldq], k/v [B*Sk, ld], head h in columns [h*hd, (h+1)*hd); Sk <= 192 and K / V of one head in LDS:
 * 4 (Sk (2 hd + 5) + 4 hd) bytes <= 160 KiB (hd = 128: Sk <= 154; anything else is refused); no padding mask
 * (the reference always passes full-length clips, gesture_vae.py:124-160). */
int rg_mha(rg_handle* h, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o,
           int ldo, int B, int H, int Sq, int Sk, int hd, void* stream);
/* Same operation on the matrix cores for the bf16 path (K, V rounded to bf16, Q and the softmax
 * probabilities as bf16 hi + lo pairs, fp32 accumulation): hd in {16, 32, 64, 128}, Sk <= 192 (Sk <= 512 at hd = 64: wav2vec2 windows), row
 * strides multiples of 4 floats.  out_is_bf16 = 1: o is bf16 [B*Sq, ldo] (the A operand of the out-projection). */
int rg_mha_bf16(rg_handle* h, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, void* o, int ldo,
                int out_is_bf16, int B, int H, int Sq, int Sk, int hd, void* stream);

/* nn.LayerNorm(dim), eps 1e-5, fp32 rows (detr_utils.py norm1/norm2/norm3, encoder/decoder norm). */
int rg_layernorm(rg_handle* h, const float* x, const float* gamma, const float* beta, float* out, int rows, int dim,
                 void* out_bf16, void* stream);

/* LayerNorm(x + residual) with the caller's eps (residual may be NULL): the post-norm steps of the conditioning encoders
 * (BERT eps 1e-12, wav2vec2 1e-5; transformers BertSelfOutput / Wav2Vec2EncoderLayer).  out_bf16: optional bf16 copy. */
int rg_layernorm_res(rg_handle* h, const float* x, const float* residual, const float* gamma, const float* beta, float* out,
                     int rows, int dim, float eps, void* out_bf16, void* stream);

/* ---------------------------------------------------------------- conditioning feature extraction
 * tools/longform_synthesis.py:64-94 computes, per 10-second window, BERT-base-cased hidden states (sum of the last four
 * layers) of the window's transcript and the wav2vec2-base-960h last hidden state [499, 768] of its audio.  Both encoders
 * run on rg_gemm / rg_mha_bf16 / rg_layernorm_res (host: rag-gesture_amd/features.py); these are the remaining pieces:
 *   rg_embed_sum3: out[t] = word[ids[t]] + type0 + pos[t]  (BertEmbeddings before its LayerNorm; ids int64 on device)
 *   rg_time_groupnorm_gelu: x [T][C] fp32 -> GELU(GroupNorm_{groups = C}(x)) as bf16 and / or fp32 (either output may
 *     be NULL; normalisation over TIME per channel: layer 0 of the wav2vec2 feature extractor, feat_extract_norm =
 *     "group"); workspace: 2 * C floats
 *   rg_im2col_grouped: out[g][t][k * C/groups + ci] = x[t + k - pad][g * C/groups + ci] (zero outside [0, T)), bf16: the
 *     patch matrices of the positional convolution (Conv1d(768, 768, 128, padding 64, groups 16)), one GEMM per group. */
int rg_embed_sum3(rg_handle* h, const int64_t* ids, const float* word, const float* pos, const float* type0, float* out,
                  int L, int dim, void* stream);
int rg_time_groupnorm_gelu(rg_handle* h, const float* x, const float* gamma, const float* beta, void* out_bf16,
                           float* out_f32, int T, int C, float eps, float* workspace, void* stream);
int rg_im2col_grouped(rg_handle* h, const float* x, void* out_bf16, int T, int C, int groups, int ksize, int pad, void* stream);

/* The same encoders over MANY windows per call (features.py Wav2Vec2Features.batch / BertFeatures.batch; the reference calls
 * them one window at a time: mogen/datasets/beatx_dataset.py:823-832, 1171-1179, tools/longform_synthesis.py:64-94).  B audio
 * windows of one length share every launch.  The strided convolutions stay GEMMs over overlapping rows because every window
 * gets n_pad = P * ceil(n / P) samples (P = the product of the strides, 320) and layer i T_pad_i = n_pad / (5 * 2^i) rows: row
 * b * T_pad + t of a layer then starts at the right element of the previous one, and one GEMM with M = B * T_pad does a layer.
 * Rows t >= T_i of a window are junk: finite, never read by a valid row of the next layer, dropped at the end.
 *   rg_wave_normalize: Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm (transformers feature_extraction_wav2vec2.py) per
 *     window: out[b][i] = (x[b][i] - mean_b) / sqrt(var_b + 1e-7) for i < n, 0 for n <= i < n_pad; x [B][ldx], out [B][n_pad];
 *     var_b is the biased variance about the mean (two passes), the mean is taken about the window's first sample; fp32, fixed
 *     reduction order (one workgroup per window).  normalize = 0: copy into the padded layout only.
 *   rg_time_groupnorm_gelu_batched: rg_time_groupnorm_gelu on x [B][T_pad][C]: mean and variance per (window, channel) over
 *     the rows t < T only, output rows t >= T written as zero; C % 4 == 0, B <= 65535; workspace: 2 * B * C floats; fixed
 *     reduction order.
 *   rg_im2col_grouped_batched: rg_im2col_grouped on x [B * T][C]: out[g][b * T + t][k * C/groups + ci] =
 *     x[b * T + t + k - pad][g * C/groups + ci], zero where t + k - pad is outside the window's own [0, T); (C / groups) % 4 == 0.
 * Token sequences of different lengths are concatenated row-wise: sequence s owns rows seq_off[s] .. seq_off[s + 1) (int32
 * [n_seq + 1] on the device; seq_off_host: the same table in host memory, checked: starts at 0, does not decrease).
 *   rg_embed_sum3_ragged: rg_embed_sum3 with out[t] = word[ids[t]] + type0 + pos[t - seq_off[s]]; no sequence longer than
 *     max_pos (the rows of pos).
 *   rg_mha_bf16_ragged: rg_mha_bf16 (self-attention: Sq = Sk = the sequence's length, q / k / v / o rows indexed like the
 *     tokens) with one grid for all sequences: (n_seq * H, ceil(longest / 64)) workgroups; the key capacity (192, or 512 at
 *     hd = 64) is chosen from the longest sequence.  Rows of o outside every sequence are not written. */
int rg_wave_normalize(rg_handle* h, const float* x, int64_t ldx, float* out, int B, int n, int n_pad, int normalize,
                      void* stream);
int rg_time_groupnorm_gelu_batched(rg_handle* h, const float* x, const float* gamma, const float* beta, void* out_bf16,
                                   float* out_f32, int B, int T, int T_pad, int C, float eps, float* workspace, void* stream);
int rg_im2col_grouped_batched(rg_handle* h, const float* x, void* out_bf16, int B, int T, int C, int groups, int ksize, int pad,
                              void* stream);
int rg_embed_sum3_ragged(rg_handle* h, const int64_t* ids, const float* word, const float* pos, const float* type0, float* out,
                         const int* seq_off, const int* seq_off_host, int n_seq, int dim, int max_pos, void* stream);
int rg_mha_bf16_ragged(rg_handle* h, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, void* o, int ldo,
                       int out_is_bf16, const int* seq_off, const int* seq_off_host, int n_seq, int H, int hd, void* stream);

/* Grouped forms: n <= 4 problems of ONE shape in one launch (host arrays of n device pointers; everything else shared).
 * The four body-part VAEs run the same layer sequence on different weights and rows: issuing a layer of all four as one
 * launch divides the number of dependent launches of a VAE encode / decode by four (vae.py records the parts' launch
 * sequences and zips them).  Result bits equal the single calls. */
int rg_layernorm_grouped(rg_handle* h, int n, const float* const* x, const float* const* gamma, const float* const* beta,
                         float* const* out, int rows, int dim, void* const* out_bf16, void* stream);
int rg_add_rows_grouped(rg_handle* h, int n, const float* const* a, const float* const* b, float* const* out, int64_t n_elems,
                        int64_t period, void* stream);
int rg_copy_rows_grouped(rg_handle* h, int n, const float* const* src, float* const* dst, int groups, int nrows_per, int dim,
                         int rows_src_per, int src_row0, int rows_dst_per, int dst_row0, void* stream);
int rg_mha_bf16_grouped(rg_handle* h, int n, const float* const* q, int ldq, const float* const* k, int ldk,
                        const float* const* v, int ldv, void* const* o, int ldo, int out_is_bf16, int B, int H, int Sq, int Sk,
                        int hd, void* stream);
/* out[i] = a[i] + b[i % period]: positional embeddings / `with_pos_embed` (detr_utils.py:357-358). */
int rg_add_rows(rg_handle* h, const float* a, const float* b, float* out, int64_t n, int64_t period, void* stream);

/* Row gather/scatter between [groups, rows_per, dim] tensors (token prepend, latent slicing:
 * gesture_vae.py:150-158, 214-216; diffusion_transformer.py:239-254, 273-278). rows_src_per = 0
 * broadcasts the same source rows to every group. */
int rg_copy_rows(rg_handle* h, const float* src, float* dst, int groups, int nrows_per, int dim, int rows_src_per,
                 int src_row0, int rows_dst_per, int dst_row0, void* stream);

/* Column copy dst[r, dcol+c] = src[r, scol+c]; columns flagged in rel_mask are made relative to the
 * first frame of their clip (frames rows per clip): `trans[:,:,0] -= trans[:,0:1,0]`
 * (diffusion_transformer.py:231-232). */
int rg_copy_cols(rg_handle* h, const float* src, int ld_src, int scol, float* dst, int ld_dst, int dcol, int rows,
                 int ncols, int frames, unsigned rel_mask, void* stream);

/* Reparameterisation with explicit noise, scattered into the [B,T,D] diffusion latent:
 * latent[b, row_off + c, :] = mu + exp(logvar)^0.5 * eps, mu/logvar = tokens 0/1 of the encoder
 * output enc [B*n_chunks, seq, D] (gesture_vae.py:173-193). */
int rg_vae_reparam(rg_handle* h, const float* enc, int seq, const float* eps, float* latent, int B, int n_chunks,
                   int D, int T, int row_off, void* stream);

/* The same reparameterisation from CACHED posteriors, all four body parts of E exemplars in one launch (T = 4 n_chunks + 3):
 * latent[e, p (n_chunks + 1) + c, :] = mu[r] + exp(logvar[r])^0.5 * eps_p[e n_chunks + c, :] with cache row
 * r = slot[e] * 4 n_chunks + p n_chunks + c; the three separator rows are written as zero.
 *   mu / logvar   fp32 [cache_rows][D] (rg_venc_args: post_mu / post_logvar)      slot   int32 [E] (device)
 *   eps0 .. eps3  fp32 [E * n_chunks][D], one per part (upper, hands, face, lowertrans)    latent   fp32 [E][T][D]
 * D must be a multiple of 4; a slot outside [0, cache_rows / (4 n_chunks)) yields NaN rows, never an access out of bounds. */
int rg_vae_reparam_cached(rg_handle* h, const float* mu, const float* logvar, const int* slot, const float* eps0,
                          const float* eps1, const float* eps2, const float* eps3, float* latent, int E, int n_chunks, int D,
                          int cache_rows, void* stream);

/* axis-angle [rows, joints*3] -> 6D [rows, joints*6] written at column col_off of out, and back
 * (rotation_conversions.py:416-430 + 535-550; 511-532 + 433-447). */
int rg_aa_to_6d(rg_handle* h, const float* aa, int ld_in, float* out, int ld_out, int col_off, int rows, int joints,
                void* stream);
int rg_6d_to_aa(rg_handle* h, const float* d6, int ld_in, int col_off, float* out, int ld_out, int rows, int joints,
                void* stream);
/* What follows the decoders of n <= 4 body parts (diffusion_transformer.py:270-330), all parts in ONE launch (gridDim.y = n):
 * of part i's decoder output src[i] fp32 [rows, ld_src[i]], columns [0, 6 joints[i]) go through rg_6d_to_aa into aa[i]
 * [rows, 3 joints[i]], and up to two column ranges are copied as rg_copy_cols copies them: columns [colsK_col[i], + colsK_n[i])
 * into colsK[i] [rows, colsK_n[i]] (K = 0, 1; colsK[i] == NULL: no such range).  Every argument but `rows` is a host array of n
 * entries.  Result bits equal the single calls. */
int rg_decode_outputs(rg_handle* h, int n, const float* const* src, const int* ld_src, float* const* aa, const int* joints,
                      float* const* cols0, const int* cols0_col, const int* cols0_n, float* const* cols1, const int* cols1_col,
                      const int* cols1_n, int rows, void* stream);

/* ---------------------------------------------------------------- caller-side packing
 * tools/visualize.py:208-213: pred_motion[..., part_mask] = pred_part for upper / lower / hands / face in one
 * pass.  The masks are whole joints: src_part[j] in {0 upper, 1 lower, 2 hands, 3 face, -1 none (zeros)},
 * src_joint[j] = joint index inside that part.  out is [rows, joints*3]. */
int rg_scatter_joints(rg_handle* h, const float* upper, int ld_u, const float* lower, int ld_l, const float* hands,
                      int ld_h, const float* face, int ld_f, const int* src_part, const int* src_joint, float* out,
                      int rows, int joints, void* stream);
/* tools/visualize.py:266-291 / longform_synthesis.py:714-741: axis-angle -> 6D, F.interpolate(mode='linear',
 * scale_factor=scale, align_corners=False) along time, 6D -> axis-angle, fused.  aa [B,n,joints*3] ->
 * out [B,n*scale,joints*3].  rg_interp_linear: the same interpolation for plain features (expressions, trans). */
int rg_interp_aa(rg_handle* h, const float* aa, float* out, int B, int n, int joints, int scale, void* stream);
int rg_interp_linear(rg_handle* h, const float* x, float* out, int B, int n, int dim, int scale, void* stream);
/* tools/longform_synthesis.py:431-476: blend of a new window with the last `overlap` frames of the motion so
 * far.  Every frame of the window goes axis-angle -> 6D -> axis-angle; on frames t < overlap the 6D value is
 * prev6D*(1-w_t) + new6D*w_t, w = torch.linspace(0, 1, overlap).  prev_tail [B,overlap,joints*3], cur/out
 * [B,n,joints*3].  rg_blend_linear blends plain features in place on cur[:, :overlap]. */
int rg_blend_aa(rg_handle* h, const float* prev_tail, const float* cur, float* out, int B, int n, int joints, int overlap,
                void* stream);
int rg_blend_linear(rg_handle* h, const float* prev_tail, float* cur, int B, int n, int dim, int overlap, void* stream);

/* ---------------------------------------------------------------- retrieval sweep
 * Score of every DB entry for a query relation (sense, connective), float64, the reference's
 * operation order (rag/discourse_retrieval.py:86-222): +2 sense present, +4 exact connective among the
 * entry's relations of that sense, +3 same speaker, + mean over those relations (prominence known on
 * both sides) of 4/(1+2|p_db - p_q|).  The DB is integer-coded CSR: rel_off[n_entries+1] indexes
 * rel_sense / rel_conn / rel_prom (NaN = unknown); a connective code of -1: the connective is not in the DB
 * vocabulary; a query prominence of NaN = unknown.  top_out[e] = index (within the entry) of the relation whose
 * bounds are reported (`top_rel_idx`), -1 if the sense is absent.
 * All queries of a batch in ONE launch: params[q] = (sense code, connective code, speaker id,
 * query prominence or NaN) as four doubles (the integer codes are exact); score_out / top_out are
 * [n_queries][n_entries].  Replaces the per-query loop over raggesture.py:498-511 -> discourse_retrieval. */
int rg_discourse_scores_batched(rg_handle* h, const int* spk, const int* rel_off, const int* rel_sense,
                                const int* rel_conn, const double* rel_prom, int n_entries, const double* params,
                                int n_queries, double* score_out, int* top_out, void* stream);

/* Score of every DB entry for ONE query gesture label (type, word) of the gesture_type retrieval method
 * (rag/gesture_type_retrieval.py:41-117) and of the llm method (rag/llm_retrieval.py:278-419), float64: over the
 * entry's non-beat labels of the query type (CSR lab_off / lab_type / lab_word, words integer coded): +2 type present,
 * +spk_bonus same speaker (2 for gesture_type, 1 for llm), +5 exact word or +3/(1+2*max_r word_sim[lab_word[r]]);
 * word_sim[v] = get_word_similarity_score(DB word v, query word) computed by the caller; q_word = -1 if the query
 * word is not a DB word.  llm only: lab_prom (NaN = unknown; NULL for gesture_type) and q_prom (NaN = unknown) add
 * the mean of 4/(1+2|lab_prom - q_prom|) and move the reported label to the one of smallest difference.
 * sim_f32 != 0: the similarity model returns numpy float32 and NumPy >= 2 promotion applies, which makes the
 * reference's score arithmetic float32 from the similarity term on; 0: float64 (python floats, or NumPy < 1.24).
 * top_out = index (within the entry's non-beat labels) of the label whose bounds are reported, -1 if the type is
 * absent. */
int rg_gesture_scores(rg_handle* h, const int* spk, const int* lab_off, const int* lab_type, const int* lab_word,
                      const double* lab_prom, const double* word_sim, int n_entries, int q_type, int q_word, int q_spk,
                      double spk_bonus, double q_prom, int sim_f32, double* score_out, int* top_out, void* stream);

/* Sweep of the `prosody` retrieval method for every query word of a batch in ONE launch, float64.  The reference names this
 * method and raises NotImplementedError (raggesture.py:426-431, rag/prosodic_prominence.py is empty): the scoring is THIS
 * project's own.  It reuses the reference's prominence term 4/(1+2|dp|) (rag/discourse_retrieval.py) and feeds the reference's
 * ranking walk; what it retrieves on real speech is not measured and not claimed.
 * DB: CSR over entries -- word_off [n_entries+1] (and the same values in HOST memory, word_off_host: checked to start at 0, not to
 * decrease and to end at n_words), word_code [n_words] (index into a vocabulary of n_vocab cleaned words), word_prom [n_words]
 * (NaN / not finite = unknown), word_dur [n_words] (end - start in seconds), spk [n_entries].  With n_words == 0 the three
 * word arrays are still valid pointers (never read).
 * Queries: params [n_queries][3] doubles = (prominence p_q, duration dur_q, speaker as a double: exact); sim
 * [n_queries][n_vocab] = partial_ratio(vocabulary word, query word) / 100 (rg_partial_ratio rows).
 * For entry e over its words j (CSR order) with a finite word_prom[j], in this association:
 *   s_j   = (4 / (1 + 2 |word_prom[j] - p_q|) + 2 sim[q][word_code[j]]) + 1 / (1 + 4 |word_dur[j] - dur_q|)
 *   score = max_j s_j (the lowest j among bit-equal maxima) + (spk[e] == speaker ? 3 : 0);   top = that j - word_off[e]
 * and score 0, top -1 for an entry without such a word.  Every product is by a power of two and float64 division is correctly
 * rounded: a host restatement in IEEE float64 gives the same bits, however the words were spread over lanes.  A word_code
 * outside [0, n_vocab) counts as similarity 0 (nothing is read out of bounds).
 * score_out / top_out [n_queries][n_entries]: what rg_select_top_scores_batched takes.  The word table is read from memory once
 * per launch (a workgroup stages a tile of entries' words in LDS and loops over the queries). */
int rg_prosody_scores_batched(rg_handle* h, const int* spk, const int* word_off, const int* word_off_host, const int* word_code,
                              const double* word_prom, const double* word_dur, int n_entries, int n_words, const double* sim,
                              int n_vocab, const double* params, int n_queries, double* score_out, int* top_out, void* stream);

/* Sweep of the `motion` retrieval method (exemplars by a motion example) for every query of a batch in ONE launch.  The
 * reference has no counterpart: scoring and method are THIS project's own; how good the exemplars it finds are on real motion
 * is not measured and not claimed.
 * DB: lat fp32 [n_entries][4][L][D], contiguous, 16-byte aligned (as qlat and sp_out) -- per entry and body part (upper, hands, face, lower+trans:
 * the model's order) the VAE posterior MEANS of its L latent chunks; spk [n_entries].  1 <= L <= 10, D % 4 == 0.
 * Queries: qlat, one ragged fp32 array -- query q holds n_q = q_off[q + 1] - q_off[q] chunks and owns the 4 n_q D floats behind
 * float 4 D q_off[q], laid out [4][n_q][D]; q_off int32 [n_queries + 1] in chunks, on the device and (q_off_host) on the host;
 * params [n_queries][6] doubles = (w_upper, w_hands, w_face, w_lower, speaker as a double: exact, bonus), on the device and
 * (params_host) on the host.
 * For query q and entry e over the offsets o = 0 .. L - n_q:
 *   S_p(o) = sum_{c < n_q} sum_{k < D} (lat[e][p][o + c][k] - qlat[q][p][c][k])^2   fp32: a subtraction and a fused multiply-add
 *                                                                                   per term, in a fixed order (no Gram form)
 *   d(o)   = sum over the parts p with w_p > 0, in order, of (double)w_p * (double)S_p(o)     float64, nothing contracted
 *   o*     = the offset with the smallest d; among equal d the lowest o
 *   score  = 1.0 / (1.0 + d(o*) / ((double)(n_q D) * (((w_0 + w_1) + w_2) + w_3))) + (spk[e] == speaker ? bonus : 0)
 *   top    = o*
 * Every term of S_p is non-negative, so its error is relative -- at most (n_q D + 2) 2^-24 of the exact sum -- and an example
 * copied from the table scores exactly 1.0 at its offset.  The rows of a part with w_p = 0 are not read.
 * score_out float64 / top_out int32 [n_queries][n_entries]: what rg_select_top_scores_batched takes.  sp_out: NULL, or fp32
 * [n_queries][n_entries][4] that receives S_p(o*) (0 for a part without weight) -- the device's own sums, from which a host
 * restatement reproduces score_out bit for bit.
 * The host copies are checked before anything is launched (RG_ERR_INVALID, rg_last_error): offsets start at 0 and do not
 * decrease, every n_q is within 1 .. L, weights are finite, non-negative and not all zero, the bonus is finite, D % 4 == 0;
 * the device copies must hold the same values (a device offset pair that fails the same checks gives score NaN, top -1 and
 * reads nothing).  The table is read from memory once per launch whatever n_queries is (a workgroup stages one entry's weighted
 * parts in LDS and loops over the queries); a query's output row depends on that query and the table alone, so a batch equals
 * its queries launched one by one, bit for bit.  No allocation, synchronisation or read-back. */
int rg_motion_scores_batched(rg_handle* h, const float* lat, int n_entries, int L, int D, const int* spk, const float* qlat,
                             const int* q_off, const int* q_off_host, const double* params, const double* params_host,
                             int n_queries, double* score_out, int* top_out, float* sp_out, void* stream);

/* Word similarity of the gesture_type / llm methods as the reference effectively computes it (rag/utils.py:239-272:
 * the word2vec / fasttext models are undefined, so every call returns `fuzz.partial_ratio(db_word, query_word) / 100`,
 * fuzzywuzzy 0.18, pure-python SequenceMatcher flavour): out[v] = partial_ratio(vocab word v, query) / 100 for the
 * n_words strings vocab[v][0 .. vocab_len[v]) (int32 code points, row stride `stride`) -- the word_sim vector
 * rg_gesture_scores takes.  query_host: HOST int32 code points.  Strings longer than rg_partial_ratio_max_len() code
 * points give NaN (the host computes those with the standard library's difflib). */
int rg_partial_ratio(rg_handle* h, const int* vocab, const int* vocab_len, int n_words, int stride,
                     const int* query_host, int query_len, double* out, void* stream);
int rg_partial_ratio_max_len(void);

/* Candidate selection for the ranking walk of rag/discourse_retrieval.py:224-300: the reference sorts
 * all scores and visits entries until it holds 10, so only entries with score >= the 10th largest
 * score (with multiplicity; all ties included) and score > 0 can be visited.  Appends those
 * entries (index, top_rel_idx, score) in arbitrary order to out_*[0..cap) and leaves their count in
 * *cursor (a count > cap means the lists were truncated).  workspace: rg_select_workspace_doubles(n)
 * doubles.  Comparisons only: exact. */
int rg_select_top_scores(rg_handle* h, const double* score, const int* top, int n_entries, double* workspace,
                         int* cursor, int cap, int* out_idx, int* out_top, double* out_score, void* stream);
int rg_select_workspace_doubles(int n_entries);
/* The same for n_queries score rows at once (three launches in all): score / top [n_queries][n_entries], workspace
 * [n_queries][rg_select_workspace_doubles(n)], cursor [n_queries], out_* [n_queries][cap]. */
int rg_select_top_scores_batched(rg_handle* h, const double* score, const int* top, int n_entries, int n_queries,
                                 double* workspace, int* cursor, int cap, int* out_idx, int* out_top,
                                 double* out_score, void* stream);
/* rg_discourse_scores_batched + rg_select_top_scores_batched in TWO launches without the [n_queries][n_entries] score / relation
 * arrays (rag/discourse_retrieval.py:86-300 for all query relations of a batch): the scores stay in registers, the per-slice
 * top-10 lists give every query's threshold, and a second pass over the integer-coded DB (L2-resident) appends the entries
 * that reach it.  Same arithmetic and comparisons as the two-step form: identical survivor sets.  params [n_queries][4]
 * doubles as for rg_discourse_scores_batched; workspace [n_queries][rg_select_workspace_doubles(n)]; cursor [n_queries]
 * (zeroed by the call); out_* [n_queries][cap]. */
int rg_discourse_select_fused(rg_handle* h, const int* spk, const int* rel_off, const int* rel_sense, const int* rel_conn,
                              const double* rel_prom, int n_entries, const double* params, int n_queries, double* workspace,
                              int* cursor, int cap, int* out_idx, int* out_top, double* out_score, void* stream);

/* Tie-break similarity (rag/utils.py:109-121) of query q to DB entry c: mean_{i < min(Lq, L_c)} q[i,:].feats_c[i,:];
 * feats is the ragged [sum L, dim] fp32 token-feature table with int64 row offsets feat_off[n_entries+1]; fp32 products,
 * fp64 accumulation in a fixed order (a pair's bits do not depend on its place in a launch).
 * For n_pairs (DB entry, query) pairs of n_queries different queries in ONE launch, one workgroup per pair:
 * out[p] (device) = the similarity of query pair_query_host[p] to entry pair_entry_host[p].  q_feat_host[q]: DEVICE pointer to
 * query q's fp32 [q_len_host[q]][dim] features (16-byte aligned); the arrays themselves are HOST memory: the call checks every
 * index, writes table and pairs into a page-locked block the handle owns and uploads it in one copy on `stream`.  A later
 * call waits on the host until this call's launch has run before it reuses that block. */
int rg_text_diag_sim_many(rg_handle* h, const void* const* q_feat_host, const int* q_len_host, int n_queries,
                          const int* pair_entry_host, const int* pair_query_host, int n_pairs, const float* feats,
                          const int64_t* feat_off, int n_entries, int dim, double* out, void* stream);

/* Discourse retrieval of a whole batch in one call (rag/discourse_retrieval.py:86-300 for n_queries query relations), on
 * `stream`: (1) the sweep of rg_discourse_select_fused over params_host [n_queries][4] (uploaded here); (2) a pack launch that
 * turns the survivor lists into one contiguous block (the counts, then every query's survivors, ragged) in a buffer of the
 * handle; (3) ONE fixed-size read-back of that block and a stream synchronisation -- a batch whose survivors do not fit makes
 * the pack write the counts alone, the host grows the block and packs again; (4) the ranking on the host: survivors in ascending
 * entry order, stable sort by descending score, the leading tiers of bit-equal score > 0 while fewer than 10 entries are held;
 * (5) ONE rg_text_diag_sim_many launch for the members of every multi-member tier of every query (q_feat_host / q_len_host:
 * each query relation's clip features, as there); (6) read-back, synchronise; (7) every multi-member tier reordered by a stable
 * sort on descending similarity, the first 10 kept.  Two host synchronisations per batch (one if no tier has two members).
 * Results (HOST): n_ranked_host [n_queries] (0..10), entry_host / top_host [n_queries][10] (the ranked DB entries and, for
 * each, the index of the relation whose bounds are reported).  Every device buffer it needs belongs to the handle. */
int rg_discourse_search_batch(rg_handle* h, const int* spk, const int* rel_off, const int* rel_sense, const int* rel_conn,
                              const double* rel_prom, int n_entries, const float* feats, const int64_t* feat_off, int dim,
                              const double* params_host, int n_queries, const void* const* q_feat_host, const int* q_len_host,
                              int* n_ranked_host, int* entry_host, int* top_host, void* stream);
/* Steps (2)-(7) of rg_discourse_search_batch over the device survivor lists of ANY sweep (the gesture_type / llm methods rank
 * the lists their own rg_gesture_scores + rg_select_top_scores sweep left): cursor [n_queries] (a count above cap is read as
 * cap), idx / top / score [n_queries][cap] as rg_select_top_scores writes them.  The ranking itself -- tier cut and tie-break
 * walk -- is stated once, in csrc/rg_retrieval_host.h.  Other arguments and results as there. */
int rg_rank_survivors_batch(rg_handle* h, const int* cursor, const int* idx, const int* top, const double* score, int n_queries,
                            int cap, const float* feats, const int64_t* feat_off, int n_entries, int dim,
                            const void* const* q_feat_host, const int* q_len_host, int* n_ranked_host, int* entry_host,
                            int* top_host, void* stream);
/* Rows (16 bytes each) of the handle's survivor block; rows > 0 sets it first (tests: a block smaller than a batch's survivors
 * takes the growth path).  It starts at 4096 rows and only grows by itself. */
int rg_retrieval_pack_rows(rg_handle* h, int rows);

/* ---------------------------------------------------------------- FGD evaluation (tools/evaluate.py:267-275, :436)
 * One layer of the EMAGE skeleton-convolution encoder VAESKConv.map2latent (mogen/models/eval_models/model.py:12-107,
 * :231-251; skeleton.py:551-590 SkeletonResidual) over a RAGGED batch of clips, one workgroup per clip:
 *   r = SkeletonConv k=4 stride 2 pad 1 (zero padding at both ends of every clip; skeleton.py:13-115 weight * mask)
 *   s = SkeletonConv k=1 stride 2 (the shortcut)
 *   y = GroupNorm(groups, c_out)(r) + s   (statistics over the clip's c_out/groups channels x T/2 frames, two-pass)
 *   out = tanh(pool(y))                    (skeleton.py:166-240 SkeletonPool, a fixed averaging matrix; no pool: tanh(y))
 * The masked weights are packed per output channel (CSR over the input channels the mask keeps): row_ptr [c_out+1], col
 * [nnz], w_res [nnz][4] (the four taps), w_sc [nnz].  The pool is pool_k (source channel, weight) pairs per output channel,
 * source -1 = unused; pool_src = NULL: no pool (c_pool = c_out).
 * clip_off are the frame offsets of the LAYER-0 input ([n_clips+1], starting at 0, every clip a multiple of 16 frames):
 * layer L reads rows [off >> L, ...) of x ([off[n] >> L][c_in]) and writes rows [off >> (L+1), ...) of y ([.][c_pool]);
 * r and s are scratch of [off[n] >> (L+1)][c_out] floats each.  clip_off_host is the same table in host memory (checked).
 * fp32 FMAs in a fixed order: a clip's result does not depend on the other clips of the launch. */
typedef struct rg_fgd_layer_args {
  const float* x;
  float* y;
  float* r;
  float* s;
  const int* clip_off;
  const int* clip_off_host;
  const int* row_ptr;
  const int* col;
  const float* w_res;
  const float* w_sc;
  const float* b_res;
  const float* b_sc;
  const float* gamma;
  const float* beta;
  const int* pool_src;
  const float* pool_w;
  int n_clips;
  int layer;
  int c_in;
  int c_out;
  int c_pool;
  int pool_k;
  int groups;
  float eps;
} rg_fgd_layer_args;
int rg_fgd_encoder_layer(rg_handle* h, const rg_fgd_layer_args* args_host, void* stream);
/* Column mean and covariance (N-1 normalisation, np.cov(rowvar=False)) of n x dim fp32 latents, both accumulated in fp64
 * and in two passes (mean first, then sum (x - mean)(x - mean)^T): the moments of metric.py:253-258.  mean [dim], cov
 * [dim][dim] (exactly symmetric).  n >= 2, 1 <= dim <= 4096. */
int rg_latent_moments(rg_handle* h, const float* lat, int n, int dim, double* mean, double* cov, void* stream);

/* ---------------------------------------------------------------- SMPL-X joint metrics (rg_motion.hip)
 * Forward kinematics of the 55 SMPL-X joints: what smplx.SMPLX.forward(..., return_joints=True)["joints"][:, :55] computes
 * for the calls of tools/evaluate.py:286-327 and tools/evaluate_mm.py:158-172 (zero translation, zero expression), i.e.
 * J_transformed of smplx.lbs.batch_rigid_transform:
 *   v = poses[f][3j..3j+2] (+ pose_mean[3j..3j+2]: SMPLX.forward adds the hand mean pose unless flat_hand_mean)
 *   R_j = batch_rodrigues(v)  (angle = |v + 1e-8|, R = I + sin K + (1 - cos) K^2)
 *   G_root = [R_0 | J_0],  G_j = G_parent(j) . [R_j | J_j - J_parent(j)]  in parent order;  joints[f][j] = G_j[:3, 3]
 * poses [F][165] axis-angle in SMPL-X full_pose order (global, body 21, jaw, leye, reye, lhand 15, rhand 15); rest
 * [n_clips][55][3] the rest joints of each clip (J_regressor (v_template + shapedirs . betas)); parents [55] with
 * parents[0] < 0 and parents[j] in [0, j) (parents_host: the same table in host memory, checked); clip_off [n_clips+1] frame
 * offsets (clip_off_host checked).  fold != 0 first maps each joint's rotation vector to the equivalent one with angle in
 * [0, pi], which is what evaluate.py:261-280's axis-angle -> 6D -> axis-angle round trip does before the model adds
 * pose_mean.  fp32 in a fixed order, one wave per frame: a frame's joints do not depend on the rest of the launch. */
typedef struct rg_smplx_joints_args {
  const float* poses;
  const float* rest;
  const float* pose_mean;         /* [165] or NULL */
  const int* parents;
  const int* parents_host;
  const int* clip_off;
  const int* clip_off_host;
  float* joints;                  /* [F][55][3] */
  int n_clips;
  int fold;
} rg_smplx_joints_args;
int rg_smplx_joints(rg_handle* h, const rg_smplx_joints_args* args_host, void* stream);
/* One workgroup per clip of joints [F][55][3] (clip_off [n_clips+1], clip_off_host checked, every clip >= 2 frames):
 *  l1_sum[c]  = sum over frames x 165 columns of |x - column mean of the clip|, fp64, two passes (metric.py:12-24 L1div.run)
 *  beats      (NULL: skipped) [F][55] 0 / 1: metric.py:78-127 alignment.load_pose(joints, t_margin, n - t_margin, fps) as
 *             evaluate.py:406 calls it.  vel = |central (forward / backward at the ends) difference over dt, dt2 = 2 dt| / mmae[j]
 *             (fp32 differences and norm, fp64 division); window index w of vel[t_margin : n - t_margin] is a beat when
 *             argrelextrema(np.less, order, mode='clip') marks it AND vel at frame w (not t_margin + w: metric.py:122 compares
 *             the window-relative index with absolute frame indices) > threshold.  The flag is stored at frame t_margin + w.
 *  mpjpe_sum  (NULL: skipped) [n_clips]: with retr_off[c] >= 0, sum over (frame, joint) of mask * |(x - x[0][0]) - (y - y[0][0])|
 *             in fp64, y = retr_joints rows retr_off[c].., mask = joint_mask[j] and retr_poses[row][3j..3j+2] not all zero
 *             (evaluate.py:243-254, :372-388, metric.py:352-382); retr_off[c] < 0: 0. */
typedef struct rg_joint_stats_args {
  const float* joints;
  const int* clip_off;
  const int* clip_off_host;
  double* l1_sum;
  unsigned char* beats;
  const double* mmae;             /* [55] */
  const float* retr_joints;       /* [.][55][3] */
  const float* retr_poses;        /* [.][165] */
  const int* retr_off;            /* [n_clips] */
  const unsigned char* joint_mask;/* [55] */
  double* mpjpe_sum;
  int n_clips;
  int t_margin;
  int order;
  float dt;
  float dt2;
  double threshold;
} rg_joint_stats_args;
int rg_joint_clip_stats(rg_handle* h, const rg_joint_stats_args* args_host, void* stream);
/* For every group g of rows of x [N][dim] (group_off [n_groups+1], group_off_host checked): out[g] = sum over pairs i < j of
 * the group of ||x_i - x_j||_2, in fp64.  Differences in fp32, squares accumulated per pair in fp64 (no Gram form: rows of one
 * group may be near-duplicates), 32 x 32 pair tiles of the upper triangle, sums in a fixed order (no atomics): the result does
 * not depend on how groups are batched.  partial is scratch of partial_len >= n_groups * T * T doubles, T = ceil(max group
 * rows / 32).  Diversity (metric.py:330-345) is one group of all clips, multimodality (evaluate_mm.py:180-181) one group per
 * clip of its repetitions; the callers divide by the frame count and the pair count. */
typedef struct rg_pair_dist_args {
  const float* x;
  const int* group_off;
  const int* group_off_host;
  double* partial;
  double* out;
  int64_t partial_len;
  int n_groups;
  int dim;
} rg_pair_dist_args;
int rg_pair_distance_sums(rg_handle* h, const rg_pair_dist_args* args_host, void* stream);
/* SRGR, semantic-relevance gesture recall (mogen/models/utils/metric.py:30-52 SRGR.run as tools/evaluate.py:413-426 calls it),
 * one workgroup per clip of pred / gt joints [F][n_joints][3] (clip_off [n_clips+1], clip_off_host checked: starts at 0, does
 * not decrease; an empty clip gives 0 / 0).  For frame i and joint j of a clip, diff = (|dx| + |dy|) + |dz| in fp32 is a
 * success when diff < threshold (an fp32 comparison):
 *   wsum[c]  = sum over the clip's successes of weights[frame]   (= sum_i w[i] count_i), fp64
 *   count[c] = the number of successes                            (= sum_i count_i)
 * weights [F] is the clip's sem_score per frame (the caller resamples it to the pose rate); the caller divides by 0.165,
 * n_joints and the frame count (metric.py:45-48).  The reference uses threshold = 0.3 and n_joints = 55.  fp64 accumulation,
 * sums in a fixed order that depends on the clip alone (no atomics): a clip gives the same bits alone and inside a batch. */
typedef struct rg_srgr_args {
  const float* pred;              /* [F][n_joints][3] */
  const float* gt;                /* [F][n_joints][3] */
  const float* weights;           /* [F] */
  const int* clip_off;
  const int* clip_off_host;
  double* wsum;                   /* [n_clips] */
  int64_t* count;                 /* [n_clips] */
  int n_clips;
  int n_joints;
  float threshold;
} rg_srgr_args;
int rg_srgr_clip_sums(rg_handle* h, const rg_srgr_args* args_host, void* stream);

/* ---------------------------------------------------------------- audio onsets (rg_audio.hip)
 * The onset times beat alignment compares the motion beats with (mogen/models/utils/metric.py:64-76 alignment.load_audio:
 * librosa.onset.onset_detect(y, sr=16000, hop_length=512, units="time")), the library's defaults restated, in two launches over
 * a ragged batch: samples holds the clips one after the other, clip c is samples[sample_off[c] .. sample_off[c + 1]) at 16 kHz
 * and has 1 + n / 512 frames, frames frame_off[c] .. frame_off[c + 1) of the batch (the *_host copies are checked: start at 0,
 * do not decrease, agree with each other).
 *
 * rg_onset_mel_db, one workgroup per frame t of a clip: window position k reads sample 512 t - 1024 + k (zero outside the
 * clip) times window[k] (the periodic Hann window), a 2048-point complex fp32 FFT in LDS with the turns read from
 * twiddle[m] = exp(-2 pi i m / 2048) (re, im; m < 2048), the power |X|^2 of bins 0 .. 1024, and for every mel filter m < 128
 * the sum of mel_weight[m][j] * power[mel_start[m] + j] over j < mel_len[m] (mel_len <= RG_ONSET_MEL_STRIDE, checked on the
 * *_host copies):
 *   db[frame][m] = 10 log10(max(1e-10, sum))
 *   clip_max[c]  = the largest db of the clip, as the order-preserving unsigned image of the float (sign bit set for values
 *                  >= 0, all bits flipped below: unsigned order = float order); the entry point zeroes it first. */
#define RG_ONSET_N_FFT 2048
#define RG_ONSET_HOP 512
#define RG_ONSET_MELS 128
#define RG_ONSET_MEL_STRIDE 64
typedef struct rg_onset_mel_args {
  const float* samples;
  const int64_t* sample_off;      /* [n_clips + 1] */
  const int64_t* sample_off_host;
  const int64_t* frame_off;       /* [n_clips + 1] */
  const int64_t* frame_off_host;
  const float* window;            /* [2048] */
  const float* twiddle;           /* [2048][2] */
  const int* mel_start;           /* [128] */
  const int* mel_len;             /* [128] */
  const int* mel_start_host;
  const int* mel_len_host;
  const float* mel_weight;        /* [128][RG_ONSET_MEL_STRIDE] */
  float* db;                      /* [frames][128] */
  unsigned int* clip_max;         /* [n_clips] */
  int n_clips;
} rg_onset_mel_args;
int rg_onset_mel_db(rg_handle* h, const rg_onset_mel_args* args_host, void* stream);
/* rg_onset_pick, one workgroup per clip of N frames, on what rg_onset_mel_db wrote (metric.py:64-76 alignment.load_audio:
 * librosa's onset_strength and peak_pick with the parameters its defaults come to at 16 kHz and hop 512):
 *   db         <- max(db, max of the clip - top_db), in place (power_to_db's top_db, against this clip's maximum only)
 *   env[t]     = mean over the 128 bands of max(0, db[t - 2] - db[t - 3]) for t >= 3, else 0 (lag 1, centred frames: 3 in front)
 *   x[t]       = (env[t] - min env) / (max (env - min env) + FLT_MIN); 0 everywhere when env is 0 everywhere
 *   avg[t]     = mean of x[max(t - pre_avg, 0) .. min(t + post_avg, N))
 *   frame t is an onset when x[t] > 0 and x[t] >= avg[t] + delta (pre_max 0, post_max 1, wait 0: nothing else is thinned out)
 * onset_frames[frame_off[c] ..] receives the clip's onset frames in ascending order, onset_count[c] their number.  The
 * reference's values: top_db 80, pre_avg 3, post_avg 4, delta 0.07. */
typedef struct rg_onset_pick_args {
  float* db;                      /* [frames][128] */
  const unsigned int* clip_max;   /* [n_clips] */
  const int64_t* frame_off;       /* [n_clips + 1] */
  const int64_t* frame_off_host;
  float* x;                       /* [frames] */
  float* avg;                     /* [frames] */
  int* onset_frames;              /* [frames] */
  int* onset_count;               /* [n_clips] */
  int n_clips;
  int pre_avg;
  int post_avg;
  float top_db;
  float delta;
} rg_onset_pick_args;
int rg_onset_pick(rg_handle* h, const rg_onset_pick_args* args_host, void* stream);

/* ---------------------------------------------------------------- audio resampling (rg_audio.hip)
 * Recorded audio as a WAV file stores it -> float32 mono at the rate the models hear (what mogen/datasets/beatx_dataset.py:474-475
 * gets from librosa.load and librosa.resample(..., target_sr=16000); the filter is this project's own, below), for a ragged
 * batch of clips that share rate, channel count and sample format, in one launch.  src holds the clips' interleaved frames
 * one after the other: clip c is frames src_off[c] .. src_off[c + 1) of `channels` samples each, and becomes out[out_off[c] ..
 * out_off[c + 1)), n_out = ceil(n up / down) samples for n frames (the *_host copies are checked: start at 0, do not decrease,
 * agree with each other).
 *
 * Decode and downmix, fused into the load:  x[k] = (sum over the channels, in channel order, of sample * scale) * (1.0f / channels)
 * with scale 2^-15 (RG_RESAMPLE_PCM16: int16), 2^-23 (RG_RESAMPLE_PCM24: 3 bytes per sample, little-endian, two's complement),
 * 2^-31 (RG_RESAMPLE_PCM32: int32) or 1 (RG_RESAMPLE_F32: float32); x[k] = 0 outside 0 <= k < n, so no clip hears its neighbour.
 *
 * Polyphase resampling by up / down with the 2 half_len + 1 taps h of a low-pass filter (scipy.signal.resample_poly(x, up,
 * down, window=h / up)):
 *   y[m] = sum over k of h[m down - k up + half_len] x[k]                         (|m down - k up| <= half_len)
 * read from coeff [up][taps], coeff[p][j] = h[p + j up] (0 past the end of h), taps = 2 half_len / up + 1:
 *   p = (m down + half_len) % up,  k_hi = (m down + half_len) / up,  y[m] = sum over j < taps of coeff[p][j] x[k_hi - j]
 * added up in fp32 in ascending j, one fused multiply-add per tap from 0: an output's bits depend on its clip alone, not on the
 * batch around it.  All of m down and k up is 64-bit arithmetic.  A workgroup of 256 threads produces RG_RESAMPLE_TILE consecutive
 * outputs of one clip from the (RG_RESAMPLE_TILE - 1) down / up + taps + 1 input samples it stages, decoded, in LDS (at most
 * 64 KB: up to down / up = 15); with up <= 2 the table is staged there too.
 * coeff == NULL (only with up = down = taps = 1, half_len = 0): y = x, the decoded and downmixed samples bit for bit. */
#define RG_RESAMPLE_PCM16 0
#define RG_RESAMPLE_PCM24 1
#define RG_RESAMPLE_PCM32 2
#define RG_RESAMPLE_F32 3
#define RG_RESAMPLE_TILE 1024
#define RG_RESAMPLE_MAX_CHANNELS 8
int rg_resample_poly(rg_handle* h, const void* src, int fmt, int channels, const int64_t* src_off, const int64_t* src_off_host,
                     const int64_t* out_off, const int64_t* out_off_host, int n_clips, int up, int down, int half_len, int taps,
                     const float* coeff, float* out, void* stream);

/* ---------------------------------------------------------------- word timings and frame-aligned word vectors (rg_ctc.hip)
 * The reference reads word timings from annotation files a forced aligner wrote offline and lays BERT word vectors onto the
 * motion frames when it builds its dataset (mogen/datasets/beatx_dataset.py:858-869, get_word_vectors :1126-1161).  Here the
 * timings come from the character emissions of the CTC head of the audio encoder that already runs (facebook/wav2vec2-base-960h:
 * lm_head [32, 768]); the aligner is this project's own, the frame rule restates the reference's lines.
 *
 * rg_ctc_log_softmax: logits [rows][V] fp32, 2 <= V <= RG_CTC_MAX_VOCAB -> logp [rows][V] = (x - max) - logf(sum of expf(x - max))
 * and best [rows] = the lowest class index among the row's maxima.  One wave per row, lane = class; maximum and sum by an xor
 * butterfly over the 64 lanes (32, 16, ..., 1; lanes >= V hold -inf and 0): a row's bits depend on that row alone.
 *
 * rg_ctc_align: Viterbi alignment of a ragged batch, one workgroup per item.  Item i owns the emission rows E = logp[frame_off[i]
 * .. frame_off[i + 1]) (T >= 1 of them) and the target tokens y = tokens[tok_off[i] .. tok_off[i + 1]) (L >= 1; each in [0, V),
 * none equal to `blank`: the caller checks them on its host copy -- an item that holds another gets status 2 and no alignment).
 * Extended sequence z of S = 2 L + 1 <= RG_CTC_MAX_STATES states: z[2 j] = blank, z[2 j + 1] = y[j].  In fp32, NEG = -inf:
 *   a[0][0] = E[0][blank], a[0][1] = E[0][y[0]], a[0][s] = NEG otherwise
 *   a[t][s] = E[t][z[s]] + max of, in this order and replaced only by a strictly greater value,
 *             a[t-1][s] (code 0), a[t-1][s-1] if s >= 1 (code 1), a[t-1][s-2] if s >= 2, z[s] != blank, z[s] != z[s-2] (code 2)
 *   end state S - 1, unless a[T-1][S-2] > a[T-1][S-1]: then S - 2
 * The codes are 2 bits each, RG_CTC_STATES_PER_THREAD = 16 to a uint32 (state s: bits 2 (s % 16) of word s / 16); frame t >= 1 of
 * item i is words backptr[backptr_off[i] + t W ..+ W), W = ceil(S / 16), so an item needs T W words of scratch.  Outputs:
 * path[frame_off[i] + t] = the state of frame t; tok_first / tok_last[tok_off[i] + j] = the first / last frame in state 2 j + 1;
 * score[i] = the end value; status[i] = 0.  When the end value is -inf (T < L + the number of adjacent equal tokens): status[i]
 * = 1, path all 0, tok_first = tok_last = -1.  An item's outputs depend on that item alone.  The *_host copies are checked:
 * start at 0, do not decrease, T >= 1, L >= 1, S within the cap, scratch large enough.
 *
 * rg_word_frames: out[frame_off[b] + f][D] for frame f of window b (frame_off[b + 1] - frame_off[b] frames: frames beyond are
 * never written, as the reference's slice clamps) = the mean of hidden[r][D] over r in tok_row_off[w] .. tok_row_off[w + 1]
 * (ascending, serial fp32 sum, divided by (float)count) for the LAST word w in word_off[b] .. word_off[b + 1] with
 * start_frame[w] <= f < end_frame[w] (the reference assigns slices in word order: later words overwrite), zeros when no word
 * covers f.  tok_row_off has one entry more than there are words; rows that belong to no word ([CLS], [SEP]) are given to a word
 * of no frames (start_frame = end_frame).  A word without rows is the caller's to refuse. */
#define RG_CTC_MAX_VOCAB 64
#define RG_CTC_MAX_STATES 4096
#define RG_CTC_STATES_PER_THREAD 16
int rg_ctc_log_softmax(rg_handle* h, const float* logits, int64_t rows, int V, float* logp, int* best, void* stream);
int rg_ctc_align(rg_handle* h, const float* logp, int V, const int64_t* frame_off, const int64_t* frame_off_host, const int* tokens,
                 const int64_t* tok_off, const int64_t* tok_off_host, int n_items, int blank, unsigned* backptr,
                 const int64_t* backptr_off, const int64_t* backptr_off_host, int* path, int* tok_first, int* tok_last, float* score,
                 int* status, void* stream);
int rg_word_frames(rg_handle* h, const float* hidden, const int* tok_row_off, const int* start_frame, const int* end_frame,
                   const int* word_off, const int* word_off_host, const int64_t* frame_off, const int64_t* frame_off_host, int n_windows,
                   int D, float* out, void* stream);

/* ---------------------------------------------------------------- word prosodic prominence (rg_prosody.hip)
 * Discourse retrieval compares the prosodic prominence of connectives (rag/utils.py:171-228 map_conns_to_prominence, rag/
 * discourse_retrieval.py:172-192); the reference reads the values from prom/<recording>.prom files an offline wavelet-prosody tool
 * wrote (mogen/datasets/beatx_dataset.py:660-670).  Here they are estimated from 16 kHz audio and word timings by the published
 * recipe -- f0, energy and word duration normalised and summed, a Mexican-hat wavelet transform over scales, lines of maximum
 * amplitude read per word -- restated as this project's own arithmetic: the values live on this estimator's scale, parity with
 * that tool is not claimed.  Four launches for a ragged batch of n_rec recordings; recording i owns samples sample_off[i] ..
 * sample_off[i + 1]) (n of them), frames frame_off[i] .. frame_off[i + 1]) (T = 1 + n / RG_PROSODY_HOP, frame t stands at t / 100 s)
 * and words word_off[i] .. word_off[i + 1]).  The *_host copies are checked before the launch: start at 0, do not decrease, agree
 * with each other.  A recording's outputs depend on that recording alone (fixed summation orders, no atomics).
 *
 * rg_prosody_frames, one workgroup per frame.  Window x[k] = sample 160 t - 512 + k, k < RG_PROSODY_WIN, 0 outside the recording.
 *   energy[t] = logf(sum of x[k]^2 / 1024 + 1e-10f); the sum: thread j < 256 adds k = j, j + 256, j + 512, j + 768 in that order,
 *   then an xor butterfly over the wave's lanes (32, 16, .., 1), then the four waves in order.
 *   N = RG_PROSODY_WIN - RG_PROSODY_LAG_MAX - 1 = 757.  For every lag L in LAG_MIN - 1 .. LAG_MAX + 1 (one thread each), serial and
 *   ascending in i < N with one fused multiply-add per product:  xy = sum x[i] x[i + L],  yy = sum x[i + L]^2, and xx = sum x[i]^2;
 *   r(L) = xy / sqrtf(xx * yy + 1e-20f).
 *   The chosen lag is the argmax over LAG_MIN .. LAG_MAX of r(L) - 0.05f * (float)L / (float)LAG_MAX, ties to the smallest lag.
 *   d = r(L - 1) - 2 r(L) + r(L + 1); delta = d == 0 ? 0 : clamp(0.5f * (r(L - 1) - r(L + 1)) / d, -0.5f, 0.5f).
 *   nccf[t] = r(L), lag[t] = L, logf0[t] = logf(16000.0f / ((float)L + delta)).
 *
 * rg_prosody_signal, one workgroup per recording.
 *   emax = max energy; floor = emax - 11.5f; voiced[t] = nccf[t] >= 0.5f && energy[t] >= floor (fp32 comparisons); energy is clamped
 *   from below at floor.
 *   fill(knots): a frame that is no knot, between the nearest knots a < t < b, takes v[a] + (v[b] - v[a]) * ((float)(t - a) /
 *   (float)(b - a)); before the first knot or after the last it takes that knot's value; without knots every frame is 0.
 *   f0 = fill(voiced frames, logf0); status[i] = 1 when no frame is voiced (f0 all 0: not an error), else 0.
 *   Duration: word w with frames (start_frame[w] < end_frame[w]; a recording's words are sorted, start_frame[w] >= end_frame[w - 1])
 *   is a knot at frame (start_frame + end_frame - 1) / 2 with value logf(fmaxf(word_end[w] - word_start[w], 0.01f)) (seconds, fp32);
 *   dur = fill(those knots).  `knot` is [frames] int32 scratch.
 *   Each track z-normalised over the recording: mean, then the population variance around it, both in fp64 (a thread adds its
 *   contiguous share of the frames in order, then butterfly, then the waves in order); z = (float)((v - mean) / max(std, 1e-6)).
 *   c[t] = fmaf(w_dur, dz, fmaf(w_en, ez, w_f0 * f0z)).  Written: voiced, f0 (filled), f0z, ez, dz, c.
 *
 * rg_prosody_cwt, one workgroup per tile of RG_PROSODY_TILE frames of one recording (tile_off: prefix sums of ceil(T / TILE)), c
 * staged with RG_PROSODY_HALO frames on both sides (0 outside the recording) and the taps in LDS.  Scale j < RG_PROSODY_SCALES:
 *   s_j = 2 * 2^(j / 2) frames, R_j = ceil(5 s_j) = 10 15 20 29 40 57 80 114 160 227,
 *   W[j][t] = sum over k = -R_j .. R_j, serial and ascending, one fused multiply-add per tap from 0, of c[t + k] psi_j[k],
 *   psi_j[k] = (1 - u^2) exp(-u^2 / 2) / sqrt(s_j), u = k / s_j: computed in float64 by the caller, rounded once, the scales' taps
 *   one after the other (RG_PROSODY_TAPS = sum of 2 R_j + 1 floats).  W is [RG_PROSODY_SCALES][frames of the whole batch].
 *
 * rg_prosody_words, one workgroup per recording, two phases.  Lines: frame p starts a peak line when W[0][p] > 0, W[0][p] >
 * W[0][p - 1] and W[0][p] >= W[0][p + 1] (a missing neighbour is -inf).  pos_0 = p, strength = W[0][p]; for j = 1 .. 9 in order: among
 * the frames q of the recording with |q - pos_(j-1)| <= ceil(s_j) = 3 4 6 8 12 16 23 32 46 that pass the same test on W[j], the nearest
 * to pos_(j-1) (ties: the lower q) becomes pos_j and strength += W[j][q] (fp32); without one the line ends.  Valley lines: the same on
 * -W.  peak_strength[t] / valley_strength[t] = the strength of the line that starts at t, 0 where none does (a line's strength is > 0).
 * Words, one wave each (lanes stride over the frames, then a butterfly; the larger strength wins, the lower frame among equals):
 *   prominence[w] = the largest peak_strength in [start_frame[w], end_frame[w]), prom_frame[w] the frame it stands at (0, -1: none);
 *   boundary[w] = the largest valley_strength in [mid_w, mid_v), mid = (start_frame + end_frame - 1) / 2, v the next word that has
 *   frames (for the last one: up to the end of the recording), bnd_frame[w] its frame.  A word without frames gets 0, 0, -1, -1. */
#define RG_PROSODY_HOP 160
#define RG_PROSODY_WIN 1024
#define RG_PROSODY_LAG_MIN 40
#define RG_PROSODY_LAG_MAX 266
#define RG_PROSODY_SCALES 10
#define RG_PROSODY_TILE 256
#define RG_PROSODY_HALO 227
#define RG_PROSODY_TAPS 1514
int rg_prosody_frames(rg_handle* h, const float* samples, const int64_t* sample_off, const int64_t* sample_off_host,
                      const int64_t* frame_off, const int64_t* frame_off_host, int n_rec, float* energy, float* nccf, int* lag,
                      float* logf0, void* stream);
int rg_prosody_signal(rg_handle* h, const float* energy, const float* nccf, const float* logf0, const int64_t* frame_off,
                      const int64_t* frame_off_host, const int64_t* word_off, const int64_t* word_off_host, const int* start_frame,
                      const int* end_frame, const int* start_frame_host, const int* end_frame_host, const float* word_start,
                      const float* word_end, int n_rec, float w_f0, float w_en, float w_dur, int* voiced, float* f0, float* f0z,
                      float* ez, float* dz, float* c, int* knot, int* status, void* stream);
int rg_prosody_cwt(rg_handle* h, const float* c, const int64_t* frame_off, const int64_t* frame_off_host, const int64_t* tile_off,
                   const int64_t* tile_off_host, int n_rec, const float* taps, float* W, void* stream);
int rg_prosody_words(rg_handle* h, const float* W, const int64_t* frame_off, const int64_t* frame_off_host, const int64_t* word_off,
                     const int64_t* word_off_host, const int* start_frame, const int* end_frame, const int* start_frame_host,
                     const int* end_frame_host, int n_rec, float* peak_strength, float* valley_strength, float* prominence,
                     float* boundary, int* prom_frame, int* bnd_frame, void* stream);

/* ---------------------------------------------------------------- baseline JPEG of rendered frames (rg_jpeg.hip)
 * uint8 RGB frames -> the entropy-coded scan of a baseline sequential JPEG (ITU-T T.81: 8 bit, three components, YCbCr 4:2:0,
 * the Annex K.3 Huffman tables, one restart interval per MCU row), which rag-gesture_amd/video.py wraps into JFIF files and a
 * Motion-JPEG AVI.  The reference's tools write H.264 through ffmpeg (mogen/utils/visualization.py:71-136); this encoder is
 * the project's own.  An MCU is 16 x 16 pixels; a frame of H x W pixels has mcu_rows = ceil(H / 16) by mcu_cols = ceil(W / 16)
 * of them, the pixels past its edges repeating the edge's.
 *
 * rg_jpeg_dct_quant: frames [n_frames][height][pitch][3] uint8 (pitch in pixels: a panel of a wider buffer is its first pixel
 * and the buffer's width) -> coef [n_frames][mcu_rows * mcu_cols][6][64] int16, the blocks Y00, Y01, Y10, Y11, Cb, Cr of an
 * MCU, each in zig-zag order.  In fp32:
 *   Y = 0.299 R + 0.587 G + 0.114 B - 128,  Cb = -0.168736 R - 0.331264 G + 0.5 B,  Cr = 0.5 R - 0.418688 G - 0.081312 B
 *   (JFIF full range, level-shifted, never rounded to 8 bit), chroma = the mean of each 2 x 2 pixels, the orthonormal 8 x 8
 *   DCT-II, and coefficient k = sign(v) floor(|v| / q[k] + 0.5) with q_luma / q_chroma [64] in zig-zag order, each 1 .. 255.
 *
 * rg_jpeg_entropy_count / rg_jpeg_entropy_write: the same coder twice.  Interval i = frame i / mcu_rows, MCU row i % mcu_rows:
 * the Huffman codes of its blocks in order, the DC prediction starting from 0, the last byte filled with 1 bits, a 0x00 behind
 * every 0xFF byte, and the marker RSTm (m = row % 8) behind every interval but a frame's last.  count stores lengths[i], the
 * bytes of interval i with its marker; write puts them at out + offsets[i], offsets being the exclusive sum of the lengths
 * (the caller's), and nothing at or beyond out + capacity.  A frame's scan is the bytes of its intervals one after the other.
 * Coefficients beyond the baseline's range (AC +-1023, DC difference +-2047) are coded as the nearest value inside it. */
#define RG_JPEG_MCU 16
#define RG_JPEG_BLOCKS 6
#define RG_JPEG_MAX_MCUS 4096
int rg_jpeg_dct_quant(rg_handle* h, const unsigned char* frames, int n_frames, int height, int width, int pitch,
                      const unsigned char* q_luma, const unsigned char* q_chroma, int16_t* coef, void* stream);
int rg_jpeg_entropy_count(rg_handle* h, const int16_t* coef, int n_frames, int mcu_rows, int mcu_cols, int* lengths, void* stream);
int rg_jpeg_entropy_write(rg_handle* h, const int16_t* coef, int n_frames, int mcu_rows, int mcu_cols, const int64_t* offsets,
                          unsigned char* out, int64_t capacity, void* stream);

/* ---------------------------------------------------------------- SMPL-X mesh and face metrics (rg_mesh.hip)
 * smplx.lbs as smplx.SMPLX.forward calls it, in two launches over "rows" (frames):
 *   v_posed[r] = base[clip(r)] + coeff[r] . basis        (the blend shapes of the row's active columns; every column whose
 *                                                           coefficient is the same for all rows is folded into base)
 *   vertex[r][v] = (sum_j weights[v][j] A[r][j]) . [v_posed[r][v]; 1]
 * Per row, rg_mesh_transforms writes coefficient columns 0..99 = the expression psi (exprs NULL: zeros) and, for every joint j
 * with pf_col[j] >= 0, columns pf_col[j] .. pf_col[j] + 8 = R_j - I row-major (smplx's pose_feature entries of joint j), and
 * A[r][j] = [R_g | t_g - R_g J_j] (3 x 4 row-major), where J_j = j_clip[clip][j] + j_expr[j] . psi (J_regressor of v_shaped:
 * the joints move with the expression), R_j = batch_rodrigues(fold(poses[r][3j..]) + pose_mean[3j..]) as rg_smplx_joints,
 * and G = [R_g | t_g] the chain of the kinematic tree.  joints (NULL: skipped) [rows][55][3] = t_g.  Columns the launch
 * does not own keep their values (the caller zeroes coeff).  poses [rows][165], exprs [rows][100], j_clip [n_clips][55][3],
 * j_expr [55][3][100], pf_col [55] (pf_col_host: the same, checked; pf_col[0] < 0), coeff [rows][k_pad], A [rows][55][12].
 * One wave per row: a row does not depend on the rest of the launch. */
typedef struct rg_mesh_transforms_args {
  const float* poses;
  const float* exprs;             /* [rows][100] or NULL */
  const float* j_clip;
  const float* j_expr;
  const float* pose_mean;         /* [165] or NULL */
  const int* parents;
  const int* parents_host;
  const int* clip_off;
  const int* clip_off_host;
  const int* pf_col;
  const int* pf_col_host;
  float* coeff;
  float* A;
  float* joints;                  /* [rows][55][3] or NULL */
  int n_clips;
  int k_pad;
  int fold;
} rg_mesh_transforms_args;
int rg_mesh_transforms(rg_handle* h, const rg_mesh_transforms_args* args_host, void* stream);

#define RG_MESH_RAW 0             /* out[r][0 .. d_pad) = v_posed[r] (no skinning) */
#define RG_MESH_VERTICES 1        /* out[r][v][3] = vertex[r][v] (+ transl[r]) */
#define RG_MESH_FACE 2            /* rows 2p / 2p+1 = prediction / ground truth of frame pair p: partial, no vertex written */
/* coeff [coeff_rows >= rows rounded up to 64][k_pad] (k_pad a multiple of 16; pad rows and columns zero), basis
 * [k_pad][d_pad] (column 3v + c, d_pad = 3 * (n_verts rounded up to 64), pad zero), base [n_clips][d_pad] (base_per_clip
 * != 0: clip_off [n_clips+1] row offsets, checked through clip_off_host) or [1][d_pad].  Skinning (VERTICES, FACE): A
 * [rows][55][12] of rg_mesh_transforms, per vertex skin_n[v] <= max_nnz nonzero weights skin_w[v][q] of joints skin_j[v][q].
 * FACE: partial [rows / 2][n_groups][2] (partial_len doubles at least) = per frame pair and group g of vertex tiles (tiles
 * g, g + n_groups, ...) the sums over vertices and coordinates of d^2 and |d|, d = vertex[2p] - vertex[2p+1] (fp32
 * difference, fp64 sums in a fixed order); every clip holds an even number of rows.  The GEMM is fp32 in, fp32 out on
 * v_mfma_f32_32x32x2_f32 (each element an fp32 fma chain in k order), so no row depends on the rest of the launch. */
typedef struct rg_mesh_blend_args {
  const float* coeff;
  const float* basis;
  const float* base;
  const int* clip_off;
  const int* clip_off_host;
  const float* A;
  const int* skin_n;
  const int* skin_j;
  const float* skin_w;
  const float* transl;            /* [rows][3] or NULL (VERTICES) */
  float* out;
  double* partial;
  int64_t partial_len;
  int mode;
  int n_clips;
  int rows;
  int coeff_rows;
  int k_pad;
  int n_verts;
  int d_pad;
  int max_nnz;
  int n_groups;
  int base_per_clip;
} rg_mesh_blend_args;
int rg_mesh_blend_skin(rg_handle* h, const rg_mesh_blend_args* args_host, void* stream);
/* One workgroup per clip of frame pairs (pair_off [n_clips+1], pair_off_host checked): sums[c][0] = the clip's partial[.][.][0]
 * over all its pairs, sums[c][1] = partial[.][.][1] over pairs 1 .. n-1; fp64, a fixed order that depends on the clip alone. */
typedef struct rg_mesh_face_sums_args {
  const double* partial;
  const int* pair_off;
  const int* pair_off_host;
  double* sums;                   /* [n_clips][2] */
  int n_clips;
  int n_groups;
} rg_mesh_face_sums_args;
int rg_mesh_face_sums(rg_handle* h, const rg_mesh_face_sums_args* args_host, void* stream);

/* ---------------------------------------------------------------- SMPL-X clip rendering (rg_render.hip)
 * What mogen/utils/visualization.py:339-440 `render_smplx_debug_video` draws per frame (a mesh of one colour over a
 * checkerboard floor, seen by a pyrender PerspectiveCamera, yfov = pi / 3, aspect = width / height, znear = 0.05, no far plane)
 * as a software rasteriser in three launches over a chunk of frames.  Screen space: x to the right, y DOWN, pixel (px, py) has
 * its centre at (px + 0.5, py + 0.5); positions are int32 fixed point with RG_RENDER_SUBPIXEL_BITS fractional bits, snapped as
 * floor(v * 256 + 0.5) and clamped to +-RG_RENDER_COORD_MAX, so coverage is integer arithmetic and does not depend on float
 * rounding.  The shading is this project's own definition (DESIGN.md "Rendering"), not pyrender's.
 *
 * rg_render_project, per frame and vertex: p_c = R^T (p - t) for the row-major 4 x 4 camera pose [R | t]; view depth
 * z = -p_c.z; screen = ((p_c.x / (z aspect tan(yfov / 2)) + 1) width / 2, (1 - p_c.y / (z tan(yfov / 2))) height / 2), snapped;
 * a vertex with z < znear gets screen (0, 0) and keeps its z (rg_render_bin drops its faces).  normal = the normalised sum over
 * the vertex's faces csr_face[csr_off[v] .. csr_off[v + 1]) (in that order: no atomics) of cross(p1 - p0, p2 - p0), world space;
 * (0, 0, 0) for a vertex without faces or a zero sum. */
#define RG_RENDER_SUBPIXEL_BITS 8
#define RG_RENDER_COORD_MAX (1 << 22)
#define RG_RENDER_TILE 32          /* a raster workgroup owns a 32 x 32 pixel tile */
#define RG_RENDER_BOX_NONE 0x000000ffu
typedef struct rg_render_project_args {
  const float* verts;             /* [frames][n_verts][3] world space */
  const int* faces;               /* [n_faces][3] */
  const int* csr_off;             /* [n_verts + 1] */
  const int* csr_face;            /* [csr_off[n_verts]] face indices, ascending per vertex */
  int* screen;                    /* out [frames][n_verts][2] */
  float* depth;                   /* out [frames][n_verts] view depth */
  float* normal;                  /* out [frames][n_verts][3] */
  float cam[16];                  /* camera pose, row-major (host values) */
  int frames;
  int n_verts;
  int n_faces;
  int width;
  int height;
} rg_render_project_args;
int rg_render_project(rg_handle* h, const rg_render_project_args* args_host, void* stream);

/* Per frame and face: box[frame][face] = the range of tiles its covered pixel centres can fall into, packed
 * tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24, or RG_RENDER_BOX_NONE when the face is dropped: a vertex at depth < znear, a back or
 * degenerate face (front faces are counter-clockwise as the viewer sees them: in the y-down screen coordinates the doubled area
 * (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) of the snapped positions is < 0), or no pixel centre inside its bounds on the screen. */
typedef struct rg_render_bin_args {
  const int* screen;
  const float* depth;
  const int* faces;
  unsigned* box;                  /* out [frames][n_faces] */
  int frames;
  int n_verts;
  int n_faces;
  int width;                      /* <= 255 tiles each way */
  int height;
} rg_render_bin_args;
int rg_render_bin(rg_handle* h, const rg_render_bin_args* args_host, void* stream);

/* One workgroup per tile and frame.  Coverage: with (v0, v1, v2) = the face's vertices 0, 2, 1 (positive area on the y-down
 * screen), pixel centre c is inside when, for each edge a -> b of v1 -> v2, v2 -> v0, v0 -> v1, E = (bx - ax)(cy - ay) - (by - ay)(cx - ax) > 0, or E == 0 and the edge is a top edge (dy == 0,
 * dx > 0) or a left edge (dy < 0): 64-bit integers.  Depth: with b_i = (float)E_i * (1 / (float)area), w = b0 / z0 + b1 / z1 +
 * b2 / z2 (1 / view depth, exactly linear on the screen) in fp32; the face with the largest w wins, the LOWEST face index among
 * equal w (one 64-bit integer maximum per pixel in LDS: no float atomics, no global atomics, the result does not depend on the
 * order).  Frames with active[frame] == 0 draw no face.
 * Resolve (same kernel): mesh pixel: n = normalise(sum b_i normal_i), shade = 0.35 + 0.65 max(0, n . l), l = column 2 of the
 * camera pose (from the surface towards both of the reference's directional lights, which shine along the camera's -Z);
 * rgb = floor(shade * color + 0.5).  Floor (draw_floor != 0): the ray of the pixel centre meets y = floor_y at view depth s > 0;
 * accepted when -6 <= x < 6 and -6 <= z < 6; colour 170 when floor(x + 6) + floor(z + 6) is even, else 120, shaded with the +Y
 * normal by the same formula; it shows where 1 / s > w of the mesh (or there is no mesh).  Otherwise the background, 191.
 * out[frame][py][col + px][3] uint8 with `pitch` pixels per row (two panels can share one [n][H][2W][3] buffer);
 * face_id (optional) [frames][height][width]: the visible mesh face or -1. */
typedef struct rg_render_raster_args {
  const int* screen;
  const float* depth;
  const float* normal;
  const int* faces;
  const unsigned* box;
  const unsigned char* active;    /* [frames] or NULL (all active) */
  unsigned char* out;
  int* face_id;                   /* [frames][height][width] or NULL */
  float cam[16];
  float floor_y;
  float color[3];                 /* 0 .. 255 */
  int draw_floor;
  int frames;
  int n_verts;
  int n_faces;
  int width;
  int height;
  int pitch;                      /* pixels per output row, >= col + width */
  int col;
} rg_render_raster_args;
int rg_render_raster(rg_handle* h, const rg_render_raster_args* args_host, void* stream);

/* ---------------------------------------------------------------- raw SMPL-X recordings -> model inputs (rg_clip.hip)
 * What mogen/datasets/beatx_dataset.py computes on the motion side of a raw BEAT-X recording (poses [n][165], trans [n][3],
 * expressions [n][100] at 30 fps, betas [300]).  Several recordings go through one call as concatenated "raw rows": clip c
 * owns raw rows raw_off[c] .. raw_off[c + 1] and output frames clip_off[c] .. clip_off[c + 1]; output frame t of the clip reads
 * raw row raw_off[c] + t * stride (beatx_dataset.py:354-360 keeps every `stride = 30 // pose_fps`-th frame).  Both tables are
 * checked through their _host copies: they start at 0, do not decrease, raw_off ends at or below raw_rows (the row count of
 * the raw buffers), and a clip of n > 0 frames owns at least (n - 1) * stride + 1 raw rows.
 *
 * rg_smplx_joints_expr: the posed joints of smplx.SMPLX.forward(betas, transl, expression, ...)["joints"][:, :55] as
 * beatx_dataset.py:373-415 (cache_generation) and :206-272 (calculate_mean_velocity) call it.  As rg_smplx_joints (same
 * pose_mean, fold and batch_rodrigues conventions, same chain, one wave per output frame), but the rest joints move with the
 * expression per frame, J_j = rest[c][j] + j_expr[j] . psi (fp32 fma chain over the 100 coefficients; j_expr [55][3][100] =
 * J_regressor @ shapedirs[..., 300:400]; exprs NULL: J = rest), and transl [raw_rows][3] (NULL: none) is added to every joint.
 * Nothing vertex-sized is read or written.  joints [F][55][3], F = clip_off[n_clips]. */
typedef struct rg_smplx_joints_expr_args {
  const float* poses;             /* [raw_rows][165] */
  const float* exprs;             /* [raw_rows][100] or NULL */
  const float* transl;            /* [raw_rows][3] or NULL */
  const float* rest;              /* [n_clips][55][3] */
  const float* j_expr;            /* [55][3][100] (exprs != NULL) */
  const float* pose_mean;         /* [165] or NULL */
  const int* parents;
  const int* parents_host;
  const int* clip_off;
  const int* clip_off_host;
  const int* raw_off;
  const int* raw_off_host;
  float* joints;                  /* [F][55][3] */
  int n_clips;
  int raw_rows;
  int stride;
  int fold;
} rg_smplx_joints_expr_args;
int rg_smplx_joints_expr(rg_handle* h, const rg_smplx_joints_expr_args* args_host, void* stream);
/* Per output frame f (raw row r) of every clip, one workgroup:
 *   motion[f] = poses[r], trans_out[f] = trans[r], facial[f] = exprs[r]                  (beatx_dataset.py:358-360)
 *   upper / lower / hands / face [f][k] = poses[r][part_cols[k']]: part_cols [159] holds the 39 + 27 + 90 + 3 source columns
 *   of the four parts in that order, the `pose[:, mask.astype(bool)]` of :426-440 (the inverse of rg_scatter_joints; copies,
 *   bit-exact; part_cols_host checked: every entry in [0, 165))
 *   contact[f][q], q = joints (7, 8, 10, 11): :417-424 -- feetv = ||joints[f + 1][j] - joints[f][j]||_2 over consecutive
 *   output frames of the SAME clip (fp32: differences, then sqrt(dx dx + dy dy + dz dz) as an fma chain in that order),
 *   contact = feetv < threshold ? 1.0 : 0.0 (the reference: 0.01); a clip's last frame has feetv = 0, so it is 1.
 * joints [F][55][3] are the clips' output frames from rg_smplx_joints_expr with the same tables and stride. */
typedef struct rg_clip_prepare_args {
  const float* poses;             /* [raw_rows][165] */
  const float* trans;             /* [raw_rows][3] */
  const float* exprs;             /* [raw_rows][100] */
  const float* joints;            /* [F][55][3] */
  const int* part_cols;           /* [159] */
  const int* part_cols_host;
  const int* clip_off;
  const int* clip_off_host;
  const int* raw_off;
  const int* raw_off_host;
  float* motion;                  /* [F][165] */
  float* trans_out;               /* [F][3] */
  float* facial;                  /* [F][100] */
  float* upper;                   /* [F][39] */
  float* lower;                   /* [F][27] */
  float* hands;                   /* [F][90] */
  float* face;                    /* [F][3] */
  float* contact;                 /* [F][4] */
  int n_clips;
  int raw_rows;
  int stride;
  float threshold;
} rg_clip_prepare_args;
int rg_clip_prepare(rg_handle* h, const rg_clip_prepare_args* args_host, void* stream);
/* beatx_dataset.py:272-288 (calculate_mean_velocity) per clip of joints [F][55][3] (clip_off [n_clips + 1], clip_off_host
 * checked, every clip >= 2 frames): velocity = forward difference over dt at the first frame, central over 2 dt in the middle,
 * backward over dt at the last (fp32), its norm per joint (fp32), sums[c][j] = the sum over the clip's frames in fp64.  One
 * workgroup per clip, a fixed order that depends on the clip alone (no atomics).  The caller adds the clips' sums and divides
 * by the total frame count (the np.mean of :288). */
typedef struct rg_joint_speed_args {
  const float* joints;
  const int* clip_off;
  const int* clip_off_host;
  double* sums;                   /* [n_clips][55] */
  int n_clips;
  float dt;
} rg_joint_speed_args;
int rg_joint_speed_sums(rg_handle* h, const rg_joint_speed_args* args_host, void* stream);

/* ---------------------------------------------------------------- foot skating and contact planting (csrc/rg_foot.hip)
 * This project's own: the reference neither scores foot sliding nor reads the four contact flags its lower-body VAE decodes
 * (the skating ratio follows Guided Motion Diffusion).  Both entry points take joints [F][55][3]
 * (world positions: the forward kinematics WITH the translation, rg_smplx_joints_expr; up is y), the clips' row table clip_off
 * [n_clips + 1] (clip_off_host: the same on the host, checked) and look at the foot joints k = (7, 8, 10, 11) only.  A pair is
 * (t, t + 1) inside a clip; flag contact[t][k] ([F][4]) belongs to pair (t, t + 1), as rg_clip_prepare makes it, and a clip's
 * last flag is not read.  All arithmetic is fp64 on the fp32 inputs.  One workgroup of 256 threads per clip walks its pairs in
 * tiles of 256: a clip's result depends on that clip alone.  No atomics, no workspace.
 *
 * rg_foot_skate_sums: per clip RG_FOOT_SUMS doubles.  With h[t][k] = y[t][k] - min_t y[t][k] (height above the joint's own lowest
 * point in the clip), a joint-pair is GROUNDED when h[t][k] < height and h[t + 1][k] < height, s = fps sqrt(dx^2 + dz^2) its
 * horizontal speed, d = |p[t + 1][k] - p[t][k]| its 3-D displacement, and it is FLAGGED when contact[t][k] >= contact_thr:
 *   0 pairs (n - 1)                                            4 flagged joint-pairs
 *   1 pairs in which any joint is grounded with s > speed      5 sum of d over flagged joint-pairs
 *   2 grounded joint-pairs                                     6 flagged joint-pairs with d >= move_thr
 *   3 sum of s over grounded joint-pairs
 * contact == NULL: entries 4 to 6 are 0.  The sums are added in a fixed order: the lanes of a wave (xor butterfly), the waves
 * 0 to 3, the tiles in order.
 *
 * rg_foot_plant: only the translation changes.  With S_t = {k : contact[t][k] >= contact_thr}: off[0] = 0, off[t + 1] = off[t]
 * when S_t is empty, else off[t] - mean_{k in S_t} (p[t + 1][k] - p[t][k]) in x and z; trans_out[t] = fp32(trans_in[t] + off[t])
 * in x and z, trans_out[t].y = trans_in[t].y bit for bit.  trans_in / trans_out [F][3]; trans_out may alias trans_in.  The
 * prefix sum runs inside a wave by shuffles, across the waves in order through LDS, from tile to tile in a register.
 *
 * Refused before the launch: null pointers, n_clips < 1, clip_off not starting at 0 or decreasing, an empty clip, clip_off[n_clips]
 * >= 2^31 / 165, thresholds that are not numbers, fps <= 0. */
#define RG_FOOT_SUMS 7
int rg_foot_skate_sums(rg_handle* h, const float* joints, const float* contact /* nullable */,
                       const int* clip_off, const int* clip_off_host, int n_clips,
                       float fps, float height, float speed, float contact_thr, float move_thr,
                       double* sums /* [n_clips][RG_FOOT_SUMS] */, void* stream);
int rg_foot_plant(rg_handle* h, const float* joints, const float* contact, const float* trans_in,
                  const int* clip_off, const int* clip_off_host, int n_clips,
                  float contact_thr, float* trans_out, void* stream);

/* ---------------------------------------------------------------- contact ankles locked by leg IK (csrc/rg_footlock.hip)
 * This project's own: the reference has no counterpart.  The root path stays as predicted; each flagged
 * ANKLE is pinned to one world position for the length of its contact and the leg is re-solved analytically.  Legs are (hip,
 * knee, ankle) = (1, 4, 7) and (2, 5, 8); the ankle flags are contact[t][0] and contact[t][1], the toe flags [2], [3] are NOT
 * read.  Flag c[t] belongs to the pair (t, t + 1); a clip's last flag is not read.  p[t] is the ankle's world position (joints
 * [F][55][3] from rg_smplx_joints_expr WITH the translation), taken to fp64; all arithmetic below is fp64, nothing contracted.
 *
 * rg_foot_lock_targets, per clip of n frames and per ankle:
 *   member   m[t] = (t <= n - 2 and c[t] >= contact_thr) or (t >= 1 and c[t - 1] >= contact_thr); a RUN is a maximal interval
 *            [s, e] of member frames
 *   anchor   A = (sum over t in [s, e] of p[t]) / (e - s + 1), per coordinate
 *   offset   member frame: d[t] = A - p[t].  Other frames: with e the last member frame before t and s' the first after it
 *            (either may be absent: weight 0), w(k) = max(0, 1 - k / (blend + 1)), w1 = w(t - e), w2 = w(s' - t):
 *            d[t] = (w1 d[e] + w2 d[s']) / max(1, w1 + w2).  blend = 0: zero outside the runs.
 *   offsets [F][2][3] fp64 (the target of the ankle is p[t] + d[t]); stats [n_clips][RG_FOOT_LOCK_STATS] fp64:
 *     0 member ankle-frames   1 runs   2 ankle-frames with a non-zero offset
 *     3 sum of |d| over the member ankle-frames   4 max of |d| over them   (|d| = sqrt((dx^2 + dy^2) + dz^2))
 * One workgroup of 256 threads per clip walks 256-frame tiles twice: forward (segmented sums and counts of the runs, the
 * previous run's end) and backward (the run's anchor from its last frame, the next run's start), scans inside a wave by
 * shuffles, across the waves in order through LDS, from tile to tile in registers; between the two walks the offsets buffer
 * holds the forward results.  A fixed order, no atomics, no workspace beyond the outputs; a clip's result depends on that
 * clip alone; any n >= 1.
 *
 * rg_foot_lock_ik, per frame and leg, only where d[t] != 0 (else the leg's 9 channels are copied): the forward kinematics of
 * rg_smplx_joints_expr (csrc/rg_smplx.h: stride 1, no expression, no fold; fp32) gives world rotations W_j and positions a, b,
 * c of hip, knee, ankle; then in fp64, T = c + d, l1 = |b - a|, l2 = |c - b|:
 *   dist = clamp(|T - a|, |l1 - l2| (1 + 1e-3) + 1e-9, stretch (l1 + l2))
 *   A0 = angle(c - a, b - a), K0 = angle(a - b, c - b)            (angle(u, v) = atan2(|u x v|, u . v))
 *   A1 = acos((l1^2 + dist^2 - l2^2) / (2 l1 dist)), K1 = acos((l1^2 + l2^2 - dist^2) / (2 l1 l2)), arguments clamped to [-1, 1]
 *   n0 = normalize((c - a) x (b - a)); |(c - a) x (b - a)| < 1e-5 |c - a| |b - a| (a straight leg): n0 = normalize(W_hip (1, 0, 0))
 *   B0 = rot(n0, A1 - A0), B1 = rot(n0, K1 - K0)
 *   n1 = normalize((c - a) x (T - a)), S = rot(n1, angle(c - a, T - a)); |(c - a) x (T - a)| < 1e-12 |c - a| |T - a|: S = I
 *   W_hip' = S B0 W_hip, W_knee' = S B0 B1 W_knee, W_ankle' = W_ankle (the foot keeps its world orientation)
 *   new axis-angles = log(W_parent(hip)^T W_hip'), log(W_hip'^T W_knee'), log(W_knee'^T W_ankle), angle in [0, pi], minus the
 *   joint's pose_mean; stored as fp32.  A target out of reach is approached along the hip-target line and not met.
 * poses_out [F][165]: every other channel, and every frame whose two offsets are zero, is copied bit for bit; poses_out may
 * alias poses.  reach [F][2] fp32 = |T - a| / (l1 + l2), 0 where nothing was solved.  The translation is only read.  One wave
 * per frame, four frames per workgroup; lanes 0 and 1 solve the two legs.  rest [n_clips][55][3], pose_mean [165] or NULL,
 * parents / parents_host [55] (checked: joint 0 the root, parents[j] in [0, j), and the legs 1-4-7 and 2-5-8 are chains).
 *
 * Refused before the launch: null pointers, n_clips < 1, clip_off not starting at 0 or decreasing, an empty clip, clip_off[n_clips]
 * >= 2^31 / 165, a contact_thr that is not a number, blend < 0, stretch outside (0, 1] or not a number. */
#define RG_FOOT_LOCK_STATS 5
int rg_foot_lock_targets(rg_handle* h, const float* joints, const float* contact,
                         const int* clip_off, const int* clip_off_host, int n_clips,
                         float contact_thr, int blend,
                         double* offsets /* [F][2][3] */, double* stats /* [n_clips][RG_FOOT_LOCK_STATS] */, void* stream);
int rg_foot_lock_ik(rg_handle* h, const float* poses, const float* transl, const float* rest,
                    const float* pose_mean /* nullable */, const int* parents, const int* parents_host,
                    const int* clip_off, const int* clip_off_host, int n_clips,
                    const double* offsets, float stretch,
                    float* poses_out, float* reach /* [F][2] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RG_GESTURE_H */
