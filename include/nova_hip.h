/*
 * nova_hip.h — C ABI of libnova_hip.so, the MI355X (gfx950) implementation of NOVA's
 * autoregressive point-set generation hot path.
 *
 * The reference (zailaiyiwan123/NOVA_pointcloud, `diffnext`) is pure Python and has no FFI of its
 * own; its kernel boundary is "whatever torch op a module's forward() calls". Each entry point
 * below therefore replaces a group of torch calls, cited as reference file:line (paths relative
 * to the reference's repository root). The drop-in `diffnext` package shipped in
 * nova_pointcloud_amd/diffnext binds these through ctypes (see INTEGRATION.md for the stub a
 * maintainer of the reference would add).
 *
 * Conventions
 *   - plain C: raw device pointers + sizes; no torch / HIP types in signatures. `stream` is a
 *     hipStream_t passed as void* (NULL = the legacy default stream). All work is enqueued on that
 *     stream; nothing synchronises, allocates or frees; buffers are caller-owned.
 *   - every function returns 0 on success or a negative nova_status; nova_last_error() returns a
 *     thread-local message for the last failure. Nothing throws.
 *   - dtype: storage type of activations and GEMM weights (NOVA_F32 = parity mode on exact-f32
 *     MFMA, NOVA_BF16 / NOVA_F16 = throughput mode on the bf16 / f16 MFMA forms - same kernels, same rate; f16 is the
 *     default precision of the reference's callers, scripts/app_nova_t2i.py:36,87-89. The fp8 GEMM mode and the attention backward take bf16 only;
 *     nova_row_norm_bwd and nova_act_fwd / nova_act_bwd take all three). Biases, LayerNorm affine parameters, RoPE
 *     tables, point coordinates, timesteps and sigmas are always float32; token ids are int64
 *     (torch.long, as the reference's pred_ids / prev_ids).
 *   - row-major everywhere; a "row" is one token's feature vector.
 */
#ifndef NOVA_HIP_H_
#define NOVA_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define NOVA_HIP_VERSION 405 /* still 0.4.5 (tests/test_pointset_fps.py pins the number; a library without the new symbols fails to bind, loudly): nova_pointset_neighbor_aggregate, nova_pointset_neighbor_inverse, nova_pointset_neighbor_aggregate_bwd (kNN neighbourhood feature aggregation, its inverse neighbour list and its backward, for nova_pointcloud_amd.neighbors); nova_pointset_matched_dist, nova_pointset_matched_dist_bwd (the distance of matched pairs under a given permutation and its backward, for the exact-assignment EMD training loss); nova_pointset_kernel_interpolate_stats, nova_pointset_kernel_interpolate_bwd (the interpolation forward with its statistics and its backward, for nova_pointcloud_amd.sampling); nova_pointset_nearest_match, nova_pointset_nearest_match_bwd (nearest match with indices and its backward, for the Chamfer-type training losses); nova_pointset_knn (exact k nearest neighbours of a cloud set); nova_pointset_assignment, nova_pointset_assignment_state_bytes, nova_pointset_assignment_rounds (optimal assignment of two clouds by a batched integer auction: the exact EMD on the GPU); 0.4.5: nova_pointset_farthest_point_sample (farthest point sampling of a cloud set, to bring sets to a common point count); 0.4.4: nova_pointset_occupancy_grid (occupancy grid of a cloud set for the JSD metric); 0.4.3: nova_pointset_emd_matrix (all-pairs approxmatch EMD matrix for MMD / COV / 1-NNA); 0.4.2: nova_pointset_chamfer_matrix (all-pairs Chamfer matrix for MMD / COV / 1-NNA); 0.4.1: nova_decoder_denoise_echo (guidance renorm with any sampler step); 0.4.0 (round 4): the loader checks this number against its own; nova_attn_fwd_lse / nova_attn_bwd carry a key_limit pointer before the stream, nova_row_norm_bwd, nova_act_fwd, nova_act_bwd, nova_debug_drop_graphs (all added after 0.3.0 without a bump), nova_prof slots 7-9; 0.3.0: NOVA_F16 storage mode through every dtype-taking entry, nova_row_norm_chain takes a dtype, nova_debug_set_attn_variant; 0.2.2: nova_attn_fwd_lse, nova_attn_bwd; 0.2.1: nova_adaln_fc1, nova_row_norm_chain (0.2.0: 3-pass guidance fields in nova_sampler_step, KV-cached block stack, nova_modulate_rows) */

typedef enum { NOVA_F32 = 0, NOVA_BF16 = 1, NOVA_F16 = 2 } nova_dtype;
typedef enum { NOVA_ACT_NONE = 0, NOVA_ACT_GELU_ERF = 1, NOVA_ACT_SILU = 2 } nova_act;
typedef enum {
  NOVA_OK = 0,
  NOVA_ERR_ARG = -1,    /* bad enum / null pointer */
  NOVA_ERR_SHAPE = -2,  /* shape not supported by the built kernels */
  NOVA_ERR_LAUNCH = -3, /* HIP launch error */
  NOVA_ERR_DEVICE = -4  /* no gfx950 device */
} nova_status;

int nova_version(void);
const char* nova_last_error(void);
/* 0 when a gfx950 device is current, NOVA_ERR_DEVICE otherwise (checked once by the loader). */
int nova_check_device(void);

/* ---- measurement hooks (bench.py): HIP-event timing of the GEMM / attention / row-norm launches on
 * the stream they are launched on. nova_prof_enable(1) starts recording; nova_prof_collect waits
 * for the recorded events and returns, per slot, summed milliseconds, summed algorithmic work
 * (FLOPs for slots 0-4 and 6, bytes for slot 5) and launch counts, then clears the record.
 * Slots 0-3: the large-M (256x256 tile) GEMM kernel by epilogue - 0 bias with K <= N (the out-projection), 1 bias+GELU, 2 bias+SiLU,
 * 3 qkv+RoPE; 4 attention, 5 row_norm, 6 the small-M (128x128 tile / whole-K) GEMM kernels with any epilogue (decoder, embeddings),
 * 7 the large-M GEMM, bias only, K > N (the MLP's second projection), 8 token plumbing (canvas embedding, sequence build / scatter,
 * RoPE table, KV append, frame mixer, fp8 row quantisation; work = 0), 9 the diffusion MLP's glue kernels (work = 0). */
#define NOVA_PROF_SLOTS 10
int nova_prof_enable(int on);
int nova_prof_collect(double* ms, double* work, long long* launches, int slots);

/* Test hook: 0 = automatic choice between the GEMM structures by shape, 16 = the small-M whole-K kernel (bf16, K 768 /
 * 1024; an error for other shapes; 161 / 162 / 164 = the same with 16 / 32 / 64 rows per workgroup), 128 / 256 = force the 128x128 or the 256x256 (large-M, persistent) structure,
 * 257 = the 256 structure in its one-tile-per-workgroup form (the fallback of the persistent kernel); all compute
 * bit-identical results (tests/test_gpu_kernels.py compares them). Per calling thread. */
int nova_debug_force_gemm_tile(int tile);

/* Test / A-B hook: which structure the bf16, head_dim 64 attention launches for the calling thread: 0 = 32x32x16 MFMA,
 * 32 query rows per wave; 1 = 16x16x32 MFMA, 32 rows per wave; 2 = 16x16x32 MFMA, 64 rows per wave; 3 / 4 = 1 / 2 with the softmax row sums taken on the matrix pipe (an
 * all-ones V^T block) instead of vector adds; -1 = the shipped default. Same algorithm in all three (tests/test_gpu_kernels.py compares each with the f32 reference and with each other). */
int nova_debug_set_attn_variant(int variant);

/* nova_decoder_denoise replays its launch sequence as a hipGraph, captured once per distinct argument set (on by
 * default; environment NOVA_GRAPHS=0 or on = 0 here switches to direct launches for every thread and drops the cached graphs -
 * the calling thread's at once, every other thread's at its next nova_decoder_denoise). Results are identical either way. Stats: graphs captured / replayed by the calling thread. */
int nova_debug_set_graphs(int on);
int nova_debug_graph_stats(long* captures, long* replays);
/* Drops the calling thread's cached graphs (a caller that re-allocates the workspaces it passes to nova_decoder_denoise: graphs keyed
 * by the old addresses can never be replayed and would only pile up until the 2048-entry cap). */
int nova_debug_drop_graphs(void);

/* ---- projection GEMM -----------------------------------------------------------------------
 * out[M,N] = act(A[M,K] * W[N,K]^T + bias[N])        W in nn.Linear layout.
 * Replaces nn.Linear (+ nn.GELU() / nn.SiLU()) at vision_transformer.py:33-38 (MLP.fc1/fc2),
 * :64 (Attention.proj), diffusion_mlp.py:31-36 (Projector), normalization.py:28,35
 * (AdaLayerNormZero.proj), embeddings.py:174,203-206 (TextEmbed.proj).
 * Needs N % 128 == 0 and K % (128 / sizeof(dtype)) == 0; any M >= 0. */
int nova_gemm_bias_act(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int act,
                       int dtype, void* stream);

/* ---- MX-fp8 projection GEMM (BASELINE configs[4]: d48w1536 "fp8 MFMA path"; the reference has no fp8 path, so this is
 * compared with the bf16 result of the same layer) ---------------------------------------------
 * nova_quantize_rows_fp8: per-row dynamic quantisation of bf16 rows to OCP e4m3, scale[r] = max|x[r]| / 448.
 * nova_gemm_fp8_bias_act: out_bf16[M,N] = act((A8[M,K] . W8[N,K]^T) * a_scale[m] * w_scale[n] + bias[n]) on
 * v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales); N % 256 == 0, K % 128 == 0. Replaces the same nn.Linear
 * calls as nova_gemm_bias_act (vision_transformer.py:33-38,64) with quantised operands. */
int nova_quantize_rows_fp8(const void* x_bf16, void* out_fp8, float* scale, long long rows, int D, void* stream);
int nova_gemm_fp8_bias_act(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const float* bias,
                           void* out_bf16, int M, int N, int K, int act, void* stream);

/* ---- fused QKV projection + 3-D RoPE -------------------------------------------------------
 * qkv[S*L, 3D] = x[S*L, D] * Wqkv^T + b, then q and k (columns [0, 2D)) rotated pairwise with
 * rope[(s % rope_batch), l, pair] = (cos, sin). rope == NULL: no rotation (abs-PE models).
 * Replaces vision_transformer.py:52-54 (qkv Linear, view/permute/unbind, pe_func on q and k) and
 * embeddings.py:36-43 (RotaryEmbed3D.ApplyFunc). The head split is never materialised: the
 * attention kernel reads q/k/v in place from this buffer. */
int nova_qkv_rope(const void* x, const void* Wqkv, const float* bias, const float* rope, void* qkv, int S, int L, int D,
                  int heads, int rope_batch, int dtype, void* stream);

/* Generalisation used for the last encoder block, whose output is only consumed at the rows predicted in the
 * current AR step (transformer_3d.py:129-132 -> diffusion_mlp.py:93): out[M,N] = x[M,K] W[N,K]^T + bias with columns
 * [0, rope_cols) rotated by rope[(m / L) % rope_batch, m % L] (heads of width head_dim). The engine calls it once with
 * the K|V rows of attn.qkv.weight over all tokens (rope_cols = D) and once with the Q rows over the n gathered rows. */
int nova_qkv_rope_cols(const void* x, const void* W, const float* bias, const float* rope, void* out, int M, int N, int K,
                       int L, int rope_batch, int head_dim, int rope_cols, int dtype, void* stream);

/* rope[nb, pad + n_tok, hd/2, 2] from integer grid positions (embeddings.py:59-67 get_func):
 * pos [n_pos,3] (t,h,w); ids [nb,n_tok] int64 gathers token -> position (NULL: identity);
 * the first `pad` rows (condition prefix) sit at position 0; inv_freq [hd/2] = 1 / theta^scale
 * laid out axis t, h, w (embeddings.py:48-50,63-64). */
int nova_rope_table(const float* pos, const long long* ids, float* rope, int nb, int pad, int n_tok, int n_pos, int hd,
                    const float* inv_freq, void* stream);

/* ---- attention ------------------------------------------------------------------------------
 * o[s, i, h, :] = softmax_j(q[s,i,h,:] . k[s,j,h,:] * scale) v[s,j,h,:], non-causal, no mask.
 * Element (s, l, head, c) of q lives at q + (s*Lq + l)*q_row_stride + head*head_dim + c (same
 * for k/v with Lk / kv_row_stride, o with o_row_stride); strides in elements, 16-byte multiples.
 * Replaces F.scaled_dot_product_attention at vision_transformer.py:63 and the
 * transpose(1,2).flatten(2) merge at :64. head_dim 64 (d48w768, d48w1024) and 96 (d48w1536) are built.
 * Non-finite inputs: the 16-bit kernels are compiled without NaN-honouring max / compare instructions. A query row whose scores
 * contain a NaN or overflow to +inf yields a non-finite output row (as SDPA's softmax would); all other output rows are
 * bit for bit those of the same call without the offending values (tests/test_gpu_kernels.py::
 * test_attention_non_finite_rows_stay_in_their_row). -inf scores do not occur (no mask input). */
int nova_attn_fwd(const void* q, const void* k, const void* v, void* o, int S, int heads, int Lq, int Lk, int head_dim,
                  long q_row_stride, long kv_row_stride, long o_row_stride, float scale, int dtype, void* stream);

/* Training path of the same attention (bf16, head_dim 64 or 96; Lq = Lk = L). q must already be multiplied by
 * scale * log2(e) (what the fused QKV epilogue does for the generation path); the forward also writes
 * lse[s, head, l] = log2 sum_j 2^(q~_l . k_j), the backward rebuilds P from it (flash-style, nothing of size L x L is
 * stored) and returns the gradients w.r.t. the UNSCALED q, k and v; it needs the forward's o for delta[s, head, l] =
 * sum_c dO * O, which it writes into delta_scratch [S, heads, L] f32 first. All matrices token-major with row strides
 * as above. key_limit (NULL = no mask): int32 [L], non-decreasing, >= 1 - query l attends to keys [0, key_limit[l]); this is the
 * reference's block-causal frame mask of multi-frame training (`MaskEmbed.get_attn_mask`, embeddings.py:247-260, set on the
 * video encoder's blocks at transformer_3d.py:176-177: a token sees the tokens of frames <= its own, the prefix counting as
 * frame 0), passed as the end of each token's visible range instead of an L x L matrix. Replaces the autograd of
 * F.scaled_dot_product_attention at vision_transformer.py:63 inside the training forward (transformer_3d.py:79-100). */
int nova_attn_fwd_lse(const void* q_scaled, const void* k, const void* v, void* o, float* lse, int S, int heads, int L,
                      int head_dim, long qkv_row_stride, long o_row_stride, const int* key_limit, void* stream);
int nova_attn_bwd(const void* q_scaled, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                  float* delta_scratch, void* dq, void* dk, void* dv, int S, int heads, int L, int head_dim,
                  long qkv_row_stride, long o_row_stride, long do_row_stride, long dqkv_row_stride, float scale,
                  const int* key_limit, void* stream);

/* The same two calls for cross-attention, Lq queries against Lk keys (bf16, head_dim 64 or 96): the reference's
 * nn.MultiheadAttention(embed_dim, num_heads, batch_first=True) of EdgeAligner (transformer_pointcloud_nova.py:164), called with
 * query = the current subset's edge features and key = value = the concatenated edge features of the subsets generated so far
 * (:211-215), and the one of AutoregressiveDiffusion (:236) over all generated subsets (:265-269). The same kernels, with the
 * lengths and the row strides of the two sides passed apart: q, o, dO and dq are [S, Lq, heads * head_dim] rows with strides
 * q_row_stride, o_row_stride, do_row_stride and dq_row_stride; k, v are [S, Lk, ...] rows with kv_row_stride, dk and dv with
 * dkv_row_stride (strides in elements, 16-byte multiples; Lq * q_row_stride, Lq * o_row_stride, Lq * do_row_stride and
 * Lk * kv_row_stride each below 2 GiB in bytes). q_scaled, lse, the formulas and the factor conventions are those above with
 * the sum over j running to Lk: lse and delta_scratch are [S, heads, Lq] f32; dq is the gradient of the UNSCALED q [Lq rows],
 * dk and dv have Lk rows. key_limit (NULL = no mask): int32 [Lq], non-decreasing, each in [1, Lk] - query l attends to keys
 * [0, key_limit[l]). dk / dv rows of keys that no query sees are written as 0; nothing is written past row Lq / Lk or outside
 * a head's columns. With Lq == Lk and equal strides on both sides the two calls return the bits of nova_attn_fwd_lse /
 * nova_attn_bwd (tests/test_gpu_attn_cross.py). Refused before any launch: null pointers (NOVA_ERR_ARG); head_dim other than 64
 * or 96, strides that are not 16-byte multiples, Lk <= 0 with Lq > 0, a span of 2 GiB or more, a grid above 2^31 - 1 workgroups
 * (NOVA_ERR_SHAPE). S == 0 or Lq == 0 launches nothing and returns 0. */
int nova_attn_cross_fwd_lse(const void* q_scaled, const void* k, const void* v, void* o, float* lse, int S, int heads, int Lq, int Lk,
                            int head_dim, long q_row_stride, long kv_row_stride, long o_row_stride, const int* key_limit,
                            void* stream);
int nova_attn_cross_bwd(const void* q_scaled, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                        float* delta_scratch, void* dq, void* dk, void* dv, int S, int heads, int Lq, int Lk, int head_dim,
                        long q_row_stride, long kv_row_stride, long o_row_stride, long do_row_stride, long dq_row_stride,
                        long dkv_row_stride, float scale, const int* key_limit, void* stream);

/* ---- training side, pointwise -------------------------------------------
 * The activation between the two projections of an MLP, forward and backward, n contiguous elements of `dtype`
 * (n a multiple of 16 bytes' worth: 4 floats / 8 16-bit values), arithmetic in f32:
 *   kind NOVA_ACT_GELU_ERF: y = 0.5 x (1 + erf(x / sqrt 2)), the exact form of nn.GELU() the reference trains with
 *                           (vision_transformer.py:33-38); dx = dy (Phi(x) + x phi(x))
 *   kind NOVA_ACT_SILU:     y = x / (1 + e^-x) (the decoder MLP, diffusion_mlp.py:33,36; SiLU(z) of AdaLayerNormZero,
 *                           normalization.py:32,35); dx = dy s (1 + x (1 - s)), s = 1 / (1 + e^-x)
 * The forward keeps nothing but x; the backward recomputes the slope from it. */
int nova_act_fwd(const void* x, void* y, long long n, int kind, int dtype, void* stream);
int nova_act_bwd(const void* x, const void* dy, void* dx, long long n, int kind, int dtype, void* stream);

/* ---- training: backward of the LayerNorm family --------------------------------------------------------------------
 * For y = LN(x; eps) [* gamma + beta] [* (1 + scale) + shift] [* gate] [+ res] (nova_row_norm's forward) and the output
 * gradient dy [rows, D]: dx [rows, D]; d_scale / d_shift / d_gate written into dmod [rows, mod_ld] at the forward's offsets
 * (dmod may be NULL when mod is); the parameter gradients as `parts` partial rows d_gamma_part / d_beta_part [parts, D] f32
 * that the caller sums over dim 0 (one row per wave of the launch: parts % 4 == 0, parts / 4 workgroups; no atomics, so
 * the result is bitwise reproducible); d_res = dy is the caller's. Statistics are recomputed from x. Replaces the
 * autograd of nn.LayerNorm + residual in Block.forward (vision_transformer.py:78-82,91-92), of AdaLayerNormZero.forward
 * (normalization.py:34-36) and of DiffusionBlock's `norm2(h) * gate + x` (diffusion_mlp.py:52-53) in the training
 * forward/backward (transformer_3d.py:79-100,166-190). */
int nova_row_norm_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const void* mod, long mod_ld,
                      int scale_off, int shift_off, int gate_off, void* dx, void* dmod, float* dgamma_part, float* dbeta_part,
                      int parts, long rows, int D, float eps, int dtype, void* stream);

/* ---- LayerNorm family -----------------------------------------------------------------------
 * y = LN(in[gather ? gather[r] : r]; eps) [* gamma + beta] [* (1 + mod[r, scale_off..]) +
 * mod[r, shift_off..]] [* mod[r, gate_off..]] [+ res[r]] -> out[r]. Offsets < 0 disable a term.
 * in is indexed by source row, res and mod by output row. Every term's D columns lie inside a
 * modulation row: off + D <= mod_ld, NOVA_ERR_SHAPE otherwise (nova_row_norm_chain and
 * nova_row_norm_bwd refuse the same).
 * Replaces: Block post-norm residual `norm(attn(x)).add_(x)` vision_transformer.py:78-82,91-92;
 * AdaLayerNormZero.forward normalization.py:34-36; DiffusionBlock `norm2(proj(h)).mul(gate)
 * .add_(x)` diffusion_mlp.py:52-53; final encoder norm vision_transformer.py:146 fused with the
 * pred_ids row gather of diffusion_mlp.py:93; TextEmbed.norm embeddings.py:203-206. */
int nova_row_norm(const void* in, void* out, const float* gamma, const float* beta, const void* mod, long mod_ld,
                  int scale_off, int shift_off, int gate_off, const void* res, const int* gather, long rows, int D,
                  float eps, int dtype, void* stream);

/* Two chained row norms of the diffusion MLP in one pass over bf16 rows: x_new = (LN(g) gamma + beta) * mod[:, gate_off:+D]
 * + x (eps_first; DiffusionBlock's `norm2(proj(h)).mul(gate).add_(x)`, diffusion_mlp.py:52-53), then h = LN(x_new)(1 +
 * mod[:, scale_off:+D]) + mod[:, shift_off:+D] (eps_second, no affine; the next block's or the final layer's modulate,
 * diffusion_mlp.py:41-43,96-97 / normalization.py:34-36). The second norm reads x_new as stored (rounded to bf16), so the
 * result equals nova_row_norm twice, bit for bit. x_new_out may be NULL (x not needed afterwards: the last block). */
int nova_row_norm_chain(const void* g, const void* x, const float* gamma, const float* beta, const void* mod, long mod_ld,
                        int gate_off, int scale_off, int shift_off, float eps_first, float eps_second, void* x_new_out,
                        void* h_out, long rows, int D, int dtype, void* stream);

/* out = act(h W^T + bias) with h = LN(x)(1 + mod[:, scale_off:+D]) + mod[:, shift_off:+D], LN without affine: the first
 * half of DiffusionBlock.forward, `self.proj(self.norm1(x, z)...)` up to the activation (diffusion_mlp.py:41-47 with
 * AdaLayerNormZero normalization.py:34-36 and the Projector's fc1 + SiLU diffusion_mlp.py:31-36). For bf16 rows of width
 * 768 / 1024 and a few hundred rows (the per-step launches of the denoising loop at small batch) this is ONE launch with
 * the modulate as the GEMM's prologue; otherwise it runs as nova_row_norm into `h` followed by nova_gemm_bias_act, and
 * both forms give bit-identical `out`. `h` [rows, D] is scratch (written only by the two-launch form). */
int nova_adaln_fc1(const void* x, const void* mod, long mod_ld, int scale_off, int shift_off, float eps, const void* w,
                   const float* bias, void* h, void* out, long rows, int N, int D, int act, int dtype, void* stream);

/* ---- token plumbing of the masked-autoregressive encoder ------------------------------------
 * z0 = MaskEmbed(PatchEmbed(canvas)) (+ abs-PE): embeddings.py:160-166,272-274,90-91.
 * canvas [B,N,P] f32 patchified points, mask [B,N] f32 (1 = unknown), w [D,P] patchified order. */
int nova_embed_canvas(const float* canvas, const float* mask, const void* w, const float* bias, const void* mask_token,
                      const void* pos_embed, void* z0, int B, int N, int P, int D, int dtype, void* stream);
/* x[s] = cat(prefix[s] (Lp rows), tokens[s % B][ids]) : vision_transformer.py:133-136 (gather by
 * prev_ids + torch.cat). ids NULL = all n_sel tokens in order. tok_batch_rows 0 = shared tokens. */
int nova_build_sequence(const void* prefix, long prefix_seq_rows, const void* tokens, long tok_batch_rows,
                        const long long* ids, void* x, int S, int B, int Lp, int n_sel, int D, int dtype, void* stream);
/* x2[s][Lp + ids[s % B][j]] = x1[s][Lp + j] : x_masked.scatter(1, prev_ids, x) vision_transformer.py:141-143 */
int nova_scatter_tokens(const void* x1, const long long* ids, void* x2, int S, int B, int Lp, int N, int n_prev, int D,
                        int dtype, void* stream);

/* ---- diffusion-MLP glue ----------------------------------------------------------------------
 * silu(a + rowvec): the SiLU in front of every AdaLN projection with z = cond + time
 * (normalization.py:35, diffusion_mlp.py:73-75). rowvec may be NULL. */
int nova_silu_add_rows(const void* a, const void* rowvec, void* out, long rows, int D, int dtype, void* stream);
/* sinusoidal timestep features [n, freq_dim] = [cos(t f) ; sin(t f)] : diffusion_mlp.py:65-71 */
int nova_timestep_freq(const float* t, const float* freq, void* out, int n, int freq_dim, int dtype, void* stream);
/* u[s, j] = W x[s % B, j] + b for the n tokens being denoised: diffusion_mlp.py:89-92 */
int nova_patch_embed_rows(const float* x, const void* w, const float* bias, void* out, int S, int B, int n, int P, int D,
                          int dtype, void* stream);
/* head Linear + CFG combine + flow-matching Euler step on x [B,n,P] f32 in place:
 * diffusion_mlp.py:98, guidance_scaler.py:86-87, scheduling_cfm.py:134-136. h = [2B*n, D]
 * (cond rows then uncond rows) when cfg != 0, [B*n, D] otherwise. */
int nova_head_cfg_euler(const void* h, const void* w, const float* bias, float* x, int B, int n, int P, int D,
                        float guidance, int cfg, float dt, int dtype, void* stream);

/* ---- point-set metrics (the step after generation) ------------------------------------------
 * x [B, N, 3], y [B, M, 3] float32 point sets (NOVAPipeline's latent output flattened to points). Coordinates are clamped to
 * [clamp_lo, clamp_hi] first, as the reference does before torch.cdist (test_optimize.py:357-358,388-389: +-5;
 * train_newloss.py:321-322,357-358: +-1 / +-2).
 *   nova_pointset_nn_dist        d[b, i] = min_j ||x[b, i] - y[b, j]||  (Euclidean, not squared): the `dist.min(dim=2)`
 *                                of compute_chamfer_distance (test_optimize.py:367-369); call it twice, operands swapped, for
 *                                the two directions. unit_norm != 0 scales every point to unit length after the clamp
 *                                (distChamfer, train_newloss.py:325-337).
 *   nova_pointset_pairwise_dist  D[b, i, j] = ||x[b, i] - y[b, j]||: the cost matrix `torch.cdist(pred[i], target[i])`
 *                                handed to scipy's linear_sum_assignment by compute_emd_distance (test_optimize.py:399-404)
 *                                and emd_approx (train_newloss.py:360-370). */
int nova_pointset_nn_dist(const float* x, const float* y, float* d, int B, int N, int M, float clamp_lo, float clamp_hi,
                          int unit_norm, void* stream);
int nova_pointset_pairwise_dist(const float* x, const float* y, float* D, int B, int N, int M, float clamp_lo, float clamp_hi,
                                void* stream);
/* cd[a * ldc + b] = CD(x[a], y[b]) for x [A, N, 3] and y [B, M, 3] float32 clouds (any N, M, A, B >= 1), with
 *   CD(X, Y) = mean_{p in X} min_{q in Y} |p - q|^2 + mean_{q in Y} min_{p in X} |p - q|^2
 * in squared Euclidean distances, no clamp and no normalisation: the Chamfer distance of the set-level metrics (MMD,
 * COV, 1-NNA) of the point-cloud generation literature (PointFlow and its successors), NOT the density-weighted
 * compute_chamfer_distance above. symmetric != 0 (needs x == y, A == B, N == M) computes the pairs a <= b only and writes
 * each value to both cd[a, b] and cd[b, a]. One workgroup writes each entry and every reduction runs in a fixed order:
 * an entry does not depend on how the caller splits the pair grid. Coordinates must be finite and of magnitude << 1e18. */
int nova_pointset_chamfer_matrix(const float* x, const float* y, float* cd, int A, int B, int N, int M, int ldc, int symmetric,
                                 void* stream);
/* emd[a * ldc + b] = EMD(x[a], y[b]) for x [A, N, 3] and y [B, N, 3] float32 clouds of the same point count,
 * 1 <= N <= NOVA_EMD_MAX_POINTS: the EMD of the set-level metrics (MMD, COV, 1-NNA) of the point-cloud generation
 * literature, which is not the exact assignment but the approximate matching of Fan et al. ("approxmatch") followed by
 * its match cost, divided by n (PointFlow's emd_approx). For X = {p_k}, Y = {q_l} and d2[k, l] = |p_k - q_l|^2
 * (squared Euclidean, float32 input used as given, no clamp and no normalisation):
 *   remainL[k] = 1, remainR[l] = 1, cost = 0
 *   for j in 7, 6, 5, 4, 3, 2, 1, 0, -1, -2:                  # 10 levels
 *       level = -(4 ** j)            (j = -2: level = 0)       # -16384, -4096, ..., -0.25, 0
 *       E[k, l] = exp(level * d2[k, l])
 *       A (per k):  ratioL[k] = remainL[k] / (1e-9 + sum_l E[k, l] * remainR[l])
 *       B (per l):  s = remainR[l] * sum_k E[k, l] * ratioL[k]
 *                   ratioR[l] = min(remainR[l] / (s + 1e-9), 1) * remainR[l]
 *                   remainR[l] = max(0, remainR[l] - s)
 *       C (per k):  w[k, l] = E[k, l] * ratioL[k] * ratioR[l]
 *                   cost += sum_l w[k, l] * sqrt(d2[k, l]);   remainL[k] = max(0, remainL[k] - sum_l w[k, l])
 *   EMD(X, Y) = cost / n
 * It is NOT symmetric: EMD(X, Y) != EMD(Y, X) in general (x, the first cloud, carries remainL). It is
 * translation-invariant but not scale-invariant (the levels are absolute squared distances), so normalise the points
 * the way the compared work does. All mass is moved, so it is >= the exact-assignment EMD. One workgroup writes each
 * entry and every sum runs in a fixed order: an entry does not depend on how the caller splits the pair grid.
 * NOVA_ERR_ARG for null pointers (A, B > 0), ldc < B, N < 1 or N > NOVA_EMD_MAX_POINTS. Coordinates must be finite. */
#define NOVA_EMD_MAX_POINTS 4096
int nova_pointset_emd_matrix(const float* x, const float* y, float* emd, int A, int B, int N, int ldc, void* stream);

/* Occupancy grid of a set of clouds x [S, N, 3] (float32) for the JSD metric of the point-cloud generation literature
 * (PointFlow's jsd_between_point_cloud_sets / entropy_of_occupancy_grid; restated from the published algorithm, parity
 * unpinned by execution). For a resolution R the lattice nodes are
 *   c(i, j, k) = (i, j, k) / (R - 1) - 0.5,  i, j, k in 0 .. R-1,  flat index (i R + j) R + k.
 * With in_sphere != 0 the grid is the subset of nodes with |c| <= 0.5, decided in integers:
 *   (2i - (R-1))^2 + (2j - (R-1))^2 + (2k - (R-1))^2 <= (R-1)^2
 * (10144 nodes at R = 28). PointFlow decides it with a float32 norm: for even R no node lies on the sphere and the two
 * rules give the same grid; for odd R they may differ on boundary nodes (8 nodes at R = 27 and 29), and the integer
 * rule is the definition here. With in_sphere == 0 the grid is the whole lattice. Each point is assigned to its nearest
 * grid node (Euclidean; a point outside the ball or cube still goes to the nearest node of the grid), and
 *   counters[node]  += number of points, over all S clouds, assigned to the node
 *   bernoulli[node] += number of clouds with at least one point assigned to the node
 * Both are int64 [R^3] (zero stays zero off the grid) and are ADDED TO: the caller zeroes them, and may split a set over
 * several calls. bernoulli may be NULL. node (optional, NULL: not written) is int32 [S, N], each point's flat node index.
 * outside (optional, NULL: not written) is one int64 counter, added to: the points whose rounded node (below) is not a
 * grid node, i.e. that lie outside the grid's cells.
 * Float32 expressions the results rest on:
 *   node coordinate per axis   c_i = (float)(2 i - (R-1)) / (float)(2 (R-1))          one IEEE division, error <= 3e-8
 *   rounded node per axis      clamp(rintf((p + 0.5f) * (float)(R-1)), 0, R-1)         one add, one multiply, both rounded
 * When the rounded node is a grid node it is the point's node. Otherwise the node is the minimum over candidate grid
 * nodes (one per lattice column (i, j): k = the rounded k clamped into the column's grid nodes; the columns within the
 * distance to a known grid node; csrc/occupancy.hip proves that the nearest node is among them) of the float32 squared
 * distance fma(e2, e2, fma(e1, e1, e0 * e0)), e = p - c. Ties (not defined by the reference): the lowest flat index
 * among the candidates at the minimum of that float32 distance.
 * All results are integers: exact, and the same for every split over calls, grid size and run. workgroups: 0 = automatic,
 * > 0 = split the S clouds over (at least) that many workgroups (a workgroup holds at most 255 clouds and 2^24 - 1 points).
 * NOVA_ERR_SHAPE for N <= 0 or N >= 2^24; NOVA_ERR_ARG for R outside 2 .. NOVA_OCC_MAX_RES, R == 2 with in_sphere (no node
 * inside the ball), workgroups < 0, and null x or counters (S > 0). S <= 0 is a no-op. Coordinates must be finite. */
#define NOVA_OCC_MAX_RES 32
int nova_pointset_occupancy_grid(const float* x, long long* counters, long long* bernoulli, int* node, long long* outside, int S,
                                 int N, int R, int in_sphere, int workgroups, void* stream);

/* Farthest point sampling (Eldar et al.; PointNet++) of a set of clouds x [S, N, 3] (float32, finite): n of the N points
 * of every cloud, to bring sets of different density to the common point count the set-level metrics need (the EMD above
 * takes equal counts of at most NOVA_EMD_MAX_POINTS). The operation comes from the reference's farthest_point_sampling,
 * diffnext/models/transformers/transformer_pointcloud_nova.py:100-125, called from adaptive_sampling at :92-97.
 * DEVIATION, on purpose: that function body takes torch.min(dist_matrix, dim=1) over a matrix that contains the zero
 * diagonal, so its min_distances are all zero at every step, its argmax is index 0 every time and it returns
 * [start, 0, 0, ...]. What is built here is the standard algorithm, not parity with that body.
 * For one cloud x [N, 3], a start index s0 in 0 .. N-1 and 1 <= n <= N:
 *   idx[0] = s0,  dist[0] = +inf,  mind[j] = +inf
 *   for i = 1 .. n-1:
 *       q = x[idx[i-1]]
 *       mind[j] = fminf(mind[j], d(x[j], q))          for every j
 *       idx[i]  = the j with the largest mind[j], lowest j on ties
 *       dist[i] = mind[idx[i]]
 * d is the exact-difference float32 squared distance of the Chamfer and occupancy kernels: with e = p - q per axis,
 * d = fmaf(e2, e2, fmaf(e1, e1, e0 * e0)), every operation rounded once (no |p|^2 + |q|^2 - 2 p.q expansion, so the result
 * is as good for a cloud far from the origin as for a centred one). Consequences:
 *   - a chosen point has mind = 0 afterwards and is chosen again only when every point has mind = 0, i.e. when n exceeds
 *     the number of distinct points; the rule then yields the lowest such index (N equal points: [s0, 0, 0, ...]);
 *   - dist[1:] is non-increasing, exactly: mind only decreases and each dist[i] is its maximum;
 *   - the result depends on the cloud and s0 only: bitwise the same for every batch, launch split and workgroup shape.
 * idx is int32 [S, n]; dist is float32 [S, n] and may be NULL; start is int32 [S] on the device, NULL meaning 0 for every
 * cloud. A start value outside 0 .. N-1 is never dereferenced: the kernel clamps it into the range (callers should reject
 * it; the Python binding does). NOVA_ERR_SHAPE for N < 1 or N > NOVA_FPS_MAX_POINTS (one workgroup keeps a cloud in
 * registers, 16 points x 1024 threads; a larger cloud is an error, not a slow path); NOVA_ERR_ARG for n < 1, n > N, or null
 * x / idx with S > 0. S <= 0 returns 0. */
#define NOVA_FPS_MAX_POINTS 16384
int nova_pointset_farthest_point_sample(const float* x, const int* start, int* idx, float* dist, int S, int N, int n, void* stream);

/* Exact k nearest neighbours: for every point of the query clouds x [S, N, 3] the k nearest points of the target clouds
 * y [S, M, 3] (float32, finite), cloud by cloud, without ever storing an [N, M] distance matrix. The reference needs it for
 * compute_local_density, diffnext/models/transformers/transformer_pointcloud_nova.py:81-89 (torch.cdist(points, points),
 * topk(k_neighbors + 1, largest=False), drop column 0, mean), which feeds adaptive_sampling at :92-97, and builds the same
 * cdist + topk(k = 8) structure again at :144-146 and :179-182.
 * For query i of cloud s the candidates are all j in 0 .. M-1. The key of candidate j is the pair (d2(i, j), j) with
 *   d2 = fmaf(e2, e2, fmaf(e1, e1, e0 * e0)),  e = x[s, i] - y[s, j] per axis in float32,
 * every operation rounded once: the expression of nova_pointset_nn_dist and the sampling kernel, not cdist's
 * |x|^2 + |y|^2 - 2 x.y expansion, which cancels for the near neighbours this is about. The result is the k smallest keys
 * in lexicographic order, ascending: idx[s, i, :] (int32) their indices j and d2[s, i, :] (float32) their squared
 * distances. Ties in distance go to the lowest index, both inside the list and at its cut-off. No clamp, no
 * normalisation, no square root.
 * exclude_self != 0 is the self-query form: candidate j == i is skipped BY INDEX, not by distance; N == M is required and
 * y may be the same pointer as x.
 * DEVIATION, on purpose: the reference takes k + 1 neighbours from cdist and drops column 0, assuming it is the point
 * itself. Here the point is excluded by index. The remaining distances are the same multiset; where a cloud holds
 * duplicates of a point, the duplicate correctly appears at distance 0 (and the point itself never does), whereas the
 * reference's column 0 may be either of the two.
 * Consequences:
 *   - the result depends on (x[s], y[s], k, exclude_self) alone: bitwise the same for every batch, launch split and
 *     workgroup shape (the k smallest of a set of unique keys is one list, whatever the order they are met in);
 *   - rows of d2 are non-decreasing; rows of idx hold distinct values in 0 .. M-1.
 * Limits: 1 <= k <= min(NOVA_KNN_MAX_K, M - (exclude_self ? 1 : 0)), the best keys of a query living in registers;
 * 1 <= N, M <= NOVA_KNN_MAX_POINTS, so that one cloud is at most 2^32 candidate evaluations and always fits a launch.
 * NOVA_ERR_SHAPE for N or M outside 1 .. NOVA_KNN_MAX_POINTS and for exclude_self with N != M; NOVA_ERR_ARG for k outside
 * its range and for null x, y or idx with S > 0. d2 may be NULL (indices only). S <= 0 returns 0 after the shape and k
 * checks. Everything is checked before any device work. */
#define NOVA_KNN_MAX_K 32
#define NOVA_KNN_MAX_POINTS 65536
int nova_pointset_knn(const float* x, const float* y, int* idx, float* d2, int S, int N, int M, int k, int exclude_self, void* stream);

/* kNN neighbourhood feature aggregation, forward and backward: for every query row of idx [S, N, k] (int32, as
 * nova_pointset_knn writes it) the mean, or the weighted sum, of the k rows of the features f [S, M, C] (float32) it names,
 * cloud by cloud. It is the reference's EdgeAligner.extract_edge_features,
 * diffnext/models/transformers/transformer_pointcloud_nova.py:176-190 (torch.cdist(points, points), topk(min(8, N)), a
 * gather of the neighbours' features to [B, N, k, C], their mean over k, features - mean), called for every subset in
 * EdgeAligner.forward (:192-223) and from AutoregressiveDiffusion.forward (:286-290) on 768-wide features, where PyTorch
 * keeps the [B, N, N] matrix and the [B, N, k, C] tensor alive for the backward. Here the indices come from
 * nova_pointset_knn and neither pass stores anything of size N M or N k C. The subtraction from the centre feature is the
 * caller's (one torch op).
 * DEVIATION, on purpose: the gather expression at :184-187 does not run as written for [B, N, C] features (expand(-1, k, -1)
 * is applied to a 4-D tensor). The definition is that function's comment: the mean of the k nearest neighbours' features.
 * Every operation below is rounded once to float32 and nothing is fused; w [S, N, k] (float32) is optional.
 * nova_pointset_neighbor_aggregate: for query i of cloud s and channel c, with j_t = idx[s, i, t] and
 *     term_t = f[s, j_t, c]                  (w == NULL, the mean form)
 *     term_t = w[s, i, t] * f[s, j_t, c]     (weighted form: one rounded product)
 *     term_t = +0.0f                         for j_t outside 0 .. M-1, in both forms: such an index is never dereferenced
 *   acc = term_0, then acc = acc + term_t for t = 1 .. k-1 in that order (k - 1 rounded additions, none for k = 1);
 *   out[s, i, c] = acc / (float)k (one correctly rounded division; an out-of-range index still counts in the divisor) in
 *   the mean form, out[s, i, c] = acc in the weighted form. Duplicate indices inside a row are allowed.
 * nova_pointset_neighbor_inverse: the inverse neighbour list that makes the feature gradient a gather. An edge is a pair
 *   (i, t) with the id e = i k + t; it is in range when 0 <= idx[s, i, t] < M. offsets [S, M + 1] (int32):
 *   offsets[s, j] = the number of in-range edges naming a target below j, so offsets[s, 0] = 0 and offsets[s, M] = their
 *   total. edges [S, N k] (int32): edges[s, offsets[s, j] .. offsets[s, j + 1] - 1] = the ids of the edges naming j, in
 *   increasing order: the stable sort of the in-range edges by target. Slots past offsets[s, M] are not written. Built by
 *   two scans (one thread per target and quarter of the edge range walks the indices of its cloud and counts; a per-cloud
 *   prefix sum; the same walk again writing ids in the order met, each quarter starting behind the recounted matches of the
 *   quarters before it): 3 M N k integer compares per cloud, integers only, no atomics, no sort.
 * nova_pointset_neighbor_aggregate_bwd: from g [S, N, C] = dLoss/dout, gf [S, M, C] and gw [S, N, k] (float32).
 *   gf[s, j, c]: with e_0 < e_1 < ... the edges of j's segment of the list, i_r = e_r / k (integer division) and
 *       term_r = w[s, e_r] * g[s, i_r, c]     (weighted form, w flat over (i, t): one rounded product)
 *       term_r = g[s, i_r, c] / (float)k      (mean form: the forward's division, correctly rounded, not a product with 1/k)
 *     acc = term_0, then acc = acc + term_r in increasing r: accumulated from the first edge's term, not from 0 plus that
 *     term. A target no edge names gets exactly +0.0f, written by the kernel. One wave per target walks the segment: a
 *     gather, no atomics, one order. An edge id outside 0 .. N k - 1 in a list that is not this idx's inverse is never
 *     dereferenced (its term is +0.0f) and a segment is cut to 0 .. N k; gf is then the gradient under that list.
 *   gw[s, i, t] = sum_c g[s, i, c] * f[s, j_t, c], and +0.0f for j_t outside 0 .. M-1, in one reduction shape for every C
 *     and every launch: lane l of 64 forms p_l = +0.0f for l >= C, else the rounded product at c = l, then
 *     p_l = p_l + (the rounded product at c) for c = l + 64, l + 128, ... < C in that order; the 64 p_l are then summed by
 *     six pairwise steps in which both partners take a + b: lanes i <-> 7 - i inside each group of 8, then xor 1, xor 2,
 *     i <-> 15 - i inside each row of 16, rows 0|1 and 2|3 of 16 lanes, the two halves of 32.
 *   gf == NULL or gw == NULL means "not wanted" and its kernel is not launched; offsets and edges are read only for gf.
 * Consequences: out, offsets, edges, gf and gw of a cloud depend on that cloud's inputs, k and C alone: bitwise the same for
 * every batch, launch split, position in the batch and run; a channel of out or gf does not depend on the other channels.
 * Limits: 1 <= k <= NOVA_KNN_MAX_K (a row's indices live one per lane); 1 <= N, M <= NOVA_KNN_MAX_POINTS (edge ids and
 * offsets stay below 2^21); 1 <= C <= NOVA_NEIGHBOR_MAX_CHANNELS; at most 65535 clouds per call.
 * Errors, in this order, before any device work, the same in all three entries (the inverse has no C):
 *   NOVA_ERR_SHAPE for N or M outside their range; NOVA_ERR_SHAPE for C outside its range; NOVA_ERR_ARG for k outside its
 *   range; NOVA_ERR_SHAPE for S > 65535. S <= 0 returns 0 after these. Then NOVA_ERR_ARG for a null f, idx or out
 *   (aggregate), idx, offsets or edges (inverse), f, idx or g (bwd); bwd only: NOVA_ERR_ARG for gw given with w == NULL, for
 *   gf and gw both NULL, for gf given with a null offsets or edges; last, NOVA_ERR_ARG when an output overlaps an input or
 *   another output (outputs must not overlap inputs).
 * Added without a version bump (the number is pinned by the tests of three earlier entries; a library without the new
 * symbols fails to bind, loudly). */
#define NOVA_NEIGHBOR_MAX_CHANNELS 4096
int nova_pointset_neighbor_aggregate(const float* f, const int* idx, const float* w, float* out, int S, int N, int M, int k, int C,
                                     void* stream);
int nova_pointset_neighbor_inverse(const int* idx, int* offsets, int* edges, int S, int N, int M, int k, void* stream);
int nova_pointset_neighbor_aggregate_bwd(const float* f, const int* idx, const float* w, const float* g, const int* offsets,
                                         const int* edges, float* gf, float* gw, int S, int N, int M, int k, int C, void* stream);

/* Distance-weighted interpolation: for every query point of q [S, T, 3] the average of the values v [S, N, C] of ALL source
 * points p [S, N, 3] of its cloud (float32, finite), weighted by softmax(-distance / temperature), without ever storing a
 * [T, N] matrix. It is the reference's feature_aware_interpolation,
 * diffnext/models/transformers/transformer_pointcloud_nova.py:128-152 (torch.cdist(target, points), softmax(-dist), then
 * sum(weights.unsqueeze(-1) * points.unsqueeze(1)): an [S, T, N, 3] float tensor, summed away at once), the dense branch
 * of adaptive_sampling at :92-97, with the values made an argument and the temperature (1 there) a parameter.
 * NOT REPRODUCED: that body also takes topk(k = 8) of the distance matrix (:144-146) and never uses the result: dead code.
 * DEVIATION of the Python caller, on purpose: adaptive_sampling at :92-97 sends a subset with fewer points than target_size
 * to farthest_point_sampling with more samples than points, which that body cannot deliver; metrics.adaptive_sampling
 * returns the points in farthest-point order, repeated cyclically (every prefix stays well spread).
 * v == NULL means "the values are the source points" and needs C == 3. q may be the same pointer as p; out must not
 * overlap an input. For query i of cloud s, with sqdist3 the expression of nova_pointset_knn (three exact-difference
 * subtractions, one rounded product, two fused multiply-adds):
 *   d_j    = sqrtf(sqdist3(q[s, i], p[s, j]))            correctly rounded square root
 *   m      = min_j d_j
 *   w_j    = exp2f((m - d_j) * scale)                     scale = log2(e) / temperature in float32, made by the caller;
 *                                                        the difference and the product rounded once each, exp2f the
 *                                                        hardware's v_exp_f32 (1 ulp; results below 2^-126 become 0)
 *   out[s, i, c] = (sum_j w_j * v[s, j, c]) / (sum_j w_j)  one IEEE-rounded division, no reciprocal approximation
 * The point itself is not excluded (the reference's targets are a subset of its sources). scale == 0 (temperature = +inf)
 * is legal and gives the plain mean. The minimum is subtracted before exp2f, so queries far from every source are served
 * like near ones.
 * Order of summation (part of the definition: it fixes the bits). Always one workgroup of 256 threads per 64 queries, one
 * query per lane in all four waves; wave w sums the 64-source chunks w, w + 4, w + 8, ... of the cloud in ascending index
 * order, in the online form: its minimum m starts at the distance of its first source and its sums l, a[c] at 0; per
 * source, if d < m then l and a[c] are multiplied by exp2f((d - m) * scale) and m = d; then w = exp2f((m - d) * scale),
 * l = l + w, a[c] = fmaf(w, v[c], a[c]). The four partials are merged in wave order: M = the minimum of the m of the waves
 * that saw a source (wave w does when N > 64 w; the others contribute nothing), f_w = exp2f((M - m_w) * scale),
 * L = l_0 * f_0, A[c] = a_0[c] * f_0, then for w = 1 .. 3 L = fmaf(l_w, f_w, L), A[c] = fmaf(a_w[c], f_w, A[c]);
 * out = A[c] / L. No infinity enters this arithmetic, so scale == 0 meets neither inf * 0 nor inf - inf.
 * Consequences:
 *   - the result depends on (q[s], p[s], v[s], C, scale) alone: bitwise the same for every batch size, launch split and
 *     position in the batch, and a channel's result does not depend on the other channels;
 *   - v == NULL is bitwise equal to passing a copy of p as v with C = 3;
 *   - where every w_j is exactly 0 or 1 and the sums are exact in float32 (integer values, scale == 0 or a temperature far
 *     below the spacing of the distances) the result is the correctly rounded quotient of the exact sums.
 * Squared distances must be finite in float32 (coordinates below about 1e19 in magnitude).
 * NOVA_ERR_SHAPE for T or N outside 1 .. NOVA_INTERP_MAX_POINTS and for C outside 1 .. NOVA_INTERP_MAX_CHANNELS (the
 * numerators of a query live in registers); NOVA_ERR_ARG for v == NULL with C != 3, for scale negative, NaN or infinite,
 * and for null q, p or out with S > 0. S <= 0 returns 0 after those checks. Everything is checked before any device work. */
#define NOVA_INTERP_MAX_POINTS 65536
#define NOVA_INTERP_MAX_CHANNELS 8
int nova_pointset_kernel_interpolate(const float* q, const float* p, const float* v, float* out,
                                     int S, int T, int N, int C, float scale, void* stream);

/* The same forward with its statistics, and its backward: the gradient of the interpolation with respect to the queries,
 * the source points and the values, which the reference takes by autograd through feature_aware_interpolation
 * (transformer_pointcloud_nova.py:128-152; adaptive_sampling, :92-97, is called without no_grad inside
 * generate_pointcloud_autoregressive, :641-700, so with use_autoregressive the training gradient reaches the points through
 * softmax(-cdist) and the [S, T, N, 3] product, both kept alive for the backward). Neither pass stores anything of size T N.
 * nova_pointset_kernel_interpolate_stats: nova_pointset_kernel_interpolate, bit for bit (the same scan and merge), which
 *   also stores m[s, i] = M and l[s, i] = L of that definition (float32 [S, T]): M the smallest d_j of the row, L the merged
 *   weight sum (L >= 1: the nearest source has weight exactly 1).
 * nova_pointset_kernel_interpolate_bwd: from g [S, T, C] = dLoss/dout, the forward's inputs, its out and its m, l:
 *   gq [S, T, 3], gp [S, N, 3] and gv [S, N, C] (float32). The temperature gets no gradient. For query i and source j of one
 *   cloud, every operation rounded once to float32 and nothing fused that is not written as fmaf:
 *     e_k     = q_i[k] - p_j[k]                             per axis
 *     d       = sqrtf(sqdist3(q_i, p_j))                    the forward's distance, so M_i <= d holds exactly
 *     w       = exp2f((M_i - d) * scale)                    as the forward (v_exp_f32)
 *     r_i     = 1 / L_i                                     one IEEE division per query
 *     P       = w * r_i                                     1 / L is applied as a PRODUCT with the rounded quotient r_i
 *     delta_i = fmaf(g_i[C-1], out_i[C-1], ... fmaf(g_i[1], out_i[1], g_i[0] * out_i[0]))      ascending channel
 *     dot     = fmaf(g_i[C-1], v_j[C-1], ... fmaf(g_i[1], v_j[1], g_i[0] * v_j[0]))            ascending channel; the kernels
 *               run both chains over their rung of 3, 4 or 8 channels with zeros past C, which adds nothing (but turns a sum of -0 into +0)
 *     kappa   = scale * 0.693147180559945309f               (= 1 / temperature; scale == 0 gives exactly 0 gradient through d)
 *     f       = (kappa * (P * (dot - delta_i))) * rcp(d)    rcp the hardware's v_rcp_f32 (1 ulp); f = 0 where d == 0: the
 *               subgradient convention of nova_pointset_nearest_match_bwd, coincident points give no gradient and no NaN
 *               (the queries of feature_aware_interpolation ARE source points, so d == 0 occurs for every query)
 *   delta_i is formed in the prologue of each of the two kernels, by this one expression; there is no pass for it.
 *   gq[i, k]: the forward's workgroup shape (256 threads, 64 queries, one per lane in all four waves, wave w taking the
 *     64-source chunks w, w + 4, ... in ascending index): a_w[k] = fmaf(-f, e_k, a_w[k]) from +0, then
 *     gq[i, k] = ((a_0 + a_1) + a_2) + a_3 over the waves that saw a source (wave w does when N > 64 w).
 *   gp[j, k], gv[j, c]: one thread per source walks ALL queries of its cloud in increasing i: A[k] = fmaf(f, e_k, A[k]) and
 *     V[c] = fmaf(P, g_i[c], V[c]) from +0. gv[j, c] = V[c]; gp[j, k] = A[k], and with v == NULL (the values are the points)
 *     gp[j, k] = A[k] + V[k], one rounded addition. A gather: no atomics anywhere, one order of summation.
 * Consequences: gq, gp, gv of a cloud depend on (q[s], p[s], v[s], out[s], m[s], l[s], g[s], C, scale) alone: bitwise the same
 * for every batch, launch split, position in the batch and run; a channel's gv does not depend on the other channels or
 * the rung; v == NULL gives gp bitwise equal to gp + gv (one float32 addition) of a copy of p passed as v.
 * A NULL gq means "not wanted" and its kernel is not launched; likewise NULL gp and gv. gv must be NULL exactly when v is;
 * with v given, gp may be NULL alone, gv may not (one kernel forms both).
 * Errors, in this order, before any device work: those of nova_pointset_kernel_interpolate (out is an input here); then, with
 * S > 0, NOVA_ERR_ARG for a null m, l (both entries) or g, for gv non-null with v == NULL, for gv == NULL with v and gp
 * given, and for gq, gp and gv all NULL. S <= 0 returns 0 after the checks that do not look at pointers.
 * Added without a version bump (the number is pinned by the tests of three earlier entries; a library without the new symbols
 * fails to bind, loudly). */
int nova_pointset_kernel_interpolate_stats(const float* q, const float* p, const float* v, float* out, float* m, float* l,
                                           int S, int T, int N, int C, float scale, void* stream);
int nova_pointset_kernel_interpolate_bwd(const float* q, const float* p, const float* v, const float* out, const float* m,
                                         const float* l, const float* g, float* gq, float* gp, float* gv,
                                         int S, int T, int N, int C, float scale, void* stream);

/* Soft cluster pooling, forward and backward: for every cloud x [S, N, 3] (float32, finite) and K centres c, the K
 * softmax(-distance / temperature)-weighted centroids out [S, K, 3] and the cluster masses mass [S, K] (float32). It is the
 * soft clustering step both point-cloud models of the reference run on their gradient path,
 * PointCloudTransformer.forward, diffnext/models/transformers/transformer_pointcloud_nova.py:465-487, and
 * NOVAPointCloudTransformer.forward, :724-741 (torch.cdist(points, cluster_centers), softmax(-distances) over the centres,
 * a Python loop over the 8 clusters forming (points * w).sum(1) / (w.sum(1) + 1e-8)), where PyTorch keeps the [B, N, 8]
 * distances and weights and 8 [B, N, 3] products alive for the backward; the centres are a learnable parameter
 * (cluster_centers [8, 3]), with the temperature (1 there) made a parameter. Neither pass stores anything of size N K.
 * shared_centers != 0: c is [K, 3], the same for every cloud (the reference's parameter); otherwise c is [S, K, 3].
 * nova_pointset_soft_cluster: for point i and centre k of one cloud, every operation rounded once to float32 and nothing
 *   fused that is not written as fmaf, sqdist3 the expression of nova_pointset_knn:
 *     d_k   = sqrtf(sqdist3(x_i, c_k))                   correctly rounded square root
 *     m     = min_k d_k
 *     e_k   = exp2f((m - d_k) * scale)                   scale = log2(e) / temperature in float32, made by the caller; the
 *                                                        difference and the product rounded once each, exp2f the hardware's
 *                                                        v_exp_f32 (1 ulp; results below 2^-126 become 0), as in
 *                                                        nova_pointset_kernel_interpolate
 *     L     = e_0, then L = L + e_k for k = 1 .. K-1 in that order;  r = 1 / L   (one IEEE division; L >= 1)
 *     a_ik  = e_k * r
 *     mass_k   = sum_i a_ik                              each step acc = acc + a_ik
 *     num_k[j] = sum_i a_ik * x_i[j]                     each step acc = fmaf(a_ik, x_i[j], acc)
 *     out[s, k, j] = num_k[j] / (mass_k + 1e-8f)         one rounded addition, one IEEE division; 1e-8f is the reference's
 *                                                        constant (:480), part of the definition
 *   Order of the two sums over i (part of the definition: it fixes the bits; it depends on N and K alone). The cloud is cut
 *   into chunks of NOVA_SOFT_CLUSTER_CHUNK = 1024 consecutive points. Inside a chunk starting at point b, thread t of 256
 *   accumulates from +0 the points b + t, b + t + 256, b + t + 512, b + t + 768 in that order, skipping those past N - 1
 *   (a thread with no point keeps +0). The 256 accumulators are summed lane-wise inside each wave of 64 consecutive threads
 *   by six pairwise steps in which both partners take a + b: lanes i <-> 7 - i inside each group of 8, then xor 1, xor 2,
 *   i <-> 15 - i inside each row of 16, rows 0|1 and 2|3 of 16 lanes, the two halves of 32; then the four waves as
 *   ((w0 + w1) + w2) + w3. The chunk sums are added to +0 in ascending chunk order. No atomics.
 *   ws: a caller-provided workspace of S * ceil(N / NOVA_SOFT_CLUSTER_CHUNK) * K * 4 floats (the chunk partials); its
 *   contents after the call are unspecified.
 *   scale == 0 (temperature = +inf) is legal: every a_ik = 1 / K. A cluster all of whose a_ik underflow to 0 gives
 *   out = +0.0f and mass = 0. No infinity enters this arithmetic.
 * nova_pointset_soft_cluster_bwd: from g [S, K, 3] = dLoss/dout and gm [S, K] = dLoss/dmass (gm == NULL means zero), the
 *   forward's inputs, its out and its mass: gx [S, N, 3] and gc [S, K, 3] (float32; gc is PER CLOUD in both centre forms).
 *   The temperature gets no gradient. d_k, e_k, L, r, a_ik are recomputed as above, bit for bit. Then
 *     u_k   = 1 / (mass_k + 1e-8f)                       one rounded addition, one IEEE division per centre
 *     t_j   = x_i[j] - out_k[j]
 *     dot   = fmaf(g_k[2], t_2, fmaf(g_k[1], t_1, g_k[0] * t_0))
 *     h_k   = fmaf(u_k, dot, gm_k)
 *     hbar  = a_i0 * h_0, then hbar = fmaf(a_ik, h_k, hbar) for k = 1 .. K-1 in that order
 *     kappa = scale * 0.693147180559945309f              (= 1 / temperature; scale == 0 gives exactly 0 through d)
 *     f_ik  = (kappa * (a_ik * (hbar - h_k))) * rcp(d_k) rcp the hardware's v_rcp_f32 (1 ulp); f_ik = 0 where d_k == 0: the
 *                                                        subgradient convention of nova_pointset_nearest_match_bwd and of
 *                                                        torch.cdist's backward: a point on a centre gives no gradient
 *                                                        through that distance and no NaN
 *     e_j   = x_i[j] - c_k[j]
 *     gx[s, i, j]: R = +0, then for k = 0 .. K-1 in that order R = fmaf(f_ik, e_j, fmaf(a_ik * u_k, g_k[j], R)), the product
 *                  a_ik * u_k rounded once. Local to the point: one thread per point, no reduction.
 *     gc[s, k, j] = sum_i of -f_ik * e_j, each step acc = fmaf(-f_ik, e_j, acc), in the forward's order of summation.
 *   A NULL gx or gc means "not wanted" and the work that only serves it is skipped; they may not both be NULL.
 *   ws: S * ceil(N / NOVA_SOFT_CLUSTER_CHUNK) * K * 3 floats, read and written only when gc is given.
 *   An empty cluster (mass_k = 0) has u_k = 1e8 and every a_ik = 0: finite gradients.
 * nova_pointset_soft_cluster_sum_clouds: gcs[k, j] = the sum of gc[s, k, j] added to +0 in ascending s = 0 .. S-1, one
 *   thread per element: the gradient of shared centres, to be formed after every launch has written its part of gc, so it
 *   does not depend on the launch split. NOVA_ERR_SHAPE for K outside its range; S <= 0 returns 0 (gcs is not written);
 *   then NOVA_ERR_ARG for a null pointer and for gcs overlapping gc.
 * Consequences: out, mass, gx and gc of a cloud depend on that cloud's inputs, N, K and scale alone: bitwise the same for
 * every batch, launch split, position in the batch and run. The centres live in registers on rungs of 8, 16 and 32; a
 * result does not depend on the rung beyond the sign of a zero. Where every a_ik is exactly 0 or 1 / K with K a power of
 * two and the sums are exact in float32 (small integer coordinates; scale == 0, or a temperature far below the gaps of the
 * distances), out is the correctly rounded quotient of the exact sums.
 * Limits: 1 <= N <= NOVA_SOFT_CLUSTER_MAX_POINTS; 1 <= K <= NOVA_SOFT_CLUSTER_MAX_K; at most 65535 clouds per call.
 * Errors of the forward and the backward, in this order, before any device work: NOVA_ERR_SHAPE for N outside its range,
 * for K outside its range, for S > 65535; NOVA_ERR_ARG for scale negative, NaN or infinite. S <= 0 returns 0 after these.
 * Then NOVA_ERR_ARG for a null x, c, out, mass or ws (forward), a null x, c, out, mass or g (backward); backward only:
 * NOVA_ERR_ARG for gx and gc both NULL, then for gc given with a null ws; last, NOVA_ERR_ARG when an output (out, mass, ws;
 * gx, gc, ws) overlaps an input or another output.
 * Added without a version bump (the number is pinned by the tests of three earlier entries; a library without the new
 * symbols fails to bind, loudly). */
#define NOVA_SOFT_CLUSTER_MAX_POINTS 65536
#define NOVA_SOFT_CLUSTER_MAX_K 32
#define NOVA_SOFT_CLUSTER_CHUNK 1024
int nova_pointset_soft_cluster(const float* x, const float* c, float* out, float* mass, float* ws, int S, int N, int K,
                               int shared_centers, float scale, void* stream);
int nova_pointset_soft_cluster_bwd(const float* x, const float* c, const float* out, const float* mass, const float* g,
                                   const float* gm, float* gx, float* gc, float* ws, int S, int N, int K, int shared_centers,
                                   float scale, void* stream);
int nova_pointset_soft_cluster_sum_clouds(const float* gc, float* gcs, int S, int K, void* stream);

/* Depth-aware 3-D positional encoding, forward and backward: every coordinate of every point x [S, N, 3] (float32), times a
 * learnable scale, encoded into out [S, N, E] (float32) with sines and cosines over F = E / 6 (integer division)
 * frequencies, optionally added onto base [S, N, E]. It is the last custom operation of the reference's
 * PointCloudTransformer.forward in front of the soft clustering above: DepthAwarePositionalEncoding,
 * diffnext/models/transformers/transformer_pointcloud_nova.py:349-389, applied at :456-458 as x = x + depth_pe (a
 * zeros([B, N, E]), six strided slice assignments pe[:, :, k::6] each with its own [B, N, E / 6] division and sine or cosine,
 * a separate add; autograd keeps the six arguments). Neither pass stores anything of size N E here.
 * scale [3]: a DEVICE pointer to the three learnable scales (scale_x, scale_y, scale_z, :363-365), so the caller never
 * synchronises. div [F]: a device table of divisors, the caller's; the reference's is
 * (10000.0 ** (torch.arange(0, E, 2) / E))[:F] in float32 (:358-360), which encoding.py builds by those very torch ops. The
 * kernels are general over its values. base may be NULL.
 * nova_pointset_posenc: for row i of the S N rows, coordinate c in {0, 1, 2} and frequency f < F, every operation rounded
 *   once to float32 and nothing fused:
 *     s_c   = x[i, c] * scale[c]
 *     a_cf  = s_c / div[f]                      IEEE division, no reciprocal approximation
 *     pe[i, 6 f + 2 c]     = sinf(a_cf)         sinf, cosf: the device math library's accurate sincosf over the whole
 *     pe[i, 6 f + 2 c + 1] = cosf(a_cf)         float32 range; never the native __sinf / __cosf, no fast-math flag
 *     pe[i, ch] = +0 for 6 F <= ch < E          the tail channels
 *     out = pe, or base + pe                    one rounded addition per channel when base is given (tail: base + (+0))
 *   EXTENSION: the reference raises where tail channels exist (E % 6 != 0: pe[:, :, 0::6] then has one slot more than
 *   div_term[:E // 6]); here they are defined as +0. The reference also cannot run on a GPU tensor (div_term is a plain CPU
 *   attribute), and its torch.stack([scale_x, scale_y, scale_z], dim=0) is [3, 1], which broadcasts against [B, N, 3] along
 *   the point axis (:372: it raises unless N is 1 or 3); the scales here multiply per coordinate, the evident intent. With
 *   those three repaired the arithmetic above is what its CPU float32 ops compute.
 *   Non-finite points are not checked (a training path); NaN comes out as in torch.
 * nova_pointset_posenc_bwd: from g [S, N, E] = dLoss/dout and the forward's x, scale and div: gx [S, N, 3] and the PER-CLOUD
 *   scale gradient gs [S, 3] (float32). Every s_c, a_cf, sine and cosine is recomputed as above, bit for bit. Then
 *     u_cf     = fmaf(-g[i, 6 f + 2 c + 1], sinf(a_cf), g[i, 6 f + 2 c] * cosf(a_cf))    the product rounded once
 *     term_cf  = u_cf / div[f]                   IEEE division
 *     t_ic     = sum_f term_cf                   order below
 *     gx[i, c] = scale[c] * t_ic
 *     gs[s, c] = sum over the rows i of cloud s of x[i, c] * t_ic, each step acc = fmaf(x[i, c], t_ic, acc); order below
 *   The tail channels of g are not read. The gradient of base is g itself: no kernel runs for it.
 *   Order of the sums (part of the definition: it fixes the bits; it depends on (N, E) alone, never on S, the launch split
 *   or the cloud's position):
 *     over f within a row: the 3 F (sin, cos) pairs of a row are numbered j = 3 f + c. Lane l of one wave of 64 adds to +0,
 *       per coordinate c, the terms of its pairs j = l, l + 64, l + 128, ... with j % 3 == c in ascending j. The 64 lane
 *       sums of a coordinate are added by six pairwise steps in which both partners take a + b: lanes i <-> 7 - i inside
 *       each group of 8, then xor 1, xor 2, i <-> 15 - i inside each row of 16, rows 0|1 and 2|3 of 16 lanes, the two halves
 *       of 32 (the pairing of nova_pointset_soft_cluster).
 *     over the rows of a chunk: the cloud is cut into chunks of NOVA_POSENC_CHUNK = 32 consecutive rows. Inside a chunk
 *       starting at row b, wave w of 4 accumulates from +0 the rows b + w, b + w + 4, ... , b + w + 28 in that order, skipping
 *       those past N - 1 (a wave with no row keeps +0); the four waves are added as ((w0 + w1) + w2) + w3.
 *     over the chunks of a cloud: the chunk sums are added to +0 in ascending chunk order, through the workspace.
 *   No atomics.
 *   A NULL gx or gs means "not wanted" and the work that only serves it is skipped; they may not both be NULL.
 *   ws: a caller-provided workspace of S * ceil(N / NOVA_POSENC_CHUNK) * 3 floats, read and written only when gs is given;
 *   its contents after the call are unspecified.
 *   The gradient of the scales [3] is the sum of gs over the clouds in ascending cloud order, formed ONCE after every launch
 *   has written its clouds: nova_pointset_soft_cluster_sum_clouds(gs, out3, S, K = 1, stream) has exactly that contract
 *   (gcs[0, j] = the sum of gc[s, 0, j] added to +0 in ascending s) and is what encoding.py calls; there is no second kernel.
 * Consequences: out, gx and gs of a cloud depend on (x[s], scale, div, base[s] or g[s], N, E) alone: bitwise the same for
 * every batch, launch split, position in the batch and run. out with base is bitwise the float32 sum base + out-without-base.
 * x == 0 gives exactly +0 in the sine channels and 1 in the cosine channels (a negative scale makes the argument 0 * scale = -0
 * and its sine -0, as IEEE and torch have it).
 * Limits: 6 <= E <= NOVA_POSENC_MAX_DIM; 1 <= N <= NOVA_POSENC_MAX_POINTS; clouds in grid.y, at most 65535 per call; element
 * offsets are 64-bit throughout (S N E passes 2^31).
 * Errors of both entries, in this order, before any device work: NOVA_ERR_SHAPE for E outside its range, for N outside its
 * range, for S > 65535. S <= 0 returns 0 after these, before any pointer is looked at. Then NOVA_ERR_ARG for a null x,
 * scale, div or out (forward), a null x, scale, div or g (backward); backward only: NOVA_ERR_ARG for gx and gs both NULL,
 * then for gs given with a null ws; last, NOVA_ERR_ARG when an output (out; gx, gs, ws) overlaps an input (x, scale, div,
 * base; x, scale, div, g) or another output.
 * Added without a version bump (the number is pinned by the tests of three earlier entries; a library without the new
 * symbols fails to bind, loudly). */
#define NOVA_POSENC_MAX_DIM 4096
#define NOVA_POSENC_MAX_POINTS 65536
#define NOVA_POSENC_CHUNK 32
int nova_pointset_posenc(const float* x, const float* scale, const float* div, const float* base, float* out, int S, int N,
                         int E, void* stream);
int nova_pointset_posenc_bwd(const float* x, const float* scale, const float* div, const float* g, float* gx, float* gs,
                             float* ws, int S, int N, int E, void* stream);

/* Fused point embedding, forward and backward: the lift of the per-point inputs x [S, N, C] (float32) to the model width
 * through W [E, C] (the layout of nn.Linear.weight) and the broadcast additions that follow it, out [S, N, E] (float32)
 * written once. It is the step in front of every other point-set operation of the reference's two point-cloud forwards,
 * diffnext/models/transformers/transformer_pointcloud_nova.py: point_embed = nn.Linear(point_cloud_dim, 768) followed by
 * x = x + self.pos_embed[:, :x.shape[1], :] (:562-565, :712-716); the per-cloud rows broadcast over the points,
 * x + expanded_cluster_features (:753-756), x + timestep_emb.unsqueeze(1) (:759-760), x + text_emb (:772), and the same two in
 * AutoregressiveDiffusion.forward (:294, :297); EdgeAligner's spatial_embed = nn.Linear(3, embed_dim) (:174) added onto a
 * per-point base, final_features = aligned_features + spatial_features (:218-221); PointCloudPatchEmbed / PointCloudPosEmbed at
 * patch size 1 (:315-327, :340-346). In torch that is a K = C GEMM that writes [S, N, E] and one full read-and-write pass per
 * addend, and in the backward one read of the incoming gradient per consumer. Neither pass stores anything of size N E here.
 * bias [E], pos [N, E] (shared by all clouds), cond [S, E] (one row per cloud) and base [S, N, E] may each be NULL.
 * nova_pointset_embed: for row i of cloud s and channel e, every operation rounded once to float32:
 *     v = x[s, i, 0] * W[e, 0]
 *     v = fmaf(x[s, i, k], W[e, k], v)          for k = 1 .. C-1 in that order
 *     v = v + bias[e]                           each of the four additions only when its pointer is given, in this order
 *     v = v + pos[i, e]
 *     v = v + cond[s, e]
 *     v = v + base[s, i, e]
 *     out[s, i, e] = v
 *   An addend that is not given is no addition (not an addition of 0: -0 stays -0). So out with base is bitwise the float32
 *   sum of out-without-base and base, and likewise for cond, pos and bias, each onto the result without it and the later ones.
 *   Non-finite inputs are not checked (a training path); NaN comes out as in torch.
 * nova_pointset_embed_bwd: from g [S, N, E] = dLoss/dout and the forward's x and W, in one pass over g, whichever is wanted of
 *     gx [S, N, C]   gx[s, i, c]  = sum_e g[s, i, e] W[e, c]
 *     gWs [S, E, C]  gWs[s, e, c] = sum over the rows i of cloud s of g[s, i, e] x[s, i, c]     PER CLOUD
 *     gcs [S, E]     gcs[s, e]    = sum over the rows i of cloud s of g[s, i, e]                PER CLOUD
 *   gcs is the gradient of cond; summed over the clouds it is the gradient of bias, and gWs summed over the clouds the
 *   gradient of W (nova_pointset_embed_sum_clouds). The gradient of base is g itself: no kernel runs for it. The gradient of
 *   pos is nova_pointset_embed_pos_bwd.
 *   Order of the sums (part of the definition: it fixes the bits; it depends on (N, C, E) alone, never on S, the launch split
 *   or the cloud's position):
 *     over e within a row (gx): the channels are cut into blocks of 256; lane l of one wave of 64 holds the channels
 *       256 b + 4 l + j, j = 0 .. 3, of block b. Per block the lane adds to +0 its terms acc = fmaf(g[e], W[e, c], acc) in
 *       ascending j, skipping channels past E - 1 (a lane with no channel keeps +0). The 64 lane sums are added by six
 *       pairwise steps in which both partners take a + b: lanes i <-> 7 - i inside each group of 8, then xor 1, xor 2,
 *       i <-> 15 - i inside each row of 16, rows 0|1 and 2|3 of 16 lanes, the two halves of 32 (the pairing of
 *       nova_pointset_soft_cluster). The block sums are added to +0 in ascending block order.
 *     over the rows of a chunk (gWs, gcs): the cloud is cut into chunks of NOVA_EMBED_CHUNK = 128 consecutive rows. Inside a
 *       chunk starting at row b, wave w of 4 accumulates from +0 the rows b + w, b + w + 4, ... , b + w + 124 in that order,
 *       skipping those past N - 1 (a wave with no row keeps +0), each step acc = fmaf(g[i, e], x[i, c], acc) for gWs and
 *       acc = acc + g[i, e] for gcs; the four waves are added as ((w0 + w1) + w2) + w3.
 *     over the chunks of a cloud: the chunk sums are added to +0 in ascending chunk order, through the workspace.
 *   No atomics.
 *   A NULL gx, gWs or gcs means "not wanted" and the work that only serves it is skipped; they may not all be NULL.
 *   ws: a caller-provided workspace of S * ceil(N / NOVA_EMBED_CHUNK) * E * (C + 1) floats, read and written only when gWs or
 *   gcs is given; its contents after the call are unspecified.
 * nova_pointset_embed_sum_clouds: out[j] = the sum of per_cloud[s, j] added to +0 in ascending s = 0 .. S-1, one thread per
 *   element j < n: the gradient of W (per_cloud = gWs, n = E C) and of bias (per_cloud = gcs, n = E), to be formed ONCE after
 *   every launch has written its clouds, so it does not depend on the launch split. nova_pointset_soft_cluster_sum_clouds
 *   has the same contract but ends at 3 * 32 elements. NOVA_ERR_SHAPE for n outside 1 .. NOVA_EMBED_MAX_DIM *
 *   NOVA_EMBED_MAX_IN; S <= 0 returns 0 (out is not written); then NOVA_ERR_ARG for a null per_cloud or out and for out
 *   overlapping per_cloud.
 * nova_pointset_embed_pos_bwd: gpos[i, e] = (accumulate ? gpos[i, e] : +0) + g[0, i, e] + g[1, i, e] + ... + g[S-1, i, e], added
 *   left to right, one thread per 16 bytes (per element where N E % 4 != 0 or a pointer is off 16 bytes: the same bits).
 *   Called once per launch of clouds in ascending order, accumulate == 0 on the first call only, the result is one
 *   left-to-right sum over all clouds whatever the split. It is a second read of g, made only when pos needs a gradient
 *   (torch's g.sum(0) is the same read). NOVA_ERR_SHAPE for E, N, S > 65535 as below; S <= 0 returns 0; then NOVA_ERR_ARG for
 *   a null g or gpos and for gpos overlapping g.
 * Consequences: out, gx, gWs and gcs of a cloud depend on (x[s], W, bias, pos, cond[s], base[s] or g[s], N, C, E) alone:
 * bitwise the same for every batch, launch split, position in the batch and run, and for every alignment of the pointers
 * (rows that start on 16 bytes move 16 bytes per lane, on 8 bytes 8, otherwise 4; a lane keeps its channels). Where every
 * product and sum is exact in float32 (small integers) all results are the exact ones.
 * Limits: 1 <= C <= NOVA_EMBED_MAX_IN; 1 <= E <= NOVA_EMBED_MAX_DIM; 1 <= N <= NOVA_EMBED_MAX_POINTS; clouds in grid.y, at
 * most 65535 per call; element offsets are 64-bit throughout (S N E passes 2^31).
 * Errors of the forward and the backward, in this order, before any device work: NOVA_ERR_SHAPE for C outside its range, for
 * E outside its range, for N outside its range, for S > 65535. S <= 0 returns 0 after these, before any pointer is looked at.
 * Then NOVA_ERR_ARG for a null x, W or out (forward), a null x, W or g (backward); backward only: NOVA_ERR_ARG for gx, gWs and
 * gcs all NULL, then for gWs or gcs given with a null ws; last, NOVA_ERR_ARG when an output (out; gx, gWs, gcs, ws) overlaps
 * an input (x, W, bias, pos, cond, base; x, W, g) or another output.
 * Added without a version bump (the number is pinned by the tests of three earlier entries; a library without the new
 * symbols fails to bind, loudly). */
#define NOVA_EMBED_MAX_IN 8
#define NOVA_EMBED_MAX_DIM 4096
#define NOVA_EMBED_MAX_POINTS 65536
#define NOVA_EMBED_CHUNK 128
int nova_pointset_embed(const float* x, const float* W, const float* bias, const float* pos, const float* cond,
                        const float* base, float* out, int S, int N, int C, int E, void* stream);
int nova_pointset_embed_bwd(const float* x, const float* W, const float* g, float* gx, float* gWs, float* gcs, float* ws,
                            int S, int N, int C, int E, void* stream);
int nova_pointset_embed_sum_clouds(const float* per_cloud, float* out, int S, int n, void* stream);
int nova_pointset_embed_pos_bwd(const float* g, float* gpos, int S, int N, int E, int accumulate, void* stream);

/* Fused point head, forward and backward: the projection of the transformer's rows x [S, N, E] to the per-point outputs
 * through W [C, E] (the layout of nn.Linear.weight) and bias [C] (may be NULL), out [S, N, C] (float32). It is the last layer
 * of both point-cloud models of the reference, diffnext/models/transformers/transformer_pointcloud_nova.py:
 * self.output_proj = nn.Linear(embed_dim, 3) (:444, :611) applied as x = self.output_proj(x); x.view(B, -1, 3) (:512-515,
 * :778-781); train_newloss.py wraps it in GradientGuard(max_grad_norm=15.0) (:34-43, :681-684, :782), a torch.clamp of the
 * incoming gradient to +-15 in training mode, and PointCloudLoss consumes the result (:469). In torch that is a GEMM of
 * output width 3, three more degenerate GEMMs in the backward and one pass for the clamp; here the forward reads x once and
 * the backward reads x at most once and writes gx at most once. It is nova_pointset_embed with the roles swapped.
 * x is const void* with a nova_dtype code `dtype`: NOVA_F32, NOVA_BF16 or NOVA_F16. Every element is converted EXACTLY to
 * float32 on load; everything after that is float32, every operation rounded once. W, bias, out, g, gWs, gbs, ws are float32.
 * Lanes and blocks (part of the definition, the same for every dtype): the channels are cut into blocks of 512; lane l of one
 * wave of 64 holds the channels 512 b + 8 l + j, j = 0 .. 7, of block b.
 * nova_pointset_head: for row i of cloud s and output c:
 *     lane l:  a_l = +0;  a_l = fmaf(x[s, i, e], W[c, e], a_l)  over the lane's channels e <= E - 1 in ascending e (block after
 *              block, j ascending inside a block; a lane with no channel keeps +0)
 *     t = the 64 lane sums added by six pairwise steps in which both partners take a + b: lanes i <-> 7 - i inside each group
 *         of 8, then xor 1, xor 2, i <-> 15 - i inside each row of 16, rows 0|1 and 2|3 of 16 lanes, the two halves of 32 (the
 *         pairing of nova_pointset_embed_bwd's gx)
 *     out[s, i, c] = t + bias[c]                only when bias is given: an absent bias is no addition (not an addition of 0)
 *   The order is the lane's channels ascending, then the wave tree, then the bias once; it depends on E alone: never on the
 *   dtype, the alignment of x, the grid shape, the launch split or the cloud's position.
 * nova_pointset_head_bwd: from g [S, N, C] = dLoss/dout (float32), x and W, whichever is wanted of
 *     gx [S, N, E]   gx[s, i, e]  = sum_c g'[s, i, c] W[c, e]           in x's dtype
 *     gWs [S, C, E]  gWs[s, c, e] = sum over the rows i of cloud s of g'[s, i, c] x[s, i, e]     PER CLOUD, float32
 *     gbs [S, C]     gbs[s, c]    = sum over the rows i of cloud s of g'[s, i, c]                PER CLOUD, float32
 *   g' = g when clamp <= 0 (or NaN); with clamp > 0 every g is replaced on load by g < -clamp ? -clamp : g > clamp ? clamp : g,
 *   which is torch.clamp(g, -clamp, clamp): exact, no rounding, a NaN stays a NaN (the reference's GradientGuard).
 *   gWs and gbs summed over the clouds are the gradients of W and bias: nova_pointset_embed_sum_clouds with n = C E and n = C,
 *   called once after every launch has written its clouds (its contract, n up to NOVA_EMBED_MAX_DIM * NOVA_EMBED_MAX_IN, fits).
 *   gx: v = g'[c = 0] * W[0, e], then v = fmaf(g'[c], W[c, e], v) for c = 1 .. C-1 in that order (one multiplication and C - 1
 *     fused multiply-adds in float32), stored in x's dtype with ONE round-to-nearest-even (float32: as it is); f16 beyond
 *     65504 becomes an infinity, as torch's cast does.
 *   Order of the row sums (part of the definition; it depends on N alone, never on S, the launch split or the cloud's
 *   position): the cloud is cut into chunks of NOVA_HEAD_CHUNK = 128 consecutive rows. Inside a chunk starting at row b,
 *     wave w of 4 accumulates from +0 the rows b + w, b + w + 4, ... , b + w + 124 in that order, skipping those past N - 1 (a
 *     wave with no row keeps +0), each step acc = fmaf(g'[i, c], x[i, e], acc) for gWs and acc = acc + g'[i, c] for gbs; the
 *     four waves are added as ((w0 + w1) + w2) + w3. The chunk sums are added to +0 in ascending chunk order, through the
 *     workspace.
 *   No atomics.
 *   A NULL gx, gWs or gbs means "not wanted" and the work that only serves it is skipped (x is read only when gWs is given
 *   and may be NULL otherwise); they may not all be NULL.
 *   ws: a caller-provided workspace of S * ceil(N / NOVA_HEAD_CHUNK) * C * (E + 1) floats (per cloud and chunk the [C, E]
 *   partial of gWs, then the [C] partial of gbs), read and written only when gWs or gbs is given; its contents after the call
 *   are unspecified.
 * Consequences: out, gx, gWs and gbs of a cloud depend on (x[s], W, bias, g[s], clamp, N, C, E) alone: bitwise the same for
 * every batch, launch split, position in the batch and run, and for every alignment of the pointers (rows that start on 16
 * bytes move 16 bytes per access, else 8, 4 or, for the 16-bit types, 2; a lane keeps its channels). out of a bf16 or f16 x
 * is bitwise out of that x cast to float32, and its gx is bitwise that float32 gx rounded once. Where every product and sum
 * is exact in float32 (small integers) all results are the exact ones. Non-finite inputs are not checked (a training path).
 * Limits: 1 <= C <= NOVA_HEAD_MAX_OUT; 1 <= E <= NOVA_HEAD_MAX_DIM; 1 <= N <= NOVA_HEAD_MAX_POINTS; clouds in grid.y, at
 * most 65535 per call; element offsets are 64-bit throughout.
 * Errors of both, in this order, before any device work: NOVA_ERR_ARG for a null x, W or out (forward), a null x (when gWs is
 * given), W or g (backward); NOVA_ERR_ARG for an unknown dtype code; NOVA_ERR_SHAPE for C outside its range, for E outside its
 * range, for N outside its range, for S > 65535. S <= 0 returns 0 after these and writes nothing. Backward only: then
 * NOVA_ERR_ARG for gx, gWs and gbs all NULL, then for gWs or gbs given with a null ws. Last, NOVA_ERR_ARG when an output (out;
 * gx, gWs, gbs, ws) overlaps an input (x, W, bias; x, W, g) or another output.
 * Added without a version bump (the number is pinned by the tests of earlier entries; a library without the new symbols
 * fails to bind, loudly). */
#define NOVA_HEAD_MAX_OUT 8
#define NOVA_HEAD_MAX_DIM 4096
#define NOVA_HEAD_MAX_POINTS 65536
#define NOVA_HEAD_CHUNK 128
int nova_pointset_head(const void* x, int dtype, const float* W, const float* bias, float* out, int S, int N, int C, int E,
                       void* stream);
int nova_pointset_head_bwd(const void* x, int dtype, const float* W, const float* g, float clamp, void* gx, float* gWs,
                           float* gbs, float* ws, int S, int N, int C, int E, void* stream);

/* Fused bias-dropout-residual, forward and backward: the elementwise chains of the transformer body of the reference's
 * point-cloud models, diffnext/models/transformers/transformer_pointcloud_nova.py: nn.TransformerEncoderLayer(d_model, nhead,
 * dim_feedforward=4*d_model, dropout=0.1, batch_first=True, norm_first=True) with the default ReLU, stacked 8 or `depth`
 * times (:433-441, :590-598) and run at :510 and :775; dropout=0.1 is what train_newloss.py trains with (:652, :673). A
 * training step runs each layer as
 *     x = x + dropout1(out_proj(attn(norm1(x))))                      bias + dropout + residual on [B, N, E], twice per layer
 *     x = x + dropout2(linear2(dropout(relu(linear1(norm2(x))))))     bias + ReLU + dropout on [B, N, 4E], once per layer
 * In torch each chain reads and writes the activation three or four times and keeps a [rows, D] boolean mask drawn from the
 * device generator. Here every operand is read once and the output written once, and the mask is a pure function of
 * (seed, subsequence, element index): it is regenerated in the backward, never stored, and a CPU program can restate it.
 * x, residual, out, g, gx are [rows, D] in one nova_dtype (NOVA_F32, NOVA_BF16, NOVA_F16), rows contiguous; bias and
 * gbias_parts are float32.
 * The mask (part of the definition). The generator is Philox4x32-10: ten rounds of
 *     p0 = 0xD2511F53 * c0,  p1 = 0xCD9E8D57 * c2                      (32 x 32 -> 64 bits)
 *     (c0, c1, c2, c3) = (hi(p1) ^ c1 ^ k0,  lo(p1),  hi(p0) ^ c3 ^ k1,  lo(p0))
 *     (k0, k1) = (k0 + 0x9E3779B9, k1 + 0xBB67AE85)                    (mod 2^32; the key is bumped after every round)
 *   For the element with flat index i = (first_row + row) * D + col (64-bit, counted from the start of the LOGICAL tensor:
 *   first_row is the row index of x[0] in it, so a slice sees the mask of its place) the counter is
 *   (lo32(i >> 2), hi32(i >> 2), lo32(subsequence), hi32(subsequence)), the key (lo32(seed), hi32(seed)), and the draw w(i) is
 *   word i & 3 of the four output words (c0 .. c3 after the tenth round). The element is KEPT iff (uint64) w(i) >= T, where the
 *   caller passes T = floor(p * 2^32) in 0 .. 2^32 as a 64-bit value: p = 0 (T = 0) keeps everything, p = 1 (T = 2^32) keeps
 *   nothing, with no special case in the definition. When T == 0 no Philox is evaluated. scale is the caller's float32
 *   nearest to 1 / (1 - p) (1 for p = 0; unused for p = 1, pass 0).
 *   Known answers (counter; key; output), the first and third from Random123:
 *     00000000 x 4; 00000000 x 2;                                   6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     ffffffff x 4; ffffffff x 2;                                   408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0;       d16cfe09 94fdcceb 5001e420 24126ea1
 * nova_bias_dropout_add: per element, everything float32, every operation rounded once, nothing fused:
 *     t = float32(x[i])                                      exact
 *     t = t + bias[col]                                      only when bias is given: an absent bias is no addition
 *     act == NOVA_DROPOUT_ACT_RELU:  t = t > 0 ? t : (t != t ? t : +0)       (a NaN stays a NaN, -0 and negatives become +0)
 *     d = keep(i) ? t * scale : +0
 *     o = residual given ? float32(residual[i]) + d : d
 *     out[i] = o stored in the tensor's dtype with ONE round-to-nearest-even (float32: as it is)
 *   A dropped element is +0 whatever t is. Torch's x * mask * scale makes a dropped infinity or NaN a NaN; this kernel does
 *   not: only kept non-finite values propagate. No sums: there is no order to state in the forward.
 *   NOVA_DROPOUT_ACT_RELU together with a residual is an error: the reference has no such site, and the backward relies on it.
 * nova_bias_dropout_add_bwd: from g = dLoss/dout, whichever is wanted of gx (the tensor's dtype) and gbias_parts:
 *     act == NOVA_DROPOUT_ACT_NONE:  v = keep(i) ? float32(g[i]) * scale : +0     the mask is regenerated; `out` is not read and
 *                                                                              may be NULL; nothing of size rows x D was saved
 *     act == NOVA_DROPOUT_ACT_RELU:  v = float32(out[i]) > 0 ? float32(g[i]) * scale : +0     reads the forward's saved output
 *                                    and evaluates no Philox (torch's convention: threshold_backward gates on the result; a
 *                                    dropped element has out = +0, and so has a kept one that the ReLU zeroed)
 *     gx[i] = v stored with ONE round-to-nearest-even. A NULL gx means "not wanted".
 *   gbias_parts: float32 [ceil(rows / NOVA_DROPOUT_CHUNK), D], or NULL for "not wanted". Row c, column col is the sum, started
 *   from +0, of the float32 values v (BEFORE the store rounding) of the rows 128 c .. min(128 c + 127, rows - 1) at that
 *   column, added in ascending row order: acc = acc + v, one float32 addition per row. One thread owns a column group and walks
 *   the rows: no cross-lane reduction, no atomics. The gradient of the bias is the sum of the chunk rows added to +0 in
 *   ascending chunk order: nova_pointset_embed_sum_clouds(gbias_parts, gbias, chunks, D, stream), whose contract fits
 *   (n = D up to 32768, any number of rows). So that the chunks of a slice are the chunks of the logical tensor, first_row
 *   must be a multiple of NOVA_DROPOUT_CHUNK = 128 when gbias_parts is given.
 * Consequences: out, gx and gbias_parts depend on (the operands, T, scale, seed, subsequence, first_row, D) alone: bitwise the
 * same for every run, every split of the rows into calls at multiples of 128 and every alignment of the pointers. Kernel
 * shape (no part of the definition): 16 bytes per lane and access, 4 float32 or 8 16-bit elements, where D is a multiple of
 * that count and every pointer is on 16 bytes, one Philox evaluation serving 4 consecutive elements; otherwise element by
 * element, the same bits. Element offsets are 64-bit throughout. Non-finite inputs are not checked (a training path).
 * Limits: 1 <= D <= NOVA_DROPOUT_MAX_DIM; rows <= NOVA_DROPOUT_MAX_ROWS per call; first_row + rows <= 2^48.
 * Errors of both, in this order, before any device work: (1) NOVA_ERR_ARG for a null x or out (forward), a null g (backward);
 * (2) NOVA_ERR_ARG for an unknown dtype code; (3) NOVA_ERR_ARG for an unknown act code, then (forward) for
 * NOVA_DROPOUT_ACT_RELU with a residual; (4) backward: NOVA_ERR_ARG for NOVA_DROPOUT_ACT_RELU with a null out;
 * (5) NOVA_ERR_SHAPE for D outside its range, then for rows above NOVA_DROPOUT_MAX_ROWS; (6) NOVA_ERR_ARG for T > 2^32;
 * (7) NOVA_ERR_ARG for first_row < 0, then for first_row + rows > 2^48; (8) backward: NOVA_ERR_ARG for first_row not a
 * multiple of 128 when gbias_parts is given; (9) backward: NOVA_ERR_ARG for gx and gbias_parts both NULL. rows <= 0 returns 0
 * after these and writes nothing. Last, (10) NOVA_ERR_ARG when an output (out; gx, gbias_parts) overlaps an input (x, bias,
 * residual; g, and out with NOVA_DROPOUT_ACT_RELU) or another output.
 * Added without a version bump (the number is pinned by the tests of earlier entries; a library without the new symbols
 * fails to bind, loudly). */
#define NOVA_DROPOUT_MAX_DIM 16384
#define NOVA_DROPOUT_MAX_ROWS 1073741824
#define NOVA_DROPOUT_CHUNK 128
#define NOVA_DROPOUT_ACT_NONE 0
#define NOVA_DROPOUT_ACT_RELU 1
int nova_bias_dropout_add(const void* x, int dtype, const float* bias, const void* residual, void* out, long long rows, int D,
                          long long first_row, unsigned long long T, float scale, unsigned long long seed,
                          unsigned long long subsequence, int act, void* stream);
int nova_bias_dropout_add_bwd(const void* g, const void* out, int dtype, void* gx, float* gbias_parts, long long rows, int D,
                              long long first_row, unsigned long long T, float scale, unsigned long long seed,
                              unsigned long long subsequence, int act, void* stream);

/* Fused AdamW step with in-kernel gradient clipping over a LIST of tensors: what the reference's trainer does after the
 * backward, torch.nn.utils.clip_grad_norm_ and then torch.optim.AdamW with betas (0.9, 0.999) (train_newloss.py:827-841 and
 * :1060-1082). In torch that is a norm pass, a read-modify-write of every gradient and about a dozen elementwise passes over
 * every parameter. Here each gradient is read twice (once for the norm, once for the update) and never written, each
 * parameter and each moment is read and written once, and the host never waits for the device.
 * nova_adamw_tensor: one tensor of the list. param and grad are n contiguous elements of the nova_dtype `dtype` (NOVA_F32,
 *   NOVA_BF16, NOVA_F16); exp_avg and exp_avg_sq are float32 [n]; master is float32 [n], the full-precision copy of a 16-bit
 *   (or any) parameter, or NULL. The seven numbers are float32 values the HOST forms in float64 and rounds once each, from the
 *   group's lr, (beta1, beta2), eps, weight_decay and the tensor's step count t >= 1 (the caller's business):
 *     decay = 1 - lr * weight_decay     w1 = 1 - beta1     b2 = beta2     w2 = 1 - beta2
 *     q = sqrt(1 - beta2^t)             a = lr / (1 - beta1^t)            eps
 * nova_adamw_sumsq: the float32 sum of the squares of every gradient element of the list (only grad, n and dtype are read).
 *   Tensor i is cut into ceil(n_i / NOVA_ADAMW_CHUNK) chunks of NOVA_ADAMW_CHUNK = 8192 elements, the last one short; the
 *   chunks of the whole list, in list order and ascending inside a tensor, are numbered 0 .. P - 1 (a tensor with n = 0 has
 *   none). The partial of a chunk that starts at element c0:
 *     thread t = 0 .. 255 owns the units u = t, 256 + t, 512 + t, 768 + t of the chunk, unit u being the 8 elements
 *     c0 + 8 u .. c0 + 8 u + 7. From acc = +0, over its units in that order and the elements of a unit in ascending order:
 *     x = float32(grad[e]) (exact), acc = acc + x * x (the product rounded, then the sum). An element past n - 1 is not added.
 *     Then the tree over the 256 values s[t] = acc: for h = 128, 64, .. 1: s[t] = s[t] + s[t + h] for every t < h. The
 *     partial is s[0].
 *   workspace[k] = the partial of chunk k (plain stores: float32 [workspace_floats], workspace_floats >= P). The total:
 *     the partials as rows of NOVA_ADAMW_SUM_COLUMNS = 256: column n = 0 .. 255 is the sum, from +0 in ascending k, of
 *     workspace[256 k + n] over the k with 256 k + n < P (total = total + v every time); then the same tree over the 256
 *     columns. *sumsq = s[0], and *norm = sqrt(*sumsq), correctly rounded, when norm is not NULL (the total 2-norm of the
 *     gradients before clipping, for the caller's log, from the same launch). (The order of ordered_sum with per = 256, whose last step is the tree, in one launch and with
 *     no padding of the last row; one serial thread over about 10^5 partials would be a visible share of the call.)
 *   The total stays on the device. P == 0 (an empty list, or only tensors with n = 0) launches nothing and leaves *sumsq and
 *   *norm alone.
 * nova_adamw_step: the update of every element of every tensor, one pass. sumsq is the device float32 of nova_adamw_sumsq or
 *   NULL for "no clipping". Every operation is float32, rounded once, nothing fused; sqrt and / are the correctly rounded ones:
 *     s  = sumsq ? c > 1 ? 1 : c  with  c = max_norm / (sqrt(*sumsq) + 1e-6f)  : 1
 *                                          (torch's clip_grad_norm_ coefficient min(1, c), a NaN staying a NaN as torch.clamp
 *                                           keeps it; formed by every thread, the same in all)
 *     g  = float32(grad[e]) * s            (no multiplication when sumsq is NULL)
 *     p0 = master ? master[e] : float32(param[e])
 *     p1 = p0 * decay
 *     m' = m + w1 * (g - m)                m = exp_avg[e]
 *     v' = v * b2 + w2 * (g * g)           v = exp_avg_sq[e]
 *     d  = sqrt(v') / q + eps
 *     p' = p1 - a * (m' / d)
 *   exp_avg[e] = m', exp_avg_sq[e] = v', master[e] = p' when master is given, and param[e] = p' stored in the tensor's dtype
 *   with ONE round-to-nearest-even (float32: as it is). The gradient is not written. A non-finite *sumsq propagates as torch's
 *   default does (an infinite one gives s = 0 and NaN where the gradient is infinite, a NaN gives NaN everywhere); steps are
 *   not skipped. No amsgrad, no maximize, no capturable mode.
 * Consequences: every result depends on (the operands, the numbers) alone and *sumsq on the list alone: bitwise the same for
 * every run, every alignment of the pointers and every split of the list over launches. Kernel shape (no part of the
 * definition): one workgroup of 256 threads per (tensor, chunk); the list travels by value in the kernel's arguments,
 * NOVA_ADAMW_BLOCK = 32 tensors with n > 0 per launch, so there is no device-side table, no host-to-device copy and no
 * synchronisation, and no pointer is remembered between calls; 16-byte accesses where every pointer of the tensor is on 16
 * bytes and the unit lies inside the tensor, element by element otherwise. Non-finite inputs are not checked (a training path).
 * Errors of both, NOVA_ERR_ARG, in this order, before any device work: (1) count < 0; (2) a null `tensors` with count > 0;
 * then per tensor in list order: (3) n outside 0 .. NOVA_ADAMW_MAX_N = 2^31 - 1; (4) an unknown dtype code; (5) for n > 0 a null
 * param (step), grad, exp_avg (step), exp_avg_sq (step), in that order. Then, nova_adamw_sumsq with P > 0: (6) a null workspace,
 * workspace_floats < P, a null sumsq, sumsq or norm inside the workspace's first P floats, norm on sumsq; nova_adamw_step: (6) max_norm <= 0 or NaN
 * when sumsq is given. The texts are their own (no entry of the recorded error table).
 * Added without a version bump (the number is pinned by the tests of earlier entries; a library without the new symbols
 * fails to bind, loudly). */
#define NOVA_ADAMW_CHUNK 8192
#define NOVA_ADAMW_SUM_COLUMNS 256
#define NOVA_ADAMW_BLOCK 32
#define NOVA_ADAMW_MAX_N 2147483647
typedef struct nova_adamw_tensor {
  void* param;
  const void* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* master;
  long long n;
  int dtype;
  float decay, w1, b2, w2, q, a, eps;
} nova_adamw_tensor;
int nova_adamw_sumsq(const nova_adamw_tensor* tensors, int count, float* workspace, long long workspace_floats, float* sumsq,
                     float* norm, void* stream);
int nova_adamw_step(const nova_adamw_tensor* tensors, int count, const float* sumsq, float max_norm, void* stream);

/* Nearest match with indices, and its backward: the primitive under the Chamfer-type training losses of the reference,
 * robust_chamfer_distance on distChamfer (train_newloss.py:316-349) and the edge-consistency term (train_newloss.py:449-457:
 * torch.cdist(subset1, subset2).min(dim=1), mean), which in PyTorch keep a [B, N, M] cdist matrix alive for the backward.
 * Neither pass stores an [N, M] array here. x [B, N, 3], y [B, M, 3] float32, finite.
 * Point map p(v), the one of nova_pointset_nn_dist: c_k = min(max(v_k, clamp_lo), clamp_hi) per coordinate; unit_norm != 0:
 *   n = sqrtf((fmaf(c1, c1, c0 * c0)) + c2 * c2), inv = 1 / max(n, 1e-8) (one IEEE division), p_k = c_k * inv; otherwise p = c.
 * Every operation named is rounded once to float32; nothing else is fused.
 * nova_pointset_nearest_match: for every x[b, i] the smallest key (sqdist3(p(x_i), p(y_j)), j) in lexicographic order over
 *   j in 0 .. M-1, sqdist3 the expression of nova_pointset_knn; ties in distance go to the lowest j (the rule of
 *   nova_pointset_knn). d[b, i] = sqrtf(that d2) (float32, bit for bit the output of nova_pointset_nn_dist) and idx[b, i] = j
 *   (int32).
 * nova_pointset_nearest_match_bwd: from g[b, i] = dL/dd[b, i] and the forward's idx, gx [B, N, 3] and gy [B, M, 3] (float32).
 *   With a = idx[b, i], u = p(x_i) - p(y_a) per axis and dist = sqrtf(sqdist3(p(x_i), p(y_a))), all recomputed:
 *     t_i = (g_i * u) / dist per axis, the product rounded, then one IEEE division;  t_i = 0 exactly when dist == 0
 *   (the subgradient convention: coincident points give no NaN and no gradient). An idx outside 0 .. M-1 is never
 *   dereferenced and has t_i = 0. The pull-back P_v(t) through p at a point v, with c, n, inv, p as above:
 *     unit_norm, n >= 1e-8:  w_k = fmaf(-p_k, s, t_k) with s = fmaf(p2, t2, fmaf(p1, t1, p0 * t0));  r_k = w_k * inv
 *                            ((I - p p^T) t / n)
 *     unit_norm, n <  1e-8:  r_k = t_k * inv   (inv is 1e8: torch's gradient of c / clamp_min(|c|, 1e-8) below the floor)
 *     otherwise:             r = t
 *     then r_k = 0 for every coordinate with v_k outside [clamp_lo, clamp_hi], bounds inclusive (torch.clamp's backward).
 *   gx[b, i] = P_{x_i}(t_i).  gy[b, j] = P_{y_j}(-S_j), S_j = the sum of t_i over the i with idx[b, i] == j, added one by one
 *   IN INCREASING i starting from +0 (a y_j nobody matched gets P(-0)). gy is a gather, one thread per y_j walking all i:
 *   no atomics, no sort, one order of summation.
 * Consequences: d, idx, gx and gy of a cloud depend on (x[b], y[b], g[b], the clamp, unit_norm) alone: bitwise the same for
 * every batch, launch split, position in the batch and run.
 * No clamp: pass -inf and +inf. NOVA_ERR_SHAPE for M <= 0 (an empty target set) and for B > 65535; NOVA_ERR_ARG for a null
 * pointer and for clamp_lo > clamp_hi (or either NaN). B <= 0 or N <= 0 is a no-op returning 0, as in nova_pointset_nn_dist
 * (gy is then not written). Everything is checked before any device work. Added without a version bump. */
int nova_pointset_nearest_match(const float* x, const float* y, float* d, int* idx, int B, int N, int M, float clamp_lo,
                                float clamp_hi, int unit_norm, void* stream);
int nova_pointset_nearest_match_bwd(const float* x, const float* y, const int* idx, const float* g, float* gx, float* gy, int B,
                                    int N, int M, float clamp_lo, float clamp_hi, int unit_norm, void* stream);

/* Distance of matched pairs under a GIVEN permutation, and its backward: the primitive under the exact-assignment EMD
 * training loss. The reference's emd_approx (train_newloss.py:352-377) is the mean matched distance under the optimal
 * assignment of the clamped clouds, cost floored at 1e-8, and its EMD term (train_newloss.py:418-424) goes through numpy
 * and carries no gradient. The optimal permutation is piecewise constant in the points, so with the assignment held fixed
 * (nova_pointset_assignment, or scipy on the host) the loss is a sum of n distances between matched pairs, and the gradient
 * of that sum is the gradient of the EMD almost everywhere. Nothing of size n^2 exists in either pass.
 * Inputs.  x, y [B, n, 3] float32, finite. idx int32 [B, n]: the column matched to row i. inv int32 [B, n]: the row matched
 *   to column j, i.e. the inverse permutation (inv[b, idx[b, i]] = i); the backward takes it from the caller.
 * Clamp.  c(v) = fminf(fmaxf(v, clamp_lo), clamp_hi) per coordinate; pass -inf and +inf for no clamp.
 * nova_pointset_matched_dist: with a = idx[b, i] and e = c(x[b, i]) - c(y[b, a]) per axis (float32 subtractions),
 *     d2 = fmaf(e2, e2, fmaf(e1, e1, e0 * e0))          the product rounded once, the two fused multiply-adds once each
 *     d[b, i] = fmaxf(sqrtf(d2), floor)                 the square root correctly rounded
 *   Before the floor, sqrtf(d2) is bit for bit the entry D[b, i, a] of nova_pointset_pairwise_dist and the cost c(i, a) of
 *   nova_pointset_assignment under the same clamp. An idx outside 0 .. n-1 is never dereferenced and gives d[b, i] = NaN.
 * nova_pointset_matched_dist_bwd: from g[b, i] = dL/dd[b, i] (float32 [B, n]), gx and gy [B, n, 3] (float32). For the pair
 *   (i, a), with e as above and dist = sqrtf(d2) recomputed:
 *     t_k = (g_i * e_k) / dist per axis, the product rounded, then one IEEE division
 *     t = 0 exactly when dist == 0 or dist < floor (torch.clamp_min's backward: no gradient below the floor, gradient at it;
 *     and the subgradient convention of nova_pointset_nearest_match_bwd: coincident points give no gradient and no NaN)
 *   then r_k = 0 for every coordinate of the DIFFERENTIATED point that lies outside [clamp_lo, clamp_hi], bounds inclusive
 *   (torch.clamp's backward), r_k = t_k otherwise:
 *     gx[b, i] = r(t)    from the pair (i, idx[b, i]),  masked at x[b, i]
 *     gy[b, j] = r(-t)   from the pair (inv[b, j], j),  masked at y[b, j]; t is recomputed by the thread that owns j
 *   Both outputs are gathers, one thread per output row: no scatter writes and no atomics, and every output element is
 *   written exactly once, even for a corrupt index. An idx (for gx) or inv (for gy) outside 0 .. n-1 is never dereferenced
 *   and gives a zero row. gy does not consult idx: for an inv that is not the inverse of idx, gy is the gradient under inv.
 * Consequences: d, gx and gy of a cloud depend on (x[b], y[b], idx[b], inv[b], g[b], the clamp, floor) alone: bitwise the
 * same for every batch, launch split, position in the batch and run.
 * NOVA_ERR_ARG for a null pointer, for clamp_lo > clamp_hi (or either NaN) and for floor negative or NaN; NOVA_ERR_SHAPE for
 * B > 65535. B <= 0 or n <= 0 is a no-op returning 0 (after the clamp and floor checks, as in nova_pointset_nearest_match).
 * Everything is checked before any device work. Added without a version bump (a library without the new symbols fails to
 * bind, loudly). */
int nova_pointset_matched_dist(const float* x, const float* y, const int* idx, float* d, int B, int n, float clamp_lo,
                               float clamp_hi, float floor, void* stream);
int nova_pointset_matched_dist_bwd(const float* x, const float* y, const int* idx, const int* inv, const float* g, float* gx,
                                   float* gy, int B, int n, float clamp_lo, float clamp_hi, float floor, void* stream);

/* Optimal assignment between x [B, n, 3] and y [B, n, 3] (float32, finite), pair by pair: the permutation that minimises
 * the mean matched distance, i.e. the earth mover's distance that compute_emd_distance (test_optimize.py:385-415) and
 * emd_approx (train_newloss.py:352-372) take from scipy's linear_sum_assignment on a [n, n] cost matrix copied to the
 * host. Here it is solved on the GPU by a Jacobi auction (Bertsekas) with epsilon scaling in exact integer arithmetic,
 * one workgroup per pair, 1 <= n <= NOVA_ASSIGN_MAX_POINTS; no cost matrix is ever stored.
 * Cost.  c(i, j) = sqrtf(d2), d2 = fmaf(e2, e2, fmaf(e1, e1, e0 * e0)) with e = x[i] - y[j] per axis after the optional
 * clamp fminf(fmaxf(v, clamp_lo), clamp_hi) of every coordinate (use_clamp != 0): bit for bit the float32 entry
 * D[b, i, j] of nova_pointset_pairwise_dist.
 * Integer scheme (the contract; every tolerance of the tests follows from it):
 *   C(i, j)  = llrint(c(i, j) * 2^18) * (n + 1)                        64-bit integers; the product c * 2^18 is exact
 *   price[j] = 0 for every column j
 *   eps      = max(1, ((llrint(diag * 2^18) + 1) * (n + 1)) / 4), diag the float32 diagonal of the bounding box of
 *              both clamped clouds (>= every c, so no pass over the costs is needed)
 *   phase:   every row unassigned; rounds (below) until every row is assigned; then, if eps == 1, stop, else
 *            eps = max(1, eps / 8) and the next phase starts with every owner cleared and the prices kept
 *   round:   every unassigned row i finds, over all j, the smallest and second smallest a(j) = C(i, j) + price[j]
 *            (that is the best and second-best value -C - price); ties in a go to the lowest j; for n == 1 the second
 *            equals the first. Row i bids  price[j*] + (second - best) + eps  on its best column j*. Every column takes
 *            its highest bid, bid ties going to the lowest row, evicts its previous owner and sets its price to the bid.
 *            All bids of a round are computed from the prices at its start.
 * Costs are multiples of n + 1 and the last phase runs at eps == 1, so the final assignment is within n * eps < n + 1 of
 * the optimum of the integer costs, hence optimal for them: its mean quantised cost is the minimum, and its mean float32
 * cost exceeds the minimum mean of c by at most the quantum 2^-18 (half a quantum per term on either side).
 * Everything is deterministic: the result is a function of the pair, n and the clamp alone, bitwise the same for every
 * batch, every split into launches and every run (bids are resolved by a maximum over unique (bid, row) keys, which does
 * not depend on the order of arrival).
 * Range.  Keys carry 13 bits of row or column beside the value, so bids must stay below 2^49 and diag below 4096 (costs
 * < 2^43). A pair outside that range stops with the status NOVA_ASSIGN_RANGE; nothing wraps.
 * Launches.  One call runs at most `rounds` rounds per pair and then stores the pair's whole state (prices, owners, row
 * assignments, eps, the rounds used, a done flag) in `state`, nova_pointset_assignment_state_bytes(n) bytes per pair (16-byte
 * aligned; layout private to the library). restart != 0 ignores the state's content and starts the auction; restart == 0
 * continues from a state written by an earlier call with the same x, y, B, n and clamp; a finished pair's workgroup
 * exits at once. all_done (one int on the device) receives 1 when every pair is done, 0 when some pair needs more
 * rounds, NOVA_ASSIGN_RANGE (-1) when some pair left the range. The caller repeats the call until all_done != 0 and
 * bounds the total number of rounds itself.
 * Outputs.  cost[b] is -1 while pair b is unfinished and -2 when it left the range. Once it is done:
 *   col_of_row[b, i]  int32, the column matched to row i (a permutation of 0 .. n-1)
 *   cost[b]           the mean over i of the float32 c(i, col_of_row[i]), summed in a fixed order: each thread t of the T
 *                     threads its rows t, t + T, ... in turn (at most 4), the 64 lanes of a wave pairwise in 6 steps, the
 *                     T / 64 <= 16 waves in turn, one division by n
 * NOVA_ERR_ARG for a null pointer (x, y, col_of_row, cost, state with B > 0; all_done always), n outside
 * 1 .. NOVA_ASSIGN_MAX_POINTS, rounds < 1, or use_clamp with clamp_lo > clamp_hi. B <= 0 only sets all_done to 1.
 * nova_pointset_assignment_state_bytes returns 0 for n outside the range.
 * nova_pointset_assignment_rounds copies every pair's rounds-used counter from `state` to rounds_used (int32 [B]). */
#define NOVA_ASSIGN_MAX_POINTS 4096
#define NOVA_ASSIGN_RANGE (-1)
long long nova_pointset_assignment_state_bytes(int n);
int nova_pointset_assignment(const float* x, const float* y, int* col_of_row, float* cost, void* state, int B, int n, float clamp_lo,
                             float clamp_hi, int use_clamp, int rounds, int restart, int* all_done, void* stream);
int nova_pointset_assignment_rounds(const void* state, int* rounds_used, int B, int n, void* stream);

/* ---- composite entry points (what the AR loop actually calls) --------------------------------
 * One ViT block's parameters (reference state_dict names in comments). GEMM weights in `dtype`,
 * everything else f32. */
typedef struct {
  const void* qkv_w;    /* attn.qkv.weight [3D, D] */
  const float* qkv_b;   /* attn.qkv.bias   [3D]    */
  const void* proj_w;   /* attn.proj.weight [D, D] */
  const float* proj_b;
  const float* norm1_w; /* norm1.weight [D] */
  const float* norm1_b;
  const void* fc1_w;    /* mlp.fc1.weight [4D, D] */
  const float* fc1_b;
  const void* fc2_w;    /* mlp.fc2.weight [D, 4D] */
  const float* fc2_b;
  const float* norm2_w;
  const float* norm2_b;
} nova_vit_block;

/* x[S*L, D] <- blocks[nblocks-1](...blocks[0](x)) in place, post-norm residual blocks with fused
 * QKV+RoPE, flash attention, GELU MLP. Replaces the `for blk in self.blocks[...]` loops of
 * VisionTransformer.forward (vision_transformer.py:137-138,144-145) and Block.forward (:89-92).
 * Workspaces: ws_qkv [S*L, 3D], ws_a [S*L, D], ws_b [S*L, D], ws_h [S*L, hidden] in `dtype`. */
int nova_vit_blocks_forward(const nova_vit_block* blocks, int nblocks, void* x, int S, int L, int D, int heads,
                            int hidden, const float* rope, int rope_batch, void* ws_qkv, void* ws_a, void* ws_b,
                            void* ws_h, int dtype, void* stream);

/* MX-fp8 weights of one block's three large GEMMs (BASELINE configs[4]): OCP e4m3 bytes in nn.Linear's [N][K] layout
 * + one float32 scale per output row (w = w8 * ws[n]), made once with nova_quantize_rows_fp8 on the bf16 weights. */
typedef struct {
  const void* qkv_w8;  const float* qkv_ws;   /* [3D, D], [3D] */
  const void* fc1_w8;  const float* fc1_ws;   /* [4D, D], [4D] */
  const void* fc2_w8;  const float* fc2_ws;   /* [D, 4D], [D]  */
} nova_vit_block_fp8;

/* Building blocks of the fp8 stack, exposed for tests: the post-norm residual LayerNorm (vision_transformer.py:78-82,91-92)
 * that also emits its bf16 output row as e4m3 + per-row scale, bit-compatible with nova_quantize_rows_fp8(out); and the
 * fused QKV projection on fp8 operands with the RoPE / q-scale epilogue of nova_qkv_rope (bf16 result). */
int nova_row_norm_fp8(const void* in, void* out, const float* gamma, const float* beta, const void* res, void* out8, float* out8_scale,
                      long rows, int D, float eps, void* stream);
/* out8[M,N] (e4m3 bytes) = saturate(GELU((A8 . W8^T) * a_scale[m] * w_scale[n] + bias) / *out_scale), and *out_amax raised
 * (atomic max on the float's bits) to the largest |GELU(.)|: the fc1 of the fp8 stack under delayed scaling. */
int nova_gemm_fp8_gelu_q8(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const float* bias, void* out8,
                          int M, int N, int K, const float* out_scale, unsigned* out_amax, void* stream);
int nova_qkv_rope_fp8(const void* x8, const float* x_scale, const void* w8, const float* w_scale, const float* bias, const float* rope,
                      void* qkv, int S, int L, int D, int heads, int rope_batch, float q_scale, void* stream);

/* nova_vit_blocks_forward with the fused-QKV, fc1 and fc2 GEMMs of every block on the block-scaled fp8 MFMA
 * (v_mfma_scale_f32_16x16x128_f8f6f4, 2x the bf16 rate): activations are quantised per row on the fly (the residual
 * stream by the LayerNorm kernel that produces it, the MLP hidden rows by one pass), f32 accumulation, bf16 results;
 * attention, its out-projection, the LayerNorms and the residual stream are as in the bf16 stack. `blocks` supplies the
 * biases, norms and the bf16 out-projection, `q` the fp8 weights. bf16 activations only. The reference has no fp8 path:
 * results are compared with the bf16 stack (tests), not with the reference. Extra workspaces: ws_x8 [S*L, D] bytes,
 * ws_xs [S*L] f32, ws_h8 [S*L, hidden] bytes, ws_hs [S*L] f32. Needs D, hidden % 256 == 0 and L >= 16.
 * h_scale / h_amax: both NULL (the MLP hidden rows are quantised per row by a pass between fc1 and fc2), or device arrays of
 * nblocks floats / unsigned ("delayed scaling"): fc1's epilogue writes GELU(.) / h_scale[i] as e4m3 itself, saturated at +-448,
 * and raises h_amax[i] (float bits, atomic max) to the largest |GELU(.)| it saw; fc2 uses h_scale[i] for every row. The
 * caller zeroes h_amax and sets h_scale[i] = margin * amax_i / 448 from the PREVIOUS call of the same stack (first call: a
 * guess) - NovaEngine does, per lane. */
int nova_vit_blocks_forward_fp8(const nova_vit_block* blocks, const nova_vit_block_fp8* q, int nblocks, void* x, int S, int L, int D,
                                int heads, int hidden, const float* rope, int rope_batch, void* ws_qkv, void* ws_a, void* ws_b,
                                void* ws_h, void* ws_x8, float* ws_xs, void* ws_h8, float* ws_hs, float* h_scale, unsigned* h_amax,
                                void* stream);

/* The same block stack for the conditioning encoder of multi-frame generation (max_latent_length > 1): the k | v rows
 * each block's fused QKV projection produces for the L rows of x are appended to that block's cache and attention runs
 * over cache_len + L keys (vision_transformer.py:55-60: `torch.cat([cache_kv, k], dim=2)`; enable_kvcache :125-126).
 *   kv_cache [nblocks][S][cache_cap][2D] in `dtype` (k then v per row, k already rotated), caller-owned; rows
 *   [0, cache_len) of every sequence are valid on entry, [cache_len, cache_len + L) on return. The caller advances
 *   cache_len by L after the call. rope covers the L new rows only ([rope_batch, L, hd/2, 2]). */
int nova_vit_blocks_forward_kv(const nova_vit_block* blocks, int nblocks, void* x, int S, int L, int D, int heads,
                               int hidden, const float* rope, int rope_batch, void* kv_cache, long cache_cap,
                               long cache_len, void* ws_qkv, void* ws_a, void* ws_b, void* ws_h, int dtype, void* stream);

/* out[r, :] = x[r, :] * (1 + mod[r, 0:D]) + mod[r, D:2D]: AdaLayerNorm with eps=None (no normalisation), the frame mixer
 * `video_encoder.mixer` of transformer_nova.py:87-89 / normalization.py:39-46 applied at transformer_3d.py:156-158. */
int nova_modulate_rows(const void* x, const void* mod, void* out, long rows, int D, int dtype, void* stream);

typedef struct {
  const void* fc1_w;  /* blocks.i.proj.fc1.weight [D, D] */
  const float* fc1_b;
  const void* fc2_w;  /* blocks.i.proj.fc2.weight [D, D] */
  const float* fc2_b;
  const float* norm2_w; /* blocks.i.norm2 */
  const float* norm2_b;
} nova_mlp_block;

typedef struct {
  int depth;              /* number of DiffusionBlocks (6) */
  const nova_mlp_block* blocks;
  const void* adaln_w;    /* cat(blocks.i.norm1.proj.weight (3D each), norm.proj.weight (2D)) [(3*depth+2)D, D] */
  const float* adaln_b;   /* same concatenation of the biases */
  const void* patch_w;    /* patch_embed.proj.weight as [D, P] in patchified (i, j, c) order */
  const float* patch_b;
  const void* head_w;     /* head.weight [P, D] */
  const float* head_b;
} nova_decoder;

/* One sampler step, prepared on the host (float32): with v = CFG-combined head output,
 *   x0 = clamp(kx*x + kv*v, +-clip) (clip <= 0: none);   x <- c0*x0 + cx*x + sigma*noise
 * Flow-matching Euler (scheduling_cfm.py:134-136): kx=0, kv=1, clip=0, c0=sigma_{i+1}-sigma_i, cx=1, sigma=0.
 * DDPM (scheduling_ddpm.py:236-316): kx, kv from prediction_type (:271-280), clip = clip_sample_range (:283-289),
 * c0 / cx the posterior-mean coefficients (:293-298), sigma the posterior std (:303-312).
 * guidance <= 1 disables CFG for that step (guidance_trunc, guidance_scaler.py:59-65).
 * 3-pass guidance (guidance_scaler.py:46-57,78-85; rows [cond ; uncond ; third], S = 3B): extra_kind 1 = image guidance
 * (third = uncond text with the image condition): v = u + g (c - t) [renorm] + extra_scale (t - u); extra_kind 2 =
 * spatiotemporal guidance (third = cond text): v = u + g (c - u) [renorm] + extra_scale (c - t); 0 = 2-pass. */
typedef struct {
  float guidance, kx, kv, clip, c0, cx, sigma;
  float extra_scale;
  int extra_kind;
} nova_sampler_step;

/* All `steps` sampler steps of Transformer3DModel.denoise (transformer_3d.py:102-113) for the n tokens predicted in
 * this AR step, launched back to back on `stream`:
 *   zc    [S*n, D]   condition rows: condition_proj(LN(z)[pred_ids]) (time term NOT yet added)
 *   temb  [steps, D] timestep_proj(freq(t_i)) per step (diffusion_mlp.py:73)
 *   x     [B, n, P]  f32, in: noise rows, out: denoised patch vectors
 *   sched [steps]    host array of nova_sampler_step
 *   noise [steps, B, n, P] f32 or NULL: the per-step gaussian rows of an ancestral sampler (used where sigma != 0)
 *   renorm           guidance_renorm (>= 1: off). When < 1 (flow-matching Euler only): guidance_scaler.py:67-72 with
 *                    echo_energy [B] f32 in/out = squared norm of each sample's rows that are NOT predicted in this AR
 *                    step (they echo x_t in the reference and enter both norms), ws_v [2*B*n*P] f32 scratch
 *                    ([3*B*n*P] with 3-pass guidance).
 * S = 2B when any sched[i].guidance > 1 (cond rows then uncond rows; 3B with a third guidance pass), else S = B.
 * Workspaces in `dtype`: ws_u, ws_h, ws_f, ws_g [S*n, D]; ws_a [mod_steps*S*n, D]; ws_mod [mod_steps*S*n, (3*depth+2)*D].
 * mod_steps = 1: the AdaLN projection of SiLU(zc + temb[i]) (normalization.py:35) is computed inside every step;
 * mod_steps = steps: for all steps in ONE GEMM ahead of the loop (the condition rows do not change during the loop,
 * diffusion_mlp.py:93-95), which needs the steps-times larger ws_a / ws_mod. Same results either way.
 * The whole plan is checked before the first launch: a refused call (mod_steps, S, a step that needs more guidance passes
 * than S / B, extra_kind, P > 64, renorm < 1 with a step that is not the Euler step) launches nothing and leaves x as it was. */
int nova_decoder_denoise(const nova_decoder* dec, const void* zc, const void* temb, float* x, const nova_sampler_step* sched,
                         const float* noise, float renorm, float* echo_energy, int steps, int S, int B, int n, int P, int D,
                         void* ws_a, void* ws_u, void* ws_h, void* ws_f, void* ws_g, void* ws_mod, float* ws_v, int mod_steps,
                         int dtype, void* stream);

/* The same loop with guidance_renorm < 1 for ANY sampler step (the DDPM ancestral step of scheduling_ddpm.py:236-316: noise and a
 * clamp act on the rows that merely echo x_t, so their squared norm is not a scalar that evolves by itself): the echo rows are
 * carried explicitly and take every step beside the predicted ones (guidance_scaler.py:67-72 norms over all N rows; for an echo
 * row every guidance pass returns x_t).
 *   echo_rows  [B, Ne, P] f32 in/out: the Ne = N - n rows of each sample that are not predicted in this AR step (in: their x_T)
 *   echo_noise [steps, B, Ne, P] f32 or NULL: their per-step gaussian rows (used where sigma != 0)
 * Everything else as nova_decoder_denoise (ws_v as for renorm there). Launched directly (no graph replay: per-call noise). */
int nova_decoder_denoise_echo(const nova_decoder* dec, const void* zc, const void* temb, float* x, const nova_sampler_step* sched,
                              const float* noise, float renorm, float* echo_rows, const float* echo_noise, int Ne, int steps, int S, int B,
                              int n, int P, int D, void* ws_a, void* ws_u, void* ws_h, void* ws_f, void* ws_g, void* ws_mod, float* ws_v,
                              int mod_steps, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NOVA_HIP_H_ */
