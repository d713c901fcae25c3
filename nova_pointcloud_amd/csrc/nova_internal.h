// Internal declarations shared by the kernel translation units and the C ABI (capi.hip, denoise.hip). The point-set files declare nothing
// here: each defines its extern "C" entry points itself and takes only set_error, check_launch, NOVA_REQUIRE and NOVA_TRY from this header.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/nova_hip.h"

#include "common.h"

namespace nova {

// storage dtype code <-> element type. Every dtype-generic launcher goes through dispatch_dtype, so a new storage type is
// one more branch here plus the traits in common.h.
template <typename T> constexpr int dtype_of() { return sizeof(T) == 4 ? NOVA_F32 : NOVA_BF16; }
template <> constexpr int dtype_of<f16_t>() { return NOVA_F16; }
inline bool dtype_is16(int dtype) { return dtype == NOVA_BF16 || dtype == NOVA_F16; }
template <typename F> inline auto dispatch_dtype(int dtype, F&& f) {
  return dtype == NOVA_BF16 ? f(bf16_t{}) : dtype == NOVA_F16 ? f(f16_t{}) : f(float{});
}
template <typename F> inline auto dispatch_half(int dtype, F&& f) { return dtype == NOVA_F16 ? f(f16_t{}) : f(bf16_t{}); }
inline bool bad_dtype(int dtype) { return dtype != NOVA_F32 && dtype != NOVA_BF16 && dtype != NOVA_F16; }
inline size_t esize(int dtype) { return dtype_is16(dtype) ? 2 : 4; }

// thread-local last-error record; returns `code` so callers can `return set_error(...)`.
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// hipGetLastError() -> NOVA_ERR_LAUNCH (+ message) or 0. Never synchronises.
int check_launch(const char* what);
#define NOVA_REQUIRE(cond, code, ...) do { if (!(cond)) return set_error(code, __VA_ARGS__); } while (0)
#define NOVA_TRY(expr) do { const int rc_ = (expr); if (rc_ != 0) return rc_; } while (0)

// ---- optional per-kernel timing with HIP events on the launch stream (capi.hip). Slots: one per
// kernel family; `work` = algorithmic FLOPs (or bytes) of the launch. No-ops unless enabled.
// PROF_GEMM_* : the 256x256 (large-M, encoder) GEMM kernels by epilogue (PROF_GEMM_NONE: bias-only launches with K <= N, the
// out-projection; PROF_GEMM_WIDEK: bias-only launches with K > N, the MLP's second projection); PROF_GEMM_SMALL: the 128x128 and
// small-M kernels, any epilogue; PROF_TOKENS: the token plumbing of the split encoder (canvas embedding, sequence build / scatter,
// RoPE table, KV append, frame mixer, fp8 row quantisation); PROF_DECODER: the diffusion MLP's glue kernels (timestep features,
// SiLU-add, patch embedding of the predicted rows, head + guidance + sampler step)
enum { PROF_GEMM_NONE = 0, PROF_GEMM_GELU, PROF_GEMM_SILU, PROF_GEMM_ROPE, PROF_ATTN, PROF_ROWNORM, PROF_GEMM_SMALL, PROF_GEMM_WIDEK,
       PROF_TOKENS, PROF_DECODER, PROF_SLOTS };
inline int prof_gemm_slot(int epi, int N, int K) { return epi == 0 && K > N ? PROF_GEMM_WIDEK : PROF_GEMM_NONE + epi; }
struct ProfScope {
  ProfScope(int slot, double work, hipStream_t st);
  ~ProfScope();
  int idx;
  hipStream_t st;
};
bool prof_enabled();  // nova_prof_enable(1) is in force: launches carry event brackets (and the denoising loop is not captured)

// ---- gemm.hip, gemm256.hip: the epilogue of out = epi(A W^T + bias), one vocabulary for every GEMM structure
struct GemmEpi {
  const float* bias;     // [N] or nullptr
  const float* rope;     // [rope_batch, L, hd/2, 2] (cos, sin) or nullptr
  int L;                 // tokens per sequence (rows m -> (s = m / L, l = m % L))
  int rope_batch;        // table batch count; sequence s uses table s % rope_batch
  int hd;                // head dim
  int rope_cols;         // columns [0, rope_cols) are rotated (q and k thirds of the fused QKV)
  float q_scale;         // columns [0, q_cols) are multiplied by this after rotation (softmax scale folded into q)
  int q_cols;
};
inline GemmEpi epi_bias(const float* bias) { return {bias, nullptr, 1, 1, 2, 0, 1.0f, 0}; }
// the fused QKV projection [.., 3D]: q and k thirds rotated where there is a table, the q third scaled where q_scale says anything
inline GemmEpi epi_qkv(const float* bias, const float* rope, int L, int rope_batch, int hd, int D, float q_scale) {
  return {bias, rope, L, rope ? rope_batch : 1, hd, rope ? 2 * D : 0, q_scale, q_scale != 1.0f ? D : 0};
}
// EPI_NONE .. EPI_SILU are the public activation codes (NOVA_ACT_*). EPI_GELU_Q8 (fp8 operands only, gemm256.hip): GELU, then the
// result is written as OCP e4m3 bytes, value / *q8_scale saturated at +-448, instead of bf16 - the A operand of the next fp8 GEMM
// without a quantisation pass ("delayed scaling": the caller derives the next call's scale from q8_amax).
enum { EPI_NONE = 0, EPI_GELU = 1, EPI_SILU = 2, EPI_ROPE = 3, EPI_GELU_Q8 = 5 };
// epilogue code -> compile-time tag, for the four epilogues every structure and storage type has: f(std::integral_constant<int, EPI_x>{})
// launches; returns 0, or the error for any other code
template <typename F> inline int dispatch_epi(int epi, F&& f) {
  switch (epi) {
    case EPI_NONE: f(std::integral_constant<int, EPI_NONE>{}); return 0;
    case EPI_GELU: f(std::integral_constant<int, EPI_GELU>{}); return 0;
    case EPI_SILU: f(std::integral_constant<int, EPI_SILU>{}); return 0;
    case EPI_ROPE: f(std::integral_constant<int, EPI_ROPE>{}); return 0;
    default: return set_error(NOVA_ERR_ARG, "gemm: unknown epilogue %d", epi);
  }
}
int gemm_bias_act(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int act,
                  int dtype, hipStream_t st);
int gemm_qkv_rope(const void* x, const void* Wqkv, const float* bias, const float* rope, void* qkv, int S, int L,
                  int D, int heads, int rope_batch, int dtype, hipStream_t st, float q_scale = 1.0f);

int gemm_rope_cols(const void* x, const void* W, const float* bias, const float* rope, void* out, int M, int N, int K,
                   int L, int rope_batch, int hd, int rope_cols, int dtype, hipStream_t st);
int gemm_force_tile(int tile);  // 0 on success, -1 for a value this build does not know
int gemm_forced_tile();  // the calling thread's current setting (part of the decoder graph key)
// traversal direction of the NEXT launches of the row-tiled kernels (persistent GEMM, attention, row_norm); see
// xcd_remap_dir in common.h. Set by the block composites, false for direct calls of the single-kernel entry points.
void walk_reverse(bool on);
bool walk_is_reverse();

// ---- attn.hip
// kv_seq_stride: elements between the first key rows of consecutive sequences (0 = Lk * kv_row_stride, i.e. packed);
// a KV cache of capacity cap rows per sequence passes cap * kv_row_stride.
int attn_fwd(const void* q, const void* k, const void* v, void* o, int S, int heads, int Lq, int Lk, int hd,
             long q_row_stride, long kv_row_stride, long o_row_stride, float scale, int dtype, hipStream_t st,
             bool q_prescaled = false, long kv_seq_stride = 0, float* lse = nullptr, const int* klim = nullptr);
// One 16-bit forward call as its kernels take it: cl = what q still has to be multiplied by (1 when its producer folded
// scale * log2 e in), klim [Lq] the optional per-query key limit (training forward, block-causal frame mask).
struct AttnFwdArgs {
  const void *q, *k, *v;
  void* o;
  int S, heads, Lq, Lk, hd;
  long q_rs, kv_rs, o_rs;
  float cl;
  int dtype;
  hipStream_t st;
  long kv_ss;
  float* lse;
  const int* klim;
};
// Every 16-bit forward kernel takes the same leading arguments (a masked one: klim after them), named here once. One workgroup
// = rows_per_wg query rows of one (sequence, head); attn_fwd has checked the grid at 128 rows, the smallest.
template <typename E, typename K, typename... X> inline void attn_launch(K kernel, int rows_per_wg, const AttnFwdArgs& a, X... extra) {
  const int nq = (a.Lq + rows_per_wg - 1) / rows_per_wg;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((long)nq * a.heads * a.S)), dim3(256), 0, a.st, (const E*)a.q, (const E*)a.k, (const E*)a.v, (E*)a.o,
                     a.Lq, a.Lk, a.q_rs, a.kv_rs, a.o_rs, a.cl, a.heads, nq, walk_is_reverse() ? 1 : 0, a.kv_ss, a.lse, extra...);
}
// Which head_dim 64 structure a variant number (nova_debug_set_attn_variant) means: the MFMA shape (32 = attn_bf16 in attn.hip,
// 16 = attn16.hip), 16-query blocks per wave, row sums on the matrix pipe, software-pipelined (P V of tile t-1 beside the
// exponentials of tile t). head_dim 96 and the masked forward are built as ATTN_FORMS[3] only, whatever is asked of the 16x16 family.
struct AttnForm {
  int mfma, nqb;
  bool summ, pipelined;
};
constexpr AttnForm ATTN_FORMS[6] = {{32, 2, false, false}, {16, 2, false, false}, {16, 4, false, false},
                                    {16, 2, true, false},  {16, 4, true, false},  {16, 4, true, true}};
// 16x16x32, 32 rows per wave, row sums on the matrix pipe: +8 .. 11 % over variant 0 at every L measured (profiles/r03_attn_variants_ab.txt)
constexpr int NOVA_ATTN_DEFAULT_VARIANT = 3;
int attn_fwd_m16(const AttnFwdArgs& a, AttnForm f);  // attn16.hip; attn_fwd checks shapes, strides and the grid before it dispatches here
int attn_set_variant(int v);  // -1 default, 0 .. 5 (attn.hip); -1 returned for other values
int attn_variant();
// attn_bwd.hip (bf16, head_dim 64 / 96): gradients of the attention above from q (pre-scaled by scale * log2 e), k, v, the
// forward's output o and log2-domain row log-sum-exp, and dO; delta [S, heads, Lq] is scratch (filled with sum_c dO * O first).
// All matrices token-major with row strides: q, o, dO, dq [S, Lq, heads * hd]; k, v, dk, dv [S, Lk, heads * hd]. Self-attention
// is Lq == Lk with q_rs == kv_rs and dq_rs == dkv_rs (nova_attn_bwd); nova_attn_cross_bwd passes them apart.
int attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse, float* delta, void* dq,
             void* dk, void* dv, int S, int heads, int Lq, int Lk, int hd, long q_rs, long kv_rs, long o_rs, long do_rs, long dq_rs,
             long dkv_rs, float scale, hipStream_t st,
             const int* klim = nullptr);  // klim [Lq]: optional per-query key limit in [1, Lk], non-decreasing

// ---- rowops.hip
struct RowNormArgs {
  const void* in;        // [rows, D]
  void* out;             // [rows, D]
  const float* gamma;    // [D] or null
  const float* beta;     // [D] or null
  const void* mod;       // modulation rows [rows, mod_ld] or null
  long mod_ld;
  int scale_off, shift_off, gate_off;   // column offsets inside a mod row; -1 = absent
  const void* res;       // residual [rows, D] or null
  const int* gather;     // optional source row index per output row (rows of `in`), or null
  long rows;
  int D;
  float eps;
  int rev = 0;           // set by row_norm() from walk_is_reverse(); callers leave it
  void* out8 = nullptr;  // bf16 only, optional: the output row once more as OCP e4m3 bytes [rows, D] with the per-row
  float* out8_scale = nullptr;  // scale amax / 448 [rows] (the fp8 A operand of the next GEMM; same rule as quantize_rows_fp8)
};
int row_norm(const RowNormArgs& a, int dtype, hipStream_t st);

// ---- skinny.hip: small-M GEMM (bf16 / f16, K in {768, 1024}), bit-identical to the tile kernels; optional AdaLN-modulate prologue
bool skinny_gemm_fits(int M, int N, int K, bool modulate);
bool gemm_modulate_fused(int M, int N, int K, int dtype);  // gemm.hip: modulate + GEMM taken as one launch
int skinny_forced_row_blocks();  // the calling thread's current setting (part of the decoder graph key)
void skinny_force_row_blocks(int rb);  // calling thread: 1 / 2 / 4 = rows per workgroup 16 / 32 / 64 for plain launches, 0 = by rule
int skinny_gemm(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int act,
                const RowNormArgs* pro, int dtype, hipStream_t st);
int row_norm_chain(const RowNormArgs& a2, const RowNormArgs& a1, void* x_new_out, int dtype, hipStream_t st);  // rowops.hip, bf16 / f16: two chained norms, one pass
// out = act(modulate(pro) W^T + bias): one launch where skinny.hip applies, else row_norm into pro.out followed by the GEMM
int gemm_modulate_act(const RowNormArgs& pro, const void* W, const float* bias, void* out, int M, int N, int K, int act,
                      int dtype, hipStream_t st);

int rope_table(const float* pos, const long long* ids, float* table, int nb, int pad, int n_tok, int n_pos,
               int hd, const float* inv_freq, hipStream_t st);
int embed_canvas(const float* canvas, const float* mask, const void* w, const float* bias, const void* mask_token,
                 const void* pos_embed, void* z0, int B, int N, int P, int D, int dtype, hipStream_t st);
int build_sequence(const void* prefix, long prefix_seq_rows, const void* tokens, long tok_batch_rows,
                   const long long* ids, void* x, int S, int B, int Lp, int n_sel, int D, int dtype, hipStream_t st);
int scatter_tokens(const void* x1, const long long* ids, void* x2, int S, int B, int Lp, int N, int n_prev, int D,
                   int dtype, hipStream_t st);
int quantize_rows_fp8(const void* x, void* out, float* scale, long rows, int D, hipStream_t st);
// gemm256.hip: C = epi((A8 W8^T) * sa[m] * sw[n] + bias) on MX-fp8 operands (OCP e4m3 bytes); C is bf16, or e4m3 bytes with EPI_GELU_Q8
struct Fp8Gemm {
  const void* A8;       // [M, K]
  const float* sa;      // [M] row scales of A8, or one scale for all rows with sa_scalar
  int sa_scalar = 0;
  const void* W8;       // [N, K]
  const float* sw;      // [N]
  void* C;              // [M, N]
  int M, N, K;
  int epi;              // EPI_*
  GemmEpi e;
  const float* q8_scale = nullptr;  // EPI_GELU_Q8 only: the scale the e4m3 result is divided by ...
  unsigned* q8_amax = nullptr;      // ... and the word that takes max |GELU(.)| (float bits)
};
int gemm256_fp8_launch(const Fp8Gemm& g, hipStream_t st);
int silu_add_rows(const void* a, const void* rowvec, void* out, long rows, int D, int dtype, hipStream_t st);
int silu_add_steps(const void* a, const void* vecs, void* out, long rows, int nvec, int D, int dtype, hipStream_t st);
int timestep_freq(const float* t, const float* freq, void* out, int n, int freq_dim, int dtype, hipStream_t st);
int patch_embed_rows(const float* x, const void* w, const float* bias, void* out, int S, int B, int n, int P, int D,
                     int dtype, hipStream_t st);
using SamplerStep = nova_sampler_step;  // the kernels take the ABI's struct itself (include/nova_hip.h)
int head_cfg_step(const void* h, const void* w, const float* bias, float* x, const float* noise, float* vhat, float* cond,
                  float* extra, int B, int n, int P, int D, const SamplerStep& sp, int defer, int dtype, hipStream_t st);
int scale_vector(float* v, int n, float f, hipStream_t st);
int renorm_euler(float* x, const float* vhat, const float* cond, const float* extra, float* echo, int B, int n, int P, float dt,
                 float renorm, hipStream_t st);
int renorm_step(float* x, const float* vhat, const float* cond, const float* extra, const float* noise, float* echo, const float* echo_noise,
                int B, int nP, int eP, const SamplerStep& sp, float renorm, int echo_only, hipStream_t st);
int kv_append(const void* qkv, void* cache, int S, int Lq, int D, long cap, long base, int dtype, hipStream_t st);
int modulate_rows(const void* x, const void* mod, void* out, long rows, int D, int dtype, hipStream_t st);

}  // namespace nova
