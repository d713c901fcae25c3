// C ABI of libnova_hip.so (include/nova_hip.h): the error and profiling records, the single-kernel wrappers of the model's kernels with their
// argument checks and the ViT block stacks. The denoising loop, its hipGraph cache and the nova_debug_*_graphs entries are denoise.hip; the
// nova_pointset_* entry points are defined in their kernel files (pointset.hip .. assign.hip). All check with nova_internal.h's macros.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <cmath>
#include <mutex>
#include <utility>
#include <vector>
#include "common.h"
#include "nova_internal.h"

namespace nova {

static thread_local char g_err[512] = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  return set_error(NOVA_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// ---- profiling: event pairs recorded around selected launches, summed on nova_prof_collect()
struct ProfRec { hipEvent_t a, b; int slot; double work; };
static std::atomic<bool> g_prof_on{false};
static std::mutex g_prof_mu;  // the record list is shared by all calling threads
static std::vector<ProfRec> g_prof;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;

bool prof_enabled() { return g_prof_on.load(std::memory_order_relaxed); }

ProfScope::ProfScope(int slot, double work, hipStream_t s) : idx(-1), st(s) {
  if (!prof_enabled()) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r;
  if (!g_prof_pool.empty()) {
    r.a = g_prof_pool.back().first;
    r.b = g_prof_pool.back().second;
    g_prof_pool.pop_back();
  } else if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
    return;
  }
  r.slot = slot;
  r.work = work;
  (void)hipEventRecord(r.a, st);
  g_prof.push_back(r);
  idx = (int)g_prof.size() - 1;
}
ProfScope::~ProfScope() {
  if (idx < 0) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (idx < (int)g_prof.size()) (void)hipEventRecord(g_prof[idx].b, st);
}

// Host-side launch state is per calling thread (ctypes releases the GIL during a call): the walk direction is set by a
// composite for the launches it issues itself and restored when it returns, on every path.
static thread_local bool g_walk_rev = false;
void walk_reverse(bool on) { g_walk_rev = on; }
bool walk_is_reverse() { return g_walk_rev; }
#ifdef NOVA_EXPERIMENTS
static int g_walk_alternate = 1;  // nova_debug_force_gemm_tile(50000 / 50001) switches the alternation off / on
void walk_set_alternate(int on) { g_walk_alternate = on; }
#else
constexpr int g_walk_alternate = 1;
#endif
// every launch of a block stack walks its row tiles in the opposite direction of the previous one (fresh-first reads, common.h)
struct Walk {
  int k = 0;
  void next() { walk_reverse(g_walk_alternate && (k++ & 1)); }
  ~Walk() { walk_reverse(false); }
};
}  // namespace nova

using namespace nova;

extern "C" {

int nova_version(void) { return NOVA_HIP_VERSION; }
const char* nova_last_error(void) { return g_err; }

int nova_check_device(void) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(NOVA_ERR_DEVICE, "no HIP device");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return set_error(NOVA_ERR_DEVICE, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(NOVA_ERR_DEVICE, "device %d is %s; libnova_hip is built for gfx950 only", dev, prop.gcnArchName);
  return 0;
}

int nova_debug_force_gemm_tile(int tile) {
  NOVA_REQUIRE(gemm_force_tile(tile) == 0, NOVA_ERR_ARG,
               "force_gemm_tile: this build knows 0 (auto), 16 (small-M kernel; 161 / 162 / 164 with 16 / 32 / 64 rows per workgroup), 64 / 128 (the small-M tile kernels), 256 (persistent), 257 (one tile per workgroup) and 258 (persistent, prologue form); experiment codes need the NOVA_EXPERIMENTS build");
  return 0;
}

int nova_prof_enable(int on) {
  g_prof_on.store(on != 0);
  return 0;
}

int nova_prof_collect(double* ms, double* work, long long* launches, int slots) {
  NOVA_REQUIRE(ms && work && launches && slots >= PROF_SLOTS, NOVA_ERR_ARG, "prof_collect: need %d slots", PROF_SLOTS);
  for (int i = 0; i < slots; ++i) { ms[i] = 0; work[i] = 0; launches[i] = 0; }
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) {
    float t = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
      ms[r.slot] += t;
      work[r.slot] += r.work;
      launches[r.slot] += 1;
    }
    g_prof_pool.emplace_back(r.a, r.b);
  }
  g_prof.clear();
  return 0;
}

int nova_gemm_bias_act(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int act,
                       int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "gemm: bad dtype %d", dtype);
  NOVA_REQUIRE(M == 0 || (A && W && out), NOVA_ERR_ARG, "gemm: null pointer");
  return gemm_bias_act(A, W, bias, out, M, N, K, act, dtype, (hipStream_t)stream);
}

int nova_quantize_rows_fp8(const void* x, void* out, float* scale, long long rows, int D, void* stream) {
  NOVA_REQUIRE(rows <= 0 || (x && out && scale), NOVA_ERR_ARG, "quantize_rows_fp8: null pointer");
  return quantize_rows_fp8(x, out, scale, (long)rows, D, (hipStream_t)stream);
}

int nova_gemm_fp8_bias_act(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const float* bias,
                           void* out, int M, int N, int K, int act, void* stream) {
  NOVA_REQUIRE(M <= 0 || (A8 && a_scale && W8 && w_scale && out), NOVA_ERR_ARG, "gemm_fp8: null pointer");
  NOVA_REQUIRE(act >= NOVA_ACT_NONE && act <= NOVA_ACT_SILU, NOVA_ERR_ARG, "gemm_fp8: bad activation %d", act);
  return gemm256_fp8_launch({.A8 = A8, .sa = a_scale, .W8 = W8, .sw = w_scale, .C = out, .M = M, .N = N, .K = K, .epi = act, .e = epi_bias(bias)},
                            (hipStream_t)stream);
}

int nova_qkv_rope(const void* x, const void* Wqkv, const float* bias, const float* rope, void* qkv, int S, int L, int D,
                  int heads, int rope_batch, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "qkv_rope: bad dtype %d", dtype);
  NOVA_REQUIRE(S * L == 0 || (x && Wqkv && qkv), NOVA_ERR_ARG, "qkv_rope: null pointer");
  return gemm_qkv_rope(x, Wqkv, bias, rope, qkv, S, L, D, heads, rope_batch, dtype, (hipStream_t)stream);
}

int nova_qkv_rope_cols(const void* x, const void* W, const float* bias, const float* rope, void* out, int M, int N, int K,
                       int L, int rope_batch, int head_dim, int rope_cols, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "qkv_rope_cols: bad dtype %d", dtype);
  NOVA_REQUIRE(M == 0 || (x && W && out), NOVA_ERR_ARG, "qkv_rope_cols: null pointer");
  NOVA_REQUIRE(L > 0 && head_dim > 0 && head_dim % 4 == 0 && rope_cols % 128 == 0 && rope_cols <= N, NOVA_ERR_SHAPE,
               "qkv_rope_cols: bad L/head_dim/rope_cols");
  return gemm_rope_cols(x, W, bias, rope, out, M, N, K, L, rope_batch, head_dim, rope_cols, dtype, (hipStream_t)stream);
}

int nova_rope_table(const float* pos, const long long* ids, float* rope, int nb, int pad, int n_tok, int n_pos, int hd,
                    const float* inv_freq, void* stream) {
  NOVA_REQUIRE(pos && rope && inv_freq, NOVA_ERR_ARG, "rope_table: null pointer");
  NOVA_REQUIRE(hd > 0 && hd % 8 == 0, NOVA_ERR_SHAPE, "rope_table: head_dim %d", hd);
  return rope_table(pos, ids, rope, nb, pad, n_tok, n_pos, hd, inv_freq, (hipStream_t)stream);
}

int nova_attn_fwd(const void* q, const void* k, const void* v, void* o, int S, int heads, int Lq, int Lk, int head_dim,
                  long q_row_stride, long kv_row_stride, long o_row_stride, float scale, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "attn_fwd: bad dtype %d", dtype);
  NOVA_REQUIRE(q && k && v && o, NOVA_ERR_ARG, "attn_fwd: null pointer");
  return attn_fwd(q, k, v, o, S, heads, Lq, Lk, head_dim, q_row_stride, kv_row_stride, o_row_stride, scale, dtype,
                  (hipStream_t)stream);
}

int nova_attn_fwd_lse(const void* q_scaled, const void* k, const void* v, void* o, float* lse, int S, int heads, int L,
                      int head_dim, long qkv_row_stride, long o_row_stride, const int* key_limit, void* stream) {
  NOVA_REQUIRE(q_scaled && k && v && o && lse, NOVA_ERR_ARG, "attn_fwd_lse: null pointer");
  return attn_fwd(q_scaled, k, v, o, S, heads, L, L, head_dim, qkv_row_stride, qkv_row_stride, o_row_stride, 1.0f, NOVA_BF16,
                  (hipStream_t)stream, true, 0, lse, key_limit);
}

int nova_attn_bwd(const void* q_scaled, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                  float* delta_scratch, void* dq, void* dk, void* dv, int S, int heads, int L, int head_dim,
                  long qkv_row_stride, long o_row_stride, long do_row_stride, long dqkv_row_stride, float scale,
                  const int* key_limit, void* stream) {
  NOVA_REQUIRE(q_scaled && k && v && o && d_o && lse && delta_scratch && dq && dk && dv, NOVA_ERR_ARG, "attn_bwd: null pointer");
  return attn_bwd(q_scaled, k, v, o, d_o, lse, delta_scratch, dq, dk, dv, S, heads, L, L, head_dim, qkv_row_stride, qkv_row_stride,
                  o_row_stride, do_row_stride, dqkv_row_stride, dqkv_row_stride, scale, (hipStream_t)stream, key_limit);
}

int nova_attn_cross_fwd_lse(const void* q_scaled, const void* k, const void* v, void* o, float* lse, int S, int heads, int Lq, int Lk,
                            int head_dim, long q_row_stride, long kv_row_stride, long o_row_stride, const int* key_limit,
                            void* stream) {
  NOVA_REQUIRE(q_scaled && k && v && o && lse, NOVA_ERR_ARG, "attn_cross_fwd_lse: null pointer");
  if (S <= 0 || Lq <= 0) return 0;
  // the kernels address a sequence's rows with 32-bit byte offsets
  NOVA_REQUIRE((long)Lq * q_row_stride * 2 <= 0x7fffffffL && (long)Lq * o_row_stride * 2 <= 0x7fffffffL &&
                   (long)Lk * kv_row_stride * 2 <= 0x7fffffffL,
               NOVA_ERR_SHAPE, "attn_cross_fwd_lse: a sequence's rows must span < 2 GiB");
  return attn_fwd(q_scaled, k, v, o, S, heads, Lq, Lk, head_dim, q_row_stride, kv_row_stride, o_row_stride, 1.0f, NOVA_BF16,
                  (hipStream_t)stream, true, 0, lse, key_limit);
}

int nova_attn_cross_bwd(const void* q_scaled, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                        float* delta_scratch, void* dq, void* dk, void* dv, int S, int heads, int Lq, int Lk, int head_dim,
                        long q_row_stride, long kv_row_stride, long o_row_stride, long do_row_stride, long dq_row_stride,
                        long dkv_row_stride, float scale, const int* key_limit, void* stream) {
  NOVA_REQUIRE(q_scaled && k && v && o && d_o && lse && delta_scratch && dq && dk && dv, NOVA_ERR_ARG, "attn_cross_bwd: null pointer");
  return attn_bwd(q_scaled, k, v, o, d_o, lse, delta_scratch, dq, dk, dv, S, heads, Lq, Lk, head_dim, q_row_stride, kv_row_stride,
                  o_row_stride, do_row_stride, dq_row_stride, dkv_row_stride, scale, (hipStream_t)stream, key_limit);
}

int nova_row_norm(const void* in, void* out, const float* gamma, const float* beta, const void* mod, long mod_ld,
                  int scale_off, int shift_off, int gate_off, const void* res, const int* gather, long rows, int D,
                  float eps, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "row_norm: bad dtype %d", dtype);
  NOVA_REQUIRE(rows == 0 || (in && out), NOVA_ERR_ARG, "row_norm: null pointer");
  RowNormArgs a{in, out, gamma, beta, mod, mod_ld, scale_off, shift_off, gate_off, res, gather, rows, D, eps};
  return row_norm(a, dtype, (hipStream_t)stream);
}

int nova_row_norm_chain(const void* g, const void* x, const float* gamma, const float* beta, const void* mod, long mod_ld,
                        int gate_off, int scale_off, int shift_off, float eps_first, float eps_second, void* x_new_out,
                        void* h_out, long rows, int D, int dtype, void* stream) {
  NOVA_REQUIRE(dtype_is16(dtype), NOVA_ERR_ARG, "row_norm_chain: dtype %d is not a 16-bit storage type", dtype);
  NOVA_REQUIRE(rows == 0 || (g && x && mod && h_out), NOVA_ERR_ARG, "row_norm_chain: null pointer");
  RowNormArgs a2{g, nullptr, gamma, beta, mod, mod_ld, -1, -1, gate_off, x, nullptr, rows, D, eps_first};
  RowNormArgs a1{nullptr, h_out, nullptr, nullptr, mod, mod_ld, scale_off, shift_off, -1, nullptr, nullptr, rows, D, eps_second};
  return row_norm_chain(a2, a1, x_new_out, dtype, (hipStream_t)stream);
}

int nova_adaln_fc1(const void* x, const void* mod, long mod_ld, int scale_off, int shift_off, float eps, const void* w,
                   const float* bias, void* h, void* out, long rows, int N, int D, int act, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "adaln_fc1: bad dtype %d", dtype);
  NOVA_REQUIRE(rows == 0 || (x && mod && w && h && out), NOVA_ERR_ARG, "adaln_fc1: null pointer");
  NOVA_REQUIRE(rows >= 0 && rows <= 0x7fffffffL && scale_off >= 0 && shift_off >= 0, NOVA_ERR_ARG, "adaln_fc1: bad rows / offsets");
  RowNormArgs m{x, h, nullptr, nullptr, mod, mod_ld, scale_off, shift_off, -1, nullptr, nullptr, rows, D, eps};
  return gemm_modulate_act(m, w, bias, out, (int)rows, N, D, act, dtype, (hipStream_t)stream);
}

int nova_embed_canvas(const float* canvas, const float* mask, const void* w, const float* bias, const void* mask_token,
                      const void* pos_embed, void* z0, int B, int N, int P, int D, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "embed_canvas: bad dtype %d", dtype);
  NOVA_REQUIRE(canvas && mask && w && bias && mask_token && z0, NOVA_ERR_ARG, "embed_canvas: null pointer");
  return embed_canvas(canvas, mask, w, bias, mask_token, pos_embed, z0, B, N, P, D, dtype, (hipStream_t)stream);
}

int nova_build_sequence(const void* prefix, long prefix_seq_rows, const void* tokens, long tok_batch_rows,
                        const long long* ids, void* x, int S, int B, int Lp, int n_sel, int D, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "build_sequence: bad dtype %d", dtype);
  NOVA_REQUIRE(x && (Lp == 0 || prefix) && (n_sel == 0 || tokens) && B > 0, NOVA_ERR_ARG, "build_sequence: null pointer");
  return build_sequence(prefix, prefix_seq_rows, tokens, tok_batch_rows, ids, x, S, B, Lp, n_sel, D, dtype, (hipStream_t)stream);
}

int nova_scatter_tokens(const void* x1, const long long* ids, void* x2, int S, int B, int Lp, int N, int n_prev, int D,
                        int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "scatter_tokens: bad dtype %d", dtype);
  NOVA_REQUIRE(n_prev == 0 || (x1 && ids && x2 && B > 0), NOVA_ERR_ARG, "scatter_tokens: null pointer");
  return scatter_tokens(x1, ids, x2, S, B, Lp, N, n_prev, D, dtype, (hipStream_t)stream);
}

int nova_silu_add_rows(const void* a, const void* rowvec, void* out, long rows, int D, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "silu_add_rows: bad dtype %d", dtype);
  NOVA_REQUIRE(rows == 0 || (a && out), NOVA_ERR_ARG, "silu_add_rows: null pointer");
  return silu_add_rows(a, rowvec, out, rows, D, dtype, (hipStream_t)stream);
}

int nova_timestep_freq(const float* t, const float* freq, void* out, int n, int freq_dim, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "timestep_freq: bad dtype %d", dtype);
  NOVA_REQUIRE(t && freq && out && freq_dim % 2 == 0, NOVA_ERR_ARG, "timestep_freq: bad argument");
  return timestep_freq(t, freq, out, n, freq_dim, dtype, (hipStream_t)stream);
}

int nova_patch_embed_rows(const float* x, const void* w, const float* bias, void* out, int S, int B, int n, int P, int D,
                          int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "patch_embed_rows: bad dtype %d", dtype);
  NOVA_REQUIRE(x && w && bias && out && B > 0, NOVA_ERR_ARG, "patch_embed_rows: null pointer");
  return patch_embed_rows(x, w, bias, out, S, B, n, P, D, dtype, (hipStream_t)stream);
}

int nova_head_cfg_euler(const void* h, const void* w, const float* bias, float* x, int B, int n, int P, int D,
                        float guidance, int cfg, float dt, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "head_cfg_euler: bad dtype %d", dtype);
  NOVA_REQUIRE(h && w && bias && x, NOVA_ERR_ARG, "head_cfg_euler: null pointer");
  // the kernel takes "guidance > 1" as the CFG switch; cfg != 0 with g <= 1 still combines (u + g (c - u))
  NOVA_REQUIRE(!cfg || guidance > 1.0f, NOVA_ERR_ARG, "head_cfg_euler: cfg needs guidance > 1");
  SamplerStep sp{cfg ? guidance : 1.0f, 0.f, 1.f, 0.f, dt, 1.f, 0.f, 0.f, 0};
  return head_cfg_step(h, w, bias, x, nullptr, nullptr, nullptr, nullptr, B, n, P, D, sp, 0, dtype, (hipStream_t)stream);
}


// One invocation of the block stack of VisionTransformer.forward, as the three nova_vit_blocks_forward* entries fill it.
struct VitCall {
  const nova_vit_block* blocks;
  const nova_vit_block_fp8* q = nullptr;  // optional: the weights of the three large linears as e4m3 rows (the fp8 stack below; bf16 only)
  int nblocks;
  void* x;  // [S * L, D], in place
  int S, L, D, heads, hidden;
  const float* rope;
  int rope_batch;
  void *ws_qkv, *ws_a, *ws_b, *ws_h;
  // optional KV cache: the k | v rows of every block are appended to that block's cache ([S][cap][2D], `cache_len` rows already valid) and
  // attention runs over cache_len + L keys (vision_transformer.py:55-60, the conditioning encoder of multi-frame generation)
  void* cache = nullptr;
  long cap = 0, cache_len = 0;
  // with q: x and the MLP hidden rows as e4m3 bytes with their row scales; h_scale / h_amax [nblocks] select delayed scaling of the hidden rows
  void *ws_x8 = nullptr, *ws_h8 = nullptr;
  float *ws_xs = nullptr, *ws_hs = nullptr, *h_scale = nullptr;
  unsigned* h_amax = nullptr;
  int dtype;
  hipStream_t st;
};

// One of a block's three large linears (fused QKV, fc1, fc2 = 11/12 of its GEMM FLOPs): g.C = epi(in W^T + bias), described by g. The launch
// follows the data, not the entry point: the MX-fp8 one where the call carries fp8 weights (g.A8, g.W8), else `in` and `w` in c.dtype.
static int vit_linear(const VitCall& c, const Fp8Gemm& g, const void* in, const void* w) {
  if (c.q) return gemm256_fp8_launch(g, c.st);
  if (g.epi == EPI_ROPE) return gemm_qkv_rope(in, w, g.e.bias, c.rope, g.C, c.S, c.L, c.D, c.heads, c.rope_batch, c.dtype, c.st, g.e.q_scale);
  return gemm_bias_act(in, w, g.e.bias, g.C, g.M, g.N, g.K, g.epi, c.dtype, c.st);
}

// x = LN(ws_b) * w + b + x, the post-norm residual; with `side8` the new x once more as e4m3 rows, the A operand of the next fp8 linear
static int vit_post_norm(const VitCall& c, const float* w, const float* b, bool side8) {
  RowNormArgs n{c.ws_b, c.x, w, b, nullptr, 0, -1, -1, -1, c.x, nullptr, c.S * c.L, c.D, 1e-5f};
  n.out8 = side8 ? c.ws_x8 : nullptr;
  n.out8_scale = side8 ? c.ws_xs : nullptr;
  return row_norm(n, c.dtype, c.st);
}

// The walk over the blocks, for all three entries. With fp8 weights (BASELINE configs[4]) they were quantised once per output row at pack
// time and the activations are quantised per row on the fly: the residual stream by the LayerNorm kernel that produces it (fp8 side
// output), the MLP hidden rows by fc1's epilogue (delayed scaling) or by one quantisation pass. Attention, its out-projection, the
// LayerNorm statistics and the residual stream stay bf16 / f32.
static int vit_blocks(const VitCall& c) {
  const int M = c.S * c.L, D = c.D, hidden = c.hidden, hd = D / c.heads, dtype = c.dtype;
  hipStream_t st = c.st;
  if (M == 0 || c.nblocks == 0) return 0;
  const size_t es = esize(dtype);
  const float scale = 1.0f / sqrtf((float)hd);
  // bf16 / f16: the softmax scale (in the exp2 domain) is folded into q by the QKV epilogue, before the 16-bit rounding
  // (epi_qkv then scales the q third: scale * log2 e is 1 for no head width the library accepts)
  const bool pre = dtype_is16(dtype);
  const float q_scale = pre ? scale * 1.4426950408889634f : 1.0f;
  const bool delayed = c.h_scale != nullptr;
  const char* qkv = static_cast<const char*>(c.ws_qkv);
  Walk walk;
  if (c.q) NOVA_TRY(quantize_rows_fp8(c.x, c.ws_x8, c.ws_xs, M, D, st));  // the stack's input rows; later ones come from the LN kernels
  for (int i = 0; i < c.nblocks; ++i) {
    const nova_vit_block& b = c.blocks[i];
    const nova_vit_block_fp8 w = c.q ? c.q[i] : nova_vit_block_fp8{};
    walk.next();
    NOVA_TRY(vit_linear(c, {.A8 = c.ws_x8, .sa = c.ws_xs, .W8 = w.qkv_w8, .sw = w.qkv_ws, .C = c.ws_qkv, .M = M, .N = 3 * D, .K = D, .epi = EPI_ROPE,
                            .e = epi_qkv(b.qkv_b, c.rope, c.L, c.rope_batch, hd, D, q_scale)},
                        c.x, b.qkv_w));
    walk.next();
    if (c.cache) {
      char* cb = static_cast<char*>(c.cache) + (size_t)i * c.S * c.cap * 2 * D * es;
      NOVA_TRY(kv_append(c.ws_qkv, cb, c.S, c.L, D, c.cap, c.cache_len, dtype, st));
      NOVA_TRY(attn_fwd(qkv, cb, cb + (size_t)D * es, c.ws_a, c.S, c.heads, c.L, (int)(c.cache_len + c.L), hd, 3L * D, 2L * D, D, scale, dtype,
                        st, pre, c.cap * 2L * D));
    } else {
      NOVA_TRY(attn_fwd(qkv, qkv + (size_t)D * es, qkv + (size_t)2 * D * es, c.ws_a, c.S, c.heads, c.L, c.L, hd, 3L * D, 3L * D, D,
                        scale, dtype, st, pre));
    }
    walk.next();
    NOVA_TRY(gemm_bias_act(c.ws_a, b.proj_w, b.proj_b, c.ws_b, M, D, D, NOVA_ACT_NONE, dtype, st));
    walk.next();
    NOVA_TRY(vit_post_norm(c, b.norm1_w, b.norm1_b, c.q != nullptr));
    walk.next();
    // delayed scaling: fc1 writes GELU(.) / h_scale[i] as e4m3 itself and records max |GELU(.)| in h_amax[i], from which the caller sets
    // the scale of the next call, and fc2 reads one scale for all rows; else fp8 hidden rows take one quantisation pass with a scale each
    NOVA_TRY(vit_linear(c, {.A8 = c.ws_x8, .sa = c.ws_xs, .W8 = w.fc1_w8, .sw = w.fc1_ws, .C = delayed ? c.ws_h8 : c.ws_h, .M = M, .N = hidden, .K = D,
                            .epi = delayed ? EPI_GELU_Q8 : EPI_GELU, .e = epi_bias(b.fc1_b), .q8_scale = delayed ? c.h_scale + i : nullptr,
                            .q8_amax = delayed ? c.h_amax + i : nullptr},
                        c.x, b.fc1_w));
    if (c.q && !delayed) NOVA_TRY(quantize_rows_fp8(c.ws_h, c.ws_h8, c.ws_hs, M, hidden, st));
    walk.next();
    NOVA_TRY(vit_linear(c, {.A8 = c.ws_h8, .sa = delayed ? c.h_scale + i : c.ws_hs, .sa_scalar = delayed, .W8 = w.fc2_w8, .sw = w.fc2_ws, .C = c.ws_b,
                            .M = M, .N = D, .K = hidden, .epi = EPI_NONE, .e = epi_bias(b.fc2_b)},
                        c.ws_h, b.fc2_w));
    walk.next();
    NOVA_TRY(vit_post_norm(c, b.norm2_w, b.norm2_b, c.q && i + 1 < c.nblocks));  // fp8: the next block's QKV input
  }
  return 0;
}

int nova_vit_blocks_forward(const nova_vit_block* blocks, int nblocks, void* x, int S, int L, int D, int heads,
                            int hidden, const float* rope, int rope_batch, void* ws_qkv, void* ws_a, void* ws_b,
                            void* ws_h, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "vit_blocks: bad dtype %d", dtype);
  NOVA_REQUIRE(nblocks == 0 || (blocks && x && ws_qkv && ws_a && ws_b && ws_h), NOVA_ERR_ARG, "vit_blocks: null pointer");
  NOVA_REQUIRE(heads > 0 && D % heads == 0, NOVA_ERR_SHAPE, "vit_blocks: D %% heads != 0");
  return vit_blocks({.blocks = blocks, .nblocks = nblocks, .x = x, .S = S, .L = L, .D = D, .heads = heads, .hidden = hidden, .rope = rope,
                     .rope_batch = rope_batch, .ws_qkv = ws_qkv, .ws_a = ws_a, .ws_b = ws_b, .ws_h = ws_h, .dtype = dtype, .st = (hipStream_t)stream});
}

int nova_row_norm_fp8(const void* in, void* out, const float* gamma, const float* beta, const void* res, void* out8, float* out8_scale,
                      long rows, int D, float eps, void* stream) {
  NOVA_REQUIRE(rows == 0 || (in && out && out8 && out8_scale), NOVA_ERR_ARG, "row_norm_fp8: null pointer");
  RowNormArgs a{in, out, gamma, beta, nullptr, 0, -1, -1, -1, res, nullptr, rows, D, eps};
  a.out8 = out8;
  a.out8_scale = out8_scale;
  return row_norm(a, NOVA_BF16, (hipStream_t)stream);
}

int nova_gemm_fp8_gelu_q8(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const float* bias, void* out8,
                          int M, int N, int K, const float* out_scale, unsigned* out_amax, void* stream) {
  NOVA_REQUIRE(M <= 0 || (A8 && a_scale && W8 && w_scale && out8 && out_scale && out_amax), NOVA_ERR_ARG, "gemm_fp8_gelu_q8: null pointer");
  return gemm256_fp8_launch({.A8 = A8, .sa = a_scale, .W8 = W8, .sw = w_scale, .C = out8, .M = M, .N = N, .K = K, .epi = EPI_GELU_Q8,
                             .e = epi_bias(bias), .q8_scale = out_scale, .q8_amax = out_amax},
                            (hipStream_t)stream);
}

int nova_qkv_rope_fp8(const void* x8, const float* x_scale, const void* w8, const float* w_scale, const float* bias, const float* rope,
                      void* qkv, int S, int L, int D, int heads, int rope_batch, float q_scale, void* stream) {
  NOVA_REQUIRE(S * L == 0 || (x8 && x_scale && w8 && w_scale && qkv), NOVA_ERR_ARG, "qkv_rope_fp8: null pointer");
  NOVA_REQUIRE(heads > 0 && D % heads == 0, NOVA_ERR_SHAPE, "qkv_rope_fp8: D %% heads != 0");
  return gemm256_fp8_launch({.A8 = x8, .sa = x_scale, .W8 = w8, .sw = w_scale, .C = qkv, .M = S * L, .N = 3 * D, .K = D, .epi = EPI_ROPE,
                             .e = epi_qkv(bias, rope, L, rope_batch, D / heads, D, q_scale)},
                            (hipStream_t)stream);
}

// The block stack with the three large linears of every block on the MX-fp8 MFMA path (vit_blocks above)
int nova_vit_blocks_forward_fp8(const nova_vit_block* blocks, const nova_vit_block_fp8* q, int nblocks, void* x, int S, int L, int D,
                                int heads, int hidden, const float* rope, int rope_batch, void* ws_qkv, void* ws_a, void* ws_b,
                                void* ws_h, void* ws_x8, float* ws_xs, void* ws_h8, float* ws_hs, float* h_scale, unsigned* h_amax,
                                void* stream) {
  NOVA_REQUIRE(nblocks == 0 || (blocks && q && x && ws_qkv && ws_a && ws_b && ws_h && ws_x8 && ws_xs && ws_h8 && ws_hs), NOVA_ERR_ARG,
               "vit_blocks_fp8: null pointer");
  NOVA_REQUIRE((h_scale == nullptr) == (h_amax == nullptr), NOVA_ERR_ARG, "vit_blocks_fp8: h_scale and h_amax come together");
  NOVA_REQUIRE(heads > 0 && D % heads == 0, NOVA_ERR_SHAPE, "vit_blocks_fp8: D %% heads != 0");
  NOVA_REQUIRE(D % 256 == 0 && hidden % 256 == 0, NOVA_ERR_SHAPE, "vit_blocks_fp8: D and hidden must be multiples of 256");
  NOVA_REQUIRE(!rope || L >= 16, NOVA_ERR_SHAPE, "vit_blocks_fp8: L >= 16 with RoPE");
  return vit_blocks({.blocks = blocks, .q = q, .nblocks = nblocks, .x = x, .S = S, .L = L, .D = D, .heads = heads, .hidden = hidden, .rope = rope,
                     .rope_batch = rope_batch, .ws_qkv = ws_qkv, .ws_a = ws_a, .ws_b = ws_b, .ws_h = ws_h, .ws_x8 = ws_x8, .ws_h8 = ws_h8,
                     .ws_xs = ws_xs, .ws_hs = ws_hs, .h_scale = h_scale, .h_amax = h_amax, .dtype = NOVA_BF16, .st = (hipStream_t)stream});
}

int nova_vit_blocks_forward_kv(const nova_vit_block* blocks, int nblocks, void* x, int S, int L, int D, int heads,
                               int hidden, const float* rope, int rope_batch, void* kv_cache, long cache_cap,
                               long cache_len, void* ws_qkv, void* ws_a, void* ws_b, void* ws_h, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "vit_blocks_kv: bad dtype %d", dtype);
  NOVA_REQUIRE(nblocks == 0 || (blocks && x && kv_cache && ws_qkv && ws_a && ws_b && ws_h), NOVA_ERR_ARG, "vit_blocks_kv: null pointer");
  NOVA_REQUIRE(heads > 0 && D % heads == 0, NOVA_ERR_SHAPE, "vit_blocks_kv: D %% heads != 0");
  NOVA_REQUIRE(cache_len >= 0 && cache_len + L <= cache_cap, NOVA_ERR_SHAPE, "vit_blocks_kv: %ld cached + %d new rows exceed the capacity %ld",
               cache_len, L, cache_cap);
  return vit_blocks({.blocks = blocks, .nblocks = nblocks, .x = x, .S = S, .L = L, .D = D, .heads = heads, .hidden = hidden, .rope = rope,
                     .rope_batch = rope_batch, .ws_qkv = ws_qkv, .ws_a = ws_a, .ws_b = ws_b, .ws_h = ws_h, .cache = kv_cache, .cap = cache_cap,
                     .cache_len = cache_len, .dtype = dtype, .st = (hipStream_t)stream});
}

int nova_modulate_rows(const void* x, const void* mod, void* out, long rows, int D, int dtype, void* stream) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "modulate_rows: bad dtype %d", dtype);
  NOVA_REQUIRE(rows == 0 || (x && mod && out), NOVA_ERR_ARG, "modulate_rows: null pointer");
  return modulate_rows(x, mod, out, rows, D, dtype, (hipStream_t)stream);
}

int nova_debug_set_attn_variant(int variant) {
  NOVA_REQUIRE(attn_set_variant(variant) == 0, NOVA_ERR_ARG, "nova_debug_set_attn_variant: %d is not one of -1 .. 5", variant);
  return 0;
}

}  // extern "C"
