// Fused bias-dropout-residual, forward and backward: the three elementwise chains of the transformer body of the reference's
// point-cloud models, diffnext/models/transformers/transformer_pointcloud_nova.py:
//   nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward=4*d_model, dropout=0.1, batch_first=True, norm_first=True)
//   stacked at :433-441 and :590-598, run at :510 and :775; dropout=0.1 from train_newloss.py:652, :673
//     x = x + dropout1(out_proj(attn(norm1(x))))                      bias + dropout + residual on [B, N, E]
//     x = x + dropout2(linear2(dropout(relu(linear1(norm2(x))))))     bias + ReLU + dropout on [B, N, 4E], then the first form
// The GEMMs stay on the libraries; this is what follows each of them, in one pass: every operand read once, the output
// written once, and the mask a pure function of (seed, subsequence, element index) that is regenerated, never stored. The
// definition (the generator, every rounding, the order of the bias gradient's sum) is in include/nova_hip.h at
// nova_bias_dropout_add; this file is that text as code.
//
//   dropout_add_kernel<T, BWD, RELU, WIDE, CHUNKED>  one kernel body for both directions. A thread owns one column group of a row, 16
//     bytes (4 float32 or 8 16-bit elements), and walks rows: DA_AHEAD of them per step, their loads issued together. A
//     group of 4 elements whose flat index starts on a multiple of 4 takes its four draws from ONE Philox4x32-10 evaluation.
//     Two launch shapes, the same per-element arithmetic:
//       flat     (forward; backward without the bias gradient) thread v of the grid owns column group v % G and the rows
//                v / G, v / G + step, ...: the grid is a multiple of G threads, so the group, its columns and its bias values
//                are fixed per thread and no division stands in the loop. No lane idles whatever G is.
//       chunked  (backward with gbias_parts) one workgroup column per DA_CHUNK = 128 rows: the thread walks the chunk's rows
//                in ascending order and adds its float32 gx values to accumulators that start from +0; the chunk's row of
//                gbias_parts is written by plain stores. No cross-lane reduction, no atomics, no LDS. There is about one
//                wave per SIMD here (rows / 128 x D / 8 threads), so the loads of the next step are issued before the
//                arithmetic of this one.
//   WIDE: D % VEC == 0 and every row pointer on 16 bytes: one 16-byte access per operand and row, and the group's flat index
//     is a multiple of 4, so 1 (float32) or 2 (16-bit) Philox evaluations serve it. Otherwise the same column groups move
//     element by element, the last group of a row is short, and a group that starts off a multiple of 4 takes one more
//     evaluation: the same draws for the same elements, the same bits.
// Cost per element (counted): one Philox evaluation is 20 32 x 32 -> 64-bit multiplies for 4 elements; the
// compiler forms each round's two products as full 64-bit ones, so the high and the low word cost one multiply together.
#include "fused_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int DA_MAX_D = NOVA_DROPOUT_MAX_DIM;  // include/nova_hip.h
constexpr int DA_CHUNK = NOVA_DROPOUT_CHUNK;    // rows per row of gbias_parts
constexpr int DA_T = 256;                       // threads per workgroup
constexpr int DA_FLAT_BLOCKS = 4096;            // flat shape: about this many workgroups, 16 per compute unit (no part of the definition)
constexpr unsigned long long DA_T_MAX = 1ull << 32;
constexpr long long DA_MAX_ROW = 1ll << 48;  // first_row + rows: the flat index stays below 2^62
static_assert(DA_CHUNK == 128 && DA_MAX_D == 16384, "the chunk and the width limit are part of the definition");

constexpr int DA_AHEAD = 4;  // rows a thread works on per step (no part of the definition)

// Philox4x32-10 (Salmon et al., Random123): ten rounds, the key bumped by the Weyl constants after every round
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

struct DaArgs {
  const void* in;      // forward: x; backward: g
  const void* aux;     // forward: residual or NULL; backward: the saved out (RELU) or NULL
  const float* bias;   // forward: [D] or NULL
  void* res;           // forward: out; backward: gx or NULL
  float* parts;        // backward, chunked: gbias_parts [ceil(rows / 128), D]
  long long rows, first_row;
  int D, G;            // G = ceil(D / VEC) column groups per row
  unsigned long long T, sub;
  uint32_t k0, k1;
  float scale;
  unsigned row_step;   // flat: threads of the grid / G
};

// a group as loaded: the 16 bytes as they are (WIDE), or the nc <= VEC elements one by one, already float32
template <typename T, bool WIDE> struct DaRaw { u4v v; };
template <typename T> struct DaRaw<T, false> { float f[16 / sizeof(T)]; };

template <typename T, bool WIDE> __device__ __forceinline__ void da_load(const T* __restrict__ p, int nc, DaRaw<T, WIDE>& raw) {
  constexpr int VEC = 16 / sizeof(T);
  if constexpr (WIDE) raw.v = *reinterpret_cast<const u4v*>(p);
  else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) raw.f[j] = j < nc ? to_f<T>(p[j]) : 0.f;
  }
}

// the group's elements converted exactly to float32
template <typename T, bool WIDE> __device__ __forceinline__ void da_unpack(const DaRaw<T, WIDE>& raw, float (&v)[16 / sizeof(T)]) {
  constexpr int VEC = 16 / sizeof(T);
  if constexpr (WIDE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (sizeof(T) == 4) v[k] = __uint_as_float(raw.v[k]);
      else {
        const f2v h = Half16<T>::unpack(raw.v[k]);
        v[2 * k] = h[0], v[2 * k + 1] = h[1];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = raw.f[j];
  }
}

// the group's elements to p in T, each rounded once to nearest even (float32: as they are)
template <typename T, bool WIDE> __device__ __forceinline__ void da_store(T* __restrict__ p, int nc, const float (&v)[16 / sizeof(T)]) {
  constexpr int VEC = 16 / sizeof(T);
  if constexpr (WIDE) {
    u4v t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (sizeof(T) == 4) t[k] = __float_as_uint(v[k]);
      else t[k] = Half16<T>::pack(v[2 * k], v[2 * k + 1]);
    }
    *reinterpret_cast<u4v*>(p) = t;
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (j < nc) p[j] = from_f<T>(v[j]);
  }
}

// keep[j] for the VEC elements from flat index i0 on: word (i0 + j) & 3 of Philox at counter (i0 + j) >> 2, kept iff >= T.
// WIDE: i0 is a multiple of 4
template <int VEC, bool WIDE> __device__ __forceinline__ void da_keep(const DaArgs& a, uint64_t i0, bool (&keep)[VEC]) {
  constexpr int NQ = VEC / 4 + (WIDE ? 0 : 1);
  const uint64_t q0 = i0 >> 2;
  const int sh = WIDE ? 0 : (int)(i0 & 3);
  uint32_t w[NQ * 4];
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    uint32_t o[4] = {0, 0, 0, 0};
    if (k < VEC / 4 || sh != 0) philox4x32_10((uint32_t)(q0 + k), (uint32_t)((q0 + k) >> 32), (uint32_t)a.sub, (uint32_t)(a.sub >> 32), a.k0, a.k1, o);
    w[4 * k] = o[0], w[4 * k + 1] = o[1], w[4 * k + 2] = o[2], w[4 * k + 3] = o[3];
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    uint32_t d = w[j];
    if constexpr (!WIDE) d = sh == 0 ? w[j] : sh == 1 ? w[j + 1] : sh == 2 ? w[j + 2] : w[j + 3];
    keep[j] = (uint64_t)d >= a.T;
  }
}

template <typename T, bool BWD, bool RELU, bool WIDE, bool CHUNKED> __global__ __launch_bounds__(DA_T) void dropout_add_kernel(const DaArgs a) {
  static_assert(BWD || !CHUNKED, "the chunked shape serves the bias gradient");
  constexpr int VEC = 16 / sizeof(T), AHEAD = DA_AHEAD;
  const int D = a.D;
  int cg;
  long long r, r1, rs;
  if constexpr (CHUNKED) {
    cg = blockIdx.y * DA_T + threadIdx.x;
    r = (long long)blockIdx.x * DA_CHUNK, r1 = r + DA_CHUNK < a.rows ? r + DA_CHUNK : a.rows, rs = 1;
    if (cg >= a.G) return;
  } else {
    const uint32_t v0 = blockIdx.x * DA_T + threadIdx.x;
    cg = (int)(v0 % (uint32_t)a.G), r = v0 / (uint32_t)a.G, r1 = a.rows, rs = a.row_step;
  }
  const int col0 = cg * VEC, nc = D - col0 < VEC ? D - col0 : VEC;  // a column past D - 1 is neither read nor written
  const T* in = (const T*)a.in;
  const T* aux = (const T*)a.aux;
  T* res = (T*)a.res;
  const bool masked = a.T != 0 && !(BWD && RELU);  // T == 0: everything is kept and no Philox is evaluated
  float bv[VEC], acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    bv[j] = !BWD && a.bias && j < nc ? a.bias[col0 + j] : 0.f;
    acc[j] = 0.f;
  }
  // the step's AHEAD rows from rb on: their loads are issued together (a row past the last is read at the step's first row
  // and not used)
  auto load = [&](long long rb, DaRaw<T, WIDE>(&bi)[AHEAD], DaRaw<T, WIDE>(&ba)[AHEAD]) {
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const long long rr = rb + u * rs < r1 ? rb + u * rs : rb;
      const size_t off = (size_t)rr * D + col0;
      da_load<T, WIDE>(in + off, nc, bi[u]);
      if (aux) da_load<T, WIDE>(aux + off, nc, ba[u]);
    }
  };
  auto work = [&](long long r, const DaRaw<T, WIDE>(&cin)[AHEAD], const DaRaw<T, WIDE>(&caux)[AHEAD]) {
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const long long rr = r + u * rs;
      if (rr >= r1) break;
      float vin[VEC], vaux[VEC];
      da_unpack<T, WIDE>(cin[u], vin);
      if (aux) da_unpack<T, WIDE>(caux[u], vaux);
      bool keep[VEC];
      if (masked) da_keep<VEC, WIDE>(a, (uint64_t)(a.first_row + rr) * (uint64_t)D + (uint64_t)col0, keep);
      float o[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if constexpr (BWD) {
          const bool on = RELU ? vaux[j] > 0.f : !masked || keep[j];
          o[j] = on ? vin[j] * a.scale : 0.f;
          acc[j] = acc[j] + o[j];
        } else {
          float t = vin[j];
          if (a.bias) t = t + bv[j];  // an absent bias is no addition
          if constexpr (RELU) t = t > 0.f ? t : (t != t ? t : 0.f);
          const float d = !masked || keep[j] ? t * a.scale : 0.f;  // a dropped element is +0 whatever t is
          o[j] = aux ? vaux[j] + d : d;
        }
      }
      if (res) da_store<T, WIDE>(res + (size_t)rr * D + col0, nc, o);
    }
  };
  DaRaw<T, WIDE> cin[AHEAD], caux[AHEAD];
  if constexpr (CHUNKED) {
    // the rows of the NEXT step are loaded before those of this one are worked on: this shape has about one wave per SIMD,
    // and nothing else would cover the Philox rounds with memory traffic
    DaRaw<T, WIDE> nin[AHEAD], naux[AHEAD];
    if (r < r1) load(r, cin, caux);
    for (; r < r1; r += rs * AHEAD) {
      if (r + rs * AHEAD < r1) load(r + rs * AHEAD, nin, naux);
      work(r, cin, caux);
#pragma unroll
      for (int u = 0; u < AHEAD; ++u) cin[u] = nin[u], caux[u] = naux[u];
    }
  } else {
    for (; r < r1; r += rs * AHEAD) {
      load(r, cin, caux);
      work(r, cin, caux);
    }
  }
  if constexpr (CHUNKED) {
    if (a.parts) {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (j < nc) a.parts[(size_t)blockIdx.x * D + col0 + j] = acc[j];
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

static unsigned da_gcd(unsigned a, unsigned b) {
  while (b) {
    const unsigned t = a % b;
    a = b, b = t;
  }
  return a;
}

// checks 2, 3 (without the residual) and 5 .. 7 of the order include/nova_hip.h states, shared by both entries
static int da_check_head(const char* who, int dtype, int act) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "%s: unknown dtype code %d (NOVA_F32, NOVA_BF16, NOVA_F16)", who, dtype);
  NOVA_REQUIRE(act == NOVA_DROPOUT_ACT_NONE || act == NOVA_DROPOUT_ACT_RELU, NOVA_ERR_ARG,
               "%s: unknown act code %d (NOVA_DROPOUT_ACT_NONE, NOVA_DROPOUT_ACT_RELU)", who, act);
  return 0;
}
static int da_check_tail(const char* who, long long rows, int D, long long first_row, unsigned long long T) {
  NOVA_REQUIRE(D >= 1 && D <= DA_MAX_D, NOVA_ERR_SHAPE, "%s: D %d outside 1 .. %d (NOVA_DROPOUT_MAX_DIM)", who, D, DA_MAX_D);
  NOVA_REQUIRE(rows <= NOVA_DROPOUT_MAX_ROWS, NOVA_ERR_SHAPE, "%s: %lld rows exceed one launch (%lld, NOVA_DROPOUT_MAX_ROWS)", who, rows,
               (long long)NOVA_DROPOUT_MAX_ROWS);
  NOVA_REQUIRE(T <= DA_T_MAX, NOVA_ERR_ARG, "%s: threshold T %llu exceeds 2^32 (T = floor(p 2^32), 0 <= p <= 1)", who, T);
  NOVA_REQUIRE(first_row >= 0, NOVA_ERR_ARG, "%s: first_row %lld is negative", who, first_row);
  NOVA_REQUIRE(first_row <= DA_MAX_ROW && (rows <= 0 || rows <= DA_MAX_ROW - first_row), NOVA_ERR_ARG,
               "%s: first_row %lld + rows %lld exceeds 2^48", who, first_row, rows);
  return 0;
}

static void da_launch(DaArgs& a, int dtype, bool bwd, bool relu, bool chunked, hipStream_t st) {
  const int vec = 16 / (int)esize(dtype);
  a.G = (a.D + vec - 1) / vec;
  dim3 grid;
  if (chunked) {
    grid = dim3((unsigned)((a.rows + DA_CHUNK - 1) / DA_CHUNK), (a.G + DA_T - 1) / DA_T);
    a.row_step = 1;
  } else {  // a multiple of G threads: whole workgroups in units of G / gcd(G, 256)
    const unsigned long long unit = (unsigned)a.G / da_gcd((unsigned)a.G, DA_T);
    unsigned long long need = ((unsigned long long)a.rows * a.G + DA_T - 1) / DA_T;
    if (need > DA_FLAT_BLOCKS) need = DA_FLAT_BLOCKS;
    const unsigned long long blocks = (need + unit - 1) / unit * unit;  // below 2 * 4096
    grid = dim3((unsigned)blocks);
    a.row_step = (unsigned)(blocks * DA_T / a.G);
  }
  const uintptr_t bits = (uintptr_t)a.in | (uintptr_t)a.aux | (uintptr_t)a.res;
  const bool wide = a.D % vec == 0 && bits % 16 == 0;
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto go = [&](auto b, auto r, auto w) {
      if constexpr (decltype(b)::value) {
        if (chunked) {
          hipLaunchKernelGGL((dropout_add_kernel<T, true, decltype(r)::value, decltype(w)::value, true>), grid, dim3(DA_T), 0, st, a);
          return;
        }
      }
      hipLaunchKernelGGL((dropout_add_kernel<T, decltype(b)::value, decltype(r)::value, decltype(w)::value, false>), grid, dim3(DA_T), 0, st, a);
    };
    dispatch_flag(bwd, [&](auto b) { dispatch_flag(relu, [&](auto r) { dispatch_flag(wide, [&](auto w) { go(b, r, w); }); }); });
    return 0;
  });
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_bias_dropout_add(const void* x, int dtype, const float* bias, const void* residual, void* out, long long rows, int D,
                          long long first_row, unsigned long long T, float scale, unsigned long long seed,
                          unsigned long long subsequence, int act, void* stream) {
  const char* who = "bias_dropout_add";
  NOVA_REQUIRE(x, NOVA_ERR_ARG, "%s: null pointer x", who);
  NOVA_REQUIRE(out, NOVA_ERR_ARG, "%s: null pointer out", who);  // bias and residual may be NULL
  NOVA_TRY(da_check_head(who, dtype, act));
  NOVA_REQUIRE(!(act == NOVA_DROPOUT_ACT_RELU && residual), NOVA_ERR_ARG, "%s: NOVA_DROPOUT_ACT_RELU takes no residual", who);
  NOVA_TRY(da_check_tail(who, rows, D, first_row, T));
  if (rows <= 0) return 0;
  const size_t n = (size_t)rows * D * esize(dtype);
  const void* ins[3] = {x, bias, residual};
  const size_t nins[3] = {n, (size_t)D * 4, n};
  const char* names[3] = {"x", "bias", "residual"};
  NOVA_TRY(check_no_overlap(who, out, n, "out", ins, nins, names, 3));
  DaArgs a{x, residual, bias, out, nullptr, rows, first_row, D, 0, T, subsequence, (uint32_t)seed, (uint32_t)(seed >> 32), scale, 0};
  da_launch(a, dtype, false, act == NOVA_DROPOUT_ACT_RELU, false, (hipStream_t)stream);
  return check_launch(who);
}

int nova_bias_dropout_add_bwd(const void* g, const void* out, int dtype, void* gx, float* gbias_parts, long long rows, int D,
                              long long first_row, unsigned long long T, float scale, unsigned long long seed,
                              unsigned long long subsequence, int act, void* stream) {
  const char* who = "bias_dropout_add_bwd";
  NOVA_REQUIRE(g, NOVA_ERR_ARG, "%s: null pointer g", who);
  NOVA_TRY(da_check_head(who, dtype, act));
  NOVA_REQUIRE(!(act == NOVA_DROPOUT_ACT_RELU && !out), NOVA_ERR_ARG, "%s: NOVA_DROPOUT_ACT_RELU needs the saved out (null pointer out)", who);
  NOVA_TRY(da_check_tail(who, rows, D, first_row, T));
  NOVA_REQUIRE(!gbias_parts || first_row % DA_CHUNK == 0, NOVA_ERR_ARG,
               "%s: first_row %lld is not a multiple of %d (NOVA_DROPOUT_CHUNK) while gbias_parts is given", who, first_row, DA_CHUNK);
  NOVA_REQUIRE(gx || gbias_parts, NOVA_ERR_ARG, "%s: no gradient wanted (gx and gbias_parts are both NULL)", who);
  if (rows <= 0) return 0;
  const bool relu = act == NOVA_DROPOUT_ACT_RELU;
  const size_t n = (size_t)rows * D * esize(dtype), np = (size_t)((rows + DA_CHUNK - 1) / DA_CHUNK) * D * 4;
  const void* ins[2] = {g, relu ? out : nullptr};  // out is not read without an activation
  const size_t nins[2] = {n, n};
  const char* names[2] = {"g", "out"};
  const void* outs[2] = {gx, gbias_parts};
  const size_t nouts[2] = {n, np};
  const char* onames[2] = {"gx", "gbias_parts"};
  for (int o = 0; o < 2; ++o) NOVA_TRY(check_no_overlap(who, outs[o], nouts[o], onames[o], ins, nins, names, 2));  // both against the inputs first
  NOVA_REQUIRE(!ranges_overlap(gx, n, gbias_parts, np), NOVA_ERR_ARG, "%s: gx and gbias_parts overlap each other", who);
  DaArgs a{g, relu ? out : nullptr, nullptr, gx, gbias_parts, rows, first_row, D, 0, T, subsequence, (uint32_t)seed, (uint32_t)(seed >> 32), scale, 0};
  da_launch(a, dtype, true, relu, gbias_parts != nullptr, (hipStream_t)stream);
  return check_launch(who);
}

}  // extern "C"
