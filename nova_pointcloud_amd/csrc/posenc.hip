// Depth-aware 3-D positional encoding, forward and backward: for every point x [S, N, 3] the E-channel encoding
// out [S, N, E] of its three coordinates, each multiplied by a learnable scale and taken through F = E / 6 frequencies as
// (sin, cos) pairs, optionally added onto base [S, N, E]. The reference has it in PointCloudTransformer.forward,
//   DepthAwarePositionalEncoding          diffnext/models/transformers/transformer_pointcloud_nova.py:349-389
//   x = x + depth_pe                      :456-458
// (a zeros([B, N, E]), six strided slice assignments each with its own [B, N, E / 6] division and sine or cosine, a separate
// add: about 30 launches, and six [B, N, E / 6] arguments kept alive for the backward). Here the forward writes out once and
// the backward recomputes every argument, sine and cosine from x, scale and div: nothing of size N E is stored. The
// definition (every rounding, the order of every sum) is in include/nova_hip.h at nova_pointset_posenc; this file is that
// text as code.
//
//   posenc_fwd_kernel       one workgroup of 256 threads per (cloud, chunk of PE_CHUNK = 32 rows): wave w takes the rows
//                           w, w + 4, ... of the chunk; lane l takes the (sin, cos) pairs j = l, l + 64, ... of a row, with
//                           f = j / 3 and c = j % 3, so pair j sits at channels 2 j and 2 j + 1: one argument, one division and
//                           one sincosf per pair, 8 contiguous bytes per lane, 512 per wave-instruction. The table div lives
//                           in LDS, loaded once per workgroup (three neighbouring lanes read one address: a broadcast); the
//                           three scaled coordinates of a row are wave-uniform.
//   posenc_bwd_kernel       the forward's shape; three accumulators per lane (one per coordinate), wave_sum, then lanes 0 .. 2
//                           store gx; the x t products of a wave's rows are accumulated in row order, the four waves merged
//                           in wave order through LDS, the chunk's partial written to the caller's workspace.
//   ordered_sum_kernel      (fused_common.h) one thread per element of gs [S, 3]: the chunk partials in ascending chunk order.
//                           This file defines no summing kernel of its own.
// No atomics. A cloud's results depend on (x[s], scale, div, base[s] or g[s], N, E) alone.
// WIDE: rows start on 8 bytes (E even, 8-byte-aligned out, base, g), so a pair moves as one 8-byte access; otherwise as two
// 4-byte ones. The values are the same.
#include "fused_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int PE_MAX_E = NOVA_POSENC_MAX_DIM;  // include/nova_hip.h
constexpr int PE_MAX_N = NOVA_POSENC_MAX_POINTS;
constexpr int PE_CHUNK = NOVA_POSENC_CHUNK;    // rows per workgroup, the unit of the workspace
constexpr int PE_T = 256;                      // threads per workgroup
constexpr int PE_WAVES = PE_T / 64;
constexpr int PE_MAX_F = PE_MAX_E / 6;
static_assert(PE_CHUNK == 32 && PE_CHUNK % PE_WAVES == 0, "the chunk shape is part of the definition");

// div[0 .. F) into LDS and the three scales into registers; ends with a barrier
__device__ __forceinline__ void posenc_prologue(const float* __restrict__ div, const float* __restrict__ scale, float* dv, int F,
                                                float (&sc)[3]) {
  for (int f = threadIdx.x; f < F; f += PE_T) dv[f] = div[f];
  sc[0] = scale[0];
  sc[1] = scale[1];
  sc[2] = scale[2];
  __syncthreads();
}

// a_cf of the definition for pair j = 3 f + c of a row with scaled coordinates s: one IEEE division
__device__ __forceinline__ float posenc_arg(const float (&s)[3], const float* dv, int j, int& f, int& c) {
  f = j / 3;
  c = j - 3 * f;
  const float sc = c == 0 ? s[0] : c == 1 ? s[1] : s[2];
  return __fdiv_rn(sc, dv[f]);
}

template <bool HAS_BASE, bool WIDE>
__global__ __launch_bounds__(PE_T) void posenc_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ div, const float* __restrict__ base,
                                                          float* __restrict__ out, int N, int E, int F) {
  __shared__ float dv[PE_MAX_F];
  float sc[3];
  posenc_prologue(div, scale, dv, F, sc);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pairs = 3 * F;
  const size_t s = blockIdx.y;
  for (int r = wave; r < PE_CHUNK; r += PE_WAVES) {
    const int i = blockIdx.x * PE_CHUNK + r;
    if (i >= N) break;  // a row past the cloud is neither read nor written
    const size_t row = s * (size_t)N + i;
    const float* xr = x + row * 3;
    const float sx[3] = {__fmul_rn(xr[0], sc[0]), __fmul_rn(xr[1], sc[1]), __fmul_rn(xr[2], sc[2])};
    float* o = out + row * (size_t)E;
    const float* b = HAS_BASE ? base + row * (size_t)E : nullptr;
    for (int j = lane; j < pairs; j += 64) {
      int f, c;
      const float a = posenc_arg(sx, dv, j, f, c);
      float sn, cs;
      sincosf(a, &sn, &cs);
      if (WIDE) {
        if (HAS_BASE) {
          const float2 bb = *reinterpret_cast<const float2*>(b + 2 * j);
          sn = bb.x + sn;
          cs = bb.y + cs;
        }
        *reinterpret_cast<float2*>(o + 2 * j) = make_float2(sn, cs);
      } else {
        if (HAS_BASE) {
          sn = b[2 * j] + sn;
          cs = b[2 * j + 1] + cs;
        }
        o[2 * j] = sn;
        o[2 * j + 1] = cs;
      }
    }
    for (int ch = 2 * pairs + lane; ch < E; ch += 64) o[ch] = HAS_BASE ? b[ch] + 0.f : 0.f;  // the tail channels: +0
  }
}

template <bool WANT_GX, bool WANT_GS, bool WIDE>
__global__ __launch_bounds__(PE_T) void posenc_bwd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ div, const float* __restrict__ g,
                                                          float* __restrict__ gx, float* __restrict__ ws, int N, int E, int F) {
  __shared__ float dv[PE_MAX_F];
  __shared__ float red[WANT_GS ? PE_WAVES * 3 : 1];
  float sc[3];
  posenc_prologue(div, scale, dv, F, sc);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pairs = 3 * F;
  const size_t s = blockIdx.y;
  float gsw[3] = {0.f, 0.f, 0.f};  // this wave's x t sums over its rows, per coordinate (wave-uniform)
  for (int r = wave; r < PE_CHUNK; r += PE_WAVES) {
    const int i = blockIdx.x * PE_CHUNK + r;
    if (i >= N) break;  // a row past the cloud adds nothing
    const size_t row = s * (size_t)N + i;
    const float* xr = x + row * 3;
    const float xv[3] = {xr[0], xr[1], xr[2]};
    const float sx[3] = {__fmul_rn(xv[0], sc[0]), __fmul_rn(xv[1], sc[1]), __fmul_rn(xv[2], sc[2])};
    const float* gr = g + row * (size_t)E;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = lane; j < pairs; j += 64) {
      int f, c;
      const float a = posenc_arg(sx, dv, j, f, c);
      float sn, cs;
      sincosf(a, &sn, &cs);
      float g0, g1;
      if (WIDE) {
        const float2 gg = *reinterpret_cast<const float2*>(gr + 2 * j);
        g0 = gg.x;
        g1 = gg.y;
      } else {
        g0 = gr[2 * j];
        g1 = gr[2 * j + 1];
      }
      const float u = __builtin_fmaf(-g1, sn, __fmul_rn(g0, cs));
      const float term = __fdiv_rn(u, dv[f]);
      acc[0] = acc[0] + (c == 0 ? term : 0.f);  // + 0 leaves the sum as it is: each accumulator sees its own terms alone
      acc[1] = acc[1] + (c == 1 ? term : 0.f);
      acc[2] = acc[2] + (c == 2 ? term : 0.f);
    }
    float t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = wave_sum(acc[c]);
    if (WANT_GX && lane < 3) gx[row * 3 + lane] = __fmul_rn(lane == 0 ? sc[0] : lane == 1 ? sc[1] : sc[2], lane == 0 ? t[0] : lane == 1 ? t[1] : t[2]);
    if (WANT_GS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gsw[c] = __builtin_fmaf(xv[c], t[c], gsw[c]);
    }
  }
  if (WANT_GS) {
    if (lane < 3) red[wave * 3 + lane] = lane == 0 ? gsw[0] : lane == 1 ? gsw[1] : gsw[2];
    __syncthreads();
    if (threadIdx.x < 3) {
      float total = red[threadIdx.x];
#pragma unroll
      for (int w = 1; w < PE_WAVES; ++w) total = total + red[w * 3 + threadIdx.x];
      ws[(s * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = total;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// the checks both entries share, in the order include/nova_hip.h states: E, N, S
static int pe_check(const char* who, int S, int N, int E) {
  NOVA_REQUIRE(E >= 6 && E <= PE_MAX_E, NOVA_ERR_SHAPE, "%s: E %d outside 6 .. %d (NOVA_POSENC_MAX_DIM)", who, E, PE_MAX_E);
  NOVA_REQUIRE(N >= 1 && N <= PE_MAX_N, NOVA_ERR_SHAPE, "%s: N %d outside 1 .. %d (NOVA_POSENC_MAX_POINTS)", who, N, PE_MAX_N);
  NOVA_REQUIRE(S <= 65535, NOVA_ERR_SHAPE, "%s: %d clouds exceed one launch (65535)", who, S);
  return 0;
}

static bool pe_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

template <bool WIDE>
static void pe_bwd_launch(dim3 grid, hipStream_t st, const float* x, const float* scale, const float* div, const float* g, float* gx,
                          float* gs, float* ws, int N, int E, int F) {
  const dim3 block(PE_T);
  if (gx && gs) hipLaunchKernelGGL((posenc_bwd_kernel<true, true, WIDE>), grid, block, 0, st, x, scale, div, g, gx, ws, N, E, F);
  else if (gx) hipLaunchKernelGGL((posenc_bwd_kernel<true, false, WIDE>), grid, block, 0, st, x, scale, div, g, gx, ws, N, E, F);
  else hipLaunchKernelGGL((posenc_bwd_kernel<false, true, WIDE>), grid, block, 0, st, x, scale, div, g, gx, ws, N, E, F);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_posenc(const float* x, const float* scale, const float* div, const float* base, float* out, int S, int N, int E,
                         void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_posenc";
  NOVA_TRY(pe_check(who, S, N, E));
  if (S <= 0) return 0;
  const int F = E / 6;
  const size_t nx = (size_t)S * N * 12, no = (size_t)S * N * E * 4;
  const void* ins[4] = {x, scale, div, base};
  const size_t nins[4] = {nx, 12, (size_t)F * 4, no};
  const char* names[4] = {"x", "scale", "div", "base"};
  for (int b = 0; b < 3; ++b) NOVA_REQUIRE(ins[b], NOVA_ERR_ARG, "%s: null pointer %s", who, names[b]);  // base may be NULL
  NOVA_REQUIRE(out, NOVA_ERR_ARG, "%s: null pointer out", who);
  NOVA_TRY(check_no_overlap(who, out, no, "out", ins, nins, names, 4));
  const dim3 grid((N + PE_CHUNK - 1) / PE_CHUNK, S), block(PE_T);
  const bool wide = E % 2 == 0 && pe_aligned8(out) && pe_aligned8(base);
  if (base && wide) hipLaunchKernelGGL((posenc_fwd_kernel<true, true>), grid, block, 0, st, x, scale, div, base, out, N, E, F);
  else if (base) hipLaunchKernelGGL((posenc_fwd_kernel<true, false>), grid, block, 0, st, x, scale, div, base, out, N, E, F);
  else if (wide) hipLaunchKernelGGL((posenc_fwd_kernel<false, true>), grid, block, 0, st, x, scale, div, base, out, N, E, F);
  else hipLaunchKernelGGL((posenc_fwd_kernel<false, false>), grid, block, 0, st, x, scale, div, base, out, N, E, F);
  return check_launch(who);
}

int nova_pointset_posenc_bwd(const float* x, const float* scale, const float* div, const float* g, float* gx, float* gs, float* ws, int S,
                             int N, int E, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_posenc_bwd";
  NOVA_TRY(pe_check(who, S, N, E));
  if (S <= 0) return 0;
  const int F = E / 6, chunks = (N + PE_CHUNK - 1) / PE_CHUNK;
  const size_t nx = (size_t)S * N * 12, ng = (size_t)S * N * E * 4;
  const void* ins[4] = {x, scale, div, g};
  const size_t nins[4] = {nx, 12, (size_t)F * 4, ng};
  const char* names[4] = {"x", "scale", "div", "g"};
  for (int b = 0; b < 4; ++b) NOVA_REQUIRE(ins[b], NOVA_ERR_ARG, "%s: null pointer %s", who, names[b]);
  NOVA_REQUIRE(gx || gs, NOVA_ERR_ARG, "%s: no gradient wanted (gx and gs are both NULL)", who);
  NOVA_REQUIRE(ws || !gs, NOVA_ERR_ARG, "%s: gs needs the workspace ws", who);
  const void* outs[3] = {gx, gs, gs ? ws : nullptr};
  const size_t nouts[3] = {nx, (size_t)S * 12, (size_t)S * chunks * 12};
  const char* onames[3] = {"gx", "gs", "ws"};
  NOVA_TRY(check_no_overlap(who, outs, nouts, onames, 3, ins, nins, names, 4));
  const dim3 grid(chunks, S);
  if (E % 2 == 0 && pe_aligned8(g)) pe_bwd_launch<true>(grid, st, x, scale, div, g, gx, gs, ws, N, E, F);
  else pe_bwd_launch<false>(grid, st, x, scale, div, g, gx, gs, ws, N, E, F);
  if (gs) ordered_sum(st, ws, gs, nullptr, S, chunks, 3, 3);
  return check_launch(who);
}

}  // extern "C"
