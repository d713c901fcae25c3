// Fused point head, forward and backward: the projection of the transformer's rows x [S, N, E] (float32, bf16 or f16) to
// the per-point outputs through W [C, E] (the layout of nn.Linear.weight), out [S, N, C] float32. The reference ends both
// point-cloud models with it, diffnext/models/transformers/transformer_pointcloud_nova.py:
//   self.output_proj = nn.Linear(embed_dim, 3); x = self.output_proj(x); x.view(B, -1, 3)         :444, :512-515, :611, :778-781
//   train_newloss.py: GradientGuard(max_grad_norm=15.0), torch.clamp of the incoming gradient     :34-43, :681-684, :782
// (an N = 3 GEMM; in the backward three more degenerate GEMMs and one pass for the clamp). It is point_embed.hip with the
// roles swapped: here the forward is the wave reduction over the channels and the backward's gx the store stream. The
// definition (every rounding, the order of every sum) is in include/nova_hip.h at nova_pointset_head; this file is that
// text as code.
//
//   head_fwd_kernel    one workgroup of 256 threads per (cloud, 64 or 16 rows): wave w takes the rows w, w + 4, ..., four of
//                      them at a time (their loads are issued together). The channels go in blocks of HD_BLOCK = 512, lane l
//                      holding the eight channels 512 b + 8 l .. + 7 of block b: 16 contiguous bytes per lane for the 16-bit
//                      types, two such accesses for float32. Each lane keeps C accumulators per row over all of its channels;
//                      the row's C sums go through wave_sum and lane c writes out[row, c]. For E <= 1024 (two blocks) the
//                      lane's 16 C weights are loaded once per wave and stay in registers over its rows; above that they are
//                      read again from the cache per block and group of four rows (the same lanes, channels and order).
//   head_bwd_kernel    one workgroup per (cloud, chunk of HD_CHUNK = 128 rows), the forward's lanes and blocks, the block loop
//                      outside the row loop: per block a lane holds 8 C weights and 8 C accumulators of gWs, whatever E is. The
//                      row's C gradients are wave-uniform; gx is 16 bytes per lane and store. The four waves' accumulators are
//                      merged in wave order through LDS (64 KiB at C = 8) and the chunk's partial goes to the workspace.
//   ordered_sum_kernel (fused_common.h) one thread per element of gWs [S, C, E] and gbs [S, C]: the chunk partials in ascending
//                      chunk order. This file defines no summing kernel of its own.
// Where the grid of (rows, clouds) has fewer than FEW_WORKGROUPS workgroups, the forward takes 16 rows per workgroup
// instead of 64 and the backward puts one channel block per workgroup in grid.z: the same lanes, channels and orders.
// No atomics. A cloud's results depend on (x[s], W, bias, g[s], clamp, N, C, E) alone.
// VEC: a lane's eight channels move in accesses of 16 bytes where the rows start on 16 bytes (E sizeof(T) % 16 == 0 and
// 16-byte-aligned x and gx), of 8 or 4 bytes where they start on those, and for the 16-bit types of 2 bytes otherwise.
// The lane keeps the same channels, so the values are the same. Loads of channels past E - 1 are made at channel 0 and not
// used (no branch around a load); stores there are not made. The 16-byte kernels are compiled for that width; the others take
// the width as a wave-uniform argument: one switch in front of a group's loads.
#include "fused_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int HD_MAX_C = NOVA_HEAD_MAX_OUT;  // include/nova_hip.h
constexpr int HD_MAX_E = NOVA_HEAD_MAX_DIM;
constexpr int HD_MAX_N = NOVA_HEAD_MAX_POINTS;
constexpr int HD_CHUNK = NOVA_HEAD_CHUNK;  // rows per workgroup of the backward, the unit of the workspace
constexpr int HD_T = 256;                  // threads per workgroup
constexpr int HD_WAVES = HD_T / 64;
constexpr int HD_LANE = 8;                 // channels per lane and block: 16 bytes of a 16-bit type
constexpr int HD_BLOCK = 512;              // channels per block
constexpr int HD_RESIDENT = 2;             // blocks whose weights a wave of the forward keeps in registers (no part of the definition)
constexpr int HD_FWD_ROWS = 64;            // rows per workgroup of the forward on a large grid, HD_FWD_ROWS_FEW on a small one (likewise)
constexpr int HD_FWD_ROWS_FEW = 16;
constexpr int HD_AHEAD = 4;                // rows of x a wave has in flight (likewise)
static_assert(HD_CHUNK == 128 && HD_CHUNK % HD_WAVES == 0 && HD_BLOCK == HD_LANE * 64, "the chunk and block shapes are part of the definition");
static_assert(HD_FWD_ROWS % (HD_AHEAD * HD_WAVES) == 0 && HD_FWD_ROWS_FEW % (HD_AHEAD * HD_WAVES) == 0, "a workgroup's rows are whole groups");

constexpr int hd_dwords(int elem_bytes) { return HD_LANE * elem_bytes / 4; }  // a lane's eight channels as stored: 8 dwords, or 4

// the lane's eight channels e .. e + 7 of the row at p, as stored, in accesses of BYTES bytes; a channel past E - 1 is read at
// channel 0 and must not be used
template <typename T, int BYTES> __device__ __forceinline__ void head_load8(const T* __restrict__ p, int e, int E, uint32_t (&d)[hd_dwords(sizeof(T))]) {
  constexpr int VEC = BYTES / (int)sizeof(T);
#pragma unroll
  for (int h = 0; h < HD_LANE / VEC; ++h) {
    const T* q = p + (e + VEC * h < E ? e + VEC * h : 0);
    if constexpr (BYTES == 16) {
      const u4v t = *reinterpret_cast<const u4v*>(q);
      d[4 * h] = t[0], d[4 * h + 1] = t[1], d[4 * h + 2] = t[2], d[4 * h + 3] = t[3];
    } else if constexpr (BYTES == 8) {
      const u2v t = *reinterpret_cast<const u2v*>(q);
      d[2 * h] = t[0], d[2 * h + 1] = t[1];
    } else if constexpr (BYTES == 4) {
      d[h] = *reinterpret_cast<const uint32_t*>(q);
    } else {
      const uint32_t t = *reinterpret_cast<const uint16_t*>(q);
      d[h / 2] = h % 2 ? d[h / 2] | (t << 16) : t;
    }
  }
}

template <typename T, int BYTES> __device__ __forceinline__ void head_store8(T* __restrict__ p, int e, int E, const uint32_t (&d)[hd_dwords(sizeof(T))]) {
  constexpr int VEC = BYTES / (int)sizeof(T);
#pragma unroll
  for (int h = 0; h < HD_LANE / VEC; ++h) {
    if (e + VEC * h >= E) continue;
    T* q = p + e + VEC * h;
    if constexpr (BYTES == 16) *reinterpret_cast<u4v*>(q) = u4v{d[4 * h], d[4 * h + 1], d[4 * h + 2], d[4 * h + 3]};
    else if constexpr (BYTES == 8) *reinterpret_cast<u2v*>(q) = u2v{d[2 * h], d[2 * h + 1]};
    else if constexpr (BYTES == 4) *reinterpret_cast<uint32_t*>(q) = d[h];
    else *reinterpret_cast<uint16_t*>(q) = (uint16_t)(d[h / 2] >> (16 * (h % 2)));
  }
}

// channel j of the eight as float32: exact
template <typename T> __device__ __forceinline__ float head_elem(const uint32_t (&d)[hd_dwords(sizeof(T))], int j) {
  if constexpr (sizeof(T) == 4) return __uint_as_float(d[j]);
  else return to_f<T>(__builtin_bit_cast(T, (uint16_t)(d[j / 2] >> (16 * (j % 2)))));
}

// eight float32 values as T, each rounded once to nearest even (float32: as they are)
template <typename T> __device__ __forceinline__ void head_pack8(const float (&v)[HD_LANE], uint32_t (&d)[hd_dwords(sizeof(T))]) {
#pragma unroll
  for (int k = 0; k < hd_dwords(sizeof(T)); ++k) {
    if constexpr (sizeof(T) == 4) d[k] = __float_as_uint(v[k]);
    else d[k] = Half16<T>::pack(v[2 * k], v[2 * k + 1]);
  }
}

// f(integral_constant<int, BYTES>) for the bytes per access. WIDE: 16, known when the kernel is compiled (the kernels of
// the narrow accesses hold many more values in flight, and a kernel's registers are those of its widest path); otherwise the
// wave-uniform `bytes`: 8 down to sizeof(T)
template <typename T, bool WIDE, typename F> __device__ __forceinline__ void head_with_bytes(int bytes, F&& f) {
  if constexpr (WIDE) f(std::integral_constant<int, 16>{});
  else if (bytes == 8) f(std::integral_constant<int, 8>{});
  else if (sizeof(T) == 4 || bytes == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, sizeof(T) == 4 ? 4 : 2>{});
}

// HD_AHEAD of a wave's rows rb, rb + 4, ... at a time: their loads are issued together (a row past the last is read at
// the group's first row and not used)
template <typename T, bool WIDE> __device__ __forceinline__ void head_load_rows(const T* __restrict__ xr, int rb, int rows, int e, int E, int bytes,
                                                                      uint32_t (&raw)[HD_AHEAD][hd_dwords(sizeof(T))]) {
  head_with_bytes<T, WIDE>(bytes, [&](auto v) {
#pragma unroll
    for (int u = 0; u < HD_AHEAD; ++u) {
      const int r = rb + u * HD_WAVES;
      head_load8<T, decltype(v)::value>(xr + (size_t)(r < rows ? r : rb) * E, e, E, raw[u]);
    }
  });
}

// W[c, e + j] for the lane's eight channels; for a channel past E - 1 (read at channel 0) +0
template <int C> __device__ __forceinline__ void head_load_w(const float* __restrict__ W, int e, int E, float (&w)[HD_LANE][C]) {
  if ((((uintptr_t)W | ((uintptr_t)E * 4)) & 15) == 0) {  // wave-uniform: the rows of W start on 16 bytes, two accesses per row
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 t = *reinterpret_cast<const float4*>(W + (size_t)c * E + (e + 4 * h < E ? e + 4 * h : 0));
        const bool in = e + 4 * h < E;  // E % 4 == 0: all four or none
        w[4 * h][c] = in ? t.x : 0.f, w[4 * h + 1][c] = in ? t.y : 0.f, w[4 * h + 2][c] = in ? t.z : 0.f, w[4 * h + 3][c] = in ? t.w : 0.f;
      }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int j = 0; j < HD_LANE; ++j) {
        const float t = W[(size_t)c * E + (e + j < E ? e + j : 0)];
        w[j][c] = e + j < E ? t : 0.f;
      }
  }
}

// torch.clamp(g, -t, t) for t > 0: exact, and a NaN stays a NaN (both comparisons are false)
__device__ __forceinline__ float head_guard(float g, float t) { return g < -t ? -t : g > t ? t : g; }

// the terms of one channel block: acc[u][c] = fmaf(x[row u, e + j], W[c, e + j], acc[u][c]) in ascending j; FULL: no channel of
// the block lies past E - 1. A channel past E - 1 is skipped by the definition; here its term is fmaf(-0, +0, acc) (head_load_w
// gives +0, and what was read at channel 0 is replaced by -0: it may be a NaN): the product is -0, and a + (-0) is a bit for bit
// for every a, both zeros included (an acc can be -0: a product that underflows from below zero rounds to it).
template <typename T, int C, bool FULL>
__device__ __forceinline__ void head_fwd_terms(const uint32_t (&raw)[HD_AHEAD][hd_dwords(sizeof(T))], const float (&w)[HD_LANE][C], int e, int E,
                                               float (&acc)[HD_AHEAD][C]) {
#pragma unroll
  for (int u = 0; u < HD_AHEAD; ++u)
#pragma unroll
    for (int j = 0; j < HD_LANE; ++j) {
      const float xf = FULL || e + j < E ? head_elem<T>(raw[u], j) : -0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[u][c] = __builtin_fmaf(xf, w[j][c], acc[u][c]);
    }
}

template <typename T, int C, bool RESIDENT, bool WIDE>
__global__ __launch_bounds__(HD_T) void head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                        float* __restrict__ out, int N, int E, int rows_per_wg, int bytes) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t s = blockIdx.y;
  const int i0 = blockIdx.x * rows_per_wg;
  const int rows = min(rows_per_wg, N - i0);  // a row past the cloud is neither read nor written
  const size_t row0 = s * (size_t)N + i0;
  const T* xr = x + row0 * (size_t)E;
  float* outr = out + row0 * C;
  const int nb = (E + HD_BLOCK - 1) / HD_BLOCK;
  float wres[RESIDENT ? HD_RESIDENT : 1][HD_LANE][C];
  if (RESIDENT) {
#pragma unroll
    for (int b = 0; b < HD_RESIDENT; ++b) head_load_w<C>(W, b * HD_BLOCK + HD_LANE * lane, E, wres[b]);
  }
  float bv[C];
#pragma unroll
  for (int c = 0; c < C; ++c) bv[c] = bias ? bias[c] : 0.f;
  for (int rb = wave; rb < rows; rb += HD_AHEAD * HD_WAVES) {
    float acc[HD_AHEAD][C];
#pragma unroll
    for (int u = 0; u < HD_AHEAD; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[u][c] = 0.f;
    auto terms = [&](int b, const uint32_t(&raw)[HD_AHEAD][hd_dwords(sizeof(T))], const float(&w)[HD_LANE][C]) {
      const int e = b * HD_BLOCK + HD_LANE * lane;
      if ((b + 1) * HD_BLOCK <= E) head_fwd_terms<T, C, true>(raw, w, e, E, acc);
      else head_fwd_terms<T, C, false>(raw, w, e, E, acc);
    };
    if constexpr (RESIDENT) {  // the loads of both blocks are issued before the first block's terms
      static_assert(HD_RESIDENT == 2, "two blocks written out");
      uint32_t raw0[HD_AHEAD][hd_dwords(sizeof(T))], raw1[HD_AHEAD][hd_dwords(sizeof(T))];
      head_load_rows<T, WIDE>(xr, rb, rows, HD_LANE * lane, E, bytes, raw0);
      if (nb > 1) head_load_rows<T, WIDE>(xr, rb, rows, HD_BLOCK + HD_LANE * lane, E, bytes, raw1);
      terms(0, raw0, wres[0]);
      if (nb > 1) terms(1, raw1, wres[1]);
    } else {
      for (int b = 0; b < nb; ++b) {
        float w[HD_LANE][C];
        uint32_t raw[HD_AHEAD][hd_dwords(sizeof(T))];
        head_load_w<C>(W, b * HD_BLOCK + HD_LANE * lane, E, w);
        head_load_rows<T, WIDE>(xr, rb, rows, b * HD_BLOCK + HD_LANE * lane, E, bytes, raw);
        terms(b, raw, w);
      }
    }
#pragma unroll
    for (int u = 0; u < HD_AHEAD; ++u) {
      const int r = rb + u * HD_WAVES;
      if (r >= rows) break;
      float mine = 0.f;  // lane c < C keeps out[row, c]
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float t = wave_sum(acc[u][c]);
        t = bias ? t + bv[c] : t;  // a bias that is not there is no addition (a + 0 would turn -0 into +0)
        mine = lane == c ? t : mine;
      }
      if (lane < C) outr[(size_t)r * C + lane] = mine;
    }
  }
}

template <typename T, int C, bool WIDE>
__global__ __launch_bounds__(HD_T) void head_bwd_kernel(const T* __restrict__ x, const float* __restrict__ W, const float* __restrict__ g, float clamp,
                                                        T* __restrict__ gx, float* __restrict__ ws, int N, int E, int want_gw, int want_gb, int bytes) {
  __shared__ float red[HD_WAVES][C * HD_BLOCK];  // per wave: [C][512] of gWs; 64 KiB at C = 8
  __shared__ float redb[HD_WAVES][C];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t s = blockIdx.y;
  const int i0 = blockIdx.x * HD_CHUNK;
  const int rows = min(HD_CHUNK, N - i0);  // a row past the cloud adds nothing
  const size_t row0 = s * (size_t)N + i0;
  const float* gr = g + row0 * C;
  const bool want_gx = gx != nullptr, guarded = clamp > 0.f;
  const int nb = (E + HD_BLOCK - 1) / HD_BLOCK;
  float* part = ws ? ws + (s * gridDim.x + blockIdx.x) * ((size_t)C * E + C) : nullptr;  // [C, E] of gWs, then [C] of gbs
  if (want_gx || want_gw) {
    const T* xr = x + row0 * (size_t)E;  // not dereferenced unless gWs is wanted
    T* gxr = gx + row0 * (size_t)E;
    for (int b = blockIdx.z; b < nb; b += gridDim.z) {  // every block, or one block per grid.z
      const int e = b * HD_BLOCK + HD_LANE * lane;
      float w[HD_LANE][C], aw[HD_LANE][C];
      if (want_gx) head_load_w<C>(W, e, E, w);
#pragma unroll
      for (int j = 0; j < HD_LANE; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) aw[j][c] = 0.f;
      for (int rb = wave; rb < rows; rb += HD_AHEAD * HD_WAVES) {
        uint32_t raw[HD_AHEAD][hd_dwords(sizeof(T))];
        if (want_gw) head_load_rows<T, WIDE>(xr, rb, rows, e, E, bytes, raw);
#pragma unroll
        for (int u = 0; u < HD_AHEAD; ++u) {
          const int r = rb + u * HD_WAVES;
          if (r >= rows) break;
          float gv[C];
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float t = gr[r * C + c];
            gv[c] = guarded ? head_guard(t, clamp) : t;
          }
          if (want_gx) {
            float o[HD_LANE];
#pragma unroll
            for (int j = 0; j < HD_LANE; ++j) {
              float a = __fmul_rn(gv[0], w[j][0]);
#pragma unroll
              for (int c = 1; c < C; ++c) a = __builtin_fmaf(gv[c], w[j][c], a);
              o[j] = a;
            }
            uint32_t od[hd_dwords(sizeof(T))];
            head_pack8<T>(o, od);  // one round-to-nearest-even to x's type
            head_with_bytes<T, WIDE>(bytes, [&](auto v) { head_store8<T, decltype(v)::value>(gxr + (size_t)r * E, e, E, od); });
          }
          if (want_gw) {
#pragma unroll
            for (int j = 0; j < HD_LANE; ++j) {
              const float xf = head_elem<T>(raw[u], j);
#pragma unroll
              for (int c = 0; c < C; ++c) aw[j][c] = __builtin_fmaf(gv[c], xf, aw[j][c]);
            }
          }
        }
      }
      if (want_gw) {  // the accumulators of channels past E - 1 hold channel 0's terms and are not written out
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int j = 0; j < HD_LANE; ++j) red[wave][c * HD_BLOCK + HD_LANE * lane + j] = aw[j][c];
        __syncthreads();
        for (int idx = threadIdx.x; idx < C * HD_BLOCK; idx += HD_T) {
          float total = red[0][idx];
#pragma unroll
          for (int wv = 1; wv < HD_WAVES; ++wv) total = total + red[wv][idx];
          const int c = idx / HD_BLOCK, ee = b * HD_BLOCK + idx % HD_BLOCK;
          if (ee < E) part[(size_t)c * E + ee] = total;
        }
        __syncthreads();  // red is written again in the next block
      }
    }
  }
  if (want_gb && blockIdx.z == 0) {  // the row sums of g do not depend on the channel block: the first workgroup of grid.z forms them
    float ab[C];
#pragma unroll
    for (int c = 0; c < C; ++c) ab[c] = 0.f;
    for (int r = wave; r < rows; r += HD_WAVES) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = gr[r * C + c];
        ab[c] = ab[c] + (guarded ? head_guard(t, clamp) : t);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) redb[wave][c] = ab[c];
    }
    __syncthreads();
    if (threadIdx.x < C) {
      float total = redb[0][threadIdx.x];
#pragma unroll
      for (int wv = 1; wv < HD_WAVES; ++wv) total = total + redb[wv][threadIdx.x];
      part[(size_t)C * E + threadIdx.x] = total;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// the checks the two entries share after the null pointers, in the order include/nova_hip.h states: dtype, C, E, N, S
static int hd_check(const char* who, int dtype, int S, int N, int C, int E) {
  NOVA_REQUIRE(!bad_dtype(dtype), NOVA_ERR_ARG, "%s: unknown dtype code %d (NOVA_F32, NOVA_BF16, NOVA_F16)", who, dtype);
  NOVA_REQUIRE(C >= 1 && C <= HD_MAX_C, NOVA_ERR_SHAPE, "%s: C %d outside 1 .. %d (NOVA_HEAD_MAX_OUT)", who, C, HD_MAX_C);
  NOVA_REQUIRE(E >= 1 && E <= HD_MAX_E, NOVA_ERR_SHAPE, "%s: E %d outside 1 .. %d (NOVA_HEAD_MAX_DIM)", who, E, HD_MAX_E);
  NOVA_REQUIRE(N >= 1 && N <= HD_MAX_N, NOVA_ERR_SHAPE, "%s: N %d outside 1 .. %d (NOVA_HEAD_MAX_POINTS)", who, N, HD_MAX_N);
  NOVA_REQUIRE(S <= 65535, NOVA_ERR_SHAPE, "%s: %d clouds exceed one launch (65535)", who, S);
  return 0;
}

// bytes per access: what E and the row pointers (NULL: no constraint) allow, from 16 down to one element
static int hd_bytes(int dtype, int E, const void* a, const void* b = nullptr) {
  const uintptr_t es = esize(dtype), bits = (uintptr_t)a | (uintptr_t)b | ((uintptr_t)E * es);
  for (uintptr_t bytes = 16; bytes > es; bytes /= 2)
    if (bits % bytes == 0) return (int)bytes;
  return (int)es;
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_head(const void* x, int dtype, const float* W, const float* bias, float* out, int S, int N, int C, int E, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_head";
  NOVA_REQUIRE(x, NOVA_ERR_ARG, "%s: null pointer x", who);
  NOVA_REQUIRE(W, NOVA_ERR_ARG, "%s: null pointer W", who);
  NOVA_REQUIRE(out, NOVA_ERR_ARG, "%s: null pointer out", who);  // bias may be NULL
  NOVA_TRY(hd_check(who, dtype, S, N, C, E));
  if (S <= 0) return 0;
  const size_t no = (size_t)S * N * C * 4;
  const void* ins[3] = {x, W, bias};
  const size_t nins[3] = {(size_t)S * N * E * esize(dtype), (size_t)C * E * 4, (size_t)C * 4};
  const char* names[3] = {"x", "W", "bias"};
  NOVA_TRY(check_no_overlap(who, out, no, "out", ins, nins, names, 3));
  // a small grid (a single cloud, say) leaves compute units idle: there a workgroup takes fewer rows. A row's result does
  // not depend on who computes the others.
  const int rows_per_wg = ((N + HD_FWD_ROWS - 1) / HD_FWD_ROWS) * S < FEW_WORKGROUPS ? HD_FWD_ROWS_FEW : HD_FWD_ROWS;
  const dim3 grid((N + rows_per_wg - 1) / rows_per_wg, S), block(HD_T);
  const int bytes = hd_bytes(dtype, E, x);
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    dispatch_count8(C, [&](auto c) {
      dispatch_flag(E <= HD_RESIDENT * HD_BLOCK, [&](auto resident) {
        dispatch_flag(bytes == 16, [&](auto wide) {
          hipLaunchKernelGGL((head_fwd_kernel<T, decltype(c)::value, decltype(resident)::value, decltype(wide)::value>), grid, block, 0, st, (const T*)x, W,
                             bias, out, N, E, rows_per_wg, bytes);
        });
      });
    });
    return 0;
  });
  return check_launch(who);
}

int nova_pointset_head_bwd(const void* x, int dtype, const float* W, const float* g, float clamp, void* gx, float* gWs, float* gbs, float* ws,
                           int S, int N, int C, int E, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_head_bwd";
  NOVA_REQUIRE(x || !gWs, NOVA_ERR_ARG, "%s: null pointer x", who);  // x serves gWs alone
  NOVA_REQUIRE(W, NOVA_ERR_ARG, "%s: null pointer W", who);
  NOVA_REQUIRE(g, NOVA_ERR_ARG, "%s: null pointer g", who);
  NOVA_TRY(hd_check(who, dtype, S, N, C, E));
  if (S <= 0) return 0;
  NOVA_REQUIRE(gx || gWs || gbs, NOVA_ERR_ARG, "%s: no gradient wanted (gx, gWs and gbs are all NULL)", who);
  NOVA_REQUIRE(ws || !(gWs || gbs), NOVA_ERR_ARG, "%s: gWs and gbs need the workspace ws", who);
  const int chunks = (N + HD_CHUNK - 1) / HD_CHUNK;
  const size_t nx = (size_t)S * N * E * esize(dtype);
  const void* ins[3] = {gWs ? x : nullptr, W, g};
  const size_t nins[3] = {nx, (size_t)C * E * 4, (size_t)S * N * C * 4};
  const char* names[3] = {"x", "W", "g"};
  const void* outs[4] = {gx, gWs, gbs, gWs || gbs ? ws : nullptr};
  const size_t nouts[4] = {nx, (size_t)S * C * E * 4, (size_t)S * C * 4, (size_t)S * chunks * ((size_t)C * E + C) * 4};
  const char* onames[4] = {"gx", "gWs", "gbs", "ws"};
  NOVA_TRY(check_no_overlap(who, outs, nouts, onames, 4, ins, nins, names, 3));
  const dim3 grid(chunks, S, gx || gWs ? few_workgroups_split(chunks * S, E, HD_BLOCK) : 1), block(HD_T);
  float* part = gWs || gbs ? ws : nullptr;
  const int bytes = hd_bytes(dtype, E, gWs ? x : nullptr, gx);
  dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    dispatch_count8(C, [&](auto c) {
      dispatch_flag(bytes == 16, [&](auto wide) {
        hipLaunchKernelGGL((head_bwd_kernel<T, decltype(c)::value, decltype(wide)::value>), grid, block, 0, st, (const T*)x, W, g, clamp, (T*)gx, part, N,
                           E, gWs ? 1 : 0, gbs ? 1 : 0, bytes);
      });
    });
    return 0;
  });
  if (part) ordered_sum(st, part, gWs, gbs, S, chunks, C * E + C, C * E);
  return check_launch(who);
}

}  // extern "C"
