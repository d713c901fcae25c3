// Fused point embedding, forward and backward: the lift of the per-point inputs x [S, N, C] to the model width through
// W [E, C] (the layout of nn.Linear.weight) and the broadcast additions that follow it, out [S, N, E] written once. The
// reference has it at the head of both point-cloud forwards, diffnext/models/transformers/transformer_pointcloud_nova.py:
//   point_embed = nn.Linear(point_cloud_dim, 768); x = x + self.pos_embed[:, :x.shape[1], :]      :562-565, :712-716
//   x + expanded_cluster_features, x + timestep_emb.unsqueeze(1), x + text_emb                    :753-756, :759-760, :772
//   AutoregressiveDiffusion.forward: the same two broadcasts                                      :294, :297
//   EdgeAligner: spatial_embed = nn.Linear(3, embed_dim); aligned_features + spatial_features     :174, :218-221
//   PointCloudPatchEmbed / PointCloudPosEmbed at patch size 1                                     :315-327, :340-346
// (a K = C GEMM that writes [S, N, E], then one full read-and-write pass per addend; in the backward one read of the
// incoming gradient per consumer). Here the forward writes out once and the backward reads g once for gx, gW and the
// per-cloud row sums. The definition (every rounding, the order of every sum) is in include/nova_hip.h at
// nova_pointset_embed; this file is that text as code.
//
//   embed_fwd_kernel    one workgroup of 256 threads per (cloud, EM_FWD_ROWS = 64 rows): wave w takes the rows w, w + 4, ...;
//                       the channels go in blocks of EM_BLOCK = 256, lane l holding the four channels 256 b + 4 l .. + 3 of
//                       block b: 16 contiguous bytes per lane, 1 KiB per wave-instruction. The block loop is the outer one:
//                       a wave loads its 4 C weights, 4 bias and 4 cond values once per block and keeps them in registers
//                       over its rows; the row's C inputs are wave-uniform.
//   embed_bwd_kernel    one workgroup per (cloud, chunk of EM_CHUNK = 128 rows), the forward's lanes and blocks. Per block a
//                       lane holds 4 C weights and 4 (C + 1) accumulators (gW and the row sum of its four channels), whatever
//                       E is. Per row the gx terms of the block go through wave_sum and are added, block after block, to the
//                       row's slot in LDS; the four waves' accumulators are merged in wave order through LDS and the chunk's
//                       partial goes to the caller's workspace.
//   ordered_sum_kernel  (fused_common.h) one thread per element of gWs [S, E, C] and gcs [S, E]: the chunk partials in ascending
//                       chunk order; and one thread per element of nova_pointset_embed_sum_clouds, the clouds in ascending order.
//   embed_pos_bwd_kernel  one thread per 16 bytes (per element), the clouds in ascending order.
// Where the grid of (rows, clouds) has fewer than FEW_WORKGROUPS workgroups, the forward, and the backward when gx is not
// wanted, put one channel block per workgroup in grid.z: the same lanes, channels and orders, three times the workgroups at
// E = 768.
// No atomics. A cloud's results depend on (x[s], W, the addends' rows of that cloud, g[s], N, C, E) alone.
// W GOES STRAIGHT THROUGH THE CACHE, not through LDS: with the block loop outside the row loop every wave reads each of its
// weights exactly once per workgroup, into registers, so LDS would add a round trip and a barrier and save no load; the
// table (9 KiB at E = 768, C = 3) stays in L2 for the other workgroups.
// VEC: a lane's four channels move as one 16-byte access where the rows start on 16 bytes (E % 4 == 0 and 16-byte-aligned
// out, pos, base or g), as two 8-byte ones where they start on 8, otherwise as four 4-byte ones. The lane keeps the same
// channels, so the values are the same. Loads of channels past E - 1 are made at channel 0 and not used (no branch around a
// load); stores there are not made.
#include "fused_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int EM_MAX_C = NOVA_EMBED_MAX_IN;  // include/nova_hip.h
constexpr int EM_MAX_E = NOVA_EMBED_MAX_DIM;
constexpr int EM_MAX_N = NOVA_EMBED_MAX_POINTS;
constexpr int EM_CHUNK = NOVA_EMBED_CHUNK;  // rows per workgroup of the backward, the unit of the workspace
constexpr int EM_T = 256;                   // threads per workgroup
constexpr int EM_WAVES = EM_T / 64;
constexpr int EM_BLOCK = 256;               // channels per block: four per lane
constexpr int EM_FWD_ROWS = 64;             // rows per workgroup of the forward (no part of the definition)
constexpr int EM_AHEAD = 8;                 // rows of g a wave of the backward has in flight (no part of the definition)
static_assert(EM_CHUNK == 128 && EM_CHUNK % EM_WAVES == 0 && EM_BLOCK == 4 * 64, "the chunk and block shapes are part of the definition");

// the lane's four channels e .. e + 3 of the row at p; a channel past E - 1 is read at channel 0 and must not be used
template <int VEC> __device__ __forceinline__ void embed_load4(const float* __restrict__ p, int e, int E, float (&v)[4]) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + (e < E ? e : 0));
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else if (VEC == 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float2 t = *reinterpret_cast<const float2*>(p + (e + 2 * h < E ? e + 2 * h : 0));
      v[2 * h] = t.x, v[2 * h + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p[e + j < E ? e + j : 0];
  }
}

template <int VEC> __device__ __forceinline__ void embed_store4(float* __restrict__ p, int e, int E, const float (&v)[4]) {
  if (VEC == 4) {
    if (e < E) *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  } else if (VEC == 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (e + 2 * h < E) *reinterpret_cast<float2*>(p + e + 2 * h) = make_float2(v[2 * h], v[2 * h + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e + j < E) p[e + j] = v[j];
  }
}

// W[e + j, c] for the lane's four channels (rows past E - 1: row E - 1, not used)
template <int C> __device__ __forceinline__ void embed_load_w(const float* __restrict__ W, int e, int E, float (&w)[4][C]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float* wr = W + (size_t)(e + j < E ? e + j : E - 1) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) w[j][c] = wr[c];
  }
}

// the rows r = wave, wave + 4, ... < rows of one workgroup for the channel block at e
template <int C, int VEC, bool HAS_POS, bool HAS_BASE>
__device__ __forceinline__ void embed_fwd_rows(const float* __restrict__ xs, const float (&w)[4][C], const float (&bv)[4], bool has_bias,
                                               const float* __restrict__ posr, const float (&cv)[4], bool has_cond,
                                               const float* __restrict__ baser, float* __restrict__ outr, int wave, int rows, int e, int E) {
#pragma unroll 4
  for (int r = wave; r < rows; r += EM_WAVES) {
    float xv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] = xs[r * C + c];
    float pv[4], sv[4], v[4];
    if (HAS_POS) embed_load4<VEC>(posr + (size_t)r * E, e, E, pv);
    if (HAS_BASE) embed_load4<VEC>(baser + (size_t)r * E, e, E, sv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = __fmul_rn(xv[0], w[j][0]);
#pragma unroll
      for (int c = 1; c < C; ++c) a = __builtin_fmaf(xv[c], w[j][c], a);
      a = has_bias ? a + bv[j] : a;  // an addend that is not there is no addition (a + 0 would turn -0 into +0)
      if (HAS_POS) a = a + pv[j];
      a = has_cond ? a + cv[j] : a;
      if (HAS_BASE) a = a + sv[j];
      v[j] = a;
    }
    embed_store4<VEC>(outr + (size_t)r * E, e, E, v);
  }
}

template <int C, int VEC>
__global__ __launch_bounds__(EM_T) void embed_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                         const float* __restrict__ pos, const float* __restrict__ cond,
                                                         const float* __restrict__ base, float* __restrict__ out, int N, int E) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t s = blockIdx.y;
  const int i0 = blockIdx.x * EM_FWD_ROWS;
  const int rows = min(EM_FWD_ROWS, N - i0);  // a row past the cloud is neither read nor written
  const size_t row0 = s * (size_t)N + i0;
  const float* xs = x + row0 * C;
  float* outr = out + row0 * (size_t)E;
  const float* baser = base ? base + row0 * (size_t)E : nullptr;
  const float* posr = pos ? pos + (size_t)i0 * E : nullptr;
  for (int e0 = blockIdx.z * EM_BLOCK; e0 < E; e0 += gridDim.z * EM_BLOCK) {  // every block, or one block per grid.z
    const int e = e0 + 4 * lane;
    float w[4][C], bv[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
    embed_load_w<C>(W, e, E, w);
    if (bias) embed_load4<1>(bias, e, E, bv);
    if (cond) embed_load4<1>(cond + s * (size_t)E, e, E, cv);
    if (pos && base) embed_fwd_rows<C, VEC, true, true>(xs, w, bv, bias != nullptr, posr, cv, cond != nullptr, baser, outr, wave, rows, e, E);
    else if (pos) embed_fwd_rows<C, VEC, true, false>(xs, w, bv, bias != nullptr, posr, cv, cond != nullptr, baser, outr, wave, rows, e, E);
    else if (base) embed_fwd_rows<C, VEC, false, true>(xs, w, bv, bias != nullptr, posr, cv, cond != nullptr, baser, outr, wave, rows, e, E);
    else embed_fwd_rows<C, VEC, false, false>(xs, w, bv, bias != nullptr, posr, cv, cond != nullptr, baser, outr, wave, rows, e, E);
  }
}

template <int C, int VEC>
__global__ __launch_bounds__(EM_T) void embed_bwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ g,
                                                         float* __restrict__ gx, float* __restrict__ ws, int N, int E, int want_gw, int want_gc) {
  __shared__ float red[EM_WAVES][EM_BLOCK * (C + 1)];  // per wave: [256][C] of gW, then [256] row sums; 36 KiB at C = 8
  __shared__ float gxs[EM_CHUNK][C];                   // the rows' gx, added to block after block by the row's own wave
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t s = blockIdx.y;
  const int i0 = blockIdx.x * EM_CHUNK;
  const int rows = min(EM_CHUNK, N - i0);  // a row past the cloud adds nothing
  const size_t row0 = s * (size_t)N + i0;
  const float* xs = x + row0 * C;
  const float* gr = g + row0 * (size_t)E;
  const bool want_gx = gx != nullptr;
  float* part = ws ? ws + (s * gridDim.x + blockIdx.x) * (size_t)E * (C + 1) : nullptr;  // [E, C] of gW, then [E] row sums
  if (want_gx && lane < C)
    for (int r = wave; r < rows; r += EM_WAVES) gxs[r][lane] = 0.f;
  for (int e0 = blockIdx.z * EM_BLOCK; e0 < E; e0 += gridDim.z * EM_BLOCK) {  // every block, or one block per grid.z
    const int e = e0 + 4 * lane;
    float w[4][C], aw[4][C], ac[4] = {0.f, 0.f, 0.f, 0.f};
    embed_load_w<C>(W, e, E, w);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) aw[j][c] = 0.f;
    // EM_AHEAD of the wave's rows at a time: their loads are issued together (a row past the last is read at the group's
    // first row and not used), then the rows are taken in order
    for (int rb = wave; rb < rows; rb += EM_AHEAD * EM_WAVES) {
      float gq[EM_AHEAD][4];
#pragma unroll
      for (int u = 0; u < EM_AHEAD; ++u) {
        const int r = rb + u * EM_WAVES;
        embed_load4<VEC>(gr + (size_t)(r < rows ? r : rb) * E, e, E, gq[u]);
      }
#pragma unroll
      for (int u = 0; u < EM_AHEAD; ++u) {
        const int r = rb + u * EM_WAVES;
        if (r >= rows) break;
        const float(&gv)[4] = gq[u];
        float xv[C];
#pragma unroll
        for (int c = 0; c < C; ++c) xv[c] = xs[r * C + c];
        if (want_gx) {
          float mine = 0.f;  // lane c < C keeps the block's term of gx[row, c]
#pragma unroll
          for (int c = 0; c < C; ++c) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) a = e + j < E ? __builtin_fmaf(gv[j], w[j][c], a) : a;  // a channel past E - 1 is skipped
            const float t = wave_sum(a);
            mine = lane == c ? t : mine;
          }
          if (lane < C) gxs[r][lane] = gxs[r][lane] + mine;
        }
        if (want_gw) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) aw[j][c] = __builtin_fmaf(gv[j], xv[c], aw[j][c]);
        }
        if (want_gc) {
#pragma unroll
          for (int j = 0; j < 4; ++j) ac[j] = ac[j] + gv[j];
        }
      }
    }
    if (want_gw || want_gc) {  // the accumulators of channels past E - 1 hold channel 0's terms and are not written out
      if (want_gw) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int c = 0; c < C; ++c) red[wave][(4 * lane + j) * C + c] = aw[j][c];
      }
      if (want_gc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave][EM_BLOCK * C + 4 * lane + j] = ac[j];
      }
      __syncthreads();
      const int lo = want_gw ? 0 : EM_BLOCK * C, hi = want_gc ? EM_BLOCK * (C + 1) : EM_BLOCK * C;
      for (int idx = lo + threadIdx.x; idx < hi; idx += EM_T) {
        float total = red[0][idx];
#pragma unroll
        for (int wv = 1; wv < EM_WAVES; ++wv) total = total + red[wv][idx];
        if (idx < EM_BLOCK * C) {
          if (e0 + idx / C < E) part[(size_t)e0 * C + idx] = total;
        } else {
          const int ee = e0 + idx - EM_BLOCK * C;
          if (ee < E) part[(size_t)E * C + ee] = total;
        }
      }
      __syncthreads();  // red is written again in the next block
    }
  }
  if (want_gx && lane < C)
    for (int r = wave; r < rows; r += EM_WAVES) gx[(row0 + r) * C + lane] = gxs[r][lane];
}

// thread t takes the VEC elements from VEC t on of [N, E] (n = N E, n % VEC == 0)
template <int VEC>
__global__ __launch_bounds__(EM_T) void embed_pos_bwd_kernel(const float* __restrict__ g, float* __restrict__ gpos, int S, size_t n, int accumulate) {
  const size_t at = ((size_t)blockIdx.x * EM_T + threadIdx.x) * VEC;
  if (at >= n) return;
  if (VEC == 4) {
    float4 total = accumulate ? *reinterpret_cast<const float4*>(gpos + at) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const float4 t = *reinterpret_cast<const float4*>(g + (size_t)s * n + at);
      total.x = total.x + t.x, total.y = total.y + t.y, total.z = total.z + t.z, total.w = total.w + t.w;
    }
    *reinterpret_cast<float4*>(gpos + at) = total;
  } else {
    float total = accumulate ? gpos[at] : 0.f;
    for (int s = 0; s < S; ++s) total = total + g[(size_t)s * n + at];
    gpos[at] = total;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// the checks the entries share, in the order include/nova_hip.h states: C, E, N, S
static int em_check(const char* who, int S, int N, int C, int E) {
  NOVA_REQUIRE(C >= 1 && C <= EM_MAX_C, NOVA_ERR_SHAPE, "%s: C %d outside 1 .. %d (NOVA_EMBED_MAX_IN)", who, C, EM_MAX_C);
  NOVA_REQUIRE(E >= 1 && E <= EM_MAX_E, NOVA_ERR_SHAPE, "%s: E %d outside 1 .. %d (NOVA_EMBED_MAX_DIM)", who, E, EM_MAX_E);
  NOVA_REQUIRE(N >= 1 && N <= EM_MAX_N, NOVA_ERR_SHAPE, "%s: N %d outside 1 .. %d (NOVA_EMBED_MAX_POINTS)", who, N, EM_MAX_N);
  NOVA_REQUIRE(S <= 65535, NOVA_ERR_SHAPE, "%s: %d clouds exceed one launch (65535)", who, S);
  return 0;
}

// 4, 2 or 1 floats per access: what E and the row pointers (NULL: no constraint) allow
static int em_vec(int E, const void* a, const void* b = nullptr, const void* c = nullptr) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | ((uintptr_t)E * 4);
  return bits % 16 == 0 ? 4 : bits % 8 == 0 ? 2 : 1;
}

template <typename F> static void em_dispatch_vec(int vec, F&& f) {
  if (vec == 4) f(std::integral_constant<int, 4>{});
  else if (vec == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 1>{});
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_embed(const float* x, const float* W, const float* bias, const float* pos, const float* cond, const float* base,
                        float* out, int S, int N, int C, int E, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_embed";
  NOVA_TRY(em_check(who, S, N, C, E));
  if (S <= 0) return 0;
  const size_t no = (size_t)S * N * E * 4;
  const void* ins[6] = {x, W, bias, pos, cond, base};
  const size_t nins[6] = {(size_t)S * N * C * 4, (size_t)E * C * 4, (size_t)E * 4, (size_t)N * E * 4, (size_t)S * E * 4, no};
  const char* names[6] = {"x", "W", "bias", "pos", "cond", "base"};
  for (int b = 0; b < 2; ++b) NOVA_REQUIRE(ins[b], NOVA_ERR_ARG, "%s: null pointer %s", who, names[b]);  // every addend may be NULL
  NOVA_REQUIRE(out, NOVA_ERR_ARG, "%s: null pointer out", who);
  NOVA_TRY(check_no_overlap(who, out, no, "out", ins, nins, names, 6));
  const int groups = (N + EM_FWD_ROWS - 1) / EM_FWD_ROWS;
  const dim3 grid(groups, S, few_workgroups_split(groups * S, E, EM_BLOCK)), block(EM_T);
  dispatch_count8(C, [&](auto c) {
    em_dispatch_vec(em_vec(E, out, pos, base), [&](auto v) {
      hipLaunchKernelGGL((embed_fwd_kernel<decltype(c)::value, decltype(v)::value>), grid, block, 0, st, x, W, bias, pos, cond, base, out, N, E);
    });
  });
  return check_launch(who);
}

int nova_pointset_embed_bwd(const float* x, const float* W, const float* g, float* gx, float* gWs, float* gcs, float* ws, int S, int N, int C,
                            int E, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_embed_bwd";
  NOVA_TRY(em_check(who, S, N, C, E));
  if (S <= 0) return 0;
  const int chunks = (N + EM_CHUNK - 1) / EM_CHUNK;
  const void* ins[3] = {x, W, g};
  const size_t nins[3] = {(size_t)S * N * C * 4, (size_t)E * C * 4, (size_t)S * N * E * 4};
  const char* names[3] = {"x", "W", "g"};
  for (int b = 0; b < 3; ++b) NOVA_REQUIRE(ins[b], NOVA_ERR_ARG, "%s: null pointer %s", who, names[b]);
  NOVA_REQUIRE(gx || gWs || gcs, NOVA_ERR_ARG, "%s: no gradient wanted (gx, gWs and gcs are all NULL)", who);
  NOVA_REQUIRE(ws || !(gWs || gcs), NOVA_ERR_ARG, "%s: gWs and gcs need the workspace ws", who);
  const void* outs[4] = {gx, gWs, gcs, gWs || gcs ? ws : nullptr};
  const size_t nouts[4] = {nins[0], (size_t)S * E * C * 4, (size_t)S * E * 4, (size_t)S * chunks * E * (C + 1) * 4};
  const char* onames[4] = {"gx", "gWs", "gcs", "ws"};
  NOVA_TRY(check_no_overlap(who, outs, nouts, onames, 4, ins, nins, names, 3));
  const dim3 grid(chunks, S, gx ? 1 : few_workgroups_split(chunks * S, E, EM_BLOCK)), block(EM_T);  // gx sums over the blocks: one workgroup takes them all
  float* part = gWs || gcs ? ws : nullptr;
  dispatch_count8(C, [&](auto c) {
    em_dispatch_vec(em_vec(E, g), [&](auto v) {
      hipLaunchKernelGGL((embed_bwd_kernel<decltype(c)::value, decltype(v)::value>), grid, block, 0, st, x, W, g, gx, part, N, E, gWs ? 1 : 0, gcs ? 1 : 0);
    });
  });
  if (part) ordered_sum(st, part, gWs, gcs, S, chunks, E * (C + 1), E * C);
  return check_launch(who);
}

int nova_pointset_embed_sum_clouds(const float* per_cloud, float* out, int S, int n, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_embed_sum_clouds";
  NOVA_REQUIRE(n >= 1 && n <= EM_MAX_E * EM_MAX_C, NOVA_ERR_SHAPE, "%s: n %d outside 1 .. %d (NOVA_EMBED_MAX_DIM * NOVA_EMBED_MAX_IN)", who, n,
               EM_MAX_E * EM_MAX_C);
  if (S <= 0) return 0;
  NOVA_REQUIRE(per_cloud, NOVA_ERR_ARG, "%s: null pointer per_cloud", who);
  NOVA_REQUIRE(out, NOVA_ERR_ARG, "%s: null pointer out", who);
  NOVA_REQUIRE(!ranges_overlap(out, (size_t)n * 4, per_cloud, (size_t)S * n * 4), NOVA_ERR_ARG, "%s: out overlaps the input per_cloud", who);
  ordered_sum(st, per_cloud, out, nullptr, 1, S, n, n);
  return check_launch(who);
}

int nova_pointset_embed_pos_bwd(const float* g, float* gpos, int S, int N, int E, int accumulate, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_embed_pos_bwd";
  NOVA_TRY(em_check(who, S, N, 1, E));
  if (S <= 0) return 0;
  NOVA_REQUIRE(g, NOVA_ERR_ARG, "%s: null pointer g", who);
  NOVA_REQUIRE(gpos, NOVA_ERR_ARG, "%s: null pointer gpos", who);
  const size_t n = (size_t)N * E;
  NOVA_REQUIRE(!ranges_overlap(gpos, n * 4, g, (size_t)S * n * 4), NOVA_ERR_ARG, "%s: gpos overlaps the input g", who);
  const bool wide = n % 4 == 0 && ((uintptr_t)g | (uintptr_t)gpos) % 16 == 0;
  const size_t threads = wide ? n / 4 : n;
  const dim3 grid((unsigned)((threads + EM_T - 1) / EM_T)), block(EM_T);
  if (wide) hipLaunchKernelGGL(embed_pos_bwd_kernel<4>, grid, block, 0, st, g, gpos, S, n, accumulate ? 1 : 0);
  else hipLaunchKernelGGL(embed_pos_bwd_kernel<1>, grid, block, 0, st, g, gpos, S, n, accumulate ? 1 : 0);
  return check_launch(who);
}

}  // extern "C"
