// Soft cluster pooling, forward and backward: for every cloud x [S, N, 3] and K centres c (shared [K, 3] or per cloud
// [S, K, 3]) the K softmax(-distance / temperature)-weighted centroids out [S, K, 3] and the cluster masses mass [S, K]. The
// reference has it on its gradient path in both point-cloud models,
//   PointCloudTransformer.forward          diffnext/models/transformers/transformer_pointcloud_nova.py:465-487
//   NOVAPointCloudTransformer.forward      :724-741
// (torch.cdist to the learnable cluster_centers [8, 3], softmax(-distances), a Python loop over the 8 clusters forming
// (points * w).sum(1) / (w.sum(1) + 1e-8)): about 40 launches, with the [B, N, 8] distances and weights and 8 [B, N, 3]
// products kept alive for the backward. Here nothing of size N K exists in either pass: the backward recomputes every
// weight from x, c and scale. The definition (every rounding, the order of every sum) is in include/nova_hip.h at
// nova_pointset_soft_cluster; this file is that text as code.
//
//   soft_cluster_fwd_kernel    one workgroup of 256 threads per (cloud, chunk of SC_CHUNK = 1024 points): thread t takes the
//                              points t, t + 256, t + 512, t + 768 of the chunk in that order, one at a time; the centres are
//                              broadcast from LDS; the 4 K accumulators (num[3], mass per centre) live in registers, on the
//                              rungs KR = 8 / 16 / 32 centres, and are reduced by wave_sum's fixed pairing and then over the
//                              four waves in wave order. The chunk's partials go to the caller's workspace.
//   soft_cluster_merge_kernel  one thread per (cloud, centre): the chunk partials in ascending chunk order, then the division.
//   soft_cluster_bwd_kernel    the forward's shape; per centre the LDS holds c, out, g, u = 1 / (mass + 1e-8) and gm. gx is
//                              local to the point (no reduction); the 3 K sums of gc take the forward's reduction, chunk
//                              partials to the workspace; gx or gc not wanted: its arithmetic is compiled out.
//   ordered_sum_kernel         (fused_common.h) one thread per element of gc [S, K, 3]: the chunk partials in ascending chunk
//                              order; and one thread per element of [K, 3]: gc[s] in ascending s, for the shared centres' gradient.
// No atomics. A cloud's results depend on (x[s], c, N, K, scale) and, backward, (out[s], mass[s], g[s], gm[s]) alone.
//
// Cost per (point, centre): the distance 6 + 17 (correctly rounded square root), the weight 3 (v_exp_f32 at a quarter rate),
// the product with r 1, four accumulations: about 35 issue slots forward, and 12 bytes of x per point, so the forward is
// bound by instruction issue, not by memory, from K = 2 on.
#include "interp_common.h"
#include "fused_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int SC_MAX_N = NOVA_SOFT_CLUSTER_MAX_POINTS;  // include/nova_hip.h
constexpr int SC_MAX_K = NOVA_SOFT_CLUSTER_MAX_K;
constexpr int SC_T = 256;                               // threads per workgroup
constexpr int SC_WAVES = SC_T / 64;
constexpr int SC_CHUNK = NOVA_SOFT_CLUSTER_CHUNK;       // points per workgroup
constexpr int SC_STEPS = SC_CHUNK / SC_T;               // points per thread, one at a time
constexpr float SC_EPS = 1e-8f;                         // the reference's constant (:480)
constexpr float SC_LN2 = 0.693147180559945309f;
static_assert(SC_CHUNK == 1024 && SC_CHUNK % SC_T == 0, "the chunk shape is part of the definition");
static_assert(SC_MAX_K <= 32, "the rungs end at 32 centres");

// d_k, then a_k = e_k * r of one point against the KR-rung of centres in LDS (cs[k] = (c0, c1, c2, .)); centres past K get
// a = 0 and d = 0 and take no part in the minimum or in L.
template <int KR>
__device__ __forceinline__ void soft_assign(float x0, float x1, float x2, const f4v* cs, int stride, int K, float scale, float (&d)[KR],
                                            float (&a)[KR]) {
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    d[k] = 0.f;
    if (k < K) {
      const f4v c = cs[k * stride];
      d[k] = interp_dist(x0, x1, x2, c[0], c[1], c[2]);
      m = k == 0 ? d[0] : fminf(m, d[k]);
    }
  }
  float L = 0.f;
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    a[k] = 0.f;
    if (k < K) {
      a[k] = interp_weight(m, d[k], scale);
      L = k == 0 ? a[0] : L + a[k];
    }
  }
  const float r = __fdiv_rn(1.0f, L);  // L >= 1: the nearest centre has weight exactly 1
#pragma unroll
  for (int k = 0; k < KR; ++k) a[k] = a[k] * r;
}

// The thread's SC_STEPS points of its chunk, all loaded before the first is used (one memory latency per workgroup instead of
// one per step); a point past the cloud is not read.
__device__ __forceinline__ void chunk_points(const float* __restrict__ xs, int chunk, int N, float (&px)[SC_STEPS][3]) {
#pragma unroll
  for (int step = 0; step < SC_STEPS; ++step) {
    const int i = chunk * SC_CHUNK + step * SC_T + (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < 3; ++j) px[step][j] = i < N ? xs[(size_t)i * 3 + j] : 0.f;
  }
}

// The reduction every sum over a cloud's points takes: acc[q] of the 256 threads by wave_sum's pairing, then the four
// waves in wave order ((w0 + w1) + w2) + w3; thread q < count stores sum q to dst[q].
template <int Q> __device__ __forceinline__ void chunk_reduce(float (&acc)[Q], float* red, float* dst, int count) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    if (q < count) {  // uniform: the rung's unused centres are not reduced
      const float v = wave_sum(acc[q]);
      if ((t & 63) == 0) red[(t >> 6) * Q + q] = v;
    }
  }
  __syncthreads();
  if (t < count) {
    float total = red[t];
#pragma unroll
    for (int w = 1; w < SC_WAVES; ++w) total = total + red[w * Q + t];
    dst[t] = total;
  }
}

template <int KR>
__global__ __launch_bounds__(SC_T) void soft_cluster_fwd_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                                float* __restrict__ ws, int N, int K, size_t cstride, float scale) {
  __shared__ f4v cs[KR];
  __shared__ float red[SC_WAVES * 4 * KR];
  const int t = threadIdx.x;
  const int chunk = blockIdx.x, chunks = gridDim.x;
  const size_t s = blockIdx.y;
  if (t < K) {
    const float* cc = c + s * cstride + (size_t)t * 3;
    cs[t] = f4v{cc[0], cc[1], cc[2], 0.f};
  }
  __syncthreads();
  float acc[4 * KR];  // [k][num0, num1, num2, mass]
#pragma unroll
  for (int q = 0; q < 4 * KR; ++q) acc[q] = 0.f;
  float px[SC_STEPS][3];
  chunk_points(x + s * (size_t)N * 3, chunk, N, px);
  for (int step = 0; step < SC_STEPS; ++step) {
    // the wider rungs re-read the centres from LDS at every step: held in registers across the steps (12 KR of them in the
    // backward) they push the accumulators out to scratch
    if (KR > 8) __asm__ volatile("" ::: "memory");
    const int i = chunk * SC_CHUNK + step * SC_T + t;
    if (i < N) {  // a point past the cloud adds nothing
      const float x0 = px[step][0], x1 = px[step][1], x2 = px[step][2];
      float d[KR], a[KR];
      soft_assign<KR>(x0, x1, x2, cs, 1, K, scale, d, a);
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        if (k < K) {
          acc[4 * k] = __builtin_fmaf(a[k], x0, acc[4 * k]);
          acc[4 * k + 1] = __builtin_fmaf(a[k], x1, acc[4 * k + 1]);
          acc[4 * k + 2] = __builtin_fmaf(a[k], x2, acc[4 * k + 2]);
          acc[4 * k + 3] = acc[4 * k + 3] + a[k];
        }
      }
    }
  }
  chunk_reduce<4 * KR>(acc, red, ws + (s * chunks + chunk) * (size_t)(4 * K), 4 * K);
}

__global__ __launch_bounds__(SC_T) void soft_cluster_merge_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                  float* __restrict__ mass, int S, int K, int chunks) {
  const size_t e = (size_t)blockIdx.x * SC_T + threadIdx.x;  // (s, k)
  if (e >= (size_t)S * K) return;
  const size_t s = e / K;
  const int k = (int)(e % K);
  float n0 = 0.f, n1 = 0.f, n2 = 0.f, ms = 0.f;
  for (int ch = 0; ch < chunks; ++ch) {
    const float* p = ws + ((s * chunks + ch) * (size_t)K + k) * 4;
    n0 = n0 + p[0];
    n1 = n1 + p[1];
    n2 = n2 + p[2];
    ms = ms + p[3];
  }
  const float den = ms + SC_EPS;
  out[e * 3] = __fdiv_rn(n0, den);
  out[e * 3 + 1] = __fdiv_rn(n1, den);
  out[e * 3 + 2] = __fdiv_rn(n2, den);
  mass[e] = ms;
}

// per centre in LDS: (c0, c1, c2, u), (o0, o1, o2, gm), (g0, g1, g2, .)
template <int KR, bool WANT_GX, bool WANT_GC>
__global__ __launch_bounds__(SC_T) void soft_cluster_bwd_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                                const float* __restrict__ out, const float* __restrict__ mass,
                                                                const float* __restrict__ g, const float* __restrict__ gm,
                                                                float* __restrict__ gx, float* __restrict__ ws, int N, int K,
                                                                size_t cstride, float scale) {
  __shared__ f4v cs[3 * KR];
  __shared__ float red[WANT_GC ? SC_WAVES * 3 * KR : 1];
  const int t = threadIdx.x;
  const int chunk = blockIdx.x, chunks = gridDim.x;
  const size_t s = blockIdx.y;
  if (t < K) {
    const float* cc = c + s * cstride + (size_t)t * 3;
    const size_t e = s * K + t;
    cs[3 * t] = f4v{cc[0], cc[1], cc[2], __fdiv_rn(1.0f, mass[e] + SC_EPS)};
    cs[3 * t + 1] = f4v{out[e * 3], out[e * 3 + 1], out[e * 3 + 2], gm ? gm[e] : 0.f};
    cs[3 * t + 2] = f4v{g[e * 3], g[e * 3 + 1], g[e * 3 + 2], 0.f};
  }
  __syncthreads();
  const float kappa = scale * SC_LN2;
  float acc[3 * KR];  // gc partials [k][axis]
#pragma unroll
  for (int q = 0; q < 3 * KR; ++q) acc[q] = 0.f;
  float px[SC_STEPS][3];
  chunk_points(x + s * (size_t)N * 3, chunk, N, px);
  for (int step = 0; step < SC_STEPS; ++step) {
    if (KR > 8) __asm__ volatile("" ::: "memory");  // as in the forward
    const int i = chunk * SC_CHUNK + step * SC_T + t;
    if (i < N) {
      const float x0 = px[step][0], x1 = px[step][1], x2 = px[step][2];
      float d[KR], a[KR], h[KR];
      soft_assign<KR>(x0, x1, x2, cs, 3, K, scale, d, a);
      float hbar = 0.f;
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        h[k] = 0.f;
        if (k < K) {
          const f4v cu = cs[3 * k], o = cs[3 * k + 1], gk = cs[3 * k + 2];
          const float dot = __builtin_fmaf(gk[2], x2 - o[2], __builtin_fmaf(gk[1], x1 - o[1], gk[0] * (x0 - o[0])));
          h[k] = __builtin_fmaf(cu[3], dot, o[3]);
          hbar = k == 0 ? a[0] * h[0] : __builtin_fmaf(a[k], h[k], hbar);
        }
      }
      float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        if (k < K) {
          const f4v cu = cs[3 * k];
          const float e0 = x0 - cu[0], e1 = x1 - cu[1], e2 = x2 - cu[2];
          const float rd = d[k] != 0.f ? __builtin_amdgcn_rcpf(d[k]) : 0.f;  // d is 0 or above 3e-23: never subnormal
          const float f = (kappa * (a[k] * (hbar - h[k]))) * rd;
          if (WANT_GX) {
            const f4v gk = cs[3 * k + 2];
            const float au = a[k] * cu[3];
            r0 = __builtin_fmaf(f, e0, __builtin_fmaf(au, gk[0], r0));
            r1 = __builtin_fmaf(f, e1, __builtin_fmaf(au, gk[1], r1));
            r2 = __builtin_fmaf(f, e2, __builtin_fmaf(au, gk[2], r2));
          }
          if (WANT_GC) {
            acc[3 * k] = __builtin_fmaf(-f, e0, acc[3 * k]);
            acc[3 * k + 1] = __builtin_fmaf(-f, e1, acc[3 * k + 1]);
            acc[3 * k + 2] = __builtin_fmaf(-f, e2, acc[3 * k + 2]);
          }
        }
      }
      if (WANT_GX) {
        float* o = gx + (s * (size_t)N + i) * 3;
        o[0] = r0;
        o[1] = r1;
        o[2] = r2;
      }
    }
  }
  if (WANT_GC) chunk_reduce<3 * KR>(acc, red, ws + (s * chunks + chunk) * (size_t)(3 * K), 3 * K);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// the checks both entries share, in the order include/nova_hip.h states: N, K, S (shape), then scale (argument)
static int sc_check(const char* who, int S, int N, int K, float scale) {
  if (N < 1 || N > SC_MAX_N) return set_error(NOVA_ERR_SHAPE, "%s: N %d outside 1 .. %d (NOVA_SOFT_CLUSTER_MAX_POINTS)", who, N, SC_MAX_N);
  if (K < 1 || K > SC_MAX_K) return set_error(NOVA_ERR_SHAPE, "%s: K %d outside 1 .. %d (NOVA_SOFT_CLUSTER_MAX_K)", who, K, SC_MAX_K);
  if (S > 65535) return set_error(NOVA_ERR_SHAPE, "%s: %d clouds exceed one launch (65535)", who, S);
  return check_scale(who, scale);
}

template <int KR>
static void sc_bwd_launch(dim3 grid, hipStream_t st, const float* x, const float* c, const float* out, const float* mass, const float* g,
                          const float* gm, float* gx, float* gc, float* ws, int N, int K, size_t cstride, float scale) {
  const dim3 block(SC_T);
  if (gx && gc)
    hipLaunchKernelGGL((soft_cluster_bwd_kernel<KR, true, true>), grid, block, 0, st, x, c, out, mass, g, gm, gx, ws, N, K, cstride, scale);
  else if (gx)
    hipLaunchKernelGGL((soft_cluster_bwd_kernel<KR, true, false>), grid, block, 0, st, x, c, out, mass, g, gm, gx, ws, N, K, cstride, scale);
  else
    hipLaunchKernelGGL((soft_cluster_bwd_kernel<KR, false, true>), grid, block, 0, st, x, c, out, mass, g, gm, gx, ws, N, K, cstride, scale);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_soft_cluster(const float* x, const float* c, float* out, float* mass, float* ws, int S, int N, int K, int shared_centers,
                               float scale, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_soft_cluster";
  if (const int rc = sc_check(who, S, N, K, scale)) return rc;
  if (S <= 0) return 0;
  if (!x || !c || !out || !mass || !ws) return set_error(NOVA_ERR_ARG, "%s: null pointer", who);
  const int chunks = (N + SC_CHUNK - 1) / SC_CHUNK;
  const size_t nx = (size_t)S * N * 12, nc = (size_t)(shared_centers ? 1 : S) * K * 12, no = (size_t)S * K * 12, nm = (size_t)S * K * 4,
               nw = (size_t)S * chunks * K * 16;
  const void* outs[3] = {out, mass, ws};
  const size_t nouts[3] = {no, nm, nw};
  for (int a = 0; a < 3; ++a) {
    if (ranges_overlap(outs[a], nouts[a], x, nx) || ranges_overlap(outs[a], nouts[a], c, nc))
      return set_error(NOVA_ERR_ARG, "%s: out, mass or ws overlaps an input", who);
    for (int b = a + 1; b < 3; ++b)
      if (ranges_overlap(outs[a], nouts[a], outs[b], nouts[b])) return set_error(NOVA_ERR_ARG, "%s: out, mass and ws overlap each other", who);
  }
  const dim3 grid(chunks, S), block(SC_T);
  const size_t cstride = shared_centers ? 0 : (size_t)K * 3;
  if (K <= 8) hipLaunchKernelGGL((soft_cluster_fwd_kernel<8>), grid, block, 0, st, x, c, ws, N, K, cstride, scale);
  else if (K <= 16) hipLaunchKernelGGL((soft_cluster_fwd_kernel<16>), grid, block, 0, st, x, c, ws, N, K, cstride, scale);
  else hipLaunchKernelGGL((soft_cluster_fwd_kernel<32>), grid, block, 0, st, x, c, ws, N, K, cstride, scale);
  hipLaunchKernelGGL(soft_cluster_merge_kernel, dim3((unsigned)(((size_t)S * K + SC_T - 1) / SC_T)), block, 0, st, ws, out, mass, S, K, chunks);
  return check_launch(who);
}

int nova_pointset_soft_cluster_bwd(const float* x, const float* c, const float* out, const float* mass, const float* g, const float* gm,
                                   float* gx, float* gc, float* ws, int S, int N, int K, int shared_centers, float scale, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_soft_cluster_bwd";
  if (const int rc = sc_check(who, S, N, K, scale)) return rc;
  if (S <= 0) return 0;
  if (!x || !c || !out || !mass || !g) return set_error(NOVA_ERR_ARG, "%s: null pointer (x, c, out, mass or g)", who);
  if (!gx && !gc) return set_error(NOVA_ERR_ARG, "%s: no gradient wanted (gx and gc are both NULL)", who);
  if (gc && !ws) return set_error(NOVA_ERR_ARG, "%s: gc needs the workspace ws", who);
  const int chunks = (N + SC_CHUNK - 1) / SC_CHUNK;
  const size_t nx = (size_t)S * N * 12, nc = (size_t)(shared_centers ? 1 : S) * K * 12, no = (size_t)S * K * 12, nm = (size_t)S * K * 4,
               nw = (size_t)S * chunks * K * 12;
  const void* ins[6] = {x, c, out, mass, g, gm};
  const size_t nins[6] = {nx, nc, no, nm, no, nm};
  const void* outs[3] = {gx, gc, gc ? ws : nullptr};
  const size_t nouts[3] = {nx, no, nw};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 6; ++b)
      if (ranges_overlap(outs[a], nouts[a], ins[b], nins[b])) return set_error(NOVA_ERR_ARG, "%s: gx, gc or ws overlaps an input", who);
    for (int b = a + 1; b < 3; ++b)
      if (ranges_overlap(outs[a], nouts[a], outs[b], nouts[b])) return set_error(NOVA_ERR_ARG, "%s: gx, gc and ws overlap each other", who);
  }
  const dim3 grid(chunks, S);
  const size_t cstride = shared_centers ? 0 : (size_t)K * 3;
  if (K <= 8) sc_bwd_launch<8>(grid, st, x, c, out, mass, g, gm, gx, gc, ws, N, K, cstride, scale);
  else if (K <= 16) sc_bwd_launch<16>(grid, st, x, c, out, mass, g, gm, gx, gc, ws, N, K, cstride, scale);
  else sc_bwd_launch<32>(grid, st, x, c, out, mass, g, gm, gx, gc, ws, N, K, cstride, scale);
  if (gc) ordered_sum(st, ws, gc, nullptr, S, chunks, 3 * K, 3 * K);
  return check_launch(who);
}

int nova_pointset_soft_cluster_sum_clouds(const float* gc, float* gcs, int S, int K, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_soft_cluster_sum_clouds";
  if (K < 1 || K > SC_MAX_K) return set_error(NOVA_ERR_SHAPE, "%s: K %d outside 1 .. %d (NOVA_SOFT_CLUSTER_MAX_K)", who, K, SC_MAX_K);
  if (S <= 0) return 0;
  if (!gc || !gcs) return set_error(NOVA_ERR_ARG, "%s: null pointer", who);
  if (ranges_overlap(gcs, (size_t)K * 12, gc, (size_t)S * K * 12)) return set_error(NOVA_ERR_ARG, "%s: gcs overlaps gc", who);
  ordered_sum(st, gc, gcs, nullptr, 1, S, 3 * K, 3 * K);
  return check_launch(who);
}

}  // extern "C"
