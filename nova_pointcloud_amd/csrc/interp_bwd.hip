// Backward of the distance-weighted interpolation (interp.hip): from the upstream gradient g [S, T, C] of out, the
// gradients gq [S, T, 3] of the queries, gp [S, N, 3] of the source points and gv [S, N, C] of the values. The reference
// reaches this through autograd of feature_aware_interpolation (transformer_pointcloud_nova.py:128-152, called without
// no_grad from adaptive_sampling, :92-97, inside generate_pointcloud_autoregressive, :641-700), which keeps the [S, T, N]
// softmax and the [S, T, N, 3] product alive for it. Here nothing of size T N exists: both kernels recompute d, w and P of
// every pair from the forward's statistics M and L. The definition (every rounding, the order of every sum) is in
// include/nova_hip.h at nova_pointset_kernel_interpolate_bwd; this file is that text as code. An attention backward with
// 3-D keys, plain VALU work like the forward: K = 3 is no MFMA shape (knn.hip).
//
// One pair (i, j), the same in both kernels (interp_pair):
//   e_k = q_i[k] - p_j[k], d = sqrtf(sqdist3) (the forward's interp_dist: M_i <= d bit for bit), w = exp2f((M_i - d) scale),
//   P = w r_i with r_i = 1 / L_i (one IEEE division per query, then one rounded product per pair),
//   dot = g_i . v_j (one product, then fused multiply-adds in ascending channel), s = dot - delta_i,
//   f = (kappa (P s)) rcp(d), rcp the hardware's v_rcp_f32 (1 ulp) and f = 0 where d == 0 (coincident points: no gradient,
//   no NaN), kappa = scale ln 2 rounded once (= 1 / temperature);
//   the query side adds fmaf(-f, e_k, .), the source side fmaf(f, e_k, .) and fmaf(P, g_i[c], .).
// delta_i = g_i . out_i is formed in each kernel's prologue by one expression (interp_delta): no pass of its own, no buffer.
//
//   interp_gq_kernel    the forward's shape unchanged: 256 threads, 64 queries, one per lane in all four waves; tiles of
//                       IGQ_TILE = 1024 sources (points, values) broadcast from LDS; wave w takes the 64-source chunks w,
//                       w + 4, ... in ascending order; M and L are known, so there is no running minimum and no rescale; the
//                       four partial 3-vectors are added by wave 0 in wave order.
//   interp_gpv_kernel   the transpose: 256 threads, one source per lane; the workgroup stages records of IGP_TILE = 512
//                       queries in LDS (q, M, r, delta, g[C]: 3 or 4 float4 each, 24 or 32 KiB), formed once per tile by the
//                       256 threads, and every lane reads them back as broadcasts, walking ALL queries of its cloud in
//                       increasing index and adding: a gather, no atomics, one order of summation.
// Both results depend on (q[s], p[s], v[s], out[s], M[s], L[s], g[s], C, scale) alone: bitwise the same for every batch,
// launch split, position in the batch and run.
//
// Cost per (query, source) pair: the distance 6 + 17 (correctly rounded square root), the weight 3 (v_exp_f32 at a quarter
// rate), P 1, the dot product C', s and the two products 3, the reciprocal 3 (v_rcp_f32 at a quarter rate, compare,
// select), f 1, three fused multiply-adds; the source side adds C' more for gv. As compiled (forms v == NULL, C <= 4,
// C <= 8): 38.75 / 39.75 / 44 vector instructions per pair in the query-side loop and 39.5 / 40.5 / 48.5 in the source-side
// loop, three of them at a quarter rate (+9 issue slots), plus 2 to 4 LDS reads: about 48 to 53 and 49 to 58 slots against
// 43 + C' for the forward, so the backward is 2.2 forward-like passes. Forming a record costs about 60 instructions and
// every workgroup of 256 sources forms all T of its cloud: 60 T / 256 per thread against ~50 T in the walk, 0.5 % on top.
// Compiler report (query side / source side): 56 / 58, 77 / 63, 93 / 81 VGPRs, no scratch; LDS 16 / 24, 32 / 24, 48 / 32 KiB;
// 8 / 6, 5 / 6, 3 / 5 waves per SIMD (the query side's last two bounded by LDS, like the forward's). The record tile is 512
// and not the forward's 1024 for that budget: 1024 records of 64 bytes would leave 2 workgroups per CU of 160 KiB.
#include "interp_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

// the query side keeps the forward's workgroup shape (== INTERP_T, INTERP_Q, INTERP_TILE, INTERP_CHUNK, INTERP_GROUP of
// interp.hip; tests/test_pointset_interp_grad.py compares the two files)
constexpr int IGQ_T = 256;      // threads per workgroup
constexpr int IGQ_Q = 64;       // queries per workgroup: one per lane, in every wave
constexpr int IGQ_WAVES = IGQ_T / IGQ_Q;
constexpr int IGQ_TILE = 1024;  // source points staged per LDS tile
constexpr int IGQ_CHUNK = 64;   // consecutive sources one wave takes in turn
constexpr int IGQ_GROUP = 4;    // sources whose reads, distances and weights are issued together
static_assert(IGQ_TILE % (IGQ_WAVES * IGQ_CHUNK) == 0, "chunk ownership is chunk mod 4 across tiles");
// the source side
constexpr int IGP_T = 256;     // threads per workgroup: one source each
constexpr int IGP_TILE = 512;  // query records staged per LDS tile
constexpr float INTERP_LN2 = 0.693147180559945309f;

// g_i . o_i: one rounded product, then fused multiply-adds in ascending channel (channels past C are zero in both)
template <int CH> __device__ __forceinline__ float interp_delta(const float (&g)[CH], const float (&o)[CH]) {
  float t = g[0] * o[0];
#pragma unroll
  for (int k = 1; k < CH; ++k) t = __builtin_fmaf(g[k], o[k], t);
  return t;
}

// M, r = 1 / L, g[CH], delta of query `row` (a flat index s T + i); channels past C are zero
template <int CH>
__device__ __forceinline__ void interp_query_state(const float* __restrict__ out, const float* __restrict__ m, const float* __restrict__ l,
                                                   const float* __restrict__ g, size_t row, int C, float& M, float& r, float& delta,
                                                   float (&gi)[CH]) {
  float o[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    gi[k] = k < C ? g[row * C + k] : 0.f;
    o[k] = k < C ? out[row * C + k] : 0.f;
  }
  M = m[row];
  r = __fdiv_rn(1.0f, l[row]);  // L >= 1
  delta = interp_delta<CH>(gi, o);
}

// One pair: P, and f = kappa P (g . v - delta) / d, zero at d == 0. (x: the query, y: the source, as the forward has them.)
template <int CH>
__device__ __forceinline__ void interp_pair(float e0, float e1, float e2, float d, float M, float r, float delta, const float (&g)[CH],
                                            const float (&val)[CH], float scale, float kappa, float& P, float& f) {
  P = interp_weight(M, d, scale) * r;
  float dot = g[0] * val[0];
#pragma unroll
  for (int k = 1; k < CH; ++k) dot = __builtin_fmaf(g[k], val[k], dot);
  const float e = kappa * (P * (dot - delta));
  const float rd = d != 0.f ? __builtin_amdgcn_rcpf(d) : 0.f;  // d is 0 or above 3e-23 (the root of a float32): never subnormal
  f = e * rd;
}

template <int CH>
__global__ __launch_bounds__(IGQ_T) void interp_gq_kernel(const float* __restrict__ q, const float* __restrict__ p,
                                                          const float* __restrict__ v, const float* __restrict__ out,
                                                          const float* __restrict__ m, const float* __restrict__ l,
                                                          const float* __restrict__ g, float* __restrict__ gq, int T, int N, int C,
                                                          float scale, int qblocks) {
  constexpr bool SELF = CH == 3;
  constexpr int VQ = SELF ? 0 : CH / 4;  // float4 of values per source
  static_assert((IGQ_WAVES - 1) * 3 * IGQ_Q <= IGQ_TILE * 4, "the partials fit the point tile");
  __shared__ f4v ps[IGQ_TILE];  // the source tile during the scan, then the partials of waves 1 .. 3 as [wave - 1][axis][query]
  __shared__ f4v vs[SELF ? 1 : IGQ_TILE * VQ];  // [source][VQ]
  float* part = reinterpret_cast<float*>(ps);
  const int t = threadIdx.x;
  const int qi = t % IGQ_Q, wave = t / IGQ_Q;
  const size_t c = blockIdx.x / (unsigned)qblocks;
  const int i = (int)(blockIdx.x % (unsigned)qblocks) * IGQ_Q + qi;
  const float* pc = p + c * (size_t)N * 3;
  const float* vc = SELF ? nullptr : v + c * (size_t)N * C;
  // a lane past the last query works on the origin with g = 0, r = 0 and stores nothing
  float x0 = 0.f, x1 = 0.f, x2 = 0.f, M = 0.f, r = 0.f, delta = 0.f, gi[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) gi[k] = 0.f;
  if (i < T) {
    const size_t row = c * (size_t)T + i;
    x0 = q[row * 3];
    x1 = q[row * 3 + 1];
    x2 = q[row * 3 + 2];
    interp_query_state<CH>(out, m, l, g, row, C, M, r, delta, gi);
  }
  const float kappa = scale * INTERP_LN2;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;

  for (int j0 = 0; j0 < N; j0 += IGQ_TILE) {
    const int cnt = min(IGQ_TILE, N - j0);
    __syncthreads();  // the previous tile has been read by every wave
    for (int j = t; j < cnt; j += IGQ_T) {
      const float* s = pc + (size_t)(j0 + j) * 3;
      ps[j] = f4v{s[0], s[1], s[2], 0.f};
      if (!SELF) {
        const float* sv = vc + (size_t)(j0 + j) * C;
#pragma unroll
        for (int h = 0; h < VQ; ++h) {
          f4v val;
#pragma unroll
          for (int k = 0; k < 4; ++k) val[k] = 4 * h + k < C ? sv[4 * h + k] : 0.f;
          vs[j * VQ + h] = val;
        }
      }
    }
    __syncthreads();
    for (int b = wave * IGQ_CHUNK; b < cnt; b += IGQ_WAVES * IGQ_CHUNK) {
      const int e = min(b + IGQ_CHUNK, cnt);
      int j = b;
      // IGQ_GROUP sources at a time: their LDS reads, square roots and exponentials are independent and go ahead of the
      // three sums, which take the sources one by one in index order
      for (; j + IGQ_GROUP <= e; j += IGQ_GROUP) {
        f4v s[IGQ_GROUP];
        float val[IGQ_GROUP][CH], P[IGQ_GROUP], f[IGQ_GROUP];
#pragma unroll
        for (int u = 0; u < IGQ_GROUP; ++u) s[u] = ps[j + u];
#pragma unroll
        for (int u = 0; u < IGQ_GROUP; ++u) interp_values<CH>(val[u], s[u], vs, j + u);
#pragma unroll
        for (int u = 0; u < IGQ_GROUP; ++u)
          interp_pair<CH>(x0 - s[u][0], x1 - s[u][1], x2 - s[u][2], interp_dist(x0, x1, x2, s[u][0], s[u][1], s[u][2]), M, r, delta, gi,
                          val[u], scale, kappa, P[u], f[u]);
#pragma unroll
        for (int u = 0; u < IGQ_GROUP; ++u) {
          a0 = __builtin_fmaf(-f[u], x0 - s[u][0], a0);
          a1 = __builtin_fmaf(-f[u], x1 - s[u][1], a1);
          a2 = __builtin_fmaf(-f[u], x2 - s[u][2], a2);
        }
      }
      for (; j < e; ++j) {
        const f4v s = ps[j];
        float val[CH], P, f;
        interp_values<CH>(val, s, vs, j);
        interp_pair<CH>(x0 - s[0], x1 - s[1], x2 - s[2], interp_dist(x0, x1, x2, s[0], s[1], s[2]), M, r, delta, gi, val, scale, kappa, P, f);
        a0 = __builtin_fmaf(-f, x0 - s[0], a0);
        a1 = __builtin_fmaf(-f, x1 - s[1], a1);
        a2 = __builtin_fmaf(-f, x2 - s[2], a2);
      }
    }
  }

  __syncthreads();  // every wave is done with the last tile: the point array changes hands
  if (wave > 0) {
    float* mine = part + (wave - 1) * 3 * IGQ_Q + qi;
    mine[0] = a0;
    mine[IGQ_Q] = a1;
    mine[2 * IGQ_Q] = a2;
  }
  __syncthreads();
  if (wave > 0) return;
  // wave w has a source when N > 64 w, the same for every query; the others contribute nothing
#pragma unroll
  for (int w = 1; w < IGQ_WAVES; ++w) {
    if (w * IGQ_CHUNK < N) {
      const float* theirs = part + (w - 1) * 3 * IGQ_Q + qi;
      a0 = a0 + theirs[0];
      a1 = a1 + theirs[IGQ_Q];
      a2 = a2 + theirs[2 * IGQ_Q];
    }
  }
  if (i < T) {
    float* o = gq + (c * (size_t)T + i) * 3;
    o[0] = a0;
    o[1] = a1;
    o[2] = a2;
  }
}

template <int CH>
__global__ __launch_bounds__(IGP_T) void interp_gpv_kernel(const float* __restrict__ q, const float* __restrict__ p,
                                                           const float* __restrict__ v, const float* __restrict__ out,
                                                           const float* __restrict__ m, const float* __restrict__ l,
                                                           const float* __restrict__ g, float* __restrict__ gp, float* __restrict__ gv, int T,
                                                           int N, int C, float scale, int pblocks) {
  constexpr bool SELF = CH == 3;
  constexpr int RQ = (6 + CH + 3) / 4;  // float4 per record: (q0, q1, q2, M), (r, delta, g0, g1), (g2, ...), zero-padded
  __shared__ f4v rec[IGP_TILE * RQ];
  const int t = threadIdx.x;
  const size_t c = blockIdx.x / (unsigned)pblocks;
  const int j = (int)(blockIdx.x % (unsigned)pblocks) * IGP_T + t;
  // a lane past the last source works on the origin with zero values and stores nothing
  float y0 = 0.f, y1 = 0.f, y2 = 0.f, val[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) val[k] = 0.f;
  if (j < N) {
    const float* s = p + (c * (size_t)N + j) * 3;
    y0 = s[0];
    y1 = s[1];
    y2 = s[2];
    if (SELF) {
      val[0] = y0;
      val[1] = y1;
      val[2] = y2;
    } else {
      const float* sv = v + (c * (size_t)N + j) * C;
#pragma unroll
      for (int k = 0; k < CH; ++k) val[k] = k < C ? sv[k] : 0.f;
    }
  }
  const float kappa = scale * INTERP_LN2;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, av[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) av[k] = 0.f;

  for (int i0 = 0; i0 < T; i0 += IGP_TILE) {
    const int cnt = min(IGP_TILE, T - i0);
    __syncthreads();  // the previous tile has been read by every wave
    for (int k = t; k < cnt; k += IGP_T) {
      const size_t row = c * (size_t)T + i0 + k;
      float flat[RQ * 4], gi[CH];
#pragma unroll
      for (int u = 0; u < RQ * 4; ++u) flat[u] = 0.f;
      flat[0] = q[row * 3];
      flat[1] = q[row * 3 + 1];
      flat[2] = q[row * 3 + 2];
      interp_query_state<CH>(out, m, l, g, row, C, flat[3], flat[4], flat[5], gi);
#pragma unroll
      for (int u = 0; u < CH; ++u) flat[6 + u] = gi[u];
#pragma unroll
      for (int h = 0; h < RQ; ++h) rec[k * RQ + h] = f4v{flat[4 * h], flat[4 * h + 1], flat[4 * h + 2], flat[4 * h + 3]};
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < cnt; ++k) {  // increasing i; every lane reads the same LDS addresses: broadcasts
      float flat[RQ * 4], gi[CH], P, f;
#pragma unroll
      for (int h = 0; h < RQ; ++h) {
        const f4v u = rec[k * RQ + h];
#pragma unroll
        for (int z = 0; z < 4; ++z) flat[4 * h + z] = u[z];
      }
#pragma unroll
      for (int u = 0; u < CH; ++u) gi[u] = flat[6 + u];
      const float e0 = flat[0] - y0, e1 = flat[1] - y1, e2 = flat[2] - y2;
      interp_pair<CH>(e0, e1, e2, interp_dist(flat[0], flat[1], flat[2], y0, y1, y2), flat[3], flat[4], flat[5], gi, val, scale, kappa, P, f);
      a0 = __builtin_fmaf(f, e0, a0);
      a1 = __builtin_fmaf(f, e1, a1);
      a2 = __builtin_fmaf(f, e2, a2);
#pragma unroll
      for (int u = 0; u < CH; ++u) av[u] = __builtin_fmaf(P, gi[u], av[u]);
    }
  }
  if (j >= N) return;
  if (gp) {
    float* o = gp + (c * (size_t)N + j) * 3;
    o[0] = SELF ? a0 + av[0] : a0;  // v == NULL: the values are the points, whose gradient takes both parts
    o[1] = SELF ? a1 + av[1] : a1;
    o[2] = SELF ? a2 + av[2] : a2;
  }
  if (!SELF && gv) {
    float* o = gv + (c * (size_t)N + j) * C;
#pragma unroll
    for (int k = 0; k < CH; ++k)
      if (k < C) o[k] = av[k];
  }
}

template <int CH>
static int interp_bwd_launch(const char* who, const float* q, const float* p, const float* v, const float* out, const float* m, const float* l,
                             const float* g, float* gq, float* gp, float* gv, int S, int T, int N, int C, float scale, hipStream_t st) {
  const int qblocks = (T + IGQ_Q - 1) / IGQ_Q, pblocks = (N + IGP_T - 1) / IGP_T;
  if ((long long)S * qblocks > 0x7fffffffLL || (long long)S * pblocks > 0x7fffffffLL)
    return set_error(NOVA_ERR_SHAPE, "%s: %d clouds of %d queries and %d sources exceed one launch", who, S, T, N);
  if (gq)
    hipLaunchKernelGGL((interp_gq_kernel<CH>), dim3((unsigned)(S * qblocks)), dim3(IGQ_T), 0, st, q, p, v, out, m, l, g, gq, T, N, C, scale,
                       qblocks);
  if (gp || gv)
    hipLaunchKernelGGL((interp_gpv_kernel<CH>), dim3((unsigned)(S * pblocks)), dim3(IGP_T), 0, st, q, p, v, out, m, l, g, gp, gv, T, N, C,
                       scale, pblocks);
  return check_launch(who);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_kernel_interpolate_bwd(const float* q, const float* p, const float* v, const float* out, const float* m, const float* l,
                                         const float* g, float* gq, float* gp, float* gv, int S, int T, int N, int C, float scale, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_kernel_interpolate_bwd";
  if (const int rc = interp_check(who, q, p, v, out, S, T, N, C, scale)) return rc;
  if (S > 0) {
    if (!m || !l || !g) return set_error(NOVA_ERR_ARG, "%s: null pointer (m, l or g)", who);
    if (!v && gv) return set_error(NOVA_ERR_ARG, "%s: gv must be NULL when v is (the values are the points: their gradient is in gp)", who);
    if (v && gp && !gv) return set_error(NOVA_ERR_ARG, "%s: gv must be given with gp when v is (one kernel forms both)", who);
    if (!gq && !gp && !gv) return set_error(NOVA_ERR_ARG, "%s: no gradient wanted (gq, gp and gv are all NULL)", who);
  }
  if (S <= 0) return 0;
  if (!v) return interp_bwd_launch<3>(who, q, p, v, out, m, l, g, gq, gp, gv, S, T, N, C, scale, st);
  if (C <= 4) return interp_bwd_launch<4>(who, q, p, v, out, m, l, g, gq, gp, gv, S, T, N, C, scale, st);
  return interp_bwd_launch<8>(who, q, p, v, out, m, l, g, gq, gp, gv, S, T, N, C, scale, st);
}

}  // extern "C"
