// All-pairs EMD matrix for the set-level quality metrics of generated point clouds (MMD, COV, 1-NNA under the Earth
// Mover's Distance; PointFlow and its successors): emd[a, b] = EMD(x_a, y_b) for A x-clouds and B y-clouds of N points.
//
// The EMD is not the exact assignment but the approximate matching of Fan et al. ("approxmatch") followed by its match
// cost, divided by n (PointFlow's emd_approx). For X = {p_k}, Y = {q_l}, both of n points, and d2[k, l] = |p_k - q_l|^2
// (squared Euclidean, float32 input used as given, no clamp and no normalisation):
//
//   remainL[k] = 1, remainR[l] = 1, cost = 0
//   for j in 7, 6, 5, 4, 3, 2, 1, 0, -1, -2:                  # 10 levels
//       level = -(4 ** j)            (j = -2: level = 0)       # -16384, -4096, ..., -0.25, 0
//       E[k, l] = exp(level * d2[k, l])
//       A (per k):  ratioL[k] = remainL[k] / (1e-9 + sum_l E[k, l] * remainR[l])
//       B (per l):  s = remainR[l] * sum_k E[k, l] * ratioL[k]
//                   ratioR[l] = min(remainR[l] / (s + 1e-9), 1) * remainR[l]
//                   remainR[l] = max(0, remainR[l] - s)
//       C (per k):  w[k, l] = E[k, l] * ratioL[k] * ratioR[l]
//                   cost += sum_l w[k, l] * sqrt(d2[k, l]);   remainL[k] = max(0, remainL[k] - sum_l w[k, l])
//   EMD(X, Y) = cost / n
//
// It is not symmetric (X, the first cloud, carries remainL), it is translation-invariant but not scale-invariant (the
// levels are absolute squared distances), and all mass is moved (level 0 matches the whole remainder), so it is >= the
// exact-assignment EMD. The n x n match matrix is never formed: the cost is linear in it and is accumulated in pass C.
//
// One workgroup owns one cloud pair and is the only writer of its entry: no global atomics, and every sum runs in a
// fixed order, so an entry is bitwise the same whatever pair grid the host launches. Each sum of the algorithm is a
// per-point serial loop over the other cloud (A and C: k outside, l inside; B: l outside, k inside); only the final
// cost is a workgroup reduction, in a fixed order.
//
// Layout: both clouds in LDS as float4 (x, y, z, weight), read as wave-wide broadcasts four points per step. The L
// weight is ratioL, the R weight ratioR, and remainR has an array of its own. A lane owns R points of each cloud
// (point i = r * T + t): as k it keeps remainL and ratioL in registers, as l it keeps remainR and is the only writer of
// that point's LDS weights. Pass C of level j and pass A of level j - 1 run in one sweep (both k outside, l inside; both
// weights are known after pass B), so a pair takes 21 sweeps instead of 30, with every sum in its own order.
// Precision: E = v_exp_f32(level * log2(e) * d2), sqrt = v_sqrt_f32, exact differences p - q as in chamfer.hip (no
// |p|^2 + |q|^2 - 2 p.q). Padded points (i >= N) carry zero weight and zero mass: their terms are exactly +0.
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

constexpr int EMD_MAX_N = NOVA_EMD_MAX_POINTS;  // include/nova_hip.h
constexpr int EMD_LEVELS = 10;

template <int NP, int WAVES> struct EmdShared {
  float4 L[NP];   // (x, y, z, ratioL)
  float4 R[NP];   // (x, y, z, ratioR)
  float rem[NP];  // remainR
  float red[WAVES];
};

// level * log2(e) of level index 0..9 (j = 7 - index): exp(level * d2) = exp2(emd_level_log2(i) * d2)
__device__ __forceinline__ float emd_level_log2(int i) {
  return i == EMD_LEVELS - 1 ? -0.f : -(float)(1 << (2 * (EMD_LEVELS - 2 - i))) * 0.25f * 1.4426950408889634f;
}

// One sweep with the lane's points (R per lane) outside and the n4 points of the other side (Rq) inside, each lane point
// with its own serial sums:
//   DO_C: sw[r] = sum_l E_c[k, l] ratioR[l], sc[r] = sum_l E_c[k, l] ratioR[l] sqrt(d2[k, l])  (pass C, level cC)
//   DO_A: sa[r] = sum_l E_a[k, l] remainR[l] (rem)                                             (pass A, level cA)
//         or, with A_FROM_W, sum_k E_a[k, l] ratioL[k] (Rq's weight): pass B, the lane's l points against the L side
template <int R, bool DO_C, bool DO_A, bool A_FROM_W = false>
__device__ __forceinline__ void emd_row_sweep(const float4* __restrict__ Rq, const float* __restrict__ rem, int n4,
                                              const float (&px)[R], const float (&py)[R], const float (&pz)[R], float cC,
                                              float cA, float (&sw)[R], float (&sc)[R], float (&sa)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) sw[r] = sc[r] = sa[r] = 0.f;
  for (int l = 0; l < n4; l += 4) {
    float4 q[4];
    float m[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      q[u] = Rq[l + u];  // same address in every lane: broadcast
      m[u] = DO_A ? (A_FROM_W ? q[u].w : rem[l + u]) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float d2 = sqdist3(px[r], py[r], pz[r], q[u].x, q[u].y, q[u].z);
        if (DO_C) {
          const float t = __builtin_amdgcn_exp2f(cC * d2) * q[u].w;
          sw[r] += t;
          sc[r] = __builtin_fmaf(t, __builtin_amdgcn_sqrtf(d2), sc[r]);
        }
        if (DO_A) sa[r] = __builtin_fmaf(__builtin_amdgcn_exp2f(cA * d2), m[u], sa[r]);
      }
  }
}

template <int T, int R>
__global__ __launch_bounds__(T) void emd_matrix_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       float* __restrict__ emd, int B, int N, long ldc) {
  constexpr int NP = T * R;
  __shared__ EmdShared<NP, T / 64> s;
  const long pair = blockIdx.x, a = pair / B, b = pair - a * B;
  const float* xa = x + (size_t)a * N * 3;
  const float* yb = y + (size_t)b * N * 3;
  const int t = threadIdx.x, n4 = (N + 3) & ~3;

  float px[R], py[R], pz[R], remL[R], ratL[R], remR[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = r * T + t;
    const bool ok = i < N;
    px[r] = ok ? xa[(size_t)i * 3] : 0.f;
    py[r] = ok ? xa[(size_t)i * 3 + 1] : 0.f;
    pz[r] = ok ? xa[(size_t)i * 3 + 2] : 0.f;
    s.R[i] = ok ? make_float4(yb[(size_t)i * 3], yb[(size_t)i * 3 + 1], yb[(size_t)i * 3 + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    remL[r] = remR[r] = ok ? 1.f : 0.f;
    s.rem[i] = remR[r];
  }
  __syncthreads();

  float sw[R], sc[R], sa[R], cost = 0.f;
  // pass A of the first level
  emd_row_sweep<R, false, true>(s.R, s.rem, n4, px, py, pz, 0.f, emd_level_log2(0), sw, sc, sa);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ratL[r] = remL[r] / (1e-9f + sa[r]);
    s.L[r * T + t] = make_float4(px[r], py[r], pz[r], ratL[r]);
  }
  for (int lev = 0; lev < EMD_LEVELS; ++lev) {
    const float c = emd_level_log2(lev);
    __syncthreads();  // ratioL of every k is in LDS; the readers of the R weights (the last row sweep) are done
    // pass B: the lane's l points against every k
    float qx[R], qy[R], qz[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 q = s.R[r * T + t];
      qx[r] = q.x;
      qy[r] = q.y;
      qz[r] = q.z;
    }
    emd_row_sweep<R, false, true, true>(s.L, nullptr, n4, qx, qy, qz, 0.f, c, sw, sc, sa);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = r * T + t;
      const float sB = remR[r] * sa[r];
      s.R[i].w = fminf(remR[r] / (sB + 1e-9f), 1.f) * remR[r];
      remR[r] = fmaxf(0.f, remR[r] - sB);
      s.rem[i] = remR[r];
    }
    __syncthreads();  // ratioR and remainR of every l are in LDS; the readers of ratioL (pass B) are done
    // pass C of this level, fused with pass A of the next
    if (lev + 1 < EMD_LEVELS)
      emd_row_sweep<R, true, true>(s.R, s.rem, n4, px, py, pz, c, emd_level_log2(lev + 1), sw, sc, sa);
    else
      emd_row_sweep<R, true, false>(s.R, s.rem, n4, px, py, pz, c, 0.f, sw, sc, sa);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cost += ratL[r] * sc[r];
      remL[r] = fmaxf(0.f, remL[r] - ratL[r] * sw[r]);
      if (lev + 1 < EMD_LEVELS) {
        ratL[r] = remL[r] / (1e-9f + sa[r]);
        s.L[r * T + t].w = ratL[r];
      }
    }
  }

  // block_sum_fixed's order (wave_sum's pairing, then the waves in index order), with thread 0 alone reading the slots
  cost = wave_sum(cost);
  if ((t & 63) == 0) s.red[t >> 6] = cost;
  __syncthreads();
  if (t == 0) {
    float total = s.red[0];
#pragma unroll
    for (int w = 1; w < T / 64; ++w) total += s.red[w];
    emd[a * ldc + b] = total / (float)N;
  }
}

template <int T, int R>
static void emd_launch(const float* x, const float* y, float* emd, long pairs, int B, int N, int ldc, hipStream_t st) {
  hipLaunchKernelGGL((emd_matrix_kernel<T, R>), dim3((unsigned)pairs), dim3(T), 0, st, x, y, emd, B, N, (long)ldc);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_emd_matrix(const float* x, const float* y, float* emd, int A, int B, int N, int ldc, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(A <= 0 || B <= 0 || (x && y && emd), NOVA_ERR_ARG, "pointset_emd_matrix: null pointer");
  NOVA_REQUIRE(ldc >= B, NOVA_ERR_ARG, "pointset_emd_matrix: ldc %d < B %d", ldc, B);
  NOVA_REQUIRE(N >= 1 && N <= EMD_MAX_N, NOVA_ERR_ARG,
               "pointset_emd_matrix: N %d outside 1 .. %d (the maximum point count NOVA_EMD_MAX_POINTS)", N, EMD_MAX_N);
  if (A <= 0 || B <= 0) return 0;
  const long pairs = (long)A * B;
  if (pairs > 0x7fffffffL)
    return set_error(NOVA_ERR_SHAPE, "pointset_emd_matrix: %ld cloud pairs in one launch; split the pair grid", pairs);
  if (N <= 256)
    emd_launch<256, 1>(x, y, emd, pairs, B, N, ldc, st);
  else if (N <= 512)
    emd_launch<256, 2>(x, y, emd, pairs, B, N, ldc, st);
  else if (N <= 1024)
    emd_launch<256, 4>(x, y, emd, pairs, B, N, ldc, st);
  else if (N <= 2048)
    emd_launch<256, 8>(x, y, emd, pairs, B, N, ldc, st);
  else
    emd_launch<512, 8>(x, y, emd, pairs, B, N, ldc, st);
  return check_launch("pointset_emd_matrix");
}

}  // extern "C"
