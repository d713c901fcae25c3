// Nearest match with indices, and its backward: the primitive under the Chamfer-type training losses of the reference
//   robust_chamfer_distance on distChamfer     train_newloss.py:316-349, 381-384
//   _compute_edge_consistency                  train_newloss.py:449-457  (torch.cdist(...).min(dim=1), mean)
// which in PyTorch keep a [B, N, M] cdist matrix alive for the backward, per direction and per subset pair. Here no
// [N, M] array exists in either pass. The definition (point map p, key order, t_i, the pull-back, the order of the gy sum) is
// in include/nova_hip.h at nova_pointset_nearest_match; this file is that text as code. Plain VALU work on 12-byte
// points, like the rest of the family: K = 3 is no MFMA shape (see the note at the top of pointset.hip).
//
//   nearest_match_kernel      nn_dist_kernel's structure with the index carried along: one query per thread, y tiles of
//                             NM_TILE points mapped through p once and broadcast from LDS (every lane reads one address: no
//                             bank conflicts). A candidate replaces the best only when strictly smaller, and a thread meets
//                             its candidates in ascending j: ties go to the lowest index.
//   nearest_match_gx_kernel   one thread per x point: its term t_i pulled back through p at x_i.
//   nearest_match_gy_kernel   a GATHER: one thread per y_j walks ALL i of its cloud in increasing order and adds the
//                             records that name it. The records (t_i, idx_i) are formed by the workgroup NM_TILE at a time,
//                             staged in LDS as 16-byte entries and read back as broadcasts; every record is added under
//                             idx_i == j, a selected 0.0f otherwise, so each sum has one order whatever the hardware
//                             schedules. No atomics (float atomics would make gy depend on arrival order), no sort.
//
// Cost. Forward: per candidate 1 LDS read (b128), 3 subtractions, 1 multiply, 2 fused multiply-adds, a compare and two
// selects, about 11 issues as compiled, N M of them per cloud. gy: per (record, target) 1 LDS read (b128), a compare, three
// selects and three additions, about 7.5 issues as compiled, N M of them per cloud; forming a record costs about 120
// issues (two point maps, three divisions, square roots) and every workgroup of 256 targets forms all N of its cloud,
// 120 N / 256 per thread against 7.5 N in the walk: 6 % on top. Bytes: every workgroup reads its cloud's x, idx, g and
// the matched y points once, about 32 N bytes (64 KiB at N = 2048) for 256 N pair visits: issue-bound, as the forward is.
#include "nova_internal.h"
#include "pointset_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int NM_T = 256;      // threads per workgroup: queries (forward, gx) or targets (gy)
constexpr int NM_TILE = 1024;  // forward: y points per LDS tile; gy: match records per LDS tile (16 KiB either way)

__global__ __launch_bounds__(NM_T) void nearest_match_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ d,
                                                             int* __restrict__ idx, int N, int M, float lo, float hi, int unit) {
  __shared__ f4v ys[NM_TILE];
  const int b = blockIdx.y;
  const int i = blockIdx.x * NM_T + threadIdx.x;
  const float* xb = x + (size_t)b * N * 3;
  const float* yb = y + (size_t)b * M * 3;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f;
  if (i < N) load_point(xb + (size_t)i * 3, lo, hi, unit, x0, x1, x2);
  float best = __builtin_huge_valf();
  int arg = 0;  // a cloud whose every distance overflows to +inf still names a point
  for (int j0 = 0; j0 < M; j0 += NM_TILE) {
    const int cnt = min(NM_TILE, M - j0);
    __syncthreads();  // the previous tile has been read by every wave
    for (int j = threadIdx.x; j < cnt; j += NM_T) {
      float a, bb, c;
      load_point(yb + (size_t)(j0 + j) * 3, lo, hi, unit, a, bb, c);
      ys[j] = f4v{a, bb, c, 0.f};
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const f4v q = ys[j];
      const float d2 = sqdist3(x0, x1, x2, q[0], q[1], q[2]);
      const bool lower = d2 < best;  // strict, candidates in ascending j: the smallest key (d2, j)
      best = lower ? d2 : best;
      arg = lower ? j0 + j : arg;
    }
  }
  if (i < N) {
    d[(size_t)b * N + i] = sqrtf(best);
    idx[(size_t)b * N + i] = arg;
  }
}

// t_i = g_i u / d for the match (x_i, y_a), a = idx_i: u = p(x_i) - p(y_a) per axis, d = sqrtf(sqdist3) as the forward
// has it, each product g_i u_k rounded and then divided by d, correctly rounded; zero when d == 0 (the subgradient
// convention: coincident points give no NaN and no gradient). Returns a, or -1 for an index outside 0 .. M-1, which is
// never dereferenced and whose term is zero.
__device__ __forceinline__ int match_term(const float* xb, const float* yb, const int* idxb, const float* gb, int i, int M, float lo,
                                          float hi, int unit, float& t0, float& t1, float& t2) {
  t0 = t1 = t2 = 0.f;
  const int a = idxb[i];
  if (a < 0 || a >= M) return -1;
  float p0, p1, p2, q0, q1, q2;
  load_point(xb + (size_t)i * 3, lo, hi, unit, p0, p1, p2);
  load_point(yb + (size_t)a * 3, lo, hi, unit, q0, q1, q2);
  const float dist = sqrtf(sqdist3(p0, p1, p2, q0, q1, q2));
  if (dist != 0.f) {
    const float g = gb[i];
    t0 = __fdiv_rn(__fmul_rn(g, p0 - q0), dist);
    t1 = __fdiv_rn(__fmul_rn(g, p1 - q1), dist);
    t2 = __fdiv_rn(__fmul_rn(g, p2 - q2), dist);
  }
  return a;
}

// J^T t at the point v, J the Jacobian of p: with c = clamp(v), n = |c| (norm3) and inv = 1 / max(n, 1e-8) as load_point has
// them, and pc = c inv,
//   unit, n >= 1e-8:  w = t - pc (pc . t), the dot product as fmaf(pc2, t2, fmaf(pc1, t1, pc0 t0)), each w_k one fmaf; r = w inv
//   unit, n <  1e-8:  r = t inv   (inv = 1e8: torch's gradient of c / clamp_min(|c|, 1e-8) below the floor)
//   otherwise:        r = t
// and r_k = 0 for every coordinate with v_k outside [lo, hi] (bounds inclusive, as torch.clamp's backward has them).
__device__ __forceinline__ void point_pullback(const float* v, float lo, float hi, int unit, float t0, float t1, float t2, float& r0,
                                               float& r1, float& r2) {
  const float v0 = v[0], v1 = v[1], v2 = v[2];
  r0 = t0, r1 = t1, r2 = t2;
  if (unit) {
    const float c0 = clampf(v0, lo, hi), c1 = clampf(v1, lo, hi), c2 = clampf(v2, lo, hi);
    const float n = norm3(c0, c1, c2);
    const float inv = 1.0f / fmaxf(n, 1e-8f);
    if (n >= 1e-8f) {
      const float pc0 = __fmul_rn(c0, inv), pc1 = __fmul_rn(c1, inv), pc2 = __fmul_rn(c2, inv);
      const float dot = __builtin_fmaf(pc2, t2, __builtin_fmaf(pc1, t1, __fmul_rn(pc0, t0)));
      r0 = __builtin_fmaf(-pc0, dot, t0);
      r1 = __builtin_fmaf(-pc1, dot, t1);
      r2 = __builtin_fmaf(-pc2, dot, t2);
    }
    r0 = __fmul_rn(r0, inv);
    r1 = __fmul_rn(r1, inv);
    r2 = __fmul_rn(r2, inv);
  }
  r0 = (v0 >= lo && v0 <= hi) ? r0 : 0.f;
  r1 = (v1 >= lo && v1 <= hi) ? r1 : 0.f;
  r2 = (v2 >= lo && v2 <= hi) ? r2 : 0.f;
}

__global__ __launch_bounds__(NM_T) void nearest_match_gx_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const int* __restrict__ idx, const float* __restrict__ g,
                                                                float* __restrict__ gx, int N, int M, float lo, float hi, int unit) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * NM_T + threadIdx.x;
  if (i >= N) return;
  const float* xb = x + (size_t)b * N * 3;
  float t0, t1, t2, r0, r1, r2;
  match_term(xb, y + (size_t)b * M * 3, idx + (size_t)b * N, g + (size_t)b * N, i, M, lo, hi, unit, t0, t1, t2);
  point_pullback(xb + (size_t)i * 3, lo, hi, unit, t0, t1, t2, r0, r1, r2);
  float* out = gx + ((size_t)b * N + i) * 3;
  out[0] = r0;
  out[1] = r1;
  out[2] = r2;
}

__global__ __launch_bounds__(NM_T) void nearest_match_gy_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const int* __restrict__ idx, const float* __restrict__ g,
                                                                float* __restrict__ gy, int N, int M, float lo, float hi, int unit) {
  __shared__ f4v rec[NM_TILE];  // (t0, t1, t2, the bits of idx_i) of NM_TILE consecutive i
  const int b = blockIdx.y;
  const int j = blockIdx.x * NM_T + threadIdx.x;
  const float* xb = x + (size_t)b * N * 3;
  const float* yb = y + (size_t)b * M * 3;
  const int* idxb = idx + (size_t)b * N;
  const float* gb = g + (size_t)b * N;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i0 = 0; i0 < N; i0 += NM_TILE) {
    const int cnt = min(NM_TILE, N - i0);
    __syncthreads();  // the previous tile has been read by every wave
    for (int k = threadIdx.x; k < cnt; k += NM_T) {
      float t0, t1, t2;
      const int a = match_term(xb, yb, idxb, gb, i0 + k, M, lo, hi, unit, t0, t1, t2);
      rec[k] = f4v{t0, t1, t2, __int_as_float(a)};
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {  // increasing i; every lane reads the same LDS address: broadcast
      const f4v r = rec[k];
      const bool mine = __float_as_int(r[3]) == j;
      s0 += mine ? r[0] : 0.f;
      s1 += mine ? r[1] : 0.f;
      s2 += mine ? r[2] : 0.f;
    }
  }
  if (j >= M) return;
  float r0, r1, r2;
  point_pullback(yb + (size_t)j * 3, lo, hi, unit, -s0, -s1, -s2, r0, r1, r2);
  float* out = gy + ((size_t)b * M + j) * 3;
  out[0] = r0;
  out[1] = r1;
  out[2] = r2;
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_nearest_match(const float* x, const float* y, float* d, int* idx, int B, int N, int M, float lo, float hi, int unit,
                                void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(B <= 0 || N <= 0 || (x && y && d && idx), NOVA_ERR_ARG, "pointset_nearest_match: null pointer");
  NOVA_REQUIRE(lo <= hi, NOVA_ERR_ARG, "pointset_nearest_match: empty clamp range");
  if (B <= 0 || N <= 0) return 0;
  if (M <= 0) return set_error(NOVA_ERR_SHAPE, "pointset_nearest_match: empty target set");
  if (B > 65535) return set_error(NOVA_ERR_SHAPE, "pointset_nearest_match: batch %d too large", B);
  hipLaunchKernelGGL(nearest_match_kernel, dim3((N + NM_T - 1) / NM_T, B), dim3(NM_T), 0, st, x, y, d, idx, N, M, lo, hi, unit);
  return check_launch("pointset_nearest_match");
}

int nova_pointset_nearest_match_bwd(const float* x, const float* y, const int* idx, const float* g, float* gx, float* gy, int B, int N, int M,
                                    float lo, float hi, int unit, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(B <= 0 || N <= 0 || (x && y && idx && g && gx && gy), NOVA_ERR_ARG, "pointset_nearest_match_bwd: null pointer");
  NOVA_REQUIRE(lo <= hi, NOVA_ERR_ARG, "pointset_nearest_match_bwd: empty clamp range");
  if (B <= 0 || N <= 0) return 0;
  if (M <= 0) return set_error(NOVA_ERR_SHAPE, "pointset_nearest_match_bwd: empty target set");
  if (B > 65535) return set_error(NOVA_ERR_SHAPE, "pointset_nearest_match_bwd: batch %d too large", B);
  hipLaunchKernelGGL(nearest_match_gx_kernel, dim3((N + NM_T - 1) / NM_T, B), dim3(NM_T), 0, st, x, y, idx, g, gx, N, M, lo, hi, unit);
  hipLaunchKernelGGL(nearest_match_gy_kernel, dim3((M + NM_T - 1) / NM_T, B), dim3(NM_T), 0, st, x, y, idx, g, gy, N, M, lo, hi, unit);
  return check_launch("pointset_nearest_match_bwd");
}

}  // extern "C"
