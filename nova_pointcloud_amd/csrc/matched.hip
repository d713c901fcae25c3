// Matched-pair distance and its backward: the primitive under the exact-assignment EMD training loss, the reference's
//   emd_approx / robust_emd                    train_newloss.py:352-377, 418-424
// made differentiable with the assignment held fixed: once the permutation is known (assign.hip or scipy), the loss is a sum
// of n distances between matched pairs, and that is its gradient almost everywhere. The definition (clamp, d2, the floor,
// t_k, the masks, corrupt indices) is in include/nova_hip.h at nova_pointset_matched_dist; this file is that text as code.
//
//   matched_dist_kernel      one thread per row i: the pair (i, idx[i]).
//   matched_dist_gx_kernel   one thread per row i: the term of the pair (i, idx[i]), masked by the clamp at x_i.
//   matched_dist_gy_kernel   one thread per column j: the term of the pair (inv[j], j) RECOMPUTED and negated, masked by
//                            the clamp at y_j. A gather through the inverse permutation: no scatter, no atomics, every output
//                            element written exactly once whatever the indices hold.
//
// Cost. A memory-bound row kernel: per point 12 B of x, 4 B of idx and 4 B of g read coalesced (the 12-byte rows of a wave
// are one contiguous 768 B span), one dependent 12 B gather of the partner, 4 or 12 B written: a few dozen bytes and about
// forty issues a point, against the n^2 of the assignment in front of it. Nothing here is tuned and nothing should be.
#include "nova_internal.h"
#include "pointset_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int MD_T = 256;  // threads per workgroup: one point each

__global__ __launch_bounds__(MD_T) void matched_dist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const int* __restrict__ idx, float* __restrict__ d, int n, float lo, float hi,
                                                            float floor) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * MD_T + threadIdx.x;
  if (i >= n) return;
  const size_t row = (size_t)b * n + i;
  const int a = idx[row];
  float out = __builtin_nanf("");  // an index outside 0 .. n-1 is never dereferenced
  if (a >= 0 && a < n) {
    float p0, p1, p2, q0, q1, q2;
    load_point(x + row * 3, lo, hi, 0, p0, p1, p2);
    load_point(y + ((size_t)b * n + a) * 3, lo, hi, 0, q0, q1, q2);
    out = fmaxf(sqrtf(sqdist3(p0, p1, p2, q0, q1, q2)), floor);
  }
  d[row] = out;
}

// t = g_i e / dist for the pair (x_i, y_a) of one cloud: e = c(x_i) - c(y_a) per axis, dist = sqrtf(sqdist3) as the forward
// has it, each product g_i e_k rounded and then divided by dist, correctly rounded; zero when dist == 0 or dist < floor
// (clamp_min's backward and the subgradient convention of nearest_match: no NaN). The caller has checked i and a.
__device__ __forceinline__ void pair_term(const float* xb, const float* yb, const float* gb, int i, int a, float lo, float hi, float floor,
                                          float& t0, float& t1, float& t2) {
  t0 = t1 = t2 = 0.f;
  float p0, p1, p2, q0, q1, q2;
  load_point(xb + (size_t)i * 3, lo, hi, 0, p0, p1, p2);
  load_point(yb + (size_t)a * 3, lo, hi, 0, q0, q1, q2);
  const float dist = sqrtf(sqdist3(p0, p1, p2, q0, q1, q2));
  if (dist != 0.f && !(dist < floor)) {
    const float g = gb[i];
    t0 = __fdiv_rn(__fmul_rn(g, p0 - q0), dist);
    t1 = __fdiv_rn(__fmul_rn(g, p1 - q1), dist);
    t2 = __fdiv_rn(__fmul_rn(g, p2 - q2), dist);
  }
}

// out = t where the coordinate of the differentiated point v lies in [lo, hi], bounds inclusive (torch.clamp's backward), else 0
__device__ __forceinline__ void store_masked(float* out, const float* v, float lo, float hi, float t0, float t1, float t2) {
  const float v0 = v[0], v1 = v[1], v2 = v[2];
  out[0] = (v0 >= lo && v0 <= hi) ? t0 : 0.f;
  out[1] = (v1 >= lo && v1 <= hi) ? t1 : 0.f;
  out[2] = (v2 >= lo && v2 <= hi) ? t2 : 0.f;
}

__global__ __launch_bounds__(MD_T) void matched_dist_gx_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const int* __restrict__ idx, const float* __restrict__ g,
                                                               float* __restrict__ gx, int n, float lo, float hi, float floor) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * MD_T + threadIdx.x;
  if (i >= n) return;
  const float* xb = x + (size_t)b * n * 3;
  const int a = idx[(size_t)b * n + i];
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
  if (a >= 0 && a < n) pair_term(xb, y + (size_t)b * n * 3, g + (size_t)b * n, i, a, lo, hi, floor, t0, t1, t2);
  store_masked(gx + ((size_t)b * n + i) * 3, xb + (size_t)i * 3, lo, hi, t0, t1, t2);
}

__global__ __launch_bounds__(MD_T) void matched_dist_gy_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const int* __restrict__ inv, const float* __restrict__ g,
                                                               float* __restrict__ gy, int n, float lo, float hi, float floor) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * MD_T + threadIdx.x;
  if (j >= n) return;
  const float* yb = y + (size_t)b * n * 3;
  const int i = inv[(size_t)b * n + j];
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
  if (i >= 0 && i < n) pair_term(x + (size_t)b * n * 3, yb, g + (size_t)b * n, i, j, lo, hi, floor, t0, t1, t2);
  store_masked(gy + ((size_t)b * n + j) * 3, yb + (size_t)j * 3, lo, hi, -t0, -t1, -t2);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_matched_dist(const float* x, const float* y, const int* idx, float* d, int B, int n, float lo, float hi, float floor,
                               void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(B <= 0 || n <= 0 || (x && y && idx && d), NOVA_ERR_ARG, "pointset_matched_dist: null pointer");
  NOVA_REQUIRE(lo <= hi, NOVA_ERR_ARG, "pointset_matched_dist: empty clamp range");
  NOVA_REQUIRE(floor >= 0.f, NOVA_ERR_ARG, "pointset_matched_dist: floor must be >= 0");
  if (B <= 0 || n <= 0) return 0;
  if (B > 65535) return set_error(NOVA_ERR_SHAPE, "pointset_matched_dist: batch %d too large", B);
  hipLaunchKernelGGL(matched_dist_kernel, dim3((n + MD_T - 1) / MD_T, B), dim3(MD_T), 0, st, x, y, idx, d, n, lo, hi, floor);
  return check_launch("pointset_matched_dist");
}

int nova_pointset_matched_dist_bwd(const float* x, const float* y, const int* idx, const int* inv, const float* g, float* gx, float* gy, int B,
                                   int n, float lo, float hi, float floor, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(B <= 0 || n <= 0 || (x && y && idx && inv && g && gx && gy), NOVA_ERR_ARG, "pointset_matched_dist_bwd: null pointer");
  NOVA_REQUIRE(lo <= hi, NOVA_ERR_ARG, "pointset_matched_dist_bwd: empty clamp range");
  NOVA_REQUIRE(floor >= 0.f, NOVA_ERR_ARG, "pointset_matched_dist_bwd: floor must be >= 0");
  if (B <= 0 || n <= 0) return 0;
  if (B > 65535) return set_error(NOVA_ERR_SHAPE, "pointset_matched_dist_bwd: batch %d too large", B);
  const dim3 grid((n + MD_T - 1) / MD_T, B);
  hipLaunchKernelGGL(matched_dist_gx_kernel, grid, dim3(MD_T), 0, st, x, y, idx, g, gx, n, lo, hi, floor);
  hipLaunchKernelGGL(matched_dist_gy_kernel, grid, dim3(MD_T), 0, st, x, y, inv, g, gy, n, lo, hi, floor);
  return check_launch("pointset_matched_dist_bwd");
}

}  // extern "C"
