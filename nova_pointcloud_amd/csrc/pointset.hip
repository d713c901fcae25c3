// Point-set metrics of the step after generation: the O(N M) pairwise-distance work behind the
// reference's Chamfer and EMD evaluations
//   compute_chamfer_distance / compute_emd_distance   test_optimize.py:354-415  (torch.cdist + min / linear assignment)
//   distChamfer / emd_approx                          train_newloss.py:316-372  (same structure on normalised points)
// Points are [B, n, 3] float32 (what NOVAPipeline's latent output flattens to). Both kernels are plain VALU work on
// 12-byte points: K = 3 is no MFMA shape (a 16-deep contraction would be 81 % padding), the arithmetic is in exact
// differences (x - y)^2 rather than cdist's |x|^2 + |y|^2 - 2 x.y expansion, which cancels for the near neighbours that
// Chamfer is about.
//   nn_dist        d[b, i] = min_j ||clamp(x[b, i]) - clamp(y[b, j])||     one thread per x point, y tiles through LDS
//   pairwise_dist  D[b, i, j] = ||clamp(x[b, i]) - clamp(y[b, j])||        the cost matrix of the assignment problem
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

constexpr int PS_TILE = 1024;  // y points staged per LDS tile (12 KiB)

// load_point (pointset_common.h) is the point map: clamp, and with unit != 0 the scaling to unit norm after it

__global__ __launch_bounds__(256) void nn_dist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                      float* __restrict__ d, int N, int M, float lo, float hi, int unit) {
  __shared__ float ys[PS_TILE * 3];
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float* xb = x + (size_t)b * N * 3;
  const float* yb = y + (size_t)b * M * 3;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f;
  if (i < N) load_point(xb + (size_t)i * 3, lo, hi, unit, x0, x1, x2);
  float best = __builtin_huge_valf();
  for (int j0 = 0; j0 < M; j0 += PS_TILE) {
    const int cnt = min(PS_TILE, M - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) {
      float a, bb, c;
      load_point(yb + (size_t)(j0 + j) * 3, lo, hi, unit, a, bb, c);
      ys[3 * j] = a;
      ys[3 * j + 1] = bb;
      ys[3 * j + 2] = c;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {  // every lane reads the same LDS address: broadcast, no conflicts
      const float d2 = sqdist3(x0, x1, x2, ys[3 * j], ys[3 * j + 1], ys[3 * j + 2]);
      best = fminf(best, d2);
    }
  }
  if (i < N) d[(size_t)b * N + i] = sqrtf(best);
}

__global__ __launch_bounds__(256) void pairwise_dist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            float* __restrict__ D, int N, int M, float lo, float hi) {
  // one workgroup = 16 x points x 256 y points... laid out so that consecutive lanes write consecutive j (coalesced rows)
  const int b = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int i0 = blockIdx.y * 16;
  const float* xb = x + (size_t)b * N * 3;
  const float* yb = y + (size_t)b * M * 3;
  float y0 = 0.f, y1 = 0.f, y2 = 0.f;
  if (j < M) load_point(yb + (size_t)j * 3, lo, hi, 0, y0, y1, y2);
  for (int ii = 0; ii < 16; ++ii) {
    const int i = i0 + ii;
    if (i >= N) break;
    float a, bb, c;
    load_point(xb + (size_t)i * 3, lo, hi, 0, a, bb, c);  // wave-uniform address: one scalar-like broadcast load
    if (j < M) D[((size_t)b * N + i) * M + j] = sqrtf(sqdist3(a, bb, c, y0, y1, y2));
  }
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_nn_dist(const float* x, const float* y, float* d, int B, int N, int M, float lo, float hi, int unit, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(B * (long)N == 0 || (x && y && d), NOVA_ERR_ARG, "pointset_nn_dist: null pointer");
  NOVA_REQUIRE(lo <= hi, NOVA_ERR_ARG, "pointset_nn_dist: empty clamp range");
  if (B <= 0 || N <= 0) return 0;
  if (M <= 0) return set_error(NOVA_ERR_SHAPE, "pointset_nn_dist: empty target set");
  if (B > 65535) return set_error(NOVA_ERR_SHAPE, "pointset_nn_dist: batch %d too large", B);
  hipLaunchKernelGGL(nn_dist_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, x, y, d, N, M, lo, hi, unit);
  return check_launch("pointset_nn_dist");
}

int nova_pointset_pairwise_dist(const float* x, const float* y, float* D, int B, int N, int M, float lo, float hi, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(B * (long)N * M == 0 || (x && y && D), NOVA_ERR_ARG, "pointset_pairwise_dist: null pointer");
  NOVA_REQUIRE(lo <= hi, NOVA_ERR_ARG, "pointset_pairwise_dist: empty clamp range");
  if (B <= 0 || N <= 0 || M <= 0) return 0;
  if (B > 65535 || (N + 15) / 16 > 65535) return set_error(NOVA_ERR_SHAPE, "pointset_pairwise_dist: grid too large");
  hipLaunchKernelGGL(pairwise_dist_kernel, dim3((M + 255) / 256, (N + 15) / 16, B), dim3(256), 0, st, x, y, D, N, M, lo, hi);
  return check_launch("pointset_pairwise_dist");
}

}  // extern "C"
