// All-pairs Chamfer matrix for the set-level quality metrics of generated point clouds (MMD, COV, 1-NNA; PointFlow
// and its successors): cd[a, b] = CD(x_a, y_b) for A x-clouds [N, 3] and B y-clouds [M, 3], with
//   CD(X, Y) = mean_{x in X} min_{y in Y} |x - y|^2 + mean_{y in Y} min_{x in X} |x - y|^2
// in squared Euclidean distances, no clamp and no normalisation (unlike the density-weighted Chamfer of pointset.hip).
//
// One workgroup owns one cloud pair and writes its entry (and the mirrored entry in symmetric mode): no global atomics,
// and every sum runs in a fixed order, so an entry is bitwise the same whatever pair grid the host launches.
//
// Form: exact differences e = p - q, d = sqdist3 (pointset_common.h) on the vector unit. For near points p - q is
// exact (Sterbenz), so d carries a few ulp of relative error whatever the translation of the clouds. The expansion
// |p|^2 + |q|^2 - 2 p.q (the f32 MFMA could take the dot products) loses ~1e-7 |p|^2 / d^2 per term: with 2048 points on
// the unit sphere (nearest-neighbour d^2 ~ 6e-3) that is ~2e-5 per term centred and ~3e-3 after a shift by (8, -8, 8).
//
// Each squared distance feeds both minima. The register side P holds CM_R points per lane (CM_XC = 2048 per
// workgroup); the streamed side Q is staged through LDS as float4 and read as a wave-wide broadcast, four points per
// step. A lane keeps its row minima in registers; for the column minima of the four points, the lane's CM_R values are
// folded in-lane, then across the wave by v_permlane32_swap (c0|c1, c2|c3 halves), v_permlane16_swap (rows) and four
// DPP steps inside each row (10 issues for four columns), and merged over the waves with ds_min_u32 on the bit
// patterns (non-negative floats order as unsigned integers). All minima run on the bit patterns, so no NaN-quieting
// canonicalisation sits in the loop.
// Roles: P = x when N <= CM_XC, else P = y when M <= CM_XC (both fused); when both clouds exceed CM_XC the workgroup
// runs the row pass twice, once per direction. Ragged sizes are padded: P with +1e18, Q with -1e18 (finite
// squares ~1e37 that never win a minimum against points of magnitude << 1e18), and padded entries are not summed.
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

constexpr int CM_THREADS = 256;
constexpr int CM_R = 8;                       // register-side points per lane
constexpr int CM_XC = CM_THREADS * CM_R;      // register-side points per pass
constexpr int CM_TQ = 1024;                   // streamed points per LDS tile (16 KiB of float4 + 4 KiB of minima)
constexpr float CM_PAD = 1e18f;

struct CmShared {
  float4 q[CM_TQ];
  uint32_t colmin[CM_TQ];
  float red[CM_THREADS / 64];
};

// rsum = sum over p in P of min_{q in Q} |p - q|^2; with COLS (requires nP <= CM_XC) also
// csum = sum over q in Q of min_{p in P} |p - q|^2. Both are workgroup-uniform on return.
template <bool COLS>
__device__ void cm_sweep(const float* __restrict__ P, int nP, const float* __restrict__ Q, int nQ, CmShared& s, float& rsum,
                         float& csum) {
  const int t = threadIdx.x, lane = t & 63;
  float racc = 0.f, cacc = 0.f;
  for (int p0 = 0; p0 < nP; p0 += CM_XC) {
    float px[CM_R], py[CM_R], pz[CM_R];
    uint32_t rmin[CM_R];
#pragma unroll
    for (int r = 0; r < CM_R; ++r) {
      const int i = p0 + r * CM_THREADS + t;
      const bool ok = i < nP;
      px[r] = ok ? P[(size_t)i * 3] : CM_PAD;
      py[r] = ok ? P[(size_t)i * 3 + 1] : CM_PAD;
      pz[r] = ok ? P[(size_t)i * 3 + 2] : CM_PAD;
      rmin[r] = F32_INF_BITS;
    }
    for (int q0 = 0; q0 < nQ; q0 += CM_TQ) {
      const int cnt = min(CM_TQ, nQ - q0), cnt4 = (cnt + 3) & ~3;
      __syncthreads();  // the previous tile's readers are done
      for (int j = t; j < cnt4; j += CM_THREADS) {
        const float* src = Q + (size_t)(q0 + j) * 3;
        s.q[j] = j < cnt ? make_float4(src[0], src[1], src[2], 0.f) : make_float4(-CM_PAD, -CM_PAD, -CM_PAD, 0.f);
        if (COLS) s.colmin[j] = F32_INF_BITS;
      }
      __syncthreads();
      for (int j = 0; j < cnt4; j += 4) {
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float4 q = s.q[j + k];  // same address in every lane: broadcast
#pragma unroll
          for (int r = 0; r < CM_R; ++r) {
            const uint32_t d = __float_as_uint(sqdist3(px[r], py[r], pz[r], q.x, q.y, q.z));
            rmin[r] = umin(rmin[r], d);
            c[k] = r == 0 ? d : umin(c[k], d);
          }
        }
        if (COLS) {
          // halves: lanes 0-31 -> column 0 (m01) / 2 (m23), lanes 32-63 -> column 1 / 3
          const auto h01 = __builtin_amdgcn_permlane32_swap(c[0], c[1], false, false);
          const auto h23 = __builtin_amdgcn_permlane32_swap(c[2], c[3], false, false);
          const uint32_t m01 = umin(h01[0], h01[1]), m23 = umin(h23[0], h23[1]);
          // rows: row 0 -> column 0, row 1 -> column 2, row 2 -> column 1, row 3 -> column 3
          const auto rr = __builtin_amdgcn_permlane16_swap(m01, m23, false, false);
          uint32_t m = umin(rr[0], rr[1]);
          m = row_combine(m, [](uint32_t a, uint32_t b) { return umin(a, b); });
          const int row = lane >> 4;
          if ((lane & 15) == 0) atomicMin(&s.colmin[j + (((row & 1) << 1) | (row >> 1))], m);
        }
      }
      if (COLS) {
        __syncthreads();
        for (int j = t; j < cnt; j += CM_THREADS) cacc += __uint_as_float(s.colmin[j]);
      }
    }
#pragma unroll
    for (int r = 0; r < CM_R; ++r)
      if (p0 + r * CM_THREADS + t < nP) racc += __uint_as_float(rmin[r]);
  }
  rsum = block_sum_fixed<CM_THREADS / 64>(racc, s.red);
  csum = COLS ? block_sum_fixed<CM_THREADS / 64>(cacc, s.red) : 0.f;
}

__global__ __launch_bounds__(CM_THREADS) void chamfer_matrix_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    float* __restrict__ cd, int B, int N, int M, long ldc,
                                                                    int symmetric) {
  __shared__ CmShared s;
  const long k = blockIdx.x;
  long a, b;
  if (symmetric) {  // k = b (b + 1) / 2 + a with a <= b
    b = (long)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
    while (b * (b + 1) / 2 > k) --b;
    while ((b + 1) * (b + 2) / 2 <= k) ++b;
    a = k - b * (b + 1) / 2;
  } else {
    a = k / B;
    b = k - a * B;
  }
  const float* xa = x + (size_t)a * N * 3;
  const float* yb = y + (size_t)b * M * 3;
  float tx, ty, rs, cs;  // tx = mean over x of min over y, ty = the reverse
  if (N <= CM_XC) {
    cm_sweep<true>(xa, N, yb, M, s, rs, cs);
    tx = rs / (float)N;
    ty = cs / (float)M;
  } else if (M <= CM_XC) {
    cm_sweep<true>(yb, M, xa, N, s, rs, cs);
    tx = cs / (float)N;
    ty = rs / (float)M;
  } else {
    cm_sweep<false>(xa, N, yb, M, s, rs, cs);
    tx = rs / (float)N;
    cm_sweep<false>(yb, M, xa, N, s, rs, cs);
    ty = rs / (float)M;
  }
  if (threadIdx.x == 0) {
    const float v = tx + ty;
    cd[a * ldc + b] = v;
    if (symmetric && a != b) cd[b * ldc + a] = v;
  }
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_chamfer_matrix(const float* x, const float* y, float* cd, int A, int B, int N, int M, int ldc, int symmetric,
                                 void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  NOVA_REQUIRE(A <= 0 || B <= 0 || (x && y && cd), NOVA_ERR_ARG, "pointset_chamfer_matrix: null pointer");
  NOVA_REQUIRE(ldc >= B, NOVA_ERR_ARG, "pointset_chamfer_matrix: ldc %d < B %d", ldc, B);
  NOVA_REQUIRE(!symmetric || (x == y && A == B && N == M), NOVA_ERR_ARG,
               "pointset_chamfer_matrix: symmetric mode needs x == y, A == B and N == M");
  if (A <= 0 || B <= 0) return 0;
  if (N <= 0 || M <= 0) return set_error(NOVA_ERR_SHAPE, "pointset_chamfer_matrix: empty cloud (N %d, M %d)", N, M);
  const long pairs = symmetric ? (long)A * (A + 1) / 2 : (long)A * B;
  if (pairs > 0x7fffffffL)
    return set_error(NOVA_ERR_SHAPE, "pointset_chamfer_matrix: %ld cloud pairs in one launch; split the pair grid", pairs);
  hipLaunchKernelGGL(chamfer_matrix_kernel, dim3((unsigned)pairs), dim3(CM_THREADS), 0, st, x, y, cd, B, N, M, (long)ldc,
                     symmetric);
  return check_launch("pointset_chamfer_matrix");
}

}  // extern "C"
