// Farthest point sampling of a set of clouds (Eldar et al.; PointNet++): n of the N points of each cloud, each new one the
// point farthest from those chosen so far. It brings clouds of different density (15 000-point reference shapes against
// 2048-point generated ones) to the common point count the EMD and the other set-level metrics need. The operation comes
// from the reference's farthest_point_sampling (diffnext/models/transformers/transformer_pointcloud_nova.py:100-125, called
// from adaptive_sampling at :92-97); the definition, and where it deliberately departs from that function body, is in
// include/nova_hip.h at nova_pointset_farthest_point_sample.
//
// The algorithm is n dependent steps, each a distance update of every point plus an argmax over the cloud: latency-bound,
// no roofline to meet. What counts is the time of one step.
//
// Layout: one workgroup of T threads owns one cloud for all n steps and keeps it in registers: thread t holds the points
// r T + t, r = 0 .. P-1, as (x, y, z, mind), the coordinates in pairs so that the three differences, the product and the
// two fused multiply-adds are packed float32 operations (two points per issue, each element rounded exactly as the scalar
// expression of the header). Padded slots carry mind = 0 and can never win.
//
// One step:
//   1. every thread updates its P mind values against the last chosen point q (broadcast in scalar registers) and folds its
//      own best (mind bits, slot), lowest slot on ties;
//   2. the wave reduces the 64-bit key  mind bits << 32 | (0xFFFFFFFF - index)  under max, in two halves on the DPP /
//      v_permlane16_swap / v_permlane32_swap pairing of common.h (wave_combine): first the maximum of the high words, then
//      the maximum of the low words among the lanes that hold it. mind >= 0, so bit order is value order, and the
//      complement makes the lowest index win a tie. No LDS shuffles;
//   3. the lane that owns the wave's winner picks its coordinates (a wave-uniform slot number: one scalar branch, no
//      per-slot selects) and writes key and coordinates to the wave's LDS slot; the slots are double-buffered, so a single
//      workgroup barrier per step orders everything: a slot written in step i is last read before the barrier of step i + 1;
//   4. every wave reads the at most 16 slots (lane l reads slot l mod 16, so every row of 16 lanes sees them all), reduces
//      them with the four in-row DPP steps, and takes q from the winning slot with v_readlane. All waves compute the same q.
// A single-wave workgroup (T = 64) skips 3 and 4: the winner's coordinates come straight out of its lane with v_readlane.
// The barrier is a bare s_barrier behind s_waitcnt lgkmcnt(0): __syncthreads() would also wait for the global stores of
// idx / dist that thread 0 issues each step, a memory round trip on the critical path.
//
// T and P follow N (fps_config below): a small cloud does not pay for a 16-wave barrier, and up to 4096 points the
// workgroup is 4 waves, one per SIMD of a compute unit; more waves add no vector throughput to one cloud, only capacity.
// The result depends on the cloud and its start index alone (a maximum of unique keys has one value whatever the pairing):
// it is bitwise the same for every batch, launch split and workgroup shape.
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

constexpr int FPS_MAX_N = NOVA_FPS_MAX_POINTS;  // include/nova_hip.h

struct FpsShared {
  u4v a[2][16];  // (mind bits, 0xFFFFFFFF - index, x bits, y bits) of a wave's winner
  float z[2][16];
};

__device__ __forceinline__ float fps_readlane(float v, int lane_uniform) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane_uniform));
}

template <int P, int T>
__global__ __launch_bounds__(T) void fps_kernel(const float* __restrict__ x, const int* __restrict__ start, int* __restrict__ idx,
                                               float* __restrict__ dist, int N, int n) {
  constexpr int W = T / 64;             // waves
  constexpr int H = P > 1 ? P / 2 : 1;  // coordinate pairs per thread (P = 1 holds one pair whose second slot is always padding)
  constexpr int SLOTS = 2 * H;
  static_assert(W >= 1 && W <= 16 && (T & (T - 1)) == 0 && P >= 1 && P <= 16 && (P & (P - 1)) == 0, "shape");
  __shared__ FpsShared s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t c = blockIdx.x;
  const float* xc = x + c * (size_t)N * 3;

  f2v px[H], py[H], pz[H];
  uint32_t mind[SLOTS];
#pragma unroll
  for (int r = 0; r < SLOTS; ++r) {
    const int i = r * T + t;
    const bool ok = i < N;
    px[r >> 1][r & 1] = ok ? xc[(size_t)i * 3] : 0.f;
    py[r >> 1][r & 1] = ok ? xc[(size_t)i * 3 + 1] : 0.f;
    pz[r >> 1][r & 1] = ok ? xc[(size_t)i * 3 + 2] : 0.f;
    mind[r] = ok ? F32_INF_BITS : 0u;  // a padded slot stays at 0 under min
  }
  const int s0 = start ? min(max(start[c], 0), N - 1) : 0;  // clamped: an out-of-range start is never dereferenced
  float qx = xc[(size_t)s0 * 3], qy = xc[(size_t)s0 * 3 + 1], qz = xc[(size_t)s0 * 3 + 2];
  int* idx_c = idx + c * (size_t)n;
  float* dist_c = dist ? dist + c * (size_t)n : nullptr;
  if (t == 0) {
    idx_c[0] = s0;
    if (dist_c) dist_c[0] = __uint_as_float(F32_INF_BITS);
  }

  const auto mx = [](uint32_t a, uint32_t b) { return umax(a, b); };
  int buf = 0;
  for (int step = 1; step < n; ++step) {
    // 1. update and fold
    const f2v q2x = {qx, qx}, q2y = {qy, qy}, q2z = {qz, qz};
    uint32_t bh = 0, br = 0;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const f2v e0 = px[h] - q2x, e1 = py[h] - q2y, e2 = pz[h] - q2z;
      const f2v d = __builtin_elementwise_fma(e2, e2, __builtin_elementwise_fma(e1, e1, e0 * e0));  // sqdist3, element by element
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = 2 * h + k;
        mind[r] = umin(mind[r], __float_as_uint(d[k]));
        if (r == 0) {
          bh = mind[0];
        } else if (mind[r] > bh) {  // strict: the lowest slot, i.e. the thread's lowest index, keeps a tie
          bh = mind[r];
          br = r;
        }
      }
    }
    // 2. the wave's maximum key
    const uint32_t mine = br * T + t;
    const uint32_t lo = mine < (uint32_t)N ? 0xFFFFFFFFu - mine : 0u;
    const uint32_t w_hi = wave_combine(bh, mx);
    const uint32_t w_lo = wave_combine(bh == w_hi ? lo : 0u, mx);
    // the winner's coordinates, in the lane that holds them. w_lo == 0 (a wave of padding only): slot number out of range,
    // nothing selected, and the key 0 written below can never win
    const uint32_t w_idx = 0xFFFFFFFFu - (uint32_t)__builtin_amdgcn_readfirstlane((int)w_lo);
    const int w_r = (int)(w_idx / T), w_lane = (int)(w_idx & 63);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    switch (w_r) {  // wave-uniform
#define NOVA_FPS_CASE(R)                                              \
  case R:                                                             \
    if (R < SLOTS) {                                                  \
      sx = px[(R < SLOTS ? R : 0) >> 1][R & 1];                       \
      sy = py[(R < SLOTS ? R : 0) >> 1][R & 1];                       \
      sz = pz[(R < SLOTS ? R : 0) >> 1][R & 1];                       \
    }                                                                 \
    break;
      NOVA_FPS_CASE(0) NOVA_FPS_CASE(1) NOVA_FPS_CASE(2) NOVA_FPS_CASE(3) NOVA_FPS_CASE(4) NOVA_FPS_CASE(5) NOVA_FPS_CASE(6)
      NOVA_FPS_CASE(7) NOVA_FPS_CASE(8) NOVA_FPS_CASE(9) NOVA_FPS_CASE(10) NOVA_FPS_CASE(11) NOVA_FPS_CASE(12)
      NOVA_FPS_CASE(13) NOVA_FPS_CASE(14) NOVA_FPS_CASE(15)
#undef NOVA_FPS_CASE
      default: break;
    }
    uint32_t g_hi, g_idx;
    if (W == 1) {
      g_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_hi);
      g_idx = w_idx;
      qx = fps_readlane(sx, w_lane);
      qy = fps_readlane(sy, w_lane);
      qz = fps_readlane(sz, w_lane);
    } else {
      // 3. one slot per wave, 4. every wave reduces the slots
      if (lane == w_lane) {
        s.a[buf][wave] = u4v{w_hi, w_lo, __float_as_uint(sx), __float_as_uint(sy)};
        s.z[buf][wave] = sz;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const int k = lane & 15;
      u4v a = {0u, 0u, 0u, 0u};
      float z = 0.f;
      if (k < W) {
        a = s.a[buf][k];
        z = s.z[buf][k];
      }
      const uint32_t r_hi = row_combine(a[0], mx);
      const uint32_t r_lo = row_combine(a[0] == r_hi ? a[1] : 0u, mx);
      g_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)r_hi);
      g_idx = 0xFFFFFFFFu - (uint32_t)__builtin_amdgcn_readfirstlane((int)r_lo);
      const int g_wave = (int)((g_idx & (T - 1)) >> 6);  // the wave that owns the point: lane g_wave of row 0 read its slot
      qx = fps_readlane(__uint_as_float(a[2]), g_wave);
      qy = fps_readlane(__uint_as_float(a[3]), g_wave);
      qz = fps_readlane(z, g_wave);
      buf ^= 1;
    }
    if (t == 0) {
      idx_c[step] = (int)g_idx;
      if (dist_c) dist_c[step] = __uint_as_float(g_hi);
    }
  }
}

// Workgroup shape by point count: (P, T) with P T >= N. One wave up to 128 points (no LDS, no barrier), four waves (one
// per SIMD) up to 4096, then as many waves as 16 points per thread need. tools/fps_bench.py and metrics.py restate it.
struct FpsConfig {
  int P, T;
};
static FpsConfig fps_config(int N) {
  if (N <= 64) return {1, 64};
  if (N <= 128) return {2, 64};
  if (N <= 256) return {1, 256};
  if (N <= 512) return {2, 256};
  if (N <= 1024) return {4, 256};
  if (N <= 2048) return {8, 256};
  if (N <= 4096) return {16, 256};
  if (N <= 8192) return {16, 512};
  return {16, 1024};
}

template <int P, int T>
static void fps_launch(const float* x, const int* start, int* idx, float* dist, int S, int N, int n, hipStream_t st) {
  hipLaunchKernelGGL((fps_kernel<P, T>), dim3((unsigned)S), dim3(T), 0, st, x, start, idx, dist, N, n);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_farthest_point_sample(const float* x, const int* start, int* idx, float* dist, int S, int N, int n, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (N < 1 || N > FPS_MAX_N)
    return set_error(NOVA_ERR_SHAPE, "pointset_farthest_point_sample: N %d outside 1 .. %d (NOVA_FPS_MAX_POINTS)", N, FPS_MAX_N);
  if (n < 1 || n > N) return set_error(NOVA_ERR_ARG, "pointset_farthest_point_sample: n %d outside 1 .. N = %d", n, N);
  if (S <= 0) return 0;
  if (!x || !idx) return set_error(NOVA_ERR_ARG, "pointset_farthest_point_sample: null pointer");
  const FpsConfig cfg = fps_config(N);
  switch (cfg.T * 32 + cfg.P) {
    case 64 * 32 + 1: fps_launch<1, 64>(x, start, idx, dist, S, N, n, st); break;
    case 64 * 32 + 2: fps_launch<2, 64>(x, start, idx, dist, S, N, n, st); break;
    case 256 * 32 + 1: fps_launch<1, 256>(x, start, idx, dist, S, N, n, st); break;
    case 256 * 32 + 2: fps_launch<2, 256>(x, start, idx, dist, S, N, n, st); break;
    case 256 * 32 + 4: fps_launch<4, 256>(x, start, idx, dist, S, N, n, st); break;
    case 256 * 32 + 8: fps_launch<8, 256>(x, start, idx, dist, S, N, n, st); break;
    case 256 * 32 + 16: fps_launch<16, 256>(x, start, idx, dist, S, N, n, st); break;
    case 512 * 32 + 16: fps_launch<16, 512>(x, start, idx, dist, S, N, n, st); break;
    default: fps_launch<16, 1024>(x, start, idx, dist, S, N, n, st); break;
  }
  return check_launch("pointset_farthest_point_sample");
}

}  // extern "C"
