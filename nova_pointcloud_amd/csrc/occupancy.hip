// Occupancy grid of a point-cloud set for the JSD column of the set-level quality tables (PointFlow and its successors):
// every point of S clouds [N, 3] is assigned to its nearest node of an R^3 lattice over [-0.5, 0.5]^3 (with in_sphere:
// of the nodes inside the ball of radius 0.5), and per node the kernel counts the points (counters) and the clouds with
// at least one point there (bernoulli). The definition, the tie rule and the two float32 expressions the results rest
// on are in include/nova_hip.h at nova_pointset_occupancy_grid.
//
// All results are integers: they are exact and the same for every launch split, grid size and run. No float atomics.
//
// Layout: one workgroup of 1024 threads owns a block of consecutive clouds and keeps its histogram in LDS, one 32-bit
// word per node: bits 0-23 count the points, bits 24-31 the clouds (so a workgroup takes at most 255 clouds and 2^24 - 1
// points; the launcher sizes the grid by that). A per-cloud "seen" bitmap (R^3 bits, cleared between clouds) tells the
// first point of a cloud on a node from the later ones: ds_or_rtn on the bitmap, then one ds_add of 1 or 1 + 2^24. At the
// end the workgroup adds its non-zero words to the global int64 arrays with ordinary vector atomic adds.
//
// Fast path (the rounded node is a grid node: every point when in_sphere = 0, ~96 % of the points of a cloud that fills
// the ball): per axis i = clamp(rint((p + 0.5) (R - 1)), 0, R - 1), membership in integers. That is the nearest node:
// the squared distance is a sum over the axes and the rounded index minimises each term over the whole lattice.
//
// Slow path (the rounded node is outside the ball): a bounded search, not a scan of all nodes.
//   1. Columns. For fixed (i, j) the grid nodes are k in [klo(i, j), R - 1 - klo(i, j)] (the ball is convex and symmetric),
//      and |p - c(i, j, k)|^2 = a(i, j) + (pz - c_k)^2 with c_k increasing in k, so the nearest node of the column is
//      k = clamp(k_rounded, klo, R - 1 - klo): one candidate per column, R^2 candidates at most. klo is tabulated per
//      workgroup (255 = empty column).
//   2. Window. Let n0 be any grid node and D0 = |p - n0|. The nearest node n* has |p - n*| <= D0, hence |px - c_i*| <= D0
//      and |py - c_j*| <= D0: only the columns with c_i in [px - D0, px + D0] and c_j in [py - D0, py + D0] can hold it.
//      n0 is the rounded node of q = p * min(1, (0.5 - 0.87 h) / |p|), h = 1 / (R - 1): a rounded node lies within
//      sqrt(3)/2 h < 0.87 h of its point, so |n0| <= 0.5 and n0 is a grid node (checked in integers; if float rounding
//      ever says otherwise, n0 is the centre node and the window is simply larger). D0 is inflated by 1e-5 D0 + 1e-6
//      before the window is cut with floor / ceil, far more than the float32 error of either. For a point just outside
//      the grid D0 <= |p| - 0.5 + 1.74 h, a window of about 5 x 5 columns; for a point far away it is the whole grid,
//      R^2 columns, which is the worst case the launch cap of metrics.py is sized by.
//   3. The candidates are compared by the exact-difference squared distance sqdist3, as a 64-bit key
//      (distance bits << 32 | flat index): the minimum key is the nearest node, ties to the lowest flat index.
// Slow-path points do not hold up the fast-path lanes of their wave: after the fast-path commit the wave compacts them
// (ballot + a 64-entry list per wave in LDS) and gives each 64 / m' lanes (m' = the count rounded up to a power of two),
// which split the point's columns and merge their keys by xor shuffles. One slow point in a wave uses all 64 lanes, 64 slow
// points use one lane each, and the loop has no cross-lane traffic.
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

constexpr int OCC_THREADS = 1024;
constexpr int OCC_WAVES = OCC_THREADS / 64;
constexpr int OCC_MAX_R = NOVA_OCC_MAX_RES;  // include/nova_hip.h
constexpr int OCC_COUNT_BITS = 24;
constexpr int OCC_MAX_CLOUDS = 255;                          // the cloud field of a histogram word
constexpr long OCC_MAX_POINTS = (1L << OCC_COUNT_BITS) - 1;  // the point field
constexpr int OCC_MIN_CLOUDS = 2;  // clouds per workgroup of the automatic grid, at least (flush cost against parallelism:
                                   // profiles/occupancy_grid_bench.json sweeps the grid size)
constexpr int OCC_MAX_GRID = 256;     // one workgroup per CU (LDS)

struct OccShared {
  uint32_t hist[OCC_MAX_R * OCC_MAX_R * OCC_MAX_R];       // 128 KiB: points | clouds << 24
  uint32_t seen[OCC_MAX_R * OCC_MAX_R * OCC_MAX_R / 32];  // 4 KiB: nodes the current cloud has touched
  float4 slow[OCC_WAVES][64];                             // 16 KiB: (x, y, z, source lane) of a wave's slow-path points
  float coord[OCC_MAX_R];                                 // node coordinate per axis index
  uint8_t klo[OCC_MAX_R * OCC_MAX_R];                     // first k of column (i, j) inside the ball; 255 = none
  uint32_t outside;
};
static_assert(sizeof(OccShared) <= 160 * 1024, "LDS");

// clamp(rint((p + 0.5) (R - 1)), 0, R - 1), clamped as a float (any finite p, and NaN -> 0, stay in range)
__device__ __forceinline__ int occ_round(float p, float rm1) {
  return (int)fminf(fmaxf(rintf(__fmul_rn(__fadd_rn(p, 0.5f), rm1)), 0.f), rm1);
}

__device__ __forceinline__ bool occ_member(int i, int j, int k, int rm1) {
  const int ti = 2 * i - rm1, tj = 2 * j - rm1, tk = 2 * k - rm1;
  return ti * ti + tj * tj + tk * tk <= rm1 * rm1;
}

__device__ __forceinline__ void occ_commit(OccShared& s, int flat, int* __restrict__ node, size_t point) {
  const uint32_t bit = 1u << (flat & 31);
  const uint32_t old = atomicOr(&s.seen[flat >> 5], bit);
  atomicAdd(&s.hist[flat], (old & bit) ? 1u : 1u + (1u << OCC_COUNT_BITS));
  if (node) node[point] = flat;
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_grid_kernel(const float* __restrict__ x,
                                                                     unsigned long long* __restrict__ counters,
                                                                     unsigned long long* __restrict__ bernoulli,
                                                                     int* __restrict__ node,
                                                                     unsigned long long* __restrict__ outside, int S, int N,
                                                                     int R, int in_sphere, int clouds_per_wg) {
  __shared__ OccShared s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rm1 = R - 1, R3 = R * R * R;
  const float rm1f = (float)rm1;

  for (int c = t; c < R3; c += OCC_THREADS) s.hist[c] = 0;
  if (t < R) s.coord[t] = __fdiv_rn((float)(2 * t - rm1), (float)(2 * rm1));
  if (t < R * R) {
    const int ti = 2 * (t / R) - rm1, tj = 2 * (t % R) - rm1, rem = rm1 * rm1 - ti * ti - tj * tj;
    int k = 0;
    while (2 * k <= rm1 && (2 * k - rm1) * (2 * k - rm1) > rem) ++k;
    s.klo[t] = in_sphere ? (2 * k <= rm1 ? (uint8_t)k : (uint8_t)255) : (uint8_t)0;
  }
  if (t == 0) s.outside = 0;

  const int c0 = blockIdx.x * clouds_per_wg, c1 = min(S, c0 + clouds_per_wg);
  for (int c = c0; c < c1; ++c) {
    __syncthreads();  // the tables are written; the previous cloud's commits are done
    for (int w = t; w < (R3 + 31) / 32; w += OCC_THREADS) s.seen[w] = 0;
    __syncthreads();
    const float* xc = x + (size_t)c * N * 3;
    for (int base = wave * 64; base < N; base += OCC_THREADS) {  // wave-uniform
      const int p = base + lane;
      const bool valid = p < N;
      const float px = valid ? xc[(size_t)p * 3] : 0.f, py = valid ? xc[(size_t)p * 3 + 1] : 0.f,
                  pz = valid ? xc[(size_t)p * 3 + 2] : 0.f;
      const int i = occ_round(px, rm1f), j = occ_round(py, rm1f), k = occ_round(pz, rm1f);
      const bool is_slow = valid && in_sphere && !occ_member(i, j, k, rm1);
      if (valid && !is_slow) occ_commit(s, (i * R + j) * R + k, node, (size_t)c * N + p);
      const unsigned long long mask = __ballot(is_slow);
      if (mask == 0) continue;  // wave-uniform

      // ---- slow path: compact the wave's slow points, 64 / m' lanes each
      const int m = __popcll(mask);
      if (is_slow) s.slow[wave][__popcll(mask & ((1ull << lane) - 1))] = make_float4(px, py, pz, __int_as_float(lane));
      if (lane == 0) atomicAdd(&s.outside, (uint32_t)m);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int mp = m <= 1 ? 1 : 1 << (32 - __clz(m - 1));  // m rounded up to a power of two
      const int g = 64 / mp, e = lane / g, sub = lane - e * g;
      const bool active = e < m;
      const float4 q = s.slow[wave][active ? e : 0];
      // n0: the rounded node of the point pulled inside the radius 0.5 - 0.87 h
      const float rin = 0.5f - 0.87f / rm1f, r = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z);
      const float sc = r > rin ? rin / r : 1.f;
      int i0 = occ_round(q.x * sc, rm1f), j0 = occ_round(q.y * sc, rm1f), k0 = occ_round(q.z * sc, rm1f);
      if (!occ_member(i0, j0, k0, rm1)) i0 = j0 = k0 = R / 2;  // the centre node (a grid node for every R >= 3)
      const float d0 = sqdist3(q.x, q.y, q.z, s.coord[i0], s.coord[j0], s.coord[k0]);
      uint64_t best = ((uint64_t)__float_as_uint(d0) << 32) | (uint32_t)((i0 * R + j0) * R + k0);
      const float D0 = sqrtf(d0) * (1.f + 1e-5f) + 1e-6f;
      const int ilo = (int)fminf(fmaxf(floorf((q.x - D0 + 0.5f) * rm1f), 0.f), rm1f);
      const int ihi = (int)fminf(fmaxf(ceilf((q.x + D0 + 0.5f) * rm1f), 0.f), rm1f);
      const int jlo = (int)fminf(fmaxf(floorf((q.y - D0 + 0.5f) * rm1f), 0.f), rm1f);
      const int jhi = (int)fminf(fmaxf(ceilf((q.y + D0 + 0.5f) * rm1f), 0.f), rm1f);
      const int wj = max(jhi - jlo + 1, 1), ncol = active ? max(ihi - ilo + 1, 0) * wj : 0;
      const float inv_wj = 1.f / (float)wj;  // (col + 0.5) / wj is at least 1 / 64 from an integer: the float quotient floors right
      const int kr = occ_round(q.z, rm1f);
      for (int col = sub; col < ncol; col += g) {
        const int io = (int)(((float)col + 0.5f) * inv_wj);
        const int ci = ilo + io, cj = jlo + col - io * wj;
        const int lo = s.klo[ci * R + cj];
        if (lo == 255) continue;
        const int ck = min(max(kr, lo), rm1 - lo);
        const float d = sqdist3(q.x, q.y, q.z, s.coord[ci], s.coord[cj], s.coord[ck]);
        const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)((ci * R + cj) * R + ck);
        best = umin(key, best);
      }
      for (int off = g >> 1; off >= 1; off >>= 1) {  // wave-uniform: the g lanes of a point are an aligned group
        const uint32_t hi = __shfl_xor((int)(best >> 32), off), lo = __shfl_xor((int)(uint32_t)best, off);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        best = umin(other, best);
      }
      if (active && sub == 0) occ_commit(s, (int)(uint32_t)best, node, (size_t)c * N + base + __float_as_int(q.w));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the list is read before the next batch overwrites it
      __builtin_amdgcn_wave_barrier();
    }
  }

  __syncthreads();
  for (int c = t; c < R3; c += OCC_THREADS) {
    const uint32_t v = s.hist[c];
    if (v) {
      atomicAdd(&counters[c], (unsigned long long)(v & ((1u << OCC_COUNT_BITS) - 1)));
      if (bernoulli) atomicAdd(&bernoulli[c], (unsigned long long)(v >> OCC_COUNT_BITS));
    }
  }
  if (t == 0 && outside && s.outside) atomicAdd(outside, (unsigned long long)s.outside);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_occupancy_grid(const float* x, long long* counters, long long* bernoulli, int* node, long long* outside, int S, int N,
                                 int R, int in_sphere, int workgroups, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (N <= 0) return set_error(NOVA_ERR_SHAPE, "pointset_occupancy_grid: empty cloud (N %d)", N);
  if (N > OCC_MAX_POINTS)
    return set_error(NOVA_ERR_SHAPE, "pointset_occupancy_grid: N %d above %ld points per cloud", N, OCC_MAX_POINTS);
  if (R < 2 || R > OCC_MAX_R)
    return set_error(NOVA_ERR_ARG, "pointset_occupancy_grid: resolution %d outside 2 .. %d (NOVA_OCC_MAX_RES)", R, OCC_MAX_R);
  if (in_sphere && R == 2)
    return set_error(NOVA_ERR_ARG, "pointset_occupancy_grid: resolution 2 with in_sphere has no node inside the ball");
  if (workgroups < 0) return set_error(NOVA_ERR_ARG, "pointset_occupancy_grid: workgroups %d < 0", workgroups);
  if (S <= 0) return 0;
  if (!x || !counters) return set_error(NOVA_ERR_ARG, "pointset_occupancy_grid: null pointer");
  const long cap = std::min<long>(OCC_MAX_CLOUDS, OCC_MAX_POINTS / N);  // clouds a workgroup's histogram words can hold
  const long want = workgroups > 0 ? ((long)S + workgroups - 1) / workgroups
                                   : std::max<long>(OCC_MIN_CLOUDS, ((long)S + OCC_MAX_GRID - 1) / OCC_MAX_GRID);
  const int per_wg = (int)std::max<long>(1, std::min(cap, want));
  const unsigned grid = (unsigned)(((long)S + per_wg - 1) / per_wg);
  hipLaunchKernelGGL(occupancy_grid_kernel, dim3(grid), dim3(OCC_THREADS), 0, st, x, (unsigned long long*)counters,
                     (unsigned long long*)bernoulli, node, (unsigned long long*)outside, S, N, R, in_sphere, per_wg);
  return check_launch("pointset_occupancy_grid");
}

}  // extern "C"
