// Exact k nearest neighbours of a set of clouds: for every query point of x [S, N, 3] the k points of y [S, M, 3] with the
// smallest keys (float32 squared distance, index), in ascending order. It is the primitive under every local statistic of
// a generated cloud (neighbour spacing, density, outlier filtering); the reference needs it for compute_local_density
// (diffnext/models/transformers/transformer_pointcloud_nova.py:81-89: torch.cdist, topk(k + 1), drop the self column) and
// builds the same cdist + topk(8) structure again at :144-146 and :179-182. The definition, and where it departs from
// that function body, is in include/nova_hip.h at nova_pointset_knn. No [N, M] matrix is ever stored (900 MB per
// 15 000-point cloud in the reference's form, to keep 9 of 15 000 columns per row).
//
// The work is N M candidate evaluations per cloud, plain VALU work on 12-byte points like the other point-set kernels:
// K = 3 is no MFMA shape, and the distance is the exact-difference form (x - y)^2, not cdist's |x|^2 + |y|^2 - 2 x.y
// expansion that cancels for exactly the near neighbours kNN is about.
//
// Layout: a workgroup of 256 threads, one query per thread (SPLIT = 1: 256 queries) or one query per lane with the four
// waves sharing the candidates (SPLIT = 4: 64 queries; wave w owns the 64-point chunks w, w + 4, ... of every tile).
//   1. the workgroup stages a tile of KNN_TILE = 1024 target points in LDS as (x, y, z, -) float4: one ds_read_b128 per
//      candidate, every lane of a wave at the same address (a broadcast: no bank conflicts);
//   2. each thread keeps its K best keys as a sorted list in registers, distances as their bit patterns (d2 >= 0, so bit
//      order is value order; an empty slot is 0xFFFFFFFF, above every distance including +inf). K is a template parameter
//      from the ladder 1 / 2 / 4 / 8 / 16 / 32: the runtime k selects the smallest rung >= k and only the first k entries
//      are written. All list accesses are static after unrolling: no scratch;
//   3. a candidate enters behind a single test  d2 < worst  (one compare and a branch the wave skips when no lane needs
//      it). The insertion is a fully unrolled pass over the list, slot r taking max(list[r-1], min(new, list[r])) and the
//      matching index by two selects: 5 vector instructions per slot. A thread meets its candidates in ascending index
//      order, so the strict test gives a distance tie to the lowest index, inside the list and at its cut-off;
//   4. SPLIT = 4 only: waves 1 .. 3 leave their lists in LDS and wave 0 inserts those 3 K keys into its own, now by the
//      full lexicographic comparison (distance, index), because another wave's candidates are not later in index order.
//      The k smallest of a set of unique keys is one set whatever the order of insertion, so the result is the defined one.
// Self exclusion is by index: candidate j == i gets the empty key and can never pass the test.
//
// SPLIT follows the launch (knn_split below): one 15 000-point cloud is only 59 workgroups of 256 queries on 256 compute
// units, so a launch with fewer than KNN_SPLIT_BELOW such workgroups runs 64 queries per workgroup instead, four times as
// many workgroups with a quarter of the candidates per wave. The result depends on (x[s], y[s], k, exclude_self) alone:
// bitwise the same for every batch, launch split, rung and workgroup shape.
//
// Cost per candidate: 1 LDS read, 3 subtractions, 1 multiply, 2 fused multiply-adds, the self-exclusion compare and select,
// the test: about 10 vector issues, plus 5 K per insertion. A query sees about K ln(M / K) insertions over a cloud in random
// order, and a wave pays for one whenever any of its 64 lanes needs it: at k = 8 and M = 15 000 about a quarter of the
// candidates (some 10 issues each on average), at k = 32 nearly all of them (some 160).
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

constexpr int KNN_MAX_N = NOVA_KNN_MAX_POINTS;  // include/nova_hip.h
constexpr int KNN_MAX_K = NOVA_KNN_MAX_K;
constexpr int KNN_T = 256;            // threads per workgroup
constexpr int KNN_TILE = 1024;        // target points staged per LDS tile (16 KiB)
constexpr int KNN_CHUNK = 64;         // SPLIT = 4: consecutive tile points one wave takes in turn
constexpr int KNN_SPLIT_BELOW = 512;  // launches with fewer 256-query workgroups than this run SPLIT = 4
constexpr uint32_t KNN_EMPTY = 0xFFFFFFFFu;

// (cd, ci) < (d, i); LEX = false compares the distances alone (candidates arriving in ascending index order)
template <bool LEX> __device__ __forceinline__ bool knn_less(uint32_t cd, int ci, uint32_t d, int i) {
  return LEX ? (cd < d || (cd == d && ci < i)) : cd < d;
}

// the sorted list with the key (cd, ci) inserted and its last entry dropped. A key that is not below the last entry leaves
// the list as it is, so the caller's test is an early exit only.
template <int K, bool LEX> __device__ __forceinline__ void knn_insert(uint32_t (&d)[K], int (&ix)[K], uint32_t cd, int ci) {
#pragma unroll
  for (int r = K - 1; r >= 1; --r) {  // downwards: slot r - 1 still holds its old value when slot r takes it
    const bool up = knn_less<LEX>(cd, ci, d[r - 1], ix[r - 1]);  // the new key goes in front of slot r - 1: r - 1 moves to r
    const bool here = knn_less<LEX>(cd, ci, d[r], ix[r]);
    ix[r] = up ? ix[r - 1] : (here ? ci : ix[r]);
    d[r] = umax(d[r - 1], umin(cd, d[r]));  // the median, as d[r - 1] <= d[r]
  }
  ix[0] = knn_less<LEX>(cd, ci, d[0], ix[0]) ? ci : ix[0];
  d[0] = umin(cd, d[0]);
}

template <int K, int SPLIT>
__global__ __launch_bounds__(KNN_T) void knn_kernel(const float* __restrict__ x, const float* __restrict__ y, int* __restrict__ idx,
                                                    float* __restrict__ d2, int N, int M, int k, int exclude_self, int qblocks) {
  constexpr int QPB = KNN_T / SPLIT;                       // queries per workgroup
  constexpr int CH = SPLIT == 1 ? KNN_TILE : KNN_CHUNK;    // tile points a slice takes in one turn
  constexpr int PARTS = (SPLIT - 1) * K * QPB;             // keys the slices 1 .. SPLIT - 1 hand to slice 0
  static_assert(SPLIT == 1 || QPB == 64, "a slice is one wave");
  // one LDS array: the target tile during the scan, then the lists of the slices 1 .. SPLIT - 1 as [slice - 1][r][query]
  __shared__ f4v lds[KNN_TILE > PARTS / 2 ? KNN_TILE : PARTS / 2];
  f4v* ys = lds;
  uint32_t* part_d = reinterpret_cast<uint32_t*>(lds);
  int* part_i = reinterpret_cast<int*>(lds) + PARTS;
  const int t = threadIdx.x;
  const int qi = t % QPB, slice = t / QPB;  // slice is wave-uniform
  const size_t c = blockIdx.x / (unsigned)qblocks;
  const int i = (int)(blockIdx.x % (unsigned)qblocks) * QPB + qi;
  const float* xc = x + c * (size_t)N * 3;
  const float* yc = y + c * (size_t)M * 3;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f;
  if (i < N) {
    x0 = xc[(size_t)i * 3];
    x1 = xc[(size_t)i * 3 + 1];
    x2 = xc[(size_t)i * 3 + 2];
  }
  const int skip = exclude_self ? i : -1;

  uint32_t d[K];
  int ix[K];
#pragma unroll
  for (int r = 0; r < K; ++r) {
    d[r] = KNN_EMPTY;
    ix[r] = 0x7fffffff;
  }

  for (int j0 = 0; j0 < M; j0 += KNN_TILE) {
    const int cnt = min(KNN_TILE, M - j0);
    __syncthreads();  // the previous tile has been read by every wave
    for (int j = t; j < cnt; j += KNN_T) {
      const float* p = yc + (size_t)(j0 + j) * 3;
      ys[j] = f4v{p[0], p[1], p[2], 0.f};
    }
    __syncthreads();
    for (int b = slice * CH; b < cnt; b += SPLIT * CH) {
      const int e = min(b + CH, cnt);
#pragma unroll 4
      for (int j = b; j < e; ++j) {
        const f4v q = ys[j];
        uint32_t bits = __float_as_uint(sqdist3(x0, x1, x2, q[0], q[1], q[2]));
        bits = (j0 + j == skip) ? KNN_EMPTY : bits;
        if (bits < d[K - 1]) knn_insert<K, false>(d, ix, bits, j0 + j);
      }
    }
  }

  if (SPLIT > 1) {
    __syncthreads();  // every wave is done with the last tile: the array changes hands
    if (slice > 0) {
#pragma unroll
      for (int r = 0; r < K; ++r) {
        part_d[((slice - 1) * K + r) * QPB + qi] = d[r];
        part_i[((slice - 1) * K + r) * QPB + qi] = ix[r];
      }
    }
    __syncthreads();
    if (slice > 0) return;
#pragma unroll 1
    for (int e = 0; e < (SPLIT - 1) * K; ++e) {
      const uint32_t cd = part_d[e * QPB + qi];
      const int ci = part_i[e * QPB + qi];
      if (knn_less<true>(cd, ci, d[K - 1], ix[K - 1])) knn_insert<K, true>(d, ix, cd, ci);
    }
  }

  if (i < N) {
    int* out_i = idx + (c * (size_t)N + i) * (size_t)k;
    float* out_d = d2 ? d2 + (c * (size_t)N + i) * (size_t)k : nullptr;
#pragma unroll
    for (int r = 0; r < K; ++r) {
      if (r < k) {
        out_i[r] = ix[r];
        if (out_d) out_d[r] = __uint_as_float(d[r]);
      }
    }
  }
}

// Queries per workgroup by the size of the launch: SPLIT = 4 (64 queries, the four waves sharing the candidates) while
// 256-query workgroups would be fewer than KNN_SPLIT_BELOW, two per compute unit. tools/knn_bench.py and metrics.py restate it.
static int knn_split(int S, int N) { return (long long)S * ((N + KNN_T - 1) / KNN_T) < KNN_SPLIT_BELOW ? 4 : 1; }

template <int K>
static int knn_launch(const float* x, const float* y, int* idx, float* d2, int S, int N, int M, int k, int exclude_self, hipStream_t st) {
  const int split = knn_split(S, N);
  const int qpb = KNN_T / split;
  const int qblocks = (N + qpb - 1) / qpb;
  const long long blocks = (long long)S * qblocks;
  if (blocks > 0x7fffffffLL) return set_error(NOVA_ERR_SHAPE, "pointset_knn: %d clouds of %d points exceed one launch", S, N);
  if (split == 4)
    hipLaunchKernelGGL((knn_kernel<K, 4>), dim3((unsigned)blocks), dim3(KNN_T), 0, st, x, y, idx, d2, N, M, k, exclude_self, qblocks);
  else
    hipLaunchKernelGGL((knn_kernel<K, 1>), dim3((unsigned)blocks), dim3(KNN_T), 0, st, x, y, idx, d2, N, M, k, exclude_self, qblocks);
  return check_launch("pointset_knn");
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_knn(const float* x, const float* y, int* idx, float* d2, int S, int N, int M, int k, int exclude_self, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (N < 1 || N > KNN_MAX_N || M < 1 || M > KNN_MAX_N)
    return set_error(NOVA_ERR_SHAPE, "pointset_knn: N %d or M %d outside 1 .. %d (NOVA_KNN_MAX_POINTS)", N, M, KNN_MAX_N);
  if (exclude_self && N != M) return set_error(NOVA_ERR_SHAPE, "pointset_knn: exclude_self needs N == M, got N %d and M %d", N, M);
  const int k_max = min(KNN_MAX_K, M - (exclude_self ? 1 : 0));
  if (k < 1 || k > k_max)
    return set_error(NOVA_ERR_ARG, "pointset_knn: k %d outside 1 .. %d (NOVA_KNN_MAX_K %d, %d candidates per query)", k, k_max, KNN_MAX_K,
                     M - (exclude_self ? 1 : 0));
  if (S <= 0) return 0;
  if (!x || !y || !idx) return set_error(NOVA_ERR_ARG, "pointset_knn: null pointer");
  if (k <= 1) return knn_launch<1>(x, y, idx, d2, S, N, M, k, exclude_self, st);
  if (k <= 2) return knn_launch<2>(x, y, idx, d2, S, N, M, k, exclude_self, st);
  if (k <= 4) return knn_launch<4>(x, y, idx, d2, S, N, M, k, exclude_self, st);
  if (k <= 8) return knn_launch<8>(x, y, idx, d2, S, N, M, k, exclude_self, st);
  if (k <= 16) return knn_launch<16>(x, y, idx, d2, S, N, M, k, exclude_self, st);
  return knn_launch<32>(x, y, idx, d2, S, N, M, k, exclude_self, st);
}

}  // extern "C"
