// kNN neighbourhood feature aggregation, forward and backward: for every query row of idx [S, N, k] the mean, or the weighted
// sum, of the k rows of f [S, M, C] it names. The reference has it on its gradient path as
//   EdgeAligner.extract_edge_features            diffnext/models/transformers/transformer_pointcloud_nova.py:176-190
// (torch.cdist, topk(8), a gather to [B, N, k, C], mean, on 768-wide features, called for every subset in
// EdgeAligner.forward, :192-223), keeping the [B, N, N] matrix and the [B, N, k, C] tensor alive for the backward. Here
// nova_pointset_knn supplies the indices and nothing of size N M or N k C exists in either pass. The definition (every
// rounding, the order of every sum, out-of-range indices) is in include/nova_hip.h at nova_pointset_neighbor_aggregate;
// this file is that text as code.
//
//   neighbor_fwd_kernel     one wave per query row: lane t < k holds the row's index t (and weight), read once; the wave walks
//                           the channels in chunks of 64 lanes x V floats (V = 4: 16-byte loads when C % 4 == 0 and the rows
//                           are 16-byte aligned, V = 1 otherwise) and, per chunk, the k neighbour rows in order t. A channel's
//                           arithmetic does not depend on V, so both widths give the same bits.
//   neighbor_gw_kernel      one wave per query row: per neighbour t the dot product of the g row and the neighbour's f row,
//                           lane l summing its channels l, l + 64, ... in turn, then wave_sum's fixed pairing. Always 4-byte
//                           loads (one reduction shape for every C); lane t keeps result t and the row is stored once.
//   neighbor_gf_kernel      one wave per TARGET row j: it walks j's segment of the inverse list 64 edge ids at a time (lane r
//                           holds edge r of the batch and its weight), and per edge adds one g row. A gather: no atomics.
//   neighbor_count_kernel,  the inverse list by two scans: the indices of a cloud are walked from LDS tiles (one 16-byte LDS read, the
//   neighbor_scan_kernel,   same address in every lane, per 4 indices), one target per lane, 64 targets per workgroup, its four waves
//   neighbor_fill_kernel    taking a quarter of the edge range each, and the matches are counted; one workgroup per cloud turns the
//                           counts into exclusive prefix sums; the walk is repeated, writing edge ids from the target's offset plus
//                           the counts of the quarters before (recounted: a third walk). A thread meets its edges in increasing
//                           e and the quarters are in increasing e, so the list is the stable sort of the in-range edges by
//                           target without a sort. 3 M N k integer compares per cloud (2 M N k in the definition's two scans,
//                           one recount); integers only, so the result is one list for every launch.
//
// Cost. Forward: (M + N) C 4 compulsory bytes per cloud plus N k C 4 gathered bytes, which a kNN graph mostly finds in
// cache (neighbours of neighbouring queries overlap); gf the same with the roles swapped. A hub (a target named by every
// query, in-degree N) is walked by ONE wave: correct, and as slow as N sequential row reads; see DESIGN.md.
#include "nova_internal.h"
#include "pointset_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int NB_MAX_N = NOVA_KNN_MAX_POINTS;  // include/nova_hip.h
constexpr int NB_MAX_K = NOVA_KNN_MAX_K;
constexpr int NB_MAX_C = NOVA_NEIGHBOR_MAX_CHANNELS;
constexpr int NB_T = 256;              // threads per workgroup
constexpr int NB_WAVES = NB_T / 64;    // rows per workgroup of the wave-per-row kernels
constexpr int NB_TILE = 4096;          // indices staged per LDS tile of the inverse walk (16 KiB)
constexpr int NB_Q = 64;               // targets per workgroup of the inverse walk, one per lane
constexpr int NB_SLICES = NB_T / NB_Q; // waves sharing those targets: each walks a quarter of the cloud's edges
constexpr int NB_SLICE_TILE = NB_TILE / NB_SLICES;  // indices per slice and turn
static_assert(NB_MAX_K <= 64, "a row's indices live one per lane");

template <int V> struct nb_vec;
template <> struct nb_vec<1> {
  using type = float;
  static __device__ __forceinline__ float zero() { return 0.f; }
  static __device__ __forceinline__ float div(float a, float b) { return __fdiv_rn(a, b); }
};
template <> struct nb_vec<4> {
  using type = f4v;
  static __device__ __forceinline__ f4v zero() { return f4v{0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ f4v div(f4v a, float b) {
    return f4v{__fdiv_rn(a[0], b), __fdiv_rn(a[1], b), __fdiv_rn(a[2], b), __fdiv_rn(a[3], b)};
  }
};

__device__ __forceinline__ int lane_value(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane));
}

template <int V, bool WEIGHTED>
__global__ __launch_bounds__(NB_T) void neighbor_fwd_kernel(const float* __restrict__ f, const int* __restrict__ idx,
                                                            const float* __restrict__ w, float* __restrict__ out, int N, int M, int k,
                                                            int C) {
  using vec = nb_vec<V>;
  using vt = typename vec::type;
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * NB_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (i >= N) return;
  const size_t row = (size_t)s * N + i;
  int jl = -1;
  float wl = 0.f;
  if (lane < k) {
    jl = idx[row * k + lane];
    if (WEIGHTED) wl = w[row * k + lane];
  }
  const float* fs = f + (size_t)s * M * C;
  float* o = out + row * C;
  const float kf = (float)k;
  for (int c0 = 0; c0 < C; c0 += 64 * V) {  // every lane stays in the loop: the lane reads below need no active lane
    const int c = c0 + lane * V;
    const bool live = c < C;
    // term t of the definition; the next term's load is issued before this one is added (two rows in flight per wave)
    auto term_of = [&](int t) -> vt {
      const int j = lane_value(jl, t);
      const float wt = WEIGHTED ? lane_value(wl, t) : 1.f;
      vt term = vec::zero();  // an index outside 0 .. M-1 is never dereferenced and contributes +0
      if (j >= 0 && j < M && live) {
        term = *reinterpret_cast<const vt*>(fs + (size_t)j * C + c);
        if (WEIGHTED) term = wt * term;
      }
      return term;
    };
    vt acc = term_of(0);
    vt next = k > 1 ? term_of(1) : vec::zero();
    for (int t = 1; t < k; ++t) {
      const vt term = next;
      if (t + 1 < k) next = term_of(t + 1);
      acc = acc + term;
    }
    if (live) *reinterpret_cast<vt*>(o + c) = WEIGHTED ? acc : vec::div(acc, kf);
  }
}

__global__ __launch_bounds__(NB_T) void neighbor_gw_kernel(const float* __restrict__ f, const int* __restrict__ idx,
                                                           const float* __restrict__ g, float* __restrict__ gw, int N, int M, int k,
                                                           int C) {
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * NB_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (i >= N) return;
  const size_t row = (size_t)s * N + i;
  const int jl = lane < k ? idx[row * k + lane] : -1;
  const float* fs = f + (size_t)s * M * C;
  const float* gr = g + row * C;
  float res = 0.f;
  for (int t = 0; t < k; ++t) {
    const int j = lane_value(jl, t);
    float p = 0.f;
    if (j >= 0 && j < M) {  // wave-uniform: all 64 lanes enter wave_sum together
      const float* fr = fs + (size_t)j * C;
      if (lane < C) {
        p = gr[lane] * fr[lane];
        for (int c = lane + 64; c < C; c += 64) p = p + gr[c] * fr[c];
      }
      p = wave_sum(p);
    }
    res = lane == t ? p : res;
  }
  if (lane < k) gw[row * k + lane] = res;
}

template <int V, bool WEIGHTED>
__global__ __launch_bounds__(NB_T) void neighbor_gf_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                           const int* __restrict__ offsets, const int* __restrict__ edges,
                                                           float* __restrict__ gf, int N, int M, int k, int C) {
  using vec = nb_vec<V>;
  using vt = typename vec::type;
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * NB_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (j >= M) return;
  const int E = N * k;
  const int* off = offsets + (size_t)s * (M + 1);
  // a list that is not this idx's inverse must not lead outside g: the segment is cut to 0 .. E and an edge id outside
  // 0 .. E-1 is skipped (it adds +0)
  const int beg = min(max(__builtin_amdgcn_readfirstlane(off[j]), 0), E);
  const int end = min(max(__builtin_amdgcn_readfirstlane(off[j + 1]), beg), E);
  const int* ed = edges + (size_t)s * E;
  const float* ws = WEIGHTED ? w + (size_t)s * E : nullptr;
  const float* gs = g + (size_t)s * N * C;
  float* o = gf + ((size_t)s * M + j) * C;
  const float kf = (float)k;
  for (int c0 = 0; c0 < C; c0 += 64 * V) {
    const int c = c0 + lane * V;
    const bool live = c < C;
    vt acc = vec::zero();  // a target no edge names gets +0
    for (int p0 = beg; p0 < end; p0 += 64) {
      const int cnt = min(64, end - p0);
      int el = -1;
      float wl = 0.f;
      if (lane < cnt) {
        el = ed[p0 + lane];
        if (el < 0 || el >= E) el = -1;
        if (WEIGHTED && el >= 0) wl = ws[el];
      }
      auto term_of = [&](int r) -> vt {
        const int e = lane_value(el, r);
        const float we = WEIGHTED ? lane_value(wl, r) : 1.f;
        vt term = vec::zero();
        if (e >= 0 && live) {
          const vt gv = *reinterpret_cast<const vt*>(gs + (size_t)(e / k) * C + c);
          term = WEIGHTED ? we * gv : vec::div(gv, kf);
        }
        return term;
      };
      vt next = term_of(0);  // cnt >= 1; the next edge's row is loaded before this one is added
      for (int r = 0; r < cnt; ++r) {
        const vt term = next;
        if (r + 1 < cnt) next = term_of(r + 1);
        acc = (p0 == beg && r == 0) ? term : acc + term;
      }
    }
    if (live) *reinterpret_cast<vt*>(o + c) = acc;
  }
}

// The walk both inverse kernels share. A workgroup owns NB_Q = 64 targets, one per lane in all NB_SLICES = 4 waves; wave
// (slice) w takes the quarter [w Q, (w + 1) Q) of the cloud's edge ids, Q = ceil(E / 4) rounded up to a multiple of 4, through
// its own quarter of the LDS tile. Thread (w, lane) meets every index of its quarter equal to j in increasing edge id and
// calls hit(e) for each; the quarters are in increasing e too, so slice by slice a target's edges come in increasing order.
// Every slice runs the same number of turns (the barriers are uniform); the tile is padded with -1, which no target equals.
// BRANCHY: eight indices are tested together before any of them is looked at (the fill pass: a hit is rare and costs a
// store); otherwise every comparison is a plain add (the count pass).
template <bool BRANCHY, typename F>
__device__ __forceinline__ void neighbor_walk(const int* __restrict__ is, int E, int j, int4* tile, F hit) {
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int Q = ((E + NB_SLICES - 1) / NB_SLICES + 3) & ~3;
  const int lo = min(slice * Q, E), hi = min(lo + Q, E);
  int4* mine = tile + slice * (NB_SLICE_TILE / 4);
  for (int t0 = 0; t0 < Q; t0 += NB_SLICE_TILE) {
    const int e0 = lo + t0;
    const int n = max(0, min(NB_SLICE_TILE, hi - e0));
    __syncthreads();  // the previous turn's tile has been read
    for (int q = lane; q < NB_SLICE_TILE; q += 64) reinterpret_cast<int*>(mine)[q] = q < n ? is[e0 + q] : -1;
    __syncthreads();
    const int n8 = (n + 7) / 8;  // pairs of int4; the padding makes the second of a pair readable
    for (int q = 0; q < n8; ++q) {
      const int4 u = mine[2 * q], v = mine[2 * q + 1];
      if (BRANCHY && !((u.x == j) | (u.y == j) | (u.z == j) | (u.w == j) | (v.x == j) | (v.y == j) | (v.z == j) | (v.w == j))) continue;
      const int e = e0 + 8 * q;
      if (u.x == j) hit(e);
      if (u.y == j) hit(e + 1);
      if (u.z == j) hit(e + 2);
      if (u.w == j) hit(e + 3);
      if (v.x == j) hit(e + 4);
      if (v.y == j) hit(e + 5);
      if (v.z == j) hit(e + 6);
      if (v.w == j) hit(e + 7);
    }
  }
}

// offsets[s, j] = the number of edges naming target j (the scan turns the counts into prefix sums in place)
__global__ __launch_bounds__(NB_T) void neighbor_count_kernel(const int* __restrict__ idx, int* __restrict__ offsets, int N, int M,
                                                              int k) {
  __shared__ int4 tile[NB_TILE / 4];
  __shared__ int part[NB_SLICES][NB_Q];
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int j = blockIdx.x * NB_Q + lane;
  const int E = N * k;
  int cnt = 0;
  neighbor_walk<false>(idx + (size_t)s * E, E, j < M ? j : -2, tile, [&](int) { ++cnt; });
  part[slice][lane] = cnt;
  __syncthreads();
  if (slice == 0 && j < M) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < NB_SLICES; ++w) total += part[w][lane];
    offsets[(size_t)s * (M + 1) + j] = total;
  }
}

// one workgroup per cloud: counts [M] -> exclusive prefix sums [M + 1], in place. Thread t owns the chunk t of ceil(M / NB_T)
// consecutive counts; integer sums, so the order does not matter.
__global__ __launch_bounds__(NB_T) void neighbor_scan_kernel(int* __restrict__ offsets, int M) {
  __shared__ int tot[NB_T];
  int* off = offsets + (size_t)blockIdx.x * (M + 1);
  const int tid = threadIdx.x;
  const int chunk = (M + NB_T - 1) / NB_T;
  const int lo = min(tid * chunk, M), hi = min(lo + chunk, M);
  int sum = 0;
  for (int q = lo; q < hi; ++q) sum += off[q];
  tot[tid] = sum;
  __syncthreads();
  int base = 0;
  for (int u = 0; u < tid; ++u) base += tot[u];
  for (int q = lo; q < hi; ++q) {
    const int v = off[q];
    off[q] = base;
    base += v;
  }
  if (tid == NB_T - 1) off[M] = base;  // the last thread's chunk ends at M: base is the total
}

__global__ __launch_bounds__(NB_T) void neighbor_fill_kernel(const int* __restrict__ idx, const int* __restrict__ offsets,
                                                             int* __restrict__ edges, int N, int M, int k) {
  __shared__ int4 tile[NB_TILE / 4];
  __shared__ int part[NB_SLICES][NB_Q];
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int j = blockIdx.x * NB_Q + lane;
  const int E = N * k;
  const bool mine = j < M;
  const int* is = idx + (size_t)s * E;
  // the quarters' counts again: slice w starts at its target's offset plus the counts of the quarters before it
  int cnt = 0;
  neighbor_walk<false>(is, E, mine ? j : -2, tile, [&](int) { ++cnt; });
  part[slice][lane] = cnt;
  __syncthreads();
  const int* off = offsets + (size_t)s * (M + 1);
  int pos = mine ? off[j] : 0;
  for (int w = 0; w < slice; ++w) pos += part[w][lane];
  const int lim = mine ? min(pos + cnt, min(off[j + 1], E)) : 0;  // the segment the count pass sized: nothing is written past it
  int* ed = edges + (size_t)s * E;
  neighbor_walk<true>(is, E, mine ? j : -2, tile, [&](int e) {
    if (pos >= 0 && pos < lim) ed[pos] = e;
    ++pos;
  });
}

// ---- host side -----------------------------------------------------------------------------------------------------------

static bool nb_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the checks the three entries share, in the order include/nova_hip.h states: N, M (and C), k, S
static int nb_shape(const char* who, int S, int N, int M, int k, int C) {
  if (N < 1 || N > NB_MAX_N || M < 1 || M > NB_MAX_N)
    return set_error(NOVA_ERR_SHAPE, "%s: N %d or M %d outside 1 .. %d (NOVA_KNN_MAX_POINTS)", who, N, M, NB_MAX_N);
  if (C < 1 || C > NB_MAX_C) return set_error(NOVA_ERR_SHAPE, "%s: C %d outside 1 .. %d (NOVA_NEIGHBOR_MAX_CHANNELS)", who, C, NB_MAX_C);
  if (k < 1 || k > NB_MAX_K) return set_error(NOVA_ERR_ARG, "%s: k %d outside 1 .. %d (NOVA_KNN_MAX_K)", who, k, NB_MAX_K);
  if (S > 65535) return set_error(NOVA_ERR_SHAPE, "%s: %d clouds exceed one launch (65535)", who, S);
  return 0;
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_neighbor_aggregate(const float* f, const int* idx, const float* w, float* out, int S, int N, int M, int k, int C,
                                     void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_neighbor_aggregate";
  if (const int rc = nb_shape(who, S, N, M, k, C)) return rc;
  if (S <= 0) return 0;
  if (!f || !idx || !out) return set_error(NOVA_ERR_ARG, "%s: null pointer", who);
  const size_t nf = (size_t)S * M * C * 4, ni = (size_t)S * N * k * 4, no = (size_t)S * N * C * 4;
  if (ranges_overlap(out, no, f, nf) || ranges_overlap(out, no, idx, ni) || ranges_overlap(out, no, w, ni))
    return set_error(NOVA_ERR_ARG, "%s: out overlaps an input", who);
  const dim3 grid((N + NB_WAVES - 1) / NB_WAVES, S), block(NB_T);
  const bool v4 = C % 4 == 0 && nb_aligned16(f) && nb_aligned16(out);
  if (w) {
    if (v4) hipLaunchKernelGGL((neighbor_fwd_kernel<4, true>), grid, block, 0, st, f, idx, w, out, N, M, k, C);
    else hipLaunchKernelGGL((neighbor_fwd_kernel<1, true>), grid, block, 0, st, f, idx, w, out, N, M, k, C);
  } else {
    if (v4) hipLaunchKernelGGL((neighbor_fwd_kernel<4, false>), grid, block, 0, st, f, idx, w, out, N, M, k, C);
    else hipLaunchKernelGGL((neighbor_fwd_kernel<1, false>), grid, block, 0, st, f, idx, w, out, N, M, k, C);
  }
  return check_launch(who);
}

int nova_pointset_neighbor_inverse(const int* idx, int* offsets, int* edges, int S, int N, int M, int k, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_neighbor_inverse";
  if (const int rc = nb_shape(who, S, N, M, k, 1)) return rc;
  if (S <= 0) return 0;
  if (!idx || !offsets || !edges) return set_error(NOVA_ERR_ARG, "%s: null pointer", who);
  const size_t ni = (size_t)S * N * k * 4, noff = (size_t)S * (M + 1) * 4;
  if (ranges_overlap(offsets, noff, idx, ni) || ranges_overlap(edges, ni, idx, ni) || ranges_overlap(offsets, noff, edges, ni))
    return set_error(NOVA_ERR_ARG, "%s: offsets or edges overlap idx or each other", who);
  const dim3 grid((M + NB_Q - 1) / NB_Q, S), block(NB_T);
  hipLaunchKernelGGL(neighbor_count_kernel, grid, block, 0, st, idx, offsets, N, M, k);
  hipLaunchKernelGGL(neighbor_scan_kernel, dim3(S), block, 0, st, offsets, M);
  hipLaunchKernelGGL(neighbor_fill_kernel, grid, block, 0, st, idx, offsets, edges, N, M, k);
  return check_launch(who);
}

int nova_pointset_neighbor_aggregate_bwd(const float* f, const int* idx, const float* w, const float* g, const int* offsets,
                                         const int* edges, float* gf, float* gw, int S, int N, int M, int k, int C, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_neighbor_aggregate_bwd";
  if (const int rc = nb_shape(who, S, N, M, k, C)) return rc;
  if (S <= 0) return 0;
  if (!f || !idx || !g) return set_error(NOVA_ERR_ARG, "%s: null pointer", who);
  if (gw && !w) return set_error(NOVA_ERR_ARG, "%s: gw given without w (the mean form has no weights)", who);
  if (!gf && !gw) return set_error(NOVA_ERR_ARG, "%s: gf and gw are both NULL", who);
  if (gf && (!offsets || !edges)) return set_error(NOVA_ERR_ARG, "%s: gf needs the inverse list (offsets, edges)", who);
  const size_t nf = (size_t)S * M * C * 4, ni = (size_t)S * N * k * 4, ng = (size_t)S * N * C * 4, noff = (size_t)S * (M + 1) * 4;
  if (ranges_overlap(gf, nf, f, nf) || ranges_overlap(gf, nf, idx, ni) || ranges_overlap(gf, nf, w, ni) || ranges_overlap(gf, nf, g, ng) ||
      ranges_overlap(gf, nf, offsets, noff) || ranges_overlap(gf, nf, edges, ni) || ranges_overlap(gw, ni, f, nf) ||
      ranges_overlap(gw, ni, idx, ni) || ranges_overlap(gw, ni, w, ni) || ranges_overlap(gw, ni, g, ng) || ranges_overlap(gw, ni, gf, nf))
    return set_error(NOVA_ERR_ARG, "%s: gf or gw overlaps an input or each other", who);
  const dim3 block(NB_T);
  if (gf) {
    const dim3 grid((M + NB_WAVES - 1) / NB_WAVES, S);
    const bool v4 = C % 4 == 0 && nb_aligned16(g) && nb_aligned16(gf);
    if (w) {
      if (v4) hipLaunchKernelGGL((neighbor_gf_kernel<4, true>), grid, block, 0, st, g, w, offsets, edges, gf, N, M, k, C);
      else hipLaunchKernelGGL((neighbor_gf_kernel<1, true>), grid, block, 0, st, g, w, offsets, edges, gf, N, M, k, C);
    } else {
      if (v4) hipLaunchKernelGGL((neighbor_gf_kernel<4, false>), grid, block, 0, st, g, w, offsets, edges, gf, N, M, k, C);
      else hipLaunchKernelGGL((neighbor_gf_kernel<1, false>), grid, block, 0, st, g, w, offsets, edges, gf, N, M, k, C);
    }
  }
  if (gw) hipLaunchKernelGGL(neighbor_gw_kernel, dim3((N + NB_WAVES - 1) / NB_WAVES, S), block, 0, st, f, idx, g, gw, N, M, k, C);
  return check_launch(who);
}

}  // extern "C"
