// Distance-weighted interpolation of a set of clouds: every query point of q [S, T, 3] becomes the average of the values
// v [S, N, C] of ALL source points p [S, N, 3] of its cloud, weighted by softmax(-distance / temperature). It is the
// expensive branch of the reference's adaptive_sampling (diffnext/models/transformers/transformer_pointcloud_nova.py:92-97):
// feature_aware_interpolation, :128-152, which builds torch.cdist [T, N], softmax, and the product
// weights.unsqueeze(-1) * points.unsqueeze(1), an [S, T, N, 3] float tensor (1.3 GB for one 15 000-point cloud at half
// size) that it sums away at once. The definition, and what is left out of that function body (its topk(8) is dead code),
// is in include/nova_hip.h at nova_pointset_kernel_interpolate. Neither the matrix nor the product is ever stored.
//
// The operation is an attention with 3-D keys: scores -d(i, j), values v. It is computed flash-style: a running minimum
// distance, a running weight sum and C running numerators per query in registers. K = 3 is no MFMA shape (knn.hip), so
// the work is plain VALU work on 12-byte points.
//
// Layout: ONE workgroup shape, whatever the launch: 256 threads, 64 queries, one query per lane in all four waves, the
// four waves sharing the sources (SPLIT = 4 of knn.hip; that kernel's 256-query shape is not used, because the order of
// summation is part of the result and must not depend on the batch).
//   1. the workgroup stages a tile of INTERP_TILE = 1024 source points in LDS as (x, y, z, -) float4 and their values as
//      one (C <= 4) or two (C <= 8) float4, unused channels zero: 16 + 16 = 32 or 16 + 32 = 48 KiB. Every lane of a wave reads the same address (a
//      broadcast: one ds_read_b128 per float4, no bank conflicts). With v == NULL the values are the source points and
//      come from the float4 already read (no second array, no second read);
//   2. wave w takes the 64-source chunks w, w + 4, ... of every tile in ascending index order; 1024 is a multiple of 256,
//      so chunk c of the whole cloud always belongs to wave c mod 4;
//   3. per source: d = sqrt(sqdist3) (IEEE square root); on a new minimum, behind a test the wave skips when no lane needs
//      it, the sums are rescaled by exp2((m_new - m_old) scale); then w = exp2((m - d) scale), l += w, a[c] = fma(w, v[c],
//      a[c]). The minimum starts at the distance of the wave's FIRST source (chunk w, read from global memory ahead of
//      the loop) and the sums at zero, so no infinity ever enters the arithmetic: scale == 0 (the plain mean) meets
//      neither inf * 0 nor inf - inf. A wave without a source (N <= 64 w) takes no part in the merge;
//   4. waves 1 .. 3 leave (m, l, a[]) in LDS (the tile array, reused); wave 0 takes the minimum M of the m of the waves
//      that saw a source, then adds the partials in wave order 0 .. 3, each scaled by exp2((M - m_w) scale), and divides
//      (IEEE division).
// The result depends on (q[s], p[s], v[s], C, scale) alone: bitwise the same for every batch, launch split and position
// in the batch. The channel rung (4 or 8 numerators) does not change a channel's operations, so v == NULL equals a copy
// of p passed as v with C = 3 bit for bit.
//
// Cost per (query, source) pair, in vector issue slots of a wave (the compiled loop at C' = 3 has 40 vector instructions
// per source on the path without a rescale): 1 LDS read of the point + 1 or 2 of the values; 3 subtractions, 1 multiply,
// 2 fused multiply-adds (sqdist3); the correctly rounded square root, 17: v_sqrt_f32 at a quarter of the plain rate (4
// slots) inside a scaling for small arguments, two correction steps (2 integer adds, 2 fused multiply-adds, 2 compares,
// 2 selects) and the zero / infinity class test; the minimum test and its wave-wide branch (3); subtract, multiply,
// v_exp_f32 (4 slots, quarter rate), the add to l and C' fused multiply-adds, C' = 3, 4 or 8 numerators: about 43 + C'
// slots, of which the square root is 20. At 32 lanes per SIMD and cycle, 1024 SIMDs and 2.4 GHz that is ~1.7e12 pairs/s
// at C' = 3 and ~1.5e12 at C' = 8. The rescale costs 8 + 2 C' more whenever any of a wave's 64 lanes meets a new
// minimum: about ln(N / 4) times per lane over a cloud in random order, so a few hundred of a wave's N / 4 sources.
#include "interp_common.h"

namespace nova {

constexpr int INTERP_T = 256;      // threads per workgroup
constexpr int INTERP_Q = 64;       // queries per workgroup: one per lane, in every wave
constexpr int INTERP_WAVES = INTERP_T / INTERP_Q;
constexpr int INTERP_TILE = 1024;  // source points staged per LDS tile
constexpr int INTERP_CHUNK = 64;   // consecutive sources one wave takes in turn
constexpr int INTERP_GROUP = 4;    // sources whose reads and distances are issued together
static_assert(INTERP_TILE % (INTERP_WAVES * INTERP_CHUNK) == 0, "chunk ownership is chunk mod 4 across tiles");

// one source at distance d with the values val enters the running state (m, l, a) of a query
template <int CH> __device__ __forceinline__ void interp_step(float& m, float& l, float (&a)[CH], float d, const float (&val)[CH], float scale) {
  const bool lower = d < m;
  // a new minimum: what has been summed so far shrinks by exp2((d - m) scale). The test is on the whole wave (a scalar
  // branch: left as a per-lane `if`, the compiler turns it into selects and pays the second exp2 for every source)
  if (__builtin_amdgcn_ballot_w64(lower) != 0) {
    const float r = interp_weight(d, m, scale);  // of no meaning in the other lanes, which keep their state
    l = lower ? __fmul_rn(l, r) : l;
#pragma unroll
    for (int k = 0; k < CH; ++k) a[k] = lower ? __fmul_rn(a[k], r) : a[k];
    m = lower ? d : m;
  }
  const float w = interp_weight(m, d, scale);
  l += w;
#pragma unroll
  for (int k = 0; k < CH; ++k) a[k] = __builtin_fmaf(w, val[k], a[k]);
}

// CH: numerators kept per query (3: v == NULL, the values are the source points; 4 | 8: explicit values of C <= CH channels)
// STATS: also store the merged minimum M and weight sum L of every query, what the backward (interp_bwd.hip) starts from;
// the scan and the merge are the same code, so out is the same bits with and without
template <int CH, bool STATS>
__global__ __launch_bounds__(INTERP_T) void interp_kernel(const float* __restrict__ q, const float* __restrict__ p,
                                                          const float* __restrict__ v, float* __restrict__ out, float* __restrict__ mo,
                                                          float* __restrict__ lo, int T, int N, int C, float scale, int qblocks) {
  constexpr bool SELF = CH == 3;
  constexpr int VQ = SELF ? 0 : CH / 4;  // float4 of values per source
  constexpr int PART = 2 + CH;           // floats one wave hands over per query
  static_assert((INTERP_WAVES - 1) * PART * INTERP_Q <= INTERP_TILE * 4, "the partials fit the point tile");
  __shared__ f4v ps[INTERP_TILE];  // the source tile during the scan, then the partials of waves 1 .. 3 as [wave - 1][item][query]
  __shared__ f4v vs[SELF ? 1 : INTERP_TILE * VQ];  // [source][VQ]
  float* part = reinterpret_cast<float*>(ps);
  const int t = threadIdx.x;
  const int qi = t % INTERP_Q, wave = t / INTERP_Q;
  const size_t c = blockIdx.x / (unsigned)qblocks;
  const int i = (int)(blockIdx.x % (unsigned)qblocks) * INTERP_Q + qi;
  const float* qc = q + c * (size_t)T * 3;
  const float* pc = p + c * (size_t)N * 3;
  const float* vc = SELF ? nullptr : v + c * (size_t)N * C;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f;  // a lane past the last query works on the origin and stores nothing
  if (i < T) {
    x0 = qc[(size_t)i * 3];
    x1 = qc[(size_t)i * 3 + 1];
    x2 = qc[(size_t)i * 3 + 2];
  }

  // the state starts from the wave's first source: a finite minimum and empty sums
  const int first = wave * INTERP_CHUNK;
  const bool has = first < N;  // wave-uniform
  float m = 0.f, l = 0.f, a[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) a[k] = 0.f;
  if (has) m = interp_dist(x0, x1, x2, pc[(size_t)first * 3], pc[(size_t)first * 3 + 1], pc[(size_t)first * 3 + 2]);

  for (int j0 = 0; j0 < N; j0 += INTERP_TILE) {
    const int cnt = min(INTERP_TILE, N - j0);
    __syncthreads();  // the previous tile has been read by every wave
    for (int j = t; j < cnt; j += INTERP_T) {
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
    for (int b = wave * INTERP_CHUNK; b < cnt; b += INTERP_WAVES * INTERP_CHUNK) {
      const int e = min(b + INTERP_CHUNK, cnt);
      int j = b;
      // INTERP_GROUP sources at a time: their LDS reads and square roots are independent and go ahead of the dependent
      // chain of minimum tests and sums, which takes the sources one by one in index order
      for (; j + INTERP_GROUP <= e; j += INTERP_GROUP) {
        f4v s[INTERP_GROUP];
        float val[INTERP_GROUP][CH], d[INTERP_GROUP];
#pragma unroll
        for (int g = 0; g < INTERP_GROUP; ++g) s[g] = ps[j + g];
#pragma unroll
        for (int g = 0; g < INTERP_GROUP; ++g) interp_values<CH>(val[g], s[g], vs, j + g);
#pragma unroll
        for (int g = 0; g < INTERP_GROUP; ++g) d[g] = interp_dist(x0, x1, x2, s[g][0], s[g][1], s[g][2]);
#pragma unroll
        for (int g = 0; g < INTERP_GROUP; ++g) interp_step<CH>(m, l, a, d[g], val[g], scale);
      }
      for (; j < e; ++j) {
        const f4v s = ps[j];
        float val[CH];
        interp_values<CH>(val, s, vs, j);
        interp_step<CH>(m, l, a, interp_dist(x0, x1, x2, s[0], s[1], s[2]), val, scale);
      }
    }
  }

  __syncthreads();  // every wave is done with the last tile: the point array changes hands
  if (wave > 0) {
    float* mine = part + (wave - 1) * PART * INTERP_Q + qi;
    mine[0] = m;
    mine[INTERP_Q] = l;
#pragma unroll
    for (int k = 0; k < CH; ++k) mine[(2 + k) * INTERP_Q] = a[k];
  }
  __syncthreads();
  if (wave > 0) return;

  // wave 0 always has a source (N >= 1); wave w has one when N > 64 w, the same for every query
  float M = m;
#pragma unroll
  for (int w = 1; w < INTERP_WAVES; ++w)
    if (w * INTERP_CHUNK < N) M = fminf(M, part[(w - 1) * PART * INTERP_Q + qi]);
  const float f0 = interp_weight(M, m, scale);
  l = __fmul_rn(l, f0);
#pragma unroll
  for (int k = 0; k < CH; ++k) a[k] = __fmul_rn(a[k], f0);
#pragma unroll
  for (int w = 1; w < INTERP_WAVES; ++w) {
    if (w * INTERP_CHUNK < N) {
      const float* theirs = part + (w - 1) * PART * INTERP_Q + qi;
      const float f = interp_weight(M, theirs[0], scale);
      l = __builtin_fmaf(theirs[INTERP_Q], f, l);
#pragma unroll
      for (int k = 0; k < CH; ++k) a[k] = __builtin_fmaf(theirs[(2 + k) * INTERP_Q], f, a[k]);
    }
  }
  if (i < T) {
    float* o = out + (c * (size_t)T + i) * (size_t)C;
#pragma unroll
    for (int k = 0; k < CH; ++k)
      if (k < C) o[k] = __fdiv_rn(a[k], l);  // l >= 1: the nearest source of the whole cloud has weight exactly 1
    if (STATS) {
      mo[c * (size_t)T + i] = M;
      lo[c * (size_t)T + i] = l;
    }
  }
}

template <int CH, bool STATS>
static int interp_launch(const char* who, const float* q, const float* p, const float* v, float* out, float* m, float* l, int S, int T, int N,
                         int C, float scale, hipStream_t st) {
  const int qblocks = (T + INTERP_Q - 1) / INTERP_Q;
  const long long blocks = (long long)S * qblocks;
  if (blocks > 0x7fffffffLL) return set_error(NOVA_ERR_SHAPE, "%s: %d clouds of %d queries exceed one launch", who, S, T);
  hipLaunchKernelGGL((interp_kernel<CH, STATS>), dim3((unsigned)blocks), dim3(INTERP_T), 0, st, q, p, v, out, m, l, T, N, C, scale, qblocks);
  return check_launch(who);
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_pointset_kernel_interpolate(const float* q, const float* p, const float* v, float* out, int S, int T, int N, int C, float scale,
                                     void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_kernel_interpolate";
  if (const int rc = interp_check(who, q, p, v, out, S, T, N, C, scale)) return rc;
  if (S <= 0) return 0;
  if (!v) return interp_launch<3, false>(who, q, p, v, out, nullptr, nullptr, S, T, N, C, scale, st);
  if (C <= 4) return interp_launch<4, false>(who, q, p, v, out, nullptr, nullptr, S, T, N, C, scale, st);
  return interp_launch<8, false>(who, q, p, v, out, nullptr, nullptr, S, T, N, C, scale, st);
}

int nova_pointset_kernel_interpolate_stats(const float* q, const float* p, const float* v, float* out, float* m, float* l, int S, int T, int N,
                                           int C, float scale, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* who = "pointset_kernel_interpolate_stats";
  if (const int rc = interp_check(who, q, p, v, out, S, T, N, C, scale)) return rc;
  if (S > 0 && (!m || !l)) return set_error(NOVA_ERR_ARG, "%s: null pointer (m or l)", who);
  if (S <= 0) return 0;
  if (!v) return interp_launch<3, true>(who, q, p, v, out, m, l, S, T, N, C, scale, st);
  if (C <= 4) return interp_launch<4, true>(who, q, p, v, out, m, l, S, T, N, C, scale, st);
  return interp_launch<8, true>(who, q, p, v, out, m, l, S, T, N, C, scale, st);
}

}  // extern "C"
