// Device helpers shared by the point-set kernels (pointset, chamfer, emd, occupancy, fps, assign, knn, interp): every result of
// that family is bitwise the same for every batch and launch split, which rests on all of them computing one distance
// expression and summing in one fixed order. Both are defined here once. After them, the two host-side argument checks
// that more than one entry point states in the same words.
#pragma once
#include "nova_internal.h"

namespace nova {

constexpr uint32_t F32_INF_BITS = 0x7f800000u;  // +inf; non-negative floats order as their bit patterns

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax(uint64_t a, uint64_t b) { return a > b ? a : b; }

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// |p - q|^2 in float32, the expression include/nova_hip.h defines for every point-set entry point: three exact-difference
// subtractions, one product rounded to float32 and two fused multiply-adds on top of it, in this order. The roundings
// are WRITTEN OUT (see rope_rotate4 in common.h: left to fp-contract, two kernels inlining the same source line can round
// differently), so the kNN distances, the Chamfer minima, the assignment's costs and pairwise_dist agree bit for bit.
__device__ __forceinline__ float sqdist3(float px, float py, float pz, float qx, float qy, float qz) {
  const float e0 = px - qx, e1 = py - qy, e2 = pz - qz;
  return __builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, __fmul_rn(e0, e0)));
}

// |c| of a clamped point, as the unit-norm point map takes it: a a and c c rounded to float32, b b fused onto a a, the two
// halves added, the square root correctly rounded. Contraction is off for the operators written inside (__fmul_rn and
// __fadd_rn are plain * and + compiled elsewhere, which the pragma does not reach), so the expression is these five
// roundings in every kernel that inlines it.
__device__ __forceinline__ float norm3(float a, float b, float c) {
#pragma clang fp contract(off)
  const float aa = a * a, cc = c * c;
  const float ab = __builtin_fmaf(b, b, aa);
  return sqrtf(ab + cc);
}

// The point map p of nn_dist, nearest_match and its backward: every coordinate clamped to [lo, hi]; unit != 0: then scaled
// by inv = 1 / max(|c|, 1e-8) (distChamfer, train_newloss.py:325-337: x / max(|x|, 1e-8)). The three products are rounded
// to float32 and never fused into a caller's subtraction.
__device__ __forceinline__ void load_point(const float* p, float lo, float hi, int unit, float& a, float& b, float& c) {
#pragma clang fp contract(off)
  a = clampf(p[0], lo, hi);
  b = clampf(p[1], lo, hi);
  c = clampf(p[2], lo, hi);
  if (unit) {
    const float inv = 1.0f / fmaxf(norm3(a, b, c), 1e-8f);
    a = a * inv;
    b = b * inv;
    c = c * inv;
  }
}

// Workgroup sum in a fixed order: wave_sum's pairing inside each wave, then the WAVES waves in index order through one
// LDS slot each. Every thread gets the sum. Earlier code may still be reading red, so a barrier comes first.
template <int WAVES> __device__ __forceinline__ float block_sum_fixed(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  const int t = threadIdx.x;
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  float total = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) total += red[w];
  return total;
}

// ---- host side: each point-set file defines its own extern "C" nova_pointset_* entry points after its kernels, with all of
// their checks in one place (include/nova_hip.h is the contract). Only checks that are the same text everywhere live here.

// do the byte ranges [a, a + na) and [b, b + nb) intersect? A NULL pointer overlaps nothing.
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + nb && b0 < a0 + na;
}

// scale = log2(e) / temperature of the interpolation and the soft clusters: finite and >= 0 (NaN fails); 0 when it passes
inline int check_scale(const char* who, float scale) {
  if (!(scale >= 0.0f && scale <= 3.402823466e+38f))
    return set_error(NOVA_ERR_ARG, "%s: scale %g must be finite and >= 0 (log2(e) / temperature)", who, (double)scale);
  return 0;
}

}  // namespace nova
