// What the distance-weighted interpolation (interp.hip) and its backward (interp_bwd.hip) share: the two expressions,
// distance and weight, that both passes must form bit for bit alike (the backward relies on M_i <= d_ij, which holds
// exactly only for the forward's own distance), the read of a source's values from the LDS tile, and the argument
// checks. The definition is in include/nova_hip.h at nova_pointset_kernel_interpolate.
#pragma once
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

__device__ __forceinline__ float interp_dist(float x0, float x1, float x2, float y0, float y1, float y2) {
  return sqrtf(sqdist3(x0, x1, x2, y0, y1, y2));  // correctly rounded (v_sqrt_f32 and two correction steps), as pairwise_dist
}
// exp2((a - b) * scale): a - b <= 0 wherever it is used, so the result is in [0, 1]
__device__ __forceinline__ float interp_weight(float a, float b, float scale) { return __builtin_amdgcn_exp2f(__fmul_rn(a - b, scale)); }

// the values of tile source j: the point itself (CH == 3, from the float4 already read) or CH / 4 float4 of the value tile
template <int CH> __device__ __forceinline__ void interp_values(float (&val)[CH], const f4v& s, const f4v* vs, int j) {
  if (CH == 3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) val[k] = s[k];
  } else {
#pragma unroll
    for (int h = 0; h < CH / 4; ++h) {
      const f4v u = vs[j * (CH / 4) + h];
#pragma unroll
      for (int k = 0; k < 4; ++k) val[4 * h + k] = u[k];
    }
  }
}

// the forward's argument checks, shared by every entry of the family; 0 when they pass
inline int interp_check(const char* who, const float* q, const float* p, const float* v, const float* out, int S, int T, int N, int C,
                        float scale) {
  if (T < 1 || T > NOVA_INTERP_MAX_POINTS || N < 1 || N > NOVA_INTERP_MAX_POINTS)
    return set_error(NOVA_ERR_SHAPE, "%s: T %d or N %d outside 1 .. %d (NOVA_INTERP_MAX_POINTS)", who, T, N, NOVA_INTERP_MAX_POINTS);
  if (C < 1 || C > NOVA_INTERP_MAX_CHANNELS)
    return set_error(NOVA_ERR_SHAPE, "%s: C %d outside 1 .. %d (NOVA_INTERP_MAX_CHANNELS)", who, C, NOVA_INTERP_MAX_CHANNELS);
  if (!v && C != 3) return set_error(NOVA_ERR_ARG, "%s: v == NULL means the values are the source points and needs C == 3, got C %d", who, C);
  NOVA_TRY(check_scale(who, scale));
  if (S > 0 && (!q || !p || !out)) return set_error(NOVA_ERR_ARG, "%s: null pointer", who);
  return 0;
}

}  // namespace nova
