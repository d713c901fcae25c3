// What the fused training ops (posenc, point_embed, point_head, dropout_add, and the sums of soft_cluster) share: the one
// kernel that adds float32 partials in ascending order, and the host-side pieces their entry points state in the same words.
// The argument checks here serve the four files outside the recorded error table (soft_cluster.hip keeps its own texts).
#pragma once
#include "pointset_common.h"

namespace nova {

constexpr int SUM_T = 256;           // threads per workgroup of ordered_sum_kernel
constexpr int SUM_AHEAD = 16;        // partials a thread has in flight (no part of any definition)
constexpr int FEW_WORKGROUPS = 512;  // below two workgroups per compute unit a grid counts as small (likewise)

// grid (ceil(per / 256), groups): element n < per of group s is the sum of parts[(s count + k) per + n] over k = 0 .. count - 1,
// from +0 in ascending k (total + v every time, so a lone -0 comes out as +0). It goes to a[s split + n] for n < split and to
// b[s (per - split) + n - split] after that; an output that is NULL is not formed. The loads of SUM_AHEAD partials are issued
// together (one past count - 1 is made at the group's first index and not used), the additions are made in order. Only
// additions: nothing here can be contracted. One copy per file that includes this (static), each with the same text.
__global__ __launch_bounds__(SUM_T) static void ordered_sum_kernel(const float* __restrict__ parts, float* __restrict__ a, float* __restrict__ b,
                                                                   int count, int per, int split) {
  const int n = blockIdx.x * SUM_T + threadIdx.x;
  if (n >= per) return;
  const size_t s = blockIdx.y;
  const bool first = n < split;
  if (!(first ? a : b)) return;
  const float* mine = parts + s * count * (size_t)per + n;
  float total = 0.f;
  for (int k0 = 0; k0 < count; k0 += SUM_AHEAD) {
    float v[SUM_AHEAD];
#pragma unroll
    for (int u = 0; u < SUM_AHEAD; ++u) v[u] = mine[(size_t)(k0 + u < count ? k0 + u : k0) * per];
#pragma unroll
    for (int u = 0; u < SUM_AHEAD; ++u) total = k0 + u < count ? total + v[u] : total;
  }
  if (first) a[s * (size_t)split + n] = total;
  else b[s * (size_t)(per - split) + (n - split)] = total;
}

// groups <= 65535 (grid.y), which every caller has checked; split == per: everything goes to a
static void ordered_sum(hipStream_t st, const float* parts, float* a, float* b, int groups, int count, int per, int split) {
  hipLaunchKernelGGL(ordered_sum_kernel, dim3((per + SUM_T - 1) / SUM_T, groups), dim3(SUM_T), 0, st, parts, a, b, count, per, split);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// f(integral_constant<int, C>) for the runtime C in 1 .. 8 (the caller has checked the range)
template <typename F> static void dispatch_count8(int C, F&& f) {
  switch (C) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

template <typename F> static void dispatch_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// No output may overlap an input or another output (NULL overlaps nothing). For each output in index order: the inputs in
// index order, then the later outputs; the first overlap found is the error.
inline int check_no_overlap(const char* who, const void* const* outs, const size_t* nouts, const char* const* onames, int n_out,
                            const void* const* ins, const size_t* nins, const char* const* names, int n_in) {
  for (int a = 0; a < n_out; ++a) {
    for (int b = 0; b < n_in; ++b)
      NOVA_REQUIRE(!ranges_overlap(outs[a], nouts[a], ins[b], nins[b]), NOVA_ERR_ARG, "%s: %s overlaps the input %s", who, onames[a], names[b]);
    for (int b = a + 1; b < n_out; ++b)
      NOVA_REQUIRE(!ranges_overlap(outs[a], nouts[a], outs[b], nouts[b]), NOVA_ERR_ARG, "%s: %s and %s overlap each other", who, onames[a], onames[b]);
  }
  return 0;
}
// the same for a single output
inline int check_no_overlap(const char* who, const void* out, size_t nout, const char* oname, const void* const* ins, const size_t* nins,
                            const char* const* names, int n_in) {
  return check_no_overlap(who, &out, &nout, &oname, 1, ins, nins, names, n_in);
}

// A small grid (a single cloud, say) leaves compute units idle and every wave waiting on its own loads: there the channel
// blocks are spread over grid.z, one per workgroup. A block's results do not depend on who computes the others.
inline unsigned few_workgroups_split(int workgroups, int channels, int block) {
  return workgroups < FEW_WORKGROUPS ? (channels + block - 1) / block : 1;
}

}  // namespace nova
