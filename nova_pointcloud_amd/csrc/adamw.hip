// Fused AdamW step with in-kernel gradient clipping: what a training step of the reference does after the backward,
// torch.nn.utils.clip_grad_norm_ and then torch.optim.AdamW with betas (0.9, 0.999) (train_newloss.py:827-841, :1060-1082), over
// a LIST of tensors. The definition (every rounding, the chunking and the order of the sum of squares) is in
// include/nova_hip.h at nova_adamw_step; this file is that text as code.
//
//   adamw_sumsq_kernel   one workgroup per (tensor, chunk of NOVA_ADAMW_CHUNK elements): per-thread sums in ascending element
//                        order, a fixed tree through LDS, one plain store of the chunk's partial. No atomics.
//   adamw_total_kernel   one workgroup: the partials as [count, 256], column sums in ascending row order, the same tree; the
//                        total and, where wanted, its correctly rounded square root (the norm) are stored.
//   adamw_step_kernel    one workgroup per (tensor, chunk): each gradient read once, parameter and moments (and the float32
//                        master copy) read and written once, the gradient never written. The clip coefficient is formed by
//                        every thread from the one float32 the sum left on the device: no host round trip.
// The list reaches the kernels BY VALUE, NOVA_ADAMW_BLOCK tensors per launch in the kernel's argument block: no device-side
// table, no copy, no synchronisation, and nothing about a pointer outlives the call. A workgroup finds its tensor by walking
// the block's chunk counts (wave-uniform, at most 32 steps).
// Access: a thread owns units of 8 consecutive elements (unit u of a chunk = elements 8 u .. 8 u + 7, thread t the units
// t, 256 + t, 512 + t, 768 + t). Where every pointer of the tensor is on 16 bytes a whole unit moves in 16-byte accesses
// (two per float32 operand, one per 16-bit one); a unit that the tensor's end cuts, and every unit of a tensor with a
// pointer off 16 bytes, moves element by element. The same element always meets the same arithmetic, so neither alignment nor
// the split of the list over launches changes a bit.
// sqrtf and / below are the correctly rounded ones (the compiler's default for HIP); __fsqrt_rn is NOT, it is the native
// approximation in this toolchain, so it is not used.
#include "fused_common.h"

#pragma clang fp contract(off)  // every rounding below is written out; nothing is fused behind the text

namespace nova {

constexpr int AW_CHUNK = NOVA_ADAMW_CHUNK;  // include/nova_hip.h
constexpr int AW_CAP = NOVA_ADAMW_BLOCK;    // tensors per launch
constexpr int AW_T = 256;                   // threads per workgroup
constexpr int AW_UNIT = 8;                  // consecutive elements a thread handles at a time
constexpr int AW_UNITS = AW_CHUNK / (AW_T * AW_UNIT);
constexpr int AW_PER = NOVA_ADAMW_SUM_COLUMNS;  // columns of the partials' last sum
static_assert(AW_CHUNK == 8192 && AW_PER == 256 && AW_PER == AW_T && AW_UNITS * AW_T * AW_UNIT == AW_CHUNK,
              "the chunk, the columns and the unit walk are part of the definition");
static_assert(sizeof(nova_adamw_tensor) == 80, "the struct is ABI");

struct AwGrad {
  const void* grad;
  int n, dtype;
};
// first[i]: chunks of this launch before tensor i; first[count .. AW_CAP] hold the launch's total, so the walk ends
struct AwSumBlock {
  AwGrad t[AW_CAP];
  int first[AW_CAP + 1];
  float* parts;  // at this launch's first chunk
};
struct AwStepBlock {
  nova_adamw_tensor t[AW_CAP];
  int first[AW_CAP + 1];
  const float* sumsq;
  float max_norm;
};
static_assert(sizeof(AwStepBlock) <= 4096 && sizeof(AwSumBlock) <= 4096, "a block travels in the kernel's argument block");

// the tensor of workgroup b: the last i with first[i] <= b (wave-uniform)
__device__ __forceinline__ int aw_find(const int (&first)[AW_CAP + 1], int b) {
  int i = 0;
  while (i < AW_CAP - 1 && b >= first[i + 1]) ++i;
  return __builtin_amdgcn_readfirstlane(i);
}

// the 8 elements of an aligned whole unit, exactly widened to float32
template <typename T> __device__ __forceinline__ void aw_load8(const T* __restrict__ p, float (&v)[AW_UNIT]) {
  if constexpr (sizeof(T) == 4) {
    const f4v a = *reinterpret_cast<const f4v*>(p), b = *reinterpret_cast<const f4v*>(p + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = a[k], v[4 + k] = b[k];
  } else {
    const u4v r = *reinterpret_cast<const u4v*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f2v h = Half16<T>::unpack(r[k]);
      v[2 * k] = h[0], v[2 * k + 1] = h[1];
    }
  }
}
// and back, each rounded once to nearest even (float32: as they are)
template <typename T> __device__ __forceinline__ void aw_store8(T* __restrict__ p, const float (&v)[AW_UNIT]) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f4v*>(p) = f4v{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f4v*>(p + 4) = f4v{v[4], v[5], v[6], v[7]};
  } else {
    u4v r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = Half16<T>::pack(v[2 * k], v[2 * k + 1]);
    *reinterpret_cast<u4v*>(p) = r;
  }
}

__device__ __forceinline__ bool aw_on16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// s[0] of the 256 values after the tree s[t] = s[t] + s[t + h] for h = 128, 64, .. 1 (t < h), given to thread 0
__device__ __forceinline__ float aw_tree(float v, float* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int h = AW_T / 2; h >= 1; h >>= 1) {
    if (t < h) s[t] = s[t] + s[t + h];
    __syncthreads();
  }
  return s[0];
}

template <typename T> __device__ __forceinline__ float aw_chunk_sumsq(const T* __restrict__ g, long long n, long long c0) {
  const bool wide = aw_on16(g);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < AW_UNITS; ++j) {
    const long long e0 = c0 + (long long)(j * AW_T + (int)threadIdx.x) * AW_UNIT;
    if (wide && e0 + AW_UNIT <= n) {
      float x[AW_UNIT];
      aw_load8<T>(g + e0, x);
#pragma unroll
      for (int k = 0; k < AW_UNIT; ++k) acc = acc + x[k] * x[k];
    } else {
      for (int k = 0; k < AW_UNIT && e0 + k < n; ++k) {  // an element past n - 1 is neither read nor added
        const float x = to_f<T>(g[e0 + k]);
        acc = acc + x * x;
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(AW_T) void adamw_sumsq_kernel(const AwSumBlock blk) {
  __shared__ float red[AW_T];
  const int b = blockIdx.x, i = aw_find(blk.first, b);
  const AwGrad& t = blk.t[i];
  const long long c0 = (long long)(b - blk.first[i]) * AW_CHUNK;
  float acc;
  if (t.dtype == NOVA_BF16) acc = aw_chunk_sumsq<bf16_t>((const bf16_t*)t.grad, t.n, c0);
  else if (t.dtype == NOVA_F16) acc = aw_chunk_sumsq<f16_t>((const f16_t*)t.grad, t.n, c0);
  else acc = aw_chunk_sumsq<float>((const float*)t.grad, t.n, c0);
  const float total = aw_tree(acc, red);
  if (threadIdx.x == 0) blk.parts[b] = total;
}

// the P partials as rows of 256: column n = parts[n] + parts[256 + n] + .. from +0 in ascending order (the loads of SUM_AHEAD
// rows issued together), then the tree over the 256 columns
__global__ __launch_bounds__(AW_T) void adamw_total_kernel(const float* __restrict__ parts, long long P, float* __restrict__ out,
                                                           float* __restrict__ norm) {
  __shared__ float red[AW_T];
  const int n = threadIdx.x;
  float total = 0.f;
  for (long long k0 = n; k0 < P; k0 += (long long)SUM_AHEAD * AW_PER) {
    float v[SUM_AHEAD];
#pragma unroll
    for (int u = 0; u < SUM_AHEAD; ++u) {
      const long long k = k0 + (long long)u * AW_PER;
      v[u] = parts[k < P ? k : k0];
    }
#pragma unroll
    for (int u = 0; u < SUM_AHEAD; ++u) total = k0 + (long long)u * AW_PER < P ? total + v[u] : total;
  }
  const float sum = aw_tree(total, red);
  if (n == 0) {
    *out = sum;
    if (norm) *norm = sqrtf(sum);
  }
}

struct AwNumbers {
  float decay, w1, b2, w2, q, a, eps, s;
  bool clip;
};

// one element: the definition of include/nova_hip.h line by line
__device__ __forceinline__ void aw_update(const AwNumbers& k, float g, float p0, float& m, float& v, float& p) {
  if (k.clip) g = g * k.s;
  const float p1 = p0 * k.decay;
  m = m + k.w1 * (g - m);
  v = v * k.b2 + k.w2 * (g * g);
  const float d = sqrtf(v) / k.q + k.eps;
  p = p1 - k.a * (m / d);
}

template <typename T> __device__ __forceinline__ void aw_chunk_step(const nova_adamw_tensor& t, const AwNumbers& k, long long c0) {
  T* __restrict__ param = (T*)t.param;
  const T* __restrict__ grad = (const T*)t.grad;
  float* __restrict__ em = t.exp_avg;
  float* __restrict__ ev = t.exp_avg_sq;
  float* __restrict__ master = t.master;
  const long long n = t.n;
  const bool wide = aw_on16(param) && aw_on16(grad) && aw_on16(em) && aw_on16(ev) && aw_on16(master);
#pragma unroll
  for (int j = 0; j < AW_UNITS; ++j) {
    const long long e0 = c0 + (long long)(j * AW_T + (int)threadIdx.x) * AW_UNIT;
    if (wide && e0 + AW_UNIT <= n) {
      float g[AW_UNIT], p0[AW_UNIT], m[AW_UNIT], v[AW_UNIT], p[AW_UNIT];
      aw_load8<T>(grad + e0, g);
      aw_load8<float>(em + e0, m);
      aw_load8<float>(ev + e0, v);
      if (master) aw_load8<float>(master + e0, p0);
      else aw_load8<T>(param + e0, p0);
#pragma unroll
      for (int e = 0; e < AW_UNIT; ++e) aw_update(k, g[e], p0[e], m[e], v[e], p[e]);
      aw_store8<float>(em + e0, m);
      aw_store8<float>(ev + e0, v);
      if (master) aw_store8<float>(master + e0, p);
      aw_store8<T>(param + e0, p);
    } else {
      for (int e = 0; e < AW_UNIT && e0 + e < n; ++e) {  // an element past n - 1 is neither read nor written
        const long long i = e0 + e;
        float m = em[i], v = ev[i], p;
        aw_update(k, to_f<T>(grad[i]), master ? master[i] : to_f<T>(param[i]), m, v, p);
        em[i] = m, ev[i] = v;
        if (master) master[i] = p;
        param[i] = from_f<T>(p);
      }
    }
  }
}

__global__ __launch_bounds__(AW_T) void adamw_step_kernel(const AwStepBlock blk) {
  const int b = blockIdx.x, i = aw_find(blk.first, b);
  const nova_adamw_tensor& t = blk.t[i];
  const long long c0 = (long long)(b - blk.first[i]) * AW_CHUNK;
  AwNumbers k{t.decay, t.w1, t.b2, t.w2, t.q, t.a, t.eps, 1.f, blk.sumsq != nullptr};
  if (k.clip) {  // torch's clip_grad_norm_ coefficient; a NaN stays a NaN (torch.clamp's rule)
    const float c = blk.max_norm / (sqrtf(*blk.sumsq) + 1e-6f);
    k.s = c > 1.f ? 1.f : c;
  }
  if (t.dtype == NOVA_BF16) aw_chunk_step<bf16_t>(t, k, c0);
  else if (t.dtype == NOVA_F16) aw_chunk_step<f16_t>(t, k, c0);
  else aw_chunk_step<float>(t, k, c0);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

inline int aw_chunks(long long n) { return (int)((n + AW_CHUNK - 1) / AW_CHUNK); }

// checks 1 .. 5 of the order include/nova_hip.h states, shared by both entries; step: the update's pointers are required too
static int aw_check_list(const char* who, const nova_adamw_tensor* tensors, int count, bool step) {
  NOVA_REQUIRE(count >= 0, NOVA_ERR_ARG, "%s: count %d is negative", who, count);
  NOVA_REQUIRE(count == 0 || tensors, NOVA_ERR_ARG, "%s: null pointer tensors", who);
  for (int i = 0; i < count; ++i) {
    const nova_adamw_tensor& t = tensors[i];
    NOVA_REQUIRE(t.n >= 0 && t.n <= NOVA_ADAMW_MAX_N, NOVA_ERR_ARG, "%s: tensor %d: n %lld outside 0 .. 2^31 - 1", who, i, t.n);
    NOVA_REQUIRE(!bad_dtype(t.dtype), NOVA_ERR_ARG, "%s: tensor %d: unknown dtype code %d (NOVA_F32, NOVA_BF16, NOVA_F16)", who, i, t.dtype);
    if (t.n == 0) continue;
    if (step) NOVA_REQUIRE(t.param, NOVA_ERR_ARG, "%s: tensor %d: null pointer param", who, i);
    NOVA_REQUIRE(t.grad, NOVA_ERR_ARG, "%s: tensor %d: null pointer grad", who, i);
    if (step) {
      NOVA_REQUIRE(t.exp_avg, NOVA_ERR_ARG, "%s: tensor %d: null pointer exp_avg", who, i);
      NOVA_REQUIRE(t.exp_avg_sq, NOVA_ERR_ARG, "%s: tensor %d: null pointer exp_avg_sq", who, i);
    }
  }
  return 0;
}

// The list in blocks of up to AW_CAP tensors with n > 0, in list order: fill(block, slot, tensor) takes each one, and
// launch(block, tensors in it, chunks in it, chunks of the list before it) sends a full block, and the last one, out.
template <typename Block, typename Fill, typename Launch>
static void aw_for_blocks(const nova_adamw_tensor* tensors, int count, Fill&& fill, Launch&& launch) {
  Block blk;
  int used = 0;
  long long before = 0;
  auto flush = [&]() {
    for (int s = used; s < AW_CAP; ++s) blk.first[s + 1] = blk.first[used];
    launch(blk, used, blk.first[used], before);
    before += blk.first[used], used = 0;
  };
  blk.first[0] = 0;
  for (int i = 0; i < count; ++i) {
    if (tensors[i].n == 0) continue;
    fill(blk, used, tensors[i]);
    blk.first[used + 1] = blk.first[used] + aw_chunks(tensors[i].n);  // at most 32 x 2^18 chunks per block
    if (++used == AW_CAP) flush();
  }
  if (used) flush();
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_adamw_sumsq(const nova_adamw_tensor* tensors, int count, float* workspace, long long workspace_floats, float* sumsq,
                     float* norm, void* stream) {
  const char* who = "adamw_sumsq";
  NOVA_TRY(aw_check_list(who, tensors, count, false));
  long long P = 0;
  for (int i = 0; i < count; ++i) P += aw_chunks(tensors[i].n);
  if (P == 0) return 0;
  NOVA_REQUIRE(workspace, NOVA_ERR_ARG, "%s: null pointer workspace", who);
  NOVA_REQUIRE(workspace_floats >= P, NOVA_ERR_ARG, "%s: the workspace holds %lld floats, the list has %lld chunks of %d", who, workspace_floats, P,
               AW_CHUNK);
  NOVA_REQUIRE(sumsq, NOVA_ERR_ARG, "%s: null pointer sumsq", who);
  NOVA_REQUIRE(!ranges_overlap(sumsq, 4, workspace, (size_t)P * 4), NOVA_ERR_ARG, "%s: sumsq overlaps the workspace", who);
  NOVA_REQUIRE(!ranges_overlap(norm, 4, workspace, (size_t)P * 4), NOVA_ERR_ARG, "%s: norm overlaps the workspace", who);
  NOVA_REQUIRE(!ranges_overlap(norm, 4, sumsq, 4), NOVA_ERR_ARG, "%s: norm and sumsq overlap each other", who);
  hipStream_t st = (hipStream_t)stream;
  aw_for_blocks<AwSumBlock>(
      tensors, count, [](AwSumBlock& b, int s, const nova_adamw_tensor& t) { b.t[s] = AwGrad{t.grad, (int)t.n, t.dtype}; },
      [&](AwSumBlock& b, int, int chunks, long long before) {
        b.parts = workspace + before;
        hipLaunchKernelGGL(adamw_sumsq_kernel, dim3((unsigned)chunks), dim3(AW_T), 0, st, b);
      });
  hipLaunchKernelGGL(adamw_total_kernel, dim3(1), dim3(AW_T), 0, st, (const float*)workspace, P, sumsq, norm);
  return check_launch(who);
}

int nova_adamw_step(const nova_adamw_tensor* tensors, int count, const float* sumsq, float max_norm, void* stream) {
  const char* who = "adamw_step";
  NOVA_TRY(aw_check_list(who, tensors, count, true));
  NOVA_REQUIRE(!sumsq || max_norm > 0.f, NOVA_ERR_ARG, "%s: max_norm %g must be > 0 when sumsq is given", who, (double)max_norm);
  hipStream_t st = (hipStream_t)stream;
  bool any = false;
  aw_for_blocks<AwStepBlock>(
      tensors, count, [](AwStepBlock& b, int s, const nova_adamw_tensor& t) { b.t[s] = t; },
      [&](AwStepBlock& b, int, int chunks, long long) {
        b.sumsq = sumsq, b.max_norm = max_norm;
        hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)chunks), dim3(AW_T), 0, st, b);
        any = true;
      });
  return any ? check_launch(who) : 0;
}

}  // extern "C"
