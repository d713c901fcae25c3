// NOVA hot path: the bf16 / head_dim 64 self-attention of attn.hip rebuilt on v_mfma_f32_16x16x32_bf16
//   o = softmax(q k^T * scale) v        (reference diffnext/models/vision_transformer.py:63)
//
// Why a second shape: the four MFMA kernels of the generation path run power-limited; on random
// data the chip holds a higher clock on the 16x16x32 shape than on 32x32x16 at equal cycles per FLOP
// (MI355X_MICROARCH 'DVFS give-back' item 7; tools/mfma_issue_probe.hip at this loop's VALU density: +6 % FLOP/s).
// The 16x16 output block also makes the work per wave a free parameter: NQB 16-query blocks per wave share every K and
// V fragment read from LDS, so NQB = 4 (64 query rows per wave, 256 per workgroup) halves the LDS read bytes per FLOP
// of the NQB = 2 form (32 rows per wave, 128 per workgroup - the geometry of attn.hip).
//
// Same algorithm and semantics as attn_bf16 (attn.hip): S^T = K Q^T so that a query's scores sit on lanes {i, i+16,
// i+32, i+48} x 4 registers per 16-key block; q arrives pre-scaled by scale * log2 e and the running max rides in as the
// C operand of the first MFMA of a score chain (p = exp2(acc)); deferred rescale (only when some query of the wave grew
// by more than 2^8 - and only then is the max reduced across the four lanes of a query: the decision itself needs no
// cross-lane step); the bf16-packed S^T block pair IS the B operand of O^T = V^T P^T (k order inside the 32-key
// contraction: element j < 4 from block 2kp, j >= 4 from block 2kp + 1, and the transposing V read fetches exactly
// those rows); K/V 64-key tiles by LDS-DMA, double buffered, one barrier per tile.
// Workgroup decode, LDS images (Layout16), staging, Q load, fragment reads, key mask and output store: attn_tile.h.
#include <type_traits>
#include "attn_tile.h"
#include "common.h"
#include "nova_internal.h"

namespace nova {

namespace {
constexpr int B_KV = AT_KV, B_T = AT_T64;  // keys per tile, bytes of one 64-wide image

// This file is compiled with -fno-honor-nans (Makefile): in IEEE mode hipcc canonicalises every MFMA result
// before an fmaxf (one extra v_max per score, 16 of the loop's ~90 vector instructions per tile); without it plain
// fmaxf(fmaxf(a, b), c) becomes one v_max3_f32 and the scheduler is free to interleave the chains. The loop produces no
// NaN (masked scores are -inf, and -inf only ever meets finite values).
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
// max of the 16 scores a lane holds for one 16-query block: a depth-3 tree of 8 instructions
__device__ __forceinline__ float max16(const f4v (&s)[4]) {
  const float t0 = max3(s[0][0], s[0][1], s[0][2]), t1 = max3(s[0][3], s[1][0], s[1][1]), t2 = max3(s[1][2], s[1][3], s[2][0]);
  const float t3 = max3(s[2][1], s[2][2], s[2][3]), t4 = max3(s[3][0], s[3][1], s[3][2]);
  return fmaxf(max3(t0, t1, t2), max3(t3, t4, s[3][3]));
}
__device__ __forceinline__ float max_over_g(float x) {  // over lanes {i, i+16, i+32, i+48}
  const uint32_t u = __float_as_uint(x);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float y = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const uint32_t w = __float_as_uint(y);
  const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float sum_over_g(float x) {
  const uint32_t u = __float_as_uint(x);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float y = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const uint32_t w = __float_as_uint(y);
  const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
}  // namespace

// HD = 96 (d48w1536): a 64-wide image plus a 32-wide image (64-byte rows) per K / V tile, as attn.hip, so every LDS-DMA piece
// stays row aligned.
// MASK (the training forward of multi-frame models): a per-query key limit klim[Lq] - query i attends to keys [0, klim[i]), klim
// non-decreasing and >= 1 - which is what the reference's block-causal frame mask is (embeddings.py:247-260: token i sees the tokens
// of frames <= its own; the prefix counts as frame 0). Tiles are then walked in natural order (tile 0 holds an allowed key for
// every row, so the first step's max is finite), every tile applies the limit, and tiles past the workgroup's largest limit are
// never staged.
#ifdef NOVA_CLOCK
// Diagnostic build only (tools/kernel_clock.py): shader cycles and 100 MHz ticks between a workgroup's start and end, kept for the
// last workgroup that used each of 1024 slots (MI355X_MICROARCH.md, 'DVFS give-back' item 6)
__device__ long long g_attn_clock[2 * 1024];
#endif
template <typename E, int HD, int NQB, bool LSE, bool SUMM, bool MASK = false>  // E: bf16_t / f16_t (same loads, LDS images and stores; MFMA form and pair packing differ)
__global__ __launch_bounds__(256, (NQB == 2 && HD == 64) ? 3 : 2) void attn_bf16_m16(
    const E* __restrict__ q, const E* __restrict__ k, const E* __restrict__ v, E* __restrict__ o, int Lq, int Lk, long q_rs, long kv_rs, long o_rs,
    float c, int heads, int nq, int rev, long kv_ss, float* __restrict__ lse, const int* __restrict__ klim = nullptr) {
  constexpr int NDS = HD / 32, NDVB = HD / 16, RW = 16 * NQB, B_T32 = AT_T32, BUF = AT_BUF<HD>;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
#ifdef NOVA_CLOCK
  const long long ck_t0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const AttnWg wg(blockIdx.x, gridDim.x, rev, nq, heads, 4 * RW);
  const int q0 = wg.row0 + wid * RW;
  const E* qb_ = wg.seq(q, (long)Lq * q_rs, HD);
  const E* kb_ = wg.seq(k, kv_ss, HD);
  const E* vb_ = wg.seq(v, kv_ss, HD);

  // Q fragments, B operand of S^T = K Q^T: lane (i, g) holds Q[q0 + 16 qb + i][32 ds + 8 g + 0..7]
  u4v qf[NQB][NDS];
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) load_q<E, 32>(qb_ + (size_t)min(q0 + 16 * qb + i, Lq - 1) * q_rs + 8 * g, c, qf[qb]);

  const KvStage<Layout16, HD> kv(wid, lane, kv_rs);
  auto stage = [&](int buf, int kt) {
    char* lk = smem + buf * BUF;
    kv.stage(kv.tile(kb_, kt), kv.tile(vb_, kt), kv.last_row(Lk, kt), lk, lk + B_T);
  };

  f4v ot[NQB][NDVB], negm[NQB], lacc[NQB];  // lacc (SUMM): row sums of the bf16-rounded P from an all-ones V^T block
  float m_run[NQB], l_run[NQB];
  const u4v ones = {Half16<E>::ONE2, Half16<E>::ONE2, Half16<E>::ONE2, Half16<E>::ONE2};
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    m_run[qb] = 0.f;
    l_run[qb] = 0.f;
    negm[qb] = f4v{0.f, 0.f, 0.f, 0.f};
    lacc[qb] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < NDVB; ++d) ot[qb][d] = f4v{0.f, 0.f, 0.f, 0.f};
  }

  const Read16<HD> rd(lane);

  int kl[NQB];  // MASK: this lane's key limit per query block
  int k_end = Lk;
  if constexpr (MASK) {
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) kl[qb] = min(klim[min(q0 + 16 * qb + i, Lq - 1)], Lk);
    k_end = min(klim[min(wg.row0 + 4 * RW - 1, Lq - 1)], Lk);  // the workgroup's last row has its largest limit
  }
  const int nkt = (k_end + B_KV - 1) / B_KV;
  // Tile order: the (possibly ragged) LAST tile goes first, as a peeled step (softmax does not care about key order), so the
  // steady-state loop carries neither masking code nor the first-tile case, and the compiler is free to run the lane-local
  // max chains under the score MFMAs: step 0 <-> tile nkt - 1, step j >= 1 <-> tile j - 1; K/V of step j in buffer j & 1.
  auto step = [&](auto first, int buf, int tile) {
    constexpr bool FIRST = decltype(first)::value;
    const char* tk = smem + buf * BUF;
    const char* tv = tk + B_T;
    const char* tk32 = tk + 2 * B_T;
    const char* tv32 = tk32 + B_T32;
    // ---- S^T[key][q] - m: 4 key blocks x NQB query blocks, every K fragment feeds NQB MFMAs
    f4v st[NQB][4];
    u4v pb[NQB][2];
    float psum[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) psum[qb] = 0.f;
    // p = exp2(S - m) of the key-block pair kp, packed to 16 bits: the B operand of the P V product
    auto exps = [&](int kp) {
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) {
        u4v packed;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float p0 = __builtin_amdgcn_exp2f(st[qb][2 * kp + h2][2 * j]);
            const float p1 = __builtin_amdgcn_exp2f(st[qb][2 * kp + h2][2 * j + 1]);
            if (!SUMM) psum[qb] += p0 + p1;
            packed[2 * h2 + j] = Half16<E>::pack(p0, p1);
          }
        pb[qb][kp] = packed;
      }
    };
    // O^T[dv][q] += V^T[dv][key] P^T[key][q] for the key-block pair kp (every V fragment feeds NQB MFMAs); SUMM: l += 1 P^T on the same pipe
    auto pv = [&](int kp) {
#pragma unroll
      for (int dvb = 0; dvb < NDVB; ++dvb) {
        const u4v vf = rd.vfrag(tv, kp, dvb, tv32);
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) ot[qb][dvb] = Half16<E>::mfma16(vf, pb[qb][kp], ot[qb][dvb]);
      }
      if (SUMM) {
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) lacc[qb] = Half16<E>::mfma16(ones, pb[qb][kp], lacc[qb]);
      }
    };
    // The d-steps of TWO key blocks are interleaved (and the order prescribed to the scheduler), so that an MFMA never directly follows the one whose
    // result it accumulates on (hipcc's own order put the two d-steps of a score block back to back, with wait states between); K fragment reads
    // run two ahead of their MFMAs. + 0.4-0.6 % (profiles/r04_attn_weave_ab.txt, second part); same operations in the same order per score: bit-identical.
#pragma unroll
    for (int kb2 = 0; kb2 < 4; kb2 += 2) {
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int kb = kb2 + kk;
          const u4v kf = rd.kfrag(tk, kb, ds, tk32);
#pragma unroll
          for (int qb = 0; qb < NQB; ++qb)
            st[qb][kb] = Half16<E>::mfma16(kf, qf[qb][ds], ds == 0 ? negm[qb] : st[qb][kb]);
        }
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // K fragment reads run two ahead of the MFMAs that use them
#pragma unroll
      for (int i = 0; i < 2 * NDS; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, NQB, 0);  // the NQB MFMAs of one K fragment
        if (i < 2 * NDS - 2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one more read
      }
    }
    if constexpr (MASK) {  // every tile: keys at or past the query's limit (which is <= Lk) contribute nothing
      mask_keys16(st, tile, g, [&](int qb) { return kl[qb]; });
    } else if constexpr (FIRST) {
      if ((Lk & (B_KV - 1)) != 0) mask_keys16(st, tile, g, [&](int) { return Lk; });  // ragged tile: keys >= Lk contribute nothing
    }
    // ---- online softmax. Lane-local maxima decide (wave-uniformly) whether anything moves; the reduction across the four
    // lanes of a query only runs inside the branch.
    float mx[NQB], mall = NEG_INF;
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      mx[qb] = max16(st[qb]);
      mall = qb == 0 ? mx[qb] : fmaxf(mall, mx[qb]);
    }
    if (FIRST || __any(mall > 8.0f)) {
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) {
        const float mr = max_over_g(mx[qb]);
        const float delta = FIRST ? mr : fmaxf(mr, 0.f);
        if constexpr (!FIRST) {
          const float alpha = __builtin_amdgcn_exp2f(-delta);
          if (SUMM) lacc[qb] *= alpha;
          else l_run[qb] *= alpha;
#pragma unroll
          for (int d = 0; d < NDVB; ++d) ot[qb][d] *= alpha;
        }
        m_run[qb] += delta;
        negm[qb] = f4v{-m_run[qb], -m_run[qb], -m_run[qb], -m_run[qb]};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) st[qb][kb] -= delta;
      }
    }
#ifndef NOVA_ATTN_NO_WEAVE
    // The exponentials of the second key-block pair are woven into the P V MFMAs of the first (one MFMA, two exponentials, one pack,
    // prescribed to the scheduler): left alone hipcc emits all 32 exponentials, then all 20 MFMAs, and a wave's vector and matrix work
    // overlap only through the SIMD's other waves. Same operations on the same values: bit-identical. Measured (tools/ab_attn.py, one process,
    // -DNOVA_ATTN_NO_WEAVE for the plain order): + 1-2 % at head_dim 64 (L = 2049 .. 2560), + 2.5-3.7 % at head_dim 96, level at L <= 1537;
    // in the benchmark's pass 979-983 -> 999-1000 TFLOP/s on one box (profiles/r04_attn_weave_ab.txt). 137 instead of 122 registers at head_dim 64.
    exps(0);
    __builtin_amdgcn_sched_barrier(0);
    exps(1);
    pv(0);
#pragma unroll
    for (int i = 0; i < NQB * NDVB; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
      __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);  // two exponentials
      __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);  // one pack
    }
    __builtin_amdgcn_sched_barrier(0);
    pv(1);
#else
    exps(0);
    exps(1);
    pv(0);
    pv(1);
#endif
    if (!SUMM) {
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) l_run[qb] += psum[qb];
    }
  };

  auto tile_of = [&](int j) { return MASK ? j : (j == 0 ? nkt - 1 : j - 1); };
  stage(0, tile_of(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA pieces (asm: not counted by the compiler)
  __syncthreads();
  if (nkt > 1) stage(1, tile_of(1));
  step(std::true_type{}, 0, tile_of(0));
  for (int j = 1; j < nkt; ++j) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (j + 1 < nkt) stage((j + 1) & 1, tile_of(j + 1));
    step(std::false_type{}, j & 1, tile_of(j));
  }
  // (Skipping the steps of a wave whose query rows all lie past Lq - `if (q0 < Lq) step(...)`, wave-uniform - was measured and lost at
  // every length, 2 % at L = 2560 where no wave is idle and 24 % at L = 768: the guarded call changes the loop hipcc builds.
  // profiles/r04_attn_dead_wave_skip_rejected.txt)

  // ---- finalize: lane (i, g) holds O[q0 + 16 qb + i][16 dvb + 4 g + 0..3]
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb)
    store_block16<E, NDVB, LSE>(wg, ot[qb], SUMM ? lacc[qb][0] : sum_over_g(l_run[qb]), m_run[qb], q0 + 16 * qb + i, g, o, Lq, o_rs, lse);
#ifdef NOVA_CLOCK
  if (tid == 0) {
    g_attn_clock[2 * (blockIdx.x & 1023)] = __builtin_amdgcn_s_memtime() - ck_t0;
    g_attn_clock[2 * (blockIdx.x & 1023) + 1] = __builtin_amdgcn_s_memrealtime() - ck_r0;
  }
#endif
}


// ------------------------------------------------------------------------------------------------------------------
// Software-pipelined form, 64 query rows per wave: the P V product of tile t-1 shares a basic block with the
// exponentials of tile t, so one wave's matrix work and vector work overlap in its own instruction stream instead of
// relying on the SIMD's other waves (2 per SIMD at this register count). Schedule of iteration t:
//   wait + barrier | stage K(t+1), V(t) | S(t) = K(t) Q^T - m | lane-local max, rare rescale (also of the pending packed
//   P(t-1)) | { p(t) = exp2(S(t)), pack  ||  O += V(t-1) P(t-1), l += 1 P(t-1) }
// V lags K by one tile in the LDS ring (V(t) is staged with K(t+1) and read in iteration t+1), so two buffers suffice.
// Row sums ride on the matrix pipe (all-ones block). Results equal attn_bf16_m16<4, LSE, true> bit for bit.
template <typename E, bool LSE>
__global__ __launch_bounds__(256, 2) void attn_bf16_m16p(const E* __restrict__ q, const E* __restrict__ k,
                                                          const E* __restrict__ v, E* __restrict__ o, int Lq, int Lk,
                                                          long q_rs, long kv_rs, long o_rs, float c, int heads, int nq, int rev,
                                                          long kv_ss, float* __restrict__ lse) {
  constexpr int NQB = 4, HD = 64, NDS = 2, NDVB = 4, RW = 64;
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * B_T + 4 * 64 * 128];  // [buffer][K | V], then the waves' Q rows
  const int tid = threadIdx.x, lane = tid & 63;
#ifdef NOVA_CLOCK
  const long long ck_t0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const AttnWg wg(blockIdx.x, gridDim.x, rev, nq, heads, 4 * RW);
  const int q0 = wg.row0 + wid * RW;
  const E* qb_ = wg.seq(q, (long)Lq * q_rs, HD);
  const E* kb_ = wg.seq(k, kv_ss, HD);
  const E* vb_ = wg.seq(v, kv_ss, HD);

  // The wave's 64 Q rows live in its own 8 KiB of LDS (K's image and swizzle; written once, read back as B fragments at the
  // top of every tile): 32 registers that the exp / P V block of the pipeline needs more than the score block does.
  char* qs = smem + 2 * 2 * B_T + wid * (64 * 128);
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int row = 16 * qb + i;
    const E* qp = qb_ + (size_t)min(q0 + row, Lq - 1) * q_rs + 8 * g;
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) {
      u4v f[1];
      load_q<E, 0>(qp + 32 * ds, c, f);
      *reinterpret_cast<u4v*>(qs + Image<Layout16>::k64(row, 4 * ds + g)) = f[0];
    }
  }

  const KvStage<Layout16, HD> kv(wid, lane, kv_rs);
  // one image (K or V) of tile kt into LDS at dst
  auto stage_k = [&](char* dst, int kt) { kv.stage_k64(kv.tile(kb_, kt), kv.last_row(Lk, kt), dst); };
  auto stage_v = [&](char* dst, int kt) { kv.stage_v64(kv.tile(vb_, kt), kv.last_row(Lk, kt), dst); };

  f4v ot[NQB][NDVB], lacc[NQB];
  float m_run[NQB];
  const u4v ones = {Half16<E>::ONE2, Half16<E>::ONE2, Half16<E>::ONE2, Half16<E>::ONE2};
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    m_run[qb] = 0.f;
    lacc[qb] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < NDVB; ++d) ot[qb][d] = f4v{0.f, 0.f, 0.f, 0.f};
  }
  const Read16<HD> rd(lane);

  const int nkt = (Lk + B_KV - 1) / B_KV;

  // Tile order: the (possibly ragged) LAST tile is processed first, in the prologue, so the steady-state loop carries no
  // masking code at all (softmax does not care about key order): step 0 <-> tile nkt - 1, step j >= 1 <-> tile j - 1.
  // Scores of a step minus the carried max, lane-local max, rescale (FIRST: always, sets m; else rare, and O, l and the
  // pending packed P of the previous step move too). `buf` = LDS buffer of the step's K image.
  auto score_block = [&](auto first, int buf, f4v (&st)[NQB][4], u4v (&pend)[NQB][2]) {
    constexpr bool FIRST = decltype(first)::value;
    const char* tk = smem + buf * 2 * B_T;
    u4v qf[NQB][NDS];
    f4v negm[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) qf[qb][ds] = rd.kfrag(qs, qb, ds);
      float nm = -m_run[qb];
      asm volatile("" : "+v"(nm));  // rebuilt per tile: the 4-register -m block is not carried through the exp / P V block
      negm[qb] = f4v{nm, nm, nm, nm};
    }
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) {
        const u4v kf = rd.kfrag(tk, kb, ds);
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb)
          st[qb][kb] = Half16<E>::mfma16(kf, qf[qb][ds], ds == 0 ? negm[qb] : st[qb][kb]);
      }
    }
    if constexpr (FIRST) {
      if ((Lk & (B_KV - 1)) != 0) mask_keys16(st, nkt - 1, g, [&](int) { return Lk; });  // ragged tile: keys >= Lk contribute nothing
    }
    float mx[NQB], mall = 0.f;
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      mx[qb] = max16(st[qb]);
      mall = qb == 0 ? mx[qb] : fmaxf(mall, mx[qb]);
    }
    if (FIRST || __any(mall > 8.0f)) {
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb) {
        const float mr = max_over_g(mx[qb]);
        const float delta = FIRST ? mr : fmaxf(mr, 0.f);
        if constexpr (!FIRST) {  // everything still at the old max moves exactly once: O, l and the pending P of the previous step
          const float alpha = __builtin_amdgcn_exp2f(-delta);
          lacc[qb] *= alpha;
#pragma unroll
          for (int d = 0; d < NDVB; ++d) ot[qb][d] *= alpha;
#pragma unroll
          for (int kp = 0; kp < 2; ++kp) {
            u4v w = pend[qb][kp];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const f2v t = Half16<E>::unpack(w[e]);
              w[e] = Half16<E>::pack(t[0] * alpha, t[1] * alpha);
            }
            pend[qb][kp] = w;
          }
        }
        m_run[qb] += delta;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) st[qb][kb] -= delta;
      }
    }
  };
  // p = exp2(s), two per v_cvt_pk: the 8 probabilities of (qb, kp) in the B-operand order of the P V product
  auto exp_pack = [&](const f4v (&st)[NQB][4], int qb, int kp) -> u4v {
    u4v packed;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        packed[2 * h2 + j] = Half16<E>::pack(__builtin_amdgcn_exp2f(st[qb][2 * kp + h2][2 * j]), __builtin_amdgcn_exp2f(st[qb][2 * kp + h2][2 * j + 1]));
    return packed;
  };
  // O^T += V^T(tile) P^T for one (kp, dvb): one transposed fragment, NQB MFMAs
  auto pv_step = [&](const char* tv, const u4v (&pend)[NQB][2], int kp, int dvb) {
    const u4v vf = rd.vfrag(tv, kp, dvb);
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) ot[qb][dvb] = Half16<E>::mfma16(vf, pend[qb][kp], ot[qb][dvb]);
  };
  auto sum_step = [&](const u4v (&pend)[NQB][2], int kp) {
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) lacc[qb] = Half16<E>::mfma16(ones, pend[qb][kp], lacc[qb]);
  };

  u4v pbp[NQB][2];  // packed P of the previous step, pending its P V product
  auto tile_of = [&](int step) { return step == 0 ? nkt - 1 : step - 1; };
  // ---- prologue: step 0 (the last tile) up to its packed P. Ring: K(step) in buffer step & 1, V(step) likewise; V lags K
  // by one step (staged with K(step + 1), read during step + 1).
  stage_k(smem, tile_of(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nkt > 1) stage_k(smem + 2 * B_T, tile_of(1));
  stage_v(smem + B_T, tile_of(0));
  {
    f4v st[NQB][4];
    score_block(std::true_type{}, 0, st, pbp);
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) pbp[qb][kp] = exp_pack(st, qb, kp);
  }
  // ---- steady state: this step's scores, then { P V of the previous step || exp2 / pack of this one } as ONE basic block,
  // written interleaved: after each (kp, dvb) fragment's MFMAs comes one (qb, kp) slice of exponentials
  for (int j = 1; j < nkt; ++j) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (j + 1 < nkt) stage_k(smem + ((j + 1) & 1) * 2 * B_T, j);  // tile_of(j + 1) = j
    stage_v(smem + (j & 1) * 2 * B_T + B_T, j - 1);               // tile_of(j) = j - 1
    const char* tv = smem + ((j + 1) & 1) * 2 * B_T + B_T;  // V(step j - 1)
    f4v st[NQB][4];
    score_block(std::false_type{}, j & 1, st, pbp);
    u4v pbn[NQB][2];
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
#pragma unroll
      for (int dvb = 0; dvb < NDVB; ++dvb) {
        pv_step(tv, pbp, kp, dvb);
        const int u = kp * NDVB + dvb;  // 0..7 -> (qb, kp') = (u >> 1, u & 1)
        pbn[u >> 1][u & 1] = exp_pack(st, u >> 1, u & 1);
      }
      sum_step(pbp, kp);
    }
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) { pbp[qb][0] = pbn[qb][0]; pbp[qb][1] = pbn[qb][1]; }
  }
  // ---- epilogue: the last step's P V
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  {
    const char* tv = smem + ((nkt + 1) & 1) * 2 * B_T + B_T;  // V(step nkt - 1)
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
#pragma unroll
      for (int dvb = 0; dvb < NDVB; ++dvb) pv_step(tv, pbp, kp, dvb);
      sum_step(pbp, kp);
    }
  }

#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) store_block16<E, NDVB, LSE>(wg, ot[qb], lacc[qb][0], m_run[qb], q0 + 16 * qb + i, g, o, Lq, o_rs, lse);
#ifdef NOVA_CLOCK
  if (tid == 0) {
    g_attn_clock[2 * (blockIdx.x & 1023)] = __builtin_amdgcn_s_memtime() - ck_t0;
    g_attn_clock[2 * (blockIdx.x & 1023) + 1] = __builtin_amdgcn_s_memrealtime() - ck_r0;
  }
#endif
}

#ifdef NOVA_CLOCK
}  // namespace nova
extern "C" int nova_debug_attn_clock(long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(nova::g_attn_clock), (size_t)(n < 2048 ? n : 2048) * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
namespace nova {
#endif

// head_dim 96 and the masked training forward are built in the shipped form only: 32 rows per wave, row sums on the matrix pipe
template <typename E, bool LSE> static void launch_m16(const AttnFwdArgs& a, const AttnForm& f) {
  if (a.klim) {
    if constexpr (LSE) {
      if (a.hd == 64) attn_launch<E>(attn_bf16_m16<E, 64, 2, true, true, true>, 128, a, a.klim);
      else attn_launch<E>(attn_bf16_m16<E, 96, 2, true, true, true>, 128, a, a.klim);
    }
  } else if (a.hd == 96) attn_launch<E>(attn_bf16_m16<E, 96, 2, LSE, true>, 128, a, a.klim);
  else if (f.pipelined) attn_launch<E>(attn_bf16_m16p<E, LSE>, 256, a);
  else if (f.nqb == 2 && !f.summ) attn_launch<E>(attn_bf16_m16<E, 64, 2, LSE, false>, 128, a, a.klim);
  else if (f.nqb == 2) attn_launch<E>(attn_bf16_m16<E, 64, 2, LSE, true>, 128, a, a.klim);
  else if (!f.summ) attn_launch<E>(attn_bf16_m16<E, 64, 4, LSE, false>, 256, a, a.klim);
  else attn_launch<E>(attn_bf16_m16<E, 64, 4, LSE, true>, 256, a, a.klim);
}

int attn_fwd_m16(const AttnFwdArgs& a, AttnForm f) {
  dispatch_half(a.dtype, [&](auto tag) {
    using E = decltype(tag);
    if (a.lse) launch_m16<E, true>(a, f);
    else launch_m16<E, false>(a, f);
    return 0;
  });
  return check_launch(a.klim ? "attn_fwd_m16 (masked)" : "attn_fwd_m16");
}

}  // namespace nova
