// What the three 16-bit attention forward kernels share, each defined once: attn_bf16 (attn.hip, v_mfma 32x32x16) and
// attn_bf16_m16 / attn_bf16_m16p (attn16.hip, v_mfma 16x16x32). A kernel keeps its own tile loop, softmax and schedule;
// the workgroup decode, the LDS images of a K/V tile (written by LDS-DMA, read as MFMA fragments), the Q fragment load,
// the 16x16 key mask and the 16x16 output store come from here.
#pragma once
#include "common.h"

namespace nova {

constexpr float NEG_INF = -__builtin_huge_valf();
constexpr int AT_KV = 64;              // keys per K/V tile
constexpr int AT_T64 = AT_KV * 128;    // 64-wide image: 128-byte rows, 8 KiB
constexpr int AT_T32 = AT_KV * 64;     // 32-wide image (head_dim 96 only, columns 64 .. 95): 64-byte rows, 4 KiB
template <int HD> constexpr int AT_BUF = 2 * AT_T64 + (HD == 96 ? 2 * AT_T32 : 0);  // one tile: [K64 | V64 | K32 | V32]

// ---- workgroup decode. XCD-aware order: all query tiles of one (sequence, head) are consecutive in the remapped list, so
// they run on one XCD and its K/V is served from that XCD's L2 after the first tile; `rev` walks each XCD's chunk backwards.
struct AttnWg {
  int s, head, qt, heads, row0;  // sequence, head, query tile and its first query row
  __device__ __forceinline__ AttnWg(int bid, int nwg, int rev, int nq, int heads_, int rows_per_wg) : heads(heads_) {
    const int t = xcd_remap_dir(bid, nwg, rev != 0);
    const int sh = t / nq;
    qt = t - sh * nq;
    head = sh % heads;
    s = sh / heads;
    row0 = qt * rows_per_wg;
  }
  // first row of this (sequence, head) in a token-major matrix whose sequences lie seq_stride elements apart
  template <typename E> __device__ __forceinline__ E* seq(E* p, long seq_stride, int HD) const { return p + (size_t)s * seq_stride + head * HD; }
  template <typename E> __device__ __forceinline__ E* out_row(E* o, int Lq, int qrow, long o_rs, int HD) const {
    return o + ((size_t)s * Lq + qrow) * o_rs + head * HD;
  }
  // training: the row's log2-domain log-sum-exp of the scaled scores, what the backward kernels rebuild P from (attn_bwd.hip)
  __device__ __forceinline__ float* lse_row(float* lse, int Lq, int qrow) const { return lse + ((size_t)s * heads + head) * Lq + qrow; }
};

// ---- image layouts. An image holds 16-byte chunk c of row r at chunk c ^ swizzle(r). A layout is the four swizzles; the
// staging offsets (KvStage) and every read offset (Image, Read16) are derived from them, so reads cannot drift from writes.
// 32x32x16: K64 conflict-free for the 32-row ds_read_b128 fragment read, V64 for ds_read_b64_tr_b16; in the 32-wide V image 4
// consecutive 64-byte rows per 32-lane half are one 256-byte bank row, conflict-free as they lie.
struct Layout32 {
  static constexpr uint32_t k64(uint32_t row) { return (row >> 1) & 7; }
  static constexpr uint32_t v64(uint32_t row) { return ((row >> 1) & 1) << 2; }
  static constexpr uint32_t k32(uint32_t row) { return (row >> 2) & 3; }
  static constexpr uint32_t v32(uint32_t) { return 0; }
};
// 16x16x32: K64 conflict-free for the 16-row ds_read_b128 fragment read, V64 for ds_read_b64_tr_b16 over 8 consecutive rows x
// 32 B; K32 chunk ^ s((row >> 2) & 3) with s = (0, 2, 3, 1)
struct Layout16 {
  static constexpr uint32_t k64(uint32_t row) { return (row >> 1) & 7; }
  static constexpr uint32_t v64(uint32_t row) { return ((row >> 1) & 3) << 1; }
  static constexpr uint32_t k32(uint32_t row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }
  static constexpr uint32_t v32(uint32_t row) { return ((row >> 2) & 1) << 1; }
};
// byte offset of chunk `chunk` of row `row` inside an image
template <typename L> struct Image {
  static constexpr uint32_t k64(uint32_t row, uint32_t chunk) { return row * 128u + ((chunk ^ L::k64(row)) << 4); }
  static constexpr uint32_t v64(uint32_t row, uint32_t chunk) { return row * 128u + ((chunk ^ L::v64(row)) << 4); }
  static constexpr uint32_t k32(uint32_t row, uint32_t chunk) { return row * 64u + ((chunk ^ L::k32(row)) << 4); }
  static constexpr uint32_t v32(uint32_t row, uint32_t chunk) { return row * 64u + ((chunk ^ L::v32(row)) << 4); }
};
// true when every swizzle repeats every 16 rows: a lane's offset for row r then serves rows r + 16, r + 32, .. as well
template <typename L> constexpr bool swizzles_repeat_every_16_rows() {
  for (uint32_t r = 0; r + 16 < AT_KV; ++r)
    if (L::k64(r) != L::k64(r + 16) || L::v64(r) != L::v64(r + 16) || L::k32(r) != L::k32(r + 16) || L::v32(r) != L::v32(r + 16)) return false;
  return true;
}

// 8 x 16 bit from two hardware-transposing reads (ds_read_b64_tr_b16): the A operand of O^T += V^T P^T
__device__ __forceinline__ u4v read_tr16_pair(const char* a0, const char* a1) {
  const bf4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf4v*)a0);
  const bf4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf4v*)a1);
  return __builtin_bit_cast(u4v, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- K/V staging: wave w moves LDS-DMA pieces 2w, 2w+1 (8 rows x 128 B each) of the 64-wide K and V images and, for HD = 96,
// piece w (16 rows x 64 B) of the 32-wide ones (source columns 64 .. 95 = byte 128 + 16 * chunk). The swizzle is applied to
// the SOURCE chunk (the LDS side of LDS-DMA is lane-linear). Per-lane byte offsets inside a tile are loop invariant (32-bit)
// and the tile base is a wave-uniform scalar, so a full tile costs no vector address arithmetic; only a ragged tile
// recomputes clamped rows (rows past `lim`, the tile's last valid row, re-read it: their scores are masked to -inf).
template <typename L, int HD> struct KvStage {
  int wid, srow0, srow1, srow32;
  uint32_t rowB, ck0, ck1, cv0, cv1, ck32, cv32, ko0, ko1, vo0, vo1, ko32, vo32;
  __device__ __forceinline__ KvStage(int wid_, int lane, long kv_rs) : wid(wid_), rowB((uint32_t)kv_rs * 2u) {
    const uint32_t scp = lane & 7, scp32 = lane & 3;
    srow0 = (wid * 2) * 8 + (lane >> 3), srow1 = srow0 + 8, srow32 = wid * 16 + (lane >> 2);
    ck0 = (scp ^ L::k64(srow0)) << 4, ck1 = (scp ^ L::k64(srow1)) << 4;
    cv0 = (scp ^ L::v64(srow0)) << 4, cv1 = (scp ^ L::v64(srow1)) << 4;
    ck32 = 128u + ((scp32 ^ L::k32(srow32)) << 4), cv32 = 128u + ((scp32 ^ L::v32(srow32)) << 4);
    ko0 = srow0 * rowB + ck0, ko1 = srow1 * rowB + ck1, vo0 = srow0 * rowB + cv0, vo1 = srow1 * rowB + cv1;
    ko32 = srow32 * rowB + ck32, vo32 = srow32 * rowB + cv32;
  }
  // byte address of tile kt of a K or V matrix (wave-uniform) and the tile's last valid row
  template <typename E> __device__ __forceinline__ const char* tile(const E* rows, int kt) const {
    return reinterpret_cast<const char*>(rows) + (size_t)kt * AT_KV * rowB;
  }
  static __device__ __forceinline__ int last_row(int Lk, int kt) { return Lk - 1 - kt * AT_KV; }
  // K and V of one tile into the buffer whose K64 / V64 images are lk / lv
  __device__ __forceinline__ void stage(const char* kbase, const char* vbase, int lim, char* lk, char* lv) const {
    auto put = [&](uint32_t k0, uint32_t v0, uint32_t k1, uint32_t v1, uint32_t k32, uint32_t v32) {
      glds16(kbase, k0, lk + wid * 2048);
      glds16(vbase, v0, lv + wid * 2048);
      glds16(kbase, k1, lk + wid * 2048 + 1024);
      glds16(vbase, v1, lv + wid * 2048 + 1024);
      if constexpr (HD == 96) {
        glds16(kbase, k32, lk + 2 * AT_T64 + wid * 1024);
        glds16(vbase, v32, lk + 2 * AT_T64 + AT_T32 + wid * 1024);
      }
    };
    if (lim >= AT_KV - 1) {
      put(ko0, vo0, ko1, vo1, ko32, vo32);
    } else {
      const uint32_t r0 = (uint32_t)min(srow0, lim) * rowB, r1 = (uint32_t)min(srow1, lim) * rowB, r32 = (uint32_t)min(srow32, lim) * rowB;
      put(r0 + ck0, r0 + cv0, r1 + ck1, r1 + cv1, r32 + ck32, r32 + cv32);
    }
  }
  // one 64-wide image on its own, always clamped (the pipelined kernel's ring, where V lags K)
  __device__ __forceinline__ void stage_k64(const char* base, int lim, char* dst) const { image64(base, lim, dst, ck0, ck1); }
  __device__ __forceinline__ void stage_v64(const char* base, int lim, char* dst) const { image64(base, lim, dst, cv0, cv1); }
  __device__ __forceinline__ void image64(const char* base, int lim, char* dst, uint32_t c0, uint32_t c1) const {
    glds16(base, (uint32_t)min(srow0, lim) * rowB + c0, dst + wid * 2048);
    glds16(base, (uint32_t)min(srow1, lim) * rowB + c1, dst + wid * 2048 + 1024);
  }
};

// ---- Q fragments: N 16-byte pieces STEP elements apart, multiplied by c when q is not pre-scaled by its producer (c != 1:
// generic nova_attn_fwd callers; the block composites fold scale * log2 e into the fused QKV GEMM epilogue)
template <typename E, int STEP, int N> __device__ __forceinline__ void load_q(const E* qp, float c, u4v (&qf)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) qf[n] = *reinterpret_cast<const u4v*>(qp + STEP * n);
  if (c != 1.0f) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f2v t = Half16<E>::unpack(qf[n][j]);
        qf[n][j] = Half16<E>::pack(t[0] * c, t[1] * c);
      }
  }
}

// ---- the 16x16x32 kernels' side (lane = 16 g + i; a query's scores sit on lanes {i, i+16, i+32, i+48} x 4 registers per key block)
// Lane constants of their two read kinds. K fragment of key block kb at d-step ds: rows 16 kb + i, chunk 4 ds + g (d-step 2 =
// the 32-wide image, chunk g). Transposing V read of key-block pair kp for output block dvb: lane 4 q + p of each 16-lane
// group supplies row 32 kp + 4 g + q (and + 16), columns 16 dvb + 4 p .. 4 p + 3.
template <int HD> struct Read16 {
  static_assert(swizzles_repeat_every_16_rows<Layout16>(), "one offset per lane serves every key block");
  using I = Image<Layout16>;
  uint32_t koff[HD / 32], voff[HD / 16];
  __device__ __forceinline__ explicit Read16(int lane) {
    const uint32_t i = lane & 15, g = lane >> 4, t_q = (lane & 15) >> 2, t_p = lane & 3, vrow = 4 * g + t_q;
    koff[0] = I::k64(i, g), koff[1] = I::k64(i, g + 4u);
    if constexpr (HD == 96) koff[2] = I::k32(i, g);
#pragma unroll
    for (int dvb = 0; dvb < HD / 16; ++dvb)
      voff[dvb] = (dvb < 4 ? I::v64(vrow, 2 * dvb + (t_p >> 1)) : I::v32(vrow, 2 * (dvb - 4) + (t_p >> 1))) + 8u * (t_p & 1);
  }
  __device__ __forceinline__ u4v kfrag(const char* tk, int kb, int ds, const char* tk32 = nullptr) const {  // tk32 / tv32: the 32-wide images (HD = 96)
    return ds < 2 ? *reinterpret_cast<const u4v*>(tk + kb * 2048 + koff[ds]) : *reinterpret_cast<const u4v*>(tk32 + kb * 1024 + koff[HD / 32 - 1]);
  }
  __device__ __forceinline__ u4v vfrag(const char* tv, int kp, int dvb, const char* tv32 = nullptr) const {
    const char* a0 = dvb < 4 ? tv + kp * 4096 + voff[dvb] : tv32 + kp * 2048 + voff[dvb];
    return read_tr16_pair(a0, a0 + (dvb < 4 ? 2048 : 1024));
  }
};

// keys at or past a query block's limit contribute nothing: register r of key block kb on lane (i, g) is key
// tile * 64 + 16 kb + 4 g + r; limit(qb) = Lk for a ragged last tile, the lane's per-query key limit under a mask
template <int NQB, typename F> __device__ __forceinline__ void mask_keys16(f4v (&st)[NQB][4], int tile, int g, F limit) {
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = tile * AT_KV + 16 * kb + 4 * g + r;
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb)
        if (key >= limit(qb)) st[qb][kb][r] = NEG_INF;  // (as a select, `key < limit ? s : -inf`: 8 .. 21 VGPRs more in attn_bf16_m16 at head_dim 64)
    }
}

// one 16-query block out: lane (i, g) holds O[qrow][16 dvb + 4 g + 0..3] unnormalised, l_tot the row's sum, m its running max
template <typename E, int NDVB, bool LSE>
__device__ __forceinline__ void store_block16(const AttnWg& wg, const f4v (&ot)[NDVB], float l_tot, float m, int qrow, int g, E* o, int Lq,
                                              long o_rs, float* lse) {
  const float inv = 1.0f / l_tot;
  if (qrow < Lq) {
    if (LSE && g == 0) *wg.lse_row(lse, Lq, qrow) = m + __log2f(l_tot);
    E* op = wg.out_row(o, Lq, qrow, o_rs, 16 * NDVB) + 4 * g;
#pragma unroll
    for (int dvb = 0; dvb < NDVB; ++dvb) {
      u2v pk = {Half16<E>::pack(ot[dvb][0] * inv, ot[dvb][1] * inv), Half16<E>::pack(ot[dvb][2] * inv, ot[dvb][3] * inv)};
      *reinterpret_cast<u2v*>(op + 16 * dvb) = pk;
    }
  }
}

}  // namespace nova
