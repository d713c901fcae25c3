// Optimal assignment between two clouds of n points each: the earth mover's distance of compute_emd_distance
// (test_optimize.py:385-415) and emd_approx (train_newloss.py:352-372), which the reference and, until now, this project
// solve with scipy's linear_sum_assignment on the host from a [n, n] cost matrix. Here it is a batched Jacobi auction
// (Bertsekas) with epsilon scaling in exact integer arithmetic, one workgroup per cloud pair. The integer scheme, the tie
// rules and the outputs are the contract written out in include/nova_hip.h at nova_pointset_assignment; this file is how
// it runs.
//
// Nothing of size n^2 exists anywhere: a cost c(i, j) is recomputed from the two points whenever it is needed (three
// subtractions, a product, two fused multiply-adds, one correctly rounded square root: the float32 expression of
// pairwise_dist_kernel in pointset.hip, so device and host path see the same float32 costs).
//
// LDS per pair (36 B per point of capacity NP): the y cloud as three float arrays, one 64-bit word per column, one 64-bit
// bid slot per column, the row -> column table and the list of unassigned rows.
//   column word  key[j] = price[j] << 13 | (8191 - owner[j])     low 13 bits 0: no owner
//   bid slot     bid << 13 | (8191 - row)                        0: no bid this round
// A bid always exceeds the price it was computed from (epsilon >= 1), so the winning bid slot simply becomes the column
// word. The bid slots take LDS 64-bit unsigned maxima (ds_max_u64): the keys of one round are unique (a row bids once),
// and a maximum of unique keys has one value in whatever order the waves arrive. Highest bid wins, lowest row on ties.
//
// One round, three workgroup barriers:
//   1. compaction: every thread looks at its rows; the unassigned ones go to list[] (wave ballot, one LDS add per wave
//      for the base; the ORDER of the list depends on wave timing, the SET does not, and nothing below depends on order);
//   2. bidding: a wave takes a listed row at a time, its lanes stride the columns. A lane folds the packed keys
//      (C(i, j) + price[j]) << 13 | j  into its two smallest; the wave merges the pairs of minima on the DPP / permlane
//      pairing of common.h (wave_combine). Keys are unique in j, so the smallest is the best column with value ties going
//      to the lowest j, and the second smallest carries the second-best value. Lane 0 posts the bid. Bids are computed
//      from the column words as they stood at the start of the round: nothing writes them during this step (Jacobi);
//   3. merge: every thread looks at its columns; a column with a bid evicts its owner, takes the bid as its word and
//      records the new owner. Evicted rows were assigned and did not bid; winners were unassigned: the writes are disjoint.
// When the list comes out empty the phase is over: epsilon == 1 ends the auction, otherwise epsilon /= 8, every owner is
// cleared and the prices stay.
//
// A launch runs at most `rounds` rounds and then stores the column words, the row table, epsilon, the rounds used and the
// done flag to the caller's state buffer; the next launch picks up from there and is bitwise the continuation (the state
// is complete and every step is a function of it alone). Phase changes are bounded by the 14 divisions that take any
// first epsilon to 1, so no loop in here depends on the data for its end.
//
// Capacity forms by point count (assign_config below), workgroup size T and capacity NP:
//   n <= 64: 64 / 64 (one wave)   <= 256: 256 / 256   <= 1024: 256 / 1024   <= 2048: 512 / 2048   <= 4096: 1024 / 4096
#include "nova_internal.h"
#include "pointset_common.h"

namespace nova {

constexpr int ASSIGN_MAX_N = NOVA_ASSIGN_MAX_POINTS;  // include/nova_hip.h
constexpr int ASSIGN_SCALE_LOG2 = 18;                 // the quantum 2^-18 of the header
constexpr int ASSIGN_ROW_BITS = 13;                   // rows 0 .. 4095 and the "no owner" code fit with room
constexpr uint64_t ASSIGN_ROW_MASK = (1ull << ASSIGN_ROW_BITS) - 1;
constexpr uint64_t ASSIGN_NONE = ~0ull;
// bit budget: costs < 2^43 (diagonal < 4096, times 2^18, times n + 1 <= 2^12 + 1), bids < 2^49, so C + price < 2^50 and
// every packed key < 2^63
constexpr float ASSIGN_MAX_DIAGONAL = 4096.f;
constexpr int64_t ASSIGN_BID_LIMIT = 1ll << 49;
constexpr int ASSIGN_HEADER_BYTES = 32;

struct AssignHeader {
  long long eps;
  int rounds_used;
  int done;  // 0 running, 1 done, -1 out of range (NOVA_ASSIGN_RANGE)
  int pad[4];
};
static_assert(sizeof(AssignHeader) == ASSIGN_HEADER_BYTES, "state header");

static size_t assign_state_bytes(int n) { return ((size_t)ASSIGN_HEADER_BYTES + 12 * (size_t)n + 15) & ~(size_t)15; }

template <int NP> struct AssignShared {
  uint64_t key[NP];
  uint64_t bid[NP];
  float yx[NP], yy[NP], yz[NP];
  int col_of_row[NP];
  int list[NP];
  float red[6][16];
  unsigned cnt;
  int err;
};

// a 64-bit key moved as its two halves
template <int CTRL> __device__ __forceinline__ uint64_t assign_dpp(uint64_t v) {
  const uint32_t lo = dpp_move<CTRL>((uint32_t)v), hi = dpp_move<CTRL>((uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}
// the two smallest of the union of two pairs (m1 < m2 within a pair; all keys distinct except the ASSIGN_NONE padding)
__device__ __forceinline__ void assign_merge(uint64_t& m1, uint64_t& m2, uint64_t p1, uint64_t p2) {
  const uint64_t lo = umin(m1, p1), hi = umax(m1, p1);
  m2 = umin(hi, umin(m2, p2));
  m1 = lo;
}
template <int CTRL> __device__ __forceinline__ void assign_merge_dpp(uint64_t& m1, uint64_t& m2) {
  const uint64_t p1 = assign_dpp<CTRL>(m1), p2 = assign_dpp<CTRL>(m2);
  assign_merge(m1, m2, p1, p2);
}
// v_permlane{16,32}_swap of a value with itself: both partners end with both values
template <bool HALVES> __device__ __forceinline__ void assign_swap(uint64_t v, uint64_t& a, uint64_t& b) {
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  const auto rl = HALVES ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false) : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto rh = HALVES ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false) : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  a = (uint64_t)rh[0] << 32 | rl[0];
  b = (uint64_t)rh[1] << 32 | rl[1];
}
template <bool HALVES> __device__ __forceinline__ void assign_merge_swap(uint64_t& m1, uint64_t& m2) {
  uint64_t a1, b1, a2, b2;
  assign_swap<HALVES>(m1, a1, b1);
  assign_swap<HALVES>(m2, a2, b2);
  m1 = a1;
  m2 = a2;
  assign_merge(m1, m2, b1, b2);
}
// every lane ends with the wave's two smallest keys, on the pairing of wave_combine
__device__ __forceinline__ void assign_wave_min2(uint64_t& m1, uint64_t& m2) {
  assign_merge_dpp<0x141>(m1, m2);
  assign_merge_dpp<0xb1>(m1, m2);
  assign_merge_dpp<0x4e>(m1, m2);
  assign_merge_dpp<0x140>(m1, m2);
  assign_merge_swap<false>(m1, m2);
  assign_merge_swap<true>(m1, m2);
}

__device__ __forceinline__ float assign_clamp(float v, float lo, float hi, int use) { return use ? clampf(v, lo, hi) : v; }

// the float32 cost of the header, as pairwise_dist_kernel (pointset.hip) computes it: sqdist3 and a correctly rounded square root
__device__ __forceinline__ float assign_dist(float ax, float ay, float az, float bx, float by, float bz) {
  return sqrtf(sqdist3(ax, ay, az, bx, by, bz));
}
// llrint(c * 2^18): the product is exact (a power of two), rintf rounds to nearest even, and c < 4097 keeps it in int32
__device__ __forceinline__ int64_t assign_quantise(float c) { return (int64_t)(int)__builtin_rintf(c * (float)(1 << ASSIGN_SCALE_LOG2)); }

template <int T, int NP>
__global__ __launch_bounds__(T) void assign_kernel(const float* __restrict__ x, const float* __restrict__ y, int* __restrict__ col_out,
                                                   float* __restrict__ cost_out, char* __restrict__ state, size_t state_stride, int n,
                                                   float lo, float hi, int use_clamp, int rounds, int restart, int* __restrict__ all_done) {
  constexpr int W = T / 64;
  static_assert(NP % T == 0 && W >= 1 && W <= 16, "shape");
  __shared__ AssignShared<NP> s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t b = blockIdx.x;
  AssignHeader* hdr = (AssignHeader*)(state + b * state_stride);
  uint64_t* g_key = (uint64_t*)(state + b * state_stride + ASSIGN_HEADER_BYTES);
  int* g_col = (int*)(g_key + n);
  if (!restart) {
    const int was = hdr->done;  // the same word in every thread: a finished pair leaves at once
    if (was != 0) {
      if (was < 0 && t == 0) atomicMin(all_done, -1);
      return;
    }
  }
  const float* xb = x + b * (size_t)n * 3;
  const float* yb = y + b * (size_t)n * 3;
  const int64_t n1 = n + 1;

  // the y cloud, clamped, into LDS; the state from the buffer, or a fresh one
  float mn[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
  float mx[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
  for (int i = t; i < NP; i += T) {
    const bool ok = i < n;
    float q[3] = {0.f, 0.f, 0.f};
    if (ok) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        q[k] = assign_clamp(yb[(size_t)i * 3 + k], lo, hi, use_clamp);
        if (restart) {
          const float p = assign_clamp(xb[(size_t)i * 3 + k], lo, hi, use_clamp);
          mn[k] = fminf(mn[k], fminf(p, q[k]));
          mx[k] = fmaxf(mx[k], fmaxf(p, q[k]));
        }
      }
    }
    s.yx[i] = q[0];
    s.yy[i] = q[1];
    s.yz[i] = q[2];
    s.key[i] = (ok && !restart) ? g_key[i] : 0ull;
    s.col_of_row[i] = (ok && !restart) ? g_col[i] : -1;
    s.bid[i] = 0ull;
  }
  if (t == 0) {
    s.cnt = 0u;
    s.err = 0;
  }
  int64_t eps;
  int used = 0;
  if (restart) {
    // first epsilon from the bounding box of both clamped clouds: every cost is at most its diagonal (no n^2 pass)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mn[k] = wave_combine(mn[k], [](float a, float c) { return fminf(a, c); });
      mx[k] = wave_combine(mx[k], [](float a, float c) { return fmaxf(a, c); });
      if (lane == 0) {
        s.red[k][wave] = mn[k];
        s.red[3 + k][wave] = mx[k];
      }
    }
    __syncthreads();
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float a = s.red[k][0], c = s.red[3 + k][0];
      for (int w = 1; w < W; ++w) {
        a = fminf(a, s.red[k][w]);
        c = fmaxf(c, s.red[3 + k][w]);
      }
      d2 = __builtin_fmaf(c - a, c - a, d2);
    }
    const float diag = sqrtf(d2);
    if (!(diag < ASSIGN_MAX_DIAGONAL)) {  // also catches a NaN or an infinity in the input
      if (t == 0) {
        hdr->eps = 0;
        hdr->rounds_used = 0;
        hdr->done = -1;
        cost_out[b] = -2.f;
        atomicMin(all_done, -1);
      }
      return;
    }
    const int64_t bound = (assign_quantise(diag) + 1) * n1;
    eps = bound / 4 > 1 ? bound / 4 : 1;
  } else {
    eps = hdr->eps;
    used = hdr->rounds_used;
  }
  __syncthreads();

  int done = 0;
  for (int round = 0;;) {
    // 1. compaction of the unassigned rows
    for (int i0 = 0; i0 < NP; i0 += T) {
      const int i = i0 + t;
      const bool un = i < n && s.col_of_row[i] < 0;
      const uint64_t mask = __ballot(un);
      if (mask != 0ull) {  // wave-uniform
        unsigned base = 0u;
        if (lane == 0) base = atomicAdd(&s.cnt, (unsigned)__popcll(mask));
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (un) s.list[base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = i;
      }
    }
    __syncthreads();
    const int cnt = (int)s.cnt;
    if (cnt == 0) {
      if (eps == 1) {
        done = 1;
        break;
      }
      // next phase: a smaller epsilon, every owner cleared, the prices kept
      eps = eps / 8 > 1 ? eps / 8 : 1;
      for (int i = t; i < n; i += T) {
        s.key[i] &= ~ASSIGN_ROW_MASK;
        s.col_of_row[i] = -1;
      }
      __syncthreads();
      continue;  // at most 14 times from any first epsilon: no round is spent, and the loop still ends
    }
    if (round == rounds) break;

    // 2. bidding: one row per wave at a time
    for (int k = wave; k < cnt; k += W) {
      const int i = __builtin_amdgcn_readfirstlane(s.list[k]);
      const float px = assign_clamp(xb[(size_t)i * 3], lo, hi, use_clamp);
      const float py = assign_clamp(xb[(size_t)i * 3 + 1], lo, hi, use_clamp);
      const float pz = assign_clamp(xb[(size_t)i * 3 + 2], lo, hi, use_clamp);
      uint64_t m1 = ASSIGN_NONE, m2 = ASSIGN_NONE;
      for (int j = lane; j < n; j += 64) {
        const int64_t c = assign_quantise(assign_dist(px, py, pz, s.yx[j], s.yy[j], s.yz[j])) * n1;
        const uint64_t a = ((uint64_t)c + (s.key[j] >> ASSIGN_ROW_BITS)) << ASSIGN_ROW_BITS | (uint64_t)j;
        m2 = umin(m2, umax(m1, a));
        m1 = umin(m1, a);
      }
      assign_wave_min2(m1, m2);
      if (lane == 0) {
        const int js = (int)(m1 & ASSIGN_ROW_MASK);
        const int64_t best = (int64_t)(m1 >> ASSIGN_ROW_BITS);
        const int64_t second = m2 == ASSIGN_NONE ? best : (int64_t)(m2 >> ASSIGN_ROW_BITS);  // n == 1
        const int64_t bidv = (int64_t)(s.key[js] >> ASSIGN_ROW_BITS) + (second - best) + eps;
        if (bidv >= ASSIGN_BID_LIMIT)
          s.err = 1;  // the key's bit budget: reported, never wrapped
        else
          __hip_atomic_fetch_max(&s.bid[js], (uint64_t)bidv << ASSIGN_ROW_BITS | (ASSIGN_ROW_MASK - (uint64_t)i), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    __syncthreads();
    if (s.err) {
      done = -1;
      break;
    }

    // 3. merge: the columns take their highest bid
    for (int j = t; j < n; j += T) {
      const uint64_t nb = s.bid[j];
      if (nb != 0ull) {
        const uint64_t old = s.key[j] & ASSIGN_ROW_MASK;
        if (old != 0ull) s.col_of_row[(int)(ASSIGN_ROW_MASK - old)] = -1;
        s.col_of_row[(int)(ASSIGN_ROW_MASK - (nb & ASSIGN_ROW_MASK))] = j;
        s.key[j] = nb;
        s.bid[j] = 0ull;
      }
    }
    if (t == 0) s.cnt = 0u;  // every thread read it before the barrier above
    ++round;
    ++used;
    __syncthreads();
  }

  // state back to the caller's buffer; the outputs of a finished pair
  for (int i = t; i < n; i += T) {
    g_key[i] = s.key[i];
    g_col[i] = s.col_of_row[i];
  }
  if (t == 0) {
    hdr->eps = eps;
    hdr->rounds_used = used;
    hdr->done = done;
    if (done < 0) cost_out[b] = -2.f;
    if (done == 0 && restart) cost_out[b] = -1.f;
    if (done <= 0) atomicMin(all_done, done);
  }
  if (done == 1) {
    // the mean matched distance in a fixed order: a thread's rows in index order, then block_sum_fixed's order (wave_sum's
    // pairing, the waves in index order) with thread 0 alone reading the slots, one division
    float sum = 0.f;
    for (int i = t; i < NP; i += T) {
      float c = 0.f;
      if (i < n) {
        const int j = s.col_of_row[i];
        col_out[b * (size_t)n + i] = j;
        c = assign_dist(assign_clamp(xb[(size_t)i * 3], lo, hi, use_clamp), assign_clamp(xb[(size_t)i * 3 + 1], lo, hi, use_clamp),
                        assign_clamp(xb[(size_t)i * 3 + 2], lo, hi, use_clamp), s.yx[j], s.yy[j], s.yz[j]);
      }
      sum += c;
    }
    sum = wave_sum(sum);
    __syncthreads();  // s.red was last read before the first barrier of the main loop; kept apart all the same
    if (lane == 0) s.red[0][wave] = sum;
    __syncthreads();
    if (t == 0) {
      float total = s.red[0][0];
      for (int w = 1; w < W; ++w) total += s.red[0][w];
      cost_out[b] = total / (float)n;
    }
  }
}

__global__ void assign_flag_kernel(int* flag, int v) { *flag = v; }

__global__ void assign_rounds_kernel(const char* __restrict__ state, size_t state_stride, int* __restrict__ out, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) out[b] = ((const AssignHeader*)(state + (size_t)b * state_stride))->rounds_used;
}

// Capacity form by point count: (T, NP) with NP >= n. tests/test_pointset_assignment.py restates the boundaries.
template <int T, int NP>
static void assign_launch(const float* x, const float* y, int* col, float* cost, void* state, int B, int n, float lo, float hi,
                          int use_clamp, int rounds, int restart, int* all_done, hipStream_t st) {
  hipLaunchKernelGGL((assign_kernel<T, NP>), dim3((unsigned)B), dim3(T), 0, st, x, y, col, cost, (char*)state, assign_state_bytes(n), n,
                     lo, hi, use_clamp, rounds, restart, all_done);
}

}  // namespace nova

using namespace nova;

extern "C" {

long long nova_pointset_assignment_state_bytes(int n) { return n >= 1 && n <= ASSIGN_MAX_N ? (long long)assign_state_bytes(n) : 0; }

int nova_pointset_assignment(const float* x, const float* y, int* col, float* cost, void* state, int B, int n, float lo, float hi,
                             int use_clamp, int rounds, int restart, int* all_done, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (n < 1 || n > ASSIGN_MAX_N)
    return set_error(NOVA_ERR_ARG, "pointset_assignment: n %d outside 1 .. %d (NOVA_ASSIGN_MAX_POINTS)", n, ASSIGN_MAX_N);
  if (rounds < 1) return set_error(NOVA_ERR_ARG, "pointset_assignment: rounds %d < 1", rounds);
  if (use_clamp && !(lo <= hi)) return set_error(NOVA_ERR_ARG, "pointset_assignment: empty clamp range");
  if (!all_done) return set_error(NOVA_ERR_ARG, "pointset_assignment: null pointer");
  if (B > 0 && (!x || !y || !col || !cost || !state)) return set_error(NOVA_ERR_ARG, "pointset_assignment: null pointer");
  hipLaunchKernelGGL(assign_flag_kernel, dim3(1), dim3(1), 0, st, all_done, 1);
  if (B > 0) {
    if (n <= 64)
      assign_launch<64, 64>(x, y, col, cost, state, B, n, lo, hi, use_clamp, rounds, restart, all_done, st);
    else if (n <= 256)
      assign_launch<256, 256>(x, y, col, cost, state, B, n, lo, hi, use_clamp, rounds, restart, all_done, st);
    else if (n <= 1024)
      assign_launch<256, 1024>(x, y, col, cost, state, B, n, lo, hi, use_clamp, rounds, restart, all_done, st);
    else if (n <= 2048)
      assign_launch<512, 2048>(x, y, col, cost, state, B, n, lo, hi, use_clamp, rounds, restart, all_done, st);
    else
      assign_launch<1024, 4096>(x, y, col, cost, state, B, n, lo, hi, use_clamp, rounds, restart, all_done, st);
  }
  return check_launch("pointset_assignment");
}

int nova_pointset_assignment_rounds(const void* state, int* rounds_used, int B, int n, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (n < 1 || n > ASSIGN_MAX_N)
    return set_error(NOVA_ERR_ARG, "pointset_assignment_rounds: n %d outside 1 .. %d (NOVA_ASSIGN_MAX_POINTS)", n, ASSIGN_MAX_N);
  if (B <= 0) return 0;
  if (!state || !rounds_used) return set_error(NOVA_ERR_ARG, "pointset_assignment_rounds: null pointer");
  hipLaunchKernelGGL(assign_rounds_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (const char*)state, assign_state_bytes(n),
                     rounds_used, B);
  return check_launch("pointset_assignment_rounds");
}

}  // extern "C"
