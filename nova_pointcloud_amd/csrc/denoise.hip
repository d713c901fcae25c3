// The denoising loop of one AR step (nova_decoder_denoise, nova_decoder_denoise_echo): a call struct that each entry fills once,
// the plan of a sampler step, the launch sequence, and its replay as a captured hipGraph.
#include <atomic>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <utility>
#include "nova_internal.h"

namespace nova {

// What a call does, under guidance renorm, with the rows of a sample that are NOT predicted in this AR step (they echo x_t and enter
// both norms): nothing (renorm off), their squared norm as one scalar per sample (the Euler step only), or the rows themselves.
enum class Echo { none, energy, rows };

struct DenoiseCall {  // the arguments of the two entries (include/nova_hip.h)
  const nova_decoder* dec;
  const void *zc, *temb;
  float* x;
  const nova_sampler_step* sched;
  const float *noise, *echo_noise;
  float renorm;
  Echo echo;
  float *echo_energy, *echo_rows;
  int Ne, steps, S, B, n, P, D;
  void *ws_a, *ws_u, *ws_h, *ws_f, *ws_g, *ws_mod;
  float* ws_v;
  int mod_steps, dtype;
  hipStream_t st;
};

// what the two entries check alike, under the entry's name
static int check_call(const char* entry, const DenoiseCall& c) {
  NOVA_REQUIRE(!bad_dtype(c.dtype), NOVA_ERR_ARG, "%s: bad dtype %d", entry, c.dtype);
  NOVA_REQUIRE(c.dec && c.zc && c.temb && c.x && c.sched && c.ws_a && c.ws_u && c.ws_h && c.ws_f && c.ws_g && c.ws_mod, NOVA_ERR_ARG, "%s: null pointer", entry);
  NOVA_REQUIRE(c.S == c.B || c.S == 2 * c.B || c.S == 3 * c.B, NOVA_ERR_SHAPE, "%s: S must be B, 2B or 3B", entry);
  NOVA_REQUIRE(c.dec->depth >= 1 && c.dec->blocks, NOVA_ERR_ARG, "%s: the decoder needs at least one block", entry);
  return 0;
}

// One sampler step as the loop runs it: guidance on / off, the guidance passes and with them the sequences and rows of its launches
struct StepPlan { bool cfg; int passes, Se; long rows; };
static StepPlan step_plan(const nova_sampler_step& s, int B, int n) {
  const int passes = s.guidance > 1.0f ? (s.extra_kind ? 3 : 2) : 1;
  return {passes > 1, passes, passes * B, (long)(passes * B) * n};
}

// The row passes of a step on `rows` rows of the modulation `mod` (scale | shift | gate columns per block, then the final layer's scale | shift).
// modulate: h <- LN(u) (1 + scale) + shift of block b (b == depth: the final layer); gate: u <- (LN(g) gamma + beta) gate + u of block b.
static long mod_ld(const DenoiseCall& c) { return (long)(3 * c.dec->depth + 2) * c.D; }
static RowNormArgs modulate_args(const DenoiseCall& c, const void* mod, long rows, int b) {
  return {c.ws_u, c.ws_h, nullptr, nullptr, mod, mod_ld(c), b * 3 * c.D, b * 3 * c.D + c.D, -1, nullptr, nullptr, rows, c.D, 1e-6f};
}
static RowNormArgs gate_args(const DenoiseCall& c, const void* mod, long rows, int b) {
  const nova_mlp_block& blk = c.dec->blocks[b];
  return {c.ws_g, c.ws_u, blk.norm2_w, blk.norm2_b, mod, mod_ld(c), -1, -1, b * 3 * c.D + 2 * c.D, c.ws_u, nullptr, rows, c.D, 1e-5f};
}

// The launch sequence of one AR step's denoising loop (called directly, or once under stream capture: see below).
static int denoise_launches(const DenoiseCall& c) {
  // The whole plan is checked before the first launch: a refused call leaves x (and the echo energy / rows) as they were, captured or not
  NOVA_REQUIRE(c.mod_steps == 1 || c.mod_steps == c.steps, NOVA_ERR_ARG, "decoder_denoise: mod_steps must be 1 or steps");
  NOVA_REQUIRE(c.P >= 1 && c.P <= 64, NOVA_ERR_SHAPE, "decoder_denoise: patch vector length %d unsupported", c.P);
  for (int i = 0; i < c.steps; ++i) {
    const nova_sampler_step& s = c.sched[i];
    NOVA_REQUIRE(s.extra_kind >= 0 && s.extra_kind <= 2, NOVA_ERR_ARG, "decoder_denoise: extra_kind must be 0, 1 or 2");
    const int passes = step_plan(s, c.B, c.n).passes;
    NOVA_REQUIRE(c.S >= passes * c.B, NOVA_ERR_SHAPE, "decoder_denoise: step %d needs %d guidance passes but S = %d, B = %d", i, passes, c.S, c.B);
    // the scalar echo energy follows the Euler step only, on the steps without guidance (guidance_trunc) as well: they scale it too
    NOVA_REQUIRE(c.echo != Echo::energy || (s.kx == 0.f && s.kv == 1.f && s.cx == 1.f && s.sigma == 0.f && s.clip <= 0.f),
                 NOVA_ERR_ARG, "decoder_denoise: guidance renorm with a scalar echo energy holds for the flow-matching Euler step only "
                 "(other samplers: nova_decoder_denoise_echo with the echo rows)");
  }
  const nova_decoder& dec = *c.dec;
  const int depth = dec.depth, B = c.B, n = c.n, P = c.P, D = c.D, dtype = c.dtype;
  const size_t es = esize(dtype), nP = (size_t)B * n * P;
  const long ld = mod_ld(c), rows_all = (long)c.S * n;
  hipStream_t st = c.st;
  // mod_steps == steps: the AdaLN projections of ALL steps in one GEMM ahead of the loop (M = steps * S * n rows: the large-M kernel at ~2.5x the
  // rate of the per-step small-M launches, and two launches fewer per step). Rows are laid out per step for the full S sequences; a step that
  // runs fewer guidance passes (guidance_trunc) reads its leading rows.
  const bool hoist = c.mod_steps == c.steps && c.steps > 1;
  if (hoist) {
    NOVA_TRY(silu_add_steps(c.zc, c.temb, c.ws_a, rows_all, c.steps, D, dtype, st));
    NOVA_TRY(gemm_bias_act(c.ws_a, dec.adaln_w, dec.adaln_b, c.ws_mod, (int)(rows_all * c.steps), (int)ld, D, NOVA_ACT_NONE, dtype, st));
  }
  for (int i = 0; i < c.steps; ++i) {
    const nova_sampler_step& sp = c.sched[i];
    const StepPlan p = step_plan(sp, B, n);
    const int rows = (int)p.rows;
    void* const mod = hoist ? static_cast<char*>(c.ws_mod) + (size_t)i * rows_all * ld * es : c.ws_mod;
    if (!hoist) {
      NOVA_TRY(silu_add_rows(c.zc, static_cast<const char*>(c.temb) + (size_t)i * D * es, c.ws_a, p.rows, D, dtype, st));
      NOVA_TRY(gemm_bias_act(c.ws_a, dec.adaln_w, dec.adaln_b, mod, rows, (int)ld, D, NOVA_ACT_NONE, dtype, st));
    }
    NOVA_TRY(patch_embed_rows(c.x, dec.patch_w, dec.patch_b, c.ws_u, p.Se, B, n, P, D, dtype, st));
    // Per block: m1 (modulate -> h), fc1 + SiLU, fc2, m2 (gated norm + residual -> u). Where the small-M kernel does not take m1 + fc1 as one
    // launch (more than ~320 rows: every step of the batch-32 workload but the first few), m2 of block b and m1 of block b + 1 are ONE row pass
    // (row_norm_chain: u is written, h comes out of the same registers; bit-identical to the two launches), so a block is 3 launches instead of 4.
    const bool m1_fused = gemm_modulate_fused(rows, D, D, dtype);  // m1 rides inside the fc1 launch (skinny.hip)
    const bool chain = !m1_fused && dtype_is16(dtype);
    for (int b = 0; b < depth; ++b) {
      const nova_mlp_block& blk = dec.blocks[b];
      if (chain && b > 0) NOVA_TRY(gemm_bias_act(c.ws_h, blk.fc1_w, blk.fc1_b, c.ws_f, rows, D, D, NOVA_ACT_SILU, dtype, st));  // h: the previous block's chain launch
      else NOVA_TRY(gemm_modulate_act(modulate_args(c, mod, p.rows, b), blk.fc1_w, blk.fc1_b, c.ws_f, rows, D, D, NOVA_ACT_SILU, dtype, st));  // one launch at small M
      NOVA_TRY(gemm_bias_act(c.ws_f, blk.fc2_w, blk.fc2_b, c.ws_g, rows, D, D, NOVA_ACT_NONE, dtype, st));
      const RowNormArgs m2 = gate_args(c, mod, p.rows, b);
      if (b == depth - 1 && dtype_is16(dtype)) {
        // last block: its gated norm + residual and the final layer's modulate in ONE row pass (x itself is not needed
        // any more, so it is neither written nor read back); bit-identical to the two launches (rownorm.h)
        NOVA_TRY(row_norm_chain(m2, modulate_args(c, mod, p.rows, depth), nullptr, dtype, st));
      } else if (chain) {
        NOVA_TRY(row_norm_chain(m2, modulate_args(c, mod, p.rows, b + 1), c.ws_u, dtype, st));  // u <- m2 in place (row-local), h <- m1 of the next block
      } else {
        NOVA_TRY(row_norm(m2, dtype, st));
        if (b == depth - 1) NOVA_TRY(row_norm(modulate_args(c, mod, p.rows, depth), dtype, st));
      }
    }
    const float* nz = (c.noise && sp.sigma != 0.f) ? c.noise + (size_t)i * nP : nullptr;
    const float* enz = (c.echo_noise && sp.sigma != 0.f) ? c.echo_noise + (size_t)i * B * c.Ne * P : nullptr;
    if (c.echo != Echo::none && p.cfg) {
      // guidance renorm (guidance_scaler.py:67-72): the head leaves x alone, the renorm launch takes the step with the ratio of the norms
      // over the whole sample - any sampler step with the echo rows carried explicitly, the Euler step on their scalar energy
      float *vhat = c.ws_v, *cond = c.ws_v + nP, *extra = p.passes == 3 ? c.ws_v + 2 * nP : nullptr;
      NOVA_TRY(head_cfg_step(c.ws_h, dec.head_w, dec.head_b, c.x, nullptr, vhat, cond, extra, B, n, P, D, sp, 1, dtype, st));
      if (c.echo == Echo::rows) NOVA_TRY(renorm_step(c.x, vhat, cond, extra, nz, c.echo_rows, enz, B, n * P, c.Ne * P, sp, c.renorm, 0, st));
      else NOVA_TRY(renorm_euler(c.x, vhat, cond, extra, c.echo_energy, B, n, P, sp.c0, c.renorm, st));
    } else {
      NOVA_TRY(head_cfg_step(c.ws_h, dec.head_w, dec.head_b, c.x, nz, nullptr, nullptr, nullptr, B, n, P, D, sp, 0, dtype, st));
      // guidance switched off for this step (guidance_trunc): no renorm, but the echo rows still take the step
      if (c.echo == Echo::rows) NOVA_TRY(renorm_step(nullptr, nullptr, nullptr, nullptr, nullptr, c.echo_rows, enz, B, n * P, c.Ne * P, sp, c.renorm, 1, st));
      if (c.echo == Echo::energy) NOVA_TRY(scale_vector(c.echo_energy, B, (1.0f + sp.c0) * (1.0f + sp.c0), st));
    }
  }
  return 0;
}

// ---- hipGraph replay of the denoising loop.
// One AR step issues 25 x (15 to 27) launches of 4-15 us kernels from one host thread. The sequence is a pure function of the call's
// arguments, so it is captured once per distinct argument set - pointers, shapes, the per-step sampler plan and the decoder's weight
// pointers all go into the key - and replayed with one hipGraphLaunch afterwards. The engine keeps every buffer of the call at a stable
// address (workspace slots), so from the second generation on every AR step of a fixed schedule is a replay.
// Measured (tools/host_vs_gpu.py): the host thread's time in a batch-8 generation call drops 907 -> 795 ms; wall time is unchanged at
// batch 8 and 32 (the device, not the launch rate, bounds both), the first call of a schedule pays ~3 ms per captured graph.
// Calls that read per-call tensors the engine allocates afresh (ancestral noise, guidance-renorm scratch) and profiled runs (HIP-event
// brackets around launches) stay on the direct path.
static std::atomic<long> g_graph_epoch{0};  // bumped by nova_debug_set_graphs(0): every thread drops its cache at its next call
struct DecoderGraphs {
  std::unordered_map<std::string, hipGraphExec_t> execs;
  long captures = 0, replays = 0, epoch = 0;
  ~DecoderGraphs() { clear(false); }  // thread exit / process teardown: the runtime may already be going down, no device call but the destroys
  // A launch of one of these execs may still be queued or running on some stream (the host runs ahead of the device, and the caller
  // drops the cache exactly when it is about to re-plan: a workspace that changed shape, graphs switched off): wait for the device
  // before the execs and their kernel-argument storage go. Rare by construction (shape changes), so the wait is not a cost.
  void clear(bool wait = true) {
    if (wait && !execs.empty()) (void)hipDeviceSynchronize();
    for (auto& kv : execs) (void)hipGraphExecDestroy(kv.second);
    execs.clear();
  }
  // Replays the graph kept under `key` on `st`; the first call of a key captures it from `launches` and instantiates it. Where the stream
  // cannot be captured or the graph not instantiated, nothing has executed yet (the launches were only recorded): `launches` runs directly.
  template <typename F> int run(std::string key, hipStream_t st, F&& launches) {
    if (const long now = g_graph_epoch.load(std::memory_order_relaxed); now != epoch) {
      clear();
      epoch = now;
    }
    auto it = execs.find(key);
    if (it == execs.end()) {
      if (execs.size() >= 2048) clear();  // schedules come and go: start over rather than grow
      hipGraphExec_t exec = nullptr;
      hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        const int rc = launches();
        hipGraph_t graph = nullptr;
        e = hipStreamEndCapture(st, &graph);
        if (e == hipSuccess && graph && rc == 0) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (rc != 0) return rc;
      }
      if (e != hipSuccess || !exec) {
        (void)hipGetLastError();
        return launches();
      }
      it = execs.emplace(std::move(key), exec).first;
      ++captures;
    } else {
      ++replays;
    }
    const hipError_t el = hipGraphLaunch(it->second, st);
    NOVA_REQUIRE(el == hipSuccess, NOVA_ERR_LAUNCH, "decoder_denoise: hipGraphLaunch failed: %s", hipGetErrorString(el));
    return 0;
  }
};
static thread_local DecoderGraphs g_dec_graphs;
static std::atomic<int> g_graphs_on{-1};  // -1: not decided yet (NOVA_GRAPHS env, default on)

static bool graphs_enabled() {
  int v = g_graphs_on.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("NOVA_GRAPHS");
    g_graphs_on.store(v = (e && e[0] == '0') ? 0 : 1);
  }
  return v != 0;
}

template <typename T> static void key_put(std::string& k, const T& v) { k.append(reinterpret_cast<const char*>(&v), sizeof(T)); }

// Everything the launch sequence is a function of, field by field: nova_decoder has a 4-byte hole behind `depth` whose bytes are
// whatever the caller's memory held. The blocks are keyed by their contents, not by the array's address.
static std::string graph_key(const DenoiseCall& c) {
  std::string key;
  key.reserve(512 + sizeof(nova_sampler_step) * c.steps + sizeof(nova_mlp_block) * c.dec->depth);
  key_put(key, c.dec->depth);
  const void* dec_ptrs[] = {c.dec->adaln_w, c.dec->adaln_b, c.dec->patch_w, c.dec->patch_b, c.dec->head_w, c.dec->head_b};
  key_put(key, dec_ptrs);
  for (int b = 0; b < c.dec->depth; ++b) key_put(key, c.dec->blocks[b]);
  for (int i = 0; i < c.steps; ++i) key_put(key, c.sched[i]);
  const void* ptrs[] = {c.zc, c.temb, c.x, c.ws_a, c.ws_u, c.ws_h, c.ws_f, c.ws_g, c.ws_mod, (const void*)c.st};
  key_put(key, ptrs);
  const int ints[] = {c.steps, c.S, c.B, c.n, c.P, c.D, c.mod_steps, c.dtype, walk_is_reverse() ? 1 : 0, gemm_forced_tile(), skinny_forced_row_blocks()};
  key_put(key, ints);
  return key;
}

static int denoise(const DenoiseCall& c) {  // a checked call
  if (c.n == 0 || c.B == 0) return 0;
  // direct launches where they read per-call tensors (renorm, noise), with graphs off, under profiling and for a single step
  if (c.echo != Echo::none || !graphs_enabled() || prof_enabled() || c.noise != nullptr || c.steps < 2) return denoise_launches(c);
  return g_dec_graphs.run(graph_key(c), c.st, [&c] { return denoise_launches(c); });
}

}  // namespace nova

using namespace nova;

extern "C" {

int nova_debug_set_graphs(int on) {
  g_graphs_on.store(on ? 1 : 0);
  if (!on) {  // the calling thread's graphs go now, every other thread's at its next nova_decoder_denoise (the caches are thread-local)
    g_graph_epoch.fetch_add(1);
    g_dec_graphs.clear();
  }
  return 0;
}

int nova_debug_drop_graphs(void) {
  g_dec_graphs.clear();
  return 0;
}

int nova_debug_graph_stats(long* captures, long* replays) {
  if (captures) *captures = g_dec_graphs.captures;
  if (replays) *replays = g_dec_graphs.replays;
  return 0;
}

int nova_decoder_denoise(const nova_decoder* dec, const void* zc, const void* temb, float* x, const nova_sampler_step* sched,
                         const float* noise, float renorm, float* echo_energy, int steps, int S, int B, int n, int P, int D,
                         void* ws_a, void* ws_u, void* ws_h, void* ws_f, void* ws_g, void* ws_mod, float* ws_v, int mod_steps,
                         int dtype, void* stream) {
  const DenoiseCall c{dec, zc, temb, x, sched, noise, nullptr, renorm, renorm < 1.0f ? Echo::energy : Echo::none, echo_energy, nullptr, 0,
                      steps, S, B, n, P, D, ws_a, ws_u, ws_h, ws_f, ws_g, ws_mod, ws_v, mod_steps, dtype, (hipStream_t)stream};
  NOVA_TRY(check_call("decoder_denoise", c));
  NOVA_REQUIRE(c.echo == Echo::none || (echo_energy && ws_v), NOVA_ERR_ARG, "decoder_denoise: renorm needs echo_energy and ws_v");
  return denoise(c);
}

int nova_decoder_denoise_echo(const nova_decoder* dec, const void* zc, const void* temb, float* x, const nova_sampler_step* sched,
                              const float* noise, float renorm, float* echo_rows, const float* echo_noise, int Ne, int steps, int S, int B,
                              int n, int P, int D, void* ws_a, void* ws_u, void* ws_h, void* ws_f, void* ws_g, void* ws_mod, float* ws_v,
                              int mod_steps, int dtype, void* stream) {
  const DenoiseCall c{dec, zc, temb, x, sched, noise, echo_noise, renorm, Echo::rows, nullptr, echo_rows, Ne,
                      steps, S, B, n, P, D, ws_a, ws_u, ws_h, ws_f, ws_g, ws_mod, ws_v, mod_steps, dtype, (hipStream_t)stream};
  NOVA_TRY(check_call("decoder_denoise_echo", c));
  NOVA_REQUIRE(renorm < 1.0f && echo_rows && ws_v && Ne >= 0, NOVA_ERR_ARG,
               "decoder_denoise_echo: for guidance_renorm < 1 with the echo rows given (else: nova_decoder_denoise)");
  return denoise(c);
}

}  // extern "C"
