"""Benchmark of the NOVA point-set generation hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one full `NOVAPipeline.__call__` (prompt embeddings -> point sets) of the workload
BASELINE.json's metric is quoted on: NOVA-d48w1024 (0.6B), 2048 points per sample, 64 AR steps x 25
diffusion steps, CFG on, bf16, batch 32 PER GPU (weak scaling; configs[2] at N=1, configs[3] at
N=8). Prompts are synthetic and already resident in HBM; weights are random-init (no network).
Rank 0 prints ONE JSON line: whole-job generated points/s and ms_per_step. A plain run does nothing
else: set up, warm up, time --steps steps, print. With --full the line also carries
  roofline      the dominant kernel family (MFMA GEMM / attention), timed with HIP events on the
                launch stream (nova_prof_*) in one extra serialised pass of the step after the timed
                region, against the 2.5 PFLOP/s dense bf16 MFMA peak of MI355X_MICROARCH.md
  cpu_baseline  the oracle (oracle/nova_oracle.py, a port of the reference's CPU path) timed on the
                host cores on a bounded sample of the same workload (rank 0, N=1 only).
--dump-outputs DIR writes the point sets of the last timed step as DIR/points.npy (float32); with
the same arguments every run draws the same weights, prompts and noise.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "nova_pointcloud_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
MFMA_FP8_PEAK_TFLOPS = 5000.0   # dense fp8 (block-scaled MFMA), same table

WORKLOADS = {
    # name: (width, heads, latent H, W, per-GPU batch)   N = H*W points, Nv = N/4 condition tokens
    "d48w1024_2048pts_b32": (1024, 16, 32, 64, 32),
    "d48w768_1024pts_b8": (768, 12, 32, 32, 8),
    "d48w768_256pts_b1": (768, 12, 16, 16, 1),
    "d48w1536_2048pts_b32": (1536, 16, 32, 64, 32),  # configs[4] architecture (head_dim 96) in bf16
}


def flops_per_sample(D, N, Nv, Lt, schedule, S, P=3, token_dim=2560):
    """Algorithmic FLOPs of one generated sample with CFG (SURVEY §8d formula, exact integer schedule)."""
    blk = lambda L: 24.0 * D * D * L + 4.0 * L * L * D
    total = 16 * blk(Lt + Nv) + Lt * 2.0 * token_dim * D
    done = 0
    for n in schedule:
        total += 16 * blk(Nv + done) + 16 * blk(Nv + N)
        total += S * n * (68.0 * D * D + 4.0 * D * P)
        done += n
    return 2.0 * total


def build_pipeline(width, heads, H, W, dtype, device, seed=0):
    from diffnext.models.transformers.transformer_nova import NOVATransformer3DModel
    from diffnext.pipelines import NOVAPipeline
    from diffnext.schedulers import FlowMatchEulerDiscreteScheduler

    torch.manual_seed(seed)
    model = NOVATransformer3DModel(
        image_dim=3, image_size=(16 * H, 16 * W), image_stride=16, text_token_dim=2560, text_token_len=256,
        image_base_size=[H, W], video_base_size=[1, H // 2, W // 2], rotary_pos_embed=True,
        arch=(f"vit_d16w{width}", f"vit_d32w{width}", f"mlp_d6w{width}"))
    model = model.to(dtype=dtype).to(device).eval()
    return NOVAPipeline(transformer=model, scheduler=FlowMatchEulerDiscreteScheduler(num_train_timesteps=1000, shift=1.0))


def synthetic_prompts(B, device, dtype, seed=1234):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(8, 65, (B,), generator=g).tolist()
    return [(0.02 * torch.randn(n, 2560, generator=g)).to(device=device, dtype=dtype) for n in lens]


def host_cores():
    """CPU share of this process: cgroup quota if set, else the affinity mask (never the machine's core count)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 32))


def cpu_baseline(pipe, width, heads, H, W, threads, with_config0=False):
    """Oracle (port of the reference CPU path) on a bounded sample of the SAME architecture, as BASELINE.md section 4 plans it:
    B=1, all N points, 4 AR x 4 diffusion steps (2 x 2 above width 1024, to stay near 20 s of CPU work), converted to points/s
    of the full 64 x 25 workload by the FLOP ratio. `with_config0`: BASELINE configs[0] (d48w768, 256 points, 4 x 4, batch 1,
    the reference's own CPU-runnable case) timed IN FULL as well, reported under "config0"."""
    from oracle import nova_oracle as O

    torch.set_num_threads(threads)
    N, Nv = H * W, (H // 2) * (W // 2)
    sd = {k: v.detach().float().cpu() for k, v in pipe.transformer.state_dict().items()}
    cfg = O.make_config(3, (H, W), 1, width, heads, 16, 32, 6, 256, rotary=True)
    g = torch.Generator().manual_seed(5)
    prompt = O.encode_prompt_embeds(sd["text_embed.weight"], [0.02 * torch.randn(24, 2560, generator=g)], 256)
    K = S = 4 if width <= 1024 else 2
    sched = [int(v) for v in O.cosine_schedule(N, K) if v > 0]
    t0 = time.time()
    with torch.no_grad():
        O.generate(sd, cfg, prompt, sched, num_diffusion_steps=S, guidance_scale=5.0, generator=g)
    dt = time.time() - t0
    sample_flops = flops_per_sample(width, N, Nv, 256, sched, S)
    full = flops_per_sample(width, N, Nv, 256, [int(v) for v in O.cosine_schedule(N, 64) if v > 0], 25)
    tflops = sample_flops / dt / 1e12
    rec = {"value": round(tflops * 1e12 / (full / N), 3), "unit": "points/s", "cores": threads, "kind": "port",
           "sample": f"oracle fp32, same d48w{width} weights, B=1, {N} points, {K} AR x {S} diffusion steps "
                     f"({sample_flops / 1e12:.2f} TFLOP in {dt:.1f} s = {tflops:.3f} TFLOP/s), scaled by FLOPs to 64x25"}
    if with_config0:
        del sd
        p0 = build_pipeline(768, 12, 16, 16, torch.float32, torch.device("cpu"))
        sd0 = {k: v.detach().float() for k, v in p0.transformer.state_dict().items()}
        cfg0 = O.make_config(3, (16, 16), 1, 768, 12, 16, 32, 6, 256, rotary=True)
        prompt0 = O.encode_prompt_embeds(sd0["text_embed.weight"], [0.02 * torch.randn(24, 2560, generator=g)], 256)
        sched0 = [int(v) for v in O.cosine_schedule(256, 4) if v > 0]
        t0 = time.time()
        with torch.no_grad():
            O.generate(sd0, cfg0, prompt0, sched0, num_diffusion_steps=4, guidance_scale=5.0, generator=g)
        dt0 = time.time() - t0
        f0 = flops_per_sample(768, 256, 64, 256, sched0, 4)
        rec["config0"] = {"workload": "d48w768, 256 points, 4 AR x 4 diffusion steps, batch 1, in full (BASELINE configs[0])",
                          "seconds": round(dt0, 2), "points_per_s": round(256 / dt0, 1), "tflops": round(f0 / dt0 / 1e12, 3)}
    return rec


# kernel names (tools/pmc_summary.py's short form) behind each timed family, in the bf16 run and in the fp8 GEMM mode
PMC_KERNEL_FP8 = {"attention": "attn_bf16_m16<bf16,96,2,false,true,false>", "gemm_bias": "gemm256c_kernel<bf16,0,false>", "gemm_bias_wide_k": "gemm256p_kernel<fp8,0>",
                  "gemm_bias_gelu": "gemm256p_kernel<fp8,5>", "qkv_gemm_rope": "gemm256p_kernel<fp8,3>"}
PMC_KERNEL = {"attention": "attn_bf16_m16<bf16,64,2,false,true,false>", "gemm_bias": "gemm256c_kernel<bf16,0,false>[proj]", "gemm_bias_wide_k": "gemm256c_kernel<bf16,0,false>[fc2]",
              "gemm_bias_gelu": "gemm256c_kernel<bf16,1,false>", "qkv_gemm_rope": "gemm256c_kernel<bf16,3,true>"}
MFMA_FAMILIES = ("attention", "qkv_gemm_rope", "gemm_bias", "gemm_bias_wide_k", "gemm_bias_gelu", "gemm_bias_silu", "gemm_small_tile")


def pmc_traffic(family, workload, fp8=False):
    pmc_traffic.clock_ghz = None
    """HBM bytes per launch of the dominant kernel from the newest profiles/r*_pmc.json (tools/pmc_collect.sh +
    tools/pmc_summary.py: separate rocprofv3 --pmc passes; counters cannot be read from inside the process). The file
    records the sha256 of the kernel sources it was measured on: a stale file is reported as such, not used."""
    import glob
    import hashlib

    # bf16: one block at the d48w1024 shapes (profiles/r*_pmc.json); fp8 GEMM mode: one block at the d48w1536 shapes (r*_pmc_fp8.json)
    if (workload, fp8) not in (("d48w1024_2048pts_b32", False), ("d48w1536_2048pts_b32", True)):
        return None, "PMC passes are taken at the d48w1024 shapes (bf16) and the d48w1536 shapes (fp8 mode) only"
    names, pattern = (PMC_KERNEL_FP8, "r*_pmc_fp8.json") if fp8 else (PMC_KERNEL, "r*_pmc.json")
    h = hashlib.sha256()
    csrc = os.path.join(PKG, "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
        try:
            doc = json.load(open(path))
            rec = doc["kernels"][names[family]]
        except (OSError, KeyError, ValueError):
            continue
        name = os.path.basename(path)
        if doc.get("source_sha256") != h.hexdigest():
            return None, f"profiles/{name} was measured on other kernel sources (sha mismatch): re-run tools/pmc_collect.sh"
        note = f"profiles/{name}: {doc['shape']}; 2 x FETCH_SIZE + WRITE_SIZE of the {names[family]} launch, separate rocprofv3 --pmc passes"
        if rec.get("hbm_over_algorithmic") is not None:
            note += f"; {rec['hbm_over_algorithmic']} x the launch's algorithmic bytes"
        pmc_traffic.clock_ghz = rec.get("clock_ghz")  # GRBM_GUI_ACTIVE / 8 / duration of the same passes (the chip lowers its clock under load)
        return rec.get("hbm_bytes"), note
    return None, "no profiles/r*_pmc.json"


def kernel_pass_fields(prof, prof_elapsed, dtype, workload):
    """`roofline` and `kernels` of the --full line from the serialised kernel pass: per-slot (ms, work, launches) of the
    library's HIP-event hooks and the wall time of the pass."""
    BYTES = ("row_norm",)          # work counted in bytes (HBM-bound row kernels); the slots below carry no work figure
    NOWORK = ("token_plumbing", "decoder_glue")
    fams = {}
    for k, (ms, wk, n) in prof.items():
        if not n:
            continue
        fams[k] = {"ms": round(ms, 2), "launches": n}
        if k not in NOWORK:
            fams[k].update(rate=round(wk / ms / (1e6 if k in BYTES else 1e9), 2) if ms > 0 else 0.0, unit="GB/s" if k in BYTES else "TFLOP/s")
    mfma = {k: v for k, v in fams.items() if k in MFMA_FAMILIES}

    def peak_of(k):
        # fp8 mode: the fc1 (+GELU), QKV (+RoPE) and fc2 kernels are pure fp8 launches -> dense fp8 peak; attention, the
        # out-projection and the small-tile kernels are bf16
        return MFMA_FP8_PEAK_TFLOPS if (dtype == "fp8" and k in ("gemm_bias_gelu", "qkv_gemm_rope", "gemm_bias_wide_k")) else MFMA_BF16_PEAK_TFLOPS

    for k, v in mfma.items():
        v["frac"] = round(v["rate"] / peak_of(k), 4)
    pass_ms = prof_elapsed * 1e3
    for v in fams.values():
        v["share"] = round(v["ms"] / pass_ms, 4)
    # the reported kernel: the family with the most time; families within 2 % of it count as tied and the tie goes to the
    # LOWER fraction of peak (so the choice does not flip between runs towards the better-looking kernel)
    top_ms = max(v["ms"] for v in mfma.values())
    dom = min((k for k, v in mfma.items() if v["ms"] >= 0.98 * top_ms), key=lambda k: mfma[k]["frac"])
    # HBM traffic of that kernel comes from a separate rocprofv3 --pmc run (counters cannot be read from inside the process);
    # the committed summary is for one launch of that kernel at the workload's shapes, reported with its context.
    traffic, traffic_note = pmc_traffic(dom, workload, fp8=dtype == "fp8")
    peak = peak_of(dom)
    work_tflop = {k: mfma[k]["rate"] * mfma[k]["ms"] / 1e3 for k in mfma}  # TFLOP executed per family in the pass
    weighted = sum(work_tflop[k] / peak_of(k) for k in mfma) / (sum(v["ms"] for v in mfma.values()) / 1e3)
    timed_ms = sum(v["ms"] for v in fams.values())
    return {
        "roofline": {"bound": "mfma", "kernel": dom, "achieved": mfma[dom]["rate"], "peak": peak,
                     "unit": "TFLOP/s", "frac": round(mfma[dom]["rate"] / peak, 4), "traffic": traffic, "traffic_note": traffic_note,
                     "clock_ghz_under_counters": pmc_traffic.clock_ghz,
                     "clock_note": "shader clock the chip held under this kernel in the rocprofv3 counter passes (GRBM_GUI_ACTIVE / 8 / duration; "
                                   "nominal 2.4 GHz, which `peak` is priced at); in-kernel clock reads of every encoder kernel, on random and on "
                                   "zero-filled operands: profiles/r04_kernel_clock.txt (not measured in this run)",
                     "avg_launch_ms": round(mfma[dom]["ms"] / mfma[dom]["launches"], 4),
                     "share_of_step_time": mfma[dom]["share"],
                     "kernel_choice": "family with the most time in the serialised pass; ties within 2 % go to the lower fraction",
                     "families": {k: {"ms": v["ms"], "share": v["share"], "achieved": v["rate"], "frac": v["frac"]}
                                  for k, v in sorted(mfma.items(), key=lambda kv: -kv[1]["ms"])},
                     "mfma_time_weighted_frac": round(weighted, 4),
                     "pass": {"ms": round(pass_ms, 1), "timed_kernels_ms": round(timed_ms, 1),
                              "untimed_ms": round(pass_ms - timed_ms, 1),
                              "note": "untimed = PyTorch's own kernels (draws, copies, argsort), launch gaps of the direct-launched "
                                      "denoising loop and host time of the serialised pass; no library kernel is outside the slots"},
                     "timing": "HIP events on the launch stream; one extra pass of the same step after the timed region with the "
                               "two half-batch lanes serialised (concurrent lanes would put the other lane's kernels "
                               "inside each event bracket)"},
        "kernels": fams,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="d48w1024_2048pts_b32", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch override (0 = workload default)")
    ap.add_argument("--ar-steps", type=int, default=64)
    ap.add_argument("--diffusion-steps", type=int, default=25)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32", "fp8"],
                    help="fp8: bf16 model with the encoder's QKV / fc1 / fc2 GEMMs on the block-scaled fp8 MFMA (configs[4]; never the headline)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="total samples over all ranks (0 = gpus x per-GPU batch); a value that does not divide gives ragged shards")
    ap.add_argument("--full", action="store_true",
                    help="also the serialised kernel pass (per-family timings, roofline) and the CPU baseline; off: the timed steps only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's point sets as DIR/points.npy (float32)")
    ap.add_argument("--cpu-dry-run", action="store_true",
                    help="rehearse the multi-process control flow on CPU (gloo, PyTorch module path, f32): not a measurement")
    args = ap.parse_args()

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    dry = args.cpu_dry_run
    if dry:
        device = torch.device("cpu")
    else:
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    torch.set_num_threads(max(1, host_cores() // world))  # N ranks build N CPU-initialised copies of the weights
    dist = None
    # one rank per GPU under torch.distributed.run; a one-rank launch under it also goes through the process group (RCCL
    # init, barrier, all_gather of the points, max-over-ranks of the time), a plain `python bench.py` does not
    distributed = world > 1 or "TORCHELASTIC_RUN_ID" in os.environ
    if distributed:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    from nova_pointcloud_amd import hip
    from nova_pointcloud_amd.sharding import generate_sharded
    from diffnext.pipelines.nova.pipeline_nova import cosine_set_sizes

    width, heads, H, W, B = WORKLOADS[args.workload]
    B = args.batch or B
    dtype = torch.float32 if (dry or args.dtype == "f32") else torch.float16 if args.dtype == "f16" else torch.bfloat16
    call_extra = {"gemm_dtype": "fp8"} if args.dtype == "fp8" else {}
    pipe = build_pipeline(width, heads, H, W, dtype, device)
    # the GLOBAL batch of prompts and ONE seed on every rank: each rank generates its contiguous block of samples and draws
    # the order / noise tensors of the global batch (sharding.py: sharded(seed) == unsharded(seed))
    G = args.global_batch or world * B  # global batch
    prompts = synthetic_prompts(G, device, dtype, seed=1234)
    gen = torch.Generator(device=device).manual_seed(0)
    sync = (lambda: None) if dry else torch.cuda.synchronize
    N, Nv = H * W, (H // 2) * (W // 2)

    def step(**extra):
        # per-rank pipeline call on its shard + the path's only exchange: all_gather of the generated point sets
        # (RCCL over xGMI; no collective at N = 1)
        if dry:
            gen.manual_seed(0)  # rehearsal: every step regenerates the same batch, so rank 0 can check it against an unsharded run
        return generate_sharded(pipe, prompts, rank, world, num_inference_steps=args.ar_steps,
                                num_diffusion_steps=args.diffusion_steps, guidance_scale=5, generator=gen, **call_extra, **extra)

    def fence():
        if distributed:
            dist.barrier()
        sync()

    if os.environ.get("NOVA_DUMP_MAPS"):  # diagnostics: attribute the frames of a native crash report to their libraries
        import shutil

        shutil.copyfile("/proc/self/maps", os.environ["NOVA_DUMP_MAPS"])
    for _ in range(args.warmup):
        pts = step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pts = step()
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        out = pts.cpu().numpy().astype(np.float32)
        out = out[:max(1, (64 << 20) // out[0].nbytes)]  # leading samples up to 64 MB (a fixed sample of the batch)
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "points.npy"), out)
    # Kernel pass (--full; after the timed region, not part of `value`): the same step once more with the engine's two
    # half-batch lanes serialised and the library's HIP-event hooks on. In the timed region the lanes' kernels run
    # concurrently on two streams, so an event bracket around one kernel there also spans the other lane's kernels;
    # serialised, the brackets measure each kernel alone (and agree with rocprofv3 --kernel-trace, profiles/).
    prof, prof_elapsed = {}, 0.0
    if args.full and not dry:
        hip.prof_enable(True)
        hip.prof_collect()
        t1 = time.perf_counter()
        step(lanes=1)
        fence()
        prof_elapsed = time.perf_counter() - t1
        prof = hip.prof_collect()
        hip.prof_enable(False)
    assert torch.isfinite(pts).all(), "non-finite points generated"
    assert pts.shape[0] == G, "gathered point sets do not cover the global batch"
    from nova_pointcloud_amd.sharding import shard_range

    ranks_seen, shards = [0], [[0, 0, G]]
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
        # what the process group itself reports: every rank contributes its own rank id through the collective, so the
        # JSON line proves how many ranks RCCL (gloo in the dry run) actually connected
        ids = torch.empty(world, dtype=torch.int64, device=device)
        dist.all_gather_into_tensor(ids, torch.tensor([rank], dtype=torch.int64, device=device))
        ranks_seen = sorted(int(v) for v in ids.tolist())
        assert ranks_seen == list(range(dist.get_world_size())), ranks_seen
        # per-rank prompt order: [rank, lo, hi) of the global prompt list each rank generated, as the ranks report it
        mine = torch.tensor([rank, *shard_range(G, rank, world)], dtype=torch.int64, device=device)
        allr = torch.empty(world * 3, dtype=torch.int64, device=device)
        dist.all_gather_into_tensor(allr, mine)
        shards = allr.view(world, 3).tolist()

    if rank == 0:
        schedule = [int(v) for v in cosine_set_sizes(N, args.ar_steps) if v > 0]
        fl = flops_per_sample(width, N, Nv, 256, schedule, args.diffusion_steps)
        value = G * N * args.steps / elapsed
        e2e_tflops = value / N * fl / 1e12 / world  # per GPU
        if dry:
            # rehearsal only: rank 0 also generates the whole batch unsharded from the same seed - the gathered rows must
            # be the same samples in the same (prompt) order
            from diffnext.pipelines.nova.pipeline_nova import points_from_latents

            whole = points_from_latents(pipe(prompt_embeds=prompts, output_type="latent", disable_progress_bar=True,
                                             num_inference_steps=args.ar_steps, num_diffusion_steps=args.diffusion_steps, guidance_scale=5,
                                             generator=torch.Generator(device=device).manual_seed(0)).frames).float()
            diff = float((whole - pts.float()).abs().max() / whole.abs().max())
            print(json.dumps({"dry_run": True, "n_gpus": world, "ranks_seen": ranks_seen, "shards": shards, "points": list(pts.shape),
                              "sharded_vs_unsharded_max_rel_diff": diff, "ms_per_step": round(elapsed / args.steps * 1e3, 2)}), flush=True)
            if distributed:
                dist.barrier()
                dist.destroy_process_group()
            return
        rec = {
            "metric": "generated points/sec/node, NOVA-d48w1024 @2048 pts, 64-step sample" if args.workload.startswith("d48w1024")
            else f"generated points/sec/node, {args.workload}",
            "value": round(value, 2), "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "fp8 (QKV / fc1 / fc2 GEMMs) + bf16" if args.dtype == "fp8" else args.dtype, "data": "synthetic",
            "config": {"workload": args.workload, "points_per_sample": N, "ar_steps": len(schedule),
                       "diffusion_steps": args.diffusion_steps, "batch_per_gpu": B, "global_batch": G, "shards": shards,
                       "guidance": "cfg 2-pass", "sharding": f"batch rows over {world} GPU(s), all_gather of points",
                       "ranks_seen": ranks_seen, "process_group": (dist.get_backend() if distributed else "none")},
            "end_to_end": {"tflops_per_gpu": round(e2e_tflops, 1), "frac_of_mfma_peak": round(e2e_tflops / MFMA_BF16_PEAK_TFLOPS, 4),
                           "gflop_per_point": round(fl / N / 1e9, 2)},
        }
        if args.full:
            rec.update(kernel_pass_fields(prof, prof_elapsed, args.dtype, args.workload))
            if world == 1 and not args.no_cpu_baseline:
                rec["cpu_baseline"] = cpu_baseline(pipe, width, heads, H, W, threads=host_cores(), with_config0=args.workload.startswith("d48w1024"))
        print(json.dumps(rec), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
