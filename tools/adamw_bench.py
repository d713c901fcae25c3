"""Gradient clipping + AdamW step over a whole parameter list, three forms on the same GPU:

    torch_foreach   torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True)    what the Trainer does with target AdamW
    torch_fused     torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True)
    hip             nova_pointcloud_amd.optim.FusedAdamW.step(max_grad_norm=...)         csrc/adamw.hip: two entry points

on two parameter lists built from shapes alone (the models are made on the meta device; only the shapes are used):

    d48w1024   the headline generator, arch (vit_d16w1024, vit_d32w1024, mlp_d6w1024): 652 tensors, 0.64 G parameters
    tiny       the toy generator of the training tests (1 + 2 blocks and a 1-block head of width 64) on the geometry of
               configs/train_pointcloud_tiny.yaml: 72 tensors, 0.2 M parameters; host launch work dominates here

each in float32, and in bfloat16 with master weights: FusedAdamW(master_weights=True) against torch forms that keep their
own float32 copy of every parameter, cast the bfloat16 gradients to float32, clip and step the copies, and cast the copies
back into the bfloat16 parameters (three more passes, which is what mixed-precision training with torch.optim costs).

    python3 tools/adamw_bench.py [--out profiles/adamw_bench.json]      every case, one JSON line
    python3 tools/adamw_bench.py --case d48w1024_f32                    one case in this process

Every case runs in a child process of its own under a time limit (--limit seconds); after a case that fails or runs out of
time nothing more is started. One call is clip + step with the gradients in place (the torch forms scale their gradients in
place, every call, as clip_grad_norm_ does; the HIP form never writes them). After a warm-up, a timed window is as many
calls in a row as last about --window seconds, between two device events, with no synchronisation inside; the windows of the
forms alternate, --reps of each (5 by default): the best time per call and the spread (max - min) / min. A form that torch
does not offer on this build is recorded with its error text. The compulsory traffic of the HIP form per element: float32
4 (norm) + 16 read + 12 written = 32 bytes; bfloat16 with master weights 2 + 14 + 14 = 30 bytes; over the time per call and
HBM_BYTES_PER_S it is the call's share of the achievable streaming rate. No ratio is fixed in advance: the times are reported,
not asserted. tests/test_fused_adamw.py holds the kernels to their definition bit for bit."""
import argparse
import json
import os
import subprocess
import sys

from pointset_bench_common import best_and_spread, calls_per_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = {"d48w1024": ("vit_d16w1024", "vit_d32w1024", "mlp_d6w1024"), "tiny": ("bench_vit_d1w64", "bench_vit_d2w64", "bench_mlp_d1w64")}
CASES = {f"{name}_{dtype}": (name, dtype) for name in LISTS for dtype in ("f32", "bf16")}
HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy); 8.0e12 is the specification
HIP_BYTES_PER_ELEMENT = {"f32": 32, "bf16": 30}
MAX_NORM = 1.0
HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def parameter_shapes(name):
    """The shapes of the trainable parameters of the list's model, which is made on the meta device: no weight exists."""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "nova_pointcloud_amd"))
    from diffnext.models.transformers import transformer_nova as TN

    TN.VIDEO_ENCODERS.register("bench_vit_d1w64", TN._vit, depth=1, embed_dim=64, num_heads=2)  # once per process: a case is a process
    TN.IMAGE_ENCODERS.register("bench_vit_d2w64", TN._vit, depth=2, embed_dim=64, num_heads=2)
    TN.IMAGE_DECODERS.register("bench_mlp_d1w64", TN._mlp, depth=1, embed_dim=64)
    with torch.device("meta"):
        model = TN.NOVATransformer3DModel(image_dim=3, image_size=(128, 128), image_stride=16, text_token_dim=64, text_token_len=8,
                                          image_base_size=[8, 8], video_base_size=[1, 4, 4], rotary_pos_embed=True, arch=LISTS[name])
    return [tuple(p.shape) for p in model.parameters()]


def make_forms(shapes, dtype_name):
    """{form: call} with each form's own parameters, gradients and optimizer state; a form torch refuses maps to its error."""
    import torch

    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd.optim import FusedAdamW

    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    gen = torch.Generator(device="cuda").manual_seed(7)

    def leaves():
        params = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen).to(dtype)) for s in shapes]
        for p in params:
            p.grad = (torch.randn(p.shape, device="cuda", generator=gen) * 0.01).to(dtype)
        return params

    def torch_form(**mode):
        params = leaves()
        if dtype == torch.float32:
            opt = torch.optim.AdamW(params, **HYPER, **mode)

            def call():
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
        else:  # the float32 copies are what the optimizer owns
            copies = [torch.nn.Parameter(p.detach().float()) for p in params]
            opt = torch.optim.AdamW(copies, **HYPER, **mode)

            def call():
                for c, p in zip(copies, params):
                    c.grad = p.grad.float()
                torch.nn.utils.clip_grad_norm_(copies, MAX_NORM)
                opt.step()
                torch._foreach_copy_([p.detach() for p in params], [c.detach() for c in copies])
        return call

    forms = {}
    for key, mode in (("torch_foreach", dict(foreach=True)), ("torch_fused", dict(fused=True))):
        try:
            forms[key] = torch_form(**mode)
            forms[key]()
        except Exception as e:  # this build of torch does not offer the form
            forms[key] = f"{type(e).__name__}: {e}"
    params = leaves()
    fused = FusedAdamW(params, **HYPER, master_weights=True)
    forms["hip"] = lambda: fused.step(max_grad_norm=MAX_NORM)
    return forms


def run_case(name, reps, seconds):
    import torch

    list_name, dtype_name = CASES[name]
    shapes = parameter_shapes(list_name)
    elements = sum(int(torch.Size(s).numel()) for s in shapes)
    forms = make_forms(shapes, dtype_name)
    sys.path.insert(0, ROOT)
    from nova_pointcloud_amd import optim

    refused = {key: fn for key, fn in forms.items() if isinstance(fn, str)}
    forms = {key: fn for key, fn in forms.items() if not isinstance(fn, str)}
    for fn in forms.values():  # warm-up: library load, first launches, the optimizers' state, the allocator's blocks
        fn()
        fn()
    before = dict(optim.stats)
    forms["hip"]()
    launches = {key: optim.stats[key] - before[key] for key in before}
    inner = {key: calls_per_window(fn, seconds) for key, fn in forms.items()}
    times = {key: [] for key in forms}
    for _ in range(reps):  # the forms alternate, so drift of the clock or the host meets all alike
        for key, fn in forms.items():
            times[key].append(window(fn, inner[key])[1])
    props = torch.cuda.get_device_properties(0)
    case = {"list": list_name, "dtype": dtype_name, "tensors": len(shapes), "elements": elements, "max_norm": MAX_NORM, "device": props.name,
            "compute_units": props.multi_processor_count, "hip_launches_per_call": launches, "hbm_bytes_per_s": HBM_BYTES_PER_S, "forms": {}, "refused": refused}
    for key in forms:
        t, spread = best_and_spread(times[key])
        case["forms"][key] = {"s": t, "spread": round(spread, 4), "calls_per_window": inner[key]}
    hip = case["forms"]["hip"]
    hip["bytes"] = elements * HIP_BYTES_PER_ELEMENT[dtype_name]
    hip["share_of_hbm_rate"] = round(hip["bytes"] / hip["s"] / HBM_BYTES_PER_S, 4)
    for key in forms:
        if key != "hip":
            other = case["forms"][key]
            beyond = 1 + hip["spread"] + other["spread"]
            other.update({"over_hip": round(other["s"] / hip["s"], 3), "hip_wins_beyond_spread": bool(other["s"] > hip["s"] * beyond),
                          "torch_wins_beyond_spread": bool(hip["s"] > other["s"] * beyond)})
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls one timed window lasts")
    ap.add_argument("--limit", type=int, default=150, help="seconds one case may take")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.case:
        print(json.dumps(run_case(args.case, args.reps, args.window)))
        return
    res = {"reps": args.reps, "window_s": args.window, "cases": {}}  # no GPU work in this process: the cases run in children
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--window", str(args.window)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.limit} s; nothing more is started")
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit(f"{name}: exit status {out.returncode}; nothing more is started")
        res["cases"][name] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        print(f"{name}: {res['cases'][name]}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
