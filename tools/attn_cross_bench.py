"""Cross-length training attention, forward + backward of `autograd.attention` (csrc/attn16.hip, attn_bwd.hip through
nova_attn_cross_fwd_lse / nova_attn_cross_bwd, with the layout copies the binding makes) against PyTorch's SDPA forward +
backward on the same bf16 tensors, at EdgeAligner's shapes (transformer_pointcloud_nova.py:211-215, 12 heads x 64): 2048 points
in 20 subsets - 102 queries against the 1938 keys of the 19 earlier subsets, batch 32 - and 15 000 points - 750 against
14 250, batch 1 - each beside the self-attention call of the same query count. The two forms alternate; per form the best of
5 rounds and the spread (max - min) over them. Writes profiles/attn_cross_bench.json (or the path given as argument)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nova_pointcloud_amd import autograd as A, hip  # noqa: E402

if os.environ.get("NOVA_HIP_LIB"):  # A/B another build of the library
    hip._LIB_PATH = os.environ["NOVA_HIP_LIB"]
from microbench import timeit  # noqa: E402

H, D = 12, 64
SHAPES = ((32, 102, 1938), (32, 102, 102), (1, 750, 14250), (1, 750, 750))
ROUNDS = 5


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "attn_cross_bench.json")
    rows = []
    for (S, Lq, Lk) in SHAPES:
        g = torch.Generator().manual_seed(0)
        mk = lambda L: torch.randn(S, H, L, D, generator=g).bfloat16().cuda()
        q, k, v, do = mk(Lq), mk(Lk), mk(Lk), mk(Lq)
        forms = {"hip": A.attention, "torch": torch.nn.functional.scaled_dot_product_attention}
        leaves = {}
        for name in forms:
            leaves[name] = tuple(t.clone().requires_grad_(True) for t in (q, k, v))
        step = lambda name: forms[name](*leaves[name]).backward(do)
        ms = {name: [] for name in forms}
        for _ in range(ROUNDS):
            for name in forms:  # alternate the two forms
                ms[name].append(timeit(lambda: step(name), iters=10, warm=3))
        best = {name: min(t) for name, t in ms.items()}
        spread = {name: max(t) - min(t) for name, t in ms.items()}
        flop = 3.5 * 4.0 * S * H * Lq * Lk * D  # forward 4 S h Lq Lk d, backward 2.5 times that (algorithmic)
        row = dict(S=S, heads=H, head_dim=D, Lq=Lq, Lk=Lk, hip_ms=round(best["hip"], 4), hip_spread_ms=round(spread["hip"], 4),
                   torch_ms=round(best["torch"], 4), torch_spread_ms=round(spread["torch"], 4),
                   torch_over_hip=round(best["torch"] / best["hip"], 3), hip_tflops=round(flop / best["hip"] / 1e9, 1),
                   dq_workgroups=((Lq + 127) // 128) * H * S, dkv_workgroups=((Lk + 127) // 128) * H * S,
                   all_rounds_ms={name: [round(x, 4) for x in t] for name, t in ms.items()})
        rows.append(row)
        print(f"S={S} Lq={Lq} Lk={Lk}: forward + backward HIP {best['hip']:.3f} ms (spread {spread['hip']:.3f})  torch {best['torch']:.3f} ms "
              f"(spread {spread['torch']:.3f})  torch / HIP {row['torch_over_hip']:.2f}", flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rounds=ROUNDS, iters_per_round=10, what="forward + backward, bf16, best of rounds",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
