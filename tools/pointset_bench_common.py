"""Seeded inputs and device-event timers shared by the point-set bench tools (chamfer_matrix_bench, emd_matrix_bench,
fps_bench, assignment_bench, knn_bench, interp_bench, chamfer_loss_bench, interp_grad_bench, emd_loss_bench, neighbor_bench, soft_cluster_bench, posenc_bench, point_embed_bench, point_head_bench, dropout_add_bench). torch is imported on first use: knn_bench's and interp_bench's parent
processes do no GPU work."""


def ball_clouds(S, N, seed):
    """Points in the ball of radius 0.5, denser towards the centre (a shape-like, non-uniform cloud)."""
    import torch

    g = torch.Generator().manual_seed(seed)
    p = torch.randn(S, N, 3, generator=g)
    return (p / p.norm(dim=-1, keepdim=True) * 0.5 * torch.rand(S, N, 1, generator=g)).cuda()


def shell_clouds(S, n, seed):
    """Noisy unit spheres, each cloud with a scale and an offset of its own."""
    import torch

    g = torch.Generator().manual_seed(seed)
    p = torch.randn(S, n, 3, generator=g)
    p = p / p.norm(dim=-1, keepdim=True) * (1 + 0.05 * torch.randn(S, n, 1, generator=g))
    p = p * (0.5 + torch.rand(S, 1, 3, generator=g)) + 0.2 * torch.randn(S, 1, 3, generator=g)  # per-shape scale / offset
    return p.cuda()


def timed_once(fn):
    """(result, seconds) of one call between two device events."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) / 1e3


def timed(fn, reps):
    """(result, best seconds, (max - min) / min) over `reps` calls, each between two device events."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return out, min(times), (max(times) - min(times)) / min(times)


def window(fn, inner):
    """(result, seconds per call) of `inner` calls in a row between two device events."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) / 1e3 / inner


def calls_per_window(fn, seconds):
    """How many calls in a row last about `seconds` (from one warm call)."""
    return max(1, int(seconds / max(window(fn, 1)[1], 1e-6)) + 1)


def best_and_spread(times):
    return min(times), (max(times) - min(times)) / min(times)
