"""The differentiable Chamfer-type losses (nova_pointcloud_amd.losses on csrc/nearest_match.hip): argument, device and C ABI
checks (CPU), and the two kernels against a float64 restatement of their definition (GPU).

The definition restated here (include/nova_hip.h, nova_pointset_nearest_match and _bwd): the point map p clamps every
coordinate and, in unit mode, divides by max(|c|, 1e-8); the match of x_i is the smallest key (|p(x_i) - p(y_j)|^2, j); the
gradient is that of sum_i w_i |p(x_i) - p(y_idx_i)| with the indices held fixed, zero at a coincident pair. In float64: clamp
and normalisation from the float32 inputs, the full distance matrix, the index as the first column of a stable sort (the
lowest-index tie rule), the gradients by torch autograd (torch's norm has the zero subgradient at 0, torch.clamp the
inclusive mask, clamp_min the gradient 1e8 below the floor).

Bounds.
  indices, lattice      integer coordinates make every float32 operation of the forward exact: idx equals the restatement's,
                        no tolerance, and at least a fifth of the rows (shapes with M >= 255) have a tie for the minimum.
  indices, random       the kernel's idx replayed in float64 is the nearest up to REL = 1e-6 on squared distances in non-unit
                        mode (the kNN tests' derivation: 8 roundings of 6e-8 per distance, twice that per comparison) and up
                        to an absolute 1e-6 on the distance in unit mode (a unit vector's coordinates carry about 3
                        roundings, a chord about 8 * 2^-24 * sqrt(3) = 8.3e-7).
  gradients, lattice    u, g u and the sums are exact, so a term carries the square root (a relative 2^-24 on d: at most 1 ulp
                        of the value) and the division (0.5 ulp): bound 2 ulp of the float64 value per component; exact
                        zeros stay exact zeros.
  gradients, random     per component, in units of 2^-24: a term i contributes |g_i| (C1 + C2 / d_i), divided in unit mode by
                        the norm n of the clamped point the gradient lands on; a gy sum of K terms adds K sum|terms|.
                        C1 = 16, C2 = 0 (non-unit) or 16 (unit). The roundings the definition contains, non-unit: the
                        difference u (1), sqdist3 (3, with the 2 of the squared differences: 2.5 on d), the square root (1),
                        the product with g (1), the quotient (1): 6.5 <= C1. Unit mode adds, through the pull-back, the rounded unit
                        vector (norm3 1.5, its square root 1, the reciprocal 1, the product 1: 4.5 per coordinate), the dot
                        product and the fused w_k (3 + 1) and the product with inv (1): typical errors add in quadrature
                        and stay below C1; and two rounded unit vectors are subtracted, 4.5 each on a chord of length d,
                        entering u and d alike: C2 = 16 covers 9 / d twice over in quadrature.
Every element of every output is compared.

Shapes (B, N, M): the ones the issue lists, and both sides of every boundary of the kernels as built:
  forward   256 queries per workgroup: N = 255 | 256 | 257;  1024 targets per LDS tile: M = 1023 | 1024 | 1025, 2048 | 2049
  gx        256 points per workgroup: N = 255 | 256 | 257
  gy        256 targets per workgroup: M = 255 | 256 | 257;  1024 match records per LDS tile: N = 1023 | 1024 | 1025,
            2048 | 2049."""
import ctypes
import functools
import math

import pytest
import torch

EPS = 2.0 ** -24
REL = 1e-6
C1 = 16.0
SHAPES = [(3, 1, 1), (2, 1, 300), (2, 300, 1), (2, 255, 255), (2, 256, 256), (2, 257, 257), (1, 65, 1023), (1, 65, 1024), (1, 65, 1025),
          (1, 257, 2049), (1, 1025, 257), (1, 2049, 300), (2, 2048, 2048),
          # the backward's record tile over i, with M on both sides of its workgroup over j
          (1, 1023, 255), (1, 1024, 256), (1, 2048, 513)]
MODES = [(None, False), (1.0, False), (1.0, True)]  # (clamp, unit_norm)


# --------------------------------------------------------------------------------------------- restatement
def point_map64(v, clamp, unit):
    c = v.double()
    if clamp is not None:
        c = c.clamp(-clamp, clamp)
    if unit:
        c = c / c.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    return c


def distances64(x, y, clamp, unit):
    """[B, N, M] float64 squared distances of the mapped points."""
    p, q = point_map64(x, clamp, unit), point_map64(y, clamp, unit)
    d = torch.zeros(x.shape[0], x.shape[1], y.shape[1], dtype=torch.float64, device=x.device)
    for c in range(3):
        d += (p[:, :, None, c] - q[:, None, :, c]) ** 2
    return d


def restated_match(x, y, clamp=None, unit=False):
    """(d float64 [B, N], idx int64 [B, N], the sorted squared distances [B, N, M])."""
    vals, order = torch.sort(distances64(x, y, clamp, unit), dim=-1, stable=True)
    return vals[..., 0].sqrt(), order[..., 0].contiguous(), vals


def restated_grads(x, y, idx, w, clamp=None, unit=False):
    """(gx, gy, d) in float64: torch autograd on sum_i w_i |p(x_i) - p(y_idx_i)| with the indices given."""
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    p, q = point_map64(x64, clamp, unit), point_map64(y64, clamp, unit)
    d = (p - torch.gather(q, 1, idx[:, :, None].expand(-1, -1, 3))).norm(dim=-1)
    gx, gy = torch.autograd.grad((w.double() * d).sum(), (x64, y64))
    return gx, gy, d.detach()


def grad_bounds(x, y, idx, w, d, clamp, unit):
    """The per-component bounds of the module docstring on (gx, gy): tensors [B, N, 1] and [B, M, 1]."""
    c2 = 16.0 if unit else 0.0
    term = w.double().abs() * (C1 + c2 / d) * EPS  # [B, N]
    size = w.double().abs()
    norm = lambda v: point_map64(v, clamp, False).norm(dim=-1).clamp_min(1e-8) if unit else torch.ones_like(v[..., 0], dtype=torch.float64)
    zeros = torch.zeros(y.shape[0], y.shape[1], dtype=torch.float64, device=y.device)
    count = zeros.scatter_add(1, idx, torch.ones_like(term))
    by = (zeros.scatter_add(1, idx, term) + count * EPS * zeros.scatter_add(1, idx, size)) / norm(y)
    return (term / norm(x))[..., None], by[..., None]


def lattice(B, N, seed, half=8):
    return torch.randint(-half, half, (B, N, 3), generator=torch.Generator().manual_seed(seed)).float()


def clouds(B, N, seed):
    return 0.5 * torch.randn(B, N, 3, generator=torch.Generator().manual_seed(seed))


def integer_weights(B, N, seed):
    return torch.randint(-3, 4, (B, N), generator=torch.Generator().manual_seed(seed)).float()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ulp32(v):
    """The float32 spacing at the magnitude of the float64 values v (0 at 0)."""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 24))


def test_restatement_on_hand_cases():
    one = lambda *pts: torch.tensor([list(map(list, pts))], dtype=torch.float32)
    # ties go to the lowest index; a coincident pair gives a zero gradient
    x, y = one((0, 0, 0), (2, 0, 0), (5, 5, 5)), one((1, 0, 0), (-1, 0, 0), (5, 5, 5), (3, 0, 0))
    d, idx, _ = restated_match(x, y)
    assert idx.tolist() == [[0, 0, 2]] and d.tolist() == [[1.0, 1.0, 0.0]]
    gx, gy, _ = restated_grads(x, y, idx, torch.tensor([[1.0, 2.0, 7.0]]))
    # two x matched to one y: gy is the sum of the two terms; the coincident pair adds nothing on either side
    assert gx.tolist() == [[[-1.0, 0, 0], [2.0, 0, 0], [0, 0, 0]]]
    assert gy.tolist() == [[[1.0 - 2.0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]]
    # a coordinate beyond the clamp gets zero in that coordinate only; a coordinate ON the bound keeps its gradient
    x, y = one((3.0, 0.5, 1.0)), one((0.0, 0.0, 0.0))
    d, idx, _ = restated_match(x, y, clamp=1.0)
    gx, gy, _ = restated_grads(x, y, idx, torch.ones(1, 1), clamp=1.0)
    assert d.item() == pytest.approx(1.5) and gx[0, 0, 0].item() == 0.0 and gx[0, 0, 1].item() == pytest.approx(1 / 3)
    assert gx[0, 0, 2].item() == pytest.approx(2 / 3) and gy[0, 0].tolist() == pytest.approx([-2 / 3, -1 / 3, -2 / 3])
    # unit mode: a radial perturbation of x changes nothing, so the gradient is orthogonal to x; and below the floor it is 1e8 t
    x, y = one((0.3, -0.4, 0.2), (0.1, 0.1, 0.7)), one((0.5, 0.5, 0.1), (-0.2, 0.6, 0.3))
    _, idx, _ = restated_match(x, y, clamp=1.0, unit=True)
    gx, gy, _ = restated_grads(x, y, idx, torch.tensor([[1.0, -2.0]]), clamp=1.0, unit=True)
    assert float((gx * x.double()).sum(-1).abs().max()) < 1e-15 and float((gy * y.double()).sum(-1).abs().max()) < 1e-15
    assert float(gx.abs().max()) > 0.1
    tiny = one((1e-9, 0.0, 0.0))
    gx, _, d = restated_grads(tiny, one((0.0, 1.0, 0.0)), torch.zeros(1, 1, dtype=torch.long), torch.ones(1, 1), clamp=1.0, unit=True)
    assert gx[0, 0].tolist() == pytest.approx([1e8 * 0.1 / d.item(), 1e8 * -1.0 / d.item(), 0.0], rel=1e-6)  # p = (0.1, 0, 0): u = (0.1, -1, 0)
    # the lattice of the exact tests has the ties they are for
    for N, M in ((300, 300), (257, 1025), (65, 2049)):
        vals = restated_match(lattice(1, N, 5000 + N), lattice(1, M, 6000 + M))[2]
        assert float((vals[..., 0] == vals[..., 1]).double().mean()) >= 0.2


def restated_descent(x, y, lr, steps):
    x = x.double()
    values = []
    for _ in range(steps + 1):
        ixy, iyx = restated_match(x, y)[1], restated_match(y, x)[1]
        a, _, dxy = restated_grads(x, y, ixy, torch.full(ixy.shape, 1.0 / ixy.numel()))
        _, b, dyx = restated_grads(y, x, iyx, torch.full(iyx.shape, 1.0 / iyx.numel()))
        values.append(float(dxy.mean() + dyx.mean()))
        x = x - lr * (a + b)
    return values


DESCENT_LR = 1.0


def test_descent_step_size_on_the_restatement():
    values = restated_descent(clouds(1, 64, 71), clouds(1, 64, 72), DESCENT_LR, 10)
    assert all(b < a for a, b in zip(values, values[1:])), values


# --------------------------------------------------------------------------------------------- CPU: checks
def test_input_errors_on_cpu_tensors():
    from nova_pointcloud_amd import hip, losses

    ok, other = torch.zeros(2, 8, 3), torch.zeros(2, 5, 3)
    for fn in (losses.nearest_match, losses.dist_chamfer, losses.chamfer_loss, losses.edge_consistency_loss):
        with pytest.raises(ValueError, match="expected a tensor"):
            fn([[0.0, 0, 0]], ok)
        with pytest.raises(ValueError, match="expected a tensor"):
            fn(ok, None)
        for bad in (torch.zeros(2, 8, 2), torch.zeros(8, 3), torch.zeros(2, 8, 3, 1)):
            with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
                fn(bad, ok)
            with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
                fn(ok, bad)
        with pytest.raises(ValueError, match="same number of clouds"):
            fn(ok, torch.zeros(3, 8, 3))
        with pytest.raises(ValueError, match="finite"):
            fn(torch.full((2, 4, 3), float("nan")), ok)
        with pytest.raises(ValueError, match="finite"):
            fn(ok, torch.tensor([[[0.0, 0, 0], [float("inf"), 0, 0]]] * 2))
        with pytest.raises(ValueError, match="floating"):
            fn(torch.zeros(2, 8, 3, dtype=torch.int64), ok)
        with pytest.raises(hip.NovaHipError, match="GPU"):  # valid CPU tensors: no CPU path
            fn(ok, other)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="same device"):
            losses.nearest_match(ok.cuda(), other)
    with pytest.raises(ValueError, match="at least one point"):
        losses.nearest_match(ok, torch.zeros(2, 0, 3))
    for bad in (0, -1.0, float("inf"), float("nan"), True, "1"):
        with pytest.raises(ValueError, match="clamp must be"):
            losses.nearest_match(ok, other, clamp=bad)
    with pytest.raises(ValueError, match="unit_norm"):
        losses.nearest_match(ok, other, unit_norm=1)
    with pytest.raises(ValueError, match="return_indices"):
        losses.nearest_match(ok, other, return_indices=None)
    for bad in (0, -2, 1.0, True):
        with pytest.raises(ValueError, match="max_clouds_per_launch"):
            losses.nearest_match(ok, other, max_clouds_per_launch=bad)
    with pytest.raises(hip.NovaHipError, match="GPU"):
        losses.nearest_match(ok.requires_grad_(True), other, clamp=1.0, unit_norm=True, return_indices=True, max_clouds_per_launch=1)
    with pytest.raises(ValueError, match=r"generated_subsets\[1\]"):
        losses.autoregressive_consistency_loss([ok, torch.zeros(2, 8)], [ok, ok])
    with pytest.raises(hip.NovaHipError, match="GPU"):
        losses.autoregressive_consistency_loss([ok, other], [ok, other])


def test_abi_rejections():
    """Argument checks of the two entry points run before any device work (no GPU needed)."""
    from nova_pointcloud_amd import hip

    lib = hip.load(check_device=False)
    assert "nova_pointset_nearest_match" in hip.SIGNATURES and "nova_pointset_nearest_match_bwd" in hip.SIGNATURES
    inf = math.inf
    p = [ctypes.c_void_p(4096 * i) for i in range(1, 7)]  # never dereferenced: rejected first
    fwd = lambda ptrs, B, N, M, lo=-inf, hi=inf: lib.nova_pointset_nearest_match(*ptrs, B, N, M, lo, hi, 0, None)
    bwd = lambda ptrs, B, N, M, lo=-inf, hi=inf: lib.nova_pointset_nearest_match_bwd(*ptrs, B, N, M, lo, hi, 1, None)
    for fn, n, name in ((fwd, 4, b"pointset_nearest_match:"), (bwd, 6, b"pointset_nearest_match_bwd:")):
        ptrs = p[:n]
        assert fn(ptrs, 2, 8, 0) == -2 and b"empty target set" in lib.nova_last_error() and name in lib.nova_last_error()
        assert fn(ptrs, 2, 8, -1) == -2
        assert fn(ptrs, 65536, 8, 8) == -2 and b"65536" in lib.nova_last_error()
        for k in range(n):
            assert fn(ptrs[:k] + [None] + ptrs[k + 1:], 2, 8, 8) == -1 and b"null" in lib.nova_last_error()
        assert fn(ptrs, 2, 8, 8, 1.0, -1.0) == -1 and b"clamp" in lib.nova_last_error()
        assert fn(ptrs, 2, 8, 8, float("nan"), 1.0) == -1
        assert fn([None] * n, 0, 8, 8) == 0 and fn([None] * n, 2, 0, 8) == 0 and fn([None] * n, -3, 8, 0) == 0  # nothing to do
        assert fn([None] * n, 0, 8, 8, 1.0, -1.0) == -1  # but the clamp range is still checked


def test_point_cloud_loss_without_points_and_empty_subsets():
    from nova_pointcloud_amd import losses

    scheduler = object()
    loss = losses.PointCloudLoss(scheduler)
    assert loss.scheduler is scheduler and isinstance(loss, torch.nn.Module)
    assert (loss.cd_weight, loss.emd_weight, loss.diffusion_weight, loss.autoregressive_weight, loss.edge_alignment_weight,
            loss.emd_assignment) == (0.1, 0.05, 1.0, 0.2, 0.1, "host")
    with pytest.raises(ValueError, match="assignment"):
        losses.PointCloudLoss(None, emd_assignment="gpu")
    g = torch.Generator().manual_seed(5)
    pred, target = torch.randn(2, 16, 3, generator=g).requires_grad_(True), torch.randn(2, 16, 3, generator=g)
    pts = torch.randn(2, 16, 3, generator=g)
    for kwargs in (dict(use_only_diffusion=True, pred_points=pts, target_points=pts), dict(), dict(pred_points=pts),
                   dict(target_points=pts, generated_subsets=[pts], target_subsets=[pts])):
        loss = losses.PointCloudLoss(None, diffusion_weight=0.5)
        total = loss(pred, target, **kwargs)
        want = 0.5 * torch.nn.functional.mse_loss(pred, target)
        assert torch.equal(total, want) and total.requires_grad
        assert loss.last_components == {"diffusion_loss": float(want.detach()) * 2, "total_loss": float(want.detach())}
    bad = pred.detach().clone()
    bad[0, 0, 0] = float("nan")
    loss = losses.PointCloudLoss(None)
    assert float(loss(bad, target)) == pytest.approx(0.1) and loss.last_components["diffusion_loss"] == pytest.approx(0.1)
    # empty subset lists: the reference's tensor 0.0, on the CPU when there is nothing to take a device from
    for gen, tgt in (([], []), ([], [pts]), ([pts], [])):
        zero = losses.autoregressive_consistency_loss(gen, tgt)
        assert torch.is_tensor(zero) and zero.shape == () and float(zero) == 0.0 and zero.device == pts.device
    assert float(losses.autoregressive_consistency_loss([pts], [pts])) == 0.0  # one subset: no pair
    assert isinstance(losses.stats["nearest_match_launches"], int)


# --------------------------------------------------------------------------------------------- GPU
def run(x, y, w, clamp=None, unit=False, **kw):
    """(d, idx, gx, gy) of nearest_match and its backward under the output weights w."""
    from nova_pointcloud_amd import losses

    x, y = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    d, idx = losses.nearest_match(x, y, clamp, unit, return_indices=True, **kw)
    B, N = x.shape[0], x.shape[1]
    assert d.shape == (B, N) and d.dtype == torch.float32 and d.device == x.device and d.requires_grad
    assert idx.shape == (B, N) and idx.dtype == torch.int64 and not idx.requires_grad
    d.backward(w.to(d.dtype))
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and y.grad.shape == y.shape and y.grad.dtype == y.dtype
    return d.detach(), idx, x.grad, y.grad


@functools.lru_cache(maxsize=None)
def lattice_case(B, N, M):
    """(x, y, w, restated idx, tie share, gx64, gy64, matches per y) of the exact tests at one shape; computed once, never modified.
    The lattice is narrowed to -4 .. 3 where -8 .. 7 leaves fewer than a fifth of the rows with a tie."""
    for half in (8, 4):
        x, y = lattice(B, N, 5000 + N, half).cuda(), lattice(B, M, 6000 + M, half).cuda()
        _, idx, vals = restated_match(x, y)
        tied = float((vals[..., 0] == vals[..., 1]).double().mean()) if M > 1 else 0.0
        if tied >= 0.2 or M < 255:
            break
    w = integer_weights(B, N, 7000 + N).cuda()
    gx, gy, _ = restated_grads(x, y, idx, w)
    count = torch.zeros(B, M, device="cuda").scatter_add(1, idx, torch.ones(B, N, device="cuda"))
    return x, y, w, idx, tied, gx, gy, count


@functools.lru_cache(maxsize=None)
def random_case(B, N, M, clamp, unit):
    """(x, y, w, float64 squared distances) of the random tests at one shape and mode; computed once, never modified."""
    x, y = clouds(B, N, 100 + N).cuda(), clouds(B, M, 200 + M).cuda()
    w = torch.randn(B, N, generator=torch.Generator().manual_seed(300 + N)).cuda()
    return x, y, w, distances64(x, y, clamp, unit)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_forward_is_nn_dist_bit_for_bit(hip, B, N, M):
    from nova_pointcloud_amd import losses, metrics

    x, y = clouds(B, N, 100 + N).cuda(), clouds(B, M, 200 + M).cuda()
    for unit in (False, True):
        d = losses.nearest_match(x, y, 1.0, unit)
        assert not d.requires_grad and bits_equal(d, metrics.nn_dist(x, y, 1.0, unit_norm=unit))
    x, y = lattice_case(B, N, M)[:2]
    assert bits_equal(losses.nearest_match(x, y, 20.0), metrics.nn_dist(x, y, 20.0))


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_lattice_indices_and_gradients(hip, B, N, M):
    x, y, w, want_idx, tied, gx64, gy64, count = lattice_case(B, N, M)
    d, idx, gx, gy = run(x, y, w)
    print(f"lattice B {B} N {N} M {M}: share of rows with a tie for the minimum {tied:.2f}, "
          f"rows with another index {int((idx != want_idx).sum())}")
    if M >= 255:
        assert tied >= 0.2
    assert torch.equal(idx, want_idx)
    single = (count == 1)[..., None].expand_as(gy)
    err_x, err_y = (gx.double() - gx64).abs() / ulp32(gx64).clamp_min(1e-300), (gy.double() - gy64).abs() / ulp32(gy64).clamp_min(1e-300)
    print(f"  largest error in ulp of the float64 value: gx {float(err_x[gx64 != 0].max()) if bool((gx64 != 0).any()) else 0:.2f}, "
          f"gy at single matches {float(err_y[single & (gy64 != 0)].max()) if bool((single & (gy64 != 0)).any()) else 0:.2f}")
    assert bool((gx[gx64 == 0] == 0).all()) and bool(((gx.double() - gx64).abs() <= 2 * ulp32(gx64)).all())
    assert bool((gy[(count == 0)[..., None].expand_as(gy)] == 0).all())
    assert bool((gy[single & (gy64 == 0)] == 0).all())
    assert bool((((gy.double() - gy64).abs() <= 2 * ulp32(gy64)) | ~single).all())
    # y points with several matches: the bound of the random test (non-unit mode, no clamp)
    d64 = restated_grads(x, y, idx, w)[2]
    far = d64 > 0  # a coincident pair contributes an exact zero on both sides
    _, by = grad_bounds(x, y, idx, torch.where(far, w, torch.zeros_like(w)), torch.where(far, d64, torch.ones_like(d64)), None, False)
    assert bool(((gy.double() - gy64).abs() <= by).all())


@pytest.mark.gpu
@pytest.mark.parametrize("clamp,unit", MODES[1:])
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_random_indices_and_gradients(hip, B, N, M, clamp, unit):
    x, y, w, d2 = random_case(B, N, M, clamp, unit)
    d, idx, gx, gy = run(x, y, w, clamp, unit)
    assert bool((idx >= 0).all()) and bool((idx < M).all())
    got, best = d2.gather(-1, idx[..., None])[..., 0], d2.min(dim=-1).values
    assert float(best.min()) > 0
    if unit:
        print(f"unit B {B} N {N} M {M}: largest excess of a chosen distance over the nearest {float((got.sqrt() - best.sqrt()).max()):.3e}, "
              f"largest error of a distance {float((d.double() - got.sqrt()).abs().max()):.3e} (bounds 1e-6 absolute)")
        assert bool((got.sqrt() <= best.sqrt() + 1e-6).all()) and bool(((d.double() - got.sqrt()).abs() <= 1e-6).all())
    else:
        print(f"non-unit B {B} N {N} M {M}: largest relative excess of a chosen squared distance over the nearest "
              f"{float((got / best).max()) - 1:.3e}, largest relative error of a distance {float(((d.double() - got.sqrt()).abs() / got.sqrt()).max()):.3e} "
              f"(bounds {REL:.0e})")
        assert bool((got <= best * (1 + REL)).all()) and bool(((d.double() - got.sqrt()).abs() <= REL * got.sqrt()).all())
    gx64, gy64, d64 = restated_grads(x, y, idx, w, clamp, unit)
    bx, by = grad_bounds(x, y, idx, w, d64, clamp, unit)
    ex, ey = (gx.double() - gx64).abs(), (gy.double() - gy64).abs()
    print(f"  largest error over its bound: gx {float((ex / bx).max()):.3f}, gy {float((ey / by.clamp_min(1e-300)).max()):.3f}; "
          f"share of clamped coordinates {float((x.abs() > clamp).double().mean()):.3f}")
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())
    assert bool((ex <= bx).all()) and bool((ey <= by).all())
    beyond = x.abs() > clamp
    assert bool((gx[beyond] == 0).all()) and bool((gy[y.abs() > clamp] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,M,seed", [(2, 300, 300, 1), (1, 1025, 257, 2)])
def test_edge_consistency_against_dense_autograd(hip, B, N, M, seed):
    from nova_pointcloud_amd import losses

    x, y = clouds(B, N, 400 + seed).cuda(), clouds(B, M, 500 + seed).cuda()
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    dist = torch.cdist(x64, y64, compute_mode="donot_use_mm_for_euclid_dist")
    near = dist.detach().sort(dim=-1).values
    margin = float(((near[..., 1] - near[..., 0]) / near[..., 0]).min())
    print(f"B {B} N {N} M {M}: smallest relative margin between nearest and second nearest {margin:.2e}")
    assert margin > 1e-5  # the reference's own argmin is unambiguous
    want = dist.min(dim=2).values.mean()
    gx64, gy64 = torch.autograd.grad(want, (x64, y64))
    xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    got = losses.edge_consistency_loss(xs, ys)
    got.backward()
    got, want = got.detach(), want.detach()
    idx = dist.detach().argmin(dim=2)
    w = torch.full((B, N), 1.0 / (B * N), device="cuda")
    bx, by = grad_bounds(x, y, idx, w, dist.detach().min(dim=2).values, None, False)
    print(f"  value error {abs(float(got) - float(want)):.3e} (bound {C1 * EPS * float(want):.3e}); largest error over its bound: "
          f"gx {float(((xs.grad.double() - gx64).abs() / bx).max()):.3f}, gy {float(((ys.grad.double() - gy64).abs() / by.clamp_min(1e-300)).max()):.3f}")
    # every distance carries 3.5 roundings and the float32 mean's pairwise tree log2(B N) <= 11 more: within C1 in all
    assert abs(float(got) - float(want)) <= C1 * EPS * float(want)
    assert bool(((xs.grad.double() - gx64).abs() <= bx).all()) and bool(((ys.grad.double() - gy64).abs() <= by).all())


def literal_dist_chamfer64(a, b):
    """distChamfer of train_newloss.py:316-349, statement by statement, in float64."""
    x, y = torch.clamp(a.double(), -1.0, 1.0), torch.clamp(b.double(), -1.0, 1.0)
    x = x / torch.clamp(torch.norm(x, dim=-1, keepdim=True), min=1e-8)
    y = y / torch.clamp(torch.norm(y, dim=-1, keepdim=True), min=1e-8)
    dist = torch.clamp(torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist"), min=1e-8)
    log_dist = torch.clamp(torch.log(dist + 1e-8), min=-10, max=10)
    return log_dist.min(2)[0].exp().mean(), log_dist.min(1)[0].exp().mean()


@pytest.mark.gpu
def test_loss_values(hip):
    from nova_pointcloud_amd import losses, metrics

    for B, N, M in ((2, 300, 300), (1, 1025, 257), (2, 256, 2049)):
        a, b = clouds(B, N, 600 + N).cuda(), clouds(B, M, 700 + M).cuda()
        with torch.no_grad():
            dl, dr = losses.dist_chamfer(a, b)
            ml, mr = metrics.distChamfer(a, b)
            assert bits_equal(dl, ml) and bits_equal(dr, mr)
            loss = losses.chamfer_loss(a, b)
            assert bits_equal(loss, metrics.robust_chamfer_distance(a, b))
        wl, wr = literal_dist_chamfer64(a, b)
        print(f"B {B} N {N} M {M}: chamfer_loss {float(loss):.7f}, error against the literal float64 form {abs(float(loss) - float((wl + wr) / 2)):.3e} (bound 2e-6)")
        assert abs(float(dl) - float(wl)) <= 2e-6 and abs(float(dr) - float(wr)) <= 2e-6
        assert abs(float(loss) - float((wl + wr) / 2)) <= 2e-6
        a.requires_grad_(True)
        with pytest.raises(hip.NovaHipError, match="evaluation-only"):  # metrics stays as it is
            metrics.distChamfer(a, b)
        assert bits_equal(losses.chamfer_loss(a, b).detach(), loss)


@pytest.mark.gpu
def test_coincident_clouds(hip):
    from nova_pointcloud_amd import losses

    for N in (1, 300, 1025):
        a = clouds(2, N, 800 + N).cuda().requires_grad_(True)
        b = a.detach().clone().requires_grad_(True)
        for fn in (losses.chamfer_loss, losses.edge_consistency_loss):
            a.grad = b.grad = None
            value = fn(a, b)
            value.backward()
            assert math.isfinite(float(value))
            assert bool((a.grad == 0).all()) and bool((b.grad == 0).all())
    assert float(losses.edge_consistency_loss(a, b)) == 0.0


@pytest.mark.gpu
def test_invariance(hip):
    B, N, M = 3, 300, 1100
    x, y = clouds(B, N, 901).cuda(), clouds(B, M, 902).cuda()
    w = torch.randn(B, N, generator=torch.Generator().manual_seed(903)).cuda()
    perm = torch.tensor([2, 0, 1], device="cuda")
    for clamp, unit in MODES:
        base = run(x, y, w, clamp, unit)
        same = lambda got, sel=slice(None): all(torch.equal(g, b[sel]) if g.dtype == torch.int64 else bits_equal(g, b[sel].contiguous())
                                                for g, b in zip(got, base))
        assert same(run(x, y, w, clamp, unit))  # a second run
        for per in (1, 2, B):
            assert same(run(x, y, w, clamp, unit, max_clouds_per_launch=per)), per
        assert same(run(x[perm], y[perm], w[perm], clamp, unit), perm)
        for s in range(B):
            assert same(run(x[s:s + 1], y[s:s + 1], w[s:s + 1], clamp, unit), slice(s, s + 1)), s
    for dtype in (torch.bfloat16, torch.float16):
        xh, yh = x.to(dtype), y.to(dtype)
        d, idx, gx, gy = run(xh, yh, w, 1.0, True)
        assert gx.dtype == dtype and gy.dtype == dtype and d.dtype == torch.float32
        d32, idx32, gx32, gy32 = run(xh.float(), yh.float(), w, 1.0, True)
        assert bits_equal(d, d32) and torch.equal(idx, idx32)
        assert torch.equal(gx, gx32.to(dtype)) and torch.equal(gy, gy32.to(dtype))  # the float32 gradient, rounded once


@pytest.mark.gpu
def test_autoregressive_launch_count(hip):
    from nova_pointcloud_amd import losses

    cloud = clouds(2, 2048, 950).cuda()
    sizes = [102] * 19 + [110]
    leaves = [s.clone().requires_grad_(True) for s in cloud.split(sizes, dim=1)]
    before = losses.stats["nearest_match_launches"]
    value = losses.autoregressive_consistency_loss(leaves, leaves)
    assert losses.stats["nearest_match_launches"] - before == 2  # 171 pairs of (102, 102) and 19 of (102, 110)
    value.backward()
    again = [s.detach().clone().requires_grad_(True) for s in leaves]
    total, terms = 0.0, [torch.zeros(2, n, device="cuda") for n in sizes]
    for i in range(19):
        for j in range(i + 1, 20):
            total = total + losses.edge_consistency_loss(again[i], again[j])
            with torch.no_grad():
                idx = losses.nearest_match(again[i], again[j], return_indices=True)[1]
            terms[i] += 1
            terms[j].scatter_add_(1, idx, torch.ones(2, sizes[i], device="cuda"))
    assert losses.stats["nearest_match_launches"] - before == 2 + 2 * 190
    total = total / 190
    total.backward()
    print(f"autoregressive: stacked {float(value):.8f}, pair by pair {float(total):.8f}")
    # both are float32 sums of the same 190 means in two orders: a mean of 204 or 220 distances is a pairwise tree of depth 8 either
    # way (2 x 8 roundings), the sums add one rounding per addition (2 x 190), the division by 190 one
    assert abs(float(value) - float(total)) <= (16 + 380 + 2) * EPS * float(total)
    g = 1.0 / (190 * 2 * 102)  # the largest weight of a term
    for s, (a, b) in enumerate(zip(leaves, again)):
        # T terms of at most g land on a point: each within C1 g 2^-24 of its value, and two orders of adding T of them
        bound = (g * terms[s] * (C1 + terms[s]) * EPS)[..., None]
        assert bool(((a.grad.double() - b.grad.double()).abs() <= bound).all()), s


@pytest.mark.gpu
def test_point_cloud_loss_end_to_end(hip):
    from nova_pointcloud_amd import losses, metrics

    g = torch.Generator().manual_seed(960)
    noise_pred, noise_target = torch.randn(2, 256, 3, generator=g).cuda(), torch.randn(2, 256, 3, generator=g).cuda()
    points, target = clouds(2, 256, 961).cuda(), clouds(2, 256, 962).cuda()

    def call(module):
        pred = points.clone().requires_grad_(True)
        subsets = list(pred.split(64, dim=1))
        total = module(noise_pred, noise_target, pred_points=pred, target_points=target, generated_subsets=subsets,
                       target_subsets=list(target.split(64, dim=1)))
        total.backward()
        return total.detach(), pred.grad, pred

    module = losses.PointCloudLoss(None)
    total, grad, pred = call(module)
    mse = torch.nn.functional.mse_loss(noise_pred, noise_target)
    cd = losses.chamfer_loss(pred, target)
    emd = metrics.robust_emd(points, target)
    ar = losses.autoregressive_consistency_loss(list(pred.split(64, dim=1)), [target])
    want = 1.0 * mse + 0.1 * cd + 0.05 * emd + 0.2 * ar
    assert bits_equal(total, want.detach())
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    assert module.last_components == {"diffusion_loss": float(mse), "cd_loss": float(cd), "emd_loss": float(emd),
                                      "autoregressive_loss": float(ar), "total_loss": float(want)}
    assert all(isinstance(v, float) for v in module.last_components.values()) and float(emd) > 0
    other_total, other_grad, _ = call(losses.PointCloudLoss(None, emd_weight=3.0))
    assert float(other_total) > float(total) and bits_equal(other_grad, grad)  # the EMD term is a constant
    device_total, device_grad, _ = call(losses.PointCloudLoss(None, emd_assignment="device"))
    # metrics.emd_approx: the device assignment's mean is within 2^-18 + 1e-8 of the host's; four float32 additions on top
    assert abs(float(device_total) - float(total)) <= 0.05 * (metrics.ASSIGN_QUANTUM + 1e-8) + 4 * EPS * float(total)
    assert bits_equal(device_grad, grad)
    # unequal point counts: both cut to the smaller one
    short = losses.PointCloudLoss(None)
    value = short(noise_pred, noise_target, pred_points=points.clone().requires_grad_(True), target_points=target[:, :200])
    assert math.isfinite(float(value)) and short.last_components["autoregressive_loss"] == 0.0


@pytest.mark.gpu
def test_descent(hip):
    from nova_pointcloud_amd import losses

    x, y = clouds(1, 64, 71).cuda(), clouds(1, 64, 72).cuda()
    values = []
    for _ in range(11):
        x = x.detach().requires_grad_(True)
        value = losses.edge_consistency_loss(x, y) + losses.edge_consistency_loss(y, x)
        value.backward()
        values.append(float(value))
        x = x - DESCENT_LR * x.grad
    print("descent:", " ".join(f"{v:.5f}" for v in values))
    assert all(b < a for a, b in zip(values, values[1:])), values
