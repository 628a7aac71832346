"""Fused L1 + D-SSIM (gs_loss_forward / gs_loss_backward) against a plain
PyTorch fp32 statement of the reference's formula (src/core/loss.py:9-63,
completed with the missing `return 1 - ssim.mean()`), forward values and
autograd gradients.  The reference SSIMLoss itself returns None, so this
row's parity is pinned to the formula, not to reference outputs."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def torch_loss(pred, target, lam=0.2, K=11):
    """loss.py:17-39 + :56-58 in fp32 (pred/target [C,H,W])."""
    x = torch.arange(K, device=pred.device).float() - (K - 1) / 2
    g1d = torch.exp(-x ** 2 / (2 * (K / 6) ** 2))
    g1d = (g1d / g1d.sum()).view(1, 1, K)
    pad = K // 2
    C = pred.shape[0]
    wx = g1d.unsqueeze(2).repeat(C, 1, 1, 1)  # [C,1,1,K]
    wy = g1d.unsqueeze(3).repeat(C, 1, 1, 1)  # [C,1,K,1]

    def blur(img):
        out = F.conv2d(img[None], wx, padding=(0, pad), groups=C)
        return F.conv2d(out, wy, padding=(pad, 0), groups=C)[0]

    mu_x, mu_y = blur(pred), blur(target)
    sigma_x = blur(pred ** 2) - mu_x ** 2
    sigma_y = blur(target ** 2) - mu_y ** 2
    sigma_xy = blur(pred * target) - mu_x * mu_y
    ssim = ((2 * mu_x * mu_y + 0.01 ** 2) * (2 * sigma_xy + 0.03 ** 2)) / (
        (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sigma_x + sigma_y + 0.03 ** 2))
    dssim = 1 - ssim.clamp(0, 1).mean()
    l1 = (pred - target).abs().mean()
    return (1 - lam) * l1 + lam * dssim, l1, dssim


def _pair(shape, seed, dev, blur_target=False):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g)
    t = (p + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1) if blur_target else torch.rand(shape, generator=g)
    return p.to(dev), t.to(dev)


@pytest.mark.parametrize("shape,lam,K", [((3, 64, 48), 0.2, 11), ((3, 37, 53), 0.2, 11), ((1, 5, 7), 0.5, 11),
                                         ((3, 40, 40), 1.0, 7), ((2, 33, 17), 0.0, 3), ((3, 270, 480), 0.2, 11)])
def test_fused_loss_matches_torch(pkg, cuda, shape, lam, K):
    p, t = _pair(shape, sum(shape), cuda, blur_target=True)
    p1 = p.clone().requires_grad_()
    total, l1, dssim = pkg.loss.photometric_loss(p1, t, lam, K)
    total.backward()
    p2 = p.clone().requires_grad_()
    rt, rl1, rd = torch_loss(p2, t, lam, K)
    rt.backward()
    assert math.isclose(l1.item(), rl1.item(), rel_tol=2e-6, abs_tol=1e-7)
    assert math.isclose(dssim.item(), rd.item(), rel_tol=1e-5, abs_tol=1e-6)
    assert math.isclose(total.item(), rt.item(), rel_tol=1e-5, abs_tol=1e-6)
    err = (p1.grad - p2.grad).abs().max().item()
    assert err <= 1e-3 * p2.grad.abs().max().item() + 1e-9, err


def test_modules_and_batched_input(pkg, cuda):
    p, t = _pair((1, 3, 32, 40), 3, cuda)
    d = pkg.SSIMLoss()(p, t)
    _, _, rd = torch_loss(p[0], t[0], 1.0, 11)
    assert math.isclose(d.item(), rd.item(), rel_tol=1e-5)
    total, logs = pkg.GaussianLoss(0.2)(p, t)
    rt, rl1, rd = torch_loss(p[0], t[0], 0.2, 11)
    assert set(logs) == {"l1", "dssim", "total_loss"} and all(isinstance(v, float) for v in logs.values())
    assert math.isclose(logs["total_loss"], rt.item(), rel_tol=1e-5)
    assert math.isclose(logs["l1"], rl1.item(), rel_tol=1e-5)
    # identical images: D-SSIM 0, L1 0, gradient of the L1 term 0 (sign(0) = 0)
    q = p.clone().requires_grad_()
    tot, l1, ds = pkg.loss.photometric_loss(q, p, 0.2)
    tot.backward()
    assert l1.item() == 0.0 and abs(ds.item()) < 1e-6 and q.grad.abs().max().item() < 1e-5


def test_loss_deterministic(pkg, cuda):
    p, t = _pair((3, 135, 240), 9, cuda)
    res = []
    for _ in range(2):
        q = p.clone().requires_grad_()
        tot, _, _ = pkg.loss.photometric_loss(q, t)
        tot.backward()
        res.append((tot.detach().clone(), q.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# --------------------------------------------------------------------------
# fp64 statement and the paths the fp32 comparison above never launches: every
# window radius (one kernel instantiation each), the clamp gate closed, an
# upstream gradient, the forward without maps, a non-contiguous pred, a batch.
#
# Bound: the kernel's max abs error against the fp64 statement may be at most
# 8x that of the fp32 statement above (err32, same inputs and device) plus 1e-7
# of the statement's largest magnitude -- the kernel sums the same taps by FMA
# in a fixed order, forms 1/D once and reduces in a tree: the same precision
# class with other constants.  For K = 11 the gradient bound must also stay
# under 2e-5 max|grad|, the weight of the window's corner tap.
#
# Measured on an MI355X: per window, the case (of six shapes x two lambdas)
# closest to its bound; kernel / fp32 statement, the gradient as a fraction of
# max|grad|, the scalars absolute.  The K = 11 gradient bounds came to at most
# 5.7e-6 max|grad|.
#
#   case                    grad               l1                 dssim              total
#   every window K=1        7.1e-06 / 9.9e-07  2.7e-09 / 4.7e-09  4.1e-08 / 4.1e-08  4.1e-08 / 4.1e-08
#   every window K=3        7.1e-06 / 9.7e-07  3.5e-09 / 3.5e-09  1.3e-07 / 4.7e-08  2.8e-08 / 9.2e-09
#   every window K=5        7.3e-07 / 4.8e-07  3.2e-09 / 3.2e-09  7.4e-09 / 3.8e-09  7.4e-09 / 3.8e-09
#   every window K=7        3.2e-07 / 2.1e-07  4.2e-09 / 4.2e-09  9.0e-09 / 2.2e-09  9.0e-09 / 2.2e-09
#   every window K=9        3.0e-07 / 1.7e-07  2.9e-09 / 2.9e-09  2.1e-09 / 2.4e-10  2.1e-09 / 2.4e-10
#   every window K=11       8.0e-07 / 3.4e-07  6.2e-09 / 1.2e-09  1.7e-08 / 2.1e-09  1.7e-08 / 2.1e-09
#   gate (3,40,72) K=11     4.5e-07 / 7.1e-07  1.6e-08 / 1.4e-08  3.3e-08 / 2.7e-08  1.9e-08 / 1.0e-08
#   gate (1,33,65) K=5      5.0e-07 / 6.2e-07  1.2e-08 / 1.2e-08  2.1e-08 / 2.1e-08  1.9e-08 / 1.9e-08
#   gate (2,31,34) K=9      2.7e-07 / 4.8e-07  7.8e-09 / 7.8e-09  3.3e-08 / 2.6e-08  1.2e-08 / 1.2e-08
#   gate (3,40,72) K=3      2.9e-06 / 6.5e-06  9.2e-10 / 9.2e-10  2.0e-08 / 4.0e-08  3.2e-09 / 3.2e-09
#   gate (3,40,72) K=7      4.2e-07 / 7.0e-07  2.7e-09 / 2.7e-09  2.1e-08 / 3.9e-08  2.0e-09 / 2.8e-08
#   six planes K=11         5.9e-07 / 5.4e-07  3.5e-09 / 3.5e-09  6.1e-09 / 9.9e-09  2.1e-09 / 2.1e-09
#
# Closest to the bound: D-SSIM of (1,3,70) K=11, 0.87 of it (1.7e-8 against a
# lucky 2.1e-9 of the fp32 statement).  While the forward summed SSIM and
# formed 1 - mean at the end, that figure was 2.5e-8 and over the bound: the
# sum's rounding went whole into a D-SSIM of 0.023.  It now sums 1 - SSIM.
# --------------------------------------------------------------------------
def window64(K, dev):
    """The window in double, rounded to fp32 as the library's window_of does."""
    x = torch.arange(K, dtype=torch.float64) - (K - 1) / 2
    g = torch.exp(-x ** 2 / (2 * (K / 6.0) ** 2))
    return (g / g.sum()).float().double().to(dev)


def _blur64(img, w):
    """Separable zero-padded window sums of [C,H,W], tap by tap."""
    K, (H, W) = len(w), img.shape[-2:]
    a = F.pad(img, (K // 2, K // 2, 0, 0))
    a = sum(w[k] * a[..., :, k:k + W] for k in range(K))
    a = F.pad(a, (0, 0, K // 2, K // 2))
    return sum(w[k] * a[..., k:k + H, :] for k in range(K))


def torch_loss64(pred, target, lam=0.2, K=11, gate=True):
    """torch_loss in fp64; also returns the SSIM map.  gate=False leaves the
    clamp out (what a gate stuck open would differentiate)."""
    x, y = pred.double(), target.double()
    w = window64(K, pred.device)
    mu_x, mu_y = _blur64(x, w), _blur64(y, w)
    sigma_x = _blur64(x * x, w) - mu_x ** 2
    sigma_y = _blur64(y * y, w) - mu_y ** 2
    sigma_xy = _blur64(x * y, w) - mu_x * mu_y
    ssim = ((2 * mu_x * mu_y + 0.01 ** 2) * (2 * sigma_xy + 0.03 ** 2)) / (
        (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sigma_x + sigma_y + 0.03 ** 2))
    dssim = 1 - (ssim.clamp(0, 1) if gate else ssim).mean()
    l1 = (x - y).abs().mean()
    return (1 - lam) * l1 + lam * dssim, l1, dssim, ssim.detach()


def _three_ways(pkg, p, t, lam, K):
    """(values, gradient) of the kernel, the fp32 statement and the fp64 one."""
    res = []
    for fn in (lambda q: pkg.loss.photometric_loss(q, t, lam, K), lambda q: torch_loss(q, t, lam, K),
               lambda q: torch_loss64(q, t, lam, K)):
        q = (p.double() if len(res) == 2 else p.clone()).requires_grad_()  # (an fp64 leaf: its gradient stays fp64)
        out = fn(q)
        out[0].backward()
        res.append(([float(v.item()) for v in out[:3]], q.grad.double(), out[3] if len(out) > 3 else None))
    return res


def _near_unsafe(ssim, K):
    """Pixels within the window radius of one whose |SSIM| < 1e-4 (fp64): its
    gate may fall the other way in fp32, and it feeds these gradients."""
    unsafe = (ssim.abs() < 1e-4).double()
    return F.max_pool2d(unsafe[None], K, stride=1, padding=K // 2)[0] > 0


def _check_against_fp64(pkg, label, p, t, lam, K):
    """Print every figure, then hold the kernel to 8 err32 + 1e-7 max|ref|."""
    (kv, kg, _), (fv, fg, _), (rv, rg, ssim) = _three_ways(pkg, p, t, lam, K)
    keep = ~_near_unsafe(ssim, K)
    assert (~keep).double().mean().item() <= 0.02
    gmax = rg.abs().max().item()
    figs = [("grad", ((kg - rg).abs() * keep).max().item(), ((fg - rg).abs() * keep).max().item(), gmax)]
    figs += [(n, abs(kv[i] - rv[i]), abs(fv[i] - rv[i]), abs(rv[i])) for i, n in enumerate(("total", "l1", "dssim"))]
    bad = []
    for name, ek, e32, mag in figs:
        bound = 8 * e32 + 1e-7 * mag
        print(f"loss {label} K={K} lam={lam} {name}: kernel {ek:.3e} fp32 {e32:.3e} bound {bound:.3e} max {mag:.3e}")
        if not ek <= bound:
            bad.append((name, ek, e32, bound))
        if name == "grad" and K == 11 and not bound < 2e-5 * gmax:
            bad.append(("K = 11 gradient bound above the corner tap", bound, 2e-5 * gmax))
    assert not bad, bad
    return kg, rg, ssim, 8 * figs[0][2] + 1e-7 * gmax


# the image edge on, one inside and one past a 32-pixel tile edge; 1, 2, 3, 6, 9
# and 12 tiles (below 8, not divisible by 8); a height below the radius
SHAPES64 = [(1, 1, 1), (1, 32, 32), (1, 33, 31), (3, 31, 65), (2, 64, 96), (1, 3, 70)]


@pytest.mark.parametrize("lam", [0.2, 1.0])
@pytest.mark.parametrize("shape", SHAPES64)
@pytest.mark.parametrize("K", [1, 3, 5, 7, 9, 11])
def test_every_window_against_fp64(pkg, cuda, K, shape, lam):
    p, t = _pair(shape, sum(shape) + K, cuda, blur_target=True)
    _check_against_fp64(pkg, str(shape), p, t, lam, K)


def _half_anticorrelated(shape, seed, dev):
    """Right half of the width: target = pred + noise (SSIM in (0, 1)); left
    half: target = 1 - pred + noise (SSIM < 0, the clamp gate closed)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g)
    noise = 0.1 * torch.randn(shape, generator=g)
    left = torch.arange(shape[-1]) < shape[-1] // 2
    t = torch.where(left, 1 - p + noise, p + noise).clamp(0, 1)
    return p.to(dev), t.to(dev)


@pytest.mark.parametrize("shape,K", [((3, 40, 72), 11), ((1, 33, 65), 5), ((2, 31, 34), 9), ((3, 40, 72), 3),
                                     ((3, 40, 72), 7)])
def test_clamp_gate_closed(pkg, cuda, shape, K):
    lam = 0.2
    p, t = _half_anticorrelated(shape, 100 + K, cuda)
    kg, rg, ssim, bound = _check_against_fp64(pkg, "gate " + str(shape), p, t, lam, K)
    clamped = (ssim < 0) | (ssim > 1)
    assert clamped.double().mean().item() >= 0.25
    # where every pixel of the window is clamped the D-SSIM term has no gradient;
    # with the gate stuck open it would have the unclamped formula's
    q = p.double().requires_grad_()
    torch_loss64(q, t, lam, K, gate=False)[0].backward()
    inside = F.max_pool2d((~clamped).double()[None], K, stride=1, padding=K // 2)[0] == 0
    assert inside.sum().item() >= 20
    n = p.numel()
    assert torch.allclose(rg[inside], (1 - lam) / n * torch.sign(p.double() - t.double())[inside], rtol=1e-12, atol=0)
    assert ((q.grad - rg).abs() * inside).max().item() > 100 * bound
    assert ((kg - q.grad).abs() * inside).max().item() > 100 * bound


def test_host_side_paths(pkg, cuda):
    """Upstream gradient, forward without maps, non-contiguous pred, batch."""
    lam, K = 0.2, 11
    p, t = _pair((3, 37, 53), 21, cuda, blur_target=True)
    q1 = p.clone().requires_grad_()
    tot, l1, ds = pkg.loss.photometric_loss(q1, t, lam, K)
    tot.backward()
    # g_total: the kernel multiplies once, as 2.5 * grad does
    q2 = p.clone().requires_grad_()
    (2.5 * pkg.loss.photometric_loss(q2, t, lam, K)[0]).backward()
    assert torch.equal(q2.grad, 2.5 * q1.grad) and q1.grad.abs().max().item() > 0
    # maps == NULL
    with torch.no_grad():
        n_tot, n_l1, n_ds = pkg.loss.photometric_loss(p, t, lam, K)
    assert not n_tot.requires_grad
    assert torch.equal(torch.stack([n_tot, n_l1, n_ds]), torch.stack([tot.detach(), l1, ds]))
    f_tot, f_l1, f_ds = pkg.loss.photometric_loss(p, t, lam, K)  # (no requires_grad on pred either)
    assert torch.equal(torch.stack([f_tot, f_l1, f_ds]), torch.stack([tot.detach(), l1, ds]))
    # [H,W,C] storage seen as [C,H,W]
    hwc = p.permute(1, 2, 0).contiguous().requires_grad_()
    view = hwc.permute(2, 0, 1)
    assert not view.is_contiguous() and torch.equal(view.detach(), p)
    v_tot, v_l1, v_ds = pkg.loss.photometric_loss(view, t, lam, K)
    v_tot.backward()
    assert torch.equal(torch.stack([v_tot.detach(), v_l1, v_ds]), torch.stack([tot.detach(), l1, ds]))
    assert torch.equal(hwc.grad.permute(2, 0, 1), q1.grad)
    # [2,3,H,W]: the six planes averaged
    pb, tb = _pair((2, 3, 37, 53), 22, cuda, blur_target=True)
    qb = pb.clone().requires_grad_()
    outb = pkg.loss.photometric_loss(qb, tb, lam, K)
    outb[0].backward()
    q6 = pb.reshape(6, 37, 53).clone().requires_grad_()
    out6 = pkg.loss.photometric_loss(q6, tb.reshape(6, 37, 53), lam, K)
    out6[0].backward()
    assert torch.equal(torch.stack([o.detach() for o in outb]), torch.stack([o.detach() for o in out6]))
    assert qb.grad.shape == pb.shape and torch.equal(qb.grad.reshape(6, 37, 53), q6.grad)
    _check_against_fp64(pkg, "six planes", pb.reshape(6, 37, 53), tb.reshape(6, 37, 53), lam, K)
