"""The fp64 statements of the four normal-consistency kernels
(include/gsplat_mi355x.h, "Normal consistency"), in torch so that autograd can
check the hand-written backward statements, and the generators of the GPU
tests' cases.  Everything takes and returns numpy arrays unless it says
otherwise; fp32 inputs are promoted, never rounded."""
import math

import numpy as np
import torch

T = lambda a: torch.as_tensor(np.asarray(a, np.float64))


# ------------------------------------------------------------ per Gaussian ----
def rotation_columns(q):
    """[n, 3, 3] torch fp64 R(q) of (w, x, y, z) rows, R[:, :, k] its column k."""
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def gaussian_normals_torch(q, scaling, xyz, view):
    """torch fp64 in, torch fp64 out: (normals [n, 3], axis [n], n_c . p_c [n]
    before the flip, p_c [n, 3])."""
    s0, s1, s2 = scaling.unbind(-1)
    k = torch.where(s1 < s0, torch.where(s2 < s1, 2, 1), torch.where(s2 < s0, 2, 0))  # the first among equals
    qh = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    R = rotation_columns(qh)
    nw = R[torch.arange(q.shape[0]), :, k]
    Rv, t = view[:3, :3], view[:3, 3]
    nc = nw @ Rv.T
    pc = xyz @ Rv.T + t
    d = (nc * pc).sum(-1)
    sign = torch.where(d > 0, -1.0, 1.0).to(torch.float64)
    return nc * sign[:, None], k, d, pc


def gaussian_normals64(q, scaling, xyz, view):
    with torch.no_grad():
        n, k, d, pc = gaussian_normals_torch(T(q), T(scaling), T(xyz), T(view))
    return n.numpy(), k.numpy(), d.numpy(), pc.numpy()


def gaussian_normals_backward64(q, scaling, xyz, view, g):
    """The header's backward: through the flip sign, Rv, column k of R and the
    normalisation, written out by hand (numpy fp64)."""
    q, g, view = (np.asarray(a, np.float64) for a in (q, g, view))
    _, k, d, _ = gaussian_normals64(q, scaling, xyz, view)
    sign = np.where(d > 0, -1.0, 1.0)
    ln = np.sqrt((q * q).sum(1))
    unit = ln >= 1e-12
    inv = 1.0 / np.maximum(ln, 1e-12)
    w, x, y, z = (q * inv[:, None]).T
    a0, a1, a2 = ((g * sign[:, None]) @ view[:3, :3]).T  # Rv^T g
    o = np.zeros_like(w)
    J = {  # d(column k) / d(w, x, y, z): rows of three
        0: [(o, 2 * z, -2 * y), (o, 2 * y, 2 * z), (-4 * y, 2 * x, -2 * w), (-4 * z, 2 * w, 2 * x)],
        1: [(-2 * z, o, 2 * x), (2 * y, -4 * x, 2 * w), (2 * x, o, 2 * z), (-2 * w, -4 * z, 2 * y)],
        2: [(2 * y, -2 * x, o), (2 * z, -2 * w, -4 * x), (2 * w, 2 * z, -4 * y), (2 * x, 2 * y, o)],
    }
    dq = np.zeros_like(q)
    for kk, rows in J.items():
        sel = k == kk
        for c, (j0, j1, j2) in enumerate(rows):
            dq[sel, c] = (j0 * a0 + j1 * a1 + j2 * a2)[sel]
    qh = np.stack([w, x, y, z], 1)
    along = np.where(unit, (qh * dq).sum(1), 0.0)
    return (dq - qh * along[:, None]) * inv[:, None]


def gaussian_case(n, seed, view=None):
    """fp32 (rotation, scaling, xyz, view [4,4], g) whose every decision is
    safe by construction: log-scales a random permutation of log(1, 1.6, 2.5)
    plus a per-row offset plus jitter in +-0.05 (smallest gap >= 0.37),
    positions resampled in fp64 until |n_c . p_c| >= 0.05 |p_c|, quaternion
    norms spread over e^(+-1)."""
    rng = np.random.default_rng(seed)
    if view is None:
        view = random_view(rng)
    q = rng.normal(size=(n, 4))
    q *= (np.exp(rng.uniform(-1, 1, n)) / np.linalg.norm(q, axis=1))[:, None]
    base = np.log([1.0, 1.6, 2.5])
    s = np.stack([rng.permutation(base) for _ in range(n)]) + rng.normal(size=(n, 1)) + rng.uniform(-0.05, 0.05, (n, 3))
    q, s = q.astype(np.float32), s.astype(np.float32)
    srt = np.sort(s.astype(np.float64), 1)
    assert (srt[:, 1] - srt[:, 0]).min() >= 0.37
    xyz = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    for _ in range(200):
        _, _, d, pc = gaussian_normals64(q, s, xyz, view)
        bad = np.abs(d) < 0.05 * np.linalg.norm(pc, axis=1)
        if not bad.any():
            break
        xyz[bad] = rng.uniform(-3, 3, (int(bad.sum()), 3)).astype(np.float32)
    else:
        raise AssertionError("no safe positions")
    g = rng.normal(size=(n, 3)).astype(np.float32)
    return q, s, xyz, view, g


def random_view(rng):
    """A random rigid world -> camera matrix [4, 4], fp32."""
    a = rng.normal(size=4)
    R = rotation_columns(T(a / np.linalg.norm(a))[None])[0].numpy()
    view = np.eye(4)
    view[:3, :3], view[:3, 3] = R, rng.uniform(-1, 1, 3) + [0, 0, 4]
    return view.astype(np.float32)


# --------------------------------------------------------------- per pixel ----
def rays(H, W, fx, fy, cx, cy):
    """torch fp64 [3, H, W]: ((x - cx) / fx, -(y - cy) / fy, 1)."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return torch.stack([(x - cx) / fx, -(y - cy) / fy, torch.ones_like(x)])


def surface_torch(depth, intr):
    """torch fp64 depth [H, W] -> (n_d [3, H, W], m [3, H, W], dx, dy, |m| with
    0 where n_d is 0, r): the definition, differences of P = D r as they stand."""
    H, W = depth.shape
    r = rays(H, W, *intr)
    P = depth[None] * r
    dx, dy = torch.zeros_like(P), torch.zeros_like(P)
    ok = torch.zeros(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        dx[:, 1:-1, 1:-1] = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
        dy[:, 1:-1, 1:-1] = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
        ok[1:-1, 1:-1] = True
    m = torch.cross(dx, dy, dim=0)
    ln = m.norm(dim=0)
    ok = ok & torch.isfinite(ln) & (ln > 1e-20)
    safe = torch.where(ok, ln, torch.ones_like(ln))
    nd = torch.where(ok[None], m / safe[None], torch.zeros_like(m))
    return nd, m, dx, dy, torch.where(ok, ln, torch.zeros_like(ln)), r


def consistency_torch(normals, depth, alpha, intr):
    """torch fp64: (error [H, W], n_d [3, H, W]); alpha is a weight (detached)."""
    nd = surface_torch(depth, intr)[0]
    return 1 - alpha.detach() * (normals * nd).sum(0), nd


def consistency64(normals, depth, alpha, intr):
    with torch.no_grad():
        e, nd = consistency_torch(T(normals), T(depth), T(alpha), intr)
    return e.numpy(), nd.numpy()


def consistency_backward64(normals, depth, alpha, intr, g_error):
    """The header's backward as a gather, by hand (torch fp64 inside): (d_normals, d_depth)."""
    Nr, D, A, g = T(normals), T(depth), T(alpha), T(g_error)
    with torch.no_grad():
        nd, _, dx, dy, ln, r = surface_torch(D, intr)
        coef = -(A * g)
        d_normals = coef[None] * nd
        gn = coef[None] * Nr
        ok = ln > 0
        safe = torch.where(ok, ln, torch.ones_like(ln))
        gm = torch.where(ok[None], (gn - nd * (nd * gn).sum(0, keepdim=True)) / safe[None], torch.zeros_like(gn))
        gdx, gdy = torch.cross(dy, gm, dim=0), torch.cross(gm, dx, dim=0)
        pad = lambda t: torch.nn.functional.pad(t, (1, 1, 1, 1))  # (a neighbour outside the image: 0)
        px, py = pad(gdx), pad(gdy)
        v = px[:, 1:-1, :-2] - px[:, 1:-1, 2:] + py[:, :-2, 1:-1] - py[:, 2:, 1:-1]
        d_depth = (r * v).sum(0)
    return d_normals.numpy(), d_depth.numpy()


def intrinsics(W, H, fovx=1.0, fovy=0.8):
    """(fx, fy, cx, cy) as camera_params forms them, rounded to fp32 as the ABI does."""
    v = (0.5 * W / math.tan(fovx * 0.5), 0.5 * H / math.tan(fovy * 0.5), W * 0.5, H * 0.5)
    return tuple(float(np.float32(x)) for x in v)


PLANE_N = np.array([0.3, -0.2, -0.93]) / np.linalg.norm([0.3, -0.2, -0.93])
PLANE_D = -3.0


def plane_depth(H, W, intr):
    """fp64 [H, W]: the depth D = d / (n . r) of the plane n . P = d along every pixel's ray."""
    r = rays(H, W, *intr).numpy()
    return PLANE_D / np.einsum("k,khw->hw", PLANE_N, r)


def pixel_case(H, W, seed):
    """fp32 (normals [3,H,W], depth 3 + 0.5 U(0,1), alpha in (0.2, 1), g_error)."""
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)
    return (f(rng.normal(size=(3, H, W))), f(3 + 0.5 * rng.uniform(size=(H, W))), f(rng.uniform(0.2, 1, (H, W))),
            f(rng.normal(size=(H, W))))
