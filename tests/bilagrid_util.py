"""The fp64 statements of the bilateral-grid kernels (include/gsplat_mi355x.h,
"Bilateral grid") -- the slice, its backward written out as the header states
it, the total variation -- the same slice through torch's grid_sample, and the
generators of the tests' cases.  numpy in, numpy out unless it says otherwise;
fp32 inputs are promoted, never rounded."""
import numpy as np
import torch

COEF = np.array([0.299, 0.587, 0.114])
SHAPES = [(2, 2, 2), (16, 16, 8), (5, 3, 16)]              # (Gw, Gh, L)
BIG_SHAPE = (33, 31, 9)  # 442 KB: more than the per-pixel kernels keep in LDS, so they read it from memory
IMAGES = [(1, 1), (3, 3), (17, 19), (33, 18), (64, 48), (257, 5)]  # (W, H)
KINK = 1e-4  # the generator keeps gray (L - 1) this far from an integer, and gray from 0 and 1

f64 = lambda a: np.asarray(a, np.float64)


def _axis(t, n):
    i0 = np.clip(np.floor(t), 0, n - 2).astype(np.int64)
    return i0, t - i0


def _cell(G, rgb):
    """What forward and backward share: per pixel the cell (iz, iy, ix), the
    fractions (fz, fy, fx) and the gray, each [H, W]."""
    _, L, Gh, Gw = G.shape
    _, H, W = rgb.shape
    ix, fx = _axis((np.arange(W) + 0.5) / W * (Gw - 1), Gw)
    iy, fy = _axis((np.arange(H) + 0.5) / H * (Gh - 1), Gh)
    gray = np.tensordot(COEF, rgb, 1)
    iz, fz = _axis(np.clip(gray, 0.0, 1.0) * (L - 1), L)
    bc = lambda a, axis: np.broadcast_to(a[None, :] if axis == 1 else a[:, None], (H, W))
    return (iz, bc(iy, 0), bc(ix, 1)), (fz, bc(fy, 0), bc(fx, 1)), gray


def _sliced(G, cell, frac):
    """A and dA / dz [12, H, W]: nested lerps, x, then y, then z."""
    (iz, iy, ix), (fz, fy, fx) = cell, frac
    c = lambda dz, dy, dx: G[:, iz + dz, iy + dy, ix + dx]
    lerp = lambda a, b, f: a + f * (b - a)
    a0 = lerp(lerp(c(0, 0, 0), c(0, 0, 1), fx), lerp(c(0, 1, 0), c(0, 1, 1), fx), fy)
    a1 = lerp(lerp(c(1, 0, 0), c(1, 0, 1), fx), lerp(c(1, 1, 0), c(1, 1, 1), fx), fy)
    return a0 + fz * (a1 - a0), a1 - a0


def slice64(G, rgb):
    """The corrected image [3, H, W]."""
    G, rgb = f64(G), f64(rgb)
    cell, frac, _ = _cell(G, rgb)
    A, _ = _sliced(G, cell, frac)
    return np.stack([A[4 * c] * rgb[0] + A[4 * c + 1] * rgb[1] + A[4 * c + 2] * rgb[2] + A[4 * c + 3] for c in range(3)])


def slice_backward64(G, rgb, g):
    """(d_rgb [3, H, W], d_grid [12, L, Gh, Gw]) as the header states them:
    d_grid a sum over the pixels of w_x w_y w_z g[c] (r, g, b, 1)[k] on the
    cell's eight nodes; d_rgb through the affine map and, where 0 < gray < 1,
    through z."""
    G, rgb, g = f64(G), f64(rgb), f64(g)
    L = G.shape[1]
    cell, frac, gray = _cell(G, rgb)
    (iz, iy, ix), (fz, fy, fx) = cell, frac
    A, dA = _sliced(G, cell, frac)
    rgb1 = np.concatenate([rgb, np.ones_like(rgb[:1])])
    d_grid = np.zeros_like(G)
    for dz, wz in ((0, 1 - fz), (1, fz)):
        for dy, wy in ((0, 1 - fy), (1, fy)):
            for dx, wx in ((0, 1 - fx), (1, fx)):
                w = wx * wy * wz
                for c in range(3):
                    for k in range(4):
                        np.add.at(d_grid[4 * c + k], (iz + dz, iy + dy, ix + dx), w * g[c] * rgb1[k])
    dz = sum(g[c] * (dA[4 * c:4 * c + 4] * rgb1).sum(0) for c in range(3))
    dgray = np.where((gray > 0) & (gray < 1), dz * (L - 1), 0.0)
    d_rgb = np.stack([sum(g[c] * A[4 * c + k] for c in range(3)) + COEF[k] * dgray for k in range(3)])
    return d_rgb, d_grid


def slice_grid_sample(G, rgb):
    """torch fp64 in (both may require grad), torch fp64 out: the same slice
    through torch.nn.functional.grid_sample -- 5-D input, bilinear, border
    padding, align_corners -- which clamps the guidance itself."""
    _, L, Gh, Gw = G.shape
    _, H, W = rgb.shape
    u = ((torch.arange(W, dtype=torch.float64) + 0.5) / W * 2 - 1).expand(H, W)
    v = ((torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1)[:, None].expand(H, W)
    gray = (torch.as_tensor(COEF)[:, None, None] * rgb).sum(0)
    coords = torch.stack([u, v, gray * 2 - 1], -1)[None, None]  # [1, 1, H, W, (x, y, z)]
    A = torch.nn.functional.grid_sample(G[None], coords, mode="bilinear", padding_mode="border",
                                        align_corners=True)[0, :, 0]  # [12, H, W]
    rgb1 = torch.cat([rgb, torch.ones_like(rgb[:1])])
    return (A.reshape(3, 4, H, W) * rgb1[None]).sum(1)


def tv_torch(G):
    """torch in, torch out."""
    return ((G[..., 1:] - G[..., :-1]) ** 2).mean() + ((G[..., 1:, :] - G[..., :-1, :]) ** 2).mean() + \
        ((G[:, 1:] - G[:, :-1]) ** 2).mean()


def tv64(G):
    """(tv, d tv / d G) written out: the header's closed form."""
    G = f64(G)
    tv, d = 0.0, np.zeros_like(G)
    for axis in (3, 2, 1):
        diff = np.diff(G, axis=axis)
        tv += (diff ** 2).mean()
        pad = [(0, 0)] * 4
        pad[axis] = (1, 1)
        p = np.pad(diff, pad)  # p[n] = G[n] - G[n - 1], 0 where there is no neighbour
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        d += (2.0 / diff.size) * (p[tuple(lo)] - p[tuple(hi)])
    return tv, d


# ------------------------------------------------------------------ cases ----
def identity(shape):
    gw, gh, gl = shape
    G = np.zeros((12, gl, gh, gw), np.float32)
    G[0] = G[5] = G[10] = 1
    return G


def random_grid(shape, seed):
    """The identity plus noise of 0.3: affine maps of an ordinary size whose
    nodes all differ."""
    rng = np.random.default_rng(seed)
    return (identity(shape) + rng.uniform(-0.3, 0.3, identity(shape).shape)).astype(np.float32)


def near_kink(rgb, L):
    gray = np.tensordot(COEF, f64(rgb), 1)
    z = gray * (L - 1)
    return (np.abs(z - np.round(z)) <= KINK) | (np.abs(gray) <= KINK) | (np.abs(gray - 1) <= KINK)


def image_case(W, H, L, seed, edges=False):
    """(rgb, g) fp32 [3, H, W]: colours in [-0.3, 1.3], so that some pixels have
    gray < 0 and some gray > 1 wherever the image has room for them, and no
    pixel within KINK of a kink of the z interpolation (the z derivative jumps
    there, and fp32 and fp64 may land on different sides): such pixels are
    nudged until none remain.  edges=True (forward-only checks) then puts
    pixels onto the clamp's two edges: rgb = 0, gray exactly 0, and rgb = 1,
    gray 1 to rounding."""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(-0.3, 1.3, (3, H, W)).astype(np.float32)
    if H * W >= 4:  # both clamped sides, by construction
        flat = rgb.reshape(3, -1)
        flat[:, 0], flat[:, 1] = -0.2, 1.2
    for _ in range(100):
        bad = near_kink(rgb, L)
        if not bad.any():
            break
        rgb[:, bad] += np.float32(3.3 * KINK)
    assert not near_kink(rgb, L).any()
    if edges:
        flat = rgb.reshape(3, -1)
        flat[:, -1] = 0.0
        if H * W >= 2:
            flat[:, -2] = 1.0
    g = rng.uniform(-1, 1, (3, H, W)).astype(np.float32)
    return rgb, g
