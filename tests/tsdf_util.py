"""fp64 numpy statements of the TSDF fusion and of the surface-nets extraction
(include/gsplat_mi355x.h, "TSDF fusion and mesh extraction"), the cases the
tests fuse, and the mesh checks (manifold, Euler, orientation).  The
statements read the kernels' own fp32 inputs: every scalar is rounded to fp32
first and every side / validity test reads stored fp32 values, so only the
arithmetic differs."""
import math

import numpy as np

from stubs import Cam

f32 = lambda v: np.float32(v).astype(np.float64)


# ----------------------------------------------------------------- cameras ----
def look_at_view(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """A 4x4 world-to-camera matrix in the projection's convention (x right, y
    up, looking along +z: py = -fy Y / Z + cy) for a camera at `eye`."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    if abs(np.dot(fwd, up)) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    R = np.stack([right, upv, fwd])
    wv = np.eye(4)
    wv[:3, :3], wv[:3, 3] = R, -R @ eye
    return wv.astype(np.float32)


def camera_row64(cam):
    """{view[12], fx, fy, cx, cy} as the package forms them (fp32 values, in fp64)."""
    W, H = cam._width, cam._height
    fx = 0.5 * W / math.tan(cam._FoVx * 0.5)
    fy = 0.5 * H / math.tan(cam._FoVy * 0.5)
    wv = np.asarray(cam.world_view_transform(), np.float32).reshape(16)[:12]
    return np.concatenate([wv.astype(np.float64), f32([fx, fy, W * 0.5, H * 0.5])])


def nodes64(origin, h, dims):
    """Node positions [Nz, Ny, Nx, 3] in fp64 from the fp32 origin and voxel size."""
    nx, ny, nz = dims
    o, h = f32(origin), float(f32(h))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[0] + h * i, o[1] + h * j, o[2] + h * k], -1)


# ------------------------------------------------------------------ fusion ----
BRANCHES = ("behind_near", "outside_image", "no_depth", "beyond_depth_max", "low_alpha", "behind_surface", "clamped",
            "updated")


def integrate64(tsdf, weight, color, origin, h, cams, depth, alpha, image, near, trunc, alpha_min, depth_max):
    """The fusion rule in fp64 on fp32 inputs.  tsdf, weight [Nz, Ny, Nx],
    color [3, Nz, Ny, Nx] or None; depth [V, H, W], alpha the same or None,
    image [V, 3, H, W] or None.  Returns (tsdf, weight, color, flagged,
    counts): flagged marks the nodes one of whose decisions is within
    rounding -- px + 0.5 or py + 0.5 within 1e-3 of an integer, |s + trunc| <
    1e-4, |Z - near| < 1e-4, d within 1e-6 of depth_max -- and counts says how
    many (node, view) pairs took each branch."""
    nz, ny, nx = tsdf.shape
    P = nodes64(origin, h, (nx, ny, nz))
    t, w = tsdf.astype(np.float64).copy(), weight.astype(np.float64).copy()
    c = None if color is None else color.astype(np.float64).copy()
    near, trunc, alpha_min = float(f32(near)), float(f32(trunc)), float(f32(alpha_min))
    depth_max = float(np.float32(depth_max))
    V, H, W = depth.shape
    flagged = np.zeros(t.shape, bool)
    counts = dict.fromkeys(BRANCHES, 0)
    near_int = lambda a: np.abs(a - np.rint(a)) < 1e-3
    for v in range(V):
        row = camera_row64(cams[v])
        X = P @ row[0:3] + row[3]
        Y = P @ row[4:7] + row[7]
        Z = P @ row[8:11] + row[11]
        flagged |= np.abs(Z - near) < 1e-4
        live = Z > near
        counts["behind_near"] += int((~live).sum())
        Zs = np.where(live, Z, 1.0)
        px, py = row[12] * X / Zs + row[14], -row[13] * Y / Zs + row[15]
        u, vv = np.floor(px + 0.5), np.floor(py + 0.5)
        # (a pixel more than one outside the image stays outside under any rounding)
        flagged |= live & (near_int(px + 0.5) | near_int(py + 0.5)) & (u >= -1) & (u <= W) & (vv >= -1) & (vv <= H)
        inside = live & (u >= 0) & (u < W) & (vv >= 0) & (vv < H)
        counts["outside_image"] += int((live & ~inside).sum())
        ui, vi = np.where(inside, u, 0).astype(np.int64), np.where(inside, vv, 0).astype(np.int64)
        d = depth[v][vi, ui].astype(np.float64)
        with np.errstate(invalid="ignore"):
            has = inside & (d > 0)
            counts["no_depth"] += int((inside & ~has).sum())
            flagged |= has & (np.abs(d - depth_max) < 1e-6)
            cut = has & (d > depth_max)
            counts["beyond_depth_max"] += int(cut.sum())
            has &= ~cut
            if alpha is not None:
                low = has & (alpha[v][vi, ui] < np.float32(alpha_min))
                counts["low_alpha"] += int(low.sum())
                has &= ~low
            s = d - Z
            flagged |= has & (np.abs(s + trunc) < 1e-4)
            behind = has & (s < -trunc)
            counts["behind_surface"] += int(behind.sum())
            upd = has & ~behind
            tau = np.minimum(1.0, s / trunc)
            counts["clamped"] += int((upd & (s / trunc > 1.0)).sum())
        counts["updated"] += int(upd.sum())
        w1 = w + 1.0
        t = np.where(upd, (t * w + np.where(upd, tau, 0.0)) / w1, t)
        if c is not None and image is not None:
            for ch in range(3):
                c[ch] = np.where(upd, (c[ch] * w + image[v, ch][vi, ui].astype(np.float64)) / w1, c[ch])
        w = np.where(upd, w1, w)
    return t, w, c, flagged, counts


def fusion_case(dims, seed, h=0.11, origin=(-2.0, -1.2, -0.5), W=45, H=31, views=2):
    """Cameras about 4 units from the volume's centre plus one inside it, a
    smooth depth field around 4 with 5 % of its pixels zeroed, alpha on both
    sides of 0.5, an image, and a depth_max that cuts some pixels."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    centre = np.asarray(origin) + 0.5 * h * (np.array([nx, ny, nz]) - 1)
    cams = []
    for i in range(views):
        th, ph = 2 * math.pi * (i + 0.3 * rng.random()) / views, 0.2 + 0.5 * rng.random()
        eye = centre + 4.0 * np.array([math.cos(th) * math.cos(ph), math.sin(th) * math.cos(ph), math.sin(ph)])
        cams.append(Cam(W, H, 0.9, 0.65, look_at_view(eye, centre + 0.2 * rng.standard_normal(3))))
    cams.append(Cam(W, H, 0.9, 0.65, look_at_view(centre + np.array([0.05, 0.03, 0.02]), centre + np.array([1.0, 0.4, 0.1]))))
    V = len(cams)
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    depth = np.stack([4.0 + 0.9 * np.sin(2.1 * x + v) * np.cos(1.7 * y - 0.5 * v) + 0.05 * rng.standard_normal((H, W))
                      for v in range(V)])
    depth[-1] = 0.9 + 0.5 * x * y  # the camera inside the volume looks at something near
    depth[rng.random(depth.shape) < 0.05] = 0.0
    alpha = rng.random(depth.shape)
    alpha[rng.random(depth.shape) < 0.7] = 1.0
    # Eight more views with constant maps, so that a volume of a single node also
    # takes every branch: from 4 units away the centre has Z = 4, and a depth of
    # 0 / 5 / 2 / 4.55 / 4.1 skips for no depth, cuts at depth_max, lies behind the
    # surface, clamps tau, updates; one view has alpha 0.1; one camera looks 45
    # degrees past the volume and one away from it.
    eye = centre + 4.0 * np.array([0.6, -0.64, 0.48])
    at = centre + np.array([0.031, 0.017, -0.023])
    side = np.cross(at - eye, [0.0, 0.0, 1.0])
    side *= 4.0 / np.linalg.norm(side)
    for d_const, a_const, target in ((0.0, 1.0, at), (5.0, 1.0, at), (4.1, 0.1, at), (2.0, 1.0, at), (4.55, 1.0, at),
                                     (4.1, 1.0, at), (4.1, 1.0, at + side), (4.1, 1.0, 2 * eye - at)):
        cams.append(Cam(W, H, 0.9, 0.65, look_at_view(eye, target)))
        depth = np.concatenate([depth, np.full((1, H, W), d_const)])
        alpha = np.concatenate([alpha, np.full((1, H, W), a_const)])
    image = rng.random((len(cams), 3, H, W))
    return cams, depth.astype(np.float32), alpha.astype(np.float32), image.astype(np.float32), 4.6


# -------------------------------------------------------------- extraction ----
_AXES = ((0, 1, 2), (1, 2, 0), (2, 0, 1))  # (a, b, c): x -> (y, z), y -> (z, x), z -> (x, y)


def extract64(tsdf, weight, color, origin, h, min_weight=1.0):
    """Surface nets in fp64 on the stored fp32 volume.  Returns (vertices
    [Vn, 3] fp64, faces [Fn, 3] int64, colors [Vn, 3] fp64 or None)."""
    nz, ny, nx = tsdf.shape
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64), None if color is None else np.zeros((0, 3))
    f = tsdf.astype(np.float32)
    inside = f < 0
    ok = weight.astype(np.float32) >= np.float32(min_weight)
    corner = lambda a, dx, dy, dz: a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    offs = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    valid = np.all([corner(ok, *o) for o in offs], axis=0)
    n_in = np.sum([corner(inside, *o) for o in offs], axis=0)
    active = valid & (n_in > 0) & (n_in < 8)
    rank = np.cumsum(active.reshape(-1)).reshape(active.shape) - 1  # [k, j, i], i fastest
    o, h = f32(origin), float(f32(h))
    F = f.astype(np.float64)
    verts, cols = [], []
    # the 12 edges: x edges by (dy, dz), y edges by (dx, dz), z edges by (dx, dy), lexicographic
    edges = []
    for axis in range(3):
        for o0 in (0, 1):
            for o1 in (0, 1):
                a = [0, 0, 0]
                others = [d for d in range(3) if d != axis]
                a[others[0]], a[others[1]] = o0, o1
                b = list(a)
                b[axis] = 1
                edges.append((tuple(a), tuple(b)))
    for k, j, i in zip(*np.nonzero(active)):
        qs, cs = [], []
        for a, b in edges:
            fa, fb = F[k + a[2], j + a[1], i + a[0]], F[k + b[2], j + b[1], i + b[0]]
            if (fa < 0) == (fb < 0):
                continue
            r = fa / (fa - fb)
            qs.append(np.asarray(a, np.float64) + r * (np.asarray(b, np.float64) - np.asarray(a, np.float64)))
            if color is not None:
                ca = color[:, k + a[2], j + a[1], i + a[0]].astype(np.float64)
                cb = color[:, k + b[2], j + b[1], i + b[0]].astype(np.float64)
                cs.append(ca + r * (cb - ca))
        verts.append(o + h * (np.array([i, j, k], np.float64) + np.mean(qs, axis=0)))
        if color is not None:
            cols.append(np.mean(cs, axis=0))
    faces = []
    cell_ok = lambda c: all(0 <= c[d] < (nx - 1, ny - 1, nz - 1)[d] for d in range(3)) and valid[c[2], c[1], c[0]]
    # only nodes next to a sign change can emit: walk those, in linear node order
    cand = np.zeros(inside.shape, bool)
    cand[:, :, :-1] |= inside[:, :, :-1] != inside[:, :, 1:]
    cand[:, :-1, :] |= inside[:, :-1, :] != inside[:, 1:, :]
    cand[:-1, :, :] |= inside[:-1, :, :] != inside[1:, :, :]
    dims = (nx, ny, nz)
    for k, j, i in zip(*np.nonzero(cand)):
        n = np.array([i, j, k])
        for a, b, c in _AXES:
            if n[a] + 1 >= dims[a]:
                continue
            m = n.copy()
            m[a] += 1
            if inside[k, j, i] == inside[m[2], m[1], m[0]]:
                continue
            eb, ec = np.eye(3, dtype=np.int64)[b], np.eye(3, dtype=np.int64)[c]
            quad = [n - eb - ec, n - ec, n, n - eb]
            if not all(cell_ok(q) for q in quad):
                continue
            c00, c10, c11, c01 = (int(rank[q[2], q[1], q[0]]) for q in quad)
            if inside[k, j, i]:
                faces += [(c00, c10, c11), (c00, c11, c01)]
            else:
                faces += [(c00, c11, c10), (c00, c01, c11)]
    V = np.asarray(verts, np.float64).reshape(-1, 3)
    return V, np.asarray(faces, np.int64).reshape(-1, 3), None if color is None else np.asarray(cols).reshape(-1, 3)


def sphere_volume(dims, R=0.8, h=None, trunc=None, centre_offset=(0.013, -0.021, 0.017)):
    """The exact signed distance of a sphere, clip((|p - c| - R) / trunc, -1, 1),
    on a volume centred (nearly) at the origin: (tsdf fp32, weight, color, origin, h)."""
    nx, ny, nz = dims
    h = 2.4 * R / (min(dims) - 1) if h is None else h
    trunc = 4 * h if trunc is None else trunc
    origin = tuple(-0.5 * h * (n - 1) + off for n, off in zip(dims, centre_offset))
    P = nodes64(origin, h, dims)
    tsdf = np.clip((np.linalg.norm(P, axis=-1) - R) / trunc, -1, 1).astype(np.float32)
    color = np.moveaxis(0.5 + 0.4 * np.sin(3.0 * P), -1, 0).astype(np.float32)
    return tsdf, np.ones_like(tsdf), color, origin, h


# ------------------------------------------------------------- mesh checks ----
def edge_uses(faces):
    """{(a, b): count} over the faces' directed edges."""
    uses = {}
    for t in np.asarray(faces).tolist():
        for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            uses[e] = uses.get(e, 0) + 1
    return uses


def check_closed_manifold(vertices, faces):
    """Every edge is used by exactly two faces, in opposite directions, and V - E + F = 2."""
    uses = edge_uses(faces)
    assert all(n == 1 for n in uses.values()), "an edge is used twice in one direction"
    assert all((b, a) in uses for a, b in uses), "an edge without its opposite"
    E = len(uses) // 2
    assert len(vertices) - E + len(faces) == 2, (len(vertices), E, len(faces))
    assert len(np.unique(np.asarray(faces))) == len(vertices), "a vertex no face uses"


def check_outward(vertices, faces, centre=(0.0, 0.0, 0.0)):
    """Every face normal has a positive dot product with its centroid (relative to `centre`)."""
    v = np.asarray(vertices, np.float64) - np.asarray(centre, np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3) > 0).all()


# --------------------------------------------------------------------- PLY ----
def read_ply(path):
    """(vertices [Vn, 3] f4, faces [Fn, 3] i4, colors [Vn, 3] u1 or None) of a
    binary little-endian PLY as save_mesh_ply writes it."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    vn = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    fn = int([l for l in lines if l.startswith("element face")][0].split()[2])
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    assert props[-1] == ["list", "uchar", "int", "vertex_indices"]
    kinds = {"float": "<f4", "uchar": "u1"}
    vt = np.dtype([(name, kinds[kind]) for kind, name in props[:-1]])
    ft = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(raw) == end + vn * vt.itemsize + fn * ft.itemsize
    vert = np.frombuffer(raw, vt, vn, end)
    face = np.frombuffer(raw, ft, fn, end + vn * vt.itemsize)
    assert (face["n"] == 3).all()
    colors = np.stack([vert["red"], vert["green"], vert["blue"]], 1) if "red" in vt.names else None
    return np.stack([vert["x"], vert["y"], vert["z"]], 1), face["i"].copy(), colors
