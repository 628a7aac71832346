"""Device-resident frames (gs_render_fwd_args.device_counts = 1) driven
without a graph, and the numpy statements they are checked against.

device_frame() fills gs_render_forward's / gs_render_backward's arguments as
graph_step.GraphedStep._capture does and runs them on the current stream.
Every buffer a capacity sizes is allocated with a guard behind it and filled
with garbage first: tile keys past T are 0xABABABAB (larger than any tile
id), gradient partials that were not written this frame are NaN, and a write
past a buffer's end changes a guard byte.  The frame is read back through
gs_frame_offsets / gs_tile_offsets.

The statements: index_statement() -- the depth order, the rectangles and the
tile lists of a frame from its own projections (test_index_work_bit_exact's)
-- and frame_status() -- counters[4] and counters[5]."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from stubs import Cam

GUARD = 4096
FILL = 0xAB
FILL_WORD = 0xABABABAB
GRAD_NAMES = ("xyz", "scaling", "rotation", "color", "opacity")
_SINGLE_SIGMA_PX = (0.4, 1.5)  # radius = 3 sqrt(lambda_max) <= 3 * 1.5 * sqrt(1 + tan^2 + tan^2) < 5.6 px


# ------------------------------------------------------------------ scenes
def camera(pkg, W, H, bg=(0.1, 0.2, 0.3)):
    """The synthetic scenes' camera (identity view, FoVx 60 degrees) as CameraParams."""
    fovx, fovy = pkg.synthetic.fov_pair(W, H)
    st = pkg.RenderSettings(image_height=H, image_width=W, bg_color=torch.tensor(bg, dtype=torch.float32))
    return pkg.camera_params(Cam(W, H, fovx, fovy), st)


def single_tile_gaussians(pkg, W, H, z, gen, tile=16):
    """len(z) Gaussians that each touch exactly one tile under the identity
    camera: the centre on the middle of a (seeded) tile, an isotropic scale of
    0.4 .. 1.5 px, so that the truncated radius stays below 7 px."""
    assert W % tile == 0 and H % tile == 0, "tile centres are taken from whole tiles"
    k = int(z.shape[0])
    fovx, fovy = pkg.synthetic.fov_pair(W, H)
    fx, fy = 0.5 * W / math.tan(0.5 * fovx), 0.5 * H / math.tan(0.5 * fovy)
    tiles_x, tiles_y = W // tile, H // tile
    t = torch.randint(0, tiles_x * tiles_y, (k,), generator=gen)
    px = (t % tiles_x).double() * tile + 0.5 * tile + 0.5
    py = (t // tiles_x).double() * tile + 0.5 * tile + 0.5
    zd = z.double()
    x = (px - 0.5 * W) * zd / fx
    y = -(py - 0.5 * H) * zd / fy
    lo, hi = _SINGLE_SIGMA_PX
    sigma = (torch.rand(k, generator=gen).double() * (hi - lo) + lo) * zd / fx
    scaling = torch.log(sigma).float()[:, None].repeat(1, 3)
    rot = torch.randn(k, 4, generator=gen)
    rot = rot / rot.norm(dim=1, keepdim=True)
    opacity = torch.randn(k, 1, generator=gen)
    fdc = torch.rand(k, 1, 3, generator=gen)
    return pkg.synthetic.SyntheticScene(torch.stack([x.float(), y.float(), z.float()], 1), scaling, rot, fdc, opacity,
                                        W, H, fovx, fovy)


def concat_scenes(pkg, a, b):
    cat = lambda name: torch.cat([getattr(a, name), getattr(b, name)], 0)
    return pkg.synthetic.SyntheticScene(cat("xyz"), cat("scaling"), cat("rotation"), cat("features_dc"),
                                        cat("opacity"), a.width, a.height, a.fovx, a.fovy)


def scene_with_T(pkg, target, W, H, n_base, seed, cuda=None):
    """A seeded scene whose frame has exactly `target` tile touches: a
    synthetic.make_scene base of n_base Gaussians (rectangles of mixed sizes),
    rendered once on the host path for its T0, plus target - T0 single-tile
    Gaussians at depths drawn from the base's z range (they interleave in
    depth order).  n_base = 0: single-tile Gaussians only.  target None: the
    base alone.  The caller renders the scene on the host path and asserts
    its T (a missed target is a failure of the test)."""
    cuda = torch.device("cuda:0") if cuda is None else cuda
    gen = torch.Generator().manual_seed(1000 + seed)
    if n_base:
        base = pkg.synthetic.make_scene(n_base, W, H, seed=seed, sigma_range=(0.002, 0.02))
        if target is None:
            return base
        T0 = host_frame(pkg, model_of(pkg, base, cuda), camera(pkg, W, H)).T
        z_lo, z_hi = float(base.xyz[:, 2].min()), float(base.xyz[:, 2].max())
    else:
        base, T0, z_lo, z_hi = None, 0, 2.0, 6.0
    extra = target - T0
    assert extra >= 0, f"the base of {n_base} Gaussians already has T = {T0} > {target}"
    assert n_base + extra <= 20000, "scenes stay at n <= 20000"
    z = torch.rand(extra, generator=gen) * (z_hi - z_lo) + z_lo
    singles = single_tile_gaussians(pkg, W, H, z, gen)
    return singles if base is None else concat_scenes(pkg, base, singles)


def depth_ulp_scene(pkg, W, H, n, seed, z0=3.0, span=200):
    """n single-tile Gaussians whose depths are z0 + k ulp, k = i mod (span + 1):
    the visible depth bits span exactly `span`."""
    gen = torch.Generator().manual_seed(2000 + seed)
    assert n > span
    bits = np.float32(z0).view(np.uint32).astype(np.int64) + (np.arange(n) % (span + 1))
    bits = bits[torch.randperm(n, generator=gen).numpy()]
    z = torch.from_numpy(bits.astype(np.uint32).view(np.float32).copy())
    return single_tile_gaussians(pkg, W, H, z, gen)


def behind_camera_scene(pkg, n, W, H, seed):
    sc = pkg.synthetic.make_scene(n, W, H, seed=seed)
    sc.xyz[:, 2] *= -1.0
    return sc


def off_screen_scene(pkg, n, W, H, seed):
    """In front of the camera, every centre far to the right of the image
    (more than radius_max = 50 px past its edge)."""
    sc = pkg.synthetic.make_scene(n, W, H, seed=seed)
    sc.xyz[:, 0] = 10.0 * sc.xyz[:, 2]
    return sc


def model_of(pkg, scene, cuda):
    return pkg.synthetic.to_model(scene, pkg.GaussianModel, cuda)


def cotangents(H, W, cuda, seed=1):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.rand(s, generator=g) * 2 - 1).to(cuda) for s in ((3, H, W), (1, H, W), (1, H, W)))


# --------------------------------------------------------------- host path
def _raw(model):
    return tuple(None if t is None else t.detach() for t in
                 (model._xyz, None, model._scaling, model._rotation, model._features_dc[:, 0, :], model._opacity))


def host_frame(pkg, model, cam, cot=None):
    """The frame on the host path with 32-bit depth keys (RZ.forward_pipeline
    through the frame entry points, and backward_pipeline with the three pixel
    cotangents): outputs, the frame's index work, and the five gradients."""
    RZ = pkg.rasterizer
    raw = _raw(model)
    with torch.no_grad():
        img, al, dp, m2, cn, rd, vi, fr = RZ.forward_pipeline(cam, *raw, opacity_is_logit=True, depth_window_ok=False,
                                                              need_grad=cot is not None)
    assert fr.calls is True, "the host path of these tests is the frame entry points'"
    h = SimpleNamespace(image=img, alpha=al, depth=dp, means2d=m2, conics=cn, radii=rd, vis=vi, fr=fr, M=int(fr.M),
                        T=int(fr.T), zmin=int(fr.fa.depth_min_bits), zmax=int(fr.fa.depth_max_bits), grads=None)
    if h.M > 0:
        h.sorted_gauss = fr.sorted_gauss.clone()
        h.ranges, h.rects, h.pair_offset = fr.ranges.clone(), fr.rects.clone(), fr.pair_offset.clone()
    if cot is not None:
        d = RZ.backward_pipeline(cam, fr, *raw, m2, cn, cot[0], cot[1], cot[2], None, None, opacity_is_logit=True,
                                 outputs=(img, al, dp))
        h.grads = {"xyz": d[0], "scaling": d[2], "rotation": d[3], "color": d[4], "opacity": d[5]}
    torch.cuda.synchronize()
    return h


# ------------------------------------------------------------------ driver
class _Guarded:
    """`nbytes` bytes of device memory with a guard behind them, all filled with `fill`."""

    def __init__(self, nbytes, fill, cuda):
        self.nbytes, self.fill = int(nbytes), fill
        self.buf = torch.full((self.nbytes + GUARD,), fill, dtype=torch.uint8, device=cuda)
        self.view = self.buf[:self.nbytes]

    def refill(self):
        self.buf.fill_(self.fill)

    def guard_intact(self):
        return bool((self.buf[self.nbytes:] == self.fill).all())


def _bind(pkg, cuda, model, cam, capacity, window, msd, hc):
    """The buffers and gs_render_forward's arguments of one frame of `model`
    into a tile workspace of `capacity` entries (device_counts still 0)."""
    RZ, N = pkg.rasterizer, pkg._native
    lib = N.load()
    n, H, W = int(model._xyz.shape[0]), cam.image_height, cam.image_width
    tiles, cells, groups = cam.tiles_x * cam.tiles_y, cam.cells, cam.groups
    f = SimpleNamespace(n=n, H=H, W=W, tiles=tiles, cells=cells, groups=groups, capacity=int(capacity), lib=lib,
                        native=N, window=window, hc=hc, model=model, cam=cam)
    f.frame_ws = _Guarded(lib.gs_frame_workspace_bytes(n, W, H, cam.tile_size), FILL, cuda)
    f.tile_ws = _Guarded(lib.gs_tile_workspace_bytes(capacity, tiles, cells, groups), FILL, cuda)
    f.pair_grads = _Guarded(capacity * groups * N.GS_PARTIAL_STRIDE * 4, 0xFF, cuda)
    nan = float("nan")
    f.means2d, f.conics, f.radii = (torch.full(s, nan, dtype=torch.float32, device=cuda)
                                    for s in ((n, 2), (n, 2, 2), (n,)))
    f.vis = torch.zeros((n,), dtype=torch.bool, device=cuda)
    f.image, f.alpha, f.depth = (torch.full((c, H, W), nan, dtype=torch.float32, device=cuda) for c in (3, 1, 1))
    fa = N.GsRenderFwdArgs()
    RZ._bind_frame_args(fa, cam, RZ._build_gaussians_struct(n, model._xyz, None, model._scaling, model._rotation,
                                                            model._features_dc, model._opacity,
                                                            opacity_is_logit=True),
                        (f.means2d, f.conics, f.radii, f.vis), (f.image, f.alpha, f.depth), f.frame_ws.view)
    RZ._bind_tile_ws(fa, f.tile_ws.view, int(capacity))
    assert fa.fb.tile_ws_bytes == f.tile_ws.nbytes and fa.fb.frame_ws_bytes == f.frame_ws.nbytes
    fa.key_base, fa.key_bits = window if window is not None else (0, 32)
    fa.depth_sort_msd = 1 if msd else 0
    fa.zero_slot_flags = 1
    fa.host_counters_dev, fa.host_counters_host = hc.dptr, hc.t.data_ptr()
    f.fa = fa
    return f


def device_frame(pkg, cuda, model, cam, capacity, window=None, msd=False, words=None, hc=None, backward=None):
    """One device-resident forward of (model, cam) on the current stream, no
    graph; with `backward` = (g_image, g_alpha, g_depth) the matching
    gs_render_backward too.  window: (key_base, key_bits) or None (32-bit
    keys).  words: int32 device tensor, [0] the sticky step flags, [1] the
    frame counter (None: neither is passed, the pinned sequence word is the
    frame's host_seq).  hc: a rasterizer._HostCounters shared between frames.
    Asserts that every guard is intact, and returns the frame read back."""
    RZ, N = pkg.rasterizer, pkg._native
    hc = RZ._HostCounters() if hc is None else hc
    f = _bind(pkg, cuda, model, cam, capacity, window, msd, hc)
    lib, fa, n = f.lib, f.fa, f.n
    for g in (f.frame_ws, f.tile_ws, f.pair_grads):
        g.refill()
    fa.device_counts = 1
    if words is not None:
        fa.step_flags, fa.frame_seq = words.data_ptr(), words.data_ptr() + 4
    else:
        fa.host_seq = hc.next_seq()
    f.host_seq = int(fa.host_seq)
    s = N.stream_ptr(cuda)
    N.check(lib.gs_render_forward(C.byref(fa), s), "gs_render_forward (device-resident, plain stream)")
    assert fa.M == -1 and fa.T == -1, "a device-resident forward leaves M and T on the device"
    f.grads = None
    if backward is not None:
        f.cot = tuple(t.detach().to(cuda, torch.float32).contiguous() for t in backward)
        f.grads = {k: torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)
                   for k, shape in zip(GRAD_NAMES, ((n, 3), (n, 3), (n, 4), (n, 3), (n,)))}
        ba = N.GsRenderBwdArgs()
        ba.cam, ba.fb, ba.g = fa.cam, fa.fb, fa.g
        ba.M = ba.T = -1
        ba.tile_alt = fa.tile_alt
        ba.means2d, ba.conics, ba.vis = fa.means2d, fa.conics, fa.vis
        ba.image, ba.alpha, ba.depth = fa.image, fa.alpha, fa.depth
        ba.g_image, ba.g_alpha, ba.g_depth = (t.data_ptr() for t in f.cot)
        ba.pair_grads = f.pair_grads.buf.data_ptr()
        ba.flags_zeroed, ba.project, ba.device_counts = 1, 1, 1
        gr = f.grads
        ba.d_xyz, ba.d_scaling, ba.d_rotation = gr["xyz"].data_ptr(), gr["scaling"].data_ptr(), gr["rotation"].data_ptr()
        ba.d_color_logits, ba.d_opacity = gr["color"].data_ptr(), gr["opacity"].data_ptr()
        N.check(lib.gs_render_backward(C.byref(ba), s), "gs_render_backward (device-resident, plain stream)")
        f.ba = ba
    torch.cuda.synchronize(cuda)
    for name in ("frame_ws", "tile_ws", "pair_grads"):
        assert getattr(f, name).guard_intact(), f"a kernel wrote past the end of {name}"
    _read_back(f)
    return f


def _read_back(f):
    n, cap = f.n, f.capacity
    N = f.native
    fo = N.frame_offsets(n, f.W, f.H, f.cam.tile_size)
    to = N.tile_offsets(cap, f.tiles, f.cells, f.groups)
    assert fo.total == f.frame_ws.nbytes and to.total == f.tile_ws.nbytes
    fw, tw = f.frame_ws.view, f.tile_ws.view

    def words(buf, off, count):
        return buf[off:off + 4 * count].view(torch.int32).cpu().numpy().view(np.uint32)
    f.counters = [int(v) for v in words(fw, fo.counters, 6)]
    f.M, f.T, f.zmin, f.zmax, f.status, f.T_eff = f.counters
    f.rects = fw[fo.rects:fo.rects + 8 * n].view(torch.int32).view(n, 2).clone()
    f.records = fw[fo.records:fo.records + 48 * n].view(torch.float32).view(n, 12).clone()
    f.pair_offset = fw[fo.pair_offset:fo.pair_offset + 4 * n].view(torch.int32).clone()
    f.ranges = fw[fo.ranges:fo.ranges + 8 * f.tiles].view(torch.int32).view(f.tiles, 2).clone()
    alt = int(f.fa.tile_alt)
    # keys 0 / 1, Gaussian ids 0 / 1, all `cap` entries
    f.tile_halves = [words(tw, off, cap) for off in (to.tk0, to.tk1, to.tv0, to.tv1)]
    f.sorted_keys, f.sorted_gauss = f.tile_halves[alt], f.tile_halves[2 + alt]
    f.slot_flags = tw[to.flags:to.flags + cap * f.groups].cpu().numpy()
    f.pinned = None
    if f.hc.dptr is not None:
        f.pinned = [int(v) & 0xFFFFFFFF for v in f.hc.np[:8].tolist()]


def host_forward_status(pkg, cuda, model, cam, capacity, window, msd=False):
    """gs_render_forward on the host path (device_counts = 0) with the window
    given: (gs_status, M, T, zmin, zmax) as the call returns them."""
    RZ, N = pkg.rasterizer, pkg._native
    hc = RZ._HostCounters()
    assert hc.dptr is not None, "the host path's frame entry point needs pinned counters the device can address"
    f = _bind(pkg, cuda, model, cam, capacity, window, msd, hc)
    f.fa.host_seq = hc.next_seq()
    st = f.lib.gs_render_forward(C.byref(f.fa), N.stream_ptr(cuda))
    torch.cuda.synchronize(cuda)
    assert f.frame_ws.guard_intact() and f.tile_ws.guard_intact()
    fa = f.fa
    return int(st), int(fa.M), int(fa.T), int(fa.depth_min_bits), int(fa.depth_max_bits)


# -------------------------------------------------------------- statements
def index_statement(means2d, radii, vis, z, w, h, tile):
    """The index work of a frame from its own projections (numpy arrays):
    the depth order (ascending z, ties by Gaussian index), each Gaussian's
    pixel rectangle by the reference's int() rule (renderer.py:278-293), and
    the tile lists -- every (tile, Gaussian) of the depth-ordered rectangles,
    stable by tile id (renderer.py:294-298) -- with their [start, end)."""
    s = SimpleNamespace()
    vis = vis.astype(bool)
    s.vidx = np.nonzero(vis)[0]
    s.order = s.vidx[np.argsort(z[s.vidx], kind="stable")]
    mx, my = means2d.T.astype(np.float32)
    ri = np.trunc(radii).astype(np.int64)
    icx, icy = np.trunc(mx).astype(np.int64), np.trunc(my).astype(np.int64)
    s.x0, s.x1 = np.maximum(icx - ri, 0), np.minimum(icx + 1 + ri, w)
    s.y0, s.y1 = np.maximum(icy - ri, 0), np.minimum(icy + 1 + ri, h)
    s.ne = (s.x0 < s.x1) & (s.y0 < s.y1)
    s.tiles_x, s.tiles_y = (w + tile - 1) // tile, (h + tile - 1) // tile
    og = s.order[s.ne[s.order]]
    nx = (s.x1[og] - 1) // tile - s.x0[og] // tile + 1
    kk = nx * ((s.y1[og] - 1) // tile - s.y0[og] // tile + 1)
    gs = np.repeat(og, kk)
    local = np.arange(int(kk.sum())) - np.repeat(np.cumsum(kk) - kk, kk)  # rank in the rectangle, row-major
    nxr = np.repeat(nx, kk)
    keys = (np.repeat(s.y0[og] // tile, kk) + local // nxr) * s.tiles_x + np.repeat(s.x0[og] // tile, kk) + local % nxr
    srt = np.argsort(keys, kind="stable")
    s.T = len(keys)
    s.keys, s.gauss = keys[srt], gs[srt]
    s.counts = np.bincount(keys, minlength=s.tiles_x * s.tiles_y)
    s.starts = np.concatenate([[0], np.cumsum(s.counts)[:-1]])
    return s


def frame_status(pkg, M, T, zmin, zmax, capacity, window):
    """(counters[4], counters[5]) of a device-resident frame."""
    RZ, N = pkg.rasterizer, pkg._native
    status = 0
    if T > capacity:
        status |= N.GS_FRAME_NEED_CAPACITY
    if not RZ.window_holds(window, zmin, zmax):
        status |= N.GS_FRAME_WINDOW_MISS
    if M == 0:
        status |= N.GS_FRAME_EMPTY
    return status, (0 if status else T)


def _np(t):
    return t.detach().cpu().numpy()


def assert_frame_matches_host(pkg, f, h, window=None):
    """A device-resident frame that succeeded, against the host path's frame
    `h` of the same scene (host_frame, with gradients when f has them) and the
    index statement."""
    M, T = h.M, h.T
    assert f.counters == [M, T, h.zmin, h.zmax, 0, T], (f.counters, (M, T, h.zmin, h.zmax))
    assert (f.status, f.T_eff) == frame_status(pkg, M, T, h.zmin, h.zmax, f.capacity, window)
    if f.pinned is not None:
        assert f.pinned[:4] == [M, T, h.zmin, h.zmax] and f.pinned[5] == 0
    st = index_statement(_np(f.means2d), _np(f.radii), _np(f.vis), _np(f.records[:, 9]), f.W, f.H, f.cam.tile_size)
    assert st.T == T and len(st.vidx) == M
    assert np.array_equal(f.sorted_keys[:T].astype(np.int64), st.keys)
    assert np.array_equal(f.sorted_gauss[:T].astype(np.int64), st.gauss)
    assert np.array_equal(f.sorted_gauss[:T], _np(h.sorted_gauss[:T]).view(np.uint32))
    # nothing is emitted or sorted past T: the garbage is where it was
    for half in f.tile_halves:
        assert np.all(half[T:] == FILL_WORD)
    assert np.all(f.slot_flags[T * f.groups:] == FILL), "slot flags past T were written"
    assert torch.equal(f.ranges, h.ranges) and torch.equal(f.rects, h.rects)
    assert torch.equal(f.pair_offset, h.pair_offset)
    rng_ = _np(f.ranges).astype(np.int64)
    nz = st.counts > 0
    assert np.array_equal(rng_[nz, 0], st.starts[nz]) and np.array_equal(rng_[nz, 1], (st.starts + st.counts)[nz])
    assert np.all(rng_[~nz, 0] == rng_[~nz, 1])
    for name in ("image", "alpha", "depth", "means2d", "conics", "radii", "vis"):
        a, b = getattr(f, name), getattr(h, name)
        assert torch.equal(a, b), name
        assert not torch.isnan(a.float()).any(), name
    if f.grads is not None:
        for name in GRAD_NAMES:
            assert torch.equal(f.grads[name], h.grads[name]), name
            assert torch.isfinite(f.grads[name]).all(), name


def assert_failed_frame(pkg, f, want_counters, empty):
    """A device-resident frame the count flagged: `want_counters` (six words),
    empty lists, cleared rectangles, nothing emitted, the image, alpha and
    depth of a frame that draws nothing (`empty`: host_frame of the
    behind-camera scene of the same camera), zero gradients."""
    assert f.counters == want_counters, (f.counters, want_counters)
    assert f.status != 0 and f.T_eff == 0
    if f.pinned is not None:
        assert f.pinned[:4] == want_counters[:4] and f.pinned[5] == f.status
    rng_ = _np(f.ranges)
    assert np.all(rng_[:, 0] == rng_[:, 1]), "every tile's list is empty"
    assert bool((f.rects == 1).all()), "every rectangle is cleared to (1, 1)"
    for half in f.tile_halves:
        assert np.all(half == FILL_WORD), "a failed frame emits and sorts nothing"
    assert np.all(f.slot_flags == FILL), "a failed frame has no slot to flag"
    assert empty.M == 0
    assert not failed_frame_image_differences(f, empty), failed_frame_image_differences(f, empty)
    for name in ("image", "alpha", "depth"):
        assert torch.equal(getattr(f, name), getattr(empty, name)), name
    if f.grads is not None:
        for name in GRAD_NAMES:
            g = f.grads[name]
            assert torch.isfinite(g).all() and bool((g == 0).all()), name


def failed_frame_image_differences(f, empty):
    """Per colour channel (the failed frame's values, the empty host frame's
    values, pixels that differ): empty when the two images are bit-identical."""
    diffs = []
    for c in range(3):
        a, b = f.image[c], empty.image[c]
        if not torch.equal(a, b):
            diffs.append((c, sorted(set(a.flatten().tolist()))[:4], sorted(set(b.flatten().tolist()))[:4],
                          int((a != b).sum())))
    return diffs
