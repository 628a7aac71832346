"""Host-side logic of the drop-in API (no GPU needed)."""
import math

import numpy as np
import pytest
import torch


class _Cam:
    _width, _height, _FoVx, _FoVy = 48, 32, math.radians(70), math.radians(50)

    def world_view_transform(self):
        m = torch.eye(4)
        m[:3, 3] = torch.tensor([0.1, 0.2, 0.3])
        return m


def test_camera_params_follow_reference_intrinsics(pkg):
    """renderer.py:140-152: fx = 0.5 W / tan(FoVx/2) from the CAMERA size,
    image size from the SETTINGS."""
    st = pkg.RenderSettings(image_height=20, image_width=30, bg_color=torch.tensor([0.1, 0.2, 0.3]))
    c = pkg.camera_params(_Cam(), st)
    assert (c.image_width, c.image_height) == (30, 20)
    assert c.fx == pytest.approx(0.5 * 48 / math.tan(math.radians(35)))
    assert c.fy == pytest.approx(0.5 * 32 / math.tan(math.radians(25)))
    assert (c.cx, c.cy) == (24.0, 16.0)
    assert c.view[3] == pytest.approx(0.1) and c.view[7] == pytest.approx(0.2) and c.view[11] == pytest.approx(0.3)
    assert c.tiles_x == 2 and c.tiles_y == 2
    assert c.bg == pytest.approx((0.1, 0.2, 0.3))


def test_world_view_as_tensor_attribute(pkg):
    class Cam2(_Cam):
        pass
    cam = Cam2()
    cam.world_view_transform = torch.eye(4)
    c = pkg.camera_params(cam, pkg.RenderSettings(8, 8, torch.zeros(3)))
    assert c.view == tuple([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


def test_no_cpu_fallback(pkg):
    """The product path must fail loudly without a HIP device tensor."""
    m = pkg.GaussianModel()
    m.create_from_random(10)
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.GaussianRenderer().render(_Cam(), m, pkg.RenderSettings(8, 8, torch.zeros(3)))


def test_renderer_constructor_range(pkg):
    """GaussianRenderer(tile_size, radius_min, radius_max) (renderer.py:24-28):
    any tile edge >= 1 (the reference takes any int; 0 divides by zero there)
    and finite radii are taken as given.  The kernels' edge is the tile_size,
    or max(W, H) when it is larger (one tile holds the image either way:
    effective_tile); tiles of many cells replay them in batches within a
    memory budget (rasterizer.cell_batch)."""
    for t in (1, 8, 12, 16, 32, 256, 257, 1000, 10 ** 6):
        r = pkg.GaussianRenderer(tile_size=t, radius_max=80.0)
        assert r.tile_size == t and r.radius_max == 80.0
    c = pkg.camera_params(_Cam(), pkg.RenderSettings(20, 30, torch.zeros(3)), tile_size=8)
    assert (c.tiles_x, c.tiles_y, c.cells) == (4, 3, 1)
    assert pkg.camera_params(_Cam(), pkg.RenderSettings(20, 30, torch.zeros(3)), tile_size=32).cells == 16
    # a tile above the image: one tile of max(W, H) = 30 px
    for t in (31, 1000, 10 ** 9):
        c = pkg.camera_params(_Cam(), pkg.RenderSettings(20, 30, torch.zeros(3)), tile_size=t)
        assert (c.tile_size, c.tiles_x, c.tiles_y) == (30, 1, 1)
    big = pkg.RenderSettings(4000, 4000, torch.zeros(3))
    assert pkg.camera_params(_Cam(), big, tile_size=300).groups == 1444  # one partial per 8x8 cell
    assert pkg.camera_params(_Cam(), big, tile_size=256).groups == 1024
    # tiles above 4096 px (round 6; ABI 21 stopped at 4096): a 5000-px image as
    # one tile, or in 2 x 2 tiles of 4500 px
    assert pkg._native.GS_MAX_TILE == 16384
    c = pkg.camera_params(_Cam(), pkg.RenderSettings(5000, 5000, torch.zeros(3)), tile_size=10 ** 6)
    assert (c.tile_size, c.tiles_x, c.tiles_y, c.cells) == (5000, 1, 1, 625 ** 2)
    c = pkg.camera_params(_Cam(), pkg.RenderSettings(5000, 5000, torch.zeros(3)), tile_size=4500)
    assert (c.tile_size, c.tiles_x, c.tiles_y) == (4500, 2, 2)
    # an image wider than GS_MAX_TILE cannot be one tile: a tile edge that would
    # cover it raises, where the reference renders it as one tile
    with pytest.raises(ValueError):
        pkg.camera_params(_Cam(), pkg.RenderSettings(100, 40000, torch.zeros(3)), tile_size=10 ** 6)
    with pytest.raises(ValueError):  # a 70000-px image in tiles above 16384 px that do not cover it
        pkg.camera_params(_Cam(), pkg.RenderSettings(100, 70000, torch.zeros(3)), tile_size=35000)
    for bad in (dict(tile_size=0), dict(tile_size=-3), dict(tile_size=8.5), dict(radius_max=float("inf")),
                dict(radius_min=3.0, radius_max=2.0)):
        with pytest.raises(ValueError):
            pkg.GaussianRenderer(**bad)


def test_cell_batches_and_bitmap_budget(pkg):
    """Bounded memory at any tile size: the backward's partials
    [T, G] and the forward's liveness bitmap stay within their budgets; the
    default tile's four cells never batch (the performance path), whatever T."""
    RZ = pkg.rasterizer
    lib = pkg._native.load()
    B = RZ.PARTIAL_BUDGET_BYTES
    assert RZ.cell_batch(4, 10 ** 9) == 4
    assert RZ.cell_batch(16, 10 ** 5) == 16
    for cells, T in ((1444, 1_050_000), (57_600, 1_000_000), (262_144, 4_000_000), (1024, 50_000_000)):
        g = RZ.cell_batch(cells, T)
        assert 1 <= g <= cells and (g == 1 or 41 * T * g <= B)
    # ADVICE r04's case: 1080p, one 1920-px tile (57,600 cells), 1M entries: ~7 GB of bitmap -> none
    assert RZ.live_bitmap_bytes(lib, 57_600, 1_000_000, 1) == 0
    assert RZ.live_bitmap_bytes(lib, 4, 4_411_397, 8160) == 8 * 4 * (4_411_397 // 64 + 8160 + 2)
    small = RZ.live_bitmap_bytes(lib, 1444, 3000, 6)
    assert 0 < small <= RZ.LIVE_BUDGET_BYTES


@pytest.mark.parametrize("n,W,H,tile", [(0, 64, 48, 16), (300, 64, 48, 20), (1_000_000, 1920, 1080, 16)])
def test_named_workspace_offsets(pkg, n, W, H, tile):
    """_native.frame_offsets / tile_offsets name gs_frame_offsets' and
    gs_tile_offsets' arrays in the library's order: the byte offsets do not
    decrease along the tuple, are 256-aligned, and `total` is what the sizing
    call returns -- with and without a liveness bitmap."""
    N, RZ = pkg._native, pkg.rasterizer
    lib = N.load()
    assert N.FRAME_OFFSET_NAMES == ("records", "rects", "keys", "vals", "key_minmax", "counters", "sort_ws", "bin_ws",
                                    "pair_offset", "ranges", "pix_flags", "cell_neval", "grad_sums", "total")
    assert N.TILE_OFFSET_NAMES == ("tk0", "tk1", "tv0", "tv1", "sort_ws", "live", "flags", "total", "live_words")
    fo = N.frame_offsets(n, W, H, tile)
    assert fo._fields == N.FRAME_OFFSET_NAMES
    assert list(fo) == sorted(fo) and all(o % 256 == 0 for o in fo)
    assert fo.total == lib.gs_frame_workspace_bytes(n, W, H, tile)
    tiles, cells = -(-W // tile) * -(-H // tile), (-(-tile // 8)) ** 2
    for cap in (1, 4096, 4_411_397):
        groups = RZ.flag_groups(cells, cap, lib.gs_partial_groups(tile))
        for live_cells in (0, cells):
            to = N.tile_offsets(cap, tiles, live_cells, groups)
            assert to._fields == N.TILE_OFFSET_NAMES
            offsets = list(to[:-1])  # (live_words is a count)
            assert offsets == sorted(offsets) and all(o % 256 == 0 for o in offsets)
            assert to.total == lib.gs_tile_workspace_bytes(cap, tiles, live_cells, groups)
            assert to.live_words == (lib.gs_blend_live_words(cap, tiles) if live_cells else 0)
            assert to.flags - to.live >= 8 * live_cells * to.live_words and to.total - to.flags >= cap * groups


@pytest.mark.parametrize("cap", (1, 4096, 4_411_397))
@pytest.mark.parametrize("cells", (1, 4, 9, 1444, 57_600))
def test_flag_groups_hold_every_frame(pkg, cells, cap):
    """rasterizer.flag_groups: cap * flag_groups slot flags hold [T,
    frame_groups(T)] at T = cap and at T = 1, in no more flags per entry than
    the byte count the stage path allocated before the tile workspace carried
    them (that rule, restated here)."""
    RZ = pkg.rasterizer
    tile = 8 * math.isqrt(cells)
    cam = RZ.CameraParams(1920, 1080, 1000.0, 1000.0, 960.0, 540.0, (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0),
                          (0.0, 0.0, 0.0), tile_size=tile)
    assert cam.cells == cells
    groups, budget = cam.groups, RZ.PARTIAL_BUDGET_BYTES
    fg = RZ.flag_groups(cells, cap, groups)
    for T in (cap, 1):
        assert cap * fg >= cam.frame_groups(T) * T
    if 0 < groups < cells:
        flag_bytes = groups * cap
    elif cells <= 4:
        flag_bytes = cells * cap
    else:
        flag_bytes = max(min(cells * cap, budget // 41), cap)
    assert 1 <= fg <= -(-flag_bytes // cap)


def test_gaussian_model_layout(pkg):
    """test_gaussian_model.py:35-72 restated for this package's model."""
    m = pkg.GaussianModel()
    m.create_from_random(64, 1.0, generator=torch.Generator().manual_seed(0))
    assert m._xyz.shape == (64, 3) and m._features_dc.shape == (64, 1, 3)
    assert m._features_rest.shape == (64, 15, 3) and m._scaling.shape == (64, 3)
    assert m._rotation.shape == (64, 4) and m._opacity.shape == (64, 1)
    assert m.get_features.shape == (64, 16, 3)
    assert torch.all(m.get_scaling > 0)
    assert torch.allclose(m.get_rotation.norm(dim=-1), torch.ones(64), atol=1e-5)
    a = m.get_opacity
    assert torch.all(a > 0) and torch.all(a < 1)


def test_covariance_property_works(pkg):
    """Reference get_covariance is broken (gaussian_model.py:127); ours equals
    compute_3d_covariance and the oracle's restatement."""
    import golden_io as G
    m = pkg.GaussianModel()
    m.create_from_random(32, generator=torch.Generator().manual_seed(1))
    cov = m.get_covariance.detach().numpy()
    ref = G.oracle().covariance(m._scaling.detach().numpy(), m._rotation.detach().numpy())
    assert np.allclose(cov, ref, atol=1e-6, rtol=1e-5)


def test_camera_world_view_matches_reference_producer(pkg):
    """CameraUtils.build_world_view_matrix (camera.py:80-141): C2W -> W2C."""
    ang = 0.4
    R = np.array([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1]], np.float32)
    C = np.array([1.0, -2.0, 0.5], np.float32)
    cam = pkg.Camera(0, R, C, 1.0, 1.0, None, "x", 16, 16)
    wv = cam.world_view_transform().numpy()
    assert np.allclose(wv[:3, :3], R.T, atol=1e-6)
    assert np.allclose(wv[:3, 3], -R.T @ C, atol=1e-6)
    assert np.allclose(cam.camera_center.numpy(), C, atol=1e-5)


def test_synthetic_scene_distribution(pkg):
    sc = pkg.synthetic.make_scene(5000, 192, 108, seed=0)
    z = sc.xyz[:, 2]
    assert z.min() >= 2 and z.max() <= 6
    s = sc.scaling.exp()
    assert s.min() >= 0.002 - 1e-6 and s.max() <= 0.01 + 1e-6
    assert torch.allclose(sc.rotation.norm(dim=1), torch.ones(5000), atol=1e-5)
    sc2 = pkg.synthetic.make_scene(5000, 192, 108, seed=0)
    assert torch.equal(sc.xyz, sc2.xyz)


def test_depth_window_choice(pkg):
    """rasterizer.depth_window: a window of key bits around the previous
    frame's visible fp32 depth bits, widened by 1/8 of the range each side;
    None when the range needs all 32 bits.  Visible keys stay below
    255 << (bits - 8): the MSD depth sort's top bucket is the culled sentinel's."""
    import struct
    RZ = pkg.rasterizer
    bits = lambda z: struct.unpack("<I", struct.pack("<f", z))[0]
    w = RZ.depth_window(bits(2.0), bits(6.0))  # the C3 distribution: 24 bits, 3 passes
    assert w is not None and w[1] <= 24
    assert RZ.window_holds(w, bits(2.0), bits(6.0)) and RZ.window_holds(w, bits(2.1), bits(5.5))
    assert not RZ.window_holds(w, bits(0.5), bits(6.0)) and not RZ.window_holds(w, bits(2.0), bits(60.0))
    w = RZ.depth_window(bits(0.01), bits(1000.0))  # 28 bits: no LSD pass saved, but the MSD sort's
    assert w is not None and 24 < w[1] < 32 and RZ.window_holds(w, bits(0.01), bits(1000.0))
    assert RZ.depth_window(bits(1e-38), bits(3e38)) is None  # all 32 bits
    assert RZ.depth_window(0xFFFFFFFF, 0) is None  # nothing visible
    assert RZ.window_holds(None, bits(0.01), bits(1e30))
    base, nb = RZ.depth_window(bits(3.0), bits(3.0))  # a single depth
    assert nb >= 1 and RZ.window_holds((base, nb), bits(3.0), bits(3.0))


def test_render_input_validation(pkg, monkeypatch):
    """Inputs the kernels would misread raise before any launch: wrong row
    counts or shapes, non-float dtypes, a missing covariance; other float
    dtypes are cast to fp32 (on the autograd tape)."""
    import sys
    R = sys.modules[pkg.__name__ + ".rasterizer"]
    monkeypatch.setattr(R, "_check_inputs", lambda x: None)  # (no HIP device here)
    n = 4

    def call(**kw):
        a = dict(xyz=torch.zeros(n, 3), cov3d=torch.zeros(n, 3, 3), scaling=None, rotation=None,
                 logits=torch.zeros(n, 3), opacity=torch.zeros(n))
        a.update(kw)
        R.rasterize(None, a["xyz"], a["cov3d"], a["scaling"], a["rotation"], a["logits"], a["opacity"])

    with pytest.raises(ValueError, match="opacity"):
        call(opacity=torch.zeros(n + 1))
    with pytest.raises(ValueError, match="cov3d"):
        call(cov3d=torch.zeros(n, 3))
    with pytest.raises(ValueError, match="xyz"):
        call(xyz=torch.zeros(n, 2))
    with pytest.raises(TypeError, match="colour"):
        call(logits=torch.zeros(n, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="covariance"):
        call(cov3d=None)
    with pytest.raises(ValueError, match="rotation"):
        call(cov3d=None, scaling=torch.zeros(n, 3), rotation=torch.zeros(n, 3))
    # fp64 passes validation (cast), then reaches the launch path (camera None here)
    with pytest.raises(AttributeError):
        call(logits=torch.zeros(n, 3, dtype=torch.float64))


def test_host_scalars_and_struct_caches(pkg):
    """camera_params reads the view and background as fp32 values from any
    tensor / sequence form; the ABI structs cached by value
    (CameraParams.to_struct, rasterizer._gaussians_struct) follow every
    change of what they hold."""
    import torch
    R, RZ = pkg.renderer, pkg.rasterizer
    wv = torch.arange(16, dtype=torch.float64).reshape(4, 4) / 7
    want = [float(v) for v in wv.float().reshape(-1)]
    assert R._host_f32(wv, 16) == want
    assert R._host_f32(wv.float(), 16) == want
    assert R._host_f32(wv.float().reshape(-1), 16) == want
    assert R._host_f32([0.1, 0.2, 0.3], 3) == [float(v) for v in torch.tensor([0.1, 0.2, 0.3])]
    with pytest.raises(ValueError):
        R._host_f32(torch.zeros(3, 3), 16)
    cp = RZ.CameraParams(64, 48, 50.0, 50.0, 32.0, 24.0, tuple(range(12)), (0.0, 0.5, 1.0))
    a = cp.to_struct()
    assert a is cp.to_struct() and (a.image_width, a.image_height, a.bg[1]) == (64, 48, 0.5)
    cp2 = RZ.CameraParams(64, 48, 50.0, 50.0, 32.0, 24.0, tuple(range(12)), (0.0, 0.25, 1.0))
    assert cp2.to_struct().bg[1] == 0.25 and a.bg[1] == 0.5
    xyz, sc, rot = torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 4)
    col, op = torch.zeros(5, 1, 3), torch.zeros(5, 1)
    g = RZ._gaussians_struct(5, xyz, None, sc, rot, col, op, True)
    assert g is RZ._gaussians_struct(5, xyz, None, sc, rot, col, op, True)
    assert (g.xyz, g.color_logits, g.color_stride, g.opacity_is_logit) == (xyz.data_ptr(), col.data_ptr(), 3, 1)
    g2 = RZ._gaussians_struct(5, xyz, None, sc, rot, col, op, False)
    assert g2.opacity_is_logit == 0 and g.opacity_is_logit == 1
    xyz2 = torch.zeros(5, 3)
    assert RZ._gaussians_struct(5, xyz2, None, sc, rot, col, op, True).xyz == xyz2.data_ptr()


def test_fused_adam_runs_step_hooks(pkg):
    """torch.optim.Optimizer's step pre / post hooks (per optimizer
    and global) run around FusedAdam.step and step_ranges, in torch's order;
    a pre hook may rewrite the arguments.  (No gradients: nothing launches.)"""
    import torch
    from torch.optim.optimizer import register_optimizer_step_post_hook
    p = torch.nn.Parameter(torch.zeros(3))
    opt = pkg.optim.FusedAdam([p])
    calls = []
    h1 = opt.register_step_pre_hook(lambda o, a, k: calls.append(("pre", a)))
    h2 = opt.register_step_post_hook(lambda o, a, k: calls.append(("post", a)))
    h3 = register_optimizer_step_post_hook(lambda o, a, k: calls.append(("global_post", a)))
    try:
        assert opt.step() is None
        opt.step_ranges([(0, 3)])
    finally:
        h1.remove(), h2.remove(), h3.remove()
    assert [c[0] for c in calls] == ["pre", "post", "global_post"] * 2
    assert calls[0][1] == (None,) and calls[3][1] == ([(0, 3)], None)
    calls.clear()
    opt.step()
    assert calls == []


@pytest.fixture
def rz_state(pkg):
    """rasterizer with its per-device guesses emptied for a test, restored after."""
    RZ = pkg.rasterizer
    dicts = (RZ._T_SEEN, RZ._DEPTH_HIST, RZ._WINDOW_STATE, RZ._MSD_BACKOFF)
    saved, msd = [dict(d) for d in dicts], RZ._DEPTH_MSD
    for d in dicts:
        d.clear()
    try:
        yield RZ
    finally:
        RZ._DEPTH_MSD = msd
        for d, s in zip(dicts, saved):
            d.clear()
            d.update(s)


def _f32_bits(z):
    import struct
    return struct.unpack("<I", struct.pack("<f", z))[0]


def test_capacity_guess(rz_state):
    """The tile-entry capacity tried before T is known: nothing without a
    frame seen, else the last T and a quarter, plus 4096."""
    RZ, dev = rz_state, torch.device("cuda:0")
    assert RZ._capacity_guess(dev) == 0
    RZ._T_SEEN[dev] = 16
    assert RZ._capacity_guess(dev) == 4116
    assert RZ._capacity_guess(torch.device("cuda:1")) == 0


def test_depth_keys_state_machine(rz_state):
    """_depth_keys: 32-bit keys without a window; the MSD sort for windows of
    9..31 bits unless switched off or backing off; the backoff is counted down
    only by a frame that wanted the MSD sort, and never by a capture."""
    RZ, dev = rz_state, torch.device("cuda:0")
    assert RZ._depth_keys(dev, True) == (None, 0, 32, False)
    RZ._DEPTH_HIST[dev] = [(_f32_bits(2.0), _f32_bits(6.0))]
    w = RZ._window_for(dev)
    assert w is not None and 9 <= w[1] <= 31
    assert RZ._depth_keys(dev, True) == (w, w[0], w[1], True)
    assert RZ._depth_keys(dev, False) == (None, 0, 32, False)
    assert RZ._depth_keys(dev, True, window=(5, 12)) == ((5, 12), 5, 12, True)  # (GraphedStep.window)
    assert RZ._depth_keys(dev, True, window=None) == (None, 0, 32, False)
    assert dev not in RZ._MSD_BACKOFF
    RZ._MSD_BACKOFF[dev] = 2
    assert RZ._depth_keys(dev, True, consume=False) == (w, w[0], w[1], False)
    assert RZ._MSD_BACKOFF[dev] == 2
    assert RZ._depth_keys(dev, True) == (w, w[0], w[1], False)
    assert RZ._MSD_BACKOFF[dev] == 1
    assert RZ._depth_keys(dev, False)[3] is False and RZ._MSD_BACKOFF[dev] == 1  # (no window: not an MSD frame)
    assert RZ._depth_keys(dev, True)[3] is False and RZ._MSD_BACKOFF[dev] == 0
    assert RZ._depth_keys(dev, True)[3] is True  # (the backoff is spent)
    RZ._MSD_BACKOFF[dev] = 2
    RZ._DEPTH_MSD = False
    assert RZ._depth_keys(dev, True) == (w, w[0], w[1], False) and RZ._MSD_BACKOFF[dev] == 2
    RZ._DEPTH_MSD = True
    RZ._DEPTH_HIST[dev] = [(_f32_bits(3.0), _f32_bits(3.0))]  # a single depth: a window of a few bits
    w = RZ._window_for(dev)
    assert w is not None and w[1] <= 8
    assert RZ._depth_keys(dev, True) == (w, w[0], w[1], False) and RZ._MSD_BACKOFF[dev] == 2


def test_frame_missed_and_done(rz_state):
    """A frame to render again: a poisoned depth max starts the MSD backoff
    and is no window miss, anything else is one; both keep the frame's T.  A
    finished frame leaves its T and its depth range."""
    RZ, dev = rz_state, torch.device("cuda:0")
    misses = lambda: RZ.depth_window_stats(dev)["misses"]
    RZ._frame_missed(dev, 0xFFFFFFFF, 700)
    assert RZ._MSD_BACKOFF[dev] == RZ._MSD_BACKOFF_FRAMES and misses() == 0 and RZ._T_SEEN[dev] == 700
    RZ._MSD_BACKOFF.clear()
    RZ._frame_missed(dev, _f32_bits(9.0), 900)
    assert misses() == 1 and dev not in RZ._MSD_BACKOFF and RZ._T_SEEN[dev] == 900
    RZ._frame_missed(dev, 0, 5)
    assert misses() == 2 and RZ._T_SEEN[dev] == 5
    frames = RZ.depth_window_stats(dev)["frame"]
    RZ._frame_done(dev, 1234, _f32_bits(2.0), _f32_bits(6.0))
    assert RZ._T_SEEN[dev] == 1234 and RZ._DEPTH_HIST[dev] == [(_f32_bits(2.0), _f32_bits(6.0))]
    assert RZ.depth_window_stats(dev)["frame"] == frames + 1
    RZ._frame_done(dev, 0, 0xFFFFFFFF, 0)  # nothing visible: counted, no range
    assert RZ._T_SEEN[dev] == 0 and len(RZ._DEPTH_HIST[dev]) == 1
    assert RZ.depth_window_stats(dev)["frame"] == frames + 2


def test_host_counter_sequence(pkg):
    """The counters' sequence word: 1 .. 2^31 - 1, wrapping past the cleared 0."""
    hc = object.__new__(pkg.rasterizer._HostCounters)  # (no pinned buffer here)
    hc.seq = 0
    assert [hc.next_seq(), hc.next_seq()] == [1, 2] and hc.seq == 2
    hc.seq = 0x7FFFFFFE
    assert [hc.next_seq(), hc.next_seq()] == [0x7FFFFFFF, 1]


def test_grad_buffers(pkg):
    """_grad_buffers: the caller's tensors from `out` are the kernels'
    destinations (viewed to the kernels' shapes), the rest is allocated; the
    row-range callback and its chunk count are taken out of `out`."""
    RZ, n, cpu = pkg.rasterizer, 6, torch.device("cpu")
    ready = lambda lo, hi: None
    out = {"xyz": torch.zeros(n * 3), "opacity": torch.zeros(n, 1), "color": torch.zeros(n, 1, 3),
           "_rows_ready": ready, "_chunks": 3}
    (d_xyz, d_cov, d_scl, d_rot, d_col, d_op, d_sh), rows_ready, chunks = RZ._grad_buffers(out, n, True, 0, cpu)
    assert rows_ready is ready and chunks == 3
    assert "_rows_ready" in out and "_chunks" in out  # (the caller's dict is left alone)
    assert d_xyz.data_ptr() == out["xyz"].data_ptr() and d_xyz.shape == (n, 3)
    assert d_op.data_ptr() == out["opacity"].data_ptr() and d_op.shape == (n,)
    assert d_col.data_ptr() == out["color"].data_ptr() and d_col.shape == (n, 3)
    assert d_cov is None and d_sh is None
    assert d_scl.shape == (n, 3) and d_rot.shape == (n, 4) and d_scl.dtype == torch.float32
    grads, rows_ready, chunks = RZ._grad_buffers({"_chunks": 4}, n, False, 2, cpu)
    assert rows_ready is None and chunks == 1  # (no callback: one range)
    assert grads[1].shape == (n, 3, 3) and grads[2] is None and grads[3] is None
    assert grads[6].shape == (n, pkg._native.GS_SH_REST, 3)
    grads, rows_ready, chunks = RZ._grad_buffers(None, n, True, 0, cpu)
    assert rows_ready is None and chunks == 1 and grads[0].shape == (n, 3)
    assert RZ._grad_buffers({"_rows_ready": ready}, n, True, 0, cpu)[1:] == (ready, 1)


class _FakeLib:
    """Records the projection backward's calls: (entry point, the struct passed, its g.n)."""

    def __init__(self):
        self.calls = []

    def gs_project_backward(self, ref, stream):
        self.calls.append(("gs_project_backward", ref._obj, ref._obj.g.n))
        return 0

    def gs_project_backward_pose(self, ref, stream):
        self.calls.append(("gs_project_backward_pose", ref._obj, ref._obj.bwd.g.n))
        return 0


def test_project_backward_ranges(pkg):
    """_project_backward_ranges: n * k // chunks row bounds, one launch per
    range and its rows_ready right after; the struct itself for the whole
    range; with d_view one pose launch over every Gaussian."""
    RZ, N = pkg.rasterizer, pkg._native
    n = 10
    pb = N.GsProjectBwdArgs()
    pb.g.n = n
    lib, log = _FakeLib(), []

    def ready(lo, hi):
        log.append((lo, hi, len(lib.calls)))
    RZ._project_backward_ranges(lib, pb, n, 3, ready, None, None)
    assert [c[0] for c in lib.calls] == ["gs_project_backward"] * 3
    assert [c[2] for c in lib.calls] == [3, 3, 4] and all(c[1] is not pb for c in lib.calls)
    assert log == [(0, 3, 1), (3, 6, 2), (6, 10, 3)]  # (each range announced once it is queued)
    assert pb.g.n == n
    lib.calls.clear(), log.clear()
    RZ._project_backward_ranges(lib, pb, n, 1, ready, None, None)
    assert len(lib.calls) == 1 and lib.calls[0][1] is pb and log == [(0, 10, 1)]
    lib.calls.clear(), log.clear()
    RZ._project_backward_ranges(lib, pb, n, 1, None, None, None)
    assert len(lib.calls) == 1 and lib.calls[0][1] is pb
    lib.calls.clear()
    d_view = torch.zeros(12)
    RZ._project_backward_ranges(lib, pb, n, 3, ready, d_view, None)  # (the pose reduction wants one range)
    assert [(c[0], c[2]) for c in lib.calls] == [("gs_project_backward_pose", n)] and log == [(0, 10, 1)]
    assert lib.calls[0][1].d_view == d_view.data_ptr()
