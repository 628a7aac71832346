"""Device-resident frames (gs_render_forward / gs_render_backward with
device_counts = 1, the frame graph_step.GraphedStep replays and bench.py
times) at the edges of their capacity-sized stages, run on a plain stream
through tests/device_frame_util.py:

  * the tile sort sized by the capacity -- gs_internal_small_sort with n_dev
    up to 16384 entries, gs_internal_radix_sort_pairs with n_dev above -- with
    T == capacity, T == capacity - 1, and T a small or block-aligned part of
    the launch;
  * the frame status of k_bin_scan_partials (T > capacity, the depth-key
    window's two edges, M == 0), counters[5], the sticky step flags, the
    frame counter and the pinned words 4..7;
  * the failed-frame branch of k_bin_emit (cleared rectangles, nothing
    emitted, zero gradients).

Every comparison is bit-exact, against the host path's frame of the same
scene (32-bit depth keys) and the numpy statements of device_frame_util.
Workspaces are filled with garbage and guarded (see device_frame_util)."""
import numpy as np
import pytest
import torch

import device_frame_util as U

pytestmark = pytest.mark.gpu

W, H = 320, 240

# (W, H, capacity, T, n_base): T by construction (device_frame_util.scene_with_T)
_ONE_WG = [(W, H, 16384, t, nb) for t, nb in ((16384, 8000), (16383, 8000), (1025, 500), (1024, 500), (2, 0), (1, 0))]
_ONE_WG += [(W, H, 4096, 4096, 1500), (W, H, 4096, 4095, 1500)]
_RADIX = [(W, H, 16385, 16385, 8000), (W, H, 16385, 16384, 8000)]
_RADIX += [(W, H, 65536, t, nb) for t, nb in ((1, 0), (2047, 800), (2048, 800), (2049, 800), (4098, 1500),
                                               (20000, 10000))]
_ONE_TILE = [(16, 16, 4096, 300, 200), (16, 16, 16385, 300, 200)]
_TWO_TILES = [(32, 16, 4096, 301, 200)]
SUCCESS = _ONE_WG + _RADIX + _ONE_TILE + _TWO_TILES

_SCENES: dict = {}


def _scene(pkg, cuda, w, h, target, n_base):
    """(model, camera, cotangents, host frame) of the scene with T == target,
    built and rendered on the host path once per session and never modified."""
    key = (w, h, target, n_base)
    if key not in _SCENES:
        seed = n_base % 97 + (0 if target is None else target % 89)
        sc = U.scene_with_T(pkg, target, w, h, n_base, seed, cuda)
        model, cam = U.model_of(pkg, sc, cuda), U.camera(pkg, w, h)
        g = U.cotangents(h, w, cuda)
        host = U.host_frame(pkg, model, cam, g)
        assert target is None or host.T == target, f"the scene has T = {host.T} on the host path, not {target}"
        _SCENES[key] = (model, cam, g, host)
    return _SCENES[key]


def _empty(pkg, cuda, w, h):
    """The host path's frame of the behind-camera scene: what a frame that draws nothing looks like."""
    key = (w, h, "empty")
    if key not in _SCENES:
        model, cam = U.model_of(pkg, U.behind_camera_scene(pkg, 300, w, h, seed=11), cuda), U.camera(pkg, w, h)
        g = U.cotangents(h, w, cuda)
        host = U.host_frame(pkg, model, cam, g)
        assert host.M == 0 and host.T == 0
        _SCENES[key] = (model, cam, g, host)
    return _SCENES[key]


@pytest.mark.parametrize("keys", ["full", "window"])
@pytest.mark.parametrize("w,h,capacity,target,n_base", SUCCESS)
def test_frame_equals_host_path(pkg, cuda, w, h, capacity, target, n_base, keys):
    """A device-resident frame and its backward, with T at and around the tile
    workspace's capacity and the one-workgroup sort's edge (16384, decided by
    the capacity), equal the host path's frame: counters, tile lists (also the
    numpy statement's), ranges, rectangles, slots, every output and gradient.
    keys: 32-bit depth keys, or the window of the scene's own depth range with
    the MSD depth sort asked for."""
    RZ = pkg.rasterizer
    model, cam, cot, host = _scene(pkg, cuda, w, h, target, n_base)
    assert host.M > 0
    window = None
    if keys == "window":
        window = RZ.depth_window(host.zmin, host.zmax)
        assert window is not None and RZ.window_holds(window, host.zmin, host.zmax)
    f = U.device_frame(pkg, cuda, model, cam, capacity, window=window, msd=window is not None, backward=cot)
    U.assert_frame_matches_host(pkg, f, host, window)


@pytest.mark.parametrize("keys", ["full", "window"])
def test_frame_with_the_msd_depth_sort(pkg, cuda, keys):
    """20 000 Gaussians: above the one-workgroup depth sort's 16384, so a
    windowed frame's depth sort is gs_depth_sort_msd; T = 1.5 n in a capacity
    of 65536 (the radix tile sort, half filled)."""
    RZ = pkg.rasterizer
    model, cam, cot, host = _scene(pkg, cuda, W, H, None, 20000)
    assert 16384 < host.T < 65536
    window = None
    if keys == "window":
        window = RZ.depth_window(host.zmin, host.zmax)
        assert window is not None and 9 <= window[1] <= 31
    f = U.device_frame(pkg, cuda, model, cam, 65536, window=window, msd=window is not None, backward=cot)
    U.assert_frame_matches_host(pkg, f, host, window)


@pytest.mark.parametrize("capacity,n_base", [(16384, 8000), (16385, 8000), (256, 100)])
def test_capacity_exceeded_by_one(pkg, cuda, capacity, n_base):
    """T == capacity + 1 (the same capacities hold T == capacity in
    test_frame_equals_host_path): GS_FRAME_NEED_CAPACITY, a frame drawn with
    empty lists, nothing emitted, zero gradients, every guard intact."""
    N = pkg._native
    model, cam, cot, host = _scene(pkg, cuda, W, H, capacity + 1, n_base)
    f = U.device_frame(pkg, cuda, model, cam, capacity, backward=cot)
    assert U.frame_status(pkg, host.M, host.T, host.zmin, host.zmax, capacity, None) == (N.GS_FRAME_NEED_CAPACITY, 0)
    U.assert_failed_frame(pkg, f, [host.M, host.T, host.zmin, host.zmax, N.GS_FRAME_NEED_CAPACITY, 0],
                          _empty(pkg, cuda, W, H)[3])
    # the capacity itself holds the same scene's frame
    g = U.device_frame(pkg, cuda, model, cam, capacity + 1, backward=cot)
    U.assert_frame_matches_host(pkg, g, host)


WINDOW_BITS = (8, 9, 16, 31)


@pytest.mark.parametrize("bits", WINDOW_BITS)
def test_window_edges_three_implementations(pkg, cuda, bits):
    """Depths 3.0 + k ulp, k = 0..200, and windows of `bits` bits whose edges
    touch them: key_base = zmax - lim + 1 (the last that holds), zmax - lim
    (misses), zmin (holds), zmin + 1 (misses), lim = rasterizer._msd_limit.
    The device status (window_held in gs_bin.hip), rasterizer.window_holds
    (the definition) and the host path's gs_render_forward (window_holds in
    gs_render.hip: GS_RETRY_FULL_KEYS or not) give the same answer; frames
    that hold equal the host path's 32-bit-key frame.

    key_base is a uint32 in the ABI: with 31 bits zmax - lim is negative for
    these depths, and the two upper-edge bases are passed modulo 2^32 -- far
    above every depth, so all three must call them a miss."""
    RZ, N = pkg.rasterizer, pkg._native
    w, h, n, cap = 64, 48, 603, 1024
    key = (w, h, "ulp")
    if key not in _SCENES:
        model, cam = U.model_of(pkg, U.depth_ulp_scene(pkg, w, h, n, seed=0), cuda), U.camera(pkg, w, h)
        g = U.cotangents(h, w, cuda)
        _SCENES[key] = (model, cam, g, U.host_frame(pkg, model, cam, g))
    model, cam, cot, host = _SCENES[key]
    zmin, zmax = host.zmin, host.zmax
    z3 = int(np.float32(3.0).view(np.uint32))
    assert (host.M, host.T, zmin, zmax) == (n, n, z3, z3 + 200)
    lim = RZ._msd_limit(bits)
    assert zmax - zmin < lim
    want = {zmax - lim + 1: True, zmax - lim: False, zmin: True, zmin + 1: False}
    for base, holds in want.items():
        if base < 0:
            base, holds = base % (1 << 32), False
        window = (base, bits)
        assert RZ.window_holds(window, zmin, zmax) == holds, window
        status, t_eff = U.frame_status(pkg, n, n, zmin, zmax, cap, window)
        assert status == (0 if holds else N.GS_FRAME_WINDOW_MISS)
        f = U.device_frame(pkg, cuda, model, cam, cap, window=window, msd=bits >= 9, backward=cot)
        assert f.counters == [n, n, zmin, zmax, status, t_eff], (window, f.counters)
        st, M, T, lo, hi = U.host_forward_status(pkg, cuda, model, cam, cap, window, msd=bits >= 9)
        assert (M, T, lo, hi) == (n, n, zmin, zmax)
        assert st == (0 if holds else N.GS_RETRY_FULL_KEYS), (window, st)  # (0: GS_OK)
        if holds:
            U.assert_frame_matches_host(pkg, f, host, window)
        else:
            U.assert_failed_frame(pkg, f, [n, n, zmin, zmax, N.GS_FRAME_WINDOW_MISS, 0], _empty(pkg, cuda, w, h)[3])


@pytest.mark.parametrize("scene", ["behind", "off_screen"])
def test_empty_frame(pkg, cuda, scene):
    """M == 0 with n > 0 -- every Gaussian behind the camera, or in front of
    it and off the screen: GS_FRAME_EMPTY, M == T == 0, the depth range
    0xFFFFFFFF / 0, and the image of the host path's empty frame."""
    N = pkg._native
    make = U.behind_camera_scene if scene == "behind" else U.off_screen_scene
    model, cam = U.model_of(pkg, make(pkg, 700, W, H, seed=12), cuda), U.camera(pkg, W, H)
    cot = U.cotangents(H, W, cuda)
    assert U.frame_status(pkg, 0, 0, 0xFFFFFFFF, 0, 4096, None) == (N.GS_FRAME_EMPTY, 0)
    host = U.host_frame(pkg, model, cam, cot)
    assert (host.M, host.T) == (0, 0)
    empty = _empty(pkg, cuda, W, H)[3]
    for name in ("image", "alpha", "depth"):
        assert torch.equal(getattr(host, name), getattr(empty, name))
    for window in (None, (0x40000000, 24)):
        f = U.device_frame(pkg, cuda, model, cam, 4096, window=window, msd=window is not None, backward=cot)
        U.assert_failed_frame(pkg, f, [0, 0, 0xFFFFFFFF, 0, N.GS_FRAME_EMPTY, 0], empty)
        for name in U.GRAD_NAMES:
            assert torch.equal(f.grads[name], host.grads[name]), name


def test_two_status_bits_at_once(pkg, cuda):
    """A window the depths miss and a capacity below T: status 3."""
    N = pkg._native
    model, cam, cot, host = _scene(pkg, cuda, W, H, 4096, 1500)
    window = (host.zmin + 1, 31)
    want = N.GS_FRAME_NEED_CAPACITY | N.GS_FRAME_WINDOW_MISS
    assert want == 3 and U.frame_status(pkg, host.M, host.T, host.zmin, host.zmax, 4095, window) == (3, 0)
    f = U.device_frame(pkg, cuda, model, cam, 4095, window=window, msd=True, backward=cot)
    U.assert_failed_frame(pkg, f, [host.M, host.T, host.zmin, host.zmax, 3, 0], _empty(pkg, cuda, W, H)[3])


@pytest.mark.parametrize("kind", ["capacity", "window", "both", "empty"])
def test_failed_frame_image_is_the_empty_frames(pkg, cuda, kind):
    """A failed frame's image equals the image the host path returns for a
    frame of the same camera and background that draws nothing (the
    behind-camera scene: the background once, renderer.py:74-83).  The blend
    of a flagged frame's empty lists alone composites bg + (1 - 0) * bg, as
    the reference does for a pixel nothing covers when M > 0 (renderer.py:273,
    :359) -- (0.2, 0.4, 0.6) in every pixel at this background, where the
    empty frame is (0.1, 0.2, 0.3); k_failed_frame_pixels rewrites them."""
    N = pkg._native
    model, cam, cot, host = _scene(pkg, cuda, W, H, 4096, 1500)
    empty = _empty(pkg, cuda, W, H)
    miss = (host.zmin + 1, 31)
    capacity, window = {"capacity": (4095, None), "window": (4096, miss), "both": (4095, miss),
                        "empty": (4096, None)}[kind]
    if kind == "empty":
        model = empty[0]
    f = U.device_frame(pkg, cuda, model, cam, capacity, window=window, msd=window is not None)
    want = {"capacity": N.GS_FRAME_NEED_CAPACITY, "window": N.GS_FRAME_WINDOW_MISS, "both": 3,
            "empty": N.GS_FRAME_EMPTY}[kind]
    assert f.status == want
    diffs = U.failed_frame_image_differences(f, empty[3])
    assert not diffs, f"channel, device values, host values, differing pixels: {diffs}"
    for name in ("alpha", "depth"):
        assert torch.equal(getattr(f, name), getattr(empty[3], name)), name


def test_sticky_words_across_frames(pkg, cuda):
    """Four frames over one (step_flags, frame_seq) pair and one pinned
    buffer -- ok, capacity failure, ok, window miss: the frame counter and
    pinned [4] count the frames, [5] is each frame's status, [6] and
    *step_flags the OR of all so far, [7] the first failure's sequence word
    (never overwritten by a later failure); a frame behind a failure is
    flagged sticky but drawn correctly."""
    RZ, N = pkg.rasterizer, pkg._native
    model, cam, cot, host = _scene(pkg, cuda, W, H, 4096, 1500)
    hc = RZ._HostCounters()
    assert hc.dptr is not None, "GraphedStep needs pinned counters the device can address; so does this test"
    hc.t.zero_()
    words = torch.zeros((64,), dtype=torch.int32, device=cuda)
    CAP, MISS = N.GS_FRAME_NEED_CAPACITY, N.GS_FRAME_WINDOW_MISS
    frames = [(4096, None, 0), (4095, None, CAP), (4096, None, 0), (4096, (host.zmin + 1, 31), MISS)]
    sticky = 0
    for k, (cap, window, status) in enumerate(frames, start=1):
        f = U.device_frame(pkg, cuda, model, cam, cap, window=window, msd=window is not None, words=words, hc=hc,
                           backward=cot)
        sticky |= status
        assert f.status == status, (k, f.counters)
        assert words[:2].tolist() == [sticky, k], (k, words[:2].tolist())
        assert not words[2:].any()
        p = f.pinned
        assert p[:4] == [host.M, host.T, host.zmin, host.zmax]
        assert (p[4], p[5], p[6]) == (k, status, sticky), (k, p)
        assert p[7] == (2 if k >= 2 else 0), (k, p)
        if status == 0:
            U.assert_frame_matches_host(pkg, f, host, window)
        else:
            U.assert_failed_frame(pkg, f, [host.M, host.T, host.zmin, host.zmax, status, 0],
                                  _empty(pkg, cuda, W, H)[3])


def test_pinned_words_without_device_words(pkg, cuda):
    """No step_flags and no frame_seq: the pinned sequence word is the
    frame's host_seq, [6] the frame's own status and [7] its host_seq when it
    failed."""
    RZ, N = pkg.rasterizer, pkg._native
    model, cam, cot, host = _scene(pkg, cuda, W, H, 4096, 1500)
    hc = RZ._HostCounters()
    assert hc.dptr is not None
    hc.t.zero_()
    f = U.device_frame(pkg, cuda, model, cam, 4096, hc=hc)
    assert f.pinned[4:8] == [f.host_seq, 0, 0, 0] and f.host_seq == 1
    f = U.device_frame(pkg, cuda, model, cam, 4095, hc=hc)
    assert f.pinned[4:8] == [2, N.GS_FRAME_NEED_CAPACITY, N.GS_FRAME_NEED_CAPACITY, 2] and f.host_seq == 2
    f = U.device_frame(pkg, cuda, model, cam, 4096, hc=hc)
    assert f.pinned[4:8] == [3, 0, 0, 2]
