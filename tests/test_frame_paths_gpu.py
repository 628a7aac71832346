"""One _Frame whichever host path made it: the frame entry points' (calls)
and the stage-by-stage path's frames of the same render hold the same
buffers under the same names, and their backward -- the first and a second
one of the same frame -- gives the same gradients, bit for bit.  The scene is
the 300 Gaussians of tests/golden/launch/scene.npz (64 x 48, identity view).

Every view is compared in full but `live_bits`, which the blend defines only
on the words of each tile's 64-entry batches (gs_blend_live_words: word
start / 64 + tile + batch of each cell's row); the words between them are
whatever the allocation held."""
import math
import os

import numpy as np
import pytest
import torch

import golden_io as G

pytestmark = pytest.mark.gpu

VIEWS = ("records", "rects", "order", "pair_offset", "ranges", "pix_flags", "cell_neval", "sorted_gauss", "live_bits",
         "slot_live")


def _scene(pkg, dev, tile):
    f = np.load(os.path.join(G.GOLDEN, "launch", "scene.npz"))
    W, H = int(f["width"]), int(f["height"])
    view = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    cam = pkg.rasterizer.CameraParams(W, H, 0.5 * W / math.tan(float(f["fovx"]) * 0.5),
                                      0.5 * H / math.tan(float(f["fovy"]) * 0.5), W * 0.5, H * 0.5, view,
                                      tuple(float(v) for v in f["bg"]), tile_size=tile)
    n = f["xyz"].shape[0]
    t = {k: torch.tensor(f[k], device=dev) for k in ("xyz", "cov3d", "color_logits", "opacity")}
    raw = (t["xyz"].reshape(n, 3), t["cov3d"].reshape(n, 3, 3), None, None, t["color_logits"].reshape(n, 3),
           t["opacity"].reshape(n))
    cot = tuple(torch.tensor(np.random.default_rng(s).uniform(-1, 1, (c, H, W)).astype(np.float32), device=dev)
                for s, c in ((1, 3), (2, 1), (3, 1)))
    return cam, raw, cot


def _defined(fr, name):
    """The view `name` of a frame, cloned, with the elements no kernel defines zeroed."""
    v = getattr(fr, name)
    if v is None:
        return None
    v = v.clone()
    if name == "live_bits":
        keep = torch.zeros_like(v, dtype=torch.bool)
        for tile, (s, e) in enumerate(fr.ranges.tolist()):
            keep[:, s // 64 + tile:s // 64 + tile + (e - s + 63) // 64] = True
        v[~keep] = 0
    return v


def _render(pkg, dev, tile, calls, need_grad, backwards=2, seen=None):
    """One forward on the path `calls` names, with no guess from a frame before
    it (seen: the T of a frame before it to guess the capacity from), and
    `backwards` backwards of its frame: the outputs, the frame, its views
    after the first backward, and each backward's gradients."""
    RZ = pkg.rasterizer
    cam, raw, cot = _scene(pkg, dev, tile)
    saved = RZ._FRAME_CALLS
    try:
        RZ._FRAME_CALLS = calls
        for d in (RZ._T_SEEN, RZ._DEPTH_HIST, RZ._WINDOW_STATE, RZ._MSD_BACKOFF):
            d.clear()
        if seen is not None:
            RZ._T_SEEN[dev] = seen
        with torch.no_grad():
            *outs, fr = RZ.forward_pipeline(cam, *raw, need_grad=need_grad)
    finally:
        RZ._FRAME_CALLS = saved
    assert fr.calls is calls and fr.flags_zeroed is need_grad
    grads, views = [], None
    for _ in range(backwards):
        d = RZ.backward_pipeline(cam, fr, *raw, outs[3], outs[4], cot[0], cot[1], cot[2], None, None,
                                 outputs=tuple(outs[:3]))
        assert fr.flags_zeroed is False
        grads.append([g.clone() for g in d if g is not None])
        if views is None:
            views = {name: _defined(fr, name) for name in VIEWS}
    torch.cuda.synchronize()
    return outs, fr, views, grads


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("seen", (None, 1000))
@pytest.mark.parametrize("need_grad", (True, False))
def test_both_paths_make_the_same_frame(pkg, cuda, need_grad, seen):
    """Tile 16: the call path's and the stage path's frame of one render --
    every named view (slot_live after the backward), M, T, groups, the
    outputs and all gradients equal; and on each path a second backward of
    the frame (retain_graph) repeats the first one's gradients.  seen: no
    capacity guess (the tile workspace is made for T after the read-back), and
    one that holds (the emission queued before the read-back into a workspace
    for more than T entries: the flags' offset and the bitmap's stride come
    from the capacity).  No guess is too small for this scene's T (a guess is
    at least 4097 entries): that branch is test_emit_capacity_guess's."""
    stage = _render(pkg, cuda, 16, False, need_grad, seen=seen)
    call = _render(pkg, cuda, 16, True, need_grad, seen=seen)
    (so, sf, sv, sg), (co, cf, cv, cg) = stage, call
    assert sf.M > 0 and (sf.M, sf.T, sf.groups, sf.n) == (cf.M, cf.T, cf.groups, cf.n)
    assert sf.fb.capacity == (sf.T if seen is None else seen + seen // 4 + 4096) and sf.fb.capacity >= sf.T
    # (depth_alt may differ: the one-launch sort of a small frame leaves the ids in the other half)
    assert (sf.fb.capacity, sf.fb.live_cells, sf.fb.flag_groups) == (cf.fb.capacity, cf.fb.live_cells, cf.fb.flag_groups)
    _same(so, co)
    for name in VIEWS:
        assert sv[name] is not None and torch.equal(sv[name], cv[name]), name
    assert sv["slot_live"].numel() == sf.T * sf.groups and int(sv["slot_live"].count_nonzero()) > 0
    assert int(sv["live_bits"].count_nonzero()) > 0
    _same(sg[0], cg[0])
    _same(sg[1], sg[0])
    _same(cg[1], cg[0])


def test_frame_without_liveness_bitmap(pkg, cuda):
    """Tile 20 (9 cells) with the bitmap over its budget: the frame has no
    live_bits, and its outputs and gradients are the bitmap run's."""
    RZ = pkg.rasterizer
    outs, fr, views, grads = _render(pkg, cuda, 20, False, True)
    assert fr.live_bits is not None and fr.fb.live_cells == 9 and not fr.calls
    saved = RZ.LIVE_BUDGET_BYTES
    try:
        RZ.LIVE_BUDGET_BYTES = 1
        outs0, fr0, views0, grads0 = _render(pkg, cuda, 20, False, True)
    finally:
        RZ.LIVE_BUDGET_BYTES = saved
    assert fr0.live_bits is None and fr0.fb.live_cells == 0 and views0["live_bits"] is None
    assert (fr0.M, fr0.T, fr0.groups) == (fr.M, fr.T, fr.groups) and fr.M > 0
    _same(outs0, outs)
    _same(grads0[0], grads[0])
    _same(grads0[1], grads0[0])
    _same(grads[1], grads[0])
