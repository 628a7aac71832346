"""Helpers of tests/test_contrib_gpu.py: one render of a fixture with the
identity feature matrix (so that the oracle-verified feature image is the
weight image Wt[g, p] = c_g(p)), contribution statistics and the dominant
maps; the fp32 summation bound; the hidden-Gaussian scene; and the child
process of the cell-batch / no-bitmap test (the budgets are read at import)."""
import os
import sys

import numpy as np
import torch

import golden_io as G
from features_util import camera_of, gaussians_of, settings_of

U24 = 2.0 ** -24


def tile_of(f):
    return int(f["tile"]) if "tile" in f else 16


def stats_arrays(st):
    return dict(weight_sum=st.weight_sum.cpu().numpy().copy(), weight_max=st.weight_max.cpu().numpy().copy(),
                pixels=st.pixels.cpu().numpy().copy(), views=st.views.cpu().numpy().copy())


def prefilled(pkg, n, dev):
    """A ContributionStats with recognisable non-zero contents in every row."""
    st = pkg.ContributionStats(n, dev)
    st.weight_sum.copy_(torch.arange(n, dtype=torch.float32) * 0.25 + 3.0)
    st.weight_max.copy_(torch.full((n,), 2.0 ** -20))
    st.pixels.copy_(torch.arange(n, dtype=torch.int64) + (1 << 33))
    st.views.copy_(torch.arange(n, dtype=torch.int32) + 5)
    return st


def identity_case(pkg, dev, f, stats=None, camera=None, model=None):
    """One render with features = eye(N), `stats` (default: fresh zeros) and
    dominant=True.  Returns numpy: Wt [N, H*W], the statistics, the maps, vis,
    alpha."""
    n = f["xyz"].shape[0]
    model = gaussians_of(pkg, dev, f)[0] if model is None else model
    st = pkg.ContributionStats(n, dev) if stats is None else stats
    with torch.no_grad():
        out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(
            camera or camera_of(f), model, settings_of(pkg, f), features=torch.eye(n, device=dev),
            contribution_stats=st, dominant=True)
    torch.cuda.synchronize()
    H, W = int(f["height"]), int(f["width"])
    res = stats_arrays(st)
    res.update(Wt=out["features"].cpu().numpy().reshape(n, H * W),
               dom_id=out["dominant_gaussian"].cpu().numpy().reshape(H * W),
               dom_w=out["dominant_weight"].cpu().numpy().reshape(H * W),
               vis=out["visibility_filter"].cpu().numpy().astype(bool), alpha=out["alpha"].cpu().numpy(), H=H, W=W)
    assert out["dominant_gaussian"].dtype == torch.int32 and out["dominant_weight"].dtype == torch.float32
    assert tuple(out["dominant_gaussian"].shape) == (H, W) == tuple(out["dominant_weight"].shape)
    return res


def sum_chain(Wt, H, W, tile):
    """Per Gaussian, the longest chain of fp32 additions a term of its
    weight_sum can pass through: 6 tree levels inside a cell, one addition per
    (slot, cell) partial of the Gaussian, and the one onto the running value.
    The slots are counted from below, as the tiles the Gaussian contributes to
    (its rectangle holds at least those): a smaller chain, a tighter bound."""
    n = Wt.shape[0]
    img = Wt.reshape(n, H, W) > 0
    tx, ty = -(-W // tile), -(-H // tile)
    pad = np.zeros((n, ty * tile, tx * tile), bool)
    pad[:, :H, :W] = img
    tiles = pad.reshape(n, ty, tile, tx, tile).any(axis=(2, 4)).sum(axis=(1, 2))
    cells = (-(-tile // 8)) ** 2
    return 6 + cells * tiles + 1


def check_sum(got, Wt, H, W, tile, what):
    """weight_sum against the fp64 sum of Wt: every term is >= 0, so the
    relative error of the fp32 sum is at most chain x 2^-24; twice that."""
    exact = Wt.astype(np.float64).sum(axis=1)
    bound = 2.0 * sum_chain(Wt, H, W, tile) * U24 * exact
    err = np.abs(got.astype(np.float64) - exact)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if len(exact) else 0.0
    print(f"  {what}: weight_sum max err / bound = {worst:.3g}")
    assert (err <= bound).all(), f"{what}: weight_sum off by up to {worst:.3g} x its bound"


def check_against_weights(r, prefill=None, what=""):
    """Everything test 6 asserts of one identity_case result.  prefill: the
    statistics' contents before the render (numpy dict), or None for zeros."""
    Wt, vis = r["Wt"], r["vis"]
    n = Wt.shape[0]
    zero = dict(weight_sum=np.zeros(n, np.float32), weight_max=np.zeros(n, np.float32),
                pixels=np.zeros(n, np.int64), views=np.zeros(n, np.int32))
    pre = zero if prefill is None else prefill
    wmax = Wt.max(axis=1) if Wt.shape[1] else np.zeros(n, np.float32)
    assert r["weight_max"].dtype == np.float32 and r["pixels"].dtype == np.int64 and r["views"].dtype == np.int32
    if prefill is None:
        assert np.array_equal(r["weight_max"].view(np.uint32), wmax.view(np.uint32)), f"{what}: weight_max"
        assert np.array_equal(r["pixels"], (Wt > 0).sum(axis=1)), f"{what}: pixels"
        assert np.array_equal(r["views"], vis.astype(np.int32)), f"{what}: views"
    else:
        seen = vis
        assert np.array_equal(r["weight_max"][seen], np.maximum(pre["weight_max"], wmax)[seen])
        assert np.array_equal(r["pixels"][seen], (pre["pixels"] + (Wt > 0).sum(axis=1))[seen])
        assert np.array_equal(r["views"][seen], (pre["views"] + 1)[seen])
    for k in ("weight_sum", "weight_max", "pixels", "views"):  # culled rows: their bits as they were
        assert np.array_equal(r[k][~vis].view(np.uint8), pre[k][~vis].view(np.uint8)), f"{what}: {k} of culled rows"
    dmax = Wt.max(axis=0) if n else np.zeros(Wt.shape[1], np.float32)
    assert np.array_equal(r["dom_w"].view(np.uint32), dmax.view(np.uint32)), f"{what}: dominant_weight"
    assert np.array_equal(r["dom_id"] == -1, dmax == 0), f"{what}: dominant id -1 where nothing contributes"
    hit = r["dom_id"] >= 0
    assert (r["dom_id"][hit] < n).all()
    assert np.array_equal(Wt[r["dom_id"][hit], np.nonzero(hit)[0]], r["dom_w"][hit]), f"{what}: dominant id"


def hidden_scene(tile):
    """Two coaxial opaque walls, one small front Gaussian and two small ones
    hidden behind the walls (ISSUE 11), as a fixture-like dict (cov3d stub,
    64x64, identity view, 60 degree FoV)."""
    xyz = np.array([[0, 0, 4.0], [0, 0, 4.5], [0.3, 0.2, 3.0], [0, 0, 6.0], [0.05, -0.03, 7.0]], np.float32)
    sig = np.array([1.44, 1.44, 0.1, 0.05, 0.04], np.float32)
    cov = np.stack([np.eye(3, dtype=np.float32) * s * s for s in sig])
    op = np.array([1.0, 1.0, 0.7, 0.9, 0.8], np.float32)
    logits = np.array([[0.5, -0.2, 0.1], [-0.4, 0.3, 0.9], [1.0, 1.0, -1.0], [2.0, -2.0, 0.0], [-1.5, 0.7, 0.2]],
                      np.float32)
    fov = float(np.radians(60.0))
    return dict(xyz=xyz, cov3d=cov, opacity=op, color_logits=logits, width=64, height=64, cam_width=64,
                cam_height=64, fovx=fov, fovy=fov, wv=np.eye(4, dtype=np.float32), bg=np.zeros(3, np.float32),
                tile=tile)


def trainer_config(pkg, out, **kw):
    """Twelve iterations on the small synthetic scene, no densification."""
    base = dict(iterations=12, densify_from_iter=10 ** 6, densify_until_iter=10 ** 6, num_random_points=3000,
                log_interval=1, output_path=str(out), position_lr_init=1.6e-3, position_lr_final=1.6e-5)
    base.update(kw)
    return pkg.TrainingConfig(**base)


def _child(mode, path):
    """tile32 under the budgets of this process's environment: the identity
    case twice (asserted bitwise equal), the batch size it ran with, saved."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    f = G.load("tile32")
    r1, r2 = (identity_case(pkg, dev, f) for _ in range(2))
    keys = ("weight_sum", "weight_max", "pixels", "views", "dom_id", "dom_w", "Wt")
    same = all(np.array_equal(r1[k], r2[k]) for k in keys)
    R = pkg.rasterizer
    T = int(R._T_SEEN[dev])
    cells = R.CameraParams(1, 1, 1, 1, 0, 0, (0,) * 12, (0, 0, 0), tile_size=tile_of(f)).cells
    batch = R.contribution_cell_batch(cells, T)
    if mode == "batches":
        assert 1 <= batch < 16, batch
    else:
        assert R.live_bitmap_bytes(pkg._native.load(), cells, T, 1) == 0, "the bitmap is over its budget"
    np.savez(path, same=same, batch=batch, T=T, **{k: r1[k] for k in keys})


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child(sys.argv[1], sys.argv[2])
