"""The library calls one rasterize() forward and backward makes, in order, with
the scalars that fix the summation order of the gradients: accumulate (acc),
feature_accumulate (facc), partial_groups (G), cell_begin (c0), cell_count
(cc), chunk and first_batch (first), and for the projection backward what it
reads (partials and flags, sums already gathered, or no blend gradient).

Every combination of passes and cotangents below renders the 300 Gaussians of
tests/golden/launch/scene.npz (seeded numpy: a 64 x 48 image, identity view)
at two shapes: tile 16 in one batch, where the first extra pass finds the
colour pass's partials not yet gathered, and tile 20 (9 cells) under a partial
budget of four cells, so that every pass runs in the batches 4 + 4 + 1 and
each one adds to the sums of the one before.

EXPECTED holds the recorded sequences.  They were recorded once, by running
this file as a script (it prints the dictionary) on the commit before the
replay passes' host code was folded together, and are literals since: a host
refactor that reorders, drops or re-parameterises a launch fails here even
where the result would agree to rounding.  The per-device guesses of the
forward (entry capacity, depth-key window) are cleared before each render, so
that its calls do not depend on the renders before it."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import golden_io as G

pytestmark = pytest.mark.gpu

SCALARS = (("accumulate", "acc"), ("feature_accumulate", "facc"), ("partial_groups", "G"), ("cell_begin", "c0"),
           ("cell_count", "cc"), ("chunk", "chunk"), ("first_batch", "first"))
QUERIES = ("gs_abi_version", "gs_last_error", "gs_blend_live_words", "gs_tile_quads", "gs_partial_groups",
           "gs_blend_backward_groups", "gs_frame_offsets", "gs_tile_offsets")
SHAPES = ("tile16", "tile20")
COMBOS = ("colour", "features", "distortion", "both", "abs_stats", "feature_cotangent_only",
          "distortion_cotangent_only")
BATCH_CELLS = 4  # tile 20: 9 cells in batches of 4, 4 and 1


def _describe(name, args):
    st = getattr(args[0], "_obj", None) if args else None
    vals = []
    if isinstance(st, C.Structure):
        if name == "gs_project_backward_pose":
            st = st.bwd
        if name == "gs_gather_partials":
            vals.append(f"acc={int(args[1])}")
        vals += [f"{short}={int(getattr(st, field))}" for field, short in SCALARS if hasattr(st, field)]
        if name in ("gs_project_backward", "gs_project_backward_pose"):
            vals.append("reads=" + ("partials" if st.pair_grads else "sums" if st.grad_sums else "nothing"))
    return name[3:] + ("[" + ",".join(vals) + "]" if vals else "")


def _record(monkeypatch, lib, names):
    calls = []
    for name in names:
        if name in QUERIES or name.endswith("_bytes"):
            continue
        fn = getattr(lib, name)

        def wrapper(*a, _fn=fn, _name=name):
            calls.append(_describe(_name, a))
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapper)
    return calls


def _forget_guesses(RZ):
    for d in (RZ._T_SEEN, RZ._DEPTH_HIST, RZ._WINDOW_STATE, RZ._MSD_BACKOFF):
        d.clear()


def _scene(pkg, dev, tile):
    f = np.load(os.path.join(G.GOLDEN, "launch", "scene.npz"))
    W, H = int(f["width"]), int(f["height"])
    view = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    cam = pkg.rasterizer.CameraParams(W, H, 0.5 * W / math.tan(float(f["fovx"]) * 0.5),
                                      0.5 * H / math.tan(float(f["fovy"]) * 0.5), W * 0.5, H * 0.5, view,
                                      tuple(float(v) for v in f["bg"]), tile_size=tile)
    leaf = lambda k: torch.tensor(f[k], device=dev, requires_grad=True)
    return cam, {k: leaf(k) for k in ("xyz", "cov3d", "color_logits", "opacity", "features")}


def _cotangent(shape, seed, dev):
    return torch.tensor(np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32), device=dev)


def _run(pkg, dev, monkeypatch, shape, combo):
    """The calls of one forward and one backward of `combo` at `shape`."""
    RZ, N = pkg.rasterizer, pkg._native
    cam, t = _scene(pkg, dev, 16 if shape == "tile16" else 20)
    H, W, n = cam.image_height, cam.image_width, t["xyz"].shape[0]
    kw = {}
    if combo in ("features", "both", "feature_cotangent_only"):
        kw["features"] = t["features"]
    if combo in ("distortion", "both", "distortion_cotangent_only"):
        kw["depth_distortion"] = True
    if combo == "abs_stats":
        kw["density_stats"] = pkg.DensityStats(n, dev, abs_grad=True)
    render = lambda: RZ.rasterize(cam, t["xyz"], t["cov3d"], None, None, t["color_logits"], t["opacity"], **kw)
    saved = RZ.PARTIAL_BUDGET_BYTES
    try:
        if shape == "tile20":
            assert cam.cells == 9
            _forget_guesses(RZ)
            with torch.no_grad():
                RZ.rasterize(cam, t["xyz"], t["cov3d"], None, None, t["color_logits"], t["opacity"])
            T = int(RZ._T_SEEN[dev])
            RZ.PARTIAL_BUDGET_BYTES = 41 * T * BATCH_CELLS + 1
            assert RZ.cell_batch(cam.cells, T) == BATCH_CELLS
        _forget_guesses(RZ)
        calls = _record(monkeypatch, N.load(), N.EXPORTS)
        outs = render()
        rest = list(outs[7:])
        feat = rest.pop(0) if "features" in kw else None
        dist = rest.pop(0) if "depth_distortion" in kw else None
        loss = 0.0
        if not combo.endswith("_cotangent_only"):
            loss = loss + (outs[0] * _cotangent((3, H, W), 1, dev)).sum()
        if feat is not None and combo != "distortion_cotangent_only":
            loss = loss + (feat * _cotangent((6, H, W), 2, dev)).sum()
        if dist is not None and combo != "feature_cotangent_only":
            loss = loss + (dist * _cotangent((H, W), 3, dev)).sum()
        calls.append("backward:")
        loss.backward()
        torch.cuda.synchronize()
    finally:
        RZ.PARTIAL_BUDGET_BYTES = saved
        monkeypatch.undo()
    assert t["xyz"].grad is not None and bool(t["xyz"].grad.any())
    return calls


EXPECTED = {
    ("tile16", "colour"): """
        render_forward render_forward
        backward: render_backward""",
    ("tile16", "features"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_features_forward
        backward: blend_backward[c0=0,cc=0] gather_partials[acc=0,G=4] blend_features_backward[c0=0,cc=4,chunk=0]
        gather_feature_partials[acc=1,facc=0,G=4] blend_features_backward[c0=0,cc=4,chunk=1]
        gather_feature_partials[acc=1,facc=0,G=4] project_backward[G=4,reads=sums]""",
    ("tile16", "distortion"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_distortion_forward
        backward: blend_backward[c0=0,cc=0] gather_partials[acc=0,G=4] blend_distortion_backward[c0=0,cc=4]
        gather_partials[acc=1,G=4] project_backward[G=4,reads=sums]""",
    ("tile16", "both"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_features_forward blend_distortion_forward
        backward: blend_backward[c0=0,cc=0] gather_partials[acc=0,G=4] blend_features_backward[c0=0,cc=4,chunk=0]
        gather_feature_partials[acc=1,facc=0,G=4] blend_features_backward[c0=0,cc=4,chunk=1]
        gather_feature_partials[acc=1,facc=0,G=4] blend_distortion_backward[c0=0,cc=4] gather_partials[acc=1,G=4]
        project_backward[G=4,reads=sums]""",
    ("tile16", "abs_stats"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        backward: blend_backward_abs[c0=0,cc=0] gather_abs_partials[acc=0,G=4] project_backward[G=4,reads=partials]
        density_accumulate_abs""",
    ("tile16", "feature_cotangent_only"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_features_forward
        backward: blend_features_backward[c0=0,cc=4,chunk=0] gather_feature_partials[acc=0,facc=0,G=4]
        blend_features_backward[c0=0,cc=4,chunk=1] gather_feature_partials[acc=1,facc=0,G=4]
        project_backward[G=4,reads=sums]""",
    ("tile16", "distortion_cotangent_only"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_distortion_forward
        backward: blend_distortion_backward[c0=0,cc=4] gather_partials[acc=0,G=4] project_backward[G=4,reads=sums]""",
    ("tile20", "colour"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        backward: blend_backward[c0=0,cc=4] gather_partials[acc=0,G=4] blend_backward[c0=4,cc=4]
        gather_partials[acc=1,G=4] blend_backward[c0=8,cc=1] gather_partials[acc=1,G=1]
        project_backward[G=4,reads=sums]""",
    ("tile20", "features"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_features_forward
        backward: blend_backward[c0=0,cc=4] gather_partials[acc=0,G=4] blend_backward[c0=4,cc=4]
        gather_partials[acc=1,G=4] blend_backward[c0=8,cc=1] gather_partials[acc=1,G=1]
        blend_features_backward[c0=0,cc=4,chunk=0] gather_feature_partials[acc=1,facc=0,G=4]
        blend_features_backward[c0=4,cc=4,chunk=0] gather_feature_partials[acc=1,facc=1,G=4]
        blend_features_backward[c0=8,cc=1,chunk=0] gather_feature_partials[acc=1,facc=1,G=1]
        blend_features_backward[c0=0,cc=4,chunk=1] gather_feature_partials[acc=1,facc=0,G=4]
        blend_features_backward[c0=4,cc=4,chunk=1] gather_feature_partials[acc=1,facc=1,G=4]
        blend_features_backward[c0=8,cc=1,chunk=1] gather_feature_partials[acc=1,facc=1,G=1]
        project_backward[G=4,reads=sums]""",
    ("tile20", "distortion"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_distortion_forward
        backward: blend_backward[c0=0,cc=4] gather_partials[acc=0,G=4] blend_backward[c0=4,cc=4]
        gather_partials[acc=1,G=4] blend_backward[c0=8,cc=1] gather_partials[acc=1,G=1]
        blend_distortion_backward[c0=0,cc=4] gather_partials[acc=1,G=4] blend_distortion_backward[c0=4,cc=4]
        gather_partials[acc=1,G=4] blend_distortion_backward[c0=8,cc=1] gather_partials[acc=1,G=1]
        project_backward[G=4,reads=sums]""",
    ("tile20", "both"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_features_forward blend_distortion_forward
        backward: blend_backward[c0=0,cc=4] gather_partials[acc=0,G=4] blend_backward[c0=4,cc=4]
        gather_partials[acc=1,G=4] blend_backward[c0=8,cc=1] gather_partials[acc=1,G=1]
        blend_features_backward[c0=0,cc=4,chunk=0] gather_feature_partials[acc=1,facc=0,G=4]
        blend_features_backward[c0=4,cc=4,chunk=0] gather_feature_partials[acc=1,facc=1,G=4]
        blend_features_backward[c0=8,cc=1,chunk=0] gather_feature_partials[acc=1,facc=1,G=1]
        blend_features_backward[c0=0,cc=4,chunk=1] gather_feature_partials[acc=1,facc=0,G=4]
        blend_features_backward[c0=4,cc=4,chunk=1] gather_feature_partials[acc=1,facc=1,G=4]
        blend_features_backward[c0=8,cc=1,chunk=1] gather_feature_partials[acc=1,facc=1,G=1]
        blend_distortion_backward[c0=0,cc=4] gather_partials[acc=1,G=4] blend_distortion_backward[c0=4,cc=4]
        gather_partials[acc=1,G=4] blend_distortion_backward[c0=8,cc=1] gather_partials[acc=1,G=1]
        project_backward[G=4,reads=sums]""",
    ("tile20", "abs_stats"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        backward: blend_backward_abs[c0=0,cc=4] gather_abs_partials[acc=0,G=4] gather_partials[acc=0,G=4]
        blend_backward_abs[c0=4,cc=4] gather_abs_partials[acc=1,G=4] gather_partials[acc=1,G=4]
        blend_backward_abs[c0=8,cc=1] gather_abs_partials[acc=1,G=1] gather_partials[acc=1,G=1]
        project_backward[G=4,reads=sums] density_accumulate_abs""",
    ("tile20", "feature_cotangent_only"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_features_forward
        backward: blend_features_backward[c0=0,cc=4,chunk=0] gather_feature_partials[acc=0,facc=0,G=4]
        blend_features_backward[c0=4,cc=4,chunk=0] gather_feature_partials[acc=1,facc=1,G=4]
        blend_features_backward[c0=8,cc=1,chunk=0] gather_feature_partials[acc=1,facc=1,G=1]
        blend_features_backward[c0=0,cc=4,chunk=1] gather_feature_partials[acc=1,facc=0,G=4]
        blend_features_backward[c0=4,cc=4,chunk=1] gather_feature_partials[acc=1,facc=1,G=4]
        blend_features_backward[c0=8,cc=1,chunk=1] gather_feature_partials[acc=1,facc=1,G=1]
        project_backward[G=4,reads=sums]""",
    ("tile20", "distortion_cotangent_only"): """
        project_forward radix_sort_pairs bin_count bin_emit radix_sort_pairs tile_ranges blend_forward
        blend_distortion_forward
        backward: blend_distortion_backward[c0=0,cc=4] gather_partials[acc=0,G=4]
        blend_distortion_backward[c0=4,cc=4] gather_partials[acc=1,G=4] blend_distortion_backward[c0=8,cc=1]
        gather_partials[acc=1,G=1] project_backward[G=4,reads=sums]""",
}


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("shape", SHAPES)
def test_launch_sequence(pkg, cuda, monkeypatch, shape, combo):
    calls = _run(pkg, cuda, monkeypatch, shape, combo)
    print("\n".join(calls))
    if shape == "tile20":
        begins = {c.split("c0=")[1].split(",")[0] for c in calls if c.startswith("blend_") and "c0=" in c}
        assert len(begins) >= 3, "at least three cell batches"
    assert calls == EXPECTED[shape, combo].split()


if __name__ == "__main__":  # the recorder: prints EXPECTED as a literal
    import sys
    sys.path.insert(0, G.ROOT)
    import __graft_entry__ as ge
    _pkg, _dev = ge.load_package(), torch.device("cuda:0")
    print("EXPECTED = {")
    for _shape in SHAPES:
        for _combo in COMBOS:
            _calls = _run(_pkg, _dev, pytest.MonkeyPatch(), _shape, _combo)
            print(f'    ("{_shape}", "{_combo}"): """')
            _line = "       "
            for _c in _calls:
                if len(_line) + len(_c) + 1 > 116 or _c == "backward:":
                    print(_line)
                    _line = "       "
                _line += " " + _c
            print(_line + '""",')
    print("}")
