"""Bilateral-grid appearance compensation (gs_bilagrid_slice_*, gs_bilagrid_tv;
bilagrid.py), the parts that need no GPU: the struct layouts against the
compiled header, the exports, the argument checks (they return before any HIP
call), the fp64 statements of tests/bilagrid_util.py checked against torch's
grid_sample with autograd and against central differences, the TrainingConfig
fields and the Python refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import bilagrid_util as BU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_bilagrid_slice_forward", "gs_bilagrid_slice_backward", "gs_bilagrid_tv")
T = lambda a: torch.as_tensor(np.asarray(a, np.float64))


def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    structs = (("gs_bilagrid_slice_args", N.GsBilagridSliceArgs), ("gs_bilagrid_tv_args", N.GsBilagridTvArgs))
    src = tmp_path / "sz.c"
    body = "".join(f'printf(" %zu", sizeof({c}));' + "".join(f'printf(" %zu", offsetof({c}, {n}));' for n, _ in S._fields_)
                   for c, S in structs)
    body += 'printf(" %d %d %d", GS_BILAGRID_CHANNELS, GS_BILAGRID_MAX_L, GS_BILAGRID_MAX_XY);'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){' + body + "}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = []
    for _, S in structs:
        want += [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert sizes == want + [N.GS_BILAGRID_CHANNELS, N.GS_BILAGRID_MAX_L, N.GS_BILAGRID_MAX_XY]
    assert N.load().gs_abi_version() == 23 == N.GS_ABI_VERSION
    assert all(name in N.EXPORTS and hasattr(N.load(), name) for name in NEW)
    assert pkg.slice_bilateral_grid is pkg.bilagrid.slice_bilateral_grid
    assert pkg.bilateral_grid_tv is pkg.bilagrid.bilateral_grid_tv and pkg.BilateralGrids is pkg.bilagrid.BilateralGrids


def test_stale_library_is_named_by_its_missing_exports(pkg, tmp_path, monkeypatch):
    """A library built before this feature has the same ABI number: load()
    names the three exports it lacks, and no other."""
    N = pkg._native
    old = [e for e in N.EXPORTS if e not in NEW and e not in ("gs_abi_version", "gs_last_error")]
    src = tmp_path / "old.c"
    src.write_text("int gs_abi_version(void) { return %d; }\nconst char *gs_last_error(void) { return \"\"; }\n"
                   % N.GS_ABI_VERSION + "".join(f"int {e}(void) {{ return 1; }}\n" for e in old))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.NativeLibraryError, match="out of date") as e:
        N.load(str(so))
    assert "lacks " + ", ".join(NEW) + ";" in str(e.value)


def _refused(lib, name, call):
    assert call() == 1, name  # GS_ERR_INVALID_ARG
    msg = lib.gs_last_error()
    assert name.encode() in msg, (name, msg)


def test_bad_arguments_are_refused_before_any_hip_call(pkg):
    """No device here and none needed: every call returns from its checks.  The
    non-NULL pointers are host memory no launch could read."""
    N = pkg._native
    lib = N.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    good = dict(width=8, height=6, grid_w=4, grid_h=3, grid_l=2)
    bad_shapes = (dict(grid_w=1), dict(grid_h=1), dict(grid_l=1), dict(grid_w=0), dict(grid_h=-3), dict(grid_l=0),
                  dict(grid_w=65), dict(grid_h=65), dict(grid_l=17), dict(grid_l=-2))
    for name, fields in (("gs_bilagrid_slice_forward", ("grid", "rgb", "out")),
                         ("gs_bilagrid_slice_backward", ("grid", "rgb", "g_out", "d_rgb", "d_grid"))):
        fn = getattr(lib, name)
        _refused(lib, name, lambda: fn(None, None))
        for missing in fields:
            a = N.GsBilagridSliceArgs(**good, **{k: p for k in fields if k != missing})
            _refused(lib, name, lambda: fn(C.byref(a), None))
        for bad in bad_shapes + (dict(width=0), dict(height=0), dict(width=-4), dict(height=-1), dict(height=262141)):
            a = N.GsBilagridSliceArgs(**{**good, **{k: p for k in fields}, **bad})
            _refused(lib, name, lambda: fn(C.byref(a), None))
    fn, name, fields = lib.gs_bilagrid_tv, "gs_bilagrid_tv", ("grid", "tv", "d_grid")
    good = dict(grid_w=4, grid_h=3, grid_l=2)
    _refused(lib, name, lambda: fn(None, None))
    for missing in fields:
        a = N.GsBilagridTvArgs(**good, **{k: p for k in fields if k != missing})
        _refused(lib, name, lambda: fn(C.byref(a), None))
    for bad in bad_shapes:
        a = N.GsBilagridTvArgs(**{**good, **{k: p for k in fields}, **bad})
        _refused(lib, name, lambda: fn(C.byref(a), None))


@pytest.mark.parametrize("shape", BU.SHAPES)
@pytest.mark.parametrize("W,H", [(1, 1), (3, 3), (17, 19), (33, 18)])
def test_statement_against_grid_sample(W, H, shape):
    """slice64 and slice_backward64 against torch's grid_sample in fp64 with
    autograd, to 1e-12 of scale; the cases hold pixels clamped on both sides."""
    G = BU.random_grid(shape, 7)
    rgb, g = BU.image_case(W, H, shape[2], 100 * W + H)
    gray = np.tensordot(BU.COEF, BU.f64(rgb), 1)
    if W * H >= 4:
        assert (gray < 0).any() and (gray > 1).any() and ((gray > 0) & (gray < 1)).any()
    Gt, rt = T(G).requires_grad_(True), T(rgb).requires_grad_(True)
    out = BU.slice_grid_sample(Gt, rt)
    (out * T(g)).sum().backward()
    want = out.detach().numpy()
    assert np.abs(BU.slice64(G, rgb) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    d_rgb, d_grid = BU.slice_backward64(G, rgb, g)
    assert np.abs(d_rgb - rt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(d_rgb).max())
    assert np.abs(d_grid - Gt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(d_grid).max())
    # forward only: the clamp's edges themselves
    rgb_e, _ = BU.image_case(W, H, shape[2], 100 * W + H, edges=True)
    with torch.no_grad():
        want = BU.slice_grid_sample(T(G), T(rgb_e)).numpy()
    assert np.abs(BU.slice64(G, rgb_e) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_statement_against_central_differences():
    shape, (W, H) = (5, 3, 16), (17, 19)
    G = BU.random_grid(shape, 3)
    rgb, g = BU.image_case(W, H, shape[2], 5)
    d_rgb, d_grid = BU.slice_backward64(G, rgb, g)
    loss = lambda G_, rgb_: (BU.slice64(G_, rgb_) * g).sum()
    rng = np.random.default_rng(0)
    h = 1e-6  # (KINK = 1e-4 keeps every pixel's cell fixed over the step)
    touched = np.argwhere(d_grid != 0)
    for n in touched[rng.choice(len(touched), 8, replace=False)]:
        e = np.zeros(G.shape)
        e[tuple(n)] = h
        fd = (loss(BU.f64(G) + e, rgb) - loss(BU.f64(G) - e, rgb)) / (2 * h)
        assert abs(fd - d_grid[tuple(n)]) <= 1e-7 * max(1.0, np.abs(d_grid).max()), n
    gray = np.tensordot(BU.COEF, BU.f64(rgb), 1)
    picks = [np.argwhere(gray < 0)[0], np.argwhere(gray > 1)[0]] + list(np.argwhere((gray > 0) & (gray < 1))[:6])
    for y, x in picks:
        for k in range(3):
            e = np.zeros(rgb.shape)
            e[k, y, x] = h
            fd = (loss(G, BU.f64(rgb) + e) - loss(G, BU.f64(rgb) - e)) / (2 * h)
            assert abs(fd - d_rgb[k, y, x]) <= 1e-7 * max(1.0, np.abs(d_rgb).max()), (k, y, x)


def test_known_answers_of_the_statement():
    """The identity grid returns the image exactly; untouched nodes get exact zeros."""
    rgb, g = BU.image_case(3, 3, 8, 1)
    assert np.array_equal(BU.slice64(BU.identity((16, 16, 8)), rgb), BU.f64(rgb))
    _, d_grid = BU.slice_backward64(BU.identity((16, 16, 8)), rgb, g)
    columns = (d_grid != 0).any(axis=(0, 1))
    assert 0 < columns.sum() < columns.size / 2


@pytest.mark.parametrize("shape", BU.SHAPES)
def test_tv_statement_against_autograd(shape):
    G = BU.random_grid(shape, 11)
    Gt = T(G).requires_grad_(True)
    tv = BU.tv_torch(Gt)
    tv.backward()
    want, d = BU.tv64(G)
    assert abs(want - float(tv.detach())) <= 1e-14 * float(tv.detach()) and np.abs(d - Gt.grad.numpy()).max() <= 1e-14
    tv0, d0 = BU.tv64(np.full_like(G, 0.7))
    assert tv0 == 0 and (d0 == 0).all()


def test_training_config(pkg):
    cfg = pkg.TrainingConfig()
    assert (cfg.bilateral_grid, cfg.bilateral_grid_shape, cfg.bilateral_grid_lr, cfg.bilateral_grid_warmup,
            cfg.lambda_tv) == (False, (16, 16, 8), 2e-3, 1000, 10.0)
    cfg.check()
    pkg.TrainingConfig(bilateral_grid=True, bilateral_grid_shape=[5, 3, 16], bilateral_grid_lr=1e-2,
                       bilateral_grid_warmup=0, lambda_tv=0.0).check()
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="bilateral_grid "):
            pkg.TrainingConfig(bilateral_grid=bad).check()
    for bad in ((16, 16), (1, 16, 8), (16, 1, 8), (16, 16, 1), (65, 16, 8), (16, 65, 8), (16, 16, 17), (16.0, 16, 8),
                (True, 16, 8), "16x16x8", None):
        with pytest.raises(ValueError, match="bilateral_grid_shape"):
            pkg.TrainingConfig(bilateral_grid_shape=bad).check()
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bilateral_grid_lr"):
            pkg.TrainingConfig(bilateral_grid_lr=bad).check()
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="bilateral_grid_warmup"):
            pkg.TrainingConfig(bilateral_grid_warmup=bad).check()
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_tv"):
            pkg.TrainingConfig(lambda_tv=bad).check()


def test_python_refusals(pkg):
    """ValueError before anything is launched (there is no device here to launch on)."""
    G, img = torch.zeros(12, 8, 16, 16), torch.zeros(3, 8, 8)
    for args, what in (((G[:11], img), "grid must be"), ((G[0], img), "grid must be"), ((G.double(), img), "fp32"),
                       ((G[:, :1], img), "shape"), ((torch.zeros(12, 17, 4, 4), img), "shape"),
                       ((torch.zeros(12, 4, 65, 4), img), "shape"), ((G, img[:2]), "image must be"),
                       ((G, img[0]), "image must be"), ((G, img.double()), "fp32"), ((G, torch.zeros(3, 0, 8)), "1x1"),
                       ((G, img.to("meta")), "image is on")):
        with pytest.raises(ValueError, match=what):
            pkg.slice_bilateral_grid(*args)
    for bad, what in ((G[:11], "grid must be"), (G.double(), "fp32"), (G[:, :, :1], "shape")):
        with pytest.raises(ValueError, match=what):
            pkg.bilateral_grid_tv(bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.slice_bilateral_grid(G, img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.bilateral_grid_tv(G)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_images"):
            pkg.BilateralGrids(bad, "cpu")
    for bad in ((16, 16), (1, 16, 8), (16, 16, 17)):
        with pytest.raises(ValueError, match="grid_shape"):
            pkg.BilateralGrids(2, "cpu", bad)
    grids = pkg.BilateralGrids(3, "cpu", (5, 3, 16))
    assert len(grids) == 3 and all(g.shape == (12, 16, 3, 5) and g.is_leaf and g.requires_grad for g in grids.grids)
    assert all(np.array_equal(g.detach().numpy(), BU.identity((5, 3, 16))) for g in grids.grids)
    for bad in (3, -1, 1.0, True):
        with pytest.raises(ValueError, match="grid index"):
            grids.slice(bad, torch.zeros(3, 4, 4))
        with pytest.raises(ValueError, match="grid index"):
            grids.tv(bad)
    # the state of grids no step has touched, and its round trip
    st = grids.state()
    assert st["grids"].shape == (3, 12, 16, 3, 5) and not st["m"].any() and not st["v"].any() and st["step"].tolist() == [0, 0, 0]
    grids.load_state(st)
    with pytest.raises(ValueError, match="state"):
        grids.load_state({**st, "m": st["m"][:2]})
