"""Depth distortion without a GPU: the reference helper's prefix form and
gradient formulas against the brute-force double sum and torch fp64 autograd,
the ctypes mirror of the two new argument structs, and the argument checks of
the entry points, render() and TrainingConfig (all before any launch)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import distortion_util as DU
import replay_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_case(seed, n=9, P=7, near_far=None):
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, 0.7, (n, P))
    alpha[rng.uniform(size=(n, P)) < 0.25] = 0.0  # skipped pairs
    T = np.cumprod(np.vstack([np.ones((1, P)), 1 - alpha[:-1]]), 0)
    z = np.sort(rng.uniform(2.0, 9.0, n))
    return T * alpha, DU.mapped(z, near_far)


@pytest.mark.parametrize("near_far", [None, DU.NEAR_FAR])
def test_prefix_form_is_the_double_sum(near_far):
    for seed in range(5):
        c, m = _random_case(seed, near_far=near_far)
        want = DU.brute_distortion(c, m)
        got = DU.prefix_distortion(c, m)
        assert np.all(want > 0)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-15)
        # a shift common to all m changes nothing
        assert np.allclose(DU.prefix_distortion(c, m - m[0]), want, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("near_far", [None, DU.NEAR_FAR])
def test_gradient_formulas_match_autograd(near_far):
    c, m = _random_case(17, near_far=near_far)
    ct = torch.tensor(c, dtype=torch.float64, requires_grad=True)
    mt = torch.tensor(m, dtype=torch.float64, requires_grad=True)
    d = (mt[:, None] - mt[None, :]).abs()
    D = torch.einsum("ip,jp,ij->p", ct, ct, d)
    D.sum().backward()
    assert np.allclose(DU.dD_dc(c, m), ct.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert np.allclose(DU.dD_dm(c, m).sum(1), mt.grad.numpy(), rtol=1e-11, atol=1e-14)
    # the torch statement of the prefix form (the gradient reference of the GPU tests) too
    ct.grad = mt.grad = None
    DU.prefix_distortion(ct, mt, xp=torch).sum().backward()
    assert np.allclose(DU.dD_dc(c, m), ct.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert np.allclose(DU.dD_dm(c, m).sum(1), mt.grad.numpy(), rtol=1e-11, atol=1e-14)


def test_euler_and_shift_identities():
    c, m = _random_case(23)
    D = DU.prefix_distortion(c, m)
    assert np.allclose((c * DU.dD_dc(c, m)).sum(0), 2 * D, rtol=1e-12)
    assert np.abs(DU.dD_dm(c, m).sum(0)).max() <= 1e-14


def test_median_rule():
    c = np.array([[0.0, 0.2, 0.0, 0.6], [0.3, 0.0, 0.0, 0.0], [0.0, 0.3, 0.0, 0.1], [0.25, 0.1, 0.0, 0.0]], np.float32)
    row, A = DU.median_rule(c)
    # column 0: 0.3, 0.55 -> row 3; column 1: 0.2, 0.5 -> row 2; column 2: none; column 3: 0.6 at once
    assert row.tolist() == [3, 2, -1, 0]
    assert A.dtype == np.float32 and np.array_equal(A, c.sum(0, dtype=np.float32))
    row, _ = DU.median_rule(np.array([[0.1], [0.0], [0.2], [0.0]], np.float32))
    assert row.tolist() == [2]  # never reaches 0.5: the last contributor


# ---- the ABI ------------------------------------------------------------------
def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    structs = (("gs_distortion_fwd_args", N.GsDistortionFwdArgs), ("gs_distortion_bwd_args", N.GsDistortionBwdArgs))
    lines = []
    for cname, t in structs:
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname) for fname, *_ in t._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gsplat_mi355x.h"\nint main(){' +
                   "".join(lines) + "}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = []
    for _, t in structs:
        want.append(C.sizeof(t))
        want += [getattr(t, fname).offset for fname, *_ in t._fields_]
    assert got == want
    # the frame inside both structs, field by field, and the bytes the flat structs had
    replay_layout.check(pkg, tmp_path, ["gs_distortion_fwd_args", "gs_distortion_bwd_args"])
    assert "gs_blend_distortion_forward" in N.EXPORTS and "gs_blend_distortion_backward" in N.EXPORTS
    assert N.GS_ABI_VERSION == 23


def _fwd_args(N):
    a = N.GsDistortionFwdArgs()
    a.cam.image_width = a.cam.image_height = 16
    a.cam.tile_size = 16
    a.tiles_x = a.tiles_y = 1
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)
    for name in ("ranges", "sorted_gauss", "records", "cell_neval", "distortion", "moments", "median_depth",
                 "median_id"):
        setattr(a, name, p)
    a.num_pairs, a.num_gaussians = 4, 2
    return a, buf


def _bwd_args(N):
    a = N.GsDistortionBwdArgs()
    a.cam.image_width = a.cam.image_height = 16
    a.cam.tile_size = 16
    a.tiles_x = a.tiles_y = 1
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)
    for name in ("ranges", "sorted_gauss", "records", "cell_neval", "distortion", "moments", "g_distortion",
                 "pair_grads", "slot_live"):
        setattr(a, name, p)
    a.num_pairs, a.num_gaussians = 4, 2
    return a, buf


BAD_NEAR_FAR = [(0.0, 1.0), (1.0, 0.0), (-1.0, 2.0), (2.0, 2.0), (3.0, 2.0), (float("nan"), 2.0),
                (1.0, float("nan")), (1.0, float("inf")), (float("inf"), float("inf"))]


def test_entry_points_reject_bad_arguments(pkg):
    """GS_ERR_INVALID_ARG (1) before any HIP call: this runs without a GPU."""
    N = pkg._native
    lib = N.load()
    for fn, make, required in (
            (lib.gs_blend_distortion_forward, _fwd_args,
             ("ranges", "sorted_gauss", "records", "cell_neval", "distortion", "moments", "median_depth",
              "median_id")),
            (lib.gs_blend_distortion_backward, _bwd_args,
             ("ranges", "sorted_gauss", "records", "cell_neval", "distortion", "moments", "g_distortion",
              "pair_grads", "slot_live"))):
        assert fn(None, None) == 1
        assert b"gs_blend_distortion" in lib.gs_last_error()
        for name in required:
            a, buf = make(N)
            setattr(a, name, None)
            assert fn(C.byref(a), None) == 1, name
        for near, far in BAD_NEAR_FAR:
            a, buf = make(N)
            a.near, a.far = near, far
            assert fn(C.byref(a), None) == 1, (near, far)
            assert b"near" in lib.gs_last_error()
        a, buf = make(N)
        a.live_bits, a.live_words = C.addressof(buf), 0
        assert fn(C.byref(a), None) == 1
        a, buf = make(N)
        a.tiles_x = 2
        assert fn(C.byref(a), None) == 1
    a, buf = _bwd_args(N)
    a.cell_begin, a.cell_count = 3, 2  # past the default tile's four cells
    assert lib.gs_blend_distortion_backward(C.byref(a), None) == 1


# ---- host validation ----------------------------------------------------------
def test_render_refuses_bad_arguments_before_reading_anything(pkg):
    r = pkg.GaussianRenderer()
    # (camera, gaussians and settings are never touched: None would raise AttributeError)
    with pytest.raises(ValueError, match="depth_distortion"):
        r.render(None, None, None, distortion_near_far=(0.1, 100.0))
    for bad in BAD_NEAR_FAR + [(1.0,), (1.0, 2.0, 3.0), "ab", 5.0]:
        with pytest.raises(ValueError, match="distortion_near_far"):
            r.render(None, None, None, depth_distortion=True, distortion_near_far=bad)
    assert pkg.rasterizer.check_distortion_near_far(None) == (0.0, 0.0)
    assert pkg.rasterizer.check_distortion_near_far([0.5, 8]) == (0.5, 8.0)


def test_training_config_checks(pkg):
    cfg = pkg.TrainingConfig()
    assert cfg.lambda_distortion == 0.0 and cfg.distortion_from_iter == 0 and cfg.distortion_near_far is None
    cfg.check()
    pkg.TrainingConfig(lambda_distortion=100.0, distortion_from_iter=3000, distortion_near_far=[0.1, 100.0]).check()
    for kw in (dict(lambda_distortion=-1.0), dict(lambda_distortion=float("nan")),
               dict(lambda_distortion=float("inf")), dict(distortion_from_iter=-1), dict(distortion_from_iter=1.5),
               dict(distortion_near_far=(0.0, 1.0)), dict(distortion_near_far=(2.0, 1.0)),
               dict(distortion_near_far=(1.0, float("inf"))), dict(distortion_near_far=(1.0,)),
               dict(distortion_near_far=(float("nan"), 1.0)), dict(distortion_near_far=3.0)):
        with pytest.raises(ValueError):
            pkg.TrainingConfig(**kw).check()
