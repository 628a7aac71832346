"""The screen-space low-pass filter (gs_screen_filter), the parts that need no
GPU: the struct layout against the compiled header, the argument checks (they
return before any HIP call), the Python settings, and the yardsticks of
tests/screen_filter_util.py checked against each other and the pinned oracle."""
import ctypes as C
import math  # noqa: F401
import os
import subprocess

import numpy as np
import pytest
import torch

import golden_io as G
import project_reference as PR
import screen_filter_util as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gs_screen_filter), '
                   'offsetof(gs_screen_filter, variance), offsetof(gs_screen_filter, compensate), '
                   'offsetof(gs_project_args, filter), sizeof(gs_project_args), '
                   'offsetof(gs_project_bwd_args, filter), sizeof(gs_project_bwd_args), '
                   'offsetof(gs_project_pose_args, bwd) + offsetof(gs_project_bwd_args, filter), '
                   'offsetof(gs_render_fwd_args, filter), sizeof(gs_render_fwd_args), '
                   'offsetof(gs_render_bwd_args, filter), sizeof(gs_render_bwd_args));}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    F, P, B, Po, RF, RB = (N.GsScreenFilter, N.GsProjectArgs, N.GsProjectBwdArgs, N.GsProjectPoseArgs,
                           N.GsRenderFwdArgs, N.GsRenderBwdArgs)
    assert sizes == [C.sizeof(F), F.variance.offset, F.compensate.offset, P.filter.offset, C.sizeof(P),
                     B.filter.offset, C.sizeof(B), Po.bwd.offset + B.filter.offset, RF.filter.offset, C.sizeof(RF),
                     RB.filter.offset, C.sizeof(RB)]
    assert C.sizeof(F) == 8
    # the last field of each argument struct
    for S in (P, B, RF, RB):
        assert S._fields_[-1][0] == "filter" and S.filter.offset + C.sizeof(F) <= C.sizeof(S) < S.filter.offset + 16
    assert N.load().gs_abi_version() == 23 == N.GS_ABI_VERSION


@pytest.mark.parametrize("variance", [-0.3, -1e-30, float("nan"), float("inf"), -float("inf")])
def test_bad_variance_is_refused_before_any_hip_call(pkg, variance):
    """n > 0 with NULL buffers: an entry point that went past the filter check
    would report those (or launch); each names the filter instead."""
    N = pkg._native
    lib = N.load()
    f = N.GsScreenFilter(variance, 1)
    pa = N.GsProjectArgs()
    pa.g.n, pa.key_bits, pa.filter = 4, 32, f
    pa.cam.image_width = pa.cam.image_height = 32
    pa.cam.tile_size, pa.cam.radius_max = 16, 50.0
    pb = N.GsProjectBwdArgs()
    pb.g.n, pb.filter = 4, f
    ra = N.GsRenderFwdArgs()
    ra.g.n, ra.filter = 4, f
    ra.cam.image_width = ra.cam.image_height = 32
    ra.cam.tile_size = 16
    rb = N.GsRenderBwdArgs()
    rb.g.n, rb.filter = 4, f
    po = N.GsProjectPoseArgs()
    po.bwd.g.n, po.bwd.filter = 4, f
    ad = N.GsAdamArgs()
    calls = [("gs_project_forward", lambda: lib.gs_project_forward(C.byref(pa), None)),
             ("gs_project_backward", lambda: lib.gs_project_backward(C.byref(pb), None)),
             ("gs_render_forward", lambda: lib.gs_render_forward(C.byref(ra), None)),
             ("gs_render_backward", lambda: lib.gs_render_backward(C.byref(rb), None)),
             ("gs_project_backward_pose", lambda: lib.gs_project_backward_pose(C.byref(po), None)),
             ("gs_project_backward_adam", lambda: lib.gs_project_backward_adam(C.byref(pb), C.byref(ad), None))]
    for name, call in calls:
        assert call() == 1, name  # GS_ERR_INVALID_ARG
        msg = lib.gs_last_error()
        assert name.encode() in msg and b"filter.variance" in msg, (name, msg)


def test_zero_filter_passes_the_check(pkg):
    """variance 0 (with or without the flag) is no error of the filter's: the
    calls go on to their other checks (n == 0: GS_OK, nothing launched)."""
    N = pkg._native
    lib = N.load()
    for comp in (0, 1):
        pb = N.GsProjectBwdArgs()
        pb.filter = N.GsScreenFilter(0.0, comp)
        assert lib.gs_project_backward(C.byref(pb), None) == 0
        pa = N.GsProjectArgs()
        pa.key_bits, pa.filter = 32, N.GsScreenFilter(0.0, comp)
        pa.cam.image_width = pa.cam.image_height = 32
        pa.cam.tile_size, pa.cam.radius_max = 16, 50.0
        assert lib.gs_project_forward(C.byref(pa), None) == 0


def test_python_settings(pkg):
    st = pkg.RenderSettings(8, 8, torch.zeros(3))
    assert st.screen_filter == 0.0 and st.filter_compensate is True
    cfg = pkg.TrainingConfig()
    assert cfg.screen_filter == 0.0 and cfg.filter_compensate is True
    cfg.check()
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="screen_filter"):
            pkg.RenderSettings(8, 8, torch.zeros(3), screen_filter=bad)
        with pytest.raises(ValueError, match="screen_filter"):
            pkg.TrainingConfig(screen_filter=bad).check()
        st = pkg.RenderSettings(8, 8, torch.zeros(3))
        st.screen_filter = bad  # (set after construction: caught where the host scalars are made)

        class _Cam:
            _width, _height, _FoVx, _FoVy = 8, 8, 1.0, 1.0
            world_view_transform = torch.eye(4)
        with pytest.raises(ValueError, match="screen_filter"):
            pkg.camera_params(_Cam(), st)
    RZ = pkg.rasterizer
    base = (64, 48, 50.0, 50.0, 32.0, 24.0, tuple(range(12)), (0.0, 0.5, 1.0))
    off = RZ.CameraParams(*base)
    assert off.screen_filter == 0.0 and off.filter_compensate is True
    fs = off.filter_struct()
    assert (fs.variance, fs.compensate) == (0.0, 0)
    on = RZ.CameraParams(*base, screen_filter=0.3)
    plain = RZ.CameraParams(*base, screen_filter=0.3, filter_compensate=False)
    assert (on.filter_struct().variance, on.filter_struct().compensate) == (np.float32(0.3), 1)
    assert (plain.filter_struct().variance, plain.filter_struct().compensate) == (np.float32(0.3), 0)
    # carried from the settings, and a part of the struct cache's key
    st = pkg.RenderSettings(48, 64, torch.zeros(3), screen_filter=0.1, filter_compensate=False)
    cp = pkg.camera_params(_Cam(), st)
    assert (cp.screen_filter, cp.filter_compensate) == (0.1, False)
    off.to_struct(), on.to_struct(), plain.to_struct()
    tail = lambda c: (c.screen_filter, c.filter_compensate)
    keys = [k for k in RZ._CAM_STRUCTS if k[:8] == base]
    assert {k[-2:] for k in keys} >= {tail(off), tail(on), tail(plain)}
    # a trainer's settings carry its config's filter
    tr = pkg.GaussianTrainer(pkg.TrainingConfig(screen_filter=0.3, filter_compensate=False))
    s = tr._settings(_Cam())
    assert (s.screen_filter, s.filter_compensate) == (0.3, False)


# ------------------------------------------------- the yardsticks themselves ----
def _statement_camera(f):
    return PR.make_camera(int(f["width"]), int(f["height"]), float(f["fovx"]), float(f["fovy"]), f["wv"],
                          cam_width=int(f["cam_width"]), cam_height=int(f["cam_height"]))


def test_composite_gradients_equal_filtered_statement():
    """map -> unfiltered projection against the filtered projection, fp64
    autograd of one random scalar: 1e-6 of each gradient's scale."""
    f = G.load("posed_camera")
    s = 0.3
    cam = _statement_camera(f)
    scene = G.scene_of(f)
    n = f["xyz"].shape[0]
    rng = np.random.default_rng(5)
    acc = torch.tensor(rng.uniform(-1, 1, (n, 10)))
    t32 = lambda a, shape: torch.tensor(np.asarray(a, np.float32).reshape(shape))
    inputs = dict(xyz=t32(f["xyz"], (n, 3)), cov3d=t32(f["cov3d"], (n, 3, 3)), color_logits=t32(f["color_logits"], (n, 3)),
                  opacity=t32(f["opacity"], (n,)))
    ref = SF.backward(cam, inputs, s, True, acc)
    xyz, cov3d, opacity = SF._leaves(scene)
    fx, fy = SF.intrinsics(scene)
    assert (fx, fy) == (cam.fx, cam.fy)
    cov_eq, op_eq, ratio = SF.equivalent_map(xyz, cov3d, opacity, scene.wv, fx, fy, s, True)
    assert float(ratio.detach().min()) > SF.RHO_FLOOR * 1.001  # (no row on the floor: the map's gradient is the smooth one)
    out = PR.project(cam, xyz, inputs["color_logits"].double(), op_eq, cov3d=cov_eq)
    gx, gc, go = torch.autograd.grad(PR.blend_scalar(out, acc).sum(), [xyz, cov3d, opacity])
    for name, got in (("xyz", gx), ("cov3d", gc), ("opacity", go)):
        scale = float(ref[name].abs().max())
        err = float((got - ref[name]).abs().max())
        print(f"  {name}: {err / scale:.3g} of scale {scale:.3g}")
        assert scale > 0 and err <= 1e-6 * scale, (name, err / scale)


@pytest.mark.parametrize("name", ["posed_camera", "random_bg", "model_random"])
@pytest.mark.parametrize("s", [0.1, 0.3])
def test_oracle_cov2d_of_equivalent_scene(name, s):
    """The oracle's fp32 cov2d for the equivalent scene against V = V0 + s I of
    the fp64 statement: 1e-6 relative (row-wise, of the row's largest entry)."""
    f = G.load(name)
    scene = G.scene_of(f)
    eq, _ = SF.equivalent_scene(scene, s, True)
    o = G.oracle().render_forward(eq)
    n = f["xyz"].shape[0]
    t32 = lambda a, shape: torch.tensor(np.asarray(a, np.float32).reshape(shape))
    inputs = dict(xyz=t32(f["xyz"], (n, 3)), cov3d=t32(f["cov3d"], (n, 3, 3)), color_logits=t32(f["color_logits"], (n, 3)),
                  opacity=t32(f["opacity"], (n,)))
    ref = SF.forward(_statement_camera(f), inputs, s, True)
    V = ref["cov2d"].numpy()
    rel = np.abs(o["cov2d"].astype(np.float64) - V).reshape(n, -1).max(1) / np.abs(V).reshape(n, -1).max(1)
    print(f"  {name} s={s}: cov2d max rel {rel.max():.3g}")
    assert rel.max() <= 1e-6
    # and the compensated opacity is the statement's, rounded once
    assert np.abs(eq.opacity.astype(np.float64) - ref["opacity"].numpy()).max() <= 1e-7


def test_multiscale_table_with_the_oracle():
    """Rendered at 1/4 and 1/8 resolution, the compensated filter's image is at
    most half as far (RMSE) from the box-averaged full-resolution render as the
    unfiltered one."""
    o = G.oracle()
    for name in ("random_bg", "zero_bg_random"):
        scene = G.scene_of(G.load(name))
        full = o.render_forward(scene)["image"]
        for k in (4, 8):
            low = SF.downscaled(scene, k)
            ref = SF.box_average(full, k)
            off = SF.rmse(o.render_forward(low)["image"], ref)
            comp = SF.rmse(o.render_forward(SF.equivalent_scene(low, 0.3, True)[0])["image"], ref)
            plain = SF.rmse(o.render_forward(SF.equivalent_scene(low, 0.3, False)[0])["image"], ref)
            print(f"  {name} /{k}: off {off:.4f}  +0.3 {plain:.4f}  +0.3 compensated {comp:.4f}  ratio {comp / off:.2f}")
            assert comp <= 0.5 * off, (name, k, comp, off)
