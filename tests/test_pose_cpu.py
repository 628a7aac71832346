"""Camera-pose gradients, the parts that need no GPU: se3_exp against
torch.linalg.matrix_exp and gradcheck, the package exports, the C ABI of
gs_project_backward_pose (struct size, argument errors: these return before
any HIP call), and the pose fixtures' recorded reference deviation."""
import ctypes as C
import json
import math
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_GOLDEN = os.path.join(ROOT, "tests", "golden", "pose")


def twist_matrix(xi):
    v, w = xi[:3], xi[3:]
    T = torch.zeros(4, 4, dtype=xi.dtype)
    T[0, 1], T[0, 2], T[1, 0], T[1, 2], T[2, 0], T[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    T[:3, 3] = v
    return T


def _unit(g):
    a = torch.randn(3, dtype=torch.float64, generator=g)
    return a / a.norm()


def test_se3_exp_matches_matrix_exp(pkg):
    g = torch.Generator().manual_seed(0)
    # angles across [0, pi), both sides of the series threshold (theta^2 = 1e-2) included
    for theta in (0.0, 0.05, 0.0999, 0.1001, 0.3, 1.0, 2.0, 3.0, math.pi - 1e-3):
        xi = torch.cat([torch.randn(3, dtype=torch.float64, generator=g), _unit(g) * theta])
        err = (pkg.se3_exp(xi) - torch.linalg.matrix_exp(twist_matrix(xi))).abs().max().item()
        assert err <= 1e-12, (theta, err)
    for theta in (1e-12, 1e-9, 1e-7, 1e-5, 1e-3):
        xi = torch.cat([torch.randn(3, dtype=torch.float64, generator=g), _unit(g) * theta])
        err = (pkg.se3_exp(xi) - torch.linalg.matrix_exp(twist_matrix(xi))).abs().max().item()
        assert err <= 1e-9, (theta, err)
    E = pkg.se3_exp(torch.zeros(6, dtype=torch.float64))
    assert torch.equal(E, torch.eye(4, dtype=torch.float64))
    assert pkg.se3_exp(torch.zeros(6)).dtype == torch.float32
    with pytest.raises(ValueError):
        pkg.se3_exp(torch.zeros(3))


def test_se3_exp_autograd(pkg):
    g = torch.Generator().manual_seed(1)
    for theta in (0.0, 1e-6, 0.0999, 0.1001, 0.7, 2.5):
        xi = torch.cat([torch.randn(3, dtype=torch.float64, generator=g), _unit(g) * theta]).requires_grad_(True)
        assert torch.autograd.gradcheck(pkg.se3_exp, (xi,), eps=1e-6, atol=1e-7, rtol=1e-6), theta
    # the gradient at xi = 0 is the se(3) generators: finite, no NaN from sqrt
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    J = torch.autograd.functional.jacobian(pkg.se3_exp, xi)
    assert torch.isfinite(J).all()
    for k in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[k] = 1.0
        assert torch.allclose(J[..., k], twist_matrix(e), atol=1e-15)


def test_camera_pose_module(pkg):
    from stubs import Cam
    wv = torch.eye(4)
    wv[:3, 3] = torch.tensor([0.1, -0.2, 3.0])
    pose = pkg.CameraPose(Cam(40, 24, 1.0, 0.7, wv.numpy()))
    assert [n for n, _ in pose.named_parameters()] == ["xi"] and pose.xi.shape == (6,)
    assert torch.equal(pose.xi.detach(), torch.zeros(6))
    assert (pose._width, pose._height, pose._FoVx, pose._FoVy) == (40, 24, 1.0, 0.7)
    v = pose.world_view_transform()
    assert v.requires_grad and torch.equal(v.detach(), wv)
    with torch.no_grad():
        pose.xi.copy_(torch.tensor([0.1, 0.0, 0.0, 0.0, 0.0, 0.2]))
    v = pose.world_view_transform().detach()
    assert torch.allclose(v, pkg.se3_exp(pose.xi.detach()) @ wv)
    pose.bake()
    assert torch.equal(pose.xi.detach(), torch.zeros(6)) and torch.allclose(pose.world_view_transform().detach(), v)
    # a tensor attribute instead of a method, as the reference's own Camera has
    pose2 = pkg.CameraPose(Cam(8, 8, 1.0, 1.0, wv.numpy(), method=False))
    assert torch.equal(pose2.world_view_transform().detach(), wv)


def test_exports(pkg):
    for name in ("CameraPose", "se3_exp"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert "gs_project_backward_pose" in pkg._native.EXPORTS
    assert hasattr(pkg._native.load(), "gs_project_backward_pose")
    assert pkg._native.GS_ABI_VERSION == 23 == pkg._native.load().gs_abi_version()


def test_pose_struct_layout_matches_c(pkg, tmp_path):
    N = pkg._native
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(gs_project_pose_args), sizeof(gs_project_bwd_args), '
                   'offsetof(gs_project_pose_args, pose_partials), offsetof(gs_project_pose_args, pose_partial_rows), '
                   'offsetof(gs_project_pose_args, d_view));}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    P = N.GsProjectPoseArgs
    assert sizes == [C.sizeof(P), C.sizeof(N.GsProjectBwdArgs), P.pose_partials.offset, P.pose_partial_rows.offset,
                     P.d_view.offset]


def test_pose_bad_arguments_are_reported(pkg):
    N = pkg._native
    lib = N.load()
    assert lib.gs_project_backward_pose(None, None) == 1
    assert b"gs_project_backward_pose" in lib.gs_last_error() and b"null" in lib.gs_last_error()
    a = N.GsProjectPoseArgs()
    a.bwd.g.n = 300
    assert lib.gs_project_backward_pose(C.byref(a), None) == 1  # no d_view
    assert b"d_view" in lib.gs_last_error()
    dv = (C.c_float * 12)()
    a.d_view = C.cast(dv, C.c_void_p)
    assert lib.gs_project_backward_pose(C.byref(a), None) == 1  # no partials
    assert b"pose_partials" in lib.gs_last_error()
    rows = (C.c_double * 32)()
    a.pose_partials, a.pose_partial_rows = C.cast(rows, C.c_void_p), 1  # 300 Gaussians: 2 workgroups
    assert lib.gs_project_backward_pose(C.byref(a), None) == 1
    assert b"pose_partial_rows" in lib.gs_last_error()
    a.pose_partial_rows = 2
    assert lib.gs_project_backward_pose(C.byref(a), None) == 1  # the projection backward's own buffers
    assert b"null buffer" in lib.gs_last_error() and b"gs_project_backward_pose" in lib.gs_last_error()
    order = (C.c_uint32 * 300)()
    a.bwd.order = C.cast(order, C.c_void_p)
    assert lib.gs_project_backward_pose(C.byref(a), None) == 3
    assert b"order" in lib.gs_last_error()
    with pytest.raises(RuntimeError, match="gs_status=3"):
        N.check(lib.gs_project_backward_pose(C.byref(a), None), "gs_project_backward_pose")


def test_fixture_manifest_reference_deviation():
    man = json.load(open(os.path.join(POSE_GOLDEN, "manifest.json")))
    names = sorted(os.path.splitext(f)[0] for f in os.listdir(POSE_GOLDEN) if f.endswith(".npz"))
    assert names == sorted(man) and len(names) >= 7
    for name, rec in man.items():
        assert rec["ref_dev_R"] <= 5e-5 and rec["ref_dev_t"] <= 5e-5, (name, rec)
        assert rec["W"] <= 64 and rec["H"] <= 64 and rec["N"] <= 100, (name, rec)
        assert os.path.getsize(os.path.join(POSE_GOLDEN, name + ".npz")) <= 100 * 1024
