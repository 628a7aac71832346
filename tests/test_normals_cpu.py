"""Normal consistency (gs_gaussian_normals_*, gs_normal_consistency_*;
normals.py), the parts that need no GPU: the struct layouts against the
compiled header, the exports, the argument checks (they return before any HIP
call), the fp64 statements of tests/normals_util.py checked against central
differences, autograd and a plane's closed form, the TrainingConfig fields and
render(normals=True)'s refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import normals_util as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_gaussian_normals_forward", "gs_gaussian_normals_backward",
       "gs_normal_consistency_forward", "gs_normal_consistency_backward")


def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    structs = (("gs_gaussian_normals_args", N.GsGaussianNormalsArgs), ("gs_normal_consistency_args", N.GsNormalConsistencyArgs))
    src = tmp_path / "sz.c"
    body = "".join(f'printf(" %zu", sizeof({c}));' + "".join(f'printf(" %zu", offsetof({c}, {n}));' for n, _ in S._fields_)
                   for c, S in structs)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){' + body + "}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = []
    for _, S in structs:
        want += [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert sizes == want
    assert N.load().gs_abi_version() == 23 == N.GS_ABI_VERSION
    assert all(name in N.EXPORTS and hasattr(N.load(), name) for name in NEW)
    assert pkg.gaussian_normals is pkg.normals.gaussian_normals and pkg.normal_consistency is pkg.normals.normal_consistency


def test_stale_library_is_named_by_its_missing_exports(pkg, tmp_path, monkeypatch):
    """A library built before this feature has the same ABI number: load()
    names the four exports it lacks, and no other."""
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
    nan, inf = float("nan"), float("inf")
    view = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    common = ("rotation", "scaling", "xyz")
    for name, fields in (("gs_gaussian_normals_forward", common + ("normals",)),
                         ("gs_gaussian_normals_backward", common + ("g_normals", "d_rotation"))):
        fn = getattr(lib, name)
        _refused(lib, name, lambda: fn(None, None))
        for missing in fields:
            a = N.GsGaussianNormalsArgs(n=2, xyz_stride=3, view=view, **{k: p for k in fields if k != missing})
            _refused(lib, name, lambda: fn(C.byref(a), None))
        for bad in (dict(n=-1), dict(xyz_stride=2), dict(xyz_stride=-3)):
            a = N.GsGaussianNormalsArgs(**{**dict(n=2, xyz_stride=3, view=view), **{k: p for k in fields}, **bad})
            _refused(lib, name, lambda: fn(C.byref(a), None))
        # nothing to do: GS_OK with nothing launched (NULL pointers are not even looked at)
        assert fn(C.byref(N.GsGaussianNormalsArgs(n=0)), None) == 0
    good = dict(width=8, height=6, fx=10.0, fy=-9.0, cx=4.0, cy=3.0)
    for name, fields in (("gs_normal_consistency_forward", ("normals", "depth", "alpha", "error")),
                         ("gs_normal_consistency_backward", ("normals", "depth", "alpha", "g_error", "d_normals", "d_depth"))):
        fn = getattr(lib, name)
        _refused(lib, name, lambda: fn(None, None))
        for missing in fields:
            a = N.GsNormalConsistencyArgs(**good, **{k: p for k in fields if k != missing})
            _refused(lib, name, lambda: fn(C.byref(a), None))
        for bad in (dict(width=0), dict(height=0), dict(width=-4), dict(height=-1), dict(fx=0.0), dict(fy=0.0),
                    dict(fx=nan), dict(fy=nan), dict(fx=inf), dict(fy=-inf), dict(cx=nan), dict(cy=inf)):
            a = N.GsNormalConsistencyArgs(**{**good, **{k: p for k in fields}, **bad})
            _refused(lib, name, lambda: fn(C.byref(a), None))


def test_gaussian_backward_statement():
    """gaussian_normals_backward64 (the header's formulas) against central
    differences and autograd of the fp64 forward; the forward's normals are
    unit vectors that face the camera."""
    q, s, xyz, view, g = NU.gaussian_case(300, 3)
    n, k, d, pc = NU.gaussian_normals64(q, s, xyz, view)
    assert set(k.tolist()) == {0, 1, 2} and (d > 0).sum() > 50 and (d < 0).sum() > 50
    # (the view is a rotation rounded to fp32: orthogonal to an fp32 ulp, not to fp64's)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 2e-7 and ((n * pc).sum(1) < 0).all()
    dq = NU.gaussian_normals_backward64(q, s, xyz, view, g)
    qt = NU.T(q).requires_grad_(True)
    (NU.gaussian_normals_torch(qt, NU.T(s), NU.T(xyz), NU.T(view))[0] * NU.T(g)).sum().backward()
    scale = np.linalg.norm(g, axis=1) / np.linalg.norm(q.astype(np.float64), axis=1)
    assert (np.abs(qt.grad.numpy() - dq).max(1) <= 1e-13 * scale).all()
    L = lambda q_: (NU.gaussian_normals64(q_, s, xyz, view)[0] * g).sum(1)
    h = 1e-6
    for c in range(4):
        e = np.zeros(4)
        e[c] = h
        fd = (L(q.astype(np.float64) + e) - L(q.astype(np.float64) - e)) / (2 * h)
        assert (np.abs(fd - dq[:, c]) <= 1e-7 * np.maximum(scale, 1)).all(), c
    # the gradient is tangent to the quaternion (R(q^) does not depend on |q|)
    assert (np.abs((dq * q).sum(1)) <= 1e-13 * np.linalg.norm(g, axis=1)).all()


def test_gaussian_exact_rows():
    """Equal scales take axis 0; the identity quaternion under an identity view is +-e_k."""
    eye = np.eye(4)
    q = np.tile([[1.0, 0, 0, 0]], (4, 1))
    s = np.array([[0.5, 0.5, 0.5], [0.1, -1.0, 0.3], [0.2, 0.2, -3.0], [-2.0, 0.0, -2.0]])
    xyz = np.array([[1.0, 2, 3], [1.0, 2, 3], [-1.0, -2, -3], [0.5, 1, 1]])
    n, k, _, _ = NU.gaussian_normals64(q, s, xyz, eye)
    assert k.tolist() == [0, 1, 2, 0]
    assert np.array_equal(n, [[-1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0]])
    # an exact 0 of n_c . p_c keeps the sign
    n, _, d, _ = NU.gaussian_normals64(q[:1], s[:1], np.array([[0.0, 2, 3]]), eye)
    assert d[0] == 0 and np.array_equal(n, [[1, 0, 0]])


@pytest.mark.parametrize("W,H", [(3, 3), (17, 19), (33, 18)])
def test_consistency_backward_statement(W, H):
    """consistency_backward64 (the header's gather) against autograd of the fp64
    forward to 1e-13 of scale, and central differences on a few pixels."""
    intr = NU.intrinsics(W, H)
    Nr, D, A, g = NU.pixel_case(H, W, W + H)
    dn, dd = NU.consistency_backward64(Nr, D, A, intr, g)
    nt, dt, at = NU.T(Nr).requires_grad_(True), NU.T(D).requires_grad_(True), NU.T(A).requires_grad_(True)
    (NU.consistency_torch(nt, dt, at, intr)[0] * NU.T(g)).sum().backward()
    assert at.grad is None
    assert np.abs(nt.grad.numpy() - dn).max() <= 1e-13 * max(1.0, np.abs(dn).max())
    assert np.abs(dt.grad.numpy() - dd).max() <= 1e-13 * max(1.0, np.abs(dd).max())
    assert np.abs(dd).max() > 0 and (dn[:, 0] == 0).all() and (dn[:, :, -1] == 0).all()
    L = lambda D_: (NU.consistency64(Nr, D_, A, intr)[0] * g).sum()
    rng = np.random.default_rng(0)
    h = 1e-6
    for _ in range(6):
        y, x = int(rng.integers(H)), int(rng.integers(W))
        e = np.zeros((H, W))
        e[y, x] = h
        fd = (L(D.astype(np.float64) + e) - L(D.astype(np.float64) - e)) / (2 * h)
        assert abs(fd - dd[y, x]) <= 1e-6 * max(1.0, np.abs(dd).max()), (y, x)


def test_plane_closed_form_and_degenerate_depth():
    """Independent of the restatement: every interior normal of a plane's depth
    map is the plane's, facing the camera; borders are exactly 0; images
    without an interior have error exactly 1; zeros in the depth map give
    n_d = 0 and finite gradients."""
    W, H = 16, 16
    intr = NU.intrinsics(W, H)
    D = NU.plane_depth(H, W, intr)
    assert 2.5 < D.min() and D.max() < 4.2
    e, nd = NU.consistency64(np.tile(NU.PLANE_N[:, None, None], (1, H, W)), D, np.ones((H, W)), intr)
    inner = nd[:, 1:-1, 1:-1]
    assert np.abs(inner - NU.PLANE_N[:, None, None]).max() <= 2e-15 and NU.PLANE_N[2] < 0
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert (nd[:, border] == 0).all() and (e[border] == 1).all() and np.abs(e[~border]).max() <= 4e-15
    for w, h in ((1, 1), (2, 2), (3, 1)):
        Nr, Dd, A, g = NU.pixel_case(h, w, 5)
        e, nd = NU.consistency64(Nr, Dd, A, NU.intrinsics(w, h))
        dn, dd = NU.consistency_backward64(Nr, Dd, A, NU.intrinsics(w, h), g)
        assert (e == 1).all() and (nd == 0).all() and (dn == 0).all() and (dd == 0).all()
    W, H = 50, 37
    intr = NU.intrinsics(W, H)
    Nr, Dd, A, g = NU.pixel_case(H, W, 6)
    Dd[10:20, 5:30] = 0
    e, nd = NU.consistency64(Nr, Dd, A, intr)
    dn, dd = NU.consistency_backward64(Nr, Dd, A, intr, g)
    assert (nd[:, 12:18, 7:28] == 0).all() and (e[12:18, 7:28] == 1).all()
    assert np.isfinite(dn).all() and np.isfinite(dd).all() and np.isfinite(nd).all()


def test_training_config(pkg):
    cfg = pkg.TrainingConfig()
    assert (cfg.lambda_normal, cfg.normal_from_iter) == (0.0, 0)
    cfg.check()
    pkg.TrainingConfig(lambda_normal=0.05, normal_from_iter=7000).check()
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lambda_normal"):
            pkg.TrainingConfig(lambda_normal=bad).check()
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="normal_from_iter"):
            pkg.TrainingConfig(normal_from_iter=bad).check()


def test_python_refusals(pkg):
    """ValueError before anything is launched (there is no device here to launch on)."""
    from stubs import Cam, Gauss
    cam = Cam(16, 16, 1.0, 1.0)
    st = pkg.RenderSettings(16, 16, torch.zeros(3))
    r = pkg.GaussianRenderer()
    n = 5
    stub = Gauss(np.zeros((n, 3)), np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3)), np.full(n, 0.5), "cpu")
    with pytest.raises(ValueError, match="normals=True needs this package's GaussianModel"):
        r.render(cam, stub, st, normals=True)
    m = pkg.GaussianModel()
    m._set(torch.zeros(n, 3), torch.zeros(n, 1, 3), torch.zeros(n, 15, 3), torch.zeros(n, 3),
           torch.ones(n, 4), torch.zeros(n, 1))
    with pytest.raises(ValueError, match="GS_MAX_FEATURE_CHANNELS"):
        r.render(cam, m, st, normals=True, features=torch.zeros(n, 254))
    with pytest.raises(ValueError, match="features must be"):
        r.render(cam, m, st, normals=True, features=torch.zeros(n + 1, 4))
    q, s, x, wv = torch.ones(n, 4), torch.zeros(n, 3), torch.zeros(n, 3), torch.eye(4)
    for args, what in (((q[:, :3], s, x, wv), "rotation"), ((q, s[:4], x, wv), "scaling"), ((q, s, x.double(), wv), "fp32"),
                       ((q, s, x[:, :2], wv), "xyz"), ((q, s, x, torch.eye(3)), "world_view")):
        with pytest.raises(ValueError, match=what):
            pkg.gaussian_normals(*args)
    img = torch.zeros(3, 8, 8)
    for args, what in (((img[:2], img[0], img[0]), "normals"), ((img, img[0, :4], img[0]), "depth"),
                       ((img, img[0], img[0, :, :3]), "alpha")):
        with pytest.raises(ValueError, match=what):
            pkg.normal_consistency(*args, cam)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.normal_consistency(img, img[0], img[0], cam)
