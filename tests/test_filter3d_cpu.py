"""The 3D smoothing filter (gs_filter3d_*; filter3d.py), the parts that need no
GPU: the struct layouts against the compiled header, the exports, the argument
checks (they return before any HIP call), the fp64 statements of
tests/filter3d_util.py checked against finite differences and each other, the
TrainingConfig fields and render(filter_3d=...)'s refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import filter3d_util as F3
import golden_io as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_filter3d_accumulate", "gs_filter3d_forward", "gs_filter3d_backward")


def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    R, A = N.GsFilter3dRateArgs, N.GsFilter3dArgs
    rate = [n for n, _ in R._fields_]
    args = [n for n, _ in A._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){'
                   'printf("%d %zu %zu", GS_FILTER3D_CAMERA_FLOATS, sizeof(gs_filter3d_rate_args), sizeof(gs_filter3d_args));'
                   + "".join(f'printf(" %zu", offsetof(gs_filter3d_rate_args, {n}));' for n in rate)
                   + "".join(f'printf(" %zu", offsetof(gs_filter3d_args, {n}));' for n in args) + "}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert sizes == [N.GS_FILTER3D_CAMERA_FLOATS, C.sizeof(R), C.sizeof(A)] + [getattr(R, n).offset for n in rate] + \
        [getattr(A, n).offset for n in args]
    assert N.GS_FILTER3D_CAMERA_FLOATS == 18
    assert N.load().gs_abi_version() == 23 == N.GS_ABI_VERSION
    assert all(name in N.EXPORTS and hasattr(N.load(), name) for name in NEW)


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
    nan, inf = float("nan"), float("inf")
    # -- the rate pass
    name = "gs_filter3d_accumulate"
    _refused(lib, name, lambda: lib.gs_filter3d_accumulate(None, None))
    good = dict(n=2, xyz=p, xyz_stride=3, cameras=p, num_cameras=1, near=0.2, margin=0.15, max_rate=p)
    for bad in (dict(xyz=None), dict(cameras=None), dict(max_rate=None), dict(n=-1), dict(num_cameras=-1),
                dict(xyz_stride=2), dict(near=0.0), dict(near=-0.2), dict(near=nan), dict(near=inf),
                dict(margin=-0.01), dict(margin=nan), dict(margin=inf), dict(margin=-inf)):
        a = N.GsFilter3dRateArgs(**{**good, **bad})
        _refused(lib, name, lambda: lib.gs_filter3d_accumulate(C.byref(a), None))
    # a bad scalar is refused even when there is nothing to do
    a = N.GsFilter3dRateArgs(**{**good, "n": 0, "near": nan})
    _refused(lib, name, lambda: lib.gs_filter3d_accumulate(C.byref(a), None))
    # nothing to do: GS_OK with nothing launched (NULL pointers are not even looked at)
    for empty in (dict(n=0), dict(num_cameras=0)):
        a = N.GsFilter3dRateArgs(**{**good, "xyz": None, "cameras": None, "max_rate": None, **empty})
        assert lib.gs_filter3d_accumulate(C.byref(a), None) == 0
    # -- the map
    fwd = ("scaling", "opacity", "filter", "scaling_out", "opacity_out")
    bwd = ("scaling", "opacity", "filter", "g_scaling_out", "g_opacity_out", "d_scaling", "d_opacity")
    for name, fields in (("gs_filter3d_forward", fwd), ("gs_filter3d_backward", bwd)):
        fn = getattr(lib, name)
        _refused(lib, name, lambda: fn(None, None))
        for missing in fields:
            a = N.GsFilter3dArgs(n=2, **{k: p for k in fields if k != missing})
            _refused(lib, name, lambda: fn(C.byref(a), None))
        a = N.GsFilter3dArgs(n=-1, **{k: p for k in fields})
        _refused(lib, name, lambda: fn(C.byref(a), None))
        assert fn(C.byref(N.GsFilter3dArgs(n=0)), None) == 0


def test_backward_statement_against_finite_differences():
    """map_backward64 (the header's formulas) against central differences of
    map64 in fp64, on rows where the map is not flat to fp64's resolution."""
    s, o, f, g_s, g_o = (a.astype(np.float64) for a in F3.map_inputs(400, 3))
    s = np.clip(s, -30, 20)  # (exp(2 s) against f^2 >= 1e-12: below, d s'/ds is under the differences' noise)
    d_s, d_o = F3.map_backward64(s, o, f, g_s, g_o)

    def L(s_, o_):
        with torch.no_grad():
            so, oo = F3.map64(s_, o_, f)
        return (so.numpy() * g_s).sum(-1) + oo.numpy() * g_o
    h = 1e-5
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd = (L(s + e, o) - L(s - e, o)) / (2 * h)
        assert np.abs(fd - d_s[:, k]).max() <= 1e-8, k
    fd = (L(s, o + h) - L(s, o - h)) / (2 * h)
    assert np.abs(fd - d_o).max() <= 1e-8
    # and autograd of the fp64 forward says the same
    st, ot = torch.tensor(s, requires_grad=True), torch.tensor(o, requires_grad=True)
    so, oo = F3.map64(st, ot, f)
    ((so * torch.tensor(g_s)).sum() + (oo * torch.tensor(g_o)).sum()).backward()
    assert np.abs(st.grad.numpy() - d_s).max() <= 1e-12 and np.abs(ot.grad.numpy() - d_o).max() <= 1e-12


def test_fp32_restatement_and_the_recorded_errors():
    """The fp32 restatement is finite over the whole range, copies f == 0 rows,
    and its errors against fp64 are the ones filter3d_util's table records."""
    inputs = F3.map_inputs(1000, 0)
    s, o, f, g_s, g_o = inputs
    got = F3.map32(s, o, f) + F3.map_backward32(*inputs)
    assert all(np.isfinite(a).all() for a in got)
    off = f == 0
    assert off.sum() > 100 and np.array_equal(got[0][off].view(np.int32), s[off].view(np.int32))
    assert np.array_equal(got[2][off].view(np.int32), g_s[off].view(np.int32))
    e = F3.errors(got, F3.reference64(inputs))
    print("  fp32 restatement against fp64:", {k: f"{v:.2g}" for k, v in e.items()})
    recorded = dict(s_out=1.1e-07, o_out=1.6e-07, d_s=1.9e-07, d_o=7.2e-08)
    for k, v in e.items():  # (glibc / numpy versions may round an exp the other way: a factor of two)
        assert 0 < v <= 2 * recorded[k], (k, v)


def test_equivalent_map_is_the_oracles_covariance():
    """With f = 0 the equivalent scene's cov3d is the oracle's R diag(exp(2 s)) R^T."""
    d = F3.model_scene(200, 1)
    d["filter"] = np.zeros_like(d["filter"])
    with torch.no_grad():
        cov, op = F3.equivalent_map(*F3._leaves(d), d["filter"])
    want = G.oracle().covariance(d["scaling"], d["rotation"]).reshape(-1, 3, 3)
    assert np.abs(cov.numpy() - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(op.numpy() - 1 / (1 + np.exp(-d["opacity_raw"].astype(np.float64)))).max() <= 1e-15


def test_rate_statement_and_cases():
    xyz, cams, rate = F3.rate_case(1000, 17, 5)
    assert xyz.dtype == np.float32 and cams.shape == (17, 18)
    one = [F3.rate_statement(xyz, cams[k:k + 1], 0.2, 0.15)[0] for k in range(17)]
    assert np.array_equal(np.max(one, 0), rate)
    seen_by = np.sum([r > 0 for r in one], 0)
    assert (seen_by == 0).sum() > 50 and (seen_by > 1).sum() > 50
    # one camera on the axis: the rate is focal / depth
    cam = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 50, 40, 16, 16, 32, 32]], np.float32)
    r, _ = F3.rate_statement(np.array([[0, 0, 4], [0, 0, 0.1], [0, 0, -4], [3, 0, 4]], np.float32), cam, 0.2, 0.15)
    assert np.array_equal(r, [12.5, 0, 0, 0])


def test_training_config(pkg):
    cfg = pkg.TrainingConfig()
    assert (cfg.filter_3d, cfg.filter_3d_variance, cfg.filter_3d_interval) == (False, 0.2, 100)
    cfg.check()
    pkg.TrainingConfig(filter_3d=True, filter_3d_variance=0.0, filter_3d_interval=1).check()
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="filter_3d_variance"):
            pkg.TrainingConfig(filter_3d_variance=bad).check()
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError, match="filter_3d_interval"):
            pkg.TrainingConfig(filter_3d_interval=bad).check()
    assert pkg.GaussianTrainer(pkg.TrainingConfig()).filter_3d is None


def test_filter_object_and_render_refusals(pkg):
    """ValueError before anything is launched (there is no device here to launch on)."""
    from stubs import Cam, Gauss
    for bad in (-0.2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="variance"):
            pkg.Filter3D(4, "cpu", variance=bad)
    with pytest.raises(ValueError, match="near"):
        pkg.Filter3D(4, "cpu", near=0.0)
    with pytest.raises(ValueError, match="margin"):
        pkg.Filter3D(4, "cpu", margin=-1.0)
    flt = pkg.Filter3D(5, "cpu")
    assert flt.max_rate.shape == flt.values.shape == (5,) and flt.values.dtype == torch.float32
    cam = Cam(16, 16, 1.0, 1.0)
    st = pkg.RenderSettings(16, 16, torch.zeros(3))
    r = pkg.GaussianRenderer()
    n = 5
    stub = Gauss(np.zeros((n, 3)), np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3)), np.full(n, 0.5), "cpu")
    with pytest.raises(ValueError, match="get_covariance"):
        r.render(cam, stub, st, filter_3d=flt)
    m = pkg.GaussianModel()
    m._set(torch.zeros(n, 3), torch.zeros(n, 1, 3), torch.zeros(n, 15, 3), torch.zeros(n, 3),
           torch.ones(n, 4), torch.zeros(n, 1))
    with pytest.raises(ValueError, match="Gaussians"):
        r.render(cam, m, st, filter_3d=pkg.Filter3D(n + 1, "cpu"))
    with pytest.raises(ValueError, match="Filter3D"):
        r.render(cam, m, st, filter_3d=torch.zeros(n))
    flt.values = flt.values.double()
    with pytest.raises(ValueError, match="fp32"):
        r.render(cam, m, st, filter_3d=flt)
    flt = pkg.Filter3D(n, "cpu")
    flt.variance = -1.0  # (set after construction)
    with pytest.raises(ValueError, match="variance"):
        r.render(cam, m, st, filter_3d=flt)
    with pytest.raises(ValueError, match="apply_filter_3d"):
        pkg.apply_filter_3d(torch.zeros(n, 3), torch.zeros(n + 1), torch.zeros(n))
    with pytest.raises(ValueError, match="fp32"):
        pkg.apply_filter_3d(torch.zeros(n, 3), torch.zeros(n), torch.zeros(n, dtype=torch.float64))
