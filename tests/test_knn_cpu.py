"""k-nearest neighbours without a GPU: gs_knn's argument checks (they return
before any HIP call) and its struct against the C compiler's size, the torch
CPU path against the fp64 reference of tests/knn_util.py on every generator,
the ValueErrors, GaussianModel's scale_init on the CPU, the config check, and
two closed forms that pin the reference itself."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import knn_util as KU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------- C ABI ----
def _args(N, **kw):
    a = N.GsKnnArgs(300, 3, 256, 256, 256, 256, 256, 1 << 30)
    for name, v in kw.items():
        setattr(a, name, v)
    return a


def test_knn_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    call = lambda a: lib.gs_knn(C.byref(a), None)
    assert lib.gs_knn(None, None) == 1
    assert b"gs_knn" in lib.gs_last_error() and b"null" in lib.gs_last_error()
    for bad in (dict(points=None), dict(dist2=None, index=None, mean_dist2=None), dict(k=0), dict(k=17), dict(k=-1),
                dict(n=-1), dict(workspace=None), dict(workspace_bytes=lib.gs_knn_workspace_bytes(300) - 1),
                dict(workspace_bytes=0), dict(workspace=264)):
        assert call(_args(N, **bad)) == 1, bad
        assert b"gs_knn" in lib.gs_last_error(), bad
    for n in ((1 << 30) + 1, (1 << 31) - 1):
        assert call(_args(N, n=n)) == 3, n
        assert b"gs_knn" in lib.gs_last_error() and b"2^30" in lib.gs_last_error()
    # nothing to search: GS_OK with nothing launched (no pointer is looked at)
    assert call(_args(N, n=0, points=None, workspace=None, workspace_bytes=0)) == 0
    with pytest.raises(RuntimeError, match="gs_status=1"):
        N.check(call(_args(N, k=0)), "gs_knn")


def test_knn_workspace_bytes(pkg):
    lib = pkg._native.load()
    sort = lib.gs_radix_sort_workspace_bytes
    for n in (1, 255, 256, 257, 100_000, 1 << 30):
        nb = -(-n // 256)
        # two key / value pairs and the high key words, the sort's, the sorted points, the boxes, the cloud's box
        need = 5 * 4 * n + sort(n) + 16 * n + 2 * 16 * nb + 2 * 16 * nb + 32
        assert need <= lib.gs_knn_workspace_bytes(n) <= need + 12 * 256, n
    assert [lib.gs_knn_workspace_bytes(n) for n in (0, -5, (1 << 30) + 1)] == [0, 0, 0]
    assert pkg._native.GS_KNN_MAX_K == 16


def test_struct_layout_matches_c(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gsplat_mi355x.h"\n'
                   'int main(){printf("%zu %d\\n", sizeof(gs_knn_args), GS_KNN_MAX_K);}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, max_k = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(pkg._native.GsKnnArgs) and max_k == pkg._native.GS_KNN_MAX_K


# ----------------------------------------------------- the reference itself ----
def test_reference_on_a_lattice():
    """10 x 10 x 10, spacing 0.25: every point, corners included, has three
    neighbours at exactly one spacing."""
    d, idx = KU.ref_knn(KU.lattice(), 3)
    assert (d == 0.0625).all()
    assert (idx[0] == (1, 10, 100)).all()  # the corner's: +z, +y, +x, by index


def test_reference_on_a_line():
    d, idx = KU.ref_knn(KU.line(), 3)
    want_d, want_i = KU.line_expected()
    assert np.array_equal(d, want_d.astype(np.float64)) and np.array_equal(idx, want_i.astype(np.int64))
    assert d[5].tolist() == [0.25, 0.25, 1.0] and d[0].tolist() == d[-1].tolist() == [0.25, 1.0, 2.25]
    assert np.array_equal(KU.ref_mean(KU.line(), 3)[:2], [3.5 / 3, 0.5])


# ------------------------------------------------------ the torch CPU path ----
CPU_CASES = [(name, k) for name in KU.GENERATORS for k in (3, 8)] + \
            [(f"uniform{n}", k) for n, k in ((1, 1), (1, 3), (2, 3), (3, 3), (4, 3), (4, 16), (17, 16), (257, 1),
                                             (1000, 4), (2000, 3), (2000, 16))]


def _points(name):
    return KU.GENERATORS[name]() if name in KU.GENERATORS else KU.uniform_cube(int(name[len("uniform"):]))


@pytest.mark.parametrize("name,k", CPU_CASES)
def test_cpu_path_against_reference(pkg, name, k):
    pts = _points(name)
    assert len(pts) <= 2000
    d, i = pkg.knn(torch.from_numpy(pts), k)
    m = pkg.mean_knn_dist2(torch.from_numpy(pts), k)
    assert d.device.type == "cpu" and i.dtype == torch.int32
    KU.check_against_ref(pts, k, d.numpy(), i.numpy(), m.numpy())
    assert pkg.knn(torch.from_numpy(pts), k, return_index=False)[1] is None


def test_cpu_path_closed_forms(pkg):
    d, i = pkg.knn(torch.from_numpy(KU.lattice()), 3)
    assert bool((d == 0.0625).all()) and i[0].tolist() == [1, 10, 100]
    assert bool((pkg.mean_knn_dist2(torch.from_numpy(KU.lattice())) == 0.0625).all())
    d, i = pkg.knn(torch.from_numpy(KU.line()), 3)
    want_d, want_i = KU.line_expected()
    assert np.array_equal(d.numpy(), want_d) and np.array_equal(i.numpy(), want_i)
    # duplicates: distance 0, smaller rows first, never the row itself
    d, i = pkg.knn(torch.from_numpy(KU.identical(6)), 3)
    assert bool((d == 0).all()) and i.tolist()[0] == [1, 2, 3] and i.tolist()[2] == [0, 1, 3] and i.tolist()[5] == [0, 1, 2]
    # fewer than k neighbours
    d, i = pkg.knn(torch.tensor([[0.0, 0, 0], [3.0, 4, 0]]), 3)
    assert d.tolist() == [[25.0, math.inf, math.inf]] * 2 and i.tolist() == [[1, -1, -1], [0, -1, -1]]
    assert pkg.mean_knn_dist2(torch.tensor([[0.0, 0, 0], [3.0, 4, 0]]), 3).tolist() == [25.0, 25.0]
    assert pkg.mean_knn_dist2(torch.tensor([[1.0, 2, 3]]), 3).tolist() == [0.0]
    # a float64 input is searched in fp32
    d64, _ = pkg.knn(torch.from_numpy(KU.line()).double(), 3)
    assert d64.dtype == torch.float32 and np.array_equal(d64.numpy(), want_d)


def test_value_errors(pkg):
    ok = torch.zeros(5, 3)
    bad_calls = [
        lambda: pkg.knn(torch.zeros(5, 2)), lambda: pkg.knn(torch.zeros(5)), lambda: pkg.knn(torch.zeros(2, 5, 3)),
        lambda: pkg.knn(np.zeros((5, 3), np.float32)), lambda: pkg.knn(torch.zeros(5, 3, dtype=torch.int32)),
        lambda: pkg.knn(ok, 0), lambda: pkg.knn(ok, 17), lambda: pkg.knn(ok, 2.0), lambda: pkg.knn(ok, True),
        lambda: pkg.knn(torch.tensor([[0.0, float("nan"), 0]])), lambda: pkg.knn(torch.tensor([[float("inf"), 0, 0]])),
        lambda: pkg.knn(ok.to("meta")),
        lambda: pkg.mean_knn_dist2(torch.zeros(5, 4)), lambda: pkg.mean_knn_dist2(ok, 0),
        lambda: pkg.mean_knn_dist2(ok, 17), lambda: pkg.mean_knn_dist2(torch.tensor([[0.0, float("-inf"), 0]])),
    ]
    for n, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {n} raised nothing")
    d, i = pkg.knn(torch.zeros(0, 3), 4)
    assert d.shape == (0, 4) and d.dtype == torch.float32 and i.shape == (0, 4) and i.dtype == torch.int32
    assert pkg.mean_knn_dist2(torch.zeros(0, 3)).shape == (0,)
    assert "knn" in pkg.__all__ and "mean_knn_dist2" in pkg.__all__


# ---------------------------------------------------------- model and config ----
def _scaling_atol(want):
    """log sqrt halves the relative error of the mean (knn_util's rule: RTOL plus
    the fp32 sum's roundings) into an absolute one on the log; sqrt and log then
    round in fp32 (4 ulp of the largest |log| for the two)."""
    return 0.5 * (KU.RTOL + 4 * 2.0 ** -24) + 4 * 2.0 ** -24 * max(1.0, float(np.abs(want).max()))


def test_create_from_points_scale_init(pkg):
    pts = KU.clusters(200)
    points, colors = torch.from_numpy(pts), torch.rand(len(pts), 3)

    def make(**kw):
        torch.manual_seed(11)
        g = pkg.GaussianModel()
        g.create_from_points(points, colors, **kw)
        return g

    default, extent, knn = make(), make(scale_init="extent"), make(scale_init="knn")
    for name in ("_scaling", "_rotation", "_opacity", "_xyz", "_features_dc"):
        assert torch.equal(getattr(default, name), getattr(extent, name)), name
    ext = float((points.max(0).values - points.min(0).values).mean())
    assert torch.equal(default._scaling, torch.full((len(pts), 3), math.log(0.01 * ext)))
    # "knn": 3DGS's rule from the reference's distances; nothing else moves, no extra draw
    want = np.log(np.sqrt(np.maximum(KU.ref_mean(pts, 3), 1e-7)))
    got = knn._scaling.detach().numpy()
    assert got.shape == (len(pts), 3) and (got[:, :1] == got).all()
    np.testing.assert_allclose(got[:, 0], want, rtol=0, atol=_scaling_atol(want))
    for name in ("_rotation", "_opacity", "_xyz", "_features_dc", "_features_rest"):
        assert torch.equal(getattr(knn, name), getattr(extent, name)), name
    assert not torch.equal(knn._scaling, extent._scaling)
    # coincident points: the clamp, not -inf
    g = pkg.GaussianModel()
    g.create_from_points(torch.zeros(4, 3), scale_init="knn")
    assert torch.equal(g._scaling, torch.full((4, 3), 1e-7).sqrt().log())
    for bad in ("nope", None, "KNN"):
        with pytest.raises(ValueError, match="scale_init"):
            pkg.GaussianModel().create_from_points(points, scale_init=bad)
        with pytest.raises(ValueError, match="scale_init"):
            pkg.GaussianModel().create_from_random(10, scale_init=bad)
        with pytest.raises(ValueError, match="scale_init"):
            pkg.GaussianModel().create_from_pcd("nowhere.ply", scale_init=bad)


def test_create_from_random_scale_init(pkg):
    def make(**kw):
        g = pkg.GaussianModel()
        g.create_from_random(400, scene_extent=1.3, device="cpu", generator=torch.Generator().manual_seed(5), **kw)
        return g

    default, extent, knn = make(), make(scale_init="extent"), make(scale_init="knn")
    for a, b in zip(default.parameter_list(), extent.parameter_list()):
        assert torch.equal(a, b)
    assert torch.equal(default._scaling, torch.full((400, 3), math.log(0.02 * 1.3)))
    for name in ("_xyz", "_features_dc", "_rotation", "_opacity"):
        assert torch.equal(getattr(knn, name), getattr(extent, name)), name
    want = np.log(np.sqrt(np.maximum(KU.ref_mean(knn._xyz.detach().numpy(), 3), 1e-7)))
    np.testing.assert_allclose(knn._scaling.detach().numpy()[:, 0], want, rtol=0, atol=_scaling_atol(want))


def test_config_scale_init(pkg):
    assert pkg.TrainingConfig().scale_init == "extent"
    pkg.TrainingConfig().check()
    pkg.TrainingConfig(scale_init="knn").check()
    with pytest.raises(ValueError, match="scale_init"):
        pkg.TrainingConfig(scale_init="nope").check()
