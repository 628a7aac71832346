"""TSDF fusion and mesh extraction without a GPU: the entry points' argument
checks (they return before any HIP call), the ctypes structs against the C
compiler's sizes, every ValueError of tsdf.py, the PLY writer's round trip, and
the fp64 restatement of tests/tsdf_util.py against a sphere's closed forms --
which pins the winding and ordering rules independently of the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_util as TU
from stubs import Cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------- C ABI ----
def _volume(N, nx=4, ny=4, nz=4, h=0.1, ptr=64):
    return N.GsTsdfVolume(nx, ny, nz, (C.c_float * 3)(0, 0, 0), h, ptr, ptr, None)


def _integrate_args(N, vol=None, **kw):
    a = N.GsTsdfIntegrateArgs(vol if vol is not None else _volume(N), 1, 8, 8, 64, 64, None, None, 0.2, 0.4, 0.5,
                              float("inf"))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_integrate_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    call = lambda a: lib.gs_tsdf_integrate(C.byref(a), None)
    assert lib.gs_tsdf_integrate(None, None) == 1
    assert b"gs_tsdf_integrate" in lib.gs_last_error() and b"null" in lib.gs_last_error()
    for bad in (dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("nan")), dict(trunc=float("inf")),
                dict(near=float("nan")), dict(near=0.0), dict(alpha_min=float("nan")), dict(depth_max=float("nan")),
                dict(num_views=0), dict(width=0), dict(height=-1), dict(cameras=None), dict(depth=None)):
        assert call(_integrate_args(N, **bad)) == 1, bad
        assert b"gs_tsdf_integrate" in lib.gs_last_error(), bad
    assert call(_integrate_args(N, _volume(N, ptr=None))) == 1
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        assert call(_integrate_args(N, _volume(N, *dims))) == 1, dims
        assert b"dimension" in lib.gs_last_error()
    for dims in ((2048, 1024, 1024), (1 << 16, 1 << 15, 1), (1291, 1291, 1291)):  # 2^31, 2^31, just above
        assert call(_integrate_args(N, _volume(N, *dims))) == 3, dims
        assert b"gs_tsdf_integrate" in lib.gs_last_error() and b"2^31" in lib.gs_last_error()
    assert call(_integrate_args(N, _volume(N, h=0.0))) == 1
    with pytest.raises(RuntimeError, match="gs_status=1"):
        N.check(call(_integrate_args(N, trunc=0.0)), "gs_tsdf_integrate")


def test_mesh_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    for name in ("gs_mesh_classify", "gs_mesh_emit"):
        f = getattr(lib, name)
        assert f(None, None) == 1
        assert name.encode() in lib.gs_last_error() and b"null" in lib.gs_last_error()
        for dims in ((0, 4, 4), (4, 4, 0)):
            assert f(C.byref(N.GsMeshArgs(_volume(N, *dims), 1.0, 64, 64, 64)), None) == 1, (name, dims)
            assert name.encode() in lib.gs_last_error()
        assert f(C.byref(N.GsMeshArgs(_volume(N, 2048, 1024, 1024), 1.0, 64, 64, 64)), None) == 3
        assert f(C.byref(N.GsMeshArgs(_volume(N, ptr=None), 1.0, 64, 64, 64)), None) == 1
    assert lib.gs_mesh_classify(C.byref(N.GsMeshArgs(_volume(N), float("nan"), 64, 64, 64)), None) == 1
    assert lib.gs_mesh_classify(C.byref(N.GsMeshArgs(_volume(N), 1.0, None, 64, 64)), None) == 1
    assert lib.gs_mesh_classify(C.byref(N.GsMeshArgs(_volume(N), 1.0, 64, None, 64)), None) == 1
    emit = lambda **kw: lib.gs_mesh_emit(C.byref(N.GsMeshArgs(_volume(N), 1.0, 64, 64, 64, **kw)), None)
    assert emit(num_vertices=-1) == 1
    assert emit(num_vertices=28) == 1 and b"more vertices than cells" in lib.gs_last_error()  # 27 cells
    assert emit(num_vertices=3, cell_rank=64, vertices=None) == 1
    assert emit(num_faces=2, cell_rank=64, node_faces=64, faces=None) == 1
    assert emit(num_vertices=3, cell_rank=64, vertices=64, colors=64) == 1  # colours without a colour volume
    assert emit() == 0  # nothing to emit: no launch


def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    names = ["gs_tsdf_volume", "gs_tsdf_integrate_args", "gs_mesh_args"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gsplat_mi355x.h"\nint main(){' +
                   "".join('printf("%%zu\\n", sizeof(%s));' % n for n in names) + "}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(t) for t in (N.GsTsdfVolume, N.GsTsdfIntegrateArgs, N.GsMeshArgs)]
    assert N.GS_TSDF_CAMERA_FLOATS == 16 <= N.GS_FILTER3D_CAMERA_FLOATS


# ----------------------------------------------------------------- tsdf.py ----
def test_volume_value_errors(pkg):
    V = pkg.TSDFVolume
    ok = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(3, 4, 5), device="cpu")
    vol = V(**ok)
    assert vol.tsdf.shape == (5, 4, 3) and vol.color.shape == (3, 5, 4, 3) and vol.trunc == pytest.approx(0.4)
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all()) and bool((vol.color == 0).all())
    assert V(color=False, **ok).color is None
    for bad in (dict(origin=(0, 0)), dict(origin=(0, float("nan"), 0)), dict(origin="abc"), dict(voxel_size=0.0),
                dict(voxel_size=float("inf")), dict(voxel_size="1"), dict(dims=(3, 4)), dict(dims=(3, 0, 5)),
                dict(dims=(3.0, 4, 5)), dict(dims=(2048, 1024, 1024)), dict(trunc=0.0), dict(trunc=float("nan")),
                dict(near=0.0), dict(near=float("nan"))):
        with pytest.raises(ValueError):
            V(**dict(ok, **bad))
    b = V.from_bounds((-1, -1, -1), (1, 0.5, 1.04), 0.1, "cpu", color=False)
    assert b.dims == (21, 16, 22) and b.origin == (-1.0, -1.0, -1.0)
    for lo, hi, h in (((0, 0, 0), (1, -1, 1), 0.1), ((0, 0), (1, 1, 1), 0.1), ((0, 0, 0), (1, 1, 1), 0.0),
                      ((0, 0, 0), (1, 1, float("inf")), 0.1)):
        with pytest.raises(ValueError):
            V.from_bounds(lo, hi, h, "cpu")
    # state round trip, and its errors
    vol.tsdf.uniform_(-1, 1)
    vol.weight.fill_(2)
    st = {k: v.clone() for k, v in vol.state().items()}
    vol.reset()
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all())
    vol.load_state(st)
    assert torch.equal(vol.tsdf, st["tsdf"]) and torch.equal(vol.weight, st["weight"])
    for bad in (dict(st, tsdf=st["tsdf"][:-1]), dict(st, weight=st["weight"].double()),
                {k: v for k, v in st.items() if k != "color"}):
        with pytest.raises(ValueError):
            vol.load_state(bad)
    with pytest.raises(ValueError):
        vol.extract_mesh(float("nan"))


def test_integrate_value_errors(pkg):
    vol = pkg.TSDFVolume((0, 0, 0), 0.1, (3, 4, 5), "cpu")
    cam, small = Cam(8, 6, 0.9, 0.7), Cam(7, 6, 0.9, 0.7)
    d, dv = torch.ones(6, 8), torch.ones(2, 6, 8)
    bad_calls = [
        lambda: vol.integrate(torch.ones(8), cam),                                  # not [H, W] / [V, H, W]
        lambda: vol.integrate(np.ones((6, 8), np.float32), cam),                    # not a tensor
        lambda: vol.integrate(d, [cam]),                                            # a list with [H, W]
        lambda: vol.integrate(dv, cam),                                             # one camera with [V, H, W]
        lambda: vol.integrate(dv, [cam]),                                           # V cameras != V maps
        lambda: vol.integrate(torch.ones(0, 6, 8), []),                             # no view
        lambda: vol.integrate(torch.ones(6, 0), cam),                               # an empty map
        lambda: vol.integrate(d.double(), cam),                                     # dtype
        lambda: vol.integrate(d.to("meta"), cam),                                   # device
        lambda: vol.integrate(d, small),                                            # the camera's size
        lambda: vol.integrate(dv, [cam, small]),
        lambda: vol.integrate(d, cam, alpha=torch.ones(6, 7)),                      # alpha's shape
        lambda: vol.integrate(d, cam, alpha=d.half()),
        lambda: vol.integrate(d, cam, image=torch.ones(6, 8)),                      # image's shape
        lambda: vol.integrate(dv, [cam, cam], image=torch.ones(3, 6, 8)),
        lambda: vol.integrate(d, cam, image=torch.ones(3, 6, 8, dtype=torch.float64)),
        lambda: vol.integrate(d, cam, alpha_min=float("nan")),
        lambda: vol.integrate(d, cam, depth_max=float("nan")),
        lambda: vol.integrate_renders(None, None, [], depth="mean"),
        lambda: vol.integrate_renders(None, None, [], views_per_launch=0),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} raised nothing")
    assert bool((vol.weight == 0).all())


# --------------------------------------------------------------------- PLY ----
@pytest.mark.parametrize("with_colors", [False, True])
def test_save_mesh_ply_round_trips(pkg, tmp_path, with_colors):
    rng = np.random.default_rng(5)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (9, 3)).astype(np.int32)
    c = np.array([[-0.5, 0.0, 0.25], [1.0, 1.5, 0.5], [0.999, 0.001, 0.2]] + [[0.3, 0.6, 0.9]] * 4, np.float32)
    path = tmp_path / "m.ply"
    pkg.save_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c) if with_colors else None)
    rv, rf, rc = TU.read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and rf.dtype == np.int32
    if with_colors:
        assert rc.tolist()[:3] == [[0, 0, 64], [255, 255, 128], [255, 0, 51]]
    else:
        assert rc is None
    pkg.save_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))  # an empty mesh
    rv, rf, _ = TU.read_ply(path)
    assert rv.shape == (0, 3) and rf.shape == (0, 3)
    for bad in (lambda: pkg.save_mesh_ply(path, v[:, :2], f), lambda: pkg.save_mesh_ply(path, v, f.astype(np.float32)),
                lambda: pkg.save_mesh_ply(path, v, f + 7), lambda: pkg.save_mesh_ply(path, v, f, c[:3])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------ the fp64 restatement ----
def test_restatement_on_a_sphere():
    """The sphere's exact signed distance on a 24 x 23 x 22 volume: a closed,
    consistently oriented surface of genus 0 within a voxel of the sphere."""
    R = 0.8
    tsdf, weight, color, origin, h = TU.sphere_volume((24, 23, 22), R)
    v, f, c = TU.extract64(tsdf, weight, color, origin, h)
    assert len(v) > 500 and len(f) == 2 * len(v) - 4
    TU.check_closed_manifold(v, f)
    TU.check_outward(v, f)
    assert np.abs(np.linalg.norm(v, axis=1) - R).max() < h
    # the colour field 0.5 + 0.4 sin(3 p) is smooth: the interpolated colour is the field at the vertex, nearly
    assert np.abs(c - (0.5 + 0.4 * np.sin(3.0 * v))).max() < 0.4 * 3.0 * h
    # vertex ranks follow linear cell order, i fastest; faces linear node order
    cell = np.floor((v - TU.f32(origin)) / float(TU.f32(h)) + 1e-9).astype(np.int64)
    lin = (cell[:, 2] * 22 + cell[:, 1]) * 23 + cell[:, 0]
    assert (np.diff(lin) > 0).all()
    # invalid corners remove their cells, and with them the faces around
    weight[:, :, 12] = 0
    v2, f2, _ = TU.extract64(tsdf, weight, color, origin, h)
    assert 0 < len(v2) < len(v) and len(f2) < len(f)
    cell2 = np.floor((v2 - TU.f32(origin)) / float(TU.f32(h)) + 1e-9).astype(np.int64)
    assert not np.isin(cell2[:, 0], (11, 12)).any()
    uses = TU.edge_uses(f2)
    assert max(uses.values()) == 1 and any((b, a) not in uses for a, b in uses)


def test_restatement_fusion_known_answer():
    """A fronto-parallel wall at depth 3 seen by one camera at the origin
    looking along +z: tsdf = clip((3 - z) / trunc, ., 1) at every node in view,
    weight 1 there, nothing behind the wall by more than trunc."""
    dims, h, origin = (9, 7, 30), 0.1, (-0.4, -0.3, 1.0)
    cam = Cam(33, 25, 0.9, 0.7)  # the identity view
    depth = np.full((1, 25, 33), 3.0, np.float32)
    t, w, c, flagged, counts = TU.integrate64(np.ones((30, 7, 9), np.float32), np.zeros((30, 7, 9), np.float32), None,
                                              origin, h, [cam], depth, None, None, 0.2, 0.4, 0.5, np.inf)
    z = TU.nodes64(origin, h, dims)[..., 2]
    seen = z <= 3.0 + 0.4 + 1e-9
    assert counts["outside_image"] == 0 and counts["behind_near"] == 0
    sure = ~flagged
    assert np.array_equal(w[sure], seen[sure].astype(np.float64))
    assert np.allclose(t[sure & seen], np.minimum(1.0, (3.0 - z) / float(TU.f32(0.4)))[sure & seen], atol=1e-6)
    assert (t[sure & ~seen] == 1).all()
    assert counts["clamped"] > 0 and counts["behind_surface"] > 0
