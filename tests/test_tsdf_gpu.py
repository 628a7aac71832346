"""TSDF fusion and mesh extraction on the GPU (gs_tsdf_integrate,
gs_mesh_classify, gs_mesh_emit; tsdf.py; GaussianTrainer.extract_mesh).

The fusion against its fp64 statement (tests/tsdf_util.py) on the same fp32
inputs: the nodes one of whose decisions is within rounding are left out (at
most 2 % of a case), every other node agrees exactly on which views updated
it, and tsdf / colour agree at four times the deviation measured on the
MI355X, never above 1e-5.  The extraction against its statement: faces
exactly, vertices and colours at the same rule.  End to end: rendered depth
maps of a sphere of Gaussians to a mesh, and the trainer's PLY."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import tsdf_util as TU
from stubs import Cam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_bits = lambda t: t.detach().contiguous().view(torch.int32)
_np = lambda t: t.detach().cpu().numpy()
_dev = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

# Four times the largest deviation from the fp64 statement measured on the
# MI355X over every case of this file (the measurement in brackets), never
# above CAP = 1e-5.
CAP = 1e-5
TOL_TSDF = 4 * 1.32e-6          # absolute, tsdf in [-1, 1] [1.32e-6 at 257 x 2 x 2; 6.44e-7 end to end]
TOL_COLOR = 4 * 1.09e-7         # absolute, colours in [0, 1] [1.09e-7 at 37 x 21 x 10]
TOL_VERTEX = 4 * 1.60e-7        # relative to the largest coordinate in the volume [1.60e-7 end to end, median depth]
TOL_VERTEX_COLOR = 4 * 1.25e-7  # absolute, colours in [0.1, 0.9] [1.25e-7 at 40 x 33 x 29]
assert max(TOL_TSDF, TOL_COLOR, TOL_VERTEX, TOL_VERTEX_COLOR) <= CAP
MAX_FLAGGED = 0.02

ORIGIN, H_VOXEL, NEAR, ALPHA_MIN = (-2.0, -1.2, -0.5), 0.11, 0.2, 0.5
FUSION_DIMS = [(37, 21, 10), (64, 3, 5), (1, 1, 1), (257, 2, 2)]  # 257: past the 256th node of a row, a block one node wide
_CASES = {}


def fusion_reference(dims):
    """The case of `dims` and its fp64 result from a fresh volume, computed once."""
    if dims not in _CASES:
        cams, depth, alpha, image, depth_max = TU.fusion_case(dims, 7 + dims[0], H_VOXEL, ORIGIN)
        nx, ny, nz = dims
        want = TU.integrate64(np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32),
                              np.zeros((3, nz, ny, nx), np.float32), ORIGIN, H_VOXEL, cams, depth, alpha, image, NEAR,
                              4 * H_VOXEL, ALPHA_MIN, depth_max)
        for a in want[:4]:
            a.setflags(write=False)
        _CASES[dims] = (cams, depth, alpha, image, depth_max, want)
    return _CASES[dims]


def _volume(pkg, dev, dims, **kw):
    return pkg.TSDFVolume(ORIGIN, H_VOXEL, dims, dev, near=NEAR, **kw)


# ------------------------------------------------------------------ fusion ----
@pytest.mark.parametrize("dims", FUSION_DIMS)
def test_fusion_against_fp64(pkg, cuda, dims):
    cams, depth, alpha, image, depth_max, (t64, w64, c64, flagged, counts) = fusion_reference(dims)
    print(f"  {dims}: {len(cams)} views, branches {counts}, flagged {flagged.mean():.4%}")
    for name in TU.BRANCHES:
        assert counts[name] > 0, f"no node takes the branch {name}"
    assert flagged.mean() <= MAX_FLAGGED
    vol = _volume(pkg, cuda, dims)
    vol.integrate(_dev(depth, cuda), cams, alpha=_dev(alpha, cuda), image=_dev(image, cuda), alpha_min=ALPHA_MIN,
                  depth_max=depth_max)
    torch.cuda.synchronize()
    sure = ~flagged
    w = _np(vol.weight)
    assert np.array_equal(w[sure].astype(np.float64), w64[sure]), "a view updated a node it should not, or missed one"
    e_t = np.abs(_np(vol.tsdf).astype(np.float64) - t64)[sure].max()
    e_c = np.abs(_np(vol.color).astype(np.float64) - c64)[:, sure].max()
    print(f"  {dims}: tsdf max err {e_t:.3g}, colour max err {e_c:.3g}, weights up to {w.max():.0f}")
    assert e_t <= TOL_TSDF and e_c <= TOL_COLOR
    # untouched nodes are the initial state exactly
    idle = sure & (w64 == 0)
    assert (_np(vol.tsdf)[idle] == 1).all() and (_np(vol.color)[:, idle] == 0).all()


def test_batched_launch_equals_single_views(pkg, cuda):
    """One launch of 5 views gives the bits of 5 launches of one view each, and a second run the same bits."""
    dims = FUSION_DIMS[0]
    cams, depth, alpha, image, depth_max, _ = fusion_reference(dims)
    order = [0, 1, 2, 8, 7]  # two outside views, the inside one, and two constant maps (updating, clamped)
    cams = [cams[i] for i in order]
    d, a, im = (_dev(x[order], cuda) for x in (depth, alpha, image))
    vols = [_volume(pkg, cuda, dims) for _ in range(3)]
    for vol in vols[:2]:
        vol.integrate(d, cams, alpha=a, image=im, depth_max=depth_max)
    for v in range(5):
        vols[2].integrate(d[v], cams[v], alpha=a[v], image=im[v], depth_max=depth_max)
    torch.cuda.synchronize()
    assert float(vols[0].weight.max()) >= 3
    for other in vols[1:]:
        for name in ("tsdf", "weight", "color"):
            assert torch.equal(_bits(getattr(vols[0], name)), _bits(getattr(other, name))), name


def test_untouched_nodes_keep_their_bits(pkg, cuda):
    """A volume filled with sentinel bit patterns (NaNs with payloads among
    them) keeps them at every node no view updates."""
    dims = FUSION_DIMS[0]
    cams, depth, alpha, image, depth_max, (_, w64, _, flagged, _) = fusion_reference(dims)
    vol = _volume(pkg, cuda, dims)
    n = vol.tsdf.numel()
    pattern = lambda seed, count: ((torch.arange(count, dtype=torch.int64) * 2654435761 + seed) % (1 << 32)).to(torch.int32)
    sent = {"tsdf": pattern(1, n) | 0x7FC00000, "weight": pattern(2, n), "color": pattern(3, 3 * n) | 0x7F800001}
    for name, bits in sent.items():
        getattr(vol, name).view(torch.int32).copy_(bits.view(getattr(vol, name).shape).to(cuda))
    vol.integrate(_dev(depth, cuda), cams, alpha=_dev(alpha, cuda), image=_dev(image, cuda), depth_max=depth_max)
    torch.cuda.synchronize()
    idle = torch.from_numpy((~flagged) & (w64 == 0))
    touched = torch.from_numpy((~flagged) & (w64 > 0))
    assert int(idle.sum()) > 100 and int(touched.sum()) > 100
    for name, bits in sent.items():
        got, want = _bits(getattr(vol, name)).cpu(), bits.view(getattr(vol, name).shape)
        assert torch.equal(got[..., idle], want[..., idle]), name
    assert not torch.equal(_bits(vol.weight).cpu()[touched], sent["weight"].view(vol.weight.shape)[touched])


def test_single_view_without_alpha_image_or_colour(pkg, cuda):
    dims = FUSION_DIMS[0]
    cams, depth, _, _, _, _ = fusion_reference(dims)
    nx, ny, nz = dims
    t64, w64, _, flagged, counts = TU.integrate64(np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32),
                                                  None, ORIGIN, H_VOXEL, cams[:1], depth[:1], None, None, NEAR,
                                                  4 * H_VOXEL, ALPHA_MIN, np.inf)
    assert counts["updated"] > 100 and flagged.mean() <= MAX_FLAGGED
    vol = _volume(pkg, cuda, dims, color=False)
    vol.integrate(_dev(depth[0], cuda), cams[0])
    torch.cuda.synchronize()
    sure = ~flagged
    assert vol.color is None
    assert np.array_equal(_np(vol.weight)[sure].astype(np.float64), w64[sure])
    e_t = np.abs(_np(vol.tsdf).astype(np.float64) - t64)[sure].max()
    print(f"  one view: tsdf max err {e_t:.3g}")
    assert e_t <= TOL_TSDF
    # a colour volume without an image keeps its colours; an image without a colour volume is ignored
    vol2 = _volume(pkg, cuda, dims)
    vol2.integrate(_dev(depth[0], cuda), cams[0])
    assert torch.equal(_bits(vol2.tsdf), _bits(vol.tsdf)) and bool((vol2.color == 0).all())


# -------------------------------------------------------------- extraction ----
MESH_DIMS = [(24, 23, 22), (40, 33, 29)]  # the second: more vertices and faces than one block
_SPHERES = {}


def sphere_reference(dims):
    if dims not in _SPHERES:
        tsdf, weight, color, origin, h = TU.sphere_volume(dims, 0.8)
        want = TU.extract64(tsdf, weight, color, origin, h)
        _SPHERES[dims] = (tsdf, weight, color, origin, h, want)
    return _SPHERES[dims]


def _load(pkg, dev, tsdf, weight, color, origin, h):
    nz, ny, nx = tsdf.shape
    vol = pkg.TSDFVolume(origin, h, (nx, ny, nz), dev, color=color is not None)
    vol.load_state({k: _dev(v, dev) for k, v in (("tsdf", tsdf), ("weight", weight), ("color", color)) if v is not None})
    return vol


def _extent(origin, h, dims):
    return max(max(abs(o), abs(o + h * (n - 1))) for o, n in zip(origin, dims))


@pytest.mark.parametrize("dims", MESH_DIMS)
def test_extraction_against_fp64(pkg, cuda, dims):
    tsdf, weight, color, origin, h, (v64, f64, c64) = sphere_reference(dims)
    vol = _load(pkg, cuda, tsdf, weight, color, origin, h)
    mesh = vol.extract_mesh()
    torch.cuda.synchronize()
    v, f, c = _np(mesh["vertices"]), _np(mesh["faces"]), _np(mesh["colors"])
    assert mesh["faces"].dtype == torch.int32 and v.shape == v64.shape and c.shape == c64.shape
    if dims == MESH_DIMS[1]:
        assert len(v) > 2 * 256 and len(f) > 2 * 256
    assert np.array_equal(f, f64)
    e_v = np.abs(v.astype(np.float64) - v64).max() / _extent(origin, h, dims)
    e_c = np.abs(c.astype(np.float64) - c64).max()
    print(f"  {dims}: {len(v)} vertices, {len(f)} faces, vertex max err {e_v:.3g} of the extent, colour {e_c:.3g}")
    assert e_v <= TOL_VERTEX and e_c <= TOL_VERTEX_COLOR
    TU.check_closed_manifold(v, f)
    TU.check_outward(v, f)
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.8).max() < h
    again = vol.extract_mesh()
    for name in ("vertices", "faces", "colors"):
        assert torch.equal(_bits(mesh[name]), _bits(again[name])), name
    # without a colour volume: the same geometry, no colours
    bare = _load(pkg, cuda, tsdf, weight, None, origin, h).extract_mesh()
    assert bare["colors"] is None
    assert torch.equal(_bits(bare["vertices"]), _bits(mesh["vertices"])) and torch.equal(bare["faces"], mesh["faces"])


def test_unobserved_slab_opens_the_mesh(pkg, cuda):
    dims = MESH_DIMS[0]
    tsdf, weight, color, origin, h, _ = sphere_reference(dims)
    weight = weight.copy()
    weight[:, 9:11, :] = 0  # nodes j = 9, 10: the cells j = 8 .. 10 touch them
    vol = _load(pkg, cuda, tsdf, weight, color, origin, h)
    mesh = vol.extract_mesh()
    v, f = _np(mesh["vertices"]).astype(np.float64), _np(mesh["faces"])
    v64, f64, _ = TU.extract64(tsdf, weight, color, origin, h)
    assert np.array_equal(f, f64) and len(v) == len(v64) and len(f) > 0
    cell_j = np.floor((v[:, 1] - float(TU.f32(origin[1]))) / float(TU.f32(h)) + 1e-6).astype(np.int64)
    assert not np.isin(cell_j, (8, 9, 10)).any()
    uses = TU.edge_uses(f)
    assert max(uses.values()) == 1, "an edge used twice in one direction"
    boundary = [e for e in uses if (e[1], e[0]) not in uses]
    assert len(boundary) > 0 and all(uses[e] == 1 for e in boundary)
    undirected = {}
    for (a, b), n in uses.items():
        undirected[(min(a, b), max(a, b))] = undirected.get((min(a, b), max(a, b)), 0) + n
    assert max(undirected.values()) <= 2
    # a larger min_weight than any node has: nothing
    assert vol.extract_mesh(min_weight=2.0)["vertices"].shape == (0, 3)


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 9, 9), (33, 1, 5), (40, 9, 1), (12, 11, 10)])
def test_empty_meshes(pkg, cuda, dims):
    """Thin volumes have no cell, an all-positive one no crossing: [0, 3] arrays."""
    nx, ny, nz = dims
    vol = pkg.TSDFVolume((0, 0, 0), 0.1, dims, cuda)
    vol.weight.fill_(3.0)
    if min(dims) == 1:  # (thin: even with a sign change)
        vol.tsdf.view(-1)[::2] = -0.5
    mesh = vol.extract_mesh()
    assert mesh["vertices"].shape == (0, 3) and mesh["faces"].shape == (0, 3) and mesh["colors"].shape == (0, 3)
    assert mesh["faces"].dtype == torch.int32 and mesh["vertices"].device == vol.device


# -------------------------------------------------------------- end to end ----
def sphere_scene(pkg, dev, n=2000):
    """About 2000 flat opaque Gaussians on the unit sphere, their thin axis radial."""
    g = torch.Generator().manual_seed(11)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    # the rotation taking e_z to d: axis e_z x d = (-dy, dx, 0), q = (1 + dz, axis)
    q = torch.nn.functional.normalize(torch.stack([1 + d[:, 2], -d[:, 1], d[:, 0], torch.zeros(n)], 1), dim=1)
    model = pkg.GaussianModel()
    model._set(d.to(dev), (d.reshape(n, 1, 3) * 1.5).to(dev), torch.zeros(n, 15, 3, device=dev),
               torch.log(torch.tensor([0.06, 0.06, 0.004])).expand(n, 3).contiguous().to(dev), q.to(dev),
               torch.full((n, 1), 6.0).to(dev))
    return model


def axis_cameras(size=64, distance=4.0):
    eyes = [(distance, 0, 0), (-distance, 0, 0), (0, distance, 0), (0, -distance, 0), (0, 0, distance), (0, 0, -distance)]
    return [Cam(size, size, 0.7, 0.7, TU.look_at_view(e)) for e in eyes]


# mean | |v| - 1 | of the extracted sphere, measured on the MI355X (examples/extract_mesh.py prints it): 0.0406
# with the median depth, 0.0537 with the expected depth -- 0.41 and 0.54 voxels, the latter above half a voxel:
# the expected depth mixes the sphere's front and back along the silhouette.  The bound is four times the
# measurement and never above one voxel: one voxel for both.
E2E_VOXEL = 0.1
E2E_BOUND = {"median": min(4 * 0.0406, E2E_VOXEL), "expected": min(4 * 0.0537, E2E_VOXEL)}


@pytest.mark.parametrize("depth", ["median", "expected"])
def test_renders_to_mesh(pkg, cuda, depth):
    model, cams = sphere_scene(pkg, cuda), axis_cameras()
    renderer = pkg.GaussianRenderer()
    vol = pkg.TSDFVolume.from_bounds((-1.3,) * 3, (1.3,) * 3, E2E_VOXEL, cuda)
    assert vol.dims == (27, 27, 27)
    vol.integrate_renders(renderer, model, cams, depth=depth, views_per_launch=4)
    mesh = vol.extract_mesh()
    # the same maps, downloaded, through the statement
    maps = []
    with torch.no_grad():
        for cam in cams:
            out = renderer.render(cam, model, pkg.RenderSettings(64, 64, torch.zeros(3)), depth_distortion=depth == "median")
            maps.append([_np(out["median_depth" if depth == "median" else "depth"]).reshape(64, 64),
                         _np(out["alpha"]).reshape(64, 64), _np(out["image"])])
    d, a, im = (np.stack([m[k] for m in maps]).astype(np.float32) for k in range(3))
    t64, w64, c64, flagged, counts = TU.integrate64(np.ones((27,) * 3, np.float32), np.zeros((27,) * 3, np.float32),
                                                    np.zeros((3, 27, 27, 27), np.float32), vol.origin, E2E_VOXEL, cams,
                                                    d, a, im, vol.near, vol.trunc, 0.5, np.inf)
    sure = ~flagged
    assert flagged.mean() <= MAX_FLAGGED and counts["updated"] > 1000 and counts["low_alpha"] > 0
    assert np.array_equal(_np(vol.weight)[sure].astype(np.float64), w64[sure])
    e_t = np.abs(_np(vol.tsdf).astype(np.float64) - t64)[sure].max()
    e_c = np.abs(_np(vol.color).astype(np.float64) - c64)[:, sure].max()
    v64, f64, c64v = TU.extract64(_np(vol.tsdf), _np(vol.weight), _np(vol.color), vol.origin, E2E_VOXEL)
    v, f = _np(mesh["vertices"]).astype(np.float64), _np(mesh["faces"])
    assert np.array_equal(f, f64) and len(f) > 500
    e_v = np.abs(v - v64).max() / 1.3
    e_vc = np.abs(_np(mesh["colors"]).astype(np.float64) - c64v).max()
    off = np.abs(np.linalg.norm(v, axis=1) - 1.0)
    print(f"  {depth}: flagged {flagged.mean():.3%}, tsdf err {e_t:.3g}, colour err {e_c:.3g}, vertex err {e_v:.3g}, "
          f"vertex colour err {e_vc:.3g}; {len(v)} vertices, {len(f)} faces, mean ||v| - 1| = {off.mean():.4f} "
          f"(max {off.max():.4f}) at voxel {E2E_VOXEL}")
    assert e_t <= TOL_TSDF and e_c <= TOL_COLOR and e_v <= TOL_VERTEX and e_vc <= TOL_VERTEX_COLOR
    assert off.mean() <= E2E_BOUND[depth] <= E2E_VOXEL


def test_trainer_extract_mesh_writes_ply(pkg, cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_synthetic as ts
    ds = ts.build_scene(pkg, views=8, size=64, gt_gaussians=2000, device=cuda)
    tr = ts.make_trainer(pkg, ds, iters=4)
    before = [p.detach().clone() for p in (tr.gaussians._xyz, tr.gaussians._opacity)]
    path = tmp_path / "mesh.ply"
    mesh = tr.extract_mesh(voxel_size=0.1, path=str(path))
    v, f, c = TU.read_ply(path)
    assert len(v) == mesh["vertices"].shape[0] > 0 and len(f) == mesh["faces"].shape[0] > 0 and c.shape == v.shape
    assert np.array_equal(v, _np(mesh["vertices"])) and np.array_equal(f, _np(mesh["faces"]))
    assert f.max() < len(v) and f.min() >= 0
    for p, q in zip(before, (tr.gaussians._xyz, tr.gaussians._opacity)):
        assert torch.equal(p, q)
    # bounds, the expected depth and a camera subset; no file without a path
    cams = tr.dataset.get_train_cameras()[:2]
    small = tr.extract_mesh(voxel_size=0.2, bounds=((-1, -1, -1), (1, 1, 1)), depth="expected", cameras=cams)
    assert small["vertices"].shape[1] == 3 and small["faces"].dtype == torch.int32
    for bad in ((0, 1), ((0, 0, 0),), ((0, 0, 0), (1, 1))):
        with pytest.raises(ValueError):
            tr.extract_mesh(bounds=bad)
