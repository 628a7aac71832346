"""gs_knn on the device against the fp64 reference and comparison rule of
tests/knn_util.py, at the edges of the box logic (boxes hold 256 points, the
lists 4, 8 or 16 entries), on degenerate extents and density contrasts, and
bit for bit where the definition of the result says so: a second run, a
permutation of the rows, and every distance recomputed on its own pair."""
import functools
import math

import numpy as np
import pytest
import torch

import knn_util as KU
from scene_util import load_scene, write_scene_files

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(points, fp64 reference at k = 16): made once, shared, never written to."""
    pts = KU.GENERATORS[name]() if name in KU.GENERATORS else KU.uniform_cube(int(name[len("uniform"):]))
    pts.setflags(write=False)
    return pts, KU.ref_knn(pts, 16)


def ref_at(name, k):
    pts, (rd, ri) = cloud(name)
    return pts, (rd[:, :k], ri[:, :k])  # (the k smallest of the 16 smallest)


def run(pkg, cuda, pts, k):
    x = torch.tensor(pts, device=cuda)
    d, i = pkg.knn(x, k)
    m = pkg.mean_knn_dist2(x, k)
    assert d.device == i.device == m.device == x.device
    return d.cpu().numpy(), i.cpu().numpy(), m.cpu().numpy()


def check(pkg, cuda, name, k):
    pts, ref = ref_at(name, k)
    d, i, m = run(pkg, cuda, pts, k)
    KU.check_against_ref(pts, k, d, i, m, ref=ref)
    return d, i, m


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 17])
def test_fewer_points_than_neighbours(pkg, cuda, n, k):
    d, i, m = check(pkg, cuda, f"uniform{n}", k)
    found = min(k, n - 1)
    assert np.isposinf(d[:, found:]).all() and (i[:, found:] == -1).all() and np.isfinite(d[:, :found]).all()
    if n == 1:
        assert m.tolist() == [0.0]


@pytest.mark.parametrize("k", [1, 3, 4, 8, 16])
@pytest.mark.parametrize("n", [255, 256, 257, 513, 1000, 5000])
def test_uniform_cube(pkg, cuda, n, k):
    check(pkg, cuda, f"uniform{n}", k)


def test_degenerate_extents(pkg, cuda):
    d, i, m = check(pkg, cuda, "identical", 3)
    assert (d == 0).all() and (m == 0).all()
    d, i, m = check(pkg, cuda, "identical", 16)
    assert (d == 0).all() and (i[0] == np.arange(1, 17)).all() and (i[299] == np.arange(16)).all()
    d, _, m = check(pkg, cuda, "repeated", 3)
    assert (d == 0).all() and (m == 0).all()
    check(pkg, cuda, "on_line", 3)
    check(pkg, cuda, "on_line", 8)
    check(pkg, cuda, "on_plane", 3)
    check(pkg, cuda, "on_plane", 16)


@pytest.mark.parametrize("k", [3, 8])
def test_density_contrast(pkg, cuda, k):
    d, i, _ = check(pkg, cuda, "clusters", k)
    pts, _ = cloud("clusters")
    far = np.abs(pts).max(1) > 1e3  # the five outliers: their neighbours are far away too
    assert far.sum() == 5 and (d[far, 0] > 9e7).all() and (d[~far] < 1.0).all()


def test_offset_cloud(pkg, cuda):
    check(pkg, cuda, "offset", 3)
    check(pkg, cuda, "offset", 8)


def test_closed_forms_exact(pkg, cuda):
    d, i, m = run(pkg, cuda, KU.lattice(), 3)
    assert (d == np.float32(0.0625)).all() and (m == np.float32(0.0625)).all() and i[0].tolist() == [1, 10, 100]
    d, i, m = run(pkg, cuda, KU.line(), 3)
    want_d, want_i = KU.line_expected()
    assert np.array_equal(d, want_d) and np.array_equal(i, want_i)
    n = 700  # a line across three boxes: the tie rule across box borders
    d, i, _ = run(pkg, cuda, KU.line(n), 3)
    want_d, want_i = KU.line_expected(n)
    assert np.array_equal(d, want_d) and np.array_equal(i, want_i)


def test_lattice_of_290_boxes(pkg, cuda):
    """42^3 points, 290 boxes: the sweep over the boxes takes a second round of
    256.  Closed form: three neighbours at exactly one spacing, and of the up
    to six at that distance the three smallest rows; the same distances, bit
    for bit, when the rows are shuffled."""
    side = 42
    pts = KU.lattice(side)
    n = len(pts)
    d, i, m = run(pkg, cuda, pts, 3)
    assert (d == np.float32(0.0625)).all() and (m == np.float32(0.0625)).all()
    ix, iy, iz = np.unravel_index(np.arange(n), (side, side, side))
    cand = np.stack([np.where(ix > 0, np.arange(n) - side * side, n), np.where(iy > 0, np.arange(n) - side, n),
                     np.where(iz > 0, np.arange(n) - 1, n), np.where(iz < side - 1, np.arange(n) + 1, n),
                     np.where(iy < side - 1, np.arange(n) + side, n),
                     np.where(ix < side - 1, np.arange(n) + side * side, n)], 1)  # (ascending; n: no such neighbour)
    assert np.array_equal(i, np.sort(cand, 1)[:, :3].astype(np.int32))
    perm = np.random.default_rng(4).permutation(n)
    dp, ip, _ = run(pkg, cuda, pts[perm], 3)
    assert (dp == np.float32(0.0625)).all()
    own = ((pts[perm].astype(np.float64)[:, None, :] - pts[perm].astype(np.float64)[ip]) ** 2).sum(-1)
    assert (own == 0.0625).all() and (ip != np.arange(n)[:, None]).all()


def test_same_bits_every_run(pkg, cuda):
    for name, k in (("uniform5000", 8), ("clusters", 3)):
        pts, _ = cloud(name)
        a, b = run(pkg, cuda, pts, k), run(pkg, cuda, pts, k)
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.int32), v.view(np.int32))


@pytest.mark.parametrize("name,k", [("uniform5000", 3), ("uniform5000", 16), ("lattice", 3), ("lattice", 8)])
def test_same_bits_under_row_permutation(pkg, cuda, name, k):
    """The definition does not know the input order: the distances of a point
    are the same bits wherever its row and its neighbours' rows stand."""
    pts = KU.lattice() if name == "lattice" else cloud(name)[0]
    perm = np.random.default_rng(9).permutation(len(pts))
    d, _, m = run(pkg, cuda, pts, k)
    dp, _, mp = run(pkg, cuda, pts[perm], k)
    assert np.array_equal(dp.view(np.int32), d[perm].view(np.int32))
    assert np.array_equal(mp.view(np.int32), m[perm].view(np.int32))


def test_one_distance_function(pkg, cuda):
    """Every returned (i, j, d): the search of the two-point cloud {p_j, p_i}
    gives d bit for bit -- culls and lists compute distances nowhere else."""
    pts, _ = cloud("uniform257")
    d, idx, _ = run(pkg, cuda, pts, 3)
    x = torch.tensor(pts, device=cuda)
    pairs = []
    for i in range(len(pts)):
        for s in range(3):
            pairs.append(pkg.knn(x[[int(idx[i, s]), i]], 1, return_index=False)[0])
    got = torch.stack(pairs).cpu().numpy()  # [n * 3, 2, 1]
    want = np.repeat(d.reshape(-1), 2).reshape(-1, 2, 1)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_device_and_cpu_paths_agree(pkg, cuda):
    """Both are within 5 * 2^-24 of the fp64 distances, so within RTOL of each other."""
    for name, k in (("uniform1000", 8), ("clusters", 3), ("repeated", 3)):
        pts, _ = cloud(name)
        d, i, m = run(pkg, cuda, pts, k)
        dc, ic = pkg.knn(torch.tensor(pts), k)
        mc = pkg.mean_knn_dist2(torch.tensor(pts), k)
        np.testing.assert_allclose(d, dc.numpy(), rtol=KU.RTOL, atol=0)
        np.testing.assert_allclose(m, mc.numpy(), rtol=KU.RTOL + (k + 1) * 2.0 ** -24, atol=0)
        KU.check_against_ref(pts, k, dc.numpy(), ic.numpy())


def test_create_from_points_on_the_device(pkg, cuda):
    pts, _ = cloud("clusters")
    torch.manual_seed(3)
    dev_model, cpu_model = pkg.GaussianModel(), pkg.GaussianModel()
    dev_model.create_from_points(torch.tensor(pts, device=cuda), scale_init="knn")
    cpu_model.create_from_points(torch.tensor(pts), scale_init="knn")
    s_dev, s_cpu = dev_model._scaling.detach().cpu().numpy(), cpu_model._scaling.detach().numpy()
    assert dev_model._scaling.device.type == "cuda" and s_dev.shape == (len(pts), 3) and np.isfinite(s_dev).all()
    # rtol 1e-6 on the squared distances is 0.5e-6 absolute on log sqrt; sqrt and log round in fp32 on both sides
    atol = 0.5 * KU.RTOL + 8 * 2.0 ** -24 * max(1.0, float(np.abs(s_cpu).max()))
    np.testing.assert_allclose(s_dev, s_cpu, rtol=0, atol=atol)
    want = np.log(np.sqrt(np.maximum(KU.ref_mean(pts, 3), 1e-7)))
    np.testing.assert_allclose(s_dev[:, 0], want, rtol=0, atol=atol + 0.5 * 4 * 2.0 ** -24)


# ------------------------------------------------------------------ trainer ----
@pytest.fixture(scope="module")
def scene(pkg, cuda, tmp_path_factory):
    root = tmp_path_factory.mktemp("knn_scene")
    write_scene_files(root, 8, 64)
    return root, load_scene(pkg, root, cuda, 64, split=False)


def _config(pkg, out, **kw):
    return pkg.TrainingConfig(iterations=6, densify_from_iter=100, densify_until_iter=100, num_random_points=2000,
                              log_interval=1, output_path=str(out), position_lr_init=1.6e-3, position_lr_final=1.6e-5,
                              **kw)


def test_trainer_scale_init(pkg, cuda, scene):
    root, ds = scene
    tr = pkg.GaussianTrainer(_config(pkg, root / "default"), ds)
    tr.setup()
    # the default: the scales it has always started with, bit for bit
    assert torch.equal(tr.gaussians._scaling.detach().cpu(), torch.full((2000, 3), math.log(0.02 * 1.3)))
    start = [p.detach().clone() for p in tr.gaussians.parameter_list()]

    tk = pkg.GaussianTrainer(_config(pkg, root / "knn", scale_init="knn"), ds)
    tk.setup()
    for name, a, b in zip(("xyz", "dc", "rest", "scaling", "rotation", "opacity"), start, tk.gaussians.parameter_list()):
        assert torch.equal(a, b.detach()) == (name != "scaling"), name
    xyz = tk.gaussians._xyz.detach().cpu().numpy()
    want = np.log(np.sqrt(np.maximum(KU.ref_mean(xyz, 3), 1e-7)))
    got = tk.gaussians._scaling.detach().cpu().numpy()
    assert (got[:, :1] == got).all()
    np.testing.assert_allclose(got[:, 0], want, rtol=0, atol=0.5 * KU.RTOL + 8 * 2.0 ** -24 * float(np.abs(want).max()))
    for _ in range(6):
        tk.train(1)
    torch.cuda.synchronize()
    assert len(tk.train_losses) == 6 and all(math.isfinite(v) for v in tk.train_losses)
    for p in tk.gaussians.parameter_list():
        assert bool(torch.isfinite(p).all())
