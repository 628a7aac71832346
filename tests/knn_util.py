"""The independent reference of the k-NN tests, their input generators and the
comparison rule (tests/test_knn_cpu.py, tests/test_knn_gpu.py).

Reference: numpy fp64 brute force, chunked, on the fp32 inputs widened to
fp64; ties broken by index; ascending dist2 and index, +inf / -1 padding.

Comparison rule.  The fp32 d2 under test, ((dx dx) + (dy dy)) + (dz dz),
differs from the fp64 value by at most five roundings (one per difference, one
per square, two for the sums; every term is non-negative, so nothing cancels
after the differences): a relative error <= 5 * 2^-24 ~ 3e-7.  Sorted distance
rows are compared with rtol = 1e-6 (three times that) and atol = 0.  A
near-tie that resolves differently in fp32 changes which neighbour is taken
but moves the sorted distances by no more than the same rounding, so indices
are not compared to the reference's: each must be in range, differ from its
row, be distinct within its row and reproduce its own dist2 in fp64 to the
same rtol.  The generators keep every non-zero separation >= 1e-4, so nothing
underflows; exact duplicates give exactly 0 on both sides."""
import numpy as np

RTOL = 1e-6


def ref_knn(points, k, chunk_elems=1 << 22):
    """(dist2 [n, k] float64 ascending, index [n, k] int64) by fp64 brute force."""
    p = np.ascontiguousarray(points, dtype=np.float32).astype(np.float64)
    n = len(p)
    dist2 = np.full((n, k), np.inf)
    index = np.full((n, k), -1, np.int64)
    m = min(k, n - 1)
    if m <= 0:
        return dist2, index
    step = max(1, chunk_elems // n)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        diff = p[r0:r1, None, :] - p[None, :, :]
        d = diff[..., 0] ** 2 + diff[..., 1] ** 2 + diff[..., 2] ** 2
        d[np.arange(r1 - r0), np.arange(r0, r1)] = np.inf  # not its own neighbour
        order = np.argsort(d, axis=1, kind="stable")[:, :m]  # stable: equal distances by index
        dist2[r0:r1, :m] = np.take_along_axis(d, order, 1)
        index[r0:r1, :m] = order
    return dist2, index


def ref_mean(points, k):
    """The mean of the min(k, n - 1) reference distances (0 when n == 1)."""
    n = len(points)
    m = min(k, n - 1)
    if m <= 0:
        return np.zeros(n)
    return ref_knn(points, k)[0][:, :m].mean(1)


def check_against_ref(points, k, dist2, index=None, mean=None, ref=None):
    """The comparison rule, on numpy arrays of a result for `points`."""
    p32 = np.ascontiguousarray(points, dtype=np.float32)
    p = p32.astype(np.float64)
    n = len(p)
    rd, _ = ref if ref is not None else ref_knn(p32, k)
    m = max(min(k, n - 1), 0)
    dist2 = np.asarray(dist2)
    assert dist2.shape == (n, k) and dist2.dtype == np.float32
    assert np.isposinf(dist2[:, m:]).all(), "padding must be +inf"
    np.testing.assert_allclose(dist2[:, :m].astype(np.float64), rd[:, :m], rtol=RTOL, atol=0)
    assert (np.diff(dist2[:, :m].astype(np.float64), axis=1) >= 0).all(), "rows must ascend"
    if index is not None:
        index = np.asarray(index)
        assert index.shape == (n, k) and index.dtype == np.int32
        assert (index[:, m:] == -1).all(), "padding must be -1"
        idx = index[:, :m].astype(np.int64)
        assert ((idx >= 0) & (idx < n)).all()
        assert (idx != np.arange(n)[:, None]).all(), "a point is not its own neighbour"
        srt = np.sort(idx, axis=1)
        assert (np.diff(srt, axis=1) > 0).all(), "indices must be distinct within a row"
        own = ((p[:, None, :] - p[idx]) ** 2).sum(-1) if m else np.zeros((n, 0))
        np.testing.assert_allclose(dist2[:, :m].astype(np.float64), own, rtol=RTOL, atol=0)
    if mean is not None:
        mean = np.asarray(mean)
        assert mean.shape == (n,) and mean.dtype == np.float32
        want = rd[:, :m].mean(1) if m else np.zeros(n)
        # the m distances within RTOL each, plus m roundings of the fp32 sum and division
        np.testing.assert_allclose(mean.astype(np.float64), want, rtol=RTOL + (m + 1) * 2.0 ** -24, atol=0)


# ------------------------------------------------------------ generators ----
# Every coordinate is a multiple of a grid step >= 1e-4 (distinct points are
# then >= 1e-4 apart on some axis), or an exact duplicate.
def _snap(x, step):
    return (np.round(np.asarray(x, np.float64) / step) * step).astype(np.float32)


def uniform_cube(n, seed=0):
    return _snap(np.random.default_rng(seed).uniform(-1, 1, (n, 3)), 1e-3 if n <= 1000 else 2.5e-4)


def identical(n=300):
    return np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (n, 1))


def repeated(n=250, times=4, seed=1):
    return np.repeat(uniform_cube(n, seed), times, axis=0)


def on_line(n=500, seed=2):
    t = _snap(np.random.default_rng(seed).uniform(-4, 4, n), 1e-3)
    return np.stack([t, np.full(n, 0.5, np.float32), np.full(n, -2.0, np.float32)], 1).astype(np.float32)


def on_plane(n=900, seed=3):
    xy = _snap(np.random.default_rng(seed).uniform(-2, 2, (n, 2)), 1e-3)
    return np.concatenate([xy, np.full((n, 1), 7.0, np.float32)], 1).astype(np.float32)


def clusters(n_each=600, seed=4):
    """Two clusters of sigma 0.01, 100 apart, and five outliers at distance 1e4."""
    rng = np.random.default_rng(seed)
    a = _snap(rng.normal(0, 0.01, (n_each, 3)), 1e-4)
    b = _snap(rng.normal(0, 0.01, (n_each, 3)), 1e-4) + np.array([100, 0, 0], np.float32)
    out = np.array([[1e4, 0, 0], [-1e4, 0, 0], [0, 1e4, 0], [0, -1e4, 0], [0, 0, 1e4]], np.float32)
    pts = np.concatenate([a, b, out]).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def offset_cloud(n=2000, seed=5):
    """Spacing ~0.01 around (1e4, 1e4, 1e4): multiples of 2^-7 (exact in fp32 there)."""
    rng = np.random.default_rng(seed)
    return (np.float32(1e4) + rng.integers(-64, 64, (n, 3)).astype(np.float32) * np.float32(2.0 ** -7)).astype(np.float32)


def lattice(side=10, spacing=0.25):
    g = np.arange(side, dtype=np.float32) * np.float32(spacing)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def line(n=40, spacing=0.5):
    return np.stack([np.arange(n, dtype=np.float32) * np.float32(spacing), np.zeros(n, np.float32),
                     np.zeros(n, np.float32)], 1)


def line_expected(n=40):
    """k = 3 on line(): the rows the tie rule gives (spacing 0.5)."""
    d = np.tile(np.array([0.25, 0.25, 1.0], np.float32), (n, 1))
    i = np.arange(n)
    idx = np.stack([i - 1, i + 1, i - 2], 1)
    d[0], idx[0] = (0.25, 1.0, 2.25), (1, 2, 3)
    d[n - 1], idx[n - 1] = (0.25, 1.0, 2.25), (n - 2, n - 3, n - 4)
    idx[1] = (0, 2, 3)  # 0.25, 0.25, then 1.0 only at row 3
    idx[n - 2] = (n - 3, n - 1, n - 4)
    return d, idx.astype(np.int32)


GENERATORS = {
    "identical": identical, "repeated": repeated, "on_line": on_line, "on_plane": on_plane,
    "clusters": clusters, "offset": offset_cloud,
}
