"""gs_gather_partials alone, through the C ABI: every instantiation of
k_gather_slots (<1,4>, <2,2>, <4,2,4>, the generic <4,2> with one, two and
three passes over a slot's groups and a remainder, and the walk in `order`)
on synthetic slots.  Partials are integers in [-8, 8], so every sum is exact
in fp32 in any order and the expectation -- a plain numpy sum over the live
flags -- is compared for equality.  Dead partials and a guard region after
the last slot hold NaN: a partial read that should not be shows in the sum.
Below, the order of the sums itself: the four gather entry points against a
numpy statement of the walk, bit for bit, on float partials."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GS_ERR_UNSUPPORTED = 3
TOUCHES = list(range(14)) + [24, 25, 97, 300]  # across kGatherNB * HL = 6 (two slot lanes) and 12 (four)
SIZES = (1, 31, 32, 33, 64, 65, 257, 1000)
GUARD = 64  # slots after the last one, inside the allocation: flags 1, partials NaN


def make_case(rng, n, ng, integer=True):
    touches = rng.choice(TOUCHES, n)
    full = n > len(TOUCHES)
    if full:  # every count present
        touches[:len(TOUCHES)] = TOUCHES
        touches = rng.permutation(touches)
    vis = np.ones(n, np.uint8)
    hidden = (rng.random(n) < 0.1) & (touches != 300)  # culled, with a rectangle all the same: no slot, a zero row
    if full:
        hidden[np.nonzero(touches == 5)[0][0]] = True
    vis[hidden] = 0
    rects = np.empty((n, 2), np.uint32)
    for g, t in enumerate(touches):
        if t == 0:
            rects[g] = (1, 1)  # the empty rectangle: tx0 = 1 > tx1 = 0
            continue
        w = int(rng.choice([d for d in range(1, t + 1) if t % d == 0 and d <= 256]))
        h = t // w
        x0, y0 = int(rng.integers(0, 200)), int(rng.integers(0, 200))
        rects[g] = (x0 | ((x0 + w - 1) << 16), y0 | ((y0 + h - 1) << 16))
    own = np.where(vis == 1, touches, 0)
    pair_offset = (np.cumsum(own) - own).astype(np.uint32)  # exclusive prefix in index order
    T = int(own.sum())
    live = (rng.random((T + GUARD, ng)) < 0.6).astype(np.uint8)
    dead = rng.random(n) < 0.15  # Gaussians with every flag dead
    if full:
        dead[np.nonzero(own == 7)[0][:1]] = dead[np.nonzero(own == 97)[0][:1]] = True
    for g in np.nonzero(dead)[0]:
        live[pair_offset[g]:pair_offset[g] + own[g]] = 0
    live[T:] = 1
    if integer:
        part = rng.integers(-8, 9, (T + GUARD, ng, 10)).astype(np.float32)
    else:
        part = (rng.standard_normal((T + GUARD, ng, 10)) * np.exp(rng.uniform(-3, 3, (T + GUARD, ng, 1)))).astype(np.float32)
    want = np.zeros((n, 10), np.float64)
    terms = np.zeros(n, np.int64)
    mag = np.zeros((n, 10), np.float64)
    for g in range(n):
        sl = slice(int(pair_offset[g]), int(pair_offset[g]) + int(own[g]))
        m = live[sl].astype(bool)
        want[g] = part[sl][m].astype(np.float64).sum(0)
        mag[g] = np.abs(part[sl][m].astype(np.float64)).sum(0)
        terms[g] = int(m.sum())
    part[live == 0] = np.nan
    part[T:] = np.nan
    return dict(n=n, ng=ng, T=T, vis=vis, rects=rects, pair_offset=pair_offset, live=live, part=part, want=want,
                terms=terms, mag=mag, hidden=hidden, own=own)


def gather(pkg, cuda, c, sums, accumulate=0, order=None):
    """gs_gather_partials of case c into the device tensor `sums` [n,10]; returns the status."""
    N = pkg._native
    lib = N.load()
    dev = {k: torch.tensor(c[k].view(np.int32) if c[k].dtype == np.uint32 else c[k], device=cuda)
           for k in ("vis", "rects", "pair_offset", "live", "part")}
    od = None if order is None else torch.tensor(np.asarray(order, np.int32), device=cuda)
    a = N.GsProjectBwdArgs()
    a.g.n = c["n"]
    a.vis, a.rects, a.pair_offset = N.ptr(dev["vis"]), N.ptr(dev["rects"]), N.ptr(dev["pair_offset"])
    a.pair_grads, a.slot_live, a.grad_sums = N.ptr(dev["part"]), N.ptr(dev["live"]), N.ptr(sums)
    a.order = N.ptr(od)
    a.partial_groups = c["ng"]
    st = lib.gs_gather_partials(C.byref(a), accumulate, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("ng", [1, 2, 3, 4, 5, 9, 16])
def test_gather_integer_partials_exact(pkg, cuda, ng):
    rng = np.random.default_rng(40 + ng)
    for n in SIZES:
        c = make_case(rng, n, ng)
        assert n < 20 or (c["own"].max() == 300 and (c["terms"][c["own"] > 0] == 0).any() and
                          (c["hidden"] & (c["rects"][:, 0] != 1)).any()), "the case covers what it is for"
        # accumulate = 0 overwrites whatever the sums held
        sums = torch.full((n + 1, 10), float("nan"), device=cuda)
        assert gather(pkg, cuda, c, sums) == 0
        got = sums.cpu().numpy()
        assert np.isnan(got[n]).all(), "written past row n"
        assert np.array_equal(got[:n], c["want"].astype(np.float32)), (ng, n)
        assert not got[:n][c["hidden"]].any()
        # accumulate = 1 adds to them
        before = rng.integers(-100, 101, (n, 10)).astype(np.float32)
        sums = torch.tensor(before, device=cuda)
        assert gather(pkg, cuda, c, sums, accumulate=1) == 0
        assert np.array_equal(sums.cpu().numpy(), (before + c["want"]).astype(np.float32)), (ng, n, "accumulate")


def test_gather_order(pkg, cuda):
    """The walk in `order` (the default tile's 4 groups only) gives the index-order result."""
    rng = np.random.default_rng(50)
    for n in SIZES:
        c = make_case(rng, n, 4)
        sums = torch.full((n, 10), float("nan"), device=cuda)
        assert gather(pkg, cuda, c, sums, order=rng.permutation(n)) == 0
        assert np.array_equal(sums.cpu().numpy(), c["want"].astype(np.float32)), n
    c = make_case(rng, 33, 2)
    sums = torch.zeros((33, 10), device=cuda)
    assert gather(pkg, cuda, c, sums, order=rng.permutation(33)) == GS_ERR_UNSUPPORTED
    assert b"order" in pkg._native.load().gs_last_error()


@pytest.mark.parametrize("ng", [1, 2, 4, 5])
def test_gather_float_partials(pkg, cuda, ng):
    """Random float partials: within terms * 2^-24 * sum|x| of the fp64 sum
    (any summation order of `terms` fp32 values), bit-identical on a second
    run and between the index-order walk and a permuted one."""
    rng = np.random.default_rng(60 + ng)
    n = 257
    c = make_case(rng, n, ng, integer=False)
    runs = []
    for _ in range(2):
        sums = torch.full((n, 10), float("nan"), device=cuda)
        assert gather(pkg, cuda, c, sums) == 0
        runs.append(sums.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    err = np.abs(runs[0].astype(np.float64) - c["want"])
    bound = c["terms"][:, None] * 2.0 ** -24 * c["mag"]
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (c["terms"] > 100).any()
    if ng == 4:
        sums = torch.full((n, 10), float("nan"), device=cuda)
        assert gather(pkg, cuda, c, sums, order=rng.permutation(n)) == 0
        assert np.array_equal(sums.cpu().numpy(), runs[0])


# ---- the order itself --------------------------------------------------------
# The header promises one order for the four gathers (gs_gather_partials,
# gs_gather_abs_partials, gs_gather_feature_partials, gs_contrib_accumulate).
# Here it is stated in numpy, fp32, independently of the kernels: QL x HL
# lanes per Gaussian, lane l = h QL + q sums sequentially its live partials --
# groups qc = q, q + QL, ... < ng outer, slots e = h, h + HL, ... < touches
# inner -- and the lane sums are combined v[l] += v[l ^ 1], v[l] += v[l ^ 2]
# (4 lanes and more), v[l] += v[7 - l] (8 lanes), read on lane 0.  Float
# partials of widely varying magnitude: another order gives other bits.
ORDER_N = (33, 257)
ORDER_NG = (1, 2, 3, 4, 5, 9)
_order_cases = {}


def lanes_of(ng):
    """(QL, HL) for a slot's ng partial groups: the host dispatch's."""
    return (1, 4) if ng == 1 else (2, 2) if ng == 2 else (4, 2)


def walk_sums(c, values):
    """values [T + GUARD, ng, K] fp32 summed per Gaussian in the walk's order -> [n, K] fp32."""
    ng, live = c["ng"], c["live"]
    QL, HL = lanes_of(ng)
    idx = np.arange(QL * HL)
    out = np.zeros((c["n"], values.shape[2]), np.float32)
    for g in range(c["n"]):
        off, cnt = int(c["pair_offset"][g]), int(c["own"][g])
        v = np.zeros((QL * HL, values.shape[2]), np.float32)
        for h in range(HL):
            for q in range(QL):
                acc = v[h * QL + q]
                for qc in range(q, ng, QL):
                    for e in range(h, cnt, HL):
                        if live[off + e, qc]:
                            acc += values[off + e, qc]  # (in place, fp32)
        v = v + v[idx ^ 1]
        if QL * HL >= 4:
            v = v + v[idx ^ 2]
        if QL * HL == 8:
            v = v + v[7 - idx]
        out[g] = v[0]
    return out


def order_case(n, ng):
    """The float case of (n, ng) and its sums in the walk's order: computed once, shared, never written."""
    if (n, ng) not in _order_cases:
        c = make_case(np.random.default_rng(1000 * ng + n), n, ng, integer=False)
        c["walk"] = walk_sums(c, c["part"])
        assert c["walk"].dtype == np.float32 and not np.isnan(c["walk"]).any()
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _order_cases[(n, ng)] = c
    return _order_cases[(n, ng)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def slot_lists_on(cuda, c):
    return {k: torch.tensor(c[k].view(np.int32) if c[k].dtype == np.uint32 else c[k], device=cuda)
            for k in ("vis", "rects", "pair_offset", "live")}


@pytest.mark.parametrize("ng", ORDER_NG)
def test_gather_partials_order(pkg, cuda, ng):
    rng = np.random.default_rng(70 + ng)
    for n in ORDER_N:
        c = order_case(n, ng)
        sums = torch.full((n, 10), float("nan"), device=cuda)
        assert gather(pkg, cuda, c, sums) == 0
        assert same_bits(sums.cpu().numpy(), c["walk"]), (ng, n)
        before = rng.standard_normal((n, 10)).astype(np.float32)
        sums = torch.tensor(before, device=cuda)
        assert gather(pkg, cuda, c, sums, accumulate=1) == 0
        assert same_bits(sums.cpu().numpy(), before + c["walk"]), (ng, n, "accumulate")
        if ng == 4:
            sums = torch.full((n, 10), float("nan"), device=cuda)
            assert gather(pkg, cuda, c, sums, order=rng.permutation(n)) == 0
            assert same_bits(sums.cpu().numpy(), c["walk"]), (n, "order")


@pytest.mark.parametrize("ng", ORDER_NG)
def test_gather_abs_partials_order(pkg, cuda, ng):
    N = pkg._native
    lib = N.load()
    for n in ORDER_N:
        c = order_case(n, ng)
        dev = slot_lists_on(cuda, c)
        absg = torch.tensor(np.ascontiguousarray(c["part"][:, :, :2]), device=cuda)
        sums = torch.full((n, 2), float("nan"), device=cuda)
        a = N.GsAbsGatherArgs(n, N.ptr(dev["vis"]), N.ptr(dev["rects"]), N.ptr(dev["pair_offset"]), N.ptr(absg),
                              N.ptr(dev["live"]), ng, 0, N.ptr(sums))
        assert lib.gs_gather_abs_partials(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert same_bits(sums.cpu().numpy(), c["walk"][:, :2]), (ng, n)


@pytest.mark.parametrize("ng", ORDER_NG)
def test_gather_feature_partials_order(pkg, cuda, ng):
    """Values 0..5 into grad_sums (6..9 zeroed), 6..9 into a 4-channel window of d_features."""
    N = pkg._native
    lib = N.load()
    begin, stride = 3, 9
    for n in ORDER_N:
        c = order_case(n, ng)
        dev = slot_lists_on(cuda, c)
        part = torch.tensor(c["part"], device=cuda)
        sums = torch.full((n, 10), float("nan"), device=cuda)
        feats = torch.full((n, stride), float("nan"), device=cuda)
        a = N.GsFeatureGatherArgs(n, N.ptr(dev["vis"]), N.ptr(dev["rects"]), N.ptr(dev["pair_offset"]), N.ptr(part),
                                  N.ptr(dev["live"]), ng, 0, N.ptr(sums), N.ptr(feats), stride, begin, 4, 0)
        assert lib.gs_gather_feature_partials(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        got, gf = sums.cpu().numpy(), feats.cpu().numpy()
        assert same_bits(got[:, :6], c["walk"][:, :6]) and not got[:, 6:].any(), (ng, n)
        assert same_bits(gf[:, begin:begin + 4], c["walk"][:, 6:]), (ng, n)
        assert np.isnan(gf[:, :begin]).all() and np.isnan(gf[:, begin + 4:]).all(), "written outside the window"


@pytest.mark.parametrize("ng", ORDER_NG)
def test_contrib_accumulate_order(pkg, cuda, ng):
    """Partials (sum, max, count, 0): the sum in the walk's order, the max, the
    counts (integers <= 64 as floats) added, one view; rows with vis = 0 untouched."""
    N = pkg._native
    lib = N.load()
    for n in ORDER_N:
        c = order_case(n, ng)
        rng = np.random.default_rng(80 + 100 * ng + n)
        dev = slot_lists_on(cuda, c)
        live = c["live"].astype(bool)
        part = np.full(c["live"].shape + (4,), np.nan, np.float32)
        part[..., 0] = c["part"][..., 0]
        part[..., 1] = np.abs(c["part"][..., 1])
        part[..., 2] = np.where(live, rng.integers(0, 65, live.shape), np.nan)
        part[c["T"]:] = np.nan
        seen = c["vis"] == 1
        want_max = np.zeros(n, np.float32)
        want_px = np.zeros(n, np.int64)
        for g in np.nonzero(seen)[0]:
            sl = slice(int(c["pair_offset"][g]), int(c["pair_offset"][g]) + int(c["own"][g]))
            m = live[sl]
            want_max[g] = part[sl][m][:, 1].max(initial=0.0)
            want_px[g] = int(part[sl][m][:, 2].sum())
        w0 = rng.standard_normal(n).astype(np.float32)
        wsum, wmax = torch.tensor(w0, device=cuda), torch.full((n,), 0.25, device=cuda)
        px, views = torch.full((n,), 7, dtype=torch.int64, device=cuda), torch.full((n,), 3, dtype=torch.int32, device=cuda)
        a = N.GsContribGatherArgs(n, N.ptr(dev["vis"]), N.ptr(dev["rects"]), N.ptr(dev["pair_offset"]),
                                  N.ptr(torch.tensor(part, device=cuda)), N.ptr(dev["live"]), ng, 1, N.ptr(wsum),
                                  N.ptr(wmax), N.ptr(px), N.ptr(views))
        assert lib.gs_contrib_accumulate(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert same_bits(wsum.cpu().numpy(), np.where(seen, w0 + c["walk"][:, 0], w0)), (ng, n)
        assert same_bits(wmax.cpu().numpy(), np.where(seen, np.maximum(np.float32(0.25), want_max), np.float32(0.25)))
        assert np.array_equal(px.cpu().numpy(), 7 + want_px)
        assert np.array_equal(views.cpu().numpy(), 3 + seen.astype(np.int32))
