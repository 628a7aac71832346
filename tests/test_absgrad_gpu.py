"""Absolute screen-space gradients (AbsGS) on the device: gs_blend_backward_abs
against the fp64 statement of tests/absgrad_reference.py per (list entry, 8x8
cell), gs_gather_abs_partials on exact integer partials,
gs_density_accumulate_abs against gs_density_accumulate and an fp64 statement,
the render path end to end, the densification on both statistics, and training.

The bound of the stage tests (tests/test_absgrad_cpu.py fixes K on the CPU):

    |x_gpu - x_fp64| <= K (n_p + 1) 2^-24 M,   K = 3

with M = blend_reference.reference_tile's M[:, q, 0:2] and n_p the cell's
evaluated entries.  The signed partials keep test_blend_stage's K = 51.

Largest ratio on an MI355X, per case: GPU_RATIOS below."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import absgrad_reference as AR
import blend_reference as B
import test_blend_stage as TBS
from test_absgrad_cpu import K, K_CPU_MEASURED

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# case -> largest ratio of the absolute partials on an MI355X
GPU_RATIOS = {
    "ordinary16": 0.0245, "thin16": 0.0124, "general16": 0.0226, "opaque16": 0.0171, "bright16": 0.0136,
    "subpixel16": 0.0721, "ordinary12 (one batch, batches)": 0.0219,
    "tile20 (one batch, batches, no bitmap)": 0.0274,
}

GUARD = 64  # (entry, group) pairs after the last one, inside the allocation: stay NaN
STAGE_CASES = ["ordinary16", "thin16", "general16", "opaque16", "bright16", "subpixel16"]


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- stage level -----------------------------------------------------------------------
def _launch_backward_abs(pkg, r, cot, live, begin=0, count=0):
    """gs_blend_backward_abs on run r's forward.  The signed partials and the
    flags as test_blend_stage._launch_backward pre-fills them (7.0, 0); the
    absolute ones NaN, with a guard region."""
    N = pkg._native
    lib = N.load()
    dev = r.records.device
    G_ = count or r.fr.cells
    assert 0 <= begin and begin + G_ <= r.fr.cells
    grads = torch.full((r.T * G_, N.GS_PARTIAL_STRIDE), 7.0, device=dev)
    flags = torch.zeros((r.T * G_,), dtype=torch.uint8, device=dev)
    absg = torch.full((r.T * G_ + GUARD, 2), float("nan"), device=dev)
    gi, ga, gd = (None if c is None else torch.from_numpy(c).to(dev).contiguous() for c in cot)
    fwd = r.fwd
    lb = fwd["live"] if live else None
    ba = N.GsBlendBwdArgs(r.cam.to_struct(), r.cam.tiles_x, r.cam.tiles_y, N.ptr(r.ranges), N.ptr(r.sorted_gauss),
                          N.ptr(r.records), N.ptr(fwd["image"]), N.ptr(fwd["alpha"]), N.ptr(fwd["depth"]),
                          N.ptr(fwd["flags"]), N.ptr(fwd["cell_neval"]), N.ptr(gi), N.ptr(ga), N.ptr(gd), N.ptr(lb),
                          r.live_words if live else 0, N.ptr(grads), N.ptr(flags), r.T, begin, count)
    N.check(lib.gs_blend_backward_abs(C.byref(ba), N.ptr(absg), torch.cuda.current_stream().cuda_stream),
            "gs_blend_backward_abs")
    torch.cuda.synchronize()
    return grads, flags, absg


def _gather_abs(pkg, r, absg, flags, groups, sums=None):
    N = pkg._native
    lib = N.load()
    accumulate = sums is not None
    if sums is None:
        sums = torch.full((r.n, 2), float("nan"), device=r.records.device)
    a = N.GsAbsGatherArgs(r.n, N.ptr(r.frame.vis), N.ptr(r.frame.rects), N.ptr(r.frame.pair_offset), N.ptr(absg),
                          N.ptr(flags), groups, 1 if accumulate else 0, N.ptr(sums))
    N.check(lib.gs_gather_abs_partials(C.byref(a), torch.cuda.current_stream().cuda_stream), "gs_gather_abs_partials")
    torch.cuda.synchronize()
    return sums


def _abs_references(r, which):
    """Per tile the fp64 absolute partials [n, cells, 2], decisions forced from
    the GPU forward as test_blend_stage._references forces them."""
    key = ("abs", which)
    cot, refs = TBS._references(r, which)
    if key not in r.refs:
        nev, fl = _np(r.fwd["neval"]), _np(r.fwd["flags"])
        r.refs[key] = {t: AR.abs_partials(r.fr, AR.pixel_gradients(r.fr, t, *cot, neval=nev, flags=fl)) for t in refs}
    return cot, refs, r.refs[key]


def check_abs_backward(pkg, r, which, live=True, batches=None):
    """Every absolute partial within the bound; nothing written where the flag
    is 0; the signed partials and flags gs_blend_backward's bits; under negated
    cotangents the same absolute bits and negated signed ones; abs >= |signed|.
    Returns the absolute partials [T, cells, 2] (NaN where unwritten), the
    per-Gaussian sums gathered batch by batch, and the largest ratio."""
    fr = r.fr
    cot, refs, wants = _abs_references(r, which)
    neg = tuple(None if c is None else -c for c in cot)
    Q = fr.cells
    full = np.full((r.T, Q, 2), np.nan, np.float32)
    worst = 0.0
    sums = None
    for b, (begin, count) in enumerate(batches or [(0, Q)]):
        cnt_arg = 0 if (begin, count) == (0, Q) else count
        grads, flags, absg = _launch_backward_abs(pkg, r, cot, live, begin, cnt_arg)
        g0, f0 = TBS._launch_backward(pkg, r, r.fwd, cot, live, begin, cnt_arg)
        assert torch.equal(flags, f0), "slot_live differs from gs_blend_backward's"
        assert np.array_equal(_bits(_np(grads)), _bits(_np(g0))), "signed partials differ from gs_blend_backward's"
        want_flags, where = TBS.expected_slot_flags(r, refs, live, begin, count)
        assert np.array_equal(_np(flags), want_flags)
        a = _np(absg)
        assert np.isnan(a[r.T * count:]).all(), "written past the last partial"
        a = a[:r.T * count]
        assert np.isnan(a[want_flags == 0]).all(), "an absolute partial written where slot_live is 0"
        assert np.isfinite(a[want_flags == 1]).all() and (a[want_flags == 1] >= 0).all()
        ngr, nfl, nabs = _launch_backward_abs(pkg, r, neg, live, begin, cnt_arg)
        assert torch.equal(nfl, flags)
        assert np.array_equal(_bits(_np(nabs)), _bits(_np(absg))), "negated cotangents change the absolute partials"
        sg, nsg = _np(grads).reshape(-1, 10)[want_flags == 1], _np(ngr).reshape(-1, 10)[want_flags == 1]
        assert np.array_equal(nsg, -sg), "negated cotangents do not negate the signed partials"
        g = _np(grads).reshape(r.T, count, 10)
        a = a.reshape(r.T, count, 2)
        for k, (t, i, q) in where.items():
            ref = refs[t]
            got = a[k // count, k % count]
            full[k // count, q] = got
            if not ref["live"][i, q]:
                assert not got.any(), f"tile {t} entry {i} cell {q}: no pixel evaluated it, absolute partial {got}"
            unit = (ref["n_cell"][q] + 1) * B.U24 * ref["M"][i, q, 0:2]
            err = np.abs(got.astype(np.float64) - wants[t][i, q])
            with np.errstate(divide="ignore", invalid="ignore"):
                rt = np.nan_to_num(np.where(err > 0, err / unit, 0.0), nan=np.inf)
            worst = max(worst, float(rt.max()))
            assert (rt <= K).all(), (
                f"{r.name} {which}: tile {t} entry {i} (Gaussian {ref['ids'][i]}) cell {q}: abs {got!r} vs fp64 "
                f"{wants[t][i, q]!r}, {rt} units of {unit} (K = {K})")
            signed = np.abs(g[k // count, k % count, 0:2].astype(np.float64))
            assert (got + K * unit >= signed).all(), (t, i, q, got, signed)
        sums = _gather_abs(pkg, r, absg, flags, count, sums if b else None)
    return full, _np(sums), worst


def _report(name, what, ratio):
    print(f"GPU ratio {name} {what}: absolute partials {ratio:.3g} (K = {K}; CPU formulation {K_CPU_MEASURED})")


@pytest.mark.parametrize("name", STAGE_CASES)
def test_abs_partials(pkg, cuda, name):
    r = TBS._frame(pkg, cuda, name)
    _, worst = check_abs_backward(pkg, r, "all")[1:]
    _report(name, "all", worst)


def test_abs_partials_ordinary12_in_batches(pkg, cuda):
    """The general instantiation: tile 12, one batch of its four cells and the
    batches (0,2), (2,2) -- the same partial bits."""
    r = TBS._frame(pkg, cuda, "ordinary12")
    assert r.fr.cells == 4
    one, s1, worst = check_abs_backward(pkg, r, "all")
    two, s2, w2 = check_abs_backward(pkg, r, "all", batches=[(0, 2), (2, 2)])
    assert np.array_equal(_bits(one), _bits(two))
    _check_gathered(r, one, s1)
    _check_gathered(r, two, s2)
    _report("ordinary12", "one batch / batches", max(worst, w2))


def _check_gathered(r, full, sums):
    """The gathered sums against the fp64 sum of the partials the blend wrote:
    `terms` fp32 additions in any order stay within terms 2^-24 sum|x|."""
    fr = r.fr
    want, terms = np.zeros((r.n, 2)), np.zeros(r.n)
    for t in range(r.tiles):
        ids, slots = fr.entries(t), fr.slots(t)
        for i, g in enumerate(ids):
            p = full[int(slots[i])]
            m = ~np.isnan(p[:, 0])
            want[g] += p[m].astype(np.float64).sum(0)
            terms[g] += m.sum()
    assert np.isfinite(sums).all()
    assert (np.abs(sums - want) <= (terms[:, None] + 1) * B.U24 * want).all()
    assert not sums[terms == 0].any(), "a Gaussian with no live partial gets zeros"
    return want


def test_abs_partials_tile20_batches_and_no_bitmap(pkg, cuda):
    """Nine cells per tile, three ways: one batch; the batches (0,4), (4,4),
    (8,1) with gs_gather_abs_partials accumulating -- every partial the same
    bits (a partial's summation does not depend on the batch), the gathered
    sums the same values up to the order of their fp32 additions (one batch
    walks nine groups on four group lanes, the batches 4 + 4 + 1); and no
    liveness bitmap -- other chunks, within the bound."""
    r = TBS._frame(pkg, cuda, "tile20")
    assert r.fr.cells == 9
    one, s1, w1 = check_abs_backward(pkg, r, "all")
    batched, s3, w3 = check_abs_backward(pkg, r, "all", batches=[(0, 4), (4, 4), (8, 1)])
    assert np.array_equal(_bits(one), _bits(batched))
    want = _check_gathered(r, one, s1)
    _check_gathered(r, batched, s3)
    assert want.max() > 0
    nobits, _, wn = check_abs_backward(pkg, r, "all", live=False)
    assert np.isnan(one).sum() > np.isnan(nobits).sum(), "the bitmap-free replay writes entries the bitmap skips"
    _report("tile20", "one batch / batches / no bitmap", max(w1, w3, wn))


# ---- the gather ------------------------------------------------------------------------
@pytest.mark.parametrize("ng", [1, 2, 3, 4, 5, 9, 16])
def test_gather_abs_integer_partials_exact(pkg, cuda, ng):
    """Integer partials in [0, 8]: every sum exact in fp32 in any order, compared
    for equality with a numpy sum over the live flags; dead partials and the
    guard hold NaN.  Sizes and slot counts as tests/test_gather_partials.py."""
    from test_gather_partials import SIZES, make_case
    N = pkg._native
    lib = N.load()
    rng = np.random.default_rng(140 + ng)
    for n in SIZES:
        c = make_case(rng, n, ng)
        T = c["T"]
        part = rng.integers(0, 9, (len(c["live"]), ng, 2)).astype(np.float32)
        want = np.zeros((n, 2))
        for g in range(n):
            sl = slice(int(c["pair_offset"][g]), int(c["pair_offset"][g]) + int(c["own"][g]))
            want[g] = part[sl][c["live"][sl].astype(bool)].astype(np.float64).sum(0)
        part[c["live"] == 0] = np.nan
        part[T:] = np.nan
        dev = {k: torch.tensor(c[k].view(np.int32) if c[k].dtype == np.uint32 else c[k], device=cuda)
               for k in ("vis", "rects", "pair_offset", "live")}
        dpart = torch.tensor(part, device=cuda)

        def gather(sums, accumulate):
            a = N.GsAbsGatherArgs(n, N.ptr(dev["vis"]), N.ptr(dev["rects"]), N.ptr(dev["pair_offset"]), N.ptr(dpart),
                                  N.ptr(dev["live"]), ng, accumulate, N.ptr(sums))
            assert lib.gs_gather_abs_partials(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            return _np(sums)

        got = gather(torch.full((n + 1, 2), float("nan"), device=cuda), 0)
        assert np.isnan(got[n]).all(), "written past row n"
        assert np.array_equal(got[:n], want.astype(np.float32)), (ng, n)
        assert not got[:n][c["hidden"]].any() and not got[:n][c["terms"] == 0].any()
        before = rng.integers(-100, 101, (n, 2)).astype(np.float32)
        got = gather(torch.tensor(before, device=cuda), 1)
        assert np.array_equal(got, (before + want).astype(np.float32)), (ng, n, "accumulate")


# ---- gs_density_accumulate_abs ---------------------------------------------------------
KW, KH, KN = 52, 44, 300  # W != H; two 256-blocks, the second partial (tests/test_density_gpu.py)


@pytest.mark.parametrize("variant", ["both", "no_abs_sums", "no_g_means2d", "neither"])
def test_accumulate_abs_kernel(pkg, cuda, variant):
    N = pkg._native
    lib = N.load()
    rng = np.random.default_rng(15)
    sums = rng.normal(0, 1e-3, (KN, 10)).astype(np.float32)
    asum = np.abs(rng.normal(0, 3e-3, (KN, 2))).astype(np.float32)
    gm = rng.normal(0, 1e-3, (KN, 2)).astype(np.float32)
    radii = rng.uniform(0.5, 40.0, KN).astype(np.float32)
    vis = rng.random(KN) > 1 / 3
    start = [rng.uniform(0.0, 0.05, KN).astype(np.float32), rng.integers(0, 9, KN).astype(np.float32),
             rng.uniform(0.0, 30.0, KN).astype(np.float32), rng.uniform(0.0, 0.2, KN).astype(np.float32)]
    inv = ~vis
    assert 80 < inv.sum() < 120 and vis[256:].any() and inv[256:].any()
    for s in start:  # invisible rows keep their bits, whatever they are
        s[np.nonzero(inv)[0][::3]] = np.nan
    asum[np.nonzero(inv)[0][1::3]] = np.nan  # (and are not read)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    d_sums, d_asum, d_gm, d_vis, d_radii = dev(sums), dev(asum), dev(gm), dev(vis), dev(radii)
    use_a, use_m = variant in ("both", "no_g_means2d"), variant in ("both", "no_abs_sums")
    acc, den, rad, ab = (dev(a) for a in start)
    acc0, den0, rad0 = (dev(a) for a in start[:3])
    st = N.GsDensityStatsArgs(KN, KW, KH, N.ptr(d_vis), N.ptr(d_radii), N.ptr(d_sums), N.ptr(d_gm) if use_m else None,
                              N.ptr(acc), N.ptr(den), N.ptr(rad))
    st0 = N.GsDensityStatsArgs(KN, KW, KH, N.ptr(d_vis), N.ptr(d_radii), N.ptr(d_sums), N.ptr(d_gm) if use_m else None,
                               N.ptr(acc0), N.ptr(den0), N.ptr(rad0))
    a = N.GsDensityAbsArgs(st, N.ptr(d_asum) if use_a else None, N.ptr(ab))
    want = start[3].astype(np.float64)
    ax = (asum[:, 0].astype(np.float64) if use_a else 0.0) + (np.abs(gm[:, 0].astype(np.float64)) if use_m else 0.0)
    ay = (asum[:, 1].astype(np.float64) if use_a else 0.0) + (np.abs(gm[:, 1].astype(np.float64)) if use_m else 0.0)
    norm = np.sqrt((0.5 * KW * ax) ** 2 + (0.5 * KH * ay) ** 2) * np.ones(KN)
    for step in range(2):  # two successive accumulations into non-zero starting values
        N.check(lib.gs_density_accumulate_abs(C.byref(a), N.stream_ptr()), "gs_density_accumulate_abs")
        N.check(lib.gs_density_accumulate(C.byref(st0), N.stream_ptr()), "gs_density_accumulate")
        want = np.where(vis, want + norm, want)
    torch.cuda.synchronize()
    for got, ref in ((acc, acc0), (den, den0), (rad, rad0)):  # gs_density_accumulate's bits
        assert _np(got).tobytes() == _np(ref).tobytes()
    got = _np(ab)
    assert got[inv].tobytes() == start[3][inv].tobytes()
    rel = np.abs(got[vis] - want[vis]) / np.maximum(np.abs(want[vis]), 1e-30)
    print(f"abs_accum ({variant}): max rel err {rel.max():.3g}")
    # two products, a sum and a square root in fp32 stay within 3 ulp; each accumulation rounds once
    assert np.isfinite(got[vis]).all() and rel.max() <= 1e-6
    if variant == "neither":
        assert np.array_equal(got[vis], start[3][vis])  # the norm of nothing: + 0


# ---- render level ----------------------------------------------------------------------
class _Run:
    pass


_RENDER = {}


def _scene_run(pkg, cuda, key, sc):
    """A scene dict (blend_reference.make_scene) as a run like test_blend_stage._frame's:
    the library's own frame, copied to the host for the fp64 statement."""
    if key in _RENDER:
        return _RENDER[key]
    RZ = pkg.rasterizer
    W, H, L = sc["W"], sc["H"], sc["L"]
    cam = RZ.CameraParams(W, H, B.FX, B.FX, W * 0.5, H * 0.5, (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0),
                          tuple(float(v) for v in sc["bg"]), 0.01, 50.0, L)
    t = lambda a: torch.from_numpy(a).to(cuda)
    RZ._T_SEEN.pop(cuda, None)
    frame = RZ.forward_pipeline(cam, t(sc["xyz"]), t(sc["cov3d"]), None, None, t(sc["color_logits"]), t(sc["opacity"]),
                                need_grad=True, stage_path=True)[-1]
    torch.cuda.synchronize()
    r = _Run()
    r.name, r.sc, r.cam, r.frame = key, sc, cam, frame
    r.n, r.T, r.tiles = len(sc["opacity"]), int(frame.T), cam.tiles_x * cam.tiles_y
    r.records, r.ranges, r.sorted_gauss, r.live_bits = frame.records, frame.ranges, frame.sorted_gauss, frame.live_bits
    r.live_words = int(frame.live_bits.shape[1])
    r.fr = B.Frame(_np(frame.records).copy(), _np(frame.sorted_gauss).astype(np.int64),
                   _np(frame.ranges).astype(np.int64), W, H, L, sc["bg"])
    assert r.fr.T == r.T > 0 and r.fr.sorted_gauss.max() < r.n
    r.fwd = TBS._launch_forward(pkg, r, live=True, counts=False, neval=True)
    _RENDER[key] = r
    return r


def _statistic_statement(r, cot):
    """Per Gaussian, from the fp64 statement summed over tiles: the signed and
    the absolute (x, y) sums and the summed bounds' units of each."""
    fr = r.fr
    nev, fl, al = _np(r.fwd["neval"]), _np(r.fwd["flags"]), _np(r.fwd["alpha"])
    signed, absolute, unit = np.zeros((r.n, 2)), np.zeros((r.n, 2)), np.zeros((r.n, 2))
    for t in range(r.tiles):
        ids = fr.entries(t)
        if not len(ids):
            continue
        ref = B.reference_tile(fr, t, *cot, neval=nev, flags=fl, alpha_fwd=al)
        assert not B.validate_termination(ref, r.name)
        pg = AR.pixel_gradients(fr, t, *cot, neval=nev, flags=fl)
        s, a = AR.cell_sums(fr, pg, False), AR.cell_sums(fr, pg, True)
        u = (ref["n_cell"][None, :, None] + 1) * B.U24 * ref["M"][:, :, 0:2]
        for i, g in enumerate(ids):
            signed[g] += s[i].sum(0)
            absolute[g] += a[i].sum(0)
            unit[g] += u[i].sum(0)
    return signed, absolute, unit


def _ndc(v, W, H):
    return np.sqrt((0.5 * W * v[:, 0]) ** 2 + (0.5 * H * v[:, 1]) ** 2)


def _render(pkg, cuda, r, cot, stats, twice=False):
    sc = r.sc
    leaves = {k: torch.from_numpy(sc[k]).to(cuda).requires_grad_(True) for k in ("xyz", "cov3d", "color_logits", "opacity")}
    outs = pkg.rasterize(r.cam, leaves["xyz"], leaves["cov3d"], None, None, leaves["color_logits"], leaves["opacity"],
                         density_stats=stats)
    gi, ga, gd = (torch.from_numpy(c).to(cuda) for c in cot)
    L = (outs[0] * gi).sum() + (outs[1] * ga).sum() + (outs[2] * gd).sum()
    L.backward(retain_graph=twice)
    if twice:
        once = (stats.abs_accum.clone(), stats.grad_accum.clone())
        L.backward()
        torch.cuda.synchronize()
        return once
    torch.cuda.synchronize()
    return [_np(o) for o in outs], {k: _np(v.grad) for k, v in leaves.items()}


@pytest.mark.parametrize("L", [16, 12])
def test_render_statistics_and_bit_identity(pkg, cuda, L):
    """64x48, 200 Gaussians: outputs and every gradient the same bits with
    DensityStats(abs_grad=True), DensityStats() and no statistics; abs_accum
    against the fp64 statement summed over tiles; a second backward of one
    frame adds the view twice."""
    sc = B._random_scene(seed=21, n=200, W=64, H=48, L=L, sigma=(2.0, 6.0), opacity=(0.02, 0.5))
    r = _scene_run(pkg, cuda, ("render", L), sc)
    cot = B.cotangents(64, 48, seed=9)
    n = r.n
    s_abs, s_plain = pkg.DensityStats(n, cuda, abs_grad=True), pkg.DensityStats(n, cuda)
    runs = [_render(pkg, cuda, r, cot, s) for s in (s_abs, s_plain, None)]
    for outs, grads in runs[1:]:
        assert len(outs) == 7 and len(grads) == 4
        for a, b in zip(runs[0][0], outs):
            assert a.tobytes() == b.tobytes()
        for k in grads:
            assert runs[0][1][k].tobytes() == grads[k].tobytes(), k
    for a, b in ((s_abs.grad_accum, s_plain.grad_accum), (s_abs.denom, s_plain.denom), (s_abs.max_radii, s_plain.max_radii)):
        assert torch.equal(a, b), "the signed statistics' values change"
    vis = runs[0][0][6].astype(bool)
    signed, absolute, unit = _statistic_statement(r, cot)
    want = np.where(vis, _ndc(absolute, 64, 48), 0.0)
    # each partial within K units, the gather's and the norm's fp32 roundings on top
    tol = K * _ndc(unit, 64, 48) + 1e-6 * want
    got = _np(s_abs.abs_accum).astype(np.float64)
    worst = float((np.abs(got - want)[vis] / np.maximum(tol[vis], 1e-300)).max())
    print(f"tile {L}: abs_accum within {worst:.3g} of its tolerance; mean abs / signed statistic "
          f"{want[vis].mean() / _ndc(signed, 64, 48)[vis].mean():.3g}")
    assert vis.sum() > 150 and want[vis].min() > 0
    assert (np.abs(got - want) <= tol).all() and not got[~vis].any()
    assert (got >= _np(s_abs.grad_accum) * (1 - 1e-6) - TBS.K * _ndc(unit, 64, 48)).all()
    # a second backward of one frame adds the view twice
    s2 = pkg.DensityStats(n, cuda, abs_grad=True)
    once_abs, once_signed = _render(pkg, cuda, r, cot, s2, twice=True)
    assert torch.equal(once_abs, s_abs.abs_accum) and torch.equal(s2.abs_accum, once_abs + once_abs)
    assert torch.equal(s2.grad_accum, once_signed + once_signed) and torch.equal(s2.denom, 2 * s_abs.denom)


@pytest.mark.parametrize("L", [16, 12])
def test_cancellation_case(pkg, cuda, L):
    """What the signed statistic cannot see: one isolated isotropic Gaussian
    centred between four pixels under a cotangent symmetric about its centre
    (constant).  Its per-pixel gradients cancel in the signed sum; the absolute
    one matches the fp64 value, far from 0."""
    cx, cy = {16: (31.5, 31.5), 12: (35.5, 23.5)}[L]  # on a tile corner: four tiles, every pixel within reach in them
    sc = B.make_scene(64, 48, L, [cx], [cy], [3.0], [1.5], [1.5], [0.0], [0.5], [[0.8, 0.3, 0.6]])
    r = _scene_run(pkg, cuda, ("cancel", L), sc)
    H, W = 48, 64
    cot = (np.broadcast_to(np.array([0.7, -0.3, 0.5], np.float32)[:, None, None], (3, H, W)).copy(),
           np.full((H, W), 0.2, np.float32), np.full((H, W), 0.1, np.float32))
    signed, absolute, unit = _statistic_statement(r, cot)
    assert len(r.fr.sorted_gauss) == 4, "the Gaussian straddles four tiles"
    # the construction: fp64's signed sum is rounding noise beside the absolute one
    assert np.abs(signed[0]).max() <= 1e-12 * absolute[0].min()
    stats = pkg.DensityStats(1, cuda, abs_grad=True)
    _render(pkg, cuda, r, cot, stats)
    got_signed, got_abs = float(stats.grad_accum[0]), float(stats.abs_accum[0])
    want = float(_ndc(absolute, W, H)[0])
    bound_signed = TBS.K * float(_ndc(unit, W, H)[0])
    bound_abs = K * float(_ndc(unit, W, H)[0]) + 1e-6 * want
    print(f"tile {L}: signed statistic {got_signed:.3g} (bound {bound_signed:.3g}), absolute {got_abs:.6g} "
          f"(fp64 {want:.6g})")
    assert float(stats.denom[0]) == 1.0
    assert got_signed <= bound_signed
    assert abs(got_abs - want) <= bound_abs
    assert want > 1000 * bound_signed


# ---- densification on both statistics ----------------------------------------------------
def test_densify_splits_on_abs_and_clones_on_signed(pkg, cuda):
    """n = 300 (two classify blocks), against the torch statement of
    tests/test_densify.py evaluated once per rule: the split test on the mean
    absolute gradient against its threshold, the clone test on the signed mean."""
    import math
    from test_densify import LARGE, NAMES, SMALL, _model, ref_densify
    n, th, th_abs, ext, min_op, seed = 300, 2e-4, 8e-4, 1.0, 0.01, 93
    i = torch.arange(n)
    abs_cls, sg_cls, size_cls, dead = i % 2, (i // 2) % 2, (i // 4) % 3, (i // 12) % 2
    unseen = i % 25 == 7

    def model():
        torch.manual_seed(16)  # (_model draws the rest features from the default generator)
        m, _ = _model(pkg, cuda, n=n, seed=16)
        with torch.no_grad():
            m._scaling.copy_(torch.tensor([LARGE, SMALL, math.log(0.02)])[size_cls][:, None].expand(-1, 3))
            m._opacity.copy_(torch.where(dead == 1, -10.0, 2.0)[:, None])
        return m

    denom = torch.where(unseen, 0.0, 1.0 + (i % 5).float())
    q_abs = torch.tensor([0.5, 2.0])[abs_cls] * th_abs
    q_sg = torch.tensor([0.5, 2.0])[sg_cls] * th
    accum = torch.where(unseen, torch.full((n,), 7.0), q_sg * denom)
    abs_accum = torch.where(unseen, torch.full((n,), 9.0), q_abs * denom)
    quot = lambda a: torch.where(denom > 0, a / denom.clamp_min(1), torch.zeros(n))
    g_abs = torch.stack([quot(abs_accum), torch.zeros(n), torch.zeros(n)], -1)
    g_sg = torch.stack([quot(accum), torch.zeros(n), torch.zeros(n)], -1)
    for g, t in ((g_abs, th_abs), (g_sg, th)):  # no decision on a threshold
        assert torch.all((g[:, 0] == 0) | ((g[:, 0] / t - 0.5).abs() < 1e-3) | ((g[:, 0] / t - 2).abs() < 1e-3))
    m = model()
    A, (nkA, nsA, _), (keepA, spA, _, _, s, o) = ref_densify(m, g_abs, th_abs, ext, min_op, seed, masks=True, clone=False)
    Bc, (nkB, _, ncB), (_, _, clB, _, _, _) = ref_densify(m, g_sg, th, ext, min_op, seed, masks=True, split=False)
    want = {k: torch.cat([A[k], Bc[k][nkB:]]) for k in NAMES}
    # the rule shows: large Gaussians split that the signed mean would leave, and the reverse
    hot_abs, hot_sg, large = quot(abs_accum) > th_abs, quot(accum) > th, s > 0.03 * ext
    alive = o > min_op
    assert (spA & ~hot_sg.cpu()).sum() > 5 and (large & hot_sg & ~hot_abs & alive & keepA).sum() > 5
    assert (clB & ~hot_abs.cpu()).sum() > 5 and nsA > 10 and ncB > 10
    combos = {(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(abs_cls, sg_cls, size_cls, dead)}
    assert len(combos) == 24
    stats = pkg.DensityStats(n, cuda, abs_grad=True)
    stats.grad_accum.copy_(accum), stats.denom.copy_(denom), stats.abs_accum.copy_(abs_accum)
    info = m.densify_and_prune(th, ext, min_op, seed=seed, stats=stats, abs_grad_threshold=th_abs)
    assert (info["kept"], info["split"], info["cloned"]) == (nkA, nsA, ncB)
    assert info["n"] == nkA + 2 * nsA + ncB == m.get_num_points()
    got = dict(zip(NAMES, [p.detach().cpu().double() for p in m.parameter_list()]))
    for k in NAMES:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        tol = 1e-4 if k == "op" else 1e-5  # (as tests/test_densify.py)
        assert (got[k] - want[k]).abs().max().item() < tol, k
    assert m.density_stats.n == info["n"]
    # split_accum = NULL: the signed rule as it was, whatever the absolute statistic holds
    old, counts = ref_densify(model(), g_sg, th, ext, min_op, seed)
    m1, m2 = model(), model()
    plain = pkg.DensityStats(n, cuda)
    plain.grad_accum.copy_(accum), plain.denom.copy_(denom)
    stats.abs_accum.fill_(float("nan"))
    i1 = m1.densify_and_prune(th, ext, min_op, seed=seed, stats=plain)
    i2 = m2.densify_and_prune(th, ext, min_op, seed=seed, stats=stats)
    assert i1 == i2 and (i1["kept"], i1["split"], i1["cloned"]) == counts
    for a, b in zip(m1.parameter_list(), m2.parameter_list()):
        assert torch.equal(a.detach(), b.detach())
    for k, p in zip(NAMES, m1.parameter_list()):
        assert (p.detach().cpu().double() - old[k]).abs().max().item() < (1e-4 if k == "op" else 1e-5), k


# ---- training --------------------------------------------------------------------------
def _middle(v):
    """The midpoint of the two middle values: about half above, none on it."""
    v = torch.sort(v.double().cpu()).values
    assert v.numel() >= 2 and v[v.numel() // 2 - 1] < v[v.numel() // 2]
    return float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2)


def test_trainer_densifies_on_absolute_gradients(pkg, cuda, tmp_path):
    """300 iterations of tests/test_density_training_gpu.py's scene with
    densify_absgrad: densification runs, PSNR rises, and a run resumed from
    the checkpoint of iteration 200 equals the uninterrupted one bit for bit.
    (200 is right after a densification, where the statistics are zeros: the
    one kind of iteration at which a checkpoint that lost them could not
    show.  tests/test_resume_gpu.py resumes where they are live.)"""
    from scene_util import load_scene, write_scene_files
    write_scene_files(tmp_path, 12, 64)
    ds = load_scene(pkg, tmp_path, cuda, 64)
    cfg = pkg.TrainingConfig(iterations=300, densify_from_iter=100, densify_until_iter=300, densify_interval=100,
                             num_random_points=3000, log_interval=100, output_path=str(tmp_path / "out"),
                             position_lr_init=1.6e-3, position_lr_final=1.6e-5, densify_criterion="screen",
                             densify_absgrad=True, prune_screen_radius=20.0)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    before = tr.validate()
    st = tr.gaussians.density_stats
    assert st.n == 3000 and st.abs_accum is not None and not st.abs_accum.any()
    tr.train(99)
    seen = st.denom > 0
    assert int(seen.sum()) > 100 and bool((st.abs_accum[seen] >= st.grad_accum[seen] * (1 - 1e-3)).all())
    ratio = float(st.mean_abs_grad()[seen].mean() / st.mean_grad()[seen].mean())
    cfg.densify_grad_threshold = _middle(st.mean_grad()[seen])
    cfg.densify_abs_grad_threshold = _middle(st.mean_abs_grad()[seen])
    tr.train(1)
    first = dict(tr.last_densify)
    print(f"mean abs / signed statistic {ratio:.3g}; thresholds {cfg.densify_grad_threshold:.3g} / "
          f"{cfg.densify_abs_grad_threshold:.3g}: first densification {first}")
    assert first["split"] + first["cloned"] > 0
    s = tr.gaussians.density_stats
    assert s.n == first["n"] and s.abs_accum.shape == (first["n"],) and not s.abs_accum.any() and not s.denom.any()
    tr.train(100)
    assert tr.iteration == 200 and not tr.gaussians.density_stats.denom.any()
    tr.save_checkpoint(200)
    tr.train(100)
    after = tr.validate()
    n = tr.gaussians.get_num_points()
    print(f"PSNR {before['psnr']:.2f} -> {after['psnr']:.2f} dB; Gaussians 3000 -> {n}")
    assert after["psnr"] > before["psnr"] and tr.last_densify["n"] == n
    for p in tr.gaussians.parameter_list():
        assert torch.isfinite(p).all()
    tr2 = pkg.GaussianTrainer(cfg, ds)
    tr2.load_checkpoint(200)
    s2 = tr2.gaussians.density_stats
    assert s2.abs_accum is not None and s2.abs_accum.shape == s2.denom.shape and not s2.abs_accum.any()
    tr2.train(100)
    assert tr2.iteration == tr.iteration == 300 and tr2.gaussians.get_num_points() == n
    for a, b in zip(tr.gaussians.parameter_list(), tr2.gaussians.parameter_list()):
        assert torch.equal(a.detach(), b.detach())


def _two_rank_statement(pkg, ds, cfg, world, stop_before_densify=False):
    """tests/test_density_training_gpu.py's single-process statement of two
    ranks, with the absolute statistic: one DensityStats(abs_grad=True) per
    simulated rank, added at the densification as the all-reduce adds them."""
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    cams = ds.get_train_cameras()
    g = tr.gaussians
    new = lambda: [pkg.DensityStats(g.get_num_points(), g._xyz.device, abs_grad=True) for _ in range(world)]
    per_rank = new()
    for it in range(1, cfg.iterations + 1):
        tr.iteration = it
        if per_rank[0].n != g.get_num_points():
            per_rank = new()
        grads = []
        for r in range(world):
            cam = cams[int(tr._perm[(it * world + r) % len(cams)])]
            tr.optimizer.zero_grad()
            out = tr.renderer.render(cam, g, tr._settings(cam), density_stats=per_rank[r])
            pkg.loss.photometric_loss(out["image"], cam._image, cfg.lambda_dssim)[0].backward()
            grads.append([p.grad.clone() for p in g.grad_parameters()])
        for i, p in enumerate(g.grad_parameters()):
            s = grads[0][i].clone()
            for k in range(1, world):
                s += grads[k][i]
            p.grad = s / world
        tr.optimizer.update_learning_rate(it)
        tr.optimizer.step()
        if tr.optimizer.density_controller.should_densify(it):
            total = g.density_stats
            total.grad_accum.copy_(per_rank[0].grad_accum + per_rank[1].grad_accum)
            total.denom.copy_(per_rank[0].denom + per_rank[1].denom)
            total.max_radii.copy_(torch.maximum(per_rank[0].max_radii, per_rank[1].max_radii))
            total.abs_accum.copy_(per_rank[0].abs_accum + per_rank[1].abs_accum)
            tr.reduced_abs = total.abs_accum.clone()
            if stop_before_densify:
                return tr
        tr.last_densify = tr.optimizer.densify_and_prune(it, tr.scene_extent) or tr.last_densify
    return tr


def test_dp_two_ranks_all_reduce_the_absolute_statistic(pkg, cuda, tmp_path):
    from dp_absgrad_worker import absgrad_config
    from scene_util import load_scene, write_scene_files
    from test_dp_training_gpu import _free_port
    write_scene_files(tmp_path)
    ds = load_scene(pkg, tmp_path, cuda, split=False)
    pre = _two_rank_statement(pkg, ds, absgrad_config(pkg, tmp_path / "pre", 1.0, 1.0), 2, stop_before_densify=True)
    st = pre.gaussians.density_stats
    assert float(st.denom.max()) == 4.0  # two ranks, two iterations
    seen = st.denom > 0
    th, th_abs = _middle(st.mean_grad()[seen]), _middle(st.mean_abs_grad()[seen])
    port = _free_port()
    outs = [tmp_path / f"rank{r}.npz" for r in range(2)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", GS_ALLREDUCE_CHUNKS="2", GS_ALLREDUCE_MIN_ROWS="256")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_absgrad_worker.py"), str(r), "2", str(port),
                               str(tmp_path), str(outs[r]), repr(th), repr(th_abs)], env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0], rcs
    a, b = (np.load(o) for o in outs)
    n0 = absgrad_config(pkg, tmp_path, th, th_abs).num_random_points
    print(f"DP absgrad, thresholds {th:.3g} / {th_abs:.3g}: {n0} -> {int(a['n'])} Gaussians "
          f"(split {int(a['split'])}, cloned {int(a['cloned'])})")
    assert int(a["iteration"]) == 3 and int(a["n"]) == int(b["n"]) != n0
    assert float(a["abs_threshold"]) == th_abs
    for i in range(6):
        assert np.array_equal(a[f"p{i}"], b[f"p{i}"]), f"replicas diverged in parameter {i}"
    for k in ("reduced_abs", "reduced_accum", "reduced_denom"):
        assert np.array_equal(a[k], b[k]), f"the ranks densified on different {k}"
    ref = _two_rank_statement(pkg, ds, absgrad_config(pkg, tmp_path / "ref", th, th_abs), 2)
    assert np.array_equal(a["reduced_abs"], _np(ref.reduced_abs)), "reduced abs_accum != the single-process sum"
    assert a["reduced_abs"].max() > 0 and a["reduced_denom"].max() == 4.0
    assert ref.gaussians.get_num_points() == int(a["n"])
    assert (ref.last_densify["split"], ref.last_densify["cloned"]) == (int(a["split"]), int(a["cloned"]))
    for i, p in enumerate(ref.gaussians.parameter_list()):
        assert np.array_equal(_np(p), a[f"p{i}"]), f"DP step != two-rank statement (parameter {i})"
    # after the densification each rank's statistics hold its own view of iteration 3 only
    assert a["abs_after"].shape == (int(a["n"]),) and a["denom_after"].max() == 1.0
    assert not np.array_equal(a["abs_after"], b["abs_after"])
