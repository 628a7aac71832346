"""Stage test of the replays of the colour blend (csrc/gs_features.hip:
k_feat_fwd, k_feat_bwd, k_gather_feat, k_contrib, k_contrib_gather,
k_dist_fwd<kInv>, k_dist_bwd<kInv>): every float, count, id and gradient
partial the seven kernels write, launched through the C entry points on the
library's own frame, against the fp64 statements of tests/replay_reference.py,
per (list entry, 8x8 cell).

The bound has the project's form (stage by stage):

    |x_gpu - x_fp64| <= K (n + 1) 2^-24 M(x)

M(x): the statement's expression for x with every term replaced by its
absolute value (geometric monomials at their maximum over the cell), n: the
pixel's or the cell's evaluated entries.  K, per family, is 4 x the largest
ratio that the documented formulation shows in plain numpy fp32
(replay_reference.emulate_*, on blend_reference's phases) on host-built frames
of every case below, rounded up, not below 8 -- set before the GPU is asked:

    family         measured on the CPU                             K
    features       1.941 (subpixel16, the forward image)           8
    contributions  2.821 (far)                                     12
    distortion     2.232 (subpixel16, linear, the forward D)       9

(test_fp32_formulation_sets_K; the blend's 51 comes from its fixture frames
and does not carry over.)  The other cases stay below 0.92.  Four
deliberately wrong emulations exceed K on the statement: row moments about
row 0 (subpixel16: 1510 and 685 units), the terminating entry given the live
formula (opaque16: T = 0, not finite), the last chunk's cotangent of the
channels >= C unmasked (a partial where the statement has exactly 0), the
distortion on unshifted depths (far_scene: over 1e10 units).

Largest ratio on an MI355X per case and family: GPU_RATIOS below; over all of
them 2.49 (features forward), 1.90 (features partials), 0.106 (features
gathered), 1.67 (contributions), 2.39 (dominant weight), 2.01 (distortion
forward), 0.873 (distortion partials), all on subpixel16 but the gathered
sums (tile20).  No kernel needed a change.

The decisions are reproduced, not exempted: the skip in numpy fp32 bit for
bit, the termination from the forward's pix_neval, validated; the dominant
and median ids exact wherever the fp64 margin exceeds the bound, and the
pixels inside the margin at most 2 % of a case's covered pixels (checked on
the statement alone, on the CPU) -- but for the median id of the four dense
low-opacity cases, whose open pixels are counted and recorded (MEDIAN_OPEN)."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_reference as B
import distortion_util as DU
import features_util as FU
import replay_reference as R
import test_blend_stage as TBS

CASES = ("ordinary16", "ordinary12", "thin16", "general16", "opaque16", "subpixel16", "tile8", "tile20")
MAPS = (None, DU.NEAR_FAR)
CPU_C = 5  # two chunks, the last with one channel

# family -> the largest ratio of the numpy fp32 formulation on host-built frames (test_fp32_formulation_sets_K)
K_CPU_MEASURED = {"features": 1.941, "contributions": 2.821, "distortion": 2.232}
K_FEATURES, K_CONTRIB, K_DISTORTION = 8.0, 12.0, 9.0
# case -> largest ratios on an MI355X: features (forward, partials), contributions (partials, dominant weight),
# distortion (forward, partials), both depth maps; tile20 with its batches and without the bitmap
GPU_RATIOS = {
    "ordinary16": ((0.0806, 0.0829), (0.144, 0.0207), (0.0724, 0.0649)),
    "ordinary12": ((0.138, 0.229), (0.312, 0.0701), (0.0877, 0.0575)),
    "thin16": ((0.0721, 0.124), (0.141, 0.0186), (0.0677, 0.0351)),
    "general16": ((0.311, 0.7), (0.699, 0.138), (0.799, 0.214)),
    "opaque16": ((0.0753, 0.176), (0.19, 0.0175), (0.0547, 0.0642)),
    "subpixel16": ((2.49, 1.9), (1.67, 2.39), (2.01, 0.873)),
    "tile8": ((0.217, 0.523), (0.511, 0.0919), (0.236, 0.22)),
    "tile20": ((0.132, 0.327), (0.354, 0.0798), (0.124, 0.327)),
    "far": (None, None, (0.412, 0.246)),
    "tile8, 256 channels": ((0.247, None), None, None),
    "gathered feature sums (ordinary16, tile20 in batches)": ((None, 0.106), None, None),
}
K_OF = {"features": K_FEATURES, "contributions": K_CONTRIB, "distortion": K_DISTORTION}
MARGIN_SHARE = 0.02  # pixels whose dominant / median id the bound cannot decide, of a case's covered pixels
# The four dense low-opacity cases cannot meet that share for the median id, whatever their seed: their pixels
# evaluate 225 to 240 entries of opacity <= 0.15, so the running A passes 0.5 in steps of ~0.005 against a margin
# of 8 (n_p + 1) 2^-24 ~ 1.1e-4 on either side of two entries.  Undecided pixels of their 960 on the host-built
# frame, recorded here; test_cases_reach_their_paths_and_decide_their_ids holds every other case to the share.
# An undecided pixel is not waved through: median_agrees accepts only a neighbour that a running A within the
# margin of the statement's can select.
MEDIAN_OPEN = {"ordinary16": 64, "thin16": 29, "general16": 27, "opaque16": 44}


def far_scene():
    """DU.far_scene() as a scene of blend_reference (one 64 x 64 image, 16-px tiles, focal length 3200 px)."""
    f = DU.far_scene()
    return dict(W=64, H=64, L=16, fx=3200.0, xyz=f["xyz"], cov3d=f["cov3d"], opacity=f["opacity"],
                color_logits=f["color_logits"], bg=np.zeros(3, np.float32))


def payload(n, C, W, H, seed=31):
    """Features of mixed sign and per-channel scale, and their cotangent."""
    f01, a, b = FU.random_features(n, C, seed)
    g = np.random.default_rng(seed + 1).uniform(-1, 1, (C, H, W)).astype(np.float32)
    return (a * f01 + b).astype(np.float32), g


def dist_cotangent(W, H, seed=41):
    return np.random.default_rng(seed).uniform(-1, 1, (H, W)).astype(np.float32)


# ---- host-built frames, their fp32 decisions, the statements --------------------------
_HOST = {}


class _Host:
    pass


def _host(name):
    if name in _HOST:
        return _HOST[name]
    h = _Host()
    if name == "far":
        h.sc, mutate = far_scene(), None
    else:
        h.sc, mutate = B.case_scene(name), B.CASES[name][1]
    h.name = name
    h.fr = fr = B.cpu_frame(h.sc)
    h.info = mutate(fr) if mutate else None
    h.em = B.whole_frame(fr, lambda t: R.emulate_chain(fr, t))
    nev, al = np.zeros(fr.W * fr.H, np.int64), np.zeros(fr.W * fr.H, np.float32)
    for em in h.em.values():
        nev[em["pix"]], al[em["pix"]] = em["neval"], em["A"]
    h.chains = B.whole_frame(fr, lambda t: R.chain(fr, t, neval=nev, alpha_fwd=al))
    for t, k in h.chains.items():
        bad = B.validate_termination(k, name)
        assert not bad, bad[:5]
    h.stmt = {}
    _HOST[name] = h
    return h


def feature_statement(h, C, grads=True):
    key = ("features", C, grads)
    if key not in h.stmt:
        fr = h.fr
        F, g = payload(len(fr.records), C, fr.W, fr.H)
        h.stmt[key] = F, g, {t: R.feature_tile(fr, t, k, F.astype(np.float64), g if grads else None)
                             for t, k in h.chains.items()}
    return h.stmt[key]


def contrib_statement(h):
    if "contrib" not in h.stmt:
        h.stmt["contrib"] = {t: R.contrib_tile(h.fr, k) for t, k in h.chains.items()}
    return h.stmt["contrib"]


def distortion_statement(h, nf, grads=True):
    key = ("distortion", nf, grads)
    if key not in h.stmt:
        g = dist_cotangent(h.fr.W, h.fr.H)
        h.stmt[key] = g, {t: R.distortion_tile(h.fr, t, k, nf, g if grads else None) for t, k in h.chains.items()}
    return h.stmt[key]


def partial_ratio(k, st, got, small):
    """Largest err / unit of one tile's partials [n, cells, 10] against the
    statement st (partials, M, M_dQ11_recentred); the entries `small` (sigma_y
    < 2 px) also against the recentred moments' own bound."""
    err = np.abs(np.asarray(got, np.float64) - st["partials"])
    nc = k["n_cell"]
    return max(R.ratio(err, st["M"], nc[None, :, None]),
               R.ratio(err[small][:, :, 4], st["M_dQ11_recentred"][small], nc[None, :]))


def undecided_dominant(k, cs, K):
    """Pixels whose fp64 top-two margin does not exceed the bound there."""
    return (cs["top1"] - cs["top2"]) <= K * (k["n_p"] + 1) * B.U24 * (cs["top1"] + cs["top2"])


def median_delta(k):
    return 8.0 * (k["n_p"] + 1) * B.U24


def undecided_median(k, ds):
    return ds["median_margin"] <= median_delta(k)


def median_agrees(k, ds, entry):
    """The median entry [P] against the statement's: equal where the margin
    decides; elsewhere one of its neighbours among the contributors, and one
    that a running A within the margin of the statement's can select."""
    decided = ~undecided_median(k, ds)
    near = (entry == ds["median_entry"]) | (entry == ds["median_prev"]) | (entry == ds["median_next"])
    return np.where(decided, entry == ds["median_entry"], near & R.median_consistent(ds, entry, median_delta(k)))


# ---- the statements, pinned on the CPU -------------------------------------------------
def test_feature_statement_equals_blend_statement():
    """With F = the records' colours and g_out = g_image, on a case with bg = 0
    and no clamped pixel, the feature statement's image and partials are
    blend_reference.reference_tile's."""
    h = _host("ordinary16")
    fr = h.fr
    assert not fr.bg.any()
    gi = B.case_cotangents(h.sc)[0]
    nev = np.zeros(fr.W * fr.H, np.int64)
    for em in h.em.values():
        nev[em["pix"]] = em["neval"]
    F = fr.records[:, 6:9].astype(np.float64)
    for t, k in h.chains.items():
        ref = B.reference_tile(fr, t, gi, neval=nev, flags=np.zeros(fr.W * fr.H, np.uint8))
        assert not ref["blocked"].any()
        st = R.feature_tile(fr, t, k, F, gi)
        assert np.abs(st["out"] - ref["image"]).max() <= 1e-12 * np.abs(ref["image"]).max()
        for c in range(9):
            a, b = st["partials"][0][:, :, c], ref["partials"][:, :, c]
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (t, B.COMPONENTS[c])
        assert not st["partials"][0][:, :, 9].any()
        assert np.allclose(st["M"][0][:, :, :9], ref["M"][:, :, :9], rtol=1e-12, atol=0)
        assert np.allclose(st["M_dQ11_recentred"][0], ref["M_dQ11_recentred"], rtol=1e-12, atol=0)


def _fd(loss, base, got_of, scale_of, rows, cols, what):
    worst = 0.0
    for i in rows:
        for c in cols:
            hh = 1e-6 * max(1.0, abs(base[i, c]))
            vp, vm = base.copy(), base.copy()
            vp[i, c] += hh
            vm[i, c] -= hh
            fd = (loss(vp) - loss(vm)) / (2 * hh)
            got = got_of(i, c)
            scale = max(abs(fd), scale_of(c))
            worst = max(worst, abs(fd - got) / scale)
            assert abs(fd - got) <= 1e-7 * scale, (what, i, c, fd, got)
    return worst


def _fd_frame():
    sc = B.fd_scene()
    fr = B.cpu_frame(sc)
    assert len(fr.entries(0)) == 6 and fr.cells == 1
    k = R.chain(fr, 0)
    assert (B.skip_exponent(fr.records[fr.entries(0)], k["xs"], k["ys"]) > B.SKIP_T + 1).all()
    assert k["A"].max() < 0.9 and not k["stopped"].any() and (k["ncontrib"] == 6).all()
    return sc, fr, k, fr.records[k["ids"]][:, list(B.REC_COL)].astype(np.float64)


def test_feature_statement_matches_finite_differences():
    """6 Gaussians on 8x8 pixels, C = 5 (two chunks): the autograd partials
    against central differences in fp64 -- the geometry of both chunks summed,
    every feature column of its own chunk, the columns past C exactly 0."""
    sc, fr, k, base = _fd_frame()
    F, g = payload(6, CPU_C, 8, 8)
    F = F.astype(np.float64)
    st = R.feature_tile(fr, 0, k, F, g)
    P = st["partials"]
    assert not P[1][:, :, 7:].any() and not st["M"][1][:, :, 7:].any()
    Fi = F[k["ids"]]
    loss_v = lambda v: R.feature_tile(fr, 0, R.chain(fr, 0, values=v), F, g)["loss"]
    loss_f = lambda f: R.feature_tile(fr, 0, k, F, g, fvalues=f)["loss"]
    geo = P.sum(0)[:, 0, :6]
    w1 = _fd(loss_v, base, lambda i, c: geo[i, c], lambda c: np.abs(geo[:, c]).max(), range(6), range(6), "geometry")
    dF = np.concatenate([P[0][:, 0, 6:10], P[1][:, 0, 6:7]], 1)
    w2 = _fd(loss_f, Fi, lambda i, c: dF[i, c], lambda c: np.abs(dF[:, c]).max(), range(6), range(CPU_C), "features")
    print(f"feature finite differences: worst relative difference {max(w1, w2):.3g}")


@pytest.mark.parametrize("nf", MAPS, ids=("linear", "inverse"))
def test_distortion_statement_matches_finite_differences(nf):
    """Both maps, d_z included; and nothing flows through the reference depth:
    sum_i dL/dm_i = 0 per pixel."""
    sc, fr, k, base = _fd_frame()
    g = dist_cotangent(8, 8)
    st = R.distortion_tile(fr, 0, k, nf, g)
    assert (st["ncontrib"] >= 3).all() and len(np.unique(fr.records[k["ids"], 9])) == 6
    P = st["partials"][:, 0]
    assert not P[:, 6:9].any()
    loss = lambda v: R.distortion_tile(fr, 0, R.chain(fr, 0, values=v), nf, g)["loss"]
    w = _fd(loss, base, lambda i, c: P[i, c], lambda c: np.abs(P[:, c]).max(), range(6), (0, 1, 2, 3, 4, 5, 9), nf)
    print(f"distortion finite differences ({nf}): worst relative difference {w:.3g}")
    dm = st["dL_dm"]
    assert (np.abs(dm.sum(0)) <= 1e-12 * np.abs(dm).sum(0)).all()


@pytest.mark.parametrize("name", CASES + ("far",))
def test_prefix_distortion_is_the_double_sum(name):
    h = _host(name)
    for nf in MAPS:
        _, sts = distortion_statement(h, nf, grads=False)
        for t, st in sts.items():
            brute = DU.brute_distortion(st["c"], st["m"][:, 0])
            assert (np.abs(st["D"] - brute) <= 1e-12 * np.maximum(brute, st["M_D"])).all(), (name, nf, t)


@pytest.mark.parametrize("name", CASES)
def test_contribution_sums_add_up(name):
    """The (entry, cell) sums of a Gaussian add up to the sum of its row of c."""
    h = _host(name)
    n = len(h.fr.records)
    rows, cells = np.zeros(n), np.zeros(n)
    for t, cs in contrib_statement(h).items():
        k = h.chains[t]
        np.add.at(rows, k["ids"], k["c"].sum(1))
        np.add.at(cells, k["ids"], cs["sum"].sum(1))
    assert rows.max() > 0 and np.abs(rows - cells).max() <= 1e-12 * rows.max()


# ---- the fp32 formulations set K --------------------------------------------------------
def _feature_ratios(h, wrong=None, guard=None):
    fr = h.fr
    F, g, sts = feature_statement(h, CPU_C)
    wf = wp = 0.0
    for t, k in h.chains.items():
        em = R.emulate_features(fr, t, F, g, wrong=wrong, guard=guard)
        st = sts[t]
        wf = max(wf, R.ratio(np.abs(em["out"] - st["out"]), st["M_out"], k["n_p"][:, None]))
        small = B.small_y(fr.records[k["ids"]])
        for j in range(R.chunks_of(CPU_C)):
            sj = dict(partials=st["partials"][j], M=st["M"][j], M_dQ11_recentred=st["M_dQ11_recentred"][j])
            wp = max(wp, partial_ratio(k, sj, em["partials"][j], small))
    return wf, wp


def _contrib_ratios(h):
    fr = h.fr
    sts = contrib_statement(h)
    worst = 0.0
    exact = True
    for t, k in h.chains.items():
        em, cs = R.emulate_contrib(fr, t), sts[t]
        nc = k["n_cell"][None, :]
        worst = max(worst, R.ratio(np.abs(em["sum"] - cs["sum"]), cs["sum"], nc),
                    R.ratio(np.abs(em["max"] - cs["max"]), cs["max"], nc),
                    R.ratio(np.abs(em["dom_w"] - cs["top1"]), cs["top1"], k["n_p"]))
        if (fr.records[k["ids"], 5] >= np.float32(1e-20)).all():
            exact &= np.array_equal(em["count"], cs["count"])
        decided = ~undecided_dominant(k, cs, K_CONTRIB)
        assert np.array_equal(em["dom_id"][decided], cs["dom_id"][decided])
    assert exact
    return worst


def _distortion_ratios(h, nf, wrong=None):
    fr = h.fr
    g, sts = distortion_statement(h, nf)
    wf = wp = 0.0
    for t, k in h.chains.items():
        em, st = R.emulate_distortion(fr, t, nf, g, wrong=wrong), sts[t]
        wf = max(wf, R.ratio(np.abs(em["D"] - st["D"]), st["M_D"], k["n_p"]))
        if wrong is None:
            wf = max(wf, R.ratio(np.abs(em["S"] - st["S"]), st["M_S"], k["n_p"]))
            assert np.array_equal(em["A"], em["em"]["A"])
            assert median_agrees(k, st, em["median_entry"]).all(), (h.name, nf, t)
        small = B.small_y(fr.records[k["ids"]])
        wp = max(wp, partial_ratio(k, st, em["partials"], small))
    return wf, wp


_MEASURED = {}


@pytest.mark.parametrize("name", CASES + ("far",))
def test_fp32_formulation_sets_K(name):
    """The documented formulations in numpy fp32 against the statements on a
    host-built frame of every case: 4 x the largest ratio stays below the
    family's K (the forced terminations validated in _host)."""
    h = _host(name)
    ff, fp = _feature_ratios(h)
    cc = _contrib_ratios(h)
    dd = [_distortion_ratios(h, nf) for nf in MAPS]
    print(f"{name}: fp32 formulation err / unit: features forward {ff:.3g}, partials {fp:.3g}; contributions {cc:.3g}; "
          f"distortion linear forward {dd[0][0]:.3g}, partials {dd[0][1]:.3g}; inverse forward {dd[1][0]:.3g}, "
          f"partials {dd[1][1]:.3g}")
    got = {"features": max(ff, fp), "contributions": cc, "distortion": max(max(d) for d in dd)}
    _MEASURED[name] = got
    for fam, v in got.items():
        assert 4.0 * v <= K_OF[fam], (fam, v)
        assert v <= K_CPU_MEASURED[fam] * 1.0005, (fam, v, "larger than the recorded measurement")


def test_K_is_four_times_the_measured_ratio():
    for fam, K in K_OF.items():
        assert K == max(8.0, float(np.ceil(4.0 * K_CPU_MEASURED[fam]))), fam


# ---- the statement must be able to fail ---------------------------------------------------
def test_wrong_row_moments_exceed_K():
    """(a) Row moments about row 0 instead of the nearest row: dQ11 of sub-pixel rows."""
    h = _host("subpixel16")
    _, wp = _feature_ratios(h, wrong="row0")
    _, wd = _distortion_ratios(h, None, wrong="row0")
    print(f"row moments about row 0: features {wp:.3g}, distortion {wd:.3g} units")
    assert wp > K_FEATURES and wd > K_DISTORTION


def test_wrong_terminating_entry_exceeds_K():
    """(b) The terminating entry given the live formula X + PG / T instead of X."""
    h = _host("opaque16")
    _, wp = _feature_ratios(h, wrong="terminating_live")
    _, wd = _distortion_ratios(h, None, wrong="terminating_live")
    print(f"terminating entry with the live formula: features {wp:.3g}, distortion {wd:.3g} units")
    assert wp > K_FEATURES and wd > K_DISTORTION


def test_wrong_unmasked_last_chunk_exceeds_K():
    """(c) The last chunk's cotangent of the channels >= C read from a non-zero guard plane."""
    h = _host("ordinary12")
    guard = np.full((h.fr.H, h.fr.W), 0.75, np.float32)
    _, wp = _feature_ratios(h, wrong="unmasked", guard=guard)
    assert wp > K_FEATURES


def test_wrong_unshifted_depths_exceed_K():
    """(d) The distortion evaluated on unshifted depths, where the spread is 2.5e-4 of the depth."""
    h = _host("far")
    for nf in MAPS:
        wf, _ = _distortion_ratios(h, nf, wrong="unshifted")
        print(f"unshifted depths ({nf}): {wf:.3g} units")
        assert wf > K_DISTORTION


# ---- the cases reach their paths -------------------------------------------------------------
def check_replay_reach(name, fr, chains, info):
    if name in ("ordinary16", "ordinary12", "thin16", "general16", "opaque16", "subpixel16", "tile20"):
        TBS.check_reach(name, fr, chains, info)
    deep = words = False
    for t, k in chains.items():
        z = fr.records[k["ids"], 9]
        for p in np.nonzero(k["ncontrib"] >= 3)[0]:
            deep |= len(np.unique(z[k["c"][:, p] > 0])) >= 3
            if deep:
                break
        words |= bool((k["cell_neval"] > 128).any())
    if name != "subpixel16":  # (one or two sub-pixel rows per pixel, by construction)
        assert deep, "no pixel with three contributors of distinct depths"
    if name in ("ordinary16", "thin16", "general16", "opaque16"):
        assert words, "no cell whose evaluated prefix spans three words"


@pytest.mark.parametrize("name", CASES + ("far",))
def test_cases_reach_their_paths_and_decide_their_ids(name):
    """On the statement alone: the paths, and the 2 % conditions -- the share
    of covered pixels whose dominant or median id the bound leaves open."""
    h = _host(name)
    check_replay_reach(name, h.fr, h.chains, h.info)
    cs = contrib_statement(h)
    covered = sum(int((k["ncontrib"] > 0).sum()) for k in h.chains.values())
    open_dom = sum(int((undecided_dominant(k, cs[t], K_CONTRIB) & (k["ncontrib"] > 0)).sum()) for t, k in h.chains.items())
    assert covered > 0 and open_dom <= MARGIN_SHARE * covered, (open_dom, covered)
    _, ds = distortion_statement(h, None, grads=False)  # (the weights, hence the margins, do not depend on the map)
    open_med = sum(int((undecided_median(k, ds[t]) & (k["ncontrib"] > 0)).sum()) for t, k in h.chains.items())
    print(f"{name}: covered {covered}, dominant id open at {open_dom}, median id open at {open_med}")
    assert open_med == MEDIAN_OPEN.get(name, open_med), "the recorded count is stale"
    if name not in MEDIAN_OPEN:
        assert open_med <= MARGIN_SHARE * covered, (open_med, covered)


# ---- the kernels --------------------------------------------------------------------------------
SENT = 7.0
GPU_CASES = CASES
BATCHES = [(0, 4), (4, 4), (8, 1)]  # tile20's nine cells


class Guarded:
    """A device buffer pre-filled with a sentinel, with a guard region behind
    it inside the same allocation that must come back untouched."""

    def __init__(self, shape, dev, dtype=torch.float32, fill=SENT, guard=1024, guard_fill=None):
        self.n = int(np.prod(shape))
        self.gf = fill if guard_fill is None else guard_fill
        self.full = torch.full((self.n + guard,), self.gf, dtype=dtype, device=dev)
        self.t = self.full[:self.n].view(shape)
        self.t.fill_(fill)

    def set(self, a):
        self.t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(self.t.device).view(self.t.shape))
        return self

    def intact(self):
        return bool((self.full[self.n:] == self.gf).all())

    def np(self):
        return self.t.cpu().numpy()


def _gpu(pkg, cuda, name):
    """test_blend_stage's frame of the case (the library's lists, slots and
    liveness words, the colour forward run), with the chains forced to the
    forward's terminations, validated."""
    r = TBS._frame(pkg, cuda, name, scene=far_scene() if name == "far" else None)
    if not hasattr(r, "chains"):
        fr = r.fr
        nev, al = r.fwd["neval"].cpu().numpy(), r.fwd["alpha"].cpu().numpy()
        r.chains = B.whole_frame(fr, lambda t: R.chain(fr, t, neval=nev, alpha_fwd=al))
        for t, k in r.chains.items():
            bad = B.validate_termination(k, name)
            assert not bad, bad[:5]
            assert np.array_equal(r.fwd["cell_neval"].cpu().numpy()[t], k["cell_neval"])
        r.stmt = {}
        r.worst = {}
    return r


def _replay_args(N, r, live):
    return N.GsReplayFrame(r.cam.to_struct(), r.cam.tiles_x, r.cam.tiles_y, N.ptr(r.ranges), N.ptr(r.sorted_gauss),
                           N.ptr(r.records), N.ptr(r.fwd["cell_neval"]), N.ptr(r.fwd["live"]) if live else None,
                           r.live_words if live else 0, r.T, r.n)


def _run(pkg, fn, args):
    N = pkg._native
    N.check(getattr(N.load(), fn)(C.byref(args), torch.cuda.current_stream().cuda_stream), fn)
    torch.cuda.synchronize()


def _note(r, family, v):
    r.worst[family] = max(r.worst.get(family, 0.0), v)
    return v


def _count(r, count):
    assert 0 <= count <= r.fr.cells
    return count or r.fr.cells


def _scratch(r, count, stride, dev):
    G_ = _count(r, count)
    return Guarded((r.T * G_, stride), dev), Guarded((r.T * G_,), dev, torch.uint8, fill=0, guard_fill=9)


def feat_forward(pkg, r, F, live=True):
    N = pkg._native
    dev = r.records.device
    Cn = F.shape[1]
    staged = pkg.rasterizer._stage_features(torch.from_numpy(np.ascontiguousarray(F)).to(dev))
    assert staged.shape == (R.chunks_of(Cn), r.n, 4)
    out = Guarded((Cn, r.fr.H, r.fr.W), dev)
    _run(pkg, "gs_blend_features_forward",
         N.GsFeatureFwdArgs(_replay_args(N, r, live), Cn, N.ptr(staged), N.ptr(out.t)))
    assert out.intact(), "written past the feature image"
    return staged, out


def feat_backward(pkg, r, staged, out, g_out, Cn, chunk, live=True, begin=0, count=0):
    N = pkg._native
    grads, flags = _scratch(r, count, N.GS_PARTIAL_STRIDE, r.records.device)
    a = N.GsFeatureBwdArgs(_replay_args(N, r, live), Cn, chunk, N.ptr(staged), N.ptr(out.t), N.ptr(g_out.t),
                           N.ptr(grads.t), N.ptr(flags.t), begin, count)
    _run(pkg, "gs_blend_features_backward", a)
    assert grads.intact() and flags.intact() and g_out.intact() and out.intact()
    return grads, flags


def check_partials(r, st_of, K, grads, flags, live=True, begin=0, count=0, zero_bits=()):
    """Every partial a backward wrote for the cells [begin, begin + count): all
    ten components within K units of the statement st_of(t), exactly 0 where no
    pixel of the cell evaluated the entry, the flags the expected set, every
    other slot its sentinel.  Returns the partials [T, cells, 10] (NaN where
    unwritten), the largest ratio, and per Gaussian the expected sums and the
    summed bounds."""
    fr = r.fr
    G_ = _count(r, count)
    g = grads.np().reshape(r.T, G_, 10)
    want, where = TBS.expected_slot_flags(r, r.chains, live, begin, G_)
    assert np.array_equal(flags.np(), want), "slot_live differs from the expected set"
    assert (g.reshape(-1, 10)[want == 0] == SENT).all(), "a partial written without its flag"
    full = np.full((r.T, fr.cells, 10), np.nan, np.float32)
    expect, bound = np.zeros((r.n, 10)), np.zeros((r.n, 10))
    worst = 0.0
    by_tile = {}
    for kk, (t, i, q) in where.items():
        by_tile.setdefault(t, []).append((kk // G_, i, q))
    for t, lst in by_tile.items():
        k, st = r.chains[t], st_of(t)
        rows, ii, qq = (np.array(v) for v in zip(*lst))
        got = g[rows, qq - begin]
        assert np.isfinite(got).all()
        full[rows, qq] = got
        dead = ~k["live"][ii, qq]
        assert not got[dead].any(), f"tile {t}: a partial of an entry no pixel of the cell evaluated is not 0"
        for c in zero_bits:
            assert not got[:, c].view(np.uint32).any(), f"component {c} is not +0"
        unit = (k["n_cell"][qq] + 1)[:, None] * B.U24 * st["M"][ii, qq]
        err = np.abs(got.astype(np.float64) - st["partials"][ii, qq])
        with np.errstate(divide="ignore", invalid="ignore"):
            rt = np.nan_to_num(np.where(err > 0, err / unit, 0.0), nan=np.inf)
        worst = max(worst, float(rt.max()))
        if not (rt <= K).all():
            j, c = np.unravel_index(int(np.argmax(rt)), rt.shape)
            raise AssertionError(f"{r.name}: tile {t} entry {ii[j]} cell {qq[j]} component {c}: {got[j, c]!r} vs fp64 "
                                 f"{st['partials'][ii[j], qq[j], c]!r}, {rt[j, c]:.3g} units of {unit[j, c]:.3g} (K = {K})")
        small = B.small_y(fr.records[k["ids"]])[ii]
        unit_r = (k["n_cell"][qq] + 1) * B.U24 * st["M_dQ11_recentred"][ii, qq]
        assert (err[small, 4] <= K * unit_r[small]).all(), f"{r.name}: tile {t}: dQ11 of a sub-2-px row"
        np.add.at(expect, k["ids"][ii], st["partials"][ii, qq])
        np.add.at(bound, k["ids"][ii], K * unit)
    return full, worst, expect, bound


def _chunk_statement(sts, j):
    return lambda t: dict(partials=sts[t]["partials"][j], M=sts[t]["M"][j], M_dQ11_recentred=sts[t]["M_dQ11_recentred"][j])


def _g_out(r, g, dev):
    """The cotangent with a non-zero guard of four planes behind it."""
    return Guarded(g.shape, dev, guard=4 * r.fr.H * r.fr.W, guard_fill=0.75).set(g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_feature_forward(pkg, cuda, name):
    """C in {1, 3, 4, 5, 9}: every pixel of every channel within K units; the
    same bits without the liveness bitmap."""
    r = _gpu(pkg, cuda, name)
    check_replay_reach(name, r.fr, r.chains, r.info)
    for Cn in (1, 3, 4, 5, 9):
        F, _, sts = feature_statement(r, Cn, grads=Cn in (1, 5, 9))
        _, out = feat_forward(pkg, r, F)
        got = out.np().reshape(Cn, -1)
        seen = np.zeros(r.fr.W * r.fr.H, bool)
        for t, k in r.chains.items():
            seen[k["pix"]] = True
            rt = _note(r, "features forward", R.ratio(np.abs(got[:, k["pix"]].T - sts[t]["out"]), sts[t]["M_out"],
                                                      k["n_p"][:, None]))
            assert rt <= K_FEATURES, (name, Cn, t, rt)
        assert not got[:, ~seen].any(), "a pixel of a tile without entries is not 0"
        _, nobits = feat_forward(pkg, r, F, live=False)
        assert torch.equal(nobits.t.view(torch.int32), out.t.view(torch.int32))
    print(f"GPU ratios {name}: features forward {r.worst['features forward']:.3g} (K = {K_FEATURES})")


@pytest.mark.gpu
def test_feature_forward_256_channels(pkg, cuda):
    """64 chunks on grid y, channel k scaled by its own factor: every channel within the bound."""
    r = _gpu(pkg, cuda, "tile8")
    Cn = 256
    F, _ = payload(r.n, Cn, r.fr.W, r.fr.H, seed=77)
    F = (F * (1.0 + 0.37 * np.arange(Cn))[None, :]).astype(np.float32)
    assert len(np.unique(np.abs(F).max(0))) == Cn
    _, out = feat_forward(pkg, r, F)
    got = out.np().reshape(Cn, -1)
    worst = 0.0
    for t, k in r.chains.items():
        st = R.feature_tile(r.fr, t, k, F.astype(np.float64))
        worst = max(worst, R.ratio(np.abs(got[:, k["pix"]].T - st["out"]), st["M_out"], k["n_p"][:, None]))
    print(f"GPU ratios tile8: features forward, 256 channels {worst:.3g} (K = {K_FEATURES})")
    assert worst <= K_FEATURES


def _feature_backward_case(pkg, r, Cn, live=True, batches=None):
    dev = r.records.device
    F, g, sts = feature_statement(r, Cn)
    staged, out = feat_forward(pkg, r, F)
    g_out = _g_out(r, g, dev)
    Q = r.fr.cells
    fulls, written = [], 0
    for j in range(R.chunks_of(Cn)):
        full = np.full((r.T, Q, 10), np.nan, np.float32)
        for begin, count in (batches or [(0, 0)]):
            grads, flags = feat_backward(pkg, r, staged, out, g_out, Cn, j, live, begin, count)
            part, w, _, _ = check_partials(r, _chunk_statement(sts, j), K_FEATURES, grads, flags, live, begin, count)
            _note(r, "features partials", w)
            sl = slice(begin, begin + _count(r, count))
            full[:, sl] = part[:, sl]
        fulls.append(full)
        written += int((~np.isnan(full[:, :, 0])).sum())
    return fulls, written


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in GPU_CASES if n != "tile20"])
def test_feature_backward(pkg, cuda, name):
    """Every chunk of C in {1, 5, 9}: all ten components of every written partial."""
    r = _gpu(pkg, cuda, name)
    for Cn in (1, 5, 9):
        _feature_backward_case(pkg, r, Cn)
    print(f"GPU ratios {name}: features partials {r.worst['features partials']:.3g} (K = {K_FEATURES})")


@pytest.mark.gpu
def test_feature_backward_tile20_batches_and_no_bitmap(pkg, cuda):
    r = _gpu(pkg, cuda, "tile20")
    for Cn in (1, 5, 9):
        one, n_one = _feature_backward_case(pkg, r, Cn)
        batched, _ = _feature_backward_case(pkg, r, Cn, batches=BATCHES)
        for a, b in zip(one, batched):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "a partial depends on its batch"
        _, n_nobits = _feature_backward_case(pkg, r, Cn, live=False)
        assert n_nobits > n_one, "the bitmap-free replay writes entries the bitmap skips"
    print(f"GPU ratios tile20: features partials {r.worst['features partials']:.3g} (K = {K_FEATURES})")


# ---- gs_gather_feature_partials ------------------------------------------------------------------
def _feature_gather_args(N, n, vis, rects, pair_offset, grads, flags, groups, acc, sums, df, stride, cb, cc, facc):
    return N.GsFeatureGatherArgs(n, N.ptr(vis), N.ptr(rects), N.ptr(pair_offset), N.ptr(grads), N.ptr(flags), groups, acc,
                                 N.ptr(sums), N.ptr(df), stride, cb, cc, facc)


@pytest.mark.gpu
@pytest.mark.parametrize("name,batches", [("ordinary16", None), ("tile20", BATCHES)])
def test_feature_gather_on_the_real_partials(pkg, cuda, name, batches):
    """Per chunk and batch, with the accumulate / feature_accumulate sequence
    of rasterizer._feature_backward: the geometry sums and d_features within
    the summed bounds; grad_sums[:, 6:10] zeroed by the first call, untouched
    afterwards."""
    N = pkg._native
    r = _gpu(pkg, cuda, name)
    Cn = 9
    F, g, sts = feature_statement(r, Cn)
    staged, out = feat_forward(pkg, r, F)
    g_out = _g_out(r, g, cuda)
    sums, df = Guarded((r.n, 10), cuda), Guarded((r.n, Cn), cuda)
    expect, bound = np.zeros((r.n, 6 + Cn)), np.zeros((r.n, 6 + Cn))
    have = False
    for j in range(R.chunks_of(Cn)):
        cb, cc = 4 * j, min(4, Cn - 4 * j)
        for b, (begin, count) in enumerate(batches or [(0, 0)]):
            grads, flags = feat_backward(pkg, r, staged, out, g_out, Cn, j, True, begin, count)
            _, _, e, bd = check_partials(r, _chunk_statement(sts, j), K_FEATURES, grads, flags, True, begin, count)
            expect[:, :6] += e[:, :6]
            bound[:, :6] += bd[:, :6]
            expect[:, 6 + cb:6 + cb + cc] += e[:, 6:6 + cc]
            bound[:, 6 + cb:6 + cb + cc] += bd[:, 6:6 + cc]
            a = _feature_gather_args(N, r.n, r.frame.vis, r.frame.rects, r.frame.pair_offset, grads.t, flags.t,
                                     _count(r, count), 1 if have else 0, sums.t, df.t, Cn, cb, cc, 1 if b else 0)
            _run(pkg, "gs_gather_feature_partials", a)
            have = True
            assert sums.intact() and df.intact()
            assert not sums.np()[:, 6:].view(np.uint32).any(), "grad_sums[:, 6:10] is not +0"
    got = np.concatenate([sums.np()[:, :6], df.np()], 1).astype(np.float64)
    err = np.abs(got - expect)
    assert (err <= bound + 1e-30).all(), "gathered sums outside the summed bounds"
    with np.errstate(divide="ignore", invalid="ignore"):
        w = float(np.nan_to_num(np.where(err > 0, err / (bound / K_FEATURES), 0.0), nan=np.inf).max())
    print(f"GPU ratios {name}: features gathered {w:.3g} (K = {K_FEATURES})")


def _synthetic(cuda, c):
    return {k: torch.tensor(c[k].view(np.int32) if c[k].dtype == np.uint32 else c[k], device=cuda)
            for k in ("vis", "rects", "pair_offset", "live")}


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [1, 2, 3, 4, 5, 9, 16])
def test_feature_gather_integer_partials_exact(pkg, cuda, ng):
    """Integer partials (test_gather_partials.make_case: a Gaussian with 300
    slots, invisible ones, dead flags between live ones), all three lane
    layouts: exact sums; the channel windows (0,4), (4,1), (8,3) into rows of
    stride 13; columns outside the window and rows >= n keep their sentinel."""
    from test_gather_partials import make_case
    N = pkg._native
    rng = np.random.default_rng(240 + ng)
    stride = 13
    for n in (1, 33, 257, 1000):
        c = make_case(rng, n, ng)
        assert n < 20 or (c["own"].max() == 300 and c["hidden"].any() and (c["terms"][c["own"] > 0] == 0).any())
        dev = _synthetic(cuda, c)
        part = torch.tensor(c["part"], device=cuda)
        want = c["want"].astype(np.float32)
        for cb, cc in ((0, 4), (4, 1), (8, 3)):
            for acc, facc in ((0, 0), (1, 1), (0, 1), (1, 0)):
                before_s = rng.integers(-100, 101, (n + 1, 10)).astype(np.float32)
                before_f = rng.integers(-100, 101, (n + 1, stride)).astype(np.float32)
                before_s[n], before_f[n] = SENT, SENT
                sums, df = torch.tensor(before_s, device=cuda), torch.tensor(before_f, device=cuda)
                a = _feature_gather_args(N, n, dev["vis"], dev["rects"], dev["pair_offset"], part, dev["live"], ng, acc,
                                         sums, df, stride, cb, cc, facc)
                _run(pkg, "gs_gather_feature_partials", a)
                es, ef = before_s.copy(), before_f.copy()
                es[:n, :6] = want[:, :6] + (before_s[:n, :6] if acc else 0)
                if not acc:
                    es[:n, 6:] = 0
                ef[:n, cb:cb + cc] = want[:, 6:6 + cc] + (before_f[:n, cb:cb + cc] if facc else 0)
                assert np.array_equal(sums.cpu().numpy(), es), (ng, n, cb, cc, acc, facc)
                assert np.array_equal(df.cpu().numpy(), ef), (ng, n, cb, cc, acc, facc)


# ---- contributions ------------------------------------------------------------------------------------
def contributions(pkg, r, live=True, begin=0, count=0, dominant=True):
    N = pkg._native
    dev = r.records.device
    part, flags = _scratch(r, count, N.GS_CONTRIB_STRIDE, dev)
    did = Guarded((r.fr.H * r.fr.W,), dev, torch.int32, fill=-7, guard_fill=9)
    dw = Guarded((r.fr.H * r.fr.W,), dev)
    a = N.GsContribArgs(_replay_args(N, r, live), N.ptr(part.t), N.ptr(flags.t), begin, count,
                        N.ptr(did.t) if dominant else None, N.ptr(dw.t) if dominant else None)
    _run(pkg, "gs_blend_contributions", a)
    assert part.intact() and flags.intact() and did.intact() and dw.intact()
    return part, flags, did, dw


def check_contributions(r, part, flags, live=True, begin=0, count=0):
    fr = r.fr
    G_ = _count(r, count)
    cs_all = contrib_statement(r)
    p = part.np().reshape(r.T, G_, 4)
    want, where = TBS.expected_slot_flags(r, r.chains, live, begin, G_)
    assert np.array_equal(flags.np(), want), "slot_live differs from the expected set"
    assert (p.reshape(-1, 4)[want == 0] == SENT).all()
    full = np.full((r.T, fr.cells, 4), np.nan, np.float32)
    by_tile = {}
    for kk, (t, i, q) in where.items():
        by_tile.setdefault(t, []).append((kk // G_, i, q))
    worst = 0.0
    for t, lst in by_tile.items():
        k, cs = r.chains[t], cs_all[t]
        rows, ii, qq = (np.array(v) for v in zip(*lst))
        got = p[rows, qq - begin]
        full[rows, qq] = got
        assert not got[:, 3].view(np.uint32).any()
        nc = k["n_cell"][qq]
        worst = max(worst, R.ratio(np.abs(got[:, 0] - cs["sum"][ii, qq]), cs["sum"][ii, qq], nc),
                    R.ratio(np.abs(got[:, 1] - cs["max"][ii, qq]), cs["max"][ii, qq], nc))
        if (fr.records[k["ids"], 5] >= np.float32(1e-20)).all():
            assert np.array_equal(got[:, 2], cs["count"][ii, qq].astype(np.float32)), (r.name, t)
        else:
            assert (got[:, 2] == np.rint(got[:, 2])).all() and (got[:, 2] <= 64).all()
    assert worst <= K_CONTRIB, (r.name, worst)
    return full, _note(r, "contributions", worst)


def check_dominant(r, did, dw):
    cs_all = contrib_statement(r)
    ids, wts = did.np(), dw.np()
    seen = np.zeros(r.fr.W * r.fr.H, bool)
    worst, open_px, covered = 0.0, 0, 0
    for t, k in r.chains.items():
        cs = cs_all[t]
        pix = k["pix"]
        seen[pix] = True
        worst = max(worst, R.ratio(np.abs(wts[pix] - cs["top1"]), cs["top1"], k["n_p"]))
        und = undecided_dominant(k, cs, K_CONTRIB) & (cs["top1"] > 0)
        assert np.array_equal(ids[pix][~und], cs["dom_id"][~und]), (r.name, t)
        assert ((ids[pix][und] == cs["dom_id"][und]) | (ids[pix][und] == cs["second_id"][und])).all()
        none = cs["top1"] == 0
        assert (ids[pix][none] == -1).all() and not wts[pix][none].view(np.uint32).any()
        open_px, covered = open_px + int(und.sum()), covered + int((cs["top1"] > 0).sum())
    assert (ids[~seen] == -1).all() and not wts[~seen].any()
    assert worst <= K_CONTRIB and open_px <= MARGIN_SHARE * covered, (r.name, worst, open_px, covered)
    return _note(r, "dominant weight", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_contributions(pkg, cuda, name):
    r = _gpu(pkg, cuda, name)
    part, flags, did, dw = contributions(pkg, r)
    one, _ = check_contributions(r, part, flags)
    check_dominant(r, did, dw)
    if name == "tile20":
        ids = Guarded((r.fr.H * r.fr.W,), cuda, torch.int32, fill=-7)
        full = np.full_like(one, np.nan)
        for begin, count in BATCHES:
            part, flags, d2, w2 = contributions(pkg, r, True, begin, count)
            b, _ = check_contributions(r, part, flags, True, begin, count)
            full[:, begin:begin + count] = b[:, begin:begin + count]
            wrote = d2.t != -7
            assert torch.equal(d2.t[wrote], did.t[wrote]) and torch.equal(w2.t[wrote], dw.t[wrote])
            ids.t[wrote] = d2.t[wrote]
        assert np.array_equal(full.view(np.uint32), one.view(np.uint32)), "a partial depends on its batch"
        assert torch.equal(ids.t, did.t), "the batches' cells do not cover the dominant map"
        part, flags, d3, w3 = contributions(pkg, r, live=False)
        nobits, _ = check_contributions(r, part, flags, live=False)
        assert np.isnan(one).sum() > np.isnan(nobits).sum()
        check_dominant(r, d3, w3)
        part, flags, d4, _ = contributions(pkg, r, dominant=False)
        assert (d4.t == -7).all()
    print(f"GPU ratios {name}: contributions {r.worst['contributions']:.3g}, dominant weight "
          f"{r.worst['dominant weight']:.3g} (K = {K_CONTRIB})")


def contrib_partials_case(rng, n, ng):
    """test_gather_partials.make_case with contribution partials (sum, max,
    count, reserved = NaN) of small integers; the counts of a 300-slot
    Gaussian with a live flag are 2^17 + 1 each and add up to an odd total
    above 2^24, which no fp32 holds.  Returns the case, the partials, per
    Gaussian (sum, max, count) and the live flags."""
    from test_gather_partials import GUARD as SLOT_GUARD, make_case
    c = make_case(rng, n, ng)
    T = c["T"]
    live = c["live"].astype(bool)
    part = np.zeros((T + SLOT_GUARD, ng, 4), np.float32)
    part[:, :, 0] = rng.integers(0, 9, (T + SLOT_GUARD, ng))
    part[:, :, 1] = rng.integers(0, 1000, (T + SLOT_GUARD, ng))
    part[:, :, 2] = rng.integers(0, 65, (T + SLOT_GUARD, ng))
    slots = lambda g: slice(int(c["pair_offset"][g]), int(c["pair_offset"][g]) + int(c["own"][g]))
    for g in np.nonzero(c["own"] == 300)[0]:
        on = np.argwhere(live[slots(g)])
        if len(on):
            part[slots(g), :, 2] = 2.0 ** 17 + 1.0
            if len(on) % 2 == 0:
                part[slots(g).start + on[0][0], on[0][1], 2] += 1.0
    want = np.zeros((n, 3), np.int64)
    for g in range(n):
        v = part[slots(g)][live[slots(g)]].astype(np.int64)
        want[g] = (v[:, 0].sum(), v[:, 1].max(initial=0), v[:, 2].sum())
    part[~live] = np.nan
    part[T:] = np.nan
    part[:, :, 3] = np.nan
    return c, part, want, live


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [1, 2, 3, 4, 5, 9, 16])
def test_contrib_accumulate_integer_partials_exact(pkg, cuda, ng):
    """Integer partials: sums, max, int64 counts (one Gaussian's total above
    2^24, odd) and views under first_batch 1 then 0, exact; vis == 0 rows keep
    their sentinel."""
    N = pkg._native
    rng = np.random.default_rng(340 + ng)
    for n in (1, 33, 257, 1000):
        c, part, want, live = contrib_partials_case(rng, n, ng)
        assert n < 20 or (want[:, 2].max() > 2 ** 24 and want[:, 2].max() % 2 == 1)
        dev = _synthetic(cuda, c)
        dpart = torch.tensor(part, device=cuda)
        hidden = c["vis"] == 0
        ws0 = rng.integers(0, 50, n + 1).astype(np.float32)
        wm0 = rng.integers(0, 500, n + 1).astype(np.float32)
        px0, vw0 = rng.integers(0, 1000, n + 1), rng.integers(0, 5, n + 1).astype(np.int32)
        ws, wm = torch.tensor(ws0, device=cuda), torch.tensor(wm0, device=cuda)
        px, vw = torch.tensor(px0, device=cuda), torch.tensor(vw0, device=cuda)
        assert px.dtype == torch.int64 and vw.dtype == torch.int32
        e_ws, e_wm, e_px, e_vw = ws0.copy(), wm0.copy(), px0.copy(), vw0.copy()
        seen = np.concatenate([~hidden, [False]])
        for first in (1, 0):
            a = N.GsContribGatherArgs(n, N.ptr(dev["vis"]), N.ptr(dev["rects"]), N.ptr(dev["pair_offset"]), N.ptr(dpart),
                                      N.ptr(dev["live"]), ng, first, N.ptr(ws), N.ptr(wm), N.ptr(px), N.ptr(vw))
            _run(pkg, "gs_contrib_accumulate", a)
            e_ws[:n][~hidden] += want[~hidden, 0]
            e_wm[:n][~hidden] = np.maximum(e_wm[:n][~hidden], want[~hidden, 1])
            e_px[:n][~hidden] += want[~hidden, 2]
            e_vw[seen] += first
            assert np.array_equal(ws.cpu().numpy(), e_ws) and np.array_equal(wm.cpu().numpy(), e_wm), (ng, n, first)
            assert np.array_equal(px.cpu().numpy(), e_px) and np.array_equal(vw.cpu().numpy(), e_vw), (ng, n, first)


# ---- distortion -------------------------------------------------------------------------------------------
def _nf(nf):
    return (0.0, 0.0) if nf is None else tuple(float(v) for v in nf)


def dist_forward(pkg, r, nf, live=True):
    N = pkg._native
    dev = r.records.device
    H, W = r.fr.H, r.fr.W
    o = dict(D=Guarded((H * W,), dev), moments=Guarded((2, H * W), dev), median_depth=Guarded((H * W,), dev),
             median_id=Guarded((H * W,), dev, torch.int32, fill=-7, guard_fill=9))
    a = N.GsDistortionFwdArgs(_replay_args(N, r, live), *_nf(nf), N.ptr(o["D"].t), N.ptr(o["moments"].t),
                              N.ptr(o["median_depth"].t), N.ptr(o["median_id"].t))
    _run(pkg, "gs_blend_distortion_forward", a)
    assert all(v.intact() for v in o.values())
    return o


def dist_backward(pkg, r, nf, fwd, g_out, live=True, begin=0, count=0):
    N = pkg._native
    grads, flags = _scratch(r, count, N.GS_PARTIAL_STRIDE, r.records.device)
    a = N.GsDistortionBwdArgs(_replay_args(N, r, live), *_nf(nf), N.ptr(fwd["D"].t), N.ptr(fwd["moments"].t),
                              N.ptr(g_out.t), N.ptr(grads.t), N.ptr(flags.t), begin, count)
    _run(pkg, "gs_blend_distortion_backward", a)
    assert grads.intact() and flags.intact() and g_out.intact()
    return grads, flags


def check_dist_forward(r, nf, o):
    _, sts = distortion_statement(r, nf)
    D, mom = o["D"].np(), o["moments"].np()
    mz, mid = o["median_depth"].np(), o["median_id"].np()
    alpha = r.fwd["alpha"].cpu().numpy().reshape(-1)
    seen = np.zeros(r.fr.W * r.fr.H, bool)
    worst = 0.0
    open_px = covered = 0
    for t, k in r.chains.items():
        st, pix = sts[t], k["pix"]
        seen[pix] = True
        worst = max(worst, R.ratio(np.abs(D[pix] - st["D"]), st["M_D"], k["n_p"]),
                    R.ratio(np.abs(mom[1][pix] - st["S"]), st["M_S"], k["n_p"]))
        # (the colour forward clamps its alpha to [0, 1]; A_n of these chains never leaves it)
        assert np.array_equal(mom[0][pix].view(np.uint32), alpha[pix].view(np.uint32)), "A_n is not the forward's alpha"
        pos = {int(g): i for i, g in enumerate(k["ids"])}
        entry = np.array([pos.get(int(g), -2) if g >= 0 else -1 for g in mid[pix]])
        assert median_agrees(k, st, entry).all(), (r.name, nf, t)
        z = r.fr.records[:, 9]
        has = entry >= 0
        assert np.array_equal(mz[pix][has].view(np.uint32), z[mid[pix][has]].view(np.uint32)), "median_depth"
        assert not mz[pix][~has].view(np.uint32).any()
        open_px += int((undecided_median(k, st) & (k["ncontrib"] > 0)).sum())
        covered += int((k["ncontrib"] > 0).sum())
    assert (mid[~seen] == -1).all() and not D[~seen].any() and not mom[:, ~seen].any() and not mz[~seen].any()
    assert worst <= K_DISTORTION, (r.name, nf, worst)
    if r.name not in MEDIAN_OPEN:
        assert open_px <= MARGIN_SHARE * covered
    return _note(r, "distortion forward", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES + ("far",))
def test_distortion(pkg, cuda, name):
    """Both maps: D, S_n, A_n, the median; every partial (six geometry values
    and d_z within K units, components 6, 7, 8 the bits of +0); on tile20 the
    batches and the replay without the bitmap."""
    N = pkg._native
    r = _gpu(pkg, cuda, name)
    check_replay_reach(name, r.fr, r.chains, r.info)
    for nf in MAPS:
        g, sts = distortion_statement(r, nf)
        fwd = dist_forward(pkg, r, nf)
        check_dist_forward(r, nf, fwd)
        nobits = dist_forward(pkg, r, nf, live=False)
        for key in fwd:
            assert torch.equal(nobits[key].t.view(torch.int32), fwd[key].t.view(torch.int32)), key
        g_out = Guarded(g.shape, cuda, guard_fill=0.75).set(g)
        st_of = lambda t: sts[t]
        grads, flags = dist_backward(pkg, r, nf, fwd, g_out)
        one, w, expect, bound = check_partials(r, st_of, K_DISTORTION, grads, flags, zero_bits=(6, 7, 8))
        _note(r, "distortion partials", w)
        # gathered onto known sums with accumulate = 1: within the summed bounds, the colour columns' bits unchanged
        before = np.random.default_rng(5).uniform(-1, 1, (r.n, 10)).astype(np.float32) * 1e-3
        sums = Guarded((r.n, 10), cuda).set(before)
        ga = N.GsProjectBwdArgs()
        ga.g.n = r.n
        ga.vis, ga.rects, ga.pair_offset = N.ptr(r.frame.vis), N.ptr(r.frame.rects), N.ptr(r.frame.pair_offset)
        ga.pair_grads, ga.slot_live, ga.grad_sums, ga.partial_groups = N.ptr(grads.t), N.ptr(flags.t), N.ptr(sums.t), r.fr.cells
        N.check(N.load().gs_gather_partials(C.byref(ga), 1, torch.cuda.current_stream().cuda_stream), "gs_gather_partials")
        torch.cuda.synchronize()
        got = sums.np()
        assert sums.intact() and np.array_equal(got[:, 6:9].view(np.uint32), before[:, 6:9].view(np.uint32))
        err = np.abs(got.astype(np.float64) - (before.astype(np.float64) + expect))
        slack = bound + 4.0 * B.U24 * (np.abs(before) + np.abs(expect))  # (the addition onto the sums held before)
        assert (err <= slack).all(), "gathered sums outside the summed bounds"
        if name == "tile20":
            full = np.full_like(one, np.nan)
            for begin, count in BATCHES:
                gb, fb = dist_backward(pkg, r, nf, fwd, g_out, True, begin, count)
                b, _, _, _ = check_partials(r, st_of, K_DISTORTION, gb, fb, True, begin, count, zero_bits=(6, 7, 8))
                full[:, begin:begin + count] = b[:, begin:begin + count]
            assert np.array_equal(full.view(np.uint32), one.view(np.uint32)), "a partial depends on its batch"
            gn, fn_ = dist_backward(pkg, r, nf, fwd, g_out, live=False)
            nb, w, _, _ = check_partials(r, st_of, K_DISTORTION, gn, fn_, live=False, zero_bits=(6, 7, 8))
            _note(r, "distortion partials", w)
            assert np.isnan(one).sum() > np.isnan(nb).sum()
    print(f"GPU ratios {name}: distortion forward {r.worst['distortion forward']:.3g}, partials "
          f"{r.worst['distortion partials']:.3g} (K = {K_DISTORTION})")
