"""The screen-space low-pass filter on the GPU (gs_screen_filter;
RenderSettings.screen_filter / filter_compensate).

Stage level: gs_project_forward / gs_project_backward / _pose / _adam through
the C ABI on the populations of tests/test_project_stage.py, against the
filtered fp64 statement of tests/screen_filter_util.py by that file's quantile
rule (the kernel's median, p90, p99 and max row-relative errors each at most
4 x the fp32 statement's, + 1e-7).  End to end: GaussianRenderer.render against
the pinned oracle on the equivalent scene (screen_filter_util), image 1e-4,
gradients 1e-4 of scale + 1e-7 after the pull-back through the map."""
import ctypes as C
import dataclasses  # noqa: F401

import numpy as np
import pytest
import torch

import features_util as FU
import golden_io as G
import project_reference as PR
import screen_filter_util as SF
import test_project_stage as TPS
from test_project_stage import camera, case_inputs, cotangents, population, quantile_errors, vis_flips  # noqa: F401

pytestmark = pytest.mark.gpu

FILTERS = [(0.1, False), (0.1, True), (0.3, False), (0.3, True)]
POPS = ("plain", "needles", "posed", "radius_clamp")
SIZES = lambda pop: (257, TPS.SIZES[pop])
_np = FU.np_


def _stage_cases(configs):
    return [(p, n, c, s, comp) for p in POPS for n in SIZES(p) for c in configs for s, comp in FILTERS]


_REFS: dict = {}
_FWD: dict = {}


def references(pop, n, config, s, comp):
    """fp64 and fp32 filtered statement, forward and backward, of one case (computed once)."""
    key = (pop, n, config, s, comp)
    if key not in _REFS:
        cam = camera(pop)
        d, deg, logit = case_inputs(pop, n, config)
        cot = cotangents(pop, n, config)
        r = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            r[name] = dict(fwd=SF.forward(cam, d, s, comp, dt, deg, logit),
                           bwd=SF.backward(cam, d, s, comp, *cot, dt, deg, logit))
        _REFS[key] = r
    return _REFS[key]


def gpu_forward(pkg, cuda, pop, n, config, s, comp, cache=True):
    """gs_project_forward with the filter in the trailing field (guard rows behind every output)."""
    key = (pop, n, config, s, comp)
    if cache and key in _FWD:
        return _FWD[key]
    N = pkg._native
    lib = N.load()
    d, deg, logit = case_inputs(pop, n, config)
    cs, gst, dd = TPS._structs(pkg, cuda, pop, d, deg, logit)
    nan = float("nan")
    nblk = (n + 255) // 256
    g = TPS._guarded
    o = dict(means2d=g(n, 2, torch.float32, nan, cuda), conics=g(n, 4, torch.float32, nan, cuda),
             radii=g(n, 0, torch.float32, nan, cuda), vis=g(n, 0, torch.uint8, 7, cuda),
             records=g(n, 12, torch.float32, nan, cuda), rects=g(n, 2, torch.int32, -7, cuda),
             depth_keys=g(n, 0, torch.int32, -7, cuda), key_minmax=g(2 * nblk, 0, torch.int32, -7, cuda))
    a = N.GsProjectArgs(cs, gst, *(N.ptr(o[k]) for k in ("means2d", "conics", "radii", "vis", "records", "rects",
                                                          "depth_keys")), 0, 32, N.ptr(o["key_minmax"]),
                        N.GsScreenFilter(s, 1 if comp else 0))
    N.check(lib.gs_project_forward(C.byref(a), torch.cuda.current_stream().cuda_stream), "gs_project_forward")
    torch.cuda.synchronize()
    fills = dict(means2d=nan, conics=nan, radii=nan, vis=7, records=nan, rects=-7, depth_keys=-7, key_minmax=-7)
    for k, t in o.items():
        rows = 2 * nblk if k == "key_minmax" else n
        assert TPS._guard_intact(t, rows, fills[k]), f"{k}: written past row {rows}"
    res = {k: t[:(2 * nblk if k == "key_minmax" else n)] for k, t in o.items()}
    res["_inputs"], res["_structs"] = dd, (cs, gst)
    if cache:
        _FWD[key] = res
    return res


@pytest.mark.parametrize("pop,n,config,s,comp", _stage_cases(["hot", "cov_cot"]))
def test_project_forward_filtered(pkg, cuda, pop, n, config, s, comp):
    out = gpu_forward(pkg, cuda, pop, n, config, s, comp)
    ref = references(pop, n, config, s, comp)
    r64, r32 = ref["f64"]["fwd"], ref["f32"]["fwd"]
    name = f"{pop}[{n}] {config} s={s} comp={comp}"
    print(name)
    cpu = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}
    vis = cpu["vis"].astype(bool)
    assert set(np.unique(cpu["vis"])) <= {0, 1}
    vis_flips(name, vis, r64)
    errs = []
    for k in ("means2d", "conics", "radii"):
        errs += quantile_errors(k, cpu[k], r32[k].numpy().reshape(n, -1), r64[k].numpy().reshape(n, -1))
    both = vis & r64["vis"].numpy()
    rec = cpu["records"]
    assert both.any()
    errs += quantile_errors("opacity", rec[:, 5:6], r32["opacity"].numpy()[:, None], r64["opacity"].numpy()[:, None], both)
    assert not errs, errs
    # the record repeats the filtered conic bit for bit
    assert np.array_equal(rec[vis][:, [0, 1, 2, 3]], np.concatenate([cpu["means2d"], cpu["conics"][:, [0, 3]]], 1)[vis])
    assert np.array_equal(rec[vis][:, 4], (cpu["conics"][:, 1] + cpu["conics"][:, 2])[vis])
    # rectangles, keys and the block key range: exact, from the kernel's own (filtered) floats
    z = np.where(vis, rec[:, 9], 1.0).astype(np.float32)
    rects, word11, keys, mm, ok = TPS.expected_integers(cpu["means2d"], cpu["radii"], z, vis)
    assert np.array_equal(cpu["rects"].view(np.uint32), rects)
    assert np.array_equal(rec[vis][:, 11].view(np.uint32), word11[vis])
    assert np.array_equal(cpu["depth_keys"].view(np.uint32), keys)
    assert np.array_equal(cpu["key_minmax"].view(np.uint32), mm)
    # the filter is there: the unfiltered statement's conics are far from these
    plain = PR.forward(camera(pop), case_inputs(pop, n, config)[0], torch.float64, 0, TPS.CONFIGS[config][2])
    far = TPS.row_rel(cpu["conics"][both], plain["conics"].numpy().reshape(n, -1)[both], "conics")
    assert far.max() > 1e-2
    ratio = r64["ratio"].numpy()
    if pop == "radius_clamp" and n == TPS.SIZES[pop]:
        floored = ratio <= SF.RHO_FLOOR
        assert floored.sum() == 1000 and not (np.abs(ratio / SF.RHO_FLOOR - 1) < 1e-3).any()
        if comp:  # the floored rows carry sqrt(floor) times their opacity
            op = torch.sigmoid(population(pop, n)["opacity"].double()).numpy()
            sel = floored & both
            assert sel.any() and np.allclose(rec[sel, 5], op[sel] * np.sqrt(SF.RHO_FLOOR), rtol=1e-6, atol=0)


@pytest.mark.parametrize("pop,config", [(p, c) for p in POPS for c in ("hot", "cov_cot")])
def test_zero_variance_is_the_unfiltered_call(pkg, cuda, pop, config):
    """s = 0 with the flag set: every output bit for bit the call with the field zeroed."""
    n = TPS.SIZES[pop]
    a = gpu_forward(pkg, cuda, pop, n, config, 0.0, True, cache=False)
    b = gpu_forward(pkg, cuda, pop, n, config, 0.0, False, cache=False)
    c = TPS.gpu_forward(pkg, cuda, pop, n, config)  # (the argument struct built without the field)
    for k in ("means2d", "conics", "radii", "vis", "records", "rects", "depth_keys", "key_minmax"):
        for other in (b, c):
            x, y = a[k].contiguous(), other[k].contiguous()
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


# ------------------------------------------------------------ backward ----
def _bwd_args(pkg, cuda, pop, n, config, s, comp):
    N = pkg._native
    kind, deg, logit, _ = TPS.CONFIGS[config]
    fwd = gpu_forward(pkg, cuda, pop, n, config, s, comp)
    cs, gst = fwd["_structs"]
    acc, gm, gc = (None if t is None else t.to(cuda) for t in cotangents(pop, n, config))
    nan = float("nan")
    g = TPS._guarded
    o = dict(d_xyz=g(n, 3, torch.float32, nan, cuda), d_color_logits=g(n, 3, torch.float32, nan, cuda),
             d_opacity=g(n, 0, torch.float32, nan, cuda))
    if kind == "raw":
        o.update(d_scaling=g(n, 3, torch.float32, nan, cuda), d_rotation=g(n, 4, torch.float32, nan, cuda))
    else:
        o["d_cov3d"] = g(n, 9, torch.float32, nan, cuda)
    rects = torch.zeros((n, 2), dtype=torch.int32, device=cuda)
    pair_offset = torch.zeros((n,), dtype=torch.int32, device=cuda)
    a = N.GsProjectBwdArgs(cs, gst, N.ptr(fwd["means2d"]), N.ptr(fwd["conics"]), N.ptr(fwd["vis"]), N.ptr(rects),
                           N.ptr(pair_offset), None, None, N.ptr(gm), N.ptr(gc), N.ptr(o["d_xyz"]),
                           N.ptr(o.get("d_cov3d")), N.ptr(o.get("d_scaling")), N.ptr(o.get("d_rotation")),
                           N.ptr(o["d_color_logits"]), N.ptr(o["d_opacity"]), None, None, N.ptr(acc), 0,
                           N.GsScreenFilter(s, 1 if comp else 0))
    return a, o, (fwd, acc, gm, gc, rects, pair_offset)


def gpu_backward(pkg, cuda, pop, n, config, s, comp, pose=False):
    N = pkg._native
    lib = N.load()
    a, o, keep = _bwd_args(pkg, cuda, pop, n, config, s, comp)
    stream = torch.cuda.current_stream().cuda_stream
    d_view = None
    if pose:
        rows = (n + N.GS_POSE_BLOCK - 1) // N.GS_POSE_BLOCK
        partials = torch.empty((rows, N.GS_POSE_ROW), dtype=torch.float64, device=cuda)
        d_view = torch.full((12 + TPS.GUARD,), float("nan"), device=cuda)
        pa = N.GsProjectPoseArgs(a, partials.data_ptr(), rows, d_view.data_ptr())
        N.check(lib.gs_project_backward_pose(C.byref(pa), stream), "gs_project_backward_pose")
    else:
        N.check(lib.gs_project_backward(C.byref(a), stream), "gs_project_backward")
    torch.cuda.synchronize()
    for k, t in o.items():
        assert TPS._guard_intact(t, n, float("nan")), f"{k}: written past row {n}"
    res = {k: t[:n].cpu().numpy() for k, t in o.items()}
    if pose:
        assert bool(torch.isnan(d_view[12:]).all())
        res["d_view"] = d_view[:12].cpu().numpy().astype(np.float64).reshape(3, 4)
    del keep
    return res


def _check_backward(got, pop, n, config, s, comp):
    ref = references(pop, n, config, s, comp)
    r64, r32 = ref["f64"]["bwd"], ref["f32"]["bwd"]
    ratio = ref["f64"]["fwd"]["ratio"].numpy()
    # a row within 1e-3 of the floor could take either branch: none in these inputs
    assert not (np.abs(ratio / SF.RHO_FLOOR - 1) < 1e-3).any()
    errs = []
    for k, v in got.items():
        if k == "d_view":
            continue
        p = TPS.GRAD_OF[k]
        errs += quantile_errors(k, v.reshape(n, -1), r32[p].numpy().reshape(n, -1), r64[p].numpy().reshape(n, -1))
    kind = TPS.CONFIGS[config][0]
    geo = r64["scaling" if kind == "raw" else "cov3d"].numpy().reshape(n, -1)
    assert not geo[0::16].any()  # all-zero cotangents: the early return
    if comp and n > 17:
        # rows 1::16 have cotangents on opacity and colour only: compensated, they have geometry
        # gradients (where the floor does not bind) that a missed early-out test would leave zero
        # (radius_clamp's first thousand rows are all on the floor: its small case has no such row)
        live = (ratio[1::16] > SF.RHO_FLOOR)
        assert live.any() or (pop == "radius_clamp" and n < 1000)
        assert (np.abs(geo[1::16][live]).max(1) > 0).all()
        key = "d_scaling" if kind == "raw" else "d_cov3d"
        assert (np.abs(got[key].reshape(n, -1)[1::16][live]).max(1) > 0).all(), "opacity-only rows lost their geometry gradient"
    return errs


@pytest.mark.parametrize("pop,n,config,s,comp", _stage_cases(["hot", "raw_cot", "cov_cot"]))
def test_project_backward_filtered(pkg, cuda, pop, n, config, s, comp):
    print(f"{pop}[{n}] {config} s={s} comp={comp}")
    got = gpu_backward(pkg, cuda, pop, n, config, s, comp)
    errs = _check_backward(got, pop, n, config, s, comp)
    assert not errs, errs


@pytest.mark.parametrize("pop,n,config,s,comp", _stage_cases(["hot", "raw_cot", "cov_cot"]))
def test_project_backward_pose_filtered(pkg, cuda, pop, n, config, s, comp):
    """The pose form (index order): every d_* by the quantile rule, and d_view
    within 1e-4 of its largest entry of the fp64 statement's view gradient."""
    print(f"{pop}[{n}] {config} s={s} comp={comp}")
    got = gpu_backward(pkg, cuda, pop, n, config, s, comp, pose=True)
    errs = _check_backward(got, pop, n, config, s, comp)
    d, deg, logit = case_inputs(pop, n, config)
    want = SF.backward_view(camera(pop), d, s, comp, *cotangents(pop, n, config), opacity_is_logit=logit).numpy()
    scale = np.abs(want).max()
    err = np.abs(got["d_view"] - want).max()
    print(f"  d_view: max err {err / scale:.3g} of its largest entry {scale:.3g}")
    assert scale > 0 and err <= 1e-4 * scale, (err, scale)
    assert not errs, errs


@pytest.mark.parametrize("pop,n,s,comp", [(p, n, s, c) for p in POPS for n in SIZES(p) for s, c in FILTERS])
def test_project_backward_adam_filtered(pkg, cuda, pop, n, s, comp):
    """gs_project_backward_adam against the plain filtered backward followed by gs_adam_step: bit for bit."""
    N = pkg._native
    lib = N.load()
    stream = torch.cuda.current_stream().cuda_stream
    a, o, keep = _bwd_args(pkg, cuda, pop, n, "hot", s, comp)
    dd = keep[0]["_inputs"]
    N.check(lib.gs_project_backward(C.byref(a), stream), "gs_project_backward")
    names = ("xyz", "color_logits", "opacity", "scaling", "rotation")
    grads = ("d_xyz", "d_color_logits", "d_opacity", "d_scaling", "d_rotation")
    gen = torch.Generator().manual_seed(n)
    m0 = {k: (torch.randn(dd[k].shape, generator=gen) * 0.01).to(cuda) for k in names}
    v0 = {k: (torch.rand(dd[k].shape, generator=gen) * 1e-4).to(cuda) for k in names}
    lrs = (1.6e-4, 2.5e-3, 0.05, 5e-3, 1e-3)
    step = 7
    bc1, bc2s = 1 - 0.9 ** step, (1 - 0.999 ** step) ** 0.5

    def adam_args(m, v, out, with_grads):
        ad = N.GsAdamArgs()
        ad.num_tensors, ad.beta1, ad.beta2, ad.eps = 5, 0.9, 0.999, 1e-15
        ad.one_minus_beta1, ad.one_minus_beta2 = 1 - 0.9, 1 - 0.999
        for i, (k, gk) in enumerate(zip(names, grads)):
            t = ad.t[i]
            t.param, t.exp_avg, t.exp_avg_sq = N.ptr(dd[k]), N.ptr(m[k]), N.ptr(v[k])
            t.grad = N.ptr(o[gk]) if with_grads else None
            t.numel, t.lr, t.bias_correction1, t.bias_correction2_sqrt = dd[k].numel(), lrs[i], bc1, bc2s
            t.param_out = N.ptr(out[k])
        return ad

    res = []
    for fused in (False, True):
        m = {k: t.clone() for k, t in m0.items()}
        v = {k: t.clone() for k, t in v0.items()}
        out = {k: torch.full_like(dd[k], float("nan")) for k in names}
        ad = adam_args(m, v, out, not fused)
        if fused:
            N.check(lib.gs_project_backward_adam(C.byref(a), C.byref(ad), stream), "gs_project_backward_adam")
        else:
            N.check(lib.gs_adam_step(C.byref(ad), stream), "gs_adam_step")
        torch.cuda.synchronize()
        res.append((m, v, out))
    for k in names:
        for x, y in zip(res[0], res[1]):
            assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), k
        assert not torch.equal(res[0][2][k], dd[k]) and bool(torch.isfinite(res[0][2][k]).all())
    del keep


# ---------------------------------------------------------- end to end ----
E2E_FWD = ["random_bg", "posed_camera", "tile8", "tile32", "model_random", "c1_forward"]
E2E_BWD = E2E_FWD[:-1]


def _settings(pkg, f, s, comp):
    return pkg.RenderSettings(image_height=int(f["height"]), image_width=int(f["width"]),
                              bg_color=torch.tensor(np.asarray(f["bg"], np.float32)), screen_filter=s,
                              filter_compensate=comp)


def _outputs(out):
    return dict(image=_np(out["image"]), alpha=_np(out["alpha"]), depth=_np(out["depth"]),
                means2d=_np(out["viewspace_points"]), conics=_np(out["conics"]), radii=_np(out["radii"]),
                vis=_np(out["visibility_filter"]).astype(bool))


def _render(pkg, dev, f, s, comp, **kw):
    model, leaves, _ = FU.gaussians_of(pkg, dev, f)
    out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(FU.camera_of(f), model, _settings(pkg, f, s, comp), **kw)
    return model, leaves, out


@pytest.mark.parametrize("s,comp", FILTERS)
@pytest.mark.parametrize("name", E2E_FWD)
def test_render_forward_vs_oracle(pkg, cuda, name, s, comp):
    f = G.load(name)
    eq, _ = SF.equivalent_scene(G.scene_of(f), s, comp)
    ref = G.oracle().render_forward(eq, margins=True)
    assert int(G.knife_edge(ref["margin"]).sum()) == 0  # (the precondition of comparing every pixel)
    with torch.no_grad():
        _, _, out = _render(pkg, cuda, f, s, comp)
        _, _, off = _render(pkg, cuda, f, 0.0, True)
    o = _outputs(out)
    errs = G.check_projection(o, ref) + G.check_image(o, ref, 1e-4)
    diff = float((out["image"] - off["image"]).abs().max())
    print(f"  {name} s={s} comp={comp}: filtered - unfiltered image up to {diff:.3g}")
    assert diff > 0.05, "the filter changed nothing"
    assert not errs, errs


@pytest.mark.parametrize("name", E2E_BWD)
def test_render_backward_vs_oracle(pkg, cuda, name):
    s, comp = 0.3, True
    f = G.load(name)
    n = f["xyz"].shape[0]
    scene = G.scene_of(f)
    eq, ratio = SF.equivalent_scene(scene, s, comp)
    assert ratio.min() >= 5e-4  # (far above the floor: the map is smooth at every row)
    H, W = int(f["height"]), int(f["width"])
    rng = np.random.default_rng(11)
    gi, ga, gd = (rng.uniform(-1, 1, sh).astype(np.float32) for sh in ((3, H, W), (1, H, W), (1, H, W)))
    ref = G.oracle().render_backward(eq, gi, ga, gd, margins=True)
    assert int(G.knife_edge(ref["margin"]).sum()) == 0
    model, leaves, out = _render(pkg, cuda, f, s, comp)
    L = sum((out[k] * FU.tensor(v, cuda)).sum() for k, v in (("image", gi), ("alpha", ga), ("depth", gd)))
    L.backward()
    o = _outputs(out)
    errs = G.check_projection(o, ref) + G.check_image(o, ref, 1e-4)
    g = ref["grads"]
    want = SF.pull_back(scene, s, comp, g["xyz"], g["cov3d"], g["opacity"])
    errs += G.check_grad("xyz", FU.leaf_grad("xyz", leaves["xyz"], n), want["xyz"])
    errs += G.check_grad("color_logits", FU.leaf_grad("color_logits", leaves["color_logits"], n), g["color_logits"])
    if "scaling" in f:  # the model path: through Sigma(scaling, rotation) and the opacity's sigmoid
        ds, dr = G.oracle().covariance_backward(f["scaling"], f["rotation"], want["cov3d"].astype(np.float32))
        op = 1.0 / (1.0 + np.exp(-np.asarray(f["opacity_raw"], np.float64)))
        errs += G.check_grad("scaling", FU.leaf_grad("scaling", leaves["scaling"], n), ds)
        errs += G.check_grad("rotation", FU.leaf_grad("rotation", leaves["rotation"], n), dr)
        errs += G.check_grad("opacity_raw", FU.leaf_grad("opacity_raw", leaves["opacity_raw"], n),
                             want["opacity"] * op * (1 - op))
    else:
        errs += G.check_grad("cov3d", FU.leaf_grad("cov3d", leaves["cov3d"], n), want["cov3d"])
        errs += G.check_grad("opacity", FU.leaf_grad("opacity", leaves["opacity"], n), want["opacity"])
    assert not errs, errs


def test_feature_render_with_filter(pkg, cuda):
    """C = 5 feature channels composited with the filtered colour pass's weights."""
    s, comp, c = 0.3, True, 5
    f = G.load("random_bg")
    n = f["xyz"].shape[0]
    f01, a, b = FU.random_features(n, c, 21)
    g_eq, _, _ = SF.equivalent_fixture(f, s, comp)
    exp, _, edge = FU.oracle_features(g_eq, f01, a, b)
    assert not edge.any()
    with torch.no_grad():
        _, _, out = _render(pkg, cuda, f, s, comp, features=FU.tensor(a * f01 + b, cuda))
        _, _, off = _render(pkg, cuda, f, 0.0, True, features=FU.tensor(a * f01 + b, cuda))
    err = np.abs(_np(out["features"]) - exp).max()
    scale = max(1.0, np.abs(exp).max())
    print(f"  features: max err {err:.3g} (scale {scale:.3g})")
    assert err <= 1e-4 * scale
    assert float((out["features"] - off["features"]).abs().max()) > 0.05


def test_density_statistics_with_filter(pkg, cuda):
    """gs_density_accumulate's formula on the filtered frame's blend gradient
    at means2d (the oracle's, on the equivalent scene: the map leaves means2d alone)."""
    s, comp = 0.3, True
    f = G.load("random_bg")
    n = f["xyz"].shape[0]
    H, W = int(f["height"]), int(f["width"])
    eq, _ = SF.equivalent_scene(G.scene_of(f), s, comp)
    r = G.oracle().render_backward(eq, f["g_image"], f["g_alpha"], f["g_depth"])
    vis = np.asarray(r["vis"], bool)
    gxy = r["grads"]["means2d"].astype(np.float64)
    want = np.where(vis, np.sqrt((0.5 * W * gxy[:, 0]) ** 2 + (0.5 * H * gxy[:, 1]) ** 2), 0.0)
    stats = pkg.DensityStats(n, cuda)
    _, _, out = _render(pkg, cuda, f, s, comp, density_stats=stats)
    L = sum((out[k] * FU.tensor(f["g_" + k], cuda)).sum() for k in ("image", "alpha", "depth"))
    L.backward()
    torch.cuda.synchronize()
    assert np.array_equal(_np(out["visibility_filter"]).astype(bool), vis)
    assert np.array_equal(_np(stats.denom), vis.astype(np.float32))
    assert np.array_equal(_np(stats.max_radii), np.where(vis, _np(out["radii"]), np.float32(0)))
    errs = G.check_grad("stats", _np(stats.grad_accum), want)
    assert want[vis].max() > 0 and not errs, errs


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("name", ["random_bg", "zero_bg_random"])
def test_multiscale(pkg, cuda, name, k):
    """At 1/k resolution the compensated filter's render is at most half as far
    (RMSE) from the box-averaged full-resolution oracle image as the unfiltered one."""
    f = G.load(name)
    ref = SF.box_average(G.oracle().render_forward(G.scene_of(f))["image"], k)
    low = dict(f)
    for key in ("width", "height", "cam_width", "cam_height"):
        assert int(f[key]) % k == 0
        low[key] = np.asarray(int(f[key]) // k)
    with torch.no_grad():
        on = _np(_render(pkg, cuda, low, 0.3, True)[2]["image"])
        off = _np(_render(pkg, cuda, low, 0.0, True)[2]["image"])
    e_on, e_off = SF.rmse(on, ref), SF.rmse(off, ref)
    print(f"  {name} /{k}: unfiltered {e_off:.4f}, filtered {e_on:.4f}, ratio {e_on / e_off:.2f}")
    assert e_on <= 0.5 * e_off


# -------------------------------------------------------------- trainer ----
def _trainer(pkg, cuda, root, **kw):
    from scene_util import load_scene, write_scene_files
    if not (root / "transforms_train.json").exists():
        write_scene_files(root, n_views=4, size=32)
    ds = load_scene(pkg, root, cuda, size=32, split=False)
    cfg = pkg.TrainingConfig(iterations=10, densify_from_iter=5, densify_until_iter=8, densify_interval=5,
                             num_random_points=600, log_interval=5, output_path=str(root / "out"),
                             position_lr_init=1.6e-3, position_lr_final=1.6e-5, **kw)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    return tr


def test_trainer_renders_with_its_filter(pkg, cuda, tmp_path):
    tr = _trainer(pkg, cuda, tmp_path, screen_filter=0.3)
    cam = tr._camera_for(1)
    st = pkg.RenderSettings(cam._height, cam._width, torch.zeros(3), screen_filter=0.3, filter_compensate=True)
    with torch.no_grad():
        want = pkg.GaussianRenderer().render(cam, tr.gaussians, st)["image"].clone()
        off = pkg.GaussianRenderer().render(cam, tr.gaussians, pkg.RenderSettings(cam._height, cam._width,
                                                                                 torch.zeros(3)))["image"].clone()
    seen = []
    render = tr.renderer.render

    def spy(camera, gaussians, settings, **kw):
        out = render(camera, gaussians, settings, **kw)
        seen.append((camera, settings, out["image"].detach().clone()))
        return out
    tr.renderer.render = spy
    tr.train(1)
    camera, settings, image = seen[0]
    assert camera is cam and (settings.screen_filter, settings.filter_compensate) == (0.3, True)
    assert torch.equal(image, want) and not torch.equal(image, off)
    # evaluation renders with it too
    seen.clear()
    tr.validate()
    assert seen and all(st_.screen_filter == 0.3 for _, st_, _ in seen)


def test_trainer_is_reproducible_with_filter(pkg, cuda, tmp_path):
    params = []
    for _ in range(2):
        tr = _trainer(pkg, cuda, tmp_path, screen_filter=0.3)
        tr.train(10)
        torch.cuda.synchronize()
        params.append([p.detach().clone() for p in tr.gaussians.parameter_list()])
    for a, b in zip(*params):
        assert a.shape == b.shape and torch.equal(a, b)


def test_graphed_step_refuses_a_filter(pkg, cuda):
    scene = pkg.synthetic.make_scene(500, 64, 64, seed=0)
    model = pkg.synthetic.to_model(scene, pkg.GaussianModel, cuda)
    cot = [torch.zeros(sh, device=cuda) for sh in ((3, 64, 64), (1, 64, 64), (1, 64, 64))]
    from stubs import Cam
    st = pkg.RenderSettings(64, 64, torch.zeros(3), screen_filter=0.3)
    with pytest.raises(ValueError, match="GraphedStep renders without a screen filter"):
        pkg.GraphedStep(pkg.GaussianRenderer(), Cam(64, 64, scene.fovx, scene.fovy), model, st, cot)
