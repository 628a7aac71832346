"""The 3D smoothing filter on the GPU (gs_filter3d_*; filter3d.py;
GaussianRenderer.render(filter_3d=...); TrainingConfig.filter_3d).

Stage level: the rate pass against the fp64 statement rounded once (1 ulp),
the map and its gradient against fp64 within four times the fp32
restatement's own error (tests/filter3d_util.py).  End to end: a closed form,
the pinned oracle on the equivalent scene (image 1e-4, gradients 1e-4 of scale
+ 1e-7 after the pull-back through the fp64 map), and the trainer."""
import ctypes as C
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import features_util as FU
import filter3d_util as F3
import golden_io as G
import screen_filter_util as SF
from scene_util import load_scene, write_scene_files
from stubs import Cam

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [1, 255, 256, 257, 1000]  # the block edges
_np = FU.np_
_bits = lambda t: t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------ rate pass ----
def _accumulate(pkg, dev, xyz, cams, max_rate, near=0.2, margin=0.15):
    N = pkg._native
    x, c = FU.tensor(xyz, dev), FU.tensor(cams, dev)
    a = N.GsFilter3dRateArgs(x.shape[0], x.data_ptr(), 3, c.data_ptr(), c.shape[0], near, margin, max_rate.data_ptr())
    N.check(N.load().gs_filter3d_accumulate(C.byref(a), N.stream_ptr(dev)), "gs_filter3d_accumulate")
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("n", SIZES)
def test_rate_pass(pkg, cuda, n, K):
    xyz, cams, rate = F3.rate_case(n, K, 7 * K + n)
    seen = rate > 0
    if n >= 255:  # (the populations the case is about)
        behind = (F3.rate_statement(xyz, cams, 1e-30, 1e30)[0] == 0)  # Z <= 0 at every camera
        assert behind.sum() > 0 and (~seen & ~behind).sum() > 0 and seen.sum() > 0
    rng = np.random.default_rng(n + K)
    # what was there before: small values a seen row replaces, huge ones that stay, and a NaN
    init = np.where(rng.uniform(size=n) < 0.1, 1e9, rng.uniform(0, 1e-3, n)).astype(np.float32)
    if n > 1:
        init[np.flatnonzero(~seen)[:1]] = np.nan
    got = FU.tensor(init, cuda)
    _accumulate(pkg, cuda, xyz, cams, got)
    g = _np(got)
    assert np.array_equal(g[~seen].view(np.int32), init[~seen].view(np.int32)), "a row no camera sees changed"
    fresh = seen & (init < 1.0)
    assert F3.within_one_ulp(g[fresh], rate[fresh]).all()
    assert np.array_equal(g[seen & ~fresh], init[seen & ~fresh])
    # a second call with other cameras keeps the maximum
    cams2 = F3.cameras(K, 900 + K)
    rate2, clear2 = F3.rate_statement(xyz, cams2, 0.2, 0.15)
    ok = clear2.min(1) > 1e-6  # (the same points: their decisions at the new cameras may be close calls)
    zero = torch.zeros(n, device=cuda)
    _accumulate(pkg, cuda, xyz, cams, zero)
    first = _np(zero).copy()
    _accumulate(pkg, cuda, xyz, cams2, zero)
    both = np.maximum(rate, rate2)
    g2 = _np(zero)
    assert F3.within_one_ulp(g2[ok], both[ok]).all() and (g2 >= first).all()
    kept = ok & (rate2 < rate * (1 - 1e-6))
    assert np.array_equal(g2[kept], first[kept])


def test_rate_pass_strided_rows_and_filter_update(pkg, cuda):
    """Filter3D.update from camera objects: the rows camera_params forms, the
    values' rule (sqrt(variance) / rate, the largest value where unseen)."""
    n = 1000
    rng = np.random.default_rng(4)
    cams = [Cam(64, 48, 0.9, 0.7, np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 3.0 + i], [0, 0, 0, 1]]))
            for i in range(3)]
    rows = np.asarray([pkg.filter3d.camera_row(c) for c in cams], np.float32)
    for c, row in zip(cams, rows):
        cp = pkg.camera_params(c, pkg.RenderSettings(48, 64, torch.zeros(3)))
        assert np.array_equal(row, np.asarray(list(cp.view) + [cp.fx, cp.fy, cp.cx, cp.cy, 64, 48], np.float32))
    pts = np.zeros((0, 3), np.float32)
    while len(pts) < n:
        p = rng.uniform([-6, -6, -9], [6, 6, 6], (4 * n, 3)).astype(np.float32)
        pts = np.concatenate([pts, p[F3.rate_statement(p, rows, 0.2, 0.15)[1].min(1) > 1e-6]])
    pts = pts[:n]
    rate, _ = F3.rate_statement(pts, rows, 0.2, 0.15)
    seen = rate > 0
    assert 50 < seen.sum() < n - 50
    flt = pkg.Filter3D(n, cuda, variance=0.3)
    wide = torch.zeros(n, 5, device=cuda)
    wide[:, :3] = FU.tensor(pts, cuda)
    flt.max_rate.fill_(7.0)  # (update starts from zero)
    flt.update(cams, wide[:, :3])
    torch.cuda.synchronize()
    assert F3.within_one_ulp(_np(flt.max_rate), rate).all()
    r32 = _np(flt.max_rate)
    want = np.float32(math.sqrt(0.3)) / r32[seen]
    v = _np(flt.values)
    assert np.abs(v[seen] - want).max() <= 2e-7 * want.max() and np.all(v[~seen] == v[seen].max())
    # none seen: zeros
    flt.update(cams, torch.full((n, 3), -50.0, device=cuda))
    assert float(flt.values.abs().max()) == 0.0 and float(flt.max_rate.abs().max()) == 0.0
    # no cameras, no Gaussians: nothing launched
    flt.update([], wide[:, :3].contiguous())
    assert float(flt.values.abs().max()) == 0.0
    pkg.Filter3D(0, cuda).update(cams, torch.zeros(0, 3, device=cuda))


# ------------------------------------------------------------------ map ----
@pytest.mark.parametrize("n", SIZES)
def test_map_forward_backward(pkg, cuda, n):
    inputs = F3.map_inputs(n, 40 + n)
    s, o, f, g_s, g_o = inputs
    ref = F3.reference64(inputs)
    host = F3.errors(F3.map32(s, o, f) + F3.map_backward32(*inputs), ref)
    st, ot = FU.tensor(s, cuda, grad=True), FU.tensor(o, cuda, grad=True)
    so, oo = pkg.apply_filter_3d(st, ot, FU.tensor(f, cuda))
    torch.autograd.backward([so, oo], [FU.tensor(g_s, cuda), FU.tensor(g_o, cuda)])
    torch.cuda.synchronize()
    got = (_np(so), _np(oo), _np(st.grad), _np(ot.grad))
    assert all(np.isfinite(a).all() for a in got)
    gpu = F3.errors(got, ref)
    for k in gpu:
        print(f"  n={n} {k}: GPU {gpu[k]:.3g}, fp32 restatement {host[k]:.3g}")
    off = f == 0
    assert np.array_equal(got[0][off].view(np.int32), s[off].view(np.int32))
    assert np.array_equal(got[2][off].view(np.int32), g_s[off].view(np.int32))
    for k in gpu:
        # (at n = 1 the single row may be exact in the restatement: the table's figure then)
        allow = F3.GPU_FACTOR * max(host[k], 0.0 if n >= 255 else {"s_out": 1.1e-7, "o_out": 1.6e-7, "d_s": 1.9e-7,
                                                                  "d_o": 7.2e-8}[k])
        assert gpu[k] <= allow, (k, gpu[k], allow)


def test_map_shapes_and_no_grad(pkg, cuda):
    """Opacity [N, 1] keeps its shape; under no_grad and with f alone requiring grad nothing is taped."""
    s, o, f, _, _ = F3.map_inputs(300, 2)
    st, ot = FU.tensor(s, cuda, grad=True), FU.tensor(o.reshape(-1, 1), cuda, grad=True)
    ft = FU.tensor(f, cuda, grad=True)
    so, oo = pkg.apply_filter_3d(st, ot, ft)
    assert so.shape == (300, 3) and oo.shape == (300, 1)
    (so.sum() + oo.sum()).backward()
    assert ft.grad is None and st.grad.shape == (300, 3) and ot.grad.shape == (300, 1)
    with torch.no_grad():
        s2, o2 = pkg.apply_filter_3d(st, ot, ft)
    assert not s2.requires_grad and torch.equal(_bits(s2), _bits(so)) and torch.equal(_bits(o2), _bits(oo))
    e_s, e_o = pkg.apply_filter_3d(torch.zeros(0, 3, device=cuda), torch.zeros(0, device=cuda), torch.zeros(0, device=cuda))
    assert e_s.shape == (0, 3) and e_o.shape == (0,)


# ----------------------------------------------------------- end to end ----
def _model(pkg, dev, d):
    n = d["xyz"].shape[0]
    m = pkg.GaussianModel()
    m._set(FU.tensor(d["xyz"], dev), FU.tensor(d["color_logits"], dev).reshape(n, 1, 3),
           torch.zeros(n, 15, 3, device=dev), FU.tensor(d["scaling"], dev), FU.tensor(d["rotation"], dev),
           FU.tensor(d["opacity_raw"], dev).reshape(n, 1))
    return m


def _camera(d, scale=1.0):
    """The scene's camera; scale: the focal length's factor at the same image size."""
    fov = lambda a: 2.0 * math.atan(math.tan(0.5 * a) / scale)
    return Cam(d["width"], d["height"], fov(d["fovx"]), fov(d["fovy"]), d["wv"])


def _settings(pkg, d, **kw):
    return pkg.RenderSettings(d["height"], d["width"], torch.tensor(d["bg"]), **kw)


def test_closed_form_single_gaussian(pkg, cuda):
    """One isotropic Gaussian on the optical axis at depth d, sigma = f / 4:
    cov2d = (F/d)^2 sigma^2 + variance + 1e-6 at the training camera -- the
    filter is `variance` px^2 there by construction -- and 16 x the variance
    at four times the focal length; the centre pixel's alpha is
    sigmoid(o) (sigma^2 / (sigma^2 + f^2))^(3/2) at both."""
    F, dep, var, logit = 80.0, 4.0, 0.2, 3.0
    f = math.sqrt(var) * dep / F
    sig = f / 4
    d = dict(xyz=np.array([[0, 0, dep]], np.float32), scaling=np.full((1, 3), math.log(sig), np.float32),
             rotation=np.array([[1, 0, 0, 0]], np.float32), opacity_raw=np.array([logit], np.float32),
             color_logits=np.zeros((1, 3), np.float32), wv=np.eye(4, dtype=np.float32), width=64, height=64,
             fovx=2 * math.atan(32 / F), fovy=2 * math.atan(32 / F), bg=np.zeros(3, np.float32))
    m = _model(pkg, cuda, d)
    flt = pkg.Filter3D(1, cuda, variance=var).update([_camera(d)], m._xyz.detach())
    torch.cuda.synchronize()
    assert abs(float(flt.max_rate[0]) - F / dep) <= 1e-5 and abs(float(flt.values[0]) - f) <= 1e-7
    alpha = 1 / (1 + math.exp(-logit)) * (sig * sig / (sig * sig + f * f)) ** 1.5
    r = pkg.GaussianRenderer()
    for k in (1.0, 4.0):
        with torch.no_grad():
            out = r.render(_camera(d, k), m, _settings(pkg, d), filter_3d=flt)
        want = 1.0 / ((k * F / dep) ** 2 * sig * sig + k * k * var + 1e-6)
        q = _np(out["conics"]).reshape(-1)
        print(f"  focal x{k:g}: conic {q[0]:.6f} (want {want:.6f}), alpha {float(out['alpha'][0, 32, 32]):.6f} "
              f"(want {alpha:.6f})")
        assert abs(q[0] - want) <= G.IMG_ATOL and abs(q[3] - want) <= G.IMG_ATOL and abs(q[1]) + abs(q[2]) <= G.IMG_ATOL
        assert abs(float(out["alpha"][0, 32, 32]) - alpha) <= G.IMG_ATOL
        assert np.abs(_np(out["viewspace_points"]) - 32.0).max() <= G.IMG_ATOL


@pytest.fixture(scope="module")
def scene():
    """1000 Gaussians at 64 x 64 with the oracle's render and gradients of the equivalent scene."""
    d = F3.model_scene(1000, 0)
    o = G.oracle()
    rng = np.random.default_rng(11)
    H, W = d["height"], d["width"]
    cot = [rng.uniform(-1, 1, sh).astype(np.float32) for sh in ((3, H, W), (1, H, W), (1, H, W))]
    ref = o.render_backward(F3.equivalent_scene(o, d), *cot, margins=True)
    assert int(G.knife_edge(ref["margin"]).sum()) == 0  # (the precondition of comparing every pixel)
    return d, cot, ref


def _outputs(out):
    return dict(image=_np(out["image"]), alpha=_np(out["alpha"]), depth=_np(out["depth"]),
                means2d=_np(out["viewspace_points"]), conics=_np(out["conics"]), radii=_np(out["radii"]),
                vis=_np(out["visibility_filter"]).astype(bool))


def _filter_of(pkg, dev, d):
    flt = pkg.Filter3D(d["xyz"].shape[0], dev)
    flt.values = FU.tensor(d["filter"], dev)
    return flt


def _loss(out, cot, dev):
    return sum((out[k] * FU.tensor(v, dev)).sum() for k, v in zip(("image", "alpha", "depth"), cot))


LEAVES = ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity")


def test_equivalent_scene(pkg, cuda, scene):
    d, cot, ref = scene
    n = d["xyz"].shape[0]
    m, flt = _model(pkg, cuda, d), _filter_of(pkg, cuda, d)
    r = pkg.GaussianRenderer()
    out = r.render(_camera(d), m, _settings(pkg, d), filter_3d=flt)
    _loss(out, cot, cuda).backward()
    with torch.no_grad():
        off = r.render(_camera(d), m, _settings(pkg, d))
    o = _outputs(out)
    errs = G.check_projection(o, ref) + G.check_image(o, ref, G.IMG_ATOL)
    assert float((out["image"].detach() - off["image"]).abs().max()) > 0.05, "the filter changed nothing"
    g = ref["grads"]
    want = F3.pull_back(d, g["cov3d"], g["opacity"])
    errs += G.check_grad("xyz", _np(m._xyz.grad), g["xyz"])
    errs += G.check_grad("color_logits", _np(m._features_dc.grad).reshape(n, 3), g["color_logits"])
    errs += G.check_grad("scaling", _np(m._scaling.grad), want["scaling"])
    errs += G.check_grad("rotation", _np(m._rotation.grad), want["rotation"])
    errs += G.check_grad("opacity_raw", _np(m._opacity.grad).reshape(n), want["opacity_raw"])
    assert not errs, errs
    # bit for bit the rasterizer on apply_filter_3d's outputs
    m2 = _model(pkg, cuda, d)
    s2, o2 = pkg.apply_filter_3d(m2._scaling, m2._opacity, flt.values)
    cam = pkg.camera_params(_camera(d), _settings(pkg, d), r.radius_min, r.radius_max, r.tile_size)
    direct = pkg.rasterize(cam, m2._xyz, None, s2, m2._rotation, m2._features_dc, o2, opacity_is_logit=False)
    _loss(dict(zip(("image", "alpha", "depth"), direct[:3])), cot, cuda).backward()
    for a, b in zip(direct[:5], (out[k] for k in ("image", "alpha", "depth", "viewspace_points", "conics"))):
        assert torch.equal(_bits(a), _bits(b))
    for name in LEAVES:
        assert torch.equal(_bits(getattr(m, name).grad), _bits(getattr(m2, name).grad)), name


def test_filter_none_is_todays_render(pkg, cuda, scene):
    d, cot, _ = scene
    res = []
    for kw in ({}, {"filter_3d": None}):
        m = _model(pkg, cuda, d)
        out = pkg.GaussianRenderer().render(_camera(d), m, _settings(pkg, d), **kw)
        _loss(out, cot, cuda).backward()
        res.append([out[k] for k in ("image", "alpha", "depth", "viewspace_points", "conics", "radii")]
                   + [getattr(m, name).grad for name in LEAVES])
    for a, b in zip(*res):
        assert torch.equal(_bits(a.float()), _bits(b.float()))
    # and a zero filter is the same image up to the sigmoid's place (kernel or map)
    with torch.no_grad():
        z = pkg.GaussianRenderer().render(_camera(d), _model(pkg, cuda, d), _settings(pkg, d),
                                          filter_3d=pkg.Filter3D(d["xyz"].shape[0], cuda))
    assert float((z["image"] - res[0][0]).abs().max()) <= 1e-5


def test_combined_with_features_statistics_and_screen_filter(pkg, cuda, scene):
    """filter_3d with features=, density_stats= and a compensated screen filter
    against the composition of the statements: the oracle on the screen
    filter's equivalent scene of the 3D filter's equivalent scene."""
    d, cot, _ = scene
    s, comp, c = 0.3, True, 5
    n, H, W = d["xyz"].shape[0], d["height"], d["width"]
    fx3 = F3.fixture_of(G.oracle(), d)
    g_eq, eq, _ = SF.equivalent_fixture(fx3, s, comp)
    f01, a, b = FU.random_features(n, c, 21)
    exp, _, edge = FU.oracle_features(g_eq, f01, a, b)
    assert not edge.any()
    ref = G.oracle().render_backward(eq, *cot, margins=True)
    assert int(G.knife_edge(ref["margin"]).sum()) == 0
    m, flt = _model(pkg, cuda, d), _filter_of(pkg, cuda, d)
    stats = pkg.DensityStats(n, cuda)
    out = pkg.GaussianRenderer().render(_camera(d), m, _settings(pkg, d, screen_filter=s, filter_compensate=comp),
                                        features=FU.tensor(a * f01 + b, cuda), density_stats=stats, filter_3d=flt)
    _loss(out, cot, cuda).backward()
    torch.cuda.synchronize()
    o = _outputs(out)
    errs = G.check_projection(o, ref) + G.check_image(o, ref, G.IMG_ATOL)
    err = np.abs(_np(out["features"]) - exp).max()
    scale = max(1.0, np.abs(exp).max())
    print(f"  features: max err {err:.3g} (scale {scale:.3g})")
    assert err <= 1e-4 * scale
    vis = np.asarray(ref["vis"], bool)
    gxy = ref["grads"]["means2d"].astype(np.float64)
    want = np.where(vis, np.sqrt((0.5 * W * gxy[:, 0]) ** 2 + (0.5 * H * gxy[:, 1]) ** 2), 0.0)
    assert np.array_equal(_np(stats.denom), vis.astype(np.float32))
    errs += G.check_grad("stats", _np(stats.grad_accum), want)
    errs += G.check_grad("xyz", _np(m._xyz.grad), SF.pull_back(G.scene_of(fx3), s, comp, ref["grads"]["xyz"],
                                                               ref["grads"]["cov3d"], ref["grads"]["opacity"])["xyz"])
    assert want[vis].max() > 0 and not errs, errs
    assert all(bool(torch.isfinite(getattr(m, name).grad).all()) for name in LEAVES)


# -------------------------------------------------------------- trainer ----
def _trainer(pkg, cuda, root, iterations=30, **kw):
    if not (root / "transforms_train.json").exists():
        write_scene_files(root, n_views=12, size=64)
    ds = load_scene(pkg, root, cuda, size=64, split=False)
    base = dict(iterations=iterations, densify_from_iter=10, densify_until_iter=10, densify_interval=10,
                densify_grad_threshold=2e-5, num_random_points=2000, log_interval=10, output_path=str(root / "out"),
                position_lr_init=1.6e-3, position_lr_final=1.6e-5, filter_3d_interval=7)
    base.update(kw)
    tr = pkg.GaussianTrainer(pkg.TrainingConfig(**base), ds)
    tr.setup()
    return tr


def _state(tr):
    torch.cuda.synchronize()
    st = [p.detach().clone() for p in tr.gaussians.parameter_list()]
    if tr.filter_3d is not None:
        st += [tr.filter_3d.values.clone(), tr.filter_3d.max_rate.clone()]
    return st


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_trainer_with_filter(pkg, cuda, tmp_path):
    tr = _trainer(pkg, cuda, tmp_path, filter_3d=True)
    n0 = tr.gaussians.get_num_points()
    assert tr.filter_3d.n == n0 and float(tr.filter_3d.values.min()) > 0
    seen = []
    render = tr.renderer.render

    def spy(camera, gaussians, settings, **kw):
        seen.append(kw.get("filter_3d"))
        assert kw["filter_3d"].n == gaussians.get_num_points()
        return render(camera, gaussians, settings, **kw)
    tr.renderer.render = spy
    tr.train(15)
    n1 = tr.gaussians.get_num_points()
    assert n1 != n0 and tr.filter_3d.n == n1 == tr.filter_3d.values.shape[0]  # rebuilt at the densification
    tr.save_checkpoint(15)
    tr.train(15)
    val = tr.validate()
    tr.compact(threshold=0.02)
    assert tr.filter_3d.n == tr.gaussians.get_num_points() <= n1
    assert len(seen) == 30 + 12 + 12 and all(s is not None for s in seen) and math.isfinite(val["psnr"])
    # the values are those of an update on the final rows
    want = pkg.Filter3D(tr.filter_3d.n, cuda, 0.2).update(tr.dataset.get_train_cameras(), tr.gaussians._xyz.detach())
    assert torch.equal(_bits(want.values), _bits(tr.filter_3d.values))
    # a second run: the same bits
    tr.renderer.render = render
    a = _trainer(pkg, cuda, tmp_path, filter_3d=True)
    a.train(30)
    b = _trainer(pkg, cuda, tmp_path, filter_3d=True)
    b.train(30)
    assert _same(_state(a), _state(b))
    # resumed from iteration 15 in a new trainer: the same bits as the uninterrupted run
    c = pkg.GaussianTrainer(a.config, a.dataset)
    c.load_checkpoint(15)
    assert c.filter_3d is not None and c.filter_3d.n == n1 and c.iteration == 15
    c.train(15)
    assert _same(_state(a), _state(c))
    off = _trainer(pkg, cuda, tmp_path)
    off.train(30)
    assert not _same(_state(a)[:6], _state(off)[:6]), "the filter changed nothing"


def test_trainer_without_filter_never_builds_one(pkg, cuda, tmp_path, monkeypatch):
    """filter_3d=False (the default): no Filter3D is constructed, no render gets
    the argument, the checkpoint has no such key, and the parameters are the
    bits of a run whose config never names the option."""
    plain = _trainer(pkg, cuda, tmp_path)
    plain.train(15)

    def never(*a, **k):
        raise AssertionError("a Filter3D was constructed")
    monkeypatch.setattr(pkg.trainer, "Filter3D", never)
    tr = _trainer(pkg, cuda, tmp_path, filter_3d=False, filter_3d_variance=0.5, filter_3d_interval=1)
    render = tr.renderer.render

    def spy(camera, gaussians, settings, **kw):
        assert "filter_3d" not in kw
        return render(camera, gaussians, settings, **kw)
    tr.renderer.render = spy
    tr.train(15)
    tr.validate()
    assert tr.filter_3d is None and _same(_state(tr), _state(plain))
    from safetensors import safe_open
    with safe_open(tr.save_checkpoint(15), framework="pt") as f:
        assert not [k for k in f.keys() if k.startswith("filter_3d")]


def test_mcmc_with_filter(pkg, cuda, tmp_path):
    from dp_mcmc_worker import mcmc_config
    write_scene_files(tmp_path)
    ds = load_scene(pkg, tmp_path, cuda, split=False)
    states = []
    for _ in range(2):
        cfg = mcmc_config(pkg, tmp_path / "out")
        cfg.filter_3d, cfg.filter_3d_interval = True, 3
        tr = pkg.GaussianTrainer(cfg, ds)
        tr.setup()
        tr.train(4)
        assert tr.gaussians.get_num_points() == 3100 == tr.filter_3d.n
        states.append(_state(tr))
    assert all(bool(torch.isfinite(t).all()) for t in states[0]) and _same(*states)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_dp_two_ranks_stay_bit_identical(pkg, cuda, tmp_path):
    write_scene_files(tmp_path)
    port = _free_port()
    outs = [tmp_path / f"rank{r}.npz" for r in range(2)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", GS_ALLREDUCE_CHUNKS="2", GS_ALLREDUCE_MIN_ROWS="256")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_filter3d_worker.py"), str(r), "2", str(port),
                               str(tmp_path), str(outs[r])], env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0], rcs
    a, b = (np.load(o) for o in outs)
    print(f"DP filter: n {int(a['n0'])} -> {int(a['n'])}")
    assert int(a["iteration"]) == 6 and int(a["n"]) == int(b["n"]) != int(a["n0"])
    assert a["values"].shape == (int(a["n"]),) and (a["values"] > 0).all()
    for k in [f"p{i}" for i in range(6)] + ["values", "max_rate"]:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"replicas diverged in {k}"
