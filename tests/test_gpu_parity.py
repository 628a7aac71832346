"""GPU parity: the HIP render path (through the C ABI) against the
reference's golden vectors and the pinned CPU oracle.

Tolerances are in tests/golden_io.py (1e-4 abs on image/alpha, gated depth,
grads 1e-4 x max|ref| + 1e-7 outside knife-edge-touched Gaussians)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import golden_io as G
from device_frame_util import index_statement
from stubs import Cam, Gauss, grad_or_zero

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().float().cpu().numpy()


def _outputs(out):
    return dict(image=_np(out["image"]), alpha=_np(out["alpha"]), depth=_np(out["depth"]),
                means2d=_np(out["viewspace_points"]), conics=_np(out["conics"]), radii=_np(out["radii"]),
                vis=_np(out["visibility_filter"]).astype(bool))


def _render_stub(pkg, dev, f, method=True):
    cam = Cam(f["cam_width"], f["cam_height"], f["fovx"], f["fovy"], f["wv"], method=method)
    st = pkg.RenderSettings(image_height=int(f["height"]), image_width=int(f["width"]),
                            bg_color=torch.tensor(np.asarray(f["bg"], np.float32)))
    g = Gauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], dev)
    return g, pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(cam, g, st)


def _loss(out, f, dev):
    t = lambda k: torch.tensor(np.asarray(f[k], np.float32), device=dev)
    L = (out["image"] * t("g_image")).sum() + (out["alpha"] * t("g_alpha")).sum() + (out["depth"] * t("g_depth")).sum()
    if "g_means2d" in f:
        L = L + (out["viewspace_points"] * t("g_means2d")).sum() + (out["conics"] * t("g_conics")).sum()
    return L


STUB_CASES = [n for n in G.fixture_names() if "scaling" not in G.load(n)]


@pytest.mark.parametrize("name", STUB_CASES)
def test_reference_fixture(pkg, cuda, name):
    f = G.load(name)
    g, out = _render_stub(pkg, cuda, f)
    o = _outputs(out)
    errs = G.check_image(o, f) + G.check_projection(o, f)
    assert out["image"].shape == (3, int(f["height"]), int(f["width"]))
    assert out["visibility_filter"].dtype == torch.bool
    if "g_image" in f:
        _loss(out, f, cuda).backward()
        n = f["xyz"].shape[0]
        errs += G.check_grad("xyz", grad_or_zero(g.xyz, (n, 3)), f["d_xyz"])
        errs += G.check_grad("cov3d", grad_or_zero(g.cov, (n, 3, 3)), f["d_cov3d"])
        errs += G.check_grad("color", grad_or_zero(g.feats, (n, 16, 3))[:, 0], f["d_color_logits"])
        errs += G.check_grad("opacity", grad_or_zero(g.op, (n, 1))[:, 0], f["d_opacity"])
        rest = grad_or_zero(g.feats, (n, 16, 3))[:, 1:]
        assert not rest.any(), "features_rest must get a zero gradient (reference only renders DC)"
    assert not errs, errs


def test_reference_model_path(pkg, cuda):
    """Raw-parameter (fused covariance) path vs reference GaussianModel grads."""
    f = G.load("model_random")
    m = pkg.GaussianModel()
    n = f["xyz"].shape[0]
    T = lambda a, shape=None: torch.tensor(np.asarray(a, np.float32)).reshape(shape or np.shape(a)).to(cuda)
    m._set(T(f["xyz"]), T(f["color_logits"], (n, 1, 3)), torch.zeros(n, 15, 3, device=cuda), T(f["scaling"]),
           T(f["rotation"]), T(f["opacity_raw"], (n, 1)))
    cam = Cam(f["cam_width"], f["cam_height"], f["fovx"], f["fovy"], f["wv"])
    st = pkg.RenderSettings(image_height=int(f["height"]), image_width=int(f["width"]),
                            bg_color=torch.tensor(np.asarray(f["bg"], np.float32)))
    out = pkg.GaussianRenderer().render(cam, m, st)
    o = _outputs(out)
    errs = G.check_image(o, f) + G.check_projection(o, f)
    _loss(out, f, cuda).backward()
    errs += G.check_grad("xyz", _np(m._xyz.grad), f["d_xyz"])
    errs += G.check_grad("scaling", _np(m._scaling.grad), f["d_scaling"])
    errs += G.check_grad("rotation", _np(m._rotation.grad), f["d_rotation"])
    errs += G.check_grad("features_dc", _np(m._features_dc.grad)[:, 0], f["d_color_logits"])
    errs += G.check_grad("opacity", _np(m._opacity.grad)[:, 0], f["d_opacity_raw"])
    assert not errs, errs


def test_tensor_world_view_transform(pkg, cuda):
    """world_view_transform as a tensor attribute (reference Camera style)."""
    f = G.load("posed_camera")
    _, out = _render_stub(pkg, cuda, f, method=False)
    assert not G.check_image(_outputs(out), f)


def test_kat_front_to_back(pkg, cuda):
    """test_renderer.py:127-161 restated: alpha 0.75, rgb 0.5 s(c0)+0.25 s(c1), depth 4/3."""
    cam = Cam(64, 64, np.radians(60), np.radians(60))
    st = pkg.RenderSettings(64, 64, torch.zeros(3))
    g = Gauss([[0, 0, 1], [0, 0, 2]], np.stack([np.diag([1e-4] * 3)] * 2), [[1, 0, 0], [0, 1, 0]], [0.5, 0.5], cuda)
    out = pkg.GaussianRenderer().render(cam, g, st)
    s = torch.sigmoid
    exp = 0.5 * s(torch.tensor([1.0, 0, 0])) + 0.25 * s(torch.tensor([0.0, 1, 0]))
    assert abs(out["alpha"][0, 32, 32].item() - 0.75) < 1e-3
    assert torch.allclose(out["image"][:, 32, 32].cpu(), exp, atol=1e-3)
    assert abs(out["depth"][0, 32, 32].item() - 4 / 3) < 2e-2


_EMPTY_FRAMES: dict = {}  # (case, frame_calls) -> (out, Gaussians) of _empty_frame


def _empty_frame(pkg, cuda, case, frame_calls):
    """A frame that draws nothing, rendered (once per test session) through
    the frame entry points or the stage path, and its means2D backward."""
    key = (case, frame_calls)
    if key not in _EMPTY_FRAMES:
        RZ = pkg.rasterizer
        if case == "culled":  # everything behind the camera
            cam = Cam(32, 32, np.radians(60), np.radians(60))
            st = pkg.RenderSettings(64, 64, torch.tensor([0.2, 0.3, 0.4]))
            g = Gauss([[0, 0, -1], [0, 0, -2]], np.stack([np.diag([1e-4] * 3)] * 2), [[1, 0, 0], [0, 1, 0]],
                      [0.5, 0.5], cuda)
        else:  # an empty model
            cam = Cam(32, 24, np.radians(60), np.radians(50))
            st = pkg.RenderSettings(24, 32, torch.tensor([0.2, 0.3, 0.4]))
            g = Gauss(np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0), cuda)
        saved = RZ._FRAME_CALLS
        try:
            RZ._FRAME_CALLS = frame_calls
            out = pkg.GaussianRenderer().render(cam, g, st)
            out["viewspace_points"].sum().backward()  # cotangent on means2D still flows
        finally:
            RZ._FRAME_CALLS = saved
        _EMPTY_FRAMES[key] = (out, g)
    return _EMPTY_FRAMES[key]


def _assert_same_empty_frame(pkg, cuda, case):
    """The frame entry points and the stage path draw the same empty frame."""
    (a, ga), (b, gb) = (_empty_frame(pkg, cuda, case, fc) for fc in (True, False))
    for k in ("image", "alpha", "depth", "viewspace_points", "conics", "radii", "visibility_filter"):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for name in ("xyz", "cov", "feats", "op"):
        x, y = getattr(ga, name).grad, getattr(gb, name).grad
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), name


@pytest.mark.parametrize("frame_calls", [True, False])
def test_all_culled_returns_bg(pkg, cuda, frame_calls):
    """test_renderer.py:113-125: everything behind the camera -> image == bg, alpha 0
    (through the frame entry points and the stage path, bit for bit alike)."""
    out, g = _empty_frame(pkg, cuda, "culled", frame_calls)
    assert torch.allclose(out["image"].cpu(), torch.tensor([0.2, 0.3, 0.4]).view(3, 1, 1).expand(3, 64, 64))
    assert torch.count_nonzero(out["alpha"]) == 0
    assert g.xyz.grad is not None and torch.isfinite(g.xyz.grad).all()
    _assert_same_empty_frame(pkg, cuda, "culled")


def _oracle_scene(sc, cov, bg, wv=None):
    o = G.oracle()
    return o.Scene(xyz=sc.xyz.numpy(), cov3d=cov, color_logits=sc.features_dc[:, 0].numpy(),
                   opacity=torch.sigmoid(sc.opacity[:, 0]).numpy(), wv=np.eye(4) if wv is None else wv,
                   width=sc.width, height=sc.height, fovx=sc.fovx, fovy=sc.fovy, bg=np.asarray(bg, np.float32))


@pytest.mark.parametrize("n,w,h,sig", [(3000, 200, 152, (0.01, 0.05)), (20000, 320, 240, (0.002, 0.02))])
def test_random_scene_vs_oracle(pkg, cuda, n, w, h, sig):
    """Larger random scenes (partial edge tiles, many overlaps) vs the oracle."""
    syn = pkg.synthetic
    sc = syn.make_scene(n, w, h, seed=n, sigma_range=sig)
    m = syn.to_model(sc, pkg.GaussianModel, cuda)
    cov = G.oracle().covariance(sc.scaling.numpy(), sc.rotation.numpy())
    bg = [0.1, 0.0, 0.3]
    cam = Cam(w, h, sc.fovx, sc.fovy)
    out = pkg.GaussianRenderer().render(cam, m, pkg.RenderSettings(h, w, torch.tensor(bg)))
    rng = np.random.default_rng(1)
    gi, ga, gd = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((3, h, w), (1, h, w), (1, h, w)))
    L = sum((out[k] * torch.tensor(v, device=cuda)).sum() for k, v in (("image", gi), ("alpha", ga), ("depth", gd)))
    L.backward()
    ref = G.oracle().render_backward(_oracle_scene(sc, cov, bg), gi, ga, gd)
    errs = G.check_image(_outputs(out), ref) + G.check_projection(_outputs(out), ref)
    ds, dr = G.oracle().covariance_backward(sc.scaling.numpy(), sc.rotation.numpy(), ref["grads"]["cov3d"])
    op = torch.sigmoid(sc.opacity[:, 0]).numpy()
    errs += G.check_grad("xyz", _np(m._xyz.grad), ref["grads"]["xyz"])
    errs += G.check_grad("scaling", _np(m._scaling.grad), ds)
    errs += G.check_grad("rotation", _np(m._rotation.grad), dr)
    errs += G.check_grad("features_dc", _np(m._features_dc.grad)[:, 0], ref["grads"]["color_logits"])
    errs += G.check_grad("opacity", _np(m._opacity.grad)[:, 0], ref["grads"]["opacity"] * op * (1 - op))
    assert not errs, errs


@pytest.mark.parametrize("seed", [11, 12])
def test_needle_gaussians_vs_oracle(pkg, cuda, seed):
    """Needle-shaped Gaussians (one axis 25-2000x the others): 2D conics with
    condition numbers on both sides of the blend's wave-culling limit
    (quad_mask), whose exp(-s/2) >= 1e-5 region reaches well past the 3-sigma
    rectangle they are binned by.  Both sides project the SAME fp32 cov3d
    (the reference's get_covariance path): building a covariance this
    ill-conditioned amplifies a 1-ulp exp() difference beyond any tolerance."""
    syn = pkg.synthetic
    n, w, h = 4000, 160, 128
    sc = syn.make_scene(n, w, h, seed=seed)
    g = torch.Generator().manual_seed(seed)
    sc.scaling[:, 0] = torch.empty(n).uniform_(math.log(0.05), math.log(0.2), generator=g)
    sc.scaling[:, 1:] = torch.empty(n, 2).uniform_(math.log(1e-4), math.log(2e-3), generator=g)
    cov = G.oracle().covariance(sc.scaling.numpy(), sc.rotation.numpy())
    op = torch.sigmoid(sc.opacity[:, 0]).numpy()
    bg = [0.2, 0.1, 0.0]
    gs = Gauss(sc.xyz.numpy(), cov, sc.features_dc[:, 0].numpy(), op, cuda)
    out = pkg.GaussianRenderer().render(Cam(w, h, sc.fovx, sc.fovy), gs, pkg.RenderSettings(h, w, torch.tensor(bg)))
    rng = np.random.default_rng(seed)
    gi, ga, gd = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((3, h, w), (1, h, w), (1, h, w)))
    L = sum((out[k] * torch.tensor(v, device=cuda)).sum() for k, v in (("image", gi), ("alpha", ga), ("depth", gd)))
    L.backward()
    ref = G.oracle().render_backward(_oracle_scene(sc, cov, bg), gi, ga, gd)
    errs = G.check_image(_outputs(out), ref) + G.check_projection(_outputs(out), ref)
    errs += G.check_grad("xyz", _np(gs.xyz.grad), ref["grads"]["xyz"])
    errs += G.check_grad("features_dc", _np(gs.feats.grad)[:, 0], ref["grads"]["color_logits"])
    errs += G.check_grad("opacity", _np(gs.op.grad)[:, 0], ref["grads"]["opacity"])
    # dL/dcov3d = J^T (-Q G Q) J R-rotated: an fp32 summation-order difference
    # in G = dL/dconic (tile pairs summed in another order) is amplified by
    # cond(Q)^2, so it is compared where the 2D conic is well conditioned
    q = ref["conics"].reshape(n, 4).astype(np.float64)
    hm, hd = 0.5 * (q[:, 0] + q[:, 3]), np.sqrt((0.5 * (q[:, 0] - q[:, 3])) ** 2 + q[:, 1] * q[:, 2])
    cond = (hm + hd) / np.maximum(hm - hd, 1e-30)
    well = cond < 1e3
    assert well.sum() > 100 and (~well & ref["vis"].astype(bool)).sum() > 50, "both conditioning regimes covered"
    errs += G.check_grad("cov3d", _np(gs.cov.grad).reshape(n, 9)[well], ref["grads"]["cov3d"].reshape(n, 9)[well])
    assert not errs, errs


def test_degenerate_inputs_vs_oracle(pkg, cuda):
    """Degenerate parameters through the model path, against the oracle:
    zero and far-from-unit quaternions (normalize's 1e-12 floor,
    gaussian_model.py:116-117), opacity logits of +-40 (sigmoid 1.0 and
    4e-18 in fp32), Gaussians 0.02-0.2 in front of the camera (radius clamp
    at 50 px, huge Jacobians), behind it (culled), and sub-micro scales
    (radius_min 0.01: one-pixel rectangles).  Image and projection as
    everywhere; gradients on every row (rotation per quaternion-norm group,
    each on its own scale)."""
    syn = pkg.synthetic
    n, w, h = 3000, 160, 128
    sc = syn.make_scene(n, w, h, seed=21)
    g = torch.Generator().manual_seed(21)
    sc.rotation[0:50] = 0.0
    sc.rotation[50:100] *= 1e6
    sc.rotation[100:150] *= 1e-6
    sc.opacity[150:200] = 40.0
    sc.opacity[200:250] = -40.0
    z = torch.empty(50).uniform_(0.02, 0.2, generator=g)
    sc.xyz[250:300, 2] = z
    sc.xyz[250:300, 0] = (torch.rand(50, generator=g) * 2 - 1) * z * math.tan(sc.fovx / 2)
    sc.xyz[250:300, 1] = (torch.rand(50, generator=g) * 2 - 1) * z * math.tan(sc.fovy / 2)
    sc.xyz[300:350, 2] = -sc.xyz[300:350, 2]
    sc.scaling[350:400] = math.log(1e-6)
    m = syn.to_model(sc, pkg.GaussianModel, cuda)
    cov = G.oracle().covariance(sc.scaling.numpy(), sc.rotation.numpy())
    bg = [0.3, 0.2, 0.1]
    out = pkg.GaussianRenderer().render(Cam(w, h, sc.fovx, sc.fovy), m, pkg.RenderSettings(h, w, torch.tensor(bg)))
    vis = out["visibility_filter"].cpu()
    assert not vis[300:350].any() and vis[250:300].any()
    assert float(out["radii"][250:300][vis[250:300]].max()) == 50.0
    rng = np.random.default_rng(21)
    gi, ga, gd = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((3, h, w), (1, h, w), (1, h, w)))
    L = sum((out[k] * torch.tensor(v, device=cuda)).sum() for k, v in (("image", gi), ("alpha", ga), ("depth", gd)))
    L.backward()
    ref = G.oracle().render_backward(_oracle_scene(sc, cov, bg), gi, ga, gd)
    errs = G.check_image(_outputs(out), ref) + G.check_projection(_outputs(out), ref)
    ds, dr = G.oracle().covariance_backward(sc.scaling.numpy(), sc.rotation.numpy(), ref["grads"]["cov3d"])
    op = torch.sigmoid(sc.opacity[:, 0]).numpy()
    errs += G.check_grad("xyz", _np(m._xyz.grad), ref["grads"]["xyz"])
    errs += G.check_grad("scaling", _np(m._scaling.grad), ds)
    # rotation by quaternion norm group, each on its own scale (the 1e-6-norm
    # rows' gradients are 1e6 x the others'; R is quadratic in the normalised
    # q, so the zero rows' gradient is zero on both sides)
    drot = _np(m._rotation.grad)
    assert np.isfinite(drot).all()
    rest = np.ones(n, bool)
    rest[0:150] = False
    for name, rows in (("rotation zero q", slice(0, 50)), ("rotation |q| 1e6", slice(50, 100)),
                       ("rotation |q| 1e-6", slice(100, 150)), ("rotation", rest)):
        errs += G.check_grad(name, drot[rows], dr[rows])
    errs += G.check_grad("features_dc", _np(m._features_dc.grad)[:, 0], ref["grads"]["color_logits"])
    errs += G.check_grad("opacity", _np(m._opacity.grad)[:, 0], ref["grads"]["opacity"] * op * (1 - op))
    assert not errs, errs


def test_radix_sort_matches_stable_argsort(pkg, cuda):
    import ctypes as C
    N = pkg._native
    lib = N.load()
    rng = np.random.default_rng(3)
    # (n, bits, top): top = a constant top byte (depth keys with z in [2, 4):
    # the last of four 8-bit passes sees one digit only), 24 = a depth window
    # (4.5M, 13): a C3-sized tile sort; (.., 8, 20): a bit range not starting
    # at 0; iota = 0: caller-given values.  The workspace is refilled with
    # garbage before every call (the look-back status must be cleared by the sort).
    for n, bits, top, lo, iota in ((1, 8, None, 0, 1), (1000, 13, None, 0, 1), (123457, 32, None, 0, 1),
                                   (70000, 4, None, 0, 1), (50000, 32, 0x40, 0, 1), (100000, 24, None, 0, 1),
                                   (4099, 20, None, 0, 1), (4_500_000, 13, None, 0, 0), (30000, 20, None, 8, 0),
                                   (2048, 16, None, 0, 0), (2049, 16, None, 0, 1)):
        k = rng.integers(0, 1 << min(bits, 31), n, dtype=np.int64).astype(np.uint32)
        if top is not None:
            k = (k & 0x00FFFFFF) | np.uint32(top << 24)
        if bits == 32:
            k[::7] = 0xFFFFFFFF
        keys = torch.tensor(k.view(np.int32), device=cuda)
        kk = torch.empty((2, n), dtype=torch.int32, device=cuda)
        vv = torch.empty((2, n), dtype=torch.int32, device=cuda)
        kk[0].copy_(keys)
        v0 = rng.permutation(n).astype(np.uint32)
        if not iota:
            vv[0].copy_(torch.tensor(v0.view(np.int32)))
        ws = torch.full((lib.gs_radix_sort_workspace_bytes(n),), 0xAB, dtype=torch.uint8, device=cuda)
        alt = C.c_int32(0)
        N.check(lib.gs_radix_sort_pairs(N.ptr(kk[0]), N.ptr(vv[0]), N.ptr(kk[1]), N.ptr(vv[1]), n, lo, bits, iota,
                                        N.ptr(ws), ws.numel(), C.byref(alt), torch.cuda.current_stream().cuda_stream),
                "sort")
        digit = (k >> np.uint32(lo)) & np.uint32((1 << (bits - lo)) - 1) if bits - lo < 32 else k
        order = np.argsort(digit, kind="stable")
        want_v = order.astype(np.uint32) if iota else v0[order]
        assert np.array_equal(vv[alt.value].cpu().numpy().view(np.uint32), want_v), (n, bits, lo, iota)
        assert np.array_equal(kk[alt.value].cpu().numpy().view(np.uint32), k[order]), (n, bits, lo, iota)


def test_depth_sort_msd_matches_stable_argsort(pkg, cuda):
    """gs_depth_sort_msd (one MSD pass + a sort per bucket in LDS) gives the
    LSD sort's result -- np.argsort(kind="stable") of the keys, values = input
    positions -- for windowed keys below 255 << (bits - 8) plus culled
    sentinels (2^bits - 1); a bucket over 16384 keys sets the overflow word."""
    import ctypes as C
    N = pkg._native
    lib = N.load()
    rng = np.random.default_rng(11)
    # (n, bits, culled fraction, clumped): clumped = every visible key in two buckets
    for n, bits, culled, clump in ((1, 9, 0.0, False), (5, 12, 0.4, False), (1000, 9, 0.1, False),
                                   (100_000, 16, 0.0, False), (1_000_000, 24, 0.0, False),
                                   (300_000, 20, 0.5, False), (40_000, 24, 0.0, True), (2049, 17, 1.0, False),
                                   (600_000, 25, 0.1, False), (200_000, 28, 0.2, False), (100_000, 32, 0.0, False)):
        lim = 255 << (bits - 8)
        if clump:
            k = (rng.integers(0, 2, n) << (bits - 8)) + rng.integers(0, 50, n)  # ~20k keys per bucket
        else:
            k = rng.integers(0, lim, n)
        k = k.astype(np.uint32)
        k[rng.random(n) < culled] = (1 << bits) - 1
        kk = torch.empty((2, n), dtype=torch.int32, device=cuda)
        vv = torch.full((2, n), -7, dtype=torch.int32, device=cuda)
        kk[0].copy_(torch.tensor(k.view(np.int32)))
        ws = torch.full((lib.gs_radix_sort_workspace_bytes(n),), 0xAB, dtype=torch.uint8, device=cuda)
        flag = torch.zeros((2,), dtype=torch.int32, device=cuda)
        alt = C.c_int32(0)
        N.check(lib.gs_depth_sort_msd(N.ptr(kk[0]), N.ptr(vv[0]), N.ptr(kk[1]), N.ptr(vv[1]), n, bits, N.ptr(ws),
                                      ws.numel(), N.ptr(flag) + 4, C.byref(alt), torch.cuda.current_stream().cuda_stream),
                "msd sort")
        torch.cuda.synchronize()
        assert alt.value == 1
        if clump:
            assert int(flag[1]) == -1, "a bucket over capacity must set the overflow word"
            continue
        assert int(flag[1]) == 0, (n, bits)
        order = np.argsort(k, kind="stable")
        assert np.array_equal(vv[1].cpu().numpy().view(np.uint32), order.astype(np.uint32)), (n, bits)
        assert np.array_equal(kk[1].cpu().numpy().view(np.uint32), k[order]), (n, bits)
    with pytest.raises(RuntimeError):
        N.check(lib.gs_depth_sort_msd(N.ptr(kk[0]), N.ptr(vv[0]), N.ptr(kk[1]), N.ptr(vv[1]), 10, 33, N.ptr(ws),
                                      ws.numel(), N.ptr(flag), C.byref(alt), None), "msd sort")


def test_depth_sort_msd_overflow_falls_back(pkg, cuda):
    """A scene whose visible depths clump into one MSD bucket (> 16384
    Gaussians at nearly the same depth) renders exactly as with the LSD depth
    sort: the overflow poisons the frame's depth max, the frame is sorted
    again, and the LSD path is kept for the next frames."""
    from mini3dgs_amd import rasterizer as RZ
    rng = np.random.default_rng(5)
    n, W, H = 60_000, 320, 240
    scene = pkg.synthetic.make_scene(n, W, H, seed=3)
    model = pkg.synthetic.to_model(scene, pkg.GaussianModel, cuda)
    with torch.no_grad():
        z = torch.tensor(rng.uniform(2, 6, n), dtype=torch.float32, device=cuda)
        z[: n // 2] = 3.0 + torch.arange(n // 2, device=cuda, dtype=torch.float32) * 1e-7  # a depth clump
        model._xyz[:, :2] *= (z / model._xyz[:, 2])[:, None]
        model._xyz[:, 2] = z
    cam = Cam(W, H, scene.fovx, scene.fovy)
    st = pkg.RenderSettings(image_height=H, image_width=W, bg_color=torch.zeros(3))
    r = pkg.GaussianRenderer()
    RZ._MSD_BACKOFF.clear()
    # (earlier tests' scenes may have switched the depth-key windows off: start clean)
    RZ._WINDOW_STATE.pop(model._xyz.device, None)
    RZ._DEPTH_HIST.pop(model._xyz.device, None)
    try:
        with torch.no_grad():
            outs = [r.render(cam, model, st)["image"].clone() for _ in range(3)]  # windowed keys + overflow
            assert RZ._MSD_BACKOFF.get(model._xyz.device, 0) > 0, "the clump must overflow an MSD bucket"
            RZ._DEPTH_MSD = False
            ref = r.render(cam, model, st)["image"]
    finally:
        RZ._DEPTH_MSD = True
        RZ._MSD_BACKOFF.clear()
    for o in outs:
        assert torch.equal(o, ref)


def test_forward_capacity_paths(pkg, cuda):
    """The forward queues the emission before the T read-back into buffers
    sized from the last frame's T (+ 25 %); a frame whose T outgrows that
    guess is emitted again after the read-back.  Both paths give the same
    frame bit for bit."""
    W, H = 320, 240
    small = pkg.synthetic.make_scene(2000, W, H, seed=61)
    big = pkg.synthetic.make_scene(20000, W, H, seed=62)
    r = pkg.GaussianRenderer()
    cam = Cam(W, H, small.fovx, small.fovy)
    st = pkg.RenderSettings(H, W, torch.tensor([0.1, 0.2, 0.3]))
    mb = pkg.synthetic.to_model(big, pkg.GaussianModel, cuda)
    with torch.no_grad():
        r.render(cam, pkg.synthetic.to_model(small, pkg.GaussianModel, cuda), st)
        a = r.render(cam, mb, st)  # T far above the small frame's: the redo path
        b = r.render(cam, mb, st)  # the same T again: emitted before the read-back
    for key in ("image", "alpha", "depth"):
        assert torch.equal(a[key], b[key]), key


def test_tile_ranges_every_tile(pkg, cuda):
    """gs_tile_ranges writes every tile, empty ones as [p, p) (no memset), and
    all-empty lists."""
    import ctypes as C
    N = pkg._native
    lib = N.load()
    stream = torch.cuda.current_stream().cuda_stream
    for keys, ntiles in (([2, 2, 5, 5, 5, 9], 12), ([0, 0, 1], 2), ([], 7), ([3], 4)):
        k = torch.tensor(keys if keys else [0], dtype=torch.int32, device=cuda)
        ranges = torch.full((ntiles, 2), -7, dtype=torch.int32, device=cuda)
        ra = N.GsRangeArgs(len(keys), ntiles, N.ptr(k), N.ptr(ranges))
        N.check(lib.gs_tile_ranges(C.byref(ra), stream), "gs_tile_ranges")
        want = []
        for t in range(ntiles):
            lo = sum(1 for v in keys if v < t)
            hi = sum(1 for v in keys if v <= t)
            want.append((lo, hi))
        assert ranges.cpu().tolist() == [list(w) for w in want], (keys, ranges.cpu().tolist())


def test_blend_ranges_clamped_to_entries(pkg, cuda):
    """Round-3 review (weak 7): the blend kernels read sorted_gauss[start + lane]
    from the tile ranges; ranges are clamped to the T entries
    (gs_blend_*_args.num_pairs), so a ranges table past T reads no memory
    outside the list.  Re-blends a frame with the true ranges (the same image)
    and with every range pushed past T ([T - 5, T + 1000): clamped to the
    last 5 entries; finite output, no fault)."""
    RZ, N = pkg.rasterizer, pkg._native
    lib = N.load()
    syn = pkg.synthetic
    W, H = 96, 80
    sc = syn.make_scene(3000, W, H, seed=5, sigma_range=(0.01, 0.05))
    m = syn.to_model(sc, pkg.GaussianModel, cuda)
    cam = pkg.camera_params(Cam(W, H, sc.fovx, sc.fovy), pkg.RenderSettings(H, W, torch.zeros(3)))
    image, alpha, depth, _, _, _, _, fr = RZ.forward_pipeline(
        cam, m._xyz, None, m._scaling, m._rotation, m._features_dc[:, 0, :], torch.sigmoid(m._opacity).squeeze(1))
    T = fr.T
    assert T > 5
    stream = torch.cuda.current_stream().cuda_stream
    bad = torch.empty_like(fr.ranges)
    bad[:, 0], bad[:, 1] = T - 5, T + 1000
    for ranges, want in ((fr.ranges, image), (bad, None)):
        img = torch.full_like(image, -1.0)
        al, dp = torch.empty_like(alpha), torch.empty_like(depth)
        flags, cneval = torch.empty_like(fr.pix_flags), torch.empty_like(fr.cell_neval)
        live = torch.empty_like(fr.live_bits)
        fa = N.GsBlendFwdArgs(cam.to_struct(), cam.tiles_x, cam.tiles_y, N.ptr(ranges), N.ptr(fr.sorted_gauss),
                              N.ptr(fr.records), N.ptr(img), N.ptr(al), N.ptr(dp), N.ptr(flags), N.ptr(cneval),
                              N.ptr(live), live.shape[1], None, T, None)
        N.check(lib.gs_blend_forward(C.byref(fa), stream), "gs_blend_forward")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(img).all()) and float(img.min()) >= 0.0
        if want is not None:
            assert torch.equal(img, want)
    fa.num_pairs = -1
    assert lib.gs_blend_forward(C.byref(fa), stream) == 1


@pytest.mark.parametrize("tile", [16, 300, 480])
def test_deterministic(pkg, cuda, tile):
    """No float atomics anywhere, at any tile size: two runs are
    bit-identical, grads included.  Tiles of 300 / 480 px (1,444 / 3,600
    cells) also run with a partial budget that forces cell batches (summed
    batch by batch by gs_gather_partials) and with no liveness bitmap."""
    RZ = pkg.rasterizer
    syn = pkg.synthetic
    sc = syn.make_scene(50000 if tile == 16 else 8000, 480, 270, seed=5, sigma_range=(0.002, 0.02))
    budgets = [(RZ.PARTIAL_BUDGET_BYTES, RZ.LIVE_BUDGET_BYTES)]
    if tile > 16:
        budgets += [(41 * 9000 * 100, RZ.LIVE_BUDGET_BYTES), (41 * 9000 * 300, 1)]
    saved = budgets[0]
    outs = []
    try:
        for pb, lb in budgets:
            RZ.PARTIAL_BUDGET_BYTES, RZ.LIVE_BUDGET_BYTES = pb, lb
            res = []
            for _ in range(2):
                m = syn.to_model(sc, pkg.GaussianModel, cuda)
                out = pkg.GaussianRenderer(tile_size=tile).render(Cam(480, 270, sc.fovx, sc.fovy), m,
                                                                  pkg.RenderSettings(270, 480, torch.zeros(3)))
                (out["image"].sum() + out["depth"].mean()).backward()
                res.append((out["image"].clone(), m._xyz.grad.clone(), m._rotation.grad.clone(),
                            m._opacity.grad.clone()))
            for a, b in zip(*res):
                assert torch.equal(a, b)
            outs.append(res[0])
    finally:
        RZ.PARTIAL_BUDGET_BYTES, RZ.LIVE_BUDGET_BYTES = saved
    # batched / bitmap-free runs: the same image; gradients summed in another
    # order (per batch), so equal to rounding
    for r in outs[1:]:
        assert torch.equal(r[0], outs[0][0])
        for a, b in zip(r[1:], outs[0][1:]):
            scale = float(b.abs().max()) + 1e-12
            assert float((a - b).abs().max()) <= 1e-5 * scale


def test_emit_capacity_guess(pkg, cuda):
    """The tile emission is queued before T is read back, into buffers sized
    from the previous frame's T: a guess too small (emit skipped, re-emitted
    after the sync), none (first frame) and a good one give bit-identical
    frames and gradients."""
    RZ = pkg.rasterizer
    syn = pkg.synthetic
    sc = syn.make_scene(50000, 480, 270, seed=6, sigma_range=(0.002, 0.02))
    res = []
    for guess in (None, 16, "last"):
        if guess is None:
            RZ._T_SEEN.pop(cuda, None)
        elif guess != "last":
            RZ._T_SEEN[cuda] = guess
        m = syn.to_model(sc, pkg.GaussianModel, cuda)
        out = pkg.GaussianRenderer().render(Cam(480, 270, sc.fovx, sc.fovy), m,
                                            pkg.RenderSettings(270, 480, torch.zeros(3)))
        (out["image"].sum() + out["depth"].sum()).backward()
        res.append((out["image"].clone(), out["depth"].clone(), m._xyz.grad.clone(), m._opacity.grad.clone()))
        assert RZ._T_SEEN[cuda] > 16
    for r in res[1:]:
        for a, b in zip(res[0], r):
            assert torch.equal(a, b)


@pytest.mark.parametrize("guess,scene", [("last", "40k"), (16, "40k"), ("last", "5k"), (16, "5k"), ("last", "5k_wide"),
                                         ("last", "16384"), ("last", "16385")])
def test_frame_entry_points_match(pkg, cuda, guess, scene):
    """The default tile renders through the frame entry points
    (gs_render_forward / gs_render_backward, one library call per direction);
    the stage-by-stage path (GS_FRAME_CALLS=0, every other tile size) launches
    the same kernels: outputs, gradients and the frame's index work are
    bit-identical -- with a capacity guess that holds, and one far too small
    (GS_NEED_CAPACITY, then the call resumed with a larger tile workspace).
    Small frames (5k: n and T within one workgroup's sort; 5k_wide: n within
    it, T not) sort in one launch there (gs_internal_small_sort), with the
    radix passes' result."""
    RZ = pkg.rasterizer
    syn = pkg.synthetic
    n, sig = {"40k": (40000, (0.002, 0.02)), "5k": (5000, (0.002, 0.01)), "5k_wide": (5000, (0.02, 0.06)),
              # the one-workgroup depth sort's edge (gs_internal_small_sort: n <= 16384)
              "16384": (16384, (0.002, 0.01)), "16385": (16385, (0.002, 0.01))}[scene]
    sc = syn.make_scene(n, 480, 270, seed=8, sigma_range=sig)
    res = []
    saved = RZ._FRAME_CALLS
    try:
        for fast in (False, True):
            RZ._FRAME_CALLS = fast
            m = syn.to_model(sc, pkg.GaussianModel, cuda)
            if guess != "last":
                RZ._T_SEEN[cuda] = guess
            out = pkg.GaussianRenderer().render(Cam(480, 270, sc.fovx, sc.fovy), m,
                                                pkg.RenderSettings(270, 480, torch.tensor([0.1, 0.2, 0.3])))
            if fast and scene in ("5k", "5k_wide"):
                T = RZ._T_SEEN[cuda]
                assert (T <= 16384) == (scene == "5k"), T
            (out["image"].sum() + out["alpha"].mean() + out["depth"].mean() + out["viewspace_points"].sum()).backward()
            res.append([out[k].clone() for k in ("image", "alpha", "depth", "viewspace_points", "radii", "conics",
                                                 "visibility_filter")] +
                       [m._xyz.grad.clone(), m._scaling.grad.clone(), m._rotation.grad.clone(),
                        m._features_dc.grad.clone(), m._opacity.grad.clone()])
    finally:
        RZ._FRAME_CALLS = saved
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_frame_entry_points_data_parallel_ranges(pkg, cuda):
    """The frame backward with the data-parallel reduction's row ranges
    (projection backward per range, gs_render_backward project = 0) equals
    the one-range backward bit for bit."""
    RZ = pkg.rasterizer
    syn = pkg.synthetic
    sc = syn.make_scene(20000, 320, 240, seed=9, sigma_range=(0.002, 0.02))
    got = []
    for chunks in (1, 3):
        m = syn.to_model(sc, pkg.GaussianModel, cuda)
        cam = pkg.camera_params(Cam(320, 240, sc.fovx, sc.fovy), pkg.RenderSettings(240, 320, torch.zeros(3)))
        raw = (m._xyz, None, m._scaling, m._rotation, m._features_dc[:, 0, :], m._opacity)
        with torch.no_grad():
            img, al, dp, m2, cn, rd, vi, fr = RZ.forward_pipeline(cam, *[None if t is None else t.detach() for t in raw],
                                                                  opacity_is_logit=True, need_grad=True)
        assert fr.calls is True
        seen = []
        out = {"_rows_ready": lambda lo, hi: seen.append((lo, hi)), "_chunks": chunks}
        g = torch.ones_like(img)
        d = RZ.backward_pipeline(cam, fr, *[None if t is None else t.detach() for t in raw], m2, cn, g, None, None,
                                 None, None, opacity_is_logit=True, out=out, outputs=(img, al, dp))
        assert seen == [(20000 * k // chunks, 20000 * (k + 1) // chunks) for k in range(chunks)]
        got.append([t.clone() for t in d if t is not None])
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_fused_adam_matches_torch_adam(pkg, cuda):
    """FusedAdam (one gs_adam_step launch) vs torch.optim.Adam, 5 groups as in
    the reference's GaussianOptimizer (optimizer.py:100-113), one param without grad."""
    g = torch.Generator().manual_seed(0)
    shapes = [(1000, 3), (1000, 1, 3), (1000, 1), (1000, 3), (1000, 4), (1000, 15, 3)]
    lrs = [1.6e-4, 2.5e-3, 0.05, 5e-3, 1e-3, 2.5e-3]
    a = [torch.randn(s, generator=g).to(cuda).requires_grad_() for s in shapes]
    b = [t.detach().clone().requires_grad_() for t in a]
    oa = pkg.optim.FusedAdam([{"params": [t], "lr": lr} for t, lr in zip(a, lrs)])
    ob = torch.optim.Adam([{"params": [t], "lr": lr} for t, lr in zip(b, lrs)])
    for it in range(5):
        for i, (x, y) in enumerate(zip(a, b)):
            if i == 5:
                x.grad = y.grad = None
                continue
            gr = torch.randn(shapes[i], generator=g).to(cuda)
            x.grad, y.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
    for x, y in zip(a, b):
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-5), (x - y).abs().max()  # fp32 rounding of two Adam kernels


def test_fused_adam_param_out(pkg, cuda):
    """gs_adam_tensor.param_out: the parameter is only read and the update
    goes to the output tensor, bit-identical to the in-place step's value;
    the moments advance as in place.  Three steps from the same parameters
    against in-place FusedAdam steps whose parameters are put back each time."""
    g = torch.Generator().manual_seed(5)
    shapes = [(999, 3), (1000, 4), (17,)]
    a = [torch.randn(s, generator=g).to(cuda).requires_grad_() for s in shapes]
    b = [t.detach().clone().requires_grad_() for t in a]
    p0 = [t.detach().clone() for t in a]
    oa = pkg.optim.FusedAdam([{"params": [t], "lr": 1e-2 * (i + 1)} for i, t in enumerate(a)])
    ob = pkg.optim.FusedAdam([{"params": [t], "lr": 1e-2 * (i + 1)} for i, t in enumerate(b)])
    outs = [torch.full_like(t, float("nan")) for t in a]
    for t, o in zip(a, outs):
        oa.set_output(t, o)
    for it in range(3):
        for x, y, s in zip(a, b, shapes):
            gr = torch.randn(s, generator=g).to(cuda)
            x.grad, y.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
        for x, y, o, q in zip(a, b, outs, p0):
            assert torch.equal(x.detach(), q)        # the parameter is untouched
            assert torch.equal(o, y.detach())        # the update, bit for bit
            with torch.no_grad():
                y.copy_(q)                           # in-place reference back to the same start
    for x, y in zip(a, b):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[x][k], ob.state[y][k])
    with pytest.raises(ValueError):
        oa.set_output(a[0], a[0])


@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (0.3, 0.2, 0.1)])
def test_long_tile_lists_vs_oracle(pkg, cuda, bg):
    """Tiles with > 256 entries (several forward batches, many backward
    batches) and low opacities, so pixels run deep into their lists."""
    syn = pkg.synthetic
    n, w, h = 20000, 48, 40
    sc = syn.make_scene(n, w, h, seed=7, sigma_range=(0.05, 0.15), z_range=(3.0, 4.0))
    sc.opacity.fill_(-2.5)  # sigmoid ~ 0.08: ~90% of pixels terminate, thousands of entries deep
    m = syn.to_model(sc, pkg.GaussianModel, cuda)
    out = pkg.GaussianRenderer().render(Cam(w, h, sc.fovx, sc.fovy), m, pkg.RenderSettings(h, w, torch.tensor(bg)))
    rng = np.random.default_rng(2)
    gi, ga, gd = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((3, h, w), (1, h, w), (1, h, w)))
    L = sum((out[k] * torch.tensor(v, device=cuda)).sum() for k, v in (("image", gi), ("alpha", ga), ("depth", gd)))
    L.backward()
    cov = G.oracle().covariance(sc.scaling.numpy(), sc.rotation.numpy())
    ref = G.oracle().render_backward(_oracle_scene(sc, cov, bg), gi, ga, gd)
    assert ref["T"] / ((w + 15) // 16 * ((h + 15) // 16)) > 512, "scene must give long tile lists"
    errs = G.check_image(_outputs(out), ref) + G.check_projection(_outputs(out), ref)
    ds, dr = G.oracle().covariance_backward(sc.scaling.numpy(), sc.rotation.numpy(), ref["grads"]["cov3d"])
    errs += G.check_grad("xyz", _np(m._xyz.grad), ref["grads"]["xyz"])
    errs += G.check_grad("scaling", _np(m._scaling.grad), ds)
    errs += G.check_grad("rotation", _np(m._rotation.grad), dr)
    errs += G.check_grad("features_dc", _np(m._features_dc.grad)[:, 0], ref["grads"]["color_logits"])
    assert not errs, errs


def _scene_vs_oracle(pkg, cuda, sc, W, H, bg, seed=1, renderer_kw=None, knife=True, label="", wv=None):
    """Render sc (this package's model, raw-parameter path) fwd + bwd of a
    seeded cotangent and compare with the oracle on the same inputs.  With
    knife=True, pixels out of tolerance are accepted only where the oracle's
    replay came within rounding of a decision (golden_io.knife_edge), and
    every such pixel is printed with its margins."""
    import os
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
    kw = renderer_kw or {}
    out = pkg.GaussianRenderer(**kw).render(Cam(W, H, sc.fovx, sc.fovy, wv=wv), m,
                                            pkg.RenderSettings(H, W, torch.tensor(bg)))
    rng = np.random.default_rng(seed)
    gi, ga, gd = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((3, H, W), (1, H, W), (1, H, W)))
    L = sum((out[k] * torch.tensor(v, device=cuda)).sum() for k, v in (("image", gi), ("alpha", ga), ("depth", gd)))
    L.backward()
    cov = G.oracle().covariance(sc.scaling.numpy(), sc.rotation.numpy())
    osc = _oracle_scene(sc, cov, bg, wv=wv)
    osc.tile = kw.get("tile_size", 16)
    osc.radius_min, osc.radius_max = kw.get("radius_min", 0.01), kw.get("radius_max", 50.0)
    ref = G.oracle().render_backward(osc, gi, ga, gd, nthreads=min(16, os.cpu_count() or 1), margins=True)
    o = _outputs(out)
    assert np.array_equal(o["vis"], ref["vis"])
    bad = G.pixel_errors(o, ref)
    edge = G.knife_edge(ref["margin"])
    for y, x in zip(*np.nonzero(bad)):
        print(f"{label} px ({y},{x}): image err {np.abs(o['image'][:, y, x] - ref['image'][:, y, x]).max():.3g} "
              f"alpha {o['alpha'][0, y, x]:.7f} vs {ref['alpha'][0, y, x]:.7f}; margins w {ref['margin'][0, y, x]:.3g} "
              f"ulps, A {ref['margin'][1, y, x]:.3g} ulps")
    print(f"{label}: {int(bad.sum())} of {H * W} px out of tolerance, {int((bad & edge).sum())} of them knife-edge; "
          f"knife-edge px overall {int(edge.sum())}, flipped {int(G.flipped_pixels(o, ref, edge).sum())}; "
          f"T={ref['T']} E={ref['E']} C={ref['C']}")
    errs = G.check_image(o, ref, exempt=edge if knife else None) + G.check_projection(o, ref)
    ds, dr = G.oracle().covariance_backward(sc.scaling.numpy(), sc.rotation.numpy(), ref["grads"]["cov3d"])
    op = torch.sigmoid(sc.opacity[:, 0]).numpy()
    # Gradients: a knife-edge pixel whose decision flipped changes the
    # gradient of every Gaussian in its chain; those Gaussians (footprint
    # covering the pixel) are exempt from the 1e-4 check and reported beside
    # the others.  Flipped = knife-edge and visibly different: image > 1e-5 or
    # alpha > 1e-6 (rounding differences are ~1e-7; a flip past the last
    # contributor moves A by that contributor's c, which may stay under the
    # 1e-4 image tolerance)
    flipped = G.flipped_pixels(o, ref, edge) if knife else np.zeros_like(edge)
    flipped = list(zip(*np.nonzero(flipped)))
    touch = G.touching_gaussians(o["means2d"], o["conics"], o["vis"], flipped)
    rows = ~touch
    pairs = (("xyz", _np(m._xyz.grad), ref["grads"]["xyz"]), ("scaling", _np(m._scaling.grad), ds),
             ("rotation", _np(m._rotation.grad), dr),
             ("features_dc", _np(m._features_dc.grad)[:, 0], ref["grads"]["color_logits"]),
             ("opacity", _np(m._opacity.grad)[:, 0], ref["grads"]["opacity"] * op * (1 - op)))
    for name, d, r in pairs:
        msg = f"{label} grad {name}: max err / max|ref| = {G.grad_rel_err(d, r, rows):.3g} over the {int(rows.sum())}"
        msg += f" Gaussians off the flipped pixels"
        if touch.any():
            msg += f"; {G.grad_rel_err(d, r, touch):.3g} over the {int(touch.sum())} touching them"
        print(msg)
        errs += G.check_grad(name, d, r, rows=rows)
    if touch.any():
        # Round-3 review (weak 8): the exempted Gaussians checked too.  The
        # oracle replays the frame again with the GPU's per-pixel termination
        # points (decision-forced: gso_scene.force_neval = the forward's n_eval,
        # every skip decision still its own), so a pixel whose A lands within
        # an ulp of 0.995 on one side and not the other is compared on the same
        # chain: image and EVERY Gaussian's gradient at the standard tolerances.
        RZ = pkg.rasterizer
        camp = pkg.camera_params(Cam(W, H, sc.fovx, sc.fovy, wv=wv), pkg.RenderSettings(H, W, torch.tensor(bg)),
                                 **{k: kw[k] for k in ("radius_min", "radius_max", "tile_size") if k in kw})
        pix_neval = torch.empty((H * W,), dtype=torch.int32, device=cuda)
        with torch.no_grad():
            RZ.forward_pipeline(camp, m._xyz, None, m._scaling, m._rotation, m._features_dc[:, 0, :],
                                torch.sigmoid(m._opacity).squeeze(1), pix_neval=pix_neval)
        neval = pix_neval.view(H, W).cpu().numpy()
        osc.force_neval = neval
        reff = G.oracle().render_backward(osc, gi, ga, gd, nthreads=min(16, os.cpu_count() or 1))
        badf = G.pixel_errors(o, reff)
        print(f"{label} decision-forced oracle: {int(badf.sum())} of {H * W} px out of tolerance")
        errs += G.check_image(o, reff)
        dsf, drf = G.oracle().covariance_backward(sc.scaling.numpy(), sc.rotation.numpy(), reff["grads"]["cov3d"])
        forced = (("xyz", _np(m._xyz.grad), reff["grads"]["xyz"]), ("scaling", _np(m._scaling.grad), dsf),
                  ("rotation", _np(m._rotation.grad), drf),
                  ("features_dc", _np(m._features_dc.grad)[:, 0], reff["grads"]["color_logits"]),
                  ("opacity", _np(m._opacity.grad)[:, 0], reff["grads"]["opacity"] * op * (1 - op)))
        for name, d, r in forced:
            print(f"{label} decision-forced grad {name}: max err / max|ref| = {G.grad_rel_err(d, r):.3g} over all "
                  f"{d.shape[0]} Gaussians ({G.grad_rel_err(d, r, touch):.3g} over the {int(touch.sum())} formerly exempt)")
            errs += [f"forced: {e}" for e in G.check_grad(name, d, r)]
    return errs, bad, edge


def test_c3_full_size_vs_oracle(pkg, cuda):
    """BASELINE config C3 (1M Gaussians, 1920x1080): full frame, fwd + bwd, vs
    the oracle (OpenMP).  Decisions match the oracle except where its replay
    came within rounding of a threshold; each such pixel is listed with its
    margins (golden_io.knife_edge) and no other pixel may differ."""
    W, H = 1920, 1080
    sc = pkg.synthetic.make_scene(1_000_000, W, H, seed=0)
    errs, bad, knife = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.0, 0.0, 0.0), label="C3")
    assert bad.sum() <= 64, f"{int(bad.sum())} knife-edge pixels"
    assert not errs, errs


def test_c2_full_size_vs_oracle(pkg, cuda):
    """BASELINE config C2 (100k Gaussians, 800x800, SURVEY 8(d) distribution),
    bg != 0 (the doubled-background path), fwd + bwd vs the oracle."""
    W, H = 800, 800
    sc = pkg.synthetic.make_scene(100_000, W, H, seed=2)
    errs, bad, knife = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.2, 0.3, 0.4), seed=3, label="C2")
    assert bad.sum() <= 16, f"{int(bad.sum())} knife-edge pixels"
    assert not errs, errs


def test_c2_posed_camera_vs_oracle(pkg, cuda):
    """C2 size through a rotated, translated camera (world_view_transform not
    the identity: the projection's Rv, Tv and the y flip at scale), fwd + bwd
    vs the oracle."""
    W, H = 800, 800
    sc = pkg.synthetic.make_scene(100_000, W, H, seed=12)
    ax, ay = np.radians(6.0), np.radians(-9.0)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    wv = np.eye(4)
    wv[:3, :3] = ry @ rx
    wv[:3, 3] = [0.12, -0.07, 0.25]
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.05, 0.1, 0.0), seed=4, label="C2 posed",
                                    wv=wv.astype(np.float32))
    assert bad.sum() <= 16
    assert not errs, errs


@pytest.mark.parametrize("tile", [1, 3, 4, 8, 20, 32, 64])
def test_tile_sizes_vs_oracle(pkg, cuda, tile):
    """GaussianRenderer(tile_size=L): every pixel blends its L x L tile's list
    (renderer.py:261-311), so L changes the image.  Partial edge tiles,
    cells clipped to tiles (L = 1, 3, 4, 20: one pixel per tile up to cells
    partly outside it), several cells per tile (32, 64)."""
    W, H = (200, 152) if tile >= 4 else (72, 56)
    sc = pkg.synthetic.make_scene(3000, W, H, seed=20 + tile, sigma_range=(0.01, 0.05))
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.1, 0.0, 0.3), renderer_kw=dict(tile_size=tile),
                                    label=f"tile{tile}")
    assert bad.sum() <= 2
    assert not errs, errs


@pytest.mark.parametrize("tile", [300, 480, 5000])
def test_large_tiles_vs_oracle(pkg, cuda, tile):
    """Large tile edges: 300 -- 3 x 2 tiles of 1,444 cells, partial
    edge tiles; 480: tiles as tall as the image; 5000, far above the image:
    rendered as one tile of max(W, H) = 640 px (renderer.effective_tile), while
    the oracle bins with the edge as given -- the same outputs, as the
    reference's one-tile binning predicts."""
    W, H = 640, 480
    sc = pkg.synthetic.make_scene(3000, W, H, seed=40, sigma_range=(0.01, 0.05))
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.1, 0.0, 0.3), renderer_kw=dict(tile_size=tile),
                                    label=f"tile{tile}")
    assert bad.sum() <= 2
    assert not errs, errs


@pytest.mark.parametrize("tile", [4150, 10 ** 6])
def test_wide_image_large_tiles_vs_oracle(pkg, cuda, tile):
    """Tile edges above 4096 px (GS_MAX_TILE is 16384 since round 6): a
    4200 x 40 image in two tiles of 4150 px (the second 50 px wide), and
    tile_size above the image, rendered as one tile of 4200 px -- both as the
    reference's binning (renderer.py:261-298).  519^2 / 525^2 cells per tile:
    the backward replays them in memory-bounded batches."""
    W, H = 4200, 40
    sc = pkg.synthetic.make_scene(2500, W, H, seed=53)
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.2, 0.1, 0.0), renderer_kw=dict(tile_size=tile),
                                    label=f"wide tile{tile}")
    assert bad.sum() <= 2
    assert not errs, errs


def test_max_tile_edge_vs_oracle(pkg, cuda):
    """The largest tile edge, GS_MAX_TILE = 16384: a 16384 x 8 image as one
    tile (2048^2 cells, 33.5 M blend workgroups, the partials in dozens of
    cell batches) against the oracle, gradients included."""
    W, H = pkg._native.GS_MAX_TILE, 8
    sc = pkg.synthetic.make_scene(1500, W, H, seed=59)
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.1, 0.2, 0.3), renderer_kw=dict(tile_size=10 ** 6),
                                    label="max tile")
    assert bad.sum() <= 2
    assert not errs, errs


def test_wide_rects_vs_oracle(pkg, cuda):
    """radius_max far above the default: rectangles up to 101 x 76 tiles of
    4 px, so a round of 256 Gaussians emits ~1M entries through many windows
    of the emission's LDS owner map; radius_min clamps the small ones."""
    W, H = 300, 200
    sc = pkg.synthetic.make_scene(600, W, H, seed=31, sigma_range=(0.02, 0.6), z_range=(2.0, 3.0))
    sc.opacity.fill_(-3.0)
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.0, 0.2, 0.1),
                                    renderer_kw=dict(tile_size=4, radius_min=2.5, radius_max=200.0), label="wide")
    assert bad.sum() <= 2
    assert not errs, errs


def test_sparse_frame_vs_oracle(pkg, cuda):
    """A few small Gaussians in a 640 x 480 frame of 4-px tiles (19,200
    tiles): runs of thousands of empty tiles between the tile lists, written
    by whole waves in k_tile_ranges."""
    W, H = 640, 480
    sc = pkg.synthetic.make_scene(6, W, H, seed=47, sigma_range=(0.004, 0.01))
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.3, 0.1, 0.0), renderer_kw=dict(tile_size=4),
                                    label="sparse")
    assert bad.sum() <= 2
    assert not errs, errs


@pytest.mark.parametrize("bg", [(0.95, 0.6, 0.0), (1.0, 1.0, 1.0)])
def test_clamped_pixels_vs_oracle(pkg, cuda, bg):
    """Composites that leave [0, 1]: the blend backward reads its per-pixel
    state from the forward's outputs and a clamp-flag byte (round 5), so a
    blocked channel's gradient must come from the flag, not from the
    clamped image.  A bright background (counted twice, renderer.py:273,
    :359) saturates many pixels' red channel; white saturates all three."""
    W, H = 160, 120
    sc = pkg.synthetic.make_scene(6000, W, H, seed=77, sigma_range=(0.01, 0.06))
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, bg, seed=7, label=f"bg {bg}")
    assert bad.sum() <= 2
    assert not errs, errs
    # (the scene does clamp: a forward of it has saturated pixels)
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
    with torch.no_grad():
        img = pkg.GaussianRenderer().render(Cam(W, H, sc.fovx, sc.fovy), m,
                                            pkg.RenderSettings(H, W, torch.tensor(bg)))["image"]
    assert int((img[0] == 1.0).sum()) > 100


@pytest.mark.parametrize("wh", [(1, 1), (5, 3), (17, 1), (1, 33), (129, 65)])
def test_odd_image_sizes_vs_oracle(pkg, cuda, wh):
    """Images of one pixel, one row, one column, and sizes just past a tile
    multiple: every cell of a tile but one is outside the image."""
    W, H = wh
    sc = pkg.synthetic.make_scene(400, W, H, seed=40 + W + H, sigma_range=(0.01, 0.2))
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.2, 0.1, 0.0), label=f"{W}x{H}")
    assert bad.sum() <= 1
    assert not errs, errs


def test_4k_frame_vs_oracle(pkg, cuda):
    """3840x2160 (32,400 tiles: 15-bit tile keys), fwd + bwd vs the oracle."""
    W, H = 3840, 2160
    sc = pkg.synthetic.make_scene(60_000, W, H, seed=9)
    errs, bad, _ = _scene_vs_oracle(pkg, cuda, sc, W, H, (0.0, 0.0, 0.0), label="4K")
    assert bad.sum() <= 16
    assert not errs, errs


class _OneRankDist:
    """torch.distributed stand-in for one rank: all_reduce is the identity,
    slices handed to it are recorded."""
    class ReduceOp:
        SUM, AVG = "sum", "avg"

    class _Work:
        def wait(self):
            return True

    def __init__(self):
        self.sliced = []

    def is_initialized(self):
        return False

    def get_world_size(self, group=None):
        return 1

    def all_reduce(self, t, op=None, group=None, async_op=False):
        self.sliced.append(t.numel())
        return self._Work() if async_op else None


def test_grad_bucket_adoption(pkg, cuda):
    """GradAllReduce.attach (data-parallel path): the render backward writes
    the gradients straight into the all-reduce bucket and autograd adopts the
    views as .grad (no copies); the values equal a plain backward's."""
    syn = pkg.synthetic
    sc = syn.make_scene(20000, 320, 240, seed=3)
    res = []
    for attach in (False, True):
        m = syn.to_model(sc, pkg.GaussianModel, cuda)
        params = m.grad_parameters()
        stub = _OneRankDist()
        red = pkg.distributed.GradAllReduce(params, dist=stub, chunks=2, min_chunk_rows=4096)
        if attach:
            red.attach(m)
        out = pkg.GaussianRenderer().render(Cam(320, 240, sc.fovx, sc.fovy), m,
                                            pkg.RenderSettings(240, 320, torch.zeros(3)))
        (out["image"].sum() + out["depth"].sum()).backward()
        if attach:
            # the backward handed its rows over in two ranges, one slice per parameter each
            assert red.ranges_reduced == 2 and len(stub.sliced) == 2 * len(params)
            red2 = pkg.distributed.GradAllReduce(params, dist=_OneRankDist())
            assert red2.overlap_chunks() == 1  # the default: the whole bucket in one call
            assert sum(stub.sliced) == sum(p.numel() for p in params)
            red.all_reduce_mean()
        res.append([p.grad.clone() for p in params])
        if attach:
            for p, v in zip(params, torch.split(red._flat, red._sizes)):
                assert p.grad.data_ptr() == v.data_ptr()
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("native", [True, False])
def test_rccl_range_reduction_world1(pkg, cuda, native, monkeypatch):
    """The RCCL path itself (backend nccl, world size 1, in this process): the
    backward hands its rows over in ranges, each range's five parameter
    slices reduced as one collective group -- through the native RCCL
    communicator (rccl.RcclComm) or torch.distributed's coalescing manager --;
    the gradients equal a plain backward's bit for bit (a mean over one rank),
    and a pipelined Adam (GradAllReduce.reduce_and_step -> FusedAdam.step_ranges)
    equals one FusedAdam step on them."""
    monkeypatch.setenv("GS_DP_NATIVE", "1" if native else "0")
    import os
    import socket
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group already exists")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(cuda))
    try:
        syn = pkg.synthetic
        sc = syn.make_scene(20000, 320, 240, seed=5)
        res, stepped = [], []
        for ranges in (0, 1, 3, 3):
            m = syn.to_model(sc, pkg.GaussianModel, cuda)
            params = m.grad_parameters()
            opt = pkg.optim.FusedAdam([{"params": [p], "lr": 1e-3} for p in params])
            red = None
            if ranges:
                red = pkg.distributed.GradAllReduce(params, chunks=ranges, min_chunk_rows=4096).attach(m)
                assert red._coalesce and (red._native is not None) == native
            out = pkg.GaussianRenderer().render(Cam(320, 240, sc.fovx, sc.fovy), m,
                                                pkg.RenderSettings(240, 320, torch.zeros(3)))
            (out["image"].sum() + out["alpha"].sum() + out["depth"].sum()).backward()
            if red is not None:
                assert red.ranges_reduced == ranges
            if red is not None and len(res) == 3:
                red.reduce_and_step(opt)  # pipelined: each range's Adam behind its collective
            else:
                if red is not None:
                    red.all_reduce_mean()
                opt.step()
            torch.cuda.synchronize()
            res.append([p.grad.clone() for p in params])
            stepped.append([p.detach().clone() for p in params])
        for other in res[1:]:
            for a, b in zip(res[0], other):
                assert torch.equal(a, b)
        for other in stepped[1:]:
            for a, b in zip(stepped[0], other):
                assert torch.equal(a, b)
    finally:
        pkg.distributed.close_native_comms()
        dist.destroy_process_group()


def test_depth_window_miss_rerenders(pkg, cuda):
    """The depth sort runs over a window of key bits chosen from the union of
    the last frames' visible depth ranges (rasterizer._window_for); a frame
    whose depths leave the window is rendered again with 32-bit keys (a miss,
    counted), and a second miss within _MISS_SPAN frames turns windows off for
    a while.  Held, missed and windowless frames all equal the frame a fresh
    renderer gives, bit for bit."""
    RZ = pkg.rasterizer
    syn = pkg.synthetic
    W, H = 320, 240
    narrow = syn.make_scene(20000, W, H, seed=41, z_range=(2.0, 2.5))
    wide = syn.make_scene(20000, W, H, seed=42, z_range=(0.5, 60.0))

    def frame(sc):
        m = syn.to_model(sc, pkg.GaussianModel, cuda)
        out = pkg.GaussianRenderer().render(Cam(W, H, sc.fovx, sc.fovy), m, pkg.RenderSettings(H, W, torch.zeros(3)))
        (out["image"].sum() + out["depth"].sum()).backward()
        return out["image"].clone(), out["depth"].clone(), m._xyz.grad.clone(), m._scaling.grad.clone()

    def reset():
        RZ._DEPTH_HIST.pop(cuda, None)
        RZ._WINDOW_STATE.pop(cuda, None)

    def misses():
        return RZ.depth_window_stats(cuda)["misses"]

    try:
        reset()
        fresh_wide = frame(wide)             # 32-bit keys (no history yet)
        reset()
        frame(narrow)                        # a narrow window for the next frame
        w = RZ._window_for(cuda)
        assert w is not None and w[1] <= 24
        missed = frame(wide)                 # leaves the window: re-rendered with 32-bit keys
        assert misses() == 1
        held = frame(wide)                   # the union of both ranges now
        frame(narrow)
        held_narrow = frame(narrow)          # inside the union: no miss
        assert misses() == 1
        reset()
        fresh_narrow = frame(narrow)
        for a, b in zip(fresh_wide, missed):
            assert torch.equal(a, b)
        for a, b in zip(fresh_wide, held):
            assert torch.equal(a, b)
        for a, b in zip(fresh_narrow, held_narrow):
            assert torch.equal(a, b)
        # the wide frame misses a narrow-only history; once it has left the
        # history again it misses again, and a second miss within _MISS_SPAN
        # frames switches the windows off
        again = frame(wide)                  # miss 1 after the reset
        for _ in range(RZ._WINDOW_FRAMES):
            frame(narrow)
        again2 = frame(wide)                 # miss 2, RZ._WINDOW_FRAMES + 1 frames later
        assert misses() == 2 and RZ._window_for(cuda) is None
        for a, b, c in zip(fresh_wide, again, again2):
            assert torch.equal(a, b) and torch.equal(a, c)
    finally:
        reset()


@pytest.mark.parametrize("frame_calls", [True, False])
def test_no_gaussians(pkg, cuda, frame_calls):
    """N = 0 (an empty model): the early return of renderer.py:74-83 (bg once,
    zero alpha and depth) and empty gradients (through the frame entry points
    and the stage path, bit for bit alike)."""
    out, g = _empty_frame(pkg, cuda, "empty", frame_calls)
    assert torch.allclose(out["image"].cpu(), torch.tensor([0.2, 0.3, 0.4]).view(3, 1, 1).expand(3, 24, 32))
    assert out["alpha"].abs().sum() == 0 and out["depth"].abs().sum() == 0
    assert out["viewspace_points"].shape == (0, 2) and out["radii"].shape == (0,)
    assert g.xyz.grad is not None and g.xyz.grad.shape == (0, 3)
    _assert_same_empty_frame(pkg, cuda, "empty")


def test_float64_inputs_cast(pkg, cuda):
    """Stub Gaussians in float64 (the reference's torch code would accept
    them): rendered as their fp32 cast, gradients flowing back to the fp64
    leaves; an input on another device raises instead of being read."""
    cam = Cam(64, 64, np.radians(60), np.radians(60))
    st = pkg.RenderSettings(64, 64, torch.zeros(3))
    args = ([[0, 0, 1], [0.1, 0, 2]], np.stack([np.diag([1e-3] * 3)] * 2), [[1, 0, 0], [0, 1, 0]], [0.5, 0.7])
    g32 = Gauss(*args, cuda)
    g64 = Gauss(*args, cuda)
    for name in ("xyz", "cov", "feats", "op"):
        setattr(g64, name, getattr(g64, name).detach().double().requires_grad_())
    a = pkg.GaussianRenderer().render(cam, g32, st)
    b = pkg.GaussianRenderer().render(cam, g64, st)
    for k in ("image", "alpha", "depth"):
        assert torch.equal(a[k], b[k]), k
    # the reference's output dtypes: projection outputs in the input dtype,
    # image in the background's, alpha / depth float32
    for k in ("viewspace_points", "conics", "radii"):
        assert b[k].dtype == torch.float64 and torch.equal(b[k].float(), a[k]), k
    assert b["image"].dtype == torch.float32 and b["alpha"].dtype == b["depth"].dtype == torch.float32
    st64 = pkg.RenderSettings(64, 64, torch.zeros(3, dtype=torch.float64))
    assert pkg.GaussianRenderer().render(cam, g64, st64)["image"].dtype == torch.float64
    (a["image"].sum() + a["depth"].sum()).backward()
    (b["image"].sum() + b["depth"].sum()).backward()
    assert g64.xyz.grad.dtype == torch.float64
    assert torch.allclose(g64.xyz.grad.float(), g32.xyz.grad) and torch.allclose(g64.op.grad.float(), g32.op.grad)
    g_bad = Gauss(*args, cuda)
    g_bad.op = g_bad.op.detach().cpu()
    with pytest.raises(RuntimeError, match="opacity"):
        pkg.GaussianRenderer().render(cam, g_bad, st)


@pytest.mark.parametrize("n,w,h,tile", [(20000, 320, 240, 16), (100000, 800, 800, 16), (6000, 200, 152, 8),
                                         (1000000, 1920, 1080, 16)])
def test_index_work_bit_exact(pkg, cuda, n, w, h, tile):
    """The integer and index stages bit-exact: the visible set and
    count M, the depth order (ascending z, ties by Gaussian index -- a stable
    sort of the frame's own depths), each visible Gaussian's tile rectangle by
    the reference's int() rule (renderer.py:278-293), and every tile's list
    (renderer.py:294-298: Gaussians in depth order) with its [start, end)
    range, T entries in all.  The GPU's own projections are the inputs, so no
    rounding enters; M, T and the depth order are also equal to the oracle's
    on these scenes."""
    from mini3dgs_amd import rasterizer as RZ
    sc = pkg.synthetic.make_scene(n, w, h, seed=n % 97)
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
    cam = pkg.camera_params(Cam(w, h, sc.fovx, sc.fovy), pkg.RenderSettings(h, w, torch.zeros(3)), tile_size=tile)
    with torch.no_grad():
        _, _, _, means2d, _, radii, vis, fr = RZ.forward_pipeline(
            cam, m._xyz, None, m._scaling, m._rotation, m._features_dc[:, 0, :],
            torch.sigmoid(m._opacity).squeeze(1))
    torch.cuda.synchronize()
    M, T = fr.M, fr.T
    z = fr.records.view(-1, 12)[:, 9].cpu().numpy()
    order = fr.order.cpu().numpy()[:M].astype(np.int64)
    # the statement (device_frame_util.index_statement, shared with the device-resident frames' tests)
    st = index_statement(means2d.cpu().numpy(), radii.cpu().numpy(), vis.cpu().numpy(), z, w, h, tile)
    vidx = st.vidx
    assert M == len(vidx)
    assert np.array_equal(order, st.order)
    # rectangles: renderer.py:278-293 from this frame's means and radii
    rects = fr.rects.view(-1, 2).cpu().numpy().astype(np.int64)
    gx0, gx1, gy0, gy1 = rects[:, 0] & 0xFFFF, rects[:, 0] >> 16, rects[:, 1] & 0xFFFF, rects[:, 1] >> 16
    v = vidx[st.ne[vidx]]
    assert np.array_equal(gx0[v], st.x0[v] // tile) and np.array_equal(gx1[v], (st.x1[v] - 1) // tile)
    assert np.array_equal(gy0[v], st.y0[v] // tile) and np.array_equal(gy1[v], (st.y1[v] - 1) // tile)
    # tile lists: every (tile, Gaussian) of the depth-ordered rectangles, stable by tile
    assert T == st.T
    assert np.array_equal(fr.sorted_gauss[:T].cpu().numpy().astype(np.int64), st.gauss)
    counts, starts = st.counts, st.starts
    rng_ = fr.ranges.cpu().numpy().astype(np.int64)
    nz = counts > 0
    assert np.array_equal(rng_[nz, 0], starts[nz]) and np.array_equal(rng_[nz, 1], (starts + counts)[nz])
    assert np.all(rng_[~nz, 0] == rng_[~nz, 1])
    # and the oracle's count and order on the same scene
    if tile == 16:
        cov = G.oracle().covariance(sc.scaling.numpy(), sc.rotation.numpy())
        ref = G.oracle().render_forward(_oracle_scene(sc, cov, (0.0, 0.0, 0.0)), nthreads=8)
        assert ref["M"] == M and ref["T"] == T
        assert np.array_equal(ref["sorted_idx"].astype(np.int64), order)


def test_counters_polled_and_copied_agree(pkg, cuda):
    """(M, T) reach the host either written by gs_bin_count into the pinned
    buffer through its device address and polled (the default), or copied in
    the stream behind an event (where the runtime does not map the buffer):
    both give the same frame, including a frame whose T exceeds the previous
    frame's capacity guess (a re-emission)."""
    from mini3dgs_amd import rasterizer as RZ
    syn = pkg.synthetic
    W, H = 256, 192
    small, big = (syn.make_scene(n, W, H, seed=90 + n % 7) for n in (2000, 30000))
    st = pkg.RenderSettings(H, W, torch.tensor([0.0, 0.1, 0.2]))

    def frames():
        out = []
        for sc in (small, big, small):
            m = syn.to_model(sc, pkg.GaussianModel, cuda)
            with torch.no_grad():
                o = pkg.GaussianRenderer().render(Cam(W, H, sc.fovx, sc.fovy), m, st)
            out.append((o["image"].clone(), o["alpha"].clone()))
        return out

    polled = frames()
    hc = RZ._HOST_COUNTERS.bufs[cuda]
    assert hc.dptr is not None  # the runtime maps pinned memory on this image
    saved = hc.dptr
    try:
        hc.dptr = None
        RZ._T_SEEN.pop(cuda, None)
        copied = frames()
    finally:
        hc.dptr = saved
    for (a, b), (c, d) in zip(polled, copied):
        assert torch.equal(a, c) and torch.equal(b, d)


def test_concurrent_renders_two_threads(pkg, cuda):
    """SURVEY 8(b) threading row: renders from two host threads on their own
    streams, concurrently, give each thread's frames exactly as a lone render
    does (each thread reads back its own counters)."""
    import threading
    syn = pkg.synthetic
    W, H = 320, 240
    scenes = [syn.make_scene(n, W, H, seed=70 + i) for i, n in enumerate((15000, 40000))]
    models = [syn.to_model(sc, pkg.GaussianModel, cuda) for sc in scenes]
    st = pkg.RenderSettings(H, W, torch.tensor([0.1, 0.1, 0.1]))

    def render(i):
        with torch.no_grad():
            return pkg.GaussianRenderer().render(Cam(W, H, scenes[i].fovx, scenes[i].fovy), models[i], st)["image"]
    want = [render(0).clone(), render(1).clone()]
    torch.cuda.synchronize()
    got = [[], []]
    errors = []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(6):
                    got[i].append(render(i).clone())
            s.synchronize()
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(i,)) for i in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not errors, errors
    for i in (0, 1):
        assert len(got[i]) == 6
        for img in got[i]:
            assert torch.equal(img, want[i]), i


def test_frame_poll_timeout_synchronises_before_failing(pkg, cuda):
    """gs_render_forward's counter poll gives up after its
    patience (here 1 ms) only after synchronising the stream and reading the
    word once more -- a healthy stream with a long queue ahead of the count
    renders normally (the same image as without the queue)."""
    RZ = pkg.rasterizer
    sc = pkg.synthetic.make_scene(20000, 320, 240, seed=4)
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
    st = pkg.RenderSettings(240, 320, torch.tensor([0.1, 0.2, 0.3]))
    cam = Cam(320, 240, sc.fovx, sc.fovy)
    with torch.no_grad():
        ref = pkg.GaussianRenderer().render(cam, m, st)["image"].clone()
        saved = RZ._POLL_TIMEOUT_MS
        try:
            RZ._POLL_TIMEOUT_MS = 1
            a = torch.randn(4096, 4096, device=cuda)
            for _ in range(40):  # tens of ms of work queued ahead of the frame's count
                a = a @ a
                a = a / a.abs().max()
            out = pkg.GaussianRenderer().render(cam, m, st)["image"]
        finally:
            RZ._POLL_TIMEOUT_MS = saved
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_second_backward_of_one_frame(pkg, cuda):
    """a second backward over the same frame
    (retain_graph=True) clears the slot flags the first one left, at the
    default tile (frame entry points) and at a tile replayed in cell batches
    (stage path): the gradients accumulate to exactly twice the first."""
    RZ = pkg.rasterizer
    sc = pkg.synthetic.make_scene(3000, 96, 72, seed=6, sigma_range=(0.005, 0.03))
    saved = RZ.PARTIAL_BUDGET_BYTES
    try:
        for tile, budget in ((16, saved), (64, 41 * 2000 * 8)):
            RZ.PARTIAL_BUDGET_BYTES = budget
            m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
            out = pkg.GaussianRenderer(tile_size=tile).render(Cam(96, 72, sc.fovx, sc.fovy), m,
                                                             pkg.RenderSettings(72, 96, torch.tensor([0.1, 0.2, 0.3])))
            loss = out["image"].sum() + out["alpha"].mean()
            loss.backward(retain_graph=True)
            first = [p.grad.clone() for p in m.grad_parameters() if p.grad is not None]
            loss.backward()
            second = [p.grad for p in m.grad_parameters() if p.grad is not None]
            for a_, b_ in zip(first, second):
                assert torch.equal(b_, a_ * 2), tile
    finally:
        RZ.PARTIAL_BUDGET_BYTES = saved
