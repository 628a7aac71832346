"""Parameter rows with a stride other than the dense one.  gs_gaussians carries
xyz_stride, color_stride, opacity_stride and sh_rest_stride, and the rasterizer
hands strided views through without a copy -- the layout of a model that keeps
its SH features in one [N,16,3] tensor.  A render of such views must equal,
bit for bit, the render of contiguous clones of the same values, and the
gradients must reach the base buffers inside the views and nowhere else."""
import pytest
import torch

from stubs import Cam

pytestmark = pytest.mark.gpu

N_G, W, H = 3000, 96, 72
OUTS = ("image", "alpha", "depth", "means2d", "conics", "radii", "vis")


def _buffers(pkg, cuda):
    """Base buffers (leaves) whose views are the renderer's inputs."""
    sc = pkg.synthetic.make_scene(N_G, W, H, seed=31, sigma_range=(0.01, 0.05))
    g = torch.Generator().manual_seed(32)
    buf = torch.randn(N_G, 7, generator=g)
    buf[:, 1:4] = sc.xyz
    feats = 0.4 * torch.randn(N_G, 16, 3, generator=g)
    feats[:, 0, :] = torch.rand(N_G, 3, generator=g) * 4 - 2
    obuf = torch.randn(N_G, 5, generator=g)
    obuf[:, 2:3] = sc.opacity
    leaf = lambda t: t.to(cuda).requires_grad_()
    cam = pkg.camera_params(Cam(W, H, sc.fovx, sc.fovy), pkg.RenderSettings(H, W, torch.tensor([0.1, 0.2, 0.3])))
    return cam, dict(buf=leaf(buf), feats=leaf(feats), obuf=leaf(obuf), scaling=leaf(sc.scaling), rotation=leaf(sc.rotation))


def _views(b):
    xyz, logits, rest, op = b["buf"][:, 1:4], b["feats"][:, 0, :], b["feats"][:, 1:, :], b["obuf"][:, 2:3]
    assert (xyz.stride(0), logits.stride(0), rest.stride(0), op.stride(0)) == (7, 48, 48, 5)
    return xyz, logits, rest, op


def _cotangent(cuda):
    g = torch.Generator().manual_seed(33)
    return [(torch.rand(s, generator=g) * 2 - 1).to(cuda) for s in ((3, H, W), (1, H, W), (1, H, W), (N_G, 2))]


def _loss(out, cot, viewspace):
    """viewspace: with a cotangent on means2d (the generic projection backward; without, the training one)."""
    L = (out[0] * cot[0]).sum() + (out[1] * cot[1]).sum() + (out[2] * cot[2]).sum()
    return L + (out[3] * cot[3]).sum() if viewspace else L


@pytest.mark.parametrize("degree", [0, 3])
@pytest.mark.parametrize("frame_calls", [True, False])
def test_strided_views_render_as_dense(pkg, cuda, frame_calls, degree):
    RZ = pkg.rasterizer
    cam, b = _buffers(pkg, cuda)
    cot = _cotangent(cuda)
    saved = RZ._FRAME_CALLS
    try:
        RZ._FRAME_CALLS = frame_calls
        xyz, logits, rest, op = _views(b)
        out = RZ.rasterize(cam, xyz, None, b["scaling"], b["rotation"], logits, op, opacity_is_logit=True,
                           sh_rest=rest if degree else None, sh_degree=degree)
        _loss(out, cot, degree > 0).backward()
        dense = [t.detach().clone().contiguous().requires_grad_() for t in (xyz, logits, rest, op, b["scaling"], b["rotation"])]
        ref = RZ.rasterize(cam, dense[0], None, dense[4], dense[5], dense[1], dense[3], opacity_is_logit=True,
                           sh_rest=dense[2] if degree else None, sh_degree=degree)
        _loss(ref, cot, degree > 0).backward()
    finally:
        RZ._FRAME_CALLS = saved
    assert int(ref[6].sum()) > 1000
    for name, a, r in zip(OUTS, out, ref):
        assert torch.equal(a, r), name
    gb, gf, go = b["buf"].grad, b["feats"].grad, b["obuf"].grad
    assert torch.equal(gb[:, 1:4], dense[0].grad) and float(dense[0].grad.abs().max()) > 0
    assert not gb[:, [0, 4, 5, 6]].any()
    assert torch.equal(gf[:, 0, :], dense[1].grad) and float(dense[1].grad.abs().max()) > 0
    if degree:
        assert torch.equal(gf[:, 1:, :], dense[2].grad) and float(dense[2].grad.abs().max()) > 0
    else:
        assert not gf[:, 1:, :].any()
    assert torch.equal(go[:, 2:3], dense[3].grad) and float(dense[3].grad.abs().max()) > 0
    assert not go[:, [0, 1, 3, 4]].any()
    assert torch.equal(b["scaling"].grad, dense[4].grad) and torch.equal(b["rotation"].grad, dense[5].grad)


def test_strided_views_in_row_ranges(pkg, cuda):
    """The projection backward in row ranges (out["_chunks"]): every range's
    pointers advance by the views' own strides."""
    RZ = pkg.rasterizer
    cam, b = _buffers(pkg, cuda)
    cot = _cotangent(cuda)
    xyz, logits, rest, op = (t.detach() for t in _views(b))
    scl, rot = b["scaling"].detach(), b["rotation"].detach()
    got = []
    for strided, chunks in ((False, 1), (True, 3), (True, 1)):
        ins = (xyz, logits, rest, op) if strided else tuple(t.clone().contiguous() for t in (xyz, logits, rest, op))
        x, lg, rs, o = ins
        with torch.no_grad():
            img, al, dp, m2, cn, rd, vi, fr = RZ.forward_pipeline(cam, x, None, scl, rot, lg, o, opacity_is_logit=True,
                                                                  sh_rest=rs, sh_degree=3, need_grad=True)
        seen = []
        out = {"_rows_ready": lambda lo, hi: seen.append((lo, hi)), "_chunks": chunks}
        d = RZ.backward_pipeline(cam, fr, x, None, scl, rot, lg, o, m2, cn, cot[0], cot[1], cot[2], cot[3], None,
                                 opacity_is_logit=True, sh_rest=rs, sh_degree=3, out=out, outputs=(img, al, dp))
        assert seen == [(N_G * k // chunks, N_G * (k + 1) // chunks) for k in range(chunks)]
        got.append([t.clone() for t in (img, al, dp, m2, cn)] + [t.clone() for t in d if t is not None])
    for other in got[1:]:
        assert len(other) == len(got[0]) == 11
        for a, r in zip(other, got[0]):
            assert torch.equal(a, r)
    assert all(float(t.abs().max()) > 0 for t in got[0][5:])


@pytest.mark.parametrize("n", [16384, 16385])
def test_frame_entry_points_at_the_sort_switch(pkg, cuda, n):
    """n = 16384 Gaussians sort their depths in one workgroup in the frame
    entry points, 16385 with the radix passes: both equal the stage path bit
    for bit, outputs and gradients."""
    RZ = pkg.rasterizer
    syn = pkg.synthetic
    w, h = 320, 240
    sc = syn.make_scene(n, w, h, seed=41, sigma_range=(0.002, 0.01))
    res = []
    saved = RZ._FRAME_CALLS
    try:
        for fast in (False, True):
            RZ._FRAME_CALLS = fast
            m = syn.to_model(sc, pkg.GaussianModel, cuda)
            out = pkg.GaussianRenderer().render(Cam(w, h, sc.fovx, sc.fovy), m,
                                                pkg.RenderSettings(h, w, torch.tensor([0.1, 0.2, 0.3])))
            (out["image"].sum() + out["alpha"].mean() + out["depth"].mean() + out["viewspace_points"].sum()).backward()
            res.append([out[k].clone() for k in ("image", "alpha", "depth", "viewspace_points", "radii", "conics",
                                                 "visibility_filter")] +
                       [m._xyz.grad.clone(), m._scaling.grad.clone(), m._rotation.grad.clone(),
                        m._features_dc.grad.clone(), m._opacity.grad.clone()])
    finally:
        RZ._FRAME_CALLS = saved
    assert int(res[0][6].sum()) > n // 2
    for a, b in zip(*res):
        assert torch.equal(a, b)
