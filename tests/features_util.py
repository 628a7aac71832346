"""Helpers of tests/test_features_gpu.py: rendering a fixture with a feature
tensor, the pinned oracle's expectation for any C and range, and the child
process of the cell-batch test (GS_PARTIAL_BUDGET is read at import)."""
import dataclasses
import os
import sys

import numpy as np
import torch

import golden_io as G
from stubs import Cam, Gauss


def np_(t):
    return t.detach().float().cpu().numpy()


def tensor(a, dev, grad=False):
    return torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=grad)


def settings_of(pkg, f):
    return pkg.RenderSettings(image_height=int(f["height"]), image_width=int(f["width"]),
                              bg_color=torch.tensor(np.asarray(f["bg"], np.float32)))


def camera_of(f):
    return Cam(f["cam_width"], f["cam_height"], f["fovx"], f["fovy"], f["wv"])


def gaussians_of(pkg, dev, f):
    """(model, leaves): the fixture's Gaussians -- this package's GaussianModel
    (raw scaling / rotation, the fused path) when the fixture has them, else
    the reference-style stub (cov3d).  leaves: name -> leaf tensor, named as
    the fixture's golden gradients d_<name>; "logits" is the [N, 3] DC colour."""
    n = f["xyz"].shape[0]
    if "scaling" in f:
        m = pkg.GaussianModel()
        m._set(tensor(f["xyz"], dev), tensor(f["color_logits"], dev).reshape(n, 1, 3),
               torch.zeros(n, 15, 3, device=dev), tensor(f["scaling"], dev), tensor(f["rotation"], dev),
               tensor(f["opacity_raw"], dev).reshape(n, 1))
        leaves = dict(xyz=m._xyz, scaling=m._scaling, rotation=m._rotation, opacity_raw=m._opacity,
                      color_logits=m._features_dc)
        return m, leaves, m._features_dc[:, 0, :]
    g = Gauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], dev)
    return g, dict(xyz=g.xyz, cov3d=g.cov, opacity=g.op, color_logits=g.feats), g.feats[:, 0, :]


def leaf_grad(name, t, n):
    """A leaf's gradient in its golden fixture's shape (zeros when none came)."""
    g = np.zeros(tuple(t.shape), np.float32) if t.grad is None else np_(t.grad)
    if name == "color_logits":
        return g.reshape(n, -1, 3)[:, 0, :]
    if name in ("opacity", "opacity_raw"):
        return g.reshape(n)
    return g


def render(pkg, dev, f, features=None, model=None, camera=None):
    model = gaussians_of(pkg, dev, f)[0] if model is None else model
    kw = {} if features is None else {"features": features}
    out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(camera or camera_of(f), model, settings_of(pkg, f), **kw)
    return model, out


def camera_depths(f):
    """Each Gaussian's camera-space Z in fp32, in the projection's order."""
    wv, x = np.asarray(f["wv"], np.float32), np.asarray(f["xyz"], np.float32)
    return ((x[:, 0] * wv[2, 0] + x[:, 1] * wv[2, 1]) + x[:, 2] * wv[2, 2]) + wv[2, 3]


def random_features(n, c, seed):
    """F01 ~ U(0.05, 0.95) [n, c], per-channel a (|a| in [0.5, 3], random sign:
    inside the [-3, 3] range, away from 0 where the map back through a would
    divide by nothing), b in [-2, 2]; F = a F01 + b."""
    rng = np.random.default_rng(seed)
    f01 = rng.uniform(0.05, 0.95, (n, c))
    a = rng.uniform(0.5, 3.0, c) * rng.choice([-1.0, 1.0], c)
    b = rng.uniform(-2.0, 2.0, c)
    return f01, a, b


def oracle_features(f, f01, a, b, g_features=None):
    """The pinned oracle's feature image for F = a F01 + b, and with a
    cotangent its gradients: the oracle renders ceil(C/3) colour passes with
    color_logits = logit(F01[:, 3j:3j+3]) and bg = 0, where its image is
    sum_i c_i F01 (no clamp binds), so features = a E01 + b alpha.  Backward:
    g_image = a gF per pass, g_alpha = sum_k b_k gF_k once; the geometry
    gradients add over the passes, d_color_logits maps back through
    F01 (1 - F01) and a."""
    o = G.oracle()
    n, c = f01.shape
    passes = (c + 2) // 3
    pad = np.full((n, 3 * passes), 0.5)
    pad[:, :c] = f01
    H, W = int(f["height"]), int(f["width"])
    base = G.scene_of(f)
    exp = np.zeros((c, H, W))
    grads = None if g_features is None else dict(xyz=0.0, cov3d=0.0, opacity=0.0, features=np.zeros((n, c)))
    edge = np.zeros((H, W), bool)
    alpha = None
    for j in range(passes):
        p01 = pad[:, 3 * j:3 * j + 3]
        sc = dataclasses.replace(base, color_logits=np.log(p01 / (1 - p01)).astype(np.float32),
                                 bg=np.zeros(3, np.float32))
        ks = [k for k in range(3 * j, 3 * j + 3) if k < c]
        if g_features is None:
            r = o.render_forward(sc, margins=True)
        else:
            gi = np.zeros((3, H, W), np.float32)
            for k in ks:
                gi[k - 3 * j] = a[k] * g_features[k]
            ga = np.tensordot(b, g_features, 1) if j == 0 else np.zeros((H, W))
            r = o.render_backward(sc, gi, ga, np.zeros((H, W)), margins=True)
            for name in ("xyz", "cov3d", "opacity"):
                grads[name] = grads[name] + r["grads"][name].astype(np.float64)
            p32 = 1.0 / (1.0 + np.exp(-sc.color_logits.astype(np.float64)))
            for k in ks:
                grads["features"][:, k] = r["grads"]["color_logits"][:, k - 3 * j] / (
                    p32[:, k - 3 * j] * (1 - p32[:, k - 3 * j])) / a[k]
        edge |= G.knife_edge(r["margin"])
        alpha = r["alpha"][0].astype(np.float64)
        for k in ks:
            exp[k] = a[k] * r["image"][k - 3 * j] + b[k] * alpha
    return exp, grads, edge


def feature_case(pkg, dev, f, c, seed, backward=True):
    """One render of fixture f (cov3d stub) with random features [N, c] and
    one backward of <gF, features>; everything as numpy."""
    n = f["xyz"].shape[0]
    f01, a, b = random_features(n, c, seed)
    H, W = int(f["height"]), int(f["width"])
    gF = np.random.default_rng(seed + 1).uniform(-1, 1, (c, H, W)).astype(np.float32)
    g = Gauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], dev)
    F = tensor(a * f01 + b, dev, grad=True)
    _, out = render(pkg, dev, f, F, model=g)
    res = dict(f01=f01, a=a, b=b, gF=gF, features=np_(out["features"]))
    if backward:
        (out["features"] * tensor(gF, dev)).sum().backward()
        res.update(d_features=np_(F.grad), d_xyz=np_(g.xyz.grad), d_cov3d=np_(g.cov.grad),
                   d_opacity=np_(g.op.grad).reshape(n))
    return res


def _child(name, c, seed, path):
    """The cell-batch test's child: the same case twice under the
    GS_PARTIAL_BUDGET of its environment, asserted bitwise equal, saved."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    f = G.load(name)
    r1, r2 = (feature_case(pkg, dev, f, c, seed) for _ in range(2))
    keys = ("features", "d_features", "d_xyz", "d_cov3d", "d_opacity")
    same = all(np.array_equal(r1[k], r2[k]) for k in keys)
    T = int(pkg.rasterizer._T_SEEN[dev])
    batch = pkg.rasterizer.cell_batch(pkg.rasterizer.CameraParams(1, 1, 1, 1, 0, 0, (0,) * 12, (0, 0, 0),
                                                                 tile_size=int(f["tile"])).cells, T)
    np.savez(path, same=same, batch=batch, **{k: r1[k] for k in keys})


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
