"""Generate the camera-pose gradient fixtures (tests/golden/pose/) by running
the REFERENCE renderer with the view matrix a leaf that requires grad.

    python tests/golden/make_pose_golden.py --ref <reference checkout> [--only NAME ...]

Like make_golden.py this runs at fixture-generation time only, never from the
tests.  Each case is rendered twice, in fp32 and in fp64 (every input cast,
torch's default dtype switched so that the renderer's own accumulators are
fp64 too), with the same cotangents; <name>.npz holds

  inputs : as make_golden.py (xyz, cov3d, color_logits, opacity, wv, sizes,
           fov, bg, tile, radii; + scaling, rotation, opacity_raw for the
           model case)
  cotangents: g_image, g_alpha, g_depth (+ g_means2d, g_conics)
  grads  : d_xyz, d_cov3d (or d_scaling, d_rotation), d_color_logits,
           d_opacity (or d_opacity_raw) of the fp32 run
  d_wv   : [4,4] dL/d(world_view_transform) of the fp32 run
  d_wv_f64: the same of the fp64 run

A case is refused (nothing written) when the two runs differ by more than
REF_DEV_MAX = 5e-5 of the largest fp64 entry of the R block or of the t
column: half of the gradient bar (golden_io.GRAD_RTOL = 1e-4), so that the
reference alone is shown to sit inside the bar and the GPU gets the other
half.  The measured deviations go to pose/manifest.json.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pose")
sys.path.insert(0, HERE)
from make_golden import ModelAdapter, StubCamera, fov_pair, synth  # noqa: E402

REF_DEV_MAX = 5e-5


class Gaussians:
    """make_golden.StubGaussians in a chosen dtype."""

    def __init__(self, xyz, cov3d, logits, opacity, dtype):
        n = xyz.shape[0]
        t = lambda a: torch.tensor(np.asarray(a, np.float32), dtype=dtype, requires_grad=True)
        self.xyz, self.cov = t(xyz), t(cov3d)
        feats = np.zeros((n, 16, 3), np.float32)
        feats[:, 0, :] = logits
        self.feats = t(feats)
        self.op = t(np.asarray(opacity, np.float32).reshape(n, 1))

    get_xyz = property(lambda s: s.xyz)
    get_covariance = property(lambda s: s.cov)
    get_features = property(lambda s: s.feats)
    get_opacity = property(lambda s: s.op)


def pose(ax, ay, t):
    """W2C [R | t]: a turn of ay about y after one of ax about x."""
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    wv = np.eye(4)
    wv[:3, :3] = Ry @ Rx
    wv[:3, 3] = t
    return wv.astype(np.float32)


def to_world(xc, wv):
    """Camera-frame points of synth() as world points seen by `wv`."""
    return ((xc - wv[:3, 3]) @ wv[:3, :3]).astype(np.float32)


def render_once(dtype, c, cot, model_state):
    from src.core.renderer import GaussianRenderer, RenderSettings
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        wv = torch.tensor(c["wv"], dtype=dtype, requires_grad=True)
        cam = StubCamera(c["cam_width"], c["cam_height"], c["fovx"], c["fovy"], wv)
        if model_state is not None:
            from src.core.gaussian_model import GaussianModel
            from config.config import TrainingConfig
            m = GaussianModel(TrainingConfig())
            for k, v in model_state.items():
                setattr(m, k, torch.nn.Parameter(v.detach().clone().to(dtype)))
            gs = ModelAdapter(m)
        else:
            m = None
            gs = Gaussians(c["xyz"], c["cov3d"], c["color_logits"], c["opacity"], dtype)
        st = RenderSettings(image_height=c["height"], image_width=c["width"],
                            bg_color=torch.tensor(c["bg"], dtype=dtype))
        out = GaussianRenderer(tile_size=c["tile"], radius_min=c["radius_min"],
                               radius_max=c["radius_max"]).render(cam, gs, st)
        loss = 0.0
        for key, name in (("g_image", "image"), ("g_alpha", "alpha"), ("g_depth", "depth"),
                          ("g_means2d", "viewspace_points"), ("g_conics", "conics")):
            if key in cot:
                loss = loss + (out[name] * torch.tensor(cot[key], dtype=dtype)).sum()
        if isinstance(loss, torch.Tensor) and loss.requires_grad:
            loss.backward()
        n = c["xyz"].shape[0]
        z = lambda t, shape: (t.grad.numpy() if t.grad is not None else np.zeros(shape))
        if m is not None:
            grads = dict(d_xyz=z(m._xyz, (n, 3)), d_scaling=z(m._scaling, (n, 3)), d_rotation=z(m._rotation, (n, 4)),
                         d_color_logits=z(m._features_dc, (n, 1, 3))[:, 0, :],
                         d_opacity_raw=z(m._opacity, (n, 1))[:, 0])
        else:
            grads = dict(d_xyz=z(gs.xyz, (n, 3)), d_cov3d=z(gs.cov, (n, 3, 3)),
                         d_color_logits=z(gs.feats, (n, 16, 3))[:, 0, :], d_opacity=z(gs.op, (n, 1))[:, 0])
        return z(wv, (4, 4)), grads, int(out["visibility_filter"].sum())
    finally:
        torch.set_default_dtype(old)


def run_pose_case(name, xyz, cov, logits, opac, wv, W, H, fovx, fovy, bg, cam_wh=None, extra_cot=False, seed=1,
                  model=None, tile=16):
    cw, ch = cam_wh if cam_wh is not None else (W, H)
    c = dict(width=W, height=H, cam_width=cw, cam_height=ch, fovx=fovx, fovy=fovy, wv=np.asarray(wv, np.float32),
             bg=np.asarray(bg, np.float32), tile=int(tile), radius_min=0.01, radius_max=50.0)
    state = None
    if model is not None:
        m = model
        state = {k: getattr(m, k) for k in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation",
                                             "_opacity")}
        c.update(xyz=m._xyz.detach().numpy(), scaling=m._scaling.detach().numpy(),
                 rotation=m._rotation.detach().numpy(), cov3d=m.compute_3d_covariance().detach().numpy(),
                 color_logits=m._features_dc.detach().numpy()[:, 0, :], opacity_raw=m._opacity.detach().numpy()[:, 0],
                 opacity=m.get_opacity.detach().numpy()[:, 0])
    else:
        c.update(xyz=xyz, cov3d=cov, color_logits=logits, opacity=np.asarray(opac, np.float32))
    g = np.random.default_rng(seed)
    n = c["xyz"].shape[0]
    cot = dict(g_image=g.uniform(-1, 1, (3, H, W)).astype(np.float32),
               g_alpha=g.uniform(-1, 1, (1, H, W)).astype(np.float32),
               g_depth=g.uniform(-1, 1, (1, H, W)).astype(np.float32))
    if extra_cot:
        cot["g_means2d"] = g.uniform(-1, 1, (n, 2)).astype(np.float32)
        cot["g_conics"] = g.uniform(-1, 1, (n, 2, 2)).astype(np.float32)
    d32, grads, visible = render_once(torch.float32, c, cot, state)
    d64, _, visible64 = render_once(torch.float64, c, cot, state)
    dev = {}
    for blk, sl in (("R", np.s_[:3, :3]), ("t", np.s_[:3, 3])):
        scale = float(np.abs(d64[sl]).max())
        dev[blk] = float(np.abs(d32[sl].astype(np.float64) - d64[sl]).max() / scale) if scale > 0 else 0.0
    rec = dict(name=name, N=int(n), W=W, H=H, tile=int(tile), visible=visible, ref_dev_R=dev["R"], ref_dev_t=dev["t"],
               max_R=float(np.abs(d64[:3, :3]).max()), max_t=float(np.abs(d64[:3, 3]).max()))
    if visible != visible64 or max(dev.values()) > REF_DEV_MAX or np.abs(d32[3]).max() != 0 or np.abs(d64[3]).max() != 0:
        raise SystemExit(f"{name}: refused -- fp32 vs fp64 reference {dev} (limit {REF_DEV_MAX}), visible "
                         f"{visible} / {visible64}: {rec}")
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **c, **cot,
                        **{k: np.asarray(v, np.float32) for k, v in grads.items()},
                        d_wv=d32.astype(np.float32), d_wv_f64=d64.astype(np.float64))
    return rec


def cases(only=None):
    out = []

    def want(n):
        return only is None or n in only

    wv = pose(0.2, 0.3, [0.3, -0.2, 0.5])
    for name, extra in (("pose_base", False), ("pose_extra_cot", True)):
        if want(name):
            rng = np.random.default_rng(21)
            xc, cov, lg, op, fx, fy = synth(60, 32, 32, rng, slo=0.02, shi=0.08)
            out.append(run_pose_case(name, to_world(xc, wv), cov, lg, op, wv, 32, 32, fx, fy, [0.2, 0.3, 0.4],
                                     extra_cot=extra))
    if want("pose_model"):
        # the reference GaussianModel through ModelAdapter (grads to the raw parameters)
        from src.core.gaussian_model import GaussianModel
        from config.config import TrainingConfig
        torch.manual_seed(23)
        m = GaussianModel(TrainingConfig())
        m.create_from_random(60, 1.0)
        wvm = pose(-0.15, 0.25, [0.1, 0.2, 3.2])
        with torch.no_grad():
            m._opacity.normal_()
            m._scaling.add_(torch.empty_like(m._scaling).uniform_(-0.2, 0.9))
        fx, fy = fov_pair(32, 32, 60.0)
        out.append(run_pose_case("pose_model", None, None, None, None, wvm, 32, 32, fx, fy, [0, 0, 0], model=m))
    if want("pose_culled"):
        # 40x24 image of a 44x28 camera; a third of the Gaussians behind the camera or off screen
        rng = np.random.default_rng(24)
        xc, cov, lg, op, fx, fy = synth(90, 40, 24, rng, slo=0.02, shi=0.08)
        xc[0::6, 2] *= -1.0                 # behind
        xc[1::6, 0] += 4.0 * xc[1::6, 2]    # far off screen
        wvc = pose(0.1, -0.35, [-0.4, 0.1, 0.3])
        out.append(run_pose_case("pose_culled", to_world(xc, wvc), cov, lg, op, wvc, 40, 24, fx, fy,
                                 [0.05, 0.1, 0.0], cam_wh=(44, 28), extra_cot=True))
    for name, tile in (("pose_tile8", 8), ("pose_tile_above", 100)):
        if want(name):
            rng = np.random.default_rng(25)
            xc, cov, lg, op, fx, fy = synth(50, 40, 32, rng, slo=0.02, shi=0.08)
            out.append(run_pose_case(name, to_world(xc, wv), cov, lg, op, wv, 40, 32, fx, fy, [0.1, 0.0, 0.2],
                                     tile=tile))
    if want("pose_all_behind"):
        rng = np.random.default_rng(26)
        xc, cov, lg, op, fx, fy = synth(20, 32, 32, rng, slo=0.02, shi=0.08)
        xc[:, 2] *= -1.0
        out.append(run_pose_case("pose_all_behind", to_world(xc, wv), cov, lg, op, wv, 32, 32, fx, fy,
                                 [0.2, 0.3, 0.4]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    man_path = os.path.join(OUT, "manifest.json")
    manifest = json.load(open(man_path)) if os.path.exists(man_path) else {}
    for rec in cases(set(a.only) if a.only else None):
        manifest[rec["name"]] = rec
        print(json.dumps(rec), flush=True)
    json.dump(manifest, open(man_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
