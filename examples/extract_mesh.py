"""From Gaussians to a triangle mesh: render a depth map per view, fuse the
maps into a TSDF volume, extract the surface with surface nets, write a PLY.

    vol = TSDFVolume.from_bounds(lo, hi, voxel_size, device)
    vol.integrate_renders(renderer, gaussians, cameras, depth="median")
    mesh = vol.extract_mesh()                      # {"vertices", "faces", "colors"}
    save_mesh_ply("mesh.ply", **mesh)

or, after training, trainer.extract_mesh(path="mesh.ply").  The scene here has
a known answer: flat opaque Gaussians on the unit sphere, their thin axis
radial, seen from the six axis directions.  The script prints, for the median
and the expected depth, the mesh's size and the mean and largest distance of
its vertices from the sphere, in world units and in voxels.

    python examples/extract_mesh.py [--gaussians 2000] [--size 64] [--voxel 0.1] [--out DIR]

Needs a HIP device.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class AxisCamera:
    """What the renderer and the fusion read of a camera: its size, its fields
    of view and its world-to-camera matrix (x right, y up, looking along +z)."""

    def __init__(self, size: int, fov: float, eye):
        import torch
        self._width = self._height = int(size)
        self._FoVx = self._FoVy = float(fov)
        eye = torch.tensor(eye, dtype=torch.float64)
        fwd = -eye / eye.norm()
        up = torch.tensor([0.0, 1.0, 0.0] if abs(float(fwd[2])) > 0.99 else [0.0, 0.0, 1.0], dtype=torch.float64)
        right = torch.linalg.cross(fwd, up)
        right = right / right.norm()
        R = torch.stack([right, torch.linalg.cross(right, fwd), fwd])
        wv = torch.eye(4, dtype=torch.float64)
        wv[:3, :3], wv[:3, 3] = R, -R @ eye
        self.world_view_transform = wv.float()


def sphere_model(pkg, n: int, device):
    import torch
    g = torch.Generator().manual_seed(11)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    # the rotation taking e_z to d: q = (1 + d_z, e_z x d)
    q = torch.nn.functional.normalize(torch.stack([1 + d[:, 2], -d[:, 1], d[:, 0], torch.zeros(n)], 1), dim=1)
    model = pkg.GaussianModel()
    model._set(d.to(device), (d.reshape(n, 1, 3) * 1.5).to(device), torch.zeros(n, 15, 3, device=device),
               torch.log(torch.tensor([0.06, 0.06, 0.004])).expand(n, 3).contiguous().to(device), q.to(device),
               torch.full((n, 1), 6.0).to(device))
    return model


def run(gaussians: int = 2000, size: int = 64, voxel: float = 0.1, out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    model = sphere_model(pkg, gaussians, dev)
    cams = [AxisCamera(size, 0.7, e) for e in ((4, 0, 0), (-4, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 4), (0, 0, -4))]
    renderer = pkg.GaussianRenderer()
    report = {}
    for depth in ("median", "expected"):
        vol = pkg.TSDFVolume.from_bounds((-1.3,) * 3, (1.3,) * 3, voxel, dev)
        vol.integrate_renders(renderer, model, cams, depth=depth)
        mesh = vol.extract_mesh()
        off = (mesh["vertices"].norm(dim=1) - 1.0).abs()
        report[depth] = {"dims": list(vol.dims), "vertices": int(mesh["vertices"].shape[0]),
                         "faces": int(mesh["faces"].shape[0]), "mean_abs_radius_error": float(off.mean()),
                         "max_abs_radius_error": float(off.max()), "mean_in_voxels": float(off.mean()) / voxel}
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            pkg.save_mesh_ply(os.path.join(out_dir, f"sphere_{depth}.ply"), mesh["vertices"], mesh["faces"], mesh["colors"])
        if verbose:
            r = report[depth]
            print(f"{depth:9s} depth: volume {r['dims']}, {r['vertices']} vertices, {r['faces']} faces, "
                  f"mean | |v| - 1 | = {r['mean_abs_radius_error']:.4f} ({r['mean_in_voxels']:.3f} voxels), "
                  f"max {r['max_abs_radius_error']:.4f}")
    return report


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=2000)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--out", default=None, help="directory for sphere_median.ply and sphere_expected.ply")
    a = ap.parse_args()
    run(a.gaussians, a.size, a.voxel, a.out)
