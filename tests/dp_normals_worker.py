"""One rank of the data-parallel normal-consistency test (tests/test_normals_gpu.py):
    python tests/dp_normals_worker.py <rank> <world> <port> <scene_dir> <out.npz>
tests/dp_filter3d_worker.py's run with lambda_normal on in place of the filter:
six iterations, the second a densification.  The rotation's gradient arrives in
two pieces (the render's and the normals'), so no render may write into the
bucket: the worker counts the renders that were handed a gradient sink."""
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def normals_config(pkg, out):
    return pkg.TrainingConfig(iterations=6, densify_from_iter=2, densify_until_iter=2, densify_interval=2,
                              densify_grad_threshold=2e-5, num_random_points=3000, log_interval=1,
                              output_path=str(out), position_lr_init=1.6e-3, position_lr_final=1.6e-5,
                              lambda_normal=0.05)


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    scene_dir, out = Path(sys.argv[4]), sys.argv[5]
    import numpy as np
    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    from scene_util import load_scene
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    ds = load_scene(pkg, scene_dir, dev, split=False)
    tr = pkg.GaussianTrainer(normals_config(pkg, scene_dir / f"out{rank}"), ds)
    tr.setup()
    assert tr._dist is not None
    counts = {"calls": 0, "sinks": 0}
    consistency, rasterize = pkg.normals.normal_consistency, pkg.renderer.rasterize

    def counted(*a, **k):
        counts["calls"] += 1
        return consistency(*a, **k)

    def watched(*a, grad_dest=None, **k):
        counts["sinks"] += grad_dest is not None
        return rasterize(*a, grad_dest=grad_dest, **k)
    pkg.normals.normal_consistency, pkg.renderer.rasterize = counted, watched
    n0 = tr.gaussians.get_num_points()
    tr.train(6)
    torch.cuda.synchronize()
    params = tr.gaussians.parameter_list()
    np.savez(out, **{f"p{i}": p.detach().cpu().numpy() for i, p in enumerate(params)},
             iteration=tr.iteration, n0=n0, n=tr.gaussians.get_num_points(), **counts)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
