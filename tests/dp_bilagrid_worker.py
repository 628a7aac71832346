"""One rank of the data-parallel bilateral-grid test (tests/test_bilagrid_gpu.py):
    python tests/dp_bilagrid_worker.py <rank> <world> <port> <scene_dir> <out.npz>
Six iterations with bilateral_grid on, the second a densification.  Twelve
views and two ranks: each step the ranks draw different images, and every rank
must apply both updates.  The worker saves the Gaussians' parameters, every
grid, both moments and the per-image step counts."""
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def bilagrid_config(pkg, out):
    return pkg.TrainingConfig(iterations=6, densify_from_iter=2, densify_until_iter=2, densify_interval=2,
                              densify_grad_threshold=2e-5, num_random_points=3000, log_interval=1,
                              output_path=str(out), position_lr_init=1.6e-3, position_lr_final=1.6e-5,
                              bilateral_grid=True, bilateral_grid_warmup=2, bilateral_grid_lr=1e-2)


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
    tr = pkg.GaussianTrainer(bilagrid_config(pkg, scene_dir / f"out{rank}"), ds)
    tr.setup()
    assert tr._dist is not None and tr.bilagrid is not None
    n0 = tr.gaussians.get_num_points()
    tr.train(6)
    torch.cuda.synchronize()
    params = tr.gaussians.parameter_list()
    st = tr.bilagrid.state()
    np.savez(out, **{f"p{i}": p.detach().cpu().numpy() for i, p in enumerate(params)},
             **{f"bilagrid_{k}": v.cpu().numpy() for k, v in st.items()},
             iteration=tr.iteration, n0=n0, n=tr.gaussians.get_num_points())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
