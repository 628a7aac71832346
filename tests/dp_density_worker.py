"""One rank of the data-parallel density-statistics test
(tests/test_density_training_gpu.py):
    python tests/dp_density_worker.py <rank> <world> <port> <scene_dir> <out.npz> <threshold>
tests/dp_worker.py's run with the "screen" criterion: every rank adds its own
views to its replica's statistics, and the densification all-reduces them."""
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def screen_config(pkg, out, threshold):
    import dataclasses
    from scene_util import dp_config
    return dataclasses.replace(dp_config(pkg, out), densify_criterion="screen", densify_grad_threshold=threshold,
                               prune_screen_radius=20.0)


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    scene_dir, out, threshold = Path(sys.argv[4]), sys.argv[5], float(sys.argv[6])
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
    tr = pkg.GaussianTrainer(screen_config(pkg, scene_dir / f"out{rank}", threshold), ds)
    tr.setup()
    assert tr._dist is not None
    tr.train(3)
    torch.cuda.synchronize()
    st = tr.gaussians.density_stats
    np.savez(out, **{f"p{i}": p.detach().cpu().numpy() for i, p in enumerate(tr.gaussians.parameter_list())},
             iteration=tr.iteration, n=tr.gaussians.get_num_points(), split=tr.last_densify["split"],
             cloned=tr.last_densify["cloned"], denom=st.denom.cpu().numpy(), accum=st.grad_accum.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
