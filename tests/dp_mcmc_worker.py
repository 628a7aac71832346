"""One rank of the data-parallel MCMC test (tests/test_mcmc_gpu.py):
    python tests/dp_mcmc_worker.py <rank> <world> <port> <scene_dir> <out.npz>
tests/dp_worker.py's run with densify_criterion = "mcmc": four iterations, the
second a refinement that relocates and grows (3000 -> 3100 rows).  The dead
line is put at the initial opacity, sigmoid(-2) = 0.1192, so that after two
Adam steps the Gaussians whose opacity went down are dead and the others are
not."""
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def mcmc_config(pkg, out):
    return pkg.TrainingConfig(iterations=4, densify_from_iter=2, densify_until_iter=2, densify_interval=2,
                              num_random_points=3000, log_interval=1, output_path=str(out),
                              position_lr_init=1.6e-3, position_lr_final=1.6e-5, densify_criterion="mcmc",
                              mcmc_cap_max=3100, mcmc_min_opacity=0.119, mcmc_noise_lr=5e4)


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
    tr = pkg.GaussianTrainer(mcmc_config(pkg, scene_dir / f"out{rank}"), ds)
    tr.setup()
    assert tr._dist is not None
    tr.train(4)
    torch.cuda.synchronize()
    params = tr.gaussians.parameter_list()
    state = tr.optimizer.optimizer.state
    np.savez(out, **{f"p{i}": p.detach().cpu().numpy() for i, p in enumerate(params)},
             **{f"m{i}": (state[p]["exp_avg"] if p in state else torch.zeros(0)).cpu().numpy()
                for i, p in enumerate(params)},
             iteration=tr.iteration, n=tr.gaussians.get_num_points(), relocated=tr.last_densify["relocated"],
             added=tr.last_densify["added"])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
