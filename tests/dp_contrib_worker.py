"""One rank of the data-parallel contribution-pruning test
(tests/test_contrib_gpu.py):
    python tests/dp_contrib_worker.py <rank> <world> <port> <scene_dir> <out.npz> <threshold>
The trainer's compact(): this rank renders cameras[rank::world] into its
replica's statistics, they are all-reduced, and every rank prunes alike."""
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    scene_dir, out, threshold = Path(sys.argv[4]), sys.argv[5], float(sys.argv[6])
    import numpy as np
    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    from scene_util import load_scene
    from contrib_util import trainer_config
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    ds = load_scene(pkg, scene_dir, dev, 64, split=False)
    tr = pkg.GaussianTrainer(trainer_config(pkg, scene_dir / f"out{rank}"), ds)
    tr.setup()
    assert tr._dist is not None
    xyz0 = tr.gaussians._xyz.detach().cpu().numpy().copy()
    rendered = []
    inner = tr.renderer.render

    def render(cam, *a, **kw):
        rendered.append(cam)
        return inner(cam, *a, **kw)

    tr.renderer.render = render
    info = tr.compact(threshold)
    torch.cuda.synchronize()
    np.savez(out, xyz0=xyz0, xyz=tr.gaussians._xyz.detach().cpu().numpy(), n_before=info["n_before"],
             n_after=info["n_after"], cameras=len(rendered))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
