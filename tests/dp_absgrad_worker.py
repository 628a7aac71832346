"""One rank of the data-parallel absolute-gradient test (tests/test_absgrad_gpu.py):
    python tests/dp_absgrad_worker.py <rank> <world> <port> <scene_dir> <out.npz> <threshold> <abs_threshold>
tests/dp_density_worker.py's run with densify_absgrad: every rank adds its own
views to its replica's statistics, the absolute one among them, and the
densification all-reduces the four.  The reduced abs_accum the densification
read is recorded on its way in."""
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def absgrad_config(pkg, out, threshold, abs_threshold):
    import dataclasses
    from dp_density_worker import screen_config
    return dataclasses.replace(screen_config(pkg, out, threshold), densify_absgrad=True,
                               densify_abs_grad_threshold=abs_threshold)


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    scene_dir, out, threshold, abs_threshold = Path(sys.argv[4]), sys.argv[5], float(sys.argv[6]), float(sys.argv[7])
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
    tr = pkg.GaussianTrainer(absgrad_config(pkg, scene_dir / f"out{rank}", threshold, abs_threshold), ds)
    tr.setup()
    assert tr._dist is not None and tr.gaussians.density_stats.abs_accum is not None
    seen = {}
    densify = tr.gaussians.densify_and_prune

    def recording(*args, **kw):  # (the controller has all-reduced the statistics by now)
        st = kw["stats"]
        seen.update(abs_accum=st.abs_accum.cpu().numpy(), accum=st.grad_accum.cpu().numpy(),
                    denom=st.denom.cpu().numpy(), abs_threshold=kw["abs_grad_threshold"])
        return densify(*args, **kw)

    tr.gaussians.densify_and_prune = recording
    tr.train(3)
    torch.cuda.synchronize()
    st = tr.gaussians.density_stats
    np.savez(out, **{f"p{i}": p.detach().cpu().numpy() for i, p in enumerate(tr.gaussians.parameter_list())},
             iteration=tr.iteration, n=tr.gaussians.get_num_points(), split=tr.last_densify["split"],
             cloned=tr.last_densify["cloned"], reduced_abs=seen["abs_accum"], reduced_accum=seen["accum"],
             reduced_denom=seen["denom"], abs_threshold=seen["abs_threshold"], abs_after=st.abs_accum.cpu().numpy(),
             denom_after=st.denom.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
