"""One rank of the data-parallel visibility-gated Adam test
(tests/test_visible_adam_gpu.py):
    python tests/dp_visible_adam_worker.py <rank> <world> <port> <scene_dir> <out.npz>
tests/dp_worker.py's run with visible_adam and no densification, on a scene
widened so that every camera misses part of it.  Per step it records this
rank's own visibility, which rows changed in any parameter or moment, and
which rows the averaged gradient reached."""
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STEPS = 3


def visible_config(pkg, out):
    import dataclasses
    from scene_util import dp_config
    return dataclasses.replace(dp_config(pkg, out), densify_from_iter=10_000, densify_until_iter=10_000,
                               visible_adam=True)


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
    tr = pkg.GaussianTrainer(visible_config(pkg, scene_dir / f"out{rank}"), ds)
    tr.setup()
    assert tr._dist is not None
    g = tr.gaussians
    with torch.no_grad():
        g._xyz.mul_(1.5)  # (the same on every rank: a cube of +-1.95 around cameras that see +-1.4 of it)
    rec = {}

    def state():
        opt = tr.optimizer.optimizer
        ts = [p.detach().clone() for p in g.grad_parameters()]
        for p in g.grad_parameters():
            st = opt.state.get(p, {})
            ts += [st[k].clone() if k in st else torch.zeros_like(p) for k in ("exp_avg", "exp_avg_sq")]
        return ts

    for step in range(STEPS):
        tr.iteration += 1
        cam = tr._camera_for(tr.iteration)
        with torch.no_grad():
            vis = tr.renderer.render(cam, g, tr._settings(cam))["visibility_filter"].clone()
        before = state()
        tr.train_step(cam)
        after = state()
        n = vis.shape[0]
        changed = torch.zeros(n, dtype=torch.bool, device=dev)
        for a, b in zip(before, after):
            changed |= (a.view(n, -1).view(torch.int32) != b.view(n, -1).view(torch.int32)).any(1)
        reached = torch.zeros(n, dtype=torch.bool, device=dev)
        for p in g.grad_parameters():
            reached |= (p.grad.view(n, -1) != 0).any(1)
        rec[f"vis{step}"] = vis.cpu().numpy()
        rec[f"changed{step}"] = changed.cpu().numpy()
        rec[f"reached{step}"] = reached.cpu().numpy()
    torch.cuda.synchronize()
    opt = tr.optimizer.optimizer
    for i, p in enumerate(g.parameter_list()):
        rec[f"p{i}"] = p.detach().cpu().numpy()
        st = opt.state.get(p, {})
        if "exp_avg" in st:
            rec[f"m{i}"], rec[f"v{i}"], rec[f"t{i}"] = st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), st["step"]
    np.savez(out, iteration=tr.iteration, ranges=tr._reducer.ranges_reduced, **rec)
    dist.barrier()
    tr.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
