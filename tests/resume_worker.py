"""The resumed run of tests/test_resume_gpu.py in a process of its own:
    python tests/resume_worker.py <scene_dir> <images.npz> <out_dir> <state.npz> <threshold> <abs_threshold>
A cold process: no render has run in it, so the rasterizer's module state (the
depth-key window history, the capacity guesses) is empty and its first frames
take the paths a warm process has left behind.  The camera images come from
the parent's file, not from a render.  Loads the checkpoint of iteration K the
parent wrote under <out_dir>, trains to END and saves its state."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    scene_dir, images, out_dir, out = sys.argv[1:5]
    th, th_abs = float(sys.argv[5]), float(sys.argv[6])
    import numpy as np
    import torch
    import __graft_entry__ as ge
    import resume_util as RU
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds = pkg.NeRFSyntheticDataset(scene_dir, device=dev)
    ds.load_cameras()
    imgs = np.load(images)["images"]
    assert len(ds.cameras) == imgs.shape[0]
    for cam, img in zip(ds.cameras, imgs):
        cam._image = torch.from_numpy(img).to(dev)
    ds.split_train_test(0.25)
    cfg = RU.base_config(pkg, out_dir, densify_criterion="screen", prune_screen_radius=20.0, densify_absgrad=True,
                         densify_grad_threshold=th, densify_abs_grad_threshold=th_abs)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.load_checkpoint(RU.K)
    assert tr.iteration == RU.K and tr.gaussians.density_stats.denom.any()
    tr.train(RU.END - RU.K)
    np.savez(out, **RU.state_to_numpy(RU.state(tr)))


if __name__ == "__main__":
    main()
