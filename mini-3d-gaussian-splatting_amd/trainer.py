"""GaussianTrainer (reference src/train/trainer.py:12-89, whose methods are
all `pass`).

One iteration: pick a training camera, render it (HIP path), fused L1 +
D-SSIM against its image, backward, [N > 1: one RCCL mean all-reduce of the
Gaussian gradients], learning-rate schedule, FusedAdam step, and density
control every densify_interval iterations inside [densify_from_iter,
densify_until_iter] (optimizer.py:34-141) -- on |dL/dxyz| of the iteration's
view, or with densify_criterion = "screen" on the 3DGS statistics every
render's backward adds to gaussians.density_stats (with densify_absgrad the
absolute gradient among them, which the split test then reads; then also
prune_screen_radius and, every opacity_reset_interval iterations, the 3DGS
opacity reset), or with densify_criterion = "mcmc" the 3DGS-MCMC family
(_mcmc_update: regularisers, relocation and capped growth in place of split /
clone / prune, position noise every iteration).  With filter_3d every render
-- training, validation, contribution pruning -- applies Mip-Splatting's 3D
smoothing filter, recomputed from all training cameras every
filter_3d_interval iterations and whenever the rows change.  With lambda_distortion > 0 the
loss gains, from distortion_from_iter on, lambda_distortion times the mean
depth distortion of the view (render(depth_distortion=True)), and with lambda_normal > 0, after
iteration normal_from_iter, lambda_normal times the mean normal consistency error of the view
(render(normals=True), normals.normal_consistency; no state between steps).  With visible_adam the Adam step
updates only the Gaussians the step's view saw (the render's visibility_filter); every other row
keeps its parameters and both moments bit for bit.  With bilateral_grid every training camera has a
bilateral grid of affine colour transforms (bilagrid.BilateralGrids, indexed by the camera's position in
get_train_cameras()): the step's render is sliced through its camera's grid before the photometric loss, the
loss gains lambda_tv times that grid's total variation, and the grid takes its own Adam step right after the
backward; only that grid and its moments change.  Nothing in a step reads a value
back to the host; losses are logged every log_interval iterations.  A
checkpoint holds what a later step reads -- parameters, Adam moments and step
counts, the 3D filter, the "screen" statistics accumulated since the last
densification, the bilateral grids with their moments and step counts -- so
a resumed run is the uninterrupted one, bit for bit.

Data parallel: with torch.distributed initialised,
rank r renders camera perm[(i * world + r) mod n] at iteration i; every rank
applies the same averaged gradients and the same densification (the
gradients are identical after the all-reduce and the clone jitter is seeded
by the iteration), so the replicas stay bit-identical.  With visible_adam the
step's mask is the union of the ranks' visibility (one MAX all-reduce of the N
mask bytes, issued after the render and before the backward's gradient
ranges): the averaged gradient is non-zero for the rows any rank saw.  With
bilateral_grid each rank divides its grid's gradient by the world size, the
ranks all-gather (image index, gradient), and every rank applies all of them
in rank order -- summed first, in rank order, where two ranks drew the same
image -- in one Adam step (the gathered image indices are the one value such a
step reads back to the host).
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from .config import TrainingConfig
from .dataset import CameraDataset, load_dataset
from . import bilagrid as _bilagrid
from .filter3d import Filter3D
from .gaussian_model import GaussianModel
from .loss import photometric_loss
from . import normals as _normals
from .optim import GaussianOptimizer
from .renderer import GaussianRenderer, RenderSettings
from .tsdf import TSDFVolume, save_mesh_ply


class GaussianTrainer:
    def __init__(self, config: TrainingConfig, dataset: Optional[CameraDataset] = None):
        self.config = config
        self.dataset: Optional[CameraDataset] = dataset
        self.gaussians: Optional[GaussianModel] = None
        self.renderer = GaussianRenderer()
        self.optimizer: Optional[GaussianOptimizer] = None
        self.iteration = 0
        self.scene_extent = 0.0
        self.train_losses: List[float] = []
        self.val_losses: List[float] = []
        self._dist = None
        self._reducer = None
        self._reducer_n = -1
        self._perm: Optional[np.ndarray] = None
        self.last_densify: Optional[dict] = None  # the counts of the latest densification
        self.last_compact: Optional[dict] = None  # the counts of the latest contribution pruning
        self.filter_3d: Optional[Filter3D] = None  # config.filter_3d: the 3D smoothing filter of every render
        # config.bilateral_grid: one grid per training camera, and where each camera stands in that list
        self.bilagrid: Optional[_bilagrid.BilateralGrids] = None
        self._grid_index: Dict[int, int] = {}

    # -- setup (trainer.py:32-44) ------------------------------------------
    def _device(self) -> torch.device:
        c = self.config
        return torch.device(c.device if c.device != "cuda" else f"cuda:{torch.cuda.current_device()}")

    def _setup_run(self) -> None:
        """Everything but the model: dataset, process group, scene extent and
        the camera order -- shared by setup() and load_checkpoint() (a resumed
        run needs them as much as a fresh one)."""
        c = self.config
        c.check()
        if self.dataset is None:
            self.dataset = load_dataset(c.data_path, device=self._device())
        if torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size() > 1:
            self._dist = torch.distributed
        self.scene_extent = self.get_scene_extent()
        n = len(self.dataset.get_train_cameras())
        self._perm = np.random.default_rng(c.seed).permutation(n)

    def setup(self) -> None:
        c = self.config
        c.check()
        dev = self._device()
        self._setup_run()
        g = GaussianModel(c)
        gen = torch.Generator().manual_seed(c.seed)
        if self.dataset.points is not None and len(self.dataset.points):
            g.create_from_points(torch.from_numpy(self.dataset.points).to(dev),
                                 torch.from_numpy(self.dataset.colors).to(dev) if self.dataset.colors is not None else None,
                                 scale_init=c.scale_init)
        else:
            # Blender scenes have no points: uniform in [-1.3, 1.3]^3 (the NeRF-synthetic object box)
            g.create_from_random(c.num_random_points, scene_extent=1.3, device=dev, generator=gen,
                                 scale_init=c.scale_init)
        self.gaussians = g
        self.optimizer = GaussianOptimizer(g, c)
        self.optimizer.setup_optimizer()
        self._update_filter_3d()
        self._setup_bilagrid()

    def _setup_bilagrid(self) -> None:
        """config.bilateral_grid: identity grids, one per training camera."""
        c = self.config
        if not c.bilateral_grid:
            return
        cams = self.dataset.get_train_cameras()
        self.bilagrid = _bilagrid.BilateralGrids(len(cams), self._device(), c.bilateral_grid_shape,
                                                 lr=c.bilateral_grid_lr)
        self._grid_index = {id(cam): i for i, cam in enumerate(cams)}

    def _bilagrid_lr(self, it: int) -> float:
        c = self.config
        ramp = 1.0 if c.bilateral_grid_warmup <= 0 else min(1.0, 0.01 + 0.99 * it / c.bilateral_grid_warmup)
        return c.bilateral_grid_lr * ramp * 0.01 ** (it / max(c.iterations, 1))

    def _bilagrid_step(self, index: int) -> None:
        """The step's grid update, right after the backward.  Data parallel:
        every rank's (image index, gradient / world) is gathered through the
        process group and applied by every rank, in rank order."""
        bg = self.bilagrid
        bg.set_lr(self._bilagrid_lr(self.iteration))
        if self._dist is not None:
            world = self._dist.get_world_size()
            grad = bg.grids[index].grad / world
            dev = grad.device
            idx = torch.tensor([index], dtype=torch.int64, device=dev)
            all_idx = [torch.empty_like(idx) for _ in range(world)]
            all_grad = [torch.empty_like(grad) for _ in range(world)]
            self._dist.all_gather(all_idx, idx)
            self._dist.all_gather(all_grad, grad.contiguous())
            grads: Dict[int, torch.Tensor] = {}
            for i, g in zip(torch.cat(all_idx).tolist(), all_grad):
                grads[i] = grads[i] + g if i in grads else g
            bg.set_grads(grads)
        bg.step()

    def _update_filter_3d(self) -> None:
        """config.filter_3d: the filter of the current rows from all training
        cameras (every rank the full list: the replicas' filters are the same
        bits)."""
        if not self.config.filter_3d:
            return
        xyz = self.gaussians._xyz.detach()
        if self.filter_3d is None or self.filter_3d.n != xyz.shape[0]:
            self.filter_3d = Filter3D(xyz.shape[0], xyz.device, self.config.filter_3d_variance)
        self.filter_3d.update(self.dataset.get_train_cameras(), xyz)

    def _render_extra(self) -> dict:
        return {} if self.filter_3d is None else {"filter_3d": self.filter_3d}

    def get_scene_extent(self) -> float:
        """trainer.py:87-89: camera-centre radius (get_scene_info)."""
        return float(self.dataset.get_scene_info()["radius"])

    def _settings(self, cam) -> RenderSettings:
        c = self.config
        return RenderSettings(image_height=cam._height, image_width=cam._width, bg_color=torch.zeros(3),
                              screen_filter=c.screen_filter, filter_compensate=c.filter_compensate)

    def _camera_for(self, it: int):
        cams = self.dataset.get_train_cameras()
        world = self._dist.get_world_size() if self._dist else 1
        rank = self._dist.get_rank() if self._dist else 0
        return cams[int(self._perm[(it * world + rank) % len(cams)])]

    # -- one step (trainer.py:65-69) ---------------------------------------
    def train_step(self, camera) -> Dict[str, torch.Tensor]:
        g, opt = self.gaussians, self.optimizer
        c = self.config
        if (c.sh_degree > g.active_sh_degree and c.sh_increase_interval > 0
                and self.iteration > 0 and self.iteration % c.sh_increase_interval == 0):
            g.max_sh_degree = max(g.max_sh_degree, c.sh_degree)
            g.oneup_sh_degree()
        if c.filter_3d and self.iteration % c.filter_3d_interval == 0:
            self._update_filter_3d()
        opt.zero_grad()
        grid = None
        if self.bilagrid is not None:
            grid = self._grid_index.get(id(camera))
            if grid is None:
                raise ValueError("bilateral_grid: train_step needs one of the dataset's training cameras (each has "
                                 "its own grid)")
            self.bilagrid.zero_grad()
        if self._dist is not None:
            # the bucket is attached before the render, so that its backward
            # writes the gradients into it and reduces them range by range
            params = g.grad_parameters()
            if self._reducer is None or self._reducer_n != g.get_num_points():
                from .distributed import GradAllReduce
                self._reducer = GradAllReduce(params, self._dist).attach(g)
                self._reducer_n = g.get_num_points()
            self._reducer.params = params
        extra = self._render_extra()
        if c.densify_criterion == "screen":
            extra["density_stats"] = g.density_stats
        # the distortion term: the eager stage path (no replayed step renders it)
        distort = c.lambda_distortion > 0 and self.iteration >= c.distortion_from_iter
        if distort:
            extra["depth_distortion"] = True
            if c.distortion_near_far is not None:
                extra["distortion_near_far"] = c.distortion_near_far
        # the normal consistency term: eager too, next to the distortion; after iteration
        # normal_from_iter (2DGS: lambda_normal if iteration > 7000 else 0)
        normal = c.lambda_normal > 0 and self.iteration > c.normal_from_iter
        if normal:
            extra["normals"] = True
        out = self.renderer.render(camera, g, self._settings(camera), **extra)
        visible = self._visible_mask(out) if c.visible_adam else None
        target = camera._image
        image = out["image"] if grid is None else self.bilagrid.slice(grid, out["image"])
        total, l1, dssim = photometric_loss(image, target, self.config.lambda_dssim)
        if grid is not None and c.lambda_tv > 0:
            total = total + c.lambda_tv * self.bilagrid.tv(grid)
        if distort:
            total = total + c.lambda_distortion * out["distortion"].mean()
        if normal:
            total = total + c.lambda_normal * _normals.normal_consistency(out["normals"], out["depth"], out["alpha"],
                                                                          camera).mean()
        total.backward()
        if grid is not None:
            self._bilagrid_step(grid)
        opt.update_learning_rate(self.iteration)
        if c.densify_criterion == "mcmc":
            self._mcmc_update(visible)
            return {"loss": total.detach(), "l1": l1, "dssim": dssim}
        if self._dist is not None:
            # mean all-reduce, then Adam; pipelined per Gaussian range when the
            # backward handed its rows over in ranges (GS_ALLREDUCE_CHUNKS)
            self._reducer.reduce_and_step(opt.optimizer, visible=visible)
        else:
            opt.step(visible=visible)
        info = opt.densify_and_prune(self.iteration, self.scene_extent, dist=self._dist)
        if info is not None:
            self._reducer = None
            self.last_densify = info
            self._update_filter_3d()
        if (c.opacity_reset_interval > 0 and self.iteration % c.opacity_reset_interval == 0
                and self.iteration <= c.densify_until_iter):
            opt.cap_opacity()
        if c.contribution_prune_iterations and self.iteration in c.contribution_prune_iterations:
            self.last_compact = self.compact()
        return {"loss": total.detach(), "l1": l1, "dssim": dssim}

    def _visible_mask(self, out) -> torch.Tensor:
        """config.visible_adam: the step's row mask, the render's
        visibility_filter as [N] uint8; data parallel the union over the
        ranks (every rank renders another camera, and the averaged gradient
        is non-zero for the rows any of them saw): one MAX all-reduce of the
        mask bytes through the process group, as the density statistics are
        reduced, so every rank steps the same rows."""
        mask = out["visibility_filter"].view(torch.uint8)
        if self._dist is not None:
            mask = mask.clone()
            self._dist.all_reduce(mask, op=self._dist.ReduceOp.MAX)
        return mask

    def _mcmc_update(self, visible: Optional[torch.Tensor] = None) -> None:
        """The rest of a step with densify_criterion "mcmc", after the backward:
        [gradient mean], the regularisers' gradients, Adam, on a refinement
        iteration relocate_and_grow, and the position noise.  Every seed is
        the iteration's, and the regulariser is added after the mean (the
        same bits on every rank), so replicas and resumed runs stay
        bit-identical.  The bucket is dropped only when tensors were replaced:
        once N is at mcmc_cap_max nothing moves again.  visible (config.
        visible_adam): the Adam step updates the marked rows only, so the
        regularisers' gradients on the rows the view did not see are ignored
        with the rest of those rows' gradients (the opacity and scale
        penalties act on a Gaussian in the steps that see it); relocation and
        the position noise are not gated."""
        opt, c = self.optimizer, self.config
        if self._dist is not None:
            self._reducer.all_reduce_mean()
        opt.mcmc_regularize()
        opt.step(visible=visible)
        info = opt.relocate_and_grow(self.iteration)
        if info is not None:
            self.last_densify = info
            if info["added"]:
                self._reducer = None
            self._update_filter_3d()
        opt.mcmc_noise(self.iteration)
        if c.contribution_prune_iterations and self.iteration in c.contribution_prune_iterations:
            self.last_compact = self.compact()

    @torch.no_grad()
    def compact(self, threshold: Optional[float] = None, cameras=None) -> Dict[str, int]:
        """Contribution pruning: render `cameras` (default: the training
        cameras) with the training render settings into
        gaussians.contribution_stats, without gradients, and drop every
        Gaussian whose largest blend weight over all of them is not above
        `threshold` (default: config.contribution_prune_threshold); Adam
        moments follow the kept ones.  Data parallel: each rank renders
        cameras[rank::world], the statistics are all-reduced, and every rank
        takes the same decision.  Returns {"n_before", "n_after"}."""
        g, c = self.gaussians, self.config
        if threshold is None:
            threshold = c.contribution_prune_threshold
        if not float(threshold) >= 0.0:
            raise ValueError(f"the contribution threshold must be >= 0, got {threshold!r}")
        cams = list(self.dataset.get_train_cameras() if cameras is None else cameras)
        if self._dist is not None:
            cams = cams[self._dist.get_rank()::self._dist.get_world_size()]
        stats = g.contribution_stats
        stats.reset()
        for cam in cams:
            self.renderer.render(cam, g, self._settings(cam), contribution_stats=stats, **self._render_extra())
        if self._dist is not None:
            stats.all_reduce(self._dist)
        info = self.optimizer.prune_by_contribution(stats, threshold)
        self._reducer = None  # (the bucket was sized for the old N)
        g.contribution_stats.reset()
        self._update_filter_3d()
        return info

    @torch.no_grad()
    def extract_mesh(self, voxel_size: Optional[float] = None, bounds=None, depth: str = "median", cameras=None,
                     min_weight: float = 1.0, path: Optional[str] = None) -> Dict[str, Optional[torch.Tensor]]:
        """A triangle mesh of the model: render `cameras` (default: the training
        cameras) with the training render settings -- the screen filter and
        the 3D filter -- fuse their depth maps ("median" or "expected",
        tsdf.TSDFVolume.integrate_renders) into a TSDF volume over `bounds` =
        (lo, hi) (default: the bounding box of the model's positions, one host
        read) with `voxel_size` (default: that box's longest edge / 256), and
        extract the surface.  Returns {"vertices", "faces", "colors"}; with
        `path` the mesh is also written there as a binary PLY.  Every rank
        fuses all the cameras (data-parallel fusion is not implemented); no
        training state changes."""
        g = self.gaussians
        if bounds is None:
            xyz = g._xyz.detach().reshape(-1, 3)
            if xyz.shape[0] == 0:
                raise ValueError("extract_mesh needs bounds for a model without Gaussians")
            lo, hi = xyz.min(0).values.tolist(), xyz.max(0).values.tolist()
        else:
            ok = isinstance(bounds, (tuple, list)) and len(bounds) == 2 and \
                all(isinstance(b, (tuple, list)) and len(b) == 3 for b in bounds)
            if not ok:
                raise ValueError(f"bounds must be (lo, hi), each of three numbers, got {bounds!r}")
            lo, hi = bounds
        if voxel_size is None:
            voxel_size = max(float(b) - float(a) for a, b in zip(lo, hi)) / 256.0
        cams = list(self.dataset.get_train_cameras() if cameras is None else cameras)
        vol = TSDFVolume.from_bounds(lo, hi, voxel_size, g._xyz.device)
        vol.integrate_renders(self.renderer, g, cams, self._settings, depth=depth, **self._render_extra())
        mesh = vol.extract_mesh(min_weight)
        if path is not None:
            save_mesh_ply(path, mesh["vertices"], mesh["faces"], mesh["colors"])
        return mesh

    def close(self) -> None:
        """Tear down the data-parallel transport: the native RCCL communicators
        go before the caller destroys the process group (every rank calls this
        at the same point, after its last step).  Also registered at exit by
        distributed._native_comm."""
        if self._dist is not None:
            from .distributed import close_native_comms
            close_native_comms()
        self._reducer = None

    # -- loop (trainer.py:46-63) -------------------------------------------
    def train(self, iterations: Optional[int] = None) -> None:
        if self.gaussians is None:
            self.setup()
        elif self._perm is None:
            self._setup_run()
        n = self.config.iterations if iterations is None else iterations
        for _ in range(n):
            self.iteration += 1
            st = self.train_step(self._camera_for(self.iteration))
            if self.iteration % self.config.log_interval == 0:
                self.train_losses.append(float(st["loss"]))

    @torch.no_grad()
    def validate(self) -> Dict[str, float]:
        """trainer.py:71-75: mean PSNR and loss over the test cameras (train if
        none).  The renders are not corrected by config.bilateral_grid's grids:
        a test camera has none, so the metrics are those of the raw render
        (colour-corrected evaluation is not implemented)."""
        cams = self.dataset.get_test_cameras() or self.dataset.get_train_cameras()
        psnr, loss = [], []
        for cam in cams:
            img = self.renderer.render(cam, self.gaussians, self._settings(cam), **self._render_extra())["image"]
            mse = torch.mean((img - cam._image) ** 2)
            psnr.append(-10.0 * torch.log10(mse.clamp_min(1e-12)))
            loss.append(photometric_loss(img, cam._image, self.config.lambda_dssim)[0])
        out = {"psnr": float(torch.stack(psnr).mean()), "loss": float(torch.stack(loss).mean()),
               "num_gaussians": self.gaussians.get_num_points()}
        self.val_losses.append(out["loss"])
        return out

    # -- checkpoints (trainer.py:77-85): safetensors, no pickle --------------
    def _ckpt_path(self, iteration: int) -> str:
        return os.path.join(self.config.output_path, f"ckpt_{iteration:06d}.safetensors")

    def save_checkpoint(self, iteration: int) -> str:
        from safetensors.torch import save_file
        os.makedirs(self.config.output_path, exist_ok=True)
        names = ["xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"]
        tensors = {}
        for name, p in zip(names, self.gaussians.parameter_list()):
            tensors[name] = p.detach().contiguous()
            st = self.optimizer.optimizer.state.get(p, {})
            if "exp_avg" in st:
                tensors[f"adam.{name}.m"] = st["exp_avg"].contiguous()
                tensors[f"adam.{name}.v"] = st["exp_avg_sq"].contiguous()
                tensors[f"adam.{name}.step"] = torch.tensor([st["step"]], dtype=torch.int64)
        if self.filter_3d is not None:
            for name, v in self.filter_3d.state().items():
                tensors[f"filter_3d.{name}"] = v.contiguous()
        if self._density_stats_in_checkpoint():
            for name, v in self._density_state().items():
                tensors[f"density.{name}"] = v.contiguous()
        if self.bilagrid is not None:
            for name, v in self.bilagrid.state().items():
                tensors[f"bilagrid.{name}"] = v.contiguous()
        meta = {"iteration": str(iteration), "active_sh_degree": str(self.gaussians.active_sh_degree)}
        if self.last_densify is not None:
            meta["last_densify"] = json.dumps(self.last_densify)
        path = self._ckpt_path(iteration)
        save_file({k: v.cpu() for k, v in tensors.items()}, path, metadata=meta)
        return path

    def _density_stats_in_checkpoint(self) -> bool:
        """The "screen" criterion's statistics are state between two
        densifications and go into the checkpoint (keys written only when the
        option is on, as the filter's are).  Not data parallel: each rank's
        statistics are its own partial sums until the densification's
        all-reduce, and one file read by every rank would count them world
        times; such a run resumes with zeros."""
        if self.config.densify_criterion != "screen":
            return False
        return self._dist is None or self._dist.get_world_size() <= 1

    def _density_state(self) -> Dict[str, torch.Tensor]:
        st = self.gaussians.density_stats
        out = {"grad_accum": st.grad_accum, "denom": st.denom, "max_radii": st.max_radii}
        if self.config.densify_absgrad and st.abs_accum is not None:
            out["abs_accum"] = st.abs_accum
        return out

    def _load_density_state(self, t: Dict[str, torch.Tensor]) -> None:
        """Copy the density.* tensors of a checkpoint into the model's fresh
        (zero) statistics; a buffer the file does not hold stays zero (an older
        checkpoint, or one of a run without densify_absgrad), and abs_accum is
        ignored without densify_absgrad."""
        st = self.gaussians.density_stats
        for name, dst in self._density_state().items():
            src = t.get(f"density.{name}")
            if src is None:
                continue
            if tuple(src.shape) != (st.n,) or src.dtype != torch.float32:
                raise ValueError(f"the checkpoint's density.{name} must be fp32 [{st.n}], got {src.dtype} "
                                 f"{tuple(src.shape)}")
            dst.copy_(src)

    def load_checkpoint(self, iteration: int) -> None:
        from safetensors import safe_open
        path = self._ckpt_path(iteration)
        dev = self.gaussians._xyz.device if self.gaussians is not None else self._device()
        with safe_open(path, framework="pt") as f:
            t = {k: f.get_tensor(k) for k in f.keys()}
            meta = f.metadata() or {}
        if self.gaussians is None:
            self.gaussians = GaussianModel(self.config)
        names = ["xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"]
        self.gaussians._set(*[t[n].to(dev) for n in names])
        self.optimizer = GaussianOptimizer(self.gaussians, self.config)
        self.optimizer.setup_optimizer()
        for name, p in zip(names, self.gaussians.parameter_list()):
            if f"adam.{name}.m" in t:
                self.optimizer.optimizer.state[p] = {"step": int(t[f"adam.{name}.step"][0]),
                                                     "exp_avg": t[f"adam.{name}.m"].to(dev),
                                                     "exp_avg_sq": t[f"adam.{name}.v"].to(dev)}
        self.iteration = int(meta.get("iteration", iteration))
        self.gaussians.active_sh_degree = int(meta.get("active_sh_degree", 0))
        self.last_densify = json.loads(meta["last_densify"]) if "last_densify" in meta else None
        self._reducer = None
        if self._perm is None:
            self._setup_run()
        if self._density_stats_in_checkpoint():
            self._load_density_state(t)
        if self.config.filter_3d:
            n = self.gaussians.get_num_points()
            if "filter_3d.values" in t:
                self.filter_3d = Filter3D(n, dev, self.config.filter_3d_variance)
                self.filter_3d.load_state({k: t[f"filter_3d.{k}"] for k in ("max_rate", "values")})
            else:  # (a checkpoint of a run without the filter)
                self.filter_3d = None
                self._update_filter_3d()
        if self.config.bilateral_grid:
            self._setup_bilagrid()  # identity grids: what a checkpoint of a run without the option resumes from
            if "bilagrid.grids" in t:
                self.bilagrid.load_state({k: t[f"bilagrid.{k}"].to(dev) if k != "step" else t[f"bilagrid.{k}"]
                                          for k in ("grids", "m", "v", "step")})


__all__ = ["GaussianTrainer", "TrainingConfig"]
