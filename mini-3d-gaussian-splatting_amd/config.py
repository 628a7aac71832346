"""TrainingConfig (reference config/config.py:33-67), flat, no import-time
side effects (the reference prints on import, :97-98).  Fields and defaults
are the reference's; the few the trainer adds are marked."""
from __future__ import annotations

from dataclasses import asdict, dataclass, fields
from pathlib import Path
from typing import Optional

try:  # optional, as in the reference (config.py:1-8)
    import yaml
except ImportError:  # pragma: no cover
    yaml = None


@dataclass
class TrainingConfig:
    data_path: str = "data/scene"
    output_path: str = "output"

    iterations: int = 30000
    learning_rate: float = 0.0025
    batch_size: int = 1

    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_delay_mult: float = 0.01
    position_lr_max_steps: int = 30000

    feature_lr: float = 0.0025
    opacity_lr: float = 0.05
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001

    densify_from_iter: int = 500
    densify_until_iter: int = 15000
    densify_grad_threshold: float = 0.0002
    densify_interval: int = 100

    image_height: int = 800
    image_width: int = 800

    device: str = "cuda"

    # added by this trainer (not in the reference config)
    lambda_dssim: float = 0.2          # loss.py:42 default
    num_random_points: int = 100_000   # random init when the dataset has no points
    min_opacity: float = 0.01          # optimizer.py:64
    test_every: int = 8                # every k-th camera held out when a dataset has no test split
    log_interval: int = 100
    seed: int = 0
    sh_degree: int = 0                 # max SH degree of the colour (0 = the reference's DC-only render)
    sh_increase_interval: int = 1000   # active SH degree +1 every this many iterations, up to sh_degree
    # after a densification the reference builds a fresh Adam (optimizer.py:133-137: moments and step
    # counts dropped); False keeps the kept Gaussians' moments (new ones start at zero)
    reset_adam_on_densify: bool = False
    # what densification reads: "xyz_grad", |dL/dxyz| of the iteration's one view, or "screen", the
    # 3DGS criterion: the NDC-unit gradient norm at the projected centre, averaged over the views that
    # saw the Gaussian since the last densification (the quantity densify_grad_threshold is the 3DGS
    # value of); or "mcmc", the 3DGS-MCMC family (the mcmc_* fields below)
    densify_criterion: str = "xyz_grad"
    # "screen" with AbsGS's rule (gsplat's absgrad): the split test reads the mean *absolute* screen-space
    # gradient -- the per-pixel |dL/dmu| summed, which a large Gaussian's pixels cannot cancel -- against
    # densify_abs_grad_threshold (0.0008: gsplat's published absgrad value); the clone test keeps the
    # signed mean against densify_grad_threshold.  The renders then take the stage path (the same image
    # and gradients) with the absolute-gradient blend backward
    densify_absgrad: bool = False
    densify_abs_grad_threshold: float = 0.0008
    prune_screen_radius: float = 0.0   # "screen": also prune Gaussians whose largest screen radius (px) exceeded it; 0 = off
    # cap opacities at 0.01 every this many iterations while densifying (0 = never); a Gaussian the
    # training has not raised above min_opacity again by the next densification is pruned there
    opacity_reset_interval: int = 0
    # screen-space low-pass filter of every render, training and evaluation (RenderSettings.screen_filter:
    # the variance in px^2, 0 = off, 0.3 = 3DGS's dilation, 0.1 = Mip-Splatting's), and whether the
    # opacities are scaled so that a filtered splat keeps its energy
    screen_filter: float = 0.0
    filter_compensate: bool = True
    # Mip-Splatting's 3D smoothing filter in every render, training and evaluation (filter3d.Filter3D;
    # with screen_filter = 0.1 the pair is Mip-Splatting's anti-aliased mode): its variance in px^2 at
    # each Gaussian's highest training sampling rate, and how often (iterations) the rates are recomputed
    # from all training cameras -- besides every time the rows change (densification, relocation, pruning)
    filter_3d: bool = False
    filter_3d_variance: float = 0.2
    filter_3d_interval: int = 100
    # contribution pruning (GaussianTrainer.compact): at these iterations, after the optimizer step,
    # every training camera is rendered and the Gaussians whose largest blend weight over all of them
    # is not above the threshold are dropped (0.01: RadSplat's default); () = never
    contribution_prune_iterations: tuple = ()
    contribution_prune_threshold: float = 0.01
    # densify_criterion "mcmc" (3DGS-MCMC, on the densify_from_iter / _until_iter / _interval schedule):
    # nothing is pruned; at a refinement the Gaussians with opacity <= mcmc_min_opacity are relocated onto
    # live ones and N grows by mcmc_grow_factor up to mcmc_cap_max, after which no tensor is reallocated;
    # every iteration the positions get opacity-gated noise of mcmc_noise_lr * the position learning rate,
    # and the loss gains mcmc_opacity_reg * mean(opacity) + mcmc_scale_reg * mean(scale)
    mcmc_cap_max: int = 1_000_000
    mcmc_min_opacity: float = 0.005
    mcmc_noise_lr: float = 5e5
    mcmc_opacity_reg: float = 0.01
    mcmc_scale_reg: float = 0.01
    mcmc_grow_factor: float = 1.05
    # depth distortion (Mip-NeRF 360 / 2DGS): from distortion_from_iter on the loss gains
    # lambda_distortion * mean over the pixels of sum_ij c_i c_j |m_i - m_j| (render(depth_distortion=True));
    # m is the camera-space depth, or with distortion_near_far = (near, far) 2DGS's inverse depth.
    # 0 = off: the step's launches are the ones they were
    lambda_distortion: float = 0.0
    distortion_from_iter: int = 0
    distortion_near_far: Optional[tuple] = None
    # normal consistency (2DGS, also gsplat and RaDe-GS): once normal_from_iter iterations are done (the
    # steps numbered above it, 2DGS's `iteration > 7000`) the step renders with normals=True and the loss
    # gains lambda_normal * mean over the pixels of 1 - alpha (N_r . n_d), N_r the rendered normals and n_d
    # the depth map's (normals.normal_consistency).  2DGS uses 0.05 from iteration 7000.  0 = off: the
    # step's launches are the ones they were
    lambda_normal: float = 0.0
    normal_from_iter: int = 0
    # visibility-gated Adam (gsplat's visible_adam, the sparse Adam of Taming 3DGS): a step updates only the
    # Gaussians its view saw (the render's visibility_filter; data parallel: the union over the ranks' views);
    # every other row keeps its parameters and both Adam moments bit for bit instead of drifting along a
    # stale first moment.  Step counts stay per tensor.  Not for the replayed step (GraphedStep)
    visible_adam: bool = False
    # bilateral-grid appearance compensation (Wang et al. 2024; gsplat's use_bilateral_grid; bilagrid.py): every
    # training image gets a learnable (Gw, Gh, L) grid of affine colour transforms -- bilateral_grid_shape --
    # that is sliced per pixel and applied to the training render before the photometric loss, absorbing the
    # frame's exposure and white balance; the loss gains lambda_tv * the grid's total variation.  The grids have
    # their own Adam: bilateral_grid_lr * min(1, 0.01 + 0.99 it / bilateral_grid_warmup) * 0.01^(it / iterations).
    # Evaluation renders stay uncorrected.  False: no new launch, the step's bits are the ones they were
    bilateral_grid: bool = False
    bilateral_grid_shape: tuple = (16, 16, 8)
    bilateral_grid_lr: float = 2e-3
    bilateral_grid_warmup: int = 1000
    lambda_tv: float = 10.0
    # the start-up scales (GaussianModel.create_from_points / create_from_random): "extent", one scale for
    # every Gaussian (1 % / 2 % of the cloud's extent), or "knn", 3DGS's rule -- each Gaussian the size of its
    # neighbourhood, the root of the mean squared distance to its three nearest points (knn.mean_knn_dist2)
    scale_init: str = "extent"

    def __post_init__(self):
        # (a YAML file holds the iterations as a list)
        if isinstance(self.contribution_prune_iterations, list):
            self.contribution_prune_iterations = tuple(self.contribution_prune_iterations)
        if isinstance(self.distortion_near_far, list):
            self.distortion_near_far = tuple(self.distortion_near_far)
        if isinstance(self.bilateral_grid_shape, list):
            self.bilateral_grid_shape = tuple(self.bilateral_grid_shape)

    def check(self) -> None:
        """Values no run can use (the trainer asks at setup)."""
        if self.densify_criterion not in DENSIFY_CRITERIA:
            raise ValueError(f"densify_criterion must be one of {DENSIFY_CRITERIA}, got {self.densify_criterion!r}")
        if self.densify_absgrad and self.densify_criterion != "screen":
            raise ValueError("densify_absgrad needs densify_criterion 'screen' (the absolute gradient is a screen-space "
                             f"statistic), got {self.densify_criterion!r}")
        t = float(self.densify_abs_grad_threshold)
        if not (t >= 0.0 and t != float("inf")):
            raise ValueError(f"densify_abs_grad_threshold must be finite and >= 0, got {self.densify_abs_grad_threshold!r}")
        s = float(self.screen_filter)
        if not (s >= 0.0 and s != float("inf")):
            raise ValueError(f"screen_filter must be a finite variance >= 0 (px^2), got {self.screen_filter!r}")
        v = float(self.filter_3d_variance)
        if not (v >= 0.0 and v != float("inf")):
            raise ValueError(f"filter_3d_variance must be a finite variance >= 0 (px^2), got {self.filter_3d_variance!r}")
        it = self.filter_3d_interval
        if isinstance(it, bool) or not isinstance(it, int) or it < 1:
            raise ValueError(f"filter_3d_interval must be an integer >= 1, got {it!r}")
        if not float(self.contribution_prune_threshold) >= 0.0:
            raise ValueError(f"contribution_prune_threshold must be >= 0, got {self.contribution_prune_threshold!r}")
        its = self.contribution_prune_iterations
        if isinstance(its, (str, bytes)) or not all(isinstance(i, int) and not isinstance(i, bool) and i > 0
                                                    for i in its):
            raise ValueError(f"contribution_prune_iterations must hold positive iteration numbers, got {its!r}")
        lam = float(self.lambda_distortion)
        if not (lam >= 0.0 and lam != float("inf")):
            raise ValueError(f"lambda_distortion must be finite and >= 0, got {self.lambda_distortion!r}")
        it = self.distortion_from_iter
        if isinstance(it, bool) or not isinstance(it, int) or it < 0:
            raise ValueError(f"distortion_from_iter must be an integer >= 0, got {it!r}")
        lam = float(self.lambda_normal)
        if not (lam >= 0.0 and lam != float("inf")):
            raise ValueError(f"lambda_normal must be finite and >= 0, got {self.lambda_normal!r}")
        it = self.normal_from_iter
        if isinstance(it, bool) or not isinstance(it, int) or it < 0:
            raise ValueError(f"normal_from_iter must be an integer >= 0, got {it!r}")
        if not isinstance(self.bilateral_grid, bool):
            raise ValueError(f"bilateral_grid must be a bool, got {self.bilateral_grid!r}")
        gs = self.bilateral_grid_shape
        if not (isinstance(gs, tuple) and len(gs) == 3 and all(isinstance(v, int) and not isinstance(v, bool) for v in gs)
                and 2 <= gs[0] <= 64 and 2 <= gs[1] <= 64 and 2 <= gs[2] <= 16):
            raise ValueError("bilateral_grid_shape must be (Gw, Gh, L) integers with 2 <= Gw, Gh <= 64 and 2 <= L <= 16, "
                             f"got {gs!r}")
        lr = float(self.bilateral_grid_lr)
        if not (lr > 0.0 and lr != float("inf")):
            raise ValueError(f"bilateral_grid_lr must be finite and > 0, got {self.bilateral_grid_lr!r}")
        it = self.bilateral_grid_warmup
        if isinstance(it, bool) or not isinstance(it, int) or it < 0:
            raise ValueError(f"bilateral_grid_warmup must be an integer >= 0, got {it!r}")
        lam = float(self.lambda_tv)
        if not (lam >= 0.0 and lam != float("inf")):
            raise ValueError(f"lambda_tv must be finite and >= 0, got {self.lambda_tv!r}")
        if self.scale_init not in SCALE_INITS:
            raise ValueError(f"scale_init must be one of {SCALE_INITS}, got {self.scale_init!r}")
        nf = self.distortion_near_far
        if nf is not None:
            ok = isinstance(nf, (tuple, list)) and len(nf) == 2 and all(isinstance(v, (int, float)) for v in nf)
            if not (ok and 0.0 < float(nf[0]) < float(nf[1]) < float("inf")):
                raise ValueError(f"distortion_near_far must be None or finite (near, far) with 0 < near < far, got {nf!r}")
        if self.densify_criterion == "mcmc":
            if isinstance(self.mcmc_cap_max, bool) or not isinstance(self.mcmc_cap_max, int) or self.mcmc_cap_max < 1:
                raise ValueError(f"mcmc_cap_max must be an integer >= 1, got {self.mcmc_cap_max!r}")
            for name in ("mcmc_noise_lr", "mcmc_opacity_reg", "mcmc_scale_reg"):
                v = float(getattr(self, name))
                if not (v >= 0.0 and v != float("inf")):
                    raise ValueError(f"{name} must be finite and >= 0, got {getattr(self, name)!r}")
            if not (float(self.mcmc_grow_factor) >= 1.0 and float(self.mcmc_grow_factor) != float("inf")):
                raise ValueError(f"mcmc_grow_factor must be finite and >= 1, got {self.mcmc_grow_factor!r}")
            if not 0.0 < float(self.mcmc_min_opacity) < 1.0:
                raise ValueError(f"mcmc_min_opacity must lie in (0, 1), got {self.mcmc_min_opacity!r}")
            if self.opacity_reset_interval > 0 or self.prune_screen_radius > 0:
                raise ValueError("opacity_reset_interval and prune_screen_radius belong to the split / clone / prune "
                                 "criteria, not to densify_criterion 'mcmc'")


DENSIFY_CRITERIA = ("xyz_grad", "screen", "mcmc")
SCALE_INITS = ("extent", "knn")  # scale_init, here and in GaussianModel.create_from_*


def _need_yaml():
    if yaml is None:
        raise ImportError("PyYAML is not installed")


class ConfigManager:
    """config.py:69-95: YAML load / save of the flat config (unknown keys are
    rejected instead of silently ignored).  The reference's names
    (load_from_yaml, save_to_yaml, get_default_config) and short aliases."""

    @staticmethod
    def load_from_yaml(config_path: str) -> TrainingConfig:
        _need_yaml()
        with open(config_path, encoding="utf-8") as f:
            data = yaml.safe_load(f) or {}
        names = {f.name for f in fields(TrainingConfig)}
        unknown = sorted(set(data) - names)
        if unknown:
            raise KeyError(f"unknown config keys: {unknown}")
        return TrainingConfig(**data)

    @staticmethod
    def save_to_yaml(config: TrainingConfig, config_path: str) -> None:
        _need_yaml()
        Path(config_path).parent.mkdir(parents=True, exist_ok=True)
        with open(config_path, "w", encoding="utf-8") as f:
            yaml.safe_dump(asdict(config), f, sort_keys=False, allow_unicode=True)

    @staticmethod
    def get_default_config() -> TrainingConfig:
        return TrainingConfig()

    load = load_from_yaml
    save = save_to_yaml
