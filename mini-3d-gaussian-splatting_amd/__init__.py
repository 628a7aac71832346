"""MI355X-native differentiable Gaussian-splatting rasterizer.

Drop-in for the render path of Loveof1ife7/mini-3d-gaussian-splatting:
GaussianRenderer.render() (src/core/renderer.py) and the GaussianModel /
Camera interfaces it reads.  Compute runs only in the hand-written HIP
library libgsplat_mi355x.so (csrc/, C ABI in include/gsplat_mi355x.h).
"""
from .renderer import GaussianRenderer, RenderSettings, camera_params  # noqa: F401
from .gaussian_model import GaussianModel, build_rotation_matrix  # noqa: F401
from .camera import Camera, CameraUtils  # noqa: F401
from .rasterizer import CameraParams, ContributionStats, DensityStats, rasterize  # noqa: F401
from .filter3d import Filter3D, apply_filter_3d  # noqa: F401
from .normals import gaussian_normals, normal_consistency  # noqa: F401
from .bilagrid import BilateralGrids, bilateral_grid_tv, slice_bilateral_grid  # noqa: F401
from .tsdf import TSDFVolume, save_mesh_ply  # noqa: F401
from .knn import knn, mean_knn_dist2  # noqa: F401
from .loss import SSIMLoss, GaussianLoss, photometric_loss  # noqa: F401
from .config import TrainingConfig, ConfigManager  # noqa: F401
from .dataset import CameraDataset, NeRFSyntheticDataset, COLMAPDataset, load_dataset  # noqa: F401
from .trainer import GaussianTrainer  # noqa: F401
from .graph_step import GraphedStep  # noqa: F401
from .pose import CameraPose, se3_exp  # noqa: F401
from .mcmc import mcmc_sample, mcmc_relocate, mcmc_noise, mcmc_regularize  # noqa: F401
from . import _native, synthetic, distributed, optim, loss, dataset, trainer, graph_step, pose, mcmc, filter3d, normals, bilagrid, tsdf  # noqa: F401

__all__ = ["GaussianRenderer", "RenderSettings", "GaussianModel", "Camera", "CameraUtils",
           "CameraParams", "rasterize", "camera_params", "SSIMLoss", "GaussianLoss", "photometric_loss",
           "TrainingConfig", "ConfigManager", "CameraDataset", "NeRFSyntheticDataset", "COLMAPDataset",
           "load_dataset", "GaussianTrainer", "GraphedStep", "CameraPose", "se3_exp", "DensityStats",
           "ContributionStats", "mcmc_sample", "mcmc_relocate", "mcmc_noise", "mcmc_regularize",
           "Filter3D", "apply_filter_3d", "gaussian_normals", "normal_consistency",
           "BilateralGrids", "bilateral_grid_tv", "slice_bilateral_grid", "TSDFVolume", "save_mesh_ply",
           "knn", "mean_knn_dist2"]
