"""Drop-in GaussianRenderer / RenderSettings (reference: src/core/renderer.py).

Same class names, constructor arguments, render() signature and output
dict as the reference (renderer.py:13-114).  The four stages run as HIP
kernels (see rasterizer.py); the duck-typed inputs are read exactly where
the reference reads them:

  camera._width/_height/_FoVx/_FoVy, camera.world_view_transform()  (:140-150)
  gaussians.get_xyz (:135), get_covariance (:166), get_features or
  _features_dc (:88-92), get_opacity (:94)

Differences a caller can observe (all documented in DESIGN.md):
  * `world_view_transform` may be a method (what the reference calls) or a
    tensor/property (what the reference's own Camera defines).
  * When `gaussians` is this package's GaussianModel, covariance is built
    inside the projection kernel from the raw `_scaling`/`_rotation` (same
    math as GaussianModel.compute_3d_covariance) and colours are read from
    `_features_dc` instead of materialising get_features; gradients reach the
    same leaves, except `_features_rest`, whose gradient is identically zero
    in the reference and is left as None here.
  * `radii` and `visibility_filter` carry no gradient.
  * A `world_view_transform` that requires grad receives its gradient, as in
    the reference (pose refinement: pose.CameraPose); with torch.no_grad or a
    plain tensor nothing about the render changes.
  * `settings.scale_modifier` and `settings.debug` are ignored, as in the
    reference.
  * `render(..., features=F)` (not in the reference) also returns
    "features": F [N, C] composited with the colour pass's own weights.
  * `render(..., density_stats=S)` (not in the reference) adds the view to the
    density-control statistics S at the end of its backward (DensityStats).
  * `render(..., depth_distortion=True)` (not in the reference) also returns
    "distortion", "median_depth" and "median_gaussian".
  * `settings.screen_filter` (not in the reference; default 0 = off) low-pass
    filters every splat in screen space, cov2d + s I, and with
    `settings.filter_compensate` keeps its energy (anti-aliasing).
  * `render(..., filter_3d=Filter3D)` (not in the reference) convolves every
    Gaussian with Mip-Splatting's 3D smoothing filter before the projection
    (filter3d.py); with `settings.screen_filter` the pair is its anti-aliased
    mode.
  * `render(..., normals=True)` (not in the reference) also returns "normals",
    the camera-space normal of every Gaussian (normals.gaussian_normals)
    composited like a feature: the rendered half of the normal consistency
    term (normals.normal_consistency).
  * `settings.sh_degree` (default: the model's `active_sh_degree`, else 0)
    switches on view-dependent SH colour; at 0 -- the default for the
    reference's own model and stubs -- colours are the reference's
    sigmoid(DC).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _native as N
from .filter3d import Filter3D, apply_filter_3d, check_filter_3d_variance
from . import normals as _normals
from .rasterizer import (CameraParams, ContributionStats, DensityStats, check_distortion_near_far,
                         check_screen_filter, rasterize)


@dataclass
class RenderSettings:
    """renderer.py:13-20"""
    image_height: int
    image_width: int
    bg_color: torch.Tensor
    scale_modifier: float = 1.0
    debug: bool = False
    # View-dependent colour (not in the reference, which renders
    # DC only): None takes `gaussians.active_sh_degree` when the model has one,
    # else 0 (the reference's behaviour).  1..3 evaluates SH of that degree from
    # get_features[:, 1:, :] (include/gsplat_mi355x.h, gs_gaussians).
    sh_degree: Optional[int] = None
    # Screen-space low-pass filter (anti-aliasing; not in the reference): the
    # variance s in px^2 added to every projected covariance, cov2d + s I, before
    # the conic, the radius and the culling (include/gsplat_mi355x.h,
    # gs_screen_filter).  0 is off -- the reference's projection, bit for bit;
    # 0.3 is 3DGS's dilation, 0.1 Mip-Splatting's.  A negative, NaN or infinite
    # value is a ValueError.
    screen_filter: float = 0.0
    # with the filter: scale each opacity by sqrt(det cov2d / det(cov2d + s I)), so
    # that a splat keeps its energy (Mip-Splatting / gsplat "antialiased"); False
    # is the plain 3DGS dilation.  Read only when screen_filter > 0.
    filter_compensate: bool = True

    def __post_init__(self):
        check_screen_filter(self.screen_filter)


def _world_view(camera) -> torch.Tensor:
    wv = camera.world_view_transform
    if callable(wv):
        wv = wv()
    return torch.as_tensor(wv)


def effective_tile(tile_size: int, width: int, height: int) -> int:
    """The tile edge the kernels use for GaussianRenderer(tile_size) on a
    width x height image: tile_size, or max(width, height) when it is larger
    -- the same image and gradients, since every tile of at least max(W, H)
    holds the whole image (renderer.py:263-298: one tile, every Gaussian whose
    rectangle meets the image, in depth order).  Edges up to GS_MAX_TILE."""
    t = int(tile_size)
    if t > max(int(width), int(height)):
        t = max(int(width), int(height), 1)
    if t > N.GS_MAX_TILE:
        raise ValueError(f"tile_size {tile_size} on a {width}x{height} image: a tile edge of {t} px (the "
                         f"smaller of tile_size and max(W, H)) is above GS_MAX_TILE = {N.GS_MAX_TILE}, "
                         f"which is not supported")
    return t


def _host_f32(t, count: int) -> list:
    """The values of `t` (a tensor or sequence of `count` numbers) rounded to
    fp32, as Python floats, row-major (a CPU fp32 tensor is read as is)."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cpu" or t.dtype != torch.float32:
        t = torch.as_tensor(t).detach().to("cpu", torch.float32)
    if t.numel() != count:
        raise ValueError(f"expected {count} values, got a tensor of shape {tuple(t.shape)}")
    d = t.dim()
    if d == 1:
        return t.tolist()
    if d == 2:  # (a 4x4 view matrix: tolist and flatten, 1 us instead of reshape + tolist's 3)
        return [v for row in t.tolist() for v in row]
    return t.reshape(count).tolist()


def camera_params(camera, settings: RenderSettings, radius_min=0.01, radius_max=50.0, tile_size=16,
                  world_view=None) -> CameraParams:
    """Host scalars of renderer.py:140-152 (python double -> fp32 in the ABI).
    world_view: the camera's world_view_transform when the caller has read it
    already."""
    W, H = camera._width, camera._height
    fx = 0.5 * W / math.tan(camera._FoVx * 0.5)
    fy = 0.5 * H / math.tan(camera._FoVy * 0.5)
    view = tuple(_host_f32(_world_view(camera) if world_view is None else world_view, 16)[:12])
    bg = tuple(_host_f32(settings.bg_color, 3))
    tile = effective_tile(tile_size, settings.image_width, settings.image_height)
    return CameraParams(int(settings.image_width), int(settings.image_height), fx, fy, W * 0.5, H * 0.5,
                        view, bg, float(radius_min), float(radius_max), tile,
                        float(getattr(settings, "screen_filter", 0.0)), bool(getattr(settings, "filter_compensate", True)))


def _check_filter_3d(filter_3d, gaussians, fused) -> None:
    """ValueError for a filter_3d this render cannot apply, before any launch."""
    if not isinstance(filter_3d, Filter3D):
        raise ValueError(f"filter_3d must be a Filter3D, got {type(filter_3d).__name__}")
    if not fused:
        raise ValueError("filter_3d needs this package's GaussianModel (scaling and rotation): a model rendered "
                         "through get_covariance cannot take the 3D filter")
    check_filter_3d_variance(filter_3d.variance)
    s, v = gaussians._scaling, filter_3d.values
    if v.dim() != 1 or v.shape[0] != s.shape[0] or filter_3d.n != s.shape[0]:
        raise ValueError(f"filter_3d holds {tuple(v.shape)} values for a model of {s.shape[0]} Gaussians")
    if v.device != s.device:
        raise ValueError(f"filter_3d is on {v.device}, the model on {s.device}")
    if v.dtype != torch.float32 or s.dtype != torch.float32 or gaussians._opacity.dtype != torch.float32:
        raise ValueError(f"filter_3d needs fp32 values, scaling and opacity, got {v.dtype}, {s.dtype}, "
                         f"{gaussians._opacity.dtype}")


def _check_normals(gaussians, fused, features) -> None:
    """ValueError for a render(normals=True) that cannot be done, before any launch."""
    if not fused:
        raise ValueError("normals=True needs this package's GaussianModel (scaling and rotation): a model rendered "
                         "through get_covariance has no axes to take a normal from")
    if features is not None:
        if not isinstance(features, torch.Tensor):
            raise TypeError(f"features must be a tensor, got {type(features).__name__}")
        if features.dim() != 2:
            raise ValueError(f"features must be [N, C], got {tuple(features.shape)}")
        n, c = int(gaussians._rotation.shape[0]), int(features.shape[1])
        if c + 3 > N.GS_MAX_FEATURE_CHANNELS:
            raise ValueError(f"normals=True takes three feature channels: features may have at most "
                             f"{N.GS_MAX_FEATURE_CHANNELS - 3} (GS_MAX_FEATURE_CHANNELS - 3), got {c}")
        if features.shape[0] != n or not features.is_floating_point() or features.device != gaussians._rotation.device:
            raise ValueError(f"features must be floating-point [{n}, C] on {gaussians._rotation.device}, got "
                             f"{features.dtype} {tuple(features.shape)} on {features.device}")


class GaussianRenderer:
    """renderer.py:22-114"""

    def __init__(self, tile_size=16, radius_min=0.01, radius_max=50.0):
        # any tile edge the reference's binning can use (renderer.py:261-298):
        # every int >= 1 (0 divides by zero in the reference); edges above
        # the image render as one tile of max(W, H) (effective_tile); radii as
        # the reference clamps them (:190)
        if int(tile_size) != tile_size or tile_size < 1:
            raise ValueError(f"tile_size must be an integer >= 1, got {tile_size!r}")
        if not (math.isfinite(radius_max) and 0 <= radius_min <= radius_max):
            raise ValueError(f"need 0 <= radius_min <= radius_max < inf, got {radius_min!r}, {radius_max!r}")
        self.tile_size = int(tile_size)
        self.radius_min = radius_min
        self.radius_max = radius_max
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

    def render(self, camera, gaussians, settings: RenderSettings,
               features: Optional[torch.Tensor] = None,
               density_stats: Optional[DensityStats] = None,
               contribution_stats: Optional[ContributionStats] = None,
               dominant: bool = False, depth_distortion: bool = False,
               distortion_near_far=None, filter_3d: Optional[Filter3D] = None,
               normals: bool = False) -> Dict[str, torch.Tensor]:
        """normals: the result also holds "normals", fp32 [3, H, W]: each pixel's
        sum_i c_i n_i with the colour pass's own weights, n_i the camera-space
        normal of Gaussian i (normals.gaussian_normals on the model's raw
        _rotation, _scaling and _xyz: its shortest axis, facing the camera).
        Not normalised: its length is about alpha.  The three channels ride the
        feature pass, behind `features` when both are given (C + 3 <=
        GS_MAX_FEATURE_CHANNELS), and the frame takes the stage path: the seven
        standard outputs and their gradients are the same bits.  With filter_3d
        the raw scaling still decides the axis (the filter's map is monotone in
        every axis, so the shortest stays the shortest).  The rotation's
        gradient arrives in two pieces, the render's and the normals', so a
        data-parallel bucket is not written by the kernels, as with filter_3d.
        The normals read the view as host scalars: a world_view_transform that
        requires grad gets its gradient from every other output and none
        through the normals.  Only this package's GaussianModel: a duck-typed
        model is a ValueError before anything is launched.  False is the render
        without the argument, launch for launch.
        filter_3d: optional Filter3D of the model's size on its device
        (Mip-Splatting's 3D smoothing filter, filter3d.py).  The model's raw
        _scaling and _opacity then pass through apply_filter_3d and the
        projection reads the results: scaling' and the probability opacity'.
        Gradients reach the leaves through autograd; a data-parallel bucket is
        not written by the kernels then (the projection's d_scaling is
        scaling''s, not the leaf's) and takes the .grad tensors at its
        all-reduce.  Only this package's GaussianModel: a duck-typed model (the
        get_covariance path), a size, device or dtype mismatch, or a negative
        or non-finite variance is a ValueError before anything is launched.
        None is the render without the argument, launch for launch.
        depth_distortion: the result also holds
          "distortion"      fp32 [H, W]: sum_i sum_j c_i c_j |m_i - m_j| over
                            the pixel's contributors, with the colour pass's
                            own weights c -- how spread out along the ray they
                            are (the Mip-NeRF 360 / 2DGS distortion loss is its
                            mean).  Differentiable in the geometry, the opacity
                            and, through the depths and the weights, the pose.
          "median_depth"    fp32 [H, W]: the camera-space depth of the
                            Gaussian at which the accumulated opacity reaches
                            one half (the last contributor where it never
                            does, 0 where there is none).  No gradient.
          "median_gaussian" int32 [H, W]: that Gaussian's index, -1 for none.
        m is the camera-space depth z, or with distortion_near_far=(near, far),
        finite with 0 < near < far, 2DGS's inverse depth
        far (z - near) / ((far - near) z).  A differentiable median depth is one
        gather of the camera-space z in torch:
          z_cam = (xyz @ R.T + t)[:, 2];  z_cam[out["median_gaussian"].clamp_min(0).long()]
        The frame takes the stage path, as with features=: the seven standard
        outputs and their gradients are the same bits, and the distortion's
        backward runs only when "distortion" takes part in the loss.  With
        density_stats the statistics see the summed dL/d(viewspace_points),
        the distortion's part included.  A bad distortion_near_far, or one
        without depth_distortion, is a ValueError before anything is launched.
        contribution_stats: optional ContributionStats of the model's size
        on its device.  The forward of this render then ends with the
        contribution pass: per Gaussian, the sum and the maximum over the
        image of its blend weight c_i(p) -- the weights the colour pass
        itself used -- the number of pixels with c_i(p) > 0 and one more view
        for every visible Gaussian are added to it.  No backward is needed: a
        render under torch.no_grad() counts.  Mismatches are a ValueError
        before anything is launched.
        dominant: the result also holds "dominant_gaussian" (int32 [H, W],
        the index of each pixel's strongest contributor, the first in depth
        order among equals, -1 where nothing contributes) and
        "dominant_weight" (fp32 [H, W], its c).
        With either, the frame takes the stage path, as with features=: the
        seven standard outputs and their gradients are the same bits.
        density_stats: optional DensityStats of the model's size on its
        device.  The backward of this render then ends with one launch that
        adds the view to them: per visible Gaussian the NDC-unit norm of
        dL/d(viewspace_points) -- the blend's part, which never surfaces as a
        .grad, plus the caller's own cotangent on out["viewspace_points"] --
        one more view seen, and the largest radius (what 3DGS trainers gather
        with viewspace_points.retain_grad() + add_densification_stats).  No
        backward, no statistics: a render under torch.no_grad(), or one whose
        backward never runs, adds nothing; backward twice (retain_graph) adds
        the view twice.  A size, device, dtype or layout mismatch is a
        ValueError before anything is launched.  DensityStats(n, device,
        abs_grad=True) also accumulate the absolute screen-space gradient
        (AbsGS): per visible Gaussian the same norm of sum_p |dL/dmu(p)| over
        the colour pass's pixels plus |the cotangent on viewspace_points|.
        The frame then takes the stage path (the same bits); a feature image
        or a distortion map adds its gradient to the signed statistic only.
        features: optional floating-point [N, C] per-Gaussian values
        (normals, embeddings, positions, ...) on the Gaussians' device.  The
        result then also holds "features" [C, H, W] fp32: each pixel's
        sum_i c_i features[g_i] with exactly the weights c_i the colour pass
        gave its contributors -- no sigmoid, clamp, background or
        normalisation (a feature background b is the caller's
        out["features"] + (1 - out["alpha"]) * b).  Gradients reach the
        features and, through the weights, the geometry and the pose."""
        if distortion_near_far is not None:
            if not depth_distortion:
                raise ValueError("distortion_near_far needs depth_distortion=True")
            check_distortion_near_far(distortion_near_far)
        wv = _world_view(camera)
        cam = camera_params(camera, settings, self.radius_min, self.radius_max, self.tile_size, world_view=wv)
        # a view on the autograd tape receives its gradient (the reference's
        # autograd reaches world_view_transform(), renderer.py:150-168); any
        # other view is host scalars only, as before
        pose = {"view": wv} if wv.requires_grad else {}
        xyz = gaussians.get_xyz
        fused = getattr(gaussians, "_gs_fused_covariance", False)
        if filter_3d is not None:
            _check_filter_3d(filter_3d, gaussians, fused)
        if normals:
            _check_normals(gaussians, fused, features)
        if fused:
            # this package's GaussianModel: covariance from the raw scaling /
            # rotation and get_opacity's sigmoid are computed in the kernels;
            # the [N,1,3] / [N,1] leaves go in as they are (no view node on the
            # tape: the rasterizer reads rows by stride and returns gradients
            # in the leaves' shapes)
            cov3d, scaling, rotation = None, gaussians._scaling, gaussians._rotation
            logits = gaussians._features_dc
        else:
            cov3d, scaling, rotation = gaussians.get_covariance, None, None
            feats = gaussians.get_features  # one read: the SH rest below is a view of it
            if feats.dim() == 3 and feats.shape[1] >= 1:
                logits = feats[:, 0, :]
            else:
                logits = gaussians._features_dc.squeeze(1)
        opacity = gaussians._opacity if fused else gaussians.get_opacity.squeeze(1)
        opacity_is_logit = fused
        if filter_3d is not None:
            scaling, opacity = apply_filter_3d(scaling, opacity, filter_3d.values)
            opacity_is_logit = False
        sh_degree = settings.sh_degree
        if sh_degree is None:
            sh_degree = int(getattr(gaussians, "active_sh_degree", 0))
        sh_rest = None
        if sh_degree > 0:
            sh_rest = gaussians._features_rest if fused else feats[:, 1:, :]
        grad_dest = None
        # (with a 3D filter the projection's scaling / opacity gradients are those of
        # the map's outputs: they must not land in the bucket as the leaves')
        # (with normals the rotation's gradient has a second part, from the normals' backward)
        sink = getattr(gaussians, "_gs_grad_sink", None) if fused and filter_3d is None and not normals else None
        if sink is not None:
            # data-parallel bucket (distributed.GradAllReduce.attach): the
            # gradient kernels write straight into it when it can take them
            names = ["xyz", "color", "opacity", "scaling", "rotation"]
            leaves = [gaussians._xyz, gaussians._features_dc, gaussians._opacity, gaussians._scaling,
                      gaussians._rotation]
            if sh_degree > 0:
                names.append("sh_rest")
                leaves.append(gaussians._features_rest)

            def grad_dest():
                views = sink.grad_destinations(leaves)
                if views is None:
                    return None
                d = dict(zip(names, views))
                # reduce finished ranges during the backward -- only when the
                # render writes every row of the bucket: a bucket parameter the
                # render does not reach (e.g. _features_rest with sh_degree 0
                # while the model's active degree is > 0) is filled (zero or
                # its .grad) by all_reduce_mean before its collective instead
                if hasattr(sink, "rows_ready") and getattr(sink, "covers", lambda _: False)(leaves):
                    d["_rows_ready"], d["_chunks"] = sink.rows_ready, sink.overlap_chunks()
                return d
        extra = dict(pose)
        if normals:
            n_c = _normals.gaussian_normals(gaussians._rotation, gaussians._scaling, gaussians._xyz, wv)
            extra["features"] = n_c if features is None else torch.cat([features.float(), n_c], dim=1)
        elif features is not None:
            extra["features"] = features
        if density_stats is not None:
            extra["density_stats"] = density_stats
        if contribution_stats is not None:
            extra["contribution_stats"] = contribution_stats
        if dominant:
            extra["dominant"] = True
        if depth_distortion:
            extra["depth_distortion"], extra["distortion_near_far"] = True, distortion_near_far
        image, alpha, depth, means2d, conics, radii, vis, *feature_image = rasterize(
            cam, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit=opacity_is_logit,
            sh_rest=sh_rest, sh_degree=sh_degree, grad_dest=grad_dest, **extra)
        # the reference's output dtypes (renderer.py:74-83, :273-275, :359-367):
        # the projection outputs in the Gaussians' dtype, image in the
        # background's (out_rgb starts as bg), alpha / depth float32 (zeros of
        # the default dtype).  Computed in fp32 here either way.
        if xyz.dtype == torch.float64:
            means2d, conics, radii = means2d.double(), conics.double(), radii.double()
        if torch.as_tensor(settings.bg_color).dtype == torch.float64:
            image = image.double()
        out = {
            "image": image,
            "alpha": alpha,
            "depth": depth,
            "viewspace_points": means2d,
            "visibility_filter": vis,
            "radii": radii,
            "conics": conics,
        }
        if dominant:
            out["dominant_gaussian"], out["dominant_weight"] = feature_image[-2:]
            feature_image = feature_image[:-2]
        if depth_distortion:
            out["distortion"], out["median_depth"], out["median_gaussian"] = feature_image[-3:]
            feature_image = feature_image[:-3]
        if normals:
            if features is None:
                out["normals"] = feature_image[0]
            else:
                c = features.shape[1]
                out["features"], out["normals"] = feature_image[0][:c], feature_image[0][c:]
        elif feature_image:
            out["features"] = feature_image[0]
        return out
