"""Density control on screen-space statistics, the parts that need no GPU:
the C ABI's argument checks (they return before any HIP call) and struct
layout, the config fields, and the 3DGS opacity reset."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_density_accumulate_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    assert "gs_density_accumulate" in N.EXPORTS
    assert lib.gs_density_accumulate(None, None) == 1
    assert b"gs_density_accumulate" in lib.gs_last_error() and b"null" in lib.gs_last_error()
    buf = (C.c_float * 8)()
    p = C.addressof(buf)
    a = N.GsDensityStatsArgs(n=4, image_width=52, image_height=44, vis=None, radii=p, grad_sums=None,
                             g_means2d=None, grad_accum=p, denom=p, max_radii=p)
    assert lib.gs_density_accumulate(C.byref(a), None) == 1  # NULL vis with n > 0
    assert b"vis" in lib.gs_last_error()
    a.vis, a.image_width = p, 0
    assert lib.gs_density_accumulate(C.byref(a), None) == 1  # W = 0
    assert b"image_width" in lib.gs_last_error()
    a.image_width, a.image_height = 52, -1
    assert lib.gs_density_accumulate(C.byref(a), None) == 1
    a.image_height, a.n = 44, -1
    assert lib.gs_density_accumulate(C.byref(a), None) == 1
    # n == 0: GS_OK with nothing launched, whatever the pointers
    assert lib.gs_density_accumulate(C.byref(N.GsDensityStatsArgs(n=0, image_width=8, image_height=8)), None) == 0


def test_densify_refuses_two_gradient_criteria(pkg):
    N = pkg._native
    lib = N.load()
    buf = (C.c_float * 8)()
    p = C.addressof(buf)
    a = N.GsDensifyArgs()
    a.xyz_grad, a.grad_accum, a.grad_denom = p, p, p
    assert lib.gs_densify_count(C.byref(a), None) == 1
    assert b"grad_accum" in lib.gs_last_error()
    a.xyz_grad, a.grad_denom = None, None  # grad_accum without its denominator
    assert lib.gs_densify_count(C.byref(a), None) == 1
    assert b"grad_denom" in lib.gs_last_error()
    assert lib.gs_densify_emit(C.byref(a), None) == 1


def test_density_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(gs_density_stats_args), '
                   'offsetof(gs_density_stats_args, vis), offsetof(gs_density_stats_args, max_radii), '
                   'sizeof(gs_densify_args), offsetof(gs_densify_args, grad_accum), '
                   'offsetof(gs_densify_args, max_screen_radius));}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S, D = N.GsDensityStatsArgs, N.GsDensifyArgs
    assert sizes == [C.sizeof(S), S.vis.offset, S.max_radii.offset, C.sizeof(D), D.grad_accum.offset,
                     D.max_screen_radius.offset]


def test_config_fields_and_yaml_round_trip(pkg, tmp_path):
    c = pkg.TrainingConfig()
    assert (c.densify_criterion, c.prune_screen_radius, c.opacity_reset_interval) == ("xyz_grad", 0.0, 0)
    c.check()
    c2 = pkg.TrainingConfig(densify_criterion="screen", prune_screen_radius=20.0, opacity_reset_interval=3000)
    c2.check()
    path = tmp_path / "cfg.yaml"
    pkg.ConfigManager.save(c2, str(path))
    back = pkg.ConfigManager.load(str(path))
    assert back == c2
    assert (back.densify_criterion, back.prune_screen_radius, back.opacity_reset_interval) == ("screen", 20.0, 3000)


def test_unknown_criterion_is_refused_at_setup(pkg, tmp_path):
    cfg = pkg.TrainingConfig(densify_criterion="viewspace", data_path=str(tmp_path / "nothing"))
    with pytest.raises(ValueError, match="densify_criterion"):
        pkg.GaussianTrainer(cfg).setup()


def test_density_stats_object(pkg):
    assert "DensityStats" in pkg.__all__
    s = pkg.DensityStats(5, "cpu")
    for t in (s.grad_accum, s.denom, s.max_radii):
        assert t.shape == (5,) and t.dtype == torch.float32 and t.is_contiguous() and not t.any()
    s.grad_accum += torch.tensor([1.0, 2.0, 3.0, 0.0, 5.0])
    s.denom += torch.tensor([2.0, 0.0, 3.0, 0.0, 1.0])
    assert torch.equal(s.mean_grad(), torch.tensor([0.5, 0.0, 1.0, 0.0, 5.0]))
    s.max_radii += 1
    s.reset()
    assert not s.grad_accum.any() and not s.denom.any() and not s.max_radii.any()
    # the model carries one of its own size, re-made as zeros with the reference-named buffers
    m = pkg.GaussianModel()
    m.create_from_random(7, device="cpu", generator=torch.Generator().manual_seed(0))
    assert m.density_stats.n == 7 and m.xyz_gradient_accum.shape == (7, 3) and m.denom.shape == (7, 1)
    m.density_stats.denom += 1
    m.prune_points(torch.tensor([True, False, True, True, False, True, True]))
    assert m.density_stats.n == 5 and not m.density_stats.denom.any() and m.max_radii2D.shape == (5,)


def test_density_stats_are_checked_before_any_launch(pkg):
    """Size, dtype and layout mismatches are ValueErrors of rasterize's own
    argument check (a host function: no launch can have happened)."""
    check = pkg.rasterizer._check_density_stats
    cpu = torch.device("cpu")
    check(pkg.DensityStats(4, "cpu"), 4, cpu)
    wrong_dtype, strided = pkg.DensityStats(4, "cpu"), pkg.DensityStats(4, "cpu")
    wrong_dtype.denom = wrong_dtype.denom.double()
    strided.max_radii = torch.zeros(8)[::2]
    for bad in (pkg.DensityStats(3, "cpu"), wrong_dtype, strided):
        with pytest.raises(ValueError, match="density_stats"):
            check(bad, 4, cpu)
    with pytest.raises(TypeError, match="DensityStats"):
        check(torch.zeros(4), 4, cpu)


def test_cap_opacity(pkg):
    m = pkg.GaussianModel()
    m.create_from_random(8, device="cpu", generator=torch.Generator().manual_seed(1))
    cap = torch.tensor(math.log(0.01 / 0.99), dtype=torch.float32)  # -4.59512
    logits = torch.tensor([-9.0, -4.6, float(cap), -4.59, -4.0, 0.0, 3.0, -4.5952])
    assert (logits < cap).sum() == 3 and (logits > cap).sum() == 4
    with torch.no_grad():
        m._opacity.copy_(logits[:, None])
    opt = pkg.optim.GaussianOptimizer(m, pkg.TrainingConfig())
    opt.setup_optimizer()
    g = torch.Generator().manual_seed(2)
    for p in m.parameter_list():
        opt.optimizer.state[p] = {"step": 7, "exp_avg": torch.randn(p.shape, generator=g),
                                  "exp_avg_sq": torch.rand(p.shape, generator=g)}
    others = [p for p in m.parameter_list() if p is not m._opacity]
    before = [(opt.optimizer.state[p], opt.optimizer.state[p]["exp_avg"], opt.optimizer.state[p]["exp_avg_sq"],
               opt.optimizer.state[p]["exp_avg"].clone(), opt.optimizer.state[p]["exp_avg_sq"].clone())
              for p in others]
    param = m._opacity
    opt.cap_opacity()
    assert m._opacity is param
    assert torch.equal(m._opacity.detach()[:, 0], torch.minimum(logits, cap))
    st = opt.optimizer.state[m._opacity]
    assert st["step"] == 7 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert st["exp_avg"].shape == (8, 1) and st["exp_avg_sq"].shape == (8, 1)
    assert len(others) == 5
    for p, (state, ea, eas, ea0, eas0) in zip(others, before):
        s = opt.optimizer.state[p]
        assert s is state and s["step"] == 7 and s["exp_avg"] is ea and s["exp_avg_sq"] is eas
        assert torch.equal(ea, ea0) and torch.equal(eas, eas0)
    # another cap, and the reference-named reset keeps its own meaning (every opacity set)
    opt.cap_opacity(0.5)
    assert torch.equal(m._opacity.detach()[:, 0], torch.minimum(logits, cap))
    opt.reset_opacity()
    assert torch.allclose(torch.sigmoid(m._opacity.detach()), torch.full((8, 1), 0.01))
