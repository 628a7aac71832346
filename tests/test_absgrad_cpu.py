"""Absolute screen-space gradients (AbsGS), the parts that need no GPU: the
fp64 statement of tests/absgrad_reference.py tied to the pinned one and to
finite differences, the fp32 formulation that sets the constant K of the GPU
tests' bound, the C ABI's layouts and argument checks (they return before any
HIP call), and the host rules.

The bound of tests/test_absgrad_gpu.py, fixed here before any GPU run:

    |x_gpu - x_fp64| <= K (n_p + 1) 2^-24 M

x: the absolute partial sum_p |dL/dmu_x(p)| or sum_p |dL/dmu_y(p)| of one
(list entry, 8x8 cell); M: blend_reference.reference_tile's M[:, q, 0] and
M[:, q, 1] -- sums of absolute values already, so they bound the absolute
partial as they bound the signed one; n_p: the cell's evaluated entries.
K = 4 x the largest ratio err / ((n_p + 1) 2^-24 M) that the documented
formulation shows in plain numpy fp32 (absgrad_reference.emulate_abs_tile)
against the statement, on a host-built frame of every blend_reference.CASES
entry under each of the four cotangent sets (CPU_RATIOS below):

    K = 3 = ceil(4 x 0.657);  measured on the CPU: 0.657 (subpixel16, no_depth).

The absolute sum has no cancellation and no moments, so it stays far below the
signed partials' constant (test_blend_stage: 12.5 measured, K = 51); the
largest ratios are the sub-pixel rows', whose weight exp(-s/2) carries the
fp32 rounding of s at |s/2| times its own size."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import absgrad_reference as AR
import blend_reference as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 3.0
K_CPU_MEASURED = 0.657
# case -> the numpy fp32 formulation's largest ratio under (all, no_alpha, no_depth, image_only)
CPU_RATIOS = {
    "ordinary16": (0.0281, 0.0228, 0.0223, 0.0173), "ordinary12": (0.0338, 0.0335, 0.0295, 0.0332),
    "thin16": (0.0107, 0.00996, 0.00951, 0.00841), "thin12": (0.0115, 0.0145, 0.0237, 0.0261),
    "opaque16": (0.0155, 0.0171, 0.0233, 0.0227), "opaque12": (0.00959, 0.00934, 0.0215, 0.0238),
    "general16": (0.0203, 0.0210, 0.0216, 0.0170), "general12": (0.0358, 0.0346, 0.0282, 0.0242),
    "bright16": (0.0164, 0.0163, 0.0488, 0.0176), "bright12": (0.0354, 0.0400, 0.144, 0.0228),
    "subpixel16": (0.0301, 0.0372, 0.657, 0.582), "tile8": (0.0237, 0.0224, 0.0340, 0.0272),
    "tile20": (0.0219, 0.0177, 0.0630, 0.0497),
}


@functools.lru_cache(maxsize=2)
def _host_case(name, which):
    return AR.host_case(name, which)


# ---- the statement -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.CASES))
def test_fp32_formulation_sets_K_and_statement_ties_to_the_pinned_one(name):
    """Every case under the four cotangent sets: the per-pixel gradients summed
    per cell equal reference_tile's dmu partials to fp64 rounding, the absolute
    sums dominate them, and the fp32 formulation stays within K / 4."""
    assert set(CPU_RATIOS) == set(B.CASES)
    ratios = []
    for which in B.COTANGENTS:
        fr, cot, ems, refs, pgs = _host_case(name, which)
        worst = 0.0
        for t, ref in refs.items():
            pg = pgs[t]
            signed, want = AR.cell_sums(fr, pg, False), AR.abs_partials(fr, pg)
            M = ref["M"][:, :, 0:2]
            # (the same autograd graph summed in another order: 1e-12 of the absolute-value sum)
            assert (np.abs(signed - ref["partials"][:, :, 0:2]) <= 1e-12 * M).all(), (name, which, t)
            assert (want >= np.abs(signed) - 1e-12 * M).all()
            assert (want <= M * (1 + 1e-9)).all(), "M bounds the absolute partial"
            worst = max(worst, AR.abs_ratio(AR.emulate_abs_tile(fr, t, *cot, em=ems[t]), want, ref))
        ratios.append(worst)
    print(f"{name}: fp32 formulation err / unit {', '.join(f'{r:.3g}' for r in ratios)} (K = {K})")
    assert 4.0 * max(ratios) <= K
    # (the recorded table is this measurement, up to the host's exp)
    assert np.allclose(ratios, CPU_RATIOS[name], rtol=0.1), (ratios, CPU_RATIOS[name])


def test_K_is_four_times_the_measured_ratio():
    assert max(max(v) for v in CPU_RATIOS.values()) == K_CPU_MEASURED
    assert K == float(np.ceil(4.0 * K_CPU_MEASURED))


def test_pixel_gradients_match_finite_differences():
    """6 Gaussians on 8x8 pixels, away from every decision (the scene of
    test_blend_stage's finite-difference test): the gradient of each
    (entry, pixel) leaf of mu_x, mu_y against central differences in fp64."""
    rng = np.random.default_rng(5)
    n = 6
    sc = B.make_scene(8, 8, 8, rng.uniform(1, 7, n), rng.uniform(1, 7, n), np.linspace(2, 4, n), rng.uniform(2.5, 4, n),
                      rng.uniform(2.5, 4, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.1, 0.4, n),
                      rng.uniform(0.2, 0.8, (n, 3)), bg=(0.05, 0.1, 0.02))
    fr = B.cpu_frame(sc)
    assert len(fr.entries(0)) == n
    gi, ga, gd = B.case_cotangents(sc)
    pg = AR.pixel_gradients(fr, 0, gi, ga, gd)
    G = pg["G"]
    P = G.shape[1]
    assert P == 64 and (G != 0).all()
    # both signs among an entry's pixels: what the signed sum cancels
    assert ((G > 0).any(1) & (G < 0).any(1)).all()
    base = np.repeat(fr.records[fr.entries(0)][:, list(B.REC_COL)].astype(np.float64)[:, None, :], P, 1)
    loss = lambda v: AR.pixel_gradients(fr, 0, gi, ga, gd, values=v)["loss"]
    worst = 0.0
    for i in range(n):
        for p in range(i, P, 7):
            for k in range(2):
                h = 1e-6
                vp, vm = base.copy(), base.copy()
                vp[i, p, k] += h
                vm[i, p, k] -= h
                fd = (loss(vp) - loss(vm)) / (2 * h)
                scale = np.abs(G[i, :, k]).max()
                worst = max(worst, abs(fd - G[i, p, k]) / scale)
                assert abs(fd - G[i, p, k]) <= 1e-7 * scale, (i, p, k, fd, G[i, p, k])
    print(f"finite differences: worst relative difference {worst:.3g}")


# ---- the C ABI -----------------------------------------------------------------------
def test_abi_version_and_exports(pkg):
    N = pkg._native
    assert N.GS_ABI_VERSION == 23 and N.load().gs_abi_version() == 23
    for name in ("gs_blend_backward_abs", "gs_gather_abs_partials", "gs_density_accumulate_abs"):
        assert name in N.EXPORTS and hasattr(N.load(), name)


def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(gs_abs_gather_args), offsetof(gs_abs_gather_args, vis), '
                   'offsetof(gs_abs_gather_args, partial_groups), offsetof(gs_abs_gather_args, accumulate), '
                   'offsetof(gs_abs_gather_args, abs_sums), '
                   'sizeof(gs_density_abs_args), offsetof(gs_density_abs_args, abs_sums), '
                   'offsetof(gs_density_abs_args, abs_accum), '
                   'sizeof(gs_densify_args), offsetof(gs_densify_args, max_screen_radius), '
                   'offsetof(gs_densify_args, split_accum), offsetof(gs_densify_args, split_threshold));}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    A, D, S = N.GsAbsGatherArgs, N.GsDensityAbsArgs, N.GsDensifyArgs
    assert sizes == [C.sizeof(A), A.vis.offset, A.partial_groups.offset, A.accumulate.offset, A.abs_sums.offset,
                     C.sizeof(D), D.abs_sums.offset, D.abs_accum.offset,
                     C.sizeof(S), S.max_screen_radius.offset, S.split_accum.offset, S.split_threshold.offset]
    # gs_density_stats_args' fields, then the two new ones
    assert D.stats.offset == 0 and D.abs_sums.offset == C.sizeof(N.GsDensityStatsArgs)


def test_stale_library_is_named_by_its_missing_exports(pkg, tmp_path, monkeypatch):
    """A library built before this feature has the same ABI number: load()
    names the three exports it lacks, and no other."""
    N = pkg._native
    new = ("gs_blend_backward_abs", "gs_gather_abs_partials", "gs_density_accumulate_abs")
    old = [e for e in N.EXPORTS if e not in new and e not in ("gs_abi_version", "gs_last_error")]
    src = tmp_path / "old.c"
    src.write_text("int gs_abi_version(void) { return %d; }\nconst char *gs_last_error(void) { return \"\"; }\n"
                   % N.GS_ABI_VERSION + "".join(f"int {e}(void) {{ return 1; }}\n" for e in old))
    so = tmp_path / "libold.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.NativeLibraryError, match="out of date") as e:
        N.load(str(so))
    msg = str(e.value)
    assert all(name in msg for name in new)
    assert "lacks " + ", ".join(new) in msg


def test_bad_arguments_return_before_any_launch(pkg):
    N = pkg._native
    lib = N.load()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    # gs_blend_backward_abs: its own check first, then gs_blend_backward's
    assert lib.gs_blend_backward_abs(None, p, None) == 1 and b"gs_blend_backward_abs" in lib.gs_last_error()
    ba = N.GsBlendBwdArgs()
    assert lib.gs_blend_backward_abs(C.byref(ba), None, None) == 1 and b"abs_grads" in lib.gs_last_error()
    assert lib.gs_blend_backward_abs(C.byref(ba), p + 4, None) == 1 and b"aligned" in lib.gs_last_error()
    assert lib.gs_blend_backward_abs(C.byref(ba), p, None) != 0 and b"gs_blend_backward_abs" in lib.gs_last_error()
    # gs_gather_abs_partials
    assert lib.gs_gather_abs_partials(None, None) == 1 and b"gs_gather_abs_partials" in lib.gs_last_error()
    ga = N.GsAbsGatherArgs(n=4, partial_groups=4)
    assert lib.gs_gather_abs_partials(C.byref(ga), None) == 1 and b"null buffer" in lib.gs_last_error()
    for name in ("vis", "rects", "pair_offset", "abs_grads", "slot_live", "abs_sums"):
        setattr(ga, name, p)
    ga.partial_groups = 0
    assert lib.gs_gather_abs_partials(C.byref(ga), None) == 1
    ga.partial_groups, ga.n = 4, -1
    assert lib.gs_gather_abs_partials(C.byref(ga), None) == 1
    assert lib.gs_gather_abs_partials(C.byref(N.GsAbsGatherArgs(n=0)), None) == 0  # nothing to gather: no launch
    # gs_density_accumulate_abs: gs_density_accumulate's checks, and abs_accum
    assert lib.gs_density_accumulate_abs(None, None) == 1 and b"gs_density_accumulate_abs" in lib.gs_last_error()
    st = N.GsDensityStatsArgs(n=4, image_width=52, image_height=44, vis=p, radii=p, grad_sums=None, g_means2d=None,
                              grad_accum=p, denom=p, max_radii=p)
    da = N.GsDensityAbsArgs(st, None, None)
    assert lib.gs_density_accumulate_abs(C.byref(da), None) == 1 and b"abs_accum" in lib.gs_last_error()
    da.abs_accum, da.stats.vis = p, None
    assert lib.gs_density_accumulate_abs(C.byref(da), None) == 1 and b"vis" in lib.gs_last_error()
    da.stats.vis, da.stats.image_width = p, 0
    assert lib.gs_density_accumulate_abs(C.byref(da), None) == 1 and b"image_width" in lib.gs_last_error()
    da.stats.image_width, da.stats.n = 52, 0
    assert lib.gs_density_accumulate_abs(C.byref(da), None) == 0
    # gs_densify_args.split_accum needs the signed statistics beside it
    a = N.GsDensifyArgs()
    a.split_accum = p
    assert lib.gs_densify_count(C.byref(a), None) == 1 and b"split_accum" in lib.gs_last_error()
    assert lib.gs_densify_emit(C.byref(a), None) == 1
    a.grad_accum = p  # (still no denominator)
    assert lib.gs_densify_count(C.byref(a), None) == 1


# ---- host rules ----------------------------------------------------------------------
def test_config_fields_check_and_yaml_round_trip(pkg, tmp_path):
    c = pkg.TrainingConfig()
    assert (c.densify_absgrad, c.densify_abs_grad_threshold) == (False, 0.0008)
    c.check()
    for criterion in ("xyz_grad", "mcmc"):
        with pytest.raises(ValueError, match="densify_absgrad"):
            pkg.TrainingConfig(densify_criterion=criterion, densify_absgrad=True).check()
    with pytest.raises(ValueError, match="densify_abs_grad_threshold"):
        pkg.TrainingConfig(densify_criterion="screen", densify_absgrad=True, densify_abs_grad_threshold=-1.0).check()
    c2 = pkg.TrainingConfig(densify_criterion="screen", densify_absgrad=True, densify_abs_grad_threshold=0.002)
    c2.check()
    path = tmp_path / "cfg.yaml"
    pkg.ConfigManager.save(c2, str(path))
    back = pkg.ConfigManager.load(str(path))
    assert back == c2 and (back.densify_absgrad, back.densify_abs_grad_threshold) == (True, 0.002)


def test_absgrad_with_another_criterion_is_refused_at_setup(pkg, tmp_path):
    for criterion in ("xyz_grad", "mcmc"):
        cfg = pkg.TrainingConfig(densify_criterion=criterion, densify_absgrad=True, data_path=str(tmp_path / "nothing"))
        with pytest.raises(ValueError, match="densify_absgrad"):
            pkg.GaussianTrainer(cfg).setup()


def test_density_stats_object_with_abs_grad(pkg):
    s = pkg.DensityStats(5, "cpu")
    assert s.abs_accum is None
    with pytest.raises(ValueError, match="abs_grad=True"):
        s.mean_abs_grad()
    s = pkg.DensityStats(5, "cpu", abs_grad=True)
    t = s.abs_accum
    assert t.shape == (5,) and t.dtype == torch.float32 and t.is_contiguous() and not t.any()
    s.abs_accum += torch.tensor([1.0, 2.0, 3.0, 0.0, 5.0])
    s.denom += torch.tensor([2.0, 0.0, 3.0, 0.0, 1.0])
    assert torch.equal(s.mean_abs_grad(), torch.tensor([0.5, 0.0, 1.0, 0.0, 5.0]))
    s.reset()
    assert s.abs_accum is t and not t.any() and not s.denom.any()
    # the model's statistics follow config.densify_absgrad wherever they are re-made
    m = pkg.GaussianModel(pkg.TrainingConfig(densify_criterion="screen", densify_absgrad=True))
    m.create_from_random(7, device="cpu", generator=torch.Generator().manual_seed(0))
    assert m.density_stats.n == 7 and m.density_stats.abs_accum.shape == (7,)
    m.density_stats.abs_accum += 1
    m.prune_points(torch.tensor([True, False, True, True, False, True, True]))
    assert m.density_stats.n == 5 and m.density_stats.abs_accum.shape == (5,) and not m.density_stats.abs_accum.any()
    m0 = pkg.GaussianModel()
    m0.create_from_random(3, device="cpu", generator=torch.Generator().manual_seed(0))
    assert m0.density_stats.abs_accum is None


def test_abs_accum_is_checked_before_any_launch(pkg):
    check = pkg.rasterizer._check_density_stats
    cpu = torch.device("cpu")
    check(pkg.DensityStats(4, "cpu", abs_grad=True), 4, cpu)
    shape, dtype, strided, kind = (pkg.DensityStats(4, "cpu", abs_grad=True) for _ in range(4))
    shape.abs_accum = torch.zeros(4, 2)
    dtype.abs_accum = torch.zeros(4, dtype=torch.float64)
    strided.abs_accum = torch.zeros(8)[::2]
    kind.abs_accum = [0.0] * 4
    for bad in (shape, dtype, strided, kind, pkg.DensityStats(3, "cpu", abs_grad=True)):
        with pytest.raises(ValueError, match="density_stats"):
            check(bad, 4, cpu)
    # the model refuses an absolute threshold its statistics cannot serve (before any launch)
    m = pkg.GaussianModel()
    m.create_from_random(4, device="cpu", generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="abs_grad=True"):
        m.densify_and_prune(0.0002, 1.0, stats=m.density_stats, abs_grad_threshold=0.0008)
