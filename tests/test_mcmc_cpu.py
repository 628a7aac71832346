"""MCMC density control, the parts that need no GPU: the config fields and
their checks, the C ABI's argument checks (they return before any HIP call)
and struct layouts, and the identities of the float64 statements the kernels
are checked against (tests/mcmc_util.py)."""
import ctypes as C
import dataclasses
import math
import os
import subprocess

import numpy as np
import pytest

import mcmc_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_config_defaults_and_yaml_round_trip(pkg, tmp_path):
    c = pkg.TrainingConfig()
    assert (c.mcmc_cap_max, c.mcmc_min_opacity, c.mcmc_noise_lr, c.mcmc_opacity_reg, c.mcmc_scale_reg,
            c.mcmc_grow_factor) == (1_000_000, 0.005, 5e5, 0.01, 0.01, 1.05)
    assert "mcmc" in pkg.config.DENSIFY_CRITERIA and c.densify_criterion == "xyz_grad"
    c2 = pkg.TrainingConfig(densify_criterion="mcmc", mcmc_cap_max=2400, mcmc_noise_lr=1e4, mcmc_grow_factor=1.1)
    c2.check()
    path = tmp_path / "cfg.yaml"
    pkg.ConfigManager.save(c2, str(path))
    back = pkg.ConfigManager.load(str(path))
    assert back == c2 and back.densify_criterion == "mcmc" and back.mcmc_cap_max == 2400


@pytest.mark.parametrize("bad", [
    {"mcmc_cap_max": 0}, {"mcmc_cap_max": -5},
    {"mcmc_noise_lr": -1.0}, {"mcmc_noise_lr": NAN}, {"mcmc_noise_lr": INF},
    {"mcmc_opacity_reg": -0.01}, {"mcmc_opacity_reg": NAN}, {"mcmc_scale_reg": -0.01}, {"mcmc_scale_reg": INF},
    {"mcmc_grow_factor": 0.99}, {"mcmc_grow_factor": NAN},
    {"opacity_reset_interval": 3000}, {"prune_screen_radius": 20.0},
])
def test_config_check_rejects(pkg, bad):
    good = pkg.TrainingConfig(densify_criterion="mcmc")
    good.check()
    with pytest.raises(ValueError, match="|".join(bad)):
        dataclasses.replace(good, **bad).check()
    # the other criteria do not read the mcmc_* fields
    other = {k: v for k, v in bad.items() if k.startswith("mcmc_")}
    if other:
        pkg.TrainingConfig(densify_criterion="screen", **other).check()


def test_exports(pkg):
    for name in ("mcmc_sample", "mcmc_relocate", "mcmc_noise", "mcmc_regularize"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("gs_mcmc_sample", "gs_mcmc_relocate", "gs_mcmc_noise", "gs_mcmc_regularize"):
        assert name in pkg._native.EXPORTS
    assert hasattr(pkg.GaussianModel, "relocate_and_grow")
    assert pkg._native.load().gs_abi_version() == 23


def _buf():
    buf = (C.c_float * 64)()
    return buf, C.addressof(buf)


def test_sample_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    keep, p = _buf()
    assert lib.gs_mcmc_sample(None, None) == 1
    assert b"gs_mcmc_sample" in lib.gs_last_error() and b"null" in lib.gs_last_error()
    a = N.GsMcmcSampleArgs(n=4, num_samples=3, cdf=p, seed=1, idx=p, counts=p)
    for field in ("cdf", "idx", "counts"):
        b = N.GsMcmcSampleArgs.from_buffer_copy(a)
        setattr(b, field, None)
        assert lib.gs_mcmc_sample(C.byref(b), None) == 1, field
    for field in ("n", "num_samples"):
        b = N.GsMcmcSampleArgs.from_buffer_copy(a)
        setattr(b, field, -1)
        assert lib.gs_mcmc_sample(C.byref(b), None) == 1, field
    # nothing to draw, or nothing to draw from: GS_OK with nothing launched, whatever the pointers
    assert lib.gs_mcmc_sample(C.byref(N.GsMcmcSampleArgs(n=4, num_samples=0)), None) == 0
    assert lib.gs_mcmc_sample(C.byref(N.GsMcmcSampleArgs(n=0, num_samples=7)), None) == 0


def test_relocate_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    keep, p = _buf()
    p = (p + 15) & ~15
    assert lib.gs_mcmc_relocate(None, None) == 1
    assert b"gs_mcmc_relocate" in lib.gs_last_error()
    arrays = N.GsModelArrays(p, p, p, p, p, p)
    a = N.GsMcmcRelocateArgs(n=4, rows=6, rest_floats=45, num_samples=2, params=arrays, idx=p, counts=p, dst=p,
                             min_opacity=0.005, workspace=p, workspace_bytes=32)
    assert lib.gs_mcmc_relocate_workspace_bytes(2) == 32 and lib.gs_mcmc_relocate_workspace_bytes(0) == 0
    for field in ("idx", "counts", "dst", "workspace"):
        b = N.GsMcmcRelocateArgs.from_buffer_copy(a)
        setattr(b, field, None)
        assert lib.gs_mcmc_relocate(C.byref(b), None) == 1, field
    for field in ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"):
        b = N.GsMcmcRelocateArgs.from_buffer_copy(a)
        setattr(b.params, field, None)
        assert lib.gs_mcmc_relocate(C.byref(b), None) == 1, field
    for field, bad in (("n", -1), ("rows", 3), ("rest_floats", -1), ("num_samples", -1), ("workspace_bytes", 31),
                       ("workspace", p + 4), ("min_opacity", NAN), ("min_opacity", INF), ("min_opacity", 0.0),
                       ("min_opacity", 1.0)):
        b = N.GsMcmcRelocateArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.gs_mcmc_relocate(C.byref(b), None) == 1, (field, bad)
    assert lib.gs_mcmc_relocate(C.byref(N.GsMcmcRelocateArgs(n=4, rows=4, num_samples=0, min_opacity=0.005)), None) == 0
    assert lib.gs_mcmc_relocate(C.byref(N.GsMcmcRelocateArgs(n=0, rows=0, num_samples=5, min_opacity=0.005)), None) == 0


def test_noise_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    keep, p = _buf()
    p = (p + 15) & ~15
    assert lib.gs_mcmc_noise(None, None) == 1
    a = N.GsMcmcNoiseArgs(n=4, xyz=p, scaling=p, rotation=p, opacity=p, seed=3, scale=0.1)
    assert (a.gate_steepness, round(a.gate_midpoint, 6)) == (100.0, 0.005)  # the binding's defaults
    for field in ("xyz", "scaling", "rotation", "opacity"):
        b = N.GsMcmcNoiseArgs.from_buffer_copy(a)
        setattr(b, field, None)
        assert lib.gs_mcmc_noise(C.byref(b), None) == 1, field
    for field, bad in (("n", -1), ("scale", NAN), ("scale", INF), ("gate_steepness", NAN), ("gate_midpoint", -INF),
                       ("rotation", p + 4)):
        b = N.GsMcmcNoiseArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.gs_mcmc_noise(C.byref(b), None) == 1, (field, bad)
    assert b"gs_mcmc_noise" in lib.gs_last_error()
    # n == 0 or scale == 0: GS_OK, nothing launched
    assert lib.gs_mcmc_noise(C.byref(N.GsMcmcNoiseArgs(n=0, scale=0.1)), None) == 0
    b = N.GsMcmcNoiseArgs.from_buffer_copy(a)
    b.scale = 0.0
    assert lib.gs_mcmc_noise(C.byref(b), None) == 0


def test_regularize_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    keep, p = _buf()
    assert lib.gs_mcmc_regularize(None, None) == 1
    a = N.GsMcmcRegularizeArgs(n=4, opacity=p, scaling=p, d_opacity=p, d_scaling=p, lambda_opacity=0.01,
                               lambda_scale=0.01)
    for field, bad in (("n", -1), ("lambda_opacity", NAN), ("lambda_scale", INF), ("opacity", None), ("scaling", None)):
        b = N.GsMcmcRegularizeArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.gs_mcmc_regularize(C.byref(b), None) == 1, (field, bad)
    assert b"gs_mcmc_regularize" in lib.gs_last_error()
    assert lib.gs_mcmc_regularize(C.byref(N.GsMcmcRegularizeArgs(n=0, lambda_opacity=0.01)), None) == 0
    b = N.GsMcmcRegularizeArgs.from_buffer_copy(a)
    b.d_opacity = b.d_scaling = None  # no gradient to add to: nothing launched
    assert lib.gs_mcmc_regularize(C.byref(b), None) == 0


def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    names = ["gs_mcmc_sample_args", "gs_mcmc_relocate_args", "gs_mcmc_noise_args", "gs_mcmc_regularize_args"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){' +
                   "".join('printf("%%zu\\n", sizeof(%s));' % n for n in names) +
                   'printf("%zu %zu %zu %zu\\n", offsetof(gs_mcmc_sample_args, counts), '
                   'offsetof(gs_mcmc_relocate_args, workspace_bytes), offsetof(gs_mcmc_noise_args, gate_midpoint), '
                   'offsetof(gs_mcmc_regularize_args, lambda_scale));}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S, R, Z, G = N.GsMcmcSampleArgs, N.GsMcmcRelocateArgs, N.GsMcmcNoiseArgs, N.GsMcmcRegularizeArgs
    assert got == [C.sizeof(S), C.sizeof(R), C.sizeof(Z), C.sizeof(G), S.counts.offset, R.workspace_bytes.offset,
                   Z.gate_midpoint.offset, G.lambda_scale.offset]


# -- the statements' own identities -------------------------------------------
def test_ratio_one_changes_nothing():
    for o in (0.005, 0.02, 0.5, 0.99, 1.0 - 2.0 ** -24):
        logit = math.log(o / (1.0 - o))
        scale = np.array([-3.0, -4.5, 0.25])
        new_logit, new_scale = mu.relocate_values(logit, scale, 0, 0.005)
        assert mu.relocation_denominator(o, 1) == o
        assert abs(new_logit - logit) <= 4e-16 * max(1.0, abs(logit)) / min(o, 1.0 - o)  # (logit's own conditioning)
        # x = 1 - (1 - o) is o to half an ulp of 1: 1.1e-16 / 0.005 of relative error at the most
        assert np.abs(new_scale - scale).max() <= 1e-13


def test_denominator_is_positive():
    """D > 0 over o in [0.005, 1 - 2^-24] x R in 1..51, and the alternating
    sum's cancellation (sum of |terms| over |D|) stays below 5e4: float64
    leaves ~1e-11 of relative error, far inside the kernel test's 1e-6."""
    opacities = np.concatenate([np.geomspace(0.005, 0.5, 12), 1.0 - np.geomspace(0.5, 2.0 ** -24, 12)])
    worst = 0.0
    for o in opacities:
        for ratio in range(1, mu.MAX_RATIO + 1):
            x = 1.0 - (1.0 - o) ** (1.0 / ratio)
            d = mu.relocation_denominator(x, ratio)
            assert d > 0.0 and math.isfinite(d), (o, ratio, d)
            mag = sum(math.comb(i - 1, k) * x ** (k + 1) / math.sqrt(k + 1)
                      for i in range(1, ratio + 1) for k in range(i))
            worst = max(worst, mag / d)
    assert worst < 5e4, worst


def test_zero_weight_rows_are_never_sampled():
    rng = np.random.default_rng(5)
    w = rng.integers(1, 1 << 24, 200)
    zero = np.zeros(200, bool)
    zero[[0, 1, 2, 57, 58, 120, 198, 199]] = True  # runs at the start, inside and at the end
    w[zero] = 0
    cdf = np.cumsum(w.astype(np.int64))
    for seed in (0, 0x3C3C0000 + 200):
        idx, counts = mu.sample_statement(cdf, 3000, seed)
        assert idx.min() >= 0 and idx.max() < 200 and counts.sum() == 3000
        assert not counts[zero].any() and not zero[idx].any()
        assert (counts[~zero] > 0).sum() > 150  # (and the rest are drawn)
    # a single live row takes every sample, wherever it is
    for only in (0, 99, 199):
        w1 = np.zeros(200, np.int64)
        w1[only] = 12345
        idx, _ = mu.sample_statement(np.cumsum(w1), 50, 9)
        assert (idx == only).all()
