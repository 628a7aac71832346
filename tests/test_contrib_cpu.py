"""The contribution pass without a GPU: the ctypes mirrors have the C
compiler's layout, the entry points reject bad arguments before any HIP call,
the Python layers refuse mismatches before any native call, pruning carries
the Adam state, and the statistics all-reduce as SUM / MAX / SUM / SUM."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import replay_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _camera(a, width=40, height=24, tile=16):
    a.cam.image_width, a.cam.image_height, a.cam.tile_size = width, height, tile
    a.tiles_x, a.tiles_y = (width + tile - 1) // tile, (height + tile - 1) // tile


def _buffer():
    buf = (C.c_float * 16)()
    return buf, C.cast(buf, C.c_void_p).value


# ------------------------------------------------------------ 1: layouts ----
def test_abi_version_unchanged(pkg):
    N = pkg._native
    assert N.load().gs_abi_version() == 23 and N.GS_ABI_VERSION == 23
    assert N.GS_CONTRIB_STRIDE == 4
    assert "gs_blend_contributions" in N.EXPORTS and "gs_contrib_accumulate" in N.EXPORTS


def test_struct_layouts_match_c(pkg, tmp_path):
    N = pkg._native
    structs = [("gs_contrib_args", N.GsContribArgs), ("gs_contrib_gather_args", N.GsContribGatherArgs)]
    body = []
    for cname, mirror in structs:
        body.append('printf("%%zu\\n", sizeof(%s));' % cname)
        for field, _ in mirror._fields_:
            body.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){' + "".join(body) +
                   'printf("%d\\n", GS_CONTRIB_STRIDE);}')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    exp = []
    for _, mirror in structs:
        exp.append(C.sizeof(mirror))
        exp.extend(getattr(mirror, field).offset for field, _ in mirror._fields_)
    exp.append(N.GS_CONTRIB_STRIDE)
    assert got == exp
    # the frame inside gs_contrib_args, field by field, and the bytes the flat struct had
    replay_layout.check(pkg, tmp_path, ["gs_contrib_args"])


# --------------------------------------------------------- 2: validation ----
_CONTRIB_REQUIRED = ("ranges", "sorted_gauss", "records", "cell_neval", "partials", "slot_live")


def _valid_contrib(N, p):
    a = N.GsContribArgs()
    _camera(a, tile=24)  # 9 cells
    for name in _CONTRIB_REQUIRED:
        setattr(a, name, p)
    a.num_pairs, a.num_gaussians = 3, 2
    return a


def test_contributions_reject_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    buf, p = _buffer()
    assert lib.gs_blend_contributions(None, None) == 1
    assert b"gs_blend_contributions" in lib.gs_last_error() and b"null" in lib.gs_last_error()
    a = _valid_contrib(N, p)
    a.cam.tile_size = 0
    assert lib.gs_blend_contributions(C.byref(a), None) == 3
    a = _valid_contrib(N, p)
    a.tiles_x += 1
    assert lib.gs_blend_contributions(C.byref(a), None) == 1
    assert b"tiles_x" in lib.gs_last_error()
    for name in _CONTRIB_REQUIRED:  # each required pointer
        a = _valid_contrib(N, p)
        setattr(a, name, None)
        assert lib.gs_blend_contributions(C.byref(a), None) == 1, name
        assert b"null buffer" in lib.gs_last_error()
    a = _valid_contrib(N, p)
    a.live_bits, a.live_words = p, 0  # a bitmap without its row length
    assert lib.gs_blend_contributions(C.byref(a), None) == 1
    for field in ("num_pairs", "num_gaussians"):  # negative sizes
        a = _valid_contrib(N, p)
        setattr(a, field, -1)
        assert lib.gs_blend_contributions(C.byref(a), None) == 1, field
        assert b"negative" in lib.gs_last_error()
    for begin, count in ((-1, 2), (0, 10), (8, 2), (9, 1), (3, -1), (4, 0)):  # outside the tile's 9 cells
        a = _valid_contrib(N, p)
        a.cell_begin, a.cell_count = begin, count
        assert lib.gs_blend_contributions(C.byref(a), None) == 1, (begin, count)
        assert b"cell batch" in lib.gs_last_error()
    for one in ("dominant_id", "dominant_weight"):  # one map without the other
        a = _valid_contrib(N, p)
        setattr(a, one, p)
        assert lib.gs_blend_contributions(C.byref(a), None) == 1, one
        assert b"dominant" in lib.gs_last_error()


def test_contributions_of_nothing_are_ok(pkg):
    """n == 0 or num_pairs == 0 without the maps: GS_OK and no launch (this
    process has no device)."""
    N = pkg._native
    lib = N.load()
    buf, p = _buffer()
    for field in ("num_gaussians", "num_pairs"):
        a = _valid_contrib(N, p)
        setattr(a, field, 0)
        assert lib.gs_blend_contributions(C.byref(a), None) == 0, field
    a = _valid_contrib(N, p)
    a.num_pairs, a.sorted_gauss = 0, None  # (no list: nothing to read it for)
    assert lib.gs_blend_contributions(C.byref(a), None) == 0


_GATHER_REQUIRED = ("vis", "rects", "pair_offset", "partials", "slot_live", "weight_sum", "weight_max", "pixels",
                    "views")


def test_accumulate_rejects_bad_arguments(pkg):
    N = pkg._native
    lib = N.load()
    buf, p = _buffer()
    assert lib.gs_contrib_accumulate(None, None) == 1
    assert b"gs_contrib_accumulate" in lib.gs_last_error()

    def valid():
        a = N.GsContribGatherArgs(n=4, partial_groups=4, first_batch=1)
        for name in _GATHER_REQUIRED:
            setattr(a, name, p)
        return a

    for name in _GATHER_REQUIRED:
        a = valid()
        setattr(a, name, None)
        assert lib.gs_contrib_accumulate(C.byref(a), None) == 1, name
        assert b"null buffer" in lib.gs_last_error()
    a = valid()
    a.n = -1
    assert lib.gs_contrib_accumulate(C.byref(a), None) == 1
    for bad in (0, -2):
        a = valid()
        a.partial_groups = bad
        assert lib.gs_contrib_accumulate(C.byref(a), None) == 1
    a = valid()
    a.n = 0
    assert lib.gs_contrib_accumulate(C.byref(a), None) == 0


# ------------------------------------------------- 3: Python-side refusals ----
def test_contribution_stats_object(pkg):
    st = pkg.ContributionStats(5, "cpu")
    assert [(t.dtype, tuple(t.shape)) for t in (st.weight_sum, st.weight_max, st.pixels, st.views)] == [
        (torch.float32, (5,)), (torch.float32, (5,)), (torch.int64, (5,)), (torch.int32, (5,))]
    assert not any(bool(t.any()) for t in (st.weight_sum, st.weight_max, st.pixels, st.views))
    st.weight_sum.copy_(torch.tensor([6.0, 0.0, 1.0, 0.5, 9.0]))
    st.pixels.copy_(torch.tensor([3, 0, 4, 1, 0]))
    assert torch.equal(st.mean_weight(), torch.tensor([2.0, 0.0, 0.25, 0.5, 0.0]))
    st.views.fill_(2)
    st.weight_max.fill_(0.5)
    st.reset()
    assert not any(bool(t.any()) for t in (st.weight_sum, st.weight_max, st.pixels, st.views))
    assert st.device == torch.device("cpu") and st.n == 5


def test_contribution_stats_mismatches_raise_before_any_launch(pkg, monkeypatch):
    R = pkg.rasterizer
    monkeypatch.setattr(pkg._native, "load", lambda *a, **k: pytest.fail("a native call was made"))
    dev = torch.device("cpu")
    with pytest.raises(TypeError):
        R._check_contribution_stats(pkg.DensityStats(4, dev), 4, dev)
    with pytest.raises(ValueError, match="holds 3"):
        R._check_contribution_stats(pkg.ContributionStats(3, dev), 4, dev)
    R._check_contribution_stats(pkg.ContributionStats(4, dev), 4, dev)
    with pytest.raises(ValueError, match="on meta"):  # device
        R._check_contribution_stats(pkg.ContributionStats(4, dev), 4, torch.device("meta"))
    for name, bad in (("weight_sum", torch.zeros(4, dtype=torch.float64)),   # dtype
                      ("weight_max", torch.zeros(8)[::2]),                   # layout
                      ("pixels", torch.zeros(4, dtype=torch.int32)),         # dtype
                      ("views", torch.zeros((4, 1), dtype=torch.int32)),     # shape
                      ("views", torch.zeros(4, dtype=torch.int64))):
        st = pkg.ContributionStats(4, dev)
        setattr(st, name, bad)
        with pytest.raises(ValueError, match=name):
            R._check_contribution_stats(st, 4, dev)


def test_config_check_rejects(pkg):
    cfg = pkg.TrainingConfig()
    assert cfg.contribution_prune_iterations == () and cfg.contribution_prune_threshold == 0.01
    cfg.check()
    pkg.TrainingConfig(contribution_prune_iterations=(10, 500), contribution_prune_threshold=0.0).check()
    for bad in (-0.01, float("nan")):
        with pytest.raises(ValueError, match="contribution_prune_threshold"):
            pkg.TrainingConfig(contribution_prune_threshold=bad).check()
    for bad in ((0,), (100, -5), (2.5,)):
        with pytest.raises(ValueError, match="contribution_prune_iterations"):
            pkg.TrainingConfig(contribution_prune_iterations=bad).check()


def _cpu_model(pkg, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = pkg.GaussianModel()
    m._set(torch.randn(n, 3, generator=g), torch.randn(n, 1, 3, generator=g), torch.randn(n, 15, 3, generator=g),
           torch.randn(n, 3, generator=g), torch.randn(n, 4, generator=g), torch.randn(n, 1, generator=g))
    return m


def test_prune_by_contribution_negative_threshold(pkg, monkeypatch):
    monkeypatch.setattr(pkg._native, "load", lambda *a, **k: pytest.fail("a native call was made"))
    m = _cpu_model(pkg, 6)
    opt = pkg.optim.GaussianOptimizer(m, pkg.TrainingConfig())
    st = pkg.ContributionStats(6, "cpu")
    for bad in (-1e-9, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            opt.prune_by_contribution(st, bad)
    with pytest.raises(ValueError, match="holds 5"):
        opt.prune_by_contribution(pkg.ContributionStats(5, "cpu"), 0.0)
    assert m.get_num_points() == 6


# ------------------------------------------------------- 4: prune_points ----
def test_prune_points_carries_adam_state(pkg):
    n = 9
    m = _cpu_model(pkg, n, seed=1)
    params = m.parameter_list()
    opt = torch.optim.Adam([{"params": [m._xyz], "lr": 1e-3}, {"params": [m._features_dc, m._features_rest]},
                            {"params": [m._opacity]}, {"params": [m._scaling]}, {"params": [m._rotation]}])
    g = torch.Generator().manual_seed(2)
    before = []
    for i, p in enumerate(params):
        if i == 2:  # (features_rest: no state yet, as while SH colour is off)
            before.append(None)
            continue
        st = {"step": 7 + i, "exp_avg": torch.randn(p.shape, generator=g),
              "exp_avg_sq": torch.rand(p.shape, generator=g)}
        opt.state[p] = st
        before.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()})
    values = [p.detach().clone() for p in params]
    mask = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=torch.bool)
    m.contribution_stats.weight_max.fill_(1.0)
    m.prune_points(mask, opt)
    new = m.parameter_list()
    assert m.get_num_points() == int(mask.sum()) == m.contribution_stats.n == m.density_stats.n
    assert not m.contribution_stats.weight_max.any(), "the statistics start over when N changes"
    assert [id(p) for grp in opt.param_groups for p in grp["params"]] == [
        id(q) for q in (new[0], new[1], new[2], new[5], new[3], new[4])]
    assert len(opt.state) == 5 and all(p not in opt.state for p in params)
    for q, v, st0 in zip(new, values, before):
        assert isinstance(q, torch.nn.Parameter) and q.is_contiguous()
        assert torch.equal(q.detach(), v[mask])
        if st0 is None:
            assert q not in opt.state
            continue
        st = opt.state[q]
        assert st["step"] == st0["step"]
        assert torch.equal(st["exp_avg"], st0["exp_avg"][mask]) and st["exp_avg"].is_contiguous()
        assert torch.equal(st["exp_avg_sq"], st0["exp_avg_sq"][mask]) and st["exp_avg_sq"].is_contiguous()


def test_prune_points_without_optimizer_is_unchanged(pkg):
    a, b = _cpu_model(pkg, 7, seed=3), _cpu_model(pkg, 7, seed=3)
    mask = torch.tensor([0, 1, 1, 0, 1, 0, 1], dtype=torch.bool)
    a.prune_points(mask)
    # (what the method did before it took an optimizer)
    exp = [torch.nn.Parameter(p.data[mask].contiguous()) for p in b.parameter_list()]
    for p, q in zip(a.parameter_list(), exp):
        assert isinstance(p, torch.nn.Parameter) and torch.equal(p.detach(), q.detach()) and p.shape == q.shape
    assert a.density_stats.n == 4 and a.xyz_gradient_accum.shape == (4, 3) and a.max_radii2D.shape == (4,)


# --------------------------------------------------------- 5: all_reduce ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_all_reduce_two_gloo_ranks(tmp_path):
    port = _free_port()
    outs = [tmp_path / f"rank{r}.npz" for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "contrib_reduce_worker.py"), str(r), "2", str(port),
                               str(outs[r])]) for r in range(2)]
    try:
        rcs = [p.wait(timeout=120) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0], rcs
    from contrib_reduce_worker import rank_values
    (s0, m0, p0, v0), (s1, m1, p1, v1) = rank_values(0), rank_values(1)
    for o in outs:
        z = np.load(o)
        assert np.array_equal(z["weight_sum"], (s0 + s1).numpy())
        assert np.array_equal(z["weight_max"], torch.maximum(m0, m1).numpy())
        assert np.array_equal(z["pixels"], (p0 + p1).numpy()) and z["pixels"].dtype == np.int64
        assert np.array_equal(z["views"], (v0 + v1).numpy()) and z["views"].dtype == np.int32
