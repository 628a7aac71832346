"""MCMC density control on the GPU: the four kernels against the float64
statements of tests/mcmc_util.py, GaussianModel.relocate_and_grow, the trainer
with densify_criterion = "mcmc", and two data-parallel ranks.  Not in the
reference: the statements are this project's own (include/gsplat_mi355x.h,
"MCMC density control")."""
import dataclasses
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mcmc_util as mu
from scene_util import load_scene, write_scene_files
from test_dp_training_gpu import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N = 600  # two full 256-thread blocks and a partial one


def _i32(a, cuda):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32, device=cuda)


# -- sample ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0x3C3C0000 + 2 * 100, 7])
def test_sample_matches_statement(pkg, cuda, seed):
    rng = np.random.default_rng(11)
    w = rng.integers(1, 1 << 24, 1000).astype(np.int64)
    for lo, hi in ((0, 5), (400, 437), (990, 1000)):  # zero weights at the start, inside and at the end
        w[lo:hi] = 0
    w[700] = 0
    cdf = np.cumsum(w)
    want_idx, want_counts = mu.sample_statement(cdf, 4096, seed)
    idx, counts = pkg.mcmc_sample(torch.from_numpy(cdf).to(cuda), 4096, seed)
    assert idx.dtype == torch.int32 and counts.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert int(counts.sum()) == 4096 and not counts.cpu().numpy()[w == 0].any()


def test_sample_edge_sizes(pkg, cuda):
    # n = 1: every sample is row 0
    idx, counts = pkg.mcmc_sample(torch.tensor([5], dtype=torch.int64, device=cuda), 300, 3)
    assert not idx.any() and counts.tolist() == [300]
    # weights near 2^40: the product h * total needs all 128 bits
    w = np.array([(1 << 40) - 3, (1 << 40) + 12345, (1 << 39) + 1], dtype=np.int64)
    cdf = np.cumsum(w)
    want_idx, want_counts = mu.sample_statement(cdf, 2000, 99)
    idx, counts = pkg.mcmc_sample(torch.from_numpy(cdf).to(cuda), 2000, 99)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert min(want_counts) > 100
    # no samples, and nothing to draw from: the outputs keep their bits
    cdf_dev = torch.from_numpy(cdf).to(cuda)
    idx = torch.full((8,), -7, dtype=torch.int32, device=cuda)
    counts = torch.full((3,), 5, dtype=torch.int32, device=cuda)
    pkg.mcmc_sample(cdf_dev, 0, 1, idx=idx[:0], counts=counts)
    pkg.mcmc_sample(torch.zeros(3, dtype=torch.int64, device=cuda), 8, 1, idx=idx, counts=counts)
    torch.cuda.synchronize()
    assert idx.tolist() == [-7] * 8 and counts.tolist() == [5] * 3


# -- relocate -------------------------------------------------------------------
def _rows(cuda, n, seed, opacity_range=(0.005, 0.99)):
    """Six parameter tensors (gs_model_arrays order) of n rows, opacities uniform in the range."""
    g = torch.Generator().manual_seed(seed)
    o = opacity_range[0] + (opacity_range[1] - opacity_range[0]) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    ps = [torch.randn(n, 3, generator=g), torch.randn(n, 1, 3, generator=g), torch.randn(n, 15, 3, generator=g),
          torch.log(0.005 + 0.05 * torch.rand(n, 3, generator=g)), torch.randn(n, 4, generator=g),
          torch.log(o / (1 - o)).float()]
    return [p.to(cuda).contiguous() for p in ps]


def test_relocate_matches_statement(pkg, cuda):
    params = _rows(cuda, N, 21)
    params[5][4] = 20.0  # sigmoid rounds to 1 in fp32: the statement's clamp to 1 - 2^-24
    g = torch.Generator().manual_seed(22)
    moments = [[torch.randn(p.shape, generator=g).to(cuda) for p in params] for _ in range(2)]
    # 90 destination rows (never sampled), the other rows sampled 300 times: row 3 alone 80 times
    # (its ratio clamps to 51), the saturated row 4 three times
    perm = torch.randperm(N, generator=g).numpy()
    perm = perm[(perm != 3) & (perm != 4)]
    dst = np.sort(perm[:90]).astype(np.int32)
    src_pool = perm[90:]
    idx = np.concatenate([np.full(80, 3), np.full(3, 4),
                          src_pool[torch.randint(0, 120, (217,), generator=g).numpy()]]).astype(np.int32)
    idx = idx[torch.randperm(300, generator=g).numpy()]
    dst_all = np.concatenate([dst, np.arange(N, N + 210)]).astype(np.int32)  # rows past n: appended ones
    counts = np.bincount(idx, minlength=N).astype(np.int32)
    assert counts[3] == 80 and counts[4] == 3 and (counts == 1).any() and (counts[src_pool] > 1).any()

    def grown(t):  # 210 appended rows holding NaN: only the kernel's stores make them finite
        return torch.cat([t, torch.full((210,) + tuple(t.shape[1:]), float("nan"), device=cuda)]).contiguous()
    params = [grown(p) for p in params]
    moments = [[grown(m) for m in ms] for ms in moments]
    before = [p.clone() for p in params]
    m_before = [[m.clone() for m in ms] for ms in moments]
    min_op = 0.005
    want_op, want_sc = mu.relocate_statement(before[5][:, 0].cpu().numpy(), before[3].cpu().numpy(), idx, counts, min_op)
    pkg.mcmc_relocate(params, _i32(idx, cuda), _i32(counts, cuda), _i32(dst_all, cuda), min_op, moments[0], moments[1])
    torch.cuda.synchronize()
    src, d = torch.as_tensor(idx, dtype=torch.long), torch.as_tensor(dst_all, dtype=torch.long)
    # opacity and scale of both rows of every sample: the statement, both sides double rounded once to fp32
    for rows in (src, d):
        got_op = params[5][rows.to(cuda), 0].double().cpu().numpy()
        got_sc = params[3][rows.to(cuda)].double().cpu().numpy()
        err_op, err_sc = np.abs(got_op - want_op), np.abs(got_sc - want_sc)
        print(f"relocate: max |d logit| {err_op.max():.3g}, max |d log-scale| {err_sc.max():.3g}")
        assert (err_op <= 1e-6 + 1e-6 * np.abs(want_op)).all()
        assert (err_sc <= 1e-6 + 1e-6 * np.abs(want_sc)).all()
    # copied fields: the source's bits
    for k in (0, 1, 2, 4):
        assert torch.equal(params[k][d.to(cuda)], before[k][src.to(cuda)]), k
    # rows that are neither sampled nor a destination keep every bit; touched rows' moments are zero
    touched = torch.zeros(N + 210, dtype=torch.bool)
    touched[src] = True
    touched[d] = True
    assert int((~touched).sum()) > 100
    rest = (~touched).to(cuda)
    for k in range(6):
        assert torch.equal(params[k][rest], before[k][rest]), k
        for t in range(2):
            assert torch.equal(moments[t][k][rest], m_before[t][k][rest]), (t, k)
            assert not moments[t][k][touched.to(cuda)].any(), (t, k)


def test_relocate_without_moments_and_rest(pkg, cuda):
    """NULL moment arrays are skipped, and a model without rest coefficients ([n, 0, 3]) has no rest row to copy."""
    params = _rows(cuda, 300, 31, opacity_range=(0.2, 0.9))
    params[2] = torch.empty(300, 0, 3, device=cuda)
    before = [p.clone() for p in params]
    idx, dst = np.array([5, 5, 9], np.int32), np.array([0, 299, 100], np.int32)
    counts = np.bincount(idx, minlength=300).astype(np.int32)
    m_xyz = torch.ones(300, 3, device=cuda)
    pkg.mcmc_relocate(params, _i32(idx, cuda), _i32(counts, cuda), _i32(dst, cuda), 0.005,
                      [m_xyz, None, None, None, None, None], None)
    want_op, want_sc = mu.relocate_statement(before[5][:, 0].cpu().numpy(), before[3].cpu().numpy(), idx, counts, 0.005)
    for j, (s, d) in enumerate(zip(idx, dst)):
        for r in (s, d):
            assert abs(params[5][r, 0].item() - want_op[j]) <= 1e-6 + 1e-6 * abs(want_op[j])
            assert np.abs(params[3][r].cpu().numpy() - want_sc[j]).max() <= 2e-6
        assert torch.equal(params[0][d], before[0][s]) and torch.equal(params[4][d], before[4][s])
    assert sorted(torch.nonzero(m_xyz.sum(1) == 0)[:, 0].tolist()) == [0, 5, 9, 100, 299]


# -- noise ----------------------------------------------------------------------
def _noise_inputs(cuda):
    params = _rows(cuda, N, 41)
    g = torch.Generator().manual_seed(42)
    o = torch.exp(torch.rand(N, 1, generator=g, dtype=torch.float64) * math.log(0.9 / 1e-4) + math.log(1e-4))
    params[5] = torch.log(o / (1 - o)).float().to(cuda)  # opacities 1e-4 .. 0.9, log-uniform
    return params


def test_noise_matches_statement(pkg, cuda):
    params = _noise_inputs(cuda)
    before = [p.clone() for p in params]
    scale, seed = 5e5 * 1.6e-4, 0x401E0000 + 17
    want = mu.noise_statement(*(before[k].cpu().numpy() for k in (0, 3, 4)), before[5][:, 0].cpu().numpy(), scale, seed)
    o = torch.sigmoid(before[5][:, 0].double()).cpu().numpy()
    gate = 1 / (1 + np.exp(-100 * (0.005 - o)))
    assert (gate > 0.4).sum() > 50 and (gate < 1e-6).sum() > 50  # gated and ungated rows both occur
    pkg.mcmc_noise(params[0], params[3], params[4], params[5], scale, seed)
    torch.cuda.synchronize()
    got = (params[0].double() - before[0].double()).cpu().numpy()
    half_ulp = np.spacing(np.abs(before[0].cpu().numpy()).astype(np.float32)).astype(np.float64) / 2
    big = np.abs(want).max()
    err = np.abs(got - want)
    print(f"noise: largest |delta| {big:.3g}, max err {err.max():.3g} ({(err - half_ulp).max() / big:.3g} of it)")
    assert big > 0 and (err <= 1e-4 * big + half_ulp).all()
    for k in (1, 2, 3, 4, 5):
        assert torch.equal(params[k], before[k]), k
    # the same seed: the same bits; another seed: other noise
    again = [p.clone() for p in before]
    pkg.mcmc_noise(again[0], again[3], again[4], again[5], scale, seed)
    other = [p.clone() for p in before]
    pkg.mcmc_noise(other[0], other[3], other[4], other[5], scale, seed + 1)
    assert torch.equal(again[0], params[0]) and not torch.equal(other[0], params[0])
    # scale 0 and n = 0: nothing is launched
    pkg.mcmc_noise(again[0], again[3], again[4], again[5], 0.0, seed)
    pkg.mcmc_noise(*(t[:0] for t in (again[0], again[3], again[4], again[5])), scale, seed)
    assert torch.equal(again[0], params[0])


# -- regularize -----------------------------------------------------------------
def test_regularize_matches_autograd(pkg, cuda):
    params = _noise_inputs(cuda)
    g = torch.Generator().manual_seed(51)
    d_op = (torch.randn(N, 1, generator=g) * 1e-6).to(cuda)
    d_sc = (torch.randn(N, 3, generator=g) * 1e-6).to(cuda)
    d_op0, d_sc0 = d_op.clone(), d_sc.clone()
    lam_o, lam_s = 0.01, 0.02
    want_op, want_sc = mu.regularizer_grads(params[5], params[3], lam_o, lam_s)
    pkg.mcmc_regularize(params[5], params[3], d_op, d_sc, lam_o, lam_s)
    for got, base, want in ((d_op, d_op0, want_op), (d_sc, d_sc0, want_sc)):
        total = base.double().cpu() + want
        err = (got.double().cpu() - total).abs()
        tol = 1e-5 * torch.maximum(total.abs(), total.abs().max())
        print(f"regularize: max err {err.max():.3g}, largest value {total.abs().max():.3g}")
        assert (err <= tol).all() and want.abs().max() > 0
    # a NULL gradient skips its term and leaves the other as it would be
    only = d_sc0.clone()
    pkg.mcmc_regularize(params[5], params[3], None, only, lam_o, lam_s)
    assert torch.equal(only, d_sc)
    only = d_op0.clone()
    pkg.mcmc_regularize(params[5], params[3], only, None, lam_o, lam_s)
    assert torch.equal(only, d_op)


# -- model ----------------------------------------------------------------------
def test_model_relocates_and_grows_to_the_cap(pkg, cuda):
    n0, cap, min_op = 2000, 2400, 0.005
    m = pkg.GaussianModel()
    m._set(*_rows(cuda, n0, 61, opacity_range=(0.5, 0.9)))
    opt = pkg.optim.FusedAdam([{"params": [p], "lr": 1e-3} for p in m.parameter_list()])

    def step():
        for p in m.parameter_list():
            p.grad = torch.randn_like(p) * 1e-3
        opt.step()

    def kill(rows):
        with torch.no_grad():
            m._opacity[rows] = -8.0  # sigmoid 3.4e-4: dead

    def dead():
        return int((torch.sigmoid(m._opacity.detach()) <= min_op).sum())

    step()
    sizes = []
    for call, want_n in enumerate((2100, 2205, 2315, 2400, 2400)):
        kill(torch.arange(0, m.get_num_points(), 13, device=cuda))
        n_dead, n_before = dead(), m.get_num_points()
        assert n_dead > 100
        ptrs = [p.data_ptr() for p in m.parameter_list()] + \
               [opt.state[p][k].data_ptr() for p in m.parameter_list() for k in ("exp_avg", "exp_avg_sq")]
        info = m.relocate_and_grow(cap, min_op, 0x3C3C0000 + 2 * call, optimizer=opt)
        assert info == {"n_before": n_before, "relocated": n_dead, "added": want_n - n_before, "n": want_n}
        assert m.get_num_points() == want_n and dead() == 0
        sizes.append(info["n"])
        now = [p.data_ptr() for p in m.parameter_list()] + \
              [opt.state[p][k].data_ptr() for p in m.parameter_list() for k in ("exp_avg", "exp_avg_sq")]
        if info["added"] == 0:  # at the cap: relocation in place, nothing moves
            assert now == ptrs
        for p in m.parameter_list():
            assert p.shape[0] == want_n and torch.isfinite(p).all()
            st = opt.state[p]
            assert st["step"] == call + 1 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert [g["params"][0] for g in opt.param_groups] == m.parameter_list()
        step()  # the optimizer keeps stepping
    assert sizes == [2100, 2205, 2315, 2400, 2400]
    # nothing dead and at the cap: nothing happens at all
    before = [p.detach().clone() for p in m.parameter_list()]
    assert m.relocate_and_grow(cap, min_op, 1, optimizer=opt) == {"n_before": 2400, "relocated": 0, "added": 0, "n": 2400}
    assert all(torch.equal(a, b) for a, b in zip(before, m.parameter_list()))
    # every row dead: nothing to draw from, nothing changes
    kill(slice(None))
    assert m.relocate_and_grow(3000, min_op, 2, optimizer=opt)["n"] == 2400


# -- trainer --------------------------------------------------------------------
def _mcmc_config(pkg, out, **kw):
    base = dict(iterations=300, densify_from_iter=50, densify_until_iter=300, densify_interval=50,
                num_random_points=2000, log_interval=1, output_path=str(out), position_lr_init=1.6e-3,
                position_lr_final=1.6e-5, densify_criterion="mcmc", mcmc_cap_max=2400, mcmc_noise_lr=5e4)
    base.update(kw)
    return pkg.TrainingConfig(**base)


@pytest.fixture(scope="module")
def scene(pkg, cuda, tmp_path_factory):
    root = tmp_path_factory.mktemp("mcmc_scene")
    write_scene_files(root, 12, 64)
    return root, load_scene(pkg, root, cuda, 64, split=False)


def _run(pkg, cfg, ds, iterations, watch=None):
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    for _ in range(iterations):
        tr.train(1)
        if watch is not None:
            watch(tr)
    torch.cuda.synchronize()
    return tr


def test_trainer_mcmc(pkg, cuda, scene):
    root, ds = scene
    cfg = _mcmc_config(pkg, root / "out")
    sizes, infos = [], []

    def watch(tr):
        sizes.append(tr.gaussians.get_num_points())
        if tr.iteration % 50 == 0:
            infos.append(dict(tr.last_densify))

    tr = _run(pkg, cfg, ds, 300, watch)
    assert max(sizes) <= 2400 and sizes[-1] == 2400 and sizes[48] == 2000 and sizes[49] == 2100
    assert [i["n"] for i in infos] == [2100, 2205, 2315, 2400, 2400, 2400]
    assert sum(i["relocated"] for i in infos) > 0, "the run must hold a relocation"
    for p in tr.gaussians.parameter_list():
        assert torch.isfinite(p).all()
    first, last = np.mean(tr.train_losses[:12]), np.mean(tr.train_losses[-12:])  # (one round of the 12 views each)
    print(f"mcmc trainer: loss {first:.4f} -> {last:.4f}; relocated {[i['relocated'] for i in infos]}")
    assert len(tr.train_losses) == 300 and last < first and tr.train_losses[-1] < tr.train_losses[0]
    # a second run: the same bits
    again = _run(pkg, _mcmc_config(pkg, root / "out2"), ds, 300)
    for a, b in zip(tr.gaussians.parameter_list(), again.gaussians.parameter_list()):
        assert torch.equal(a, b)
    assert again.train_losses == tr.train_losses


def test_other_criteria_do_not_read_the_mcmc_fields(pkg, cuda, scene):
    root, ds = scene
    cfg = pkg.TrainingConfig(iterations=110, densify_from_iter=100, densify_until_iter=110, densify_interval=100,
                             num_random_points=2000, log_interval=10, output_path=str(root / "s1"),
                             position_lr_init=1.6e-3, position_lr_final=1.6e-5, densify_criterion="screen",
                             densify_grad_threshold=1e-7)  # (every Gaussian a view saw is hot)
    a = _run(pkg, cfg, ds, 110)
    b = _run(pkg, dataclasses.replace(cfg, output_path=str(root / "s2"), mcmc_cap_max=7, mcmc_min_opacity=0.5,
                                      mcmc_noise_lr=1e9, mcmc_opacity_reg=3.0, mcmc_scale_reg=5.0,
                                      mcmc_grow_factor=2.0), ds, 110)
    assert a.last_densify is not None and a.last_densify["n"] != 2000
    assert a.last_densify == b.last_densify and a.train_losses == b.train_losses
    for p, q in zip(a.gaussians.parameter_list(), b.gaussians.parameter_list()):
        assert torch.equal(p, q)


# -- two gloo ranks on one GPU --------------------------------------------------
def test_dp_two_ranks_stay_bit_identical(pkg, cuda, tmp_path):
    write_scene_files(tmp_path)
    port = _free_port()
    outs = [tmp_path / f"rank{r}.npz" for r in range(2)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", GS_ALLREDUCE_CHUNKS="2", GS_ALLREDUCE_MIN_ROWS="256")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_mcmc_worker.py"), str(r), "2", str(port),
                               str(tmp_path), str(outs[r])], env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0], rcs
    a, b = (np.load(o) for o in outs)
    print(f"DP mcmc: relocated {int(a['relocated'])}, added {int(a['added'])}, n {int(a['n'])}")
    assert int(a["iteration"]) == 4 and int(a["n"]) == int(b["n"]) == 3100
    assert int(a["relocated"]) == int(b["relocated"]) > 0 and int(a["added"]) == int(b["added"]) == 100
    for i in range(6):
        assert np.array_equal(a[f"p{i}"], b[f"p{i}"]), f"replicas diverged in parameter {i}"
        assert np.array_equal(a[f"m{i}"], b[f"m{i}"]), f"replicas diverged in the moments of parameter {i}"
