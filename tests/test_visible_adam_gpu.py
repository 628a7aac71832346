"""Visibility-gated Adam (gs_adam_step_rows, FusedAdam.step(visible=), the
trainer's visible_adam) on the GPU.

The yardstick is the dense step, not the new kernel: for identical inputs,
with after = gs_adam_step(before), the masked step must leave exactly
where(mask[:, None], after, before) in p, exp_avg and exp_avg_sq -- compared
with torch.equal.  Adam is elementwise and both kernels inline the same
adam_update, so nothing but bit identity is acceptable; and a masked row's
gradient (NaN and Inf on the second step) must reach nothing.

The fp64 check ties the rule to its definition as well: torch.optim.Adam on
the visible rows alone, against the fp64 statement of tests/test_adam.py,
under that file's bound (4x torch's own fp32 error plus 2 ulp of the largest
magnitude)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from scene_util import load_scene, write_scene_files
from test_adam import Adam64, _ulp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
COLS = (3, 3, 1, 2, 3, 4, 45)  # the model's tensors, and a gradient-less one (index 3) in the middle of the table
NOGRAD = 3


def _masks(rows, R, gen):
    """name -> [rows] bool (CPU), the cases that exist at this row count."""
    out = {"zeros": torch.zeros(rows, dtype=torch.bool), "ones": torch.ones(rows, dtype=torch.bool),
           "random30": torch.rand(rows, generator=gen) < 0.3, "alternating": torch.arange(rows) % 2 == 0}
    for r in sorted({0, R - 1, R, rows - 1}):
        if 0 <= r < rows:
            m = torch.zeros(rows, dtype=torch.bool)
            m[r] = True
            out[f"single{r}"] = m
    if rows >= 3 * R:
        m = torch.zeros(rows, dtype=torch.bool)
        m[R:2 * R] = True
        out["one_block"] = m
    return out


def _at_offset(t, off):
    """A copy of the flat tensor t that starts `off` floats into its buffer."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = buf[off:off + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view


def _call(pkg, tensors, grads, t, rows=None, mask=None):
    """gs_adam_step (mask None) or gs_adam_step_rows over `tensors` = [(p, m, v)], step count t."""
    N = pkg._native
    b1, b2 = HYPER["betas"]
    rows_args = N.GsAdamRowsArgs() if mask is not None else None
    a = rows_args.adam if mask is not None else N.GsAdamArgs()
    a.num_tensors, a.beta1, a.beta2, a.eps = len(tensors), b1, b2, HYPER["eps"]
    a.one_minus_beta1, a.one_minus_beta2 = 1.0 - b1, 1.0 - b2
    for k, ((p, m, v), g) in enumerate(zip(tensors, grads)):
        a.t[k] = N.GsAdamTensor(N.ptr(p), N.ptr(m), N.ptr(v), N.ptr(g) or None, p.numel(), HYPER["lr"] * (k + 1),
                                1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5, None)
    if mask is None:
        N.check(N.load().gs_adam_step(C.byref(a), N.stream_ptr()), "gs_adam_step")
        return
    rows_args.rows, rows_args.row_mask = rows, N.ptr(mask)
    for k, c in enumerate(COLS):
        rows_args.cols[k] = c
    N.check(N.load().gs_adam_step_rows(C.byref(rows_args), N.stream_ptr()), "gs_adam_step_rows")


def _expect(mask, cols, after, before):
    return torch.where(mask.repeat_interleave(cols), after, before)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))  # (NaN-proof, and -0.0 is not +0.0)


@pytest.mark.parametrize("offset", [0, 1, 3], ids=["aligned", "offset4B", "offset12B"])
@pytest.mark.parametrize("rows_of", [lambda R: 1, lambda R: R - 1, lambda R: R, lambda R: R + 1, lambda R: 4 * R + 3],
                         ids=["1", "R-1", "R", "R+1", "4R+3"])
def test_kernel_against_the_dense_step(pkg, cuda, rows_of, offset):
    """Two consecutive steps per mask; on the second the moments are non-zero
    and the masked rows' gradients are NaN and Inf.  offset: every tensor of
    the masked step starts 4 / 12 bytes into its buffer (the scalar path)."""
    R = pkg._native.GS_ADAM_ROW_BLOCK
    rows = rows_of(R)
    gen = torch.Generator().manual_seed(100 + rows)
    rnd = lambda c, f=torch.randn: f(rows * c, generator=gen).to(cuda)
    init = [(rnd(c), 0.1 * rnd(c), 0.01 * rnd(c, torch.rand)) for c in COLS]
    g1 = [rnd(c) for c in COLS]
    g2 = [rnd(c) for c in COLS]
    for name, mask_cpu in _masks(rows, R, gen).items():
        mask = mask_cpu.to(cuda)
        mask_u8 = mask.to(torch.uint8) * 7 if name == "random30" else mask  # (any non-zero byte marks a row)
        dense = [tuple(x.clone() for x in t) for t in init]
        ours = [tuple(_at_offset(x, offset) for x in t) for t in init]
        for t, grads in ((1, g1), (2, g2)):
            grads = [g.clone() for g in grads]
            if t == 2:
                for g, c in zip(grads, COLS):
                    hidden = ~mask.repeat_interleave(c)
                    poison = torch.tensor([float("nan"), float("inf"), -float("inf")], device=cuda)
                    g[hidden] = poison[torch.arange(int(hidden.sum()), device=cuda) % 3]
            grads[NOGRAD] = None
            before = [tuple(x.clone() for x in t3) for t3 in ours]
            for d, o in zip(dense, ours):  # identical inputs
                for x, y in zip(d, o):
                    x.copy_(y)
            _call(pkg, dense, grads, t)
            _call(pkg, ours, [None if g is None else _at_offset(g, offset) for g in grads], t, rows, mask_u8)
            for k, c in enumerate(COLS):
                for q, (after, got, was) in enumerate(zip(dense[k], ours[k], before[k])):
                    want = was if k == NOGRAD else _expect(mask, c, after, was)
                    assert _bits_equal(got, want), (name, rows, offset, "step", t, "tensor", k, "pmv"[q])
        if name == "ones":  # (the yardstick moved: the comparison is not vacuous)
            assert not torch.equal(ours[0][0], init[0][0])


def test_visible_rows_against_fp64(pkg, cuda):
    """Six masked steps: the visible rows within tests/test_adam.py's bound of
    the fp64 statement, torch.optim.Adam stepping the visible rows alone; the
    other rows as they started."""
    R = pkg._native.GS_ADAM_ROW_BLOCK
    rows, cols = 2 * R + 37, (3, 3, 1, 3, 4, 45)
    gen = torch.Generator().manual_seed(7)
    mask = (torch.rand(rows, generator=gen) < 0.3).to(cuda)
    a = [torch.randn(rows, c, generator=gen).to(cuda).requires_grad_() for c in cols]
    start = [t.detach().clone() for t in a]
    b = [t.detach()[mask].clone().requires_grad_() for t in a]
    oa, ob = pkg.optim.FusedAdam(a, **HYPER), torch.optim.Adam(b, **HYPER)
    ref = Adam64(b, [HYPER] * len(cols))
    for _ in range(6):
        grads = [torch.randn(rows, c, generator=gen).to(cuda) for c in cols]
        for x, y, g in zip(a, b, grads):
            x.grad, y.grad = g.clone(), g[mask].clone()
        oa.step(visible=mask)
        ob.step()
        ref.step([g[mask] for g in grads])
    bad = []
    for i, c in enumerate(cols):
        sa, sb = oa.state[a[i]], ob.state[b[i]]
        assert sa["step"] == 6
        for name, fa, fb, r, was in (("p", a[i].detach(), b[i].detach(), ref.p[i], start[i]),
                                     ("exp_avg", sa["exp_avg"], sb["exp_avg"], ref.m[i], torch.zeros_like(start[i])),
                                     ("exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"], ref.v[i],
                                      torch.zeros_like(start[i]))):
            assert _bits_equal(fa[~mask], was[~mask]), (i, name)
            ea = (fa[mask].double() - r).abs().max().item()
            eb = (fb.double() - r).abs().max().item()
            bound = 4 * eb + 2 * _ulp(r.abs().max().item())
            print(f"visible adam tensor {i} cols {c} {name}: fused {ea:.3e} torch {eb:.3e} bound {bound:.3e}")
            assert np.isfinite(ea)
            if not ea <= bound:
                bad.append((i, name, ea, eb, bound))
    assert not bad, bad


def _state(params, opt):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]


def test_fused_adam_step_and_step_ranges(pkg, cuda):
    """step(visible=) and step_ranges(unaligned ranges, visible=) leave the same
    where(...) of the dense step; a dense step after a masked one continues
    from that state bit for bit."""
    R = pkg._native.GS_ADAM_ROW_BLOCK
    rows, shapes = 2 * R + 5, [(3,), (1, 3), (1,), (4,), (15, 3)]
    ranges = [(0, 5), (5, 5), (5, R + 2), (R + 2, rows)]
    gen = torch.Generator().manual_seed(11)
    mask = (torch.rand(rows, generator=gen) < 0.4).to(cuda)
    init = [torch.randn((rows,) + s, generator=gen).to(cuda) for s in shapes]
    sets = [[t.clone().requires_grad_() for t in init] for _ in range(3)]
    groups = lambda ps: [dict(HYPER, params=ps[:3]), dict(HYPER, lr=5e-3, params=ps[3:])]
    dense, by_step, by_ranges = (pkg.optim.FusedAdam(groups(ps)) for ps in sets)

    def give(grads):
        for ps in sets:
            for p, g in zip(ps, grads):
                p.grad = g.clone()

    for it in range(2):  # (the second masked step has moments behind it)
        before = _state(sets[0], dense) if it else [(t, torch.zeros_like(t), torch.zeros_like(t)) for t in init]
        give([torch.randn((rows,) + s, generator=gen).to(cuda) for s in shapes])
        dense.step()
        by_step.step(visible=mask)
        by_ranges.step_ranges(ranges, visible=mask.to(torch.uint8))
        want = [tuple(torch.where(mask.view((rows,) + (1,) * (x.dim() - 1)), x, y) for x, y in zip(after, was))
                for after, was in zip(_state(sets[0], dense), before)]
        for ps, opt in ((sets[1], by_step), (sets[2], by_ranges)):
            for got, w in zip(_state(ps, opt), want):
                assert all(_bits_equal(x, y) for x, y in zip(got, w))
        # the dense optimizer continues from the masked state
        with torch.no_grad():
            for p, (wp, wm, wv) in zip(sets[0], want):
                p.copy_(wp)
                dense.state[p]["exp_avg"].copy_(wm)
                dense.state[p]["exp_avg_sq"].copy_(wv)
    give([torch.randn((rows,) + s, generator=gen).to(cuda) for s in shapes])
    dense.step()
    by_step.step()  # visible=None after masked steps: the dense step, cached plan and all
    by_ranges.step_ranges(ranges)
    want = _state(sets[0], dense)
    for ps, opt in ((sets[1], by_step), (sets[2], by_ranges)):
        assert all(opt.state[p]["step"] == 3 for p in ps)
        for got, w in zip(_state(ps, opt), want):
            assert all(_bits_equal(x, y) for x, y in zip(got, w))


# -- trainer --------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(pkg, cuda, tmp_path_factory):
    root = tmp_path_factory.mktemp("visible_scene")
    write_scene_files(root, 12, 64)
    return root, load_scene(pkg, root, cuda, 64, split=False)


def _wide_model_tensors(cam_b, cuda):
    """300 Gaussians in the ball every camera looks at, and 100 on camera B's
    axis, 1.2 to 1.8 in front of it: far outside the frustum of a camera a
    quarter turn away."""
    gen = torch.Generator().manual_seed(21)
    d = torch.randn(300, 3, generator=gen)
    ball = d / d.norm(dim=1, keepdim=True) * 0.7 * torch.rand(300, 1, generator=gen) ** (1 / 3)
    centre = cam_b.camera_center.detach().cpu().float()
    axis = centre / centre.norm()  # (the cameras look at the origin)
    side = axis[None] * (2.2 + 0.6 * torch.rand(100, 1, generator=gen)) + 0.1 * torch.randn(100, 3, generator=gen)
    xyz = torch.cat([ball, side])
    n = xyz.shape[0]
    return [t.to(cuda) for t in (xyz, torch.rand(n, 1, 3, generator=gen), torch.zeros(n, 15, 3),
                                 torch.log(0.03 + 0.04 * torch.rand(n, 3, generator=gen)),
                                 torch.nn.functional.normalize(torch.randn(n, 4, generator=gen), dim=-1),
                                 torch.full((n, 1), 0.5))]


def _trainer(pkg, cfg, ds, tensors):
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    tr.gaussians._set(*[t.clone() for t in tensors])
    tr.optimizer = pkg.optim.GaussianOptimizer(tr.gaussians, cfg)
    tr.optimizer.setup_optimizer()
    return tr


def _snapshot(tr):
    out, opt = [], tr.optimizer.optimizer
    for p in tr.gaussians.parameter_list():
        st = opt.state.get(p, {})
        out.append((p.detach().clone(), st["exp_avg"].clone() if st else torch.zeros_like(p),
                    st["exp_avg_sq"].clone() if st else torch.zeros_like(p), st.get("step", 0)))
    return out


@pytest.mark.parametrize("criterion", ["xyz_grad", "mcmc"])
def test_trainer_hidden_rows_keep_their_bits(pkg, cuda, scene, criterion):
    """One step on camera B gives the Gaussians in front of it moments; the
    next step is on camera A, which does not see them.  With visible_adam they
    keep every bit; without it they move along the stale first moment.  The
    rows A sees equal an independently composed step (this render and loss,
    backward, [the MCMC regularisers,] the dense FusedAdam on a clone)."""
    root, ds = scene
    cams = ds.get_train_cameras()
    cam_a, cam_b = cams[0], cams[3]
    tensors = _wide_model_tensors(cam_b, cuda)
    n = tensors[0].shape[0]
    kw = dict(iterations=100, num_random_points=400, densify_from_iter=10_000, densify_until_iter=10_000, log_interval=1,
              position_lr_init=1.6e-3, position_lr_final=1.6e-5, densify_criterion=criterion)
    if criterion == "mcmc":
        kw.update(mcmc_cap_max=n, mcmc_noise_lr=0.0)  # (the position noise is not gated: off, to see the step alone)
    runs = {}
    for on in (True, False):
        cfg = pkg.TrainingConfig(output_path=str(root / f"{criterion}{int(on)}"), visible_adam=on, **kw)
        tr = _trainer(pkg, cfg, ds, tensors)
        tr.iteration = 1
        tr.train_step(cam_b)
        mid = _snapshot(tr)
        # the composed step, on clones of the state in between
        model = pkg.GaussianModel(cfg)
        model._set(*[p.clone() for p, _, _, _ in mid])
        opt = pkg.optim.GaussianOptimizer(model, cfg)
        opt.setup_optimizer()
        for p, (_, m, v, t) in zip(model.parameter_list(), mid):
            if t:
                opt.optimizer.state[p] = {"step": t, "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        out = pkg.GaussianRenderer().render(cam_a, model, tr._settings(cam_a))
        vis_a = out["visibility_filter"].clone()
        total = pkg.loss.photometric_loss(out["image"], cam_a._image, cfg.lambda_dssim)[0]
        total.backward()
        opt.update_learning_rate(2)
        if criterion == "mcmc":
            opt.mcmc_regularize()
        opt.step()
        composed = [(p.detach(), opt.optimizer.state[p]["exp_avg"], opt.optimizer.state[p]["exp_avg_sq"])
                    if opt.optimizer.state.get(p) else (p.detach(), m, v)
                    for p, (_, m, v, _) in zip(model.parameter_list(), mid)]
        with torch.no_grad():
            vis_b = pkg.GaussianRenderer().render(cam_b, model, tr._settings(cam_b))["visibility_filter"].clone()
        tr.iteration = 2
        tr.train_step(cam_a)
        torch.cuda.synchronize()
        runs[on] = (mid, _snapshot(tr), composed, vis_a, vis_b)

    mid, end, composed, vis_a, _ = runs[True]
    hidden = ~vis_a
    had_moments = (mid[0][1][hidden] != 0).any(1)  # xyz rows hidden from A that B's step reached
    print(f"visible adam trainer ({criterion}): {n} Gaussians, A sees {int(vis_a.sum())}, hidden {int(hidden.sum())}, "
          f"of which {int(had_moments.sum())} carry moments from B's step")
    assert int(hidden.sum()) >= 100 and int(vis_a.sum()) >= 100 and int(had_moments.sum()) >= 20
    for (p0, m0, v0, t0), (p1, m1, v1, t1), (pc, mc, vc) in zip(mid, end, composed):
        assert t1 == t0 + 1 if t0 else t1 in (0, 1)  # (the step count is the tensor's, not a row's)
        sel = vis_a.view((n,) + (1,) * (p0.dim() - 1))
        for got, was, dense in ((p1, p0, pc), (m1, m0, mc), (v1, v0, vc)):
            assert _bits_equal(got[hidden], was[hidden]), "a row hidden from the step's view changed"
            assert _bits_equal(got, torch.where(sel, dense, was)), "a visible row differs from the composed dense step"
    assert not torch.equal(end[0][0][vis_a], mid[0][0][vis_a]), "the visible rows must move"

    # the behaviour the option is for: the dense step moves what the view does not see
    mid, end, composed, vis_a2, _ = runs[False]
    assert torch.equal(vis_a2, vis_a)
    moved = (end[0][0][hidden] != mid[0][0][hidden]).any(1)
    assert torch.equal(moved, had_moments) or int((moved & had_moments).sum()) >= 20
    assert not _bits_equal(end[0][1][hidden], mid[0][1][hidden]), "the dense step decays the hidden rows' moments"
    for (p1, m1, v1, _), (pc, mc, vc) in zip(end, composed):  # (and is the composed step on every row)
        assert _bits_equal(p1, pc) and _bits_equal(m1, mc) and _bits_equal(v1, vc)


# -- two gloo ranks on one GPU --------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_dp_two_ranks_step_the_union(pkg, cuda, tmp_path):
    """Every rank renders another camera; the step's mask is the union of the
    ranks' visibility.  Three steps: the replicas end bit-identical, a row
    neither rank saw is untouched, and a row one rank alone saw (and the
    averaged gradient reached) is updated on both."""
    write_scene_files(tmp_path)
    port = _free_port()
    outs = [tmp_path / f"rank{r}.npz" for r in range(2)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", GS_ALLREDUCE_CHUNKS="2", GS_ALLREDUCE_MIN_ROWS="256")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_visible_adam_worker.py"), str(r), "2", str(port),
                               str(tmp_path), str(outs[r])], env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0], rcs
    a, b = (np.load(o) for o in outs)
    assert int(a["iteration"]) == int(b["iteration"]) == 3
    assert int(a["ranges"]) == 6, "the pipelined path: two ranges a step"
    for i in range(6):
        assert np.array_equal(a[f"p{i}"], b[f"p{i}"]), f"replicas diverged in parameter {i}"
        if f"m{i}" in a:
            assert np.array_equal(a[f"m{i}"], b[f"m{i}"]) and np.array_equal(a[f"v{i}"], b[f"v{i}"]), i
            assert int(a[f"t{i}"]) == int(b[f"t{i}"]) == 3
    for step in range(3):
        va, vb = a[f"vis{step}"], b[f"vis{step}"]
        union, one = va | vb, va ^ vb
        reached = a[f"reached{step}"]
        assert np.array_equal(reached, b[f"reached{step}"])
        print(f"DP visible adam step {step}: rank 0 sees {va.sum()}, rank 1 {vb.sum()}, union {union.sum()} of "
              f"{union.size}, one rank alone {one.sum()}, of which the gradient reached {(one & reached).sum()}")
        assert (~union).sum() >= 100 and (one & reached).sum() >= 100 and not np.array_equal(va, vb)
        for rec in (a, b):
            changed = rec[f"changed{step}"]
            assert not changed[~union].any(), "a row no rank saw changed"
            assert changed[union & reached].all(), "a row a rank saw, with a gradient, was not updated"
