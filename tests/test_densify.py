"""GPU densification (gs_densify_count / gs_densify_emit) against a torch
statement of the semantics in include/gsplat_mi355x.h ("Densification"),
which follow gaussian_model.py:131-197 and optimizer.py:64.  The reference's
own densify cannot run (_append_points reads a missing `_scaling_log`,
gaussian_model.py:229), so this row's parity is pinned to that statement."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def normal_of(seed, i, k):
    h = mix64(seed ^ mix64(i * 4 + k))
    u1 = ((h >> 40) + 1) * 2.0 ** -24
    u2 = ((h >> 16) & 0xFFFFFF) * 2.0 ** -24
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(2 * math.pi * u2)


def _mix64_np(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)  # (uint64 arrays wrap modulo 2^64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def normals_of(seed, n):
    """normal_of(seed, i, k) for i < n, k < 3, as an [n, 3] float64 array."""
    idx = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(4) + np.arange(3, dtype=np.uint64)[None, :]
    h = _mix64_np(np.uint64(seed) ^ _mix64_np(idx))
    u1 = ((h >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)


def test_normals_of_is_normal_of():
    got = normals_of(0x5EED0007, 300)
    assert got.shape == (300, 3)
    assert all(got[i, k] == normal_of(0x5EED0007, i, k) for i in (0, 1, 17, 255, 256, 299) for k in range(3))


def ref_densify(m, grad, th, extent, min_op, seed, masks=False, split=True, clone=True, prune=True):
    """The statement; masks=True also returns (keep, split, clone, hot, s, o)
    over the input Gaussians (the trainer parity test remaps Adam moments
    with them and checks no decision sits on a threshold).  split / clone /
    prune: the GS_DENSIFY_* flags."""
    xyz, fdc, frest, scl, rot, op = [p.detach().cpu().double() for p in m.parameter_list()]
    g = grad.detach().cpu().double()
    n = xyz.shape[0]
    s = scl.exp().mean(-1)
    hot = g.norm(dim=-1) > th
    split = hot & (s > 0.03 * extent) if split else torch.zeros_like(hot)
    clone = hot & (s < 0.01 * extent) if clone else torch.zeros_like(hot)
    o = torch.sigmoid(op[:, 0])
    alive = o > min_op if prune else torch.ones_like(hot)
    child_op = torch.logit(o).clamp(-6, 6)
    child_alive = torch.sigmoid(child_op) > min_op if prune else torch.ones_like(hot)
    keep, sp, cl = ~split & alive, split & child_alive, clone & alive
    q = F.normalize(rot, dim=-1)
    w, x, y, z = q.unbind(-1)
    d = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], -1)
    off = d * (s * 0.5)[:, None]
    jit = torch.from_numpy(normals_of(seed, n))
    rows = {
        "xyz": [xyz[keep], (xyz - off)[sp], (xyz + off)[sp], (xyz + jit * (s * 0.5)[:, None])[cl]],
        "fdc": [fdc[keep], fdc[sp], fdc[sp], fdc[cl]],
        "frest": [frest[keep], frest[sp], frest[sp], frest[cl]],
        "scl": [scl[keep], torch.log(scl.exp() * 0.75)[sp], torch.log(scl.exp() * 0.75)[sp], scl[cl]],
        "rot": [rot[keep], q[sp], q[sp], rot[cl]],
        "op": [op[keep], child_op[sp, None], child_op[sp, None], op[cl]],
    }
    out = {k: torch.cat(v) for k, v in rows.items()}, (int(keep.sum()), int(sp.sum()), int(cl.sum()))
    if masks:
        return out + ((keep, sp, cl, hot, s, o),)
    return out


def _model(pkg, cuda, n=6000, seed=4):
    syn = pkg.synthetic
    sc = syn.make_scene(n, 64, 48, seed=seed, sigma_range=(0.002, 0.05))
    g = torch.Generator().manual_seed(seed)
    sc.opacity[:] = torch.randn(n, 1, generator=g) * 3.0  # some below the 0.01 prune line
    m = syn.to_model(sc, pkg.GaussianModel, cuda)
    m._features_rest.data.normal_(generator=None)
    grad = (torch.randn(n, 3, generator=g) * 3e-4).to(cuda)
    return m, grad


def test_densify_matches_statement(pkg, cuda):
    m, grad = _model(pkg, cuda)
    ext = 1.0
    ref, counts = ref_densify(m, grad, 2e-4, ext, 0.01, 77)
    info = m.densify_and_prune(2e-4, ext, 0.01, seed=77, xyz_grad=grad)
    assert (info["kept"], info["split"], info["cloned"]) == counts
    assert counts[1] > 10 and counts[2] > 10 and info["n"] == counts[0] + 2 * counts[1] + counts[2]
    got = dict(zip(["xyz", "fdc", "frest", "scl", "rot", "op"], [p.detach().cpu().double() for p in m.parameter_list()]))
    for k in ref:
        # children's opacity logit(sigmoid(x)) loses ~1e-5 to fp32 cancellation in 1 - o
        tol = 1e-4 if k == "op" else 1e-5
        err = (got[k] - ref[k]).abs().max().item() if ref[k].numel() else 0.0
        assert err < tol, (k, err)


def test_densify_flags_and_empty(pkg, cuda):
    m, grad = _model(pkg, cuda, n=2000, seed=8)
    n0 = m.get_num_points()
    info = m.densify_and_prune(1e9, 1.0, 0.0, xyz_grad=grad)  # threshold never reached, no prune
    assert info == {"kept": n0, "split": 0, "cloned": 0, "n": n0}
    m.density_and_clone(2e-4, 1.0)  # reference-named wrapper: grad None -> nothing
    assert m.get_num_points() == n0
    m.prune_points(torch.arange(n0, device=cuda) % 2 == 0)
    assert m.get_num_points() == (n0 + 1) // 2


def test_densify_remaps_adam_state(pkg, cuda):
    m, grad = _model(pkg, cuda, n=3000, seed=11)
    opt = pkg.optim.FusedAdam([{"params": [p], "lr": 1e-3} for p in m.parameter_list()])
    for p in m.parameter_list():
        p.grad = torch.randn_like(p) * 1e-3
    opt.step()
    before = {i: (opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
              for i, p in enumerate(m.parameter_list())}
    _, counts = ref_densify(m, grad, 2e-4, 1.0, 0.01, 5)
    xyz_before = m._xyz.detach().clone()
    op = torch.sigmoid(m._opacity.detach()[:, 0])
    s = m._scaling.detach().exp().mean(-1)
    hot = grad.norm(dim=-1) > 2e-4
    keep = ~(hot & (s > 0.03)) & (op > 0.01)
    # the allocator hands freed blocks out again as they are: leave NaN in
    # them, so that a moment row the kernel does not write cannot read as zero
    junk = [torch.full((200_000,), float("nan"), device=cuda) for _ in range(24)]
    junk += [torch.full((n,), float("nan"), device=cuda) for n in (3, 9, 12, 3000, 9000, 12000, 135_000) for _ in range(4)]
    del junk
    info = m.densify_and_prune(2e-4, 1.0, 0.01, optimizer=opt, seed=5, xyz_grad=grad)
    assert info["kept"] == counts[0] == int(keep.sum())
    params = m.parameter_list()
    assert [g["params"][0] for g in opt.param_groups] == params
    for i, p in enumerate(params):
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape
        assert torch.equal(st["exp_avg"][:info["kept"]], before[i][0][keep])
        assert torch.equal(st["exp_avg_sq"][:info["kept"]], before[i][1][keep])
        assert st["exp_avg"][info["kept"]:].abs().max().item() == 0.0 if info["n"] > info["kept"] else True
        # every split and clone row starts from zero moments, both of them (the
        # outputs are torch.empty: only the kernel's own stores make them zero)
        assert st["exp_avg_sq"].shape == p.shape
        assert torch.equal(st["exp_avg"][info["kept"]:], torch.zeros_like(p[info["kept"]:])), i
        assert torch.equal(st["exp_avg_sq"][info["kept"]:], torch.zeros_like(p[info["kept"]:])), i
    assert counts[1] > 10 and counts[2] > 10 and info["n"] == counts[0] + 2 * counts[1] + counts[2]
    assert torch.equal(m._xyz.detach()[:info["kept"]], xyz_before[keep])
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    opt.step()  # the remapped state is usable


# --------------------------------------------------------------------------
# The paths the three tests above never launch: the scan's carry over passes of
# 256 blocks, block-edge sizes, empty categories and an empty output, the flags
# with a real gradient, a model without rest coefficients, saturated opacities.
# --------------------------------------------------------------------------
NAMES = ["xyz", "fdc", "frest", "scl", "rot", "op"]
HOT, LARGE, SMALL = 1e-3, math.log(0.04), math.log(0.005)  # |grad| > 2e-4; scales beyond 0.03 / under 0.01


def _force(m, grad, rows, kind):
    """Make `rows` keep / split / clone candidates at th = 2e-4, extent 1 (opacity well alive)."""
    with torch.no_grad():
        grad[rows] = 0.0
        if kind != "keep":
            grad[rows, 0] = HOT
            m._scaling[rows] = LARGE if kind == "split" else SMALL
        m._opacity[rows] = 2.0


def _make_safe(m, grad, th, extent, min_op):
    """No decision of the fp64 statement within 1e-4 (relative) of its
    threshold: offending rows are nudged (gradient row x 1.01, scaling and
    opacity logit + 0.01), then the condition is asserted on the final inputs."""
    def near(q, t):
        return (q - t).abs() <= 1e-4 * abs(t)

    def offenders():
        g = grad.double().norm(dim=-1)
        s = m._scaling.detach().double().exp().mean(-1)
        o = torch.sigmoid(m._opacity.detach().double()[:, 0])
        oc = torch.sigmoid(torch.logit(o).clamp(-6, 6))
        return near(g, th), near(s, 0.03 * extent) | near(s, 0.01 * extent), near(o, min_op) | near(oc, min_op)

    bg, bs, bo = offenders()
    with torch.no_grad():
        grad[bg] *= 1.01
        m._scaling[bs] += 0.01
        m._opacity[bo] += 0.01
    assert not any(b.any().item() for b in offenders())
    return int(bg.sum() + bs.sum() + bo.sum())


def _densify_vs_statement(pkg, m, grad, th=2e-4, ext=1.0, min_op=0.01, seed=77, **flags):
    """densify_and_prune against ref_densify: the counts and every output array."""
    _make_safe(m, grad, th, ext, min_op)
    ref, counts, masks = ref_densify(m, grad, th, ext, min_op, seed, masks=True, **flags)
    info = m.densify_and_prune(th, ext, min_op, seed=seed, xyz_grad=grad, **flags)
    assert (info["kept"], info["split"], info["cloned"]) == counts
    assert info["n"] == counts[0] + 2 * counts[1] + counts[2] == m.get_num_points()
    got = dict(zip(NAMES, [p.detach().cpu().double() for p in m.parameter_list()]))
    for k in NAMES:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert not torch.isnan(got[k]).any(), k
        tol = 1e-4 if k == "op" else 1e-5  # (as test_densify_matches_statement)
        err = (got[k] - ref[k]).abs().max().item() if ref[k].numel() else 0.0
        assert err < tol, (k, err)
    return info, counts, masks


def test_scan_carry(pkg, cuda):
    """258 blocks: the scan takes two passes and the second starts from the
    first's totals.  Every category has rows in the first and the last block."""
    n = 65_795
    m, grad = _model(pkg, cuda, n=n, seed=21)
    for base in (0, n - 3):
        for j, kind in enumerate(("keep", "split", "clone")):
            _force(m, grad, [base + j], kind)
    info, counts, (keep, sp, cl, *_) = _densify_vs_statement(pkg, m, grad)
    for mask in (keep, sp, cl):
        assert mask[:256].any() and mask[257 * 256:].any()
        assert mask[:65_536].sum() > 256 and mask.sum() > mask[:65_536].sum()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_edges(pkg, cuda, n):
    m, grad = _model(pkg, cuda, n=n, seed=30 + n)
    _force(m, grad, [n - 1], "split")  # the last thread of the last block emits two rows
    info, counts, _ = _densify_vs_statement(pkg, m, grad)
    assert counts[1] >= 1


@pytest.mark.parametrize("kind", ["split", "clone", "pruned", "keep"])
def test_one_category_only(pkg, cuda, kind):
    """Two of the three categories empty, and nothing at all."""
    n = 700
    m, grad = _model(pkg, cuda, n=n, seed=40)
    _force(m, grad, list(range(n)), "keep" if kind == "pruned" else kind)
    if kind == "pruned":
        with torch.no_grad():
            m._opacity.fill_(-10.0)
            grad[::2, 0] = HOT  # (split candidates too: their children are as dead)
    info, counts, _ = _densify_vs_statement(pkg, m, grad)
    want = {"split": (0, n, 0), "clone": (n, 0, n), "pruned": (0, 0, 0), "keep": (n, 0, 0)}[kind]
    assert counts == want
    if kind == "pruned":
        assert m.get_num_points() == 0 and all(p.shape[0] == 0 for p in m.parameter_list())
        again = m.densify_and_prune(2e-4, 1.0, 0.01, seed=1, xyz_grad=torch.zeros(0, 3, device=cuda))
        assert again == {"kept": 0, "split": 0, "cloned": 0, "n": 0}


@pytest.mark.parametrize("off", ["split", "clone", "prune"])
def test_flags_with_a_gradient(pkg, cuda, off):
    m, grad = _model(pkg, cuda, n=1500, seed=50)
    o = torch.sigmoid(m._opacity.detach()[:, 0])
    info, counts, (keep, sp, cl, hot, s, _) = _densify_vs_statement(pkg, m, grad, **{off: False})
    if off == "split":
        assert counts[1] == 0 and counts[2] > 10 and (hot & (s > 0.03) & keep).sum() > 10  # hot and large, kept whole
    elif off == "clone":
        assert counts[2] == 0 and counts[1] > 10
    else:
        assert counts[1] > 10 and counts[2] > 10 and (keep.to(o.device) & (o < 0.01)).sum() > 10  # faint ones survive
        assert counts[0] == int((~(hot & (s > 0.03))).sum())


def test_no_rest_coefficients(pkg, cuda):
    """rest_floats == 0: features_rest is [n, 0, 3] (a null pointer on both sides)."""
    m, grad = _model(pkg, cuda, n=1500, seed=60)
    m._features_rest = torch.nn.Parameter(torch.empty(1500, 0, 3, device=cuda))
    info, counts, _ = _densify_vs_statement(pkg, m, grad)
    assert min(counts) > 10 and m._features_rest.shape == (info["n"], 0, 3)


def test_saturated_opacity_logits(pkg, cuda):
    """Opacity logits of +-30 and +-100 on split rows: sigmoid saturates to 0
    or 1 in fp32, logit to -inf / +inf, and the children get -6 or 6, no NaN."""
    m, grad = _model(pkg, cuda, n=1500, seed=70)
    rows = list(range(8))
    _force(m, grad, rows, "split")
    vals = [30.0, -30.0, 100.0, -100.0, 30.0, -30.0, 100.0, -100.0]
    with torch.no_grad():
        m._opacity[rows, 0] = torch.tensor(vals, device=cuda)
    # min_opacity under sigmoid(-6): the children of the faint rows stay
    info, counts, (keep, sp, *_) = _densify_vs_statement(pkg, m, grad, min_op=0.001)
    assert sp[:8].all()
    first = int(sp[:8].sum())
    for half in (0, 1):
        child = m._opacity.detach()[info["kept"] + half * info["split"]:][:first, 0].cpu()
        assert torch.equal(child, torch.tensor([6.0 if v > 0 else -6.0 for v in vals]))
