"""FusedAdam (gs_adam_step, k_adam) against an fp64 statement of
torch.optim.Adam (default flags), stepped alongside:

    m += (1 - b1) (g - m);  v = b2 v + (1 - b2) g^2
    p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps),  bc = 1 - beta^t

The yardstick is torch.optim.Adam in fp32 on the same device and inputs: per
tensor and per quantity (p, exp_avg, exp_avg_sq), FusedAdam's max abs error
against fp64 may be at most 4x torch's plus 2 ulp (fp32) of the largest
magnitude in that tensor.  The kernel and torch perform the same fp32
operations in possibly different association (factor 4); an error that grows
with the value is not covered.

The cases reach what the one older comparison (tensors of 1000..4000 floats)
does not: the full-chunk float4 branch (numel >= 4096), the tail after whole
chunks, the unaligned scalar branch (step_ranges at byte offsets 4 and 12), a
grad == NULL tensor in the middle of the block table, more than 8 tensors in a
batch, several (betas, eps) batches, and param_out over whole chunks.

Measured on an MI355X, max abs error against fp64 after 6 steps (FusedAdam /
torch.optim.Adam fp32):

  case                     p                  exp_avg            exp_avg_sq
  (a) 8 tensors, randn     5.3e-07 / 5.3e-07  7.5e-09 / 2.0e-09  6.1e-09 / 4.2e-09
  (b) 10 tensors, 3 groups 5.0e-07 / 5.0e-07  7.7e-08 / 6.7e-08  5.1e-09 / 5.1e-09
  (b) 9 tensors, 1 group   5.1e-07 / 5.1e-07  9.1e-08 / 5.9e-08  5.3e-09 / 4.9e-09
  (c) wide gradients       5.6e-07 / 5.6e-07  1.2e-05 / 1.0e-05  2.9e-04 / 2.9e-04
  (d) step_ranges          6.0e-07 / 6.0e-07  7.3e-08 / 6.5e-08  5.5e-09 / 5.5e-09

(the tensor and quantity of each case that came closest to its bound; the
largest magnitudes are ~4 for p, ~1 for the moments, 1e3 and 1e6 in (c)).

Before gs_adam_args carried 1 - beta formed in double, the kernel formed
1.f - (float)0.999 = 0.99998713e-3 itself and exp_avg_sq sat 1.29e-5 (relative)
under the fp64 statement (3.5e-7 where torch has 4e-9..6e-9 and the bound is
2e-8..3e-8): cases (a)-(d) failed on it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 6
DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


def _randn(shape, gen):
    return torch.randn(shape, generator=gen)


def _wide(shape, gen):
    """Exact zeros in a tenth of the entries, the rest log-uniform in
    1e-12..1e3 with random sign (g^2 >= 1e-24: clear of fp32 denormals)."""
    mag = torch.pow(10.0, torch.rand(shape, generator=gen, dtype=torch.float64) * 15 - 12).float()
    g = torch.where(torch.rand(shape, generator=gen) < 0.5, -mag, mag)
    g[torch.rand(shape, generator=gen) < 0.1] = 0.0
    return g


class Adam64:
    """The fp64 statement, one state per tensor; hyper-parameters as Python doubles."""

    def __init__(self, params, hypers):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(params)
        self.h = hypers

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.double()
            h = self.h[i]
            (b1, b2), lr, eps = h["betas"], h["lr"], h["eps"]
            self.t[i] += 1
            bc1, bc2 = 1 - b1 ** self.t[i], 1 - b2 ** self.t[i]
            self.m[i] += (1 - b1) * (g - self.m[i])
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            self.p[i] -= lr / bc1 * self.m[i] / (self.v[i].sqrt() / bc2 ** 0.5 + eps)


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _setup(pkg, cuda, shapes, groups, seed):
    """groups: [(tensor indices, hyper-parameter overrides)].  Returns the
    fused / torch parameter lists and optimizers and the fp64 statement."""
    gen = torch.Generator().manual_seed(seed)
    a = [torch.randn(s, generator=gen).to(cuda).requires_grad_() for s in shapes]
    b = [t.detach().clone().requires_grad_() for t in a]
    hypers = [None] * len(shapes)
    ga, gb = [], []
    for idx, over in groups:
        h = dict(DEFAULTS, **over)
        for i in idx:
            hypers[i] = h
        ga.append(dict(h, params=[a[i] for i in idx]))
        gb.append(dict(h, params=[b[i] for i in idx]))
    assert all(h is not None for h in hypers)
    return gen, a, b, pkg.optim.FusedAdam(ga), torch.optim.Adam(gb), Adam64(a, hypers)


def _advance(gen, cuda, shapes, a, b, ref, grad_fn, nograd, step_a, step_b):
    for _ in range(STEPS):
        grads = []
        for i, s in enumerate(shapes):
            if i in nograd:
                a[i].grad = b[i].grad = None
                grads.append(None)
                continue
            g = grad_fn(s, gen).to(cuda)
            a[i].grad, b[i].grad = g.clone(), g.clone()
            grads.append(g)
        step_a()
        step_b()
        ref.step(grads)


def _compare(case, shapes, a, oa, b, ob, ref, nograd=()):
    """Print every figure, then hold FusedAdam to 4x torch's error + 2 ulp."""
    bad = []
    for i, s in enumerate(shapes):
        if i in nograd:
            assert not oa.state[a[i]] and torch.equal(a[i].detach().double(), ref.p[i])  # untouched
            continue
        sa, sb = oa.state[a[i]], ob.state[b[i]]
        for name, fa, fb, r in (("p", a[i], b[i], ref.p[i]), ("exp_avg", sa["exp_avg"], sb["exp_avg"], ref.m[i]),
                                ("exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"], ref.v[i])):
            ea = (fa.detach().double() - r).abs().max().item()
            eb = (fb.detach().double() - r).abs().max().item()
            bound = 4 * eb + 2 * _ulp(r.abs().max().item())
            print(f"adam {case} tensor {i} {tuple(s)} {name}: fused {ea:.3e} torch {eb:.3e} bound {bound:.3e}")
            assert np.isfinite(ea)
            if not ea <= bound:
                bad.append((i, name, ea, eb, bound))
    assert not bad, bad


# (a): numel 1, 4095, 4096 | grad-less 5000 | 4097, 8192, 12293, 3 * 4096
SHAPES_A = [(1,), (1365, 3), (4096,), (5000,), (4097,), (8192,), (12293,), (4096, 3)]


def test_eight_tensors_one_launch(pkg, cuda):
    """One launch of 8 descriptors; the fourth tensor has no gradient."""
    gen, a, b, oa, ob, ref = _setup(pkg, cuda, SHAPES_A, [(range(8), {})], seed=1)
    _advance(gen, cuda, SHAPES_A, a, b, ref, _randn, {3}, oa.step, ob.step)
    _compare("(a)", SHAPES_A, a, oa, b, ob, ref, nograd={3})


def test_null_grad_in_the_middle_of_the_block_table(pkg, cuda):
    """gs_adam_step with all 8 descriptors, the fourth with grad == NULL (two
    equal entries in the kernel's block table; FusedAdam.step itself leaves
    such a tensor out of the launch): every other tensor as FusedAdam.step
    leaves it, bit for bit, the grad-less one and its moments untouched."""
    N = pkg._native
    gen = torch.Generator().manual_seed(2)
    p = [torch.randn(s, generator=gen).to(cuda) for s in SHAPES_A]
    q = [t.clone().requires_grad_() for t in p]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    m[3].fill_(3.0)
    v[3].fill_(5.0)
    p3 = p[3].clone()
    opt = pkg.optim.FusedAdam([t for i, t in enumerate(q) if i != 3], **DEFAULTS)
    b1, b2 = DEFAULTS["betas"]
    for t in range(1, 3):
        grads = [_randn(s, gen).to(cuda) for s in SHAPES_A]
        args = N.GsAdamArgs()
        args.num_tensors, args.beta1, args.beta2, args.eps = 8, b1, b2, DEFAULTS["eps"]
        args.one_minus_beta1, args.one_minus_beta2 = 1.0 - b1, 1.0 - b2
        for k in range(8):
            args.t[k] = N.GsAdamTensor(N.ptr(p[k]), N.ptr(m[k]), N.ptr(v[k]), None if k == 3 else N.ptr(grads[k]),
                                       p[k].numel(), DEFAULTS["lr"], 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5, None)
        N.check(N.load().gs_adam_step(C.byref(args), N.stream_ptr()), "gs_adam_step")
        for k in range(8):
            q[k].grad = None if k == 3 else grads[k]
        opt.step()
    for k in range(8):
        if k == 3:
            assert torch.equal(p[3], p3) and (m[3] == 3.0).all() and (v[3] == 5.0).all()
            continue
        st = opt.state[q[k]]
        assert torch.equal(p[k], q[k].detach()), k
        assert torch.equal(m[k], st["exp_avg"]) and torch.equal(v[k], st["exp_avg_sq"]), k


SHAPES_B = [(4096,), (1500, 3), (4097,), (7,), (8192,), (2731, 3), (1,), (4095,), (12293,), (3000, 4)]
GROUPS_B = [([0, 1, 2, 3], {}),
            ([4, 5, 6, 7, 8], dict(lr=5e-3, betas=(0.5, 0.9), eps=1e-15)),
            ([9], dict(lr=0.05, betas=(0.8, 0.99), eps=1e-6))]
SHAPES_B9 = [(4096,), (100, 3), (4097,), (7,), (8192,), (1,), (4095,), (5000,), (2731, 3)]


@pytest.mark.parametrize("case,shapes,groups", [("(b) 3 groups", SHAPES_B, GROUPS_B),
                                                ("(b) 9 tensors", SHAPES_B9, [(range(9), {})])])
def test_more_than_one_launch(pkg, cuda, case, shapes, groups):
    """Three (betas, eps) batches, one launch each; and nine tensors in one
    batch, which takes two launches (GS_ADAM_MAX_TENSORS = 8)."""
    gen, a, b, oa, ob, ref = _setup(pkg, cuda, shapes, groups, seed=3)
    _advance(gen, cuda, shapes, a, b, ref, _randn, (), oa.step, ob.step)
    _compare(case, shapes, a, oa, b, ob, ref)


def test_gradient_magnitudes(pkg, cuda):
    """Exact zeros and magnitudes over 15 decades, in the scalar tail, the
    float4 tail and whole chunks, under both sets of betas / eps."""
    shapes = [(4097,), (8192,), (2731, 3), (4097,), (8192,)]
    groups = [([0, 1, 2], {}), ([3, 4], dict(betas=(0.5, 0.9), eps=1e-15))]
    gen, a, b, oa, ob, ref = _setup(pkg, cuda, shapes, groups, seed=4)
    _advance(gen, cuda, shapes, a, b, ref, _wide, (), oa.step, ob.step)
    _compare("(c)", shapes, a, oa, b, ob, ref)


def test_step_ranges_unaligned(pkg, cuda):
    """Row ranges at byte offsets 4 and 12 (and 8 after 4098 rows): the scalar
    branch over whole chunks.  Bit-equal to step() and within the bound."""
    n = 9001
    shapes = [(n, 1), (n, 3)]
    gen, a, b, oa, ob, ref = _setup(pkg, cuda, shapes, [([0], {}), ([1], dict(lr=5e-3))], seed=5)
    c = [t.detach().clone().requires_grad_() for t in a]
    oc = pkg.optim.FusedAdam([dict(DEFAULTS, params=[c[0]]), dict(DEFAULTS, lr=5e-3, params=[c[1]])])
    ranges = [(0, 1), (1, 4098), (4098, n)]

    def step_b():
        for x, y in zip(a, c):
            y.grad = x.grad.clone()
        oc.step()
        ob.step()

    _advance(gen, cuda, shapes, a, b, ref, _randn, (), lambda: oa.step_ranges(ranges), step_b)
    for x, y in zip(a, c):
        assert torch.equal(x.detach(), y.detach())
        assert torch.equal(oa.state[x]["exp_avg"], oc.state[y]["exp_avg"])
        assert torch.equal(oa.state[x]["exp_avg_sq"], oc.state[y]["exp_avg_sq"])
        assert oa.state[x]["step"] == oc.state[y]["step"] == STEPS
    _compare("(d)", shapes, a, oa, b, ob, ref)


def test_set_output_whole_chunks(pkg, cuda):
    """param_out over whole chunks and a tail: the output equals the in-place
    step's parameter bit for bit, the parameter is only read, nothing of the
    output's NaN prefill is left."""
    shapes = [(8192,), (12293,)]
    gen = torch.Generator().manual_seed(6)
    a = [torch.randn(s, generator=gen).to(cuda).requires_grad_() for s in shapes]
    b = [t.detach().clone().requires_grad_() for t in a]
    p0 = [t.detach().clone() for t in a]
    oa, ob = pkg.optim.FusedAdam(a, **DEFAULTS), pkg.optim.FusedAdam(b, **DEFAULTS)
    outs = [torch.full_like(t, float("nan")) for t in a]
    for t, o in zip(a, outs):
        oa.set_output(t, o)
    for _ in range(STEPS):
        for x, y, s in zip(a, b, shapes):
            g = _randn(s, gen).to(cuda)
            x.grad, y.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
        for x, y, o, q in zip(a, b, outs, p0):
            assert torch.equal(x.detach(), q)
            assert not torch.isnan(o).any()
            assert torch.equal(o, y.detach()) and not torch.equal(o, q)
            assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"])
            assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])
            with torch.no_grad():
                y.copy_(q)  # both start every step from the same parameters
                o.fill_(float("nan"))
