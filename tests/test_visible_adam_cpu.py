"""Visibility-gated Adam, the parts that need no GPU: the layout of
gs_adam_rows_args against its ctypes mirror, the C ABI's argument checks (they
return before any HIP call, with host pointers that are never dereferenced),
FusedAdam's validation of the mask, and the configuration plumbing."""
import ctypes as C
import os
import subprocess
import types

import pytest
import torch

from stubs import Cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 3


def test_status_codes_match_the_header():
    text = open(os.path.join(ROOT, "include", "gsplat_mi355x.h"), encoding="utf-8").read()
    for name, value in (("GS_OK", OK), ("GS_ERR_INVALID_ARG", INVALID), ("GS_ERR_UNSUPPORTED", UNSUPPORTED)):
        assert f"{name} = {value}" in text, name


def test_layout_matches_c(pkg, tmp_path):
    N = pkg._native
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat_mi355x.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(gs_adam_rows_args), offsetof(gs_adam_rows_args, adam), '
                   'offsetof(gs_adam_rows_args, rows), offsetof(gs_adam_rows_args, cols), '
                   'offsetof(gs_adam_rows_args, row_mask), GS_ADAM_ROW_BLOCK, GS_ADAM_ROWS_MAX_COLS);}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    A = N.GsAdamRowsArgs
    assert got == [C.sizeof(A), A.adam.offset, A.rows.offset, A.cols.offset, A.row_mask.offset, N.GS_ADAM_ROW_BLOCK,
                   N.GS_ADAM_ROWS_MAX_COLS]
    assert A.adam.offset == 0 and A.rows.offset == C.sizeof(N.GsAdamArgs)
    assert N.GS_ADAM_ROW_BLOCK % 4 == 0


def test_abi_version_and_export(pkg):
    N = pkg._native
    lib = N.load()
    assert lib.gs_abi_version() == 23 and N.GS_ABI_VERSION == 23
    assert "gs_adam_step_rows" in N.EXPORTS and hasattr(lib, "gs_adam_step_rows")
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    assert " T gs_adam_step_rows" in out


def _args(N, p, rows=8, cols=(3, 1), grads=(True, True)):
    """Two tensors over a host buffer nothing reads."""
    a = N.GsAdamRowsArgs()
    a.rows, a.row_mask = rows, p
    ad = a.adam
    ad.num_tensors, ad.beta1, ad.beta2, ad.eps = len(cols), 0.9, 0.999, 1e-8
    for k, c in enumerate(cols):
        a.cols[k] = c
        ad.t[k] = N.GsAdamTensor(p, p, p, p if grads[k] else None, rows * c, 1e-3, 0.1, 0.03, None)
    return a


def test_argument_errors(pkg):
    N = pkg._native
    lib = N.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    call = lambda a: lib.gs_adam_step_rows(C.byref(a), None)
    assert lib.gs_adam_step_rows(None, None) == INVALID
    assert b"gs_adam_step_rows" in lib.gs_last_error()

    a = _args(N, p)
    a.row_mask = None
    assert call(a) == INVALID  # a NULL row_mask
    a = _args(N, p, rows=0)
    a.row_mask = None
    assert call(a) == INVALID  # ... whatever the row count
    a = _args(N, p)
    a.rows = -1
    assert call(a) == INVALID
    for bad_cols in (0, -3):
        a = _args(N, p)
        a.cols[1] = bad_cols
        assert call(a) == INVALID, bad_cols
    a = _args(N, p)
    a.adam.t[0].numel = 8 * 3 + 1  # numel != rows * cols
    assert call(a) == INVALID
    a = _args(N, p)
    a.cols[0] = 4
    assert call(a) == INVALID
    for field in ("param", "exp_avg", "exp_avg_sq"):  # a NULL buffer behind a non-NULL grad
        a = _args(N, p)
        setattr(a.adam.t[1], field, None)
        assert call(a) == INVALID, field
    for n in (-1, N.GS_ADAM_MAX_TENSORS + 1):
        a = _args(N, p)
        a.adam.num_tensors = n
        assert call(a) == INVALID, n
    # a tensor without a grad is skipped: its other fields are not looked at
    a = _args(N, p, rows=0, grads=(True, False))
    a.cols[1], a.adam.t[1].param, a.adam.t[1].numel = 0, None, 77
    assert call(a) == OK

    for field in ("skip_flag", "hyper", "hyper_row"):
        a = _args(N, p)
        setattr(a.adam, field, p)
        assert call(a) == UNSUPPORTED, field
    a = _args(N, p)
    a.adam.t[1].param_out = p
    assert call(a) == UNSUPPORTED
    assert b"param_out" in lib.gs_last_error()
    a = _args(N, p, cols=(N.GS_ADAM_ROWS_MAX_COLS + 1, 1))
    assert call(a) == UNSUPPORTED

    # nothing to do: GS_OK with nothing launched
    assert call(_args(N, p, rows=0)) == OK
    assert call(_args(N, p, grads=(False, False))) == OK
    a = _args(N, p)
    a.adam.num_tensors = 0
    assert call(a) == OK


def _params(n=6, device="cpu"):
    ps = [torch.zeros(n, 3, device=device, requires_grad=True), torch.zeros(n, 1, device=device, requires_grad=True)]
    for q in ps:
        q.grad = torch.ones_like(q)
    return ps


@pytest.mark.parametrize("bad,match", [
    (lambda: torch.ones(6), "bool or uint8"),                               # dtype
    (lambda: torch.ones(6, dtype=torch.int32), "bool or uint8"),
    (lambda: [1, 0, 1, 1, 0, 1], "bool or uint8"),                          # not a tensor
    (lambda: torch.ones(6, 1, dtype=torch.bool), "contiguous"),             # layout: not [N]
    (lambda: torch.ones(12, dtype=torch.uint8)[::2], "contiguous"),         # layout: strided
    (lambda: torch.ones(5, dtype=torch.bool), "rows"),                      # size
    (lambda: torch.ones(7, dtype=torch.uint8), "rows"),
    (lambda: torch.ones(6, dtype=torch.bool, device="meta"), "is on meta"),  # device
])
def test_fused_adam_rejects_the_mask(pkg, bad, match):
    ps = _params()
    opt = pkg.optim.FusedAdam(ps)
    for call in (lambda m: opt.step(visible=m), lambda m: opt.step_ranges([(0, 3), (3, 6)], visible=m)):
        with pytest.raises(ValueError, match=match):
            call(bad())
    assert not opt.state[ps[0]] and not opt.state[ps[1]], "nothing was counted"


def test_fused_adam_rejects_rows_that_differ_and_set_output(pkg):
    ps = _params()
    odd = torch.zeros(4, 2, requires_grad=True)
    odd.grad = torch.ones_like(odd)
    scalar = torch.zeros((), requires_grad=True)
    scalar.grad = torch.ones(())
    mask = torch.ones(6, dtype=torch.bool)
    for extra in (odd, scalar):
        opt = pkg.optim.FusedAdam(ps + [extra])
        with pytest.raises(ValueError, match="rows"):
            opt.step(visible=mask)
        # ... a parameter without a gradient is not stepped and may have any shape:
        # the mask is then accepted, and the step gets as far as asking for HIP tensors
        extra.grad = None
        with pytest.raises(RuntimeError, match="HIP tensors"):
            opt.step(visible=mask)
    opt = pkg.optim.FusedAdam(ps)
    opt.set_output(ps[1], torch.zeros(6, 1))
    with pytest.raises(ValueError, match="set_output"):
        opt.step(visible=mask)
    with pytest.raises(ValueError, match="set_output"):
        opt.step_ranges([(0, 6)], visible=mask)


def test_config_field_and_yaml_round_trip(pkg, tmp_path):
    assert pkg.TrainingConfig().visible_adam is False
    c = pkg.TrainingConfig(visible_adam=True, densify_criterion="mcmc")
    c.check()
    path = tmp_path / "cfg.yaml"
    pkg.ConfigManager.save(c, str(path))
    assert pkg.ConfigManager.load(str(path)) == c


def test_replayed_step_refuses_visible_adam(pkg):
    """GraphedStep replays the dense update: a model configured for
    visible_adam is refused before anything touches a device."""
    model = types.SimpleNamespace(config=pkg.TrainingConfig(visible_adam=True), _gs_fused_covariance=True)
    with pytest.raises(ValueError, match="visible_adam"):
        pkg.GraphedStep(pkg.GaussianRenderer(), Cam(64, 64, 1.0, 1.0), model, None, ())


def test_gaussian_optimizer_forwards_the_mask(pkg):
    """GaussianOptimizer.step hands the mask on, and calls the dense step
    exactly as before without one."""
    calls = []

    class Opt:
        def step(self, **kw):
            calls.append(("step", kw))

    go = pkg.optim.GaussianOptimizer.__new__(pkg.optim.GaussianOptimizer)
    go.optimizer = Opt()
    mask = torch.ones(3, dtype=torch.uint8)
    go.step()
    go.step(visible=mask)
    assert calls == [("step", {}), ("step", {"visible": mask})]
