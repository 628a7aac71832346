"""What tests/test_resume_gpu.py, tests/test_resume_cpu.py and
tests/resume_worker.py share: the state a training run carries from one step
to the next, read out of a GaussianTrainer and compared bit for bit, and the
schedule of the resume-equivalence matrix."""
import numpy as np
import torch

PARAMS = ["xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"]
STATS = ["grad_accum", "denom", "max_radii", "abs_accum"]

# One schedule for the whole matrix.  Densifications at 8 and 16 (before K) and
# at 24 and 32 (after it); the one at 24 reads the views of iterations 17..24,
# accumulated on both sides of K.  K is a multiple of no interval any mode sets
# (8, 17, 15, 7) and not the contribution-pruning iteration (K + 5).
# ITERATIONS is config.iterations in every trainer: it sets the learning-rate
# schedule, so only the argument of train(n) differs between the runs.
FROM, INTERVAL, UNTIL = 8, 8, 40
K, END, ITERATIONS = 20, 36, 40
K_AT_DENSIFY = 16  # (reset_adam's second case: the optimizer state is empty there)
RESET_INTERVAL, SH_INTERVAL, FILTER_INTERVAL = 17, 15, 7


def base_config(pkg, out, **kw):
    base = dict(iterations=ITERATIONS, densify_from_iter=FROM, densify_until_iter=UNTIL, densify_interval=INTERVAL,
                num_random_points=2000, log_interval=1, output_path=str(out), position_lr_init=1.6e-3,
                position_lr_final=1.6e-5)
    base.update(kw)
    return pkg.TrainingConfig(**base)


def bits(t):
    """The tensor's bit pattern (fp32 as int32): NaNs and signed zeros compare
    as what they are."""
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def state(tr):
    """Everything a later step reads, as a flat dict of cloned tensors and
    plain values (a key is absent where the trainer holds nothing)."""
    if tr.gaussians._xyz.is_cuda:
        torch.cuda.synchronize()
    g = tr.gaussians
    out = {}
    for name, p in zip(PARAMS, g.parameter_list()):
        out[name] = p.detach().clone()
        st = tr.optimizer.optimizer.state.get(p, {})
        if "exp_avg" in st:
            out[f"adam.{name}.m"] = st["exp_avg"].clone()
            out[f"adam.{name}.v"] = st["exp_avg_sq"].clone()
            out[f"adam.{name}.step"] = int(st["step"])
    for name in STATS:
        t = getattr(g.density_stats, name)
        if t is not None:
            out[f"density.{name}"] = t.clone()
    if tr.filter_3d is not None:
        out["filter_3d.values"] = tr.filter_3d.values.clone()
        out["filter_3d.max_rate"] = tr.filter_3d.max_rate.clone()
    out["active_sh_degree"] = int(g.active_sh_degree)
    out["iteration"] = int(tr.iteration)
    out["n"] = int(g.get_num_points())
    out["last_densify"] = None if tr.last_densify is None else dict(tr.last_densify)
    return out


def differences(a, b):
    """The keys in which two states differ (a key only one of them has, a
    shape, a dtype, or one bit)."""
    bad = sorted(set(a) ^ set(b))
    for k in sorted(set(a) & set(b)):
        x, y = a[k], b[k]
        if isinstance(x, torch.Tensor) != isinstance(y, torch.Tensor):
            bad.append(k)
        elif isinstance(x, torch.Tensor):
            if x.shape != y.shape or x.dtype != y.dtype or not torch.equal(bits(x), bits(y)):
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad


def assert_same(a, b, what):
    bad = differences(a, b)
    assert not bad, f"{what}: differ in {bad}"


def state_to_numpy(st):
    """A state as np.savez keywords (tensors as arrays, ints as 0-d arrays,
    last_densify's counts under ld.*)."""
    out = {}
    for k, v in st.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.cpu().numpy()
        elif k == "last_densify":
            for kk, vv in (v or {}).items():
                out[f"ld.{kk}"] = np.int64(vv)
        else:
            out[k] = np.int64(v)
    return out


def state_from_numpy(z, device):
    out, ld = {}, {}
    for k in z.files:
        v = z[k]
        if k.startswith("ld."):
            ld[k[3:]] = int(v)
        elif v.ndim == 0:
            out[k] = int(v)
        else:
            out[k] = torch.from_numpy(v).to(device)
    out["last_densify"] = ld or None
    return out
