"""The absolute screen-space gradient of the blend (AbsGS; gs_blend_backward_abs)
for tests/test_absgrad_cpu.py and tests/test_absgrad_gpu.py, built from
tests/blend_reference.py's blocks (Frame, skip_exponent, cpu_frame, case_scene,
forced neval / flags).

`pixel_gradients` (torch fp64, autograd) is blend_reference.reference_tile's
loop over one tile with the record values expanded into leaves per (list
entry, pixel) -- but it returns the leaves' own gradients of mu_x and mu_y,
G[i, p, 0:2] = dL/dmu(p) of entry i at pixel p, instead of their sums over a
cell.  reference_tile's partials[..., 0:2] are their signed sums per cell
(test_absgrad_cpu pins that); the absolute partial of (entry, cell) is
`abs_partials`: sum over the cell's pixels of |G|.  No hand-derived backward.

`emulate_abs_tile` is the formulation the header and gs_blend.hip document,
in plain numpy fp32: blend_reference.emulate_tile's phase A (the per-pixel
chain carrying A, T1 = 1 - A and PG, giving dop and the signed weight c per
(entry, pixel)), then per (entry, cell) and column

    ax += |ds| |fma(qo, dy_r, 2 q00 bx)|,  ay += |ds| |fma(2 q11, dy_r, qo bx)|

over the 8 rows (dy_r = (y0 + r) - my, the forward's own dy; bx the column's
dx), scaled once by |hop| = |o / 2| and summed over the columns in oct_sum's
order.  It runs without a GPU and measures the constant K of the bound

    |x_gpu - x_fp64| <= K (n_p + 1) 2^-24 M,

M = reference_tile's M[:, q, 0] and M[:, q, 1]: sums of absolute values
already, they bound the absolute partial itself."""
import numpy as np
import torch

import blend_reference as B

F32 = np.float32


def pixel_gradients(fr, t, g_image, g_alpha=None, g_depth=None, neval=None, flags=None, values=None):
    """One tile.  Arguments as blend_reference.reference_tile; values: fp64
    [n, 10] or, per (entry, pixel), [n, P, 10] in place of the records' (in
    COMPONENTS order; the skip decisions stay the records').  Returns ids, xs,
    ys, cq, the loss and G [n, P, 2] = d loss / d (mu_x, mu_y) of each leaf."""
    ids = fr.entries(t)
    n = len(ids)
    xs, ys, cq = fr.pixels(t)
    P = len(xs)
    pix = ys * fr.W + xs
    rec = fr.records[ids]
    skip = torch.from_numpy(B.skip_exponent(rec, xs, ys) < B.SKIP_T) if n else torch.zeros((0, P), dtype=torch.bool)
    base = rec[:, list(B.REC_COL)].astype(np.float64) if values is None else np.asarray(values, np.float64)
    V = torch.from_numpy(base)
    V = (V[:, None, :].expand(n, P, 10) if V.dim() == 2 else V).clone()
    V.requires_grad_(True)
    X_, Y_ = torch.from_numpy(xs.astype(np.float64)), torch.from_numpy(ys.astype(np.float64))
    bg = torch.from_numpy(fr.bg.astype(np.float64))
    nev = None if neval is None else torch.from_numpy(np.asarray(neval).reshape(-1)[pix].astype(np.int64))
    A = torch.zeros(P, dtype=torch.float64)
    D = torch.zeros(P, dtype=torch.float64)
    acc = bg[None, :].expand(P, 3).clone()
    for i in range(n):
        mx, my, q00, qo, q11, o, r, g, b, z = V[i].unbind(-1)
        dx, dy = X_ - mx, Y_ - my
        s = q00 * dx * dx + qo * dx * dy + q11 * dy * dy
        w = torch.exp(-0.5 * s).clamp(0.0, 1.0)
        ai = (o * w).clamp(0.0, 1.0)
        run = (A.detach() < B.STOP) if nev is None else (i < nev)
        c = (1.0 - A) * ai
        take = run & ~skip[i] & (c.detach() > 0)
        c = torch.where(take, c, torch.zeros_like(c))
        acc = acc + c[:, None] * torch.stack([r, g, b], -1)
        D = D + c * z
        A = A + c
    comp = acc + (1.0 - A)[:, None] * bg
    if flags is None:
        blocked = torch.cat([~((comp.detach() >= 0) & (comp.detach() <= 1)),
                             ~((A.detach() >= 0) & (A.detach() <= 1))[:, None]], 1)
    else:
        fl = torch.from_numpy(np.asarray(flags).reshape(-1)[pix].astype(np.int64))
        blocked = torch.stack([(fl >> k) & 1 for k in range(4)], 1).bool()
    image = torch.where(blocked[:, :3], comp.detach().clamp(0, 1), comp)
    alpha = torch.where(blocked[:, 3], A.detach().clamp(0, 1), A)
    depth = D / (A + float(B.EPS))
    gi = torch.from_numpy(np.asarray(g_image, np.float64).reshape(3, -1)[:, pix].T.copy())
    L = (gi * image).sum()
    if g_alpha is not None:
        L = L + (torch.from_numpy(np.asarray(g_alpha, np.float64).reshape(-1)[pix]) * alpha).sum()
    if g_depth is not None:
        L = L + (torch.from_numpy(np.asarray(g_depth, np.float64).reshape(-1)[pix]) * depth).sum()
    out = dict(ids=ids, xs=xs, ys=ys, cq=cq, pix=pix, loss=float(L.detach()))
    if n:
        L.backward()
        out["G"] = V.grad.numpy()[:, :, 0:2].copy()
    else:
        out["G"] = np.zeros((0, P, 2))
    return out


def cell_sums(fr, pg, absolute):
    """[n, cells, 2]: G (or |G|) summed over each cell's pixels."""
    G = np.abs(pg["G"]) if absolute else pg["G"]
    out = np.zeros((G.shape[0], fr.cells, 2))
    for q in range(fr.cells):
        m = pg["cq"] == q
        if m.any():
            out[:, q] = G[:, m].sum(1)
    return out


def abs_partials(fr, pg):
    return cell_sums(fr, pg, True)


def _oct_sum(v):
    """gs_device.h's oct_sum over the last axis (8 columns), in its order:
    neighbours, pairs of neighbours, then the two halves."""
    a = v[..., 0::2] + v[..., 1::2]
    b = a[..., 0::2] + a[..., 1::2]
    return b[..., 0] + b[..., 1]


def emulate_abs_tile(fr, t, g_image, g_alpha=None, g_depth=None, em=None):
    """The absolute partials [n, cells, 2] of one tile in numpy fp32, from the
    decisions and outputs of blend_reference.emulate_tile (em, computed here
    when not given): phase A as there, then the per-pixel absolute sums."""
    if em is None:
        em = B.emulate_tile(fr, t, g_image, g_alpha, g_depth)
    ids = fr.entries(t)
    n = len(ids)
    xs, ys, cq = fr.pixels(t)
    P = len(xs)
    pix = ys * fr.W + xs
    Q = fr.cells
    out = np.zeros((n, Q, 2), F32)
    if n == 0:
        return out
    rec = fr.records[ids].astype(F32)
    tq = B.skip_exponent(rec, xs, ys)
    one, zero = F32(1), F32(0)
    bg = fr.bg.astype(F32)
    o, col, z = rec[:, 5], rec[:, 6:9], rec[:, 9]
    fma = B._fma
    with np.errstate(all="ignore"):
        e_all = np.exp(tq).astype(F32)
        w_all = np.clip(e_all, zero, one)
        u_all = o[:, None] * w_all
        ai_all = np.clip(u_all, zero, one)
        # the pixel header (emulate_tile's, from its forward)
        image, alpha, depth = em["image"], em["alpha"], em["depth"]
        blocked = np.stack([(em["flags"] >> k) & 1 for k in range(4)], 1).astype(bool)
        gi = np.asarray(g_image, F32).reshape(3, -1)[:, pix].T
        gR = np.where(blocked[:, :3], zero, gi)
        tbb = one - alpha
        tr = image - tbb[:, None] * bg[None, :]
        den = alpha + B.EPS
        Dt = depth * den
        gA = -gR[:, 0] * bg[0] - gR[:, 1] * bg[1] - gR[:, 2] * bg[2]
        if g_alpha is not None:
            gA = gA + np.where(blocked[:, 3], zero, np.asarray(g_alpha, F32).reshape(-1)[pix])
        gD = np.zeros(P, F32)
        if g_depth is not None:
            gdp = np.asarray(g_depth, F32).reshape(-1)[pix]
            gD = gdp / den
            gA = gA + (-gdp * Dt / (den * den))
        K = (gR[:, 0] * tr[:, 0] + gR[:, 1] * tr[:, 1]) + (gR[:, 2] * tr[:, 2] + gD * Dt)
        G0 = fma(gA, tbb, -K)
        PG = ((gR[:, 0] * bg[0] + gR[:, 1] * bg[1]) + gR[:, 2] * bg[2]) + G0
        # phase A: the replayed chain
        A = np.zeros(P, F32)
        T1 = np.ones(P, F32)
        run = np.ones(P, bool)
        dop = np.zeros((n, P), F32)
        cw = np.zeros((n, P), F32)
        for i in range(n):
            live = run & ~(tq[i] < B.SKIP_T)
            X = fma(gR[:, 0], col[i, 0], fma(gR[:, 1], col[i, 1], fma(gR[:, 2], col[i, 2], gD * z[i])))
            trans = T1
            c = trans * np.where(live, ai_all[i], zero)
            A = A + c
            PG = fma(c, X, PG)
            term = ~(A < F32(B.STOP))
            T1 = one - A
            d_live = fma(one / T1, PG, X)
            dal = trans * np.where(term, X + gA, d_live)
            run = run & ~term
            g = np.where(ai_all[i] == u_all[i], dal * w_all[i], zero)
            dop[i] = np.where(c > 0, g, zero)
            cw[i] = np.where(w_all[i] == e_all[i], c, -c)
        # phase B, the absolute sums: per pixel, not through the moments
        q00, q11, qo = rec[:, 2:3], rec[:, 3:4], rec[:, 4:5]
        ah = np.abs(F32(-0.5) * o)[:, None]
        for q in range(Q):
            m = cq == q
            if not m.any():
                continue
            x0c, y0c = fr.cell_origin(t, q)
            dq = np.zeros((n, 8, 8), F32)   # [entry, row, column]
            cq_ = np.zeros((n, 8, 8), F32)
            rr, cc = ys[m] - y0c, xs[m] - x0c
            dq[:, rr, cc], cq_[:, rr, cc] = dop[:, m], cw[:, m]
            bx = np.arange(x0c, x0c + 8).astype(F32)[None, :] - rec[:, 0:1]   # [n, 8]
            qxx, qxy, q11x2 = (F32(2) * q00) * bx, qo * bx, F32(2) * q11
            ax = np.zeros((n, 8), F32)
            ay = np.zeros((n, 8), F32)
            for r in range(8):
                ads = np.abs(np.where(cq_[:, r] > 0, dq[:, r], zero))
                dyr = F32(y0c + r) - rec[:, 1:2]
                ax = fma(ads, np.abs(fma(qo, dyr, qxx)), ax)
                ay = fma(ads, np.abs(fma(q11x2, dyr, qxy)), ay)
            out[:, q, 0] = _oct_sum(ax * ah)
            out[:, q, 1] = _oct_sum(ay * ah)
    return out


def host_case(name, which):
    """A committed case on a host-built frame, decisions forced from the fp32
    emulation as test_blend_stage._host_refs does: the frame, the cotangents,
    per tile the emulation, blend_reference.reference_tile's result and the
    per-pixel gradients."""
    sc = B.case_scene(name)
    fr = B.cpu_frame(sc)
    mutate = B.CASES[name][1]
    if mutate:
        mutate(fr)
    cot = B.case_cotangents(sc, which)
    ems = B.whole_frame(fr, lambda t: B.emulate_tile(fr, t, *cot))
    nev, fl, al = np.zeros(fr.W * fr.H, np.int64), np.zeros(fr.W * fr.H, np.uint8), np.zeros(fr.W * fr.H, F32)
    for em in ems.values():
        nev[em["pix"]], fl[em["pix"]], al[em["pix"]] = em["neval"], em["flags"], em["alpha"]
    refs = B.whole_frame(fr, lambda t: B.reference_tile(fr, t, *cot, neval=nev, flags=fl, alpha_fwd=al))
    pgs = B.whole_frame(fr, lambda t: pixel_gradients(fr, t, *cot, neval=nev, flags=fl))
    return fr, cot, ems, refs, pgs


def abs_ratio(got, want, ref):
    """Largest |got - want| / ((n_p + 1) 2^-24 M) over a tile's [n, cells, 2]
    absolute partials (inf where the bound is 0 and they differ)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    return B.ratio(err, ref["M"][:, :, 0:2], ref["n_cell"][None, :, None])
