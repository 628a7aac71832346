"""An independent statement of the alpha blend (renderer.py:302-367 of the
reference, per pixel) for tests/test_blend_stage.py: every quantity the blend
kernels write, from the frame exactly as they see it.

Inputs: a `Frame` -- the fp32 records [n, 12] (mx my q00 q11 | qo o r g |
b z slot info), the tile lists (sorted_gauss, ranges), the image geometry and
background -- and the cotangents.

`reference_tile` (torch fp64, autograd) restates the blend of one tile:

* the `w < 1e-5` skip is decided in numpy fp32 exactly as the kernels do
  (`skip_exponent`: t = ((dx dx) h00 + (ho dx) dy) + (dy dy) h11 with the conic
  staged as -Q/2, skipped iff t < -0.5f * 23.0258509f): plain fp32 operations
  of a library built without contraction, reproducible bit for bit;
* the `A >= 0.995` termination is taken from the forward's pix_neval (1 + the
  list index of the pixel's terminating entry, the list length for a pixel
  that never terminated) or, with neval=None, decided by the fp64 chain
  itself; the caller validates a forced decision against A_after;
* the clamp decisions (pix_flags) likewise: forced, or the fp64 composite's;
* the record values are expanded into leaves per (list entry, pixel), so the
  gradient of a leaf summed over a cell's pixels is the partial the backward
  writes for that (entry, cell) -- no hand-derived backward;
* M, the same expressions with every term replaced by its absolute value, for
  the bound  |x_gpu - x_fp64| <= K (n_p + 1) 2^-24 M(x)  (DESIGN.md, section 2).

`emulate_tile` is the formulation the header and the kernel comments document,
evaluated in plain numpy fp32: a sequential per-pixel chain carrying A,
T1 = 1 - A and PG, then column and row moments (about row 0, or about the row
nearest the mean for an entry with sigma_y < 2 px).  It runs without a GPU and
measures the constant K of the bound.

`cpu_frame` builds a stand-in frame on the host (tests/project_reference.py in
fp64, rounded to fp32; the reference's binning) so that the statement and the
emulation run on every committed case without a GPU; the GPU tests build
their frames with the library."""
from dataclasses import dataclass

import numpy as np
import torch

import project_reference as PR

U24 = 2.0 ** -24
STOP = 0.995
F32 = np.float32
SKIP_T = F32(-0.5) * F32(23.0258509)
EPS = F32(1e-6)
COMPONENTS = ("dmu_x", "dmu_y", "dQ00", "dQ01", "dQ11", "d_opacity", "d_r", "d_g", "d_b", "d_z")
REC_COL = (0, 1, 2, 4, 3, 5, 6, 7, 8, 9)  # record column of each component's leaf
FX = 32.0  # focal length of the test camera, px (fx = fy, exact in fp32)


@dataclass
class Frame:
    records: np.ndarray       # [n, 12] fp32
    sorted_gauss: np.ndarray  # [T] int64
    ranges: np.ndarray        # [tiles, 2] int64
    W: int
    H: int
    L: int
    bg: np.ndarray            # [3] fp32

    @property
    def tiles_x(self):
        return (self.W + self.L - 1) // self.L

    @property
    def tiles_y(self):
        return (self.H + self.L - 1) // self.L

    @property
    def QX(self):
        return (self.L + 7) // 8

    @property
    def cells(self):
        return self.QX * self.QX

    @property
    def T(self):
        return len(self.sorted_gauss)

    def entries(self, t):
        s, e = (int(v) for v in self.ranges[t])
        e = min(e, self.T)
        return self.sorted_gauss[min(s, e):e]

    def pixels(self, t):
        """The tile's pixels inside the image: x, y, the cell of each."""
        tx, ty = t % self.tiles_x, t // self.tiles_x
        x0, y0 = tx * self.L, ty * self.L
        ys, xs = np.mgrid[y0:min(y0 + self.L, self.H), x0:min(x0 + self.L, self.W)]
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        return xs, ys, ((ys - y0) // 8) * self.QX + (xs - x0) // 8

    def cell_origin(self, t, q):
        tx, ty = t % self.tiles_x, t // self.tiles_x
        return tx * self.L + (q % self.QX) * 8, ty * self.L + (q // self.QX) * 8

    def slots(self, t):
        """Gradient slot of each entry of tile t: pair_offset[g] (record word 10)
        + the tile's index in g's rectangle (word 11: tx0 | ty0 << 12 | (width - 1) << 24)."""
        ids = self.entries(t)
        tx, ty = t % self.tiles_x, t // self.tiles_x
        w10 = self.records[ids, 10].view(np.uint32).astype(np.int64)
        info = self.records[ids, 11].view(np.uint32).astype(np.int64)
        return w10 + (ty - ((info >> 12) & 0xFFF)) * ((info >> 24) + 1) + (tx - (info & 0xFFF))


def skip_exponent(rec, xs, ys):
    """t = -s/2 [n, P] in fp32, operation for operation as the kernels form it."""
    rec = rec.astype(F32)
    h00, h11, ho = F32(-0.5) * rec[:, 2:3], F32(-0.5) * rec[:, 3:4], F32(-0.5) * rec[:, 4:5]
    dx = xs.astype(F32)[None, :] - rec[:, 0:1]
    dy = ys.astype(F32)[None, :] - rec[:, 1:2]
    with np.errstate(over="ignore", invalid="ignore"):
        return ((dx * dx) * h00 + (ho * dx) * dy) + (dy * dy) * h11


def simple_entry(rec):
    """simple_entry of gs_blend.hip in fp32: the clamps provably never bind."""
    rec = rec.astype(F32)
    q00, q11, qo, o = rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5]
    q01 = F32(0.5) * qo
    det, tr = q00 * q11 - q01 * q01, q00 + q11
    return (o >= F32(1e-20)) & (o <= F32(1)) & (tr > 0) & (det > 0) & ((tr + np.abs(qo)) * tr <= F32(1e4) * det)


def small_y(rec):
    """Phase B's recentring test in fp32: Sigma_yy = q00 / det < 4."""
    rec = rec.astype(F32)
    q00, q11, q01h = rec[:, 2], rec[:, 3], F32(0.5) * rec[:, 4]
    return q00 < F32(4) * (q00 * q11 - q01h * q01h)


# ---- the fp64 statement ---------------------------------------------------------
def reference_tile(fr, t, g_image, g_alpha=None, g_depth=None, neval=None, flags=None, grads=True, values=None,
                   alpha_fwd=None):
    """One tile.  g_image [3, H, W], g_alpha / g_depth [H, W] or None (numpy);
    neval / flags: the forward's pix_neval / pix_flags [H * W], or None for the
    chain's own decisions.  alpha_fwd: the forward's alpha [H * W], which tells
    a pixel that terminated on its list's last entry from one that ran out of
    entries.  values: fp64 [n, 10] in place of the entries' record values (in
    COMPONENTS order; the skip decisions stay the records').  Returns a dict of
    numpy arrays over the tile's P inside pixels and n entries."""
    ids = fr.entries(t)
    n = len(ids)
    xs, ys, cq = fr.pixels(t)
    P = len(xs)
    pix = ys * fr.W + xs
    rec = fr.records[ids]
    skip = torch.from_numpy(skip_exponent(rec, xs, ys) < SKIP_T) if n else torch.zeros((0, P), dtype=torch.bool)
    base = rec[:, list(REC_COL)].astype(np.float64) if values is None else np.asarray(values, np.float64)
    V = torch.from_numpy(base)[:, None, :].expand(n, P, 10).clone()
    V.requires_grad_(grads)
    X_, Y_ = torch.from_numpy(xs.astype(np.float64)), torch.from_numpy(ys.astype(np.float64))
    bg = torch.from_numpy(fr.bg.astype(np.float64))
    nev = None if neval is None else torch.from_numpy(np.asarray(neval).reshape(-1)[pix].astype(np.int64))
    A = torch.zeros(P, dtype=torch.float64)
    D = torch.zeros(P, dtype=torch.float64)
    acc = bg[None, :].expand(P, 3).clone()  # out_rgb starts at bg (renderer.py:273)
    own = torch.full((P,), n, dtype=torch.int64)
    cs, ws, passes, eles, A_after = [], [], [], [], []
    for i in range(n):
        mx, my, q00, qo, q11, o, r, g, b, z = V[i].unbind(-1)
        dx, dy = X_ - mx, Y_ - my
        s = q00 * dx * dx + qo * dx * dy + q11 * dy * dy
        e = torch.exp(-0.5 * s)
        w = e.clamp(0.0, 1.0)          # (autograd's clamp mask is inclusive: the kernel's w == e)
        u = o * w
        ai = u.clamp(0.0, 1.0)         # (likewise ai == u)
        run = (A.detach() < STOP) if nev is None else (i < nev)
        c = (1.0 - A) * ai
        take = run & ~skip[i] & (c.detach() > 0)  # :336, :340, :345
        c = torch.where(take, c, torch.zeros_like(c))
        acc = acc + c[:, None] * torch.stack([r, g, b], -1)
        D = D + c * z
        A = A + c
        if nev is None:
            own = torch.where(run & (A.detach() >= STOP), torch.full_like(own, i + 1), own)
        cs.append(c.detach())
        ws.append(w.detach())
        passes.append(take & (u.detach() >= 0) & (u.detach() <= 1))
        eles.append(e.detach() <= 1)
        A_after.append(A.detach().clone())
    comp = acc + (1.0 - A)[:, None] * bg  # :359 (bg twice, as the reference)
    own_blocked = torch.cat([~((comp.detach() >= 0) & (comp.detach() <= 1)), ~((A.detach() >= 0) & (A.detach() <= 1))[:, None]], 1)
    if flags is None:
        blocked = own_blocked
    else:
        fl = torch.from_numpy(np.asarray(flags).reshape(-1)[pix].astype(np.int64))
        blocked = torch.stack([(fl >> k) & 1 for k in range(4)], 1).bool()
    image = torch.where(blocked[:, :3], comp.detach().clamp(0, 1), comp)
    alpha = torch.where(blocked[:, 3], A.detach().clamp(0, 1), A)
    den = A + float(EPS)
    depth = D / den
    gi = torch.from_numpy(np.asarray(g_image, np.float64).reshape(3, -1)[:, pix].T.copy())
    ga = None if g_alpha is None else torch.from_numpy(np.asarray(g_alpha, np.float64).reshape(-1)[pix])
    gd = None if g_depth is None else torch.from_numpy(np.asarray(g_depth, np.float64).reshape(-1)[pix])
    out = dict(ids=ids, xs=xs, ys=ys, cq=cq, pix=pix, image=image.detach().numpy(), comp=comp.detach().numpy(),
               alpha=alpha.detach().numpy(), A=A.detach().numpy(), D=D.detach().numpy(),
               blocked=own_blocked.numpy(), neval=(own if nev is None else nev).numpy(),
               A_after=torch.stack(A_after).numpy() if n else np.zeros((0, P)))
    if nev is None:
        out["stopped"] = out["A"] >= STOP
    else:
        out["stopped"] = out["neval"] < n
        if alpha_fwd is not None:
            out["stopped"] |= np.asarray(alpha_fwd, F32).reshape(-1)[pix] >= F32(STOP)
    c_all = torch.stack(cs) if n else torch.zeros((0, P), dtype=torch.float64)
    colabs = V.detach()[:, :, 6:9].abs()
    zabs = V.detach()[:, :, 9].abs()
    out["ncontrib"] = (c_all > 0).sum(0).numpy()
    out["M_image"] = (bg.abs()[None] * (2.0 - A.detach())[:, None] + (c_all[:, :, None] * colabs).sum(0)).numpy()
    Dabs = (c_all * zabs).sum(0)
    out["M_D"] = Dabs.numpy()
    nv = out["neval"]
    running = (np.arange(n)[:, None] < nv[None, :]) & ~skip.numpy()
    Q = fr.cells
    out["live"] = np.stack([running[:, cq == q].any(1) for q in range(Q)], 1) if n else np.zeros((0, Q), bool)
    out["cell_neval"] = np.array([nv[cq == q].max(initial=0) for q in range(Q)])
    out["n_p"] = nv  # the pixel's evaluated entries: the n_p of the bound
    out["n_cell"] = out["cell_neval"]
    if not grads or n == 0:
        return out
    L = (gi * image).sum()
    if ga is not None:
        L = L + (ga * alpha).sum()
    if gd is not None:
        L = L + (gd * depth).sum()
    out["loss"] = float(L.detach())
    L.backward()
    G = V.grad.numpy()
    # ---- the same expressions in absolute values
    Af, denf = A.detach(), den.detach()
    gR = gi.abs() * (~blocked[:, :3])
    gD = torch.zeros(P, dtype=torch.float64) if gd is None else gd.abs() / denf
    gA_abs = (gR * bg.abs()).sum(1)
    if ga is not None:
        gA_abs = gA_abs + ga.abs() * (~blocked[:, 3])
    if gd is not None:
        gA_abs = gA_abs + gd.abs() * Dabs / (denf * denf)
    Xabs = (gR[None] * colabs).sum(2) + gD[None] * zabs                    # [n, P]
    cX = c_all * Xabs
    Pabs = (gR * bg.abs()).sum(1)[None] + torch.cumsum(cX, 0)
    Kabs = (gR * bg.abs()).sum(1) + cX.sum(0)
    Aa = torch.stack(A_after)
    Tnext = 1.0 - Aa
    Tprev = 1.0 - (Aa - c_all)
    tail = Pabs + Kabs[None] + (gA_abs * (1.0 - Af))[None]
    live_form = Xabs + tail / torch.where(Tnext > 0, Tnext, torch.ones_like(Tnext))
    Mdal = Tprev * torch.where(Tnext > 0, live_form, Xabs + gA_abs[None])
    Mdal = Mdal * (c_all > 0)
    dop_abs = Mdal * torch.stack(ws) * torch.stack(passes)
    oabs = V.detach()[:, :, 5].abs()
    dLds_abs = 0.5 * oabs * dop_abs * torch.stack(eles)
    part = np.zeros((n, Q, 10))
    M = np.zeros((n, Q, 10))
    M_rec = np.zeros((n, Q))  # dQ11 of an entry whose row moments are taken about the row nearest its mean
    r64 = rec.astype(np.float64)
    for q in range(Q):
        m = cq == q
        if not m.any():
            continue
        part[:, q] = G[:, m].sum(1)
        x0c, y0c = fr.cell_origin(t, q)
        dxm = np.abs(np.arange(x0c, x0c + 8)[None, :] - r64[:, 0:1]).max(1)
        dym = np.abs(np.arange(y0c, y0c + 8)[None, :] - r64[:, 1:2]).max(1)
        mt = torch.from_numpy(m)
        S = dLds_abs[:, mt].sum(1).numpy()
        q00, q11, qo = np.abs(r64[:, 2]), np.abs(r64[:, 3]), np.abs(r64[:, 4])
        M[:, q, 0] = S * (2 * q00 * dxm + qo * dym)
        M[:, q, 1] = S * (qo * dxm + 2 * q11 * dym)
        M[:, q, 2] = S * dxm * dxm
        M[:, q, 3] = S * dxm * dym
        M[:, q, 4] = S * dym * dym
        rc = np.clip(np.rint(r64[:, 1] - y0c), 0, 7)
        arm = np.abs(y0c + rc - r64[:, 1])[:, None] + np.abs((ys[m] - y0c)[None, :] - rc[:, None])
        M_rec[:, q] = (dLds_abs[:, mt].numpy() * arm * arm).sum(1)
        M[:, q, 5] = dop_abs[:, mt].sum(1).numpy()
        M[:, q, 6:9] = (c_all[:, mt, None] * gR[None, mt]).sum(1).numpy()
        M[:, q, 9] = (c_all[:, mt] * gD[None, mt]).sum(1).numpy()
    out["partials"], out["M"], out["M_dQ11_recentred"] = part, M, M_rec
    return out


def validate_termination(ref, what=""):
    """The forced termination against the fp64 chain: with delta =
    8 (n_p + 1) 2^-24, A >= 0.995 - delta after a pixel's stopping entry and
    A < 0.995 + delta after every entry before it.  Returns the violations."""
    A = ref["A_after"]
    n, P = A.shape
    bad = []
    if n == 0:
        return bad
    nv = ref["neval"]
    delta = 8.0 * (ref["n_p"] + 1) * U24
    idx = np.arange(n)[:, None]
    before = idx < (nv[None, :] - 1)
    over = before & (A >= STOP + delta[None, :])
    for i, p in zip(*np.nonzero(over)):
        bad.append(f"{what} pixel ({ref['xs'][p]}, {ref['ys'][p]}): A = {A[i, p]:.9f} after entry {i}, before its stop {nv[p]}")
    stopped = ref["stopped"]
    for p in np.nonzero(stopped)[0]:
        a = A[nv[p] - 1, p]
        if not a >= STOP - delta[p]:
            bad.append(f"{what} pixel ({ref['xs'][p]}, {ref['ys'][p]}): stopped at entry {nv[p] - 1} with A = {a:.9f}")
    # a pixel that did not stop: its last entry stays below the threshold too
    for p in np.nonzero(~stopped & (nv > 0))[0]:
        if A[nv[p] - 1, p] >= STOP + delta[p]:
            bad.append(f"{what} pixel ({ref['xs'][p]}, {ref['ys'][p]}): ran on with A = {A[nv[p] - 1, p]:.9f}")
    return bad


# ---- the documented formulation in numpy fp32 ----------------------------------
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def emulate_tile(fr, t, g_image, g_alpha=None, g_depth=None, recenter=True):
    """The forward and the backward of one tile in numpy fp32 (its own
    termination and clamp decisions, numpy's exp).  recenter=False: every row
    moment about the cell's row 0 (what the recentring exists to avoid).  Returns image [P, 3],
    alpha, depth, D, flags, neval over the tile's inside pixels and the
    partials [n, cells, 10]."""
    ids = fr.entries(t)
    n = len(ids)
    xs, ys, cq = fr.pixels(t)
    P = len(xs)
    pix = ys * fr.W + xs
    rec = fr.records[ids].astype(F32)
    tq = skip_exponent(rec, xs, ys)
    one, zero = F32(1), F32(0)
    bg = fr.bg.astype(F32)
    o, col, z = rec[:, 5], rec[:, 6:9], rec[:, 9]
    with np.errstate(all="ignore"):
        e_all = np.exp(tq).astype(F32)
        w_all = np.clip(e_all, zero, one)
        u_all = o[:, None] * w_all
        ai_all = np.clip(u_all, zero, one)
        # forward
        A = np.zeros(P, F32)
        D = np.zeros(P, F32)
        acc = np.tile(bg, (P, 1))
        neval = np.full(P, n, np.int64)
        for i in range(n):
            run = A < F32(STOP)
            lv = run & ~(tq[i] < SKIP_T)
            c = (one - A) * np.where(lv, ai_all[i], zero)
            acc = _fma(c[:, None], col[i][None, :], acc)
            A = A + c
            D = _fma(c, z[i], D)
            neval = np.where(run & ~(A < F32(STOP)), i + 1, neval)
        tb = one - A
        comp = acc + tb[:, None] * bg[None, :]
        image = np.clip(comp, zero, one)
        alpha = np.clip(A, zero, one)
        depth = D / (A + EPS)
        blocked = np.concatenate([~((comp >= 0) & (comp <= 1)), ~((A >= 0) & (A <= 1))[:, None]], 1)
        out = dict(image=image, alpha=alpha, depth=depth, D=D, neval=neval, pix=pix,
                   flags=(blocked * np.array([1, 2, 4, 8])).sum(1).astype(np.uint8))
        if n == 0:
            out["partials"] = np.zeros((0, fr.cells, 10), F32)
            return out
        # backward: the pixel header
        gi = np.asarray(g_image, F32).reshape(3, -1)[:, pix].T
        gR = np.where(blocked[:, :3], zero, gi)
        At = alpha
        tbb = one - At
        tr = image - tbb[:, None] * bg[None, :]
        den = At + EPS
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
        G0 = _fma(gA, tbb, -K)
        PG = ((gR[:, 0] * bg[0] + gR[:, 1] * bg[1]) + gR[:, 2] * bg[2]) + G0
        A = np.zeros(P, F32)
        T1 = np.ones(P, F32)
        run = np.ones(P, bool)
        dop = np.zeros((n, P), F32)
        cw = np.zeros((n, P), F32)
        for i in range(n):
            live = run & ~(tq[i] < SKIP_T)
            X = _fma(gR[:, 0], col[i, 0], _fma(gR[:, 1], col[i, 1], _fma(gR[:, 2], col[i, 2], gD * z[i])))
            trans = T1
            c = trans * np.where(live, ai_all[i], zero)
            A = A + c
            PG = _fma(c, X, PG)
            term = ~(A < F32(STOP))
            T1 = one - A
            inv = one / T1
            d_live = _fma(inv, PG, X)
            dal = trans * np.where(term, X + gA, d_live)
            run = run & ~term
            g = np.where(ai_all[i] == u_all[i], dal * w_all[i], zero)
            dop[i] = np.where(c > 0, g, zero)
            cw[i] = np.where(w_all[i] == e_all[i], c, -c)
        out["partials"] = emulate_phase_b(fr, t, rec, xs, ys, cq, dop, cw,
                                          np.concatenate([gR, gD[:, None]], 1), recenter)
    return out


def emulate_phase_b(fr, t, rec, xs, ys, cq, dop, cw, gRD, recenter=True):
    """Phase B of the backward in numpy fp32: the column and row moments per
    (entry, cell) from phase A's dop and +-c [n, P] and the pixels' payload
    cotangents gRD [P, 4].  recenter: True, the rows of an entry with
    sigma_y < 2 px about the row nearest its mean; False, every row moment
    about row 0; "always", every entry recentred (the replays of
    gs_features.hip).  Returns the partials [n, cells, 10]."""
    n = len(rec)
    one, zero = F32(1), F32(0)
    o = rec[:, 5]
    with np.errstate(all="ignore"):
        Q = fr.cells
        part = np.zeros((n, Q, 10), F32)
        q00, q11, qo = rec[:, 2], rec[:, 3], rec[:, 4]
        hop = F32(-0.5) * o
        sm = np.ones(n, bool) if recenter == "always" else small_y(rec) & bool(recenter)
        for q in range(Q):
            m = cq == q
            if not m.any():
                continue
            x0c, y0c = fr.cell_origin(t, q)
            dq = np.zeros((n, 8, 8), F32)   # [entry, row, column]
            cq_ = np.zeros((n, 8, 8), F32)
            pgq = np.zeros((8, 8, 4), F32)
            rr, cc = ys[m] - y0c, xs[m] - x0c
            dq[:, rr, cc], cq_[:, rr, cc], pgq[rr, cc] = dop[:, m], cw[:, m], gRD[m]
            rc = np.where(sm, np.clip(np.rint(rec[:, 1] - F32(y0c)), 0, 7), 0).astype(F32)  # [n]
            S0 = np.zeros((n, 8), F32)
            Soy, Soyy, g5 = S0.copy(), S0.copy(), S0.copy()
            g69 = np.zeros((n, 8, 4), F32)
            for r in range(8):
                ds = np.where(cq_[:, r] > 0, dq[:, r], zero)
                wr = (F32(r) - rc)[:, None]
                S0 = S0 + ds
                Soy = _fma(ds, wr, Soy)
                Soyy = _fma(ds, wr * wr, Soyy)
                g5 = g5 + dq[:, r]
                g69 = _fma(pgq[r][None], np.abs(cq_[:, r])[:, :, None], g69)
            S0, Soy, Soyy = S0 * hop[:, None], Soy * hop[:, None], Soyy * hop[:, None]
            bx = (np.arange(x0c, x0c + 8).astype(F32))[None, :] - rec[:, 0:1]
            by = (F32(y0c) + rc - rec[:, 1])[:, None]
            Sx, Sy = bx * S0, _fma(by, S0, Soy)
            g2, g3 = bx * Sx, bx * Sy
            g4 = _fma(by, _fma(by, S0, F32(2) * Soy), Soyy)
            Sx, Sy, g2, g3, g4, g5 = (v.sum(1, dtype=F32) for v in (Sx, Sy, g2, g3, g4, g5))
            part[:, q, 0] = -(F32(2) * q00 * Sx + qo * Sy)
            part[:, q, 1] = -(qo * Sx + F32(2) * q11 * Sy)
            part[:, q, 2], part[:, q, 3], part[:, q, 4], part[:, q, 5] = g2, g3, g4, g5
            part[:, q, 6:10] = g69.sum(1, dtype=F32)
    return part


def ratio(err, M, n_p):
    """max err / ((n_p + 1) 2^-24 M); inf where M = 0 and err > 0."""
    err, M = np.asarray(err, np.float64), np.asarray(M, np.float64)
    unit = (np.asarray(n_p, np.float64) + 1.0) * U24 * M
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / unit, 0.0)
    return float(np.nan_to_num(r, nan=np.inf).max(initial=0.0))


# ---- frames without a GPU ---------------------------------------------------------
def frame_from_screen(means2d, conics, radii, vis, opacity, colour, z, W, H, L, bg):
    """The reference's binning (renderer.py:261-298) on fp32 screen-space
    values: rectangles of int(centre) +- int(radius) clipped to the image,
    lists in (depth bits, index) order, slots numbered in Gaussian order."""
    n = len(radii)
    means2d, z = np.asarray(means2d, F32), np.asarray(z, F32)
    Q = np.asarray(conics, F32).reshape(n, 4)
    vis = np.asarray(vis, bool)
    ri = np.trunc(np.where(vis, radii, 0)).astype(np.int64)
    icx = np.trunc(np.where(vis, means2d[:, 0], 0)).astype(np.int64)
    icy = np.trunc(np.where(vis, means2d[:, 1], 0)).astype(np.int64)
    x0, x1 = np.maximum(icx - ri, 0), np.minimum(icx + 1 + ri, W)
    y0, y1 = np.maximum(icy - ri, 0), np.minimum(icy + 1 + ri, H)
    ok = vis & (x0 < x1) & (y0 < y1)
    tx0, tx1, ty0, ty1 = x0 // L, (x1 - 1) // L, y0 // L, (y1 - 1) // L
    rec = np.zeros((n, 12), F32)
    rec[:, 0:2] = means2d
    rec[:, 2], rec[:, 3], rec[:, 4] = Q[:, 0], Q[:, 3], Q[:, 1] + Q[:, 2]
    rec[:, 5], rec[:, 6:9], rec[:, 9] = opacity, colour, z
    count = np.where(ok, (tx1 - tx0 + 1) * (ty1 - ty0 + 1), 0)
    offset = np.cumsum(count) - count
    rec[:, 10] = offset.astype(np.uint32).view(F32)
    rec[:, 11] = np.where(ok, tx0 | (ty0 << 12) | ((tx1 - tx0) << 24), 0).astype(np.uint32).view(F32)
    tiles_x, tiles_y = (W + L - 1) // L, (H + L - 1) // L
    idx = np.nonzero(ok)[0]
    order = idx[np.lexsort((idx, z[idx].view(np.uint32)))]
    lists = [[] for _ in range(tiles_x * tiles_y)]
    for g in order:
        for ty in range(ty0[g], ty1[g] + 1):
            for tx in range(tx0[g], tx1[g] + 1):
                lists[ty * tiles_x + tx].append(g)
    lens = np.array([len(l) for l in lists])
    ends = np.cumsum(lens)
    return Frame(rec, np.array([g for l in lists for g in l], np.int64), np.stack([ends - lens, ends], 1), W, H, L,
                 np.asarray(bg, F32))


def cpu_frame(sc):
    """A scene (make_scene) as a host frame: projected in fp64, rounded to fp32.
    sc["fx"], where present, is its focal length in place of FX."""
    W, H = sc["W"], sc["H"]
    fx = float(sc.get("fx", FX))
    cam = PR.Camera(W, H, fx, fx, W * 0.5, H * 0.5, (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0), tile_size=sc["L"])
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    p = PR.project(cam, t64(sc["xyz"]), t64(sc["color_logits"]), t64(sc["opacity"]), cov3d=t64(sc["cov3d"]))
    f32 = lambda k: p[k].numpy().astype(F32)
    return frame_from_screen(f32("means2d"), f32("conics"), f32("radii"), p["vis"].numpy(), f32("opacity"), f32("color"),
                             f32("Z"), W, H, sc["L"], sc["bg"])


# ---- scenes and cases ---------------------------------------------------------------
def make_scene(W, H, L, mx, my, z, sx, sy, theta, opacity, colour, bg=(0.0, 0.0, 0.0)):
    """3-D Gaussians (flat, facing the identity camera) whose projection has
    the given screen-space means, sigmas (px) and rotation."""
    mx, my, z, sx, sy, theta = (np.asarray(v, np.float64) for v in (mx, my, z, sx, sy, theta))
    X, Y = (mx - W * 0.5) * z / FX, -(my - H * 0.5) * z / FX
    c, s = np.cos(theta), np.sin(theta)
    Sxx, Syy = c * c * sx * sx + s * s * sy * sy, s * s * sx * sx + c * c * sy * sy
    Sxy = c * s * (sx * sx - sy * sy)
    k = (z / FX) ** 2
    cov = np.zeros((len(z), 3, 3))
    cov[:, 0, 0], cov[:, 1, 1], cov[:, 0, 1], cov[:, 1, 0] = Sxx * k, Syy * k, -Sxy * k, -Sxy * k
    colour = np.clip(np.asarray(colour, np.float64), 1e-4, 1 - 1e-4)
    return dict(W=W, H=H, L=L, xyz=np.stack([X, Y, z], 1).astype(F32), cov3d=cov.astype(F32),
                opacity=np.asarray(opacity, F32), color_logits=np.log(colour / (1 - colour)).astype(F32),
                bg=np.asarray(bg, F32))


def fd_scene():
    """6 Gaussians on 8x8 pixels, one tile, one cell, away from every
    decision: the scene of the finite-difference tests."""
    rng = np.random.default_rng(5)
    n = 6
    return make_scene(8, 8, 8, rng.uniform(1, 7, n), rng.uniform(1, 7, n), np.linspace(2, 4, n), rng.uniform(2.5, 4, n),
                      rng.uniform(2.5, 4, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.1, 0.4, n),
                      rng.uniform(0.2, 0.8, (n, 3)), bg=(0.05, 0.1, 0.02))


def _random_scene(seed, n, W, H, L, sigma, opacity, bg=(0.0, 0.0, 0.0), thin=0.0):
    """n Gaussians with means on and just around the image; `thin`: the share
    with sigma_y in [0.3, 1.9] px (the rest sigma in `sigma`)."""
    rng = np.random.default_rng(seed)
    mx, my = rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n)
    sx, sy = rng.uniform(*sigma, n), rng.uniform(*sigma, n)
    theta = rng.uniform(-0.6, 0.6, n)
    is_thin = rng.random(n) < thin
    sy = np.where(is_thin, rng.uniform(0.3, 1.9, n), sy)
    theta = np.where(is_thin, rng.uniform(-0.05, 0.05, n), theta)
    return make_scene(W, H, L, mx, my, rng.uniform(2.0, 5.0, n), sx, sy, theta, rng.uniform(*opacity, n),
                      rng.uniform(0.05, 0.95, (n, 3)), bg)


def _subpixel_scene(seed, W, H, L):
    """Sub-pixel rows (sigma_y 0.03 .. 0.3 px) whose means lie 6 to 7 rows
    below their cell's first row, one or two per pixel: about row 0 their dy^2
    moments cancel from 49 S0 to ~0.01 S0."""
    rng = np.random.default_rng(seed)
    mx, my = np.meshgrid(np.arange(3.0, W, 6.0), np.arange(6.5, H, 8.0))
    mx, my = mx.reshape(-1), my.reshape(-1)
    n = len(mx)
    mx, my = mx + rng.uniform(-0.4, 0.4, n), my + rng.uniform(-0.45, 0.45, n)
    return make_scene(W, H, L, mx, my, rng.uniform(2.0, 5.0, n), rng.uniform(0.4, 1.5, n), rng.uniform(0.03, 0.3, n),
                      np.zeros(n), rng.uniform(0.3, 0.9, n), rng.uniform(0.05, 0.95, (n, 3)))


def cotangents(W, H, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (3, H, W)).astype(F32), rng.uniform(-1, 1, (H, W)).astype(F32),
            rng.uniform(-1, 1, (H, W)).astype(F32))


def _set(fr, g, **kw):
    """Mutate floats 0..9 of Gaussian g's record (words 10 and 11 stay)."""
    col = dict(mx=0, my=1, q00=2, q11=3, qo=4, o=5, r=6, g=7, b=8, z=9)
    for k, v in kw.items():
        fr.records[g, col[k]] = F32(v)


def busiest_tile(fr):
    return int(np.argmax(fr.ranges[:, 1] - fr.ranges[:, 0]))


def mutate_opaque(fr):
    """In the busiest tile: entry 0 becomes an opaque (o = 1) sub-pixel
    Gaussian on a pixel centre (A >= 0.995 after the first entry, T1 = 0
    there), and entries 63 and 64 likewise on two other pixels (terminations on
    the last entry of a word and on the first of the next)."""
    t = busiest_tile(fr)
    ids = fr.entries(t)
    assert len(ids) > 66, len(ids)
    x0, y0 = (t % fr.tiles_x) * fr.L, (t // fr.tiles_x) * fr.L
    for k, (ox, oy) in ((0, (1, 1)), (63, (4, 2)), (64, (6, 5))):
        assert ids[k] not in ids[:k]
        _set(fr, ids[k], mx=x0 + ox, my=y0 + oy, q00=2.0, q11=2.0, qo=0.0, o=1.0)
    return dict(tile=t, pixels=[(x0 + 1, y0 + 1, 1), (x0 + 4, y0 + 2, 64), (x0 + 6, y0 + 5, 65)])


def mutate_general(fr):
    """In the busiest tile, entries 2, 5, ... of its list leave simple_entry:
    opacities 1.5, 0, -0.25 and 1e-30, two conics past the conditioning test
    and a non-positive-definite conic with s < 0 at some pixels."""
    t = busiest_tile(fr)
    ids = fr.entries(t)
    assert len(ids) > 40, len(ids)
    x0, y0 = (t % fr.tiles_x) * fr.L, (t // fr.tiles_x) * fr.L
    picks = [int(ids[k]) for k in (2, 5, 9, 12, 17, 21, 30)]
    assert len(set(picks)) == len(picks)
    for g, o in zip(picks[:4], (1.5, 0.0, -0.25, 1e-30)):
        _set(fr, g, o=o)
    _set(fr, picks[4], mx=x0 + 5.3, my=y0 + 4.6, q00=60.0, q11=0.002, qo=0.0, o=0.6)     # a needle along y
    _set(fr, picks[5], mx=x0 + 3.2, my=y0 + 6.1, q00=0.004, q11=60.0, qo=0.3, o=0.5)     # a needle along x, tilted
    _set(fr, picks[6], mx=x0 + 4.4, my=y0 + 3.7, q00=0.06, q11=-0.02, qo=0.0, o=0.3)     # indefinite: e > 1 along y
    return dict(tile=t, picks=picks)


# name -> (scene arguments, mutation or None)
_LOW = (0.004, 0.05)
CASES = {
    "ordinary16": (dict(seed=1, n=300, W=40, H=24, L=16, sigma=(2.5, 7.0), opacity=_LOW), None),
    "ordinary12": (dict(seed=2, n=120, W=30, H=20, L=12, sigma=(2.0, 6.0), opacity=(0.01, 0.2)), None),
    "thin16": (dict(seed=3, n=300, W=40, H=24, L=16, sigma=(3.0, 8.0), opacity=(0.01, 0.15), thin=0.5), None),
    "thin12": (dict(seed=4, n=140, W=30, H=20, L=12, sigma=(3.0, 8.0), opacity=(0.01, 0.2), thin=0.5), None),
    "opaque16": (dict(seed=5, n=300, W=40, H=24, L=16, sigma=(2.5, 7.0), opacity=_LOW), mutate_opaque),
    "opaque12": (dict(seed=6, n=300, W=30, H=20, L=12, sigma=(2.5, 7.0), opacity=_LOW), mutate_opaque),
    "general16": (dict(seed=7, n=300, W=40, H=24, L=16, sigma=(2.5, 7.0), opacity=(0.01, 0.1)), mutate_general),
    "general12": (dict(seed=8, n=140, W=30, H=20, L=12, sigma=(2.5, 7.0), opacity=(0.01, 0.2)), mutate_general),
    "bright16": (dict(seed=9, n=300, W=40, H=24, L=16, sigma=(2.0, 6.0), opacity=(0.02, 0.5),
                      bg=(0.7, 0.2, 0.45)), None),
    "bright12": (dict(seed=10, n=120, W=30, H=20, L=12, sigma=(2.0, 6.0), opacity=(0.02, 0.5),
                      bg=(0.7, 0.2, 0.45)), None),
    "subpixel16": (dict(kind="subpixel", seed=13, W=24, H=16, L=16), None),
    "tile8": (dict(seed=11, n=100, W=30, H=20, L=8, sigma=(1.0, 5.0), opacity=(0.02, 0.6), thin=0.2), None),
    "tile20": (dict(seed=12, n=100, W=30, H=20, L=20, sigma=(1.0, 5.0), opacity=(0.02, 0.6), thin=0.2), None),
}
COTANGENTS = ("all", "no_alpha", "no_depth", "image_only")


def case_scene(name):
    kw = dict(CASES[name][0])
    return _subpixel_scene(**kw) if kw.pop("kind", None) == "subpixel" else _random_scene(**kw)


def case_cotangents(sc, which="all"):
    gi, ga, gd = cotangents(sc["W"], sc["H"])
    return gi, (ga if which in ("all", "no_depth") else None), (gd if which in ("all", "no_alpha") else None)


def whole_frame(fr, fn):
    """fn(t) for every tile with entries."""
    return {t: fn(t) for t in range(fr.tiles_x * fr.tiles_y) if len(fr.entries(t))}
