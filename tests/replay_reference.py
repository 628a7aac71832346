"""Independent statements of the three replays of csrc/gs_features.hip (the
feature channels, the contribution statistics, the depth distortion) for
tests/test_replay_stage.py, in the style of blend_reference.reference_tile:
every quantity the seven kernels write, from the frame exactly as they see it.

`chain` (torch fp64, autograd) restates the weights c_i(p) of one tile:

* the `t < kSkipT` skip is decided in numpy fp32 exactly as the kernels do
  (blend_reference.skip_exponent), bit for bit;
* the `A >= 0.995` termination is taken from the forward's pix_neval (or, with
  neval=None, decided by the fp64 chain) and validated by the caller with
  blend_reference.validate_termination;
* the weight and alpha clamp masks are autograd's, inclusive;
* the record values are expanded into leaves per (list entry, pixel), so the
  gradient of a leaf summed over a cell's pixels is the partial a backward
  writes for that (entry, cell) -- no hand-derived backward;
* the replays have no background, no pixel clamp, no alpha or depth cotangent.

From it `feature_tile`, `contrib_tile` and `distortion_tile` state what each
family writes, with M: the same expression with every term replaced by its
absolute value (geometric monomials at their maximum over the cell, dQ11 also
with the recentred arm, which these kernels always take), for the bound

    |x_gpu - x_fp64| <= K (n + 1) 2^-24 M(x),   n the pixel's or cell's evaluated entries.

`emulate_*` are the formulations the kernel comments document, in plain numpy
fp32, built on blend_reference's phases (emulate_phase_b with every entry
recentred): they run without a GPU and measure K.  Their `wrong=` arms are
deliberately wrong formulations, which the statement must be able to refuse."""
import numpy as np
import torch

import blend_reference as B
import distortion_util as DU

F32 = np.float32
U24 = B.U24
CHUNK = 4  # GS_FEATURE_CHUNK


def ratio(err, M, n):
    """blend_reference.ratio, with an error that is not finite counted as inf."""
    err = np.asarray(err, np.float64)
    return B.ratio(np.where(np.isfinite(err), err, np.inf), M, n)


# ---- the fp64 chain -----------------------------------------------------------------
def chain(fr, t, neval=None, values=None, alpha_fwd=None, grads=True):
    """The weights of tile t.  neval: the forward's pix_neval [H * W], or None
    for the chain's own termination; values: fp64 [n, 10] in place of the
    entries' record values (B.COMPONENTS order; the skip stays the records').
    Returns a dict: numpy arrays over the tile's P inside pixels and n entries,
    and under "_V", "_c" the leaves [n, P, 10] and the weights [n, P] with
    their graph."""
    ids = fr.entries(t)
    n = len(ids)
    xs, ys, cq = fr.pixels(t)
    P = len(xs)
    pix = ys * fr.W + xs
    rec = fr.records[ids]
    skip = torch.from_numpy(B.skip_exponent(rec, xs, ys) < B.SKIP_T) if n else torch.zeros((0, P), dtype=torch.bool)
    base = rec[:, list(B.REC_COL)].astype(np.float64) if values is None else np.asarray(values, np.float64)
    V = torch.from_numpy(base)[:, None, :].expand(n, P, 10).clone()
    V.requires_grad_(grads)
    X_, Y_ = torch.from_numpy(xs.astype(np.float64)), torch.from_numpy(ys.astype(np.float64))
    nev = None if neval is None else torch.from_numpy(np.asarray(neval).reshape(-1)[pix].astype(np.int64))
    A = torch.zeros(P, dtype=torch.float64)
    own = torch.full((P,), n, dtype=torch.int64)
    cs, ws, passes, eles, A_after = [], [], [], [], []
    for i in range(n):
        mx, my, q00, qo, q11, o = V[i, :, :6].unbind(-1)
        dx, dy = X_ - mx, Y_ - my
        s = q00 * dx * dx + qo * dx * dy + q11 * dy * dy
        e = torch.exp(-0.5 * s)
        w = e.clamp(0.0, 1.0)
        u = o * w
        ai = u.clamp(0.0, 1.0)
        run = (A.detach() < B.STOP) if nev is None else (i < nev)
        c = (1.0 - A) * ai
        take = run & ~skip[i] & (c.detach() > 0)
        c = torch.where(take, c, torch.zeros_like(c))
        A = A + c
        if nev is None:
            own = torch.where(run & (A.detach() >= B.STOP), torch.full_like(own, i + 1), own)
        cs.append(c)
        ws.append(w.detach())
        passes.append(take & (u.detach() >= 0) & (u.detach() <= 1))
        eles.append(e.detach() <= 1)
        A_after.append(A.detach().clone())
    z2 = torch.zeros((0, P), dtype=torch.float64)
    c_all = torch.stack(cs) if n else z2
    nv = (own if nev is None else nev).numpy()
    k = dict(ids=ids, xs=xs, ys=ys, cq=cq, pix=pix, rec=rec, n=n, P=P, neval=nv, n_p=nv, skip=skip.numpy(),
             A=A.detach().numpy(), A_after=torch.stack(A_after).numpy() if n else np.zeros((0, P)),
             c=c_all.detach().numpy(), _V=V, _c=c_all, _w=torch.stack(ws) if n else z2,
             _passes=torch.stack(passes) if n else z2.bool(), _eles=torch.stack(eles) if n else z2.bool())
    if nev is None:
        k["stopped"] = k["A"] >= B.STOP
    else:
        k["stopped"] = nv < n
        if alpha_fwd is not None:
            k["stopped"] = k["stopped"] | (np.asarray(alpha_fwd, F32).reshape(-1)[pix] >= F32(B.STOP))
    running = (np.arange(n)[:, None] < nv[None, :]) & ~k["skip"]
    Q = fr.cells
    k["live"] = np.stack([running[:, cq == q].any(1) for q in range(Q)], 1) if n else np.zeros((0, Q), bool)
    k["cell_neval"] = np.array([nv[cq == q].max(initial=0) for q in range(Q)])
    k["n_cell"] = k["cell_neval"]
    k["ncontrib"] = (k["c"] > 0).sum(0)
    return k


def _geometry_bounds(fr, t, k, Xabs):
    """M of the six geometry values [n, cells, 6] and of dQ11 with the
    recentred arm [n, cells], for a backward whose dL/dc_i has the absolute
    expression Xabs [n, P] (reference_tile's, without background and alpha)."""
    n, Q = k["n"], fr.cells
    c = torch.from_numpy(k["c"])
    Aa = torch.from_numpy(k["A_after"])
    cX = c * Xabs
    tail = torch.cumsum(cX, 0) + cX.sum(0)[None]
    Tnext = 1.0 - Aa
    Tprev = 1.0 - (Aa - c)
    live_form = Xabs + tail / torch.where(Tnext > 0, Tnext, torch.ones_like(Tnext))
    Mdal = Tprev * torch.where(Tnext > 0, live_form, Xabs) * (c > 0)
    dop_abs = Mdal * k["_w"] * k["_passes"]
    oabs = k["_V"].detach()[:, :, 5].abs()
    dLds_abs = (0.5 * oabs * dop_abs * k["_eles"]).numpy()
    dop_abs = dop_abs.numpy()
    M, M_rec = np.zeros((n, Q, 6)), np.zeros((n, Q))
    r64 = k["rec"].astype(np.float64)
    q00, q11, qo = np.abs(r64[:, 2]), np.abs(r64[:, 3]), np.abs(r64[:, 4])
    for q in range(Q):
        m = k["cq"] == q
        if not m.any():
            continue
        x0c, y0c = fr.cell_origin(t, q)
        dxm = np.abs(np.arange(x0c, x0c + 8)[None, :] - r64[:, 0:1]).max(1)
        dym = np.abs(np.arange(y0c, y0c + 8)[None, :] - r64[:, 1:2]).max(1)
        S = dLds_abs[:, m].sum(1)
        M[:, q, 0] = S * (2 * q00 * dxm + qo * dym)
        M[:, q, 1] = S * (qo * dxm + 2 * q11 * dym)
        M[:, q, 2] = S * dxm * dxm
        M[:, q, 3] = S * dxm * dym
        M[:, q, 4] = S * dym * dym
        rc = np.clip(np.rint(r64[:, 1] - y0c), 0, 7)
        arm = np.abs(y0c + rc - r64[:, 1])[:, None] + np.abs((k["ys"][m] - y0c)[None, :] - rc[:, None])
        M_rec[:, q] = (dLds_abs[:, m] * arm * arm).sum(1)
        M[:, q, 5] = dop_abs[:, m].sum(1)
    return M, M_rec


def _cell_sums(fr, k, G):
    """A per-(entry, pixel) array [n, P, ...] summed over each cell's pixels."""
    out = np.zeros((k["n"], fr.cells) + G.shape[2:])
    for q in range(fr.cells):
        m = k["cq"] == q
        if m.any():
            out[:, q] = G[:, m].sum(1)
    return out


def chunks_of(C):
    return (C + CHUNK - 1) // CHUNK


# ---- features ------------------------------------------------------------------------
def feature_tile(fr, t, k, F, g_out=None, fvalues=None):
    """out[p, ch] = sum_i c_i F[g_i, ch] over chain k of tile t; F [N, C] fp64.
    With the cotangent g_out [C, H, W]: per chunk j of four channels the
    partials [chunks, n, cells, 10] = (dmu_x, dmu_y, dQ00, dQ01, dQ11,
    d_opacity, dF_4j .. dF_4j+3) of L_j = sum over the chunk's channels, the
    columns past C exactly 0; their M; and "loss" = sum_j L_j."""
    n, P = k["n"], k["P"]
    F = np.asarray(F, np.float64)
    C = F.shape[1]
    Fi = F[k["ids"]] if fvalues is None else np.asarray(fvalues, np.float64)
    grads = g_out is not None and n > 0
    Fv = torch.from_numpy(Fi)[:, None, :].expand(n, P, C).clone()
    Fv.requires_grad_(grads)
    c = k["_c"]
    out = (c[:, :, None] * Fv).sum(0)
    cd = torch.from_numpy(k["c"])
    res = dict(out=out.detach().numpy(), M_out=(cd[:, :, None] * Fv.detach().abs()).sum(0).numpy())
    if not grads:
        return res
    J, Q = chunks_of(C), fr.cells
    g = torch.from_numpy(np.asarray(g_out, np.float64).reshape(C, -1)[:, k["pix"]].T.copy())  # [P, C]
    part, M, M_rec = np.zeros((J, n, Q, 10)), np.zeros((J, n, Q, 10)), np.zeros((J, n, Q))
    loss = 0.0
    for j in range(J):
        ks = list(range(CHUNK * j, min(CHUNK * j + CHUNK, C)))
        L = (g[:, ks] * out[:, ks]).sum()
        loss += float(L.detach())
        GV, GF = torch.autograd.grad(L, [k["_V"], Fv], retain_graph=True)
        part[j, :, :, :6] = _cell_sums(fr, k, GV.numpy()[:, :, :6])
        part[j, :, :, 6:6 + len(ks)] = _cell_sums(fr, k, GF.numpy()[:, :, ks])
        Xabs = (g[None, :, ks].abs() * Fv.detach()[:, :, ks].abs()).sum(2)
        M[j, :, :, :6], M_rec[j] = _geometry_bounds(fr, t, k, Xabs)
        M[j, :, :, 6:6 + len(ks)] = _cell_sums(fr, k, (cd[:, :, None] * g[None, :, ks].abs()).numpy())
    res.update(partials=part, M=M, M_dQ11_recentred=M_rec, loss=loss)
    return res


# ---- contributions -------------------------------------------------------------------
def contrib_tile(fr, k):
    """Per (entry, cell): sum_p c, max_p c, #{p : c > 0}; per pixel the
    dominant entry (the first in list order among equals), its Gaussian (-1
    where no entry contributes) and its c, and the two largest c."""
    n, P, Q = k["n"], k["P"], fr.cells
    c = k["c"]
    s, mx, cnt = np.zeros((n, Q)), np.zeros((n, Q)), np.zeros((n, Q), np.int64)
    for q in range(Q):
        m = k["cq"] == q
        if m.any():
            s[:, q], mx[:, q], cnt[:, q] = c[:, m].sum(1), c[:, m].max(1), (c[:, m] > 0).sum(1)
    if n:
        dom = c.argmax(0)
        top1 = c.max(0)
        rest = c.copy()
        rest[dom, np.arange(P)] = -1.0
        top2 = np.maximum(rest.max(0), 0.0) if n > 1 else np.zeros(P)
        second = rest.argmax(0) if n > 1 else dom
    else:
        dom, top1, top2, second = np.zeros(P, np.int64), np.zeros(P), np.zeros(P), np.zeros(P, np.int64)
    ids = np.asarray(k["ids"])
    return dict(sum=s, max=mx, count=cnt, dom_entry=dom, dom_id=np.where(top1 > 0, ids[dom] if n else -1, -1),
                second_id=np.where(top2 > 0, ids[second] if n else -1, -1), top1=top1, top2=top2)


# ---- distortion ------------------------------------------------------------------------
def kappa32(near_far):
    """near_far_kappa of gs_features.hip: far near / (far - near) in fp64 of the fp32 bounds, rounded."""
    near, far = (float(F32(v)) for v in near_far)
    return F32(far * near / (far - near))


def distortion_tile(fr, t, k, near_far=None, g=None):
    """Per pixel D = 2 sum_i c_i (m_i A_{i-1} - S_{i-1}) (the prefix form),
    A_n, S_n relative to the pixel's first contributor, the median entry (the
    first with c > 0 after whose addition A >= 0.5, else the last with c > 0)
    with the margin |A_i - 0.5| at the deciding entries; with the cotangent g
    [H, W] the partials [n, cells, 10] = (six geometry values, 0, 0, 0, d_z)."""
    n, P = k["n"], k["P"]
    V = k["_V"]
    c = k["_c"]
    z = V[:, :, 9]
    m = z if near_far is None else DU.mapped(z, tuple(float(F32(v)) for v in near_far))
    cd = k["c"]
    pos = cd > 0
    has = pos.any(0)
    first = np.where(has, pos.argmax(0), 0) if n else np.zeros(P, np.int64)
    cols = np.arange(P)
    # relative to the pixel's first contributor (D does not change under the shift; in fp64 as in fp32 the
    # prefix form then has no term larger than the pixel's own depth spread)
    msh = m - m[torch.from_numpy(first), torch.from_numpy(cols)][None, :] if n else m
    cm = c * msh
    A, S = torch.cumsum(c, 0), torch.cumsum(cm, 0)
    D = 2.0 * (c * (msh * (A - c) - (S - cm))).sum(0)
    md, ms = m.detach().numpy(), msh.detach().numpy()
    Ad = np.cumsum(cd, 0)
    Ap = Ad - cd
    Sabs = np.cumsum(cd * np.abs(ms), 0)
    res = dict(D=D.detach().numpy(), A=Ad[-1] if n else np.zeros(P), S=(cd * ms).sum(0), c=cd, m=md,
               M_D=2.0 * (cd * (np.abs(ms) * Ap + (Sabs - cd * np.abs(ms)))).sum(0),
               M_S=Sabs[-1] if n else np.zeros(P))
    # the median entry and its margin
    hit = pos & (Ad >= 0.5)
    took = hit.any(0)
    last = np.where(has, n - 1 - pos[::-1].argmax(0), -1) if n else np.full(P, -1)
    med = np.where(took, hit.argmax(0), last) if n else last
    margin = np.full(P, np.inf)
    prev, nxt = med.copy(), med.copy()
    for p in range(P):
        if med[p] < 0:
            continue
        i = int(med[p])
        before = np.nonzero(pos[:i, p])[0]
        after = np.nonzero(pos[i + 1:, p])[0]
        if took[p]:
            margin[p] = Ad[i, p] - 0.5
            if len(before):
                margin[p] = min(margin[p], 0.5 - Ad[before[-1], p])
        else:
            margin[p] = 0.5 - Ad[i, p]
        prev[p] = before[-1] if len(before) else i
        nxt[p] = i + 1 + after[0] if len(after) else i
    res.update(median_entry=med, median_margin=margin, median_prev=prev, median_next=nxt, ncontrib=pos.sum(0),
               A_run=Ad)
    if g is None or n == 0:
        return res
    gp = torch.from_numpy(np.asarray(g, np.float64).reshape(-1)[k["pix"]])
    L = (gp * D).sum()
    res["loss"] = float(L.detach())
    GV, Gm = torch.autograd.grad(L, [V, m], retain_graph=True)
    GV = GV.numpy()
    part = np.zeros((n, fr.cells, 10))
    part[:, :, :6] = _cell_sums(fr, k, GV[:, :, :6])
    part[:, :, 9] = _cell_sums(fr, k, GV[:, :, 9])
    res["dL_dm"] = Gm.numpy()
    ga = np.abs(np.asarray(g, np.float64).reshape(-1)[k["pix"]])[None, :]
    An = Ad[-1][None, :]
    Sp = Sabs - cd * np.abs(ms)
    Xabs = 2.0 * ga * (np.abs(ms) * (Ap + Ad + An) + Sabs[-1][None, :] + Sabs + Sp)
    M = np.zeros((n, fr.cells, 10))
    M[:, :, :6], M_rec = _geometry_bounds(fr, t, k, torch.from_numpy(Xabs))
    zd = z.detach().numpy()
    dmdz = np.ones_like(zd) if near_far is None else float(kappa32(near_far)) / (zd * zd)
    M[:, :, 9] = _cell_sums(fr, k, 2.0 * ga * cd * (Ap + Ad + An) * np.abs(dmdz))
    res.update(partials=part, M=M, M_dQ11_recentred=M_rec)
    return res


def median_consistent(ds, entry, delta):
    """Whether list entry `entry` [P] (-1: none) can be the median of a chain
    whose running A lies within delta [P] of the statement's: a contributor,
    the previous contributor's A below 0.5 + delta, its own A at least
    0.5 - delta unless it is the last contributor."""
    c, A = ds["c"], ds["A_run"]
    n, P = c.shape
    ok = np.zeros(P, bool)
    for p in range(P):
        pos = np.nonzero(c[:, p] > 0)[0]
        j = int(entry[p])
        if not len(pos):
            ok[p] = j == -1
            continue
        at = np.nonzero(pos == j)[0]
        if not len(at):
            continue
        r = int(at[0])
        before = r == 0 or A[pos[r - 1], p] < 0.5 + delta[p]
        ok[p] = before and (A[j, p] >= 0.5 - delta[p] or r == len(pos) - 1)
    return ok


# ---- the documented formulations in numpy fp32 -------------------------------------------
def emulate_chain(fr, t):
    """The forward replay of one tile in numpy fp32 (k_feat_fwd's weights): the
    values every replay shares.  Its own termination decisions."""
    ids = fr.entries(t)
    n = len(ids)
    xs, ys, cq = fr.pixels(t)
    P = len(xs)
    rec = fr.records[ids].astype(F32)
    tq = B.skip_exponent(rec, xs, ys)
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        e = np.exp(tq).astype(F32)
        w = np.clip(e, zero, one)
        u = rec[:, 5:6] * w
        ai = np.clip(u, zero, one)
        A = np.zeros(P, F32)
        c = np.zeros((n, P), F32)
        run_before = np.zeros((n, P), bool)
        neval = np.full(P, n, np.int64)
        for i in range(n):
            run = A < F32(B.STOP)
            run_before[i] = run
            lv = run & ~(tq[i] < B.SKIP_T)
            c[i] = (one - A) * np.where(lv, ai[i], zero)
            A = A + c[i]
            neval = np.where(run & ~(A < F32(B.STOP)), i + 1, neval)
    return dict(ids=ids, n=n, P=P, xs=xs, ys=ys, cq=cq, pix=ys * fr.W + xs, rec=rec, tq=tq, e=e, w=w, u=u, ai=ai, c=c,
                A=A, neval=neval, run_before=run_before)


def _phase_a(em, X_of, PG0, wrong=None):
    """Phase A of the replays' backward in fp32: the pixel's chain again with
    PG = P - K carried as one sum.  X_of(i, c, A_before, A_after) -> X [P] (and
    what phase B needs besides).  Returns dop, +-c [n, P]."""
    n, P = em["n"], em["P"]
    one, zero = F32(1), F32(0)
    A = np.zeros(P, F32)
    T1 = np.ones(P, F32)
    run = np.ones(P, bool)
    PG = PG0.astype(F32)
    dop, cw = np.zeros((n, P), F32), np.zeros((n, P), F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            live = run & ~(em["tq"][i] < B.SKIP_T)
            trans = T1
            c = trans * np.where(live, em["ai"][i], zero)
            Ap = A
            A = A + c
            X = X_of(i, c, Ap, A)
            PG = B._fma(c, X, PG)
            term = ~(A < F32(B.STOP))
            T1 = one - A
            inv = one / T1
            d_live = B._fma(inv, PG, X)
            dal = trans * (d_live if wrong == "terminating_live" else np.where(term, X, d_live))
            run = run & ~term
            g = np.where(em["ai"][i] == em["u"][i], dal * em["w"][i], zero)
            dop[i] = np.where(c > 0, g, zero)
            cw[i] = np.where(em["w"][i] == em["e"][i], c, -c)
    return dop, cw


def emulate_features(fr, t, F, g_out=None, wrong=None, guard=None):
    """k_feat_fwd and k_feat_bwd of one tile in numpy fp32: out [P, C] and,
    with g_out [C, H, W], the partials [chunks, n, cells, 10].  wrong:
    "row0" -- row moments about row 0; "terminating_live" -- the terminating
    entry given X + PG / T; "unmasked" -- the last chunk's cotangent of the
    channels >= C read from `guard` [H, W] instead of masked to 0."""
    em = emulate_chain(fr, t)
    n, P = em["n"], em["P"]
    F = np.asarray(F, F32)
    C = F.shape[1]
    J = chunks_of(C)
    Fp = np.zeros((n, J * CHUNK), F32)
    Fp[:, :C] = F[em["ids"]]
    out = np.zeros((P, J * CHUNK), F32)
    for i in range(n):
        out = B._fma(em["c"][i][:, None], Fp[i][None, :], out)
    res = dict(em=em, out=out[:, :C])
    if g_out is None or n == 0:
        return res
    gp = np.zeros((P, J * CHUNK), F32)
    gp[:, :C] = np.asarray(g_out, F32).reshape(C, -1)[:, em["pix"]].T
    if wrong == "unmasked":
        gp[:, C:] = np.asarray(guard, F32).reshape(-1)[em["pix"]][:, None]
    part = np.zeros((J, n, fr.cells, 10), F32)
    for j in range(J):
        gF, oF, Fj = gp[:, CHUNK * j:CHUNK * j + CHUNK], out[:, CHUNK * j:CHUNK * j + CHUNK], Fp[:, CHUNK * j:CHUNK * j + CHUNK]
        K = (gF[:, 0] * oF[:, 0] + gF[:, 1] * oF[:, 1]) + (gF[:, 2] * oF[:, 2] + gF[:, 3] * oF[:, 3])
        X_of = lambda i, c, Ap, A: B._fma(gF[:, 0], Fj[i, 0], B._fma(gF[:, 1], Fj[i, 1],
                                                                      B._fma(gF[:, 2], Fj[i, 2], gF[:, 3] * Fj[i, 3])))
        dop, cw = _phase_a(em, X_of, -K, wrong)
        part[j] = B.emulate_phase_b(fr, t, em["rec"], em["xs"], em["ys"], em["cq"], dop, cw, gF,
                                    False if wrong == "row0" else "always")
    res["partials"] = part
    return res


def _cell_grid(em, fr, t, q, v):
    """v [n, P] on cell q's 8x8 grid [n, row, column], zero outside."""
    m = em["cq"] == q
    x0c, y0c = fr.cell_origin(t, q)
    g = np.zeros((em["n"], 8, 8), F32)
    g[:, em["ys"][m] - y0c, em["xs"][m] - x0c] = v[:, m]
    return g


def _column_then_lanes(g, op="sum"):
    """k_contrib's phase B order: rows 0..7 of a column in order, then the eight columns."""
    acc = g[:, 0].copy()
    for r in range(1, 8):
        acc = acc + g[:, r] if op == "sum" else np.maximum(acc, g[:, r])
    return acc.sum(1, dtype=F32) if op == "sum" else acc.max(1)


def emulate_contrib(fr, t):
    """k_contrib of one tile in numpy fp32: per (entry, cell) sum, max, count;
    per pixel the dominant entry's Gaussian and weight."""
    em = emulate_chain(fr, t)
    n, P, Q = em["n"], em["P"], fr.cells
    s, mx, cnt = np.zeros((n, Q), F32), np.zeros((n, Q), F32), np.zeros((n, Q), np.int64)
    for q in range(Q):
        if (em["cq"] == q).any():
            g = _cell_grid(em, fr, t, q, em["c"])
            s[:, q], mx[:, q], cnt[:, q] = _column_then_lanes(g), _column_then_lanes(g, "max"), (g > 0).sum((1, 2))
    best, best_id = np.zeros(P, F32), np.full(P, -1, np.int64)
    for i in range(n):
        better = em["c"][i] > best
        best, best_id = np.where(better, em["c"][i], best), np.where(better, em["ids"][i], best_id)
    return dict(em=em, sum=s, max=mx, count=cnt, dom_id=best_id, dom_w=best)


def emulate_distortion(fr, t, near_far=None, g=None, wrong=None):
    """k_dist_fwd and k_dist_bwd of one tile in numpy fp32: D, A_n, S_n, the
    median entry per pixel and, with g [H, W], the partials [n, cells, 10].
    wrong: "unshifted" -- the depths not taken relative to the first
    contributor; "row0" / "terminating_live" as emulate_features."""
    em = emulate_chain(fr, t)
    n, P = em["n"], em["P"]
    one, zero = F32(1), F32(0)
    z = em["rec"][:, 9]
    inv = near_far is not None
    with np.errstate(all="ignore"):
        if inv:
            kap = kappa32(near_far)
            qz, rz = kap / z, one / z
            m_un = (F32(near_far[1]) * (z - F32(near_far[0])) / ((F32(near_far[1]) - F32(near_far[0])) * z)).astype(F32)
        else:
            qz, rz, m_un = np.ones(n, F32), np.ones(n, F32), z
        A, S, D = np.zeros(P, F32), np.zeros(P, F32), np.zeros(P, F32)
        zf, rf = np.zeros(P, F32), np.ones(P, F32)
        med = np.full(P, -1, np.int64)
        md_all = np.zeros((n, P), F32)
        for i in range(n):
            c = em["c"][i]
            have = A > 0
            zf = np.where(have, zf, z[i])
            md = z[i] - zf
            if inv:
                rf = np.where(have, rf, rz[i])
                md = md * (qz[i] * rf)
            if wrong == "unshifted":
                md = np.full(P, m_un[i], F32)
            md_all[i] = md
            D = B._fma(c, B._fma(md, A, -S), D)
            S = B._fma(c, md, S)
            med = np.where((c > 0) & (A < F32(0.5)), i, med)
            A = A + c
        dist = F32(2) * D
        res = dict(em=em, D=dist, A=A, S=S, median_entry=med)
        if g is None or n == 0:
            return res
        g2 = F32(2) * np.asarray(g, F32).reshape(-1)[em["pix"]]
        An, Sn = A, S
        state = dict(S=np.zeros(P, F32))
        dm = np.zeros((n, P), F32)

        def X_of(i, c, Ap, Aq):
            Sp = state["S"]
            Snew = B._fma(c, md_all[i], Sp)
            state["S"] = Snew
            u3 = (Ap + Aq) - An
            dm[i] = (g2 * c) * u3
            return g2 * B._fma(md_all[i], u3, (Sn - Snew) - Sp)

        dop, cw = _phase_a(em, X_of, -(g2 * dist), wrong)
        part = B.emulate_phase_b(fr, t, em["rec"], em["xs"], em["ys"], em["cq"], dop, cw, np.zeros((P, 4), F32),
                                 False if wrong == "row0" else "always")
        part[:, :, 6:10] = zero
        for q in range(fr.cells):
            if (em["cq"] == q).any():
                g9 = _column_then_lanes(_cell_grid(em, fr, t, q, dm))
                part[:, q, 9] = g9 * (qz * rz) if inv else g9
        res["partials"] = part
    return res
