"""Numpy restatement of the pooled panel regressions (A23, fm_pool) and the panels its tests use.

The definition is the textbook one (Petersen 2009; Cameron, Gelbach and Miller 2011): pooled OLS of
y on [1, x] (or, under month fixed effects, of the within-month demeaned y on the demeaned x), and
for its coefficients the classical, White, month-clustered, firm-clustered and two-way clustered
sandwiches.  Everything here is computed directly in the RAW parametrisation (design [1, x], bread
(D'D)^-1) with means, moments and solves in np.longdouble; the kernel works on centred data and maps
the covariance back, so the two share no algebra beyond the definition."""
import numpy as np

LD = np.longdouble
FITTED, SKIPPED, INF_X, INF_Y, RANK_DEF, NEG_VAR = 0x1, 0x2, 0x4, 0x8, 0x40, 0x100
KINDS = ("classical", "white", "month", "firm", "twoway")
REFIT_REL, CONST_REL = 1e-6, 1e-20


def clip_cols(cols, seg_off, lo, hi):
    """fm_gram's clip: max with lo, then min with hi, per (column, month); a NaN bound is ignored."""
    out = [np.array(c, dtype=np.float64) for c in cols]
    if lo is None:
        return out
    for c in range(len(out)):
        for t in range(len(seg_off) - 1):
            s = slice(int(seg_off[t]), int(seg_off[t + 1]))
            v = out[c][s]
            with np.errstate(invalid="ignore"):
                if not np.isnan(lo[c, t]):
                    v = np.where(v < lo[c, t], lo[c, t], v)
                if not np.isnan(hi[c, t]):
                    v = np.where(v > hi[c, t], hi[c, t], v)
            out[c][s] = v
    return out


def _inv(a):
    """Inverse of a small symmetric positive definite matrix in longdouble (Gauss-Jordan, no pivoting)."""
    n = a.shape[0]
    m = np.concatenate([a.astype(LD), np.eye(n, dtype=LD)], axis=1)
    for k in range(n):
        m[k] = m[k] / m[k, k]
        for r in range(n):
            if r != k:
                m[r] = m[r] - m[r, k] * m[k]
    return m[:, n:]


def _chol_ok(sxx):
    """fm_solve's pivot rule on the centred Sxx: every Cholesky pivot above REFIT_REL of its diagonal entry."""
    a = sxx.astype(LD).copy()
    n = a.shape[0]
    for k in range(n):
        if not (sxx[k, k] > 0 and a[k, k] > LD(REFIT_REL) * sxx[k, k]):
            return False
        a[k + 1:, k] = a[k + 1:, k] / np.sqrt(a[k, k])
        for j in range(k + 1, n):
            a[j:, j] = a[j:, j] - a[j:, k] * a[j, k]
    return True


def _group_meat(u, g):
    """sum over the groups of (sum of the group's scores)(..)'; returns it and the number of groups."""
    keys, inv = np.unique(g, return_inverse=True)
    s = np.zeros((len(keys), u.shape[1]), dtype=LD)
    np.add.at(s, inv, u)
    return s.T @ s, len(keys)


def pooled(cols, seg_off, firm, y, xs, level=None, u=0, lo=None, hi=None, month_fe=False, small_sample=True,
           seg_lo=0, seg_hi=None):
    """One problem.  Returns dict(coef [K+1], se [5, K+1], cov [5, K+1, K+1], stat [8], status, resid [rows],
    cond, N, Gt, Gf); index 0 is the intercept (NaN under month FE)."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    T = len(seg_off) - 1
    seg_hi = T if seg_hi is None else seg_hi
    n = int(seg_off[-1])
    K = len(xs)
    cl = clip_cols([cols[c] for c in list(xs) + [y]], seg_off, None if lo is None else lo[list(xs) + [y]],
                   None if hi is None else hi[list(xs) + [y]])
    month = np.repeat(np.arange(T), np.diff(seg_off))
    use = (month >= seg_lo) & (month < seg_hi)
    for c in list(xs) + [y]:
        use &= ~np.isnan(cols[c])
    if level is not None:
        use &= level >= u
    N = int(use.sum())
    X = np.column_stack([cl[k][use] for k in range(K)]).astype(LD) if N else np.zeros((0, K), dtype=LD)
    Y = cl[K][use].astype(LD)
    mo, fi = month[use], np.asarray(firm)[use]
    Gt, Gf = len(np.unique(mo)), len(np.unique(fi))
    nan = np.nan
    out = dict(coef=np.full(K + 1, nan), se=np.full((5, K + 1), nan), cov=np.full((5, K + 1, K + 1), nan),
               stat=np.array([N, Gt, nan, nan, nan, nan, nan, 0.0]), status=0, resid=np.full(n, nan), cond=nan,
               N=N, Gt=Gt, Gf=Gf)
    p0 = K + 1
    dof = N - K - Gt if month_fe else N - K - 1
    if N < p0 + 1 or dof < 1:
        out["status"] = SKIPPED
        return out
    st = (INF_X if np.isinf(X.astype(np.float64)).any() else 0) | (INF_Y if np.isinf(Y.astype(np.float64)).any() else 0)
    if st:
        out["status"] = st
        return out
    # centred data: about the pooled means, or each month's own
    if month_fe:
        xc, yc = X.copy(), Y.copy()
        for t in np.unique(mo):
            r = mo == t
            xc[r] = X[r] - X[r].sum(axis=0) / LD(r.sum())
            yc[r] = Y[r] - Y[r].sum() / LD(r.sum())
    else:
        xc, yc = X - X.sum(axis=0) / LD(N), Y - Y.sum() / LD(N)
    sxx = xc.T @ xc
    raw = (X * X).sum(axis=0)
    if any(not (sxx[k, k] > LD(CONST_REL) * raw[k]) for k in range(K)) or not _chol_ok(sxx):
        out["status"] = RANK_DEF
        return out
    out["cond"] = float(np.linalg.cond(sxx.astype(np.float64)))
    D = xc if month_fe else np.column_stack([np.ones(N, dtype=LD), X])
    A = _inv(D.T @ D)
    theta = A @ (D.T @ (yc if month_fe else Y))
    e = (yc if month_fe else Y) - D @ theta
    ssr = (e * e).sum()
    syy = (yc * yc).sum()
    s2 = ssr / LD(dof)
    sc = D * e[:, None]
    Mm, _ = _group_meat(sc, mo)
    Mf, _ = _group_meat(sc, fi)
    cw = LD(N) / LD(N - p0) if small_sample else LD(1)
    cn = LD(N - 1) / LD(N - p0) if small_sample else LD(1)
    cm = (LD(Gt) / LD(Gt - 1) * cn if small_sample else LD(1)) if Gt >= 2 else LD(nan)
    cf = (LD(Gf) / LD(Gf - 1) * cn if small_sample else LD(1)) if Gf >= 2 else LD(nan)
    V = [s2 * A, A @ (sc.T @ sc) @ A * cw, A @ Mm @ A * cm, A @ Mf @ A * cf]
    V.append(V[3] + V[2] - V[1])
    off = 1 if month_fe else 0
    status = FITTED
    for k in range(5):
        v = V[k].astype(np.float64)
        out["cov"][k, off:, off:] = v
        d = np.diag(v)
        with np.errstate(invalid="ignore"):
            se = np.sqrt(d)
        if k == 4:
            se = np.where(d > 0, se, nan)
            if (~np.isnan(d) & ~(d > 0)).any():
                status |= NEG_VAR
        out["se"][k, off:] = se
    out["coef"][off:] = theta.astype(np.float64)
    out["stat"] = np.array([N, Gt, Gf, float(1 - ssr / syy), float(ssr), float(s2), dof, 0.0])
    out["status"] = status
    out["resid"][use] = e.astype(np.float64)
    return out


def problems(models):
    """[(model, level, K)] in the engine's order."""
    return [(mi, u, len(xs)) for mi, (y, xs, levels) in enumerate(models) for u in levels]


def pooled_all(d, models, lo=None, hi=None, **kw):
    """Every problem of a panel dict (cols, seg_off, firm, level) -> list of pooled() results."""
    return [pooled(d["cols"], d["seg_off"], d["firm"], models[mi][0], models[mi][1], d.get("level"), u, lo, hi, **kw)
            for mi, u, _ in problems(models)]


def assert_benign(ref, what=""):
    """What the 1e-9 variance tolerance relies on: a well-conditioned Gram, and a two-way variance that
    is at least a tenth of the White one (the subtraction in V_twoway then costs at most one digit)."""
    assert ref["status"] == FITTED, (what, ref["status"])
    assert ref["cond"] < 100, (what, ref["cond"])
    off = int(np.isnan(ref["coef"][0]))
    ratio = np.diag(ref["cov"][4])[off:] / np.diag(ref["cov"][1])[off:]
    assert (ratio >= 0.1).all(), (what, ratio)


# ------------------------------------------------------------------------------------------ panels
PARITY_NCOLS = 18
PARITY_XS, PARITY_Y = (2, 9, 17), 5          # a model narrower than the panel, columns past the 16th
PARITY_MODELS = [(PARITY_Y, PARITY_XS, (0, 1, 2))]
PARITY_LENS = [90, 0, 3, 130, 70, 100, 64, 65, 110]


def _codes(ids):
    return np.unique(ids, return_inverse=True)[1].astype(np.int32)


def parity_panel(seed=11):
    """9 months (one empty, one of 3 rows, one of 130), 150 firms with sparse int64 ids in random
    subsets, K = 3, firm and month components in x (loadings 0.6 / 0.5) and in e (0.7 / 0.6), 3 % NaN in
    x and 2 % in y, three universe levels."""
    rng = np.random.default_rng(seed)
    F, T = 150, len(PARITY_LENS)
    ids_all = np.sort(rng.choice(10 ** 6, size=F, replace=False)).astype(np.int64)
    fx, gx = rng.normal(size=(F, 3)), rng.normal(size=(T, 3))
    fe, ge = rng.normal(size=F), rng.normal(size=T)
    flevel = rng.choice([0, 1, 2], size=F, p=[0.3, 0.3, 0.4]).astype(np.uint8)
    rows_f, rows_t = [], []
    for t, n in enumerate(PARITY_LENS):
        f = np.sort(rng.choice(F, size=n, replace=False))
        rows_f.append(f)
        rows_t.append(np.full(n, t))
    f, t = np.concatenate(rows_f), np.concatenate(rows_t)
    n = len(f)
    x = 0.6 * fx[f] + 0.5 * gx[t] + rng.normal(size=(n, 3))
    e = 0.7 * fe[f] + 0.6 * ge[t] + rng.normal(size=n)
    yv = 0.5 + x @ np.array([0.8, -0.5, 0.3]) + e
    cols = [rng.normal(size=n) for _ in range(PARITY_NCOLS)]
    for c in (0, 7):                                   # columns no model reads: NaN there drops nothing
        cols[c][rng.random(n) < 0.3] = np.nan
    for k, c in enumerate(PARITY_XS):
        cols[c] = x[:, k].copy()
        cols[c][rng.random(n) < 0.03] = np.nan
    cols[PARITY_Y] = yv.copy()
    cols[PARITY_Y][rng.random(n) < 0.02] = np.nan
    seg_off = np.concatenate([[0], np.cumsum(PARITY_LENS)]).astype(np.int64)
    ids = ids_all[f]
    return dict(cols=cols, seg_off=seg_off, ids=ids, firm=_codes(ids), nfirms=len(np.unique(ids)),
                level=flevel[f].copy())


CHECKER_MODELS = [(1, (0,), (0,))]


def checker_panel():
    """The 4 x 4 balanced integer panel: x_it = a_i a_t, e_it = c_i c_t, y = 1 + 2 x + e with a = (1, 1, -1,
    -1) and c = (1, -1, 1, -1).  b = (1, 2) exactly; with the small-sample corrections V_white = 1/14 on
    both coefficients, V_month = V_firm = 0 and V_twoway = -1/14."""
    a, c = np.array([1.0, 1, -1, -1]), np.array([1.0, -1, 1, -1])
    x = np.concatenate([a * a[t] for t in range(4)])
    e = np.concatenate([c * c[t] for t in range(4)])
    ids = np.tile(np.array([10, 20, 30, 40], dtype=np.int64), 4)
    return dict(cols=[x, 1 + 2 * x + e], seg_off=np.arange(0, 17, 4).astype(np.int64), ids=ids, firm=_codes(ids),
                nfirms=4, level=None)


BLOCK_MODELS = [(2, (0, 1), (0,))]


def block_panel(nfirms, block=256, seed=5):
    """5 months, K = 2, ``nfirms`` firms (ids 7 * code + 3).  Month 0 holds every firm; month 1 none of the
    upper half of the codes and month 2 none of the first block's (where there is a second one), so
    firm blocks have months without a row; months 3 and 4 hold random subsets; the last firm is
    present in month 0 alone; with more than one block, every row of the second block's firms has a NaN
    x, so that block adds nothing."""
    rng = np.random.default_rng(seed + nfirms)
    code = np.arange(nfirms)
    present = [np.ones(nfirms, bool), code < (nfirms + 1) // 2,
               code >= block if nfirms > block else rng.random(nfirms) < 0.5,
               rng.random(nfirms) < 0.5, rng.random(nfirms) < 0.7]
    for t in range(1, 5):
        present[t][nfirms - 1] = False
    f = np.concatenate([code[p] for p in present])
    t = np.concatenate([np.full(int(p.sum()), k) for k, p in enumerate(present)])
    n = len(f)
    ff, gg = rng.normal(size=(nfirms, 3)), rng.normal(size=(5, 3))
    x = 0.6 * ff[f, :2] + 0.5 * gg[t, :2] + rng.normal(size=(n, 2))
    e = 0.7 * ff[f, 2] + 0.6 * gg[t, 2] + rng.normal(size=n)
    yv = -0.2 + x @ np.array([0.5, 0.4]) + e
    x0 = x[:, 0].copy()
    if nfirms > block:
        x0[(f >= block) & (f < 2 * block)] = np.nan
    ids = (7 * f + 3).astype(np.int64)
    seg_off = np.concatenate([[0], np.cumsum([int(p.sum()) for p in present])]).astype(np.int64)
    return dict(cols=[x0, x[:, 1].copy(), yv], seg_off=seg_off, ids=ids, firm=f.astype(np.int32), nfirms=nfirms,
                level=None)
