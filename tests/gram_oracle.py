"""Plain-numpy reference of fm_gram's per-(chunk, bucket) partial Grams and of the problem Gram
fm_solve forms from them (test infrastructure only).

A row's bucket is ``pattern_id * nlevels + level``: the pattern is the set of models whose column
mask holds no NaN in the row (``lut`` from engine.plan_patterns maps it to an id, 255 drops the
row) and the level is the row's own universe level.  z = [1, (clip(x) - shift) * inv_scale ...],
every operation rounded once in float64 (the library is built without FMA contraction); a NaN
bound is no bound.  Per (chunk, bucket) the reference is the packed upper triangle of Z'Z, entry
(i, j >= i) at ``i*zw - i*(i-1)/2 + (j-i)``: exactly, in int64, where z is integer-valued up to a
power of two, and in longdouble otherwise, with sum |z_i z_j| for the error bound.
"""
import numpy as np


def packed_index(i, j, zw):
    """Packed position of entry (i, j) (either order) of a zw x zw upper triangle."""
    i, j = (i, j) if i <= j else (j, i)
    return i * zw - (i * (i - 1)) // 2 + (j - i)


def packed_pairs(zw):
    """(I, J) index arrays of the packed entries, in packed order."""
    I, J = np.triu_indices(zw)
    return I, J


def zwidth(ncols):
    return 16 if ncols <= 15 else 32


def row_buckets(cols, level, nlevels, masks, lut):
    """Per row: (pattern id or -1 where the row is dropped, bucket or -1)."""
    cols = np.asarray(cols, dtype=np.float64)
    n = cols.shape[1]
    nn = np.zeros(n, dtype=np.int64)
    for c in range(cols.shape[0]):
        nn |= (~np.isnan(cols[c])).astype(np.int64) << c
    pat = np.zeros(n, dtype=np.int64)
    for m, mask in enumerate(masks):
        pat |= ((nn & mask) == mask).astype(np.int64) << m
    pid = np.asarray(lut, dtype=np.int64)[pat]
    pid = np.where(pid == 255, -1, pid)
    lvl = np.zeros(n, dtype=np.int64) if level is None else np.asarray(level, dtype=np.int64)
    assert lvl.min(initial=0) >= 0 and lvl.max(initial=0) < nlevels
    return pid, np.where(pid >= 0, pid * nlevels + lvl, -1)


def z_values(cols, seg_off, lo=None, hi=None, shift=None, inv_scale=None):
    """Z [n, zw] float64: column 0 ones, column 1 + c the transformed panel column c, columns past
    ncols zero (never compared).  lo / hi / shift / inv_scale: [ncols][nseg] or None."""
    cols = np.asarray(cols, dtype=np.float64)
    C, n = cols.shape
    seg = np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))
    Z = np.zeros((n, zwidth(C)), dtype=np.float64)
    Z[:, 0] = 1.0
    with np.errstate(invalid="ignore"):
        for c in range(C):
            x = cols[c].copy()
            if lo is not None:
                x = np.fmax(x, np.asarray(lo[c], dtype=np.float64)[seg])   # fmax / fmin: a NaN bound is no bound
            if hi is not None:
                x = np.fmin(x, np.asarray(hi[c], dtype=np.float64)[seg])
            if shift is not None:
                x = x - np.asarray(shift[c], dtype=np.float64)[seg]
            else:
                x = x - 0.0
            if inv_scale is not None:
                x = x * np.asarray(inv_scale[c], dtype=np.float64)[seg]
            Z[:, 1 + c] = x
    return Z


def pattern_columns(masks, pats):
    """Per pattern, the union of its models' column masks."""
    out = []
    for P in pats:
        u = 0
        for m, mask in enumerate(masks):
            if (P >> m) & 1:
                u |= mask
        out.append(u)
    return out


def defined_mask(masks, pats, nlevels, zw):
    """bool [nb, PK]: entry (i, j) of bucket (pattern P, level) is defined when i and j are each 0
    or 1 + c with column c in the union of the masks of P's models."""
    I, J = packed_pairs(zw)
    out = np.zeros((len(pats) * nlevels, len(I)), dtype=bool)
    for p, u in enumerate(pattern_columns(masks, pats)):
        ok = np.array([z == 0 or bool((u >> (z - 1)) & 1) for z in range(zw)])
        out[p * nlevels:(p + 1) * nlevels] = ok[I] & ok[J]
    return out


def _pow2_scale(Z):
    """The smallest power of two s with Z * s integer-valued (Z finite), or None."""
    for k in range(0, 24):
        s = float(2 ** k)
        if np.array_equal(np.rint(Z * s), Z * s):
            return s
    return None


class GramRef:
    """n [nchunks, nb] row counts, gram / absum [nchunks, nb, PK] (gram: float64 holding exact
    values when ``exact``, else longdouble), bucket [n] and Z [n, zw]."""

    def __init__(self, n, gram, absum, bucket, Z, exact, zw, nb):
        self.n, self.gram, self.absum = n, gram, absum
        self.bucket, self.Z, self.exact, self.zw, self.nb = bucket, Z, exact, zw, nb


def gram_reference(cols, seg_off, chunk_seg, chunk_row, lo, hi, shift, inv_scale, level, nlevels, masks,
                   lut, npatterns, exact=True):
    """The reference partials of one model group under one chunk plan.  ``exact``: z must be
    integer-valued up to a power of two on every column its bucket defines (don't-care values
    -- NaN, and whatever a NaN went through -- count as 0); the Gram is then formed in int64."""
    cols = np.asarray(cols, dtype=np.float64)
    zw = zwidth(cols.shape[0])
    I, J = packed_pairs(zw)
    nb = npatterns * nlevels
    _, bucket = row_buckets(cols, level, nlevels, masks, lut)
    Z = z_values(cols, seg_off, lo, hi, shift, inv_scale)
    chunk_row = np.asarray(chunk_row, dtype=np.int64).reshape(-1, 2)
    nch = len(chunk_row)
    cnt = np.zeros((nch, nb), dtype=np.int64)
    absum = np.zeros((nch, nb, len(I)), dtype=np.longdouble)
    if exact:
        Zf = np.where(np.isfinite(Z), Z, 0.0)
        s = _pow2_scale(Zf)
        assert s is not None, "exact reference: z is not integer-valued up to a power of two"
        Zi = np.rint(Zf * s).astype(np.int64)
        gram = np.zeros((nch, nb, len(I)), dtype=np.float64)
    else:
        Zl = Z.astype(np.longdouble)
        gram = np.zeros((nch, nb, len(I)), dtype=np.longdouble)
    for k, (r0, r1) in enumerate(chunk_row):
        assert seg_off[chunk_seg[k]] <= r0 <= r1 <= seg_off[chunk_seg[k] + 1]
        bk = bucket[r0:r1]
        for b in range(nb):
            rows = r0 + np.flatnonzero(bk == b)
            cnt[k, b] = len(rows)
            if not len(rows):
                continue
            if exact:
                G = Zi[rows].T @ Zi[rows]
                A = np.abs(Zi[rows]).T @ np.abs(Zi[rows])
                assert A.max() < 2 ** 53   # the int64 sums are exact and so is their float64 image
                gram[k, b] = G[I, J].astype(np.float64) / (s * s)
                absum[k, b] = A[I, J].astype(np.longdouble) / (s * s)
            else:
                with np.errstate(invalid="ignore"):
                    P = Zl[rows][:, I] * Zl[rows][:, J]
                    gram[k, b] = P.sum(axis=0)
                    absum[k, b] = np.abs(P).sum(axis=0)
    return GramRef(cnt, gram, absum, bucket, Z, exact, zw, nb)


CLASS_FINITE, CLASS_NAN, CLASS_PINF, CLASS_NINF = 0, 1, 2, 3


def classify(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), CLASS_NAN, np.where(x == np.inf, CLASS_PINF,
                    np.where(x == -np.inf, CLASS_NINF, CLASS_FINITE)))


def gram_classes(Z, rows, zw):
    """Class and value of every packed entry of the Gram of ``rows`` when z may hold +-inf: NaN
    where a product is NaN or products of both infinite signs occur, else the infinity that
    occurs, else the (exact, integer data) finite sum.  None of it depends on the summation order."""
    I, J = packed_pairs(zw)
    with np.errstate(invalid="ignore"):
        P = Z[rows][:, I] * Z[rows][:, J]
    nan = np.isnan(P).any(axis=0)
    pos = (P == np.inf).any(axis=0)
    neg = (P == -np.inf).any(axis=0)
    cls = np.where(nan | (pos & neg), CLASS_NAN, np.where(pos, CLASS_PINF, np.where(neg, CLASS_NINF, CLASS_FINITE)))
    val = np.where(np.isfinite(P), P, 0.0).sum(axis=0)
    return cls, val


def problem_gram(ref, pats, nlevels, chunks, model, level, zidx):
    """The Gram fm_solve forms for one problem of one month: the sum over the month's ``chunks``,
    the patterns that contain ``model`` and the levels >= ``level``, restricted to the z indices
    ``zidx`` (0 = intercept, 1 + c = panel column c).  Returns (G [nz, nz] longdouble, n, means
    G0i / n, centered G_ij - G0i G0j / n) over zidx[1:]."""
    nz = len(zidx)
    G = np.zeros((nz, nz), dtype=np.longdouble)
    for q, P in enumerate(pats):
        if not (P >> model) & 1:
            continue
        for lv in range(level, nlevels):
            img = ref.gram[chunks, q * nlevels + lv].astype(np.longdouble).sum(axis=0)
            for a in range(nz):
                for b in range(nz):
                    G[a, b] += img[packed_index(zidx[a], zidx[b], ref.zw)]
    n = G[0, 0]
    if n == 0:
        return G, 0, None, None
    mean = G[0, 1:] / n
    cen = G[1:, 1:] - np.outer(G[0, 1:], G[0, 1:]) / n
    return G, int(n), mean, cen
