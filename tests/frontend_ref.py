"""Reference and error bounds for the driver's device stages (vbx_frontend.hpp)  --  test helper, not a test.

    xproj = l2_norm( l2_norm(x - mean1) lda - mean2 )           vbhmm.py:125-129
    fea   = (xproj - plda_mu) plda_tr^T [:, :fea_dim]           vbhmm.py:153

``project_ref`` evaluates both in ``np.longdouble`` (64-bit significand on x86: 2^11 times finer than float64), or in
float64 for the self-check of tests/test_frontend_ref_host.py.  The bounds are first-order forward-error bounds of a
float64 evaluation in ANY summation order, evaluated elementwise on the long-double intermediates; u = 2^-53:

  centre, normalise     v = fl(x - mean1) carries u; the sum of Din squares Din u on ss, half of it on the norm; the
                        square root and the division u each: relative error of y1 at most eA = (Din + 4) u
  first product         a sum of Kp terms, then - mean2:  bz = (eA + (Kp + 1) u) (|y1| |lda|) + 2 u |mean2|
  second normalisation  p = z / |z|:  dp = (dz - p <p, dz>) / |z|, so |dp| <= (bz + |p| ||bz||_2) / |z|, and the
                        normalisation's own rounding (Dl + 4) u |p|
  tolerance             2 bp (second-order terms, and the reference's own error of 2^-64 per operation)

  second product        x P - (mu P) with mu P summed on the host: 2 (Kp2 + Dl + 2) u (|xproj| |P| + |mu| |P|), against the
                        long-double product of the xproj the device itself holds -- the error of xproj is not counted twice

The shapes and the inputs of the GPU tests live here as well, so that the host self-check runs on the very same cases.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble

# (n, Din, Dl, fea_dim, dtype of x)                        what it exercises
SHAPES = [
    (1, 5, 7, 3, np.float64),                              # smallest case, all paddings
    (15, 4, 16, 16, np.float32),                           # no padding at all
    (17, 63, 30, 17, np.float64),                          # odd sizes everywhere
    (64, 64, 128, 128, np.float32),                        # exact tile sizes
    (65, 65, 129, 128, np.float64),                        # Np = 144: second pass of the column loop; Kp2 = 132 != Dl
    (130, 257, 200, 130, np.float32),                      # Np = 208, Np2 = 144; three workgroups, last wave partly empty
    (63, 100, 260, 1, np.float64),                         # Np = 272: third pass; a single output column
    (257, 256, 128, 128, np.float32),                      # the driver's own shape
]


def shape_id(shape):
    n, din, dl, fea_dim, dtype = shape
    return f'n{n}-Din{din}-Dl{dl}-fea{fea_dim}-{np.dtype(dtype).name}'


def round_up(a, m):
    return (a + m - 1) // m * m


def make_case(shape, seed=None):
    """Seeded inputs of one shape: rows of x scaled by 10^U(-3, 3) (the normalisation must remove the scale), means of
    order 0.1, standard normal transforms; for float32 input mean1 is rounded to float32 as well."""
    n, din, dl, fea_dim, dtype = shape
    rng = np.random.default_rng(1000 + SHAPES.index(shape) if seed is None else seed)
    x = (rng.standard_normal((n, din)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))).astype(dtype)
    mean1 = 0.1 * rng.standard_normal(din)
    if dtype == np.float32:
        mean1 = mean1.astype(np.float32).astype(np.float64)
    return dict(x=x, mean1=mean1, lda=rng.standard_normal((din, dl)), mean2=0.1 * rng.standard_normal(dl),
                plda_mu=0.1 * rng.standard_normal(dl), plda_tr=rng.standard_normal((dl, dl)), fea_dim=fea_dim)


def _l2_norm(a):
    return a / np.sqrt((a * a).sum(axis=1))[:, np.newaxis]


def project_ref(x, mean1, lda, mean2, plda_mu, plda_tr, fea_dim, dtype=LD):
    """-> (y1, z, xproj, fea), every operation in ``dtype``."""
    x, mean1, lda, mean2, plda_mu, plda_tr = (np.asarray(a).astype(dtype) for a in (x, mean1, lda, mean2, plda_mu, plda_tr))
    y1 = _l2_norm(x - mean1)
    z = y1.dot(lda) - mean2
    xproj = _l2_norm(z)
    fea = (xproj - plda_mu).dot(plda_tr.T)[:, :fea_dim]
    return y1, z, xproj, fea


def xproj_bound(y1, z, xproj, lda, mean2):
    """Elementwise tolerance [n][Dl] of a float64 xproj, from the long-double intermediates of ``project_ref``."""
    din, dl = lda.shape
    e_a = (din + 4) * U
    bz = (e_a + (round_up(din, 4) + 1) * U) * np.abs(y1).dot(np.abs(lda).astype(LD)) + 2 * U * np.abs(mean2).astype(LD)
    p = np.abs(xproj)
    norm_z = np.sqrt((z * z).sum(axis=1))[:, np.newaxis]
    norm_bz = np.sqrt((bz * bz).sum(axis=1))[:, np.newaxis]
    bp = (bz + p * norm_bz) / norm_z + (dl + 4) * U * p
    return 2 * bp


def fea_bound(xproj_dev, plda_mu, plda_tr, fea_dim):
    """-> (fea, tolerance), both [n][fea_dim]: the long-double product (xproj_dev - plda_mu) P and the elementwise
    tolerance of its float64 evaluation as x P - (mu P), P = plda_tr^T[:, :fea_dim]."""
    dl = len(plda_mu)
    P = np.asarray(plda_tr).astype(LD).T[:, :fea_dim]
    xp, mu = np.asarray(xproj_dev).astype(LD), np.asarray(plda_mu).astype(LD)
    fea = (xp - mu).dot(P)
    tol = 2 * (round_up(dl, 4) + dl + 2) * U * (np.abs(xp).dot(np.abs(P)) + np.abs(mu).dot(np.abs(P)))
    return fea, tol


def ratio(got, want, tol):
    """max |got - want| / tol (long double)."""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - want) / tol))


# ---- the device arg-sort -----------------------------------------------------------------------------------------
def top2_ref(gamma, storage):
    """(first, second) speaker as the device reports them: a stable argsort of -gamma taken in the batch's storage type
    (ties go to the lower index); second is None for one speaker."""
    g = np.asarray(gamma).astype(storage)
    order = np.argsort(-g, axis=1, kind='stable')
    return order[:, 0], (order[:, 1] if g.shape[1] > 1 else None)


def top2_patterns(T, S, seed=0):
    """[T][S] float64 rows that cycle through the tie patterns of the arg-sort; every value is a multiple of 2^-k or
    1/3-based, positive, and no row is normalised (the setter takes responsibilities as they come)."""
    rng = np.random.default_rng(seed)
    mid = S // 2
    rows = []
    for t in range(T):
        kind = t % 12
        r = np.full(S, 0.125)
        a, b, c = (int(v) for v in rng.permutation(S)[:3]) if S >= 3 else (0, S - 1, 0)
        if kind == 0:                                       # unique maximum at index 0
            r[0] = 0.5
        elif kind == 1:                                     # ... at S - 1
            r[S - 1] = 0.5
        elif kind == 2:                                     # ... in the middle
            r[mid] = 0.5
        elif kind == 3:                                     # two-way tie for first place
            r[[a, b]] = 0.5
        elif kind == 4:                                     # three-way tie for first place
            r[[a, b, c]] = 0.5
        elif kind == 5:                                     # all equal
            pass
        elif kind == 6:                                     # a tie for second place only
            r[a] = 0.5
            if S >= 3:
                r[[b, c]] = 0.25
        elif kind == 7:                                     # strictly ascending
            r = (1.0 + np.arange(S)) / 1024.0
        elif kind == 8:                                     # strictly descending
            r = (S - np.arange(S)) / 1024.0
        elif kind == 9:                                     # ordered in float64, tied in float32
            r = np.full(S, 0.25)
            r[0] = 1.0 / 3.0
            if S > 1:
                r[1] = 1.0 / 3.0 + 1e-12
        elif kind == 10:                                    # the same pair the other way round, away from index 0
            r = np.full(S, 0.25)
            r[S - 1] = 1.0 / 3.0
            r[mid] = 1.0 / 3.0 + 1e-12 if mid != S - 1 else r[mid]
        else:                                               # the maximum last, the runner-up tied before it
            r[S - 1] = 0.5
            if S >= 3:
                r[[0, mid]] = 0.25
        rows.append(r)
    return np.array(rows)


# ---- initial responsibilities ------------------------------------------------------------------------------------
def qinit_ref(labels, S, smoothing):
    """softmax(smoothing * onehot(labels)) as its two values (vbhmm.py:150-152): -> (gamma [T][S] float64, hi, lo)."""
    z = np.exp(-float(smoothing))
    hi = 1.0 / (1.0 + (S - 1) * z)
    lo = z * hi
    onehot = np.arange(S)[np.newaxis, :] == np.asarray(labels)[:, np.newaxis]
    return np.where(onehot, hi, lo), hi, lo
