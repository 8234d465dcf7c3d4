"""numpy restatement of the backend recipe of vbx_amd/backend.py  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The statistics are plain sums in a caller-chosen dtype (np.longdouble for the kernel tests), and the PLDA estimation is Kaldi's
loop over the classes one by one (plda.cc: PldaEstimator), NOT the form grouped by class size that the product uses: the two
formulations check each other.  Also here: the synthetic two-covariance training set of the end-to-end tests and the chain
vbhmm.py:125-162 on the host through oracle/ alone.
"""
import numpy as np


def l2_norm(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def first_appearance(speakers):
    ids = {}
    return np.array([ids.setdefault(s, len(ids)) for s in speakers], dtype=np.int32), list(ids)


# ---- statistics ------------------------------------------------------------------------------------------------------------
def class_sums(x, cls, K, dtype=np.float64):
    """-> (sums [K][D], sum of |terms| [K][D], counts [K])"""
    x = np.asarray(x).astype(dtype)
    sums, mags = np.zeros((K, x.shape[1]), dtype=dtype), np.zeros((K, x.shape[1]), dtype=dtype)
    np.add.at(sums, cls, x)
    np.add.at(mags, cls, np.abs(x))
    return sums, mags, np.bincount(cls, minlength=K)


def second_moments(rows, offsets, dtype=np.float64):
    """-> (out [G][D][D], sum of |terms| [G][D][D], the latter in float64: it only scales a bound).  The blocks above the diagonal are computed and mirrored (longdouble products
    do not run in BLAS; a product does not depend on the order of its factors)."""
    rows = np.asarray(rows).astype(dtype)
    G, D = len(offsets) - 1, rows.shape[1]
    out, mags = np.zeros((G, D, D), dtype=dtype), np.zeros((G, D, D))
    for g in range(G):
        r = rows[offsets[g]:offsets[g + 1]]
        a = np.abs(r).astype(np.float64)
        for i in range(0, D, 64):
            out[g, i:i + 64, i:] = r[:, i:i + 64].T.dot(r[:, i:])
            mags[g, i:i + 64, i:] = a[:, i:i + 64].T.dot(a[:, i:])
            out[g, i:, i:i + 64] = out[g, i:i + 64, i:].T
            mags[g, i:, i:i + 64] = mags[g, i:i + 64, i:].T
    return out, mags


# ---- LDA -------------------------------------------------------------------------------------------------------------------
def sign_convention(v):
    v = v.copy()
    for c in range(v.shape[1]):
        if v[np.argmax(np.abs(v[:, c])), c] < 0:
            v[:, c] = -v[:, c]
    return v


def lda_scatters(y, cls, K):
    ybar = y.mean(axis=0)
    St = (y - ybar).T.dot(y - ybar)
    Sb = np.zeros_like(St)
    for k in range(K):
        rows = y[cls == k]
        m = rows.mean(axis=0) - ybar
        Sb += len(rows) * np.outer(m, m)
    return ybar, St, Sb


def lda(ybar, St, Sb, lda_dim):
    from scipy.linalg import eigh
    _w, v = eigh(Sb, St - Sb)
    v = sign_convention(v[:, ::-1][:, :lda_dim])
    return v, v.T.dot(ybar)


# ---- Kaldi PLDA ------------------------------------------------------------------------------------------------------------
def plda_stats(u, cls, K):
    """-> (class means [K][d], counts [K], offset_scatter [d][d])"""
    counts = np.bincount(cls, minlength=K)
    mu = np.zeros((K, u.shape[1]))
    np.add.at(mu, cls, u)
    mu /= counts[:, None]
    scatter = u.T.dot(u)
    for k in range(K):
        scatter -= counts[k] * np.outer(mu[k], mu[k])
    return mu, counts, scatter


def plda_class_loop(mu, counts, offset_scatter, iters=10, visit=None):
    """Kaldi's EM, the classes visited one by one in the order ``visit`` (default: as numbered).  -> (mean, W, B)"""
    K, d = mu.shape
    N = int(np.sum(counts))
    visit = range(K) if visit is None else visit
    mean = mu.sum(axis=0) / K
    W, B = np.eye(d), np.eye(d)
    for _ in range(iters):
        Winv, Binv = np.linalg.inv(W), np.linalg.inv(B)
        Wstats, Wcount, Bstats, Bcount = offset_scatter.copy(), N - K, np.zeros((d, d)), 0
        for k in visit:
            n = int(counts[k])
            mixed = np.linalg.inv(Binv + n * Winv)
            m = mu[k] - mean
            w = mixed.dot(n * Winv.dot(m))
            Bstats += mixed + np.outer(w, w)
            Bcount += 1
            Wstats += n * mixed + n * np.outer(m - w, m - w)
            Wcount += 1
        W, B = Wstats / Wcount, Bstats / Bcount
    return mean, W, B


def plda_output(W, B):
    """-> (transform, psi) as Kaldi writes them"""
    T1 = np.linalg.inv(np.linalg.cholesky(W))
    s, U = np.linalg.eigh(T1.dot(B).dot(T1.T))
    s = np.maximum(s, 0.0)
    order = np.argsort(-s, kind='stable')
    return U[:, order].T.dot(T1), s[order]


def train(x, speakers, lda_dim, iters=10):
    """The whole recipe on the host, float64.  -> dict(mean1, lda, mean2, mean, W, B, transform, psi)"""
    cls, names = first_appearance(speakers)
    K = len(names)
    x = np.asarray(x, dtype=np.float64)
    mean1 = x.mean(axis=0)
    y = l2_norm(x - mean1)
    ybar, St, Sb = lda_scatters(y, cls, K)
    v, mean2 = lda(ybar, St, Sb, lda_dim)
    u = l2_norm(y.dot(v) - mean2)
    mu, counts, scatter = plda_stats(u, cls, K)
    mean, W, B = plda_class_loop(mu, counts, scatter, iters)
    transform, psi = plda_output(W, B)
    return dict(mean1=mean1, lda=v, mean2=mean2, mean=mean, W=W, B=B, transform=transform, psi=psi)


def rel_dist(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


# ---- the synthetic two-covariance world of the end-to-end tests ----------------------------------------------------------------
DIN, LDA_DIM, K_TRAIN = 24, 8, 60
# The seed of the end-to-end tests.  Chosen on the CPU: with the backend trained by train() below, host_chain() makes no error on
# the held-out recording for the seeds 1, 2, 4, 5 and 7 of 1 ... 7 (for 3 and 6 the AHC stage merges two of the three speakers).
E2E_SEED = 1


class World:
    """Speaker means with standard deviation 3 ... 1 on 8 directions of a random orthonormal basis of 24; the other 16 directions
    carry within-speaker noise only; noise 0.6 everywhere, plus a constant offset.  float32 rows."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.basis = np.linalg.qr(self.rng.standard_normal((DIN, DIN)))[0]
        self.sd = np.concatenate([np.linspace(3.0, 1.0, LDA_DIM), np.zeros(DIN - LDA_DIM)])
        self.offset = self.rng.standard_normal(DIN) * 2.0

    def speaker(self):
        return (self.rng.standard_normal(DIN) * self.sd).dot(self.basis.T)

    def rows(self, mean, n):
        return (mean + 0.6 * self.rng.standard_normal((n, DIN)) + self.offset).astype(np.float32)

    def training_set(self):
        """K = 60 speakers with 1 ... 12 rows each, interleaved.  -> (x [N][24] f32, speaker names [N])"""
        xs, spk = [], []
        for k in range(K_TRAIN):
            n = 1 + k % 12
            xs.append(self.rows(self.speaker(), n))
            spk += [f'spk{k:02d}'] * n
        x, spk = np.concatenate(xs), np.array(spk)
        order = self.rng.permutation(len(x))
        return x[order], spk[order].tolist()

    def recording(self, windows=150, speakers=3, turn=5):
        """Held-out speakers, turns of ``turn`` windows.  -> (x [windows][24] f32, truth [windows])"""
        means = [self.speaker() for _ in range(speakers)]
        truth = np.repeat(self.rng.integers(0, speakers, size=windows // turn), turn)
        truth[:speakers * turn] = np.repeat(np.arange(speakers), turn)          # (everybody speaks)
        return np.concatenate([self.rows(means[s], 1) for s in truth]), truth


def same_partition(a, b):
    """Do the label sequences agree up to a renaming of the speakers?"""
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


def host_chain(x, model, lda_dim, Fa=0.3, Fb=17.0, loopP=0.9, threshold=0.0, init_smoothing=5.0):
    """vbhmm.py:107-162 (AHC+VB) on the host for one recording, through oracle/ and SciPy alone.  -> labels"""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.linalg import eigh
    from scipy.spatial.distance import squareform
    from scipy.special import softmax
    from oracle import ahc_oracle, vbx_oracle
    tr, psi = model['transform'], model['psi']
    W = np.linalg.inv(tr.T.dot(tr))
    B = np.linalg.inv((tr.T / psi).dot(tr))
    acvar, wccn = eigh(B, W)
    plda_psi, plda_tr = acvar[::-1], wccn.T[::-1]
    x = l2_norm(l2_norm(np.asarray(x, dtype=np.float64) - model['mean1']).dot(model['lda']) - model['mean2'])
    scr = ahc_oracle.cos_similarity(x)
    thr, _ = ahc_oracle.twoGMMcalib_lin(scr.ravel())
    lin = linkage(squareform(-scr, checks=False), method='average')
    adjust = abs(lin[:, 2].min())
    lin[:, 2] += adjust
    labels = fcluster(lin, -(thr + threshold) + adjust, criterion='distance') - 1
    qinit = np.zeros((len(labels), labels.max() + 1))
    qinit[range(len(labels)), labels] = 1.0
    qinit = softmax(qinit * init_smoothing, axis=1)
    fea = (x - model['mean']).dot(plda_tr.T)[:, :lda_dim]
    q = vbx_oracle.VBx(fea, plda_psi[:lda_dim], pi=qinit.shape[1], gamma=qinit, maxIters=40, epsilon=1e-6, loopProb=loopP, Fa=Fa,
                       Fb=Fb)[0]
    return np.argsort(-q, axis=1)[:, 0]
