"""Train the x-vector backend the chain reads: the transform (``mean1``, ``lda``, ``mean2`` of vbhmm.py:125-129) and the Kaldi
PLDA (``ivector-compute-plda``), from labelled x-vectors.

    python -m vbx_amd.backend --xvec-ark-file X.ark --utt2spk FILE --lda-dim 128 --out-transform transform.npz --out-plda plda

The recipe, all in float64, speakers numbered in order of first appearance, n_k rows for speaker k:

    mean1 = mean x;  y = l2norm(x - mean1)
    St = sum (y - ybar)(y - ybar)^T,  Sb = sum_k n_k (m_k - ybar)(m_k - ybar)^T,  Sw = St - Sb
    lda = the lda_dim largest eigenvectors of eigh(Sb, Sw), largest first, each column's entry of largest magnitude positive
    mean2 = lda^T ybar;  u = l2norm(lda^T y - mean2)
    Kaldi's PLDA estimation on u, one weight per speaker, ``plda_iters`` EM iterations from W = B = I

What is O(N) runs on the device (vbx_backend.hpp): two statistics passes over the resident rows and the second moments of the
class means (Sb, the between-class part of the PLDA's offset scatter, and the scatters G_n of the means of the speakers with n
rows).  The EM iterations only need those: with A_n = (B^-1 + n W^-1)^-1 n W^-1 the sums over the speakers with n rows are
A_n G_n A_n^T and (I - A_n) G_n (I - A_n)^T.  ``estimate_lda`` and ``estimate_plda`` are that D x D host algebra.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from .kaldi_formats import write_plda


def class_index(speakers):
    """-> (class of every row, int32; the speakers in order of first appearance)."""
    ids, names = {}, []
    cls = np.empty(len(speakers), dtype=np.int32)
    for t, s in enumerate(speakers):
        k = ids.get(s)
        if k is None:
            k = ids[s] = len(names)
            names.append(s)
        cls[t] = k
    return cls, names


def sign_convention(v):
    """Every column flipped so that its entry of largest magnitude is positive (the eigensolver leaves the sign open)."""
    v = np.array(v, dtype=np.float64)
    top = np.abs(v).argmax(axis=0)
    flip = v[top, np.arange(v.shape[1])] < 0
    v[:, flip] = -v[:, flip]
    return v


def estimate_lda(ybar, St, Sb, lda_dim):
    """-> (lda [D][lda_dim], mean2 [lda_dim]) from the mean, the total and the between-class scatter of y."""
    from scipy.linalg import eigh
    ybar, St, Sb = (np.asarray(a, dtype=np.float64) for a in (ybar, St, Sb))
    D = ybar.shape[0]
    if not 1 <= lda_dim <= D:
        raise ValueError(f'lda_dim={lda_dim} outside [1, {D}]')
    _w, v = eigh(Sb, St - Sb)                                     # ascending
    lda = sign_convention(v[:, ::-1][:, :lda_dim])
    return lda, lda.T.dot(ybar)


def count_groups(counts):
    """The classes sorted by their number of rows (stable): -> (order [K], distinct counts n [G], offsets [G + 1] into order)."""
    counts = np.asarray(counts, dtype=np.int64)
    order = np.argsort(counts, kind='stable')
    n, first = np.unique(counts[order], return_index=True)
    return order, n, np.concatenate([first, [len(counts)]]).astype(np.int64)


def estimate_plda(n, classes, G, offset_scatter, N, mean, iters=10):
    """Kaldi's PLDA estimation (plda.cc, one weight per class) from grouped statistics.

    n [g]: the distinct class sizes; classes [g]: how many classes have that size; G [g][d][d]: the scatter of their means about
    ``mean`` = (sum of the class means) / K; offset_scatter [d][d] = sum_t u_t u_t^T - sum_k n_k mu_k mu_k^T; N rows in all.
    -> dict(mean, transform, psi, W, B): the model as Kaldi writes it, and the two covariances it diagonalises."""
    n = np.asarray(n, dtype=np.int64)
    classes = np.asarray(classes, dtype=np.int64)
    G = np.asarray(G, dtype=np.float64)
    offset_scatter = np.asarray(offset_scatter, dtype=np.float64)
    d = offset_scatter.shape[0]
    K = int(classes.sum())
    if N - K < 1:
        raise ValueError(f'{N} rows of {K} speakers: the within-speaker covariance needs a speaker with two rows')
    W, B, eye = np.eye(d), np.eye(d), np.eye(d)
    for _ in range(iters):
        Winv, Binv = np.linalg.inv(W), np.linalg.inv(B)
        Wstats, Bstats = offset_scatter.copy(), np.zeros((d, d))
        for ng, cg, Gg in zip(n.tolist(), classes.tolist(), G):
            mixed = np.linalg.inv(Binv + ng * Winv)
            A = mixed.dot(ng * Winv)
            Bstats += cg * mixed + A.dot(Gg).dot(A.T)
            Wstats += cg * ng * mixed + ng * (eye - A).dot(Gg).dot((eye - A).T)
        W, B = Wstats / N, Bstats / K                            # (Wcount = N - K + K, Bcount = K)
    T1 = np.linalg.inv(np.linalg.cholesky(W))
    s, U = np.linalg.eigh(T1.dot(B).dot(T1.T))
    s = np.maximum(s, 0.0)
    order = np.argsort(-s, kind='stable')
    return dict(mean=np.array(mean, dtype=np.float64), transform=U[:, order].T.dot(T1), psi=s[order], W=W, B=B)


class Backend:
    """What ``train_backend`` returns: mean1, lda, mean2 (the transform), plda_mean, plda_transform, plda_psi (the Kaldi PLDA),
    and ``stats``, the intermediate statistics."""

    def __init__(self, mean1, lda, mean2, plda_mean, plda_transform, plda_psi, stats):
        self.mean1, self.lda, self.mean2 = mean1, lda, mean2
        self.plda_mean, self.plda_transform, self.plda_psi = plda_mean, plda_transform, plda_psi
        self.stats = stats

    def arrays(self):
        return self.mean1, self.lda, self.mean2, self.plda_mean, self.plda_transform, self.plda_psi

    def save(self, transform_path, plda_path):
        """The transform as ``.npz`` (or ``.h5`` where h5py is installed) and the PLDA in Kaldi's binary format: what
        ``read_xvec_transform`` and ``read_plda`` read."""
        path = str(transform_path)
        if path.endswith('.npz'):
            with open(path, 'wb') as fd:
                np.savez(fd, mean1=self.mean1, mean2=self.mean2, lda=self.lda)
        elif path.endswith('.h5'):
            try:
                import h5py
            except ImportError:
                raise ValueError(f'{path}: writing HDF5 needs h5py, which is not installed; name the transform *.npz '
                                 f'(read_xvec_transform reads it)') from None
            with h5py.File(path, 'w') as f:
                for name in ('mean1', 'mean2', 'lda'):
                    f.create_dataset(name, data=getattr(self, name))
        else:
            raise ValueError(f'{path}: the transform is written as .npz (or .h5 with h5py)')
        write_plda(plda_path, self.plda_mean, self.plda_transform, self.plda_psi)


def check_training_set(N, Din, K, lda_dim):
    if K < 2:
        raise ValueError(f'{K} speaker(s): the backend needs at least two')
    if N - K < 1:
        raise ValueError(f'{N} x-vectors of {K} speakers: every speaker has one x-vector, there is no within-speaker covariance')
    if not 1 <= lda_dim <= min(Din, K - 1):
        raise ValueError(f'lda_dim={lda_dim} outside [1, min(Din={Din}, K - 1={K - 1})]: the between-speaker scatter has rank '
                         f'K - 1 at most')


def train_backend(x, speakers, lda_dim, plda_iters=10, device=None):
    """The backend of the x-vectors ``x`` [N][Din] (float32 as an archive holds them, or float64) whose rows belong to
    ``speakers`` [N] (any hashable labels).  -> ``Backend``.  The passes over the rows run on the device."""
    from . import _capi
    x = np.asarray(x)
    if x.ndim != 2 or len(speakers) != x.shape[0]:
        raise ValueError(f'x {x.shape} and {len(speakers)} speaker labels do not match')
    cls, names = class_index(speakers)
    N, Din, K = x.shape[0], x.shape[1], len(names)
    check_training_set(N, Din, K, lda_dim)
    counts = np.bincount(cls, minlength=K).astype(np.int64)
    ctx = _capi.default_context(device)
    t0 = time.perf_counter()
    be = _capi.BackendStats(ctx, x, cls, K)
    try:
        t1 = time.perf_counter()
        mean1, ysum, ymom = be.stage1()
        ybar = ysum.sum(axis=0) / N
        ymean = ysum / counts[:, None]
        St = ymom - N * np.outer(ybar, ybar)
        Sb = _capi.backend_second_moments(ctx, np.sqrt(counts)[:, None] * (ymean - ybar), [0, K])[0]
        lda, mean2 = estimate_lda(ybar, St, Sb, lda_dim)
        t2 = time.perf_counter()
        usum, umom = be.stage2(lda, mean2)
        kernel_ms = list(be.kernel_ms)
    finally:
        be.close()
    mu = usum / counts[:, None]
    total = mu.sum(axis=0)
    mean = total / K
    between = _capi.backend_second_moments(ctx, np.sqrt(counts)[:, None] * mu, [0, K])[0]
    offset_scatter = umom - between
    order, n, off = count_groups(counts)
    G = _capi.backend_second_moments(ctx, mu[order] - mean, off)
    t3 = time.perf_counter()
    plda = estimate_plda(n, np.diff(off), G, offset_scatter, N, mean, plda_iters)
    t4 = time.perf_counter()
    stats = dict(N=N, K=K, counts=counts, speakers=names, ybar=ybar, y_class_sums=ysum, y_moment=ymom, St=St, Sb=Sb,
                 u_class_sums=usum, u_moment=umom, offset_scatter=offset_scatter, count_values=n, count_classes=np.diff(off),
                 G=G, W=plda['W'], B=plda['B'],
                 seconds=dict(upload=t1 - t0, stage1_and_lda=t2 - t1, stage2_and_scatters=t3 - t2, plda_em=t4 - t3),
                 kernel_ms=dict(stage1=kernel_ms[0], stage2=kernel_ms[1]))
    return Backend(mean1, lda, mean2, plda['mean'], plda['transform'], plda['psi'], stats)


# ---- files -----------------------------------------------------------------------------------------------------------------
def read_utt2spk(path):
    """Kaldi ``utt2spk``: one ``<utterance> <speaker>`` per line -> {utterance: speaker}, in file order."""
    out = {}
    with open(path) as fd:
        for no, line in enumerate(fd, 1):
            f = line.split()
            if not f:
                continue
            if len(f) != 2:
                raise ValueError(f'{path}:{no}: expected "<utterance> <speaker>", found {line.rstrip()!r}')
            if f[0] in out:
                raise ValueError(f'{path}:{no}: utterance {f[0]} appears twice')
            out[f[0]] = f[1]
    return out


def read_xvectors(ark_path):
    """-> (keys, x [N][Din]) of a Kaldi vector archive, in file order."""
    from . import _capi
    from .kaldi_formats import read_vec_flt_ark
    with open(ark_path, 'rb') as fd:
        raw = fd.read()
    idx = _capi.ark_index(raw)
    if idx is None:
        keys, vecs = zip(*read_vec_flt_ark(ark_path))
        if len({len(v) for v in vecs}) != 1:
            raise ValueError(f'{ark_path}: the x-vectors differ in dimension')
        return list(keys), np.array(vecs)
    key_off, key_len, data_off, dim, esize = idx
    if len(dim) == 0:
        raise ValueError(f'{ark_path}: no x-vectors')
    if np.any(dim != dim[0]) or np.any(esize != esize[0]):
        raise ValueError(f'{ark_path}: the x-vectors differ in dimension or type')
    keys = [raw[o:o + n].decode() for o, n in zip(key_off.tolist(), key_len.tolist())]
    d, e = int(dim[0]), int(esize[0])
    return keys, _capi.gather_rows(np.frombuffer(raw, dtype=np.uint8), data_off, d * e, '<f4' if e == 4 else '<f8')


def load_training_set(ark_path, utt2spk_path, min_utts=1):
    """-> (x, speaker of every row): the archive's x-vectors with their speakers, without the speakers that have fewer than
    ``min_utts`` of them."""
    keys, x = read_xvectors(ark_path)
    u2s = read_utt2spk(utt2spk_path)
    missing = [k for k in keys if k not in u2s]
    if missing:
        raise ValueError(f'{len(missing)} of the {len(keys)} x-vectors of {ark_path} have no speaker in {utt2spk_path}: '
                         + ', '.join(missing[:5]) + (' ...' if len(missing) > 5 else ''))
    speakers = [u2s[k] for k in keys]
    if min_utts > 1:
        cls, names = class_index(speakers)
        keep = np.bincount(cls, minlength=len(names))[cls] >= min_utts
        x, speakers = x[keep], [s for s, k in zip(speakers, keep.tolist()) if k]
    return x, speakers


def build_parser():
    p = argparse.ArgumentParser(prog='python -m vbx_amd.backend', description=__doc__.split('\n\n')[0])
    p.add_argument('--xvec-ark-file', required=True, help='Kaldi archive of x-vectors')
    p.add_argument('--utt2spk', required=True, help='Kaldi utt2spk: the speaker of every x-vector of the archive')
    p.add_argument('--lda-dim', required=True, type=int, help='columns of the LDA transform = dimensions of the PLDA')
    p.add_argument('--out-transform', required=True, help='mean1, lda, mean2: *.npz (or *.h5 where h5py is installed)')
    p.add_argument('--out-plda', required=True, help='the PLDA model in Kaldi\'s binary format')
    p.add_argument('--min-utts', type=int, default=1, help='drop speakers with fewer x-vectors than this')
    p.add_argument('--plda-iters', type=int, default=10, help='EM iterations of the PLDA estimation')
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--timing', action='store_true', help='print where the time went')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        if str(args.out_transform).endswith('.h5'):
            try:
                import h5py                                      # noqa: F401
            except ImportError:
                raise ValueError(f'{args.out_transform}: writing HDF5 needs h5py, which is not installed; name the transform '
                                 f'*.npz (read_xvec_transform reads it)') from None
        elif not str(args.out_transform).endswith('.npz'):
            raise ValueError(f'{args.out_transform}: the transform is written as .npz (or .h5 with h5py)')
        t0 = time.perf_counter()
        x, speakers = load_training_set(args.xvec_ark_file, args.utt2spk, args.min_utts)
        if len(speakers) == 0:
            raise ValueError(f'no speaker has {args.min_utts} x-vectors')
        cls, names = class_index(speakers)
        check_training_set(x.shape[0], x.shape[1], len(names), args.lda_dim)
        t1 = time.perf_counter()
        model = train_backend(x, speakers, args.lda_dim, args.plda_iters, args.device)
        model.save(args.out_transform, args.out_plda)
    except ValueError as exc:
        print(f'backend: {exc}', file=sys.stderr)
        return 2
    st = model.stats
    print(f'{st["N"]} x-vectors of {st["K"]} speakers, {x.shape[1]} -> {args.lda_dim} dimensions: {args.out_transform}, {args.out_plda}')
    if args.timing:
        sec, ms = st['seconds'], st['kernel_ms']
        print(f'read {t1 - t0:.3f} s, upload {sec["upload"]:.3f} s, stage 1 + LDA {sec["stage1_and_lda"]:.3f} s (kernels {ms["stage1"]:.2f} ms), '
              f'stage 2 + scatters {sec["stage2_and_scatters"]:.3f} s (kernels {ms["stage2"]:.2f} ms), PLDA EM {sec["plda_em"]:.3f} s')
    return 0


if __name__ == '__main__':
    sys.exit(main())
