"""The statistics kernels of backend training on the device (-m gpu): ``vbx_backend_class_sums`` and
``vbx_backend_second_moments`` against tests/backend_ref.py evaluated in np.longdouble, at every tile, k-step and chunk edge.

Tolerance per entry: C_TOL * n * 2^-53 * sum |terms|, n the number of terms of the entry (the rows of its class or segment).

Where C_TOL = 2 comes from.  An entry is a sum of n terms.  For a class sum a term is a row's element (a float32 widens to
float64 exactly) and the n terms meet in n - 1 float64 additions, in whatever order the chunks impose; a term passes through at
most n - 1 of them, so |error| <= gamma_(n-1) * sum |x_t| with gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2: the bound holds for every summation order).  For a second moment a term is a
product a_t b_t: one rounding where the matrix instruction rounds the product (none where it fuses it into the addition), then
again at most n - 1 additions -- the additions of zero for rows and columns of padding are exact -- so at most n roundings per
term and |error| <= gamma_n * sum |a_t b_t| (section 3.1, again for every order).  With n <= 2574 here gamma_n < 1.0000003 n u,
so n u sum |terms| holds to first order; the factor 2 covers the second-order part of gamma_n, the rounding of the longdouble
reference (2^-64 per operation: a 2000th of u) and of its conversion for the comparison.  It is derived, not measured; the
largest measured ratio error / bound is printed by every test (one MI355X: DESIGN section 25).
"""
import ctypes as C

import numpy as np
import pytest

import backend_ref as ref

pytestmark = pytest.mark.gpu
C_TOL = 2.0
U = 2.0 ** -53
DIMS = [1, 15, 16, 17, 63, 64, 65, 256]
LENGTHS = [1, 3, 4, 5, 511, 512, 513, 1025]                   # the MFMA's k-step of 4 and the chunk of 512
CLASSES = [1, 2, 37]
SEED = 2510


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


def rows_for(rng, n, D):
    """Rows with a common offset, so that sums do not hover about zero and magnitudes differ between columns."""
    return rng.standard_normal((n, D)) * np.linspace(0.5, 2.0, D) + 0.25


def check(got, want, mags, n, tag):
    """-> the largest error / bound; asserts every entry within C_TOL n u sum |terms| (n broadcasts against the entries)."""
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    bound = C_TOL * np.asarray(n, dtype=np.float64) * U * mags.astype(np.float64)
    ratio = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))
    assert np.all(err <= bound), (tag, ratio, np.argwhere(err > bound)[:3].tolist())
    return ratio


@pytest.mark.parametrize('D', DIMS)
def test_class_sums_equal_the_longdouble_sums_for_interleaved_classes_of_every_length(D, ctx):
    from vbx_amd import _capi
    rng = np.random.default_rng(SEED + D)
    worst = 0.0
    for K in CLASSES:
        lengths = [LENGTHS[(k + K) % len(LENGTHS)] for k in range(K)]
        if K == 1:
            lengths = [1025]
        cls = rng.permutation(np.repeat(np.arange(K), lengths)).astype(np.int32)       # interleaved in archive order
        x64 = rows_for(rng, len(cls), D)
        for x in (x64, x64.astype(np.float32)):
            sums, counts = _capi.backend_class_sums(ctx, x, cls, K)
            again, _ = _capi.backend_class_sums(ctx, x, cls, K)
            want, mags, n = ref.class_sums(x, cls, K, np.longdouble)
            assert sums.shape == (K, D) and np.array_equal(counts, n) and np.array_equal(counts, lengths)
            assert np.array_equal(sums, again), 'two runs differ'
            worst = max(worst, check(sums, want, mags, n[:, None], (D, K, x.dtype)))
    print(f'class sums, D = {D}: largest error / bound = {worst:.3f}')


@pytest.mark.parametrize('D', DIMS)
def test_second_moments_equal_the_longdouble_products_for_segments_of_every_length(D, ctx):
    """The eight lengths and a segment without rows, then all rows as one segment (six chunks added in order)."""
    from vbx_amd import _capi
    rng = np.random.default_rng(SEED + 100 + D)
    lengths = LENGTHS[:4] + [0] + LENGTHS[4:]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = rows_for(rng, int(off[-1]), D)
    want_seg, mags_seg = ref.second_moments(rows, off, np.longdouble)
    part = np.array([5, 5 + 513], dtype=np.int64)                # a segment that starts inside a chunk of the others
    cases = [(off, want_seg, mags_seg),
             (np.array([0, off[-1]], dtype=np.int64), want_seg.sum(axis=0)[None], mags_seg.sum(axis=0)[None]),
             (part, *ref.second_moments(rows, part, np.longdouble))]
    worst = 0.0
    for offsets, want, mags in cases:
        got = _capi.backend_second_moments(ctx, rows, offsets)
        again = _capi.backend_second_moments(ctx, rows, offsets)
        assert got.shape == (len(offsets) - 1, D, D)
        assert np.array_equal(got, again), 'two runs differ'
        assert np.array_equal(got, got.transpose(0, 2, 1)), 'not symmetric to the last bit'
        if len(offsets) == len(off):
            assert not got[4].any()                              # the segment without rows
        worst = max(worst, check(got, want, mags, np.diff(offsets)[:, None, None], (D, len(offsets))))
    print(f'second moments, D = {D}: largest error / bound = {worst:.3f}')


def test_second_moments_have_the_same_bits_however_many_launches_share_the_partials(ctx, monkeypatch):
    """The partials of a long input are produced a batch of chunks at a time (256 MB of them); a segment that spans batches
    continues from what the earlier launch left.  With the batch cut to 2 chunks (an experiment knob) the 3-chunk, 1-chunk and
    5-chunk segments here start, end and continue at batch edges: same bits as in one batch."""
    from vbx_amd import _capi
    rng = np.random.default_rng(SEED + 7)
    D = 17
    off = np.array([0, 1025, 1025, 1030, 1030 + 2049], dtype=np.int64)
    rows = rows_for(rng, int(off[-1]), D)
    whole = _capi.backend_second_moments(ctx, rows, off)
    monkeypatch.setenv('VBX_AMD_EXPERIMENT', '1')
    for chunks in ('1', '2', '3'):
        monkeypatch.setenv('VBX_AMD_BACKEND_BATCH_CHUNKS', chunks)
        assert np.array_equal(_capi.backend_second_moments(ctx, rows, off), whole), chunks
    want, mags = ref.second_moments(rows, off, np.longdouble)
    print(f'largest error / bound = {check(whole, want, mags, np.diff(off)[:, None, None], "batches"):.3f}')


def test_bad_input_is_refused_with_a_message_before_anything_is_launched(ctx):
    from vbx_amd import _capi
    lib, p = ctx._lib, _capi._ptr
    x = np.ones((4, 3))
    cls = np.array([0, 1, 0, 1], dtype=np.int32)
    out = np.empty((2, 3))

    def refused(rc, pattern):
        with pytest.raises(_capi.VbxError, match=pattern):
            ctx.check(rc, 'call')

    sums = lib.vbx_backend_class_sums
    refused(sums(ctx._h, 4, 3, None, _capi.VBX_F64, 2, p(cls), p(out), None), 'NULL')
    refused(sums(ctx._h, 4, 3, p(x), _capi.VBX_F64, 2, None, p(out), None), 'NULL')
    refused(sums(ctx._h, 4, 3, p(x), _capi.VBX_F64, 2, p(cls), None, None), 'NULL')
    refused(sums(ctx._h, 0, 3, p(x), _capi.VBX_F64, 2, p(cls), p(out), None), 'N=0')
    refused(sums(ctx._h, 4, 0, p(x), _capi.VBX_F64, 2, p(cls), p(out), None), 'D=0')
    refused(sums(ctx._h, 4, 3, p(x), _capi.VBX_F64, 0, p(cls), p(out), None), 'K=0')
    refused(sums(ctx._h, 4, 1025, p(x), _capi.VBX_F64, 2, p(cls), p(out), None), 'D <= 1024')
    refused(sums(ctx._h, 4, 3, p(x), 7, 2, p(cls), p(out), None), 'f32 or f64')
    with pytest.raises(_capi.VbxError, match=r'class 2 of row 1 outside \[0, 2\)'):
        _capi.backend_class_sums(ctx, x, [0, 2, 0, 1], 2)
    with pytest.raises(_capi.VbxError, match=r'class -1 of row 3 outside'):
        _capi.backend_class_sums(ctx, x, [0, 1, 0, -1], 2)
    with pytest.raises(_capi.VbxError, match='class 2 has no row'):
        _capi.backend_class_sums(ctx, x, [0, 1, 3, 1], 4)

    mom = lib.vbx_backend_second_moments
    off = np.array([0, 4], dtype=np.int64)
    big = np.empty((1, 3, 3))
    refused(mom(ctx._h, 4, 3, None, 1, p(off), p(big)), 'NULL')
    refused(mom(ctx._h, 4, 3, p(x), 1, None, p(big)), 'NULL')
    refused(mom(ctx._h, 4, 3, p(x), 1, p(off), None), 'NULL')
    refused(mom(ctx._h, 4, 3, p(x), 0, p(off), p(big)), 'G=0')
    refused(mom(ctx._h, 4, 1025, p(x), 1, p(off), p(big)), 'D <= 1024')
    with pytest.raises(_capi.VbxError, match=r'offsets\[2\] = 1 does not ascend'):
        _capi.backend_second_moments(ctx, x, [0, 3, 1, 4])
    with pytest.raises(_capi.VbxError, match='leave the 4 rows'):
        _capi.backend_second_moments(ctx, x, [0, 5])
    with pytest.raises(_capi.VbxError, match='leave the 4 rows'):
        _capi.backend_second_moments(ctx, x, [-1, 4])

    h = C.c_void_p()
    create = lib.vbx_backend_create
    refused(create(ctx._h, 4, 3, None, _capi.VBX_F64, 2, p(cls), C.byref(h)), 'NULL')
    refused(create(ctx._h, 4, 1025, p(x), _capi.VBX_F64, 2, p(cls), C.byref(h)), 'D <= 1024')
    with pytest.raises(_capi.VbxError, match='class 1 has no row'):
        _capi.BackendStats(ctx, x, [0, 0, 2, 2], 3)
