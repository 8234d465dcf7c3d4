"""The kernels of the x-vector network one by one (vbx_resnet.hpp through the step-level entry points vbx_resnet_conv,
vbx_resnet_stem, vbx_resnet_pool) against the same operation in f64 on the CPU, fed the same f32 inputs.

The bound is derived, not tuned.  Every output of a convolution is an f32 fma chain over K = ks^2 Cin terms in k order,
then + bias, then + res, so

    |y - y64| <= gamma(K + 2) (sum_k |a_k| |w_k| + |bias| + |res|),   gamma(m) = m u / (1 - m u),   u = 2^-24

per element; ReLU is 1-Lipschitz, so it holds after it too.  The bracket is the f64 convolution of |x| with |w|.  An
indexing fault (a wrong tap, row or channel, a dropped K slice) gives errors of order 1: thousands of times this bound.
Outputs are written into a sentinel-filled buffer with a guard band either side (_capi.resnet_conv): a store outside the
payload and an element never written are both seen."""
import ctypes as C

import numpy as np
import pytest

import resnet_shapes as rs
from vbx_amd import _capi, xvector

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def gamma(m):
    return m * U / (1.0 - m * U)


@pytest.fixture(scope='module')
def ctx():
    return _capi.default_context(0)


def conv_ref(x, w, bias, ks, stride, res=None, relu=False):
    """The convolution in f64 as a sum over taps of (shifted slice) @ (that tap's weights): x [n][H][W][Cin], w [ks ks
    Cin][Cout].  Padded taps are skipped, not multiplied by zero, so a non-finite input reaches only the outputs it
    belongs to.  ReLU keeps NaN, as F.relu does."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    n, H, W, Cin = x.shape
    Cout, P = w.shape[1], ks // 2
    Ho, Wo = rs.rn_out(H, stride), rs.rn_out(W, stride)
    y = np.zeros((n, Ho, Wo, Cout))
    for r in range(ks):
        for s in range(ks):
            # outputs ho with 0 <= ho stride - P + r < H
            h0 = max(0, -((r - P) // stride))
            h1 = min(Ho, (H - 1 - r + P) // stride + 1)
            w0 = max(0, -((s - P) // stride))
            w1 = min(Wo, (W - 1 - s + P) // stride + 1)
            if h1 <= h0 or w1 <= w0:
                continue
            xs = x[:, h0 * stride - P + r:(h1 - 1) * stride - P + r + 1:stride, w0 * stride - P + s:(w1 - 1) * stride - P + s + 1:stride]
            y[:, h0:h1, w0:w1] += xs @ w[(r * ks + s) * Cin:(r * ks + s + 1) * Cin]
    y += np.asarray(bias, dtype=np.float64)
    if res is not None:
        y += np.asarray(res, dtype=np.float64).reshape(y.shape)
    return np.where(y < 0, 0.0, y) if relu else y


def conv_bound(x, w, bias, ks, stride, res=None):
    K = ks * ks * x.shape[3]
    return gamma(K + 2) * conv_ref(np.abs(x), np.abs(w), np.abs(bias), ks, stride, None if res is None else np.abs(res))


def make(rng, ks, n, H, W, Cin, Cout, stride, with_res=True):
    x = rng.standard_normal((n, H, W, Cin)).astype(np.float32)
    w = rng.standard_normal((ks * ks * Cin, Cout)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32)
    res = rng.standard_normal((n, rs.rn_out(H, stride), rs.rn_out(W, stride), Cout)).astype(np.float32) if with_res else None
    return x, w, bias, res


def check_conv(ctx, x, w, bias, ks, stride, res, relu, tile, what):
    y, guard, unwritten = _capi.resnet_conv(ctx, x, w, bias, ks, stride, res=res, relu=relu, tile=tile)
    assert guard == 0, (what, 'stores outside the output', guard)
    assert unwritten == 0, (what, 'outputs never written', unwritten)
    with np.errstate(invalid='ignore', over='ignore'):
        ref = conv_ref(x, w, bias, ks, stride, res, relu)
        bound = conv_bound(x, w, bias, ks, stride, res)
    assert np.array_equal(np.isfinite(y), np.isfinite(ref)) and np.array_equal(np.isnan(y), np.isnan(ref)), \
        (what, 'non-finite outputs differ from the reference')
    fin = np.isfinite(ref)
    with np.errstate(invalid='ignore'):
        err = np.abs(y.astype(np.float64) - ref)
        bad = fin & ~(err <= bound)
    assert not bad.any(), (what, int(bad.sum()), 'elements past the bound; worst error / bound',
                           float(np.nanmax(np.where(fin, err / bound, 0.0))), 'first at', np.argwhere(bad)[0].tolist())
    return y


def test_the_reference_is_conv2d():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(1)
    for ks, stride, H, W in [(1, 1, 5, 7), (1, 2, 5, 6), (3, 1, 5, 7), (3, 2, 5, 7), (3, 2, 6, 8), (3, 2, 1, 1), (3, 1, 1, 2),
                             (3, 2, 2, 1)]:
        x, w, bias, res = make(rng, ks, 2, H, W, 16, 32, stride)
        wt = torch.from_numpy(w.astype(np.float64).reshape(ks, ks, 16, 32)).permute(3, 2, 0, 1)
        t = F.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), wt, torch.from_numpy(bias.astype(np.float64)),
                     stride=stride, padding=ks // 2).permute(0, 2, 3, 1).numpy() + res
        ref = conv_ref(x, w, bias, ks, stride, res)
        assert ref.shape == t.shape and np.abs(ref - t).max() <= 1e-12 * np.abs(t).max()


@pytest.mark.parametrize('case', rs.FORCED_CASES, ids=lambda c: 'k%ds%d-%dx%d-n%dh%dw%d' % c)
def test_every_instantiation_forced(ctx, case):
    ks, stride, bn, bm, n, H, W = case
    rng = np.random.default_rng(abs(hash(case)) % 2 ** 31)
    x, w, bias, res = make(rng, ks, n, H, W, 32, 2 * bn, stride)
    check_conv(ctx, x, w, bias, ks, stride, res, True, (bn, bm), case)


GEOMETRY = [(3, 5, 7), (3, 6, 8), (3, 5, 1), (3, 5, 2), (3, 1, 7), (5, 1, 1), (2, 4, 9)]      # (n, H, W)


@pytest.mark.parametrize('ks,stride', rs.KS_STRIDE)
@pytest.mark.parametrize('tile', [None, (128, 64), (64, 128)])
def test_geometry_edges(ctx, ks, stride, tile):
    rng = np.random.default_rng(100 * ks + stride)
    bn = tile[0] if tile else 32
    for n, H, W in GEOMETRY:
        x, w, bias, res = make(rng, ks, n, H, W, 32, bn, stride)
        check_conv(ctx, x, w, bias, ks, stride, res, True, tile, (ks, stride, tile, n, H, W))
    for cin in (16, 32, 48, 256):
        for cout in (bn, 3 * bn):
            x, w, bias, res = make(rng, ks, 3, 5, 7, cin, cout, stride)
            check_conv(ctx, x, w, bias, ks, stride, res, False, tile, (ks, stride, tile, 'Cin', cin, 'Cout', cout))
    x, w, bias, res = make(rng, ks, 3, 6, 7, 48, bn, stride)
    for r in (None, res):
        for relu in (False, True):
            y = check_conv(ctx, x, w, bias, ks, stride, r, relu, tile, (ks, stride, tile, 'res', r is not None, 'relu', relu))
            assert (y.min() >= 0) == relu


def test_the_networks_own_layers(ctx):
    for ks, stride, cin, cout, H, W, n in rs.layer_cases(embedding=True):
        rng = np.random.default_rng(cin + cout + W + n)
        x, w, bias, res = make(rng, ks, n, H, W, cin, cout, stride, with_res=ks == 1)
        w *= np.float32(1.0 / np.sqrt(ks * ks * cin))
        check_conv(ctx, x, w, bias, ks, stride, res, True, None, (ks, stride, cin, cout, H, W, n))


@pytest.mark.parametrize('ks,stride', [(1, 1), (3, 2)])
def test_one_result_any_tile(ctx, ks, stride):
    rng = np.random.default_rng(7)
    x, w, bias, res = make(rng, ks, 3, 9, 11, 64, 256, stride)
    want = check_conv(ctx, x, w, bias, ks, stride, res, True, None, 'dispatcher')
    assert want[..., 0].size % 128 != 0 and want[..., 0].size % 64 != 0
    for tile in rs.TILES:
        y, guard, unwritten = _capi.resnet_conv(ctx, x, w, bias, ks, stride, res=res, relu=True, tile=tile)
        assert guard == 0 and unwritten == 0 and np.array_equal(y.view(np.uint32), want.view(np.uint32)), tile


@pytest.mark.parametrize('ks,stride', rs.KS_STRIDE)
@pytest.mark.parametrize('tile', [None, (128, 64)])
def test_non_finite_values(ctx, ks, stride, tile):
    rng = np.random.default_rng(9)
    x, w, bias, res = make(rng, ks, 3, 6, 7, 32, 128, stride)
    for relu in (False, True):
        for bad in (np.nan, np.inf):
            for pos in ((0, 0, 0, 0), (1, 3, 4, 17), (2, 5, 6, 31)):
                xb = x.copy()
                xb[pos] = bad
                y = check_conv(ctx, xb, w, bias, ks, stride, res, relu, tile, (ks, stride, tile, relu, bad, pos))
                if ks == 3 or stride == 1:
                    assert not np.isfinite(y).all()
        rb = res.copy()
        rb[1, 1, 2, 5] = np.nan
        y = check_conv(ctx, x, w, bias, ks, stride, rb, relu, tile, 'NaN in res')
        assert np.isnan(y).sum() == 1
        bb = bias.copy()
        bb[77] = np.nan
        y = check_conv(ctx, x, w, bb, ks, stride, res, relu, tile, 'NaN in bias')
        assert np.isnan(y[..., 77]).all() and np.isnan(y).sum() == y[..., 77].size


def test_refusals(ctx):
    rng = np.random.default_rng(3)
    x, w, bias, res = make(rng, 1, 2, 4, 4, 32, 128, 1)

    def refused(x=x, w=w, bias=bias, ks=1, stride=1, tile=None):
        with pytest.raises(_capi.VbxError, match=r'\(-1\): vbx_resnet_conv: .+'):
            _capi.resnet_conv(ctx, x, w, bias, ks, stride, tile=tile)

    refused(ks=2, w=np.zeros((4 * 32, 128), np.float32))
    refused(ks=5, w=np.zeros((25 * 32, 128), np.float32))
    refused(stride=3)
    refused(stride=0)
    refused(x=x[..., :8], w=w[:8])                                         # Cin = 8
    refused(x=np.zeros((2, 4, 4, 24), np.float32), w=np.zeros((24, 128), np.float32))
    refused(w=w[:, :48], bias=bias[:48])                                   # Cout = 48, dispatcher
    refused(w=w[:, :64], bias=bias[:64], tile=(128, 64))                   # Cout = 64 under BN = 128
    refused(w=w[:, :96], bias=bias[:96], tile=(64, 64))
    for tile in ((32, 64), (128, 32), (64, 0), (0, 128), (256, 128), (-32, 128)):
        refused(tile=tile)
    refused(x=x[:0])
    refused(x=x[:, :0])
    lib, y = ctx._lib, np.zeros(2 * 4 * 4 * 128, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, p(w), p(bias), p(y)), (p(x), None, p(bias), p(y)), (p(x), p(w), None, p(y)), (p(x), p(w), p(bias), None)):
        rc = lib.vbx_resnet_conv(ctx._h, 1, 1, 2, 4, 4, 32, 128, args[0], args[1], args[2], None, 0, 0, 0, args[3], 0)
        assert rc == -1 and b'NULL' in lib.vbx_last_error(ctx._h)
    assert lib.vbx_resnet_conv(ctx._h, 1, 1, 2, 4, 4, 32, 128, p(x), p(w), p(bias), None, 0, 0, 0, p(y), -1) == -1
    with pytest.raises(_capi.VbxError):
        _capi.resnet_conv_tile(100, 48)
    with pytest.raises(_capi.VbxError):
        _capi.resnet_conv_tile(0, 64)
    check_conv(ctx, x, w, bias, 1, 1, res, True, None, 'a valid call after the refusals')


# ---- stem ----------------------------------------------------------------------------------------------------------
# (n 64 T 32 is always a multiple of the 256 threads of a workgroup: the kernel's idx >= total guard never cuts a block)
@pytest.mark.parametrize('n,T', [(3, 1), (2, 2), (3, 3), (2, 10), (3, 143), (1, 144)])
def test_stem(ctx, n, T):
    rng = np.random.default_rng(T)
    x = rng.standard_normal((n, 64, T)).astype(np.float32)
    w = rng.standard_normal((9, 32)).astype(np.float32)
    bias = rng.standard_normal(32).astype(np.float32)
    y, guard, unwritten = _capi.resnet_stem(ctx, x, w, bias)
    assert guard == 0 and unwritten == 0
    ref = conv_ref(x[..., None], w, bias, 3, 1, relu=True)
    bound = gamma(9 + 1) * conv_ref(np.abs(x)[..., None], np.abs(w), np.abs(bias), 3, 1)
    assert y.shape == ref.shape and (np.abs(y - ref) <= bound).all(), float((np.abs(y - ref) / bound).max())
    # a NaN input touches exactly its 3 x 3 neighbourhood x 32 channels
    for h, t in {(0, 0), (63, T - 1), (31, T // 2)}:
        xb = x.copy()
        xb[n - 1, h, t] = np.nan
        yb, guard, unwritten = _capi.resnet_stem(ctx, xb, w, bias)
        want = np.zeros(y.shape, dtype=bool)
        want[n - 1, max(h - 1, 0):h + 2, max(t - 1, 0):t + 2] = True
        assert guard == 0 and unwritten == 0 and np.array_equal(np.isnan(yb), want)
        assert np.array_equal(yb[~want], y[~want])


# ---- pooling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W4', [1, 2, 3, 18, 19])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('kind', ['normal', 'constant', 'cancellation'])
def test_pool(ctx, n, W4, kind):
    rng = np.random.default_rng(W4 + 10 * n)
    x = rng.standard_normal((n, 8, W4, 1024)).astype(np.float32)
    if kind == 'constant':
        x[:] = x[:, :, :1]
    elif kind == 'cancellation':                              # mean 1e3, deviation 1e-2: what the f64 sums are there for
        x = (1e3 + 1e-2 * x).astype(np.float32)
    out, guard, unwritten = _capi.resnet_pool(ctx, x)
    assert guard == 0 and unwritten == 0 and out.shape == (n, 16384)
    xl = x.astype(np.longdouble)
    mean, msq = xl.mean(axis=2), (xl * xl).mean(axis=2)                    # [n][8][1024]: the output order h 1024 + c
    std = np.sqrt(msq - mean * mean + np.longdouble(1e-10))
    got_mean, got_std = out[:, :8192].reshape(n, 8, 1024), out[:, 8192:].reshape(n, 8, 1024)
    # one f32 rounding of the result, plus the f64 sum's own error
    tol = 2.0 ** -24 * np.abs(mean) + (W4 + 1) * 2.0 ** -53 * np.abs(xl).mean(axis=2)
    assert (np.abs(got_mean - mean) <= tol).all(), float((np.abs(got_mean - mean) / tol).max())
    # the final rounding to f32 (2^-24 std, doubled); then the f64 error of mean(x^2) - mean^2, at most about
    # (W4 + 2) 2^-53 mean(x^2) for the W4 additions and the two roundings of the subtraction, through the square root's
    # derivative 1 / (2 std), doubled
    tol = 2.0 ** -23 * std + (W4 + 2) * 2.0 ** -53 * msq / std
    assert (np.abs(got_std - std) <= tol).all(), float((np.abs(got_std - std) / tol).max())


def test_pool_output_order(ctx):
    x = np.zeros((2, 8, 3, 1024), np.float32)
    x[1, 5, :, 700] = 2.0
    out, _, _ = _capi.resnet_pool(ctx, x)
    assert out[1, 5 * 1024 + 700] == 2.0 and np.count_nonzero(out[:, :8192]) == 1
    assert np.allclose(out[:, 8192:], 1e-5, rtol=1e-6)
