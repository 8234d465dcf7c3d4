"""The split-mode convolution kernels of the x-vector network (vbx_resnet_split.hpp through vbx_resnet_conv_gemm) against
the same convolution in f64 on the CPU (test_gpu_resnet_kernels.conv_ref), fed the same f32 inputs.

The bound is derived from the representation, with no fitted factor.  Per product, with a' = a 2^ea and w' = w 2^ew
(ea from the largest finite |a| of the row's window, A; ew from the largest |w| of the output channel, Wc):

  * representation.  f16 keeps 11 significant bits, so |v - hi| <= 2^-11 2^E (E the exponent of hi), and lo = f16(v - hi)
    errs by half a unit of ITS last place: at most 2^-23 |v| while lo is a normal f16 number, and at most 2^-25 (half the
    subnormal spacing 2^-24) when it is not.  The scaled group maximum lies in [2^13, 2^14), so 2^-e <= 2^-13 amax and
    the floor is 2^-25 2^-13 amax = 2^-38 amax in unscaled terms:
        |a - (ah + al) 2^-ea| <= 2^-23 |a| + 2^-38 A =: da,      |w - (wh + wl) 2^-ew| <= 2^-23 |w| + 2^-38 Wc =: dw
    (The issue that asked for this mode wrote 2^-39 for the floors; that holds only for a group maximum of 2^14 or more,
    which [2^13, 2^14) excludes.  vbx_amd.xvector.split_terms reaches 2^-38.00 amax at amax = 1: test_xvector_split_host.)
  * the dropped term.  |al| <= 2^-11 |ah| <= 2^-11 (1 + 2^-11) |a'|, likewise wl: |al wl| <= 2^-22 (1 + 2^-10) |a' w'|.
  * what is summed, ah wh + ah wl + al wh = a' w' - da' w' - a' dw' + da' dw' - al wl, so per product the error is at most
        da |w| + |a| dw + da dw + 2^-22 (1 + 2^-10) |a| |w|
  * accumulation.  The f16 products are exact in f32 (11 + 11 bits); 3 K of them are added in f32, then the exact power-of-
    two scale, + bias, + res: gamma(3 K + 2) of the sum of magnitudes, gamma(m) = m u / (1 - m u), u = 2^-24.  The three
    summed terms together are at most (1 + 2^-9) |a' w'| in magnitude.

Over the K products, with S = sum |a| |w| (non-padded taps):

    |y - y64| <= (2 2^-23 + 2^-22 + gamma(3 K + 2)) (1 + 2^-9) (S + |bias| + |res|)
                 + 2^-38 (1 + 2^-22) (A sum |w| + Wc sum |a|) + taps 2^-76 A Wc

ReLU is 1-Lipschitz.  At K = 16 .. 64 the first factor is 3.3e-6 .. 1.2e-5: a kernel that leaves out hi lo or lo hi errs by
2^-12 = 2.4e-4 of a product and fails the small-K cases (checked once with such a build, which is not kept).

Non-finite inputs: the window's scale comes from its finite elements; a NaN reaches exactly the outputs it reaches in f64.
An Inf gives hi = Inf and lo = Inf - Inf = NaN, so the outputs it reaches are NaN where f64 gives +-Inf: for an Inf the test
asks for the same set of non-finite outputs, not the same kind, and takes that set from the f64 convolution BEFORE the
ReLU (f64 turns a -Inf into 0 there; a NaN stays, as the ReLU keeps NaN)."""
import ctypes as C

import numpy as np
import pytest

import resnet_shapes as rs
from test_gpu_resnet_kernels import conv_ref, gamma, make
from vbx_amd import _capi, xvector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return _capi.default_context(0)


def finite_amax(a, axis):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return np.where(np.isfinite(a), a, 0.0).max(axis=axis)


def split_bound(x, w, bias, ks, stride, res=None):
    K = ks * ks * x.shape[3]
    ax, aw = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64))
    zero = np.zeros(w.shape[1])
    S = conv_ref(ax, aw, np.abs(bias), ks, stride, None if res is None else np.abs(res))        # S + |bias| + |res|
    A = finite_amax(x.reshape(len(x), -1), 1)[:, None, None, None]
    Wc = finite_amax(w, 0)
    sum_w = conv_ref(np.ones_like(ax), aw, zero, ks, stride)
    sum_a = conv_ref(ax, np.ones_like(aw), zero, ks, stride)
    taps = conv_ref(np.ones_like(ax), np.ones_like(aw), zero, ks, stride)
    return (2 * 2.0 ** -23 + 2.0 ** -22 + gamma(3 * K + 2)) * (1 + 2.0 ** -9) * S \
        + 2.0 ** -38 * (1 + 2.0 ** -22) * (A * sum_w + Wc * sum_a) + taps * 2.0 ** -76 * A * Wc


def check_split(ctx, x, w, bias, ks, stride, res, relu, tile, what, same_kind=True):
    y, guard, unwritten, amax = _capi.resnet_conv_gemm(ctx, 'split', x, w, bias, ks, stride, res=res, relu=relu, tile=tile)
    assert guard == 0, (what, 'stores outside the output', guard)
    assert unwritten == 0, (what, 'outputs never written', unwritten)
    with np.errstate(invalid='ignore', over='ignore'):
        ref = conv_ref(x, w, bias, ks, stride, res, relu)
        bound = split_bound(x, w, bias, ks, stride, res)
    if same_kind:
        assert np.array_equal(np.isfinite(y), np.isfinite(ref)) and np.array_equal(np.isnan(y), np.isnan(ref)), \
            (what, 'non-finite outputs differ from the reference')
    else:                                       # an Inf input: NaN wherever the f64 convolution before the ReLU is not finite
        with np.errstate(invalid='ignore', over='ignore'):
            pre = conv_ref(x, w, bias, ks, stride, res, False)
        assert np.array_equal(np.isfinite(y), np.isfinite(pre)), (what, 'the set of non-finite outputs differs from the reference')
    fin = np.isfinite(ref) & np.isfinite(y)
    with np.errstate(invalid='ignore'):
        err = np.abs(y.astype(np.float64) - ref)
        bad = fin & ~(err <= bound)
        worst = float(np.nanmax(np.where(fin, err / bound, 0.0)))
    print('worst error / bound %.3f' % worst, what)
    assert not bad.any(), (what, int(bad.sum()), 'elements past the bound; worst error / bound', worst, 'first at',
                           np.argwhere(bad)[0].tolist())
    # what the kernel records for its consumer: max |y| over the finite outputs of every image, exactly
    want = finite_amax(y.reshape(len(y), -1), 1).astype(np.float32)
    assert np.array_equal(amax.view(np.uint32), want.view(np.uint32)), (what, 'per-window max |y|', amax, want)
    return y


@pytest.mark.parametrize('case', rs.FORCED_CASES, ids=lambda c: 'k%ds%d-%dx%d-n%dh%dw%d' % c)
def test_every_instantiation_forced(ctx, case):
    ks, stride, bn, bm, n, H, W = case
    rng = np.random.default_rng(abs(hash(case)) % 2 ** 31)
    x, w, bias, res = make(rng, ks, n, H, W, 32, 2 * bn, stride)
    check_split(ctx, x, w, bias, ks, stride, res, True, (bn, bm), case)


GEOMETRY = [(3, 5, 7), (3, 6, 8), (3, 5, 1), (3, 5, 2), (3, 1, 7), (5, 1, 1), (2, 4, 9), (2, 2, 2), (130, 1, 1)]      # (n, H, W)


@pytest.mark.parametrize('ks,stride', rs.KS_STRIDE)
@pytest.mark.parametrize('tile', [None] + rs.TILES)
def test_geometry_edges(ctx, ks, stride, tile):
    rng = np.random.default_rng(100 * ks + stride)
    bn = tile[0] if tile else 32
    for n, H, W in GEOMETRY:
        x, w, bias, res = make(rng, ks, n, H, W, 32, bn, stride)
        check_split(ctx, x, w, bias, ks, stride, res, True, tile, (ks, stride, tile, n, H, W))
    for cin in (16, 32, 48, 80, 256):
        for cout in (bn, 3 * bn):
            x, w, bias, res = make(rng, ks, 3, 5, 7, cin, cout, stride)
            check_split(ctx, x, w, bias, ks, stride, res, False, tile, (ks, stride, tile, 'Cin', cin, 'Cout', cout))
    x, w, bias, res = make(rng, ks, 3, 6, 7, 48, bn, stride)
    for r in (None, res):
        for relu in (False, True):
            y = check_split(ctx, x, w, bias, ks, stride, r, relu, tile, (ks, stride, tile, 'res', r is not None, 'relu', relu))
            assert (y.min() >= 0) == relu


@pytest.mark.parametrize('tile', [None] + rs.TILES)
@pytest.mark.parametrize('cin', [16, 32, 48, 64])
def test_small_k_sees_every_term(ctx, cin, tile):
    """K = 16 .. 64: the bound is 3.3e-6 .. 1.2e-5 of the magnitudes, a left-out hi lo or lo hi term is 2.4e-4."""
    rng = np.random.default_rng(cin)
    bn = tile[0] if tile else 64
    for stride in (1, 2):
        x, w, bias, res = make(rng, 1, 3, 9, 11, cin, bn, stride)
        bias *= np.float32(0.01)                                                   # (the bound is relative to S + |bias| + |res|)
        check_split(ctx, x, w, bias, 1, stride, None, False, tile, ('small K', cin, stride, tile))
    assert (2 * 2.0 ** -23 + 2.0 ** -22 + gamma(3 * cin + 2)) * (1 + 2.0 ** -9) < 2.0 ** -12 / 16


def test_the_networks_own_layers(ctx):
    for ks, stride, cin, cout, H, W, n in rs.layer_cases():
        rng = np.random.default_rng(cin + cout + W + n)
        x, w, bias, res = make(rng, ks, n, H, W, cin, cout, stride, with_res=ks == 1)
        w *= np.float32(1.0 / np.sqrt(ks * ks * cin))
        check_split(ctx, x, w, bias, ks, stride, res, True, None, (ks, stride, cin, cout, H, W, n))


@pytest.mark.parametrize('ks,stride', rs.KS_STRIDE)
@pytest.mark.parametrize('tile', [None, (128, 64), (64, 128), (32, 128)])
def test_windows_of_very_different_scale_in_one_tile(ctx, ks, stride, tile):
    """Images of 15 or fewer output positions, scaled by 2^0, 2^20, 2^-20, ...: every tile holds rows of many windows, and
    every row must meet the bound of its own window (a batch-wide scale would leave the small windows ~2^-20 / 2^-23 of
    their own magnitude as error)."""
    rng = np.random.default_rng(5 + ks + stride)
    bn = tile[0] if tile else 64
    x, w, bias, res = make(rng, ks, 40, 3, 5, 32, bn, stride)
    scale = np.float32(2.0) ** np.tile([0, 20, -20, 7], 10)
    x *= scale[:, None, None, None].astype(np.float32)
    bias[:] = 0
    y = check_split(ctx, x, w, bias, ks, stride, None, False, tile, ('scales', ks, stride, tile))
    assert np.abs(y[2]).max() < 2.0 ** -10 and np.abs(y[1]).max() > 2.0 ** 15
    w[:, 1::2] *= np.float32(2.0 ** -18)                                           # ... and channels of very different scale
    check_split(ctx, x, w, bias, ks, stride, None, False, tile, ('channel scales', ks, stride, tile))


@pytest.mark.parametrize('ks,stride', [(1, 1), (3, 2)])
def test_one_result_any_tile(ctx, ks, stride):
    rng = np.random.default_rng(7)
    x, w, bias, res = make(rng, ks, 3, 9, 11, 64, 256, stride)
    want = check_split(ctx, x, w, bias, ks, stride, res, True, None, 'dispatcher')
    assert want[..., 0].size % 128 != 0 and want[..., 0].size % 64 != 0
    for tile in rs.TILES:
        y, guard, unwritten, _ = _capi.resnet_conv_gemm(ctx, 'split', x, w, bias, ks, stride, res=res, relu=True, tile=tile)
        assert guard == 0 and unwritten == 0 and np.array_equal(y.view(np.uint32), want.view(np.uint32)), tile
    # a window's rows do not depend on the batch around it
    alone = _capi.resnet_conv_gemm(ctx, 'split', x[1:2], w, bias, ks, stride, res=res[1:2], relu=True)[0]
    assert np.array_equal(alone.view(np.uint32), want[1:2].view(np.uint32))


def test_exact_mode_of_the_two_mode_entry_is_vbx_resnet_conv(ctx):
    rng = np.random.default_rng(8)
    x, w, bias, res = make(rng, 3, 3, 9, 11, 32, 128, 2)
    a = _capi.resnet_conv(ctx, x, w, bias, 3, 2, res=res, relu=True)[0]
    b = _capi.resnet_conv_gemm(ctx, 'exact', x, w, bias, 3, 2, res=res, relu=True)[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('ks,stride', rs.KS_STRIDE)
@pytest.mark.parametrize('tile', [None, (128, 64)])
def test_non_finite_values(ctx, ks, stride, tile):
    """Three images of at most 42 output positions share one tile."""
    rng = np.random.default_rng(9)
    x, w, bias, res = make(rng, ks, 3, 6, 7, 32, 128, stride)
    for relu in (False, True):
        clean = check_split(ctx, x, w, bias, ks, stride, res, relu, tile, (ks, stride, tile, relu, 'clean'))
        for bad in (np.nan, np.inf, -np.inf):
            for pos in ((0, 0, 0, 0), (1, 3, 4, 17), (2, 5, 6, 31)):
                xb = x.copy()
                xb[pos] = bad
                y = check_split(ctx, xb, w, bias, ks, stride, res, relu, tile, (ks, stride, tile, relu, bad, pos),
                                same_kind=np.isnan(bad))
                if ks == 3 or stride == 1:
                    assert not np.isfinite(y).all()
                others = [b for b in range(3) if b != pos[0]]
                assert np.array_equal(y[others].view(np.uint32), clean[others].view(np.uint32)), 'another window changed'
        rb = res.copy()
        rb[1, 1, 2, 5] = np.nan
        y = check_split(ctx, x, w, bias, ks, stride, rb, relu, tile, 'NaN in res')
        assert np.isnan(y).sum() == 1
        bb = bias.copy()
        bb[77] = np.nan
        y = check_split(ctx, x, w, bb, ks, stride, res, relu, tile, 'NaN in bias')
        assert np.isnan(y[..., 77]).all() and np.isnan(y).sum() == y[..., 77].size


def test_refusals(ctx):
    rng = np.random.default_rng(3)
    x, w, bias, res = make(rng, 1, 2, 4, 4, 32, 128, 1)

    def refused(x=x, w=w, bias=bias, ks=1, stride=1, tile=None, gemm='split'):
        with pytest.raises(_capi.VbxError, match=r'\(-1\): vbx_resnet_conv_gemm: .+'):
            _capi.resnet_conv_gemm(ctx, gemm, x, w, bias, ks, stride, tile=tile)

    for gemm in ('split', 'exact'):
        refused(ks=2, w=np.zeros((4 * 32, 128), np.float32), gemm=gemm)
        refused(ks=5, w=np.zeros((25 * 32, 128), np.float32), gemm=gemm)
        refused(stride=3, gemm=gemm)
        refused(stride=0, gemm=gemm)
        refused(x=x[..., :8], w=w[:8], gemm=gemm)                                      # Cin = 8
        refused(x=np.zeros((2, 4, 4, 24), np.float32), w=np.zeros((24, 128), np.float32), gemm=gemm)
        refused(w=w[:, :48], bias=bias[:48], gemm=gemm)                                # Cout = 48, dispatcher
        refused(w=w[:, :64], bias=bias[:64], tile=(128, 64), gemm=gemm)                # Cout = 64 under BN = 128
        refused(w=w[:, :96], bias=bias[:96], tile=(64, 64), gemm=gemm)
        for tile in ((32, 64), (128, 32), (64, 0), (0, 128), (256, 128), (-32, 128)):
            refused(tile=tile, gemm=gemm)
        refused(x=x[:0], gemm=gemm)
        refused(x=x[:, :0], gemm=gemm)
    lib, y = ctx._lib, np.zeros(2 * 4 * 4 * 128, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, p(w), p(bias), p(y)), (p(x), None, p(bias), p(y)), (p(x), p(w), None, p(y)), (p(x), p(w), p(bias), None)):
        rc = lib.vbx_resnet_conv_gemm(ctx._h, 1, 1, 1, 2, 4, 4, 32, 128, args[0], args[1], args[2], None, 0, 0, 0, args[3], 0, None)
        assert rc == -1 and b'NULL' in lib.vbx_last_error(ctx._h)
    assert lib.vbx_resnet_conv_gemm(ctx._h, 1, 1, 1, 2, 4, 4, 32, 128, p(x), p(w), p(bias), None, 0, 0, 0, p(y), -1, None) == -1
    assert lib.vbx_resnet_conv_gemm(ctx._h, 2, 1, 1, 2, 4, 4, 32, 128, p(x), p(w), p(bias), None, 0, 0, 0, p(y), 0, None) == -1
    check_split(ctx, x, w, bias, 1, 1, res, True, None, 'a valid call after the refusals')
