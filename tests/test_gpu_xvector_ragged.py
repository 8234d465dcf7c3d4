"""Windows of mixed lengths through the x-vector network in one batch (the *_ragged entry points): every window must have
THE SAME BITS as that window run alone through the uniform path, kernel by kernel and through the whole network, in both
gemm modes.  That is not a tolerance: a ragged kernel reads the same taps in the same k order and zeros where a tap is
padded, so any difference is an indexing fault.  tests/test_gpu_resnet_kernels.py and tests/test_gpu_xvector.py pin the
single-window side to f64.  Outputs are compared as uint32 (a NaN equals itself), guard bands and sentinels must be intact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ragged_shapes as rg
import resnet_shapes as rs
from vbx_amd import _capi, fbank, xvector
from vbx_amd import kaldi_formats as kf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_PATH = os.path.join(REPO, 'tests', 'golden', 'resnet_cases.npz')
F_PATH = os.path.join(REPO, 'tests', 'golden', 'fbank_cases.npz')
R, F = np.load(R_PATH), np.load(F_PATH)
SEED, E = int(R['seed']), int(R['embed_dim'])
NAMES = [str(n) for n in F['names']]
GEMMS = ['exact', 'split']


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def ctx():
    return _capi.default_context(0)


# ---- kernel by kernel ------------------------------------------------------------------------------------------------
def make(rng, ks, stride, H, widths, cin, cout):
    xs = [rng.standard_normal((H, W, cin)).astype(np.float32) * np.float32(1 + b) for b, W in enumerate(widths)]
    w = rng.standard_normal((ks * ks * cin, cout)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    res = [rng.standard_normal((rs.rn_out(H, stride), rs.rn_out(W, stride), cout)).astype(np.float32) for W in widths]
    return xs, w, bias, res


def check_ragged_conv(ctx, gemm, xs, w, bias, ks, stride, res, relu, tile, what):
    ys, guard, unwritten, amax = _capi.resnet_conv_ragged(ctx, gemm, xs, w, bias, ks, stride, res=res, relu=relu, tile=tile)
    assert guard == 0, (what, 'stores outside the output', guard)
    assert unwritten == 0, (what, 'outputs never written', unwritten)
    for b, x in enumerate(xs):
        r = None if res is None else res[b][None]
        # (the dispatcher's tile depends on M: a window alone is pinned to the tile the batch ran with)
        alone, g1, u1, a1 = _capi.resnet_conv_gemm(ctx, gemm, x[None], w, bias, ks, stride, res=r, relu=relu, tile=tile)
        assert g1 == 0 and u1 == 0
        assert ys[b].shape == alone[0].shape, (what, b)
        diff = bits(ys[b]) != bits(alone[0])
        assert not diff.any(), (what, 'window', b, int(diff.sum()), 'elements differ, first at', np.argwhere(diff)[0].tolist())
        assert bits(amax[b:b + 1])[0] == bits(a1)[0], (what, 'amax_y of window', b, float(amax[b]), float(a1[0]))
    return ys


@pytest.mark.parametrize('gemm', GEMMS)
@pytest.mark.parametrize('inst', rg.INSTANTIATIONS, ids=lambda c: 'k%ds%d-%dx%d' % c)
def test_every_instantiation_ragged(ctx, gemm, inst):
    ks, stride, bn, bm = inst
    rng = np.random.default_rng(1000 * ks + 100 * stride + bn + bm)
    for H, widths, cin, cf in rg.kernel_cases(stride, bm):
        xs, w, bias, res = make(rng, ks, stride, H, widths, cin, cf * bn)
        for r, relu in ((res, True), (None, False)):
            ys = check_ragged_conv(ctx, gemm, xs, w, bias, ks, stride, r, relu, (bn, bm), (inst, H, widths, cin, relu))
            assert (min(float(y.min()) for y in ys) >= 0) == relu


@pytest.mark.parametrize('gemm', GEMMS)
def test_the_dispatchers_tile_and_non_finite_windows(ctx, gemm):
    rng = np.random.default_rng(5)
    widths = [7, 1, 40, 2, 18, 3]
    for ks, stride in rs.KS_STRIDE:
        xs, w, bias, res = make(rng, ks, stride, 8, widths, 32, 128)
        M = sum(rg.out_rows(8, widths, stride))
        tile = _capi.resnet_conv_tile(M, 128)
        want = check_ragged_conv(ctx, gemm, xs, w, bias, ks, stride, res, True, tile, (ks, stride, 'forced', tile))
        ys, guard, unwritten, _ = _capi.resnet_conv_ragged(ctx, gemm, xs, w, bias, ks, stride, res=res, relu=True)
        assert guard == 0 and unwritten == 0
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ys, want)), (ks, stride, 'dispatcher', tile)
        # a NaN and an Inf stay in their windows, bit for bit what those windows give alone; the rest does not move
        bad = [x.copy() for x in xs]
        bad[2][3, 20, 5] = np.nan
        bad[4][0, 0, 0] = np.inf
        got = check_ragged_conv(ctx, gemm, bad, w, bias, ks, stride, res, True, tile, (ks, stride, 'non-finite'))
        for b in (0, 1, 3, 5):
            assert np.isfinite(got[b]).all() and np.array_equal(bits(got[b]), bits(want[b])), b
        if ks == 3 or stride == 1:
            assert not np.isfinite(got[2]).all() and not np.isfinite(got[4]).all()


def test_stem_ragged(ctx):
    rng = np.random.default_rng(6)
    xs = [rng.standard_normal((64, T)).astype(np.float32) for T in rg.STEM_WIDTHS]
    w = rng.standard_normal((9, 32)).astype(np.float32)
    bias = rng.standard_normal(32).astype(np.float32)
    for order in (range(len(xs)), reversed(range(len(xs)))):
        order = list(order)
        ys, guard, unwritten = _capi.resnet_stem_ragged(ctx, [xs[b] for b in order], w, bias)
        assert guard == 0 and unwritten == 0
        for y, b in zip(ys, order):
            alone, g1, u1 = _capi.resnet_stem(ctx, xs[b][None], w, bias)
            assert g1 == 0 and u1 == 0 and np.array_equal(bits(y), bits(alone[0])), b


def test_pool_ragged(ctx):
    rng = np.random.default_rng(7)
    xs = [(3.0 + rng.standard_normal((8, W4, 1024))).astype(np.float32) for W4 in rg.STEM_WIDTHS]
    xs[1][2, 0, 77] = np.nan
    for order in (range(len(xs)), reversed(range(len(xs)))):
        order = list(order)
        out, guard, unwritten = _capi.resnet_pool_ragged(ctx, [xs[b] for b in order])
        assert guard == 0 and unwritten == 0 and out.shape == (len(xs), 16384)
        for y, b in zip(out, order):
            alone, g1, u1 = _capi.resnet_pool(ctx, xs[b][None])
            assert g1 == 0 and u1 == 0 and np.array_equal(bits(y), bits(alone[0])), b
    assert np.isnan(out).sum() == 2                            # the mean and the deviation of one (h, c) of one window


def test_an_equal_width_batch_has_the_same_bits_through_both_entries(ctx):
    """The uniform and the ragged kernels are instantiations of one body chosen in one place: n = 3 windows of one width give
    the same bits through the uniform entry (whose own window index -- m / (Ho Wo), t / 64, bh >> 3 -- the tests above see
    at n = 1 only) as through the ragged one.  The convolution has M = 36 rows < BM: three windows inside one tile, the
    first wave's 32-row slab over all three; in the split mode amax_y and y itself also compare the two amax kernels."""
    rng = np.random.default_rng(9)

    def same(a, b, what):
        (ya, ga, ua), (yb, gb, ub) = a[:3], b[:3]
        assert ga == 0 and gb == 0 and ua == 0 and ub == 0, (what, ga, gb, ua, ub)
        assert len(ya) == len(yb) == 3, what
        for j in range(3):
            assert np.array_equal(bits(ya[j]), bits(yb[j])), (what, 'window', j)

    xs = [rng.standard_normal((64, 5)).astype(np.float32) for _ in range(3)]
    w = rng.standard_normal((9, 32)).astype(np.float32)
    bias = rng.standard_normal(32).astype(np.float32)
    same(_capi.resnet_stem(ctx, np.stack(xs), w, bias), _capi.resnet_stem_ragged(ctx, xs, w, bias), 'stem')
    xs = [(3.0 + rng.standard_normal((8, 3, 1024))).astype(np.float32) for _ in range(3)]
    same(_capi.resnet_pool(ctx, np.stack(xs)), _capi.resnet_pool_ragged(ctx, xs), 'pool')
    xs, w, bias, res = make(rng, 3, 2, 8, [5, 5, 5], 16, 32)
    for gemm in GEMMS:
        a = _capi.resnet_conv_gemm(ctx, gemm, np.stack(xs), w, bias, 3, 2, res=np.stack(res), relu=True, tile=(32, 128))
        b = _capi.resnet_conv_ragged(ctx, gemm, xs, w, bias, 3, 2, res=res, relu=True, tile=(32, 128))
        same(a, b, ('conv', gemm))
        assert np.array_equal(bits(a[3]), bits(b[3])), ('amax_y', gemm, a[3], b[3])
        assert (a[3] > 0).all() == (gemm == 'split')


def test_step_entry_points_refuse_bad_arguments(ctx):
    rng = np.random.default_rng(8)
    xs, w, bias, res = make(rng, 1, 1, 2, [3, 1, 4], 16, 32)
    lib = ctx._lib
    p = lambda a: None if a is None else a.ctypes.data_as(_capi.C.c_void_p)
    x = np.concatenate([a.reshape(-1) for a in xs])
    y = np.zeros(2 * 8 * 32, np.float32)

    def conv(n=3, W=np.array([3, 1, 4], np.int32), x=x, w=w, bias=bias, y=y, gemm=0, ks=1, stride=1, tile=(0, 0), cin=16, cout=32):
        return lib.vbx_resnet_conv_ragged(ctx._h, gemm, ks, stride, n, 2, p(W), cin, cout, p(x), p(w), p(bias), None, 0, tile[0],
                                          tile[1], p(y), 0, None)

    def refused(match, **kw):
        assert conv(**kw) == -1
        msg = lib.vbx_last_error(ctx._h).decode()
        assert msg.startswith('vbx_resnet_conv_ragged: ') and match in msg, msg

    refused('n = 0', n=0)
    refused('n = -2', n=-2)
    refused('NULL', W=None)
    refused('window 1 has T = 0', W=np.array([3, 0, 4], np.int32))
    refused('window 2 has T = -1', W=np.array([3, 1, -1], np.int32))
    for name in ('x', 'w', 'bias', 'y'):
        refused('NULL', **{name: None})
    refused('gemm', gemm=2)
    refused('kernel size', ks=2)
    refused('stride', stride=3)
    refused('Cin = 8', cin=8)
    refused('Cout = 48', cout=48)
    refused('tile', tile=(32, 64))
    assert conv() == 0
    T = np.array([3, 0], np.int32)
    buf = np.zeros(64 * 3 * 32, np.float32)
    assert lib.vbx_resnet_stem_ragged(ctx._h, 2, p(T), p(buf), p(buf), p(buf), p(buf), 0) == -1
    assert 'vbx_resnet_stem_ragged: window 1 has T = 0' in lib.vbx_last_error(ctx._h).decode()
    assert lib.vbx_resnet_stem_ragged(ctx._h, 0, p(T), p(buf), p(buf), p(buf), p(buf), 0) == -1
    assert lib.vbx_resnet_stem_ragged(ctx._h, 1, p(T), None, p(buf), p(buf), p(buf), 0) == -1
    assert 'NULL' in lib.vbx_last_error(ctx._h).decode()
    assert lib.vbx_resnet_pool_ragged(ctx._h, 2, p(T), p(buf), p(buf), 0) == -1
    assert 'vbx_resnet_pool_ragged: window 1 has T = 0' in lib.vbx_last_error(ctx._h).decode()
    assert lib.vbx_resnet_pool_ragged(ctx._h, 1, None, p(buf), p(buf), 0) == -1
    assert lib.vbx_resnet_pool_ragged(ctx._h, 1, p(T), p(buf), None, 0) == -1


# ---- the network -----------------------------------------------------------------------------------------------------
def window(j):
    name = NAMES[R['win_rec'][j]]
    rows = F['rows_' + name]
    s, a, n = int(R['win_seg'][j]), int(R['win_start'][j]), int(R['win_len'][j])
    r0 = int(rows[:s].sum())
    return np.ascontiguousarray(F['fea_' + name][r0 + a:r0 + a + n].T, dtype=np.float32)


@pytest.fixture(scope='module')
def windows():
    return [window(j) for j in range(len(R['win_len']))]


@pytest.fixture(scope='module', params=GEMMS)
def net(request):
    return xvector.ResNet101.from_checkpoint(xvector.synthetic_state_dict(SEED, E), gemm=request.param)


@pytest.fixture(scope='module')
def alone(net, windows):
    """every fixture window through the uniform path on its own: computed once per gemm mode, never changed"""
    out = np.stack([net.embed(w[None])[0] for w in windows])
    out.setflags(write=False)
    return out


def test_the_fixture_windows_in_one_call(net, windows, alone):
    lens = sorted({w.shape[1] for w in windows})
    assert len(windows) == 41 and lens[-1] == 144 and lens[0] >= 19 and lens[-2] <= 128
    got = net.embed_ragged(windows)
    assert got.shape == (41, E) and got.dtype == np.float32 and np.isfinite(got).all()
    assert net.gemm_in_effect() == net.dev.gemm_in_effect() and sum(net.times().values()) > 0
    for j in range(41):
        assert np.array_equal(bits(got[j]), bits(alone[j])), (j, windows[j].shape[1])
    order = np.random.default_rng(21).permutation(41)
    assert (order != np.arange(41)).any()
    shuffled = net.embed_ragged([windows[j] for j in order])
    assert np.array_equal(bits(shuffled), bits(alone[order]))
    # one concatenated array and the lengths: the other form of the same call
    flat = net.embed_ragged(np.concatenate([w.reshape(-1) for w in windows]), [w.shape[1] for w in windows])
    assert np.array_equal(bits(flat), bits(alone))
    if net.gemm_in_effect() == 'exact':
        for j in range(41):
            scale = np.abs(R['emb_f64'][j]).max()
            assert np.abs(got[j] - R['emb_ref'][j]).max() <= 2e-5 * scale, j
            assert np.abs(got[j] - R['emb_f64'][j]).max() <= 1e-5 * scale, j


def test_lengths_the_cli_never_makes(net, windows):
    rng = np.random.default_rng(22)
    base = np.concatenate([windows[0], windows[1][:, ::-1]], axis=1)
    assert base.shape[1] >= max(rg.NETWORK_LENGTHS)
    xs = [(base[:, :T] + 0.1 * rng.standard_normal((64, T))).astype(np.float32) for T in rg.NETWORK_LENGTHS]
    got = net.embed_ragged(xs)
    assert got.shape == (len(xs), E)
    for x, g in zip(xs, got):
        assert np.array_equal(bits(g), bits(net.embed(x[None])[0])), x.shape[1]


def test_a_batch_of_one_window(net, windows, alone):
    for j in (0, 7):
        assert np.array_equal(bits(net.embed_ragged([windows[j]])), bits(alone[j:j + 1])), j


def test_a_nan_window_among_finite_ones(net, windows, alone):
    idx = [3, 0, 11, 25, 40]
    xs = [windows[j].copy() for j in idx]
    xs[2][17, xs[2].shape[1] // 2] = np.nan
    got = net.embed_ragged(xs)
    assert np.isnan(got[2]).all()
    assert np.array_equal(bits(got[[0, 1, 3, 4]]), bits(alone[[3, 0, 25, 40]]))


def test_run_ragged_refuses_bad_arguments(net):
    lib, h, ctx = net.ctx._lib, net.dev._h, net.ctx
    p = lambda a: None if a is None else a.ctypes.data_as(_capi.C.c_void_p)
    x, out = np.zeros(64 * 7, np.float32), np.zeros((2, E), np.float32)
    T = np.array([3, 4], np.int32)
    ptr = _capi.C.c_void_p()
    for args, match in (((0, p(T), p(x), 0, p(out), 0), 'n = 0'), ((-1, p(T), p(x), 0, p(out), 0), 'n = -1'),
                        ((2, None, p(x), 0, p(out), 0), 'NULL'), ((2, p(T), None, 0, p(out), 0), 'NULL'),
                        ((2, p(T), p(x), 0, None, 0), 'NULL'),
                        ((2, p(np.array([3, 0], np.int32)), p(x), 0, p(out), 0), 'window 1 has T = 0'),
                        ((2, p(np.array([-5, 4], np.int32)), p(x), 0, p(out), 0), 'window 0 has T = -5')):
        assert lib.vbx_resnet_run_ragged(h, *args) == -1
        msg = lib.vbx_last_error(ctx._h).decode()
        assert msg.startswith('vbx_resnet_run_ragged: ') and match in msg, msg
    assert lib.vbx_resnet_input_ragged(h, 2, p(np.array([3, 0], np.int32)), _capi.C.byref(ptr)) == -1
    assert 'vbx_resnet_input_ragged: window 1 has T = 0' in lib.vbx_last_error(ctx._h).decode()
    assert lib.vbx_resnet_input_ragged(h, 0, p(T), _capi.C.byref(ptr)) == -1
    assert lib.vbx_resnet_input_ragged(h, 2, p(T), None) == -1
    assert lib.vbx_resnet_run_ragged(h, 2, p(T), p(x), 0, p(out), 0) == 0


# ---- the front end, device inputs, the command line -------------------------------------------------------------------
def _front_end(name='rec16'):
    sr = int(F['rates'][NAMES.index(name)])
    labs = np.atleast_2d((np.loadtxt(str(F['lab_' + name]).splitlines(), usecols=(0, 1)) * sr).astype(int))
    fe = fbank.front_end(sr)
    sig, segs = fbank.prepare(F['sig_' + name].astype(np.int64), labs, sr)
    return fe, fe.run([(sig, segs)])[0], segs, sr


def test_ragged_gather_equals_the_gather_per_length():
    fe, rows, _, _ = _front_end()
    total = fe.dev.rows
    starts = [0, 5, 100, 3, 7, 0, total - 1, total - 144, 24, 1]
    lens = [144, 26, 1, 26, 144, 2, 1, 144, 19, 128]
    got = fe.dev.windows_ragged(starts, lens)
    assert got.shape == (64 * sum(lens),)
    off = 0
    for s, n in zip(starts, lens):
        want = fe.dev.windows([s], n)[0]
        assert np.array_equal(bits(got[off:off + 64 * n].reshape(64, n)), bits(want)), (s, n)
        off += 64 * n
    for bad_starts, bad_lens, match in (([0, -1], [3, 3], 'window 1'), ([0, total - 2], [3, 3], 'past the'), ([0, 1], [3, 0], 'lens = 0')):
        with pytest.raises(_capi.VbxError, match=match):
            fe.dev.windows_ragged(bad_starts, bad_lens)
    with pytest.raises(_capi.VbxError, match='n = 0'):
        fe.dev.windows_ragged([], [])


DEVICE_INPUTS = '''
import sys
import numpy as np
import torch                                          # first: libvbx_hip.so then binds to PyTorch's HIP runtime
sys.path.insert(0, sys.argv[1])
from vbx_amd import fbank, xvector
g = np.load(sys.argv[2])
r = np.load(sys.argv[3])
sr = 16000
labs = np.atleast_2d((np.loadtxt(str(g['lab_rec16']).splitlines(), usecols=(0, 1)) * sr).astype(int))
fe = fbank.front_end(sr)
sig, segs = fbank.prepare(g['sig_rec16'].astype(np.int64), labs, sr)
rows = fe.run([(sig, segs)])[0]
starts, lens = [0, 24, 3, 130, 7, 48], [144, 26, 26, 144, 1, 77]
for gemm in ('exact', 'split'):
    net = xvector.ResNet101.from_checkpoint(xvector.synthetic_state_dict(int(r['seed']), int(r['embed_dim'])), gemm=gemm)
    host = [fe.windows([s], n)[0] for s, n in zip(starts, lens)]
    a = net.embed_ragged(host)
    flat = torch.from_numpy(np.concatenate([w.reshape(-1) for w in host])).cuda()
    b = net.embed_ragged(flat, lens)
    assert b.device.type == 'cuda' and b.dtype == torch.float32 and tuple(b.shape) == a.shape
    c = net.embed_windows_ragged(fe, starts, lens)
    assert np.array_equal(b.cpu().numpy().view(np.uint32), a.view(np.uint32)), gemm
    assert np.array_equal(c.view(np.uint32), a.view(np.uint32)), gemm
    for s, n, e in zip(starts, lens, a):
        assert np.array_equal(net.embed_windows(fe, [s], n)[0].view(np.uint32), e.view(np.uint32)), (gemm, s, n)
print('device inputs OK')
'''


def test_device_inputs_give_the_same_bits():
    res = subprocess.run([sys.executable, '-c', DEVICE_INPUTS, REPO, F_PATH, R_PATH], capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0 and 'device inputs OK' in res.stdout, res.stderr[-3000:]


def test_cli_writes_the_vectors_of_every_window_alone(tmp_path):
    """The inputs of test_gpu_xvector.py::test_cli_with_a_checkpoint_reproduces_predict_py: the ark holds exactly what
    embed_windows(fe, [start], length) gives window by window, and the segments file is the fixture's."""
    import torch
    from vbx_amd import predict
    wav, lab = tmp_path / 'wav', tmp_path / 'lab'
    wav.mkdir()
    lab.mkdir()
    for name, sr in zip(NAMES, F['rates']):
        fbank.write_wav(str(wav / f'{name}.wav'), F['sig_' + name], int(sr))
        (lab / f'{name}.lab').write_text(str(F['lab_' + name]))
    (tmp_path / 'list.txt').write_text(''.join(n + '\n' for n in NAMES))
    ck = str(tmp_path / 'ckpt.pth')
    sd = xvector.synthetic_state_dict(SEED, E)
    torch.save({'state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    ark, seg = str(tmp_path / 'out.ark'), str(tmp_path / 'out.seg')
    argv = ['--gpus', '0', '--checkpoint', ck, '--in-file-list', str(tmp_path / 'list.txt'), '--in-lab-dir', str(lab),
            '--in-wav-dir', str(wav), '--out-ark-fn', ark, '--out-seg-fn', seg, '--batch-size', '16']
    res = subprocess.run([sys.executable, '-m', 'vbx_amd.predict'] + argv, env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = list(kf.read_vec_flt_ark(ark))
    # the same files window by window, one run of the network each
    args = predict.parse_args(argv)
    net = xvector.ResNet101(sd)
    want, lines, ragged_calls = [], [], []
    for name in NAMES:
        sr, sig, segs = predict._load(args, name)
        fe = fbank.front_end(sr)
        rows = fe.run([(sig, segs)])[0]
        for w in fbank.window_plan(name, segs, sr, args.seg_len, args.seg_jump):
            want.append((w.key, net.embed_windows(fe, [rows[w.seg] + w.start], w.end - w.start)[0]))
            lines.append(w.line)

        def spy(fe_, starts, lengths):
            ragged_calls.append(list(lengths))
            return net.embed_windows_ragged(fe_, starts, lengths)
        via = predict.embed_file(net.embed_windows, fe, name, sig, segs, sr, args, spy)
        assert [k for k, _, _ in via] == [k for k, _ in want[-len(via):]]
    assert [k for k, _ in got] == [k for k, _ in want]
    for (key, a), (_, b) in zip(got, want):
        assert a.dtype == np.float32 and np.array_equal(bits(a), bits(b)), key
    with open(seg) as f:
        text = f.read()
    assert text == str(R['segments']) and text == ''.join(line + os.linesep for line in lines)
    # the tails did go through the ragged path, mixed lengths together, bounded batches
    assert ragged_calls and any(len(set(c)) > 1 for c in ragged_calls)
    assert all(144 not in c and sum(c) <= 16 * 144 for c in ragged_calls)
