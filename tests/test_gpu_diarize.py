"""``python -m vbx_amd.diarize`` -- wav files to RTTM in one process, the x-vectors kept on the device -- against the
two-program route it replaces, and the two device entry points under it:

  row flags          rows_nan_flags_kernel behind vbx_rows_nan_flags: np.isnan(x).any(1), exactly
  device projection  vbx_xvectors_project_device: bit for bit vbx_xvectors_project of a host copy of the kept rows
  the whole route    predict + vbhmm in fresh child processes against diarize with the same arguments: the same RTTM bytes

Every comparison is an equality of bits or bytes.  The device arrays of the first two groups come from the HIP runtime the
library itself is bound to (its hipMalloc, reached through the library's handle), so they are plain device memory to it as
a torch tensor's storage is in the child processes of the third group.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diarize_util as du
import frontend_ref as fr

pytestmark = pytest.mark.gpu
REPO = du.REPO
ENV = dict(os.environ, PYTHONPATH=REPO)
# The transform and the PLDA are those of real x-vectors; the synthetic network's embeddings share one large component they
# do not centre, so the voices lie close together in their space.  AHC separates them at a threshold of 0; VB-HMM keeps
# them apart with the speaker prior weak against the data (Fa 4, Fb 1) and merges them at the recipe's Fa 0.3, Fb 17
# (worked out with the CPU stages of tests/test_driver.py on the network's f32 CPU forward, not with the code under test).
THRESHOLD, FA, FB = '0.0', '4.0', '1.0'
HYPER = ['--threshold', THRESHOLD, '--lda-dim', '128', '--Fa', FA, '--Fb', FB, '--loopP', '0.99']


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


class DeviceArray:
    """A host array copied into device memory of the runtime libvbx_hip.so uses."""

    def __init__(self, ctx, a):
        self.lib = ctx._lib
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipFree.argtypes = [C.c_void_p]
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(a.nbytes, 4)) == 0
        self.ptr = p.value
        assert self.lib.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0          # hipMemcpyHostToDevice

    def close(self):
        if self.ptr:
            assert self.lib.hipFree(self.ptr) == 0
            self.ptr = None


# ---- row flags -----------------------------------------------------------------------------------------------------
def _nan_patterns(n, D):
    """{name: [(row, column)]} of NaN placements for an [n][D] array."""
    cols = sorted({0, D // 2, D - 1})
    rows = {'first row': [0], 'last row': [n - 1], 'two adjacent rows': sorted({n // 2, min(n // 2 + 1, n - 1)})}
    out = {'none': []}
    for rname, rr in rows.items():
        for c in cols:
            out[f'{rname}, column {c}'] = [(r, c) for r in rr]
    out['every row'] = [(r, (7 * r) % D) for r in range(n)]
    return out


@pytest.mark.parametrize('D', [256, 5, 63])
@pytest.mark.parametrize('n', [1, 4, 5, 63, 64, 65, 257])
def test_row_flags_are_numpys_isnan_any(n, D, ctx):
    from vbx_amd import _capi
    rng = np.random.default_rng(1000 * n + D)
    base = rng.standard_normal((n, D)).astype(np.float32)
    for name, where in _nan_patterns(n, D).items():
        x = base.copy()
        x[n // 3] = np.inf                                      # a row of +inf is no NaN row ...
        x[(n // 3 + 2) % n, D - 1] = -np.inf
        for r, c in where:
            x[r, c] = np.nan                                    # ... unless one is put into it
        if where and n > 2:
            x[where[0][0], where[0][1]] = np.float32(np.uint32(0xFFC00001).view(np.float32))          # a negative NaN with a payload
        want = np.isnan(x).any(1)
        assert want.sum() == len({r for r, _ in where})
        d = DeviceArray(ctx, x)
        try:
            got = _capi.nan_rows(ctx, d.ptr, n, D)
        finally:
            d.close()
        assert got.dtype == bool and got.shape == (n,)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])


def test_row_flags_refuse_bad_arguments(ctx):
    from vbx_amd import _capi
    x = np.zeros((4, 8), dtype=np.float32)
    d = DeviceArray(ctx, x)
    flags = np.zeros(4, dtype=np.int32)
    try:
        lib = ctx._lib
        for ptr, n, D, out in ((None, 4, 8, flags), (d.ptr, 0, 8, flags), (d.ptr, -1, 8, flags), (d.ptr, 4, 0, flags),
                               (d.ptr, 4, 8, None)):
            rc = lib.vbx_rows_nan_flags(ctx._h, C.c_void_p(ptr), n, D, _capi._ptr(out))
            assert rc != 0
            with pytest.raises(_capi.VbxError, match='bad argument'):
                ctx.check(rc, 'vbx_rows_nan_flags')
        with pytest.raises(_capi.VbxError, match='not device memory'):      # a host array is not what the kernel may read
            _capi.nan_rows(ctx, x.ctypes.data, 4, 8)
        assert _capi.nan_rows(ctx, d.ptr, 0, 8).shape == (0,)
        assert not _capi.nan_rows(ctx, d.ptr, 4, 8).any()                   # (the context is as usable as before)
    finally:
        d.close()


# ---- device projection ---------------------------------------------------------------------------------------------
GRID = sorted({s[:4] for s in fr.SHAPES})


def _keep_lists(n):
    lists = {'all': None, 'all, listed': np.arange(n), 'drop first': np.arange(1, n), 'drop last': np.arange(n - 1),
             'drop two adjacent in the middle': np.delete(np.arange(n), [n // 2, min(n // 2 + 1, n - 1)]),
             'keep one': np.array([n // 2])}
    return {k: v for k, v in lists.items() if v is None or len(v) > 0}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize('shape', GRID, ids=[f'n{s[0]}-Din{s[1]}-Dl{s[2]}-fea{s[3]}' for s in GRID])
def test_device_projection_has_the_bits_of_the_projection_of_a_host_copy(shape, ctx):
    from vbx_amd import _capi
    n, din, dl, fea_dim = shape
    c = fr.make_case(shape + (np.float32,), seed=2000 + GRID.index(shape))
    assert c['x'].dtype == np.float32 and c['x'].shape == (n, din)
    model = (c['mean1'], c['lda'], c['mean2'], c['plda_mu'], c['plda_tr'])
    d = DeviceArray(ctx, c['x'])
    try:
        for name, rows in _keep_lists(n).items():
            host = _capi.XVectors(ctx, c['x'] if rows is None else c['x'][rows], *model, fea_dim)
            dev = _capi.XVectors.from_device(ctx, d.ptr, n, din, rows, *model, fea_dim)
            try:
                assert dev.n == host.n == (n if rows is None else len(rows)) and (dev.dl, dev.fea_dim) == (dl, fea_dim)
                for which in (0, 1):
                    a, b = dev.get(which), host.get(which)
                    assert a.shape == b.shape == (dev.n, (dl, fea_dim)[which])
                    assert np.array_equal(_bits(a), _bits(b)), (name, which)
                assert np.array_equal(_bits(dev.get(0)), _bits(dev.get('xproj'))) and np.array_equal(_bits(dev.get(1)), _bits(dev.get('fea')))
            finally:
                host.close()
                dev.close()
    finally:
        d.close()


def test_resident_scores_of_device_projected_rows_are_the_same_bits(ctx):
    from vbx_amd import _capi
    shape = (130, 257, 200, 130)
    n, din, dl, fea_dim = shape
    c = fr.make_case(shape + (np.float32,), seed=2100)
    model = (c['mean1'], c['lda'], c['mean2'], c['plda_mu'], c['plda_tr'])
    rows = np.delete(np.arange(n), [0, 64, 65, n - 1])
    d = DeviceArray(ctx, c['x'])
    host = _capi.XVectors(ctx, c['x'][rows], *model, fea_dim)
    dev = _capi.XVectors.from_device(ctx, d.ptr, n, din, rows, *model, fea_dim)
    try:
        for row0, T in ((0, len(rows)), (len(rows) // 3, 70)):
            a = _capi.Scores.cos_similarity_resident(ctx, dev, row0, T)
            b = _capi.Scores.cos_similarity_resident(ctx, host, row0, T)
            try:
                assert len(a) == len(b) == T * T and np.array_equal(_bits(a.get()), _bits(b.get()))
            finally:
                a.close()
                b.close()
    finally:
        host.close()
        dev.close()
        d.close()


def test_device_projection_refuses_bad_arguments(ctx):
    from vbx_amd import _capi
    n, din, dl, fea_dim = 17, 63, 30, 17
    c = fr.make_case((n, din, dl, fea_dim, np.float32), seed=2200)
    model = [np.ascontiguousarray(c[k], dtype=np.float64) for k in ('mean1', 'lda', 'mean2', 'plda_mu', 'plda_tr')]
    d = DeviceArray(ctx, c['x'])
    lib = ctx._lib

    def call(x_ptr, n_src, n_, rows, fea_dim_=fea_dim, models=model, context=ctx, out=True):
        h = C.c_void_p()
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        rc = lib.vbx_xvectors_project_device(context._h, n_src, din, dl, fea_dim_, C.c_void_p(x_ptr), n_, _capi._ptr(rows),
                                             *[_capi._ptr(m) for m in models], C.byref(h) if out else None)
        assert not h.value
        context.check(rc, 'vbx_xvectors_project_device')

    try:
        for rows, message in (([2, 2], 'does not increase'), ([3, 1], 'does not increase'), ([0, 5, 4, 9], 'does not increase'),
                              ([0, n], 'outside'), ([-1, 3], 'outside'), ([n + 5], 'outside')):
            with pytest.raises(_capi.VbxError, match=message):
                call(d.ptr, n, len(rows), rows)
            with pytest.raises(_capi.VbxError, match=message):
                _capi.XVectors.from_device(ctx, d.ptr, n, din, rows, *model, fea_dim)
        for args in ((d.ptr, n, 0, []), (d.ptr, n, -1, None), (d.ptr, 0, 0, None), (d.ptr, n, n - 1, None),      # n <= 0; NULL rows, n != n_src
                     (d.ptr, n, n + 1, np.arange(n + 1)), (None, n, n, None)):
            with pytest.raises(_capi.VbxError, match='bad argument'):
                call(*args)
        with pytest.raises(_capi.VbxError, match='bad argument'):
            _capi.XVectors.from_device(ctx, d.ptr, n, din, [], *model, fea_dim)
        for k in range(5):                                                   # every model pointer; the result pointer
            with pytest.raises(_capi.VbxError, match='bad argument'):
                call(d.ptr, n, n, None, models=[None if j == k else m for j, m in enumerate(model)])
        with pytest.raises(_capi.VbxError, match='bad argument'):
            call(d.ptr, n, n, None, out=False)
        for bad in (0, dl + 1):
            with pytest.raises(_capi.VbxError, match='bad argument'):
                call(d.ptr, n, n, None, fea_dim_=bad)
        # memory that is not this context's device's: a host array; with a second GPU, a context of that device
        with pytest.raises(_capi.VbxError, match='not device memory of device 0'):
            call(c['x'].ctypes.data, n, n, None)
        count = C.c_int()
        assert lib.hipGetDeviceCount(C.byref(count)) == 0
        if count.value > 1:
            other = _capi.Context(1)
            try:
                with pytest.raises(_capi.VbxError, match='not device memory of device 1'):
                    call(d.ptr, n, n, None, context=other)
            finally:
                other.close()
                assert lib.hipSetDevice(0) == 0
        # (the context and the array are as usable as before)
        xv = _capi.XVectors.from_device(ctx, d.ptr, n, din, None, *model, fea_dim)
        assert np.all(np.isfinite(xv.get(1)))
        xv.close()
    finally:
        d.close()


# ---- the whole route -----------------------------------------------------------------------------------------------
def _child(module_argv, timeout=300):
    res = subprocess.run([sys.executable, '-m'] + module_argv, env=ENV, cwd=REPO, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


def _predict_argv(p, ark, seg, extra):
    return ['vbx_amd.predict', '--gpus', '0', '--checkpoint', p['ckpt'], '--in-file-list', p['list'], '--in-lab-dir', p['lab'],
            '--in-wav-dir', p['wav'], '--out-ark-fn', ark, '--out-seg-fn', seg, '--batch-size', '16'] + list(extra)


def _vbhmm_argv(p, ark, seg, out, extra):
    return ['vbx_amd.vbhmm', '--out-rttm-dir', out, '--xvec-ark-file', ark, '--segments-file', seg, '--xvec-transform',
            p['transform'], '--plda-file', p['plda']] + HYPER + list(extra)


def _diarize_argv(p, out, extra):
    return ['vbx_amd.diarize', '--gpus', '0', '--checkpoint', p['ckpt'], '--in-file-list', p['list'], '--in-lab-dir', p['lab'],
            '--in-wav-dir', p['wav'], '--batch-size', '16', '--out-rttm-dir', out, '--xvec-transform', p['transform'],
            '--plda-file', p['plda']] + HYPER + list(extra)


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('diarize')
    p = du.write_corpus(tmp, du.standard_corpus())
    p.update(du.write_models(tmp), ckpt=du.write_checkpoint(tmp), tmp=str(tmp))
    return p


@pytest.fixture(scope='module')
def predicted(corpus):
    """gemm -> (ark, seg) written by ``python -m vbx_amd.predict``, once per mode."""
    cache = {}

    def get(gemm):
        if gemm not in cache:
            ark, seg = (os.path.join(corpus['tmp'], f'{gemm}.{ext}') for ext in ('ark', 'seg'))
            _child(_predict_argv(corpus, ark, seg, ['--gemm', gemm]))
            cache[gemm] = (ark, seg)
        return cache[gemm]
    return get


ROUTES = {
    'ahc+vb, second speaker': ('exact', ['--init', 'AHC+VB', '--output-2nd', 'True']),
    'ahc only': ('exact', ['--init', 'AHC']),
    'plda scores': ('exact', ['--init', 'AHC+VB', '--ahc-scores', 'plda', '--target-energy', '0.5']),
    'split gemm': ('split', ['--init', 'AHC+VB', '--output-2nd', 'True']),
}


def _assert_the_input_is_not_trivial(first, second):
    """On the two-step output, so a property of the input: at least two recordings with >= 2 speakers and >= 6 RTTM lines,
    and a second-speaker file that differs from its first-speaker file."""
    stats = {f: du.rttm_speakers_and_lines(data) for f, data in first.items()}
    print('two-step route: (speakers, lines) per file:', stats)
    assert sum(1 for s, l in stats.values() if s >= 2 and l >= 6) >= 2, stats
    assert any(second[f] != first[f] for f in second), 'every second-speaker file equals its first-speaker file'


@pytest.mark.parametrize('route', list(ROUTES), ids=[r.replace(' ', '-').replace(',', '') for r in ROUTES])
def test_one_process_writes_the_rttm_bytes_of_the_two_step_route(route, corpus, predicted, tmp_path):
    gemm, extra = ROUTES[route]
    ark, seg = predicted(gemm)
    two, one = str(tmp_path / 'two'), str(tmp_path / 'one')
    _child(_vbhmm_argv(corpus, ark, seg, two, extra))
    side = [str(tmp_path / 'one.ark'), str(tmp_path / 'one.seg')]
    _child(_diarize_argv(corpus, one, extra + ['--gemm', gemm, '--out-ark-fn', side[0], '--out-seg-fn', side[1]]))
    want, want2 = du.rttm_dir(two), du.rttm_dir(two + '2nd')
    assert sorted(want) == ['recA.rttm', 'recB.rttm', 'recC.rttm']
    if '--output-2nd' in extra:
        assert set(want2) <= set(want)
        _assert_the_input_is_not_trivial(want, want2)
    else:
        assert want2 == {}
    got, got2 = du.rttm_dir(one), du.rttm_dir(one + '2nd')
    assert sorted(got) == sorted(want) and sorted(got2) == sorted(want2)
    for f in want:
        assert got[f] == want[f], f
    for f in want2:
        assert got2[f] == want2[f], f
    # the side product: predict's two files
    assert open(side[1], 'rb').read() == open(seg, 'rb').read()
    assert open(side[0], 'rb').read() == open(ark, 'rb').read()
    keys = [l.split()[0] for l in open(seg).read().splitlines()]
    spans = [tuple(int(v) for v in k.rsplit('_', 1)[1].split('-')[1:]) for k in keys]
    assert any(a == 0 and b < 144 for a, b in spans), 'no segment that yields a tail window alone'


def _dropped(stderr):
    return [l.split('NaN found, not processing: ', 1)[1].strip() for l in stderr.splitlines() if 'NaN found, not processing: ' in l]


def test_nan_embeddings_are_dropped_as_predict_drops_them(tmp_path):
    """A network that overflows on one kind of input (diarize_util.write_checkpoint(overflow=True)) and recordings that hold
    it: recN -- voices, then a VAD segment of bursts; recZ -- bursts only, of which no x-vector is left (the two-step route
    never sees it); recA -- voices only.  (Digital silence without dither, the input the front end's golden cases suggest,
    gives no NaN here: the front end floors the Mel energies at 1 and the network is finite on zeros.)"""
    a = du.synth_recording(5, 16000, 8, 2)
    n = du.synth_recording(6, 16000, 8, 2, bursts=2.5)
    z = (np.rint(du.burst(3 * 16000, 16000, np.random.default_rng(8))).astype(np.int16), '0.100000 2.900000 sp\n')
    p = du.write_corpus(tmp_path, {'recN': (n[0], 16000, n[1]), 'recZ': (z[0], 16000, z[1]), 'recA': (a[0], 16000, a[1])})
    p.update(du.write_models(tmp_path), ckpt=du.write_checkpoint(tmp_path, overflow=True))
    ark, seg, two, one = (str(tmp_path / f) for f in ('x.ark', 'x.seg', 'two', 'one'))
    extra = ['--init', 'AHC+VB', '--output-2nd', 'True']
    pre = _child(_predict_argv(p, ark, seg, []))
    dropped = _dropped(pre.stderr)
    kept = [l.split()[0] for l in open(seg).read().splitlines()]
    print('predict dropped', len(dropped), 'keys and kept', len(kept))
    assert len(dropped) >= 1 and any(k.startswith('recN_') for k in dropped)
    assert any(k.startswith('recN_') for k in kept) and any(k.startswith('recA_') for k in kept)
    assert not any(k.startswith('recZ_') for k in kept) and any(k.startswith('recZ_') for k in dropped)
    _child(_vbhmm_argv(p, ark, seg, two, extra))
    res = _child(_diarize_argv(p, one, extra + ['--out-ark-fn', str(tmp_path / 'one.ark'), '--out-seg-fn', str(tmp_path / 'one.seg')]))
    assert _dropped(res.stderr) == dropped
    want = du.rttm_dir(two)
    assert sorted(want) == ['recA.rttm', 'recN.rttm']
    assert du.rttm_dir(one) == want and du.rttm_dir(one + '2nd') == du.rttm_dir(two + '2nd')
    assert open(tmp_path / 'one.seg', 'rb').read() == open(seg, 'rb').read()
    assert open(tmp_path / 'one.ark', 'rb').read() == open(ark, 'rb').read()
    # no x-vector left of recZ: no RTTM file and one log line
    assert len([l for l in res.stderr.splitlines() if 'recZ: no x-vector left' in l]) == 1


LIBRARY_CALL = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
p = json.load(open(sys.argv[2]))
from vbx_amd import diarize
names = [l.strip() for l in open(p['list'])]
state, timing = diarize.diarize_files(names, p['wav'], p['lab'], p['ckpt'], p['transform'], p['plda'], out_rttm_dir=p['out'],
                                      threshold=float(p['threshold']), Fa=float(p['Fa']), Fb=float(p['Fb']), output_2nd=True,
                                      batch_size=16)
out = {'timing': json.dumps(timing), 'names': np.array(list(state))}
for name, st in state.items():
    assert set(st) == {'labels1st', 'labels2nd', 'n_iters', 'thr', 'starts', 'ends'}, set(st)
    for key in ('labels1st', 'labels2nd', 'starts', 'ends'):
        if st[key] is not None:                                  # (no second speaker where VB-HMM kept one)
            out[f'{name}/{key}'] = np.asarray(st[key])
    out[f'{name}/n_iters'] = st['n_iters']
np.savez(p['npz'], **out)
print('library call OK')
'''


def test_the_library_call_returns_the_labels_the_rttm_files_encode(corpus, tmp_path):
    import io
    from vbx_amd.kaldi_formats import write_rttm
    from vbx_amd.vbhmm import merge_adjacent_labels
    p = dict(corpus, out=str(tmp_path / 'rttm'), npz=str(tmp_path / 'state.npz'), threshold=THRESHOLD, Fa=FA, Fb=FB)
    with open(tmp_path / 'p.json', 'w') as f:
        json.dump(p, f)
    res = subprocess.run([sys.executable, '-c', LIBRARY_CALL, REPO, str(tmp_path / 'p.json')], env=ENV, cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'library call OK' in res.stdout, res.stderr[-3000:]
    g = np.load(p['npz'], allow_pickle=False)
    timing = json.loads(str(g['timing']))
    for key in ('read', 'fbank', 'network', 'project', 'ahc', 'vb', 'rttm', 'total'):
        assert isinstance(timing[key], float) and timing[key] >= 0.0, key
    assert timing['total'] >= timing['network'] > 0.0
    assert g['names'].tolist() == ['recA', 'recB', 'recC']
    files, files2 = du.rttm_dir(p['out']), du.rttm_dir(p['out'] + '2nd')
    assert sorted(files) == ['recA.rttm', 'recB.rttm', 'recC.rttm'] and len(files2) >= 1
    for name in g['names'].tolist():
        assert int(g[f'{name}/n_iters']) >= 1
        for key, data in (('labels1st', files), ('labels2nd', files2)):
            if f'{name}/{key}' not in g.files:
                assert key == 'labels2nd' and f'{name}.rttm' not in data
                continue
            labels, starts, ends = g[f'{name}/{key}'], g[f'{name}/starts'], g[f'{name}/ends']
            assert labels.shape == starts.shape == ends.shape and np.all(ends > starts)
            fp = io.StringIO()
            write_rttm(fp, name, *[merge_adjacent_labels(starts, ends, labels)[i] for i in (2, 0, 1)])
            assert fp.getvalue().encode() == data[f'{name}.rttm'], (name, key)
