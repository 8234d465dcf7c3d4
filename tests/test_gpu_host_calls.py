"""The host side the one-shot entry points share (vbx_host_call.hpp: the holder of a call's device blocks; vbx_rttm_score.hpp:
the plan both scorers run the three RTTM kernels on).  Neither has numbers of its own, so both tests compare bytes: a context a
call has failed on against a fresh one, and the two entry points that share the plan against each other.
"""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
Q = 2.0 ** -10                                 # the time grid of tests/test_gpu_score.py: every sum below is exact in float64


def test_a_failed_call_leaves_the_context_clean():
    """vbx_frame_counts is refused after its first phase has allocated, launched and synchronized (out one entry too small);
    the same context then gives the bytes a fresh one gives"""
    from vbx_amd import _capi
    # one pair, two reference and two system turns: the smallest input that reaches the second phase
    counts = np.array([[2, 2, 2, 2]], dtype=np.int32)
    extent = np.array([[0.0, 1.0]])
    turns = np.array([[0.0, 0.5], [0.25, 1.0], [0.0, 0.75], [0.5, 1.0]])
    spk = np.array([0, 1, 0, 1], dtype=np.int32)
    fresh = _capi.Context(0)
    info0, classes0, out0 = _capi.frame_counts(fresh, counts, extent, turns, spk, 0.01)
    need = 2 + 2 + 2 * 2 + int(info0[0, 1]) * int(info0[0, 2])
    assert info0[0, 0] >= 2 and need <= out0.size
    ctx = _capi.Context(0)
    info, classes, out = np.zeros_like(info0), np.zeros_like(classes0), np.zeros(need, dtype=np.int64)
    rc = ctx._lib.vbx_frame_counts(ctx._h, 1, _capi._ptr(counts), _capi._ptr(extent), _capi._ptr(turns), _capi._ptr(spk), 0.01,
                                   _capi._ptr(info), _capi._ptr(classes), _capi._ptr(out), need - 1)
    assert rc != 0
    with pytest.raises(_capi.VbxError, match=f'the result has {need} entries, out has room for {need - 1}'):
        ctx.check(rc, 'vbx_frame_counts')
    info1, classes1, out1 = _capi.frame_counts(ctx, counts, extent, turns, spk, 0.01)
    assert info1.tobytes() == info0.tobytes() and classes1.tobytes() == classes0.tobytes()
    assert out1[:need].tobytes() == out0[:need].tobytes()
    fresh.close()
    ctx.close()


def test_one_plan_behind_both_entry_points():
    """T = kLabBlock + 1 alternating labels against two reference speakers: the label route's turns cross a scan pass and the pair
    has more than one classification block; vbx_labels_score and vbx_rttm_score on numpy's turns and score._Pair's edges agree
    bit for bit"""
    from vbx_amd import _capi, build, score
    src = open(os.path.join(build.CSRC, 'vbx_labels_score.hpp')).read() + open(os.path.join(build.CSRC, 'vbx_rttm_score.hpp')).read()
    c = {k: int(v) for k, v in re.findall(r'constexpr int (k\w+) = (\d+);', src)}
    T = c['kLabBlock'] + 1
    starts = 1.0 + 8 * np.arange(T) * Q                               # windows of 48 grid steps every 8: neighbours overlap
    ends = starts + 48 * Q
    labels = (np.arange(T) % 2).astype(np.int32)
    ref = [(0.5, 1.75, 'a'), (1.5, 2.5, 'b'), (2.25, 3.5, 'a'), (3.0, 4.0, 'b')]
    collar = 0.25
    ctx = _capi.default_context(0)
    r = score._LabelsRef(ref, starts, ends, collar)
    assert r.ok and len(r.ref_names) == 2
    lab_out, info = _capi.labels_score(ctx, [(T, r.rb.size, 2, r.edges.size)], np.concatenate([r.starts, r.ends]),
                                       np.stack([r.rb, r.re], axis=1), r.rs, r.edges, [(0, 2)], labels, collar, False)
    turns = score.labels_turns(starts, ends, labels)
    pair = score._Pair(ref, turns, collar)
    assert info[0, 0] == len(turns) == T and len(turns) > c['kLabBlock']             # the turns cross a scan pass
    assert info[0, 1] == pair.edges.size and pair.edges.size - 1 > c['kRttmClsBlock']   # more than one classification block
    assert (pair.n_ref, pair.n_sys) == (2, 2)
    rttm_out = _capi.rttm_score(ctx, *score._pack([pair]), collar, False)
    assert lab_out.size == rttm_out.size == 4 + 2 * 2
    assert lab_out.tobytes() == rttm_out.tobytes()
    assert lab_out[0] > 0                                             # reference speech was scored
