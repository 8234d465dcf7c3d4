"""Ragged batches of the x-vector network, host side (no GPU): the layout tables, the kernel-case table of
tests/ragged_shapes.py, the argument checks that need no device, and how predict cuts a file's tail windows into batches."""
import ctypes as C

import numpy as np
import pytest

import ragged_shapes as rg
import resnet_shapes as rs
from vbx_amd import _capi, predict, xvector


def layout_by_loop(lengths):
    n = len(lengths)
    pos = [[0] * (n + 1) for _ in range(4)]
    wid = [[0] * n for _ in range(4)]
    for b, T in enumerate(lengths):
        W = T
        for lvl in range(4):
            if lvl:
                W = (W - 1) // 2 + 1
            wid[lvl][b] = W
    for lvl, H in enumerate((64, 32, 16, 8)):
        for b in range(n):
            pos[lvl][b + 1] = pos[lvl][b] + H * wid[lvl][b]
    return pos, wid


@pytest.mark.parametrize('lengths', [[144], [1], [1, 2, 3, 4, 5, 6, 7, 8, 9], rg.NETWORK_LENGTHS, [144, 19, 128, 20, 20, 77],
                                     list(range(10, 145))[::-1]], ids=lambda v: f'n{len(v)}')
def test_ragged_layout_is_the_direct_loop(lengths):
    pos, wid = xvector.ragged_layout(lengths)
    want_pos, want_wid = layout_by_loop(lengths)
    assert pos.dtype == np.int64 and wid.dtype == np.int32
    assert pos.shape == (4, len(lengths) + 1) and wid.shape == (4, len(lengths))
    assert pos.tolist() == want_pos and wid.tolist() == want_wid
    # the widths are the ones the network walk gives a window of that length alone, level by level
    for b, T in enumerate(lengths):
        seen = sorted({W for _, _, W in xvector.walk(T)}, reverse=True)
        assert seen == sorted(set(wid[:, b].tolist()), reverse=True)


def test_ragged_layout_past_2_31():
    pos, _ = xvector.ragged_layout([2 ** 24] * 3)
    assert pos[0, 3] == 3 * 64 * 2 ** 24 > 2 ** 31


def test_ragged_layout_refuses_bad_lengths():
    with pytest.raises(ValueError, match='no windows'):
        xvector.ragged_layout([])
    with pytest.raises(ValueError, match=r'window 2 has 0 frames'):
        xvector.ragged_layout([5, 7, 0, 3])
    with pytest.raises(ValueError, match=r'window 0 has -4 frames'):
        xvector.ragged_layout([-4])


def test_kernel_case_table_meets_its_conditions():
    assert len(rg.INSTANTIATIONS) == 20 and len(set(rg.INSTANTIATIONS)) == 20
    assert {(ks, s) for ks, s, _, _ in rg.INSTANTIATIONS} == set(rs.KS_STRIDE)
    assert {(bn, bm) for _, _, bn, bm in rg.INSTANTIATIONS} == set(rs.TILES)
    for _, stride, _, bm in rg.INSTANTIATIONS:
        rg.check_cases(stride, bm, rg.kernel_cases(stride, bm))
    # the check itself sees a table that lacks something
    for drop in range(3):
        cases = rg.kernel_cases(1, 64)
        del cases[drop]
        with pytest.raises(AssertionError):
            rg.check_cases(1, 64, cases)
    assert set(rg.STEM_WIDTHS) == {1, 2, 3, 18}
    assert set(rg.NETWORK_LENGTHS) == {1, 2, 9, 10, 11, 23, 143, 144, 145, 167}


def test_entry_points_refuse_a_null_handle():
    lib = _capi.load()
    T = np.array([3, 4], dtype=np.int32)
    buf = np.zeros(64 * 7, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    assert lib.vbx_resnet_run_ragged(None, 2, p(T), p(buf), 0, p(buf), 0) == -1
    assert lib.vbx_resnet_input_ragged(None, 2, p(T), C.byref(out)) == -1
    assert lib.vbx_fbank_windows_ragged(None, 2, p(np.zeros(2, np.int64)), p(T), p(buf), 0) == -1
    assert lib.vbx_resnet_conv_ragged(None, 0, 1, 1, 2, 1, p(T), 16, 32, p(buf), p(buf), p(buf), None, 0, 0, 0, p(buf), 0, None) == -1
    assert lib.vbx_resnet_stem_ragged(None, 2, p(T), p(buf), p(buf), p(buf), p(buf), 0) == -1
    assert lib.vbx_resnet_pool_ragged(None, 2, p(T), p(buf), p(buf), 0) == -1


def test_embed_ragged_checks_its_arguments_before_the_device():
    net = object.__new__(xvector.ResNet101)                # (no device: every refusal comes before the first call to it)
    net.embed_dim = 8
    assert net.embed_ragged([]).shape == (0, 8)
    assert net.embed_windows_ragged(None, [], []).shape == (0, 8)
    with pytest.raises(ValueError, match=r'window 1: expected \[64\]\[T\]'):
        net.embed_ragged([np.zeros((64, 3), np.float32), np.zeros((63, 3), np.float32)])
    with pytest.raises(ValueError, match='window 1 has 0 frames'):
        net.embed_ragged(np.zeros(64 * 3, np.float32), [3, 0])
    with pytest.raises(ValueError, match=r'the lengths ask for 64 x 7'):
        net.embed_ragged(np.zeros(64 * 6, np.float32), [3, 4])
    with pytest.raises(ValueError, match='2 starts, 1 lengths'):
        net.embed_windows_ragged(None, [0, 5], [3])


def test_predict_cuts_the_tails_into_bounded_batches():
    lengths = [100, 40, 10, 144, 1, 143, 143, 20]
    parts = predict.ragged_batches(lengths, 288)
    assert [i for p in parts for i in p] == list(range(len(lengths)))
    assert all(p and sum(lengths[i] for i in p) <= 288 for p in parts)
    assert parts == [[0, 1, 2], [3, 4, 5], [6, 7]]
    assert predict.ragged_batches([], 288) == []
    assert predict.ragged_batches([144, 144], 144) == [[0], [1]]
    assert predict.ragged_batches([300], 144) == [[0]]       # (a window is never split)


def test_the_row_lookup_enumerates_every_window_in_order():
    """What a ragged kernel does with the tables: row m belongs to the last window b with pos[b] <= m, and
    (m - pos[b]) = ho W_b + wo walks that window's [H][W_b] positions row by row."""
    lengths = [5, 1, 144, 2, 19, 1, 33]
    pos, wid = xvector.ragged_layout(lengths)
    for lvl, H in enumerate((64, 32, 16, 8)):
        m = np.arange(pos[lvl, -1])
        b = np.searchsorted(pos[lvl], m, side='right') - 1
        assert b.min() == 0 and b.max() == len(lengths) - 1 and (np.diff(b) >= 0).all()
        rem = m - pos[lvl, b]
        ho, wo = rem // wid[lvl, b], rem % wid[lvl, b]
        assert (ho < H).all()
        for k in range(len(lengths)):
            sel = b == k
            want = [(h, w) for h in range(H) for w in range(wid[lvl, k])]
            assert list(zip(ho[sel].tolist(), wo[sel].tolist())) == want
