"""The device route of ``vbx_amd.metrics`` (vbx_frame_score.hpp: frame_bounds / frame_sort / frame_cells / frame_masks /
frame_firsts / frame_classes / frame_acc behind vbx_frame_counts) against the numpy route of the same module and against the
dense referee ``tests/metrics_ref.py``.  Everything the device returns is an integer: every comparison here is exact.

All pairs of this file go to the device in ONE call (the fixture ``scored``); the tests compare what came back.
"""
import os

import numpy as np
import pytest

import metrics_ref
from metrics_util import CLASSES_OVER_CAP, CRAFTED, SPEAKERS_64, SPEAKERS_65, chain, grid_pair, random_pair
from test_score_host import REF_RTTM, es2005a  # noqa: F401  (es2005a: the fixture that writes the system RTTM)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BLOCK = 256                                    # kFrmBlock: boundaries, cells, result entries per workgroup; turns, cells per LDS chunk

# ---- tile edges: kFrmBlock is the one constant that tiles anything ------------------------------------------------------
# chain(n) against one turn of the other side: n cells, n + 1 turns, 2 n + 4 boundaries (their number is always even).
# Cells 255, 256, 257 and 511, 512, 513; turns 255, 256, 257; boundaries 254, 256, 258 and 510, 512, 514; and with
# grid_pair(k, s) a result of k + s + 2 k s = 255, 256, 257 entries (test_tile_edge_pairs_have_the_sizes_they_are_meant_to).
CHAINS = (125, 126, 127, 253, 254, 255, 256, 257, 511, 512, 513)
EDGES = {f'chain_{n}': (chain(n), [(0.0, 1.0, 'x')]) for n in CHAINS}
EDGES.update({f'sys_chain_{n}': ([(0.0, 1.0, 'A')], chain(n, ('x', 'y', 'z'))) for n in (255, 256, 257)})
ENTRIES = {'entries_255': grid_pair(36, 3), 'entries_256': grid_pair(28, 4), 'entries_257': grid_pair(51, 2)}
RANDOM = {f'random_{seed}': random_pair(seed) for seed in range(36)}
ALL = dict(CRAFTED, **SPEAKERS_64, **SPEAKERS_65, **EDGES, **ENTRIES, **RANDOM, classes_over_cap=CLASSES_OVER_CAP)


@pytest.fixture(scope='module')
def scored():
    from vbx_amd import metrics
    names = list(ALL)
    return dict(zip(names, metrics.frame_counts([ALL[n] for n in names], device=0)))


@pytest.fixture(scope='module')
def host():
    from vbx_amd import metrics
    names = list(ALL)
    return dict(zip(names, metrics.frame_counts([ALL[n] for n in names], device=None)))


@pytest.mark.parametrize('name', [n for n in ALL if n not in RANDOM])
def test_device_equals_the_numpy_route(name, scored, host):
    metrics_ref.assert_counts_equal(scored[name], host[name], name)


def test_tile_edge_pairs_have_the_sizes_they_are_meant_to(host):
    from vbx_amd import metrics
    cells, turns, bounds = set(), set(), set()
    for name in EDGES:
        p = metrics._Frames(*ALL[name])
        times = np.concatenate([p.rb, p.re, p.sb, p.se, [p.lo, p.hi]])
        cells.add(np.unique(metrics._frame_index(times, 0.01, p.n_frames(0.01))).size - 1)
        turns.add(p.rb.size + p.sb.size)
        bounds.add(times.size)
    assert cells >= {BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1}
    assert turns >= {BLOCK - 1, BLOCK, BLOCK + 1}
    assert bounds >= {BLOCK - 2, BLOCK, BLOCK + 2, 2 * BLOCK - 2, 2 * BLOCK, 2 * BLOCK + 2}
    entries = {sum(host[name][k].size for k in ('ref_durs', 'sys_durs', 'inter', 'cm')) for name in ENTRIES}
    assert entries == {BLOCK - 1, BLOCK, BLOCK + 1}


@pytest.mark.parametrize('name', list(RANDOM) + list(EDGES) + list(ENTRIES))
def test_device_equals_the_referee(name, scored):
    ref, hyp = ALL[name]
    metrics_ref.assert_counts_equal(scored[name], metrics_ref.counts(ref, hyp), name)


def test_limits_taken_and_fallen_back(scored):
    """64 speakers a side go to the device, 65 and 512 classes come from the numpy route: told apart at the entry point"""
    from vbx_amd import _capi, metrics
    ctx = _capi.default_context(0)
    for name, (ref, hyp) in SPEAKERS_64.items():
        p = metrics._Frames(ref, hyp)
        assert max(p.n_ref, p.n_sys) == 64
        info, classes, flat = _capi.frame_counts(ctx, *metrics._pack([p]), 0.01)
        rec = scored[name]
        assert info[0, 1:3].tolist() == [len(rec['ref_classes']), len(rec['sys_classes'])]
        assert flat[:p.n_ref].tolist() == rec['ref_durs'].tolist() and flat[p.n_ref:p.n_ref + p.n_sys].tolist() == rec['sys_durs'].tolist()
    p = metrics._Frames(*SPEAKERS_65['ref_65'])
    with pytest.raises(_capi.VbxError, match='at most 64'):
        _capi.frame_counts(ctx, *metrics._pack([p]), 0.01)
    p = metrics._Frames(*CLASSES_OVER_CAP)
    info, classes, flat = _capi.frame_counts(ctx, *metrics._pack([p]), 0.01)
    assert info[0].tolist() == [512, 512, 2, 0] and flat.size >= p.n_ref + p.n_sys + p.n_ref * p.n_sys
    assert len(scored['classes_over_cap']['ref_classes']) == 512             # the record is there all the same


def test_entry_point_refuses_what_it_cannot_index():
    from vbx_amd import _capi
    ctx = _capi.default_context(0)
    ok = _capi.frame_counts(ctx, [[1, 1, 1, 1]], [[0.0, 1.0]], [[0.0, 1.0], [0.0, 0.5]], [0, 0], 0.01)
    assert ok[0][0].tolist() == [2, 1, 2, 0] and ok[2][:4].tolist() == [100, 50, 50, 50]
    for counts, extent, turns, spk, step in (
            ([[1, 1, 1, 1]], [[0.0, 1.0]], [[0.0, 1.0], [0.0, 0.5]], [0, 1], 0.01),         # a speaker outside [0, n_sys)
            ([[1, 1, 1, 1]], [[0.0, 1.0]], [[0.0, 1.5], [0.0, 0.5]], [0, 0], 0.01),         # a turn outside the extent
            ([[1, 1, 1, 1]], [[0.0, 1.0]], [[0.5, 0.25], [0.0, 0.5]], [0, 0], 0.01),        # a turn that ends before it begins
            ([[1, 1, 1, 1]], [[0.0, 1.0]], [[0.0, 1.0], [0.0, 0.5]], [0, 0], 0.0),          # no step
            ([[1, 1, 1, 1]], [[0.0, 1e12]], [[0.0, 1.0], [0.0, 0.5]], [0, 0], 1e-3)):       # 2^40 frames or more
        with pytest.raises(_capi.VbxError):
            _capi.frame_counts(ctx, counts, extent, turns, spk, step)
    again = _capi.frame_counts(ctx, [[1, 1, 1, 1]], [[0.0, 1.0]], [[0.0, 1.0], [0.0, 0.5]], [0, 0], 0.01)
    assert all(np.array_equal(a, b) for a, b in zip(ok, again))


def test_a_pair_is_the_same_bytes_alone_and_in_any_batch(scored):
    from vbx_amd import metrics
    probes = ['three_overlapping', 'chain_257', 'random_7', 'entries_256']
    alone = {n: metrics.frame_counts([ALL[n]], device=0)[0] for n in probes}
    mixed = ['classes_over_cap', probes[2], 'both_empty', probes[0], 'ref_65', probes[3], 'random_3', probes[1]]
    batch = dict(zip(mixed, metrics.frame_counts([ALL[n] for n in mixed], device=0)))
    for n in probes:
        for rec in (batch[n], scored[n]):
            for k in ('ref_durs', 'sys_durs', 'inter', 'cm'):
                assert rec[k].tobytes() == alone[n][k].tobytes() and rec[k].shape == alone[n][k].shape, (n, k)
            assert rec['ref_classes'] == alone[n]['ref_classes'] and rec['sys_classes'] == alone[n]['sys_classes']


def test_other_steps_on_the_device():
    from vbx_amd import metrics
    pairs = [CRAFTED['product_edges'], CRAFTED['starts_after_zero'], RANDOM['random_5']]
    for step in (0.02, 0.003):
        for (ref, hyp), got in zip(pairs, metrics.frame_counts(pairs, step=step, device=0)):
            metrics_ref.assert_counts_equal(got, metrics_ref.counts(ref, hyp, step), f'step {step}')


def test_es2005a_row_on_the_device(es2005a, capsys):  # noqa: F811
    from vbx_amd import metrics
    assert metrics.main(['-r', REF_RTTM, '-s', es2005a, '--collar', '0.25', '--ignore_overlaps', '--device', '0']) == 0
    got = [l.rstrip() for l in capsys.readouterr().out.splitlines()]
    assert got == [l.rstrip() for l in open(os.path.join(GOLDEN, 'es2005a_dscore_table.txt')).read().splitlines()]
    dev = metrics.score_rttm(REF_RTTM, es2005a, 0.25, True, device=0)[0]['ES2005a']
    cpu = metrics.score_rttm(REF_RTTM, es2005a, 0.25, True, device=None)[0]['ES2005a']
    assert dev['cm'].shape == (15, 8)
    metrics_ref.assert_counts_equal(dev, cpu)
    assert all(dev[k] == cpu[k] for k in metrics.COLUMNS[1:])              # the same integers: the same bits
