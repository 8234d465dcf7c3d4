"""The device path of ``score.score_labels`` (vbx_labels_score.hpp: labels_turns / labels_edges in front of the three kernels of
vbx_rttm_score.hpp) against the exact referee ``tests/score_ref.py`` on the turns numpy's ``merge_adjacent_labels`` gives, against
the existing device route ``score_turns(device=0)`` on those turns, and ``vbx_amd.tune`` against ``vbx_amd.vbhmm`` point by point.

Kernel inputs are dyadic, the argument of tests/test_gpu_score.py: every time is a multiple of 2^-10 s below 2^12 s, so are the
collars, and the midpoint of two of them lies on 2^-11.  Every cell length, product and partial sum is then exact in float64 and
the device's numbers must EQUAL the referee's -- no tolerance.  Gaps are at least one grid step and the times of those cases
stay below 64 s, where isclose's tolerance (1e-8 + 1e-5 t < 6.5e-4) is below the step (9.8e-4): a gap there is a gap.  Shapes sit
at every pass boundary of the scans (kLabBlock) and at the constants of the cell kernels, one either side.
"""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import score_ref
import tune_util
from score_util import KEYS, assert_within_bound, rounding_bound

pytestmark = pytest.mark.gpu
Q = 2.0 ** -10
PROTOCOLS = {'full': (0.0, False), 'collar': (0.25, False), 'forgiving': (0.25, True)}


def constants():
    """kLabBlock, kRttmClsBlock, kRttmGroupCells, kRttmMaxSpk as the headers have them"""
    import re
    from vbx_amd import _capi, build
    lab = open(os.path.join(build.CSRC, 'vbx_labels_score.hpp')).read()
    rttm = open(os.path.join(build.CSRC, 'vbx_rttm_score.hpp')).read()
    c = {k: int(v) for k, v in re.findall(r'constexpr int (k\w+) = (\d+);', lab + rttm)}
    assert (c['kLabBlock'], c['kRttmClsBlock'], c['kRttmGroupCells'], c['kRttmMaxSpk']) == \
        (_capi.LABELS_BLOCK, _capi.RTTM_CLS_BLOCK, _capi.RTTM_GROUP_CELLS, _capi.RTTM_MAX_SPEAKERS)
    return c['kLabBlock'], c['kRttmClsBlock'], c['kRttmGroupCells'], c['kRttmMaxSpk']


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def segments(layout, T, seed=0, t0=1.0):
    """starts, ends on the grid: 'gaps' (disjoint), 'touching', 'overlap' (windows of 48 steps every 8), 'identical' (overlap,
    with every third window repeated twice more: three neighbours that share both times)"""
    rng = np.random.default_rng(seed)
    if layout in ('gaps', 'touching'):
        length = rng.integers(1, 12, T)
        gap = rng.integers(1, 9, T) if layout == 'gaps' else np.zeros(T, dtype=np.int64)
        s = np.cumsum(np.concatenate([[0], (length + gap)[:-1]]))
        e = s + length
    else:
        k = np.arange(T)
        if layout == 'identical':                                    # windows 3..5, 12..14, ... collapse onto their first
            k = np.array([i - i % 3 if i // 3 % 3 == 1 else i for i in range(T)])
        s = 8 * k
        e = s + 48
    assert e[-1] * Q + t0 < 64.0
    return t0 + s * Q, t0 + e * Q


def reference(seed, lo, hi, n_ref=3, n_turns=14):
    """n_turns dyadic reference turns of n_ref speakers over [lo - 1, hi + 1] (every speaker has one)"""
    rng = np.random.default_rng(seed)
    a, b = int((lo - 1.0) / Q), int((hi + 1.0) / Q)
    out = []
    for k in range(max(n_turns, n_ref)):
        s = int(rng.integers(a, b - 2))
        e = int(min(b, s + rng.integers(1, max(2, (b - a) // 4))))
        out.append((s * Q, e * Q, f'r{k % n_ref:02d}'))
    return out


def label_runs(T, cuts, S):
    """labels that change exactly at the segment indices in cuts, cycling through S values"""
    lab = np.zeros(T, dtype=np.int64)
    for c in cuts:
        if 0 < c < T:
            lab[c:] += 1
    return lab % S


def build_cases():
    """name -> (reference turns, starts, ends, labels)"""
    B, cls, group, maxspk = constants()
    cases = {}

    def add(name, layout, T, labels, seed, **kw):
        s, e = segments(layout, T, seed)
        cases[name] = (reference(seed + 1000, s[0], e[-1], **kw), s, e, np.asarray(labels))
    # T at every pass boundary of the scans: alternating labels give T turns and 2 T boundaries, so kernel A crosses its block at
    # T = B, 2 B and kernel B at T = B / 2, B; one label on touching segments gives one turn whatever T is
    for n, T in enumerate(sorted({1, 2, B // 2 - 1, B // 2, B // 2 + 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1})):
        add(f'alternate_T{T}', 'overlap', T, np.arange(T) % 2, 10 + n)
        add(f'equal_T{T}', 'touching', T, np.zeros(T, dtype=int), 40 + n)
    # runs that end on the scan block edge, one either side, in every layout
    T = 2 * B + 1
    for n, layout in enumerate(('gaps', 'touching', 'overlap', 'identical')):
        add(f'runs_{layout}', layout, T, label_runs(T, [B - 1, B, B + 1, 2 * B - 1, 2 * B], 3), 70 + n)
        rng = np.random.default_rng(80 + n)
        add(f'random_{layout}', layout, B + 1, np.repeat(rng.integers(0, 4, B + 1), rng.integers(1, 5, B + 1))[:B + 1], 80 + n)
    add('gaps_equal', 'gaps', B + 1, np.zeros(B + 1, dtype=int), 90)             # every gap cuts: B + 1 turns of one speaker
    # identical times: windows 3, 4, 5 share both times; labels 0 7 0 there give label 7 a turn WITHOUT duration, its only one
    lab = np.arange(30) % 2
    lab[3:6] = [0, 7, 0]
    add('zero_length_only', 'identical', 30, lab, 91)
    for n, S in enumerate((1, 2, 32, 33, maxspk, maxspk + 1)):
        T = max(2 * S + 3, 70)
        add(f'S{S}', 'overlap', T, np.arange(T) % S, 100 + n)
    add(f'nref{maxspk + 1}', 'overlap', 150, np.arange(150) % 3, 110, n_ref=maxspk + 1, n_turns=2 * maxspk + 2)
    add(f'nref{maxspk}', 'overlap', 150, np.arange(150) % 3, 111, n_ref=maxspk, n_turns=2 * maxspk)
    return cases


HOST_ROUTE = ('S65', 'nref65')           # more than 64 speakers a side: the numpy route (checked against kRttmMaxSpk below)


@pytest.fixture(scope='module')
def scored():
    """every case under every protocol: ONE score_labels call per protocol, and the existing device route on the numpy turns"""
    from vbx_amd import score
    cases = build_cases()
    names = list(cases)
    turns = {n: score.labels_turns(*cases[n][1:]) for n in names}
    new, old = {}, {}
    for proto, (collar, ignore) in PROTOCOLS.items():
        got = score.score_labels([(cases[n][0], cases[n][1], cases[n][2], [cases[n][3]]) for n in names], collar, ignore, device=0)
        new[proto] = {n: g[0] for n, g in zip(names, got)}
        old[proto] = dict(zip(names, score.score_turns([(cases[n][0], turns[n]) for n in names], collar, ignore, device=0)))
    return cases, turns, new, old


def case_names():
    return list(build_cases())


def assert_equal_to_referee(got, ref, hyp, collar, ignore):
    exact = score_ref.score_exact(ref, hyp, Fraction(collar), ignore)
    for key in KEYS:
        assert Fraction(got[key]) == exact[key], (key, got[key], float(exact[key]))
    names = {(r, s): got['C'][i, j] for i, r in enumerate(got['ref_speakers']) for j, s in enumerate(got['sys_speakers'])}
    assert set(names) == set(exact['C'])
    wrong = [(k, names[k], float(v)) for k, v in exact['C'].items() if Fraction(float(names[k])) != v]
    assert not wrong, wrong[:5]
    return exact


def assert_same_record(a, b):
    for key in KEYS + ('der',):
        assert np.float64(a[key]).tobytes() == np.float64(b[key]).tobytes(), key
    assert a['ref_speakers'] == b['ref_speakers'] and a['sys_speakers'] == b['sys_speakers'] and a['mapping'] == b['mapping']
    assert a['C'].shape == b['C'].shape and a['C'].tobytes() == b['C'].tobytes()


@pytest.mark.parametrize('proto', list(PROTOCOLS))
@pytest.mark.parametrize('name', case_names())
def test_label_sequences_equal_the_referee_and_the_turn_route_bit_for_bit(name, proto, scored):
    cases, turns, new, old = scored
    collar, ignore = PROTOCOLS[proto]
    ref, starts, ends, labels = cases[name]
    got = new[proto][name]
    _, _, _, maxspk = constants()
    assert HOST_ROUTE == (f'S{maxspk + 1}', f'nref{maxspk + 1}')
    if name in HOST_ROUTE:                                            # numpy sums: within the rounding bound
        exact = score_ref.score_exact(ref, turns[name], Fraction(collar), ignore)
        assert_within_bound(got, exact, name)
        assert max(len(got['ref_speakers']), len(got['sys_speakers'])) == maxspk + 1
    else:
        exact = assert_equal_to_referee(got, ref, turns[name], collar, ignore)
        assert_same_record(got, old[proto][name])
    if proto == 'full':
        assert exact['ref_time'] > 0
    if name == 'zero_length_only':
        assert 7 not in got['sys_speakers'] and got['sys_speakers'] == [0, 1]
    elif name.startswith('S'):
        assert len(got['sys_speakers']) == int(name[1:])


# ---- the entry point itself: what came back about turns and edges --------------------------------------------------------------
def raw(recs, hyps, collar=0.0, ignore=False):
    """vbx_labels_score on recs = [(reference turns, starts, ends)] and hyps = [(recording, labels, n_sys)]
    -> ([bytes of (tot, C) per hypothesis], info [n_hyp][4], [(tot, C)])"""
    from vbx_amd import _capi, score
    refs = [score._LabelsRef(r, s, e, collar) for r, s, e in recs]
    assert all(r.ok for r in refs)
    flat, info = _capi.labels_score(
        _capi.default_context(0), [(r.starts.size, r.rb.size, len(r.ref_names), r.edges.size) for r in refs],
        np.concatenate([a for r in refs for a in (r.starts, r.ends)]), np.concatenate([np.stack([r.rb, r.re], axis=1) for r in refs]),
        np.concatenate([r.rs for r in refs]), np.concatenate([r.edges for r in refs]), [(h[0], h[2]) for h in hyps],
        np.concatenate([np.asarray(h[1], dtype=np.int32) for h in hyps]), collar, ignore)
    out, parts, off = [], [], 0
    for rec, _lab, n_sys in hyps:
        n = 4 + len(refs[rec].ref_names) * n_sys
        out.append(flat[off:off + n].tobytes())
        parts.append((flat[off:off + 4].copy(), flat[off + 4:off + n].reshape(-1, n_sys).copy()))
        off += n
    return out, info, parts


def test_counts_of_turns_and_edges_and_the_zero_column():
    """the turns and the distinct edges the device made are as many as numpy's, and a label that never occurs is a zero column"""
    from vbx_amd import score
    cases = build_cases()
    names = [n for n in cases if n not in HOST_ROUTE]
    for collar in (0.0, 0.25):
        recs = [cases[n][:3] for n in names]
        hyps = [(k, cases[n][3], min(int(cases[n][3].max()) + 2, 64)) for k, n in enumerate(names)]   # one label more than occur
        _, info, parts = raw(recs, hyps, collar)
        all_turns = [score.labels_turns(*cases[n][1:]) for n in names]
        pairs = [score._Pair(cases[n][0], turns, collar) for n, turns in zip(names, all_turns)]
        via_turns = score._device_totals(pairs, collar, False, 0)
        for n, inf, (tot, C), hyp, turns, pair, (tot_old, C_old) in zip(names, info, parts, hyps, all_turns, pairs, via_turns):
            assert inf[0] == len(turns), n
            assert inf[1] == pair.edges.size, n
            mask = (int(inf[3]) & 0xffffffff) << 32 | (int(inf[2]) & 0xffffffff)
            assert [s for s in range(64) if mask >> s & 1] == sorted(pair.sys_names), n
            assert C.shape[1] == hyp[2] and tot.tobytes() == tot_old.tobytes(), n
            for s in range(hyp[2]):                                   # column s IS label s; a label without a turn: zeros
                want = C_old[:, pair.sys_names.index(s)] if s in pair.sys_names else np.zeros(C.shape[0])
                assert C[:, s].tobytes() == want.tobytes(), (n, s)
            assert n == 'S64' or not C[:, hyp[2] - 1].any()


def isclose_case(t, steps_below_tolerance):
    """two segments of one label round t whose gap is the largest grid multiple below isclose's tolerance at the second start,
    shifted by so many steps; -> starts, ends, gap"""
    e0 = np.floor(t / Q) * Q
    tol = 1e-8 + 1e-5 * e0
    g = (np.floor(tol / Q) + steps_below_tolerance) * Q
    return np.array([e0 - 1.0, e0 + g]), np.array([e0, e0 + g + 1.0]), g


def test_isclose_at_both_scales():
    from vbx_amd import score
    cases = []
    # near t = 3000 s the tolerance is 0.03 s, about 30 grid steps: the largest multiple of the step not above it merges ...
    s, e, g = isclose_case(3000.0, 0)
    assert g > 0.029 and np.isclose(e[0], s[1]) and g <= 1e-8 + 1e-5 * s[1]
    cases.append((s, e, 1))
    s, e, g = isclose_case(3000.0, -1)                                # ... and so does one step less
    assert np.isclose(e[0], s[1])
    cases.append((s, e, 1))
    s, e, g = isclose_case(3000.0, 2)                                 # ... one step above the tolerance does not
    assert g > 1e-8 + 1e-5 * s[1] and not np.isclose(e[0], s[1]) and g < 0.033
    cases.append((s, e, 2))
    s, e, g = isclose_case(3000.0, 1)                                 # the first multiple above it: not close
    assert not np.isclose(e[0], s[1])
    cases.append((s, e, 2))
    # near t = 0 the tolerance is 1e-8: a gap of 0 merges, a gap of one step does not
    cases.append((np.array([0.0, 1.0]), np.array([1.0, 2.0]), 1))
    cases.append((np.array([0.0, 1.0 + Q]), np.array([1.0, 2.0]), 2))
    cases.append((np.array([Q, 2 * Q]), np.array([2 * Q, 3 * Q]), 1))
    cases.append((np.array([0.0, 2 * Q]), np.array([Q, 3 * Q]), 2))
    items = [([(s[0] - 0.5, e[1] + 0.5, 'x')], s, e, [[3, 3]]) for s, e, _ in cases]
    recs = [(it[0], it[1], it[2]) for it in items]
    _, info, _ = raw(recs, [(k, [0, 0], 1) for k in range(len(cases))])
    for collar, ignore in PROTOCOLS.values():
        got = score.score_labels(items, collar, ignore, device=0)
        for k, (s, e, n_turns) in enumerate(cases):
            turns = score.labels_turns(s, e, [3, 3])
            assert len(turns) == n_turns == info[k][0], k
            exact = assert_equal_to_referee(got[k][0], items[k][0], turns, collar, ignore)
            if collar == 0.0:                       # the reference covers everything and 0.5 s either side: the rest of the miss IS the gap
                assert got[k][0]['miss'] == 1.0 + (0.0 if n_turns == 1 else s[1] - e[0]) and exact['fa'] == 0


def test_edge_merging_and_cell_counts():
    from vbx_amd import score
    B, cls, group, _ = constants()
    ref = [(8.0, 12.0, 'x'), (10.0, 16.0, 'y')]
    cases = {
        'on_a_reference_boundary': ([9.0, 10.0, 11.0], [10.0, 11.0, 12.0], [0, 1, 0]),           # 10, 12: begins and ends of the reference
        'on_a_collar_end': ([9.0, 10.25, 11.0], [10.25, 11.0, 15.75], [0, 1, 0]),                # 10 + 0.25, 16 - 0.25
        'outside_both_sides': ([2.0, 9.0, 17.0], [9.0, 17.0, 20.0], [0, 1, 0]),
        'outside_left_inside_right': ([2.0, 9.0], [9.0, 13.0], [0, 1]),
        'first_and_last_are_lo_and_hi': ([8.0, 11.0], [11.0, 16.0], [0, 1]),
        'all_boundaries_are_reference_edges': ([8.0, 10.0, 12.0], [10.0, 12.0, 16.0], [0, 1, 0]),
    }
    items = [(ref, np.array(s), np.array(e), [np.array(l)]) for s, e, l in cases.values()]
    for collar, ignore in PROTOCOLS.values():
        got = score.score_labels(items, collar, ignore, device=0)
        old = score.score_turns([(ref, score.labels_turns(it[1], it[2], it[3][0])) for it in items], collar, ignore, device=0)
        _, info, _ = raw([it[:3] for it in items], [(k, it[3][0], 2) for k, it in enumerate(items)], collar, ignore)
        for k, name in enumerate(cases):
            turns = score.labels_turns(items[k][1], items[k][2], items[k][3][0])
            assert_equal_to_referee(got[k][0], ref, turns, collar, ignore)
            assert_same_record(got[k][0], old[k])
            assert info[k][1] == score._Pair(ref, turns, collar).edges.size, name
    assert info[5][1] == score._LabelsRef(ref, items[5][1], items[5][2], 0.25).edges.size           # nothing kept
    # cell counts either side of kRttmClsBlock and kRttmGroupCells: one reference turn over T touching turns inside it cuts
    # T + 2 cells (collar 0)
    counts = [cls - 1, cls, cls + 1, group - 1, group, group + 1]
    items = []
    for n, cells in enumerate(counts):
        s, e = segments('touching', cells - 2, 300 + n, t0=2.0)
        items.append(([(1.0, e[-1] + 1.0, 'x')], s, e, [np.arange(cells - 2) % 2]))
    got = score.score_labels(items, 0.0, False, device=0)
    _, info, _ = raw([it[:3] for it in items], [(k, it[3][0], 2) for k, it in enumerate(items)])
    for k, cells in enumerate(counts):
        assert info[k][1] - 1 == cells
        exact = assert_equal_to_referee(got[k][0], items[k][0], score.labels_turns(*items[k][1:3], items[k][3][0]), 0.0, False)
        assert exact['n_cells'] == cells


def test_a_hypothesis_has_the_same_bytes_wherever_it_stands_in_a_batch():
    B, _, group, _ = constants()
    rng = np.random.default_rng(5)
    recs = []
    for k, (layout, T) in enumerate([('overlap', 2 * B + 77), ('gaps', 40), ('touching', B), ('identical', 3 * B), ('overlap', 1)]):
        s, e = segments(layout, T, 400 + k)
        # millisecond decimals on the reference: sums that round, so that an order that depended on the batch would show
        ref = [(round(b + 0.0007, 4), round(x + 0.0013, 4), spk) for b, x, spk in reference(500 + k, s[0], e[-1], 4, 30)]
        recs.append((ref, s, e))

    def random_hyp(r):
        T = recs[r][1].size
        S = int(rng.integers(1, 9))
        return (r, np.repeat(rng.integers(0, S, T), rng.integers(1, 7, T))[:T], S)
    probe = (0, np.repeat(rng.integers(0, 5, 2 * B + 77), rng.integers(1, 3, 2 * B + 77))[:2 * B + 77], 5)
    others = [random_hyp(k % len(recs)) for k in range(40)]
    collar, ignore = 0.25, False
    alone, info, parts = raw(recs[:1], [probe], collar, ignore)
    assert parts[0][0][0] > 0 and info[0][0] > B                     # more turns than one pass of the scan
    assert raw(recs, [probe] + others, collar, ignore)[0][0] == alone[0]
    assert raw(recs, others + [probe], collar, ignore)[0][40] == alone[0]
    assert raw(recs, others[:20] + [probe] + others[20:], collar, ignore)[0][20] == alone[0]
    same_rec = [probe if k == 7 else random_hyp(0) for k in range(16)]                          # 16 hypotheses of one recording
    assert raw(recs[:1], same_rec, collar, ignore)[0][7] == alone[0]
    assert raw(recs[:1], [probe, probe], collar, ignore)[0] == [alone[0], alone[0]] and raw(recs[:1], [probe], collar, ignore)[0] == alone


def test_decimal_inputs_within_the_rounding_bound_of_both_routes():
    """millisecond decimals everywhere: the sums round, the two device routes cut the same cells and add them in the same order"""
    from vbx_amd import score
    import test_tune_host as host
    B, _, _, _ = constants()
    items = [host.sliding_windows(seed, T) for seed, T in ((21, 1), (22, B + 3), (23, 2 * B + 1), (24, 700))]
    for collar, ignore in PROTOCOLS.values():
        got = score.score_labels([(it[0], it[1], it[2], [it[3], (it[3] + 1) % 3]) for it in items], collar, ignore, device=0)
        for k, it in enumerate(items):
            for j, labels in enumerate((it[3], (it[3] + 1) % 3)):
                turns = score.labels_turns(it[1], it[2], labels)
                exact = score_ref.score_exact([(Fraction(str(b)), Fraction(str(e)), s) for b, e, s in it[0]],
                                              [(Fraction(b), Fraction(e), s) for b, e, s in turns], Fraction(str(collar)), ignore)
                assert_within_bound(got[k][j], exact, f'item {k} hypothesis {j}')
                via_turns = score.score_turns([(it[0], turns)], collar, ignore, device=0)[0]
                bound = rounding_bound(exact)
                assert all(abs(via_turns[key] - got[k][j][key]) <= bound for key in KEYS)
                assert_same_record(got[k][j], via_turns)              # (in fact the same cells in the same order: the same bytes)


def test_entry_point_refuses_bad_arguments():
    from vbx_amd import _capi
    ctx = _capi.default_context(0)
    rec, seg, turns, spk, edges = [[2, 1, 1, 2]], [0.0, 1.0, 1.0, 2.0], [[0.0, 2.0]], [0], [0.0, 2.0]

    def call(rec=rec, seg=seg, turns=turns, spk=spk, edges=edges, hyp=((0, 2),), labels=(0, 1), collar=0.0):
        return _capi.labels_score(ctx, rec, seg, turns, spk, edges, list(hyp), list(labels), collar, False)
    ok, info = call()
    assert ok.tolist() == [2.0, 0.0, 0.0, 2.0, 1.0, 1.0] and info.tolist() == [[2, 3, 3, 0]]
    with pytest.raises(_capi.VbxError, match='label 2 of segment 1 outside'):
        call(labels=(0, 2))
    with pytest.raises(_capi.VbxError, match='label -1 of segment 0 outside'):
        call(labels=(-1, 0))
    with pytest.raises(_capi.VbxError, match='times decrease at segment 1'):
        call(seg=[1.0, 0.5, 2.0, 2.5], edges=[0.0, 2.5])
    with pytest.raises(_capi.VbxError, match='times decrease at segment 1'):
        call(seg=[0.0, 0.5, 2.0, 1.5])
    with pytest.raises(_capi.VbxError, match='no positive finite duration'):
        call(seg=[0.0, 1.0, 1.0, 1.0])
    with pytest.raises(_capi.VbxError, match='no positive finite duration'):
        call(seg=[0.0, 1.0, 1.0, float('nan')])
    with pytest.raises(_capi.VbxError, match='not sorted and distinct'):
        call(edges=[2.0, 0.0])
    with pytest.raises(_capi.VbxError, match='do not span'):
        call(edges=[0.5, 2.0])
    with pytest.raises(_capi.VbxError, match='speaker 1 of reference turn 0'):
        call(spk=[1])
    with pytest.raises(_capi.VbxError, match='at most 64'):
        call(hyp=((0, 65),))
    with pytest.raises(_capi.VbxError, match='at most 64'):
        call(rec=[[2, 1, 65, 2]])

    def direct(rec=rec, seg=seg, turns=turns, spk=spk, edges=edges, hyp=((0, 2),), labels=(0, 1), out=np.zeros(6)):
        f64 = lambda a: None if a is None else np.array(a, dtype=np.float64)
        i32 = lambda a: None if a is None else np.array(a, dtype=np.int32)
        arrays = [i32(rec), f64(seg), f64(turns), i32(spk), f64(edges), i32(hyp), i32(labels)]      # (alive during the call)
        ptr = [_capi._ptr(a) for a in arrays]
        ctx.check(ctx._lib.vbx_labels_score(ctx._h, 1, *ptr[:5], 1, *ptr[5:], 0.0, 0, _capi._ptr(out), None), 'vbx_labels_score')
        return out
    assert direct().tolist() == ok.tolist()
    with pytest.raises(_capi.VbxError, match='names recording 1 of 1'):
        direct(hyp=((1, 2),))
    with pytest.raises(_capi.VbxError, match='negative or oversized count'):
        direct(rec=[[2, -1, 1, 2]])
    with pytest.raises(_capi.VbxError, match='negative or oversized count'):
        direct(rec=[[-2, 1, 1, 2]])
    with pytest.raises(_capi.VbxError, match='negative or oversized count'):
        direct(hyp=((0, -1),))
    for null in ('seg', 'edges', 'hyp', 'labels', 'out'):                                 # NULLs
        with pytest.raises(_capi.VbxError, match='bad argument'):
            direct(**{null: None})
    with pytest.raises(_capi.VbxError, match='NULL argument'):
        direct(turns=None)
    with pytest.raises(_capi.VbxError, match='collar'):
        call(collar=-1.0)
    again, info2 = call()                                             # and the context still works
    assert again.tolist() == ok.tolist() and info2.tolist() == info.tolist()


# ---- the driver -------------------------------------------------------------------------------------------------------------
GRID = dict(Fa=[0.2, 0.4], Fb=[11.0, 17.0], loopP=[0.9, 0.99])


def grid_argv():
    return [a for k, vs in GRID.items() for a in ['--' + k] + [str(v) for v in vs]]


@pytest.fixture(scope='module')
def tuned(tmp_path_factory):
    """the library call, the program in a fresh child process, and the driver run at every grid point"""
    import contextlib
    import io
    from vbx_amd import score, tune, vbhmm
    tmp = tmp_path_factory.mktemp('tune')
    p = tune_util.make_dev_set(tmp, 3, 120, seed=3)
    argv = tune_util.data_argv(p) + grid_argv()
    lib_args = tune.build_parser().parse_args(argv + ['--best-rttm-dir', str(tmp / 'best_lib'), '--out-json', str(tmp / 'lib.json')])
    result = tune.tune(lib_args, log=lambda *a: None)
    child = subprocess.run([sys.executable, '-m', 'vbx_amd.tune'] + argv + ['--best-rttm-dir', str(tmp / 'best_cli'), '--out-json', str(tmp / 'cli.json')],
                           env=dict(os.environ, PYTHONPATH=tune_util.REPO), cwd=tune_util.REPO, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    runs = []
    for gi, (Fa, Fb, loopP) in enumerate(result['grid']):
        out = str(tmp / f'vbhmm{gi}')
        vargs = vbhmm.build_parser().parse_args(['--init', 'AHC+VB', '--out-rttm-dir', out] + tune_util.data_argv(p)
                                                + ['--Fa', str(Fa), '--Fb', str(Fb), '--loopP', str(loopP)])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            state, _ = vbhmm.diarize(vargs, log=lambda *a: None)
        written, overall = score.score_written(out, p['names'], p['ref'], 0.25, False, 0)
        runs.append(dict(out=out, state=state, table=buf.getvalue(), written=written, overall=overall))
    return p, tmp, result, child.stdout, runs


def test_tune_equals_the_driver_at_every_grid_point(tuned):
    from vbx_amd import score, tune
    p, tmp, result, printed, runs = tuned
    assert result['grid'] == tune.grid_points(**GRID) and len(runs) == 8 and result['names'] == p['names']
    ref = {n: score.read_turns(os.path.join(p['ref'], n + '.rttm'))[n] for n in p['names']}
    from vbx_amd.kaldi_formats import read_xvector_timing_dict
    segs = read_xvector_timing_dict(p['seg'])
    items = [(ref[n], *segs[n][1].T, [result['labels'][g][k] for g in range(8)]) for k, n in enumerate(p['names'])]
    host = score.score_labels(items, 0.25, False, device=None)
    for g, run in enumerate(runs):
        n_turns = 0
        for k, n in enumerate(p['names']):
            assert np.array_equal(result['labels'][g][k], run['state'][n]['labels1st']), (g, n)          # integer equality
            rec, numpy_rec = result['records'][g][k], host[k][g]
            # both are sums in float64 of the SAME float inputs: each within the rounding bound of the exact sums of those
            exact = score_ref.score_exact([(Fraction(b), Fraction(e), s) for b, e, s in ref[n]],
                                          [(Fraction(b), Fraction(e), s) for b, e, s in score.labels_turns(*items[k][1:3], items[k][3][g])],
                                          Fraction(1, 4), False)
            assert_within_bound(rec, exact, f'device, point {g} {n}')
            assert_within_bound(numpy_rec, exact, f'numpy, point {g} {n}')
            assert all(abs(rec[key] - numpy_rec[key]) <= 2 * rounding_bound(exact) for key in KEYS), (g, n)
            assert rec['sys_speakers'] == numpy_rec['sys_speakers']
            n_turns += len(open(os.path.join(run['out'], n + '.rttm')).read().splitlines())
        pooled = result['pooled'][g]
        assert pooled == score._pool(result['records'][g]) and pooled['ref_time'] > 0
        assert run['table'] == score.format_table(run['written'], run['overall']) + '\n'              # what vbhmm --ref-rttm-dir printed
        bound = 100.0 * 3 * 2 * n_turns * 1e-6 / run['overall']['ref_time']
        print(f'point {g}: tune {pooled["der"]!r} text {run["overall"]["der"]!r} bound {bound:.3e}')
        assert abs(pooled['der'] - run['overall']['der']) <= bound
    best = result['best']
    assert best == tune.best_point(result['pooled'])
    want = {f: open(os.path.join(runs[best]['out'], f), 'rb').read() for f in sorted(os.listdir(runs[best]['out']))}
    for d in ('best_lib', 'best_cli'):
        assert {f: open(tmp / d / f, 'rb').read() for f in sorted(os.listdir(tmp / d))} == want and len(want) == 3
    # the program: the table of the library call, and the same JSON but for the timings
    assert printed == tune.format_table(result) + '\n'
    lib, cli = json.load(open(tmp / 'lib.json')), json.load(open(tmp / 'cli.json'))
    assert lib['points'] == cli['points'] and lib['best'] == cli['best'] and lib['best']['index'] == best and len(lib['points']) == 8
