"""``vbx_amd.score`` without a GPU: the numpy path (``device=None``) against the one published figure there is, against hand
cases worked out below, and against the exact referee ``tests/score_ref.py``; the command line, the table and the refusals;
the new entry point in the header and the ABI list.

The anchor: the reference's README gives DER 7.06 for its example recording ES2005a under ``--collar 0.25
--ignore_overlaps`` (run_example.sh:40).  ``tests/golden/es2005a_ref.rttm`` is that recipe's reference RTTM,
``es2005a.npz: rttm_committed`` the system RTTM the reference ships for it.
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import score_ref
from score_util import KEYS, assert_within_bound, random_pair

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
REF_RTTM = os.path.join(GOLDEN, 'es2005a_ref.rttm')


# ---- the ES2005a anchor -------------------------------------------------------------------------------------------------
def es2005a_system_text():
    """the shipped system RTTM as write_rttm writes it (six decimals; the stored doubles have at most two)"""
    import io
    from vbx_amd.kaldi_formats import write_rttm
    g = np.load(os.path.join(GOLDEN, 'es2005a.npz'))['rttm_committed']
    fp = io.StringIO()
    write_rttm(fp, 'ES2005a', g[:, 2].astype(int) - 1, g[:, 0], g[:, 0] + g[:, 1])
    return fp.getvalue()


@pytest.fixture(scope='module')
def es2005a(tmp_path_factory):
    path = tmp_path_factory.mktemp('es2005a') / 'sys.rttm'
    path.write_text(es2005a_system_text())
    return str(path)


def test_es2005a_scores_the_published_der(es2005a, capsys):
    from vbx_amd import score
    assert score.main(['-r', REF_RTTM, '-s', es2005a, '--collar', '0.25', '--ignore_overlaps']) == 0
    out = capsys.readouterr().out
    rows = [l.split() for l in out.splitlines()]
    assert rows[0] == ['File', 'DER', 'Miss', 'FA', 'Conf']
    row = next(r for r in rows if r[0] == 'ES2005a')
    assert row[1] == '7.06', out                                 # README.md of the reference: ES2005a 7.06
    assert rows[-1][:3] == ['***', 'OVERALL', '***'] and rows[-1][3] == '7.06'


# protocol -> (DER, miss, fa, confusion, scored reference time) as DESIGN section 17 gives them (worked out with a throwaway script before any of this was written)
ES2005A_TABLE = {
    'forgiving': (dict(collar=0.25, ignore_overlaps=True), (7.0634, 0.0, 0.0, 12.738, 180.337)),
    'fair': (dict(collar=0.25, ignore_overlaps=False), (17.2748, 24.521, 0.0, 14.834, 227.818)),
    'full': (dict(collar=0.0, ignore_overlaps=False), (26.2792, 62.168, 0.101, 25.077, 332.377)),
}


@pytest.mark.parametrize('protocol', list(ES2005A_TABLE))
def test_es2005a_protocols_equal_the_referee(protocol, es2005a):
    from vbx_amd import score
    kw, (der, miss, fa, conf, ref_time) = ES2005A_TABLE[protocol]
    records, overall = score.score_rttm(REF_RTTM, es2005a, **kw)
    got = records['ES2005a']
    exact = score_ref.score_exact(score_ref.read_rttm_exact(REF_RTTM)['ES2005a'], score_ref.read_rttm_exact(es2005a)['ES2005a'],
                                  Fraction(str(kw['collar'])), kw['ignore_overlaps'])
    assert_within_bound(got, exact, protocol)
    # the referee's values are the table's, to the digits the table has
    assert round(float(exact['der']), 4) == der and round(float(exact['miss']), 3) == miss and round(float(exact['fa']), 3) == fa
    assert round(float(exact['confusion']), 3) == conf and round(float(exact['ref_time']), 3) == ref_time
    assert overall['der'] == got['der']                            # one recording: OVERALL is its row


# ---- hand cases ---------------------------------------------------------------------------------------------------------
def one(ref, hyp, **kw):
    from vbx_amd import score
    got = score.score_turns([(ref, hyp)], **kw)[0]
    exact = score_ref.score_exact(ref, hyp, Fraction(kw.get('collar', 0)), kw.get('ignore_overlaps', False))
    assert_within_bound(got, exact)
    return got


def test_identical_turns_score_zero():
    turns = [(0.0, 10.0, 'A'), (10.0, 20.0, 'B')]
    got = one(turns, turns)
    assert got['der'] == 0.0 and got['ref_time'] == 20.0 and got['mapping'] == {'A': 'A', 'B': 'B'}


def test_swapped_labels_score_zero_through_the_mapping():
    got = one([(0.0, 10.0, 'A'), (10.0, 20.0, 'B')], [(0.0, 10.0, 'y'), (10.0, 20.0, 'x')])
    assert got['der'] == 0.0 and got['mapping'] == {'A': 'y', 'B': 'x'} and got['confusion'] == 0.0


def test_a_missed_speaker():
    # B's 5 s are nobody's: miss 5 of 15 s of reference speech
    got = one([(0.0, 10.0, 'A'), (10.0, 15.0, 'B')], [(0.0, 10.0, 1)])
    assert (got['miss'], got['fa'], got['confusion'], got['ref_time']) == (5.0, 0.0, 0.0, 15.0)
    assert got['der'] == 100.0 * 5.0 / 15.0 and got['mapping'] == {'A': 1}


def test_a_system_turn_outside_the_reference_extent_is_false_alarm():
    # the extent runs to the system's last end, 14: [12, 14] is scored, nobody speaks there in the reference
    got = one([(0.0, 10.0, 'A')], [(0.0, 10.0, 1), (12.0, 14.0, 1)])
    assert (got['miss'], got['fa'], got['confusion'], got['ref_time']) == (0.0, 2.0, 0.0, 10.0) and got['der'] == 20.0


def test_overlapping_reference_speakers_against_one_system_speaker():
    ref, hyp = [(0.0, 10.0, 'A'), (5.0, 10.0, 'B')], [(0.0, 10.0, 1)]
    # [0, 5]: A against 1.  [5, 10]: two reference speakers, one system speaker: 5 s of miss; both = 10, C[A][1] = 10,
    # C[B][1] = 5: the mapping takes A, confusion 0.  DER = 5 / 15.
    got = one(ref, hyp)
    assert (got['miss'], got['fa'], got['confusion'], got['ref_time']) == (5.0, 0.0, 0.0, 15.0)
    assert got['C'].tolist() == [[10.0], [5.0]] and got['der'] == 100.0 * 5.0 / 15.0
    # overlapped reference speech not scored: only [0, 5] is left
    got = one(ref, hyp, ignore_overlaps=True)
    assert (got['miss'], got['ref_time'], got['der']) == (0.0, 5.0, 0.0) and got['C'].tolist() == [[5.0], [0.0]]


def test_a_collar_swallows_a_short_turn():
    # B speaks [10, 10.5] between two turns of A; the system hears one speaker throughout
    ref, hyp = [(0.0, 10.0, 'A'), (10.0, 10.5, 'B'), (10.5, 20.0, 'A')], [(0.0, 20.0, 1)]
    got = one(ref, hyp)                                          # no collar: B's half second is confusion, 0.5 / 20
    assert (got['confusion'], got['ref_time'], got['der']) == (0.5, 20.0, 2.5)
    # collar 0.25: not scored (-0.25, 0.25), (9.75, 10.25), (10.25, 10.75), (19.75, 20.25) -- all of B's turn; the cell edge
    # 10.25 itself has no length.  Scored: [0.25, 9.75] and [10.75, 19.75], 9.5 + 9 s of A against 1
    got = one(ref, hyp, collar=0.25)
    assert (got['miss'], got['fa'], got['confusion'], got['ref_time'], got['der']) == (0.0, 0.0, 0.0, 18.5, 0.0)
    assert got['C'].tolist() == [[18.5], [0.0]]


def test_touching_turns_of_one_speaker():
    from vbx_amd import score
    ref, hyp = [(0.0, 5.0, 'A'), (5.0, 10.0, 'A'), (12.0, 13.0, 'A'), (12.5, 14.0, 'A'), (20.0, 20.0, 'A')], [(0.0, 14.0, 1)]
    # merged: touching and overlapping turns become one, the turn of no duration goes
    assert score.merge_turns(ref) == [(0.0, 10.0, 'A'), (12.0, 14.0, 'A')]
    assert score.merge_turns(ref, touching=False) == [(0.0, 5.0, 'A'), (5.0, 10.0, 'A'), (12.0, 14.0, 'A')]
    # without a collar the scorer cannot tell: 12 s of A, 2 s of false alarm in the gap
    got, merged = one(ref, hyp), one(score.merge_turns(ref), hyp)
    assert (got['ref_time'], got['fa'], got['der']) == (12.0, 2.0, 100.0 * 2.0 / 12.0)
    assert all(got[k] == merged[k] for k in KEYS + ('der',))
    # with one, the boundary at 5 keeps its zone (dscore merges only turns that overlap: what ES2005a's 7.06 rests on):
    # scored reference time 12 - 0.25 - 0.5 - 0.25 - 0.25 - 0.25 = 10.5 against 11 for the merged turns
    assert one(ref, hyp, collar=0.25)['ref_time'] == 10.5 and one(score.merge_turns(ref), hyp, collar=0.25)['ref_time'] == 11.0


# ---- the host path against the referee ------------------------------------------------------------------------------------
@pytest.mark.parametrize('collar, ignore_overlaps', [(0.0, False), (0.25, False), (0.25, True), (0.1, True)])
@pytest.mark.parametrize('seed, n_ref, n_sys, n_turns', [(1, 2, 2, 8), (2, 4, 3, 40), (3, 3, 6, 25), (4, 1, 1, 5)])
def test_host_path_against_the_referee(seed, n_ref, n_sys, n_turns, collar, ignore_overlaps):
    from vbx_amd import score
    (ref, ref_x), (hyp, hyp_x) = random_pair(seed, n_ref, n_sys, n_turns)
    got = score.score_turns([(ref, hyp)], collar=collar, ignore_overlaps=ignore_overlaps)[0]
    exact = score_ref.score_exact(ref_x, hyp_x, Fraction(str(collar)), ignore_overlaps)
    assert exact['n_cells'] > n_turns and exact['ref_time'] > 0
    assert_within_bound(got, exact, f'seed {seed}')


def test_more_than_64_speakers_run_on_the_host_path_whatever_the_device():
    """70 reference speakers: the record comes from the numpy path even with a device named -- no GPU is touched here."""
    from vbx_amd import score
    ref = [(float(i), i + 1.5, f'r{i:02d}') for i in range(70)]
    hyp = [(float(i), i + 1.0, f's{i % 3}') for i in range(70)]
    a = score.score_turns([(ref, hyp)], collar=0.25, device=None)[0]
    b = score.score_turns([(ref, hyp)], collar=0.25, device=0)[0]
    assert len(a['ref_speakers']) == 70 and all(a[k] == b[k] for k in KEYS + ('der',)) and np.array_equal(a['C'], b['C'])
    assert_within_bound(a, score_ref.score_exact(ref, hyp, Fraction('0.25')))


# ---- the command line ---------------------------------------------------------------------------------------------------
def rttm_text(rec, turns):
    return ''.join(f'SPEAKER {rec} 1 {b:.3f} {e - b:.3f} <NA> <NA> {s} <NA> <NA>\n' for b, e, s in turns)


@pytest.fixture()
def corpus(tmp_path):
    """recA: 100 s, 10 s missed.  recB: 10 s, 5 s confused.  recC: in the reference only.  recD: reference turns of no duration."""
    ref = {'recA': [(0.0, 100.0, 'A')], 'recB': [(0.0, 5.0, 'A'), (5.0, 10.0, 'B')], 'recC': [(0.0, 4.0, 'A')],
           'recD': [(1.0, 1.0, 'A')]}
    hyp = {'recA': [(0.0, 90.0, 1)], 'recB': [(0.0, 10.0, 1)], 'recD': [(0.0, 0.0, 1)]}
    (tmp_path / 'ref.rttm').write_text(''.join(rttm_text(k, v) for k, v in ref.items()))
    (tmp_path / 'sysAB.rttm').write_text(''.join(rttm_text(k, hyp[k]) for k in ('recA', 'recB')))
    (tmp_path / 'sysD.rttm').write_text(rttm_text('recD', hyp['recD']))
    return tmp_path


def test_table_and_pooled_overall_row(corpus, capsys):
    from vbx_amd import score
    argv = ['-r', str(corpus / 'ref.rttm'), '-s', str(corpus / 'sysAB.rttm'), str(corpus / 'sysD.rttm')]
    assert score.main(argv) == 0
    rows = {tuple(l.split()[:-4]): l.split()[-4:] for l in capsys.readouterr().out.splitlines() if not l.startswith('-')}
    assert rows[('File',)] == ['DER', 'Miss', 'FA', 'Conf']
    assert rows[('recA',)] == ['10.00', '10.00', '0.00', '0.00']
    assert rows[('recB',)] == ['50.00', '0.00', '0.00', '50.00']
    assert rows[('recC',)] == ['100.00', '100.00', '0.00', '0.00']          # no system turn: all miss
    assert rows[('recD',)] == ['nan'] * 4                                   # no scored reference time
    # pooled: (10 + 5 + 4) / (100 + 10 + 4) = 16.67 %, not the mean 53.33 of the three rates; recD adds nothing
    assert rows[('***', 'OVERALL', '***')] == ['16.67', '12.28', '0.00', '4.39']
    records, overall = score.score_rttm([str(corpus / 'ref.rttm')], [str(corpus / 'sysAB.rttm'), str(corpus / 'sysD.rttm')])
    assert list(records) == ['recA', 'recB', 'recC', 'recD'] and np.isnan(records['recD']['der'])
    assert (overall['miss'], overall['fa'], overall['confusion'], overall['ref_time']) == (14.0, 0.0, 5.0, 114.0)
    assert overall['der'] == 100.0 * 19.0 / 114.0


def test_refusals(corpus, capsys, monkeypatch):
    from vbx_amd import diarize, score, vbhmm
    ref, hyp = str(corpus / 'ref.rttm'), str(corpus / 'sysAB.rttm')
    with pytest.raises(SystemExit):                                          # no UEM
        score.main(['-r', ref, '-s', hyp, '-u', 'all.uem'])
    assert 'not supported' in capsys.readouterr().err
    (corpus / 'stray.rttm').write_text(rttm_text('recZ', [(0.0, 1.0, 1)]))
    with pytest.raises(ValueError, match='recZ'):
        score.score_rttm(ref, [hyp, str(corpus / 'stray.rttm')])
    with pytest.raises(SystemExit):
        score.main(['-r', ref, '-s', hyp, str(corpus / 'stray.rttm')])
    assert 'recZ' in capsys.readouterr().err
    with pytest.raises(ValueError, match='collar'):
        score.score_turns([([], [])], collar=-1.0)
    # --ref-rttm-dir under torchrun with several ranks: refused before anything is read or any process group is formed
    monkeypatch.setenv('WORLD_SIZE', '2')
    argv = ['--init', 'AHC', '--out-rttm-dir', str(corpus / 'out'), '--xvec-ark-file', 'none.ark', '--segments-file', 'none.seg',
            '--xvec-transform', 'none.h5', '--plda-file', 'none', '--threshold', '0', '--lda-dim', '128', '--Fa', '0.3', '--Fb',
            '17', '--loopP', '0.99', '--ref-rttm-dir', str(corpus)]
    with pytest.raises(SystemExit):
        vbhmm.main(argv)
    assert 'more than one rank' in capsys.readouterr().err and not (corpus / 'out').exists()
    with pytest.raises(ValueError, match='more than one rank'):
        vbhmm.check_ref_rttm_dir(vbhmm.build_parser().parse_args(argv))
    with pytest.raises(SystemExit):
        diarize.parse_args(['--gpus', '0', '--checkpoint', 'none.pth', '--in-file-list', 'l', '--in-lab-dir', 'l', '--in-wav-dir',
                            'w'] + argv[:4] + argv[8:])
    assert 'more than one rank' in capsys.readouterr().err
    monkeypatch.setenv('WORLD_SIZE', '1')
    args = vbhmm.build_parser().parse_args(argv)
    vbhmm.check_ref_rttm_dir(args)                                           # one rank: accepted
    assert (args.collar, args.ignore_overlaps) == (0.25, False)
    assert vbhmm.build_parser().parse_args(argv[:-2]).ref_rttm_dir is None


def test_help_says_der_only(capsys):
    from vbx_amd import score
    with pytest.raises(SystemExit):
        score.main(['--help'])
    text = capsys.readouterr().out
    assert 'DER ONLY' in text and 'JER' in text and '--ignore_overlaps' in text and '--collar' in text


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_built_from_its_header():
    from vbx_amd import _capi, build, score
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'\bint vbx_rttm_score\s*\(', header) and 'vbx_rttm_score' in _capi.ABI_SYMBOLS
    assert '#define VBX_ABI_VERSION 7' in header
    assert 'vbx_rttm_score.hpp' in build.HEADERS and 'vbx_rttm_score.hpp' not in build.ITERATION_SOURCES
    src = open(os.path.join(build.CSRC, 'vbx_rttm_score.hpp')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (kRttm\w+) = (\d+);', src)}
    assert (_capi.RTTM_CLS_BLOCK, _capi.RTTM_TURN_CHUNK, _capi.RTTM_GROUP_CELLS, _capi.RTTM_ACC_CHUNK, _capi.RTTM_MAX_SPEAKERS) == \
        (const['kRttmClsBlock'], const['kRttmTurnChunk'], const['kRttmGroupCells'], const['kRttmAccChunk'], const['kRttmMaxSpk'])
    assert score.MAX_DEVICE_SPEAKERS == const['kRttmMaxSpk'] == _capi.MAX_REF_LABELS
    assert 'atomic' not in src.split('#pragma once')[1]                      # sums in a fixed order
