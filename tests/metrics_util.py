"""Pairs shared by the host and the GPU tests of ``vbx_amd.metrics``: the crafted ones of DESIGN section 20, pairs with a
given number of cells or result entries, seeded random pairs."""
import numpy as np


def shifted(turns, by):
    return [(b + by, e + by, s) for b, e, s in turns]


def chain(n, speakers=('A', 'B'), length=0.05, start=0.0):
    """n turns back to back, the speakers taking them in rotation: n + 1 distinct boundaries, n cells"""
    return [(start + length * i, start + length * (i + 1), speakers[i % len(speakers)]) for i in range(n)]


def grid_pair(k, s, frames=4):
    """k reference speakers one after the other, s system speakers one after the other over the same extent: k reference and s
    system classes, a result of k + s + 2 k s entries"""
    total = k * s * frames * 0.01
    ref = [(total * i / k, total * (i + 1) / k, f'r{i:02d}') for i in range(k)]
    hyp = [(total * i / s, total * (i + 1) / s, f's{i:02d}') for i in range(s)]
    return ref, hyp


def counter_pair(bits, cell=0.02):
    """2^bits cells; reference speaker k speaks in cell c where bit k of c is set: 2^bits reference classes"""
    ref = []
    for k in range(bits):
        run = 1 << k
        ref += [(cell * c, cell * (c + run), f'r{k}') for c in range(run, 1 << bits, 2 * run)]
    return ref, [(0.0, cell * (1 << bits) / 2, 'x')]


def many_speakers(n, side='ref'):
    spk = [(0.5 * i, 0.5 * i + 0.75, f'p{i:02d}') for i in range(n)]
    few = [(0.0, 0.5 * n / 2, 'u'), (0.5 * n / 2 - 1.0, 0.5 * n + 0.25, 'v')]
    return (spk, few) if side == 'ref' else (few, spk)


# boundaries on frame times where quotient, product and literal disagree in float64 (test_metrics_host spells it out)
EDGE_REF = [(0.07, 0.29, 'A'), (0.29, 0.57, 'B'), (0.57, 1.0, 'A')]
EDGE_SYS = [(0.0, 0.07, 'x'), (0.07, 0.57, 'y'), (0.29, 0.9, 'x')]

CRAFTED = {
    'product_edges': (EDGE_REF, EDGE_SYS),
    'product_edges_swapped': (EDGE_SYS, EDGE_REF),
    'shorter_than_a_frame': ([(0.0, 1.0, 'A'), (0.123, 0.127, 'C'), (1.0, 2.0, 'B')], [(0.0, 2.0, 'x'), (0.4711, 0.4712, 'y')]),
    'three_overlapping': ([(0.0, 3.0, 'A'), (1.0, 4.0, 'B'), (2.0, 5.0, 'C')], [(0.5, 2.5, 'x'), (2.25, 4.75, 'y'), (2.4, 2.6, 'z')]),
    'starts_after_zero': (shifted(EDGE_REF, 1234.5), shifted(EDGE_SYS, 1234.56)),
    'empty_system': ([(0.0, 1.0, 'A'), (1.5, 2.0, 'B')], []),
    'empty_reference_with_speech': ([], [(0.3, 1.0, 'x'), (0.5, 2.0, 'y')]),
    'empty_reference_without_frames': ([], [(0.001, 0.002, 'x')]),
    'both_empty': ([], []),
    'one_frame': ([(0.0, 0.011, 'A')], [(0.0, 0.011, 'x')]),
    'below_one_frame': ([(0.0, 0.009, 'A')], [(0.001, 0.008, 'x')]),
    'integer_labels': ([(0.0, 1.0, 'A'), (1.0, 2.0, 'B')], [(0.0, 1.2, 2), (1.2, 2.0, 1)]),
    'same_speaker_overlapping_turns': ([(0.0, 1.0, 'A'), (0.5, 1.5, 'A'), (1.5, 2.0, 'A')], [(0.25, 1.75, 'x'), (1.75, 1.75, 'y')]),
}
SPEAKERS_64 = {'ref_64': many_speakers(64, 'ref'), 'sys_64': many_speakers(64, 'sys')}
SPEAKERS_65 = {'ref_65': many_speakers(65, 'ref'), 'sys_65': many_speakers(65, 'sys')}
CLASSES_OVER_CAP = counter_pair(9)              # 512 reference classes: more than the 256 the device returns


def random_pair(seed):
    """1 to 64 speakers a side, 0 to 600 turns, durations from 0.001 s to 2000 s, starts up to 1e5 s; most times have three
    decimals, as in RTTM files, so that boundaries of the two sides coincide now and then"""
    rng = np.random.default_rng(seed)
    offset = float(rng.choice([0.0, rng.uniform(0.0, 1e5)]))
    longest = float(rng.choice([2.0, 20.0, 2000.0], p=[0.5, 0.4, 0.1]))
    window = float(rng.choice([5.0, 60.0, 600.0]))
    digits = int(rng.choice([2, 3, 3, 9]))
    n_turns = int(rng.choice([0, 1, 3, 40, 255, 256, 600, int(rng.integers(0, 601))]))
    n_ref_turns = int(rng.integers(0, n_turns + 1))
    sides = []
    for n, tag in ((n_ref_turns, 'r'), (n_turns - n_ref_turns, 's')):
        n_spk = int(rng.integers(1, 65))
        start = offset + np.round(rng.uniform(0.0, window, n), digits)
        dur = np.round(np.exp(rng.uniform(np.log(0.001), np.log(longest), n)), digits)
        spk = rng.integers(0, n_spk, n)
        sides.append([(float(b), float(b + d), f'{tag}{k:02d}') for b, d, k in zip(start, dur, spk)])
    return sides[0], sides[1]
