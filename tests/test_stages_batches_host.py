"""What ``DeviceStages.vb``, ``vb_turns`` and ``vb_random`` ask of ``_capi.Batch``, call by call, without a device and without
the library: which batches are made, with which constructor arguments and in which order, which slot is set with what, what
is fetched after the run, where the results land, and that a batch is closed whatever happens.  The device side is
tests/test_gpu_diarize.py, tests/test_gpu_random_init.py and tests/test_gpu_turn_init.py."""
import types

import numpy as np
import pytest

NAN = float('nan')
T = [11, 12, 13, 14, 15, 16, 17, 18]                        # x-vectors of the eight resident recordings
ROW0 = [0, 11, 23, 36, 50, 65, 81, 98, 116]
KS = [5, 2, 7, 3]                                            # the four recordings asked for, not in archive order
STATES = [3, 70, 16, 17]                                     # -> padded 16, 128, 16, 32
RUN = dict(init_smoothing=5.0, maxIters=40, epsilon=1e-6, precision='fp32', loopProb=0.9, Fa=0.3, Fb=17.0)
TAIL = (5.0, 'Phi', 0.9, 0.3, 17.0)                          # init_smoothing, Phi, loopProb, Fa, Fb: how every setter call ends


class _World:
    """The fake ``_capi``: ``Batch`` records every call in ``log`` as (batch number, method, arguments)."""

    def __init__(self, elbos=(), fail_run=False):
        self.log, self.elbos, self.fail_run, self.n_batches = [], list(elbos), fail_run, 0

    def Batch(self, *args, **kwargs):
        n, self.n_batches = self.n_batches, self.n_batches + 1
        self.log.append((n, 'Batch', args, kwargs))
        return _Batch(self, n)


class _Batch:
    def __init__(self, world, n):
        self.world, self.n = world, n

    def __getattr__(self, method):
        if not method.startswith('set_recording_'):
            raise AttributeError(method)
        return lambda *args: self.world.log.append((self.n, method, args))

    def run(self, *args):
        self.world.log.append((self.n, 'run', args))
        if self.world.fail_run:
            raise RuntimeError('the run failed')

    def labels(self, b):
        self.world.log.append((self.n, 'labels', (b,)))
        return f'first {self.n}.{b}', f'second {self.n}.{b}'

    def n_iters(self, b):
        self.world.log.append((self.n, 'n_iters', (b,)))
        return 100 * self.n + b

    def final_elbos(self):
        self.world.log.append((self.n, 'final_elbos', ()))
        return self.world.elbos

    def close(self):
        self.world.log.append((self.n, 'close', ()))


def _stages(world):
    from vbx_amd import vbhmm
    stages = object.__new__(vbhmm.DeviceStages)
    stages.T, stages.row0, stages.Phi, stages.lda_dim, stages.xv, stages.ctx = T, np.array(ROW0, dtype=np.int64), 'Phi', 128, 'xv', 'ctx'
    stages._capi = types.SimpleNamespace(Batch=world.Batch)
    return stages


def _same(got, want):
    """Equal entry by entry; an array only counts as the very object that was handed in."""
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    if isinstance(want, dict):
        return isinstance(got, dict) and got.keys() == want.keys() and all(_same(got[k], want[k]) for k in want)
    if isinstance(want, np.ndarray):
        return got is want
    return type(got) is not np.ndarray and bool(got == want)


def _check_log(log, want):
    for line, (g, w) in enumerate(zip(log, want)):
        assert _same(g, w), f'call {line}: {g!r}, expected {w!r}'
    assert len(log) == len(want), log[len(want):] or want[len(log):]


def _batch(n, Ts, Ss):
    return (n, 'Batch', ('ctx', Ts, Ss, 128), dict(precision='fp32', max_iters=40))


def _fetch(n, slots):
    return [c for b in slots for c in ((n, 'labels', (b,)), (n, 'n_iters', (b,)))]


def _three_batches(setter, args):
    """The log of four recordings with STATES states: padded 16 (members 0 and 2), 32 (member 3), 128 (member 1)."""
    want = []
    for n, members in enumerate(([0, 2], [3], [1])):
        want.append(_batch(n, [T[KS[j]] for j in members], [STATES[j] for j in members]))
        want += [(n, setter, (b, 'xv', ROW0[KS[j]]) + tuple(args[j]) + TAIL) for b, j in enumerate(members)]
        want += [(n, 'run', (40, 1e-6))] + _fetch(n, range(len(members))) + [(n, 'close', ())]
    return want


THREE_BATCHES_RESULT = [('first 0.0', 'second 0.0', 0), ('first 2.0', 'second 2.0', 200), ('first 0.1', 'second 0.1', 1),
                        ('first 1.0', 'second 1.0', 100)]


def test_vb_makes_one_batch_per_padded_state_count_in_ascending_order():
    world = _World()
    labels = [np.array([0, 2, 1] + [0] * (T[KS[0]] - 3)), np.array([69, 0]), np.array([15]), np.array([3, 16, 0])]
    out = _stages(world).vb(KS, labels, **RUN)
    _check_log(world.log, _three_batches('set_recording_resident', [(lab,) for lab in labels]))
    assert out == THREE_BATCHES_RESULT


def test_vb_turns_buckets_by_the_speakers_of_the_turns_and_hands_the_ticks_over():
    world = _World()
    turns = [tuple(np.arange(3) + 10 * j + c for c in range(3)) + (s,) for j, s in enumerate(STATES)]       # (u, v, spk, S)
    segments = [(np.arange(2) + 100 * j, np.arange(2) + 100 * j + 50) for j in range(4)]                    # (a, b)
    out = _stages(world).vb_turns(KS, turns, segments, **RUN)
    _check_log(world.log, _three_batches('set_recording_turns', [segments[j] + turns[j][:3] for j in range(4)]))
    assert out == THREE_BATCHES_RESULT


def test_vb_random_runs_the_restarts_side_by_side_and_fetches_only_the_winners():
    elbos = [NAN, -5.0, -4.0, -2.0, -2.0, -3.0]
    world = _World(elbos)
    from vbx_amd import vbhmm
    out = _stages(world).vb_random([6, 1], 4, 3, 7, ['recA', 'dev000'], **RUN)
    want = [_batch(0, [T[6]] * 3 + [T[1]] * 3, [4] * 6)]
    for j, (k, name) in enumerate(((6, 'recA'), (1, 'dev000'))):
        want += [(0, 'set_recording_random', (3 * j + r, 'xv', ROW0[k], -1 if r == 0 else 3 * j, 7, vbhmm.name_hash(name), r) + TAIL)
                 for r in range(3)]
    assert [c[2][3] for c in want[1:]] == [-1, 0, 0, -1, 3, 3]
    want += [(0, 'run', (40, 1e-6)), (0, 'final_elbos', ())] + _fetch(0, [2, 3]) + [(0, 'close', ())]
    _check_log(world.log, want)
    assert len(out) == 2 and out[0][:4] == ('first 0.2', 'second 0.2', 2, 2) and out[1][:4] == ('first 0.3', 'second 0.3', 3, 0)
    assert [np.isnan(out[0][4][0]), list(out[0][4][1:]), list(out[1][4])] == [True, [-5.0, -4.0], [-2.0, -2.0, -3.0]]


def test_vb_random_with_one_restart_and_one_recording():
    world = _World([-9.5])
    from vbx_amd import vbhmm
    out = _stages(world).vb_random([4], 2, 1, 0, ['recB'], **RUN)
    _check_log(world.log, [_batch(0, [T[4]], [2]), (0, 'set_recording_random', (0, 'xv', ROW0[4], -1, 0, vbhmm.name_hash('recB'), 0) + TAIL),
                           (0, 'run', (40, 1e-6)), (0, 'final_elbos', ())] + _fetch(0, [0]) + [(0, 'close', ())])
    assert out == [('first 0.0', 'second 0.0', 0, 0, [-9.5])]


def test_no_recordings_make_no_batch_and_vb_random_still_checks_its_arguments():
    world = _World()
    stages = _stages(world)
    assert stages.vb([], [], **RUN) == [] and stages.vb_turns([], [], [], **RUN) == []
    assert stages.vb_random([], 4, 3, 7, [], **RUN) == []
    for N, restarts in ((4, 0), (0, 3), (4, -1)):
        with pytest.raises(ValueError, match='both must be >= 1'):
            stages.vb_random([], N, restarts, 7, [], **RUN)
        with pytest.raises(ValueError, match='both must be >= 1'):
            stages.vb_random([6], N, restarts, 7, ['recA'], **RUN)
    assert world.log == []


@pytest.mark.parametrize('method', ['vb', 'vb_turns', 'vb_random'])
def test_a_run_that_raises_still_closes_the_batch_and_nothing_is_fetched(method):
    world = _World([-1.0, -2.0], fail_run=True)
    stages = _stages(world)
    with pytest.raises(RuntimeError, match='the run failed'):
        if method == 'vb':
            stages.vb([5, 2], [np.array([0, 2]), np.array([69])], **RUN)
        elif method == 'vb_turns':
            stages.vb_turns([5, 2], [(np.arange(1),) * 3 + (3,), (np.arange(1),) * 3 + (70,)], [(np.arange(2),) * 2] * 2, **RUN)
        else:
            stages.vb_random([5, 2], 4, 1, 0, ['recA', 'recB'], **RUN)
    assert [c[1] for c in world.log[-2:]] == ['run', 'close'] and world.n_batches == 1        # (no second batch after the failure)
    assert not any(c[1] in ('labels', 'n_iters', 'final_elbos') for c in world.log)


def test_padded_states_is_the_batch_modules_rule():
    from vbx_amd import vbhmm
    assert [vbhmm.DeviceStages.padded_states(s) for s in (1, 3, 16, 17, 32, 33, 64, 65, 70, 128, 129, 16384)] == \
        [16, 16, 16, 32, 32, 64, 64, 128, 128, 128, 256, 16384]
