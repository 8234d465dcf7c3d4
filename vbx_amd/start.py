"""Where a run of the VB-HMM starts: ``--init`` with ``--init-rttm-dir``, ``--random-restarts`` and ``--seed``, decided once.

``AHC`` / ``AHC+VB`` start from the clusters of the AHC stage, ``random_<N>`` from random labels over N speakers (DESIGN section
23), ``RTTM`` / ``RTTM+VB`` from the speaker turns of a diarization that exists.  ``check_options`` is the one
validation of the four options; ``from_args`` gives the ``Start`` that the drivers (``vbhmm.diarize_recordings``,
``tune.tune_recordings``) ask at every stage.  Nothing else knows which kind of start is in play."""
import numpy as np

from ._capi import MAX_SPEAKERS


class Start:
    """One kind of start.  ``runs_ahc``: stage 1 is the AHC (and holds a T x T score matrix); ``runs_vb``: the VB-HMM follows;
    ``n_random``: N of random_<N>, else None; ``from_turns``: the start is read from ``init_rttm_dir``.  Every kind has
    ``states(name, labels)``, the number of states the device runs the recording with (``labels``: what stage 1 gave), and
    ``run(stages, ks, names, labels, common)``, the stage call of the VB-HMM for the recordings ``ks`` (indices into ``names`` and
    ``labels``) with the arguments it takes today (``common``: the keywords all three share)."""
    runs_ahc = from_turns = False
    result_keys = ()                          # what a result of ``run`` holds beyond labels and iterations, for the state entry

    def __init__(self, init, runs_vb=True, n_random=None):
        self.init, self.runs_vb, self.n_random = init, runs_vb, n_random
        self.init_rttm_dir, self.restarts, self.seed = None, 1, 0

    def read(self, names, segs_dict):
        """Before anything runs: the files the start needs, for the recordings ``names`` and no others."""

    def stage1(self, stages, k, name, threshold, ahc_kw):
        """Stage 1 of recording k -> (labels or None, calibrated threshold or nan)."""
        return None, float('nan')

    def too_many(self, n, tune_name=None, most=MAX_SPEAKERS):
        """Why a recording of ``n`` > ``most`` states is left out (MAX_SPEAKERS; ``--decode viterbi``: the decode's limit);
        ``tune_name``: as tune words it, which ends there."""
        return self.TOO_MANY.format(who='' if tune_name is None else f'{tune_name}: ', init=self.init, n=n, most=most)


class AhcStart(Start):
    runs_ahc = True
    TOO_MANY = '{who}AHC left {n} clusters, the device path takes at most {most}'
    use_instead = 'AHC+VB or random_<N>'

    def stage1(self, stages, k, name, threshold, ahc_kw):
        return stages.ahc(k, threshold, **ahc_kw)

    def states(self, name, labels):
        return int(np.max(labels)) + 1 if self.runs_vb else 0        # (AHC alone: nothing runs with states)

    def run(self, stages, ks, names, labels, common):
        return stages.vb(ks, [labels[k] for k in ks], **common)


class RandomStart(Start):
    TOO_MANY = '--init {init}: the device path takes at most {most} states'         # (every recording alike: nobody is named)
    result_keys = ('restart', 'elbos')                               # the winning restart and every restart's final ELBO

    def states(self, name, labels):
        return self.n_random

    def run(self, stages, ks, names, labels, common):
        return stages.vb_random(ks, self.n_random, self.restarts, self.seed, [names[k] for k in ks], **common)


class TurnStart(Start):
    from_turns = True
    TOO_MANY = '{who}--init {init}: {n} speakers, the device path takes at most {most}'
    use_instead = 'RTTM+VB'

    def read(self, names, segs_dict):
        from .turn_init import read_init_turns, window_ticks
        self.given = {}                                              # {name: ((a, b), (u, v, spk, S))} in ticks
        for name in names:
            u, v, spk, speakers = read_init_turns(self.init_rttm_dir, name)
            self.given[name] = (window_ticks(segs_dict[name][1]), (u, v, spk, len(speakers)))

    def stage1(self, stages, k, name, threshold, ahc_kw):
        segments, turns = self.given[name]
        final = not self.runs_vb and turns[3] <= MAX_SPEAKERS        # RTTM only (too many speakers: reported after the run)
        return (stages.turn_labels(k, turns, segments) if final else None), float('nan')

    def states(self, name, labels):
        return self.given[name][1][3]

    def run(self, stages, ks, names, labels, common):
        return stages.vb_turns(ks, [self.given[names[k]][1] for k in ks], [self.given[names[k]][0] for k in ks], **common)


def parse(init):
    """The ``Start`` of an ``--init`` value, its other options at their defaults; ValueError for anything that is none."""
    if init in ('AHC', 'AHC+VB'):
        return AhcStart(init, init == 'AHC+VB')
    if init in ('RTTM', 'RTTM+VB'):
        return TurnStart(init, init == 'RTTM+VB')
    head, sep, digits = str(init).partition('_')
    if head != 'random' or not sep or not digits.isascii() or not digits.isdigit() or int(digits) < 1:
        raise ValueError(f"invalid choice: {init!r} (choose from 'AHC', 'AHC+VB', 'RTTM', 'RTTM+VB', 'random_<N>' with N a decimal integer >= 1)")
    return RandomStart(init, n_random=int(digits))


def check_options(init, init_rttm_dir=None, random_restarts=None, seed=None, need_vb=False):
    """The one check of ``--init``, ``--init-rttm-dir``, ``--random-restarts`` and ``--seed`` (None: not given) -> (restarts, seed)
    with the defaults 1 and 0, or ValueError.  ``need_vb``: a start that runs no VB-HMM is refused (tune)."""
    start = parse(init)
    if need_vb and not start.runs_vb:
        raise ValueError(f'--init {init} runs no VB-HMM: Fa, Fb and loopP change nothing; use {start.use_instead}')
    if start.from_turns != (init_rttm_dir is not None):
        raise ValueError(f'--init {init} needs --init-rttm-dir: the diarization to start from' if start.from_turns else
                         f'--init-rttm-dir needs --init RTTM or RTTM+VB: --init {init} reads no diarization')
    for flag, value in (('--random-restarts', random_restarts), ('--seed', seed)):
        if start.n_random is None and value is not None:
            raise ValueError(f'{flag} needs --init random_<N>: --init {init} draws nothing')
    restarts, seed = (1 if random_restarts is None else int(random_restarts)), (0 if seed is None else int(seed))
    if restarts < 1:
        raise ValueError(f'--random-restarts {restarts}: must be >= 1')
    if not 0 <= seed < 1 << 64:
        raise ValueError(f'--seed {seed}: must be in 0 .. 2^64 - 1')
    return restarts, seed


def from_args(args, need_vb=False):
    """The checked ``Start`` of a run from a namespace; ``init`` defaults to AHC+VB where absent (tune, before it had the option)."""
    start = parse(getattr(args, 'init', 'AHC+VB'))
    start.init_rttm_dir = getattr(args, 'init_rttm_dir', None)
    start.restarts, start.seed = check_options(start.init, start.init_rttm_dir, getattr(args, 'random_restarts', None),
                                               getattr(args, 'seed', None), need_vb)
    return start


def ahc_options_ignored(init):
    """The line a command prints where ``--init`` runs no AHC; None where it does."""
    return None if parse(init).runs_ahc else f'--init {init} runs no AHC: --threshold, --ahc-scores and --target-energy are ignored'
