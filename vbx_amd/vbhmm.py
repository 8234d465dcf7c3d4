#!/usr/bin/env python
"""Diarization driver with the command line of the reference's ``VBx/vbhmm.py``, built around the batched
MI355X path:

    python -m vbx_amd.vbhmm --init AHC+VB --out-rttm-dir out --xvec-ark-file x.ark --segments-file x.seg \\
        --xvec-transform transform.h5 --plda-file plda --threshold -0.015 --lda-dim 128 --Fa 0.3 --Fb 17 --loopP 0.99

The reference walks the recordings of the archive one after another (vbhmm.py:120) and runs everything on one
CPU thread.  Here the loop is split into stages:

  0. ALL x-vectors of this rank go to the device once; the projections of vbhmm.py:125-129 and the PLDA projection
     ``fea`` of vbhmm.py:153 are computed there for the whole archive and stay resident;
  1. per recording: AHC initialisation -- similarity matrix of the resident rows, threshold calibration and the
     average-linkage nearest-neighbour chain on the device (one persistent workgroup per recording, several recordings
     side by side on their own streams), the cut of the dendrogram on the host;
  2. ALL recordings of this rank in one ``vbx_batch``: initial responsibilities from the AHC labels on the device
     (vbhmm.py:150-152), one launch sequence per EM iteration for the whole archive, convergence per recording on the
     device (vbhmm.py:154-158 call, batched), first / second speaker by a device arg-sort (vbhmm.py:160-162);
  3. per recording, as soon as its labels exist: merging of adjacent segments and the RTTM file (vbhmm.py:166-179).

Under ``torchrun`` (one process per GPU) the recordings are dealt to the ranks by cost; every rank writes the
RTTM files of its own recordings and the ranks only meet in a barrier at the end.  Same flags, same files, same
RTTM bytes as the reference driver.

``--init random_N`` (the reference's README.md:24) skips stage 1: stage 2 starts every recording from random
labels over N speakers drawn on the device from (``--seed``, the recording's name, the restart), ``--random-restarts R`` times
side by side in the one batch, and keeps the restart with the largest final ELBO.  No T x T matrix is ever held.

``--init RTTM+VB --init-rttm-dir DIR`` skips stage 1 too: stage 2 starts every recording from the speaker
turns of ``DIR/<recording>.rttm``, a diarization that exists, resampled onto the x-vector windows on the device -- the VB-HMM
as the second stage of a system.  ``--init RTTM`` only writes that resampling out.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from .batch import padded_states
from .kaldi_formats import (read_plda, read_vec_flt_ark_grouped, read_xvec_transform, read_xvector_timing_dict,
                            write_rttm)
from .start import ahc_options_ignored, check_options, from_args, parse

__all__ = ['main', 'diarize', 'diarize_recordings', 'DeviceStages', 'tune_host_process', 'load_models', 'cluster', 'cut_linkage', 'merge_adjacent_labels', 'l2_norm',
           'random_init_states', 'name_hash', 'best_restart', 'add_init_arguments', 'check_init_arguments', 'turn_init', 'runs_vb',
           'runs_ahc']


def l2_norm(vec_or_matrix):
    """Rows (or the vector) scaled to unit Euclidean length.  diarization_lib.py:169-187."""
    a = np.asarray(vec_or_matrix)
    if a.ndim == 1:
        return a / np.linalg.norm(a)
    if a.ndim == 2:
        return a / np.linalg.norm(a, axis=1, ord=2)[:, np.newaxis]
    raise ValueError('Wrong number of dimensions, 1 or 2 is supported, not %i.' % a.ndim)


def merge_adjacent_labels(starts, ends, labels):
    """Adjacent or overlapping segments with the same label become one; overlapping segments with different
    labels meet in the middle of the overlap.  diarization_lib.py:116-137."""
    starts, ends, labels = np.asarray(starts), np.asarray(ends), np.asarray(labels)
    touching = np.logical_or(np.isclose(ends[:-1], starts[1:]), ends[:-1] > starts[1:])
    cut = np.nonzero(np.logical_or(~touching, labels[1:] != labels[:-1]))[0]
    starts = starts[np.r_[0, cut + 1]]
    ends = ends[np.r_[cut, -1]]
    labels = labels[np.r_[0, cut + 1]]
    over = np.nonzero(starts[1:] < ends[:-1])[0]
    ends[over] = starts[over + 1] = (ends[over] + starts[over + 1]) / 2.0
    return starts, ends, labels


def random_init_states(init):
    """N for ``--init random_N`` (N a decimal integer >= 1), None for ``AHC``, ``AHC+VB``, ``RTTM`` and ``RTTM+VB``; ValueError
    for anything else (as from the three below: ``start.parse`` is the one place that reads the value)."""
    return parse(init).n_random


def turn_init(init):
    """Does this ``--init`` start from the speaker turns of ``--init-rttm-dir``?  RTTM and RTTM+VB do."""
    return parse(init).from_turns


def runs_ahc(init):
    """Does this ``--init`` run the AHC stage (and hold its T x T score matrix)?"""
    return parse(init).runs_ahc


def runs_vb(init):
    """Does this ``--init`` run the VB-HMM?  AHC+VB, RTTM+VB and random_N do (README.md:24: 'and run VBx')."""
    return parse(init).runs_vb


def name_hash(name):
    """FNV-1a-64 of the recording's name (UTF-8): the half of the Philox key that makes a recording's random labels its own,
    wherever it stands in the archive and whichever rank it is dealt to."""
    h = 0xcbf29ce484222325
    for byte in name.encode('utf-8'):
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def best_restart(final_elbos):
    """Index of the restart with the largest final ELBO: the lowest among equals, never one whose ELBO is nan; 0 if all are."""
    best = 0
    for r, v in enumerate(final_elbos):
        if v == v and (final_elbos[best] != final_elbos[best] or v > final_elbos[best]):
            best = r
    return best


def load_models(xvec_transform, plda_file):
    """x-vector transform and the PLDA model in the simultaneously diagonalised form of vbhmm.py:107-113."""
    from scipy.linalg import eigh
    mean1, mean2, lda = read_xvec_transform(xvec_transform)
    plda_mu, plda_tr, plda_psi = read_plda(plda_file)
    with _small_blas_pool():       # 256 x 256: 0.30 s with the BLAS pool of a 256-core host, 0.01 s on four threads
        W = np.linalg.inv(plda_tr.T.dot(plda_tr))
        B = np.linalg.inv((plda_tr.T / plda_psi).dot(plda_tr))
        acvar, wccn = eigh(B, W)
    return dict(mean1=mean1, mean2=mean2, lda=lda, plda_mu=plda_mu, plda_psi=acvar[::-1], plda_tr=wccn.T[::-1],
                kaldi_plda=(plda_mu, plda_tr, plda_psi))          # the raw model: what --ahc-scores plda scores under


def cut_linkage(lin_mat, thr, threshold):
    """vbhmm.py:142-146: the linkage matrix shifted to non-negative distances and cut at the calibrated threshold ->
    integer cluster label per x-vector (``vbx_fcluster_distance``: SciPy's fcluster(criterion='distance'), native)."""
    from . import _capi
    if len(lin_mat) == 0:
        return np.zeros(1, dtype=np.int64)
    adjust = abs(lin_mat[:, 2].min())
    lin_mat[:, 2] += adjust
    return _capi.fcluster_distance(lin_mat, -(thr + threshold) + adjust).astype(np.int64) - 1


def cluster(cond, thr, threshold):
    """Average-linkage clustering of condensed negated similarities held on the HOST, cut at the calibrated threshold
    (vbhmm.py:140-146): ``vbx_linkage_average`` (nearest-neighbour chain, SciPy's linkage matrix bit for bit -- SciPy is
    the stand-in for the un-installed fastcluster, whose average-linkage update may differ from it in the last bit).
    The driver itself clusters on the device (``DeviceStages.ahc``); this serves callers with their own matrix."""
    from . import _capi
    return cut_linkage(_capi.linkage_average(cond), thr, threshold)


class DeviceStages:
    """The device side of the driver (no host fallback: without the HIP library every method raises).  Which of ``vb``,
    ``vb_random`` and ``vb_turns`` a run calls, and what stage 1 is, is decided once, by the ``Start`` of ``vbx_amd/start.py``.

    project   every x-vector of this rank goes up ONCE; the projections of vbhmm.py:125-129 and the PLDA projection of
              vbhmm.py:153 run on the device for all recordings together and stay resident (vbx_xvectors)
    ahc       per recording: cosine-similarity matrix of its resident rows (or, ``ahc_scores='plda'``, their dense PLDA
              scores under the raw Kaldi model: diarization_lib.py:59-93), two-Gaussian calibration and the
              average-linkage nearest-neighbour chain, all on the T x T matrix where it lies in HBM (vbhmm.py:135-141);
              the T - 1 merges come back and are cut on the host (vbhmm.py:142-146).  Every driver thread has its own
              context (device stream), so the chains of several recordings run side by side on different CUs
    vb        ALL recordings in one ``vbx_batch``: initial responsibilities built on the device from the AHC labels
              (vbhmm.py:150-152), one launch sequence per EM iteration for the whole archive, convergence per recording
              on the device (vbhmm.py:154-158), first / second speaker by a device arg-sort (vbhmm.py:160-162): only
              labels come back
    vb_random ``--init random_N``: no AHC; the restarts of ALL recordings in one ``vbx_batch``, every restart from labels drawn
              on the device, the restarts of a recording around one rho; the winner by final ELBO, only its labels come back
    vb_turns  ``--init RTTM+VB``: no AHC; initial responsibilities from the speaker turns of a diarization that exists,
              resampled onto the x-vector windows on the device: only window edges and turns go up (``turn_labels``: ``--init
              RTTM``, that resampling alone)
    """

    def __init__(self, device=None):
        import threading
        from . import _capi
        self._capi = _capi
        self.ctx = _capi.default_context(device)
        self.xv = None
        self._local = threading.local()
        self._thread_ctxs = []

    def _thread_ctx(self):
        """A context (= a HIP stream) of its own for every driver thread: a ctx is not thread-safe."""
        ctx = getattr(self._local, 'ctx', None)
        if ctx is None:
            ctx = self._local.ctx = self._capi.Context(self.ctx.device)
            self._thread_ctxs.append(ctx)
        return ctx

    def _layout(self, T, models, lda_dim):
        self.T = [int(t) for t in T]
        self.row0 = np.concatenate([[0], np.cumsum(self.T)]).astype(np.int64)
        self.Phi = np.ascontiguousarray(models['plda_psi'][:lda_dim])
        self.lda_dim = lda_dim
        self.kaldi_plda = models.get('kaldi_plda')
        self._plda_full = None

    def project(self, recordings, models, lda_dim):
        self._layout([len(r[1]) for r in recordings], models, lda_dim)
        if not recordings:
            return
        x = np.concatenate([np.asarray(r[2]) for r in recordings])
        self.xv = self._capi.XVectors(self.ctx, x, models['mean1'], models['lda'], models['mean2'], models['plda_mu'],
                                      models['plda_tr'], lda_dim)

    def project_device(self, T, xvectors, models, lda_dim):
        """Adopts x-vectors projected where the network left them (``XVectors.from_device`` with ``lda_dim`` as its
        ``fea_dim``): recording k owns the T[k] rows from sum(T[:k]) on.  Nothing goes up; close() releases them."""
        self._layout(T, models, lda_dim)
        if xvectors is None:
            if self.T:
                raise ValueError('project_device: recordings without x-vectors')
            return
        if xvectors.n != int(self.row0[-1]) or xvectors.fea_dim != lda_dim or xvectors.ctx.device != self.ctx.device:
            raise ValueError(f'project_device: {xvectors.n} rows of {xvectors.fea_dim} dimensions on device '
                             f'{xvectors.ctx.device}, the recordings ask for {int(self.row0[-1])} of {lda_dim} on device '
                             f'{self.ctx.device}')
        self.xv = xvectors

    # The device linkage merges all reciprocal nearest-neighbour pairs per round on the whole chip (round 4: 1.2 ms at
    # T = 1025, 2.2 ms at 4000, 5.8 ms at 10 000, 19 ms at 20 000; the one-workgroup chain of rounds 2-3: 12 / 54 / 174 / 512 ms);
    # the host routine needs ~3 ns per matrix entry plus the condensed matrix over PCIe (3 ms at T = 1025): the device from ~600
    DEVICE_LINKAGE_FROM = 600

    def _plda_scores(self, k, target_energy):
        """Dense PLDA scores of the resident rows of recording k (kaldi_ivector_plda_scoring_dense)."""
        from . import diarization_lib
        if self.kaldi_plda is None:
            raise ValueError("ahc_scores='plda' needs the raw PLDA model: load_models()['kaldi_plda']")
        if target_energy >= 1.0 and self._plda_full is None:         # all dimensions kept: one projection for every recording
            self._plda_full = diarization_lib.plda_projection(self.kaldi_plda, None)     # (pure: a race computes it twice)
        sc, _pca_dim = diarization_lib.plda_dense_scores(self._thread_ctx(), self.kaldi_plda,
                                                         resident=(self.xv, self.row0[k], self.T[k]),
                                                         target_energy=target_energy, full_projection=self._plda_full)
        return sc

    def ahc(self, k, threshold, ahc_scores='cos', target_energy=1.0):
        """-> (AHC labels of recording k, calibrated threshold)."""
        if ahc_scores == 'plda':
            if self.T[k] == 1:                        # nothing to score: one x-vector is one cluster
                return np.zeros(1, dtype=np.int64), float('nan')
            sc = self._plda_scores(k, target_energy)
        elif ahc_scores == 'cos':
            sc = self._capi.Scores.cos_similarity_resident(self._thread_ctx(), self.xv, self.row0[k], self.T[k])
        else:
            raise ValueError(f"ahc_scores must be 'cos' or 'plda', not {ahc_scores!r}")
        try:
            thr, _ = sc.two_gmm_calib(20, want_llr=False)
            if self.T[k] >= self.DEVICE_LINKAGE_FROM and self._capi.linkage_variant() == 'scipy':
                lin_mat = sc.linkage_average(self.T[k])                # (SciPy's update formula; the tree of the host routine)
            else:                                     # short recording: the host chain beats the device's step latency
                lin_mat = self._capi.linkage_average(sc.get_condensed(self.T[k], -1.0)) if self.T[k] > 1 else np.empty((0, 4))
        finally:
            sc.close()
        return cut_linkage(lin_mat, thr, threshold), float(thr)

    padded_states = staticmethod(padded_states)       # the padded state count a batch of this many speakers runs with

    @staticmethod
    def _read_out(batch, decode):
        """first / second speaker of a slot: the frame-wise argmax of the responsibilities (vbhmm.py:160-162) or, ``--decode
        viterbi``, the most probable speaker sequence and the best other speaker of every frame (``Batch.path``)."""
        if decode not in DECODES:
            raise ValueError(f'decode must be one of {DECODES}, not {decode!r}')
        return batch.path if decode == 'viterbi' else batch.labels

    def _run_batches(self, ks, S, slots, set_slots, maxIters, epsilon, precision, collect=None, decode='posterior'):
        """The batch work of every start -> one result per recording of ``ks``, in their order.  ``S[j]`` states and ``slots`` batch
        slots for ``ks[j]``; ``set_slots(batch, b, j)`` sets the slots b .. b + slots - 1 of ``ks[j]``; after the run ``collect(batch)``
        is called once and what it returns once per recording, with its first slot (default: the slot's labels and iterations).
        One ``vbx_batch`` per padded state count, the narrowest first: every recording of a batch runs with the widest one's
        padding, and one recording with more than 64 states would push a whole archive from the fused kernels (responsibilities
        and lattices on the chip) onto the wide scan -- about 5x slower per iteration."""
        buckets = {}
        for j, s in enumerate(S):
            buckets.setdefault(self.padded_states(s), []).append(j)
        out = [None] * len(ks)
        for _sp, members in sorted(buckets.items()):
            batch = self._capi.Batch(self.ctx, [self.T[ks[j]] for j in members for _r in range(slots)],
                                     [S[j] for j in members for _r in range(slots)], self.lda_dim, precision=precision, max_iters=maxIters)
            try:
                for b, j in enumerate(members):
                    set_slots(batch, b * slots, j)
                batch.run(maxIters, epsilon)
                read_out = self._read_out(batch, decode)
                result_of = collect(batch) if collect else lambda b: (*read_out(b), batch.n_iters(b))
                for b, j in enumerate(members):
                    out[j] = result_of(b * slots)
            finally:
                batch.close()
        return out

    def vb(self, ks, labels, init_smoothing, maxIters, epsilon, precision, loopProb, Fa, Fb, decode='posterior'):
        """-> [(labels1st, labels2nd or None, iterations)] for the recordings ``ks`` with AHC labels ``labels``."""
        def set_slots(batch, b, j):
            batch.set_recording_resident(b, self.xv, self.row0[ks[j]], labels[j], init_smoothing, self.Phi, loopProb, Fa, Fb)
        return self._run_batches(ks, [int(np.max(lab)) + 1 for lab in labels], 1, set_slots, maxIters, epsilon, precision,
                                 decode=decode)

    def vb_random(self, ks, N, restarts, seed, names, init_smoothing, maxIters, epsilon, precision, loopProb, Fa, Fb,
                  decode='posterior'):
        """-> [(labels1st, labels2nd or None, iterations, winning restart, [final ELBO of every restart])] for the recordings
        ``ks`` (``names[j]`` names ``ks[j]``) started from random labels over N states, ``--init random_N``.

        ONE ``vbx_batch`` of len(ks) x restarts slots, since every slot has N states: restart 0 of a recording owns its rho,
        the others share it.  The labels are drawn on the device from (seed, name, restart); after the run only the ELBOs come
        back, the winner is picked here (``best_restart``) and only the winners' labels follow (``decode='viterbi'``: only the
        winner is decoded)."""
        R = int(restarts)
        if R < 1 or int(N) < 1:
            raise ValueError(f'vb_random: restarts={restarts}, N={N}: both must be >= 1')

        def set_slots(batch, b, j):
            h = name_hash(names[j])
            for r in range(R):
                batch.set_recording_random(b + r, self.xv, self.row0[ks[j]], -1 if r == 0 else b, seed, h, r, init_smoothing,
                                           self.Phi, loopProb, Fa, Fb)

        def winners(batch):
            elbos = batch.final_elbos()
            read_out = self._read_out(batch, decode)

            def winner(b):
                win = best_restart(elbos[b:b + R])
                return (*read_out(b + win), batch.n_iters(b + win), win, elbos[b:b + R])
            return winner
        return self._run_batches(ks, [int(N)] * len(ks), R, set_slots, maxIters, epsilon, precision, collect=winners)

    def turn_labels(self, k, turns, segments):
        """-> the labels of ``--init RTTM`` for recording k: per window ``segments`` = (a, b) the speaker of ``turns`` =
        (u, v, spk, S) (``turn_init.turn_ticks``, all in ticks) with the largest overlap, the nearest turn's where none overlaps
        (``_capi.turn_weights``, on the device)."""
        (a, b), (u, v, spk, S) = segments, turns
        if len(a) != self.T[k]:
            raise ValueError(f'recording {k}: {len(a)} windows in the segments file, {self.T[k]} x-vectors')
        return self._capi.turn_weights(self._thread_ctx(), a, b, u, v, spk, S, 0.0, want=('labels',))[0].astype(np.int64)

    def vb_turns(self, ks, turns, segments, init_smoothing, maxIters, epsilon, precision, loopProb, Fa, Fb, decode='posterior'):
        """-> [(labels1st, labels2nd or None, iterations)] for the recordings ``ks`` started from given speaker turns, ``--init
        RTTM+VB``: ``turns[j]`` = (u, v, spk, S) and ``segments[j]`` = (a, b) of ``ks[j]``, all in ticks (``turn_init``).  The
        responsibilities are built on the device from the ticks (``Batch.set_recording_turns``)."""
        def set_slots(batch, b, j):
            (a, e), (u, v, spk, _S) = segments[j], turns[j]
            batch.set_recording_turns(b, self.xv, self.row0[ks[j]], a, e, u, v, spk, init_smoothing, self.Phi, loopProb, Fa, Fb)
        return self._run_batches(ks, [int(t[3]) for t in turns], 1, set_slots, maxIters, epsilon, precision, decode=decode)

    def close_thread_contexts(self):
        """The per-thread contexts (a HIP stream each) of the AHC stage: closed before the VB batch creates its stream
        group, so that the group's streams do not share hardware queues with idle ones (8 queues per process)."""
        for ctx in self._thread_ctxs:
            ctx.close()
        self._thread_ctxs = []
        self._local = __import__('threading').local()

    def close(self):
        if self.xv is not None:
            self.xv.close()
            self.xv = None
        self.close_thread_contexts()


def _small_blas_pool():
    """Context manager: at most four BLAS / LAPACK threads (no-op without ``threadpoolctl`` or with VBX_AMD_TUNE_HOST=0)."""
    import contextlib
    if os.environ.get('VBX_AMD_TUNE_HOST', '1') == '0':
        return contextlib.nullcontext()
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
    except ImportError:
        return contextlib.nullcontext()
    # never RAISE a pool: a BLAS that started with one thread (torchrun exports OMP_NUM_THREADS=1) has per-thread buffers
    # for one, and scipy.linalg.eigh on a pool widened to four crashed in LAPACK (SIGSEGV, seen on both ranks of a node)
    now = [i.get('num_threads', 1) for i in threadpool_info() if i.get('user_api') == 'blas']
    limit = min([4] + now)
    return threadpool_limits(limits=limit, user_api='blas')


def tune_host_process():
    """Process-wide settings for a run that mixes worker threads with many multi-megabyte NumPy temporaries (measured
    on a 256-core host: without them the per-recording host work of stage 1 runs 5-10x slower than alone):

      * glibc serves every array above 128 KB with its own mmap and returns it with munmap; each munmap interrupts
        every core the process has threads on (BLAS pool, HIP runtime, clustering workers).  Raising the mmap and
        trim thresholds keeps those arrays in the heap, where they are recycled without system calls;
      * the matrix products of one recording are tiny (1000 x 256 x 128): a 64-thread BLAS pool costs more to wake
        than it saves.

    Returns a context manager that limits the BLAS pools (a no-op without ``threadpoolctl``).  Both are process-wide:
    an application that embeds ``diarize()`` and manages its own heap / BLAS settings switches them off with
    ``VBX_AMD_TUNE_HOST=0``."""
    import contextlib
    import ctypes
    if os.environ.get('VBX_AMD_TUNE_HOST', '1') == '0':
        return contextlib.nullcontext()
    try:
        libc = ctypes.CDLL(None)
        libc.mallopt(ctypes.c_int(-3), ctypes.c_int(1 << 30))     # M_MMAP_THRESHOLD (glibc clamps it to 32 MB)
        libc.mallopt(ctypes.c_int(-1), ctypes.c_int((1 << 31) - 1))   # M_TRIM_THRESHOLD
    except (OSError, AttributeError):
        pass
    return _small_blas_pool()


def driver_threads():
    """Worker threads of stage 1 (``VBX_AMD_DRIVER_THREADS``, default 6; one core stays free): the Python glue between the native calls
    limits the useful threads for short recordings; each holds a T x T score matrix on the device while it works (T = 20 000: 3.2 GB)."""
    return max(1, min(int(os.environ.get('VBX_AMD_DRIVER_THREADS', '6')), (os.cpu_count() or 2) - 1))


def _read_recordings(ark_path):
    """[(recording, names, x[T, D])] in archive order; x-vectors of a recording are consecutive (vbhmm.py:119)."""
    return read_vec_flt_ark_grouped(ark_path)


def _rank_world():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except ImportError:
        pass
    return int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))


def _write_rttm_files(args, file_name, st, segs_dict):
    """vbhmm.py:166-179 for one recording (nothing where ``args.out_rttm_dir`` is None: a library call that wants labels only)."""
    assert np.all(segs_dict[file_name][0] == st['seg_names'])                 # vbhmm.py:166
    if args.out_rttm_dir is None:
        return
    start, end = segs_dict[file_name][1].T
    starts, ends, out_labels = merge_adjacent_labels(start, end, st['labels1st'])
    os.makedirs(args.out_rttm_dir, exist_ok=True)
    with open(os.path.join(args.out_rttm_dir, f'{file_name}.rttm'), 'w') as fp:
        write_rttm(fp, file_name, out_labels, starts, ends)
    if args.output_2nd and runs_vb(args.init) and st['labels2nd'] is not None:
        starts, ends, out_labels2 = merge_adjacent_labels(start, end, st['labels2nd'])
        second = f'{args.out_rttm_dir}2nd'
        os.makedirs(second, exist_ok=True)
        with open(os.path.join(second, f'{file_name}.rttm'), 'w') as fp:
            write_rttm(fp, file_name, out_labels2, starts, ends)


def diarize(args, stages=None, log=print, ahc_scores=None):
    """The whole archive.  ``stages`` defaults to ``DeviceStages()`` (the CPU test-suite injects an object with the same
    four methods built on its checkers).  Returns ``({recording: dict(labels1st, labels2nd, n_iters, thr)}, timing)``
    for the recordings of this rank.  ``ahc_scores`` ('cos' | 'plda', default: ``args.ahc_scores``, 'cos' where absent)
    names the similarity of the AHC stage; 'plda' uses ``args.target_energy``.

    A recording the device path cannot take (more than ``VBX_MAX_SPEAKERS`` = 16 384 AHC clusters, or one whose batch
    fails) does not take the archive down with it: every other recording is diarized and written, then a
    ``RuntimeError`` names the ones left out.  RTTM files are written as soon as their labels exist.

    This is the part that reads the files; the stages are ``diarize_recordings``."""
    from .batch import shard_recordings
    assert 0 <= args.loopP <= 1, f'Expecting loopP between 0 and 1, got {args.loopP} instead.'
    _ahc_kw(args, ahc_scores)                                     # (a bad name fails before anything is read)
    t_start = time.perf_counter()
    segs_dict = read_xvector_timing_dict(args.segments_file)
    models = load_models(args.xvec_transform, args.plda_file)
    recordings = _read_recordings(args.xvec_ark_file)
    rank, world = _rank_world()
    if world > 1:                                                 # AHC is O(T^2), the VB loop O(T S): deal by T^2
        power = 2 if runs_ahc(args.init) else 1                          # (no AHC: O(T); the labels do not depend on the deal)
        assignment = shard_recordings([float(len(r[1])) ** power for r in recordings], world)
        recordings = [r for k, r in enumerate(recordings) if assignment[k] == rank]
    if turn_init(args.init):                                      # (a missing directory fails before anything runs)
        from .turn_init import check_init_rttm_dir
        check_init_rttm_dir(getattr(args, 'init_rttm_dir', None))
    t_read = time.perf_counter()
    ref_rttm_dir = getattr(args, 'ref_rttm_dir', None)
    if ref_rttm_dir is not None:
        check_ref_rttm_dir(args, world)
    state, timing = diarize_recordings(recordings, segs_dict, models, args, stages, log=log, ahc_scores=ahc_scores,
                                       t_start=t_start, t_read=t_read, rank=rank, world=world)
    if ref_rttm_dir is not None:                                  # on the device the stages ran on (injected host stages: in numpy)
        if stages is None:
            from ._capi import default_context
            device = default_context().device
        else:
            device = getattr(getattr(stages, 'ctx', None), 'device', None)
        score_state(args, state, device)
    return state, timing


def check_ref_rttm_dir(args, world=None):
    """``--ref-rttm-dir`` scores the RTTM files one process wrote: refused under ``torchrun`` with several ranks, and without
    an output directory."""
    if world is None:
        world = _rank_world()[1]
    if world > 1:
        raise ValueError('--ref-rttm-dir is not supported with more than one rank: every rank writes only its share of the '
                         'recordings; score the merged output with `python -m vbx_amd.score -r REF -s OUT/*.rttm`')
    if args.out_rttm_dir is None:
        raise ValueError('--ref-rttm-dir scores the RTTM files as written: it needs an output directory (out_rttm_dir)')
    if not os.path.isdir(args.ref_rttm_dir):                      # (found before the run, not after it)
        raise ValueError(f'--ref-rttm-dir {args.ref_rttm_dir}: no such directory')


def score_state(args, state, device=None):
    """The ``--ref-rttm-dir`` step of both drivers: the RTTM files just written, parsed back from their text, against
    ``<ref_rttm_dir>/<recording>.rttm`` on the run's device (``device=None``, a run on injected host stages: in numpy); the
    table goes to stdout and every recording's ``der`` into its state entry."""
    from . import score
    records, overall = score.score_written(args.out_rttm_dir, list(state), args.ref_rttm_dir, getattr(args, 'collar', 0.25),
                                           getattr(args, 'ignore_overlaps', False), device)
    print(score.format_table(records, overall))
    for name, rec in records.items():
        state[name]['der'] = rec['der']
    return records, overall


def _ahc_kw(args, ahc_scores):
    if ahc_scores is None:
        ahc_scores = getattr(args, 'ahc_scores', 'cos')
    if ahc_scores not in ('cos', 'plda'):
        raise ValueError(f"ahc_scores must be 'cos' or 'plda', not {ahc_scores!r}")
    return dict(ahc_scores='plda', target_energy=getattr(args, 'target_energy', 1.0)) if ahc_scores == 'plda' else {}


def diarize_recordings(recordings, segs_dict, models, args, stages=None, log=print, ahc_scores=None, xvectors=None,
                       t_start=None, t_read=None, rank=0, world=1):
    """The stages of ``diarize`` for recordings already in memory: ``[(name, seg_names, x_or_None)]``, ``segs_dict`` as
    ``read_xvector_timing_dict`` gives it, ``models`` from ``load_models``, ``args`` with the hyper-parameters
    (init, threshold, lda_dim, Fa, Fb, loopP, init_smoothing, output_2nd, out_rttm_dir and, optionally, precision,
    ahc_scores, target_energy, decode; init_rttm_dir with init = RTTM or RTTM+VB: ``<init_rttm_dir>/<name>.rttm`` is read for every
    recording given, and for no other).  Returns what ``diarize`` returns.

    ``xvectors``: the x-vectors of all recordings, in order, projected on the device already (``XVectors.from_device``,
    ``fea_dim`` = ``args.lda_dim``); the third entry of a recording is not read then and nothing is uploaded
    (``stages.project_device``).  ``stages`` adopts them: they are released with it (or by the caller of injected stages).
    ``t_start`` / ``t_read``: when the caller began and finished reading, for the timing (default: now)."""
    from ._capi import MAX_DECODE_STATES, MAX_SPEAKERS, VbxError
    assert 0 <= args.loopP <= 1, f'Expecting loopP between 0 and 1, got {args.loopP} instead.'
    ahc_kw = _ahc_kw(args, ahc_scores)
    decode = getattr(args, 'decode', 'posterior')
    if decode not in DECODES:
        raise ValueError(f'decode must be one of {DECODES}, not {decode!r}')
    if t_read is None:
        t_read = time.perf_counter()
    if t_start is None:
        t_start = t_read
    start = from_args(args)                                      # the one place that knows which kind of start this is
    names = [r[0] for r in recordings]
    start.read(names, segs_dict)                                 # (only the files of the recordings of this rank)
    own_stages = stages is None
    if own_stages:
        stages = DeviceStages()
    failed = {}
    try:
        # ---- stage 0: every x-vector of this rank to the device, projections for all recordings at once ---------------
        if xvectors is None:
            stages.project(recordings, models, args.lda_dim)
        else:
            stages.project_device([len(r[1]) for r in recordings], xvectors, models, args.lda_dim)
        t_proj = time.perf_counter()

        # ---- stage 1: AHC initialisation -----------------------------------------------------------------------------
        # A few recordings at a time on worker threads, each with its own device stream: the device calls run without
        # the interpreter lock and the nearest-neighbour chains of different recordings run on different CUs.
        from concurrent.futures import ThreadPoolExecutor

        def prepare(k):
            file_name, seg_names, _ = recordings[k]
            labels1st, thr = start.stage1(stages, k, file_name, args.threshold, ahc_kw)
            st = dict(labels1st=labels1st, labels2nd=None, thr=thr, n_iters=0, seg_names=seg_names)
            if not start.runs_vb and labels1st is not None:
                _write_rttm_files(args, file_name, st, segs_dict)        # AHC only, RTTM only: the result is final
            return file_name, st

        state = {}
        for rec in recordings:
            log(rec[0])                                               # vbhmm.py:121
        with tune_host_process(), ThreadPoolExecutor(max_workers=driver_threads()) as pool:
            for file_name, st in pool.map(prepare, range(len(recordings))):      # results in archive order
                state[file_name] = st
        if hasattr(stages, 'close_thread_contexts'):
            stages.close_thread_contexts()
        t_ahc = time.perf_counter()

        # ---- stage 2: every recording of this rank in one batch ------------------------------------------------------
        n_states = {name: start.states(name, state[name]['labels1st']) for name in names}
        most = MAX_DECODE_STATES if decode == 'viterbi' and start.runs_vb else MAX_SPEAKERS
        failed.update((name, start.too_many(n, most=most)) for name, n in n_states.items() if n > most)
        ks = [k for k, name in enumerate(names) if name not in failed]
        if start.runs_vb and recordings:
            common = dict(init_smoothing=args.init_smoothing, maxIters=40, epsilon=1e-6, precision=getattr(args, 'precision', 'fp64'),
                          loopProb=args.loopP, Fa=args.Fa, Fb=args.Fb)
            if decode != 'posterior':                                 # (the default: the stage calls as they have always been)
                common['decode'] = decode

            def finish(k, result):
                st = state[names[k]]
                st['labels1st'], st['labels2nd'], st['n_iters'] = result[:3]
                st.update(zip(start.result_keys, result[3:]))
                _write_rttm_files(args, names[k], st, segs_dict)

            def run_vb(some):
                return start.run(stages, some, names, {k: state[names[k]]['labels1st'] for k in some}, common)

            try:
                for k, result in zip(ks, run_vb(ks)):
                    finish(k, result)
            except VbxError as exc:          # one recording at a time, so that a bad one only costs itself
                log(f'batched VB-HMM failed ({exc}); retrying the recordings one by one')
                for k in ks:
                    try:
                        finish(k, run_vb([k])[0])
                    except VbxError as exc_k:
                        failed[names[k]] = str(exc_k)
        t_vb = time.perf_counter()
    finally:
        if own_stages:
            stages.close()
    for name in failed:
        state.pop(name, None)
    for st in state.values():
        st.pop('seg_names', None)
    t_end = time.perf_counter()
    timing = dict(read=t_read - t_start, project=t_proj - t_read, ahc=t_ahc - t_proj, vb=t_vb - t_ahc, rttm=t_end - t_vb,
                  total=t_end - t_start, recordings=len(state), xvectors=int(sum(len(st['labels1st']) for st in state.values())),
                  rank=rank, world=world)
    if failed:
        raise RuntimeError('no RTTM written for: ' + '; '.join(f'{k} ({v})' for k, v in failed.items()))
    return state, timing


def build_parser():
    """The arguments of vbhmm.py:54-101, plus the knobs of this implementation."""
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_init_arguments(p)
    p.add_argument('--out-rttm-dir', required=True, type=str, help='Directory to store output rttm files')
    p.add_argument('--xvec-ark-file', required=True, type=str,
                   help='Kaldi ark file with x-vectors from one or more input recordings (all x-vectors of one '
                        'recording consecutive)')
    p.add_argument('--segments-file', required=True, type=str, help='File with x-vector timing info')
    p.add_argument('--xvec-transform', required=True, type=str, help='x-vector transformation: h5 (or npz) file')
    p.add_argument('--plda-file', required=True, type=str, help='PLDA model in Kaldi format')
    p.add_argument('--threshold', required=True, type=float, help='threshold (bias) used for AHC')
    p.add_argument('--lda-dim', required=True, type=int, help='x-vectors are reduced to this dimensionality for VB-HMM')
    p.add_argument('--Fa', required=True, type=float, help='Parameter of VB-HMM (see VBx.VBx)')
    p.add_argument('--Fb', required=True, type=float, help='Parameter of VB-HMM (see VBx.VBx)')
    p.add_argument('--loopP', required=True, type=float, help='Parameter of VB-HMM (see VBx.VBx)')
    p.add_argument('--target-energy', required=False, type=float, default=1.0,
                   help='Parameter affecting AHC if the similarity matrix is obtained with PLDA (--ahc-scores plda): the '
                        'share of the x-vectors\' variability the PCA before the scoring keeps; >= 1 keeps every dimension')
    p.add_argument('--ahc-scores', required=False, type=str, default='cos', choices=['cos', 'plda'],
                   help='similarity of the AHC stage: cosine (what the reference driver computes) or the Kaldi-recipe '
                        'PLDA scores of diarization_lib.kaldi_ivector_plda_scoring_dense')
    p.add_argument('--init-smoothing', required=False, type=float, default=5.0,
                   help='smoothing of the hard AHC labels into the initial soft assignments')
    p.add_argument('--output-2nd', required=False, type=bool, default=False,
                   help='Output also second most likely speaker of VB-HMM')
    p.add_argument('--precision', default='fp64', choices=['fp64', 'fp32', 'fp32-split'],
                   help='arithmetic of the VB-HMM kernels (fp64 = the reference\'s dtype and iteration counts)')
    p.add_argument('--timing', action='store_true', help='print a JSON line with the stage timings of this rank')
    add_decode_argument(p)
    add_score_arguments(p)
    return p


DECODES = ('posterior', 'viterbi')


def add_decode_argument(p):
    """``--decode`` of vbhmm, diarize and tune."""
    p.add_argument('--decode', required=False, type=str, default='posterior', choices=list(DECODES),
                   help='how the VB-HMM is read out.  posterior: every x-vector gets the speaker of its largest responsibility, '
                        'frame by frame (what the reference driver writes; the default).  viterbi: the jointly most probable '
                        'speaker sequence of the HMM under the model of the last iteration, decoded on the device (at most 1024 '
                        'speakers per recording); with --output-2nd the second file holds the best other speaker of every frame')


def check_decode_argument(args, error):
    """After parsing: ``--decode viterbi`` decodes a VB-HMM, so an ``--init`` that runs none is refused."""
    if getattr(args, 'decode', 'posterior') == 'viterbi' and not runs_vb(args.init):
        return error(f'--decode viterbi needs the VB-HMM: --init {args.init} runs none (use {parse(args.init).use_instead})')


def _init_argument(value):
    try:
        random_init_states(value)
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc)) from None
    return value


def add_init_arguments(p, default=None):
    """``--init``, ``--random-restarts``, ``--seed`` and ``--init-rttm-dir`` of vbhmm, diarize and tune.  ``default`` None:
    ``--init`` is required."""
    p.add_argument('--init', required=default is None, default=default, type=_init_argument,
                   metavar='{AHC,AHC+VB,RTTM,RTTM+VB,random_<N>}',
                   help='AHC for using only AHC, AHC+VB for VB-HMM after AHC initilization, random_<N> for VB-HMM from random '
                        'labels over N speakers without any AHC (long recordings: AHC holds a T x T matrix), RTTM+VB for VB-HMM '
                        'from the diarization in --init-rttm-dir without any AHC, RTTM for only resampling that diarization '
                        'onto the x-vector windows')
    p.add_argument('--init-rttm-dir', required=False, type=str, default=None, metavar='DIR',
                   help='with --init RTTM or RTTM+VB: the diarization to start from, DIR/<recording>.rttm for every recording')
    p.add_argument('--random-restarts', required=False, type=int, default=None, metavar='R',
                   help='with --init random_<N>: runs from R different random labellings, the one with the largest final ELBO '
                        'wins (default: 1)')
    p.add_argument('--seed', required=False, type=int, default=None,
                   help='with --init random_<N>: seed of the random labels, 0 .. 2^64 - 1 (default: 0; a run is reproducible)')


def check_init_arguments(args, error, warn=None):
    """After parsing: what ``start.check_options`` refuses goes to ``error(message)``; with random_N ``--random-restarts`` and ``--seed``
    get their defaults 1 and 0; with anything but AHC and AHC+VB one line about the ignored AHC options goes to ``warn`` (default: stderr)."""
    try:
        restarts, seed = check_options(args.init, getattr(args, 'init_rttm_dir', None), args.random_restarts, args.seed)
    except ValueError as exc:
        return error(str(exc))
    if parse(args.init).n_random is not None:
        args.random_restarts, args.seed = restarts, seed
    message = ahc_options_ignored(args.init)
    if message is not None:
        (warn or (lambda text: print(f'warning: {text}', file=sys.stderr)))(message)


def add_score_arguments(p):
    """The scoring step the reference's recipes run after this program (dscore/score.py), as an option of it."""
    p.add_argument('--ref-rttm-dir', required=False, type=str, default=None,
                   help='score the RTTM files written against <dir>/<recording>.rttm on the device and print the DER table '
                        'of `python -m vbx_amd.score` (DER only; one process: not under torchrun with several ranks)')
    p.add_argument('--collar', required=False, type=float, default=0.25,
                   help='with --ref-rttm-dir: no-score zone round every reference turn boundary, seconds (default: %(default)s)')
    p.add_argument('--ignore_overlaps', action='store_true',
                   help='with --ref-rttm-dir: do not score where two or more reference speakers speak')


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_init_arguments(args, parser.error)
    check_decode_argument(args, parser.error)
    if args.ref_rttm_dir is not None:
        try:
            check_ref_rttm_dir(args, int(os.environ.get('WORLD_SIZE', 1)))
        except ValueError as exc:
            parser.error(str(exc))
    dist = None
    if int(os.environ.get('WORLD_SIZE', 1)) > 1:                  # launched by torchrun: one process per GPU
        import torch
        import torch.distributed as dist
        # one GPU per rank (LOCAL_RANK); VBX_AMD_DEVICE / VBX_AMD_DIST_BACKEND override both, e.g. several ranks sharing
        # one device over gloo (RCCL refuses two ranks on one GPU)
        if torch.cuda.is_available():
            os.environ.setdefault('VBX_AMD_DEVICE', os.environ.get('LOCAL_RANK', '0'))
            torch.cuda.set_device(int(os.environ['VBX_AMD_DEVICE']))
        dist.init_process_group(os.environ.get('VBX_AMD_DIST_BACKEND') or ('nccl' if torch.cuda.is_available() else 'gloo'))
    error = None
    timing = None
    try:
        try:
            _state, timing = diarize(args)
        except Exception as exc:           # the other ranks wait in the barrier below: meet them there first, then fail
            error = exc
        if dist is not None:
            dist.barrier()
    finally:
        if dist is not None and dist.is_initialized():
            dist.destroy_process_group()
    if error is not None:
        print(f'vbhmm: {type(error).__name__}: {error}', file=sys.stderr)
        return 1
    if args.timing:
        import json
        # one write, line end included: the ranks of a torchrun job share the stream, and an unbuffered one takes print's
        # text and line end separately, so that two ranks' lines could come out as one
        sys.stdout.write(json.dumps(timing) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
