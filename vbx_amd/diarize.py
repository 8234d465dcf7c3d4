#!/usr/bin/env python
"""python -m vbx_amd.diarize: wav files to RTTM files in one process, the x-vectors never leaving the device.

    python -m vbx_amd.diarize --gpus 0 --checkpoint raw_81.pth --in-file-list list.txt --in-wav-dir wav --in-lab-dir lab \\
        --init AHC+VB --out-rttm-dir out --xvec-transform transform.h5 --plda-file plda --threshold -0.015 --lda-dim 128 \\
        --Fa 0.3 --Fb 17 --loopP 0.99

is ``python -m vbx_amd.predict`` followed by ``python -m vbx_amd.vbhmm`` with the same flags -- the same RTTM bytes --
without the ark file, the second process and the upload between them:

  per file      the front end, the window plan and the model calls of ``predict`` (full windows --batch-size at a time,
                the others in ragged batches), the next file read and dithered ahead on a host thread; every embedding is
                written into ONE device array that lives until the end of the list
  after the     ``_capi.nan_rows`` flags the embeddings ``predict`` would drop (only the flags come back), the kept rows
  last file     are projected where they lie (``XVectors.from_device``) and ``vbhmm.diarize_recordings`` runs its stages
                on them: AHC per recording, all recordings in one VB batch per padded state count, the RTTM files

The segment times take the way they take between the two programs: ``window_plan``'s text line, parsed back by
``read_xvector_timing_dict``.  ``--out-ark-fn`` with ``--out-seg-fn`` also writes ``predict``'s two files (the one case in
which the embeddings are copied to the host).  One process, one GPU, ``--checkpoint`` networks only: ``torchrun`` sharding
stays with ``vbx_amd.vbhmm``, TorchScript modules with ``vbx_amd.predict``.

As a library: ``diarize_files(file_names, wav_dir, lab_dir, checkpoint, xvec_transform, plda_file, ...)``.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import io
import itertools
import logging
import os
import sys
import time

import numpy as np

from . import fbank, predict, vbhmm
from .kaldi_formats import read_xvector_timing_dict

__all__ = ['main', 'diarize_files', 'build_parser', 'parse_args', 'segment_times', 'plan_recordings']

logger = logging.getLogger('vbx_amd.diarize')

TIMING_KEYS = ('read', 'fbank', 'network', 'project', 'ahc', 'vb', 'rttm', 'total')


def build_parser():
    """The union of predict's and vbhmm's command lines; the files that connect the two become optional."""
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # ---- predict
    p.add_argument('--gpus', type=str, default='', help='the device to run on (first index of the list); required')
    p.add_argument('--checkpoint', type=str, default=None,
                   help="ResNet101 weights in predict.py's --weights format (e.g. raw_81.pth), run in HIP; required")
    p.add_argument('--gemm', default='exact', choices=['exact', 'split'],
                   help='how the network multiplies: exact f32 matrix instructions (default), or f16 matrix instructions on '
                        'error-compensated operand pairs (f32-level accuracy, faster)')
    p.add_argument('--model', type=str, default=None, help='not supported: use --checkpoint')
    p.add_argument('--weights', type=str, default=None, help='not supported: use --checkpoint')
    p.add_argument('--model-file', type=str, default=None, help='not supported here: TorchScript modules run in vbx_amd.predict')
    p.add_argument('--backend', default='pytorch', choices=['pytorch', 'onnx'], help='only pytorch is supported')
    p.add_argument('--ndim', type=int, default=64, help='dimensionality of features')
    p.add_argument('--embed-dim', type=int, default=256, help='dimensionality of the emb')
    p.add_argument('--seg-len', type=int, default=144, help='segment length')
    p.add_argument('--seg-jump', type=int, default=24, help='segment jump')
    p.add_argument('--in-file-list', required=True, type=str, help='input list of files')
    p.add_argument('--in-lab-dir', required=True, type=str, help='input directory with VAD labels')
    p.add_argument('--in-wav-dir', required=True, type=str, help='input directory with wavs')
    p.add_argument('--resample-to', type=int, default=None, choices=[8000, 16000], metavar='{8000,16000}',
                   help='take wavs of any PCM format, channel count and rate (vbx_amd.audio) and convert them on the device to '
                        'mono 16-bit at this rate first (default: only mono 16-bit wavs at 8 or 16 kHz are taken)')
    p.add_argument('--out-ark-fn', type=str, default=None, help="optional: also write predict's embedding file")
    p.add_argument('--out-seg-fn', type=str, default=None, help="optional: also write predict's segments file")
    p.add_argument('--batch-size', type=int, default=128, help='full windows per model call')
    p.add_argument('--no-dither', action='store_true', help='skip the dither (the reference always adds it)')
    p.add_argument('--dither', default='host', choices=['host', 'device'],
                   help="where the dither is drawn: by numpy on the host (default), or by the front end's MT19937 kernel on "
                        'the device, to the same bits')
    # ---- vbhmm
    vbhmm.add_init_arguments(p)
    p.add_argument('--out-rttm-dir', required=True, type=str, help='Directory to store output rttm files')
    p.add_argument('--xvec-transform', required=True, type=str, help='x-vector transformation: h5 (or npz) file')
    p.add_argument('--plda-file', required=True, type=str, help='PLDA model in Kaldi format')
    p.add_argument('--threshold', required=True, type=float, help='threshold (bias) used for AHC')
    p.add_argument('--lda-dim', required=True, type=int, help='x-vectors are reduced to this dimensionality for VB-HMM')
    p.add_argument('--Fa', required=True, type=float, help='Parameter of VB-HMM (see VBx.VBx)')
    p.add_argument('--Fb', required=True, type=float, help='Parameter of VB-HMM (see VBx.VBx)')
    p.add_argument('--loopP', required=True, type=float, help='Parameter of VB-HMM (see VBx.VBx)')
    p.add_argument('--target-energy', required=False, type=float, default=1.0,
                   help='with --ahc-scores plda: the share of the x-vectors\' variability the PCA before the scoring keeps')
    p.add_argument('--ahc-scores', required=False, type=str, default='cos', choices=['cos', 'plda'],
                   help='similarity of the AHC stage: cosine or the Kaldi-recipe PLDA scores')
    p.add_argument('--init-smoothing', required=False, type=float, default=5.0,
                   help='smoothing of the hard AHC labels into the initial soft assignments')
    p.add_argument('--output-2nd', required=False, type=bool, default=False,
                   help='Output also second most likely speaker of VB-HMM')
    p.add_argument('--precision', default='fp64', choices=['fp64', 'fp32', 'fp32-split'],
                   help='arithmetic of the VB-HMM kernels (fp64 = the reference\'s dtype and iteration counts)')
    p.add_argument('--timing', action='store_true', help='print a JSON line with the stage timings')
    vbhmm.add_decode_argument(p)
    vbhmm.add_score_arguments(p)
    return p


def _check(args, error):
    """What predict's and vbhmm's parsers refuse, plus what only the two-program route offers."""
    if args.backend == 'onnx':
        error('--backend onnx is not supported: the one-process route runs the --checkpoint network in HIP')
    if args.model_file is not None:
        error('--model-file is not supported here: the one-process route keeps the embeddings of the --checkpoint network on '
              'the device; run a TorchScript module with vbx_amd.predict and vbx_amd.vbhmm')
    if args.model is not None or args.weights is not None or args.checkpoint is None:
        error('--model/--weights are not supported: pass ResNet101 weights with --checkpoint (e.g. --checkpoint '
              'VBx/models/ResNet101_16kHz/nnet/raw_81.pth)')
    if args.no_dither and args.dither == 'device':
        error('--no-dither and --dither device exclude each other')
    if str(args.gpus).strip() == '':
        error('--gpus is empty: this route runs on a GPU only; pass a device index such as --gpus 0')
    if args.ndim != fbank.N_MEL:
        error(f'--ndim must be {fbank.N_MEL} (the filterbank has {fbank.N_MEL} channels)')
    if args.seg_len <= 0 or args.seg_jump <= 0 or args.batch_size <= 0:
        error('--seg-len, --seg-jump and --batch-size must be positive')
    if (args.out_ark_fn is None) != (args.out_seg_fn is None):
        error('--out-ark-fn and --out-seg-fn go together: pass both or neither')
    if getattr(args, 'resample_to', None) not in (None, 8000, 16000):
        error(f'--resample-to must be 8000 or 16000, got {args.resample_to}')
    if not 0 <= args.loopP <= 1:
        error(f'Expecting loopP between 0 and 1, got {args.loopP} instead.')
    if getattr(args, 'ref_rttm_dir', None) is not None:
        try:
            vbhmm.check_ref_rttm_dir(args, int(os.environ.get('WORLD_SIZE', 1)))
        except ValueError as exc:
            error(str(exc))


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    _check(args, p.error)
    vbhmm.check_init_arguments(args, p.error)
    vbhmm.check_decode_argument(args, p.error)
    return args


# ---- host logic between the network and the stages ----------------------------------------------------------------
def segment_times(lines):
    """``{recording: (x-vector names, [n, 2] start / end seconds)}`` of ``window_plan``'s lines, through the text form:
    the parser that reads ``predict``'s segments file reads them, so ``merge_adjacent_labels`` sees the same doubles."""
    if not lines:
        return {}
    return read_xvector_timing_dict(io.StringIO(''.join(line + os.linesep for line in lines)))


def plan_recordings(file_names, keys, lines, nan_flags, warn=logger.warning):
    """What is left of the windows once the NaN embeddings are dropped.  keys / lines: of every embedded window in list
    order; nan_flags bool [n].  -> (rows, recordings, segs_dict, vanished): rows int64 -- the kept indices, None where
    nothing is dropped; recordings [(name, x-vector names, None)] as ``read_vec_flt_ark_grouped`` would group the kept
    keys; segs_dict from the kept lines; vanished: the files no x-vector is left of (no window, or every one dropped).
    Every dropped key is reported with predict's warning text."""
    nan_flags = np.asarray(nan_flags, dtype=bool).reshape(-1)
    assert len(keys) == len(lines) == nan_flags.shape[0]
    for i in np.flatnonzero(nan_flags):
        warn(f'NaN found, not processing: {keys[i]}{os.linesep}')
    kept = np.flatnonzero(~nan_flags).astype(np.int64)
    kept_keys = [keys[i] for i in kept]
    recordings = [(name, np.array(list(group)), None)
                  for name, group in itertools.groupby(kept_keys, lambda key: key.rsplit('_', 1)[0])]
    segs_dict = segment_times([lines[i] for i in kept])
    left = {r[0] for r in recordings}
    vanished = [fn for fn in file_names if fn not in left]
    return (None if len(kept) == len(keys) else kept), recordings, segs_dict, vanished


# ---- the device array of all embeddings ----------------------------------------------------------------------------
class _DeviceRows:
    """[capacity][E] f32 on the device (a torch tensor: plain memory to the library); grows by doubling, contents kept."""

    def __init__(self, torch, device, E, capacity):
        self.torch, self.device, self.E = torch, torch.device('cuda', device), int(E)
        self.buf = torch.empty((max(int(capacity), 1), self.E), dtype=torch.float32, device=self.device)
        self.stage = None
        self.n = 0
        torch.cuda.synchronize(self.device)

    def reserve(self, extra):
        need = self.n + int(extra)
        if need > self.buf.shape[0]:
            grown = self.torch.empty((max(need, 2 * self.buf.shape[0]), self.E), dtype=self.torch.float32, device=self.device)
            grown[:self.n].copy_(self.buf[:self.n])
            self.torch.cuda.synchronize(self.device)
            self.buf = grown

    def ptr(self, row=0):
        return self.buf.data_ptr() + 4 * self.E * int(row)

    def staging(self, n):
        if self.stage is None or self.stage.shape[0] < n:
            self.stage = self.torch.empty((int(n), self.E), dtype=self.torch.float32, device=self.device)
            self.torch.cuda.synchronize(self.device)
        return self.stage

    def scatter(self, positions):
        """rows positions[j] <- staging row j (the library's run has synchronized its stream: the staging rows are there)"""
        idx = self.torch.as_tensor(np.asarray(positions, dtype=np.int64), device=self.device)
        self.buf.index_copy_(0, idx, self.stage[:len(positions)])
        self.torch.cuda.synchronize(self.device)


def _embed_file_device(net, fe, fn, sig, segs, sr, args, dest, timing):
    """predict.embed_file with the embeddings left on the device: window i of the file's plan is row dest.n + i.  A batch
    whose windows are neighbours in the plan is written where it belongs; any other lands in a staging block and is
    moved row by row on the device.  -> the plan."""
    t0 = time.perf_counter()
    rows = (fe.run_raw if args.dither == 'device' else fe.run)([(sig, segs)])[0]
    plan = fbank.window_plan(fn, segs, sr, args.seg_len, args.seg_jump)
    t1 = time.perf_counter()
    dest.reserve(len(plan))
    start = lambda i: rows[plan[i].seg] + plan[i].start
    for part, length in predict.window_batches(plan, args, True):
        straight = part[-1] - part[0] == len(part) - 1
        out_ptr = dest.ptr(dest.n + part[0]) if straight else dest.staging(len(part)).data_ptr()
        if length is None:
            net.embed_windows_ragged(fe, [start(i) for i in part], [plan[i].end - plan[i].start for i in part], out_ptr=out_ptr)
        else:
            net.embed_windows(fe, [start(i) for i in part], length, out_ptr=out_ptr)
        if not straight:
            dest.scatter([dest.n + i for i in part])
    dest.n += len(plan)
    timing['fbank'] += t1 - t0
    timing['network'] += time.perf_counter() - t1
    return plan


def _run(args, file_names, log=print):
    """-> ({recording: dict(labels1st, labels2nd, n_iters, thr, starts, ends)}, timing)"""
    import torch
    from . import _capi, xvector
    t_start = time.perf_counter()
    timing = dict.fromkeys(TIMING_KEYS, 0.0)
    device = int(str(args.gpus).split(',')[0])
    if not torch.cuda.is_available() or device >= torch.cuda.device_count():
        raise SystemExit(f'--gpus {args.gpus}: no such GPU visible to PyTorch')
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    nxt = pool.submit(predict._read_ahead, args, file_names[0]) if file_names else None
    try:
        net = xvector.ResNet101.from_checkpoint(args.checkpoint, device, embed_dim=args.embed_dim, gemm=args.gemm)
    except (ValueError, OSError) as exc:
        raise SystemExit(f'--checkpoint {args.checkpoint}: {exc}')
    models = vbhmm.load_models(args.xvec_transform, args.plda_file)
    timing['read'] += time.perf_counter() - t_start
    keys, lines, dest = [], [], None
    with torch.no_grad():
        for k, fn in enumerate(file_names):
            t0 = time.perf_counter()
            got = nxt.result()
            nxt = pool.submit(predict._read_ahead, args, file_names[k + 1]) if k + 1 < len(file_names) else None
            sr, sig, segs = predict._loaded(args, fn, got, device)        # (--resample-to: the conversion, on this thread)
            timing['read'] += time.perf_counter() - t0
            fe = fbank.front_end(sr, device)
            if dest is None:
                dest = _DeviceRows(torch, device, net.embed_dim, 0)
            plan = _embed_file_device(net, fe, fn, sig, segs, sr, args, dest, timing)
            keys += [w.key for w in plan]
            lines += [w.line for w in plan]
            logger.info(f'{fn}: {time.perf_counter() - t0:.3f} s')
    pool.shutdown()
    n = len(keys)
    t_proj = time.perf_counter()
    ctx = _capi.default_context(device)
    flags = _capi.nan_rows(ctx, dest.ptr(), n, net.embed_dim) if n else np.zeros(0, dtype=bool)
    rows, recordings, segs_dict, vanished = plan_recordings(file_names, keys, lines, flags)
    for fn in vanished:
        logger.warning(f'{fn}: no x-vector left, no RTTM file is written')
    if args.out_ark_fn is not None:                         # predict's two files: the one copy of the embeddings to the host
        emb = dest.buf[:n].cpu().numpy() if n else np.empty((0, net.embed_dim), np.float32)
        with open(args.out_seg_fn, 'w') as seg_file, open(args.out_ark_fn, 'wb') as ark_file:
            for i in np.flatnonzero(~flags):
                seg_file.write(lines[i] + os.linesep)
                ark_file.write(predict._ark_entry(keys[i], emb[i]))
    state, core = {}, dict(project=0.0, ahc=0.0, vb=0.0, rttm=0.0, recordings=0, xvectors=0)
    if recordings:
        xv = _capi.XVectors.from_device(ctx, dest.ptr(), n, net.embed_dim, rows, models['mean1'], models['lda'], models['mean2'],
                                        models['plda_mu'], models['plda_tr'], args.lda_dim)
        dest = None                                         # (the projections are all the stages read)
        stages = vbhmm.DeviceStages(device)
        try:
            state, core = vbhmm.diarize_recordings(recordings, segs_dict, models, args, stages, log=log, xvectors=xv,
                                                   t_start=t_proj, t_read=t_proj)
        finally:
            if stages.xv is None:
                xv.close()
            stages.close()
    for name, st in state.items():
        st['starts'], st['ends'] = segs_dict[name][1][:, 0].copy(), segs_dict[name][1][:, 1].copy()
    if getattr(args, 'ref_rttm_dir', None) is not None:
        vbhmm.score_state(args, state, device)
    for key in ('project', 'ahc', 'vb', 'rttm'):
        timing[key] = core[key]
    timing['total'] = time.perf_counter() - t_start
    timing.update(recordings=core['recordings'], xvectors=core['xvectors'], windows=n, dropped=int(np.count_nonzero(flags)))
    return state, timing


def diarize_files(file_names, wav_dir, lab_dir, checkpoint, xvec_transform, plda_file, *, out_rttm_dir=None, device=0,
                  init='AHC+VB', threshold=-0.015, lda_dim=128, Fa=0.3, Fb=17.0, loopP=0.99, target_energy=1.0,
                  ahc_scores='cos', init_smoothing=5.0, output_2nd=False, precision='fp64', gemm='exact', embed_dim=256,
                  seg_len=144, seg_jump=24, batch_size=128, no_dither=False, dither='host', out_ark_fn=None, out_seg_fn=None,
                  log=None, ref_rttm_dir=None, collar=0.25, ignore_overlaps=False, resample_to=None, random_restarts=None,
                  seed=None, init_rttm_dir=None, decode='posterior'):
    """Diarize ``wav_dir/<name>.wav`` with the VAD labels ``lab_dir/<name>.lab`` for every name of ``file_names``.

    -> ``({recording: dict(labels1st, labels2nd, n_iters, thr, starts, ends)}, timing)``: per x-vector of the recording its
    speaker (and the second most likely one after VB-HMM), the VB iterations, the calibrated AHC threshold and the
    x-vector's start and end in seconds; ``timing`` in seconds with the keys read, fbank, network, project, ahc, vb, rttm,
    total.  A recording no x-vector is left of has no entry.  With ``out_rttm_dir`` the RTTM files ``python -m
    vbx_amd.diarize`` writes are written too (``<out_rttm_dir>2nd`` with ``output_2nd``).  ``checkpoint``: a path in
    predict.py's ``--weights`` format, or a state_dict.  The hyper-parameters are the command line's.

    ``ref_rttm_dir`` (needs ``out_rttm_dir``): the RTTM files written are scored against ``<ref_rttm_dir>/<name>.rttm`` on the
    device with ``collar`` / ``ignore_overlaps`` (``vbx_amd.score``), the DER table is printed and every recording's entry
    gets its ``der``.  Without it nothing is scored, printed or added.

    ``resample_to`` (8000 or 16000): the wav files may be of any format ``vbx_amd.audio`` reads and are converted on the
    device to mono int16 at that rate first.  Without it only mono 16-bit files at 8 or 16 kHz are taken.

    ``init='random_<N>'``: no AHC; the VB-HMM starts from random labels over N speakers, ``random_restarts`` times (default 1),
    drawn from ``seed`` (default 0) and the recording's name (``vbhmm.DeviceStages.vb_random``); an entry then also holds the
    winning ``restart`` and the final ``elbos`` of all of them, and ``thr`` is nan.

    ``init='RTTM+VB'`` with ``init_rttm_dir``: no AHC; the VB-HMM starts from the diarization ``<init_rttm_dir>/<name>.rttm``,
    resampled on the device onto the windows the extraction left (``vbhmm.DeviceStages.vb_turns``); ``init='RTTM'`` returns and
    writes that resampling alone.  ``thr`` is nan.

    ``decode='viterbi'`` (with an ``init`` that runs the VB-HMM): ``labels1st`` is the jointly most probable speaker sequence
    of the HMM under the model of the last iteration instead of the frame-wise largest responsibility, ``labels2nd`` the best
    other speaker of every frame (``vbhmm.DeviceStages``, ``_capi.Batch.path``); at most 1024 speakers per recording."""
    if decode not in vbhmm.DECODES:
        raise ValueError(f'decode must be one of {vbhmm.DECODES}, not {decode!r}')
    args = argparse.Namespace(
        gpus=str(device), checkpoint=checkpoint, gemm=gemm, model=None, weights=None, model_file=None, backend='pytorch',
        ndim=fbank.N_MEL, embed_dim=embed_dim, seg_len=seg_len, seg_jump=seg_jump, in_file_list=None, in_lab_dir=lab_dir,
        in_wav_dir=wav_dir, out_ark_fn=out_ark_fn, out_seg_fn=out_seg_fn, batch_size=batch_size, no_dither=no_dither,
        dither=dither, init=init, out_rttm_dir=out_rttm_dir, xvec_transform=xvec_transform, plda_file=plda_file,
        threshold=threshold, lda_dim=lda_dim, Fa=Fa, Fb=Fb, loopP=loopP, target_energy=target_energy, ahc_scores=ahc_scores,
        init_smoothing=init_smoothing, output_2nd=output_2nd, precision=precision, timing=False, resample_to=resample_to,
        random_restarts=random_restarts, seed=seed, init_rttm_dir=init_rttm_dir, decode=decode)
    if ref_rttm_dir is not None:
        args.ref_rttm_dir, args.collar, args.ignore_overlaps = ref_rttm_dir, collar, ignore_overlaps
    try:
        vbhmm.random_init_states(init)
    except ValueError:
        raise ValueError(f"init must be 'AHC', 'AHC+VB', 'RTTM', 'RTTM+VB' or 'random_<N>', not {init!r}") from None

    def error(msg):
        raise ValueError(msg)
    _check(args, error)
    vbhmm.check_init_arguments(args, error, warn=lambda _message: None)       # (a library call has said what it wants)
    vbhmm.check_decode_argument(args, error)
    if vbhmm.turn_init(init):                                                 # (a missing directory fails before the extraction)
        from .turn_init import check_init_rttm_dir
        check_init_rttm_dir(init_rttm_dir)
    return _run(args, [str(f) for f in file_names], log=log or (lambda *a: None))


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    file_names = [str(f) for f in np.atleast_1d(np.loadtxt(args.in_file_list, dtype=object))]
    try:
        _state, timing = _run(args, file_names)
    except RuntimeError as exc:                                   # (recordings the device path could not take: vbhmm.main)
        print(f'diarize: {type(exc).__name__}: {exc}', file=sys.stderr)
        return 1
    if args.timing:
        import json
        print(json.dumps(timing))
    return 0


if __name__ == '__main__':
    sys.exit(main())
