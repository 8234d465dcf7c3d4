"""python -m vbx_amd.predict: predict.py's x-vector extraction with the front end on the GPU.

The command line is predict.py's.  The features of a file come from the device front end (vbx_amd.fbank: log-Mel
filterbank, floating CMN, windows cut straight into the model's [B, 64, 144] layout); the embedding model is either
ResNet101 from a checkpoint in predict.py's ``--weights`` format (``--checkpoint``, run by vbx_amd.xvector in HIP, the
windows gathered straight into its input buffer) or a TorchScript module (``--model-file``) run by PyTorch on the same
device.  Full windows go ``--batch-size`` at a time.  The other windows of a file -- one tail of its own length per VAD
segment -- go through the ``--checkpoint`` network together, as ragged batches of at most ``--batch-size`` x ``--seg-len``
frames (every embedding has the bits its window gives alone); a ``--model-file`` module takes them grouped by length.
The ark file and the segments file are the ones predict.py writes, in its order.  The dither of the next file is drawn on the host while the
device works on the current one; with ``--dither device`` the device draws it (the same MT19937 stream, the same bits), the
int16 samples go up instead of the f64 signal, and the host only reads the files ahead.

Not supported: ``--backend onnx`` and ``--model/--weights`` (pass the ResNet101 weights with ``--checkpoint``).
"""
from __future__ import annotations

import argparse
import concurrent.futures
import logging
import os
import struct
import sys
import time

import numpy as np

from . import fbank

logger = logging.getLogger('vbx_amd.predict')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--gpus', type=str, default='', help='the device to run on (first index of the list); required')
    p.add_argument('--model', type=str, default=None, help='not supported: use --checkpoint or --model-file')
    p.add_argument('--weights', type=str, default=None, help='not supported: use --checkpoint or --model-file')
    p.add_argument('--checkpoint', type=str, default=None,
                   help="ResNet101 weights in predict.py's --weights format (e.g. raw_81.pth), run in HIP")
    p.add_argument('--gemm', default='exact', choices=['exact', 'split'],
                   help='how the --checkpoint network multiplies: exact f32 matrix instructions (default), or f16 matrix '
                        'instructions on error-compensated operand pairs (f32-level accuracy, faster)')
    p.add_argument('--model-file', type=str, default=None, help='TorchScript embedding model: [B, ndim, T] -> [B, embed]')
    p.add_argument('--ndim', type=int, default=64, help='dimensionality of features')
    p.add_argument('--embed-dim', type=int, default=256, help='dimensionality of the emb')
    p.add_argument('--seg-len', type=int, default=144, help='segment length')
    p.add_argument('--seg-jump', type=int, default=24, help='segment jump')
    p.add_argument('--in-file-list', required=True, type=str, help='input list of files')
    p.add_argument('--in-lab-dir', required=True, type=str, help='input directory with VAD labels')
    p.add_argument('--in-wav-dir', required=True, type=str, help='input directory with wavs')
    p.add_argument('--out-ark-fn', required=True, type=str, help='output embedding file')
    p.add_argument('--out-seg-fn', required=True, type=str, help='output segments file')
    p.add_argument('--backend', default='pytorch', choices=['pytorch', 'onnx'], help='only pytorch is supported')
    p.add_argument('--batch-size', type=int, default=128, help='full windows per model call')
    p.add_argument('--no-dither', action='store_true', help='skip the dither (the reference always adds it)')
    p.add_argument('--dither', default='host', choices=['host', 'device'],
                   help="where the dither is drawn: by numpy on the host (default), or by the front end's MT19937 kernel on "
                        'the device, to the same bits')
    p.add_argument('--resample-to', type=int, default=None, choices=[8000, 16000], metavar='{8000,16000}',
                   help='take wavs of any PCM format, channel count and rate (vbx_amd.audio) and convert them on the device to '
                        'mono 16-bit at this rate first (default: only mono 16-bit wavs at 8 or 16 kHz are taken)')
    args = p.parse_args(argv)
    if args.no_dither and args.dither == 'device':
        p.error('--no-dither and --dither device exclude each other')
    if args.backend == 'onnx':
        p.error('--backend onnx is not supported: export the model to TorchScript and pass --model-file')
    if args.model is not None or (args.model_file is None and args.checkpoint is None):
        p.error('--model/--weights are not supported: pass ResNet101 weights with --checkpoint (e.g. --checkpoint '
                'VBx/models/ResNet101_16kHz/nnet/raw_81.pth) or a TorchScript module with --model-file')
    if args.model_file is not None and args.checkpoint is not None:
        p.error('--checkpoint and --model-file exclude each other: pass one embedding model')
    if args.gemm != 'exact' and args.checkpoint is None:
        p.error('--gemm applies to the --checkpoint network only')
    if args.gpus.strip() == '':
        p.error('--gpus is empty: this extractor runs on a GPU only; pass a device index such as --gpus 0')
    if args.ndim != fbank.N_MEL:
        p.error(f'--ndim must be {fbank.N_MEL} (the filterbank has {fbank.N_MEL} channels)')
    if args.seg_len <= 0 or args.seg_jump <= 0 or args.batch_size <= 0:
        p.error('--seg-len, --seg-jump and --batch-size must be positive')
    return args


def _ark_entry(key: str, vec: np.ndarray) -> bytes:
    """kaldi_io.write_vec_flt: '<key> \\0B' + 'FV ' / 'DV ' + '\\4' + int32 dim + the values."""
    tag = b'FV ' if vec.dtype == np.float32 else b'DV '
    return (key + ' ').encode('latin1') + b'\0B' + tag + b'\4' + struct.pack('<i', vec.shape[0]) + vec.tobytes()


def _load(args, fn):
    return _prepare(args, fn, *fbank.read_wav(os.path.join(args.in_wav_dir, fn) + '.wav', raw=args.dither == 'device'))


def _read_ahead(args, fn):
    """What the reader thread does for a file: all of _load, or with --resample-to only the reading of its bytes (the
    conversion is a device call, and those stay on the thread that owns the context: _loaded)."""
    if getattr(args, 'resample_to', None) is None:
        return _load(args, fn)
    from . import audio
    return audio.read_audio(os.path.join(args.in_wav_dir, fn) + '.wav')


def _loaded(args, fn, got, device):
    """_load's result from _read_ahead's: with --resample-to the bytes become mono int16 at that rate on the device, and
    everything after sees them as if fbank.read_wav had read the converted file."""
    if getattr(args, 'resample_to', None) is None:
        return got
    from . import audio
    data, fmt, channels, sr, _frames = got
    samples = audio.to_mono16([data], fmt, channels, sr, args.resample_to, device=device)[0]
    return _prepare(args, fn, samples if args.dither == 'device' else samples.astype(np.int64), args.resample_to)


def _prepare(args, fn, samples, sr):
    labs = fbank.read_lab(os.path.join(args.in_lab_dir, fn) + '.lab', sr)
    if args.dither == 'device':                  # the samples as read: embed_file has the device dither them
        return sr, samples, fbank.segments(labs, len(samples), sr)
    sig, segs = fbank.prepare(samples, labs, sr, dither_signal=not args.no_dither)
    return sr, sig, segs


def ragged_batches(lengths, max_frames):
    """Consecutive runs of the windows (indices into lengths) of at most max_frames frames in all -- at least one window
    each: what bounds the workspace of a ragged run."""
    out, cur, frames = [], [], 0
    for i, n in enumerate(lengths):
        if cur and frames + n > max_frames:
            out.append(cur)
            cur, frames = [], 0
        cur.append(i)
        frames += n
    if cur:
        out.append(cur)
    return out


def window_batches(plan, args, ragged):
    """The model calls of one file, in the order embed_file makes them: [(indices into plan, length)].  With ragged, the
    windows that are not full ones come first, in ragged batches (length None); the others are grouped by length, full
    windows --batch-size at a time."""
    groups = {}
    for i, w in enumerate(plan):
        groups.setdefault(w.end - w.start, []).append(i)
    out = []
    if ragged:
        rest = [i for i, w in enumerate(plan) if w.end - w.start != args.seg_len]
        groups = {n: idx for n, idx in groups.items() if n == args.seg_len}
        lengths = [plan[i].end - plan[i].start for i in rest]
        for part in ragged_batches(lengths, args.batch_size * args.seg_len):
            out.append(([rest[j] for j in part], None))
    for length, idx in groups.items():
        step = args.batch_size if length == args.seg_len else len(idx)
        for b0 in range(0, len(idx), step):
            out.append((idx[b0:b0 + step], length))
    return out


def embed_file(embed, fe, fn, sig, segs, sr, args, embed_ragged=None):
    """(key, segments line, embedding) of every window of one file, in predict.py's order.  embed(fe, starts, length):
    the embeddings [n][E] (numpy) of the windows of `length` frames from feature rows `starts`.  embed_ragged(fe, starts,
    lengths), if given, takes the windows that are not full ones, of whatever lengths, in one call; without it they are
    grouped by length.  sig is the dithered f64 signal, or with --dither device the integer samples."""
    rows = (fe.run_raw if getattr(args, 'dither', 'host') == 'device' else fe.run)([(sig, segs)])[0]
    plan = fbank.window_plan(fn, segs, sr, args.seg_len, args.seg_jump)
    emb = [None] * len(plan)
    start = lambda i: rows[plan[i].seg] + plan[i].start
    for part, length in window_batches(plan, args, embed_ragged is not None):
        if length is None:
            y = embed_ragged(fe, [start(i) for i in part], [plan[i].end - plan[i].start for i in part])
        else:
            y = embed(fe, [start(i) for i in part], length)
        for i, v in zip(part, y):
            emb[i] = v
    return [(w.key, w.line, e) for w, e in zip(plan, emb)]


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    import torch
    device = int(args.gpus.split(',')[0])
    if not torch.cuda.is_available() or device >= torch.cuda.device_count():
        raise SystemExit(f'--gpus {args.gpus}: no such GPU visible to PyTorch')
    if args.checkpoint is not None:
        from . import xvector
        try:
            sd = xvector.load_checkpoint(args.checkpoint, embed_dim=args.embed_dim)
        except (ValueError, OSError) as exc:
            raise SystemExit(f'--checkpoint {args.checkpoint}: {exc}')
        net = xvector.ResNet101(sd, device, gemm=args.gemm)
        del sd
        embed, embed_ragged = net.embed_windows, net.embed_windows_ragged
    else:
        embed_ragged = None
        model = torch.jit.load(args.model_file, map_location=torch.device('cuda', device))
        model.eval()

        def embed(fe, starts, length):
            return model(fe.windows(starts, length, out='torch')).detach().cpu().numpy()
    file_names = [str(f) for f in np.atleast_1d(np.loadtxt(args.in_file_list, dtype=object))]
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    nxt = pool.submit(_read_ahead, args, file_names[0]) if file_names else None
    with torch.no_grad(), open(args.out_seg_fn, 'w') as seg_file, open(args.out_ark_fn, 'wb') as ark_file:
        for k, fn in enumerate(file_names):
            t0 = time.time()
            got = nxt.result()
            nxt = pool.submit(_read_ahead, args, file_names[k + 1]) if k + 1 < len(file_names) else None
            sr, sig, segs = _loaded(args, fn, got, device)
            fe = fbank.front_end(sr, device)
            for key, line, vec in embed_file(embed, fe, fn, sig, segs, sr, args, embed_ragged):
                if np.isnan(vec).any():
                    logger.warning(f'NaN found, not processing: {key}{os.linesep}')
                    continue
                seg_file.write(line + os.linesep)
                ark_file.write(_ark_entry(key, vec))
            logger.info(f'{fn}: {time.time() - t0:.3f} s')
    pool.shutdown()
    return 0


if __name__ == '__main__':
    sys.exit(main())
