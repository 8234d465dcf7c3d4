"""Any PCM wav in: decode, downmix and resample to mono int16 at 8 or 16 kHz -- the files ``fbank.read_wav`` takes, made
from the files people have (44.1 or 48 kHz, stereo, 24-bit or float).  DESIGN section 21.

The result is defined in integers, so that the host path, the device path and any other implementation agree bit for bit.

  input     a RIFF/WAVE file: format tag 1 (PCM: 8-bit unsigned, 16-, 24-, 32-bit signed), 3 (IEEE float32) or 0xFFFE
            (EXTENSIBLE) with one of these as its sub-format; 1 to 8 channels; any integer sample rate
  scale     every sample becomes an integer q at 24-bit scale:
              u8   (b - 128) << 16        s16  x << 8        s24  x        s32  x >> 8 (arithmetic: floor)
              f32  NaN -> 0, else clamp(rint_half_even(x 2^23), -2^23, 2^23 - 1)      (the product is exact in f32)
            and the C channels of frame j are summed: X[j] = sum_c q_c[j]
  filter    for sr_in -> sr_out in {8000, 16000}: g = gcd, L = sr_out / g, M = sr_in / g, R = max(L, M), Z = 32, P = Z R,
            beta = 10; at the L-times upsampled rate, for i = -P .. P, in f64:
              h[i]  = (L / R) sinc(i / R) I0(beta sqrt(1 - (i / P)^2)) / I0(beta)
              hq[i] = rint(h[i] 2^24)
            then, for every phase p in [0, L) -- the taps P + i with P + i = p (mod L) --, 2^24 - sum hq of the phase is
            added to the phase's tap of largest |hq| (the lowest index on a tie): every phase sums to exactly 2^24
  output    n_out = ceil(n L / M);  for m in [0, n_out):
              acc[m] = sum_j X[j] hq[P + m M - j L]      over the j in [0, n) with |m M - j L| <= P
              y[m]   = clamp(floor((2 acc + D) / (2 D)), -32768, 32767),  D = C 2^32      (round half up)

|X| <= 2^26 and sum |hq| < 2^26 over a phase (asserted), so every partial sum is an integer below 2^52: the sum is exact in
int64 and in f64, in any order.  At equal rates the prototype is the unit impulse, and a mono s16 file at 8 or 16 kHz comes
out sample for sample as ``fbank.read_wav`` gives it.

    read_audio           (bytes of the data chunk, format, channels, sample rate, frames) by a chunk parser of its own
    resample_filter      L, M, P and hq of a rate pair
    to_mono16            the definition for a batch of recordings of one (format, channels, rate pair): in numpy with int64
                         (device=None) or by the kernel of vbx_resample.hpp (device=N), all recordings in one call
    load_mono16          read_audio + to_mono16 of one file
    python -m vbx_amd.audio   wav files in, mono 16-bit wav files out
"""
from __future__ import annotations

import argparse
import functools
import math
import os
import struct
import sys
import warnings
from dataclasses import dataclass

import numpy as np

from . import fbank

Z, BETA, ONE = 32, 10.0, 1 << 24
MAX_L, MAX_M, MAX_CHANNELS = 640, 1024, 8
FORMATS = {'u8': (0, 1), 's16': (1, 2), 's24': (2, 3), 's32': (3, 4), 'f32': (4, 4)}      # name: (code of the C entry, bytes a sample)
BATCH_BYTES = 1 << 30            # bytes per device call of the command line
TARGETS = (8000, 16000)
_TAG_NAMES = {0: 'unknown', 1: 'PCM', 2: 'ADPCM', 3: 'IEEE float', 6: 'A-law', 7: 'mu-law', 0x11: 'IMA ADPCM', 0x31: 'GSM 6.10', 0x55: 'MPEG layer 3',
              0xFFFE: 'EXTENSIBLE'}
_GUID_TAIL = bytes.fromhex('000000001000800000aa00389b71')      # KSDATAFORMAT_SUBTYPE_*: the tag, then these 14 bytes


# ---- input -------------------------------------------------------------------------------------------------------------
def _tag_name(tag: int) -> str:
    return f'format tag 0x{tag:04X} ({_TAG_NAMES.get(tag, "not PCM")})'


def read_audio(path: str):
    """(bytes, format, channels, sample rate, frames) of a RIFF/WAVE file: the interleaved frames of its ``data`` chunk as a
    uint8 array, as they lie in the file, and format as a key of FORMATS.  Chunks before ``data`` are skipped (with the pad
    byte of an odd size); a ``data`` chunk longer than the file, or not a whole number of frames, is cut to whole frames
    with a warning.  Anything but PCM of 8, 16, 24 or 32 bits and IEEE float32, plain or EXTENSIBLE, of 1 to 8 channels is
    refused with a ValueError that names what was found."""
    raw = np.fromfile(path, dtype=np.uint8)
    head = raw[:12].tobytes()
    if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
        raise ValueError(f'{path}: not a RIFF/WAVE file')
    pos, fmt = 12, None
    while True:
        if pos + 8 > raw.size:
            raise ValueError(f'{path}: no data chunk' if fmt is not None else f'{path}: no fmt chunk')
        cid, size = struct.unpack_from('<4sI', raw, pos)
        pos += 8
        if cid == b'data':
            break
        if cid == b'fmt ':
            body = raw[pos:pos + size].tobytes()
            if len(body) < 16:
                raise ValueError(f'{path}: fmt chunk of {len(body)} bytes, need at least 16')
            tag, ch, sr, _rate, align, bits = struct.unpack_from('<HHIIHH', body, 0)
            if tag == 0xFFFE:
                if len(body) < 40:
                    raise ValueError(f'{path}: EXTENSIBLE fmt chunk of {len(body)} bytes, need 40')
                sub = body[24:40]
                tag = struct.unpack_from('<H', sub, 0)[0]
                if sub[2:] != _GUID_TAIL or tag not in (1, 3):
                    raise ValueError(f'{path}: EXTENSIBLE sub-format {sub.hex()} is not supported: only PCM and IEEE float32')
            fmt = (tag, ch, sr, align, bits)
        pos += size + (size & 1)
    if fmt is None:
        raise ValueError(f'{path}: no fmt chunk before the data chunk')
    tag, ch, sr, align, bits = fmt
    if tag == 1 and bits in (8, 16, 24, 32):
        name = 'u8' if bits == 8 else f's{bits}'
    elif tag == 3 and bits == 32:
        name = 'f32'
    elif tag in (1, 3):
        raise ValueError(f'{path}: {bits}-bit {_TAG_NAMES[tag]} is not supported: only PCM of 8, 16, 24 or 32 bits and IEEE float32')
    else:
        raise ValueError(f'{path}: {_tag_name(tag)} is not supported: only PCM (1), IEEE float32 (3) and EXTENSIBLE (0xFFFE) with one of them')
    if not 1 <= ch <= MAX_CHANNELS:
        raise ValueError(f'{path}: {ch} channels; 1 to {MAX_CHANNELS} are supported')
    if sr <= 0:
        raise ValueError(f'{path}: sample rate {sr}')
    fb = ch * FORMATS[name][1]
    if align != fb:
        raise ValueError(f'{path}: frames of {align} bytes for {ch} channel(s) of {bits} bits; only packed samples ({fb} bytes) are supported')
    have = min(size, raw.size - pos)
    frames = have // fb
    if have != size or frames * fb != size:
        warnings.warn(f'{path}: data chunk of {size} bytes, {have} of them in the file: cut to {frames} whole frames of {fb} bytes')
    return raw[pos:pos + frames * fb], name, ch, sr, frames


# ---- the filter ----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ResampleFilter:
    """L, M, P of a rate pair and the integer prototype hq[0 .. 2P] (int64; hq[P + i] is the tap at i)."""
    sr_in: int
    sr_out: int
    L: int
    M: int
    P: int
    hq: np.ndarray

    @property
    def taps(self) -> int:
        """Taps of a phase (of phase 0; a later phase may have one fewer): what one output sums over."""
        return 2 * self.P // self.L + 1

    def phase_table(self) -> np.ndarray:
        """int32 [L][taps], phase-major, as vbx_resample_pcm takes it: table[p][k] = hq[p + k L], 0 past hq[2P]."""
        K = self.taps
        flat = np.zeros(self.L * K, dtype=np.int32)
        flat[:self.hq.size] = self.hq                            # [k][p]
        return np.ascontiguousarray(flat.reshape(K, self.L).T)


def prototype(L: int, M: int) -> np.ndarray:
    """h[i], i = -P .. P, in f64: the Kaiser-windowed sinc at the L-times upsampled rate, cut off at the lower Nyquist."""
    R = max(L, M)
    P = Z * R
    i = np.arange(-P, P + 1, dtype=np.float64)
    return (L / R) * np.sinc(i / R) * np.i0(BETA * np.sqrt(1.0 - (i / P) ** 2)) / np.i0(BETA)


@functools.lru_cache(maxsize=None)
def resample_filter(sr_in: int, sr_out: int) -> ResampleFilter:
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_out not in TARGETS:
        raise ValueError(f'Only 8kHz and 16kHz are supported as targets. Got {sr_out} instead.')
    if sr_in <= 0:
        raise ValueError(f'sample rate {sr_in}')
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    if L > MAX_L or M > MAX_M:
        raise ValueError(f'{sr_in} Hz -> {sr_out} Hz is {L} / {M} in lowest terms; at most {MAX_L} / {MAX_M} is supported (8, 11.025, 12, 16, '
                         '22.05, 24, 32, 44.1, 48, 88.2, 96, 176.4 and 192 kHz are)')
    P = Z * max(L, M)
    hq = np.rint(prototype(L, M) * ONE).astype(np.int64)
    for p in range(L):
        phase = hq[p::L]                                         # (a view)
        phase[np.argmax(np.abs(phase))] += ONE - int(phase.sum())
    assert all(int(hq[p::L].sum()) == ONE and int(np.abs(hq[p::L]).sum()) < 1 << 26 for p in range(L))
    hq.setflags(write=False)
    return ResampleFilter(sr_in, sr_out, L, M, P, hq)


# ---- the numpy path --------------------------------------------------------------------------------------------------
def decode(data, fmt: str, channels: int) -> np.ndarray:
    """X[j], int64 [frames]: the samples of raw interleaved frames at 24-bit scale, summed over the channels."""
    data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, dtype=np.uint8).reshape(-1)
    width = FORMATS[fmt][1]
    n = data.size // (width * channels)
    data = data[:n * width * channels]
    if fmt == 'u8':
        q = (data.astype(np.int64) - 128) << 16
    elif fmt == 's16':
        q = np.frombuffer(data.tobytes(), dtype='<i2').astype(np.int64) << 8
    elif fmt == 's24':
        b = data.reshape(-1, 3).astype(np.int64)
        q = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        q = q - ((q & 0x800000) << 1)
    elif fmt == 's32':
        q = np.frombuffer(data.tobytes(), dtype='<i4').astype(np.int64) >> 8
    elif fmt == 'f32':
        x = np.frombuffer(data.tobytes(), dtype='<f4').astype(np.float32)
        with np.errstate(invalid='ignore', over='ignore'):
            y = np.clip(np.rint(x * np.float32(1 << 23)), np.float32(-(1 << 23)), np.float32((1 << 23) - 1))
        q = np.where(np.isnan(x), np.float32(0), y).astype(np.int64)
    else:
        raise ValueError(f'format {fmt!r}: one of {", ".join(FORMATS)}')
    return q.reshape(n, channels).sum(axis=1)


def _filter_host(X, channels: int, f: ResampleFilter, block: int = 1 << 20) -> np.ndarray:
    n, L, M, P, K = len(X), f.L, f.M, f.P, f.taps
    n_out = -(-n * L // M)
    table = f.phase_table().astype(np.int64)
    Xp = np.concatenate([np.zeros(K - 1, np.int64), X, np.zeros(P // L + 1, np.int64)])      # frame j at K - 1 + j
    D = channels << 32
    y = np.empty(n_out, dtype=np.int16)
    for m0 in range(0, n_out, block):
        top = P + np.arange(m0, min(m0 + block, n_out), dtype=np.int64) * M
        p, at = top % L, top // L + (K - 1)
        acc = np.zeros(len(top), dtype=np.int64)
        for k in range(K):
            acc += (table[0, k] if L == 1 else table[p, k]) * Xp[at - k]
        y[m0:m0 + len(top)] = np.clip((2 * acc + D) // (2 * D), -32768, 32767)
    return y


# ---- the public calls ------------------------------------------------------------------------------------------------
def _bytes_of(x) -> np.ndarray:
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(x, dtype=np.uint8)
    x = np.asarray(x)
    if x.dtype != np.uint8:
        raise ValueError(f'a recording is its raw bytes (bytes or a uint8 array), got dtype {x.dtype}')
    return x.reshape(-1)


def to_mono16(recordings, fmt: str, channels: int, sr_in: int, sr_out: int, device=None, times=None) -> list:
    """The mono int16 samples at ``sr_out`` of every recording: a list of the raw interleaved frames (bytes or uint8 arrays,
    what read_audio returns first) of one format, channel count and rate.  ``device=None`` computes in numpy with int64,
    ``device=N`` on GPU N, all recordings in one call of vbx_resample_pcm; the two agree bit for bit.  ``times``: a dict
    that receives the device milliseconds ``upload`` and ``kernels`` of that call."""
    if fmt not in FORMATS:
        raise ValueError(f'format {fmt!r}: one of {", ".join(FORMATS)}')
    if not 1 <= int(channels) <= MAX_CHANNELS:
        raise ValueError(f'{channels} channels; 1 to {MAX_CHANNELS} are supported')
    f = resample_filter(sr_in, sr_out)
    code, width = FORMATS[fmt]
    fb = width * int(channels)
    raws = [_bytes_of(x) for x in recordings]
    raws = [x[:x.size // fb * fb] for x in raws]
    if not raws:
        return []
    if device is None:
        return [_filter_host(decode(x, fmt, channels), int(channels), f) for x in raws]
    from . import _capi
    if _capi._lib is None:
        try:                             # (PyTorch-ROCm's HIP runtime first, as fbank.FrontEnd explains)
            import torch  # noqa: F401
        except ImportError:
            pass
    sizes = np.array([x.size for x in raws], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    rec = np.stack([offs[:-1], sizes // fb], axis=1)
    data = raws[0] if len(raws) == 1 else np.concatenate(raws)               # (one recording goes up from where it lies)
    out, ms = _capi.resample_pcm(_capi.default_context(int(device)), data, rec, code, int(channels), f.L, f.M, f.phase_table(),
                                 times=times is not None)
    if times is not None:
        times.update(upload=float(ms[0]), kernels=float(ms[1]))
    ends = np.cumsum(-(-rec[:, 1] * f.L // f.M))
    return [out[b - c:b] for b, c in zip(ends, np.diff(np.concatenate([[0], ends])))]


def load_mono16(path: str, sr_out: int, device=None):
    """(int16 samples, sr_out) of one file of any accepted format: what ``fbank.read_wav(converted, raw=True)`` would give."""
    data, fmt, channels, sr, _frames = read_audio(path)
    return to_mono16([data], fmt, channels, sr, sr_out, device=device)[0], int(sr_out)


def convert_files(paths, sr_out: int, device=None) -> list:
    """The int16 samples at ``sr_out`` of every file, in order: files of one (format, channels, rate) run together, in
    batches of at most BATCH_BYTES."""
    from .vad import batches
    files = [read_audio(p) for p in paths]
    out = [None] * len(files)
    for key in sorted({f[1:4] for f in files}):
        idx = [i for i, f in enumerate(files) if f[1:4] == key]
        for group in batches([files[i][0].size for i in idx], BATCH_BYTES):
            got = to_mono16([files[idx[j]][0] for j in group], *key, sr_out, device=device)
            for j, y in zip(group, got):
                out[idx[j]] = y
    return out


# ---- command line -----------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m vbx_amd.audio', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--in-file-list', required=True, type=str, help='input list of files')
    p.add_argument('--in-wav-dir', required=True, type=str, help='input directory with wavs of any accepted format')
    p.add_argument('--out-wav-dir', required=True, type=str, help='output directory for the mono 16-bit wavs')
    p.add_argument('--rate', type=int, default=16000, choices=TARGETS, help='sample rate of the output')
    p.add_argument('--device', type=int, default=None, metavar='N', help='run on GPU N (default: in numpy on the host)')
    return p


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    try:
        names = [str(f) for f in np.atleast_1d(np.loadtxt(args.in_file_list, dtype=object))]
        got = convert_files([os.path.join(args.in_wav_dir, f'{fn}.wav') for fn in names], args.rate, device=args.device)
    except (ValueError, OSError) as exc:
        ap.error(str(exc))
    os.makedirs(args.out_wav_dir, exist_ok=True)
    for fn, y in zip(names, got):
        fbank.write_wav(os.path.join(args.out_wav_dir, f'{fn}.wav'), y, args.rate)
    return 0


if __name__ == '__main__':
    sys.exit(main())
