"""The referee of vbx_amd.audio: the definition in Python integers and plain loops over outputs and taps,
written from the definition alone -- it imports nothing of vbx_amd -- and a WAV writer of its own for every accepted format.

    filter_table(sr_in, sr_out)      L, M, P, hq (Python ints, hq[P + i] the tap at i) and the f64 prototype h
    decode(data, fmt, C)             X[j] of raw interleaved frames
    resample(X, C, filt)             y[m]
    reference(data, fmt, C, sr_in, sr_out)
    encode(values, fmt)              the bytes of sample values (integers at the format's own scale; floats for f32)
    wav_bytes(...)                   a RIFF/WAVE file: plain or EXTENSIBLE header, chunks before ``data``, odd sizes padded
"""
import math
import struct

import numpy as np

Z, BETA = 32, 10.0
WIDTH = {'u8': 1, 's16': 2, 's24': 3, 's32': 4, 'f32': 4}
FULL_SCALE = {'u8': (0, 255), 's16': (-32768, 32767), 's24': (-(1 << 23), (1 << 23) - 1), 's32': (-(1 << 31), (1 << 31) - 1), 'f32': (-1.0, 1.0)}
PAIRS = [(48000, 16000), (44100, 16000), (11025, 16000), (8000, 16000), (44100, 8000), (16000, 16000)]
_filters = {}


def filter_table(sr_in, sr_out):
    key = (sr_in, sr_out)
    if key not in _filters:
        g = math.gcd(sr_in, sr_out)
        L, M = sr_out // g, sr_in // g
        R = max(L, M)
        P = Z * R
        i = np.arange(-P, P + 1, dtype=np.float64)
        h = (L / R) * np.sinc(i / R) * np.i0(BETA * np.sqrt(1.0 - (i / P) ** 2)) / np.i0(BETA)
        hq = [int(v) for v in np.rint(h * 2.0 ** 24)]
        for p in range(L):
            idx = list(range(p, 2 * P + 1, L))
            best = idx[0]
            for t in idx:
                if abs(hq[t]) > abs(hq[best]):
                    best = t
            hq[best] += (1 << 24) - sum(hq[t] for t in idx)
        _filters[key] = dict(L=L, M=M, P=P, hq=hq, h=h)
    return _filters[key]


def _rint_half_even(v):
    """The integer nearest to the float v, ties to even; v is finite."""
    f = math.floor(v)
    d = v - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        f += 1
    return int(f)


def sample_q(raw: bytes, fmt):
    """One sample's bytes -> q at 24-bit scale."""
    if fmt == 'u8':
        return (raw[0] - 128) << 16
    if fmt == 's16':
        return int.from_bytes(raw, 'little', signed=True) << 8
    if fmt == 's24':
        return int.from_bytes(raw, 'little', signed=True)
    if fmt == 's32':
        return int.from_bytes(raw, 'little', signed=True) >> 8              # (Python's >> floors)
    x = struct.unpack('<f', raw)[0]
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return (1 << 23) - 1 if x > 0 else -(1 << 23)
    return min(max(_rint_half_even(x * 2.0 ** 23), -(1 << 23)), (1 << 23) - 1)     # (x 2^23 is exact in f64 as in f32)


def decode(data: bytes, fmt, C):
    w = WIDTH[fmt]
    n = len(data) // (w * C)
    return [sum(sample_q(data[(j * C + c) * w:(j * C + c + 1) * w], fmt) for c in range(C)) for j in range(n)]


def resample(X, C, filt, clamp=True):
    """y[m]; clamp=False: before the clamp to int16, to see that a test signal does pass the range."""
    L, M, P, hq = filt['L'], filt['M'], filt['P'], filt['hq']
    n = len(X)
    n_out = -(-n * L // M)
    D = C << 32
    y = []
    for m in range(n_out):
        acc = 0
        # the j with |m M - j L| <= P, clipped to the recording
        j_lo = max(-((P - m * M) // L), 0)                    # ceil((m M - P) / L)
        j_hi = min((m * M + P) // L, n - 1)
        for j in range(j_lo, j_hi + 1):
            acc += X[j] * hq[P + m * M - j * L]
        v = (2 * acc + D) // (2 * D)
        y.append(min(max(v, -32768), 32767) if clamp else v)
    return y


def reference(data: bytes, fmt, C, sr_in, sr_out):
    return resample(decode(bytes(data), fmt, C), C, filter_table(sr_in, sr_out))


# ---- writing -------------------------------------------------------------------------------------------------------------
def encode(values, fmt) -> bytes:
    """Interleaved sample values -> bytes: u8 takes 0 .. 255, the signed formats their own range, f32 floats."""
    if fmt == 'u8':
        return bytes(int(v) for v in values)
    if fmt == 'f32':
        return b''.join(struct.pack('<f', float(v)) for v in values)
    return b''.join(int(v).to_bytes(WIDTH[fmt], 'little', signed=True) for v in values)


def random_values(rng, fmt, count, sigma=0.2):
    """count Gaussian sample values of the format, sigma as a share of full scale, clipped to the range."""
    x = np.clip(rng.standard_normal(count) * sigma, -1.0, 1.0)
    if fmt == 'f32':
        return [float(np.float32(v)) for v in x]
    if fmt == 'u8':
        return [int(v) for v in np.clip(np.rint(x * 127) + 128, 0, 255)]
    lo, hi = FULL_SCALE[fmt]
    return [int(min(max(round(v * hi), lo), hi)) for v in x]


def random_bytes(seed, fmt, C, n, sigma=0.2) -> bytes:
    return encode(random_values(np.random.default_rng(seed), fmt, n * C, sigma), fmt)


def wav_bytes(data: bytes, fmt, C, sr, extensible=False, before=(), data_size=None, tag=None, bits=None, align=None) -> bytes:
    """A RIFF/WAVE file.  before: (id, payload) chunks between ``fmt `` and ``data`` (an odd payload gets its pad byte).
    data_size: what the data chunk's header claims (default: the truth).  tag / bits / align: override the header fields."""
    w = WIDTH[fmt]
    base = 3 if fmt == 'f32' else 1
    bits = 8 * w if bits is None else bits
    align = C * w if align is None else align

    def chunk(cid, body):
        return cid + struct.pack('<I', len(body)) + body + (b'\0' if len(body) & 1 else b'')
    if extensible:
        sub = struct.pack('<H', base if tag is None else tag) + bytes.fromhex('000000001000800000aa00389b71')
        body = struct.pack('<HHIIHH', 0xFFFE, C, sr, sr * align, align, bits) + struct.pack('<HHI', 22, bits, (1 << C) - 1) + sub
    else:
        body = struct.pack('<HHIIHH', base if tag is None else tag, C, sr, sr * align, align, bits)
    out = b'WAVE' + chunk(b'fmt ', body) + b''.join(chunk(cid, payload) for cid, payload in before)
    out += b'data' + struct.pack('<I', len(data) if data_size is None else data_size) + data + (b'\0' if len(data) & 1 else b'')
    return b'RIFF' + struct.pack('<I', len(out)) + out
