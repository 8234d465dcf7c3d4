"""The referee of ``--init random_N``, written from its definition and from nothing else: numpy's Philox
generator and Python integers.  No import from vbx_amd.

    key    = [seed, FNV-1a-64(name.encode('utf-8'))]
    w[t]   = np.random.Philox(key=key, counter=[0, r, 0, 0]).random_raw(T)[t]
           = word t % 4 of the Philox4x64-10 block with counter [t // 4 + 1, r, 0, 0]
    label  = (w[t] * N) >> 64
    winner = the restart with the largest final ELBO, the lowest among equals, never a nan; 0 if all are nan
"""
import numpy as np

MASK = (1 << 64) - 1
FNV_OFFSET, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3
PHILOX_M0, PHILOX_M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
PHILOX_W0, PHILOX_W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


def fnv1a64(data: bytes) -> int:
    h = FNV_OFFSET
    for byte in data:
        h = ((h ^ byte) * FNV_PRIME) & MASK
    return h


def name_hash(name: str) -> int:
    return fnv1a64(name.encode('utf-8'))


def words(seed, h, restart, T):
    """The T 64-bit words of restart ``restart`` as Python integers, from numpy's generator."""
    bg = np.random.Philox(key=np.array([seed, h], dtype=np.uint64), counter=np.array([0, restart, 0, 0], dtype=np.uint64))
    return [int(w) for w in bg.random_raw(T)]


def labels(seed, name, restart, T, N):
    """int64 [T] in [0, N): the initial labels of restart ``restart`` of the recording ``name``."""
    return labels_hashed(seed, name_hash(name), restart, T, N)


def labels_hashed(seed, h, restart, T, N):
    return np.array([(w * N) >> 64 for w in words(seed, h, restart, T)], dtype=np.int64)


def philox4x64_10(counter, key):
    """One block by hand: ten rounds of Philox4x64 on Python integers -> the four output words."""
    c, k = [int(v) & MASK for v in counter], [int(v) & MASK for v in key]
    for _round in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 64) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + PHILOX_W0) & MASK, (k[1] + PHILOX_W1) & MASK]
    return c


def increment(counter):
    """The 256-bit counter plus one, word 0 the least significant (what numpy does before every block)."""
    out, carry = [], 1
    for v in counter:
        v = int(v) + carry
        out.append(v & MASK)
        carry = v >> 64
    return out


def best_restart(final_elbos):
    best = None
    for r, v in enumerate(final_elbos):
        if v != v:
            continue
        if best is None or v > final_elbos[best]:
            best = r
    return 0 if best is None else best
