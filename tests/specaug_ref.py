"""Reference of the spec-augment-layer's masks (kf_ops.h kf_specaug_rows /
kf_specaug_apply): Kaldi's GeneralDropoutComponent with specaugment-max-proportion followed by
its SpecAugmentTimeMaskComponent, restated in numpy on dropout_ref.philox4x32_10.

  X(b, kind, i) = word i % 4 of Philox(counter {step, 0x80000000 | (2k + kind), b, i // 4},
                                       key = the seed's low and high words)
  u24(x) = x >> 8, randint(x, n) = (u24(x) n) >> 24
  band of sequence b:  count = randint(X(b,0,0), Z + 1), start = randint(X(b,0,1), D - count + 1)
  time mask (z > 0):   region 0 zeroed iff float32(u24(X(b,1,0))) 2^-24 < float32(z); region r
                       zeroed iff that XOR (r odd); len_r = 1 + randint(X(b,1,1 + r), m or m_n)
"""
import math

import numpy as np

from dropout_ref import philox4x32_10

_U32 = 0xFFFFFFFF


def max_bins(D: int, f: float) -> int:
    """Z = min(D, floor(D f + 0.5))"""
    return min(D, int(math.floor(D * float(f) + 0.5)))


def max_kept(m: int, z: float) -> int:
    """m_n = max(1, floor(m (1 - z) / z)) in double (capped at 2^31 - 1); 1 when z = 0 (unused)"""
    if not z > 0:
        return 1
    return int(min(2 ** 31 - 1, max(1.0, math.floor(float(m) * (1.0 - float(z)) / float(z)))))


def draws(seed: int, step: int, k: int, b: int, kind: int, i0: int, n: int) -> np.ndarray:
    """X(b, kind, i) for i in [i0, i0 + n) as Python-int-safe uint64"""
    i = np.arange(i0, i0 + n, dtype=np.uint64)
    ctr = np.stack([np.full_like(i, step & _U32), np.full_like(i, 0x80000000 | (2 * k + kind)), np.full_like(i, b),
                    i // np.uint64(4)], axis=-1)
    x = philox4x32_10(ctr, np.array([seed & _U32, (seed >> 32) & _U32], np.uint64))
    return x[np.arange(n), (i % np.uint64(4)).astype(np.int64)].astype(np.uint64)


def randint(x, n: int):
    return ((np.asarray(x, np.uint64) >> np.uint64(8)) * np.uint64(n)) >> np.uint64(24)


def band(seed, step, k, b, D, Z):
    """(start, count) of sequence b"""
    x = draws(seed, step, k, b, 0, 0, 2)
    count = int(randint(x[0], Z + 1))
    start = int(randint(x[1], D - count + 1))
    return start, count


def regions(seed, step, k, b, length, z, m, m_n):
    """[(first frame, frames, zeroed)] tiling [0, length): the time mask of sequence b (z > 0)"""
    first = bool(np.float32(int(draws(seed, step, k, b, 1, 0, 1)[0]) >> 8) * np.float32(2.0 ** -24) < np.float32(z))
    out, t, r = [], 0, 0
    while t < length:
        x = draws(seed, step, k, b, 1, 1 + r, 64)      # a batch of region draws
        for j in range(64):
            zeroed = first ^ bool((r + j) & 1)
            ln = 1 + int(randint(x[j], m if zeroed else m_n))
            ln = min(ln, length - t)                   # the last region is clipped
            out.append((t, ln, zeroed))
            t += ln
            if t >= length:
                break
        r += 64
    return out


def specaug_rows(seed, step, k, seq_row0, D, Z, z, m, m_n) -> np.ndarray:
    """row_band int32 [T]: -1 for a zeroed frame, else start | count << 16 of its sequence"""
    so = [int(v) for v in seq_row0]
    rows = np.empty(so[-1], np.int32)
    for b in range(len(so) - 1):
        start, count = band(seed, step, k, b, D, Z)
        seg = rows[so[b]:so[b + 1]]
        seg[:] = start | (count << 16)
        if z > 0:
            for t0, ln, zeroed in regions(seed, step, k, b, so[b + 1] - so[b], z, m, m_n):
                if zeroed:
                    seg[t0:t0 + ln] = -1
    return rows


def specaug_apply(x: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """the select on the bit patterns of fp16 x [T x D]: +0 on zeroed rows and inside the band"""
    u = np.ascontiguousarray(x).view(np.uint16).copy()
    rows = np.asarray(rows, np.int32)
    start, count = rows & 0xFFFF, rows >> 16
    c = np.arange(u.shape[1])[None, :]
    zero = (rows[:, None] == -1) | ((c >= start[:, None]) & (c < (start + count)[:, None]))
    u[zero] = 0
    return u.view(np.float16)
