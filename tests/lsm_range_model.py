"""TEST INFRASTRUCTURE — a plain-Python model of the level key-range check of LsmStorage.get
(``first_key <= key <= last_key``, reference src/lsm_storage.py:173) on raw byte strings, and the
C-ABI layouts of ``pbf_key_range_mask`` (include/pebblebloom.h): concatenated bytes + uint64
offsets in, one LSB-first bit mask of ceil(n/8) bytes per table out.

Python compares ``bytes`` as memcmp over the common length, then by length — the kernel's
contract — and for UTF-8 encodings that order is the ``str`` order of the reference's expression
(tests/test_lsm_range_model_cpu.py pins both statements).
"""
from __future__ import annotations

import numpy as np


def range_bits(keys, bounds) -> np.ndarray:
    """bool [T, n]: row t, column i = ``first_t <= key_i <= last_t`` (Python ``bytes`` order)."""
    out = np.zeros((len(bounds), len(keys)), dtype=bool)
    for t, (first, last) in enumerate(bounds):
        out[t] = [first <= k <= last for k in keys]
    return out


def range_bits_ranked(keys, bounds) -> np.ndarray:
    """``range_bits`` for many tables: every string is replaced by its rank in Python's sorted
    order of all the distinct strings of the call (equal strings share a rank), and the ranks are
    compared with numpy."""
    rank = {s: r for r, s in enumerate(sorted({*keys, *(b for pair in bounds for b in pair)}))}
    k = np.fromiter((rank[s] for s in keys), dtype=np.int64, count=len(keys))
    f = np.fromiter((rank[a] for a, _ in bounds), dtype=np.int64, count=len(bounds))
    l = np.fromiter((rank[b] for _, b in bounds), dtype=np.int64, count=len(bounds))
    return (f[:, None] <= k[None, :]) & (k[None, :] <= l[:, None])


def pack_strings(strings, prefix: bytes = b""):
    """(uint8 buffer, uint64 offsets[len + 1]) of byte strings laid end to end behind `prefix`.
    The offsets index the buffer, so offsets[0] = len(prefix): a non-empty prefix gives the
    layout of a window (offsets[0] != 0)."""
    lens = np.fromiter(map(len, strings), dtype=np.int64, count=len(strings))
    offs = np.zeros(len(strings) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    offs += np.uint64(len(prefix))
    buf = np.frombuffer(prefix + b"".join(strings), dtype=np.uint8).copy()
    return buf, offs


def pack_bounds(bounds, prefix: bytes = b""):
    """The 2T bound strings (first_0, last_0, first_1, ...) as ``pack_strings`` packs them."""
    return pack_strings([b for pair in bounds for b in pair], prefix)


def unpack_strings(buf, offs) -> list:
    """The byte strings of a packed (buffer, offsets) pair whose offsets index the buffer."""
    raw = bytes(buf)
    return [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def row_bytes(n: int) -> int:
    return (n + 7) // 8


def pack_mask(bits) -> np.ndarray:
    """uint8 [T, ceil(n/8)] LSB-first, the pad bits of each row's last byte zero."""
    bits = np.asarray(bits, dtype=bool)
    if bits.shape[1] == 0:
        return np.zeros((bits.shape[0], 0), dtype=np.uint8)
    return np.packbits(bits, axis=1, bitorder="little")


def unpack_mask(mask, ntables: int, n: int) -> np.ndarray:
    """bool [T, n] from the flat or [T, ceil(n/8)] mask bytes; pad bits are dropped."""
    m = np.asarray(mask, dtype=np.uint8).reshape(ntables, row_bytes(n))
    if n == 0:
        return np.zeros((ntables, 0), dtype=bool)
    return np.unpackbits(m, axis=1, bitorder="little")[:, :n].astype(bool)


# The UTF-8 length boundaries (1 | 2 | 3 | 4 bytes per code point), no surrogates.
BOUNDARY_CODE_POINTS = (0x0000, 0x007F, 0x0080, 0x07FF, 0x0800, 0xFFFF, 0x10000, 0x10FFFF)


def boundary_strs() -> list:
    """Every boundary code point alone, every ordered pair of them, each behind and in front of
    an ASCII letter, and the empty string: prefixes of one another included."""
    cps = [chr(c) for c in BOUNDARY_CODE_POINTS]
    out = [""] + cps + [a + b for a in cps for b in cps]
    out += ["k" + a for a in cps] + [a + "k" for a in cps] + ["k", "kk"]
    return sorted(set(out))
