"""TEST INFRASTRUCTURE — data sections written byte by byte, for the resident-SSTable tests that
need tables no builder writes (tests/test_gpu_sstable_read_edges.py): stored keys with bytes
>= 0x80, broken framing, crafted u16 arrays.

The layout is the one stated in the header of pebbledb_amd/csrc/sstable_read_kernels.hpp and in
oracle/sstable_oracle.py: a block is its records back to back (i32 key_size ‖ key ‖ i32
value_size ‖ value, key_size in BYTES), then one u16 offset per record (from the block's start),
then the u16 record count; a data section is its blocks back to back.
tests/test_sstable_raw_cpu.py pins this to the oracle for ASCII keys.

Also here, because they need no device: the record layout of the 130-table case
(`many_table_rows`), the place of a value in a file by the model's rules (`locate`), and
`key_prefix` as the kernel header defines it.
"""
from __future__ import annotations

import struct

import numpy as np

import sstable_get_model as M


def record(key: bytes, value: bytes) -> bytes:
    return struct.pack("<i", len(key)) + key + struct.pack("<i", len(value)) + value


def raw_block(records, offsets=None, count=None) -> bytes:
    """One block.  `records`: (key bytes, value bytes) pairs, or ready record bytes (anything,
    for broken framing).  `offsets` / `count` replace the u16 array / the count the records
    give (a crafted block; the block's length follows the array that is written)."""
    recs = [r if isinstance(r, (bytes, bytearray)) else record(*r) for r in records]
    own, at = [], 0
    for r in recs:
        own.append(at)
        at += len(r)
    offs = own if offsets is None else list(offsets)
    return b"".join(recs) + struct.pack(f"<{len(offs)}H", *offs) + struct.pack("<H", len(offs) if count is None else count)


def join_blocks(blocks) -> tuple[bytes, np.ndarray]:
    """(data section, block_off uint32[nb+1]) of ready block bytes."""
    off = np.zeros(len(blocks) + 1, dtype=np.uint32)
    np.cumsum([len(b) for b in blocks], out=off[1:])
    return b"".join(blocks), off


def raw_data_section(blocks) -> tuple[bytes, np.ndarray]:
    """(data section, block_off uint32[nb+1]); each block a list of (key bytes, value bytes)."""
    return join_blocks([raw_block(b) for b in blocks])


def split_blocks(keys, values, block_size: int):
    """The reference's block rule (a record joins the block while the records' bytes stay within
    block_size), over bytes keys: [[(key, value), ...], ...]."""
    blocks, cur, used = [], [], 0
    for k, v in zip(keys, values):
        size = 8 + len(k) + len(v)
        if cur and used + size > block_size:
            blocks.append(cur)
            cur, used = [], 0
        cur.append((k, v))
        used += size
    blocks.append(cur)
    return blocks


def key_prefix(key: bytes) -> int:
    """The first 8 bytes as a big-endian word, zero-padded (sstable_read_kernels.hpp)."""
    return int.from_bytes(key[:8].ljust(8, b"\0"), "big")


def pack_bytes(keys):
    """PackedKeys in the offsets layout over bytes keys (any byte values)."""
    from pebbledb_amd.keys import PackedKeys
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in keys], out=offs[1:])
    return PackedKeys(np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8), len(keys), offsets=offs)


def locate(model: M.ModelTable, key: str):
    """(offset of the value in the data section, its length) by the model's rules
    (ModelTable.find_block_id, then the first record of the block with that key), or None."""
    b = model.find_block_id(key)
    if b is None:
        return None
    start = model.meta_blocks[b][2]
    end = model.meta_blocks[b + 1][2] if b + 1 < len(model.meta_blocks) else model.meta_block_offset
    blk = model.data[start:end]
    nrec, = struct.unpack("<H", blk[-2:])
    want = key.encode("utf-8")
    for o in struct.unpack(f"<{nrec}H", blk[len(blk) - 2 - 2 * nrec:len(blk) - 2]):
        ks, = struct.unpack("<i", blk[o:o + 4])
        if blk[o + 4:o + 4 + ks] == want:
            vs, = struct.unpack("<i", blk[o + 4 + ks:o + 8 + ks])
            return start + o + 8 + ks, vs
    return None


# ------------------------------------------------------------------ raw handles
class RawTable:
    """A resident table opened straight from a data section: what `sstable_read.lookup` /
    `gather` need of a DeviceSSTable (`_h`, `device`)."""

    def __init__(self, h, device: int, data_len: int):
        self._h, self.device, self.data_len = h, device, data_len

    def close(self) -> None:
        from pebbledb_amd import _native
        h, self._h = self._h, None
        if h is not None:
            assert _native.lib().pbf_sst_close(h) == 0


def open_raw(data: bytes, block_off, device: int = 0) -> RawTable:
    """pbf_sst_open(data_on_device=0) of a data section; ValueError (the library's message) when
    the table is refused.  The caller closes it (the GPU tests' `opened` fixture does)."""
    import ctypes

    from pebbledb_amd import _native
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    off = np.ascontiguousarray(block_off, dtype=np.uint32)
    h = ctypes.c_void_p()
    rc = _native.lib().pbf_sst_open(device, ctypes.c_void_p(buf.ctypes.data), len(data), ctypes.c_void_p(off.ctypes.data),
                                    len(off) - 1, 0, ctypes.byref(h))
    if rc:
        assert h.value is None
    _native.check(rc, "pbf_sst_open")
    return RawTable(h, device, len(data))


# ------------------------------------------------------------------ the 130-table case
MANY_ROWS = 130
MANY_UNIVERSE = 300
MANY_L0 = 70          # rows [0, 70) stand as level 0; rows [70, 128) as one level of disjoint ranges
MANY_SLOT = 5         # row 70 + j holds keys of [5j, 5j + 5) only
# key index -> the rows that store it
MANY_SPECIAL = {3: (0,), 4: (0,), 13: (63,), 14: (63,), 23: (64,), 24: (64,), 285: (127,), 286: (127,),
                33: (128,), 34: (128,), 43: (129,), 44: (129,), 53: (63, 64), 54: (63, 64), 55: (63, 64),
                0: (10, 70, 129), 1: (10, 70, 129)}


def many_key(i: int) -> str:
    return f"t{i:04d}"


def many_value(row: int, i: int) -> bytes:
    """Rows r1 != r2 give one key different lengths unless r1 = r2 (mod 41), and different bytes."""
    return M.value_of(row * 1000 + i, 1 + (row * 5 + i) % 41)


def many_table_rows():
    """130 dicts key -> value (6..12 records each, records of at most 58 bytes).  Keys
    t0000..t0299: MANY_SPECIAL as listed, every index = 9 (mod 10) nowhere, the others in their
    slot's row of [70, 128) and / or up to two rows of level 0 (fixed seed); filler keys
    "tNNNN~RRRq" (one row each, inside the row's slot for rows 70..127) bring every row to at
    least 6 records."""
    rng = np.random.default_rng(130)
    rows = [dict() for _ in range(MANY_ROWS)]
    for i, where in MANY_SPECIAL.items():
        for r in where:
            rows[r][many_key(i)] = many_value(r, i)
    for i in range(MANY_UNIVERSE):
        if i in MANY_SPECIAL or i % 10 == 9:
            continue
        where = set()
        slot_row = MANY_L0 + i // MANY_SLOT
        if slot_row < 128 and rng.random() < 0.6:
            where.add(slot_row)
        where.update(int(x) for x in rng.choice(MANY_L0, size=int(rng.integers(0, 3)), replace=False))
        if rng.random() < 0.04:
            where.add(128 + int(rng.integers(0, 2)))
        lens = set()
        for r in sorted(where):
            v = many_value(r, i)
            if len(rows[r]) < 11 and len(v) not in lens:
                lens.add(len(v))
                rows[r][many_key(i)] = v
    for r, row in enumerate(rows):
        q = 0
        while len(row) < 6:
            base = (r - MANY_L0) * MANY_SLOT + q % MANY_SLOT if MANY_L0 <= r < 128 else (r * 7 + q * 37) % MANY_UNIVERSE
            row[f"{many_key(base)}~{r:03d}{q}"] = many_value(r, 500 + q)
            q += 1
    return rows


def first_row(rows, key, keep=None):
    """The lowest row that stores `key` (and, with `keep`, whose entry keep[row] is None or
    true), or -1: the answer of the get walk."""
    for r, row in enumerate(rows):
        if key in row and (keep is None or keep[r] is None or keep[r]):
            return r
    return -1
