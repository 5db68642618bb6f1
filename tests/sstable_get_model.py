"""TEST INFRASTRUCTURE — a plain-Python restatement of the reference's point lookup, and the
record / probe rules of tests/golden/sstable_get.json (tools/gen_golden_get.py writes that
fixture from the REAL reference with these rules; tests/test_sstable_read_cpu.py pins this
model to it).

Restated, linear as the reference is:
* SSTableEncoding.from_bytes (src/sstable.py:88-113) and MetaBlock.from_bytes (blocks.py:142-151);
* SSTable.find_block_id (sstable.py:150-159): the first meta block whose last_key >= key holds
  the key iff its first_key <= key;
* DataBlock.from_bytes / get (blocks.py:40-65) over Record._from_bytes (record.py:74-85): the
  first record of the block whose key equals the probe;
* LsmStorage.get's walk over the SSTables (lsm_storage.py:164-179), the bloom decisions given
  by the caller (one bool array per table).
"""
from __future__ import annotations

import struct

# ----------------------------------------------------------------------------- the model


class ModelTable:
    def __init__(self, file_bytes: bytes):
        data = bytes(file_bytes)
        n = len(data)
        meta_offset, bloom_offset = struct.unpack("ii", data[n - 8:])
        self.bloom = data[bloom_offset:n - 8]  # bitmap ‖ k
        self.meta_block_offset = meta_offset
        self.meta_blocks = []  # (first_key, last_key, offset)
        enc = data[meta_offset:bloom_offset]
        while enc:
            fs = struct.unpack("H", enc[0:2])[0]
            first = enc[2:2 + fs].decode("utf-8")
            ls = struct.unpack("H", enc[2 + fs:4 + fs])[0]
            last = enc[4 + fs:4 + fs + ls].decode("utf-8")
            off = struct.unpack("i", enc[4 + fs + ls:8 + fs + ls])[0]
            self.meta_blocks.append((first, last, off))
            enc = enc[8 + fs + ls:]
        self.data = data[:meta_offset]
        self.first_key = self.meta_blocks[0][0]
        self.last_key = self.meta_blocks[-1][1]

    def find_block_id(self, key: str):
        for i, (first, last, _) in enumerate(self.meta_blocks):
            if last < key:
                continue
            if first <= key <= last:
                return i
            if key <= first:
                return None
        return None

    def block_records(self, block_id: int):
        start = self.meta_blocks[block_id][2]
        end = self.meta_blocks[block_id + 1][2] if block_id + 1 < len(self.meta_blocks) else self.meta_block_offset
        blk = self.data[start:end]
        nrec = struct.unpack("H", blk[-2:])[0]
        offs_start = len(blk) - 2 - 2 * nrec
        offsets = struct.unpack("H" * nrec, blk[offs_start:len(blk) - 2])
        for o in offsets:
            ks = struct.unpack("i", blk[o:o + 4])[0]
            key = blk[o + 4:o + 4 + ks].decode("utf-8")
            vs = struct.unpack("i", blk[o + 4 + ks:o + 8 + ks])[0]
            yield key, blk[o + 8 + ks:o + 8 + ks + vs]

    def get(self, key: str):
        b = self.find_block_id(key)
        if b is None:
            return None
        for k, v in self.block_records(b):
            if k == key:
                return v
        return None


def lsm_get(i: int, key: str, level0, levels, hits):
    """LsmStorage.get (lsm_storage.py:164-179) with empty memtables for probe i: (table row or
    -1, value or None, rows read).  level0 / levels hold ModelTables; hits[t][i] = may_contain of
    row t (L0 first, then level by level)."""
    read = []
    for t, sst in enumerate(level0):
        if not hits[t][i]:
            continue
        read.append(t)
        v = sst.get(key)
        if v is not None:
            return t, v, read
    t = len(level0)
    for level in levels:
        for sst in level:
            if sst.first_key <= key <= sst.last_key and hits[t][i]:
                read.append(t)
                v = sst.get(key)
                if v is not None:
                    return t, v, read
            t += 1
    return -1, None, read


# ----------------------------------------------------------------------------- fixture rules
def value_of(i: int, n: int) -> bytes:
    return bytes(((i * 131 + j * 29) & 0xFF) for j in range(n))


SEAM_BASE = "seam-0123456789abcdefghij"  # 25 bytes: seams at bytes 7, 8, 9, 15, 16, 17
SEAMS = (7, 8, 9, 15, 16, 17)


def _swap(s: str, p: int, c: str) -> str:
    return s[:p] + c + s[p + 1:]


def table_records(name: str):
    """(keys ascending, values, block_size) of a single-table case."""
    if name in ("small_blocks", "small_blocks_empty_key"):
        keys = [f"key{3 * i:05d}" for i in range(300 - len(SEAMS) - 1)]
        keys += [SEAM_BASE] + [_swap(SEAM_BASE, p, "Z") for p in SEAMS]
        if name == "small_blocks_empty_key":
            keys[0] = ""
        keys.sort()
        # every 23rd record fills a block alone (8 + key + 230 > 256 - the smallest record)
        vals = [value_of(i, 230 if i % 23 == 11 else (i * 7) % 41) for i in range(len(keys))]
        return keys, vals, 256
    if name == "exact_fit":  # tools/gen_golden_sstable.py's shape: every block ends at block_size
        return [f"k{i:07d}" for i in range(40)], [value_of(i, 48) for i in range(40)], 256
    if name == "one_record":
        return ["solo"], [b"v"], 65_536
    raise KeyError(name)


TABLE_CASES = ("small_blocks", "small_blocks_empty_key", "exact_fit", "one_record")


def table_probes(keys, metas) -> list[str]:
    """Every stored key; keys between two blocks, before the first and after the last; strict
    prefixes and one-byte extensions; the empty key; the word-compare seams; non-ASCII keys."""
    p = list(keys)
    for (_, last, _), (first, _, _) in zip(metas, metas[1:]):
        p.append(last + "\x01")            # just after a block's last key
        p.append(first[:-1] + chr(ord(first[-1]) - 1) + "~" if first else "")  # just before the next one's first
    p += ["", " ", "~~~~", keys[-1] + "0", "\x7f"]
    for k in keys[::7]:
        p.append(k[:-1])
        p.append(k + "0")
        p.append(k + "\x00")
    for s in SEAMS:
        p += [_swap(SEAM_BASE, s, "Y"), _swap(SEAM_BASE, s, "Z"), _swap(SEAM_BASE, s, "\x7f"), SEAM_BASE[:s],
              SEAM_BASE[:s + 1]]
    p += ["clé-0001", "é", "key00003é", "\U0001f511", "ключ", "key0000ÿ"]
    return p


# the LSM case: (level, first index, stop, step, version); L0 newest first
LSM_UNIVERSE = 20_000
LSM_BLOCK_SIZE = 1024
LSM_SPECS = (
    (0, 0, 9000, 3, 1), (0, 5000, 16000, 2, 2), (0, 12000, 20000, 5, 3), (0, 100, 2900, 1, 4),
    (1, 0, 6000, 1, 5), (1, 6000, 13000, 1, 6), (1, 13000, 20000, 1, 7),
    (2, 1500, 9000, 1, 8), (2, 8000, 19990, 1, 9), (2, 14242, 14243, 1, 10),
)


def lsm_key(i: int) -> str:
    return f"k{i:05d}"


def lsm_table_records(spec):
    _, a, b, step, ver = spec
    idx = range(a, b, step)
    keys = [lsm_key(i) for i in idx]
    vals = [b"" if (i + ver) % 31 == 0 else value_of(i * 17 + ver, 1 + (i * 5 + ver * 3) % 29) for i in idx]
    return keys, vals


def lsm_probes() -> list[str]:
    p = [lsm_key(i) for i in range(LSM_UNIVERSE)]
    p += [lsm_key(i) + "5" for i in range(LSM_UNIVERSE)]
    p += ["", "0", "zzz", "\U0001f600", "é", "k", "k99999", "k1999"]
    return p
