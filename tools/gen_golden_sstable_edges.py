"""Golden SSTable files at the data-block encoder's limits, from the REAL reference's
SSTableBuilder (build container only):

    python tools/gen_golden_sstable_edges.py

Writes tests/golden/sstable_build_edges.json.  Same recipe as tools/gen_golden_sstable.py (the
reference's ``SSTableBuilder.add`` / ``build``, src/sstable.py:209-288), other record sets: a
block of exactly 65536 data bytes, a record that misses that by two bytes, one record filling a
block alone, a 65522-byte key of four-byte code points, the 8192-record block (81922 encoded
bytes, the most a block can hold), 12-byte blocks, and keys of 1..4-byte code points at every
16-byte residue.  Inputs are given by rule (``records``: a Python expression the tests evaluate
again); files as length, sha256, data-section length and block offsets; a meta block's key longer
than 64 characters as its sizes and sha256.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "sstable_build_edges.json")
sys.path.insert(0, HERE)

from gen_golden_sstable import build  # noqa: E402  (drives the reference's SSTableBuilder)

# keys of 0..40 characters drawn from a 1-, 2-, 3- and 4-byte code point; every fourth key has
# no one-byte character at all
UTF8_MIX = ("[(''.join('a\\u00e9\\u2713\\U0001f511'[(i * 7 + j * 3 + j // 4) % 4 if i % 4 != 3 else 1 + (i + j) % 3] "
            "for j in range(i % 41)), bytes([i & 255]) * (i % 5)) for i in range(246)]")

CASES = [
    {"name": "full_4096x16", "block_size": 65536, "records": "[(f'{i:04x}', b'abcd') for i in range(4101)]"},
    {"name": "off_by_one", "block_size": 65536,
     "records": "[(f'{i:04x}', b'abcd') for i in range(4095)] + [('zzzzz', b'abcd'), ('zzzzzz', b'abcd')]"},
    # one byte under the limit: 4095 * 16 + 15 = 65535, the next record opens block 2
    {"name": "one_under_full", "block_size": 65536,
     "records": "[(f'{i:04x}', b'abcd') for i in range(4095)] + [('zzz', b'abcd'), ('z', b'')]"},
    {"name": "one_big_value","block_size": 65536, "records": "[('a', b'x'), ('b', bytes(65527)), ('c', b'x')]"},
    {"name": "big_unicode_key", "block_size": 65536,
     "records": "[('a', b'x'), ('\\U0001f511' * 16380 + 'zz', b''), ('\\U0001f512', b'')]"},
    {"name": "max_count", "block_size": 65536, "records": "[('', b'')] * 8192 + [('a', b'')]"},
    {"name": "bs8_empty", "block_size": 8, "records": "[('', b'')] * 5"},
    {"name": "utf8_mix", "block_size": 256, "records": UTF8_MIX},
]


def residues(keys):
    """(start offsets mod 16, end offsets mod 16, continuation-byte positions mod 16) of the
    keys packed back to back."""
    starts, ends, conts, at = set(), set(), set(), 0
    for k in keys:
        b = k.encode("utf-8")
        starts.add(at % 16)
        ends.add((at + len(b)) % 16)
        conts.update((at + j) % 16 for j, c in enumerate(b) if c & 0xC0 == 0x80)
        at += len(b)
    return starts, ends, conts


def key_entry(k: str):
    if len(k) <= 64:
        return k
    b = k.encode("utf-8")
    return {"chars": len(k), "bytes": len(b), "sha256": hashlib.sha256(b).hexdigest()}


def main() -> None:
    cases = []
    for c in CASES:
        recs = eval(c["records"])
        keys, vals = [k for k, _ in recs], [v for _, v in recs]
        if c["name"] == "utf8_mix":
            full = set(range(16))
            assert residues(keys) == (full, full, full)
            assert {len(k) for k in keys} == set(range(41))
            assert any(k and all(ord(ch) > 127 for ch in k) for k in keys)
        data, metas, meta_off = build(keys, vals, c["block_size"])
        metas = [{"first_key": key_entry(m["first_key"]), "last_key": key_entry(m["last_key"]), "offset": m["offset"]}
                 for m in metas]
        cases.append(dict(c, file_len=len(data), file_sha256=hashlib.sha256(data).hexdigest(), meta_blocks=metas,
                          meta_block_offset=meta_off))
        print(c["name"], len(data), "bytes,", meta_off, "data bytes,", len(metas), "blocks")
    with open(OUT, "w") as f:
        json.dump({"generator": "tools/gen_golden_sstable_edges.py (reference SSTableBuilder)", "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
