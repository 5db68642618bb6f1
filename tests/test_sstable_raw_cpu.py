"""tests/sstable_raw.py (the byte-by-byte data sections of the resident-SSTable edge tests) against
the oracle's restatement of the reference's writer, and the properties the 130-table case relies
on.  No device."""
import struct

import numpy as np
import pytest

from oracle import sstable_oracle as so

import sstable_get_model as M
import sstable_raw as R


@pytest.mark.parametrize("name", ["exact_fit", "small_blocks"])
def test_raw_data_section_equals_the_oracle(name):
    keys, vals, bs = M.table_records(name)
    want_data, _, metas = so.data_and_meta(keys, vals, bs)
    blocks = R.split_blocks([k.encode() for k in keys], vals, bs)
    data, off = R.raw_data_section(blocks)
    assert data == want_data
    assert off.dtype == np.uint32 and off.tolist() == [m[2] for m in metas] + [len(want_data)]
    assert [(b[0][0].decode(), b[-1][0].decode()) for b in blocks] == [(m[0], m[1]) for m in metas]
    assert len(blocks) > 5 and sum(len(b) for b in blocks) == len(keys)


def test_key_size_counts_bytes_and_crafted_arrays_are_written_as_given():
    key = "clé".encode()  # 3 characters, 4 bytes
    blk = R.raw_block([(key, b"v")])
    assert blk == struct.pack("<i", 4) + key + struct.pack("<i", 1) + b"v" + struct.pack("<HH", 0, 1)
    assert blk != so.data_blocks(["clé"], [b"v"], 64)[0][2]  # the reference writes key_size = 3
    rec = R.record(b"k", b"")
    assert R.raw_block([rec, rec], offsets=[0, 9, 9], count=7) == rec + rec + struct.pack("<HHHH", 0, 9, 9, 7)
    data, off = R.join_blocks([b"abc", b"", b"z"])
    assert data == b"abcz" and off.tolist() == [0, 3, 3, 4]
    assert R.key_prefix(b"") == 0 and R.key_prefix(b"a") == R.key_prefix(b"a\0") == 0x61 << 56
    assert R.key_prefix(b"\x80" * 9) == 0x8080808080808080
    pk = R.pack_bytes([b"", b"\xff\x00", b"a"])
    assert pk.offsets.tolist() == [0, 0, 2, 3] and [pk.key(i) for i in range(3)] == [b"", b"\xff\x00", b"a"]


def test_locate_equals_the_model(oracle):
    from test_sstable_read_cpu import reference_file
    keys, vals, bs = M.table_records("small_blocks_empty_key")
    m = M.ModelTable(reference_file(oracle, keys, vals, bs))
    for k in keys[::5] + ["", "nope", keys[3] + "0"]:
        at = R.locate(m, k)
        v = m.get(k)
        assert (at is None) == (v is None)
        if at is not None:
            assert m.data[at[0]:at[0] + at[1]] == v


def test_many_table_rows_hold_what_the_case_needs():
    rows = R.many_table_rows()
    assert len(rows) == R.MANY_ROWS == 130
    assert all(6 <= len(r) <= 12 for r in rows)
    assert all(8 + len(k) + len(v) <= 64 for r in rows for k, v in r.items())
    where = {i: tuple(r for r in range(130) if R.many_key(i) in rows[r]) for i in range(R.MANY_UNIVERSE)}
    for i, rs in R.MANY_SPECIAL.items():
        assert where[i] == rs
    for only in (0, 63, 64, 127, 128, 129):
        assert sum(1 for rs in where.values() if rs == (only,)) >= 2
    assert sum(1 for rs in where.values() if not rs) >= 30
    assert sum(1 for rs in where.values() if len(rs) >= 2) >= 40
    # one key's values differ in length from row to row
    for i, rs in where.items():
        assert len({len(rows[r][R.many_key(i)]) for r in rs}) == len(rs)
    # rows 70..127: disjoint ascending key ranges (a well-formed level)
    spans = [(min(rows[r]), max(rows[r])) for r in range(R.MANY_L0, 128)]
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))
    assert R.first_row(rows, R.many_key(53)) == 63 and R.first_row(rows, R.many_key(9)) == -1
    keep = [None] * 130
    keep[63] = False
    assert R.first_row(rows, R.many_key(53), keep) == 64
