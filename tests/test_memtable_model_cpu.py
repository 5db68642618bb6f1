"""tests/memtable_model.py (the GPU memtable-flush tests' oracle) pinned to the REAL reference's
flushes (tests/golden/memtable_flush.json, tools/gen_golden_memtable.py: MemTable.put,
create_from_wal, MemTableIterator, SSTableBuilder as _do_flush): the run's record count, key,
value and put-index hashes, the WAL's bytes and — through the oracle restatement of the SSTable
encoding and the C bloom oracle — the flushed file.  Then the host half of the feature:
PackedRecords.from_wal and the argument checks of pbf_log_sort that come before any device call."""
import ctypes
import hashlib
import json
import os
import re
import struct

import numpy as np
import pytest

from oracle import sstable_oracle as so
from oracle.oracle import sizing
from pebbledb_amd import _native, memtable
from pebbledb_amd.keys import PackedKeys, PackedRecords

import memtable_model as MT

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "memtable_flush.json")
CASES = json.load(open(GOLDEN))["cases"]
IDS = [c["name"] for c in CASES]
vp = ctypes.c_void_p


def test_golden_holds_the_models_cases():
    """The fixture was generated from the rules the model states now."""
    keys = ("name", "n", "seed", "key", "vlen", "block_size")
    assert [{k: c[k] for k in keys} for c in CASES] == [{k: c[k] for k in keys} for c in MT.CASES]
    assert any(c["n"] > 2 * memtable.SORT_TILE for c in CASES) and any(c["records"] == 1 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_matches_reference(oracle, case):
    puts = MT.case_puts(case)
    wal = MT.wal_bytes(puts)
    assert (len(wal), hashlib.sha256(wal).hexdigest()) == (case["wal_len"], case["wal_sha256"])
    run = MT.flush_run(puts)
    assert len(run) == case["records"]
    assert MT.stream_hashes(run) == (case["keys_sha256"], case["values_sha256"])
    assert MT.index_hash(i for _, _, i in run) == case["index_sha256"]
    ks, vs = [k.decode() for k, _, _ in run], [v for _, v, _ in run]
    nb, k = sizing(len(ks), 0.001)
    f = so.sstable_file(ks, vs, case["block_size"], oracle.build(nb, k, PackedKeys.from_strs(ks)), k)
    assert (len(f), hashlib.sha256(f).hexdigest()) == (case["sst_len"], case["sst_sha256"])


def records_of(pr):
    """[(key bytes, value bytes)] of a PackedRecords."""
    kb, vb = pr.keys.data.tobytes(), np.asarray(pr.values).tobytes()
    ko = pr.keys.offsets if pr.keys.offsets is not None else np.arange(pr.n + 1, dtype=np.uint64) * pr.keys.key_len
    vo = pr.value_offsets
    assert len(ko) == len(vo) == pr.n + 1 and int(ko[-1]) == len(kb) and int(vo[-1]) == len(vb)
    return [(kb[int(ko[i]):int(ko[i + 1])], vb[int(vo[i]):int(vo[i + 1])]) for i in range(pr.n)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_from_wal_is_the_puts_in_order(case):
    """Log order, duplicate keys kept; bytes, bytearray and memoryview streams alike."""
    puts = MT.case_puts(case)
    wal = MT.wal_bytes(puts)
    want = [(k.encode(), v) for k, v in puts]
    for stream in (wal, bytearray(wal), memoryview(wal)):
        pr = PackedRecords.from_wal(stream)
        assert pr.n == case["n"] and pr.ascii and records_of(pr) == want
    same = PackedRecords.from_encoded([struct.pack("<i", len(k)) + k + struct.pack("<i", len(v)) + v for k, v in want])
    assert records_of(same) == want and same.keys.key_len == PackedRecords.from_wal(wal).keys.key_len


def test_from_wal_empty_and_flags():
    pr = PackedRecords.from_wal(b"")
    assert pr.n == 0 and records_of(pr) == [] and list(pr.value_offsets) == [0]
    puts = [("é", b"x"), ("", b""), ("é", b"")]
    pr = PackedRecords.from_wal(MT.wal_bytes(puts))
    # (the model writes key_size in bytes; the reference's character count is why such a log is refused)
    assert not pr.ascii and records_of(pr) == [(k.encode(), v) for k, v in puts]
    with pytest.raises(UnicodeDecodeError):
        PackedRecords.from_wal(struct.pack("<i", 2) + b"\xc3\x28" + struct.pack("<i", 0))
    with pytest.raises(TypeError):
        PackedRecords.from_wal("not bytes")


TORN_PUTS = [("first", b"0123456789"), ("second-key", b"abcdef"), ("k3", b"")]


def torn_cases():
    wal = MT.wal_bytes(TORN_PUTS)
    r0 = 4 + 5 + 4 + 10  # the first record's length = the second one's offset
    r1 = r0 + 4 + 10 + 4 + 6
    assert len(wal) == r1 + 4 + 2 + 4
    return [
        ("first_header", wal[:3], 0, "header"),
        ("inside_a_key", wal[:4 + 2], 0, "key"),
        ("first_value_size", wal[:4 + 5 + 1], 0, "value size"),
        ("inside_a_value", wal[:r0 - 1], 0, "value"),
        ("second_header", wal[:r0 + 2], r0, "header"),
        ("second_key", wal[:r0 + 4 + 9], r0, "key"),
        ("second_value", wal[:r1 - 3], r0, "value"),
        ("last_value_size", wal[:r1 + 4 + 2 + 1], r1, "value size"),
    ]


@pytest.mark.parametrize("name,stream,offset,part", torn_cases(), ids=[c[0] for c in torn_cases()])
def test_torn_stream_is_refused_with_the_offset(name, stream, offset, part):
    with pytest.raises(ValueError, match=rf"byte offset {offset} .*torn.* inside its {part}$"):
        PackedRecords.from_wal(stream)


def test_negative_size_is_refused_with_the_offset():
    wal = MT.wal_bytes(TORN_PUTS)
    r0 = 23
    for bad in (wal[:r0] + struct.pack("<i", -1) + wal[r0 + 4:],                  # key size of record 1
                wal[:r0 + 14] + struct.pack("<i", -6) + wal[r0 + 18:]):           # its value size
        with pytest.raises(ValueError, match=rf"negative key or value size .* byte offset {r0} "):
            PackedRecords.from_wal(bad)
    assert PackedRecords.from_wal(wal).n == 3


def test_cases_tell_a_broken_comparator():
    """What the GPU cases must catch, shown on the model: without the put-index tiebreak (any put
    of a key may come last in its group: here the first) the same-key and duplicate cases change;
    taking a tie on the zero-padded 8-byte prefix as equality merges "a" with "a\\x00"."""
    def first_put_wins(puts):
        first = {}
        for i, (k, v) in enumerate(puts):
            first.setdefault(MT._b(k), (v, i))
        return [(k, v, i) for k, (v, i) in sorted(first.items())]

    def prefix_is_the_key(puts):
        last = {}
        for i, (k, v) in enumerate(puts):
            last[MT._b(k)[:8].ljust(8, b"\0")] = (MT._b(k), v, i)
        return [(k, v, i) for _, (k, v, i) in sorted(last.items())]

    by = {c["name"]: MT.case_puts(c) for c in MT.CASES}
    for name in ("same_key", "dups_one_tile", "dups_three_tiles"):
        good, bad = MT.flush_run(by[name]), first_put_wins(by[name])
        assert [k for k, _, _ in good] == [k for k, _, _ in bad] and MT.stream_hashes(good)[1] != MT.stream_hashes(bad)[1]
        assert MT.index_hash(i for _, _, i in good) != MT.index_hash(i for _, _, i in bad)
    nul = [("a", b"1"), ("a\x00", b"2"), ("a\x00\x00", b"3")]
    assert [k for k, _, _ in MT.flush_run(nul)] == [b"a", b"a\x00", b"a\x00\x00"]
    assert len(prefix_is_the_key(nul)) == 1
    assert len(prefix_is_the_key(by["trailing_nul"])) < len(MT.flush_run(by["trailing_nul"]))


def test_model_semantics_by_hand():
    puts = [("b", b"1"), ("a", b"2"), ("b", b""), ("", b"3"), ("a\x00", b"4"), ("b", b"5"), ("a", b"")]
    assert MT.flush_run(puts) == [(b"", b"3", 3), (b"a", b"", 6), (b"a\x00", b"4", 4), (b"b", b"5", 5)]
    assert MT.index_runs([4, 5, 6, 2, 3, 9]) == [[4, 3], [2, 2], [9, 1]]
    assert MT.wal_bytes(puts[:2]) == b"\x01\0\0\0b\x01\0\0\x001" + b"\x01\0\0\0a\x01\0\0\x002"


def test_constants_agree_with_the_kernels():
    kernels = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "memtable_kernels.hpp")).read()
    read = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sstable_read_kernels.hpp")).read()
    assert re.search(r"kMtTile\s*=\s*kScanTile", kernels)
    threads, per = (int(re.search(rf"{n}\s*=\s*(\d+)", read).group(1)) for n in ("kScanThreads", "kScanPer"))
    assert threads * per == memtable.SORT_TILE == 2048
    assert int(re.search(r"kMtFanIn\s*=\s*(\d+)", kernels).group(1)) == memtable.FAN_IN
    T, F = memtable.SORT_TILE, memtable.FAN_IN
    assert [memtable.merge_passes(n) for n in (0, 1, T, T + 1, F * T, F * T + 1, F * F * T, F * F * T + 1)] == \
        [0, 0, 0, 1, 1, 2, 2, 3]
    stages = int(re.search(r"#define\s+PBF_LOG_SORT_STAGES\s+(\d+)", open(_native.HEADER).read()).group(1))
    assert stages == 8


def log_sort_rc(ko, vo, n, keys=b"", values=b""):
    """pbf_log_sort of a hand-made log with roomy outputs: (rc, message)."""
    ko, vo = np.asarray(ko, dtype=np.uint64), np.asarray(vo, dtype=np.uint64)
    kin, vin = np.frombuffer(keys + b"\0", dtype=np.uint8), np.frombuffer(values + b"\0", dtype=np.uint8)
    out = [np.zeros(64, dtype=np.uint64) for _ in range(4)]
    z = [ctypes.c_uint64() for _ in range(3)]
    L = _native.lib()
    rc = L.pbf_log_sort(0, vp(kin.ctypes.data), vp(ko.ctypes.data), vp(vin.ctypes.data), vp(vo.ctypes.data), n,
                        vp(out[0].ctypes.data), 512, vp(out[1].ctypes.data), vp(out[2].ctypes.data), 512,
                        vp(out[3].ctypes.data), 64, None, *[ctypes.byref(x) for x in z])
    return rc, L.pbf_last_error().decode() if rc else ""


def test_log_sort_refusals_need_no_gpu():
    """The offsets and the count are validated on the host before any launch."""
    inv = _native.PBF_ERR_INVALID
    rc, msg = log_sort_rc([0, 3, 2, 5], [0, 1, 2, 3], 3, b"abcde", b"xyz")
    assert rc == inv and "key offsets must ascend" in msg
    rc, msg = log_sort_rc([0, 2, 3, 5], [0, 2, 1, 3], 3, b"abcde", b"xyz")
    assert rc == inv and "value offsets must ascend" in msg
    rc, msg = log_sort_rc([1, 2, 3, 5], [0, 1, 2, 3], 3, b"abcde", b"xyz")
    assert rc == inv and "key offsets must start at 0" in msg
    rc, msg = log_sort_rc([0, 2, 3, 5], [2, 2, 2, 3], 3, b"abcde", b"xyz")
    assert rc == inv and "value offsets must start at 0" in msg
    rc, msg = log_sort_rc([0, 1, 1 + 2 ** 31], [0, 0, 0], 2)
    assert rc == inv and "2^31" in msg
    rc, msg = log_sort_rc([0, 1, 2], [0, 2 ** 31, 2 ** 31], 2)
    assert rc == inv and "2^31" in msg
    rc, msg = log_sort_rc([0], [0], 2 ** 32 - 1)
    assert rc == inv and "2^32 - 1" in msg
    z = ctypes.c_uint64()
    L = _native.lib()
    assert L.pbf_log_sort(0, None, None, None, None, 0, None, 0, None, None, 0, None, 0, None, ctypes.byref(z),
                          ctypes.byref(z), ctypes.byref(z)) == inv and b"null pointer" in L.pbf_last_error()
    with pytest.raises(ValueError, match="non-ASCII"):
        memtable.sort_log([("clé", b"v")])
