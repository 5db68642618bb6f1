"""Edge tests of the SSTable write side: the data-block encoder (k_encode_blocks,
csrc/sstable_kernels.hpp) and its three host doors (pbf_encode_data_blocks, pbf_build_sstable,
pbf_build_sstables).  Everything is bit-exact, against files the REAL reference wrote
(tests/golden/sstable_build_edges.json, compaction_split_edges.json) and the oracle restatement
(oracle/sstable_oracle.py).

What each group enters (DESIGN.md "Write-side edge tests" has the table):
1. golden files through every door — blocks of exactly 65536 / 65535 data bytes, 8192 records
   (a full LDS carve, count and offsets past one byte), one record per block, 12-byte blocks
   (total < head), four-byte code points and continuation bytes at every chunk residue;
2. guard bytes — every (destination alignment, block length 12..45) pair and multi-pass stores,
   with every byte outside the blocks checked;
3. source pointers at odd byte offsets and offset windows whose first offsets are not 0;
4. an empty block inside a host plan, and a grid of 70000 blocks;
5. the device's refusal of an oversized block (the error counter);
6. every host refusal, with the outputs untouched and the filters usable afterwards.
Device plans here are monotonic and in range: the kernel does not guard them."""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

from oracle import sstable_oracle as so
from pebbledb_amd import _native
from pebbledb_amd.bloom_filter import BloomFilter
from pebbledb_amd.keys import PackedKeys, PackedRecords
from pebbledb_amd.sstable_data import (build_sstable, build_sstables, encode_data_blocks, key_offsets, pack_values,
                                       plan_blocks, plan_blocks_native)

from test_compaction_cpu import case_records
from test_sstable_edges_cpu import COMPACTION_CASES, COMPACTION_IDS, SST_CASES, SST_IDS, golden_metas, key_entry

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

vp = ctypes.c_void_p
GUARD = 0xA5
SLACK = 64  # sentinel bytes kept at both ends of a guarded output


# ------------------------------------------------------------------ 1. golden files, every door
def _check_file(case, f, metas):
    assert len(f) == case["file_len"]
    assert hashlib.sha256(bytes(f)).hexdigest() == case["file_sha256"]
    assert [(key_entry(a), key_entry(b), o) for a, b, o in metas] == golden_metas(case)


@pytest.mark.parametrize("case", SST_CASES, ids=SST_IDS)
def test_edge_file_from_lists(case):
    f, metas, _ = build_sstable(case["_keys"], case["_vals"], case["block_size"])
    _check_file(case, f, metas)


@pytest.mark.parametrize("case", SST_CASES, ids=SST_IDS)
def test_edge_file_from_packed_records(case):
    keys, vals = case["_keys"], case["_vals"]
    srcs = [PackedRecords.from_iter(zip(keys, vals))]
    if all(k.isascii() for k in keys):  # encoded records split as Record._from_bytes does
        srcs.append(PackedRecords.from_encoded([so.record_bytes(k, v) for k, v in zip(keys, vals)]))
    for pr in srcs:
        f, metas, _ = build_sstable(pr, block_size=case["block_size"])
        _check_file(case, f, metas)


@pytest.mark.parametrize("case", SST_CASES, ids=SST_IDS)
def test_edge_data_section_host_pointers(case):
    """pbf_encode_data_blocks with host pointers on its own (group 4's full and minimal blocks:
    max_count, full_4096x16, one_big_value, bs8_empty are among the cases)."""
    keys, vals, bs = case["_keys"], case["_vals"], case["block_size"]
    pk = PackedKeys.from_strs(keys)
    vb, vo = pack_values(vals)
    bf, bo = plan_blocks(np.asarray(key_offsets(pk), np.uint64), vo, bs)
    got = encode_data_blocks(pk, vb, vo, bf, bo)
    want, _, _ = so.data_and_meta(keys, vals, bs)
    assert len(got) == case["meta_block_offset"]
    assert got.tobytes() == want


def _check_compaction(case, keys, vals, outs, written):
    assert written == case["records_written"]
    assert len(outs) == len(case["outputs"])
    for (f, metas, bloom), o in zip(outs, case["outputs"]):
        assert len(f) == o["file_len"]
        assert hashlib.sha256(bytes(f)).hexdigest() == o["file_sha256"], o["first_record"]
        assert (bloom.nb_bytes, bloom.nb_hash_functions) == (o["nb_bytes"], o["k"])
        assert (metas[0][0], metas[-1][1]) == (o["first_key"], o["last_key"])
        one, _, _ = build_sstable(keys[o["first_record"]:o["end_record"]], vals[o["first_record"]:o["end_record"]],
                                  case["block_size"])
        assert bytes(one) == bytes(f), o["first_record"]


@pytest.mark.parametrize("case", COMPACTION_CASES, ids=COMPACTION_IDS)
def test_build_sstables_equals_reference_compaction_edges(case):
    keys, vals = case_records(case)
    outs, written = build_sstables(keys, vals, case["max_sstable_size"], case["block_size"])
    _check_compaction(case, keys, vals, outs, written)


def test_split_every_block_from_packed_records():
    """40 outputs from a PackedRecords run: five times the stream pool the filters are dealt from."""
    case = next(c for c in COMPACTION_CASES if c["name"] == "split_every_block")
    keys, vals = case_records(case)
    outs, written = build_sstables(PackedRecords.from_iter(zip(keys, vals)), max_sstable_size=case["max_sstable_size"],
                                   block_size=case["block_size"])
    _check_compaction(case, keys, vals, outs, written)


# ------------------------------------------------------------------ device-pointer helpers
def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _padded(data: np.ndarray, shift: int = 0, pad: int = 48):
    """`data` at byte `shift` of a device allocation with >= `pad` readable bytes after it;
    returns (the allocation, the data's device address)."""
    host = np.full(shift + len(data) + pad, 0x5A, np.uint8)
    host[shift:shift + len(data)] = data
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + shift


def _encode_device(kptr, ko, vptr, vo, n, bf, bo, out_ptr):
    """pbf_encode_data_blocks(on_device = 1); ko / vo / bf / bo are device tensors or addresses."""
    ptr = lambda x: x if isinstance(x, int) else x.data_ptr()  # noqa: E731
    nblocks = len(bf) - 1
    torch.cuda.synchronize()
    return _native.lib().pbf_encode_data_blocks(0, kptr, ptr(ko), vptr, ptr(vo), n, ptr(bf), ptr(bo), nblocks, out_ptr, 1)


def _block_bytes(keys, vals) -> bytes:
    """DataBlock.to_bytes (blocks.py:33-37) of one block's records."""
    recs = [so.record_bytes(k, v) for k, v in zip(keys, vals)]
    offs = np.cumsum([0] + [len(r) for r in recs[:-1]]) if recs else []
    return b"".join(recs) + struct.pack("H" * len(recs), *[int(x) for x in offs]) + struct.pack("H", len(recs))


def _run_guarded(groups, aligns, gap=16):
    """Encode `groups` (one block each: (keys, values)) through device pointers into an output
    filled with GUARD, block i at an ADDRESS that is aligns[i] mod 16, with >= gap sentinel bytes
    between blocks and SLACK at both ends.  Returns (output bytes, positions, expected blocks,
    the blocks' address residues)."""
    keys = [k for g in groups for k in g[0]]
    vals = [v for g in groups for v in g[1]]
    blocks = [_block_bytes(*g) for g in groups]
    bf = np.cumsum([0] + [len(g[0]) for g in groups]).astype(np.uint64)
    size = 2 * SLACK + sum(len(b) + gap + 16 for b in blocks) + 16
    out = torch.full((size,), GUARD, dtype=torch.uint8, device="cuda")
    pos, at = [], SLACK
    for blk, a in zip(blocks, aligns):
        at += gap
        at += (a - (out.data_ptr() + at)) % 16
        pos.append(at)
        at += len(blk)
    assert at + SLACK <= size  # every block, and 64 sentinel bytes after the last, inside the tensor
    bo = np.asarray(pos + [at], np.uint64)
    pk = PackedKeys.from_strs(keys)
    vb, vo = pack_values(vals)
    kt, kptr = _padded(pk.data)
    vt, vptr = _padded(vb)
    rc = _encode_device(kptr, _dev(np.asarray(key_offsets(pk), np.uint64)), vptr, _dev(vo), len(keys), _dev(bf), _dev(bo),
                        out.data_ptr())
    _native.check(rc, "pbf_encode_data_blocks")
    return out.cpu().numpy(), pos, blocks, [(out.data_ptr() + p) % 16 for p in pos]


def _assert_guarded(got, pos, blocks):
    inside = np.zeros(len(got), bool)
    for i, (p, blk) in enumerate(zip(pos, blocks)):
        assert got[p:p + len(blk)].tobytes() == blk, f"block {i} ({len(blk)} bytes at {p})"
        inside[p:p + len(blk)] = True
    stray = np.flatnonzero((got != GUARD) & ~inside)
    assert stray.size == 0, f"{stray.size} byte(s) written outside the blocks, first at {stray[:8].tolist()}"


# ------------------------------------------------------------------ 2. guard bytes
def test_guard_bytes_every_alignment_and_length():
    """One-record blocks of 12..45 bytes (keys of 0..33 bytes, empty values) at every destination
    alignment: totals below `head` (h = total), totals that are whole 16-byte stores, every tail
    length; no byte outside a block changes."""
    groups, aligns = [], []
    for a in range(16):
        for L in range(34):
            groups.append((["".join(chr(97 + (a + L + 3 * j) % 26) for j in range(L))], [b""]))
            aligns.append(a)
    got, pos, blocks, at = _run_guarded(groups, aligns)
    assert at == aligns and sorted({len(b) for b in blocks}) == list(range(12, 46))
    _assert_guarded(got, pos, blocks)


def _multi_record_group(seed, target):
    """Records (ASCII and 2..4-byte code points, values of 0..40 bytes) up to about `target` bytes."""
    rng = np.random.default_rng(seed)
    keys, vals, size = [], [], 0
    while size < target:
        L = int(rng.integers(0, 20))
        k = "".join("aé✓\U0001f511z"[int(x)] for x in rng.integers(0, 5, L))
        v = rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8).tobytes()
        keys.append(k)
        vals.append(v)
        size += 8 + len(k.encode()) + len(v)
    return keys, vals


def test_guard_bytes_multi_record_blocks():
    """Blocks of about 300, 5000 and 20000 bytes at alignments 1, 7 and 15: record offsets past
    one byte, and (20000 bytes = 1250 stores for 512 lanes) a second pass of the store loop."""
    groups, aligns = [], []
    for a in (1, 7, 15):
        for target in (300, 5000, 20000):
            groups.append(_multi_record_group(a * 100000 + target, target))
            aligns.append(a)
    got, pos, blocks, at = _run_guarded(groups, aligns, gap=48)
    assert at == aligns and max(len(b) for b in blocks) > 512 * 16 * 2
    _assert_guarded(got, pos, blocks)


# ------------------------------------------------------------------ 3. source alignment, windows
def _window_records():
    rng = np.random.default_rng(42)
    keys, vals = [], []
    for i in range(400):
        L = int(rng.integers(0, 30))
        k = "".join(chr(97 + int(x)) for x in rng.integers(0, 26, L))
        if i % 7 == 3:
            k += "é\U0001f512✓"
        keys.append(k)
        vals.append(rng.integers(0, 256, int(rng.integers(0, 70)), dtype=np.uint8).tobytes())
    return keys, vals


@pytest.mark.parametrize("kshift,vshift", [(0, 0), (1, 15), (5, 8), (8, 5), (15, 1)])
def test_source_slices_and_offset_windows(kshift, vshift):
    """keys / values passed as slices at odd byte offsets of their allocations (>= 48 readable
    bytes after the last one), the whole run and a window of it (key_offsets + r0,
    value_offsets + r0: first offsets neither 0 nor multiples of 16, block_first relative to the
    window): the data section equals the oracle's over those records."""
    keys, vals = _window_records()
    bs = 256
    pk = PackedKeys.from_strs(keys)
    vb, vo = pack_values(vals)
    ko = np.asarray(key_offsets(pk), np.uint64)
    kt, kptr = _padded(pk.data, kshift)
    vt, vptr = _padded(vb, vshift)
    dko, dvo = _dev(ko), _dev(vo)
    r0 = next(r for r in range(5, len(keys)) if ko[r] % 16 and vo[r] % 16)
    for first in (0, r0):
        bf, bo = plan_blocks(ko[first:], vo[first:], bs)
        assert int(bf[-1]) == len(keys) - first
        want, _, _ = so.data_and_meta(keys[first:], vals[first:], bs)
        assert int(bo[-1]) == len(want)
        out = torch.full((len(want) + 2 * SLACK,), GUARD, dtype=torch.uint8, device="cuda")
        rc = _encode_device(kptr, dko.data_ptr() + 8 * first, vptr, dvo.data_ptr() + 8 * first, len(keys) - first,
                            _dev(bf), _dev(bo), out.data_ptr() + SLACK)
        _native.check(rc, "pbf_encode_data_blocks")
        got = out.cpu().numpy()
        assert got[SLACK:SLACK + len(want)].tobytes() == want, first
        assert (got[:SLACK] == GUARD).all() and (got[SLACK + len(want):] == GUARD).all(), first


# ------------------------------------------------------------------ 4. empty block, large grid
def test_host_plan_with_an_empty_block():
    """pbf_encode_data_blocks accepts r1 == r0: the block encodes as the u16 count 0 alone."""
    keys = ["a", "bb", "clé", "dddd", "", "f"]
    vals = [b"1", b"", b"333", b"4" * 20, b"5", b""]
    pk = PackedKeys.from_strs(keys)
    vb, vo = pack_values(vals)
    first = _block_bytes(keys[:2], vals[:2])
    last = _block_bytes(keys[2:], vals[2:])
    bf = np.array([0, 2, 2, 6], np.uint64)
    bo = np.cumsum([0, len(first), 2, len(last)]).astype(np.uint64)
    got = encode_data_blocks(pk, vb, vo, bf, bo)
    assert got.tobytes() == first + b"\x00\x00" + last


def test_seventy_thousand_minimal_blocks():
    """bs8_empty scaled up: 70000 blocks of one empty record (12 bytes each), a grid past 65535
    workgroups, every destination alignment mod 16 in turn (12 * b)."""
    n = 70000
    pk = PackedKeys(np.zeros(0, np.uint8), n, offsets=np.zeros(n + 1, np.uint64))
    vo = np.zeros(n + 1, np.uint64)
    bf, bo = plan_blocks_native(np.asarray(key_offsets(pk), np.uint64), vo, 8)
    assert len(bf) - 1 == n and int(bo[-1]) == 12 * n
    got = encode_data_blocks(pk, np.zeros(0, np.uint8), vo, bf, bo)
    assert got.tobytes() == (b"\x00" * 10 + b"\x01\x00") * n


# ------------------------------------------------------------------ 5. the device's refusal
def test_device_refuses_an_oversized_block_and_recovers():
    """A device plan whose middle block holds 65537 data bytes: the kernel leaves that block
    unwritten and counts it, the call reports it, the neighbours are written, and the counter
    does not leak into the next call."""
    keys = ["a", "b", "big", "y", "z"]
    vals = [b"1", b"22", bytes(65537 - 8 - 3), b"", b"zz"]
    groups = [(keys[:2], vals[:2]), (keys[2:3], vals[2:3]), (keys[3:], vals[3:])]
    blocks = [_block_bytes(*g) for g in groups]
    assert len(blocks[1]) == 65537 + 4
    pos = [SLACK + 3, SLACK + 3 + len(blocks[0]) + 21]
    pos.append(pos[1] + len(blocks[1]) + 9)
    size = pos[2] + len(blocks[2]) + SLACK
    bf = np.array([0, 2, 3, 5], np.uint64)
    bo = np.asarray(pos + [size - SLACK], np.uint64)
    pk = PackedKeys.from_strs(keys)
    vb, vo = pack_values(vals)
    kt, kptr = _padded(pk.data)
    vt, vptr = _padded(vb)
    dko, dvo, dbf, dbo = _dev(np.asarray(key_offsets(pk), np.uint64)), _dev(vo), _dev(bf), _dev(bo)
    out = torch.full((size,), GUARD, dtype=torch.uint8, device="cuda")
    rc = _encode_device(kptr, dko, vptr, dvo, len(keys), dbf, dbo, out.data_ptr())
    assert rc == _native.PBF_ERR_INVALID
    msg = _native.lib().pbf_last_error().decode()
    assert "1 block(s) exceed" in msg and "not written" in msg
    # the two good blocks are there; the refused block's range, like every other byte, is untouched
    _assert_guarded(out.cpu().numpy(), [pos[0], pos[2]], [blocks[0], blocks[2]])
    # the next valid call succeeds: the counter was reset
    bf2, bo2 = np.array([0, 2], np.uint64), np.asarray([SLACK, SLACK + len(blocks[0])], np.uint64)
    out2 = torch.full((len(blocks[0]) + 2 * SLACK,), GUARD, dtype=torch.uint8, device="cuda")
    rc = _encode_device(kptr, dko, vptr, dvo, 2, _dev(bf2), _dev(bo2), out2.data_ptr())
    assert rc == _native.PBF_OK
    _assert_guarded(out2.cpu().numpy(), [SLACK], [blocks[0]])
    # and so does a host-pointer call on the encoder's own stream
    hb, ho = plan_blocks(np.asarray(key_offsets(pk), np.uint64)[:3], vo[:3], 64)
    small = PackedKeys.from_strs(keys[:2])
    assert encode_data_blocks(small, vb[:int(vo[2])], vo[:3], hb, ho).tobytes() == so.data_and_meta(keys[:2], vals[:2], 64)[0]


# ------------------------------------------------------------------ 6. host refusals
COVER = "block plan must cover records [0, n) from byte 0"
COVER_W = "block plan must cover records [0, written) from byte 0"
MONO = "block plan not monotonic"
INCR = "block plan not increasing"
OVER = "a block's records exceed 65536 bytes"
SIZES = "block_out does not match the blocks' encoded sizes"
NULL = "null pointer"
START = "offsets must start at 0"


def _valid_args():
    """Six records in three blocks of two (block size 32), two tables (blocks [0, 2) and [2, 3))."""
    keys = [f"k{i}" for i in range(6)]
    vals = [b"v" * i for i in range(6)]
    pk = PackedKeys.from_strs(keys)
    v, vo = pack_values(vals)
    ko = np.asarray(key_offsets(pk), np.uint64).copy()
    bf, bo = plan_blocks(ko, vo, 32)
    assert bf.tolist() == [0, 2, 4, 6]
    return dict(k=pk.data.copy(), ko=ko, v=v.copy(), vo=vo.copy(), n=6, bf=bf.copy(), bo=bo.copy(), nblocks=3,
                tb=np.array([0, 2, 3], np.uint64)), so.data_and_meta(keys, vals, 32)[0]


def _set(name, index, value):
    def f(a):
        a[name] = a[name].copy()
        a[name][index] = value
    return f


def _bump(name, index, by):
    def f(a):
        a[name] = a[name].copy()
        a[name][index] = int(a[name][index]) + by
    return f


def _null(name):
    def f(a):
        a[name] = None
    return f


def _huge_values(a):  # values of 40000 bytes: every block of two records holds 80000+
    a["v"] = np.zeros(6 * 40000, np.uint8)
    a["vo"] = (np.arange(7) * 40000).astype(np.uint64)


def _decreasing(a):  # block 0 = records [0, 4) with its true size, then block 1 runs backwards
    a["bf"] = np.array([0, 4, 2, 6], np.uint64)
    dl = int(a["ko"][4] + a["vo"][4]) + 8 * 4
    a["bo"] = np.array([0, dl + 2 * 4 + 2, 0, 0], np.uint64)


def _empty_block(a):  # r1 == r0 in the middle, sizes consistent
    a["bf"] = np.array([0, 2, 2, 6], np.uint64)
    d0 = int(a["ko"][2] + a["vo"][2]) + 16
    d2 = int(a["ko"][6] - a["ko"][2] + a["vo"][6] - a["vo"][2]) + 32
    a["bo"] = np.cumsum([0, d0 + 6, 2, d2 + 10]).astype(np.uint64)


def _beyond_n(a):  # an interior entry past n: refused before any offset is read through it
    a["bf"] = np.array([0, 2, 6 + 1000, 6], np.uint64)


PLAN_REFUSALS = [  # (id, mutation, message of encode / build_sstable, message of build_sstables)
    ("first_not_0", _set("bf", 0, 1), COVER, COVER_W),
    ("last_past_n", _set("bf", 3, 7), COVER, COVER_W),
    ("last_short_of_n", _set("bf", 3, 5), COVER, SIZES),  # a compaction plan may end early: its sizes must still fit
    ("out_not_0", _set("bo", 0, 1), COVER, COVER_W),
    ("decreasing", _decreasing, MONO, INCR),
    ("entry_beyond_n", _beyond_n, MONO, INCR),
    ("over_65536", _huge_values, OVER, OVER),
    ("out_plus_1", _bump("bo", 2, 1), SIZES, SIZES),
    ("out_minus_1", _bump("bo", 2, -1), SIZES, SIZES),
    ("null_key_offsets", _null("ko"), NULL, NULL),
    ("null_block_out", _null("bo"), NULL, NULL),
]
PLAN_IDS = [r[0] for r in PLAN_REFUSALS]


def _p(a):
    return vp(a.ctypes.data) if a is not None else None


def _refused(rc, message):
    assert rc == _native.PBF_ERR_INVALID
    assert message in _native.lib().pbf_last_error().decode()


def _still_usable(*filters):
    for i, f in enumerate(filters):
        f.add(f"probe{i}")
        assert f.may_contain(f"probe{i}")


def _call_encode(a, out):
    return _native.lib().pbf_encode_data_blocks(0, _p(a["k"]), _p(a["ko"]), _p(a["v"]), _p(a["vo"]), a["n"], _p(a["bf"]),
                                                _p(a["bo"]), a["nblocks"], _p(out), 0)


def _call_build(f, a, out, bitmap):
    return _native.lib().pbf_build_sstable(f.handle, _p(a["k"]), _p(a["ko"]), _p(a["v"]), _p(a["vo"]), a["n"], _p(a["bf"]),
                                           _p(a["bo"]), a["nblocks"], _p(out), _p(bitmap))


def _call_builds(filters, a, outs, bitmaps, ntables=None):
    nt = len(filters) if ntables is None else ntables
    hs = (vp * len(filters))(*[None if f is None else f.handle.value for f in filters])
    douts = (vp * len(outs))(*[None if o is None else o.ctypes.data for o in outs])
    bouts = (vp * len(bitmaps))(*[b.ctypes.data for b in bitmaps])
    return _native.lib().pbf_build_sstables(hs, nt, _p(a["k"]), _p(a["ko"]), _p(a["v"]), _p(a["vo"]), a["n"], _p(a["bf"]),
                                            _p(a["bo"]), a["nblocks"], _p(a["tb"]), douts, bouts)


def _guarded_host(n):
    return np.full(n, GUARD, np.uint8)


def _untouched(*bufs):
    for b in bufs:
        assert (b == GUARD).all()


@pytest.mark.parametrize("name,mutate,message,_m", PLAN_REFUSALS, ids=PLAN_IDS)
def test_encode_data_blocks_refuses_bad_host_plan(name, mutate, message, _m):
    a, want = _valid_args()
    out = _guarded_host(len(want) + 64)
    mutate(a)
    _refused(_call_encode(a, out), message)
    _untouched(out)


def test_encode_data_blocks_null_output_and_valid_plan():
    a, want = _valid_args()
    _refused(_call_encode(a, None), NULL)
    out = _guarded_host(len(want) + 64)
    assert _call_encode(a, out) == _native.PBF_OK  # the unmutated plan is a good one
    assert out[:len(want)].tobytes() == want
    _untouched(out[len(want):])


BUILD_REFUSALS = PLAN_REFUSALS + [
    ("key_offsets_from_1", _set("ko", 0, 1), START, START),
    ("value_offsets_from_1", _set("vo", 0, 1), START, START),
    ("null_keys", _null("k"), NULL, NULL),
    ("null_values", _null("v"), NULL, NULL),
]
BUILD_IDS = [r[0] for r in BUILD_REFUSALS]


@pytest.mark.parametrize("name,mutate,message,_m", BUILD_REFUSALS, ids=BUILD_IDS)
def test_build_sstable_refuses_bad_host_plan(name, mutate, message, _m):
    a, want = _valid_args()
    f = BloomFilter(32, 3)
    out, bitmap = _guarded_host(len(want) + 64), _guarded_host(32)
    mutate(a)
    _refused(_call_build(f, a, out, bitmap), message)
    _untouched(out, bitmap)
    assert f.bitmap() == bytes(32)
    _still_usable(f)


def test_build_sstable_no_records_null_output_and_valid_plan():
    a, want = _valid_args()
    f = BloomFilter(32, 3)
    out, bitmap = _guarded_host(len(want) + 64), _guarded_host(32)
    for field in ("n", "nblocks"):
        b = dict(a)
        b[field] = 0
        _refused(_call_build(f, b, out, bitmap), "an SSTable needs at least one record")
    _refused(_call_build(f, a, None, bitmap), NULL)
    _untouched(out, bitmap)
    _still_usable(f)
    g = BloomFilter(32, 3)
    assert _call_build(g, a, out, bitmap) == _native.PBF_OK
    assert out[:len(want)].tobytes() == want
    _untouched(out[len(want):])
    assert bitmap.tobytes() == g.bitmap() != bytes(32)
    _still_usable(g)


def _tables_setup():
    a, want = _valid_args()
    filters = [BloomFilter(32, 3), BloomFilter(32, 3)]
    split = int(a["bo"][2])
    outs = [_guarded_host(split + 64), _guarded_host(len(want) - split + 64)]
    bitmaps = [_guarded_host(32), _guarded_host(32)]
    return a, want, filters, outs, bitmaps, split


@pytest.mark.parametrize("name,mutate,_m,message", BUILD_REFUSALS + [
    ("empty_block", _empty_block, None, INCR),
    ("no_blocks", lambda a: a.update(nblocks=0), None, COVER_W),
    ("tables_from_1", _set("tb", 0, 1), None, "tables must cover the blocks"),
    ("tables_end_early", _set("tb", 2, 2), None, "tables must cover the blocks"),
    ("tables_end_late", _set("tb", 2, 4), None, "tables must cover the blocks"),
    ("table_without_blocks", _set("tb", 1, 0), None, "a table without blocks"),
    ("second_table_empty", lambda a: a.update(tb=np.array([0, 3, 3], np.uint64)), None, "a table without blocks"),
    ("null_table_blocks", _null("tb"), None, NULL),
], ids=BUILD_IDS + ["empty_block", "no_blocks", "tables_from_1", "tables_end_early", "tables_end_late",
                    "table_without_blocks", "second_table_empty", "null_table_blocks"])
def test_build_sstables_refuses_bad_host_plan(name, mutate, _m, message):
    a, want, filters, outs, bitmaps, _ = _tables_setup()
    mutate(a)
    _refused(_call_builds(filters, a, outs, bitmaps), message)
    _untouched(*outs, *bitmaps)
    assert all(f.bitmap() == bytes(32) for f in filters)
    _still_usable(*filters)


def test_build_sstables_refuses_bad_filter_sets_and_builds_the_valid_one():
    a, want, filters, outs, bitmaps, split = _tables_setup()
    _refused(_call_builds([filters[0], filters[0]], a, outs, bitmaps), "a filter appears twice")
    _refused(_call_builds([filters[0], None], a, outs, bitmaps), "null filter or output in the set")
    _refused(_call_builds(filters, a, [outs[0], None], bitmaps), "null filter or output in the set")
    _untouched(*outs, *bitmaps)
    assert all(f.bitmap() == bytes(32) for f in filters)
    _still_usable(*filters)
    # the plan with an empty block that pbf_build_sstables refuses is one pbf_encode_data_blocks takes
    b = dict(a)
    _empty_block(b)
    sec = _guarded_host(int(b["bo"][3]))
    assert _call_encode(b, sec) == _native.PBF_OK
    # the unmutated set builds: both data sections, both bitmaps
    fresh = [BloomFilter(32, 3), BloomFilter(32, 3)]
    assert _call_builds(fresh, a, outs, bitmaps) == _native.PBF_OK
    assert outs[0][:split].tobytes() + outs[1][:len(want) - split].tobytes() == want
    _untouched(outs[0][split:], outs[1][len(want) - split:])
    assert [b.tobytes() for b in bitmaps] == [f.bitmap() for f in fresh]
    _still_usable(*fresh)


def test_build_sstables_refuses_filters_on_different_devices():
    if _native.device_count() < 2:
        pytest.skip("needs two devices")
    a, want, filters, outs, bitmaps, _ = _tables_setup()
    filters[1] = BloomFilter(32, 3, device=1)
    _refused(_call_builds(filters, a, outs, bitmaps), "the outputs' filters must share a device")
    _untouched(*outs, *bitmaps)
    _still_usable(*filters)
