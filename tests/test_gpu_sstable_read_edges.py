"""Branches of the resident-SSTable point lookup (pbf_sst_open / pbf_sst_get / pbf_sst_gather,
csrc/sstable_read_kernels.hpp) that the golden shapes of tests/test_gpu_sstable_read.py do not
enter: more than 64 tables in one call, the length scan's carry loop and 64-bit totals, every
(source, destination) alignment of the gather, the validator's rules one by one, stored keys
with bytes >= 0x80, dense key collisions, a window of a key batch.  Every expected value is
plain Python over the test's own inputs (dicts, bytes slicing, numpy.cumsum) or ModelTable."""
import collections
import ctypes
import itertools
import struct

import numpy as np
import pytest

from pebbledb_amd import DeviceSSTable, _native, lsm_get
from pebbledb_amd.keys import PackedKeys
from pebbledb_amd.sstable_data import build_sstable
from pebbledb_amd.sstable_read import gather, lookup

import sstable_get_model as M
import sstable_raw as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

vp = ctypes.c_void_p
TABLES_PER_LAUNCH = 64  # kSstTablesPerLaunch
SCAN_TILE = 2048        # kScanTile: 256 threads x 8 lengths


@pytest.fixture
def opened():
    """open_raw that closes what it opened."""
    handles = []

    def _open(data, block_off):
        handles.append(R.open_raw(data, block_off))
        return handles[-1]

    yield _open
    for t in handles:
        t.close()


def slices(values, offs):
    raw = values.tobytes()
    return [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


# ------------------------------------------------------------------ 1. more than 64 tables
_MANY = {}


def many():
    """The 130 tables of sstable_raw.many_table_rows at block size 64, built once."""
    if not _MANY:
        rows = R.many_table_rows()
        files, tables = [], []
        for row in rows:
            keys = sorted(row)
            f, _, _ = build_sstable(keys, [row[k] for k in keys], 64)
            files.append(bytes(f))
            tables.append(DeviceSSTable.from_bytes(f))
        universe = [R.many_key(i) for i in range(R.MANY_UNIVERSE)]
        fillers = sorted(k for row in rows for k in row if "~" in k)
        probes = universe + fillers + ["", "t", "t0000x", "t0299~", "u0000", "s9999"]
        probes += ["t03"] * (len(probes) % 8 == 0)  # n is not a multiple of 8
        _MANY.update(rows=rows, files=files, tables=tables, models=[M.ModelTable(f) for f in files],
                     universe=universe, probes=probes)
    return _MANY


def check_walk(rows, models, probes, table, val_off, val_len, values, offs, keep=None):
    """table[i] = the lowest row that stores probe i (and whose mask keeps it), the value and
    its offset that row's."""
    got = slices(values, offs)
    for i, k in enumerate(probes):
        r = R.first_row(rows, k, None if keep is None else [None if m is None else m[i] for m in keep])
        assert table[i] == r, (i, k)
        if r < 0:
            assert val_len[i] == -1 and got[i] == b""
        else:
            assert got[i] == rows[r][k] and val_len[i] == len(rows[r][k]), (i, k, r)
            assert (int(val_off[i]), int(val_len[i])) == R.locate(models[r], k), (i, k, r)
    assert int(offs[-1]) == values.size


def many_masks(n, rows, probes):
    """Bool masks for rows 5, 63, 64, 65, 129 (None elsewhere): about a quarter of the bits
    cleared (fixed seed), and the cases that cross a launch boundary set by hand."""
    rng = np.random.default_rng(64)
    keep = [None] * R.MANY_ROWS
    for r in (5, 63, 64, 65, 129):
        keep[r] = rng.random(n) < 0.75
    at = {k: i for i, k in enumerate(probes)}
    keep[63][at[R.many_key(53)]] = False   # stored in 63 and 64: masked in launch 0, found in launch 1
    keep[64][at[R.many_key(53)]] = True
    keep[63][at[R.many_key(54)]] = False   # masked in both
    keep[64][at[R.many_key(54)]] = False
    keep[63][at[R.many_key(55)]] = True    # launch 0 wins although launch 1 also holds it
    keep[129][at[R.many_key(43)]] = True   # stored only in row 129: a hit of launch 2 alone
    keep[129][at[R.many_key(44)]] = False
    keep[64][at[R.many_key(23)]] = True    # stored only in row 64
    keep[64][at[R.many_key(24)]] = False
    return keep


def test_many_tables_three_launches():
    """130 tables = 3 launches of k_lsm_get and k_gather_values (t0 = 0, 64, 128): the row, the
    offset and the value of every probe, without masks, with masks on rows 5, 63, 64, 65, 129
    (the compacted mask slot of the host path differs from the row), in both key layouts."""
    m = many()
    rows, tables, models, probes = m["rows"], m["tables"], m["models"], m["probes"]
    assert -(-len(tables) // TABLES_PER_LAUNCH) == 3 and len(probes) % 8 != 0
    pk = PackedKeys.from_strs(probes)
    fixed = PackedKeys.from_strs(m["universe"])
    assert pk.offsets is not None and fixed.key_len == 5 and fixed.n % 8 != 0
    for keys, batch in ((probes, pk), (m["universe"], fixed)):
        keep = many_masks(len(keys), rows, keys)
        masks = [None if k is None else np.packbits(k, bitorder="little") for k in keep]
        assert [r for r, k in enumerate(masks) if k is not None] == [5, 63, 64, 65, 129]
        for mk, kp in ((None, None), (masks, keep)):
            table, val_off, val_len = lookup(tables, batch, mk)
            values, offs = gather(tables, table, val_off, val_len)
            check_walk(rows, models, keys, table, val_off, val_len, values, offs, kp)
    # the hand-set cases moved the winner as intended
    keep = many_masks(len(probes), rows, probes)
    table, _, _ = lookup(tables, pk, [None if k is None else np.packbits(k, bitorder="little") for k in keep])
    at = {k: i for i, k in enumerate(probes)}
    assert [int(table[at[R.many_key(i)]]) for i in (53, 54, 55, 43, 44, 23, 24)] == [64, -1, 63, 129, -1, 64, -1]


def test_many_tables_device_pointers():
    """The same call with keys, masks and outputs in device memory (offsets layout)."""
    m = many()
    rows, tables, probes = m["rows"], m["tables"], m["probes"]
    n, T = len(probes), len(tables)
    pk = PackedKeys.from_strs(probes)
    keep = many_masks(n, rows, probes)
    L = _native.lib()
    hs = (vp * T)(*[t.handle.value for t in tables])
    kd = torch.from_numpy(pk.data.copy()).cuda()
    od = torch.from_numpy(pk.offsets.view(np.int64).copy()).cuda()
    md = {r: torch.from_numpy(np.packbits(k, bitorder="little")).cuda() for r, k in enumerate(keep) if k is not None}
    table = torch.empty(n, dtype=torch.int32, device="cuda")
    val_off = torch.empty(n, dtype=torch.int64, device="cuda")
    val_len = torch.empty(n, dtype=torch.int32, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for mp, kp in (((vp * T)(), None), ((vp * T)(*[md[r].data_ptr() if r in md else None for r in range(T)]), keep)):
        _native.check(L.pbf_sst_get(hs, T, vp(kd.data_ptr()), vp(od.data_ptr()), 0, n, mp, 1, vp(sp or None),
                                    vp(table.data_ptr()), vp(val_off.data_ptr()), vp(val_len.data_ptr())), "pbf_sst_get")
        torch.cuda.synchronize()
        total = int(np.maximum(val_len.cpu().numpy(), 0).sum())
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        _native.check(L.pbf_sst_gather(hs, T, vp(table.data_ptr()), vp(val_off.data_ptr()), vp(val_len.data_ptr()), n,
                                       vp(out.data_ptr()), total, vp(offs.data_ptr()), 1, vp(sp or None)), "pbf_sst_gather")
        torch.cuda.synchronize()
        check_walk(rows, m["models"], probes, table.cpu().numpy(), val_off.cpu().numpy(), val_len.cpu().numpy(),
                   out.cpu().numpy(), offs.cpu().numpy(), kp)


def test_many_tables_get_batch():
    """lsm_get.get_batch over the 130 tables: rows [0, 70) as level 0, rows [70, 128) as one level
    (disjoint ascending ranges), rows 128 and 129 as a level each (they share keys with rows 70
    and 10, so they cannot join the level of disjoint ranges).  A filter has no false negative,
    so the answer is the first row in order that stores the key.  The filter stage has no table
    limit of its own (it loops over sets of 64 / 8 filters), so this leg runs all 130."""
    m = many()
    rows, tables, probes = m["rows"], m["tables"], m["probes"]
    level0, levels = tables[:R.MANY_L0], [tables[R.MANY_L0:128], [tables[128]], [tables[129]]]
    table, values, offs = lsm_get.get_batch(probes, level0, levels)
    got = slices(values, offs)
    for i, k in enumerate(probes):
        r = R.first_row(rows, k)
        assert table[i] == r and got[i] == (rows[r][k] if r >= 0 else b""), (i, k)


@pytest.mark.parametrize("first,count", [(1, 64), (0, 65)])
def test_exactly_64_and_65_tables(first, count):
    """64 tables: one launch, its last slot used; 65: a second launch of one table.  Row 64's
    own keys are found at index 64 - first."""
    m = many()
    rows, tables = m["rows"][first:first + count], m["tables"][first:first + count]
    probes = [R.many_key(i) for i in (23, 24, 53, 13, 3, 9, 33)] + sorted(m["rows"][64])
    table, val_off, val_len = lookup(tables, probes)
    values, offs = gather(tables, table, val_off, val_len)
    check_walk(rows, m["models"][first:first + count], probes, table, val_off, val_len, values, offs)
    assert table[0] == table[1] == 64 - first and table[2] == 63 - first


# ------------------------------------------------------------------ 2. the length scan
def block_records():
    return [(f"s{i:03d}".encode(), M.value_of(i, 56)) for i in range(60)]


@pytest.fixture
def one_block(opened):
    """One table of one block of about 4 KiB of known bytes."""
    data, off = R.raw_data_section([block_records()])
    assert 4096 <= len(data) <= 4300 and len(off) == 2
    return opened(data, off), data


def gather_arrays(rng, n, data_len, lens):
    val_len = np.asarray(lens, dtype=np.int32)
    table = np.where(val_len >= 0, 0, -1).astype(np.int32)
    val_off = rng.integers(0, data_len - 3, n).astype(np.uint64)  # off + len <= data_len for len <= 3
    return table, val_off, val_len


def check_gather(t, data, table, val_off, val_len):
    values, offs = gather([t], table, val_off, val_len)
    lens = np.maximum(val_len, 0).astype(np.int64)
    want_offs = np.concatenate([[0], np.cumsum(lens)])
    assert np.array_equal(offs.astype(np.int64), want_offs)
    src = np.repeat(val_off.astype(np.int64), lens) + (np.arange(want_offs[-1]) - np.repeat(want_offs[:-1], lens))
    assert np.array_equal(values, np.frombuffer(data, dtype=np.uint8)[src])


def test_scan_carry_loop(one_block):
    """n = 2048 * 259 + 5: 260 tiles, so k_len_tile_scan's loop runs twice and the second pass
    starts from a non-zero carry."""
    t, data = one_block
    n = SCAN_TILE * 256 + SCAN_TILE * 3 + 5
    assert -(-n // SCAN_TILE) > 256
    rng = np.random.default_rng(2048)
    table, val_off, val_len = gather_arrays(rng, n, len(data), rng.integers(-1, 4, n))
    assert np.maximum(val_len[:SCAN_TILE * 256], 0).sum() > 0  # the carry into the second pass
    check_gather(t, data, table, val_off, val_len)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097])
def test_scan_tile_edges(one_block, n):
    t, data = one_block
    rng = np.random.default_rng(n)
    for lens in (rng.integers(-1, 4, n), np.full(n, -1), np.zeros(n, dtype=np.int64)):
        table, val_off, val_len = gather_arrays(rng, n, len(data), lens)
        check_gather(t, data, table, val_off, val_len)
        if lens.max() <= 0:
            values, offs = gather([t], table, val_off, val_len)
            assert values.size == 0 and not offs.any()


def test_scan_totals_over_32_bits(one_block):
    """Offsets only (out_bytes = NULL): no value is copied, so the entries need not be valid."""
    t, _ = one_block
    big = 2 ** 31 - 1
    val_len = np.array([big, -1, big, 0, big], dtype=np.int32)
    table = np.zeros(5, dtype=np.int32)
    val_off = np.zeros(5, dtype=np.uint64)
    offs = np.full(6, 0xAA, dtype=np.uint64)
    hs = (vp * 1)(t._h.value)
    _native.check(_native.lib().pbf_sst_gather(hs, 1, vp(table.ctypes.data), vp(val_off.ctypes.data),
                                               vp(val_len.ctypes.data), 5, None, 0, vp(offs.ctypes.data), 0, None),
                  "pbf_sst_gather")
    assert offs.tolist() == [0, big, big, 2 * big, 2 * big, 3 * big] and 3 * big == 3 * 2 ** 31 - 3 > 2 ** 32


# ------------------------------------------------------------------ 3. gather alignment
SWEEP_LENS = list(range(1, 41)) + [63, 64, 65, 127, 128, 129, 143, 144, 145, 255, 256, 257]


def sweep_entries(data_len):
    """(val_off, val_len, is_pad): one entry per (source offset mod 16, destination offset mod
    16, length), the destination alignment set by a pad entry in front where needed."""
    entries, at, idx = [], 0, 0
    spread = (data_len - 257 - 16) // 16
    for s, d, ln in itertools.product(range(16), range(16), SWEEP_LENS):
        pad = (d - at) % 16
        if pad:
            entries.append((0, pad, True))
            at += pad
        assert at % 16 == d
        entries.append((16 * (idx % spread) + s, ln, False))
        at += ln
        idx += 1
    return entries


def test_gather_alignment_sweep(one_block):
    """Every (source mod 16, destination mod 16, length) of k_gather_values' three parts: the
    head = L case (short values that end before the boundary), nq = 0, lengths around one pass
    of the 8 lanes (128).  Host path, and device path with the output's base at +0 and +5 bytes
    (the head is computed from the absolute address)."""
    t, data = one_block
    entries = sweep_entries(len(data))
    n = len(entries)
    assert 20_000 < n < 30_000 and sum(not e[2] for e in entries) == 16 * 16 * len(SWEEP_LENS)
    val_off = np.array([e[0] for e in entries], dtype=np.uint64)
    val_len = np.array([e[1] for e in entries], dtype=np.int32)
    table = np.zeros(n, dtype=np.int32)
    want = b"".join(data[o:o + ln] for o, ln, _ in entries)
    want_offs = np.concatenate([[0], np.cumsum(val_len.astype(np.int64))])
    seen = {(int(o) % 16, int(a) % 16, int(ln)) for (o, ln, pad), a in zip(entries, want_offs) if not pad}
    assert seen == set(itertools.product(range(16), range(16), SWEEP_LENS))
    values, offs = gather([t], table, val_off, val_len)
    assert np.array_equal(offs.astype(np.int64), want_offs) and values.tobytes() == want
    L = _native.lib()
    hs = (vp * 1)(t._h.value)
    td, od, ld = (torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in (table, val_off, val_len))
    offs_d = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    for base in (0, 5):
        buf = torch.full((len(want) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        out = buf[base:]
        torch.cuda.synchronize()
        _native.check(L.pbf_sst_gather(hs, 1, vp(td.data_ptr()), vp(od.data_ptr()), vp(ld.data_ptr()), n,
                                       vp(out.data_ptr()), len(want), vp(offs_d.data_ptr()), 1, vp(sp or None)), "pbf_sst_gather")
        torch.cuda.synchronize()
        got = buf.cpu().numpy().tobytes()
        assert got[base:base + len(want)] == want
        assert got[:base] == b"\xee" * base and got[base + len(want):] == b"\xee" * (32 - base)  # nothing written outside
        assert np.array_equal(offs_d.cpu().numpy(), want_offs)


def test_a_60000_byte_value_among_short_ones():
    keys = ["a", "b", "c", "d", "e"]
    vals = [M.value_of(1, 6000), M.value_of(2, 60_000), M.value_of(3, 6000), b"short", b""]
    t = DeviceSSTable.from_bytes(build_sstable(keys, vals, 65_536)[0])
    assert ("b", "b") in [(m[0], m[1]) for m in t.meta_blocks]  # a block of its own
    probes = ["d", "b", "a", "zz", "e", "c", "b"]
    found, values, offs = t.get_many(probes)
    stored = dict(zip(keys, vals))
    assert found.tolist() == [k in stored for k in probes]
    assert slices(values, offs) == [stored.get(k, b"") for k in probes]
    t.close()


# ------------------------------------------------------------------ 4. gather refusals
def call_gather(hs, nt, table, val_off, val_len, cap):
    table, val_len = np.asarray(table, dtype=np.int32), np.asarray(val_len, dtype=np.int32)
    val_off = np.asarray(val_off, dtype=np.uint64)
    out = np.full(cap, 0xEE, dtype=np.uint8)
    offs = np.zeros(len(table) + 1, dtype=np.uint64)
    rc = _native.lib().pbf_sst_gather(hs, nt, vp(table.ctypes.data), vp(val_off.ctypes.data), vp(val_len.ctypes.data),
                                      len(table), vp(out.ctypes.data), cap, vp(offs.ctypes.data), 0, None)
    return rc, _native.lib().pbf_last_error().decode(), out, offs


def test_gather_refuses_entries_outside_their_table(one_block):
    """The kernel's own bounds check.  Every refused entry lies within 16 bytes of the data
    section's end (the handle pads by 16), so nothing outside the allocation would be read even
    if the check were wrong."""
    t, data = one_block
    dl = len(data)
    hs = (vp * 1)(t._h.value)
    bad = [(1, 0, 4), (-1, 0, 4), (0, dl - 3, 5), (0, dl + 1, 1)]
    good = [(0, 10, 7), (0, dl - 5, 5), (0, 100, 20)]
    for refused in [[b] for b in bad] + [bad]:
        batch = [good[0]] + refused[:1] + [good[1]] + refused[1:] + [good[2]]
        tb, vo, vl = zip(*batch)
        rc, msg, out, offs = call_gather(hs, 1, tb, vo, vl, sum(vl))
        assert rc == _native.PBF_ERR_INVALID and msg.startswith(f"{len(refused)} entries name no table or lie outside"), msg
        assert offs.tolist() == [0] + list(np.cumsum(vl))
        for i, e in enumerate(batch):
            if e in good:
                assert out[int(offs[i]):int(offs[i + 1])].tobytes() == data[e[1]:e[1] + e[2]]
    rc, msg, out, offs = call_gather(hs, 1, *zip(*good), sum(g[2] for g in good))
    assert rc == 0 and out.tobytes() == b"".join(data[o:o + ln] for _, o, ln in good)


def test_gather_bounds_are_those_of_the_named_row():
    """ntables = 130: an offset valid for row 1 but past row 0's end is copied from row 1; rows
    64 and 129 (later launches) are indexed from their launch's t0."""
    m = many()
    order = sorted(range(R.MANY_ROWS), key=lambda r: len(m["models"][r].data))
    small, large = order[0], order[-1]
    rest = [r for r in range(R.MANY_ROWS) if r not in (small, large)]
    rows = [small, large] + rest
    files = [m["models"][r].data for r in rows]
    tables = [m["tables"][r] for r in rows]
    assert len(files[1]) > len(files[0]) and len(tables) == 130
    hs = (vp * 130)(*[t.handle.value for t in tables])
    batch = [(1, len(files[1]) - 4, 4), (0, 3, 9), (64, 5, 11), (129, len(files[129]) - 6, 6), (63, 0, 8), (128, 7, 3)]
    tb, vo, vl = zip(*batch)
    rc, msg, out, offs = call_gather(hs, 130, tb, vo, vl, sum(vl))
    assert rc == 0, msg
    assert out.tobytes() == b"".join(files[r][o:o + ln] for r, o, ln in batch)


# ------------------------------------------------------------------ 5. the validator's rules
RULES = ("block count", "record offsets", "record sizes", "key order")
ASC = [f"r{i:02d}".encode() for i in range(10)]
ASC_V = [bytes([65 + i]) * 5 for i in range(10)]  # records of 4 + 3 + 4 + 5 = 16 bytes
RECS = list(zip(ASC, ASC_V))
B0, B1, B2 = RECS[:4], RECS[4:8], RECS[8:]  # the blocks block_size 64 gives


def patched(block, at, fmt, value):
    b = bytearray(R.raw_block(block))
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def _descending():
    """u16 array [0, 32, 16] over a 32-byte record and a 16-byte one; the bytes at [16, 48) also
    frame as a record (inside the first one's value), so only the offsets rule is broken."""
    inner = struct.pack("<i", 3) + b"zzz" + struct.pack("<i", 21)  # header of a 32-byte record at byte 16
    first = R.record(b"r04", b"\0" * 5 + inner + b"\0" * 5)
    assert len(first) == 32
    return R.raw_block([first, RECS[5]], offsets=[0, 32, 16])


def _many_records(swaps):
    keys = [f"k{i:04d}".encode() for i in range(600)]
    for i in swaps:
        keys[i], keys[i + 1] = keys[i + 1], keys[i]
    return [R.raw_block([(k, b"vvv") for k in keys])]


# name -> (blocks as bytes, bad blocks, bad records, order violations, rules named).  "bad
# records" counts the records that failed the offsets or the sizes rule; "bad blocks" the blocks
# with a bad count or a bad u16 array.
INVALID = {
    "first_offset_not_zero": ([R.raw_block(B0), R.raw_block(B1, offsets=[1, 16, 32, 48]), R.raw_block(B2)], 1, 1, 0, {1}),
    "equal_offsets": ([R.raw_block(B0), R.raw_block([RECS[4], (b"r05", b"x" * 21)], offsets=[0, 16, 16])], 1, 1, 0, {1}),
    "descending_offsets": ([R.raw_block(B0), _descending()], 1, 1, 0, {1}),
    "offset_past_the_record_area": ([R.raw_block(B0), R.raw_block(B1, offsets=[0, 16, 32, 70])], 1, 2, 0, {1}),
    "extent_under_8_bytes": ([R.raw_block([R.record(*RECS[0]), b"\1\0\0\0", R.record(*RECS[1])])], 0, 1, 0, {2}),
    "negative_key_size": ([R.raw_block(B0), patched(B1, 16, "<i", -1)], 0, 1, 0, {2}),
    "key_size_over_the_extent": ([R.raw_block(B0), patched(B1, 16, "<i", 9)], 0, 1, 0, {2}),
    "negative_value_size": ([R.raw_block(B0), patched(B1, 32 + 7, "<i", -1)], 0, 1, 0, {2}),
    "empty_block": ([R.raw_block(B0), b"", R.raw_block(B1)], 1, 0, 0, {0}),
    "one_byte_block": ([R.raw_block(B0), b"\1", R.raw_block(B1)], 1, 0, 0, {0}),
    "equal_keys_across_a_seam": ([R.raw_block([(b"aa", b"1"), (b"ab", b"2")]), R.raw_block([(b"ab", b"3"), (b"ac", b"4")])],
                                 0, 0, 1, {3}),
    "prefix_key_across_a_seam": ([R.raw_block([(b"aa", b"1"), (b"abc", b"2")]), R.raw_block([(b"ab", b"3"), (b"ac", b"4")])],
                                 0, 0, 1, {3}),
    "two_rules_in_two_blocks": ([R.raw_block(B0, count=0), R.raw_block(B1), patched(B2, 16, "<i", 4)], 1, 1, 0, {0, 2}),
    "three_rules_in_three_blocks": ([R.raw_block(B0, count=0), R.raw_block([RECS[5], RECS[4], RECS[6]]),
                                     patched(B2, 16, "<i", 4)], 1, 1, 1, {0, 2, 3}),
    "three_swapped_pairs_of_600": (_many_records([10, 300, 598]), 0, 0, 3, {3}),
}


@pytest.mark.parametrize("name", list(INVALID))
def test_validator_rules(opened, name):
    """One crafted data section per clause of k_sst_validate / k_sst_validate_seams: refused at
    open with the rule's name (and no other rule's) and the three counts."""
    blocks, bad_blocks, bad_records, order, rules = INVALID[name]
    good = opened(*R.raw_data_section([B0, B1, B2]))  # the unpatched shape opens and answers
    _, _, val_len = lookup([good], ["r07", "r0"])
    assert val_len.tolist() == [5, -1]
    with pytest.raises(ValueError) as e:
        opened(*R.join_blocks(blocks))
    msg = str(e.value)
    assert f"({bad_blocks} bad blocks, {bad_records} bad records, {order} order violations)" in msg, msg
    assert {i for i, r in enumerate(RULES) if r + ":" in msg} == rules, msg


def test_the_600_record_block_opens_unswapped(opened):
    t = opened(*R.join_blocks(_many_records([])))
    _, _, val_len = lookup([t], ["k0010", "k0599", "k0600"])
    assert val_len.tolist() == [3, 3, -1]


def test_open_refusals_on_the_host():
    """Refused by pbf_sst_open's argument checks; *out stays null."""
    data, off = R.raw_data_section([B0, B1, B2])
    buf = np.frombuffer(data, dtype=np.uint8)
    L = _native.lib()

    def refused(block_off, nblocks, data_len, text):
        bo = np.asarray(block_off, dtype=np.uint32)
        h = vp(0x1234)
        rc = L.pbf_sst_open(0, vp(buf.ctypes.data), data_len, vp(bo.ctypes.data), nblocks, 0, ctypes.byref(h))
        assert rc == _native.PBF_ERR_INVALID and h.value is None
        assert text in L.pbf_last_error().decode()

    o = off.tolist()
    refused([1] + o[1:], 3, len(data), "from 0 to the data section's length")
    refused(o[:3] + [o[3] - 1], 3, len(data), "from 0 to the data section's length")
    refused([0, o[2], o[1], o[3]], 3, len(data), "must ascend")
    refused(o, 0, len(data), "at least one data block")
    refused([0, 0x80000000], 1, 0x80000000, "2 GiB")  # checked before any byte is read


def test_from_bytes_refusals():
    """DeviceSSTable's meta checks; a good table still opens afterwards."""
    keys, vals = [k.decode() for k in ASC], ASC_V
    good = bytes(build_sstable(keys, vals, 64)[0])
    meta_off, bloom_off = struct.unpack("<ii", good[-8:])
    entries, o = [], meta_off  # (offset of the first key, of the last key, of the i32)
    while o < bloom_off:
        fs, = struct.unpack_from("<H", good, o)
        ls, = struct.unpack_from("<H", good, o + 2 + fs)
        entries.append((o + 2, o + 4 + fs, o + 4 + fs + ls))
        o += 8 + fs + ls
    assert len(entries) == 3

    def with_bytes(at, new):
        return good[:at] + new + good[at + len(new):]

    cases = [
        (with_bytes(entries[1][0], b"r03"), "meta block 1 does not name"),  # block 1 starts at r04
        (with_bytes(entries[2][1], b"r08"), "meta block 2 does not name"),  # block 2 ends at r09
        (with_bytes(entries[2][2], struct.pack("<i", 1)), "meta block offsets must ascend"),
        (good[:bloom_off - 1] + good[bloom_off:-8] + struct.pack("<ii", meta_off, bloom_off - 1),
         "meta blocks do not parse|runs past the meta section"),
    ]
    for data, text in cases:
        with pytest.raises(ValueError, match=text):
            DeviceSSTable.from_bytes(data)
        t = DeviceSSTable.from_bytes(good)
        assert t.get("r07") == ASC_V[7]
        t.close()


# ------------------------------------------------------------------ 6. unsigned byte order
ALPHABET = (0x00, 0x61, 0x7F, 0x80, 0xFF)
CROSS = {0x7F: 0x80, 0x80: 0x7F, 0x61: 0xFF, 0xFF: 0x61, 0x00: 0x80}


def unsigned_keys():
    """Keys over ALPHABET of 0..18 bytes: pairs that first differ at byte 0, 7, 8, 15, 16, 17 by
    (0x7F, 0x80) and by (0x61, 0xFF) (a signed compare orders each pair the other way), with
    nothing and with a tail after the byte, and 150 random keys."""
    rng = np.random.default_rng(0x80)
    keys = {b""}
    for pos, (lo, hi) in itertools.product((0, 7, 8, 15, 16, 17), ((0x7F, 0x80), (0x61, 0xFF))):
        head = bytes(ALPHABET[(3 * j + pos) % 5] for j in range(pos))
        for tail in (b"", bytes(ALPHABET[(j + pos) % 5] for j in range(18 - pos - 1))):
            keys.update((head + bytes([lo]) + tail, head + bytes([hi]) + tail))
    while len(keys) < 200:
        keys.add(bytes(ALPHABET[int(x)] for x in rng.integers(0, 5, int(rng.integers(0, 19)))))
    return sorted(keys)


@pytest.mark.parametrize("block_size", [32, 128])
def test_stored_keys_order_as_unsigned_bytes(opened, block_size):
    """A table whose stored keys hold bytes >= 0x80 must open (a signed compare, in the bswapped
    words or in the byte tail, would call it unordered) and answer as the dict does.  At block
    size 32 nearly every record is a block of its own, so the pairs are seams and block last
    keys; at 128 they are neighbours inside blocks too."""
    keys = unsigned_keys()
    vals = [bytes([i & 0xFF]) * (1 + i % 3) for i in range(len(keys))]
    stored = dict(zip(keys, vals))
    for pos, (lo, hi) in itertools.product((0, 7, 8, 15, 16, 17), ((0x7F, 0x80), (0x61, 0xFF))):
        assert any(k[pos:pos + 1] == bytes([lo]) and k[:pos] + bytes([hi]) + k[pos + 1:] in stored for k in keys)
    blocks = R.split_blocks(keys, vals, block_size)
    assert len(blocks) >= (len(keys) * 3 // 4 if block_size == 32 else 20) and len(blocks) < len(keys)
    t = opened(*R.raw_data_section(blocks))
    probes = list(keys)
    for k in keys:
        probes += [k[:j] + bytes([CROSS[k[j]]]) + k[j + 1:] for j in range(len(k))]
    want = [stored.get(k) for k in probes]
    assert sum(v is not None for v in want) > len(keys) and sum(v is None for v in want) > 1000

    def check(batch, expect):
        table, val_off, val_len = lookup([t], batch)
        values, offs = gather([t], table, val_off, val_len)
        assert val_len.tolist() == [-1 if v is None else len(v) for v in expect]
        assert slices(values, offs) == [v or b"" for v in expect]

    check(R.pack_bytes(probes), want)
    by_len = collections.defaultdict(list)
    for k in probes:
        by_len[len(k)].append(k)
    for ln, group in by_len.items():
        if ln:
            check(PackedKeys(np.frombuffer(b"".join(group), dtype=np.uint8), len(group), key_len=ln),
                  [stored.get(k) for k in group])


# ------------------------------------------------------------------ 7. dense universes
def dense_universe(alphabet, head=""):
    return [head + "".join(p) for n in range(11) for p in itertools.product(alphabet, repeat=n)]


@pytest.mark.parametrize("block_size", [32, 64, 256])
@pytest.mark.parametrize("kind", ["nul_and_a", "shared_prefix"])
def test_dense_universe(kind, block_size):
    """All 2,047 strings of 0..10 characters over a two-letter alphabet, a random half stored:
    over {NUL, "a"} keys differ only by trailing NULs, which key_prefix's zero padding cannot
    tell apart; behind "pppppppp" every block's last key has the same key_prefix, so the block
    search is decided by the lp == kpre branch alone."""
    universe = dense_universe("\0a") if kind == "nul_and_a" else dense_universe("ab", "pppppppp")
    assert len(universe) == len(set(universe)) == 2047
    rng = np.random.default_rng(2047 + block_size)
    keys = sorted(k for k, keep in zip(universe, rng.random(2047) < 0.5) if keep)
    stored = {k: M.value_of(i, i % 4) for i, k in enumerate(keys)}
    f = build_sstable(keys, [stored[k] for k in keys], block_size)[0]
    t = DeviceSSTable.from_bytes(f)
    metas = t.meta_blocks
    top = collections.Counter(R.key_prefix(m[1].encode()) for m in metas).most_common(1)[0][1]
    if kind == "shared_prefix":
        assert 2 * top >= len(metas) and len(metas) > 8
    found, values, offs = t.get_many(universe)
    got = [v if ok else None for ok, v in zip(found, slices(values, offs))]
    assert got == [stored.get(k) for k in universe]
    model = M.ModelTable(bytes(f))
    for i in range(0, 2047, 13):
        assert model.get(universe[i]) == got[i]
    t.close()


# ------------------------------------------------------------------ 8. a window of a key batch
def test_key_window():
    """Keys [350, 650) of a packed batch of 1,000, passed as a slice of its offsets
    (offsets[0] != 0).  Host pointers: `keys` is the buffer the offsets index (the call copies
    keys + offsets[0]).  Device pointers: `keys` points at the window's first byte, as
    include/pebblebloom.h states the layout (key i = keys[offsets[i] - offsets[0], ...))."""
    stored_keys = [f"w{i:05d}" + "x" * (i % 7) for i in range(0, 1500, 3)]
    vals = [M.value_of(i, i % 23) for i in range(len(stored_keys))]
    t = DeviceSSTable.from_bytes(build_sstable(stored_keys, vals, 256)[0])
    probes = [f"w{i:05d}" + "x" * (i % 7) for i in range(250, 1250)]
    pk = PackedKeys.from_strs(probes)
    assert pk.n == 1000 and pk.offsets is not None
    win = PackedKeys(pk.data, 300, offsets=pk.offsets[350:651])
    assert win.offsets[0] != 0 and win.data.size == pk.data.size
    want = lookup([t], PackedKeys.from_strs(probes[350:650]))
    stored = dict(zip(stored_keys, vals))
    assert want[2].tolist() == [len(stored[k]) if k in stored else -1 for k in probes[350:650]]
    assert 50 < (want[2] >= 0).sum() < 250
    got = lookup([t], win)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    kd = torch.from_numpy(pk.data.copy()).cuda()
    od = torch.from_numpy(win.offsets.view(np.int64).copy()).cuda()
    table = torch.empty(300, dtype=torch.int32, device="cuda")
    val_off = torch.empty(300, dtype=torch.int64, device="cuda")
    val_len = torch.empty(300, dtype=torch.int32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    hs = (vp * 1)(t.handle.value)
    _native.check(_native.lib().pbf_sst_get(hs, 1, vp(kd.data_ptr() + int(win.offsets[0])), vp(od.data_ptr()), 0, 300,
                                            None, 1, vp(sp or None), vp(table.data_ptr()), vp(val_off.data_ptr()),
                                            vp(val_len.data_ptr())), "pbf_sst_get")
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), want[0])
    assert np.array_equal(val_off.cpu().numpy().view(np.uint64), want[1])
    assert np.array_equal(val_len.cpu().numpy(), want[2])
    t.close()
