"""Device SSTable point lookup (pbf_sst_open / pbf_sst_get / pbf_sst_gather, DeviceSSTable,
lsm_get.get_batch): equal to the real reference's recorded answers (tests/golden/sstable_get.json)
and, at sizes the golden cannot hold, to the plain-Python model pinned to it
(tests/sstable_get_model.py, tests/test_sstable_read_cpu.py)."""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

from oracle import sstable_oracle as so
from pebbledb_amd import DeviceSSTable, _native, lsm_get
from pebbledb_amd.keys import PackedKeys, PackedRecords
from pebbledb_amd.sstable_data import build_sstable
from pebbledb_amd.sstable_read import gather, lookup

import sstable_get_model as M
from test_sstable_read_cpu import B36, GOLD, assert_lsm_counts, lsm_levels, reference_file, total_digest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def values_of(found, values, offs):
    raw = values.tobytes()
    return [raw[int(offs[i]):int(offs[i + 1])] if found[i] else None for i in range(len(found))]


def check_batch(table, probes, stored):
    """get_many over `probes` in the layout PackedKeys.from_strs picks (fixed key_len when all
    probes share a byte length, offsets otherwise) equals the dict of stored records."""
    found, values, offs = table.get_many(probes)
    got = values_of(found, values, offs)
    want = [stored.get(k) for k in probes]
    assert got == want
    assert int(offs[-1]) == sum(len(v) for v in want if v is not None) == values.size
    return got


@pytest.mark.parametrize("case", GOLD["tables"], ids=[c["name"] for c in GOLD["tables"]])
def test_single_table_equals_reference(case):
    """The small-block shapes (single-record blocks, blocks that end exactly at block_size, a
    one-record table): every stored key, keys between blocks, before the first and after the
    last, prefixes and extensions, the empty key stored and not stored, the word-compare seams,
    non-ASCII probes — in the offsets layout (the whole list) and the fixed layout (the probes
    of each byte length)."""
    keys, vals, bs = M.table_records(case["name"])
    f, metas, _ = build_sstable(keys, vals, bs)
    assert hashlib.sha256(bytes(f)).hexdigest() == case["file_sha256"]
    t = DeviceSSTable.from_bytes(f)
    assert (t.nblocks, t.nrecords) == (len(case["meta_blocks"]), case["n_records"])
    assert [list(m) for m in t.meta_blocks] == case["meta_blocks"]
    assert (t.first_key, t.last_key) == (keys[0], keys[-1])
    probes = M.table_probes(keys, [tuple(m) for m in case["meta_blocks"]])
    stored = dict(zip(keys, vals))
    assert PackedKeys.from_strs(probes).offsets is not None or case["name"] == "one_record"
    got = check_batch(t, probes, stored)
    assert [-1 if v is None else len(v) for v in got] == case["found_len"]
    assert total_digest(got) == case["values_sha256"]
    by_len = {}
    for k in probes:
        by_len.setdefault(len(k.encode()), []).append(k)
    for L, group in by_len.items():
        if L > 0 and len(group) > 1:
            assert PackedKeys.from_strs(group).key_len == L
            check_batch(t, group, stored)
    assert t.get(keys[0]) == vals[0] and t.get(keys[-1] + "x") is None
    t.close()


def test_one_large_block():
    """3,000 records of 8-byte keys and 8-byte values at block_size 65536: a block of 2,730
    records (a deep in-block search; more records than k_sst_validate's workgroup has lanes)."""
    keys = [f"{7 * i:08d}" for i in range(3000)]
    vals = [struct.pack("<q", i * 1_000_003) for i in range(3000)]
    f, metas, _ = build_sstable(keys, vals, 65_536)
    t = DeviceSSTable.from_bytes(f)
    assert t.nblocks == 2 and t.nrecords == 3000
    stored = dict(zip(keys, vals))
    probes = keys + [f"{7 * i + 3:08d}" for i in range(3000)] + ["", "0", "99999999", "0000000", "000000000"]
    check_batch(t, probes, stored)
    m = M.ModelTable(bytes(f))
    for k in probes[::97]:
        assert m.get(k) == stored.get(k)


def test_mask_cases():
    keys = [f"m{i:03d}" for i in range(13)]
    vals = [bytes([i]) * (i + 1) for i in range(13)]
    t = DeviceSSTable.from_bytes(build_sstable(keys, vals, 64)[0])
    stored = dict(zip(keys, vals))
    mask = np.ones(13, dtype=bool)  # n is not a multiple of 8
    mask[[2, 8, 12]] = False
    for m in (mask, np.packbits(mask, bitorder="little")):
        found, values, offs = t.get_many(keys, mask=m)
        assert found.tolist() == mask.tolist()  # a cleared mask bit makes a present key absent
        assert values_of(found, values, offs) == [stored[k] if mask[i] else None for i, k in enumerate(keys)]
    for bit in (True, False):  # n = 1
        found, values, offs = t.get_many([keys[5]], mask=np.array([bit]))
        assert found.tolist() == [bit] and values.tobytes() == (vals[5] if bit else b"") and offs.tolist() == [0, 6 * bit]
    with pytest.raises(ValueError):
        t.get_many(keys, mask=np.ones(12, dtype=bool))
    found, values, offs = t.get_many([])
    assert found.size == 0 and values.size == 0 and offs.tolist() == [0]


_LARGE = {}


def large_table():
    """20,000 random records (keys 0-40 bytes, values 0-200 bytes, 4 KiB blocks), built once."""
    if not _LARGE:
        rng = np.random.default_rng(20261020)
        stored = {}
        while len(stored) < 20_000:
            L = int(rng.integers(0, 41))
            k = "".join(chr(97 + int(x)) for x in rng.integers(0, 26, L))
            stored.setdefault(k, rng.integers(0, 256, int(rng.integers(0, 201)), dtype=np.uint8).tobytes())
        keys = sorted(stored)
        f, _, _ = build_sstable(keys, [stored[k] for k in keys], 4096)
        _LARGE.update(keys=keys, stored=stored, file=bytes(f), table=DeviceSSTable.from_bytes(f))
    return _LARGE


def test_larger_table_equals_model_and_stored_bytes():
    lt = large_table()
    keys, stored, t = lt["keys"], lt["stored"], lt["table"]
    assert t.nrecords == 20_000 and t.nblocks > 400
    absent = [k + "!" for k in keys[::3]] + [k[:-1] + "A" for k in keys[1::5] if k] + ["", "zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzz"]
    absent = [k for k in absent if k not in stored]
    check_batch(t, keys, stored)      # all present
    got = check_batch(t, absent, stored)  # all absent
    assert all(v is None for v in got)
    mixed = [k for pair in zip(keys[::2], absent) for k in pair]
    got = check_batch(t, mixed, stored)
    m = M.ModelTable(lt["file"])
    for i in range(0, len(mixed), 41):
        assert m.get(mixed[i]) == got[i]


def lsm_tables():
    if "lsm" not in _LARGE:
        g = GOLD["lsm"]
        tables = []
        for spec, facts in zip(M.LSM_SPECS, g["tables"]):
            keys, vals = M.lsm_table_records(spec)
            f, _, _ = build_sstable(keys, vals, g["block_size"])
            assert hashlib.sha256(bytes(f)).hexdigest() == facts["file_sha256"]
            t = DeviceSSTable.from_bytes(f)
            assert (t.first_key, t.last_key, t.nrecords) == (facts["first_key"], facts["last_key"], facts["n_records"])
            tables.append(t)
        _LARGE["lsm"] = tables
    return _LARGE["lsm"]


def test_lsm_get_equals_reference():
    """get_batch / get_many over the golden's LSM equal LsmStorage.get's recorded answers: keys
    found behind a filter false positive, keys stored in several tables (newest wins), stored
    empty values."""
    g = GOLD["lsm"]
    assert_lsm_counts(g)
    level0, levels = lsm_levels(lsm_tables())
    probes = M.lsm_probes()
    table, values, offs = lsm_get.get_batch(probes, level0, levels)
    assert "".join("-" if t < 0 else B36[t] for t in table) == g["table_chars"]
    got = values_of(table >= 0, values, offs)
    assert "".join("-" if v is None else B36[len(v)] for v in got) == g["len_chars"]
    assert total_digest(got) == g["values_sha256"]
    for i, sha in g["value_sha256"].items():
        assert hashlib.sha256(got[int(i)]).hexdigest() == sha
    assert all(got[i] == b"" for i in g["empties"])
    pick = sorted(set(g["not_first"]) | set(g["multi"]) | set(g["empties"]) | set(range(19_990, 20_020)) |
                  {len(probes) - 8 + j for j in range(8)})
    assert lsm_get.get_many([probes[i] for i in pick], level0, levels) == [got[i] for i in pick]
    # the candidate rows are the ones the reference read (the walk consumed exactly these masks)
    masks = lsm_get.candidate_masks([probes[i] for i in pick], level0, levels)
    lists = lsm_get.candidate_lists(masks, len(pick))
    for j, i in enumerate(pick):
        read = g["reads"].get(str(i), [int(table[i])] if table[i] >= 0 else [])
        assert lists[j][:len(read)] == read


def test_round_trip_of_a_packed_flush():
    n = 5000
    keys = [f"{i:016x}" for i in range(0, 3 * n, 3)]
    vals = [M.value_of(i, 40 + i % 64) for i in range(n)]
    f, metas, bloom = build_sstable(PackedRecords.from_iter(zip(keys, vals)))
    t = DeviceSSTable.from_bytes(f)
    assert t.nrecords == n and len(t.meta_blocks) == len(metas)
    assert t.bloom_filter.to_bytes() == bloom.to_bytes()
    found, values, offs = t.get_many(PackedKeys.from_strs(keys))
    assert found.all() and values.tobytes() == b"".join(vals)
    assert np.array_equal(np.diff(offs.astype(np.int64)), [len(v) for v in vals])


def test_device_pointers():
    """Keys, masks and outputs in device memory (torch tensors), and a data section opened from
    device memory: the same answers as the host path."""
    lt = large_table()
    keys, stored, t = lt["keys"], lt["stored"], lt["table"]
    probes = keys[::5] + [k + "?" for k in keys[::7]]
    n = len(probes)
    pk = PackedKeys.from_strs(probes)
    want_t, want_o, want_l = lookup([t], pk)
    want_v, want_offs = gather([t], want_t, want_o, want_l)
    # a second handle over the same bytes, its data section handed over in device memory
    meta_off = t.meta_block_offset
    data_d = torch.from_numpy(np.frombuffer(lt["file"], dtype=np.uint8)[:meta_off].copy()).cuda()
    boff = np.asarray([m[2] for m in t.meta_blocks] + [meta_off], dtype=np.uint32)
    L = _native.lib()
    vp = ctypes.c_void_p
    h = vp()
    torch.cuda.synchronize()
    _native.check(L.pbf_sst_open(0, vp(data_d.data_ptr()), meta_off, vp(boff.ctypes.data), len(boff) - 1, 1,
                                 ctypes.byref(h)), "pbf_sst_open")
    kd = torch.from_numpy(pk.data.copy()).cuda()
    od = torch.from_numpy(pk.offsets.view(np.int64)).cuda()
    mask = np.ones(n, dtype=bool)
    mask[::4] = False
    md = torch.from_numpy(np.packbits(mask, bitorder="little")).cuda()
    table = torch.empty(n, dtype=torch.int32, device="cuda")
    val_off = torch.empty(n, dtype=torch.int64, device="cuda")
    val_len = torch.empty(n, dtype=torch.int32, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    hs = (vp * 1)(h.value)
    for m_ptrs, keep in (((vp * 1)(None), np.ones(n, dtype=bool)), ((vp * 1)(md.data_ptr()), mask)):
        _native.check(L.pbf_sst_get(hs, 1, vp(kd.data_ptr()), vp(od.data_ptr()), 0, n, m_ptrs, 1, vp(sp or None),
                                    vp(table.data_ptr()), vp(val_off.data_ptr()), vp(val_len.data_ptr())), "pbf_sst_get")
        wl = np.where(keep, want_l, -1)
        total = int(np.maximum(wl, 0).sum())
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        _native.check(L.pbf_sst_gather(hs, 1, vp(table.data_ptr()), vp(val_off.data_ptr()), vp(val_len.data_ptr()), n,
                                       vp(out.data_ptr()), total, vp(offs.data_ptr()), 1, vp(sp or None)), "pbf_sst_gather")
        torch.cuda.synchronize()
        assert np.array_equal(val_len.cpu().numpy(), wl)
        assert np.array_equal(table.cpu().numpy(), np.where(wl >= 0, 0, -1))
        assert np.array_equal(val_off.cpu().numpy()[wl >= 0], want_o.astype(np.int64)[wl >= 0])
        got = out.cpu().numpy().tobytes()
        assert got == b"".join(stored[k] for k, kp in zip(probes, keep) if kp and k in stored)
        assert int(offs[-1].item()) == total
    # an output buffer that is too small is refused, not overrun
    rc = L.pbf_sst_gather(hs, 1, vp(table.data_ptr()), vp(val_off.data_ptr()), vp(val_len.data_ptr()), n,
                          vp(out.data_ptr()), total - 1, vp(offs.data_ptr()), 1, vp(sp or None))
    assert rc == _native.PBF_ERR_INVALID and b"bytes" in L.pbf_last_error()
    assert np.array_equal(want_v, np.frombuffer(b"".join(stored[k] for k in probes if k in stored), dtype=np.uint8))
    assert L.pbf_sst_close(h) == 0
    # a closed handle is refused by every later call, without being touched
    assert L.pbf_sst_info(h, None, None, None) == _native.PBF_ERR_INVALID
    assert L.pbf_sst_close(h) == _native.PBF_ERR_INVALID


def test_close_waits_for_lookups_and_later_lookups_are_refused():
    """pbf_sst_close takes the handle's lock exclusively and lookups hold it shared: reader
    threads that race a close either get the right answer or are refused (ValueError), and
    every lookup after the close is refused."""
    import threading
    keys = [f"c{i:04d}" for i in range(2000)]
    vals = [M.value_of(i, i % 50) for i in range(2000)]
    t = DeviceSSTable.from_bytes(build_sstable(keys, vals, 1024)[0])
    pk = PackedKeys.from_strs(keys)
    want = np.array([len(v) for v in vals], dtype=np.int32)
    h = t.handle  # the raw handle, as a reader that fetched it before the close holds it
    hs = (ctypes.c_void_p * 1)(h.value)
    L = _native.lib()
    stop = threading.Event()
    stats = {"ok": 0, "refused": 0, "wrong": 0}

    def reader():
        table = np.empty(pk.n, dtype=np.int32)
        off = np.empty(pk.n, dtype=np.uint64)
        ln = np.empty(pk.n, dtype=np.int32)
        while not stop.is_set():
            rc = L.pbf_sst_get(hs, 1, pk.data.ctypes.data, None, pk.key_len, pk.n, None, 0, None, table.ctypes.data,
                               off.ctypes.data, ln.ctypes.data)
            if rc == 0:
                stats["ok" if np.array_equal(ln, want) else "wrong"] += 1
            elif rc == _native.PBF_ERR_INVALID:
                stats["refused"] += 1
                if stats["refused"] > 8:
                    return
            else:
                stats["wrong"] += 1
                return

    threads = [threading.Thread(target=reader) for _ in range(4)]
    for th in threads:
        th.start()
    while stats["ok"] < 20 and all(th.is_alive() for th in threads):
        pass
    t.close()
    for th in threads:
        th.join(timeout=30)
    stop.set()
    assert stats["wrong"] == 0 and stats["ok"] >= 20 and stats["refused"] >= 4, stats
    with pytest.raises(ValueError, match="closed"):
        t.get_many(keys)


# ------------------------------------------------------------------------------ refusals
def crafted_file(oracle, keys, vals, block_size, patch=None) -> bytes:
    """A file in the reference's layout (oracle/sstable_oracle.py: no order or charset checks),
    optionally with bytes of its data section replaced: patch(data: bytearray, metas)."""
    data = bytearray(reference_file(oracle, keys, vals, block_size))
    if patch:
        meta_off, = struct.unpack("i", data[-8:-4])
        _, _, metas = so.data_and_meta(keys, vals, block_size)
        patch(data, [m[2] for m in metas] + [meta_off])
    return bytes(data)


ASC = [f"r{i:02d}" for i in range(10)]
ASC_V = [bytes([65 + i]) * 5 for i in range(10)]  # records of 4 + 3 + 4 + 5 = 16 bytes


def _set_count(block, count):
    def patch(data, offs):
        struct.pack_into("H", data, offs[block + 1] - 2, count)
    return patch


def _bump_value_size(data, offs):  # the third record of block 0: value_size 5 -> 6
    struct.pack_into("i", data, offs[0] + 2 * 16 + 4 + 3, 6)


REFUSALS = {
    "non_ascii_stored_key": (["a", "clé-0001", "z"], [b"1", b"22", b"333"], 65_536, None, "record sizes"),
    "two_keys_swapped": (ASC[:4] + [ASC[5], ASC[4]] + ASC[6:], ASC_V, 65_536, None, "key order"),
    "two_keys_swapped_across_blocks": ([ASC[0], ASC[3], ASC[2], ASC[5]], ASC_V[:4], 32, None, "key order"),
    "equal_keys": (ASC[:3] + [ASC[2]] + ASC[4:], ASC_V, 65_536, None, "key order"),
    "truncated_u16_array": (ASC, ASC_V, 64, _set_count(1, 5), "record offsets"),
    "count_past_the_block": (ASC, ASC_V, 64, _set_count(0, 0xFFFF), "block count"),
    "value_size_overruns_the_record": (ASC, ASC_V, 64, _bump_value_size, "record sizes"),
    "count_zero": (ASC, ASC_V, 64, _set_count(2, 0), "block count"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_tables_raise_before_any_lookup(oracle, name):
    """Validation paths of well-formed launches: the table is refused at open (ValueError that
    names the rule), so no lookup ever runs on it."""
    keys, vals, bs, patch, rule = REFUSALS[name]
    good = crafted_file(oracle, ASC, ASC_V, bs)
    assert DeviceSSTable.from_bytes(good).get(ASC[7]) == ASC_V[7]  # the unpatched shape opens
    with pytest.raises(ValueError, match=rule):
        DeviceSSTable.from_bytes(crafted_file(oracle, keys, vals, bs, patch))


def test_tables_on_two_devices_are_refused():
    t0 = DeviceSSTable.from_bytes(build_sstable(ASC, ASC_V, 64)[0], device=0)
    if _native.device_count() > 1:
        t1 = DeviceSSTable.from_bytes(build_sstable(ASC, ASC_V, 64)[0], device=1)
        hs = (ctypes.c_void_p * 2)(t0.handle.value, t1.handle.value)
        out = np.zeros(4, dtype=np.int64)
        p = ctypes.c_void_p(out.ctypes.data)
        rc = _native.lib().pbf_sst_get(hs, 2, b"r01", None, 3, 1, None, 0, None, p, p, p)
        assert rc == _native.PBF_ERR_INVALID and b"share a device" in _native.lib().pbf_last_error()
    else:  # one GPU: a second table that claims another device
        t1 = DeviceSSTable.from_bytes(build_sstable(ASC, ASC_V, 64)[0], device=0)
        t1.device = 1
    with pytest.raises(ValueError, match="share a device"):
        lookup([t0, t1], ASC)
    with pytest.raises(ValueError, match="share a device"):
        lsm_get.get_batch(ASC, [t0], [[t1]])
    t0.close()
    with pytest.raises(ValueError, match="closed"):
        t0.get(ASC[0])
