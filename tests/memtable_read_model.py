"""TEST INFRASTRUCTURE — a plain-Python restatement of the memtable's read side and of the store
that keeps memtables in front of its tables, and the input rules of
tests/golden/memtable_read.json (tools/gen_golden_memtable_read.py writes that fixture from the REAL
reference with these rules; tests/test_memtable_read_cpu.py pins this model to it).

Restated:
* MemTable.put / get (src/memtable.py:64-79): a dict filled in put order; get returns the value of
  the last put or None, and a stored empty value is b"" (a hit: LsmStorage.get tests `is not None`).
* LsmStorage.get (src/lsm_storage.py:153-181): the active memtable, the immutable memtables
  (index 0 the newest), level 0 newest first, then the levels; the first holder answers.
* LsmStorage.scan (:183-191): MergingIterator over [active, *immutables, *level 0]; the lowest
  iterator index wins a key.  A memtable's range here is the SSTable's (inclusive at both ends,
  upper == "" open): the reference's own MemTable.scan drops in-range keys (red_black_tree.py:56-69)
  and is NOT restated; what is pinned is the store's scan after its memtables were flushed, which a
  scan with the memtables as sources must equal.

A layer (memtable or table) is a list of (key, value) pairs in key order; layers are listed newest
first.
"""
from __future__ import annotations

import hashlib
from bisect import bisect_left, bisect_right

import memtable_model as MT
import merge_model as MM
import scan_model as SM

_b = MM._b


# ----------------------------------------------------------------------------- the model
class ModelMemTable:
    """MemTable: last put wins, get -> value or None."""

    def __init__(self, puts=()):
        self.map = {}
        self.approximate_size = 0
        for k, v in puts:
            self.put(k, v)

    def put(self, key, value) -> None:
        kb = _b(key)
        self.map[kb] = value
        self.approximate_size += 8 + len(kb) + len(value)  # Record.size (record.py:62-72), ASCII keys

    def get(self, key):
        return self.map.get(_b(key))

    def rows(self):
        """MemTableIterator(memtable): [(key bytes, value)] in key order."""
        return sorted(self.map.items())

    def window(self, lower, upper):
        """[lo, hi) of rows() in [lower, upper]; upper == "" is open (scan_model.window)."""
        return SM.window(self.rows(), lower, upper)


def get_layers(layers, key):
    """(value or None, index of the layer that answered or -1): the first layer that holds the key."""
    kb = _b(key)
    for u, rows in enumerate(layers):
        keys = [_b(k) for k, _ in rows]
        i = bisect_left(keys, kb)
        if i < len(keys) and keys[i] == kb:
            return rows[i][1], u
    return None, -1


def get_many(layers, keys):
    """[(value or None, layer)] with one dict per layer."""
    maps = [{_b(k): v for k, v in rows} for rows in layers]
    out = []
    for key in keys:
        kb = _b(key)
        for u, m in enumerate(maps):
            if kb in m:
                out.append((m[kb], u))
                break
        else:
            out.append((None, -1))
    return out


def scan(layers, lower, upper):
    """[(key bytes, value, source layer)]: merge_model.merge over the layers' windows."""
    return SM.scan([[(_b(k), v) for k, v in rows] for rows in layers], lower, upper)


def windows(layers, lower, upper):
    return SM.windows(layers, lower, upper)


def lower_bound(keys, probe):
    """(index of the first key >= probe, whether it equals the probe) over sorted key bytes."""
    i = bisect_left(keys, _b(probe))
    return i, i < len(keys) and keys[i] == _b(probe)


def in_range(rows, lower, upper):
    """The rows with lower <= key <= upper, upper == "" open: the filter MemTable.scan should be."""
    lo, up = _b(lower), _b(upper)
    return [(k, v) for k, v in rows if _b(k) >= lo and (not up or _b(k) <= up)]


# ----------------------------------------------------------------------------- fixture rules: put logs
def log_probes(puts) -> list[str]:
    """The probe list of a put log: every stored key, absent keys below, between and above,
    proper prefixes and NUL extensions of stored keys, and the empty string."""
    stored = sorted({k for k, _ in puts})
    out = list(stored)
    out += ["", " ", "~~~~", "\x7f"]
    step = max(1, len(stored) // 64)
    for k in stored[::step]:
        out += [k + "\0", k + "5", k[:-1], k[:len(k) // 2], k + "\0\0"]
    return out


def probe_digest(results) -> dict:
    """What the fixture keeps of [(value or None)] per probe: hits, misses, stored empty values, the
    sha256 of the hit values back to back, and of the hit pattern (one byte per probe)."""
    hits = [v for v in results if v is not None]
    return {"hits": len(hits), "misses": len(results) - len(hits), "empty_hits": sum(1 for v in hits if v == b""),
            "values_sha256": hashlib.sha256(b"".join(hits)).hexdigest(),
            "pattern_sha256": hashlib.sha256(bytes(0 if v is None else 1 for v in results)).hexdigest()}


# ----------------------------------------------------------------------------- fixture rules: the store
# Put p of the store has key 'k%05d' % (h % KEYSPACE) and value value_of(p, vlen), vlen = 0 where
# h // KEYSPACE % 5 == 0, else 1 + h // KEYSPACE % 23 (h = mix(SEED, p)).  The memtable freezes by
# itself once approximate_size >= MAX_SSTABLE_SIZE (lsm_storage.py:133-141).  Phases: puts until 2
# memtables froze, both flushed and level 0 compacted (the level); puts until 3 more froze, flushed
# (level 0); puts until 2 more froze (the immutables), then ACTIVE_PUTS puts (the active memtable).
STORE = {"seed": 77, "keyspace": 1500, "max_sstable_size": 12288, "block_size": 1024, "active_puts": 250,
         "frozen_per_phase": [2, 3, 2]}


def store_put(p: int):
    h = MT.mix(STORE["seed"], p)
    q = h // STORE["keyspace"]
    return "k%05d" % (h % STORE["keyspace"]), MT.value_of(p, 0 if q % 5 == 0 else 1 + q % 23)


def store_memtables():
    """The put ranges of the store's memtables in freeze order: [[first put, stop put], ...], 7
    frozen by themselves and the active one last."""
    out, p = [], 0
    for _ in range(sum(STORE["frozen_per_phase"])):
        first, size = p, 0
        while size < STORE["max_sstable_size"]:
            k, v = store_put(p)
            size += 8 + len(k) + len(v)
            p += 1
        out.append([first, p])
    out.append([p, p + STORE["active_puts"]])
    return out


def store_layers(level_slices=None):
    """The store's layers newest first: [active, imm0, imm1, l0_0, l0_1, l0_2, *level tables], each
    [(key str, value)] in key order.  The level is the merge of the first two memtables as _compact
    split it: level_slices = [[first record, count], ...] of that merged run per output table (the
    fixture records them: _compact does not write the records of its last open block)."""
    mem = [ModelMemTable(store_put(p) for p in range(a, b)) for a, b in store_memtables()]
    rows = [[(k.decode(), v) for k, v in m.rows()] for m in mem]
    layers = [rows[7], rows[6], rows[5], rows[4], rows[3], rows[2]]
    merged = [(k.decode(), v) for k, v, _ in MM.merge([rows[1], rows[0]])]
    if level_slices is None:
        level_slices = [[0, len(merged)]]
    return layers + [merged[a:a + n] for a, n in level_slices]


def store_probes() -> list[str]:
    """About 4,000 probes: every key of the key space (stored or not), keys between, below and
    above, proper prefixes and NUL extensions, and the empty string."""
    ks = STORE["keyspace"]
    out = ["k%05d" % i for i in range(ks + 20)]
    out += ["k%05d5" % i for i in range(ks)]
    out += ["k%05d\0" % i for i in range(0, ks, 2)]
    out += ["k%04d" % i for i in range(0, ks // 10, 1)]
    out += ["", " ", "k", "~", "l00000", "j99999", "\x7f"]
    return out


def ranges_for(layers) -> list[tuple[str, str, str]]:
    """scan_model.case_ranges' rules over the given layers (its table rules replaced by them)."""
    orig = MM.case_tables
    MM.case_tables = lambda case: layers
    try:
        return SM.case_ranges(None)
    finally:
        MM.case_tables = orig
