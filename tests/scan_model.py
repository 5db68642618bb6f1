"""TEST INFRASTRUCTURE — a plain-Python restatement of the reference's bounded scan, and the
range rules of tests/golden/lsm_scan.json (tools/gen_golden_scan.py writes that fixture from the
REAL reference with these rules; tests/test_scan_model_cpu.py pins this model to it).

Restated:
* SSTableIterator(sstable, start_key, end_key) (src/iterators.py:58-141): the records with
  lower <= key <= upper, inclusive at both ends, in key order.  DataBlockIterator.__next__ tests
  ``if self._end_key and ...``, so upper == "" is NO upper bound.  Here: ``bisect_left`` /
  ``bisect_right`` over the table's key bytes give the window [lo, hi) (hi = max(hi, lo): an
  inverted range is empty).
* LsmStorage.scan (src/lsm_storage.py:183-191) over SSTables: MergingIterator over the tables'
  scans — ``merge_model.merge`` over the windows.

A table is a list of (key, value) pairs in its own key order, as in merge_model; bounds are str
(compared as UTF-8 bytes, Python's str order for the ASCII keys a table holds) or bytes.
"""
from __future__ import annotations

from bisect import bisect_left, bisect_right

import merge_model as MM

_b = MM._b


def window(rows, lower, upper) -> tuple[int, int]:
    """[lo, hi): the records of one table in [lower, upper]; upper == "" (or b"") is open."""
    keys = [_b(k) for k, _ in rows]
    lo = bisect_left(keys, _b(lower))
    up = _b(upper)
    hi = bisect_right(keys, up) if up else len(keys)
    return lo, max(hi, lo)


def windows(tables, lower, upper) -> list[tuple[int, int]]:
    return [window(rows, lower, upper) for rows in tables]


def scan(tables, lower, upper):
    """[(key bytes, value, source table)] of MergingIterator([t.scan(lower, upper) for t in tables])."""
    return MM.merge([rows[lo:hi] for rows, (lo, hi) in zip(tables, windows(tables, lower, upper))])


def scan_one(rows, lower, upper):
    """[(key bytes, value)] of SSTable.scan(lower, upper)."""
    lo, hi = window(rows, lower, upper)
    return [(_b(k), v) for k, v in rows[lo:hi]]


def presum(tables, lower, upper) -> tuple[int, int, int]:
    """(records, key bytes, value bytes) of the windows together, before de-duplication."""
    n = kb = vb = 0
    for rows, (lo, hi) in zip(tables, windows(tables, lower, upper)):
        n += hi - lo
        kb += sum(len(_b(k)) for k, _ in rows[lo:hi])
        vb += sum(len(v) for _, v in rows[lo:hi])
    return n, kb, vb


# ----------------------------------------------------------------------------- fixture rules
# The golden cases are merge_model's table rules of these names; case_ranges gives their ranges.
CASE_NAMES = ("overlap3", "overlap5", "every_table", "empty_newest")
CASES = [c for c in MM.CASES if c["name"] in CASE_NAMES]
LSM_CASE = "overlap3"  # also driven through a real LsmStorage by the generator


def _absent_after(key: str, union: set) -> str:
    """A key no table stores that sorts just after `key`: the next index of the same format that
    is free, where the key ends in digits and one is free below the next stored key; else the key
    extended by '5'."""
    digits = len(key) - len(key.rstrip("0123456789"))
    if digits:
        cand = key[:-digits] + f"{int(key[-digits:]) + 1:0{digits}d}"
        if len(cand) == len(key) and cand not in union:
            return cand
    return key + "5"


def case_ranges(case) -> list[tuple[str, str, str]]:
    """[(name, lower, upper)] for a case, by rule from its tables' keys."""
    tables = MM.case_tables(case)
    sets = [{k for k, _ in rows} for rows in tables]
    union = set().union(*sets)
    keys = sorted(union)
    n = len(keys)
    a, b = keys[n // 4], keys[(3 * n) // 4]
    mid, later = keys[n // 2], keys[n // 2 + min(200, n // 4)]
    out = [("both_stored", a, b),
           ("both_absent", _absent_after(keys[n // 5], union), _absent_after(keys[(4 * n) // 5], union)),
           ("lower_eq_upper_absent", _absent_after(mid, union), _absent_after(mid, union)),
           ("inverted", b, a),
           ("from_start", "", mid),
           ("to_end", mid, ""),
           ("everything", "", ""),
           ("below_all", " ", "!"),
           ("above_all", "~", "~~"),
           ("prefix_bounds", mid[:-1], later[:-1]),       # proper prefixes of stored keys
           ("extended_bounds", mid + "0", later + "0"),  # stored keys extended by one character
           ("non_ascii_bounds", mid[:-1] + "é", later + "€"),
           ("non_ascii_lower_only", "é", "")]
    # lower == upper on a key as many tables as possible store
    shared = max(keys, key=lambda k: (sum(k in s for s in sets), k == mid))
    out.append(("lower_eq_upper_stored", shared, shared))
    # bounds some tables store and others do not; where one exists, a lower bound held by tables
    # 0 and 2 but not table 1
    in02 = [k for k in keys if k in sets[0] and k in sets[2] and k not in sets[1]]
    some = [k for k in keys if 0 < sum(k in s for s in sets) < len(sets)]
    if in02:
        lo = in02[len(in02) // 3]
        ups = [k for k in some if k > lo]
        out.append(("lower_in_tables_0_and_2", lo, ups[min(150, len(ups) - 1)]))
    if some:
        out.append(("bounds_in_some_tables", some[len(some) // 6], some[(5 * len(some)) // 6]))
    return out
