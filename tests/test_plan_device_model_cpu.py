"""The numpy restatement of the device planner (tests/plan_device_model.py) against the host
planners ``sstable_data.plan_blocks`` / ``plan_compaction``: the edge list of tests/plan_cases.py,
a few thousand random size sequences (with small chunks, so seams, splits and dropped tails fall
everywhere), and the Python-side refusals of the resident write path that need no native call."""
from __future__ import annotations

import numpy as np
import pytest

import plan_cases
from plan_device_model import Oversize, plan_device_model
from pebbledb_amd.sstable_data import plan_blocks, plan_compaction

CASES = plan_cases.cases()
IDS = [c[0] for c in CASES]


def _same(got, want):
    for g, w, what in zip(got[:3], want[:3], ("block_first", "block_out", "table_blocks")):
        assert np.array_equal(np.asarray(g, np.uint64), np.asarray(w, np.uint64)), what
    assert got[3] == want[3]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_matches_host_planners(case):
    _, ko, vo, bs, mx = case
    bf, bo = plan_blocks(ko, vo, bs)
    _same(plan_device_model(ko, vo, bs, 0), (bf, bo, np.array([0, len(bf) - 1]), len(ko) - 1))
    _same(plan_device_model(ko, vo, bs, mx), plan_compaction(ko, vo, bs, mx))


def test_model_refuses_an_oversized_record():
    _, ko, vo, bs, mx = plan_cases.OVERSIZE
    for m in (0, mx):
        with pytest.raises(Oversize, match="a record is larger than block_size"):
            plan_device_model(ko, vo, bs, m)


def test_model_random_sequences():
    rng = np.random.default_rng(7)
    for it in range(3000):
        n = int(rng.integers(1, 120))
        bs = int(rng.choice([8, 12, 16, 40, 64, 100, 256]))
        sizes = rng.integers(8, bs + 1, n)
        if it % 3 == 0:
            sizes[:] = rng.integers(8, min(bs, 14) + 1)
        ko, vo = plan_cases.offsets(sizes)
        mx = int(rng.choice([1, 2 * bs, 5 * bs + 3, 20 * bs, int(sizes.sum()) + 2 * n]))
        chunk = int(rng.choice([1, 2, 7, 16, 64, 8192]))
        bf, bo = plan_blocks(ko, vo, bs)
        _same(plan_device_model(ko, vo, bs, 0, chunk), (bf, bo, np.array([0, len(bf) - 1]), n))
        _same(plan_device_model(ko, vo, bs, mx, chunk), plan_compaction(ko, vo, bs, mx))


# ------------------------------------------------------------------ refusals before any native call
class _NoTable:
    device = 0
    _h = None


def test_resident_compaction_refuses_bad_arguments_before_any_native_call(monkeypatch):
    from pebbledb_amd import _native, compaction

    def no_lib():
        raise AssertionError("a native call was made")

    monkeypatch.setattr(_native, "lib", no_lib)
    for fn in (compaction.compact_l0_resident, compaction.compact_level_resident):
        with pytest.raises(ValueError, match="no tables"):
            fn([])
        with pytest.raises(ValueError, match="at most 64 tables"):
            fn([_NoTable()] * 65)
        for mx in (0, -1):
            with pytest.raises(ValueError, match="max_sstable_size must be positive"):
                fn([_NoTable()], max_sstable_size=mx)
        for bs in (0, -5, 65_537):
            with pytest.raises(ValueError, match="block_size must be in"):
                fn([_NoTable()], block_size=bs)


def test_resident_flush_refuses_bad_arguments_before_any_native_call(monkeypatch):
    from pebbledb_amd import _native, memtable

    def no_lib():
        raise AssertionError("a native call was made")

    monkeypatch.setattr(_native, "lib", no_lib)
    for bs in (0, 65_537):
        with pytest.raises(ValueError, match="block_size must be in"):
            memtable.flush_log_resident([("a", b"1")], block_size=bs)
    with pytest.raises(ValueError, match="at least one record"):
        memtable.flush_log_resident([])
    with pytest.raises(ValueError, match="non-ASCII"):
        memtable.flush_log_resident([("é", b"1")])
