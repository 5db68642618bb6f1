"""The device planner (``pbf_plan_device``, csrc/sstable_plan_kernels.hpp) against the host
planners, entry for entry and in both modes, over the edge list of tests/plan_cases.py.  The
inputs are torch tensors; every output sits between 0xA5 guard bytes, and nothing past
nblocks + 1 / ntables + 1 entries may be written."""
import ctypes

import numpy as np
import pytest

import plan_cases
from pebbledb_amd import _native
from pebbledb_amd.sstable_data import plan_blocks_native, plan_compaction_native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = plan_cases.cases()
IDS = [c[0] for c in CASES]
GUARD = 0xA5
SLACK = 4  # guard entries in front of every output


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _plan_device(ko, vo, block_size, max_sstable_size, cap=None):
    """(rc, block_first, block_out, table_blocks, written, guards intact) of one call; the three
    outputs hold `cap` entries (default n + 1) after SLACK guard entries, all filled with 0xA5."""
    n = len(ko) - 1
    cap = n + 1 if cap is None else cap
    dko, dvo = _dev(ko), _dev(vo)
    outs = [torch.full(((SLACK + cap) * 8,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(3)]
    nb, nt, w = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    torch.cuda.synchronize()
    rc = _native.lib().pbf_plan_device(0, None, dko.data_ptr(), dvo.data_ptr(), n, block_size, max_sstable_size,
                                       *[o.data_ptr() + SLACK * 8 for o in outs], cap, ctypes.byref(nb),
                                       ctypes.byref(nt), ctypes.byref(w))
    host = [o.cpu().numpy() for o in outs]
    used = (nb.value + 1, nb.value + 1, nt.value + 1) if rc == 0 else (0, 0, 0)
    intact = all(bool((h[:SLACK * 8] == GUARD).all()) and bool((h[(SLACK + u) * 8:] == GUARD).all())
                 for h, u in zip(host, used))
    arrays = [h[SLACK * 8:(SLACK + u) * 8].view(np.uint64) for h, u in zip(host, used)]
    return rc, arrays[0], arrays[1], arrays[2], w.value, intact


def _same(got, want):
    rc, bf, bo, tb, written, intact = got
    assert rc == 0, _native.lib().pbf_last_error().decode()
    print("nblocks", len(bf) - 1, "ntables", len(tb) - 1, "written", written)
    assert np.array_equal(bf, np.asarray(want[0], np.uint64)), "block_first"
    assert np.array_equal(bo, np.asarray(want[1], np.uint64)), "block_out"
    assert np.array_equal(tb, np.asarray(want[2], np.uint64)), "table_blocks"
    assert written == want[3]
    assert intact, "an entry outside nblocks + 1 / ntables + 1 was written"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_blocks_mode_matches_plan_blocks(case):
    _, ko, vo, bs, _ = case
    bf, bo = plan_blocks_native(ko, vo, bs)
    _same(_plan_device(ko, vo, bs, 0), (bf, bo, [0, len(bf) - 1], len(ko) - 1))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compaction_mode_matches_plan_compaction(case):
    _, ko, vo, bs, mx = case
    _same(_plan_device(ko, vo, bs, mx), plan_compaction_native(ko, vo, bs, mx))


def test_the_listed_shapes_are_what_they_claim():
    """The cases hit the situations they are named for (judged on the host plan)."""
    by = {c[0]: c for c in CASES}

    def comp(name):
        _, ko, vo, bs, mx = by[name]
        return plan_compaction_native(ko, vo, bs, mx)

    bf, _, tb, w = comp("lone_record_is_the_last")
    assert w == 10 and list(bf[-2:]) == [9, 10] and len(tb) == 3
    assert comp("dropped_tail")[3] == 10 and comp("dropped_tail_long")[3] < 5 * 4000 + 3
    assert len(comp("inside_first_open_block")[2]) == 1 and comp("inside_first_open_block")[3] == 0
    assert len(comp("position_exactly_max")[0]) < len(comp("position_one_under_max")[0]) or \
        list(comp("position_exactly_max")[2]) != list(comp("position_one_under_max")[2])
    assert int(comp("position_exactly_max")[2][1]) == 4 and int(comp("position_one_under_max")[2][1]) == 5
    bf, _ = plan_blocks_native(by["empty_8192_one_block"][1], by["empty_8192_one_block"][2], 65536)
    assert list(bf) == [0, 8192]
    bf, _ = plan_blocks_native(by["empty_8193"][1], by["empty_8193"][2], 65536)
    assert list(bf) == [0, 8192, 8193]
    bf, _ = plan_blocks_native(by["block_ends_on_chunk_seam"][1], by["block_ends_on_chunk_seam"][2], 64 * 128)
    assert plan_cases.CHUNK in bf
    bf, _ = plan_blocks_native(by["block_straddles_chunk_seam"][1], by["block_straddles_chunk_seam"][2], 64 * 100)
    assert plan_cases.CHUNK not in bf
    assert len(comp("large_random")[0]) > 2000 and len(comp("large_random")[2]) > 3


def test_oversized_record_is_refused_and_the_next_call_succeeds():
    _, ko, vo, bs, mx = plan_cases.OVERSIZE
    for m in (0, mx):
        rc, _, _, _, _, intact = _plan_device(ko, vo, bs, m)
        assert rc == _native.PBF_ERR_INVALID
        assert "a record is larger than block_size" in _native.lib().pbf_last_error().decode()
        assert intact, "a refused plan wrote to its outputs"
    _, ko, vo, bs, mx = CASES[0]
    _same(_plan_device(ko, vo, bs, mx), plan_compaction_native(ko, vo, bs, mx))


def test_capacity_exactly_the_plan_and_one_short():
    """cap_entries = nblocks + 1 suffices; one less is refused without a write past the arrays."""
    _, ko, vo, bs, mx = next(c for c in CASES if c[0] == "split_every_block")
    want = plan_compaction_native(ko, vo, bs, mx)
    _same(_plan_device(ko, vo, bs, mx, cap=len(want[0])), want)
    rc, _, _, _, _, _ = _plan_device(ko, vo, bs, mx, cap=len(want[0]) - 1)
    assert rc == _native.PBF_ERR_INVALID and "cap_entries" in _native.lib().pbf_last_error().decode()
