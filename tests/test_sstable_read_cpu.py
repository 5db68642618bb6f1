"""CPU checks of the SSTable point lookup's test infrastructure and host side: the plain-Python
model (tests/sstable_get_model.py) equals the real reference's recorded answers
(tests/golden/sstable_get.json, tools/gen_golden_get.py), the host parsing of trailer and meta
blocks equals the reference's meta blocks, and the header declares the new exports."""
import hashlib
import struct

import numpy as np
import pytest

from conftest import load_golden
from oracle import sstable_oracle as so
from oracle.oracle import sizing
from pebbledb_amd import _native
from pebbledb_amd.keys import PackedKeys

import sstable_get_model as M

GOLD = load_golden("sstable_get.json")
B36 = "0123456789abcdefghijklmnopqrstuvwxyz"


def reference_file(oracle, keys, vals, block_size) -> bytes:
    """The file the reference's SSTableBuilder writes (the restatement of oracle/sstable_oracle.py
    with the C oracle's filter); callers compare its sha256 with the golden's."""
    nb_bytes, k = sizing(len(keys), 0.001)
    bitmap = oracle.build(nb_bytes, k, PackedKeys.from_strs(keys))
    return so.sstable_file(keys, vals, block_size, bitmap, k)


def total_digest(results) -> str:
    h = hashlib.sha256()
    for i, v in enumerate(results):
        if v is not None:
            h.update(struct.pack("<qq", i, len(v)))
            h.update(v)
    return h.hexdigest()


def table_case(oracle, case):
    keys, vals, bs = M.table_records(case["name"])
    data = reference_file(oracle, keys, vals, bs)
    assert len(data) == case["file_len"] and hashlib.sha256(data).hexdigest() == case["file_sha256"]
    probes = M.table_probes(keys, [tuple(m) for m in case["meta_blocks"]])
    assert len(probes) == case["n_probes"]
    return keys, vals, data, probes


_LSM = {}


def lsm_case(oracle):
    """(files, probes, per-row may_contain bool arrays): built once per session."""
    if not _LSM:
        g = GOLD["lsm"]
        files, hits = [], []
        probes = M.lsm_probes()
        pk = PackedKeys.from_strs(probes)
        for spec, facts in zip(M.LSM_SPECS, g["tables"]):
            keys, vals = M.lsm_table_records(spec)
            data = reference_file(oracle, keys, vals, g["block_size"])
            assert hashlib.sha256(data).hexdigest() == facts["file_sha256"]
            files.append(data)
            nb_bytes, k = sizing(len(keys), 0.001)
            bitmap = np.frombuffer(M.ModelTable(data).bloom[:-1], dtype=np.uint8)
            hits.append(np.unpackbits(oracle.probe(bitmap, k, pk), bitorder="little")[:len(probes)].astype(bool))
        _LSM.update(files=files, probes=probes, hits=hits)
    return _LSM["files"], _LSM["probes"], _LSM["hits"]


def lsm_levels(tables):
    """(level0, levels) of the LSM case's rows, in the reference's order."""
    level0 = [t for t, s in zip(tables, M.LSM_SPECS) if s[0] == 0]
    nlev = max(s[0] for s in M.LSM_SPECS)
    levels = [[t for t, s in zip(tables, M.LSM_SPECS) if s[0] == lv] for lv in range(1, nlev + 1)]
    return level0, levels


def assert_lsm_counts(g):
    """The fixture holds the coverage the generator asserted (a thinned-out fixture fails here)."""
    c = g["counts"]
    assert c["found_not_in_first_candidate"] >= 20 and len(g["not_first"]) == c["found_not_in_first_candidate"]
    assert c["reads_of_a_table_without_the_key"] >= 5
    assert c["keys_in_several_tables_with_different_values"] >= 20 and len(g["multi"]) >= 20
    assert c["stored_empty_values_returned"] >= 5 and len(g["empties"]) >= 5
    assert all(g["len_chars"][i] == "0" for i in g["empties"])
    assert all(len(g["reads"][str(i)]) > 1 and g["table_chars"][i] != "-" for i in g["not_first"])
    misses = sum(len(r) - (g["table_chars"][int(i)] != "-") for i, r in g["reads"].items())
    assert misses == c["reads_of_a_table_without_the_key"]
    assert len(g["table_chars"]) == len(g["len_chars"]) == g["n_probes"]


@pytest.mark.parametrize("case", GOLD["tables"], ids=[c["name"] for c in GOLD["tables"]])
def test_model_equals_reference_single_table(oracle, case):
    keys, vals, data, probes = table_case(oracle, case)
    t = M.ModelTable(data)
    got = [t.get(k) for k in probes]
    assert [-1 if v is None else len(v) for v in got] == case["found_len"]
    assert total_digest(got) == case["values_sha256"]
    assert sum(a == b for a, b, _ in t.meta_blocks) == case["single_record_blocks"]
    if case["name"].startswith("small_blocks"):
        assert case["single_record_blocks"] >= 5 and len(t.meta_blocks) > 40


def test_model_equals_reference_lsm(oracle):
    g = GOLD["lsm"]
    assert_lsm_counts(g)
    files, probes, hits = lsm_case(oracle)
    level0, levels = lsm_levels([M.ModelTable(f) for f in files])
    table, results = [], []
    for i, key in enumerate(probes):
        t, v, read = M.lsm_get(i, key, level0, levels, hits)
        table.append(t)
        results.append(v)
        assert read == g["reads"].get(str(i), [t] if t >= 0 else []), (i, key)
    assert "".join("-" if t < 0 else B36[t] for t in table) == g["table_chars"]
    assert "".join("-" if v is None else B36[len(v)] for v in results) == g["len_chars"]
    assert total_digest(results) == g["values_sha256"]
    for i, sha in g["value_sha256"].items():
        assert hashlib.sha256(results[int(i)]).hexdigest() == sha


@pytest.mark.parametrize("case", GOLD["tables"], ids=[c["name"] for c in GOLD["tables"]])
def test_host_parsing_equals_reference_meta_blocks(oracle, case):
    from pebbledb_amd.sstable_bloom import bloom_section_bounds
    from pebbledb_amd.sstable_read import parse_meta_blocks
    _, _, data, _ = table_case(oracle, case)
    meta_offset, bloom_offset, end = bloom_section_bounds(data)
    assert meta_offset == case["meta_block_offset"] and end == len(data) - 8
    metas = parse_meta_blocks(data[meta_offset:bloom_offset])
    assert [list(m) for m in metas] == case["meta_blocks"]
    with pytest.raises(ValueError):
        parse_meta_blocks(data[meta_offset:bloom_offset - 3])  # a section cut inside a meta block


def test_header_declares_the_sstable_read_exports():
    names = set(_native.header_functions())
    new = {"pbf_sst_open", "pbf_sst_close", "pbf_sst_info", "pbf_sst_block_index", "pbf_sst_get", "pbf_sst_gather"}
    assert new <= names and new <= set(_native.SIGNATURES)
    L = _native.lib()
    for name in new:
        assert hasattr(L, name)
    # argument checks that need no device
    assert L.pbf_sst_close(None) == _native.PBF_OK
    assert L.pbf_sst_get(None, 0, None, None, 0, 0, None, 0, None, None, None, None) == _native.PBF_ERR_INVALID
    assert b"no tables" in L.pbf_last_error()
