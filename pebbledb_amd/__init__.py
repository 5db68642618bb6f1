"""pebbledb_amd — MI355X-native bloom-filter engine for pebbledb's per-SSTable filter path.

Drop-in for MaudGautier/pebbledb ``src/bloom_filter.py`` (``BloomFilter``), backed by
hand-written HIP kernels for gfx950 in ``libpebblebloom.so`` (C-ABI: include/pebblebloom.h).
"""
from .bloom_filter import BloomFilter, may_contain_multi, may_contain_set, probe_multi_device, set_default_device
from .compaction import (compact_l0, compact_l0_resident, compact_level, compact_level_resident, concat_tables,
                         merge_tables)
from .device_memtable import DeviceMemTable
from .keys import PackedKeys
from .lsm_scan import count_ranges, scan_ranges, scan_tables
from .memtable import flush_log, flush_log_resident, flush_wal, flush_wal_resident, sort_log
from .sstable_read import DeviceSSTable

__all__ = ["BloomFilter", "DeviceMemTable", "DeviceSSTable", "PackedKeys", "compact_l0", "compact_l0_resident",
           "compact_level", "compact_level_resident", "concat_tables", "count_ranges", "flush_log",
           "flush_log_resident", "flush_wal", "flush_wal_resident", "may_contain_multi", "may_contain_set",
           "merge_tables", "probe_multi_device", "scan_ranges", "scan_tables", "set_default_device", "sort_log"]
