// Compaction's record run over SSTables resident in HBM (reference MergingIterator /
// ConcatenatingIterator over SSTableIterators, src/iterators.py:110-207, as
// force_compaction_l0 / force_compaction_l1_or_more_level feed them to _compact,
// src/lsm_storage.py:253-284), gfx950.
//
// The reference pops a heap keyed (key, iterator index) and drops a record whose key equals the
// previous one's: the run is every distinct key in ascending unsigned bytewise order, each with
// the record of the lowest table index that stores it.  Here the merge is by rank, with no
// sequential step: every input record finds its own place.
//
//   * sst_lower_bound — the table-wide index of a table's first record whose key is >= the
//     probe, and whether that key equals it: sst_find's two binary searches (blocks by
//     last_prefix, records by the u16 array), plus rec_base[nblocks+1], the prefix sum of the
//     validated index's block counts.
//   * merge_record_at — record i of a table: its block by a binary search over rec_base, its slot
//     through the block's u16 array.  The scan's kernels walk to their records with it too.
//   * k_merge_rank — one lane per input record (t, i): rank = i + sum over u<t of (lb_u + eq_u)
//     + sum over u>t of lb_u is the record's place among ALL input records ordered by (key,
//     table), a permutation of [0, N); keep = no table u<t holds the key.  Concatenate mode runs
//     no search: rank = the records of the tables before t, plus i.  The lane writes
//     slots[rank].
//   * k_merge_tile_sums / k_merge_tile_scan / k_merge_offsets — exclusive scans over the slots in
//     rank order (the three-launch scan of sstable_read_kernels.hpp, three sums at once): a kept
//     record's output index, key byte offset and value byte offset.
//   * k_merge_copy — 8 lanes per kept slot copy its key and value bytes (k_gather_values' rules:
//     bytes up to the destination's 16-byte boundary, aligned 16-byte stores whose source loads
//     lie inside the record, then the tail bytes).
//
// Every loop is bounded by a count from the validated index (at most 32 halvings) or by a byte
// count the validator checked against the record's extent.  Nothing is read outside a validated
// extent; the host launches k_merge_offsets / k_merge_copy only after the totals fit the
// caller's capacities.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sstable_read_kernels.hpp"

namespace pbf {

// The input tables of one merge, by value in the kernel arguments (as SstSet).
struct MergeSet {
    const uint8_t* data[kSstTablesPerLaunch];
    const SstBlock* index[kSstTablesPerLaunch];
    const uint64_t* last_prefix[kSstTablesPerLaunch];
    const uint32_t* rec_base[kSstTablesPerLaunch];  // [nblocks+1]: records before each block
    uint32_t nblocks[kSstTablesPerLaunch];
    uint64_t in_base[kSstTablesPerLaunch];  // records of the tables before this one
    uint32_t nt;
};

// One input record at its rank.
struct MergeSlot {
    uint32_t rec_off;  // the record's offset in its table's data section
    uint32_t klen, vlen;
    uint32_t table_keep;  // table | keep << 31
};
constexpr uint32_t kMergeKeep = 0x80000000u;

// totals[]: records kept, their key bytes, their value bytes
constexpr uint32_t kMergeTotals = 3;

// The first record of table t whose key >= the probe: its table-wide index in [0, nrecords], and
// *eq = its key equals the probe.
__device__ __forceinline__ uint32_t sst_lower_bound(const SstView& t, const uint32_t* __restrict__ rec_base,
                                                    const uint8_t* key, uint32_t kl, uint64_t kpre, bool* eq) {
    *eq = false;
    // the first block whose last key >= key (sst_find's block search)
    uint32_t lo = 0, hi = t.nblocks;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t lp = gld(t.last_prefix + mid);
        bool less = lp < kpre;
        if (lp == kpre) {
            const uint8_t* r = t.data + gld(&t.index[mid].last_off);
            less = sst_key_cmp(r + 4, uint32_t(ld_i32(r)), key, kl) < 0;
        }
        if (less)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= t.nblocks) return gld(rec_base + t.nblocks);  // every key is below the probe
    const SstBlock blk = ld_block(t.index + lo);
    const uint8_t* offs = t.data + blk.u16_off;
    // the block's first record whose key >= key: it exists, the block's last key is one
    uint32_t a = 0, b = blk.count;
    for (int it = 0; it < 32 && a < b; ++it) {
        const uint32_t mid = a + ((b - a) >> 1);
        const uint8_t* r = t.data + blk.first_off + ld_u16(offs + 2 * mid);
        const int c = sst_key_cmp(r + 4, uint32_t(ld_i32(r)), key, kl);
        if (c == 0) {  // keys ascend strictly: this is the only one
            *eq = true;
            a = mid;
            break;
        }
        if (c < 0)
            a = mid + 1;
        else
            b = mid;
    }
    return gld(rec_base + lo) + a;
}

// Record i of table t (its block through rec_base, its slot through the u16 array): the record's
// offset in the data section, *kl / *vl = its header.  The one record walk: k_merge_rank,
// k_scan_rank and k_scan_sizes (sstable_scan_kernels.hpp) all find their record here.
__device__ __forceinline__ uint32_t merge_record_at(const MergeSet& set, uint32_t t, uint32_t i, uint32_t* kl,
                                                    uint32_t* vl) {
    const uint32_t* rb = set.rec_base[t];
    uint32_t lo = 0, hi = set.nblocks[t];  // rec_base[lo] <= i < rec_base[hi]
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (gld(rb + mid) <= i)
            lo = mid;
        else
            hi = mid;
    }
    const SstBlock blk = ld_block(set.index[t] + lo);
    const uint32_t slot = min(i - gld(rb + lo), blk.count - 1);  // (inside the block whatever rec_base holds)
    const uint8_t* data = set.data[t];
    const uint32_t rec_off = blk.first_off + ld_u16(data + blk.u16_off + 2 * slot);
    const uint8_t* r = data + rec_off;
    *kl = uint32_t(ld_i32(r));
    *vl = uint32_t(ld_i32(r + 4 + *kl));
    return rec_off;
}

// dedup = 1: MergingIterator; 0: ConcatenatingIterator.  n = the tables' records together.
__global__ void __launch_bounds__(256) k_merge_rank(MergeSet set, uint64_t n, int dedup, MergeSlot* __restrict__ slots) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        // the lane's table: the last t with in_base[t] <= g
        uint32_t t = 0;
        for (uint32_t u = 1; u < set.nt; ++u) t += set.in_base[u] <= g;
        const uint32_t i = uint32_t(g - set.in_base[t]);
        uint32_t kl, vl;
        const uint32_t rec_off = merge_record_at(set, t, i, &kl, &vl);
        const uint8_t* key = set.data[t] + rec_off + 4;
        uint64_t rank = g;
        uint32_t keep = kMergeKeep;
        if (dedup) {
            const uint64_t kpre = key_prefix(key, kl);
            rank = i;
            for (uint32_t u = 0; u < set.nt; ++u) {
                if (u == t) continue;
                const SstView v{set.data[u], set.index[u], set.last_prefix[u], set.nblocks[u]};
                bool eq;
                const uint32_t lb = sst_lower_bound(v, set.rec_base[u], key, kl, kpre, &eq);
                rank += lb;
                if (u < t && eq) {  // table u's copy comes first and is the one that survives
                    rank += 1;
                    keep = 0;
                }
            }
        }
        if (rank < n) slots[rank] = MergeSlot{rec_off, kl, vl, t | keep};
    }
}

// ------------------------------------------------------------------ scans over the slots
struct MergeSums {
    uint64_t cnt, kb, vb;
};

__device__ __forceinline__ MergeSums merge_slot_sums(const MergeSlot* __restrict__ slots, uint64_t r, uint64_t n) {
    if (r >= n) return MergeSums{0, 0, 0};
    const uint4 s = gld(reinterpret_cast<const uint4*>(slots + r));
    if (!(s.w & kMergeKeep)) return MergeSums{0, 0, 0};
    return MergeSums{1, s.y, s.z};
}

// sums[c * ntiles + tile], c = 0 (records kept), 1 (key bytes), 2 (value bytes)
__global__ void __launch_bounds__(kScanThreads) k_merge_tile_sums(const MergeSlot* __restrict__ slots, uint64_t n,
                                                                  uint64_t* __restrict__ sums, uint64_t ntiles) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    MergeSums s{0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
        const MergeSums x = merge_slot_sums(slots, base + j, n);
        s.cnt += x.cnt;
        s.kb += x.kb;
        s.vb += x.vb;
    }
    uint64_t tc, tk, tv;
    block_exclusive(s.cnt, sh, &tc);
    block_exclusive(s.kb, sh, &tk);
    block_exclusive(s.vb, sh, &tv);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = tc;
        sums[ntiles + blockIdx.x] = tk;
        sums[2 * ntiles + blockIdx.x] = tv;
    }
}

// In place: every sum becomes its tile's offset; totals[c] = the sum over all tiles.  One
// workgroup.
__global__ void __launch_bounds__(kScanThreads) k_merge_tile_scan(uint64_t* __restrict__ sums, uint64_t ntiles,
                                                                  uint64_t* __restrict__ totals) {
    __shared__ uint64_t sh[kScanThreads];
    for (uint32_t c = 0; c < kMergeTotals; ++c) {
        uint64_t* s = sums + c * ntiles;
        uint64_t carry = 0;
        for (uint64_t c0 = 0; c0 < ntiles; c0 += kScanThreads) {
            const uint64_t i = c0 + threadIdx.x;
            uint64_t tot;
            const uint64_t ex = block_exclusive(i < ntiles ? s[i] : 0, sh, &tot);
            if (i < ntiles) s[i] = carry + ex;
            carry += tot;
        }
        if (threadIdx.x == 0) totals[c] = carry;
    }
}

// For every kept slot r: pos[r] = its output index j, key_offsets[j] / value_offsets[j] = its
// byte offsets.  (The host has checked the totals against the offsets arrays' capacity.)
__global__ void __launch_bounds__(kScanThreads) k_merge_offsets(const MergeSlot* __restrict__ slots, uint64_t n,
                                                                const uint64_t* __restrict__ sums, uint64_t ntiles,
                                                                uint64_t* __restrict__ pos,
                                                                uint64_t* __restrict__ key_offsets,
                                                                uint64_t* __restrict__ value_offsets) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    MergeSums x[kScanPer], s{0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
        x[j] = merge_slot_sums(slots, base + j, n);
        s.cnt += x[j].cnt;
        s.kb += x[j].kb;
        s.vb += x[j].vb;
    }
    uint64_t tot;
    uint64_t rc = sums[blockIdx.x] + block_exclusive(s.cnt, sh, &tot);
    uint64_t rk = sums[ntiles + blockIdx.x] + block_exclusive(s.kb, sh, &tot);
    uint64_t rv = sums[2 * ntiles + blockIdx.x] + block_exclusive(s.vb, sh, &tot);
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
        if (base + j < n && x[j].cnt) {
            pos[base + j] = rc;
            key_offsets[rc] = rk;
            value_offsets[rc] = rv;
            rc += 1;
            rk += x[j].kb;
            rv += x[j].vb;
        }
    }
}

// dst[0, len) = src[0, len) by the lanes of one group: bytes up to dst's first 16-byte boundary,
// whole 16-byte chunks (source loads inside [src, src + len)), then the tail bytes.
__device__ __forceinline__ void merge_copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane) {
    const uint32_t head = min(len, uint32_t((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15));
    const uint32_t nq = (len - head) / 16;
    for (uint32_t j = lane; j < head; j += kGatherLanes) dst[j] = src[j];
    for (uint32_t q = lane; q < nq; q += kGatherLanes) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * q, 16);
        *reinterpret_cast<uint4*>(dst + head + 16 * q) = v;
    }
    for (uint32_t j = head + 16 * nq + lane; j < len; j += kGatherLanes) dst[j] = src[j];
}

// keys_out[key_offsets[j], +klen) and values_out[value_offsets[j], +vlen) of every kept slot
// (j = pos[r]); the first lane closes both offsets arrays with the totals.
__global__ void __launch_bounds__(256) k_merge_copy(MergeSet set, const MergeSlot* __restrict__ slots, uint64_t n,
                                                    const uint64_t* __restrict__ pos,
                                                    const uint64_t* __restrict__ totals,
                                                    uint64_t* __restrict__ key_offsets,
                                                    uint64_t* __restrict__ value_offsets,
                                                    uint8_t* __restrict__ keys_out, uint8_t* __restrict__ values_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        key_offsets[totals[0]] = totals[1];
        value_offsets[totals[0]] = totals[2];
    }
    const uint32_t lane = threadIdx.x % kGatherLanes;
    const uint64_t groups = uint64_t(gridDim.x) * (blockDim.x / kGatherLanes);
    for (uint64_t r = uint64_t(blockIdx.x) * (blockDim.x / kGatherLanes) + threadIdx.x / kGatherLanes; r < n;
         r += groups) {
        const uint4 s = gld(reinterpret_cast<const uint4*>(slots + r));
        if (!(s.w & kMergeKeep)) continue;
        const uint32_t t = s.w & ~kMergeKeep;
        if (t >= set.nt) continue;
        const uint64_t j = pos[r];
        const uint8_t* rec = set.data[t] + s.x;
        if (s.y) merge_copy_bytes(keys_out + key_offsets[j], rec + 4, s.y, lane);
        if (s.z) merge_copy_bytes(values_out + value_offsets[j], rec + 8 + s.y, s.z, lane);
    }
}

}  // namespace pbf
