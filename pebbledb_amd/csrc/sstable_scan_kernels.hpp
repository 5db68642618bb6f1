// Range scan over SSTables resident in HBM (reference SSTable.scan, src/sstable.py:189; the
// bounded SSTableIterator, src/iterators.py:58-141; the MergingIterator LsmStorage.scan yields
// from, src/lsm_storage.py:187-190), gfx950.
//
// A batch is Q ranges [lower_q, upper_q] (inclusive at both ends; upper_open_q = no upper bound)
// over T tables.  Segment s = q * T + t is table t's record window [lo, hi) for range q; a
// bounded scan is the rank merge of sstable_merge_kernels.hpp restricted to those windows, all
// ranges in one launch, every selected record finding its own place.
//
//   * k_scan_bounds — one lane per segment: lo = sst_lower_bound(lower), hi = nrecords (open) or
//     sst_lower_bound(upper) + (upper is stored), hi = max(hi, lo).  Writes seg_lo, seg_cnt.
//   * the exclusive scan of seg_cnt into seg_base[Q*T + 1] is sstable_read_kernels.hpp's
//     k_len_tile_sums / k_len_tile_scan / k_len_offsets as they stand: a count is below 2^31 (a
//     data section is at most 2 GiB - 1 and a record at least 8 bytes), so the u32 counts are
//     read as the non-negative i32 lengths those kernels scan.  seg_base[Q*T] = N, the selected
//     input records.
//   * k_scan_sizes — the key and value bytes of the N selected records (before de-duplication).
//   * k_scan_rank — one lane per selected record g: its segment is the last s with
//     seg_base[s] <= g (empty segments share a base: the last one is the one that holds g),
//     j = g - seg_base[s], table-wide index i = seg_lo[s] + j (the record itself through
//     sstable_merge_kernels.hpp's merge_record_at, as in k_merge_rank and k_scan_sizes);
//         rank = seg_base[q*T] + j + sum over u<t of (lb_u + eq_u - lo_u) + sum over u>t of (lb_u - lo_u)
//         keep = no table u<t holds the key
//     where (lb_u, eq_u) = sst_lower_bound(table u, key) and lo_u = seg_lo[q*T + u].  The key lies
//     in [lower, upper], so lo_u <= lb_u and lb_u + eq_u <= hi_u: every term counts records of
//     table u's window that order before (key, t), and the ranks of one range are a permutation
//     of [seg_base[q*T], seg_base[(q+1)*T]).  A table whose window is empty contributes 0 and is
//     not searched (lb_u == lo_u there).  The lane writes slots[rank]; the slots were zeroed, and
//     a rank outside its range's span is dropped.
//   * k_merge_tile_sums / k_merge_tile_scan / k_merge_offsets / k_merge_copy run over the N slots
//     unchanged.
//   * k_scan_range_offsets — range_offsets[q] = the kept records before slot seg_base[q*T],
//     closed by the total: range q is records [range_offsets[q], range_offsets[q+1]) of the run.
//
// Neighbouring lanes of k_scan_rank hold neighbouring records of one segment, so their searches
// walk the same blocks of the other tables.  Every loop is bounded by a validated count, by 32
// halvings or by kScanTile; nothing is read outside a validated extent or the bounds' own bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sstable_merge_kernels.hpp"

namespace pbf {

// The ranges of one batch, in device memory: bound q = bytes[offsets[q] - offsets[0],
// offsets[q+1] - offsets[0]).
struct ScanBounds {
    const uint8_t* lowers;
    const uint64_t* lower_offsets;  // [nranges+1]
    const uint8_t* uppers;
    const uint64_t* upper_offsets;  // [nranges+1]
    const uint8_t* upper_open;      // [nranges], or null: every range has its upper bound
};

// totals of k_scan_sizes: key bytes, value bytes
constexpr uint32_t kScanSizeTotals = 2;

__global__ void __launch_bounds__(256) k_scan_bounds(MergeSet set, ScanBounds b, uint64_t nseg,
                                                     uint32_t* __restrict__ seg_lo, uint32_t* __restrict__ seg_cnt) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint64_t l0 = gld(b.lower_offsets), u0 = gld(b.upper_offsets);
    for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        const uint64_t q = s / set.nt;
        const uint32_t t = uint32_t(s - q * set.nt);
        const SstView v{set.data[t], set.index[t], set.last_prefix[t], set.nblocks[t]};
        const uint32_t* rb = set.rec_base[t];
        const uint64_t la = gld(b.lower_offsets + q), lb = gld(b.lower_offsets + q + 1);
        const uint8_t* lk = b.lowers + (la - l0);
        const uint32_t ll = uint32_t(lb - la);
        bool eq;
        const uint32_t lo = sst_lower_bound(v, rb, lk, ll, key_prefix(lk, ll), &eq);
        uint32_t hi;
        if (b.upper_open && b.upper_open[q]) {
            hi = gld(rb + v.nblocks);
        } else {
            const uint64_t ua = gld(b.upper_offsets + q), ub = gld(b.upper_offsets + q + 1);
            const uint8_t* uk = b.uppers + (ua - u0);
            const uint32_t ul = uint32_t(ub - ua);
            hi = sst_lower_bound(v, rb, uk, ul, key_prefix(uk, ul), &eq);
            hi += eq ? 1u : 0u;
        }
        hi = max(hi, lo);  // lower > upper: nothing
        seg_lo[s] = lo;
        seg_cnt[s] = hi - lo;
    }
}

// The segment of selected record g < seg_base[nseg]: the last s with seg_base[s] <= g.
__device__ __forceinline__ uint64_t scan_segment_of(const uint64_t* __restrict__ seg_base, uint64_t nseg, uint64_t g) {
    uint64_t lo = 0, hi = nseg;  // seg_base[lo] <= g < seg_base[hi]
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (gld(seg_base + mid) <= g)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// totals[0] += the key bytes, totals[1] += the value bytes of the n selected records (totals
// zeroed before the launch).
__global__ void __launch_bounds__(kScanThreads) k_scan_sizes(MergeSet set, const uint64_t* __restrict__ seg_base,
                                                             const uint32_t* __restrict__ seg_lo, uint64_t nseg,
                                                             uint64_t n, unsigned long long* __restrict__ totals) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    uint64_t kb = 0, vb = 0;
    for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint64_t s = scan_segment_of(seg_base, nseg, g);
        const uint32_t t = uint32_t(s % set.nt);
        const uint32_t i = gld(seg_lo + s) + uint32_t(g - gld(seg_base + s));
        uint32_t kl, vl;
        merge_record_at(set, t, i, &kl, &vl);
        kb += kl;
        vb += vl;
    }
    uint64_t tk, tv;
    block_exclusive(kb, sh, &tk);
    block_exclusive(vb, sh, &tv);
    if (threadIdx.x == 0) {
        if (tk) atomicAdd(totals, static_cast<unsigned long long>(tk));
        if (tv) atomicAdd(totals + 1, static_cast<unsigned long long>(tv));
    }
}

// n = seg_base[nseg], the selected records; slots[n] zeroed before the launch.
__global__ void __launch_bounds__(256) k_scan_rank(MergeSet set, const uint64_t* __restrict__ seg_base,
                                                   const uint32_t* __restrict__ seg_lo,
                                                   const uint32_t* __restrict__ seg_cnt, uint64_t nseg, uint64_t n,
                                                   MergeSlot* __restrict__ slots) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint64_t s = scan_segment_of(seg_base, nseg, g);
        const uint32_t t = uint32_t(s % set.nt);
        const uint64_t s0 = s - t;  // q * T
        const uint32_t j = uint32_t(g - gld(seg_base + s));
        uint32_t kl, vl;
        const uint32_t rec_off = merge_record_at(set, t, gld(seg_lo + s) + j, &kl, &vl);
        const uint8_t* key = set.data[t] + rec_off + 4;
        const uint64_t kpre = key_prefix(key, kl);
        const uint64_t first = gld(seg_base + s0), end = gld(seg_base + s0 + set.nt);  // the range's span
        uint64_t rank = first + j;
        uint32_t keep = kMergeKeep;
        for (uint32_t u = 0; u < set.nt; ++u) {
            if (u == t || gld(seg_cnt + s0 + u) == 0) continue;  // an empty window holds nothing below the key
            const SstView v{set.data[u], set.index[u], set.last_prefix[u], set.nblocks[u]};
            bool eq;
            const uint32_t lb = sst_lower_bound(v, set.rec_base[u], key, kl, kpre, &eq);
            rank += lb - gld(seg_lo + s0 + u);
            if (u < t && eq) {  // table u's copy comes first and is the one that survives
                rank += 1;
                keep = 0;
            }
        }
        if (rank >= first && rank < end) slots[rank] = MergeSlot{rec_off, kl, vl, t | keep};
    }
}

// After k_merge_offsets: range_offsets[q] = the kept slots before slot seg_base[q * T], q in
// [0, nranges]; sums = the tile offsets of the kept count (the first ntiles words of
// k_merge_tile_scan's array), totals[0] = the run's records.  A range's first slot holds its
// lowest (key, table) and is kept, so pos names its place; a start that is not kept (a slot no
// record claimed) is counted from its tile's offset instead.
__global__ void __launch_bounds__(256) k_scan_range_offsets(const uint64_t* __restrict__ seg_base, uint32_t nt,
                                                            uint64_t nranges, const MergeSlot* __restrict__ slots,
                                                            uint64_t n, const uint64_t* __restrict__ pos,
                                                            const uint64_t* __restrict__ sums,
                                                            const uint64_t* __restrict__ totals,
                                                            uint64_t* __restrict__ range_offsets) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t q = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; q <= nranges; q += stride) {
        const uint64_t r = q < nranges ? gld(seg_base + q * nt) : n;
        uint64_t out;
        if (r >= n) {
            out = totals[0];
        } else if (gld(reinterpret_cast<const uint4*>(slots + r)).w & kMergeKeep) {
            out = pos[r];
        } else {
            const uint64_t tile = r / kScanTile;
            out = sums[tile];
            for (uint64_t x = tile * kScanTile; x < r; ++x)
                out += (gld(reinterpret_cast<const uint4*>(slots + x)).w & kMergeKeep) ? 1 : 0;
        }
        range_offsets[q] = out;
    }
}

}  // namespace pbf
