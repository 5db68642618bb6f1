// Point lookup over SSTables resident in HBM (reference SSTable.get, src/sstable.py:150-187;
// DataBlock.get, src/blocks.py:60-65; the get loop of LsmStorage.get, src/lsm_storage.py:164-179),
// gfx950.
//
// A resident table is its data section (every DataBlock back to back, blocks.py:33-37: records ‖
// u16 offset per record ‖ u16 count) plus a block index the validator writes: per block the
// absolute offset of its first record, of its last record, of its u16 array, and its count,
// and beside it the first 8 bytes of every block's last key.
//
//   * k_sst_validate — one workgroup per block: checks the block's framing (count, u16 offsets,
//     every record's sizes against its extent) and that adjacent keys ascend strictly in unsigned
//     bytewise order, then writes the block's index entry.  After a table passed, every offset a
//     lookup derives from the index and the u16 arrays lies inside the data section, and every
//     record's key and value extents are the ones its header states.
//   * sst_find — the reference's linear walk (first meta block whose last_key >= key, then
//     first_key <= key, then the first record whose key equals the probe) as two binary searches:
//     for strictly ascending keys they give the same answer.  Every loop is bounded by a count
//     from the validated index (at most 32 halvings), never by data found on the way.
//   * k_lsm_get — one lane per key: walks the key's candidate tables in row order and stops at
//     the first that holds it.
//   * k_gather_values — packs the found values into one buffer at the offsets an exclusive scan
//     of their lengths gave: 8 lanes per value, aligned 16-byte stores.
//
// Loads wider than a byte are 8-byte words inside both keys' extents (compare) and 16-byte
// chunks inside the value's extent (gather); the bytes at the ends go one by one.  Nothing is
// read outside a validated extent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloom_kernels.hpp"

namespace pbf {

struct SstBlock {
    uint32_t first_off;  // first record (= the block's start)
    uint32_t last_off;   // last record
    uint32_t u16_off;    // the u16 offset array (= the end of the record area)
    uint32_t count;      // records
};

// Validation outcome (device memory, zeroed before the launch).
struct SstReport {
    unsigned long long records;
    unsigned long long bad_records;       // a record whose sizes do not match its extent
    unsigned long long order_violations;  // adjacent keys of a block not strictly ascending
    unsigned int bad_blocks;              // framing: count, u16 array
    unsigned int rules;                   // kSstRule* of every violation seen
};

constexpr unsigned int kSstRuleCount = 1;     // count >= 1 and 2*count+2 <= block bytes
constexpr unsigned int kSstRuleOffsets = 2;   // offsets[0] == 0, strictly ascending, inside the record area
constexpr unsigned int kSstRuleSizes = 4;     // 8 + key_size + value_size == extent, sizes >= 0
constexpr unsigned int kSstRuleOrder = 8;     // keys strictly ascending (unsigned bytewise)

constexpr uint32_t kSstTablesPerLaunch = 64;

__device__ __forceinline__ uint32_t ld_u16(const uint8_t* p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8); }
__device__ __forceinline__ int32_t ld_i32(const uint8_t* p) {
    return int32_t(uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24));
}
__device__ __forceinline__ uint64_t ld_u64_any(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// The first 8 bytes of a key as a big-endian word, zero-padded: where two keys' words differ, the
// words order as the keys do (a padding zero meets either the same zero byte or a larger one).
__device__ __forceinline__ uint64_t key_prefix(const uint8_t* k, uint32_t kl) {
    if (kl >= 8) return __builtin_bswap64(ld_u64_any(k));
    uint64_t v = 0;
    for (uint32_t j = 0; j < kl; ++j) v |= uint64_t(k[j]) << (56 - 8 * j);
    return v;
}

// memcmp-then-length over unsigned bytes (Python str order for valid UTF-8, as
// lsm_kernels.hpp's cmp_key_bound): <0, 0, >0.  Words of 8 bytes while both keys hold 8 more,
// bytes after.
__device__ __forceinline__ int sst_key_cmp(const uint8_t* a, uint32_t al, const uint8_t* b, uint32_t bl) {
    const uint32_t m = min(al, bl);
    uint32_t off = 0;
    for (; off + 8 <= m; off += 8) {
        const uint64_t x = ld_u64_any(a + off), y = ld_u64_any(b + off);
        if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
    }
    for (; off < m; ++off) {
        const uint32_t x = a[off], y = b[off];
        if (x != y) return x < y ? -1 : 1;
    }
    return al < bl ? -1 : (al > bl ? 1 : 0);
}

// ------------------------------------------------------------------ validation
// Block b = data[block_off[b], block_off[b+1]); the host has checked that block_off ascends from
// 0 to data_len.
__global__ void __launch_bounds__(256) k_sst_validate(const uint8_t* __restrict__ data,
                                                      const uint32_t* __restrict__ block_off, uint32_t nblocks,
                                                      SstBlock* __restrict__ index, uint64_t* __restrict__ last_prefix,
                                                      SstReport* __restrict__ rep) {
    __shared__ unsigned int s_bad, s_rules;
    const uint32_t b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    if (b >= nblocks) return;
    const uint32_t b0 = block_off[b], bs = block_off[b + 1] - b0;
    const uint8_t* blk = data + b0;
    if (tid == 0) {
        s_bad = 0;
        s_rules = 0;
    }
    __syncthreads();
    const uint32_t count = bs >= 2 ? ld_u16(blk + bs - 2) : 0;
    if (count < 1 || 2 * count + 2 > bs) {  // (uniform over the workgroup)
        if (tid == 0) {
            index[b] = SstBlock{0, 0, 0, 0};
            last_prefix[b] = 0;
            atomicAdd(&rep->bad_blocks, 1u);
            atomicOr(&rep->rules, kSstRuleCount);
        }
        return;
    }
    const uint32_t area = bs - 2 * count - 2;  // record bytes; the u16 array starts here
    const uint8_t* offs = blk + area;
    unsigned int bad = 0, rules = 0;
    for (uint32_t i = tid; i < count; i += nt) {
        const uint32_t o = ld_u16(offs + 2 * i);
        const uint32_t next = i + 1 < count ? ld_u16(offs + 2 * (i + 1)) : area;
        if ((i == 0 && o != 0) || o >= next || next > area) {
            ++bad;
            rules |= kSstRuleOffsets;
            continue;
        }
        const uint32_t ext = next - o;
        bool ok = ext >= 8;
        if (ok) {
            const int32_t ks = ld_i32(blk + o);
            ok = ks >= 0 && uint32_t(ks) <= ext - 8;
            if (ok) {
                const int32_t vs = ld_i32(blk + o + 4 + uint32_t(ks));
                ok = vs >= 0 && 8 + uint32_t(ks) + uint32_t(vs) == ext;
            }
        }
        if (!ok) {
            ++bad;
            rules |= kSstRuleSizes;
        }
    }
    if (bad) {
        atomicAdd(&s_bad, bad);
        atomicOr(&s_rules, rules);
    }
    __syncthreads();
    const unsigned int block_bad = s_bad;
    if (block_bad) {  // keys are compared only in a block whose every record is framed
        if (tid == 0) {
            index[b] = SstBlock{0, 0, 0, 0};
            last_prefix[b] = 0;
            if (s_rules & kSstRuleOffsets) atomicAdd(&rep->bad_blocks, 1u);
            atomicAdd(&rep->bad_records, (unsigned long long)block_bad);
            atomicOr(&rep->rules, s_rules);
        }
        return;
    }
    unsigned int viol = 0;
    for (uint32_t i = tid; i + 1 < count; i += nt) {
        const uint8_t* r0 = blk + ld_u16(offs + 2 * i);
        const uint8_t* r1 = blk + ld_u16(offs + 2 * (i + 1));
        if (sst_key_cmp(r0 + 4, uint32_t(ld_i32(r0)), r1 + 4, uint32_t(ld_i32(r1))) >= 0) ++viol;
    }
    if (viol) {
        atomicAdd(&rep->order_violations, (unsigned long long)viol);
        atomicOr(&rep->rules, kSstRuleOrder);
    }
    if (tid == 0) {
        const uint8_t* last = blk + ld_u16(offs + 2 * (count - 1));
        index[b] = SstBlock{b0, uint32_t(last - data), b0 + area, count};
        last_prefix[b] = key_prefix(last + 4, uint32_t(ld_i32(last)));
        atomicAdd(&rep->records, (unsigned long long)count);
    }
}

// last_key(b) < first_key(b+1) for every adjacent block pair, one lane per pair.  Runs only on
// an index whose every block passed k_sst_validate.
__global__ void __launch_bounds__(256) k_sst_validate_seams(const uint8_t* __restrict__ data,
                                                            const SstBlock* __restrict__ index, uint32_t nblocks,
                                                            SstReport* __restrict__ rep) {
    const uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (b + 1 >= nblocks) return;
    const uint8_t* r0 = data + index[b].last_off;
    const uint8_t* r1 = data + index[b + 1].first_off;
    if (sst_key_cmp(r0 + 4, uint32_t(ld_i32(r0)), r1 + 4, uint32_t(ld_i32(r1))) >= 0) {
        atomicAdd(&rep->order_violations, 1ull);
        atomicOr(&rep->rules, kSstRuleOrder);
    }
}

// ------------------------------------------------------------------ lookup
struct SstView {
    const uint8_t* data;
    const SstBlock* index;
    const uint64_t* last_prefix;  // key_prefix of every block's last key
    uint32_t nblocks;
};

__device__ __forceinline__ SstBlock ld_block(const SstBlock* p) {
    const uint4 v = gld(reinterpret_cast<const uint4*>(p));
    return SstBlock{v.x, v.y, v.z, v.w};
}

// SSTable.get(key): true and the value's (offset into the data section, length) when the table
// holds the key.
__device__ __forceinline__ bool sst_find(const SstView& t, const uint8_t* key, uint32_t kl, uint64_t kpre,
                                         uint64_t* val_off, int32_t* val_len) {
    // find_block_id (sstable.py:150-159): the first block whose last key >= key ...  A step is
    // decided by the last key's 8-byte prefix (one load) wherever it differs from the probe's
    // (kpre = key_prefix(key)); only equal prefixes read the record.
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
    if (lo >= t.nblocks) return false;
    const SstBlock blk = ld_block(t.index + lo);
    // ... holds the key only if its first key <= key
    const uint8_t* f = t.data + blk.first_off;
    if (sst_key_cmp(key, kl, f + 4, uint32_t(ld_i32(f))) < 0) return false;
    // DataBlock.get (blocks.py:60-65): the record whose key equals the probe
    const uint8_t* offs = t.data + blk.u16_off;
    uint32_t a = 0, b = blk.count;
    for (int it = 0; it < 32 && a < b; ++it) {
        const uint32_t mid = a + ((b - a) >> 1);
        const uint8_t* r = t.data + blk.first_off + ld_u16(offs + 2 * mid);
        const uint32_t ks = uint32_t(ld_i32(r));
        const int c = sst_key_cmp(r + 4, ks, key, kl);
        if (c == 0) {
            *val_len = ld_i32(r + 4 + ks);
            *val_off = uint64_t(r + 8 + ks - t.data);
            return true;
        }
        if (c < 0)
            a = mid + 1;
        else
            b = mid;
    }
    return false;
}

// Tables [t0, t0 + nt) of one launch, by value in the kernel arguments (no per-call upload).
struct SstSet {
    const uint8_t* data[kSstTablesPerLaunch];
    const SstBlock* index[kSstTablesPerLaunch];
    const uint64_t* last_prefix[kSstTablesPerLaunch];
    const uint8_t* mask[kSstTablesPerLaunch];  // LSB-first candidate mask of the batch, or null = every key
    uint32_t nblocks[kSstTablesPerLaunch];
    uint32_t t0, nt;
    uint32_t first;  // the first launch of a call initialises the outputs
};

// LsmStorage.get's walk (lsm_storage.py:164-179) for a batch: key i reads its candidate tables
// in row order and stops at the first that holds it.  table[i] = that row or -1; val_off[i] the
// value's offset in that table's data section; val_len[i] its length, -1 if absent (0 is a
// stored empty value).
template <int KM>
__global__ void __launch_bounds__(256) k_lsm_get(KeySet ks, uint64_t n, SstSet set, int32_t* __restrict__ table,
                                                 uint64_t* __restrict__ val_off, int32_t* __restrict__ val_len) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (!set.first && table[i] >= 0) continue;  // an earlier launch's tables hold it
        const uint8_t* kp;
        uint32_t kl;
        if constexpr (KM == kVar) {
            const uint64_t o0 = gld(ks.off0), a = gld(ks.offsets + i);
            kp = ks.data + (a - o0);
            kl = uint32_t(gld(ks.offsets + i + 1) - a);
        } else {
            kp = ks.data + i * uint64_t(ks.key_len);
            kl = ks.key_len;
        }
        const uint64_t kpre = key_prefix(kp, kl);
        int32_t tf = -1, vl = -1;
        uint64_t vo = 0;
        for (uint32_t t = 0; t < set.nt; ++t) {
            const uint8_t* m = set.mask[t];
            if (m && !((m[i >> 3] >> (i & 7)) & 1u)) continue;
            const SstView v{set.data[t], set.index[t], set.last_prefix[t], set.nblocks[t]};
            if (sst_find(v, kp, kl, kpre, &vo, &vl)) {
                tf = int32_t(set.t0 + t);
                break;
            }
        }
        if (tf < 0) {
            vl = -1;
            vo = 0;
        }
        if (set.first || tf >= 0) {
            table[i] = tf;
            val_off[i] = vo;
            val_len[i] = vl;
        }
    }
}

// ------------------------------------------------------------------ gather
struct SstDataSet {
    const uint8_t* data[kSstTablesPerLaunch];
    uint32_t data_len[kSstTablesPerLaunch];
    uint32_t t0, nt;
};

// value_offsets[n+1] = the exclusive scan of max(val_len, 0), closed by the total, in three
// launches: the sum of every tile of kScanTile lengths, the exclusive scan of those sums (one
// workgroup), and the offsets inside every tile.  (rocPRIM's device scan would do, but its host
// dispatch carries the names of every architecture it knows, and this library is gfx950 only.)
constexpr uint32_t kScanThreads = 256, kScanPer = 8, kScanTile = kScanThreads * kScanPer;

__device__ __forceinline__ uint64_t len_at(const int32_t* __restrict__ val_len, uint64_t i, uint64_t n) {
    if (i >= n) return 0;
    const int32_t v = val_len[i];
    return v > 0 ? uint64_t(v) : 0;
}

// One value per thread of a kScanThreads workgroup: returns the thread's exclusive prefix,
// *total = the workgroup's sum.  sh holds kScanThreads words and is free again on return.
__device__ __forceinline__ uint64_t block_exclusive(uint64_t v, uint64_t* sh, uint64_t* total) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t add = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const uint64_t incl = sh[tid];
    *total = sh[kScanThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(kScanThreads) k_len_tile_sums(const int32_t* __restrict__ val_len, uint64_t n,
                                                                uint64_t* __restrict__ sums) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    uint64_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) s += len_at(val_len, base + j, n);
    uint64_t tot;
    block_exclusive(s, sh, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// In place: sums[t] becomes the offset of tile t.  One workgroup.
__global__ void __launch_bounds__(kScanThreads) k_len_tile_scan(uint64_t* __restrict__ sums, uint64_t ntiles) {
    __shared__ uint64_t sh[kScanThreads];
    uint64_t carry = 0;
    for (uint64_t c = 0; c < ntiles; c += kScanThreads) {
        const uint64_t i = c + threadIdx.x;
        uint64_t tot;
        const uint64_t ex = block_exclusive(i < ntiles ? sums[i] : 0, sh, &tot);
        if (i < ntiles) sums[i] = carry + ex;
        carry += tot;
    }
}

__global__ void __launch_bounds__(kScanThreads) k_len_offsets(const int32_t* __restrict__ val_len, uint64_t n,
                                                              const uint64_t* __restrict__ sums,
                                                              uint64_t* __restrict__ offs) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    uint64_t l[kScanPer], s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
        l[j] = len_at(val_len, base + j, n);
        s += l[j];
    }
    uint64_t tot;
    uint64_t run = sums[blockIdx.x] + block_exclusive(s, sh, &tot);
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
        const uint64_t i = base + j;
        if (i < n) {
            offs[i] = run;
            run += l[j];
            if (i == n - 1) offs[n] = run;
        }
    }
}

constexpr uint32_t kGatherLanes = 8;  // lanes per value

// out[offs[i], offs[i+1]) = value i, for the values of tables [t0, t0 + nt).  An entry that does
// not lie inside its table's data section is not copied and counts in *err.
__global__ void __launch_bounds__(256) k_gather_values(SstDataSet set, const int32_t* __restrict__ table,
                                                       const uint64_t* __restrict__ val_off,
                                                       const int32_t* __restrict__ val_len, uint64_t n,
                                                       const uint64_t* __restrict__ offs, uint8_t* __restrict__ out,
                                                       uint32_t ntables, unsigned int* __restrict__ err) {
    const uint32_t lane = threadIdx.x % kGatherLanes;
    const uint64_t groups = uint64_t(gridDim.x) * (blockDim.x / kGatherLanes);
    for (uint64_t i = uint64_t(blockIdx.x) * (blockDim.x / kGatherLanes) + threadIdx.x / kGatherLanes; i < n;
         i += groups) {
        const int32_t len = val_len[i];
        if (len <= 0) continue;
        const int32_t t = table[i];
        if (t < 0 || uint32_t(t) >= ntables) {
            if (lane == 0 && set.t0 == 0) atomicAdd(err, 1u);
            continue;
        }
        if (uint32_t(t) < set.t0 || uint32_t(t) >= set.t0 + set.nt) continue;
        const uint64_t so = val_off[i];
        if (so > set.data_len[t - set.t0] || uint64_t(len) > set.data_len[t - set.t0] - so) {
            if (lane == 0) atomicAdd(err, 1u);
            continue;
        }
        const uint8_t* src = set.data[t - set.t0] + so;
        uint8_t* dst = out + offs[i];
        const uint32_t L = uint32_t(len);
        // bytes up to dst's first 16-byte boundary, whole 16-byte chunks (source loads inside
        // the value), then the tail bytes
        const uint32_t head = min(L, uint32_t((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15));
        const uint32_t nq = (L - head) / 16;
        for (uint32_t j = lane; j < head; j += kGatherLanes) dst[j] = src[j];
        for (uint32_t q = lane; q < nq; q += kGatherLanes) {
            uint4 v;
            __builtin_memcpy(&v, src + head + 16 * q, 16);
            *reinterpret_cast<uint4*>(dst + head + 16 * q) = v;
        }
        for (uint32_t j = head + 16 * nq + lane; j < L; j += kGatherLanes) dst[j] = src[j];
    }
}

}  // namespace pbf
