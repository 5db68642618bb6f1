/*
 * pebblebloom — C-ABI of the MI355X bloom-filter engine (libpebblebloom.so).
 *
 * Drop-in boundary for MaudGautier/pebbledb's per-SSTable filter, src/bloom_filter.py.  The
 * reference has no FFI layer: its boundary is the Python class BloomFilter, whose callers are
 * src/sstable.py:274 (build), :82 (to_bytes), :100 (from_bytes), :146 (__eq__) and
 * src/lsm_storage.py:165,175 (may_contain).  pebbledb_amd/bloom_filter.py keeps that class's
 * surface and binds every entry point below through ctypes.
 *
 * Conventions
 *   - All functions return 0 (PBF_OK) or a negative PBF_ERR_*; pbf_last_error() gives the
 *     message of the last failure on the calling thread.
 *   - Keys are UTF-8 bytes (bloom_filter.py:43).  A batch is either fixed-width (key i =
 *     keys[i*key_len, (i+1)*key_len)) or variable-length (offsets has n+1 entries, key i is
 *     offsets[i+1] - offsets[i] bytes).  offsets[0] may be non-zero (a window of a larger
 *     batch): with host pointers `keys` is the buffer the offsets index (key i =
 *     keys[offsets[i], offsets[i+1])); with device pointers `keys` is the window's first byte
 *     (key i = keys[offsets[i] - offsets[0], offsets[i+1] - offsets[0])).
 *   - keys_on_device = 0: keys/offsets/hitmask are host pointers; the call copies what it needs
 *     (pinned staging + hipMemcpyAsync) and returns when the host buffers may be reused.
 *     keys_on_device = 1: they are device pointers on the filter's device; the call is
 *     asynchronous on the filter's stream (pbf_stream) and the caller keeps them alive until
 *     pbf_sync (or an event recorded on that stream) completes.
 *   - A handle is one filter on one device with one HIP stream.  Calls that build, load or
 *     batch-probe take the handle's lock exclusively; one-key probes (pbf_may_contain,
 *     pbf_may_contain_set) of a built filter take it SHARED and run on a per-thread reader
 *     stream, so reader threads probe one filter concurrently (the reference builds a filter
 *     under the flush mutex, lsm_storage.py:220, and then probes it from any reader thread
 *     without a lock, lsm_storage.py:153-179); distinct handles run concurrently.
 *   - Working memory of the tiled pipelines and the host staging path is a per-device pool
 *     shared by all handles (pbf_trim releases it), not per-filter: a long-lived filter holds
 *     only its bitmap.
 */
#ifndef PEBBLEBLOOM_H
#define PEBBLEBLOOM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBF_OK 0
#define PBF_ERR_INVALID (-1)   /* bad argument (null handle or pointer, size mismatch) */
#define PBF_ERR_HIP (-2)       /* a HIP runtime call failed */
#define PBF_ERR_ZERO_SIZE (-3) /* nb_bytes == 0: the reference raises ZeroDivisionError at
                                  `hashed_key % self.bits_size` (bloom_filter.py:47) */

/* Build strategies (pbf_set_build_mode).  All give bit-identical bitmaps. */
#define PBF_BUILD_AUTO 0
#define PBF_BUILD_ATOMIC 1 /* one lane per key, k global atomicOr */
#define PBF_BUILD_TILED 2  /* partition positions by LDS tile, OR in LDS, write tiles once */

/* Probe strategies (pbf_set_probe_mode).  All give identical hit masks. */
#define PBF_PROBE_AUTO 0
#define PBF_PROBE_DIRECT 1 /* one lane per key, k random word loads, wave ballot */
#define PBF_PROBE_TILED 2  /* partition (key, position) entries by LDS tile, test in LDS, gather */

/* What the last probe ran (pbf_last_probe_detail): bit flags | (filters per fused gather << 8)
 * | (tiled pipelines the key batch was split into << 16). */
#define PBF_DETAIL_RING 1    /* tiled: ring partition (k_part_ring) */
#define PBF_DETAIL_SORT 2    /* tiled: counting-sort partition (k_part) */
#define PBF_DETAIL_ONE_KEY 4 /* pbf_may_contain's one-key launch */
#define PBF_DETAIL_SET 8     /* multi-filter direct probe (k_probe_set: each key hashed once for the set) */
#define PBF_DETAIL_PACKED 16 /* tiled build: region entries packed three positions per 8 bytes */
#define PBF_DETAIL_SHARED 32 /* one-key probe under the handle's lock held shared (a reader stream) */
#define PBF_DETAIL_RESIDENT 64 /* one-key probe answered by the resident reader wave (no launch per key) */

typedef struct pbf_filter pbf_filter_t;

/* Library version (major*10000 + minor*100 + patch). */
int pbf_version(void);

/* Number of visible HIP devices. */
int pbf_device_count(int* count);

/* BloomFilter(nb_bytes, nb_hash_functions) — bloom_filter.py:26-31.  The bitmap is
 * 8*nb_bytes bits, all zero.  nb_bytes == 0 → PBF_ERR_ZERO_SIZE (the Python layer keeps such a
 * filter host-side and raises ZeroDivisionError on add/may_contain, like the reference).
 * Any nb_hash_functions is accepted, as in the reference; serialising one above 255 fails in
 * the Python layer exactly where the reference's struct.pack("B", k) does (bloom_filter.py:80). */
int pbf_create(int device, uint64_t nb_bytes, uint32_t nb_hash_functions, pbf_filter_t** out);
int pbf_destroy(pbf_filter_t* f);

/* Reset to the all-zero filter (bits = 0, bloom_filter.py:31). */
int pbf_clear(pbf_filter_t* f);

/* BloomFilter.add for a batch of keys (bloom_filter.py:60-65): ORs k bits per key. */
int pbf_add_fixed(pbf_filter_t* f, const uint8_t* keys, uint32_t key_len, uint64_t n, int keys_on_device);
int pbf_add(pbf_filter_t* f, const uint8_t* keys, const uint64_t* offsets, uint64_t n, int keys_on_device);
/* The same call under SURVEY.md §8b's name. */
int pbf_build(pbf_filter_t* f, const uint8_t* keys, const uint64_t* offsets, uint64_t n, int keys_on_device);

/* BloomFilter.may_contain for a batch (bloom_filter.py:67-74).  hitmask receives ceil(n/8)
 * bytes, LSB-first: bit (i & 7) of hitmask[i >> 3] = may_contain(key i).  The hitmask pointer
 * is host or device memory as keys_on_device says. */
int pbf_probe_fixed(pbf_filter_t* f, const uint8_t* keys, uint32_t key_len, uint64_t n, uint8_t* hitmask,
                    int keys_on_device);
int pbf_probe(pbf_filter_t* f, const uint8_t* keys, const uint64_t* offsets, uint64_t n, uint8_t* hitmask,
              int keys_on_device);

/* LsmStorage.get's filter checks for a batch of keys against several SSTable filters
 * (src/lsm_storage.py:164-169 L0 newest-first, :173-175 per level): hitmasks[i] receives
 * may_contain over the batch for filters[i], ceil(n/8) bytes LSB-first, host or device memory as
 * keys_on_device says (hitmasks itself is a host array of nfilters pointers).  Filters must be
 * distinct; with keys_on_device = 1 they must share one device, while a HOST batch over filters
 * on several devices fans out to one host thread per device (pbf_probe_multi_placed, grouped by
 * device).  When they share (nb_bytes, k) and are large (the tiled
 * probe) the keys are hashed and partitioned once for up to 8 filters and only the tile test
 * and gather run per filter.  Otherwise -- SSTable filters of mixed sizes, the usual LSM case
 * (each sized from its own key count, sstable.py:274) -- the filters whose own probe is direct
 * are probed by one kernel per k and 64 filters that hashes every key ONCE and tests every
 * filter from those hashes (MurmurHash3 does not depend on m); large filters of distinct sizes
 * each run their own pipeline on their own stream.  With keys_on_device = 1 the call is
 * asynchronous on filters[0]'s stream (pbf_sync(filters[0])); every other filter's stream is
 * ordered before and after it. */
int pbf_probe_multi_fixed(pbf_filter_t* const* filters, uint32_t nfilters, const uint8_t* keys, uint32_t key_len,
                          uint64_t n, uint8_t* const* hitmasks, int keys_on_device);
int pbf_probe_multi(pbf_filter_t* const* filters, uint32_t nfilters, const uint8_t* keys, const uint64_t* offsets,
                    uint64_t n, uint8_t* const* hitmasks, int keys_on_device);

/* The host-batch multi-probe over a filter set placed on several devices from one process (an
 * LSM's SSTable filters spread one per GPU; LsmStorage.get, src/lsm_storage.py:164-179):
 * group_of[i] names filter i's placement group (filters of one group must share a device; a
 * device may hold several groups).  Each group runs pbf_probe_multi on its own host thread,
 * staging the batch to its device itself (a replicated H2D); hitmasks[i] receives filter i's
 * mask, so the masks come back in the caller's (get) order.  offsets == NULL: fixed key_len.
 * Synchronous. */
int pbf_probe_multi_placed(pbf_filter_t* const* filters, uint32_t nfilters, const uint32_t* group_of,
                           const uint8_t* keys, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                           uint8_t* const* hitmasks);

/* The placement step of pbf_probe_multi_placed (and of a host-batch pbf_probe_multi over
 * filters on several devices, grouped by device), as a pure function that runs without a GPU:
 * slot_of[i] = filter i's group in first-appearance order of group_of (the order the groups'
 * host threads start), *ngroups = the number of groups.  PBF_ERR_INVALID when two filters of
 * one group name different devices (device_of[i] = filter i's device). */
int pbf_plan_groups(const uint32_t* group_of, const int32_t* device_of, uint32_t n, uint32_t* slot_of,
                    uint32_t* ngroups);

/* BloomFilter.may_contain(key) for ONE key (bloom_filter.py:67-74), the per-key call of
 * LsmStorage.get (lsm_storage.py:165,175): key is host memory (UTF-8 bytes, len may be 0),
 * *out = 1 or 0.  Synchronous; the key goes to the kernel through mapped pinned memory and the
 * hit byte comes back the same way (one launch, no copies, no allocation after the first call
 * on a thread). */
int pbf_may_contain(pbf_filter_t* f, const uint8_t* key, uint64_t len, int* out);

/* LsmStorage.get's bloom checks for ONE key over a set of SSTable filters of any sizes
 * (lsm_storage.py:164-179: every L0 filter, then each level filter whose key range holds the
 * key — the range check stays with the caller): out_bits[i >> 3] bit (i & 7) =
 * filters[i].may_contain(key), ceil(nfilters/8) bytes LSB-first.  One launch per k and 64
 * filters (the key hashed once, one lane per filter), the key in and the answer out through
 * mapped pinned memory; synchronous.  All filters on one device (a filter may repeat). */
int pbf_may_contain_set(pbf_filter_t* const* filters, uint32_t nfilters, const uint8_t* key, uint64_t len,
                        uint8_t* out_bits);

/* pbf_may_contain / pbf_may_contain_set on built, idle filters (nothing queued on their streams)
 * are answered by a resident reader: ONE wave per device stays on a stream of its own while keys
 * arrive, polling per-thread request slots in mapped pinned memory (no launch per key); it leaves
 * after PBF_RESIDENT_IDLE_US (default 2000) without a key and is relaunched by the next one.
 * PBF_RESIDENT_READER=0 (read once) launches per key instead.  Keys over 1024 bytes, k > 32 and
 * threads beyond 64 per device take the per-key launch.  *launches = the waves started so far on
 * `device` (0 before the first resident answer). */
int pbf_resident_launches(int device, uint32_t* launches);
/* Requests the device's resident reader has answered so far, and the wave's time on them: from
 * seeing a request in its poll to writing the answer (device wall clock), summed.  The rest of a
 * call's time is the host's and the bus's (posting, the poll's round trip, the answer's write). */
int pbf_resident_stats(int device, uint64_t* requests, uint64_t* device_ns);
/* Turns the resident reader on (1) or off (0) for later calls of the process (overrides
 * PBF_RESIDENT_READER; a wave already resident leaves after its idle time). */
int pbf_resident_enable(int on);

/* mmh3.hash(key, seed) (bloom_filter.py:46: MurmurHash3_x86_32, signed int32) of one host key
 * of at most 4096 bytes, computed on `device` (one launch). */
int pbf_murmur3_x86_32(int device, const uint8_t* key, uint64_t len, uint32_t seed, int32_t* out);

/* The k bit indices of each key, BloomFilter._hash (bloom_filter.py:38-49): out[i*k + s] =
 * mmh3.hash(key_i, s) % bits_size (Python floor-mod).  out is host or device memory as
 * keys_on_device says (n*k uint64).  Used for index-math parity at any m. */
int pbf_hash_indices_fixed(pbf_filter_t* f, const uint8_t* keys, uint32_t key_len, uint64_t n, uint64_t* out,
                           int keys_on_device);
int pbf_hash_indices(pbf_filter_t* f, const uint8_t* keys, const uint64_t* offsets, uint64_t n, uint64_t* out,
                     int keys_on_device);

/* to_bytes() minus the trailing k byte (bloom_filter.py:76-81): copies the nb_bytes-byte
 * little-endian bitmap into host memory `out` (nb_bytes must equal the filter's). */
int pbf_get_bitmap(pbf_filter_t* f, uint8_t* out, uint64_t nb_bytes);

/* from_bytes() (bloom_filter.py:83-90): loads an nb_bytes-byte bitmap from host memory. */
int pbf_set_bitmap(pbf_filter_t* f, const uint8_t* in, uint64_t nb_bytes);

/* from_bytes() / to_bytes() against DEVICE memory on the filter's device (nb_bytes bytes, the
 * little-endian bitmap without the k byte), e.g. a tensor an RCCL all-gather filled with other
 * ranks' filters.  Asynchronous on the filter's stream (order a producer on another stream with
 * pbf_wait_stream, a consumer with pbf_signal_stream or pbf_sync). */
int pbf_set_bitmap_device(pbf_filter_t* f, const void* in_dev, uint64_t nb_bytes);
int pbf_get_bitmap_device(pbf_filter_t* f, void* out_dev, uint64_t nb_bytes);

/* A replica of a built filter on dst_device (the same device or another): *out = a new handle
 * with src's nb_bytes, k and bitmap -- what from_bytes(src.to_bytes()) onto that device gives
 * (src/sstable.py:99-100), without the host round trip.  The bitmap goes device to device
 * (hipMemcpyPeerAsync over xGMI, peer access enabled once per device pair where the platform
 * allows it; the runtime stages the copy otherwise), or with flags = PBF_COPY_BOUNCE through
 * pinned host memory.  Synchronous: the replica is complete on return and src may change after.
 * An LSM builds each SSTable's filter once (src/sstable.py:274) and every get probes all of them
 * (src/lsm_storage.py:164-179): the key-partitioned multi-GPU layout holds every filter on every
 * GPU by replication, not by rebuilding. */
#define PBF_COPY_BOUNCE 1
int pbf_copy_filter(pbf_filter_t* src, int dst_device, int flags, pbf_filter_t** out);

/* Population count of the bitmap (device reduction; host-visible result). */
int pbf_popcount(pbf_filter_t* f, uint64_t* out);

/* Wait for all work queued on the filter's stream. */
int pbf_sync(pbf_filter_t* f);

/* The device index map of a filter of nb_bytes (host-side, no GPU): how `hash % bits_size`
 * (Python floor-mod of the signed hash, bloom_filter.py:47) is computed for m = 8*nb_bytes.
 * mode 0: m a power of two <= 2^32, u32(h) & (m-1); 1: m < 2^30, a mod m = a - (mulhi(a, magic)
 * >> shift) * m for a = h >= 0 ? h : ~h; 2: m >= 2^31, h or h + m; 3: 2^30 < m < 2^31, one
 * conditional subtract.  Exposed so the reciprocal can be checked exhaustively on the host. */
int pbf_index_params(uint64_t nb_bytes, uint32_t* mode, uint64_t* magic, uint32_t* shift);

/* Stream ordering for device-pointer calls (keys_on_device = 1) without a device-wide sync:
 * pbf_wait_stream makes the filter's stream wait for everything queued on `stream` so far
 * (e.g. the torch stream that produced a key batch; NULL = the null stream) -- the next
 * add / probe of f runs after that producer; pbf_signal_stream makes `stream` wait for
 * everything queued on the filter's stream so far (a consumer of a device hit mask or bitmap).
 * Both only enqueue an event record + wait; neither blocks the host. */
int pbf_wait_stream(pbf_filter_t* f, void* stream);
int pbf_signal_stream(pbf_filter_t* f, void* stream);

/* The filter's hipStream_t (for events / interop) and its device bitmap (uint32 words). */
void* pbf_stream(pbf_filter_t* f);
void* pbf_device_bitmap(pbf_filter_t* f);

/* Select the build strategy (PBF_BUILD_*); the strategy actually used by the last add is
 * returned by pbf_last_build_mode. */
int pbf_set_build_mode(pbf_filter_t* f, int mode);
int pbf_last_build_mode(pbf_filter_t* f);

/* Select the probe strategy (PBF_PROBE_*); the one used by the last probe is returned by
 * pbf_last_probe_mode, and how it ran by pbf_last_probe_detail (PBF_DETAIL_*). */
int pbf_set_probe_mode(pbf_filter_t* f, int mode);
int pbf_last_probe_mode(pbf_filter_t* f);
uint32_t pbf_last_probe_detail(pbf_filter_t* f);
/* How the last tiled build ran: PBF_DETAIL_RING or _SORT [| _PACKED] | (keys per sub-chunk / 256) << 12. */
uint32_t pbf_last_build_detail(pbf_filter_t* f);

/* What the host planner picks for one tiled build or probe pipeline: the kernel / geometry variant
 * chosen from (nb_bytes, k, key layout, n, filters per fused probe).  Every field is a uint64_t
 * (flags are 0 / 1), so the struct has no padding.  When `tiled` is 0 only probe, nf, tiled_ok, tiled,
 * tb, B and cspace are meaningful. */
typedef struct pbf_tiled_plan {
    uint64_t probe, nf;           /* as asked (nf = 1 for a build) */
    uint64_t tiled_ok;            /* the filter's tile geometry admits the tiled paths at all */
    uint64_t tiled;               /* ... and so do k, the partition's LDS and (probes) the tile size */
    uint64_t tb, B, cspace;       /* log2 positions per tile, tiles, m > 2^32 */
    uint64_t key_mode;            /* 0 fixed 16-byte aligned, 1 fixed length, 2 variable length */
    uint64_t n;                   /* keys of the pipeline described (the call's last one) */
    uint64_t pipelines, keys_per_pipeline;
    uint64_t ring;                /* ring partition: LDS ring entries per tile (0 = counting sort) */
    uint64_t G, cap, kps, nsub, kpw, nq, scap, spill_cap;  /* PartGeom */
    uint64_t rounds;              /* multi-filter ring probe: workgroup rounds planned (1..4) */
    uint64_t pk3;                 /* packed build entries */
    uint64_t part_kmax;           /* register bucket (or exact k) of the partition kernel */
    uint64_t exact_k;             /* the partition kernel has k fixed at compile time */
    uint64_t pow2;                /* ring partition's POW2 branch */
    uint64_t gsplit, gtq, gather_threads;
    uint64_t gather_nf;           /* k_gather_ring<1> or <8> */
    uint64_t lds_part;            /* bytes; the ring partition declares the CU's 160 KiB statically */
    uint64_t lds_gather, lds_tile;
    uint64_t tab, tabw, wsh;      /* tile test table mode, TAB 1 chunk words, region shift */
    uint64_t use_hw;              /* the gather ANDs key words (then hw_is_mask or k_hw_to_hitmask) */
    uint64_t hw_is_mask;          /* pbf_plan_tiled: assuming a 4-byte aligned mask address */
} pbf_tiled_plan;

/* The plan for n keys of the given layout (key_len 0 = variable length; keys_16B_aligned matters
 * for key_len 16 only) against a filter of (nb_bytes, k), nf filters probed together, spare_cu =
 * a resident one-key reader holds a CU.  Host arithmetic only (no GPU), by the functions the
 * launches use.  The environment overrides (PBF_PART, PBF_PART_G, PBF_GATHER_SPLIT, PBF_PK3) are
 * read once per process. */
int pbf_plan_tiled(uint64_t nb_bytes, uint32_t k, uint32_t key_len, int keys_16B_aligned, uint64_t n, int probe,
                   uint32_t nf, int spare_cu, pbf_tiled_plan* out);
/* The plan the filter's last batch build (probe = 0) or batch probe (probe = 1) launched, for the
 * call's last pipeline, with the call's pipeline count and the real hw_is_mask.  PBF_ERR_INVALID
 * when there was none or that batch call was not tiled.  One-key probes (pbf_may_contain,
 * pbf_may_contain_set) run under the handle's lock held shared and leave the report as it is. */
int pbf_last_tiled_plan(pbf_filter_t* f, int probe, pbf_tiled_plan* out);

/* Release the device's pooled working memory (waits for its last users); the next call
 * re-allocates what it needs.  pbf_scratch_bytes reports what the pool holds now. */
int pbf_trim(int device);
int pbf_scratch_bytes(int device, uint64_t* out);

/* SSTableBuilder's data section (src/sstable.py:224-268; DataBlock.to_bytes blocks.py:33-37;
 * Record.to_bytes record.py:66-72, key_size = the key's UTF-8 CHARACTER count as the reference's
 * len(str), record.py:24).  Record i = (keys[key_offsets[i], key_offsets[i+1]),
 * values[value_offsets[i], value_offsets[i+1])).  The caller plans the blocks with the
 * DataBlockBuilder rule (blocks.py:78-95; pebbledb_amd/sstable_data.py plan_blocks): block b
 * holds records [block_first[b], block_first[b+1]) (block_first has nblocks+1 entries, 0 .. n)
 * and is written at byte block_out[b] of out (block_out[nblocks] = section size); a block's
 * records may total at most 65536 bytes.  One workgroup per block assembles it in LDS.
 * on_device = 0: all pointers are host memory (checked, staged, section copied back);
 * on_device = 1: every pointer is device memory and nothing is checked on the host (n is not
 * used): the plan must be monotonic and in range; a block whose records exceed 65536 bytes is
 * left unwritten and the call returns PBF_ERR_INVALID ("N block(s) exceed ..."), the other
 * blocks are written.  keys, values and out may have any byte alignment (a slice of a larger
 * allocation).  Offsets index from the keys / values pointers as passed: byte j of key i is
 * keys[key_offsets[i] + j]; the first offset a block uses need not be 0 (key_offsets + r0,
 * value_offsets + r0 with block_first relative to r0 encode a window of a run), and block_out
 * need not be contiguous.  The kernel reads a span in whole 16-byte chunks aligned by ADDRESS:
 * for a non-empty span [p, q) it may read any byte of [p & ~15, (q + 15) & ~15) — up to 15
 * bytes before the first and after the last byte, never beyond the 16-byte line (hence the
 * page) that holds a byte of the span; an empty span is not read.  It writes exactly the
 * bytes [out + block_out[b], + the block's encoded size) of each block.  The kernel runs on the
 * NULL stream and the call returns after it has finished.  Synchronous. */
int pbf_encode_data_blocks(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint8_t* values,
                           const uint64_t* value_offsets, uint64_t n, const uint64_t* block_first,
                           const uint64_t* block_out, uint64_t nblocks, uint8_t* out, int on_device);

/* SSTableBuilder.add x n + build (src/sstable.py:224-288) in one call, for the flush of a
 * packed run of records (host memory; offsets start at 0): one H2D of the keys, values and
 * block plan (as for pbf_encode_data_blocks), the data blocks encoded on the device, the filter
 * f (sized by the caller with the reference's build_from_keys_and_fp_rate expression, fp 0.001)
 * built from the SAME device copy of the keys, and D2H of the data section into data_out
 * (block_out[nblocks] bytes) and of the bitmap into bitmap_out (f's nb_bytes, may be NULL) —
 * the caller points both at their slices of the SSTable file buffer.  Synchronous. */
int pbf_build_sstable(pbf_filter_t* f, const uint8_t* keys, const uint64_t* key_offsets, const uint8_t* values,
                      const uint64_t* value_offsets, uint64_t n, const uint64_t* block_first, const uint64_t* block_out,
                      uint64_t nblocks, uint8_t* data_out, uint8_t* bitmap_out);

/* Compaction's output SSTables (LsmStorage._compact, src/lsm_storage.py:233-251: a new
 * SSTableBuilder once current_buffer_position >= max_sstable_size) from ONE upload of the
 * compacted record run (host memory, offsets start at 0; n records).  The caller plans the split
 * on the host (pebbledb_amd/sstable_data.plan_compaction): blocks as for pbf_build_sstable but over
 * the whole run, block_out laid end to end over the outputs' data sections, output t = blocks
 * [table_blocks[t], table_blocks[t+1]) (table_blocks has ntables+1 entries, 0 .. nblocks; the
 * plan may end before record n: the reference does not write records left in its last builder's
 * first open block).  filters[t] is output t's filter (sized by the caller from its key count
 * with build_from_keys_and_fp_rate's expression, fp 0.001, sstable.py:274), built from its slice
 * of the SAME device copy of the keys on its own stream; data_outs[t] / bitmap_outs[t]
 * (bitmap_outs or an entry may be NULL) receive the output's data section and bitmap, the
 * caller's slices of each SSTable file buffer.  Synchronous. */
int pbf_build_sstables(pbf_filter_t* const* filters, uint32_t ntables, const uint8_t* keys, const uint64_t* key_offsets,
                       const uint8_t* values, const uint64_t* value_offsets, uint64_t n, const uint64_t* block_first,
                       const uint64_t* block_out, uint64_t nblocks, const uint64_t* table_blocks,
                       uint8_t* const* data_outs, uint8_t* const* bitmap_outs);

/* DataBlockBuilder's greedy blocks (src/blocks.py:78-95, sstable.py:224-244) over n records
 * whose key / value bytes are given by their offsets: block_first[0..nblocks] record indices,
 * block_out[0..nblocks] byte offsets of the encoded blocks (both sized n+1 by the caller);
 * *nblocks receives the count.  Host-side planning for pbf_build_sstable. */
int pbf_plan_blocks(const uint64_t* key_offsets, const uint64_t* value_offsets, uint64_t n, uint64_t block_size,
                    uint64_t* block_first, uint64_t* block_out, uint64_t* nblocks);

/* Compaction's output split (LsmStorage._compact, src/lsm_storage.py:233-251) over n records,
 * host-side: the greedy blocks of pbf_plan_blocks over the whole run, a new table whenever the
 * builder's position (advanced per finished block, src/sstable.py:246-266) reaches
 * max_sstable_size (the table's last block then holds only the record that finished the previous
 * one), the last builder kept only if its position is past 0.  Outputs for pbf_build_sstables:
 * block_first / block_out (n+1 entries each; block_out laid end to end over the tables' data
 * sections), table_blocks (n+1 entries; table t = blocks [table_blocks[t], table_blocks[t+1])),
 * the counts, and the records covered (*written <= n).  max_sstable_size 0 is refused
 * (PBF_ERR_INVALID). */
int pbf_plan_compaction(const uint64_t* key_offsets, const uint64_t* value_offsets, uint64_t n, uint64_t block_size,
                        uint64_t max_sstable_size, uint64_t* block_first, uint64_t* block_out, uint64_t* table_blocks,
                        uint64_t* nblocks, uint64_t* ntables, uint64_t* written);

/* The level key-range pre-check of LsmStorage.get (src/lsm_storage.py:171-175) for a batch:
 * out[t * ceil(n/8) + i/8] bit (i & 7) = (first_t <= key_i <= last_t), Python str order =
 * bytewise lexicographic order of the UTF-8 keys.  Bounds are 2*ntables byte strings
 * (first_0, last_0, first_1, last_1, ...) of at most 65536 bytes each, bound j being
 * bound_offsets[j+1] - bound_offsets[j] bytes.  bound_offsets[0] may be non-zero, as offsets[0]
 * may (a window): with host pointers `bounds` and `keys` are the buffers the offsets index
 * (bound j = bounds[bound_offsets[j], bound_offsets[j+1])), with device pointers they are the
 * windows' first bytes (bound j = bounds[bound_offsets[j] - bound_offsets[0], bound_offsets[j+1] -
 * bound_offsets[0])).  Keys as in pbf_probe (offsets != NULL) or fixed key_len (offsets ==
 * NULL).  Every byte of the T rows is written (the pad bits of a row's last byte as zeros) and
 * nothing outside them.  The mask layout is the hit-mask layout, so it ANDs directly with
 * the table's filter hit mask.  on_device = 0: host pointers, synchronous; on_device = 1:
 * device pointers (bound_offsets is read back first), asynchronous on `stream`. */
int pbf_key_range_mask(int device, void* stream, const uint8_t* keys, const uint64_t* offsets, uint32_t key_len,
                       uint64_t n, const uint8_t* bounds, const uint64_t* bound_offsets, uint32_t ntables, uint8_t* out,
                       int on_device);

/* ---- Resident SSTables: the point lookup of SSTable.get (src/sstable.py:150-187) and of
 * LsmStorage.get's walk (src/lsm_storage.py:164-179) for a batch of keys, over tables whose data
 * sections stay in device memory until closed (no cache, no eviction). */
typedef struct pbf_sstable pbf_sstable_t;

/* Copies a data section (every DataBlock back to back, blocks.py:33-37; data_len bytes, host
 * memory, or device memory on `device` with data_on_device = 1) to the device once and validates
 * it there.  Block b is data[block_off[b], block_off[b+1]) -- the meta blocks' offsets plus
 * meta_block_offset, nblocks+1 entries in HOST memory, from 0 to data_len.  Per block: count >= 1
 * and 2*count+2 <= block bytes; offsets[0] == 0, strictly ascending, inside the record area; per
 * record 8 + key_size + value_size == its extent with both sizes >= 0; keys strictly ascending in
 * unsigned bytewise order, inside and across blocks.  Any violation: PBF_ERR_INVALID and a
 * message that names the rule; nothing stays allocated.  A table that passed cannot make a lookup
 * read outside its data section.  (The reference writes key_size in characters, record.py:25, and
 * reads it as bytes, :77-79: it cannot read back a table that stores a non-ASCII key; such a
 * table breaks the size rule and is refused.)  Synchronous. */
int pbf_sst_open(int device, const uint8_t* data, uint64_t data_len, const uint32_t* block_off, uint32_t nblocks,
                 int data_on_device, pbf_sstable_t** out);
/* Waits for every lookup that holds the table (lookups hold its lock shared, close takes it
 * exclusively; asynchronous lookups are waited for through their streams' events), then frees it.
 * A handle that was closed is refused (PBF_ERR_INVALID) by every later call. */
int pbf_sst_close(pbf_sstable_t* t);
int pbf_sst_info(pbf_sstable_t* t, uint32_t* nblocks, uint64_t* nrecords, uint64_t* data_len);
/* The validated block index, 4 words per block: offset of the first record, of the last record,
 * of the u16 array, and the record count (offsets into the data section). */
int pbf_sst_block_index(pbf_sstable_t* t, uint32_t* out, uint32_t nblocks);

/* The get walk for n keys (layouts as pbf_probe: offsets != NULL, or fixed key_len) over
 * `ntables` tables in row order: key i reads the tables whose mask has bit i set (masks[t]:
 * ceil(n/8) bytes LSB-first, the hit-mask layout; masks == NULL or masks[t] == NULL: every key)
 * and stops at the first that holds it.  table_out[i] = that row or -1; val_off_out[i] = the
 * value's offset in that table's data section; val_len_out[i] = its length, -1 if absent (0 is a
 * stored empty value, which the reference returns as b"").  ntables = 1 with no mask is
 * SSTable.get.  `tables` and `masks` are host arrays; the tables share one device
 * (PBF_ERR_INVALID otherwise).  on_device = 0: keys, masks and outputs are host memory,
 * synchronous; on_device = 1: device pointers, asynchronous on `stream`. */
int pbf_sst_get(pbf_sstable_t* const* tables, uint32_t ntables, const uint8_t* keys, const uint64_t* offsets,
                uint32_t key_len, uint64_t n, const uint8_t* const* masks, int on_device, void* stream,
                int32_t* table_out, uint64_t* val_off_out, int32_t* val_len_out);

/* Packs the values pbf_sst_get found: out_offsets[n+1] = the exclusive scan of max(val_len, 0)
 * closed by the total, out_bytes[out_offsets[i], out_offsets[i+1]) = value i.  out_bytes == NULL:
 * offsets only; otherwise it holds out_cap bytes (PBF_ERR_INVALID when the total is larger; an
 * entry that names no table or lies outside its data section is refused the same way).
 * on_device as for pbf_sst_get; with device pointers the work is ordered on `stream`, and the call
 * returns once the total has been read back. */
int pbf_sst_gather(pbf_sstable_t* const* tables, uint32_t ntables, const int32_t* table_idx, const uint64_t* val_off,
                   const int32_t* val_len, uint64_t n, uint8_t* out_bytes, uint64_t out_cap, uint64_t* out_offsets,
                   int on_device, void* stream);

/* ---- Compaction's record run over resident tables: MergingIterator over SSTableIterators
 * (src/iterators.py:110-190, force_compaction_l0 src/lsm_storage.py:253-260) or
 * ConcatenatingIterator (iterators.py:193-207, force_compaction_l1_or_more_level), in the layout
 * pbf_build_sstables reads. */
#define PBF_MERGE_DEDUP  0   /* MergingIterator over SSTableIterators */
#define PBF_MERGE_CONCAT 1   /* ConcatenatingIterator */

/* tables[0] is the first iterator.  PBF_MERGE_DEDUP: every distinct key in ascending unsigned
 * bytewise order, each with the record of the lowest table index that stores it (the heap key is
 * (key, iterator index) and _filter_duplicate_keys keeps the first record of a key; an empty
 * value is a value like any other).  PBF_MERGE_CONCAT: every record, table after table in list
 * order, whatever the tables' key ranges.  Record j of the run = keys_out[key_offsets_out[j],
 * key_offsets_out[j+1]), values_out[value_offsets_out[j], value_offsets_out[j+1]); both offsets
 * arrays receive *n_out + 1 entries, from 0 to the total.  keys_cap / values_cap are the bytes
 * and offsets_cap the entries (in each offsets array) the caller provides.  n_out, key_bytes_out
 * and value_bytes_out are host pointers and are set whenever the run was counted, also when it
 * does not fit.
 * on_device = 0: outputs are host memory, synchronous.  on_device = 1: device pointers; the work
 * is ordered on `stream` and the call returns once the three totals have been read back (the
 * tables must not be closed from another thread before the stream is done: pbf_sst_close waits
 * for it, as for lookups).
 * PBF_ERR_INVALID, nothing written to the outputs: ntables == 0 or > 64; a null, closed or
 * unknown handle; the same handle listed twice; tables on different devices; a capacity too
 * small (the message states the size needed, and the totals are set, so a caller can retry). */
int pbf_sst_merge(pbf_sstable_t* const* tables, uint32_t ntables, int mode, uint8_t* keys_out, uint64_t keys_cap,
                  uint64_t* key_offsets_out, uint8_t* values_out, uint64_t values_cap, uint64_t* value_offsets_out,
                  uint64_t offsets_cap, uint64_t* n_out, uint64_t* key_bytes_out, uint64_t* value_bytes_out,
                  int on_device, void* stream);

/* ---- Range scan over resident tables: SSTable.scan (src/sstable.py:189, the bounded
 * SSTableIterator of src/iterators.py:58-141) and the MergingIterator LsmStorage.scan yields from
 * (src/lsm_storage.py:187-190), for a batch of ranges in one call.
 * Range q is [lower_q, upper_q], inclusive at both ends, compared as unsigned bytes: bound q =
 * lowers[lower_offsets[q], lower_offsets[q+1]) and likewise uppers (offsets arrays of nranges + 1
 * ascending entries).  lower > upper selects nothing; an empty lower starts at the first record.
 * upper_open (NULL, or nranges bytes): non-zero = no upper bound, uppers' entry is ignored (the
 * reference reads upper == "" that way).  tables[0] is the first iterator; per range the result
 * is PBF_MERGE_DEDUP's run over the records in range.  The ranges are host memory in both calls.
 * At most 64 tables and nranges * ntables <= PBF_SCAN_MAX_SEGMENTS. */
#define PBF_SCAN_MAX_SEGMENTS (1ull << 22)

/* Counts a batch (synchronous, host outputs): *n_in, *key_bytes_in, *value_bytes_in = the records
 * in range over all tables and ranges and their key and value bytes BEFORE de-duplication: they
 * always suffice as pbf_sst_scan's capacities (offsets_cap = *n_in + 1) and are exact when no key
 * repeats across tables.  seg_lo_out / seg_hi_out (each NULL, or nranges * ntables entries, index
 * q * ntables + t): table t's records [lo, hi) lie in range q. */
int pbf_sst_scan_size(pbf_sstable_t* const* tables, uint32_t ntables, const uint8_t* lowers,
                      const uint64_t* lower_offsets, const uint8_t* uppers, const uint64_t* upper_offsets,
                      const uint8_t* upper_open, uint64_t nranges, uint32_t* seg_lo_out, uint32_t* seg_hi_out,
                      uint64_t* n_in, uint64_t* key_bytes_in, uint64_t* value_bytes_in);

/* The run: the ranges' records back to back in pbf_sst_merge's layout (outputs, capacities, totals,
 * on_device and stream as there), range q = records [range_offsets_out[q], range_offsets_out[q+1])
 * of it.  range_offsets_out receives nranges + 1 entries and is host or device memory as the other
 * outputs are.  A record that lies in two ranges appears in both.  nranges == 0: PBF_OK, an empty
 * run (both offsets arrays = {0}, range_offsets_out[0] = 0).
 * PBF_ERR_INVALID, nothing written to the outputs: as pbf_sst_merge, and more ranges x tables than
 * PBF_SCAN_MAX_SEGMENTS. */
int pbf_sst_scan(pbf_sstable_t* const* tables, uint32_t ntables, const uint8_t* lowers, const uint64_t* lower_offsets,
                 const uint8_t* uppers, const uint64_t* upper_offsets, const uint8_t* upper_open, uint64_t nranges,
                 uint8_t* keys_out, uint64_t keys_cap, uint64_t* key_offsets_out, uint8_t* values_out,
                 uint64_t values_cap, uint64_t* value_offsets_out, uint64_t offsets_cap, uint64_t* n_out,
                 uint64_t* key_bytes_out, uint64_t* value_bytes_out, uint64_t* range_offsets_out, int on_device,
                 void* stream);

/* ---- Memtable flush: MemTableIterator's run (src/iterators.py:24-55) of a put log: every distinct
 * key in ascending unsigned bytewise order, each with the value of its LAST put (the memtable's
 * tree replaces the data of a key it holds, src/red_black_tree.py:118-120; an empty value is a
 * value like any other).  The log is the n puts in put order, packed as pbf_build_sstable reads
 * records: put i = keys[key_offsets[i], key_offsets[i+1]), values[value_offsets[i],
 * value_offsets[i+1]).  Inputs and outputs are host memory; synchronous.
 * The output layout, the totals and the capacity rules are pbf_sst_merge's: both offsets arrays
 * receive *n_out + 1 entries; the totals are set whenever the run was counted, also when it does
 * not fit, and then nothing is written and the message states the size needed.
 * put_index_out (NULL, or offsets_cap entries): put_index_out[j] = the log index of the put that
 * record j came from.  n == 0: PBF_OK, an empty run (both offsets arrays = {0}).
 * PBF_ERR_INVALID, checked on the host before any launch: offsets that do not start at 0 or that
 * descend; n >= 2^32 - 1; a key or value of 2^31 bytes or more; a null pointer. */
int pbf_log_sort(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint8_t* values,
                 const uint64_t* value_offsets, uint64_t n,
                 uint8_t* keys_out, uint64_t keys_cap, uint64_t* key_offsets_out,
                 uint8_t* values_out, uint64_t values_cap, uint64_t* value_offsets_out,
                 uint64_t offsets_cap, uint32_t* put_index_out /* NULL, or offsets_cap entries */,
                 uint64_t* n_out, uint64_t* key_bytes_out, uint64_t* value_bytes_out);

/* Device time of the last successful pbf_log_sort on `device`, by stage (HIP events on the call's
 * stream; tools/bench_flush.py): upload of the log, k_mt_entries, k_mt_tile_sort, the merge
 * passes together, k_mt_mark, the scans and offsets (with the read-back of the totals between
 * them), k_mt_copy, download of the run.  ms_out receives PBF_LOG_SORT_STAGES entries;
 * *merge_passes_out (or NULL) the k_mt_merge_rank launches. */
#define PBF_LOG_SORT_STAGES 8
int pbf_log_sort_stage_ms(int device, float* ms_out, uint32_t* merge_passes_out);

/* ---- Resident write path: compaction and flush that plan on the device and open their outputs
 * there.  Resident tables or a put log in, resident tables out; file bytes on request
 * (pbf_sst_read_data).  Nothing of the record run touches host memory.
 *
 * The device planner (csrc/sstable_plan_kernels.hpp) over a run's two offsets arrays in device
 * memory (n + 1 entries each, from 0, n > 0): max_sstable_size == 0 plans pbf_plan_blocks' blocks
 * (one table, every record written), otherwise pbf_plan_compaction's split.  block_first_dev /
 * block_out_dev receive *nblocks + 1 entries and table_blocks_dev *ntables + 1, entry for entry what
 * the host planners return; each array holds cap_entries entries (n + 1 always suffices; a plan
 * that does not fit is refused) and nothing past the entries named is written.  A record larger
 * than block_size: PBF_ERR_INVALID "a record is larger than block_size", nothing written.  The
 * kernels run on `stream` (NULL = the null stream); the call returns when the plan is complete. */
int pbf_plan_device(int device, void* stream, const uint64_t* key_offsets_dev, const uint64_t* value_offsets_dev,
                    uint64_t n, uint64_t block_size, uint64_t max_sstable_size, uint64_t* block_first_dev,
                    uint64_t* block_out_dev, uint64_t* table_blocks_dev, uint64_t cap_entries, uint64_t* nblocks,
                    uint64_t* ntables, uint64_t* written);

/* A job is two-phase because each output's filter is sized from its own record count (by the
 * caller, with build_from_keys_and_fp_rate's expression): `begin` produces the run into
 * job-owned device memory and plans it, pbf_job_table_info reports what the caller needs per
 * output, pbf_job_finish builds the outputs.  A refusal in any phase leaves no table registered
 * and no memory held; pbf_job_finish frees the job whatever it returns, pbf_job_abort frees one
 * that will not be finished.  A handle that was finished or aborted is refused.
 *
 * pbf_compact_begin: pbf_sst_merge's run (mode PBF_MERGE_DEDUP or PBF_MERGE_CONCAT; the same
 * refusals) planned by pbf_plan_compaction's rule.  The tables are held shared for this call only:
 * the run is a copy, they may be closed before pbf_job_finish.  *ntables_out may be 0 (the run lies
 * wholly in its first open block); *written = records covered by the outputs.
 * pbf_flush_begin: pbf_log_sort's run of a put log in host memory (the same checks), left on the
 * device and planned as one table by pbf_plan_blocks' rule; n == 0 is refused. */
typedef struct pbf_job pbf_job_t;
int pbf_compact_begin(pbf_sstable_t* const* tables, uint32_t ntables, int mode, uint64_t block_size,
                      uint64_t max_sstable_size, pbf_job_t** job, uint64_t* ntables_out, uint64_t* written);
int pbf_flush_begin(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint8_t* values,
                    const uint64_t* value_offsets, uint64_t n, uint64_t block_size, pbf_job_t** job);
/* Output t: its records, data blocks, data section bytes, and the bytes of its blocks' first and
 * last keys together (its meta blocks take 8 * nblocks + bound_key_bytes bytes).  Any may be NULL. */
int pbf_job_table_info(pbf_job_t* job, uint32_t t, uint64_t* nrecords, uint64_t* nblocks, uint64_t* data_len,
                       uint64_t* bound_key_bytes);
/* Builds every output: its data blocks are encoded straight into the allocation the new table
 * owns (followed by the 16 zero bytes pbf_sst_open writes; no copy of the section), filters[t] is
 * built from the output's slice of the run's keys on the filter's own stream, the blocks' first and
 * last keys are gathered, and the validator of pbf_sst_open builds the block index from the
 * section, so a table made here keeps that call's promise.  Outputs, all host memory, laid output
 * after output: block_off_out, (nblocks_t + 1) entries per output, block b of output t at
 * [block_off[b], block_off[b+1]) of its section; bounds_offsets_out, 2 * (all blocks) + 1 entries
 * from 0, bounds_out[offs[2 b], offs[2 b + 1]) = block b's first key and [offs[2 b + 1], offs[2 b +
 * 2]) its last (keys are ASCII on this path: bytes are characters); tables_out[t] = the new handle.
 * An output that breaks a rule of pbf_sst_open is refused, with one exception: under
 * PBF_MERGE_CONCAT over tables that are out of key order the outputs' keys do not ascend, as in
 * the files the reference writes; such an output is registered (its framing holds, so no lookup
 * leaves its section) but only its records in stored order are meaningful.
 * filters: one per output, on the job's device, distinct.  A job without outputs finishes with
 * nothing to do (every pointer may be NULL).  Synchronous. */
int pbf_job_finish(pbf_job_t* job, pbf_filter_t* const* filters, uint32_t* block_off_out, uint8_t* bounds_out,
                   uint64_t* bounds_offsets_out, pbf_sstable_t** tables_out);
int pbf_job_abort(pbf_job_t* job);
/* Device time of the last finished job on `device` by stage (HIP events): the run, the plan, the
 * encode with the bounds gather, the wait for the filters, the validation.  PBF_JOB_STAGES entries. */
#define PBF_JOB_STAGES 5
int pbf_job_stage_ms(int device, float* ms_out);

/* Copies a resident table's data section (len = its data_len) to host memory, for the file. */
int pbf_sst_read_data(pbf_sstable_t* t, uint8_t* out_host, uint64_t len);

/* ---- Device memtable: MemTable (src/memtable.py) as one resident sorted run, searched and windowed
 * on the device, in front of the tables in LsmStorage.get (src/lsm_storage.py:153-162: the active
 * memtable, then the immutable ones, deque index 0 first) and LsmStorage.scan (:184-190).
 * A memtable owns ONE run in device memory: its records strictly ascending and de-duplicated in
 * pbf_sst_merge's output layout, plus the 8-byte prefix of every key (csrc/memtable_read_kernels.hpp).
 * Readers hold the handle's lock shared, pbf_mt_apply and pbf_mt_destroy exclusively; asynchronous
 * readers leave a per-stream event both wait for before a run is freed.  At most
 * PBF_MT_MAX_PER_CALL memtables per call, memtables + tables <= 64, all on one device; a handle
 * listed twice, a null or destroyed handle: PBF_ERR_INVALID. */
#define PBF_MT_MAX_PER_CALL 16
typedef struct pbf_memtable pbf_memtable_t;

/* MemTable() (memtable.py:17-27): an empty memtable on `device`.  pbf_mt_destroy waits for every
 * reader, then frees the run; a destroyed handle is refused by every later call. */
int pbf_mt_create(int device, pbf_memtable_t** out);
int pbf_mt_destroy(pbf_memtable_t* mt);

/* MemTable.put x n (memtable.py:64-72; the tree replaces the data of a key it holds,
 * red_black_tree.py:118-120): a put log in put order, in host memory, packed and checked as
 * pbf_log_sort's input.  The log is sorted on the device by pbf_log_sort's chain and merged with the
 * current run, the new batch winning every shared key, into a new run; the old one is freed once
 * its readers are done.  n == 0 is a no-op; the first batch of an empty memtable is not merged.
 * Synchronous. */
int pbf_mt_apply(pbf_memtable_t* mt, const uint8_t* keys, const uint64_t* key_offsets, const uint8_t* values,
                 const uint64_t* value_offsets, uint64_t n);

/* The run's records and its key and value bytes (any pointer may be NULL). */
int pbf_mt_info(pbf_memtable_t* mt, uint64_t* nrecords, uint64_t* key_bytes, uint64_t* value_bytes);

/* MemTableIterator's whole run (src/iterators.py:24-55) to host memory, pbf_log_sort's run of every
 * put so far: both offsets arrays receive nrecords + 1 entries.  Capacities as in pbf_sst_merge: too
 * small is PBF_ERR_INVALID with the size needed in the message, nothing written. */
int pbf_mt_read(pbf_memtable_t* mt, uint8_t* keys_out, uint64_t keys_cap, uint64_t* key_offsets_out, uint8_t* values_out,
                uint64_t values_cap, uint64_t* value_offsets_out, uint64_t offsets_cap);

/* MemTable.get (memtable.py:74-79) for n keys (layouts as pbf_probe) over the memtables in list
 * order, as LsmStorage.get reads them (lsm_storage.py:155-162): src_out[i] = the index of the
 * first memtable that holds key i, or -1; val_off_out[i] = the value's offset in that memtable's
 * value bytes; val_len_out[i] = its length, -1 if absent (0 is a stored empty value: the reference
 * tests `is not None`).  miss_mask_out: ceil(n/8) bytes in the hit-mask layout, bit i set iff no
 * memtable holds key i, pad bits zero: ANDed into the tables' candidate masks, a key a memtable
 * answered is searched in no table.  on_device / stream as pbf_sst_get. */
int pbf_mt_get(pbf_memtable_t* const* mts, uint32_t nmts, const uint8_t* keys, const uint64_t* offsets, uint32_t key_len,
               uint64_t n, int on_device, void* stream, int32_t* src_out, uint64_t* val_off_out, int32_t* val_len_out,
               uint8_t* miss_mask_out);

/* pbf_sst_gather for a batch whose hits come partly from memtables and partly from tables
 * (LsmStorage.get's return value, lsm_storage.py:155-179): where[i] >= 0 names tables[where[i]]
 * (val_off into its data section), -2 - m names mts[m] (val_off into its value bytes), -1 nothing.
 * Outputs, capacities, on_device and stream as pbf_sst_gather; ntables may be 0. */
int pbf_mt_gather(pbf_memtable_t* const* mts, uint32_t nmts, pbf_sstable_t* const* tables, uint32_t ntables,
                  const int32_t* where, const uint64_t* val_off, const int32_t* val_len, uint64_t n, uint8_t* out_bytes,
                  uint64_t out_cap, uint64_t* out_offsets, int on_device, void* stream);

/* pbf_sst_scan_size / pbf_sst_scan with the memtables' iterators in front of the tables', as
 * LsmStorage.scan builds its MergingIterator (lsm_storage.py:184-190): the sources are mts[0..],
 * then tables[0..], the lowest source index wins a key; segment index q * (nmts + ntables) + u.
 * Ranges, outputs, capacities, totals, on_device and stream are exactly those of the table calls.
 * ntables may be 0; nmts == 0 is refused (pbf_sst_scan is that call); nranges * (nmts + ntables) <=
 * PBF_SCAN_MAX_SEGMENTS.  A memtable range is SSTable.scan's: inclusive at both ends, lower > upper
 * empty, upper_open = no upper bound.  (The reference's MemTable.scan, memtable.py:81-86 over
 * red_black_tree.py:56-69, drops in-range keys and is not reproduced: DESIGN.md section 3.) */
int pbf_mt_scan_size(pbf_memtable_t* const* mts, uint32_t nmts, pbf_sstable_t* const* tables, uint32_t ntables,
                     const uint8_t* lowers, const uint64_t* lower_offsets, const uint8_t* uppers,
                     const uint64_t* upper_offsets, const uint8_t* upper_open, uint64_t nranges, uint32_t* seg_lo_out,
                     uint32_t* seg_hi_out, uint64_t* n_in, uint64_t* key_bytes_in, uint64_t* value_bytes_in);
int pbf_mt_scan(pbf_memtable_t* const* mts, uint32_t nmts, pbf_sstable_t* const* tables, uint32_t ntables,
                const uint8_t* lowers, const uint64_t* lower_offsets, const uint8_t* uppers, const uint64_t* upper_offsets,
                const uint8_t* upper_open, uint64_t nranges, uint8_t* keys_out, uint64_t keys_cap,
                uint64_t* key_offsets_out, uint8_t* values_out, uint64_t values_cap, uint64_t* value_offsets_out,
                uint64_t offsets_cap, uint64_t* n_out, uint64_t* key_bytes_out, uint64_t* value_bytes_out,
                uint64_t* range_offsets_out, int on_device, void* stream);

/* LsmStorage._do_flush (lsm_storage.py:193-205) of a resident memtable: pbf_flush_begin without the
 * upload and the sort, over a device copy of the memtable's run (the memtable stays as it is and may
 * be destroyed before the job is finished).  An empty memtable is refused as n == 0 is there.  The
 * job is finished by pbf_job_finish or freed by pbf_job_abort. */
int pbf_mt_flush_begin(pbf_memtable_t* mt, uint64_t block_size, pbf_job_t** job);

/* Synthetic keys straight into device memory (bench / tests; definitions in
 * pebbledb_amd/keys.py): 16 hex chars of splitmix64(seed + start + i), and the variable-length
 * 8..64-byte family (offsets must already hold the n+1 offsets, relative to offsets[0]).
 * stream = NULL: the keys are complete on return (filters run on non-blocking streams, which the
 * null stream does not order); otherwise asynchronous on `stream`. */
int pbf_gen_splitmix_hex(int device, void* stream, uint8_t* out_dev, uint64_t seed, uint64_t start, uint64_t n);
int pbf_gen_varlen(int device, void* stream, uint8_t* out_dev, const uint64_t* offsets_dev, uint64_t seed,
                   uint64_t start, uint64_t n);

/* Message of the last failure on this thread ("" if none). */
const char* pbf_last_error(void);

/* sha256 (hex) of the kernel sources the library was compiled from (pebbledb_amd/build.py
 * source_digest()); the Python binding refuses a library whose digest is not the tree's. */
const char* pbf_source_digest(void);

#ifdef __cplusplus
}
#endif
#endif /* PEBBLEBLOOM_H */
