/*
 * polyhip.h -- C ABI of libpolyhip.so: the MI355X (gfx950) implementation of
 * bebop/poly's search hot path.
 *
 * The reference (pure Go, no FFI of its own) exposes this path as the
 * exported API of four packages; a drop-in keeps those Go signatures and
 * binds the entry points below through cgo (stubs: INTEGRATION.md, go/).
 * Each entry point names the reference function it replaces; citations are
 * relative to the reference checkout.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only.
 *  - Every function returns POLYHIP_OK (0) or a negative polyhip_status; the
 *    message of the last failure on the calling thread is
 *    polyhip_last_error().
 *  - Two flavours per operation:
 *      NAME      host pointers (what cgo hands over).  Synchronous: stages
 *                through device memory on the current device and returns
 *                when the outputs are written.
 *      NAME_dev  device pointers + a hipStream_t (passed as void*; NULL = the
 *                null stream).  Asynchronous: enqueues on the stream and
 *                returns; inputs/outputs stay resident in HBM.
 *  - Batches are packed: one contiguous byte buffer + (n+1) uint64 offsets,
 *    sequence i = bytes [offsets[i], offsets[i+1]).  The library never keeps
 *    a caller pointer after returning (cgo pointer rule).
 *  - Thread safe: no unsynchronised globals; the current HIP device of the
 *    calling thread is used (polyhip_set_device is a thin hipSetDevice).
 *  - There is NO CPU fallback: without a usable HIP device every compute
 *    entry point fails with POLYHIP_ERR_HIP.
 *  - Sequence bytes must be ASCII (< 0x80) wherever the reference would
 *    case-fold or map them through string(byte) (Go treats bytes >= 0x80 as
 *    UTF-8 there); such input is rejected with POLYHIP_ERR_INVALID rather
 *    than silently diverging.
 */
#ifndef POLYHIP_H
#define POLYHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POLYHIP_ABI_VERSION 1

typedef enum {
    POLYHIP_OK = 0,
    POLYHIP_ERR_INVALID = -1,     /* bad argument (null pointer, unsorted offsets, ...) */
    POLYHIP_ERR_HIP = -2,         /* HIP runtime / device failure (message has the hipError) */
    POLYHIP_ERR_UNSUPPORTED = -3, /* outside the implemented range (documented per call) */
    POLYHIP_ERR_PANIC = -4,       /* the reference would panic on these arguments */
    POLYHIP_ERR_SYMBOL = -5       /* align: "Symbol X not in alphabet" (see polyhip_sw_*) */
} polyhip_status;

typedef void *polyhip_stream_t; /* hipStream_t */

/* ---- runtime --------------------------------------------------------- */
int polyhip_abi_version(void);
const char *polyhip_last_error(void); /* thread-local, never NULL */
int polyhip_device_count(void);       /* >= 0, or a negative status */
int polyhip_set_device(int device);
/* name of the current device's gcnArch (e.g. "gfx950:sramecc+:xnack-") */
int polyhip_device_arch(char *buf, size_t buflen);

/* ---- one host call over several GPUs  (polyhip_init(n_devices); 8e) ---- */
/*
 * The reference is single-threaded Go (search/mash/mash.go:68-140, search/align/align.go:171-232,
 * primers/primers.go:70-128, seqhash/seqhash.go:127-224 are plain loops); a Go host that keeps that API has ONE call
 * per batch, so the node's GPUs have to be reached from inside that call.  The library keeps one device list per
 * process.  Empty (the default): every host-pointer entry point runs on the calling thread's current device.  With n
 * entries the host-pointer entry points
 *     polyhip_mash_sketch_batch, polyhip_mash_distance_matrix, polyhip_mash_sketch_distance_matrix,
 *     polyhip_sw_batch, polyhip_sw_align_batch, polyhip_sw_align_batch_packed, polyhip_nw_align_batch,
 *     polyhip_santalucia_scan, polyhip_santalucia_scan_first, polyhip_santalucia_batch, polyhip_marmurdoty_batch,
 *     polyhip_least_rotation_batch, polyhip_seqhash_batch
 * cut their batch into n contiguous shards balanced by bytes (reads, pairs, window starts, matrix rows: SURVEY 8e's
 * partitioning; no data-path collective) and run shard q on a worker thread that lives on device ids[q], each with
 * its own streams and two-slot upload / compute / download pipeline, results written straight into the caller's
 * buffers.  Results, error codes and messages are those of the one-device call (the status reported is the lowest
 * failing shard's, i.e. the first failure in batch order; positions in messages are positions of the whole batch).
 * An id may appear more than once ("0,0,0"): the shards then share that GPU (testing on a one-GPU box).  The _dev
 * entry points, the feeders, the polyhip_bwt_* calls (they run on their handle's device) and polyhip_scoring_create are not affected (a scoring handle is copied to the other
 * devices of the list on first use).  polyhip_sw_last_path and friends then describe the first non-empty shard's kernels.
 *   polyhip_set_devices(ids, n)  n = 0 clears the list.  Calls in flight finish on the list they started with.
 *   polyhip_get_devices          -> the list's length (ids filled up to `capacity`).
 *   polyhip_init(n)              = polyhip_set_devices({0 .. n-1}); n <= 0: every visible device.
 *   polyhip_shutdown()           = polyhip_set_devices(NULL, 0).
 *   POLYHIP_DEVICES=0,1,2 | all  in the environment: the list a process starts with (read once, at the first
 *                                host-pointer call, unless polyhip_set_devices came first).
 */
int polyhip_set_devices(const int *ids, int n);
int polyhip_get_devices(int *ids, int capacity);
int polyhip_init(int n_devices);
int polyhip_shutdown(void);

/* ---- synthetic inputs (bench/test plumbing) ------------- */
/* d_out[i] = "ACGT"[(x >> 2*(i&31)) & 3], x = splitmix64 output number
 * (first + i)/32 + 1 of the stream seeded with `seed`; `first` must be a
 * multiple of 32 (lets ranks generate disjoint slices of one stream). */
int polyhip_synth_dna_dev(uint64_t seed, uint64_t first, uint8_t *d_out,
                          uint64_t n, polyhip_stream_t stream);

/* ---- K1: search/mash (*Mash).Sketch  (search/mash/mash.go:68-104) ------ */
/*
 * For every sequence i: hash each of the (len_i - k) windows (the reference
 * skips the last k-mer, mash.go:73) with MurmurHash3_x86_32 seed 0
 * (murmur3.Sum32, mash.go:76) over the raw bytes, and leave in
 * out[i*s .. i*s+s) exactly what Sketch leaves in Mash.Sketches:
 *   len_i - k >= s : the s smallest hashes, ascending, duplicates kept;
 *   0 < len_i - k < s : out[i*s + j] = hash of window j for j < len_i - k,
 *                       remaining entries NOT written (caller's prior state
 *                       survives, as in the reference);
 *   len_i - k <= 0 : nothing written.
 * So `out` is in/out: pass the current Sketches (zeros after mash.New).
 * Range: any k; s <= 2^24.  SketchSize up to 8192 with KmerSize up to 4096 run the LDS-resident kernels (k = 17 / 21 / 31
 * specialised); beyond that (mash.New(21, 10000) is ordinary usage) a kernel that hashes every window straight from
 * global memory and keeps its candidates in a stream-ordered scratch allocation (hipMallocAsync / hipFreeAsync on
 * `stream`) -- same results, about an order of magnitude slower per k-mer.
 * s < 2 is the reference's behaviour READ BY READ (mash.go:96,98 index Sketches[-1]): with s == 0 a sequence panics iff it
 * has a window (len > k); with s == 1 window 0 fills Sketches[0] and the sequence panics iff a LATER window hashes below
 * it.  If any sequence of the batch would panic the call returns POLYHIP_ERR_PANIC naming the first one (rows of the
 * sequences that do not panic are written as the reference leaves them, the others are left alone); otherwise
 * POLYHIP_OK.  This one case synchronises `stream` (the verdict comes from the device).
 */
int polyhip_mash_sketch_batch(const uint8_t *seqs, const uint64_t *offsets,
                              uint64_t n, uint32_t k, uint32_t s,
                              uint32_t *out);
int polyhip_mash_sketch_batch_dev(const uint8_t *d_seqs,
                                  const uint64_t *d_offsets, uint64_t n,
                                  uint32_t k, uint32_t s, uint32_t *d_out,
                                  polyhip_stream_t stream);

/* ---- K2: search/mash (*Mash).Similarity / Distance  (search/mash/mash.go:107-140) */
/*
 * For two sets of sketches X (nx x sx, the receivers) and Y (ny x sy):
 *     d_counts[i * ld + j] = sameHashes of X_i.Similarity(Y_j)   (mash.go:108-132)
 * i.e. the reference's result before the division, INCLUDING its behaviour on
 * sketches that are not ascending (a sequence with fewer than SketchSize
 * windows leaves a positional, zero/stale-padded sketch, mash.go:81-84): those
 * pairs run the reference's own range early-out + merge loop.  All-vs-all on
 * one GPU: X == Y.  Sharded over ranks: Y = the all-gathered sketches, X = this
 * rank's row block of Y, d_counts = its row block of the matrix.
 * Similarity = counts / min(sx, sy); Distance = 1 - that (next call).
 * SketchSize 0 -> POLYHIP_ERR_PANIC (mash.go:117 indexes Sketches[-1]).
 * Range: sx, sy <= 65535; nx, ny < 2^31.  A Y set of 2^32 hashes or more is joined in column stripes of fewer than
 * that, one index after the other in the same workspace (polyhip_mash_shared_counts_dev only; the index_build / reuse
 * pair keeps ONE index and so ny*sy < 2^32).  POLYHIP_K2_MAX_ITEMS=<n> lowers the stripe bound (testing aid).
 * d_work: polyhip_mash_shared_counts_workspace_bytes(...) bytes of scratch.
 */
size_t polyhip_mash_shared_counts_workspace_bytes(uint64_t nx, uint32_t sx,
                                                  uint64_t ny, uint32_t sy);
int polyhip_mash_shared_counts_dev(const uint32_t *d_X, uint64_t nx,
                                   uint32_t sx, const uint32_t *d_Y,
                                   uint64_t ny, uint32_t sy,
                                   uint16_t *d_counts, uint64_t ld,
                                   void *d_work, size_t work_bytes,
                                   polyhip_stream_t stream);
/*
 * The same in two steps, for callers that put several X against one Y (row blocks of one matrix, queries against a
 * resident sketch database): polyhip_mash_index_build_dev builds Y's inverted index into d_work (a third of a
 * 12,500 x 100,000 block's time), polyhip_mash_shared_counts_reuse_dev joins an X against the index that an earlier
 * polyhip_mash_index_build_dev / polyhip_mash_shared_counts_dev call with the SAME d_Y, ny, sy left in the SAME
 * d_work (the Y side sits at the front of the workspace, wherever nx puts the rest).  Workspace:
 * polyhip_mash_shared_counts_workspace_bytes(largest nx, ...); index_build alone needs ..._workspace_bytes(0, ...).
 */
int polyhip_mash_index_build_dev(const uint32_t *d_Y, uint64_t ny, uint32_t sy,
                                 void *d_work, size_t work_bytes,
                                 polyhip_stream_t stream);
int polyhip_mash_shared_counts_reuse_dev(const uint32_t *d_X, uint64_t nx,
                                         uint32_t sx, const uint32_t *d_Y,
                                         uint64_t ny, uint32_t sy,
                                         uint16_t *d_counts, uint64_t ld,
                                         void *d_work, size_t work_bytes,
                                         polyhip_stream_t stream);
/*
 * The index built in PARTS (multi-rank all-vs-all: SURVEY 8e, BASELINE configs[2]).  Every rank holds the same
 * gathered Y; rank r calls polyhip_mash_index_build_part_dev(part = r, nparts = nranks): it runs the cheap whole-set
 * steps (ascending check, coarse histogram) and then sorts only ITS share of the value range -- coarse buckets chosen from
 * the histogram so that every part holds about the same number of items -- writing its items and bucket starts at their
 * FINAL offsets in d_work.  polyhip_mash_index_allgather_dev then exchanges the parts in place (two ragged RCCL
 * all-gathers, polyhip_allgatherv_dev) and finishes the header; after it polyhip_mash_shared_counts_reuse_dev works as
 * after polyhip_mash_index_build_dev.  Both calls synchronise `stream` once (the part bounds are read from the device's
 * histogram).  Building parts 0 .. nparts-1 one after the other into ONE workspace, then polyhip_mash_index_finalize_dev,
 * gives the same index as polyhip_mash_index_build_dev (same bucket starts; the same items in every bucket, in whatever
 * order the atomics put them) -- how the parts are tested on one GPU.  polyhip_mash_index_part_spans reports where the
 * parts sit: item_spans / start_spans get nparts + 1 byte offsets into d_work each (part p = [spans[p], spans[p+1])); it
 * synchronises `stream` as well (the spans are host values computed from the device's histogram and header).
 */
struct polyhip_comm;
int polyhip_mash_index_build_part_dev(const uint32_t *d_Y, uint64_t ny, uint32_t sy,
                                      uint32_t part, uint32_t nparts,
                                      void *d_work, size_t work_bytes,
                                      polyhip_stream_t stream);
int polyhip_mash_index_part_spans(uint64_t ny, uint32_t sy, uint32_t nparts,
                                  const void *d_work, size_t work_bytes,
                                  uint64_t *item_spans, uint64_t *start_spans,
                                  polyhip_stream_t stream);
int polyhip_mash_index_finalize_dev(uint64_t ny, uint32_t sy, void *d_work,
                                    size_t work_bytes, polyhip_stream_t stream);
/* The three read-backs below (polyhip_mash_index_format_dev, polyhip_mash_index_build_info_dev,
 * polyhip_mash_shared_counts_mode_dev) take no stream: each waits for ALL work outstanding on the current device
 * (hipDeviceSynchronize) and then copies the workspace's header, so it reports the last build or join enqueued on that
 * workspace whatever stream it was enqueued on -- a non-blocking one included.  They are diagnostics: keep them out of a
 * pipeline that must stay asynchronous. */
/* Bytes per item of the index in d_work (synchronous read-back; tests, profiling, sizing an exchange): 8 = (value, sketch
 * id | occurrence number); 4 = the compact form the build picks ON THE DEVICE when the join to come is the one-stripe dense
 * join (up to ~113k columns of 10-bit counters) and the value's bits below its bucket plus the largest multiplicity of a
 * hash inside one sketch fit 11 bits: the item then carries the LDS counter it bumps (dword and field), so the join's
 * inner step is subtract, compare, two shifts, and, ds_add.  An index built on its own assumes X sets of Y's SketchSize;
 * a join that does not fit that assumption rebuilds the index with 8-byte items first.  POLYHIP_K2_COMPACT=0 keeps the
 * 8-byte items (testing aid). */
int polyhip_mash_index_format_dev(const void *d_work, uint32_t *item_bytes);
/* How the index in d_work was built (synchronous read-back; tests and profiling).  info[0]: 0 = the two-level build on
 * 8-byte intermediate items, 1 = the sliced build on 4-byte intermediate items (the default where its conditions hold:
 * compact items, SketchSize <= 1024, <= 131,072 sketches, 2^16 <= largest hash < 2^30, 4 <= bucket shift <= 10; the device
 * decides the last three), 2 = the sliced build was planned and called off on the device (a sketch repeats a hash more
 * often than a compact item numbers, or more than 65,536 repeated hashes): the two-level build ran.  For the sliced
 * build info[1] = coarse buckets (hash >> 16), info[2] = parts of the value range, info[3] = coarse buckets per part,
 * info[4] = coarse buckets level 2 could not hold in registers (two passes), info[5] = repeated hashes it numbered.
 * POLYHIP_K2_B4=0 keeps the two-level build (testing aid; the parts API and the in-process item exchange always use it). */
int polyhip_mash_index_build_info_dev(const void *d_work, uint32_t info[6]);
int polyhip_mash_index_allgather_dev(struct polyhip_comm *c, uint64_t ny,
                                     uint32_t sy, void *d_work,
                                     size_t work_bytes, polyhip_stream_t stream);
/* What the last polyhip_mash_shared_counts_dev call on this workspace did
 * (synchronous read-back; tests and profiling): mode 0 = hash join, 1 = the
 * reference's merge for every pair; the number of non-ascending sketches on
 * each side; the rows the join handed to the merge (more related sketches
 * than its LDS table holds); the index's self-join size sum_b |Y_b|^2.
 * Any pointer may be NULL. */
int polyhip_mash_shared_counts_mode_dev(const void *d_work, uint32_t *mode,
                                        uint32_t *n_irregular_x,
                                        uint32_t *n_irregular_y,
                                        uint32_t *n_overflow_rows,
                                        uint64_t *join_estimate);
/* d_dist[i * ld_dist + j] = 1 - float64(counts[i][j]) / float64(min(sx, sy))
 * (mash.go:134,139; so 8 shared of 10 gives 0.19999999999999996). */
int polyhip_mash_distance_from_counts_dev(const uint16_t *d_counts,
                                          uint64_t nx, uint64_t ny,
                                          uint64_t ld_counts, uint32_t sx,
                                          uint32_t sy, double *d_dist,
                                          uint64_t ld_dist,
                                          polyhip_stream_t stream);
/* host flavour: counts (nx*ny u16) and/or dist (nx*ny f64) may be NULL. */
int polyhip_mash_distance_matrix(const uint32_t *X, uint64_t nx, uint32_t sx,
                                 const uint32_t *Y, uint64_t ny, uint32_t sy,
                                 uint16_t *counts, double *dist);
/*
 * BASELINE configs[2] in one host call: mash.New(k, s).Sketch(seq_i) for every sequence of a packed batch
 * (mash.go:59-104), then X_i.Similarity(X_j) / X_i.Distance(X_j) for every ordered pair (mash.go:107-140) -- the two
 * nested loops a caller of the reference writes.  The sketches stay in HBM between the two steps.
 *   sketches  n * s in/out like polyhip_mash_sketch_batch's `out` (prior Sketches in, new ones out), or NULL: zeros in
 *             (= mash.New), nothing out.
 *   counts    n * n sameHashes (u16), and/or  dist  n * n float64 Distance; either may be NULL (both NULL: sketch only).
 * On a device list (polyhip_set_devices) this is SURVEY 8e's flow inside one process: the reads shard by bytes, every
 * device sketches its shard, and the devices build ONE index of all n sketches together without gathering the sketches
 * (round 4): each runs the index's first level on its own rows, the 8-byte items travel by value range
 * (hipMemcpyPeerAsync -- no RCCL, no process per device), the second level runs on 1/N of the range per device, the
 * finished parts are exchanged; each device then joins the rows it sketched, which go straight into the caller's
 * matrix.  A set with an irregular sketch (a read with fewer than s windows: its pairs take the reference's merge,
 * which reads raw sketches), a matrix too wide for the dense join, or POLYHIP_K2_EXCHANGE=0 take the gather instead:
 * the devices pull each other's sketches and each builds the whole index.  polyhip_mash_sketch_distance_matrix_last_path
 * says which ran.  Range: s <= 65535, n < 2^31.  SketchSize < 2: the status of
 * polyhip_mash_sketch_batch (the reference panics in Sketch); SketchSize 0 with a matrix asked for: POLYHIP_ERR_PANIC
 * (mash.go:117).
 */
int polyhip_mash_sketch_distance_matrix(const uint8_t *seqs,
                                        const uint64_t *offsets, uint64_t n,
                                        uint32_t k, uint32_t s,
                                        uint32_t *sketches, uint16_t *counts,
                                        double *dist);
/* the calling thread's last polyhip_mash_sketch_distance_matrix: 0 = one device, 1 = a device list with the item exchange,
 * 2 = a device list with the sketch gather (tests) */
int polyhip_mash_sketch_distance_matrix_last_path(void);
/* What the calling thread's last polyhip_mash_sketch_distance_matrix did (round 5: so that the first run on more than one
 * physical GPU explains itself).  path as above; devices = entries of the device list (1 without one); the device-to-device
 * copies of the call -- rows of sketches on the gather path, index items and finished index parts on the exchange path --
 * counted by TRANSPORT: peer (hipDeviceCanAccessPeer said yes and peer access is on: xGMI), staged (it said no: the runtime
 * bounces the copy through host memory -- correct, and several times slower) and local (both ends on one device: a list
 * that names a device twice); the bytes they moved; wall milliseconds of the call's rounds as the calling thread saw them
 * (each round ends when its slowest device does): sketching, the index (exchange path: its five rounds; gather path: 0,
 * the index is built inside the join), and the join incl. the rows' way back to the host. */
typedef struct polyhip_matrix_info {
    int32_t path, devices;
    int32_t peer_copies, staged_copies, local_copies, reserved;
    uint64_t bytes_peer, bytes_staged, bytes_local;
    double ms_sketch, ms_index, ms_join;
} polyhip_matrix_info;
int polyhip_mash_sketch_distance_matrix_last_info(polyhip_matrix_info *info);

/* ---- K2 neighbour lists: the all-vs-all answered as CSR instead of a dense matrix ----
 * shared(i, j) is the cell (i, j) of polyhip_mash_shared_counts_dev (mash.go:107-132, the early-out of :117 and irregular
 * sketches included).  Row i of the list keeps the entries (j, shared) with
 *     shared(i, j) >= min_shared            (min_shared >= 1: pairs without a shared hash are never listed; 0 is
 *                                            POLYHIP_ERR_INVALID)
 *     j != i + self_offset                  if exclude_self (self_offset = the column of X's row 0 when X is a row block of Y)
 *     the k largest shared, ties towards the smaller column, if k > 0 (a row with fewer candidates returns all of them)
 * as CSR: first uint64[nx + 1] (first[0] = 0), cols uint32, shared uint16, dist float64 = 1 - shared / min(sx, sy) (the
 * value polyhip_mash_distance_from_counts_dev writes for that cell; may be NULL).  Rows in order; inside a row ascending
 * column (k == 0) or shared descending, then column ascending (k > 0).  The same input gives the same bytes.
 * capacity = entries cols / shared / dist hold: first[] ALWAYS carries the true counts and nothing is written beyond the
 * capacity, so a caller whose buffers were too small (first[nx] > capacity) resizes and repeats the call; cols = shared =
 * NULL asks for the counts alone.
 * Y may hold up to 2^31 sketches: it is joined in column blocks of one dense stripe (about 105k sketches at SketchSize <=
 * 1023), each with its own index, one after the other in the workspace.  SketchSize 0 / > 65535 as
 * polyhip_mash_shared_counts_dev; nx == 0 or ny == 0: the empty list.  The call synchronises `stream` (once per row range).
 * d_work: polyhip_mash_neighbors_workspace_bytes(...) bytes.  It holds the block index and a temporary list of
 * max(1024 * nx, ny) entries; rows that need more are joined again in pieces (polyhip_neighbors_info.row_chunks > 1). */
/* Largest k of the top-k form: the selection is k rounds over a row's candidates on one wave, so a larger k is
 * POLYHIP_ERR_INVALID rather than a kernel that runs for minutes (threshold the list and select on the host instead). */
#define POLYHIP_MASH_NEIGHBORS_MAX_K 1024u
size_t polyhip_mash_neighbors_workspace_bytes(uint64_t nx, uint32_t sx,
                                              uint64_t ny, uint32_t sy);
int polyhip_mash_neighbors_dev(const uint32_t *d_X, uint64_t nx, uint32_t sx,
                               const uint32_t *d_Y, uint64_t ny, uint32_t sy,
                               uint32_t min_shared, uint32_t k,
                               int exclude_self, uint64_t self_offset,
                               uint64_t *d_first, uint32_t *d_cols,
                               uint16_t *d_shared, double *d_dist,
                               uint64_t capacity, void *d_work,
                               size_t work_bytes, polyhip_stream_t stream);
/* host flavour; on a device list (polyhip_set_devices) the rows of X shard over the devices, every device sees all of Y,
 * and the lists concatenate in row order. */
int polyhip_mash_neighbors(const uint32_t *X, uint64_t nx, uint32_t sx,
                           const uint32_t *Y, uint64_t ny, uint32_t sy,
                           uint32_t min_shared, uint32_t k, int exclude_self,
                           uint64_t self_offset, uint64_t *first,
                           uint32_t *cols, uint16_t *shared, double *dist,
                           uint64_t capacity);
/* What the calling thread's last polyhip_mash_neighbors / _dev did: column blocks of Y, index builds, row ranges joined
 * (1 unless the temporary list overflowed), the CSR assembly that ran (1 = one pass with reserved segments and a reorder
 * kernel), entries that passed the threshold and entries listed (after top-k), devices. */
typedef struct polyhip_neighbors_info {
    uint32_t column_blocks, index_builds, row_chunks, assembly;
    uint64_t entries_thresholded, entries;
    uint32_t devices, reserved;
} polyhip_neighbors_info;
int polyhip_mash_neighbors_last_info(polyhip_neighbors_info *info);

/* ---- K3: search/align SmithWaterman  (search/align/align.go:171-232) ---- */
/*
 * align.Scoring{SubstitutionMatrix, GapPenalty} (align.go:73-95) flattened
 * through the matrix's public Score() (its score table is unexported,
 * matrix.go:13-17):  lut[a*256 + b] = Score(string(byte a), string(byte b)),
 * validA[a] != 0 iff byte a is a symbol of FirstAlphabet, validB likewise
 * for SecondAlphabet (bytes >= 0x80 are never valid: string(byte) is a
 * two-byte UTF-8 string).  All three tables are HOST pointers (parameters,
 * not data) and are copied.  The handle owns small device tables on the HIP
 * device that is current at creation and must be used on that device.
 * Range: |gap| and |scores| such that  max|score| * (lenA + lenB) < 2^31.
 */
typedef struct polyhip_scoring polyhip_scoring;
int polyhip_scoring_create(const int32_t *lut256x256, const uint8_t *validA256,
                           const uint8_t *validB256, int64_t gap,
                           polyhip_scoring **out);
int polyhip_scoring_destroy(polyhip_scoring *sc);

/*
 * Score pass of SmithWaterman for a batch of pairs (A_p, B_p):
 *   H[i][j] = max(0, H[i-1][j-1] + S(a_i, b_j), H[i-1][j] + gap, H[i][j-1] + gap)
 * (align.go:192-195) with the reference's argmax: first maximum in row-major
 * order, i over A outer, j over B inner (strict '>' at align.go:197).
 * Outputs per pair p:
 *   score[p]        maxScore
 *   endA[p],endB[p] (maxScoreRow, maxScoreCol), 1-based; 0,0 when score == 0
 *   err[p]          0, or (which << 8) | symbol for the reference's
 *                   "Symbol X not in alphabet" error (align.go:189-191):
 *                   which = 1 (A / FirstAlphabet) or 2 (B / SecondAlphabet),
 *                   symbol = the byte the reference would name -- a[0] if
 *                   invalid, else the first invalid b[j], else the first
 *                   invalid a[i]; never set when either string is empty.
 *                   score/endA/endB are 0 for such pairs.
 * A is a packed batch (d_A, d_offA).  B is either ONE shared sequence
 * (d_offB == NULL, d_B[0..lenB)) or a packed batch (d_offB != NULL, lenB =
 * the maximum B length).  max_lenA >= every A length (the Go wrapper knows it
 * from packing; a longer A sets err[p] = 0xFFFFFFFF).
 * d_work: polyhip_sw_workspace_bytes(...) bytes of device scratch.
 */
size_t polyhip_sw_workspace_bytes(const polyhip_scoring *sc, uint64_t npairs,
                                  uint32_t max_lenA, uint64_t lenB,
                                  int shared_B);
int polyhip_sw_batch_dev(const polyhip_scoring *sc, const uint8_t *d_A,
                         const uint64_t *d_offA, uint64_t npairs,
                         uint32_t max_lenA, const uint8_t *d_B,
                         const uint64_t *d_offB, uint64_t lenB,
                         int64_t *d_score, uint32_t *d_endA, uint32_t *d_endB,
                         uint32_t *d_err, void *d_work, size_t work_bytes,
                         polyhip_stream_t stream);
/* Host-pointer flavour (cgo): same outputs in host memory. offB == NULL ->
 * shared B of length lenB. */
int polyhip_sw_batch(const polyhip_scoring *sc, const uint8_t *A,
                     const uint64_t *offA, uint64_t npairs, const uint8_t *B,
                     const uint64_t *offB, uint64_t lenB, int64_t *score,
                     uint32_t *endA, uint32_t *endB, uint32_t *err);
/*
 * Traceback of SmithWaterman (align.go:205-229) for the same batch, from the
 * score pass's outputs: walk back from (endA, endB) while H > 0 preferring
 * diagonal, then up (alignB gets '-'), then left (alignA gets '-').
 * Pair p's strings are the LAST d_alnLen[p] bytes of its aln_stride-byte slots:
 *     alignA_p = d_alnA[p*aln_stride + aln_stride - len .. p*aln_stride + aln_stride)
 * (the reference builds them by prepending).  Pairs with err != 0 or score 0
 * get length 0, as the reference returns "".
 * d_score (the score pass's output; may be NULL) lets each pair shrink its window:
 * a read that aligns well needs far fewer columns than the batch-wide bound.
 * aln_stride >= polyhip_sw_traceback_stride(sc, max_lenA, lenB).
 * d_work: any size >= 256 pairs' worth; polyhip_sw_traceback_workspace_bytes
 * returns enough for all pairs at once (capped at 8 GiB); smaller workspaces
 * make the call loop over chunks of pairs.  With several chunks the lane-per-pair
 * kernels run them through the two halves of the workspace on two streams -- `stream`
 * and one the library keeps per calling thread, joined to `stream` by events before
 * and after -- so that the end of a chunk overlaps the start of the next; everything
 * is ordered on `stream` as if it had run there (POLYHIP_TB_OVERLAP=0: it does).
 */
uint32_t polyhip_sw_traceback_stride(const polyhip_scoring *sc,
                                     uint32_t max_lenA, uint64_t lenB);
size_t polyhip_sw_traceback_workspace_bytes(const polyhip_scoring *sc,
                                            uint64_t npairs, uint32_t max_lenA,
                                            uint64_t lenB);
int polyhip_sw_traceback_dev(const polyhip_scoring *sc, const uint8_t *d_A,
                             const uint64_t *d_offA, uint64_t npairs,
                             uint32_t max_lenA, const uint8_t *d_B,
                             const uint64_t *d_offB, uint64_t lenB,
                             const uint32_t *d_endA, const uint32_t *d_endB,
                             const uint32_t *d_err, const int64_t *d_score,
                             uint8_t *d_alnA,
                             uint8_t *d_alnB, uint32_t *d_alnLen,
                             uint32_t aln_stride, void *d_work,
                             size_t work_bytes, polyhip_stream_t stream);
/*
 * The whole SmithWaterman on device pointers in one call: polyhip_sw_batch_dev + polyhip_sw_traceback_dev, same
 * outputs (d_work / d_tb_work sized as for those two).  For batches that take the packed score pass and the
 * byte-profile traceback (BASELINE config 4's shape: >= 48k reads of <= 152 symbols against one reference) the
 * score pass skips its locate step -- a second DP over the columns around each pair's maximum -- and the traceback
 * kernel, which sweeps those columns anyway, finds the row-major-first maximum in its last block: about 7 % less
 * time than the two calls.  The same holds for reads of 257..1024 symbols that take the packed multi-lane pass and the
 * one-wave-per-pair traceback on a byte profile of the pair (polyhip_sw_last_path 7 / polyhip_sw_traceback_last_path 7:
 * 80k reads of 1 kb, 92 -> 82 ms).  POLYHIP_SW_FUSE=0 in the environment keeps the two passes separate (testing aid).
 */
int polyhip_sw_align_batch_dev(const polyhip_scoring *sc, const uint8_t *d_A,
                               const uint64_t *d_offA, uint64_t npairs,
                               uint32_t max_lenA, const uint8_t *d_B,
                               const uint64_t *d_offB, uint64_t lenB,
                               int64_t *d_score, uint32_t *d_endA,
                               uint32_t *d_endB, uint32_t *d_err,
                               uint8_t *d_alnA, uint8_t *d_alnB,
                               uint32_t *d_alnLen, uint32_t aln_stride,
                               void *d_work, size_t work_bytes,
                               void *d_tb_work, size_t tb_work_bytes,
                               polyhip_stream_t stream);
/* Host-pointer flavour of the whole SmithWaterman: score pass + traceback.  With one shared reference and more than
 * ~200 MB of string slots the pairs go through two device slots in chunks of 262,144 (at most eight chunks): the strings
 * of one chunk cross PCIe while the next chunk is aligned.  POLYHIP_SW_HOST_CHUNKS=1..8 sets the chunk count (testing
 * aid; 1 = single shot). */
int polyhip_sw_align_batch(const polyhip_scoring *sc, const uint8_t *A,
                           const uint64_t *offA, uint64_t npairs,
                           const uint8_t *B, const uint64_t *offB,
                           uint64_t lenB, int64_t *score, uint32_t *endA,
                           uint32_t *endB, uint32_t *err, uint8_t *alnA,
                           uint8_t *alnB, uint32_t *alnLen,
                           uint32_t aln_stride);
/* The same with PACKED strings -- what a cgo caller wants (Go strings are made from slices, not from fixed-stride slots):
 * alignA_p = alnA[alnOff[p] .. alnOff[p+1]), alignB_p = the same range of alnB (the two strings of a pair have one
 * length); alnOff has npairs + 1 entries.  A pair's strings are a few hundred of its slot's bytes (151 of 525 at BASELINE
 * config 4), so compacting them on the device cuts the PCIe traffic of 1M reads from 1.05 GB to 0.3 GB.  aln_capacity =
 * bytes each of alnA / alnB holds; if the strings need more, the call returns POLYHIP_ERR_INVALID after filling score,
 * endA, endB, err and alnOff (alnOff[npairs] = the bytes needed).  Chunked through two slots like the call above. */
int polyhip_sw_align_batch_packed(const polyhip_scoring *sc, const uint8_t *A,
                                  const uint64_t *offA, uint64_t npairs,
                                  const uint8_t *B, const uint64_t *offB,
                                  uint64_t lenB, int64_t *score, uint32_t *endA,
                                  uint32_t *endB, uint32_t *err, uint8_t *alnA,
                                  uint8_t *alnB, uint64_t *alnOff,
                                  uint64_t aln_capacity);
/* ---- search/align SmithWaterman with affine gaps (Gotoh; no counterpart in the reference) ---- */
/*
 * S is the scoring handle's table.  gap_open = go and gap_extend = ge are added values, as GapPenalty is: the first symbol
 * of a gap costs go and each further one costs ge.  The handle's own gap is ignored.
 * Rows i run over A and columns j over B.  H[i][0] = H[0][j] = 0.  E[i][0] = F[0][j] = -inf.
 *   E[i][j] = max(H[i][j-1] + go, E[i][j-1] + ge)      gap in A (alignA gets '-')
 *   F[i][j] = max(H[i-1][j] + go, F[i-1][j] + ge)      gap in B (alignB gets '-')
 *   H[i][j] = max(0, H[i-1][j-1] + S(a_i, b_j), F[i][j], E[i][j])
 * With go == ge this is polyhip_sw_batch's recurrence with gap = go: score, end cell and both strings are the same.
 * Argmax: the first maximum in row-major order wins (strict '>'), as in polyhip_sw_batch.  endA and endB are 1-based, and
 * 0, 0 when the score is 0.
 * Traceback: it starts at (endA, endB) in state H and has three states.
 *   State H at (i,j): stop if H == 0.  If H == H[i-1][j-1] + S, emit (a_i, b_j) and move to (i-1, j-1).  Otherwise, if
 *     H == F[i][j], switch to state F.  Otherwise switch to state E.  (Diagonal, then up, then left, as in the reference.)
 *   State F at (i,j): emit (a_i, '-').  If F[i][j] == H[i-1][j] + go the next state is H (open is preferred over extend),
 *     otherwise the state stays F.  Then i -= 1.
 *   State E at (i,j): the same along the row: emit ('-', b_j), test E[i][j] == H[i][j-1] + go, then j -= 1.
 * The strings are built by prepending.
 * err: exactly as polyhip_sw_batch -- a[0], then the first invalid b[j], then the first invalid a[i]; never set when a
 * side is empty.  Such pairs get score 0 and empty strings.
 * Accepted range: go <= ge <= -1, and absmax * (max_lenA + lenB) < 2^30 where absmax = max(|smin|, |smax|, |go|) over
 * the handle's table; anything else is POLYHIP_ERR_UNSUPPORTED.  The gap check comes first, before the handle is looked
 * at.  NULL arguments and offsets that do not ascend are POLYHIP_ERR_INVALID.  npairs == 0 is an empty, successful call.
 * Cells are int32, exact over the whole accepted range.
 * Column window of the traceback: a pair with score s >= 1 that ends at (endA, endB) has a path that spans at most
 *   W_p = endA + floor((smax * endA - s) / -ge)
 * columns (with x diagonal and l left steps, s <= smax * x + ge * l and x <= endA), so its strings have at most
 * endA + min(endB, W_p - endA) bytes.  The traceback re-runs the DP on rows 1..endA and columns
 * (endB - min(endB, W_p), endB] with a zero boundary on the left: windowed values never exceed the true ones, and every
 * cell the true walk enters has its whole optimal path inside the window, so each equality the walk tests holds in the
 * window exactly when it holds in the full matrix.
 * These are host-pointer entry points, like polyhip_sw_batch and polyhip_sw_align_batch_packed: B is shared when
 * offB == NULL (lenB its length), else a packed batch.  alnOff and aln_capacity behave as in
 * polyhip_sw_align_batch_packed: alnOff (npairs + 1 entries) is always filled, and if the strings need more room the call
 * returns POLYHIP_ERR_INVALID with alnOff[npairs] = the bytes needed, after filling score, endA, endB and err.
 * The calls run on the scoring handle's device, on the calling thread's own streams, never on the null stream; the device
 * list does not apply.  The direction bits of the traceback (4 per cell of a pair's window) are sized from each pair's own
 * W_p; when they would exceed 1 GiB the call loops over chunks of pairs (POLYHIP_SWA_CHUNK_PAIRS=<n> in the environment
 * forces the chunk size: a testing aid).
 * polyhip_sw_affine_last_info: the calling thread's last affine call: pairs = npairs; cells = cell updates of the score
 * pass (lenA * lenB over the pairs without err); tb_cells = cell updates of the traceback windows (0 for the score call);
 * chunks = chunks of pairs the traceback looped over; rows_per_band = rows of A a lane holds in registers per sweep of the
 * columns; table_in_lds = 1 when the compact score table was staged in LDS, 0 when scores came from global memory.
 */
typedef struct polyhip_sw_affine_info {
    uint64_t pairs, cells, tb_cells, chunks, rows_per_band, table_in_lds;
} polyhip_sw_affine_info;
int polyhip_sw_affine_batch(const polyhip_scoring *sc, int64_t gap_open, int64_t gap_extend,
                            const uint8_t *A, const uint64_t *offA, uint64_t npairs,
                            const uint8_t *B, const uint64_t *offB, uint64_t lenB,
                            int64_t *score, uint32_t *endA, uint32_t *endB, uint32_t *err);
int polyhip_sw_affine_align_batch_packed(const polyhip_scoring *sc, int64_t gap_open, int64_t gap_extend,
                                         const uint8_t *A, const uint64_t *offA, uint64_t npairs,
                                         const uint8_t *B, const uint64_t *offB, uint64_t lenB,
                                         int64_t *score, uint32_t *endA, uint32_t *endB, uint32_t *err,
                                         uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff,
                                         uint64_t aln_capacity);
int polyhip_sw_affine_last_info(polyhip_sw_affine_info *info);
/* ---- search/align NeedlemanWunsch  (search/align/align.go:100-166) -------------- */
/*
 * Global alignment of every pair (A_p, B_p) (B shared when d_offB == NULL): score
 * = H[lenA][lenB] with the gap-penalty boundary (:112-120), aligned strings from the
 * reference's traceback, which stops when EITHER index reaches 0 (:141) -- so
 * ("", "GAT") gives score 3*gap and two empty strings.  err as polyhip_sw_batch.
 * Strings: last d_alnLen[p] bytes of the aln_stride-byte slots, aln_stride >=
 * max_lenA + lenB.  Workspace: polyhip_nw_workspace_bytes (whole direction matrix
 * per pair; the call loops over chunks of pairs if given less, >= 256 pairs' worth).
 * Range: |gap| and |scores| such that  max|score| * (max_lenA + lenB) < 2^31; beyond
 * that the call is refused with POLYHIP_ERR_UNSUPPORTED.
 */
size_t polyhip_nw_workspace_bytes(uint64_t npairs, uint32_t max_lenA,
                                  uint64_t max_lenB);
int polyhip_nw_align_batch_dev(const polyhip_scoring *sc, const uint8_t *d_A,
                               const uint64_t *d_offA, uint64_t npairs,
                               uint32_t max_lenA, const uint8_t *d_B,
                               const uint64_t *d_offB, uint64_t lenB,
                               int64_t *d_score, uint32_t *d_err,
                               uint8_t *d_alnA, uint8_t *d_alnB,
                               uint32_t *d_alnLen, uint32_t aln_stride,
                               void *d_work, size_t work_bytes,
                               polyhip_stream_t stream);
int polyhip_nw_align_batch(const polyhip_scoring *sc, const uint8_t *A,
                           const uint64_t *offA, uint64_t npairs,
                           const uint8_t *B, const uint64_t *offB,
                           uint64_t lenB, int64_t *score, uint32_t *err,
                           uint8_t *alnA, uint8_t *alnB, uint32_t *alnLen,
                           uint32_t aln_stride);

/* which kernel family the last polyhip_sw_batch*_dev call on this thread used (tests):
 * 1 = lane-per-pair register-tiled shared-B kernel, 2 = generic kernel, 3 = packed two-pairs-per-lane
 * pass + locate + one-wave-per-pair kernel for its ties, 4 = one-wave-per-pair kernel (small batches),
 * 5 = register-tiled kernel for per-pair B, 6 = one-wave-per-pair kernel for what those cannot take (reads of
 * 257..4096 symbols, gap >= 0, scores beyond int8; shared or per-pair B), 7 = reads of 257..2048 symbols
 * against one reference, enough of them to fill the chip: packed pass with 2..16 lanes per pair + the
 * one-wave-per-pair kernel over the columns that can reach the maximum.  POLYHIP_SW_WAVE=0 /
 * POLYHIP_SW_PACKED=0 / POLYHIP_SW_PAIR=0 in the environment switch 4, 6 and 7 / 3 and 7 / 5 off (testing aids). */
int polyhip_sw_last_path(void);
/* 1 when that call's packed pass (paths 3 and 7) ran the half-float cell of gfx950 (v_pk_maximum3_f16: three
 * instructions per cell pair instead of four) -- taken when every H stays below 2048, i.e. smax * min(max_lenA, lenB)
 * <= 2047 and smax + |gap| <= 2048; same integers, bit for bit (halves scaled by 2^-11, every sum exact).
 * POLYHIP_SW_F16=0 keeps the int16 cell (testing aid). */
int polyhip_sw_last_packed_half(void);
/* ... and over how many lanes that packed pass spread the rows of a lane's two read pairs (0: no packed pass): 1 = one
 * lane holds all rows (up to 64 rows; POLYHIP_SW_PK1X2=0), 2 = sw_pk1x2_kernel (65..152 rows: two lanes, four waves per
 * SIMD), 2..16 = sw_pkb_kernel's lanes per pair above 152 rows (64 rows per lane; POLYHIP_SW_TILE64=0: 128 / 152). */
int polyhip_sw_last_packed_lanes(void);
/* ... and the last polyhip_sw_traceback_dev call: 1 = byte-profile kernel (shared B, score given,
 * the reference's profile fits LDS), 2 = register-tiled table kernel, 3 = generic kernel, 4 = one-wave-per-pair
 * kernel for reads of 153..4096 symbols (tests; POLYHIP_TB_WAVE=0 switches 4 off), 5 = the half-float byte-profile
 * kernel with TWO LANES per pair (four bands of 64 rows) for reads of 153..256 symbols against one reference under the
 * half-float condition below (POLYHIP_TB_HALF2=0 or POLYHIP_TB_F16=0: path 4 instead; testing aids), 6 = the half-float
 * kernel for EVERY PAIR ITS OWN B (reads against reads): reads of at most 152 symbols, at most six symbol codes, score
 * given, the half-float condition -- a lane builds its own profile from its pair's B symbols (tb_pair16_kernel;
 * POLYHIP_TB_PAIR16=0 or POLYHIP_TB_F16=0: path 2 instead; testing aids), 7 = the one-wave-per-pair kernel for reads of
 * 257..1024 symbols with its sweep on a BYTE PROFILE of the pair in LDS (eight instructions per cell instead of sixteen):
 * gap <= -1, smax - gap <= 127, smin - gap >= -128, the planes of four pairs fit 64 KB (shared or per-pair B;
 * POLYHIP_TB_WAVE8=0: path 4 instead; testing aid).  Paths 4 and 7 walk out of the wave's registers on the scalar unit
 * (reads of at most 1024 symbols). */
int polyhip_sw_traceback_last_path(void);
/* 1 when that call's byte-profile kernel (path 1) ran in its half-float form (gfx950: packed halves, two bands of rows
 * per lane, nine instructions per cell pair instead of eighteen) -- taken under the packed score pass's condition
 * (every H < 2048) for reads of <= 152 symbols while the table of halves fits twice into a CU's LDS.
 * POLYHIP_TB_F16=0 keeps the 32-bit form (testing aid). */
int polyhip_sw_traceback_last_half(void);
/* ... and the last polyhip_nw_align_batch_dev call: 1 = register-tiled kernel (lenA <= 64), 2 = generic kernel
 * (POLYHIP_NW_GENERIC=1 forces it), 3 = one-wave-per-pair kernel (lenA 65..4096); tests. */
int polyhip_nw_last_path(void);

/* ---- K4: primers SantaLucia / MarmurDoty / MeltingTemp  (primers/primers.go:70-128) */
/*
 * SCAN: SantaLucia(seq[i : i+L], primer_conc, salt_conc, mg_conc)
 * (primers.go:70-105) for every start i in [start0, start0 + nstarts) and every
 * length L in [Lmin, Lmax] of ONE sequence of `len` bytes (the caller of
 * primers/pcr's grow-until-Tm loops, pcr.go:47-53, reads its answers from this
 * table).  Output planes, one per length:
 *     d_tm[(L - Lmin) * ld + (i - start0)]   (likewise d_dH, d_dS),  ld >= nstarts
 * A window that runs past the end of the sequence (i + L > len) gets quiet
 * NaNs.  start0/nstarts let each rank of a multi-GPU job scan its own slice of
 * the starts while reading its (Lmax - 1)-byte halo from the same buffer.
 * Results are bit-identical to the Go code: same fp64 operation order, no FMA
 * contraction, Go's math.Log algorithm for the two logarithms.
 * Lmin == 0 -> POLYHIP_ERR_PANIC (SantaLucia("") panics, primers.go:89).
 * Range: Lmax <= 1024.  MeltingTemp (primers.go:121-128) is this call with
 * (500e-9, 50e-3, 0).
 */
int polyhip_santalucia_scan_dev(const uint8_t *d_seq, uint64_t len,
                                uint64_t start0, uint64_t nstarts,
                                uint32_t Lmin, uint32_t Lmax,
                                double primer_conc, double salt_conc,
                                double mg_conc, double *d_tm, double *d_dH,
                                double *d_dS, uint64_t ld,
                                polyhip_stream_t stream);
/* host flavour: all starts 0 .. len - Lmin, ld = len - Lmin + 1; outputs hold
 * (Lmax - Lmin + 1) * ld doubles each.  Non-ASCII bytes -> POLYHIP_ERR_INVALID. */
int polyhip_santalucia_scan(const uint8_t *seq, uint64_t len, uint32_t Lmin,
                            uint32_t Lmax, double primer_conc,
                            double salt_conc, double mg_conc, double *tm,
                            double *dH, double *dS);
/*
 * SCAN, reduced on the chip: for every start the FIRST length L in [Lmin, Lmax] whose SantaLucia Tm is not below
 * target_tm -- the grow loop of primers/pcr (pcr.go:47-53: lengthen the primer while MeltingTemp < targetTm; the
 * same comparison, so a NaN Tm stops it too) for every position of a sequence at once.  d_first_len[i - start0] = that L
 * (0: no length up to Lmax reaches the target, or no window fits), d_first_tm (may be NULL) its Tm (a NaN where no
 * length was found).  2 + 8 bytes per start leave the chip instead of 24 per window: the host flavour of the
 * full scan is bound by PCIe (1.56 GB for a 5 Mb genome), this one is not.
 */
int polyhip_santalucia_scan_first_dev(const uint8_t *d_seq, uint64_t len,
                                      uint64_t start0, uint64_t nstarts,
                                      uint32_t Lmin, uint32_t Lmax,
                                      double primer_conc, double salt_conc,
                                      double mg_conc, double target_tm,
                                      uint16_t *d_first_len, double *d_first_tm,
                                      polyhip_stream_t stream);
int polyhip_santalucia_scan_first(const uint8_t *seq, uint64_t len, uint32_t Lmin,
                                  uint32_t Lmax, double primer_conc,
                                  double salt_conc, double mg_conc,
                                  double target_tm, uint16_t *first_len,
                                  double *first_tm);
/* BATCH: one SantaLucia call per packed sequence.  An empty sequence is
 * POLYHIP_ERR_PANIC in the host flavour (quiet NaN outputs in the _dev one). */
int polyhip_santalucia_batch_dev(const uint8_t *d_seqs,
                                 const uint64_t *d_offsets, uint64_t n,
                                 double primer_conc, double salt_conc,
                                 double mg_conc, double *d_tm, double *d_dH,
                                 double *d_dS, polyhip_stream_t stream);
int polyhip_santalucia_batch(const uint8_t *seqs, const uint64_t *offsets,
                             uint64_t n, double primer_conc, double salt_conc,
                             double mg_conc, double *tm, double *dH,
                             double *dS);
/* MarmurDoty (primers.go:108-118) per packed sequence. */
int polyhip_marmurdoty_batch_dev(const uint8_t *d_seqs,
                                 const uint64_t *d_offsets, uint64_t n,
                                 double *d_tm, polyhip_stream_t stream);
int polyhip_marmurdoty_batch(const uint8_t *seqs, const uint64_t *offsets,
                             uint64_t n, double *tm);

/* ---- K5: seqhash RotateSequence  (seqhash/seqhash.go:78-138) ------------------ */
/*
 * For every packed sequence: d_rot_index[i] = boothLeastRotation(seq_i)
 * (seqhash.go:78-124: the smallest index of the lexicographically least
 * rotation, byte order, no case folding), and -- if d_rotated != NULL, same
 * packed layout as the input -- RotateSequence(seq_i) = (seq_i + seq_i)[r : r+n]
 * (seqhash.go:127-138).  Empty and one-byte sequences give index 0.
 * max_len >= every sequence length (sizes the LDS staging).
 */
int polyhip_least_rotation_batch_dev(const uint8_t *d_seqs,
                                     const uint64_t *d_offsets, uint64_t n,
                                     uint64_t max_len, uint64_t *d_rot_index,
                                     uint8_t *d_rotated,
                                     polyhip_stream_t stream);
/* host flavour; rotated may be NULL, else it is indexed by the same offsets. */
int polyhip_least_rotation_batch(const uint8_t *seqs, const uint64_t *offsets,
                                 uint64_t n, uint64_t *rot_index,
                                 uint8_t *rotated);

/* ---- S2: seqhash.Hash  (seqhash/seqhash.go:141-224) --------------------------- */
/*
 * Hash(seq_i, sequenceType, circular, doubleStranded) for every packed sequence,
 * one (type, circular, doubleStranded) triple per call: upper-case, RNA U->T,
 * alphabet check, least rotation / reverse complement / bytewise-smaller choice,
 * BLAKE3-256, "v1_" + {D,R,P}{C,L}{D,S} + "_" + 64 hex digits.
 * seq_type: 0 DNA, 1 RNA, 2 PROTEIN; anything else -> POLYHIP_ERR_INVALID with the
 * reference's message (seqhash.go:152); PROTEIN + double_stranded likewise (:175).
 * d_out: n slots of 72 bytes (71 characters + NUL; empty string on error).
 * d_err[i]: 0, or (2 << 8) | letter for seqhash.go:157 ("Only letters
 * ATUGCYRSWKMBDHVNZ are allowed for DNA/RNA. Got letter: X"), (3 << 8) | letter
 * for seqhash.go:169 (proteins) -- the first offending letter, as the reference.
 * d_offsets[0] must be 0 (the normalised copy in the workspace is addressed by the
 * batch's own offsets; the host flavour rebases); total_bytes = d_offsets[n];
 * max_len >= every sequence length.
 */
size_t polyhip_seqhash_workspace_bytes(uint64_t n, uint64_t total_bytes,
                                       int circular, int double_stranded);
int polyhip_seqhash_batch_dev(const uint8_t *d_seqs, const uint64_t *d_offsets,
                              uint64_t n, uint64_t total_bytes,
                              uint64_t max_len, int seq_type, int circular,
                              int double_stranded, char *d_out,
                              uint32_t *d_err, void *d_work, size_t work_bytes,
                              polyhip_stream_t stream);
int polyhip_seqhash_batch(const uint8_t *seqs, const uint64_t *offsets,
                          uint64_t n, int seq_type, int circular,
                          int double_stranded, char *out, uint32_t *err);

/* ---- read feeder: io/fastq (*Parser).ParseNext / ParseN  (io/fastq/fastq.go:84-216) ---- */
/*
 * A FASTQ file image (d_file, nbytes) becomes the packed batch the kernels above take:
 * d_seqs = the Sequence of every record back to back, d_offsets[0..n] (n+1 entries),
 * d_rec_start[i] (optional) = byte offset of record i's identifier line, for the host to
 * slice identifiers lazily.  Records are four '\n'-terminated lines; a '\r' is not stripped;
 * parsing stops at the first bad record and the records before it are kept (ParseN).
 * d_result[0] = n records, [1] = error code (0 none; 1 no '@' (fastq.go:203), 2 empty
 * sequence (:176), 3 empty quality (:197), 4 unexpected EOF inside a record / last line
 * without '\n' (:142-148), 5 empty identifier line and 6 identifier field without '='
 * (the reference PANICS there, :156 and :163), 7 more records than max_records),
 * [2] = the line the reference's message names, [3] = total sequence bytes.
 * Capacities: d_seqs nbytes, d_offsets / d_rec_start nbytes/7 + 2 entries (or max_records + 1;
 * the shortest record is the 7 bytes "@\nA\n\nI\n": the third line is read unseen, fastq.go:182).
 */
size_t polyhip_fastq_workspace_bytes(uint64_t nbytes);
int polyhip_fastq_pack_dev(const uint8_t *d_file, uint64_t nbytes,
                           uint8_t *d_seqs, uint64_t *d_offsets,
                           uint64_t *d_rec_start, uint64_t max_records,
                           uint64_t *d_result, void *d_work, size_t work_bytes,
                           polyhip_stream_t stream);
int polyhip_fastq_pack(const uint8_t *file, uint64_t nbytes, uint8_t *seqs,
                       uint64_t *offsets, uint64_t *rec_start,
                       uint64_t max_records, uint64_t *result);
/*
 * polyhip_fastq_pack_qual: the same parse, which also packs the Quality field (fastq.go:199, 205-210).  Records, error
 * codes, line numbers, the ParseN rule, max_records and the capacities are polyhip_fastq_pack's; seqs, offsets, rec_start
 * and result[0..3] are what that call gives on the same image.  Quality of record i is line 4 without its '\n' (a '\r'
 * stays, no byte is interpreted), at quals[qual_offsets[i] .. qual_offsets[i + 1]), n + 1 offsets.  The reference does not
 * require len(Quality) == len(Sequence) and neither does this call: hence offsets of their own.
 * result has six words: [4] = total quality bytes of the n kept records, [5] = the number of kept records whose quality
 * length differs from their sequence length (polyhip_pileup_qual needs 0).
 * Capacities: quals nbytes, qual_offsets as offsets.  Host pointers only: the qualities are parsed, scanned and gathered on
 * the device in the passes of polyhip_fastq_pack_dev, but there is no device-resident flavour of this call yet.
 */
int polyhip_fastq_pack_qual(const uint8_t *file, uint64_t nbytes, uint8_t *seqs,
                            uint64_t *offsets, uint8_t *quals, uint64_t *qual_offsets,
                            uint64_t *rec_start, uint64_t max_records, uint64_t *result);

/* ---- read feeder: io/fasta (*Parser).ParseNext / ParseN  (io/fasta/fasta.go:102-238) ---- */
/*
 * Same contract as polyhip_fastq_pack for a FASTA image, multi-line records included, with
 * the reference's rules: empty lines and ';' lines are skipped, lines before the first '>'
 * are skipped, a '>' line directly after a header is SEQUENCE (fasta.go:197-204 looks at the
 * next line only after a line has been read), a last record ending in an unterminated line is
 * dropped (ParseNext returns it with io.EOF).  d_rec_start[i] = byte offset of record i's
 * header line.  d_result[0] = n records, [1] = error code (0 none; 1 no '>' in a non-empty
 * file (:223), 2 a header without sequence (:227) -- records before it are kept; 7 more
 * records than max_records), [2] = total sequence bytes, [3] = header lines seen.
 * Capacities: d_seqs nbytes; d_offsets / d_rec_start nbytes/2 + 3 entries.
 */
size_t polyhip_fasta_workspace_bytes(uint64_t nbytes);
int polyhip_fasta_pack_dev(const uint8_t *d_file, uint64_t nbytes,
                           uint8_t *d_seqs, uint64_t *d_offsets,
                           uint64_t *d_rec_start, uint64_t max_records,
                           uint64_t *d_result, void *d_work, size_t work_bytes,
                           polyhip_stream_t stream);
int polyhip_fasta_pack(const uint8_t *file, uint64_t nbytes, uint8_t *seqs,
                       uint64_t *offsets, uint64_t *rec_start,
                       uint64_t max_records, uint64_t *result);

/* ---- search/bwt: FM-index  (search/bwt/bwt.go:186-680) ---- */
/*
 * T = sequence + '$'; its suffixes sort with '$' lowest and every other byte by its unsigned value (bwt.go:563-581),
 * so 0x00..0x23 and '!' sort after '$'.  The sequence may hold any byte but '$' (0x00 and bytes >= 0x80 included).
 * A handle owns T, the suffix array (uint32), the last column L and an occurrence structure on the HIP device that is
 * current at creation; every polyhip_bwt_* call runs on that device and returns the calling thread to its own.  The
 * device list (polyhip_set_devices) does not apply to these calls, as it does not to the feeders.
 * Rows: the n + 1 rotations of T in sorted order.  A search result is the interval [start, end) of rows that begin
 * with the pattern, by LF backward search over the whole of L ('$' included): a pattern that holds '$' or is longer
 * than T matches cyclically ("a$", "$b" on "banana": 1 row each), a symbol that does not occur gives (0, 0), and every
 * empty result is reported as (0, 0).
 *
 * create (bwt.go:455-517): "Provided sequence must not by empty. BWT cannot be constructed" for n == 0 and
 *   "Provided sequence contains the nullChar $. BWT cannot be constructed", both POLYHIP_ERR_INVALID; n >= 2^32 - 1 is
 *   refused with POLYHIP_ERR_INVALID.  The suffix array is built on the device by prefix doubling (radix-sorted 64-bit
 *   keys); the layout of the occurrence structure depends on the alphabet (polyhip_bwt_layout: 0 = nucleotide, at
 *   most 4 distinct bytes, 2-bit L in 128-byte lines with their checkpoint counts; 1 = general; POLYHIP_BWT_GENERAL=1
 *   in the environment forces 1).  _dev: d_seq is device memory ordered on `stream`, d_work holds
 *   polyhip_bwt_workspace_bytes(n) bytes; the call synchronises `stream` (it reads back the alphabet and one group
 *   count per doubling round) and returns with the handle built.
 * len (bwt.go:301-304): n.  transform (bwt.go:306-323): L, n + 1 bytes with the '$'.  suffix_array: the n + 1 rows'
 *   text positions.  rounds: the doubling rounds the build took.
 * count (bwt.go:235-247, 353-404): one pattern of the packed batch per entry: start[p], end[p] as above, count =
 *   end - start; err[p] = 1 for an empty pattern ("Pattern can not be empty"), its interval (0, 0).
 * locate (bwt.go:249-273): first[0..npat] = exclusive scan of the interval widths; out[first[p] .. first[p+1]) =
 *   SA[start .. end) in row order, the reference's order (not sorted).  Host flavour: the batch's patterns in, always
 *   fills first[]; if first[npat] > capacity it writes nothing to out and fails with POLYHIP_ERR_INVALID naming the
 *   size needed.  _dev: intervals from polyhip_bwt_count_dev in; entries at or past `capacity` are not written (compare
 *   d_first[npat] with it); d_work: polyhip_bwt_locate_workspace_bytes(npat) bytes.
 * extract (bwt.go:275-299): request i = T[start[i], end[i]) written to out[out_off[i] ..); err[i] = 0, or the
 *   reference's first failing check: 1 "Start must be strictly less than end", 2 "end [E] exceeds the max range of the
 *   BWT [n]" (end > n), 3 "start [S] exceeds the min range of the BWT [0]", 4 the slot out_off[i+1] - out_off[i] is
 *   shorter than end - start.  The host flavour wants out_off[0] == 0.
 */
typedef struct polyhip_bwt polyhip_bwt;
size_t polyhip_bwt_workspace_bytes(uint64_t n);
int polyhip_bwt_create(const uint8_t *seq, uint64_t n, polyhip_bwt **out);
int polyhip_bwt_create_dev(const uint8_t *d_seq, uint64_t n, void *d_work,
                           size_t work_bytes, polyhip_stream_t stream,
                           polyhip_bwt **out);
int polyhip_bwt_destroy(polyhip_bwt *h);
int64_t polyhip_bwt_len(const polyhip_bwt *h);
int polyhip_bwt_layout(const polyhip_bwt *h);
int polyhip_bwt_rounds(const polyhip_bwt *h);
int polyhip_bwt_transform(const polyhip_bwt *h, uint8_t *out);
int polyhip_bwt_transform_dev(const polyhip_bwt *h, uint8_t *d_out,
                              polyhip_stream_t stream);
int polyhip_bwt_suffix_array(const polyhip_bwt *h, uint32_t *out);
int polyhip_bwt_count_dev(const polyhip_bwt *h, const uint8_t *d_pat,
                          const uint64_t *d_off, uint64_t npat,
                          uint32_t *d_start, uint32_t *d_end, uint32_t *d_err,
                          polyhip_stream_t stream);
int polyhip_bwt_count(const polyhip_bwt *h, const uint8_t *pat,
                      const uint64_t *off, uint64_t npat, uint32_t *start,
                      uint32_t *end, uint32_t *err);
size_t polyhip_bwt_locate_workspace_bytes(uint64_t npat);
int polyhip_bwt_locate_dev(const polyhip_bwt *h, const uint32_t *d_start,
                           const uint32_t *d_end, uint64_t npat,
                           uint64_t *d_first, uint32_t *d_out,
                           uint64_t capacity, void *d_work, size_t work_bytes,
                           polyhip_stream_t stream);
int polyhip_bwt_locate(const polyhip_bwt *h, const uint8_t *pat,
                       const uint64_t *off, uint64_t npat, uint64_t *first,
                       uint32_t *out, uint64_t capacity, uint32_t *err);
int polyhip_bwt_extract_dev(const polyhip_bwt *h, const int64_t *d_start,
                            const int64_t *d_end, uint64_t nreq,
                            const uint64_t *d_out_off, uint8_t *d_out,
                            uint32_t *d_err, polyhip_stream_t stream);
int polyhip_bwt_extract(const polyhip_bwt *h, const int64_t *start,
                        const int64_t *end, uint64_t nreq,
                        const uint64_t *out_off, uint8_t *out, uint32_t *err);

/* ---- search/bwt with mismatches: where a pattern almost occurs (no counterpart in the reference) ---- */
/*
 * S = the handle's sequence (n bytes, without the '$'), P a pattern of m >= 1 bytes, 0 <= k <= POLYHIP_BWT_MAX_MISMATCHES:
 *   hits(P, k) = { (p, d) : 0 <= p <= n - m,  d = #{ j : S[p + j] != P[j] } <= k }
 * Mismatches are substitutions only (no insertions or deletions).  Bytes are compared raw, as count does (no case
 * folding); a pattern byte that is '$' or does not occur in S costs one mismatch wherever it stands; m > n gives no hits.
 * Matches lie inside the sequence: they never run through the '$'.  For k = 0 this is count / locate restricted to
 * patterns without '$' and with m <= n -- the cyclic cases of the exact count ("a$" on "banana": 1 row) are NOT
 * reproduced here (0 hits).
 * The search is a backward search with backtracking over the handle's index (every symbol of the sequence's alphabet is
 * tried at cost 1 while mismatches are left; '$' is never tried), one pattern per lane.
 *
 * count_mismatch: counts[p * (k + 1) + d] = the positions at which pattern p has exactly d mismatches (each <= n).
 * locate_mismatch: first[0..npat] = exclusive scan of the per-pattern totals; pattern p's hits are pos[first[p] ..
 *   first[p + 1]), sorted by position ascending, and mm[] holds each hit's d.  Capacity as in polyhip_bwt_locate: first[] is
 *   always filled; if first[npat] > capacity nothing is written to pos / mm and the call fails with POLYHIP_ERR_INVALID
 *   naming the size needed.  No device buffer for hits is allocated before that check, so the caller's capacity bounds
 *   the allocation (29 bytes per hit: two (key, value) buffers of the sort and the result).
 * err[p] = 1 for an empty pattern ("Pattern can not be empty"), with zero counts and no hits; otherwise 0.  npat == 0 is
 * an empty, successful call (first[0] = 0).
 * Errors, in this order: k > POLYHIP_BWT_MAX_MISMATCHES is POLYHIP_ERR_UNSUPPORTED (before the handle is looked at); a
 * NULL handle or NULL arguments are POLYHIP_ERR_INVALID; offsets that do not ascend are POLYHIP_ERR_INVALID.
 * The calls run on the handle's device and stream, as polyhip_bwt_count does; the device list does not apply.
 * mismatch_last_info: the calling thread's last count_mismatch / locate_mismatch call: patterns = npat; nodes = live nodes
 *   of the search tree visited: the expanded ones and the leaves, which are not expanded, so nodes - leaves is the number
 *   of expansions; occ_lines = distinct 128-byte lines (nucleotide layout) or checkpoint blocks (general layout) that the
 *   expansions read: one per range end, one in all where both ends share it, so in the nucleotide layout
 *   nodes - leaves <= occ_lines <= 2 * (nodes - leaves) whatever k is; leaves = leaf intervals; hits = positions
 *   (= first[npat]).  locate runs the search twice (totals, then positions); the figures are those of one search.
 */
#define POLYHIP_BWT_MAX_MISMATCHES 4u
typedef struct polyhip_bwt_mismatch_info {
    uint64_t patterns, nodes, occ_lines, leaves, hits;
} polyhip_bwt_mismatch_info;
int polyhip_bwt_count_mismatch(const polyhip_bwt *h, const uint8_t *pat,
                               const uint64_t *off, uint64_t npat, uint32_t k,
                               uint32_t *counts, uint32_t *err);
int polyhip_bwt_locate_mismatch(const polyhip_bwt *h, const uint8_t *pat,
                                const uint64_t *off, uint64_t npat, uint32_t k,
                                uint64_t *first, uint32_t *pos, uint8_t *mm,
                                uint64_t capacity, uint32_t *err);
int polyhip_bwt_mismatch_last_info(polyhip_bwt_mismatch_info *info);

/* ---- read mapping: FM-index seeds, diagonal clusters, SmithWaterman extension (no counterpart in the reference) ---- */
/*
 * Places every read of a packed batch on the text T (n bytes) of a polyhip_bwt handle.  For a read r of m bytes:
 *  1. strands: s = 0 with q = r; if both_strands also s = 1 with q = ReverseComplement(r) (transform.go:15-23, 78-109:
 *     unmapped bytes become 0x00).
 *  2. seeds at offsets o = 0, S, 2S, ... while o + L <= m.  A seed's occurrences are all p with T[p, p + L) = q[o, o + L)
 *     (none when it holds '$' or a byte T lacks).  A seed with more than max_occ occurrences contributes nothing and is
 *     counted in the info; every other occurrence is a hit on the diagonal d = p - o (signed).  A max_occ above n means
 *     no limit (a seed has at most n occurrences; the workspace is sized for min(max_occ, n) hits per seed).
 *  3. clusters, per strand: with the hits sorted by d, a cluster opens at the smallest unassigned diagonal d0 and takes
 *     every hit with d <= d0 + W; votes = its hits, dmax = its largest diagonal.
 *  4. candidates: all clusters of both strands ordered by (votes descending, s ascending, d0 ascending); the first
 *     max_cand are kept, the position in this order is the rank.
 *  5. extension of every kept candidate: lo = max(0, d0 - W), hi = min(n, dmax + m + W), SmithWaterman(q, T[lo, hi)) as
 *     polyhip_sw_align_batch computes it.
 *  6. if a kept candidate gives the alphabet error the read is unmapped and err is the error of the lowest such rank
 *     (polyhip_sw_batch's encoding).  Otherwise the best candidate has the highest score, ties to the lowest rank, and the
 *     read is mapped iff there is one and its score >= min_score.  A mapped read gets: score; second = the highest score
 *     among its other kept candidates (0 if none); flags bit 0 = mapped, bit 1 = reverse strand; votes of the chosen
 *     candidate; ref_end = lo + endB, ref_start = ref_end - (non-'-' symbols of alignB); read_end = endA, read_start =
 *     endA - (non-'-' symbols of alignA), both in q's coordinates; the two aligned strings.  An unmapped read gets zeros
 *     and empty strings.  A read shorter than seed_len has no seeds (unmapped, err 0); one longer than max_len is unmapped
 *     with err 0xFFFFFFFF.  nreads == 0 is an empty, successful call.
 * Strings are packed as in polyhip_sw_align_batch_packed: read i's two strings are [alnOff[i], alnOff[i + 1]) of alnA and
 * alnB (nreads + 1 offsets); when aln_capacity is too small the call returns POLYHIP_ERR_INVALID after filling everything
 * else, alnOff[nreads] = the bytes needed.  alnA == NULL: no strings are wanted (alnB, alnOff are not touched).
 * Errors, in this order: a parameter out of range (seed_len, seed_stride, max_occ >= 1; 1 <= max_cand <= 64; min_score
 * >= 1) is POLYHIP_ERR_INVALID naming the field, before any device call; max_len > 4096 or band > 1024 is
 * POLYHIP_ERR_UNSUPPORTED (the per-pair alignment kernels' limits); a NULL handle, or a scoring handle created on another
 * device than the index's, is POLYHIP_ERR_INVALID.  The call runs on the index's device, as every polyhip_bwt_* call
 * does; the device list does not apply.
 * _dev: every pointer is device memory ordered on `stream`; d_off[i] are offsets into d_reads.  The call synchronises
 * `stream` (it reads back two counts per chunk).  d_work: polyhip_map_workspace_bytes(...) holds the worst case (max_occ
 * hits per seed) of every read at once, capped at 8 GiB; with less the call loops over chunks of reads (a multiple of 256
 * each; info.chunks) with the same outputs; less than one chunk of min(nreads, 256) reads needs is POLYHIP_ERR_INVALID.
 * polyhip_map_last_info: the calling thread's last call.
 */
typedef struct polyhip_map_params {
    uint32_t seed_len, seed_stride, max_occ, band, max_cand, both_strands;
    int64_t min_score;
} polyhip_map_params;
typedef struct polyhip_map_info {
    uint64_t seeds, seeds_over_max_occ, hits, clusters, pairs_aligned, reads_mapped;
    uint32_t chunks;
} polyhip_map_info;
size_t polyhip_map_workspace_bytes(const polyhip_bwt *h, const polyhip_scoring *sc,
                                   const polyhip_map_params *params, uint64_t nreads,
                                   uint32_t max_len);
int polyhip_map_reads_dev(const polyhip_bwt *h, const polyhip_scoring *sc,
                          const polyhip_map_params *params, const uint8_t *d_reads,
                          const uint64_t *d_off, uint64_t nreads, uint32_t max_len,
                          int64_t *d_score, int64_t *d_second, uint32_t *d_flags,
                          uint32_t *d_votes, uint32_t *d_ref_start, uint32_t *d_ref_end,
                          uint32_t *d_read_start, uint32_t *d_read_end, uint32_t *d_err,
                          uint8_t *d_alnA, uint8_t *d_alnB, uint64_t *d_alnOff,
                          uint64_t aln_capacity, void *d_work, size_t work_bytes,
                          polyhip_stream_t stream);
int polyhip_map_reads(const polyhip_bwt *h, const polyhip_scoring *sc,
                      const polyhip_map_params *params, const uint8_t *reads,
                      const uint64_t *off, uint64_t nreads, uint32_t max_len,
                      int64_t *score, int64_t *second, uint32_t *flags, uint32_t *votes,
                      uint32_t *ref_start, uint32_t *ref_end, uint32_t *read_start,
                      uint32_t *read_end, uint32_t *err, uint8_t *alnA, uint8_t *alnB,
                      uint64_t *alnOff, uint64_t aln_capacity);
int polyhip_map_last_info(polyhip_map_info *info);
/* ---- read mapping with affine gaps in the extension (Gotoh) ---- */
/*
 * polyhip_map_reads_affine is polyhip_map_reads with steps 5 and 6 changed as follows; steps 1-4 (strands, seeds,
 * clusters, candidates and their ranks) are unchanged, word for word.
 *  5. every kept candidate is extended with SmithWatermanAffine(q, T[lo, hi)), as polyhip_sw_affine_align_batch_packed
 *     defines it: the table is the scoring handle's, gap_open and gap_extend are as defined there, the handle's own gap is
 *     ignored; the argmax is the first maximum in row-major order; the traceback has three states (diagonal, then F, then
 *     E) and inside a gap prefers opening over extending.
 *  6. unchanged in meaning: the alphabet error of the lowest such rank; best = the highest score, ties to the lowest
 *     rank; mapped iff score >= min_score; second, flags, votes, ref_*, read_* and the strings as before.  Only the
 *     winner's strings are ever needed, so the traceback runs for each mapped read's winning candidate only: the score
 *     pass runs on all kept candidates, the winner is picked from scores, errs and ranks, then the winner is traced.
 *     ref_start / read_start come from the winner's strings, so the traceback also runs when alnA == NULL.
 * With gap_open == gap_extend == g every output equals polyhip_map_reads with a handle whose gap is g.
 * work_limit: the most device workspace, in bytes, the call may carve its per-chunk arrays from.  0 = the default, which
 * is polyhip_map_reads': the whole batch, capped at 8 GiB.  A smaller value makes the call loop over chunks of reads
 * (each a multiple of 256) with identical outputs; a value below what one chunk of min(nreads, 256) reads needs is
 * POLYHIP_ERR_INVALID, and the message says how many bytes that chunk needs.  The workspace holds every per-chunk array
 * of the call: seeds, hits, candidates, the pair batch, the score pass's band scratch, the winners' compact batch, their
 * string slots, and the direction bits of one traceback sub-chunk.  Direction bits are sized per winner from the largest
 * window (max_len rows, max_len + 3 * band columns) and at most 1 GiB of them are held at once: the winners of a chunk of
 * reads are traced in sub-chunks (POLYHIP_SWA_CHUNK_PAIRS=<n> in the environment forces the sub-chunk size, as for
 * polyhip_sw_affine_align_batch_packed: a testing aid).  A chunk of reads without a winner launches no traceback.
 * Errors, in this order: everything polyhip_map_reads checks, in its order and with its messages (NULL arguments and
 * offsets included when nreads > 0); !(gap_open <= gap_extend <= -1) is POLYHIP_ERR_UNSUPPORTED; absmax * (max_len +
 * (max_len + 3 * band)) >= 2^30 with absmax = max(|smin|, |smax|, |gap_open|) is POLYHIP_ERR_UNSUPPORTED (the int32 cell
 * range of the affine kernel at the mapper's largest window).  String capacity behaves as in polyhip_map_reads: a short
 * aln_capacity returns POLYHIP_ERR_INVALID after filling everything else, alnOff[nreads] = the bytes needed.
 * nreads == 0 is an empty, successful call.  The call runs on the index's device, on the handle's stream; the device list
 * does not apply.  There is no device-pointer flavour.
 * polyhip_map_affine_last_info: the calling thread's last polyhip_map_reads_affine.  The first six counters and chunks are
 * as polyhip_map_info; pairs_traced = candidates whose traceback ran (== reads_mapped in every call); tb_cells = cell
 * updates of the traceback windows (endA * window columns over the winners); tb_chunks = traceback launches summed over
 * the chunks of reads.
 */
typedef struct polyhip_map_affine_info {
    uint64_t seeds, seeds_over_max_occ, hits, clusters, pairs_aligned, reads_mapped;
    uint64_t pairs_traced;
    uint64_t tb_cells;
    uint32_t chunks;
    uint32_t tb_chunks;
} polyhip_map_affine_info;
int polyhip_map_reads_affine(const polyhip_bwt *h, const polyhip_scoring *sc,
                             const polyhip_map_params *params, int64_t gap_open,
                             int64_t gap_extend, const uint8_t *reads, const uint64_t *off,
                             uint64_t nreads, uint32_t max_len, uint64_t work_limit,
                             int64_t *score, int64_t *second, uint32_t *flags, uint32_t *votes,
                             uint32_t *ref_start, uint32_t *ref_end, uint32_t *read_start,
                             uint32_t *read_end, uint32_t *err, uint8_t *alnA, uint8_t *alnB,
                             uint64_t *alnOff, uint64_t aln_capacity);
int polyhip_map_affine_last_info(polyhip_map_affine_info *info);

/* ---- read mapping of paired-end reads: proper pairs, insert size, mate rescue (no counterpart in the reference) ---- */
/*
 * polyhip_map_pairs places npairs pairs of reads: mate 1 of pair i is read i of (reads1, off1), mate 2 is read i of
 * (reads2, off2), each batch packed as polyhip_map_reads' is.  Entry 2i of every per-mate output is mate 1 of pair i, entry
 * 2i + 1 is mate 2; tlen has one entry per pair; the strings are packed as in polyhip_map_reads, in that order (2 * npairs
 * + 1 offsets).  For one pair, with mates r1, r2 of m1, m2 bytes, the text T of n bytes and W = band:
 *  1. Steps 1-5 of polyhip_map_reads_affine run on each mate on its own: strands, seeds, clusters, ranks, windows [lo, hi)
 *     and the SmithWatermanAffine(q, T[lo, hi)) score pass are unchanged.  Each kept candidate has strand s, lo, score, endA,
 *     endB and err.  A mate's err is as in step 6 there: the lowest-ranked candidate's alphabet error, or 0xFFFFFFFF when
 *     the mate is longer than max_len.  A mate with err != 0 has no usable candidate, is never an anchor and is never
 *     rescued.  A candidate is usable when its mate's err is 0 and its score is at least min_score.
 *  2. Projection.  For a usable candidate of a mate of m bytes, left = lo + endB - endA (signed 64-bit: the text position
 *     q[0] reaches along the end cell's diagonal) and right = left + m.  A candidate f of one mate and a candidate r of the
 *     other are a proper combination iff f is on strand 0 and r on strand 1, left_f <= left_r, right_f <= right_r, and
 *     min_insert <= right_r - left_f <= max_insert.  right_r - left_f is the insert.  Forward-reverse orientation only:
 *     dovetails and same-strand pairs are never proper.
 *  3. Pairing.  Among all proper combinations (k1, k2), k1 a rank of mate 1 and k2 a rank of mate 2, the best has the
 *     highest score1 + score2, ties to the smallest k1, then the smallest k2.  If there is one, both mates are mapped at
 *     those candidates, flags bit 2 (proper) is set on both and tlen[i] is the insert.
 *  4. Rescue, only when step 3 found nothing and rescue != 0.  For x = 1, 2: if mate x has a usable candidate, its anchor a
 *     is its best usable candidate as step 6 picks it (highest score, lowest rank).  With y the other mate, an attempt is
 *     made when err_y == 0 and m_y >= 1.  Anchor on strand 0: the query is q_y = ReverseComplement(r_y), the window
 *     [left_a + min_insert - m_y - W, left_a + max_insert + W).  Anchor on strand 1: the query is q_y = r_y, the window
 *     [right_a - max_insert - W, right_a - min_insert + m_y + W).  The window is clipped to [0, n); an empty window means
 *     no attempt, a non-empty one counts in rescue_attempts.  The attempt is SmithWatermanAffine(q_y, T[wlo, whi)); it
 *     succeeds iff its err is 0, its score is at least min_score and, with left_y = wlo + endB - endA, the anchor and this
 *     alignment are a proper combination by step 2.  An alphabet error of an attempt is not reported.  Of the successful
 *     attempts the one with the higher score_a + score_y wins, a tie goes to the attempt anchored on mate 1.  The anchor
 *     mate is mapped at a with flags bit 2 set; the other mate is mapped at the rescued alignment with flags = mapped |
 *     strand << 1 | proper (bit 2) | rescued (bit 3), votes 0 and ref_end = wlo + endB.  tlen[i] is the insert.
 *  5. Fallback.  Otherwise each mate is placed exactly as step 6 of polyhip_map_reads_affine places a single read; bits 2
 *     and 3 are clear and tlen[i] = 0.
 *  6. In every case: second of a mate is the highest score among its kept candidates other than the chosen one (for a
 *     rescued mate that is all of its kept candidates), 0 if there are none; ref_start, read_start and the strings come
 *     from the traceback of the chosen alignment only (a candidate or a rescue window); every mapped mate is traced and no
 *     other; unmapped mates get zeros and empty strings.
 * Host pointers only: the call runs on the index's device, on the handle's stream, as polyhip_map_reads_affine does.
 * Errors, in this order: everything polyhip_map_reads_affine checks, in its order and with its messages, the int32 cell
 * range taken over the wider of the mapping window (max_len + 3 * band columns) and, with rescue != 0, the rescue window
 * (max_insert - min_insert + max_len + 2 * band columns); a NULL pair_params, both_strands == 0, min_insert > max_insert
 * or rescue > 1 is POLYHIP_ERR_INVALID naming the field; with rescue != 0 a rescue window of more than
 * POLYHIP_MAP_MAX_RESCUE_COLS = 7168 columns (the widest window a single read's candidate can have: 4096 + 3 * 1024) is
 * POLYHIP_ERR_UNSUPPORTED.  npairs == 0 is an empty, successful call.  String capacity behaves as in polyhip_map_reads.
 * work_limit has the meaning it has in polyhip_map_reads_affine; chunks are whole pairs, a multiple of 128 pairs; the
 * message of a limit that is too small names the bytes one chunk of min(npairs, 128) pairs needs; outputs are identical
 * for every chunking.  The workspace also holds the rescue batch, and the winners' slots and direction words are sized for
 * the wider of the two windows.  A chunk without a rescue request launches no rescue pass, one without a mapped mate no
 * traceback.
 * polyhip_map_pairs_last_info: the calling thread's last polyhip_map_pairs.  The first six counters are as
 * polyhip_map_info, over all 2 * npairs mates; proper_pairs = pairs whose mates carry flags bit 2 (steps 3 and 4);
 * rescue_attempts = rescue windows scored; rescued = pairs placed by step 4; pairs_traced = alignments traced (==
 * reads_mapped in every call); chunks = chunks of pairs.
 */
#define POLYHIP_MAP_MAX_RESCUE_COLS 7168u
typedef struct polyhip_map_pair_params {
    uint32_t min_insert, max_insert, rescue;
} polyhip_map_pair_params;
typedef struct polyhip_map_pairs_info {
    uint64_t seeds, seeds_over_max_occ, hits, clusters, pairs_aligned, reads_mapped;
    uint64_t proper_pairs, rescue_attempts, rescued, pairs_traced;
    uint32_t chunks;
} polyhip_map_pairs_info;
int polyhip_map_pairs(const polyhip_bwt *h, const polyhip_scoring *sc,
                      const polyhip_map_params *params,
                      const polyhip_map_pair_params *pair_params, int64_t gap_open,
                      int64_t gap_extend, const uint8_t *reads1, const uint64_t *off1,
                      const uint8_t *reads2, const uint64_t *off2, uint64_t npairs,
                      uint32_t max_len, uint64_t work_limit, int64_t *score, int64_t *second,
                      uint32_t *flags, uint32_t *votes, uint32_t *ref_start, uint32_t *ref_end,
                      uint32_t *read_start, uint32_t *read_end, uint32_t *err, int64_t *tlen,
                      uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff, uint64_t aln_capacity);
int polyhip_map_pairs_last_info(polyhip_map_pairs_info *info);

/* ---- a reference of several contigs, and read mapping onto it (no counterpart in the reference) ---- */
/*
 * A polyhip_refs is a set of k contigs T_0 .. T_{k-1} of n_c >= 1 bytes each, given as a packed batch (seqs, off[0..k]).
 * C is their concatenation without a separator (an ACGT set keeps the index's 2-bit nucleotide layout), start_c the
 * exclusive scan of the lengths (start_k = |C|).  The set owns one FM-index over C, built by polyhip_bwt_create's path,
 * and keeps start[0..k] on the index's device.
 * refs_create errors, all decided before any device work: POLYHIP_ERR_INVALID for a NULL argument, ncontigs == 0, offsets
 *   that do not ascend or an empty contig; POLYHIP_ERR_UNSUPPORTED for ncontigs > 2^24; POLYHIP_ERR_INVALID for a '$' in a
 *   contig ("Provided sequence contains the nullChar $. BWT cannot be constructed") and for |C| >= 2^32 - 1, both as
 *   polyhip_bwt_create.
 * refs_count: k (negative status for a NULL handle).  refs_starts: out[0..k] = start (k + 1 entries).
 * refs_index: the index of C.  It is BORROWED: the set owns it, it lives until polyhip_refs_destroy, and passing it to
 *   polyhip_bwt_destroy is the caller's error.  polyhip_bwt_count / locate / extract work on it as on any index; its
 *   positions are positions in C.  NULL for a NULL handle.
 * refs_resolve: entry i is the span [pos[i], pos[i] + len[i]) of C (len == NULL: 1 each), e.g. what Locate returned with
 *   the pattern's length.  One lane per entry finds by binary search over start[] the contig c with start_c <= pos <
 *   start_{c+1}: rid[i] = c, local[i] = pos - start_c, err[i] = 0; err[i] = 2 when the span runs past the contig's end
 *   (pos + len > start_{c+1}; rid and local are still those of pos); err[i] = 1 with rid = local = 0 when pos >= |C|.
 *   n == 0 is an empty, successful call.  Host pointers; runs on the index's device and stream, as polyhip_bwt_count; the
 *   device list does not apply.
 *
 * polyhip_map_reads_refs is polyhip_map_reads_affine, and polyhip_map_pairs_refs is polyhip_map_pairs, on a set instead of
 * one text: the first argument is the set, and there is one more per-entry output, rid, before ref_start.  (With gap_open
 * == gap_extend the single-read call is polyhip_map_reads with that linear gap.)  The definition is the single-text one
 * with the changes below; everything not named here is unchanged, word for word.
 *  2. seeds.  A seed's occurrences are the p with C[p, p + L) = q[o, o + L).  max_occ is judged on that count (occurrences
 *     that straddle a boundary count towards it: it is a cost guard, and the count is known before anything is located);
 *     a max_occ above |C| means no limit.  Of a seed that passes, an occurrence is a hit only if it lies wholly inside one
 *     contig: start_c <= p and p + L <= start_c + n_c.  The hit is in contig c on the local diagonal d = p - start_c - o.
 *     Straddling occurrences are dropped and counted (polyhip_map_refs_info.straddling).
 *  3. clusters are formed per (strand, contig) on local diagonals: hits of different contigs never share a cluster.
 *  4. candidates are ordered by (votes descending, s ascending, contig ascending, d0 ascending).
 *  5. windows: lo = max(0, d0 - W), hi = min(n_c, dmax + m + W); the extension sees T_c[lo, hi) only.
 *  6. rid = the chosen candidate's contig; ref_start and ref_end are positions in T_rid; an unmapped entry has rid = 0 with
 *     its other zeros.
 *  pairs, step 2: a proper combination also needs both candidates on the same contig; left and right are local.
 *  pairs, step 4: a rescue window is clipped to [0, n_c) of the anchor's contig, and the rescued mate takes the anchor's rid.
 * Parameter checks, their order and messages, POLYHIP_MAP_MAX_RESCUE_COLS, work_limit, chunking (multiples of 256 reads or
 * 128 pairs, identical outputs for every chunking) and the string-capacity protocol are those of the single-text calls,
 * with "null index handle" said of a NULL set.  A sort key holds (read of the chunk, strand, contig, local diagonal): a
 * chunk is also limited to the reads whose keys fit 64 bits, and a set for which that is fewer than 256 reads (about
 * log2(k) + log2(longest contig + max_len + band) > 54) is POLYHIP_ERR_UNSUPPORTED.
 * The calls fill the calling thread's polyhip_map_affine_last_info / polyhip_map_pairs_last_info as their single-text
 * siblings do (hits = the hits kept), and polyhip_map_refs_last_info: contigs = k, straddling = occurrences dropped in
 * step 2, over both strands and all chunks.
 */
typedef struct polyhip_refs polyhip_refs;
typedef struct polyhip_map_refs_info {
    uint64_t contigs, straddling;
} polyhip_map_refs_info;
int polyhip_refs_create(const uint8_t *seqs, const uint64_t *off, uint64_t ncontigs,
                        polyhip_refs **out);
int polyhip_refs_destroy(polyhip_refs *h);
int64_t polyhip_refs_count(const polyhip_refs *h);
int polyhip_refs_starts(const polyhip_refs *h, uint64_t *out);
const polyhip_bwt *polyhip_refs_index(const polyhip_refs *h);
int polyhip_refs_resolve(const polyhip_refs *h, const uint32_t *pos, const uint32_t *len,
                         uint64_t n, uint32_t *rid, uint32_t *local, uint32_t *err);
int polyhip_map_reads_refs(const polyhip_refs *h, const polyhip_scoring *sc,
                           const polyhip_map_params *params, int64_t gap_open,
                           int64_t gap_extend, const uint8_t *reads, const uint64_t *off,
                           uint64_t nreads, uint32_t max_len, uint64_t work_limit,
                           int64_t *score, int64_t *second, uint32_t *flags, uint32_t *votes,
                           uint32_t *rid, uint32_t *ref_start, uint32_t *ref_end,
                           uint32_t *read_start, uint32_t *read_end, uint32_t *err,
                           uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff, uint64_t aln_capacity);
int polyhip_map_pairs_refs(const polyhip_refs *h, const polyhip_scoring *sc,
                           const polyhip_map_params *params,
                           const polyhip_map_pair_params *pair_params, int64_t gap_open,
                           int64_t gap_extend, const uint8_t *reads1, const uint64_t *off1,
                           const uint8_t *reads2, const uint64_t *off2, uint64_t npairs,
                           uint32_t max_len, uint64_t work_limit, int64_t *score, int64_t *second,
                           uint32_t *flags, uint32_t *votes, uint32_t *rid, uint32_t *ref_start,
                           uint32_t *ref_end, uint32_t *read_start, uint32_t *read_end,
                           uint32_t *err, int64_t *tlen, uint8_t *alnA, uint8_t *alnB,
                           uint64_t *alnOff, uint64_t aln_capacity);
int polyhip_map_refs_last_info(polyhip_map_refs_info *info);

/* ---- the mapper's output as alignment records: CIGAR, NM, MD, MAPQ, SAM FLAG (no counterpart in the reference) ---- */
/*
 * polyhip_aln_records turns what polyhip_map_reads, polyhip_map_reads_affine or polyhip_map_pairs returned for n entries
 * (reads, or mates in the order 2i, 2i + 1) into the fields of a SAM record.  It is a pass over those arrays: it places
 * nothing and needs no index.  read_len[i] is the length of read i, which the mapper's caller holds.  For entry i the
 * columns are c in [alnOff[i], alnOff[i + 1]) with a = alnA[c] (the oriented read q) and b = alnB[c] (the text window).
 *  Column class: a == '-' and b == '-' is invalid; a == '-' only is D (deletion from the text); b == '-' only is I
 *   (insertion); a == b is '='; anything else is X.  Bytes are compared raw, no case is folded.
 *  err[i], the first that applies, for entries with flags bit 0 (mapped) only; an unmapped entry gets 0 and its strings are
 *   never read:  4 = more than POLYHIP_ALN_MAX_COLUMNS = 2^28 - 1 columns (a BAM CIGAR length has 28 bits); this one is
 *   decided from the offsets alone, before any column is read, so such an entry is 4 whatever its columns hold;  1 = an
 *   invalid column;  2 = read_start > read_end, or read_end > read_len, or the number of columns with a != '-' differs from
 *   read_end - read_start;  3 = no columns.
 *  Live: flags bit 0 is set and err[i] == 0.  An entry that is not live gets no CIGAR entries, no MD bytes (zero bytes, not
 *   "0"), nm = 0 and mapq = 0.
 *  CIGAR, as BAM stores it: uint32 len << 4 | op with M = 0, I = 1, D = 2, S = 4, '=' = 7, X = 8.  First (read_start, S) if
 *   read_start > 0; then one entry per maximal run of columns of one class, where with eqx == 0 the classes '=' and X are
 *   one class M; last (read_len - read_end, S) if that is positive.  Coordinates are those of q, as the mapper reports them:
 *   SAM's convention for a record on the reverse strand.  A clip keeps the low 28 bits of its length.
 *  nm = the number of X, I and D columns.
 *  MD, in samtools' form: with a counter k = 0 over the columns in order, an I column is skipped; '=' adds one to k; X
 *   writes k in decimal and the byte b, then k = 0; the first column of a maximal run of D columns (maximal among all
 *   columns, so an I column between two D columns separates two runs) writes k, '^' and b, then k = 0, and every further
 *   column of the run writes its b; the end writes k.  Adjacent mismatches give ..A0C.., a deletion followed at once by a
 *   mismatch ^AC0T, the columns D I D ^A0^C.  The MD of a live entry is never empty.
 *  mapq: with s = score and t = max(second, 0): 0 if t >= s, else min(60, floor(60 * (s - t) / s)) in signed 64-bit integers
 *   (s below 2^57).  This is a stated convention, not a calibrated quality: nobody has measured how its values relate to
 *   the probability that a placement is wrong.
 *  sam_flag: 0x4 if the entry is not live; 0x10 if it is live and flags bit 1 (reverse) is set.  With paired != 0 the mate
 *   of entry i is entry i ^ 1 and further: 0x1 always; 0x2 if flags bit 2 (proper) is set and both mates are live; 0x8 if
 *   the mate is not live; 0x20 if the mate is live and its flags bit 1 is set; 0x40 for even i, 0x80 for odd i.
 * Packing and capacity are polyhip_bwt_locate's: cigar_off[0..n] and md_off[0..n] are the exclusive scans of the entries'
 * CIGAR entries and MD bytes and are always filled, as are nm, mapq, sam_flag and err; entry i's CIGAR is cigar[cigar_off[i]
 * .. cigar_off[i + 1]), its MD md[md_off[i] .. md_off[i + 1]) (no terminator).  If cigar_off[n] > cigar_capacity or md_off[n]
 * > md_capacity nothing is written to cigar or md and the call fails with POLYHIP_ERR_INVALID naming both sizes needed;
 * cigar == NULL or md == NULL with a capacity of 0 asks for the sizes only.  No device buffer for either is allocated
 * before that check.
 * Errors, in this order, all POLYHIP_ERR_INVALID: a NULL params; eqx > 1 or paired > 1, naming the field; paired != 0 with
 * an odd n; with n > 0 a NULL array (alnA and alnB may be NULL when alnOff[n] == alnOff[0]; cigar, md as above); alnOff
 * not ascending.  n == 0 is an empty, successful call: cigar_off[0] = md_off[0] = 0 where those are not NULL.
 * Host pointers only, no stream: the call copies the arrays in, runs on the calling thread's current device and copies
 * the records out; nothing that depends on n is allocated before the checks above; the device list does not apply.
 * polyhip_aln_records_last_info: the calling thread's last call: entries = n; mapped = live entries; columns = the columns
 * of the live entries; cigar_ops = cigar_off[n]; md_bytes = md_off[n]; bad = entries with err != 0.
 */
#define POLYHIP_ALN_MAX_COLUMNS 0x0FFFFFFFu
typedef struct polyhip_aln_records_params {
    uint32_t eqx, paired;
} polyhip_aln_records_params;
typedef struct polyhip_aln_records_info {
    uint64_t entries, mapped, columns, cigar_ops, md_bytes, bad;
} polyhip_aln_records_info;
int polyhip_aln_records(const polyhip_aln_records_params *params, uint64_t n,
                        const uint32_t *flags, const int64_t *score, const int64_t *second,
                        const uint32_t *read_start, const uint32_t *read_end,
                        const uint32_t *read_len, const uint8_t *alnA, const uint8_t *alnB,
                        const uint64_t *alnOff, uint64_t *cigar_off, uint32_t *cigar,
                        uint64_t cigar_capacity, uint64_t *md_off, uint8_t *md,
                        uint64_t md_capacity, uint32_t *nm, uint8_t *mapq, uint32_t *sam_flag,
                        uint32_t *err);
int polyhip_aln_records_last_info(polyhip_aln_records_info *info);

/* ---- pileup of the mapper's output: per-position counts, consensus, variant sites; polyhip_pileup_rows: the text rows ---- */
/*
 * polyhip_pileup asks what the n entries that polyhip_map_reads, polyhip_map_reads_affine or polyhip_map_pairs returned say
 * about each position of the text region [region_lo, region_hi), L = region_hi - region_lo.  It is a pass over those
 * arrays, the mapq of polyhip_aln_records (optional) and the text ref[0, ref_len) itself: it places nothing and needs no
 * index.  For entry i the columns are c in [alnOff[i], alnOff[i + 1]) with a = alnA[c] (the oriented read, so already in the
 * text's orientation) and b = alnB[c] (the text byte).  Column classes are those of polyhip_aln_records: a == '-' and
 * b == '-' is invalid, a == '-' only is D, b == '-' only is I, everything else is a base column; bytes are compared raw.
 * The text position of a column with b != '-' is ref_start[i] plus the number of earlier columns of the entry with
 * b != '-'.  The strand is s = flags bit 1.
 *  Skipped: an entry with flags bit 0 (mapped) and mapq[i] < min_mapq; min_mapq == 0 skips nothing and never reads mapq.
 *  err[i], the first that applies, for mapped entries that are not skipped; every other entry gets 0 and its strings are
 *   never read:  4 = more than POLYHIP_ALN_MAX_COLUMNS columns, decided from the offsets alone;  1 = an invalid column;
 *   2 = ref_start plus the number of columns with b != '-' differs from ref_end, or ref_end > ref_len;  3 = no columns;
 *   5 = some column has b != '-' and b != ref[its position].
 *  Used: mapped, not skipped, err[i] == 0.  Only used entries add to the counts: the whole entry is judged before any of
 *   its adds.
 *  counts, channel-major, 16 planes of L uint32: counts[ch * L + (p - region_lo)] with ch = 8 * s + k.  k = 0..3: a is A/a,
 *   C/c, G/g, T/t at a base column at p;  k = 4: any other a at a base column;  k = 5: a D column at p;  k = 6: an insertion
 *   event anchored at p, one per maximal run of I columns (maximal among all columns of the entry), anchored at the position
 *   of the last column with b != '-' before the run, ref_start - 1 if there is none;  k = 7: a deletion event anchored at
 *   p, one per maximal run of D columns, anchored the same way, so the deleted bases are p + 1 onward.  An event anchored
 *   at -1 is dropped and counted in info.edge_events (whatever the region); a position or anchor outside the region is
 *   dropped silently.  counts is zeroed by the call.  All sums are integers, so the result does not depend on the order
 *   of the adds.
 *  consensus[p - region_lo]: with depth = the sum of k = 0..5 over both strands, 'N' if depth < max(min_depth, 1), else
 *   "ACGTN*"[k] for the k in 0..5 with the highest two-strand count, ties to the lowest k.
 *  sites, ascending p and within a position SNV to A, C, G, T, then INS, then DEL; only positions with depth >=
 *   max(min_depth, 1) have any.  A count passes when count >= max(min_alt_count, 1) and count * 1000 >= min_alt_permille *
 *   depth (in uint64).  SNV (kind 1): k in 0..3 that differs from the class of ref[p] (same table, "other" is class 4) and
 *   whose two-strand count passes; alt is the upper-case base.  INS (kind 2): the count of channel 6 passes; alt = 0.  DEL
 *   (kind 3): the count of channel 7 passes; alt = 0.  pos = p, depth as above, count the two-strand count, count_fwd its
 *   strand-0 share, ref the raw ref[p], pad = 0.
 * Capacity is polyhip_bwt_locate's: *nsites is always filled; if it exceeds site_capacity nothing is written to sites and the
 * call fails with POLYHIP_ERR_INVALID naming the size needed, after counts, consensus and err have been filled; sites ==
 * NULL with a capacity of 0 asks for the size only.  No device buffer for the sites is allocated before that check.
 * Errors, in this order: a NULL params (POLYHIP_ERR_INVALID); region_lo > region_hi, region_hi > ref_len or
 * min_alt_permille > 1000 (_INVALID, naming the field); n >= 2^32 (POLYHIP_ERR_UNSUPPORTED: the counts are uint32 and an
 * entry adds at most one to a cell); min_mapq > 0 with mapq == NULL (_INVALID); a NULL array that is needed (_INVALID: ref
 * and nsites always; with n > 0 flags, ref_start, ref_end, alnOff and err; alnA and alnB may be NULL when alnOff[n] ==
 * alnOff[0]; counts and consensus may be NULL only when L == 0; sites as above); alnOff not ascending (_INVALID).  n == 0
 * and L == 0 are successful calls; with L == 0 the only outputs are err and *nsites = 0.
 * Host pointers only, no stream: the call copies the arrays in, runs on the calling thread's current device and copies the
 * results out; nothing that depends on n or on the region is allocated before the checks above; the device list does not
 * apply.  One text only; base qualities (polyhip_pileup_qual below takes them) and the inserted bytes themselves are not
 * looked at.
 * polyhip_pileup_last_info: the calling thread's last call: entries = n; used = used entries; skipped_mapq = entries
 * skipped by min_mapq; bad = entries with err != 0; columns = the columns of the used entries; edge_events = events dropped
 * for anchor -1; sites = *nsites.
 */
#define POLYHIP_PILEUP_CHANNELS 16u
typedef struct polyhip_pileup_params {
    uint64_t region_lo, region_hi; /* text positions [lo, hi); L = hi - lo */
    uint32_t min_mapq;             /* entries with mapq[i] < min_mapq are skipped; > 0 needs mapq != NULL */
    uint32_t min_depth;            /* consensus and sites need depth >= max(min_depth, 1) */
    uint32_t min_alt_count;        /* a site needs count >= max(min_alt_count, 1) ... */
    uint32_t min_alt_permille;     /* ... and count * 1000 >= min_alt_permille * depth (uint64); 0..1000 */
} polyhip_pileup_params;
typedef struct polyhip_pileup_site {
    uint32_t pos, depth, count, count_fwd;
    uint8_t kind, ref, alt, pad;
} polyhip_pileup_site;
typedef struct polyhip_pileup_info {
    uint64_t entries, used, skipped_mapq, bad, columns, edge_events, sites;
} polyhip_pileup_info;
int polyhip_pileup(const polyhip_pileup_params *params, uint64_t n, const uint32_t *flags,
                   const uint8_t *mapq, const uint32_t *ref_start, const uint32_t *ref_end,
                   const uint8_t *alnA, const uint8_t *alnB, const uint64_t *alnOff,
                   const uint8_t *ref, uint64_t ref_len, uint32_t *counts, uint8_t *consensus,
                   uint64_t *nsites, polyhip_pileup_site *sites, uint64_t site_capacity,
                   uint32_t *err);
int polyhip_pileup_last_info(polyhip_pileup_info *info);

/*
 * polyhip_pileup_qual is polyhip_pileup with the base qualities of the reads: a minimum base quality and, per base and
 * strand, the sum of the counted qualities.  Everything not named here is polyhip_pileup's definition, unchanged.
 *  Qualities: entry i's quality string is qual[qualOff[i] .. qualOff[i + 1]), of length m_i; n + 1 offsets.  It is in the
 *   orientation of the read as sequenced (the FASTQ's), NOT in that of the oriented read q.  With polyhip_fastq_pack_qual
 *   and result[5] == 0 these are quals and qual_offsets themselves; for polyhip_map_pairs the caller interleaves the mates'
 *   strings in entry order 2i, 2i + 1.
 *  Quality of a column: a column c of entry i with a != '-' has the index x = read_start[i] + (earlier columns of the entry
 *   with a != '-') in q; its index in the read as sequenced is y = x on the forward strand and y = m_i - 1 - x when flags
 *   bit 1 is set;  Q = qual[qualOff[i] + y] - qual_offset.
 *  err[i], the first that applies, in this order: 4, 1, 2, 3, 5 as in polyhip_pileup;  6 = read_start[i] plus the number
 *   of columns with a != '-' exceeds m_i;  7 = some byte of the entry's WHOLE quality string, clipped parts included, is
 *   below qual_offset or above qual_offset + 93.  The whole entry is judged before any of its adds.
 *  counts, the same 16 planes: a base column (k = 0..4) is counted only if Q >= min_base_qual.  D columns (k = 5) and the
 *   events (k = 6, 7) are NOT filtered: a deleted base has no quality of its own and this call does not lend it a
 *   neighbour's; an event is counted whatever the qualities of the inserted bases.
 *  qsum, 8 planes of L uint32: qsum[(4 * s + k) * L + (p - region_lo)], k = 0..3 = the sum of Q over the counted base
 *   columns of that base and strand at p (at most 93 per entry: hence the bound on n below).  Zeroed by the call; may be
 *   NULL only when L == 0.
 *  consensus and sites: the unchanged rules applied to the filtered counts.
 *  info: filtered_bases = the base columns of used entries with Q < min_base_qual, whatever the region (as edge_events is
 *   counted); the other fields as in polyhip_pileup_info.
 * Errors, in this order: what polyhip_pileup checks on params->base, in its order (NULL params, region_lo, region_hi,
 * min_alt_permille);  min_base_qual > 93 or qual_offset > 162 (_INVALID, naming the field);  n * 93 >= 2^32
 * (POLYHIP_ERR_UNSUPPORTED: qsum is uint32; before any array is read, it takes the place of the n >= 2^32 check);
 * min_mapq > 0 with mapq == NULL;  the NULL-array checks, where with n > 0 read_start and qualOff are needed too, qual may be
 * NULL when qualOff[n] == qualOff[0] and qsum goes with counts;  alnOff or qualOff not ascending (_INVALID).
 * Capacity behaviour, n == 0, L == 0, host pointers only and "nothing that depends on n or the region is allocated before
 * the checks" are polyhip_pileup's.  Only [qualOff[0], qualOff[n]) of qual is copied in.
 * Identity: with min_base_qual == 0 and quality strings that raise neither 6 nor 7, counts, consensus, sites, err and the
 * shared info fields equal polyhip_pileup's on the same arrays.
 */
#define POLYHIP_PILEUP_QSUM_PLANES 8u
typedef struct polyhip_pileup_qual_params {
    polyhip_pileup_params base;
    uint32_t min_base_qual;   /* 0..93; a base column with Q < min_base_qual is not counted */
    uint32_t qual_offset;     /* Phred offset of the quality bytes, 33 for FASTQ; qual_offset + 93 <= 255 */
} polyhip_pileup_qual_params;
typedef struct polyhip_pileup_qual_info {
    uint64_t entries, used, skipped_mapq, bad, columns, edge_events, sites;   /* as polyhip_pileup_info */
    uint64_t filtered_bases;
} polyhip_pileup_qual_info;
int polyhip_pileup_qual(const polyhip_pileup_qual_params *params, uint64_t n, const uint32_t *flags,
                        const uint8_t *mapq, const uint32_t *ref_start, const uint32_t *ref_end,
                        const uint32_t *read_start, const uint8_t *alnA, const uint8_t *alnB,
                        const uint64_t *alnOff, const uint8_t *qual, const uint64_t *qualOff,
                        const uint8_t *ref, uint64_t ref_len, uint32_t *counts, uint32_t *qsum,
                        uint8_t *consensus, uint64_t *nsites, polyhip_pileup_site *sites,
                        uint64_t site_capacity, uint32_t *err);
int polyhip_pileup_qual_last_info(polyhip_pileup_qual_info *info);

/*
 * polyhip_pileup_rows writes what the same entries say about each position of [region_lo, region_hi) as the text rows of the
 * six-column pileup format: one row per position, one token and one quality byte per read that covers it, the inserted and
 * deleted bytes spelled out.  It takes the arrays of polyhip_pileup_qual plus the order of the reads and the sequence name.
 *  Column classes, text positions, the strand, skipped entries, err values 4, 1, 2, 3, 5 and "used" are polyhip_pileup's, word
 *   for word.  With qual != NULL, err values 6 and 7 and the quality index of a column (x, y, Q) are polyhip_pileup_qual's;
 *   with qual == NULL neither applies and qualOff and read_start are not read.  Only used entries contribute: the whole
 *   entry is judged before anything of it is emitted.
 *  order: order[r] is the entry at rank r, as polyhip_coord_order returns it, a permutation of 0..n-1; NULL is entry order,
 *   order[r] = r.
 *  Tokens: a used entry has one token at every column with b != '-' whose position p lies in the region; the tokens at one
 *   position ascend by rank r.  With s the strand, fold upper-casing ASCII letters, cls the base class table of the counts
 *   and letter(x) = "ACGTN"[cls(x)], or "acgtn"[cls(x)] when s is set, a token is made of these parts, in this order:
 *    1. '^' and the byte min(mapq[i], 93) + 33, if this is the entry's first column with b != '-' (a NULL mapq reads as 255, so
 *       the byte is '~');
 *    2. one byte for the column: a base column gives '.' (',' when s is set) if fold(a) == fold(b), else letter(a); a D column
 *       gives '*';
 *    3. for every maximal run of I or of D columns whose anchor is this column, in column order: an I run gives '+', the run
 *       length in decimal and letter(alnA[c]) for each of its columns; a D run gives '-', the run length in decimal and
 *       letter(alnB[c]) for each of its columns.  The anchor is that of count channels 6 and 7: the last column with b != '-'
 *       before the run.  So an I run and the D run behind it share one token (".+2AC-1G"), and a run behind a D column hangs
 *       on a '*' ("*+1T");
 *    4. '$', if this is the entry's last column with b != '-'.
 *   A run with no column with b != '-' before it, that is a run that opens the entry, has no token to hang on: it is dropped
 *   and counted in info.dropped_events, whatever the region (the D columns of such a run still have their '*' tokens).  A
 *   token outside the region is dropped with the runs it carries.
 *  Quality byte of a token: a base column gives Q + 33; a D column gives the Q of the read base at index min(x, the index of
 *   the entry's last aligned read base), that is the next read base or, when none follows, the last one, plus 33; an entry
 *   without any read base gives '!'.  With qual == NULL every token gives '~'.  The output is offset 33 whatever qual_offset
 *   the input has.
 *  Row of position p with d tokens:  name \t (p - pos_origin + 1) \t R \t d \t the tokens \t their quality bytes \n,  tokens and
 *   quality bytes in the same order, R = ref[p] if it is in 0x21..0x7e and 'N' otherwise, both numbers in decimal.  With
 *   all_positions == 0 rows with d == 0 are not written; with all_positions == 1 they read  name \t pos \t R \t 0 \t * \t * \n.
 *   Rows ascend by p.  pos_origin <= region_lo lets a contig of a polyhip_refs set print its own positions.
 *  There is no minimum base quality here: a row shows every read and d equals the depth of polyhip_pileup (the sum of its
 *   channels 0..5 over both strands) on the same arrays and min_mapq.  Filtering by base quality stays with
 *   polyhip_pileup_qual.
 *  Outputs: *ntext = the bytes of all rows, always filled.  row_off (optional, L + 1 values): the row of position p is
 *   text[row_off[p - region_lo] .. row_off[p - region_lo + 1]), empty where no row is written.  err[n] as above.  Capacity is
 *   that of the sites of polyhip_pileup: if *ntext exceeds text_capacity nothing is written to text and the call fails with
 *   POLYHIP_ERR_INVALID naming the size needed, after err, row_off and *ntext have been filled; text == NULL with a capacity
 *   of 0 asks for the size only.  No device buffer for the text is allocated before that check.  The bytes are the same
 *   from run to run: no atomic decides where a byte goes or which read comes first.
 * Errors, in this order: what polyhip_pileup checks on the region fields, in its order (NULL params, region_lo, region_hi);
 * pos_origin > region_lo, all_positions > 1, qual_offset > 162 (_INVALID, naming the field);  name == NULL, name_len == 0 or a
 * name byte outside 0x21..0x7e (_INVALID);  n >= 2^32 (POLYHIP_ERR_UNSUPPORTED: order is uint32);  min_mapq > 0 with mapq ==
 * NULL;  a NULL array that is needed (_INVALID: ref and ntext always, text unless text_capacity == 0; with n > 0 flags,
 * ref_start, ref_end, alnOff and err, with qual != NULL also read_start and qualOff; alnA and alnB may be NULL when alnOff[n]
 * == alnOff[0]; mapq, qual, order and row_off may be NULL);  alnOff or, with qual != NULL, qualOff not ascending (_INVALID);
 * order not a permutation of 0..n-1 (_INVALID, naming order: checked on the device before anything is written);  more than
 * 2^32 - 1 tokens (_UNSUPPORTED: the caller splits the region; err has been filled).  n == 0 and L == 0 are successful
 * calls.  Host pointers only, no stream, and nothing that depends on n or on the region is allocated before the argument
 * checks, as polyhip_pileup.
 * polyhip_pileup_rows_last_info: the calling thread's last call: entries, used, skipped_mapq, bad, columns as
 * polyhip_pileup_info; tokens = the tokens of all rows; rows = the rows written; text_bytes = *ntext; dropped_events as
 * above; max_row_bytes = the longest row, newline included (the reference's parser refuses a line above 65536 bytes).
 */
typedef struct polyhip_pileup_rows_params {
    uint64_t region_lo, region_hi; /* text positions [lo, hi); L = hi - lo */
    uint64_t pos_origin;           /* column 2 prints p - pos_origin + 1; pos_origin <= region_lo */
    uint32_t min_mapq;             /* entries with mapq[i] < min_mapq are skipped; > 0 needs mapq != NULL */
    uint32_t qual_offset;          /* Phred offset of the input quality bytes, 33 for FASTQ; <= 162 */
    uint32_t all_positions;        /* 0: only rows with a token; 1: every position of the region */
    uint32_t pad;
} polyhip_pileup_rows_params;
typedef struct polyhip_pileup_rows_info {
    uint64_t entries, used, skipped_mapq, bad, columns, tokens, rows, text_bytes, dropped_events, max_row_bytes;
} polyhip_pileup_rows_info;
int polyhip_pileup_rows(const polyhip_pileup_rows_params *params, uint64_t n, const uint32_t *flags,
                        const uint8_t *mapq, const uint32_t *ref_start, const uint32_t *ref_end,
                        const uint32_t *read_start, const uint8_t *alnA, const uint8_t *alnB,
                        const uint64_t *alnOff, const uint8_t *qual, const uint64_t *qualOff,
                        const uint8_t *ref, uint64_t ref_len, const uint32_t *order,
                        const uint8_t *name, uint64_t name_len, uint64_t *ntext, uint8_t *text,
                        uint64_t text_capacity, uint64_t *row_off, uint32_t *err);
int polyhip_pileup_rows_last_info(polyhip_pileup_rows_info *info);

/* ---- variant calls from the mapped reads: alleles, left-aligned indels, the records of a VCF (no counterpart in the reference) ---- */
/*
 * polyhip_call_variants groups what the same entries say into alleles -- position, kind, length, bytes -- and returns one
 * record per allele that passes the pileup's thresholds: what polyhip_pileup_qual's sites leave open (what was inserted, how
 * many bases are gone, two insertions behind one position, one indel written at several columns of a repeat).  Where this
 * comment is silent, polyhip_pileup_qual's definition holds unchanged.
 *  Inputs: the arrays of polyhip_pileup_qual, in its order; in place of its outputs stand the outputs below.  qual may be
 *   NULL: qualOff and read_start are then not read, min_base_qual must be 0, every base counts with Q = 0, err 6 and 7 do
 *   not apply and every qsum field is 0 (the walk is polyhip_pileup's).  A non-NULL qual means qualities, empty or not.
 *  params: base as polyhip_pileup_qual_params;  left_align: 0 or not 0;  hom_permille: 0..1000;  max_indel: 1..
 *   POLYHIP_VAR_MAX_INDEL, 0 means POLYHIP_VAR_MAX_INDEL;  pad must be 0.
 *  Entries: err values 1..7, "used", skipped entries and the depth are exactly the pileup's: the call computes the 16 count
 *   planes (and with qualities the 8 qsum planes) on the device, filtered by min_base_qual, and does not return them.  The
 *   depth at p is the sum of the filtered planes k = 0..5 over both strands.
 *  fold(x) is x - 32 for 'a'..'z', else x.  All byte comparisons below are on folded bytes and the allele bytes that come out
 *   are folded.
 *  Events are those of the pileup's channels 6 and 7, of used entries only: a maximal run of I columns (kind 2) or of D
 *   columns (kind 3) that starts at column c0 of its entry (counted from the entry's first column) and is l columns long,
 *   anchored at p0 = the position of the last column with b != '-' before it, ref_start - 1 if there is none.  An event is
 *   judged in this order, the first that applies:
 *    1. l > max_indel: dropped, counted in info.long_events.
 *    2. left alignment, with left_align != 0.  x is the entry's a string for an insertion, its b string for a deletion.
 *       Step t = 0, 1, ... succeeds when column c0 - 1 - t exists in the entry, is a match column (a != '-', b != '-' and
 *       fold(a) == fold(b)) and fold(x[c0 - 1 - t]) == fold(x[c0 + l - 1 - t]).  k = the number of consecutive steps that
 *       succeed from t = 0 (the crossed columns are base columns, so both strings are contiguous there).  If k == c0 -- the
 *       walk reached the entry's first column, or c0 == 0 -- the read does not show where the repeat begins: the event is
 *       dropped and counted in info.open_events.  Else the anchor becomes p0 - k, kind and length stay, and an insertion's
 *       allele is fold(a[c0 - k .. c0 - k + l)).  With left_align == 0: k = 0, nothing is open, an insertion's allele is
 *       fold(a[c0 .. c0 + l)).
 *    3. an anchor of -1: dropped, counted in info.edge_events.
 *    4. everything else is kept and counted in info.events (and in info.shifted_events when k > 0), whatever the region;
 *       a kept event whose anchor is outside the region is then dropped silently.
 *  Alleles: two kept events of the region are the same allele when anchor and kind are equal and, for a deletion, the length,
 *   for an insertion the length and all allele bytes.  count = its events, count_fwd = those of strand 0.
 *   site_events(p, kind) = the sum of count over all alleles of that kind at p, before any threshold.
 *  Records (polyhip_variant), ascending pos; within a position SNV to A, C, G, T, then the insertion alleles by (length, then
 *   bytes as unsigned, lexicographic), then the deletion alleles by length.  Only positions with depth >= max(min_depth, 1)
 *   have records.  An allele passes by the pileup's rule on its own count: count >= max(min_alt_count, 1) and count * 1000
 *   >= min_alt_permille * depth (uint64).
 *    SNV (kind 1): exactly polyhip_pileup_qual's SNV sites (pos, depth, count, count_fwd, ref, alt); ref_count = the two-strand
 *     count of the class of ref[p], 0 for class "other"; qsum = the two-strand qsum of the alt base; allele_len = 1,
 *     allele_off = 0.
 *    INS (kind 2): alt = 0, ref = ref[p] raw, allele_len = l, allele_off = where the l folded bytes stand in `alleles`: the pool
 *     holds the bytes of the passing insertions back to back in record order and nothing else.  qsum = 0;  ref_count = depth
 *     - min(depth, site_events(p, 2)).
 *    DEL (kind 3): alt = 0, ref = ref[p] raw, allele_len = l: the deleted text is ref[p + 1 .. p + l].  allele_off = 0, qsum = 0,
 *     ref_count = depth - min(depth, site_events(p, 3)).
 *    gt = 2 when count * 1000 >= hom_permille * depth (uint64), else 1.
 *  Capacity: *nvariants and *nallele_bytes are always filled.  If *nvariants exceeds variant_capacity or *nallele_bytes
 *   exceeds allele_capacity nothing is written to either output and the call fails with POLYHIP_ERR_INVALID naming the first
 *   of the two that is short and the size needed ("the variants need ...", "the alleles need ..."), after err has been filled.
 *   NULL with a capacity of 0 asks for the size only.  No output-sized device buffer is allocated before that check.
 *  The records and the pool are the same from run to run: grouping is an exact stable sort by (pos, kind, length) and the
 *   allele bytes, no hash; no atomic decides where a record or a byte goes; every sum is of integers.
 * Errors, in this order: polyhip_pileup_qual's checks on params, in its order (NULL params, region_lo, region_hi,
 * min_alt_permille, min_base_qual, qual_offset);  hom_permille > 1000, max_indel > POLYHIP_VAR_MAX_INDEL, pad != 0 (_INVALID,
 * naming the field);  qual == NULL with min_base_qual > 0 (_INVALID);  with qualities n * 93 >= 2^32, without n >= 2^32
 * (POLYHIP_ERR_UNSUPPORTED);  min_mapq > 0 with mapq == NULL;  a NULL array that is needed (_INVALID: ref, nvariants and
 * nallele_bytes always, variants and alleles unless their capacity is 0; with n > 0 flags, ref_start, ref_end, alnOff and err,
 * with qual != NULL also read_start and qualOff; alnA and alnB may be NULL when alnOff[n] == alnOff[0]);  alnOff or, with qual
 * != NULL, qualOff not ascending (_INVALID);  more than 2^32 - 1 kept events in the region (_UNSUPPORTED: the caller splits
 * the region; err has been filled).  n == 0 and L == 0 are successful calls.  Host pointers only, no stream; nothing that
 * depends on n or on the region is allocated before the argument checks.
 * polyhip_call_variants_last_info: the calling thread's last call: entries, used, skipped_mapq, bad, columns as
 * polyhip_pileup_info; edge_events as above; sites = *nvariants; filtered_bases as polyhip_pileup_qual_info (0 without
 * qualities); events, long_events, open_events, shifted_events as above; alleles = the distinct alleles in the region before
 * the thresholds; allele_bytes = *nallele_bytes.
 */
#define POLYHIP_VAR_MAX_INDEL 255u
typedef struct polyhip_variants_params {
    polyhip_pileup_qual_params base;
    uint32_t left_align;      /* not 0: indels are moved to the leftmost column their read allows */
    uint32_t hom_permille;    /* gt = 2 when count * 1000 >= hom_permille * depth; 0..1000 */
    uint32_t max_indel;       /* longer runs are dropped; 1..POLYHIP_VAR_MAX_INDEL, 0 means POLYHIP_VAR_MAX_INDEL */
    uint32_t pad;             /* 0 */
} polyhip_variants_params;
typedef struct polyhip_variant {
    uint64_t allele_off;
    uint32_t pos, depth, count, count_fwd, ref_count, qsum, allele_len;
    uint8_t kind, ref, alt, gt;
} polyhip_variant;
typedef struct polyhip_variants_info {
    uint64_t entries, used, skipped_mapq, bad, columns, edge_events, sites;   /* as polyhip_pileup_info */
    uint64_t filtered_bases, events, long_events, open_events, shifted_events, alleles, allele_bytes;
} polyhip_variants_info;
int polyhip_call_variants(const polyhip_variants_params *params, uint64_t n, const uint32_t *flags,
                          const uint8_t *mapq, const uint32_t *ref_start, const uint32_t *ref_end,
                          const uint32_t *read_start, const uint8_t *alnA, const uint8_t *alnB,
                          const uint64_t *alnOff, const uint8_t *qual, const uint64_t *qualOff,
                          const uint8_t *ref, uint64_t ref_len, uint64_t *nvariants,
                          polyhip_variant *variants, uint64_t variant_capacity,
                          uint64_t *nallele_bytes, uint8_t *alleles, uint64_t allele_capacity,
                          uint32_t *err);
int polyhip_call_variants_last_info(polyhip_variants_info *info);

/* ---- duplicate marking and coordinate order of the mapper's output (no counterpart in the reference) ---- */
/*
 * polyhip_mark_duplicates marks, among the n entries that polyhip_map_reads, polyhip_map_reads_affine, polyhip_map_pairs or
 * their _refs forms returned, the copies of one template molecule: entries (or pairs) whose unclipped 5' ends coincide.  It
 * is a pass over those arrays: it places nothing and needs neither a text nor an index.  Nothing is removed; the caller
 * clears flags bit 0 of the entries with dup = 1 before a pileup, or writes 0x400 into their SAM FLAG.
 *  err[i], the first that applies, for entries with flags bit 0 (mapped) only; an unmapped entry gets 0 and its other arrays
 *   are not judged:  2 = read_start > read_end, or read_end > read_len, or ref_start > ref_end;  6 = (weight_mode 1) the
 *   length of the quality string, qualOff[i + 1] - qualOff[i], differs from read_len[i];  7 = (weight_mode 1) a byte of the
 *   quality string is below qual_offset or above qual_offset + 93.
 *  Candidate: flags bit 0 is set and err[i] == 0.
 *  Weight: w[i] = weight[i] with weight_mode 0 (0 when weight == NULL); with weight_mode 1 the sum of Q = byte - qual_offset
 *   over the WHOLE quality string of the entry, clipped parts included, counting only Q >= min_weight_qual; it is computed
 *   on the device.  weight_out (may be NULL) receives w[i], and 0 for entries that are not candidates.
 *  End key: with s = flags bit 1 (reverse) and in signed 64-bit integers, u = ref_start - read_start on the forward strand
 *   and u = ref_end - 1 + (read_len - read_end) on the reverse strand: the text position of the read's 5' end with the clips
 *   added back (coordinates are those of the oriented read, as the mapper reports them; u may be negative).  E(i) = (rid[i],
 *   u, s), compared lexicographically; rid == NULL means 0 everywhere.
 *  Fragments: with paired == 0 every candidate; with paired == 1 a candidate whose mate i ^ 1 is not a candidate.
 *  Pairs: with paired == 1, pair p = entries 2p, 2p + 1 when both are candidates.  Its lo mate is the one with the smaller
 *   (E, index), the other its hi mate, and its key is (E_lo, E_hi): which mate was read 1 is NOT part of the key (Picard's
 *   convention: the orientation is that of the leftmost end).  W(p) = w[2p] + w[2p + 1] in uint64.
 *  Pair sets: all pairs with equal keys.  The representative is the pair of greatest W, ties to the lowest p.  Every other
 *   pair of the set is a duplicate: both its mates get dup = 1, rep[lo mate] = the representative's lo mate and rep[hi mate]
 *   = its hi mate.
 *  End sets: all candidates with equal E, pair mates included whether or not their pair is a duplicate.  Ordered by (is a
 *   fragment, w descending, index ascending), the first element is the head.  Every fragment of the set other than the head
 *   gets dup = 1 and rep = the head, so a fragment always loses to any pair mate at the same end (as in Picard and
 *   samtools) and among fragments alone the greatest weight wins.  Pair mates are not changed by end sets.
 *  Every other entry gets dup = 0 and rep = i.
 * All comparisons are on integers and ties go by index, so the result does not depend on the order in which the device
 * gets to the entries.
 * Errors, in this order, all before anything that depends on n is allocated: a NULL params (POLYHIP_ERR_INVALID); paired >
 * 1, weight_mode > 1, min_weight_qual > 93 or qual_offset > 162 (_INVALID, naming the field); paired != 0 with an odd n
 * (_INVALID); n >= 2^32 (POLYHIP_ERR_UNSUPPORTED: the sort's values are uint32); with n > 0 a NULL array that is needed
 * (_INVALID: flags, ref_start, ref_end, read_start, read_end, read_len, dup, rep and err always; rid, weight and weight_out
 * never; qualOff with weight_mode 1, and qual unless qualOff[n] == qualOff[0]); with weight_mode 1 qualOff not ascending
 * (_INVALID), then some read_len[i] * 93 >= 2^32 (_UNSUPPORTED: a weight is uint32).  n == 0 is an empty, successful call.
 * Host pointers only, no stream: the call copies the arrays in (of qual only [qualOff[0], qualOff[n])), runs on the calling
 * thread's current device and copies the results out; the device list does not apply.
 * polyhip_dedup_last_info: the calling thread's last call: entries = n; candidates; bad = entries with err != 0; pairs and
 * fragments = the pairs and the fragment entries; dup_pairs = duplicate pairs (not mates); dup_fragments = duplicate
 * fragment entries; pair_sets and end_sets = the numbers of distinct keys.
 *
 * polyhip_coord_order: order[0..n) is the stable permutation that puts the entries into SAM's coordinate order.  An entry
 * is live when sam_flag[i] (of polyhip_aln_records) lacks 0x4; its place is (rid[i], ref_start[i]).  With paired != 0 an
 * entry that is not live and has a live mate i ^ 1 takes the mate's place, as a SAM writer gives it the mate's RNAME and
 * POS.  Every other entry is unplaced and sorts after all placed ones.  Ties, and the unplaced entries, go in index order.
 * rid == NULL means 0.  Errors, in this order: paired > 1 (_INVALID); paired != 0 with an odd n (_INVALID); n >= 2^32
 * (_UNSUPPORTED); with n > 0 a NULL sam_flag, ref_start or order (_INVALID).  n == 0 is an empty, successful call.  The
 * calling convention is polyhip_mark_duplicates'.
 */
typedef struct polyhip_dedup_params {
    uint32_t paired;           /* 0: every entry is a read of its own; 1: mates in the order 2i, 2i + 1 */
    uint32_t weight_mode;      /* 0: weight[] is the caller's (NULL = all 0); 1: computed from qual */
    uint32_t min_weight_qual;  /* weight_mode 1: a base adds Q to the weight only if Q >= this; 0..93 (Picard uses 15) */
    uint32_t qual_offset;      /* as polyhip_pileup_qual: <= 162 */
} polyhip_dedup_params;
typedef struct polyhip_dedup_info {
    uint64_t entries, candidates, bad, pairs, fragments, dup_pairs, dup_fragments, pair_sets, end_sets;
} polyhip_dedup_info;
int polyhip_mark_duplicates(const polyhip_dedup_params *params, uint64_t n, const uint32_t *flags,
                            const uint32_t *rid, const uint32_t *ref_start, const uint32_t *ref_end,
                            const uint32_t *read_start, const uint32_t *read_end,
                            const uint32_t *read_len, const uint32_t *weight, const uint8_t *qual,
                            const uint64_t *qualOff, uint32_t *weight_out, uint8_t *dup,
                            uint32_t *rep, uint32_t *err);
int polyhip_dedup_last_info(polyhip_dedup_info *info);
int polyhip_coord_order(uint64_t n, uint32_t paired, const uint32_t *sam_flag, const uint32_t *rid,
                        const uint32_t *ref_start, uint32_t *order);

/* ---- read trimming: quality ends, 3' adapters, mate overlap (no counterpart in the reference) ---- */
/*
 * polyhip_trim_reads cuts low-quality ends and 3' adapters off a packed batch of reads before it is mapped; the reference's
 * io/fastq only parses.  Reads (reads, off) as the mappers take them, qualities (qual, qual_off) as polyhip_fastq_pack_qual
 * gives them, or both NULL.  Adapters: nadapters (0..255) strings of 1..64 bytes of upper-case ACGT, packed as (adapters,
 * adapter_off[nadapters + 1]).  Entry i in is entry i out: no read is removed, an emptied read has length 0 in the output, so
 * pairs, rec_start and every later stage keep their indices (the mappers report a read shorter than seed_len as unmapped).
 * Per read r of m bytes, with start a and end b of what is kept:
 *  1. Judging, of the whole read before anything else looks at it.  err[i] = 1 if qualities are given and the length of the
 *   quality string differs from m; else 2 if one of its bytes is below qual_offset or above qual_offset + 93
 *   (polyhip_pileup_qual's range); else 0.  A read with err != 0 gets start = end = 0, flags = 0, is empty in the output
 *   and takes no part in anything below.
 *  2. Quality ends (BWA's rule), Q_k = qual[k] - qual_offset, both walks on the read as it came.  3' end, when min_qual_3p >
 *   0: for k = m - 1, m - 2, ... the sum s += min_qual_3p - Q_k starting from 0; the walk stops before the first k at which
 *   s < 0.  b = the k at which s first reached its greatest value, if that value is > 0 (strictly: of equal sums the largest
 *   k), else b = m.  5' end, when min_qual_5p > 0: the mirror image over k = 0, 1, ...; a = one past the k of the first
 *   greatest positive sum, else a = 0.  If a >= b then a = b = 0.  After that flags bit 0 is set iff b < m and bit 1 iff a >
 *   0; later steps do not clear them.
 *  3. 3' adapters, on r[a, b).  For adapter t of p bytes and a start s in [a, b), L = min(p, b - s).  s qualifies iff L >=
 *   min_overlap and 100 * mism <= adapter_err_pct * L, where mism counts the k < L with upper(r[s + k]) != t[k]; a read byte
 *   that is not one of ACGTacgt is a mismatch.  A whole adapter inside the read and a prefix of it at the read's end are
 *   both this rule.  The hit is the smallest qualifying s over all adapters, a tie goes to the lowest adapter index.  Then b
 *   = s, flags bit 2 is set and bits 8..15 hold the adapter's index.
 *  4. Length.  If b - a < min_len the read comes out empty and flags bit 3 is set; start and end keep a and b.
 *  5. Output.  start[i] = a, end[i] = b.  out_off has nreads + 1 entries and starts at 0; out_reads holds r[a, b) of every
 *   read that is not empty, back to back, the bytes as they were (no case change); out_qual the same slices of the quality
 *   strings under the same offsets.  out_reads and out_qual hold off[nreads] - off[0] bytes: there is no capacity argument.
 * polyhip_trim_pairs: mate 1 of pair i is read i of (reads1, off1, qual1, qual_off1), mate 2 read i of the second batch;
 * entry 2i of start / end / flags / err is mate 1 and entry 2i + 1 mate 2, as in polyhip_map_pairs, and each mate has an
 * output batch of its own.  Steps 1-3 run on each mate by itself.  Then, before step 4:
 *  P. Mate overlap, only when pair_min_overlap > 0, both mates have err == 0 and neither has flags bit 2.  An insert of I <
 *   m bases is read from both ends and runs into the adapter after I bytes, so for I in [pair_min_overlap, min(m1, m2)], on
 *   the mates as they came and from their first bytes: I qualifies iff 100 * mism <= pair_err_pct * I, where mism counts the
 *   k < I with upper(r1[k]) != comp(upper(r2[I - 1 - k])); comp is A<->T, C<->G, any other byte is a mismatch.  The greatest
 *   qualifying I wins.  On a mate with b > I: b = I, flags bit 4 is set, and if a >= b then a = b = 0.  The work of this
 *   step grows with m1 * m2.
 * Every decision is integer arithmetic and no atomic decides an output byte: the same call gives the same bytes.
 * Errors, in this order, all before anything is allocated: a NULL params (POLYHIP_ERR_INVALID); qual_offset > 162,
 * min_qual_5p > 93, min_qual_3p > 93, adapter_err_pct > 100, min_overlap == 0 or pair_err_pct > 100 (_INVALID, naming the
 * field); nadapters > 255 (_INVALID); with nadapters > 0 a NULL adapters or adapter_off, then an adapter that is empty, longer
 * than 64 bytes or holds a byte outside ACGT (_INVALID, naming the adapter's index); a cut-off > 0 with qual == NULL
 * (_INVALID); qual and qual_off not both given or both NULL, or in polyhip_trim_pairs given for one mate only (_INVALID);
 * out_qual given without qual or the other way round (_INVALID); a NULL start, end, flags, err, out_reads or out_off, or with
 * nreads > 0 a NULL reads or off (_INVALID); offsets that decrease (_INVALID); a read of 2^24 bytes or more
 * (POLYHIP_ERR_UNSUPPORTED: the running sums are 32-bit).  nreads == 0 is an empty, successful call that writes out_off[0] =
 * 0.  Host pointers only, no stream: the call copies the batch in (of the bytes only [off[0], off[nreads])), runs on the
 * calling thread's current device and copies the results out; the device list does not apply.
 * polyhip_trim_last_info: the calling thread's last call: reads = the entries (2 * npairs for pairs); bytes_in and bytes_out
 * = sequence bytes taken and kept; cut_3p, cut_5p, adapter_hits, overlap_cut, too_short = entries with flags bit 0, 1, 2, 4,
 * 3; bad = entries with err != 0.
 */
typedef struct polyhip_trim_params {
    uint32_t qual_offset;       /* Phred offset, 33 for FASTQ; <= 162 */
    uint32_t min_qual_5p;       /* quality cut-off at the 5' end, 0 = off; <= 93 */
    uint32_t min_qual_3p;       /* quality cut-off at the 3' end, 0 = off; <= 93 */
    uint32_t adapter_err_pct;   /* mismatches allowed per 100 compared bytes, 0..100 */
    uint32_t min_overlap;       /* fewest adapter bytes that count as a hit, >= 1 */
    uint32_t min_len;           /* a shorter read comes out empty */
    uint32_t pair_min_overlap;  /* polyhip_trim_pairs: shortest insert looked for, 0 = off */
    uint32_t pair_err_pct;      /* 0..100 */
} polyhip_trim_params;
typedef struct polyhip_trim_info {
    uint64_t reads, bytes_in, bytes_out, cut_3p, cut_5p, adapter_hits, overlap_cut, too_short, bad;
} polyhip_trim_info;
int polyhip_trim_reads(const polyhip_trim_params *params, const uint8_t *adapters,
                       const uint32_t *adapter_off, uint32_t nadapters, const uint8_t *reads,
                       const uint64_t *off, const uint8_t *qual, const uint64_t *qual_off,
                       uint64_t nreads, uint32_t *start, uint32_t *end, uint32_t *flags, uint32_t *err,
                       uint8_t *out_reads, uint8_t *out_qual, uint64_t *out_off);
int polyhip_trim_pairs(const polyhip_trim_params *params, const uint8_t *adapters,
                       const uint32_t *adapter_off, uint32_t nadapters, const uint8_t *reads1,
                       const uint64_t *off1, const uint8_t *qual1, const uint64_t *qual_off1,
                       const uint8_t *reads2, const uint64_t *off2, const uint8_t *qual2,
                       const uint64_t *qual_off2, uint64_t npairs, uint32_t *start, uint32_t *end,
                       uint32_t *flags, uint32_t *err, uint8_t *out_reads1, uint8_t *out_qual1,
                       uint64_t *out_off1, uint8_t *out_reads2, uint8_t *out_qual2,
                       uint64_t *out_off2);
int polyhip_trim_last_info(polyhip_trim_info *info);

/* ---- demultiplexing: pooled reads split by inline 5' barcodes (no counterpart in the reference) ---- */
/*
 * polyhip_demux_reads finds the inline barcode at the 5' end of every read of a packed batch, and hands the batch back grouped
 * by sample: sample k is a contiguous run of reads of the output batch, which goes to polyhip_trim_reads and the mappers as it
 * is (they take offsets that do not start at 0).  Reads (reads, off) and qualities (qual, qual_off) as polyhip_trim_reads takes
 * them.  A barcode set: nbarcodes (1..4096) strings of 4..64 bytes of upper-case ACGT, the lengths may differ, packed as
 * (barcodes, barcode_off[nbarcodes + 1]).  0xFFFFFFFF is "none" below.  Per read r of m bytes:
 *  1. Judging.  err[i] = 1 if qualities are given and the length of the quality string differs from m, else 0; the quality
 *   bytes are not interpreted.  A read with err != 0 has barcode = bstart = mism = none and flags = 0, is unassigned and is
 *   empty in the output.
 *  2. Distance to barcode t of p bytes.  For every start s in [0, max_shift] with s + p <= m: the number of k < p with
 *   upper(r[s + k]) != t[k]; a read byte that is not one of ACGTacgt is a mismatch.  d_t is the smallest of these numbers and
 *   s_t the smallest s that has it; d_t is none if no start fits.
 *  3. Choice.  t1 is the barcode with the smallest d, the lowest index among equals; d2 the smallest d over all t != t1, none
 *   if there is no such barcode or none of them fits.  No hit (flags bit 0): d_t1 is none or > max_mismatches.  Ambiguous
 *   (flags bit 1): a hit, d2 is not none and d2 - d_t1 < min_margin.  Otherwise the read has a barcode: barcode[i] = t1,
 *   bstart[i] = s_t1, mism[i] = d_t1.  With bit 0 or bit 1 set the three are none.
 *  4. Sample.  polyhip_demux_reads: sample[i] = barcode[i], and nsamples must equal nbarcodes; the read is assigned iff it has
 *   a barcode.  polyhip_demux_pairs: mate 1 of pair i is read i of (reads1, off1, qual1, qual_off1) and is judged against set
 *   1, mate 2 is read i of the second batch and is judged against set 2 when nbarcodes2 > 0; entries 2i and 2i + 1 of barcode
 *   / bstart / mism / flags / err are mate 1 and mate 2, as in polyhip_map_pairs.  A mate that is not judged against a set
 *   has barcode = bstart = mism = none and flags = 0; its err is judged all the same.  The pair is assigned iff neither mate
 *   has err != 0, every judged mate has a barcode and the sample is not none.  With nbarcodes2 == 0 the sample is b1 and
 *   nsamples must equal nbarcodes1; otherwise it is pair_sample[b1 * nbarcodes2 + b2], and a table value of 0xFFFFFFFF sets
 *   flags bit 2 on both entries (which keep barcode, bstart and mism).  sample[i] of an unassigned read or pair is none.
 *  5. Clip.  On an entry that has a barcode, whose read or pair is assigned, and with clip != 0: a = min(m, bstart + p +
 *   clip_extra).  Otherwise a = 0, except that an entry with err != 0 comes out empty.  The entry comes out as r[a, m) with
 *   the same slice of its quality string, the bytes as they were.
 *  6. Grouping.  Group g = sample if assigned, else nsamples.  order is the stable permutation by g: input order within a
 *   group, the unassigned last.  sample_start[k], k = 0..nsamples + 1, is the number of reads (pairs) with g < k.  Output
 *   read j is input read order[j]: sample k is the sub-batch out_off[sample_start[k] .. sample_start[k + 1]] (one entry more
 *   than reads, as every offset array), the unassigned are sample nsamples.  out_off has n + 1 entries and starts at 0;
 *   out_reads and out_qual hold off[n] - off[0] bytes: there is no capacity argument.  In polyhip_demux_pairs both mates'
 *   batches use the same order.
 * Every decision is integer arithmetic and no atomic decides an output byte: the same call gives the same bytes.
 * Errors, in this order, all before anything is allocated: a NULL params (POLYHIP_ERR_INVALID); max_shift > 63,
 * max_mismatches > 64, clip > 1, clip_extra >= 2^24, nsamples == 0 or > 65536 (_INVALID, naming the field); nbarcodes == 0 or
 * > 4096, in polyhip_demux_pairs nbarcodes1 likewise and nbarcodes2 > 4096 (_INVALID); a NULL barcodes or barcode_off of a set
 * that is not empty, then a barcode shorter than 4 or longer than 64 bytes or with a byte outside ACGT (_INVALID, naming the
 * set and the barcode's index); an nsamples that differs from nbarcodes (nbarcodes1 when nbarcodes2 == 0) (_INVALID); with
 * nbarcodes2 > 0 a NULL pair_sample, then an entry that is neither below nsamples nor 0xFFFFFFFF (_INVALID, naming the entry);
 * qual, qual_off and out_qual not all given or all NULL, or in polyhip_demux_pairs given for one mate only (_INVALID); a NULL
 * barcode, bstart, mism, flags, err, sample, order, sample_start, out_reads or out_off, or with n > 0 a NULL reads or off
 * (_INVALID); offsets that decrease (_INVALID); a read of 2^24 bytes or more, or 2^32 reads or more (POLYHIP_ERR_UNSUPPORTED).
 * n == 0 is an empty, successful call that writes out_off[0] = 0 and zeroes every sample_start.  Host pointers only, no
 * stream: the call copies the batch in, runs on the calling thread's current device and copies the results out; the device
 * list does not apply.
 * polyhip_demux_last_info: the calling thread's last call: reads = the entries (2 * npairs for pairs); assigned = entries of
 * assigned reads or pairs; exact = entries that have a barcode with mism == 0; no_barcode, ambiguous, not_in_sheet = entries
 * with flags bit 0, 1, 2; bad = entries with err != 0; bytes_in and bytes_out = sequence bytes taken and written.
 */
typedef struct polyhip_demux_params {
    uint32_t max_shift;       /* a barcode may start at byte 0..max_shift of its read; <= 63 */
    uint32_t max_mismatches;  /* <= 64 */
    uint32_t min_margin;      /* the best barcode must beat every other by this many mismatches; 0: ties to the lowest index */
    uint32_t clip;            /* 0 / 1: cut the barcode and what precedes it */
    uint32_t clip_extra;      /* further bytes cut after the barcode (a linker), < 2^24 */
    uint32_t nsamples;        /* groups of the output, 1..65536 */
} polyhip_demux_params;
typedef struct polyhip_demux_info {
    uint64_t reads, assigned, exact, no_barcode, ambiguous, not_in_sheet, bad, bytes_in, bytes_out;
} polyhip_demux_info;
int polyhip_demux_reads(const polyhip_demux_params *params, const uint8_t *barcodes,
                        const uint32_t *barcode_off, uint32_t nbarcodes, const uint8_t *reads,
                        const uint64_t *off, const uint8_t *qual, const uint64_t *qual_off,
                        uint64_t nreads, uint32_t *barcode, uint32_t *bstart, uint32_t *mism,
                        uint32_t *flags, uint32_t *err, uint32_t *sample, uint32_t *order,
                        uint64_t *sample_start, uint8_t *out_reads, uint8_t *out_qual,
                        uint64_t *out_off);
int polyhip_demux_pairs(const polyhip_demux_params *params, const uint8_t *barcodes1,
                        const uint32_t *barcode_off1, uint32_t nbarcodes1, const uint8_t *barcodes2,
                        const uint32_t *barcode_off2, uint32_t nbarcodes2, const uint32_t *pair_sample,
                        const uint8_t *reads1, const uint64_t *off1, const uint8_t *qual1,
                        const uint64_t *qual_off1, const uint8_t *reads2, const uint64_t *off2,
                        const uint8_t *qual2, const uint64_t *qual_off2, uint64_t npairs,
                        uint32_t *barcode, uint32_t *bstart, uint32_t *mism, uint32_t *flags,
                        uint32_t *err, uint32_t *sample, uint32_t *order, uint64_t *sample_start,
                        uint8_t *out_reads1, uint8_t *out_qual1, uint64_t *out_off1,
                        uint8_t *out_reads2, uint8_t *out_qual2, uint64_t *out_off2);
int polyhip_demux_last_info(polyhip_demux_info *info);

/* ---- primer dimers: which primers of a pool bind each other (no counterpart in the reference) ---- */
/*
 * A ranking screen for the ungapped Watson-Crick duplexes two primers can form, scored by nearest-neighbour stacking alone.
 * There is NO initiation term, no terminal-AT term, no dangling end, no loop and no mismatch term: the numbers rank pairs of
 * one pool against each other, they are not a Tm and not a free energy of the duplex.
 * Bytes.  ASCII lower case is folded to upper case.  A, C, G, T have the codes 0..3; every other byte, U and N among them, has
 *   code 4 and pairs with nothing.
 * Stack table.  stack_dg[16], int32 in cal/mol, entry 4 * code(a) + code(b) for the dinucleotide ab read 5'->3' on x; every
 *   entry lies in [-30000, 0].  polyhip_primer_stack_dg(temp_mK, out) fills it from the library's nearest-neighbour table
 *   (SantaLucia 1998, the 16 (dH, dS) pairs polyhip_santalucia_* use) in integers: H10 = 10 * dH, S10 = 10 * dS, num = H10 *
 *   1,000,000 - temp_mK * S10 in int64, the entry is num / 10,000 rounded half away from zero: sign(num) * ((|num| + 5000) /
 *   10000).  temp_mK is the temperature in millikelvin and must lie in [273150, 338000] (above 338028 the TA entry turns
 *   positive); anything else is POLYHIP_ERR_INVALID.  The table is symmetric under reverse complement, which makes dg_any(x,
 *   y) == dg_any(y, x).
 * Duplex of the ordered pair (x, y), x of m and y of n bytes, 1 <= m, n <= 64.  The shift s runs over -(n - 1) .. m - 1.  At
 *   shift s position i of x faces y[n - 1 - (i - s)] when 0 <= i - s <= n - 1: the antiparallel arrangement, x's 3' end on the
 *   right and y's 3' end on the left.  Position i is paired iff code(x[i]) < 4 and code(y[n - 1 - (i - s)]) == 3 - code(x[i]).
 *   A run is a maximal interval [i0, i1] of consecutive paired positions at one shift, pairs = i1 - i0 + 1, dg(run) = the sum
 *   over i = i0 .. i1 - 1 of stack_dg[4 * code(x[i]) + code(x[i + 1])].  A run of one pair has no stack and is no candidate.
 * Per pair.  dg_any is the smallest dg over the runs of two or more pairs at all shifts, and with it go shift = s + (n - 1)
 *   (so >= 0), pos = i0 and pairs; among equal dg the smallest s wins, then the smallest i0.  Without such a run dg_any = 0 and
 *   shift = pos = pairs = 0.  dg_end is the same minimum over the runs with i1 = m - 1 only -- x's 3' base is paired, the runs
 *   a polymerase can extend --, with its shift and pairs (pos = m - pairs).  dg_end(y, x), the other primer's 3' end, is the
 *   transposed pair's.
 * Primer errors.  err = 1 for an empty primer, 2 for one longer than 64 bytes, else 0.  A pair with a bad primer has dg_any =
 *   dg_end = 0 in the matrix; in the screen a bad y is never a partner and never counted, and a bad x has no partner and
 *   counts nothing.
 * Primers are packed like reads: primer i of X is X[offX[i] .. offX[i + 1]).  Pool mode: Y == NULL, offY == NULL and ny == 0
 * mean Y = X (errY may then be NULL); any other combination of a missing Y, offY or ny is refused.
 * polyhip_primer_dimer_matrix: dg_any and dg_end are row-major nx x ny; either may be NULL, not both.  nx * ny > 2^30 is
 *   POLYHIP_ERR_UNSUPPORTED: the caller tiles.
 * polyhip_primer_dimer_screen: per x, over the valid y: the partner is the j with the smallest dg, the smallest j among
 *   equals, and 0xFFFFFFFF when that dg is 0 (shift, pos and pairs are then 0); otherwise shift, pos and pairs are those of
 *   the pair (x, partner).  any_count / end_count: the valid y with dg_any <= any_threshold / dg_end <= end_threshold; both
 *   thresholds are <= 0.  In pool mode the pair of a primer with itself counts like any other.  Every output has nx entries
 *   (errY ny).  The call never holds nx x ny values: ny < 2^32 - 1 is the only limit (else POLYHIP_ERR_UNSUPPORTED).  The only
 *   atomics are an integer minimum of (dg, j) and integer sums: the result depends neither on the order of the launches nor
 *   on how the work is cut, and the same call gives the same bytes.
 * Errors, in this order, all before anything is allocated: a NULL params or stack_dg (POLYHIP_ERR_INVALID); a table entry
 * outside [-30000, 0] (_INVALID, naming the entry); any_threshold > 0, then end_threshold > 0 (_INVALID, naming the field);
 * Y, offY and ny neither all given nor all missing (_INVALID); a NULL output -- the screen's arrays; both planes of the
 * matrix; errX; errY outside pool mode -- or with nx > 0 a NULL X or offX (_INVALID); offsets that decrease (_INVALID, offX
 * before offY); the size limit (_UNSUPPORTED).  nx == 0 is an empty, successful call that writes nothing.  Host pointers only,
 * no stream: the calls copy the primers in, run on the calling thread's current device and copy the results out; the device
 * list does not apply.
 * polyhip_primer_dimer_last_info: the calling thread's last matrix or screen call: primers = nx + ny (nx in pool mode); bad =
 * those with err != 0; pairs = valid x times valid y; shifts = the sum of m + n - 1 over these pairs; launches = kernels
 * started.
 */
typedef struct polyhip_dimer_params {
    int32_t stack_dg[16];   /* cal/mol, each in [-30000, 0] */
    int32_t any_threshold;  /* any_count: the y with dg_any <= this; <= 0 */
    int32_t end_threshold;  /* end_count: the y with dg_end <= this; <= 0 */
} polyhip_dimer_params;
typedef struct polyhip_dimer_info {
    uint64_t primers, bad, pairs, shifts, launches;
} polyhip_dimer_info;
int polyhip_primer_stack_dg(uint32_t temp_mK, int32_t out[16]);
int polyhip_primer_dimer_matrix(const int32_t stack_dg[16], const uint8_t *X, const uint64_t *offX,
                                uint64_t nx, const uint8_t *Y, const uint64_t *offY, uint64_t ny,
                                int32_t *dg_any, int32_t *dg_end, uint32_t *errX, uint32_t *errY);
int polyhip_primer_dimer_screen(const polyhip_dimer_params *params, const uint8_t *X,
                                const uint64_t *offX, uint64_t nx, const uint8_t *Y,
                                const uint64_t *offY, uint64_t ny, int32_t *any_dg,
                                uint32_t *any_partner, uint32_t *any_shift, uint32_t *any_pos,
                                uint32_t *any_pairs, int32_t *end_dg, uint32_t *end_partner,
                                uint32_t *end_shift, uint32_t *end_pairs, uint32_t *any_count,
                                uint32_t *end_count, uint32_t *errX, uint32_t *errY);
int polyhip_primer_dimer_last_info(polyhip_dimer_info *info);

/* ---- R1: the path's one collective -- all-gather of per-rank sketches (RCCL over xGMI) ---- */
/*
 * For hosts without torch.distributed (the Go/cgo drop-in); one process per GPU.  RCCL is
 * resolved at run time (dlopen librccl.so.1), so libpolyhip has no link-time dependency on it.
 * Rank 0 obtains the 128-byte id and passes it to the other ranks by its own channel; every
 * rank then creates its communicator on its current HIP device.  d_all receives
 * nranks * n_local sketches in rank order; the call enqueues one ncclAllGather on `stream`.
 * EVERY rank must pass the SAME n_local (ncclAllGather's contract; the library cannot check it
 * across processes): with ragged shards, pad each rank's block to the largest shard and trim
 * after the gather, as poly_amd/sharding.py::gather_sketches does.  n_local == 0 still enters
 * the collective (all ranks then contribute nothing).  Then each rank runs
 * polyhip_mash_shared_counts_dev(X = its block of d_all, Y = d_all).
 */
typedef struct polyhip_comm polyhip_comm;
int polyhip_comm_unique_id(uint8_t id[128]);
int polyhip_comm_init_rank(const uint8_t id[128], int rank, int nranks,
                           polyhip_comm **out);
int polyhip_comm_destroy(polyhip_comm *c);
int polyhip_comm_rank(const polyhip_comm *c);
int polyhip_comm_size(const polyhip_comm *c);
int polyhip_allgather_sketches_dev(polyhip_comm *c, const uint32_t *d_local,
                                   uint64_t n_local, uint32_t s,
                                   uint32_t *d_all, polyhip_stream_t stream);
/* Ragged all-gather IN PLACE: rank r owns bytes [offsets[r], offsets[r+1]) of d_buf (nranks + 1 ascending offsets, the
 * same on every rank) and every rank ends up with all segments -- one grouped call of nranks ncclBroadcasts, each rank
 * the root of its own segment.  What polyhip_mash_index_allgather_dev moves the parts of the index with. */
int polyhip_allgatherv_dev(polyhip_comm *c, void *d_buf, const uint64_t *offsets,
                           polyhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* POLYHIP_H */
