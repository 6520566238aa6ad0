/*
 * fxgpu.h -- C ABI of libfxgpu.so: MI355X-native FASTA/FASTQ index build and
 * batched random access (the drop-in boundary under the pyfastx object API).
 *
 * pyfastx (lmdu/pyfastx v2.3.1) has no plugin/FFI layer: its hot path is a set
 * of internal C functions inside one CPython extension.  Each entry point
 * below names the reference function(s) whose work it replaces; the
 * Python-facing mirror (pyfastx_amd/) binds these with ctypes, and
 * INTEGRATION.md shows the C stub a pyfastx maintainer would add at those
 * call sites.
 *
 * Conventions
 *   - Plain C: opaque handle, pointers and sizes only.  No torch / HIP types.
 *   - All offsets are 0-based offsets into the UNCOMPRESSED byte stream, i.e.
 *     exactly the numbers the reference stores in its .fxi (seq.boff, read.soff...).
 *   - Every function returns FX_OK (0) or a negative fx_status; the message is
 *     available from fx_last_error() (thread-local).
 *   - `where` arguments say where caller-provided arrays live: FX_HOST or
 *     FX_DEVICE (device pointers must belong to the handle's GPU).
 *   - There is NO CPU fallback: without a usable gfx950 device every call that
 *     needs one fails with FX_EDEVICE.
 *   - A handle is not re-entrant; use one handle per thread / per GPU.
 */
#ifndef FXGPU_H
#define FXGPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fx_handle fx_handle;

typedef enum {
    FX_OK = 0,
    FX_ENOENT = -1,   /* input file missing            -> FileExistsError (fasta.c:84-87)  */
    FX_EFORMAT = -2,  /* not FASTA/FASTQ               -> RuntimeError    (fasta.c:107-110) */
    FX_EIO = -3,      /* read / inflate error                                               */
    FX_EDEVICE = -4,  /* no GPU, HIP error                                                  */
    FX_ENOMEM = -5,
    FX_ERANGE = -6,   /* index / interval out of range -> IndexError / ValueError           */
    FX_EINVAL = -7,
    FX_ESTATE = -8    /* call order (e.g. read before build)                                */
} fx_status;

enum { FX_HOST = 0, FX_DEVICE = 1 };

/* fetch flags (per call) */
enum {
    FX_UPPER = 1,       /* remove_space_uppercase, util.c:181-194                 */
    FX_REVERSE = 2,     /* reverse_seq, util.c:251-261                            */
    FX_COMPLEMENT = 4,  /* complement_seq / comp_map, util.c:228-237, 263-269     */
    FX_LONG = 16,       /* hint: ranges are long (KiB+): one wave per query, 1 KiB per step   */
    FX_RAW = 8          /* no despace: plain pyfastx_index_random_read (index.c:683-692), for
                           names, Sequence.raw / .description, Read.raw             */
};

const char *fx_last_error(void);
const char *fx_version(void);
int fx_device_count(void);

/* ------------------------------------------------------------------ staging
 * Replaces gzopen/gzread streaming in pyfastx_init_index (index.c:15-98) and
 * the per-query fseeko/fread | zran_seek/zran_read of pyfastx_index_random_read
 * (index.c:683-692) / pyfastx_read_random_reader (read.c:37-45): the whole
 * uncompressed stream becomes one resident blob in HBM.                        */

/* Plain or gzip file -> pinned double buffers -> hipMemcpyAsync -> HBM.  A BGZF file is inflated on the device (one wave per
 * member; every member checked against the CRC-32 of its trailer, as zlib's gzread does for the reference); a BGZF file of
 * 512 MiB or more in groups of FX_BGZF_GROUP bytes (256 MiB; 0: all at once) BEHIND its staging, the blob sized from the ratio
 * of the first group (what is left over stays with the blob: fx_size is what it holds).  A single gzip stream is inflated on
 * the host cores. */
int fx_open_file(const char *path, int device, fx_handle **out);
/* Where the last fx_open_file of a PLAIN file spent its time (this thread): *alloc_s = the device allocation of the blob --
 * the first block of tens of GB a process asks the driver for can take seconds (35 GB: 2.9 s measured), the next one of that
 * size 0.3 ms --, *stage_s = page cache -> pinned pieces -> HBM.  (The reference has no counterpart: it reads through a 1 MiB
 * buffer, kseq.h:13.) */
int fx_open_laps(double *alloc_s, double *stage_s);
/* A PLAIN file staged in the background (round 6): the handle comes back as soon as its blob is allocated, the staging lanes
 * copy the file into it in file order.  fx_stage_wait(h, upto): returns when the first `upto` bytes are on the device
 * (upto < 0: the whole file; the lanes are joined and the handle is an ordinary one from then on).  Until then the caller
 * works on PREFIXES through views of the blob -- fx_open_device(fx_device_ptr(h) + off, len + halo), fx_set_shard,
 * fx_set_halo: byte ranges as in the sharded build -- e.g. formats and ships the table leaves of an index file
 * (fx_fxi_part_*) while the rest of the input still arrives; no other call on THIS handle before fx_stage_wait(h, -1).
 * fx_close waits for the lanes.  gzip input: FX_EINVAL.  (The reference reads and indexes in one loop, fastq.c:8-182.) */
int fx_open_file_async(const char *path, int device, fx_handle **out);
int fx_stage_wait(fx_handle *h, int64_t upto);
/* ... and the last fx_fastq_build / fx_fastq_build_comp (this thread), eight doubles, seconds: [0] the sample of the stream and its
 * wait, [1] allocations + launches of the count pass, [2] the wait for it, [4] plan + allocation of the read table, [5] row kernels +
 * their wait ([3], [6], [7]: unused).  Diagnostic: a build that takes seconds instead of milliseconds is waiting for the driver. */
int fx_build_laps(double *out8);
/* What a file holds and how long its stream is once inflated -- kind 0: plain; 1: BGZF (*n_bytes = sum of the members'
 * ISIZE, from a walk over their headers); 2: a single gzip stream (*n_bytes = -1: unknown without inflating it). */
int fx_stream_size(const char *path, int64_t *n_bytes, int *kind);
/* ONE byte-range shard of a file (whole-file scan semantics of index.c:230-372 across the cuts come from the
 * stitch below): bytes [off, off + len + halo) of the uncompressed stream, clamped to its end, become the blob, and the
 * shard context is taken from the file -- base = off, prev_byte = the byte before it, is_last, halo (fx_set_shard /
 * fx_set_halo need not be called).  A plain file is read only in that range; of a BGZF file only the members that
 * cover it are read, staged and inflated.  A single gzip stream cannot be entered in the middle: FX_EINVAL. */
int fx_open_file_range(const char *path, int64_t off, int64_t len, int64_t halo, int device, fx_handle **out);
/* Copy nbytes from host memory into HBM. */
int fx_open_host(const void *data, int64_t nbytes, int device, fx_handle **out);
/* Adopt (do not copy, do not free) a blob already in this GPU's HBM; 16-byte aligned. */
int fx_open_device(const void *dptr, int64_t nbytes, int device, fx_handle **out);

/* Shard context (multi-GPU byte-range sharding): this handle holds
 * bytes [base, base+n) of a longer stream; prev_byte is stream[base-1] (pass
 * 10 when base == 0); is_last says the shard ends at end-of-stream.  Default
 * after fx_open_*: base 0, prev_byte 10, is_last 1. */
int fx_set_shard(fx_handle *h, int64_t base, int prev_byte, int is_last);

int fx_close(fx_handle *h);
/* Scratch of an open (compressed bytes of a BGZF file, its match map: hundreds of MB for tens of milliseconds) and, since
 * round 4, the blob of a closed handle are kept in a per-process pool for the next open (FX_SCRATCH_CACHE_MB, default 24576:
 * the driver clears memory it hands out or takes back, 20 ms per 3 GB in the way of the next open's copies; the library
 * empties the pool by itself before a device allocation fails).  This gives the idle blocks back to the driver now.
 * Blobs LARGER than that whole limit (the 35 GB of a sequencing run) are kept too when their handle closes -- freeing one
 * makes the process's next large allocation wait seconds for the driver -- under a cap of their own: FX_SCRATCH_KEEP_BIG_MB
 * per device (default half the device's memory; 0: none) and FX_SCRATCH_BIG_TTL_S (default 300 s idle, checked at the next
 * call into the pool; 0: no limit).  A process that SHARES its GPU with others (several ranks on one device) should call
 * fx_release_scratch after closing large files: nobody else can reclaim what idles here.  (index.c:431-474 frees
 * synchronously; there is no device memory in the reference.) */
int fx_release_scratch(void);
/* The decision behind that cap, as a pure function (tests pin it): the device holds n large idle blocks of idle_caps[]
 * bytes, one more of `cap` bytes comes back, keep_bytes are allowed in all.  -> 1: the new block is kept and the idle
 * blocks with evict[i] = 1 (the smallest, as many as needed) are freed; 0: the new block is freed and nothing else. */
int fx_scratch_policy(const int64_t *idle_caps, int n, int64_t cap, int64_t keep_bytes, int32_t *evict);
/* FX_DEBUG_FILL=<0..255> (decimal; read once at load; unset or empty: off) fills every block a plain device allocation or the
 * scratch pool hands out, fresh or reused, with that byte over its whole capacity, the device waited for on both sides of the
 * fill: a test mode that turns a forgotten clear into a wrong number (tests/test_gpu_clean_memory.py runs with 255).  The reuse
 * of a handle's grow-only arrays, its per-call scratch arena among them, is not filled.  This reports that the mode was on: *byte = the value in force or -1,
 * *blocks and *bytes = what has been filled since load (any pointer may be NULL). */
int fx_debug_fill_info(int *byte, int64_t *blocks, int64_t *bytes);
/* Pinned (page-locked) host memory out of a per-process pool, for the arrays a caller hands to the batched entry
 * points with FX_HOST: answers land in it by DMA -- no bounce buffer, no first-touch page faults of a fresh buffer
 * (what the copy out of pyfastx_index_fill_cache's cache costs the reference per getter, sequence.c:346-347, is paid
 * here once per batch) -- and query arrays in it go up without a staging copy.  Released blocks stay pinned for the
 * next request of a similar size (FX_PINNED_CACHE_MB, default 2048; fx_pinned_trim gives them back).
 * fx_pinned_holds: does [p, p + bytes) lie inside one block that is handed out? */
void *fx_pinned_alloc(int64_t bytes);
void fx_pinned_free(void *p);
int fx_pinned_holds(const void *p, int64_t bytes);
int fx_pinned_trim(void);
int64_t fx_size(const fx_handle *h);          /* uncompressed bytes held          */
/* Free and total HBM of a device, now.  The reference streams files of any size through a 1 MiB buffer (kseq.h:13,
 * index.c:229-230); here a stream larger than what is free is built and served in byte-range WINDOWS that take turns in HBM
 * (pyfastx_amd/windows.py, fx_open_file_range): this is the number that decides. */
int fx_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);
int fx_is_gzip(const fx_handle *h);           /* is_gzip_format, util.c:307-325   */
const void *fx_device_ptr(const fx_handle *h);/* device address of the blob       */
/* Raw bytes [off, off+n) of the stream -> dst (host).  Serves names,
 * Sequence.raw / .description (sequence.c:299-335), Read.raw (read.c:124-150). */
int fx_read_bytes(fx_handle *h, int64_t off, int64_t n, void *dst);
/* First non-space byte of the stream (fasta_validator / fastq_validator, util.c:95-150). */
int fx_first_byte(fx_handle *h, int *out);

/* ------------------------------------------------------------ FASTA index
 * Replaces the hot loop of pyfastx_create_index (index.c:230-372).           */
typedef struct {
    int64_t n_seq;        /* stat.seqnum                                      */
    int64_t seq_len;      /* stat.seqlen  (sum of slen)                       */
    int64_t n_lines;      /* newline-terminated lines seen (incl. EOF line)   */
    int64_t n_bytes;
} fx_fasta_summary;

/* Build the record table on the GPU (kept resident in HBM for fetches).
 * full_name, bit 0: chrom = whole header (index.c:282-285) instead of first token.
 * bit 1 (FX_BUILD_COMP): count the letters on the way -- the reference's second pass over the file
 * (pyfastx_fasta_calc_composition, fasta.c:851-961) rides on the index scan, ONE read of the stream for both; a later
 * fx_fasta_comp / _shard / _sparse then only attributes the counts to the records and reads the bytes of record
 * boundaries again.  The counts are dropped by the next build or fx_set_shard. */
#define FX_BUILD_FULL_NAME 1
#define FX_BUILD_COMP 2
int fx_fasta_build(fx_handle *h, int full_name, fx_fasta_summary *out);

/* The same in two halves: _begin ENQUEUES the whole build on the handle's stream and returns; _end waits for it and
 * reports the totals.  Device-side consumers -- fx_fasta_fetch with FX_DEVICE arrays, fx_shard_summary_dev,
 * fx_fasta_stitch_dev -- may be enqueued between the two (they read the record count from device memory), so a
 * "build, then answer a batch" step costs one host synchronisation.  Calls that need host-side totals
 * (fx_fasta_table, fx_fasta_comp, ...) complete a pending build themselves. */
int fx_fasta_build_begin(fx_handle *h, int full_name);
int fx_fasta_build_end(fx_handle *h, fx_fasta_summary *out);

/* Copy the SoA record table to caller arrays (any pointer may be NULL).
 * Columns are exactly the .fxi `seq` columns (index.c:178-189) plus the
 * header-line offset and the name span inside the stream. */
int fx_fasta_table(fx_handle *h, int where,
                   int64_t *hoff, int64_t *boff, int64_t *blen, int64_t *slen,
                   int64_t *llen, int32_t *elen, int32_t *norm, int32_t *dlen,
                   int32_t *name_len);

/* Install the record table of an existing .fxi instead of scanning (pyfastx_load_index, index.c:391-429):
 * host arrays of the `seq` columns; afterwards fx_fasta_fetch works exactly as after fx_fasta_build.
 * (Composition and the shard summary still need a scan.) */
int fx_fasta_set_table(fx_handle *h, int64_t n, const int64_t *boff, const int64_t *blen, const int64_t *slen,
                       const int64_t *llen, const int32_t *elen, const int32_t *norm);

/* Which records may be sliced with the line arithmetic of pyfastx_sequence_subscript (sequence.c:498-510)?  `norm`
 * (index.c:342: at most ONE line of another length) is 1 both for a record whose last line is the short one and for a
 * record with one odd line in the middle -- where the arithmetic addresses the wrong bytes (the reference returns them
 * from a cold cache and the true slice from a warm one, sequence.c:100-110).  reg[i] = 1: every line of record i but
 * the last holds exactly llen - elen bases (decided by the scan / fx_fasta_set_table / the stitch from the row and ONE
 * byte of the stream: the byte in front of the last line is a newline).  fx_fasta_fetch slices the other records after
 * despacing them; so do all batched paths above it.  n_seq values, where = FX_HOST / FX_DEVICE. */
int fx_fasta_line_regular(fx_handle *h, int where, int32_t *reg);

/* pyfastx_fasta_calc_composition (fasta.c:851-961): comp[n_seq][128] counts of
 * every byte value < 128 on the sequence lines of each record ('\r' included,
 * '\n' excluded).  Needs fx_fasta_build first. */
int fx_fasta_comp(fx_handle *h, int where, int64_t *comp);
/* The same for one byte-range shard (fx_set_shard).  The bytes of a shard that precede its first header line belong
 * to a record whose header lies in an earlier shard: they are counted into lead[128] (host), from global offset
 * lead_from on -- the later of the shard's start and that record's boff, so that a header line crossing the cut is
 * left out (lead_from < 0: nothing is counted, e.g. shard 0).  The owner of the record adds the lead rows of the
 * following shards up to and including the first one that holds a header line (pyfastx_amd/shard.py).              */
int fx_fasta_comp_shard(fx_handle *h, int where, int64_t *comp, int64_t lead_from, int64_t *lead);
/* The same composition in the form the `comp` table stores it (fasta.c:904-914): only the non-zero bins, as triples
 * (seqid = record index + 1, abc = byte value, num = count) in record order, letters ascending -- the dense matrix
 * never leaves HBM (5 M records: 5 GB dense, ~50 M triples).  cap: room in seqid / abc / num (where = FX_HOST /
 * FX_DEVICE); *n_out: number of triples -- with FX_ERANGE when it exceeds cap (nothing is written then);
 * total[128] (host): column sums, the seqid = 0 rows of the table (fasta.c:943-950). */
int fx_fasta_comp_sparse(fx_handle *h, int where, int64_t cap, int64_t *seqid, int64_t *abc, int64_t *num,
                         int64_t *n_out, int64_t *total);

/* ------------------------------------------------------------ FASTQ index
 * Replaces pyfastx_fastq_create_index (fastq.c:89-171).                      */
typedef struct {
    int64_t n_reads;      /* stat.counts = line_num / 4                       */
    int64_t size;         /* stat.size   = sum of rlen                        */
    int64_t n_lines;
    int64_t n_bytes;
    int64_t first_id;     /* global 0-based id of this shard's first read (0 for a whole file) */
} fx_fastq_summary;

int fx_fastq_build(fx_handle *h, fx_fastq_summary *out);
/* The same with the composition counted ON THE WAY -- pyfastx_fastq_create_index (fastq.c:8-182) and
 * pyfastx_fastq_calc_composition (fastq.c:663-795), the reference's two passes over the file, in ONE read of the stream: the
 * count pass of the build classifies the bytes it holds in registers anyway; which line of four a byte belongs to is guessed
 * per run of granules from the '+' lines and checked against the newline prefixes afterwards.  A later fx_fastq_comp then
 * only hands the counts out; when any guess was wrong (or the file has what the stream form does not do: CRLF, bytes outside
 * '!'..127 in a quality line) it counts from the read table as if this had been fx_fastq_build.  Whole streams only. */
int fx_fastq_build_comp(fx_handle *h, fx_fastq_summary *out);
/* How the last fx_fastq_build_comp counted: *runs = runs of 64 KiB the stream was cut into, each counted on a GUESS of its line
 * phase (a '+' line of one byte, or '+' and '\r'); *recounted = runs whose guess the newline prefixes proved wrong or that had
 * none -- counted again from the prefixes (-1: too many of them, nothing of the one-read result was used); *one_read = 1 when
 * fx_fastq_comp answers from the build's counters, 0 when it reads the stream again through the read table (a quality byte
 * outside '!'..127, a '\r' that is not the end of its line: fastq.c:731-745's quirks are the table kernels').  The reference
 * has no counterpart (its loop fastq.c:715-753 is one pass of its own over the file). */
int fx_fastq_comp_info(fx_handle *h, int64_t *runs, int64_t *recounted, int *one_read);


/* Sharded FASTQ: records are short, so a shard carries a HALO -- the first
 * bytes of the next shard appended to its own range (fx_set_halo) -- and owns every record
 * whose header line STARTS in its core.  The only context it needs is the global line
 * numbering: phase 1 (fx_fastq_scan) reports the newlines of the core, ONE all-gather of
 * those two integers per rank gives every rank line_offset (newlines in earlier cores) and
 * prev_nl (offset of the last of them, -1 if none), phase 2 (fx_fastq_build_ctx) builds the
 * table.  Composition and fetch then work on the owned records.                           */
int fx_set_halo(fx_handle *h, int64_t halo_bytes);
int fx_fastq_scan(fx_handle *h, int64_t *n_nl_core, int64_t *last_nl_core);
int fx_fastq_build_ctx(fx_handle *h, int64_t line_offset, int64_t prev_nl, fx_fastq_summary *out);
int fx_fastq_table(fx_handle *h, int where,
                   int64_t *name_off, int32_t *name_len, int32_t *dlen,
                   int64_t *rlen, int64_t *soff, int64_t *qoff);

/* pyfastx_fastq_calc_composition (fastq.c:715-774): base = {A,C,G,T,N},
 * meta = {maxlen, minlen, minqs, maxqs, phred} in the .fxi column order. */
int fx_fastq_comp(fx_handle *h, int64_t base[5], int64_t meta[5]);

/* ------------------------------------------------------------------ fetch
 * Replaces pyfastx_index_fill_cache (index.c:694-707) + remove_space[_uppercase]
 * (util.c:166-194) + reverse/complement (util.c:239-269) for a BATCH of byte
 * ranges: query i reads blen[i] bytes at off[i], drops bytes 10/13/32, keeps
 * the first min(kept, slen[i]) bytes, applies flags, and writes them at
 * dst + dst_off[i].  out_len[i] (optional) receives the bytes written.
 * flags: per-call if flags_per_query == NULL, else flags_per_query[i].        */
int fx_fetch_ranges(fx_handle *h, int where, int64_t n,
                    const int64_t *off, const int64_t *blen, const int64_t *slen,
                    int flags, const uint8_t *flags_per_query,
                    uint8_t *dst, const int64_t *dst_off, int64_t *out_len);

/* The same with a slice taken AFTER despacing: of the bytes query i keeps, the first skip[i] are dropped and at most
 * take[i] stored -- pyfastx_sequence_get_subseq on a record that is not line-regular (sequence.c:100-110: the whole
 * record is despaced, then `seq + start - 1` is copied), without moving the record to the host. */
int fx_fetch_slices(fx_handle *h, int where, int64_t n,
                    const int64_t *off, const int64_t *blen, const int64_t *skip, const int64_t *take,
                    int flags, const uint8_t *flags_per_query,
                    uint8_t *dst, const int64_t *dst_off, int64_t *out_len);

/* The same for ONE range and a host buffer -- what a single getter of the reference does (pyfastx_index_fill_cache +
 * the copy of slen bytes, index.c:694-707, sequence.c:346-347; pyfastx_read_random_reader, read.c:37-45): descriptor
 * and result travel through pinned host memory, one launch and one wait per call.  skip / take as in FetchQ: the
 * first `skip` kept bytes are dropped, at most `take` are stored at dst; *out_len = bytes stored. */
int fx_fetch_one(fx_handle *h, int64_t off, int64_t blen, int64_t skip, int64_t take, int flags, uint8_t *dst, int64_t *out_len);

/* Same, but queries are (record id 0-based, start, stop) half-open 0-based
 * base coordinates resolved against the resident FASTA table with the
 * arithmetic of pyfastx_sequence_subscript (sequence.c:498-510) for norm=1
 * records and despace-then-slice (sequence.c:100-110) for norm=0 records. */
int fx_fasta_fetch(fx_handle *h, int where, int64_t n,
                   const int64_t *seq_id, const int64_t *start, const int64_t *stop,
                   int flags, const uint8_t *flags_per_query,
                   uint8_t *dst, const int64_t *dst_off, int64_t *out_len);

/* The same batch from host arrays with the layout left to the library -- the loop of the reference's benchmark
 * (benchmark/pyfastx_fasta_extract_subsequences.py:8-12: fa[name][s:e].seq per interval; pyfastx_sequence_subscript
 * sequence.c:412-517 + pyfastx_sequence_get_subseq sequence.c:76-125 per call) as ONE call: the intervals are checked on
 * the device against the resident table (first invalid one -> *first_bad, FX_ERANGE), the answers are laid out back to
 * back (offsets by a device scan) and come home by DMA into pinned memory of fx_pinned_alloc: *dst (the bytes) and
 * *dst_off (n + 1 offsets) belong to the caller, who gives them back with fx_pinned_free. */
int fx_fasta_fetch_alloc(fx_handle *h, int64_t n, const int64_t *seq_id, const int64_t *start, const int64_t *stop,
                         int flags, const uint8_t *flags_per_query, uint8_t **dst, int64_t **dst_off, int64_t *first_bad);
/* Where the last fx_*_fetch_alloc call of this thread spent its time on the host, in milliseconds (measurement aid): ms[0]
 * query arrays staged + uploads enqueued, [1] counts, scan, offsets back (first wait), [2] pinned blocks, [3] kernels
 * enqueued, [4] answers back (second wait), [5] the whole call. */
int fx_fetch_phases(double *ms, int cap);

/* ------------------------------------------------------------------ search
 * Extension (the reference answers only Sequence.search, sequence.c:519-558: the first hit in one record, str.find on a
 * host copy).  Every OVERLAPPING hit of one pattern of 1..64 letters in the `seq` of the records -- what fx_fasta_fetch
 * returns for the whole record: bytes 10/13/32 dropped, Py_TOUPPER'd under FX_SEARCH_UPPER, cut at slen -- two passes over
 * the resident stream and a device scan between them (pyfastx_amd/csrc/fx_search.hpp).  No hit crosses from one record
 * into the next.
 *   pat / rpat   the patterns of the + and of the - strand (plen letters each; rpat is the caller's reverse complement of
 *                pat: fx_revcomp for an exact pattern, the IUPAC complement for a degenerate one); either may be NULL when
 *                its strand is not asked for.
 *   mode         FX_SEARCH_PLUS / FX_SEARCH_MINUS: the strands; FX_SEARCH_UPPER: the text as Fasta(uppercase=True)
 *                presents it; FX_SEARCH_DEGENERATE: pattern letters are IUPAC codes (any case, U = T) and a text letter
 *                matches when it is an IUPAC letter whose base set lies inside the pattern letter's (other bytes match
 *                nothing).  Exact mode compares bytes.
 *   ids, n_ids   the records to search (0-based, ascending for file order; NULL: all of them).
 *   cap          room for hits.  *n_hits = the number of hits; above cap: FX_ERANGE and nothing is allocated.  cap = 0
 *                with counts != NULL: counts only.
 *   rec, start, strand   the hits, by (record, start), '+' before '-' at one start: record id, 0-based start of the
 *                occurrence on the forward strand (stop = start + plen) for both strands, '+' / '-'; pinned blocks of
 *                fx_pinned_alloc that belong to the caller (fx_pinned_free each).
 *   counts       optional host array [n_sel][2]: hits per searched record on + and on -.
 * Whole streams only: a byte-range shard (fx_set_shard, fx_open_file_range) gives FX_EINVAL. */
enum { FX_SEARCH_DEGENERATE = 1, FX_SEARCH_UPPER = 2, FX_SEARCH_PLUS = 4, FX_SEARCH_MINUS = 8 };
int fx_fasta_search(fx_handle *h, const uint8_t *pat, const uint8_t *rpat, int32_t plen, int mode, const int64_t *ids, int64_t n_ids,
                    int64_t cap, int64_t **rec, int64_t **start, uint8_t **strand, int64_t *n_hits, int64_t *counts);

/* ------------------------------------------------------------------ search with mismatches
 * Extension.  Every window of plen letters of the `seq` of the records -- the text fx_fasta_search walks, with its rules:
 * bytes 10/13/32 dropped, windows across line ends and never across records, cut at slen -- that MISMATCHES the pattern at
 * no more than max_mismatch positions (Hamming distance: substitutions only, no insertion or deletion), with its distance
 * (pyfastx_amd/csrc/fx_search_approx.hpp: Shift-And with max_mismatch + 1 state words).  A position mismatches exactly
 * when fx_fasta_search would not match there under the same mode, so max_mismatch = 0 gives fx_fasta_search's hits, row
 * for row.
 *   pat, rpat, plen, mode, ids, n_ids, cap, rec, start, strand, n_hits, counts: as for fx_fasta_search.
 *   max_mismatch 0..min(8, plen - 1).
 *   anchor       bit j set: letter j of pat must not mismatch (a PAM, a primer's 3' end); given for pat, the library mirrors
 *                it for rpat (letter j of pat is letter plen - 1 - j of rpat).  0: no anchor.
 *   mismatch     a fourth array beside rec / start / strand: the distance of every hit, 0..max_mismatch.
 * FX_EINVAL: plen outside 1..64, max_mismatch outside its range, an anchor bit at or above plen (these three are refused
 * before the handle is looked at), no strand, a null pattern of a strand asked for, a byte-range shard.  FX_ESTATE: no
 * table built.  FX_ERANGE: more than cap hits, *n_hits = their number, nothing allocated. */
int fx_fasta_search_approx(fx_handle *h, const uint8_t *pat, const uint8_t *rpat, int32_t plen, int mode, int32_t max_mismatch,
                           uint64_t anchor, const int64_t *ids, int64_t n_ids, int64_t cap, int64_t **rec, int64_t **start,
                           uint8_t **strand, uint8_t **mismatch, int64_t *n_hits, int64_t *counts);

/* ------------------------------------------------------------------ search with insertions and deletions
 * Extension (nearest reference function: Sequence.search, sequence.c:519-558, exact and first hit only).  Every place in the
 * `seq` of the records -- the text fx_fasta_search walks, with its rules: bytes 10/13/32 dropped, across line ends and never
 * across records, cut at slen -- where the pattern ENDS within max_edits edits (Levenshtein distance: a substituted, an
 * inserted and a deleted letter cost 1 each), with its distance and the start of its shortest span
 * (pyfastx_amd/csrc/fx_search_edit.hpp: Myers' bit-vector column per strand).  A text letter matches a pattern letter
 * exactly where fx_fasta_search would match it under the same mode.
 *   pat, rpat, plen, mode, ids, n_ids, strand, counts: as for fx_fasta_search.
 *   max_edits    0..min(8, plen - 1).
 *   Ends         letter e of a record is an end on a strand when D[e], the least distance between that strand's pattern and
 *                any stretch of the text that ends with letter e, is at most max_edits.
 *   Rows         one per reported end: stop = e + 1, edits = D[e], start = stop - m for the smallest m such that the last m
 *                letters up to e are at distance D[e] (so plen - max_edits <= stop - start <= plen + max_edits); by
 *                (record, stop), '+' before '-' at one stop; starts are not monotone.
 *   report       FX_EDIT_ALL: every end (with max_edits = 0: fx_fasta_search's hits, row for row).  FX_EDIT_BEST: per record
 *                and strand the ends e such that e - 1 is no end or D[e-1] > D[e], and e + 1 is no end or D[e+1] >= D[e]:
 *                the leftmost minimum of every dip, at least one per stretch of consecutive ends.
 *   rec, start, stop, strand, edits   the rows: pinned blocks of fx_pinned_alloc that belong to the caller (fx_pinned_free
 *                each); edits is uint8, 0..max_edits.
 *   n_hits, n_ends   *n_hits = the rows `report` gives, *n_ends = the ends in front of the filter (equal under FX_EDIT_ALL).
 *   cap          room for ENDS, since every end is held on the device before the filter: *n_ends above cap gives FX_ERANGE
 *                and nothing is allocated, however few rows FX_EDIT_BEST would keep.  cap = 0 with counts != NULL: counts
 *                only -- the rows `report` would give per searched record on + and on -; no start is computed and no row
 *                comes home.
 * FX_EINVAL: plen outside 1..64, max_edits outside its range, an unknown report (these three are refused before the handle is
 * looked at), no strand, a null pattern of a strand asked for, a null output, a byte-range shard.  FX_ESTATE: no table built.
 * FX_ERANGE: more than cap ends. */
enum { FX_EDIT_ALL = 0, FX_EDIT_BEST = 1 };
int fx_fasta_search_edit(fx_handle *h, const uint8_t *pat, const uint8_t *rpat, int32_t plen, int mode, int32_t max_edits,
                         int32_t report, const int64_t *ids, int64_t n_ids, int64_t cap, int64_t **rec, int64_t **start,
                         int64_t **stop, uint8_t **strand, uint8_t **edits, int64_t *n_hits, int64_t *n_ends, int64_t *counts);

/* ------------------------------------------------------------------ position weight matrices
 * Extension.  Every window of plen letters of the `seq` of the records -- the text fx_fasta_search walks, with its rules:
 * bytes 10/13/32 dropped, windows across line ends and never across records, cut at slen -- whose SCORE under one position
 * weight matrix is at least min_score, on one or both strands, with its score; and the best-scoring window of every record
 * (pyfastx_amd/csrc/fx_pwm.hpp: a 2-bit history per lane, score tables of four letters at a time in LDS).
 *   Letters      A C G T in either case and U / u (= T) are the columns 0..3.  Every other kept byte (N, IUPAC codes, '*',
 *                '-', ...) makes every window that holds it unscorable: no hit, no part in a best score.
 *   mat, plen    int32 [plen][4], row j = position j of the motif, columns A C G T; 1 <= plen <= 64, every entry in
 *                -32767..32767.  All scores are exact integers, below 2^21 in size.
 *   Scores       '+': sum_j mat[j][x[start + j]].  '-': the score of the window's reverse complement under the same matrix,
 *                sum_j mat[plen - 1 - j][3 - x[start + j]] (the library derives the reverse matrix).  start is the 0-based
 *                start on the forward strand for both strands, stop = start + plen.
 *   mode         FX_SEARCH_PLUS | FX_SEARCH_MINUS, nothing else.
 *   fx_fasta_pwm_scan   the windows with score >= min_score, by (record, start), '+' before '-' at one start.  ids, n_ids,
 *                cap, rec, start, strand, n_hits, counts: as for fx_fasta_search; score: a fourth pinned block beside rec /
 *                start / strand, the int32 score of every hit.
 *   fx_fasta_pwm_best   per searched record k (ids in any order; NULL: all) and strand s (0 '+', 1 '-'): best_score[2k + s]
 *                the largest score of a scorable window, best_start[2k + s] the smallest start that has it.  A record without
 *                a scorable window, and a strand that was not asked for, get INT32_MIN and -1.  Host arrays of the caller.
 * FX_EINVAL: plen outside 1..64, a null matrix, an entry outside -32767..32767, a mode bit other than the two strands, no
 * strand (these are refused before the handle is looked at), a null output, a byte-range shard.  FX_ESTATE: no table built.
 * FX_ERANGE: more than cap hits, *n_hits = their number, nothing allocated. */
int fx_fasta_pwm_scan(fx_handle *h, const int32_t *mat, int32_t plen, int mode, int32_t min_score, const int64_t *ids, int64_t n_ids,
                      int64_t cap, int64_t **rec, int64_t **start, uint8_t **strand, int32_t **score, int64_t *n_hits,
                      int64_t *counts);
int fx_fasta_pwm_best(fx_handle *h, const int32_t *mat, int32_t plen, int mode, const int64_t *ids, int64_t n_ids, int32_t *best_score,
                      int64_t *best_start);

/* ------------------------------------------------------------------ minimizers
 * Extension (the reference has no counterpart: it has no k-mer of any kind).  The (w, k) minimizers of the `seq` of the
 * records: of every w consecutive k-mers the smallest, each distinct choice once -- the sampling step in front of seeding,
 * overlap and containment indexes, k-mer bucketing and sketching (pyfastx_amd/csrc/fx_minimizer.hpp: the 64-bit rolling code
 * of the k-mer tables, a ring of the last w keys per lane in LDS, the passes of fx_fasta_search).
 *   Sequence     the text fx_fasta_search walks, with its rules: bytes 10/13/32 dropped, windows across line ends and never
 *                across records, cut at slen.  No upper-casing plays a part.
 *   k-mers       1 <= k <= 31.  Position p (0 <= p <= slen - k) holds the k-mer seq[p .. p + k).  It is VALID when all its
 *                letters are ACGTacgt (U, N, IUPAC codes and every other byte are not).  fw: its base-4 code, A = 0 C = 1 G = 2
 *                T = 3, first letter most significant; rc: the code of its reverse complement.  With FX_MZ_CANONICAL
 *                code = min(fw, rc) and the strand is '+' when fw <= rc (a k-mer that is its own reverse complement is '+'),
 *                '-' otherwise; without it code = fw and the strand is '+'.
 *   Order        FX_MZ_LEX: key = code.  Otherwise key = mix(code), with m = 4^k - 1 and unsigned 64-bit arithmetic:
 *                    x = (~x + (x << 21)) & m;  x ^= x >> 24
 *                    x = (x + (x << 3) + (x << 8)) & m;  x ^= x >> 14
 *                    x = (x + (x << 2) + (x << 4)) & m;  x ^= x >> 28
 *                    x = (x + (x << 31)) & m
 *                a bijection of the 2k-bit words for every k, so equal keys mean equal codes.
 *   Windows      1 <= w <= 32.  Window j (0 <= j <= slen - k - w + 1) holds the positions j .. j + w - 1.  Its SELECTION is
 *                the leftmost position with the smallest key among its valid k-mers; a window without a valid k-mer has none.
 *                A record shorter than w + k - 1 letters has no window and gives no row.
 *   Rows         the distinct selections of all windows of a record, each as (record, start = position, strand, code), by
 *                (record, start).  Selections never move left as j grows, so the rows are exactly the windows whose selection
 *                exists and differs from that of window j - 1.
 *   ids, n_ids, cap, rec, start, strand, n_hits, counts: as for fx_fasta_search (counts: rows per searched record on '+' and
 *                on '-'; cap = 0 with counts != NULL: counts only); code: a fourth pinned block beside rec / start / strand, the
 *                uint64 code of every row (stop = start + k).
 * FX_EINVAL: k outside 1..31, w outside 1..32, a flag bit other than the two (these are refused before the handle is looked
 * at), a null output, a byte-range shard (no halo).  FX_ESTATE: no table built.  FX_ERANGE: more than cap rows, *n_hits =
 * their number, nothing allocated. */
enum { FX_MZ_CANONICAL = 1, FX_MZ_LEX = 2 };
int fx_fasta_minimizers(fx_handle *h, int32_t k, int32_t w, int flags, const int64_t *ids, int64_t n_ids, int64_t cap, int64_t **rec,
                        int64_t **start, uint8_t **strand, uint64_t **code, int64_t *n_hits, int64_t *counts);

/* ------------------------------------------------------------------ regions, windows, class runs
 * Composition of intervals of the records, and the maximal runs of a letter class (pyfastx_amd/csrc/fx_annot.hpp).  The text
 * of a record is the one fx_fasta_search walks: the bytes of [boff, boff + blen) with 10 / 13 / 32 dropped, cut at slen; the
 * file's own bytes are classified (no upper-casing).  Coordinates are 0-based half-open positions in that text.
 * Seven int64 columns, in this order: A C G T N other masked.  A counts 'A' and 'a', and so for C G T N; other is every other
 * kept byte (IUPAC codes, 'U' and 'u' -- U is not T here, as Sequence.gc_content counts A C G T only --, '*', '-', bytes
 * >= 128); the first six sum to the interval's length; masked counts the kept bytes in 'a'..'z' and overlaps the first six.
 * All of them rest on the RANK INDEX of the handle: per 256-byte run of the fx_fasta_search layout over all records, the
 * exclusive prefixes of the kept bytes and of the seven columns (eight int64: a quarter of the stream's size in device
 * memory, blocks of the scratch pool).
 *   fx_fasta_rank_build   builds it (one pass over the stream and a scan); a second call does nothing.  Every entry below
 *                builds it when it is not there.  A new table (fx_fasta_build*, fx_fasta_set_table, fx_fasta_set_row) or
 *                shard context makes it invalid; fx_close gives its memory back.
 *   fx_fasta_rank_free    gives its memory back now; the next entry builds it again.
 * Whole streams only: a byte-range shard gives FX_EINVAL.  FX_ESTATE: no table built.  Without a device every entry returns
 * FX_EDEVICE before it looks at an argument.
 *
 * fx_fasta_region_counts replaces slicing and counting on the host, one interval at a time (Sequence.composition,
 * gc_content, gc_skew of fa[name][a:b]: sequence.c:562-749): counts[i * 7 + c] = column c of [start[i], stop[i]) of record
 * seq_id[i].  Per query two binary searches over the index and at most two runs (512 bytes) of the stream are read,
 * whatever the interval's length.  where = FX_HOST: the four arrays are host memory; FX_DEVICE: device memory, and the
 * call returns when the kernel has run.  Ids and intervals are checked on the device, as fx_fasta_fetch_alloc checks them:
 * an id outside the table, start < 0, stop < start or stop > slen: FX_ERANGE and *first_bad = the first such query (counts
 * then hold nothing of use).  An empty interval is valid and gives zeros.
 *
 * fx_fasta_window_counts (extension; the reference has no windows): for every selected record (ids: 0-based, any order,
 * NULL: all) the windows [j * step, min(j * step + window, slen)) for every j >= 0 with j * step < slen -- with partial = 0
 * only those with j * step + window <= slen --, laid out by record (in the order of ids), then by j; made on the device from
 * a scan of the per-record window counts and answered as regions.  *n = their number; above max_windows: FX_ERANGE and
 * nothing is allocated.  rec, start, stop (n each) and counts (n * 7): pinned blocks of fx_pinned_alloc that belong to the
 * caller (fx_pinned_free each).  window < 1, step < 1, max_windows < 0: FX_EINVAL.
 *
 * fx_fasta_class_runs (extension): every MAXIMAL interval of the text of the selected records whose letters all lie in a set
 * of byte values and whose length is at least min_len (>= 1), as (record, start, stop) rows ordered by the position of the
 * record in ids (NULL: all), then by start -- no sort, no atomic.  set32: 256 bits, bit (c & 7) of byte (c >> 3) = byte value
 * c is in the set.  An interval may span any number of runs, begin at 0 or end at slen; it never joins across two records.
 * Kept bytes behind slen are not looked at: an interval that reaches the cut ends at slen.  *n_total = the number of such
 * intervals; above max_runs: FX_ERANGE, *n = 0 and nothing is allocated; else *n = *n_total rows in pinned blocks as above. */
int fx_fasta_rank_build(fx_handle *h);
int fx_fasta_rank_free(fx_handle *h);
int fx_fasta_region_counts(fx_handle *h, int where, int64_t n, const int64_t *seq_id, const int64_t *start, const int64_t *stop,
                           int64_t *counts, int64_t *first_bad);
int fx_fasta_window_counts(fx_handle *h, const int64_t *ids, int64_t n_ids, int64_t window, int64_t step, int partial,
                           int64_t max_windows, int64_t **rec, int64_t **start, int64_t **stop, int64_t **counts, int64_t *n);
int fx_fasta_class_runs(fx_handle *h, const uint8_t *set32, int64_t min_len, const int64_t *ids, int64_t n_ids, int64_t max_runs,
                        int64_t **rec, int64_t **start, int64_t **stop, int64_t *n, int64_t *n_total);

/* ------------------------------------------------------------------ low-complexity sequence (DUST triplet score; extension)
 * The mask people run before a search, a k-mer count or a sketch, and the low-complexity read filter
 * (pyfastx_amd/csrc/fx_dust.hpp).  The reference has no such call.
 *   Text and letters.  The text of a record and its coordinates are those of fx_fasta_class_runs: the kept bytes (10 / 13 / 32
 *   dropped), cut at slen, 0-based, half-open.  Letters fold as in the k-mer entries: A a = 0, C c = 1, G g = 2, T t = 3;
 *   every other kept byte (N, IUPAC codes, U, ...) is INVALID.  Soft-masked sequence therefore scores like upper case.
 *
 * fx_fasta_low_complexity: WINDOWED DUST.  window W in 4..64 letters; threshold T in 1..1000, in tenths as sdust and
 * dustmasker write it (20 means a score of 2.0); min_len >= 1.  Per record of text length L:
 *   - a triplet at position p is valid when t[p], t[p + 1], t[p + 2] are all valid; its code 16 a + 4 b + c is 0..63;
 *   - for every e in 2..L - 1 the window that ends at e holds the letters [max(0, e - W + 1), e]: windows at a record's start
 *     are shorter than W, and a record shorter than W is scored by these alone;
 *   - c_x = the number of valid triplets of code x that lie wholly inside the window, n = sum c_x,
 *     S = sum c_x (c_x - 1) / 2;
 *   - the window QUALIFIES iff n >= 2 and 10 S > T (n - 1) -- all integers, S <= 1891;
 *   - a triplet that holds an invalid letter is not counted; the window still spans W letters.
 * The masked set of the record is the union of [max(0, e - W + 1), e + 1) over its qualifying e; the rows are the maximal
 * intervals of that union (touching intervals are one row); rows shorter than min_len are dropped after the merge.  Rows are
 * ordered by the position of the record in ids (NULL: all; any order), then by start -- no sort, no atomic.  Nothing joins
 * across two records, no count or letter of one record reaches the next, a window of only N never qualifies.
 * This is the windowed form: a whole window is masked, so flanks of up to W minus about 23 letters go with a repeat at W = 64,
 * T = 20; a smaller window is the finer knob.  sdust's "perfect intervals" are not implemented and parity with sdust /
 * dustmasker is not claimed.
 * *n_total = the number of rows; above max_rows: FX_ERANGE, *n = 0 and nothing is allocated; else *n = *n_total rows in
 * pinned blocks of fx_pinned_alloc that belong to the caller (fx_pinned_free each), never NULL after FX_OK, even for 0 rows.
 * Builds the rank index when it is not there.  Without a device FX_EDEVICE before any argument is looked at.  FX_EINVAL: a
 * null handle or output pointer, window outside 4..64, threshold outside 1..1000, min_len < 1, max_rows < 0, a count of ids
 * without its array, a byte-range shard.  FX_ESTATE: no table built.  An id outside the table: FX_ERANGE.
 *
 * fx_fastq_complexity: per query, for s = seq[start:end] of read ids[q] (ids, n_ids, start, end, *first_bad exactly as
 * fx_fastq_kmers takes them: ids NULL = every read, any order, repeats allowed; start / end both NULL = whole reads):
 *   length[q]      end - start (int64);
 *   n_triplets[q]  the number of valid triplets of s (int32);
 *   dust_sum[q]    sum c_x (c_x - 1) / 2 over the triplet codes of the whole interval (int64; a read of any length, no counter
 *                  wraps below 2^32 letters);
 *   n_diff[q]      the number of j with raw byte s[j] != s[j + 1] (int32): fastp's complexity numerator.
 * The callers derive dust = 10 dust_sum / (n_triplets - 1) (0 when n_triplets < 2; prinseq's scale without its window
 * averaging) and complexity = n_diff / (length - 1).  One row per query, *n_rows of them, in pinned blocks as above.  Without
 * a device FX_EDEVICE before any argument is looked at.  FX_EINVAL: a null handle or output pointer, start without end, a
 * negative id count, a byte-range shard.  FX_ESTATE: before fx_fastq_build.  An id outside the table, or an interval outside
 * 0 <= start <= end <= rlen: *first_bad = its position among the queries, FX_ERANGE, nothing allocated. */
int fx_fasta_low_complexity(fx_handle *h, int32_t window, int32_t threshold, int64_t min_len, const int64_t *ids, int64_t n_ids,
                            int64_t max_rows, int64_t **rec, int64_t **start, int64_t **stop, int64_t *n, int64_t *n_total);
int fx_fastq_complexity(fx_handle *h, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end, int64_t **length,
                        int32_t **n_triplets, int64_t **dust_sum, int32_t **n_diff, int64_t *n_rows, int64_t *first_bad);

/* ------------------------------------------------------------------ tandem repeats
 * fx_fasta_tandem_repeats (extension; the reference has no repeat search): the perfect tandem repeats (microsatellites) of
 * period 1..8 of the selected records (pyfastx_amd/csrc/fx_tandem.hpp).  The text and the coordinates are those of the section
 * above.  Letters are folded: A a = 0, C c = 1, G g = 2, T t = 3; every other kept byte (N, IUPAC codes, U, '*', '-', bytes
 * >= 128) is INVALID and matches nothing, itself included; soft-masked repeats are found like any other.  A repeat of period
 * p is a maximal interval [a, b) of the text of one record for which
 *   - every letter is valid,
 *   - code(t[j]) == code(t[j - p]) for every j in [a + p, b), and neither a - 1 nor b can join (maximal),
 *   - b - a >= 2 p and b - a >= max(p * min_copies[p - 1], min_len),
 *   - the motif t[a : a + p] is primitive -- not a shorter word written several times; equivalently p is the smallest period
 *     of [a, b): ATATAT is a repeat of period 2 only, AAAAAA of period 1 only.
 * Repeats of different periods may overlap and all are reported: these are the maximal repetitions of stringology with a
 * bounded period, not a greedy left-to-right scan whose answer depends on where the scan stands.
 *   min_copies   max_period entries; min_copies[p - 1] is the threshold of period p, 0: period p is not searched.
 *   max_period   1..8.
 *   min_len      >= 0; a further lower bound on b - a for every period.
 *   ids, n_ids   0-based record ids, any order (NULL: all records in file order).
 *   rec, start, stop, period, motif   one row per repeat, ordered by the position of the record in ids, then by stop, then by
 *                period -- the order in which one left-to-right walk closes them; no sort, no atomic.  motif is the 2-bit
 *                code of t[a : a + p], first letter most significant.  Pinned blocks of fx_pinned_alloc that belong to the
 *                caller (fx_pinned_free each), never NULL after FX_OK, even for 0 rows.
 *   *n_total     the number of repeats; above max_rows: FX_ERANGE, *n = 0 and nothing is allocated; else *n = *n_total.
 * A repeat may span any number of runs, begin at 0 or end at slen; it never joins across two records.  Builds the rank index
 * when it is not there.  Without a device FX_EDEVICE before any argument is looked at.  FX_EINVAL: a null handle or output
 * pointer, max_period outside 1..8, an entry of min_copies that is 1 or negative, no period searched, min_len < 0,
 * max_rows < 0, a byte-range shard.  FX_ESTATE: no table built. */
int fx_fasta_tandem_repeats(fx_handle *h, const int32_t *min_copies, int32_t max_period, int64_t min_len, const int64_t *ids,
                            int64_t n_ids, int64_t max_rows, int64_t **rec, int64_t **start, int64_t **stop, uint8_t **period,
                            uint32_t **motif, int64_t *n, int64_t *n_total);

/* ------------------------------------------------------------------ open reading frames, translation
 * fx_fasta_orfs (extension; the reference reads no codon): the open reading frames of the selected records in all six frames
 * (pyfastx_amd/csrc/fx_orf.hpp).  The text and the coordinates (0-based, half-open) are those of the sections above; letters
 * fold as for the tandem repeats: A a = 0, C c = 1, G g = 2, T t = 3, every other kept byte (N, IUPAC codes, U, '*', '-',
 * bytes >= 128) is INVALID.
 *   Genetic code.  stop_mask and start_mask have one bit per codon, indexed 16 c0 + 4 c1 + c2 in that letter code; a codon in
 *   both masks is a stop.  On the reverse strand the codon that occupies the forward positions [j, j + 3) is read as its
 *   reverse complement: index 16 (3 - c2) + 4 (3 - c1) + (3 - c0).
 *   Codon classes.  A codon with an invalid letter is invalid; otherwise it is STOP, START or OTHER by the masks.  A BREAK is
 *   a STOP or an invalid codon.
 *   Frames and segments.  For each strand and residue class c in {0, 1, 2} the codons are those at j = c (mod 3) with 0 <= j
 *   and j + 3 <= slen.  A segment is a maximal run of consecutive codons of one class that are no breaks: its left end is c
 *   or the end of a break codon, its right end the start of the next break codon or the end of the last full codon of the
 *   class.  Empty segments give nothing.  A segment never joins across two records; it may span any number of runs.
 *   mode         0 (stop to stop): the row is the segment [a, b).  1: the row is [s, b), s the first START codon of the
 *                segment; a segment without one gives no row.
 *   min_len      a row is kept when it has at least max(min_len, 3) letters.  The stop codon that ends an ORF is never
 *                inside [start, stop).
 *   strands      1 forward, 2 reverse, 3 both.  The reverse strand follows the same rules on the reverse complement of the
 *                text; a row [s, e) found there is reported as [slen - e, slen - s).  In a left-to-right walk of the forward
 *                text a reverse segment opens behind a reverse-strand break on its left and closes at the break on its right,
 *                and in mode 1 its row ends at the LAST reverse START codon in front of that break.
 *   ids, n_ids   0-based record ids, any order (NULL: all records in file order).
 *   rec, start, stop (int64), frame (int8), flags (uint8)   one row per ORF.  frame: forward +1 + start % 3, reverse
 *                -(1 + (slen - stop) % 3).  flags, in the ORF's own orientation: bit 0 a STOP codon follows the 3' end (not
 *                set when an invalid codon or the end of the text ends it), bit 1 a STOP codon precedes the segment at its 5'
 *                end (not set for an invalid codon or the record's edge), bit 2 the first codon of the row is a START codon
 *                (always in mode 1).  Ordered by the position of the record in ids, then by the forward coordinate at which
 *                a left-to-right walk closes the row's segment (a forward row's stop; for a reverse row the forward right end
 *                of its segment), then forward before reverse -- no sort, no atomic.  Pinned blocks of fx_pinned_alloc that
 *                belong to the caller (fx_pinned_free each), never NULL after FX_OK, even for 0 rows.
 *   *n_total     the number of rows; above max_rows: FX_ERANGE, *n = 0 and nothing is allocated; else *n = *n_total.
 * Builds the rank index when it is not there.  Without a device FX_EDEVICE before any argument is looked at.  FX_EINVAL: a
 * null handle or output pointer, mode or strands outside its range, stop_mask == 0, mode 1 with start_mask & ~stop_mask == 0,
 * min_len < 0, max_rows < 0, a byte-range shard.  FX_ESTATE: no table built. */
int fx_fasta_orfs(fx_handle *h, uint64_t stop_mask, uint64_t start_mask, int mode, int strands, int64_t min_len, const int64_t *ids,
                  int64_t n_ids, int64_t max_rows, int64_t **rec, int64_t **start, int64_t **stop, int8_t **frame, uint8_t **flags,
                  int64_t *n, int64_t *n_total);
/* fx_fasta_translate_alloc (extension): table translation of a batch of intervals, shaped like fx_fasta_fetch_alloc above.
 * Query i is the interval [start[i], stop[i]) of the text of record seq_id[i]; with strand[i] != 0 its reverse complement
 * (strand NULL: all forward).  Amino acid k of a query is aa64[16 c0 + 4 c1 + c2] of its letters 3 k .. 3 k + 2 in the letter
 * code above; a codon with an invalid letter gives `unknown`.  A query yields (stop - start) / 3 amino acids, one or two
 * trailing letters are ignored; no codon is rewritten to M.  The intervals are checked on the device as fx_fasta_fetch_alloc
 * checks them (first invalid one -> *first_bad, FX_ERANGE); *dst (the amino acids back to back) and *dst_off (n + 1 offsets)
 * are pinned blocks that belong to the caller, never NULL after FX_OK.  Without a device FX_EDEVICE before any argument is
 * looked at.  FX_EINVAL: a null handle, table, query array or output pointer, n < 0, a byte-range shard.  FX_ESTATE: no table
 * built. */
int fx_fasta_translate_alloc(fx_handle *h, int64_t n, const int64_t *seq_id, const int64_t *start, const int64_t *stop,
                             const uint8_t *strand, const uint8_t *aa64, uint8_t unknown, uint8_t **dst, int64_t **dst_off,
                             int64_t *first_bad);

/* FASTQ reads by 0-based id (read.c:37-45, 152-167, 237-278): seq and qual
 * are rlen bytes each at dst_off[i]; quali = qual - phred as int8
 * (phred 0 -> 33, read.c:268).  Any of seq/qual/quali may be NULL. */
int fx_fastq_fetch(fx_handle *h, int where, int64_t n, const int64_t *read_id,
                   int phred, int seq_flags,
                   uint8_t *seq, uint8_t *qual, int8_t *quali, const int64_t *dst_off);
/* ... with the layout left to the library (fq[i].seq / .qual / .quali for many i, read.c:152-167, 237-278): read lengths
 * are gathered and scanned on the device, the wanted outputs (want: bit 0 seq, 1 qual, 2 quali) and *dst_off (n + 1)
 * come back in pinned memory of fx_pinned_alloc (fx_pinned_free each); an id outside the table -> *first_bad, FX_ERANGE. */
int fx_fastq_fetch_alloc(fx_handle *h, int64_t n, const int64_t *read_id, int phred, int seq_flags, int want,
                         uint8_t **seq, uint8_t **qual, int8_t **quali, int64_t **dst_off, int64_t *first_bad);

/* ------------------------------------------------------------------ FASTQ quality control
 * Extension (the reference answers whole-file questions only: composition, the quality range, the length range,
 * fastq.c:715-753).  Three passes over the resident stream and its read table (pyfastx_amd/csrc/fx_fastq_qc.hpp).  For read i
 * they look at the rlen bytes s at soff and the rlen bytes q at qoff -- what fx_fastq_fetch returns as seq and qual, a byte
 * past the end of the stream reads as 0 -- and at nothing else; q[j] is an unsigned byte and p = phred (0 -> 33, read.c:268;
 * 0..255).  Base classes are the composition's: upper-case A C G T, every other byte of s is "other".  All results are
 * integers.  Whole streams only: a byte-range shard (fx_set_shard, fx_open_file_range) gives FX_EINVAL; before
 * fx_fastq_build: FX_ESTATE; a null handle or output pointer: FX_EINVAL, nothing touched.  Every output is a pinned block
 * of fx_pinned_alloc that belongs to the caller (fx_pinned_free each; never NULL after FX_OK, even for 0 rows).
 *
 * fx_fastq_read_stats: one row per read, in the order of ids (0-based, any order, repeats allowed; ids = NULL: every read in
 *   read order, n_ids ignored).  length = rlen; qsum = sum of q[j] - p; qmin / qmax = the smallest / largest q[j] - p (0 for
 *   an empty read); n_low = bytes with q[j] - p < low_qual (0..255); n_gc = G and C in s; n_other = bytes of s outside A C G T.
 *   *n_rows = the number of rows.  An id outside the table: *first_bad = its position in ids, FX_ERANGE, nothing allocated. */
int fx_fastq_read_stats(fx_handle *h, const int64_t *ids, int64_t n_ids, int phred, int low_qual, int64_t **length, int64_t **qsum,
                        int16_t **qmin, int16_t **qmax, int32_t **n_low, int32_t **n_gc, int32_t **n_other, int64_t *n_rows,
                        int64_t *first_bad);
/* fx_fastq_cycle_hist: per position j < cycles (1..65536) over all reads with rlen > j: qual[j][b] (cycles x 256) = reads
 *   whose RAW quality byte q[j] is b; base[j][c] (cycles x 5) = reads whose s[j] is A, C, G, T, other; depth[j] = reads with
 *   rlen > j.  Positions at or beyond `cycles` are not counted; rows beyond the longest read are zero. */
int fx_fastq_cycle_hist(fx_handle *h, int32_t cycles, int64_t **qual, int64_t **base, int64_t **depth);
/* fx_fastq_select: the ascending 0-based ids of the reads that pass every criterion asked for -- min_len <= rlen (min_len
 *   < 0: not asked), rlen <= max_len (< 0: not asked), qsum * mq_den >= mq_num * rlen (mean quality >= mq_num / mq_den;
 *   mq_den = 0: not asked), n_low * lf_den <= lf_num * rlen (fraction of bytes below low_qual <= lf_num / lf_den; lf_den =
 *   0: not asked), n_other <= max_other (< 0: not asked) -- in int64, so an empty read passes both ratio tests.  Numerators
 *   and denominators within 0..10^9.  Predicate, count, scan and emit run on the device; only the ids come to the host.
 *   *n_ids = how many; they are what fx_fastq_fetch_alloc takes. */
int fx_fastq_select(fx_handle *h, int phred, int low_qual, int64_t min_len, int64_t max_len, int64_t mq_num, int64_t mq_den,
                    int64_t lf_num, int64_t lf_den, int64_t max_other, int64_t **ids, int64_t *n_ids);

/* ------------------------------------------------------------------ FASTQ trimming and trimmed records (extension)
 * The reference has no counterpart: it trims nothing and writes verbatim copies only (Read.raw, read.c:124-150).  s, q, L =
 * rlen and d[j] = q[j] - p as for the quality-control entries above (a byte past the end of the stream reads as 0); states
 * and errors as theirs (null handle / output: FX_EINVAL; before fx_fastq_build: FX_ESTATE; a byte-range shard: FX_EINVAL; an
 * id outside the table: *first_bad = its position, FX_ERANGE, nothing allocated); outputs are pinned blocks of
 * fx_pinned_alloc that belong to the caller, never NULL after FX_OK.
 *
 * fx_fastq_trim: per read (in the order of ids; ids = NULL: every read) the interval [start, end) that survives these steps,
 *   run in this order, each on what the one before left (a = start, b = end; always 0 <= a <= b <= L):
 *   1 fixed clip      a = min(clip_front, L); b = max(a, L - clip_tail)                                (both >= 0)
 *   2 3' adapter      adapter = NULL: not asked.  adapter_len 1..64 letters of A C G T N (upper case; N matches any byte),
 *                     1 <= min_overlap <= adapter_len.  For j = a, a + 1, ...: m = min(adapter_len, b - j); stop when m <
 *                     min_overlap; mm = the k < m with adapter[k] != 'N' and s[j + k] != adapter[k] (read bytes as they
 *                     are: lower case, N, IUPAC codes mismatch); the FIRST j with mm * err_den <= err_num * m: b = j.
 *   3 5' quality      front_qual < 0: not asked (else 0..255).  While a < b and d[a] < front_qual: a += 1.
 *   4 sliding window  win_len = 0: not asked.  If b > a: we = min(win_len, b - a); the first j in [a, b - we] with
 *                     (d[j] + ... + d[j + we - 1]) * win_den < win_num * we: b = j.
 *   5 3' quality      tail_qual < 0: not asked (else 0..255).  While b > a and d[b - 1] < tail_qual: b -= 1.
 *   Ratios within 0..10^9, denominators >= 1.  *n_rows = the number of rows.
 * fx_fastq_format_alloc: the four-line records of the queries, back to back: H "\n" s[a:b] "\n+\n" q[a:b] "\n", H = the dlen
 *   bytes at soff - dlen - 1 (they begin with '@') without one trailing '\r'; bytes are copied as they are.  start = end =
 *   NULL: whole reads (a = 0, b = L); else row k of both belongs to query k (what fx_fastq_trim returned for the same
 *   ids), and an interval outside 0 <= start <= end <= rlen gives *first_bad = the first such query, FX_ERANGE, nothing
 *   allocated.  A query with b - a < min_len (>= 0) produces no bytes.  Record k is dst[dst_off[k] .. dst_off[k + 1]);
 *   dst_off has *n_rows + 1 entries, *n_kept = the records that produced bytes.  Sizes, offsets and bytes are made on the
 *   device; only the finished bytes and the offsets come to the host. */
int fx_fastq_trim(fx_handle *h, const int64_t *ids, int64_t n_ids, int phred, int64_t clip_front, int64_t clip_tail,
                  const uint8_t *adapter, int32_t adapter_len, int32_t min_overlap, int64_t err_num, int64_t err_den,
                  int32_t front_qual, int32_t win_len, int64_t win_num, int64_t win_den, int32_t tail_qual,
                  int64_t **start, int64_t **end, int64_t *n_rows, int64_t *first_bad);
int fx_fastq_format_alloc(fx_handle *h, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                          int64_t min_len, uint8_t **dst, int64_t **dst_off, int64_t *n_rows, int64_t *n_kept,
                          int64_t *first_bad);

/* ------------------------------------------------------------------ barcode demultiplexing (extension)
 * The reference has no counterpart.  Integer and exact (pyfastx_amd/csrc/fx_fastq_demux.hpp).  s, L and H are those of
 * fx_fastq_trim / fx_fastq_format_alloc: s = the rlen bytes at soff, L = rlen, H = the dlen bytes at soff - dlen - 1 without one
 * trailing '\r'; a byte past the end of the stream reads as 0.
 *
 * A SAMPLE has n_seg = 1 or 2 SEGMENTS.  Segment g has a source src[g], an offset off[g] >= 0, a length len[g] in 1..32, a
 * mismatch budget mm[g] in 0..len[g] and, per sample, len[g] upper-case letters of A C G T N; `barcodes` holds n_samples
 * (1..4096) rows of len[0] + len[1] letters, segment 0 first.  For each read, segment g gives a WINDOW of len[g] slots, each a
 * byte or ABSENT:
 *   FX_DEMUX_SEQ5    slot j is s[off + j] if off + j < L, else ABSENT.
 *   FX_DEMUX_SEQ3    p = L - off - len + j; slot j is s[p] if 0 <= p < L, else ABSENT.
 *   FX_DEMUX_HEADER  off is the part number, 0 or 1.  F = the longest suffix of H that holds no ':'.  If H holds no ':' at
 *                    all, or F is longer than 65 bytes, every slot is ABSENT (nothing further back than 66 bytes is looked
 *                    at).  Part 0 is F up to its first '+', or all of F if there is none; part 1 is what follows the first
 *                    '+', empty if there is none.  Slot j is byte j of the part, ABSENT beyond its end; bytes of the part
 *                    beyond len are ignored (a prefix compare).
 * The distance of a sample's segment, d_g = the j whose barcode letter is not 'N' and whose slot is ABSENT or is not that exact
 * byte (lower case, N and IUPAC codes in the read mismatch, as in fx_fastq_trim); with one segment d_1 = 0.  A sample PASSES
 * when d_g <= mm[g] for each segment; its total is t = d_0 + d_1.  With t(1) <= t(2) the two smallest totals over the passing
 * samples:
 *   none passes                       sample = FX_DEMUX_NONE       dist = -1    second = -1
 *   exactly one passes                sample = its index           dist = t(1)  second = -1
 *   t(2) - t(1) >= margin (1..64)     sample = the one with t(1)   dist = t(1)  second = t(2)
 *   otherwise (ties included)         sample = FX_DEMUX_AMBIGUOUS  dist = t(1)  second = t(2)
 *
 * fx_fastq_demux: one row of sample / dist / second per query, in the order of ids (ids = NULL: every read; repeats allowed);
 *   counts[n_samples + 2] = the queries per sample, then NONE, then AMBIGUOUS; *n_rows = the rows.  want_order != 0: also
 *   order[n] = the query positions sorted by (bin, position) -- the bin is the sample index, n_samples for NONE, n_samples + 1
 *   for AMBIGUOUS -- and bin_off[n_samples + 3]: bin k is order[bin_off[k] .. bin_off[k + 1]); both are made on the device (a
 *   stable radix sort on the bin, a scan of the counters) and take at most 2^31 queries.  want_order = 0: order and bin_off
 *   may be NULL and are not made.  Outputs are pinned blocks of fx_pinned_alloc that belong to the caller, never NULL after
 *   FX_OK.  States and errors are those of fx_fastq_trim (a null handle or output pointer: FX_EINVAL, nothing touched; before
 *   fx_fastq_build: FX_ESTATE; a byte-range shard: FX_EINVAL; an id outside the table: *first_bad = its position, FX_ERANGE,
 *   nothing allocated); an argument outside the ranges above or a barcode byte outside A C G T N: FX_EINVAL. */
#define FX_DEMUX_SEQ5 0
#define FX_DEMUX_SEQ3 1
#define FX_DEMUX_HEADER 2
#define FX_DEMUX_NONE (-1)
#define FX_DEMUX_AMBIGUOUS (-2)
int fx_fastq_demux(fx_handle *h, const int64_t *ids, int64_t n_ids, int32_t n_seg, const int32_t *src, const int32_t *off,
                   const int32_t *len, const int32_t *mm, const uint8_t *barcodes, int32_t n_samples, int32_t margin,
                   int32_t want_order, int32_t **sample, int32_t **dist, int32_t **second, int64_t **counts, int64_t **order,
                   int64_t **bin_off, int64_t *n_rows, int64_t *first_bad);

/* ------------------------------------------------------------------ paired-end FASTQ: mate overlap, merged records (extension)
 * The reference has no counterpart: it reads one file at a time.  h1 and h2 hold the two files of a paired run; pair i is read i
 * of h1 and read i of h2, with s1, q1, L1 and s2, q2, L2 the bytes fx_fastq_fetch returns for them (a byte past the end of a
 * stream reads as 0).  Integer and exact (pyfastx_amd/csrc/fx_fastq_pair.hpp).
 *
 * Position j of read 1 MATCHES position k of the reverse-complemented read 2 when s1[j] and s2[L2-1-k] are both upper-case
 * A C G T and s1[j] is the Watson-Crick complement of s2[L2-1-k]; lower case, N and IUPAC codes mismatch, as in fx_fastq_trim.
 * DIAGONAL d, in -(L2-1) .. L1-1, places letter k of the reverse complement under s1[k+d]: lo = max(0, d), hi = min(L1, d + L2),
 * m = hi - lo, mm = the j in [lo, hi) that do not match k = j - d.  d is ACCEPTED when m >= min_overlap, mm <= max_diff and
 * mm * err_den <= err_num * m.  The diagonals are tried in the order 0, 1, ..., L1-1, -1, -2, ..., -(L2-1) -- the longest
 * overlap first in each direction -- and the first accepted one is the pair's result; there is no shortcut.
 *
 * fx_fastq_pair_overlap: per pair (in the order of ids; ids = NULL: every pair), five columns of *n_rows rows:
 *   diag        d, or FX_PAIR_NONE when no diagonal is accepted
 *   overlap     m (0 when none);  mismatches  mm (0 when none)
 *   end1, end2  what survives adapter read-through: for d < 0 end1 = min(L1, L2 + d) and end2 = L2 + d, otherwise L1 and L2
 *   (the insert follows: none: -1; d >= 0: max(L1, d + L2); d < 0: L2 + d).
 *   min_overlap >= 1, max_diff >= 0, err_num within 0..10^9, err_den within 1..10^9, else FX_EINVAL.
 * fx_fastq_pair_merge_alloc: the merged records of the queries, back to back.  diag: row k belongs to query k (what
 *   fx_fastq_pair_overlap returned for the same ids); a row that is neither FX_PAIR_NONE nor inside -(L2-1) .. L1-1 of its pair
 *   gives *first_bad = the first such query, FX_ERANGE, nothing allocated.  With F = the insert, fragment position f in [0, F)
 *   has has1 = f < L1, k = f - d, has2 = 0 <= k < L2, y = comp(s2[L2-1-k]) (comp: the complement table of fx_fastq_fetch's
 *   reverse-complement flag), b = q2[L2-1-k]; only one mate present: that mate's byte and quality; both, with x = s1[f] and a =
 *   q1[f]: x == y as bytes: x with quality max(a, b); else a >= b: x, a; else y, b (qualities compared as raw bytes).  The
 *   record is H1 "\n" seq "\n+\n" qual "\n", H1 = the header of read 1 as fx_fastq_format_alloc cuts it.  A query with diag =
 *   FX_PAIR_NONE or F < min_len (>= 0) produces no bytes.  Record k is dst[dst_off[k] .. dst_off[k + 1]); dst_off has *n_rows
 *   + 1 entries, *n_merged = the records that produced bytes.
 * ids, the pinned outputs (fx_pinned_alloc blocks that belong to the caller, never NULL after FX_OK), *first_bad and the errors
 * are those of fx_fastq_trim / fx_fastq_format_alloc (a null handle or output pointer: FX_EINVAL, nothing touched; an id
 * outside the table: *first_bad = its position, FX_ERANGE, nothing allocated), and: handles on different devices: FX_EINVAL;
 * different numbers of reads: FX_EINVAL; either handle a byte-range shard: FX_EINVAL; either handle before fx_fastq_build:
 * FX_ESTATE.  The work runs on h1's stream, which is made to wait for what h2's stream holds (an event, no device-wide wait). */
#define FX_PAIR_NONE INT32_MIN
int fx_fastq_pair_overlap(fx_handle *h1, fx_handle *h2, const int64_t *ids, int64_t n_ids, int32_t min_overlap, int32_t max_diff,
                          int64_t err_num, int64_t err_den, int32_t **diag, int32_t **overlap, int32_t **mismatches,
                          int64_t **end1, int64_t **end2, int64_t *n_rows, int64_t *first_bad);
int fx_fastq_pair_merge_alloc(fx_handle *h1, fx_handle *h2, const int64_t *ids, int64_t n_ids, const int32_t *diag, int64_t min_len,
                              uint8_t **dst, int64_t **dst_off, int64_t *n_rows, int64_t *n_merged, int64_t *first_bad);

/* ------------------------------------------------------------------ k-mer spectra (extension)
 * The reference counts single letters only (composition); these count every window of k bases, 1 <= k <= 13, into a dense
 * table of 4^k exact int64 counters on the device (pyfastx_amd/csrc/fx_kmer.hpp).  Larger k, up to 31, has a sparse form:
 * the k-mer tables below.
 *   alphabet     A C G T and a c g t, case-insensitive: A = 0, C = 1, G = 2, T = 3.  Every other byte (N, U, IUPAC codes,
 *                '-', '*', digits, bytes >= 128) is invalid, and a window that holds one is not counted.
 *   code         of the window b0 b1 .. b(k-1): sum of code(bj) * 4^(k-1-j) -- the first base is the most significant digit.
 *   flags        FX_KMER_CANONICAL: a window counts under min(code, code of its reverse complement); a window that is its
 *                own reverse complement (even k only) counts once; entries whose index is no canonical code stay 0.  The
 *                table has 4^k entries in both forms, and its sum is the number of valid windows.
 * fx_fasta_kmers: the windows are the len(s) - k + 1 windows of the `seq` s of every selected record -- the bytes
 *   fx_fasta_search walks: bytes 10 / 13 / 32 dropped, windows run across line ends, never from one record into the next and
 *   never past slen.  ids, n_ids: the records (0-based, any order, a record listed twice counts twice; ids = NULL: all of
 *   them; a non-NULL ids with n_ids = 0: none, the table is zero).  per_record = 0: one table, *n_rows = 1.  per_record != 0
 *   (k <= 6 only): one table per selected record in the order of ids, *n_rows = their number, counts[row * 4^k + code].
 * fx_fastq_kmers: the windows of s[a:b] of every selected read, s = the rlen bytes at soff (what fx_fastq_fetch returns;
 *   no line rule of its own), a = 0 and b = rlen unless start / end are given: row j of both belongs to query j, as for
 *   fx_fastq_format_alloc (what fx_fastq_trim returned for the same ids).  One table.
 * *counts is a pinned block of fx_pinned_alloc that belongs to the caller (fx_pinned_free), never NULL after FX_OK.
 * Errors: a null handle or output pointer, start without end: FX_EINVAL, nothing touched; before fx_fasta_build /
 * fx_fastq_build: FX_ESTATE; a byte-range shard (fx_set_shard, fx_open_file_range; a window across a cut has no halo):
 * FX_EINVAL; unknown flag bits, k outside 1..13 (1..6 with per_record): FX_EINVAL; an id outside the table, or an interval
 * outside 0 <= start <= end <= rlen: *first_bad = its position among the queries, FX_ERANGE, nothing allocated; no device:
 * FX_EDEVICE (there is no CPU path). */
enum { FX_KMER_CANONICAL = 1 };
int fx_fasta_kmers(fx_handle *h, int32_t k, int flags, const int64_t *ids, int64_t n_ids, int per_record, int64_t **counts,
                   int64_t *n_rows, int64_t *first_bad);
int fx_fastq_kmers(fx_handle *h, int32_t k, int flags, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                   int64_t **counts, int64_t *first_bad);

/* ------------------------------------------------------------------ k-mer tables (extension)
 * The sparse form of the spectra above for 1 <= k <= 31 (pyfastx_amd/csrc/fx_kmer_table.hpp): alphabet, code, FX_KMER_CANONICAL
 * and the windows of a selection are those of fx_fasta_kmers / fx_fastq_kmers, word for word.  A code has 2k <= 62 bits and is
 * an exact non-negative int64.  The table of a selection is the set of codes that occur at least once among its valid
 * windows, ascending, each with its exact count: codes[i] < codes[i + 1], counts[i] >= 1; with FX_KMER_CANONICAL only
 * canonical codes appear.  A record or read listed twice counts twice.
 *   min_count    >= 1: entries whose total count is below it are dropped, on the device, after every contribution to a code
 *                has been summed.
 *   *n_windows   the valid windows of the selection, before min_count (= the sum of the counts when min_count is 1).
 *   *n_parts     the sort-and-reduce rounds that ran: the codes are sorted in ranges of their leading bits, as many at a time
 *                as the budget holds; a range with more windows than that is taken in pieces whose tables are summed.
 *   max_bytes    bound on the device working memory of the call beyond the resident stream and its tables (key buffers,
 *                histograms, partial lists).  0: the default, 8 GiB -- a third of the 24 GiB the library's scratch pool
 *                keeps, so that the buffers of a call come out of it and go back into it beside the blocks an open leaves
 *                there.  A value below 1 MiB: FX_EINVAL.  The table does not depend on it, *n_parts does.
 * *codes / *counts are pinned blocks of fx_pinned_alloc that belong to the caller (fx_pinned_free), *n_distinct entries each,
 * never NULL after FX_OK; *n_distinct may be 0.
 * Errors: a null handle or output pointer, start without end: FX_EINVAL, nothing touched; before fx_fasta_build /
 * fx_fastq_build: FX_ESTATE; a byte-range shard: FX_EINVAL; unknown flag bits, k outside 1..31, min_count < 1, max_bytes
 * below 1 MiB: FX_EINVAL; an id outside the table, or an interval outside 0 <= start <= end <= rlen: *first_bad = its position
 * among the queries, FX_ERANGE, nothing allocated; no device: FX_EDEVICE (there is no CPU path); a code range whose table
 * alone does not fit the budget (or one read with more windows than a key buffer holds): FX_ENOMEM, the message names the
 * max_bytes that would do. */
int fx_fasta_kmer_table(fx_handle *h, int32_t k, int flags, const int64_t *ids, int64_t n_ids, int64_t min_count, int64_t max_bytes,
                        int64_t **codes, int64_t **counts, int64_t *n_distinct, int64_t *n_windows, int64_t *n_parts,
                        int64_t *first_bad);
int fx_fastq_kmer_table(fx_handle *h, int32_t k, int flags, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                        int64_t min_count, int64_t max_bytes, int64_t **codes, int64_t **counts, int64_t *n_distinct,
                        int64_t *n_windows, int64_t *n_parts, int64_t *first_bad);

/* ------------------------------------------------------------------ k-mer screening (extension)
 * How many of the k-mers of a read or record occur in a set of k-mers (pyfastx_amd/csrc/fx_kmer_screen.hpp): the count a
 * contaminant / adapter / rRNA filter keeps or drops reads on, and, per FASTA record, the containment index.
 * The set.  fx_kmer_set_create builds an open-addressing hash set of the `n` codes (a table's codes, for one) on the device of
 * `h`.  It lives on that device and needs `h` only at creation: any handle on the same device may use it afterwards -- one
 * contaminant set against many files --, a handle on another device gets FX_EINVAL.  flags: FX_KMER_CANONICAL or 0.  With it
 * every window is looked up under min(code, code of its reverse complement), and every code given must be canonical: one that
 * is not is FX_EINVAL, checked on the device before anything is kept.  Without it only the forward code of a window is looked
 * up.  k in 1..31; codes in [0, 4^k), else FX_EINVAL; n in 0..2^31; a code given twice is kept once; n = 0 is a valid empty
 * set that nothing hits.  A failed allocation of the set's memory (16 bytes per code or more): FX_ENOMEM.  fx_kmer_set_free
 * gives it back (NULL: nothing to do).  fx_kmer_set_contains: out[i] = 1 where codes[i] (host arrays) is in the set as given --
 * no folding to the canonical code --, else 0; a value outside [0, 4^k) is in no set.
 * Windows and selections.  Alphabet, code, the windows of a selection, ids, start / end and the cut at slen are those of
 * fx_fasta_kmer_table / fx_fastq_kmer_table, word for word; k and the canonical form come from the set.  n_windows[q] is the
 * number of valid windows of query q, n_hits[q] how many of them are in the set; a window that occurs twice counts twice.
 * One row per query in the order of ids (a record or read listed twice has two rows); *n_rows = their number.  FASTQ columns
 * are int32, FASTA columns int64.
 * The screen.  Query q passes when n_hits >= min_hits and n_hits * frac_den >= frac_num * n_windows, in int64; frac_den = 0:
 * the ratio is not asked; frac_num and frac_den lie within 0..10^9 and min_hits is not negative, else FX_EINVAL.  A query
 * without windows passes the ratio test.  invert != 0 flips the final result.  *pos: the ascending positions among the queries
 * of those that pass, *n_pos of them -- the read ids themselves when ids is NULL.  The columns stay on the device; only the
 * positions come home.
 * Outputs are pinned blocks of fx_pinned_alloc that belong to the caller (fx_pinned_free), never NULL after FX_OK.
 * Errors: a null handle, set or output pointer, start without end: FX_EINVAL, nothing touched; before fx_fasta_build /
 * fx_fastq_build: FX_ESTATE; a byte-range shard: FX_EINVAL; an id outside the table, or an interval outside 0 <= start <= end
 * <= rlen: *first_bad = its position among the queries, FX_ERANGE, nothing allocated; no device: FX_EDEVICE (there is no CPU
 * path). */
typedef struct fx_kmer_set fx_kmer_set;
int fx_kmer_set_create(fx_handle *h, int32_t k, int flags, const int64_t *codes, int64_t n, fx_kmer_set **set);
int fx_kmer_set_free(fx_kmer_set *set);
int fx_kmer_set_contains(fx_kmer_set *set, const int64_t *codes, int64_t n, uint8_t *out);
int fx_fastq_kmer_hits(fx_handle *h, const fx_kmer_set *set, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                       int32_t **n_windows, int32_t **n_hits, int64_t *n_rows, int64_t *first_bad);
int fx_fastq_kmer_screen(fx_handle *h, const fx_kmer_set *set, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                         int64_t min_hits, int64_t frac_num, int64_t frac_den, int invert,
                         int64_t **pos, int64_t *n_pos, int64_t *first_bad);
int fx_fasta_kmer_hits(fx_handle *h, const fx_kmer_set *set, const int64_t *ids, int64_t n_ids,
                       int64_t **n_windows, int64_t **n_hits, int64_t *n_rows, int64_t *first_bad);

/* ------------------------------------------------------------------ sketches (extension)
 * MinHash and FracMinHash sketches of records and read sets, and their comparison on the device
 * (pyfastx_amd/csrc/fx_sketch.hpp): what Mash and sourmash answer -- how similar are these contigs, assemblies or read sets,
 * which reference is contained in this sample, what is the approximate ANI.  The reference has no counterpart.
 * Windows.  The alphabet, code, canonical form, windows and the cut at slen are those of fx_fasta_kmer_table and
 *   fx_fastq_kmer_table, word for word: 1 <= k <= 31; valid letters are ACGTacgt (U, N, IUPAC codes and every other byte are
 *   not); A = 0 C = 1 G = 2 T = 3, the first letter most significant; windows run across line ends, never across records, and
 *   never past slen; FASTQ windows are those of s[start:end] of the selected reads.
 * Key.  key = mix(code) with m = 4^k - 1: exactly the hash of fx_fasta_minimizers, a bijection of the 2k-bit words.  With
 *   FX_SK_CANONICAL code = min(fw, rc), otherwise code = fw.  Keys are uint64, below 2^62.
 * Sets.  FASTA: one set per selected record, in ascending record order (ids, n_ids as for fx_fasta_minimizers: ids = NULL
 *   means every record; the caller passes distinct ascending ids).  FASTA with FX_SK_POOLED: one set for all selected records
 *   together, such as a multi-contig assembly.  FASTQ: always one pooled set of the selected reads; ids, start, end as for
 *   fx_fastq_kmer_table.  No selected record or read: no set (one empty set when pooled).
 * What a set keeps.  max_key (1 .. 4^k) and size (>= 0) decide.  The FracMinHash part of a set is the set of distinct keys of
 *   its valid windows with key < max_key.  With size > 0 the set is the `size` smallest of those, or all of them when there
 *   are fewer; size = 0 puts no cap on the count.  max_key = 4^k with size = s is the classic bottom-s MinHash.  (In Python
 *   `scaled`, an integer >= 1, maps to max_key = ceil(4^k / scaled): key * scaled < 4^k without the overflow.)  Every set is
 *   stored ascending and distinct.
 * Rounds.  With size > 0 not every window below max_key is emitted: round 0 gives each set a threshold near
 *   4^k * oversample * size / windows, capped at max_key; a set is final when it holds at least `size` distinct keys below
 *   its threshold, or when its threshold equals max_key; the other sets get their threshold times 8, saturating, and are
 *   walked again alone.  *n_rounds = the rounds that ran (0 without a window to walk).  oversample: 1 .. 64, 0 = the default
 *   of 4; it exists so that tests can reach the retry path.  No result depends on it, only *n_rounds does.
 * Comparison.  Sets A and B, a limit L >= 0 and a restriction max_key (0: none; otherwise both sets are first cut to their
 *   keys below it, a prefix of each).  U = the ascending distinct union, U_L = its first min(L, |U|) elements, or all of U
 *   when L = 0.  total = |U_L| and shared = |{x in U_L : x in A and x in B}|.  From these follow: Jaccard = shared / total;
 *   containment of A in B = shared / |A| at L = 0; Mash distance = -ln(2j / (1 + j)) / k with j taken at L = the sketch size,
 *   clipped to [0, 1], and 1 when j = 0; ANI estimate = containment^(1/k).
 * fx_sketch is opaque and tied to a device, like fx_kmer_set; it needs no handle after its creation.
 *   fx_fasta_sketch, fx_fastq_sketch   build one from the resident stream.
 *   fx_sketch_info        the parameters and sizes (any output may be NULL).  flags: as given, FASTQ with FX_SK_POOLED set.
 *   fx_sketch_read        *off (n_sets + 1 offsets) and *keys (n_keys keys; one item when there is none): pinned blocks of
 *                         fx_pinned_alloc that belong to the caller (fx_pinned_free each).
 *   fx_sketch_from_host   a sketch from host arrays; off[0] = 0, off[n_sets] = the number of keys.  The checks run on the
 *                         device before anything is kept: offsets that do not ascend, keys that are not strictly ascending
 *                         within a set, a key >= max_key, or a set longer than size (> 0) give FX_EINVAL.
 *   fx_sketch_compare     all pairs of the selected sets of a (ia, n_a; ia = NULL: all sets, in order) with the selected sets
 *                         of b: *shared and *total, row-major int64[n_a * n_b], pinned blocks that belong to the caller (one
 *                         item each without a pair).  Selections may repeat and come in any order.
 *   fx_sketch_free        NULL: nothing to do.
 * Errors.  k outside 1..31, unknown flag bits, max_key outside 1..4^k, size < 0, oversample outside 0..64, a null output:
 * FX_EINVAL, refused before the handle is looked at; then a null handle, start without end: FX_EINVAL; before fx_fasta_build /
 * fx_fastq_build: FX_ESTATE; a byte-range shard: FX_EINVAL; an id outside the table, or an interval outside 0 <= start <= end
 * <= rlen (*first_bad = its position among the queries): FX_ERANGE; more than 2^31 - 1 rows of keys below the thresholds in
 * one round, or rows the scratch pool cannot hold: FX_ERANGE with the count in the message, nothing allocated (a larger scaled
 * gives fewer); no device: FX_EDEVICE (there is no CPU path).  fx_sketch_compare: different k or canonical form, or different
 * devices: FX_EINVAL; a selected set outside the sketch, or more than max_pairs pairs: FX_ERANGE. */
enum { FX_SK_CANONICAL = 1, FX_SK_POOLED = 2 };
typedef struct fx_sketch fx_sketch;
int fx_fasta_sketch(fx_handle *h, int32_t k, int flags, const int64_t *ids, int64_t n_ids, uint64_t max_key, int64_t size, int32_t oversample,
                    fx_sketch **sk, int32_t *n_rounds);
int fx_fastq_sketch(fx_handle *h, int32_t k, int flags, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                    uint64_t max_key, int64_t size, int32_t oversample, fx_sketch **sk, int32_t *n_rounds, int64_t *first_bad);
int fx_sketch_info(const fx_sketch *sk, int32_t *k, int *flags, uint64_t *max_key, int64_t *size, int64_t *n_sets, int64_t *n_keys);
int fx_sketch_read(fx_sketch *sk, int64_t **off, uint64_t **keys);
int fx_sketch_from_host(int device, int32_t k, int flags, uint64_t max_key, int64_t size, int64_t n_sets, const int64_t *off, const uint64_t *keys,
                        fx_sketch **sk);
int fx_sketch_compare(fx_sketch *a, fx_sketch *b, const int64_t *ia, int64_t n_a, const int64_t *ib, int64_t n_b, int64_t limit, uint64_t max_key,
                      int64_t max_pairs, int64_t **shared, int64_t **total);
int fx_sketch_free(fx_sketch *sk);

/* ------------------------------------------------------------------ duplicate reads (extension)
 * Exact duplicate detection on the resident FASTQ stream (pyfastx_amd/csrc/fx_fastq_dedup.hpp): what FastQC's duplication
 * levels, `seqkit rmdup -s` or `fastp --dedup` answer, without a base leaving the device.  The reference has no counterpart.
 * Queries.  ids, n_ids, start, end are those of fx_fastq_kmers, word for word: ids 0-based, in any order, repeats allowed;
 * ids = NULL: every read (a non-NULL ids with n_ids = 0: no query); start and end both given or both NULL; row q of both
 * belongs to query q; 0 <= start <= end <= rlen.
 * The key of query q is the byte string s[a:b], s = the rlen bytes at soff (what fx_fastq_fetch returns), a = 0 and b = rlen
 * unless start / end are given.  The bytes are taken as they are: case-sensitive, N and IUPAC codes are ordinary bytes.  The
 * name and the quality line play no part.
 * Duplicates.  Two queries are duplicates when their keys are equal as byte strings, lengths included; all empty keys are
 * equal to one another, and a read listed twice in ids is a duplicate of its first listing.  FX_DUP_REVCOMP: two queries are
 * duplicates when the key of one equals the key of the other or its reverse complement -- the key reversed, A<->T, C<->G,
 * a<->t, c<->g, every other byte mapped to itself; that is: when min(key, rc(key)), compared as byte strings, is the same.
 * first[q] is the smallest query position p whose key is a duplicate of q's: first[q] <= q, and first[q] == q exactly for the
 * first occurrence of each group.  *n_groups = the number of groups.
 * The answer is exact, not probabilistic: queries are grouped by a 64-bit fingerprint, and every member of a group of equal
 * fingerprints is then compared with the group's first member byte by byte; the ones that differ (two keys, one fingerprint)
 * go through another round under another seed.  *n_rounds = the rounds that ran (0 without a query, 1 in practice).
 *   hash_bits    0: all 64 bits of the fingerprint; 1..64: only that many.  It exists so that tests can reach the collision
 *                path.  No result depends on it, only *n_rounds does.
 * fx_fastq_dup_first: *first, *n_rows = the number of queries.
 * fx_fastq_dedup: the ascending positions among the queries of the first occurrences whose group has at least min_copies
 *   (>= 1) and, unless max_copies < 0, at most max_copies members -- the read ids themselves when ids is NULL; *copies (the
 *   pointer may be NULL: not wanted) = the members of the group of each.  first stays on the device; only the positions and
 *   the copies come home.  *n_groups counts all groups, whatever min_copies / max_copies select.
 * Outputs are pinned blocks of fx_pinned_alloc that belong to the caller (fx_pinned_free), never NULL after FX_OK.
 * Errors: a null handle or output pointer (copies apart), start without end: FX_EINVAL, nothing touched; before
 * fx_fastq_build: FX_ESTATE; a byte-range shard, unknown flag bits, hash_bits outside 0..64, min_copies < 1, more than 2^31
 * queries (the sort carries 32-bit positions): FX_EINVAL; an id outside the table, or an interval outside 0 <= start <= end
 * <= rlen: *first_bad = its position among the queries, FX_ERANGE, nothing allocated; device working memory (about 45 bytes
 * per query, out of the library's scratch pool) not to be had: FX_ENOMEM; no device: FX_EDEVICE (there is no CPU path). */
enum { FX_DUP_REVCOMP = 1 };
int fx_fastq_dup_first(fx_handle *h, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                       int flags, int hash_bits, int64_t **first, int64_t *n_rows, int64_t *n_groups,
                       int64_t *n_rounds, int64_t *first_bad);
int fx_fastq_dedup(fx_handle *h, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                   int flags, int hash_bits, int64_t min_copies, int64_t max_copies,
                   int64_t **pos, int64_t **copies, int64_t *n_pos, int64_t *n_groups, int64_t *n_rounds,
                   int64_t *first_bad);

/* ------------------------------------------------------------------ FASTA records written back out (extension)
 * The reference writes a record only as a verbatim copy (Sequence.raw, sequence.c:314-335) and slices one interval per call
 * (sequence.c:76-125).  fx_fasta_format_alloc turns a batch of records or intervals of the resident stream back into FASTA text
 * -- the counterpart of fx_fastq_format_alloc -- formatted and laid out on the device (pyfastx_amd/csrc/fx_fasta_format.hpp).
 *
 * Queries.  Query k is (seq_id[k], start[k], stop[k]), half-open and 0-based, exactly as fx_fasta_fetch takes them.  start =
 *   stop = NULL: whole records, [0, slen).  seq_id = NULL is allowed only then and means the records 0..n-1.  An id outside
 *   the table or an interval outside 0 <= start <= stop <= slen (or longer than 2^31 - 1): *first_bad = the first such query,
 *   FX_ERANGE, nothing allocated.
 * Letters S_k, made in this order:
 *   1 what fx_fasta_fetch returns for the query with flags 0: the forward letters, bytes 10 / 13 / 32 dropped (a record that
 *     is not line-regular is despaced first and sliced then);
 *   2 FX_UPPER: a..z become A..Z;
 *   3 the mask: a letter whose forward coordinate lies in a mask row of its record is changed -- FX_MASK_SOFT turns A..Z
 *     into a..z, FX_MASK_UPPER a..z into A..Z, FX_MASK_HARD replaces every byte with mask_byte (0..255);
 *   4 FX_COMPLEMENT through the IUPAC table of the fetch kernels: case is kept, so a soft mask survives;
 *   5 FX_REVERSE.
 *   flags (bits FX_UPPER | FX_REVERSE | FX_COMPLEMENT only) hold for every query unless flags_per_query gives a byte per query,
 *   of which those three bits count.  L_k = |S_k|: for an irregular record the letters actually there, which can be fewer
 *   than stop - start.
 * Mask rows.  n_mask rows (mask_id, mask_start, mask_stop) sorted by (mask_id, mask_start), 0 <= start <= stop <= slen, every
 *   row of a record beginning at or after the end of the row before it; empty rows are allowed.  Anything else: *first_bad =
 *   the first such row, FX_EINVAL, nothing allocated (checked on the device).  mask_mode = FX_MASK_NONE ignores the rows.
 * Header H_k.  hdr = NULL: the record's own header line without '>' and without its terminator, one trailing '\r' dropped
 *   (what Sequence.description shows), copied from the stream on the device; this needs the table of fx_fasta_build
 *   (fx_fasta_set_table installs no header columns: FX_ESTATE).  Otherwise the bytes hdr[hdr_off[k] .. hdr_off[k + 1]) as
 *   they are (hdr_off: n + 1 ascending offsets from 0 on).
 * Record k is '>' H_k '\n', then S_k in lines of `width` letters, each followed by '\n'; the last line may be shorter.  width
 *   = 0: one line; L_k = 0: no sequence line; width < 0: FX_EINVAL.  Its size is |H_k| + 2 + L_k + ceil(L_k / width).  A
 *   query with L_k < min_len (>= 0) produces no bytes.
 * Outputs.  Record k is dst[dst_off[k] .. dst_off[k + 1]); *dst and *dst_off (n + 1 entries) are pinned blocks of
 *   fx_pinned_alloc that belong to the caller (fx_pinned_free each), never NULL after FX_OK.  *n_kept = the records that
 *   produced bytes, *n_bases = the sum of their L_k.  Sizes, offsets and bytes are made on the device; only the finished
 *   bytes and the offsets come to the host.
 * Errors: a null handle or output pointer, start without stop, seq_id = NULL with intervals, n < 0, unknown flag bits, a
 *   mask_mode outside the four, hdr without hdr_off or offsets that descend: FX_EINVAL, nothing touched; before
 *   fx_fasta_build: FX_ESTATE; a byte-range shard: FX_EINVAL; 2^31 queries or more: FX_ERANGE; no device: FX_EDEVICE (there is
 *   no CPU path).
 * fx_fasta_format_tile: the bytes of the output one workgroup of the emit kernel owns (tests place records across its edges). */
enum { FX_MASK_NONE = 0, FX_MASK_SOFT = 1, FX_MASK_HARD = 2, FX_MASK_UPPER = 3 };
int fx_fasta_format_alloc(fx_handle *h, int64_t n, const int64_t *seq_id, const int64_t *start, const int64_t *stop,
                          int flags, const uint8_t *flags_per_query, int64_t width,
                          const uint8_t *hdr, const int64_t *hdr_off,
                          int64_t n_mask, const int64_t *mask_id, const int64_t *mask_start, const int64_t *mask_stop,
                          int mask_mode, int mask_byte, int64_t min_len,
                          uint8_t **dst, int64_t **dst_off, int64_t *n_kept, int64_t *n_bases, int64_t *first_bad);
int fx_fasta_format_tile(void);

/* ------------------------------------------------------------------ BGZF written on the device (extension)
 * The reference writes nothing compressed.  A deflate encoder on the device (pyfastx_amd/csrc/fx_deflate.hpp) turns a buffer
 * into BGZF members, so that the record writers hand the host compressed bytes only.
 *
 * Members.  Member m carries the input bytes [m * 65280, min(n, (m + 1) * 65280)) and refers to nothing outside itself; n = 0
 *   gives no member.  A member is 18 bytes of header (1f 8b 08 04, mtime 0, XFL 0, OS ff, XLEN 6, "BC", SLEN 2, BSIZE - 1), one
 *   deflate stream of one block, the CRC-32 of the payload and ISIZE.  No EOF member is written: that is the file writer's.
 * level  0: a stored block per member.  1: a dynamic-Huffman block of literals.  2: matches (lengths 4..258, distances
 *   1..32768, inside the member) and a dynamic-Huffman block.  At 1 and 2 a member whose coded form would not be smaller is
 *   stored, so no member exceeds its payload + 31 bytes.  The same input and level give the same bytes on every call.
 * fx_bgzf_compress: n bytes of a host buffer -> *dst (*dst_bytes bytes) and *member_off (*n_members + 1 offsets of the members
 *   in *dst; the uncompressed offset of member m is m * 65280), both pinned blocks of fx_pinned_alloc that belong to the caller
 *   (fx_pinned_free), never NULL after FX_OK.
 * fx_fastq_format_bgzf_alloc, fx_fasta_format_bgzf_alloc, fx_fastq_pair_merge_bgzf_alloc: the records of their siblings without
 *   the suffix, compressed before they leave the device.  Arguments, *dst_off (offsets in the UNCOMPRESSED stream), the counts,
 *   *first_bad and every error are the sibling's; *zdst (*zbytes bytes) and *member_off (*n_members + 1) are as above.
 * Errors: a level outside 0..2, a null output pointer, n < 0: FX_EINVAL, nothing allocated; no device: FX_EDEVICE (there is no
 *   CPU path). */
int fx_bgzf_compress(const uint8_t *src, int64_t n, int level, int device, uint8_t **dst, int64_t *dst_bytes,
                     int64_t **member_off, int64_t *n_members);
int fx_fastq_format_bgzf_alloc(fx_handle *h, const int64_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end,
                               int64_t min_len, int level, uint8_t **zdst, int64_t **member_off, int64_t **dst_off,
                               int64_t *n_rows, int64_t *n_kept, int64_t *first_bad, int64_t *zbytes, int64_t *n_members);
int fx_fasta_format_bgzf_alloc(fx_handle *h, int64_t n, const int64_t *seq_id, const int64_t *start, const int64_t *stop,
                               int flags, const uint8_t *flags_per_query, int64_t width,
                               const uint8_t *hdr, const int64_t *hdr_off,
                               int64_t n_mask, const int64_t *mask_id, const int64_t *mask_start, const int64_t *mask_stop,
                               int mask_mode, int mask_byte, int64_t min_len, int level,
                               uint8_t **zdst, int64_t **member_off, int64_t **dst_off, int64_t *n_kept, int64_t *n_bases,
                               int64_t *first_bad, int64_t *zbytes, int64_t *n_members);
int fx_fastq_pair_merge_bgzf_alloc(fx_handle *h1, fx_handle *h2, const int64_t *ids, int64_t n_ids, const int32_t *diag,
                                   int64_t min_len, int level, uint8_t **zdst, int64_t **member_off, int64_t **dst_off,
                                   int64_t *n_rows, int64_t *n_merged, int64_t *first_bad, int64_t *zbytes, int64_t *n_members);
/* The code lengths (at most `limit`, 1..15) and canonical codes, bit-reversed, that the encoder gives nsym (1..288) symbol counts;
 * host only, for tests: the same routine the kernel runs. */
int fx_deflate_code_lengths(const uint32_t *freq, int nsym, int limit, uint8_t *lens, uint16_t *codes);

/* ------------------------------------------------------------------ Fastx
 * Replaces kseq_read (kseq.c:138-179) as pyfastx_fastx_next drives it (fastx.c:124-130): index-free iteration over a
 * file with kseq's own record rules -- FASTA and FASTQ records mixed, sequence / quality over any number of lines,
 * text between records skipped, white space kept inside the lines, a trailing CR dropped per ks_getuntil2 call
 * (kseq.c:106).  One record per kseq_read that returned >= 0. */
typedef struct {
    int64_t hdr_off;    /* first byte behind the '>' / '@'; name and comment are cut from these bytes (kseq.c:148-149)  */
    int64_t hdr_line;   /* number of the line that holds it                                                            */
    int64_t seq_len;    /* seq.l; qual.l of a FASTQ record is the same (kseq.c:176)                                    */
    int64_t seq_cum;    /* sum of seq_len over the records before this one                                             */
    uint32_t hdr_len;   /* bytes to the end of the line, '\n' excluded                                                  */
    uint32_t s_n;       /* lines between the header line and the line that ended the sequence                          */
    uint32_t q_n;       /* quality lines read                                                                          */
    uint32_t flags;     /* 1: FASTQ record (kseq_read went through kseq.c:167-177); 2: its quality read met the end of
                           the stream at once (the reference's buffer keeps its old content); 4: the header line has
                           no '\n' behind it                                                                           */
} fx_kseq_rec;
/* The walk over the whole resident stream.  *end_code = the negative value that ended the reference's iteration:
 * -1 end of file, -2 truncated quality string (kseq.c:131-136). */
int fx_kseq_scan(fx_handle *h, int64_t *n_records, int64_t *n_lines, int64_t *seq_bytes, int *end_code);
/* How many lines of the last scan the parallel passes took (a file of four-line FASTQ records, or of plain FASTA header /
 * sequence lines, up to the first line that is neither); the sequential walk did the rest.  FX_KSEQ_WALK_ONLY=1 in the
 * environment sends everything through the walk. */
int64_t fx_kseq_prefix_lines(const fx_handle *h);
/* Records [first, first + count) of the table, to host memory. */
int fx_kseq_records(fx_handle *h, int64_t first, int64_t count, fx_kseq_rec *out);
/* Their sequence strings, one behind the other (record k at seq_cum[k] - seq_cum[first]), and their quality strings at
 * the same offsets (zero bytes where a record has none); either destination may be NULL.  flags: FX_UPPER (sequence
 * only, fastx.c:14-22).  *n_bytes = bytes per destination. */
int fx_kseq_fetch(fx_handle *h, int where, int64_t first, int64_t count, int flags, uint8_t *seq_dst, uint8_t *qual_dst,
                  int64_t *n_bytes);


/* The same with explicit per-read offsets (the reference's call shape:
 * pyfastx_read_random_reader(read, buff, offset, bytes), read.c:37-45), for
 * callers that hold .fxi rows (soff, qoff, rlen) rather than ids. */
int fx_read_fetch(fx_handle *h, int where, int64_t n, const int64_t *soff, const int64_t *qoff,
                  const int64_t *rlen, int phred, int seq_flags,
                  uint8_t *seq, uint8_t *qual, int8_t *quali, const int64_t *dst_off);

/* ------------------------------------------------------------------ names
 * Batched name -> record id, replacing one `SELECT ... WHERE chrom=? LIMIT 1` B-tree probe per name
 * (pyfastx_index_get_seq_by_name, index.c:527-566; pyfastx_fastq_get_read_by_name, fastq.c:486-519) with an
 * open-addressing table of record ids in HBM whose keys are the name bytes of the resident stream.
 * kind: 0 = FASTA sequence names (first token, or the whole header after full_name), 1 = FASTQ read names.
 * Query names are packed: bytes of query i = qbytes[qoff[i] .. qoff[i+1]); with FX_HOST the packed buffer must
 * be readable 8 bytes past its end.  out_ids[i] = 0-based id of the first record with that name, -1 if none. */
int fx_names_build(fx_handle *h, int kind);
int fx_names_lookup(fx_handle *h, int where, int64_t nq, const uint8_t *qbytes, const int64_t *qoff, int64_t *out_ids);

/* Sorted order of the record names for the UNIQUE INDEX of the .fxi -- what `CREATE UNIQUE INDEX chromidx ON seq
 * (chrom)` (index.c:363) / `readidx ON read (name)` (fastq.c:152) sort on the CPU after the inserts.  order[i]
 * (n records, `where` = FX_HOST / FX_DEVICE) = 0-based id of the i-th smallest name in SQLite's BINARY collation
 * (memcmp, the shorter name first on a common prefix); equal names keep id order.  *n_dup (host) = number of
 * adjacent equal pairs: 0 means the names are distinct and fx_fxi_bulk_index may write the index from `order`;
 * otherwise the reference's CREATE UNIQUE INDEX fails (and is ignored), so no index is written.  kind as above. */
int fx_names_sort(fx_handle *h, int kind, int where, int64_t *order, int64_t *n_dup);

/* The record names back to back (what the `chrom` / `name` column of the .fxi stores), gathered from the record table
 * that is already in HBM: dst[name_off[i] .. name_off[i+1]) = name of record i, name_off: n + 1 host words, *total =
 * name_off[n].  FX_ERANGE when total > cap (only *total is valid then; n * longest name is a safe cap).  Host buffers. */
int fx_names_pack(fx_handle *h, int kind, uint8_t *dst, int64_t cap, int64_t *name_off, int64_t *total);
/* The same order for names that come from SEVERAL handles (the shards of one file): packed host buffer, n + 1 offsets;
 * order[i] = 0-based index of the i-th smallest name, *n_dup = adjacent equal pairs.  For the index b-tree of a merged
 * .fxi (fx_fxi_bulk_index) without CREATE UNIQUE INDEX's sort (index.c:363, fastq.c:155). */
int fx_sort_packed_names(int device, const uint8_t *names, const int64_t *name_off, int64_t n, int64_t *order, int64_t *n_dup);

/* ------------------------------------------------------------ statistics
 * Fasta.count(n), nl(p), longest, shortest, mean, median (fasta.c:573-849) ask SQLite to scan or sort the seq table, one
 * query each.  Here the lengths are already in HBM: one stable radix sort of (slen, id), a scan of the sorted lengths and
 * one probe kernel answer all of them in a call.
 *   longest_id / shortest_id: 0-based id of the FIRST record with the extreme length (SQLite's MAX()/MIN() keep the first
 *   row they met: `SELECT ID,MAX(slen) FROM seq`, fasta.c:682, 715);
 *   count_ge: records with slen >= count_min (`SELECT COUNT(*) FROM seq WHERE slen>=?`, fasta.c:586);
 *   med_lo, med_hi: the sorted lengths at (n-1)/2 and, for an even n, the one after it (fasta.c:812-816);
 *   nx_len, nx_count: N(p) / L(p) -- walking the lengths in descending order, the first length (and how many so far)
 *   at which the running sum reaches `half`, a double = p / 100.0 * stat.seqlen compared as in fasta.c:630-647; 0, 0
 *   when the sum never does.  Needs the record table (fx_fasta_build or fx_fasta_set_table). */
typedef struct {
    int64_t n_seq, sum_len;
    int64_t longest_id, longest_len, shortest_id, shortest_len;
    int64_t count_ge;
    int64_t med_lo, med_hi;
    int64_t nx_len, nx_count;
} fx_len_stats;
int fx_fasta_len_stats(fx_handle *h, int64_t count_min, double half, fx_len_stats *out);

/* pyfastx.reverse_complement / reverse_seq / complement_seq on a caller buffer
 * (module.c:44-59; util.c:239-269).  mode: FX_REVERSE | FX_COMPLEMENT.        */
int fx_revcomp(int device, int where, uint8_t *buf, int64_t n, int mode);

/* ------------------------------------------------------------ gzip inputs
 * fx_open_file inflates BGZF (bgzip) inputs on the GPU, one work-item per
 * member; other gzip files are inflated by zlib on the host (a single deflate
 * stream is serial).  fx_gz_points lists restart points for the .fxi `gzindex`
 * table (pyfastx_build_gzip_index / pyfastx_gzip_index_export, util.c:442-540,
 * 728-742): for BGZF, member boundaries about `spacing` uncompressed bytes apart
 * (cmp_off = the first byte of the member's deflate data, where zran_seek starts a raw
 * inflate; bit offset 0, no 32 KiB window needed).  Call with cap = 0 to get the count.
 * Non-BGZF inputs report 0 points here: see fx_gz_checkpoints.                 */
int fx_gz_points(fx_handle *h, int64_t spacing, int64_t *cmp_off, int64_t *uncmp_off, int64_t cap,
                 int64_t *n_out, int64_t *compressed_size);

/* The first open of a single gzip stream runs on all cores of the host (fx_pgzip.hpp: block starts searched behind T cuts
 * of the compressed bytes, the pieces decoded with markers for the 32 KiB in front of them, resolved in order; CRC-32 and
 * ISIZE checked; restart points captured) -- zran_build_index's serial pass (util.c:728-742, index.c:383) in parallel.
 * fx_open_file uses it by itself (FX_GZIP_SERIAL=1: zlib on one core, as before); this entry is the same code without
 * a device: 0 done, 1 not a case for it (small file, several members, nothing it is sure of: inflate serially),
 * FX_ERANGE when `out` is too small (*out_n then says how much is needed). */
int fx_gunzip_parallel(const uint8_t *in, int64_t n, int threads, uint8_t *out, int64_t cap, int64_t *out_n, int64_t *n_points);
/* how the open that made this handle inflated a gzip input: 0 plain, 1 BGZF on the device, 2 one stream serially (zlib),
 * 3 one stream on all host cores, 4 from the restart points of its index file (diagnostics) */
int fx_gz_open_mode(const fx_handle *h);

/* How the members of a BGZF file were inflated by the open that made this handle: out = {members, members the
 * wave-per-member decoder handed over to the serial one, INFL_RETRY + reason of the first of those} (fx_inflate_par.hpp:
 * the lanes of a wave start at 64 bit positions of a member and fall into step by Huffman self-synchronisation; anything
 * out of the ordinary, damaged members included, is decoded by one lane).  Diagnostics; replaces nothing in the reference. */
int fx_bgzf_counts(fx_handle *h, int64_t out[3]);

/* Single-stream gzip (not BGZF): the restart points zran would build (pyfastx_build_gzip_index, util.c:728-742; spacing
 * 1 MiB, window 32 KiB, index.c:70) are captured while fx_open_file inflates the stream on the host -- at deflate block
 * boundaries at least 1 MiB of output apart: offset of the next compressed byte, number of bits of the byte before it
 * that still belong to the point (zran's `bits`), offset in the inflated stream, and the 32 KiB of output before it
 * (point 0 is the start of the deflate data and has none).  fx_gz_checkpoints hands them out for the gzindex table
 * (windows: 32768 bytes per point with has_data, in order; call with cap = 0 for the counts);  fx_open_file_indexed is
 * fx_open_file with the points of an existing index: the segments between them are inflated by many host threads at
 * once, each a raw inflate primed with its bits and window (zran_seek + zran_read of index.c:685-686, for every
 * segment at the same time).  Points that do not describe the file: the serial inflate, silently.  indexed_gzip is
 * not part of the reference tree; the compiled reference of the tests imports these rows (util.c:542-726) and serves
 * its reads from them through a zran work-alike (oracle/refshim): offsets, bits and windows are pinned
 * that way, only the PLACEMENT real zran would choose for its points is not. */
int fx_gz_checkpoints(fx_handle *h, int64_t cap, int64_t *cmp_off, int64_t *uncmp_off, uint8_t *bits, uint8_t *has_data,
                      uint8_t *windows, int64_t *n_out, int64_t *n_windows);
int fx_open_file_indexed(const char *path, int device, int64_t n_points, const int64_t *cmp_off, const int64_t *uncmp_off,
                         const uint8_t *bits, const uint8_t *has_data, const uint8_t *windows, int64_t uncompressed_size,
                         fx_handle **out);

/* ------------------------------------------------------------ .fxi bulk load
 * Host-side.  Replaces the per-record `sqlite3_step(INSERT)` of index.c:239-251 / fastq.c:136-149 for the one big
 * table of an index file: rows arrive in rowid order, so the table b-tree (leaf pages left to right, a few interior
 * pages on top) is written straight into the database file that SQLite created.  `path`: a database with the
 * schema in place and NO open connection; `rootpage`: sqlite_master.rootpage of the (empty) table; rows i = 0..n-1
 * get rowid i+1 and are (NULL [the INTEGER PRIMARY KEY], names[name_off[i] .. name_off[i+1]) as TEXT, cols[0][i], ...
 * cols[ncols-1][i] as INTEGER).  FX_ERANGE: some row needs an overflow page -- use INSERTs instead.  The UNIQUE
 * INDEX is created by SQLite afterwards. */
int fx_fxi_bulk_rows(const char *path, int rootpage, int64_t n, const uint8_t *names, const int64_t *name_off,
                     int ncols, const int64_t *const *cols);

/* The UNIQUE INDEX on the name column (index.c:363 `CREATE UNIQUE INDEX chromidx`, fastq.c:152 `readidx`) loaded the
 * same way: `rootpage` of the (empty) index; names / name_off as given to fx_fxi_bulk_rows; order[i] = 0-based row of
 * the i-th smallest name (memcmp order, the shorter first on a common prefix = SQLite's BINARY collation;
 * fx_names_sort produces it on the GPU and reports whether the names are distinct -- only then may this be used).
 * FX_ERANGE: an entry would need an overflow page -- let SQLite build the index. */
int fx_fxi_bulk_index(const char *path, int rootpage, int64_t n, const uint8_t *names, const int64_t *name_off,
                      const int64_t *order);
/* A non-unique INDEX on an INTEGER column (fasta.c:952 `CREATE INDEX seqidx ON comp (seqid)`): key[row], order[i] =
 * row of the i-th entry in (key, rowid) order.  fx_fxi_bulk_rows with names = name_off = NULL loads a table without a
 * TEXT column (`comp`: rowid, then cols[] as INTEGERs). */
int fx_fxi_bulk_index_int(const char *path, int rootpage, int64_t n, const int64_t *key, const int64_t *order);

/* The same two b-trees formatted ON THE DEVICE (round 5, csrc/fx_fxi_dev.hpp): the record table of the handle's last
 * build, the names where they are in the resident stream and the sorted order never leave HBM -- only finished 4 KiB
 * pages cross PCIe and go into the file (pinned pieces, several copy threads, fallocate running ahead of them).  Replaces
 * the INSERT loop and CREATE UNIQUE INDEX of fastq.c:29-60, 136-171 (`read`, `readidx`) and index.c:178-207, 239-251, 363
 * (`seq`, `chromidx`) for a NEW index file.
 *   fx_fxi_dev_sort:  kind 0 = FASTA table, 1 = FASTQ table; the BINARY-collation order of the record names is computed
 *                     and kept in the handle; *n_dup = adjacent equal pairs (> 0: the names are not distinct, SQLite's
 *                     CREATE UNIQUE INDEX would fail and the reference ignores that: write the table only).
 *   fx_fxi_dev_write: `path` = a database with the schema in place and NO open connection, 4 KiB pages;
 *                     root_table / root_index = sqlite_master.rootpage of the empty table / of the empty UNIQUE INDEX on its
 *                     name column (0: no index; else fx_fxi_dev_sort must have run).  laps (8 doubles, may be NULL), seconds:
 *                     [0] table shape, [1] table leaf kernels, [2] table leaves to the file, [3] file grown and allocated
 *                     (fallocate), [4] index shape + the dividers for the upper levels, [5] index leaf kernels, [6] index
 *                     leaves to the file, [7] rest of the host's levels + header; filled on every way out.  FX_ERANGE: a row / entry needs an overflow page (or
 *                     >= 2^32 records) -- nothing usable was written, use the host loaders or INSERTs; FX_EINVAL: not a
 *                     database this loader can extend (other page size, reserved bytes, auto-vacuum). */
int fx_fxi_dev_sort(fx_handle *h, int kind, int64_t *n_dup);
int fx_fxi_dev_write(fx_handle *h, int kind, const char *path, int root_table, int root_index, double *laps);
/* Both in one call (round 6), the sort and the shape of the index computed BESIDE the copy-out of the table's leaves (a second
 * stream, a second thread: the device is idle while 6 GB of pages cross PCIe).  The schema must hold the empty UNIQUE INDEX
 * already (root_index >= 2) -- whether the names are distinct is only known when the sort is done: *n_dup > 0 means no index
 * was written and the caller drops the empty one (fastq.c:152-156 / index.c:363-366 ignore the failed CREATE UNIQUE INDEX).
 * laps as fx_fxi_dev_write, [4] = what of sort + index shape the table's copy-out did NOT hide. */
int fx_fxi_dev_build(fx_handle *h, int kind, const char *path, int root_table, int root_index, int64_t *n_dup, double *laps);
/* Room for those pages set aside while the stream is still being staged: `path` = the database SQLite has just created
 * (schema in place, no open connection); a thread of the library grows the file to `bytes` with fallocate (on tmpfs the
 * allocation of 10 GB takes 0.6 s and must not run beside the stores into the file; beside the staging it costs nothing);
 * device >= 0: the thread runs on the CPUs next to that device, so that the pages lie in the memory the copy threads of
 * fx_fxi_dev_write are next to (-1: wherever).
 * The database header keeps saying where the database ends; fx_fxi_dev_write uses the room and cuts the file to what it
 * needed.  fx_fxi_presize_end waits for the thread (cancel != 0: stops it at the next 256 MiB step first).  An estimate
 * that is too small only means the rest is allocated by fx_fxi_dev_write.  No counterpart in the reference: its index
 * file grows one INSERT at a time (fastq.c:136-149). */
int fx_fxi_presize_begin(const char *path, int64_t bytes, int device, void **token);
int fx_fxi_presize_end(void *token, int cancel);

/* ONE index file from SEVERAL handles (round 6): a file indexed by byte range -- one process per GPU, the
 * devices of one process, or windows of one device that take turns -- has the rows of `read` / `seq` in several handles;
 * part r holds rows [row_base_r, row_base_r + n_r), in order.  Every part formats ITS table leaves on its own device and
 * copies them into its own page range of the one file; the index needs all names in one order, so every part hands its
 * names to device memory the caller moves to the writing rank (the process group's gather: RCCL over xGMI), which sorts
 * them once and formats the index leaves from that buffer.  Replaces, for a sharded build, the same reference loops as
 * fx_fxi_dev_write (fastq.c:29-60, 136-171; index.c:178-207, 239-251, 363).  Order of the calls:
 *   every part   fx_fxi_part_shape(h, kind, row_base, out3): out3 = rows, table leaves, bytes of names.  The caller adds up
 *                the leaves over the parts (they travel with the build's all-gather).
 *   writer       creates the database (schema + the empty UNIQUE INDEX), no open connection; fx_fxi_join_grow(path,
 *                root_table, all parts' leaves, extra_bytes, device, &first_new_page) makes room for the table's pages and
 *                extra_bytes behind them (an estimate of the index; best effort) and says where the new pages begin --
 *                every part needs that number.
 *   every part   fx_fxi_part_leaves(h, kind, path, first_new_page, leaves of the parts before this one, laps2): kernels +
 *                copy-out into the file (laps2: seconds in the kernels, in the copies).  The parts may run at the same
 *                time, from different processes.  A table with ONE leaf in all: leaf_base = -root_table (it lives in
 *                the root page).
 *   every part   fx_fxi_part_names(h, kind, d_names, d_lens): DEVICE pointers on the handle's device, room for out3[2] + 64
 *                bytes and out3[0] lengths; fx_fxi_part_firsts(h, first_rows): 0-based first row of each of its leaves
 *                (host, out3[1] values) for the table's interior pages.
 *   writer       fx_fxi_join_begin(device, all names back to back in part order, all lengths, n, &j, &n_dup): one sort;
 *                n_dup > 0: the names are not distinct, write no index (fastq.c:152-156 ignores the failure of CREATE
 *                UNIQUE INDEX) -- pass root_index = 0 below and drop the empty index from the schema.
 *                fx_fxi_join_write(j, path, root_table, root_index, rows, table leaves, first_rows of all parts in order,
 *                first_new_page, laps6) once every part's fx_fxi_part_leaves has returned: the table's interior levels,
 *                the index (leaves on the device, upper levels on the host), the header; laps6: file grown, index shape +
 *                dividers, index leaf kernels, index leaves to the file, host levels + header, table interior.
 *                fx_fxi_join_end(j).
 * FX_ERANGE from any of them: a row / entry needs an overflow page -- remove the file and use the host loaders. */
typedef struct fx_fxi_join fx_fxi_join;
int fx_fxi_part_shape(fx_handle *h, int kind, int64_t row_base, int64_t *out3);
int fx_fxi_part_firsts(fx_handle *h, int64_t *first_rows);
int fx_fxi_part_names(fx_handle *h, int kind, uint8_t *d_names, int32_t *d_lens);
int fx_fxi_part_leaves(fx_handle *h, int kind, const char *path, int64_t first_new_page, int64_t leaf_base, double *laps);
int fx_fxi_join_grow(const char *path, int root_table, int64_t nleaf_table, int64_t extra_bytes, int device, int64_t *first_new_page);
int fx_fxi_join_begin(int device, const uint8_t *d_names, const int32_t *d_lens, int64_t n, fx_fxi_join **out, int64_t *n_dup);
int fx_fxi_join_write(fx_fxi_join *j, const char *path, int root_table, int root_index, int64_t n_rows, int64_t nleaf_table,
                      const int64_t *first_rows, int64_t first_new_page, double *laps);
void fx_fxi_join_end(fx_fxi_join *j);

/* ------------------------------------------------------- sync and timing
 * Calls that take FX_DEVICE arrays return after ENQUEUEING work on the
 * handle's stream; fx_sync waits for it.  (FX_HOST calls are synchronous.)   */
int fx_sync(fx_handle *h);

/* Optional per-kernel timing with HIP events on the handle's own stream
 * (what bench.py's roofline leg reads).  Kernel ids 0..fx_prof_count()-1,
 * names from fx_prof_name (they match the rocprofv3 kernel names).           */
int fx_prof_enable(fx_handle *h, int on);      /* 0 off, 1 every kernel, 2 only k_scan (2 events per build) */
int fx_prof_default(int on);   /* handles opened afterwards start with timing on (covers k_bgzf_inflate in fx_open_file) */
int fx_prof_reset(fx_handle *h);
int fx_prof_count(void);
const char *fx_prof_name(int id);
int fx_prof_read(fx_handle *h, int id, double *total_ms, int64_t *launches);

/* ----------------------------------------------------- multi-GPU stitching
 * Boundary summary of this shard for the single all-gather of SURVEY 8e.
 * Fixed size, plain integers; valid after fx_fasta_build / fx_fastq_build on
 * a handle configured with fx_set_shard.                                      */
typedef struct {
    int64_t base, n_bytes, is_last;
    int64_t n_nl;              /* entries of the shard's line table (virtual EOF newline included) */
    int64_t first_nl, second_nl, last_nl;  /* global offsets, -1 if absent                          */
    int64_t first_nl_prev;     /* byte before first_nl; -1 if first_nl == base (= previous shard's last_byte) */
    int64_t first_byte, last_byte;
    int64_t n_hdr;             /* FASTA header lines that START in the shard                        */
    int64_t first_hdr, last_hdr;
    int64_t lead_nl;           /* newlines before first_hdr (all of them if n_hdr == 0)             */
    int64_t lead_ws;           /* first ' ' or '\t' in [base, first_nl) (the whole shard if it has no newline), -1 if none */
    int64_t lead_v1, lead_c1;  /* lead lines with both newlines in the shard: the first two ...     */
    int64_t lead_v2, lead_c2;  /* ... distinct (len+1) values and how many lines have them          */
    /* the last record that starts in this shard, as far as the shard can tell */
    int64_t tail_e;            /* newline ending its header line, -1 if that is in a later shard    */
    int64_t tail_first_end;    /* newline ending its first sequence line, -1 if later               */
    int64_t tail_nl_after;     /* shard newlines after tail_e                                       */
    int64_t tail_bad;          /* bad lines counted locally (valid when tail_first_end >= 0)        */
    int64_t tail_elen, tail_dlen, tail_name_len;   /* dlen -1: header unterminated; name_len -1: no whitespace seen */
    int64_t lead_prev_nl;      /* second-to-last newline before first_hdr (of the shard if n_hdr == 0), -1 if lead_nl < 2   */
    int64_t second_last_nl;    /* second-to-last newline of the shard, -1 if n_nl < 2: with the field above, the length of
                                  the LAST line of a record that ends in a later shard (line-regular test, see above)     */
} fx_shard_summary;            /* 28 x int64: travels as one all-gather payload */

int fx_shard_summary_get(fx_handle *h, fx_shard_summary *out);

/* Device-resident variant of the same exchange, so that a sharded build never leaves the GPU between
 * the collective and the fetches: fx_shard_summary_dev ENQUEUES the summary (28 x int64) into d_out (a
 * device buffer of the caller, e.g. the send buffer of the all-gather); after the all-gather,
 * fx_fasta_stitch_dev ENQUEUES the completion of this rank's last record from the gathered summaries
 * d_all[world][28] (device) -- the integer logic of index.c:234-353 across shard cuts -- and rewrites
 * that row of the resident table.  Both run on the handle's stream: order them against the collective's
 * stream with fx_stream() (an opaque hipStream_t) and stream events.                                    */
int fx_shard_summary_dev(fx_handle *h, int64_t *d_out);
int fx_fasta_stitch_dev(fx_handle *h, const int64_t *d_all, int world, int rank, int full_name);
void *fx_stream(fx_handle *h);

/* After the all-gather the owner of a record that crosses shard cuts rewrites
 * that row of the resident table (and of what fx_fasta_table returns).  norm: bit 0 = the norm column, bit 1 = the
 * line-regular bit of that record (fx_fasta_line_regular). */
int fx_fasta_set_row(fx_handle *h, int64_t k, int64_t boff, int64_t blen, int64_t slen, int64_t llen,
                     int32_t elen, int32_t norm, int32_t dlen, int32_t name_len);

/* Host side of a batched fetch over byte-range shards (the "Fetch" half of SURVEY 8e; no device work, no handle):
 * n queries (record id, 0-based [start, stop)) against the GLOBAL record table -> byte ranges of the global stream by
 * the reference's line arithmetic (sequence.c:498-510: line-regular records exactly the bytes; the others the whole
 * record, sliced after despacing, sequence.c:100-110) -> the shard [bases[r], ends[r]) that holds the first byte of
 * each (that rank answers it) and the number of shards the range touches.  Outputs are in ROUTED order -- by
 * answering shard, then by position in the batch: order[k] = index of the query at routed position k;
 * shard_start[r] .. shard_start[r + 1] = the routed positions of shard r (n_shard + 1 entries); off / len / skip /
 * take / fl[k] = what fx_fetch_slices takes for that query (fl: flags_per_query or `flags`), cnt[k] = shards touched
 * (0: empty range or past the end of the stream, fread semantics index.c:689; > 1: the range crosses a cut and its
 * pieces are put together by the caller).  Replaces per-batch numpy passes of the Python layer (29 ms per 1 M
 * queries in round 1). */
int fx_shard_route(int64_t n, const int64_t *ids, const int64_t *starts, const int64_t *stops,
                   int64_t n_rec, const int64_t *boff, const int64_t *blen, const int64_t *llen, const int64_t *elen,
                   const uint8_t *reg, int n_shard, const int64_t *bases, const int64_t *ends,
                   int flags, const uint8_t *flags_per_query,
                   int64_t *order, int64_t *shard_start, int64_t *off, int64_t *len, int64_t *skip, int64_t *take,
                   uint8_t *fl, int32_t *cnt);

/* ------------------------------------------------- the collective under the C ABI
 * pyfastx_create_index (index.c:109-388) and pyfastx_fastq_create_index (fastq.c:8-182) scan one file in one
 * thread; the reference's only parallel story is "re-open per process" (docs/advance.rst:1-40).  Here a whole-file
 * build shards by byte range over the GPUs of a node, ONE process per GPU, and the ONE exchange it needs -- the
 * all-gather of the 28-word boundary summaries (RCCL over xGMI) -- lives in this library, so that a C caller
 * (multi-GPU) needs no Python and no torch:
 *
 *     rank 0: fx_comm_unique_id(id);  ... id reaches every rank (file, pipe, MPI_Bcast, env) ...
 *     all:    fx_comm_init(rank, world, id, device, &c);
 *             fx_open_file_range(path, size * rank / world, size * (rank + 1) / world - size * rank / world, 0, device, &h);
 *             fx_fasta_build_sharded(h, c, full_name, &summary);      rows of the records that START in this range,
 *             fx_fasta_table(h, FX_HOST, ...);                        the one that crosses the cut completed
 *
 * RCCL is loaded at run time (dlopen librccl.so.1, or the copy the process already carries; FX_RCCL_LIB overrides):
 * a single-GPU user never loads it; without it these entries return FX_EDEVICE.                               */
typedef struct fx_comm fx_comm;
int fx_comm_unique_id(uint8_t id[128]);                       /* ncclGetUniqueId: once, on one rank */
int fx_comm_init(int rank, int world, const uint8_t id[128], int device, fx_comm **out);   /* ncclCommInitRank: all ranks */
int fx_comm_destroy(fx_comm *c);
int fx_comm_rank(const fx_comm *c);
int fx_comm_world(const fx_comm *c);
/* nbytes (<= 65536) of every rank to every rank, host buffers (recv: world x nbytes) */
int fx_comm_allgather(fx_comm *c, const void *send, void *recv, int64_t nbytes);
/* scan + tables + boundary summary + ncclAllGather + stitch, all enqueued on the handle's stream; _begin returns at
 * once (device-side consumers may follow), fx_fasta_build_end reads the totals; full_name as in fx_fasta_build.    */
int fx_fasta_build_sharded_begin(fx_handle *h, fx_comm *c, int full_name);
int fx_fasta_build_sharded(fx_handle *h, fx_comm *c, int full_name, fx_fasta_summary *out);
int fx_comm_summaries(fx_comm *c, fx_handle *h, fx_shard_summary *out);    /* world entries, as the all-gather delivered them */
/* FASTQ: count pass, all-gather of (newlines of the core, last newline) per rank, rows with the global line numbering
 * (fx_set_halo first: a record that begins in the core is finished from the halo) */
int fx_fastq_build_sharded(fx_handle *h, fx_comm *c, fx_fastq_summary *out);

#ifdef __cplusplus
}
#endif
#endif
