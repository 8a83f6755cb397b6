/*
 * mdbg_hip.h -- C ABI of libmdbg_hip.so: metaMDBG's read -> minimizer -> k-min-mer hot path
 * as hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference has no FFI: its boundary is two child processes (`readSelection`, `graph`)
 * talking through files.  Each entry point below replaces the
 * compute inside one reference function, cited as file:line under /root/reference/src, and is
 * what a maintainer would call from that function (binding stubs: INTEGRATION.md).
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * MDBG_E* code, with a message available from mdbg_last_error(); objects are opaque handles
 * owned by the library and released with the matching *_free; a context is bound to one HIP
 * device and one stream and is not thread-safe (use one context per host thread / stream,
 * as the reference uses one functor copy per OpenMP thread: Commons.hpp:5846-5914).
 * Several contexts on one device may be driven concurrently from several threads; that is the intended way to keep
 * two or three batches in flight (the table kernels of one batch overlap the scan of the next -- bench.py).
 * mdbg_scan calls on the same device take turns: one scan kernel runs at a time, also across processes (an advisory file lock named
 * after the device's PCI address; MDBG_SCAN_NO_XPROC_LOCK=1 keeps the rule inside the process).
 * There is no CPU fallback: without a usable GPU every call fails with MDBG_ENODEV.
 *
 * Environment (read by the library): MDBG_SCAN_READS_PER_WAVE, MDBG_TABLE_BLOCKS_PER_CU -- defaults of the options of
 * mdbg_set_option; MDBG_TRACE -- one line per purge with the number of suspect reads.
 */
#ifndef MDBG_HIP_H
#define MDBG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDBG_OK        0
#define MDBG_EINVAL   -1   /* bad argument */
#define MDBG_ENODEV   -2   /* no HIP device / wrong architecture */
#define MDBG_ENOMEM   -3   /* device or host allocation failed */
#define MDBG_EHIP     -4   /* HIP runtime error (see mdbg_last_error) */
#define MDBG_ERANGE   -5   /* size exceeds an internal limit (see message) */
#define MDBG_EPEER    -6   /* collective calls: another rank reported a failure; this rank's data is intact, nothing was exchanged */

typedef struct mdbg_ctx mdbg_ctx;
typedef struct mdbg_reads mdbg_reads;             /* base-space reads resident in HBM, 2-bit packed */
typedef struct mdbg_minimizers mdbg_minimizers;   /* minimizer-space reads resident in HBM (CSR) */
typedef struct mdbg_table mdbg_table;             /* k-min-mer table resident in HBM */

/* ---- context ------------------------------------------------------------------------- */
int  mdbg_create(int device, mdbg_ctx **ctx);
void mdbg_destroy(mdbg_ctx *ctx);
const char *mdbg_last_error(const mdbg_ctx *ctx);      /* ctx may be NULL: last creation error of the calling thread */
int  mdbg_synchronize(mdbg_ctx *ctx);
/* Queues a kernel of one wave that idles for `microseconds` on the context's stream and returns at once.  HIP multiplexes streams
 * onto a few hardware queues; two contexts whose streams share one never overlap their kernels.  A caller that keeps several
 * batches in flight on one device finds out by spinning on two contexts at once: different queues finish together, a shared
 * queue takes twice as long (bench.py's overlap probe; no reference analogue -- the reference's threads share one CPU scheduler). */
int  mdbg_stream_spin(mdbg_ctx *ctx, uint32_t microseconds);
void *mdbg_stream(mdbg_ctx *ctx);                       /* the hipStream_t every launch goes to */
int  mdbg_device_info(mdbg_ctx *ctx, char *arch, size_t arch_len, int *n_cu, uint64_t *hbm_bytes);
int  mdbg_device_clock_khz(mdbg_ctx *ctx, int *clock_khz);   /* peak engine clock (hipDeviceProp_t::clockRate) */
/* Per-context tuning, value <= 0 restores the default:
 *   "table_blocks_per_cu"   resident blocks per CU of the kernels that walk every k-min-mer instance (default: unlimited;
 *                           1..3 when several contexts share a device, so that they do not displace another context's scan)
 *   "table_grid_blocks"     g > 0: those kernels run as exactly g workgroups (grid-stride), e.g. half a block per CU beside a scan;
 *                           0 (default): "table_blocks_per_cu" decides
 *   "table_cu_count"        c > 0: every kernel of the context except the block-structured scan kernel is confined to c compute
 *                           units (spread over the XCDs), the scan kernel runs on a stream of its own over all of them; for
 *                           several contexts in flight on one device (the other batches' table kernels then displace a running
 *                           scan on those CUs only).  Call it between steps: it synchronises and re-creates the stream, so a
 *                           handle obtained from mdbg_stream before is dead.  Default 0: one unconfined stream
 *   "pool_cache_percent"    the context keeps freed device blocks for reuse up to this share of the device memory (default 55:
 *                           several contexts share a device; a context that has the device to itself may take 90)
 *   "pool_trim"             any value: the blocks kept for reuse are given back to the device now
 *   "scan_reads_per_wave"   reads a scan wave processes before it retires; 0 (the default) = each kernel's own: 2, and for the pre-filtered
 *                           variant up to 32 by the batch's size (a workgroup's set-up is paid once per chunk of 16 x that many reads)
 *   "scan_candidate_slack"  tests only: the block-structured scan records candidate positions by the upper half of the
 *                           hash and confirms each with the full hash; a read with a false candidate is re-run.  False
 *                           candidates occur about once in 2^31 positions; this widens the test (units of 2^32 of the
 *                           hash range) so that the re-run path can be exercised.  Default 0; results never depend on it
 *   "scan_guard_slack"      tests only: the block-structured scan hashes a position with the two finalisers' upper half shared, which
 *                           is exact unless a guard word is below 68; a lane that saw one walks its span again with the exact test.
 *                           This raises the 68 (clamped to [0, 2^32 - 69]; 2^31 sends practically every span down the exact walk) so
 *                           that the slow path can be exercised.  Default 0; results never depend on it
 *   "scan_prefilter"        1 (default; negative too) = the block-structured scan takes its pre-filtered variant where that applies:
 *                           homopolymer compression, minimizer_size 15, no qualities, the two slacks above 0, a batch whose average
 *                           read is expected to select fewer rows than that variant stages (176: 27 kb at density 0.005) and whose reads
 *                           above that length hold at most 1/32 of its bases (the four-wave kernel scans those in the same call), a bitmap of
 *                           the selected keys at most a quarter full (densities up to about 0.013) and room for one workgroup of 16 or
 *                           8 waves beside "scan_lds_reserve".  The variant asks a 64 KB bitmap in LDS whether a position's key can be
 *                           selected and hashes only the positions that pass; the bitmap is built on the device when the density
 *                           changes and kept with the context.  0 = never (the four-wave kernels, as before).  The environment variable
 *                           MDBG_SCAN_PREFILTER=0 / 1 sets the default of new contexts.  Results never depend on it; mdbg_scan_info
 *                           tells which kernel ran
 *   "scan_prefilter_log2_bits"  tests only: the bitmap is built and probed with 2^value bits (10 .. 19; 0 = the kernel's own 2^19) and
 *                           used whatever its fill, so that nearly every position reaches the confirmation with the full hash and its
 *                           list overflows.  Results never depend on it
 *   "scan_confirm_table"    1 = the pre-filtered variant takes the exact verdict of a position that passed its bitmap from a table of
 *                           the selected keys in global memory (1 MB: 2^16 buckets of seven 16-bit tags, one 16-byte load a candidate; built
 *                           on the device beside the bitmap, rebuilt and freed with it) instead of hashing the key; a key of a bucket that
 *                           holds more than seven -- none at density 0.005, a handful at 0.01 -- is hashed as before.  0 (default) = every candidate
 *                           is hashed: alone the kernel is 0.3 - 1.1 % faster with the table, beside another batch's table kernels it is not
 *                           (DESIGN.md 4.1).  The environment variable MDBG_SCAN_CONFIRM_TABLE=0 / 1 sets the default of new contexts.  Results
 *                           never depend on it; mdbg_scan_confirm_info tells which path ran
 *   "scan_confirm_table_log2_buckets"  tests only: the table is built and probed with 2^value buckets (10 .. 16; 0 = the kernel's own 2^16), so
 *                           that most buckets overflow and looked-up and hashed verdicts mix in one round.  Results never depend on it
 *   "scan_persistent"       1 (default) = the pre-filtered variant is launched with as many workgroups as fit the device at once (one per
 *                           CU, fewer for a small batch) and none pending behind them; its waves draw runs of consecutive reads from one
 *                           64-bit counter in device memory until it is used up, and rows go to the region of their read's run: alone 3 %
 *                           faster on 10 kb reads and 6 % on reads of 1 - 25 kb, the benchmark's step 2 %.  0 = the chunked
 *                           form: a workgroup per chunk of reads, dealt out by the dispatcher.  An explicit non-zero "scan_reads_per_wave"
 *                           (or MDBG_SCAN_READS_PER_WAVE) names the chunked form and gets it whatever this says.  A context with
 *                           "scan_lds_reserve" > 0 and "partition_threads" 0 whose last block-kernel scan was such a launch also takes the
 *                           four-wave split kernels (below), which fit beside a scan workgroup that never retires.
 *                           MDBG_SCAN_PERSISTENT=0 / 1 sets the default of new contexts.
 *                           Results never depend on it (the rows' places do); mdbg_scan_persistent_info tells which form ran
 *   "scan_grab_reads"       consecutive reads a wave of the persistent launch draws at a time (1 .. 65536); 0 (default) = the library's own, 4.
 *                           MDBG_SCAN_GRAB_READS sets the default of new contexts
 *   "scan_persistent_blocks"  tests only: at most this many workgroups in a persistent launch (0 = no cap), so that the waves of a small
 *                           batch draw many runs.  Results never depend on it
 *   "prefix_small_limit"    tests only: the block sums (one per 4096 items) up to which one workgroup scans the middle level of a prefix scan; more are
 *                           scanned recursively (1 .. 65536, larger values are 65536; 0 or a negative value restores the default, 65536: above
 *                           2^28 items).  Results never depend on it
 *   "scan_segments"         long reads, contigs and unitigs cut into segments that the block-structured scan takes one wave each: a plain read
 *                           (no N, no case flip) of more than one segment is scanned as several views -- each owns the windows that start
 *                           in its segment and reads one 2048-base tile on behind it -- and the views' rows are joined in read order.
 *                           1 (default; negative too) = automatic: only in a batch that would otherwise leave the block-structured kernels
 *                           because of its reads' length alone (the average read expected to select more rows than a wave stages, 384:
 *                           about 64 kb at density 0.005) -- such a batch stays on them with its long reads cut; 0 = never (the routing
 *                           as before); 2 = what 1 does, and every such read in any batch that takes the block-structured kernels.  A read with a cut
 *                           behind which 2048 bases hold fewer than minimizer_size run starts (a homopolymer of about 2000 bases) stays
 *                           whole, and a read one of whose views outgrows its stage goes whole the way outgrown reads go.  The
 *                           environment variable MDBG_SCAN_SEGMENTS=0 / 1 / 2 sets the default of new contexts.  Results never depend
 *                           on it; mdbg_scan_info tells how many reads were cut
 *   "scan_segment_bases"    raw bases of a segment: a multiple of 2048 (anything else is MDBG_EINVAL); <= 0 restores the default, 16384
 *                           (expected to select 16384 * 0.005 * 0.8 * 1.4 + 24 = 116 rows, inside the pre-filtered variant's stage of
 *                           176).  The views are scanned by the variant a batch of reads of that length would take
 *   "index_tuning"          the passes above firstK over the one-slot tables (bits; default 19; negative: the default): 1 = a slot's key and
 *                           value fetched in one trip, 2 = the insert first looks at a window's home slot with plain loads (a key found
 *                           there is done without an atomic), 4 = two windows of a lane in flight (measured: no gain), 8 = look-up and
 *                           insert in one kernel (measured: slower), 16 = both slots of a key's home sector fetched at once (look-up
 *                           and the insert's first look), 32 = 32 lanes a sequence instead of 16, 128 = always insert first and look the
 *                           previous table up only for the k-windows not seen in the new one, 256 = never (neither: a sample of the
 *                           sequences decides per pass -- insert first when fewer than 0.45 of the windows are never inserted);
 *                           0 = the kernels of rounds 1 - 4.  Results never depend on it
 *   "keep_index_table"      1 (default) = the hash table an index pass filled stays with its result as the look-up structure the next
 *                           pass reads; 0 = it is dropped and built again from the rows on first use (rounds 1 - 5)
 *   "index_table_form"      0 = those passes over bucket tables (three keys per 64-byte sector: a third of the bytes, measured no
 *                           faster), 1 or negative = one 32-byte slot per key (default)
 *   "refined_form"          0 = k = firstK+1 done like an index pass (a look-up per (k-1)-window; measured slower), 1 or negative =
 *                           every distinct key first, then two look-ups per key (default)
 *   "scan_quality_stream"   FASTQ: 1 (default) = the per-read quality sums run beside the scan kernel on a side stream, 0 = in front of it
 *   "test_exchange_fail_phase"  tests only: this rank fails inside the next mdbg_shard_exchange before the counts travel (1),
 *                           when the receive buffers are allocated (2) or in the owner's reduction (3); one-shot
 *   "test_corrupt_replies"  tests only: the next exchange hands back one reply with a wrong count; one-shot
 * The environment variables MDBG_TABLE_BLOCKS_PER_CU / MDBG_SCAN_READS_PER_WAVE set the defaults at mdbg_create. */
int  mdbg_set_option(mdbg_ctx *ctx, const char *name, int64_t value);

/* Profiling aid: accumulated HIP-event time (ms) and launch count of the kernel named
 * `kernel` ("scan", "kminmer_insert", ...) since the last reset; events are recorded on
 * the context's stream only while timing is enabled. */
int  mdbg_timing_enable(mdbg_ctx *ctx, int on);
int  mdbg_timing_reset(mdbg_ctx *ctx);
int  mdbg_timing_get(mdbg_ctx *ctx, const char *kernel, double *ms_total, uint64_t *launches);

/* ---- base-space reads ---------------------------------------------------------------- */
/* Replaces the per-read copy in ReadParserParallel::parse (Commons.hpp:5868-5905): the caller
 * hands a batch of parsed reads (ASCII, concatenated; read r = bases[offsets[r] .. offsets[r+1]))
 * and optional phred+33 qualities with the same offsets (NULL for FASTA).  The batch is packed
 * to 2 bits/base (code (c>>1)&3, utils/kmer/Kmer.hpp:462) on the device.  Characters with
 * bit 3 set (N, n) are kept in a side bitmask, and so is every place where two neighbouring characters
 * differ although their codes agree ("aA", IUPAC letters): the reference's homopolymer compression compares
 * raw characters (Commons.hpp:4177-4178), and so does this path -- any byte string gives the reference's
 * minimizers.  Batches of plain upper-case ACGT carry neither mask and take the fast kernel variant. */
int  mdbg_reads_from_ascii(mdbg_ctx *ctx, const char *bases, const char *quals, const uint64_t *offsets,
                           uint32_t n_reads, mdbg_reads **out);
/* Already packed on the host: words[] holds 32 bases per u64 (base i of a word at bits [2i,2i+2)),
 * read r occupies words[word_offsets[r] .. word_offsets[r+1]) and starts on an even word.  The packed form
 * cannot say more than the code: use it for reads made of A, C, G, T only (the host feed does). */
int  mdbg_reads_from_packed(mdbg_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets,
                            const uint32_t *lengths, uint32_t n_reads, mdbg_reads **out);
/* The same without waiting for the copies: they are queued on an upload stream of the context (a copy engine: they run beside
 * the kernels of the context's own stream) and the call returns (offsets and lengths are copied before it does; the words are
 * what travels behind the caller's back).  `words` must stay untouched until
 * mdbg_reads_wait returns (or the reads are freed); page-locked memory (mdbg_host_alloc) is what makes the copy asynchronous.
 * Calls that consume the reads order themselves after the upload: mdbg_scan on the device, without a host wait -- so a feeder
 * uploads batch i+1 while batch i is scanned, inside one context: the replacement of the reference's one-reader critical
 * section (Commons.hpp:5868-5905) is then bound by the link, not by link + kernels. */
int  mdbg_reads_from_packed_async(mdbg_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint32_t *lengths,
                                  uint32_t n_reads, mdbg_reads **out);
/* The few reads of a PACKED batch (mdbg_reads_from_packed / _async) that hold characters other than upper-case A, C, G, T -- an N,
 * a soft-masked stretch, an IUPAC letter: the 2-bit words alone lose what the reference still sees (invalid k-mers, utils/kmer/
 * Kmer.hpp:574-580; a change of character starts a homopolymer run, Commons.hpp:4177-4178).  The caller hands those reads again
 * as characters (ascending indices; read read_index[i] = ascii[ascii_offsets[i] .. ascii_offsets[i+1])) and the side masks of the
 * batch are derived from them on the device, exactly as mdbg_reads_from_ascii derives them for every read.  mdbg_scan then keeps
 * the batch on its fast kernel and sends only the marked reads through the general one.  Once per batch, before any scan. */
int  mdbg_reads_mark_ascii(mdbg_ctx *ctx, mdbg_reads *r, const uint32_t *read_index, uint32_t n_listed, const char *ascii,
                           const uint64_t *ascii_offsets);
/* Qualities for reads made by mdbg_reads_from_packed_async, queued behind their words (same rules: `quals` stays untouched until
 * mdbg_reads_wait; a read has one quality per base, checked at once against the lengths given at upload). */
int  mdbg_reads_attach_qualities_async(mdbg_ctx *ctx, mdbg_reads *r, const char *quals, const uint64_t *offsets);
int  mdbg_reads_wait(mdbg_ctx *ctx, const mdbg_reads *r);
/* Phred+33 qualities (Read::_qual) for reads made by mdbg_reads_from_packed: read r = quals[offsets[r] .. offsets[r+1]),
 * offsets[r+1] - offsets[r] must equal its length.  Once per reads object. */
int  mdbg_reads_attach_qualities(mdbg_ctx *ctx, mdbg_reads *reads, const char *quals, const uint64_t *offsets);
/* Seeded synthetic read set generated directly in HBM (bench/test harness; same generator as
 * metamdbg_amd/synth.py).  thresholds[s] = cumulative species weight as u64.  Per read position one u64 draw e decides:
 * e < ins_threshold an inserted base, then del_threshold a skipped genome base, then sub_threshold a substitution
 * (HiFi 0.1 % substitutions; ONT R10 1 % + 0.5 % + 0.5 %).  window = genome bases set aside per read
 * (>= read_len; ignored without indels). */
int  mdbg_reads_synthetic(mdbg_ctx *ctx, uint64_t seed, uint32_t n_reads, uint32_t read_len,
                          uint64_t first_read, const uint64_t *species_len,
                          const uint64_t *species_threshold, uint32_t n_species,
                          uint64_t sub_threshold, uint64_t ins_threshold, uint64_t del_threshold, uint32_t window,
                          int with_quality, mdbg_reads **out);
int  mdbg_reads_info(const mdbg_reads *r, uint32_t *n_reads, uint64_t *n_bases, uint64_t *n_words);
/* Copy read `index` back as ASCII (buffer of at least its length; quals may be NULL). */
int  mdbg_reads_get(mdbg_ctx *ctx, const mdbg_reads *r, uint32_t index, char *bases, char *quals, uint32_t *length);
/* A batch as the device holds it, read only (what the tests compare bit for bit; copies, no kernel): word_offsets n_reads + 1,
 * lengths n_reads, words n_words, the invalid and the break mask n_words each (bit i of word w is base 32 w + i of the read
 * that owns the word), the per-read masked flag n_reads, and the ascending list of masked reads, info[2] of them (size it by a
 * first call, or give it n_reads).  info = {has_invalid, has_break, n_masked, n_words}.  Any pointer may be NULL.  An array the
 * batch does not hold -- a mask released because no bit of it was set, a packed batch never marked -- is filled with zeros.
 * Waits for an upload still in flight, as mdbg_reads_get does. */
int  mdbg_reads_packed_to_host(mdbg_ctx *ctx, const mdbg_reads *r, uint64_t *word_offsets, uint32_t *lengths, uint64_t *words,
                               uint32_t *invalid, uint32_t *breaks, uint8_t *masked, uint32_t *masked_list, uint64_t info[4]);
/* Bulk export of reads [first, first+count) as concatenated ASCII: offsets gets count+1 entries
 * (relative to bases[0]); bases must hold the sum of their lengths (use mdbg_reads_info / a first
 * call with bases == NULL to size it: *n_bytes is always set). */
int  mdbg_reads_export_ascii(mdbg_ctx *ctx, const mdbg_reads *r, uint32_t first, uint32_t count,
                             char *bases, uint64_t *offsets, uint64_t *n_bytes);
/* The phred+33 bytes of reads [first, first+count), concatenated in read order (same offsets as mdbg_reads_export_ascii gives
 * for the bases: a read has one quality per base); *n_bytes is always set, quals may be NULL to size the buffer. */
int  mdbg_reads_export_qualities(mdbg_ctx *ctx, const mdbg_reads *r, uint32_t first, uint32_t count, char *quals, uint64_t *n_bytes);
void mdbg_reads_free(mdbg_reads *r);

/* ---- reads -> minimizers --------------------------------------------------------------- */
typedef struct {
    uint32_t minimizer_size;      /* l, <= 16            (Parameters::_minimizerSize) */
    float    density;             /* f32 as stored in parameters.gz (Parameters::_minimizerDensity_assembly) */
    int32_t  hpc;                 /* Parameters::_useHomopolymerCompression */
    float    min_read_quality;    /* --min-read-quality   (ReadSelection.hpp:901) */
    const uint32_t *repetitive;   /* host array: repetitiveMinimizers.bin contents, may be NULL */
    uint32_t n_repetitive;
    int32_t  apply_read_filters;  /* 1: complexity + quality filters of ReadSelectionFunctor (ReadSelection.hpp:890-915);
                                     0: bare MinimizerParser::parse as CountMinimizerFunctor uses it (:599-611) */
    int32_t  quality_window;      /* per-minimizer minimum quality over the ORIGINAL coordinates
                                     0: [rle[pos], rle[pos+l])    ReadSelectionFunctor   (ReadSelection.hpp:1135, :1302-1320)
                                     1: [rle[pos], rle[pos+l-1]]  the correction scan, ReadCorrection::ReadSelectionFunctor
                                                                  (ReadCorrection.hpp:2340, :2467-2481); used with
                                                                  density = _minimizerDensity_correction, apply_read_filters = 0 */
    int32_t  no_end_trim;         /* 0: MinimizerParser's default _trimBps = 1, the first and last l-mer of a read are never
                                     selected (utils/kmer/Kmer.hpp:1362, :1395); 1: _trimBps = 0 as GenerateGfa's
                                     LoadUnitigsFunctor sets it for unitig sequences (graph/GenerateGfa.hpp:366) */
    int32_t  ignore_qualities;    /* 1: the read set's qualities are not looked at, as if it had none (every minimizer's quality
                                     is 1, the mean read quality NaN): CountMinimizerFunctor's census of minimizer values
                                     (ReadSelection.hpp:565-625) over reads that are resident with their qualities */
} mdbg_scan_params;

/* Replaces, for a whole batch, EncoderRLE::execute + MinimizerParser::parse + complexity /
 * quality filters + per-minimizer min quality of ReadSelectionFunctor::operator()
 * (readSelection/ReadSelection.hpp:669-1158; utils/kmer/Kmer.hpp:1373-1456; Commons.hpp:4163-4203).
 * Output order = read order, minimizers of a read in position order. */
int  mdbg_scan(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_scan_params *params, mdbg_minimizers **out);

int  mdbg_minimizers_info(const mdbg_minimizers *m, uint32_t *n_reads, uint64_t *n_minimizers);
/* Host copies; any pointer may be NULL.  offsets has n_reads+1 entries; per-read arrays n_reads.
 * mean_quality is the f32 of ReadSelection.hpp:878-879 (NaN without qualities). */
int  mdbg_minimizers_to_host(mdbg_ctx *ctx, const mdbg_minimizers *m, uint64_t *offsets,
                             uint32_t *minimizers, uint32_t *positions, uint8_t *directions, uint8_t *qualities,
                             uint32_t *read_lengths, float *mean_quality, uint8_t *read_flags);
#define MDBG_READ_LOW_COMPLEXITY 1u
#define MDBG_READ_LOW_QUALITY    2u
/* Upload minimizer-space sequences (read_data_corrected.txt / unitig_data.txt contents as CSR). */
int  mdbg_minimizers_from_host(mdbg_ctx *ctx, const uint32_t *minimizers, const uint64_t *offsets,
                               uint32_t n_reads, mdbg_minimizers **out);
/* Device pointers for zero-copy consumers (torch.from_dlpack-style wrapping in the harness). */
int  mdbg_minimizers_device_ptrs(const mdbg_minimizers *m, const uint64_t **d_offsets, const uint32_t **d_minimizers);
void mdbg_minimizers_free(mdbg_minimizers *m);
/* The reads of `parts[0]`, then `parts[1]`, ... as one set, appended on the device (CSR offsets rebased; positions, directions,
 * qualities and the per-read fields follow when every part is a scan output).  For read sets scanned in several resident
 * pieces -- 10 M ONT reads with their qualities are 250 GB, more than fits beside their outputs -- whose palindrome purge and
 * k-min-mer table are over ALL the reads: the reference counts k-min-mers over the whole read_data_corrected.txt however the
 * reads were parsed (graph/CreateMdbg.cpp:290-328).  The parts stay valid and are not modified. */
int  mdbg_minimizers_concat(mdbg_ctx *ctx, const mdbg_minimizers *const *parts, uint32_t n_parts, mdbg_minimizers **out);
/* The other way round: reads [first_read, first_read + n_reads) of `in` as a set of their own (values and offsets; a device copy).
 * What a rank of a sharded job holds of a read set (contiguous read ranges); a job that checks the table of a
 * whole set against the union of its shards cuts the shards with it instead of scanning the reads again. */
int  mdbg_minimizers_slice(mdbg_ctx *ctx, const mdbg_minimizers *in, uint32_t first_read, uint32_t n_reads, mdbg_minimizers **out);

/* Replaces Utils::applyDensityThreshold over every read (Commons.hpp:2507-2550; callers ReadCorrection.hpp:6385, :6435,
 * Commons.hpp:2563 getLowDensityMinimizerRead, :7252-7742 the minimizer-read parsers): keeps the minimizers whose
 * selection hash is below `density` -- the down-sampling from the correction density to the assembly density.
 * Positions / directions / qualities / per-read fields follow when `in` carries them. */
int  mdbg_apply_density_threshold(mdbg_ctx *ctx, const mdbg_minimizers *in, float density, mdbg_minimizers **out);

/* Replaces Commons::purgePalindrome over every read (Commons.hpp:1617-1723, driven by
 * ReadSelection::purgePalindromes, ReadSelection.hpp:1374-1431). */
int  mdbg_purge_palindromes(mdbg_ctx *ctx, const mdbg_minimizers *in, uint32_t first_k, uint32_t last_k,
                            mdbg_minimizers **out);

/* Replaces CountMinimizerFunctor + the global map of determineRepetitiveMinimizers
 * (ReadSelection.hpp:497-625): counts every minimizer value of `m` on the device and returns the
 * top max(1, floor(1e-5 * distinct)) by count (ties broken by smaller value; the reference's
 * tie order is std::sort-unstable).  out must hold *n_out entries on input. */
int  mdbg_repetitive_minimizers(mdbg_ctx *ctx, const mdbg_minimizers *m, uint32_t *out, uint32_t *n_out);
/* The same census fed batch by batch -- the reads of determineRepetitiveMinimizers arrive in chunks (the first
 * 1 000 001 reads of every input file, ReadSelection.hpp:497-561): mdbg_census_add counts the values of one batch's
 * minimizers on the device (nothing travels; one count per possible value -- 4 bytes x the power of two above the largest
 * value seen: 4 GiB at l = 15, 16 GiB at l = 16 --, one add per minimizer), mdbg_census_top is the selection above over
 * everything added so far.
 * mdbg_repetitive_minimizers(m) = create, add(m), top, free. */
typedef struct mdbg_census mdbg_census;
int  mdbg_census_create(mdbg_ctx *ctx, mdbg_census **out);
int  mdbg_census_add(mdbg_ctx *ctx, mdbg_census *census, const mdbg_minimizers *m);
int  mdbg_census_top(mdbg_ctx *ctx, const mdbg_census *census, uint32_t *out, uint32_t *n_out);
void mdbg_census_free(mdbg_census *census);

/* ---- minimizers -> k-min-mer table ----------------------------------------------------- */
/* First pass, k = firstK: KminmerCounter::execute + rescueKminmers
 * (graph/CreateMdbg.hpp:3591-3883, :4514-4640; graph/CreateMdbg.cpp:290-328). */
int  mdbg_kminmer_count_first(mdbg_ctx *ctx, const mdbg_minimizers *reads, uint32_t k, uint32_t min_abundance,
                              mdbg_table **out);
/* Previous-iteration abundances for k > firstK (CreateMdbg::loadRefinedAbundances,
 * graph/CreateMdbg.cpp:3401-3709): from kminmerData_abundance_prev.txt records (lo,hi,abundance;
 * abundance==1 skipped) ... */
int  mdbg_prev_from_records(mdbg_ctx *ctx, const uint8_t *records20, uint64_t n_records, mdbg_table **out);
/* ... then overlaid with the refined abundance of each unitig of unitigGraph_prev.nodes.bin
 * (unitigs as CSR; abundance[u] per unitig, 0xFFFFFFFF = unitig has no refined abundance and is skipped). */
int  mdbg_prev_overlay_unitigs(mdbg_ctx *ctx, mdbg_table *prev, const mdbg_minimizers *unitigs,
                               const uint32_t *abundance, uint32_t k_prev);
/* k = firstK+1: KminmerCounter with getRefinedAbundance (graph/CreateMdbg.hpp:3933-4005) over
 * reads and (optionally, may be NULL) unitig_data.txt sequences. */
int  mdbg_kminmer_count_refined(mdbg_ctx *ctx, const mdbg_minimizers *reads, const mdbg_minimizers *unitigs,
                                uint32_t k, const mdbg_table *prev, mdbg_table **out);
/* k >= firstK+2: IndexKminmerFunctor (graph/CreateMdbg.hpp:1240-1265, :1450-1459) over reads and unitigs. */
int  mdbg_kminmer_index(mdbg_ctx *ctx, const mdbg_minimizers *reads, const mdbg_minimizers *unitigs,
                        uint32_t k, const mdbg_table *prev, mdbg_table **out);

/* Replaces the small-contig branch of IndexKminmerFunctor (graph/CreateMdbg.hpp:1330-1352), taken in the unitig pass of
 * `graph` when k > 8: a unitig with no k-min-mer whose getAbundance(0, prevAbundances) (:988-1010, prevAbundances over
 * its k_prev-min-mers, missing => 1, :1240-1265) exceeds 1 is appended to smallContigs/smallContigs_k<k>.bin
 * (`u32 n; u8 circular; u32 m[n]`) instead of being indexed.  flags (host, one per unitig) is set to 1 for those
 * unitigs; the caller applies the k > 8 condition and writes the records.  Unitigs shorter than k_prev, for which the
 * reference reads an empty vector (undefined), are never flagged. */
int  mdbg_small_contigs(mdbg_ctx *ctx, const mdbg_minimizers *unitigs, uint32_t k, uint32_t k_prev, const mdbg_table *prev,
                        uint8_t *flags);

/* n_records = rows of kminmerData_abundance.txt; n_solid of them are solid (the rest rescued,
 * abundance 1); has_vectors = whether kminmerData_min.txt rows exist (k <= firstK+1). */
int  mdbg_table_info(const mdbg_table *t, uint32_t *k, uint64_t *n_records, uint64_t *n_solid, int *has_vectors);
/* Host copies in file layout: records20 = n_records x {u64 lo, u64 hi, u32 abundance} packed
 * (MDBG::writeKminmerAbundance, Commons.hpp:4463-4472); vectors = n_records x k u32
 * (MDBG::writeKminmer, Commons.hpp:4429-4446), same row order.  Either may be NULL. */
int  mdbg_table_to_host(mdbg_ctx *ctx, const mdbg_table *t, uint8_t *records20, uint32_t *vectors);
/* Rows [first, first + count) only, same layout: a writer streams a large table (the ONT preset's first pass leaves 75 M records per
 * 20 Gbp, most of them rescued singletons) to its files through two page-locked buffers instead of holding it all on the host. */
int  mdbg_table_to_host_range(mdbg_ctx *ctx, const mdbg_table *t, uint64_t first, uint64_t count, uint8_t *records20, uint32_t *vectors);
/* What the pass that built the table walked: stats[0] = minimizers read (M), [1] = k-min-mer instances (I = sum over the
 * sequences of max(0, n - k + 1)), [2] = distinct keys it inserted, [3] = slots of the hash table it used.  With the table's
 * rows D these are the terms of the step's algorithmic bytes 4 M + 16 I + 20 D; zeros for tables that were
 * not built from sequences (mdbg_prev_from_records, the edge indexes, mdbg_shard_keep); a share of a sharded first pass reports
 * its rank's own reads and local keys. */
int  mdbg_table_stats(const mdbg_table *t, uint64_t stats[4]);
/* How the context's last mdbg_kminmer_count_first ran.  The reference counts the first pass's k-min-mers in `_nbPartitions`
 * partitions chosen by `vecHash % P`, each sorted and run-length counted (KminmerCounter, graph/CreateMdbg.hpp:3714-3851; P from
 * graph/CreateMdbg.cpp:222-225); the library either partitions the instances by bits of the identity and counts every bucket in LDS
 * (csrc/partition.hip) or meets them in one table in HBM (csrc/kminmer.hip; small inputs, k > 32).  info[0] = 2 / 1 for the two,
 * [1] = groups of keys processed one after the other (the analogue of _nbPartitions: more than one when the instance records of
 * all keys would not fit the memory budget), [2] = bucket bits per group, [3] = levels of the radix split, [4] = attempts (a
 * bucket that outgrows its LDS table makes the pass repeat with more buckets), [5] = LDS slots per bucket, [6] = buckets per
 * group, [7] = k-min-mer instances.  Options (mdbg_set_option): "first_pass_mode" 0 by size / 1 one table / 2 partitioned,
 * "partition_auto_min" (minimizers from which mode 0 partitions); for a context that shares its device with another context's
 * scan (a block only runs beside a scan if it fits what the scan's blocks leave of a CU) "partition_tile" 2048,
 * "partition_slot_list" 0 and "partition_lds_slots" 1024 select the kernels' 24 KB forms and "scan_lds_reserve" (bytes) makes
 * the scan leave that much of every CU's LDS free; for tests "partition_bits", "partition_lds_slots" (256 / 1024 / 2048),
 * "partition_max_records" (instances per group).  mdbg_shard_begin counts a rank's share the same way.
 * "partition_threads" (MDBG_PARTITION_THREADS sets the default of new contexts) chooses the threads per block of the radix split's
 * kernels: 0 (the default) or 512 = eight waves, tiles of 4096 records (2048 under "partition_tile" 2048); 256 = four waves, one per
 * SIMD, tiles of 1024 records, at most 72 vector registers and 15 KB of LDS -- within the 96 registers per lane that another context's
 * 16-wave scan workgroup leaves of a SIMD, which the eight-wave forms are not.  Beside that scan the four-wave forms measured SLOWER and
 * the scan no faster, so they are opt-in: for that comparison and for tests -- and what 0 means in a context with
 * "scan_lds_reserve" > 0 whose last block-kernel scan was a persistent launch ("scan_persistent"): those workgroups never retire to let an eight-wave block
 * in, and beside them the four-wave forms measured faster.  Results never depend on it.
 * mdbg_first_pass_form tells which form the context's last split kernels took: form[0] = threads per block, [1] = records per tile,
 * [2] = the wave priority the context's last purge, first-pass or prefix-scan kernel was launched with (below), [3] = 0.
 * "table_wave_priority" (MDBG_TABLE_WAVE_PRIORITY sets it for new contexts): the hardware issue priority, 0 .. 3 (other values are
 * clamped, as for "scan_wave_priority", which does the same for the scan's waves), that the waves of every kernel a step launches
 * outside the scan raise themselves to on entry: mdbg_purge_palindromes, the partitioned mdbg_kminmer_count_first / mdbg_shard_begin
 * and the prefix scans they use.  These kernels wait on memory; beside another context's scan, whose waves are bound by instruction
 * issue and are the oldest on their SIMD for a whole launch, they otherwise get the issue slots the scan leaves, and crawl
 * (DESIGN.md 4.4).  Where the option was never set a context takes 1 if it shares its device ("scan_lds_reserve" > 0) and 0 if not;
 * setting it, to 0 too, overrides that.  Results never depend on it.
 * mdbg_first_pass_slot_fall_backs: the instances of the last partitioned first pass whose LDS slot the bucket count looked up a second
 * time.  Counting a bucket walks its records twice (count, then a byte per instance of a rare key); the form without a slot list keeps
 * the slots of a bucket's first 8192 records in registers between the walks, the form with one those of its first 8000 (4096 beside 2048
 * slots) in LDS, and only the records behind them are found again by their key.  0 for mdbg_shard_begin (no second walk). */
int  mdbg_first_pass_info(const mdbg_ctx *ctx, uint64_t info[8]);
int  mdbg_first_pass_form(const mdbg_ctx *ctx, uint64_t form[4]);
int  mdbg_first_pass_slot_fall_backs(const mdbg_ctx *ctx, uint64_t *n);
/* The kernels of the headline step (scan, purge, first pass) by name, and what the runtime knows of each in the loaded code object
 * (hipFuncGetAttributes): what a kernel of one context needs of a compute unit -- registers, wave slots, LDS -- against what another
 * context's scan workgroup leaves of it.  mdbg_step_kernel_name(i) = the i-th name, NULL past the last.  attr[0] = vector registers per lane, [1] = bytes
 * of static LDS per block, [2] = the most threads a block may have, [3] = threads per block as the library launches it, [4] = 0 for the
 * 16-wave scan itself / 1 for a kernel that a context sharing its device launches / 2 for a form such a context does not take by itself, [5] = bytes of scratch per thread, [6], [7] = 0.  MDBG_EINVAL for an unknown name. */
const char *mdbg_step_kernel_name(uint32_t index);
int  mdbg_kernel_attributes(mdbg_ctx *ctx, const char *kernel, uint64_t attr[8]);
/* Which block-structured scan kernels the context has launched (mdbg_scan; "scan_prefilter" above): info[0] = launches of the pre-filtered
 * variant, [1] = launches of the four-wave block kernels, [2] = selected-key bitmaps built, [3] = bits set in the last one, [4] = log2 of
 * its size in bits, [5] = waves per workgroup of the last pre-filtered launch (16, or 8 under a large "scan_lds_reserve"), [6] = 1 when
 * the last block-kernel launch was the pre-filtered variant, [7] = reads the context's last mdbg_scan scanned as segments ("scan_segments";
 * reads that fell back whole are not counted).  No reference analogue: the reference hashes every position. */
int  mdbg_scan_info(const mdbg_ctx *ctx, uint64_t info[8]);
/* The selected-key table of the pre-filtered variant's confirmation ("scan_confirm_table" above): info[0] = tables built, [1] = buckets of
 * the last one, [2] = buckets of it that ask the hash (more than seven keys; or, in a test geometry below 2^16 buckets, a tag shared with a
 * key that is not selected), [3] = 1 when the last pre-filtered launch took its verdicts from the table, 0 when it hashed its candidates. */
int  mdbg_scan_confirm_info(const mdbg_ctx *ctx, uint64_t info[4]);
/* The form of the context's last pre-filtered launch ("scan_persistent" above): info[0] = 1 persistent / 0 chunked, [1] = its workgroups,
 * [2] = reads a wave drew at a time (0 when chunked), [3] = persistent launches of the context so far. */
int  mdbg_scan_persistent_info(const mdbg_ctx *ctx, uint64_t info[4]);
/* Order-independent sums over the rows, wrapping at 2^64, computed on the device (nothing but 32 bytes travels):
 *   sums[0] = sum abundance * hash_lo -- the "Checksum kminmer abundance" the reference logs when it loads the table again
 *             (CreateMdbg::loadRefinedAbundances, graph/CreateMdbg.cpp:3300-3321, :3397: `abundance * vecHash` truncated to u64),
 *   sums[1] = sum abundance, sums[2] = sum hash_hi,
 *   sums[3] = sum (v[0] + 3 v[1] + 5 v[2] + ...) * (hash_lo | 1) over the rows' vectors (0 when the table has none).
 * The sums of the per-rank tables of a sharded pass add up to those of the single-GPU table (the union of the shares is the
 * table): what a multi-GPU job checks itself with. */
int  mdbg_table_checksum(mdbg_ctx *ctx, const mdbg_table *t, uint64_t sums[4]);
/* In-process lookup for the reference's graph multiplexer (isEdgeSupported etc.,
 * graph/CreateMdbg.cpp:3990): abundance of each of n keys, 0 when absent. */
int  mdbg_table_lookup(mdbg_ctx *ctx, const mdbg_table *t, const uint64_t *hash_lo, const uint64_t *hash_hi,
                       uint64_t n, uint32_t *abundance);
/* SURVEY.md 8(f) N2 -- EdgeIndexer (graph/CreateMdbg.hpp:4010-4230, driven by indexEdges, graph/CreateMdbg.cpp:1178-1186):
 * the distinct identities of the normalised (k-1)-prefix and (k-1)-suffix of every k-min-mer vector of `nodes`
 * (a table with vectors, i.e. the rows of kminmerData_min.txt) = the content of edges.bin.  The result is a table
 * without vectors whose abundance column is 0; *checksum = sum of the identities truncated to u64 as the reference
 * logs it.  Fetch the 16-byte records with mdbg_table_keys_to_host (u128 little-endian: lo, hi). */
int  mdbg_edge_index(mdbg_ctx *ctx, const mdbg_table *nodes, mdbg_table **edges, uint64_t *checksum);
int  mdbg_table_keys_to_host(mdbg_ctx *ctx, const mdbg_table *t, uint64_t *keys_lo_hi);
/* Replaces UnitigEdgeIndexer::partitionEdges + dereplicatePartitions (graph/CreateMdbg.hpp:4234-4512): the distinct
 * (k-1)-prefix/suffix identities of the FIRST and LAST k-min-mer of every unitig of unitigGraph.nodes.bin (uploaded as
 * minimizer-space sequences; sequences shorter than k contribute nothing).  *checksum as in mdbg_edge_index (may be NULL). */
int  mdbg_unitig_edge_index(mdbg_ctx *ctx, const mdbg_minimizers *unitigs, uint32_t k, mdbg_table **edges, uint64_t *checksum);
void mdbg_table_free(mdbg_table *t);

/* ---- k-min-mer spans in base space ---------------------------------------------------------------------------------------------------
 * Replaces, for a whole batch, what the callers that scan raw reads or contigs again do with a scan -- ToBasespaceGfa::
 * ExtractKminmerSequenceFunctor (toBasespace/ToBasespaceGfa.hpp:1177-1237), MappingContigToGraph (mapping/MappingContigToGraph.hpp:187-217,
 * :308), GenerateGfa::LoadUnitigsFunctor: MDBG::getKminmers(l, k, minimizers, minimizersPos, kminmers, kminmersInfo, rlePositions, ...)
 * (Commons.hpp:5401-5526) over the rlePositions of EncoderRLE::execute (Commons.hpp:4163-4203).  The reads and their scan go in; per
 * window of k minimizers the identity and the ReadKminmer fields come out, on the device.
 *
 * rle[j] is the original coordinate of compressed position j: L' + 1 entries, rle[L'] = the read's length; without homopolymer
 * compression rle[j] = j.  A minimizer selected at compressed position p spans [S, E) = [rle[p], rle[p + l]) of the original read.
 * Window i of a read with n minimizers (0 <= i <= n - k; none when n < k), in read order:
 *     reversed           the flag of KmerVec::normalize (a tie reverses; Commons.hpp:886-916)
 *     hash_lo, hash_hi   the identity of the normalised window, as the records of mdbg_table_to_host carry it (mdbg_table_lookup takes it)
 *     pos_start          S of its first minimizer          (ReadKminmer::_read_pos_start)
 *     pos_end            E of its last minimizer           (_read_pos_end; _length is pos_end - pos_start)
 *     seq_length_start   with f = S(second) - S(first) and b = E(last) - E(last but one): f, or b when reversed   (_seq_length_start)
 *     seq_length_end     b, or f when reversed                                                                     (_seq_length_end)
 * The four _position_of_* fields are always 0 in the reference and get no array.  One case differs from the reference on purpose:
 * without compression, with no_end_trim and the read's last l-mer selected, the reference reads one element behind rlePositions; the
 * library returns the natural p + l.
 *
 * mdbg_kminmer_spans   `mins` must carry positions and per-read lengths -- an mdbg_scan output, or an mdbg_minimizers_concat /
 *                      mdbg_apply_density_threshold result that kept them -- and describe `reads`: as many
 *                      reads, every read's recorded length the read's own, the positions of a read strictly increasing with
 *                      p + minimizer_size <= L' (minimizer_size and hpc as they were given to the scan).  Anything else is MDBG_EINVAL with
 *                      a message that names the first offending read; *out is untouched and no byte outside the inputs has been read:
 *                      the checks run on the device before anything is looked up.  k >= 2 (a window's second minimizer is read); like
 *                      mdbg_kminmer_index the call sets no upper limit: a k above every read's count gives zero windows.  A fresh scan
 *                      output is brought into read order first, as by mdbg_minimizers_to_host.  Zero reads or zero windows give empty
 *                      arrays.  The kernels are queued on the context's stream behind an asynchronous upload of `reads`; one status word
 *                      is read back, and the call returns when the result is complete.  Timer names: "spans_map", "spans_windows".
 * mdbg_spans_to_host   host copies, any pointer may be NULL: window_offsets has n_reads + 1 entries (the windows in front of each read),
 *                      min_start / min_end (S and E of every minimizer) n_minimizers, the rest n_windows.
 * mdbg_spans_device_ptrs  the same arrays on the device, for a caller that cuts the bases out there. */
typedef struct mdbg_spans mdbg_spans;
int  mdbg_kminmer_spans(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_minimizers *mins,
                        uint32_t minimizer_size, int32_t hpc, uint32_t k, mdbg_spans **out);
int  mdbg_spans_info(const mdbg_spans *s, uint32_t *n_reads, uint64_t *n_minimizers, uint64_t *n_windows, uint32_t *k);
int  mdbg_spans_to_host(mdbg_ctx *ctx, const mdbg_spans *s, uint64_t *window_offsets,
                        uint32_t *min_start, uint32_t *min_end,
                        uint64_t *hash_lo, uint64_t *hash_hi, uint8_t *reversed,
                        uint32_t *pos_start, uint32_t *pos_end, uint32_t *seq_length_start, uint32_t *seq_length_end);
int  mdbg_spans_device_ptrs(const mdbg_spans *s, const uint64_t **d_window_offsets, const uint64_t **d_hash_lo, const uint64_t **d_hash_hi,
                            const uint32_t **d_pos_start, const uint32_t **d_pos_end);
void mdbg_spans_free(mdbg_spans *s);

/* ---- k-min-mer sequences cut out of the reads ------------------------------------------------------------------------------------------
 * Replaces, for a whole batch, what the callers of the spans do with them: ToBasespaceGfa::extractKminmerSequence (toBasespace/
 * ToBasespaceGfa.hpp:1050-1103) -- a memcpy of the window, Utils::revcomp (Commons.hpp:3007-3014) of a reversed window, a substr for the
 * left or right overhang -- as the loop body of ExtractKminmerSequenceFunctor calls it (:1177-1237), and the DnaBitset2 the result is kept
 * as (utils/DnaBitset.hpp:118-242); with whole reads, LoadUnitigsFunctor's DnaBitset2(read._seq) (graph/GenerateGfa.hpp:418).  The reads
 * stay in HBM at 2 bits a base; nothing is exported as characters and cut on the host.
 *
 * A request names a window by its flat index (window_offsets[read] + i of mdbg_spans_to_host) and a part (LoadType Entire / Left / Right).
 * With the window's fields ps = pos_start, pe = pos_end, ls = seq_length_start, le = seq_length_end (the spans already exchange ls and le
 * for a reversed window) the range of the read that is taken is
 *     part               forward             reversed (the output is the reverse complement of the range)
 *     MDBG_SEQ_ENTIRE    [ps, pe)            [ps, pe)
 *     MDBG_SEQ_LEFT      [ps, ps + ls)       [pe - ls, pe)
 *     MDBG_SEQ_RIGHT     [pe - le, pe)       [ps, ps + le)
 * which is the first ls / last le characters of the oriented string, as the reference's substr takes them.  mdbg_reads_extract_ranges
 * takes the ranges from the caller instead (reversed: 0 = as it stands, anything else = reverse complement); the whole read [0, length)
 * forward is LoadUnitigsFunctor's case.  Requests may repeat, come in any order and number zero; the output keeps their order.
 *
 * Forms.  MDBG_SEQ_BITSET is DnaBitset2::_m_data: base i of a sequence in byte i / 4 at bits 6 - 2 (i % 4), codes A 0, C 1, G 2, T 3,
 * ceil(length / 4) bytes meaningful, unused bits 0.  MDBG_SEQ_ASCII is the string before it is packed: upper-case ACGT, and N where the
 * read's invalid mask is set.  In both forms sequence i starts at byte_offsets[i], a multiple of 8, and everything between its last
 * meaningful byte and byte_offsets[i + 1] is 0.  A position whose character had bit 3 set (N, n, K, M, Y ...) is code 0 in the bitset
 * in both orientations: what DnaBitset2 stores for any character outside ACGT.  One case differs from the reference on purpose: a
 * lower-case acgt, or an IUPAC letter without bit 3 (R, S, W), comes out as the base its 2-bit code names, where DnaBitset2 stores A --
 * the packed reads no longer know the case.
 *
 * Refusals, MDBG_EINVAL with a message that names the first offending request, *out untouched: a part or form out of range, reserved != 0,
 * window >= n_windows, a read index >= n_reads, spans that do not describe `reads` (another number of reads, or another length of a read
 * a request touches), a range whose start + length lies behind its read's end, ls or le larger than pe - ps.  The checks run on the
 * device before any base is read; one status word is read back, and the call returns when the result is complete.  2^32 requests or more
 * are MDBG_ERANGE.  Timer names: "extract_plan", "extract_copy".
 * mdbg_sequences_info         n sequences, their bases in all, the bytes of the buffer (padding included), the form.
 * mdbg_sequences_to_host      host copies, any pointer may be NULL: byte_offsets n + 1 entries, lengths (bases) n, bytes n_bytes.
 * mdbg_sequences_device_ptrs  the same arrays on the device. */
typedef struct { uint64_t window; uint32_t part; uint32_t reserved; } mdbg_seq_request;
typedef struct { uint32_t read, start, length, reversed; } mdbg_seq_range;
enum { MDBG_SEQ_ENTIRE = 0, MDBG_SEQ_LEFT = 1, MDBG_SEQ_RIGHT = 2 };
enum { MDBG_SEQ_BITSET = 0, MDBG_SEQ_ASCII = 1 };
typedef struct mdbg_sequences mdbg_sequences;
int  mdbg_spans_extract(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_spans *spans, const mdbg_seq_request *requests, uint64_t n,
                        int form, mdbg_sequences **out);
int  mdbg_reads_extract_ranges(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_seq_range *ranges, uint64_t n, int form,
                               mdbg_sequences **out);
int  mdbg_sequences_info(const mdbg_sequences *s, uint64_t *n, uint64_t *n_bases, uint64_t *n_bytes, int *form);
int  mdbg_sequences_to_host(mdbg_ctx *ctx, const mdbg_sequences *s, uint64_t *byte_offsets, uint32_t *lengths, uint8_t *bytes);
int  mdbg_sequences_device_ptrs(const mdbg_sequences *s, const uint64_t **d_byte_offsets, const uint32_t **d_lengths, const uint8_t **d_bytes);
void mdbg_sequences_free(mdbg_sequences *s);

/* ---- files of records handed over as BYTES (round 6) ---------------------------------------------------------------------------
 * What `graph` reads at every k -- read_data_corrected.txt and unitig_data.txt (`u32 n; u8 circular; u32 m[n]` per record,
 * readSelection/ReadSelection.hpp:1420-1426, read back by KminmerParserParallel under one critical section, Commons.hpp:7394-7424)
 * and kminmerData_abundance_prev.txt (20-byte records, loaded by CreateMdbg::loadRefinedAbundances, graph/CreateMdbg.cpp:3401-3491) --
 * need not be parsed into arrays on the host first: the file's bytes travel as they are, in pieces, from page-locked slabs
 * (mdbg_host_alloc) beside whatever else the process does, and the records are taken apart on the device.  One `graph` process per k
 * is how the reference runs the loop (pipeline/AssemblyPipeline.hpp:763-792): 97 of them in a default assembly of 10 kb reads.
 *
 * mdbg_bytes_create       a device buffer of n_bytes.
 * mdbg_bytes_upload_async `n` bytes from `host` to offset `at`, queued on the context's upload stream; returns at once when `host` is
 *                         page-locked.  *ticket (optional) names the copy: `host` may be reused once mdbg_bytes_upload_done(ticket) says so.
 * mdbg_bytes_upload_done  1 = the copy named by `ticket` (and every earlier one) is complete, 0 = not yet (wait != 0: block until it is).
 * mdbg_minimizers_from_record_bytes
 *                         the minimizer-space read set of a record file whose bytes are in `records`: `offsets` (host, n_reads + 1) are
 *                         the minimizers before each read, as the caller's walk over the record headers found them -- record r then
 *                         starts at byte 5 r + 4 offsets[r].  Every record's own count is checked against the offsets on the device
 *                         (MDBG_EINVAL on a mismatch: the bytes are not that file).  circular (optional, host, n_reads) receives the
 *                         records' flag bytes.  Uploads still in flight are waited for on the device, not by the host.
 * mdbg_prev_from_record_bytes
 *                         mdbg_prev_from_records for a table file whose bytes are in `records`. */
typedef struct mdbg_bytes mdbg_bytes;
int  mdbg_bytes_create(mdbg_ctx *ctx, uint64_t n_bytes, mdbg_bytes **out);
int  mdbg_bytes_upload_async(mdbg_ctx *ctx, mdbg_bytes *b, uint64_t at, const void *host, uint64_t n, uint64_t *ticket);
int  mdbg_bytes_upload_done(mdbg_ctx *ctx, mdbg_bytes *b, uint64_t ticket, int wait);
void mdbg_bytes_free(mdbg_bytes *b);
int  mdbg_minimizers_from_record_bytes(mdbg_ctx *ctx, const mdbg_bytes *records, const uint64_t *offsets, uint32_t n_reads,
                                       uint8_t *circular, mdbg_minimizers **out);
int  mdbg_prev_from_record_bytes(mdbg_ctx *ctx, const mdbg_bytes *records, uint64_t n_records, mdbg_table **out);

/* ---- record files SERIALISED on the device ---------------------------------------------------------------------------------------
 * The inverse of mdbg_minimizers_from_record_bytes: a minimizer set goes in, the exact bytes of its record file come out in an
 * mdbg_bytes on the device, ready for mdbg_bytes_download and a plain write().  Replaces the field-by-field write loops of
 * ReadSelection (readSelection/ReadSelection.hpp:415-467 for read_data_init.txt, :1420-1426 for read_data_corrected.txt) and the
 * caller's own serialiser.  Little-endian, no padding; with o = offsets[r] and n = offsets[r + 1] - o, in 64-bit arithmetic:
 *
 *   MDBG_RECORDS_PLAIN  `u32 n; u8 circular; u32 m[n]` (read_data_corrected.txt, unitig_data.txt).  Record r starts at byte
 *                       5 r + 4 o: count at +0, circular (always 0) at +4, values at +5.  5 n_reads + 4 n_minimizers bytes in all.
 *   MDBG_RECORDS_INIT   `u32 n; u8 circular; u32 m[n]; u32 pos[n]; u8 dir[n]; u8 qual[n]; f32 meanQ; u32 len` (read_data_init.txt).
 *                       Record r starts at byte 13 r + 10 o: count +0, circular (0) +4, m +5, pos +5 + 4 n, dir +5 + 8 n,
 *                       qual +5 + 9 n, meanQ +5 + 10 n, len +9 + 10 n.  13 n_reads + 10 n_minimizers bytes in all.  Only an mdbg_scan
 *                       output (or mdbg_minimizers_concat / mdbg_apply_density_threshold of such) has these fields: MDBG_EINVAL otherwise.  The mean
 *                       quality comes out with the bits mdbg_minimizers_to_host hands back, NaN included.
 *
 * *out is a new buffer of exactly that many bytes (release with mdbg_bytes_free); *n_bytes (optional) is its size.  Zero reads give a
 * buffer of 0 bytes.  An unknown `form` or a null argument is MDBG_EINVAL.  A fresh scan output is brought into read order first, as
 * by mdbg_minimizers_to_host.  The kernel is queued on the context's stream and the call does NOT wait for it: what the same context
 * is asked next -- mdbg_bytes_download, mdbg_minimizers_from_record_bytes, mdbg_reads_from_fastx_bytes -- is ordered behind it by the
 * stream.  Another context, or anything else that reads the buffer, calls mdbg_synchronize(ctx) first.
 * Timer name: "records_write". */
#define MDBG_RECORDS_PLAIN 0   /* read_data_corrected.txt, unitig_data.txt */
#define MDBG_RECORDS_INIT  1   /* read_data_init.txt: mdbg_scan output only */
int  mdbg_minimizers_to_record_bytes(mdbg_ctx *ctx, const mdbg_minimizers *m, int form, mdbg_bytes **out, uint64_t *n_bytes /* optional */);

/* ---- contig sequences stitched from pieces, and their FASTA text ---------------------------------------------------------------------------
 * Replaces the last step of the same caller: ToBasespaceGfa::createBaseContigs / CreateBaseContigsFunctor::operator() (toBasespace/
 * ToBasespaceGfa.hpp:1437-1795), which walks a contig's windows, looks up the stored piece of each (_readPosition_entire / _right /
 * _left, :1547-1702), to_string()s it, runs Utils::revcomp over it when the contig's window is reversed, appends, and writes
 * ">ctg<index><l|c>\n<sequence>\n" through gzwrite (:1756-1785).  The pieces of mdbg_spans_extract start at multiples of 8 bytes and
 * cannot be joined by copying; here the contig is gathered from the resident reads directly, at 2 bits a base.
 *
 * Sequence c of the result is the concatenation, in order, of the oriented pieces piece_offsets[c] .. piece_offsets[c + 1] (piece_offsets:
 * host, n_contigs + 1 entries, starts at 0, never decreases; its last entry is the number of pieces).
 *   mdbg_spans_stitch         a piece is (window, part, flip): the range extract_part_range gives for (window, part) exactly as
 *                             mdbg_spans_extract takes it, oriented by the READ's window; flip != 0 reverse-complements that oriented
 *                             piece once more -- the CONTIG window's own _isReversed -- so the net orientation of the range is
 *                             reversed ^ flip.  window == MDBG_STITCH_NONE is "no sequence for this k-min-mer": it contributes nothing
 *                             (the reference's `continue`) and its other fields are not looked at.
 *   mdbg_reads_stitch_ranges  the pieces are mdbg_seq_range as they stand; length 0 is allowed and contributes nothing.
 * The piece rule CreateBaseContigsFunctor uses: window 0 of a contig takes MDBG_SEQ_ENTIRE (flip when the contig's window is reversed);
 * every later window takes MDBG_SEQ_RIGHT with flip 0 when the contig's window is forward and MDBG_SEQ_LEFT with flip 1 when it is
 * reversed.  A window without a stored sequence is skipped but still counts as a position: the window behind a skipped window 0 is not
 * ENTIRE.
 *
 * The result is an ordinary mdbg_sequences (mdbg_sequences_info / _to_host / _device_ptrs / _free): forms MDBG_SEQ_BITSET and
 * MDBG_SEQ_ASCII, every contig at a multiple of 8 bytes, padding zero, lengths = the contig's bases.  Zero contigs, contigs without pieces
 * and contigs of empty pieces give empty sequences (length 0, no bytes).
 *
 * Invalid bases -- the one rule that differs from mdbg_spans_extract.  The reference stores the READ-oriented piece as DnaBitset2, where
 * a character outside ACGT is A, and calls Utils::revcomp on the string of a reversed contig window afterwards.  So in BITSET form a base
 * under the invalid mask is code 0 (A) when flip == 0 and code 3 (T) when flip != 0, whatever the read window's orientation.  In
 * mdbg_reads_stitch_ranges it is code 0 always, as in mdbg_reads_extract_ranges.  In ASCII form it is N in both entries.
 *
 * Refusals, MDBG_EINVAL with a message that names the first offending piece and its contig, *out untouched, no base read before the
 * checks have run on the device: every refusal of mdbg_spans_extract / mdbg_reads_extract_ranges, per piece (there is no reserved field);
 * piece_offsets that do not start at 0 or decrease (checked on the host); a form out of range.  MDBG_ERANGE: 2^32 pieces or more, 2^32
 * contigs or more, a contig of 2^32 bases or more.  Timer names: "stitch_plan", "stitch_copy".
 *
 * mdbg_sequences_to_fasta_bytes  the exact bytes CreateBaseContigsFunctor hands to gzwrite, uncompressed, in an mdbg_bytes of exactly
 *                             that size (mdbg_bytes_download, mdbg_bytes_free).  seqs must be in MDBG_SEQ_BITSET form.  names (host, n;
 *                             NULL: 0, 1, 2 ...) are the contigs' indices, circular (host, n; NULL: all 0) their flags.  A non-empty
 *                             sequence i gives ">ctg", the decimal digits of names[i], "l" for flag 0 and "c" for flags 1 and 2, '\n',
 *                             its bases as ACGT decoded from the 2-bit codes (DnaBitset2::to_string: no N, no line wrap), '\n'.  (The
 *                             functor has an "rc" for flag 2, CONTIG_CIRCULAR_RESCUED, but narrows the flag to `bool isCircular`
 *                             first, :1487, so that branch is never reached and a rescued contig is written "c": so is it here.)  An empty
 *                             sequence gives ">ctg<name>l\nA\n" whatever its flag (:1756-1764).  Zero sequences give a buffer of 0 bytes.
 *                             MDBG_EINVAL: ASCII-form input, a flag above 2, a null argument.  The call returns when the text is
 *                             complete.  Timer names: "fasta_plan", "fasta_write". */
typedef struct { uint64_t window; uint32_t part; uint32_t flip; } mdbg_stitch_piece;
#define MDBG_STITCH_NONE UINT64_MAX
int  mdbg_spans_stitch(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_spans *spans, const mdbg_stitch_piece *pieces,
                       const uint64_t *piece_offsets, uint64_t n_contigs, int form, mdbg_sequences **out);
int  mdbg_reads_stitch_ranges(mdbg_ctx *ctx, const mdbg_reads *reads, const mdbg_seq_range *ranges, const uint64_t *piece_offsets,
                              uint64_t n_contigs, int form, mdbg_sequences **out);
int  mdbg_sequences_to_fasta_bytes(mdbg_ctx *ctx, const mdbg_sequences *seqs, const uint32_t *names /* optional */,
                                   const uint8_t *circular /* optional */, mdbg_bytes **out, uint64_t *n_bytes /* optional */);

/* ---- reads mapped against reads in minimizer space: index, anchors, chains --------------------------------------------------------------
 * Replaces the data-parallel part of ReadMapper (readSelection/ReadMapper.hpp), which ReadCorrection runs over read_data_init.txt
 * (ReadCorrection.hpp:2159), at k = 2 as ReadMapper::execute sets it (:172).  It reads minimizers and their positions only -- what a scan
 * output already keeps on the device -- and no base.
 *
 * Window i of a read of n minimizers (n - 1 windows), a = m[i], b = m[i + 1]: reversed = (a >= b) (KmerVec::normalize, Commons.hpp:886-916),
 * pair = (min(a, b) << 32) | max(a, b) (packPair, :937), position = (pos[i] + pos[i + 1]) / 2, index = i.  A read's global number is the
 * call's first_read + its number in the set.
 *
 * mdbg_minimizers_attach_positions  gives a set made by mdbg_minimizers_from_host the position array a scan output has (host, one per
 *       minimizer).  MDBG_EINVAL with the first offending read: a position that is not strictly above the one before it inside its read,
 *       or one >= 2^31 (the reference takes position differences in int32_t, ReadMapper.hpp:1159-1166).  Sets that carry positions: a scan
 *       output, a concat or apply_density_threshold of scan outputs, a set with attached positions; every other set is MDBG_EINVAL below.
 *
 * mdbg_map_index_build  replaces ReadFunctor (:465-505), Commons::sortParallel and createLookupTable (:550-627): every window of every read
 *       of the chunk, reads below 10 minimizers included, grouped by pair; a pair's entries are in (read, index) order.  info: entries,
 *       distinct pairs, the longest run of one pair, reads.  _to_host gives the entries in index order (any array may be NULL).
 *       MDBG_ERANGE: 2^32 entries or more.  Timer names: "map_index", "radix_sort".
 *
 * mdbg_map_anchors  replaces the join and the per-read std::sort of AlignReadsLowDensityFunctor::operator() (:668-756) for the reads
 *       [query_begin, query_end) of `queries` (0, 0: all).  A query below 10 minimizers produces nothing (Utils::isReadTooShort,
 *       Commons.hpp:2190); every other window produces one anchor per index entry of its pair whose global read number differs from the
 *       query's own: (ref_read, ref_position, ref_index, query_position, query_index, reversed = ref.reversed != query.reversed).  The
 *       anchors of a query are in (ref_read, ref_position, query_position) order, the queries in read order; the anchors of one (query,
 *       ref_read) are a PAIR, and pairs of fewer than min_anchors anchors are dropped (processAnchors, :850: 3; 0 and 1 keep everything).
 *       Result: pair_offsets[n_queries + 1]; per pair ref_read and anchor_offsets[n_pairs + 1]; the six arrays per anchor.
 *       info: queries, pairs, anchors, the longest pair.  device_ptrs, in order: pair_offsets (u64), pair_ref_read (u32), anchor_offsets
 *       (u64), ref_read, ref_position, ref_index, query_position, query_index (u32), reversed (u8).
 *       MDBG_ERANGE: the call would produce 2^32 anchors or more -- known after the count pass, before anything is allocated for them; the
 *       message says how many query reads from query_begin fit.  MDBG_EINVAL: a query range outside the set.
 *       Timer names: "map_count", "map_fill", "map_group", "radix_sort".
 *
 * mdbg_map_chains  replaces chainAnchors + argmaxPosition (:887-1230): one row per pair, in the pairs' order.  Scores are integers: the
 *       reference's floats are sums of 20 - gap with an integer gap <= 100, exact while a pair has fewer than 2^24 / 80 = 209 715
 *       anchors; a longer pair gets flags = MDBG_CHAIN_TOO_LONG and zero fields, never an approximate chain.  For anchor i ascending,
 *       score[i] = 20 without parent unless a predecessor j = i - 1 ... max(0, i - max_chaining_band) qualifies: skipped when the
 *       reversed flags differ, ref_position or query_position are equal, d_q (q_i - q_j; q_j - q_i when reversed) > 5000, d_r > 5000,
 *       d_r <= 0, |d_r - d_q| > 100, d_q < 0; new = score[j] + 20 - |d_r - d_q|, the best strictly positive new wins, on a tie the LARGEST
 *       j.  The best anchor has the largest score, on a tie the SMALLEST i.  Its chain (the parents walked to the root) of fewer than 3
 *       anchors is no chain (flags 0, zero fields).  Otherwise flags = MDBG_CHAIN_FOUND and the fields are Chain2's as :1017-1047 leaves
 *       them, `first` the best anchor and `last` the root: score, n_matches, query_reversed = first.query_index > last.query_index (true for
 *       a same-strand match), n_diff_query, n_diff_reference, query_start / query_end (indexes), reference_start = first.ref_position,
 *       reference_end = last.ref_position, alignment_score = n_matches - n_diff_query (:1241), and the pair's match list
 *       _queryAnchorPositions: the query indexes from the best anchor to the root, turned round when query_reversed.
 *       Result: pair_offsets[n_queries + 1] (the anchors' own), chains[n_pairs], match_offsets[n_pairs + 1], matches.
 *       info: queries, pairs, chains found, matches in all.  device_ptrs, in order: pair_offsets, chains, match_offsets, matches.
 *       MDBG_EINVAL: max_chaining_band 0.  Timer names: "map_chains", "map_matches".
 *
 * ---- the per-position selection, its merge across chunks, the alignment file --------------------------------------------------------------
 * The rule (addAlignmentScore, :1233-1313, with AlignmentScoreComparator, :90-97): every query index of a pair's match list owns a heap of
 * `coverage` entries (_usedCoverageForCorrection, ReadCorrection.hpp:1728: 20) whose top is the lowest score and, among equal scores, the
 * largest read; a pair replaces the top unless its score is lower, or equal with a larger read.  Pairs arrive in ascending ref_read, so the
 * heap a position ends with is the first `coverage` of the pairs covering it under (score descending, ref_read ascending), and a pair is
 * SELECTED iff it is among them at one position of its list at least (:809-820).  The score is n_matches - n_diff_query (:1241) =
 * 2 n - (last - first + 1) of the match list (mergeAlignmentScore, :376-382); it may be zero or negative, nothing filters it (:1243).
 *
 * mdbg_map_select  replaces the heaps of AlignReadsLowDensityFunctor::operator() (:772-841), processAnchors (:848-884) and
 *       addAlignmentScore (:1233-1313) for one chunk: the pairs of `chains` with flags == MDBG_CHAIN_FOUND take part.  coverage: 1 ... 255,
 *       anything else is MDBG_EINVAL.  Result per query: sel_offsets[n_queries + 1] and the selected rows in ascending ref_read (:836) --
 *       ref_read, score, n_matches, part = 0, pair = the pair's index in `chains` -- and, gathered behind the rows, their match lists
 *       (match_offsets[n_selected + 1], matches): the object needs no other.  n_matches is the list's full length: the reference's
 *       partition record cuts it to 16 bits (:1279), which is a limit of that record, the caller's, not of the selection.
 *       Timer names: "map_select", "radix_sort".
 * mdbg_selection_from_host  a selection made of stored parts: per query the reads (strictly ascending) and per read its match list (not
 *       empty, strictly ascending).  No score is passed: the library computes 2 n - (last - first + 1), as mergeAlignmentScore (:365-443)
 *       does.  part = 0, pair = the row's own number.  MDBG_EINVAL with the first offending query: reads or a list that do not ascend
 *       strictly, an empty list, offsets that do not ascend.
 * mdbg_map_select_merge  replaces mergeAlignmentPartition (:228-363) + mergeAlignmentScore (:365-443): per query the rows of the parts
 *       -- in chunk order, all of one n_queries -- one behind the other, selected again by the same rule.  The rows' reads must ascend
 *       strictly across the parts (checked on the device; MDBG_EINVAL names the first offending query).  part = the part's number in this
 *       call, pair is carried through.  n_parts == 1 re-selects one part at another coverage.  Selecting per chunk and merging gives what
 *       one selection over all chunks' chains gives.  Timer names: "map_select", "radix_sort".
 * mdbg_selection_to_alignment_bytes  the bytes writeAlignments (:1391-1410) writes for the selection, on the device: for every query with at
 *       least one selected row u32 read = query_first_read + its number, u32 n, u32 ref_read[n], in read order; *n_bytes (optional) is
 *       their size.  Fetch with mdbg_bytes_download, release with mdbg_bytes_free.  Timer name: "select_alignment_write".
 * mdbg_selection_info  queries, selected rows, matches, candidates that took part.  _to_host: any array may be NULL.  device_ptrs, in order:
 *       sel_offsets (u64), rows (mdbg_selected), match_offsets (u64), matches (u32).  Empty inputs give empty results.
 * mdbg_select_lds_positions  positions of a query up to which the selection's counters live in LDS; a longer query counts in global memory.
 *
 * What stays with the caller: the compression of the match lists (TurboPFor, compressMatches :1315-1320) and the BGZF partition files --
 * the reference's way of carrying a chunk's result to its merge, which an mdbg_selection (or its arrays, stored and given back through
 * mdbg_selection_from_host) replaces -- and, behind mdbg_map_verify below, performPoaCorrection4 of ReadCorrection with its low-density
 * re-chaining and the graph it builds. */
typedef struct mdbg_map_index mdbg_map_index;
typedef struct mdbg_anchors mdbg_anchors;
typedef struct mdbg_chains mdbg_chains;
typedef struct { uint32_t max_chaining_band;   /* ReadCorrection.hpp:1738: (u64)(2500 * density_correction), 62 at 0.025 */
                 uint32_t min_anchors;         /* ReadMapper.hpp:850: 3 */
                 uint32_t query_begin, query_end; /* reads [begin, end) of the query set; 0, 0 = all */
                 uint32_t reserved[4]; } mdbg_map_params;
#define MDBG_CHAIN_FOUND    1u
#define MDBG_CHAIN_TOO_LONG 2u
typedef struct { uint32_t ref_read, flags; int32_t score; uint32_t n_matches, query_reversed, reserved;
                 int64_t n_diff_query, n_diff_reference, query_start, query_end, reference_start, reference_end, alignment_score; } mdbg_chain;
int  mdbg_minimizers_attach_positions(mdbg_ctx *ctx, mdbg_minimizers *m, const uint32_t *positions);
int  mdbg_map_index_build(mdbg_ctx *ctx, const mdbg_minimizers *chunk, uint32_t chunk_first_read, mdbg_map_index **out);
int  mdbg_map_index_info(const mdbg_map_index *ix, uint64_t info[4]);
int  mdbg_map_index_to_host(mdbg_ctx *ctx, const mdbg_map_index *ix, uint64_t *pairs, uint32_t *reads, uint32_t *positions, uint32_t *indexes,
                            uint8_t *reversed);
void mdbg_map_index_free(mdbg_map_index *ix);
int  mdbg_map_anchors(mdbg_ctx *ctx, const mdbg_map_index *ix, const mdbg_minimizers *queries, uint32_t query_first_read,
                      const mdbg_map_params *p, mdbg_anchors **out);
int  mdbg_anchors_info(const mdbg_anchors *a, uint64_t info[4]);
int  mdbg_anchors_to_host(mdbg_ctx *ctx, const mdbg_anchors *a, uint64_t *pair_offsets, uint32_t *pair_ref_read, uint64_t *anchor_offsets,
                          uint32_t *ref_read, uint32_t *ref_position, uint32_t *ref_index, uint32_t *query_position, uint32_t *query_index,
                          uint8_t *reversed);
int  mdbg_anchors_device_ptrs(const mdbg_anchors *a, const void *d_ptrs[9]);
void mdbg_anchors_free(mdbg_anchors *a);
int  mdbg_map_chains(mdbg_ctx *ctx, const mdbg_anchors *a, const mdbg_map_params *p, mdbg_chains **out);
int  mdbg_chains_info(const mdbg_chains *c, uint64_t info[4]);
int  mdbg_chains_to_host(mdbg_ctx *ctx, const mdbg_chains *c, uint64_t *pair_offsets, mdbg_chain *chains, uint64_t *match_offsets, uint32_t *matches);
int  mdbg_chains_device_ptrs(const mdbg_chains *c, const void *d_ptrs[4]);
void mdbg_chains_free(mdbg_chains *c);
typedef struct mdbg_selection mdbg_selection;
typedef struct { uint32_t ref_read; int32_t score; uint32_t n_matches; uint32_t part; uint64_t pair; } mdbg_selected;   /* 24 bytes */
int  mdbg_map_select(mdbg_ctx *ctx, const mdbg_chains *chains, uint32_t coverage, mdbg_selection **out);
int  mdbg_selection_from_host(mdbg_ctx *ctx, uint64_t n_queries, const uint64_t *sel_offsets, const uint32_t *ref_read, const uint64_t *match_offsets,
                              const uint32_t *matches, mdbg_selection **out);
int  mdbg_map_select_merge(mdbg_ctx *ctx, const mdbg_selection *const *parts, uint32_t n_parts, uint32_t coverage, mdbg_selection **out);
int  mdbg_selection_to_alignment_bytes(mdbg_ctx *ctx, const mdbg_selection *sel, uint32_t query_first_read, mdbg_bytes **out, uint64_t *n_bytes /* optional */);
int  mdbg_selection_info(const mdbg_selection *s, uint64_t info[4]);
int  mdbg_selection_to_host(mdbg_ctx *ctx, const mdbg_selection *s, uint64_t *sel_offsets, mdbg_selected *rows, uint64_t *match_offsets, uint32_t *matches);
int  mdbg_selection_device_ptrs(const mdbg_selection *s, const void *d_ptrs[4]);
void mdbg_selection_free(mdbg_selection *s);
uint32_t mdbg_select_lds_positions(void);

/* ---- the selected pairs verified at correction density --------------------------------------------------------------------------------
 * Replaces ReadCorrectionFunctor::filterAlignments (readSelection/ReadCorrection.hpp:5006-5117): for every read to be corrected and every
 * neighbour the selection kept for it, the join of the two reads' minimizers at the full correction density, the chain of
 * MinimizerChainer::computeChainingAlignment (readSelection/MinimizerChainer.hpp:114-705; chainAnchors / argmaxPosition :735-961), and the
 * four tests of :5088-5094.  What survives is {neighbour, isQueryReversed}, the only input performPoaCorrection4 takes.
 *
 * Names.  The reference calls the read being corrected referenceRead and the other queryRead; the selection calls the read being corrected
 * the query and mdbg_selected::ref_read the other -- the opposite way round.  Here the read being corrected is the TARGET (a query of the
 * selection) and the other read the NEIGHBOUR (a ref_read of one of its rows); the fields reference_* belong to the target, query_* to the
 * neighbour, as in AlignmentResult2.
 *
 * mdbg_minimizers_attach_strands  gives a set that has attached positions the direction bytes (one per minimizer, 0 or 1) and the raw read
 *       lengths (one per read) a scan output has.  MDBG_EINVAL: a set without positions, a scan output, a direction byte other than 0 or 1
 *       (the message names the first offending read).
 *
 * mdbg_map_verify  `reads` is the set at correction density and holds the global reads [reads_first_read, reads_first_read + n); it must
 *       carry positions, directions and read lengths: a scan output, a concat of scan outputs, the density-thresholded form of either, or a
 *       host set given mdbg_minimizers_attach_positions and mdbg_minimizers_attach_strands; anything else is MDBG_EINVAL.  A slice
 *       (mdbg_minimizers_slice) carries offsets and values only and is refused like any other set without positions: to verify against a
 *       range of a resident scan output, concat the scans of that range, or pass the whole set and let the rows outside be ABSENT.  Target t of `sel` is global read
 *       target_first_read + t.  One mdbg_verified row per selected row, in the selection's order (row_offsets is the selection's
 *       sel_offsets); a row whose target or neighbour lies outside `reads` gets MDBG_VERIFY_ABSENT and zero fields (the reference's
 *       _mReads4.find miss, :5033).  ReadCorrectionFunctor::operator() does not correct targets below 10 minimizers at assembly density
 *       (Utils::isReadTooShort); that stays the caller's business: every listed target is verified.
 *       Anchors of a pair (:5051-5069): one for every (i, j) with target.m[i] == neighbour.m[j] -- ref_position = target.pos[i],
 *       query_position = neighbour.pos[j], reversed = target.dir[i] != neighbour.dir[j] -- in (i, j) order, which is the order the
 *       reference's sort by (ref_position, query_position) leaves (MinimizerChainer.hpp:154-159).  Fewer than 3: no chain (:146).
 *       Chain: the predecessor test, score, band and both tie rules are those mdbg_map_chains documents (:862-961, :735-858); the best
 *       anchor has the largest score, on a tie the smallest i (:810-815); its parents walked to the root are the chain, FIRST the root and
 *       LAST the best anchor; a chain of 3 anchors or fewer is no chain (:268; the mapper's limit is below 3).  Scores are integers; a pair
 *       of 209 715 anchors or more gets MDBG_VERIFY_TOO_LONG and zero fields, known after the count, before anything is allocated for it.
 *       Summary (:274-307, :356-428, :547-569, :581-582, :614, :657-673), n_t, n_q the minimizer counts, L_t, L_q the raw lengths, f and l
 *       the first and last anchor, ri / qi their indexes: query_reversed = f.qi > l.qi.  Forward: overhang_start = min(tpos[f.ri],
 *       qpos[f.qi]), start_mis = min(f.ri, f.qi), overhang_end = min(L_t - tpos[l.ri - 1], L_q - qpos[l.qi - 1]), end_mis = min(n_t - l.ri
 *       - 1, n_q - l.qi - 1).  Reversed: overhang_start = min(tpos[f.ri], L_q - qpos[f.qi - 1]), start_mis = min(f.ri, n_q - f.qi - 1),
 *       overhang_end = min(L_t - tpos[l.ri - 1], qpos[l.qi]), end_mis = min(n_t - l.ri - 1, l.qi).  (The - 1 on the indexes is the
 *       reference's own.)  Overhangs are int64 cut to 32 bits.  For consecutive chain anchors a, b: rg = b.ri - a.ri - 1, qg = b.qi - a.qi
 *       - 1 (a.qi - b.qi - 1 when reversed); mismatches += min(rg, qg), the excess of rg is deletions, of qg insertions.  n_matches = the
 *       chain's length, n_mismatches = start_mis + the sum + end_mis, n_seeds = min(matches + mismatches + deletions, matches + mismatches +
 *       insertions), align_length = l.ref_position - f.ref_position, reference_start / _end = f's / l's ref_position, query_start / _end =
 *       f's / l's query_position, swapped when reversed.
 *       Kept (:5088-5094) iff overhang_start <= max_overhang and overhang_end <= max_overhang and align_length >= min_overlap_length and
 *       identity >= min_identity, identity = 1.0 - (float)(1.0 - pow(n_matches / (long double)n_seeds, 1.0 / minimizer_size)), 1 when the
 *       two are equal.  The reference compares _alignLength with a float; min_overlap_length is a uint32_t here.  The device compares
 *       n_matches with a table the host makes with that very expression (mdbg_verify_min_matches) once a call.
 *       The kept list: per target (kept_offsets[n_targets + 1]) the rows with MDBG_VERIFY_KEPT in the rows' order -- ascending neighbour,
 *       as the reference walks alignedQueryReads -- as kept_neighbour (u32) and kept_reversed (u8).
 *       MDBG_EINVAL: max_chaining_band 0, minimizer_size 0, a min_identity that is not a number, a set without positions, directions or
 *       lengths.  MDBG_ERANGE: 2^32 anchors or
 *       more in one call.  An empty selection gives an empty result.  Timer names: "verify_join", "verify_chains", "verify_rows",
 *       "radix_sort".
 * mdbg_verification_info  targets, rows, chains found, kept.  _to_host: any array may be NULL.  device_ptrs, in order: row_offsets (u64),
 *       rows (mdbg_verified), kept_offsets (u64), kept_neighbour (u32), kept_reversed (u8).
 * mdbg_verify_lds_anchors  anchors of a pair up to which its scores and parents live in LDS, and minimizers of a neighbour up to which the
 *       join keeps its lookup in LDS; a longer one goes through global memory.
 * mdbg_verify_min_matches  host only, no context: min_matches[s], s = 0 ... n_seeds_max (n_seeds_max + 1 values), the smallest n_matches
 *       whose identity at n_seeds = s is not below min_identity, or s + 1 when none is.  MDBG_EINVAL: a null argument, minimizer_size 0,
 *       n_seeds_max = 2^32 - 1 (the table would have 2^32 values), a min_identity that is not a number (mdbg_map_verify refuses that too). */
typedef struct mdbg_verification mdbg_verification;
typedef struct { uint32_t max_chaining_band;   /* ReadCorrection.hpp:1739: 62 at 0.025 */
                 uint32_t max_overhang;        /* :5088-5089: 1000 */
                 uint32_t min_overlap_length;  /* :1638: 1000 */
                 float    min_identity;        /* :1639: 0.96f */
                 uint32_t minimizer_size;      /* Parameters::_minimizerSize, the root in the identity */
                 uint32_t reserved[3]; } mdbg_verify_params;
#define MDBG_VERIFY_CHAIN     1u   /* a chain of 4 anchors or more was found; the fields are set */
#define MDBG_VERIFY_KEPT      2u   /* ... and it passed the four tests */
#define MDBG_VERIFY_ABSENT    4u   /* the target or the neighbour is not in `reads` (the reference's _mReads4.find miss, :5033) */
#define MDBG_VERIFY_TOO_LONG  8u   /* 209 715 anchors or more: never an approximate chain (as MDBG_CHAIN_TOO_LONG) */
typedef struct { uint32_t neighbour, flags, query_reversed, n_anchors;
                 int32_t n_matches, n_mismatches, n_deletions, n_insertions;
                 uint32_t overhang_start, overhang_end, align_length, n_seeds;
                 uint32_t reference_start, reference_end, query_start, query_end; } mdbg_verified;   /* 64 bytes */
int  mdbg_minimizers_attach_strands(mdbg_ctx *ctx, mdbg_minimizers *m, const uint8_t *directions, const uint32_t *read_lengths);
int  mdbg_map_verify(mdbg_ctx *ctx, const mdbg_selection *sel, uint32_t target_first_read, const mdbg_minimizers *reads, uint32_t reads_first_read,
                     const mdbg_verify_params *p, mdbg_verification **out);
int  mdbg_verification_info(const mdbg_verification *v, uint64_t info[4]);
int  mdbg_verification_to_host(mdbg_ctx *ctx, const mdbg_verification *v, uint64_t *row_offsets, mdbg_verified *rows, uint64_t *kept_offsets,
                               uint32_t *kept_neighbour, uint8_t *kept_reversed);
int  mdbg_verification_device_ptrs(const mdbg_verification *v, const void *d_ptrs[5]);
void mdbg_verification_free(mdbg_verification *v);
uint32_t mdbg_verify_lds_anchors(void);
int  mdbg_verify_min_matches(const mdbg_verify_params *p, uint32_t n_seeds_max, uint32_t *min_matches);

/* ---- the kept pairs realigned at assembly density ------------------------------------------------------------------------------------------
 * The first half of ReadCorrectionFunctor::performPoaCorrection4 (readSelection/ReadCorrection.hpp:5217-5285): everything in front of the
 * POA graph.  Per target T (the read being corrected) and per kept neighbour N with its flag `reversed` (mdbg_map_verify's kept_neighbour /
 * kept_reversed), in the kept order:
 *   1. T' = Utils::getLowDensityMinimizerRead(T, assembly_density), N' likewise (Commons.hpp:2507-2574): a minimizer stays iff
 *      Murmur3_x64_128 of its value as 8 bytes, seed 42, is below density * 2^64 -- the rule and the code of mdbg_apply_density_threshold.
 *      Positions, directions and qualities go with the kept minimizers; length and read number stay.
 *   2. Utils::isReadTooShort(N') (Commons.hpp:2190): fewer than min_minimizers -- the pair is skipped (:5253), MDBG_REALIGN_SHORT.
 *   3. reversed: N' = N'.toReverseComplement() (Commons.hpp:1042-1079): the order of minimizers, positions, directions and qualities is
 *      turned round, then dir = !dir and pos = read length - pos.
 *   4. Anchors (:5263-5279): one for every (i, j) with T'.m[i] == N'.m[j]: ref_position = T'.pos[i], query_position = N'.pos[j],
 *      reversed = T'.dir[i] != N'.dir[j], indexes i, j into the thinned, oriented reads.
 *   5. MinimizerChainer::computeChainingAlignment(anchors, T', N', max_chaining_band) (MinimizerChainer.hpp:114-705) exactly as
 *      mdbg_map_verify documents it: sorted by (ref_position, query_position), fewer than 3 anchors no result, the chain, 3 anchors or
 *      fewer in it no result.  chain_reversed = f.qi > l.qi of the chain's first and last anchor.
 *   6. The list _alignments (:330-569) of pairs (ref_index, query_index), "none" for the reference's -1: start_mis pairs (r, q) counting up
 *      from (f.ri - start_mis, f.qi -+ start_mis); per chain link a -> b the pair of a, then mis + del pairs (r, none), then mis + ins
 *      pairs (none, q), mis = min(rg, qg) and the excesses deletions and insertions as in mdbg_map_verify; then the pair of l and
 *      end_mis pairs (r, q).  The query index runs downwards when chain_reversed.  start_mis / end_mis are mdbg_map_verify's, over the
 *      THINNED counts.
 *   7. normalizeAlignment (:1015-1111), one forward pass with in-place edits: an entry without a ref_index takes that of the first entry
 *      at or behind it that has one if the two minimizers are equal, and that entry loses it; an entry without a query_index likewise
 *      with the roles exchanged; an entry that has lost both is erased.  A robbed entry is visited later in the same pass: moves cascade.
 *   8. Graph::addAlignment2 (:1179-1271) reads per entry its kind -- insertion (no ref_index), deletion (no query_index), match
 *      (T'.m[ref_index] == N'.m[query_index]) or mismatch --, ref_index, N'.m[query_index] and N'.quality[query_index]: the entry arrays.
 * What stays with the caller is the graph: Graph(T'.minimizers, T'.qualities) -- the backbone arrays below --, addAlignment2, computePath2,
 * trimCorrectedPath.
 *
 * mdbg_map_realign  `reads` is the set mdbg_map_verify took (correction density, with positions, directions and lengths; the same refusals);
 *       the call thins it itself, once.  Qualities are the set's per-minimizer qualities where it has them (a scan output, a concat, a host
 *       set given mdbg_minimizers_attach_qualities), else 0.  The kept lists are read where they lie, on the device.
 *       mdbg_map_realign_pairs takes them as host arrays (kept_offsets[n_targets + 1] rising from 0, kept_neighbour, kept_reversed 0 or 1) and
 *       runs the same routine.  Target t is global read target_first_read + t; every listed target is processed, whatever its thinned
 *       length (ReadCorrection.hpp:4935-4938 stays the caller's business: target_offsets tells).
 *       Rows: one mdbg_realigned per kept pair in the kept order (row_offsets = kept_offsets).  A row outside `reads`: MDBG_REALIGN_ABSENT;
 *       a thinned neighbour below min_minimizers: MDBG_REALIGN_SHORT; 209 715 anchors or more: MDBG_REALIGN_TOO_LONG -- zero fields and no
 *       entries each.  No chain: flags 0, n_anchors kept.  A chain: MDBG_REALIGN_CHAIN, the counts as AlignmentResult2 holds them (taken
 *       BEFORE normalisation, as the reference leaves them), _referenceStartIndex / _referenceEndIndex, and n_entries, the length of the
 *       final list.
 *       Entries (entry_offsets[rows + 1], after normalisation): ref_index (u32, 0xFFFFFFFF none), query_index (u32, into the thinned,
 *       oriented neighbour, 0xFFFFFFFF none), query_minimizer (u32), query_quality (u8) -- both 0 for a deletion --, kind (u8: 0 match,
 *       1 mismatch, 2 insertion, 3 deletion).  The backbone: target_offsets[targets + 1], target_minimizer (u32), target_quality (u8): T' of
 *       every listed target, with or without a kept row; empty for a target outside `reads`.
 *       MDBG_EINVAL: max_chaining_band 0, a density that is not > 0, min_minimizers 0, a null argument, a set without positions,
 *       directions or lengths, kept offsets that do not rise from 0, a kept_reversed other than 0 or 1.  MDBG_ERANGE: 2^32 anchors or
 *       entries or more in one call.  Empty input gives an empty result.  Timer names: "realign_thin", "realign_join", "realign_chains",
 *       "realign_lists", "radix_sort".
 * mdbg_realignment_info  targets, rows, chains, entries.  _to_host: any array may be NULL (target_offsets first tells the backbone's size).
 *       device_ptrs, in order: row_offsets (u64), rows (mdbg_realigned), entry_offsets (u64), ref_index (u32), query_index (u32),
 *       query_minimizer (u32), query_quality (u8), kind (u8), target_offsets (u64), target_minimizer (u32), target_quality (u8).
 * mdbg_realign_lds_entries  raw entries of a row up to which its list is normalised in LDS; a longer list goes through global memory.
 * mdbg_minimizers_attach_qualities  gives a set that has attached positions one quality byte per minimizer (what a scan output carries).
 *       MDBG_EINVAL: a set without positions, a scan output. */
typedef struct mdbg_realignment mdbg_realignment;
typedef struct { uint32_t max_chaining_band;   /* ReadCorrection.hpp:1739, used at :5281: 62 at 0.025 */
                 float    assembly_density;    /* Parameters::_minimizerDensity_assembly, 0.005f */
                 uint32_t min_minimizers;      /* Utils::isReadTooShort: 10 */
                 uint32_t reserved[5]; } mdbg_realign_params;                       /* 32 bytes */
#define MDBG_REALIGN_CHAIN     1u   /* a chain of 4 anchors or more; the row's entries are present */
#define MDBG_REALIGN_ABSENT    4u   /* target or neighbour not in `reads` */
#define MDBG_REALIGN_TOO_LONG  8u   /* 209 715 anchors or more (as MDBG_VERIFY_TOO_LONG) */
#define MDBG_REALIGN_SHORT    16u   /* the thinned neighbour has fewer than min_minimizers (:5253) */
typedef struct { uint32_t neighbour, flags, oriented_reversed /* the flag given */, chain_reversed /* f.qi > l.qi */;
                 uint32_t n_anchors, n_entries;
                 int32_t  n_matches, n_mismatches, n_deletions, n_insertions;      /* AlignmentResult2's counts, before normalisation */
                 uint32_t reference_start_index, reference_end_index; } mdbg_realigned;   /* 48 bytes */
int  mdbg_map_realign(mdbg_ctx *ctx, const mdbg_verification *v, uint32_t target_first_read, const mdbg_minimizers *reads, uint32_t reads_first_read,
                      const mdbg_realign_params *p, mdbg_realignment **out);
int  mdbg_map_realign_pairs(mdbg_ctx *ctx, uint64_t n_targets, const uint64_t *kept_offsets, const uint32_t *kept_neighbour, const uint8_t *kept_reversed,
                            uint32_t target_first_read, const mdbg_minimizers *reads, uint32_t reads_first_read, const mdbg_realign_params *p, mdbg_realignment **out);
int  mdbg_realignment_info(const mdbg_realignment *r, uint64_t info[4]);
int  mdbg_realignment_to_host(mdbg_ctx *ctx, const mdbg_realignment *r, uint64_t *row_offsets, mdbg_realigned *rows, uint64_t *entry_offsets, uint32_t *ref_index,
                              uint32_t *query_index, uint32_t *query_minimizer, uint8_t *query_quality, uint8_t *kind, uint64_t *target_offsets,
                              uint32_t *target_minimizer, uint8_t *target_quality);
int  mdbg_realignment_device_ptrs(const mdbg_realignment *r, const void *d_ptrs[11]);
void mdbg_realignment_free(mdbg_realignment *r);
uint32_t mdbg_realign_lds_entries(void);
int  mdbg_minimizers_attach_qualities(mdbg_ctx *ctx, mdbg_minimizers *m, const uint8_t *qualities);
/* The library's stable radix sort (8-bit digits, least significant first; a digit in which all keys agree is skipped) on caller-chosen
   data: n uint64 keys from byte keys_at of `keys` and their n uint32 values from byte values_at of `values`, sorted by key in place, equal
   keys keeping their order.  Returns when done.  info (optional): digit passes run, digit passes skipped.  MDBG_EINVAL: a null argument,
   keys_at not a multiple of 8, values_at not a multiple of 4, a range that leaves its object, overlapping ranges of one object.
   MDBG_ERANGE: 2^32 items or more.  Timer name: "radix_sort". */
int  mdbg_bytes_sort_u64_pairs(mdbg_ctx *ctx, mdbg_bytes *keys, uint64_t keys_at, mdbg_bytes *values, uint64_t values_at, uint64_t n,
                               uint64_t info[2]);

/* ---- FASTA / FASTQ text taken apart on the device -----------------------------------------------------------------------------------
 * Replaces the host side of ReadParserParallel for a plain file: the kseq loop (KSEQ_INIT(gzFile, gzread), Commons.hpp:82) that
 * ReadParser::parse / ReadParserParallel::parse run over every character (Commons.hpp:5827-5922).  The file's bytes travel as they are
 * (mdbg_bytes_*); records are found, stripped of line ends and packed by kernels.  The result is the mdbg_reads that
 * mdbg_reads_from_ascii builds from the same records (words, offsets, lengths, side masks, masked list, qualities).
 *
 * [begin, end) of `text` holds a whole number of records -- a whole file, or a slab cut at record starts -- and text[begin] is '>'
 * (FASTA) or '@' (FASTQ); anything else is MDBG_EINVAL.  An empty range gives zero reads.  Uploads still in flight on `text` are
 * waited for on the device.  info (optional) receives {format (0 FASTA, 1 FASTQ), n_reads, n_bases, n_masked}.
 *
 * FASTA: a record starts at every line whose first byte is '>'; that line is skipped; the sequence is every byte of the following
 *        lines except \n, \r, space and tab (multi-line, LF or CR-LF, blank lines, a last line without \n).  A header directly
 *        followed by a header is a read of length 0.  A non-header line that starts with '@' or '+' is refused (MDBG_EINVAL): kseq
 *        would switch format there.
 * FASTQ: four lines per record, counted, not recognised by their first byte (a quality line may start with '@' or '+'): line 4i
 *        starts with '@', line 4i+2 with '+', line 4i+3 has as many bytes as line 4i+1 (one trailing \r dropped from both).  Lines of
 *        nothing but \r after the last record are ignored.  Multi-line FASTQ, a length mismatch and a truncated last record are
 *        MDBG_EINVAL with a message that names the first offending line; nothing is built.  Bases are stripped of space, tab and \r
 *        as in FASTA (the quality of a stripped byte goes with it); quality bytes are otherwise passed through unchanged.
 * A read longer than 0xFFFFFFF0 bases is MDBG_ERANGE. */
int  mdbg_reads_from_fastx_bytes(mdbg_ctx *ctx, const mdbg_bytes *text, uint64_t begin, uint64_t end, mdbg_reads **out, uint64_t info[4]);

/* ---- BGZF blocks inflated on the device ------------------------------------------------------------------------------------------------
 * Replaces gzread under the same kseq loop (KSEQ_INIT(gzFile, gzread), Commons.hpp:82; the read loop, Commons.hpp:5842-5870) for BGZF
 * input -- what samtools fastq, bam2fastq and bgzip write: independent gzip members of at most 64 KB, each stating its compressed and
 * its uncompressed size.  The caller reads the block table from the members' headers and trailers; the compressed bytes travel as they
 * are (mdbg_bytes_*) and are inflated into an mdbg_bytes that mdbg_reads_from_fastx_bytes reads.
 *
 * mdbg_bgzf_block   src: offset in `comp` of the block's raw DEFLATE payload (behind the 12 + XLEN header bytes); csize: payload bytes;
 *                   isize, crc: the member's trailer.  csize <= 65536 and isize <= 65536.
 * mdbg_bytes_inflate_bgzf
 *     Block i inflates to text[text_at + sum(isize[0..i)) ...); *n_text is the total.  Uploads still in flight on `comp` (and `text`)
 *     are waited for on the device.  The call returns after the per-block status words have been read back: a later
 *     mdbg_reads_from_fastx_bytes on `text` needs no extra synchronisation.  n_blocks == 0 and blocks with isize == 0 (the EOF marker)
 *     are fine.
 *     MDBG_EINVAL: a null argument; a block whose [src, src + csize) lies outside `comp`; csize > 65536; isize > 65536; a total that does not fit
 *     `text` behind text_at (nothing has run then); or a block that does not decode -- the message names the first such block's index
 *     and the reason: reserved block type / stored LEN/NLEN mismatch / over-subscribed or unusably incomplete code / invalid symbol /
 *     distance beyond the block's own output / input exhausted / output not equal to isize / CRC-32 mismatch.  On error nothing is
 *     promised about the bytes of `text` inside [text_at, text_at + total); bytes outside it are never written in any case.
 *     Decoding: a raw DEFLATE stream (RFC 1951) per block, any number of stored, fixed and dynamic deflate blocks -- everything zlib's
 *     deflate emits at every level and strategy.  A distance code with a single length-1 code, or with none, is accepted (as zlib and
 *     host/inflate.hpp do); every other incomplete code is refused.  A BGZF block never refers to bytes before its own output: the
 *     window is the block.  The CRC-32 (gzip polynomial, reflected) is computed on the device over the produced bytes.
 * mdbg_bytes_download
 *     a plain synchronous device-to-host copy of [at, at + n) of `b`; MDBG_EINVAL outside the buffer.
 * mdbg_fastx_whole_records
 *     where the last whole record of text[begin, end) ends when more text may follow `end`: text[begin] must start a record; *format is
 *     0 for '>' and 1 for '@' (anything else, or an empty range: MDBG_EINVAL).  *cut is the largest offset in (begin, end] up to which
 *     [begin, cut) is known to hold whole records.  FASTA: the offset of the last '>' that directly follows a '\n'; none behind begin:
 *     begin.  FASTQ: the four-line rule of mdbg_reads_from_fastx_bytes -- with N the '\n' in the range, the offset just behind
 *     newline number 4 * floor(N / 4); N < 4: begin. */
typedef struct { uint64_t src; uint32_t csize, isize, crc, reserved; } mdbg_bgzf_block;
int  mdbg_bytes_inflate_bgzf(mdbg_ctx *ctx, const mdbg_bytes *comp, const mdbg_bgzf_block *blocks, uint64_t n_blocks,
                             mdbg_bytes *text, uint64_t text_at, uint64_t *n_text);
int  mdbg_bytes_download(mdbg_ctx *ctx, const mdbg_bytes *b, uint64_t at, void *host, uint64_t n);
int  mdbg_fastx_whole_records(mdbg_ctx *ctx, const mdbg_bytes *text, uint64_t begin, uint64_t end, uint64_t *cut, int *format);

/* ---- ordinary gzip inflated on the device ---------------------------------------------------------------------------------------------
 * Replaces gzread under the same kseq loop for gzip input that is not BGZF -- what gzip, pigz and zlib write: one deflate stream per
 * member, no index, every block free to refer to the 32 KB in front of it.  The scheme is the two-pass one of host/gzip_parallel.hpp:
 * the caller cuts the compressed file into CHUNKS that start at deflate block headers (finding them stays on the host:
 * mdbg_host::gzip_find_block); the device decodes every chunk without its window into 16-bit symbols, resolves the windows in order,
 * translates the symbols to text and checks every member that ended against its trailer.
 *
 * mdbg_gzip_stream   what one gzip FILE carries from call to call: the last 32 KB of text, the open member's CRC register and length.
 *                    It advances only when a call succeeds.
 * mdbg_gzip_chunk    bits [start_bit, stop_bit) counted from the start of `comp`.  chunks[i].stop_bit == chunks[i + 1].start_bit.  A
 *                    chunk is decoded from start_bit and must end exactly on stop_bit, at a block boundary; behind a member's last block
 *                    that boundary is the next member's first block header (trailer and header are read by the chunk the member ends
 *                    in), or, for the last chunk of a call, the byte behind the trailer.  The last chunk's stop_bit is the next call's
 *                    first start or MDBG_GZIP_TO_END: through the end of the last member -- what follows it and is no gzip member header
 *                    is ignored, as gzread does.  On a fresh stream (and after a call that ended behind a trailer) chunks[0].start_bit is
 *                    the byte-aligned position of a gzip member header, which the device reads (magic, CM = 8, FEXTRA / FNAME / FCOMMENT /
 *                    FHCRC by its flags); every other start is a deflate block header inside a member.  A chunk spans at most 2 MB.
 * mdbg_bytes_inflate_gzip
 *     The text is contiguous at text[text_at ...), *n_text its length; info (optional) = {n_text, members that ended in this call, 1 if
 *     the file's last member ended, the bit just behind the last bit consumed}.  `comp` may be re-based from call to call (the bits
 *     count from its start).  Uploads still in flight on `comp` (and `text`) are waited for on the device; the call returns after the
 *     verdicts have been read back.
 *     MDBG_EINVAL: a null argument, a chunk outside `comp`, or a chunk that does not decode -- the message names the first such chunk and
 *     the reason: those of mdbg_bytes_inflate_bgzf, or: ran past the next chunk's start (that start was not a block header) / reference
 *     before the member's start / bad member header / length does not match ISIZE / CRC-32 mismatch / the stream ended in front of the
 *     chunk's stop.  MDBG_ERANGE: the text does not fit behind text_at; *n_text then holds the room needed and nothing of the stream has
 *     changed.  Bytes of `text` outside [text_at, text_at + n_text) are never written.
 * mdbg_bytes_copy
 *     a device copy of src[src_at, +n) to dst[dst_at, +n), ordered on the context's stream behind the uploads of both; MDBG_EINVAL when a
 *     range lies outside its buffer or the two overlap in one buffer. */
typedef struct mdbg_gzip_stream mdbg_gzip_stream;
typedef struct { uint64_t start_bit, stop_bit; } mdbg_gzip_chunk;
#define MDBG_GZIP_TO_END (~0ull)
int  mdbg_gzip_stream_create(mdbg_ctx *ctx, mdbg_gzip_stream **out);
void mdbg_gzip_stream_free(mdbg_gzip_stream *s);
int  mdbg_bytes_inflate_gzip(mdbg_ctx *ctx, mdbg_gzip_stream *s, const mdbg_bytes *comp, const mdbg_gzip_chunk *chunks, uint64_t n_chunks,
                             mdbg_bytes *text, uint64_t text_at, uint64_t *n_text, uint64_t info[4]);
int  mdbg_bytes_copy(mdbg_ctx *ctx, mdbg_bytes *dst, uint64_t dst_at, const mdbg_bytes *src, uint64_t src_at, uint64_t n);
/* Exclusive prefix sums of n unsigned values of `width` bytes (4 or 8) that start at byte in_at of `in`:
   n + 1 uint64 values (the last one the total) written from byte out_at of `out`.  The library's own device-wide scan (every CSR offset
   array, every flags -> rows compaction) on caller-chosen values, sizes and alignments; queued on the context's stream behind the uploads of
   both objects, not waited for.  n == 0 writes the single total 0.  MDBG_EINVAL: a null argument, a width other than 4 or 8, in_at not a
   multiple of width, out_at not a multiple of 8, a range that leaves its object, `in` and `out` one object with overlapping ranges. */
int  mdbg_bytes_prefix_sum(mdbg_ctx *ctx, const mdbg_bytes *in, uint64_t in_at, int width, uint64_t n,
                           mdbg_bytes *out, uint64_t out_at);

/* Page-locked host memory for read batches handed to mdbg_reads_from_ascii / _from_packed: uploads from it
 * run at PCIe rate instead of through the driver's staging copies.  Release with mdbg_host_free. */
int  mdbg_host_alloc(mdbg_ctx *ctx, size_t bytes, void **out);
void mdbg_host_free(mdbg_ctx *ctx, void *p);

/* Stream-ordered device-to-device copy on the context stream followed by a synchronize; lets a
 * harness move library-owned rows into buffers it owns (e.g. torch tensors for RCCL). */
int  mdbg_memcpy_device(mdbg_ctx *ctx, void *dst, const void *src, uint64_t bytes);

/* ---- sharded first pass (one process per GPU; the caller moves the bytes, e.g. RCCL all-to-all over xGMI) ----
 * Reads shard across ranks; only the counts are global.  Keys are partitioned by owner rank (top bits of hash_hi
 * scaled to [0, n_ranks), n_ranks <= 64).  Per rank and step:
 *     mdbg_shard_begin   local counts -> rows [hash_lo, hash_hi, count] grouped by owner                (send: all-to-all)
 *     mdbg_shard_reduce  owner sums the rows it received; reply[i] answers received row i                 (send back: all-to-all
 *                        with the transposed split sizes; replies arrive in the order the rows were sent)
 *     mdbg_shard_finish  global counts -> this rank's share of the solid rows + rescue of its own reads
 * A reply is the GLOBAL count of the row's key (low 32 bits) plus bit 63 on exactly one of the rows of each key: the
 * rank that sent that row lists the key in its table, with the vector from its own reads -- vectors never travel.
 * The union over ranks of the finished tables equals mdbg_kminmer_count_first on the union of the reads.
 * Nearest reference analogue: KminmerCounter's on-disk partitioning `vecHash % _nbPartitions`
 * (graph/CreateMdbg.hpp:3714-3724).  Rows are mdbg_row_words(k) = 3 u64 words each. */
typedef struct mdbg_shard mdbg_shard;
uint32_t mdbg_row_words(uint32_t k);
/* *d_rows: device rows of every distinct local key, owner 0 first; counts[r] = rows for rank r.  `reads` must stay
 * alive until mdbg_shard_free. */
int  mdbg_shard_begin(mdbg_ctx *ctx, const mdbg_minimizers *reads, uint32_t k, uint32_t n_ranks,
                      mdbg_shard **shard, const uint64_t **d_rows, uint64_t *counts);
/* d_recv: device rows received from all ranks (any order; free to reuse once the call returns).
 * *d_reply: n_recv u64, aligned with d_recv, valid until mdbg_shard_free. */
int  mdbg_shard_reduce(mdbg_ctx *ctx, mdbg_shard *shard, const uint64_t *d_recv, uint64_t n_recv, const uint64_t **d_reply);
/* d_replies: n_sent u64, the replies for the rows of mdbg_shard_begin in the order they were sent. */
int  mdbg_shard_finish(mdbg_ctx *ctx, mdbg_shard *shard, const uint64_t *d_replies, uint32_t min_abundance, mdbg_table **out);
/* Both exchanges of a sharded pass among `n` shards that live on one device (begun with n_ranks = n on contexts of that device):
 * rows to their owners, mdbg_shard_reduce on every owner, the replies back in the order the rows were sent -- what
 * mdbg_shard_exchange does between GPUs, with device-to-device copies in place of the wire.  counts[src * n + dst] = rows shard
 * src holds for owner dst (the `counts` of its mdbg_shard_begin / _from_table), d_rows[src] its rows; d_replies[src] receives the
 * replies for mdbg_shard_finish / _keep (owned by the shard).  For a job that checks itself against the union of shards (bench.py's
 * self-checks: the table of a whole read set against the shares of its halves) and for tests; nothing in the reference
 * corresponds to it -- its partitions meet on disk (graph/CreateMdbg.hpp:3714-3851). */
int  mdbg_shard_exchange_local(mdbg_ctx *ctx, mdbg_shard *const *shards, uint32_t n, const uint64_t *const *d_rows, const uint64_t *counts,
                               const uint64_t **d_replies);
void mdbg_shard_free(mdbg_shard *shard);
/* Sharded k > firstK (the refined pass and the index passes, graph/CreateMdbg.cpp:391-468).  The abundance of a k-min-mer at
 * these k is a function of the key and the previous table, not of a count, so nothing is summed: every rank holds the whole
 * previous table (20 bytes per key: a few hundred MB at 40 M reads -- all-gather the records of the previous step and load them
 * with mdbg_prev_from_records), runs mdbg_kminmer_count_refined / mdbg_kminmer_index over ITS reads, and the ranks then only
 * agree on who lists a key that several of them found:
 *     mdbg_shard_from_table  rows [hash_lo, hash_hi, abundance] of the local table grouped by owner           (send: all-to-all)
 *     mdbg_shard_reduce      the owner marks the first row of every key (bit 63 of its reply), as in the first pass
 *     mdbg_shard_keep        the rows this rank was told to list, vectors included when the table has them
 * The union over ranks of the kept tables equals the single-GPU table over the union of the reads.  `local` must stay alive
 * until mdbg_shard_free; the exchange in between is mdbg_shard_exchange or the caller's own. */
int  mdbg_shard_from_table(mdbg_ctx *ctx, const mdbg_table *local, uint32_t n_ranks, mdbg_shard **shard, const uint64_t **d_rows,
                           uint64_t *counts);
int  mdbg_shard_keep(mdbg_ctx *ctx, mdbg_shard *shard, const uint64_t *d_replies, mdbg_table **out);

/* ---- the exchange inside the library: peer copies or RCCL point-to-point, over xGMI --------------------------------
 * For callers that do not want to move the bytes themselves (the C++ pipeline: src/pipeline has no communication layer).
 * One communicator per context that takes part; rank 0 makes the id (128 bytes) and hands it to the other ranks by whatever
 * means it has (a file in the shared tmp dir, a socket, MPI, torch.distributed -- bench.py broadcasts it).  Ranks may be
 * processes (one per GPU) or threads of one process driving one context each (mdbg_tool graph --gpus G).
 *     mdbg_comm_unique_id    ncclGetUniqueId (128 random bytes when RCCL is not installed: enough for MDBG_COMM_PEER)
 *     mdbg_comm_create_mode  collective, every rank calls it with the same id and mode:
 *         MDBG_COMM_PEER   the two all-to-alls as PEER COPIES.  Every rank stages its rows (grouped by owner) and later its replies in
 *                          a buffer of its own; every owner PULLS its slice from every sender with a device-to-device copy, one
 *                          stream per peer, so the seven xGMI links of a GPU carry their slices at once; the replies travel the
 *                          same way back.  Between processes the buffers are shared by hipIpcGetMemHandle / hipIpcOpenMemHandle,
 *                          between threads of one process they are plain pointers (peer access enabled between the devices).  The
 *                          hand-shakes -- the count matrix, "my rows are staged", the status words of the failure protocol below --
 *                          are words in a block of host memory the ranks share (csrc/peerlink.hpp: a POSIX shared-memory object named
 *                          after the id, unlinked once everybody is attached), polled with a deadline (MDBG_PEER_TIMEOUT_S, default
 *                          120): no collective kernel has to become resident beside another batch's scan -- RCCL's needs 37.6 KB of
 *                          LDS a block, a scan leaves 28 -- and no exchange can hang.  Creation ends with a self-test: a small
 *                          exchange of known rows through the very buffers, whose verdicts the ranks agree on.
 *         MDBG_COMM_RCCL   ncclCommInitRank; every transfer an ncclSend / ncclRecv pair inside one group.  RCCL is loaded on first use.
 *         MDBG_COMM_AUTO   peer copies if every rank attaches and passes the self-test, otherwise -- all ranks together -- RCCL
 *                          (mdbg_comm_note says why).  A caller with other batches' scans in flight then keeps them off the device
 *                          during an exchange (bench.py's exchange gate).
 *         MDBG_COMM_DEFAULT  the environment's MDBG_COMM_MODE = peer | rccl | auto, "auto" when unset
 *     mdbg_comm_create       = mdbg_comm_create_mode(..., MDBG_COMM_DEFAULT, ...)
 *     mdbg_comm_adopt        wraps a communicator the caller already has (an ncclComm_t); mdbg_comm_destroy leaves it alive
 *     mdbg_comm_mode         the transport a communicator ended up with (MDBG_COMM_PEER or MDBG_COMM_RCCL)
 *     mdbg_comm_destroy      collective in peer mode (a rank frees its staging buffers once its peers have let go of them; bounded wait)
 * mdbg_kminmer_count_first_sharded = mdbg_shard_begin -> rows to their owner ranks -> mdbg_shard_reduce -> replies back ->
 * mdbg_shard_finish, all on the context's stream (the pulls on side streams it waits for).  Collective: every rank of the
 * communicator calls it, in the same order if a rank drives several communicators.  The union over ranks of the tables equals
 * mdbg_kminmer_count_first over the union of the reads.  Replaces, across GPUs, KminmerCounter's partition-to-disk +
 * per-partition dereplication (graph/CreateMdbg.hpp:3714-3724, :3744-3851). */
typedef struct mdbg_comm mdbg_comm;
#define MDBG_COMM_ID_BYTES 128
int  mdbg_comm_unique_id(uint8_t *id128);
#define MDBG_COMM_DEFAULT (-1)
#define MDBG_COMM_RCCL    0
#define MDBG_COMM_PEER    1
#define MDBG_COMM_AUTO    2
int  mdbg_comm_create(mdbg_ctx *ctx, const uint8_t *id128, int rank, int n_ranks, mdbg_comm **out);
int  mdbg_comm_create_mode(mdbg_ctx *ctx, const uint8_t *id128, int rank, int n_ranks, int mode, mdbg_comm **out);
int  mdbg_comm_mode(const mdbg_comm *comm);
const char *mdbg_comm_note(const mdbg_comm *comm);     /* "auto" that ended on RCCL: why the peer copies were not taken; else "" */
int  mdbg_comm_adopt(mdbg_ctx *ctx, void *nccl_comm, int rank, int n_ranks, mdbg_comm **out);
void mdbg_comm_destroy(mdbg_comm *comm);
/* What the communicator has carried: stats[0] = rank, [1] = ranks as the caller gave them, [2] = ncclCommCount (RCCL: create / adopt
 * fail unless it equals [1] and ncclCommUserRank equals [0]; 0 for peer copies), [3] = completed exchanges, [4] / [5] = bytes that went
 * to / came from OTHER ranks (rows and replies; peer copies: what the peers pulled from this rank / what it pulled), [6] = bytes of the
 * rank's own share (device-to-device copies, never on the wire), [7] = ncclCommUserRank; *exchange_ms (may be NULL) = host wall
 * time spent inside mdbg_shard_exchange. */
int  mdbg_comm_stats(const mdbg_comm *comm, uint64_t stats[8], double *exchange_ms);
/* Where the time inside mdbg_shard_exchange went (peer copies; RCCL reports [1] = [2] = 0): ms[0] = the whole call (= *exchange_ms above),
 * ms[1] = the owner's reduction (mdbg_shard_reduce: this rank's device work), ms[2] = waiting -- for this rank's own copies to land and
 * for its peers to reach a phase.  ms[0] - ms[1] - ms[2] is the transport's own host time. */
int  mdbg_comm_times(const mdbg_comm *comm, double ms[3]);
int  mdbg_kminmer_count_first_sharded(mdbg_ctx *ctx, mdbg_comm *comm, const mdbg_minimizers *reads, uint32_t k,
                                      uint32_t min_abundance, mdbg_table **out);
/* The collective middle part alone, between mdbg_shard_begin and mdbg_shard_finish (a caller with several batches in flight
 * overlaps the local halves and takes turns on the wire): d_rows / counts as mdbg_shard_begin returned them; *d_replies (one
 * u64 per sent row, in the order sent) is what mdbg_shard_finish takes and stays valid until the next exchange on `comm`. */
int  mdbg_shard_exchange(mdbg_ctx *ctx, mdbg_comm *comm, mdbg_shard *shard, const uint64_t *d_rows, const uint64_t *counts,
                         const uint64_t **d_replies);
/* Failure behaviour of the collective calls.  An exchange is: counts all-gathered -> rows to owners -> reduction -> replies.
 * Before each transfer the ranks agree (a status word per rank: all-gathered over RCCL, or written to the shared control block of
 * the peer copies, where waiting for a rank that died ends at a deadline with MDBG_EPEER) that everybody got that far: a rank that failed
 * locally -- bad argument, allocation, reduction -- still takes part in that small collective with its error code, returns its
 * own error, and every other rank returns MDBG_EPEER naming it; nobody is left waiting in a receive.  Send / receive groups
 * are closed on every path (an open group would swallow the thread's next RCCL call); a communicator on which an RCCL call
 * itself failed is marked broken: later exchanges on it fail at once and mdbg_comm_destroy aborts it.
 * mdbg_shard_abort is for the caller that drives begin / exchange / finish itself: when its local half (mdbg_shard_begin,
 * mdbg_shard_from_table, anything before the exchange) failed with `code`, it calls this INSTEAD of mdbg_shard_exchange so
 * that the peers, who are about to enter theirs, return MDBG_EPEER.  Returns MDBG_OK once the peers have been told. */
int  mdbg_shard_abort(mdbg_ctx *ctx, mdbg_comm *comm, int code);

#ifdef __cplusplus
}
#endif
#endif
