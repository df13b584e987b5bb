/*
 * pgx.h -- C ABI of the MI355X-native find_mems path (libpgx.so).
 *
 * The reference (parsaeskandar/pangenome-index @ 2025-10-24) has no FFI layer: its boundary is the
 * `find_mems` process contract plus C++ member functions compiled into each CLI.  This header is
 * the flat boundary a maintainer would bind instead; every entry point names the reference code
 * it replaces (paths relative to /root/reference).  Plain pointers and sizes only; no exceptions
 * cross this boundary; every function returns a pgx_status and pgx_last_error() holds the text.
 *
 * There is NO CPU fallback behind these entry points: anything that computes (rank / extend /
 * find_mems / tag queries) runs as HIP kernels on a gfx950 device and fails with
 * PGX_ERR_NO_DEVICE when none is usable.
 */
#ifndef PGX_H
#define PGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_ABI_VERSION 7 /* 2: pgx_timing grew (pairs_reads, redo_reads), pgx_index_info.image_pairs, PGX_MODE_IMAGE_PAIRS; 3: pgx_timing grew (ms_find_mems_main, traffic counters); 4: pgx_timing.ms_per_upload, pgx_pack_reads, pgx_batch_upload_packed; 5: pgx_batch_upload_text, pgx_fastx_cut, PGX_READS_*; 6: pgx_batch_locate, pgx_batch_locations, pgx_batch_device_locations, pgx_locations, PGX_LOCATE_CHAINS; 7: pgx_timing.kernels, PGX_KERNELS_*, pgx_kernel_variants; still 7, additions a caller of 7 does not see: PGX_LOCATE_SEQ_SETS (a flag 7 refused), pgx_locations.set_words (the field `reserved`, always 0 before, at the same offset), the compact result (pgx_compact_result, pgx_batch_result_compact, pgx_compact_expand, pgx_compact_bound, pgx_compact_encode: new entry points only), the device index build (pgx_build_index_from_text_device, pgx_build_index_from_texts_device, pgx_build_index_device_timing: new entry points only), the text output (pgx_batch_format, pgx_format_result, pgx_format_params, pgx_text, PGX_FORMAT_*: new entry points only), the image file (pgx_index_save_image, pgx_index_open_image, pgx_image_file_info, pgx_image_sum, pgx_image_section_name, PGX_IMAGE_*: new entry points only), the read-back of a batch's reads (pgx_batch_reads, pgx_reads_info: a new entry point only), the read hits (pgx_batch_read_hits, pgx_batch_hits, pgx_batch_device_hits, pgx_read_hits_arrays, pgx_read_hit, pgx_read_hits, PGX_HITS_*, PGX_NO_SEQUENCE: new entry points only), the read walk (pgx_batch_read_walk, pgx_batch_walked, pgx_batch_device_walked, pgx_index_paths, pgx_read_walk_arrays, pgx_read_walk, pgx_read_walks, PGX_WALK_STEPS: new entry points only) */

typedef enum {
    PGX_OK = 0,
    PGX_ERR_IO = 1,          /* cannot open / read (find_mems.cpp:30,91 exit(EXIT_FAILURE)) */
    PGX_ERR_FORMAT = 2,      /* sdsl::simple_sds::InvalidData in the reference (r-index.cpp:412-419) */
    PGX_ERR_UNSUPPORTED = 3, /* valid file, but a shape this build does not handle */
    PGX_ERR_NO_DEVICE = 4,   /* no usable HIP device / kernel image */
    PGX_ERR_HIP = 5,         /* a HIP runtime call failed */
    PGX_ERR_ARG = 6,
    PGX_ERR_NOMEM = 7
} pgx_status;

/* mode: which extension tables are loaded into the device image (same kernels either way) */
#define PGX_MODE_COMPAT 0u /* bit-exact with the reference, quirks included (default)          */
#define PGX_MODE_STRICT 1u /* textbook FMD over the true ranks; equals COMPAT on sigma=6 indexes */
/* optional bits or-ed into `mode`: force the layout of the device rank image (default: chosen from the index size;
 * results never depend on it).  PGX_ERR_UNSUPPORTED if dense is forced on a legacy-layout index without N in COMPAT. */
#define PGX_MODE_IMAGE_RL 0x100u    /* run-length blocks + directory (any size)                     */
#define PGX_MODE_IMAGE_DENSE 0x200u /* uncompressed bit planes, n bytes of device memory (64 symbols per 64-byte block)       */
#define PGX_MODE_IMAGE_DENSE2 0x400u /* two bit planes + exception runs, n / 3 bytes (384 symbols per 128-byte block; n < 2^32) */
#define PGX_MODE_IMAGE_PAIRS 0x800u  /* dense2 + the two-step PAIRS image, 4 n / 3 bytes more (n < 2^32, textbook extension tables, few N runs);
                                      * by default a PAIRS image accompanies whichever dense layout is chosen, when the index qualifies */
#define PGX_MODE_IMAGE_WIDE 0x1000u  /* modifier: the 64-bit form of dense2 / PAIRS (header counts as deltas against superblock bases, 64-bit
                                      * kernels), automatic for BWTs of 2^32 symbols or more; alone it selects dense2 + PAIRS */
#define PGX_MODE_MASK 0xFFu

/* tag file formats (SURVEY section 5 "Tag formats") */
#define PGX_TAGS_AUTO 0u
#define PGX_TAGS_BYTECODE 1u /* TagArray::load_compressed_tags      src/tag_arrays.cpp:739-763 */
#define PGX_TAGS_COMPACT 2u  /* TagArray::load_compressed_tags_sdsl src/tag_arrays.cpp:766-776 */

/* struct MEM, include/pangenome_index/algorithm.hpp:644-651 (32 bytes, same field order) */
typedef struct {
    uint64_t start;
    uint64_t end;
    uint64_t bwt_start;
    int64_t size;
} pgx_mem;

/* FastLocate::bi_interval, include/pangenome_index/r-index.hpp:118-130 */
typedef struct {
    uint64_t forward;
    uint64_t reverse;
    int64_t size;
} pgx_biint;

typedef struct pgx_index pgx_index; /* FastLocate + TagArray, host image + per-device images */
typedef struct pgx_batch pgx_batch; /* one device-resident read batch and its results */

typedef struct {
    uint64_t bwt_size;      /* FastLocate::bwt_size(), r-index.hpp:568 */
    uint64_t sigma;         /* C.size() */
    uint64_t n_sequences;   /* FastLocate::tot_strings(), r-index.hpp:484 */
    uint64_t n_ref_blocks;  /* blocks in the file (10 runs each, r-index.hpp:312) */
    uint64_t n_runs;        /* logical BWT runs held by the image */
    uint64_t n_dev_blocks;  /* 64-byte device rank blocks */
    uint64_t dir_entries;   /* directory entries (u64) */
    uint32_t dir_shift;
    uint32_t is_encoded;    /* FastLocate::is_encoded(), r-index.hpp:409 */
    uint32_t has_N;         /* encoded_has_N */
    uint32_t mode;
    uint32_t has_tags;
    uint32_t tag_format;
    uint64_t n_tag_runs;    /* ones in bwt_intervals */
    uint64_t tag_dir_entries;
    uint32_t tag_dir_shift;
    uint32_t image_in_lds;  /* 1 when the rank image fits the per-workgroup LDS budget */
    uint64_t image_bytes;   /* device bytes of the rank image (blocks + directory + block lows) */
    uint64_t tag_image_bytes;
    double ref_block_mean_bytes; /* mean encoded block size of the reference layout (B_blk) */
    uint64_t max_length;    /* Header::max_length: packed position = seq * max_length + offset (r-index.hpp:424) */
    uint64_t n_samples;     /* samples.size() = runs in the reference's numbering */
    uint32_t image_kind;    /* 0 = run-length blocks + directory, 1 = dense bit planes (64 symbols per 64-byte block),
                             * 2 = dense2 (384 symbols per 128-byte block, two planes + exception runs) */
    uint32_t image_pairs;   /* 1 = a PAIRS image (two extensions per cache line) accompanies the dense / dense2 image */
    uint32_t image_wide;    /* 1 = the 64-bit form of dense2 / PAIRS (BWTs of 2^32 symbols or more, or PGX_MODE_IMAGE_WIDE) */
    uint32_t pairs_stride;  /* positions between the starts of consecutive blocks of the PAIRS image (each covers 96): 96, or 64 = overlapping blocks; 0 without one */
} pgx_index_info;

const char *pgx_last_error(void);
int pgx_abi_version(void);

/* ---- index lifetime ---------------------------------------------------------------------- */
/* Replaces FastLocate::load_encoded (src/r-index.cpp:406-459, legacy fall-back :378-404) and
 * TagArray::load_compressed_tags{,_sdsl} (src/tag_arrays.cpp:739-776).  tags_path may be NULL.
 * Host-only: parses the files and builds the flat device image in host memory. */
pgx_status pgx_index_open(const char *ri_path, const char *tags_path, uint32_t tags_format,
                          uint32_t mode, pgx_index **out);
/* Same from memory images of the files (what std::istream-based loaders hand over).  Either image
 * may be NULL: a tags-only handle serves TagArray, an r-index-only handle serves FastLocate. */
pgx_status pgx_index_open_memory(const void *ri_bytes, uint64_t ri_n, const void *tags_bytes, uint64_t tags_n,
                                 uint32_t tags_format, uint32_t mode, pgx_index **out);
/* FastLocate's public tables: sym_map (r-index.hpp:307), C (:310), complement_table (:347) */
pgx_status pgx_index_tables(const pgx_index *h, uint8_t sym_map[256], uint64_t C[8], uint8_t complement[256]);
pgx_status pgx_index_info_get(const pgx_index *h, pgx_index_info *info);
/* Frees the host image and every device image.  Batches created from the index use its device images: free them first. */
void pgx_index_close(pgx_index *h);

/* Copy the image to a HIP device (idempotent per device). */
pgx_status pgx_index_to_device(pgx_index *h, int device);

/* Host views of the flat image (for tests that verify the layout without a GPU, and FastLocate::getSample).  `which`:
 * 0 rank blocks (64 B each), 1 directory (u64), 2 block starts (u64, host only), 3 tag run starts (u64),
 * 4 tag values (u64), 5 tag directory (u32), 6 constants table (PgxConsts, pgx_image.h), 7 block lows (u16);
 * locate image (built on first use of one of these selectors, pgx_image.h "locate image"):
 * 8 rstart (u64, first BWT position of every run + n), 9 rsamp (u64, samples[run]: what getSample returns),
 * 10 rdir (u32), 11 lpos (u64, ones of `last`), 12 lnext (u64, samples[last_to_run[i] + 1]), 13 ldir (u32),
 * 14 locate constants (PgxLocConsts); 15 exception runs of the dense2 rank image (u32);
 * literal count image of an encoded index without N: 16 block starts (u64), 17 six cumulative counts per
 * block (u64), 18 runs as the reference's late scan sees them (u64: code << 56 | length), 19 first run of every block (u32);
 * two-step PAIRS image (pgx_image.h; empty without one): 20 blocks (32 dwords each);
 * WIDE images: 22 superblock bases of the dense2 image (8 u64 each), 23 of the PAIRS image (24 u64 each). */
pgx_status pgx_index_image_view(const pgx_index *h, int which, const void **ptr, uint64_t *bytes);

/* The DEVICE copy of a view (tests: what the kernels read must be what the host built): which = 0 (rank blocks), 15 (exception runs),
 * 20 (PAIRS blocks), 22 / 23 (superblock bases); copies min(bytes, size of the view) bytes into out.
 * 30 .. 33: the LCE image, which exists on the device only (pgx_image.h; built by this call if it has not been): suffix array in text
 * coordinates (u32 x n), text at two bits per symbol, flag bits per 128-byte text line, common prefixes of neighbouring suffixes (u8 x n);
 * nothing is copied where the index has no such image. */
pgx_status pgx_index_device_view(pgx_index *h, int device, int which, void *out, uint64_t bytes);

/* ---- image file (.pgi): the built host images of an index, saved once and reopened without a .ri or a tag file ------------
 * pgx_index_open parses the reference's files (Elias-Fano vectors, ByteCode blocks) and builds the flat images on host threads on every
 * start; the reference's loaders (FastLocate::load_encoded src/r-index.cpp:406-459, TagArray::load_compressed_tags_sdsl
 * src/tag_arrays.cpp:766-776) pay the same on every start.  An image file holds what that work produced, so opening it is reading it.
 *
 * This is an INTEGRITY check against truncation, bit rot and files of another build.  It is NOT a defence against a crafted file: a
 * file whose sums and lengths are consistent is trusted, and the kernels index its sections unchecked.
 *
 * THE FILE (little-endian, versioned; no time stamp, no host name: the same index saved twice gives the same bytes).
 *   header, 64 bytes
 *      0  char[8]  magic "PGXIMAGE"
 *      8  u32      file-format version (PGX_IMAGE_FILE_VERSION)
 *     12  u32      PGX_IMAGE_LAYOUT (pgx_image.h)
 *     16  u32      sizeof(PgxConsts)        20  u32  sizeof(PgxLocConsts)
 *     24  u32      mode (PGX_MODE_COMPAT / PGX_MODE_STRICT)
 *     28  u32      has_rank                 32  u32  has_tags
 *     36  u32      number of sections S (1 .. PGX_IMAGE_MAX_SECTIONS)
 *     40  u32      bytes of the meta record (PGX_IMAGE_META_BYTES)
 *     44  u32      flags: bit 0 the locate image is stored, bit 1 the literal count image is stored
 *     48  u64      header sum: the section sum (below) of bytes [0, 64 + 32 S + meta bytes) with this field read as zero
 *     56  u64      0
 *   section table at 64, 32 bytes per entry, in ascending id order
 *      0  u32 id (PGX_IMAGE_SEC_*)   4  u32 element size   8  u64 bytes   16  u64 file offset (a multiple of 4096)   24  u64 section sum
 *   meta record behind the table: what a handle keeps of the .ri and the tag file once the images exist
 *      0  u8[256] sym_map     256  u64[8] C     320  u32 sigma (C.size())   324  u32 encoded   328  u32 hasN   332  u32 tags.format
 *    336  u64 sequence_size   344  u64 max_length   352  u64 n_file_blocks   360  f64 ref_block_mean_bytes   368  u64 samples.size()
 *    376  u64[6] symbol totals of the BWT in nuc order (\n A C G N T)
 *    424  u64 tag values stored (tvals)   432  u64 exception runs stored (exc)   440  u64 blocks / 448  u64 runs of the literal count image
 *         (the four array lengths no constant states: with them every section's length is implied exactly)
 *   sections, each at its offset, in id order, zero bytes between them; the file ends with the last section.  An empty section still
 *   has an entry (bytes 0, offset = where it would start).
 * SECTION SUM.  The section is read as 8-byte little-endian words w[0 .. ceil(bytes / 8)), the last one padded with zero bytes;
 *   sum = sum over i of mix(w[i] + (i + 1) * 0x9E3779B97F4A7C15)   (all arithmetic modulo 2^64), with
 *   mix(z):  z = (z ^ (z >> 32)) * 0xD6E8FEB86659FD93;  z ^ (z >> 32)       (xor-shift, odd multiplier, xor-shift: each step a bijection;
 *   one multiplication per word keeps the device kernel bound by memory, not by its 64-bit multiplies)
 *   For a fixed i the term is a bijection of w[i], so one changed word always changes the sum; the index enters every term, so equal
 *   words at different places give different terms; addition commutes, so threads and lanes may add in any order and the result is
 *   bitwise reproducible.  The sum of no bytes is 0.  (tests/image_file_emu.py restates the file and the sum in Python.) */
#define PGX_IMAGE_MAGIC "PGXIMAGE"
#define PGX_IMAGE_FILE_VERSION 1u
#define PGX_IMAGE_MAX_SECTIONS 64u
#define PGX_IMAGE_HEADER_BYTES 64u
#define PGX_IMAGE_ENTRY_BYTES 32u
#define PGX_IMAGE_META_BYTES 456u
#define PGX_IMAGE_ALIGN 4096u
#define PGX_IMAGE_HAS_LOCATE 1u  /* header flags */
#define PGX_IMAGE_HAS_LITERAL 2u
/* section ids; the names pgx_image_section_name gives are the lower-case suffixes (consts, blocks, .. loc_consts, rstart, .. lit_bstart, ..) */
#define PGX_IMAGE_SEC_CONSTS 1u  /* PgxConsts */
#define PGX_IMAGE_SEC_BLOCKS 2u  /* views 0, 1, 2, 7, 15, 20, 22, 23, 3, 4, 5 of pgx_index_image_view, in this order: */
#define PGX_IMAGE_SEC_DIR 3u
#define PGX_IMAGE_SEC_BSTART 4u
#define PGX_IMAGE_SEC_BLOW 5u
#define PGX_IMAGE_SEC_EXC 6u
#define PGX_IMAGE_SEC_PAIRS 7u
#define PGX_IMAGE_SEC_SBASE2 8u
#define PGX_IMAGE_SEC_PBASE 9u
#define PGX_IMAGE_SEC_TSTART 10u
#define PGX_IMAGE_SEC_TVALS 11u
#define PGX_IMAGE_SEC_TDIR 12u
#define PGX_IMAGE_SEC_N_RUNS 13u /* u64: logical BWT runs (pgx_index_info.n_runs) */
#define PGX_IMAGE_SEC_LOC_CONSTS 20u /* PgxLocConsts; views 14, 8 .. 13 */
#define PGX_IMAGE_SEC_RSTART 21u
#define PGX_IMAGE_SEC_RSAMP 22u
#define PGX_IMAGE_SEC_RDIR 23u
#define PGX_IMAGE_SEC_LPOS 24u
#define PGX_IMAGE_SEC_LNEXT 25u
#define PGX_IMAGE_SEC_LDIR 26u
#define PGX_IMAGE_SEC_LIT_BSTART 30u /* views 16 .. 19 */
#define PGX_IMAGE_SEC_LIT_CUM 31u
#define PGX_IMAGE_SEC_LIT_RUNS 32u
#define PGX_IMAGE_SEC_LIT_ROFF 33u
#define PGX_IMAGE_SEC_LIT_TABS 34u   /* u32 code_of[256], u32 cslot_of[256], u64 C[8] */
/* What is stored: the rank image with its tag runs (always), the locate image of a handle with an r-index (unless
 * PGX_IMAGE_NO_LOCATE), the literal count image exactly where pgx_count_batch goes through it (COMPAT, encoded, no N).  What exists
 * on the device only (seed tables, tag pairs and buckets, the LCE image) is rebuilt there as for any handle. */
#define PGX_IMAGE_NO_LOCATE 1u /* pgx_index_save_image: leave the locate image out */
#define PGX_IMAGE_VERIFY 1u    /* pgx_index_open_image: also sum every section on the host before returning */
typedef struct {
    uint32_t id, elem_size;
    uint64_t bytes, offset, sum;
    char name[16];
} pgx_image_section_info;
typedef struct {
    uint32_t version, layout, consts_bytes, loc_consts_bytes, mode, has_rank, has_tags, n_sections, meta_bytes, flags;
    uint64_t header_sum, file_bytes;
    pgx_image_section_info sections[PGX_IMAGE_MAX_SECTIONS];
} pgx_image_info; /* (not pgx_image_file_info: C keeps functions and typedef names in one name space) */
/* Host only.  Builds the locate image and the literal image of `h` if they are not built yet, writes the file under a temporary name
 * next to `path` and renames it; no file is left behind after an error (PGX_ERR_IO).  Works from an image-opened handle too (the same
 * bytes again).  PGX_IMAGE_NO_LOCATE from a handle that has no locate image is what it already is; without the flag such a handle
 * is PGX_ERR_UNSUPPORTED.  PGX_ERR_ARG for unknown flags. */
pgx_status pgx_index_save_image(pgx_index *h, const char *path, uint32_t flags);
/* Host only.  Checks, in this order: the magic (PGX_ERR_FORMAT: not an image file); version, layout id and struct sizes
 * (PGX_ERR_UNSUPPORTED: written by another build, make it again); the header sum; every section's entry -- id, element size, length
 * against what the constants imply, offset and length against the file size, in overflow-safe arithmetic -- (PGX_ERR_FORMAT naming the
 * section).  Then reads every section straight into its final buffer.  Nothing is allocated by a length that has not passed these checks.
 * Without PGX_IMAGE_VERIFY the section sums are not computed on the host: the device computes them at memory speed when a section is
 * uploaded, before any other kernel reads it (pgx_index_to_device and the first locate / literal call return PGX_ERR_FORMAT naming the
 * section, release that device image whole, and answer the same on the next call).  The handle answers pgx_index_image_view,
 * pgx_index_device_view, pgx_index_info_get and pgx_index_tables as the handle it was saved from.  From an image without the locate
 * image the locate entry points and views 8 .. 14 are PGX_ERR_UNSUPPORTED and find_mems runs without the LCE image. */
pgx_status pgx_index_open_image(const char *path, uint32_t flags, pgx_index **out);
/* Host only: the header and the section table of a file, after the same checks of the header (not of the sections); nothing is loaded. */
pgx_status pgx_image_file_info(const char *path, pgx_image_info *out);
/* The section sum of n bytes.  device >= 0: `bytes` is host memory, uploaded to that device and summed there by pgx_image_sum_kernel
 * (16-byte loads, grid-stride, 64-bit word indices); device < 0: on host threads.  The two agree bit for bit. */
pgx_status pgx_image_sum(int device, const void *bytes, uint64_t n, uint64_t *sum);
const char *pgx_image_section_name(uint32_t id); /* "?" for an unknown id */

/* ---- index construction (build side, run once; on the CPU, or with the suffix sorting on a device: pgx_build_index_from_text[s]_device) --- */
/* Replaces build_rindex (src/build_rindex.cpp:13-21 -> FastLocate(std::string) src/r-index.cpp:778
 * + serialize_encoded :297-376).  encoded=0 writes the legacy layout (serialize, :266-294). */
pgx_status pgx_build_rindex(const char *rlbwt_path, const char *out_ri_path, int encoded);
/* BWT of a newline-terminated sequence collection (what grlBWT produces for the reference):
 * writes the grlBWT .rl_bwt layout read by bwt_buff_reader. */
pgx_status pgx_build_rlbwt(const char *text_path, const char *out_rlbwt_path);
/* Both steps in one call (out_rlbwt_path may be NULL): the suffix array the BWT is made from also yields the SA samples
 * directly, so the sampling walk of FastLocate(std::string) (src/r-index.cpp:993-1130) is not repeated; the .ri written
 * is byte-identical to pgx_build_rlbwt + pgx_build_rindex. */
pgx_status pgx_build_index_from_text(const char *text_path, const char *out_rlbwt_path, const char *out_ri_path, int encoded);
/* The same for a collection handed over as several texts ("chromosomes"; their sequences in the order of the texts): one suffix array
 * per text, built side by side, then a k-way merge of the sorted suffix lists split over host threads.  The files are byte-identical
 * to what the single call writes for the concatenation; every text must stay below 2^31 symbols, the collection may have any size
 * (the reference takes grlBWT's output of any size: FastLocate(std::string), src/r-index.cpp:778-1139). */
pgx_status pgx_build_index_from_texts(const char *const *text_paths, uint32_t n_texts, const char *out_rlbwt_path, const char *out_ri_path, int encoded);
/* pgx_build_index_from_text / _texts with the suffix sorting, the BWT and its runs computed on `device` (prefix doubling over a hand-written
 * LSD radix sort, pgx_build_sa_kernels.hip); the host writes the two files from the runs and the suffixes at their borders, with the writers of
 * the CPU calls.  The files are byte-identical to what the CPU calls write for the same input.  No CPU fallback.
 *   Input     the rules of the CPU calls: a text that does not end in '\n' gets one; an empty file is PGX_ERR_FORMAT; several texts are their
 *             concatenation in argument order (their sequences in that order).  The device sorts the whole collection at once, so the _texts
 *             call needs no merge: it exists so that per-chromosome texts need not be concatenated on disk.
 *   Order     symbols compare by byte value ('\n' < A < C < G < N < T), two endmarkers by sequence number; the symbol before text position 0
 *             is '\n'.
 *   Alphabet  exactly '\n' A C G N T.  Any other byte: PGX_ERR_UNSUPPORTED naming the byte and its offset, before any file is written (the CPU
 *             calls fail on such a text too, at their .ri stage: "BWT symbol outside {\n,A,C,G,N,T}").
 *   Size      fewer than 2^32 - 2^20 symbols in total (text positions and ranks are uint32_t; twice what one text of the CPU calls may
 *             hold).  Beyond: PGX_ERR_UNSUPPORTED naming pgx_build_index_from_texts, decided from the file sizes (and the last byte of each
 *             text: one that lacks its newline counts one more) before any text is read or anything is allocated.
 *   Memory    the device bytes are computed from the file sizes before the first allocation (about 35 bytes a symbol; the formula is in
 *             DESIGN.md) and compared with the free device memory, or with PGX_BUILD_DEVICE_BUDGET_MB (environment, read per call, fractions
 *             allowed) in its place: PGX_ERR_NOMEM with both numbers.  There is no chunked mode.
 *   Rounds    at most 40 doubling rounds; PGX_ERR_HIP "suffix sort did not converge" after that (no text below the size bound needs more than 29).
 *   Files     written under temporary names (unique per call) and renamed when both are complete, the .ri first: no output file exists after any error.  out_rlbwt_path
 *             may be NULL.  PGX_ERR_IO when a text cannot be read or a file cannot be created.
 *   PGX_ERR_ARG for null paths or n_texts == 0, PGX_ERR_NO_DEVICE without a GPU.  One stream; a roctx range pgx_build_index_device with
 *   PGX_ROCTX=1; PGX_BUILD_TIMING=1 adds one line on stderr (sizes, device bytes, HIP-event time of the radix passes). */
pgx_status pgx_build_index_from_text_device(const char *text_path, const char *out_rlbwt_path, const char *out_ri_path, int encoded, int device);
pgx_status pgx_build_index_from_texts_device(const char *const *text_paths, uint32_t n_texts, const char *out_rlbwt_path, const char *out_ri_path, int encoded, int device);
/* stage times (ms) of this thread's last call, as pgx_build_tags_timing:
 * [0] read + upload  [1] sequence table + first sort  [2] doubling rounds  [3] BWT, runs, samples + download
 * [4] .rl_bwt / .ri written on the host  [5] number of doubling rounds (a count, not a time) */
pgx_status pgx_build_index_device_timing(double *ms, uint32_t n);
/* Write a compact sdsl tag file (format 3, src/tag_arrays.cpp:940-974 + :622-654) from parallel
 * arrays of run values (already `offset | rev<<10 | node<<11`) and run lengths. */
pgx_status pgx_write_compact_tags(const char *out_path, const uint64_t *values,
                                  const uint64_t *lengths, uint64_t n_runs);

/* convert_tags equivalent (src/convert_tags.cpp): build_tags' "algorithm format" -> a query format.
 * compact = 0: ByteCode format (load_compressed_tags, tag_arrays.cpp:739); 1: sdsl-compact (find_mems.cpp:79). */
pgx_status pgx_convert_tags(const char *in_path, const char *out_path, int compact);

/* The query-format tag file of a run list, encoded on `device`: the bytes pgx_write_compact_tags (format = PGX_TAGS_COMPACT) or
 * pgx_convert_tags(.., compact = 0) (format = PGX_TAGS_BYTECODE) write for the same runs.  values[i] = offset | rev << 10 |
 * node << 11; lengths[i] may be 0 (writes nothing) and may exceed 511 (pieces of 511, then the rest: while (len >= 512) emit 511).
 * max_node_floor as in merge_tags (the item width covers at least this node id; compact only).  The ByteCode form is what
 * pgx_convert_tags makes of the build_tags file of these runs, so it opens, like the reference's own files, with the runs that
 * convert_tags reads out of that file's 8-byte header; the compact form holds the stated runs only.  Pieces, Elias-Fano parts and select
 * tables are computed by HIP kernels, one thread per output word; the whole file is assembled in device memory, downloaded once and
 * written once, after every check: an error leaves no file.  PGX_ERR_ARG for a null path or array and for any other format
 * (PGX_TAGS_AUTO included), checked before the device is touched; PGX_ERR_FORMAT for a node id beyond 2^53 - 1 (compact: the item
 * has 64 bits) or 2^44 - 1 (ByteCode). */
pgx_status pgx_tags_encode(int device, const uint64_t *values, const uint64_t *lengths, uint64_t n_runs, uint64_t max_node_floor,
                           uint32_t format, const char *out_path);
/* stage times (ms) of this thread's last encoding (pgx_tags_encode, or pgx_build_tags / pgx_merge_tags with their device-encode
 * flags), up to n of: [0] pieces + items or ByteCodes [1] the two sd_vector bodies [2] select supports [3] download [4] file write
 * [5] bytes of the file and [6] peak device bytes of the encoder's own buffers (counts, not times) */
pgx_status pgx_tags_encode_timing(double *ms, uint32_t n);

/* merge_tags equivalent (src/merge_tags.cpp): per-chromosome tag streams (build_tags' "algorithm format": ByteCode runs
 * offset:10 | rev:1 | len:9 | node<<20, with or without the 8-byte int_vector<8> header of sdsl::int_vector_buffer) ->
 * the whole-genome tag array in the sdsl-compact query format find_mems loads.  `ri_path` is the whole-genome r-index;
 * seq_to_file[s] (n_seq = tot_strings entries) names the tag file of sequence s -- the reference derives this from the
 * GBZ (first node of path s -> weakly connected component -> the file whose first tag lies in that component,
 * merge_tags.cpp:478-512); a GBZ reader is out of scope here, so the caller states it.  Runs on `device`: document
 * array by the locate kernels, one scan + gather per file, run-length encoding.  Merged runs are maximal (the reference
 * counts them in a uint16_t, which wraps beyond 65 535) and split at 511 like append_compact_run_streamed
 * (src/tag_arrays.cpp:940-974).  PGX_ERR_FORMAT when a file holds a different number of tags than the BWT has
 * positions of its sequences; a file that cannot be read is reported the same way, with its path.  PGX_ERR_ARG for
 * n_files outside 1..250 and for any seq_to_file entry >= n_files, that of an empty sequence included.  A refused call
 * writes nothing at out_path. */
pgx_status pgx_merge_tags(const char *ri_path, const char *const *tag_paths, uint32_t n_files, const uint32_t *seq_to_file,
                          uint64_t n_seq, int device, const char *out_path);
/* As pgx_merge_tags, with flags.  PGX_MERGE_REFERENCE_RUNS: the file byte for byte as the reference writes it.  The reference
 * collects runs job by job (500 BWT runs each, src/merge_tags.cpp:600,733-823) in std::pair<pos_t, uint16_t> and joins the last
 * run of one job to the first of the next when the tags are equal (:776-777, previous_last_run), so what it hands to
 * append_compact_run_streamed is every MAXIMAL run with its length taken mod 65 536 -- a length that lands on 0 writes nothing
 * (src/tag_arrays.cpp:959) and the positions of every later run shift down.  Without the flag (and in pgx_merge_tags) lengths are
 * exact; the two outputs are the same bytes whenever no merged run reaches 65 536 positions (tests/test_merge_tags.py restates
 * the reference's job loop and checks that rule). */
#define PGX_MERGE_REFERENCE_RUNS 0x1u
/* PGX_MERGE_DEVICE_ENCODE: the output file is encoded on the device from the merged runs where they lie (as pgx_tags_encode) instead
 * of downloading them to the host writer; lengths, the mod-65 536 rule of PGX_MERGE_REFERENCE_RUNS included, come from a kernel.
 * The same bytes either way.  (The value leaves 2, 4 and 8 unassigned.) */
#define PGX_MERGE_DEVICE_ENCODE 0x10u
pgx_status pgx_merge_tags_ex(const char *ri_path, const char *const *tag_paths, uint32_t n_files, const uint32_t *seq_to_file,
                             uint64_t n_seq, int device, const char *out_path, uint32_t flags);

/* What merge_tags asks the graph (src/merge_tags.cpp:443-445,478-515; include/pangenome_index/algorithm.hpp:600-619): for every
 * GBWT sequence of the GBZ the graph node id of its first node (gbz.index.extract(i)[0]; 0 for an empty path) and that node's
 * weakly connected component (numbered by smallest node id), plus the graph's largest node id and component count.  Reads only
 * the GBWT's node records of the file (simple-sds layout).  first_node / component may be NULL; at most cap entries are written. */
pgx_status pgx_gbz_paths(const char *gbz_path, uint64_t *n_sequences, uint64_t *first_node, uint32_t *component, uint64_t cap,
                         uint64_t *max_node_id, uint32_t *n_components);
/* merge_tags with the reference's own inputs: graph.gbz, whole-genome r-index, per-chromosome tag files.  Sequence s belongs
 * to the tag file whose first tag lies in the component of the first node of path s (merge_tags.cpp:478-515); the item width
 * of the output comes from the graph's largest node id (:627-638).  Otherwise as pgx_merge_tags. */
pgx_status pgx_merge_tags_gbz(const char *gbz_path, const char *ri_path, const char *const *tag_paths, uint32_t n_files, int device,
                              const char *out_path);
pgx_status pgx_merge_tags_gbz_ex(const char *gbz_path, const char *ri_path, const char *const *tag_paths, uint32_t n_files, int device,
                                 const char *out_path, uint32_t flags); /* flags as pgx_merge_tags_ex */

/* build_tags equivalent (src/build_tags.cpp): graph + BWT -> tag array in the "algorithm format" merge_tags and convert_tags
 * read (int_vector<8> header holding the body length in bits; body = gbwt ByteCodes of offset:10 | rev:1 | len:9 | node << 20,
 * one per run piece of at most 511 rows; zero padding to 8 bytes).  The tag of BWT row i >= n_seq is Position::encode of text
 * position SA[i] = (sequence s, offset off): node_id << 11 | rev << 10 | offset within the oriented node of path s that
 * covers off; the endmarker rows [0, n_seq) have none.  Equal neighbouring tags form maximal runs.
 *
 * Not the reference's method (unique k-mers, a B+-tree, a BFS and one psi walk per sequence): the suffix array of the whole
 * BWT on `device` (the locate kernels), then one lookup per row and a run-length encoding, all HIP kernels; no CPU fallback.
 * Index sequence s is path s of the graph (GBWT sequence s), or GBWT sequence 2s with PGX_BUILD_TAGS_FORWARD_ONLY (a text of
 * one orientation per path, e.g. gbz_extract without -b).  PGX_ERR_FORMAT names the first offending sequence when the
 * index's sequence count differs from the number of paths used, a path's length differs from its sequence's length in the
 * index, a path visits a node without a sequence or one longer than 1024 bp (the offset field has 10 bits).  No output file
 * is left behind after an error. */
#define PGX_BUILD_TAGS_REFERENCE_RUNS 0x1u /* run lengths mod 65 536 as the reference's uint16_t counter leaves them
                                              (algorithm.hpp traverse_sequences_parallel); a run that becomes 0 is dropped.
                                              Without it lengths are exact; the bytes agree whenever no run reaches 65 536 */
#define PGX_BUILD_TAGS_FORWARD_ONLY 0x2u   /* index sequence s = GBWT sequence 2s; pgx_gbz_extract: even sequences only */
#define PGX_BUILD_TAGS_INPUT_RLBWT 0x4u    /* ri_path names a grlBWT .rl_bwt; its r-index is built in memory */
#define PGX_BUILD_TAGS_OUT_COMPACT 0x8u    /* out_path receives the sdsl-compact query format find_mems loads: byte for byte what
                                              pgx_convert_tags(compact = 1) makes of the file the same call writes without the
                                              flag.  Encoded on the device from the runs (as pgx_tags_encode); the algorithm-format
                                              body is neither encoded nor downloaded */
#define PGX_BUILD_TAGS_OUT_BYTECODE 0x10u  /* likewise the ByteCode query format (pgx_convert_tags(compact = 0)); both: PGX_ERR_ARG */
pgx_status pgx_build_tags(const char *gbz_path, const char *ri_path, int device, const char *out_path, uint32_t flags);
/* pgx_build_tags with the graph stated by the caller: n_seq paths, path s = path_nodes[path_offsets[s], path_offsets[s + 1])
 * with nodes as id << 1 | rev; node_length[id - first_node_id] for n_node_ids ids (0: the id has no sequence).  first_node_id is
 * any value; an id below it or from first_node_id + n_node_ids on has no sequence either.  A path of no nodes (path_offsets[s] ==
 * path_offsets[s + 1], also at the end of path_nodes) is the empty sequence; path_nodes may be NULL when no path has a node.  A path may
 * visit a node any number of times and paths may share nodes.  A run piece holds node << 20 in 64 bits: a path that visits an id of
 * 2^44 or more is PGX_ERR_FORMAT naming the id, like the other errors before any device work on the tags and without an output file. */
pgx_status pgx_build_tags_paths(const char *ri_path, uint64_t n_seq, const uint64_t *path_offsets, const uint64_t *path_nodes,
                                const uint32_t *node_length, uint64_t first_node_id, uint64_t n_node_ids, int device,
                                const char *out_path, uint32_t flags);
/* stage times (ms) of this thread's last pgx_build_tags[_paths] call, up to n of: [0] graph (GBZ parse + path extraction; 0 for
 * _paths) [1] index (read or built, locate image upload) [2] suffix array [3] tag of every row incl. the length checks [4] run
 * encoding incl. the body download [5] file write.  With an OUT flag [4] ends with the run compaction and [5] is the whole device
 * encoding, download and write included (its stages: pgx_tags_encode_timing) */
pgx_status pgx_build_tags_timing(double *ms, uint32_t n);
/* gbz_extract: the newline-separated text of every GBWT sequence of the graph spelled from its node sequences (reverse
 * complemented where the orientation bit is set), or of the even ones with PGX_BUILD_TAGS_FORWARD_ONLY. */
pgx_status pgx_gbz_extract(const char *gbz_path, const char *out_text_path, uint32_t flags);

/* ---- primitives (tests; mirror the public FastLocate / TagArray query API) ----------------- */
/* FastLocate::rank_at_cached_encoded (src/r-index.cpp:619-641): out[i*6 .. i*6+sigma) per position;
 * entries >= sigma are zero.  true_codes!=0 returns the six true code ranks instead. */
pgx_status pgx_rank_batch(pgx_index *h, int device, const uint64_t *pos, uint64_t n,
                          int true_codes, uint64_t *out);
/* FastLocate::backward_extend_encoded / forward_extend_encoded (src/r-index.cpp:713-764) */
pgx_status pgx_extend_batch(pgx_index *h, int device, const pgx_biint *in, const uint8_t *sym,
                            const uint8_t *forward, uint64_t n, pgx_biint *out);
/* TagArray::query_compressed{,_compact} (src/tag_arrays.cpp:780-890) without the printing.
 * Two-call pattern: positions==NULL returns counts only.  pos_offsets has n+1 entries. */
pgx_status pgx_tag_query_batch(pgx_index *h, int device, const uint64_t *start, const uint64_t *end,
                               uint64_t n, uint64_t *run_nums, uint64_t *pos_offsets,
                               uint64_t *positions, uint64_t positions_cap, uint64_t *n_overflow);

/* FastLocate::count / count_encoded (include/pangenome_index/r-index.hpp:540-556): backward search of
 * every read; out[i] = final BWT range, {1, 0} when empty (the query_tags path, src/query_tags.cpp:88-96).
 * In COMPAT mode on an encoded index without N the reference's rankAt_encoded mis-parses every block (it always reads
 * six cumulative varints, src/r-index.cpp:578: SURVEY 8a quirk 3); that wrong-but-deterministic result is reproduced
 * (a separate image of the reference's blocks as its scan sees them); PGX_MODE_STRICT gives the true ranges. */
typedef struct {
    uint64_t first;
    uint64_t second;
} pgx_range;
pgx_status pgx_count_batch(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads,
                           pgx_range *out);

/* One step of it -- FastLocate::LF (src/r-index.cpp:650-687) / LF_encoded (:689-711): out[i] = LF(in[i], sym[i]) for n
 * inclusive ranges; empty inputs and results are {1, 0}.  Same COMPAT restriction as pgx_count_batch. */
pgx_status pgx_lf_batch(pgx_index *h, int device, const pgx_range *in, const uint8_t *sym, uint64_t n, pgx_range *out);

/* ---- locate: suffix-array samples of the r-index ---------------------------------------- */
#define PGX_NO_POSITION (~(uint64_t)0)
#define PGX_LOCATE_SEQ_IDS 1u /* values are seqId(v) = v / max_length (r-index.hpp:429) instead of packed positions */
#define PGX_LOCATE_UNIQUE 2u  /* every query's values sorted and de-duplicated (src/r-index.cpp:1293-1294)            */
/* FastLocate::locate / locate_encoded (src/r-index.cpp:1252-1341) for n BWT ranges [first[i], last[i]] (inclusive;
 * last < first is the empty state).  flags = PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE is the reference's result
 * (sorted unique sequence ids); flags = 0 gives the packed suffix-array values pack(seq, offset) in BWT order.
 * val_offsets has n + 1 entries.  values == NULL returns the offsets only; otherwise values_cap must hold the
 * result (sum of last - first + 1 always suffices).  Ranges must end before bwt_size (PGX_ERR_ARG otherwise).
 * PGX_ERR_UNSUPPORTED in COMPAT mode on an encoded index without N: the reference's run scan skips six header
 * varints where five were written (EncodedBlock::skip_header, src/r-index.cpp:83-88). */
pgx_status pgx_locate_batch(pgx_index *h, int device, const uint64_t *first, const uint64_t *last, uint64_t n,
                            uint32_t flags, uint64_t *val_offsets, uint64_t *values, uint64_t values_cap);
/* FastLocate::locateNext (src/r-index.cpp:1363-1366) for n packed positions; PGX_NO_POSITION where the reference's
 * result is undefined (no tail sample at or before prev, or the tail of the last run). */
pgx_status pgx_locate_next_batch(pgx_index *h, int device, const uint64_t *prev, uint64_t n, uint64_t *out);
/* FastLocate::decompressSA (flags = 0) / decompressDA (flags = PGX_LOCATE_SEQ_IDS), src/r-index.cpp:1343-1361:
 * out has bwt_size entries.  Every BWT run is an independent chain from its head sample. */
pgx_status pgx_decompress_sa(pgx_index *h, int device, uint32_t flags, uint64_t *out);

/* ---- the hot path: find_mems over a batch of reads ----------------------------------------- */
#define PGX_RUN_TAGS 1u    /* also run the tag queries of find_mems.cpp:129 */
#define PGX_RUN_TIMING 2u  /* record HIP events around each kernel (pgx_batch_timing)           */

typedef struct {
    uint64_t n_reads;
    uint64_t n_mems;
    const uint64_t *mem_offsets;    /* n_reads+1; MEMs of read i = mems[mem_offsets[i] .. [i+1])   */
    const pgx_mem *mems;            /* discovery order (find_all_mems, algorithm.hpp:739-757)     */
    const uint64_t *tag_run_counts; /* per MEM: number_of_runs (tag_arrays.cpp:860); NULL w/o tags */
    const uint64_t *pos_offsets;    /* n_mems+1; NULL w/o tags                                    */
    const uint64_t *positions;      /* sorted unique graph positions per MEM (tag_arrays.cpp:882) */
    uint64_t n_positions;
    uint64_t n_extensions;          /* backward+forward extensions performed (counter)           */
    uint64_t n_tag_overflow;        /* tag queries that read past the stored runs (ref: UB)      */
} pgx_result;

typedef struct {
    float ms_find_mems;   /* the dominant kernel (pgx_find_mems_kernel) */
    float ms_compact;     /* MEM compaction + scans */
    float ms_tag_locate;
    float ms_tag_gather;
    float ms_tag_sort;
    float ms_total;       /* first launch -> last launch, device time */
    uint32_t find_mems_launches;
    uint32_t heavy_reads; /* reads whose rest went through the heavy-read kernel (filled by every run, timed or not) */
    uint32_t pairs_reads; /* != 0: the run used the two-step PAIRS kernel (2: with the reads packed in LDS; 3: and cooperative line fetches; 4: packed reads and the LCE image; `kernels` names the instance) */
    uint32_t pairs_other_steps; /* extensions the PAIRS kernel took through the image it accompanies: its own block held \n or N, or the interval was wider
                                 * than two blocks (until ABI 3's last revision: redo_reads, reads handed on to the dense2 kernel) */
    /* the first launch of the find_mems stage alone (the PAIRS kernel when pairs_reads, else pgx_find_mems_kernel): ms_find_mems
     * also covers the launches behind it (reads handed on, heavy reads) */
    float ms_find_mems_main;
    uint32_t seed_depth;  /* depth K of the k-mer seed table the run used (0 = none: no table, or min_len below every table's depth) */
    /* what the kernels asked of the memory system, counted by the kernels themselves (filled by every run, timed or not; zero for
     * images staged in LDS): 128-byte lines of the rank image fetched by rank probes -- trips whose line every lane shares (a
     * stage's first probe of the full interval) are not counted -- and seed / end table entries read (16 bytes, one line each) */
    uint64_t main_lines, main_seed_loads;   /* the launch ms_find_mems_main times */
    uint64_t other_lines, other_seed_loads; /* the other pgx_find_mems_kernel launches of the run */
    uint64_t two_step_trips;                /* PAIRS kernel: lane trips that performed two extensions from one line */
    /* Device time every FRESH batch pays before its first find_mems launch and a re-run of resident reads does not: with pgx_batch_upload the
     * pass that finds the chunks holding a byte outside A C G T and packs the reads to two bits per symbol, its read-back, the pass that lists
     * the reads concerned, and the scan of the worst-case MEM slots -- all inside the first pgx_batch_run after the upload (from its first
     * event to the first find_mems launch); with pgx_batch_upload_packed the unpack pass and the listed reads' bytes (inside the upload) plus
     * that scan.  0 for a run that found everything in place. */
    float ms_per_upload;
    /* which kernels of the find_mems stage the run launched (PGX_KERNELS_*; filled by every run, timed or not) */
    uint32_t kernels;
} pgx_timing;

/* pgx_timing.kernels.  pgx_find_mems_kernel is instantiated per (image staged in LDS, image kind, 32-bit interval state, seeded),
 * pgx_find_mems_pairs_kernel per (64-bit form, reads packed in LDS, cooperative line fetches, blocks every 64 positions, forward stages
 * through the LCE image); a run reports the instance of each it launched. */
#define PGX_KERNELS_FM 0x1u              /* pgx_find_mems_kernel was launched (over every read, or over the reads the pairs kernel skips); its instance: */
#define PGX_KERNELS_FM_SEEDED 0x2u
#define PGX_KERNELS_FM_NARROW 0x4u       /*   32-bit interval state */
#define PGX_KERNELS_FM_KIND_SHIFT 3      /*   two bits: 0 run-length image, 1 dense, 2 dense2, 3 dense2 in its 64-bit form */
#define PGX_KERNELS_FM_LDS 0x20u         /*   image staged in LDS */
#define PGX_KERNELS_FM_REDO 0x40u        /* a chunk was repeated with the 64-bit instance of the same kernel (PGX_KERNELS_FM_NARROW cleared) */
#define PGX_KERNELS_PAIRS 0x100u         /* pgx_find_mems_pairs_kernel was launched; its instance: */
#define PGX_KERNELS_PAIRS_S64 0x200u     /*   PAIRS blocks every 64 positions (else every 96) */
#define PGX_KERNELS_PAIRS_COOP 0x400u
#define PGX_KERNELS_PAIRS_PACKED 0x800u
#define PGX_KERNELS_PAIRS_WIDE 0x1000u
#define PGX_KERNELS_PAIRS_LCE 0x2000u
#define PGX_KERNELS_SIDE 0x10000u        /* the pgx_find_mems_kernel launch on the second stream, next to the pairs kernel */
#define PGX_KERNELS_HEAVY 0x20000u       /* pgx_find_mems_heavy_kernel was launched (pgx_timing.heavy_reads: over how many reads) */
#define PGX_KERNELS_FM_MASK 0x3Fu
#define PGX_KERNELS_PAIRS_MASK 0x3F00u
/* Every instance the runtime can launch, in the encoding above (PGX_KERNELS_FM | ... or PGX_KERNELS_PAIRS | ...): up to `cap` of them
 * into out (may be NULL), returns their number.  Host only. */
uint32_t pgx_kernel_variants(uint32_t *out, uint32_t cap);

/* Upload reads (read i = reads[offsets[i] .. offsets[i+1]); the `std::getline` lines of
 * find_mems.cpp:96-98, empty lines already skipped by the caller) to `device`. */
pgx_status pgx_batch_create(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets,
                            uint64_t n_reads, pgx_batch **out);
/* Pinned host memory for the read bytes handed to pgx_batch_create / pgx_batch_upload (and for anything else the caller streams to a
 * device): uploads from it run at the speed of the link, uploads from ordinary pageable memory are staged by the runtime at a fraction of
 * it (find_mems CLI, 16 M reads: 0.95 s of 1.9 s pipeline wall went into pageable uploads).  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_host_alloc(size_t bytes, void **out);
void pgx_host_free(void *p);
/* Replace the reads of an existing batch (its device and pinned host buffers only ever grow: a long-lived
 * batch costs no allocation per call).  Invalidates the results of the previous run. */
pgx_status pgx_batch_upload(pgx_batch *b, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads);
/* The same with the reads packed by the caller (the find_mems CLI's parse threads do it): a quarter of the bytes over the link, and no pass over
 * the read bytes on the device before the search.  `packed`: two bits per symbol, (byte >> 1) & 3 (A C T G = 0 1 2 3), symbol i of the
 * concatenation reads[offsets[0] ..) in bits 2 (i & 15) of word i >> 4, (offsets[n_reads] + 15) / 16 words; offsets[0] must be 0.  Reads that hold
 * any other byte are listed -- side_ids ascending, their bytes as they are concatenated in side_bytes in list order -- and what the packed words
 * say about them is ignored.  pgx_pack_reads produces all of it from a batch in the form pgx_batch_upload takes; results are the same bytes
 * either way (tests/test_gpu_parity.py).  Replaces the same per-read loop: src/find_mems.cpp:94-139. */
pgx_status pgx_batch_upload_packed(pgx_batch *b, const uint32_t *packed, const uint64_t *offsets, uint64_t n_reads, const uint64_t *side_ids,
                                   const uint8_t *side_bytes, uint64_t n_side);
/* Host side of it (no device needed): packs reads[offsets[0] .. offsets[n_reads]) into `packed` ((bytes + 15) / 16 words) on `threads` host
 * threads (0 = half the cores, at most 16) and lists the reads with a byte outside A C G T (upper case) with their bytes.  *n_side / *n_side_bytes
 * are always what the batch needs; PGX_ERR_NOMEM when that exceeds side_ids_cap / side_bytes_cap (upload such a batch as bytes). */
pgx_status pgx_pack_reads(const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads, uint32_t threads, uint32_t *packed, uint64_t *side_ids,
                          uint64_t side_ids_cap, uint8_t *side_bytes, uint64_t side_bytes_cap, uint64_t *n_side, uint64_t *n_side_bytes);
/* ---- reads as text, parsed on the device ----------------------------------------------------
 * Record rules (tests/fastx_emu.py states the same in Python).  A line is the text up to a '\n' (not included); a last line without
 * its newline counts; nothing follows a final newline.
 *   LINES  the find_mems contract (src/find_mems.cpp:94-98, std::getline): every non-empty line is a read, '\r' kept.
 *   FASTQ  strict 4-line records: '@' line, sequence, '+' line, quality.  A trailing '\r' is stripped from each line; the quality
 *          length must equal the sequence length; multi-line records and a text that ends inside a record are PGX_ERR_FORMAT.
 *   FASTA  a '>' line plus every following line up to the next '>' line; the sequence is those lines concatenated, a trailing '\r'
 *          stripped from each; blank lines add nothing; a non-blank line before the first '>' is PGX_ERR_FORMAT.
 * In FASTA and FASTQ every record is a read, one with an empty sequence included (it has no MEMs), so read i is the i-th record of
 * the text.  Sequence bytes pass as they are (lower case, N, IUPAC codes).  Error texts name the format, the record (1-based, as
 * find_mems numbers its "Seq:" lines) and the byte offset of the offending line in `text`. */
#define PGX_READS_LINES 0u /* the reference's contract: a line is a read, empty lines skipped, '\r' kept (std::getline) */
#define PGX_READS_FASTA 1u
#define PGX_READS_FASTQ 2u
/* Replace the reads of a batch with the records of `text` (whole records; the last may lack its final newline), parsed on the device.
 * *n_reads = records taken.  A refused upload (PGX_ERR_FORMAT / _ARG) leaves the batch exactly as it was.  Device memory per batch:
 * the text, 29 bytes per line (line table, byte and record scans) and the CSR reads.  Pinned `text` uploads at link speed. */
pgx_status pgx_batch_upload_text(pgx_batch *b, const uint8_t *text, uint64_t n_bytes, uint32_t format, uint64_t *n_reads);
typedef struct { uint64_t n_reads, n_bytes, longest; } pgx_reads_info;
/* The reads a batch holds on its device, as the kernels will read them: offsets[n_reads + 1] (rebased to 0) and bytes[n_bytes].
 * longest = the longest read as the batch recorded it.  offsets / bytes may be NULL (info only); PGX_ERR_ARG when a capacity is too small.
 * Valid after any of the four upload forms, before or after a run; it exists for tests (tests/test_gpu_fastx_borders.py). */
pgx_status pgx_batch_reads(pgx_batch *b, pgx_reads_info *info, uint64_t *offsets, uint64_t offsets_cap, uint8_t *bytes, uint64_t bytes_cap);
/* Host only, no device: the first record start at or after `want` (n_bytes if none); what a caller that cuts a file into batches needs.
 *   LINES  the start of the next non-empty line.
 *   FASTQ  the next line start L with byte L '@' and line L+2 starting with '+' (a quality line that starts with '@' fails: its line
 *          L+2 is a sequence line); fewer than 4 lines left from L means n_bytes.
 *   FASTA  the next line that starts with '>'.
 * PGX_ERR_ARG for an unknown format. */
pgx_status pgx_fastx_cut(const uint8_t *text, uint64_t n_bytes, uint32_t format, uint64_t want, uint64_t *cut);
/* Run find_all_mems (+ tag queries) for every read of the batch; results stay on the device.
 * (A run whose predecessor on this batch had the same shape is enqueued whole, with buffer sizes taken from that run and the
 * counts kept on the device, and synchronises once at the end: pgx_batch_spec_stats.)
 * `stream` is a hipStream_t; NULL = the batch's own non-blocking stream (every batch has one: its uploads and downloads
 * use it too, so batches driven by different host threads overlap on one device -- upload of one, kernels of another,
 * download of a third).  Asynchronous except for the few scalar read-backs that size intermediate buffers; complete
 * when it returns. */
pgx_status pgx_batch_run(pgx_batch *b, uint64_t min_len, uint64_t min_occ, uint32_t flags, void *stream);
/* Copy the results of the last run to host memory owned by the batch (valid until next run/free) */
pgx_status pgx_batch_result(pgx_batch *b, pgx_result *out);
/* The results of the last run where they are: device pointers into buffers owned by the batch (valid until the next
 * run / upload / free; the run has completed when pgx_batch_run returns).  For consumers that stay on the GPU, e.g.
 * the RCCL exchange of the chromosome-sharded mode, instead of pgx_batch_result's copy to host memory. */
typedef struct {
    uint64_t n_reads, n_mems, n_positions;
    const uint64_t *mem_offsets;    /* n_reads + 1 */
    const pgx_mem *mems;            /* n_mems */
    const uint64_t *tag_run_counts; /* n_mems        (NULL when the run had no PGX_RUN_TAGS) */
    const uint64_t *pos_offsets;    /* n_mems + 1    (NULL ...) */
    const uint64_t *positions;      /* n_positions   (NULL ...) */
} pgx_device_result;
pgx_status pgx_batch_device_result(pgx_batch *b, pgx_device_result *out);
/* Device-side totals of the last run without downloading arrays */
pgx_status pgx_batch_counts(pgx_batch *b, uint64_t *n_mems, uint64_t *n_positions, uint64_t *n_extensions);
pgx_status pgx_batch_timing(pgx_batch *b, pgx_timing *out);
/* Runs of this batch that were sized speculatively (from the totals of the previous run with the same number of reads and the
 * same parameters: no mid-run read-back, one synchronisation at the end), and how many of those had to be repeated with exact
 * sizes because a capacity was too small.  Results never depend on it; PGX_SPEC=0 in the environment switches it off. */
pgx_status pgx_batch_spec_stats(pgx_batch *b, uint32_t *speculative_runs, uint32_t *fallbacks);
void pgx_batch_free(pgx_batch *b);
/* ---- locate the MEMs of the last run, on the device --------------------------------------------------------------
 * For MEM m of the last pgx_batch_run (mems[m] of pgx_batch_result, same order) the occurrences are the suffix-array values of BWT
 * rows [bwt_start, bwt_start + size - 1], in exactly the forms pgx_locate_batch defines: flags = 0 packed positions
 * seq * max_length + offset in BWT order; PGX_LOCATE_SEQ_IDS sequence ids in BWT order; PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE sorted
 * unique sequence ids (PGX_LOCATE_UNIQUE alone: sorted unique packed positions).  MEM m's values equal
 * pgx_locate_batch(first = bwt_start, last = bwt_start + size - 1, flags); there is no other definition of correctness.
 *   max_occ (0 = no cap): a MEM with size > max_occ gets no values and counts as not located (its loc_offsets entry stays empty, its
 *     size stays in mems[m].size).
 *   size <= 0, or a range that would end at or beyond bwt_size: no values, counted as not located, never read.
 *   Support is pgx_locate_batch's: PGX_ERR_UNSUPPORTED in COMPAT mode on an encoded index without N.  A failed or refused call
 *     leaves the batch's find_mems results as they were (and no locate result).
 * Runs on the device-resident MEMs (no re-run of the search) on `stream` (as pgx_batch_run: NULL = the batch's own stream) and is
 * complete when it returns.  Where the index keeps its whole suffix array on the device (the LCE image of narrow bidirectional
 * indexes) the values are a gather from it; elsewhere the sample chains of pgx_locate_batch are walked.  PGX_LOCATE_CHAINS (tests)
 * forces the chains.  The values of a batch are produced in passes over consecutive MEMs whose intermediate buffer stays within
 * PGX_LOCATE_BUDGET_MB (environment; default a quarter of free device memory); results never depend on it.
 * PGX_ERR_ARG without a completed run.
 *
 * PGX_LOCATE_SEQ_SETS (alone or with PGX_LOCATE_CHAINS; with PGX_LOCATE_SEQ_IDS or PGX_LOCATE_UNIQUE: PGX_ERR_ARG): the sequences that hold
 * each MEM as a bitmap, the input of set AND / OR across the MEMs of a read.  With n_seq = pgx_index_info.n_sequences and
 * W = ceil(n_seq / 64), values holds n_mems x W words, MEM m's set is values[m * W .. (m + 1) * W), loc_offsets[m] = m * W and
 * n_values = n_mems * W.  Bit s & 63 of word s >> 6 is set iff s is among the values of
 * pgx_locate_batch(first = bwt_start, last = bwt_start + size - 1, PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE) for that MEM; bits at or beyond
 * n_seq are zero.  A MEM that is not located (the rules above) has an all-zero set and counts in n_not_located.  Built without writing or
 * sorting the occurrences: every occurrence sets its bit.  PGX_ERR_UNSUPPORTED where W > 64 (more than 4096 sequences: a bitmap per MEM
 * then costs more than the ids it replaces).  pgx_locate_batch does not take the flag.
 * Where W <= 64, PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE is served from the same sets (built in passes within the budget, expanded to
 * ascending ids) in place of the segmented sort: the result is the same byte for byte, and set_words tells that it happened.
 * PGX_LOCATE_SETS=0 (environment, read per call) forces the sort.  PGX_LOCATE_UNIQUE alone always sorts. */
#define PGX_LOCATE_CHAINS 4u
#define PGX_LOCATE_SEQ_SETS 8u
typedef struct {
    uint64_t n_mems;
    uint64_t n_values;
    uint64_t n_not_located;       /* MEMs skipped by max_occ or an invalid range */
    uint32_t flags;               /* what the locate ran with (PGX_LOCATE_CHAINS dropped) */
    uint32_t resident;            /* 1: gathered from the resident suffix array, 0: sample chains */
    const uint64_t *loc_offsets;  /* n_mems + 1; values of MEM m = values[loc_offsets[m] .. [m + 1]) */
    const uint64_t *values;       /* n_values */
    float ms_locate;              /* device time of the call when the last run had PGX_RUN_TIMING, else 0 */
    uint32_t set_words;           /* W when the call built sequence sets (PGX_LOCATE_SEQ_SETS, or unique sequence ids served from them), else 0 */
} pgx_locations;
pgx_status pgx_batch_locate(pgx_batch *b, uint32_t flags, uint64_t max_occ, void *stream);
/* Host copy of the last locate (buffers owned by the batch) / the same as device pointers.  Valid until the next run, upload, locate or
 * free of the batch; PGX_ERR_ARG when there is none. */
pgx_status pgx_batch_locations(pgx_batch *b, pgx_locations *out);
pgx_status pgx_batch_device_locations(pgx_batch *b, pgx_locations *out);

/* ---- read hits: every read scored against every sequence, on the device ------------------------------------------------------
 * The consumer of PGX_LOCATE_SEQ_SETS: the MEMs of a read and their sequence sets reduced to one fixed record per read, so that only
 * 40 bytes a read cross the link instead of n_mems x W set words plus the MEM array.
 *
 * DEFINITIONS.  Read r has the MEMs m in [mem_offsets[r], mem_offsets[r + 1]).
 *   len(m)    = end - start if end > start, else 0 (end is exclusive, algorithm.hpp:710-713).
 *   set(m)    = MEM m's W = ceil(n_seq / 64) words in the PGX_LOCATE_SEQ_SETS form; bits at or beyond n_seq are ignored.
 *   cov(r, s) = the number of read positions in the union of [start, end) over the MEMs of r whose set has bit s.  Overlapping and
 *               nested MEMs count a position once; a MEM with an all-zero set (not located) adds nothing.
 * Precondition: within a read the MEM starts ascend strictly (pgx_batch_run guarantees it in both modes: every step of find_all_mems
 * appends at most one MEM and moves on to a larger start).  Ends need not ascend, and the result is exact when they do not.
 * pgx_read_hit (40 bytes; offsets 0 best_score, 8 next_score, 16 covered, 24 best_seq, 28 n_best, 32 n_located, 36 n_mems):
 *   best_score  max over s < n_seq of cov(r, s); 0 if the read has no located MEM
 *   next_score  the largest cov(r, s) that is < best_score; 0 if there is none
 *   covered     the union length over all MEMs of r with a non-empty set: what a sequence holding every located MEM would score
 *   best_seq    the smallest s with cov(r, s) == best_score; PGX_NO_SEQUENCE when best_score == 0
 *   n_best      the number of such s; 0 when best_score == 0
 *   n_located   MEMs of r with a non-empty set
 *   n_mems      all MEMs of r
 * PGX_HITS_BEST_SETS adds best_sets[r * W + j]: bit s & 63 of word s >> 6 is set iff cov(r, s) == best_score > 0; bits at or beyond
 * n_seq are zero.  PGX_HITS_SCORES adds scores[r * n_seq + s] = min(cov(r, s), 2^32 - 1). */
#define PGX_HITS_BEST_SETS 1u
#define PGX_HITS_SCORES 2u
#define PGX_NO_SEQUENCE 0xFFFFFFFFu
typedef struct {
    uint64_t best_score, next_score, covered;
    uint32_t best_seq, n_best, n_located, n_mems;
} pgx_read_hit;
typedef struct {
    uint64_t n_reads, n_seq;
    uint32_t set_words; /* W */
    uint32_t flags;     /* PGX_HITS_* the call ran with */
    const pgx_read_hit *hits;  /* n_reads */
    const uint64_t *best_sets; /* n_reads x W; NULL without PGX_HITS_BEST_SETS */
    const uint32_t *scores;    /* n_reads x n_seq; NULL without PGX_HITS_SCORES */
    float ms_hits;             /* device time of the call when the run had PGX_RUN_TIMING, else 0 */
    uint32_t reserved;
} pgx_read_hits;
/* The hits of the last run from the sequence sets of the last locate, which must be a completed pgx_batch_locate(PGX_LOCATE_SEQ_SETS
 * [| PGX_LOCATE_CHAINS]) and the batch's current locate result: PGX_ERR_ARG otherwise (also for an unknown flag); the run and locate
 * results then stay as they were and there is no hits result.  One kernel launch on `stream` (NULL = the batch's own), complete on
 * return; it reads the sets where the locate left them, no value crosses the link.  Buffers grow only.  The hits stay valid until the
 * next run, upload, pgx_batch_read_hits or free of the batch; a later pgx_batch_locate of any form leaves them valid (hits first,
 * positions afterwards).  With PGX_HITS_SCORES the n_reads x n_seq x 4 bytes must fit a quarter of the free device memory:
 * PGX_ERR_NOMEM with both numbers otherwise.  A read takes Sp lanes (the power of two >= min(n_seq, 64)) of the one launch, which holds
 * fewer than 2^32 threads: a batch of 2^32 / Sp reads or more (2^26 at 64 lanes) is PGX_ERR_UNSUPPORTED, here and in pgx_read_hits_arrays.
 * The sets are taken as the locate left them: what pgx_batch_locate could not complete is not noticed here. */
pgx_status pgx_batch_read_hits(pgx_batch *b, uint32_t flags, void *stream);
/* Host copy of the last hits (pinned buffers owned by the batch) / the same as device pointers.  PGX_ERR_ARG when there are none. */
pgx_status pgx_batch_hits(pgx_batch *b, pgx_read_hits *out);
pgx_status pgx_batch_device_hits(pgx_batch *b, pgx_read_hits *out);
/* The same kernels on host arrays (how they are tested on shapes no index produces): mem_offsets (n_reads + 1 entries, from 0, never
 * decreasing; mems holds mem_offsets[n_reads] records), sets (that many x set_words words).  PGX_ERR_ARG unless set_words ==
 * ceil(n_seq / 64) and 1 <= set_words <= 64, and for a read whose MEM starts do not ascend strictly: the first such read is named, the
 * check runs on the device and nothing is written.  best_sets / scores may be NULL when their flag is clear.  PGX_ERR_NO_DEVICE without
 * a GPU. */
pgx_status pgx_read_hits_arrays(int device, const uint64_t *mem_offsets, uint64_t n_reads, const pgx_mem *mems, const uint64_t *sets, uint32_t set_words,
                                uint64_t n_seq, uint32_t flags, pgx_read_hit *hits, uint64_t *best_sets, uint32_t *scores);

/* ---- read placement: every read placed on its best sequence diagonal, on the device ------------------------------------------
 * The consumer of the packed positions (pgx_batch_locate with flags = 0): where on a sequence a read lies, not only on which one.  The
 * occurrences of a read's MEMs vote for diagonals, every diagonal is scored by the read positions it covers, and one 64-byte record
 * per read crosses the link instead of 8 bytes per occurrence.
 *
 * DEFINITIONS.  Read r has the MEMs m in [mem_offsets[r], mem_offsets[r + 1]); MEM m has the values values[loc_offsets[m] ..
 * loc_offsets[m + 1]) of a completed pgx_batch_locate(flags = 0 [| PGX_LOCATE_CHAINS]).  With L = pgx_index_info.max_length:
 *   anchor      of value v of MEM m: seq = v / L, off = v % L, diag = (int64)off - (int64)mems[m].start: the sequence offset on which
 *               read position 0 falls; negative when the read hangs over the sequence start.
 *   placement   of read r: a pair (seq, diag) that at least one anchor of r has.
 *   len(m)      as in read hits: end - start if end > start, else 0.
 *   cov(r, seq, diag) = the number of read positions in the union of [start, end) over the MEMs of r that have an anchor on
 *               (seq, diag).  Overlapping and nested MEMs count a position once.
 * A MEM that is not located (cap, invalid range, size <= 0) has no values and adds nothing.  Placements of a read are ordered by
 * (seq ascending, diag ascending as signed); "first" means first in that order.  Precondition, as for read hits: MEM starts ascend
 * strictly within a read (pgx_batch_run guarantees it; ends need not ascend).
 * pgx_read_place (64 bytes, little endian):
 *    0 best_score    u64  max over the read's placements of cov; 0 when the read has no anchor
 *    8 next_score    u64  the largest cov of a placement that is < best_score; 0 if none
 *   16 best_diag     i64  diag of the first placement that reaches best_score; 0 when best_score == 0
 *   24 n_anchors     u64  values of the read's MEMs (duplicate values inside one MEM count)
 *   32 n_placements  u64  distinct (seq, diag)
 *   40 best_seq      u32  seq of that first best placement; PGX_NO_SEQUENCE when best_score == 0
 *   44 n_best        u32  placements with cov == best_score > 0, held at 2^32 - 1
 *   48 best_mems     u32  distinct MEMs with an anchor on the first best placement; 0 when best_score == 0
 *   52 n_located     u32  MEMs of r with at least one value
 *   56 n_mems        u32  all MEMs of r
 *   60 reserved      u32  0
 * A placement whose MEMs all have len == 0 has cov == 0: it counts in n_placements but is never "best".
 * PGX_PLACE_LIST adds every placement of every read as a CSR list: place_offsets[n_reads + 1] and places[], 24-byte pgx_placement
 * records, per read in the placement order above; n_placements of the record equals the read's list length.
 * The result does not depend on the order of a MEM's values, on the memory budget, on the lane packing or on the locate path. */
#define PGX_PLACE_LIST 1u
typedef struct {
    uint64_t best_score, next_score;
    int64_t best_diag;
    uint64_t n_anchors, n_placements;
    uint32_t best_seq, n_best, best_mems, n_located, n_mems, reserved;
} pgx_read_place;
typedef struct {
    int64_t diag;
    uint64_t score; /* cov of the placement */
    uint32_t seq;
    uint32_t mems;  /* distinct MEMs with an anchor on it */
} pgx_placement;
typedef struct {
    uint64_t n_reads;
    uint64_t n_anchors;            /* values the call consumed */
    uint64_t n_places;             /* length of places: 0 without PGX_PLACE_LIST */
    uint32_t flags;                /* PGX_PLACE_* the call ran with */
    uint32_t n_passes;             /* passes over consecutive whole reads the key buffer took (PGX_PLACE_BUDGET_MB) */
    const pgx_read_place *reads;   /* n_reads */
    const uint64_t *place_offsets; /* n_reads + 1; NULL without PGX_PLACE_LIST */
    const pgx_placement *places;   /* n_places; NULL without PGX_PLACE_LIST */
    float ms_place;                /* device time of the call when the run had PGX_RUN_TIMING, else 0 */
    uint32_t reserved;
} pgx_read_places;
/* The placements of the last run from the packed positions of the last locate, which must be a completed pgx_batch_locate(0
 * [| PGX_LOCATE_CHAINS]) and the batch's current locate result: PGX_ERR_ARG otherwise, with what the last locate ran with (also for an
 * unknown flag); run, locate and an earlier place result then stay as they were.  Runs on `stream` (NULL = the batch's own), complete on
 * return.  One 64-bit key per anchor is built, the keys of each read are sorted (the segmented sort of the tag stage) and swept, in
 * passes over consecutive whole reads whose keys stay within PGX_PLACE_BUDGET_MB (environment, read per call, fractions allowed;
 * default a quarter of the free device memory); a single read whose anchors exceed it is PGX_ERR_NOMEM naming the read.  The key holds
 * sequence, biased diagonal and the MEM's ordinal within its read: where bits(n_seq * (max_length + largest MEM start)) + bits(most
 * MEMs of a read - 1) exceed 64 the call is PGX_ERR_UNSUPPORTED, as are 2^31 reads or MEMs or more, before anything is written.  With
 * PGX_PLACE_LIST the list must fit a quarter of the free device memory: PGX_ERR_NOMEM with both numbers otherwise.  Buffers grow only
 * and are the stage's own: the places stay valid until the next run, upload, pgx_batch_read_place or free of the batch, and a later
 * pgx_batch_locate of any form leaves them valid. */
pgx_status pgx_batch_read_place(pgx_batch *b, uint32_t flags, void *stream);
/* Host copy of the last places (pinned buffers owned by the batch) / the same as device pointers.  PGX_ERR_ARG when there are none. */
pgx_status pgx_batch_places(pgx_batch *b, pgx_read_places *out);
pgx_status pgx_batch_device_places(pgx_batch *b, pgx_read_places *out);
/* The same kernels on host arrays (how they are tested on shapes no index produces).  mem_offsets: n_reads + 1 entries; mems:
 * mem_offsets[n_reads] records; loc_offsets: mem_offsets[n_reads] + 1 entries; values: loc_offsets[last] values.  PGX_ERR_ARG with
 * nothing written: an unknown flag, max_length or n_seq of 0, offsets that do not start at 0 or decrease, and -- checked on the device,
 * the first offending read named -- MEM starts that do not ascend strictly and a value with v / max_length >= n_seq.  Duplicate values
 * inside one MEM are allowed (n_anchors counts them, nothing else changes).  With PGX_PLACE_LIST place_offsets takes n_reads + 1
 * entries and places up to places_cap records: PGX_ERR_NOMEM with the needed count when the list is longer (nothing is written).
 * Both may be NULL without the flag.  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_place_arrays(int device, const uint64_t *mem_offsets, uint64_t n_reads, const pgx_mem *mems, const uint64_t *loc_offsets,
                                 const uint64_t *values, uint64_t n_seq, uint64_t max_length, uint32_t flags, pgx_read_place *out,
                                 uint64_t *place_offsets, pgx_placement *places, uint64_t places_cap);

/* ---- read verify: every read laid on the indexed text at its placements, on the device ---------------------------------------
 * What a consumer of a placement does next (the reference's downstream consumer extends its seeds without gaps for the same reason):
 * the whole read is compared with the text at a candidate placement and what matches is counted, so that a read with one substitution
 * is told from one whose other half lies elsewhere, and ties between placements are broken by evidence.  The text is the TEXT image,
 * recovered on the device from the index alone (the first symbol of suffix i is the symbol whose C-bucket holds i), built on first use
 * for any index pgx_locate_batch supports with bwt_size < 2^32 - 2^20; it is not stored in image files.
 *
 * DEFINITIONS.  Read r has bytes R[0, len).  A candidate is a pair (seq, diag).  Sequence seq has Ls symbols T[0, Ls), endmarker excluded.
 *   span         the read positions i with 0 <= diag + i < Ls: [lo, hi) with lo = max(0, -diag), hi = min(len, Ls - diag); empty
 *                (hi <= lo, then lo = hi = 0) when the read does not overlap the sequence
 *   match at i   R[i] is one of upper-case A C G T and equals T[diag + i].  Everything else in the span is a mismatch: lower case, N,
 *                IUPAC codes, a text N (N opposite N too)
 *   matches, mismatches   counts over the span; they sum to hi - lo
 *   longest_run, run_start   the longest stretch of consecutive matches in the span and the smallest start of one; both 0 without a match
 *   segment      with the mismatch penalty P >= 1 the score of [a, b) inside [lo, hi) is (matches in it) - P * (mismatches in it); the
 *                segment is the non-empty [a, b) of largest score, ties to the smallest a, then the smallest b.  seg_score is that score
 *                (at least 1 whenever matches >= 1), seg_mismatches the mismatches inside it.  Without a match seg_score = 0,
 *                seg_start = seg_end = lo, seg_mismatches = 0.
 * The maximum is associative -- the monoid (total, best prefix with smallest end, best suffix with smallest start, best with the
 * lexicographically smallest (a, b)) yields exactly this tie rule --, so a kernel may split a read over lanes or walk it in one.
 * CANDIDATES of read r in the batch form: its placements with cov == best_score > 0 in placement order (seq ascending, signed diag
 * ascending), the first max_cand of them, 1 <= max_cand <= 64.  max_cand == 1 needs only the place records (best_seq, best_diag);
 * max_cand > 1 needs a place result made with PGX_PLACE_LIST.  A read with best_score == 0 has no candidate.
 * WINNER: the candidate with the largest seg_score, then the most matches, then the first in candidate order.
 * pgx_read_verify (64 bytes, little endian; every field but diag is u32):
 *    0 diag i64                  8 seq (PGX_NO_SEQUENCE and everything else 0 when the read has no candidate)
 *   12 n_cand                    candidates verified for the read (in the per-candidate list: this candidate's ordinal)
 *   16 span_lo   20 span_hi      24 matches     28 mismatches
 *   32 seg_start 36 seg_end      40 seg_score   44 seg_mismatches
 *   48 longest_run 52 run_start
 *   56 cand_index                the winner's ordinal among the candidates (in the list: this candidate's ordinal)
 *   60 n_tied                    candidates that equal the winner in (seg_score, matches), the winner included (in the list: 0)
 * PGX_VERIFY_LIST adds cand_offsets[n_reads + 1] and one such record per candidate, in candidate order.
 * A pgx_batch_read_mates call with PGX_MATES_ELECT rewrites the winner records of the batch with the candidates the pairs chose ("read mates").
 * Reads of 2^31 bytes or more are PGX_ERR_UNSUPPORTED. */
#define PGX_VERIFY_LIST 1u
#define PGX_VERIFY_MAX_CAND 64u
#define PGX_VERIFY_MAX_PENALTY (1u << 20)
typedef struct {
    int64_t diag;
    uint32_t seq, n_cand, span_lo, span_hi, matches, mismatches, seg_start, seg_end, seg_score, seg_mismatches, longest_run, run_start, cand_index, n_tied;
} pgx_read_verify;
typedef struct {
    uint64_t n_reads;
    uint64_t n_cands;              /* candidates verified over all reads */
    uint32_t flags;                /* PGX_VERIFY_* the call ran with */
    uint32_t max_cand, mismatch_penalty, reserved;
    const pgx_read_verify *reads;  /* n_reads */
    const uint64_t *cand_offsets;  /* n_reads + 1; NULL without PGX_VERIFY_LIST */
    const pgx_read_verify *cands;  /* n_cands; NULL without PGX_VERIFY_LIST */
    float ms_verify;               /* device time of the call when the run had PGX_RUN_TIMING, else 0 (the text image's build is not in it) */
    uint32_t reserved2;
} pgx_read_verifies;
/* The collection the index was built from, recovered on `device` from the index alone: seq_lengths[n_seq] (without endmarkers) and, when
 * text != NULL, the sequences as bytes, each followed by '\n' (bwt_size bytes in all).  Builds the text image if it is not built.
 * PGX_ERR_ARG when n_seq_cap is below the number of sequences or text_cap below bwt_size.  PGX_ERR_UNSUPPORTED, naming the reason: COMPAT
 * mode on an encoded index without N (locate is unsupported there), an image opened from a file saved without the locate image, bwt_size
 * >= 2^32 - 2^20.  PGX_ERR_NOMEM with both numbers when the free device memory is below what the build needs for a while (the suffix
 * array at 8 bytes a symbol, a byte a symbol, the image at half a byte a symbol). */
pgx_status pgx_index_text(pgx_index *h, int device, uint64_t *seq_lengths, uint64_t n_seq_cap, uint8_t *text, uint64_t text_cap);
/* Verifies the reads of the last run at the candidates of the last pgx_batch_read_place, which must be this run's: PGX_ERR_ARG otherwise,
 * and for max_cand outside 1 .. 64, max_cand > 1 on a place result without PGX_PLACE_LIST, mismatch_penalty 0 or above 2^20 and an
 * unknown flag; run, locate, place and an earlier verify result then stay as they were.  Builds the text image on first use
 * (PGX_ERR_UNSUPPORTED / PGX_ERR_NOMEM as pgx_index_text).  Runs on `stream` (NULL = the batch's own), complete on return.  Buffers grow
 * only and are the stage's own: the result stays valid until the next run, upload, pgx_batch_read_verify or free of the batch, and a
 * later pgx_batch_locate of any form leaves it valid. */
pgx_status pgx_batch_read_verify(pgx_batch *b, uint32_t max_cand, uint32_t mismatch_penalty, uint32_t flags, void *stream);
/* Host copy of the last verify result (pinned buffers owned by the batch) / the same as device pointers.  PGX_ERR_ARG when there is none. */
pgx_status pgx_batch_verified(pgx_batch *b, pgx_read_verifies *out);
pgx_status pgx_batch_device_verified(pgx_batch *b, pgx_read_verifies *out);
/* The same kernels on host arrays: the sequences as bytes (\n A C G N T; PGX_ERR_UNSUPPORTED naming byte and offset otherwise) with
 * seq_offsets[n_seq + 1], no endmarkers (packed on the device by the image's pack kernel); the reads as bytes with read_offsets[n_reads + 1];
 * the candidates as a CSR list per read, cand_offsets[n_reads + 1], of (cand_seq, cand_diag) -- any candidate, one that does not overlap
 * its sequence included, any number per read.  `out` takes n_reads records; with PGX_VERIFY_LIST list_offsets takes n_reads + 1 entries and
 * list up to list_cap records (PGX_ERR_NOMEM with the needed count when there are more; both may be NULL without the flag).
 * PGX_ERR_ARG with nothing written: an unknown flag, a penalty of 0 or above 2^20, offsets that do not start at 0 or decrease and --
 * checked on the device, the first offending read named -- a cand_seq >= n_seq.  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_verify_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads,
                                  const uint64_t *read_offsets, uint64_t n_reads, const uint64_t *cand_offsets, const uint32_t *cand_seq,
                                  const int64_t *cand_diag, uint32_t mismatch_penalty, uint32_t flags, pgx_read_verify *out,
                                  uint64_t *list_offsets, pgx_read_verify *list, uint64_t list_cap);

/* ---- read mates: the two reads of a pair choose their placements together, on the device --------------------------------------------
 * Short reads come in pairs: two reads from the two ends of one fragment, facing each other, a few hundred bases apart.  A read that lies
 * inside an exact repeat ties between the copies in place and in verify; its mate, placed uniquely nearby, settles it.  This stage looks
 * at the verify candidates of both mates and lets the pair choose.  It sits between verify and align and reads nothing but verify's list.
 *
 * DEFINITIONS.  Reads 2k and 2k + 1 of a batch are mates A and B of pair k.  Read r has the candidates of the verify list, in candidate
 * order, each with (seq, diag, seg_score, matches).  Sequence q has L[q] symbols, without its endmarker.
 *   twins        the index is twinned iff n_seq is even and L[2p] == L[2p + 1] for every p: a collection that holds path p forward as
 *                sequence 2p and reversed as 2p + 1 (gbz_extract -b).  A forward / reverse pair lands on twin sequences.
 *   compatible   candidate i of A and candidate j of B are compatible iff seq_i ^ 1 == seq_j and frag_min <= frag <= frag_max, with
 *                frag = L[seq_i] - diag_i - diag_j, signed 64-bit and symmetric in A and B (|diag| stays below 2^62).  For the fragment
 *                [f, f + I) of path p, A its first la bases on 2p at diag f, B the reverse complement of its last lb bases on 2p + 1 at
 *                diag L - f - I, this is frag = I; a fragment from the other strand swaps the roles and gives the same value.
 *   solo winner  verify's WINNER rule recomputed from the list (largest seg_score, then most matches, then the first), not read from the
 *                winner records: a second call on the same verify result gives the same answer after an election.
 *   best pair    the compatible pair with the largest seg_score_i + seg_score_j, then the largest matches_i + matches_j, then the
 *                smallest i, then the smallest j.  n_compatible counts the compatible pairs, n_best those that equal the best in both
 *                sums, next_score is the largest score sum of a compatible pair below the best one's, 0 if there is none.  Sums are
 *                formed and compared in 64 bits; a stored sum is held at 2^32 - 1 (verify's own records cannot reach it).
 *   PROPER       with the unpaired penalty U: a compatible pair exists and pair_score + U >= solo_score, in 64 bits.  The solo winners
 *                always score at least as much as any pair; U is what a user pays in seg_score to keep the mates together.  A PROPER
 *                pair chooses the best pair's candidates; without PROPER each mate keeps its solo winner.
 * Like place's and verify's reductions the best pair is a monoid -- (best key (score sum, matches sum, i, j), the count of pairs equal to
 * it in both sums, the best score sum below it, the count of all) merges associatively and commutatively --, so a kernel may split the
 * i x j grid any way it likes.
 * pgx_read_mates (64 bytes, little endian, one per pair):
 *    0 frag i64          frag of the best pair when one is compatible, else 0
 *    8 pair_score u32    seg_score sum of the best compatible pair         12 solo_score u32    seg_score sum of the two solo winners
 *   16 cand_a u32        ordinal of the chosen candidate of A: the best pair's if PROPER, else the solo winner's; 0 for a mate without one
 *   20 cand_b u32        the same for B
 *   24 solo_a  28 solo_b u32   ordinals of the solo winners (0 without a candidate)
 *   32 n_compatible  36 n_best  40 next_score u32   see above
 *   44 pair_matches u32  matches sum of the best compatible pair
 *   48 seq_a  52 seq_b u32    sequence of the chosen candidate; PGX_NO_SEQUENCE without one
 *   56 flags u32         PGX_MATES_PROPER, _COMPATIBLE, _HAS_A, _HAS_B (the mate has a candidate), _MOVED_A, _MOVED_B (chosen != solo)
 *   60 reserved u32      0
 * PGX_MATES_ELECT makes the chosen candidates the winners: the verify winner record of every read is overwritten with the list record of
 * its chosen candidate, n_cand set to the read's candidate count, cand_index to the chosen ordinal and n_tied to the number of the read's
 * candidates that equal the chosen one in (seg_score, matches), the chosen one included.  Reads whose chosen candidate is their solo
 * winner get the bytes they had.  pgx_batch_read_align and pgx_batch_read_walk then work on the elected winners.  Without the flag the
 * verify result is untouched. */
#define PGX_MATES_ELECT 1u
#define PGX_MATES_PROPER 1u     /* bits of pgx_read_mates.flags */
#define PGX_MATES_COMPATIBLE 2u
#define PGX_MATES_HAS_A 4u
#define PGX_MATES_HAS_B 8u
#define PGX_MATES_MOVED_A 16u
#define PGX_MATES_MOVED_B 32u
typedef struct {
    int64_t frag;
    uint32_t pair_score, solo_score, cand_a, cand_b, solo_a, solo_b, n_compatible, n_best, next_score, pair_matches, seq_a, seq_b, flags, reserved;
} pgx_read_mates;
typedef struct {
    uint64_t n_pairs;
    uint64_t n_proper, n_compatible, n_moved_a, n_moved_b; /* pairs with the flag, summed on the device */
    int64_t frag_min, frag_max;   /* what the call ran with */
    uint32_t flags;               /* PGX_MATES_ELECT or 0 */
    uint32_t penalty;
    const pgx_read_mates *pairs;  /* n_pairs */
    float ms_mates;               /* device time of the call when the run had PGX_RUN_TIMING, else 0 */
    uint32_t reserved;
} pgx_read_mates_result;
/* Whether the index is twinned (see above): *first_bad is 2^64 - 1 if it is, else the first p with L[2p] != L[2p + 1], or n_seq / 2 when
 * n_seq is odd.  Builds the text image on `device` if it is not built (errors as pgx_index_text). */
pgx_status pgx_index_twinned(pgx_index *h, int device, uint64_t *first_bad);
/* Pairs the reads of the last run from the list of the last pgx_batch_read_verify, which must be this run's and made with
 * PGX_VERIFY_LIST.  PGX_ERR_ARG with nothing changed, naming what was found: no such verify result, an unknown flag, frag_min > frag_max,
 * an odd read count.  PGX_ERR_UNSUPPORTED naming the first p that breaks it when the index is not twinned.  A pair takes the smallest
 * power of two of lanes that is at least the verify call's max_cand (PGX_MATES_LANES in the environment, read per call, 1 .. 64, raises
 * it; results never depend on it).  Runs on `stream` (NULL = the batch's own), complete on return.  Buffers grow only and are the stage's
 * own: the result stays valid until the next run, upload, pgx_batch_read_mates or free of the batch, and a later pgx_batch_locate of any
 * form leaves it valid. */
pgx_status pgx_batch_read_mates(pgx_batch *b, int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t flags, void *stream);
/* Host copy of the last mates result (a pinned buffer owned by the batch) / the same as a device pointer.  PGX_ERR_ARG when there is none. */
pgx_status pgx_batch_mated(pgx_batch *b, pgx_read_mates_result *out);
pgx_status pgx_batch_device_mated(pgx_batch *b, pgx_read_mates_result *out);
/* The same kernel on stated lists (how shapes no index produces are tested): seq_lengths[n_seq]; cand_offsets[n_reads + 1] into cands, list
 * records of pgx_read_verify of which seq, diag, seg_score and matches are read (and all 64 bytes copied with PGX_MATES_ELECT).  `out`
 * takes n_reads / 2 records; `winners` takes n_reads records with PGX_MATES_ELECT and may be NULL without it.  PGX_ERR_ARG with nothing
 * written, the first offender named: an unknown flag, frag_min > frag_max, an odd n_seq, unequal twin lengths, offsets that do not start
 * at 0 or decrease, more than 64 candidates for a read, a seq >= n_seq, an odd n_reads.  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_mates_arrays(int device, const uint64_t *seq_lengths, uint64_t n_seq, uint64_t n_reads, const uint64_t *cand_offsets,
                                 const pgx_read_verify *cands, int64_t frag_min, int64_t frag_max, uint32_t penalty, uint32_t flags,
                                 pgx_read_mates *out, pgx_read_verify *winners);

/* ---- read rescue: the unplaced mate of a pair searched for next to the placed one, on the device --------------------------------------
 * pgx_batch_read_mates chooses among the candidates place produced, and a read has one only where a MEM of min_len was located.  A mate
 * with a substitution every ten bases, or one whose MEMs the place or run limits cut away, has none near its truth.  Its mate usually sits
 * uniquely, and the pair's geometry says where to look: on the twin sequence, inside a window of frag_max - frag_min + 1 diagonals.  This
 * stage scores every diagonal of that window against the read.  It sits between verify and mates.
 *
 * DEFINITIONS.  Reads 2k and 2k + 1 are the mates of pair k; verify's list (PGX_VERIFY_LIST) gives every read its candidates; L[q] is the
 * length of sequence q without its endmarker; P is the mismatch penalty of the verify call; "compatible", "solo winner" and frag are those
 * of "read mates" under the frag_min and frag_max of this call.
 *   target       read t with mate a is a target iff the pair has no compatible candidate pair, a has at least one candidate and t has
 *                fewer than PGX_VERIFY_MAX_CAND.  A read with PGX_VERIFY_MAX_CAND candidates in such a pair gets PGX_RESCUE_FULL and is
 *                no target.  Both reads of a pair may be targets.
 *   anchors      of a target: the candidates of a that equal a's solo winner in (seg_score, matches), in candidate order, the first
 *                max_anchors of them, 1 <= max_anchors <= PGX_RESCUE_MAX_ANCHORS.
 *   task (t, anchor i)   the sequence is s = seq_i ^ 1; the window is the diagonals d with frag_min <= L[s] - diag_i - d <= frag_max,
 *                clipped to those on which the read overlaps the sequence, -(len_t - 1) <= d <= L[s] - 1; empty for len_t == 0, and a
 *                task may be empty.  All of it signed 64-bit (|diag| stays below 2^62).
 *   score of a diagonal   verify's seg_score and matches of read t at (s, d), with the same P and the same match rule.
 *   best diagonal   of a target, over all its tasks: the largest seg_score, then the most matches, then the smallest anchor ordinal,
 *                then the smallest d.  n_diags counts the diagonals scored, n_best those that equal the best in (seg_score, matches),
 *                held at 2^32 - 1; next_score is the largest seg_score strictly below the best one's, 0 if there is none.
 *   RESCUED      n_diags > 0 and the best seg_score >= min_score, min_score >= 1.
 * The best diagonal is a monoid like the best pair of "read mates", so a kernel may split windows and tasks as it likes.
 * pgx_read_rescue (64 bytes, little endian, one per read):
 *    0 diag i64          the best diagonal; 0 without one
 *    8 n_diags u64       diagonals scored over all tasks of the read
 *   16 seq u32           sequence of the best diagonal; PGX_NO_SEQUENCE for a read that is no target and for a target with n_diags == 0
 *   20 flags u32         PGX_RESCUE_TARGET, _RESCUED, _FULL
 *   24 anchor u32        ordinal, in the mate's list, of the anchor whose task holds the best diagonal
 *   28 n_anchors u32     anchors (= tasks) of the target
 *   32 seg_score  36 matches u32   of the best diagonal
 *   40 n_best  44 next_score u32   see above
 *   48 reserved u32[4]   0
 * A read that is no target has every field but seq (and the flag FULL) 0.
 * PGX_RESCUE_MERGE appends the best diagonal of every RESCUED target to its list as its last candidate: the record is byte for byte what
 * verify writes for that read at (seq, diag), with n_cand = cand_index = its ordinal and n_tied = 0.  cand_offsets and n_cands are
 * rebuilt, every winner record is recomputed by verify's WINNER rule (a target without a candidate now has a winner), and an earlier mates
 * result of the run becomes invalid.  The verify result's reported max_cand stays, though a list may now hold max_cand + 1 <= 64
 * entries.  Without the flag the verify result is untouched.  A verify result takes one merge: a second rescue call on it is PGX_ERR_ARG. */
#define PGX_RESCUE_MERGE 1u
#define PGX_RESCUE_TARGET 1u     /* bits of pgx_read_rescue.flags */
#define PGX_RESCUE_RESCUED 2u
#define PGX_RESCUE_FULL 4u
#define PGX_RESCUE_MAX_ANCHORS 8u
#define PGX_RESCUE_MAX_WINDOW 65536
typedef struct {
    int64_t diag;
    uint64_t n_diags;
    uint32_t seq, flags, anchor, n_anchors, seg_score, matches, n_best, next_score, reserved[4];
} pgx_read_rescue;
typedef struct {
    uint64_t n_reads;
    uint64_t n_targets, n_rescued, n_full, n_tasks, n_diags; /* summed on the device */
    int64_t frag_min, frag_max;     /* what the call ran with */
    uint32_t min_score, max_anchors, flags, mismatch_penalty;
    const pgx_read_rescue *reads;   /* n_reads */
    float ms_rescue;                /* device time of the call when the run had PGX_RUN_TIMING, else 0 */
    uint32_t reserved;
} pgx_read_rescue_result;
/* Rescues the reads of the last run from the list of the last pgx_batch_read_verify, which must be this run's and made with
 * PGX_VERIFY_LIST.  PGX_ERR_ARG with nothing changed, naming what was found: no such verify result, one that was already merged, an
 * unknown flag, frag_min > frag_max, frag_max - frag_min >= PGX_RESCUE_MAX_WINDOW, min_score 0, max_anchors outside 1 .. 8, an odd read
 * count.  PGX_ERR_UNSUPPORTED when the index is not twinned (the first p named) or the tasks exceed one launch.  Runs on `stream` (NULL =
 * the batch's own), complete on return.  Buffers grow only and are the stage's own: the result stays valid until the next run, upload,
 * pgx_batch_read_rescue or free of the batch. */
pgx_status pgx_batch_read_rescue(pgx_batch *b, int64_t frag_min, int64_t frag_max, uint32_t min_score, uint32_t max_anchors, uint32_t flags,
                                 void *stream);
/* Host copy of the last rescue result (a pinned buffer owned by the batch) / the same as a device pointer.  PGX_ERR_ARG when there is none. */
pgx_status pgx_batch_rescued(pgx_batch *b, pgx_read_rescue_result *out);
pgx_status pgx_batch_device_rescued(pgx_batch *b, pgx_read_rescue_result *out);
/* The same kernels on host arrays: text, sequences and reads as in pgx_read_verify_arrays (no endmarkers), the lists as in
 * pgx_read_mates_arrays.  `out` takes n_reads records.  With PGX_RESCUE_MERGE list_offsets takes n_reads + 1 entries, list up to list_cap
 * records (PGX_ERR_NOMEM with the needed count when the merged list is longer) and winners n_reads records; all three may be NULL without
 * the flag.  Refuses, with nothing written and the first offender named, what pgx_read_verify_arrays and pgx_read_mates_arrays refuse for
 * the same inputs, and the arguments pgx_batch_read_rescue refuses.  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_rescue_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads,
                                  const uint64_t *read_offsets, uint64_t n_reads, const uint64_t *cand_offsets, const pgx_read_verify *cands,
                                  int64_t frag_min, int64_t frag_max, uint32_t mismatch_penalty, uint32_t min_score, uint32_t max_anchors,
                                  uint32_t flags, pgx_read_rescue *out, uint64_t *list_offsets, pgx_read_verify *list, uint64_t list_cap,
                                  pgx_read_verify *winners);

/* ---- read align: every read aligned with gaps at its verified placement, on the device -------------------------------------------
 * Verify knows only substitutions: a read with a one-base insertion or deletion places on two neighbouring diagonals, each covering part of
 * it, and the winner reads as "half the read matches, then a wall of mismatches".  This stage computes the banded unit-cost alignment of the
 * read against the text around the verify winner and traces it back, so that the answer is "one deletion at read position 71".
 *
 * DEFINITIONS.  Read r has bytes R[0, len).  Its candidate is (seq, diag).  Sequence seq has Ls symbols T[0, Ls).  The band half-width is W,
 * 0 <= W <= 31.
 *   clips        [lo, hi) is the verify span of the candidate: lo = max(0, -diag), hi = min(len, Ls - diag).  Only Q = R[lo, hi) is aligned,
 *                with m = hi - lo and d0 = diag + lo; clip_lo = lo and clip_hi = len - hi are reported as soft clips.  Empty span:
 *                clip_lo = 0, clip_hi = len, everything else 0 (seq and diag stay the candidate's), and one S operation if len > 0.
 *                Because of the clips the main diagonal j = d0 + i lies inside the sequence for every row, so the recurrence is defined
 *                for every candidate.
 *   cells        a cell is (i, j), with i symbols of Q and text offset j consumed.  It is valid iff 0 <= i <= m, 0 <= j <= Ls and |k| <= W,
 *                where k = j - i - d0.  Cells off the sequence do not exist: nothing reads the endmarker or a neighbouring sequence.
 *   match        as in verify: Q[i-1] is an upper-case A C G T and equals T[j-1].  N, lower case, IUPAC codes and a text N never match.
 *   recurrence   unit costs.  D[0][j] = 0 for every valid j, so the start in the text is free.  D[i][j] is the minimum over valid
 *                predecessors of D[i-1][j-1] + (0 if match else 1), D[i-1][j] + 1 (insertion: a read symbol without text),
 *                D[i][j-1] + 1 (deletion).
 *   end cell     the valid cell of row m with the smallest D.  Ties go to the smallest |k|, then to the negative k.
 *   traceback    from the end cell to row 0, the first of these that reproduces D[i][j] is taken: 1. the diagonal move (= on a match, else
 *                X), 2. the insertion (I), 3. the deletion (D).  The path never starts or ends with D.
 *   results      text_start is j at row 0, text_end is j of the end cell (offsets in the sequence); edits = D of the end cell;
 *                n_match + n_mismatch + n_ins = m; n_match + n_mismatch + n_del = text_end - text_start; edits = n_mismatch + n_ins + n_del
 *   band_hit     1 iff W > 0 and some cell of the traced path, ends included, has |k| == W: the banded optimum may then not be the unbanded one
 *   CIGAR        u32 words of length << 4 | op with the BAM codes I = 1, D = 2, S = 4, = is 7, X = 8.  Operations come in read order, equal
 *                neighbours are merged.  A leading S is clip_lo, a trailing S is clip_hi, each only when non-zero.
 *   W = 0        the ungapped case: edits equals verify's mismatches, and text_start == diag + lo
 * pgx_read_align (64 bytes, little endian):
 *    0 diag i64      8 text_start u64     16 text_end u64
 *   24 seq u32 (PGX_NO_SEQUENCE and everything else 0 when the read has no candidate)
 *   28 clip_lo  32 clip_hi  36 edits  40 n_match  44 n_mismatch  48 n_ins  52 n_del  56 n_ops  60 band_hit   (u32 each; nothing is left to pad)
 * n_ops counts the read's CIGAR operations, clips included, with and without PGX_ALIGN_CIGAR.  PGX_ALIGN_CIGAR adds op_offsets[n_reads + 1]
 * and the operations.  The direction planes of the traceback (two bits a cell, max(G, 8) / 4 bytes a read position, G the power of two
 * >= 2 W + 1) live in a scratch buffer that is filled in passes over consecutive whole reads; the passes stay within PGX_ALIGN_BUDGET_MB
 * (read per call, fractions allowed, default a quarter of the free device memory) and results never depend on it.  A single read above the
 * budget is PGX_ERR_NOMEM naming the read.  Reads of 2^28 bytes or more are PGX_ERR_UNSUPPORTED (an operation's length has 28 bits). */
#define PGX_ALIGN_CIGAR 1u
#define PGX_ALIGN_MAX_BAND 31u
#define PGX_ALIGN_OP_I 1u
#define PGX_ALIGN_OP_D 2u
#define PGX_ALIGN_OP_S 4u
#define PGX_ALIGN_OP_EQ 7u
#define PGX_ALIGN_OP_X 8u
typedef struct {
    int64_t diag;
    uint64_t text_start, text_end;
    uint32_t seq, clip_lo, clip_hi, edits, n_match, n_mismatch, n_ins, n_del, n_ops, band_hit;
} pgx_read_align;
typedef struct {
    uint64_t n_reads;
    uint64_t n_ops;               /* CIGAR operations over all reads (with and without PGX_ALIGN_CIGAR) */
    uint32_t flags;               /* PGX_ALIGN_* the call ran with */
    uint32_t band;
    uint32_t passes;              /* passes over the scratch buffer of the direction planes */
    uint32_t reserved;
    const pgx_read_align *reads;  /* n_reads */
    const uint64_t *op_offsets;   /* n_reads + 1; NULL without PGX_ALIGN_CIGAR */
    const uint32_t *ops;          /* n_ops; NULL without PGX_ALIGN_CIGAR */
    uint64_t scratch_bytes;       /* direction planes of the largest pass */
    float ms_align;               /* device time of the call when the run had PGX_RUN_TIMING, else 0 */
    float ms_forward, ms_trace;   /* of it: the forward kernel's launches / the traceback's launches */
    uint32_t reserved2;
} pgx_read_aligns;
/* Aligns the reads of the last run at the winners of the last pgx_batch_read_verify, which must be this run's.  PGX_ERR_ARG with nothing
 * changed: no verify result, band > 31, an unknown flag.  Runs on `stream` (NULL = the batch's own), complete on return.  The result stays
 * valid until the next run, upload, pgx_batch_read_align or free of the batch; a later pgx_batch_locate of any form leaves it valid.  The
 * stage's buffers grow only and are its own. */
pgx_status pgx_batch_read_align(pgx_batch *b, uint32_t band, uint32_t flags, void *stream);
/* Host copy of the last align result (pinned buffers owned by the batch) / the same as device pointers.  PGX_ERR_ARG when there is none. */
pgx_status pgx_batch_aligned(pgx_batch *b, pgx_read_aligns *out);
pgx_status pgx_batch_device_aligned(pgx_batch *b, pgx_read_aligns *out);
/* The same kernels on host arrays, with one candidate per read: text, seq_offsets, reads and read_offsets as in pgx_read_verify_arrays;
 * cand_seq[n_reads] / cand_diag[n_reads], PGX_NO_SEQUENCE meaning none, any other candidate allowed, a non-overlapping one included.  `out`
 * takes n_reads records; with PGX_ALIGN_CIGAR op_offsets takes n_reads + 1 entries and ops up to ops_cap words (PGX_ERR_NOMEM with the needed
 * count when there are more; both may be NULL without the flag).  The argument checks are those of pgx_read_verify_arrays (PGX_ERR_ARG with
 * nothing written: an unknown flag, band > 31, offsets that do not start at 0 or decrease, a cand_seq that is neither below n_seq nor
 * PGX_NO_SEQUENCE, the first offending read named).  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_align_arrays(int device, const uint8_t *text, const uint64_t *seq_offsets, uint64_t n_seq, const uint8_t *reads,
                                 const uint64_t *read_offsets, uint64_t n_reads, const uint32_t *cand_seq, const int64_t *cand_diag, uint32_t band,
                                 uint32_t flags, pgx_read_align *out, uint64_t *op_offsets, uint32_t *ops, uint64_t ops_cap);

/* ---- read walk: every aligned read as a walk through the graph, on the device ------------------------------------------------------
 * The align stage ends on one indexed sequence, that is on one haplotype: "sequence 37, [81 244, 81 394)".  The tag array exists to turn the
 * index's rows into graph positions, and a path covers whole nodes, so the graph walk of a text stretch is a slice of its sequence's node
 * list.  That list is recovered from the index and its tags alone (the WALK image, csrc/pgx_image.h; no graph file is read): a text position
 * is MARKED iff its tag -- the tag of the run that truly holds its row, not the item the reference's query reads when f % 10 == 0 -- has
 * offset 0, i.e. a node visit starts there.  Reads that verify left tied between haplotypes that agree over the read have one and the same walk.
 *
 * DEFINITIONS.  Within sequence seq of Ls symbols the marks are m_0 = 0 < m_1 < ...; visit k covers [m_k, m_k+1), the last one [m_k, Ls), and
 * its node is node << 1 | rev of the tag at m_k.  A node has at most 1024 symbols (the tag's offset has ten bits).  For a read whose align
 * record has (seq, text_start, text_end) with text_end > text_start:
 *   steps        the visits that meet [text_start, text_end): k0 = the last mark <= text_start to k1 = the last mark < text_end, both inclusive
 *   n_steps      k1 - k0 + 1
 *   path_start   text_start - m_k0: where the stretch starts on the concatenated nodes of its steps
 *   path_end     path_start + (text_end - text_start)
 *   path_len     (end of visit k1) - m_k0: the summed lengths of the steps' nodes, as GAF wants it
 * A read without a candidate (seq == PGX_NO_SEQUENCE) or with an empty stretch has n_steps = 0 and every other field 0; seq is kept.
 * pgx_read_walk (32 bytes, little endian):  0 path_len u64   8 path_start u64   16 path_end u64   24 n_steps u32   28 seq u32
 * PGX_WALK_STEPS adds step_offsets[n_reads + 1] and the steps (u64, node << 1 | rev) as a CSR list; n_steps is present either way.
 * The image is defined for any tag array whose sequences start on a mark, whether or not it describes paths (tags with offset 0 everywhere
 * make every position a visit of length 1); where two marks of one sequence lie more than 1024 positions apart the two bit scans stop at
 * 1024 and path_start / path_len are cut there.
 * The WALK image is built on the first call (pgx_index_paths or pgx_batch_read_walk) and lives with the index's device image: n / 8 bytes of
 * marks, n / 64 of rank directory, 8 bytes per visit.  PGX_ERR_UNSUPPORTED naming the reason: an index without tags or without an r-index
 * (PGX_ERR_ARG), a COMPAT index without N, an image file saved without the locate image or before the span of its tag runs was kept, a BWT
 * of 2^32 - 2^20 symbols or more.  PGX_ERR_FORMAT "the tags do not belong to this index", naming the sequence: the first position of some
 * non-empty sequence is not marked (or the runs cover fewer rows than the index has).  PGX_ERR_NOMEM with the bytes needed and free. */
#define PGX_WALK_STEPS 1u
typedef struct {
    uint64_t path_len, path_start, path_end;
    uint32_t n_steps, seq;
} pgx_read_walk;
typedef struct {
    uint64_t n_reads;
    uint64_t n_steps;               /* steps over all reads (with and without PGX_WALK_STEPS) */
    uint32_t flags;                 /* PGX_WALK_* the call ran with */
    uint32_t reserved;
    const pgx_read_walk *reads;     /* n_reads */
    const uint64_t *step_offsets;   /* n_reads + 1; NULL without PGX_WALK_STEPS */
    const uint64_t *steps;          /* n_steps; NULL without PGX_WALK_STEPS */
    float ms_walk;                  /* device time of the call when the run had PGX_RUN_TIMING, else 0 */
    uint32_t reserved2;
} pgx_read_walks;
/* Walks the reads of the last run along the stretches of the last pgx_batch_read_align, which must be this run's.  PGX_ERR_ARG with nothing
 * changed: no align result, an unknown flag.  Runs on `stream` (NULL = the batch's own), complete on return; one read-back, the number of
 * steps.  The result stays valid until the next run, upload, pgx_batch_read_walk or free of the batch; a later pgx_batch_locate of any
 * form leaves it valid.  The stage's buffers grow only and are its own. */
pgx_status pgx_batch_read_walk(pgx_batch *b, uint32_t flags, void *stream);
/* Host copy of the last walk result (pinned buffers owned by the batch) / the same as device pointers.  PGX_ERR_ARG when there is none. */
pgx_status pgx_batch_walked(pgx_batch *b, pgx_read_walks *out);
pgx_status pgx_batch_device_walked(pgx_batch *b, pgx_read_walks *out);
/* The recovered node list itself: path_offsets takes n_seq + 1 entries (n_seq_cap >= the index's sequence count, else PGX_ERR_ARG naming it),
 * sequence q's visits are [path_offsets[q], path_offsets[q + 1]).  path_nodes / visit_length (either may be NULL) take the visits' node << 1 | rev
 * and lengths when cap >= the number of visits; with both NULL the call only gives the counts, with cap too small it is PGX_ERR_NOMEM with the
 * number needed, path_offsets filled.  For tags made from a graph this is the graph's path table. */
pgx_status pgx_index_paths(pgx_index *h, int device, uint64_t *path_offsets, uint64_t n_seq_cap, uint64_t *path_nodes, uint32_t *visit_length, uint64_t cap);
/* The stage's count and fill kernels on stated path tables: sequence q is seq_offsets[q] .. seq_offsets[q + 1] (no endmarkers) and consists of
 * the visits [visit_offsets[q], visit_offsets[q + 1]) with nodes visit_nodes and lengths visit_length; read r walks [text_start[r], text_end[r])
 * of sequence seq[r] (PGX_NO_SEQUENCE: none).  `out` takes n_reads records; with PGX_WALK_STEPS step_offsets takes n_reads + 1 entries and steps
 * up to steps_cap (PGX_ERR_NOMEM with the needed count when there are more; both may be NULL without the flag).  PGX_ERR_ARG with nothing
 * written, naming the first offender: an unknown flag, offsets that do not start at 0 or decrease, a visit length of 0 or above 1024, lengths
 * that do not sum to their sequence's length, a stretch that ends behind its sequence or before its start, a seq that is neither below n_seq
 * nor PGX_NO_SEQUENCE.  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_walk_arrays(int device, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                const uint32_t *visit_length, uint64_t n_reads, const uint32_t *seq, const uint64_t *text_start, const uint64_t *text_end,
                                uint32_t flags, pgx_read_walk *out, uint64_t *step_offsets, uint64_t *steps, uint64_t steps_cap);

/* ---- read mapq: how far to trust the placement of every read, on the device ----------------------------------------------------------
 * Verify's n_tied counts haplotypes: a read that lies on eight haplotypes which agree over it has n_tied = 8 and one place in the graph.  This
 * stage counts competing graph LOCI instead, treats the neighbouring diagonals of one sequence (a read with an indel) as one place, looks one
 * coverage level below the candidates, and turns the evidence into a number from 0 to 60.  It sits behind verify (and rescue and mates where
 * they run) and changes none of their results.  Everything is integer arithmetic.
 *
 * DEFINITIONS for read r.
 *   entries      the candidates of r's verify list (PGX_VERIFY_LIST, possibly after a rescue merge) in list order, n_list of them, and behind
 *                them the EXTRAS: the first min(max_extra, 64 - n_list) placements of r with cov == next_score > 0 (next_score of the place
 *                record), in placement order, 0 <= max_extra <= 63.  The stage verifies the extras itself with the verify call's P; an extra's
 *                record is what verify writes at that (seq, diag).  Extras only compete: they never become candidates or winners, and the
 *                verify result is not touched.  With max_extra == 0 no place list is needed.  A read has at most 64 entries.
 *   chosen       the entry whose ordinal is the cand_index of r's winner record (possibly after an election, PGX_MATES_ELECT).  A read whose
 *                winner has seq == PGX_NO_SEQUENCE has no chosen entry: its record is 32 zero bytes.
 *   anchor       a = seg_start of the chosen entry, a read position.
 *   locus        of entry i: defined iff span_lo_i <= a < span_hi_i; then the pair (first step, path_start) that "read walk" gives for the
 *                stretch [diag_i + a, diag_i + a + 1) of seq_i: the oriented node that holds the text position under the anchor and the
 *                offset in it.  The 1024 cut of the walk's scans applies as it does there.
 *   classes      two entries are in one class iff both loci are defined and equal; an entry without a locus is a class of its own.
 *   adjacent     a class X other than the chosen's is adjacent iff some entry i of X and some entry j of the chosen's class have
 *                seq_i == seq_j and 0 < |diag_i - diag_j| <= slack (signed 64-bit), 0 <= slack <= 1024; slack == 0: no class is adjacent.
 *                Adjacent classes do not compete.  The classes that are neither the chosen's nor adjacent are the COMPETING classes.
 *   score        of entry i: s_i = seg_score_i.  With PGX_MAPQ_PAIRED reads 2k and 2k + 1 are mates and the score is s_i + m_i in signed 64
 *                bits, under frag_min, frag_max and U of the batch's mates result: m_i = 0 if the mate has no list candidate, else the larger of
 *                (1) the largest seg_score_j over the mate's LIST candidates j compatible with i in the sense of "read mates" and (2)
 *                solo_mate - U, solo_mate the seg_score of the mate's solo winner.  When the winners were elected under the same bounds and U,
 *                the chosen entry has the largest score of its list, PROPER or not, for any U >= 0: a PROPER pair (i*, j*) has s_i* + s_j* >=
 *                every compatible sum and >= solo_a + solo_b - U >= s_i + solo_b - U; without PROPER the chosen entry is the solo winner and
 *                every compatible sum lies below solo_a + solo_b - U.
 *   S_X, S_w, d_X   S_X is the largest score in class X, S_w the score of the chosen entry, d_X = max(0, S_w - S_X).  PGX_MAPQ_OUTSCORED: some
 *                competing class has S_X > S_w (possible through extras and in the arrays route).
 *   weights      T[k] = floor(65536 * 10^(-k / 10)), k = 0 .. 49 (PGX_MAPQ_T below).  A competing class weighs T[min(49, scale * d_X)], the
 *                product in 64 bits, 1 <= scale <= 16 decibels per score unit.  The default 2 makes a mismatch (P + 1 = 5 units at the
 *                default penalty) 10 dB: a model choice, not a measurement.
 *   excess       E = the sum of the weights of the competing classes.  If the chosen entry is the candidate a rescue merge appended (the
 *                read's rescue record has PGX_RESCUE_RESCUED, the verify result is merged and the chosen ordinal is the list's last), the
 *                diagonals of the rescue window compete with it: (n_best - 1) * 65536 is added, and T[min(49, scale * (seg_score -
 *                next_score))] when next_score > 0, all from the rescue record; PGX_MAPQ_RESCUED is set.  E is summed in 64 bits and stored
 *                held at 2^32 - 1.
 *   mapq         K[q] = floor(65536 * 10^(q / 10)), q = 0 .. 60 (PGX_MAPQ_K below).  mapq is the largest q in 0 .. 60 with
 *                E * K[q] <= (E + 65536) * 65536: 10 log10 of (all weight) / (competing weight), cut at 60.  E may be held at 2^26 in the
 *                comparison (mapq is 0 from E = 253 122 on, and no E, 2^26 included, makes the two sides equal: no K[q] - 65536 divides 2^32).  E = 0: 60; one exact tie (E = 65536): 3; two: 1; one competitor 10 / 20 dB
 *                down (E = 6553 / 655): 10 / 20; E = T[48] = 1: 48.
 * pgx_read_mapq (32 bytes, little endian, u32 each):
 *    0 mapq          4 flags
 *    8 n_entries     entries of the read                       12 n_loci        classes
 *   16 n_with        entries in the chosen's class or in an adjacent class
 *   20 n_competing   competing classes                         24 best_other    largest competing S_X held to [0, 2^32 - 1]; 0 without one
 *   28 excess        E held at 2^32 - 1
 * flags: PGX_MAPQ_HAS (a chosen entry), _LOCUS (the chosen's locus is defined), _PAIRED (the paired scores were used and the mate has a list
 * candidate), _RESCUED, _OUTSCORED, and _CAPPED: some competitors may be unseen -- the list holds at least the verify call's max_cand entries,
 * or (max_extra > 0) more next-level placements exist than extras were taken.  The arrays route never sets _CAPPED. */
#define PGX_MAPQ_PAIRED 4u     /* a flag of the call and a bit of pgx_read_mapq.flags */
#define PGX_MAPQ_HAS 1u        /* bits of pgx_read_mapq.flags */
#define PGX_MAPQ_LOCUS 2u
#define PGX_MAPQ_RESCUED 8u
#define PGX_MAPQ_CAPPED 16u
#define PGX_MAPQ_OUTSCORED 32u
#define PGX_MAPQ_MAX_ENTRIES 64u
#define PGX_MAPQ_MAX_SCALE 16u
#define PGX_MAPQ_MAX_SLACK 1024u
#define PGX_MAPQ_MAX_EXTRA 63u
#define PGX_MAPQ_NO_CHOSEN 0xFFFFFFFFu
#define PGX_MAPQ_T { \
    65536, 52057, 41350, 32845, 26090, 20724, 16461, 13076, 10386, 8250, \
    6553, 5205, 4135, 3284, 2609, 2072, 1646, 1307, 1038, 825, \
    655, 520, 413, 328, 260, 207, 164, 130, 103, 82, \
    65, 52, 41, 32, 26, 20, 16, 13, 10, 8, \
    6, 5, 4, 3, 2, 2, 1, 1, 1, 0 }
#define PGX_MAPQ_K { \
    65536, 82504, 103867, 130761, 164618, 207243, 260903, 328458, 413504, 520570, \
    655360, 825049, 1038675, 1307615, 1646189, 2072430, 2609035, 3284580, 4135042, 5205709, \
    6553600, 8250493, 10386756, 13076151, 16461898, 20724302, 26090351, 32845806, 41350420, 52057095, \
    65536000, 82504935, 103867560, 130761511, 164618989, 207243028, 260903515, 328458065, 413504205, 520570951, \
    655360000, 825049357, 1038675602, 1307615110, 1646189891, 2072430287, 2609035152, 3284580654, 4135042052, 5205709519, \
    6553600000, 8250493578, 10386756026, 13076151107, 16461898917, 20724302873, 26090351529, 32845806542, 41350420527, 52057095190, \
    65536000000 }
typedef struct {
    uint32_t mapq, flags, n_entries, n_loci, n_with, n_competing, best_other, excess;
} pgx_read_mapq;
typedef struct {
    uint64_t n_reads;
    uint64_t n_has, n_unique, n_capped, sum_mapq; /* reads with PGX_MAPQ_HAS, of them with E == 0, reads with PGX_MAPQ_CAPPED, the sum of mapq: summed on the device */
    uint64_t n_extras;              /* extras verified over all reads */
    uint32_t scale, slack, max_extra, flags; /* what the call ran with */
    const pgx_read_mapq *records;   /* n_reads */
    float ms_mapq;                  /* device time of the call when the run had PGX_RUN_TIMING, else 0 (the walk image's build is not in it) */
    uint32_t reserved;
} pgx_read_mapqs;
/* The mapping qualities of the reads of the last run from the list and the winners of the last pgx_batch_read_verify, which must be this run's
 * and made with PGX_VERIFY_LIST.  With max_extra > 0 it also needs a place result of this run made with PGX_PLACE_LIST; with PGX_MAPQ_PAIRED
 * a mates result made on the current verify result and an even read count.  The rescue terms are added when the batch holds a rescue result
 * whose merge made the current list (a merged list takes no further pgx_batch_read_rescue call, with or without PGX_RESCUE_MERGE, so that
 * result stays the batch's until the next verify call).  PGX_ERR_ARG with nothing changed, naming what was found: no such result, scale outside 1 .. 16,
 * slack > 1024, max_extra > 63, an unknown flag.  Builds the WALK image on first use, with the refusals of pgx_batch_read_walk.  A read takes
 * the smallest power of two of lanes that holds the longest entry list (PGX_MAPQ_LANES in the environment, read per call, 1 .. 64, raises it;
 * results never depend on it).  Runs on `stream` (NULL = the batch's own), complete on return.  Buffers grow only and are the stage's own: the
 * result stays valid until the next run, upload, pgx_batch_read_verify, pgx_batch_read_rescue, pgx_batch_read_mates, pgx_batch_read_mapq or
 * free of the batch; a later pgx_batch_locate of any form leaves it valid. */
pgx_status pgx_batch_read_mapq(pgx_batch *b, uint32_t scale, uint32_t slack, uint32_t max_extra, uint32_t flags, void *stream);
/* Host copy of the last mapq result (a pinned buffer owned by the batch) / the same as a device pointer.  PGX_ERR_ARG when there is none. */
pgx_status pgx_batch_mapqs(pgx_batch *b, pgx_read_mapqs *out);
pgx_status pgx_batch_device_mapqs(pgx_batch *b, pgx_read_mapqs *out);
/* The same kernel on stated tables (how shapes no index produces are tested): the path tables of pgx_read_walk_arrays; read r has the entries
 * [entry_offsets[r], entry_offsets[r + 1]), pgx_read_verify records of which seq, diag, span_lo, span_hi, seg_start, seg_score and matches are
 * read; chosen[r] is an ordinal or PGX_MAPQ_NO_CHOSEN; list_len[r] says how many leading entries are list candidates, the rest are extras
 * (NULL: all are list candidates); rescue (NULL: none) holds a pgx_read_rescue record per read, and a read whose record has PGX_RESCUE_RESCUED
 * and whose chosen entry is its last list candidate takes the rescue terms.  frag_min, frag_max and penalty (U) are read under
 * PGX_MAPQ_PAIRED only.  `out` takes n_reads records.  PGX_ERR_ARG with nothing written, the first offender named: whatever
 * pgx_read_walk_arrays and pgx_read_mates_arrays refuse for the same tables (offsets, visit lengths, under PGX_MAPQ_PAIRED frag_min > frag_max,
 * an odd n_seq and unequal twins), a seq >= n_seq, a span that leaves its sequence, more than 64 entries, a list_len above the entry count, a
 * chosen >= list_len, scale, slack or a flag outside their ranges, an odd n_reads under PGX_MAPQ_PAIRED.  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_mapq_arrays(int device, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                const uint32_t *visit_length, uint64_t n_reads, const uint64_t *entry_offsets, const pgx_read_verify *entries,
                                const uint32_t *chosen, const pgx_read_rescue *rescue, int64_t frag_min, int64_t frag_max, uint32_t penalty,
                                const uint32_t *list_len, uint32_t scale, uint32_t slack, uint32_t flags, pgx_read_mapq *out);

/* ---- read pack: how many reads cover every base of every node, accumulated over batches on the device ---------------------------------
 * Every stage above returns per-read records of one batch.  This one aggregates: a vector the size of the graph that stays on the device over a
 * whole run and comes down once.  It reads what pgx_batch_read_align left on the device (records and CIGAR operations), the WALK image and,
 * with a filter, the mapq records; no GAF line is written or parsed.
 *
 * DEFINITIONS.
 *   graph coordinates   The WALK image's visits are node << 1 | rev; visit k covers [m_k, m_k+1) cut at its sequence's end.  len[id] is the
 *                length of any visit of node id; every visit of one id must have the same length, else PGX_ERR_FORMAT "the tags do not
 *                describe whole-node paths", naming the smallest such id (a visit of more than 1024 symbols counts as such an id).  Ids that no
 *                visit names have len = 0; max_id is the largest id visited; n_nodes = max_id + 1 (0 without a visit).  base[id] is the exclusive
 *                prefix sum of len over 0 .. max_id and G = base[max_id + 1].  Graph base (id, o), o counted in the node's forward orientation,
 *                is g = base[id] + o.  A text position p inside visit k at distance d = p - m_k maps to o = d when rev = 0 and to
 *                o = len - 1 - d when rev = 1.  The table is dense in the id: no sort is needed, and max_id + 2 > 2^32 is PGX_ERR_UNSUPPORTED.
 *   a read is counted   iff its align record has seq != PGX_NO_SEQUENCE and text_end > text_start and it passes the filter: min_mapq == 0, or its
 *                pgx_read_mapq.mapq >= min_mapq.  (pgx_read_pack_arrays has no text_end: there it is text_start plus the text its
 *                operations consume, and keep[r] != 0 is the filter.)
 *   what it adds        its CIGAR is walked in read order with t = text_start: S and I consume no text; D consumes text and adds nothing; = and X
 *                consume text and add 1 to the coverage of every graph base under the positions they consume.  t ends on text_end.
 *   coverage            u32 per graph base, summed over every counted read of every added batch.  Sums are modulo 2^32: a base with more than
 *                2^32 - 1 reads is out of scope.
 *   summary             for every id with len > 0: covered = bases with coverage > 0, sum (u64), max.  Ids with len = 0 have all three 0.
 *   counters            reads counted; reads filtered out (placed, with text_end > text_start, and refused by the filter); bases added (the
 *                summed lengths of the = and X operations of the counted reads, which is sum(cov) while no base wraps).
 * The device keeps a difference array in the text image's coordinates (n + 1 i32, wrap-around arithmetic): a read adds +1 / -1 at the two ends
 * of every stretch of matched text, and pgx_pack_finish folds it once -- prefix sums per tile, every covered text position projected onto its
 * graph base -- and zeroes it.  Integer adds commute: the result depends on nothing but the set of counted reads, not on lane counts, streams,
 * the order of the batches or how the reads are cut into batches.
 * Device memory of a pack: 4 (n + 1) + 4 G + 12 (max_id + 2) bytes, and 16 (max_id + 1) more for the summary.
 * pgx_pack_create returns PGX_ERR_NOMEM with the bytes needed (G bounded by n, the summary included) and the bytes free before any of these
 * is allocated. */
typedef struct pgx_pack pgx_pack;
typedef struct {
    uint64_t n_nodes;               /* max_id + 1 */
    uint64_t n_bases;               /* G */
    uint64_t n_text;                /* n: the text image's positions (tdiff holds n + 1) */
    uint64_t reads_counted, reads_filtered, bases_added; /* over every pgx_pack_add so far, summed on the device */
    uint64_t n_projected;           /* text positions the folds so far projected onto the graph */
    const uint64_t *node_base;      /* n_nodes + 1 */
    const uint32_t *node_length;    /* n_nodes */
    const uint32_t *cov;            /* n_bases */
    const uint32_t *covered;        /* n_nodes */
    const uint64_t *sum;            /* n_nodes */
    const uint32_t *max;            /* n_nodes */
    double ms_add_total;            /* device time of the pgx_pack_add calls on batches run with PGX_RUN_TIMING, summed */
    float ms_fold;                  /* device time of the last fold and summary */
    float ms_table;                 /* device time of the node table's build in pgx_pack_create (the WALK image's build is not in it) */
} pgx_pack_result;
/* A pack of index h on one device.  Builds the WALK image on first use (every refusal of pgx_batch_read_walk carries over) and the node table. */
pgx_status pgx_pack_create(pgx_index *h, int device, pgx_pack **out);
void pgx_pack_free(pgx_pack *p);
/* Adds the reads of batch b.  Needs this run's align result made with PGX_ALIGN_CIGAR, on the pack's index and device, and with min_mapq > 0
 * this run's mapq result.  PGX_ERR_ARG with nothing added, naming what was found: no such result, another index or device, min_mapq > 60, an
 * unknown flag (there are none: flags must be 0).  Runs on `stream` (NULL = the batch's own), complete on return.  May be called from several
 * threads at once on different batches.  It changes nothing in the batch. */
pgx_status pgx_pack_add(pgx_pack *p, pgx_batch *b, uint32_t min_mapq, uint32_t flags, void *stream);
/* Folds what was added and downloads the result into pinned buffers owned by the pack (valid until the next finish or the free).  After the
 * fold the difference array is all zero and cov holds the total: finish may be called again and returns the same vector, and add may continue
 * after it.  Must not run concurrently with pgx_pack_add or another finish on the same pack. */
pgx_status pgx_pack_finish(pgx_pack *p, pgx_pack_result *out);
/* The result of the last pgx_pack_finish as device pointers.  PGX_ERR_ARG when there was none. */
pgx_status pgx_pack_device_result(pgx_pack *p, pgx_pack_result *out);
/* The same kernels on stated tables: the path tables of pgx_read_walk_arrays; read r lies on sequence seq[r] (PGX_NO_SEQUENCE: none) from
 * text_start[r] with the operations ops[op_offsets[r] .. op_offsets[r + 1]) (length << 4 | op, the codes of pgx_read_align); keep (NULL: every
 * read) is the filter.  *n_nodes and *n_bases are written first; node_base takes n_nodes + 1 entries, node_length / covered / sum / max n_nodes
 * each when nodes_cap >= n_nodes, cov n_bases when cov_cap >= n_bases: PGX_ERR_NOMEM with the needed counts otherwise, nothing else written.
 * counters takes the three counters.  PGX_ERR_ARG with nothing written, the first offender named: the argument checks of pgx_read_walk_arrays,
 * an operation code that is none of I D S = X, a seq that is neither below n_seq nor PGX_NO_SEQUENCE, a text_start behind its sequence, a
 * CIGAR whose text length leaves its sequence.  PGX_ERR_FORMAT for two visits of one id with different lengths.  PGX_ERR_NO_DEVICE without a GPU. */
pgx_status pgx_read_pack_arrays(int device, const uint64_t *seq_offsets, uint64_t n_seq, const uint64_t *visit_offsets, const uint64_t *visit_nodes,
                                const uint32_t *visit_length, uint64_t n_reads, const uint32_t *seq, const uint64_t *text_start, const uint64_t *op_offsets,
                                const uint32_t *ops, const uint8_t *keep, uint64_t *n_nodes, uint64_t *n_bases, uint64_t *node_base, uint32_t *node_length,
                                uint32_t *covered, uint64_t *sum, uint32_t *max, uint64_t nodes_cap, uint32_t *cov, uint64_t cov_cap, uint64_t *counters);

/* ---- compact result: the result of a run as a byte stream, encoded on the device, expanded on the host ---------------------
 * What pgx_batch_result downloads is six dense uint64 arrays (8 bytes per read, 48 per MEM, 8 per graph position), nearly all of
 * them zero bits.  The compact form carries the same values and is expanded to the same pgx_result; only it crosses the link.
 * Opt-in: pgx_batch_result and every other output keep their bytes.  Like them it replaces the reference's per-read result
 * vectors (std::vector<MEM> of find_all_mems, include/pangenome_index/algorithm.hpp:739-757, and the position sets of
 * TagArray::query_compressed_compact, src/tag_arrays.cpp:830-890), which never leave the process there.
 *
 * THE FORMAT (part of the ABI).  Every number is an unsigned LEB128 varint: seven bits per byte, low bits first, the high bit of
 * a byte says that another follows; a uint64 takes 1 to 10 bytes (the tenth is 0 or 1); the encoder always emits the shortest
 * form.  Reads are cut into blocks of PGX_COMPACT_BLOCK_READS = 64 consecutive reads: block k covers reads
 * [64 k, min(64 k + 64, n_reads)) and occupies bytes[block_offsets[k] .. block_offsets[k + 1]); n_blocks = ceil(n_reads / 64).
 * Each block is padded with zero bytes (fewer than 8) to a multiple of 8 bytes.  A block is three homogeneous sections without
 * separators:
 *   1. for each read of the block: its number of MEMs;
 *   2. for each MEM of the block, in result order: start, end - start, bwt_start, (uint64_t)size, and with PGX_COMPACT_TAGS also
 *      tag_run_count and the MEM's number of positions;
 *   3. with PGX_COMPACT_TAGS: for each MEM in order its positions, the first as it is, each following one as the difference to
 *      its predecessor.
 * All differences are taken modulo 2^64, so any values round-trip exactly (negative size, unsorted positions).  Three tables of
 * n_blocks + 1 entries go with the bytes: block_offsets, block_first_mem (= mem_offsets[min(64 k, n_reads)]) and block_first_pos
 * (= pos_offsets[block_first_mem[k]]; all zero without PGX_COMPACT_TAGS); with them every block expands independently.  The stream
 * is canonical: one result has one encoding (tests/compact_emu.py restates it in Python). */
#define PGX_COMPACT_BLOCK_READS 64u
#define PGX_COMPACT_TAGS 1u /* pgx_compact_result.flags: the MEMs carry tag_run_count and positions */
typedef struct {
    uint64_t n_reads, n_mems, n_positions, n_extensions, n_tag_overflow; /* as in pgx_result */
    uint32_t flags;       /* PGX_COMPACT_TAGS */
    uint32_t block_reads; /* PGX_COMPACT_BLOCK_READS */
    uint64_t n_blocks;
    uint64_t n_bytes;     /* = block_offsets[n_blocks] */
    const uint64_t *block_offsets;   /* n_blocks + 1 */
    const uint64_t *block_first_mem; /* n_blocks + 1 */
    const uint64_t *block_first_pos; /* n_blocks + 1 */
    const uint8_t *bytes;            /* n_bytes */
    float ms_encode;      /* device time of the two encode kernels and the scan between them; 0 unless the run had PGX_RUN_TIMING */
} pgx_compact_result;
/* In place of pgx_batch_result: encodes the result of the last run on the batch's own stream (a sizing kernel, the scan of the
 * block sizes, a fill kernel: one wave per block) and downloads the three tables and the bytes into pinned buffers owned by the
 * batch, which only ever grow.  The host waits once for the tables -- their last entry sizes the byte buffer -- and once for the
 * bytes.  Valid until the next run, upload or free of the batch.  PGX_COMPACT_TAGS is set exactly when the run had PGX_RUN_TAGS.
 * The device result is left untouched: pgx_batch_result, pgx_batch_device_result and pgx_batch_locate give the same bytes before
 * and after.  PGX_ERR_ARG without a completed run. */
pgx_status pgx_batch_result_compact(pgx_batch *b, pgx_compact_result *out);
/* Host only, no device: expands blocks [first_block, first_block + n_blocks) of c into caller arrays sized from c's counters
 * (mem_offsets n_reads + 1, mems n_mems, and with PGX_COMPACT_TAGS tag_run_counts n_mems, pos_offsets n_mems + 1, positions
 * n_positions; without it the three may be NULL and are not touched), every entry at its global index: what pgx_batch_result
 * would have delivered there.  The closing mem_offsets[n_reads] and pos_offsets[n_mems] are written by the call whose range ends
 * at c->n_blocks (with n_reads = 0 that is the call over no blocks).  Blocks are independent: callers thread it over block
 * ranges themselves.  It never reads outside bytes[0 .. n_bytes) and never writes outside the index ranges the block tables
 * give (all checked against the counters first).  PGX_ERR_FORMAT with a message naming the block for: a block that ends inside
 * a number or before its last one, a varint longer than 10 bytes, a tenth byte above 1, non-zero or excess padding, tables that
 * decrease or point beyond n_bytes / n_mems / n_positions, counts that disagree with the block tables.  What it wrote for
 * the blocks before the offending one stays.  PGX_ERR_ARG for a null array or a block range beyond c->n_blocks. */
pgx_status pgx_compact_expand(const pgx_compact_result *c, uint64_t first_block, uint64_t n_blocks, uint64_t *mem_offsets, pgx_mem *mems,
                              uint64_t *tag_run_counts, uint64_t *pos_offsets, uint64_t *positions);
/* Host only: the largest stream any result of these counts can take (every varint 10 bytes, 7 bytes of padding a block);
 * flags: PGX_COMPACT_TAGS. */
uint64_t pgx_compact_bound(uint64_t n_reads, uint64_t n_mems, uint64_t n_positions, uint32_t flags);
/* The encoder alone, on an arbitrary result held in host arrays (how it is tested on values no small index produces): uploads
 * in->mem_offsets / mems (and, exactly when in->pos_offsets is non-NULL, tag_run_counts / pos_offsets / positions) to `device`,
 * runs the same two kernels, downloads the stream into bytes[0 .. bytes_cap) and the tables (n_blocks + 1 entries each).
 * *n_bytes is always the size of the stream; PGX_ERR_NOMEM when it exceeds bytes_cap (nothing is written to bytes then, the tables
 * are).  PGX_ERR_ARG unless mem_offsets and pos_offsets start at 0, never decrease and end at n_mems / n_positions. */
pgx_status pgx_compact_encode(int device, const pgx_result *in, uint8_t *bytes, uint64_t bytes_cap, uint64_t *block_offsets,
                              uint64_t *block_first_mem, uint64_t *block_first_pos, uint64_t *n_bytes);

/* ---- text output: the find_mems CLI's stdout (and per-read stderr) bytes of a finished batch, written on the device -------------
 * In place of downloading the result arrays and turning them into decimal text on host threads (the find_mems CLI's format_range,
 * which restates the reference's prints: src/find_mems.cpp:115-118,138 and src/tag_arrays.cpp:885-889), the device writes the
 * bytes and the host only downloads and write()s them.  Opt-in: every other output keeps its bytes.
 *
 * THE TEXT.  For read i of the batch, with seq = first_seq + i + 1 (format_range is the definition; tests/text_emu.py restates it):
 *   "Seq: <seq>\n"
 *   per MEM m of the read, in result order:
 *     "MEM START: <start>, MEM END: <end> BWT START: <bwt_start> SIZE: <size>\n"            (size as int64, '-' for negatives)
 *     "Number of unique positions: <pos_offsets[m + 1] - pos_offsets[m]>\n"
 *     "<position>, " per position, then "\n"                                                 (an empty list is just "\n")
 *     with PGX_FORMAT_LOCATE_POSITIONS: "Occurrences: <size>\n", "<v / max_length>:<v % max_length>, " per value in stored order, "\n"
 *     with PGX_FORMAT_LOCATE_SEQS:      "Sequences: <count>\n", "<v>, " per value, "\n"
 *     either locate form, a MEM without values (loc_offsets[m + 1] == loc_offsets[m]): "Occurrences: <size> (not located)\n" "\n"
 *   "\n"
 * and on the stderr side "[find_all_mems] total mems=<count>\n" per read.  Numbers are shortest decimal (uint64: up to 20 digits).
 * read_offsets[i] .. read_offsets[i + 1] is the text of read i, so a caller may cut the text at any read. */
#define PGX_FORMAT_STDERR 1u           /* also the per-read "[find_all_mems] total mems=" lines */
#define PGX_FORMAT_LOCATE_POSITIONS 2u /* needs a completed pgx_batch_locate(flags = 0 [| PGX_LOCATE_CHAINS]) */
#define PGX_FORMAT_LOCATE_SEQS 4u      /* needs pgx_batch_locate(PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE) */
typedef struct {
    uint64_t first_seq;  /* reads before this batch: read i prints as first_seq + i + 1 */
    uint64_t max_length; /* PGX_FORMAT_LOCATE_POSITIONS: the divisor of the packed values; 0 = the index's own (pgx_batch_format only) */
    uint32_t flags;      /* PGX_FORMAT_* */
    uint32_t reserved;   /* must be 0 */
} pgx_format_params;
typedef struct {
    uint64_t n_reads, n_bytes, n_err_bytes;
    const uint64_t *read_offsets; /* n_reads + 1 */
    const char *text;             /* n_bytes, not NUL-terminated */
    const char *err_text;         /* n_err_bytes; NULL without PGX_FORMAT_STDERR */
    float ms_format;              /* device time of the call when the run had PGX_RUN_TIMING, else 0 */
} pgx_text;
/* The text of the last run (and, with a locate flag, of the last locate) of the batch.  Runs on the batch's own stream: a length pass
 * (one lane per position, per located value, per MEM, per read, and the scans between them), the download of read_offsets -- the host
 * waits for it once, its last entry sizes the text -- a fill pass, and the download of the text into pinned buffers owned by the batch,
 * which only ever grow.  Valid until the next run, upload, locate, format or free of the batch -- and beyond that: there are two sets
 * of those buffers and the calls alternate between them, nothing else writes to them, so what a call returned stays readable until the
 * next call but one (or the free of the batch).  A writer thread can write the text of one batch while the next is being formatted;
 * the find_mems CLI does so.  The device result is left untouched:
 * pgx_batch_result, pgx_batch_result_compact and pgx_batch_locate give the same bytes before and after.
 * There is no chunked mode: the whole text of the batch is held on the device and in pinned host memory at once (about 450 bytes per
 * read of 150 at the tested scales), so the caller bounds it by the number of reads it uploads per batch.
 * PGX_ERR_ARG: no completed run; a run without PGX_RUN_TAGS; both locate flags; a locate flag without a completed locate of exactly
 * the flags named above (a PGX_LOCATE_SEQ_SETS result never matches); an unknown flag; reserved != 0. */
pgx_status pgx_batch_format(pgx_batch *b, const pgx_format_params *p, pgx_text *out);
/* The same kernels on a result held in host arrays (how they are tested on values no small index produces), the counterpart of
 * pgx_compact_encode: uploads in->mem_offsets / mems / pos_offsets / positions (pos_offsets must be there: the text has the positions)
 * and, with a locate flag, loc->loc_offsets / values (loc->n_mems must equal in->n_mems) to `device`, formats, and downloads
 * read_offsets (n_reads + 1 entries), the text into text[0 .. text_cap) and, with PGX_FORMAT_STDERR, the stderr lines into
 * err_text[0 .. err_cap).  *n_bytes / *n_err_bytes are always the sizes needed; PGX_ERR_NOMEM when one exceeds its capacity (nothing is
 * written to text / err_text then, read_offsets is).  PGX_ERR_ARG, decided before the device is touched: a null argument, a locate flag
 * without loc, both locate flags, PGX_FORMAT_LOCATE_POSITIONS with max_length 0, reserved != 0, and offset arrays (mem_offsets,
 * pos_offsets, loc_offsets) that do not start at 0, decrease somewhere or do not end at the count of what they index. */
pgx_status pgx_format_result(int device, const pgx_result *in, const pgx_locations *loc, const pgx_format_params *p, char *text, uint64_t text_cap,
                             uint64_t *read_offsets, uint64_t *n_bytes, char *err_text, uint64_t err_cap, uint64_t *n_err_bytes);

/* Convenience: create + run + result in one call (what the find_mems CLI uses). */
pgx_status pgx_find_mems_batch(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets,
                               uint64_t n_reads, uint64_t min_len, uint64_t min_occ, uint32_t flags,
                               pgx_batch **batch_out, pgx_result *result_out);

/* The same with the reads sharded over several devices of the node (the unit that shards is the per-read loop of
 * src/find_mems.cpp:94-139): n_slices contiguous slices of the batch, slice i on devices[i] (a device may be named more than
 * once) with its own host thread, batch and stream; the index image is replicated, there is no collective.  first_read
 * (n_slices + 1 entries) receives the slice boundaries; results_out[i] / batches_out[i] are those of slice i: concatenated
 * in slice order they are bit-identical to the unsharded result.  Free every batch with pgx_batch_free. */
pgx_status pgx_find_mems_sharded(pgx_index *h, const int *devices, uint32_t n_slices, const uint8_t *reads, const uint64_t *offsets,
                                 uint64_t n_reads, uint64_t min_len, uint64_t min_occ, uint32_t flags, pgx_batch **batches_out,
                                 pgx_result *results_out, uint64_t *first_read);

/* ---- chromosome-sharded mode (BASELINE configs[4]): exchange of per-read MEM lists over RCCL ------------------
 * Every rank (one process per GPU) holds the indexes of some chromosomes ("shards"), searches ALL reads in each of them
 * (one pgx_batch per shard, same reads) and calls pgx_exchange_mems; every rank receives, for every read, the concatenation in
 * shard order of the per-shard MEM lists -- each list bit-exact with the reference run on that shard's index.  (This is not
 * the MEM set of a merged whole-genome index: maximality, BWT coordinates and min_occ are per shard.)  The per-read
 * offsets and the 32-byte records travel device to device: ncclAllGather of u32 offsets, then one ncclBroadcast per rank of
 * exactly that rank's record count (no padding), then a device kernel interleaves the records per read.  RCCL is loaded on
 * first use.  The communicator id comes from rank 0 (pgx_comm_unique_id) and reaches the other ranks by whatever
 * means the caller has (a file, MPI, torch.distributed's store ...). */
#define PGX_COMM_ID_BYTES 128
typedef struct pgx_comm pgx_comm;
pgx_status pgx_comm_unique_id(uint8_t id[PGX_COMM_ID_BYTES]);
pgx_status pgx_comm_init(const uint8_t id[PGX_COMM_ID_BYTES], int rank, int world, int device, pgx_comm **out);
void pgx_comm_free(pgx_comm *c);
typedef struct {
    uint64_t n_reads, n_mems;
    const uint64_t *mem_offsets;  /* n_reads + 1 (device) */
    const pgx_mem *mems;          /* n_mems (device): read by read, within a read shard by shard, within a shard discovery order */
    const uint32_t *shard_of_mem; /* n_mems (device) */
} pgx_exchange_result;
/* batches[k] holds the finished run of shard shard_ids[k] of THIS rank (n_local of them); owner_of_shard[c] (n_shards entries,
 * identical on every rank) names the rank that holds shard c.  Collective: every rank of the communicator calls it.  The
 * result lives in buffers of the communicator until its next exchange. */
pgx_status pgx_exchange_mems(pgx_comm *c, pgx_batch *const *batches, const uint32_t *shard_ids, uint32_t n_local,
                             const uint32_t *owner_of_shard, uint32_t n_shards, pgx_exchange_result *out);
/* The host-side plan of an exchange, as a function of its own (no device, no RCCL: the unit tests of the slot arithmetic call it on the
 * CPU tier).  owner_of_shard as above; gathered = what the metadata all-gather delivers: `world` rows of PGX_XCH_META_HEAD + max_local
 * u64 each -- {status, n_reads, n_shards, digest of owner_of_shard, max_local, MEMs of the rank's 1st, 2nd, ... shard (ascending shard id)}.
 * Outputs (caller-allocated): slot[n_shards] = row of shard c in the gathered offsets (owner * max_local + k for the owner's k-th shard),
 * rec_base[world + 1] = first record of every rank in the gathered record array, src_base[n_shards] = first record of every shard,
 * *n_reads = the number of reads every rank that owns a shard reports.  PGX_ERR_ARG when any rank reported a non-zero status, ranks
 * disagree on n_reads / n_shards / the owner table, or the gathered offsets would exceed PGX_XCH_MAX_OFFSET_BYTES (the caller must
 * then exchange its reads in chunks: at 100 M reads x 24 shards on 8 ranks the offsets alone are 9.6 GB; 16 M reads per call keep
 * them at 1.5 GB). */
#define PGX_XCH_META_HEAD 5u
#define PGX_XCH_MAX_OFFSET_BYTES (4ull << 30)
pgx_status pgx_exchange_plan(uint32_t world, const uint32_t *owner_of_shard, uint32_t n_shards, const uint64_t *gathered,
                             uint32_t *max_local, uint32_t *slot, uint64_t *rec_base, uint64_t *src_base, uint64_t *n_reads);
/* digest of an owner table as the metadata carries it (FNV-1a over the entries) */
uint64_t pgx_exchange_owner_digest(const uint32_t *owner_of_shard, uint32_t n_shards);
/* copy the last exchange's result to host arrays (any may be NULL) */
pgx_status pgx_exchange_download(pgx_comm *c, uint64_t *mem_offsets, pgx_mem *mems, uint32_t *shard_of_mem);

/* find_mems_function (include/pangenome_index/algorithm.hpp:653-736) for n independent (read, start) pairs: query i
 * evaluates the function on read read_of[i] at start position x[i] and reports the start position it returns (next_x),
 * whether it pushed a MEM (has_mem, mem[i]) and the extensions it performed (n_ext, may be NULL).  x[i] > length is
 * undefined in the reference (:658 wraps) and defined here as "return length".  The batch entry points above are the
 * product path; this one serves the compat header's per-call find_mems_function and tests of the state machine. */
pgx_status pgx_find_mems_function_batch(pgx_index *h, int device, const uint8_t *reads, const uint64_t *offsets, uint64_t n_reads,
                                        const uint64_t *read_of, const uint64_t *x, uint64_t n, uint64_t min_len, uint64_t min_occ,
                                        uint64_t *next_x, pgx_mem *mem, uint8_t *has_mem, uint64_t *n_ext);

/* device helpers */
pgx_status pgx_device_count(int *n);
pgx_status pgx_device_name(int device, char *buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif
