"""ctypes binding of libpgx.so (include/pgx.h) -- the test / bench harness side of the C ABI.

This module holds no algorithm: it only marshals numpy arrays across the C ABI.  The library has no
CPU fallback; every compute call needs a gfx950 device and raises PgxError otherwise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("PGX_LIB") or os.path.join(PKG_DIR, "libpgx.so")  # PGX_LIB: sanitizer build (scripts/asan_host.sh)

OK, ERR_IO, ERR_FORMAT, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_HIP, ERR_ARG, ERR_NOMEM = range(8)
MODE_COMPAT, MODE_STRICT = 0, 1
MODE_IMAGE_RL, MODE_IMAGE_DENSE, MODE_IMAGE_DENSE2, MODE_IMAGE_PAIRS = 0x100, 0x200, 0x400, 0x800  # or-ed into mode: force the layout of the device rank image
MODE_IMAGE_WIDE = 0x1000  # modifier: the 64-bit form of dense2 / pairs
IMAGE_RL, IMAGE_DENSE, IMAGE_DENSE2 = 0, 1, 2
TAGS_AUTO, TAGS_BYTECODE, TAGS_COMPACT = 0, 1, 2
RUN_TAGS, RUN_TIMING = 1, 2
READS_LINES, READS_FASTA, READS_FASTQ = 0, 1, 2  # pgx_batch_upload_text / pgx_fastx_cut: record rules in include/pgx.h

MEM_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("bwt_start", "<u8"), ("size", "<i8")])
BIINT_DTYPE = np.dtype([("forward", "<u8"), ("reverse", "<u8"), ("size", "<i8")])

u64, u32, p = C.c_uint64, C.c_uint32, C.c_void_p


class IndexInfo(C.Structure):
    _fields_ = [
        ("bwt_size", u64), ("sigma", u64), ("n_sequences", u64), ("n_ref_blocks", u64), ("n_runs", u64),
        ("n_dev_blocks", u64), ("dir_entries", u64), ("dir_shift", u32), ("is_encoded", u32), ("has_N", u32),
        ("mode", u32), ("has_tags", u32), ("tag_format", u32), ("n_tag_runs", u64), ("tag_dir_entries", u64),
        ("tag_dir_shift", u32), ("image_in_lds", u32), ("image_bytes", u64), ("tag_image_bytes", u64),
        ("ref_block_mean_bytes", C.c_double), ("max_length", u64), ("n_samples", u64), ("image_kind", u32), ("image_pairs", u32),
        ("image_wide", u32), ("pairs_stride", u32),
    ]


IMAGE_NO_LOCATE = 1  # pgx_index_save_image
IMAGE_VERIFY = 1     # pgx_index_open_image
IMAGE_MAX_SECTIONS = 64


class ImageSectionInfo(C.Structure):  # pgx_image_section_info
    _fields_ = [("id", u32), ("elem_size", u32), ("bytes", u64), ("offset", u64), ("sum", u64), ("name", C.c_char * 16)]


class ImageFileInfo(C.Structure):  # pgx_image_file_info
    _fields_ = [("version", u32), ("layout", u32), ("consts_bytes", u32), ("loc_consts_bytes", u32), ("mode", u32), ("has_rank", u32),
                ("has_tags", u32), ("n_sections", u32), ("meta_bytes", u32), ("flags", u32), ("header_sum", u64), ("file_bytes", u64),
                ("sections", ImageSectionInfo * IMAGE_MAX_SECTIONS)]


class Result(C.Structure):
    _fields_ = [
        ("n_reads", u64), ("n_mems", u64), ("mem_offsets", C.POINTER(u64)), ("mems", p),
        ("tag_run_counts", C.POINTER(u64)), ("pos_offsets", C.POINTER(u64)), ("positions", C.POINTER(u64)),
        ("n_positions", u64), ("n_extensions", u64), ("n_tag_overflow", u64),
    ]


class DeviceResult(C.Structure):
    _fields_ = [("n_reads", u64), ("n_mems", u64), ("n_positions", u64), ("mem_offsets", p), ("mems", p),
                ("tag_run_counts", p), ("pos_offsets", p), ("positions", p)]


class Locations(C.Structure):  # pgx_locations: host pointers (pgx_batch_locations) or device pointers (pgx_batch_device_locations)
    _fields_ = [("n_mems", u64), ("n_values", u64), ("n_not_located", u64), ("flags", u32), ("resident", u32), ("loc_offsets", p),
                ("values", p), ("ms_locate", C.c_float), ("set_words", C.c_uint32)]


class CompactResult(C.Structure):  # pgx_compact_result
    _fields_ = [("n_reads", u64), ("n_mems", u64), ("n_positions", u64), ("n_extensions", u64), ("n_tag_overflow", u64),
                ("flags", u32), ("block_reads", u32), ("n_blocks", u64), ("n_bytes", u64),
                ("block_offsets", C.POINTER(u64)), ("block_first_mem", C.POINTER(u64)), ("block_first_pos", C.POINTER(u64)),
                ("bytes", C.POINTER(C.c_uint8)), ("ms_encode", C.c_float)]


COMPACT_BLOCK_READS = 64
COMPACT_TAGS = 1  # pgx_compact_result.flags


class FormatParams(C.Structure):  # pgx_format_params
    _fields_ = [("first_seq", u64), ("max_length", u64), ("flags", u32), ("reserved", u32)]


class Text(C.Structure):  # pgx_text
    _fields_ = [("n_reads", u64), ("n_bytes", u64), ("n_err_bytes", u64), ("read_offsets", C.POINTER(u64)), ("text", p), ("err_text", p),
                ("ms_format", C.c_float)]


FORMAT_STDERR, FORMAT_LOCATE_POSITIONS, FORMAT_LOCATE_SEQS = 1, 2, 4  # pgx_format_params.flags

HITS_BEST_SETS, HITS_SCORES = 1, 2  # pgx_batch_read_hits / pgx_read_hits_arrays flags
NO_SEQUENCE = 0xFFFFFFFF            # pgx_read_hit.best_seq of a read without a located MEM
READ_HIT_DTYPE = np.dtype([("best_score", "<u8"), ("next_score", "<u8"), ("covered", "<u8"), ("best_seq", "<u4"), ("n_best", "<u4"),
                           ("n_located", "<u4"), ("n_mems", "<u4")])  # pgx_read_hit, 40 bytes


class ReadHits(C.Structure):  # pgx_read_hits: host pointers (pgx_batch_hits) or device pointers (pgx_batch_device_hits)
    _fields_ = [("n_reads", u64), ("n_seq", u64), ("set_words", u32), ("flags", u32), ("hits", p), ("best_sets", p), ("scores", p),
                ("ms_hits", C.c_float), ("reserved", u32)]


PLACE_LIST = 1  # pgx_batch_read_place / pgx_read_place_arrays flag
READ_PLACE_DTYPE = np.dtype([("best_score", "<u8"), ("next_score", "<u8"), ("best_diag", "<i8"), ("n_anchors", "<u8"), ("n_placements", "<u8"),
                             ("best_seq", "<u4"), ("n_best", "<u4"), ("best_mems", "<u4"), ("n_located", "<u4"), ("n_mems", "<u4"),
                             ("reserved", "<u4")])  # pgx_read_place, 64 bytes
PLACEMENT_DTYPE = np.dtype([("diag", "<i8"), ("score", "<u8"), ("seq", "<u4"), ("mems", "<u4")])  # pgx_placement, 24 bytes


class ReadPlace(C.Structure):  # pgx_read_place
    _fields_ = [("best_score", u64), ("next_score", u64), ("best_diag", C.c_int64), ("n_anchors", u64), ("n_placements", u64), ("best_seq", u32),
                ("n_best", u32), ("best_mems", u32), ("n_located", u32), ("n_mems", u32), ("reserved", u32)]


class Placement(C.Structure):  # pgx_placement
    _fields_ = [("diag", C.c_int64), ("score", u64), ("seq", u32), ("mems", u32)]


class ReadPlaces(C.Structure):  # pgx_read_places: host pointers (pgx_batch_places) or device pointers (pgx_batch_device_places)
    _fields_ = [("n_reads", u64), ("n_anchors", u64), ("n_places", u64), ("flags", u32), ("n_passes", u32), ("reads", p), ("place_offsets", p),
                ("places", p), ("ms_place", C.c_float), ("reserved", u32)]


VERIFY_LIST = 1  # pgx_batch_read_verify / pgx_read_verify_arrays flag
VERIFY_DTYPE = np.dtype([("diag", "<i8"), ("seq", "<u4"), ("n_cand", "<u4"), ("span_lo", "<u4"), ("span_hi", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"),
                         ("seg_start", "<u4"), ("seg_end", "<u4"), ("seg_score", "<u4"), ("seg_mismatches", "<u4"), ("longest_run", "<u4"), ("run_start", "<u4"),
                         ("cand_index", "<u4"), ("n_tied", "<u4")])  # pgx_read_verify, 64 bytes
assert VERIFY_DTYPE.itemsize == 64


class ReadVerifies(C.Structure):  # pgx_read_verifies: host pointers (pgx_batch_verified) or device pointers (pgx_batch_device_verified)
    _fields_ = [("n_reads", u64), ("n_cands", u64), ("flags", u32), ("max_cand", u32), ("mismatch_penalty", u32), ("reserved", u32), ("reads", p),
                ("cand_offsets", p), ("cands", p), ("ms_verify", C.c_float), ("reserved2", u32)]


MATES_ELECT = 1  # pgx_batch_read_mates / pgx_read_mates_arrays flag
MATES_PROPER, MATES_COMPATIBLE, MATES_HAS_A, MATES_HAS_B, MATES_MOVED_A, MATES_MOVED_B = 1, 2, 4, 8, 16, 32  # bits of a record's flags
MATES_DTYPE = np.dtype([("frag", "<i8"), ("pair_score", "<u4"), ("solo_score", "<u4"), ("cand_a", "<u4"), ("cand_b", "<u4"), ("solo_a", "<u4"), ("solo_b", "<u4"),
                        ("n_compatible", "<u4"), ("n_best", "<u4"), ("next_score", "<u4"), ("pair_matches", "<u4"), ("seq_a", "<u4"), ("seq_b", "<u4"),
                        ("flags", "<u4"), ("reserved", "<u4")])  # pgx_read_mates, 64 bytes
assert MATES_DTYPE.itemsize == 64


class ReadMatesResult(C.Structure):  # pgx_read_mates_result: a host pointer (pgx_batch_mated) or a device pointer (pgx_batch_device_mated)
    _fields_ = [("n_pairs", u64), ("n_proper", u64), ("n_compatible", u64), ("n_moved_a", u64), ("n_moved_b", u64), ("frag_min", C.c_int64), ("frag_max", C.c_int64),
                ("flags", u32), ("penalty", u32), ("pairs", p), ("ms_mates", C.c_float), ("reserved", u32)]


MAPQ_PAIRED = 4  # pgx_batch_read_mapq / pgx_read_mapq_arrays flag, and a bit of a record's flags
MAPQ_HAS, MAPQ_LOCUS, MAPQ_RESCUED, MAPQ_CAPPED, MAPQ_OUTSCORED = 1, 2, 8, 16, 32  # bits of a record's flags
MAPQ_MAX_ENTRIES, MAPQ_MAX_SCALE, MAPQ_MAX_SLACK, MAPQ_MAX_EXTRA, MAPQ_NO_CHOSEN = 64, 16, 1024, 63, 0xFFFFFFFF
MAPQ_DTYPE = np.dtype([("mapq", "<u4"), ("flags", "<u4"), ("n_entries", "<u4"), ("n_loci", "<u4"), ("n_with", "<u4"), ("n_competing", "<u4"), ("best_other", "<u4"),
                       ("excess", "<u4")])  # pgx_read_mapq, 32 bytes
assert MAPQ_DTYPE.itemsize == 32


class ReadMapqs(C.Structure):  # pgx_read_mapqs: a host pointer (pgx_batch_mapqs) or a device pointer (pgx_batch_device_mapqs)
    _fields_ = [("n_reads", u64), ("n_has", u64), ("n_unique", u64), ("n_capped", u64), ("sum_mapq", u64), ("n_extras", u64), ("scale", u32), ("slack", u32),
                ("max_extra", u32), ("flags", u32), ("records", p), ("ms_mapq", C.c_float), ("reserved", u32)]


RESCUE_MERGE = 1  # pgx_batch_read_rescue / pgx_read_rescue_arrays flag
RESCUE_TARGET, RESCUE_RESCUED, RESCUE_FULL = 1, 2, 4  # bits of a record's flags
RESCUE_MAX_ANCHORS, RESCUE_MAX_WINDOW = 8, 65536
RESCUE_DTYPE = np.dtype([("diag", "<i8"), ("n_diags", "<u8"), ("seq", "<u4"), ("flags", "<u4"), ("anchor", "<u4"), ("n_anchors", "<u4"), ("seg_score", "<u4"),
                         ("matches", "<u4"), ("n_best", "<u4"), ("next_score", "<u4"), ("reserved", "<u4", (4,))])  # pgx_read_rescue, 64 bytes
assert RESCUE_DTYPE.itemsize == 64


class ReadRescueResult(C.Structure):  # pgx_read_rescue_result: a host pointer (pgx_batch_rescued) or a device pointer (pgx_batch_device_rescued)
    _fields_ = [("n_reads", u64), ("n_targets", u64), ("n_rescued", u64), ("n_full", u64), ("n_tasks", u64), ("n_diags", u64), ("frag_min", C.c_int64),
                ("frag_max", C.c_int64), ("min_score", u32), ("max_anchors", u32), ("flags", u32), ("mismatch_penalty", u32), ("reads", p), ("ms_rescue", C.c_float),
                ("reserved", u32)]


ALIGN_CIGAR = 1  # pgx_batch_read_align / pgx_read_align_arrays flag
ALIGN_DTYPE = np.dtype([("diag", "<i8"), ("text_start", "<u8"), ("text_end", "<u8"), ("seq", "<u4"), ("clip_lo", "<u4"), ("clip_hi", "<u4"), ("edits", "<u4"),
                        ("n_match", "<u4"), ("n_mismatch", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("n_ops", "<u4"), ("band_hit", "<u4")])  # pgx_read_align, 64 bytes
assert ALIGN_DTYPE.itemsize == 64
ALIGN_OPS = {1: "I", 2: "D", 4: "S", 7: "=", 8: "X"}  # the BAM codes of an operation word (length << 4 | op)


def cigar_text(words):
    """3S70=1D76=1X from the operation words of a read"""
    return "".join("%d%s" % (int(x) >> 4, ALIGN_OPS[int(x) & 15]) for x in words)


class ReadAligns(C.Structure):  # pgx_read_aligns: host pointers (pgx_batch_aligned) or device pointers (pgx_batch_device_aligned)
    _fields_ = [("n_reads", u64), ("n_ops", u64), ("flags", u32), ("band", u32), ("passes", u32), ("reserved", u32), ("reads", p), ("op_offsets", p), ("ops", p),
                ("scratch_bytes", u64), ("ms_align", C.c_float), ("ms_forward", C.c_float), ("ms_trace", C.c_float), ("reserved2", u32)]


WALK_STEPS = 1  # pgx_batch_read_walk / pgx_read_walk_arrays flag
WALK_DTYPE = np.dtype([("path_len", "<u8"), ("path_start", "<u8"), ("path_end", "<u8"), ("n_steps", "<u4"), ("seq", "<u4")])  # pgx_read_walk, 32 bytes
assert WALK_DTYPE.itemsize == 32


class ReadWalks(C.Structure):  # pgx_read_walks: host pointers (pgx_batch_walked) or device pointers (pgx_batch_device_walked)
    _fields_ = [("n_reads", u64), ("n_steps", u64), ("flags", u32), ("reserved", u32), ("reads", p), ("step_offsets", p), ("steps", p), ("ms_walk", C.c_float),
                ("reserved2", u32)]


class PackResult(C.Structure):  # pgx_pack_result: host pointers (pgx_pack_finish) or device pointers (pgx_pack_device_result)
    _fields_ = [("n_nodes", u64), ("n_bases", u64), ("n_text", u64), ("reads_counted", u64), ("reads_filtered", u64), ("bases_added", u64), ("n_projected", u64),
                ("node_base", p), ("node_length", p), ("cov", p), ("covered", p), ("sum", p), ("max", p), ("ms_add_total", C.c_double), ("ms_fold", C.c_float),
                ("ms_table", C.c_float)]


class DeviceArray:
    """a device buffer owned by a batch, exposed through __cuda_array_interface__ (zero copy: torch.as_tensor(a, device="cuda"));
    64-bit unsigned values are presented as int64"""

    def __init__(self, ptr, shape, owner, typestr="<i8"):
        self.owner = owner  # keeps the batch alive
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr or 0), False), "version": 2, "strides": None}


class ExchangeResult(C.Structure):
    _fields_ = [("n_reads", u64), ("n_mems", u64), ("mem_offsets", p), ("mems", p), ("shard_of_mem", p)]


class ReadsInfo(C.Structure):  # pgx_reads_info
    _fields_ = [("n_reads", u64), ("n_bytes", u64), ("longest", u64)]


class Timing(C.Structure):
    _fields_ = [
        ("ms_find_mems", C.c_float), ("ms_compact", C.c_float), ("ms_tag_locate", C.c_float),
        ("ms_tag_gather", C.c_float), ("ms_tag_sort", C.c_float), ("ms_total", C.c_float),
        ("find_mems_launches", u32), ("heavy_reads", u32), ("pairs_reads", u32), ("pairs_other_steps", u32),
        ("ms_find_mems_main", C.c_float), ("seed_depth", u32),
        ("main_lines", u64), ("main_seed_loads", u64), ("other_lines", u64), ("other_seed_loads", u64), ("two_step_trips", u64),
        ("ms_per_upload", C.c_float), ("kernels", u32),
    ]


# pgx_timing.kernels (include/pgx.h PGX_KERNELS_*): the instances of pgx_find_mems_kernel / pgx_find_mems_pairs_kernel a run launched
KERNELS_FM, KERNELS_FM_SEEDED, KERNELS_FM_NARROW, KERNELS_FM_KIND_SHIFT, KERNELS_FM_LDS, KERNELS_FM_REDO = 0x1, 0x2, 0x4, 3, 0x20, 0x40
KERNELS_PAIRS, KERNELS_PAIRS_S64, KERNELS_PAIRS_COOP, KERNELS_PAIRS_PACKED, KERNELS_PAIRS_WIDE, KERNELS_PAIRS_LCE = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000
KERNELS_SIDE, KERNELS_HEAVY = 0x10000, 0x20000
KERNELS_FM_MASK, KERNELS_PAIRS_MASK = 0x3F, 0x3F00


def kernel_variants():
    """pgx_kernel_variants: every instance of the two kernels the runtime can launch, in the encoding of pgx_timing.kernels (host only)"""
    n = lib().pgx_kernel_variants(None, 0)
    out = np.zeros(n, dtype=np.uint32)
    assert lib().pgx_kernel_variants(out.ctypes.data, n) == n
    return [int(v) for v in out]


def _u64_array(ptr, n):
    """copy n uint64 from a (possibly NULL) ctypes pointer"""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=np.uint64)
    return np.ctypeslib.as_array(ptr, shape=(n,)).copy()


class PgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pgx status %d: %s" % (code, msg))
        self.code = code


_lib = None


def build():
    """Compile libpgx.so in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    subprocess.run(["make", "-C", PKG_DIR, "-s", "-j4"], check=True)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PgxError(ERR_NO_DEVICE, "libpgx.so is not built (run __graft_entry__.build()); there is no fallback")
    L = C.CDLL(LIB_PATH)
    L.pgx_last_error.restype = C.c_char_p
    L.pgx_abi_version.restype = C.c_int
    L.pgx_kernel_variants.argtypes = [p, u32]
    L.pgx_kernel_variants.restype = u32
    L.pgx_index_open.argtypes = [C.c_char_p, C.c_char_p, u32, u32, C.POINTER(p)]
    L.pgx_index_info_get.argtypes = [p, C.POINTER(IndexInfo)]
    L.pgx_index_close.argtypes = [p]
    L.pgx_index_close.restype = None
    L.pgx_index_to_device.argtypes = [p, C.c_int]
    L.pgx_index_image_view.argtypes = [p, C.c_int, C.POINTER(p), C.POINTER(u64)]
    L.pgx_index_tables.argtypes = [p, p, p, p]
    L.pgx_index_save_image.argtypes = [p, C.c_char_p, u32]
    L.pgx_index_open_image.argtypes = [C.c_char_p, u32, C.POINTER(p)]
    L.pgx_image_file_info.argtypes = [C.c_char_p, C.POINTER(ImageFileInfo)]
    L.pgx_image_sum.argtypes = [C.c_int, p, u64, C.POINTER(u64)]
    L.pgx_image_section_name.argtypes = [u32]
    L.pgx_image_section_name.restype = C.c_char_p
    L.pgx_build_rindex.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.pgx_build_rlbwt.argtypes = [C.c_char_p, C.c_char_p]
    L.pgx_build_index_from_text.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    L.pgx_build_index_from_text_device.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.pgx_build_index_from_texts_device.argtypes = [C.POINTER(C.c_char_p), u32, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.pgx_build_index_device_timing.argtypes = [p, u32]
    L.pgx_write_compact_tags.argtypes = [C.c_char_p, p, p, u64]
    L.pgx_convert_tags.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.pgx_tags_encode.argtypes = [C.c_int, p, p, u64, u64, u32, C.c_char_p]
    L.pgx_tags_encode_timing.argtypes = [p, u32]
    L.pgx_merge_tags.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), u32, p, u64, C.c_int, C.c_char_p]
    L.pgx_gbz_paths.argtypes = [C.c_char_p, C.POINTER(u64), p, p, u64, C.POINTER(u64), C.POINTER(u32)]
    L.pgx_merge_tags_gbz.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), u32, C.c_int, C.c_char_p]
    L.pgx_merge_tags_ex.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), u32, p, u64, C.c_int, C.c_char_p, u32]
    L.pgx_merge_tags_gbz_ex.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), u32, C.c_int, C.c_char_p, u32]
    L.pgx_build_tags.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, u32]
    L.pgx_build_tags_paths.argtypes = [C.c_char_p, u64, p, p, p, u64, u64, C.c_int, C.c_char_p, u32]
    L.pgx_build_tags_timing.argtypes = [p, u32]
    L.pgx_gbz_extract.argtypes = [C.c_char_p, C.c_char_p, u32]
    L.pgx_rank_batch.argtypes = [p, C.c_int, p, u64, C.c_int, p]
    L.pgx_extend_batch.argtypes = [p, C.c_int, p, p, p, u64, p]
    L.pgx_count_batch.argtypes = [p, C.c_int, p, p, u64, p]
    L.pgx_find_mems_function_batch.argtypes = [p, C.c_int, p, p, u64, p, p, u64, u64, u64, p, p, p, p]
    L.pgx_lf_batch.argtypes = [p, C.c_int, p, p, u64, p]
    L.pgx_tag_query_batch.argtypes = [p, C.c_int, p, p, u64, p, p, p, u64, C.POINTER(u64)]
    L.pgx_locate_batch.argtypes = [p, C.c_int, p, p, u64, u32, p, p, u64]
    L.pgx_locate_next_batch.argtypes = [p, C.c_int, p, u64, p]
    L.pgx_decompress_sa.argtypes = [p, C.c_int, u32, p]
    L.pgx_batch_create.argtypes = [p, C.c_int, p, p, u64, C.POINTER(p)]
    L.pgx_batch_upload.argtypes = [p, p, p, u64]
    L.pgx_batch_upload_packed.argtypes = [p, p, p, u64, p, p, u64]
    L.pgx_batch_upload_text.argtypes = [p, p, u64, u32, C.POINTER(u64)]
    L.pgx_batch_reads.argtypes = [p, C.POINTER(ReadsInfo), p, u64, p, u64]
    L.pgx_fastx_cut.argtypes = [p, u64, u32, u64, C.POINTER(u64)]
    L.pgx_pack_reads.argtypes = [p, p, u64, u32, p, p, u64, p, u64, C.POINTER(u64), C.POINTER(u64)]
    L.pgx_host_alloc.argtypes = [C.c_size_t, C.POINTER(p)]
    L.pgx_host_free.argtypes = [p]
    L.pgx_host_free.restype = None
    L.pgx_batch_run.argtypes = [p, u64, u64, u32, p]
    L.pgx_batch_result.argtypes = [p, C.POINTER(Result)]
    L.pgx_batch_counts.argtypes = [p, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.pgx_batch_device_result.argtypes = [p, C.POINTER(DeviceResult)]
    L.pgx_batch_timing.argtypes = [p, C.POINTER(Timing)]
    L.pgx_batch_spec_stats.argtypes = [p, C.POINTER(u32), C.POINTER(u32)]
    L.pgx_batch_locate.argtypes = [p, u32, u64, p]
    L.pgx_batch_locations.argtypes = [p, C.POINTER(Locations)]
    L.pgx_batch_device_locations.argtypes = [p, C.POINTER(Locations)]
    L.pgx_batch_read_hits.argtypes = [p, u32, p]
    L.pgx_batch_hits.argtypes = [p, C.POINTER(ReadHits)]
    L.pgx_batch_device_hits.argtypes = [p, C.POINTER(ReadHits)]
    L.pgx_read_hits_arrays.argtypes = [C.c_int, p, u64, p, p, u32, u64, u32, p, p, p]
    L.pgx_batch_read_place.argtypes = [p, u32, p]
    L.pgx_batch_places.argtypes = [p, C.POINTER(ReadPlaces)]
    L.pgx_batch_device_places.argtypes = [p, C.POINTER(ReadPlaces)]
    L.pgx_read_place_arrays.argtypes = [C.c_int, p, u64, p, p, p, u64, u64, u32, p, p, p, u64]
    L.pgx_index_text.argtypes = [p, C.c_int, p, u64, p, u64]
    L.pgx_batch_read_verify.argtypes = [p, u32, u32, u32, p]
    L.pgx_batch_verified.argtypes = [p, C.POINTER(ReadVerifies)]
    L.pgx_batch_device_verified.argtypes = [p, C.POINTER(ReadVerifies)]
    L.pgx_read_verify_arrays.argtypes = [C.c_int, p, p, u64, p, p, u64, p, p, p, u32, u32, p, p, p, u64]
    L.pgx_batch_read_align.argtypes = [p, u32, u32, p]
    L.pgx_batch_aligned.argtypes = [p, C.POINTER(ReadAligns)]
    L.pgx_batch_device_aligned.argtypes = [p, C.POINTER(ReadAligns)]
    L.pgx_read_align_arrays.argtypes = [C.c_int, p, p, u64, p, p, u64, p, p, u32, u32, p, p, p, u64]
    L.pgx_index_twinned.argtypes = [p, C.c_int, C.POINTER(u64)]
    L.pgx_batch_read_mates.argtypes = [p, C.c_int64, C.c_int64, u32, u32, p]
    L.pgx_batch_mated.argtypes = [p, C.POINTER(ReadMatesResult)]
    L.pgx_batch_device_mated.argtypes = [p, C.POINTER(ReadMatesResult)]
    L.pgx_read_mates_arrays.argtypes = [C.c_int, p, u64, u64, p, p, C.c_int64, C.c_int64, u32, u32, p, p]
    L.pgx_batch_read_mapq.argtypes = [p, u32, u32, u32, u32, p]
    L.pgx_batch_mapqs.argtypes = [p, C.POINTER(ReadMapqs)]
    L.pgx_batch_device_mapqs.argtypes = [p, C.POINTER(ReadMapqs)]
    L.pgx_read_mapq_arrays.argtypes = [C.c_int, p, u64, p, p, p, u64, p, p, p, p, C.c_int64, C.c_int64, u32, p, u32, u32, u32, p]
    L.pgx_batch_read_rescue.argtypes = [p, C.c_int64, C.c_int64, u32, u32, u32, p]
    L.pgx_batch_rescued.argtypes = [p, C.POINTER(ReadRescueResult)]
    L.pgx_batch_device_rescued.argtypes = [p, C.POINTER(ReadRescueResult)]
    L.pgx_read_rescue_arrays.argtypes = [C.c_int, p, p, u64, p, p, u64, p, p, C.c_int64, C.c_int64, u32, u32, u32, u32, p, p, p, u64, p]
    L.pgx_batch_read_walk.argtypes = [p, u32, p]
    L.pgx_batch_walked.argtypes = [p, C.POINTER(ReadWalks)]
    L.pgx_batch_device_walked.argtypes = [p, C.POINTER(ReadWalks)]
    L.pgx_index_paths.argtypes = [p, C.c_int, p, u64, p, p, u64]
    L.pgx_read_walk_arrays.argtypes = [C.c_int, p, u64, p, p, p, u64, p, p, p, u32, p, p, p, u64]
    L.pgx_pack_create.argtypes = [p, C.c_int, C.POINTER(p)]
    L.pgx_pack_free.argtypes = [p]
    L.pgx_pack_free.restype = None
    L.pgx_pack_add.argtypes = [p, p, u32, u32, p]
    L.pgx_pack_finish.argtypes = [p, C.POINTER(PackResult)]
    L.pgx_pack_device_result.argtypes = [p, C.POINTER(PackResult)]
    L.pgx_read_pack_arrays.argtypes = [C.c_int, p, u64, p, p, p, u64, p, p, p, p, p, p, p, p, p, p, p, p, u64, p, u64, p]
    L.pgx_batch_result_compact.argtypes = [p, C.POINTER(CompactResult)]
    L.pgx_compact_expand.argtypes = [C.POINTER(CompactResult), u64, u64, p, p, p, p, p]
    L.pgx_compact_bound.argtypes = [u64, u64, u64, u32]
    L.pgx_compact_bound.restype = u64
    L.pgx_compact_encode.argtypes = [C.c_int, C.POINTER(Result), p, u64, p, p, p, C.POINTER(u64)]
    L.pgx_batch_format.argtypes = [p, C.POINTER(FormatParams), C.POINTER(Text)]
    L.pgx_format_result.argtypes = [C.c_int, C.POINTER(Result), C.POINTER(Locations), C.POINTER(FormatParams), p, u64, p, C.POINTER(u64), p, u64, C.POINTER(u64)]
    L.pgx_batch_free.argtypes = [p]
    L.pgx_batch_free.restype = None
    L.pgx_find_mems_batch.argtypes = [p, C.c_int, p, p, u64, u64, u64, u32, C.POINTER(p), C.POINTER(Result)]
    L.pgx_find_mems_sharded.argtypes = [p, p, u32, p, p, u64, u64, u64, u32, p, p, p]
    L.pgx_comm_unique_id.argtypes = [p]
    L.pgx_comm_init.argtypes = [p, C.c_int, C.c_int, C.c_int, C.POINTER(p)]
    L.pgx_comm_free.argtypes = [p]
    L.pgx_comm_free.restype = None
    L.pgx_exchange_mems.argtypes = [p, p, p, u32, p, u32, C.POINTER(ExchangeResult)]
    L.pgx_exchange_download.argtypes = [p, p, p, p]
    L.pgx_device_count.argtypes = [C.POINTER(C.c_int)]
    L.pgx_device_name.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    _lib = L
    return L


def _check(st):
    if st != OK:
        raise PgxError(st, lib().pgx_last_error().decode(errors="replace"))


def device_count():
    n = C.c_int(0)
    _check(lib().pgx_device_count(C.byref(n)))
    return n.value


def device_name(device=0):
    buf = C.create_string_buffer(256)
    _check(lib().pgx_device_name(device, buf, 256))
    return buf.value.decode()


class _Pinned:
    """owner of one pgx_host_alloc block (freed with the last numpy view on it)"""

    def __init__(self, nbytes):
        self.ptr = p()
        _check(lib().pgx_host_alloc(max(int(nbytes), 16), C.byref(self.ptr)))
        self.nbytes = max(int(nbytes), 16)

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().pgx_host_free(self.ptr)
            self.ptr = None


def pinned_array(n, dtype):
    """numpy array of n items in pinned host memory (pgx_host_alloc): uploads from it and downloads into it run at link speed"""
    dt = np.dtype(dtype)
    own = _Pinned(int(n) * dt.itemsize)
    buf = (C.c_uint8 * own.nbytes).from_address(own.ptr.value)
    buf._pgx_owner = own  # (the array's base is this ctypes object: the block lives as long as any view on it)
    return np.frombuffer(buf, dtype=dt, count=int(n))


def pack_reads(reads_cat, offsets, packed_out, side_ids_out, side_bytes_out, threads=0):
    """pgx_pack_reads: the batch packed to two bits per symbol into packed_out (uint32[(bytes + 15) // 16]) and the reads with a byte outside
    A C G T listed (ids, their bytes concatenated) -> (n_side, n_side_bytes); PgxError(ERR_NOMEM) when the list does not fit"""
    reads_cat = np.ascontiguousarray(reads_cat, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    assert packed_out.dtype == np.uint32 and len(packed_out) >= (len(reads_cat) + 15) // 16
    ns, nb = u64(0), u64(0)
    _check(lib().pgx_pack_reads(reads_cat.ctypes.data if len(reads_cat) else None, offsets.ctypes.data, len(offsets) - 1, threads, packed_out.ctypes.data,
                                side_ids_out.ctypes.data, len(side_ids_out), side_bytes_out.ctypes.data, len(side_bytes_out), C.byref(ns), C.byref(nb)))
    return ns.value, nb.value


def _text_bytes(buf):
    """bytes / bytearray / uint8 array -> a contiguous uint8 array (no copy where there is one already)"""
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    return np.frombuffer(buf, dtype=np.uint8)


def fastx_cut(buf, fmt, want):
    """pgx_fastx_cut: the first record start at or after `want` (len(buf) if none).  Host only."""
    t = _text_bytes(buf)
    out = u64(0)
    _check(lib().pgx_fastx_cut(t.ctypes.data if len(t) else None, len(t), fmt, want, C.byref(out)))
    return out.value


def build_rindex(rlbwt_path, out_path, encoded=True):
    _check(lib().pgx_build_rindex(rlbwt_path.encode(), out_path.encode(), 1 if encoded else 0))


def build_rlbwt(text_path, out_path):
    _check(lib().pgx_build_rlbwt(text_path.encode(), out_path.encode()))


def build_index_from_text(text_path, out_rlbwt_path, out_ri_path, encoded=True):
    _check(lib().pgx_build_index_from_text(text_path.encode(), out_rlbwt_path.encode() if out_rlbwt_path else None, out_ri_path.encode(),
                                           1 if encoded else 0))


def build_index_from_texts(text_paths, out_rlbwt_path, out_ri_path, encoded=True):
    arr = (C.c_char_p * len(text_paths))(*[t.encode() for t in text_paths])
    _check(lib().pgx_build_index_from_texts(arr, len(text_paths), out_rlbwt_path.encode() if out_rlbwt_path else None, out_ri_path.encode(),
                                            1 if encoded else 0))


BUILD_INDEX_DEVICE_STAGES = ("upload", "first_sort", "doubling", "bwt_runs", "files", "rounds")  # ms, except rounds: a count


def build_index_from_text_device(text_path, out_rlbwt_path, out_ri_path, encoded=True, device=0):
    """pgx_build_index_from_text_device: the same two files as build_index_from_text, the suffix sorting on `device`; returns the stage values"""
    _check(lib().pgx_build_index_from_text_device(text_path.encode(), out_rlbwt_path.encode() if out_rlbwt_path else None, out_ri_path.encode(),
                                                  1 if encoded else 0, device))
    return build_index_device_timing()


def build_index_from_texts_device(text_paths, out_rlbwt_path, out_ri_path, encoded=True, device=0):
    arr = (C.c_char_p * len(text_paths))(*[t.encode() for t in text_paths])
    _check(lib().pgx_build_index_from_texts_device(arr, len(text_paths), out_rlbwt_path.encode() if out_rlbwt_path else None, out_ri_path.encode(),
                                                   1 if encoded else 0, device))
    return build_index_device_timing()


def build_index_device_timing():
    ms = (C.c_double * len(BUILD_INDEX_DEVICE_STAGES))()
    _check(lib().pgx_build_index_device_timing(C.cast(ms, C.c_void_p), len(BUILD_INDEX_DEVICE_STAGES)))
    return dict(zip(BUILD_INDEX_DEVICE_STAGES, list(ms)))


def write_compact_tags(out_path, values, lengths):
    v = np.ascontiguousarray(values, dtype=np.uint64)
    l = np.ascontiguousarray(lengths, dtype=np.uint64)
    assert len(v) == len(l)
    _check(lib().pgx_write_compact_tags(out_path.encode(), v.ctypes.data, l.ctypes.data, len(v)))


def convert_tags(in_path, out_path, compact=False):
    _check(lib().pgx_convert_tags(in_path.encode(), out_path.encode(), 1 if compact else 0))


TAGS_ENCODE_STAGES = ("pieces", "sd_vectors", "select", "download", "write", "file_bytes", "device_bytes")


def tags_encode(values, lengths, out_path, fmt, max_node_floor=0, device=0):
    """pgx_tags_encode: the query-format tag file (fmt = TAGS_COMPACT or TAGS_BYTECODE) of a run list, encoded on the device: the
    bytes write_compact_tags / convert_tags(compact=False) write for the same runs.  Returns tags_encode_timing()."""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    l = np.ascontiguousarray(lengths, dtype=np.uint64)
    assert len(v) == len(l)
    _check(lib().pgx_tags_encode(device, v.ctypes.data if len(v) else None, l.ctypes.data if len(l) else None, len(v), max_node_floor, fmt,
                                 out_path.encode()))
    return tags_encode_timing()


def tags_encode_timing():
    """this thread's last device encoding: stage times in ms, then the file's bytes and the encoder's peak device bytes"""
    ms = (C.c_double * len(TAGS_ENCODE_STAGES))()
    _check(lib().pgx_tags_encode_timing(C.cast(ms, C.c_void_p), len(TAGS_ENCODE_STAGES)))
    return dict(zip(TAGS_ENCODE_STAGES, list(ms)))


_VIEW_DTYPES = {0: np.uint8, 1: np.uint64, 2: np.uint64, 3: np.uint64, 4: np.uint64, 5: np.uint32, 6: np.uint8, 7: np.uint16,
                8: np.uint64, 9: np.uint64, 10: np.uint32, 11: np.uint64, 12: np.uint64, 13: np.uint32, 14: np.uint8, 15: np.uint32,
                16: np.uint64, 17: np.uint64, 18: np.uint64, 19: np.uint32, 20: np.uint32, 21: np.uint32, 22: np.uint64, 23: np.uint64}
LOCATE_SEQ_IDS, LOCATE_UNIQUE = 1, 2
LOCATE_CHAINS = 4  # pgx_batch_locate: the sample chains even where the suffix array is resident (tests)
LOCATE_SEQ_SETS = 8  # pgx_batch_locate: one bit per sequence per MEM, set_words words a MEM
NO_POSITION = 0xFFFFFFFFFFFFFFFF


MERGE_REFERENCE_RUNS = 0x1
MERGE_DEVICE_ENCODE = 0x10  # the output file is encoded on the device (pgx_tags_encode's kernels): the same bytes


def merge_tags(ri_path, tag_paths, seq_to_file, out_path, device=0, flags=0):
    """merge_tags: per-chromosome tag streams (algorithm format) -> whole-genome sdsl-compact tag array; seq_to_file[s] =
    index into tag_paths of the file that holds the tags of sequence s of the whole-genome r-index.  flags: MERGE_REFERENCE_RUNS
    writes run lengths as the reference does (mod 65 536)"""
    s2f = np.ascontiguousarray(seq_to_file, dtype=np.uint32)
    arr = (C.c_char_p * len(tag_paths))(*[t.encode() for t in tag_paths])
    _check(lib().pgx_merge_tags_ex(ri_path.encode(), arr, len(tag_paths), s2f.ctypes.data, len(s2f), device, out_path.encode(), flags))


def gbz_paths(gbz_path):
    """(first node id per GBWT sequence, its component, max node id, number of components) of a GBZ graph"""
    n, mx, nc = u64(0), u64(0), u32(0)
    _check(lib().pgx_gbz_paths(gbz_path.encode(), C.byref(n), None, None, 0, C.byref(mx), C.byref(nc)))
    first = np.zeros(n.value, dtype=np.uint64)
    comp = np.zeros(n.value, dtype=np.uint32)
    _check(lib().pgx_gbz_paths(gbz_path.encode(), C.byref(n), first.ctypes.data, comp.ctypes.data, n.value, C.byref(mx), C.byref(nc)))
    return first, comp, mx.value, nc.value


def merge_tags_gbz(gbz_path, ri_path, tag_paths, out_path, device=0, flags=0):
    """merge_tags with the reference's inputs: the sequence -> tag file map comes from the graph"""
    arr = (C.c_char_p * len(tag_paths))(*[t.encode() for t in tag_paths])
    _check(lib().pgx_merge_tags_gbz_ex(gbz_path.encode(), ri_path.encode(), arr, len(tag_paths), device, out_path.encode(), flags))


BUILD_TAGS_REFERENCE_RUNS, BUILD_TAGS_FORWARD_ONLY, BUILD_TAGS_INPUT_RLBWT = 0x1, 0x2, 0x4
# the output is a query format (what convert_tags makes of the default output), encoded on the device; one of them at most
BUILD_TAGS_OUT_COMPACT, BUILD_TAGS_OUT_BYTECODE = 0x8, 0x10
BUILD_TAGS_STAGES = ("graph", "index", "suffix_array", "tags", "runs", "write")


def build_tags(gbz_path, ri_path, out_path, device=0, flags=0):
    """build_tags: graph + r-index (or .rl_bwt with BUILD_TAGS_INPUT_RLBWT) -> tag array in build_tags' format.  flags:
    BUILD_TAGS_REFERENCE_RUNS (lengths mod 65 536 as the reference writes them), BUILD_TAGS_FORWARD_ONLY (index sequence s =
    GBWT sequence 2s).  Returns the stage times in ms (BUILD_TAGS_STAGES)."""
    _check(lib().pgx_build_tags(gbz_path.encode(), ri_path.encode(), device, out_path.encode(), flags))
    return build_tags_timing()


def build_tags_paths(ri_path, path_offsets, path_nodes, node_length, first_node_id, out_path, device=0, flags=0):
    """build_tags with the graph stated directly: path s = path_nodes[path_offsets[s]:path_offsets[s + 1]] (id << 1 | rev),
    node_length[id - first_node_id] (0: no such node).  Returns the stage times in ms."""
    po = np.ascontiguousarray(path_offsets, dtype=np.uint64)
    pn = np.ascontiguousarray(path_nodes, dtype=np.uint64)
    nl = np.ascontiguousarray(node_length, dtype=np.uint32)
    assert len(po) >= 1 and int(po[-1]) == len(pn)
    _check(lib().pgx_build_tags_paths(ri_path.encode(), len(po) - 1, po.ctypes.data, pn.ctypes.data if len(pn) else None,
                                      nl.ctypes.data if len(nl) else None, first_node_id, len(nl), device, out_path.encode(), flags))
    return build_tags_timing()


def build_tags_timing():
    ms = (C.c_double * len(BUILD_TAGS_STAGES))()
    _check(lib().pgx_build_tags_timing(C.cast(ms, C.c_void_p), len(BUILD_TAGS_STAGES)))
    return dict(zip(BUILD_TAGS_STAGES, list(ms)))


def gbz_extract(gbz_path, out_text_path, both=True):
    """newline-separated text of the graph's GBWT sequences (both=False: the even ones, the forward orientation)"""
    _check(lib().pgx_gbz_extract(gbz_path.encode(), out_text_path.encode(), 0 if both else BUILD_TAGS_FORWARD_ONLY))


def image_file_info(path):
    """header and section table of an image file (nothing is loaded): dict of the header fields + "sections", a list of dicts"""
    fi = ImageFileInfo()
    _check(lib().pgx_image_file_info(path.encode(), C.byref(fi)))
    out = {k: getattr(fi, k) for k, _ in ImageFileInfo._fields_ if k != "sections"}
    out["sections"] = [dict(id=s.id, elem_size=s.elem_size, bytes=s.bytes, offset=s.offset, sum=s.sum, name=s.name.decode())
                       for s in fi.sections[:fi.n_sections]]
    return out


def image_sum(data, device=-1):
    """the section sum of an image file over `data` (bytes or a numpy array); device < 0: on host threads, else on that device"""
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    out = u64(0)
    _check(lib().pgx_image_sum(device, C.c_void_p(a.ctypes.data) if a.size else None, a.size, C.byref(out)))
    return out.value


class Index:
    """FastLocate + TagArray behind the C ABI."""

    def __init__(self, ri_path, tags_path=None, tags_format=TAGS_AUTO, mode=MODE_COMPAT):
        self.L = lib()
        self.h = p()
        _check(self.L.pgx_index_open(ri_path.encode(), tags_path.encode() if tags_path else None, tags_format, mode,
                                     C.byref(self.h)))

    @classmethod
    def open_image(cls, path, verify=False):
        """a handle from an image file (save_image, the pgx_image CLI): no .ri, no tag file, nothing parsed or built on the host"""
        self = cls.__new__(cls)
        self.L = lib()
        self.h = p()
        _check(self.L.pgx_index_open_image(path.encode(), IMAGE_VERIFY if verify else 0, C.byref(self.h)))
        return self

    def save_image(self, path, no_locate=False):
        _check(self.L.pgx_index_save_image(self.h, path.encode(), IMAGE_NO_LOCATE if no_locate else 0))

    def tables(self):
        """(sym_map[256], C[8], complement[256]) of pgx_index_tables"""
        sm, cc, co = np.zeros(256, np.uint8), np.zeros(8, np.uint64), np.zeros(256, np.uint8)
        _check(self.L.pgx_index_tables(self.h, sm.ctypes.data, cc.ctypes.data, co.ctypes.data))
        return sm, cc, co

    def close(self):
        if getattr(self, "h", None):
            self.L.pgx_index_close(self.h)
            self.h = None

    __del__ = close

    def info(self):
        inf = IndexInfo()
        _check(self.L.pgx_index_info_get(self.h, C.byref(inf)))
        return inf

    def to_device(self, device=0):
        _check(self.L.pgx_index_to_device(self.h, device))

    def image_view(self, which):
        ptr, nbytes = p(), u64(0)
        _check(self.L.pgx_index_image_view(self.h, which, C.byref(ptr), C.byref(nbytes)))
        if nbytes.value == 0:
            return np.zeros(0, dtype=_VIEW_DTYPES[which])
        raw = C.string_at(ptr, nbytes.value)
        return np.frombuffer(raw, dtype=_VIEW_DTYPES[which]).copy()

    def device_view(self, which, device=0):
        """the device copy of image view `which` (0, 15, 20, 22, 23) as bytes"""
        host = self.image_view(which)
        out = np.zeros(host.nbytes, dtype=np.uint8)
        _check(self.L.pgx_index_device_view(self.h, device, which, C.c_void_p(out.ctypes.data), u64(host.nbytes)))
        return out.view(host.dtype)

    def text(self, device=0):
        """pgx_index_text: (seq_lengths uint64[n_sequences], the collection as bytes, every sequence followed by a newline), recovered on the
        device from the index alone (builds the text image on first use)"""
        inf = self.info()
        lens = np.zeros(int(inf.n_sequences), dtype=np.uint64)
        buf = np.zeros(int(inf.bwt_size), dtype=np.uint8)
        _check(self.L.pgx_index_text(self.h, device, lens.ctypes.data, len(lens), buf.ctypes.data, len(buf)))
        return lens, buf.tobytes()

    def twinned(self, device=0):
        """pgx_index_twinned: None when every sequence 2p has a twin 2p + 1 of its length (what read_mates needs), else the first p without"""
        bad = u64(0)
        _check(self.L.pgx_index_twinned(self.h, device, C.byref(bad)))
        return None if bad.value == 2 ** 64 - 1 else int(bad.value)

    def paths(self, device=0):
        """pgx_index_paths: (path_offsets uint64[n_sequences + 1], path_nodes uint64[V] as node << 1 | rev, visit_length uint32[V]): the node list of
        every sequence, recovered on the device from the index and its tags alone (builds the walk image on first use)"""
        offs = np.zeros(int(self.info().n_sequences) + 1, dtype=np.uint64)
        _check(self.L.pgx_index_paths(self.h, device, offs.ctypes.data, len(offs) - 1, None, None, 0))
        v = int(offs[-1])
        nodes, lens = np.zeros(max(v, 1), dtype=np.uint64), np.zeros(max(v, 1), dtype=np.uint32)
        _check(self.L.pgx_index_paths(self.h, device, offs.ctypes.data, len(offs) - 1, nodes.ctypes.data, lens.ctypes.data, v))
        return offs, nodes[:v], lens[:v]

    def lce_view(self, which, nbytes, device=0):
        """the device's LCE image (which = 30 suffix array, 31 text, 32 line flags, 33 common prefixes) as bytes; zeros where the index has none"""
        out = np.zeros(int(nbytes), dtype=np.uint8)
        _check(self.L.pgx_index_device_view(self.h, device, which, C.c_void_p(out.ctypes.data), u64(int(nbytes))))
        return out

    # ---- primitives -------------------------------------------------------------------------
    def rank_batch(self, pos, true_codes=False, device=0):
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        out = np.zeros((len(pos), 6), dtype=np.uint64)
        _check(self.L.pgx_rank_batch(self.h, device, pos.ctypes.data, len(pos), 1 if true_codes else 0, out.ctypes.data))
        return out

    def extend_batch(self, intervals, syms, forward, device=0):
        iv = np.ascontiguousarray(intervals, dtype=BIINT_DTYPE)
        sy = np.ascontiguousarray(syms, dtype=np.uint8)
        fw = np.ascontiguousarray(forward, dtype=np.uint8)
        out = np.zeros(len(iv), dtype=BIINT_DTYPE)
        _check(self.L.pgx_extend_batch(self.h, device, iv.ctypes.data, sy.ctypes.data, fw.ctypes.data, len(iv), out.ctypes.data))
        return out

    def count_batch(self, reads_cat, offsets, device=0):
        """FastLocate::count / count_encoded for every read -> uint64[n, 2] (first, second); empty = (1, 0)"""
        reads_cat = np.ascontiguousarray(reads_cat, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros((n, 2), dtype=np.uint64)
        _check(self.L.pgx_count_batch(self.h, device, reads_cat.ctypes.data if len(reads_cat) else None, offsets.ctypes.data, n,
                                      out.ctypes.data))
        return out

    def find_mems_function_batch(self, reads_cat, offsets, read_of, xs, min_len, min_occ, device=0):
        """find_mems_function (algorithm.hpp:653-736) for (read, start) pairs -> (next_x, mems, has_mem, n_ext)"""
        reads_cat = np.ascontiguousarray(reads_cat, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ro = np.ascontiguousarray(read_of, dtype=np.uint64)
        xv = np.ascontiguousarray(xs, dtype=np.uint64)
        n = len(ro)
        nx, ne = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        mems, has = np.zeros(n, dtype=MEM_DTYPE), np.zeros(n, dtype=np.uint8)
        _check(self.L.pgx_find_mems_function_batch(self.h, device, reads_cat.ctypes.data if len(reads_cat) else None, offsets.ctypes.data,
                                                   len(offsets) - 1, ro.ctypes.data, xv.ctypes.data, n, min_len, min_occ, nx.ctypes.data,
                                                   mems.ctypes.data, has.ctypes.data, ne.ctypes.data))
        return nx, mems, has, ne

    def lf_batch(self, ranges, syms, device=0):
        """FastLocate::LF / LF_encoded: uint64[n, 2] inclusive ranges, one symbol each -> uint64[n, 2]; empty = (1, 0)"""
        rg = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 2)
        sy = np.ascontiguousarray(syms, dtype=np.uint8)
        out = np.zeros((len(rg), 2), dtype=np.uint64)
        _check(self.L.pgx_lf_batch(self.h, device, rg.ctypes.data, sy.ctypes.data, len(rg), out.ctypes.data))
        return out

    def tag_query_batch(self, start, end, device=0):
        st = np.ascontiguousarray(start, dtype=np.uint64)
        en = np.ascontiguousarray(end, dtype=np.uint64)
        n = len(st)
        rn = np.zeros(n, dtype=np.uint64)
        po = np.zeros(n + 1, dtype=np.uint64)
        nover = u64(0)
        _check(self.L.pgx_tag_query_batch(self.h, device, st.ctypes.data, en.ctypes.data, n, rn.ctypes.data, po.ctypes.data,
                                          None, 0, C.byref(nover)))
        P = int(po[-1])
        pos = np.zeros(max(P, 1), dtype=np.uint64)
        _check(self.L.pgx_tag_query_batch(self.h, device, st.ctypes.data, en.ctypes.data, n, rn.ctypes.data, po.ctypes.data,
                                          pos.ctypes.data, len(pos), C.byref(nover)))
        return rn, po, pos[:P], nover.value

    def locate_batch(self, first, last, flags=0, device=0):
        """FastLocate::locate for n BWT ranges -> (offsets[n+1], values); flags: LOCATE_SEQ_IDS | LOCATE_UNIQUE"""
        fi = np.ascontiguousarray(first, dtype=np.uint64)
        la = np.ascontiguousarray(last, dtype=np.uint64)
        n = len(fi)
        off = np.zeros(n + 1, dtype=np.uint64)
        cap = int(np.sum(np.where(la >= fi, la - fi + np.uint64(1), np.uint64(0)))) if n else 0
        vals = np.zeros(max(cap, 1), dtype=np.uint64)
        _check(self.L.pgx_locate_batch(self.h, device, fi.ctypes.data, la.ctypes.data, n, flags, off.ctypes.data, vals.ctypes.data, cap))
        return off, vals[: int(off[-1])]

    def locate_next_batch(self, prev, device=0):
        pv = np.ascontiguousarray(prev, dtype=np.uint64)
        out = np.zeros(len(pv), dtype=np.uint64)
        _check(self.L.pgx_locate_next_batch(self.h, device, pv.ctypes.data, len(pv), out.ctypes.data))
        return out

    def decompress_sa(self, seq_ids=False, device=0):
        out = np.zeros(self.info().bwt_size, dtype=np.uint64)
        _check(self.L.pgx_decompress_sa(self.h, device, LOCATE_SEQ_IDS if seq_ids else 0, out.ctypes.data))
        return out

    # ---- hot path ---------------------------------------------------------------------------
    def batch(self, reads_cat, offsets, device=0):
        return Batch(self, reads_cat, offsets, device)

    def batch_empty(self, device=0):
        """a batch without reads yet (upload / upload_packed fill it)"""
        return Batch(self, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), device)

    def find_mems(self, reads_cat, offsets, min_len, min_occ, tags=False, device=0):
        b = Batch(self, reads_cat, offsets, device)
        try:
            b.run(min_len, min_occ, RUN_TAGS if tags else 0)
            return b.result()
        finally:
            b.free()

    def find_mems_text(self, buf, fmt, min_len, min_occ, tags=False, device=0):
        """find_mems over the records of a text (READS_LINES / READS_FASTA / READS_FASTQ), parsed on the device"""
        b = self.batch_empty(device)
        try:
            b.upload_text(buf, fmt)
            b.run(min_len, min_occ, RUN_TAGS if tags else 0)
            return b.result()
        finally:
            b.free()


def _result_dict(r):
    n, m = int(r.n_reads), int(r.n_mems)
    out = dict(n_extensions=int(r.n_extensions), n_tag_overflow=int(r.n_tag_overflow))
    out["mem_offsets"] = _u64_array(r.mem_offsets, n + 1)
    out["mems"] = (np.frombuffer(C.string_at(r.mems, m * 32), dtype=MEM_DTYPE).copy() if m else np.zeros(0, MEM_DTYPE))
    if r.pos_offsets:
        out["tag_run_counts"] = _u64_array(r.tag_run_counts, m)
        out["pos_offsets"] = _u64_array(r.pos_offsets, m + 1)
        out["positions"] = _u64_array(r.positions, int(r.n_positions))
    return out


_COMPACT_COUNTERS = ("n_reads", "n_mems", "n_positions", "n_extensions", "n_tag_overflow", "flags", "block_reads", "n_blocks", "n_bytes")


def _compact_struct(c):
    """the pgx_compact_result of a dict as Batch.result_compact() / compact_encode() return it, and the arrays it points into"""
    keep = [np.ascontiguousarray(c[k], dtype=np.uint64) for k in ("block_offsets", "block_first_mem", "block_first_pos")]
    keep.append(np.ascontiguousarray(c["bytes"], dtype=np.uint8))
    r = CompactResult()
    for k in _COMPACT_COUNTERS:
        setattr(r, k, int(c[k]))
    r.block_offsets, r.block_first_mem, r.block_first_pos = (C.cast(a.ctypes.data, C.POINTER(u64)) for a in keep[:3])
    r.bytes = C.cast(keep[3].ctypes.data, C.POINTER(C.c_uint8))
    return r, keep


def compact_expand_arrays(c):
    """empty arrays of the sizes a compact result expands to (what compact_expand fills; several calls over block ranges may share them)"""
    n, m = int(c["n_reads"]), int(c["n_mems"])
    out = dict(n_extensions=int(c["n_extensions"]), n_tag_overflow=int(c["n_tag_overflow"]))
    out["mem_offsets"] = np.zeros(n + 1, dtype=np.uint64)
    out["mems"] = np.zeros(m, dtype=MEM_DTYPE)
    if int(c["flags"]) & COMPACT_TAGS:
        out["tag_run_counts"] = np.zeros(m, dtype=np.uint64)
        out["pos_offsets"] = np.zeros(m + 1, dtype=np.uint64)
        out["positions"] = np.zeros(int(c["n_positions"]), dtype=np.uint64)
    return out


def compact_expand(c, first_block=0, n_blocks=None, out=None):
    """pgx_compact_expand (host only): blocks [first_block, first_block + n_blocks) of a compact result (all from first_block on by default)
    into the dict Batch.result() returns; entries of other blocks stay as they are in `out` (zero in a fresh one)"""
    r, keep = _compact_struct(c)
    if n_blocks is None:
        n_blocks = int(c["n_blocks"]) - first_block
    if out is None:
        out = compact_expand_arrays(c)
    tags = "pos_offsets" in out
    _check(lib().pgx_compact_expand(C.byref(r), first_block, n_blocks, out["mem_offsets"].ctypes.data, out["mems"].ctypes.data,
                                    out["tag_run_counts"].ctypes.data if tags else None, out["pos_offsets"].ctypes.data if tags else None,
                                    out["positions"].ctypes.data if tags else None))
    del keep
    return out


def compact_bound(n_reads, n_mems, n_positions, flags=0):
    return int(lib().pgx_compact_bound(n_reads, n_mems, n_positions, flags))


def compact_encode(device, result, bytes_cap=None):
    """pgx_compact_encode: the device encoder on a result dict (mem_offsets, mems and, for the tagged form, tag_run_counts / pos_offsets /
    positions); returns the dict Batch.result_compact() returns.  bytes_cap: size of the byte buffer handed over (default: the bound)"""
    mo = np.ascontiguousarray(result["mem_offsets"], dtype=np.uint64)
    mems = np.ascontiguousarray(result["mems"], dtype=MEM_DTYPE)
    n, m = len(mo) - 1, len(mems)
    r = Result()
    r.n_reads, r.n_mems = n, m
    r.mem_offsets = C.cast(mo.ctypes.data, C.POINTER(u64))
    r.mems = mems.ctypes.data
    tags = "pos_offsets" in result
    keep = [mo, mems]
    npos = 0
    if tags:
        for k in ("tag_run_counts", "pos_offsets", "positions"):
            a = np.ascontiguousarray(result[k], dtype=np.uint64)
            keep.append(a)
            setattr(r, k, C.cast(a.ctypes.data, C.POINTER(u64)))
        npos = len(keep[-1])
        r.n_positions = npos
    nb = (n + COMPACT_BLOCK_READS - 1) // COMPACT_BLOCK_READS
    flags = COMPACT_TAGS if tags else 0
    cap = compact_bound(n, m, npos, flags) if bytes_cap is None else int(bytes_cap)
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    tabs = [np.zeros(nb + 1, dtype=np.uint64) for _ in range(3)]
    nbytes = u64(0)
    st = lib().pgx_compact_encode(device, C.byref(r), buf.ctypes.data, cap, tabs[0].ctypes.data, tabs[1].ctypes.data, tabs[2].ctypes.data, C.byref(nbytes))
    if st != OK:
        e = PgxError(st, lib().pgx_last_error().decode(errors="replace"))
        e.n_bytes = int(nbytes.value)  # (ERR_NOMEM: what the stream needs)
        raise e
    return dict(n_reads=n, n_mems=m, n_positions=npos, n_extensions=int(result.get("n_extensions", 0)), n_tag_overflow=int(result.get("n_tag_overflow", 0)),
                flags=flags, block_reads=COMPACT_BLOCK_READS, n_blocks=nb, n_bytes=int(nbytes.value), block_offsets=tabs[0], block_first_mem=tabs[1],
                block_first_pos=tabs[2], bytes=buf[:int(nbytes.value)].copy(), ms_encode=0.0)


def format_result(device, result, first_seq=0, flags=0, max_length=0, locations=None, text_cap=None, err_cap=None, guard=0, reserved=0):
    """pgx_format_result: the device formatter on a result dict (mem_offsets, mems, pos_offsets, positions) and, with a locate flag, a
    locations dict (loc_offsets, values); returns dict(n_bytes, n_err_bytes, read_offsets, text, err_text) with text / err_text as bytes
    (err_text None without FORMAT_STDERR).  text_cap / err_cap: the sizes of the buffers handed over (default: a first call sizes them);
    guard: bytes of 0xA5 kept behind each buffer, returned as text_guard / err_guard.  ERR_NOMEM raises with n_bytes, n_err_bytes,
    read_offsets and the untouched buffers (text_buf, err_buf) on the exception"""
    mo = np.ascontiguousarray(result["mem_offsets"], dtype=np.uint64)
    mems = np.ascontiguousarray(result["mems"], dtype=MEM_DTYPE)
    n, m = len(mo) - 1, len(mems)
    r = Result()
    r.n_reads, r.n_mems = n, m
    r.mem_offsets = C.cast(mo.ctypes.data, C.POINTER(u64))
    r.mems = mems.ctypes.data
    keep = [mo, mems]
    for k in ("pos_offsets", "positions"):
        if k in result:
            a = np.ascontiguousarray(result[k], dtype=np.uint64)
            keep.append(a)
            setattr(r, k, C.cast(a.ctypes.data, C.POINTER(u64)))
    r.n_positions = len(result["positions"]) if "positions" in result else 0
    loc = None
    if locations is not None:
        lo = np.ascontiguousarray(locations["loc_offsets"], dtype=np.uint64)
        lv = np.ascontiguousarray(locations["values"], dtype=np.uint64)
        keep += [lo, lv]
        loc = Locations()
        loc.n_mems, loc.n_values = int(locations.get("n_mems", len(lo) - 1)), len(lv)
        loc.loc_offsets, loc.values = lo.ctypes.data, lv.ctypes.data
    fp = FormatParams(first_seq, max_length, flags, reserved)
    ro = np.zeros(n + 1, dtype=np.uint64)
    nb, ne = u64(0), u64(0)
    L = lib()

    def call(tcap, ecap):
        tb = np.full(tcap + guard + 1, 0xA5, dtype=np.uint8)
        eb = np.full(ecap + guard + 1, 0xA5, dtype=np.uint8)
        st = L.pgx_format_result(device, C.byref(r), C.byref(loc) if loc is not None else None, C.byref(fp), tb.ctypes.data, tcap, ro.ctypes.data,
                                 C.byref(nb), eb.ctypes.data, ecap, C.byref(ne))
        return st, tb, eb

    if text_cap is None or err_cap is None:
        st, tb, eb = call(0, 0)  # sizes only (ERR_NOMEM unless the text is empty)
        if st not in (OK, ERR_NOMEM):
            _check(st)
        text_cap = int(nb.value) if text_cap is None else text_cap
        err_cap = int(ne.value) if err_cap is None else err_cap
    st, tb, eb = call(int(text_cap), int(err_cap))
    if st != OK:
        e = PgxError(st, L.pgx_last_error().decode(errors="replace"))
        e.n_bytes, e.n_err_bytes, e.read_offsets, e.text_buf, e.err_buf = int(nb.value), int(ne.value), ro, tb, eb
        raise e
    del keep
    nbv, nev = int(nb.value), int(ne.value)
    return dict(n_bytes=nbv, n_err_bytes=nev, read_offsets=ro, text=tb[:nbv].tobytes(), err_text=eb[:nev].tobytes() if flags & FORMAT_STDERR else None,
                text_guard=tb[nbv:], err_guard=eb[nev:])


def read_hits_arrays(device, mem_offsets, mems, sets, n_seq, flags=0, set_words=None, out=None):
    """pgx_read_hits_arrays: the read-hits kernels on host arrays (mem_offsets uint64[n_reads + 1], mems MEM_DTYPE, sets
    uint64[n_mems, W]): dict(hits READ_HIT_DTYPE[n_reads], best_sets uint64[n_reads, W] or None, scores uint32[n_reads, n_seq] or
    None).  set_words: W as handed to the library (default ceil(n_seq / 64)); out: a dict of arrays to write into (tests)"""
    mem_offsets = np.ascontiguousarray(mem_offsets, dtype=np.uint64)
    mems = np.ascontiguousarray(mems, dtype=MEM_DTYPE)
    sets = np.ascontiguousarray(sets, dtype=np.uint64)
    n = len(mem_offsets) - 1
    W = (int(n_seq) + 63) // 64 if set_words is None else int(set_words)
    res = out if out is not None else {}
    if "hits" not in res:
        res["hits"] = np.zeros(n, dtype=READ_HIT_DTYPE)
    if "best_sets" not in res:
        res["best_sets"] = np.zeros((n, max(W, 0)), dtype=np.uint64) if flags & HITS_BEST_SETS else None
    if "scores" not in res:
        res["scores"] = np.zeros((n, int(n_seq)), dtype=np.uint32) if flags & HITS_SCORES else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_hits_arrays(device, mem_offsets.ctypes.data, n, mems.ctypes.data, sets.ctypes.data, W, int(n_seq), flags,
                                      ptr(res["hits"]), ptr(res["best_sets"]), ptr(res["scores"])))
    return res


def read_place_arrays(device, mem_offsets, mems, loc_offsets, values, n_seq, max_length, flags=0, places_cap=None, out=None):
    """pgx_read_place_arrays: the read-placement kernels on host arrays (mem_offsets uint64[n_reads + 1], mems MEM_DTYPE, loc_offsets
    uint64[n_mems + 1], values uint64 packed positions): dict(reads READ_PLACE_DTYPE[n_reads], and with PLACE_LIST place_offsets
    uint64[n_reads + 1] and places PLACEMENT_DTYPE[place_offsets[-1]], else None).  places_cap: the capacity handed to the library
    (default: one placement a value, which always suffices); out: a dict of arrays to write into (tests)"""
    mem_offsets = np.ascontiguousarray(mem_offsets, dtype=np.uint64)
    mems = np.ascontiguousarray(mems, dtype=MEM_DTYPE)
    loc_offsets = np.ascontiguousarray(loc_offsets, dtype=np.uint64)
    values = np.ascontiguousarray(values, dtype=np.uint64)
    n = len(mem_offsets) - 1
    if len(mems) != int(mem_offsets[-1]) or len(loc_offsets) != len(mems) + 1 or len(values) != int(loc_offsets[-1]):
        raise ValueError("read_place_arrays: mems, loc_offsets and values must have mem_offsets[-1], that + 1 and loc_offsets[-1] entries")
    lst = bool(flags & PLACE_LIST)
    cap = len(values) if places_cap is None else int(places_cap)
    res = out if out is not None else {}
    if "reads" not in res:
        res["reads"] = np.zeros(n, dtype=READ_PLACE_DTYPE)
    if "place_offsets" not in res:
        res["place_offsets"] = np.zeros(n + 1, dtype=np.uint64) if lst else None
    if "places" not in res:
        res["places"] = np.zeros(max(cap, 1), dtype=PLACEMENT_DTYPE) if lst else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_place_arrays(device, mem_offsets.ctypes.data, n, mems.ctypes.data, loc_offsets.ctypes.data, values.ctypes.data, int(n_seq),
                                       int(max_length), flags, ptr(res["reads"]), ptr(res["place_offsets"]), ptr(res["places"]), cap))
    if lst and out is None:
        res["places"] = res["places"][: int(res["place_offsets"][-1])]
    return res


def read_verify_arrays(device, text, seq_offsets, reads, read_offsets, cand_offsets, cand_seq, cand_diag, penalty=4, flags=0, list_cap=None, out=None):
    """pgx_read_verify_arrays: the verify kernels on host arrays (text uint8, the sequences without endmarkers, with seq_offsets uint64[n_seq + 1];
    reads uint8 with read_offsets uint64[n_reads + 1]; the candidates of read r at [cand_offsets[r], cand_offsets[r + 1]) of cand_seq uint32 /
    cand_diag int64): dict(reads VERIFY_DTYPE[n_reads], and with VERIFY_LIST cand_offsets uint64[n_reads + 1] and cands VERIFY_DTYPE[n_cands], else
    None).  list_cap: the capacity handed to the library (default: the number of candidates); out: a dict of arrays to write into (tests)"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
    read_offsets = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    cand_offsets = np.ascontiguousarray(cand_offsets, dtype=np.uint64)
    cand_seq = np.ascontiguousarray(cand_seq, dtype=np.uint32)
    cand_diag = np.ascontiguousarray(cand_diag, dtype=np.int64)
    n, n_seq = len(read_offsets) - 1, len(seq_offsets) - 1
    if len(cand_offsets) != n + 1 or len(cand_seq) != len(cand_diag):
        raise ValueError("read_verify_arrays: cand_offsets must have len(read_offsets) entries, cand_seq and cand_diag the same length")
    lst = bool(flags & VERIFY_LIST)
    cap = len(cand_seq) if list_cap is None else int(list_cap)
    res = dict(out) if out else {}
    if "reads" not in res:
        res["reads"] = np.zeros(n, dtype=VERIFY_DTYPE)
    if "cand_offsets" not in res:
        res["cand_offsets"] = np.zeros(n + 1, dtype=np.uint64) if lst else None
    if "cands" not in res:
        res["cands"] = np.zeros(max(cap, 1), dtype=VERIFY_DTYPE) if lst else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_verify_arrays(device, text.ctypes.data, seq_offsets.ctypes.data, n_seq, reads.ctypes.data, read_offsets.ctypes.data, n, cand_offsets.ctypes.data,
                                        cand_seq.ctypes.data, cand_diag.ctypes.data, penalty, flags, ptr(res["reads"]), ptr(res["cand_offsets"]), ptr(res["cands"]), cap))
    if lst:
        res["cands"] = res["cands"][: int(res["cand_offsets"][-1])]
    return res


def read_rescue_arrays(device, text, seq_offsets, reads, read_offsets, cand_offsets, cands, frag_min, frag_max, penalty=4, min_score=1, max_anchors=2, flags=0,
                       list_cap=None, out=None):
    """pgx_read_rescue_arrays: the rescue kernels on host arrays (text, seq_offsets, reads, read_offsets as in read_verify_arrays; the list of read r at
    [cand_offsets[r], cand_offsets[r + 1]) of cands VERIFY_DTYPE): dict(reads RESCUE_DTYPE[n_reads], and with RESCUE_MERGE cand_offsets uint64[n_reads + 1],
    cands VERIFY_DTYPE (the merged list) and winners VERIFY_DTYPE[n_reads], else None).  list_cap: the capacity handed to the library (default: the list with
    one more entry a read); out: a dict of arrays to write into (tests)"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
    read_offsets = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    cand_offsets = np.ascontiguousarray(cand_offsets, dtype=np.uint64)
    cands = np.ascontiguousarray(cands, dtype=VERIFY_DTYPE)
    n, n_seq = len(read_offsets) - 1, len(seq_offsets) - 1
    if len(cand_offsets) != n + 1:
        raise ValueError("read_rescue_arrays: cand_offsets must have len(read_offsets) entries")
    merge = bool(flags & RESCUE_MERGE)
    cap = len(cands) + n if list_cap is None else int(list_cap)
    res = dict(out) if out else {}
    if "reads" not in res:
        res["reads"] = np.zeros(n, dtype=RESCUE_DTYPE)
    if "cand_offsets" not in res:
        res["cand_offsets"] = np.zeros(n + 1, dtype=np.uint64) if merge else None
    if "cands" not in res:
        res["cands"] = np.zeros(max(cap, 1), dtype=VERIFY_DTYPE) if merge else None
    if "winners" not in res:
        res["winners"] = np.zeros(n, dtype=VERIFY_DTYPE) if merge else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_rescue_arrays(device, text.ctypes.data, seq_offsets.ctypes.data, n_seq, reads.ctypes.data, read_offsets.ctypes.data, n, cand_offsets.ctypes.data,
                                        cands.ctypes.data, frag_min, frag_max, penalty, min_score, max_anchors, flags, ptr(res["reads"]), ptr(res["cand_offsets"]),
                                        ptr(res["cands"]), cap, ptr(res["winners"])))
    if merge:
        res["cands"] = res["cands"][: int(res["cand_offsets"][-1])]
    return res


def read_mates_arrays(device, seq_lengths, cand_offsets, cands, frag_min, frag_max, penalty, flags=0, n_reads=None, out=None):
    """pgx_read_mates_arrays: the mates kernel on stated lists (seq_lengths uint64[n_seq]; the candidates of read r at [cand_offsets[r],
    cand_offsets[r + 1]) of cands VERIFY_DTYPE, of which seq, diag, seg_score and matches count): dict(pairs MATES_DTYPE[n_reads / 2], and with
    MATES_ELECT winners VERIFY_DTYPE[n_reads], else None).  n_reads: default len(cand_offsets) - 1; out: a dict of arrays to write into (tests)"""
    seq_lengths = np.ascontiguousarray(seq_lengths, dtype=np.uint64)
    cand_offsets = np.ascontiguousarray(cand_offsets, dtype=np.uint64)
    cands = np.ascontiguousarray(cands, dtype=VERIFY_DTYPE)
    n = len(cand_offsets) - 1 if n_reads is None else int(n_reads)
    res = dict(out) if out else {}
    if "pairs" not in res:
        res["pairs"] = np.zeros(n // 2, dtype=MATES_DTYPE)
    if "winners" not in res:
        res["winners"] = np.zeros(n, dtype=VERIFY_DTYPE) if flags & MATES_ELECT else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_mates_arrays(device, seq_lengths.ctypes.data, len(seq_lengths), n, cand_offsets.ctypes.data, cands.ctypes.data, frag_min, frag_max, penalty, flags,
                                       ptr(res["pairs"]), ptr(res["winners"])))
    return res


def read_mapq_arrays(device, seq_offsets, visit_offsets, visit_nodes, visit_length, entry_offsets, entries, chosen, rescue=None, frag_min=0, frag_max=0, penalty=0,
                     list_len=None, scale=2, slack=8, flags=0, n_reads=None, out=None):
    """pgx_read_mapq_arrays: the mapq kernel on stated tables (the path tables of read_walk_arrays; the entries of read r at [entry_offsets[r],
    entry_offsets[r + 1]) of entries VERIFY_DTYPE; chosen uint32[n_reads], MAPQ_NO_CHOSEN for none; rescue RESCUE_DTYPE[n_reads] or None; list_len
    uint32[n_reads] or None: every entry is a list candidate): MAPQ_DTYPE[n_reads].  n_reads: default len(entry_offsets) - 1; out: the array to write into"""
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
    visit_offsets = np.ascontiguousarray(visit_offsets, dtype=np.uint64)
    visit_nodes = np.ascontiguousarray(visit_nodes, dtype=np.uint64)
    visit_length = np.ascontiguousarray(visit_length, dtype=np.uint32)
    entry_offsets = np.ascontiguousarray(entry_offsets, dtype=np.uint64)
    entries = np.ascontiguousarray(entries, dtype=VERIFY_DTYPE)
    chosen = np.ascontiguousarray(chosen, dtype=np.uint32)
    rescue = None if rescue is None else np.ascontiguousarray(rescue, dtype=RESCUE_DTYPE)
    list_len = None if list_len is None else np.ascontiguousarray(list_len, dtype=np.uint32)
    n = len(entry_offsets) - 1 if n_reads is None else int(n_reads)
    if len(chosen) != n or (rescue is not None and len(rescue) != n) or (list_len is not None and len(list_len) != n):
        raise ValueError("read_mapq_arrays: chosen, rescue and list_len must have an entry per read")
    if len(visit_offsets) != len(seq_offsets):
        raise ValueError("read_mapq_arrays: visit_offsets must have len(seq_offsets) entries")
    res = np.zeros(n, dtype=MAPQ_DTYPE) if out is None else out
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_mapq_arrays(device, seq_offsets.ctypes.data, len(seq_offsets) - 1, visit_offsets.ctypes.data, visit_nodes.ctypes.data, visit_length.ctypes.data, n,
                                      entry_offsets.ctypes.data, entries.ctypes.data, chosen.ctypes.data, ptr(rescue), frag_min, frag_max, penalty, ptr(list_len), scale, slack,
                                      flags, res.ctypes.data))
    return res


def read_align_arrays(device, text, seq_offsets, reads, read_offsets, cand_seq, cand_diag, band=8, flags=0, ops_cap=None, out=None):
    """pgx_read_align_arrays: the align kernels on host arrays (text, seq_offsets, reads, read_offsets as in read_verify_arrays; one candidate per
    read, cand_seq uint32[n_reads] with NO_SEQUENCE 0xFFFFFFFF for none, cand_diag int64[n_reads]): dict(reads ALIGN_DTYPE[n_reads], and with
    ALIGN_CIGAR op_offsets uint64[n_reads + 1] and ops uint32[n_ops], else None).  ops_cap: the capacity handed to the library (default: enough for
    any alignment of these reads); out: a dict of arrays to write into (tests)"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
    read_offsets = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    cand_seq = np.ascontiguousarray(cand_seq, dtype=np.uint32)
    cand_diag = np.ascontiguousarray(cand_diag, dtype=np.int64)
    n, n_seq = len(read_offsets) - 1, len(seq_offsets) - 1
    if len(cand_seq) != n or len(cand_diag) != n:
        raise ValueError("read_align_arrays: cand_seq and cand_diag must have an entry per read")
    lst = bool(flags & ALIGN_CIGAR)
    cap = int(read_offsets[-1]) + 2 * int(band) * n + 2 * n if ops_cap is None else int(ops_cap)  # (a path holds at most len + 2 W moves and two clips)
    res = dict(out) if out else {}
    if "reads" not in res:
        res["reads"] = np.zeros(n, dtype=ALIGN_DTYPE)
    if "op_offsets" not in res:
        res["op_offsets"] = np.zeros(n + 1, dtype=np.uint64) if lst else None
    if "ops" not in res:
        res["ops"] = np.zeros(max(cap, 1), dtype=np.uint32) if lst else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_align_arrays(device, text.ctypes.data, seq_offsets.ctypes.data, n_seq, reads.ctypes.data, read_offsets.ctypes.data, n, cand_seq.ctypes.data,
                                       cand_diag.ctypes.data, band, flags, ptr(res["reads"]), ptr(res["op_offsets"]), ptr(res["ops"]), cap))
    if lst:
        res["ops"] = res["ops"][: int(res["op_offsets"][-1])]
    return res


def read_walk_arrays(device, seq_offsets, visit_offsets, visit_nodes, visit_length, seq, text_start, text_end, flags=0, steps_cap=None, out=None):
    """pgx_read_walk_arrays: the walk kernels on stated path tables (sequence q = the visits [visit_offsets[q], visit_offsets[q + 1]) with nodes
    visit_nodes uint64 and lengths visit_length uint32; read r = [text_start[r], text_end[r]) of sequence seq[r], NO_SEQUENCE 0xFFFFFFFF for none):
    dict(reads WALK_DTYPE[n_reads], and with WALK_STEPS step_offsets uint64[n_reads + 1] and steps uint64[n_steps], else None).  steps_cap: the
    capacity handed to the library (default: enough for any stretches on these tables); out: a dict of arrays to write into (tests)"""
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
    visit_offsets = np.ascontiguousarray(visit_offsets, dtype=np.uint64)
    visit_nodes = np.ascontiguousarray(visit_nodes, dtype=np.uint64)
    visit_length = np.ascontiguousarray(visit_length, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    text_start = np.ascontiguousarray(text_start, dtype=np.uint64)
    text_end = np.ascontiguousarray(text_end, dtype=np.uint64)
    n, n_seq = len(seq), len(seq_offsets) - 1
    if len(text_start) != n or len(text_end) != n or len(visit_offsets) != n_seq + 1 or len(visit_nodes) != len(visit_length):
        raise ValueError("read_walk_arrays: array lengths disagree")
    lst = bool(flags & WALK_STEPS)
    if steps_cap is None:  # (a stretch of L symbols meets at most L visits)
        cap = int(np.maximum(text_end.astype(np.int64) - text_start.astype(np.int64), 0).sum()) if n else 0
    else:
        cap = int(steps_cap)
    res = dict(out) if out else {}
    if "reads" not in res:
        res["reads"] = np.zeros(n, dtype=WALK_DTYPE)
    if "step_offsets" not in res:
        res["step_offsets"] = np.zeros(n + 1, dtype=np.uint64) if lst else None
    if "steps" not in res:
        res["steps"] = np.zeros(max(cap, 1), dtype=np.uint64) if lst else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_walk_arrays(device, seq_offsets.ctypes.data, n_seq, visit_offsets.ctypes.data, visit_nodes.ctypes.data, visit_length.ctypes.data, n,
                                      seq.ctypes.data, text_start.ctypes.data, text_end.ctypes.data, flags, ptr(res["reads"]), ptr(res["step_offsets"]),
                                      ptr(res["steps"]), cap))
    if lst:
        res["steps"] = res["steps"][: int(res["step_offsets"][-1])]
    return res


def read_pack_arrays(device, seq_offsets, visit_offsets, visit_nodes, visit_length, seq, text_start, op_offsets, ops, keep=None, nodes_cap=None, cov_cap=None, out=None):
    """pgx_read_pack_arrays: the pack kernels on stated path tables (those of read_walk_arrays); read r lies on sequence seq[r] (NO_SEQUENCE for none)
    from text_start[r] with the operations ops[op_offsets[r] : op_offsets[r + 1]] (uint32, length << 4 | op); keep uint8[n_reads] or None.
    dict(n_nodes, n_bases, node_base uint64[n_nodes + 1], node_length uint32, cov uint32[n_bases], covered uint32, sum uint64, max uint32,
    reads_counted, reads_filtered, bases_added).  nodes_cap / cov_cap: the capacities handed to the library (default: what these tables need);
    out: a dict of arrays to write into (tests)"""
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
    visit_offsets = np.ascontiguousarray(visit_offsets, dtype=np.uint64)
    visit_nodes = np.ascontiguousarray(visit_nodes, dtype=np.uint64)
    visit_length = np.ascontiguousarray(visit_length, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    text_start = np.ascontiguousarray(text_start, dtype=np.uint64)
    op_offsets = np.ascontiguousarray(op_offsets, dtype=np.uint64)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    n, n_seq = len(seq), len(seq_offsets) - 1
    if len(text_start) != n or len(op_offsets) != n + 1 or (keep is not None and len(keep) != n) or len(visit_offsets) != n_seq + 1 or len(visit_nodes) != len(visit_length):
        raise ValueError("read_pack_arrays: array lengths disagree")
    ncap = (int(visit_nodes.max() >> np.uint64(1)) + 1 if len(visit_nodes) else 0) if nodes_cap is None else int(nodes_cap)
    ccap = int(visit_length.astype(np.uint64).sum()) if cov_cap is None else int(cov_cap)  # (G is at most the text)
    res = dict(out) if out else {}
    for name, shape, dt in (("node_base", ncap + 1, np.uint64), ("node_length", max(ncap, 1), np.uint32), ("covered", max(ncap, 1), np.uint32), ("sum", max(ncap, 1), np.uint64),
                            ("max", max(ncap, 1), np.uint32), ("cov", max(ccap, 1), np.uint32), ("counters", 3, np.uint64)):
        if name not in res:
            res[name] = np.zeros(shape, dtype=dt)
    nn, nb = u64(0), u64(0)
    ptr = lambda a: a.ctypes.data if a is not None else None
    _check(lib().pgx_read_pack_arrays(device, seq_offsets.ctypes.data, n_seq, visit_offsets.ctypes.data, visit_nodes.ctypes.data, visit_length.ctypes.data, n, seq.ctypes.data,
                                      text_start.ctypes.data, op_offsets.ctypes.data, ops.ctypes.data, ptr(keep), C.addressof(nn), C.addressof(nb), ptr(res["node_base"]),
                                      ptr(res["node_length"]), ptr(res["covered"]), ptr(res["sum"]), ptr(res["max"]), ncap, ptr(res["cov"]), ccap, ptr(res["counters"])))
    k, g = int(nn.value), int(nb.value)
    c = res.pop("counters")
    res.update(n_nodes=k, n_bases=g, node_base=res["node_base"][: k + 1], node_length=res["node_length"][:k], covered=res["covered"][:k], sum=res["sum"][:k], max=res["max"][:k],
               cov=res["cov"][:g], reads_counted=int(c[0]), reads_filtered=int(c[1]), bases_added=int(c[2]))
    return res


class Pack:
    """pgx_pack: the coverage of every graph base, accumulated over the batches added to it (one index, one device)"""

    def __init__(self, index, device=0):
        self.L = lib()
        self.index = index  # keeps the index alive
        self.device = device
        self.p = p()
        _check(self.L.pgx_pack_create(index.h, device, C.byref(self.p)))

    def add(self, batch, min_mapq=0, flags=0, stream=None):
        """pgx_pack_add: the reads of the batch's align result (made with ALIGN_CIGAR); min_mapq > 0 reads its mapq result too"""
        _check(self.L.pgx_pack_add(self.p, batch.b if batch is not None else None, min_mapq, flags, stream))

    def _result(self, fn):
        r = PackResult()
        _check(fn(self.p, C.byref(r)))
        return r, dict(n_nodes=int(r.n_nodes), n_bases=int(r.n_bases), n_text=int(r.n_text), reads_counted=int(r.reads_counted), reads_filtered=int(r.reads_filtered),
                       bases_added=int(r.bases_added), n_projected=int(r.n_projected), ms_add_total=float(r.ms_add_total), ms_fold=float(r.ms_fold), ms_table=float(r.ms_table))

    def finish(self):
        """pgx_pack_finish as numpy arrays: node_base uint64[n_nodes + 1], node_length uint32[n_nodes], cov uint32[n_bases], covered uint32, sum uint64 and
        max uint32 per node, with n_nodes, n_bases, n_text, the counters and the times"""
        r, out = self._result(self.L.pgx_pack_finish)
        k, g = out["n_nodes"], out["n_bases"]
        view = lambda ptr, n, dt: np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt).copy() if n else np.zeros(0, dt)
        out.update(node_base=view(r.node_base, k + 1, np.uint64), node_length=view(r.node_length, k, np.uint32), cov=view(r.cov, g, np.uint32),
                   covered=view(r.covered, k, np.uint32), sum=view(r.sum, k, np.uint64), max=view(r.max, k, np.uint32))
        return out

    def device_result(self):
        """the last finish as device arrays (valid until the next finish / close)"""
        r, out = self._result(self.L.pgx_pack_device_result)
        k, g = out["n_nodes"], out["n_bases"]
        out.update(device=True, node_base=DeviceArray(r.node_base, (k + 1,), self), node_length=DeviceArray(r.node_length, (k,), self, "<u4"),
                   cov=DeviceArray(r.cov, (g,), self, "<u4"), covered=DeviceArray(r.covered, (k,), self, "<u4"), sum=DeviceArray(r.sum, (k,), self),
                   max=DeviceArray(r.max, (k,), self, "<u4"))
        return out

    def close(self):
        if getattr(self, "p", None):
            self.L.pgx_pack_free(self.p)
            self.p = None

    __del__ = close


def find_mems_sharded(index, devices, reads_cat, offsets, min_len, min_occ, tags=False):
    """pgx_find_mems_sharded: contiguous read slices, slice i on devices[i]; returns the per-slice result dicts in slice order"""
    reads_cat = np.ascontiguousarray(reads_cat, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    k = len(devices)
    dev = (C.c_int * k)(*devices)
    batches = (p * k)()
    results = (Result * k)()
    first = (u64 * (k + 1))()
    _check(index.L.pgx_find_mems_sharded(index.h, dev, k, reads_cat.ctypes.data if len(reads_cat) else None, offsets.ctypes.data,
                                         len(offsets) - 1, min_len, min_occ, RUN_TAGS if tags else 0, batches, results, first))
    try:
        return [_result_dict(results[i]) for i in range(k)], list(first)
    finally:
        for i in range(k):
            index.L.pgx_batch_free(batches[i])


COMM_ID_BYTES = 128


XCH_META_HEAD = 5
XCH_MAX_OFFSET_BYTES = 4 << 30


def exchange_owner_digest(owner_of_shard):
    L = lib()
    L.pgx_exchange_owner_digest.restype = u64
    own = (u32 * max(len(owner_of_shard), 1))(*owner_of_shard)
    return int(L.pgx_exchange_owner_digest(own, len(owner_of_shard)))


def exchange_plan(world, owner_of_shard, gathered):
    """pgx_exchange_plan (host only, no device): gathered = `world` metadata rows of XCH_META_HEAD + max_local u64 each.
    Returns dict(max_local, slot, rec_base, src_base, n_reads)."""
    L = lib()
    n = len(owner_of_shard)
    own = (u32 * max(n, 1))(*owner_of_shard)
    g = np.ascontiguousarray(gathered, dtype=np.uint64).reshape(-1)
    ml, nr = u32(0), u64(0)
    slot = np.zeros(n, dtype=np.uint32)
    rec_base = np.zeros(world + 1, dtype=np.uint64)
    src_base = np.zeros(n, dtype=np.uint64)
    _check(L.pgx_exchange_plan(u32(world), own, u32(n), C.c_void_p(g.ctypes.data), C.byref(ml), C.c_void_p(slot.ctypes.data),
                               C.c_void_p(rec_base.ctypes.data), C.c_void_p(src_base.ctypes.data), C.byref(nr)))
    return dict(max_local=int(ml.value), slot=slot, rec_base=rec_base, src_base=src_base, n_reads=int(nr.value))


def comm_unique_id():
    """ncclGetUniqueId through libpgx: rank 0 makes it, the other ranks receive the bytes out of band"""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().pgx_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """RCCL communicator of the chromosome-sharded exchange (pgx_comm): one per rank = per process = per GPU"""

    def __init__(self, uid, rank, world, device=0):
        self.L = lib()
        self.c = p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        _check(self.L.pgx_comm_init(buf, rank, world, device, C.byref(self.c)))

    def exchange(self, batches, owner_of_shard, download=True):
        """batches: {shard id: Batch (already run)} of this rank; owner_of_shard[c] = rank holding shard c.
        Returns (n_reads, n_mems) or, with download, (mem_offsets, mems, shard_of_mem) as host arrays."""
        ids = sorted(batches)
        k = len(ids)
        arr = (p * max(k, 1))(*[batches[c].b for c in ids])
        sid = (u32 * max(k, 1))(*ids)
        own = (u32 * len(owner_of_shard))(*owner_of_shard)
        r = ExchangeResult()
        _check(self.L.pgx_exchange_mems(self.c, arr, sid, k, own, len(owner_of_shard), C.byref(r)))
        if not download:
            return int(r.n_reads), int(r.n_mems)
        mo = np.zeros(int(r.n_reads) + 1, dtype=np.uint64)
        mems = np.zeros(int(r.n_mems), dtype=MEM_DTYPE)
        shard = np.zeros(int(r.n_mems), dtype=np.uint32)
        _check(self.L.pgx_exchange_download(self.c, mo.ctypes.data, mems.ctypes.data if len(mems) else None, shard.ctypes.data if len(shard) else None))
        return mo, mems, shard

    def free(self):
        if getattr(self, "c", None):
            self.L.pgx_comm_free(self.c)
            self.c = None

    __del__ = free


class Batch:
    def __init__(self, index, reads_cat, offsets, device=0):
        self.index = index
        self.L = index.L
        reads_cat = np.ascontiguousarray(reads_cat, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n = len(offsets) - 1
        self.b = p()
        _check(self.L.pgx_batch_create(index.h, device, reads_cat.ctypes.data if len(reads_cat) else None,
                                       offsets.ctypes.data, self.n, C.byref(self.b)))

    def upload_packed(self, packed, offsets, side_ids, side_bytes, n_side):
        """pgx_batch_upload_packed: the arrays pack_reads() filled (offsets[0] == 0)"""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert packed.dtype == np.uint32 and packed.flags.c_contiguous
        self.n = len(offsets) - 1
        _check(self.L.pgx_batch_upload_packed(self.b, packed.ctypes.data, offsets.ctypes.data, self.n, side_ids.ctypes.data if n_side else None,
                                              side_bytes.ctypes.data if n_side else None, n_side))

    def upload(self, reads_cat, offsets):
        reads_cat = np.ascontiguousarray(reads_cat, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n = len(offsets) - 1
        _check(self.L.pgx_batch_upload(self.b, reads_cat.ctypes.data if len(reads_cat) else None, offsets.ctypes.data, self.n))

    def upload_text(self, buf, fmt):
        """pgx_batch_upload_text: the records of `buf` become the reads; returns their number"""
        t = _text_bytes(buf)
        n = u64(0)
        _check(self.L.pgx_batch_upload_text(self.b, t.ctypes.data if len(t) else None, len(t), fmt, C.byref(n)))
        self.n = n.value
        return n.value

    def reads(self):
        """pgx_batch_reads: the reads as the batch holds them on its device -> (cat uint8, offs uint64 rebased to 0, longest read as recorded)"""
        info = ReadsInfo()
        _check(self.L.pgx_batch_reads(self.b, C.byref(info), None, 0, None, 0))
        offs = np.zeros(int(info.n_reads) + 1, dtype=np.uint64)
        cat = np.zeros(int(info.n_bytes), dtype=np.uint8)
        _check(self.L.pgx_batch_reads(self.b, C.byref(info), offs.ctypes.data, len(offs), cat.ctypes.data if len(cat) else None, len(cat)))
        return cat, offs, int(info.longest)

    def run(self, min_len, min_occ, flags=0, stream=None):
        _check(self.L.pgx_batch_run(self.b, min_len, min_occ, flags, stream))

    def counts(self):
        a, b_, c = u64(0), u64(0), u64(0)
        _check(self.L.pgx_batch_counts(self.b, C.byref(a), C.byref(b_), C.byref(c)))
        return a.value, b_.value, c.value

    def spec_stats(self):
        """(runs sized speculatively, of which repeated with exact sizes)"""
        a, f = u32(0), u32(0)
        _check(self.L.pgx_batch_spec_stats(self.b, C.byref(a), C.byref(f)))
        return a.value, f.value

    def timing(self):
        t = Timing()
        _check(self.L.pgx_batch_timing(self.b, C.byref(t)))
        return t

    def result(self):
        r = Result()
        _check(self.L.pgx_batch_result(self.b, C.byref(r)))
        n, m = int(r.n_reads), int(r.n_mems)
        out = dict(n_extensions=int(r.n_extensions), n_tag_overflow=int(r.n_tag_overflow))
        out["mem_offsets"] = _u64_array(r.mem_offsets, n + 1)
        out["mems"] = (np.frombuffer(C.string_at(r.mems, m * 32), dtype=MEM_DTYPE).copy() if m else np.zeros(0, MEM_DTYPE))
        if r.pos_offsets:
            out["tag_run_counts"] = _u64_array(r.tag_run_counts, m)
            out["pos_offsets"] = _u64_array(r.pos_offsets, m + 1)
            out["positions"] = _u64_array(r.positions, int(r.n_positions))
        return out

    def result_compact(self, copy=True):
        """pgx_batch_result_compact: the last run's result as the compact byte stream (include/pgx.h "compact result"): the counters, the tables
        block_offsets / block_first_mem / block_first_pos (uint64[n_blocks + 1]) and bytes (uint8[n_bytes]); compact_expand() turns it into what
        result() returns.  copy=False: views of the batch's pinned buffers, valid until its next run / upload / free"""
        r = CompactResult()
        _check(self.L.pgx_batch_result_compact(self.b, C.byref(r)))
        out = {k: int(getattr(r, k)) for k in _COMPACT_COUNTERS}
        out["ms_encode"] = float(r.ms_encode)
        nb, nbytes = out["n_blocks"], out["n_bytes"]
        for k in ("block_offsets", "block_first_mem", "block_first_pos"):
            a = np.ctypeslib.as_array(getattr(r, k), shape=(nb + 1,))
            out[k] = a.copy() if copy else a
        a = np.ctypeslib.as_array(r.bytes, shape=(nbytes,)) if nbytes else np.zeros(0, dtype=np.uint8)
        out["bytes"] = a.copy() if copy else a
        return out

    def result_counts(self):
        """pgx_batch_result without copying the arrays into numpy: the download into the batch's pinned host buffers happens,
        the (n_mems, n_positions) of the result are returned (the PCIe-inclusive timing of bench.py)"""
        r = Result()
        _check(self.L.pgx_batch_result(self.b, C.byref(r)))
        return int(r.n_mems), int(r.n_positions)

    def device_result(self):
        """results of the last run as device arrays (valid until the next run / upload / free): mem_offsets int64[n + 1],
        mems int64[n_mems, 4] (start, end, bwt_start, size), and with tags tag_run_counts / pos_offsets / positions"""
        r = DeviceResult()
        _check(self.L.pgx_batch_device_result(self.b, C.byref(r)))
        n, m = int(r.n_reads), int(r.n_mems)
        out = dict(device=True, n_reads=n, n_mems=m, mem_offsets=DeviceArray(r.mem_offsets, (n + 1,), self),
                   mems=DeviceArray(r.mems, (m, 4), self))
        if r.pos_offsets:
            out["tag_run_counts"] = DeviceArray(r.tag_run_counts, (m,), self)
            out["pos_offsets"] = DeviceArray(r.pos_offsets, (m + 1,), self)
            out["positions"] = DeviceArray(r.positions, (int(r.n_positions),), self)
        return out

    def format(self, first_seq=0, flags=0, max_length=0, reserved=0, copy=True):
        """pgx_batch_format: the find_mems text of the last run (and, with a locate flag, of the last locate), written on the device:
        dict(n_reads, n_bytes, n_err_bytes, read_offsets uint64[n_reads + 1], text bytes, err_text bytes or None, ms_format).
        copy=False: the counters and ms_format only (the text stays in the batch's pinned buffers)"""
        fp = FormatParams(first_seq, max_length, flags, reserved)
        t = Text()
        _check(self.L.pgx_batch_format(self.b, C.byref(fp), C.byref(t)))
        n = int(t.n_reads)
        if not copy:
            return dict(n_reads=n, n_bytes=int(t.n_bytes), n_err_bytes=int(t.n_err_bytes), ms_format=float(t.ms_format))
        return dict(n_reads=n, n_bytes=int(t.n_bytes), n_err_bytes=int(t.n_err_bytes), read_offsets=_u64_array(t.read_offsets, n + 1),
                    text=C.string_at(t.text, int(t.n_bytes)), err_text=C.string_at(t.err_text, int(t.n_err_bytes)) if t.err_text else None,
                    ms_format=float(t.ms_format))

    def locate(self, flags=0, max_occ=0, stream=None):
        """pgx_batch_locate: the occurrences of the last run's MEMs, left on the device (locations() / device_locations())"""
        _check(self.L.pgx_batch_locate(self.b, flags, max_occ, stream))

    def _locations(self, fn):
        r = Locations()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_mems=int(r.n_mems), n_values=int(r.n_values), n_not_located=int(r.n_not_located), flags=int(r.flags),
                       resident=bool(r.resident), ms_locate=float(r.ms_locate), set_words=int(r.set_words))

    def locations(self):
        """the last locate as numpy arrays: loc_offsets uint64[n_mems + 1] (MEM m's values = values[loc_offsets[m] .. [m + 1])), values,
        with n_values, n_not_located, flags, resident (1: gathered from the resident suffix array), ms_locate, set_words.  After
        LOCATE_SEQ_SETS also sets: uint64[n_mems, set_words], the same memory as values"""
        r, out = self._locations(self.L.pgx_batch_locations)
        out["loc_offsets"] = _u64_array(C.cast(r.loc_offsets, C.POINTER(u64)), out["n_mems"] + 1)
        out["values"] = _u64_array(C.cast(r.values, C.POINTER(u64)), out["n_values"])
        if out["flags"] & LOCATE_SEQ_SETS:
            out["sets"] = out["values"].reshape(out["n_mems"], out["set_words"])
        return out

    def device_locations(self):
        """the same as device arrays (valid until the next run / upload / locate / free)"""
        r, out = self._locations(self.L.pgx_batch_device_locations)
        out["device"] = True
        out["loc_offsets"] = DeviceArray(r.loc_offsets, (out["n_mems"] + 1,), self)
        out["values"] = DeviceArray(r.values, (out["n_values"],), self)
        if out["flags"] & LOCATE_SEQ_SETS:
            out["sets"] = DeviceArray(r.values, (out["n_mems"], out["set_words"]), self)
        return out

    def read_hits(self, flags=0, stream=None):
        """pgx_batch_read_hits on the sets of the last locate(LOCATE_SEQ_SETS), then hits()"""
        _check(self.L.pgx_batch_read_hits(self.b, flags, stream))
        return self.hits()

    def _hits(self, fn):
        r = ReadHits()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_reads=int(r.n_reads), n_seq=int(r.n_seq), set_words=int(r.set_words), flags=int(r.flags), ms_hits=float(r.ms_hits))

    def hits(self):
        """the last read hits as numpy arrays: hits READ_HIT_DTYPE[n_reads], best_sets uint64[n_reads, W] (None without
        HITS_BEST_SETS), scores uint32[n_reads, n_seq] (None without HITS_SCORES), with n_reads, n_seq, set_words, flags, ms_hits"""
        r, out = self._hits(self.L.pgx_batch_hits)
        n, W, q = out["n_reads"], out["set_words"], out["n_seq"]
        out["hits"] = np.frombuffer(C.string_at(r.hits, n * 40), dtype=READ_HIT_DTYPE).copy() if n else np.zeros(0, READ_HIT_DTYPE)
        out["best_sets"] = _u64_array(C.cast(r.best_sets, C.POINTER(u64)), n * W).reshape(n, W) if r.best_sets else None
        out["scores"] = (np.frombuffer(C.string_at(r.scores, n * q * 4), dtype=np.uint32).copy() if n * q else np.zeros(0, np.uint32)).reshape(n, q) if r.scores else None
        return out

    def device_hits(self):
        """the same as device arrays (valid until the next run / upload / read_hits / free): hits int64[n_reads, 5] (the 40-byte
        records as words), best_sets int64[n_reads, W], scores uint32[n_reads, n_seq]"""
        r, out = self._hits(self.L.pgx_batch_device_hits)
        n, W, q = out["n_reads"], out["set_words"], out["n_seq"]
        out["device"] = True
        out["hits"] = DeviceArray(r.hits, (n, 5), self)
        out["best_sets"] = DeviceArray(r.best_sets, (n, W), self) if r.best_sets else None
        out["scores"] = DeviceArray(r.scores, (n, q), self, "<u4") if r.scores else None
        return out

    def read_place(self, flags=0, stream=None):
        """pgx_batch_read_place on the packed positions of the last locate(0), then places()"""
        _check(self.L.pgx_batch_read_place(self.b, flags, stream))
        return self.places()

    def _places(self, fn):
        r = ReadPlaces()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_reads=int(r.n_reads), n_anchors=int(r.n_anchors), n_places=int(r.n_places), flags=int(r.flags), n_passes=int(r.n_passes),
                       ms_place=float(r.ms_place))

    def places(self):
        """the last read placement as numpy arrays: reads READ_PLACE_DTYPE[n_reads]; with PLACE_LIST place_offsets uint64[n_reads + 1] and
        places PLACEMENT_DTYPE[n_places] (None without), with n_reads, n_anchors, n_places, flags, n_passes, ms_place"""
        r, out = self._places(self.L.pgx_batch_places)
        n, k = out["n_reads"], out["n_places"]
        records = lambda ptr, count, dt: np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(ptr), dtype=dt).copy() if count else np.zeros(0, dt)  # (string_at takes a C int)
        out["reads"] = records(r.reads, n, READ_PLACE_DTYPE)
        out["place_offsets"] = _u64_array(C.cast(r.place_offsets, C.POINTER(u64)), n + 1) if r.place_offsets else None
        out["places"] = records(r.places, k, PLACEMENT_DTYPE) if r.places else None
        return out

    def device_places(self):
        """the same as device arrays (valid until the next run / upload / read_place / free): reads int64[n_reads, 8] (the 64-byte records
        as words), place_offsets int64[n_reads + 1], places int64[n_places, 3] (the 24-byte records as words)"""
        r, out = self._places(self.L.pgx_batch_device_places)
        n, k = out["n_reads"], out["n_places"]
        out["device"] = True
        out["reads"] = DeviceArray(r.reads, (n, 8), self)
        out["place_offsets"] = DeviceArray(r.place_offsets, (n + 1,), self) if r.place_offsets else None
        out["places"] = DeviceArray(r.places, (k, 3), self) if r.places else None
        return out

    def read_verify(self, max_cand=1, penalty=4, flags=0, stream=None):
        """pgx_batch_read_verify at the candidates of the last read_place (with PLACE_LIST when max_cand > 1), then verified()"""
        _check(self.L.pgx_batch_read_verify(self.b, max_cand, penalty, flags, stream))
        return self.verified()

    def _verified(self, fn):
        r = ReadVerifies()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_reads=int(r.n_reads), n_cands=int(r.n_cands), flags=int(r.flags), max_cand=int(r.max_cand), mismatch_penalty=int(r.mismatch_penalty),
                       ms_verify=float(r.ms_verify))

    def verified(self):
        """the last verify result as numpy arrays: reads VERIFY_DTYPE[n_reads]; with VERIFY_LIST cand_offsets uint64[n_reads + 1] and cands
        VERIFY_DTYPE[n_cands] (None without), with n_reads, n_cands, flags, max_cand, mismatch_penalty, ms_verify"""
        r, out = self._verified(self.L.pgx_batch_verified)
        n, k = out["n_reads"], out["n_cands"]
        records = lambda ptr, count, dt: np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(ptr), dtype=dt).copy() if count else np.zeros(0, dt)
        out["reads"] = records(r.reads, n, VERIFY_DTYPE)
        out["cand_offsets"] = _u64_array(C.cast(r.cand_offsets, C.POINTER(u64)), n + 1) if r.cand_offsets else None
        out["cands"] = records(r.cands, k, VERIFY_DTYPE) if r.cands else None
        return out

    def device_verified(self):
        """the same as device arrays (valid until the next run / upload / read_verify / free): reads and cands int64[., 8] (the 64-byte
        records as words), cand_offsets int64[n_reads + 1]"""
        r, out = self._verified(self.L.pgx_batch_device_verified)
        n, k = out["n_reads"], out["n_cands"]
        out["device"] = True
        out["reads"] = DeviceArray(r.reads, (n, 8), self)
        out["cand_offsets"] = DeviceArray(r.cand_offsets, (n + 1,), self) if r.cand_offsets else None
        out["cands"] = DeviceArray(r.cands, (k, 8), self) if r.cands else None
        return out

    def read_rescue(self, frag_min, frag_max, min_score, max_anchors=2, flags=0, stream=None):
        """pgx_batch_read_rescue on the list of the last read_verify (made with VERIFY_LIST), then rescued(); with RESCUE_MERGE every rescued read gains
        its best diagonal as the last candidate of its list, and the winners are recomputed"""
        _check(self.L.pgx_batch_read_rescue(self.b, frag_min, frag_max, min_score, max_anchors, flags, stream))
        return self.rescued()

    def _rescued(self, fn):
        r = ReadRescueResult()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_reads=int(r.n_reads), n_targets=int(r.n_targets), n_rescued=int(r.n_rescued), n_full=int(r.n_full), n_tasks=int(r.n_tasks), n_diags=int(r.n_diags),
                       frag_min=int(r.frag_min), frag_max=int(r.frag_max), min_score=int(r.min_score), max_anchors=int(r.max_anchors), flags=int(r.flags),
                       mismatch_penalty=int(r.mismatch_penalty), ms_rescue=float(r.ms_rescue))

    def rescued(self):
        """the last rescue result: reads RESCUE_DTYPE[n_reads], with n_reads, the five counters, the parameters of the call and ms_rescue"""
        r, out = self._rescued(self.L.pgx_batch_rescued)
        k = out["n_reads"]
        out["reads"] = np.frombuffer((C.c_char * (k * 64)).from_address(r.reads), dtype=RESCUE_DTYPE).copy() if k else np.zeros(0, RESCUE_DTYPE)
        return out

    def device_rescued(self):
        """the same with reads as a device array (valid until the next run / upload / read_rescue / free): int64[n_reads, 8], the 64-byte records as words"""
        r, out = self._rescued(self.L.pgx_batch_device_rescued)
        out["device"] = True
        out["reads"] = DeviceArray(r.reads, (out["n_reads"], 8), self)
        return out

    def read_mates(self, frag_min, frag_max, penalty, flags=0, stream=None):
        """pgx_batch_read_mates on the list of the last read_verify (made with VERIFY_LIST), then mated(); with MATES_ELECT the chosen candidates
        become the verify winners"""
        _check(self.L.pgx_batch_read_mates(self.b, frag_min, frag_max, penalty, flags, stream))
        return self.mated()

    def _mated(self, fn):
        r = ReadMatesResult()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_pairs=int(r.n_pairs), n_proper=int(r.n_proper), n_compatible=int(r.n_compatible), n_moved_a=int(r.n_moved_a), n_moved_b=int(r.n_moved_b),
                       frag_min=int(r.frag_min), frag_max=int(r.frag_max), flags=int(r.flags), penalty=int(r.penalty), ms_mates=float(r.ms_mates))

    def mated(self):
        """the last mates result: pairs MATES_DTYPE[n_pairs], with n_pairs, the four counters, frag_min, frag_max, flags, penalty, ms_mates"""
        r, out = self._mated(self.L.pgx_batch_mated)
        k = out["n_pairs"]
        out["pairs"] = np.frombuffer((C.c_char * (k * 64)).from_address(r.pairs), dtype=MATES_DTYPE).copy() if k else np.zeros(0, MATES_DTYPE)
        return out

    def device_mated(self):
        """the same with pairs as a device array (valid until the next run / upload / read_mates / free): int64[n_pairs, 8], the 64-byte records as words"""
        r, out = self._mated(self.L.pgx_batch_device_mated)
        out["device"] = True
        out["pairs"] = DeviceArray(r.pairs, (out["n_pairs"], 8), self)
        return out

    def read_mapq(self, scale=2, slack=8, max_extra=16, flags=0, stream=None):
        """pgx_batch_read_mapq on the list and the winners of the last read_verify (made with VERIFY_LIST; max_extra > 0: and the places of a read_place
        with PLACE_LIST; MAPQ_PAIRED: and the last read_mates), then mapqs()"""
        _check(self.L.pgx_batch_read_mapq(self.b, scale, slack, max_extra, flags, stream))
        return self.mapqs()

    def _mapqs(self, fn):
        r = ReadMapqs()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_reads=int(r.n_reads), n_has=int(r.n_has), n_unique=int(r.n_unique), n_capped=int(r.n_capped), sum_mapq=int(r.sum_mapq), n_extras=int(r.n_extras),
                       scale=int(r.scale), slack=int(r.slack), max_extra=int(r.max_extra), flags=int(r.flags), ms_mapq=float(r.ms_mapq))

    def mapqs(self):
        """the last mapq result: records MAPQ_DTYPE[n_reads], with n_reads, the four counters, n_extras, the parameters of the call and ms_mapq"""
        r, out = self._mapqs(self.L.pgx_batch_mapqs)
        k = out["n_reads"]
        out["records"] = np.frombuffer((C.c_char * (k * 32)).from_address(r.records), dtype=MAPQ_DTYPE).copy() if k else np.zeros(0, MAPQ_DTYPE)
        return out

    def device_mapqs(self):
        """the same with records as a device array (valid until the next run / upload / read_verify / read_rescue / read_mates / read_mapq / free):
        int64[n_reads, 4], the 32-byte records as words"""
        r, out = self._mapqs(self.L.pgx_batch_device_mapqs)
        out["device"] = True
        out["records"] = DeviceArray(r.records, (out["n_reads"], 4), self)
        return out

    def read_align(self, band=8, flags=0, stream=None):
        """pgx_batch_read_align at the winners of the last read_verify, then aligned()"""
        _check(self.L.pgx_batch_read_align(self.b, band, flags, stream))
        return self.aligned()

    def _aligned(self, fn):
        r = ReadAligns()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_reads=int(r.n_reads), n_ops=int(r.n_ops), flags=int(r.flags), band=int(r.band), passes=int(r.passes), scratch_bytes=int(r.scratch_bytes),
                       ms_align=float(r.ms_align), ms_forward=float(r.ms_forward), ms_trace=float(r.ms_trace))

    def aligned(self):
        """the last align result as numpy arrays: reads ALIGN_DTYPE[n_reads]; with ALIGN_CIGAR op_offsets uint64[n_reads + 1] and ops uint32[n_ops]
        (None without), with n_reads, n_ops, flags, band, passes, scratch_bytes, ms_align, ms_forward, ms_trace"""
        r, out = self._aligned(self.L.pgx_batch_aligned)
        n, k = out["n_reads"], out["n_ops"]
        out["reads"] = np.frombuffer((C.c_char * (n * 64)).from_address(r.reads), dtype=ALIGN_DTYPE).copy() if n else np.zeros(0, ALIGN_DTYPE)
        out["op_offsets"] = _u64_array(C.cast(r.op_offsets, C.POINTER(u64)), n + 1) if r.op_offsets else None
        out["ops"] = (np.frombuffer((C.c_char * (k * 4)).from_address(r.ops), dtype=np.uint32).copy() if k else np.zeros(0, np.uint32)) if r.op_offsets else None
        return out

    def device_aligned(self):
        """the same as device arrays (valid until the next run / upload / read_align / free): reads int64[n_reads, 8] (the 64-byte records as
        words), op_offsets int64[n_reads + 1], ops uint32[n_ops]"""
        r, out = self._aligned(self.L.pgx_batch_device_aligned)
        n, k = out["n_reads"], out["n_ops"]
        out["device"] = True
        out["reads"] = DeviceArray(r.reads, (n, 8), self)
        out["op_offsets"] = DeviceArray(r.op_offsets, (n + 1,), self) if r.op_offsets else None
        out["ops"] = DeviceArray(r.ops, (k,), self, "<u4") if r.ops else None
        return out

    def read_walk(self, flags=0, stream=None):
        """pgx_batch_read_walk along the stretches of the last read_align, then walked()"""
        _check(self.L.pgx_batch_read_walk(self.b, flags, stream))
        return self.walked()

    def _walked(self, fn):
        r = ReadWalks()
        _check(fn(self.b, C.byref(r)))
        return r, dict(n_reads=int(r.n_reads), n_steps=int(r.n_steps), flags=int(r.flags), ms_walk=float(r.ms_walk))

    def walked(self):
        """the last walk result as numpy arrays: reads WALK_DTYPE[n_reads]; with WALK_STEPS step_offsets uint64[n_reads + 1] and steps uint64[n_steps]
        (None without), with n_reads, n_steps, flags, ms_walk"""
        r, out = self._walked(self.L.pgx_batch_walked)
        n, k = out["n_reads"], out["n_steps"]
        out["reads"] = np.frombuffer((C.c_char * (n * 32)).from_address(r.reads), dtype=WALK_DTYPE).copy() if n else np.zeros(0, WALK_DTYPE)
        out["step_offsets"] = _u64_array(C.cast(r.step_offsets, C.POINTER(u64)), n + 1) if r.step_offsets else None
        out["steps"] = (_u64_array(C.cast(r.steps, C.POINTER(u64)), k) if k else np.zeros(0, np.uint64)) if r.step_offsets else None
        return out

    def device_walked(self):
        """the same as device arrays (valid until the next run / upload / read_walk / free): reads int64[n_reads, 4] (the 32-byte records as words),
        step_offsets int64[n_reads + 1], steps int64[n_steps]"""
        r, out = self._walked(self.L.pgx_batch_device_walked)
        n, k = out["n_reads"], out["n_steps"]
        out["device"] = True
        out["reads"] = DeviceArray(r.reads, (n, 4), self)
        out["step_offsets"] = DeviceArray(r.step_offsets, (n + 1,), self) if r.step_offsets else None
        out["steps"] = DeviceArray(r.steps, (k,), self) if r.steps else None
        return out

    def free(self):
        if getattr(self, "b", None):
            self.L.pgx_batch_free(self.b)
            self.b = None

    __del__ = free
