"""The image file of include/pgx.h ("image file") restated in Python from the header's text alone: the 64-byte header, the section
table, the meta record and the section sum.  Nothing here calls the library; the tests compare the two."""
import struct

import numpy as np

MAGIC = b"PGXIMAGE"
FILE_VERSION = 1
HEADER_BYTES, ENTRY_BYTES, META_BYTES, ALIGN, MAX_SECTIONS = 64, 32, 456, 4096, 64
HAS_LOCATE, HAS_LITERAL = 1, 2
GOLD = np.uint64(0x9E3779B97F4A7C15)
MULT = np.uint64(0xD6E8FEB86659FD93)
S32 = np.uint64(32)

SECTION_NAMES = {1: "consts", 2: "blocks", 3: "dir", 4: "bstart", 5: "blow", 6: "exc", 7: "pairs", 8: "sbase2", 9: "pbase", 10: "tstart",
                 11: "tvals", 12: "tdir", 13: "n_runs", 20: "loc_consts", 21: "rstart", 22: "rsamp", 23: "rdir", 24: "lpos", 25: "lnext",
                 26: "ldir", 30: "lit_bstart", 31: "lit_cum", 32: "lit_runs", 33: "lit_roff", 34: "lit_tabs"}
# section id -> selector of pgx_index_image_view that shows the same bytes (n_runs and lit_tabs have none)
SECTION_VIEW = {1: 6, 2: 0, 3: 1, 4: 2, 5: 7, 6: 15, 7: 20, 8: 22, 9: 23, 10: 3, 11: 4, 12: 5, 20: 14, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12,
                26: 13, 30: 16, 31: 17, 32: 18, 33: 19}


def section_sum(data):
    """sum over the 8-byte little-endian words w[i] (tail padded with zero bytes) of mix(w[i] + (i + 1) * GOLD), modulo 2^64"""
    b = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    n = b.size
    if n == 0:
        return 0
    total = 0
    step = 1 << 24  # words per piece (bounds the temporaries)
    n_words = (n + 7) // 8
    for w0 in range(0, n_words, step):
        w1 = min(n_words, w0 + step)
        piece = b[w0 * 8:min(n, w1 * 8)]
        if piece.size % 8:
            piece = np.concatenate([piece, np.zeros(8 - piece.size % 8, dtype=np.uint8)])
        w = piece.view("<u8").astype(np.uint64)
        with np.errstate(over="ignore"):
            z = w + (np.arange(w0 + 1, w1 + 1, dtype=np.uint64) * GOLD)
            z = (z ^ (z >> S32)) * MULT
            z = z ^ (z >> S32)
            total = (total + int(z.sum(dtype=np.uint64))) & 0xFFFFFFFFFFFFFFFF
    return total


class ImageFile:
    """header, table and meta record of the bytes of an image file; raises ValueError where the text of pgx.h is violated"""

    def __init__(self, data):
        self.data = data
        if len(data) < HEADER_BYTES or data[:8] != MAGIC:
            raise ValueError("not an image file")
        (self.version, self.layout, self.consts_bytes, self.loc_consts_bytes, self.mode, self.has_rank, self.has_tags, self.n_sections,
         self.meta_bytes, self.flags, self.header_sum, self.reserved) = struct.unpack_from("<10IQQ", data, 8)
        if not 1 <= self.n_sections <= MAX_SECTIONS or self.meta_bytes != META_BYTES:
            raise ValueError("section count or meta size")
        self.head_bytes = HEADER_BYTES + ENTRY_BYTES * self.n_sections + self.meta_bytes
        if len(data) < self.head_bytes:
            raise ValueError("truncated table")
        self.sections = []
        for i in range(self.n_sections):
            sid, elem, nbytes, offset, ssum = struct.unpack_from("<IIQQQ", data, HEADER_BYTES + ENTRY_BYTES * i)
            self.sections.append(dict(id=sid, elem_size=elem, bytes=nbytes, offset=offset, sum=ssum, name=SECTION_NAMES.get(sid, "?"), entry_at=HEADER_BYTES + ENTRY_BYTES * i))
        m = self.meta_at = HEADER_BYTES + ENTRY_BYTES * self.n_sections
        self.sym_map = bytes(data[m:m + 256])
        self.C = struct.unpack_from("<8Q", data, m + 256)
        self.sigma, self.encoded, self.hasN, self.tags_format = struct.unpack_from("<4I", data, m + 320)
        self.sequence_size, self.max_length, self.n_file_blocks = struct.unpack_from("<3Q", data, m + 336)
        (self.ref_block_mean_bytes,) = struct.unpack_from("<d", data, m + 360)
        (self.n_samples,) = struct.unpack_from("<Q", data, m + 368)
        self.sym_total = struct.unpack_from("<6Q", data, m + 376)
        self.n_tag_items, self.n_exc, self.n_lit_blocks, self.n_lit_runs = struct.unpack_from("<4Q", data, m + 424)

    def computed_header_sum(self):
        head = bytearray(self.data[:self.head_bytes])
        head[48:56] = bytes(8)
        return section_sum(bytes(head))

    def section_bytes(self, s):
        return self.data[s["offset"]:s["offset"] + s["bytes"]]

    def by_name(self, name):
        return next(s for s in self.sections if s["name"] == name)


def reseal(buf):
    """a mutated copy's header sum put right again (so that a test reaches the check behind the header sum)"""
    f = ImageFile(bytes(buf))
    struct.pack_into("<Q", buf, 48, f.computed_header_sum())
    return buf
