// find_mems -- drop-in for the reference CLI (src/find_mems.cpp:13-147) on MI355X.
//
//   find_mems <r_index.ri> <tags> <reads.txt> <min_mem_length> <min_occ> [options after the 5 positionals]
//   find_mems <index.pgi> - <reads.txt> <min_mem_length> <min_occ> [...]      (an image file made by pgx_image: nothing is parsed or built on the host)
//
// stdout grammar is the reference's, byte for byte (find_mems.cpp:115-118,138,144-145 and
// tag_arrays.cpp:885-889); reads are processed in device batches but printed in file order.
// Options (ours): --device N | --gpus N (devices 0 .. N-1) | --devices a,b,.. ; --streams W (batches in flight per device);
//                 --mode compat|strict, --batch N (reads per device batch), --tags-format auto|bytecode|compact,
//                 --quiet (no per-read stderr line), --reads-format lines|fasta|fastq|auto (default lines; auto: by the first byte,
//                 '>' FASTA, '@' FASTQ, otherwise lines), --device-parse (line files parsed on the device too; FASTA / FASTQ always are),
//                 --locate positions|seqs (the occurrences of every MEM, pgx_batch_locate), --locate-max K (MEMs with more occurrences: not located),
//                 --result full|compact (default full; compact: the result crosses the link as the compact byte stream, pgx_batch_result_compact,
//                 and every formatter thread expands its own blocks, pgx_compact_expand; the same text either way),
//                 --format host|device (default host; device: the text itself is written on the device, pgx_batch_format -- no result arrays cross the link,
//                 no formatter threads run, --result has no effect; the same text either way),
//                 --hits FILE (one line per read: which indexed sequence the read matches best, pgx_batch_read_hits; stdout and stderr stay as they are),
//                 --hits-max K (MEMs with more occurrences count as not located in the hits), --hits-only (no MEM text: stdout stays empty; not with --locate)
//                 --place FILE (one line per read: the sequence diagonal the read lies on best, pgx_batch_read_place; stdout and stderr stay as they are),
//                 --place-max K (MEMs with more occurrences are left unlocated in the placement), --place-only (no MEM text, like --hits-only)
//                 --verify FILE (one line per read: the read laid on the indexed text at its best placements, pgx_batch_read_verify; runs the place
//                 stage itself without --place; stdout and stderr stay as they are), --verify-max C (candidates per read, 1 .. 64, default 1),
//                 --verify-mismatch P (the segment's mismatch penalty, default 4), --verify-only (no MEM text, like --place-only)
//                 --align FILE (one line per read: the banded alignment with gaps at the verify winner and its CIGAR, pgx_batch_read_align; runs the
//                 place and verify stages itself when they are not requested, with --place-max, --verify-max and --verify-mismatch as there; stdout
//                 and stderr stay as they are), --align-band W (0 .. 31, default 8), --align-only (no MEM text, like --verify-only)
//                 --gaf FILE (one GAF line per read: the alignment as a walk through the graph, pgx_batch_read_walk; runs the place, verify and align
//                 stages itself when they are not requested, with their options as there; stdout and stderr stay as they are), --gaf-only (no MEM
//                 text, like --align-only)
//                 --paired (the reads file is interleaved: records 2k and 2k + 1 are mates, in every --reads-format; an odd record count ends the run
//                 with status 1; every batch holds whole pairs; runs place with its list, verify with its list -- --verify-max defaults to 16 --
//                 and pgx_batch_read_mates with PGX_MATES_ELECT, so that --verify, --align and --gaf report the winners the pairs elected),
//                 --frag-min A (default 0), --frag-max B (default 1000), --mates-penalty U (default 2 * (P + 1), P of --verify-mismatch),
//                 --mates FILE (one line per pair), --mates-only (no MEM text, like --verify-only)
//                 --rescue (with --paired: pgx_batch_read_rescue with PGX_RESCUE_MERGE between verify and mates, under the bounds of --frag-min /
//                 --frag-max: a read without a placement near its placed mate is searched for on every diagonal of the window the mate names, and
//                 what is found joins its candidates, so that mates, --verify, --align and --gaf see it), --rescue-min S (default min_mem_length),
//                 --rescue-anchors R (1 .. 8, default 2), --rescued FILE (one line per read),
//                 --mapq (with --gaf or --mapq-file: pgx_batch_read_mapq behind verify, and behind rescue and mates under --paired, where it takes the
//                 paired scores; place and verify run with their lists, --verify-max defaults to 16; column 12 of a GAF line whose read has steps is the
//                 read's mapping quality), --mapq-scale D (1 .. 16, default 2), --mapq-slack K (0 .. 1024, default 8), --mapq-extra X (0 .. 63, default
//                 16), --mapq-file FILE (one line per read)
//                 --pack FILE (written once at the end: per node of the graph how many reads cover its bases, pgx_pack; runs the place, verify and align
//                 stages itself when they are not requested, align with its CIGAR list, and no walk stage; one pack per device, every worker adds its
//                 finished batch, the vectors of several devices are summed on the host; stdout and stderr stay as they are), --pack-bases FILE2 (one
//                 line per covered base), --pack-min-mapq Q (1 .. 60, with --mapq, which --pack satisfies as --gaf does: reads below Q are not
//                 counted), --pack-only (no MEM text, like --gaf-only)
// The tag file may be either query format; the reference's find_mems only loads the sdsl-compact one.
//
// The per-read loop of the reference (find_mems.cpp:94-139) becomes a pipeline: one reader thread cuts the reads file into
// batches of consecutive reads; every device has W worker threads, each with its own batch and stream (pgx_batch), which
// upload, run, download and format the text of whole batches -- so on one device the upload of batch k + 1, the kernels of
// batch k and the download / formatting of batch k - 1 overlap, and N devices take batches in turn with the index replicated
// (reads shard, no collective); the main thread writes the finished texts in file order.
// Device-parsed input (FASTA, FASTQ, --device-parse): the ranges end at record starts (pgx_fastx_cut), the parse threads only copy the raw
// bytes into pinned buffers and the workers hand them to pgx_batch_upload_text; a range's read count -- and so the numbers of the reads
// after it -- is known once it has been uploaded, and a worker formats its batch when every range before it has been counted.
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
#include <atomic>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/pgx.h"

// An image file (pgx_index_save_image, the pgx_image CLI) in the place of the r-index: the first positional starts with the image magic.  The tags
// positional must then be "-" (the image holds the tag runs), --mode may only repeat the image's, --tags-format has nothing to say.
static bool is_image_file(const char *path) {
    char m[8] = {0};
    std::ifstream f(path, std::ios::binary);
    return f && f.read(m, 8) && std::memcmp(m, PGX_IMAGE_MAGIC, 8) == 0;
}
// 0, or 1 with a message on stderr
static int open_image_index(const char *image_path, const char *tags_arg, bool mode_given, uint32_t mode, pgx_index **h) {
    if (std::string(tags_arg) != "-") {
        std::cerr << image_path << " is an image file and holds its tag runs: the tags argument must be \"-\", not " << tags_arg << std::endl;
        return 1;
    }
    pgx_image_info fi;
    if (pgx_image_file_info(image_path, &fi) != PGX_OK) { std::cerr << pgx_last_error() << std::endl; return 1; }
    if (mode_given && fi.mode != mode) {
        std::cerr << "--mode " << (mode == PGX_MODE_STRICT ? "strict" : "compat") << ": the image file was made in " << (fi.mode == PGX_MODE_STRICT ? "strict" : "compat")
                  << " mode (make another with pgx_image --mode)" << std::endl;
        return 1;
    }
    if (pgx_index_open_image(image_path, 0, h) != PGX_OK) { std::cerr << pgx_last_error() << std::endl; return 1; }
    return 0;
}

// decimal text of v at p; returns the end.  Two digits per division.
static inline char *put_u64(char *p, uint64_t v) {
    static const char d2[201] =
        "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
    char tmp[20];
    int k = 20;
    while (v >= 100) {
        const unsigned r = (unsigned)(v % 100);
        v /= 100;
        k -= 2;
        tmp[k] = d2[2 * r];
        tmp[k + 1] = d2[2 * r + 1];
    }
    if (v >= 10) { k -= 2; tmp[k] = d2[2 * v]; tmp[k + 1] = d2[2 * v + 1]; }
    else tmp[--k] = (char)('0' + v);
    std::memcpy(p, tmp + k, (size_t)(20 - k));
    return p + (20 - k);
}
static inline char *put_str(char *p, const char *s) {
    const size_t n = std::strlen(s);
    std::memcpy(p, s, n);
    return p + n;
}

// read bytes of a batch: pinned host memory from a small pool (pgx_host_alloc: uploads at link speed), ordinary memory when that fails
struct ReadBuf {
    char *p = nullptr;
    size_t cap = 0, len = 0;
    bool pinned = false;
};
class ReadBufPool {
    std::mutex mu;
    std::vector<ReadBuf> free_;
public:
    ReadBuf get(size_t bytes) {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < free_.size(); i++)
                if (free_[i].cap >= bytes) { ReadBuf b = free_[i]; free_.erase(free_.begin() + (std::ptrdiff_t)i); b.len = 0; return b; }
        }
        ReadBuf b;
        b.cap = bytes + bytes / 8 + 4096;
        void *q = nullptr;
        if (pgx_host_alloc(b.cap, &q) == PGX_OK) { b.p = static_cast<char *>(q); b.pinned = true; }
        else { b.p = static_cast<char *>(std::malloc(b.cap)); if (!b.p) throw std::bad_alloc(); }
        return b;
    }
    void put(ReadBuf b) { if (!b.p) return; std::lock_guard<std::mutex> lk(mu); free_.push_back(b); }
    ~ReadBufPool() { for (auto &b : free_) { if (b.pinned) pgx_host_free(b.p); else std::free(b.p); } }
};
struct Job { // one batch of consecutive reads
    uint64_t id = 0, first_seq = 0; // batch number, reads before it in the file
    ReadBuf cat;
    std::vector<uint64_t> offs;
    // the same reads packed to two bits per symbol by the parse thread (pgx_pack_reads): [packed words | bytes of the reads with a byte outside A C G T]
    ReadBuf pk;
    std::vector<uint64_t> side_ids;
    uint64_t n_side = 0, side_at = 0;
    bool packed = false;
};
struct Done {
    std::vector<std::string> outs, errs; // text pieces in read order
    // --format device: the text where pgx_batch_format left it, in pinned buffers of the worker's batch (lent to the writer: the worker formats its
    // next batch but one only when this one has been written)
    const char *text = nullptr, *etext = nullptr;
    size_t text_n = 0, etext_n = 0;
    double mem_s = 0, tag_s = 0;
    std::string hits; // --hits: the lines of this batch
    std::string places; // --place: the lines of this batch
    std::string verifies; // --verify: the lines of this batch
    std::string aligns; // --align: the lines of this batch
    std::string gaf; // --gaf: the lines of this batch
    std::string mates; // --mates: the lines of this batch's pairs
    std::string rescued; // --rescued: the lines of this batch
    std::string mapqs;   // --mapq-file: the lines of this batch
    std::string error;
};

// text of reads [lo, hi) of a finished batch (stdout piece + the per-read stderr lines of find_all_mems, algorithm.hpp:754)
// --locate: two more lines per MEM block (the reference's list style, every item followed by ", "):
//   positions  "Occurrences: <size>" and "<seq>:<offset>, " per occurrence in BWT order
//   seqs       "Sequences: <count>" and "<seq>, " per sorted unique sequence id
//   a MEM without values (over --locate-max): "Occurrences: <size> (not located)" and an empty line
enum { LOCATE_NONE = 0, LOCATE_POSITIONS = 1, LOCATE_SEQS = 2 };
struct LocateOut {
    int mode = LOCATE_NONE;
    uint64_t max_length = 1;
    const pgx_locations *loc = nullptr;
};
static inline char *put_i64(char *p, int64_t v) {
    if (v < 0) { *p++ = '-'; return put_u64(p, (uint64_t)(-(v + 1)) + 1u); }
    return put_u64(p, (uint64_t)v);
}

static void format_range(const pgx_result &r, size_t lo, size_t hi, uint64_t first_seq, bool quiet, const LocateOut &lo_, std::string &out, std::string &err) {
    out.clear();
    err.clear();
    // exact upper bound of the text of this range: 20 digits per number
    const uint64_t m_lo = r.mem_offsets[lo], m_hi = r.mem_offsets[hi];
    const uint64_t p_cnt = r.pos_offsets[m_hi] - r.pos_offsets[m_lo];
    const uint64_t *lof = lo_.mode ? lo_.loc->loc_offsets : nullptr;
    const uint64_t v_cnt = lo_.mode ? lof[m_hi] - lof[m_lo] : 0;
    out.resize((hi - lo) * 32 + (m_hi - m_lo) * (lo_.mode ? 256 : 192) + p_cnt * 22 + v_cnt * 44 + 64);
    char *p = &out[0];
    for (size_t i = lo; i < hi; i++) {
        const size_t seq = first_seq + i + 1;
        if (!quiet) { err += "[find_all_mems] total mems="; err += std::to_string(r.mem_offsets[i + 1] - r.mem_offsets[i]); err += '\n'; }
        p = put_str(p, "Seq: "); p = put_u64(p, seq); *p++ = '\n'; // :115
        for (uint64_t m = r.mem_offsets[i]; m < r.mem_offsets[i + 1]; m++) {
            const pgx_mem &mm = r.mems[m];
            p = put_str(p, "MEM START: "); p = put_u64(p, mm.start);
            p = put_str(p, ", MEM END: "); p = put_u64(p, mm.end);
            p = put_str(p, " BWT START: "); p = put_u64(p, mm.bwt_start);
            p = put_str(p, " SIZE: ");
            if (mm.size < 0) { *p++ = '-'; p = put_u64(p, (uint64_t)(-(mm.size + 1)) + 1u); } else p = put_u64(p, (uint64_t)mm.size);
            *p++ = '\n'; // :118
            p = put_str(p, "Number of unique positions: "); p = put_u64(p, r.pos_offsets[m + 1] - r.pos_offsets[m]); *p++ = '\n'; // tag_arrays.cpp:885
            for (uint64_t q = r.pos_offsets[m]; q < r.pos_offsets[m + 1]; q++) { p = put_u64(p, r.positions[q]); *p++ = ','; *p++ = ' '; }
            *p++ = '\n';
            if (lo_.mode) {
                const uint64_t *v = lo_.loc->values;
                if (lof[m + 1] == lof[m]) { p = put_str(p, "Occurrences: "); p = put_i64(p, mm.size); p = put_str(p, " (not located)\n"); }
                else if (lo_.mode == LOCATE_POSITIONS) {
                    p = put_str(p, "Occurrences: "); p = put_i64(p, mm.size); *p++ = '\n';
                    for (uint64_t q = lof[m]; q < lof[m + 1]; q++) {
                        p = put_u64(p, v[q] / lo_.max_length); *p++ = ':'; p = put_u64(p, v[q] % lo_.max_length); *p++ = ','; *p++ = ' ';
                    }
                } else {
                    p = put_str(p, "Sequences: "); p = put_u64(p, lof[m + 1] - lof[m]); *p++ = '\n';
                    for (uint64_t q = lof[m]; q < lof[m + 1]; q++) { p = put_u64(p, v[q]); *p++ = ','; *p++ = ' '; }
                }
                *p++ = '\n';
            }
        }
        *p++ = '\n'; // :138
    }
    out.resize((size_t)(p - &out[0]));
}

// --result compact: the arrays a worker expands its batches into (grow-only, not cleared: every entry the formatters read is written first)
template <class T> struct GrowArray {
    std::unique_ptr<T[]> p;
    size_t cap = 0;
    T *ensure(size_t n) {
        if (n > cap) { cap = n + n / 4 + 64; p.reset(new T[cap]); }
        return p.get();
    }
};
struct ExpandBufs {
    GrowArray<uint64_t> mem_off, run_counts, pos_off, positions;
    GrowArray<pgx_mem> mems;
};
// all formatter threads of a batch have expanded their blocks (a range reads the offsets that close it, which its neighbour writes)
struct Rendezvous {
    std::mutex mu;
    std::condition_variable cv;
    unsigned waiting;
    explicit Rendezvous(unsigned n) : waiting(n) {}
    void arrive_and_wait() {
        std::unique_lock<std::mutex> lk(mu);
        if (--waiting == 0) cv.notify_all();
        else cv.wait(lk, [&]() { return waiting == 0; });
    }
};

// --hits: the lines of reads [0, n) of a batch, appended to out ("read" is the number of the read's "Seq:" line)
static const char HITS_HEADER[] = "#read\tmems\tlocated\tcovered\tbest\tn_best\tbest_seq\tnext\n";
static void format_hits(const pgx_read_hit *hits, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (8 * 21));
    char *p = &out[0];
    for (size_t i = 0; i < n; i++) {
        const pgx_read_hit &x = hits[i];
        p = put_u64(p, first_seq + i + 1); *p++ = '\t';
        p = put_u64(p, x.n_mems); *p++ = '\t';
        p = put_u64(p, x.n_located); *p++ = '\t';
        p = put_u64(p, x.covered); *p++ = '\t';
        p = put_u64(p, x.best_score); *p++ = '\t';
        p = put_u64(p, x.n_best); *p++ = '\t';
        if (x.best_seq == PGX_NO_SEQUENCE) *p++ = '*'; else p = put_u64(p, x.best_seq);
        *p++ = '\t';
        p = put_u64(p, x.next_score); *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --place: the lines of reads [0, n) of a batch, appended to out; best_seq and best_pos print as * when no placement has a score
static const char PLACE_HEADER[] = "#read\tmems\tlocated\tanchors\tplacements\tbest\tn_best\tbest_seq\tbest_pos\tbest_mems\tnext\n";
static void format_places(const pgx_read_place *recs, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (11 * 21));
    char *p = &out[0];
    for (size_t i = 0; i < n; i++) {
        const pgx_read_place &x = recs[i];
        p = put_u64(p, first_seq + i + 1); *p++ = '\t';
        p = put_u64(p, x.n_mems); *p++ = '\t';
        p = put_u64(p, x.n_located); *p++ = '\t';
        p = put_u64(p, x.n_anchors); *p++ = '\t';
        p = put_u64(p, x.n_placements); *p++ = '\t';
        p = put_u64(p, x.best_score); *p++ = '\t';
        p = put_u64(p, x.n_best); *p++ = '\t';
        if (x.best_score == 0) { *p++ = '*'; *p++ = '\t'; *p++ = '*'; }
        else {
            p = put_u64(p, x.best_seq); *p++ = '\t';
            if (x.best_diag < 0) { *p++ = '-'; p = put_u64(p, 0 - (uint64_t)x.best_diag); } else p = put_u64(p, (uint64_t)x.best_diag);
        }
        *p++ = '\t';
        p = put_u64(p, x.best_mems); *p++ = '\t';
        p = put_u64(p, x.next_score); *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --verify: the lines of reads [0, n) of a batch, appended to out; seq and pos print as * when the read has no candidate
static const char VERIFY_HEADER[] = "#read\tseq\tpos\tspan_lo\tspan_hi\tmatches\tmismatches\tseg_start\tseg_end\tseg_score\tseg_mismatches\trun\trun_start\tcands\ttied\n";
static void format_verifies(const pgx_read_verify *recs, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (15 * 21));
    char *p = &out[0];
    for (size_t i = 0; i < n; i++) {
        const pgx_read_verify &x = recs[i];
        p = put_u64(p, first_seq + i + 1); *p++ = '\t';
        if (x.seq == PGX_NO_SEQUENCE) { *p++ = '*'; *p++ = '\t'; *p++ = '*'; }
        else {
            p = put_u64(p, x.seq); *p++ = '\t';
            if (x.diag < 0) { *p++ = '-'; p = put_u64(p, 0 - (uint64_t)x.diag); } else p = put_u64(p, (uint64_t)x.diag);
        }
        const uint32_t f[12] = {x.span_lo, x.span_hi, x.matches, x.mismatches, x.seg_start, x.seg_end, x.seg_score, x.seg_mismatches, x.longest_run, x.run_start, x.n_cand, x.n_tied};
        for (uint32_t v : f) { *p++ = '\t'; p = put_u64(p, v); }
        *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --mates: the lines of pairs [0, n) of a batch whose first read is first_seq (even), appended to out; frag prints as * without a compatible pair,
// seq_a / seq_b as * for a mate without a candidate
static const char MATES_HEADER[] = "#pair\tread_a\tread_b\tproper\tfrag\tpair_score\tsolo_score\tcand_a\tcand_b\tseq_a\tseq_b\tn_compatible\tn_best\tnext\tmoved_a\tmoved_b\n";
static void format_mates(const pgx_read_mates *recs, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (16 * 21));
    char *p = &out[0];
    for (size_t k = 0; k < n; k++) {
        const pgx_read_mates &x = recs[k];
        p = put_u64(p, first_seq / 2 + k + 1); *p++ = '\t';
        p = put_u64(p, first_seq + 2 * k + 1); *p++ = '\t';
        p = put_u64(p, first_seq + 2 * k + 2); *p++ = '\t';
        *p++ = (x.flags & PGX_MATES_PROPER) ? '1' : '0'; *p++ = '\t';
        if (!(x.flags & PGX_MATES_COMPATIBLE)) *p++ = '*';
        else if (x.frag < 0) { *p++ = '-'; p = put_u64(p, 0 - (uint64_t)x.frag); }
        else p = put_u64(p, (uint64_t)x.frag);
        const uint32_t f[4] = {x.pair_score, x.solo_score, x.cand_a, x.cand_b};
        for (uint32_t v : f) { *p++ = '\t'; p = put_u64(p, v); }
        const uint32_t q[2] = {x.seq_a, x.seq_b};
        for (uint32_t v : q) { *p++ = '\t'; if (v == PGX_NO_SEQUENCE) *p++ = '*'; else p = put_u64(p, v); }
        const uint32_t g[3] = {x.n_compatible, x.n_best, x.next_score};
        for (uint32_t v : g) { *p++ = '\t'; p = put_u64(p, v); }
        *p++ = '\t'; *p++ = (x.flags & PGX_MATES_MOVED_A) ? '1' : '0';
        *p++ = '\t'; *p++ = (x.flags & PGX_MATES_MOVED_B) ? '1' : '0';
        *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --rescued: the lines of reads [0, n) of a batch whose first read is first_seq, appended to out; seq and pos (the diagonal) print as * for a read
// that is no target and for a target whose windows were empty
static const char RESCUED_HEADER[] = "#read\ttarget\tanchors\tdiags\tseq\tpos\tseg_score\tmatches\tn_best\tnext\trescued\n";
static void format_rescued(const pgx_read_rescue *recs, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (11 * 21));
    char *p = &out[0];
    for (size_t k = 0; k < n; k++) {
        const pgx_read_rescue &x = recs[k];
        p = put_u64(p, first_seq + k + 1); *p++ = '\t';
        *p++ = (x.flags & PGX_RESCUE_TARGET) ? '1' : '0'; *p++ = '\t';
        p = put_u64(p, x.n_anchors); *p++ = '\t';
        p = put_u64(p, x.n_diags); *p++ = '\t';
        if (x.seq == PGX_NO_SEQUENCE) { *p++ = '*'; *p++ = '\t'; *p++ = '*'; }
        else {
            p = put_u64(p, x.seq); *p++ = '\t';
            if (x.diag < 0) { *p++ = '-'; p = put_u64(p, 0 - (uint64_t)x.diag); }
            else p = put_u64(p, (uint64_t)x.diag);
        }
        const uint32_t f[4] = {x.seg_score, x.matches, x.n_best, x.next_score};
        for (uint32_t v : f) { *p++ = '\t'; p = put_u64(p, v); }
        *p++ = '\t'; *p++ = (x.flags & PGX_RESCUE_RESCUED) ? '1' : '0';
        *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --mapq-file: the lines of reads [0, n) of a batch whose first read is first_seq, appended to out
static const char MAPQ_HEADER[] = "#read\tmapq\tentries\tloci\twith\tcompeting\tbest_other\texcess\tflags\n";
static void format_mapqs(const pgx_read_mapq *recs, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (9 * 21));
    char *p = &out[0];
    for (size_t k = 0; k < n; k++) {
        const pgx_read_mapq &x = recs[k];
        p = put_u64(p, first_seq + k + 1);
        const uint32_t f[8] = {x.mapq, x.n_entries, x.n_loci, x.n_with, x.n_competing, x.best_other, x.excess, x.flags};
        for (uint32_t v : f) { *p++ = '\t'; p = put_u64(p, v); }
        *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --align: the lines of reads [0, n) of a batch, appended to out; seq, start, end and cigar print as * when the read has no candidate
static const char ALIGN_HEADER[] = "#read\tseq\tstart\tend\tclip_lo\tclip_hi\tedits\tmatches\tmismatches\tins\tdel\tband_hit\tcigar\n";
static void format_aligns(const pgx_read_align *recs, const uint64_t *op_off, const uint32_t *ops, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (12 * 21 + 2) + (size_t)(op_off[n] - op_off[0]) * 11);
    char *p = &out[0];
    for (size_t i = 0; i < n; i++) {
        const pgx_read_align &x = recs[i];
        const bool none = x.seq == PGX_NO_SEQUENCE;
        p = put_u64(p, first_seq + i + 1); *p++ = '\t';
        if (none) { *p++ = '*'; *p++ = '\t'; *p++ = '*'; *p++ = '\t'; *p++ = '*'; }
        else { p = put_u64(p, x.seq); *p++ = '\t'; p = put_u64(p, x.text_start); *p++ = '\t'; p = put_u64(p, x.text_end); }
        const uint32_t f[8] = {x.clip_lo, x.clip_hi, x.edits, x.n_match, x.n_mismatch, x.n_ins, x.n_del, x.band_hit};
        for (uint32_t v : f) { *p++ = '\t'; p = put_u64(p, v); }
        *p++ = '\t';
        if (none || op_off[i + 1] == op_off[i]) *p++ = '*';
        for (uint64_t o = op_off[i]; o < op_off[i + 1]; o++) {
            const uint32_t op = ops[o] & 15u;
            p = put_u64(p, ops[o] >> 4);
            *p++ = op == PGX_ALIGN_OP_I ? 'I' : (op == PGX_ALIGN_OP_D ? 'D' : (op == PGX_ALIGN_OP_S ? 'S' : (op == PGX_ALIGN_OP_EQ ? '=' : 'X')));
        }
        *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --gaf: one GAF line per read of a batch, appended to out, from the align records with their operations and the walk records with their steps; len[i] =
// bytes of read i.  A read without steps prints its number, its length, * in columns 3 to 11 and 255.  The S operations stay out of cg:Z: columns 3 and 4 state them.
// Column 12 of a read with steps is 255, "missing", or under --mapq (mapqs != nullptr) the read's mapping quality.
static void format_gaf(const pgx_read_align *recs, const uint64_t *op_off, const uint32_t *ops, const pgx_read_walk *walks, const uint64_t *step_off, const uint64_t *steps,
                       const uint64_t *read_off, const pgx_read_mapq *mapqs, size_t n, uint64_t first_seq, std::string &out) {
    out.resize(n * (13 * 21 + 40) + (size_t)(op_off[n] - op_off[0]) * 11 + (size_t)(step_off[n] - step_off[0]) * 21);
    char *p = &out[0];
    for (size_t i = 0; i < n; i++) {
        const pgx_read_align &x = recs[i];
        const pgx_read_walk &w = walks[i];
        const uint64_t len = read_off[i + 1] - read_off[i];
        p = put_u64(p, first_seq + i + 1); *p++ = '\t';
        p = put_u64(p, len);
        if (w.n_steps == 0) {
            for (int k = 0; k < 9; k++) { *p++ = '\t'; *p++ = '*'; }
            p = put_str(p, "\t255\n");
            continue;
        }
        *p++ = '\t'; p = put_u64(p, x.clip_lo);
        *p++ = '\t'; p = put_u64(p, len - x.clip_hi);
        p = put_str(p, "\t+\t");
        for (uint64_t o = step_off[i]; o < step_off[i + 1]; o++) { *p++ = (steps[o] & 1) ? '<' : '>'; p = put_u64(p, steps[o] >> 1); }
        const uint64_t f[5] = {w.path_len, w.path_start, w.path_end, x.n_match, (uint64_t)x.n_match + x.n_mismatch + x.n_ins + x.n_del};
        for (uint64_t v : f) { *p++ = '\t'; p = put_u64(p, v); }
        *p++ = '\t'; p = put_u64(p, mapqs ? mapqs[i].mapq : 255u);
        p = put_str(p, "\tNM:i:"); p = put_u64(p, x.edits);
        p = put_str(p, "\ths:i:"); p = put_u64(p, x.seq);
        p = put_str(p, "\tho:i:"); p = put_u64(p, x.text_start);
        p = put_str(p, "\tcg:Z:");
        for (uint64_t o = op_off[i]; o < op_off[i + 1]; o++) {
            const uint32_t op = ops[o] & 15u;
            if (op == PGX_ALIGN_OP_S) continue;
            p = put_u64(p, ops[o] >> 4);
            *p++ = op == PGX_ALIGN_OP_I ? 'I' : (op == PGX_ALIGN_OP_D ? 'D' : (op == PGX_ALIGN_OP_EQ ? '=' : 'X'));
        }
        *p++ = '\n';
    }
    out.resize((size_t)(p - &out[0]));
}

// --pack: every device's pack finished, the vectors summed (modulo 2^32, like the device's own sums), the summary recomputed from the sum, the two
// files written.  Returns the error, or an empty string.
static std::string write_packs(const std::map<int, pgx_pack *> &packs, const std::string &file, const std::string &bases_file) {
    std::vector<uint32_t> cov, len;
    std::vector<uint64_t> base;
    for (const auto &kv : packs) {
        pgx_pack_result r;
        if (pgx_pack_finish(kv.second, &r) != PGX_OK) return pgx_last_error();
        if (base.empty()) {
            base.assign(r.node_base, r.node_base + r.n_nodes + 1);
            len.assign(r.node_length, r.node_length + r.n_nodes);
            cov.assign(r.cov, r.cov + r.n_bases);
        } else {
            if (r.n_nodes + 1 != base.size() || r.n_bases != cov.size()) return "find_mems --pack: the packs of two devices describe different graphs";
            for (uint64_t g = 0; g < r.n_bases; g++) cov[g] += r.cov[g];
        }
    }
    // the node file is a line a node and is built in memory; the base file is a line a covered base and is streamed through its FILE's buffer
    std::FILE *bfp = nullptr;
    if (!bases_file.empty()) {
        bfp = std::fopen(bases_file.c_str(), "wb");
        if (!bfp) return "Cannot open pack-bases file: " + bases_file;
        std::fputs("#node\toffset\tcoverage\n", bfp);
    }
    std::string out = "#node\tlength\tcovered\tsum\tmax\n";
    char line[128];
    for (size_t id = 0; id < len.size(); id++) {
        if (!len[id]) continue;
        uint64_t covered = 0, sum = 0;
        uint32_t mx = 0;
        for (uint32_t o = 0; o < len[id]; o++) {
            const uint32_t c = cov[base[id] + o];
            if (!c) continue;
            covered++; sum += c; mx = std::max(mx, c);
            if (bfp) std::fprintf(bfp, "%zu\t%u\t%u\n", id, o, c);
        }
        std::snprintf(line, sizeof line, "%zu\t%u\t%llu\t%llu\t%u\n", id, len[id], (unsigned long long)covered, (unsigned long long)sum, mx);
        out += line;
    }
    if (bfp) {
        const bool bad = std::ferror(bfp) != 0;
        if ((std::fclose(bfp) != 0) || bad) return "Cannot write pack-bases file: " + bases_file;
    }
    std::FILE *fp = std::fopen(file.c_str(), "wb");
    if (!fp) return "Cannot open pack file: " + file;
    const bool ok = std::fwrite(out.data(), 1, out.size(), fp) == out.size();
    if ((std::fclose(fp) != 0) || !ok) return "Cannot write pack file: " + file;
    return "";
}

static int usage() {
    std::cerr << "usage: find_mems <r_index.ri> <tags> <reads.txt> <min_mem_length> <min_occ>"
                 " [--device N | --gpus N | --devices a,b,..] [--streams W] [--mode compat|strict] [--batch N]"
                 " [--tags-format auto|bytecode|compact] [--quiet] [--reads-format lines|fasta|fastq|auto] [--device-parse]"
                 " [--locate positions|seqs] [--locate-max K] [--result full|compact] [--format host|device]"
                 " [--hits FILE [--hits-max K] [--hits-only (not with --locate)]]"
                 " [--place FILE [--place-max K] [--place-only (not with --locate)]]"
                 " [--verify FILE [--verify-max C] [--verify-mismatch P] [--verify-only (not with --locate)]]"
                 " [--align FILE [--align-band W (0 .. 31)] [--align-only (not with --locate)]]"
                 " [--gaf FILE [--gaf-only (not with --locate)]]"
                 " [--paired [--frag-min A] [--frag-max B] [--mates-penalty U] [--mates FILE [--mates-only (not with --locate)]]"
                 " [--rescue [--rescue-min S] [--rescue-anchors R (1 .. 8)] [--rescued FILE]]]"
                 " [--mapq (with --gaf or --mapq-file) [--mapq-scale D (1 .. 16)] [--mapq-slack K (0 .. 1024)] [--mapq-extra X (0 .. 63)] [--mapq-file FILE]]"
                 " [--pack FILE [--pack-bases FILE2] [--pack-min-mapq Q (1 .. 60, with --mapq)] [--pack-only (not with --locate)]]" << std::endl;
    return EXIT_FAILURE;
}

int main(int argc, char **argv) {
    if (argc < 6) return usage();
    const std::string r_index_file = argv[1], tag_array_index = argv[2], reads_file = argv[3];
    const size_t mem_length = (size_t)std::stoi(argv[4]); // find_mems.cpp:17 (std::stoi -> size_t)
    const size_t min_occ = (size_t)std::stoi(argv[5]);
    std::vector<int> devices(1, 0);
    uint32_t mode = PGX_MODE_COMPAT, tfmt = PGX_TAGS_AUTO;
    size_t batch_reads = 1u << 18; // (reads per batch.  The device alone would like 2^20 -- fresh batches 177 M reads/s at 2^18, 278 M at 2^20, profiles/r04_batch_size_sweep.txt --, but this program is bound by its own host stages: 16 M reads take 0.5-0.7 s with 2^18 and 2.7-2.9 s with 2^20, pinned buffers of 150 MB per job and the formatting of the first and last batch: profiles/r04_cli_e2e.txt)
    unsigned streams = 3;
    bool quiet = false, device_parse = false, mode_given = false;
    std::string reads_format = "lines";
    int locate_mode = LOCATE_NONE;
    uint64_t locate_max = 0;
    bool compact_result = false;
    bool format_device = false; // --format device: stdout and the per-read stderr lines come from pgx_batch_format
    std::string hits_file;      // --hits: the read hits of every batch go to this file
    uint64_t hits_max = 0;
    bool hits_max_given = false, hits_only = false;
    std::string place_file;     // --place: the read placements of every batch go to this file
    uint64_t place_max = 0;
    bool place_max_given = false, place_only = false;
    std::string verify_file;    // --verify: the verified placements of every batch go to this file
    uint32_t verify_max = 1, verify_penalty = 4;
    bool verify_opt_given = false, verify_only = false;
    std::string align_file;     // --align: the gapped alignments of every batch go to this file
    uint32_t align_band = 8;
    bool align_band_given = false, align_only = false;
    std::string gaf_file;       // --gaf: the graph walks of every batch go to this file, one GAF line per read
    bool gaf_only = false;
    bool paired = false;        // --paired: records 2k and 2k + 1 of the reads file are mates; the mates stage elects the verify winners
    std::string mates_file;     // --mates: the pair records of every batch go to this file
    int64_t frag_min = 0, frag_max = 1000;
    uint64_t mates_penalty = 0;
    bool mates_opt_given = false, mates_penalty_given = false, mates_only = false, verify_max_given = false;
    bool rescue = false;        // --rescue: pgx_batch_read_rescue with PGX_RESCUE_MERGE between verify and mates
    std::string rescued_file;   // --rescued: the rescue records of every batch go to this file
    uint64_t rescue_min = 0, rescue_anchors = 2;
    bool rescue_opt_given = false, rescue_min_given = false;
    bool mapq = false;          // --mapq: pgx_batch_read_mapq behind verify (and rescue and mates); column 12 of the GAF lines
    std::string mapq_file;      // --mapq-file: the mapq records of every batch go to this file
    uint32_t mapq_scale = 2, mapq_slack = 8, mapq_extra = 16;
    bool mapq_opt_given = false;
    std::string pack_file;      // --pack: the per-node coverage summary, written once at the end
    std::string pack_bases_file; // --pack-bases: one line per covered base
    uint32_t pack_min_mapq = 0;
    bool pack_min_mapq_given = false, pack_only = false;
    int first_opt = 6;
    // find_mems_chunked.cpp:15-28 takes an optional sixth positional (chunk_size_mb of its memory-mapped loader): accepted, unused
    if (argc > 6 && argv[6][0] >= '0' && argv[6][0] <= '9') first_opt = 7;
    for (int i = first_opt; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::cerr << "missing value for " << a << std::endl; std::exit(EXIT_FAILURE); } return argv[++i]; };
        if (a == "--device") devices.assign(1, std::stoi(next()));
        else if (a == "--gpus") { const int g = std::stoi(next()); devices.clear(); for (int d = 0; d < std::max(1, g); d++) devices.push_back(d); }
        else if (a == "--devices") {
            devices.clear();
            std::stringstream ss(next());
            for (std::string tok; std::getline(ss, tok, ',');) if (!tok.empty()) devices.push_back(std::stoi(tok));
            if (devices.empty()) { std::cerr << "--devices: empty list" << std::endl; return EXIT_FAILURE; }
        }
        else if (a == "--streams") streams = (unsigned)std::max(1, std::stoi(next()));
        else if (a == "--mode") { mode = next() == "strict" ? PGX_MODE_STRICT : PGX_MODE_COMPAT; mode_given = true; }
        else if (a == "--batch") batch_reads = (size_t)std::stoull(next());
        else if (a == "--tags-format") { const std::string f = next(); tfmt = f == "bytecode" ? PGX_TAGS_BYTECODE : f == "compact" ? PGX_TAGS_COMPACT : PGX_TAGS_AUTO; }
        else if (a == "--quiet") quiet = true;
        else if (a == "--reads-format") {
            reads_format = next();
            if (reads_format != "lines" && reads_format != "fasta" && reads_format != "fastq" && reads_format != "auto") {
                std::cerr << "--reads-format: lines, fasta, fastq or auto" << std::endl;
                return EXIT_FAILURE;
            }
        }
        else if (a == "--device-parse") device_parse = true;
        else if (a == "--locate") {
            const std::string f = next();
            if (f == "positions") locate_mode = LOCATE_POSITIONS;
            else if (f == "seqs") locate_mode = LOCATE_SEQS;
            else { std::cerr << "--locate: positions or seqs" << std::endl; return EXIT_FAILURE; }
        }
        else if (a == "--locate-max") {
            const std::string f = next();
            errno = 0;
            char *endp = nullptr;
            const unsigned long long k = f.empty() || f.size() > 19 || f.find_first_not_of("0123456789") != std::string::npos ? 0 : std::strtoull(f.c_str(), &endp, 10);
            if (!endp || *endp || errno) { std::cerr << "--locate-max: a number of occurrences >= 0 (0: no cap)" << std::endl; return EXIT_FAILURE; }
            locate_max = k;
        }
        else if (a == "--result") {
            const std::string f = next();
            if (f == "compact") compact_result = true;
            else if (f == "full") compact_result = false;
            else { std::cerr << "--result: full or compact" << std::endl; return EXIT_FAILURE; }
        }
        else if (a == "--format") {
            const std::string f = next();
            if (f == "device") format_device = true;
            else if (f == "host") format_device = false;
            else { std::cerr << "--format: host or device" << std::endl; return EXIT_FAILURE; }
        }
        else if (a == "--hits") { hits_file = next(); if (hits_file.empty()) { std::cerr << "--hits: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--hits-max") {
            const std::string f = next();
            errno = 0;
            char *endp = nullptr;
            const unsigned long long k = f.empty() || f.size() > 19 || f.find_first_not_of("0123456789") != std::string::npos ? 0 : std::strtoull(f.c_str(), &endp, 10);
            if (!endp || *endp || errno) { std::cerr << "--hits-max: a number of occurrences >= 0 (0: no cap)" << std::endl; return EXIT_FAILURE; }
            hits_max = k;
            hits_max_given = true;
        }
        else if (a == "--hits-only") hits_only = true;
        else if (a == "--place") { place_file = next(); if (place_file.empty()) { std::cerr << "--place: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--place-max") {
            const std::string f = next();
            errno = 0;
            char *endp = nullptr;
            const unsigned long long k = f.empty() || f.size() > 19 || f.find_first_not_of("0123456789") != std::string::npos ? 0 : std::strtoull(f.c_str(), &endp, 10);
            if (!endp || *endp || errno) { std::cerr << "--place-max: a number of occurrences >= 0 (0: no cap)" << std::endl; return EXIT_FAILURE; }
            place_max = k;
            place_max_given = true;
        }
        else if (a == "--place-only") place_only = true;
        else if (a == "--verify") { verify_file = next(); if (verify_file.empty()) { std::cerr << "--verify: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--verify-max" || a == "--verify-mismatch") {
            const std::string v = next();
            char *endp = nullptr;
            errno = 0;
            const unsigned long long k = v.empty() || v[0] == '-' ? 0 : std::strtoull(v.c_str(), &endp, 10);
            const unsigned long long top = a == "--verify-max" ? PGX_VERIFY_MAX_CAND : PGX_VERIFY_MAX_PENALTY;
            if (!endp || *endp || errno || k < 1 || k > top) { std::cerr << a << ": a number in 1 .. " << top << std::endl; return EXIT_FAILURE; }
            (a == "--verify-max" ? verify_max : verify_penalty) = (uint32_t)k;
            verify_opt_given = true;
            if (a == "--verify-max") verify_max_given = true;
        }
        else if (a == "--verify-only") verify_only = true;
        else if (a == "--align") { align_file = next(); if (align_file.empty()) { std::cerr << "--align: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--align-band") {
            const std::string v = next();
            char *endp = nullptr;
            errno = 0;
            const unsigned long long k = v.empty() || v[0] == '-' ? ~0ull : std::strtoull(v.c_str(), &endp, 10);
            if (!endp || *endp || errno || k > PGX_ALIGN_MAX_BAND) return usage();
            align_band = (uint32_t)k;
            align_band_given = true;
        }
        else if (a == "--align-only") align_only = true;
        else if (a == "--gaf") { gaf_file = next(); if (gaf_file.empty()) { std::cerr << "--gaf: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--gaf-only") gaf_only = true;
        else if (a == "--paired") paired = true;
        else if (a == "--mates") { mates_file = next(); if (mates_file.empty()) { std::cerr << "--mates: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--mates-only") mates_only = true;
        else if (a == "--frag-min" || a == "--frag-max") {
            const std::string v = next();
            char *endp = nullptr;
            errno = 0;
            const long long k = v.empty() ? 0 : std::strtoll(v.c_str(), &endp, 10);
            if (!endp || *endp || errno) { std::cerr << a << ": a fragment length (a signed number)" << std::endl; return EXIT_FAILURE; }
            (a == "--frag-min" ? frag_min : frag_max) = (int64_t)k;
            mates_opt_given = true;
        }
        else if (a == "--mates-penalty") {
            const std::string v = next();
            char *endp = nullptr;
            errno = 0;
            const unsigned long long k = v.empty() || v[0] == '-' ? 0 : std::strtoull(v.c_str(), &endp, 10);
            if (!endp || *endp || errno || k > 0xFFFFFFFFull) { std::cerr << a << ": a number in 0 .. 4294967295" << std::endl; return EXIT_FAILURE; }
            mates_penalty = k;
            mates_opt_given = mates_penalty_given = true;
        }
        else if (a == "--rescue") rescue = true;
        else if (a == "--rescued") { rescued_file = next(); if (rescued_file.empty()) { std::cerr << "--rescued: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--rescue-min" || a == "--rescue-anchors") {
            const bool is_min = a == "--rescue-min";
            const std::string v = next();
            char *endp = nullptr;
            errno = 0;
            const unsigned long long k = v.empty() || v[0] == '-' ? 0 : std::strtoull(v.c_str(), &endp, 10);
            if (!endp || *endp || errno || k < 1 || k > (is_min ? 0xFFFFFFFFull : (unsigned long long)PGX_RESCUE_MAX_ANCHORS)) {
                std::cerr << a << (is_min ? ": a number in 1 .. 4294967295" : ": a number in 1 .. 8") << std::endl;
                return EXIT_FAILURE;
            }
            (is_min ? rescue_min : rescue_anchors) = k;
            rescue_opt_given = true;
            if (is_min) rescue_min_given = true;
        }
        else if (a == "--mapq") mapq = true;
        else if (a == "--pack") { pack_file = next(); if (pack_file.empty()) { std::cerr << "--pack: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--pack-bases") { pack_bases_file = next(); if (pack_bases_file.empty()) { std::cerr << "--pack-bases: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--pack-only") pack_only = true;
        else if (a == "--pack-min-mapq") {
            const std::string v = next();
            char *end = nullptr;
            const unsigned long long k = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] == '-' || k < 1 || k > 60) { std::cerr << "--pack-min-mapq: an integer 1 .. 60, got '" << v << "'" << std::endl; return EXIT_FAILURE; }
            pack_min_mapq = (uint32_t)k;
            pack_min_mapq_given = true;
        }
        else if (a == "--mapq-file") { mapq_file = next(); if (mapq_file.empty()) { std::cerr << "--mapq-file: a file name" << std::endl; return EXIT_FAILURE; } }
        else if (a == "--mapq-scale" || a == "--mapq-slack" || a == "--mapq-extra") {
            const unsigned long long lo = a == "--mapq-scale" ? 1 : 0, hi = a == "--mapq-scale" ? PGX_MAPQ_MAX_SCALE : (a == "--mapq-slack" ? PGX_MAPQ_MAX_SLACK : PGX_MAPQ_MAX_EXTRA);
            const std::string v = next();
            char *endp = nullptr;
            errno = 0;
            const unsigned long long k = v.empty() || v[0] == '-' ? ~0ull : std::strtoull(v.c_str(), &endp, 10);
            if (!endp || *endp || errno || k < lo || k > hi) {
                std::cerr << a << ": a number in " << lo << " .. " << hi << std::endl;
                return EXIT_FAILURE;
            }
            (a == "--mapq-scale" ? mapq_scale : (a == "--mapq-slack" ? mapq_slack : mapq_extra)) = (uint32_t)k;
            mapq_opt_given = true;
        }
        else { std::cerr << "unknown option " << a << std::endl; return EXIT_FAILURE; }
    }
    if ((mapq_opt_given || !mapq_file.empty()) && !mapq) return usage(); // (the mapq options belong to --mapq ...
    if (mapq && gaf_file.empty() && mapq_file.empty() && pack_file.empty()) return usage(); // ... and --mapq to an output that shows or uses it)
    if ((!pack_bases_file.empty() || pack_min_mapq_given || pack_only) && pack_file.empty()) return usage(); // (the pack options belong to --pack)
    if (pack_min_mapq_given && !mapq) return usage();                                                        // (a filter on qualities needs them)
    if (pack_only && locate_mode) { std::cerr << "--pack-only makes no MEM text: it does not go with --locate" << std::endl; return EXIT_FAILURE; }
    if (rescue && !paired) return usage();                                     // (the rescue options belong to --paired ...
    if ((!rescued_file.empty() || rescue_opt_given) && !rescue) return usage(); // ... and its own to --rescue)
    if (rescue && !rescue_min_given) rescue_min = mem_length ? std::min<uint64_t>(mem_length, 0xFFFFFFFFull) : 1; // (no less evidence than a placed read: a MEM of that length)
    if (rescue && (uint64_t)frag_max - (uint64_t)frag_min >= (uint64_t)PGX_RESCUE_MAX_WINDOW && frag_min <= frag_max) {
        std::cerr << "--rescue: --frag-min " << frag_min << " .. --frag-max " << frag_max << " is a window of more than " << PGX_RESCUE_MAX_WINDOW << " diagonals" << std::endl;
        return EXIT_FAILURE;
    }
    if ((!mates_file.empty() || mates_only || mates_opt_given) && !paired) return usage(); // (the mates options belong to --paired)
    if (mates_only && mates_file.empty()) return usage();
    if (mates_only && locate_mode) { std::cerr << "--mates-only makes no MEM text: it does not go with --locate" << std::endl; return EXIT_FAILURE; }
    if (paired && frag_min > frag_max) { std::cerr << "--frag-min " << frag_min << " exceeds --frag-max " << frag_max << std::endl; return EXIT_FAILURE; }
    if ((paired || mapq) && !verify_max_given) verify_max = 16; // (a pair chooses among candidates, a quality counts them: one a read leaves nothing to choose or count)
    if (paired && !mates_penalty_given) mates_penalty = 2ull * (verify_penalty + 1); // two substitutions' worth of seg_score: each costs a match and P
    if ((hits_max_given || hits_only) && hits_file.empty()) return usage();
    if (hits_only && locate_mode) { std::cerr << "--hits-only makes no MEM text: it does not go with --locate" << std::endl; return EXIT_FAILURE; }
    if ((place_max_given || place_only) && place_file.empty()) return usage();
    if (place_only && locate_mode) { std::cerr << "--place-only makes no MEM text: it does not go with --locate" << std::endl; return EXIT_FAILURE; }
    if ((verify_only && verify_file.empty()) || (verify_opt_given && verify_file.empty() && align_file.empty() && gaf_file.empty() && pack_file.empty() && !paired && !mapq)) return usage();
    if (verify_only && locate_mode) { std::cerr << "--verify-only makes no MEM text: it does not go with --locate" << std::endl; return EXIT_FAILURE; }
    if ((align_only && align_file.empty()) || (align_band_given && align_file.empty() && gaf_file.empty() && pack_file.empty())) return usage();
    if (gaf_only && gaf_file.empty()) return usage();
    if (gaf_only && locate_mode) { std::cerr << "--gaf-only makes no MEM text: it does not go with --locate" << std::endl; return EXIT_FAILURE; }
    if (align_only && locate_mode) { std::cerr << "--align-only makes no MEM text: it does not go with --locate" << std::endl; return EXIT_FAILURE; }
    const bool want_hits = !hits_file.empty(), want_places = !place_file.empty(), want_verify = !verify_file.empty(), want_align = !align_file.empty();
    const bool want_gaf = !gaf_file.empty(), want_pack = !pack_file.empty();
    const bool run_align = want_align || want_gaf || want_pack; // (--gaf and --pack run the align stage themselves)
    const bool want_mates = !mates_file.empty(), want_rescued = !rescued_file.empty(), want_mapqs = !mapq_file.empty();
    const bool run_verify = want_verify || run_align || paired || mapq; // (--align runs the verify stage itself; --paired elects its winners; --mapq reads its list)
    const uint32_t place_flags = run_verify && (verify_max > 1 || paired || mapq) ? PGX_PLACE_LIST : 0u; // (the candidates beyond the first, and the extras of --mapq, come from the list)
    const uint32_t verify_flags = paired || mapq ? PGX_VERIFY_LIST : 0u;                                 // (the mates and the mapq stage read the candidates)
    const uint32_t mapq_flags = paired ? PGX_MAPQ_PAIRED : 0u;
    const bool no_text = hits_only || place_only || verify_only || align_only || gaf_only || mates_only || pack_only; // (either one: no tag stage, no download of result arrays, stdout empty)
    if (batch_reads == 0) batch_reads = 1;
    if (locate_max && !locate_mode) { std::cerr << "--locate-max needs --locate" << std::endl; return EXIT_FAILURE; }

    auto time1 = std::chrono::high_resolution_clock::now();
    double total_mem_time = 0.0, total_tag_time = 0.0;

    std::cerr << "Reading the rindex file (encoded)" << std::endl;
    {
        std::ifstream rin(r_index_file, std::ios::binary);
        if (!rin) { std::cerr << "Cannot open r-index: " << r_index_file << std::endl; std::exit(EXIT_FAILURE); } // :30
    }
    const bool from_image = is_image_file(r_index_file.c_str());
    // --gaf or --mapq with "-" for the tags of a .ri: the index opens without tags and the walk image's own refusal ends the run below, before any batch
    const bool gaf_no_tags = !from_image && (!gaf_file.empty() || mapq || want_pack) && tag_array_index == "-";
    if (!from_image && !gaf_no_tags) {
        std::ifstream tin(tag_array_index, std::ios::binary);
        if (!tin) { std::cerr << "Cannot open tag array: " << tag_array_index << std::endl; std::exit(EXIT_FAILURE); }
    }
    pgx_index *h = nullptr;
    if (from_image) {
        if (open_image_index(r_index_file.c_str(), tag_array_index.c_str(), mode_given, mode, &h)) return EXIT_FAILURE;
    } else if (pgx_index_open(r_index_file.c_str(), gaf_no_tags ? nullptr : tag_array_index.c_str(), tfmt, mode, &h) != PGX_OK) {
        std::cerr << pgx_last_error() << std::endl; // reference: uncaught sdsl::simple_sds::InvalidData
        return EXIT_FAILURE;
    }
    LocateOut locate_out;
    locate_out.mode = locate_mode;
    if (locate_mode) {
        pgx_index_info info;
        if (pgx_index_info_get(h, &info) != PGX_OK) { std::cerr << pgx_last_error() << std::endl; return EXIT_FAILURE; }
        locate_out.max_length = info.max_length ? info.max_length : 1;
    }
    const uint32_t locate_flags = locate_mode == LOCATE_SEQS ? (PGX_LOCATE_SEQ_IDS | PGX_LOCATE_UNIQUE) : 0u;
    auto time2 = std::chrono::high_resolution_clock::now();
    std::cerr << "Loading r-index into memory took " << std::chrono::duration<double>(time2 - time1).count() << " seconds" << std::endl;
    std::cerr << "Reading the tag array index" << std::endl;
    for (int d : devices) // the index is replicated: one image per distinct device
        if (pgx_index_to_device(h, d) != PGX_OK) { std::cerr << pgx_last_error() << std::endl; return EXIT_FAILURE; }
    auto time3 = std::chrono::high_resolution_clock::now();
    std::cerr << "Loading tag arrays took " << std::chrono::duration<double>(time3 - time2).count() << " seconds" << std::endl;
    // --hits: whether this index serves sequence sets at all is the library's to say, so ask it with a batch of one read before anything
    // is produced (more than 4096 sequences, a COMPAT index without N, an image file without the locate image)
    std::FILE *hits_fp = nullptr;
    if (want_hits) {
        static const uint8_t probe_read[4] = {'A', 'C', 'G', 'T'};
        static const uint64_t probe_offs[2] = {0, 4};
        pgx_batch *pb = nullptr;
        pgx_status st = pgx_batch_create(h, devices[0], probe_read, probe_offs, 1, &pb);
        if (st == PGX_OK) st = pgx_batch_run(pb, mem_length, min_occ, 0, nullptr);
        if (st == PGX_OK) st = pgx_batch_locate(pb, PGX_LOCATE_SEQ_SETS, hits_max, nullptr);
        if (st == PGX_OK) st = pgx_batch_read_hits(pb, 0, nullptr);
        const std::string msg = st == PGX_OK ? "" : pgx_last_error();
        pgx_batch_free(pb);
        if (st != PGX_OK) { std::cerr << msg << (st == PGX_ERR_UNSUPPORTED ? " (find_mems --hits)" : "") << std::endl; return EXIT_FAILURE; }
        hits_fp = std::fopen(hits_file.c_str(), "wb");
        if (!hits_fp) { std::cerr << "Cannot open hits file: " << hits_file << std::endl; return EXIT_FAILURE; }
        std::fwrite(HITS_HEADER, 1, sizeof HITS_HEADER - 1, hits_fp);
    }
    // --place: the same question for the packed positions (a COMPAT index without N, an image file without the locate image)
    std::FILE *place_fp = nullptr;
    if (want_places) {
        static const uint8_t probe_read[4] = {'A', 'C', 'G', 'T'};
        static const uint64_t probe_offs[2] = {0, 4};
        pgx_batch *pb = nullptr;
        pgx_status st = pgx_batch_create(h, devices[0], probe_read, probe_offs, 1, &pb);
        if (st == PGX_OK) st = pgx_batch_run(pb, mem_length, min_occ, 0, nullptr);
        if (st == PGX_OK) st = pgx_batch_locate(pb, 0, place_max, nullptr);
        if (st == PGX_OK) st = pgx_batch_read_place(pb, 0, nullptr);
        const std::string msg = st == PGX_OK ? "" : pgx_last_error();
        pgx_batch_free(pb);
        if (st != PGX_OK) {
            std::cerr << msg << (st == PGX_ERR_UNSUPPORTED ? " (find_mems --place)" : "") << std::endl;
            if (hits_fp) std::fclose(hits_fp);
            return EXIT_FAILURE;
        }
        place_fp = std::fopen(place_file.c_str(), "wb");
        if (!place_fp) { std::cerr << "Cannot open place file: " << place_file << std::endl; return EXIT_FAILURE; }
        std::fwrite(PLACE_HEADER, 1, sizeof PLACE_HEADER - 1, place_fp);
    }
    // --verify: the same question for the text image (what --place asks, and a collection of 2^32 - 2^20 symbols or more)
    std::FILE *verify_fp = nullptr, *align_fp = nullptr, *gaf_fp = nullptr, *mates_fp = nullptr, *rescued_fp = nullptr, *mapq_fp = nullptr;
    std::map<int, pgx_pack *> packs; // --pack: one per distinct device, made here (the walk image: an index without tags ends the run before any batch)
    auto free_packs = [&]() { for (auto &kv : packs) pgx_pack_free(kv.second); packs.clear(); };
    if (run_verify) {
        static const uint8_t probe_read[4] = {'A', 'C', 'G', 'T'};
        static const uint64_t probe_offs[2] = {0, 4};
        pgx_status st = PGX_OK;
        std::string msg;
        bool twin_refused = false;
        for (size_t i = 0; st == PGX_OK && i < devices.size(); i++) { // (the text image of every device is built here, before any batch)
            pgx_batch *pb = nullptr;
            st = pgx_batch_create(h, devices[i], probe_read, probe_offs, 1, &pb);
            if (st == PGX_OK) st = pgx_batch_run(pb, mem_length, min_occ, 0, nullptr);
            if (st == PGX_OK) st = pgx_batch_locate(pb, 0, place_max, nullptr);
            if (st == PGX_OK) st = pgx_batch_read_place(pb, place_flags, nullptr);
            if (st == PGX_OK) st = pgx_batch_read_verify(pb, verify_max, verify_penalty, verify_flags, nullptr);
            if (st == PGX_OK && paired) { // (a probe of one read is no pair: ask the index itself)
                uint64_t bad = 0;
                st = pgx_index_twinned(h, devices[i], &bad);
                if (st == PGX_OK && bad != ~0ull) {
                    msg = "find_mems --paired: the index is not twinned (p = " + std::to_string(bad) + "): mates need a collection with every path forward as sequence 2p and reversed as 2p + 1 (gbz_extract -b)";
                    twin_refused = true;
                    st = PGX_ERR_UNSUPPORTED;
                }
            }
            if (st == PGX_OK && run_align) st = pgx_batch_read_align(pb, align_band, PGX_ALIGN_CIGAR, nullptr);
            if (st == PGX_OK && want_gaf) st = pgx_batch_read_walk(pb, PGX_WALK_STEPS, nullptr); // (the walk image: an index without tags ends here)
            if (st == PGX_OK && mapq) st = pgx_batch_read_mapq(pb, mapq_scale, mapq_slack, mapq_extra, 0u, nullptr); // (the same image; a probe of one read is no pair)
            if (st == PGX_OK && want_pack && !packs.count(devices[i])) {
                pgx_pack *pk = nullptr;
                st = pgx_pack_create(h, devices[i], &pk);
                if (st == PGX_OK) packs[devices[i]] = pk;
            }
            if (st != PGX_OK && !twin_refused) msg = pgx_last_error();
            pgx_batch_free(pb);
        }
        if (st != PGX_OK) {
            std::cerr << msg
                      << (st != PGX_ERR_UNSUPPORTED || twin_refused ? "" : (want_verify ? " (find_mems --verify)" : (want_align ? " (find_mems --align)" : (want_gaf ? " (find_mems --gaf)" : (mapq ? " (find_mems --mapq)" : (want_pack ? " (find_mems --pack)" : " (find_mems --paired)"))))))
                      << std::endl;
            if (hits_fp) std::fclose(hits_fp);
            if (place_fp) std::fclose(place_fp);
            free_packs();
            return EXIT_FAILURE;
        }
        if (want_verify) {
            verify_fp = std::fopen(verify_file.c_str(), "wb");
            if (!verify_fp) { std::cerr << "Cannot open verify file: " << verify_file << std::endl; return EXIT_FAILURE; }
            std::fwrite(VERIFY_HEADER, 1, sizeof VERIFY_HEADER - 1, verify_fp);
        }
        if (want_align) {
            align_fp = std::fopen(align_file.c_str(), "wb");
            if (!align_fp) { std::cerr << "Cannot open align file: " << align_file << std::endl; return EXIT_FAILURE; }
            std::fwrite(ALIGN_HEADER, 1, sizeof ALIGN_HEADER - 1, align_fp);
        }
        if (want_gaf) {
            gaf_fp = std::fopen(gaf_file.c_str(), "wb");
            if (!gaf_fp) { std::cerr << "Cannot open gaf file: " << gaf_file << std::endl; return EXIT_FAILURE; }
        }
        if (want_mates) {
            mates_fp = std::fopen(mates_file.c_str(), "wb");
            if (!mates_fp) { std::cerr << "Cannot open mates file: " << mates_file << std::endl; return EXIT_FAILURE; }
            std::fwrite(MATES_HEADER, 1, sizeof MATES_HEADER - 1, mates_fp);
        }
        if (want_rescued) {
            rescued_fp = std::fopen(rescued_file.c_str(), "wb");
            if (!rescued_fp) { std::cerr << "Cannot open rescued file: " << rescued_file << std::endl; return EXIT_FAILURE; }
            std::fwrite(RESCUED_HEADER, 1, sizeof RESCUED_HEADER - 1, rescued_fp);
        }
        if (want_mapqs) {
            mapq_fp = std::fopen(mapq_file.c_str(), "wb");
            if (!mapq_fp) { std::cerr << "Cannot open mapq file: " << mapq_file << std::endl; return EXIT_FAILURE; }
            std::fwrite(MAPQ_HEADER, 1, sizeof MAPQ_HEADER - 1, mapq_fp);
        }
    }

    // ---- the reads file, mapped: the reference reads it with std::getline (find_mems.cpp:96); here a planner cuts it into byte ranges that
    //      end at a newline, PARSE threads turn ranges into batches side by side (line splitting was what bounded the single reader thread of
    //      round 2 at ~1 GB/s), device workers take the batches in file order ----
    struct MappedFile {
        const char *p = nullptr;
        size_t n = 0;
        std::vector<char> own; // fallback when the file cannot be mapped (a pipe, a FIFO)
        int fd = -1;
        bool mapped = false;
        ~MappedFile() { if (mapped) ::munmap(const_cast<char *>(p), n); if (fd >= 0) ::close(fd); }
    } mf;
    {
        mf.fd = ::open(reads_file.c_str(), O_RDONLY);
        if (mf.fd < 0) { std::cerr << "Cannot open reads file: " << reads_file << std::endl; std::exit(EXIT_FAILURE); } // :91
        struct stat st;
        if (::fstat(mf.fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
            void *m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, mf.fd, 0);
            if (m != MAP_FAILED) { mf.p = static_cast<const char *>(m); mf.n = (size_t)st.st_size; mf.mapped = true; (void)::madvise(m, mf.n, MADV_SEQUENTIAL); }
        }
        if (!mf.mapped) { // read it all (what the mapping would have paged in)
            char buf[1 << 16];
            for (;;) { const ssize_t k = ::read(mf.fd, buf, sizeof buf); if (k <= 0) break; mf.own.insert(mf.own.end(), buf, buf + k); }
            mf.p = mf.own.data(); mf.n = mf.own.size();
        }
    }

    // the format of the reads: FASTA and FASTQ are parsed on the device, line files there too with --device-parse
    uint32_t rfmt = PGX_READS_LINES;
    if (reads_format == "fasta") rfmt = PGX_READS_FASTA;
    else if (reads_format == "fastq") rfmt = PGX_READS_FASTQ;
    else if (reads_format == "auto" && mf.n) rfmt = mf.p[0] == '>' ? PGX_READS_FASTA : mf.p[0] == '@' ? PGX_READS_FASTQ : PGX_READS_LINES;
    const bool dev_parse = device_parse || rfmt != PGX_READS_LINES;
    static const char *const rfmt_name[3] = {"LINES", "FASTA", "FASTQ"};

    // ---- queues ----
    const unsigned n_workers = (unsigned)devices.size() * streams;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned n_fmt = std::max(1u, std::min(16u, hw / n_workers)); // formatting threads per batch
    unsigned n_parse = std::max(1u, std::min(8u, hw / 4));
    if (const char *e = std::getenv("PGX_CLI_PARSE_THREADS")) n_parse = (unsigned)std::max(1, std::atoi(e));
    std::mutex mu;
    std::condition_variable cv_jobs, cv_done, cv_space, cv_written;
    uint64_t written = 0;     // batches the writer is through with (--format device: their text may be overwritten)
    bool writer_done = false; // the writer has left its loop and reads no text any more
    std::map<uint64_t, std::unique_ptr<Job>> parsed;     // by id, waiting for a device worker
    std::map<uint64_t, std::unique_ptr<Done>> finished;
    bool reader_done = false, failed = false;
    uint64_t n_jobs = 0, next_write = 0, next_take = 0, next_seq_id = 0, seq_so_far = 0;
    std::map<uint64_t, uint64_t> counts;                  // reads of parsed ranges whose first_seq is not known yet
    std::map<uint64_t, uint64_t> first_seq_of;            // device-parsed ranges: first_seq, once every range before them has been counted
    const size_t max_ahead = 2 * n_workers + n_parse + 2; // ranges parsed or finished but not yet written (bounds memory)

    // ranges: about batch_reads reads each, by the length of the first lines (records: four lines of FASTQ, the '>' lines of FASTA)
    std::vector<std::pair<size_t, size_t>> ranges;
    {
        size_t probe = std::min<size_t>(mf.n, 1u << 16), lines = 0;
        for (size_t i = 0; i < probe; i++) lines += rfmt == PGX_READS_FASTA ? (mf.p[i] == '>' && (i == 0 || mf.p[i - 1] == '\n')) : mf.p[i] == '\n';
        if (rfmt == PGX_READS_FASTQ) lines /= 4;
        const double per_line = lines ? (double)probe / (double)lines : rfmt == PGX_READS_LINES ? 152.0 : (double)std::max<size_t>(probe, 1);
        const size_t want = (size_t)std::max(1.0, per_line * (double)batch_reads);
        size_t at = 0;
        while (!paired && at < mf.n) {
            size_t end = std::min(mf.n, at + want);
            if (end < mf.n && dev_parse) {
                uint64_t cut = mf.n;
                if (pgx_fastx_cut(reinterpret_cast<const uint8_t *>(mf.p), mf.n, rfmt, end, &cut) != PGX_OK) { std::cerr << pgx_last_error() << std::endl; return EXIT_FAILURE; }
                end = (size_t)cut;
            } else if (end < mf.n) {
                const char *nl = static_cast<const char *>(std::memchr(mf.p + end, '\n', mf.n - end));
                end = nl ? (size_t)(nl - mf.p) + 1 : mf.n;
            }
            ranges.emplace_back(at, end);
            at = end;
        }
        if (paired) {
            // --paired: every range holds whole pairs.  The cutter walks the file line by line, counts records while it cuts -- a non-empty line of a line
            // file, four lines of FASTQ (empty lines between records skipped), a '>' at a line start of FASTA -- and ends a range where a record ends,
            // the range holds an even number of them and at least `want` bytes.  Every cut lies where a record starts, so the device parser and
            // pgx_fastx_cut see whole records.
            const char *p = mf.p, *const stop = mf.p + mf.n;
            size_t in_range = 0, total = 0, fq_lines = 0;
            bool fa_open = false; // FASTA: a record has started and has not ended
            auto record_ends = [&](size_t e) { // a record ends at byte e
                in_range++; total++;
                if (in_range % 2 == 0 && e - at >= want) { ranges.emplace_back(at, e); at = e; in_range = 0; }
            };
            while (p < stop) {
                const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(stop - p)));
                const char *next = nl ? nl + 1 : stop;
                const size_t len = (size_t)((nl ? nl : stop) - p);
                if (rfmt == PGX_READS_LINES) { if (len) record_ends((size_t)(next - mf.p)); }
                else if (rfmt == PGX_READS_FASTQ) {
                    if (fq_lines || len) fq_lines++;
                    if (fq_lines == 4) { fq_lines = 0; record_ends((size_t)(next - mf.p)); }
                } else if (len && *p == '>') {
                    if (fa_open) record_ends((size_t)(p - mf.p));
                    fa_open = true;
                }
                p = next;
            }
            if (fa_open || fq_lines) { in_range++; total++; } // the last record of a FASTA file, a FASTQ record cut short (the parser says what is wrong with it)
            if (at < mf.n) ranges.emplace_back(at, mf.n);
            if (total % 2) {
                std::cerr << "find_mems --paired: " << reads_file << " holds " << total << " records, an odd number: records 2k and 2k + 1 are the mates of pair k" << std::endl;
                return EXIT_FAILURE;
            }
        }
    }
    n_jobs = ranges.size();
    std::atomic<uint64_t> next_range{0};

    // a range -> the reads it holds, concatenated, with offsets; empty lines are skipped (:97); a last line without a newline counts (std::getline)
    ReadBufPool pool;
    // PGX_CLI_PACKED=1: the parse threads also pack the reads to two bits per symbol (pgx_pack_reads) and the batch travels packed (pgx_batch_upload_packed).
    // Off by default: this program is bound by its host stages, not by the link -- 16 M reads, three device workers, same box: pipeline 0.65 s with byte
    // uploads, 0.88 s with packed ones (the extra pass over the bytes in the parse threads: profiles/r04_cli_e2e.txt).  A caller whose batches are already
    // packed, or whose pipeline is bound by the device, gains: bench.py fresh_batch 366 against 220 M reads/s.
    const bool use_packed = std::getenv("PGX_CLI_PACKED") && std::getenv("PGX_CLI_PACKED")[0] == '1';
    auto parse_range = [&](uint64_t id) {
        std::unique_ptr<Job> j(new Job());
        const char *q = mf.p + ranges[id].first, *end = mf.p + ranges[id].second;
        j->id = id;
        j->cat = pool.get((size_t)(end - q) + 1);
        if (dev_parse) { // the raw bytes, pinned: the device parses them (pgx_batch_upload_text)
            std::memcpy(j->cat.p, q, (size_t)(end - q));
            j->cat.len = (size_t)(end - q);
            return j;
        }
        j->offs.reserve((size_t)(end - q) / 100 + 16);
        j->offs.push_back(0);
        char *dst = j->cat.p;
        while (q < end) {
            const char *nl = static_cast<const char *>(std::memchr(q, '\n', (size_t)(end - q)));
            const size_t len = nl ? (size_t)(nl - q) : (size_t)(end - q);
            if (len) { std::memcpy(dst, q, len); dst += len; j->offs.push_back((uint64_t)(dst - j->cat.p)); }
            q += len + 1;
        }
        j->cat.len = (size_t)(dst - j->cat.p);
        // packed for the upload: a quarter of the bytes over the link and no pass over them on the device (PGX_CLI_PACKED=0: bytes as they are)
        if (use_packed && j->offs.size() > 1) {
            const size_t words = (j->cat.len + 15) / 16, side_cap = j->cat.len / 8 + 4096;
            j->pk = pool.get(words * 4 + side_cap);
            j->side_at = words * 4;
            j->side_ids.resize(side_cap / 64 + 64);
            uint64_t n_side = 0, n_side_bytes = 0;
            const pgx_status st = pgx_pack_reads(reinterpret_cast<const uint8_t *>(j->cat.p), j->offs.data(), j->offs.size() - 1, 1, reinterpret_cast<uint32_t *>(j->pk.p),
                                                 j->side_ids.data(), j->side_ids.size(), reinterpret_cast<uint8_t *>(j->pk.p) + j->side_at, side_cap, &n_side, &n_side_bytes);
            if (st == PGX_OK) { j->packed = true; j->n_side = n_side; }
            else { pool.put(j->pk); j->pk = ReadBuf(); } // (too many such reads for the side list: this batch travels as bytes)
        }
        return j;
    };
    // PGX_CLI_STATS=1: busy seconds of every stage (summed over its threads) on stderr at the end
    // (with --result compact "download" holds the encode on the device and the download of the stream, and "format" holds the host expansion
    // of the blocks next to the formatting: the two forms split the same work differently between the two figures)
    const bool cli_stats = std::getenv("PGX_CLI_STATS") != nullptr;
    // (with --format device "download" holds only the locate, "format" the whole of pgx_batch_format -- length and fill kernels and the download of the
    // text -- plus any wait for the writer to release a text buffer; a second line splits the two)
    std::atomic<uint64_t> ns_parse{0}, ns_upload{0}, ns_run{0}, ns_download{0}, ns_format{0}, ns_write{0}, ns_devfmt{0}, ns_lent{0};
    std::atomic<uint64_t> us_devfmt_kernels{0}, text_bytes{0};
    auto now_ns = []() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const uint64_t t_pipeline0 = now_ns();
    std::vector<std::thread> parsers;
    for (unsigned t = 0; t < n_parse; t++)
        parsers.emplace_back([&]() {
            for (;;) {
                const uint64_t id = next_range.fetch_add(1);
                if (id >= n_jobs) break;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv_space.wait(lk, [&]() { return failed || id < next_write + max_ahead; });
                    if (failed) break;
                }
                const uint64_t tp0 = now_ns();
                std::unique_ptr<Job> j = parse_range(id);
                ns_parse += now_ns() - tp0;
                std::lock_guard<std::mutex> lk(mu);
                if (dev_parse) { parsed[id] = std::move(j); cv_jobs.notify_all(); continue; } // (counted by the worker that uploads it)
                counts[id] = j->offs.size() - 1;
                parsed[id] = std::move(j);
                // sequence numbers: a range knows its first read's number once every range before it has been parsed
                while (counts.count(next_seq_id)) {
                    parsed[next_seq_id]->first_seq = seq_so_far;
                    seq_so_far += counts[next_seq_id];
                    counts.erase(next_seq_id);
                    next_seq_id++;
                }
                cv_jobs.notify_all();
            }
        });
    if (n_jobs == 0) reader_done = true;

    auto worker = [&](int device) {
        pgx_batch *b = nullptr; // long-lived: its device and pinned host buffers are reused by every batch of this worker
        ExpandBufs xb;          // --result compact: what the formatter threads expand into
        // --format device: the batches of this worker whose text the writer has not written yet.  The text stays where pgx_batch_format put it, in one of
        // the two pinned buffer sets of `b` that its calls alternate between, so at most two are lent at a time.  (No deadlock: the writer takes batches in
        // file order, and the worker that holds the oldest unwritten batch waits for none: everything before it has been written.)
        std::deque<uint64_t> lent;
        auto wait_written = [&](size_t keep) {
            std::unique_lock<std::mutex> lk(mu);
            while (lent.size() > keep) {
                const uint64_t id = lent.front();
                cv_written.wait(lk, [&]() { return writer_done || written > id; });
                lent.pop_front();
            }
        };
        for (;;) {
            std::unique_ptr<Job> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                // the next range in file order, once it is parsed and numbered
                cv_jobs.wait(lk, [&]() { return failed || next_take >= n_jobs || (parsed.count(next_take) && (dev_parse || next_take < next_seq_id)); });
                if (failed || next_take >= n_jobs) break;
                j = std::move(parsed[next_take]);
                parsed.erase(next_take);
                next_take++;
                if (next_take >= n_jobs) { reader_done = true; cv_jobs.notify_all(); cv_done.notify_all(); }
            }
            std::unique_ptr<Done> d(new Done());
            size_t n = j->offs.size() - 1;
            pgx_status st = PGX_OK;
            uint64_t t0 = now_ns();
            if (dev_parse) { // upload + parse on the device; then this range's count numbers the ranges behind it
                static const uint64_t no_offsets[1] = {0};
                if (!b) st = pgx_batch_create(h, device, nullptr, no_offsets, 0, &b);
                uint64_t nr = 0;
                if (st == PGX_OK) st = pgx_batch_upload_text(b, reinterpret_cast<const uint8_t *>(j->cat.p), j->cat.len, rfmt, &nr);
                n = (size_t)nr;
                std::unique_lock<std::mutex> lk(mu);
                if (st == PGX_OK) {
                    counts[j->id] = nr;
                    while (counts.count(next_seq_id)) {
                        first_seq_of[next_seq_id] = seq_so_far;
                        seq_so_far += counts[next_seq_id];
                        counts.erase(next_seq_id);
                        next_seq_id++;
                    }
                    cv_jobs.notify_all();
                } else { // the library's message, with the record and byte counted from the start of the file once the ranges before are counted
                    std::string msg = pgx_last_error();
                    // (this range is never counted: the chain stops at it, next_seq_id == j->id and seq_so_far is its first_seq)
                    cv_jobs.wait(lk, [&]() { return failed || next_seq_id == j->id; });
                    const size_t at = msg.find(" record ");
                    unsigned long long rec = 0, byte = 0;
                    int used = 0;
                    if (next_seq_id == j->id && at != std::string::npos &&
                        std::sscanf(msg.c_str() + at, " record %llu (byte %llu):%n", &rec, &byte, &used) == 2 && used > 0)
                        msg = reads_file + ": " + rfmt_name[rfmt] + " record " + std::to_string(seq_so_far + rec) + " (byte " +
                              std::to_string(ranges[j->id].first + byte) + "):" + msg.substr(at + (size_t)used);
                    d->error = msg;
                    pool.put(j->cat);
                    j->cat = ReadBuf();
                    failed = true;
                    finished[j->id] = std::move(d);
                    cv_done.notify_all();
                    cv_jobs.notify_all();
                    cv_space.notify_all();
                    continue;
                }
            }
            if (n == 0) { // a range of empty lines only
                pool.put(j->cat);
                std::lock_guard<std::mutex> lk(mu);
                finished[j->id] = std::move(d);
                cv_done.notify_all();
                continue;
            }
            pgx_result r;
            const uint8_t *rp = reinterpret_cast<const uint8_t *>(j->cat.p);
            if (j->packed) { // (never with dev_parse: those ranges are uploaded above)
                static const uint64_t no_offsets[1] = {0};
                if (!b) st = pgx_batch_create(h, device, nullptr, no_offsets, 0, &b);
                if (st == PGX_OK)
                    st = pgx_batch_upload_packed(b, reinterpret_cast<const uint32_t *>(j->pk.p), j->offs.data(), n, j->side_ids.data(),
                                                 reinterpret_cast<const uint8_t *>(j->pk.p) + j->side_at, j->n_side);
            } else if (!dev_parse) st = b ? pgx_batch_upload(b, rp, j->offs.data(), n) : pgx_batch_create(h, device, rp, j->offs.data(), n, &b);
            uint64_t t1 = now_ns();
            if (st == PGX_OK) st = pgx_batch_run(b, mem_length, min_occ, (no_text ? 0u : PGX_RUN_TAGS) | PGX_RUN_TIMING, nullptr); // (the tag positions are part of the MEM text only)
            uint64_t t2 = now_ns();
            pgx_compact_result cr;
            std::vector<pgx_read_hit> hit_recs; // --hits: the 40-byte records, taken before the locate that --locate asks for replaces the sets
            if (st == PGX_OK && want_hits) {
                st = pgx_batch_locate(b, PGX_LOCATE_SEQ_SETS, hits_max, nullptr);
                if (st == PGX_OK) st = pgx_batch_read_hits(b, 0, nullptr);
                pgx_read_hits rh;
                if (st == PGX_OK) st = pgx_batch_hits(b, &rh);
                if (st == PGX_OK) hit_recs.assign(rh.hits, rh.hits + rh.n_reads);
            }
            std::vector<pgx_read_place> place_recs; // --place: the 64-byte records; the stage's buffers are its own, the locate below does not touch them
            if (st == PGX_OK && (want_places || run_verify)) {
                st = pgx_batch_locate(b, 0, place_max, nullptr);
                if (st == PGX_OK) st = pgx_batch_read_place(b, place_flags, nullptr);
                pgx_read_places rp2;
                if (st == PGX_OK && want_places) st = pgx_batch_places(b, &rp2);
                if (st == PGX_OK && want_places) place_recs.assign(rp2.reads, rp2.reads + rp2.n_reads);
            }
            std::vector<pgx_read_mates> mate_recs;    // --mates: the 64-byte records of the batch's pairs
            std::vector<pgx_read_rescue> rescue_recs; // --rescued: the 64-byte records of the batch's reads
            std::vector<pgx_read_mapq> mapq_recs;     // --mapq: the 32-byte records of the batch's reads
            std::vector<pgx_read_verify> verify_recs; // --verify: the 64-byte records, at the candidates of the place stage above
            if (st == PGX_OK && run_verify) {
                st = pgx_batch_read_verify(b, verify_max, verify_penalty, verify_flags, nullptr);
                if (st == PGX_OK && rescue) { // the unplaced mates are searched for and join the lists, before the pairs choose
                    st = pgx_batch_read_rescue(b, frag_min, frag_max, (uint32_t)rescue_min, (uint32_t)rescue_anchors, PGX_RESCUE_MERGE, nullptr);
                    pgx_read_rescue_result rr;
                    if (st == PGX_OK && want_rescued) st = pgx_batch_rescued(b, &rr);
                    if (st == PGX_OK && want_rescued) rescue_recs.assign(rr.reads, rr.reads + rr.n_reads);
                }
                if (st == PGX_OK && paired) { // the pairs choose: the elected winners are what --verify, --align and --gaf report below
                    st = pgx_batch_read_mates(b, frag_min, frag_max, (uint32_t)mates_penalty, PGX_MATES_ELECT, nullptr);
                    pgx_read_mates_result rm;
                    if (st == PGX_OK && want_mates) st = pgx_batch_mated(b, &rm);
                    if (st == PGX_OK && want_mates) mate_recs.assign(rm.pairs, rm.pairs + rm.n_pairs);
                }
                if (st == PGX_OK && mapq) { // behind the election: the quality of the winners that --gaf reports
                    st = pgx_batch_read_mapq(b, mapq_scale, mapq_slack, mapq_extra, mapq_flags, nullptr);
                    pgx_read_mapqs rq;
                    if (st == PGX_OK) st = pgx_batch_mapqs(b, &rq);
                    if (st == PGX_OK) mapq_recs.assign(rq.records, rq.records + rq.n_reads);
                }
                pgx_read_verifies rv;
                if (st == PGX_OK && want_verify) st = pgx_batch_verified(b, &rv);
                if (st == PGX_OK && want_verify) verify_recs.assign(rv.reads, rv.reads + rv.n_reads);
            }
            std::vector<pgx_read_align> align_recs; // --align: the 64-byte records and the operations, at the winners of the verify stage above
            std::vector<uint64_t> align_op_off;
            std::vector<uint32_t> align_ops;
            if (st == PGX_OK && run_align) {
                st = pgx_batch_read_align(b, align_band, PGX_ALIGN_CIGAR, nullptr);
                pgx_read_aligns ra;
                const bool down = want_align || want_gaf; // (--pack reads the result where it lies)
                if (st == PGX_OK && down) st = pgx_batch_aligned(b, &ra);
                if (st == PGX_OK && down) {
                    align_recs.assign(ra.reads, ra.reads + ra.n_reads);
                    align_op_off.assign(ra.op_offsets, ra.op_offsets + ra.n_reads + 1);
                    align_ops.assign(ra.ops, ra.ops + ra.n_ops);
                }
            }
            if (st == PGX_OK && want_pack) st = pgx_pack_add(packs.at(device), b, pack_min_mapq, 0u, nullptr); // (behind the election and the qualities: the winners)
            std::vector<pgx_read_walk> walk_recs; // --gaf: the 32-byte records and the steps, along the stretches of the align stage above; the reads' lengths
            std::vector<uint64_t> walk_step_off, walk_steps, walk_read_off;
            if (st == PGX_OK && want_gaf) {
                st = pgx_batch_read_walk(b, PGX_WALK_STEPS, nullptr);
                pgx_read_walks rw;
                if (st == PGX_OK) st = pgx_batch_walked(b, &rw);
                if (st == PGX_OK) {
                    walk_recs.assign(rw.reads, rw.reads + rw.n_reads);
                    walk_step_off.assign(rw.step_offsets, rw.step_offsets + rw.n_reads + 1);
                    walk_steps.assign(rw.steps, rw.steps + rw.n_steps);
                    walk_read_off.resize(rw.n_reads + 1);
                    pgx_reads_info ri;
                    st = pgx_batch_reads(b, &ri, walk_read_off.data(), walk_read_off.size(), nullptr, 0);
                }
            }
            if (format_device || no_text) {
                // nothing to download: the device writes the text below, once the batch knows the number of its first read
            } else if (st == PGX_OK && compact_result) {
                st = pgx_batch_result_compact(b, &cr);
                if (st == PGX_OK) { // the arrays of r are filled block range by block range in the formatter threads below
                    std::memset(&r, 0, sizeof r);
                    r.n_reads = cr.n_reads; r.n_mems = cr.n_mems; r.n_positions = cr.n_positions;
                    r.n_extensions = cr.n_extensions; r.n_tag_overflow = cr.n_tag_overflow;
                    r.mem_offsets = xb.mem_off.ensure(cr.n_reads + 1);
                    r.mems = xb.mems.ensure(cr.n_mems + 1);
                    r.tag_run_counts = xb.run_counts.ensure(cr.n_mems + 1);
                    r.pos_offsets = xb.pos_off.ensure(cr.n_mems + 1);
                    r.positions = xb.positions.ensure(cr.n_positions + 1);
                }
            } else if (st == PGX_OK) st = pgx_batch_result(b, &r);
            pgx_locations loc;
            LocateOut lout = locate_out;
            if (st == PGX_OK && locate_mode) {
                st = pgx_batch_locate(b, locate_flags, locate_max, nullptr);
                if (st == PGX_OK && !format_device) st = pgx_batch_locations(b, &loc);
                if (st == PGX_ERR_UNSUPPORTED) d->error = std::string(pgx_last_error()) + " (find_mems: run with --mode strict)";
                lout.loc = &loc;
            }
            uint64_t t3 = now_ns();
            ns_upload += t1 - t0; ns_run += t2 - t1; ns_download += t3 - t2;
            pool.put(j->cat); // (the upload has completed: pgx_batch_upload synchronises its copies)
            j->cat = ReadBuf();
            pool.put(j->pk);
            j->pk = ReadBuf();
            if (st == PGX_OK && dev_parse) { // its number: every range before it counted
                std::unique_lock<std::mutex> lk(mu);
                cv_jobs.wait(lk, [&]() { return failed || j->id < next_seq_id; });
                if (j->id < next_seq_id) j->first_seq = first_seq_of[j->id], first_seq_of.erase(j->id);
                else { st = PGX_ERR_ARG; d->error = "find_mems: a batch before this one failed"; }
            }
            if (st != PGX_OK) { if (d->error.empty()) d->error = pgx_last_error(); }
            else {
                pgx_timing t;
                if (pgx_batch_timing(b, &t) == PGX_OK) {
                    d->mem_s = 1e-3 * (t.ms_find_mems + t.ms_compact);
                    d->tag_s = 1e-3 * (t.ms_tag_locate + t.ms_tag_gather + t.ms_tag_sort);
                }
                if (want_hits) format_hits(hit_recs.data(), hit_recs.size(), j->first_seq, d->hits);
                if (want_places) format_places(place_recs.data(), place_recs.size(), j->first_seq, d->places);
                if (want_verify) format_verifies(verify_recs.data(), verify_recs.size(), j->first_seq, d->verifies);
                if (want_mates) format_mates(mate_recs.data(), mate_recs.size(), j->first_seq, d->mates);
                if (want_rescued) format_rescued(rescue_recs.data(), rescue_recs.size(), j->first_seq, d->rescued);
                if (want_mapqs) format_mapqs(mapq_recs.data(), mapq_recs.size(), j->first_seq, d->mapqs);
                if (want_gaf && !walk_read_off.empty())
                    format_gaf(align_recs.data(), align_op_off.data(), align_ops.data(), walk_recs.data(), walk_step_off.data(), walk_steps.data(), walk_read_off.data(),
                               mapq ? mapq_recs.data() : nullptr, walk_recs.size(), j->first_seq, d->gaf);
                if (want_align && !align_op_off.empty()) format_aligns(align_recs.data(), align_op_off.data(), align_ops.data(), align_recs.size(), j->first_seq, d->aligns);
                if (format_device && !no_text) {
                    // the text of the batch from the device, handed to the writer where it is
                    const uint64_t t3w = now_ns();
                    wait_written(1);
                    ns_lent += now_ns() - t3w;
                    pgx_format_params fp;
                    std::memset(&fp, 0, sizeof fp);
                    fp.first_seq = j->first_seq;
                    fp.flags = (quiet ? 0u : PGX_FORMAT_STDERR) | (locate_mode == LOCATE_POSITIONS ? PGX_FORMAT_LOCATE_POSITIONS : locate_mode == LOCATE_SEQS ? PGX_FORMAT_LOCATE_SEQS : 0u);
                    pgx_text tx;
                    const uint64_t t3f = now_ns(); // (behind the wait for the batch's number)
                    if (pgx_batch_format(b, &fp, &tx) != PGX_OK) d->error = pgx_last_error();
                    ns_devfmt += now_ns() - t3f;
                    if (d->error.empty()) {
                        d->text = tx.text; d->text_n = (size_t)tx.n_bytes;
                        if (tx.err_text) { d->etext = tx.err_text; d->etext_n = (size_t)tx.n_err_bytes; }
                        lent.push_back(j->id);
                        us_devfmt_kernels += (uint64_t)(1e3 * (double)tx.ms_format);
                        text_bytes += tx.n_bytes + tx.n_err_bytes;
                    }
                }
                const unsigned parts = format_device || no_text ? 0u : n < 4096 ? 1u : n_fmt;
                if (parts) d->outs.resize(parts);
                if (parts) d->errs.resize(parts);
                // --result compact: the parts are cut on multiples of 64 reads and every thread expands the blocks of its part first
                auto cut = [&](unsigned w) -> size_t {
                    if (w >= parts) return n;
                    const size_t at = n * w / parts;
                    return compact_result ? at - at % PGX_COMPACT_BLOCK_READS : at;
                };
                auto expand_part = [&](unsigned w) -> std::string {
                    const uint64_t k0 = cut(w) / PGX_COMPACT_BLOCK_READS, k1 = w + 1 >= parts ? cr.n_blocks : cut(w + 1) / PGX_COMPACT_BLOCK_READS;
                    if (pgx_compact_expand(&cr, k0, k1 - k0, const_cast<uint64_t *>(r.mem_offsets), const_cast<pgx_mem *>(r.mems), const_cast<uint64_t *>(r.tag_run_counts),
                                           const_cast<uint64_t *>(r.pos_offsets), const_cast<uint64_t *>(r.positions)) != PGX_OK)
                        return pgx_last_error(); // (the message is thread-local)
                    return std::string();
                };
                if (parts == 0) { // (--format device: the text is there; --hits-only / --place-only: there is none)
                } else if (parts == 1) {
                    if (compact_result) d->error = expand_part(0);
                    if (d->error.empty()) format_range(r, 0, n, j->first_seq, quiet, lout, d->outs[0], d->errs[0]);
                } else {
                    std::vector<std::thread> pool;
                    std::vector<std::string> xerr(parts);
                    Rendezvous expanded(parts);
                    std::atomic<bool> bad{false};
                    for (unsigned w = 0; w < parts; w++)
                        pool.emplace_back([&, w]() {
                            if (compact_result) {
                                xerr[w] = expand_part(w);
                                if (!xerr[w].empty()) bad = true;
                                expanded.arrive_and_wait();
                                if (bad) return;
                            }
                            format_range(r, cut(w), cut(w + 1), j->first_seq, quiet, lout, d->outs[w], d->errs[w]);
                        });
                    for (auto &th : pool) th.join();
                    for (auto &e : xerr)
                        if (!e.empty() && d->error.empty()) d->error = e;
                }
                ns_format += now_ns() - t3;
            }
            std::lock_guard<std::mutex> lk(mu);
            if (!d->error.empty()) failed = true;
            finished[j->id] = std::move(d);
            cv_done.notify_all();
            if (failed) { cv_jobs.notify_all(); cv_space.notify_all(); }
        }
        wait_written(0); // (the writer may still be reading this batch's buffers)
        pgx_batch_free(b);
    };
    std::vector<std::thread> workers;
    for (int d : devices)
        for (unsigned w = 0; w < streams; w++) workers.emplace_back(worker, d);

    // ---- writer: batches in file order ----
    std::string error;
    for (;;) {
        std::unique_ptr<Done> d;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_done.wait(lk, [&]() { return finished.count(next_write) || (reader_done && next_write == n_jobs) || (failed && !finished.count(next_write)); });
            if (!finished.count(next_write)) break;
            d = std::move(finished[next_write]);
            finished.erase(next_write);
            next_write++;
            cv_space.notify_all();
        }
        if (!d->error.empty()) { error = d->error; break; }
        const uint64_t tw0 = now_ns();
        for (size_t w = 0; w < d->outs.size(); w++) {
            std::fwrite(d->outs[w].data(), 1, d->outs[w].size(), stdout);
            if (!d->errs[w].empty()) std::fwrite(d->errs[w].data(), 1, d->errs[w].size(), stderr);
        }
        if (d->text_n) std::fwrite(d->text, 1, d->text_n, stdout);
        if (d->etext_n) std::fwrite(d->etext, 1, d->etext_n, stderr);
        if (hits_fp && !d->hits.empty()) std::fwrite(d->hits.data(), 1, d->hits.size(), hits_fp);
        if (place_fp && !d->places.empty()) std::fwrite(d->places.data(), 1, d->places.size(), place_fp);
        if (verify_fp && !d->verifies.empty()) std::fwrite(d->verifies.data(), 1, d->verifies.size(), verify_fp);
        if (align_fp && !d->aligns.empty()) std::fwrite(d->aligns.data(), 1, d->aligns.size(), align_fp);
        if (gaf_fp && !d->gaf.empty()) std::fwrite(d->gaf.data(), 1, d->gaf.size(), gaf_fp);
        if (mates_fp && !d->mates.empty()) std::fwrite(d->mates.data(), 1, d->mates.size(), mates_fp);
        if (rescued_fp && !d->rescued.empty()) std::fwrite(d->rescued.data(), 1, d->rescued.size(), rescued_fp);
        if (mapq_fp && !d->mapqs.empty()) std::fwrite(d->mapqs.data(), 1, d->mapqs.size(), mapq_fp);
        ns_write += now_ns() - tw0;
        total_mem_time += d->mem_s;
        total_tag_time += d->tag_s;
        std::lock_guard<std::mutex> lk(mu);
        written = next_write; // (only this thread changes next_write)
        cv_written.notify_all();
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        writer_done = true;
        cv_written.notify_all();
        if (!error.empty()) failed = true;
        cv_jobs.notify_all();
        cv_space.notify_all();
    }
    for (auto &th : parsers) th.join();
    for (auto &th : workers) th.join();
    if (error.empty()) // a batch that failed behind one still in flight when the writer stopped
        for (auto &kv : finished)
            if (!kv.second->error.empty()) { error = kv.second->error; break; }
    if (error.empty() && failed) error = "find_mems: a device batch failed";
    if (hits_fp && (std::fclose(hits_fp) != 0) && error.empty()) error = "Cannot write hits file: " + hits_file;
    if (place_fp && (std::fclose(place_fp) != 0) && error.empty()) error = "Cannot write place file: " + place_file;
    if (verify_fp && (std::fclose(verify_fp) != 0) && error.empty()) error = "Cannot write verify file: " + verify_file;
    if (align_fp && (std::fclose(align_fp) != 0) && error.empty()) error = "Cannot write align file: " + align_file;
    if (gaf_fp && (std::fclose(gaf_fp) != 0) && error.empty()) error = "Cannot write gaf file: " + gaf_file;
    if (mates_fp && (std::fclose(mates_fp) != 0) && error.empty()) error = "Cannot write mates file: " + mates_file;
    if (rescued_fp && (std::fclose(rescued_fp) != 0) && error.empty()) error = "Cannot write rescued file: " + rescued_file;
    if (mapq_fp && (std::fclose(mapq_fp) != 0) && error.empty()) error = "Cannot write mapq file: " + mapq_file;
    if (want_pack && error.empty()) error = write_packs(packs, pack_file, pack_bases_file);
    free_packs();
    if (!error.empty()) {
        std::cerr << error << std::endl;
        return EXIT_FAILURE;
    }
    std::fflush(stdout);
    std::cout.flush();
    if (cli_stats)
        std::fprintf(stderr, "[find_mems] pipeline %.3f s wall; busy seconds: parse %.3f (%u threads), upload %.3f, run %.3f, download %.3f, format %.3f (wall of %u-thread pools), write %.3f; %u device workers\n",
                     1e-9 * (double)(now_ns() - t_pipeline0), 1e-9 * (double)ns_parse.load(), n_parse, 1e-9 * (double)ns_upload.load(), 1e-9 * (double)ns_run.load(),
                     1e-9 * (double)ns_download.load(), 1e-9 * (double)ns_format.load(), n_fmt, 1e-9 * (double)ns_write.load(), n_workers);
    if (cli_stats && format_device)
        std::fprintf(stderr, "[find_mems] --format device: of format %.3f s: pgx_batch_format %.3f (its kernels %.3f), waiting for the writer to release a text buffer %.3f; %.1f MB of text\n",
                     1e-9 * (double)ns_format.load(), 1e-9 * (double)ns_devfmt.load(), 1e-6 * (double)us_devfmt_kernels.load(), 1e-9 * (double)ns_lent.load(),
                     1e-6 * (double)text_bytes.load());
    if (!no_text) {
        std::cout << "\nTotal time for finding all MEMs: " << total_mem_time << " seconds" << std::endl; // :144
        std::cout << "Total time for all tag queries: " << total_tag_time << " seconds" << std::endl;   // :145
    }
    pgx_index_close(h);
    return 0;
}
