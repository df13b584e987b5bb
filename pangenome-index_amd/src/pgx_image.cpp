// pgx_image -- build the host images of an index once and keep them: the image file find_mems and query_tags open in the place of the
// r-index (include/pgx.h "image file").  Needs no GPU.
//
//   pgx_image <r_index.ri> <tags|-> <out.pgi> [--mode compat|strict] [--tags-format auto|bytecode|compact] [--image pairs|dense2|dense|rl] [--no-locate]
//   pgx_image --info <file>
//
// The reference has no such step: its CLIs load the .ri and the tag file on every start (src/find_mems.cpp:27-88).  "-" in the place of the
// tags makes the image of the r-index alone.  --info prints the header and one line per section: name, bytes, offset, sum.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../include/pgx.h"

static int usage() {
    std::cerr << "usage: pgx_image <r_index.ri> <tags|-> <out.pgi> [--mode compat|strict] [--tags-format auto|bytecode|compact]"
                 " [--image pairs|dense2|dense|rl] [--no-locate]\n       pgx_image --info <file>" << std::endl;
    return 1;
}

static int info(const char *path) {
    pgx_image_info fi;
    if (pgx_image_file_info(path, &fi) != PGX_OK) { std::cerr << pgx_last_error() << std::endl; return 1; }
    std::printf("file %s: %" PRIu64 " bytes\n", path, fi.file_bytes);
    std::printf("version %u layout %u consts_bytes %u loc_consts_bytes %u meta_bytes %u\n", fi.version, fi.layout, fi.consts_bytes, fi.loc_consts_bytes, fi.meta_bytes);
    std::printf("mode %s has_rank %u has_tags %u locate %u literal %u sections %u header_sum %016" PRIx64 "\n", fi.mode == PGX_MODE_STRICT ? "strict" : "compat", fi.has_rank,
                fi.has_tags, (fi.flags & PGX_IMAGE_HAS_LOCATE) ? 1u : 0u, (fi.flags & PGX_IMAGE_HAS_LITERAL) ? 1u : 0u, fi.n_sections, fi.header_sum);
    for (uint32_t i = 0; i < fi.n_sections; i++)
        std::printf("section %-12s bytes %" PRIu64 " offset %" PRIu64 " sum %016" PRIx64 "\n", fi.sections[i].name, fi.sections[i].bytes, fi.sections[i].offset, fi.sections[i].sum);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "--info") return argc == 3 ? info(argv[2]) : usage();
    if (argc < 4) return usage();
    const std::string ri = argv[1], tags = argv[2], out = argv[3];
    uint32_t mode = PGX_MODE_COMPAT, tfmt = PGX_TAGS_AUTO, flags = 0;
    for (int i = 4; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::cerr << "missing value for " << a << std::endl; std::exit(1); } return argv[++i]; };
        if (a == "--mode") {
            const std::string v = next();
            if (v == "strict") mode = (mode & ~PGX_MODE_MASK) | PGX_MODE_STRICT;
            else if (v == "compat") mode = (mode & ~PGX_MODE_MASK) | PGX_MODE_COMPAT;
            else { std::cerr << "--mode: compat or strict" << std::endl; return 1; }
        } else if (a == "--tags-format") {
            const std::string v = next();
            if (v == "auto") tfmt = PGX_TAGS_AUTO;
            else if (v == "bytecode") tfmt = PGX_TAGS_BYTECODE;
            else if (v == "compact") tfmt = PGX_TAGS_COMPACT;
            else { std::cerr << "--tags-format: auto, bytecode or compact" << std::endl; return 1; }
        } else if (a == "--image") {
            const std::string v = next();
            const uint32_t all = PGX_MODE_IMAGE_RL | PGX_MODE_IMAGE_DENSE | PGX_MODE_IMAGE_DENSE2 | PGX_MODE_IMAGE_PAIRS;
            const uint32_t bit = v == "pairs" ? PGX_MODE_IMAGE_PAIRS : v == "dense2" ? PGX_MODE_IMAGE_DENSE2 : v == "dense" ? PGX_MODE_IMAGE_DENSE : v == "rl" ? PGX_MODE_IMAGE_RL : 0u;
            if (!bit) { std::cerr << "--image: pairs, dense2, dense or rl" << std::endl; return 1; }
            mode = (mode & ~all) | bit;
        } else if (a == "--no-locate") flags |= PGX_IMAGE_NO_LOCATE;
        else { std::cerr << "unknown option " << a << std::endl; return usage(); }
    }
    pgx_index *h = nullptr;
    if (pgx_index_open(ri.c_str(), tags == "-" ? nullptr : tags.c_str(), tfmt, mode, &h) != PGX_OK) { std::cerr << pgx_last_error() << std::endl; return 1; }
    const pgx_status st = pgx_index_save_image(h, out.c_str(), flags);
    if (st != PGX_OK) std::cerr << pgx_last_error() << std::endl;
    pgx_index_close(h);
    return st == PGX_OK ? 0 : 1;
}
