// build_tags -- the reference CLI (src/build_tags.cpp) on MI355X: graph + BWT -> tag array ("algorithm format", the input of
// merge_tags / convert_tags).
//
//   build_tags <graph.gbz> <graph_info.rl_bwt> <output.tags> [--ri] [--device N] [--forward-only] [--reference-runs]
//              [--format algorithm|compact|bytecode]
//
// --format compact / bytecode: the output is the query format find_mems loads, encoded on the device -- the file convert_tags
// would make of the default output, in one step (pgx_build_tags, PGX_BUILD_TAGS_OUT_*).  algorithm is the default.
// The reference's argument list.  The r-index is built in memory from the .rl_bwt (as build_rindex would write it); with --ri
// the second argument is an existing .ri instead.  --forward-only: the text holds one orientation per path (index sequence s =
// GBWT sequence 2s, as gbz_extract without -b writes it); without it, a text of that shape is rejected.  --reference-runs: run
// lengths mod 65 536 as the reference writes them (pgx_build_tags).  Progress on stderr, nothing on stdout.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../include/pgx.h"

static int usage() {
    std::cerr << "usage: build_tags <graph.gbz> <graph_info.rl_bwt> <output.tags> [--ri] [--device N] [--forward-only] [--reference-runs]"
                 " [--format algorithm|compact|bytecode]"
              << std::endl;
    return EXIT_FAILURE;
}

int main(int argc, char **argv) {
    if (argc < 4) return usage();
    int device = 0;
    uint32_t flags = PGX_BUILD_TAGS_INPUT_RLBWT;
    for (int i = 4; i < argc; i++) {
        const std::string o = argv[i];
        if (o == "--ri") flags &= ~PGX_BUILD_TAGS_INPUT_RLBWT;
        else if (o == "--format" && i + 1 < argc) {
            const std::string f = argv[++i];
            flags &= ~(PGX_BUILD_TAGS_OUT_COMPACT | PGX_BUILD_TAGS_OUT_BYTECODE);
            if (f == "compact") flags |= PGX_BUILD_TAGS_OUT_COMPACT;
            else if (f == "bytecode") flags |= PGX_BUILD_TAGS_OUT_BYTECODE;
            else if (f != "algorithm") return usage();
        }
        else if (o == "--device" && i + 1 < argc) {
            char *end = nullptr;
            const long v = std::strtol(argv[++i], &end, 10);
            if (!*argv[i] || *end || v < 0) { std::cerr << "bad device: " << argv[i] << std::endl; return EXIT_FAILURE; }
            device = (int)v;
        } else if (o == "--forward-only") flags |= PGX_BUILD_TAGS_FORWARD_ONLY;
        else if (o == "--reference-runs") flags |= PGX_BUILD_TAGS_REFERENCE_RUNS;
        else { std::cerr << "unknown option " << o << std::endl; return EXIT_FAILURE; }
    }
    std::cerr << "Loading the graph " << argv[1] << " and the " << ((flags & PGX_BUILD_TAGS_INPUT_RLBWT) ? "BWT " : "r-index ") << argv[2]
              << std::endl;
    if (pgx_build_tags(argv[1], argv[2], device, argv[3], flags) != PGX_OK) {
        std::cerr << pgx_last_error() << std::endl;
        return EXIT_FAILURE;
    }
    double ms[6] = {0, 0, 0, 0, 0, 0};
    pgx_build_tags_timing(ms, 6);
    std::fprintf(stderr, "graph %.1f ms, index %.1f ms, suffix array %.1f ms, tags %.1f ms, runs %.1f ms, write %.1f ms\n", ms[0], ms[1], ms[2],
                 ms[3], ms[4], ms[5]);
    if (flags & (PGX_BUILD_TAGS_OUT_COMPACT | PGX_BUILD_TAGS_OUT_BYTECODE)) {
        double e[6] = {0, 0, 0, 0, 0, 0};
        pgx_tags_encode_timing(e, 6);
        std::fprintf(stderr, "write = device encoding: pieces %.1f ms, sd_vectors %.1f ms, select %.1f ms, download %.1f ms, file %.1f ms (%.0f bytes)\n", e[0],
                     e[1], e[2], e[3], e[4], e[5]);
    }
    std::cerr << "Tags written to " << argv[3] << std::endl;
    return 0;
}
