// gbz_extract -- the text of a GBZ graph's paths, one line per GBWT sequence, spelled from the GBWTGraph's node sequences
// (what gbz_extract -b of the vg toolchain gives for the input of grlBWT / build_rindex).
//
//   gbz_extract <graph.gbz> [-b] > text        (-b may also come first)
//
// -b: every GBWT sequence (both orientations of every path); default: the even ones (the forward orientation).
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../include/pgx.h"

int main(int argc, char **argv) {
    uint32_t flags = PGX_BUILD_TAGS_FORWARD_ONLY;
    const char *graph = nullptr;
    for (int i = 1; i < argc; i++) {
        const std::string o = argv[i];
        if (o == "-b") flags = 0;
        else if (o.size() > 1 && o[0] == '-') { std::cerr << "unknown option " << o << " (only -b: both orientations)" << std::endl; return EXIT_FAILURE; }
        else if (!graph) graph = argv[i];
        else { std::cerr << "more than one graph: " << o << std::endl; return EXIT_FAILURE; }
    }
    if (!graph) {
        std::cerr << "usage: gbz_extract <graph.gbz> [-b] > text" << std::endl;
        return EXIT_FAILURE;
    }
    std::cout.flush();
    if (pgx_gbz_extract(graph, "/dev/stdout", flags) != PGX_OK) {
        std::cerr << pgx_last_error() << std::endl;
        return EXIT_FAILURE;
    }
    return 0;
}
