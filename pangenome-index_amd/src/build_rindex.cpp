// build_rindex -- the reference CLI (src/build_rindex.cpp): run-length BWT (grlBWT .rl_bwt) -> encoded .ri on stdout.
//
//   build_rindex <file.rl_bwt> [--legacy] > out.ri
//   build_rindex --text <collection.txt> [<more.txt> ...] [--rlbwt <out.rl_bwt>] [--device N] [--legacy] > out.ri
//
// The file is byte-identical to what the reference writes for the same input (tests/test_formats.py reproduces both of the
// reference's own .ri fixtures).  --legacy writes FastLocate::serialize's layout instead of serialize_encoded's.
// The first form is host only: no GPU is needed.  The --text form starts from the collection itself (gbz_extract output; several
// texts are their concatenation) and computes the BWT on the device (pgx_build_index_from_texts_device; default device 0);
// --rlbwt also keeps the .rl_bwt, which build_tags takes.  Status 1 and the library's message on failure.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/pgx.h"

static int emit(const std::string &tmp) {
    std::ifstream in(tmp, std::ios::binary);
    std::cout << in.rdbuf();
    std::cout.flush();
    in.close();
    std::remove(tmp.c_str());
    return 0;
}

static int from_text(int argc, char **argv) {
    std::vector<const char *> texts;
    const char *rlbwt = nullptr;
    int device = 0;
    bool legacy = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--legacy") legacy = true;
        else if ((a == "--rlbwt" || a == "--device") && i + 1 < argc) {
            if (a == "--rlbwt") rlbwt = argv[++i];
            else device = std::atoi(argv[++i]);
        } else if (a.rfind("--", 0) == 0) {
            std::cerr << "build_rindex: unknown or incomplete option " << a << std::endl;
            return EXIT_FAILURE;
        } else texts.push_back(argv[i]);
    }
    if (texts.empty()) {
        std::cerr << "usage: build_rindex --text <collection.txt> [<more.txt> ...] [--rlbwt <out.rl_bwt>] [--device N] [--legacy] > out.ri" << std::endl;
        return EXIT_FAILURE;
    }
    const std::string tmp = std::string(texts[0]) + ".ri.tmp." + std::to_string((long)getpid());
    if (pgx_build_index_from_texts_device(texts.data(), (uint32_t)texts.size(), rlbwt, tmp.c_str(), legacy ? 0 : 1, device) != PGX_OK) {
        std::cerr << pgx_last_error() << std::endl;
        return EXIT_FAILURE;
    }
    return emit(tmp);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "usage: build_rindex <file.rl_bwt> [--legacy] > out.ri\n"
                     "       build_rindex --text <collection.txt> [<more.txt> ...] [--rlbwt <out.rl_bwt>] [--device N] [--legacy] > out.ri" << std::endl;
        return EXIT_FAILURE;
    }
    if (std::string(argv[1]) == "--text") return from_text(argc, argv);
    const bool legacy = argc > 2 && std::string(argv[2]) == "--legacy";
    const std::string tmp = std::string(argv[1]) + ".ri.tmp";
    if (pgx_build_rindex(argv[1], tmp.c_str(), legacy ? 0 : 1) != PGX_OK) {
        std::cerr << pgx_last_error() << std::endl;
        return EXIT_FAILURE;
    }
    return emit(tmp);
}
