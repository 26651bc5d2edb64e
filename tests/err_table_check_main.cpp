// err_table_check_main.cpp -- TEST INFRASTRUCTURE ONLY: the reader of --ErrorTable (verifybamid_amd/csrc/err_table.cpp) in a
// program of its own, so that tests/test_errfit_cohort_cpu.py can run it under the host sanitizers:
//
//     g++ -std=c++17 -fsanitize=address,undefined -I verifybamid_amd/csrc tests/err_table_check_main.cpp \
//         verifybamid_amd/csrc/err_table.cpp -o err_table_check
//     err_table_check (ok|fail) FILE [(ok|fail) FILE ...]
//
// Per file one line: "ok <taken> <q>:<rate> ..." with the qualities whose rate is not the nominal one, or "error <message>".
// Exit status 0 when every file met its expectation (a failure must come with a message that names the file).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "err_table.h"

int main(int argc, char** argv)
{
    if (argc < 3 || (argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: %s (ok|fail) FILE ...\n", argv[0]);
        return 2;
    }
    int bad = 0;
    for (int a = 1; a + 1 < argc; a += 2) {
        const bool want_ok = std::strcmp(argv[a], "ok") == 0;
        double table[vb2::kErrTableQual];
        int taken = -1;
        std::string error;
        const bool ok = vb2::read_err_table(argv[a + 1], table, &taken, &error);
        if (ok) {
            std::printf("ok %d", taken);
            for (int q = 0; q < vb2::kErrTableQual; ++q)
                if (table[q] != std::pow(10.0, q / -10.0)) std::printf(" %d:%.17g", q, table[q]);
            std::printf("\n");
        } else {
            std::printf("error %s\n", error.c_str());
        }
        if (ok != want_ok || (!ok && error.find(argv[a + 1]) == std::string::npos)) ++bad;
    }
    return bad ? 1 : 0;
}
