// err_table.cpp -- the reader of --ErrorTable (err_table.h).
#include "err_table.h"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <vector>

namespace vb2 {

namespace {

std::vector<std::string> split_tabs(const std::string& line)
{
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) {
        const size_t tab = line.find('\t', at);
        out.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
        if (tab == std::string::npos) return out;
        at = tab + 1;
    }
}

bool whole_long(const std::string& text, long* v)
{
    if (text.empty()) return false;
    errno = 0;
    char* end = nullptr;
    *v = std::strtol(text.c_str(), &end, 10);
    return errno == 0 && end == text.c_str() + text.size();
}

bool whole_double(const std::string& text, double* v)
{
    if (text.empty()) return false;
    errno = 0;
    char* end = nullptr;
    *v = std::strtod(text.c_str(), &end);
    return end == text.c_str() + text.size();            // (a NaN or an overflow parses: the range check refuses it)
}

}  // namespace

bool read_err_table(const std::string& path, double* table, int* taken, std::string* error)
{
    const auto fail = [&](const std::string& what) {
        *error = "--ErrorTable " + path + ": " + what;
        return false;
    };
    *taken = 0;
    for (int q = 0; q < kErrTableQual; ++q) table[q] = std::pow(10.0, q / -10.0);
    std::ifstream in(path);
    if (!in.is_open()) return fail("cannot be opened");
    std::string line;
    if (!std::getline(in, line)) return fail("line 1: the file is empty, a header with #Q_REPORTED and ERROR_RATE is expected");
    if (!line.empty() && line.back() == '\r') line.pop_back();
    int col_q = -1, col_e = -1;
    {
        const std::vector<std::string> names = split_tabs(line);
        for (size_t i = 0; i < names.size(); ++i) {
            if (names[i] == "#Q_REPORTED" && col_q < 0) col_q = (int)i;
            if (names[i] == "ERROR_RATE" && col_e < 0) col_e = (int)i;
        }
    }
    if (col_q < 0) return fail("line 1: the header has no column #Q_REPORTED");
    if (col_e < 0) return fail("line 1: the header has no column ERROR_RATE");
    const size_t need = (size_t)(col_q > col_e ? col_q : col_e) + 1;
    bool seen[kErrTableQual] = {};
    for (long num = 2; std::getline(in, line); ++num) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::string at = "line " + std::to_string(num) + ": ";
        const std::vector<std::string> f = split_tabs(line);
        if (f.size() < need) return fail(at + std::to_string(f.size()) + " fields, the columns of the header need " + std::to_string(need));
        long q = 0;
        if (!whole_long(f[(size_t)col_q], &q)) return fail(at + "the quality '" + f[(size_t)col_q] + "' is no whole number");
        if (q < 0 || q >= kErrTableQual) return fail(at + "the quality " + std::to_string(q) + " lies outside 0..93");
        if (seen[q]) return fail(at + "the quality " + std::to_string(q) + " is listed twice");
        double e = 0.0;
        if (!whole_double(f[(size_t)col_e], &e)) return fail(at + "the rate '" + f[(size_t)col_e] + "' is no number");
        if (!(e >= 0.0 && e <= 1.0)) return fail(at + "the rate '" + f[(size_t)col_e] + "' is a NaN or lies outside [0, 1]");
        seen[q] = true;
        table[q] = e;
        ++*taken;
    }
    return true;
}

}  // namespace vb2
