// san_by_of.cpp — sanitizer driver of the HOST checks of "statistics by key" (fmx_number_stats_by_batch, fmx_numbers_by_key_dev):
// check_by_of (index4j_amd/csrc/fmx_host_batch.cpp, linked as it is) and fm_by_rows_bad (index4j_amd/csrc/fmx_hit_by.hpp), as a
// stand-alone program for -fsanitize=address,undefined.  Every array lies on the heap with exactly the size the contract gives it
// (an array of no entries is NULL), so a read or a store outside one is a report.  Prints one " ok: " line per case; exit code 0 =
// clean.
#include "fmx_hit_by.hpp"
#include "fmx_host_stage.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace {
int g_code = 0;
std::string g_msg;
}  // namespace

namespace fmx {
int api_fail(int code, const std::string &msg) {  // the stub: what fmx_last_error would say
    g_code = code;
    g_msg = msg;
    return code;
}
}  // namespace fmx

namespace {

void require(bool ok, const char *name) {
    if (!ok) {
        std::fprintf(stderr, "FAILED %s (last message: \"%s\")\n", name, g_msg.c_str());
        std::exit(1);
    }
    std::printf(" ok: %s\n", name);
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    if (v.empty()) return nullptr;
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

int by_of_rc(const std::vector<int32_t> &by_of, int32_t m) {
    g_msg.clear();
    return fmx::check_by_of((int32_t)by_of.size(), exact(by_of).get(), m);
}

int rows_rc(const std::vector<int32_t> &by_of, const std::vector<int64_t> &val_off, int32_t P, std::vector<int64_t> *rows, int32_t *B) {
    const int32_t n = (int32_t)by_of.size(), m = (int32_t)val_off.size() - 1;
    std::unique_ptr<int64_t[]> out(new int64_t[(size_t)n + 1]);
    const int32_t rc = fmx::fm_by_rows_bad(n, exact(by_of).get(), m, exact(val_off).get(), P, out.get(), B);
    rows->assign(out.get(), out.get() + (rc == 0 && n > 0 ? n + 1 : 0));
    return rc;
}

}  // namespace

int main() {
    require(by_of_rc({}, 0) == FMX_OK && by_of_rc({}, 3) == FMX_OK, "no number pattern: nothing to judge, NULL is not read");
    require(by_of_rc({0}, 1) == FMX_OK && by_of_rc({2, 0, 1, 2}, 3) == FMX_OK, "entries inside 0 .. m - 1");
    require(by_of_rc({0}, 0) == FMX_E_ARG && g_msg.find("m == 0") != std::string::npos, "number patterns without a key pattern");
    require(by_of_rc({0, 3}, 3) == FMX_E_ARG && g_msg.find("by_of[1]") != std::string::npos, "an entry at m");
    require(by_of_rc({-1}, 3) == FMX_E_ARG && g_msg.find("by_of[0]") != std::string::npos, "a negative entry");
    std::vector<int64_t> rows;
    int32_t B = 0;
    require(rows_rc({1, 0, 1}, {0, 2, 7}, 2, &rows, &B) == 0 && rows == std::vector<int64_t>({0, 5, 7, 12}) && B == 5, "rows of a call");
    require(rows_rc({0}, {0, 0}, 0, &rows, &B) == 0 && rows == std::vector<int64_t>({0, 0}) && B == 1, "a key pattern without groups");
    require(rows_rc({1}, {0, 2}, 0, &rows, &B) == 2 && rows_rc({0}, {0, 3, 2}, 0, &rows, &B) == 3 && rows_rc({0}, {-2, 3}, 0, &rows, &B) == 3,
            "by_of outside, offsets that decrease or start below 0");
    require(rows_rc({0, 0}, {0, fmx::kHistCellsMax / 2 + 1}, 0, &rows, &B) == 4 && rows_rc({0}, {0, fmx::kHistCellsMax / 2 + 1}, 2, &rows, &B) == 5,
            "more than 2^27 rows, more than 2^27 percentiles");
    std::printf("by_of: all cases ok\n");
    return 0;
}
