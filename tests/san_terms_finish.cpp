// The host's finishing pass of acgpu_count_batch_* (csrc/acgpu_terms_finish.h) as a stand-alone program: the hand-made entry
// lists of tests/test_count_batch_cpu.py with output arrays of EXACTLY the promised sizes (n_haystacks + 1 row pointers, n_entries
// ids and counts), on the heap, so that AddressSanitizer sees any write past them.  Built with -fsanitize=address,undefined by
// tests/test_count_batch_cpu.py and run as a child process.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "acgpu_terms_finish.h"

namespace {

struct Entry {
    uint32_t h, id, count;
};

int failures = 0;

void expect(bool ok, const char *what, const char *name) {
    if (!ok) {
        std::printf("san_terms_finish: FAILED %s: %s\n", name, what);
        failures++;
    }
}

void run(const char *name, const std::vector<Entry> &in, uint32_t n_haystacks, int want_rc, const std::vector<uint64_t> &want_ptr,
         const std::vector<Entry> &want, uint32_t want_cut) {
    std::vector<uint32_t> entries;
    for (const Entry &e : in) {
        entries.push_back(e.h);
        entries.push_back(e.id);
        entries.push_back(e.count);
    }
    std::vector<uint64_t> row_ptr((size_t)n_haystacks + 1, 0xAAAAAAAAAAAAAAAAull);
    std::vector<uint32_t> ids(in.size(), 0xBBBBBBBBu), counts(in.size(), 0xCCCCCCCCu);
    uint64_t n_terms = 77;
    uint32_t cut = 77;
    const int rc = acgpu::terms_finish(entries.data(), in.size(), n_haystacks, row_ptr.data(), ids.data(), counts.data(), &n_terms, &cut);
    expect(rc == want_rc, "return code", name);
    if (rc) {
        bool clean = n_terms == 77 && cut == 77;
        for (uint64_t p : row_ptr) clean &= p == 0xAAAAAAAAAAAAAAAAull;
        for (size_t i = 0; i < in.size(); i++) clean &= ids[i] == 0xBBBBBBBBu && counts[i] == 0xCCCCCCCCu;
        expect(clean, "a refused list writes nothing", name);
        return;
    }
    expect(row_ptr == want_ptr, "row_ptr", name);
    expect(n_terms == want.size() && cut == want_cut, "n_terms / rows_cut", name);
    for (size_t i = 0; i < want.size() && i < n_terms; i++)
        expect(ids[i] == want[i].id && counts[i] == want[i].count, "ids / counts", name);
}

} // namespace

int main() {
    run("no cut", {{0, 1, 2}, {0, 5, 1}, {1, 0, 3}, {2, 4, 1}, {2, 9, 7}}, 3, 0, {0, 2, 3, 5}, {{0, 1, 2}, {0, 5, 1}, {1, 0, 3}, {2, 4, 1}, {2, 9, 7}}, 0);
    run("cut once, a shared id", {{0, 3, 1}, {1, 2, 4}, {1, 7, 1}, {1, 2, 5}, {1, 8, 2}, {2, 0, 1}}, 3, 0, {0, 1, 4, 5},
        {{0, 3, 1}, {1, 2, 9}, {1, 7, 1}, {1, 8, 2}, {2, 0, 1}}, 1);
    run("five sub-rows", {{1, 5, 1}, {1, 9, 1}, {1, 5, 2}, {1, 5, 3}, {1, 6, 1}, {1, 0, 4}, {1, 9, 1}, {1, 5, 10}}, 2, 0, {0, 0, 4},
        {{1, 0, 4}, {1, 5, 16}, {1, 6, 1}, {1, 9, 2}}, 1);
    run("empty haystacks", {{2, 1, 1}, {5, 0, 2}, {5, 3, 1}}, 9, 0, {0, 0, 0, 1, 1, 1, 3, 3, 3, 3}, {{2, 1, 1}, {5, 0, 2}, {5, 3, 1}}, 0);
    run("zero entries", {}, 4, 0, {0, 0, 0, 0, 0}, {}, 0);
    run("zero entries, zero haystacks", {}, 0, 0, {0}, {}, 0);
    run("a cut row at the end", {{0, 4, 1}, {0, 4, 1}}, 1, 0, {0, 1}, {{0, 4, 2}}, 1);
    run("descending h", {{0, 1, 1}, {2, 1, 1}, {1, 1, 1}}, 3, -1, {}, {}, 0);
    run("h out of range", {{0, 1, 1}, {3, 1, 1}}, 3, -1, {}, {}, 0);
    if (failures) return 1;
    std::printf("san_terms_finish: done\n");
    return 0;
}
