// acgpu_terms_finish.h -- the host's finishing pass of acgpu_count_batch_* (include/acgpu.h; the device side: acgpu_terms.hip).
// Host only: the C++ standard library and nothing of HIP, so that a program without a device can include it and test it.
//
// In: the device's entry list, 3 words {h, id, count} per entry.  What the device guarantees about it (acgpu_terms.hip):
//  * h never descends;
//  * the entries of one h are a sequence of SUB-ROWS, each with ids ascending and distinct -- one sub-row per block of records
//    that the haystack's run of records touches.  A haystack whose run no block or piece boundary cuts has one sub-row: a
//    finished row.
// Out: the canonical CSR matrix -- row_ptr[n_haystacks + 1], ids ascending and distinct within a row, a count per id.
//
// The pass checks the h column (the only thing that could make it write out of bounds), then walks the entries ONCE: it copies
// them to the output as they come, filling row_ptr for every haystack it passes, the empty ones included.  A row is CUT where an
// id does not exceed its predecessor's within one h -- only there a second sub-row has begun; such a row alone is sorted by id
// and its equal ids summed, and the output is compacted behind it.  The output never runs ahead of the input, so `ids` and
// `counts` need room for n_entries values (the capacity rule of the call: n_terms <= n_entries <= cap).
// One huge haystack is one row of many sub-rows: the whole list is then sorted here, on one host thread -- the limit of this form.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace acgpu {

// 0, or -1: an h that descends or is not below n_haystacks (nothing has been written then)
inline int terms_finish(const uint32_t *entries, uint64_t n_entries, uint32_t n_haystacks, uint64_t *row_ptr, uint32_t *ids, uint32_t *counts,
                        uint64_t *n_terms, uint32_t *rows_cut) {
    for (uint64_t i = 0; i < n_entries; i++)
        if (entries[3 * i] >= n_haystacks || (i && entries[3 * i] < entries[3 * (i - 1)])) return -1;
    std::vector<uint64_t> row; // a cut row as (id << 32) | count, for the sort
    uint64_t out = 0;
    uint32_t next_row = 0, cut = 0;
    for (uint64_t i = 0; i < n_entries;) {
        const uint32_t h = entries[3 * i];
        while (next_row <= h) row_ptr[next_row++] = out;
        const uint64_t row_begin = out;
        bool is_cut = false;
        for (; i < n_entries && entries[3 * i] == h; i++, out++) {
            ids[out] = entries[3 * i + 1];
            counts[out] = entries[3 * i + 2];
            is_cut |= out > row_begin && ids[out] <= ids[out - 1];
        }
        if (!is_cut) continue;
        cut++;
        row.clear();
        for (uint64_t j = row_begin; j < out; j++) row.push_back((uint64_t)ids[j] << 32 | counts[j]);
        std::sort(row.begin(), row.end());
        out = row_begin;
        for (const uint64_t e : row) {
            if (out > row_begin && ids[out - 1] == (uint32_t)(e >> 32)) {
                counts[out - 1] += (uint32_t)e;
            } else {
                ids[out] = (uint32_t)(e >> 32);
                counts[out++] = (uint32_t)e;
            }
        }
    }
    while (next_row <= n_haystacks) row_ptr[next_row++] = out;
    *n_terms = out;
    *rows_cut = cut;
    return 0;
}

} // namespace acgpu
