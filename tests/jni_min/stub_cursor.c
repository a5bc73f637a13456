/*
 * stub_cursor.c -- a CPU stand-in for the cursor entry points of include/acgpu.h (TEST INFRASTRUCTURE), with the semantics of
 * stub_acgpu.c: NOT a matcher -- a "match" is every unit equal to 'x' (U+0078), id = position modulo 1000.  Enough to drive the
 * cursor glue (tests/jni_min/cursor_env.c) under the sanitizers: pages, the empty page at the end, errors, close at any point.
 * A haystack that begins with "E3" makes the second page return ACGPU_E_NOMEM.
 */
#include <stdlib.h>
#include <string.h>

#include "acgpu.h"

struct acgpu_cursor {
    const uint16_t *hay;
    uint64_t n, pos, delivered;
    int kind, fail_second, pages;
};

int acgpu_cursor_open(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, int record_kind, acgpu_cursor **out) {
    if (!out) return ACGPU_E_INVALID;
    *out = NULL;
    if (!a || !haystack || n_units >= (1ull << 31)) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    acgpu_cursor *c = (acgpu_cursor *)calloc(1, sizeof(acgpu_cursor));
    if (!c) return ACGPU_E_NOMEM;
    c->hay = haystack;
    c->n = n_units;
    c->kind = record_kind;
    c->fail_second = n_units >= 2 && haystack[0] == 'E' && haystack[1] == '3';
    *out = c;
    return ACGPU_OK;
}

int acgpu_cursor_next(acgpu_cursor *c, void *out, uint64_t cap, uint64_t *n_out) {
    if (!c || !out || !n_out || cap == 0) return ACGPU_E_INVALID;
    *n_out = 0;
    if (c->fail_second && c->pages == 1) return ACGPU_E_NOMEM;
    int32_t *r = (int32_t *)out;
    const int cols = c->kind / 4;
    uint64_t k = 0;
    for (; c->pos < c->n && k < cap; c->pos++) { /* (every unit is read: the sanitizers see a short buffer) */
        if (c->hay[c->pos] != 'x') continue;
        r[k * cols] = (int32_t)c->pos;
        r[k * cols + 1] = (int32_t)c->pos + 1;
        if (cols == 3) r[k * cols + 2] = (int32_t)(c->pos % 1000);
        k++;
    }
    c->pages++;
    c->delivered += k;
    *n_out = k;
    return ACGPU_OK;
}

int acgpu_cursor_get_stats(const acgpu_cursor *c, acgpu_cursor_stats *st) {
    if (!c || !st) return ACGPU_E_INVALID;
    memset(st, 0, sizeof(*st));
    st->records_delivered = c->delivered;
    st->scan_end = c->pos;
    st->done = c->pos >= c->n;
    return ACGPU_OK;
}

void acgpu_cursor_close(acgpu_cursor *c) { free(c); }
