/*
 * cursor_driver.c -- scenarios for the cursor glue on the CPU (TEST INFRASTRUCTURE): tests/jni_min/cursor_env.c (mock JNIEnv +
 * the glue) over the stubs of the C ABI (stub_acgpu.c, stub_cursor.c), built with -fsanitize=address,undefined and run with
 * leak detection on by tests/test_cursor_cpu.py.  Exit code 0: every scenario held, nothing leaked, no JNI call was made with
 * an exception pending.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

const char *jh_exception_class(void);
long long jh_violations(void);
long long jh_outstanding_elements(void);
void jh_release(int32_t *p);
long long jh_build(int mode, const uint16_t *units, const uint64_t *off, const uint8_t *is_null, int n_kw, int cs, const uint16_t *lower,
                   const uint8_t *wordchars, int table_len);
void jh_free(long long handle);
long long jh_cursor_open(long long handle, const uint16_t *hay, long long n, int with_ids);
long long jh_cursor_next(long long cursor, int max_records, int32_t **out);
void jh_cursor_close(long long cursor);

static int g_failed;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                      \
        }                                                                    \
    } while (0)
static int exc_is(const char *cls) { return !strcmp(jh_exception_class(), cls); }

/* every page of a cursor over hay, concatenated; checks that no page is longer than max_records */
static long long drain(long long c, int max_records, int cols, int32_t *all, long long cap_ints) {
    long long total = 0;
    for (;;) {
        int32_t *p = NULL;
        const long long k = jh_cursor_next(c, max_records, &p);
        CHECK(k >= 0 && exc_is(""));
        if (k < 0) return -1;
        CHECK(k % cols == 0 && k <= (long long)max_records * cols);
        if (k && total + k <= cap_ints) memcpy(all + total, p, (size_t)k * sizeof(int32_t));
        jh_release(p);
        if (k == 0) return total;
        total += k;
    }
}

int main(void) {
    uint16_t kw[2] = {'x', 'y'};
    const uint64_t off[3] = {0, 1, 2};
    long long h = jh_build(0, kw, off, NULL, 2, 1, NULL, NULL, 65536);
    CHECK(h != 0 && exc_is(""));
    /* a haystack with a match at every position p where p % 7 == 3 */
    const long long n = 10007;
    uint16_t *hay = (uint16_t *)malloc((size_t)n * 2);
    long long n_x = 0;
    for (long long i = 0; i < n; i++) {
        hay[i] = (uint16_t)(i % 7 == 3 ? 'x' : 'a');
        n_x += i % 7 == 3;
    }
    int32_t *all = (int32_t *)malloc((size_t)n * 3 * sizeof(int32_t));
    /* ---- pages concatenated == every record, for both record kinds and several page sizes ---- */
    for (int with_ids = 0; with_ids < 2; with_ids++) {
        const int cols = with_ids ? 3 : 2;
        const int sizes[4] = {1, 3, 1000, 1 << 20};
        for (int s = 0; s < 4; s++) {
            long long c = jh_cursor_open(h, hay, n, with_ids);
            CHECK(c != 0 && exc_is(""));
            const long long k = drain(c, sizes[s], cols, all, n * 3);
            CHECK(k == n_x * cols);
            int ok = 1;
            for (long long r = 0; r < n_x && k == n_x * cols; r++) {
                const int32_t p = (int32_t)(7 * r + 3);
                ok &= all[r * cols] == p && all[r * cols + 1] == p + 1 && (cols == 2 || all[r * cols + 2] == p % 1000);
            }
            CHECK(ok);
            /* a page after the end: still empty */
            int32_t *p = NULL;
            CHECK(jh_cursor_next(c, 5, &p) == 0 && exc_is(""));
            jh_release(p);
            jh_cursor_close(c);
        }
    }
    /* ---- close after the first page (the listener returned false): nothing leaks ---- */
    {
        long long c = jh_cursor_open(h, hay, n, 1);
        int32_t *p = NULL;
        CHECK(jh_cursor_next(c, 4, &p) == 12 && p[0] == 3 && p[3] == 10);
        jh_release(p);
        jh_cursor_close(c);
    }
    /* ---- empty haystack: the first page is empty ---- */
    {
        long long c = jh_cursor_open(h, hay, 0, 0);
        int32_t *p = NULL;
        CHECK(c != 0 && jh_cursor_next(c, 4, &p) == 0 && exc_is(""));
        jh_release(p);
        jh_cursor_close(c);
    }
    /* ---- null haystack: NullPointerException, no cursor ---- */
    CHECK(jh_cursor_open(h, NULL, -1, 1) == 0 && exc_is("java/lang/NullPointerException"));
    /* ---- maxRecords < 1: IllegalArgumentException; the cursor stays usable ---- */
    {
        long long c = jh_cursor_open(h, hay, n, 0);
        int32_t *p = NULL;
        CHECK(jh_cursor_next(c, 0, &p) == -1 && exc_is("java/lang/IllegalArgumentException"));
        CHECK(jh_cursor_next(c, 2, &p) == 4 && exc_is("") && p[0] == 3);
        jh_release(p);
        jh_cursor_close(c);
    }
    /* ---- an error of the library: OutOfMemoryError for ACGPU_E_NOMEM ---- */
    {
        uint16_t e3[6] = {'E', '3', 'x', 'x', 'x', 'x'};
        long long c = jh_cursor_open(h, e3, 6, 0);
        int32_t *p = NULL;
        CHECK(jh_cursor_next(c, 1, &p) == 2 && exc_is(""));
        jh_release(p);
        CHECK(jh_cursor_next(c, 1, &p) == -1 && exc_is("java/lang/OutOfMemoryError"));
        jh_cursor_close(c);
    }
    /* ---- a closed (zero) cursor handle: IllegalStateException; close of zero is a no-op ---- */
    {
        int32_t *p = NULL;
        CHECK(jh_cursor_next(0, 1, &p) == -1 && exc_is("java/lang/IllegalStateException"));
        jh_cursor_close(0);
    }
    jh_free(h);
    free(all);
    free(hay);
    CHECK(jh_violations() == 0 && jh_outstanding_elements() == 0);
    if (g_failed) {
        fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    printf("all scenarios ok\n");
    return 0;
}
