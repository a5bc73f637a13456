/*
 * acgpu_jni_cursor.c -- JNI glue of the match cursor (acgpu_cursor_*, include/acgpu.h): NativeAutomaton.cursorOpen /
 * cursorNext / cursorClose.  Built together with acgpu_jni.c (see its build line); the rules of that file hold here too: no
 * critical region across a call into libacgpu, every allocation checked, no int[] longer than Java allows -- a page is at most
 * maxRecords records, so a text with more records than one int[] holds is drained page by page.
 */
#include <jni.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "acgpu.h"
#include "acgpu_jni_common.h"

/* what a Java cursor handle points to: the library's cursor, the copy of the String's units it reads until close, and the
 * buffer the pages land in before they become an int[] */
typedef struct jni_cursor {
    acgpu_cursor *c;
    jchar *units;
    int kind;
    void *page;
    uint64_t page_cap; /* records */
} jni_cursor;

JNIEXPORT jlong JNICALL Java_com_roklenarcic_util_strings_gpu_NativeAutomaton_cursorOpen(JNIEnv *env, jclass cls, jlong handle,
                                                                                           jstring haystack, jboolean withIds) {
    (void)cls;
    if (!haystack) {
        throw_new(env, "java/lang/NullPointerException", "haystack"); /* reference: haystack.length() on null */
        return 0;
    }
    const acgpu_automaton *a = (const acgpu_automaton *)(intptr_t)handle;
    const jsize n = (*env)->GetStringLength(env, haystack);
    jni_cursor *jc = (jni_cursor *)calloc(1, sizeof(jni_cursor));
    if (!jc) { throw_oom(env, "cursor"); return 0; }
    jc->kind = withIds ? ACGPU_REC_MAP : ACGPU_REC_SET;
    jc->units = (jchar *)malloc((size_t)(n ? n : 1) * sizeof(jchar));
    if (!jc->units) { throw_oom(env, "haystack copy"); free(jc); return 0; }
    for (jsize at = 0; at < n; at += REGION_SLICE) {
        const jsize len = n - at < REGION_SLICE ? n - at : REGION_SLICE;
        (*env)->GetStringRegion(env, haystack, at, len, jc->units + at);
        if ((*env)->ExceptionCheck(env)) { free(jc->units); free(jc); return 0; }
    }
    const int rc = acgpu_cursor_open(a, (const uint16_t *)jc->units, (uint64_t)n, jc->kind, &jc->c);
    if (rc != ACGPU_OK) {
        throw_rc(env, rc);
        free(jc->units);
        free(jc);
        return 0;
    }
    return (jlong)(intptr_t)jc;
}

/* the next page, flattened ((start,end) pairs or (start,end,keywordIndex) triples); an empty array: every record handed out */
JNIEXPORT jintArray JNICALL Java_com_roklenarcic_util_strings_gpu_NativeAutomaton_cursorNext(JNIEnv *env, jclass cls, jlong cursor,
                                                                                               jint maxRecords) {
    (void)cls;
    jni_cursor *jc = (jni_cursor *)(intptr_t)cursor;
    if (!jc) { throw_new(env, "java/lang/IllegalStateException", "cursor is closed"); return NULL; }
    if (maxRecords < 1) { throw_new(env, "java/lang/IllegalArgumentException", "maxRecords must be at least 1"); return NULL; }
    const uint64_t cols = (uint64_t)(jc->kind / 4);
    uint64_t cap = (uint64_t)maxRecords;
    if (cap * cols > (uint64_t)INT_MAX - 8) cap = ((uint64_t)INT_MAX - 8) / cols; /* (a page is one int[]) */
    if (jc->page_cap < cap) {
        free(jc->page);
        jc->page_cap = 0;
        jc->page = malloc(cap * (size_t)jc->kind);
        if (!jc->page) { throw_oom(env, "match records"); return NULL; }
        jc->page_cap = cap;
    }
    uint64_t n_out = 0;
    const int rc = acgpu_cursor_next(jc->c, jc->page, cap, &n_out);
    if (rc != ACGPU_OK) { throw_rc(env, rc); return NULL; }
    const jsize n_ints = (jsize)(n_out * cols);
    jintArray out = (*env)->NewIntArray(env, n_ints);
    if (out && n_ints) (*env)->SetIntArrayRegion(env, out, 0, n_ints, (const jint *)jc->page);
    return out; /* NULL: OutOfMemoryError pending */
}

JNIEXPORT void JNICALL Java_com_roklenarcic_util_strings_gpu_NativeAutomaton_cursorClose(JNIEnv *env, jclass cls, jlong cursor) {
    (void)env;
    (void)cls;
    jni_cursor *jc = (jni_cursor *)(intptr_t)cursor;
    if (!jc) return;
    acgpu_cursor_close(jc->c);
    free(jc->page);
    free(jc->units);
    free(jc);
}
