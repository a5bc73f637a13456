/*
 * cursor_env.c -- the C harness of tests/jni_min/mock_env.c extended to the cursor glue (TEST INFRASTRUCTURE):
 * ahocorasick_amd/java/jni/acgpu_jni_cursor.c is #included here, like acgpu_jni.c is in mock_env.c, and driven through the
 * same mock JNIEnv.  Linked against tests/jni_min/stub_acgpu.c + stub_cursor.c (tests/jni_min/cursor_driver.c, CPU) or against
 * libacgpu.so (GPU: the pages must equal the ctypes binding's).
 */
#include "mock_env.c"

#include "../../ahocorasick_amd/java/jni/acgpu_jni_cursor.c"

/* n < 0: a null haystack.  0: no cursor (the exception through jh_exception_class) */
JH long long jh_cursor_open(long long handle, const uint16_t *hay, long long n, int with_ids) {
    begin_call();
    jobject s = n < 0 ? NULL : new_string(hay, (jsize)n);
    const jlong c = Java_com_roklenarcic_util_strings_gpu_NativeAutomaton_cursorOpen(&g_env, NULL, (jlong)handle, s, (jboolean)(with_ids ? 1 : 0));
    end_call();
    return (long long)c;
}
/* the page's ints (0: done), -1: an exception */
JH long long jh_cursor_next(long long cursor, int max_records, int32_t **out) {
    begin_call();
    jintArray r = Java_com_roklenarcic_util_strings_gpu_NativeAutomaton_cursorNext(&g_env, NULL, (jlong)cursor, (jint)max_records);
    const long long k = take_int_array(r, out);
    end_call();
    return k;
}
JH void jh_cursor_close(long long cursor) {
    begin_call();
    Java_com_roklenarcic_util_strings_gpu_NativeAutomaton_cursorClose(&g_env, NULL, (jlong)cursor);
    end_call();
}
