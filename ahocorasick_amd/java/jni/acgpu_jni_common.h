/*
 * acgpu_jni_common.h -- helpers shared by the JNI translation units (acgpu_jni.c, acgpu_jni_cursor.c): exceptions from
 * ACGPU_E_* codes and the slice size of the String copies.
 */
#ifndef ACGPU_JNI_COMMON_H
#define ACGPU_JNI_COMMON_H

#include <jni.h>

#include "acgpu.h"

#define REGION_SLICE (32 * 1024 * 1024) /* chars per GetStringRegion call (64 MiB) */

static void throw_new(JNIEnv *env, const char *cls, const char *msg) {
    if ((*env)->ExceptionCheck(env)) return; /* keep the first one */
    jclass c = (*env)->FindClass(env, cls);
    if (c) (*env)->ThrowNew(env, c, msg);
}

static void throw_oom(JNIEnv *env, const char *what) { throw_new(env, "java/lang/OutOfMemoryError", what); }

static void throw_rc(JNIEnv *env, int rc) {
    if (rc == ACGPU_E_NOMEM) throw_oom(env, acgpu_strerror(rc));
    else if (rc == ACGPU_E_UNSUPPORTED) throw_new(env, "java/lang/UnsupportedOperationException", acgpu_strerror(rc));
    else throw_new(env, "java/lang/IllegalStateException", acgpu_strerror(rc));
}

#endif /* ACGPU_JNI_COMMON_H */
