/* TEST-ONLY fake JNIEnv for gw_jni.c's nativeDrainSerialized (tests/test_jni_row_encode.py): direct buffers and
 * strings are plain pointers, an int[] is a (length, data) block, a thrown exception is recorded. */
#include <jni.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { jsize len; jint data[8]; } fake_ints;
static char g_exc_class[256], g_exc_msg[1024];
static int g_exc;

static jclass f_find_class(JNIEnv* e, const char* n) {
    (void)e;
    snprintf(g_exc_class, sizeof g_exc_class, "%s", n);
    return (jclass)g_exc_class;
}
static jint f_throw_new(JNIEnv* e, jclass c, const char* m) {
    (void)e; (void)c;
    snprintf(g_exc_msg, sizeof g_exc_msg, "%s", m ? m : "");
    g_exc = 1;
    return 0;
}
static void* f_direct(JNIEnv* e, jobject b) { (void)e; return (void*)b; }
static const char* f_utf(JNIEnv* e, jstring s, jboolean* c) { (void)e; if (c) *c = 0; return (const char*)s; }
static void f_rel_utf(JNIEnv* e, jstring s, const char* c) { (void)e; (void)s; (void)c; }
static jsize f_len(JNIEnv* e, jarray a) { (void)e; return ((fake_ints*)a)->len; }
static void f_int_region(JNIEnv* e, jintArray a, jsize s, jsize n, jint* buf) {
    (void)e;
    memcpy(buf, ((fake_ints*)a)->data + s, (size_t)n * sizeof(jint));
}
/* (the functions nativeDrainSerialized does not call stay null) */
static const struct JNINativeInterface_ g_table = {.FindClass = f_find_class,
                                                   .ThrowNew = f_throw_new,
                                                   .GetDirectBufferAddress = f_direct,
                                                   .GetStringUTFChars = f_utf,
                                                   .ReleaseStringUTFChars = f_rel_utf,
                                                   .GetArrayLength = f_len,
                                                   .GetIntArrayRegion = f_int_region};
static JNIEnv g_env = &g_table;

JNIEnv* fake_env(void) { return &g_env; }
/* the last exception since the previous call (1) or none (0) */
int fake_exception(char* cls, char* msg, int cap) {
    if (!g_exc) return 0;
    snprintf(cls, (size_t)cap, "%s", g_exc_class);
    snprintf(msg, (size_t)cap, "%s", g_exc_msg);
    g_exc = 0;
    return 1;
}
