"""The input-channel entry points of the JNI glue (integration/jni/native/gw_jni.c:
nativeSetInputChannels, nativeInputStatus, nativeIngestChannels) compiled against the test-only
JNI header of tests/jni/rowenc/ (the one that declares int[] access) and its fake JNIEnv, then
called from Python without a device: the argument checks that come before the handle is used,
and the status -> Java exception mapping.  Every native method GpuWindowOperator.java declares
for them has its JNI function (tests/test_jni_glue.py checks all natives)."""
import ctypes

import pytest

from tests.test_jni_row_encode import CLS, FakeInts, exception, jni  # noqa: F401  (jni: the compiled glue)


@pytest.fixture()
def fns(jni):  # noqa: F811
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    set_ch = getattr(jni, CLS + "nativeSetInputChannels")
    set_ch.restype, set_ch.argtypes = None, [p, p, i64, i32]
    status = getattr(jni, CLS + "nativeInputStatus")
    status.restype, status.argtypes = None, [p, p, i64, p]
    ingest = getattr(jni, CLS + "nativeIngestChannels")
    ingest.restype = i64
    ingest.argtypes = [p, p, i64, p, p, p, p, p, ctypes.c_char_p, i32, i32]
    return set_ch, status, ingest


def test_null_handle_maps_to_illegal_argument(jni, fns):  # noqa: F811
    set_ch, status, _ = fns
    set_ch(jni.fake_env(), None, 0, 4)
    assert exception(jni)[0] == "java/lang/IllegalArgumentException"
    status(jni.fake_env(), None, 0, None)
    assert exception(jni)[0] == "java/lang/IllegalArgumentException"


def test_ingest_channels_rejects_arrays_of_different_lengths(jni, fns):  # noqa: F811
    """channels, offsets, lengths and consumed describe the same ranges: one length, at most
    GW_MAX_INPUT_CHANNELS; refused before any array or the handle is read."""
    _, _, ingest = fns
    arr = lambda n: ctypes.byref(FakeInts(n, (ctypes.c_int32 * 8)()))  # noqa: E731  (the fake env reads only len)
    for lens in ((2, 2, 2, 3), (2, 1, 2, 2), (3, 2, 2, 2), (2000, 2000, 2000, 2000)):
        a = [arr(n) for n in lens]
        assert ingest(jni.fake_env(), None, 0, None, a[0], a[1], a[2], a[3], b"JJ", 0, 1) == 0
        exc = exception(jni)
        assert exc is not None and exc[0] == "java/lang/IllegalArgumentException" and "one length" in exc[1]
