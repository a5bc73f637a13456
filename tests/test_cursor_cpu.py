"""CPU-side checks of the match cursor (include/acgpu.h: acgpu_cursor_*): argument checks that need no device, the failure of a
valid open without one, and the cursor's JNI glue (ahocorasick_amd/java/jni/acgpu_jni_cursor.c) through a compiler and the
sanitizers over a mock JNIEnv and stubs of the C ABI (tests/jni_min/cursor_driver.c)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, Cursor, utf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JDIR = os.path.join(ROOT, "tests", "jni_min")


def test_cursor_argument_checks_without_device():
    L = N.lib()
    a = Automaton(N.MODE_ALL, ["ab"], True)
    hay = utf16("zabz")
    h = ctypes.c_void_p(123)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert L.acgpu_cursor_open(None, vp(hay), 4, N.REC_SET, ctypes.byref(h)) == N.E_INVALID
    assert not h.value  # (*out is cleared)
    assert L.acgpu_cursor_open(a.handle, None, 4, N.REC_SET, ctypes.byref(h)) == N.E_INVALID
    assert L.acgpu_cursor_open(a.handle, vp(hay), 4, N.REC_SET, None) == N.E_INVALID
    assert L.acgpu_cursor_open(a.handle, vp(hay), 4, 9, ctypes.byref(h)) == N.E_INVALID
    assert L.acgpu_cursor_open(a.handle, vp(hay), 1 << 31, N.REC_MAP, ctypes.byref(h)) == N.E_INVALID
    out = np.zeros(16, np.int32)
    n = ctypes.c_uint64(7)
    assert L.acgpu_cursor_next(None, vp(out), 4, ctypes.byref(n)) == N.E_INVALID
    st = N.CursorStats()
    assert L.acgpu_cursor_get_stats(None, ctypes.byref(st)) == N.E_INVALID
    L.acgpu_cursor_close(None)  # (a no-op)
    # the tunables exist, with their defaults
    for name, default in (("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20)):
        assert N.set_tunable(name, default) == default


def test_cursor_open_fails_loudly_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    a = Automaton(N.MODE_ALL, ["ab"], True)
    with pytest.raises(N.AcgpuError) as e:
        Cursor(a, utf16("zabz"), True)
    assert e.value.code in (N.E_NODEVICE, N.E_HIP)
    with pytest.raises(N.AcgpuError):
        list(a.pages(utf16("zabz"), False))


def test_cursor_jni_glue_compiles_warning_free_and_survives_the_sanitizers(tmp_path):
    exe = str(tmp_path / "jni_cursor")
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
           "-O1", "-I", JDIR, "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(JDIR, "cursor_driver.c"),
           os.path.join(JDIR, "cursor_env.c"), os.path.join(JDIR, "stub_acgpu.c"), os.path.join(JDIR, "stub_cursor.c")]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if b.returncode != 0 and b"asan" in b.stdout.lower() and b"cannot find" in b.stdout.lower():
        pytest.skip("no libasan in this toolchain")
    assert b.returncode == 0, b.stdout.decode(errors="replace")[-4000:]
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "all scenarios ok" in out and "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
