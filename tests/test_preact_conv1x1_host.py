"""CPU-side tests of tlxmi_preact_conv1x1: the predicate — pure host code — answers by the rules of include/tlxmi.h, the entry point
refuses bad calls with distinct codes and messages before anything is launched, and the engine has the "preact" switch, on."""
import ctypes as C

F16, F32, NONE, RELU = 0, 1, 0, 1


def _lib():
    from tlxcv_amd import _lib
    return _lib.load()


def test_predicate_truth_table():
    ok = _lib().tlxmi_preact_conv1x1_supported
    assert ok(F16, 3136, 64, 128, 256, 128, RELU, RELU) == 1
    for rows, K, x_ld, Cout in ((49, 32, 64, 128), (129, 72, 256, 192), (1000, 224, 256, 256), (49, 992, 1024, 128), (129, 144, 384, 192)):
        assert ok(F16, rows, K, Cout, x_ld, Cout + 128, RELU, RELU) == 1, (rows, K, x_ld, Cout)
    assert ok(F16, 49, 8, 8, 8, 8, NONE, NONE) == 1
    assert ok(F32, 3136, 64, 128, 256, 128, RELU, RELU) == 0           # fp16 only
    assert ok(F16, 3136, 36, 128, 256, 128, RELU, RELU) == 0           # K is a multiple of 8
    assert ok(F16, 3136, 64, 128, 56, 128, RELU, RELU) == 0            # x_ld >= K
    assert ok(F16, 3136, 64, 100, 256, 128, RELU, RELU) == 0           # Cout is a multiple of 8
    assert ok(F16, 3136, 64, 128, 256, 120, RELU, RELU) == 0           # y_ld >= Cout
    assert ok(F16, 3136, 64, 128, 260, 128, RELU, RELU) == 0 and ok(F16, 3136, 64, 128, 256, 132, RELU, RELU) == 0
    assert ok(F16, 3136, 0, 128, 256, 128, RELU, RELU) == 0 and ok(F16, 0, 64, 128, 256, 128, RELU, RELU) == 0
    assert ok(F16, 3136, 64, 128, 256, 128, 2, RELU) == 0 and ok(F16, 3136, 64, 128, 256, 128, RELU, 6) == 0
    assert _lib().tlxmi_version() == 101


def test_two_gib_limit():
    ok = _lib().tlxmi_preact_conv1x1_supported
    rows = (1 << 31) // (1024 * 2)
    assert rows * 1024 * 2 == 1 << 31
    assert ok(F16, rows, 64, 128, 1024, 128, RELU, RELU) == 0          # rows * x_ld * 2 == 2^31
    assert ok(F16, rows - 1, 64, 128, 1024, 128, RELU, RELU) == 1
    assert ok(F16, rows, 64, 128, 64, 1024, RELU, RELU) == 0           # the same for y
    assert ok(F16, rows - 1, 64, 128, 64, 1024, RELU, RELU) == 1
    assert ok(F16, 1 << 40, 8, 8, 8, 8, RELU, RELU) == 0


def test_entry_point_refuses_bad_calls_without_a_device():
    import numpy as np
    lib = _lib()
    buf = np.zeros(8192, dtype=np.uint8)
    base = (buf.ctypes.data + 255) & ~255
    p, q, r, t, w = (C.c_void_p(base + 1024 * i) for i in range(5))
    odd = C.c_void_p(base + 8)
    call = lib.tlxmi_preact_conv1x1
    err = lib.tlxmi_last_error
    assert call(F16, 49, 64, 128, 256, 128, None, q, r, RELU, w, None, None, RELU, t, None) == -1 and b"null" in err()
    assert call(F16, 49, 64, 128, 256, 128, p, None, r, RELU, w, None, None, RELU, t, None) == -1
    assert call(F16, 49, 64, 128, 256, 128, p, q, r, RELU, w, None, None, RELU, None, None) == -1
    assert call(F16, 49, 36, 128, 256, 128, p, q, r, RELU, w, None, None, RELU, t, None) == -2 and b"unsupported geometry" in err()
    assert call(F32, 49, 64, 128, 256, 128, p, q, r, RELU, w, None, None, RELU, t, None) == -2
    assert call(F16, 49, 64, 128, 256, 128, odd, q, r, RELU, w, None, None, RELU, t, None) == -3 and b"16-byte aligned" in err()
    assert call(F16, 49, 64, 128, 256, 128, p, q, r, RELU, w, None, None, RELU, odd, None) == -3
    assert call(F16, 49, 64, 128, 256, 128, p, q, r, RELU, odd, None, None, RELU, t, None) == -3


def test_dispatch_option_exists_and_is_on():
    import pytest
    from tlxcv_amd import engine as E
    assert E.option("preact") is True
    E.set_option("preact", False)
    try:
        assert E.option("preact") is False
    finally:
        E.set_option("preact", True)
    with pytest.raises(KeyError):
        E.set_option("preact_", True)
