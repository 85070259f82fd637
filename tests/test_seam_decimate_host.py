"""CPU-side checks of the decimated seam's entry points (tlxmi_bottleneck_seam_dec, tlxmi_bottleneck_seam_dec_supported): the
predicate is pure host code and answers 1 exactly when the call is taken; the call validates before any HIP call."""
import ctypes

from tlxcv_amd import _lib

F16, F32, RELU = 0, 1, 1
SHAPES = [(64, 256, 128), (128, 512, 256)]


def _buffers():
    buf = (ctypes.c_char * 8192)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return buf, [ctypes.c_void_p(base + 1024 * i) for i in range(6)], ctypes.c_void_p(base + 8)


def _desc(K1, N1, N2, rows, dtype=F16, **kw):
    f = dict(dtype=dtype, rows=rows, K1=K1, N1=N1, N2=N2, t2_ld=K1, skip_ld=N1, y_ld=N1, t1_ld=N2, act=RELU)
    f.update(kw)
    return _lib.SeamDesc(**f)


def test_supported_answers_for_the_two_shapes_only():
    lib = _lib.load()
    for K1, N1, N2 in SHAPES:
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 12 * 6 * 6, 6, 6) == 1
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 2 * 7 * 5, 7, 5) == 1
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 2, 1, 1) == 1
        assert lib.tlxmi_bottleneck_seam_dec_supported(F32, K1, N1, N2, 12 * 6 * 6, 6, 6) == 0
        # rows that are not whole images
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 12 * 6 * 6 + 1, 6, 6) == 0
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 35, 7, 10) == 0
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 0, 6, 6) == 0
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 36, 0, 6) == 0
    # triples the full seam has a kernel for, but no decimated instance
    for K1, N1, N2 in [(64, 256, 64), (128, 512, 128), (256, 1024, 256), (128, 256, 256), (64, 512, 128), (128, 256, 128)]:
        assert lib.tlxmi_bottleneck_seam_supported(F16, K1, N1, N2) == 1
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, 12 * 6 * 6, 6, 6) == 0
    assert lib.tlxmi_bottleneck_seam_dec_supported(F16, 64, 250, 128, 36, 6, 6) == 0


def test_supported_keeps_its_promise_at_the_2_GiB_limit():
    """The widest operand of either shape is the skip map (N1 * 2 bytes a row): one row below the first row count at which it reaches
    2^31 bytes the predicate answers 1, at it 0, and the call refuses with TLXMI_ERR_UNSUPPORTED before any launch (the buffers
    handed over are tiny).  The compact y counts with its own rows: at 2 x 2 pixels an image it is a quarter of the skip map."""
    lib = _lib.load()
    _keep, (t2, w3, skip, y, w1, t1), _ = _buffers()
    big = 1 << 31
    for K1, N1, N2 in SHAPES:
        first = big // (2 * N1)
        assert (first - 1) * 2 * N1 < big <= first * 2 * N1
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, first - 1, 1, 1) == 1
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, first, 1, 1) == 0
        assert first % 4 == 0
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, first - 4, 2, 2) == 1
        assert lib.tlxmi_bottleneck_seam_dec_supported(F16, K1, N1, N2, first, 2, 2) == 0
        d = _desc(K1, N1, N2, first)
        rc = lib.tlxmi_bottleneck_seam_dec(ctypes.byref(d), 1, 1, t2, w3, None, None, skip, y, w1, None, None, t1, None)
        assert rc == -2 and b"2 GiB" in lib.tlxmi_last_error()


def test_call_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    _keep, (t2, w3, skip, y, w1, t1), odd = _buffers()
    err = lambda: lib.tlxmi_last_error()      # noqa: E731
    call = lambda d, H, W, **kw: lib.tlxmi_bottleneck_seam_dec(      # noqa: E731
        ctypes.byref(d), H, W, kw.get("t2", t2), w3, None, None, kw.get("skip", skip), kw.get("y", y), w1, None, None, kw.get("t1", t1), None)
    K1, N1, N2 = SHAPES[0]
    d = _desc(K1, N1, N2, 72)
    assert lib.tlxmi_bottleneck_seam_dec(None, 6, 6, t2, w3, None, None, skip, y, w1, None, None, t1, None) == -1 and b"null" in err()
    for name in ("t2", "skip", "y", "t1"):
        assert call(d, 6, 6, **{name: None}) == -1 and b"null" in err()
        assert call(d, 6, 6, **{name: odd}) == -3 and b"16-byte" in err()
    # rows that are not N * H * W
    assert call(d, 7, 5) == -1 and b"whole number" in err()
    assert call(_desc(K1, N1, N2, 73), 6, 6) == -1 and b"whole number" in err()
    assert call(d, 0, 6) == -1 and b"extent" in err()
    assert call(_desc(K1, N1, N2, 72, dtype=F32), 6, 6) == -2 and b"fp16" in err()
    assert call(_desc(64, 256, 64, 72), 6, 6) == -2 and b"no kernel" in err()
    assert call(_desc(K1, N1, N2, 72, y_ld=N1 - 8), 6, 6) == -1 and b"stride" in err()
    assert call(_desc(K1, N1, N2, 72, t1_ld=N2 + 4), 6, 6) == -3
    assert call(_desc(K1, N1, N2, 72, act=0), 6, 6) == -2 and b"ReLU" in err()


def test_symbol_table_has_the_pair():
    assert "tlxmi_bottleneck_seam_dec" in _lib.ALL_SYMBOLS and "tlxmi_bottleneck_seam_dec_supported" in _lib.ALL_SYMBOLS
    lib = _lib.load()
    assert lib.tlxmi_version() == 101
