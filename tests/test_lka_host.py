"""CPU-side tests of the large-kernel-attention entry points: the two shape predicates answer without a device, the entry points reject
null descriptors / buffers, unsupported dtypes and shapes and misaligned buffers before any HIP call, and the ctypes descriptors have
the C layout."""
import ctypes
import os
import subprocess

from conftest import REPO

F16, F32 = 0, 1


def _dw(**kw):
    from tlxcv_amd import _lib
    return _lib.LkaDwDesc(**dict(dict(dtype=F16, N=2, H=14, W=14, C=160, x_ld=160, y_ld=160), **kw))


def _gate(**kw):
    from tlxcv_amd import _lib
    return _lib.LkaGateDesc(**dict(dict(dtype=F16, rows=392, C=160, a1_ld=160, t_ld=160, res_ld=160, y_ld=160), **kw))


def test_lka_dw_predicate_without_a_gpu():
    from tlxcv_amd import _lib
    lib = _lib.load()
    # every VAN_B0 stage shape at 224 x 224 and at 96 x 160, batch 256, and the kernel tests' extents
    for H, W in ((56, 56), (28, 28), (14, 14), (7, 7), (24, 40), (12, 20), (6, 10), (3, 5), (1, 1), (57, 3), (3, 57), (1, 57), (57, 1), (23, 24)):
        for Cc in (8, 32, 64, 160, 256, 264):
            assert lib.tlxmi_lka_dw_supported(_dw(N=256, H=H, W=W, C=Cc, x_ld=Cc, y_ld=Cc + 8)) == 1, (H, W, Cc)
    assert lib.tlxmi_lka_dw_supported(None) == 0
    for kw in (dict(dtype=F32), dict(dtype=5), dict(C=164), dict(C=4, x_ld=8, y_ld=8), dict(x_ld=152), dict(y_ld=152), dict(x_ld=164),
               dict(y_ld=172), dict(W=88), dict(W=0), dict(H=0), dict(N=0), dict(N=-1)):
        assert lib.tlxmi_lka_dw_supported(_dw(**kw)) == 0, kw
    assert lib.tlxmi_lka_dw_supported(_dw(W=87, H=1000)) == 1
    # 32-bit byte offsets: ((pixels - 1) * ld + C) * 2 < 2^31 for x and for y
    n_ok = (2 ** 31 // 2 - 160) // (196 * 160)
    assert lib.tlxmi_lka_dw_supported(_dw(N=n_ok)) == 1 and lib.tlxmi_lka_dw_supported(_dw(N=n_ok + 1)) == 0
    assert lib.tlxmi_lka_dw_supported(_dw(N=n_ok, y_ld=168)) == 0 and lib.tlxmi_lka_dw_supported(_dw(N=n_ok, x_ld=168)) == 0


def test_lka_gate_predicate_without_a_gpu():
    from tlxcv_amd import _lib
    lib = _lib.load()
    for Cc in (32, 64, 96, 128, 160, 192, 224, 256):
        for rows in (1, 49, 256 * 49, 256 * 56 * 56):
            if rows * Cc * 2 < 2 ** 31:
                assert lib.tlxmi_lka_gate_supported(_gate(rows=rows, C=Cc, a1_ld=Cc, t_ld=Cc, res_ld=Cc, y_ld=Cc)) == 1, (rows, Cc)
    assert lib.tlxmi_lka_gate_supported(_gate(rows=256 * 56 * 56, C=32, a1_ld=32, t_ld=32, res_ld=32, y_ld=32)) == 1     # VAN_B0 stage 1, batch 256
    assert lib.tlxmi_lka_gate_supported(None) == 0
    for kw in (dict(dtype=F32), dict(C=320, a1_ld=320, t_ld=320, res_ld=320, y_ld=320), dict(C=48), dict(C=16), dict(C=0), dict(rows=0),
               dict(a1_ld=152), dict(t_ld=164), dict(res_ld=0), dict(y_ld=156)):
        assert lib.tlxmi_lka_gate_supported(_gate(**kw)) == 0, kw
    r_ok = (2 ** 31 - 1) // (168 * 2)
    assert lib.tlxmi_lka_gate_supported(_gate(rows=r_ok, y_ld=168)) == 1 and lib.tlxmi_lka_gate_supported(_gate(rows=r_ok + 1, y_ld=168)) == 0


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from tlxcv_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 8192)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, q, r, t = (ctypes.c_void_p(base + 1024 * i) for i in range(4))
    odd8 = ctypes.c_void_p(base + 8)
    err = lambda: lib.tlxmi_last_error()      # noqa: E731
    B = ctypes.byref
    # lka_dw(desc, x, w0, b0, w1, b1, y, stream)
    assert lib.tlxmi_lka_dw(None, p, q, None, r, None, t, None) == -1 and b"null" in err()
    assert lib.tlxmi_lka_dw(B(_dw()), None, q, None, r, None, t, None) == -1 and b"null" in err()
    assert lib.tlxmi_lka_dw(B(_dw()), p, q, None, None, None, t, None) == -1
    assert lib.tlxmi_lka_dw(B(_dw(dtype=F32)), p, q, None, r, None, t, None) == -2 and b"unsupported geometry" in err()
    assert lib.tlxmi_lka_dw(B(_dw(C=164)), p, q, None, r, None, t, None) == -2
    assert lib.tlxmi_lka_dw(B(_dw(W=88)), p, q, None, r, None, t, None) == -2 and b"W <= 87" in err()
    assert lib.tlxmi_lka_dw(B(_dw()), odd8, q, None, r, None, t, None) == -3 and b"aligned" in err()
    assert lib.tlxmi_lka_dw(B(_dw()), p, q, None, r, None, odd8, None) == -3
    # lka_gate(desc, a1, t, w1, scale1, shift1, w2, scale2, shift2, res, res_scale, y, stream)
    g = _gate()
    assert lib.tlxmi_lka_gate(None, p, q, r, None, None, r, None, None, t, None, t, None) == -1 and b"null" in err()
    assert lib.tlxmi_lka_gate(B(g), p, q, r, None, None, r, None, None, None, None, t, None) == -1 and b"null" in err()
    assert lib.tlxmi_lka_gate(B(_gate(dtype=F32)), p, q, r, None, None, r, None, None, t, None, t, None) == -2 and b"unsupported geometry" in err()
    assert lib.tlxmi_lka_gate(B(_gate(C=48)), p, q, r, None, None, r, None, None, t, None, t, None) == -2
    assert lib.tlxmi_lka_gate(B(_gate(C=320, a1_ld=320, t_ld=320, res_ld=320, y_ld=320)), p, q, r, None, None, r, None, None, t, None, t, None) == -2
    assert lib.tlxmi_lka_gate(B(g), p, q, r, None, odd8, r, None, None, t, None, t, None) == -3 and b"aligned" in err()
    assert lib.tlxmi_lka_gate(B(g), p, q, r, None, None, r, None, None, t, None, odd8, None) == -3
    # mul(a, b, y, dtype, rows, C, a_ld, b_ld, y_ld, stream)
    assert lib.tlxmi_mul(None, q, r, F16, 4, 16, 16, 16, 16, None) == -1
    assert lib.tlxmi_mul(p, q, r, 7, 4, 16, 16, 16, 16, None) == -1 and b"dtype" in err()
    assert lib.tlxmi_mul(p, q, r, F16, 4, 12, 16, 16, 16, None) == -3 and b"16-byte chunks" in err()
    assert lib.tlxmi_mul(p, q, r, F32, 4, 16, 16, 12, 16, None) == -3 and b"stride" in err()
    assert lib.tlxmi_mul(p, q, odd8, F16, 4, 16, 16, 16, 16, None) == -3 and b"aligned" in err()
    assert lib.tlxmi_mul(p, q, r, F16, 0, 16, 16, 16, 16, None) == -1


def test_descriptor_layout_matches_c(tmp_path):
    from tlxcv_amd import _lib
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "tlxmi.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tlxmi_lka_dw_desc), offsetof(tlxmi_lka_dw_desc, y_ld),'
        ' sizeof(tlxmi_lka_gate_desc), offsetof(tlxmi_lka_gate_desc, rows), offsetof(tlxmi_lka_gate_desc, C),'
        ' offsetof(tlxmi_lka_gate_desc, a1_ld), offsetof(tlxmi_lka_gate_desc, y_ld));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    G = _lib.LkaGateDesc
    assert got == [ctypes.sizeof(_lib.LkaDwDesc), _lib.LkaDwDesc.y_ld.offset, ctypes.sizeof(G), G.rows.offset, G.C.offset, G.a1_ld.offset,
                   G.y_ld.offset]
    assert got[0] == 28 and got[2] == 40
