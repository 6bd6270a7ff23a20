"""CPU-side checks of BERT4Rec's one-launch inference encoder (amid_bert_seq_fwd_gather_infer_f32, csrc/bert_seq_infer.hip): declared in
include/amid_hip.h, exported by the built library, and its shape / argument checks answer before anything touches a device."""
import ctypes
import subprocess

from amid_amd import _lib

NEW = ("amid_bert_seq_infer_supported", "amid_bert_seq_fwd_gather_infer_f32")


def test_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in protos and name in _lib.declared_symbols()
        assert name in exported
    # (x_out, 12 pointer arrays, B, T, live, table, n_rows, idx_all, seq_d2, stream)
    assert len(protos["amid_bert_seq_fwd_gather_infer_f32"][1]) == 21
    assert len(protos["amid_bert_seq_infer_supported"][1]) == 4


def test_supported_shapes():
    f = _lib.lib()._fn["amid_bert_seq_infer_supported"]
    for B, T, D, H in ((1, 1, 128, 4), (256, 64, 128, 4), (7, 17, 128, 4)):
        assert f(B, T, D, H) == 1
    assert f(8, 65, 128, 4) == 0        # more rows than a workgroup's four strips
    assert f(8, 50, 64, 4) == 0         # the reference hard-codes hidden 128
    assert f(8, 50, 128, 8) == 0        # ... and 4 heads
    assert f(0, 50, 128, 4) == 0 and f(8, 0, 128, 4) == 0


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib()._fn["amid_bert_seq_fwd_gather_infer_f32"]
    null = None
    buf = (ctypes.c_float * 256)()
    ibuf = (ctypes.c_int * 16)()
    lbuf = (ctypes.c_longlong * 16)()
    p, ip, lp = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p), ctypes.cast(lbuf, ctypes.c_void_p)
    a4 = (ctypes.c_void_p * 4)(*[p.value] * 4)
    a12 = (ctypes.c_void_p * 12)(*[p.value] * 12)
    fam = [a4, a4, a12, a12, a4, a4, a4, a4, a4, a4, a4, a4]      # la1 lb1 w3 b3 wo bo la2 lb2 w1 b1 w2 b2
    tail = (ip, p, 100, ip, lp, null)                             # live, table, n_rows, idx_all, seq_d2, stream
    assert f(null, *[null] * 12, 4, 50, null, null, 100, null, null, null) == -1      # every pointer null
    assert f(null, *fam, 4, 50, *tail) == -1                                           # no output
    for i in range(12):                                                                # a family missing
        bad = list(fam)
        bad[i] = null
        assert f(p, *bad, 4, 50, *tail) == -1, i
    hole4 = (ctypes.c_void_p * 4)(p.value, p.value, None, p.value)                     # ... or one of its entries
    hole12 = (ctypes.c_void_p * 12)(*([p.value] * 7 + [None] + [p.value] * 4))
    assert f(p, hole4, *fam[1:], 4, 50, *tail) == -1
    assert f(p, *fam[:2], hole12, *fam[3:], 4, 50, *tail) == -1
    assert f(p, *fam[:9], hole4, *fam[10:], 4, 50, *tail) == -1
    assert f(p, *fam, 4, 50, null, p, 100, ip, lp, null) == -1                         # no live list
    assert f(p, *fam, 4, 50, ip, null, 100, ip, lp, null) == -1                        # no table
    assert f(p, *fam, 4, 50, ip, p, 0, ip, lp, null) == -1                             # an empty table
    assert f(p, *fam, 4, 50, ip, p, 100, null, lp, null) == -1                         # no index list
    assert f(p, *fam, 4, 50, ip, p, 100, ip, null, null) == -1                         # no seq_d2 (the key mask)
    assert f(p, *fam, 0, 50, *tail) == -1                                              # B 0
    assert f(p, *fam, 4, 0, *tail) == -1                                               # T 0
    assert f(p, *fam, 4, 65, *tail) == -2                                              # T 65: not this kernel's shape
    assert f(p, *fam, 1 << 20, 64, *tail) == -2                                        # an output beyond a buffer descriptor's 2 GiB


def test_strip_entry_points_still_refuse_missing_operands():
    """NULL now means "do not store" for the tensors only a backward reads; the operands and the outputs the next launch reads stay required."""
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a2 = (ctypes.c_void_p * 2)(p.value, p.value)
    a6 = (ctypes.c_void_p * 6)(*[p.value] * 6)
    f = L._fn["amid_bert_strip_qkv_fwd_pro_p3_f32"]
    # (x, la, lb, w3, b3, B, T, live, y, q, k, v, seq_d2, n_keys, key_keep, tr_src, tr_dst, tr_rows, tr_cols, n_tr, stream)
    assert f(None, a2, a2, a6, a6, 4, 50, None, None, p, p, p, None, 0, None, None, None, None, None, 0, None) == -1      # no input
    assert f(p, a2, a2, a6, a6, 4, 50, None, None, None, p, p, None, 0, None, None, None, None, None, 0, None) == -1      # no q
    g = L._fn["amid_bert_strip_oproj_ffn_fwd_p3_f32"]
    # (o, x, wo, bo, la, lb, w1, b1, w2, b2, B, T, live, layer, step_state, train, p_drop, x1, y2, pre, h, x2, nla, nlb, nw3, nb3, ny, nq, nk, nv, stream)
    assert g(p, p, a2, a2, a2, a2, a2, a2, a2, a2, 4, 50, None, 0, None, 0, 0.1, None, None, None, None, None, None, None, None, None, None,
             None, None, None, None) == -1                                                                                # no block output
    assert g(p, p, a2, a2, a2, a2, a2, a2, a2, a2, 4, 50, None, 0, None, 0, 0.1, None, None, None, None, p, a2, a2, a6, a6, None, None, p, p,
             None) == -1                                                                                                  # the next block's q missing
