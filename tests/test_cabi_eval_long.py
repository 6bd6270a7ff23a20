"""CPU-side checks of the evaluation batch's entry points beyond 64 tokens (the long attention core over a live list in its inference form,
the inference forms of the two forward strip launches): declared in include/amid_hip.h, exported by the built library, and their argument
checks answer before anything touches a device."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

NEW = ["amid_attn_long_live_supported", "amid_attn_fwd_long_live_infer_f32", "amid_sas_strip_infer_supported",
       "amid_sas_strip_qkv_fwd_gather_infer_f32", "amid_sas_strip_oproj_ffn_fwd_infer_f32"]
ARG, UNSUPPORTED = -1, -2


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_and_exported(name):
    assert name in _lib.parse_header()
    assert name in _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())


def test_the_shape_queries():
    L = _lib.lib()
    q = L._fn["amid_attn_long_live_supported"]
    for shape in ((65, 128, 8), (150, 128, 8), (256, 128, 8)):
        assert q(*shape) == 1, shape
    for shape in ((64, 128, 8), (257, 128, 8), (100, 64, 8), (100, 128, 4), (0, 128, 8)):
        assert q(*shape) == 0, shape
    s = L._fn["amid_sas_strip_infer_supported"]
    assert s(65, 128) == 1 and s(150, 64) == 1
    assert s(0, 128) == 0 and s(100, 96) == 0 and s(100, 256) == 0


def _bufs():
    buf = (ctypes.c_float * 256)()
    ibuf = (ctypes.c_int * 16)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    pp = (ctypes.c_void_p * 2)(p.value, p.value)
    half = (ctypes.c_void_p * 2)(p.value, None)
    return (buf, ibuf), p, ip, pp, half


def test_the_attention_entry_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib()._fn["amid_attn_fwd_long_live_infer_f32"]
    keep, p, ip, _, _ = _bufs()
    # (q, k, v, B, T, D, H, o, live, stream)
    assert f(None, None, None, 3, 100, 128, 8, None, None, None) == ARG
    assert f(None, p, p, 3, 100, 128, 8, p, ip, None) == ARG
    assert f(p, p, p, 3, 100, 128, 8, None, ip, None) == ARG                  # no output
    assert f(p, p, p, 0, 100, 128, 8, p, ip, None) == ARG
    assert f(p, p, p, -3, 100, 128, 8, p, ip, None) == ARG
    assert f(p, p, p, 3, 0, 128, 8, p, ip, None) == ARG
    assert f(p, p, p, 3, 100, 0, 8, p, ip, None) == ARG
    assert f(p, p, p, 3, 100, 128, 0, p, ip, None) == ARG
    for T, D, H in ((64, 128, 8), (257, 128, 8), (100, 64, 8), (100, 128, 4)):
        assert f(p, p, p, 3, T, D, H, p, ip, None) == UNSUPPORTED, (T, D, H)
        assert f(p, p, p, 3, T, D, H, p, None, None) == UNSUPPORTED, (T, D, H)       # a null list is a list: the shape decides


def test_the_gathering_strip_entry_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib()._fn["amid_sas_strip_qkv_fwd_gather_infer_f32"]
    keep, p, ip, pp, half = _bufs()
    # (table, idx_all, pos0, pos1, ln_w, ln_b, w_in, b_in, ln_eps, B, T, D, live, tmq, qn, q, k, v, stream)
    good = [p, ip, p, p, pp, pp, pp, pp, 1e-8, 3, 100, 128, ip, p, p, p, p, p, None]
    assert f(*[None] * 8, 1e-8, 3, 100, 128, None, *[None] * 5, None) == ARG
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 13, 14, 15, 16, 17):                   # every operand but the (optional) live list
        a = list(good)
        a[i] = None
        assert f(*a) == ARG, i
    for i in (4, 5, 6, 7):                                                   # a family with one domain missing
        a = list(good)
        a[i] = half
        assert f(*a) == ARG, i
    for i, bad in ((9, 0), (9, -1), (10, 0), (10, -5), (11, 0), (11, -128)):
        a = list(good)
        a[i] = bad
        assert f(*a) == ARG, (i, bad)
    for D in (96, 256, 32):
        a = list(good)
        a[11] = D
        assert f(*a) == UNSUPPORTED, D


def test_the_inference_oproj_ffn_strip_entry_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib()._fn["amid_sas_strip_oproj_ffn_fwd_infer_f32"]
    keep, p, ip, pp, half = _bufs()
    # (o, qn, w_o, b_o, ln_w, ln_b, w1, b1, w2, b2, tmq, ln_eps, B, T, D, live, xo, nln_w, nln_b, nw_in, nb_in, nqn, nq, nk, nv, stream)
    last = [p, p, pp, pp, pp, pp, pp, pp, pp, pp, p, 1e-8, 3, 100, 128, ip, p, *[None] * 8, None]
    mid = [p, p, pp, pp, pp, pp, pp, pp, pp, pp, p, 1e-8, 3, 100, 128, ip, None, pp, pp, pp, pp, p, p, p, p, None]
    assert f(*[None] * 11, 1e-8, 3, 100, 128, None, *[None] * 9, None) == ARG
    for i in range(10):
        a = list(last)
        a[i] = None
        assert f(*a) == ARG, i
    for i in range(2, 10):
        a = list(last)
        a[i] = half
        assert f(*a) == ARG, i
    a = list(last)
    a[16] = None                                                              # the last layer's form without an output
    assert f(*a) == ARG
    for i in range(18, 25):                                                   # the next layer's epilogue with an operand missing
        a = list(mid)
        a[i] = None
        assert f(*a) == ARG, i
    a = list(mid)
    a[19] = half
    assert f(*a) == ARG
    for form in (last, mid):
        for i, bad in ((12, 0), (12, -1), (13, 0), (13, -7), (14, 0), (14, -64)):
            a = list(form)
            a[i] = bad
            assert f(*a) == ARG, (i, bad)
        for D in (96, 256):
            a = list(form)
            a[14] = D
            assert f(*a) == UNSUPPORTED, D
