"""CPU-side checks of the evaluation head on given user vectors (amid_eval_head_u_f32): declared in include/amid_hip.h, exported by the
built library, and its argument checks answer before anything touches a device."""
import ctypes
import subprocess

from amid_amd import _lib


def test_entry_point_is_declared_and_exported():
    assert "amid_eval_head_u_f32" in _lib.parse_header()
    assert "amid_eval_head_u_f32" in _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == "amid_eval_head_u_f32" and " T " in ln for ln in out.splitlines())


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    f = L._fn["amid_eval_head_u_f32"]
    null = None
    buf = (ctypes.c_float * 256)()
    ibuf = (ctypes.c_int * 16)()
    dom = (ctypes.c_longlong * 4)()
    p, ip, dp = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p), ctypes.cast(dom, ctypes.c_void_p)
    pp = (ctypes.c_void_p * 2)(p.value, p.value)
    nomix = (null, null, null, null, null, 0.0, null)
    # (u_src, u_dom_stride, table, ids, w1, b1, w2, b2, labels, domain_id, B, NI, D, hid, fix_value, u, p, rank, rank_raw, loss_part,
    #  itc_s, w_nn, b_nn, w_bs, b_bs, threshold, gate, stream)
    assert f(null, 0, *[null] * 8, 4, 100, 128, 32, 1e-7, null, null, null, null, null, *nomix, null) == -1                # every pointer null
    assert f(null, 0, p, ip, p, p, p, p, null, dp, 4, 4, 128, 32, 1e-7, null, null, ip, ip, null, *nomix, null) == -1        # no user vectors
    assert f(p, -1, p, ip, p, p, p, p, null, dp, 4, 4, 128, 32, 1e-7, null, null, ip, ip, null, *nomix, null) == -1          # a negative domain stride
    assert f(p, 0, p, ip, p, p, p, p, p, dp, 4, 4, 128, 32, 1e-7, null, null, ip, ip, null, *nomix, null) == -1              # labels without loss_part
    assert f(p, 0, p, ip, p, p, p, p, null, dp, 4, 4, 128, 32, 1e-7, null, null, null, null, null, *nomix, null) == -1       # no output at all
    assert f(p, 0, p, ip, p, p, p, p, null, dp, 4, 4, 128, 32, 1e-7, p, null, ip, ip, null, *nomix, null) == -1              # u aliases u_src
    assert f(p, 0, p, ip, p, p, p, p, null, dp, 4, 4, 100, 32, 1e-7, null, null, ip, ip, null, *nomix, null) == -1           # D not a multiple of 32
    assert f(p, 0, p, ip, p, p, p, p, null, dp, 4, 4, 128, 30, 1e-7, null, null, ip, ip, null, *nomix, null) == -1           # hid not a multiple of 4
    assert f(p, 0, p, ip, p, p, p, p, null, dp, 4, 100000, 128, 32, 1e-7, null, null, ip, ip, null, *nomix, null) == -2      # more scores than LDS holds
    # the mix folded into the launch: its parameters come together, the vectors are u_raw [2, B, D], the shape is the mix kernel's 512-thread one
    assert f(p, 0, p, ip, p, p, p, p, null, dp, 4, 4, 128, 32, 1e-7, null, null, ip, ip, null, null, pp, pp, pp, pp, 0.5, null, null) == -1     # parameters without scores
    assert f(p, 64 * 128, p, ip, p, p, p, p, null, dp, 64, 4, 128, 32, 1e-7, null, null, ip, ip, null, p, pp, null, pp, pp, 0.5, null, null) == -1   # a family missing
    assert f(p, 0, p, ip, p, p, p, p, null, dp, 64, 4, 128, 32, 1e-7, null, null, ip, ip, null, p, pp, pp, pp, pp, 0.5, null, null) == -1       # not the [2, B, D] stride
    assert f(p, 4 * 128, p, ip, p, p, p, p, null, dp, 4, 4, 128, 32, 1e-7, null, null, ip, ip, null, p, pp, pp, pp, pp, 0.5, null, null) == -2   # B < 32: the looped mix
    assert f(p, 64 * 96, p, ip, p, p, p, p, null, dp, 64, 4, 96, 32, 1e-7, null, null, ip, ip, null, p, pp, pp, pp, pp, 0.5, null, null) == -2   # D 96
