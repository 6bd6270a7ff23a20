"""CPU-side checks of GRU4Rec's encoder entry points (csrc/gru.hip): declared in include/amid_hip.h, exported by the built library, and
their argument checks answer before anything touches a device."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

NEW = ["amid_gru_supported", "amid_gru_proj_fwd_f32", "amid_gru_rec_fwd_f32", "amid_gru_rec_fwd_infer_f32", "amid_gru_rec_bwd_f32",
       "amid_gru_dx_f32"]
ARG, UNSUPPORTED = -1, -2
BIG_B, BIG_T = 70000, 100          # 2 B T 3 D floats = 21.5 GB: beyond 32-bit byte offsets


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_and_exported(name):
    assert name in _lib.parse_header()
    assert name in _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())


def test_header_and_library_export_the_same_gru_set():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("amid_gru_")}
    assert exported == set(NEW) == {n for n in _lib.declared_symbols() if n.startswith("amid_gru_")}


def test_the_shape_query():
    q = _lib.lib()._fn["amid_gru_supported"]
    for shape in ((1, 1, 128), (256, 50, 128), (33, 20, 128), (6990, 100, 128)):
        assert q(*shape) == 1, shape
    # 2 B T 3 D floats as bytes against 2^31 - 16: B T <= 699 050
    assert q(699050, 1, 128) == 1 and q(699051, 1, 128) == 0
    for shape in ((0, 5, 128), (5, 0, 128), (-1, 5, 128), (5, 5, 64), (5, 5, 256), (5, 5, 0), (BIG_B, BIG_T, 128)):
        assert q(*shape) == 0, shape


def _bufs():
    buf = (ctypes.c_float * 256)()
    ibuf = (ctypes.c_int * 16)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    pp = (ctypes.c_void_p * 2)(p.value, p.value)
    half = (ctypes.c_void_p * 2)(p.value, None)
    return (buf, ibuf), p, ip, pp, half


def _refusals(f, good, ptrs, fams, iB, iT, iD, iL):
    """`good`: an argument list the entry would launch; ptrs: the indices of its required pointers; fams: of its two-pointer host arrays."""
    for i in ptrs:
        a = list(good)
        a[i] = None
        assert f(*a) == ARG, i
    for i in fams:
        a = list(good)
        a[i] = _bufs()[4]
        keep = a[i]                                                       # (alive across the call)
        assert f(*a) == ARG, i
        del keep
    for i, bad in ((iB, 0), (iB, -1), (iT, 0), (iT, -7), (iD, 0), (iD, -128)):
        a = list(good)
        a[i] = bad
        assert f(*a) == ARG, (i, bad)
    for D in (64, 96, 256):
        a = list(good)
        a[iD] = D
        assert f(*a) == UNSUPPORTED, D
    a = list(good)
    a[iB], a[iT] = BIG_B, BIG_T
    assert f(*a) == UNSUPPORTED
    a[iL] = None                                                          # ... with and without a live list alike
    assert f(*a) == UNSUPPORTED
    a = list(good)
    a[iL], a[iD] = None, 64
    assert f(*a) == UNSUPPORTED


def test_the_projection_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib()._fn["amid_gru_proj_fwd_f32"]
    keep, p, ip, pp, _ = _bufs()
    # (x, w_ih, b_ih, B, T, D, live, gi, stream)
    _refusals(f, [p, pp, pp, 3, 5, 128, ip, p, None], ptrs=(0, 1, 2, 7), fams=(1, 2), iB=3, iT=4, iD=5, iL=6)


def test_the_forward_recurrences_refuse_bad_arguments_without_a_gpu():
    keep, p, ip, pp, _ = _bufs()
    # (gi, w_hh, b_hh, B, T, D, live, h, gates, ghn, hprev, stream)
    _refusals(_lib.lib()._fn["amid_gru_rec_fwd_f32"], [p, pp, pp, 3, 5, 128, ip, p, p, p, p, None], ptrs=(0, 1, 2, 7, 8, 9, 10), fams=(1, 2),
              iB=3, iT=4, iD=5, iL=6)
    # (gi, w_hh, b_hh, B, T, D, live, h, stream)
    _refusals(_lib.lib()._fn["amid_gru_rec_fwd_infer_f32"], [p, pp, pp, 3, 5, 128, ip, p, None], ptrs=(0, 1, 2, 7), fams=(1, 2), iB=3, iT=4, iD=5, iL=6)


def test_the_backward_entries_refuse_bad_arguments_without_a_gpu():
    keep, p, ip, pp, _ = _bufs()
    # (dh, gates, ghn, hprev, w_hh, B, T, D, live, zero_dead, dgi, dgh, stream)
    _refusals(_lib.lib()._fn["amid_gru_rec_bwd_f32"], [p, p, p, p, pp, 3, 5, 128, ip, 1, p, p, None], ptrs=(0, 1, 2, 3, 4, 10, 11), fams=(4,),
              iB=5, iT=6, iD=7, iL=8)
    # (dgi, w_ih, B, T, D, live, zero_dead, dx, stream)
    _refusals(_lib.lib()._fn["amid_gru_dx_f32"], [p, pp, 3, 5, 128, ip, 0, p, None], ptrs=(0, 1, 7), fams=(1,), iB=2, iT=3, iD=4, iL=5)
