"""CPU-side checks of the pair-max on raw rows (csrc/intercomp.hip: amid_itc_pairmax_raw_f32, what GRU4Rec's InterComp scores its batch
rows with): declared in include/amid_hip.h, exported by the built library, and its argument checks answer before anything touches a
device -- a launch on a machine without a GPU would come back as a HIP error code, neither -1 nor -2."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

NAME = "amid_itc_pairmax_raw_f32"
ARG, UNSUPPORTED = -1, -2


def test_entry_point_is_declared_and_exported():
    assert NAME in _lib.parse_header()
    assert NAME in _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == NAME and " T " in ln for ln in out.splitlines())


def _good():
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (x, B, T, D, s, u_raw, stream)
    return buf, [p, 3, 5, 128, p, p, None]


@pytest.mark.parametrize("i", [0, 4])
def test_null_required_pointers_are_argument_errors(i):
    keep, a = _good()
    a[i] = None
    assert _lib.lib()._fn[NAME](*a) == ARG


@pytest.mark.parametrize("i,bad", [(1, 0), (1, -1), (2, 0), (2, -7), (3, 0), (3, -128), (3, 6)])
def test_bad_sizes_are_argument_errors(i, bad):
    keep, a = _good()
    a[i] = bad
    assert _lib.lib()._fn[NAME](*a) == ARG
    a[5] = None                                   # ... with and without the optional means
    assert _lib.lib()._fn[NAME](*a) == ARG


@pytest.mark.parametrize("T", [5, 154, 155, 300])
def test_a_wide_row_is_unsupported_in_both_forms(T):
    keep, a = _good()
    a[2], a[3] = T, 256
    assert _lib.lib()._fn[NAME](*a) == UNSUPPORTED
    a[3] = 132
    assert _lib.lib()._fn[NAME](*a) == UNSUPPORTED
