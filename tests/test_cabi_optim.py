"""CPU-side checks of the clipping entry points (csrc/optim_clip.hip): declared in include/amid_hip.h, exported by the built library, and
their argument checks answer before anything touches a device."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

NEW = ["amid_grad_sqnorm_workspace_bytes", "amid_grad_sqnorm_f32", "amid_optimizer_step_clip_f32"]
ARG = -1


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_and_exported(name):
    assert name in _lib.parse_header()
    assert name in _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())


def test_the_clip_step_takes_the_plain_step_s_arguments_plus_two():
    protos = _lib.parse_header()
    plain, clip = protos["amid_optimizer_step_f32"], protos["amid_optimizer_step_clip_f32"]
    assert clip[2][:-3] == plain[2][:-1] and clip[2][-3:] == ["sqnorm", "max_norm", "stream"]
    assert clip[1][:-3] == plain[1][:-1] and clip[1][-3:] == [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]


def _bufs():
    buf = (ctypes.c_float * 260)()
    ibuf = (ctypes.c_int * 16)()
    base = ctypes.addressof(buf)
    base += (-base) % 16                                   # the entries want 16-byte boundaries
    return (buf, ibuf), ctypes.c_void_p(base), ctypes.cast(ibuf, ctypes.c_void_p)


def test_the_workspace_size():
    assert _lib.lib()._fn["amid_grad_sqnorm_workspace_bytes"]() >= 8


def test_the_norm_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib()._fn["amid_grad_sqnorm_f32"]
    keep, p, ip = _bufs()
    # (g_dense, n_dense, uniq_grad, n_uniq, cap, D, ws, out, stream)
    good = [p, 8, p, ip, 4, 64, p, p, None]
    for i in (0, 2, 3, 6, 7):
        a = list(good)
        a[i] = None
        assert f(*a) == ARG, i
    for i, bad in ((1, -1), (4, -1), (5, 0), (5, -64), (5, 6), (5, 66)):
        a = list(good)
        a[i] = bad
        assert f(*a) == ARG, (i, bad)
    a = list(good)
    a[0] = ctypes.c_void_p(p.value + 4)                    # a quad load off its boundary
    assert f(*a) == ARG
    a = list(good)
    a[2] = ctypes.c_void_p(p.value + 8)
    assert f(*a) == ARG
    del keep


def test_the_clip_step_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib()._fn["amid_optimizer_step_clip_f32"]
    keep, p, ip = _bufs()
    # (p, m, v, g, n, table, m_tab, v_tab, last, uniq_ids, n_uniq, n_uniq_max, uniq_grad, D, grad_scale, step_state, sqnorm, max_norm, stream)
    good = [p, p, p, p, 8, p, p, p, ip, ip, ip, 4, p, 64, 1.0, p, p, 1.0, None]
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 12, 15, 16):
        a = list(good)
        a[i] = None
        assert f(*a) == ARG, i
    for i, bad in ((4, -1), (11, 0), (11, -3), (13, 0), (13, -64), (13, 6), (17, -1.0), (17, float("nan"))):
        a = list(good)
        a[i] = bad
        assert f(*a) == ARG, (i, bad)
    del keep
