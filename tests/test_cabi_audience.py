"""CPU-side checks of the audience top-K entry points (csrc/audience.hip): declared in include/amid_hip.h, bound by _lib, exported by the built
library; their argument checks answer with stream = None and host buffers, before anything touches a device; and the workspace size is
negative for bad sizes and does not fall when Q, either row count or k grows."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

NEW = ["amid_audience_workspace_bytes", "amid_audience_halves_f32", "amid_audience_topk_f32", "amid_audience_target_workgroups"]
ARG, UNSUPPORTED = -1, -2
HALVES = ["vectors", "n_vectors", "slots_d1", "n_d1", "slots_d2", "n_d2", "w1", "b1", "D", "hid", "workspace", "flags", "stream"]
TOPK = ["items", "item_domain", "Q", "table", "n_rows", "w1", "w2", "b2", "slots_d1", "n_d1", "slots_d2", "n_d2", "holders", "holders_off", "D",
        "hid", "k", "workspace", "flags", "rows", "scores", "stream"]


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_bound_and_exported(name):
    assert name in _lib.parse_header()
    assert name in _lib.declared_symbols()
    assert _lib.lib().raw(name) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())


def test_header_and_library_export_the_same_audience_set():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("amid_audience_")}
    assert exported == set(NEW) == {n for n in _lib.declared_symbols() if n.startswith("amid_audience_")}


def test_parameter_names_are_the_header_s():
    protos = _lib.parse_header()
    assert protos["amid_audience_halves_f32"][2] == HALVES
    assert protos["amid_audience_topk_f32"][2] == TOPK
    assert protos["amid_audience_workspace_bytes"][2] == ["Q", "n_d1", "n_d2", "hid", "k"]


def _good():
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    halves = dict(vectors=p, n_vectors=20, slots_d1=p, n_d1=8, slots_d2=p, n_d2=5, w1=p, b1=p, D=128, hid=32, workspace=p, flags=p, stream=None)
    topk = dict(items=p, item_domain=p, Q=4, table=p, n_rows=16, w1=p, w2=p, b2=p, slots_d1=p, n_d1=8, slots_d2=p, n_d2=5, holders=p,
                holders_off=p, D=128, hid=32, k=5, workspace=p, flags=p, rows=p, scores=p, stream=None)
    return buf, halves, topk


def _call(name, names, good, **change):
    a = dict(good, **change)
    return _lib.lib().raw(name)(*[a[n] for n in names])


def test_null_pointers_are_refused_without_a_gpu():
    keep, halves, topk = _good()
    for n in ("vectors", "w1", "b1", "workspace", "flags", "slots_d1", "slots_d2"):
        assert _call("amid_audience_halves_f32", HALVES, halves, **{n: None}) == ARG, n
    for n in ("items", "item_domain", "table", "w1", "w2", "b2", "workspace", "flags", "rows", "scores", "slots_d1", "slots_d2", "holders_off"):
        assert _call("amid_audience_topk_f32", TOPK, topk, **{n: None}) == ARG, n
    del keep


def test_bad_sizes_are_refused_without_a_gpu():
    keep, halves, topk = _good()
    big = 2 ** 31 - 1
    for ch in (dict(n_vectors=0), dict(n_vectors=-1), dict(n_vectors=big), dict(n_d1=-1), dict(n_d2=-1), dict(n_d1=0, n_d2=0),
               dict(n_d1=big), dict(n_d2=big), dict(n_d1=2 ** 30, n_d2=2 ** 30)):
        assert _call("amid_audience_halves_f32", HALVES, halves, **ch) == ARG, ch
    for ch in (dict(Q=0), dict(Q=-1), dict(k=0), dict(k=-1), dict(k=257), dict(n_rows=0), dict(n_rows=-1), dict(n_d1=-1), dict(n_d2=-1),
               dict(n_d1=0, n_d2=0), dict(n_d1=big), dict(n_d2=big), dict(n_d1=2 ** 30, n_d2=2 ** 30)):
        assert _call("amid_audience_topk_f32", TOPK, topk, **ch) == ARG, ch
    for name, names, good in (("amid_audience_halves_f32", HALVES, halves), ("amid_audience_topk_f32", TOPK, topk)):
        for ch in (dict(D=32), dict(D=96), dict(D=256), dict(hid=8), dict(hid=48), dict(hid=128)):
            assert _call(name, names, good, **ch) == UNSUPPORTED, (name, ch)
    assert _call("amid_audience_topk_f32", TOPK, topk, k=256, D=32) == UNSUPPORTED      # (k = 256 itself is in range: the next check is D's)
    del keep


def test_the_target_workgroup_count_is_clamped_and_restored():
    f = _lib.lib().raw("amid_audience_target_workgroups")
    assert f(0) == 1024 and f(3) == 1024 and f(5000) == 3 and f(-5) == 1024 and f(0) == 1024


def test_the_workspace_size():
    w = _lib.lib().raw("amid_audience_workspace_bytes")
    assert w(4, 16, 3, 32, 5) > 0 and w(4, 0, 3, 16, 5) > 0 and w(4, 16, 0, 64, 5) > 0
    big = 2 ** 31 - 1
    for bad in ((0, 16, 3, 32, 5), (-1, 16, 3, 32, 5), (4, 16, 3, 32, 0), (4, 16, 3, 32, -1), (4, 16, 3, 32, 257), (4, -1, 3, 32, 5),
                (4, 16, -1, 32, 5), (4, 0, 0, 32, 5), (4, big, 3, 32, 5), (4, 16, big, 32, 5), (4, 2 ** 30, 2 ** 30, 32, 5),
                (4, 16, 3, 8, 5), (4, 16, 3, 0, 5), (4, 16, 3, 48, 5), (4, 16, 3, 128, 5)):
        assert w(*bad) < 0, bad
    Qs = [1, 7, 8, 9, 40, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 8192, 8193]
    Ns = [1, 255, 256, 257, 700, 894820, 10_000_000]
    Ks = [1, 2, 10, 100, 255, 256]
    for hid in (16, 32, 64):
        for other in (0, 1, 300):
            for n in Ns:
                for k in Ks:
                    sizes = [w(Q, n, other, hid, k) for Q in Qs]
                    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), ("Q", n, other, k)
                    assert [w(Q, other, n, hid, k) for Q in Qs] == sorted(w(Q, other, n, hid, k) for Q in Qs), ("Q", other, n, k)
            for Q in Qs:
                for k in Ks:
                    sizes = [w(Q, n, other, hid, k) for n in Ns]
                    assert sizes == sorted(sizes), ("n_d1", Q, other, k)
                    sizes = [w(Q, other, n, hid, k) for n in Ns]
                    assert sizes == sorted(sizes), ("n_d2", Q, other, k)
                for n in Ns:
                    sizes = [w(Q, n, other, hid, k) for k in Ks]
                    assert sizes == sorted(sizes), ("k", Q, n, other)
    # dense sweeps where the query-group and range counts step
    for k in (10, 100):
        sizes = [w(Q, 894820, 700, 32, k) for Q in range(1, 1100)]
        assert sizes == sorted(sizes)
        sizes = [w(256, n, 300, 32, k) for n in range(0, 3000)]
        assert sizes == sorted(sizes)
        sizes = [w(256, 300, n, 32, k) for n in range(0, 3000)]
        assert sizes == sorted(sizes)
    sizes = [w(100, 5000, 17, 32, k) for k in range(1, 257)]
    assert sizes == sorted(sizes)
    # the halves launch's share is the head of every workspace
    assert w(1, 700, 300, 32, 1) >= 1000 * 32 * 4
