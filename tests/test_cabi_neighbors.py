"""CPU-side checks of the nearest-neighbour entry points (csrc/neighbors.hip): declared in include/amid_hip.h, bound by _lib, exported by the
built library; their argument checks answer with stream = None and host buffers, before anything touches a device; and the workspace size
is negative for bad sizes and does not fall when Q, n_cand or k grows."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

NEW = ["amid_neighbors_workspace_bytes", "amid_neighbors_f32", "amid_neighbors_target_workgroups"]
ARG, UNSUPPORTED = -1, -2
# (queries, query_ids, Q, base, n_rows, D, pool, n_pool, metric, k, exclude_self, workspace, flags, ids, scores, stream)
I_QV, I_QID, I_Q, I_BASE, I_NROWS, I_D, I_POOL, I_NPOOL, I_METRIC, I_K, I_EXCL, I_WS, I_FLAGS, I_IDS, I_SCORES = range(15)


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_bound_and_exported(name):
    assert name in _lib.parse_header()
    assert name in _lib.declared_symbols()
    assert _lib.lib().raw(name) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())


def test_header_and_library_export_the_same_neighbors_set():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("amid_neighbors_")}
    assert exported == set(NEW) == {n for n in _lib.declared_symbols() if n.startswith("amid_neighbors_")}


def test_parameter_names_are_the_issue_s():
    names = _lib.parse_header()["amid_neighbors_f32"][2]
    assert names == ["queries", "query_ids", "Q", "base", "n_rows", "D", "pool", "n_pool", "metric", "k", "exclude_self", "workspace", "flags",
                     "ids", "scores", "stream"]


def _good():
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    by_id = [None, p, 4, p, 16, 128, p, 8, 1, 5, 1, p, p, p, p, None]
    by_vec = [p, None, 4, p, 16, 128, None, 0, 0, 5, 0, p, p, p, p, None]
    return buf, p, by_id, by_vec


def test_null_pointers_are_refused_without_a_gpu():
    f = _lib.lib().raw("amid_neighbors_f32")
    keep, p, by_id, by_vec = _good()
    for good in (by_id, by_vec):
        for i in (I_BASE, I_WS, I_FLAGS, I_IDS, I_SCORES):
            a = list(good)
            a[i] = None
            assert f(*a) == ARG, i
    # exactly one of queries / query_ids
    a = list(by_id)
    a[I_QID] = None
    assert f(*a) == ARG
    a = list(by_id)
    a[I_QV] = p
    assert f(*a) == ARG
    # exclude_self needs query_ids
    a = list(by_vec)
    a[I_EXCL] = 1
    assert f(*a) == ARG
    del keep


def test_bad_sizes_are_refused_without_a_gpu():
    f = _lib.lib().raw("amid_neighbors_f32")
    keep, p, by_id, by_vec = _good()
    for good in (by_id, by_vec):
        for i in (I_Q, I_NROWS, I_K):
            for bad in (0, -1):
                a = list(good)
                a[i] = bad
                assert f(*a) == ARG, (i, bad)
        a = list(good)
        a[I_K] = 257
        assert f(*a) == ARG
        a[I_K] = 256
        a[I_D] = 32                       # (k = 256 itself is in range: the next check is D's)
        assert f(*a) == UNSUPPORTED
        for D in (32, 96, 256):
            a = list(good)
            a[I_D] = D
            assert f(*a) == UNSUPPORTED, D
    for bad in (0, -1):                   # a pool with no entries
        a = list(by_id)
        a[I_NPOOL] = bad
        assert f(*a) == ARG
    for bad in (2, -1):
        a = list(by_id)
        a[I_METRIC] = bad
        assert f(*a) == ARG
    del keep


def test_the_target_workgroup_count_is_clamped_and_restored():
    f = _lib.lib().raw("amid_neighbors_target_workgroups")
    assert f(0) == 256 and f(3) == 256 and f(1000) == 3 and f(-5) == 256 and f(0) == 256


def test_the_workspace_size():
    w = _lib.lib().raw("amid_neighbors_workspace_bytes")
    assert w(4, 16, 128, 5) > 0 and w(4, 16, 64, 5) > 0
    for bad in ((0, 16, 128, 5), (-1, 16, 128, 5), (4, 0, 128, 5), (4, -1, 128, 5), (4, 16, 128, 0), (4, 16, 128, -1), (4, 16, 128, 257),
                (4, 16, 32, 5), (4, 16, 96, 5), (4, 16, 256, 5), (4, 1 << 31, 128, 5)):
        assert w(*bad) < 0, bad
    Qs = [1, 15, 16, 17, 33, 63, 64, 65, 127, 128, 129, 256, 257, 1000, 4096, 4097]
    Ns = [1, 127, 128, 129, 255, 256, 257, 700, 16384, 16385, 894820, 10_000_000]
    Ks = [1, 2, 10, 63, 64, 65, 100, 255, 256]
    for D in (64, 128):
        for n in Ns:
            for k in Ks:
                sizes = [w(Q, n, D, k) for Q in Qs]
                assert all(s > 0 for s in sizes) and sizes == sorted(sizes), ("Q", n, k)
        for Q in Qs:
            for k in Ks:
                sizes = [w(Q, n, D, k) for n in Ns]
                assert sizes == sorted(sizes), ("n_cand", Q, k)
            for n in Ns:
                sizes = [w(Q, n, D, k) for k in Ks]
                assert sizes == sorted(sizes), ("k", Q, n)
        # dense sweeps where the workgroup and range counts step
        for k in (10, 65):
            sizes = [w(Q, 894820, D, k) for Q in range(1, 400)]
            assert sizes == sorted(sizes)
            sizes = [w(256, n, D, k) for n in range(1, 3000)]
            assert sizes == sorted(sizes)
        sizes = [w(100, 5000, D, k) for k in range(1, 257)]
        assert sizes == sorted(sizes)
