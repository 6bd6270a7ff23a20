"""CPU-side checks of the list-ranking entry points (csrc/rank_lists.hip): declared in include/amid_hip.h, bound by _lib, exported by the built
library; their argument checks answer with stream = None and host buffers, before anything touches a device; the workspace size is negative
for bad sizes and does not fall when B, n_cand or k grows; and recommend.py's candidate_lists reads the two file forms alike."""
import ctypes
import subprocess

import numpy as np
import pytest

from amid_amd import _lib

NEW = ["amid_rank_lists_workspace_bytes", "amid_rank_lists_target_workgroups", "amid_rank_lists_f32"]
ARG, UNSUPPORTED = -1, -2
RANK = ["u", "u_dom_stride", "domain_id", "B", "cand", "cand_off", "n_cand", "own_items", "own_off", "rows", "table", "n_rows", "w1", "b1", "w2",
        "b2", "D", "hid", "k", "workspace", "flags", "list_scores", "ids", "scores", "positions", "stream"]
TILE = 256                  # RL_TILE: candidates per tile
UNITS = 2048                # RL_UNITS: the default (and largest) target of amid_rank_lists_target_workgroups


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_bound_and_exported(name):
    assert name in _lib.parse_header()
    assert name in _lib.declared_symbols()
    assert _lib.lib().raw(name) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())


def test_header_and_library_export_the_same_rank_lists_set():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("amid_rank_lists_")}
    assert exported == set(NEW) == {n for n in _lib.declared_symbols() if n.startswith("amid_rank_lists_")}


def test_parameter_names_are_the_header_s():
    protos = _lib.parse_header()
    assert protos["amid_rank_lists_f32"][2] == RANK
    assert protos["amid_rank_lists_workspace_bytes"][2] == ["B", "n_cand", "hid", "k"]
    assert protos["amid_rank_lists_target_workgroups"][2] == ["wgs"]


def _good():
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(u=p, u_dom_stride=0, domain_id=p, B=4, cand=p, cand_off=p, n_cand=20, own_items=p, own_off=p, rows=p, table=p, n_rows=16, w1=p,
                b1=p, w2=p, b2=p, D=128, hid=32, k=5, workspace=p, flags=p, list_scores=p, ids=p, scores=p, positions=p, stream=None)
    return buf, good


def _call(good, **change):
    a = dict(good, **change)
    return _lib.lib().raw("amid_rank_lists_f32")(*[a[n] for n in RANK])


def test_null_pointers_are_refused_without_a_gpu():
    keep, good = _good()
    for n in ("u", "domain_id", "cand", "cand_off", "table", "w1", "b1", "w2", "b2", "workspace", "flags", "own_off", "rows"):
        assert _call(good, **{n: None}) == ARG, n
    for n in ("ids", "scores", "positions"):                          # the triple given partly, with and without list_scores
        assert _call(good, **{n: None}) == ARG, n
        assert _call(good, list_scores=None, **{n: None}) == ARG, n
        assert _call(good, **{m: None for m in ("ids", "scores", "positions") if m != n}) == ARG, n
    assert _call(good, list_scores=None, ids=None, scores=None, positions=None) == ARG          # neither output
    assert _call(good, own_items=None, own_off=None, rows=None, D=32) == UNSUPPORTED              # (no history is fine: the next check is D's)
    assert _call(good, list_scores=None, D=32) == UNSUPPORTED and _call(good, ids=None, scores=None, positions=None, D=32) == UNSUPPORTED
    assert _call(good, cand=None, n_cand=0, D=32) == UNSUPPORTED                                  # (no candidates at all need no array)
    del keep


def test_bad_sizes_are_refused_without_a_gpu():
    keep, good = _good()
    for ch in (dict(B=0), dict(B=-1), dict(n_cand=-1), dict(n_cand=2 ** 31 - 1), dict(k=0), dict(k=-1), dict(k=257), dict(n_rows=0),
               dict(n_rows=-1), dict(u_dom_stride=-1)):
        assert _call(good, **ch) == ARG, ch
    for ch in (dict(D=32), dict(D=96), dict(D=256), dict(hid=8), dict(hid=48), dict(hid=128)):
        assert _call(good, **ch) == UNSUPPORTED, ch
    assert _call(good, k=256, D=32) == UNSUPPORTED                    # (k = 256 itself is in range: the next check is D's)
    assert _call(good, n_cand=2 ** 31 - 2, D=32) == UNSUPPORTED and _call(good, n_cand=0, D=32) == UNSUPPORTED
    for k in (0, -1, 257):                                            # without the triple k is not looked at
        assert _call(good, ids=None, scores=None, positions=None, k=k, D=32) == UNSUPPORTED, k
    del keep


def test_the_target_workgroup_count_is_clamped_and_restored():
    f = _lib.lib().raw("amid_rank_lists_target_workgroups")
    assert f(0) == UNITS and f(3) == UNITS and f(50000) == 3 and f(-5) == UNITS and f(0) == UNITS


def test_the_workspace_size():
    w = _lib.lib().raw("amid_rank_lists_workspace_bytes")
    assert w(4, 20, 32, 5) > 0 and w(4, 0, 16, 5) > 0 and w(1, 0, 64, 0) > 0 and w(4, 2 ** 31 - 2, 32, 256) > 0
    for bad in ((0, 20, 32, 5), (-1, 20, 32, 5), (4, -1, 32, 5), (4, 2 ** 31 - 1, 32, 5), (4, 2 ** 40, 32, 5), (4, 20, 32, -1), (4, 20, 32, 257),
                (4, 20, 8, 5), (4, 20, 0, 5), (4, 20, 48, 5), (4, 20, 128, 5)):
        assert w(*bad) < 0, bad
    Bs = [1, 7, 8, 9, 40, 255, 256, 257, 1000, 2047, 2048, 2049, 4096, 10000, 100000]
    Ns = [0, 1, TILE - 1, TILE, TILE + 1, 700, 2100, 256000, 100000 * TILE, 2 ** 31 - 2]
    Ks = [0, 1, 2, 10, 100, 255, 256]
    for hid in (16, 32, 64):
        for n in Ns:
            for k in Ks:
                sizes = [w(B, n, hid, k) for B in Bs]
                assert all(s > 0 for s in sizes) and sizes == sorted(sizes), ("B", n, hid, k)
        for B in Bs:
            for k in Ks:
                sizes = [w(B, n, hid, k) for n in Ns]
                assert sizes == sorted(sizes), ("n_cand", B, hid, k)
            for n in Ns:
                sizes = [w(B, n, hid, k) for k in Ks]
                assert sizes == sorted(sizes), ("k", B, n, hid)
    # dense sweeps across the tile size and across where the number of tiles a unit holds steps (tile bound = UNITS, 2 UNITS, ...)
    for k in (10, 256):
        for B in (1, 40, 300):
            sizes = [w(B, n, 32, k) for n in range(0, 4 * TILE + 2)]
            assert sizes == sorted(sizes), ("tile", B, k)
            for step in (1, 2, 3):
                at = (step * UNITS - B) * TILE
                sizes = [w(B, n, 32, k) for n in range(at - 2 * TILE - 1, at + 2 * TILE + 2)]
                assert sizes == sorted(sizes), ("units", B, k, step)
        for n in (0, 700, UNITS * TILE):
            sizes = [w(B, n, 32, k) for B in range(1, 2 * UNITS + 200, 3)]
            assert sizes == sorted(sizes), ("B dense", n, k)
    sizes = [w(100, 5000, 32, k) for k in range(0, 257)]
    assert sizes == sorted(sizes)
    # the user halves and the unit prefix are in every workspace
    assert w(1000, 0, 32, 0) >= 1000 * 32 * 4 + 1001 * 4


# ---- recommend.py's candidate_lists --------------------------------------------------------------------------------------------------------------
LISTS = [[5, 9, 5], [], [7], [], [1, 2, 3, 4]]


def _files(tmp_path, lists=LISTS, user_id=None):
    off = np.concatenate(([0], np.cumsum([len(li) for li in lists]))).astype(np.int64)
    items = np.array([x for li in lists for x in li], dtype=np.int64)
    extra = {} if user_id is None else {"user_id": user_id}
    np.savez(tmp_path / "c.npz", offsets=off, items=items, **extra)
    seps = (" ", ",", ", ", "\t")
    (tmp_path / "c.txt").write_text("".join(seps[i % 4].join(str(x) for x in li) + "\n" for i, li in enumerate(lists)))
    return off, items


def test_candidate_lists_reads_both_forms_alike(tmp_path):
    from amid_amd.recommend import candidate_lists
    uid = np.arange(10, 15)
    off, items = _files(tmp_path, user_id=uid)
    for name in ("c.npz", "c.txt"):
        got_i, got_o = candidate_lists(str(tmp_path / name), 5, uid)
        assert got_i.dtype == np.int64 and got_o.dtype == np.int64, name
        assert np.array_equal(got_i, items) and np.array_equal(got_o, off), name
    assert off.tolist() == [0, 3, 3, 4, 4, 8]                         # the empty lines are empty lists
    # a last line without its newline, and a file of empty lines only
    (tmp_path / "d.txt").write_text("5 9 5\n\n7\n\n1,2,3,4")
    got_i, got_o = candidate_lists(str(tmp_path / "d.txt"), 5, uid)
    assert np.array_equal(got_i, items) and np.array_equal(got_o, off)
    (tmp_path / "e.txt").write_text("\n\n\n")
    got_i, got_o = candidate_lists(str(tmp_path / "e.txt"), 3, uid[:3])
    assert got_i.size == 0 and got_o.tolist() == [0, 0, 0, 0]


def test_candidate_lists_refuses_files_of_another_csv(tmp_path):
    from amid_amd.recommend import candidate_lists
    uid = np.arange(10, 15)
    _files(tmp_path, user_id=uid)
    for name in ("c.npz", "c.txt"):
        for n in (4, 6):
            with pytest.raises(SystemExit) as e:
                candidate_lists(str(tmp_path / name), n, np.arange(n))
            assert "5 rows" in str(e.value) and f"has {n}" in str(e.value), (name, n)
    with pytest.raises(SystemExit) as e:
        candidate_lists(str(tmp_path / "c.npz"), 5, uid[::-1].copy())
    assert "user_id" in str(e.value)
    np.savez(tmp_path / "bad.npz", offsets=np.array([0, 3, 2, 4, 4, 8]), items=np.arange(8))
    with pytest.raises(SystemExit):
        candidate_lists(str(tmp_path / "bad.npz"), 5, uid)
    np.savez(tmp_path / "short.npz", offsets=np.array([0, 3, 3, 4, 4, 9]), items=np.arange(8))
    with pytest.raises(SystemExit):
        candidate_lists(str(tmp_path / "short.npz"), 5, uid)
    np.savez(tmp_path / "keys.npz", offsets=np.array([0, 1]))
    with pytest.raises(SystemExit):
        candidate_lists(str(tmp_path / "keys.npz"), 1, uid[:1])
