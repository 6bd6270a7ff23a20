"""CPU-side checks of the diversified top-K entry points (csrc/diversify.hip): declared in include/amid_hip.h, bound by _lib, exported by the
built library; their argument checks answer with stream = None and host buffers, before anything touches a device; the workspace size is
negative for bad sizes and does not fall when an argument grows; and recommend.py refuses --diversify / --shortlist where they do not
belong, before it reads or writes a file."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

NEW = ["amid_mmr_workspace_bytes", "amid_mmr_lists_f32"]
ARG, UNSUPPORTED = -1, -2
MMR = ["cand", "cand_off", "rel", "n_cand", "B", "table", "n_rows", "D", "metric", "lambda", "K", "shortlist", "ws", "flags", "out_ids",
       "out_rel", "out_value", "out_max_sim", "out_positions", "stream"]
TILE = 256                  # RL_TILE: entries per tile
UNITS = 2048                # RL_UNITS: the target number of units


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_bound_and_exported(name):
    assert name in _lib.parse_header()
    assert name in _lib.declared_symbols()
    assert _lib.lib().raw(name) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())


def test_header_and_library_export_the_same_mmr_set():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("amid_mmr_")}
    assert exported == set(NEW) == {n for n in _lib.declared_symbols() if n.startswith("amid_mmr_")}


def test_parameter_names_are_the_header_s():
    protos = _lib.parse_header()
    assert protos["amid_mmr_lists_f32"][2] == MMR
    assert protos["amid_mmr_workspace_bytes"][2] == ["B", "n_cand", "D", "K", "shortlist"]
    assert protos["amid_mmr_lists_f32"][1][MMR.index("lambda")] is ctypes.c_float


def _good():
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(cand=p, cand_off=p, rel=p, n_cand=20, B=4, table=p, n_rows=16, D=128, metric=1, K=5, shortlist=16, ws=p, flags=p, out_ids=p,
                out_rel=p, out_value=p, out_max_sim=p, out_positions=p, stream=None)
    good["lambda"] = 0.5
    return buf, good


def _call(good, **change):
    a = dict(good, **change)
    return _lib.lib().raw("amid_mmr_lists_f32")(*[a[n] for n in MMR])


def test_null_pointers_are_refused_without_a_gpu():
    keep, good = _good()
    for n in ("cand", "cand_off", "rel", "table", "ws", "flags", "out_ids"):
        assert _call(good, **{n: None}) == ARG, n
    # the outputs other than out_ids may be null, and no entries at all need neither array: the next check is D's
    for n in ("out_rel", "out_value", "out_max_sim", "out_positions"):
        assert _call(good, D=32, **{n: None}) == UNSUPPORTED, n
    assert _call(good, D=32, out_rel=None, out_value=None, out_max_sim=None, out_positions=None) == UNSUPPORTED
    assert _call(good, D=32, cand=None, rel=None, n_cand=0) == UNSUPPORTED
    del keep


def test_bad_arguments_are_refused_without_a_gpu():
    keep, good = _good()
    for ch in (dict(B=0), dict(B=-1), dict(n_cand=-1), dict(n_cand=2 ** 31 - 1), dict(K=0), dict(K=-1), dict(K=257, shortlist=256),
               dict(K=17), dict(shortlist=4), dict(shortlist=0), dict(shortlist=257), dict(K=257, shortlist=257), dict(n_rows=0),
               dict(n_rows=-1), dict(metric=2), dict(metric=-1)):
        assert _call(good, **ch) == ARG, ch
    for lam in (-0.001, 1.001, float("nan"), float("inf"), float("-inf"), -1.0, 2.0):
        assert _call(good, **{"lambda": lam}) == ARG, lam
    for ch in (dict(D=32), dict(D=96), dict(D=256), dict(D=0)):
        assert _call(good, **ch) == UNSUPPORTED, ch
    # the ends of every range are in range: the next check is D's
    for ch in (dict(K=1, shortlist=1), dict(K=256, shortlist=256), dict(K=16), dict(n_cand=2 ** 31 - 2), dict(n_cand=0), dict(metric=0),
               {"lambda": 0.0}, {"lambda": 1.0}):
        assert _call(good, D=32, **ch) == UNSUPPORTED, ch
    del keep


def test_the_workspace_size():
    w = _lib.lib().raw("amid_mmr_workspace_bytes")
    assert w(4, 20, 128, 5, 16) > 0 and w(4, 0, 64, 5, 5) > 0 and w(1, 0, 64, 1, 1) > 0 and w(4, 2 ** 31 - 2, 128, 256, 256) > 0
    for bad in ((0, 20, 64, 5, 16), (-1, 20, 64, 5, 16), (4, -1, 64, 5, 16), (4, 2 ** 31 - 1, 64, 5, 16), (4, 2 ** 40, 64, 5, 16),
                (4, 20, 64, 0, 16), (4, 20, 64, 257, 16), (4, 20, 64, 5, 0), (4, 20, 64, 5, 257), (4, 20, 32, 5, 16), (4, 20, 0, 5, 16),
                (4, 20, 96, 5, 16), (4, 20, 256, 5, 16)):
        assert w(*bad) < 0, bad
    Bs = [1, 7, 8, 9, 40, 255, 256, 257, 1000, 2047, 2048, 2049, 4096, 10000, 100000]
    Ns = [0, 1, TILE - 1, TILE, TILE + 1, 700, 2100, 256000, 100000 * TILE, 2 ** 31 - 2]
    Ks = [1, 2, 10, 100, 255, 256]
    for n in Ns:
        for k in Ks:
            for m in Ks:
                for D in (64, 128):
                    sizes = [w(B, n, D, k, m) for B in Bs]
                    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), ("B", n, D, k, m)
                assert all(w(B, n, 64, k, m) <= w(B, n, 128, k, m) for B in Bs), ("D", n, k, m)
    for B in Bs:
        for k in Ks:
            for m in Ks:
                sizes = [w(B, n, 64, k, m) for n in Ns]
                assert sizes == sorted(sizes), ("n_cand", B, k, m)
        for n in Ns:
            for fixed in Ks:
                sizes = [w(B, n, 128, k, fixed) for k in Ks]
                assert sizes == sorted(sizes), ("K", B, n, fixed)
                sizes = [w(B, n, 128, fixed, m) for m in Ks]
                assert sizes == sorted(sizes), ("shortlist", B, n, fixed)
    # dense sweeps across the tile size and across where the number of tiles a unit holds steps (tile bound = UNITS, 2 UNITS, ...)
    for m in (10, 256):
        for B in (1, 40, 300):
            sizes = [w(B, n, 64, 10, m) for n in range(0, 4 * TILE + 2)]
            assert sizes == sorted(sizes), ("tile", B, m)
            for step in (1, 2, 3):
                at = (step * UNITS - B) * TILE
                sizes = [w(B, n, 64, 10, m) for n in range(at - 2 * TILE - 1, at + 2 * TILE + 2)]
                assert sizes == sorted(sizes), ("units", B, m, step)
        for n in (0, 700, UNITS * TILE):
            sizes = [w(B, n, 64, 10, m) for B in range(1, 2 * UNITS + 200, 3)]
            assert sizes == sorted(sizes), ("B dense", n, m)
    sizes = [w(100, 5000, 64, k, 256) for k in range(1, 257)] + [w(100, 5000, 128, 256, 256)]
    assert sizes == sorted(sizes)
    sizes = [w(100, 5000, 64, 1, m) for m in range(1, 257)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert w(1000, 0, 64, 1, 1) >= 1001 * 4                            # the unit prefix is in every workspace


# ---- recommend.py's refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_cli_refuses_what_does_not_belong(tmp_path):
    from amid_amd import recommend
    no = tmp_path / "no.npz"
    common = ["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--weights", str(tmp_path / "none.pt"), "--out", str(no)]
    for extra, word in ((["--diversify", "0.5", "--similar_items", "all"], "--similar_items"),
                        (["--diversify", "0.5", "--audience_of", "all"], "--audience_of"),
                        (["--diversify", "0.5", "--topk", "10", "--shortlist", "9"], "--shortlist"),
                        (["--diversify", "0.5", "--topk", "10", "--shortlist", "257"], "--shortlist"),
                        (["--diversify", "0.5", "--topk", "256", "--shortlist", "255"], "--shortlist"),
                        (["--shortlist", "100"], "--diversify"),
                        (["--shortlist", "100", "--candidates", str(tmp_path / "c.npz")], "--diversify"),
                        (["--diversify", "1.5"], "--diversify"),
                        (["--diversify", "-0.1"], "--diversify"),
                        (["--diversify", "nan"], "--diversify")):
        with pytest.raises(SystemExit) as e:
            recommend.main(common + extra)
        assert isinstance(e.value.code, str) and word in e.value.code, extra
    with pytest.raises(SystemExit) as e:                                # a joint job stays refused, as for every other mode
        recommend.main([a if a != "toy" else "toy+toy" for a in common] + ["--diversify", "0.5"])
    assert "joint" in str(e.value.code)
    assert not no.exists() and list(tmp_path.iterdir()) == []
    # what is accepted gets its default: min(256, max(topk, 100))
    for topk, want in ((10, 100), (100, 100), (150, 150), (256, 256)):
        args = recommend.build_parser().parse_args(common + ["--diversify", "0.7", "--topk", str(topk)])
        recommend.check_diversify(args)
        assert args.shortlist == want and args.diversify == 0.7
    args = recommend.build_parser().parse_args(common + ["--diversify", "0", "--topk", "10", "--shortlist", "10"])
    recommend.check_diversify(args)
    assert args.shortlist == 10
