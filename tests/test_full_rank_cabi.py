"""CPU-side checks of the full-catalog evaluation / top-K entry points (csrc/full_rank.hip): declared, exported, and refusing bad arguments
before anything touches a device."""
import os
import subprocess

from amid_amd import _lib

NEW = ("amid_full_rank_workspace_bytes", "amid_full_rank_f32", "amid_topk_f32")


def test_full_rank_prototypes_are_declared_and_exported():
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [n for n in NEW if n not in exported]


def _rank_args(**over):
    """amid_full_rank_f32's arguments, every pointer a dummy non-null host address (never dereferenced: the checks fail first)."""
    p = 0x1000
    a = dict(u=p, u_dom_stride=0, pos=p, domain=p, B=4, pool_d1=p, n1=10, pool_d2=p, n2=10, own=None, own_off=None, rows=None, table=p,
             n_rows=100, w1=p, b1=p, w2=p, b2=p, D=128, hid=32, fix=1e-7, ws=p, flags=p, rank=p, rank_raw=p, scores=None, n_cols=0, stream=None)
    a.update(over)
    return list(a.values())


def _topk_args(**over):
    p = 0x1000
    a = dict(u=p, u_dom_stride=0, domain=p, B=4, pool_d1=p, n1=10, pool_d2=p, n2=10, own=None, own_off=None, rows=None, table=p, n_rows=100,
             w1=p, b1=p, w2=p, b2=p, D=128, hid=32, k=10, exclude=1, ws=p, flags=p, ids=p, scores=p, stream=None)
    a.update(over)
    return list(a.values())


def test_full_rank_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    f = L.raw("amid_full_rank_f32")
    assert f(*_rank_args(u=None)) == -1
    assert f(*_rank_args(pos=None)) == -1
    assert f(*_rank_args(table=None)) == -1
    assert f(*_rank_args(ws=None)) == -1
    assert f(*_rank_args(flags=None)) == -1
    assert f(*_rank_args(B=0)) == -1
    assert f(*_rank_args(n1=0)) == -1
    assert f(*_rank_args(own=0x1000)) == -1                  # an own list without its offsets / row ids
    assert f(*_rank_args(scores=0x1000, n_cols=5)) == -1     # fewer score columns than candidates
    assert f(*_rank_args(D=96)) == -2                         # shapes outside D 64 / 128, hid 16 / 32 / 64
    assert f(*_rank_args(hid=24)) == -2


def test_topk_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    f = L.raw("amid_topk_f32")
    assert f(*_topk_args(k=0)) == -1
    assert f(*_topk_args(k=257)) == -1
    assert f(*_topk_args(ids=None)) == -1
    assert f(*_topk_args(scores=None)) == -1
    assert f(*_topk_args(domain=None)) == -1
    assert f(*_topk_args(own=0x1000)) == -1
    assert f(*_topk_args(D=256)) == -2
    assert f(*_topk_args(hid=8)) == -2


def test_full_rank_workspace_query():
    L = _lib.lib()
    q = lambda *a: L.value("amid_full_rank_workspace_bytes", *a)      # noqa: E731
    assert q(0, 10, 10, 32, 0) == -1 and q(4, 10, 10, 32, 257) == -1
    rank = q(256, 1000, 2000, 32, 0)
    assert rank >= 256 * 32 * 4 + 256 * 2 * 4
    topk = q(256, 1000, 2000, 32, 10)
    assert topk >= rank + 3000 * 32 * 4                      # + the candidates' item halves
