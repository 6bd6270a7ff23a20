"""CPU-side checks of the dataset-wide top-K (csrc/own_sets.hip amid_own_from_seq_i64, csrc/full_rank.hip amid_topk_items_f32 /
amid_topk_users_f32, amid_amd/recommend.py): declared, exported, uniquely named parameters, bad arguments refused before anything touches
a device, and the command line's host-side pieces."""
import os
import subprocess

import numpy as np
import pytest

from amid_amd import _lib

NEW = ("amid_own_from_seq_i64", "amid_topk_items_f32", "amid_topk_users_f32")
P = 0x1000          # a dummy non-null host address (never dereferenced: the checks fail first)


def test_prototypes_are_declared_exported_and_name_their_parameters_uniquely():
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
        _, argtypes, names = protos[name]
        assert len(names) == len(argtypes) and len(set(names)) == len(names), name
        assert names[-1] == "stream"
    # the users half takes amid_topk_f32's arguments, name for name
    assert protos["amid_topk_users_f32"][2] == protos["amid_topk_f32"][2]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [n for n in NEW if n not in exported]


def _own_args(**over):
    a = dict(seq_d1=P, seq_d2=P, domain_id=P, B=4, T=20, cnt=P, own=P, own_off=P, stream=None)
    a.update(over)
    return list(a.values())


def _items_args(**over):
    a = dict(B=4, pool_d1=P, n1=10, pool_d2=P, n2=10, table=P, n_rows=100, w1=P, D=128, hid=32, ws=P, flags=P, stream=None)
    a.update(over)
    return list(a.values())


def _users_args(**over):
    a = dict(u=P, u_dom_stride=0, domain=P, B=4, pool_d1=P, n1=10, pool_d2=P, n2=10, own=None, own_off=None, rows=None, table=P, n_rows=100,
             w1=P, b1=P, w2=P, b2=P, D=128, hid=32, k=10, exclude=1, ws=P, flags=P, ids=P, scores=P, stream=None)
    a.update(over)
    return list(a.values())


def test_own_sets_refuse_bad_arguments_without_a_gpu():
    f = _lib.lib().raw("amid_own_from_seq_i64")
    for name in ("seq_d1", "seq_d2", "domain_id", "cnt", "own", "own_off"):
        assert f(*_own_args(**{name: None})) == -1, name
    assert f(*_own_args(B=0)) == -1 and f(*_own_args(B=-3)) == -1
    assert f(*_own_args(T=0)) == -1 and f(*_own_args(T=-1)) == -1
    assert f(*_own_args(B=1 << 20, T=2048)) == -1            # B * T does not fit own_off's int32
    assert f(*_own_args(T=2049)) == -2                        # a row's ids no longer fit the sort's LDS


def test_topk_items_refuse_bad_arguments_without_a_gpu():
    f = _lib.lib().raw("amid_topk_items_f32")
    for name in ("pool_d1", "pool_d2", "table", "w1", "ws", "flags"):
        assert f(*_items_args(**{name: None})) == -1, name
    assert f(*_items_args(B=0)) == -1
    assert f(*_items_args(n1=0)) == -1 and f(*_items_args(n2=0)) == -1
    assert f(*_items_args(n_rows=0)) == -1
    assert f(*_items_args(D=96)) == -2 and f(*_items_args(D=256)) == -2
    assert f(*_items_args(hid=24)) == -2 and f(*_items_args(hid=8)) == -2


def test_topk_users_refuse_bad_arguments_without_a_gpu():
    f = _lib.lib().raw("amid_topk_users_f32")
    for name in ("u", "domain", "pool_d1", "pool_d2", "table", "w1", "b1", "w2", "b2", "ws", "flags", "ids", "scores"):
        assert f(*_users_args(**{name: None})) == -1, name
    assert f(*_users_args(k=0)) == -1 and f(*_users_args(k=257)) == -1
    assert f(*_users_args(B=0)) == -1
    assert f(*_users_args(own=P)) == -1                       # an own list without its offsets / row ids
    assert f(*_users_args(D=96)) == -2 and f(*_users_args(hid=8)) == -2


def test_the_parser_refuses_joint_jobs(tmp_path):
    from amid_amd.recommend import main
    with pytest.raises(SystemExit, match="-dm a\\+b"):
        main(["--data_root", str(tmp_path), "-dm", "a+b", "--weights", str(tmp_path / "none.pt")])


def test_history_full_shifts_the_own_domain_sequence():
    from amid_amd.recommend import filled_batches, full_history
    pad = 99
    s1 = np.array([[pad, pad, 5, 6], [1, 2, 3, 4], [pad, pad, pad, pad]], dtype=np.int64)
    s2 = np.array([[pad, 7, 8, 9], [pad, pad, pad, 11], [12, 13, 14, 15]], dtype=np.int64)
    pos = np.array([20, 21, 22], dtype=np.int64)
    dom = np.array([0, 1, 1], dtype=np.int64)
    f1, f2 = full_history(s1, s2, pos, dom)
    assert f1.tolist() == [[pad, 5, 6, 20], [1, 2, 3, 4], [pad, pad, pad, pad]]          # row 0: its own domain is d1
    assert f2.tolist() == [[pad, 7, 8, 9], [pad, pad, 11, 21], [13, 14, 15, 22]]          # rows 1, 2: d2; a full row drops its oldest id
    assert s1[0].tolist() == [pad, pad, 5, 6] and s2[2].tolist() == [12, 13, 14, 15]      # the inputs are not written
    # a single-token sequence is replaced by the held-out item
    g1, _ = full_history(np.array([[3]]), np.array([[4]]), np.array([8]), np.array([0]))
    assert g1.tolist() == [[8]]
    # the tail batch is filled from the start of the CSV
    assert filled_batches(80, 32).tolist() == [list(range(32)), list(range(32, 64)), list(range(64, 80)) + list(range(16))]
    assert filled_batches(3, 8).tolist() == [[0, 1, 2, 0, 1, 2, 0, 1]]
    assert filled_batches(64, 32).shape == (2, 32)
