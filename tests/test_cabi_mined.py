"""CPU-side checks of the hard-negative step's surface: amid_scorer_mined_fwd_bwd_f32 (csrc/head_mined.hip) is declared in
include/amid_hip.h, bound by _lib and exported by the built library; its argument checks answer with stream = None and host buffers, before
anything touches a device; train_sr.py parses --hard_negs / --hard_skip, checks them, keeps them as resume keys, and train_sr_dr.py
refuses them; the engines' and the models' constructors refuse what DESIGN.md section 18 lists."""
import ctypes
import subprocess

import pytest

from amid_amd import _lib

ENTRY = "amid_scorer_mined_fwd_bwd_f32"
ARG, UNSUPPORTED = -1, -2
NAMES = ["u", "items", "w1", "b1", "w2", "b2", "domain_id", "kind", "keep", "skip", "B", "NI", "D", "hid", "p1", "p2", "dz1", "dz2", "loss_part",
         "du", "ditems", "sc_part", "sel", "z", "tr_src", "tr_dst", "n_tr", "stream"]


def test_entry_point_is_declared_bound_and_exported():
    assert ENTRY in _lib.parse_header()
    assert ENTRY in _lib.declared_symbols()
    assert _lib.lib().raw(ENTRY) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == ENTRY and " T " in ln for ln in out.splitlines())


def test_parameter_names_are_the_header_s():
    ret, types, names = _lib.parse_header()[ENTRY]
    assert names == NAMES and ret is ctypes.c_int
    assert [types[NAMES.index(n)] for n in ("kind", "keep", "skip", "B", "NI", "D", "hid", "n_tr")] == [ctypes.c_int] * 8
    assert types[NAMES.index("sel")] is ctypes.c_void_p and types[NAMES.index("z")] is ctypes.c_void_p
    # the listwise entry's names plus the four new ones: one table of the step's pointers serves both
    assert set(NAMES) - set(_lib.parse_header()["amid_scorer_listwise_fwd_bwd_f32"][2]) == {"keep", "skip", "sel", "z"}
    with pytest.raises(TypeError):
        _lib.lib().call_named(ENTRY, u=None)
    with pytest.raises(TypeError):
        _lib.lib().call_named(ENTRY, dict.fromkeys(NAMES), labels=None)
    with pytest.raises(TypeError):          # the listwise launch's table alone: keep / skip / sel / z are missing
        _lib.lib().call_named(ENTRY, dict.fromkeys(n for n in NAMES if n not in ("keep", "skip", "sel", "z")))


def _good():
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = {n: p for n in NAMES}
    good.update(kind=1, keep=2, skip=1, B=2, NI=5, D=64, hid=16, n_tr=0, tr_src=None, tr_dst=None, stream=None)
    return buf, good


def _call(good, **change):
    a = dict(good, **change)
    return _lib.lib().raw(ENTRY)(*[a[n] for n in NAMES])


def test_bad_arguments_are_refused_without_a_gpu():
    keep, good = _good()
    for n in ("u", "items", "w1", "b1", "w2", "b2", "domain_id", "p1", "p2", "dz1", "dz2", "loss_part", "du", "ditems", "sc_part", "sel", "z"):
        assert _call(good, **{n: None}) == ARG, n
    for ch in (dict(keep=0), dict(keep=-1), dict(skip=-1), dict(keep=5, skip=0), dict(keep=4, skip=1), dict(keep=1, skip=4), dict(keep=2, skip=3),
               dict(keep=2 ** 31 - 1, skip=2 ** 31 - 1), dict(NI=2, keep=2, skip=0), dict(NI=2, keep=1, skip=1),
               dict(keep=0, NI=1025), dict(keep=3, skip=2, D=160)):          # (ARG goes before UNSUPPORTED)
        assert _call(good, **ch) == ARG, ch
    # the listwise entry's refusals
    for ch in (dict(kind=0), dict(kind=3), dict(kind=-1), dict(NI=1), dict(NI=0), dict(NI=-5), dict(B=0), dict(D=0), dict(n_tr=-1), dict(n_tr=33),
               dict(n_tr=1), dict(NI=1, D=256), dict(kind=0, NI=2000)):
        assert _call(good, **ch) == ARG, ch
    for ch in (dict(NI=1025), dict(NI=2 ** 20), dict(D=160), dict(D=256), dict(D=48), dict(D=100), dict(hid=0), dict(hid=-4), dict(hid=68), dict(hid=6),
               dict(hid=65), dict(NI=1025, keep=1024, skip=0)):
        assert _call(good, **ch) == UNSUPPORTED, ch
    del keep


def test_train_sr_parses_the_flags_and_train_sr_dr_refuses_them():
    from amid_amd import train_sr, train_sr_dr
    args = train_sr.build_parser().parse_args(["--train_negs", "6", "--loss", "softmax", "--hard_negs", "2", "--hard_skip", "1"])
    assert args.hard_negs == 2 and args.hard_skip == 1
    train_sr.check_train_loss(args)
    train_sr.check_train_loss(train_sr.build_parser().parse_args(["--train_negs", "3", "--loss", "bpr", "--hard_negs", "2", "--hard_skip", "1"]))
    d = train_sr.build_parser().parse_args([])
    assert d.hard_negs == 0 and d.hard_skip == 0
    train_sr.check_train_loss(d)
    assert {"hard_negs", "hard_skip"} <= set(train_sr.RESUME_KEYS)
    assert train_sr._RESUME_DEFAULTS["hard_negs"] == 0 and train_sr._RESUME_DEFAULTS["hard_skip"] == 0
    for bad in (["--hard_negs", "1"],                                                          # the BCE
                ["--loss", "bce", "--train_negs", "4", "--hard_negs", "2"],
                ["--loss", "softmax", "--train_negs", "4", "--hard_negs", "-1"],
                ["--loss", "softmax", "--train_negs", "4", "--hard_negs", "2", "--hard_skip", "-1"],
                ["--loss", "softmax", "--train_negs", "4", "--hard_skip", "1"],                 # a skip without a list
                ["--loss", "softmax", "--train_negs", "4", "--hard_negs", "5"],
                ["--loss", "bpr", "--train_negs", "4", "--hard_negs", "3", "--hard_skip", "2"]):
        with pytest.raises(SystemExit):
            train_sr.check_train_loss(train_sr.build_parser().parse_args(bad))
    with pytest.raises(SystemExit, match="doubly-robust"):
        train_sr_dr.main(["--hard_negs", "2", "--model", "sasrec"])
    with pytest.raises(SystemExit, match="doubly-robust"):
        train_sr_dr.main(["--hard_skip", "1", "--model", "sasrec"])


def test_resume_defaults_in_both_directions(tmp_path):
    import torch
    from amid_amd import train_sr
    args = train_sr.build_parser().parse_args([])
    old = {k: getattr(args, k) for k in train_sr.RESUME_KEYS if k not in ("hard_negs", "hard_skip")}
    path = str(tmp_path / "last.pt")
    torch.save({"extra": {"args": old}}, path)              # a file from before the keys existed: 0 / 0
    args.resume = path
    assert train_sr.read_resume(args) is not None
    for flag, val in (("hard_negs", 2), ("hard_skip", 1)):
        a = train_sr.build_parser().parse_args([])
        a.resume = path
        setattr(a, flag, val)
        with pytest.raises(SystemExit, match="--" + flag):
            train_sr.read_resume(a)
    # a file written WITH mining against a command line without, and with the same flags
    new = dict(old, loss="softmax", train_negs=6, hard_negs=2, hard_skip=1)
    torch.save({"extra": {"args": new}}, path)
    a = train_sr.build_parser().parse_args(["--loss", "softmax", "--train_negs", "6"])
    a.resume = path
    with pytest.raises(SystemExit, match="--hard_negs"):
        train_sr.read_resume(a)
    a = train_sr.build_parser().parse_args(["--loss", "softmax", "--train_negs", "6", "--hard_negs", "2", "--hard_skip", "1"])
    a.resume = path
    assert train_sr.read_resume(a) is not None


ENGINE_REFUSALS = [dict(loss="bce", hard_negs=2), dict(hard_negs=2), dict(loss="softmax", hard_negs=-1), dict(loss="softmax", hard_skip=-1),
                   dict(loss="bpr", hard_skip=1), dict(loss="softmax", hard_negs=2, dr=True), dict(loss="softmax", hard_negs=2, compute="bf16"),
                   dict(loss="bpr", hard_negs=2, inc_bs=4)]


@pytest.mark.parametrize("kw", ENGINE_REFUSALS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_engine_constructors_refuse(kw):
    """ValueError before the library or a device is touched."""
    from amid_amd.engine import SasrecEngine
    from amid_amd.engine_bert import Bert4recEngine
    from amid_amd.engine_gru import Gru4recEngine
    for cls in (SasrecEngine, Bert4recEngine, Gru4recEngine):
        k = dict(kw)
        if cls is Bert4recEngine and "inc_bs" in k:
            k.update(comp="inc", comp_bs=k.pop("inc_bs"))
        with pytest.raises(ValueError):
            cls(100, 64, 8, 16, device="cuda:0", **k)
    with pytest.raises(ValueError):
        Gru4recEngine(100, 64, 8, 16, device="cuda:0", loss="softmax", hard_negs=2, itc_bs=4)


def test_model_constructors_refuse():
    from amid_amd.model_gru import GRU4Rec
    from amid_amd.model_seq import BERT4Rec, SASRec
    base = dict(user_length=10, user_emb_dim=64, item_length=100, item_emb_dim=64, seq_len=8, hid_dim=16, bs=4, isInC=False, isItC=False,
                threshold1=0.5, threshold2=0.5, device="cuda:0")
    for cls in (SASRec, BERT4Rec, GRU4Rec):
        for kw in (dict(hard_negs=2), dict(loss="bce", hard_negs=2), dict(loss="softmax", hard_negs=-1), dict(loss="softmax", hard_skip=1),
                   dict(loss="bpr", hard_negs=1, hard_skip=-2)):
            with pytest.raises(ValueError, match="hard_"):
                cls(**base, **kw)
    with pytest.raises(ValueError):
        SASRec(**dict(base, isInC=True), loss="softmax", hard_negs=2)
    with pytest.raises(ValueError):
        SASRec(**base, isDR=True, loss="softmax", hard_negs=2)
    with pytest.raises(ValueError):
        SASRec(**base, compute="bf16", loss="softmax", hard_negs=2)
