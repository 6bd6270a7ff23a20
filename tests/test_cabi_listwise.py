"""CPU-side checks of the listwise train step's surface: amid_scorer_listwise_fwd_bwd_f32 (csrc/head_listwise.hip) is declared in
include/amid_hip.h, bound by _lib and exported by the built library; its argument checks answer with stream = None and host buffers,
before anything touches a device; train_sr.py parses --train_negs / --loss and train_sr_dr.py refuses them; DeviceBatches takes
train_negs in the fixture mode."""
import ctypes
import os
import subprocess

import pytest

from amid_amd import _lib

ENTRY = "amid_scorer_listwise_fwd_bwd_f32"
ARG, UNSUPPORTED = -1, -2
NAMES = ["u", "items", "w1", "b1", "w2", "b2", "domain_id", "kind", "B", "NI", "D", "hid", "p1", "p2", "dz1", "dz2", "loss_part", "du", "ditems",
         "sc_part", "tr_src", "tr_dst", "n_tr", "stream"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_entry_point_is_declared_bound_and_exported():
    assert ENTRY in _lib.parse_header()
    assert ENTRY in _lib.declared_symbols()
    assert _lib.lib().raw(ENTRY) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert any(ln.split()[-1] == ENTRY and " T " in ln for ln in out.splitlines())


def test_parameter_names_are_the_header_s():
    ret, types, names = _lib.parse_header()[ENTRY]
    assert names == NAMES and ret is ctypes.c_int
    assert [types[NAMES.index(n)] for n in ("kind", "B", "NI", "D", "hid", "n_tr")] == [ctypes.c_int] * 6
    # bound by name: a missing or an unknown name is a TypeError before any launch
    with pytest.raises(TypeError):
        _lib.lib().call_named(ENTRY, u=None)
    with pytest.raises(TypeError):
        _lib.lib().call_named(ENTRY, dict.fromkeys(NAMES), labels=None)


def _good():
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = {n: p for n in NAMES}
    good.update(kind=1, B=2, NI=5, D=64, hid=16, n_tr=0, tr_src=None, tr_dst=None, stream=None)
    return buf, good


def _call(good, **change):
    a = dict(good, **change)
    return _lib.lib().raw(ENTRY)(*[a[n] for n in NAMES])


def test_bad_arguments_are_refused_without_a_gpu():
    keep, good = _good()
    for n in ("u", "items", "w1", "b1", "w2", "b2", "domain_id", "p1", "p2", "dz1", "dz2", "loss_part", "du", "ditems", "sc_part"):
        assert _call(good, **{n: None}) == ARG, n
    for ch in (dict(kind=0), dict(kind=3), dict(kind=-1), dict(NI=1), dict(NI=0), dict(NI=-5), dict(B=0), dict(D=0), dict(n_tr=-1), dict(n_tr=33),
               dict(n_tr=1), dict(NI=1, D=256), dict(kind=0, NI=2000)):      # (n_tr 1 with null lists; ARG goes before UNSUPPORTED)
        assert _call(good, **ch) == ARG, ch
    for ch in (dict(NI=1025), dict(NI=2 ** 20), dict(D=160), dict(D=256), dict(D=48), dict(D=100), dict(hid=0), dict(hid=-4), dict(hid=68), dict(hid=6),
               dict(hid=65)):
        assert _call(good, **ch) == UNSUPPORTED, ch
    del keep


def test_train_sr_parses_the_flags_and_train_sr_dr_refuses_them():
    from amid_amd import train_sr, train_sr_dr
    args = train_sr.build_parser().parse_args(["--train_negs", "4", "--loss", "softmax"])
    assert args.train_negs == 4 and args.loss == "softmax"
    train_sr.check_train_loss(args)
    d = train_sr.build_parser().parse_args([])
    assert d.train_negs == 1 and d.loss == "bce"
    assert {"train_negs", "loss"} <= set(train_sr.RESUME_KEYS) and train_sr._RESUME_DEFAULTS["loss"] == "bce" and train_sr._RESUME_DEFAULTS["train_negs"] == 1
    for bad in (["--train_negs", "0"], ["--train_negs", "1024"], ["--loss", "softmax", "--dtype", "bf16"]):
        with pytest.raises(SystemExit):
            train_sr.check_train_loss(train_sr.build_parser().parse_args(bad))
    with pytest.raises(SystemExit):
        train_sr.build_parser().parse_args(["--loss", "hinge"])
    with pytest.raises(SystemExit, match="doubly-robust"):
        train_sr_dr.main(["--loss", "softmax", "--model", "sasrec"])
    with pytest.raises(SystemExit, match="doubly-robust"):
        train_sr_dr.main(["--train_negs", "4", "--model", "sasrec"])


def test_a_last_pt_without_the_keys_means_the_defaults(tmp_path):
    import torch
    from amid_amd import train_sr
    args = train_sr.build_parser().parse_args([])
    old = {k: getattr(args, k) for k in train_sr.RESUME_KEYS if k not in ("train_negs", "loss")}
    path = str(tmp_path / "last.pt")
    torch.save({"extra": {"args": old}}, path)
    args.resume = path
    assert train_sr.read_resume(args) is not None
    for flag, val in (("loss", "softmax"), ("train_negs", 4)):
        a = train_sr.build_parser().parse_args([])
        a.resume = path
        setattr(a, flag, val)
        with pytest.raises(SystemExit, match="--" + flag):
            train_sr.read_resume(a)


def test_device_batches_takes_train_negs_in_the_fixture_mode():
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    ds = DualDomainSeqDataset.from_tokenised(os.path.join(GOLDEN, "tok_cloth_sport_train75.npz"))
    bs = 8
    assert ds.isTrain
    if ds.ref_neg.shape[1] >= 3:
        b = next(iter(DeviceBatches(ds, bs, shuffle=False, device="cpu", seed=0, negatives="fixture", train_negs=3)))
        assert tuple(b["neg_samples"].shape) == (bs, 3) and tuple(b["label"].shape) == (bs, 4)
        assert bool((b["label"][:, 0] == 1).all()) and bool((b["label"][:, 1:] == 0).all())
    else:
        with pytest.raises(ValueError, match="enough stored negatives"):
            DeviceBatches(ds, bs, shuffle=False, device="cpu", seed=0, negatives="fixture", train_negs=3)
    one = next(iter(DeviceBatches(ds, bs, shuffle=False, device="cpu", seed=0, negatives="fixture")))
    assert tuple(one["neg_samples"].reshape(bs, -1).shape) == (bs, 1)
    for bad in (0, 1024, 2.0):
        with pytest.raises(ValueError, match="train_negs"):
            DeviceBatches(ds, bs, shuffle=False, device="cpu", seed=0, negatives="fixture", train_negs=bad)
