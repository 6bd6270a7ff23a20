"""The parts of save / resume that need no GPU: the loaders' state (DeviceBatches / JointBatches.state_dict) and the command line's
--save_dir / --save_every / --resume, refused before any GPU work where they cannot apply."""
import importlib
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _loader(seed):
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    ds = DualDomainSeqDataset.from_tokenised(os.path.join(GOLDEN, "tok_cloth_sport_train75.npz"))
    return DeviceBatches(ds, 8, shuffle=True, device="cpu", seed=seed, negatives="fixture")


def test_loader_state_gives_the_same_next_epoch():
    a = _loader(3)
    a.epoch_tensors()
    st = a.state_dict()
    want = a.epoch_tensors()
    b = _loader(99)                      # another seed: only the state makes its order a's
    assert not torch.equal(b.epoch_tensors()["i_node"], want["i_node"])
    b = _loader(99)
    b.load_state_dict(st)
    got = b.epoch_tensors()
    assert b.epoch == a.epoch == 2
    assert want.keys() == got.keys()
    for k in want:
        assert torch.equal(want[k], got[k]), k


def test_joint_loader_state_covers_both_loaders():
    from amid_amd.dataset_seq import JointBatches
    a = JointBatches(_loader(3), _loader(4))
    a.epoch_tensors()
    st = a.state_dict()
    want = a.epoch_tensors()
    b = JointBatches(_loader(5), _loader(6))
    b.load_state_dict(st)
    got = b.epoch_tensors()
    for k in want:
        assert torch.equal(want[k], got[k]), k


@pytest.mark.parametrize("mod", ["train_sr", "train_sr_dr"])
def test_parser_accepts_the_checkpoint_flags(mod):
    m = importlib.import_module(f"amid_amd.{mod}")
    a = m.build_parser().parse_args(["--save_dir", "ck", "--save_every", "3", "--resume", "ck/seed0/last.pt"])
    assert (a.save_dir, a.save_every, a.resume) == ("ck", 3, "ck/seed0/last.pt")
    d = m.build_parser().parse_args([])
    assert (d.save_dir, d.save_every, d.resume) == (None, 0, None)


def _no_gpu(monkeypatch, mod):
    def touched(*a, **k):
        raise AssertionError("the GPU or the data was touched before the refusal")
    monkeypatch.setattr(torch.cuda, "_lazy_init", touched)
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(mod, "DualDomainSeqDataset", touched)


ARGS = ["--model", "sasrec", "--emb_dim", "64", "--seq_len", "20", "--hid_dim", "16", "--bs", "32", "-ds", "amazon", "-dm", "toy",
        "--overlap_ratio", "0.75"]


@pytest.mark.parametrize("mod", ["train_sr", "train_sr_dr"])
def test_resume_with_another_emb_dim_exits_before_the_gpu(tmp_path, monkeypatch, mod):
    m = importlib.import_module(f"amid_amd.{mod}")
    keys = getattr(m, "RESUME_KEYS")
    from amid_amd.train_sr import read_resume, run_signature
    path = str(tmp_path / "last.pt")
    torch.save({"format": 1, "engine": {}, "extra": {"seed": 0, "epoch": 0, "args": run_signature(m.build_parser().parse_args(ARGS), keys)}},
               path)
    assert read_resume(m.build_parser().parse_args(ARGS + ["--resume", path]), keys) is not None      # the matching command line passes
    _no_gpu(monkeypatch, m)
    other = [("128" if a == "64" else a) for a in ARGS]
    with pytest.raises(SystemExit, match="--emb_dim is 128 here but 64 in the file"):
        m.main(other + ["--resume", path, "--data_root", str(tmp_path)])


@pytest.mark.parametrize("mod", ["train_sr", "train_sr_dr"])
def test_checkpoint_flags_refused_under_data_parallel(tmp_path, monkeypatch, mod):
    m = importlib.import_module(f"amid_amd.{mod}")
    _no_gpu(monkeypatch, m)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single-GPU"):
        m.main(ARGS + ["--save_dir", str(tmp_path / "ck"), "--data_root", str(tmp_path)])
