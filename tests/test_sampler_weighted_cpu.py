"""CPU-side checks of the popularity-weighted negative sampler (csrc/sampling.hip: amid_sample_negatives_weighted_i64).  The kernel is
deterministic and tests/test_gpu_sampler_weighted.py holds it integer for integer to tests/sampler_weighted_ref.py; here that restatement
is shown to be successive sampling without replacement in proportion to the weights, the host helpers (item_counts,
popularity_weights) and the command-line checks are exercised, and the C entry point is shown to refuse bad arguments before it
touches a device."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

from amid_amd import _lib
from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset, item_counts, popularity_weights
from tests.sampler_weighted_ref import sample_negatives_weighted_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

POOL = np.arange(100, 140, dtype=np.int64)           # 40 consecutive ids
OWN = POOL[::5].copy()                               # every fifth: 8 own, 32 eligible
ELIGIBLE = np.setdiff1d(POOL, OWN)
COUNTS = 1 + (np.arange(40) % 7) ** 2                # by pool index: 1, 2, 5, 10, 17, 26, 37, 1, ...


def draw(k, seed, epoch, n_rows=1, power=1.0, max_rounds=4096):
    """n_rows rows, all of domain 0 with pool POOL, counts COUNTS and own list OWN."""
    cum = popularity_weights(COUNTS, power)[1]
    own = np.tile(OWN, n_rows)
    off = (np.arange(n_rows + 1) * len(OWN)).astype(np.int32)
    return sample_negatives_weighted_ref(POOL, cum, POOL, cum, own, off, np.zeros(n_rows, dtype=np.int64), k, seed, epoch, max_rounds)


@pytest.fixture(scope="module")
def draws():
    """power -> 4000 draws of row 0 (epochs 1..4000, seed 9, k = 2) -> [4000, 2]."""
    return {p: np.concatenate([draw(2, 9, e, power=p) for e in range(1, 4001)], axis=0) for p in (1.0, 0.5, 0.0)}


def test_every_draw_is_distinct_and_eligible(draws):
    for p, d in draws.items():
        assert d.shape == (4000, 2)
        assert np.isin(d, ELIGIBLE).all(), p
        assert (d[:, 0] != d[:, 1]).all(), p
    big = draw(20, 9, 1)
    assert np.isin(big, ELIGIBLE).all() and len(set(big[0].tolist())) == 20


@pytest.mark.parametrize("power", [1.0, 0.5, 0.0])
def test_successive_sampling_in_proportion_to_the_weights(draws, power):
    """Slot 0 against w_i / W and slot 1 against sum_{i != j} p_i w_j / (W - w_i) over the 32 eligible ids (W their weight sum: the
    rejected own ids only condition the stream): Pearson chi-square, 31 degrees of freedom, against the 1 - 1e-6 quantile.  The seeds
    are fixed, so this is a deterministic statement about the restated rule."""
    from scipy.stats import chi2
    w = popularity_weights(COUNTS, power)[0][np.isin(POOL, ELIGIBLE)].astype(np.float64)
    W = w.sum()
    p0 = w / W
    p1 = np.array([sum(p0[i] * w[j] / (W - w[i]) for i in range(32) if i != j) for j in range(32)])
    assert abs(p1.sum() - 1.0) < 1e-12
    col = np.searchsorted(ELIGIBLE, draws[power])
    bound = float(chi2.isf(1e-6, 31))
    assert 83.5 < bound < 83.7
    stats = []
    for s, p in ((0, p0), (1, p1)):
        exp = 4000.0 * p
        assert exp.min() > 9.0                                  # every expected cell large enough for the chi-square approximation
        got = np.bincount(col[:, s], minlength=32).astype(np.float64)
        stats.append(float(((got - exp) ** 2 / exp).sum()))
    print(f"weighted sampler chi-square, power {power}: slot 0 {stats[0]:.1f}, slot 1 {stats[1]:.1f} (bound {bound:.1f})")
    assert stats[0] < bound and stats[1] < bound
    if power == 1.0:       # and the weights matter: the same counts against the uniform expectation are far outside the bound
        got = np.bincount(col[:, 0], minlength=32).astype(np.float64)
        assert float(((got - 125.0) ** 2 / 125.0).sum()) > 10 * bound


def test_draw_for_k_is_a_prefix_of_the_draw_for_a_larger_k():
    big = draw(32, 5, 7)
    assert np.array_equal(np.sort(big[0]), ELIGIBLE)                # eligible == k: the whole complement
    for k in (1, 2, 8, 31):
        assert np.array_equal(draw(k, 5, 7)[0], big[0, :k])


def test_a_row_does_not_depend_on_its_neighbours():
    a, b, c = draw(8, 5, 3, 1), draw(8, 5, 3, 5), draw(8, 5, 3, 8)
    assert np.array_equal(a, b[:1]) and np.array_equal(b, c[:5])


def test_rows_epochs_seeds_and_powers_draw_differently():
    t = draw(8, 5, 3, 8)
    assert len({tuple(row) for row in t.tolist()}) == 8
    assert not np.array_equal(draw(8, 5, 3), draw(8, 5, 4))
    assert not np.array_equal(draw(8, 5, 3), draw(8, 6, 3))
    assert not np.array_equal(draw(8, 5, 3), draw(8, 5, 3, power=0.0))


def test_exhausted_row_sets_the_sentinel():
    out = draw(33, 9, 1, max_rounds=50)
    assert out[0, 0] == -1 and out[0, 32] == 0
    assert len(set(out[0, 1:32].tolist())) == 31 and np.isin(out[0, 1:32], ELIGIBLE).all()


# ---- item_counts / popularity_weights -----------------------------------------------------------------------------------------

def _toy(tmp_path, name, rows):
    path = tmp_path / name
    path.write_text("user_id,seq_d1,seq_d2,domain_id\n" + "".join(f'{u},"{s1}","{s2}",{d}\n' for u, (s1, s2, d) in enumerate(rows)))
    return DualDomainSeqDataset(seq_len=6, isTrain=True, neg_nums=1, long_length=7, pad_id=1001, csv_path=str(path))


def test_item_counts_on_a_toy_csv(tmp_path):
    ds = _toy(tmp_path, "a.csv", [([1, 2, 2, 3], [50, 51], 0),       # positive 3 held out of seq_d1: counted once, as i_node
                                  ([2, 4, 2], [51, 50, 51], 1),      # positive 51 (domain 1); its repeat leaves seq_d2 with it
                                  ([4], [7], 0),                     # 7 appears in the other domain's column only; the row's seq_d1 is empty
                                  ([3, 3, 1], [52], 0)])             # positive 1; 3 stays twice
    assert ds.pool[0].tolist() == [1, 2, 3, 4] and ds.pool[1].tolist() == [7, 50, 51, 52]
    c1, c2 = item_counts(ds)
    assert c1.dtype == np.int64 and c2.dtype == np.int64
    # d1: 1 -> row 0 seq + row 3 positive; 2 -> 2 (row 0) + 2 (row 1); 3 -> row 0 positive + 2 (row 3); 4 -> row 1 seq + row 2 positive
    assert c1.tolist() == [2, 4, 3, 2]
    # d2: 7 -> row 2 seq; 50 -> rows 0 and 1; 51 -> row 0 seq + row 1 positive (both other 51s dropped with it); 52 -> row 3
    assert c2.tolist() == [1, 2, 2, 1]
    o1, o2 = item_counts(ds, onto=(np.array([4, 9, 1], dtype=np.int64), np.array([60, 51], dtype=np.int64)))
    assert o1.tolist() == [2, 0, 2] and o2.tolist() == [0, 2]
    with pytest.raises(ValueError):
        item_counts(ds, onto=(ds.pool[0],))


def test_item_counts_on_a_tokenised_fixture():
    ds = DualDomainSeqDataset.from_tokenised(os.path.join(GOLDEN, "tok_cloth_sport_train75.npz"))
    c = item_counts(ds)
    for g, seq in enumerate((ds.seq_d1, ds.seq_d2)):
        assert c[g].shape == ds.pool[g].shape and (c[g] >= 0).all()
        n_pos = int(((ds.domain_id != 0) == bool(g)).sum())
        assert int(c[g].sum()) == int((seq != ds.pad_id).sum()) + n_pos       # every token and every positive is a pool id, counted once
        i = int(np.argmax(c[g]))
        want = int((seq == ds.pool[g][i]).sum()) + int((ds.i_node[(ds.domain_id != 0) == bool(g)] == ds.pool[g][i]).sum())
        assert c[g][i] == want
    same = item_counts(ds, onto=ds.pool)
    assert np.array_equal(same[0], c[0]) and np.array_equal(same[1], c[1])


def test_popularity_weights():
    counts = np.array([0, 1, 2, 3, 129, 129, 271], dtype=np.int64)
    for power in (1.0, 0.75, 0.5):
        w, cum = popularity_weights(counts, power)
        assert w.dtype == np.int64 and cum.dtype == np.int64
        assert w[0] == 1 and (np.diff(w[[0, 1, 2, 3, 4, 6]]) > 0).all() and w[4] == w[5]
        assert np.array_equal(cum, np.cumsum(w))
    assert popularity_weights(counts, 1.0)[0].tolist() == [1] + [c * 65536 + 1 for c in counts[1:].tolist()]
    assert popularity_weights(counts, 0.0)[0].tolist() == [65537] * 7
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="power"):
            popularity_weights(counts, bad)
    top = 2 ** 44                                                   # floor(2^44 * 65536) + 1 = 2^60 + 1
    assert int(popularity_weights(np.array([top, top, top, 2 ** 44 - 1]), 1.0)[1][-1]) == 2 ** 62 - 65536 + 4
    with pytest.raises(ValueError, match="2\\*\\*62"):
        popularity_weights(np.array([top, top, top, top]), 1.0)     # 2^62 + 4
    with pytest.raises(ValueError, match="2\\*\\*62"):
        popularity_weights(np.array([2 ** 50]), 1.0)


# ---- the C entry point without a device ---------------------------------------------------------------------------------------

def test_weighted_entry_point_is_declared_and_exported():
    assert "amid_sample_negatives_weighted_i64" in _lib.parse_header()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "amid_sample_negatives_weighted_i64" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def _neg_args(**over):
    """The entry point's arguments in the header's order, every pointer a dummy non-null host address (never dereferenced: the checks
    fail first)."""
    p = 0x1000
    a = dict(pool_d1=p, cum_d1=p, n_pool_d1=10, pool_d2=p, cum_d2=p, n_pool_d2=10, total_d1=1000, total_d2=1000, own_items=p, own_off=p,
             domain_id=p, N=4, k=5, seed=1, epoch=1, out=p, stream=None)
    assert list(a) == _lib.parse_header()["amid_sample_negatives_weighted_i64"][2]
    a.update(over)
    return list(a.values())


def test_weighted_entry_point_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib().raw("amid_sample_negatives_weighted_i64")
    for name in ("pool_d1", "cum_d1", "pool_d2", "cum_d2", "own_items", "own_off", "domain_id", "out"):
        assert f(*_neg_args(**{name: None})) == -1, name
    for name in ("N", "k", "n_pool_d1", "n_pool_d2"):
        assert f(*_neg_args(**{name: 0})) == -1, name
        assert f(*_neg_args(**{name: -3})) == -1, name
    for name in ("total_d1", "total_d2"):
        for v in (0, -5, 2 ** 62, 2 ** 63 - 1):
            assert f(*_neg_args(**{name: v})) == -1, (name, v)
    assert f(*_neg_args(k=2049)) == -2                  # 4 rows x 2049 ids x 8 bytes: past the 64 KiB of LDS a block may ask for
    assert f(*_neg_args(k=2049, total_d1=2 ** 62 - 1, total_d2=1)) == -2      # the largest and the smallest total pass the checks


# ---- the command lines --------------------------------------------------------------------------------------------------------

ARGS = ["--model", "sasrec", "--emb_dim", "64", "--seq_len", "20", "--hid_dim", "16", "--bs", "32", "-ds", "amazon", "-dm", "toy",
        "--overlap_ratio", "0.75"]
MODS = {"train_sr": [], "train_sr_dr": [], "recommend": ["--weights", "none.pt"]}


def _no_gpu(monkeypatch, mod):
    def touched(*a, **k):
        raise AssertionError("the GPU or the data was touched before the refusal")
    monkeypatch.setattr(torch.cuda, "_lazy_init", touched)
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(mod, "DualDomainSeqDataset", touched)


@pytest.mark.parametrize("mod", list(MODS))
def test_parser_takes_the_sampling_flags(mod):
    m = importlib.import_module(f"amid_amd.{mod}")
    d = m.build_parser().parse_args(MODS[mod])
    assert (d.neg_sampling, d.neg_power, d.neg_sampling_for) == ("uniform", 1.0, "both")
    a = m.build_parser().parse_args(MODS[mod] + ["--neg_sampling", "popularity", "--neg_power", "0.75", "--neg_sampling_for", "eval"])
    assert (a.neg_sampling, a.neg_power, a.neg_sampling_for) == ("popularity", 0.75, "eval")
    with pytest.raises(SystemExit):
        m.build_parser().parse_args(MODS[mod] + ["--neg_sampling", "hard"])


@pytest.mark.parametrize("mod", list(MODS))
@pytest.mark.parametrize("flags,msg", [(["--neg_sampling", "popularity", "--neg_power", "1.5"], "--neg_power must be in 0..1"),
                                       (["--neg_sampling", "popularity", "--neg_power", "-0.25"], "--neg_power must be in 0..1"),
                                       (["--neg_power", "0.5"], "--neg_power belongs to --neg_sampling popularity"),
                                       (["--neg_power", "1.0"], "--neg_power belongs to --neg_sampling popularity"),
                                       (["--neg_sampling_for", "both"], "--neg_sampling_for belongs to --neg_sampling popularity"),
                                       (["--neg_sampling", "uniform", "--neg_sampling_for", "eval"],
                                        "--neg_sampling_for belongs to --neg_sampling popularity")])
def test_bad_sampling_flags_exit_before_the_gpu(tmp_path, monkeypatch, mod, flags, msg):
    m = importlib.import_module(f"amid_amd.{mod}")
    _no_gpu(monkeypatch, m)
    with pytest.raises(SystemExit, match=msg):
        m.main(ARGS + MODS[mod] + flags + ["--data_root", str(tmp_path)])


OLD_KEYS = ("model", "emb_dim", "seq_len", "hid_dim", "isItC", "isInC", "dtype", "dataset_type", "domain_type", "bs", "overlap_ratio")


@pytest.mark.parametrize("mod", ["train_sr", "train_sr_dr"])
def test_a_last_pt_from_before_the_flags_counts_as_uniform(tmp_path, monkeypatch, mod):
    m = importlib.import_module(f"amid_amd.{mod}")
    keys = getattr(m, "RESUME_KEYS")
    assert {"neg_sampling", "neg_power", "neg_sampling_for"} <= set(keys)
    from amid_amd.train_sr import read_resume, run_signature
    old = OLD_KEYS + (("isDR",) if mod == "train_sr_dr" else ())
    path = str(tmp_path / "last.pt")
    torch.save({"format": 1, "engine": {}, "extra": {"seed": 0, "epoch": 0, "args": run_signature(m.build_parser().parse_args(ARGS), old)}}, path)
    assert read_resume(m.build_parser().parse_args(ARGS + ["--resume", path]), keys) is not None          # resumes under the defaults
    _no_gpu(monkeypatch, m)
    with pytest.raises(SystemExit, match="--neg_sampling is 'popularity' here but 'uniform' in the file"):
        m.main(ARGS + ["--neg_sampling", "popularity", "--resume", path, "--data_root", str(tmp_path)])
    # and a file of a popularity run is refused by another power
    new = str(tmp_path / "new.pt")
    pop = ARGS + ["--neg_sampling", "popularity", "--neg_power", "0.5"]
    torch.save({"format": 1, "engine": {}, "extra": {"seed": 0, "epoch": 0, "args": run_signature(m.build_parser().parse_args(pop), keys)}}, new)
    assert read_resume(m.build_parser().parse_args(pop + ["--resume", new]), keys) is not None
    with pytest.raises(SystemExit, match="--neg_power is 0.75 here but 0.5 in the file"):
        m.main(ARGS + ["--neg_sampling", "popularity", "--neg_power", "0.75", "--resume", new, "--data_root", str(tmp_path)])


# ---- DeviceBatches without a device -------------------------------------------------------------------------------------------

def test_device_batches_builds_the_prefixes_and_refuses_misaligned_counts():
    ds = DualDomainSeqDataset.from_tokenised(os.path.join(GOLDEN, "tok_cloth_sport_train75.npz"))
    db = DeviceBatches(ds, 8, shuffle=True, device="cpu", negatives="popularity", power=0.75)
    c = item_counts(ds)
    for g in (0, 1):
        w, cum = popularity_weights(c[g], 0.75)
        assert db.cum[g].dtype == torch.int64 and np.array_equal(db.cum[g].numpy(), cum) and db.total[g] == int(cum[-1]) == int(w.sum())
    assert db.k == 1 and db.state_dict().keys() == {"gen", "epoch"}
    ones = (np.ones(len(ds.pool[0]), dtype=np.int64), np.ones(len(ds.pool[1]), dtype=np.int64))
    db = DeviceBatches(ds, 8, shuffle=True, device="cpu", negatives="popularity", counts=ones, power=0.0)
    assert db.total == [65537 * len(ds.pool[0]), 65537 * len(ds.pool[1])]
    with pytest.raises(ValueError, match="aligned with ds.pool"):
        DeviceBatches(ds, 8, shuffle=True, device="cpu", negatives="popularity", counts=(ones[0][:-1], ones[1]))
    with pytest.raises(ValueError, match="aligned with ds.pool"):
        DeviceBatches(ds, 8, shuffle=True, device="cpu", negatives="popularity", counts=(ones[0],))
    with pytest.raises(ValueError, match="power"):
        DeviceBatches(ds, 8, shuffle=True, device="cpu", negatives="popularity", power=2.0)
    with pytest.raises(ValueError, match="belong to negatives='popularity'"):
        DeviceBatches(ds, 8, shuffle=True, device="cpu", counts=ones)
