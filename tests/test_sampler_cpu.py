"""CPU-side checks of the negative sampler (csrc/sampling.hip).  The kernel is deterministic in (seed, epoch, row, pool, own, k) and
tests/test_gpu_sampler.py holds it bit for bit to oracle.sample_negatives_ref; here that restatement is shown to be what the
reference's random.sample(pool - set(own), k) is -- uniform without replacement, every output slot uniform too -- at a sample size
no GPU test could afford, and the C entry point is shown to refuse bad arguments before it touches a device."""
import os
import subprocess

import numpy as np
import pytest

from amid_amd import _lib
from oracle import amid_oracle as orc

POOL = np.arange(100, 140, dtype=np.int64)           # 40 consecutive ids
OWN = POOL[::5].copy()                               # every fifth: 8 own, 32 eligible
ELIGIBLE = np.setdiff1d(POOL, OWN)
OFF1 = np.array([0, len(OWN)], dtype=np.int32)
DOM1 = np.zeros(1, dtype=np.int64)


def draw(k, seed, epoch, n_rows=1, max_rounds=4096):
    """n_rows rows, all of domain 0 with pool POOL and own list OWN."""
    own = np.tile(OWN, n_rows)
    off = (np.arange(n_rows + 1) * len(OWN)).astype(np.int32)
    return orc.sample_negatives_ref(POOL, POOL, own, off, np.zeros(n_rows, dtype=np.int64), k, seed, epoch, max_rounds)


@pytest.fixture(scope="module")
def draws():
    """4000 draws of row 0 (epochs 1..4000, seed 9, k = 8) -> [4000, 8]."""
    return np.concatenate([draw(8, 9, e) for e in range(1, 4001)], axis=0)


def test_every_draw_is_distinct_and_eligible(draws):
    assert draws.shape == (4000, 8)
    assert np.isin(draws, ELIGIBLE).all()
    s = np.sort(draws, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all()


def test_uniform_without_replacement(draws):
    """Pearson chi-square of the per-item counts (expected 4000 * 8 / 32 = 1000 each, 31 degrees of freedom) and of the item x slot
    table (expected 4000 / 32 = 125 each, 32 * 8 - 1 = 255 degrees of freedom) against the 1 - 1e-6 quantiles of chi-square.  The
    seeds are fixed, so this is a deterministic statement about the restated rule, not a flaky one."""
    from scipy.stats import chi2
    col = np.searchsorted(ELIGIBLE, draws)                                   # [4000, 8] item index 0..31
    marg = np.bincount(col.reshape(-1), minlength=32).astype(np.float64)
    chi_marg = float(((marg - 1000.0) ** 2 / 1000.0).sum())
    table = np.zeros((32, 8))
    for s in range(8):
        table[:, s] = np.bincount(col[:, s], minlength=32)
    chi_slot = float(((table - 125.0) ** 2 / 125.0).sum())
    bound_marg, bound_slot = float(chi2.isf(1e-6, 31)), float(chi2.isf(1e-6, 255))
    print(f"sampler chi-square: marginal {chi_marg:.2f} (bound {bound_marg:.2f}), item x slot {chi_slot:.1f} (bound {bound_slot:.2f})")
    assert chi_marg < bound_marg
    assert chi_slot < bound_slot


def test_eligible_equals_k_returns_the_complement():
    out = draw(32, 9, 1)
    assert np.array_equal(np.sort(out[0]), ELIGIBLE)


def test_exhausted_pool_sets_the_sentinel():
    out = draw(33, 9, 1, max_rounds=50)
    assert out[0, 0] == -1
    assert np.array_equal(np.sort(out[0, 1:32]), np.setdiff1d(ELIGIBLE, draw(32, 9, 1)[0, :1]))     # the rest of what it held stays
    assert out[0, 32] == 0                                                                          # never reached


def test_draw_for_k_is_a_prefix_of_the_draw_for_a_larger_k():
    big = draw(32, 5, 7)
    for k in (1, 2, 8, 31):
        assert np.array_equal(draw(k, 5, 7)[0], big[0, :k])


def test_a_row_does_not_depend_on_its_neighbours():
    a, b, c = draw(8, 5, 3, 1), draw(8, 5, 3, 5), draw(8, 5, 3, 8)
    assert np.array_equal(a, b[:1]) and np.array_equal(b, c[:5])


def test_identical_rows_and_consecutive_epochs_draw_differently():
    t = draw(8, 5, 3, 8)
    assert len({tuple(row) for row in t.tolist()}) == 8
    assert not np.array_equal(draw(8, 5, 3), draw(8, 5, 4))
    assert not np.array_equal(draw(8, 5, 3), draw(8, 6, 3))


# ---- the C entry point without a device -------------------------------------------------------------------------------------

def test_sample_negatives_is_declared_and_exported():
    assert "amid_sample_negatives_i64" in _lib.parse_header()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "amid_sample_negatives_i64" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def _neg_args(**over):
    """amid_sample_negatives_i64's arguments, every pointer a dummy non-null host address (never dereferenced: the checks fail first)."""
    p = 0x1000
    a = dict(pool_d1=p, n_pool_d1=10, pool_d2=p, n_pool_d2=10, own_items=p, own_off=p, domain_id=p, N=4, k=5, seed=1, epoch=1, out=p,
             stream=None)
    a.update(over)
    return list(a.values())


def test_sample_negatives_refuses_bad_arguments_without_a_gpu():
    f = _lib.lib().raw("amid_sample_negatives_i64")
    for name in ("pool_d1", "pool_d2", "own_items", "own_off", "domain_id", "out"):
        assert f(*_neg_args(**{name: None})) == -1, name
    for name in ("N", "k", "n_pool_d1", "n_pool_d2"):
        assert f(*_neg_args(**{name: 0})) == -1, name
    assert f(*_neg_args(k=2049)) == -2                  # 4 rows x 2049 ids x 8 bytes: one id per row past the 64 KiB of LDS a block may ask for


# ---- who keeps the exhausted-pool sentinel away from DeviceBatches ------------------------------------------------------------

def _toy_dataset(tmp_path, n_own, is_train, neg_nums):
    """One row of domain 0 with n_own distinct own items out of a domain-0 pool of 12 ids (a second row brings in the rest of the pool)."""
    from amid_amd.dataset_seq import DualDomainSeqDataset
    ids = list(range(1, 13))
    path = tmp_path / "toy.csv"
    path.write_text("user_id,seq_d1,seq_d2,domain_id\n"
                    f'0,"{ids[:n_own]}","[50]",0\n'
                    f'1,"{ids[n_own - 1:]}","[51, 52]",0\n')
    ds = DualDomainSeqDataset(seq_len=20, isTrain=is_train, neg_nums=neg_nums, long_length=7, pad_id=1001, csv_path=str(path))
    assert len(ds.pool[0]) == 12 and len(ds.own_items[0]) == n_own
    return ds


def test_device_batches_refuses_a_pool_that_could_exhaust(tmp_path):
    """amid_sample_negatives_i64 marks a row whose pool runs out with out[r][0] = -1 and DeviceBatches.sample_negatives never looks
    for the mark: the constructor is what keeps it from ever appearing, by refusing k + len(own) > len(pool) for any row."""
    from amid_amd.dataset_seq import DeviceBatches
    ds = _toy_dataset(tmp_path, n_own=7, is_train=False, neg_nums=5)          # 5 + 7 == 12: every eligible id is drawn, none is missing
    assert DeviceBatches(ds, 1, shuffle=False, device="cpu").k == 5
    ds = _toy_dataset(tmp_path, n_own=7, is_train=False, neg_nums=6)          # 6 + 7 == 12 + 1
    with pytest.raises(ValueError, match="negative pool smaller than neg_nums"):
        DeviceBatches(ds, 1, shuffle=False, device="cpu")
    ds = _toy_dataset(tmp_path, n_own=12, is_train=True, neg_nums=6)          # the train form draws k = 1: 1 + 12 == 12 + 1
    with pytest.raises(ValueError, match="negative pool smaller than neg_nums"):
        DeviceBatches(ds, 1, shuffle=False, device="cpu")
    ds = _toy_dataset(tmp_path, n_own=11, is_train=True, neg_nums=6)          # 1 + 11 == 12
    assert DeviceBatches(ds, 1, shuffle=False, device="cpu").k == 1
