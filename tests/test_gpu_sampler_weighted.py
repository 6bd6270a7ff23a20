"""GPU tests of the popularity-weighted negative sampler (csrc/sampling.hip): amid_sample_negatives_weighted_i64 called directly, through
DeviceBatches(negatives="popularity") and through the command line, held integer for integer to the host restatement
tests/sampler_weighted_ref.py (whose distribution tests/test_sampler_weighted_cpu.py checks)."""
import numpy as np
import pytest
import torch

from amid_amd.dataset_seq import item_counts, popularity_weights
from tests.sampler_weighted_ref import sample_negatives_weighted_ref

pytestmark = pytest.mark.gpu


def run_kernel(pools, cums, own_rows, domain, k, seed, epoch):
    """amid_sample_negatives_weighted_i64 on cuda:0 -> (int64 [N, k], own_items, own_off).  `out` starts as zeros: the slots an
    exhausted row never reaches are not written by the kernel and are 0 in the restatement."""
    from amid_amd._lib import lib
    N = len(domain)
    off = np.zeros(N + 1, dtype=np.int32)
    np.cumsum([len(o) for o in own_rows], out=off[1:])
    own = np.concatenate([np.asarray(o, dtype=np.int64) for o in own_rows]) if off[-1] else np.zeros(0, dtype=np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    p1, p2, c1, c2, d_off, d_dom = dev(pools[0]), dev(pools[1]), dev(cums[0]), dev(cums[1]), dev(off), dev(np.asarray(domain, dtype=np.int64))
    assert c1.numel() == p1.numel() and c2.numel() == p2.numel() and c1.dtype == c2.dtype == torch.int64
    d_own = dev(own if len(own) else np.zeros(1, dtype=np.int64))          # the entry point refuses a null own_items even when no row has any
    out = torch.zeros(N, k, dtype=torch.int64, device="cuda")
    lib().call("amid_sample_negatives_weighted_i64", p1.data_ptr(), c1.data_ptr(), p1.numel(), p2.data_ptr(), c2.data_ptr(), p2.numel(),
               int(cums[0][-1]), int(cums[1][-1]), d_own.data_ptr(), d_off.data_ptr(), d_dom.data_ptr(), N, k, seed, epoch, out.data_ptr(),
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), own, off


def make_pool(rng, n, lo, hi):
    return np.sort(rng.choice(np.arange(lo, hi, dtype=np.int64), size=n, replace=False))


def own_from(rng, pools, domain, lens):
    return [np.sort(rng.choice(pools[int(d != 0)], size=int(n), replace=False)) for d, n in zip(domain, lens)]


def cums_of(*counts, power=1.0):
    return tuple(popularity_weights(np.asarray(c), power)[1] for c in counts)


def zipf(rng, n):
    """Counts with a long tail, in random order over the pool: a few large, most small."""
    return rng.permutation(1 + 400 // (1 + np.arange(n)))


# every case -> pools, cums, own_rows, domain, k, seed, epoch

def case_train_form():
    rng = np.random.default_rng(11)
    pools = (make_pool(rng, 300, 1, 2000), make_pool(rng, 500, 2000, 5000))
    domain = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1])                         # N = 9 = 2 blocks of 4 rows + 1
    return pools, cums_of(zipf(rng, 300), zipf(rng, 500)), own_from(rng, pools, domain, rng.integers(1, 21, 9)), domain, 1, 3, 1


def case_eval_form():
    rng = np.random.default_rng(12)
    pools = (make_pool(rng, 300, 1, 2000), make_pool(rng, 500, 2000, 5000))
    domain = np.array([1, 0, 0, 1, 0, 1, 1, 0])
    return pools, cums_of(zipf(rng, 300), zipf(rng, 500), power=0.75), own_from(rng, pools, domain, rng.integers(1, 21, 8)), domain, 99, 3, 2


def case_one_round_cut():
    rng = np.random.default_rng(13)
    pools = (make_pool(rng, 4000, 1, 9000), make_pool(rng, 4000, 9000, 18000))
    domain = np.array([0, 1, 0, 1])
    cums = cums_of(rng.integers(1, 5, 4000), rng.integers(1, 5, 4000))     # mild weights: round 0 holds more than k + 1 = 51 distinct ids
    return pools, cums, own_from(rng, pools, domain, [5, 9, 1, 12]), domain, 50, 17, 5


def case_tiny_pool():
    rng = np.random.default_rng(14)
    pools = (np.array([3, 4, 9, 10, 11, 20, 21, 40], dtype=np.int64), np.array([50, 51, 52, 60, 61, 70, 71, 90], dtype=np.int64))
    domain = np.array([0, 1, 0, 0, 1])
    cums = cums_of([1, 8, 2, 5, 3, 8, 1, 4], [2, 2, 16, 9, 4, 2, 7, 3])     # weights within a factor of 8 of each other
    return pools, cums, own_from(rng, pools, domain, [3] * 5), domain, 5, 21, 9      # 8 ids - 3 own = 5 eligible == k


def case_single_id():
    pools = (np.array([77], dtype=np.int64), np.array([78], dtype=np.int64))
    return pools, cums_of([5], [0]), [np.zeros(0, dtype=np.int64)] * 4, np.array([0, 1, 1, 0]), 1, 5, 1


def case_lds_ceiling():
    rng = np.random.default_rng(16)
    pool = 3 * np.arange(5000, dtype=np.int64) + 7
    domain = np.array([0, 0, 1, 0, 1])
    cum = cums_of(5000 // (1 + np.arange(5000)))[0]
    return (pool, pool), (cum, cum), own_from(rng, (pool, pool), domain, [40] * 5), domain, 2048, 23, 4     # 4 x 2048 x 8 bytes = 64 KiB of LDS


def case_exhausted_row():
    rng = np.random.default_rng(17)
    pools = (make_pool(rng, 12, 1, 100), make_pool(rng, 40, 100, 300))
    domain = np.array([0, 1, 0, 0])
    own = own_from(rng, pools, domain, [2, 6, 7, 3])                       # row 2: 12 - 7 = 5 eligible < k = 6
    return pools, cums_of(rng.integers(1, 6, 12), rng.integers(1, 6, 40)), own, domain, 6, 29, 8


def case_large_seed():
    rng = np.random.default_rng(18)
    pools = (make_pool(rng, 200, 1, 1000), make_pool(rng, 150, 1000, 2000))
    domain = np.array([1, 0, 1, 0])
    return pools, cums_of(zipf(rng, 200), zipf(rng, 150)), own_from(rng, pools, domain, [4, 1, 10, 7]), domain, 20, 0xFEDCBA9876543210, 0xFFFFFFFF


def case_heavy_id():
    rng = np.random.default_rng(19)
    pools = (make_pool(rng, 200, 1, 1000), make_pool(rng, 200, 1000, 2000))
    counts = [rng.integers(1, 51, 200), rng.integers(1, 51, 200)]
    counts[0][57] = counts[1][140] = 1_000_000                             # > 99 % of the mass (the others sum to ~5 000)
    domain = np.array([0, 1, 0, 1])
    own = own_from(rng, pools, domain, [4, 6, 3, 5])
    own[2] = np.union1d(own[2], pools[0][57:58])                           # row 2 owns the heavy id: nearly all its candidates are refused
    return pools, cums_of(*counts), own, domain, 20, 31, 2


def case_zero_counts():
    rng = np.random.default_rng(20)
    pools = (make_pool(rng, 100, 1, 1000), make_pool(rng, 120, 1000, 2000))
    counts = [rng.integers(1, 30, 100), rng.integers(1, 30, 120)]
    counts[0][::2] = 0                                                     # weight 1 beside weights of 65 536 x count
    counts[1][[0, 1, 60, 118, 119]] = 0
    domain = np.array([0, 1, 1, 0, 0])
    return pools, cums_of(*counts), own_from(rng, pools, domain, [3, 8, 1, 5, 2]), domain, 10, 37, 3


def case_wide_total():
    """Prefixes passed directly: totals just under 2^62, entries far above 2^32 and weights with low bits set, so that a product cut to
    64 bits, or taken with 32 bits of the total, lands on other indices."""
    w1 = np.array([2 ** 60 + 12345, 3, 2 ** 59 + 7, 2 ** 61 - 2 ** 35, 2 ** 58 + 1, 2 ** 57 - 5, 2 ** 57 + 2 ** 33 + 11], dtype=np.int64)
    w2 = np.array([2 ** 61 - 3, 2 ** 33 + 1, 2 ** 60 + 2 ** 32, 2 ** 59 + 9, 5, 2 ** 59 - 2 ** 34], dtype=np.int64)
    assert sum(w1.tolist()) == 2 ** 62 - 3 * 2 ** 33 + 12362 and sum(w2.tolist()) == 2 ** 62 - 2 ** 32 + 12
    pools = (np.arange(10, 17, dtype=np.int64), np.arange(30, 36, dtype=np.int64))
    domain = np.array([0, 1, 1, 0, 0, 1])
    own = [np.array([13]), np.array([30]), np.zeros(0, np.int64), np.zeros(0, np.int64), np.array([10, 13]), np.array([32])]
    return pools, (np.cumsum(w1), np.cumsum(w2)), own, domain, 3, 41, 6


def _ends(n1, n2, seed):
    rng = np.random.default_rng(seed)
    pools = (make_pool(rng, n1, 1, 3000), make_pool(rng, n2, 3000, 6000))
    counts = [rng.integers(1, 4, n1), rng.integers(1, 4, n2)]
    for c in counts:                                                       # the first and the last index are met often: the search's two ends
        c[0] = c[-1] = 2 * len(c)
    domain = np.array([0, 1, 1, 0, 1, 0, 1, 0, 1])
    return pools, cums_of(*counts), [np.zeros(0, dtype=np.int64)] * 9, domain, min(8, n1, n2), 43, 7


CASES = dict(train_form=case_train_form, eval_form=case_eval_form, one_round_cut=case_one_round_cut, tiny_pool=case_tiny_pool,
             single_id=case_single_id, lds_ceiling=case_lds_ceiling, exhausted_row=case_exhausted_row, large_seed=case_large_seed,
             heavy_id=case_heavy_id, zero_counts=case_zero_counts, wide_total=case_wide_total,
             ends_1_2=lambda: _ends(1, 2, 44), ends_2_1=lambda: _ends(2, 1, 45), ends_255_257=lambda: _ends(255, 257, 46),
             ends_256_1023=lambda: _ends(256, 1023, 47), ends_1025_63=lambda: _ends(1025, 63, 48))


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_host_restatement(name):
    pools, cums, own_rows, domain, k, seed, epoch = CASES[name]()
    N = len(domain)
    off = np.zeros(N + 1, dtype=np.int32)
    np.cumsum([len(o) for o in own_rows], out=off[1:])
    own = np.concatenate([np.asarray(o, dtype=np.int64) for o in own_rows]) if off[-1] else np.zeros(0, dtype=np.int64)
    ref_of = lambda kk, **kw: sample_negatives_weighted_ref(pools[0], cums[0], pools[1], cums[1], own, off, domain, kk, seed, epoch, **kw)   # noqa: E731
    rounds: list = []
    ref = ref_of(k, rounds_out=rounds)
    # what each case is there for, shown on the restatement so that the case cannot quietly stop visiting its path
    for d in (0, 1):
        assert (np.diff(cums[d]) > 0).all() and cums[d][0] > 0 and 0 < int(cums[d][-1]) < 2 ** 62
    if name == "one_round_cut":        # round 0 alone yields more than k ids: the kernel has to cut at slot k
        assert (ref_of(k + 1, max_rounds=1)[:, 0] >= 0).all()
    if name in ("eval_form", "lds_ceiling", "heavy_id"):      # more than one round: accepted ids are read back from LDS
        assert (ref_of(k, max_rounds=1)[:, 0] == -1).any()
    if name == "tiny_pool":
        for d in (0, 1):
            w = np.diff(cums[d], prepend=0)
            assert w.max() <= 8 * w.min()
        assert all(len(pools[int(domain[r] != 0)]) - len(own_rows[r]) == k for r in range(N))
    if name == "heavy_id":
        for d, j in ((0, 57), (1, 140)):
            assert np.diff(cums[d], prepend=0)[j] > 0.99 * int(cums[d][-1])
        assert pools[0][57] in own_rows[2] and pools[0][57] not in ref[2] and pools[0][57] in ref[0] and max(rounds) > 8
    if name == "zero_counts":
        assert (np.diff(cums[0], prepend=0) == 1).sum() == 50 and (np.diff(cums[1], prepend=0) == 1).sum() == 5
    if name == "wide_total":
        for d in (0, 1):
            assert 2 ** 62 - 2 ** 40 < int(cums[d][-1]) < 2 ** 62 and (cums[d] > 2 ** 32).all()
        # a product that wraps at 64 bits, and one taken with the low word of the total alone, would pick other indices on this input
        from tests.sampler_weighted_ref import SITE_NEG_W, philox4x32
        ctr = np.array([[(3 << 20) | lane, 0, SITE_NEG_W, epoch] for lane in range(64)], dtype=np.uint32)
        x = philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32))
        tot = int(cums[0][-1])
        full = [((((int(a) << 32) | int(b)) * tot) >> 64) for a, b in x[:, :2].tolist()]
        low = [((((int(a) << 32) | int(b)) * (tot & 0xFFFFFFFF)) >> 64) for a, b in x[:, :2].tolist()]
        wrap = [((int(a) * tot) & (2 ** 64 - 1)) >> 32 for a, _ in x[:, :2].tolist()]
        idx = lambda t: np.searchsorted(cums[0], np.array(t, dtype=np.int64), side="right")     # noqa: E731
        assert (idx(full) != idx(low)).any() and (idx(full) != idx(wrap)).any()
    if name.startswith("ends_"):
        for d in (0, 1):
            rows = ref[np.asarray(domain != 0) == bool(d)]
            assert pools[d][0] in rows and pools[d][-1] in rows
        assert {len(pools[0]), len(pools[1])} == set(map(int, name.split("_")[1:]))
    if name == "exhausted_row":
        assert ref[2, 0] == -1 and (ref[[0, 1, 3], 0] >= 0).all()
        # the 5 eligible ids were all found: slot 0 gave way to the mark, 4 stay behind it, slot 5 was never reached
        assert np.isin(ref[2, 1:5], np.setdiff1d(pools[0], own_rows[2])).all() and len(set(ref[2, 1:5].tolist())) == 4 and ref[2, 5] == 0
        assert rounds[2] == 4096 and max(rounds[:2] + rounds[3:]) <= 256
    else:
        assert (ref >= 0).all() and max(rounds) <= 256, max(rounds)
        for r in range(N):                 # the restatement itself obeys the sampling rule on this case
            assert np.isin(ref[r], pools[int(domain[r] != 0)]).all() and not np.isin(ref[r], own_rows[r]).any()
            assert len(set(ref[r].tolist())) == k
    got, own_k, off_k = run_kernel(pools, cums, own_rows, domain, k, seed, epoch)
    assert np.array_equal(own_k, own) and np.array_equal(off_k, off)
    assert got.shape == ref.shape
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), f"{name}: {len(bad)} of {ref.size} slots differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


# ---- DeviceBatches(negatives="popularity") ------------------------------------------------------------------------------------

def _loader(tmp_path, seed=3, rank=0, world=1, power=1.0):
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    from tests.test_gpu_module import _write_csv
    root = tmp_path / "amazon_dataset"
    if not root.exists():
        root.mkdir()
        _write_csv(root / "toy_test.csv", 40, np.random.default_rng(5), 1, 300, 300, 700)
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=20, long_length=7, pad_id=1001, seed=3, csv_path=str(root / "toy_test.csv"))
    return ds, DeviceBatches(ds, 8, shuffle=True, device="cuda:0", seed=seed, rank=rank, world=world, negatives="popularity", power=power)


def _restated(ds, counts, power, k, seed, epoch):
    off = np.zeros(len(ds) + 1, dtype=np.int32)
    np.cumsum([len(o) for o in ds.own_items], out=off[1:])
    cums = [popularity_weights(c, power)[1] for c in counts]
    return sample_negatives_weighted_ref(ds.pool[0], cums[0], ds.pool[1], cums[1], np.concatenate(ds.own_items), off, ds.domain_id, k, seed, epoch)


def test_device_batches_draws_the_restated_table(tmp_path):
    ds, db = _loader(tmp_path, seed=6, power=0.75)
    for epoch in (1, 2):
        got = db.sample_negatives().cpu().numpy()
        ref = _restated(ds, item_counts(ds), 0.75, 20, db.seed, epoch)
        assert got.shape == (40, 20) and (ref >= 0).all()
        assert np.array_equal(got, ref), epoch


def test_resumed_loader_draws_what_the_uninterrupted_one_does(tmp_path):
    ds, db = _loader(tmp_path)
    db.sample_negatives()
    sd = db.state_dict()
    assert sd.keys() == {"gen", "epoch"}
    want = [db.sample_negatives().cpu().numpy() for _ in range(2)]
    _, fresh = _loader(tmp_path)
    fresh.load_state_dict(sd)
    got = [fresh.sample_negatives().cpu().numpy() for _ in range(2)]
    assert not np.array_equal(want[0], want[1])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_every_rank_draws_the_same_table(tmp_path):
    _, a = _loader(tmp_path, rank=0, world=2)
    _, b = _loader(tmp_path, rank=1, world=2)
    for _ in range(2):
        assert torch.equal(a.sample_negatives(), b.sample_negatives())


def test_a_short_row_raises(tmp_path):
    """Row 0 has exactly k = 5 eligible ids; one of them has weight 1 against a total near 2^61, so 4096 x 64 candidates never meet it."""
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    ids = list(range(1, 13))
    path = tmp_path / "toy.csv"
    path.write_text("user_id,seq_d1,seq_d2,domain_id\n" f'0,"{ids[:7]}","[50]",0\n' f'1,"{ids[6:]}","[51, 52]",0\n')
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=5, long_length=7, pad_id=1001, csv_path=str(path))
    assert ds.pool[0].tolist() == ids and len(ds.own_items[0]) == 7 and len(ds.own_items[1]) == 6
    c1 = np.full(12, 2 ** 40, dtype=np.int64)
    c1[10], c1[11] = 2 ** 45, 0                      # ids 11 and 12, both eligible for row 0 only: weights 2^61 + 1 and 1
    counts = (c1, np.ones(3, dtype=np.int64))
    w, cum = popularity_weights(c1, 1.0)
    assert w[11] == 1 and 2 ** 61 < int(cum[-1]) < 2 ** 61 + 2 ** 60
    ref = _restated(ds, counts, 1.0, 5, 4, 1)
    assert ref[0, 0] == -1 and 12 not in ref[0] and (ref[1] >= 0).all()
    db = DeviceBatches(ds, 1, shuffle=False, device="cuda:0", seed=4, negatives="popularity", counts=counts)
    with pytest.raises(RuntimeError, match="row 0 "):
        db.sample_negatives()
    ok = DeviceBatches(ds, 1, shuffle=False, device="cuda:0", seed=4, negatives="popularity", counts=counts, power=0.0)
    assert np.array_equal(ok.sample_negatives().cpu().numpy(), _restated(ds, counts, 0.0, 5, 4, 1))


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_cli_evaluates_on_negatives_weighted_by_the_training_counts(tmp_path, monkeypatch):
    """train_sr.py --neg_sampling popularity --neg_sampling_for eval, one epoch on a toy CSV pair: the evaluation loader draws the
    restated table for the TRAINING CSV's counts mapped onto its pools, the training loader stays uniform, and test()'s metrics are
    those model.forward gives on the same batches."""
    from amid_amd import train_sr
    from amid_amd.dataset_seq import DualDomainSeqDataset
    from tests.test_gpu_module import _write_csv
    rng = np.random.default_rng(0)
    root = tmp_path / "amazon_dataset"
    root.mkdir()
    _write_csv(root / "toy_train75.csv", 300, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_test.csv", 80, rng, 1, 400, 400, 900)
    seen = []
    orig = train_sr.test

    def spy(model, args, val_batches):
        sd = val_batches.state_dict()
        res = orig(model, args, val_batches)
        assert model.engine.EVAL_FUSED
        val_batches.load_state_dict(sd)
        model.engine.EVAL_FUSED = False
        try:
            plain = orig(model, args, val_batches)               # the same draw again, through model.forward + the rank kernel
        finally:
            model.engine.EVAL_FUSED = True
        val_batches.load_state_dict(sd)
        seen.append((val_batches, int(sd["epoch"]) + 1, val_batches.epoch_tensors()["neg_samples"].cpu().numpy(), res, plain))
        return res

    monkeypatch.setattr(train_sr, "test", spy)
    summary = train_sr.main(["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--overlap_ratio", "0.75", "--model", "sasrec",
                             "--bs", "32", "--seq_len", "20", "--emb_dim", "64", "--hid_dim", "16", "--epoch", "1", "--neg_nums", "19",
                             "--seeds", "1", "-md", str(tmp_path / "model"), "--neg_sampling", "popularity", "--neg_power", "0.75",
                             "--neg_sampling_for", "eval"])
    assert len(summary) == 1 and len(seen) == 1
    vb, epoch, neg, res, plain = seen[0]
    assert vb.negatives == "popularity" and epoch == 1
    mk = lambda f, tr: DualDomainSeqDataset(seq_len=20, isTrain=tr, neg_nums=19, long_length=7, pad_id=447411, csv_path=str(root / f))   # noqa: E731
    ds_train, ds_val = mk("toy_train75.csv", True), mk("toy_test.csv", False)
    counts = item_counts(ds_train, onto=ds_val.pool)
    assert any((c == 0).any() for c in counts) and not all(np.array_equal(a, b) for a, b in zip(counts, item_counts(ds_val)))
    ref = _restated(ds_val, counts, 0.75, 19, vb.seed, 1)
    assert (ref >= 0).all()
    assert neg.shape == (2, 32, 19) and np.array_equal(neg.reshape(64, 19), ref[:64])         # shuffle=False, drop_last
    for key, v in plain.items():
        if key == "loss":
            assert abs(res[key] - v) <= 1e-6 * abs(v)
        else:
            assert res[key] == v or all(np.isnan(a) and np.isnan(b) or a == b for a, b in zip(res[key], v)), key


def test_cli_train_sr_dr_weighs_every_training_loader_by_its_own_counts(tmp_path, monkeypatch):
    """train_sr_dr.py --neg_sampling popularity --neg_sampling_for train, one epoch: the train and the _DR loader draw the restated tables
    for their OWN CSV's counts (k = 1) and the evaluation loader stays on the uniform kernel."""
    from amid_amd import train_sr_dr
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    from tests.test_gpu_module import _write_csv
    rng = np.random.default_rng(2)
    root = tmp_path / "mybank_dataset"
    root.mkdir()
    _write_csv(root / "toy_train25.csv", 200, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_train25_DR.csv", 160, rng, 1, 400, 400, 900, ob_label=True)
    _write_csv(root / "toy_test.csv", 64, rng, 1, 400, 400, 900)
    drawn = []
    orig = DeviceBatches.sample_negatives
    monkeypatch.setattr(DeviceBatches, "sample_negatives", lambda self: drawn.append((self, self.epoch + 1, orig(self))) or drawn[-1][2])
    summary = train_sr_dr.main(["--data_root", str(tmp_path), "-ds", "mybank", "-dm", "toy", "--overlap_ratio", "0.25", "--model", "sasrec",
                                "--neg_nums", "19", "--bs", "32", "--seq_len", "20", "--emb_dim", "64", "--hid_dim", "16", "--epoch", "1",
                                "--seeds", "1", "-md", str(tmp_path / "model"), "--neg_sampling", "popularity", "--neg_sampling_for", "train"])
    assert len(summary) == 1 and all((0.0 <= v <= 1.0) or np.isnan(v) for v in summary[0].values())
    assert [(len(ld.ds), ld.negatives, ld.k) for ld, _, _ in drawn] == [(200, "popularity", 1), (64, "device", 19), (160, "popularity", 1)]
    for (ld, epoch, neg), name in zip((drawn[0], drawn[2]), ("toy_train25.csv", "toy_train25_DR.csv")):
        ds = DualDomainSeqDataset(seq_len=20, isTrain=True, neg_nums=19, long_length=7, pad_id=447411, csv_path=str(root / name))
        assert epoch == 1 and np.array_equal(neg.cpu().numpy(), _restated(ds, item_counts(ds), 1.0, 1, ld.seed, 1)), name
