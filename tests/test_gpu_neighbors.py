"""The nearest-neighbour kernel (csrc/neighbors.hip, SasrecEngine.enqueue_neighbors) against float64 on the host.

Shapes: Q in {1, 15, 16, 17, 33}; N in {1, 127, 128, 129, 255, 256, 257, 700} -- the kernel's candidate tile is 128 rows, so one row below, at
and above one and two tiles, and 700 = 6 tiles.  The scan cuts the tiles into ranges so as to fill 256 workgroups, which at these sizes is a
range per tile (N = 129 on: several lists per query, merged by the last launch); every case runs again with the target lowered to 1
workgroup (one range walks every tile: the running lists, their thresholds and the flagged merges) and to 2 (700 rows: two ranges of
three tiles, merged); k in {1, 10, 256} (k > 64 takes the
one-query-group workgroup form, k > N pads); D in {64, 128}; both metrics; queries as ids and as vectors; pool None and a strict subset;
exclude_self on and off.  Data N(0, 1) with three pairs of bit-identical rows, one all-zero row and one row scaled by 1e4.

The bar is derived, not measured.  u = 2^-24, gamma_D = D u / (1 - D u).
  dot:    2 gamma_D sum_i |a_i b_i|.  Any fp32 summation order of D products is within gamma_D times that sum (Higham, Accuracy and
          Stability of Numerical Algorithms, section 3.1); the factor 2 covers a piece-product implementation, whose dropped piece pairs are
          each at most about 2u |a_i b_i|.
  cosine: 4 gamma_D + 8u, absolute.  The dot term divided by |a||b| is at most 2 gamma_D (Cauchy-Schwarz: sum |a_i b_i| <= |a||b|); each of
          the two fp32 norms adds at most gamma_D + 4u relative (the sum of squares gamma_D, halved by the root, plus the root's, the
          inverse's and the product's roundings) to a score that is at most 1.
Per query, with every score recomputed in float64 and no candidate left out:
  1. every returned score is within the bar of the float64 score of its returned id;
  2. scores are non-increasing, equal scores in ascending id order;
  3. no candidate that was not returned has a float64 score above the worst returned float64 score plus the bar (for dot the smaller of the
     two pairs' bars);
  4. padding is exactly (-1, -inf) and appears only when the query has fewer than k candidates;
  5. a planted duplicate pair returns bit-equal scores, lower id first.
The worst observed share of the bar is logged (tests.test_gpu_sasrec.log) and recorded in profiles/neighbors.md."""
import numpy as np
import pytest
import torch

from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
QS = (1, 15, 16, 17, 33)
NS = (1, 127, 128, 129, 255, 256, 257, 700)
KS = (1, 10, 256)
GUARD = 8                     # rows of large values in front of and behind every matrix: a read outside it would win every list
_ENG = {}
_WORST = {"dot": 0.0, "cosine": 0.0}


def engine():
    if "e" not in _ENG:
        from amid_amd.engine import SasrecEngine
        _ENG["e"] = SasrecEngine(64, 64, 8, 16, device="cuda:0", lr=1e-3, seed=0)
    return _ENG["e"]


def gamma(D):
    return D * U / (1.0 - D * U)


def planted(N):
    """(duplicate pairs (lower id, higher id), zero row, scaled row) for a matrix of N rows."""
    if N < 16:
        return [], None, None
    return [(1, N - 1), (3, N // 2), (5, 7)], 2, 4


def make_data(N, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    pairs, zero, scaled = planted(N)
    for lo, hi in pairs:
        x[hi] = x[lo]
    if zero is not None:
        x[zero] = 0.0
        x[scaled] *= np.float32(1e4)
    return x


def on_device(x):
    """x [N, D] as a contiguous view inside a larger buffer whose neighbouring rows hold 1e3."""
    big = torch.full((x.shape[0] + 2 * GUARD, x.shape[1]), 1e3, dtype=torch.float32, device="cuda:0")
    base = big[GUARD:GUARD + x.shape[0]]
    base.copy_(torch.from_numpy(x))
    assert base.is_contiguous()
    return base


def query_ids(N, Q, seed):
    rng = np.random.default_rng(seed + 1)
    pairs, zero, scaled = planted(N)
    head = [p for pair in pairs[:2] for p in pair] + ([zero, scaled] if zero is not None else [])
    ids = np.array(head + rng.integers(0, N, size=64).tolist(), dtype=np.int64)[:Q]
    return ids % N


def subset_pool(N, seed):
    """A strict subset of the rows that keeps every planted row (sorted unique)."""
    rng = np.random.default_rng(seed + 2)
    pairs, zero, scaled = planted(N)
    keep = set(p for pair in pairs for p in pair) | ({zero, scaled} if zero is not None else set())
    pick = set(np.nonzero(rng.random(N) < 0.6)[0].tolist()) | keep
    if len(pick) == N:
        pick.discard(max(pick - keep) if pick - keep else N - 1)
    return np.array(sorted(pick), dtype=np.int64)


def reference(qv, x, metric):
    """float64 scores [Q, N] and the bar [Q, N] of every (query, row) pair."""
    D = x.shape[1]
    a, b = qv.astype(np.float64), x.astype(np.float64)
    dot = a @ b.T
    if metric == "dot":
        return dot, 2.0 * gamma(D) * (np.abs(a) @ np.abs(b).T)
    na = np.maximum(np.sqrt((a * a).sum(1)), 1e-8)
    nb = np.maximum(np.sqrt((b * b).sum(1)), 1e-8)
    return dot / (na[:, None] * nb[None, :]), np.full(dot.shape, 4.0 * gamma(D) + 8.0 * U)


def run(base, queries, pool, metric, k, exclude_self, expect_flag=False, wgs=0):
    """wgs: the scan's target workgroup count for this call (0: the default, 256 -- at these sizes a range per tile; 1: one range walks
    every tile, the running lists, their thresholds and the flagged merges at work; 2: ranges of several tiles, merged)."""
    from amid_amd._lib import lib
    eng = engine()
    lib().value("amid_neighbors_target_workgroups", wgs)
    try:
        return _run(eng, base, queries, pool, metric, k, exclude_self, expect_flag)
    finally:
        lib().value("amid_neighbors_target_workgroups", 0)


def _run(eng, base, queries, pool, metric, k, exclude_self, expect_flag):
    q = torch.from_numpy(queries).cuda()
    p = None if pool is None else torch.from_numpy(pool).cuda()
    ids = torch.full((q.shape[0], k), -7, dtype=torch.int64, device="cuda:0")
    sc = torch.full((q.shape[0], k), float("nan"), dtype=torch.float32, device="cuda:0")
    flags = eng.flags_holder()
    eng.stream.wait_stream(torch.cuda.current_stream())
    eng.enqueue_neighbors(q, base, p, metric, k, exclude_self, ids, sc, flags.err)
    torch.cuda.current_stream().wait_stream(eng.stream)
    if expect_flag:
        with pytest.raises(IndexError):
            eng.check_index_error(flags)
    else:
        eng.check_index_error(flags)
    return ids.cpu().numpy(), sc.cpu().numpy()


def check(tag, ids, sc, ref, bar, cands, own, pairs, metric):
    """The five checks for every query.  ref / bar [Q, N]; cands: the valid candidate rows (sorted); own [Q]: the row left out of query
    q's candidates (-1: none; None entry: the query itself is absent -> all padding)."""
    k = ids.shape[1]
    for qi in range(ids.shape[0]):
        where = (tag, qi)
        if own[qi] is None:
            assert (ids[qi] == -1).all() and np.isneginf(sc[qi]).all(), where
            continue
        cq = cands[cands != own[qi]]
        n_ret = min(k, len(cq))
        got, s = ids[qi, :n_ret], sc[qi, :n_ret]
        assert (ids[qi, n_ret:] == -1).all() and np.isneginf(sc[qi, n_ret:]).all(), where            # 4
        assert (got >= 0).all() and np.isin(got, cq).all() and len(set(got.tolist())) == n_ret, where
        if n_ret == 0:
            continue
        r, b = ref[qi], bar[qi]
        err = np.abs(s.astype(np.float64) - r[got])
        assert (err <= b[got]).all(), (where, float((err / np.maximum(b[got], 1e-300)).max()))      # 1
        share = float((err[b[got] > 0] / b[got][b[got] > 0]).max()) if (b[got] > 0).any() else 0.0
        _WORST[metric] = max(_WORST[metric], share)
        assert (s[1:] <= s[:-1]).all(), where                                                        # 2
        tie = s[1:] == s[:-1]
        assert (got[1:][tie] > got[:-1][tie]).all(), where
        rest = np.setdiff1d(cq, got)
        if len(rest):                                                                                # 3
            w = got[np.argmin(r[got])]
            assert (r[rest] <= r[w] + np.minimum(b[rest], b[w])).all(), where
        pos = {int(g): i for i, g in enumerate(got)}
        for lo, hi in pairs:                                                                         # 5
            if lo in cq and hi in cq and hi in pos:
                assert lo in pos and pos[lo] < pos[hi], (where, lo, hi)
                assert s[pos[lo]].tobytes() == s[pos[hi]].tobytes(), (where, lo, hi)


@pytest.mark.parametrize("wgs", (0, 1, 2))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("metric", ("dot", "cosine"))
@pytest.mark.parametrize("D", (64, 128))
def test_neighbors_against_float64(D, metric, N, wgs):
    seed = 1000 * D + N
    x = make_data(N, D, seed)
    base = on_device(x)
    pairs, _, _ = planted(N)
    all_rows = np.arange(N, dtype=np.int64)
    pools = [None] if N == 1 else [None, subset_pool(N, seed)]         # (one row has no strict non-empty subset)
    qid_all = query_ids(N, max(QS), seed)
    qvec_all = x[qid_all].copy()
    fresh = np.random.default_rng(seed + 3).standard_normal(qvec_all.shape).astype(np.float32)
    qvec_all[6::2] = fresh[6::2]                                       # rows of the matrix (duplicates, zero, scaled) and free vectors
    ref_id, bar_id = reference(x[qid_all], x, metric)
    ref_v, bar_v = reference(qvec_all, x, metric)
    for Q in QS:
        for k in KS:
            for pool in pools:
                cands = all_rows if pool is None else pool
                tag = (D, metric, N, Q, k, "all" if pool is None else "subset")
                for excl in (True, False):
                    ids, sc = run(base, qid_all[:Q], pool, metric, k, excl, wgs=wgs)
                    own = [int(i) if excl else -1 for i in qid_all[:Q]]
                    check(tag + ("ids", excl), ids, sc, ref_id[:Q], bar_id[:Q], cands, own, pairs, metric)
                ids, sc = run(base, qvec_all[:Q], pool, metric, k, False, wgs=wgs)
                check(tag + ("vectors",), ids, sc, ref_v[:Q], bar_v[:Q], cands, [-1] * Q, pairs, metric)
    log(f"neighbors D {D} {metric} N {N} wgs {wgs}: worst share of the bar so far {_WORST[metric]:.4f}")
    print(f"neighbors D {D} {metric} N {N} wgs {wgs}: worst share of the bar so far {_WORST[metric]:.4f}")


@pytest.mark.parametrize("metric", ("dot", "cosine"))
@pytest.mark.parametrize("D", (64, 128))
def test_a_score_does_not_depend_on_its_position(D, metric):
    """The same (query, candidate) pair inside two pools -- another tile, another slot, another range count -- and from another query slot
    and workgroup form (k = 256: the one-query-group form; k = 64: four groups): the same bits."""
    N = 700
    x = make_data(N, D, 77 + D)
    base = on_device(x)
    qids = query_ids(N, 33, 5)
    sub = subset_pool(N, 9)
    sub = sub[sub % 3 != 0]                                             # shifts every survivor's tile and slot
    full_i, full_s = run(base, qids, None, metric, 256, False)
    sub_i, sub_s = run(base, qids, sub, metric, 256, False)
    rev_i, rev_s = run(base, qids[::-1].copy(), sub, metric, 64, False, wgs=1)     # ... and one range instead of a range per tile
    vec_i, vec_s = run(base, x[qids[:5]], sub, metric, 64, False)
    n_common = 0
    for qi in range(len(qids)):
        f = {int(i): s.tobytes() for i, s in zip(full_i[qi], full_s[qi]) if i >= 0}
        for i, s in zip(sub_i[qi], sub_s[qi]):
            if int(i) in f:
                n_common += 1
                assert f[int(i)] == s.tobytes(), (qi, int(i))
        r = len(qids) - 1 - qi
        assert np.array_equal(rev_i[r], sub_i[qi, :64]) and rev_s[r].tobytes() == sub_s[qi, :64].tobytes(), qi
    assert n_common > 33 * 50
    assert np.array_equal(vec_i, sub_i[:5, :64]) and vec_s.tobytes() == sub_s[:5, :64].tobytes()      # a row as a vector: the row's bits


@pytest.mark.parametrize("D", (64, 128))
def test_out_of_range_ids_are_flagged_and_skipped(D):
    """One query id and one pool id (and a negative one of each) outside [0, N): IndexError from check_index_error, the bad query's row is
    padding, the bad candidates are absent, every other row passes the float64 checks, and nothing outside the matrix was read (the rows
    around it hold 1e3: one of them would head every dot-product list)."""
    N, k = 300, 10
    x = make_data(N, D, 31 + D)
    base = on_device(x)
    pairs, _, _ = planted(N)
    good = subset_pool(N, 4)
    for metric in ("dot", "cosine"):
        qids = query_ids(N, 17, 8)
        ref, bar = reference(x[qids % N], x, metric)
        # a bad pool id at each end (the pool stays sorted unique)
        pool = np.concatenate(([-2], good, [N + 3])).astype(np.int64)
        ids, sc = run(base, qids, pool, metric, k, True, expect_flag=True)
        check(("pool", D, metric), ids, sc, ref, bar, good, [int(i) for i in qids], pairs, metric)
        # a bad query id in the middle and a negative one
        bad = qids.copy()
        bad[3], bad[9] = N + 5, -1
        own = [None if j in (3, 9) else int(i) for j, i in enumerate(bad)]
        ids, sc = run(base, bad, None, metric, k, True, expect_flag=True)
        check(("query", D, metric), ids, sc, ref, bar, np.arange(N, dtype=np.int64), own, pairs, metric)
        # and the flag is gone once raised: a clean call passes
        ids, sc = run(base, qids, good, metric, k, True)
        check(("clean", D, metric), ids, sc, ref, bar, good, [int(i) for i in qids], pairs, metric)


def test_large_row_offsets_are_64_bit():
    """A candidate whose byte offset is past 2^32 (row 2^23 + 5 of a D = 128 table: 4 GB + 2.5 KB): found, with its row's bits."""
    D, N = 128, (1 << 23) + 16
    base = torch.zeros(N, D, dtype=torch.float32, device="cuda:0")
    rng = np.random.default_rng(3)
    v = rng.standard_normal((4, D)).astype(np.float32)
    rows = np.array([7, (1 << 23) + 5, (1 << 23) + 9, N - 1], dtype=np.int64)
    base[torch.from_numpy(rows).cuda()] = torch.from_numpy(v).cuda()
    pool = np.unique(np.concatenate((rows, np.arange(0, N, 1 << 16), np.arange((1 << 23) - 3, (1 << 23) + 12)))).astype(np.int64)
    ids, sc = run(base, v, pool, "dot", 1, False)
    assert ids[:, 0].tolist() == rows.tolist()
    ref, bar = reference(v, v, "dot")
    assert (np.abs(sc[:, 0] - np.diag(ref)) <= np.diag(bar)).all()
    ids, sc = run(base, rows[1:3].copy(), pool, "cosine", 2, False)
    assert ids[:, 0].tolist() == rows[1:3].tolist() and (np.abs(sc[:, 0] - 1.0) <= 4 * gamma(D) + 8 * U).all()
