"""tests/mmr_ref.py (the float64 restatement the GPU tests of csrc/diversify.hip compare against) against a brute-force statement in plain
Python on tiny lists, and its rules one by one: lam = 1 is the sorted deduplicated list, exact ties go to the lower id and then the lower
position, absent entries are never picked."""
import math

import pytest
import torch

from tests import mmr_ref


def brute(ids, rel, table, metric, lam, K, M):
    """The definition read aloud: Python floats (float64), one entry at a time."""
    n_rows, D = len(table), len(table[0])
    lam = float(torch.tensor(lam, dtype=torch.float32))
    oml = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(lam, dtype=torch.float32))

    def sim(a, b):
        dot = math.fsum(x * y for x, y in zip(table[a], table[b]))
        if metric == 0:
            return dot
        na, nb = (1.0 / max(math.sqrt(math.fsum(x * x for x in table[i])), 1e-8) for i in (a, b))
        return (dot * na) * nb

    present = [p for p in range(len(ids)) if 0 <= ids[p] < n_rows and not math.isnan(rel[p])]
    short = sorted(present, key=lambda p: (-rel[p], ids[p], p))[:M]
    picks = []
    while short and len(picks) < K:
        if not picks:
            best, value, ms = short[0], lam * rel[short[0]], 0.0
        else:
            best = None
            for p in short:
                if p in [q for q, _, _ in picks] or ids[p] in [ids[q] for q, _, _ in picks]:
                    continue
                m = max(sim(ids[p], ids[q]) for q, _, _ in picks)
                v = lam * rel[p] - oml * m
                if math.isnan(v):
                    continue
                if best is None or v > value or (v == value and (ids[p], p) < (ids[best], best)):
                    best, value, ms = p, v, m
            if best is None:
                break
        picks.append((best, value, ms))
    return picks


def dyadic_case(seed, n_rows=12, D=8, n=14):
    """Everything exact in both statements: table entries small integers / 8, relevances multiples of 1 / 64."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randint(-4, 5, (n_rows, D), generator=g).to(torch.float32) / 8
    ids = torch.randint(-1, n_rows + 1, (n,), generator=g)               # some ids outside the table, some repeated
    rel = torch.randint(0, 24, (n,), generator=g).to(torch.float32) / 64       # many exact ties
    rel[torch.rand(n, generator=g) < 0.15] = float("nan")
    return table, ids, rel


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("lam", (0.0, 0.25, 0.5, 1.0))
def test_the_restatement_is_the_brute_force(metric, lam):
    for seed in range(12):
        table, ids, rel = dyadic_case(seed)
        for K, M in ((1, 1), (3, 3), (3, 8), (8, 8), (14, 14)):
            got = mmr_ref.mmr_row(ids, rel, table, metric, lam, K, M)
            want = brute(ids.tolist(), rel.tolist(), table.tolist(), metric, lam, K, M)
            n = len(want)
            assert got["positions"][:n] == [p for p, _, _ in want] and got["positions"][n:] == [-1] * (K - n), (seed, K, M)
            assert got["ids"][:n] == [int(ids[p]) for p, _, _ in want] and got["ids"][n:] == [-1] * (K - n)
            assert got["rel"][:n] == [float(rel[p]) for p, _, _ in want]
            for j, (_, value, ms) in enumerate(want):
                tol = 0.0 if metric == 0 else 1e-12                     # (dot on dyadic inputs is exact in any order of summation)
                assert abs(got["value"][j] - value) <= tol and abs(got["max_sim"][j] - ms) <= tol, (seed, K, M, j)
            assert all(x == float("-inf") for f in ("rel", "value", "max_sim") for x in got[f][n:])


def test_lam_1_is_the_sorted_deduplicated_list():
    for seed in range(8):
        table, ids, rel = dyadic_case(seed, n=20)
        M = 16
        short = mmr_ref.shortlist(ids, rel, table.shape[0], M).tolist()
        seen, want = set(), []
        for p in short:
            if int(ids[p]) not in seen:
                seen.add(int(ids[p]))
                want.append(p)
        for metric in (0, 1):
            got = mmr_ref.mmr_row(ids, rel, table, metric, 1.0, M, M)
            assert got["positions"][:len(want)] == want and got["positions"][len(want):] == [-1] * (M - len(want))
            assert got["value"][:len(want)] == [float(rel[p]) for p in want] == got["rel"][:len(want)]


def test_exact_ties_go_to_the_lower_id_then_the_lower_position():
    table = torch.zeros(6, 8)
    table[:, 0] = 1.0                                                    # every row the same: every similarity is 1, every v ties
    ids = torch.tensor([4, 2, 5, 2, 3, 1])
    rel = torch.full((6,), 0.5)
    got = mmr_ref.mmr_row(ids, rel, table, 0, 0.5, 6, 6)
    # the shortlist order is (id, position): 1 @5, 2 @1, 2 @3, 3 @4, 4 @0, 5 @2; the second 2 is a duplicate of a picked id
    assert got["ids"] == [1, 2, 3, 4, 5, -1] and got["positions"] == [5, 1, 4, 0, 2, -1]
    assert got["value"][:5] == [0.25, -0.25, -0.25, -0.25, -0.25] and got["max_sim"][:5] == [0.0, 1.0, 1.0, 1.0, 1.0]
    # two entries of one id and one relevance: the lower position leads the shortlist, and is pick 1
    got = mmr_ref.mmr_row(torch.tensor([3, 3, 0]), torch.tensor([0.75, 0.75, 0.5]), table, 1, 0.5, 3, 3)
    assert got["positions"] == [0, 2, -1] and got["ids"] == [3, 0, -1]
    # a cut shortlist keeps the lower id of an exact tie at its end
    got = mmr_ref.mmr_row(torch.tensor([5, 4, 3]), torch.tensor([0.5, 0.5, 0.75]), table, 0, 1.0, 2, 2)
    assert got["ids"] == [3, 4]


def test_absent_entries_are_never_picked():
    table, _, _ = dyadic_case(3)
    ids = torch.tensor([-1, 12, 5, 7, 1 << 40, 5, 2])
    rel = torch.tensor([9.0, 9.0, 0.25, float("nan"), 9.0, 0.5, 0.125])
    for metric in (0, 1):
        for lam in (0.0, 0.5, 1.0):
            got = mmr_ref.mmr_row(ids, rel, table, metric, lam, 7, 7)
            assert sorted(p for p in got["positions"] if p >= 0) == [5, 6] and got["positions"][0] == 5       # (5 @2 is a duplicate of 5 @5)
    assert mmr_ref.mmr_row(ids[:2], rel[:2], table, 0, 0.5, 2, 2)["ids"] == [-1, -1]
    assert mmr_ref.mmr_row(ids[:0], rel[:0], table, 0, 0.5, 2, 2)["ids"] == [-1, -1]


def test_the_bound_is_positive_and_margins_are_reported():
    g = torch.Generator().manual_seed(0)
    table = torch.randn(50, 64, generator=g)
    ids, rel = torch.randperm(50, generator=g)[:30], torch.rand(30, generator=g)
    for metric in (0, 1):
        got = mmr_ref.mmr_row(ids, rel, table, metric, 0.7, 8, 16, with_bound=True)
        assert len(got["margins"]) == 7 and all(e > 0 for e in got["e_value"]) and got["e_max_sim"][0] == 0.0
        assert all(0 < e < (1e-3 if metric == 0 else 1e-5) for e in got["e_max_sim"][1:])
