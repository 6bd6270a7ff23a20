"""The data-parallel merge and optimizer at worlds of 1 to 16, on ONE GPU in one process, through the C ABI.

What the all-gather of a data-parallel step delivers is a flat buffer whose layout is written down in amid_amd.dist.packed_rows and
HipMergeBackend.chunk_rows; make_world() builds it on the host for any world size, next to a plain restatement of what the kernels must
compute from it (who holds an id, the rows of equal ids summed strictly in rank order, the dense parts summed in rank order), and hands it
to amid_optimizer_step_gathered_f32, to HipMergeBackend.merge_packed and to the padding kernels.  Every padding slot of the buffer holds
NaN, so an output without a NaN proves that no padding was read.

Tolerances: bit equality wherever both sides run the same additions in the same order; the recursive-summation bound
(world - 1) * 2^-24 * sum |term| against float64; the bars of tests/test_gpu_kernels.py for the same arithmetic elsewhere (2e-6 relative
for the segment reduce, 2e-6 / 5e-6 absolute for the lazy Adam trajectories, 1e-6 for the dense Adam)."""
import os
import socket
from types import SimpleNamespace

import pytest
import torch

from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from amid_amd._lib import lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def step_state(L, step, lr=5e-4):
    import ctypes
    n = L.value("amid_step_state_bytes")
    host = (ctypes.c_ubyte * n)()
    L.call("amid_step_state_pack", ctypes.addressof(host), 0, step, lr, 0.9, 0.999, 1e-8)
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fabricated world
def _values(g, flavour, hold, width):
    """[world, N, width] fp32 terms; hold [world, N]: which (rank, column) pairs exist (the others are never summed).
    exact: small integers times 2^-3 -- every fp32 sum of up to 16 of them is exact in any order;
    order: per element 2^24, 1 and -2^24 (either sign) dealt to three of the holders, randn for the others -- (2^24 + 1) - 2^24 = 0 but
           (2^24 - 2^24) + 1 = 1, so the rank-ordered fp32 sum differs from other orders; columns with fewer than three holders: randn;
    plain: randn."""
    world, N = hold.shape
    if flavour == "exact":
        return torch.randint(-8, 9, (world, N, width), generator=g).float() * 0.125
    out = torch.randn(world, N, width, generator=g)
    if flavour == "order":
        col = torch.arange(width)
        for n in range(N):
            holders = hold[:, n].nonzero().flatten()
            if holders.numel() < 3:
                continue
            pick = holders[torch.rand(holders.numel(), width, generator=g).argsort(0)[:3]]          # [3, width]: three distinct holders per element
            big = 16777216.0 * (torch.randint(0, 2, (width,), generator=g).float() * 2 - 1)
            out[pick[0], n, col] = big
            out[pick[1], n, col] = 1.0
            out[pick[2], n, col] = -big
    else:
        assert flavour == "plain", flavour
    return out


def _rank_ordered(terms, hold, dtype):
    """[N, width]: per column the terms of its holders added strictly in rank order, one plain addition of `dtype` per holder (no sum())."""
    acc = torch.zeros(terms.shape[1:], dtype=dtype)
    started = torch.zeros(hold.shape[1], 1, dtype=torch.bool)
    for r in range(terms.shape[0]):
        h = hold[r][:, None]
        row = terms[r].to(dtype)
        acc = torch.where(h & started, acc + row, torch.where(h, row, acc))
        started = started | h
    return acc


def make_world(world, umax, D, n_rows, n_dense, spec, seed):
    """The gathered buffer of a data-parallel step, as dist.packed_rows / HipMergeBackend.chunk_rows lay it out, with its restatement.

    Chunk r = [id_rows = ceil(umax / D) rows holding umax int32 ids: rank r's ascending unique real ids, then the sentinel n_rows |
    umax gradient rows | at dense_off = (id_rows + umax) * D the rank's dense gradient, n_dense floats], chunk_floats = chunk_rows * D.
    NaN in every gradient row past the rank's count, in the tail of the id rows and in the slack behind the dense part.
    spec: lists = callable(generator) -> `world` ascending unique int64 id tensors of at most umax entries; flavour = "exact" | "order" |
    "plain" (_values); dense = "gather" (the dense part rides in the chunk) | "allreduce" (chunks without one, dense_off = -1)."""
    g = torch.Generator().manual_seed(seed)
    lists = spec["lists"](g)
    assert len(lists) == world and all(l.numel() <= umax for l in lists)
    in_chunk = spec["dense"] == "gather"
    id_rows = (umax + D - 1) // D
    rows = id_rows + umax
    chunk_floats = (rows + ((n_dense + D - 1) // D if in_chunk else 0)) * D
    dense_off = rows * D if in_chunk else -1
    assert chunk_floats % 4 == 0 and (dense_off < 0 or dense_off % 4 == 0)          # what the entry point demands
    hold = torch.zeros(world, n_rows, dtype=torch.bool)
    for r, ids in enumerate(lists):
        assert ids.numel() == 0 or (int(ids.min()) >= 0 and int(ids.max()) < n_rows and bool((ids[1:] > ids[:-1]).all()))
        hold[r, ids] = True
    terms = _values(g, spec["flavour"], hold, D)
    dense = _values(g, spec["flavour"], torch.ones(world, 1, dtype=torch.bool), n_dense)[:, 0]
    buf = torch.full((world, chunk_floats), NAN)
    bi = buf.view(torch.int32)
    for r, ids in enumerate(lists):
        k = ids.numel()
        bi[r, :k] = ids.to(torch.int32)
        bi[r, k:umax] = n_rows
        buf[r, id_rows * D: (id_rows + k) * D] = terms[r, ids].reshape(-1)
        if in_chunk:
            buf[r, dense_off: dense_off + n_dense] = dense[r]
    uniq = hold.any(0).nonzero().flatten()
    dense32, dense64 = dense[0].clone(), dense[0].double()
    for r in range(1, world):
        dense32 = dense32 + dense[r]
        dense64 = dense64 + dense[r].double()
    return SimpleNamespace(world=world, umax=umax, D=D, n_rows=n_rows, n_dense=n_dense, id_rows=id_rows, rows=rows, chunk_floats=chunk_floats,
                           dense_off=dense_off, in_chunk=in_chunk, buf=buf.reshape(-1), lists=lists, hold=hold, uniq=uniq,
                           holders={int(x): hold[:, x].nonzero().flatten().tolist() for x in uniq},
                           row32=_rank_ordered(terms, hold, torch.float32)[uniq], row64=_rank_ordered(terms, hold, torch.float64)[uniq],
                           dense32=dense32, dense64=dense64, dense_abs=dense.double().abs().sum(0),
                           row_abs=_rank_ordered(terms.abs(), hold, torch.float64)[uniq], row_terms=hold.sum(0)[uniq])


def _pick(g, pool, k):
    return pool[torch.randperm(pool.numel(), generator=g)[:k]].sort().values


def _lists_one(n_rows):
    return lambda g: [_pick(g, torch.arange(n_rows), 5)]


def _lists_pad_id(n_rows):
    return lambda g: [torch.tensor([n_rows - 1]), torch.tensor([n_rows - 1])]


def _lists_ragged3(n_rows):
    def f(g):
        a = _pick(g, torch.arange(n_rows - 1), 7)
        return [a, torch.zeros(0, dtype=torch.long), torch.cat((a[[1, 5]], torch.tensor([n_rows - 1]))).sort().values]
    return f


def _lists_same(n_rows, world, k):
    def f(g):
        a = _pick(g, torch.arange(n_rows), k)
        return [a.clone() for _ in range(world)]
    return f


def _lists_disjoint(n_rows, world, k):
    def f(g):
        p = torch.randperm(n_rows, generator=g)
        return [p[r * k: (r + 1) * k].sort().values for r in range(world)]
    return f


def _lists_planted(n_rows, world, umax, plants, counts=None):
    """plants: [(ranks, how many ids)]: ids held by exactly those ranks; every rank then draws from the remaining ids up to its count
    (random overlap).  counts: per-rank totals (default: random in [its planted ids, umax])."""
    def f(g):
        p = torch.randperm(n_rows, generator=g)
        mine, at = [[] for _ in range(world)], 0
        for ranks, k in plants:
            for r in ranks:
                mine[r].append(p[at: at + k])
            at += k
        rest = p[at:]
        out = []
        for r in range(world):
            own = torch.cat(mine[r]) if mine[r] else torch.zeros(0, dtype=torch.long)
            total = max(own.numel(), counts[r] if counts is not None else int(torch.randint(0, umax + 1, (1,), generator=g)))
            out.append(torch.cat((own, _pick(g, rest, total - own.numel()))).sort().values)
        return out
    return f


def _lists_w9(n_rows):
    return _lists_planted(n_rows, 9, 33, [((0, 8), 5), ((4, 8), 5), (tuple(range(9)), 6)])


def _lists_w16(n_rows):
    counts = [300, 17, 120, 64, 299, 0, 1, 200, 33, 150, 250, 8, 77, 129, 256, 100]       # ragged from 0 to 300
    return _lists_planted(n_rows, 16, 300, [((3, 7, 15), 8), ((15,), 8)], counts)


# world, umax, n_rows, n_dense, lists.  n_rows of a few hundred reaches every branch; the disjoint case needs 8 x 129 distinct ids.
# n_dense = 4099 in two cases: the scalar tail of the dense role.
CASES = {
    "w1_full": (1, 5, 300, 4100, _lists_one(300)),
    "w2_pad_id": (2, 1, 300, 4100, _lists_pad_id(300)),
    "w3_ragged": (3, 7, 300, 4099, _lists_ragged3(300)),
    "w8_same64": (8, 64, 300, 4100, _lists_same(300, 8, 64)),
    "w8_disjoint129": (8, 129, 1100, 4100, _lists_disjoint(1100, 8, 129)),
    "w9_planted": (9, 33, 300, 4100, _lists_w9(300)),
    "w16_ragged300": (16, 300, 700, 4099, _lists_w16(700)),
    "w16_same16": (16, 16, 300, 4100, _lists_same(300, 16, 16)),
}
FLAVOURS = ("exact", "order", "plain")
T_NOW = 300            # the step of the one-launch cases: stamps from 1 to 298 lag by up to 298 steps, inside and beyond the 256-entry coefficient table


def test_make_world_restates_the_cases_it_promises():
    """The fabricated worlds hold what the table of cases says (no kernel involved): the ownership patterns, the ragged counts, the
    order-sensitive sums."""
    w = make_world(9, 33, 64, 300, 4100, dict(lists=_lists_w9(300), flavour="order", dense="gather"), 1)
    sets = {tuple(v) for v in w.holders.values()}
    assert (0, 8) in sets and (4, 8) in sets and tuple(range(9)) in sets
    assert not torch.equal(w.dense32.double(), w.dense64) and not torch.equal(w.row32.double(), w.row64)      # the order matters
    w = make_world(16, 300, 64, 700, 4099, dict(lists=_lists_w16(700), flavour="exact", dense="gather"), 2)
    sets = [tuple(v) for v in w.holders.values()]
    assert sets.count((3, 7, 15)) >= 8 and sets.count((15,)) >= 8             # (the planted ids, and what the random draws add)
    assert sorted(l.numel() for l in w.lists)[0] == 0 and max(l.numel() for l in w.lists) == 300
    assert torch.equal(w.dense32.double(), w.dense64) and torch.equal(w.row32.double(), w.row64)              # exact in any order
    assert any(len(v) > 1 and v[0] != 0 for v in w.holders.values())                                          # a first owner that is not rank 0
    w = make_world(3, 7, 128, 300, 4099, dict(lists=_lists_ragged3(300), flavour="plain", dense="allreduce"), 3)
    assert [l.numel() for l in w.lists] == [7, 0, 3] and w.dense_off == -1 and w.chunk_floats == (1 + 7) * 128
    assert bool(torch.isnan(w.buf).any())


def make_state(w, seed, t):
    """Parameters, moments and stamps; the table and its moments carry one extra row at index n_rows (where the sentinel points) holding a
    canary, so a write to the sentinel row is caught inside the allocation."""
    g = torch.Generator().manual_seed(seed)
    n, R, D = w.n_dense, w.n_rows, w.D
    st = dict(p=torch.randn(n, generator=g), m=0.1 * torch.randn(n, generator=g), v=0.01 * torch.rand(n, generator=g),
              table=torch.randn(R + 1, D, generator=g), tm=0.1 * torch.randn(R + 1, D, generator=g), tv=0.01 * torch.rand(R + 1, D, generator=g))
    kind = torch.randint(0, 3, (R + 1,), generator=g)
    last = torch.where(kind == 0, torch.zeros(R + 1, dtype=torch.long),
                       torch.where(kind == 1, torch.full((R + 1,), t - 1), torch.randint(1, t - 1, (R + 1,), generator=g)))
    for k in ("table", "tm", "tv"):
        st[k][R] = 12345.0
    last[R] = -7
    st["last"] = last.to(torch.int32)
    return st


STATE_KEYS = ("p", "m", "v", "table", "tm", "tv", "last")


def run_gathered(L, w, st0, t, g0, lr=5e-4):
    """amid_optimizer_step_gathered_f32 on a copy of the state -> (state after, g after)."""
    d = {k: v.clone().cuda() for k, v in st0.items()}
    g = g0.clone().cuda()
    buf = w.buf.cuda()
    ss = step_state(L, t, lr)
    L.call("amid_optimizer_step_gathered_f32", d["p"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), g.data_ptr(), w.n_dense,
           d["table"].data_ptr(), d["tm"].data_ptr(), d["tv"].data_ptr(), d["last"].data_ptr(), buf.data_ptr(), w.world, w.umax, w.chunk_floats,
           w.id_rows, w.dense_off, w.D, w.n_rows, 1.0 / w.world, ss.data_ptr(), stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}, g.cpu()


def run_restated(L, w, st0, t, lr=5e-4):
    """amid_optimizer_step_f32 on a copy of the state, fed the restatement: the unique ids, the rank-ordered fp32 row sums and dense sum."""
    d = {k: v.clone().cuda() for k, v in st0.items()}
    g, ids, rows = w.dense32.cuda(), w.uniq.to(torch.int32).cuda(), w.row32.contiguous().cuda()
    nu = torch.tensor([w.uniq.numel()], dtype=torch.int32, device="cuda")
    ss = step_state(L, t, lr)
    L.call("amid_optimizer_step_f32", d["p"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), g.data_ptr(), w.n_dense, d["table"].data_ptr(),
           d["tm"].data_ptr(), d["tv"].data_ptr(), d["last"].data_ptr(), ids.data_ptr(), nu.data_ptr(), w.uniq.numel(), rows.data_ptr(), w.D,
           1.0 / w.world, ss.data_ptr(), stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("dense", ["gather", "allreduce"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("case", list(CASES))
def test_gathered_optimizer_equals_its_restatement(L, case, D, dense, flavour):
    """amid_optimizer_step_gathered_f32 over a fabricated world against amid_optimizer_step_f32 fed the host restatement.  Both kernels call the
    same adam_quad / replay_quad / fill_coef_table, so bit equality of every output is the claim that the gathered kernel applies every id
    once, by its first owner, with the right rows added in rank order, and sums the dense parts in rank order."""
    world, umax, n_rows, n_dense, lists = CASES[case]
    w = make_world(world, umax, D, n_rows, n_dense, dict(lists=lists, flavour=flavour, dense=dense), seed=1000 * world + umax + D)
    st0 = make_state(w, seed=world + D, t=T_NOW)
    g0 = torch.full((n_dense,), -777.0) if w.in_chunk else w.dense32           # allreduce: g pre-summed by the caller
    got, g = run_gathered(L, w, st0, T_NOW, g0)
    # the dense sum: the rank-ordered restatement to the bit, and inside the recursive-summation bound of the float64 sum
    assert torch.equal(g, w.dense32)
    bound = 1.01 * (world - 1) * 2.0 ** -24 * w.dense_abs
    assert bool(((g.double() - w.dense64).abs() <= bound).all())
    want = run_restated(L, w, st0, T_NOW)
    for k in STATE_KEYS:
        assert torch.equal(got[k], want[k]), (k, float((got[k].double() - want[k].double()).abs().max()))
    # rows in no list: untouched; the canary row: untouched; every applied id stamped with t; no NaN anywhere (no padding slot was read)
    idle = torch.ones(n_rows + 1, dtype=torch.bool)
    idle[w.uniq] = False
    for k in ("table", "tm", "tv", "last"):
        assert torch.equal(got[k][idle], st0[k][idle]), k
        assert torch.equal(got[k][n_rows], st0[k][n_rows]), k
    assert bool((got["last"][w.uniq] == T_NOW).all())
    assert bool(((got["table"][w.uniq] != st0["table"][w.uniq]).any(1)).all())        # ... and every applied id moved
    for k in STATE_KEYS:
        assert not bool(torch.isnan(got[k].float()).any()), k
    assert not bool(torch.isnan(g).any())
    # reproducible: a second launch from the same state gives the same bits
    again, g2 = run_gathered(L, w, st0, T_NOW, g0)
    assert torch.equal(g2, g) and all(torch.equal(again[k], got[k]) for k in STATE_KEYS)


@pytest.mark.parametrize("gap,tol", [(0, 2e-6), (700, 5e-6)])
def test_gathered_optimizer_trajectory_equals_dense_adam(L, gap, tol):
    """Six steps of a world of five whose id sets change per step (rows go idle and return) against orc.DenseAdam on the dense-equivalent
    gradient built from the restated fp32 sums; gap: idle steps between the third and the fourth step, beyond the 256-entry coefficient
    table.  Bars: those of test_lazy_adam_equals_dense_adam_with_idle_rows / ..._long_idle_gap_beyond_coefficient_table (the same replay
    arithmetic), on the rows about to be read and, after the flush, on the whole table; 1e-6 on the dense part (test_dense_adam_...)."""
    world, D, n_rows, umax, n_dense, lr = 5, 64, 40, 9, 68, 5e-3
    g = torch.Generator().manual_seed(17 + gap)
    tab0, p0 = torch.randn(n_rows, D, generator=g), torch.randn(n_dense, generator=g)
    P = {"t": tab0.clone(), "w": p0.clone()}
    opt = orc.DenseAdam(P, lr=lr)
    d = dict(p=p0.clone().cuda(), m=torch.zeros(n_dense, device="cuda"), v=torch.zeros(n_dense, device="cuda"),
             table=torch.cat((tab0, torch.full((1, D), 12345.0))).cuda(), tm=torch.zeros(n_rows + 1, D, device="cuda"),
             tv=torch.zeros(n_rows + 1, D, device="cuda"), last=torch.zeros(n_rows + 1, dtype=torch.int32, device="cuda"))
    gd = torch.zeros(n_dense, device="cuda")
    t = 0
    for k in range(6):
        if k == 3:
            for _ in range(gap):                   # the dense optimizer keeps moving the rows through their momentum
                opt.step(P, {"t": torch.zeros(n_rows, D)})
            t += gap
        t += 1
        lists = _lists_planted(n_rows, world, umax, [((1, 3), 2), ((0, 2, 4), 1)] if k % 2 else [((4,), 2)])
        w = make_world(world, umax, D, n_rows, n_dense, dict(lists=lists, flavour="plain", dense="gather"), seed=100 * gap + k)
        ss = step_state(L, t, lr)
        # the rows about to be gathered, caught up on a copy (the gathered kernel below replays the lag itself)
        c = {kk: d[kk].clone() for kk in ("table", "tm", "tv", "last")}
        ids = w.uniq.to(torch.int32).cuda()
        nu = torch.tensor([ids.numel()], dtype=torch.int32, device="cuda")
        L.call("amid_lazy_adam_catchup_f32", c["table"].data_ptr(), c["tm"].data_ptr(), c["tv"].data_ptr(), c["last"].data_ptr(), ids.data_ptr(),
               nu.data_ptr(), ids.numel(), D, ss.data_ptr(), stream())
        torch.cuda.synchronize()
        assert float((c["table"].cpu()[w.uniq] - P["t"][w.uniq]).abs().max()) < tol, ("pre-gather", t)
        scale = torch.tensor(1.0 / world, dtype=torch.float32)
        dense_grad = torch.zeros(n_rows, D)
        dense_grad[w.uniq] = w.row32 * scale
        opt.step(P, {"t": dense_grad, "w": w.dense32 * scale})
        buf = w.buf.cuda()
        L.call("amid_optimizer_step_gathered_f32", d["p"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), gd.data_ptr(), n_dense,
               d["table"].data_ptr(), d["tm"].data_ptr(), d["tv"].data_ptr(), d["last"].data_ptr(), buf.data_ptr(), world, umax, w.chunk_floats,
               w.id_rows, w.dense_off, D, n_rows, 1.0 / world, ss.data_ptr(), stream())
        torch.cuda.synchronize()
        assert float((d["table"].cpu()[w.uniq] - P["t"][w.uniq]).abs().max()) < tol, ("applied", t)
        assert float((d["p"].cpu() - P["w"]).abs().max()) < 1e-6, t
    ss = step_state(L, t, lr)
    L.call("amid_lazy_adam_flush_f32", d["table"].data_ptr(), d["tm"].data_ptr(), d["tv"].data_ptr(), d["last"].data_ptr(), n_rows, D, ss.data_ptr(),
           stream())
    torch.cuda.synchronize()
    assert float((d["table"].cpu()[:n_rows] - P["t"]).abs().max()) < tol
    assert float(d["table"][n_rows].min()) == 12345.0 == float(d["table"][n_rows].max()) and int(d["last"][n_rows]) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the eager form and the padding kernels, through a small real engine
ENG = dict(n_items=500, T=8, hid=32)
_ENGINES = {}


def engine(D):
    """One engine per D for the module, with a plan and a merge backend of 16 x 300 entries."""
    if D not in _ENGINES:
        from amid_amd.engine import SasrecEngine
        eng = SasrecEngine(ENG["n_items"], D, ENG["T"], ENG["hid"], device="cuda:0", lr=5e-4, seed=3)
        eng.load_state_dict(orc.random_params(orc.sasrec_param_shapes(ENG["n_items"], D, ENG["T"], ENG["hid"]), seed=5))
        eng._ensure_opt_state()
        _ENGINES[D] = (eng, eng.plan(2, ENG["T"], 2, need_grad=True), eng.merge_backend(16 * 300))
    return _ENGINES[D]


@pytest.mark.parametrize("with_dense", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_pad_packed_layout_and_flag(D, with_dense):
    """HipMergeBackend.pad_packed (amid_sparse_pad_f32 / amid_sparse_pad_sum_f32): ids then the sentinel, live rows then zero rows, the dense
    gradient at packed_rows(umax, D)[1] * D -- every byte, over a NaN-poisoned send buffer; a list that fits leaves the error word clear,
    one that does not raises AMID_FLAG_UMAX_EXCEEDED in it (and still writes nothing past its umax entries)."""
    from amid_amd.dist import packed_rows
    eng, pl, be = engine(D)
    umax, cap = 37, 64
    g = torch.Generator().manual_seed(D + with_dense)
    ids = torch.randperm(eng.n_rows, generator=g)[:cap].sort().values.to(torch.int32)
    rows = torch.randn(cap, D, generator=g)
    dg = torch.randn(eng.dense.numel, generator=g)
    idd, rd = ids.cuda(), rows.cuda()
    id_rows, prow = packed_rows(umax, D)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    try:
        for n in (0, 1, umax - 1, umax, umax + 3):
            eng.dense.grad.copy_(dg)
            nu = torch.tensor([n], dtype=torch.int32, device="cuda")
            chunk = be.chunk_rows(umax, eng.dense.grad if with_dense else None) * D
            be.send[: chunk + D].fill_(NAN)
            err.zero_()
            torch.cuda.synchronize()
            be.err = err
            send = be.pad_packed(idd, rd, nu, umax, dense=eng.dense.grad if with_dense else None)
            eng.sync()
            assert send.numel() == chunk and send.data_ptr() == be.send.data_ptr()
            out = be.send[: chunk + D].cpu()
            k = min(n, umax)
            want_ids = torch.cat((ids[:k], torch.full((umax - k,), eng.n_rows, dtype=torch.int32)))
            assert torch.equal(out.view(torch.int32)[:umax], want_ids), n
            assert bool(torch.isnan(out[umax: id_rows * D]).all())                         # the tail of the id rows is nobody's
            got_rows = out[id_rows * D: prow * D].view(umax, D)
            assert torch.equal(got_rows[:k], rows[:k]) and float(got_rows[k:].abs().max() if k < umax else 0.0) == 0.0, n
            if with_dense:
                assert torch.equal(out[prow * D: prow * D + dg.numel()], dg), n
                assert bool(torch.isnan(out[prow * D + dg.numel():]).all())                # the slack behind the dense part and beyond the chunk
            else:
                assert bool(torch.isnan(out[prow * D:]).all())
            assert int(err.item()) == (2 if n > umax else 0), n
    finally:
        be.err = None
        eng.dense.grad.zero_()
        torch.cuda.synchronize()


def _engine_world(D, world, flavour):
    """One of the fabricated worlds of the table above in the engine's own layout (its n_rows, its flat dense gradient)."""
    from amid_amd.dist import packed_rows
    eng, pl, be = engine(D)
    lists = {3: (7, _lists_ragged3(eng.n_rows)), 9: (33, _lists_w9(eng.n_rows)), 16: (300, _lists_w16(eng.n_rows))}[world]
    w = make_world(world, lists[0], D, eng.n_rows, eng.dense.numel, dict(lists=lists[1], flavour=flavour, dense="gather"), seed=7 * world + D)
    assert w.chunk_floats == be.chunk_rows(w.umax, eng.dense.grad) * D and (w.id_rows, w.rows) == packed_rows(w.umax, D)
    return eng, pl, be, w


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("world", [3, 9, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_merge_packed_with_dense_sum_on_fabricated_worlds(D, world, flavour):
    """HipMergeBackend.merge_packed(..., dense=grad, sum_dense=True) = amid_merge_sorted_lists_sum_i32 + the segment reduce: the merge against
    a stable sort of the concatenation (the assertions of test_merge_sorted_lists_matches_stable_sort), the dense sum to the bit of the
    rank-ordered restatement (the aligned path of the fixed-order sums: every slot of the flat buffer is padded to 4 floats), the merged
    rows against the float64 sums: on every flavour inside the bound that holds for an fp32 sum of k terms in ANY order,
    (k - 1) * 2^-24 * sum |term| per element; on plain and exact values also inside the segment reduce's bar (2e-6 relative to the largest
    magnitude of the sums, test_segreduce_matches_index_add); on exact values equal to them.  The order flavour is built to cancel --
    2^24 + 1 - 2^24 -- so its sums are of order 1 with terms of order 2^24: no fp32 summation, the strictly rank-ordered restatement
    included, lands within 2e-6 of those (measured on the first run: off by about 1 where the largest sum is 10), so there the bar would
    test the values, not the kernel; the summation bound is the claim that can be made."""
    eng, pl, be, w = _engine_world(D, world, flavour)
    recv = be.gather_buffer(world, w.umax, dense=eng.dense.grad)
    assert recv.numel() == w.buf.numel()
    recv.copy_(w.buf.cuda())
    eng.dense.grad.fill_(-777.0)
    be.pos_sorted.fill_(-1)
    torch.cuda.synchronize()
    ids, rows, nu = be.merge_packed(recv, world, w.umax, dense=eng.dense.grad, sum_dense=True)
    eng.sync()
    n = world * w.umax
    keys = torch.cat([torch.cat((l, torch.full((w.umax - l.numel(),), eng.n_rows, dtype=torch.long))) for l in w.lists])
    order = torch.sort(keys, stable=True).indices                                 # ties in rank order
    chunk_rows = w.chunk_floats // D
    assert torch.equal(be.pos_sorted[:n].cpu().long(), w.id_rows + (order // w.umax) * chunk_rows + order % w.umax)
    wu, wc = torch.unique(keys, return_counts=True)
    has_pad = bool((keys == eng.n_rows).any())
    U = int(nu.item())
    assert U == wu.numel() - (1 if has_pad else 0) == w.uniq.numel()
    assert torch.equal(ids[:wu.numel()].cpu().long(), wu)
    assert torch.equal(be.seg_off[: wu.numel() + 1].cpu().long(), torch.cat((torch.zeros(1, dtype=torch.long), wc.cumsum(0))))
    assert torch.equal(be.seg_of[:n].cpu().long(), torch.repeat_interleave(torch.arange(wu.numel()), wc))
    assert torch.equal(eng.dense.grad.cpu(), w.dense32)
    got = rows[:U].cpu()
    assert not bool(torch.isnan(got).any())
    bound = 1.01 * (w.row_terms - 1).clamp(min=0)[:, None] * 2.0 ** -24 * w.row_abs
    err = (got.double() - w.row64).abs()
    print(f"merge_packed D={D} world={world} {flavour}: max |row - float64| {float(err.max()):.3e}, largest sum {float(w.row64.abs().max()):.3e}, "
          f"worst error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    if flavour != "order":
        assert float(err.max() / w.row64.abs().max()) < 2e-6
    if flavour == "exact":
        assert torch.equal(got.double(), w.row64)
    eng.dense.grad.zero_()
    torch.cuda.synchronize()


@pytest.mark.parametrize("world", [3, 9, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_eager_and_gathered_optimizers_agree_to_the_bit_on_exact_values(D, world):
    """The two forms of the data-parallel optimizer from equal starting state: merge + segment reduce + enqueue_optimizer(sparse=merged) and
    the one launch over the gathered chunks.  On exact values every summation order gives the same sums, so the states must match to the
    bit; on arbitrary values nothing promises that (the segment reduce adds a run that crosses a chunk border as partial + partial)."""
    eng, pl, be, w = _engine_world(D, world, "exact")
    g = torch.Generator().manual_seed(world + D)
    fp = eng.dense
    init = dict(table=torch.randn(eng.n_rows, D, generator=g), tm=0.1 * torch.randn(eng.n_rows, D, generator=g),
                tv=0.01 * torch.rand(eng.n_rows, D, generator=g), p=torch.randn(fp.numel, generator=g), m=0.1 * torch.randn(fp.numel, generator=g),
                v=0.01 * torch.rand(fp.numel, generator=g),
                last=torch.randint(0, 3, (eng.n_rows,), generator=g).to(torch.int32) * torch.randint(1, T_NOW, (eng.n_rows,), generator=g).to(torch.int32) // 2)
    slots = dict(table=eng.table, tm=eng.table_m, tv=eng.table_v, p=fp.data, m=fp.m, v=fp.v, last=eng.table_last)
    saved = {k: t.clone() for k, t in slots.items()}
    step0, scale0 = eng.step, eng.grad_scale
    out = {}
    try:
        recv = be.gather_buffer(world, w.umax, dense=fp.grad)
        for form in ("eager", "gathered"):
            for k, t in slots.items():
                t.copy_(init[k])
            recv.copy_(w.buf.cuda())
            fp.grad.fill_(-777.0)
            torch.cuda.synchronize()
            eng.set_step(T_NOW)
            eng.grad_scale = 1.0 / world
            if form == "eager":
                merged = be.merge_packed(recv, world, w.umax, dense=fp.grad, sum_dense=True)
                eng.enqueue_optimizer(pl, sparse=merged)
            else:
                eng.enqueue_optimizer_gathered(be, recv, world, w.umax, dense_in_chunk=True)
            eng.sync()
            out[form] = {k: t.cpu().clone() for k, t in slots.items()}
            out[form]["g"] = fp.grad.cpu().clone()
        for k in out["eager"]:
            assert torch.equal(out["eager"][k], out["gathered"][k]), k
            assert not bool(torch.isnan(out["eager"][k].float()).any()), k
        assert bool((out["gathered"]["last"][w.uniq] == T_NOW).all())
    finally:
        for k, t in slots.items():
            t.copy_(saved[k])
        fp.grad.zero_()
        eng.grad_scale = scale0
        eng.set_step(step0)
        torch.cuda.synchronize()


def test_gather_buffer_refuses_what_it_cannot_hold():
    eng, pl, be = engine(64)
    assert be.capacity == 4800 and be.MAX_WORLD == 16
    assert be.gather_buffer(16, 300).numel() == 16 * (5 + 300) * 64
    assert be.gather_buffer(16, 300, dense=eng.dense.grad).numel() == 16 * be.chunk_rows(300, eng.dense.grad) * 64
    with pytest.raises(ValueError):
        be.gather_buffer(16, 301)                      # world * umax > capacity
    with pytest.raises(ValueError):
        be.gather_buffer(5, 961)
    with pytest.raises(ValueError):
        be.gather_buffer(17, 8, dense=eng.dense.grad)      # more dense parts than the buffer was sized for


# ---------------------------------------------------------------------------------------------------------------------------------------
# a bound umax that is too small: AMID_FLAG_UMAX_EXCEEDED on every path of train_step_dp
OVR = dict(n_items=600, D=128, T=50, hid=32, B=12, seed=23, lr=1e-3)
# form: "pair" = graph A | all-gather | graph B (two steps on batch A capture the pair, the third replays it on batch B), "eager" =
# use_graph=False.  fused / fused_opt pick the packing tail of graph A: the fifteen-launch step's amid_grad_tail_pack_f32, the folded
# step's amid_grad_tail_live_dp_f32, and amid_grad_tail_live_dp1_f32 (the folded step's tail as one launch).
OVERRUNS = {
    "pair-pack-gather": dict(form="pair", dense="gather", fused=False, fused_opt=True, tail="amid_grad_tail_pack_f32"),
    "pair-pack-allreduce": dict(form="pair", dense="allreduce", fused=False, fused_opt=True, tail="amid_grad_tail_pack_f32"),
    "pair-live_dp-allreduce": dict(form="pair", dense="allreduce", fused=True, fused_opt=False, tail="amid_grad_tail_live_dp_f32"),
    "pair-live_dp1-gather": dict(form="pair", dense="gather", fused=True, fused_opt=True, tail="amid_grad_tail_live_dp1_f32"),
    "eager-gather": dict(form="eager", dense="gather", fused=True, fused_opt=True, tail="amid_sparse_pad_f32"),
    "eager-d64": dict(form="eager", dense="gather", fused=True, fused_opt=True, tail="amid_sparse_pad_f32", D=64, T=20),
}


def _overrun_batches(c):
    """Batch A draws every id from 6 items, batch B from a few hundred."""
    out = []
    for seed, hi in ((900, 7), (901, c["n_items"] - 1)):
        g = torch.Generator().manual_seed(seed)
        b = orc.synthetic_batch(c["B"], c["T"], c["n_items"] - 1, pad_id=c["n_items"] - 1, neg=1, seed=seed)
        b["seq_d1"] = torch.randint(1, hi, (c["B"], c["T"]), generator=g)
        b["seq_d2"] = torch.randint(1, hi, (c["B"], c["T"]), generator=g)
        b["i_node"] = torch.randint(1, hi, (c["B"],), generator=g)
        b["neg_samples"] = torch.randint(1, hi, (c["B"], 1), generator=g)
        out.append(b)
    return out


def _uniques(b):
    return int(torch.unique(torch.cat([b[k].reshape(-1) for k in ("i_node", "neg_samples", "seq_d1", "seq_d2")])).numel())


def _overrun_scenario(form, dense, fused, fused_opt, tail, D=None, T=None):
    from amid_amd._lib import lib
    from amid_amd.dist import SparseDenseExchange
    from amid_amd.engine import SasrecEngine
    c = dict(OVR, D=D or OVR["D"], T=T or OVR["T"])
    P = orc.random_params(orc.sasrec_param_shapes(c["n_items"], c["D"], c["T"], c["hid"]), seed=9)
    eng = SasrecEngine(c["n_items"], c["D"], c["T"], c["hid"], device="cuda:0", lr=c["lr"], seed=c["seed"])
    eng.FUSED_TAIL_DP, eng.FUSED_OPT = fused, fused_opt
    eng.load_state_dict(P)
    pl = eng.plan(c["B"], c["T"], 2, need_grad=True)
    # capacity = the plan's index count: the kept and the overrunning rows of a step (at most n_idx) stay inside the backend's send buffer
    be = eng.merge_backend(pl.shape.n_idx)
    ex = SparseDenseExchange(be, host_staging=True, always=True)
    A, Bb = _overrun_batches(c)
    umax = (_uniques(A) + 63) // 64 * 64
    res = dict(umax=umax, uniq_a=_uniques(A), uniq_b=_uniques(Bb), n_idx=pl.shape.n_idx, send=be.send.numel(), steps=[])
    packed = [eng.pack_batch(pl, *(b[k].cuda() for k in ("i_node", "neg_samples", "seq_d1", "seq_d2", "label", "domain_id"))) for b in (A, A, Bb)]
    eng.set_input_pool(pl, torch.stack(packed))
    if form == "pair":
        eng.capture_local_grads(pl)
    L = lib()
    calls, orig = [], L.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    L.call = spy
    try:
        for k in range(len(packed)):
            del calls[:]
            eng.train_step_dp(pl, ex, use_graph=form == "pair", umax=umax, dense=dense)
            eng.sync()
            step = dict(calls=list(calls), n_uniq=int(pl.n_uniq.item()), flag=int(pl.err.item()), raised=None)
            try:
                eng.check_index_error(pl)
            except RuntimeError as e:
                step["raised"] = str(e)
            res["steps"].append(step)
    finally:
        L.call = orig
    res["pairs"] = len(getattr(pl, "dp_graphs", {}))
    res["tail2"] = bool(pl.tail2)
    return res


def _overrun_worker(port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        torch.cuda.set_device(0)
        q.put({name: _overrun_scenario(**kw) for name, kw in OVERRUNS.items()})
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def overruns():
    """Every scenario of OVERRUNS in ONE spawned child: a world of one with always=True runs the whole exchange (gloo collectives staged
    through the host); the pytest process itself never initialises a process group."""
    import queue
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_overrun_worker, args=(port, q))
    p.start()
    out = None
    while out is None:
        try:
            out = q.get(timeout=2)
        except queue.Empty:
            assert p.exitcode in (None, 0), f"the worker process failed: {p.exitcode}"
            assert p.is_alive() or not q.empty(), "the worker process ended without a result"
    p.join(60)
    assert p.exitcode == 0
    return out


@pytest.mark.parametrize("name", list(OVERRUNS))
def test_a_too_small_umax_raises_on_every_path(overruns, name):
    """train_step_dp's promise: a step that finds more unique rows than its umax raises AMID_FLAG_UMAX_EXCEEDED through check_index_error --
    from the three packing tails of graph A and (since this test) from the eager step's padding launch; a step whose bound holds leaves
    the flag clear; the eager step's launch list holds ONE padding launch and nothing that was added for the flag."""
    kw, r = OVERRUNS[name], overruns[name]
    print(name, {k: v for k, v in r.items() if k != "steps"}, [(len(s["calls"]), s["n_uniq"], s["flag"]) for s in r["steps"]])
    assert r["uniq_a"] <= r["umax"] < r["uniq_b"] and r["umax"] % 64 == 0
    *held, over = r["steps"]
    for s in held:
        assert s["n_uniq"] <= r["umax"] and s["flag"] == 0 and s["raised"] is None, s
    assert over["n_uniq"] > r["umax"]
    assert over["flag"] & 2 and over["raised"] is not None and "umax" in over["raised"], "did not raise"
    if kw["form"] == "pair":
        assert r["pairs"] == 1 and r["tail2"] == kw["fused"]
        assert kw["tail"] in held[0]["calls"] and held[0]["calls"].count(kw["tail"]) == 1      # (the first step captures the pair: graph A's tail)
        assert [c for c in over["calls"] if not c.startswith("amid_graph_launch")] == ["amid_optimizer_step_gathered_f32"]
    else:
        assert r["pairs"] == 0
        for s in r["steps"]:
            assert sum(c.startswith("amid_sparse_pad") for c in s["calls"]) == 1 and kw["tail"] in s["calls"]
        assert held[1]["calls"] == over["calls"]           # (the first step also builds one-off tables)
