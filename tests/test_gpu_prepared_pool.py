"""An input pool prepared at pool fill (SasrecEngine.PREPARED_POOL; csrc/pool_prepare.hip, pool_slab.h): one slab per batch holding what
the step head's packing role and the five phases of the step's index sort compute -- against an independent statement, against the
per-step path, and the step on it bit for bit against the step without it."""
import pytest
import torch

from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu

D, HID = 128, 32
# B, T, table rows: one partial 64-row tile with heavy duplicates; odd sizes over two tiles a domain; the two-strip forward (FOLD_SHORT)
SHAPES = [(5, 50, 300), (33, 34, 5000), (16, 20, 3000)]


def log(msg):
    print(msg)


def pad_heavy_batch(B, T, n_rows, seed):
    """About 90 % of the sequence positions hold the pad id (the last row): its run in the sorted list spans many 64-entry chunks."""
    return orc.synthetic_batch(B, T, n_rows - 1, pad_id=n_rows - 1, neg=1, seed=seed, mean_len=T / 10.0)


_PARAMS = {}


def params(T, n_rows):
    if (T, n_rows) not in _PARAMS:
        _PARAMS[(T, n_rows)] = orc.random_params(orc.sasrec_param_shapes(n_rows, D, T, HID), seed=11 + T)
    return _PARAMS[(T, n_rows)]


def make_engine(T, n_rows, prepared, compute="f32"):
    from amid_amd.engine import SasrecEngine
    eng = SasrecEngine(n_rows, D, T, HID, lr=1e-3, seed=31, compute=compute)
    eng.PREPARED_POOL = prepared
    eng.load_state_dict(params(T, n_rows))
    return eng


def pack(eng, pl, batches):
    out = []
    for b in batches:
        cu = {k: v.cuda() for k, v in b.items()}
        out.append(eng.pack_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"]))
    return torch.stack(out)


def engine_on_pool(B, T, n_rows, prepared, batches, compute="f32"):
    eng = make_engine(T, n_rows, prepared, compute)
    pl = eng.plan(B, T, 2, need_grad=True)
    eng.set_input_pool(pl, pack(eng, pl, batches))
    return eng, pl


def slab_sections(B, T, NI):
    """The slab's layout restated (csrc/pool_slab.h): a 16-int header, then the sections, each rounded up to 4 ints."""
    n_idx, n_c = 2 * B * T + B * NI, B * T + B * NI
    off, o = {}, 16
    for name, n in (("idx_all", n_idx), ("idx_c", n_c), ("row_c", n_c), ("live", B + 1), ("pos_sorted", n_c), ("uniq_ids", n_c),
                    ("seg_off", n_c + 1), ("seg_of", n_c)):
        off[name] = (o, n)
        o += (n + 3) // 4 * 4
    return off, (o + 63) // 64 * 64


def slab_views(eng, pl, i):
    slabs = eng.pool_slabs(pl)
    assert slabs is not None, "the pool was not prepared"
    shp = pl.shape
    off, ints = slab_sections(shp.B, shp.T, shp.NI)
    assert slabs[0].shape[1] == ints
    row = slabs[0][i]
    out = {k: row[o:o + n] for k, (o, n) in off.items()}
    out["n_uniq"], out["err"] = int(row[0].item()), int(row[1].item())
    return out


def host_lists(batch, n_rows):
    """idx_all, idx_c, row_c, live of a batch, restated on the host."""
    i_node, neg, s1, s2, dom = (batch[k].long() for k in ("i_node", "neg_samples", "seq_d1", "seq_d2", "domain_id"))
    B, T = s1.shape
    items = torch.cat((i_node.reshape(B, 1), neg.reshape(B, -1)), 1)
    NI = items.shape[1]
    idx_all = torch.cat((s1.reshape(-1), s2.reshape(-1), items.reshape(-1)))
    idx_all = torch.where((idx_all < 0) | (idx_all >= n_rows), torch.zeros_like(idx_all), idx_all)
    row_seq = (dom[:, None] * B * T + torch.arange(B)[:, None] * T + torch.arange(T)[None, :]).reshape(-1)
    row_c = torch.cat((row_seq, 2 * B * T + torch.arange(B * NI)))
    live = torch.cat((torch.nonzero(dom == 0).reshape(-1), torch.nonzero(dom != 0).reshape(-1), torch.tensor([int((dom == 0).sum())])))
    return idx_all, idx_all[row_c], row_c, live


def count_launches(fn):
    from amid_amd._lib import lib
    L = lib()
    names, orig = [], L.call

    def spy(name, *a):
        names.append(name)
        return orig(name, *a)
    L.call = spy
    try:
        fn()
    finally:
        L.call = orig
    return names


def assert_folded(pl, prepared, names=None):
    """The plan's launch record: the folded step, on the prepared pool or not; the launches it names."""
    assert pl.tail2, "the shape was chosen to take the folded step"
    assert bool(pl.prepared) == prepared and bool(pl.riding) != prepared
    if names is not None:
        assert ("amid_step_head_prepared_f32" in names) == prepared, names
        assert not prepared or not [n for n in names if "_sort" in n], names
        if pl.gather_on_fwd:
            assert len(names) == 9, names


@pytest.mark.parametrize("B,T,n_rows", SHAPES)
def test_slab_against_an_independent_statement_and_the_per_step_path(B, T, n_rows):
    batches = [pad_heavy_batch(B, T, n_rows, seed=40 + 7 * i + B) for i in range(3)]
    on, pl_on = engine_on_pool(B, T, n_rows, True, batches)
    off, pl_off = engine_on_pool(B, T, n_rows, False, batches)
    assert off.pool_slabs(pl_off) is None
    on.sync()
    n_c = pl_on.n_compact
    for i, batch in enumerate(batches):
        s = {k: (v.cpu().long() if torch.is_tensor(v) else v) for k, v in slab_views(on, pl_on, i).items()}
        idx_all, idx_c, row_c, live = host_lists(batch, n_rows)
        assert torch.equal(s["idx_all"], idx_all) and torch.equal(s["idx_c"], idx_c) and torch.equal(s["row_c"], row_c), i
        assert torch.equal(s["live"], live) and s["err"] == 0, i
        # the sort carries row_c as its payload (pos_sorted = the gradient rows in sorted order); row_c is injective, so mapping it back
        # gives the permutation itself: it must be the stable sort's
        perm = torch.sort(idx_c, stable=True).indices
        back = torch.full((int(row_c.max()) + 1,), -1, dtype=torch.long)
        back[row_c] = torch.arange(n_c)
        assert torch.equal(back[s["pos_sorted"]], perm), i
        uq, cnt = torch.unique_consecutive(idx_c[perm], return_counts=True)
        U = s["n_uniq"]
        assert U == uq.numel() and torch.equal(s["uniq_ids"][:U], uq), i
        first = torch.cat((torch.zeros(1, dtype=torch.long), cnt.cumsum(0)))
        assert torch.equal(s["seg_off"][:U + 1], first), i
        assert torch.equal(s["seg_of"], torch.repeat_interleave(torch.arange(U), cnt)), i
        frac_pad = float((idx_c == n_rows - 1).float().mean())
        assert int(cnt.max()) > 64, "the pad row's run must cross 64-entry chunk borders"
        log(f"slab B={B} T={T} batch {i}: n_uniq {U}, pad fraction of the compact list {frac_pad:.2f}, longest run {int(cnt.max())}")
        # ... and against what one step of the per-step path leaves in the plan's buffers for the same batch
        names = count_launches(lambda: off.enqueue_train_step(pl_off))
        off.sync()
        assert_folded(pl_off, False, names)
        assert int(pl_off.n_uniq.item()) == U
        for k, n in (("idx_all", pl_off.shape.n_idx), ("idx_c", n_c), ("row_c", n_c), ("live", B + 1), ("pos_sorted", n_c), ("uniq_ids", U),
                     ("seg_off", U + 1), ("seg_of", n_c)):
            assert torch.equal(getattr(pl_off, k)[:n].cpu().long(), s[k][:n]), (i, k)


def run_steps(eng, pl, mode, n):
    if mode == "eager":
        for _ in range(n):
            eng.enqueue_train_step(pl)
        return
    done = 0
    if mode == "graph4":
        while n - done >= 4:
            eng.replay_train_steps(pl, 4)
            done += 4
    for _ in range(n - done):
        eng.replay_train_step(pl)


def state_of(eng):
    return dict(table=eng.table.clone(), m=eng.table_m.clone(), v=eng.table_v.clone(), last=eng.table_last.clone(), dense=eng.dense.data.clone(),
                dense_m=eng.dense.m.clone(), dense_v=eng.dense.v.clone())


@pytest.mark.parametrize("mode", ["eager", "graph1", "graph4"])
@pytest.mark.parametrize("B,T,n_rows", SHAPES)
def test_step_on_a_prepared_pool_is_bit_identical(B, T, n_rows, mode):
    """Loss, every dense gradient and the rows' gradients after one step; table, moments, stamps and dense parameters after seven steps on a
    pool of three (the pool wraps twice, rows lag and are replayed; a graph of four steps crosses the pool's end inside the graph)."""
    batches = [pad_heavy_batch(B, T, n_rows, seed=90 + 5 * i + T) for i in range(3)]
    got = {}
    for prepared in (False, True):
        eng, pl = engine_on_pool(B, T, n_rows, prepared, batches)
        if mode != "eager":
            eng.capture_train_step(pl)
            if mode == "graph4":
                eng.capture_train_steps(pl, 4)
        rec = {}
        if mode != "graph4":
            names = count_launches(lambda: run_steps(eng, pl, mode, 1)) if mode == "eager" else run_steps(eng, pl, mode, 1)
            eng.sync()
            assert_folded(pl, prepared, names)
            U = int(pl.n_uniq.item())
            rec["one"] = dict(loss=pl.loss.clone(), grad=eng.dense.grad.clone(), uniq_grad=pl.uniq_grad[:U].clone(), U=U)
            run_steps(eng, pl, mode, 6)
        else:
            run_steps(eng, pl, mode, 7)
        eng.sync()
        assert eng.step == 7
        assert_folded(pl, prepared)
        eng.check_index_error(pl)
        rec["seven"] = state_of(eng)
        got[prepared] = rec
    if "one" in got[True]:
        a, b = got[False]["one"], got[True]["one"]
        assert a["U"] == b["U"]
        for k in ("loss", "grad", "uniq_grad"):
            assert torch.equal(a[k], b[k]), k
    lagged = int((got[True]["seven"]["last"] > 0).sum()) - int((got[True]["seven"]["last"] == 7).sum())
    assert lagged > 0, "some rows must lag behind the step counter (they are replayed when they are next read)"
    for k, want in got[False]["seven"].items():
        assert torch.equal(got[True]["seven"][k], want), k


def test_refill_on_an_epoch_boundary_reprepares_in_place():
    B, T, n_rows = 33, 34, 5000
    first = [pad_heavy_batch(B, T, n_rows, seed=300 + i) for i in range(3)]
    second = [pad_heavy_batch(B, T, n_rows, seed=400 + i) for i in range(3)]
    got = {}
    for prepared in (False, True):
        eng, pl = engine_on_pool(B, T, n_rows, prepared, first)
        eng.capture_train_step(pl)
        eng.replay_train_step(pl)
        new_pool = pack(eng, pl, second)
        slabs = eng.pool_slabs(pl)
        before = slabs[0].clone() if prepared else None
        assert eng.refill_input_pool(pl, new_pool) is False, "off a pool boundary the pool stays"
        eng.sync()
        if prepared:
            assert torch.equal(slabs[0], before), "nothing is re-prepared off a boundary"
        eng.replay_train_step(pl)
        eng.replay_train_step(pl)
        addr = slabs[0].data_ptr() if prepared else None
        assert eng.refill_input_pool(pl, new_pool) is True
        eng.replay_train_step(pl)                      # (the graph captured on the first pool)
        eng.sync()
        assert eng.step == 4
        if prepared:
            assert eng.pool_slabs(pl)[0].data_ptr() == addr
            s = slab_views(eng, pl, 0)
            assert torch.equal(s["idx_c"].cpu().long(), host_lists(second[0], n_rows)[1])
        assert_folded(pl, prepared)
        eng.check_index_error(pl)
        got[prepared] = dict(state_of(eng), loss=pl.loss.clone())
    for k, want in got[False].items():
        assert torch.equal(got[True][k], want), k


@pytest.mark.parametrize("prepared", [False, True])
def test_out_of_range_id_raises_when_its_batch_has_run(prepared):
    B, T, n_rows = 33, 34, 5000
    batches = [pad_heavy_batch(B, T, n_rows, seed=500 + i) for i in range(3)]
    batches[2]["seq_d1"][3, T - 1] = n_rows + 5
    batches[2]["seq_d2"][3, T - 1] = n_rows + 5
    eng, pl = engine_on_pool(B, T, n_rows, prepared, batches)
    for _ in range(2):
        eng.enqueue_train_step(pl)
        eng.sync()
        eng.check_index_error(pl)                     # (the bad batch's slab exists already: its flag must not show before its step)
    eng.enqueue_train_step(pl)
    eng.sync()
    assert_folded(pl, prepared)
    with pytest.raises(Exception):
        eng.check_index_error(pl)


def test_plans_outside_the_prepared_path_run_the_per_step_launches():
    """compute = "bf16" folds its step onto the fp32 step's launches but keeps the per-step head and the riders; the switch off does too."""
    B, T, n_rows = 33, 34, 5000
    batches = [pad_heavy_batch(B, T, n_rows, seed=600 + i) for i in range(2)]
    eng, pl = engine_on_pool(B, T, n_rows, True, batches, compute="bf16")
    assert eng.pool_slabs(pl) is None
    names = count_launches(lambda: eng.enqueue_train_step(pl))
    eng.sync()
    assert not pl.prepared
    assert "amid_step_head_prepared_f32" not in names and "amid_sas_strip_qkv_bwd_scorer_f32" not in names and "amid_sas_wgrad_rows_ln_f32" not in names, names
    if pl.tail2:
        assert pl.riding and ("amid_step_head_w16_f32" in names or "amid_step_head_f32" in names), names
    from amid_amd._lib import lib
    assert lib().value("amid_pool_prepare_workspace_bytes", 2, B, T, 1, (1 << 20) + 1) == 0      # keys of 2^20 and more: the per-step head
    assert lib().value("amid_pool_prepare_workspace_bytes", 2, B, T, 1, 1 << 20) > 0
