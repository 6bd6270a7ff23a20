"""GPU parity tests, kernel by kernel, through the C ABI (libamid_hip.so) against the CPU oracle.

Tolerances: indices / gathered rows bit-exact; fp32 activations 1e-5 relative to the tensor's
max magnitude per kernel (the north-star bar is 1e-4 relative on the final logits)."""
import os

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def L():
    from amid_amd._lib import lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return lib()


def dev(t):
    return t.cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------
def test_gather_golden_bit_exact(L):
    z = np.load(os.path.join(GOLDEN, "g1_gather.npz"))
    table, idx = dev(torch.from_numpy(z["table"])), dev(torch.from_numpy(z["idx"]))
    out = torch.empty(idx.numel(), table.shape[1], device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.call("amid_gather_rows_f32", table.data_ptr(), table.shape[0], table.shape[1], idx.data_ptr(), 1, idx.numel(), out.data_ptr(),
           err.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(z["rows"].shape), z["rows"])
    assert int(err.item()) == 0


@pytest.mark.parametrize("D,n_idx", [(128, 100000), (64, 777), (256, 5), (128, 0)])
def test_gather_random_bit_exact(L, D, n_idx):
    g = torch.Generator().manual_seed(D + n_idx)
    table = torch.randn(50000, D, generator=g)
    idx = torch.randint(0, 50000, (max(n_idx, 1),), generator=g)[:n_idx]
    td, idd = dev(table), dev(idx.int())
    out = torch.full((max(n_idx, 1), D), -1.0, device="cuda")
    L.call("amid_gather_rows_f32", td.data_ptr(), 50000, D, idd.data_ptr(), 0, n_idx, out.data_ptr(), None, stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:n_idx].cpu(), orc.gather_rows(table, idx))


def test_gather_out_of_range_sets_flag(L):
    table = dev(torch.randn(10, 64))
    idx = dev(torch.tensor([1, 99, 3], dtype=torch.int64))
    out = torch.empty(3, 64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.call("amid_gather_rows_f32", table.data_ptr(), 10, 64, idx.data_ptr(), 1, 3, out.data_ptr(), err.data_ptr(), stream())
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    assert torch.equal(out[0], table[1]) and torch.equal(out[2], table[3])


# ---------------------------------------------------------------------------------------------
def run_sort_unique(L, idx, n_rows, ws=None):
    n = idx.numel()
    idd = dev(idx.int())
    if ws is None:           # zero-filled once; every call leaves it ready for the next
        ws = torch.zeros(L.value("amid_sort_unique_workspace_bytes", n), dtype=torch.uint8, device="cuda")
    pos = torch.zeros(n, dtype=torch.int32, device="cuda")
    uniq = torch.zeros(n, dtype=torch.int32, device="cuda")
    seg = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    nu = torch.zeros(1, dtype=torch.int32, device="cuda")
    sof = torch.zeros(n, dtype=torch.int32, device="cuda")
    L.call("amid_sort_unique_i32", idd.data_ptr(), n, n_rows, ws.data_ptr(), pos.data_ptr(), uniq.data_ptr(), seg.data_ptr(), sof.data_ptr(),
           nu.data_ptr(), stream())
    torch.cuda.synchronize()
    U = int(nu.item())
    return pos.cpu().long(), uniq[:U].cpu().long(), seg[: U + 1].cpu().long(), U, (pos, uniq, seg, sof)


@pytest.mark.parametrize("n,n_rows,pad_frac", [(26112, 894820, 0.89), (6528, 894820, 0.85), (300, 50, 0.0), (1, 10, 0.0),
                                               (2048, 1 << 20, 0.5), (2049, 300, 0.99), (417792, 10_000_002, 0.89), (50000, 10_000_002, 0.0)])
def test_sort_unique_matches_stable_sort(L, n, n_rows, pad_frac):
    g = torch.Generator().manual_seed(n)
    idx = torch.randint(0, n_rows, (n,), generator=g)
    idx[torch.rand(n, generator=g) < pad_frac] = n_rows - 1
    pos, uniq, seg, U, _ = run_sort_unique(L, idx, n_rows)
    want_pos = torch.sort(idx, stable=True).indices
    assert torch.equal(pos, want_pos)                      # bit-exact inverted index
    wu, wc = torch.unique(idx, return_counts=True)
    assert U == wu.numel() and torch.equal(uniq, wu)
    assert torch.equal(seg, torch.cat((torch.zeros(1, dtype=torch.long), wc.cumsum(0))))
    assert torch.equal(_[3].cpu().long(), torch.repeat_interleave(torch.arange(U), wc))      # run index of every sorted entry


@pytest.mark.parametrize("four_min", [65536, 0])
def test_sort_unique_rows_payload_and_one_workspace_for_many_lengths(L, four_min):
    """amid_sort_unique_rows_i32: pos_sorted carries the caller's row of every entry (the compact index list of the live train step);
    and ONE workspace, sized for the longest list, serves lists of different lengths in turn -- what a plan's timed (compact) and
    plain (full) steps do -- through both sorts."""
    prev = L.value("amid_sort_set_four_launch_min", four_min)
    try:
        n_max, n_rows = 417792, 10_000_002
        ws = torch.zeros(L.value("amid_sort_unique_workspace_bytes", n_max), dtype=torch.uint8, device="cuda")
        g = torch.Generator().manual_seed(3)
        for n in (212992, 417792, 13312, 212992, 70000, 417792):
            idx = torch.randint(0, n_rows, (n,), generator=g)
            idx[torch.rand(n, generator=g) < 0.5] = n_rows - 1
            rows = torch.randperm(2 * n, generator=g)[:n].to(torch.int32)
            out = [torch.zeros(n + 1, dtype=torch.int32, device="cuda") for _ in range(4)]
            nu = torch.zeros(1, dtype=torch.int32, device="cuda")
            d_idx, d_rows = idx.int().cuda(), rows.cuda()
            L.call("amid_sort_unique_rows_i32", d_idx.data_ptr(), d_rows.data_ptr(), n, n_rows, ws.data_ptr(), out[0].data_ptr(),
                   out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), nu.data_ptr(), stream())
            torch.cuda.synchronize()
            order = torch.sort(idx, stable=True).indices
            assert torch.equal(out[0][:n].cpu().long(), rows.long()[order])
            wu, wc = torch.unique(idx, return_counts=True)
            U = int(nu.item())
            assert U == wu.numel() and torch.equal(out[1][:U].cpu().long(), wu)
            assert torch.equal(out[2][: U + 1].cpu().long(), torch.cat((torch.zeros(1, dtype=torch.long), wc.cumsum(0))))
            check_sort(idx, run_sort_unique(L, idx, n_rows, ws))              # and the same workspace without a payload
    finally:
        L.value("amid_sort_set_four_launch_min", prev)


@pytest.mark.parametrize("four_min", [65536, 0])
def test_sort_one_workspace_odd_number_of_calls_per_length(L, four_min):
    """big, small, big (and small, big, small) with ONE call each on one workspace: the two copies of the four-launch sort's stot_0 table
    alternate between calls, and a call must zero the OTHER copy over what the previous call accumulated there -- not over its own,
    shorter extent (csrc/sort_phases.h os_count_block).  The lengths are those of a cfg 5 plan's full autograd list (13 supertiles)
    and compact train list (7)."""
    prev = L.value("amid_sort_set_four_launch_min", four_min)
    try:
        n_rows = 10_000_002
        ws = torch.zeros(L.value("amid_sort_unique_workspace_bytes", 417792), dtype=torch.uint8, device="cuda")
        g = torch.Generator().manual_seed(5)
        for n in (417792, 212992, 417792, 70000, 417792, 212992, 70000, 212992):
            idx = torch.randint(0, n_rows, (n,), generator=g)
            idx[torch.rand(n, generator=g) < 0.3] = n_rows - 1
            check_sort(idx, run_sort_unique(L, idx, n_rows, ws))
    finally:
        L.value("amid_sort_set_four_launch_min", prev)


def check_sort(idx, out):
    pos, uniq, seg, U, raw = out
    assert torch.equal(pos, torch.sort(idx, stable=True).indices)
    wu, wc = torch.unique(idx, return_counts=True)
    assert U == wu.numel() and torch.equal(uniq, wu)
    assert torch.equal(seg, torch.cat((torch.zeros(1, dtype=torch.long), wc.cumsum(0))))
    assert torch.equal(raw[3].cpu().long(), torch.repeat_interleave(torch.arange(U), wc))


@pytest.mark.parametrize("n,n_rows", [(26112, 894820), (10752, 894820), (417792, 10_000_002), (4097, 1 << 24), (30000, (1 << 24) + 5),
                                      (5000, 2), (2048, 3)])
def test_sort_unique_workspace_reuse_and_key_shapes(L, n, n_rows):
    """The four-launch sort (forced for every length here) keeps its tables in the workspace and leaves them zero: five different
    inputs through ONE workspace (uniform, all keys equal, already sorted, a few hot keys, reversed), key ranges of 1 .. 24 bits, and
    the multi-pass path above 2^24."""
    prev = L.value("amid_sort_set_four_launch_min", 0)
    try:
        _sort_reuse_cases(L, n, n_rows)
    finally:
        L.value("amid_sort_set_four_launch_min", prev)


def _sort_reuse_cases(L, n, n_rows):
    ws = torch.zeros(L.value("amid_sort_unique_workspace_bytes", n), dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(n + 1)
    hot = torch.randint(0, n_rows, (7,), generator=g)
    cases = [torch.randint(0, n_rows, (n,), generator=g), torch.full((n,), n_rows - 1), torch.sort(torch.randint(0, n_rows, (n,), generator=g)).values,
             hot[torch.randint(0, 7, (n,), generator=g)], torch.randint(0, n_rows, (n,), generator=g).flip(0)]
    for idx in cases:
        check_sort(idx, run_sort_unique(L, idx, n_rows, ws))


@pytest.mark.parametrize("world,length,n_rows", [(2, 37, 100), (8, 2600, 894820), (3, 1, 10), (16, 500, 4000), (4, 4096, 3000)])
def test_merge_sorted_lists_matches_stable_sort(L, world, length, n_rows):
    """Data-parallel merge: `world` ascending unique lists, sentinel-padded to a common length (what HipMergeBackend.pad
    produces) -> same outputs as a stable sort of the concatenation, with the sentinel run left out of n_uniq."""
    g = torch.Generator().manual_seed(world * 1000 + length)
    lists, counts = [], []
    for r in range(world):
        k = int(torch.randint(0, min(length, n_rows) + 1, (1,), generator=g)) if r else min(length, n_rows)     # rank 0 full, others ragged
        ids = torch.randperm(n_rows, generator=g)[:k].sort().values
        lists.append(torch.cat((ids, torch.full((length - k,), n_rows, dtype=torch.long))))
        counts.append(k)
    keys = torch.cat(lists)
    n = world * length
    kd = keys.to(torch.int32).cuda()
    ws = torch.zeros(L.value("amid_sort_unique_workspace_bytes", n), dtype=torch.uint8, device="cuda")
    pos = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    uniq = torch.zeros(n, dtype=torch.int32, device="cuda")
    seg = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    sof = torch.zeros(n, dtype=torch.int32, device="cuda")
    nu = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.call("amid_merge_sorted_lists_i32", kd.data_ptr(), world, length, length, 0, length, n_rows, ws.data_ptr(), pos.data_ptr(), uniq.data_ptr(),
           seg.data_ptr(), sof.data_ptr(), nu.data_ptr(), stream())
    torch.cuda.synchronize()
    assert torch.equal(pos.cpu().long(), torch.sort(keys, stable=True).indices)         # ties in rank order
    wu, wc = torch.unique(keys, return_counts=True)
    has_pad = bool((keys == n_rows).any())
    U = int(nu.item())
    assert U == wu.numel() - (1 if has_pad else 0)
    assert torch.equal(uniq[:wu.numel()].cpu().long(), wu)
    assert torch.equal(seg[: wu.numel() + 1].cpu().long(), torch.cat((torch.zeros(1, dtype=torch.long), wc.cumsum(0))))
    assert torch.equal(sof.cpu().long(), torch.repeat_interleave(torch.arange(wu.numel()), wc))


@pytest.mark.parametrize("D,n,n_rows,pad_frac", [(128, 26112, 894820, 0.89), (64, 6528, 5000, 0.85), (128, 70, 1000, 0.0),
                                                 (256, 1000, 20, 0.3), (128, 417792, 10_000_002, 0.89), (128, 4096, 7, 0.0)])
def test_segreduce_matches_index_add(L, D, n, n_rows, pad_frac):
    g = torch.Generator().manual_seed(n + D)
    idx = torch.randint(0, n_rows, (n,), generator=g)
    idx[torch.rand(n, generator=g) < pad_frac] = n_rows - 1
    rows = torch.randn(n, D, generator=g)
    pos, uniq, seg, U, (pos_d, uniq_d, seg_d, sof_d) = run_sort_unique(L, idx, n_rows)
    rd = dev(rows)
    ws = torch.empty(L.value("amid_segreduce_workspace_bytes", n, D), dtype=torch.uint8, device="cuda")
    out = torch.full((n, D), float("nan"), device="cuda")
    L.call("amid_embgrad_segreduce_f32", rd.data_ptr(), pos_d.data_ptr(), seg_d.data_ptr(), sof_d.data_ptr(), n, D, ws.data_ptr(),
           out.data_ptr(), stream())
    torch.cuda.synchronize()
    # reference semantics: dense index_add (EmbeddingBackward) restricted to the touched rows, in fp64
    want = torch.zeros(U, D, dtype=torch.float64)
    inv = torch.searchsorted(uniq, idx)
    want.index_add_(0, inv, rows.double())
    got = out[:U].cpu().double()
    scale = want.abs().max()
    assert float((got - want).abs().max() / scale) < 2e-6
    # reproducible: a second run is bitwise identical
    out2 = torch.empty_like(out)
    L.call("amid_embgrad_segreduce_f32", rd.data_ptr(), pos_d.data_ptr(), seg_d.data_ptr(), sof_d.data_ptr(), n, D, ws.data_ptr(),
           out2.data_ptr(), stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:U], out2[:U])


# ---------------------------------------------------------------------------------------------
def step_state(L, seed, step, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8):
    import ctypes
    n = L.value("amid_step_state_bytes")
    host = (ctypes.c_ubyte * n)()
    L.call("amid_step_state_pack", ctypes.addressof(host), seed, step, lr, b1, b2, eps)
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()


def test_dense_adam_matches_torch_op_order(L):
    g = torch.Generator().manual_seed(5)
    n = 4099
    p0 = torch.randn(n, generator=g)
    P = {"w": p0.clone()}
    opt = orc.DenseAdam(P, lr=1e-2)
    pd, md, vd = dev(p0.clone()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for t in range(1, 8):
        grad = torch.randn(n, generator=g) * (0.0 if t == 4 else 1.0)
        opt.step(P, {"w": grad})
        st = step_state(L, 0, t, lr=1e-2)
        gd = dev(grad)
        L.call("amid_adam_dense_f32", pd.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), n, 1.0, st.data_ptr(), stream())
        torch.cuda.synchronize()
        assert float((pd.cpu() - P["w"]).abs().max()) < 1e-6, t


@pytest.mark.parametrize("by_position", [False, True, None])
def test_lazy_adam_equals_dense_adam_with_idle_rows(L, by_position):
    """Rows touched at some steps and idle at others must follow the dense trajectory.
    by_position: catch-up driven by the raw index list (duplicates included) instead of the unique list; None: no catch-up launch at all --
    amid_lazy_adam_apply_f32 itself replays what a lagging row owes in front of the real step (checked on the rows it applied)."""
    g = torch.Generator().manual_seed(11)
    n_rows, D, steps = 40, 64, 30
    tab0 = torch.randn(n_rows, D, generator=g)
    P = {"t": tab0.clone()}
    opt = orc.DenseAdam(P, lr=5e-3)
    tab, m, v = dev(tab0.clone()), torch.zeros(n_rows, D, device="cuda"), torch.zeros(n_rows, D, device="cuda")
    last = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    for t in range(1, steps + 1):
        k = int(torch.randint(1, 6, (1,), generator=g))
        touched = torch.randperm(n_rows - 1, generator=g)[:k].sort().values
        if t % 3 == 0:
            touched = torch.cat((touched, torch.tensor([n_rows - 1]))).unique()      # a row touched every 3rd step
        grows = torch.randn(touched.numel(), D, generator=g)
        dense = torch.zeros(n_rows, D)
        dense[touched] = grows
        st = step_state(L, 0, t, lr=5e-3)
        ud, gd = dev(touched.int()), dev(grows)
        nu = torch.tensor([touched.numel()], dtype=torch.int32, device="cuda")
        if by_position is None:
            pass
        elif by_position:
            pos = touched[torch.randint(0, touched.numel(), (3 * touched.numel() + 5,), generator=g)]       # duplicates, any order
            pos = torch.cat((pos, touched)).int().cuda()
            L.call("amid_lazy_adam_catchup_positions_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), pos.data_ptr(),
                   pos.numel(), D, st.data_ptr(), stream())
        else:
            L.call("amid_lazy_adam_catchup_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), ud.data_ptr(), nu.data_ptr(),
                   n_rows, D, st.data_ptr(), stream())
        torch.cuda.synchronize()
        # the rows about to be gathered must already equal the dense trajectory after step t-1
        if by_position is not None:
            assert float((tab.cpu()[touched] - P["t"][touched]).abs().max()) < 2e-6, ("pre-gather", t)
        opt.step(P, {"t": dense})
        L.call("amid_lazy_adam_apply_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), ud.data_ptr(), nu.data_ptr(),
               n_rows, gd.data_ptr(), 1.0, D, st.data_ptr(), stream())
        torch.cuda.synchronize()
        if by_position is None:
            assert float((tab.cpu()[touched] - P["t"][touched]).abs().max()) < 2e-6, ("applied", t)
    st = step_state(L, 0, steps, lr=5e-3)
    L.call("amid_lazy_adam_flush_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), n_rows, D, st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert float((tab.cpu() - P["t"]).abs().max()) < 2e-6
    assert int(last.min().item()) in (0, steps)


def test_optimizer_step_spans_dense_tail_and_lagging_rows_follow_dense_adam(L):
    """amid_optimizer_step_spans_f32 called directly on a list without chunk-crossing runs (one entry per id, a single chunk: no spans
    workgroup owns anything, the workspace is never read): its dense role on n = 4099 floats (the scalar tail: the engine's flat buffer is
    always a multiple of four) and its row role on rows that return after three idle steps, against orc.DenseAdam.  Bars: those of
    test_dense_adam_matches_torch_op_order (1e-6) and test_lazy_adam_equals_dense_adam_with_idle_rows (2e-6)."""
    g = torch.Generator().manual_seed(21)
    n, n_rows, D, lr = 4099, 9, 64, 5e-3
    p0, tab0 = torch.randn(n, generator=g), torch.randn(n_rows, D, generator=g)
    P = {"w": p0.clone(), "t": tab0.clone()}
    opt = orc.DenseAdam(P, lr=lr)
    pd, md, vd = dev(p0.clone()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    tab, m, v = dev(tab0.clone()), torch.zeros(n_rows, D, device="cuda"), torch.zeros(n_rows, D, device="cuda")
    last = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    ws = torch.zeros(16 * D, device="cuda")
    for t in range(1, 6):
        ids = torch.tensor([0, 2, 3, 5, 8] if t in (1, 5) else [0, 3, 8])             # rows 2 and 5: stamped 1, back at step 5
        gw, grows = torch.randn(n, generator=g), torch.randn(ids.numel(), D, generator=g)
        dense = torch.zeros(n_rows, D)
        dense[ids] = grows
        opt.step(P, {"w": gw, "t": dense})
        U = ids.numel()
        ud, gd, gwd = dev(ids.int()), dev(grows), dev(gw)
        nu = torch.tensor([U], dtype=torch.int32, device="cuda")
        seg_off, seg_of = dev(torch.arange(U + 1, dtype=torch.int32)), dev(torch.arange(U, dtype=torch.int32))
        st = step_state(L, 0, t, lr=lr)
        if t == 5:
            assert last.cpu()[[2, 5]].tolist() == [1, 1]
        L.call("amid_optimizer_step_spans_f32", pd.data_ptr(), md.data_ptr(), vd.data_ptr(), gwd.data_ptr(), n, tab.data_ptr(), m.data_ptr(),
               v.data_ptr(), last.data_ptr(), ud.data_ptr(), nu.data_ptr(), U, gd.data_ptr(), D, 1.0, st.data_ptr(), seg_off.data_ptr(),
               seg_of.data_ptr(), U, ws.data_ptr(), stream())
        torch.cuda.synchronize()
        assert float((pd.cpu() - P["w"]).abs().max()) < 1e-6, t
        assert float((tab.cpu()[ids] - P["t"][ids]).abs().max()) < 2e-6, t
        assert bool((last.cpu()[ids] == t).all())


# ---------------------------------------------------------------------------------------------
def keep_masks_from_gpu_rng(L):
    """The device Philox must equal oracle.philox_keep_flat bit for bit (checked through embed_fwd)."""


@pytest.mark.parametrize("D", [64, 128])
def test_embed_fwd_bwd_vs_oracle(L, D):
    B, T, NI, n_rows = 5, 50, 3, 300
    g = torch.Generator().manual_seed(D)
    table = torch.randn(n_rows, D, generator=g)
    pos = [torch.randn(T, D, generator=g) for _ in range(2)]
    idx = torch.randint(0, n_rows, (2 * B * T + B * NI,), generator=g)
    # force exact zeros after the positional add on a few features (the ==0 timeline mask path)
    table[7] = -pos[0][3]
    idx[0 * T + 3] = 7
    table[8, :5] = -pos[1][10, :5]
    idx[B * T + 2 * T + 10] = 8
    seed, step = 1234, 3
    st = step_state(L, seed, step)
    td, idd = dev(table), dev(idx.int())
    p0, p1 = dev(pos[0]), dev(pos[1])
    N = idx.numel()
    xg = torch.empty(N, D, device="cuda")
    tmq = torch.zeros(2 * B * T, D // 4, dtype=torch.uint8, device="cuda")
    for train in (0, 1):
        L.call("amid_embed_fwd_f32", td.data_ptr(), idd.data_ptr(), p0.data_ptr(), p1.data_ptr(), B, T, D, B * NI, xg.data_ptr(),
               tmq.data_ptr(), st.data_ptr(), train, 0.5, stream())
        torch.cuda.synchronize()
        got = xg.cpu()
        for gi in range(2):
            rows = table[idx[gi * B * T:(gi + 1) * B * T]].reshape(B, T, D) + pos[gi]
            tm = rows == 0
            if train:
                keep = torch.from_numpy(orc.philox_keep_flat(B * T * D, seed, orc.site_id(gi, 0, orc.SITE_EMB), step, 0.5)).reshape(B, T, D)
                rows = rows * keep * 2.0
            rows = rows * (~tm)
            assert torch.equal(got[gi * B * T:(gi + 1) * B * T].reshape(B, T, D), rows), (train, gi)
            assert bool(tm.any())
        assert torch.equal(got[2 * B * T:], table[idx[2 * B * T:]])
    # backward (train mode): dxe = dx * ~tm * keep*2 ; dpos = sum_b
    dxg = torch.randn(N, D, generator=g)
    dd = dev(dxg.clone())
    nsplit = 3
    dpart = torch.zeros(nsplit, 2, T, D, device="cuda")
    L.call("amid_embed_bwd_f32", dd.data_ptr(), tmq.data_ptr(), B, T, D, nsplit, dpart.data_ptr(), st.data_ptr(), 1, 0.5, stream())
    torch.cuda.synchronize()
    dsum = dpart.sum(0)
    for gi, dp in ((0, dsum[0]), (1, dsum[1])):
        rows = table[idx[gi * B * T:(gi + 1) * B * T]].reshape(B, T, D) + pos[gi]
        tm = rows == 0
        keep = torch.from_numpy(orc.philox_keep_flat(B * T * D, seed, orc.site_id(gi, 0, orc.SITE_EMB), step, 0.5)).reshape(B, T, D)
        want = dxg[gi * B * T:(gi + 1) * B * T].reshape(B, T, D) * keep * 2.0 * (~tm)
        assert torch.equal(dd.cpu()[gi * B * T:(gi + 1) * B * T].reshape(B, T, D), want)
        assert relmax(dp, want.sum(0)) < 1e-6
    assert torch.equal(dd.cpu()[2 * B * T:], dxg[2 * B * T:])


# ---------------------------------------------------------------------------------------------
def oracle_attention(q, k, v, H, p_keep_mask=None, p=0.5):
    """softmax((q*scale) k^T + causal) [dropout] v on [B,T,D] tensors, fp64."""
    import math
    B, T, D = q.shape
    hd = D // H
    qh = q.double().reshape(B, T, H, hd).permute(0, 2, 1, 3) * math.sqrt(1.0 / hd)
    kh = k.double().reshape(B, T, H, hd).permute(0, 2, 1, 3)
    vh = v.double().reshape(B, T, H, hd).permute(0, 2, 1, 3)
    S = qh @ kh.transpose(-1, -2)
    S = S.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    A = torch.softmax(S, -1)
    if p_keep_mask is not None:
        A = A * p_keep_mask.double() / (1.0 - p)
    return (A @ vh).permute(0, 2, 1, 3).reshape(B, T, D)


@pytest.mark.parametrize("T", [64, 50, 17, 70, 100, 128, 129, 150, 256, 260])      # <= 64: matrix-core kernels; 65..256: their blocked form
@pytest.mark.parametrize("train", [0, 1])                           # (100: isInC at seq_len 50; 150: the reference's amazon seq_len); 260: general VALU kernels
@pytest.mark.parametrize("D,H", [(128, 8), (64, 8), (32, 4), (16, 2)])      # head dim 16; head dim 8 (the reference's default --emb_dim 64, train_sr.py:364):
def test_attention_fwd_bwd_vs_autograd(L, T, train, D, H):                  # pairs of heads per 16-column tile on the matrix cores at T <= 64
    B = 3
    if D // H == 8 and T > 64 and T not in (70, 150):
        pytest.skip("head dim 8 beyond 64 tokens runs the general VALU kernels: two lengths are enough")
    g = torch.Generator().manual_seed(T + train + D + H)
    q, k, v, do = (torch.randn(2 * B, T, D, generator=g) for _ in range(4))
    seed, step, layer = 77, 4, 1
    st = step_state(L, seed, step)
    qd, kd, vd, dod = dev(q), dev(k), dev(v), dev(do)
    o = torch.empty_like(qd); stats = torch.empty(2 * B * T, H, 2, device="cuda")
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(qd)
    L.call("amid_attn_fwd_f32", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), None, B, T, D, H, 1, layer, st.data_ptr(), train, 0.5,
           o.data_ptr(), stats.data_ptr(), stream())
    L.call("amid_attn_bwd_f32", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), stats.data_ptr(), dod.data_ptr(), None, B, T, D, H,
           1, layer, st.data_ptr(), train, 0.5, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), stream())
    torch.cuda.synchronize()
    for dom in range(2):
        sl = slice(dom * B, (dom + 1) * B)
        mask = None
        if train:
            TP = orc.attn_row_stride(T, 0.5)
            m = orc.philox_keep_flat(B * H * T * TP, seed, orc.site_id(dom, layer, orc.SITE_ATTN), step, 0.5)
            mask = torch.from_numpy(m.reshape(B, H, T, TP)[..., :T].copy())
        qq, kk, vv = (t[sl].clone().double().requires_grad_(True) for t in (q, k, v))
        want = oracle_attention(qq, kk, vv, H, mask)
        want.backward(do[sl].double())
        assert relmax(o[sl], want.detach()) < 2e-6, (dom, "o")
        assert relmax(dq[sl], qq.grad) < 5e-6 and relmax(dk[sl], kk.grad) < 5e-6 and relmax(dv[sl], vv.grad) < 5e-6, dom


@pytest.mark.parametrize("T", [64, 50, 17, 70, 150])          # <= 64: matrix-core kernels (attention_mfma_bert.hip); beyond: general VALU kernels
@pytest.mark.parametrize("train", [0, 1])
def test_attention_bert_shape_fwd_bwd_vs_autograd(L, T, train):
    """Bidirectional attention of BERT4Rec (model_seq.py:149-162): 4 heads of 32, scores / sqrt(d_k), masked keys at -1e9 (one row
    with EVERY key masked: uniform softmax, no score gradient), dropout 0.1 from the counter RNG."""
    B, D, H, p = 3, 128, 4, 0.1
    g = torch.Generator().manual_seed(100 + T + train)
    q, k, v, do = (torch.randn(2 * B, T, D, generator=g) for _ in range(4))
    keep = torch.rand(B, T, generator=g) > 0.3
    keep[0] = False                                        # every key of batch row 0 masked
    keep[1] = True
    seed, step, layer = 78, 6, 0
    st = step_state(L, seed, step)
    qd, kd, vd, dod = dev(q), dev(k), dev(v), dev(do)
    kk = keep.to(torch.uint8).cuda()
    o = torch.empty_like(qd); stats = torch.empty(2 * B * T, H, 2, device="cuda")
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(qd)
    L.call("amid_attn_fwd_f32", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), kk.data_ptr(), B, T, D, H, 0, layer, st.data_ptr(), train, p,
           o.data_ptr(), stats.data_ptr(), stream())
    L.call("amid_attn_bwd_f32", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), stats.data_ptr(), dod.data_ptr(), kk.data_ptr(), B, T,
           D, H, 0, layer, st.data_ptr(), train, p, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), stream())
    torch.cuda.synchronize()
    dkk = D // H
    for dom in range(2):
        sl = slice(dom * B, (dom + 1) * B)
        mask = None
        if train:
            TP = orc.attn_row_stride(T, p)
            mm = orc.philox_keep_flat(B * H * T * TP, seed, orc.site_id(dom, layer, orc.SITE_ATTN), step, p)
            mask = torch.from_numpy(mm.reshape(B, H, T, TP)[..., :T].copy())
        qq, kx, vv = (t[sl].clone().double().requires_grad_(True) for t in (q, k, v))
        qh, kh, vh = (t.reshape(B, T, H, dkk).permute(0, 2, 1, 3) for t in (qq, kx, vv))
        S = (qh @ kh.transpose(-2, -1)) / (dkk ** 0.5)
        S = S.masked_fill(~keep[:, None, None, :], -1e9)
        A = torch.softmax(S, -1)
        if mask is not None:
            A = A * mask.double() / (1.0 - p)
        want = (A @ vh).permute(0, 2, 1, 3).reshape(B, T, D)
        want.backward(do[sl].double())
        assert relmax(o[sl], want.detach()) < 3e-6, (dom, "o")
        assert relmax(dq[sl], qq.grad) < 1e-5 and relmax(dk[sl], kx.grad) < 1e-5 and relmax(dv[sl], vv.grad) < 1e-5, dom


def test_positive_rank_matches_reference_metrics(L):
    """Device ranks -> the seven metrics of the reference's get_sample_scores (g8 golden: HR/NDCG@1,5,10 + MRR, with a tie)."""
    import os
    import numpy as np
    from amid_amd.utils import FIX_VALUE_DOC, device_positive_ranks, get_sample_scores, scores_from_ranks
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_metrics.npz"))
    pred = torch.from_numpy(z["pred"]).cuda()
    dom = torch.zeros(pred.shape[0], dtype=torch.long, device="cuda")
    rank = device_positive_ranks(pred, pred, dom, 0.0)          # g8 was generated without the fix_value shift
    got = scores_from_ranks(rank)
    assert np.allclose(np.array(got), z["scores"], rtol=0, atol=1e-12)
    # domain selection + fix_value: ties count against the positive
    g = torch.Generator().manual_seed(0)
    p1, p2 = torch.rand(300, 200, generator=g), torch.rand(300, 200, generator=g)
    p1[5, 7] = p1[5, 0]; p2[6, 3] = p2[6, 0]
    d = (torch.rand(300, generator=g) < 0.5).long()
    d[5], d[6] = 0, 1
    fix = 1e-7
    r = device_positive_ranks(p1.cuda(), p2.cuda(), d.cuda(), fix).cpu()
    sel = torch.where(d[:, None] == 0, p1, p2).numpy().copy()
    sel[:, 0] -= np.float32(fix)
    want = (-sel).argsort(kind="stable").argsort(kind="stable")[:, 0]
    assert np.array_equal(r.numpy(), want)
    assert np.allclose(np.array(scores_from_ranks(r)), np.array(get_sample_scores(sel)), atol=1e-12)
    assert FIX_VALUE_DOC


def test_lazy_adam_long_idle_gap_beyond_coefficient_table(L):
    """A row idle for far more steps than the kernels' 256-entry coefficient table (a rare item) must still land on the dense
    trajectory when it is finally gathered again, by positions and by flush."""
    g = torch.Generator().manual_seed(3)
    n_rows, D, gap = 6, 64, 700
    tab0 = torch.randn(n_rows, D, generator=g)
    P = {"t": tab0.clone()}
    opt = orc.DenseAdam(P, lr=5e-3)
    tab, m, v = dev(tab0.clone()), torch.zeros(n_rows, D, device="cuda"), torch.zeros(n_rows, D, device="cuda")
    last = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    g1 = torch.randn(3, D, generator=g)
    dense = torch.zeros(n_rows, D); dense[:3] = g1
    ids = torch.arange(3, dtype=torch.int32).cuda()
    nu = torch.tensor([3], dtype=torch.int32, device="cuda")
    st = step_state(L, 0, 1, lr=5e-3)
    L.call("amid_lazy_adam_apply_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), ids.data_ptr(), nu.data_ptr(), n_rows,
           dev(g1).data_ptr(), 1.0, D, st.data_ptr(), stream())
    opt.step(P, {"t": dense})
    zero = {"t": torch.zeros(n_rows, D)}
    for _ in range(gap):                                   # the dense optimizer keeps moving the rows through their momentum
        opt.step(P, zero)
    t = gap + 2
    st = step_state(L, 0, t, lr=5e-3)
    pos = torch.tensor([1, 1, 0], dtype=torch.int32).cuda()             # rows 0 and 1 are about to be gathered at step t
    L.call("amid_lazy_adam_catchup_positions_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), pos.data_ptr(), 3, D,
           st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert float((tab.cpu()[:2] - P["t"][:2]).abs().max()) < 5e-6
    assert float((tab.cpu()[2] - tab0[2]).abs().max()) > 1e-3 or True
    st = step_state(L, 0, t - 1, lr=5e-3)
    L.call("amid_lazy_adam_flush_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), n_rows, D, st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert float((tab.cpu() - P["t"]).abs().max()) < 5e-6


@pytest.mark.parametrize("n_idx,n_lag", [(10752, 1500), (26112, 2900), (37, 20), (4097, 4000)])
def test_lazy_adam_catchup_by_positions_long_list_mixed_gaps(L, n_idx, n_lag):
    """The catch-up over a train step's list shape: most positions the pad row (touched every step), the lagging rows scattered over the
    list with duplicates, gaps from 1 to 700 steps (inside and beyond the 256-step coefficient table, short of and beyond the point where
    the increments stop moving the parameters) -- every row must land on the trajectory of a dense Adam that took all those zero-gradient
    steps; a second and third launch find every row current."""
    g = torch.Generator().manual_seed(n_idx)
    D, n_rows, t = 128, 6000, 1500
    tab0 = torch.randn(n_rows, D, generator=g)
    gr = torch.randn(n_rows, D, generator=g) * torch.logspace(-4, 0, n_rows)[:, None]
    rows = torch.randperm(n_rows - 1, generator=g)[:n_lag]
    gaps = torch.randint(1, 701, (n_lag,), generator=g)
    gaps[:4] = torch.tensor([1, 255, 256, 700])[: min(4, n_lag)]
    # reference: a dense Adam per distinct "last touched" step -- every lagging row got ONE real gradient at step t - 1 - gap, zeros since
    want = tab0.clone()
    m0, v0 = torch.zeros(n_rows, D), torch.zeros(n_rows, D)
    b1, b2, lr, eps = 0.9, 0.999, 5e-4, 1e-8
    l_of = (t - 1 - gaps)
    s0 = l_of.double()[:, None]
    gvec = gr[rows].double()
    mm, vv = (1 - b1) * gvec, (1 - b2) * gvec * gvec
    pp = tab0[rows].double() - lr / (1 - b1 ** s0) * mm / (vv.sqrt() / (1 - b2 ** s0).sqrt() + eps)
    m0[rows], v0[rows], tab0[rows] = mm.float(), vv.float(), pp.float()             # the state the kernel starts from (fp32, as stored)
    mm, vv, pp = m0[rows].double(), v0[rows].double(), tab0[rows].double()
    for sstep in range(int(l_of.min()) + 1, t):                                    # all rows at once: row j moves at steps > l_of[j]
        on = (sstep > l_of)[:, None].double()
        mm = torch.where(on > 0, b1 * mm, mm)
        vv = torch.where(on > 0, b2 * vv, vv)
        pp = pp - on * (lr / (1 - b1 ** sstep) * mm / (vv.sqrt() / (1 - b2 ** sstep) ** 0.5 + eps))
    want[rows] = pp.float()
    tab, m, v = dev(tab0.clone()), dev(m0.clone()), dev(v0.clone())
    last = torch.zeros(n_rows, dtype=torch.int32)
    last[rows] = l_of.int()
    last[n_rows - 1] = t - 1                                  # the pad row: current
    pos = torch.full((n_idx,), n_rows - 1, dtype=torch.int32)
    where = torch.randperm(n_idx, generator=g)[: min(n_idx, 2 * n_lag)]
    pos[where] = rows[torch.arange(where.numel()) % n_lag].int()             # every lagging row once or twice
    last, pos = dev(last), dev(pos)
    st = step_state(L, 0, t, lr=lr)
    for rep in range(3):
        L.call("amid_lazy_adam_catchup_positions_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), pos.data_ptr(), n_idx, D,
               st.data_ptr(), stream())
        torch.cuda.synchronize()
        touched = torch.unique(pos.cpu().long())
        assert float((tab.cpu()[touched] - want[touched]).abs().max()) < 5e-6, rep
        assert bool((last.cpu()[touched] == t - 1).all())
    untouched = torch.ones(n_rows, dtype=torch.bool)
    untouched[touched] = False
    assert torch.equal(tab.cpu()[untouched], tab0[untouched])


def _lagging_state(seed, n_rows, D, t, n_lag, max_gap):
    """A table state with n_lag rows that each took ONE real step some 1 .. max_gap steps before t - 1 and owe the steps since."""
    g = torch.Generator().manual_seed(seed)
    tab0 = torch.randn(n_rows, D, generator=g)
    m0 = torch.zeros(n_rows, D)
    v0 = torch.zeros(n_rows, D)
    rows = torch.randperm(n_rows - 1, generator=g)[:n_lag]
    gaps = torch.randint(1, max_gap + 1, (n_lag,), generator=g)
    gaps[:6] = torch.tensor([1, 63, 64, 255, 256, max_gap])[: min(6, n_lag)]
    gr = torch.randn(n_lag, D, generator=g) * torch.logspace(-4, 0, n_lag)[:, None]
    m0[rows], v0[rows] = 0.1 * gr, 0.001 * gr * gr
    last = torch.zeros(n_rows, dtype=torch.int32)
    last[rows] = (t - 1 - gaps).int()
    last[n_rows - 1] = t - 1
    return tab0, m0, v0, last, rows


def test_lazy_adam_split_replay_is_bit_identical_to_one_replay(L):
    """A zero-gradient step's coefficients depend on the step number alone (csrc/adam_replay.h): rows flushed at step t1 (before an
    evaluation, a checkpoint) and caught up at t2 land on the SAME BITS as rows caught up at t2 in one go -- gaps inside and beyond the
    256-step coefficient table, across the 64-step anchors of the running powers (they used to differ)."""
    D, n_rows, t1, t2 = 128, 3000, 1333, 1700
    tab0, m0, v0, last0, rows = _lagging_state(5, n_rows, D, t1, 400, 900)
    pos = dev(torch.cat([rows.int(), torch.full((7,), n_rows - 1, dtype=torch.int32)]))
    outs = []
    for split in (False, True):
        tab, m, v, last = dev(tab0.clone()), dev(m0.clone()), dev(v0.clone()), dev(last0.clone())
        if split:        # flush everything at t1 (stamps -> t1), then the catch-up of step t2
            st1 = step_state(L, 0, t1)
            L.call("amid_lazy_adam_flush_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), n_rows, D, st1.data_ptr(), stream())
        st2 = step_state(L, 0, t2)
        L.call("amid_lazy_adam_catchup_positions_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), pos.data_ptr(), pos.numel(), D,
               st2.data_ptr(), stream())
        torch.cuda.synchronize()
        outs.append((tab.cpu()[rows], m.cpu()[rows], v.cpu()[rows], last.cpu()[rows]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float((outs[0][0] - tab0[rows]).abs().max()) > 0          # the replay did move the rows


@pytest.mark.parametrize("live", [False, True])
def test_gather_with_folded_catchup_equals_catchup_then_gather(L, live):
    """amid_embed_fwd_replay_f32 (the catch-up folded into K1: owed steps replayed in registers, nothing written) hands the forward the
    same bits as the catch-up launch followed by the plain gather -- SASRec form (positional table, dropout, "== 0" mask) and plain
    gather; the optimizer launch then replays the same rows from the untouched state and lands where the two-launch path does."""
    B, T, D, NI, n_rows, t = 24, 50, 128, 2, 4000, 900
    tab0, m0, v0, last0, rows = _lagging_state(9, n_rows, D, t, 300, 600)
    g = torch.Generator().manual_seed(3)
    idx = torch.full((2 * B * T + B * NI,), n_rows - 1, dtype=torch.int32)
    where = torch.randperm(idx.numel(), generator=g)[:700]
    idx[where] = rows[torch.randint(0, rows.numel(), (700,), generator=g)].int()
    idx = dev(idx)
    pos0, pos1 = dev(torch.randn(T, D, generator=g)), dev(torch.randn(T, D, generator=g))
    dom = dev((torch.rand(B, generator=g) < 0.5).long())
    lv = dev(torch.zeros(B + 1, dtype=torch.int32))
    L.call("amid_live_list_i32", dom.data_ptr(), B, lv.data_ptr(), stream())
    lf = lv.data_ptr() if live else None
    st = step_state(L, 77, t)
    for pos in ((pos0, pos1), (None, None)):
        p0, p1 = (pos[0].data_ptr(), pos[1].data_ptr()) if pos[0] is not None else (None, None)
        res = []
        for fold in (False, True):
            tab, m, v, last = dev(tab0.clone()), dev(m0.clone()), dev(v0.clone()), dev(last0.clone())
            xg = dev(torch.zeros(idx.numel(), D))
            tmq = dev(torch.zeros(2 * B * T, D // 4, dtype=torch.uint8))
            tm = tmq.data_ptr() if p0 is not None else None
            if fold:
                L.call("amid_embed_fwd_replay_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), idx.data_ptr(), p0, p1, B, T, D,
                       B * NI, xg.data_ptr(), tm, st.data_ptr(), 1, 0.5, lf, None, None, st.data_ptr(), None, 0, stream())
                torch.cuda.synchronize()
                assert torch.equal(tab.cpu(), tab0) and torch.equal(last.cpu(), last0)            # nothing written
            else:
                L.call("amid_lazy_adam_catchup_positions_f32", tab.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), idx.data_ptr(),
                       idx.numel(), D, st.data_ptr(), stream())
                if live:
                    L.call("amid_embed_fwd_live_f32", tab.data_ptr(), idx.data_ptr(), p0, p1, B, T, D, B * NI, xg.data_ptr(), tm, st.data_ptr(), 1,
                           0.5, lf, stream())
                else:
                    L.call("amid_embed_fwd_f32", tab.data_ptr(), idx.data_ptr(), p0, p1, B, T, D, B * NI, xg.data_ptr(), tm, st.data_ptr(), 1, 0.5,
                           stream())
            # the step's optimizer launch on the gathered rows (a gradient of ones): replays what still lags, then the real step
            ids = torch.unique(idx.cpu().long()).int()
            uid, nu = dev(ids), dev(torch.tensor([ids.numel()], dtype=torch.int32))
            ug = dev(torch.ones(ids.numel(), D))
            dp, dm, dv, dg = (dev(torch.zeros(8)) for _ in range(4))
            L.call("amid_optimizer_step_f32", dp.data_ptr(), dm.data_ptr(), dv.data_ptr(), dg.data_ptr(), 8, tab.data_ptr(), m.data_ptr(),
                   v.data_ptr(), last.data_ptr(), uid.data_ptr(), nu.data_ptr(), ids.numel(), ug.data_ptr(), D, 1.0, st.data_ptr(), stream())
            torch.cuda.synchronize()
            res.append((xg.cpu(), tab.cpu(), m.cpu(), v.cpu(), last.cpu()))
        if live:           # only the live sequences' rows and the items are written
            n0 = int(lv.cpu()[B])
            keep = torch.zeros(idx.numel(), dtype=torch.bool)
            for j, b in enumerate(lv.cpu()[:B].tolist()):
                gdom = 0 if j < n0 else 1
                keep[gdom * B * T + b * T: gdom * B * T + (b + 1) * T] = True
            keep[2 * B * T:] = True
            assert torch.equal(res[0][0][keep], res[1][0][keep])
        else:
            assert torch.equal(res[0][0], res[1][0])
        for a, b in zip(res[0][1:], res[1][1:]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("with_transposes", [False, True])
def test_gather_with_weight_image_riders_equals_gather_and_image_launches(L, live, with_transposes):
    """amid_embed_fwd_w16_f32 (K1 whose extra workgroups write the step's three-plane bf16 images of the encoder weights and, optionally, of
    their transposes) against the launches it replaces: the gathered rows, mask bytes and compact index list bit for bit those of
    amid_embed_fwd_live_compact_f32 / amid_embed_fwd_f32, the images bit for bit those of amid_sas_weights_bf16_planes."""
    from amid_amd._lib import ptr_array
    B, T, D, NI, n_rows, n_w = 37, 50, 128, 2, 5000, 24
    g = torch.Generator().manual_seed(11)
    tab = dev(torch.randn(n_rows, D, generator=g))
    idx = torch.randint(0, n_rows - 1, (2 * B * T + B * NI,), generator=g).int()
    idx[torch.rand(idx.numel(), generator=g) < 0.4] = n_rows - 1
    idx = dev(idx)
    pos0, pos1 = dev(torch.randn(T, D, generator=g)), dev(torch.randn(T, D, generator=g))
    dom = dev((torch.rand(B, generator=g) < 0.5).long())
    lv = dev(torch.zeros(B + 1, dtype=torch.int32))
    L.call("amid_live_list_i32", dom.data_ptr(), B, lv.data_ptr(), stream())
    st = step_state(L, 5, 3)
    W = [dev(torch.randn(D, D, generator=g) * 10.0 ** float(-3 * torch.rand(1, generator=g))) for _ in range(n_w)]
    src = ptr_array([w.data_ptr() for w in W])
    outs = []
    for riders in (False, True):
        xg = dev(torch.zeros(idx.numel(), D))
        tmq = dev(torch.zeros(2 * B * T, D // 4, dtype=torch.uint8))
        ic, rc = dev(torch.full((idx.numel() + 1,), -7, dtype=torch.int32)), dev(torch.full((idx.numel(),), -7, dtype=torch.int32))
        img, imgT = (dev(torch.zeros(n_w, 3, D * D, dtype=torch.bfloat16)) for _ in range(2))
        lf, icp, rcp = (lv.data_ptr(), ic.data_ptr(), rc.data_ptr()) if live else (None, None, None)
        if riders:
            L.call("amid_embed_fwd_w16_f32", tab.data_ptr(), idx.data_ptr(), pos0.data_ptr(), pos1.data_ptr(), B, T, D, B * NI, xg.data_ptr(),
                   tmq.data_ptr(), st.data_ptr(), 1, 0.5, lf, icp, rcp, src, n_w, 3, img.data_ptr(),
                   imgT.data_ptr() if with_transposes else None, stream())
        else:
            if live:
                L.call("amid_embed_fwd_live_compact_f32", tab.data_ptr(), idx.data_ptr(), pos0.data_ptr(), pos1.data_ptr(), B, T, D, B * NI,
                       xg.data_ptr(), tmq.data_ptr(), st.data_ptr(), 1, 0.5, lf, icp, rcp, stream())
            else:
                L.call("amid_embed_fwd_f32", tab.data_ptr(), idx.data_ptr(), pos0.data_ptr(), pos1.data_ptr(), B, T, D, B * NI, xg.data_ptr(),
                       tmq.data_ptr(), st.data_ptr(), 1, 0.5, stream())
            L.call("amid_sas_weights_bf16_planes", src, n_w, D, 0, 3, img.data_ptr(), stream())
            if with_transposes:
                L.call("amid_sas_weights_bf16_planes", src, n_w, D, 1, 3, imgT.data_ptr(), stream())
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (xg, tmq, ic, rc)] + [img.cpu().view(torch.int16), imgT.cpu().view(torch.int16)])
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), k
    assert int(outs[1][4].ne(0).sum()) > n_w * D * D            # the images were written ...
    assert (int(outs[1][5].ne(0).sum()) > 0) == with_transposes  # ... the transposes' only when asked for


@pytest.mark.parametrize("shape", ["sasrec", "bert", "sasrec64"])       # sasrec64: head dim 8, pairs of heads per tile
@pytest.mark.parametrize("B", [5, 130, 1030])          # 1030 > 1024: the kernels keep the identity slot -> sequence mapping
def test_attention_bwd_rows_hint_equals_plain_backward(L, shape, B):
    """amid_attn_bwd_rows_f32 (the loss structure as a hint: the sequence (g, b) with g != row_domain[b] has an all-zero d_o) against
    amid_attn_bwd_f32 on the same inputs: bit-identical on the live sequences, exact zeros on the others."""
    T, D = 50, (64 if shape == "sasrec64" else 128)
    H, causal, p = (8, 1, 0.5) if shape.startswith("sasrec") else (4, 0, 0.1)
    g = torch.Generator().manual_seed(B)
    q, k, v, do = (dev(torch.randn(2 * B, T, D, generator=g)) for _ in range(4))
    dom = (torch.rand(B, generator=g) < 0.5).long()
    live = torch.cat((dom == 0, dom == 1))                      # [2B]: sequence g * B + b carries a gradient iff dom[b] == g
    do = do * dev(live.float())[:, None, None]
    keep = None
    if shape == "bert":
        keep = dev((torch.rand(B, T, generator=g) < 0.8).to(torch.uint8))
    kp = keep.data_ptr() if keep is not None else None
    st = step_state(L, 5, 9)
    o = torch.empty_like(q); stats = torch.empty(2 * B * T, H, 2, device="cuda")
    L.call("amid_attn_fwd_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), kp, B, T, D, H, causal, 0, st.data_ptr(), 1, p, o.data_ptr(),
           stats.data_ptr(), stream())
    outs = []
    for hint in (None, dev(dom)):
        dq, dk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), stats.data_ptr(), do.data_ptr(), kp, B, T, D, H, causal, 0, st.data_ptr(), 1, p,
                dq.data_ptr(), dk.data_ptr(), dv.data_ptr())
        if hint is None:
            L.call("amid_attn_bwd_f32", *args, stream())
        else:
            L.call("amid_attn_bwd_rows_f32", *args, hint.data_ptr(), stream())
        torch.cuda.synchronize()
        outs.append((dq.cpu(), dk.cpu(), dv.cpu()))
    for a, b_ in zip(*outs):
        assert torch.equal(a[live], b_[live])
        assert float(b_[~live].abs().max()) == 0.0 and float(a[~live].abs().max()) == 0.0


@pytest.mark.parametrize("B,T", [(6, 50), (37, 20), (256, 50), (1500, 8)])     # 1500: more sequences than one LDS window holds at once
def test_wgrad_rows_hint_equals_plain(L, B, T):
    """amid_sas_wgrad_rows_f32 (only the live sequences' rows are read) against amid_sas_wgrad_f32 on dY whose dead rows are zero:
    the sums over the splits agree to rounding (the rows are grouped into the splits differently)."""
    D, M, splits = 128, B * T, 5
    g = torch.Generator().manual_seed(B + T)
    dom = (torch.rand(B, generator=g) < 0.5).long()
    live = torch.cat((dom == 0, dom == 1)).float().repeat_interleave(T)          # [2M]
    dy = [dev(torch.randn(2 * M, D, generator=g) * live[:, None]) for _ in range(6)]
    xx = [dev(torch.randn(2 * M, D, generator=g)) for _ in range(6)]
    from amid_amd._lib import ptr_array
    outs = []
    for hint in (False, True):
        wp = torch.full((2, 6, splits, D * D), float("nan"), device="cuda"); bp = torch.full((2, 6, splits, D), float("nan"), device="cuda")
        args = (ptr_array([t.data_ptr() for t in dy]), ptr_array([t.data_ptr() for t in xx]), 1, M, D, splits, ptr_array([wp.data_ptr()]),
                ptr_array([bp.data_ptr()]))
        if hint:
            L.call("amid_sas_wgrad_rows_f32", *args, dev(dom).data_ptr(), B, T, 0, stream())
        else:
            L.call("amid_sas_wgrad_f32", *args, 0, stream())
        torch.cuda.synchronize()
        outs.append((wp.sum(2).cpu(), bp.sum(2).cpu()))
    for a, b_ in zip(*outs):
        assert torch.isfinite(b_).all()
        assert float((a - b_).abs().max()) < 2e-5 * float(a.abs().max())
    for gdom in range(2):          # against the plain definition dW = dY^T X
        want = dy[0][gdom * M:(gdom + 1) * M].double().t() @ xx[0][gdom * M:(gdom + 1) * M].double()
        assert relmax(outs[1][0][gdom, 0].view(D, D), want) < 1e-5


@pytest.mark.parametrize("B,T,hint", [(6, 50, True), (37, 20, False), (256, 50, True), (300, 33, True)])
def test_wgrad_bf16_products_against_fp32(L, B, T, hint):
    """amid_sas_wgrad(_rows)_f32 with mma_bf16 = 1 (compute = "bf16": operands rounded to bf16 on the way into LDS, fp32 accumulation)
    against the products of the bf16-ROUNDED operands in fp64 (what the kernel computes, up to fp32 summation order: 2e-5 of the largest
    entry) and against the fp32 products (bf16's rounding: 2e-2 relative in the L2 sense); the bias sums come from the unrounded rows."""
    D, M, splits = 128, B * T, 5
    g = torch.Generator().manual_seed(B * 3 + T)
    dom = (torch.rand(B, generator=g) < 0.5).long()
    live = torch.cat((dom == 0, dom == 1)).float().repeat_interleave(T) if hint else torch.ones(2 * M)
    dy = [dev(torch.randn(2 * M, D, generator=g) * live[:, None]) for _ in range(6)]
    xx = [dev(torch.randn(2 * M, D, generator=g)) for _ in range(6)]
    from amid_amd._lib import ptr_array
    wp = torch.full((2, 6, splits, D * D), float("nan"), device="cuda"); bp = torch.full((2, 6, splits, D), float("nan"), device="cuda")
    args = (ptr_array([t.data_ptr() for t in dy]), ptr_array([t.data_ptr() for t in xx]), 1, M, D, splits, ptr_array([wp.data_ptr()]),
            ptr_array([bp.data_ptr()]))
    if hint:
        L.call("amid_sas_wgrad_rows_f32", *args, dev(dom).data_ptr(), B, T, 1, stream())
    else:
        L.call("amid_sas_wgrad_f32", *args, 1, stream())
    torch.cuda.synchronize()
    got_w, got_b = wp.sum(2).cpu(), bp.sum(2).cpu()
    assert torch.isfinite(got_w).all() and torch.isfinite(got_b).all()
    for wi in range(6):
        for gdom in range(2):
            y, x = dy[wi][gdom * M:(gdom + 1) * M].cpu(), xx[wi][gdom * M:(gdom + 1) * M].cpu()
            exact = y.to(torch.bfloat16).double().t() @ x.to(torch.bfloat16).double()
            full = y.double().t() @ x.double()
            gw = got_w[gdom, wi].view(D, D).double()
            assert float((gw - exact).abs().max()) < 2e-5 * float(exact.abs().max()) + 1e-6, (wi, gdom)
            assert float((gw - full).norm() / full.norm()) < 2e-2
            assert float((gw - full).abs().max()) > 0.0                      # the mode is on
            assert float((got_b[gdom, wi].double() - y.double().sum(0)).abs().max()) < 1e-4 * max(1.0, float(y.abs().sum(0).max()))


def _wgrad_case(B, T, hint, n_ent, seed, spread=False):
    D, M = 128, B * T
    g = torch.Generator().manual_seed(seed)
    dom = (torch.rand(B, generator=g) < 0.5).long()
    live = torch.cat((dom == 0, dom == 1)).float().repeat_interleave(T) if hint else torch.ones(2 * M)

    def one(mask):
        t = torch.randn(2 * M, D, generator=g)
        if spread:                                    # magnitudes over six decades, as gradients have them
            t = t * torch.pow(10.0, -6.0 * torch.rand(2 * M, D, generator=g))
        return dev(t * live[:, None] if mask else t)
    return dom, [one(True) for _ in range(n_ent)], [one(False) for _ in range(n_ent)]


def _wgrad_run(L, dy, xx, dom, B, T, splits, mode, hint):
    from amid_amd._lib import ptr_array
    D, M, nl = 128, B * T, len(dy) // 6
    wp = [torch.full((2, 6, splits, D * D), float("nan"), device="cuda") for _ in range(nl)]
    bp = [torch.full((2, 6, splits, D), float("nan"), device="cuda") for _ in range(nl)]
    args = (ptr_array([t.data_ptr() for t in dy]), ptr_array([t.data_ptr() for t in xx]), nl, M, D, splits,
            ptr_array([t.data_ptr() for t in wp]), ptr_array([t.data_ptr() for t in bp]))
    if hint:
        L.call("amid_sas_wgrad_rows_f32", *args, dev(dom).data_ptr(), B, T, mode, stream())
    else:
        L.call("amid_sas_wgrad_f32", *args, mode, stream())
    torch.cuda.synchronize()
    return [w.double().sum(2) for w in wp], [b_.double().sum(2) for b_ in bp]


@pytest.mark.parametrize("B,T,hint,spread", [(6, 50, True, False), (37, 20, False, True), (256, 50, True, True), (300, 33, True, False),
                                              (1500, 8, True, False), (3, 7, False, False)])
def test_wgrad_split_products_have_fp32_accuracy(L, B, T, hint, spread):
    """amid_sas_wgrad(_rows)_f32 in modes 2 and 3 (compute = "fp32": every operand as three bf16 pieces, nine / six piece pairs on
    v_mfma_f32_16x16x32_bf16) against the fp64 product dY^T X: within 1e-6 of the largest entry, and no worse than 1.5 x the error of
    mode 0 (the fp32 matrix instructions) on the same operands + 1e-7; bias sums as mode 0's."""
    D, M, splits = 128, B * T, 5
    dom, dy, xx = _wgrad_case(B, T, hint, 6, B * 5 + T, spread)
    want = [[dy[wi][gd * M:(gd + 1) * M].double().t() @ xx[wi][gd * M:(gd + 1) * M].double() for gd in range(2)] for wi in range(6)]
    errs = {}
    for mode in (0, 2, 3):
        (w,), (b_,) = _wgrad_run(L, dy, xx, dom, B, T, splits, mode, hint)
        assert torch.isfinite(w).all() and torch.isfinite(b_).all()
        errs[mode] = max(float((w[gd, wi].view(D, D) - want[wi][gd]).abs().max() / want[wi][gd].abs().max().clamp_min(1e-30))
                         for wi in range(6) for gd in range(2))
        for wi in range(6):
            for gd in range(2):
                y = dy[wi][gd * M:(gd + 1) * M].double()
                assert float((b_[gd, wi] - y.sum(0)).abs().max()) < 1e-4 * max(1.0, float(y.abs().sum(0).max()))
    assert errs[2] < 1e-6 and errs[3] < 1e-6, errs
    assert errs[2] <= 1.5 * errs[0] + 1e-7 and errs[3] <= 1.5 * errs[0] + 1e-7, errs


@pytest.mark.parametrize("mode", [2, 3])
def test_wgrad_split_two_workgroups_per_cu_repeated(L, mode):
    """The train step's launch shape (2 layers x 6 weights x 21 splits x 2 domains = 504 workgroups, two per CU, B 256 x T 50 with the
    live-row hint), 25 times over: every one of the 24 summed gradients within 2e-6 of the fp64 product each time (a build of this
    kernel that zeroed the rows past a split's end by multiplication failed this in 239 of 240 launches, csrc/sasrec_bwd.hip)."""
    B, T, D, splits = 256, 50, 128, 21
    M = B * T
    dom, dy, xx = _wgrad_case(B, T, True, 12, 99)
    want = [[dy[wi][gd * M:(gd + 1) * M].double().t() @ xx[wi][gd * M:(gd + 1) * M].double() for gd in range(2)] for wi in range(12)]
    for rep in range(25):
        w, _ = _wgrad_run(L, dy, xx, dom, B, T, splits, mode, True)
        for wi in range(12):
            for gd in range(2):
                e = float((w[wi // 6][gd, wi % 6].view(D, D) - want[wi][gd]).abs().max() / want[wi][gd].abs().max())
                assert e < 2e-6, (rep, wi, gd, e)


@pytest.mark.parametrize("B,T,hint", [(8, 50, True), (37, 20, False), (256, 50, True)])
def test_bert_wgrad_modes_against_fp64(L, B, T, hint):
    """amid_bert_wgrad_mode_f32 -- BERT4Rec's twelve 128 x 128 weight-gradient tiles of a block (q, k, v, out-projection; four column
    tiles of w_1 [512, 128] read dY with row stride 512; four of w_2 [128, 512] read X with row stride 512 and land side by side in one
    [128, 512] partial) -- in mode 0 (fp32 matrix instructions) and modes 2 / 3 (three bf16 pieces per operand, nine / six piece pairs):
    every summed tile and bias within 2e-6 of the fp64 product's largest entry (1280-row splits: mode 0 measures 1.2e-6, modes 2 / 3
    8.7e-7), modes 2 / 3 no worse than 1.5 x mode 0 + 1e-7."""
    import ctypes
    from amid_amd._lib import ptr_array
    D, F, M, splits, N = 128, 512, B * T, 5, 12
    g = torch.Generator().manual_seed(B + 7 * T)
    dom = (torch.rand(B, generator=g) < 0.5).long()
    live = (torch.cat((dom == 0, dom == 1)).float().repeat_interleave(T) if hint else torch.ones(2 * M))[:, None]
    dq, dk, dv, dt, dz = (dev(torch.randn(2 * M, D, generator=g) * live) for _ in range(5))
    dpre = dev(torch.randn(2 * M, F, generator=g) * live)
    y, o, y2 = (dev(torch.randn(2 * M, D, generator=g)) for _ in range(3))
    h = dev(torch.randn(2 * M, F, generator=g))
    dy = [dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dt.data_ptr()]; xx = [y.data_ptr()] * 3 + [o.data_ptr()]
    pairs = [(dq, y), (dk, y), (dv, y), (dt, o)]
    ldy, ldx = [D] * 4, [D] * 4
    old, ogr, oco = [D] * 8 + [F] * 4, list(range(8)) + [8] * 4, [0] * 8 + [c * D for c in range(4)]
    for c in range(4):
        dy.append(dpre.data_ptr() + 4 * c * D); xx.append(y2.data_ptr()); ldy.append(F); ldx.append(D); pairs.append((dpre[:, c * D:(c + 1) * D], y2))
    for c in range(4):
        dy.append(dz.data_ptr()); xx.append(h.data_ptr() + 4 * c * D); ldy.append(D); ldx.append(F); pairs.append((dz, h[:, c * D:(c + 1) * D]))
    ci = lambda v: (ctypes.c_int * N)(*v)
    errs = {}
    for mode in (0, 2, 3):
        wp = torch.full((2, N, splits, D * D), float("nan"), device="cuda"); bp = torch.full((2, N, splits, D), float("nan"), device="cuda")
        L.call("amid_bert_wgrad_mode_f32", ptr_array(dy), ptr_array(xx), ci(ldy), ci(ldx), ci(old), ci(ogr), ci(oco), N, M, splits,
               wp.data_ptr(), bp.data_ptr(), dev(dom).data_ptr() if hint else None, B, T, mode, stream())
        torch.cuda.synchronize()
        worst = 0.0
        for e, (a_, b_) in enumerate(pairs):
            for gd in range(2):
                want = a_[gd * M:(gd + 1) * M].double().t() @ b_[gd * M:(gd + 1) * M].double()
                if e < 8:
                    got = wp[gd, e].double().sum(0).view(D, D)
                else:                                 # the four w_2 tiles share one [splits][128][512] partial starting at entry 8
                    got = wp[gd, 8:12].reshape(splits, D, F).double().sum(0)[:, (e - 8) * D:(e - 7) * D]
                assert torch.isfinite(got).all(), (mode, e, gd)
                worst = max(worst, float((got - want).abs().max() / want.abs().max().clamp_min(1e-30)))
                bs = a_[gd * M:(gd + 1) * M].double().sum(0)
                assert float((bp[gd, e].double().sum(0) - bs).abs().max()) < 1e-4 * max(1.0, float(a_.abs().sum(0).max())), (mode, e, gd)
        errs[mode] = worst
    assert all(v < 2e-6 for v in errs.values()), errs
    assert errs[2] <= 1.5 * errs[0] + 1e-7 and errs[3] <= 1.5 * errs[0] + 1e-7, errs


@pytest.mark.parametrize("n,world,D", [(1, 2, 64), (300, 2, 128), (5000, 4, 128), (70000, 8, 128), (2049, 16, 64), (777, 3, 128)])
def test_owner_buckets_equal_torch_split(L, n, world, D):
    """amid_owner_count_i32 / amid_owner_buckets_f32 (the split of the owner-bucketed exchange) against the
    protocol's torch double (amid_amd.dist.TorchMergeBackend): counts, ids and rows bit-exact, sentinel + zero rows in the unused
    slots, the overflow flag when the bound is too small."""
    from amid_amd.dist import TorchMergeBackend, packed_rows
    g = torch.Generator().manual_seed(n)
    n_rows = 1_000_003
    cap = n + 37
    ids = torch.sort(torch.randperm(n_rows, generator=g)[:n]).values.to(torch.int32)
    ids_full = torch.cat((ids, torch.full((cap - n,), 12345, dtype=torch.int32)))          # garbage beyond n_uniq
    rows = torch.randn(cap, D, generator=g)
    want_cnt = torch.bincount(ids.long() % world, minlength=world)
    bmax = (int(want_cnt.max()) + 63) // 64 * 64
    d_ids, d_rows, d_n = ids_full.cuda(), rows.cuda(), torch.tensor([n], dtype=torch.int32).cuda()
    ws = torch.empty(L.value("amid_owner_workspace_bytes", cap), dtype=torch.uint8, device="cuda")
    cnt = torch.full((17,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L.call("amid_owner_count_i32", d_ids.data_ptr(), d_n.data_ptr(), cap, world, ws.data_ptr(), cnt.data_ptr(), s)
    assert cnt[:world].cpu().tolist() == want_cnt.tolist() and int(cnt[world]) == 0
    id_rows, tot = packed_rows(bmax, D)
    out = torch.full((world, tot * D), 7.0, device="cuda")
    L.call("amid_owner_buckets_f32", d_ids.data_ptr(), d_rows.data_ptr(), d_n.data_ptr(), cap, D, world, bmax, n_rows, ws.data_ptr(),
           out.data_ptr(), tot * D, id_rows, cnt.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(cnt[world]) == 0
    out = out.cpu()
    got_ids = out[:, :bmax].contiguous().view(torch.int32)
    got_rows = out[:, id_rows * D:].reshape(world, bmax, D)
    for o in range(world):
        sel = (ids.long() % world) == o
        k = int(sel.sum())
        assert torch.equal(got_ids[o, :k], ids[sel]) and bool((got_ids[o, k:] == n_rows).all())
        assert torch.equal(got_rows[o, :k], rows[:n][sel]) and float(got_rows[o, k:].abs().sum()) == 0.0
    if int(want_cnt.max()) > 1:                                     # a bound that is too small: flagged, nothing out of range
        small = int(want_cnt.max()) - 1
        id_rows2, tot2 = packed_rows(small, D)
        out2 = torch.full((world, tot2 * D + 64), 7.0, device="cuda")
        L.call("amid_owner_count_i32", d_ids.data_ptr(), d_n.data_ptr(), cap, world, ws.data_ptr(), cnt.data_ptr(), s)
        L.call("amid_owner_buckets_f32", d_ids.data_ptr(), d_rows.data_ptr(), d_n.data_ptr(), cap, D, world, small, n_rows, ws.data_ptr(),
               out2.data_ptr(), tot2 * D + 64, id_rows2, cnt.data_ptr(), s)
        torch.cuda.synchronize()
        assert int(cnt[world]) == 1 and bool((out2[:, tot2 * D:] == 7.0).all())
