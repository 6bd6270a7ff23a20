"""The backward strips in the N-split build on bf16 pieces (csrc/sasrec_strip_px.hip; products mode 4 of the strip entry points,
SasrecEngine.STRIP_NSPLIT): eight waves per 64-row tile, two per SIMD, each owning half the output columns.

Kernel level: against the strip build (mode 3) on the same three-plane weight images -- every saved tensor and the LayerNorm partial sums
of live strips within 4e-6 of the tensor's largest entry (the project's bar for pieces against fp32 instructions), the NaN pattern of
untouched rows and slots equal, the same bits on three repetitions.  Beyond that bar: the build performs the strip build's operations in
its order, so without the forward's row statistics (which the forward adds part by part) it gives the strip build's BITS, held here too.
Step level: the engine's step on a pool with the switch on and off -- the first loss and every gradient bit-equal, each build inside the
oracle bars of test_gpu_timed_path._timed_vs_oracle, the launch list naming mode 4 (profiles/strip_nsplit.md).  The sort riders (phases 2, 3, 4 on a rider workgroup's first four waves) are covered at step level, on
a pool that is not prepared: the plan's buffers are then the engine's own."""
import pytest
import torch

from oracle import amid_oracle as orc
from tests.test_gpu_strip import Ctx
from tests.test_gpu_timed_path import (check_grads, dense_table_grad, gpu_relu_keep, log, make_engine, relmax, split_batch,
                                       timed_pool_step)

pytestmark = pytest.mark.gpu

D = 128
BAR = 4e-6


def set_domains(c, dom):
    """The context's live list for the given domain of every sequence."""
    c.dom = torch.as_tensor(dom).long()
    d0, d1 = torch.nonzero(c.dom == 0).flatten(), torch.nonzero(c.dom != 0).flatten()
    c.live = torch.cat((d0, d1, torch.tensor([d0.numel()]))).int().cuda()
    c.row_live = torch.cat((c.dom == 0, c.dom != 0)).repeat_interleave(c.T)


def context(B, T, live):
    if live in (None, "mixed", "all0"):
        c = Ctx(B, T, D, seed=B * 13 + T, live=live)
        if live == "mixed" and B == 3:
            set_domains(c, [0, 1, 0])                    # the embedding-epilogue test's list: both domains on it
        return c
    c = Ctx(B, T, D, seed=B * 13 + T, live="mixed")
    assert live == "one1"                                # domain 1 holds exactly one live sequence
    dom = torch.zeros(B, dtype=torch.long)
    dom[B // 2] = 1
    set_domains(c, dom)
    return c


class Case:
    """Operands of the three launches of a two-layer backward, shared by both builds."""

    def __init__(self, B, T, live):
        c = self.c = context(B, T, live)
        pa = c.pa
        lo = c.live is not None
        self.P = lambda t: pa([t[0].data_ptr(), t[1].data_ptr()])
        self.lnw = c.vec(1.0)
        self.dxo, self.h, self.r = c.act(live_only=lo), c.act().relu(), c.act()
        self.dq, self.dk, self.dv, self.dr = (c.act(live_only=lo) for _ in range(4))
        self.x = c.act()
        mats = [c.mat() for _ in range(6)]               # w1T, w2T, woT, wqT, wkT, wvT: W^T [in][out] per domain
        self.img = torch.empty(12, 3, D * D, dtype=torch.bfloat16, device="cuda")
        c.L.call("amid_sas_weights_bf16_planes", pa([m[g].data_ptr() for m in mats for g in (0, 1)]), 12, D, 0, 3, self.img.data_ptr(), c.s)
        self.I = lambda k: pa([self.img[2 * k].data_ptr(), self.img[2 * k + 1].data_ptr()])
        # the forward's row statistics: LayerNorm 1 over x at +0, LayerNorm 2 over r at +2
        self.stat = torch.zeros(2 * c.M, 4, device="cuda")
        for col, t in ((0, self.x), (2, self.r)):
            mean = t.mean(1)
            self.stat[:, col] = mean
            self.stat[:, col + 1] = 1.0 / torch.sqrt(((t - mean[:, None]) ** 2).mean(1) + 1e-8)

    def part(self):
        return torch.full((2 * self.c.stpg, 2, D), float("nan"), device="cuda")

    def qkv_head(self):
        I, c = self.I, self.c
        return (self.dq.data_ptr(), self.dk.data_ptr(), self.dv.data_ptr(), self.dr.data_ptr(), self.x.data_ptr(), self.P(self.lnw), I(3), I(4), I(5),
                1e-8, c.B, c.T, D, c.lp())

    def ffn_block(self, out, pg):
        c, I = self.c, self.I
        return (c.tmq.data_ptr(), self.h.data_ptr(), self.r.data_ptr(), self.P(self.lnw), I(0), I(1), I(2), 0, c.st.data_ptr(), 1, 0.5,
                *[t.data_ptr() for t in out], pg.data_ptr())

    def run(self, mode, stat=False, scorer=None):
        """The launches of one build -> ([saved tensors], [partial sums]).  mode 3: the strip build; 4: the N-split build through the strip
        entries; "px": the N-split build through its own entries (stat: with the forward's row statistics)."""
        c, L, s, I = self.c, self.c.L, self.c.s, self.I
        st = self.stat.data_ptr() if stat else None
        no_ffn = (*([None] * 7), 0, None, 0, 0.0, *([None] * 5))
        no_scorer = (None, None, None, 0, 0, None, None, None, None)
        out, pg = [c.out() for _ in range(4)], self.part()
        ffn = (self.dxo.data_ptr(), c.tmq.data_ptr(), self.h.data_ptr(), self.r.data_ptr(), self.P(self.lnw), I(0), I(1), I(2), 1e-8, c.B, c.T, D,
               c.lp(), 1, c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out], pg.data_ptr())
        if mode == "px":
            L.call("amid_sas_strip_ffn_bwd_px_f32", *ffn, st, None, 0, s)
        else:
            L.call("amid_sas_strip_ffn_bwd_f32", *ffn, mode, s)
        dx, pg1 = c.out(), self.part()                   # q / k / v alone
        out2, pg2, fpg2 = [c.out() for _ in range(4)], self.part(), self.part()      # ... with the layer below's feed-forward chain
        emb = [(c.out(), self.part()) for _ in range(2)]                              # ... with the embedding epilogue, dropout on / off
        if mode == "px":
            L.call("amid_sas_strip_qkv_bwd_px_f32", *self.qkv_head(), dx.data_ptr(), pg1.data_ptr(), *no_ffn, None, 0.0, st, None, None, 0, *no_scorer, s)
            L.call("amid_sas_strip_qkv_bwd_px_f32", *self.qkv_head(), None, pg2.data_ptr(), *self.ffn_block(out2, fpg2), None, 0.0, st, st, None, 0,
                   *(scorer if scorer is not None else no_scorer), s)
            for train, (e, pe) in zip((1, 0), emb):
                L.call("amid_sas_strip_qkv_bwd_px_f32", *self.qkv_head(), e.data_ptr(), pe.data_ptr(), *([None] * 7), 0, c.st.data_ptr(), train, 0.0,
                       *([None] * 5), c.tmq.data_ptr(), 0.5, st, None, None, 0, *no_scorer, s)
        else:
            L.call("amid_sas_strip_qkv_bwd_f32", *self.qkv_head(), dx.data_ptr(), pg1.data_ptr(), *no_ffn, mode, s)
            if scorer is not None:
                L.call("amid_sas_strip_qkv_bwd_scorer_f32", *self.qkv_head(), pg2.data_ptr(), *self.ffn_block(out2, fpg2), mode, *scorer, s)
            else:
                L.call("amid_sas_strip_qkv_bwd_f32", *self.qkv_head(), None, pg2.data_ptr(), *self.ffn_block(out2, fpg2), mode, s)
            for train, (e, pe) in zip((1, 0), emb):
                L.call("amid_sas_strip_qkv_bwd_emb_f32", *self.qkv_head(), e.data_ptr(), pe.data_ptr(), c.tmq.data_ptr(), c.st.data_ptr(), train, 0.5,
                       None, 0, mode, s)
        torch.cuda.synchronize()
        return out + [dx] + out2 + [e for e, _ in emb], [pg, pg1, pg2, fpg2] + [pe for _, pe in emb]

    def compare(self, tag, got, ref):
        rl = self.c.row_live.cuda()
        worst = 0.0
        for i, (a, b) in enumerate(zip(got[0], ref[0])):
            assert torch.equal(torch.isnan(a), torch.isnan(b)), (tag, i, "rows outside the live list")
            a, b = a[rl].double(), b[rl].double()
            assert torch.isfinite(a).all(), (tag, i)
            e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
            worst = max(worst, e)
            assert e < BAR, (tag, "tensor", i, e)
        for i, (a, b) in enumerate(zip(got[1], ref[1])):
            ok = torch.isfinite(b)
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool((torch.isfinite(a) == ok).all()), (tag, i, "slots of dead strips")
            a, b = a[ok].double(), b[ok].double()
            e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
            worst = max(worst, e)
            assert e < BAR, (tag, "ln_part", i, e)
        return worst

    @staticmethod
    def same_bits(tag, a, b):
        for i, (u, v) in enumerate(zip(a[0] + a[1], b[0] + b[1])):
            assert torch.equal(torch.nan_to_num(u, nan=-1.0), torch.nan_to_num(v, nan=-1.0)), (tag, i)


# B, T: B T no multiple of 64; the headline tile geometry; many tiles; a single short batch; the embedding-epilogue test's shapes
SHAPES = [(37, 20), (64, 50), (300, 33), (5, 64), (3, 12), (3, 40)]
LISTS = [(B, T, live) for (B, T) in SHAPES for live in (None, "mixed")] + [(64, 50, "all0"), (37, 20, "all0"), (64, 50, "one1"), (37, 20, "one1")]


@pytest.mark.parametrize("B,T,live", LISTS)
def test_n_split_kernels_match_the_strip_build(B, T, live):
    """The three launches (feed-forward chain; q / k / v chain alone, with the fused feed-forward chain, with the embedding epilogue under
    dropout and without) in the N-split build -- through the strip entries' mode 4 (row statistics from the rows) and through the build's
    own entries with the forward's row statistics -- against the strip build."""
    k = Case(B, T, live)
    ref = k.run(3)
    for tag, kw in (("mode 4", dict(mode=4)), ("px + ln_stat", dict(mode="px", stat=True)), ("px", dict(mode="px"))):
        got = k.run(**kw)
        w = k.compare(f"{tag} B={B} T={T} {live}", got, ref)
        print(f"NSPLIT {tag} B={B} T={T} live={live}: worst distance {w:.2e} of the largest entry")
        if "ln_stat" not in tag:                         # same operations in the same order: the strip build's bits
            k.same_bits((tag, "strip build"), got, ref)
        if tag != "px":
            for rep in range(3):
                k.same_bits((tag, rep), k.run(**kw), got)
    # the embedding epilogue did mask and drop: zeros and non-zeros among the live rows
    rl = k.c.row_live.cuda()
    e_train = got[0][-2][rl]
    assert bool((e_train == 0).any()) and bool((e_train != 0).any())


# the scorer sums' workgroups behind the tiles, and in front: the smallest batch for which ScorerSum::front is set (B 1024), T 17
@pytest.mark.parametrize("B,T", [(64, 50), (1024, 17)])
def test_n_split_fused_launch_carries_the_scorer_sums(B, T):
    k = Case(B, T, "mixed")
    c = k.c
    NI, hid = 2, 32
    HG = ((3 + NI) * hid + 1 + 3) & ~3
    g = torch.Generator().manual_seed(5)
    hidg = torch.randn(B, HG, generator=g).cuda()
    u, items = torch.randn(2, B, D, generator=g).cuda(), torch.randn(B, NI, D, generator=g).cuda()

    def sums():
        return [torch.full(n, float("nan"), device="cuda") for n in ((hid, 2 * D), (hid,), (hid,), (1,))]

    def run(mode):
        o = sums()
        sc = (hidg.data_ptr(), u.data_ptr(), items.data_ptr(), NI, hid, *[t.data_ptr() for t in o])
        return k.run(mode, scorer=sc), o

    ref, sref = run(3)
    for mode in (4, "px"):
        got, sgot = run(mode)
        k.compare(f"scorer {mode} B={B}", got, ref)
        k.same_bits(("scorer", mode), got, ref)
        for a, b in zip(sgot, sref):                     # the riders are the same code on the same operands
            assert torch.isfinite(a).all() and torch.equal(a, b), mode
    db1 = (hidg[:, :hid] + hidg[:, hid:2 * hid]).double().sum(0)      # (db1 restated: the riders did run)
    assert relmax(sref[1], db1) < 1e-5


def run_step(P, batch, T, nsplit, prepared):
    """One step on a pool as bench.py runs it -> the engine, the plan, the launches' (name, arguments)."""
    from amid_amd._lib import lib
    from amid_amd.engine import SasrecEngine
    seed, step = 21, 4
    old = SasrecEngine.STRIP_NSPLIT
    SasrecEngine.STRIP_NSPLIT = 7 if nsplit else 0
    L = lib()
    calls, orig = [], L.call

    def spy(name, *a):
        calls.append((name, a))
        return orig(name, *a)
    try:
        eng = make_engine(P, T, seed=seed)
        eng.PREPARED_POOL = prepared
        pl = eng.plan(batch["seq_d1"].shape[0], T, 2, need_grad=True)
        L.call = spy
        timed_pool_step(eng, pl, batch, step, seed)
    finally:
        L.call = orig
        SasrecEngine.STRIP_NSPLIT = old
    assert pl.tail2, "the shape was chosen to take the folded step"
    return eng, pl, calls


def strip_modes(calls):
    """The products-mode argument of the three backward strip launches, top down."""
    out = []
    for name, a in calls:
        if name in ("amid_sas_strip_ffn_bwd_f32", "amid_sas_strip_ffn_bwd_sort_f32", "amid_sas_strip_qkv_bwd_emb_f32"):
            out.append((name, a[-2]))
        elif name in ("amid_sas_strip_qkv_bwd_scorer_f32", "amid_sas_strip_qkv_bwd_sort_scorer_f32"):
            out.append((name, a[-11]))
    return out


@pytest.mark.parametrize("Bn,T", [(256, 50), (37, 47)])
@pytest.mark.parametrize("prepared", [True, False])      # False: the three launches carry the sort's phases 2, 3, 4 as riders
def test_step_with_the_n_split_strips_against_the_strip_build_and_the_oracle(Bn, T, prepared):
    hid, n_items = 32, 3000
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=300 + D + Bn)
    batch = split_batch(Bn, T, n_items, seed=Bn + T, split="mixed")
    masks = orc.philox_masks_sasrec(Bn, T, D, seed=21, step=4)
    rec = {}
    for nsplit in (False, True):
        eng, pl, calls = run_step(P, batch, T, nsplit, prepared)
        modes = strip_modes(calls)
        assert len(modes) == 3 and all(m == (4 if nsplit else 3) for _, m in modes), modes
        assert all(("_sort" in n) == (not prepared) for n, _ in modes[:2]), modes
        tag = f"nsplit={int(nsplit)} prepared={int(prepared)} B={Bn} T={T}"
        keep = gpu_relu_keep(eng, pl, batch)
        taps = {}
        loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, masks, relu_keep=keep, taps=taps)
        flips = [taps[s].get(f"relu_flip{l}", 0.0) for s in ("sac1", "sac2") for l in (0, 1)]
        assert max(flips) < 2e-5
        assert abs(float(pl.loss.item()) - float(loss)) < 1e-5 * max(1.0, abs(float(loss)))
        dom = batch["domain_id"]
        own = torch.where(dom[:, None] == 0, pl.p1.cpu(), pl.p2.cpu())
        assert relmax(own, torch.where(dom[:, None] == 0, p1, p2)) < 1e-4
        check_grads(f"strip_nsplit {tag}", eng, pl, grads, 2e-4, 5e-5)
        U = int(pl.n_uniq.item())
        rec[nsplit] = dict(loss=float(pl.loss.item()), table=dense_table_grad(eng, pl), uniq=pl.uniq_ids[:U].cpu().clone(),
                           **{name: eng.dense.view(name, eng.dense.grad).cpu().clone() for name in eng.dense.slots})
    a, b = rec[False], rec[True]
    assert a["loss"] == b["loss"]                        # the forward is the same
    assert torch.equal(a["uniq"], b["uniq"])             # the step's sort, riders or not
    dist = {name: relmax(b[name], want) for name, want in a.items() if name not in ("loss", "uniq")}
    for name, want in a.items():                         # the strips give the same bits in either build, so the step does
        if name not in ("loss", "uniq"):
            assert torch.equal(b[name], want), name
    worst = max(dist, key=dist.get)
    log(f"strip_nsplit on/off prepared={int(prepared)} B={Bn} T={T}: worst gradient distance {dist[worst]:.3e} ({worst}); "
        + " ".join(f"{k.split('.')[-2][:6]}.{k.split('.')[-1][:1]}:{v:.1e}" for k, v in sorted(dist.items()) if "." in k))
    print(f"NSPLIT step on/off prepared={int(prepared)} B={Bn} T={T}: worst {dist[worst]:.3e} ({worst})")
