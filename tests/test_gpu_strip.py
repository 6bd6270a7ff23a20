"""The register-resident strip GEMM kernels (csrc/sasrec_strip.hip) against the row-tile kernels (csrc/sasrec_fwd.hip /
sasrec_bwd.hip, themselves checked against the oracle and the reference goldens in test_gpu_sasrec.py) on the same inputs, through
the C ABI: every saved tensor / gradient to rounding (the two sum over k in different orders), LayerNorm partial sums per domain,
with and without the live-sequence list (rows of sequences outside the list must stay untouched)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 50, 128), (37, 20, 128), (5, 7, 64), (256, 50, 128), (300, 50, 64), (1, 1, 128)]


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


class Ctx:
    def __init__(self, B, T, D, seed, live):
        from amid_amd._lib import lib, ptr_array
        self.L, self.pa = lib(), ptr_array
        self.B, self.T, self.D, self.M = B, T, D, B * T
        self.g = torch.Generator().manual_seed(seed)
        self.s = torch.cuda.current_stream().cuda_stream
        host = (ctypes.c_ubyte * self.L.value("amid_step_state_bytes"))()
        self.L.call("amid_step_state_pack", ctypes.addressof(host), 11, 6, 5e-4, 0.9, 0.999, 1e-8)
        self.st = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
        self.rpt = self.L.value("amid_rows_per_tile", self.M)
        self.tpg = -(-self.M // self.rpt)
        self.stile = self.L.value("amid_sas_strip_tile_rows")
        self.stpg = -(-self.M // self.stile)
        self.dom = (torch.rand(B, generator=self.g) < 0.5).long()
        if live == "all0":
            self.dom[:] = 0
        self.live = None
        self.row_live = torch.ones(2 * self.M, dtype=torch.bool)
        if live:
            d0, d1 = torch.nonzero(self.dom == 0).flatten(), torch.nonzero(self.dom != 0).flatten()
            self.live = torch.cat((d0, d1, torch.tensor([d0.numel()]))).int().cuda()
            self.row_live = torch.cat((self.dom == 0, self.dom != 0)).repeat_interleave(T)
        self.tmq = ((torch.rand(2 * self.M, D // 4, generator=self.g) < 0.03).to(torch.uint8) * 5).cuda()

    def act(self, scale=1.0, live_only=False):
        t = torch.randn(2 * self.M, self.D, generator=self.g) * scale
        if live_only:
            t = t * self.row_live[:, None]
        return t.cuda()

    def vec(self, base=0.0):
        return ((base + 0.1 * torch.randn(self.D, generator=self.g)).cuda(), (base + 0.1 * torch.randn(self.D, generator=self.g)).cuda())

    def mat(self, rows=1):
        D = self.D
        return ((0.1 * torch.randn(rows * D, D, generator=self.g)).cuda(), (0.1 * torch.randn(rows * D, D, generator=self.g)).cuda())

    def out(self):
        return torch.full((2 * self.M, self.D), float("nan"), device="cuda")

    def lp(self):
        return self.live.data_ptr() if self.live is not None else None

    def check_rows(self, tag, got, want, tol=3e-6):
        rl = self.row_live
        assert torch.isfinite(got[rl.cuda()]).all(), tag
        e = relmax(got.cpu()[rl], want.cpu()[rl])
        assert e < tol, (tag, e)
        if self.live is not None and bool((~rl).any()):
            assert torch.isnan(got.cpu()[~rl]).all(), f"{tag}: rows outside the live list were written"

    def check_parts(self, tag, strip_part, tile_part, tol=2e-5):
        D = self.D
        a = strip_part.cpu().reshape(2, self.stpg, 2, D).double().sum(1)
        b = tile_part.cpu().reshape(2, self.tpg, 2, D).double().sum(1)
        assert torch.isfinite(a).all(), tag
        assert float((a - b).abs().max()) < tol * float(b.abs().max() + 1e-30), (tag, float((a - b).abs().max()), float(b.abs().max()))


@pytest.mark.parametrize("B,T,D", SHAPES)
@pytest.mark.parametrize("live", [None, "mixed", "all0"])
def test_strip_forward_equals_row_tile_kernels(B, T, D, live):
    c = Ctx(B, T, D, seed=B * 7 + T, live=live)
    L, pa, s, M = c.L, c.pa, c.s, c.M
    P = lambda t: pa([t[0].data_ptr(), t[1].data_ptr()])      # noqa: E731
    x = c.act()
    lnw, lnb, w_in = c.vec(1.0), c.vec(), c.mat(3)
    b_in = ((0.1 * torch.randn(3 * D, generator=c.g)).cuda(), (0.1 * torch.randn(3 * D, generator=c.g)).cuda())
    # ---- LN1 + q / k / v
    ref = [c.out() for _ in range(4)]
    L.call("amid_sas_qkv_fwd_f32", x.data_ptr(), P(lnw), P(lnb), P(w_in), P(b_in), 1e-8, M, D, c.rpt, *[t.data_ptr() for t in ref], 0, s)
    got = [c.out() for _ in range(4)]
    L.call("amid_sas_strip_qkv_fwd_f32", x.data_ptr(), P(lnw), P(lnb), P(w_in), P(b_in), 1e-8, B, T, D, c.lp(), *[t.data_ptr() for t in got], s)
    torch.cuda.synchronize()
    for n, a, b in zip("qn q k v".split(), got, ref):
        c.check_rows(f"qkv_fwd {n}", a, b)
    # ---- out-projection + LN2 + feed-forward (dropout on), alone and with the next layer's q / k / v behind it
    o, qn = c.act(), c.act()
    w_o, b_o, ln2w, ln2b, w1, b1, w2, b2 = c.mat(), c.vec(), c.vec(1.0), c.vec(), c.mat(), c.vec(), c.mat(), c.vec()
    for nxt in (False, True):
        for train in (0, 1):
            ref = [c.out() for _ in range(4)]
            refn = [c.out() for _ in range(4)]
            got = [c.out() for _ in range(4)]
            gotn = [c.out() for _ in range(4)]
            common = (o.data_ptr(), qn.data_ptr(), P(w_o), P(b_o), P(ln2w), P(ln2b), P(w1), P(b1), P(w2), P(b2), c.tmq.data_ptr(), 1e-8)
            if nxt:
                L.call("amid_sas_oproj_ffn_qkv_fwd_f32", *common, M, D, c.rpt, 1, c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in ref],
                       P(lnw), P(lnb), P(w_in), P(b_in), *[t.data_ptr() for t in refn], 0, s)
                L.call("amid_sas_strip_oproj_ffn_fwd_f32", *common, B, T, D, c.lp(), 1, c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in got],
                       P(lnw), P(lnb), P(w_in), P(b_in), *[t.data_ptr() for t in gotn], s)
            else:
                L.call("amid_sas_oproj_ffn_fwd_f32", *common, M, D, c.rpt, 1, c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in ref], 0, s)
                L.call("amid_sas_strip_oproj_ffn_fwd_f32", *common, B, T, D, c.lp(), 1, c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in got],
                       None, None, None, None, None, None, None, None, s)
            torch.cuda.synchronize()
            for n, a, b in zip("r y h xo".split(), got, ref):
                c.check_rows(f"oproj_ffn next={nxt} train={train} {n}", a, b)
            if nxt:
                for n, a, b in zip("qn q k v".split(), gotn, refn):
                    c.check_rows(f"fused next-layer {n} train={train}", a, b)


@pytest.mark.parametrize("B,T,D", SHAPES)
@pytest.mark.parametrize("live", [None, "mixed", "all0"])
def test_strip_backward_equals_row_tile_kernels(B, T, D, live):
    c = Ctx(B, T, D, seed=B * 11 + T, live=live)
    L, pa, s, M = c.L, c.pa, c.s, c.M
    P = lambda t: pa([t[0].data_ptr(), t[1].data_ptr()])      # noqa: E731
    lo = live is not None
    part_t = lambda: torch.full((2 * c.tpg, 2, D), float("nan"), device="cuda")       # noqa: E731
    part_s = lambda: torch.full((2 * c.stpg, 2, D), float("nan"), device="cuda")      # noqa: E731
    lnw = c.vec(1.0)
    # ---- feed-forward / out-projection backward
    dxo, h, r = c.act(live_only=lo), c.act().relu(), c.act()
    w1T, w2T, woT = c.mat(), c.mat(), c.mat()
    for train in (0, 1):
        ref, got = [c.out() for _ in range(4)], [c.out() for _ in range(4)]
        pr, pg = part_t(), part_s()
        L.call("amid_sas_ffn_bwd_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), P(w1T), P(w2T), P(woT), 1e-8, M, D,
               c.rpt, 1, c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in ref], pr.data_ptr(), 0, s)
        L.call("amid_sas_strip_ffn_bwd_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), P(w1T), P(w2T), P(woT), 1e-8,
               B, T, D, c.lp(), 1, c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in got], pg.data_ptr(), 0, s)
        torch.cuda.synchronize()
        for n, a, b in zip("dpre2 dpre1 dr d_o".split(), got, ref):
            c.check_rows(f"ffn_bwd train={train} {n}", a, b, tol=5e-6)
        c.check_parts(f"ffn_bwd train={train} ln_part", pg, pr)
    # ---- q / k / v + LN1 backward, alone and with the layer below's feed-forward backward behind it
    dq, dk, dv, dr = (c.act(live_only=lo) for _ in range(4))
    x = c.act()
    wq, wk, wv = c.mat(), c.mat(), c.mat()
    ref, got, pr, pg = c.out(), c.out(), part_t(), part_s()
    L.call("amid_sas_qkv_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), P(wq), P(wk), P(wv), 1e-8,
           M, D, c.rpt, ref.data_ptr(), pr.data_ptr(), 0, s)
    L.call("amid_sas_strip_qkv_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), P(wq), P(wk), P(wv),
           1e-8, B, T, D, c.lp(), got.data_ptr(), pg.data_ptr(), *([None] * 7), 0, None, 0, 0.0, *([None] * 5), 0, s)
    torch.cuda.synchronize()
    c.check_rows("qkv_bwd dx", got, ref, tol=5e-6)
    c.check_parts("qkv_bwd ln_part", pg, pr)
    for train in (0, 1):
        ref, got = [c.out() for _ in range(4)], [c.out() for _ in range(4)]
        pr, pg, fpr, fpg, dxr = part_t(), part_s(), part_t(), part_s(), c.out()
        L.call("amid_sas_qkv_ffn_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), P(wq), P(wk), P(wv),
               1e-8, M, D, c.rpt, dxr.data_ptr(), pr.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), P(w1T), P(w2T), P(woT), 0,
               c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in ref], fpr.data_ptr(), 0, s)
        L.call("amid_sas_strip_qkv_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), P(wq), P(wk), P(wv),
               1e-8, B, T, D, c.lp(), None, pg.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), P(w1T), P(w2T), P(woT), 0,
               c.st.data_ptr(), train, 0.5, *[t.data_ptr() for t in got], fpg.data_ptr(), 0, s)
        torch.cuda.synchronize()
        for n, a, b in zip("dpre2 dpre1 dr d_o".split(), got, ref):
            c.check_rows(f"qkv_ffn_bwd train={train} {n}", a, b, tol=1e-5)
        c.check_parts(f"qkv_ffn_bwd train={train} ln1_part", pg, pr)
        c.check_parts(f"qkv_ffn_bwd train={train} ln2_part", fpg, fpr)


@pytest.mark.parametrize("B,T", [(64, 50), (37, 20), (256, 50)])
@pytest.mark.parametrize("live", [None, "mixed"])
def test_strip_backward_bf16_products_within_bf16_rounding_of_fp32(B, T, live):
    """mma_bf16 = 1 (BASELINE.json configs[2]): the data-gradient products of the strip backward kernels on the bf16 matrix cores, from
    amid_sas_weights_bf16 images of the TRANSPOSED weights, against the fp32 strip kernels on the same inputs: every output within 2e-2
    of its tensor's norm, and visibly different (the mode is on)."""
    D = 128
    c = Ctx(B, T, D, seed=B * 5 + T, live=live)
    L, pa, s, M = c.L, c.pa, c.s, c.M
    P = lambda t: pa([t[0].data_ptr(), t[1].data_ptr()])      # noqa: E731
    lo = live is not None
    part_s = lambda: torch.full((2 * c.stpg, 2, D), float("nan"), device="cuda")      # noqa: E731
    lnw = c.vec(1.0)
    dxo, h, r = c.act(live_only=lo), c.act().relu(), c.act()
    dq, dk, dv, dr = (c.act(live_only=lo) for _ in range(4))
    x = c.act()
    mats = [c.mat() for _ in range(6)]                   # w1T, w2T, woT, wqT, wkT, wvT as the fp32 kernels take them: W^T [in][out] per domain
    # the bf16 images of the same matrices: amid_sas_weights_bf16 of the UN-transposed weights with transposed = 1, i.e. of (W^T)^T ... the
    # kernels' operand is the matrix they are handed, so image(W^T) = weights_bf16(src = W^T, transposed = 0)
    img = torch.empty(12, D * D, dtype=torch.bfloat16, device="cuda")
    L.call("amid_sas_weights_bf16", pa([m[g].data_ptr() for m in mats for g in (0, 1)]), 12, D, 0, img.data_ptr(), s)
    I = lambda k: pa([img[2 * k].data_ptr(), img[2 * k + 1].data_ptr()])      # noqa: E731

    def run(bf):
        W = (lambda k: I(k)) if bf else (lambda k: P(mats[k]))
        out = [c.out() for _ in range(4)]
        pg = part_s()
        L.call("amid_sas_strip_ffn_bwd_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), W(0), W(1), W(2), 1e-8,
               B, T, D, c.lp(), 1, c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out], pg.data_ptr(), bf, s)
        dx, pg1 = c.out(), part_s()
        L.call("amid_sas_strip_qkv_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), W(3), W(4), W(5),
               1e-8, B, T, D, c.lp(), dx.data_ptr(), pg1.data_ptr(), *([None] * 7), 0, None, 0, 0.0, *([None] * 5), bf, s)
        out2 = [c.out() for _ in range(4)]
        pg2, fpg2 = part_s(), part_s()
        L.call("amid_sas_strip_qkv_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), W(3), W(4), W(5),
               1e-8, B, T, D, c.lp(), None, pg2.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), W(0), W(1), W(2), 0,
               c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out2], fpg2.data_ptr(), bf, s)
        torch.cuda.synchronize()
        return out + [dx] + out2
    ref, got = run(0), run(1)
    rl = c.row_live.cuda()
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        a, b = a[rl].double(), b[rl].double()
        assert torch.isfinite(a).all(), i
        e = float((a - b).norm() / (b.norm() + 1e-30))
        worst = max(worst, e)
        assert e < 2e-2, (i, e)
    assert worst > 1e-4


@pytest.mark.parametrize("B,T", [(64, 50), (37, 20), (256, 50)])
@pytest.mark.parametrize("live", [None, "mixed"])
def test_strip_backward_on_bf16_pieces_has_fp32_accuracy(B, T, live):
    """mma_bf16 = 3 (the fp32 step's default at D 128): the data-gradient products of the strip backward kernels as six bf16 piece-pair
    products (every fp32 operand = hi + mid + lo exactly; amid_sas_weights_bf16_planes images of the transposed weights) against the fp32
    matrix instructions on the same inputs: every output within 4e-6 of its tensor's largest entry -- the spread of two fp32 summation
    orders, three decades below mma_bf16 = 1 (test above)."""
    D = 128
    c = Ctx(B, T, D, seed=B * 7 + T, live=live)
    L, pa, s = c.L, c.pa, c.s
    P = lambda t: pa([t[0].data_ptr(), t[1].data_ptr()])      # noqa: E731
    lo = live is not None
    part_s = lambda: torch.full((2 * c.stpg, 2, D), float("nan"), device="cuda")      # noqa: E731
    lnw = c.vec(1.0)
    dxo, h, r = c.act(live_only=lo), c.act().relu(), c.act()
    dq, dk, dv, dr = (c.act(live_only=lo) for _ in range(4))
    x = c.act()
    mats = [c.mat() for _ in range(6)]                   # w1T, w2T, woT, wqT, wkT, wvT: W^T [in][out] per domain
    img = torch.empty(12, 3, D * D, dtype=torch.bfloat16, device="cuda")
    L.call("amid_sas_weights_bf16_planes", pa([m[g].data_ptr() for m in mats for g in (0, 1)]), 12, D, 0, 3, img.data_ptr(), s)
    I = lambda k: pa([img[2 * k].data_ptr(), img[2 * k + 1].data_ptr()])      # noqa: E731

    def run(bf):
        W = (lambda k: I(k)) if bf else (lambda k: P(mats[k]))
        out = [c.out() for _ in range(4)]
        pg = part_s()
        L.call("amid_sas_strip_ffn_bwd_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), W(0), W(1), W(2), 1e-8,
               B, T, D, c.lp(), 1, c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out], pg.data_ptr(), bf, s)
        dx, pg1 = c.out(), part_s()
        L.call("amid_sas_strip_qkv_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), W(3), W(4), W(5),
               1e-8, B, T, D, c.lp(), dx.data_ptr(), pg1.data_ptr(), *([None] * 7), 0, None, 0, 0.0, *([None] * 5), bf, s)
        out2 = [c.out() for _ in range(4)]
        pg2, fpg2 = part_s(), part_s()
        L.call("amid_sas_strip_qkv_bwd_f32", dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), W(3), W(4), W(5),
               1e-8, B, T, D, c.lp(), None, pg2.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), W(0), W(1), W(2), 0,
               c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out2], fpg2.data_ptr(), bf, s)
        torch.cuda.synchronize()
        return out + [dx] + out2 + [pg, pg1, pg2, fpg2]
    ref, got = run(0), run(3)
    rl = c.row_live.cuda()
    if (B, T) == (256, 50):        # a race screen for the hand-placed LDS reads and the four-slot plane ring: the same bits every time
        for rep in range(20):
            again = run(3)
            for i, (a, b) in enumerate(zip(again, got)):
                a, b = (a[rl], b[rl]) if i < 9 else (a, b)
                assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), (rep, i)
    for i, (a, b) in enumerate(zip(got, ref)):
        if i < 9:
            a, b = a[rl].double(), b[rl].double()
        else:                                            # LayerNorm partial sums: the slots of live strips only (the others stay NaN in both)
            ok = torch.isfinite(b)
            assert bool((torch.isfinite(a) == ok).all()), i
            a, b = a[ok].double(), b[ok].double()
        assert torch.isfinite(a).all(), i
        e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
        assert e < 4e-6, (i, e)


@pytest.mark.parametrize("B,T", [(64, 50), (37, 20), (256, 50), (300, 33)])
@pytest.mark.parametrize("live", [None, "mixed"])
@pytest.mark.parametrize("with_stat", [False, True])
def test_strip_backward_n_split_build_on_pieces_matches_the_strip_build(B, T, live, with_stat):
    """csrc/sasrec_strip_px.hip (round 6): the feed-forward / out-projection backward chain with two waves per strip -- each owning half the
    output columns of every product, operands crossing as bf16 pieces -- against the strip build on the same three-plane weight images:
    every output within 4e-6 of its tensor's largest entry (the LayerNorm backward's row sums are added part by part), with the row
    statistics recomputed from r or taken from the forward's ln_stat array; the same bits on every repetition."""
    D = 128
    c = Ctx(B, T, D, seed=B * 11 + T, live=live)
    L, pa, s = c.L, c.pa, c.s
    P = lambda t: pa([t[0].data_ptr(), t[1].data_ptr()])      # noqa: E731
    lo = live is not None
    part_s = lambda: torch.full((2 * c.stpg, 2, D), float("nan"), device="cuda")      # noqa: E731
    lnw = c.vec(1.0)
    dxo, h, r = c.act(live_only=lo), c.act().relu(), c.act()
    mats = [c.mat() for _ in range(3)]                   # w1T, w2T, woT
    img = torch.empty(6, 3, D * D, dtype=torch.bfloat16, device="cuda")
    L.call("amid_sas_weights_bf16_planes", pa([m[g].data_ptr() for m in mats for g in (0, 1)]), 6, D, 0, 3, img.data_ptr(), s)
    I = lambda k: pa([img[2 * k].data_ptr(), img[2 * k + 1].data_ptr()])      # noqa: E731
    stat = torch.zeros(r.shape[0], 4, device="cuda")
    mean = r.mean(1)
    stat[:, 2] = mean
    stat[:, 3] = 1.0 / torch.sqrt(((r - mean[:, None]) ** 2).mean(1) + 1e-8)

    def run(px):
        out = [c.out() for _ in range(4)]
        pg = part_s()
        if px:
            L.call("amid_sas_strip_ffn_bwd_px_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), I(0), I(1), I(2), 1e-8,
                   B, T, D, c.lp(), 1, c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out], pg.data_ptr(), stat.data_ptr() if with_stat else None,
                   None, 0, s)
        else:
            L.call("amid_sas_strip_ffn_bwd_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), I(0), I(1), I(2), 1e-8,
                   B, T, D, c.lp(), 1, c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out], pg.data_ptr(), 3, s)
        torch.cuda.synchronize()
        return out + [pg]
    ref, got = run(False), run(True)
    rl = c.row_live.cuda()
    for rep in range(10 if (B, T) == (256, 50) else 2):
        again = run(True)
        for i, (a, b) in enumerate(zip(again, got)):
            a, b = (a[rl], b[rl]) if i < 4 else (a, b)
            assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), (rep, i)
    for i, (a, b) in enumerate(zip(got, ref)):
        if i < 4:
            a, b = a[rl].double(), b[rl].double()
        else:
            ok = torch.isfinite(b)
            assert bool((torch.isfinite(a) == ok).all()), i
            a, b = a[ok].double(), b[ok].double()
        assert torch.isfinite(a).all(), i
        e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
        assert e < 4e-6, (i, e)
    if (B, T, with_stat) == (256, 50, True) and live:
        def timeit(fn, n=50):
            for _ in range(5): fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n): fn()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n
        out = [c.out() for _ in range(4)]
        pg = part_s()
        t_strip = timeit(lambda: L.call("amid_sas_strip_ffn_bwd_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), I(0), I(1), I(2), 1e-8,
                                        B, T, D, c.lp(), 1, c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out], pg.data_ptr(), 3, s))
        t_px = timeit(lambda: L.call("amid_sas_strip_ffn_bwd_px_f32", dxo.data_ptr(), c.tmq.data_ptr(), h.data_ptr(), r.data_ptr(), P(lnw), I(0), I(1), I(2), 1e-8,
                                     B, T, D, c.lp(), 1, c.st.data_ptr(), 1, 0.5, *[t.data_ptr() for t in out], pg.data_ptr(), stat.data_ptr(), None, 0, s))
        print(f"PXTIME strip_ffn_bwd: strip build {t_strip:.1f} us, n-split on pieces {t_px:.1f} us (launch-to-launch, eager)")


@pytest.mark.parametrize("T", [12, 20, 40])          # one, two and three waves of a strip tile's sequences; B T = 36, 60, 120: no multiple of the tile
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("train", [1, 0])            # embedding dropout 0.5 / off
def test_embedding_backward_on_the_strip_without_a_rider_equals_its_two_launches(T, D, train):
    """amid_sas_strip_qkv_bwd_emb_f32 with sort_plan == NULL (the form no step of the engine takes: its launches always carry the sort) is
    amid_sas_strip_qkv_bwd_f32 without the fused feed-forward followed by amid_embed_bwd_f32's element-wise part on the stored rows: the
    same call record with the embedding block named and no rider.  dx of the live sequences and the LayerNorm partial sums BIT FOR BIT;
    the rows outside the live list stay untouched.  Both domains are on the list."""
    B = 3
    c = Ctx(B, T, D, seed=40 + T + D, live="mixed")
    c.dom = torch.tensor([0, 1, 0])
    c.live = torch.tensor([0, 2, 1, 2], dtype=torch.int32).cuda()      # domain 0: sequences 0 and 2; domain 1: sequence 1; n0 = 2
    c.row_live = torch.cat((c.dom == 0, c.dom != 0)).repeat_interleave(T)
    L, pa, s = c.L, c.pa, c.s
    P = lambda t: pa([t[0].data_ptr(), t[1].data_ptr()])      # noqa: E731
    dq, dk, dv, dr = (c.act(live_only=True) for _ in range(4))
    x, lnw, wq, wk, wv = c.act(), c.vec(1.0), c.mat(), c.mat(), c.mat()
    part = lambda: torch.full((2 * c.stpg, 2, D), float("nan"), device="cuda")      # noqa: E731
    two, one, p2, p1 = c.out(), c.out(), part(), part()
    head = (dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), x.data_ptr(), P(lnw), P(wq), P(wk), P(wv), 1e-8, B, T, D, c.lp())
    L.call("amid_sas_strip_qkv_bwd_f32", *head, two.data_ptr(), p2.data_ptr(), *([None] * 7), 0, None, 0, 0.0, *([None] * 5), 0, s)
    dpos = torch.zeros(1, 2, T, D, device="cuda")
    L.call("amid_embed_bwd_f32", two.data_ptr(), c.tmq.data_ptr(), B, T, D, 1, dpos.data_ptr(), c.st.data_ptr(), train, 0.5, s)
    L.call("amid_sas_strip_qkv_bwd_emb_f32", *head, one.data_ptr(), p1.data_ptr(), c.tmq.data_ptr(), c.st.data_ptr(), train, 0.5, None, 0, 0, s)
    torch.cuda.synchronize()
    rl = c.row_live
    assert torch.isfinite(one.cpu()[rl]).all() and bool((one.cpu()[rl] == 0).any()) and bool((one.cpu()[rl] != 0).any())
    assert torch.equal(one.cpu()[rl], two.cpu()[rl])
    assert torch.isnan(one.cpu()[~rl]).all(), "rows outside the live list were written"
    assert torch.equal(torch.nan_to_num(p1.cpu()), torch.nan_to_num(p2.cpu())) and torch.equal(torch.isnan(p1.cpu()), torch.isnan(p2.cpu()))
