"""tests/head_ref.py (the float64 reference of tests/test_gpu_head.py) against torch.autograd through an independent formulation
(nn.LayerNorm, nn.Linear, F.binary_cross_entropy, the two doubly-robust losses as one-line expressions), its float32 form against torch's
own float32 binary_cross_entropy where both clamps act, and the inputs of the GPU cases against the conditions they are built to meet.
None of it needs a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import head_ref as R

F64 = torch.float64
SHAPES = [(3, 5, 2, 16, 8), (2, 7, 65, 32, 16), (2, 4, 3, 8, 64)]      # (B, T, NI, D, hid)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def inputs(B, T, NI, D, hid):
    g = torch.Generator().manual_seed(7 * B + 11 * T + 13 * NI + D + hid)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    x = rn(2, B, T, D) * (0.5 + torch.rand(2, B, T, 1, generator=g, dtype=F64)) + 0.3 * rn(2, B, T, 1)
    ln = (0.5 + torch.rand(2, D, generator=g, dtype=F64), 0.2 * rn(2, D))
    W = dict(w1=rn(hid, 2 * D) / (2 * D) ** 0.5, b1=0.1 * rn(hid), w2=rn(hid) / hid ** 0.5, b2=0.1 * rn(1))
    labels = (torch.rand(B, NI, generator=g) < 0.5).to(F64)
    domain_id = torch.arange(B) % 2
    return x, ln, 0.7 * rn(B, NI, D), W, labels, domain_id


@pytest.mark.parametrize("B,T,NI,D,hid", SHAPES)
def test_head_restatement_against_autograd(B, T, NI, D, hid):
    x, ln, items, W, labels, domain_id = inputs(B, T, NI, D, hid)
    # the restatement, every backward written out
    u = R.lnmean(x, ln, F64)
    p, _ = R.scorer(u, items, W, F64)
    mb = R.masked_bce(p, labels, domain_id, F64)
    bw = R.scorer_bwd(u, items, W, p, mb["dp"], F64)
    lb = R.lnmean_bwd(x, bw["du"], ln, F64)
    # autograd through torch's own modules
    norms = [torch.nn.LayerNorm(D, eps=R.EPS).double() for _ in (0, 1)]
    lin1, lin2 = torch.nn.Linear(2 * D, hid).double(), torch.nn.Linear(hid, 1).double()
    with torch.no_grad():
        for g in (0, 1):
            norms[g].weight.copy_(ln[0][g]); norms[g].bias.copy_(ln[1][g])
        lin1.weight.copy_(W["w1"]); lin1.bias.copy_(W["b1"]); lin2.weight.copy_(W["w2"][None]); lin2.bias.copy_(W["b2"])
    xa, ia = x.clone().requires_grad_(True), items.clone().requires_grad_(True)
    ua = torch.stack([norms[g](xa[g]).mean(1) for g in (0, 1)])
    ua.retain_grad()
    cat = torch.cat((ua[:, :, None, :].expand(2, B, NI, D), ia[None].expand(2, B, NI, D)), dim=-1)
    pa = torch.sigmoid(lin2(torch.relu(lin1(cat)))).squeeze(-1)
    pa.retain_grad()
    own = torch.stack((domain_id == 0, domain_id == 1)).double()
    per = F.binary_cross_entropy(pa, labels[None].expand(2, B, NI), reduction="none") * own[:, :, None]
    loss = per.sum(0).mean()
    loss.backward()
    got = dict(u=(u, ua.detach()), p=(p, pa.detach()), loss=(mb["loss_part"].sum(), loss.detach()), dp=(mb["dp"], pa.grad), du=(bw["du"], ua.grad),
               ditems=(bw["ditems"], ia.grad), dx=(lb["dx"], xa.grad))
    rows = R.sc_part_rows(u, items, bw).sum(0)
    o = hid * 2 * D
    got["dW1"] = (rows[:o].view(hid, 2 * D), lin1.weight.grad)
    got["db1"] = (rows[o:o + hid], lin1.bias.grad)
    got["dW2"] = (rows[o + hid:o + 2 * hid], lin2.weight.grad[0])
    got["db2"] = (rows[o + 2 * hid:], lin2.bias.grad)
    part = lb["ln_part"].view(2, B, 2, D).sum(1)
    for g in (0, 1):
        got[f"dgamma{g}"] = (part[g, 0], norms[g].weight.grad)
        got[f"dbeta{g}"] = (part[g, 1], norms[g].bias.grad)
    bad = {k: rel(a, b) for k, (a, b) in got.items() if not rel(a, b) <= 1e-11}
    assert not bad, bad
    # the hidden-gradient row holds the same pieces: da | dc | dW2 | db2
    hg = R.hidg_rows(bw)
    assert hg.shape == (B, (3 + NI) * hid + 1) and R.vec_floats(NI, hid) - hg.shape[1] in (0, 1, 2, 3)
    assert torch.equal(hg[:, :2 * hid], bw["da"].reshape(B, -1)) and torch.equal(hg[:, 2 * hid:(2 + NI) * hid], bw["dc"].reshape(B, -1))
    assert torch.equal(hg[:, (2 + NI) * hid:-1], bw["dw2"]) and torch.equal(hg[:, -1], bw["db2"])
    assert R.part_floats(D, hid) - rows.numel() in (0, 1, 2, 3)
    # the plain mean (no LayerNorm)
    xa2 = x.clone().requires_grad_(True)
    ua2 = xa2.mean(2)
    (ua2 * bw["du"]).sum().backward()
    assert rel(R.lnmean(x, None, F64), ua2.detach()) <= 1e-11 and rel(R.lnmean_bwd(x, bw["du"], None, F64)["dx"], xa2.grad) <= 1e-11
    assert rel(R.layernorm_rows(x[0, 0], ln[0][0], ln[1][0], F64), norms[0](x[0, 0]).detach()) <= 1e-11


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,T,NI,D,hid", SHAPES)
def test_dr_restatement_against_autograd(B, T, NI, D, hid, mode):
    g = torch.Generator().manual_seed(100 * B + NI + mode)
    leaf = lambda: (0.05 + 0.9 * torch.rand(2, B, NI, generator=g, dtype=F64)).requires_grad_(True)      # noqa: E731
    p, ips, gf = leaf(), leaf(), leaf()
    labels = (torch.rand(B, NI, generator=g) < 0.5).to(F64)
    domain_id, ob = torch.arange(B) % 2, (torch.arange(B) % 3 != 1).long()
    w = 0.5
    ref = R.dr_loss(p.detach(), ips.detach(), gf.detach(), labels, domain_id, ob, mode, w, F64)
    pick = lambda t: torch.where(domain_id[:, None] != 0, t[1], t[0])      # noqa: E731
    c = F.binary_cross_entropy(pick(p), labels, reduction="none")
    cls, dre, drr = c.mean(), ((c - pick(gf)) ** 2 / pick(ips)).mean(), (pick(gf) ** 2 + ob[:, None] * (c ** 2 - pick(gf) ** 2) ** 2 / pick(ips)).mean()
    (cls + w * dre if mode == 0 else drr).backward()
    got = dict(cls=(ref["loss_part"][:, 0].sum(), cls.detach()), dre=(ref["loss_part"][:, 1].sum(), dre.detach()),
               drr=(ref["loss_part"][:, 2].sum(), drr.detach()), dg=(ref["dg"], gf.grad))
    if mode == 0 or bool(ob.any()):
        got["dp"], got["dips"] = (ref["dp"], p.grad), (ref["dips"], ips.grad)
    bad = {k: rel(a, b) for k, (a, b) in got.items() if not rel(a, b) <= 1e-11}
    assert not bad, bad
    other = torch.stack((domain_id != 0, domain_id == 0))[:, :, None].expand(2, B, NI)
    assert all(bool((ref[k][other] == 0).all()) for k in ("dp", "dips", "dg"))


def test_float32_restatement_at_a_saturated_logit_is_torchs_bce_bit_for_bit():
    """b2 = +40: p == 1.0f exactly, so log(1 - p) = -inf is clamped at -100 and p (1 - p) = 0 at 1e-12 -- both clamps of the restatement,
    against torch's float32 binary_cross_entropy and its backward."""
    B, T, NI, D, hid = 3, 5, 4, 16, 8
    x, ln, items, W, labels, domain_id = inputs(B, T, NI, D, hid)
    W = dict(W, b2=torch.tensor([40.0], dtype=F64))
    f32 = torch.float32
    p, _ = R.scorer(R.lnmean(x, ln, f32), items, W, f32)
    assert p.dtype == f32 and bool((p == 1.0).all())
    assert bool((labels == 0).any()) and bool((labels == 1).any())
    mb = R.masked_bce(p, labels, domain_id, f32)
    pt = p.clone().requires_grad_(True)
    val = F.binary_cross_entropy(pt, labels.float()[None].expand(2, B, NI), reduction="none")
    m, inv = R.own_mask(domain_id, f32)[:, :, None], torch.tensor(1.0 / (B * NI), dtype=f32)
    (val * m * inv).sum().backward()
    assert torch.equal(mb["bce"], val.detach()) and float(val.detach().max()) == 100.0
    assert torch.equal(mb["loss_part"], (val.detach() * m * inv).sum((0, 2)))
    assert torch.equal(mb["dp"], pt.grad) and bool(torch.isfinite(mb["dp"]).all()) and float(mb["dp"].abs().max()) > 1e9
    # the doubly-robust form reads the same two clamps
    c, dc = R.bce(p, labels.float()[None].expand(2, B, NI))
    assert torch.equal(c, val.detach()) and float(dc.abs().max()) == float(torch.tensor(1e12, dtype=f32))


def test_gpu_case_inputs_meet_their_conditions():
    """Every case builder of tests/test_gpu_head.py, at every listed shape: the ReLU margin |z| > 2 (2D + 2) 2^-24 sum_k |w_k v_k| on every hidden
    pre-activation, every p / ips / g in (0.02, 0.98), both domains (and both ob_label values) present, within the cap of 8 seed steps."""
    from tests import test_gpu_head as G
    steps = []
    for shape, ln, dom, _ in G.HEAD_CASES:
        c = G.head_case(*shape, ln=ln, dom=dom)
        u = R.lnmean(c["x"], c["ln"], F64)
        assert G.relu_margin_ok(u, c["items"], c["W"]) and G.in_range(c["ref64"]["p"]), shape
        assert set(c["labels"].unique().tolist()) <= {0.0, 1.0}
        assert shape[0] == 1 or dom != "mixed" or set(c["domain_id"].tolist()) == {0, 1}
        steps.append(c["steps"])
    assert {dom for _, _, dom, _ in G.HEAD_CASES} == {"mixed", 0, 1}
    forms = [(B, NI, D, hid, 1, 0) for B, NI, D, hid in G.SCORER_SHAPES + [(2, 3, 20, 5)]]
    forms += [(3, NI, D, hid, nh, mode) for nh, mode, NI in G.MULTI_FORMS for D, hid in ((128, 32), (64, 64))]
    for B, NI, D, hid, nh, mode in forms:
        c = G.scorer_case(B, NI, D, hid, nh, mode)
        for W in c["Ws"]:
            assert G.relu_margin_ok(c["u"], c["items"], W) and G.in_range(R.scorer(c["u"], c["items"], W, F64)[0]), (B, NI, D, hid, nh)
        assert B == 1 or (set(c["domain_id"].tolist()) == {0, 1} and set(c["ob"].tolist()) == {0, 1})
        steps.append(c["steps"])
    assert max(steps) <= G.MAX_SEED_STEPS, steps
    for B, NI in [(1, 1), (4, 16), (3, 64), (3, 65), (2, 130)]:
        for mode in (0, 1):
            c = G.dr_case(B, NI, mode)
            assert G.in_range(c["p"], c["ips"], c["g"])
    print("seed steps per case:", steps)


def test_one_ulp_in_the_objectives_inputs_is_over_the_bar_of_4():
    """Why tests/test_gpu_head.py holds a few doubly-robust tensors to more than 4 e_f32 + 2^-22 (FACTOR there, profiles/head_kernels.md): in
    the float32 restatement itself, one ulp in c = BCE(p, y) (another logf) or in the heads' p (another expf) moves those tensors past that bar --
    dips of the 2x130 mode 1 case to the 4.84e-07 measured on the GPU, where the unmoved restatement is at 3.88e-08."""
    from tests import test_gpu_head as G
    err, f32 = G.err, torch.float32
    c = G.dr_case(2, 130, 1)
    unmoved = err(c["ref32"]["dips"], c["ref64"]["dips"])
    moved = [err(R.dr_loss(c["p"], c["ips"], c["g"], c["labels"], c["domain_id"], c["ob"], 1, G.DR_W, f32, c_ulps=n)["dips"], c["ref64"]["dips"]) for n in (1, -1)]
    print(f"dr_loss 2x130 mode 1 dips: unmoved {unmoved:.3e}, c moved by +1 / -1 ulp {moved[0]:.3e} / {moved[1]:.3e}, bar of 4 {4 * unmoved + G.FLOOR:.3e}")
    assert min(moved) > 4 * unmoved + G.FLOOR and 4.0e-07 < max(moved) < 6.0e-07
    # the three-head entry: dLoss/dp from the three heads' own float32 p, each moved by one ulp (all sign patterns over the heads)
    for NI, D, hid, mode in ((1, 128, 32, 0),):
        c = G.scorer_case(3, NI, D, hid, 3, mode)
        ps = [R.scorer(c["u"], c["items"], W, f32)[0] for W in c["Ws"]]
        unmoved = err(c["ref32"]["dp"], c["ref64"]["dp"])
        worst = max(err(R.dr_loss(*[R.move_ulps(p, 1 if (pat >> h) & 1 else -1) for h, p in enumerate(ps)], c["labels"], c["domain_id"], c["ob"], mode,
                                  G.DR_W, f32)["dp"], c["ref64"]["dp"]) for pat in range(8))
        print(f"three heads NI {NI} D {D} mode {mode} dp: unmoved {unmoved:.3e}, every p moved by one ulp {worst:.3e}, bar of 4 {4 * unmoved + G.FLOOR:.3e}")
        assert worst > 4 * unmoved + G.FLOOR
