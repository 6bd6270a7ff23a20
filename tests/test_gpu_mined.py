"""amid_scorer_mined_fwd_bwd_f32 (csrc/head_mined.hip; DESIGN.md section 18: scorer forward over a row's NI candidates, the H negatives ranked
S .. S + H - 1 by own-domain logit kept, the listwise objective and the scorer backward over the compact list only -- one launch) through the
C ABI against the float64 restatement tests/mined_ref.py, which tests/test_mined_ref.py holds to torch.autograd.

Exact: sel is the rule evaluated on the host on the kernel's OWN z output (float32 compares are exact), ascending without repeats; dz of the
own domain is exactly 0 off column 0 and sel, ditems exactly 0 on the rows not kept; the other domain's dz rows and du half are 0; p1 / p2
are amid_scorer_fwd_f32's bits; the transposes are exact; every output lies between untouched guards.

Accuracy, as tests/test_gpu_listwise.py: e = max|x - ref64| / max|ref64|, e_kernel <= 4 e_f32 + 2^-22, sc_db2 against the largest row sum of
|dz|.  z is held to the float64 logits; every other tensor to the float64 restatement evaluated on the KERNEL's selection (two logits closer
than a float32 rounding may be ordered either way), e_f32 being the float32 restatement on that same selection.  That the kernel's selection
is a sound one where float64 would have chosen differently is checked on the float64 logits: with m = 2 * (4 e_f32 + 2^-22) max|z64| -- twice
the absolute error the z bar allows, so it follows from the exact selection and the z bar -- every kept logit is >= every logit ranked behind
the window minus m and <= every skipped one plus m.  The number of rows whose selection differs from float64's is logged.

Shapes (B, NI, D, hid, H, S): SHAPES below with the reason beside each.  Identity pin: at H = M, S = 0 the list is 0 .. NI - 1 and p,
loss_part and dz are amid_scorer_listwise_fwd_bwd_f32's bits (z has no counterpart there: it is pinned through p, the same expression of z,
and the bar).  Ties: w2 = 0 makes every logit b2, sel is S + 1 .. S + H and the softmax loss log(1 + H); an item row repeated at three
positions gives three equal logits, of which the lower positions win.  Saturation (b2 = +40): finite and the float32 restatement's values at
test_gpu_listwise.py's SAT_BAR.

A test of this file after which the device reports an error ends the whole pytest session (stop_at_a_gpu_fault)."""
import math

import pytest
import torch

from tests import head_ref as R
from tests import listwise_ref as LW
from tests import mined_ref as MR
from tests.test_gpu_head import take_rows
from tests.test_gpu_intercomp import FLOOR, GUARD, UNSUPPORTED, L, Out, err, pa, stream  # noqa: F401  (L: the library fixture)
from tests.test_gpu_listwise import SAT_BAR, stop_at_a_gpu_fault  # noqa: F401  (the autouse fixture that ends the session at a fault)
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
ENTRY = "amid_scorer_mined_fwd_bwd_f32"
ARG = -1
SHAPES = [(1, 3, 32, 4, 1, 0),             # the smallest; idle lanes everywhere
          (3, 2, 128, 32, 1, 0),           # H = M = 1
          (2, 65, 128, 32, 8, 0),          # the forward two chunks, the list one
          (2, 130, 64, 16, 63, 1),         # a list of exactly 64 entries
          (2, 130, 64, 16, 64, 1),         # 65 entries: the list-chunk edge
          (2, 600, 96, 24, 520, 0),        # a list over 512: two entries a thread in the objective
          (1, 1024, 128, 64, 16, 3),       # the limit shape
          (1, 1024, 128, 64, 1020, 3)]     # the limit shape with S + H = M exactly
FACTOR = {}                      # (kind, tensor) -> a factor other than 4, with its figures in profiles/hard_negatives.md: none measured over the bar
ISENT = -7777


class IntOut:
    """Out for int32: -1 where the kernel must write, ISENT in the guards."""

    def __init__(self, *shape):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + n + GUARD,), ISENT, dtype=torch.int32, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(-1)

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self, tag):
        b = self.buf.cpu()
        n = self.t.numel()
        assert bool((b[:GUARD] == ISENT).all()) and bool((b[GUARD + n:] == ISENT).all()), f"{tag}: a write outside the output"
        assert bool((b[GUARD:GUARD + n] >= 0).all()), f"{tag}: an element was not written"
        return b[GUARD:GUARD + n].view(self.t.shape).clone()


def outputs(B, NI, D, hid, H=None):
    o = dict(p1=Out(B, NI), p2=Out(B, NI), dz1=Out(B, NI), dz2=Out(B, NI), loss_part=Out(B), du=Out(2, B, D), ditems=Out(B, NI, D),
             sc_part=Out(B, R.part_floats(D, hid)))
    if H is not None:
        o.update(sel=IntOut(B, H), z=Out(B, NI))
    return o


def split_rows(o, D, hid):
    rows = take_rows(o["sc_part"], hid * 2 * D + 2 * hid + 1, "sc_part")
    w = hid * 2 * D
    return dict(sc_dW1=rows[:, :w], sc_db1=rows[:, w:w + hid], sc_dW2=rows[:, w + hid:w + 2 * hid], sc_db2=rows[:, w + 2 * hid:])


def launch(L, c, kind, H, S, n_tr, change=()):
    """The launch on a case's inputs: its outputs by name after the exact checks."""
    B, NI, D = c["items"].shape
    hid = c["W"]["b1"].numel()
    d = {k: c[k].cuda() for k in ("u", "items", "domain_id")}
    W = {k: v.cuda() for k, v in c["W"].items()}
    o = outputs(B, NI, D, hid, H)
    g = torch.Generator().manual_seed(n_tr)
    tr_src, tr_dst = [torch.randn(D, D, generator=g).cuda() for _ in range(n_tr)], [Out(D, D) for _ in range(n_tr)]
    tab = dict({k: v.data_ptr() for k, v in d.items()}, **{k: v.data_ptr() for k, v in W.items()}, kind=kind, keep=H, skip=S, B=B, NI=NI, D=D,
               hid=hid, **{k: v.data_ptr() for k, v in o.items()}, tr_src=pa(tr_src) if n_tr else None, tr_dst=pa(tr_dst) if n_tr else None,
               n_tr=n_tr, stream=stream())
    tab.update(change)                               # (the refusals' bad arguments)
    L.call_named(ENTRY, tab)
    torch.cuda.synchronize()
    # the plain scorer forward on the same inputs: the same bits
    q = dict(p1=Out(B, NI), p2=Out(B, NI))
    L.call_named("amid_scorer_fwd_f32", {k: tab[k] for k in ("u", "items", "w1", "b1", "w2", "b2", "B", "NI", "D", "hid", "stream")}, labels=None,
                 domain_id=None, dp1=None, dp2=None, loss_part=None, **{k: v.data_ptr() for k, v in q.items()})
    torch.cuda.synchronize()
    p = torch.stack((o["p1"].get("p1"), o["p2"].get("p2")))
    assert torch.equal(p, torch.stack((q["p1"].get("p1"), q["p2"].get("p2")))), "p against amid_scorer_fwd_f32"
    dz = torch.stack((o["dz1"].get("dz1"), o["dz2"].get("dz2")))
    du, ditems, z, sel = o["du"].get("du"), o["ditems"].get("ditems"), o["z"].get("z"), o["sel"].get("sel").long()
    own, ar = (c["domain_id"] != 0).long(), torch.arange(B)
    assert torch.equal(dz[1 - own, ar], torch.zeros(B, NI)), "dz of the other domain"
    assert torch.equal(du[1 - own, ar], torch.zeros(B, D)), "du of the other domain"
    # the selection: the rule on the kernel's own logits
    assert bool((sel >= 1).all()) and bool((sel <= NI - 1).all()), "sel outside 1 .. M"
    assert bool((sel[:, 1:] > sel[:, :-1]).all()), "sel not ascending / repeats"
    assert torch.equal(sel, MR.select(z, H, S)), "sel against the rule on the kernel's z"
    keep = MR.kept_mask(sel, NI)
    n_off = int((~keep).sum())
    assert torch.equal(dz[own, ar][~keep], torch.zeros(n_off)), "dz off the list"
    assert torch.equal(ditems[~keep], torch.zeros(n_off, D)), "ditems off the list"
    for i, (src, dst) in enumerate(zip(tr_src, tr_dst)):
        assert torch.equal(dst.get(f"tr_dst[{i}]"), src.cpu().t()), f"transpose {i}"
    return dict(z=z, p=p, sel=sel, dz=dz, du=du, ditems=ditems, loss_part=o["loss_part"].get("loss_part"), **split_rows(o, D, hid))


def errors(got, ref, k, dz64):
    """e of tensor k; sc_db2 (0 in exact arithmetic) against the largest row sum of |dz| (test_gpu_listwise.py's docstring)."""
    if k == "sc_db2":
        return float((got[k].double() - ref[k].double()).abs().max() / dz64.abs().sum((0, 2)).max())
    return err(got[k], ref[k].double())


def refs_on(c, kind, H, S, sel):
    """(float64, float32) restatements on the selection `sel`; z the own domain's rows (the launch's z output)."""
    out = []
    for t in (LW.F64, LW.F32):
        r = MR.launch(c["u"], c["items"], c["W"], c["domain_id"], kind, H, S, t, sel=sel)
        out.append(dict(r, z=MR.own_rows(r["z"], c["domain_id"])))
    return out


def check(kind, tag, got, ref64, ref32, factor=FACTOR):
    bad = []
    for k in got:
        if k == "sel":
            continue
        ek, ef = errors(got, ref64, k, ref64["dz"]), errors(ref32, ref64, k, ref64["dz"])
        f = factor.get((kind, k), 4)
        log(f"mined kind {kind} [{tag}] {k} e_kernel {ek:.3e} e_f32 {ef:.3e}")
        print(f"mined kind {kind} [{tag}] {k} e_kernel {ek:.3e} e_f32 {ef:.3e} bar {f * ef + FLOOR:.3e}")
        if not ek <= f * ef + FLOOR:
            bad.append((k, ek, ef))
    assert not bad, (kind, tag, bad)


def selection_is_sound(tag, got, ref64, ref32, H, S):
    """The kernel's selection on the float64 logits, within m = twice the absolute error the z bar allows (the module docstring)."""
    z64, sel = ref64["z"], got["sel"]
    B, NI = z64.shape
    m = 2 * (4 * err(ref32["z"], z64) + FLOOR) * float(z64.abs().max())
    rk = MR.ranks(got["z"])                                       # the kernel's ranks of the positions 1 .. M
    differ = int((sel != MR.select(z64, H, S)).any(1).sum())
    log(f"mined [{tag}] rows whose selection differs from float64's: {differ} of {B}, m {m:.3e}")
    print(f"mined [{tag}] rows whose selection differs from float64's: {differ} of {B}, m {m:.3e}")
    for b in range(B):
        neg = z64[b, 1:]
        kept, behind, skipped = neg[(rk[b] >= S) & (rk[b] < S + H)], neg[rk[b] >= S + H], neg[rk[b] < S]
        if behind.numel():
            assert float(kept.min()) >= float(behind.max()) - m, (tag, b, "a kept logit below one behind the window")
        if skipped.numel():
            assert float(kept.max()) <= float(skipped.min()) + m, (tag, b, "a kept logit above a skipped one")


@pytest.mark.parametrize("n_tr", [0, 3])
@pytest.mark.parametrize("dom", ["mixed", 0, 1])
@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
@pytest.mark.parametrize("B,NI,D,hid,H,S", SHAPES)
def test_mined_against_fp64(L, B, NI, D, hid, H, S, kind, dom, n_tr):
    c = LW.case(B, NI, D, hid, dom)
    got = launch(L, c, kind, H, S, n_tr)
    ref64, ref32 = refs_on(c, kind, H, S, got["sel"])
    tag = f"{B}x{NI} D {D} hid {hid} H {H} S {S} dom {dom} n_tr {n_tr}"
    check(kind, tag, got, ref64, ref32)
    selection_is_sound(tag, got, ref64, ref32, H, S)


@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
@pytest.mark.parametrize("B,NI,D,hid", [(1, 3, 32, 4), (3, 2, 128, 32), (2, 65, 128, 32), (2, 130, 64, 16), (2, 600, 96, 24), (1, 1024, 128, 64)])
def test_all_kept_is_the_listwise_launch(L, B, NI, D, hid, kind):
    """H = M, S = 0: p, loss_part and dz bit-equal to amid_scorer_listwise_fwd_bwd_f32 on the same inputs; the backward held to float64."""
    c = LW.case(B, NI, D, hid, "mixed")
    got = launch(L, c, kind, NI - 1, 0, 0)
    assert torch.equal(got["sel"], torch.arange(1, NI).expand(B, NI - 1))
    d = {k: c[k].cuda() for k in ("u", "items", "domain_id")}
    W = {k: v.cuda() for k, v in c["W"].items()}
    o = outputs(B, NI, D, hid)
    L.call_named("amid_scorer_listwise_fwd_bwd_f32", {k: v.data_ptr() for k, v in d.items()}, {k: v.data_ptr() for k, v in W.items()},
                 {k: v.data_ptr() for k, v in o.items()}, kind=kind, B=B, NI=NI, D=D, hid=hid, tr_src=None, tr_dst=None, n_tr=0, stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(got["p"], torch.stack((o["p1"].get("p1"), o["p2"].get("p2")))), "p"
    assert torch.equal(got["loss_part"], o["loss_part"].get("loss_part")), "loss_part"
    assert torch.equal(got["dz"], torch.stack((o["dz1"].get("dz1"), o["dz2"].get("dz2")))), "dz"
    ref64, ref32 = LW.refs(B, NI, D, hid, "mixed", kind)
    own = lambda r: dict(r, z=MR.own_rows(r["z"], c["domain_id"]))      # noqa: E731
    check(kind, f"{B}x{NI} D {D} hid {hid} all kept", got, own(ref64), own(ref32))


@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
@pytest.mark.parametrize("B,NI,D,hid,H,S", [(2, 65, 128, 32, 8, 0), (2, 65, 128, 32, 8, 5), (2, 130, 64, 16, 64, 1), (3, 2, 128, 32, 1, 0)])
def test_equal_logits_keep_the_first_positions(L, B, NI, D, hid, H, S, kind):
    """w2 = 0: every logit is b2; sel == S + 1 .. S + H, the softmax loss log(1 + H), every output finite (Out.get checks that)."""
    c = LW.case(B, NI, D, hid, "mixed")
    c = dict(c, W=dict(c["W"], w2=torch.zeros(hid)))
    got = launch(L, c, kind, H, S, 0)
    assert torch.equal(got["sel"], torch.arange(S + 1, S + H + 1).expand(B, H))
    assert torch.equal(got["z"], c["W"]["b2"].expand(B, NI))
    loss = float(got["loss_part"].double().sum())
    want = math.log(1 + H) if kind == LW.SOFTMAX else math.log(2.0)
    # lse = fl(m + fl(logf(NC))) (exp(0) sums exactly), minus z0, over B: a few roundings at the size |b2| + log NC, logf within 2 ulp
    tol = 4 * 2.0 ** -23 * (abs(float(c["W"]["b2"])) + math.log(1 + H))
    print(f"mined kind {kind} equal logits [{B}x{NI} H {H} S {S}] loss {loss:.9f} expected {want:.9f} tol {tol:.2e}")
    assert abs(loss - want) <= tol


@pytest.mark.parametrize("H,S,kept_of_three", [(2, 0, (0, 1)), (1, 1, (1,)), (3, 2, (2,))])
def test_a_repeated_item_row_ties_by_position(L, H, S, kept_of_three):
    """The top-ranked negative's row copied to two more positions: three equal logits at the ranks 0, 1, 2 in position order."""
    B, NI, D, hid = 2, 65, 128, 32
    c = LW.case(B, NI, D, hid, "mixed")
    zo = MR.own_rows(MR.case_z64(B, NI, D, hid, "mixed"), c["domain_id"])
    items = c["items"].clone()
    spots = []
    for b in range(B):
        order = torch.argsort(zo[b, 1:], descending=True) + 1
        assert float(zo[b, order[0]] - zo[b, order[1]]) > 1e-3, "the case's top negative is not clear of the second"
        src, low = int(order[0]), sorted(int(x) for x in order[-2:])
        items[b, low[0]] = items[b, src]
        items[b, low[1]] = items[b, src]
        spots.append(sorted([src] + low))
    c = dict(c, items=items)
    got = launch(L, c, LW.SOFTMAX, H, S, 0)
    for b in range(B):
        s = spots[b]
        assert float(got["z"][b, s[0]]) == float(got["z"][b, s[1]]) == float(got["z"][b, s[2]]), "equal rows, different logits"
        kept = [x for x in s if x in got["sel"][b].tolist()]
        assert kept == [s[i] for i in kept_of_three], (b, s, got["sel"][b].tolist())
    ref64, ref32 = refs_on(c, LW.SOFTMAX, H, S, got["sel"])
    check(LW.SOFTMAX, f"repeated row H {H} S {S}", got, ref64, ref32)


@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
@pytest.mark.parametrize("B,NI,D,hid,H,S", [(2, 65, 128, 32, 8, 0), (3, 2, 128, 32, 1, 0)])
def test_saturated_logits(L, B, NI, D, hid, H, S, kind):
    """b2 = +40, every p == 1.0f: finite, and the float32 restatement's values on the kernel's selection (test_gpu_listwise.py's bar)."""
    c = LW.case(B, NI, D, hid, "mixed", True)
    got = launch(L, c, kind, H, S, 0)
    _, ref32 = refs_on(c, kind, H, S, got["sel"])
    assert torch.equal(got["p"], torch.ones(2, B, NI)) and float(got["dz"].abs().max()) > 0
    bad = []
    for k in got:
        if k == "sel":
            continue
        e = errors(got, ref32, k, ref32["dz"].double())
        print(f"mined kind {kind} saturated [{B}x{NI} H {H}] {k} e against float32 {e:.3e} bar {SAT_BAR:.3e}")
        log(f"mined kind {kind} saturated [{B}x{NI} H {H}] {k} e against float32 {e:.3e}")
        if not e <= SAT_BAR:
            bad.append((k, e))
    assert not bad, bad


def test_refusals(L):
    from amid_amd._lib import AmidError
    B, NI, D, hid = 2, 5, 96, 24
    c = LW.case(B, NI, D, hid, "mixed")
    for change, code in ((dict(keep=0), ARG), (dict(skip=-1), ARG), (dict(keep=4, skip=1), ARG), (dict(keep=5), ARG), (dict(sel=None), ARG),
                         (dict(z=None), ARG), (dict(kind=0), ARG), (dict(NI=1), ARG), (dict(NI=1025), UNSUPPORTED), (dict(D=160), UNSUPPORTED),
                         (dict(hid=6), UNSUPPORTED), (dict(du=None), ARG)):
        with pytest.raises(AmidError) as e:
            launch(L, c, LW.SOFTMAX, 2, 1, 0, change)
        torch.cuda.synchronize()
        assert e.value.code == code, (change, e.value.code)
