"""amid_scorer_listwise_fwd_bwd_f32 (csrc/head_listwise.hip: scorer forward over a row's NI candidates, sampled softmax or BPR on the own
domain's logits, scorer backward from dLoss/dz -- one launch) through the C ABI against the float64 restatement tests/listwise_ref.py, which
tests/test_listwise_ref.py holds to torch.autograd.

Bar, per output tensor, as tests/test_gpu_head.py: e = max|x - ref64| / max|ref64|; e_kernel <= 4 e_f32 + 2^-22, e_f32 the same figure for the
float32 restatement on the CPU.  One tensor has another denominator: sc_db2, the per-row sum of dz, is 0 in exact arithmetic under both
objectives (neither changes when every logit moves alike), so max|ref64| is rounding noise (1e-19) and the quotient means nothing; its errors
are divided by the largest row sum of |dz| instead -- the size of the terms whose sum it is.  Same bar otherwise.  A tensor measured over its
bar although the kernel is right would get its factor in FACTOR with the figures (profiles/listwise_loss.md); none has been.

Exact (torch.equal): p1 / p2 against amid_scorer_fwd_f32 on the same inputs, the other domain's dz rows and du half (0), the transposed
matrices; every output lies between untouched guards (Out).

Saturation (b2 = +40: every p == 1.0f, where a gradient sent through p would be divided by p (1 - p) = 0): every output finite and held to
the FLOAT32 restatement.  Bar 2^-14, from the number format: a logit near 40 is rounded to an ulp of 2^-18, the objectives read differences
of two logits, and the device's and the host's evaluation of a logit may differ by one such rounding each -- 4 ulp on a difference, which the
exponentials pass on as a relative error of the same size; the gradients are sums of such terms with both signs, for which a further factor
of 4 is allowed: 16 * 2^-18.  With equal logits (w2 = 0) the softmax loss is log NI to that rounding.

Which case reaches what (B, NI, D, hid): (1, 2, 32, 4) the smallest, idle lanes in every phase; NI 64 / 65 the item-chunk edge (one chunk with
the forward's pre-activations reused, two chunks recomputed and dW1 accumulated in place); 130 three chunks; (1, 1024, 128, 64) the NI limit
(two candidates a thread in the objective's sums, the largest LDS carve); n_tr 3 the transpose riders on extra workgroups.

A test of this file after which the device reports an error ends the whole pytest session (stop_at_a_gpu_fault)."""
import math

import pytest
import torch

from tests import head_ref as R
from tests import listwise_ref as LW
from tests.test_gpu_head import take_rows
from tests.test_gpu_intercomp import FLOOR, UNSUPPORTED, L, Out, err, pa, stream  # noqa: F401  (L: the library fixture)
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
ENTRY = "amid_scorer_listwise_fwd_bwd_f32"
ARG = -1
SHAPES = [(1, 2, 32, 4), (3, 2, 128, 32), (2, 5, 96, 24), (2, 64, 128, 32), (2, 65, 128, 32), (2, 130, 64, 16), (1, 1024, 128, 64)]
FACTOR = {}                      # (kind, tensor) -> a factor other than 4, with its figures: none measured over the bar
SAT_BAR = 2.0 ** -14


@pytest.fixture(autouse=True)
def stop_at_a_gpu_fault():
    """A kernel that faulted leaves the device unusable for this process: end the session there instead of launching the remaining cases."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, nothing more is launched: {e}", returncode=3)


def launch(L, c, kind, n_tr, change=()):
    """The launch on a case's inputs: its outputs by name after the exact checks."""
    B, NI, D = c["items"].shape
    hid = c["W"]["b1"].numel()
    d = {k: c[k].cuda() for k in ("u", "items", "domain_id")}
    W = {k: v.cuda() for k, v in c["W"].items()}
    o = dict(p1=Out(B, NI), p2=Out(B, NI), dz1=Out(B, NI), dz2=Out(B, NI), loss_part=Out(B), du=Out(2, B, D), ditems=Out(B, NI, D),
             sc_part=Out(B, R.part_floats(D, hid)))
    g = torch.Generator().manual_seed(n_tr)
    tr_src, tr_dst = [torch.randn(D, D, generator=g).cuda() for _ in range(n_tr)], [Out(D, D) for _ in range(n_tr)]
    tab = dict({k: v.data_ptr() for k, v in d.items()}, **{k: v.data_ptr() for k, v in W.items()}, kind=kind, B=B, NI=NI, D=D, hid=hid,
               **{k: v.data_ptr() for k, v in o.items()}, tr_src=pa(tr_src) if n_tr else None, tr_dst=pa(tr_dst) if n_tr else None, n_tr=n_tr,
               stream=stream())
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
    du = o["du"].get("du")
    oth, ar = 1 - (c["domain_id"] != 0).long(), torch.arange(B)
    assert torch.equal(dz[oth, ar], torch.zeros(B, NI)), "dz of the other domain"
    assert torch.equal(du[oth, ar], torch.zeros(B, D)), "du of the other domain"
    for i, (src, dst) in enumerate(zip(tr_src, tr_dst)):
        assert torch.equal(dst.get(f"tr_dst[{i}]"), src.cpu().t()), f"transpose {i}"
    rows = take_rows(o["sc_part"], hid * 2 * D + 2 * hid + 1, "sc_part")
    w = hid * 2 * D
    return dict(p=p, dz=dz, du=du, ditems=o["ditems"].get("ditems"), loss_part=o["loss_part"].get("loss_part"), sc_dW1=rows[:, :w],
                sc_db1=rows[:, w:w + hid], sc_dW2=rows[:, w + hid:w + 2 * hid], sc_db2=rows[:, w + 2 * hid:])


def errors(got, ref, k, dz64):
    """e of tensor k; sc_db2 (0 in exact arithmetic) against the largest row sum of |dz| (the module docstring)."""
    if k == "sc_db2":
        return float((got[k].double() - ref[k].double()).abs().max() / dz64.abs().sum((0, 2)).max())
    return err(got[k], ref[k].double())


def check(kind, tag, got, ref64, ref32):
    bad = []
    for k in got:
        ek, ef = errors(got, ref64, k, ref64["dz"]), errors(ref32, ref64, k, ref64["dz"])
        f = FACTOR.get((kind, k), 4)
        log(f"listwise kind {kind} [{tag}] {k} e_kernel {ek:.3e} e_f32 {ef:.3e}")
        print(f"listwise kind {kind} [{tag}] {k} e_kernel {ek:.3e} e_f32 {ef:.3e} bar {f * ef + FLOOR:.3e}")
        if not ek <= f * ef + FLOOR:
            bad.append((k, ek, ef))
    assert not bad, (kind, tag, bad)


@pytest.mark.parametrize("n_tr", [0, 3])
@pytest.mark.parametrize("dom", ["mixed", 0, 1])
@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
@pytest.mark.parametrize("B,NI,D,hid", SHAPES)
def test_listwise_against_fp64(L, B, NI, D, hid, kind, dom, n_tr):
    c = LW.case(B, NI, D, hid, dom)
    ref64, ref32 = LW.refs(B, NI, D, hid, dom, kind)
    check(kind, f"{B}x{NI} D {D} hid {hid} dom {dom} n_tr {n_tr}", launch(L, c, kind, n_tr), ref64, ref32)


@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
@pytest.mark.parametrize("B,NI,D,hid", [(2, 65, 128, 32), (3, 2, 128, 32)])
def test_saturated_logits(L, B, NI, D, hid, kind):
    """b2 = +40, every p == 1.0f: finite, and the float32 restatement's values (the module docstring's bar)."""
    c = LW.case(B, NI, D, hid, "mixed", True)
    _, ref32 = LW.refs(B, NI, D, hid, "mixed", kind, True)
    got = launch(L, c, kind, 0)
    assert torch.equal(got["p"], torch.ones(2, B, NI)) and float(got["dz"].abs().max()) > 0
    bad = []
    for k in got:
        e = errors(got, ref32, k, ref32["dz"].double())
        print(f"listwise kind {kind} saturated [{B}x{NI}] {k} e against float32 {e:.3e} bar {SAT_BAR:.3e}")
        log(f"listwise kind {kind} saturated [{B}x{NI}] {k} e against float32 {e:.3e}")
        if not e <= SAT_BAR:
            bad.append((k, e))
    assert not bad, bad


def test_softmax_loss_of_equal_saturated_logits_is_log_ni(L):
    B, NI, D, hid = 2, 65, 128, 32
    c = LW.case(B, NI, D, hid, "mixed", True)
    c = dict(c, W=dict(c["W"], w2=torch.zeros(hid)))
    d = {k: c[k].cuda() for k in ("u", "items", "domain_id")}
    W = {k: v.cuda() for k, v in c["W"].items()}
    o = dict(p1=Out(B, NI), p2=Out(B, NI), dz1=Out(B, NI), dz2=Out(B, NI), loss_part=Out(B), du=Out(2, B, D), ditems=Out(B, NI, D),
             sc_part=Out(B, R.part_floats(D, hid)))
    L.call_named(ENTRY, {k: v.data_ptr() for k, v in d.items()}, {k: v.data_ptr() for k, v in W.items()}, {k: v.data_ptr() for k, v in o.items()},
                 kind=LW.SOFTMAX, B=B, NI=NI, D=D, hid=hid, tr_src=None, tr_dst=None, n_tr=0, stream=stream())
    torch.cuda.synchronize()
    loss = float(o["loss_part"].get("loss_part").double().sum())
    print(f"softmax loss at equal logits {loss:.9f}, log NI {math.log(NI):.9f}")
    assert abs(loss - math.log(NI)) <= 4 * 2.0 ** -18
    assert all(bool(torch.isfinite(o[k].get(k)).all()) for k in ("dz1", "dz2", "du", "ditems"))


def test_refusals(L):
    from amid_amd._lib import AmidError
    B, NI, D, hid = 2, 5, 96, 24
    c = LW.case(B, NI, D, hid, "mixed")
    for change, code in ((dict(kind=0), ARG), (dict(kind=3), ARG), (dict(NI=1), ARG), (dict(NI=1025), UNSUPPORTED), (dict(D=160), UNSUPPORTED),
                         (dict(D=48), UNSUPPORTED), (dict(hid=68), UNSUPPORTED), (dict(hid=6), UNSUPPORTED), (dict(du=None), ARG)):
        with pytest.raises(AmidError) as e:
            launch(L, c, LW.SOFTMAX, 0, change)
        torch.cuda.synchronize()
        assert e.value.code == code, (change, e.value.code)
