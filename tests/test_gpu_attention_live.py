"""The attention core of the train step over a live list -- amid_attn_fwd_live_f32 / amid_attn_bwd_live_f32 (causal, csrc/attention_mfma.hip)
and amid_attn_bert_fwd_live_f32 / amid_attn_bert_bwd_live_f32 (bidirectional, csrc/attention_mfma_bert.hip) -- through the C ABI:

  a. amid_live_list_i32 against numpy;
  b. the live pair against the full launches amid_attn_fwd_f32 / amid_attn_bwd_f32 bit for bit on the live sequences, with every dead
     sequence NaN on the way in (nothing dead is read) and NaN on the way out (nothing dead is written);
  c. the same live outputs, and the full launches of the shapes tests/test_gpu_kernels.py does not hold, against tests/attention_ref.py
     in float64;
  d. amid_attn_live_supported / amid_attn_bert_live_supported against what the entries accept, on both sides of every limit.

Bar of c, per tensor: e = max|x - ref64| / max|ref64| <= 4 e_f32 + 2^-22 (profiles/innercomp_kernels.md), e_f32 the larger figure of two
float32 restatements on the CPU (torch's exp; exp2(x log2 e) with the product rounded, the matrix-core kernels' exponential), and never
above what the full launches meet in tests/test_gpu_kernels.py: causal o 2e-6, gradients 5e-6; bidirectional o 3e-6, gradients 1e-5.  The
two columns of the row statistics: 1e-5 each (tests/test_gpu_seqn.py).  Bidirectional: the sequences whose keys are ALL masked apart from
the rest (their -1e9 row maximum would set the scale of everything else; their dq and dk are exact zeros).

A tensor the float64 reference has exactly zero -- dq and dk at T = 1, where softmax of one key has no gradient -- has no scale of its
own.  The kernels form dS = P (dP~ - delta) there from two float32 sums of the same hd products in different orders (dP~ = dscale dO . V
by the matrix cores, delta = dO . O with O = dscale V), each within hd 2^-24 (hd dscale max|dO| max|V|) of the exact value, and multiply
by one key (query) row and the score scale: |x| <= 2 hd 2^-24 . hd dscale max|dO| max|V| max|k| sqrt(1/hd) is asserted instead.

Every figure goes to the parity log; the worst per entry point and tensor: profiles/attention_kernels.md."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import attention_ref as R
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
OK, ERR_ARG, UNSUPPORTED = 0, -1, -2          # include/amid_hip.h
SEED, STEP = 77, 4
GUARD = 256                                   # floats of sentinel on both sides of every output
SENT = 12345.0
CEIL = {(1, "o"): 2e-6, (1, "g"): 5e-6, (0, "o"): 3e-6, (0, "g"): 1e-5}      # (causal, o / gradient): tests/test_gpu_kernels.py
STATS_BAR = 1e-5


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


def step_state(L, seed, step, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8):
    n = L.value("amid_step_state_bytes")
    host = (ctypes.c_ubyte * n)()
    L.call("amid_step_state_pack", ctypes.addressof(host), seed, step, lr, b1, b2, eps)
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()


class Out:
    """A NaN-filled device output between two guards."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((GUARD + n + GUARD,), SENT, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(float("nan"))

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self, tag):
        b, n = self.buf.cpu(), self.t.numel()
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), f"{tag}: a write outside the output"
        return b[GUARD:GUARD + n].view(self.t.shape).clone()


def domains(B, doms):
    if doms == "all0":
        return torch.zeros(B, dtype=torch.int64)
    if doms == "all1":
        return torch.ones(B, dtype=torch.int64)
    d = (torch.rand(B, generator=torch.Generator().manual_seed(B)) < 0.5).long()
    d[0], d[1] = 1, 0                         # both kinds, and slot 0 is not batch row 0
    return d


def live_list_ref(dom):
    d = dom.numpy()
    rows = np.arange(len(d))
    return np.concatenate((rows[d == 0], rows[d != 0], [int((d == 0).sum())])).astype(np.int32)


def run_live_list(L, dom):
    B = len(dom)
    buf = torch.full((B + 3,), -7, dtype=torch.int32, device="cuda")
    L.call("amid_live_list_i32", dev(dom).data_ptr(), B, buf.data_ptr(), stream())
    torch.cuda.synchronize()
    return buf


# ---------------------------------------------------------------------------- a. the live list
@pytest.mark.parametrize("doms", ["all0", "all1", "mixed"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1030])
def test_live_list_equals_numpy(L, B, doms):
    dom = domains(B, doms) if B > 1 else domains(B, "all1" if doms == "mixed" else doms)
    if doms == "mixed" and B > 1:
        dom = dom * 3                          # any nonzero id is domain 1
    got = run_live_list(L, dom).cpu().numpy()
    assert np.array_equal(got[:B + 1], live_list_ref(dom))
    assert got[B + 1] == -7 and got[B + 2] == -7, "the list is B + 1 ints"


# ---------------------------------------------------------------------------- the cases
# (causal, B, T, D, H, train, layer, doms)
def _causal_cases(dh, ts, edge_dh, big_dh, train0_t):
    out, i = [], 0
    for D, H in dh:
        for T in ts:
            out.append((1, 5, T, D, H, 1, i % 2, "mixed"))
            i += 1
    for (D, H), T in zip(dh, train0_t):
        out.append((1, 5, T, D, H, 0, i % 2, "mixed"))
        i += 1
    D, H = edge_dh
    out += [(1, 1, 50, D, H, 1, 0, "all0"), (1, 1, 50, D, H, 1, 1, "all1"), (1, 6, 50, D, H, 1, 1, "all0"), (1, 6, 50, D, H, 1, 0, "all1"),
            (1, 1030, 16, *big_dh, 1, 1, "mixed")]
    return out


HD16 = _causal_cases([(128, 8), (64, 4), (16, 1), (48, 3), (96, 6)], [1, 15, 16, 17, 33, 48, 49, 64], (128, 8), (64, 4), [49, 17, 64, 1, 33])
# the head counts mfma_shape admits at head dim 16 that the list above leaves out: workgroups of 2, 5 and 7 waves
HD16 += [(1, 5, T, 16 * H, H, 1, H % 2, "mixed") for H in (2, 5, 7) for T in (16, 49)]
HD8 = _causal_cases([(64, 8), (32, 4), (16, 2), (48, 6)], [1, 16, 33, 50, 64], (64, 8), (64, 8), [50, 16, 64, 33])
BERT = [(0, 5, T, 128, 4, train, (T + train) % 2, "mixed") for T in (1, 15, 16, 17, 32, 33, 48, 50, 64) for train in (0, 1)]
BERT += [(0, 1, 50, 128, 4, 1, 0, "all0"), (0, 1, 50, 128, 4, 1, 1, "all1"), (0, 6, 50, 128, 4, 1, 1, "all0"), (0, 6, 50, 128, 4, 1, 0, "all1"),
         (0, 300, 16, 128, 4, 1, 1, "mixed")]
LIVE = HD16 + HD8 + BERT
# full launches only: bidirectional heads of 32 beside the model's four -- (256, 8), (160, 5): the general kernels (bert_shape admits H <= 4);
# (64, 2), (32, 1), (96, 3): the matrix-core kernels with 2 H = 4, 2, 6 forward and H = 2, 1, 3 backward waves
FULL_BIDIR = [(0, 3, T, D, H, train, (T // 4 + train) % 2, "mixed") for D, H in ((256, 8), (160, 5), (64, 2), (32, 1), (96, 3)) for T in (20, 64)
              for train in (0, 1)]
# causal shapes of the list that test_attention_fwd_bwd_vs_autograd does not run as full launches
_HELD = {(D, H, T) for D, H in ((128, 8), (64, 8), (32, 4), (16, 2)) for T in (64, 50, 17)}
FULL = [c for c in HD16 + HD8 if c[1] == 5 and (c[3], c[4], c[2]) not in _HELD] + FULL_BIDIR


def case_id(c):
    causal, B, T, D, H, train, layer, doms = c
    return f"{'causal' if causal else 'bidir'}-B{B}-T{T}-D{D}-H{H}-train{train}-layer{layer}-{doms}"


def p_of(c):
    return 0.5 if c[0] else 0.1


@functools.lru_cache(maxsize=None)
def inputs(c):
    causal, B, T, D, H, train, layer, doms = c
    g = torch.Generator().manual_seed(1000 * T + 10 * D + H + B)
    q, k, v, d_o = (torch.randn(2 * B, T, D, generator=g) for _ in range(4))          # d_o nonzero on every sequence
    dom = domains(B, doms)
    key_keep = None
    if not causal:
        key_keep = torch.rand(B, T, generator=g) > 0.3                                   # a different mask per batch row
        if B > 1:
            key_keep[0] = False                                                          # every key of batch row 0 masked,
            key_keep[1] = True                                                           # none of batch row 1
    live_seq = torch.cat((dom == 0, dom != 0))                                           # [2B]: sequence g * B + b is live iff dom[b] == g
    return dict(q=q, k=k, v=v, d_o=d_o, dom=dom, key_keep=key_keep, live_seq=live_seq)


def launch(L, c, x, live):
    """forward then backward (on the forward's own o / stats) over every sequence (live None) or the list's; x: device inputs"""
    causal, B, T, D, H, train, layer, _ = c
    p = p_of(c)
    st = step_state(L, SEED, STEP)
    o, dq, dk, dv = (Out(2 * B, T, D) for _ in range(4))
    stats = Out(2 * B, T, H, 2)
    q, k, v, d_o = (x[n].data_ptr() for n in ("q", "k", "v", "d_o"))
    kk = x["kk"].data_ptr() if x["kk"] is not None else None
    tail = (st.data_ptr(), train, p)
    if live is None:
        L.call("amid_attn_fwd_f32", q, k, v, kk, B, T, D, H, causal, layer, *tail, o.data_ptr(), stats.data_ptr(), stream())
        L.call("amid_attn_bwd_f32", q, k, v, o.data_ptr(), stats.data_ptr(), d_o, kk, B, T, D, H, causal, layer, *tail, dq.data_ptr(),
               dk.data_ptr(), dv.data_ptr(), stream())
    elif causal:
        L.call("amid_attn_fwd_live_f32", q, k, v, B, T, D, H, 1, layer, *tail, o.data_ptr(), stats.data_ptr(), live.data_ptr(), stream())
        L.call("amid_attn_bwd_live_f32", q, k, v, o.data_ptr(), stats.data_ptr(), d_o, B, T, D, H, 1, layer, *tail, dq.data_ptr(), dk.data_ptr(),
               dv.data_ptr(), live.data_ptr(), stream())
    else:
        L.call("amid_attn_bert_fwd_live_f32", q, k, v, kk, B, T, D, H, layer, *tail, o.data_ptr(), stats.data_ptr(), live.data_ptr(), stream())
        L.call("amid_attn_bert_bwd_live_f32", q, k, v, o.data_ptr(), stats.data_ptr(), d_o, kk, B, T, D, H, layer, *tail, dq.data_ptr(),
               dk.data_ptr(), dv.data_ptr(), live.data_ptr(), stream())
    torch.cuda.synchronize()
    tag = case_id(c) + (" full" if live is None else " live")
    return {n: t.get(f"{tag} {n}") for n, t in (("o", o), ("stats", stats), ("dq", dq), ("dk", dk), ("dv", dv))}


@functools.lru_cache(maxsize=None)
def _gpu(c, which):
    from amid_amd._lib import lib
    L = lib()
    x = inputs(c)
    kk = dev(x["key_keep"].to(torch.uint8)) if x["key_keep"] is not None else None
    if which == "full":
        return launch(L, c, dict(q=dev(x["q"]), k=dev(x["k"]), v=dev(x["v"]), d_o=dev(x["d_o"]), kk=kk), None)
    dead = ~x["live_seq"]
    poisoned = {}
    for n in ("q", "k", "v", "d_o"):
        t = x[n].clone()
        t[dead] = float("nan")
        poisoned[n] = dev(t)
    live = run_live_list(L, x["dom"])
    return launch(L, c, dict(poisoned, kk=kk), live)


@functools.lru_cache(maxsize=None)
def refs(c):
    """float64 and the two float32 restatements, on all 2 B sequences"""
    causal, B, T, D, H, train, layer, _ = c
    x, p = inputs(c), p_of(c)
    keep = R.keep_masks_both(B, H, T, SEED, STEP, layer, p) if train else None

    def one(dtype, exp2):
        if causal:
            return R.causal(x["q"], x["k"], x["v"], H, dtype, keep=keep, p=p, d_o=x["d_o"], exp2=exp2)
        return R.bidirectional(x["q"], x["k"], x["v"], x["key_keep"].repeat(2, 1), H, dtype, keep=keep, p=p, d_o=x["d_o"], exp2=exp2)
    return one(torch.float64, False), (one(torch.float32, False), one(torch.float32, True))


def zero_bound(c, x, name, sel):
    """|dq|, |dk| where the reference has exact zeros: see the module's docstring"""
    D, H = c[3], c[4]
    hd = D // H
    dscale = 1.0 / (1.0 - p_of(c)) if c[5] else 1.0
    other = x["k"] if name == "dq" else x["q"]
    big = lambda t: float(t[sel].abs().max())
    return 2 * hd * 2.0 ** -24 * hd * dscale * big(x["d_o"]) * big(x["v"]) * big(other) * math.sqrt(1.0 / hd)


def _named(d):
    return {"o": d["o"], "dq": d["dq"], "dk": d["dk"], "dv": d["dv"], "stats.max": d["stats"][..., 0], "stats.rsum": d["stats"][..., 1]}


def check_fp64(c, got, sel, tag):
    """got [2B, ...] outputs, sel [2B] bool: the sequences to compare.  Logs every figure; returns the lines over their bar."""
    causal = c[0]
    x = inputs(c)
    r64, r32 = refs(c)
    got, r64, r32 = _named(got), _named(r64), [_named(y) for y in r32]
    groups = [("", sel)]
    if not causal:
        masked = (~x["key_keep"].any(1)).repeat(2)
        groups = [(" kept", sel & ~masked), (" allmasked", sel & masked)]
    bad = []
    for gname, s in groups:
        if not bool(s.any()):
            continue
        for n in got:
            gt, r = got[n][s], r64[n][s]
            assert not bool(torch.isnan(gt).any()), f"{tag}{gname} {n}: NaN"
            if float(r.abs().max()) == 0.0:
                # exact zeros: everything dropped, or no score gradient (every key masked: masked_fill) -- but for dq / dk of a single key
                ek = float(gt.abs().max())
                bar = zero_bound(c, x, n, s) if n in ("dq", "dk") and gname != " allmasked" else 0.0
                line = f"attention {tag}{gname} {n:10s} reference zero: max|x| {ek:.3e} bound {bar:.3e}"
            else:
                ek, ef = R.err(gt, r), [R.err(y[n][s], r) for y in r32]
                bar = STATS_BAR if n.startswith("stats") else min(4 * max(ef) + R.FLOOR, CEIL[(causal, "o" if n == "o" else "g")])
                line = f"attention {tag}{gname} {n:10s} e_kernel {ek:.3e} e_f32 exp {ef[0]:.3e} exp2 {ef[1]:.3e} bar {bar:.3e} ratio {ek / bar:.2f}"
            log(line)
            print(line)
            if not ek <= bar:
                bad.append(line)
    return bad


# ---------------------------------------------------------------------------- b. the live pair is the full launch on the live sequences
@pytest.mark.parametrize("c", LIVE, ids=case_id)
def test_live_launch_equals_full_launch_bits_and_touches_nothing_dead(c):
    full, live = _gpu(c, "full"), _gpu(c, "live")
    ls = inputs(c)["live_seq"]
    for n in ("o", "stats", "dq", "dk", "dv"):
        assert not bool(torch.isnan(full[n]).any()), f"{n}: the full launch left something unwritten"
        assert not bool(torch.isnan(live[n][ls]).any()), f"{n}: NaN on a live sequence (a dead sequence read, or a row not written)"
        assert bool(torch.isnan(live[n][~ls]).all()), f"{n}: a dead sequence was written"
        assert torch.equal(live[n][ls], full[n][ls]), f"{n}: live launch != full launch, relmax {relmax(live[n][ls], full[n][ls]):.3e}"


# ---------------------------------------------------------------------------- c. against float64
@pytest.mark.parametrize("c", LIVE, ids=case_id)
def test_live_launch_against_fp64(c):
    bad = check_fp64(c, _gpu(c, "live"), inputs(c)["live_seq"], case_id(c) + " live")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", FULL, ids=case_id)
def test_full_launch_against_fp64(c):
    bad = check_fp64(c, _gpu(c, "full"), torch.ones(2 * c[1], dtype=torch.bool), case_id(c) + " full")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------- d. *_supported and what the entries accept
def _arg_error(T, D, H):
    """what every attention entry calls a bad argument (attn_fill, csrc/attention.hip) rather than an unsupported shape"""
    return T <= 0 or H <= 0 or H > 8 or D % H != 0


def _try_entries(L, T, D, H, causal, bert, null=None):
    """both live entries of a form on B = 1 at (T, D, H): return codes and the outputs.  null: one argument passed as NULL."""
    Tb, Db, Hb = max(T, 1), max(D, 4), max(H, 1)
    g = torch.Generator().manual_seed(T + D + H)
    q, k, v, d_o = (dev(torch.randn(2, Tb, Db, generator=g)) for _ in range(4))
    kk = dev(torch.ones(1, Tb, dtype=torch.uint8))
    live = run_live_list(L, torch.zeros(1, dtype=torch.int64))
    st = step_state(L, SEED, STEP)
    o, dq, dk, dv, stats = Out(2, Tb, Db), Out(2, Tb, Db), Out(2, Tb, Db), Out(2, Tb, Db), Out(2, Tb, Hb, 2)
    P = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), d_o=d_o.data_ptr(), o=o.data_ptr(), stats=stats.data_ptr(), dq=dq.data_ptr(),
             dk=dk.data_ptr(), dv=dv.data_ptr(), live=live.data_ptr(), kk=kk.data_ptr())
    fwd_null, bwd_null = null if null is not None else (None, None)
    F, Bw = dict(P), dict(P)
    if fwd_null:
        F[fwd_null] = None
    if bwd_null:
        Bw[bwd_null] = None
    tail = (st.data_ptr(), 1, 0.5 if not bert else 0.1)
    if bert:
        rf = L.raw("amid_attn_bert_fwd_live_f32")(F["q"], F["k"], F["v"], F["kk"], 1, T, D, H, 0, *tail, F["o"], F["stats"], F["live"], stream())
        torch.cuda.synchronize()
        fwd_out = [o.get("o"), stats.get("stats")]
        if rf == OK and not fwd_null:
            assert not bool(torch.isnan(fwd_out[0][0]).any())
        else:                                     # the backward's check needs finite o / stats only where it would launch
            o.t.zero_(); stats.t.fill_(1.0)
        rb = L.raw("amid_attn_bert_bwd_live_f32")(Bw["q"], Bw["k"], Bw["v"], Bw["o"], Bw["stats"], Bw["d_o"], Bw["kk"], 1, T, D, H, 0, *tail, Bw["dq"],
                                                  Bw["dk"], Bw["dv"], Bw["live"], stream())
    else:
        rf = L.raw("amid_attn_fwd_live_f32")(F["q"], F["k"], F["v"], 1, T, D, H, causal, 0, *tail, F["o"], F["stats"], F["live"], stream())
        torch.cuda.synchronize()
        fwd_out = [o.get("o"), stats.get("stats")]
        if rf == OK and not fwd_null:
            assert not bool(torch.isnan(fwd_out[0][0]).any())
        else:
            o.t.zero_(); stats.t.fill_(1.0)
        rb = L.raw("amid_attn_bwd_live_f32")(Bw["q"], Bw["k"], Bw["v"], Bw["o"], Bw["stats"], Bw["d_o"], 1, T, D, H, causal, 0, *tail, Bw["dq"],
                                             Bw["dk"], Bw["dv"], Bw["live"], stream())
    torch.cuda.synchronize()
    return rf, rb, fwd_out, [dq.get("dq"), dk.get("dk"), dv.get("dv")]


def _check_point(L, T, D, H, causal, bert, supported):
    rf, rb, fwd_out, bwd_out = _try_entries(L, T, D, H, causal, bert)
    where = f"T {T} D {D} H {H} causal {causal}"
    if supported:
        assert (rf, rb) == (OK, OK), (where, rf, rb)
        for t in fwd_out + bwd_out:                # sequence (0, 0) written, sequence (1, 0) not
            assert not bool(torch.isnan(t[0]).any()) and bool(torch.isnan(t[1]).all()), where
    else:
        want = ERR_ARG if _arg_error(T, D, H) else UNSUPPORTED
        assert (rf, rb) == (want, want), (where, rf, rb, want)
        for t in fwd_out + bwd_out:
            assert bool(torch.isnan(t).all()), f"{where}: a refused call wrote something"


def test_causal_live_supported_agrees_with_the_entries(L):
    """On both sides of every limit: T 0 / 1 / 64 / 65, head dim 4 / 8 / 16 / 32, H 0 / 1 / 8 / 9, odd H at head dim 8, causal 0, D % H != 0.
    A refused call returns AMID_ERR_UNSUPPORTED -- AMID_ERR_ARG where the arguments are ones every attention entry rejects (T <= 0, H outside
    1 .. 8, D % H != 0) -- and writes nothing."""
    n_yes = 0
    for T in (0, 1, 64, 65):
        for hd in (4, 8, 16, 32):
            for H in (0, 1, 2, 3, 7, 8, 9):
                for causal in (1, 0):
                    D = hd * max(H, 1)
                    sup = L.value("amid_attn_live_supported", T, D, H, causal)
                    want = causal == 1 and 1 <= T <= 64 and 1 <= H <= 8 and (hd == 16 or (hd == 8 and H % 2 == 0))
                    assert sup == (1 if want else 0), (T, D, H, causal, sup)
                    _check_point(L, T, D, H, causal, False, sup == 1)
                    n_yes += sup
    for T, D, H in ((16, 20, 3), (16, 100, 8)):      # D % H != 0
        assert L.value("amid_attn_live_supported", T, D, H, 1) == 0
        _check_point(L, T, D, H, 1, False, False)
    assert n_yes == 2 * (5 + 2)                       # T 1, 64 x (head dim 16: H 1, 2, 3, 7, 8; head dim 8: H 2, 8)


def test_bert_live_supported_agrees_with_the_entries(L):
    n_yes = 0
    for T in (0, 1, 64, 65):
        for D, H in ((128, 4), (64, 2), (32, 1), (96, 3), (160, 5), (256, 8), (128, 8), (64, 4), (256, 4), (128, 0), (288, 9), (130, 4)):
            sup = L.value("amid_attn_bert_live_supported", T, D, H)
            assert sup == (1 if (1 <= T <= 64 and D == 128 and H == 4) else 0), (T, D, H, sup)
            _check_point(L, T, D, H, 0, True, sup == 1)
            n_yes += sup
    assert n_yes == 2


@pytest.mark.parametrize("bert", [False, True])
def test_null_live_list_or_output_is_an_argument_error(L, bert):
    T, D, H = (16, 128, 4) if bert else (16, 64, 4)
    for null in (("live", "live"), ("o", "dq"), ("o", "dk"), ("o", "dv"), ("q", "d_o"), ("k", "stats"), ("v", "o")):
        rf, rb, fwd_out, bwd_out = _try_entries(L, T, D, H, 1, bert, null)
        assert (rf, rb) == (ERR_ARG, ERR_ARG), (null, rf, rb)
        for t in fwd_out + bwd_out:
            assert bool(torch.isnan(t).all()), f"{null}: a refused call wrote something"
