"""The head of a train step -- last LayerNorm + mean over time, the predictModule scorer, the masked BCE or the doubly-robust objectives, and
their backward (amid_amd/csrc/head.hip, head_fused.hip, head_parts.h) -- entry point by entry point through the C ABI against the float64
restatement tests/head_ref.py (which tests/test_head_ref.py holds to torch.autograd), at the shapes on both sides of every form the kernels
choose between.

Bar, per output tensor, as tests/test_gpu_intercomp.py: e = max|x - ref64| / max|ref64|; e_kernel <= 4 e_f32 + 2^-22, e_f32 the same figure for
the float32 restatement on the CPU (8 or 16 instead of 4 for seven tensors of the doubly-robust objectives that were measured over it: FACTOR,
below, each with its figures and the reason).  Both figures of every case and tensor go to the parity log; the worst per entry point and tensor:
profiles/head_kernels.md.  Exact (torch.equal) and not under the bar: transposed matrices, the gradients of the head a row does not use, and
in the `own` forms the other domain's u (0), dx rows (left as they were) and ln_part slot (0).  Every output lies between guards (Out).

A test of this file after which the device reports an error (a fault is sticky for the process) ends the whole pytest session through the
autouse fixture stop_at_a_gpu_fault, later test files included: nothing more is launched on a device that faulted.

Inputs (checked on the CPU in the case builders, which tests/test_head_ref.py also runs without a GPU): every hidden pre-activation z is
farther from 0 than twice the float32 dot-product bound, |z| > 2 (2D + 2) 2^-24 sum_k |w_k v_k| (b1[j] is put into the widest gap of unit j's
pre-activations that leaves a quarter to three quarters of them positive; the seed is stepped, at most 8 times, until the condition and
the value range hold); every p, ips, g lies in (0.02, 0.98).  The clamp cases (b2 = +40, labels 0: p == 1.0f) are held to the float32
restatement, which tests/test_head_ref.py pins to torch's binary_cross_entropy bit for bit.

Which case reaches which form (B, T, NI, D, hid):
  own-sequence head, rows in registers (T <= 64)        own / own_vec at every T <= 64; (3, 64, 2, 128, 32) is the last
  lnmean_rows_own / lnmean_rows_bwd_own (T >= 65)       own / own_vec at (3, 65, 2, 128, 32), (2, 70, 130, 128, 32)
  head_own_rows_body, constant-shape form               own / own_vec at (5, 50, 2, 128, 32), (3, 64, ..), (3, 20, 2, 128, 32) without LayerNorm
  head_own_rows_body, general form                      own / own_vec at every other shape with T <= 64
  staged operands (NI <= 4), head_loss_terms (NI 2)     own / own_vec at NI 1, 2, 3, 4 with T <= 64 (staging lives in head_own_rows_impl only);
                                                        unstaged: (2, 9, 5, 96, 24), NI >= 64, and (3, 65, 2, 128, 32) although its NI is 2
  scorer_bwd_part one-barrier branch                    own_vec at (3, 17, 3, 64, 16) (192 <= 256), (1, 1, 1, 32, 4) and NI 2 at D 128 (256 <= 256);
                                                        the general branch: (3, 20, 4, 128, 64) (512 > 256), the unstaged shapes, every sc_part entry
  item chunks of 64, dW1 accumulated in place           NI 64 / 65 / 130 of the fused heads, amid_scorer_* and the one-head multi entry
  hid: one unit a lane, two, idle lanes                 hid 32 / 64 / 4, 16, 24 (amid_scorer_bwd_f32 also hid 5)
  scorer_multi_fwd_bwd_kernel, one head / three heads   test_scorer_multi_*: NI 2, 64, 65, 130 / NI 1, 2, 16 in both modes, against the same
                                                        float64 objective as amid_dr_loss_f32 (test_dr_loss_against_fp64)
  transpose_extra riders                                n_tr 7 at D 128 (112 tiles over the cap of 96), 1 at D 128, 3 at D 32, 3 on the multi entry
  head.hip's scorer_bwd_kernel, accumulate 0 / 1        test_scorer_bwd_against_fp64
  plain lnmean_* kernels, w0 == NULL                    test_lnmean_against_fp64"""
import functools

import pytest
import torch

from tests import head_ref as R
from tests.test_gpu_intercomp import FLOOR, GUARD, SENT, UNSUPPORTED, L, Out, err, pa, stream  # noqa: F401  (L: the library fixture)
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
ARG = -1                         # AMID_ERR_ARG (include/amid_hip.h)
EPS = R.EPS
F64, F32 = torch.float64, torch.float32
MAX_SEED_STEPS = 8
# (entry point, tensor) -> a factor other than 4 for a tensor MEASURED over 4 e_f32 + 2^-22 although the kernel is right; every other tensor keeps 4.
# All seven are gradients or loss terms of the doubly-robust objectives, where one float32 ulp in the BCE value c = -log p (the device's logf
# against the host's) or in p (expf) is multiplied by the objective: (c^2 - g^2)^2 carries it four times, (p - y) / (p (1 - p)) by 1 / (1 - p).
# tests/test_head_ref.py (test_one_ulp_...) moves c or p by ONE ulp in the float32 restatement and lands on the GPU's figures (dips at 2x130:
# 4.840e-07 both ways), while the unmoved restatement, whose largest element happens to round well, is at a tenth of that.
# Beside each: the case, e_kernel on the MI355X / e_f32, and need = (e_kernel - 2^-22) / e_f32; the factor is the next power of two.  e_f32 of
# these few-element tensors depends on the host the restatement runs on (torch's float32 kernels differ between CPUs): "host A" is the GPU
# machine's, "host B" a second machine, same torch, same inputs.  The last four miss the 4 only with host B's e_f32 (profiles/head_kernels.md).
THREE_HEADS = "amid_scorer_multi_fwd_bwd_f32 (3 heads)"
FACTOR = {
    ("amid_dr_loss_f32", "dips"): 8,     # 2x130 mode 1: 4.840e-07 / 3.883e-08 (both hosts), need 6.3; 3x65 mode 1: 5.574e-07 / host B 6.208e-08, need 5.1
    (THREE_HEADS, "dp"): 16,             # NI 2 D 64 mode 1: 5.157e-07 / host A 2.691e-08, need 10.3; NI 1 D 128 mode 0: 4.846e-07 / A 2.458e-08, B 1.653e-08, need 10.0, 14.9
    (THREE_HEADS, "h0_db2"): 8,          # NI 2 D 64 mode 1: 4.339e-07 / 4.066e-08 (both hosts), need 4.8
    (THREE_HEADS, "dr_loss_part"): 16,   # NI 2 D 64, both modes: 6.085e-07 / host A 1.705e-07 (need 2.2), host B 3.265e-08 (need 11.3)
    (THREE_HEADS, "h1_db1"): 8,          # NI 2 D 64 mode 1: 4.993e-07 / host A 2.243e-07 (need 1.2), host B 4.460e-08 (need 5.8)
    (THREE_HEADS, "h1_db2"): 8,          # NI 2 D 64 mode 1: 5.294e-07 / host A 1.724e-07 (need 1.7), host B 5.335e-08 (need 5.5)
    (THREE_HEADS, "h1_dW1"): 8,          # NI 2 D 64 mode 1: 4.940e-07 / host A 2.618e-07 (need 1.0), host B 6.091e-08 (need 4.2)
}


@pytest.fixture(autouse=True)
def stop_at_a_gpu_fault():
    """A kernel that faulted leaves the device unusable for this process: end the session there instead of launching the remaining cases."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, nothing more is launched: {e}", returncode=3)


def check(entry, tag, got, ref64, ref32, keys=None):
    """{name: tensor} of the kernel, the float64 reference and the float32 restatement: logs both errors, asserts the bar."""
    bad = []
    for k in (keys or got):
        ek, ef = err(got[k], ref64[k]), err(ref32[k], ref64[k])
        f = FACTOR.get((entry, k), 4)
        log(f"head {entry} [{tag}] {k} e_kernel {ek:.3e} e_f32 {ef:.3e}")
        print(f"head {entry} [{tag}] {k} e_kernel {ek:.3e} e_f32 {ef:.3e} bar {f * ef + FLOOR:.3e}")
        if not ek <= f * ef + FLOOR:
            bad.append((k, ek, ef))
    assert not bad, (entry, tag, bad)


def take_rows(o, used, tag):
    """An Out of padded rows [B][P]: the first `used` floats of every row written and finite, the padding and the guards untouched."""
    b = o.buf.cpu()
    n = o.t.numel()
    assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), f"{tag}: a write outside the output"
    t = b[GUARD:GUARD + n].view(o.t.shape)
    assert bool(torch.isfinite(t[:, :used]).all()), f"{tag}: an element was not written (or is not finite)"
    assert bool(torch.isnan(t[:, used:]).all()), f"{tag}: a row's padding was written"
    return t[:, :used].clone()


def untouched(o, fill=None):
    b = o.buf.cpu()
    n = o.t.numel()
    inner = b[GUARD:GUARD + n]
    return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()) and \
        bool(torch.isnan(inner).all() if fill is None else (inner == fill).all())


def split_part(rows, D, hid, pre="sc_"):
    o = hid * 2 * D
    return {pre + "dW1": rows[:, :o], pre + "db1": rows[:, o:o + hid], pre + "dW2": rows[:, o + hid:o + 2 * hid], pre + "db2": rows[:, o + 2 * hid:]}


def split_hidg(rows, NI, hid):
    return dict(hg_da=rows[:, :2 * hid], hg_dc=rows[:, 2 * hid:(2 + NI) * hid], hg_dW2=rows[:, (2 + NI) * hid:-1], hg_db2=rows[:, -1:])


def raises_code(L, code, name, tab):
    from amid_amd._lib import AmidError
    with pytest.raises(AmidError) as e:
        L.call_named(name, tab)
    torch.cuda.synchronize()
    assert e.value.code == code, (name, e.value.code)


# ---------------------------------------------------------------------------- inputs
def draw_scorer(g, D, hid):
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    return dict(w1=2.0 * rn(hid, 2 * D) / (2 * D) ** 0.5, b1=torch.zeros(hid), w2=1.2 * rn(hid) / hid ** 0.5, b2=0.3 * rn(1))


def operands(u, items):
    """[2, B, NI, 2D] in float64: the scorer's input vectors [u_d[b] | item[b, n]]."""
    u, items = u.double(), items.double()
    _, B, D = u.shape
    NI = items.shape[1]
    return torch.cat((u[:, :, None, :].expand(2, B, NI, D), items[None].expand(2, B, NI, D)), dim=-1)


def fit_b1(u, items, W):
    """b1[j] = minus the middle of the widest gap between unit j's sorted sums W1[j] . v that leaves a quarter to three quarters of them positive."""
    s = (operands(u, items) @ W["w1"].double().t()).reshape(-1, W["w1"].shape[0])
    v = s.sort(0).values
    N = v.shape[0]
    gaps, n_on = v[1:] - v[:-1], (N - 1 - torch.arange(N - 1))[:, None]
    ok = (4 * n_on >= N) & (4 * n_on <= 3 * N)
    if bool(ok.any()):
        gaps = torch.where(ok, gaps, torch.zeros_like(gaps))
    i = gaps.argmax(0)
    j = torch.arange(v.shape[1])
    return dict(W, b1=(-(v[i, j] + v[i + 1, j]) / 2).float())


def relu_margin_ok(u, items, W):
    """Every hidden pre-activation, in float64, farther from 0 than twice the float32 error bound of its 2D-term dot product."""
    v, w1 = operands(u, items), W["w1"].double()
    z = v @ w1.t() + W["b1"].double()
    bound = 2 * (v.shape[-1] + 2) * 2.0 ** -24 * (v.abs() @ w1.abs().t())
    return bool((z.abs() > bound).all()) and bool((z > 0).any()) and bool((z < 0).any())


def in_range(*ps):
    return all(bool((p > 0.02).all()) and bool((p < 0.98).all()) for p in ps)


def mixed_domain(B, dom):
    d = (torch.arange(B) + 1) % 2 if dom == "mixed" else torch.full((B,), int(dom), dtype=torch.long)
    assert dom != "mixed" or B == 1 or (bool((d == 0).any()) and bool((d == 1).any()))
    return d.long()


def scorer_refs(u, items, W, labels, domain_id, dtype):
    """Scorer + masked BCE + scorer backward on given user vectors."""
    p, _ = R.scorer(u, items, W, dtype)
    mb = R.masked_bce(p, labels, domain_id, dtype)
    bw = R.scorer_bwd(u, items, W, p, mb["dp"], dtype)
    D, hid, NI = u.shape[-1], W["b1"].numel(), items.shape[1]
    return dict(p=p, loss_part=mb["loss_part"], dp=mb["dp"], du=bw["du"], ditems=bw["ditems"],
                **split_part(R.sc_part_rows(u.to(dtype), items, bw), D, hid), **split_hidg(R.hidg_rows(bw), NI, hid))


def head_refs(c, dtype):
    ln = c["ln"]
    u = R.lnmean(c["x"], ln, dtype)
    r = scorer_refs(u, c["items"], c["W"], c["labels"], c["domain_id"], dtype)
    return dict(r, u=u, **R.lnmean_bwd(c["x"], r["du"], ln, dtype))


@functools.lru_cache(maxsize=None)
def head_case(B, T, NI, D, hid, ln=True, dom="mixed", clamp=False):
    """The inputs of a fused-head case and its float64 / float32 references; deterministic from the arguments."""
    for step in range(MAX_SEED_STEPS + 1):
        g = torch.Generator().manual_seed(100000 * B + 1000 * T + 10 * NI + D + hid + 7919 * step)
        rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        x = rn(2, B, T, D) * (0.5 + torch.rand(2, B, T, 1, generator=g)) + 0.3 * rn(2, B, T, 1)      # per-row scale and offset
        lnp = (0.5 + torch.rand(2, D, generator=g), 0.2 * rn(2, D)) if ln else None                  # per domain
        items = 0.7 * rn(B, NI, D)
        labels = (torch.rand(B, NI, generator=g) < 0.5).float()
        W = fit_b1(R.lnmean(x, lnp, F64), items, draw_scorer(g, D, hid))
        c = dict(shape=(B, T, NI, D, hid), x=x, ln=lnp, items=items, labels=labels, W=W, domain_id=mixed_domain(B, dom), steps=step)
        if clamp:
            c["W"], c["labels"] = dict(W, b2=torch.tensor([40.0])), torch.zeros(B, NI)
            break
        if relu_margin_ok(R.lnmean(x, lnp, F64), items, W) and in_range(R.scorer(R.lnmean(x, lnp, F64), items, W, F64)[0]):
            break
    else:
        raise AssertionError(f"no seed within {MAX_SEED_STEPS} steps meets the ReLU margin and the value range")
    c["ref64"], c["ref32"] = head_refs(c, F64), head_refs(c, F32)
    return c


@functools.lru_cache(maxsize=None)
def scorer_case(B, NI, D, hid, n_heads=1, mode=0, clamp=False):
    """User vectors given: the inputs of the amid_scorer_* entries (n_heads 1) and of the multi entry, with their references.
    clamp: head 0 (predictModule) with b2 = +40 and labels 0 after the conditions were met -- its p == 1.0f."""
    for step in range(MAX_SEED_STEPS + 1):
        g = torch.Generator().manual_seed(100000 * B + 100 * NI + D + hid + 31 * n_heads + 7919 * step)
        rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        u = 0.5 * rn(2, B, D) + 0.3 * rn(2, 1, D)
        items = 0.7 * rn(B, NI, D)
        labels = (torch.rand(B, NI, generator=g) < 0.5).float()
        Ws = [fit_b1(u, items, draw_scorer(g, D, hid)) for _ in range(n_heads)]
        if all(relu_margin_ok(u, items, W) and in_range(R.scorer(u, items, W, F64)[0]) for W in Ws):
            break
    else:
        raise AssertionError(f"no seed within {MAX_SEED_STEPS} steps meets the ReLU margin and the value range")
    domain_id = mixed_domain(B, "mixed")
    ob = (torch.arange(B) % 2 == 0).long() if B > 1 else torch.ones(1, dtype=torch.long)
    if clamp:
        Ws, labels = [dict(Ws[0], b2=torch.tensor([40.0]))] + Ws[1:], torch.zeros(B, NI)
    c = dict(u=u, items=items, labels=labels, Ws=Ws, W=Ws[0], domain_id=domain_id, ob=ob, steps=step)
    if n_heads == 1:
        c["ref64"], c["ref32"] = (scorer_refs(u, items, Ws[0], labels, domain_id, t) for t in (F64, F32))
    else:
        c["ref64"], c["ref32"] = (multi_refs(c, mode, t) for t in (F64, F32))
    return c


DR_W = 0.5


def multi_refs(c, mode, dtype):
    """Three scorers (predictModule, predict_ips, predict_gfunc) on the same (u, items), the objective of `mode` on their outputs, every scorer's
    backward: d u and d items summed over the heads."""
    u, items = c["u"], c["items"]
    ps = [R.scorer(u, items, W, dtype)[0] for W in c["Ws"]]
    dr = R.dr_loss(ps[0], ps[1], ps[2], c["labels"], c["domain_id"], c["ob"], mode, DR_W, dtype)
    dps = [dr["dp"], dr["dips"], dr["dg"]]
    bws = [R.scorer_bwd(u, items, W, p, dp, dtype) for W, p, dp in zip(c["Ws"], ps, dps)]
    D, hid = u.shape[-1], c["W"]["b1"].numel()
    r = dict(p=torch.stack(ps), dp=dr["dp"], dips=dr["dips"], dg=dr["dg"], dr_loss_part=dr["loss_part"], du=sum(b["du"] for b in bws),
             ditems=sum(b["ditems"] for b in bws))
    for h, b in enumerate(bws):
        r.update(split_part(R.sc_part_rows(u.to(dtype), items, b), D, hid, pre=f"h{h}_"))
    return r


# ---------------------------------------------------------------------------- the fused heads
# (B, T, NI, D, hid), LayerNorm, domain ids, transposes riding on the backward entries
HEAD_CASES = [
    ((5, 50, 2, 128, 32), True, "mixed", 7),      # training shape, constant-shape form; 7 matrices at D 128: 112 tiles over the cap of 96 workgroups
    ((3, 64, 2, 128, 32), True, "mixed", 1),      # last T in registers
    ((3, 65, 2, 128, 32), True, "mixed", 0),      # first T off the register form
    ((1, 1, 1, 32, 4), True, "mixed", 3),         # every minimum, B 1
    ((3, 17, 3, 64, 16), True, "mixed", 0),       # staged; one-barrier hidg branch (192 <= 256)
    ((3, 20, 4, 128, 64), True, "mixed", 0),      # staged; 512 > 256: the general branch; two hidden units a lane
    ((2, 9, 5, 96, 24), True, "mixed", 0),        # unstaged; D not a power of two
    ((2, 20, 64, 64, 32), True, "mixed", 0),      # chunk full
    ((2, 20, 65, 64, 32), True, "mixed", 0),      # second chunk of one item
    ((2, 70, 130, 128, 32), True, "mixed", 0),    # three chunks, long T
    ((3, 20, 2, 128, 32), False, "mixed", 0),     # BERT4Rec's plain mean, ln_part NULL
    ((3, 20, 2, 128, 32), True, 0, 0),            # every row of domain 0
    ((3, 17, 3, 64, 16), True, 1, 0),             # every row of domain 1
]
HEAD_IDS = ["-".join(map(str, s)) + ("" if ln else "-noln") + ("" if dom == "mixed" else f"-dom{dom}") for s, ln, dom, _ in HEAD_CASES]
VEC_CASES = [c for c in HEAD_CASES if c[0][2] != 130]            # the hidg form: NI <= 64 (NI 65: refused), so not the three-chunk shape
VEC_IDS = [i for i, c in zip(HEAD_IDS, HEAD_CASES) if c[0][2] != 130]
FWD_KEYS = ("u", "p", "loss_part", "dp")
BWD_KEYS = ("dx", "ditems", "ln_part", "sc_dW1", "sc_db1", "sc_dW2", "sc_db2")
HG_KEYS = ("hg_da", "hg_dc", "hg_dW2", "hg_db2")


class HeadRun:
    """The device inputs, the outputs (each an Out) and the named argument table of one fused-head call."""

    def __init__(self, c, n_tr=0, own=False, labels=True):
        B, T, NI, D, hid = c["shape"]
        self.c, self.own, self.n_tr = c, own, n_tr
        d = self.dev = {k: c[k].cuda() for k in ("x", "items", "labels", "domain_id")}
        d.update({k: v.cuda() for k, v in c["W"].items()})
        if c["ln"] is not None:
            d["lnw"], d["lnb"] = c["ln"][0].cuda(), c["ln"][1].cuda()
        o = self.out = dict(u=Out(2, B, D), p1=Out(B, NI), p2=Out(B, NI), dp1=Out(B, NI), dp2=Out(B, NI), loss_part=Out(B), dx=Out(2, B, T, D),
                            ditems=Out(B, NI, D), ln_part=Out(2 * B, 2, D) if c["ln"] is not None else None,
                            sc_part=Out(B, R.part_floats(D, hid)), hidg=Out(B, R.vec_floats(NI, hid)))
        if own:
            o["dx"].t.fill_(SENT)                                # the other domain's rows must stay as they are
        g = torch.Generator().manual_seed(n_tr)
        self.tr_src = [torch.randn(D, D, generator=g).cuda() for _ in range(n_tr)]
        self.tr_dst = [Out(D, D) for _ in range(n_tr)]
        self.keep = [pa([d["lnw"][0], d["lnw"][1]]), pa([d["lnb"][0], d["lnb"][1]])] if c["ln"] is not None else [None, None]
        self.keep += [pa(self.tr_src), pa(self.tr_dst)] if n_tr else [None, None]
        ptr = lambda k: d[k].data_ptr()      # noqa: E731
        self.tab = dict(x=ptr("x"), ln_w=self.keep[0], ln_b=self.keep[1], items=ptr("items"), w1=ptr("w1"), b1=ptr("b1"), w2=ptr("w2"), b2=ptr("b2"),
                        labels=ptr("labels") if labels else None, domain_id=ptr("domain_id") if labels else None, B=B, T=T, NI=NI, D=D, hid=hid,
                        eps=EPS, tr_src=self.keep[2], tr_dst=self.keep[3], n_tr=n_tr, stream=stream(),
                        **{k: (v.data_ptr() if v is not None else None) for k, v in o.items()})

    def forward(self, labels=True):
        """u, p and, with labels, loss_part and dLoss/dp: the gradient of the head a row does not use exactly 0."""
        o, dom, B = self.out, self.c["domain_id"], self.c["shape"][0]
        got = dict(u=o["u"].get("u"), p=torch.stack((o["p1"].get("p1"), o["p2"].get("p2"))))
        if labels:
            got["loss_part"], got["dp"] = o["loss_part"].get("loss_part"), torch.stack((o["dp1"].get("dp1"), o["dp2"].get("dp2")))
            assert torch.equal(got["dp"][1 - dom, torch.arange(B)], torch.zeros(B, self.c["shape"][2]))
        else:
            assert all(untouched(o[k]) for k in ("dp1", "dp2", "loss_part"))
        return got

    def backward(self, vec=False):
        o = self.out
        B, T, NI, D, hid = self.c["shape"]
        got = dict(dx=o["dx"].get("dx"), ditems=o["ditems"].get("ditems"))
        if o["ln_part"] is not None:
            got["ln_part"] = o["ln_part"].get("ln_part")
        if vec:
            got.update(split_hidg(take_rows(o["hidg"], (3 + NI) * hid + 1, "hidg"), NI, hid))
            assert untouched(o["sc_part"])
        else:
            got.update(split_part(take_rows(o["sc_part"], hid * 2 * D + 2 * hid + 1, "sc_part"), D, hid))
            assert untouched(o["hidg"])
        for i, (src, dst) in enumerate(zip(self.tr_src, self.tr_dst)):
            assert torch.equal(dst.get(f"tr_dst[{i}]"), src.cpu().t()), f"transpose {i}"
        return got

    def nothing_written(self):
        return all(untouched(v, SENT if (k == "dx" and self.own) else None) for k, v in self.out.items() if v is not None) and \
            all(untouched(t) for t in self.tr_dst)


def keys_of(c, keys):
    return [k for k in keys if k != "ln_part" or c["ln"] is not None]


def tag_of(c, n_tr=0):
    return "x".join(map(str, c["shape"])) + ("" if c["ln"] is not None else " noln") + f" dom {c['domain_id'].tolist()} n_tr {n_tr}"


def own_view(c, got, ref):
    """The `own` forms write only the sequence (domain_id[b], b) of a row: u, p and dx of the row's own domain, and everything else, as named tensors."""
    dom, ar = c["domain_id"], torch.arange(c["shape"][0])
    out = {k: v for k, v in ref.items() if k in got}
    for k in ("u", "p", "dx"):
        out[k] = ref[k][dom, ar]
    return out


@pytest.mark.parametrize("with_labels", [False, True], ids=["scores", "loss"])
@pytest.mark.parametrize("shape,ln,dom,n_tr", HEAD_CASES, ids=HEAD_IDS)
def test_head_fwd_against_fp64(L, shape, ln, dom, n_tr, with_labels):
    c = head_case(*shape, ln=ln, dom=dom)
    r = HeadRun(c, labels=with_labels)
    L.call_named("amid_head_fwd_f32", r.tab)
    torch.cuda.synchronize()
    got = r.forward(with_labels)
    check("amid_head_fwd_f32", tag_of(c), got, c["ref64"], c["ref32"])
    assert all(untouched(r.out[k]) for k in ("dx", "ditems", "sc_part", "hidg"))


@pytest.mark.parametrize("shape,ln,dom,n_tr", HEAD_CASES, ids=HEAD_IDS)
def test_head_bwd_on_the_forward_kernels_outputs_against_fp64(L, shape, ln, dom, n_tr):
    c = head_case(*shape, ln=ln, dom=dom)
    r = HeadRun(c, n_tr=n_tr)
    L.call_named("amid_head_fwd_f32", r.tab)
    L.call_named("amid_head_bwd_f32", r.tab)
    torch.cuda.synchronize()
    r.forward()                                                  # the backward's inputs are inputs: still written, still between their guards
    check("amid_head_bwd_f32", tag_of(c, n_tr), r.backward(), c["ref64"], c["ref32"], keys_of(c, BWD_KEYS))


@pytest.mark.parametrize("shape,ln,dom,n_tr", HEAD_CASES, ids=HEAD_IDS)
def test_head_fwd_bwd_against_fp64(L, shape, ln, dom, n_tr):
    c = head_case(*shape, ln=ln, dom=dom)
    r = HeadRun(c, n_tr=n_tr)
    L.call_named("amid_head_fwd_bwd_f32", r.tab)
    torch.cuda.synchronize()
    got = {**r.forward(), **r.backward()}
    check("amid_head_fwd_bwd_f32", tag_of(c, n_tr), got, c["ref64"], c["ref32"], keys_of(c, FWD_KEYS + BWD_KEYS))


def check_own(L, entry, c, n_tr, vec):
    B, T, NI, D, hid = c["shape"]
    r = HeadRun(c, n_tr=n_tr, own=True)
    L.call_named(entry, r.tab)
    torch.cuda.synchronize()
    full = {**r.forward(), **r.backward(vec)}
    dom, ar = c["domain_id"], torch.arange(B)
    assert torch.equal(full["u"][1 - dom, ar], torch.zeros(B, D)), "u of the other domain"
    assert torch.equal(full["dx"][1 - dom, ar], torch.full((B, T, D), SENT)), "dx rows of the other domain's sequences"
    if c["ln"] is not None:
        assert torch.equal(full["ln_part"].view(2, B, 2, D)[1 - dom, ar], torch.zeros(B, 2, D)), "ln_part slot of the other domain"
    got = dict(full)
    for k in ("u", "p", "dx"):
        got[k] = full[k][dom, ar]
    keys = keys_of(c, FWD_KEYS + (("dx", "ditems", "ln_part") + HG_KEYS if vec else BWD_KEYS))
    check(entry, tag_of(c, n_tr), got, own_view(c, got, c["ref64"]), own_view(c, got, c["ref32"]), keys)


@pytest.mark.parametrize("shape,ln,dom,n_tr", HEAD_CASES, ids=HEAD_IDS)
def test_head_fwd_bwd_own_against_fp64(L, shape, ln, dom, n_tr):
    check_own(L, "amid_head_fwd_bwd_own_f32", head_case(*shape, ln=ln, dom=dom), n_tr, vec=False)


@pytest.mark.parametrize("shape,ln,dom,n_tr", VEC_CASES, ids=VEC_IDS)
def test_head_fwd_bwd_own_vec_against_fp64(L, shape, ln, dom, n_tr):
    c = head_case(*shape, ln=ln, dom=dom)
    if shape[2] > 64:                                            # hidg holds one chunk's dc: more items are an argument error, and nothing is written
        r = HeadRun(c, n_tr=n_tr, own=True)
        raises_code(L, ARG, "amid_head_fwd_bwd_own_vec_f32", r.tab)
        assert r.nothing_written()
        return
    check_own(L, "amid_head_fwd_bwd_own_vec_f32", c, n_tr, vec=True)


@pytest.mark.parametrize("entry", ["amid_head_fwd_bwd_f32", "amid_head_fwd_bwd_own_vec_f32"])
def test_head_where_both_clamps_act(L, entry):
    """b2 = +40, labels 0: p == 1.0f, log(1 - p) clamped at -100, p (1 - p) at 1e-12 -- against the float32 restatement (tests/test_head_ref.py
    holds it to torch's binary_cross_entropy bit for bit), its own distance to float64 the yardstick."""
    c = head_case(3, 17, 3, 64, 16, clamp=True)
    own = entry != "amid_head_fwd_bwd_f32"
    r = HeadRun(c, own=own)
    L.call_named(entry, r.tab)
    torch.cuda.synchronize()
    got = r.forward()
    r.backward(vec=own)                                          # every gradient written, finite, inside its guards
    dom, ar = c["domain_id"], torch.arange(3)
    assert torch.equal(got["p"][dom, ar], torch.ones(3, 3))
    r32 = {k: c["ref32"][k].double() for k in ("loss_part", "dp")}
    assert all(bool(torch.isfinite(got[k]).all()) for k in r32) and float(got["dp"].abs().max()) > 1e9
    check(entry + " (clamps)", tag_of(c), got, r32, c["ref64"], ("loss_part", "dp"))


# ---------------------------------------------------------------------------- plain lnmean, LayerNorm rows, vector sum
@functools.lru_cache(maxsize=None)
def lnmean_case(B, T, D, ln):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + D)
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    x = rn(2, B, T, D) * (0.5 + torch.rand(2, B, T, 1, generator=g)) + 0.3 * rn(2, B, T, 1)
    lnp = (0.5 + torch.rand(2, D, generator=g), 0.2 * rn(2, D)) if ln else None
    du = rn(2, B, D)
    refs = [dict(u=R.lnmean(x, lnp, t), **R.lnmean_bwd(x, du, lnp, t)) for t in (F64, F32)]
    return x, lnp, du, refs[0], refs[1]


LNMEAN_SHAPES = [(1, 1, 4), (3, 7, 20), (2, 64, 64), (2, 65, 128), (2, 150, 128), (2, 9, 256)]


@pytest.mark.parametrize("ln", [True, False], ids=["ln", "mean"])
@pytest.mark.parametrize("B,T,D", LNMEAN_SHAPES)
def test_lnmean_against_fp64(L, B, T, D, ln):
    x, lnp, du, ref64, ref32 = lnmean_case(B, T, D, ln)
    xd, dud = x.cuda(), du.cuda()
    w, b = (lnp[0].cuda(), lnp[1].cuda()) if ln else (None, None)
    wp = lambda t, g: t[g].data_ptr() if ln else None      # noqa: E731
    u, dx, part = Out(2, B, D), Out(2, B, T, D), Out(2 * B, 2, D) if ln else None
    L.call_named("amid_lnmean_fwd_f32", x=xd.data_ptr(), w0=wp(w, 0), b0=wp(b, 0), w1=wp(w, 1), b1=wp(b, 1), B=B, T=T, D=D, eps=EPS, u=u.data_ptr(),
                 stream=stream())
    L.call_named("amid_lnmean_bwd_f32", x=xd.data_ptr(), du=dud.data_ptr(), w0=wp(w, 0), w1=wp(w, 1), B=B, T=T, D=D, eps=EPS, dx=dx.data_ptr(),
                 part=part.data_ptr() if ln else None, stream=stream())
    torch.cuda.synchronize()
    check("amid_lnmean_fwd_f32", f"{B}x{T}x{D} ln {ln}", dict(u=u.get("u")), ref64, ref32)
    got = dict(dx=dx.get("dx"))
    if ln:
        got["ln_part"] = part.get("part")
    check("amid_lnmean_bwd_f32", f"{B}x{T}x{D} ln {ln}", got, ref64, ref32)


@functools.lru_cache(maxsize=None)
def rows_case(rows, D):
    g = torch.Generator().manual_seed(rows + D)
    x = torch.randn(rows, D, generator=g) * (0.5 + torch.rand(rows, 1, generator=g)) + 0.3 * torch.randn(rows, 1, generator=g)
    w, b = 0.5 + torch.rand(D, generator=g), 0.2 * torch.randn(D, generator=g)
    return x, w, b, R.layernorm_rows(x, w, b, F64), R.layernorm_rows(x, w, b, F32)


@pytest.mark.parametrize("rows,D", [(1, 4), (7, 32), (9, 132), (33000, 32)])      # 33 000 rows: 4 125 groups of 8, past the 4 096 workgroups launched
def test_layernorm_rows_against_fp64(L, rows, D):
    x, w, b, ref64, ref32 = rows_case(rows, D)
    xd, wd, bd, y = x.cuda(), w.cuda(), b.cuda(), Out(rows, D)
    L.call_named("amid_layernorm_rows_f32", x=xd.data_ptr(), w=wd.data_ptr(), b=bd.data_ptr(), rows=rows, D=D, eps=EPS, y=y.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    check("amid_layernorm_rows_f32", f"{rows}x{D}", dict(y=y.get("y")), dict(y=ref64), dict(y=ref32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_sum_vector_against_fp64(L, n):
    v = 0.1 + torch.rand(n, generator=torch.Generator().manual_seed(n))
    vd, out = v.cuda(), Out(1)
    L.call_named("amid_sum_vector_f32", v=vd.data_ptr(), n=n, out=out.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    check("amid_sum_vector_f32", f"n {n}", dict(sum=out.get("sum")), dict(sum=v.double().sum().reshape(1)), dict(sum=v.sum().reshape(1)))


# ---------------------------------------------------------------------------- the scorer alone
SCORER_SHAPES = [(1, 1, 32, 4), (3, 2, 128, 32), (2, 64, 64, 64), (2, 65, 64, 32), (2, 130, 128, 24)]      # (B, NI, D, hid)


def scorer_table(c, B, NI, D, hid, W=None):
    d = {k: c[k].cuda() for k in ("u", "items", "labels", "domain_id", "ob")}
    d.update({k: v.cuda() for k, v in (W or c["W"]).items()})
    tab = dict({k: d[k].data_ptr() for k in ("u", "items", "w1", "b1", "w2", "b2", "labels", "domain_id")}, B=B, NI=NI, D=D, hid=hid, stream=stream())
    return d, tab


@pytest.mark.parametrize("with_labels", [False, True], ids=["scores", "loss"])
@pytest.mark.parametrize("B,NI,D,hid", SCORER_SHAPES)
def test_scorer_fwd_against_fp64(L, B, NI, D, hid, with_labels):
    c = scorer_case(B, NI, D, hid)
    d, tab = scorer_table(c, B, NI, D, hid)
    o = dict(p1=Out(B, NI), p2=Out(B, NI), dp1=Out(B, NI), dp2=Out(B, NI), loss_part=Out(B))
    if not with_labels:
        tab.update(labels=None, domain_id=None)
    L.call_named("amid_scorer_fwd_f32", tab, **{k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    got = dict(p=torch.stack((o["p1"].get("p1"), o["p2"].get("p2"))))
    if with_labels:
        got["loss_part"], got["dp"] = o["loss_part"].get("loss_part"), torch.stack((o["dp1"].get("dp1"), o["dp2"].get("dp2")))
        assert torch.equal(got["dp"][1 - c["domain_id"], torch.arange(B)], torch.zeros(B, NI))
    else:
        assert all(untouched(o[k]) for k in ("dp1", "dp2", "loss_part"))
    check("amid_scorer_fwd_f32", f"{B}x{NI}x{D}x{hid}", got, c["ref64"], c["ref32"])


@pytest.mark.parametrize("B,NI,D,hid", SCORER_SHAPES + [(2, 3, 20, 5)])      # D 20, hid 5: neither a multiple of 4 -- the entry's argument check takes them
def test_scorer_bwd_against_fp64(L, B, NI, D, hid):
    """head.hip's own scorer backward on given p and dLoss/dp (the float64 reference's, rounded to float32: the same inputs for the kernel and
    both restatements), written (accumulate 0), then added (accumulate 1) onto known non-zero d u / d items."""
    c = scorer_case(B, NI, D, hid)
    d, tab = scorer_table(c, B, NI, D, hid)
    p_in, dp_in = c["ref64"]["p"].float(), c["ref64"]["dp"].float()
    pd, dpd = p_in.cuda(), dp_in.cuda()
    g = torch.Generator().manual_seed(B + NI)
    base = dict(du=torch.randn(2, B, D, generator=g), ditems=torch.randn(B, NI, D, generator=g))
    refs = []
    for t in (F64, F32):
        bw = R.scorer_bwd(c["u"], c["items"], c["W"], p_in, dp_in, t)
        refs.append(dict(du=bw["du"], ditems=bw["ditems"], **split_part(R.sc_part_rows(c["u"].to(t), c["items"], bw), D, hid)))
    for acc in (0, 1):
        o = dict(du=Out(2, B, D), ditems=Out(B, NI, D), part=Out(B, R.part_floats(D, hid)))
        if acc:
            o["du"].t.copy_(base["du"]); o["ditems"].t.copy_(base["ditems"])
        L.call_named("amid_scorer_bwd_f32", {k: v for k, v in tab.items() if k not in ("labels", "domain_id")}, p1=pd[0].data_ptr(), p2=pd[1].data_ptr(),
                     dp1=dpd[0].data_ptr(), dp2=dpd[1].data_ptr(), accumulate=acc, **{k: v.data_ptr() for k, v in o.items()})
        torch.cuda.synchronize()
        got = dict(du=o["du"].get("du"), ditems=o["ditems"].get("ditems"), **split_part(take_rows(o["part"], hid * 2 * D + 2 * hid + 1, "part"), D, hid))
        r64, r32 = (dict(r, **{k: (base[k].to(r[k].dtype) + r[k]) for k in base}) if acc else r for r in refs)
        check("amid_scorer_bwd_f32", f"{B}x{NI}x{D}x{hid} accumulate {acc}", got, r64, r32)


# ---------------------------------------------------------------------------- doubly-robust objectives
@functools.lru_cache(maxsize=None)
def dr_case(B, NI, mode, clamp=False):
    g = torch.Generator().manual_seed(100 * B + NI)
    leaf = lambda: 0.05 + 0.9 * torch.rand(2, B, NI, generator=g)      # noqa: E731
    p, ips, gf = leaf(), leaf(), leaf()
    labels = (torch.rand(B, NI, generator=g) < 0.5).float()
    if clamp:
        p, labels = torch.ones(2, B, NI), torch.zeros(B, NI)
    domain_id = mixed_domain(B, "mixed")
    ob = (torch.arange(B) % 2 == 0).long() if B > 1 else torch.ones(1, dtype=torch.long)
    assert clamp or in_range(p, ips, gf)
    assert B == 1 or (bool((ob == 0).any()) and bool((ob == 1).any()))
    refs = [R.dr_loss(p, ips, gf, labels, domain_id, ob, mode, DR_W, t) for t in (F64, F32)]
    return dict(p=p, ips=ips, g=gf, labels=labels, domain_id=domain_id, ob=ob, ref64=refs[0], ref32=refs[1])


def run_dr_loss(L, c, B, NI, mode):
    d = {k: c[k].cuda() for k in ("p", "ips", "g", "labels", "domain_id", "ob")}
    o = {k: [Out(B, NI), Out(B, NI)] for k in ("dp", "dips", "dg")}
    lp = Out(B, 3)
    L.call_named("amid_dr_loss_f32", p=pa(d["p"]), ips=pa(d["ips"]), g=pa(d["g"]), labels=d["labels"].data_ptr(), domain_id=d["domain_id"].data_ptr(),
                 ob_label=d["ob"].data_ptr(), mode=mode, dr_e_w=DR_W, B=B, NI=NI, dp=pa(o["dp"]), dips=pa(o["dips"]), dg=pa(o["dg"]),
                 loss_part=lp.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    got = {k: torch.stack([t.get(f"{k}[{i}]") for i, t in enumerate(v)]) for k, v in o.items()}
    for k in o:
        assert torch.equal(got[k][1 - c["domain_id"], torch.arange(B)], torch.zeros(B, NI)), f"{k} of the head a row does not use"
    got["loss_part"] = lp.get("loss_part")
    return got


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,NI", [(1, 1), (4, 16), (3, 64), (3, 65), (2, 130)])
def test_dr_loss_against_fp64(L, B, NI, mode):
    c = dr_case(B, NI, mode)
    check("amid_dr_loss_f32", f"{B}x{NI} mode {mode}", run_dr_loss(L, c, B, NI, mode), c["ref64"], c["ref32"])


@pytest.mark.parametrize("mode", [0, 1])
def test_dr_loss_where_both_clamps_act(L, mode):
    """p == 1.0f, labels 0: the BCE is 100 and its derivative 1e12 -- against the float32 restatement, every gradient finite."""
    B, NI = 4, 16
    c = dr_case(B, NI, mode, clamp=True)
    got = run_dr_loss(L, c, B, NI, mode)
    assert float(got["dp"].abs().max()) > 1e9
    check("amid_dr_loss_f32 (clamps)", f"{B}x{NI} mode {mode}", got, {k: v.double() for k, v in c["ref32"].items()}, c["ref64"], ("loss_part", "dp"))


# ---------------------------------------------------------------------------- up to three scorers in one launch
MULTI_FORMS = [(1, 0, NI) for NI in (2, 64, 65, 130)] + [(3, mode, NI) for mode in (0, 1) for NI in (1, 2, 16)]      # (n_heads, mode, NI)


def multi_call(L, c, n_heads, mode, B, NI, D, hid, n_tr):
    d = {k: c[k].cuda() for k in ("u", "items", "labels", "domain_id", "ob")}
    Wd = [{k: v.cuda() for k, v in W.items()} for W in c["Ws"]]
    heads = lambda shape: [Out(*shape) for _ in range(n_heads)]      # noqa: E731
    o = dict(p1=heads((B, NI)), p2=heads((B, NI)), dp1=heads((B, NI)), dp2=heads((B, NI)), sc_part=heads((B, R.part_floats(D, hid))))
    one = dict(loss_part=Out(B), dr_loss_part=Out(B, 3), du=Out(2, B, D), ditems=Out(B, NI, D))
    g = torch.Generator().manual_seed(n_tr)
    tr_src, tr_dst = [torch.randn(D, D, generator=g).cuda() for _ in range(n_tr)], [Out(D, D) for _ in range(n_tr)]
    tab = dict({k: d[k].data_ptr() for k in ("u", "items", "labels", "domain_id")}, ob_label=d["ob"].data_ptr(),
               **{k: pa([W[k] for W in Wd]) for k in ("w1", "b1", "w2", "b2")}, n_heads=n_heads, mode=mode, dr_e_w=DR_W, B=B, NI=NI, D=D, hid=hid,
               **{k: pa(v) for k, v in o.items()}, **{k: v.data_ptr() for k, v in one.items()},
               tr_src=pa(tr_src) if n_tr else None, tr_dst=pa(tr_dst) if n_tr else None, n_tr=n_tr, stream=stream())
    return (d, Wd, tr_src), o, one, tr_dst, tab


@pytest.mark.parametrize("n_tr", [0, 3])
@pytest.mark.parametrize("D,hid", [(128, 32), (64, 64)])
@pytest.mark.parametrize("n_heads,mode,NI", MULTI_FORMS)
def test_scorer_multi_against_fp64(L, n_heads, mode, NI, D, hid, n_tr):
    """One head: the masked BCE, items in chunks of 64.  Three heads: the doubly-robust objective on the three outputs -- the kernel's own copy of
    amid_dr_loss_f32's arithmetic, held to the same float64 restatement --, d u and d items summed over the heads through LDS."""
    c = scorer_case(3, NI, D, hid, n_heads, mode)
    check(f"amid_scorer_multi_fwd_bwd_f32 ({n_heads} head{'s' if n_heads > 1 else ''})", f"NI {NI} D {D} hid {hid} mode {mode} n_tr {n_tr}",
          run_multi(L, c, n_heads, mode, 3, NI, D, hid, n_tr), c["ref64"], c["ref32"])


def run_multi(L, c, n_heads, mode, B, NI, D, hid, n_tr):
    """The multi entry's outputs by name, after the exact checks: guards, padding, transposes, zeros on the head a row does not use."""
    keep, o, one, tr_dst, tab = multi_call(L, c, n_heads, mode, B, NI, D, hid, n_tr)
    L.call_named("amid_scorer_multi_fwd_bwd_f32", tab)
    torch.cuda.synchronize()
    dom, ar = c["domain_id"], torch.arange(B)
    p = torch.stack([torch.stack((o["p1"][h].get("p1"), o["p2"][h].get("p2"))) for h in range(n_heads)])
    dp = torch.stack([torch.stack((o["dp1"][h].get("dp1"), o["dp2"][h].get("dp2"))) for h in range(n_heads)])
    assert torch.equal(dp[:, 1 - dom, ar], torch.zeros(n_heads, B, NI)), "gradients of the head a row does not use"
    got = dict(du=one["du"].get("du"), ditems=one["ditems"].get("ditems"))
    for h in range(n_heads):
        got.update(split_part(take_rows(o["sc_part"][h], hid * 2 * D + 2 * hid + 1, f"sc_part[{h}]"), D, hid, pre=f"h{h}_" if n_heads == 3 else "sc_"))
    if n_heads == 1:
        got.update(p=p[0], dp=dp[0], loss_part=one["loss_part"].get("loss_part"))
        assert untouched(one["dr_loss_part"])
    else:
        got.update(p=p, dp=dp[0], dips=dp[1], dg=dp[2], dr_loss_part=one["dr_loss_part"].get("dr_loss_part"))
        assert untouched(one["loss_part"])
    for i, (src, dst) in enumerate(zip(keep[2], tr_dst)):
        assert torch.equal(dst.get(f"tr_dst[{i}]"), src.cpu().t()), f"transpose {i}"
    return got


@pytest.mark.parametrize("mode", [0, 1])
def test_scorer_multi_where_both_clamps_act(L, mode):
    """The three-head kernel's own copy of the objective where p == 1.0f (head 0 with b2 = +40, labels 0): its loss terms and dLoss/dp against the
    float32 restatement, everything else written and finite."""
    B, NI, D, hid = 3, 2, 128, 32
    c = scorer_case(B, NI, D, hid, 3, mode, clamp=True)
    got = run_multi(L, c, 3, mode, B, NI, D, hid, 0)
    assert torch.equal(got["p"][0][c["domain_id"], torch.arange(B)], torch.ones(B, NI)) and float(got["dp"].abs().max()) > 1e9
    check("amid_scorer_multi_fwd_bwd_f32 (3 heads, clamps)", f"NI {NI} D {D} hid {hid} mode {mode}", got, {k: v.double() for k, v in c["ref32"].items()},
          c["ref64"], ("dr_loss_part", "dp"))


def test_scorer_multi_refuses_three_heads_beyond_16_items(L):
    B, NI, D, hid = 3, 17, 128, 32
    g = torch.Generator().manual_seed(17)
    W = draw_scorer(g, D, hid)
    c = dict(u=torch.randn(2, B, D, generator=g), items=torch.randn(B, NI, D, generator=g), labels=torch.zeros(B, NI), Ws=[W, W, W],
             domain_id=mixed_domain(B, "mixed"), ob=torch.ones(B, dtype=torch.long))
    keep, o, one, tr_dst, tab = multi_call(L, c, 3, 0, B, NI, D, hid, 0)
    raises_code(L, UNSUPPORTED, "amid_scorer_multi_fwd_bwd_f32", tab)
    assert all(untouched(t) for v in o.values() for t in v) and all(untouched(t) for t in one.values())
