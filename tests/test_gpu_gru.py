"""GRU4Rec's encoder entry points (csrc/gru.hip) through the C ABI against the float64 helper tests/gru_ref.py (pinned to the reference by
tests/test_gru_ref_golden.py), at the tile edges of 16 sequences and the first steps of the recurrence, with and without a live list.

Bar, per output tensor (tests/test_gpu_intercomp.py's): e = max|x - ref64| / max|ref64|; e_kernel <= 4 e_f32 + 2^-22, with e_f32 the same
figure for torch's float32 CPU GRU (nn.GRU and its autograd; the hand-stepped float32 layer for the tensors nn.GRU does not expose) on the
same inputs.  Both figures of every case and tensor go to the parity log; the worst ratio per tensor: profiles/gru4rec.md."""
import ctypes
import functools

import pytest
import torch

from tests import gru_ref
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
D = 128
FLOOR = 2.0 ** -22
SENT = -12345.625                # guard value: exact in float32, far from every output
GUARD = 512
BS, TS = (1, 15, 16, 17, 33), (1, 2, 3, 20, 50)
CASES = ("full", "all0", "all1", "mixed")
FWD = ("gi", "h", "gates", "ghn", "hprev")


@pytest.fixture(scope="module")
def L():
    from amid_amd._lib import lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def pa(tensors):
    from amid_amd._lib import ptr_array
    return ptr_array([t.data_ptr() for t in tensors])


class Out:
    """An output of [2, B, T, C] floats inside a larger allocation: NaN inside, SENT in the guards before and after."""

    def __init__(self, B, T, C):
        n = 2 * B * T * C
        self.n, self.shape = n, (2, B, T, C)
        self.buf = torch.full((GUARD + n + GUARD,), SENT, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*self.shape)
        self.t.fill_(float("nan"))

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self, tag, written):
        """The output on the CPU after checking the guards, that every sequence of `written` [2, B] (bool) was written in full and that
        every other sequence kept its NaNs."""
        b = self.buf.cpu()
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.n:] == SENT).all()), f"{tag}: a write outside the output"
        o = b[GUARD:GUARD + self.n].view(*self.shape).clone()
        assert bool(torch.isfinite(o[written]).all()), f"{tag}: an element was not written (or is not finite)"
        assert bool(torch.isnan(o[~written]).all()), f"{tag}: a row of a sequence outside the list was written"
        return o


def domains(B, case):
    """The batch's domain ids, or None (no live list).  mixed: n0 is no multiple of 16 and a tile boundary falls next to it (B 33: n0 17)."""
    if case == "full":
        return None
    if case == "all0":
        return torch.zeros(B, dtype=torch.long)
    if case == "all1":
        return torch.ones(B, dtype=torch.long)
    n0 = (B + 1) // 2
    d = torch.ones(B, dtype=torch.long)
    d[torch.randperm(B, generator=torch.Generator().manual_seed(B))[:n0]] = 0
    return d


@functools.lru_cache(maxsize=None)
def inputs(B, T):
    g = torch.Generator().manual_seed(100 * B + T)
    k = 1.0 / D ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k      # noqa: E731  (nn.GRU's initialisation)
    return dict(x=torch.randn(2, B, T, D, generator=g), w_ih=u(2, 3 * D, D), w_hh=u(2, 3 * D, D), b_ih=u(2, 3 * D), b_hh=u(2, 3 * D),
                dh=torch.randn(2, B, T, D, generator=g))


def reference(B, T, mask, dtype, hand):
    """Every tensor of the forward and, under the cotangent dh * mask on h, of the backward.  hand=False: h and the gradients of x and of the
    parameters from nn.GRU and its autograd; True: from the hand-stepped layer (which also gives gi, the gates, ghn, hprev, dgi, dgh)."""
    I = inputs(B, T)
    out = {k: [] for k in FWD + ("dgi", "dgh", "dx", "dw_ih", "dw_hh", "db_ih", "db_hh")}
    for g in (0, 1):
        x = I["x"][g].to(dtype).requires_grad_(True)
        w = [I[n][g].to(dtype).requires_grad_(True) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]
        cot = I["dh"][g].to(dtype) * mask[g].to(dtype)[:, None, None]
        if hand:
            taps = gru_ref.gru_taps(x, *w)
            gs = torch.autograd.grad((taps["h"] * cot).sum(), [x, *w, taps["gi"], *taps["gh_steps"]])
            for k in FWD:
                out[k].append(taps[k].detach())
            out["dgi"].append(gs[5])
            out["dgh"].append(torch.stack(gs[6:], 1))
        else:
            h = gru_ref.gru_layer(x, *w)
            gs = torch.autograd.grad((h * cot).sum(), [x, *w])
            out["h"].append(h.detach())
        for k, v in zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh"), gs[:5]):
            out[k].append(v)
    return {k: torch.stack(v) for k, v in out.items() if v}


@functools.lru_cache(maxsize=None)
def references(B, T, case):
    dom = domains(B, case)
    mask = torch.ones(2, B, dtype=torch.bool) if dom is None else torch.stack((dom == 0, dom == 1))
    r64 = reference(B, T, mask, torch.float64, True)
    assert float((r64["h"] - reference(B, T, mask, torch.float64, False)["h"]).abs().max()) < 1e-12      # the hand-stepped layer IS nn.GRU
    r32 = reference(B, T, mask, torch.float32, True)
    r32.update(reference(B, T, mask, torch.float32, False))
    return dom, mask, r64, r32


def err(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def mutants_move_the_outputs(B, T):
    """On the float64 reference: exchanging the r and z blocks of W_hh, and moving b_hn outside r * ( ), each move h by more than 100 bars
    (a kernel with either mistake cannot pass).  At T = 1 h0 = 0 hides W_hh altogether: that mutant is not asserted there."""
    I = inputs(B, T)
    _, _, r64, r32 = references(B, T, "full")
    bar = 4 * err(r32["h"], r64["h"]) + FLOOR
    for mutant in ("swap_rz", "bhn_outside"):
        if T == 1 and mutant == "swap_rz":
            continue
        h = torch.stack([gru_ref.gru_taps(I["x"][g].double(), *[I[n][g].double() for n in ("w_ih", "w_hh", "b_ih", "b_hh")], mutant=mutant)["h"]
                         for g in (0, 1)])
        moved = err(h, r64["h"])
        print(f"gru B {B} T {T} mutant {mutant}: moves h by {moved:.3e}, bar {bar:.3e}")
        assert moved > 100 * bar, (mutant, moved, bar)
    return True


def run(L, B, T, dom, dh, zero_dead=1):
    """Every entry point once: the projection, both forward forms, the backward, the data gradient, the weight gradients (the tiles of
    amid_bert_wgrad_mode_f32 the engine launches, their split partials summed).  Returns the outputs and the inference form's h."""
    I = inputs(B, T)
    dev = {k: v.cuda() for k, v in I.items()}
    fam = lambda n: pa([dev[n][0], dev[n][1]])      # noqa: E731
    live = None
    domd = None
    if dom is not None:
        domd = dom.cuda()
        live = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
        L.call("amid_live_list_i32", domd.data_ptr(), B, live.data_ptr(), stream())
    lp = None if live is None else live.data_ptr()
    assert L.value("amid_gru_supported", B, T, D) == 1
    O = {k: Out(B, T, 3 * D if k in ("gi", "gates", "dgi", "dgh") else D) for k in FWD + ("dgi", "dgh", "dx", "h_infer")}
    dhd = dh.cuda().contiguous()
    L.call("amid_gru_proj_fwd_f32", dev["x"].data_ptr(), fam("w_ih"), fam("b_ih"), B, T, D, lp, O["gi"].data_ptr(), stream())
    L.call("amid_gru_rec_fwd_f32", O["gi"].data_ptr(), fam("w_hh"), fam("b_hh"), B, T, D, lp, O["h"].data_ptr(), O["gates"].data_ptr(),
           O["ghn"].data_ptr(), O["hprev"].data_ptr(), stream())
    L.call("amid_gru_rec_fwd_infer_f32", O["gi"].data_ptr(), fam("w_hh"), fam("b_hh"), B, T, D, lp, O["h_infer"].data_ptr(), stream())
    L.call("amid_gru_rec_bwd_f32", dhd.data_ptr(), O["gates"].data_ptr(), O["ghn"].data_ptr(), O["hprev"].data_ptr(), fam("w_hh"), B, T, D, lp,
           zero_dead, O["dgi"].data_ptr(), O["dgh"].data_ptr(), stream())
    L.call("amid_gru_dx_f32", O["dgi"].data_ptr(), fam("w_ih"), B, T, D, lp, zero_dead, O["dx"].data_ptr(), stream())
    got = {}
    if zero_dead or dom is None:
        S, M, n_ent = 2, B * T, 6
        w_part = torch.full((2, n_ent, S, D * D), float("nan"), device="cuda")
        b_part = torch.full((2, n_ent, S, D), float("nan"), device="cuda")
        dy = [O["dgi"].data_ptr() + 4 * c * D for c in range(3)] + [O["dgh"].data_ptr() + 4 * c * D for c in range(3)]
        xx = [dev["x"].data_ptr()] * 3 + [O["hprev"].data_ptr()] * 3
        ia = lambda v: (ctypes.c_int * n_ent)(*v)      # noqa: E731
        from amid_amd._lib import ptr_array
        L.call("amid_bert_wgrad_mode_f32", ptr_array(dy), ptr_array(xx), ia([3 * D] * 6), ia([D] * 6), ia([D] * 6), ia(range(6)), ia([0] * 6),
               n_ent, M, S, w_part.data_ptr(), b_part.data_ptr(), None if domd is None else domd.data_ptr(), B, T, 0, stream())
        torch.cuda.synchronize()
        w, b = w_part.sum(2).cpu().view(2, 2, 3 * D, D), b_part.sum(2).cpu().view(2, 2, 3 * D)
        got.update(dw_ih=w[:, 0], dw_hh=w[:, 1], db_ih=b[:, 0], db_hh=b[:, 1])
    torch.cuda.synchronize()
    return O, got


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("B", BS)
def test_gru_entries_against_fp64(L, B, T, case):
    assert mutants_move_the_outputs(B, T)
    dom, mask, r64, r32 = references(B, T, case)
    everything = torch.ones(2, B, dtype=torch.bool)
    dh = inputs(B, T)["dh"] * mask[:, :, None, None]
    O, got = run(L, B, T, dom, dh)
    tag = f"gru B {B} T {T} {case}"
    for k in FWD:
        got[k] = O[k].get(f"{tag} {k}", mask)
    h_infer = O["h_infer"].get(f"{tag} h (inference form)", mask)
    for k in ("dgi", "dgh", "dx"):                     # zero_dead: the other sequences' rows are exact zeros
        got[k] = O[k].get(f"{tag} {k}", everything)
        assert bool((got[k][~mask] == 0).all()), f"{tag} {k}: a row outside the list is not zero"
    assert torch.equal(h_infer[mask], got["h"][mask]), f"{tag}: the inference form's h differs from the saving form's"
    assert bool((got["hprev"][mask][:, 0] == 0).all()) and torch.equal(got["hprev"][mask][:, 1:], got["h"][mask][:, :-1])
    if dom is not None:
        # the same sequences of a run without a list (same cotangent): bit for bit; without zero_dead the other rows are not touched
        Of, _ = run(L, B, T, None, dh)
        for k in FWD + ("dgi", "dgh", "dx"):
            assert torch.equal(Of[k].get(f"{tag} {k} (no list)", everything)[mask], got[k][mask]), f"{tag} {k}: differs from the run without a list"
        On, _ = run(L, B, T, dom, dh, zero_dead=0)
        for k in ("dgi", "dgh", "dx"):
            assert torch.equal(On[k].get(f"{tag} {k} (zero_dead 0)", mask)[mask], got[k][mask])
    bad = []
    for k, r in r64.items():
        # forward tensors: the listed sequences (nothing else exists); gradients: whole tensors (zeros outside the list on both sides)
        x, rr, r3 = (got[k][mask], r[mask], r32[k][mask]) if k in FWD else (got[k], r, r32[k])
        if rr.numel() == 0 or float(rr.abs().max()) == 0.0:      # (hprev at T = 1; a domain without a live sequence)
            assert float(x.abs().max()) == 0.0 if x.numel() else True, f"{tag} {k}"
            continue
        ek, ef = err(x, rr), err(r3, rr)
        log(f"{tag} {k:6s} e_kernel {ek:.3e} e_f32 {ef:.3e}")
        print(f"{tag} {k:6s} e_kernel {ek:.3e} e_f32 {ef:.3e} bar {4 * ef + FLOOR:.3e} ratio {ek / max(ef, 1e-30):.2f}")
        if not ek <= 4 * ef + FLOOR:
            bad.append((k, ek, ef))
    assert not bad, bad
