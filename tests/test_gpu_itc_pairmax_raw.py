"""The pair-max on raw rows (csrc/intercomp.hip: amid_itc_pairmax_raw_f32 -- InterComp's score and the plain means for a backbone without
a last LayerNorm, GRU4Rec) through the C ABI against float64, in both of its forms: whole-row (2 T (D + 4) floats within 160 KiB - 256
bytes: T <= 154 at D 128) and blocked (above), and on the edge between them.

Bar, per output tensor (tests/test_gpu_gru.py's): e = max|x - ref64| / max|ref64|; e_kernel <= 4 e_f32 + 2^-22, with e_f32 the same figure
for a float32 CPU restatement of the same inputs: the dot products accumulated over d = 0 .. D - 1 in order and the row sums over
t = 0 .. T - 1 in order, one float32 multiply and one float32 add a term (the plainest float32 evaluation; the kernel's fma rounds once)."""
import functools

import pytest
import torch

from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -22
SENT = -12345.625                # guard value: exact in float32, far from every output
GUARD = 256
EPS = 1e-8
SHAPES = [(B, T, 128) for B in (1, 5, 33) for T in (1, 3, 20, 154, 155, 300)] + [(5, 20, 64)]


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


def layer_norm(x, eps=EPS):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)


@functools.lru_cache(maxsize=None)
def rows(B, T, D, normalised=False):
    """[2, B, T, D] float32: values of a GRU's outputs' range (tanh of a normal), or LayerNorm'd rows (unit weight, zero bias)."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + D)
    x = torch.tanh(torch.randn(2, B, T, D, generator=g, dtype=torch.float64))
    if normalised:
        x = layer_norm(x)
    return x.float()


def restate(x, dtype, diag_only=False, ln=False):
    """s [B], u_raw [2, B, D] in `dtype`.  float64: matrix products; float32: every sum term by term in index order.
    diag_only: the MUTANT that maximises over a == c only.  ln: through the last LayerNorm (unit weight, zero bias) first."""
    x = x.to(dtype)
    if ln:
        x = layer_norm(x)
    _, B, T, D = x.shape
    if dtype == torch.float64:
        dots = x[0] @ x[1].transpose(1, 2)
        u = x.mean(2)
    else:
        dots = torch.zeros(B, T, T, dtype=dtype)
        x1t = x[1].transpose(1, 2).contiguous()
        for d in range(D):
            dots = dots + x[0][:, :, d, None] * x1t[:, None, d, :]
        acc = torch.zeros(2, B, D, dtype=dtype)
        for t in range(T):
            acc = acc + x[:, :, t]
        u = acc / T
    s = torch.diagonal(dots, dim1=1, dim2=2).amax(1) if diag_only else dots.reshape(B, -1).amax(1)
    return s, u


@functools.lru_cache(maxsize=None)
def references(B, T, D, normalised=False):
    x = rows(B, T, D, normalised)
    return restate(x, torch.float64), restate(x, torch.float32)


def err(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def guarded(n):
    buf = torch.full((GUARD + n + GUARD,), SENT, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf


def ungard(buf, n, tag):
    b = buf.cpu()
    assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), f"{tag}: a write outside the output"
    o = b[GUARD:GUARD + n].clone()
    assert bool(torch.isfinite(o).all()), f"{tag}: an element was not written (or is not finite)"
    return o


def run_raw(L, x, with_u=True):
    _, B, T, D = x.shape
    xd = x.cuda()
    s, u = guarded(B), guarded(2 * B * D)
    L.call("amid_itc_pairmax_raw_f32", xd.data_ptr(), B, T, D, s[GUARD:].data_ptr(), u[GUARD:].data_ptr() if with_u else None, stream())
    torch.cuda.synchronize()
    so = ungard(s, B, "s")
    if not with_u:
        assert bool(torch.isnan(u[GUARD:GUARD + 2 * B * D]).all().item())
        return so, None
    return so, ungard(u, 2 * B * D, "u_raw").view(2, B, D)


def check(tag, got, ref64, ref32):
    ek, ef = err(got, ref64), err(ref32, ref64)
    log(f"itc_pairmax_raw {tag}: e_kernel {ek:.3e} e_f32 {ef:.3e} ratio {ek / max(ef, 1e-30):.2f}")
    assert ek <= 4 * ef + FLOOR, (tag, ek, ef)


@pytest.mark.parametrize("B,T,D", SHAPES)
def test_scores_and_means_against_fp64(L, B, T, D):
    (s64, u64), (s32, u32) = references(B, T, D)
    s, u = run_raw(L, rows(B, T, D))
    check(f"B{B} T{T} D{D} s", s, s64, s32)
    check(f"B{B} T{T} D{D} u_raw", u, u64, u32)


@pytest.mark.parametrize("B,T,D", [(5, 3, 128), (5, 154, 128), (5, 155, 128), (5, 20, 64)])
def test_the_means_are_optional(L, B, T, D):
    s_with, _ = run_raw(L, rows(B, T, D))
    s_without, _ = run_raw(L, rows(B, T, D), with_u=False)
    assert torch.equal(s_with, s_without)


@pytest.mark.parametrize("B,T,D", [(5, 3, 128), (33, 20, 128), (5, 155, 128)])
def test_a_restatement_that_pairs_equal_positions_only_is_seen(L, B, T, D):
    (s64, _), (s32, _) = references(B, T, D)
    mutant, _ = restate(rows(B, T, D), torch.float64, diag_only=True)
    s, _ = run_raw(L, rows(B, T, D))
    assert err(s, mutant) > 4 * err(s32, s64) + FLOOR, "the bar does not tell max over (a, c) from max over a == c"
    assert err(s, s64) <= 4 * err(s32, s64) + FLOOR


@pytest.mark.parametrize("B,T,D", [(5, 3, 128), (33, 20, 128), (1, 154, 128), (5, 20, 64)])
def test_both_pair_max_kernels_on_normalised_rows(L, B, T, D):
    """Rows that are already LayerNorm'd (unit weight, zero bias) are a fixed point of the last LayerNorm up to float32 rounding, so
    amid_itc_pairmax_f32 and the raw form see the same problem; each is held to ITS float64 restatement (the bits need not agree)."""
    x = rows(B, T, D, True)
    (s64, u64), (s32, u32) = references(B, T, D, True)
    s, u = run_raw(L, x)
    check(f"normalised B{B} T{T} D{D} raw s", s, s64, s32)
    check(f"normalised B{B} T{T} D{D} raw u_raw", u, u64, u32)
    l64, l32 = restate(x, torch.float64, ln=True), restate(x, torch.float32, ln=True)
    assert err(l64[0], s64) <= 2.0 ** -18 and err(l64[1], u64) <= 2.0 ** -18      # the two float64 restatements state one problem
    xd = x.cuda()
    w, b = torch.ones(2, D, device="cuda"), torch.zeros(2, D, device="cuda")
    sl, ul = torch.empty(B, device="cuda"), torch.empty(2, B, D, device="cuda")
    L.call("amid_itc_pairmax_f32", xd.data_ptr(), pa([w[0], w[1]]), pa([b[0], b[1]]), B, T, D, EPS, sl.data_ptr(), ul.data_ptr(), stream())
    torch.cuda.synchronize()
    check(f"normalised B{B} T{T} D{D} ln s", sl.cpu(), l64[0], l32[0])
    check(f"normalised B{B} T{T} D{D} ln u_raw", ul.cpu(), l64[1], l32[1])
