"""InterComp's three entry points (csrc/intercomp.hip: amid_itc_pairmax_f32, amid_itc_mix_fwd_f32, amid_itc_mix_bwd_f32) through the C ABI
against float64 restatements of the formulas in that file's header comment (reference: InterComp.forward model_seq.py:483-497 as used at
:426-434), at the batch sizes on both sides of every dispatch edge of the two mix entry points.

Bar, per output tensor: e = max|x - ref64| / max|ref64|; e_kernel <= 4 e_f32 + 2^-22, with e_f32 the same figure for a float32 restatement
in plain torch on the CPU.  The 4 allows for another summation order (the kernels add 16 or 32 partial sums in a fixed order, torch adds
pairwise); the floor is a couple of float32 ulps of the largest entry, for tensors the restatement happens to get exact.  Both figures of
every case and tensor go to the parity log (tests/test_gpu_sasrec.py: log); the worst per entry point: profiles/intercomp_kernels.md."""
import functools

import pytest
import torch

from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
UNSUPPORTED = -2                 # AMID_ERR_UNSUPPORTED (include/amid_hip.h)
EPS = 1e-8                       # SASREC_LN_EPS
FLOOR = 2.0 ** -22
SENT = -12345.625                # guard value: exact in float32, far from every output
GUARD = 512                      # floats on either side of an output (4 rows at D 128; keeps the 16-byte alignment of the float4 stores)
FAST_LO, FAST_HI = 32, 256       # the 512-thread forms: 32 <= B <= MIXF_RG * MIXF_K = 16 * 16 (csrc/itc_mix_parts.h), D 64 / 128


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
    """An output of n floats inside a larger allocation: NaN where the kernel must write, SENT in the guards before and after."""

    def __init__(self, *shape):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((GUARD + n + GUARD,), SENT, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(float("nan"))

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self, tag):
        """The output on the CPU, after checking that every element was written and nothing outside it was."""
        b = self.buf.cpu()
        n = self.t.numel()
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), f"{tag}: a write outside the output"
        assert bool(torch.isfinite(b[GUARD:GUARD + n]).all()), f"{tag}: an element was not written (or is not finite)"
        return b[GUARD:GUARD + n].view(self.t.shape).clone()


def err(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def check(tag, got, ref64, ref32):
    """{name: tensor} of the kernel, the float64 reference and the float32 restatement: logs both errors, returns the names over the bar."""
    bad = []
    for k, r in ref64.items():
        ek, ef = err(got[k], r), err(ref32[k], r)
        log(f"intercomp {tag} {k:7s} e_kernel {ek:.3e} e_f32 {ef:.3e}")
        print(f"intercomp {tag} {k:7s} e_kernel {ek:.3e} e_f32 {ef:.3e} bar {4 * ef + FLOOR:.3e}")
        if not ek <= 4 * ef + FLOOR:
            bad.append((k, ek, ef))
    return bad


# ---------------------------------------------------------------------------- pair-max
def layer_norm(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w + b


def pairmax_ref(x, lnw, lnb, dtype):
    """s_j = max_{a,c} LN(x[0,j,a]) . LN(x[1,j,c]);  u_raw = mean_t LN(x)."""
    f = [layer_norm(x[g].to(dtype), lnw[g].to(dtype), lnb[g].to(dtype)) for g in (0, 1)]
    s = torch.matmul(f[0], f[1].transpose(1, 2)).amax(dim=(1, 2))
    return dict(s=s, u_raw=torch.stack((f[0].mean(1), f[1].mean(1))))


@functools.lru_cache(maxsize=None)
def pairmax_case(B, T, D):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + D)
    x = torch.randn(2, B, T, D, generator=g) * (0.5 + torch.rand(2, B, T, 1, generator=g)) + 0.3 * torch.randn(2, B, T, 1, generator=g)
    lnw = 0.5 + torch.rand(2, D, generator=g)                    # per domain, away from 1 / 0
    lnb = 0.2 * torch.randn(2, D, generator=g)
    return x, lnw, lnb, pairmax_ref(x, lnw, lnb, torch.float64), pairmax_ref(x, lnw, lnb, torch.float32)


def pairmax_lds(T, D):
    return 2 * T * (D + 4) * 4                                   # amid_itc_pairmax_f32: both domains' rows of a batch row, padded by 4


PAIRMAX_LDS_MAX = 160 * 1024 - 256
# (2, 150, 128): the reference's amazon length.  152 and 154 rows of 128: 160 512 and 162 624 bytes, the last lengths the entry accepts
PAIRMAX_SHAPES = [(3, 1, 64), (4, 7, 32), (5, 20, 64), (3, 50, 128), (2, 150, 128), (2, 152, 128), (2, 154, 128)]


@pytest.mark.parametrize("B,T,D", PAIRMAX_SHAPES)
def test_pairmax_against_fp64(L, B, T, D):
    x, lnw, lnb, ref64, ref32 = pairmax_case(B, T, D)
    assert pairmax_lds(T, D) <= PAIRMAX_LDS_MAX
    xd, wd, bd = x.cuda(), lnw.cuda(), lnb.cuda()
    s0, s1, u = Out(B), Out(B), Out(2, B, D)
    L.call("amid_itc_pairmax_f32", xd.data_ptr(), pa([wd[0], wd[1]]), pa([bd[0], bd[1]]), B, T, D, EPS, s0.data_ptr(), None, stream())
    L.call("amid_itc_pairmax_f32", xd.data_ptr(), pa([wd[0], wd[1]]), pa([bd[0], bd[1]]), B, T, D, EPS, s1.data_ptr(), u.data_ptr(), stream())
    torch.cuda.synchronize()
    got = dict(s=s1.get("s"), u_raw=u.get("u_raw"))
    assert torch.equal(s0.get("s (u_raw NULL)"), got["s"])       # the means are a by-product: s does not depend on asking for them
    bad = check(f"pairmax B {B} T {T} D {D}", got, ref64, ref32)
    assert not bad, bad


# ---------------------------------------------------------------------------- mix
def mix_fwd_ref(u_raw, gate, P, dtype):
    """z_g = sum_j w_bs_g[j] gate_j u_raw[1-g][j];  c_g = W_nn_g z_g + b_nn_g sum_j w_bs_g[j] + b_bs_g;  u_mix = 0.5 u_raw + 0.5 c."""
    gate = gate.to(dtype)
    z, sw, um = [], [], []
    for g in (0, 1):
        wbs = P["wbs"][g].to(dtype)
        z.append(((wbs * gate)[:, None] * u_raw[1 - g]).sum(0))
        sw.append(wbs.sum())
        c = P["wnn"][g].to(dtype) @ z[g] + P["bnn"][g].to(dtype) * sw[g] + P["bbs"][g].to(dtype)
        um.append(0.5 * u_raw[g] + 0.5 * c)
    return dict(z=torch.stack(z), sw=torch.stack(sw), u_mix=torch.stack(um))


def mix_bwd_ref(u_raw, gate, P, du_mix, dtype):
    """Autograd through mix_fwd_ref with the gate held constant."""
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    u = u_raw.to(dtype).clone().requires_grad_(True)
    out = mix_fwd_ref(u, gate, leaves, dtype)["u_mix"]
    names = ["wnn", "bnn", "wbs", "bbs"]
    gs = torch.autograd.grad((out * du_mix.to(dtype)).sum(), [u] + [leaves[n] for n in names])
    return dict(du_raw=gs[0], dw_nn=gs[1], db_nn=gs[2], dw_bs=gs[3], db_bs=gs[4].reshape(2))


def pick_gate(s):
    """The threshold in the widest gap of the float64 batch softmax of s among the gaps that leave a quarter to three quarters of the gates open,
    as the float32 value the entry point receives; the float64 gate; (distance to the nearest softmax value) / (error of a float32 softmax)."""
    B = s.numel()
    sm = torch.softmax(s.double(), 0)
    if B == 1:
        thr = 0.5                                                # softmax = 1: any threshold below 1
    else:
        v = sm.sort().values
        gaps, n_open = v[1:] - v[:-1], B - 1 - torch.arange(B - 1)          # a threshold between v[i] and v[i + 1] leaves B - 1 - i gates open
        gaps = torch.where((4 * n_open >= B) & (4 * n_open <= 3 * B), gaps, torch.zeros_like(gaps))
        i = int(gaps.argmax())
        thr = float(torch.tensor(float((v[i] + v[i + 1]) / 2), dtype=torch.float32))
    gate = sm > thr
    e32 = float((torch.softmax(s.float(), 0).double() - sm).abs().max())
    return thr, gate, float((sm - thr).abs().min()), e32


@functools.lru_cache(maxsize=None)
def mix_case(B, D):
    g = torch.Generator().manual_seed(100 * B + D)
    rn = lambda *shape: torch.randn(*shape, generator=g)      # noqa: E731
    s = 2.0 * rn(B)
    thr, gate, margin, e32 = pick_gate(s)
    # rows and domains all different; a per-domain offset, as LayerNorm's bias gives the real means
    u_raw = 0.5 * rn(2, B, D) + 0.3 * rn(2, 1, D)
    # the upstream gradient: random per element, with a per-domain mean of about two standard deviations of the batch sum, so that the sums
    # over the batch (dc, and through it every parameter gradient) are not the cancellation of their terms -- a sum that cancels has no
    # float32 accuracy to hold a kernel to -- while the random part still tells the columns apart
    du_mix = rn(2, B, D) + torch.tensor([2.0, -1.5])[:, None, None] / B ** 0.5
    sign = lambda t: torch.where(t >= 0, 1.0, -1.0)            # noqa: E731
    b = rn(2, D)
    # w_bs: every third row negative (other rows in the two domains), so both signs from B = 3 on and sum_j w_bs[j] (sw) does not cancel either
    wsign = torch.stack([torch.where(torch.arange(B) % 3 == 1 + d, -1.0, 1.0) for d in (0, 1)])
    P = dict(wnn=rn(2, D, D) / D ** 0.5,
             bnn=sign(b) * (0.05 + 0.3 * b.abs()),               # non-zero, both signs
             wbs=wsign * (0.02 + torch.rand(2, B, generator=g)) / B ** 0.5,
             bbs=torch.tensor([[0.37], [-0.21]]))
    u64 = u_raw.double()
    ref64 = {**mix_fwd_ref(u64, gate, {k: v.double() for k, v in P.items()}, torch.float64), **mix_bwd_ref(u_raw, gate, P, du_mix, torch.float64)}
    ref32 = {**mix_fwd_ref(u_raw, gate, P, torch.float32), **mix_bwd_ref(u_raw, gate, P, du_mix, torch.float32)}
    return dict(s=s, thr=thr, gate=gate, margin=margin, e32=e32, u_raw=u_raw, du_mix=du_mix, P=P, ref64=ref64, ref32=ref32)


def assert_mix_inputs(c, B):
    """Conditions on the inputs, before any launch: a gate of both kinds, and a threshold no float32 softmax can be on the wrong side of."""
    if B >= 2:
        n = int(c["gate"].sum())
        assert 0 < n < B and B <= 4 * n <= 3 * B, (n, B)
    for g in (0, 1):
        assert B < 3 or (bool((c["P"]["wbs"][g] > 0).any()) and bool((c["P"]["wbs"][g] < 0).any()))
        assert bool((c["P"]["bnn"][g] > 0).any()) and bool((c["P"]["bnn"][g] < 0).any())
    assert c["margin"] >= 100 * c["e32"], (c["margin"], c["e32"])


MIX_SHAPES = [(1, 64), (5, 32), (FAST_LO - 1, 128), (FAST_LO, 64), (33, 128), (48, 64), (255, 64), (FAST_HI, 128), (FAST_HI + 1, 128), (512, 64)]


def run_mix_fwd(L, c, B, D):
    dv = {k: v.cuda() for k, v in c["P"].items()}
    u_raw, s = c["u_raw"].cuda(), c["s"].cuda()
    out = dict(gate=Out(B), z=Out(2, D), sw=Out(2), u_mix=Out(2, B, D))
    L.call("amid_itc_mix_fwd_f32", u_raw.data_ptr(), s.data_ptr(), pa(dv["wnn"]), pa(dv["bnn"]), pa(dv["wbs"]), pa(dv["bbs"]), c["thr"], B, D,
           out["gate"].data_ptr(), out["z"].data_ptr(), out["sw"].data_ptr(), out["u_mix"].data_ptr(), stream())
    torch.cuda.synchronize()
    return dv, u_raw, out


@pytest.mark.parametrize("B,D", MIX_SHAPES)
def test_mix_forward_against_fp64(L, B, D):
    c = mix_case(B, D)
    assert_mix_inputs(c, B)
    _, _, out = run_mix_fwd(L, c, B, D)
    got = {k: o.get(k) for k, o in out.items()}
    log(f"intercomp mix fwd B {B} D {D}: threshold {c['thr']:.6e} open {int(c['gate'].sum())} margin {c['margin']:.3e} f32 softmax error {c['e32']:.3e}")
    assert torch.equal(got["gate"], c["gate"].float())
    bad = check(f"mix fwd B {B} D {D}", got, {k: c["ref64"][k] for k in ("z", "sw", "u_mix")}, c["ref32"])
    assert not bad, bad


@pytest.mark.parametrize("B,D", MIX_SHAPES)
def test_mix_backward_against_fp64_autograd(L, B, D):
    """The backward on the forward kernel's own gate, z and sw, as the engine runs it."""
    c = mix_case(B, D)
    assert_mix_inputs(c, B)
    dv, u_raw, fwd = run_mix_fwd(L, c, B, D)
    assert torch.equal(fwd["gate"].get("gate"), c["gate"].float())
    du_mix = c["du_mix"].cuda()
    out = dict(du_raw=Out(2, B, D), dw_nn=[Out(D, D), Out(D, D)], db_nn=[Out(D), Out(D)], dw_bs=[Out(B), Out(B)], db_bs=[Out(1), Out(1)])
    L.call("amid_itc_mix_bwd_f32", du_mix.data_ptr(), u_raw.data_ptr(), fwd["gate"].data_ptr(), fwd["z"].data_ptr(), fwd["sw"].data_ptr(),
           pa(dv["wnn"]), pa(dv["bnn"]), pa(dv["wbs"]), B, D, out["du_raw"].data_ptr(), pa(out["dw_nn"]), pa(out["db_nn"]), pa(out["dw_bs"]),
           pa(out["db_bs"]), stream())
    torch.cuda.synchronize()
    got = dict(du_raw=out["du_raw"].get("du_raw"))
    for k in ("dw_nn", "db_nn", "dw_bs", "db_bs"):
        got[k] = torch.stack([o.get(f"{k}[{g}]") for g, o in enumerate(out[k])])
    got["db_bs"] = got["db_bs"].reshape(2)
    for k, o in fwd.items():                                     # the backward's inputs are inputs: still what the forward wrote
        o.get(f"{k} after the backward")
    bad = check(f"mix bwd B {B} D {D}", got, {k: c["ref64"][k] for k in ("du_raw", "dw_nn", "db_nn", "dw_bs", "db_bs")}, c["ref32"])
    assert not bad, bad


# ---------------------------------------------------------------------------- refusals
def raises_unsupported(L, name, *args):
    from amid_amd._lib import AmidError
    with pytest.raises(AmidError) as e:
        L.call(name, *args)
    torch.cuda.synchronize()
    assert e.value.code == UNSUPPORTED, (name, e.value.code)


def first_refused_T(D):
    T = 1
    while pairmax_lds(T, D) <= PAIRMAX_LDS_MAX:
        T += 1
    return T


@pytest.mark.parametrize("B,T,D", [(2, first_refused_T(128), 128), (2, 8, 132)])
def test_pairmax_refuses(L, B, T, D):
    """Over the LDS limit (160 KiB less 256 bytes: 155 rows of 128 -- 152 rows, 160 512 bytes, are within it and are checked above), and a row
    wider than 32 lanes of one float4."""
    assert T == 8 or (T == 155 and pairmax_lds(T - 1, D) <= PAIRMAX_LDS_MAX < pairmax_lds(T, D))
    x, w, b = torch.randn(2, B, T, D, device="cuda"), torch.ones(2, D, device="cuda"), torch.zeros(2, D, device="cuda")
    s, u = Out(B), Out(2, B, D)
    raises_unsupported(L, "amid_itc_pairmax_f32", x.data_ptr(), pa([w[0], w[1]]), pa([b[0], b[1]]), B, T, D, EPS, s.data_ptr(), u.data_ptr(), stream())
    assert bool(torch.isnan(s.t).all()) and bool(torch.isnan(u.t).all())


def mix_fwd_lds(B, D):
    return (((B + 3) & ~3) + 4 * D + 32 * 2 * D) * 4               # amid_itc_mix_fwd_f32, the looped form: gate | z, c | 32 row groups' partials


def mix_buffers(B, D):
    z = lambda *shape: torch.zeros(*shape, device="cuda")      # noqa: E731
    return dict(u_raw=z(2, B, D), s=z(B), wnn=z(2, D, D), bnn=z(2, D), wbs=z(2, B), bbs=z(2, 1), gate=Out(B), zz=Out(2, D), sw=Out(2), u_mix=Out(2, B, D))


def mix_fwd_refused(L, B, D):
    m = mix_buffers(B, D)
    raises_unsupported(L, "amid_itc_mix_fwd_f32", m["u_raw"].data_ptr(), m["s"].data_ptr(), pa(m["wnn"]), pa(m["bnn"]), pa(m["wbs"]), pa(m["bbs"]), 0.5,
                       B, D, m["gate"].data_ptr(), m["zz"].data_ptr(), m["sw"].data_ptr(), m["u_mix"].data_ptr(), stream())
    assert all(bool(torch.isnan(m[k].t).all()) for k in ("gate", "zz", "sw", "u_mix"))


@pytest.mark.parametrize("D", [128, 32])
def test_mix_forward_refuses_the_first_batch_over_its_lds(L, D):
    B = FAST_HI + 1
    while mix_fwd_lds(B, D) <= 60 * 1024:
        B += 1
    assert mix_fwd_lds(B - 1, D) <= 60 * 1024 < mix_fwd_lds(B, D) and B == {128: 6657, 32: 13185}[D]
    mix_fwd_refused(L, B, D)


@pytest.mark.parametrize("B", [8, 48])                           # a batch of the looped form and one of the 512-thread form's range
@pytest.mark.parametrize("D", [132, 256])
def test_mix_refuses_rows_wider_than_128(L, B, D):
    """Every mix kernel gives a row 32 lanes of one float4: beyond D = 128 it would leave the columns past 128 out and still return AMID_OK."""
    mix_fwd_refused(L, B, D)
    m = mix_buffers(B, D)
    out = dict(du_raw=Out(2, B, D), dw_nn=[Out(D, D), Out(D, D)], db_nn=[Out(D), Out(D)], dw_bs=[Out(B), Out(B)], db_bs=[Out(1), Out(1)])
    raises_unsupported(L, "amid_itc_mix_bwd_f32", m["u_raw"].data_ptr(), m["u_raw"].data_ptr(), m["s"].data_ptr(), m["wnn"].data_ptr(), m["bnn"].data_ptr(),
                       pa(m["wnn"]), pa(m["bnn"]), pa(m["wbs"]), B, D, out["du_raw"].data_ptr(), pa(out["dw_nn"]), pa(out["db_nn"]), pa(out["dw_bs"]),
                       pa(out["db_bs"]), stream())
    assert bool(torch.isnan(out["du_raw"].t).all()) and all(bool(torch.isnan(o.t).all()) for k in ("dw_nn", "db_nn", "dw_bs", "db_bs") for o in out[k])
