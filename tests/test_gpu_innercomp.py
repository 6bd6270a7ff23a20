"""The entry points of csrc/innercomp.hip (amid_inc_score_f32, amid_inc_embed_fwd_f32, amid_inc_bwd_f32, amid_bert_comp_score_f32 / _fwd_f32 /
_bwd_f32 and the four data-parallel shard entries) through the C ABI against the float64 restatement tests/comp_ref.py, which
tests/test_comp_ref.py pins to the oracle, at the smallest shapes that reach each loop of the file: the 256-thread softmax and w_bs loops,
the eight row groups of S, the 256 / D column sums of dZ, the second float4 pass at D = 256, the score kernel's LDS above 64 KiB, the
grid-stride loop of the encoder-input kernel and shards that are not the first.

Bar, per output tensor: e = max|x - ref64| / max|ref64|; e_kernel <= 4 e_f32 + 2^-22, e_f32 the larger figure of two float32 restatements
on the CPU, one in torch's summation order and one that adds every sum's terms one after the other in index order (the kernels add up to a
few hundred batch terms per chain, which torch's pairwise sums beat by more than 4).  Every figure goes to the parity log; the worst per
entry point: profiles/innercomp_kernels.md.  gate, tmq, the rows of x0 that are fl32(e + pos) or copies, and zeros are held bit for bit.
Before any launch of a chained or sharded case tests/comp_ref.py: mutants_move_the_outputs shows on the CPU that a kernel with one of five
mistakes would miss these bars by a factor of 100 or more."""
import functools

import pytest
import torch

from oracle import amid_oracle as orc
from tests import comp_ref as R
from tests.test_gpu_intercomp import GUARD, SENT, UNSUPPORTED, L, Out, pa, stream      # noqa: F401  (L: the fixture)
from tests.test_gpu_kernels import step_state
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
ERR_ARG = -1                     # AMID_ERR_ARG (include/amid_hip.h)
U8_SENT, U8_UNSET = 0xA5, 0xFF   # guard and not-written values of a byte output: tmq holds 0 .. 15


class OutU8:
    """Out (tests/test_gpu_intercomp.py) for the byte output tmq."""

    def __init__(self, *shape):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((GUARD + n + GUARD,), U8_SENT, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(U8_UNSET)

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self, tag):
        b, n = self.buf.cpu(), self.t.numel()
        assert bool((b[:GUARD] == U8_SENT).all()) and bool((b[GUARD + n:] == U8_SENT).all()), f"{tag}: a write outside the output"
        assert bool((b[GUARD:GUARD + n] < 16).all()), f"{tag}: a byte was not written"
        return b[GUARD:GUARD + n].view(self.t.shape).clone()

    def untouched(self):
        return bool((self.buf[GUARD:GUARD + self.t.numel()] == U8_UNSET).all()) and bool((self.buf[:GUARD] == U8_SENT).all())


def untouched(o):
    """Nothing of a float output (or of a pair of them) was written, nor anything around it."""
    if isinstance(o, (list, tuple)):
        return all(untouched(x) for x in o)
    if isinstance(o, OutU8):
        return o.untouched()
    n = o.t.numel()
    return bool(torch.isnan(o.t).all()) and bool((o.buf[:GUARD] == SENT).all()) and bool((o.buf[GUARD + n:] == SENT).all())


def refused(L, code, name, *args):
    from amid_amd._lib import AmidError
    with pytest.raises(AmidError) as e:
        L.call(name, *args)
    torch.cuda.synchronize()
    assert e.value.code == code, (name, e.value.code)


def check(tag, got, c, names):
    """Logs e_kernel and both e_f32 of every tensor; returns the names over the bar.  A tensor the float64 reference has exactly zero is zero."""
    bad = []
    for k in names:
        r = c["ref64"][k]
        if float(r.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, f"{tag} {k}: not zero"
            continue
        ek = R.err(got[k], r)
        ef = [R.err(x[k], r) for x in c["ref32"]]
        bar = 4 * max(ef) + R.FLOOR
        line = f"innercomp {tag} {k:6s} e_kernel {ek:.3e} e_f32 torch {ef[0]:.3e} index {ef[1]:.3e} ratio {ek / bar:.2f}"
        log(line)
        print(line)
        if not ek <= bar:
            bad.append((k, ek, ef))
    return bad


# ---------------------------------------------------------------------------- a. the scores
def run_scores(L, x, cross, entry="bert"):
    B, T, D = x.shape[1:]
    xd, s = x.cuda().contiguous(), Out(2, B)
    if entry == "inc":
        L.call("amid_inc_score_f32", xd.data_ptr(), B, T, D, s.data_ptr(), stream())
    else:
        L.call("amid_bert_comp_score_f32", xd.data_ptr(), B, T, D, cross, s.data_ptr(), stream())
    torch.cuda.synchronize()
    return s


def check_scores(L, B, T, D):
    for cross in (0, 1):
        if R.score_lds(cross, T, D) > R.SCORE_LDS_MAX:
            continue
        x, r64, r32 = R.score_case(cross, B, T, D)
        s = run_scores(L, x, cross).get("s")
        ek, ef = R.err(s, r64), [R.err(r, r64) for r in r32]
        line = f"innercomp score cross {cross} B {B} T {T} D {D} s      e_kernel {ek:.3e} e_f32 torch {ef[0]:.3e} index {ef[1]:.3e} " \
               f"ratio {ek / (4 * max(ef) + R.FLOOR):.2f} range {float(r64.min()):.2f} .. {float(r64.max()):.2f}"
        log(line)
        print(line)
        assert ek <= 4 * max(ef) + R.FLOOR, (cross, ek, ef)
        if cross:
            # a . c and c . a: the same products added in the same order of k, and a maximum does not depend on the order of its operands
            assert torch.equal(s[0], s[1])
        else:
            assert torch.equal(run_scores(L, x, 0, "inc").get("s (amid_inc_score_f32)"), s)


@pytest.mark.parametrize("B,T,D", R.SCORE_SHAPES)
def test_scores_against_fp64(L, B, T, D):
    """T 1, 15, 16, 17, 50: 256 pairs are one pass of the 256 threads.  (2, 150, 128): 79 200 and 158 400 bytes of LDS, above 64 KiB."""
    check_scores(L, B, T, D)


@pytest.mark.parametrize("cross", [0, 1])
def test_scores_at_the_last_length_accepted_and_the_first_refused(L, cross):
    T = R.last_accepted_T(cross)
    assert T == (154 if cross else 309) and R.score_lds(cross, T, 128) <= R.SCORE_LDS_MAX < R.score_lds(cross, T + 1, 128)
    x, r64, r32 = R.score_case(cross, 2, T, 128)
    s = run_scores(L, x, cross).get("s")
    ek, ef = R.err(s, r64), [R.err(r, r64) for r in r32]
    log(f"innercomp score cross {cross} B 2 T {T} D 128 s      e_kernel {ek:.3e} e_f32 torch {ef[0]:.3e} index {ef[1]:.3e}")
    assert ek <= 4 * max(ef) + R.FLOOR, (ek, ef)
    xd, out = torch.zeros(2, 2, T + 1, 128, device="cuda"), Out(2, 2)
    refused(L, UNSUPPORTED, "amid_bert_comp_score_f32", xd.data_ptr(), 2, T + 1, 128, cross, out.data_ptr(), stream())
    if not cross:
        refused(L, UNSUPPORTED, "amid_inc_score_f32", xd.data_ptr(), 2, T + 1, 128, out.data_ptr(), stream())
    assert untouched(out)


# ---------------------------------------------------------------------------- b. forward and backward, chained
def weights(c):
    """The parameters on the device (to be kept alive by the caller) and the four host arrays of two device pointers."""
    dv = {k: v.cuda() for k, v in c["P"].items()}
    return dv, [pa(dv[k]) for k in ("wnn", "bnn", "wbs", "bbs")]


def fwd_outs(c, B=None):
    B, T, D = B or c["B"], c["T"], c["D"]
    o = dict(gate=Out(2, B), S=Out(2, T, D), Z=Out(2, T, D), sw=Out(2), x0=Out(2, B, 2 * T, D))
    if c["form"] == "sas":
        o["tmq"] = OutU8(2, B, 2 * T, D // 4)
    return o


def call_fwd(L, c, xd, sd, wts, o, B, shard=None, st=None, train=0, p=0.0, posd=None):
    """One forward launch of the case's form on B rows; shard = (Bg, j0, phase) for the data-parallel entry."""
    T, D = c["T"], c["D"]
    sh = tuple(shard) if shard else ()
    outs = (o["gate"].data_ptr(), o["S"].data_ptr(), o["Z"].data_ptr(), o["sw"].data_ptr(), o["x0"].data_ptr())
    if c["form"] == "sas":
        L.call("amid_inc_embed_fwd_shard_f32" if shard else "amid_inc_embed_fwd_f32", xd.data_ptr(), sd.data_ptr(), *wts, c["thr"],
               posd[0].data_ptr(), posd[1].data_ptr(), B, T, D, *sh, *outs, o["tmq"].data_ptr(), None if st is None else st.data_ptr(), train, p,
               stream())
    else:
        L.call("amid_bert_comp_fwd_shard_f32" if shard else "amid_bert_comp_fwd_f32", xd.data_ptr(), sd.data_ptr(), *wts, c["thr"], c["cross"],
               B, T, D, *sh, *outs, stream())


def bwd_outs(c, B=None, Bg=None):
    B, T, D = B or c["B"], c["T"], c["D"]
    Bg = Bg or B
    return dict(dZ=Out(2, T, D), dS=Out(2, T, D), rows=Out(2, T, 2), dw_nn=[Out(D, D), Out(D, D)], db_nn=[Out(D), Out(D)],
                dw_bs=[Out(Bg), Out(Bg)], db_bs=[Out(1), Out(1)], dxg=Out(2, B, T, D))


def call_bwd(L, c, xd, dx0d, f, wts, o, B, shard=None, dposd=None):
    """One backward launch on the forward's gate, S and sw (f); shard = (Bg, j0, phase, gscale)."""
    T, D = c["T"], c["D"]
    sh = tuple(shard) if shard else ()
    ins = (xd.data_ptr(), dx0d.data_ptr(), f["gate"].data_ptr(), f["S"].data_ptr(), f["sw"].data_ptr(), *wts[:3])
    outs = (o["dZ"].data_ptr(), o["dS"].data_ptr(), o["rows"].data_ptr(), pa(o["dw_nn"]), pa(o["db_nn"]), pa(o["dw_bs"]), pa(o["db_bs"]),
            o["dxg"].data_ptr(), stream())
    if c["form"] == "sas":
        L.call("amid_inc_bwd_shard_f32" if shard else "amid_inc_bwd_f32", dposd.data_ptr(), dposd.shape[0], *ins, B, T, D, *sh, *outs)
    else:
        L.call("amid_bert_comp_bwd_shard_f32" if shard else "amid_bert_comp_bwd_f32", *ins, c["cross"], B, T, D, *sh, *outs)


def get_bwd(o, tag):
    got = {k: o[k].get(f"{tag} {k}") for k in ("dZ", "dS", "rows", "dxg")}
    for k in ("dw_nn", "db_nn", "dw_bs", "db_bs"):
        got[k] = torch.stack([x.get(f"{tag} {k}[{g}]") for g, x in enumerate(o[k])])
    got["db_bs"] = got["db_bs"].reshape(2)
    return got


def check_x0(tag, c, got, x, keep=None, whole=True):
    """The encoder input bit for bit: fl32(src + pos) (src: the row, or the kernel's own Z), times keep * 2 under dropout, zeros where the sum
    was zero; tmq the zero bits of the sum (whole batch: some are set, the planted e = -pos)."""
    T = c["T"]
    base = torch.cat((x, got["Z"][:, None].expand(-1, x.shape[1], -1, -1)), 2)
    if c["pos"] is not None:
        base = base + c["pos"][:, None]
    want = base if keep is None else (base * keep * 2.0) * (base != 0)
    assert torch.equal(got["x0"][:, :, :T], want[:, :, :T]), f"{tag}: x0, the rows' own half"
    assert torch.equal(got["x0"][:, :, T:], want[:, :, T:]), f"{tag}: x0, the appended token group"
    if "tmq" in got:
        assert torch.equal(got["tmq"], R._tmq(base)), f"{tag}: tmq"
        assert not whole or bool((got["tmq"][:, :, :T] != 0).any()), f"{tag}: no bit of tmq is set"


def run_chain(L, c, tag, backward=True, train=0, seed=0, step=0):
    B, T, D = c["B"], c["T"], c["D"]
    xd, (dv, wts) = c["x"].cuda(), weights(c)
    posd = None if c["pos"] is None else c["pos"].cuda()
    s = run_scores(L, c["x"], c["cross"], "inc" if c["form"] == "sas" else "bert")      # the forward runs on the kernel's own scores
    f = fwd_outs(c)
    st = step_state(L, seed, step) if train else None
    call_fwd(L, c, xd, s.t, wts, f, B, st=st, train=train, p=0.5 if train else 0.0, posd=posd)
    torch.cuda.synchronize()
    got = {k: o.get(f"{tag} {k}") for k, o in f.items()}
    got["s"] = s.get(f"{tag} s")
    log(f"innercomp {tag}: threshold {c['thr']:.6e} open {int(c['gate'][0].sum())} / {int(c['gate'][1].sum())} margin {c['margin']:.3e} "
        f"f32 softmax error {c['e32']:.3e} ratio {c['margin'] / max(c['e32'], 1e-300):.0f}")
    assert torch.equal(got["gate"], c["gate"].float()), f"{tag}: gate"
    bad = check(tag, got, c, ("s",) + R.TENSORS_FWD)
    keep = None
    if train:
        keep = torch.stack([torch.from_numpy(orc.philox_keep_flat(B * 2 * T * D, seed, orc.site_id(g, 0, orc.SITE_EMB), step, 0.5))
                            .reshape(B, 2 * T, D) for g in (0, 1)])
    check_x0(tag, c, got, c["x"], keep)
    if backward:
        dx0d = c["dx0"].cuda()
        dposd = None if c["dpos_part"] is None else c["dpos_part"].cuda()
        o = bwd_outs(c)
        call_bwd(L, c, xd, dx0d, f, wts, o, B, dposd=dposd)
        torch.cuda.synchronize()
        got.update(get_bwd(o, tag))
        for k, x in f.items():                                   # the backward's inputs are inputs: still what the forward wrote
            assert torch.equal(x.get(f"{tag} {k} after the backward"), got[k]), f"{tag}: the backward changed {k}"
        bad += check(tag, got, c, R.TENSORS_BWD)
    assert not bad, bad
    return got


@pytest.mark.parametrize("form,B,T,D,nsplit", R.CHAIN_CASES)
def test_forward_and_backward_against_fp64(L, form, B, T, D, nsplit):
    """(1, 1, 64): the smallest; 7 .. 9 rows: the eight row groups; 255 .. 257 and 600: the 256-thread loops; D 256: the second float4 pass;
    D 96: 256 / D no power of two; (64, 150, 128): the reference's amazon length; (15232, 1, 128): the largest batch the forward accepts."""
    assert R.mutants_move_the_outputs(form, B, T, D, None, nsplit)
    c = R.ref_case(form, B, T, D, nsplit, None)
    R.assert_inputs(c)
    run_chain(L, c, f"{form} B {B} T {T} D {D} nsplit {nsplit}")


@pytest.mark.parametrize("form", list(R.FORMS))
def test_forward_refuses_the_first_batch_over_its_lds(L, form):
    B, T, D = R.largest_batch() + 1, 1, 128
    c = dict(form=form, cross=R.FORMS[form], T=T, D=D, thr=0.5)
    z = lambda *shape: torch.zeros(*shape, device="cuda")      # noqa: E731
    wts = [pa(z(2, D, D)), pa(z(2, D)), pa(z(2, B)), pa(z(2, 1))]
    f = fwd_outs(c, B)
    from amid_amd._lib import AmidError
    with pytest.raises(AmidError) as e:
        call_fwd(L, c, z(2, B, T, D), z(2, B), wts, f, B, posd=z(2, 2 * T, D))
    torch.cuda.synchronize()
    assert e.value.code == UNSUPPORTED
    assert all(untouched(o) for o in f.values())


def test_grid_stride_loop_of_the_encoder_input(L):
    """(220, 150, 32): 4 B T / 8 = 16 500 workgroups of eight half-wave rows are asked for and 16 384 are launched."""
    B, T, D = 220, 150, 32
    assert (4 * B * T + 7) // 8 > 16384
    c = R.case("sas", B, T, D, backward_too=False)
    R.assert_inputs(c)
    run_chain(L, c, f"sas B {B} T {T} D {D} forward", backward=False)


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("gates", ["open", "closed"])
def test_gates_all_open_and_all_closed(L, form, gates):
    c = R.case(form, 9, 20, 64, gates=gates)
    assert bool(c["gate"].all()) if gates == "open" else not bool(c["gate"].any())
    R.assert_inputs(c)
    got = run_chain(L, c, f"{form} B 9 T 20 D 64 gates {gates}")
    if gates == "closed":
        assert float(got["S"].abs().max()) == 0.0 and float(got["dw_nn"].abs().max()) == 0.0
        assert torch.equal(got["dxg"], c["dx0"][:, :, :20])


# ---------------------------------------------------------------------------- c. dropout
@pytest.mark.parametrize("B,T,D", [(9, 20, 64), (257, 3, 128)])
def test_encoder_input_dropout_bit_for_bit(L, B, T, D):
    c = R.case("sas", B, T, D)
    R.assert_inputs(c)
    run_chain(L, c, f"sas B {B} T {T} D {D} dropout", backward=False, train=1, seed=1234 + B, step=3)


# ---------------------------------------------------------------------------- d. shards
@pytest.mark.parametrize("form,Bg,T,D,sizes", R.SHARD_CASES)
def test_shards_against_the_unsharded_entry_and_fp64(L, form, Bg, T, D, sizes):
    """The ranks' calls one after the other on one GPU; the two all-reduces (S, dZ) as float32 sums in rank order."""
    assert sum(sizes) == Bg
    if len(sizes) > 1:
        assert "shard_j0" in R.mutants_move_the_outputs(form, Bg, T, D, sizes, 1)
    c = R.ref_case(form, Bg, T, D, 1, sizes)
    R.assert_inputs(c)
    tag = f"{form} Bg {Bg} T {T} D {D} shards {'+'.join(map(str, sizes))}"
    whole = run_chain(L, c, tag + " unsharded")
    world, ranges = len(sizes), R.shard_ranges(sizes)
    (dv, wts), posd = weights(c), None if c["pos"] is None else c["pos"].cuda()
    entry = "inc" if form == "sas" else "bert"
    xs = [c["x"][:, lo:hi].contiguous() for lo, hi in ranges]
    xd = [x.cuda() for x in xs]
    # all-gather of the ranks' scores, per domain in rank order
    s_all = torch.cat([run_scores(L, x, c["cross"], entry).get("s") for x in xs], 1)
    assert torch.equal(s_all, whole["s"])
    sd = s_all.cuda()
    f = [fwd_outs(c, hi - lo) for lo, hi in ranges]
    for r, (lo, hi) in enumerate(ranges):
        call_fwd(L, c, xd[r], sd, wts, f[r], hi - lo, shard=(Bg, lo, 1), posd=posd)
    torch.cuda.synchronize()
    S_sum = functools.reduce(torch.add, [o["S"].get(f"{tag} S of rank {r}") for r, o in enumerate(f)])
    for r, (lo, hi) in enumerate(ranges):
        assert torch.equal(f[r]["gate"].get(f"{tag} gate of rank {r}"), whole["gate"][:, lo:hi])
        assert torch.equal(f[r]["sw"].get(f"{tag} sw of rank {r}"), whole["sw"])
        assert untouched(f[r]["Z"]) and untouched(f[r]["x0"])                   # phase 1 ends at the all-reduce
        f[r]["S"].t.copy_(S_sum)
        call_fwd(L, c, xd[r], sd, wts, f[r], hi - lo, shard=(Bg, lo, 2), posd=posd)
    torch.cuda.synchronize()
    bad = []
    got_f = []
    for r, (lo, hi) in enumerate(ranges):
        g = {k: o.get(f"{tag} {k} of rank {r}") for k, o in f[r].items()}
        got_f.append(g)
        assert torch.equal(g["gate"], whole["gate"][:, lo:hi]) and torch.equal(g["sw"], whole["sw"]) and torch.equal(g["S"], S_sum)
        assert torch.equal(g["Z"], got_f[0]["Z"])                # every rank finishes the same group
        check_x0(f"{tag} rank {r}", c, g, xs[r], whole=False)
        assert torch.equal(g["x0"][:, :, :T], whole["x0"][:, lo:hi, :T])
        if "tmq" in g:
            assert torch.equal(g["tmq"][:, :, :T], whole["tmq"][:, lo:hi, :T])
        if world == 1:
            for k in g:
                assert torch.equal(g[k], whole[k]), f"{tag}: {k} differs from the unsharded entry's"
    bad += check(tag + " fwd", got_f[0], c, ("S", "Z", "sw"))
    # backward
    dxd = [c["dx0"][:, lo:hi].contiguous().cuda() for lo, hi in ranges]
    dposd = [None if c["dpos_part"] is None else c["dpos_part"][r:r + 1].contiguous().cuda() for r in range(world)]
    o = [bwd_outs(c, hi - lo, Bg) for lo, hi in ranges]
    for r, (lo, hi) in enumerate(ranges):
        call_bwd(L, c, xd[r], dxd[r], f[r], wts, o[r], hi - lo, shard=(Bg, lo, 1, 1.0 / world), dposd=dposd[r])
    torch.cuda.synchronize()
    dZ_sum = functools.reduce(torch.add, [x["dZ"].get(f"{tag} dZ of rank {r}") for r, x in enumerate(o)])
    for r, (lo, hi) in enumerate(ranges):
        assert all(untouched(o[r][k]) for k in ("dS", "rows", "dw_nn", "db_nn", "dw_bs", "db_bs", "dxg"))
        o[r]["dZ"].t.copy_(dZ_sum)
        call_bwd(L, c, xd[r], dxd[r], f[r], wts, o[r], hi - lo, shard=(Bg, lo, 2, 1.0 / world), dposd=dposd[r])
    torch.cuda.synchronize()
    gb = [get_bwd(o[r], f"{tag} rank {r}") for r in range(world)]
    tot = dict(dZ=dZ_sum, dS=gb[0]["dS"], rows=gb[0]["rows"], dxg=torch.cat([g["dxg"] for g in gb], 1))
    for k in ("dw_nn", "db_nn", "db_bs", "dw_bs"):               # the dense exchange sums the ranks (gscale = 1 / world is in the first three)
        tot[k] = functools.reduce(torch.add, [g[k] for g in gb])
    for r, (lo, hi) in enumerate(ranges):
        outside = torch.ones(Bg, dtype=torch.bool)
        outside[lo:hi] = False
        assert float(gb[r]["dw_bs"][:, outside].abs().max()) == 0.0 if world > 1 else True, f"{tag}: dw_bs of rank {r} outside its slice"
        assert torch.equal(gb[r]["dZ"], dZ_sum) and torch.equal(gb[r]["dS"], gb[0]["dS"]) and torch.equal(gb[r]["rows"], gb[0]["rows"])
        for k, x in f[r].items():
            assert torch.equal(x.get(f"{tag} {k} of rank {r} after the backward"), got_f[r][k])
        if world == 1:
            for k in R.TENSORS_BWD:
                assert torch.equal(gb[0][k], whole[k]), f"{tag}: {k} differs from the unsharded entry's"
    bad += check(tag + " bwd", tot, c, R.TENSORS_BWD)
    assert not bad, bad


# ---------------------------------------------------------------------------- e. refusals
def zero_case(form, B, T, D):
    c = dict(form=form, cross=R.FORMS[form], T=T, D=D, thr=0.5)
    z = lambda *shape: torch.zeros(*shape, device="cuda")      # noqa: E731
    keep = [z(2, D, D), z(2, D), z(2, B), z(2, 1)]
    return c, z, keep, [pa(t) for t in keep]


def fwd_bwd_refused(L, code, form, B, T, D, shard_f=None, shard_b=None, Bg=None):
    c, z, keep, wts = zero_case(form, Bg or B, T, D)
    f, o = fwd_outs(c, B), bwd_outs(c, B, Bg)
    from amid_amd._lib import AmidError
    with pytest.raises(AmidError) as e:
        call_fwd(L, c, z(2, B, T, D), z(2, Bg or B), wts, f, B, shard=shard_f, posd=z(2, 2 * T, D))
    assert e.value.code == code, ("forward", e.value.code)
    ins = dict(gate=z(2, B), S=z(2, T, D), sw=z(2))
    with pytest.raises(AmidError) as e:
        call_bwd(L, c, z(2, B, T, D), z(2, B, 2 * T, D), ins, wts, o, B, shard=shard_b, dposd=z(1, 2, 2 * T, D))
    assert e.value.code == code, ("backward", e.value.code)
    torch.cuda.synchronize()
    assert all(untouched(x) for x in f.values()) and all(untouched(x) for x in o.values())


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("D", [30, 66, 260, 512])
def test_refuses_rows_no_multiple_of_4_or_wider_than_256(L, form, D):
    """comp_tokens_fwd / comp_tokens_bwd: D % 4 == 0 && D <= 256, else AMID_ERR_ARG before anything is launched."""
    fwd_bwd_refused(L, ERR_ARG, form, 5, 3, D)
    fwd_bwd_refused(L, ERR_ARG, form, 5, 3, D, shard_f=(5, 0, 1), shard_b=(5, 0, 1, 1.0))


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("phase", [0, 3, -1])
def test_shard_entries_refuse_a_phase_outside_1_and_2(L, form, phase):
    fwd_bwd_refused(L, ERR_ARG, form, 5, 3, 64, shard_f=(10, 5, phase), shard_b=(10, 5, phase, 0.5), Bg=10)


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("j0,phase", [(6, 1), (6, 2), (-1, 1)])
def test_shard_entries_refuse_rows_outside_the_global_batch(L, form, j0, phase):
    """j0 + B > Bg (and j0 < 0): AMID_ERR_ARG."""
    fwd_bwd_refused(L, ERR_ARG, form, 5, 3, 64, shard_f=(10, j0, phase), shard_b=(10, j0, phase, 0.5), Bg=10)
