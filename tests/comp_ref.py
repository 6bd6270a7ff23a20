"""Plain-torch restatement of the token-group formulas in the header comment of amid_amd/csrc/innercomp.hip (reference: InnerComp.forward
model_seq.py:459-472, InterComp.forward :483-497 in front of BERT4Rec's encoders), for any dtype, with every tensor the kernels write:

    forward    s, softmax, gate, sw, S, Z, x0 (with or without positional rows), tmq
    backward   dZ, dS, rows ([2, T, 2]: sum_d dZ, sum_d dZ b_nn), dw_nn, db_nn, dw_bs, db_bs, dxg

`order` selects how every sum is taken: "torch" = torch's own ops; "index" = every sum over the batch, over T and over D one term after the
other in index order in the working dtype (an explicit loop: torch.cumsum accumulates float32 in float64 on the CPU).  The backward of
order "torch" is autograd through the forward with the gate held constant; order "index" states the same gradients as the explicit sums of
the header comment, and tests/test_comp_ref.py holds the two to each other in float64.

`mutant` restates one mistake a kernel could make (MUTANTS); tests/test_comp_ref.py asserts that each moves the float64 outputs by far more
than the bar tests/test_gpu_innercomp.py holds the kernels to.  The cases of that file (inputs, thresholds, references) are built here so
that the CPU test can check them without a GPU."""
import functools

import torch

FLOOR = 2.0 ** -22
MUTANTS = ("no_diag", "bnn_once", "dwbs_no_b", "shard_j0", "cross_own")


# ---------------------------------------------------------------------------- sums
def _sum(x, dim, order):
    if order == "torch":
        return x.sum(dim)
    acc = torch.zeros_like(x.select(dim, 0))
    for i in range(x.shape[dim]):
        acc = acc + x.select(dim, i)
    return acc


def _mm(a, b, order):
    """a [..., m, k] @ b [..., k, n]"""
    if order == "torch":
        return a @ b
    acc = torch.zeros(*torch.broadcast_shapes(a.shape[:-2], b.shape[:-2]), a.shape[-2], b.shape[-1], dtype=a.dtype)
    for k in range(a.shape[-1]):
        acc = acc + a[..., :, k, None] * b[..., None, k, :]
    return acc


def _cast(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


# ---------------------------------------------------------------------------- forward
def scores(x, cross, order="torch", mutant=None):
    """s[g][j] = max_{a,c} e[g,j,a] . e[cross ? 1-g : g, j, c]"""
    out = []
    for g in (0, 1):
        pair = _mm(x[g], x[1 - g if cross else g].transpose(1, 2), order)          # [B, T, T]
        if mutant == "no_diag" and not cross:
            T = pair.shape[-1]
            pair = pair.masked_fill(~torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
        out.append(pair.amax(dim=(1, 2)))
    return torch.stack(out)


def _tokens(x, P, gate, cross, order, mutant=None, shards=None):
    """sw [2], S [2, T, D], Z [2, T, D] from rows x [2, B, T, D] and a 0/1 gate [2, B] (a constant)."""
    sw, S, Z = [], [], []
    for g in (0, 1):
        sd = 1 - g if (cross and mutant != "cross_own") else g
        w = P["wbs"][g]
        wsrc = w
        if mutant == "shard_j0" and shards:                     # every shard reads w_bs from its own index 0
            wsrc = torch.cat([w[:hi - lo] for lo, hi in shards])
        cj = wsrc * gate[g]
        S.append(_sum(cj[:, None, None] * x[sd], 0, order))
        sw.append(_sum(w, 0, order))
        Z.append(_mm(S[g], P["wnn"][g].t(), order) + P["bnn"][g] * (1.0 if mutant == "bnn_once" else sw[g]) + P["bbs"][g])
    return sw, S, Z                                              # lists over the two modules (autograd differentiates with respect to S[g])


def _tmq(x0):
    """One byte per 4 features: bit i set where feature 4c + i of the encoder input is zero."""
    z = (x0 == 0).reshape(*x0.shape[:-1], x0.shape[-1] // 4, 4).to(torch.uint8)
    return z[..., 0] | (z[..., 1] << 1) | (z[..., 2] << 2) | (z[..., 3] << 3)


def forward(xg, P, cross, dtype, order="torch", threshold=None, gate=None, pos=None, mutant=None, shards=None):
    """gate: the given 0/1 tensor [2, B], or softmax over the batch of the scores > threshold."""
    x, P = xg.to(dtype), _cast(P, dtype)
    s = scores(x, cross, order, mutant)
    sm = torch.softmax(s, 1)
    gate = (sm > threshold) if gate is None else gate
    gate = gate.to(dtype)
    sw, S, Z = (torch.stack(v) for v in _tokens(x, P, gate, cross, order, mutant, shards))
    B = x.shape[1]
    x0 = torch.cat((x, Z[:, None].expand(-1, B, -1, -1)), 2)
    if pos is not None:
        x0 = x0 + pos.to(dtype)[:, None]
    return dict(s=s, softmax=sm, gate=gate, sw=sw, S=S, Z=Z, x0=x0, tmq=_tmq(x0))


# ---------------------------------------------------------------------------- backward
def backward(xg, P, cross, dtype, gate, dx0, order="torch", dz_parts=None, mutant=None, shards=None):
    """dx0 [2, B, 2T, D]: the cotangent of the encoder input.  dz_parts [nsplit, 2, T, D]: the cotangent of Z as partial sums (the SASRec
    form reads the embedding backward's positional partials), added in their order; None: dZ[t] = sum_b dx0[b, T + t]."""
    x, P, gate, dx0 = xg.to(dtype), _cast(P, dtype), gate.to(dtype), dx0.to(dtype)
    T = x.shape[2]
    dZ = _sum(dx0[:, :, T:], 1, order) if dz_parts is None else _sum(dz_parts.to(dtype), 0, order)
    rows = torch.stack((_sum(dZ, -1, order), _sum(dZ * P["bnn"][:, None], -1, order)), -1)
    if order == "torch":
        leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        xl = x.clone().requires_grad_(True)
        sw, S, Z = _tokens(xl, leaves, gate, cross, order, mutant, shards)
        loss = (xl * dx0[:, :, :T]).sum() + (torch.stack(Z) * dZ).sum()
        gs = torch.autograd.grad(loss, [xl, S[0], S[1]] + [leaves[n] for n in ("wnn", "bnn", "wbs", "bbs")])
        gs = (gs[0], torch.stack(gs[1:3])) + gs[3:]
        dw_bs = gs[4]
        if mutant == "dwbs_no_b":
            dw_bs = dw_bs - rows[:, :, 1].sum(1)[:, None]
        return dict(dZ=dZ, dS=gs[1], rows=rows, dw_nn=gs[2], db_nn=gs[3], dw_bs=dw_bs, db_bs=gs[5].reshape(2), dxg=gs[0])
    sw, S = (torch.stack(v) for v in _tokens(x, P, gate, cross, order, mutant, shards)[:2])
    dS = _mm(dZ, P["wnn"], order)                                               # dS[t][k] = sum_d dZ[t][d] W_nn[d][k]
    dw_nn = _mm(dZ.transpose(1, 2), S, order)                                   # sum_t dZ[t]^T S[t]
    db_nn = (1.0 if mutant == "bnn_once" else sw[:, None]) * _sum(dZ, 1, order)
    db_bs = _sum(rows[:, :, 0], 1, order)
    dxg = dx0[:, :, :T].clone()
    dw_bs = []
    for g in (0, 1):
        sd = 1 - g if (cross and mutant != "cross_own") else g
        w = P["wbs"][g]
        if mutant == "shard_j0" and shards:
            w = torch.cat([w[:hi - lo] for lo, hi in shards])
        dot = _sum(_sum(dS[g][None] * x[sd], -1, order), -1, order)
        dw_bs.append(gate[g] * dot + (0.0 if mutant == "dwbs_no_b" else _sum(rows[g, :, 1], 0, order)))
        dxg[sd] = dxg[sd] + (w * gate[g])[:, None, None] * dS[g]
    return dict(dZ=dZ, dS=dS, rows=rows, dw_nn=dw_nn, db_nn=db_nn, dw_bs=torch.stack(dw_bs), db_bs=db_bs, dxg=dxg)


# ---------------------------------------------------------------------------- the threshold
def pick_gate(s64, s32s):
    """tests/test_gpu_intercomp.py: pick_gate for two domains under one threshold: the middle of the widest gap of the float64 batch softmax
    (both domains' values together) among the gaps that leave a quarter to three quarters of BOTH domains' gates open, as the float32 value
    the entry receives; the float64 gate; the distance to the nearest softmax value; the largest error of a float32 softmax (of the
    float32-restated scores s32s) against the float64 one."""
    B = s64.shape[1]
    sm = torch.softmax(s64.double(), 1)
    if B == 1:
        thr = 0.5                                                # softmax = 1: any threshold below 1
    else:
        v = sm.reshape(-1).sort().values
        mid = (v[1:] + v[:-1]) / 2
        n_open = (sm[:, None, :] > mid[None, :, None]).sum(2)                   # [2, 2B - 1]
        ok = ((4 * n_open >= B) & (4 * n_open <= 3 * B)).all(0)
        if not bool(ok.any()):
            # a small batch whose two softmaxes do not overlap that far: a quarter to three quarters of the two domains' gates together,
            # each domain with gates of both kinds
            tot = n_open.sum(0)
            ok = (2 * tot >= B) & (2 * tot <= 3 * B) & ((n_open > 0) & (n_open < B)).all(0)
        assert bool(ok.any()), "no threshold leaves gates of both kinds in both domains"
        gaps = torch.where(ok, v[1:] - v[:-1], torch.zeros_like(mid))
        thr = float(mid[int(gaps.argmax())].float())
    gate = sm > thr
    e32 = max(float((torch.softmax(s.float(), 1).double() - sm).abs().max()) for s in s32s)
    return thr, gate, float((sm - thr).abs().min()), e32


# ---------------------------------------------------------------------------- the cases of tests/test_gpu_innercomp.py
FORMS = {"sas": 0, "bert0": 0, "bert1": 1}                       # form -> cross
SCORE_SHAPES = ([(2 + (i % 4), T, D) for i, (T, D) in enumerate((T, D) for T in (1, 15, 16, 17, 50) for D in (32, 64, 128))]
                + [(2, 150, 128)])
SCORE_LDS_MAX = 160 * 1024 - 256


def score_lds(cross, T, D):
    return (2 if cross else 1) * T * (D + 4) * 4


def last_accepted_T(cross, D=128):
    T = 1
    while score_lds(cross, T + 1, D) <= SCORE_LDS_MAX:
        T += 1
    return T


CHAIN_SHAPES = [(1, 1, 64), (7, 20, 32), (8, 3, 128), (9, 20, 64), (255, 5, 64), (256, 20, 128), (257, 20, 64), (600, 16, 128), (33, 50, 256),
                (12, 4, 96), (64, 150, 128)]
FWD_LDS_FLOATS = 16384                                           # ((B + 3) & ~3) + 9 D floats within 64 KiB


def largest_batch(D=128):
    B = FWD_LDS_FLOATS - 9 * D
    assert ((B + 3) & ~3) + 9 * D <= FWD_LDS_FLOATS < ((B + 4) & ~3) + 9 * D
    return B


# (form, B, T, D, nsplit): every shape in the three forms, the SASRec form's partials alternately 1 and 3 and both at 9 and 257 rows; the
# largest batch the forward accepts
CHAIN_CASES = [(form, B, T, D, 3 if (form == "sas" and i % 2) else 1) for form in FORMS for i, (B, T, D) in enumerate(CHAIN_SHAPES)] + \
              [("sas", 9, 20, 64, 1), ("sas", 257, 20, 64, 3)] + [(form, largest_batch(), 1, 128, 1) for form in FORMS]
# (form, Bg, T, D, shard sizes): the worlds of the data-parallel entries
SHARD_CASES = [(form, Bg, 20, 64, sizes) for form in ("sas", "bert0", "bert1")
               for Bg, sizes in ((9, (9,)), (256, (128, 128)), (257, (129, 128)), (9, (3, 3, 3)), (258, (86, 86, 86)))] + \
              [("sas", 256, 20, 128, (128, 128)), ("bert1", 9, 20, 128, (3, 3, 3))]


def shard_ranges(sizes):
    out, lo = [], 0
    for n in sizes:
        out.append((lo, lo + n))
        lo += n
    return tuple(out)


def score_rows(B, T, D, seed):
    """Rows scaled per sample so that the pair-max scores spread over several units: sigma_j in 0.08 .. 0.16 at D = 128, times sqrt(128 / D)."""
    g = torch.Generator().manual_seed(seed)
    sigma = (0.08 + 0.08 * torch.rand(2, B, 1, 1, generator=g)) * (128.0 / D) ** 0.5
    return torch.randn(2, B, T, D, generator=g) * sigma, g


@functools.lru_cache(maxsize=None)
def score_case(cross, B, T, D):
    x, _ = score_rows(B, T, D, 7000 * cross + 1000 * B + 10 * T + D)
    r64 = scores(x.double(), cross)
    r32 = [scores(x, cross, order) for order in ("torch", "index")]
    return x, r64, r32


@functools.lru_cache(maxsize=None)
def case(form, B, T, D, gates="pick", nsplit=1, backward_too=True, sizes=None):
    """Inputs, the threshold and the three references (float64; float32 in torch's order and in index order) of one chained case.  The SASRec
    form's positional partials: nsplit ranges of the batch, or with `sizes` one partial per shard."""
    cross = FORMS[form]
    x, g = score_rows(B, T, D, 31 * (1000 * B + 10 * T + D) + len(form) + cross)
    rn = lambda *shape: torch.randn(*shape, generator=g)      # noqa: E731
    pos = None
    if B >= 4096 and T == 1 and not cross:
        # thousands of random scores leave no gap 100 float32 softmax errors wide (measured: 34): put the scores |e_j|^2 on a ladder with a
        # step in its middle, even rows in 1 .. 1.5, odd rows in 2.5 .. 4
        u = torch.rand(2, B, 1, 1, generator=g)
        target = torch.where((torch.arange(B) % 2 == 0)[None, :, None, None], 1.0 + 0.5 * u, 2.5 + 1.5 * u)
        x = x * torch.sqrt(target / (x * x).sum(-1, keepdim=True))
    if form == "sas":
        pos = 0.1 * rn(2, 2 * T, D)
        x[0, 0, 0, :3] = -pos[0, 0, :3]                          # e = -pos exactly: set bits in tmq
        x[1, B - 1, T - 1, 5] = -pos[1, T - 1, 5]
    sign = lambda t: torch.where(t >= 0, 1.0, -1.0)            # noqa: E731
    b = rn(2, D)
    # w_bs: every third row negative at half the size (other rows in the two domains): both signs from B = 3 on and sum_j w_bs[j] does not
    # cancel
    wsign = torch.stack([torch.where(torch.arange(B) % 3 == 1 + d, -0.5, 1.0) for d in (0, 1)])
    P = dict(wnn=rn(2, D, D) / D ** 0.5,
             bnn=sign(b) * (0.05 + 0.3 * b.abs()),               # non-zero, both signs
             wbs=wsign * (0.02 + torch.rand(2, B, generator=g)) / B ** 0.5,
             bbs=torch.tensor([[0.37], [-0.21]]))
    # the cotangent: random per element with a per-domain mean of about two standard deviations of its batch sum, so that dZ and everything
    # behind it is not the cancellation of its terms
    dx0 = rn(2, B, 2 * T, D) + torch.tensor([2.0, -1.5])[:, None, None, None] / B ** 0.5
    s64 = scores(x.double(), cross)
    s32 = [scores(x, cross, order) for order in ("torch", "index")]
    if gates == "pick":
        thr, gate, margin, e32 = pick_gate(s64, s32)
    else:
        thr = {"open": -1.0, "closed": 1.0}[gates]               # every softmax value is above -1 and (B > 1) below 1
        sm = torch.softmax(s64, 1)
        gate, margin = sm > thr, float((sm - thr).abs().min())
        e32 = max(float((torch.softmax(s, 1).double() - sm).abs().max()) for s in s32)
    dz_parts = None
    if form == "sas":                                            # the embedding backward's positional partials: nsplit ranges of the batch
        cuts = [B * z // nsplit for z in range(nsplit + 1)]
        if sizes:
            nsplit, cuts = len(sizes), [0] + [hi for _, hi in shard_ranges(sizes)]
        dpos_part = torch.stack([dx0[:, cuts[z]:cuts[z + 1]].double().sum(1).float() for z in range(nsplit)])      # [nsplit, 2, 2T, D]
        dz_parts = dpos_part[:, :, T:]
    c = dict(form=form, cross=cross, B=B, T=T, D=D, x=x, P=P, pos=pos, dx0=dx0, thr=thr, gate=gate, margin=margin, e32=e32, s64=s64,
             dpos_part=dpos_part if form == "sas" else None, dz_parts=dz_parts)
    refs = []
    for dtype, order in ((torch.float64, "torch"), (torch.float32, "torch"), (torch.float32, "index")):
        r = forward(x, P, cross, dtype, order, gate=gate, pos=pos)
        if backward_too:
            r.update(backward(x, P, cross, dtype, gate, dx0, order, dz_parts=dz_parts))
        refs.append(r)
    c["ref64"], c["ref32"] = refs[0], refs[1:]
    return c


def ref_case(form, B, T, D, nsplit, sizes):
    """case() under one cache key for the tests and the mutant check."""
    return case(form, B, T, D, "pick", nsplit, True, sizes)


def assert_inputs(c):
    """Conditions on the inputs, before any launch."""
    B = c["B"]
    if c["thr"] not in (-1.0, 1.0) and B >= 2:
        n = [int(c["gate"][g].sum()) for g in (0, 1)]
        assert all(0 < k < B for k in n), (n, B)
        assert all(B <= 4 * k <= 3 * B for k in n) or B <= 2 * sum(n) <= 3 * B, (n, B)       # (pick_gate: the second for small batches)
    for g in (0, 1):
        assert B < 3 or (bool((c["P"]["wbs"][g] > 0).any()) and bool((c["P"]["wbs"][g] < 0).any()))
        assert abs(float(c["P"]["wbs"][g].sum())) > 0.2 * float(c["P"]["wbs"][g].abs().sum())       # sum_j w_bs[j] does not cancel
        assert bool((c["P"]["bnn"][g] > 0).any()) and bool((c["P"]["bnn"][g] < 0).any())
    assert c["margin"] >= 100 * c["e32"], (c["margin"], c["e32"])
    if c["form"] == "sas":
        assert bool((c["ref64"]["tmq"] != 0).any()) and torch.equal(c["ref64"]["tmq"], c["ref32"][0]["tmq"])


TENSORS_FWD = ("sw", "S", "Z")
TENSORS_BWD = ("dZ", "dS", "rows", "dw_nn", "db_nn", "dw_bs", "db_bs", "dxg")


def err(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def bars(c, names):
    """name -> (4 * the larger of the two float32 restatements' errors + 2^-22, the two errors)."""
    out = {}
    for k in names:
        ef = [err(r[k], c["ref64"][k]) for r in c["ref32"]]
        out[k] = (4 * max(ef) + FLOOR, ef)
    return out


def mutant_applies(mutant, c, shards):
    if mutant == "no_diag":
        return c["cross"] == 0 and c["T"] > 1                    # at T = 1 the diagonal is the only pair; cross = 1 takes all T x T pairs
    if mutant == "shard_j0":
        return bool(shards) and len(shards) > 1                  # with one shard j0 = 0
    if mutant == "cross_own":
        return c["cross"] == 1
    if mutant in ("bnn_once", "dwbs_no_b"):
        return True
    raise ValueError(mutant)


@functools.lru_cache(maxsize=None)
def mutants_move_the_outputs(form, B, T, D, sizes=None, nsplit=1):
    """On the float64 reference: each mutant that applies to the case moves at least one output by more than 100 bars (a kernel with that
    mistake cannot pass).  The mutated scores keep the case's gate: the threshold is an input."""
    c = ref_case(form, B, T, D, nsplit, sizes)
    shards = shard_ranges(sizes) if sizes else None
    bar = bars(c, TENSORS_FWD + TENSORS_BWD)
    applied = []
    for mutant in MUTANTS:
        if not mutant_applies(mutant, c, shards):
            continue
        if mutant == "no_diag":
            bs = 4 * max(err(s, c["s64"]) for s in (scores(c["x"], 0, o) for o in ("torch", "index"))) + FLOOR
            moved = {"s": err(scores(c["x"].double(), 0, mutant=mutant), c["s64"]) / bs}
        else:
            m = forward(c["x"], c["P"], c["cross"], torch.float64, gate=c["gate"], pos=c["pos"], mutant=mutant, shards=shards)
            m.update(backward(c["x"], c["P"], c["cross"], torch.float64, c["gate"], c["dx0"], dz_parts=c["dz_parts"], mutant=mutant, shards=shards))
            moved = {k: err(m[k], c["ref64"][k]) / bar[k][0] for k in TENSORS_FWD + TENSORS_BWD if float(c["ref64"][k].abs().max()) > 0}
        k = max(moved, key=moved.get)
        print(f"innercomp {form} B {B} T {T} D {D} mutant {mutant}: moves {k} by {moved[k]:.3e} bars")
        assert moved[k] > 100, (mutant, moved)
        applied.append(mutant)
    return tuple(applied)
