"""amid_amd.optim.Adam -- torch.optim.Adam's place in the reference's own loop, on the engine's lazy Adam -- and the two entry points of
csrc/optim_clip.hip.

Kernel bar, per output tensor (tests/test_gpu_gru.py's): e = max|x - ref64| / max|ref64|; e_kernel <= 4 e_f32 + 2^-22, with e_f32 the same
figure for torch's float32 CPU arithmetic on the same values.  Both figures of every case go to the parity log.
Loop bars: loss 5e-5, parameters 1e-4 absolute (test_reference_training_loop_with_torch_adam), the table relmax < 1e-5
(test_fused_train_step_matches_oracle_and_graph_is_reused), against orc.DenseAdam over every parameter, the table's dense gradient included."""
import math

import pytest
import torch

from oracle import amid_oracle as orc
from tests import gru_ref
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -22
SENT = -12345.625                # guard value: exact in float32, far from every output
GUARD = 64
TABLE = "item_emb_layer.emb_item.weight"
N_DENSE, N_UNIQ = (0, 1, 3, 4, 5, 4099), (0, 1, 8, 9, 257)


@pytest.fixture(scope="module")
def L():
    from amid_amd._lib import lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def step_state(L, seed, step, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8):
    import ctypes
    n = L.value("amid_step_state_bytes")
    host = (ctypes.c_ubyte * n)()
    L.call("amid_step_state_pack", ctypes.addressof(host), seed, step, lr, b1, b2, eps)
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()


def err(x, ref):
    x, ref = torch.as_tensor(x).double().cpu().reshape(-1), torch.as_tensor(ref).double().cpu().reshape(-1)
    if x.numel() == 0:
        return 0.0
    return float((x - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


class Guarded:
    """`n` float32 elements between two guards of SENT; the payload starts on a 256-byte boundary."""

    def __init__(self, values=None, n=None, fill=float("nan")):
        n = int(values.numel()) if values is not None else n
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENT, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        if values is not None:
            self.t.copy_(values.reshape(-1))
        else:
            self.t.fill_(fill)

    def data_ptr(self):
        return self.t.data_ptr()

    def get(self, tag):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.n:] == SENT).all()), f"{tag}: a write outside the buffer"
        return b[GUARD:GUARD + self.n].clone()


# ================================================================================================ the norm kernel
def sqnorm_inputs(n_dense, U, D):
    g = torch.Generator().manual_seed(1000 * n_dense + 10 * U + D)
    dense = torch.randn(n_dense, generator=g) * 10.0 ** float(-2 * torch.rand(1, generator=g))
    rows = torch.full((U + 64, D), float("nan"))              # cap = U + 64: the rows at and beyond U must never be read
    rows[:U] = torch.randn(U, D, generator=g) * torch.logspace(-3, 0, max(U, 1))[:U, None]
    return dense, rows


@pytest.mark.parametrize("D", [64, 128])
def test_grad_sqnorm_matches_float64_and_reruns_bit_for_bit(L, D):
    nb = L.value("amid_grad_sqnorm_workspace_bytes")
    worst = 0.0
    for n_dense in N_DENSE:
        for U in N_UNIQ:
            dense, rows = sqnorm_inputs(n_dense, U, D)
            # the dense list sits in front of NaNs too: a read past n_dense poisons the sum
            gd = Guarded(torch.cat((dense, torch.full(((-n_dense) % 4 + 8,), float("nan")))))
            gr = Guarded(rows)
            nu = torch.tensor([U], dtype=torch.int32, device="cuda")
            outs = []
            for run, junk in enumerate((0.0, 7.5)):              # the workspace carries no state: any content will do
                ws = Guarded(n=nb // 4 + 2, fill=junk)
                out = Guarded(n=1)
                L.call("amid_grad_sqnorm_f32", gd.data_ptr(), n_dense, gr.data_ptr(), nu.data_ptr(), U + 64, D, ws.data_ptr(), out.data_ptr(),
                       stream())
                torch.cuda.synchronize()
                tag = f"sqnorm n {n_dense} U {U} D {D} run {run}"
                w = ws.get(tag)
                assert bool((w[nb // 4:] == junk).all()), f"{tag}: a write past the workspace's stated size"
                outs.append(out.get(tag))
                gd.get(tag), gr.get(tag)
            assert torch.equal(outs[0], outs[1]), f"n {n_dense} U {U}: two runs differ"
            got = float(outs[0][0])
            assert math.isfinite(got), f"n {n_dense} U {U}: {got}"
            vals = torch.cat((dense, rows[:U].reshape(-1)))
            ref = float((vals.double() ** 2).sum())
            f32 = float((vals ** 2).sum())
            if ref == 0.0:
                assert got == 0.0
                continue
            e_k, e_f = abs(got - ref) / ref, abs(f32 - ref) / ref
            worst = max(worst, e_k / max(e_f, 2.0 ** -30))
            log(f"optim sqnorm n_dense {n_dense} U {U} D {D}: e_kernel {e_k:.3e} e_f32 {e_f:.3e}")
            assert e_k <= 4 * e_f + FLOOR, (n_dense, U, D, e_k, e_f)
    log(f"optim sqnorm D {D}: worst e_kernel / e_f32 {worst:.3f}")


# ================================================================================================ the clipped optimizer launch
T_NOW, LR, N_ROWS = 40, 1e-2, 700
NAMES = ("p", "m", "v", "table", "table_m", "table_v")


def opt_state(n_dense, U, D):
    """Dense parameters with moments, a table whose U gradient rows belong to rows of which half lag by 1 .. 5 steps (replay_quad runs)."""
    g = torch.Generator().manual_seed(77 * n_dense + 3 * U + D)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    nd = max(n_dense, 1)
    s = dict(p=r(nd), m=0.1 * r(nd), v=0.01 * r(nd) ** 2, g=r(nd), table=r(N_ROWS, D), table_m=torch.zeros(N_ROWS, D),
             table_v=torch.zeros(N_ROWS, D), last=torch.zeros(N_ROWS, dtype=torch.int32))
    ids = torch.sort(torch.randperm(N_ROWS, generator=g)[:U]).values.int()
    known = torch.randperm(N_ROWS, generator=g)[: N_ROWS // 2]                      # rows that took steps before; the rest: never touched
    s["table_m"][known], s["table_v"][known] = 0.1 * r(known.numel(), D), 0.01 * r(known.numel(), D) ** 2
    s["last"][known] = T_NOW - 1
    lag = ids[::2].long()                                                           # half the step's rows lag by 1 .. 5 steps
    s["table_m"][lag], s["table_v"][lag] = 0.1 * r(lag.numel(), D), 0.01 * r(lag.numel(), D) ** 2
    s["last"][lag] = (T_NOW - 2 - (torch.arange(lag.numel()) % 5)).int()
    cur = ids[1::2].long()
    s["table_m"][cur], s["table_v"][cur] = 0.1 * r(cur.numel(), D), 0.01 * r(cur.numel(), D) ** 2
    s["last"][cur] = T_NOW - 1
    ug = torch.full((U + 64, D), float("nan"))
    ug[:U] = r(U, D)
    s.update(ids=torch.cat((ids, torch.full((64,), -1, dtype=torch.int32))), ug=ug, U=U, n=n_dense, D=D)
    return s


def run_opt(L, s, entry, sq=None, max_norm=None):
    """One launch on guarded copies of the state; returns every output buffer (CPU)."""
    d = {k: Guarded(s[k]) for k in NAMES}
    last = s["last"].cuda()
    gg, ids, ug = Guarded(s["g"]), s["ids"].cuda(), Guarded(s["ug"])
    nu = torch.tensor([s["U"]], dtype=torch.int32, device="cuda")
    st = step_state(L, 3, T_NOW, lr=LR)
    n = s["n"] if entry == "amid_optimizer_step_clip_f32" else max(s["n"], 1)        # (the plain entry refuses n = 0: it steps one stand-in element)
    args = [d["p"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), gg.data_ptr(), n, d["table"].data_ptr(), d["table_m"].data_ptr(),
            d["table_v"].data_ptr(), last.data_ptr(), ids.data_ptr(), nu.data_ptr(), s["U"] + 64, ug.data_ptr(), s["D"], 1.0, st.data_ptr()]
    if entry == "amid_optimizer_step_clip_f32":
        args += [sq.data_ptr(), max_norm]
    L.call(entry, *args, stream())
    torch.cuda.synchronize()
    out = {k: d[k].get(f"{entry} {k}") for k in NAMES}
    out["last"] = last.cpu()
    return out


def adam_restated(s, c, dtype):
    """Clip, replay of the lagging rows' idle steps, Adam step T_NOW -- torch's formulas in `dtype`."""
    b1, b2, eps = 0.9, 0.999, 1e-8
    cv = lambda x: x.to(dtype).clone()      # noqa: E731

    def real(p, m, v, g, t):
        m = m + (1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        p = p - (LR / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
        return p, m, v

    out = {}
    n = s["n"]
    out["p"], out["m"], out["v"] = real(cv(s["p"]), cv(s["m"]), cv(s["v"]), cv(s["g"]) * c, T_NOW)
    if n == 0:
        out["p"], out["m"], out["v"] = cv(s["p"]), cv(s["m"]), cv(s["v"])
    tab, tm, tv = cv(s["table"]), cv(s["table_m"]), cv(s["table_v"])
    for u in range(s["U"]):
        row = int(s["ids"][u])
        p, m, v = tab[row], tm[row], tv[row]
        l = int(s["last"][row])
        if l > 0:
            for t in range(l + 1, T_NOW):
                p, m, v = real(p, m, v, torch.zeros_like(p), t)
        tab[row], tm[row], tv[row] = real(p, m, v, s["ug"][u].to(dtype) * c, T_NOW)
    out.update(table=tab, table_m=tm, table_v=tv)
    return out


@pytest.mark.parametrize("D", [64, 128])
def test_clip_step_with_infinite_max_norm_leaves_the_plain_step_s_bits(L, D):
    for n_dense in N_DENSE:
        for U in N_UNIQ:
            s = opt_state(n_dense, U, D)
            sq = torch.tensor([3.25], device="cuda")
            a = run_opt(L, s, "amid_optimizer_step_f32")
            b = run_opt(L, s, "amid_optimizer_step_clip_f32", sq, float("inf"))
            for k in a:
                if n_dense == 0 and k in ("p", "m", "v"):
                    assert torch.equal(b[k], s[k]), (n_dense, U, k)               # n = 0: the dense buffers are not touched
                else:
                    assert torch.equal(a[k], b[k]), (n_dense, U, k)
            want = s["last"].clone()
            want[s["ids"][:U].long()] = T_NOW
            assert torch.equal(b["last"], want)


@pytest.mark.parametrize("D", [64, 128])
def test_clip_step_with_a_finite_max_norm_matches_float64(L, D):
    worst = {k: 0.0 for k in NAMES}
    for n_dense in N_DENSE:
        for U in N_UNIQ:
            s = opt_state(n_dense, U, D)
            vals = torch.cat((s["g"][:n_dense], s["ug"][:U].reshape(-1)))
            sq64 = float((vals.double() ** 2).sum())
            if sq64 == 0.0:
                continue
            sq = torch.tensor([sq64], dtype=torch.float32)
            max_norm = 0.5 * math.sqrt(sq64)                                       # it bites: c is about one half
            got = run_opt(L, s, "amid_optimizer_step_clip_f32", sq.cuda(), max_norm)
            c64 = min(1.0, max_norm / (math.sqrt(float(sq)) + 1e-6))
            c32 = float(torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (sq.sqrt() + 1e-6), max=1.0))
            ref, f32 = adam_restated(s, c64, torch.float64), adam_restated(s, c32, torch.float32)
            for k in NAMES:
                if n_dense == 0 and k in ("p", "m", "v"):
                    continue
                e_k, e_f = err(got[k], ref[k]), err(f32[k], ref[k])
                worst[k] = max(worst[k], e_k / max(e_f, 2.0 ** -30))
                log(f"optim clip step n_dense {n_dense} U {U} D {D} {k}: e_kernel {e_k:.3e} e_f32 {e_f:.3e}")
                assert e_k <= 4 * e_f + FLOOR, (n_dense, U, D, k, e_k, e_f)
    log(f"optim clip step D {D}: worst e_kernel / e_f32 " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ================================================================================================ the loop
def shifted(b, off, pad):
    """The batch with every real item id moved up by `off` (the pad id and BERT4Rec's masked zeros stay)."""
    out = dict(b)
    for k in ("i_node", "neg_samples", "seq_d1", "seq_d2"):
        v = b[k]
        out[k] = torch.where((v != pad) & (v != 0), v + off, v)
    return out


def touched(b):
    return set(torch.cat([b[k].reshape(-1) for k in ("i_node", "neg_samples", "seq_d1", "seq_d2")]).tolist())


def assert_replay_exercised(batches, need=8):
    """At least `need` table rows are touched, then left alone for two or more steps, then touched again (read off the index tensors)."""
    sets = [touched(b) for b in batches]
    rows = set()
    for t1 in range(len(sets)):
        for t2 in range(t1 + 3, len(sets)):
            idle = set().union(*sets[t1 + 1:t2])
            rows |= (sets[t1] & sets[t2]) - idle
    assert len(rows) >= need, len(rows)


LOW_STEPS = (0, 3, 5)            # these batches draw from the low id range, the others from a disjoint high one


def loop_batches(make, n, off, pad):
    return [b if t in LOW_STEPS else shifted(b, off, pad) for t, b in enumerate(make(t) for t in range(n))]


def dev(b):
    return {k: v.cuda() for k, v in b.items()}


def bce_loss(p1, p2, cu):
    crit = torch.nn.BCELoss(reduction="none")
    m1, m2 = (1 - cu["domain_id"]).unsqueeze(1), cu["domain_id"].unsqueeze(1)
    return torch.mean(crit(p1, cu["label"]) * m1 + crit(p2, cu["label"]) * m2)


def check_params(model, Po, tol=1e-4, table_rel=1e-5, tag=""):
    sd = model.state_dict()
    for k, v in Po.items():
        d = (sd[k].cpu().double() - v.double()).abs()
        if k.endswith("in_proj_bias"):                      # the key bias: a softmax is blind to it, its true gradient is zero, and Adam
            n = v.numel() // 3                              # normalises the rounding noise left in its place to +-lr a step on either side
            d = torch.cat((d[:n], d[2 * n:]))
        if k.endswith("linear_layers.1.bias"):              # ... BERT4Rec's key bias (tests/test_gpu_bert4rec.py _bert_traj leaves it out too)
            continue
        assert float(d.max()) < tol, (tag, k, float(d.max()))
    if table_rel is not None:
        rel = float((sd[TABLE].cpu().double() - Po[TABLE].double()).abs().max() / Po[TABLE].double().abs().max())
        log(f"optim loop {tag}: table relmax {rel:.3e}")
        assert rel < table_rel, (tag, rel)


def verbatim_step(model, optimizer, cu, loss_fn=bce_loss):
    """forward; zero_grad; backward; step -- the reference's order.  Returns (loss, seed, step): the RNG inputs of this forward."""
    outs = model(None, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], None, None)
    seed, step = model.engine.seed, model.engine.step
    loss = loss_fn(*outs, cu)
    optimizer.zero_grad()
    loss.backward()
    assert model.get_parameter(TABLE).grad is None
    return loss, seed, step


def sasrec_model(P, T, lr, seed, cls=None, **kw):
    from amid_amd.model_seq import SASRec
    n_rows, D = P[TABLE].shape
    hid = P["predictModule.fc.0.weight"].shape[0]
    m = (cls or SASRec)(10, D, n_rows, D, T, hid, kw.pop("bs", 4), kw.pop("isInC", False), kw.pop("isItC", False), 0.5, kw.pop("ts2", 0.5),
                        lr=lr, seed=seed, **kw).cuda()
    m.load_state_dict(P)
    return m.train()


SAS = dict(T=20, Bn=8, hid=16, n_items=150)


def sas_batches(n, Bn=8, T=20, n_items=150, seed0=300):
    return loop_batches(lambda t: orc.synthetic_batch(Bn, T, 50, pad_id=n_items - 1, neg=1, seed=seed0 + t), n, 60, n_items - 1)


@pytest.mark.parametrize("D", [64, 128])
def test_reference_loop_sasrec(D):
    from amid_amd.optim import Adam
    T, Bn, hid, n_items, seed = SAS["T"], SAS["Bn"], SAS["hid"], SAS["n_items"], 21
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=2)
    m = sasrec_model(P, T, 5e-4, seed)
    optimizer = Adam(m.parameters(), lr=1e-3)
    Po = {k: v.clone() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=1e-3)
    batches = sas_batches(6)
    assert_replay_exercised(batches)
    for t, batch in enumerate(batches):
        loss, sd, st = verbatim_step(m, optimizer, dev(batch))
        optimizer.step()
        assert st == t + 1
        loss_o = orc.train_step("sasrec", Po, opt_o, batch, orc.philox_masks_sasrec(Bn, T, D, seed=sd, step=st))
        assert abs(loss.item() - loss_o) < 5e-5, t
    check_params(m, Po, tag=f"sasrec D {D}")


def test_reference_loop_bert4rec():
    from amid_amd.model_seq import BERT4Rec
    from amid_amd.optim import Adam
    from tests.test_gpu_bert4rec import batch_with_masked_keys
    T, Bn, hid, n_items, seed = 20, 8, 32, 300, 4242
    P = orc.random_params(orc.bert4rec_param_shapes(n_items, hid), seed=31)
    m = sasrec_model(P, T, 5e-4, seed, cls=BERT4Rec)
    optimizer = Adam(m.parameters(), lr=1e-3)
    Po = {k: v.clone() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=1e-3)
    batches = loop_batches(lambda t: batch_with_masked_keys(Bn, T, 60, seed=100 + t), 6, 100, 0)
    assert_replay_exercised(batches)
    for t, batch in enumerate(batches):
        loss, sd, st = verbatim_step(m, optimizer, dev(batch))
        optimizer.step()
        loss_o = orc.train_step("bert4rec", Po, opt_o, batch, orc.philox_masks_bert4rec(Bn, T, seed=sd, step=st))
        assert abs(loss.item() - loss_o) < 5e-5, t
    check_params(m, Po, tag="bert4rec")


GRU = dict(D=128, T=12, Bn=5, hid=16, n_items=200)


def gru_model(P, lr=5e-4, seed=1):
    from amid_amd.model_gru import GRU4Rec
    m = GRU4Rec(10, GRU["D"], GRU["n_items"], GRU["D"], GRU["T"], GRU["hid"], GRU["Bn"], False, False, 0.5, 0.5, lr=lr, seed=seed).cuda()
    m.load_state_dict(P, strict=True)
    return m.train()


def gru_params(seed=77):
    return orc.random_params(gru_ref.gru4rec_param_shapes(GRU["n_items"], GRU["D"], GRU["hid"]), seed=seed)


def gru_batches(n, seed0=900):
    return loop_batches(lambda t: orc.synthetic_batch(GRU["Bn"], GRU["T"], 50, pad_id=GRU["n_items"] - 1, neg=1, seed=seed0 + t), n, 60,
                        GRU["n_items"] - 1)


def test_reference_loop_gru4rec():
    from amid_amd.optim import Adam
    P = gru_params()
    m = gru_model(P)
    optimizer = Adam(m.parameters(), lr=1e-3)
    Po = {k: v.double() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=1e-3)
    batches = gru_batches(6)
    assert_replay_exercised(batches)
    for t, batch in enumerate(batches):
        loss, _, _ = verbatim_step(m, optimizer, dev(batch))
        optimizer.step()
        loss_o, _, grads = gru_ref.loss_and_grads(Po, batch)
        opt_o.step(Po, grads)
        assert abs(loss.item() - float(loss_o)) < 5e-5, t
    check_params(m, Po, tag="gru4rec")


def test_the_table_gradient_is_never_dense():
    """A 200 000 x 128 table: over a whole step the peak of allocated memory grows by less than half the table's bytes (its dense gradient
    alone would be all of them) and the table's .grad stays None."""
    from amid_amd.model_seq import SASRec
    from amid_amd.optim import Adam
    n_items, D, T, Bn = 200000, 128, 20, 8
    m = SASRec(10, D, n_items, D, T, 16, 4, False, False, 0.5, 0.5, seed=3).cuda().train()
    optimizer = Adam(m.parameters(), lr=1e-3)
    table_bytes = n_items * D * 4
    for t in range(3):
        cu = dev(orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=50 + t))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        verbatim_step(m, optimizer, cu)
        optimizer.step()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        log(f"optim loop memory step {t + 1}: peak grows by {grown / 2 ** 20:.1f} MiB, the table is {table_bytes / 2 ** 20:.1f} MiB")
        assert grown < table_bytes // 2, (t, grown)


def test_a_custom_objective_with_a_penalty_on_a_parameter():
    """A loss the engine has no kernel for: squared error on both outputs + 1e-2 |predictModule.fc.0.weight|^2 on the parameter itself."""
    from amid_amd.optim import Adam
    T, Bn, hid, n_items, D, seed, W = SAS["T"], SAS["Bn"], SAS["hid"], SAS["n_items"], 64, 9, "predictModule.fc.0.weight"
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=6)
    m = sasrec_model(P, T, 5e-4, seed)
    optimizer = Adam(m.parameters(), lr=1e-3)
    Po = {k: v.clone() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=1e-3)

    def objective(p1, p2, y, w):
        return ((p1 - y) ** 2).mean() + ((p2 - y) ** 2).mean() + 1e-2 * (w ** 2).sum()

    for t, batch in enumerate(sas_batches(4, seed0=700)):
        cu = dev(batch)
        loss, sd, st = verbatim_step(m, optimizer, cu, lambda p1, p2, c: objective(p1, p2, c["label"], m.get_parameter(W)))
        for n, p in m.named_parameters():
            assert (p.grad is None) == (n == TABLE), n
        optimizer.step()
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in Po.items()}
        o1, o2 = orc.sasrec_forward(leaves, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"],
                                    orc.philox_masks_sasrec(Bn, T, D, seed=sd, step=st))
        loss_o = objective(o1.squeeze(), o2.squeeze(), batch["label"], leaves[W])
        names = list(leaves)
        gs = torch.autograd.grad(loss_o, [leaves[n] for n in names], allow_unused=True)
        opt_o.step(Po, {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs)})
        assert abs(loss.item() - float(loss_o.detach())) < 5e-5, t
    check_params(m, Po, tol=2e-4, tag="custom objective")          # (test_sasrec_dr_module_reference_loop's bars)


DR_TS2 = 0.15


def dr_batch(t, g, Bn, T, n_items):
    b = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=600 + t)
    b["seq_d1"] = torch.randint(1, 120, (Bn, T), generator=g)
    b["seq_d2"] = torch.randint(120, n_items - 1, (Bn, T), generator=g)
    b["ob_label"] = (torch.rand(Bn, generator=g) < 0.6).long()
    return b


def test_two_optimizers_are_the_reference_s_optimizer_and_optimizer2():
    """train_sr_dr.py's two loops on SASRec(isItC, isDR), verbatim (zero_grad after the forward, which ran under whichever state was live):
    steps A A B B A against two DenseAdam objects (bars: tests/test_gpu_sasrec.py test_dr_two_optimizers_track_oracle)."""
    from amid_amd.optim import Adam
    D, T, Bn, hid, n_items, w, lr, lr2 = 64, 20, 8, 16, 300, 0.1, 1e-3, 0.5
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, itc_bs=Bn, dr=True), seed=77)
    for d in (1, 2):
        P[f"sac{d}.last_layernorm.weight"] *= 0.3
    m = sasrec_model(P, T, lr, 5, bs=Bn, isItC=True, ts2=DR_TS2, isDR=True)
    optimizer, optimizer2 = Adam(m.parameters(), lr=lr), Adam(m.parameters(), lr=lr * lr2)
    Po = {k: v.clone() for k, v in P.items()}
    opts = [orc.DenseAdam(Po, lr=lr), orc.DenseAdam(Po, lr=lr * lr2)]
    g = torch.Generator().manual_seed(1)
    for t, k in enumerate((0, 0, 1, 1, 0)):
        b = dr_batch(t, g, Bn, T, n_items)
        cu = dev(b)
        got = {}

        def objective(*a):
            lc, le, tot, lr_ = orc.dr_losses(a[:6], cu["label"], cu["domain_id"], cu["ob_label"], w)
            got.update(cls=lc, e=le)
            return tot if k == 0 else lr_

        loss, sd, st = verbatim_step(m, (optimizer, optimizer2)[k], cu, objective)
        (optimizer, optimizer2)[k].step()
        taps = {}
        info, _, grads = orc.dr_loss_and_grads(Po, b, "e" if k == 0 else "r", orc.philox_masks_sasrec(Bn, T, D, seed=sd, step=st), dr_e_w=w,
                                               isItC=True, threshold2=DR_TS2, taps=taps)
        for pre in ("itc_d1", "itc_d2"):          # the gate has rows on both sides of the threshold, none of them close to it
            assert 0 < int(taps[pre]["gate"].sum()) < Bn and taps[pre]["margin"] >= 1e-3, (t, pre, taps[pre]["margin"])
        opts[k].step(Po, grads)
        assert abs(float(got["cls"]) - float(info["loss_cls"])) < 5e-5 and abs(float(got["e"]) - float(info["loss_dr_e"])) < 5e-5, t
        assert abs(loss.item() - float(info["loss"])) < 5e-5, t
    assert opts[0].t == 3 and opts[1].t == 2
    check_params(m, Po, tol=3e-4, table_rel=None, tag="two optimizers")


def clipped_oracle(P, batches, max_norm, lr):
    """The float64 trajectory: clip over the dense gradient (torch's formula), then DenseAdam.  Returns (losses, norms, parameters)."""
    Po = {k: v.double() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=lr)
    losses, norms = [], []
    for batch in batches:
        loss_o, _, grads = gru_ref.loss_and_grads(Po, batch)
        norm = math.sqrt(sum(float((g ** 2).sum()) for g in grads.values()))
        c = min(1.0, max_norm / (norm + 1e-6))
        opt_o.step(Po, {k: g * c for k, g in grads.items()})
        losses.append(float(loss_o)); norms.append(norm)
    return losses, norms, Po


CLIP_MAX_NORM = 0.58


def test_clip_grad_norm_includes_the_sparse_rows():
    from amid_amd.optim import Adam
    P = gru_params(seed=78)
    batches = gru_batches(6, seed0=950)
    losses, norms, Po = clipped_oracle(P, batches, CLIP_MAX_NORM, 1e-3)
    log("optim clip: the oracle's gradient norms " + ", ".join(f"{n:.4f}" for n in norms) + f"; max_norm {CLIP_MAX_NORM}")
    assert all(abs(n - CLIP_MAX_NORM) > 0.01 * CLIP_MAX_NORM for n in norms)
    assert sum(n > CLIP_MAX_NORM for n in norms) >= 3 and sum(n < CLIP_MAX_NORM for n in norms) >= 1
    m = gru_model(P)
    optimizer = Adam(m.parameters(), lr=1e-3)
    worst = 0.0
    for t, batch in enumerate(batches):
        loss, _, _ = verbatim_step(m, optimizer, dev(batch))
        total = optimizer.clip_grad_norm_(CLIP_MAX_NORM)
        assert total.dim() == 0 and total.is_cuda
        # the kernel bar on the values the launch summed: the flat dense gradient and the plan's unique rows
        pl = m._last_plan
        U = int(pl.n_uniq.item())
        vals = torch.cat((m._amid_gflat.cpu(), pl.uniq_grad[:U].reshape(-1).cpu()))
        ref, f32 = float((vals.double() ** 2).sum().sqrt()), float((vals ** 2).sum().sqrt())
        e_k, e_f = abs(float(total) - ref) / ref, abs(f32 - ref) / ref
        worst = max(worst, e_k / max(e_f, 2.0 ** -30))
        log(f"optim clip step {t + 1}: norm {float(total):.6f} oracle {norms[t]:.6f} e_kernel {e_k:.3e} e_f32 {e_f:.3e}")
        assert e_k <= 4 * e_f + FLOOR, (t, e_k, e_f)
        assert (float(total) > CLIP_MAX_NORM) == (norms[t] > CLIP_MAX_NORM), t
        optimizer.step()
        assert abs(loss.item() - losses[t]) < 5e-5, t
    log(f"optim clip: worst e_kernel / e_f32 of the returned norm {worst:.3f}")
    check_params(m, Po, tag="clipped gru4rec")


def test_state_dict_resumes_bit_for_bit(tmp_path):
    from amid_amd.optim import Adam
    P = gru_params(seed=79)
    batches = gru_batches(5, seed0=970)

    def steps(m, optimizer, bs):
        for batch in bs:
            verbatim_step(m, optimizer, dev(batch))
            optimizer.step()

    m = gru_model(P)
    optimizer = Adam(m.parameters(), lr=1e-3)
    steps(m, optimizer, batches[:3])
    torch.save(optimizer.state_dict(), tmp_path / "opt.pt")          # (either order: both bring the lazy rows up to date first)
    torch.save(m.state_dict(), tmp_path / "model.pt")
    steps(m, optimizer, batches[3:])
    want, want_opt = {k: v.cpu().clone() for k, v in m.state_dict().items()}, optimizer.state_dict()
    m2 = gru_model(gru_params(seed=5), seed=99)
    optimizer2 = Adam(m2.parameters(), lr=0.5)
    m2.load_state_dict(torch.load(tmp_path / "model.pt", weights_only=True))
    optimizer2.load_state_dict(torch.load(tmp_path / "opt.pt", weights_only=True))
    assert optimizer2.param_groups[0]["lr"] == 1e-3
    steps(m2, optimizer2, batches[3:])
    got, got_opt = m2.state_dict(), optimizer2.state_dict()
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), k
    assert got_opt["state"]["step"] == want_opt["state"]["step"] == 5
    for k in ("m", "v", "table_m", "table_v", "table_last"):
        assert torch.equal(got_opt["state"][k], want_opt["state"][k]), k


def test_lr_scheduler_drives_the_engine_s_lr():
    from amid_amd.optim import Adam
    T, Bn, hid, n_items, D, seed = SAS["T"], SAS["Bn"], SAS["hid"], SAS["n_items"], 64, 13
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=8)
    m = sasrec_model(P, T, 5e-4, seed)
    optimizer = Adam(m.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(optimizer, 2, 0.5)
    Po = {k: v.clone() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=1e-3)
    batches = sas_batches(5, seed0=800)
    assert_replay_exercised(batches[:5], need=1)
    lrs = []
    for t, batch in enumerate(batches):
        loss, sd, st = verbatim_step(m, optimizer, dev(batch))
        opt_o.lr = optimizer.param_groups[0]["lr"]
        lrs.append(opt_o.lr)
        optimizer.step()
        sched.step()
        loss_o = orc.train_step("sasrec", Po, opt_o, batch, orc.philox_masks_sasrec(Bn, T, D, seed=sd, step=st))
        assert abs(loss.item() - loss_o) < 5e-5, t
    assert lrs == [1e-3, 1e-3, 5e-4, 5e-4, 2.5e-4]
    check_params(m, Po, tag="StepLR")


def test_the_loop_and_train_step_share_adam_state_0():
    """train_step() for steps 1-2, the loop for 3-4, train_step() for 5 on one model: one five-step dense-Adam trajectory."""
    from amid_amd.optim import Adam
    T, Bn, hid, n_items, D, seed = SAS["T"], SAS["Bn"], SAS["hid"], SAS["n_items"], 64, 17
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=4)
    m = sasrec_model(P, T, 1e-3, seed)
    optimizer = Adam(m.parameters(), lr=1e-3)
    Po = {k: v.clone() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=1e-3)
    for t, batch in enumerate(sas_batches(5, seed0=850)):
        cu = dev(batch)
        if t in (2, 3):
            loss, sd, st = verbatim_step(m, optimizer, cu)
            optimizer.step()
        else:
            loss = m.train_step(cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
            sd, st = m.engine.seed, m.engine.step
        assert st == t + 1
        loss_o = orc.train_step("sasrec", Po, opt_o, batch, orc.philox_masks_sasrec(Bn, T, D, seed=sd, step=st))
        assert abs(loss.item() - loss_o) < 5e-5, t
    check_params(m, Po, tag="train_step + loop")


def test_what_the_constructor_refuses():
    from amid_amd.optim import Adam
    P = gru_params()
    m, other = gru_model(P), gru_model(P)
    ps = list(m.parameters())
    with pytest.raises(ValueError, match="amid_amd model"):
        Adam(torch.nn.Linear(3, 3).cuda().parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="subset"):
        Adam(ps[1:], lr=1e-3)
    with pytest.raises(ValueError, match="more than one model"):
        Adam(ps + list(other.parameters()), lr=1e-3)
    with pytest.raises(ValueError, match="param groups"):
        Adam([{"params": ps[:1]}, {"params": ps[1:]}], lr=1e-3)
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True), dict(betas=(0.9, 1.5)), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            Adam(ps, lr=1e-3, **kw)
    assert m._amid_optims == []                                     # nothing bound by a refused constructor
    opt = Adam(ps, lr=1e-3, betas=(0.8, 0.99), eps=1e-6)            # the engine's step state carries them
    assert (m.engine.hyper["beta1"], m.engine.hyper["beta2"], m.engine.hyper["eps"], m.engine.hyper["lr"]) == (0.8, 0.99, 1e-6, 1e-3)
    with pytest.raises(ValueError):
        opt.add_param_group({"params": list(other.parameters())})
    with pytest.raises(ValueError, match="2-norm"):
        opt.clip_grad_norm_(1.0, norm_type=1.0)


def test_a_refused_step_leaves_a_model_that_trains():
    from amid_amd.optim import Adam
    T, Bn, hid, n_items, D, seed = SAS["T"], SAS["Bn"], SAS["hid"], SAS["n_items"], 64, 23
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=12)
    m = sasrec_model(P, T, 5e-4, seed)
    optimizer = Adam(m.parameters(), lr=1e-3)
    batch = sas_batches(1, seed0=990)[0]
    cu = dev(batch)
    fwd = lambda: m(None, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], None, None)      # noqa: E731
    with pytest.raises(RuntimeError, match="exactly one training-mode forward and backward"):
        optimizer.step()                                            # nothing happened at all
    fwd()
    with pytest.raises(RuntimeError, match="without a backward"):
        optimizer.step()
    fwd()
    p1, p2 = fwd()
    optimizer.zero_grad()
    bce_loss(p1, p2, cu).backward()
    with pytest.raises(RuntimeError, match="2 training-mode forwards"):
        optimizer.step()
    m.eval()
    p1, p2 = fwd()
    bce_loss(p1, p2, cu).backward()
    with pytest.raises(RuntimeError, match="exactly one training-mode forward and backward"):
        optimizer.step()                                            # an eval-mode forward bumps no counter
    m.train()
    p1, p2 = fwd()
    optimizer.zero_grad()
    (bce_loss(p1, p2, cu) + 1e-3 * (m.get_parameter(TABLE) ** 2).sum()).backward()
    with pytest.raises(ValueError, match="outside the model"):
        optimizer.step()
    assert m.get_parameter(TABLE).grad is None and m.engine.step == 0
    sd = m.state_dict()
    for k, v in P.items():
        assert torch.equal(sd[k].cpu(), v), k                       # no refusal moved a parameter
    # one good step
    Po = {k: v.clone() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=1e-3)
    loss, s0, st = verbatim_step(m, optimizer, cu)
    assert st == 1
    optimizer.step()
    loss_o = orc.train_step("sasrec", Po, opt_o, batch, orc.philox_masks_sasrec(Bn, T, D, seed=s0, step=st))
    assert abs(loss.item() - loss_o) < 5e-5
    check_params(m, Po, tag="after refusals")
    # gradient accumulation: the second backward of one forward is refused; the first one's step still goes through
    outs = fwd()
    s0, st = m.engine.seed, m.engine.step
    loss = bce_loss(*outs, cu)
    optimizer.zero_grad()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
    optimizer.step()
    loss_o = orc.train_step("sasrec", Po, opt_o, batch, orc.philox_masks_sasrec(Bn, T, D, seed=s0, step=st))
    assert st == 2 and abs(loss.item() - loss_o) < 5e-5
    check_params(m, Po, tag="after a refused second backward")
