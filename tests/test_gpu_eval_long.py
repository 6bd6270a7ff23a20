"""The fused evaluation batch beyond 64 tokens (SasrecEngine._enqueue_eval_encoders_long: plain SASRec, isDR, isItC; fp32, D 128,
64 < T <= 256): the long attention core over a live list, the inference forms of the strip launches and layer 0's gathering q / k / v strip,
each against the launch it restates, bit for bit; the whole batch against the launches it replaces (enqueue_forward over both domains with the
candidates gathered by K1 + amid_positive_rank_f32), against the oracle, through the captured graph, through train_sr.test() and downstream
in full_ranks / recommend; and the shapes that stay on enqueue_forward."""
import argparse

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc
from tests.test_gpu_eval import FIX, _write_csv, eval_batch, make_engine, old_path

pytestmark = pytest.mark.gpu
H = 8


def _lib():
    from amid_amd._lib import lib
    return lib()


def live_list(domain):
    """amid_live_list_i32 of a batch's domain ids: [B + 1] int32 on the device."""
    B = domain.numel()
    live = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    _lib().call("amid_live_list_i32", domain.cuda().to(torch.int64).data_ptr(), B, live.data_ptr(), None)
    torch.cuda.synchronize()
    return live


# ---------------------------------------------------------------------------- 1. the attention core alone
@pytest.mark.parametrize("T", [65, 128, 150, 256])
def test_long_live_attention_rows_are_the_full_launchs_bits(T):
    B, D = 3, 128
    g = torch.Generator().manual_seed(T)
    q, k, v = (torch.randn(2 * B * T, D, generator=g).cuda() for _ in range(3))
    L = _lib()
    ref = torch.zeros(2 * B * T, D, device="cuda")
    L.call("amid_attn_fwd_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), None, B, T, D, H, 1, 0, None, 0, 0.5, ref.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    ref = ref.view(2, B, T, D)
    for name, dom in (("mixed", [0, 1, 0]), ("all of domain 0", [0, 0, 0]), ("all of domain 1", [1, 1, 1]), ("null", None)):
        out = torch.full((2, B, T, D), -7.25, device="cuda")           # the sentinel the other sequences' rows must keep
        lv = None if dom is None else live_list(torch.tensor(dom))
        L.call("amid_attn_fwd_long_live_infer_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, T, D, H, out.data_ptr(),
               None if lv is None else lv.data_ptr(), None)
        torch.cuda.synchronize()
        for gd in (0, 1):
            for b in range(B):
                if dom is None or dom[b] == gd:
                    assert torch.equal(out[gd, b], ref[gd, b]), (name, gd, b, float((out[gd, b] - ref[gd, b]).abs().max()))
                else:
                    assert bool((out[gd, b] == -7.25).all()), (name, gd, b)


# ---------------------------------------------------------------------------- 2. the strips
@pytest.mark.parametrize("T", [65, 150])          # 65: the last 64-row tile of a domain holds one row of a sequence
def test_inference_strips_against_the_saving_strips(T):
    from amid_amd.plan import SASREC_LN_EPS, SASREC_P_DROP
    B, D, hid, NI, n_items = 3, 128, 32, 5, 3000
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=3 + D + T)
    # exact zeros in table[id] + pos[t]: the pad row and one position row of each domain are zero, so a padded slot there is masked
    P["item_emb_layer.emb_item.weight"][n_items - 1] = 0.0
    P["sac1.pos_emb.weight"][1] = 0.0
    P["sac2.pos_emb.weight"][T - 60] = 0.0
    eng = make_engine(P, n_items, D, T, hid)
    pl = eng.plan(B, T, NI, need_grad=False)
    L, s, st = _lib(), eng.s, eng.step_state.data_ptr()
    pos = (eng.dense.ptr("sac1.pos_emb.weight"), eng.dense.ptr("sac2.pos_emb.weight"))
    lay = lambda l, names: tuple(eng._pp("sac{d}." + n.replace("#", str(l))) for n in names)      # noqa: E731
    qkv_n = ("attention_layernorms.#.weight", "attention_layernorms.#.bias", "attention_layers.#.in_proj_weight", "attention_layers.#.in_proj_bias")
    rest_n = ("attention_layers.#.out_proj.weight", "attention_layers.#.out_proj.bias", "forward_layernorms.#.weight", "forward_layernorms.#.bias",
              "forward_layers.#.conv1.weight", "forward_layers.#.conv1.bias", "forward_layers.#.conv2.weight", "forward_layers.#.conv2.bias")
    masked = 0
    for seed, null_list in ((40, False), (41, False), (42, False), (42, True)):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, n_items, NI, seed).items()}
        torch.cuda.synchronize()
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        L.call("amid_pack_indices_live", pl.in_i_node.data_ptr(), pl.in_neg.data_ptr(), pl.in_seq_d1.data_ptr(), pl.in_seq_d2.data_ptr(),
               B, T, NI - 1, eng.n_rows, pl.idx_all.data_ptr(), pl.err.data_ptr(), None, pl.domain.data_ptr(), pl.live.data_ptr(), s)
        lf = None if null_list else pl.live.data_ptr()
        f = lambda: torch.full((2 * B * T, D), -7.25, device="cuda")      # noqa: E731
        with torch.cuda.stream(eng.stream):
            sv = {n: f() for n in ("x0", "qn0", "q0", "k0", "v0", "o0", "r0", "y0", "h0", "x1", "qn1", "q1", "k1", "v1", "o1", "r1", "y1", "h1", "x2")}
            nf = {n: f() for n in ("qn0", "q0", "k0", "v0", "qn1", "q1", "k1", "v1", "x2")}
            tm_s = torch.full((2 * B * T, D // 4), 0x55, dtype=torch.uint8, device="cuda")
            tm_n = tm_s.clone()
        p = lambda d, *ns: tuple(d[n].data_ptr() for n in ns)      # noqa: E731
        # ---- the saving launches: K1, q / k / v, [the attention core], out-projection / feed-forward (+ layer 1's q / k / v)
        if null_list:
            L.call("amid_embed_fwd_f32", eng.table.data_ptr(), pl.idx_all.data_ptr(), *pos, B, T, D, 0, sv["x0"].data_ptr(), tm_s.data_ptr(), st, 0,
                   SASREC_P_DROP, s)
        else:
            L.call("amid_embed_fwd_live_f32", eng.table.data_ptr(), pl.idx_all.data_ptr(), *pos, B, T, D, 0, sv["x0"].data_ptr(), tm_s.data_ptr(), st, 0,
                   SASREC_P_DROP, lf, s)
        L.call("amid_sas_strip_qkv_fwd_f32", sv["x0"].data_ptr(), *lay(0, qkv_n), SASREC_LN_EPS, B, T, D, lf, *p(sv, "qn0", "q0", "k0", "v0"), s)
        L.call("amid_attn_fwd_long_live_infer_f32", *p(sv, "q0", "k0", "v0"), B, T, D, H, sv["o0"].data_ptr(), lf, s)
        L.call("amid_sas_strip_oproj_ffn_fwd_f32", *p(sv, "o0", "qn0"), *lay(0, rest_n), tm_s.data_ptr(), SASREC_LN_EPS, B, T, D, lf, 0, st, 0,
               SASREC_P_DROP, *p(sv, "r0", "y0", "h0", "x1"), *lay(1, qkv_n), *p(sv, "qn1", "q1", "k1", "v1"), s)
        L.call("amid_attn_fwd_long_live_infer_f32", *p(sv, "q1", "k1", "v1"), B, T, D, H, sv["o1"].data_ptr(), lf, s)
        L.call("amid_sas_strip_oproj_ffn_fwd_f32", *p(sv, "o1", "qn1"), *lay(1, rest_n), tm_s.data_ptr(), SASREC_LN_EPS, B, T, D, lf, 1, st, 0,
               SASREC_P_DROP, *p(sv, "r1", "y1", "h1", "x2"), *([None] * 8), s)
        # ---- the inference forms, each on the saving launches' inputs
        L.call("amid_sas_strip_qkv_fwd_gather_infer_f32", eng.table.data_ptr(), pl.idx_all.data_ptr(), *pos, *lay(0, qkv_n), SASREC_LN_EPS, B, T, D,
               lf, tm_n.data_ptr(), *p(nf, "qn0", "q0", "k0", "v0"), s)
        L.call("amid_sas_strip_oproj_ffn_fwd_infer_f32", *p(sv, "o0", "qn0"), *lay(0, rest_n), tm_s.data_ptr(), SASREC_LN_EPS, B, T, D, lf, None,
               *lay(1, qkv_n), *p(nf, "qn1", "q1", "k1", "v1"), s)
        L.call("amid_sas_strip_oproj_ffn_fwd_infer_f32", *p(sv, "o1", "qn1"), *lay(1, rest_n), tm_s.data_ptr(), SASREC_LN_EPS, B, T, D, lf,
               nf["x2"].data_ptr(), *([None] * 8), s)
        eng.sync()
        eng.check_index_error(pl)
        torch.cuda.synchronize()
        dom = cu["domain_id"].tolist()
        # every buffer started from the same sentinel: equality of the whole tensors also says the same rows were written
        for n in nf:
            assert torch.equal(nf[n], sv[n]), (seed, null_list, n, float((nf[n] - sv[n]).abs().max()))
        assert torch.equal(tm_n, tm_s), (seed, null_list)
        x2 = sv["x2"].view(2, B, T, D)
        for gd in (0, 1):
            for b in range(B):
                live = null_list or dom[b] == gd
                assert bool((x2[gd, b] == -7.25).all()) != live, (seed, gd, b)
                if live:
                    assert bool(torch.isfinite(x2[gd, b]).all())
                    masked += int((tm_s.view(2, B, T, D // 4)[gd, b] == 0x0F).sum())
    assert masked > 0          # the "== 0" bytes were exercised


def poison(pl):
    """What the old path left in the plan's encoder buffers would equal what the new launches are to write there: overwrite it, so that a launch
    that wrote nothing cannot pass."""
    for t in (*pl.qn, *pl.q, *pl.k, *pl.v, *pl.o, pl.x[1], pl.x[2], pl.u):
        t.fill_(float("nan"))
    pl.tmq.fill_(0xFF)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 3. end to end against the launches replaced
CASES = [(128, 32, 65, 3, 5), (128, 32, 80, 7, 200), (128, 32, 150, 8, 1000), (128, 64, 150, 3, 5), (128, 32, 256, 2, 5)]


@pytest.mark.parametrize("D,hid,T,B,NI", CASES)
def test_eval_launches_are_bit_identical_to_the_forward_and_rank_kernels(D, hid, T, B, NI):
    n_items = 3000
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=3 + D + T)
    eng = make_engine(P, n_items, D, T, hid)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl)
    for seed in (40, 41, 42):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, n_items, NI, seed, dup_positive=NI > 4).items()}
        torch.cuda.synchronize()          # (the engine's stream does not wait for torch's)
        own, r, r0 = old_path(eng, pl, cu)
        poison(pl)
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
        eng.sync()
        eng.check_index_error(pl)
        print(f"T {T} B {B} NI {NI} seed {seed}: domains {cu['domain_id'].tolist()} max |ev_p - own| {float((pl.ev_p - own).abs().max()):.3e} "
              f"rank diffs {int((pl.ev_rank != r).sum())} raw {int((pl.ev_rank_raw != r0).sum())}")
        assert torch.equal(pl.ev_p, own), float((pl.ev_p - own).abs().max())
        assert torch.equal(pl.ev_rank, r) and torch.equal(pl.ev_rank_raw, r0)
        if NI > 4:                      # the tie rule: a row whose positive repeats among the negatives loses (at least) one more rank with fix_value
            assert bool((pl.ev_rank[::2] >= pl.ev_rank_raw[::2] + 1).all()) and bool((pl.ev_rank >= pl.ev_rank_raw).all())
            ties = (own[:, 1:] == own[:, :1]).sum(1).int()           # (the draw can repeat the positive's id, or another row of equal score)
            assert bool((pl.ev_rank - pl.ev_rank_raw >= ties).all())
        y = cu["label"]
        want = torch.nn.functional.binary_cross_entropy(own.double(), y.double(), reduction="none").sum(1) / (B * NI)      # train_sr.py:63-64
        assert float((pl.ev_loss_part.double() - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-9


# ---------------------------------------------------------------------------- 4. against the oracle
def test_eval_scores_at_150_tokens_against_the_oracle():
    """The first batch of the (150, 8, 1000) case against the CPU restatement of model_seq.py:416-443 in eval mode: fp32 logits within 1e-4
    relative; the launches replaced are held to the same bar.  Both maxima are printed (they belong in
    profiles/eval_long.md)."""
    D, hid, T, B, NI, n_items = 128, 32, 150, 8, 1000, 3000
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=3 + D + T)
    b = eval_batch(B, T, n_items, NI, 40, dup_positive=True)
    with torch.no_grad():
        p1, p2 = orc.sasrec_forward(P, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"])
    want = torch.where(b["domain_id"][:, None] != 0, p2.reshape(B, -1), p1.reshape(B, -1)).double()
    eng = make_engine(P, n_items, D, T, hid)
    pl = eng.plan(B, T, NI, need_grad=False)
    cu = {k: v.cuda() for k, v in b.items()}
    torch.cuda.synchronize()
    own, _, _ = old_path(eng, pl, cu)
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
    eng.enqueue_eval(pl, FIX, want_scores=True)
    eng.sync()
    rel = lambda got: float(((got.cpu().double() - want).abs() / want.abs().clamp_min(1e-30)).max())      # noqa: E731
    relmax = lambda got: float((got.cpu().double() - want).abs().max() / want.abs().max())                 # noqa: E731
    print(f"T 150 oracle: fused  max rel {rel(pl.ev_p):.3e} (per element) {relmax(pl.ev_p):.3e} (of the largest score)")
    print(f"T 150 oracle: forward max rel {rel(own):.3e} (per element) {relmax(own):.3e} (of the largest score)")
    assert rel(pl.ev_p) < 1e-4
    assert rel(own) < 1e-4


# ---------------------------------------------------------------------------- 5. the captured graph
def test_eval_epoch_graph_equals_eager_at_150_tokens():
    D, hid, T, B, NI, n_items = 128, 32, 150, 8, 50, 3000
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=3 + D + T)
    eng = make_engine(P, n_items, D, T, hid)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl)
    cus = [{k: v.cuda() for k, v in eval_batch(B, T, n_items, NI, 900 + i).items()} for i in range(3)]
    torch.cuda.synchronize()
    packed = torch.stack([eng.pack_batch(pl, c["i_node"], c["neg_samples"], c["seq_d1"], c["seq_d2"], c["label"], c["domain_id"]) for c in cus])
    out_g = eng.eval_epoch(pl, packed, FIX, with_loss=True, use_graph=True)
    eng.sync()
    assert (FIX, True) in pl.eval_graphs
    out_e = eng.eval_epoch(pl, packed, FIX, with_loss=True, use_graph=False)
    eng.sync()
    assert torch.equal(out_g, out_e)
    assert int(out_g[:, :B].max()) > 0
    for i, c in enumerate(cus):
        own, r, r0 = old_path(eng, pl, c)
        assert torch.equal(out_g[i, :B], r) and torch.equal(out_g[i, B:2 * B], r0), i


# ---------------------------------------------------------------------------- 6. isDR and isItC
@pytest.mark.parametrize("variant,T,B,NI", [("dr", 70, 4, 9), ("itc", 70, 32, 9)])
def test_variants_are_bit_identical_to_their_forward_and_rank_path(variant, T, B, NI):
    """isDR: the plain model's launches + its own LN / mean launch and the head on that vector.  isItC: a null live list (both domains of every
    row), the pair-max launch, the mix folded into the head (32 rows)."""
    from tests import test_gpu_eval_variants as tv
    D, hid, n_items = 128, 32, 3000
    P = orc.random_params(tv.shapes_of(variant, n_items, D, T, hid, B), seed=3 + D + T)
    eng = tv.make_engine(variant, P, n_items, D, T, hid, B, ts1=1.0 / B, ts2=1.0 / B)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl)
    for seed in (40, 41):
        cu = {k: v.cuda() for k, v in tv.eval_batch(B, T, n_items, NI, seed, dup_positive=True).items()}
        torch.cuda.synchronize()
        own, r, r0, u_own = tv.old_path(eng, pl, cu)
        poison(pl)
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
        eng.sync()
        eng.check_index_error(pl)
        print(f"{variant} seed {seed}: max |ev_p - own| {float((pl.ev_p - own).abs().max()):.3e}, max |ev_u - u| {float((pl.ev_u - u_own).abs().max()):.3e}")
        assert torch.equal(pl.ev_u, u_own)
        assert torch.equal(pl.ev_p, own), float((pl.ev_p - own).abs().max())
        assert torch.equal(pl.ev_rank, r) and torch.equal(pl.ev_rank_raw, r0)
        assert tv.loss_close(pl.ev_loss_part, own, cu["label"], B, NI)


# ---------------------------------------------------------------------------- 7. what users see
def _toy(tmp_path, n_users, neg, lo1, hi1, lo2, hi2, pad):
    from amid_amd.dataset_seq import DualDomainSeqDataset
    rng = np.random.default_rng(5)
    _write_csv(tmp_path / "toy_test.csv", n_users, rng, lo1, hi1, lo2, hi2)
    return DualDomainSeqDataset(seq_len=70, isTrain=False, neg_nums=neg, long_length=7, pad_id=pad, seed=3, csv_path=str(tmp_path / "toy_test.csv"))


def test_train_sr_test_at_70_tokens_gives_the_same_metrics_either_way(tmp_path):
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches
    from amid_amd.train_sr import test
    ds = _toy(tmp_path, 96, 99, 1, 400, 400, 900, 1001)
    model = model_seq.SASRec(10, 128, 1100, 128, 70, 32, 32, False, False, 0.5, 0.5, seed=2)
    args = argparse.Namespace(overlap=True)
    res, fused_results = {}, {}
    inner = model.eval_ranks
    for long in (True, False):
        model.engine.EVAL_LONG = long
        calls = []
        model.eval_ranks = lambda ep, fix, _c=calls: _c.append(inner(ep, fix)) or _c[-1]
        vb = DeviceBatches(ds, 32, shuffle=False, device="cuda:0", seed=9)
        res[long] = test(model, args, vb)
        fused_results[long] = calls
    assert len(fused_results[True]) == 1 and fused_results[True][0] is not None          # test() asked eval_ranks and got ranks
    assert len(fused_results[False]) == 1 and fused_results[False][0] is None            # ... and without the switch went through forward()
    assert set(res[True]) == set(res[False])
    for k, v in res[False].items():
        if k == "loss":
            assert abs(res[True][k] - v) <= 1e-6 * abs(v)
        else:
            assert res[True][k] == v or all(np.isnan(a) and np.isnan(b) or a == b for a, b in zip(res[True][k], v)), k


def test_full_ranks_and_recommend_at_70_tokens(tmp_path):
    """full_ranks / recommend take their user vectors from enqueue_user_vectors, which follows eval_fused_ok: the ranks recounted from the
    kernels' own scores (recommend over the whole table, history kept), rank_full >= rank_sampled, and neither depends on the switch."""
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches
    n_items, bs, neg = 120, 32, 30
    ds = _toy(tmp_path, 64, neg, 1, 60, 60, 119, 119)
    model = model_seq.SASRec(10, 128, n_items, 128, 70, 32, bs, False, False, 0.5, 0.5, seed=2)
    model.eval()
    res = {}
    for long in (True, False):
        model.engine.EVAL_LONG = long
        vb = DeviceBatches(ds, bs, shuffle=False, device="cuda:0", seed=9)
        ep = vb.epoch_tensors()
        pl = model.engine.plan(bs, 70, 1 + neg, need_grad=False)
        assert model.engine.eval_fused_ok(pl) == long
        sampled = model.eval_ranks(ep, FIX)
        assert (sampled is not None) == long
        fr = model.full_ranks(ep, vb, FIX)
        ids, sc = model.recommend(ep["seq_d1"][0], ep["seq_d2"][0], ep["domain_id"][0], k=n_items, exclude_history=False)
        torch.cuda.synchronize()
        res[long] = (fr["rank"].clone(), fr["rank_raw"].clone(), ids.clone(), sc.clone())
        if not long:
            continue
        assert bool((fr["rank"] >= sampled["rank"]).all()) and bool((fr["rank_raw"] >= sampled["rank_raw"]).all())
        assert int(fr["rank"].max()) > 0
        # batch 0's full ranks recounted on the host from recommend's scores of every table row
        ids_c, sc_c = ids.cpu(), sc.cpu()
        dom, pos = ep["domain_id"][0].cpu(), ep["i_node"][0].cpu()
        for b in range(bs):
            assert sorted(ids_c[b].tolist()) == list(range(n_items))
            score = torch.empty(n_items)
            score[ids_c[b]] = sc_c[b]
            cand = sorted(set(ds.pool[int(dom[b])].tolist()) - set(ds.own_items[b].tolist()))
            cs = score[torch.tensor(cand, dtype=torch.long)]
            assert int((cs > score[int(pos[b])] - torch.tensor(FIX, dtype=torch.float32)).sum()) == int(fr["rank"][0, b]), b
            assert int((cs > score[int(pos[b])]).sum()) == int(fr["rank_raw"][0, b]), b
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- 8. staying out
@pytest.mark.parametrize("D,hid,T,compute", [(64, 16, 100, "f32"), (128, 32, 300, "f32"), (128, 32, 100, "bf16")])
def test_shapes_that_keep_enqueue_forward(D, hid, T, compute):
    n_items, B, NI = 300, 4, 5
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=1)
    eng = make_engine(P, n_items, D, T, hid, compute)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert not eng.eval_fused_ok(pl)
    with pytest.raises(ValueError):
        eng.enqueue_eval(pl, FIX)
    eng.sync()
