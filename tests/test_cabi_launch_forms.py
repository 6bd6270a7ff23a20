"""CPU-side pin of the argument checks of the sequence and strip entry points (csrc/sasrec_seq.hip, sasrec_strip.hip, sasrec_strip_px.hip,
bert_strip.hip, bert_seq_infer.hip): every code below is decided before the entry point touches a device, and every expected code is a
literal recorded from the library as it stood BEFORE the entries were moved onto call records (csrc/host_launch.h) -- the rewrite has to
answer the same.  Arguments are bound by the header's parameter names; no case here passes every check (that call would launch).

Not pinned, because the entry reads before it checks (left as it is): amid_sas_strip_qkv_fwd_f32, amid_sas_strip_oproj_ffn_fwd_f32, the
amid_sas_strip_*_bwd_* entries and every amid_bert_strip_* entry copy ln_w[g], w_in[g], ... of a non-null family without looking at the
two pointers, so "a family with one domain's pointer missing" has no answer there; the tr_* arrays of amid_bert_strip_qkv_fwd_pro*_f32
are read up to n_tr entries unchecked for length."""
import ctypes
import re

import pytest

from amid_amd import _lib

ARG, UNSUPPORTED = -1, -2

_FLOATS = (ctypes.c_float * 4096)()                  # (16-byte aligned: the scorer entry checks that; also stands in for a packed sort plan)
_INTS = (ctypes.c_int * 64)(*([64] * 64))
P = ctypes.cast(_FLOATS, ctypes.c_void_p)
IP = ctypes.cast(_INTS, ctypes.c_void_p)
FAM = (ctypes.c_void_p * 12)(*([P.value] * 12))      # a family: up to [3][2][2] device pointers
HALF = (ctypes.c_void_p * 12)(P.value, None, P.value, None, P.value, None, P.value, None, P.value, None, P.value, None)   # domain 1 missing
HOLE = HALF                                           # as a saved-tensor family ([layer]): layer 1's entry missing

INT_DEFAULTS = dict(n_layers=2, B=3, T=20, D=128, H=8, train=0, NI=2, hid=32, layer=0, flayer=0, sort_phase=0, mma_bf16=0, n_keys=0, n_tr=0,
                    zero_dead=0, n_rows=100)


def _params(entry):
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % entry, text, flags=re.S)
    out = []
    for a in m.group(1).split(","):
        mm = re.match(r"^(.*?)([A-Za-z_]\w*)$", a.strip(), flags=re.S)
        out.append((re.sub(r"\s+", " ", mm.group(1)).strip(), mm.group(2)))
    return out


class Form:
    """An entry point with an argument set that passes every pointer check; call(**over) replaces arguments by name."""

    def __init__(self, entry, **base):
        self.entry, self.f, self.params = entry, _lib.lib()._fn[entry], _params(entry)
        self.names = [n for _, n in self.params]
        self.good = {}
        for decl, n in self.params:
            if decl.count("*") == 2:
                self.good[n] = FAM
            elif "*" in decl:
                self.good[n] = None if n == "stream" else IP if "int" in decl or "long long" in decl else P
            elif decl == "float":
                self.good[n] = 0.5 if "drop" in n else 1e-8
            else:
                self.good[n] = INT_DEFAULTS[n]
        self.set(**base)

    def set(self, **over):
        for n in over:
            assert n in self.good, (self.entry, n)
        self.good.update(over)

    def call(self, **over):
        for n in over:
            assert n in self.good, (self.entry, n)
        return self.f(*[over.get(n, self.good[n]) for n in self.names])

    def pointers(self, families=None):
        return [n for d, n in self.params if "*" in d and n != "stream" and (families is None or (d.count("*") == 2) == families)]

    def all_null(self):
        return self.call(**{n: None for n in self.pointers()})

    def each_null(self, names, code=ARG, **over):
        for n in names:
            assert self.call(**{**over, n: None}) == code, (self.entry, n)

    def each(self, cases, **over):
        for change, code in cases:
            assert self.call(**{**over, **change}) == code, (self.entry, change)


# ---- csrc/sasrec_seq.hip: the eleven one-launch forwards ------------------------------------------------------------------------------
PARAM_FAMILIES = ["ln1_w", "ln1_b", "w_in", "b_in", "w_o", "b_o", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2"]
# (no parameter of its own makes the shape bad: the shape query answers for all of them, behind the pointer checks)
SEQ_SHAPES = [(dict(B=0), UNSUPPORTED), (dict(B=-3), UNSUPPORTED), (dict(T=0), UNSUPPORTED), (dict(T=-1), UNSUPPORTED), (dict(T=65), UNSUPPORTED),
              (dict(D=0), UNSUPPORTED), (dict(D=-128), UNSUPPORTED), (dict(D=96), UNSUPPORTED), (dict(D=256), UNSUPPORTED), (dict(H=4), UNSUPPORTED),
              (dict(H=0), UNSUPPORTED), (dict(B=1 << 20, T=64), UNSUPPORTED), (dict(n_layers=0), ARG), (dict(n_layers=3), ARG),
              (dict(n_layers=-1), ARG)]
SAVED9 = ["qn", "q", "k", "v", "o", "stats", "r", "y", "h"]
SAVED7 = ["ln_stat", "q", "k", "v", "o", "stats", "r", "h"]


@pytest.mark.parametrize("entry", ["amid_sas_seq_fwd_f32", "amid_sas_seq_fwd_bf16w_f32", "amid_sas_seq_fwd_split_f32"])
def test_the_nine_tensor_forwards(entry):
    c = Form(entry)
    assert c.all_null() == ARG
    c.each_null(["x_in", "xout"] + PARAM_FAMILIES + SAVED9 + [n for n in ("w16", "w16x3") if n in c.names])
    c.each(SEQ_SHAPES)
    c.each([({n: HALF}, ARG) for n in PARAM_FAMILIES] + [({n: HOLE}, ARG) for n in ["x_in"] + SAVED9])
    c.each([(dict(train=1, step_state=None), ARG), (dict(train=1, step_state=None, p_drop=0.0), ARG)])
    # neither tmq nor the live list is required; with one layer the second layer's entries are not read
    c.each([(dict(tmq=None, live=None, D=96), UNSUPPORTED), (dict(n_layers=1, q=HOLE, D=96), UNSUPPORTED)])


def test_the_seven_tensor_forward():
    c = Form("amid_sas_seq_fwd_split_lnstat_f32")
    assert c.all_null() == ARG
    c.each_null(["x_in", "xout", "w16x3"] + PARAM_FAMILIES + SAVED7)
    c.each(SEQ_SHAPES + [(dict(D=64), UNSUPPORTED)])                            # (the row statistics: the pieces build, D 128)
    c.each([({n: HALF}, ARG) for n in PARAM_FAMILIES] + [({n: HOLE}, ARG) for n in ["x_in"] + SAVED7])
    c.each([(dict(train=1, step_state=None), ARG)])


def test_the_inference_forward():
    c = Form("amid_sas_seq_fwd_split_infer_f32")
    assert c.all_null() == ARG
    c.each_null(["x0", "xout", "w16x3"] + PARAM_FAMILIES)
    c.each(SEQ_SHAPES + [(dict(D=64), UNSUPPORTED)])
    c.each([({n: HALF}, ARG) for n in PARAM_FAMILIES])


HEAD_PTRS = ["last_ln_w", "last_ln_b", "items", "sw1", "sb1", "sw2", "sb2", "labels", "domain_id", "u", "p1", "p2", "dp1", "dp2", "loss_part", "dx",
             "ditems", "ln_part", "hidg"]
HEAD_SHAPES = [(dict(NI=0), ARG), (dict(NI=-2), ARG), (dict(NI=65), ARG), (dict(hid=0), ARG), (dict(hid=-4), ARG), (dict(hid=30), ARG),
               (dict(hid=68), ARG), (dict(B=0), ARG), (dict(T=0), ARG), (dict(D=0), ARG), (dict(D=80), ARG), (dict(D=256), ARG),
               (dict(D=96), UNSUPPORTED), (dict(D=64), UNSUPPORTED), (dict(T=65), UNSUPPORTED), (dict(T=12), UNSUPPORTED), (dict(H=4), UNSUPPORTED),
               (dict(n_layers=0), ARG), (dict(n_layers=3), ARG)]      # (T 12: the head rides on the builds of T 17 ... 64)


@pytest.mark.parametrize("entry", ["amid_sas_seq_fwd_split_lnstat_head_f32", "amid_sas_seq_fwd_gather_head_f32",
                                   "amid_sas_seq_fwd_gather_head_p1_f32"])
def test_the_forwards_with_the_head_on_the_tail(entry):
    c = Form(entry)
    gather = "table" in c.names
    assert c.all_null() == ARG
    # (xout is optional here: only the head reads the last layer's rows)
    c.each_null(["x_in", "w16x3", "live"] + PARAM_FAMILIES + SAVED7 + HEAD_PTRS + (["step_state", "table", "idx_all", "pos0", "pos1", "tmq"] if gather else []))
    c.each(HEAD_SHAPES)
    c.each([({n: HALF}, ARG) for n in PARAM_FAMILIES] + [({n: HOLE}, ARG) for n in ["x_in"] + SAVED7])
    c.each([(dict(xout=None, D=64), UNSUPPORTED)])
    if not gather:
        c.each([(dict(train=1, step_state=None), ARG)])


@pytest.mark.parametrize("entry", ["amid_sas_seq_fwd_gather_f32", "amid_sas_seq_fwd_gather_p1_f32"])
def test_the_gathering_forwards(entry):
    c = Form(entry)
    assert c.all_null() == ARG
    c.each_null(["x_in", "xout", "w16x3", "step_state", "table", "idx_all", "pos0", "pos1", "tmq"] + PARAM_FAMILIES + SAVED7)
    c.each_null(["live"], code=UNSUPPORTED)                                    # the gather runs over a live list only
    c.each(SEQ_SHAPES + [(dict(D=64), UNSUPPORTED)])
    c.each([({n: HALF}, ARG) for n in PARAM_FAMILIES] + [({n: HOLE}, ARG) for n in ["x_in"] + SAVED7])
    c.each([(dict(NI=-1), ARG), (dict(NI=0), ARG), (dict(items=None, NI=0, D=64), UNSUPPORTED)])       # item rows asked for: NI > 0


def test_the_gathering_inference_forward():
    c = Form("amid_sas_seq_fwd_gather_infer_f32")
    assert c.all_null() == ARG
    c.each_null(["xout", "w16x3", "table", "idx_all", "pos0", "pos1"] + PARAM_FAMILIES)
    c.each_null(["live"], code=UNSUPPORTED)
    c.each(SEQ_SHAPES + [(dict(D=64), UNSUPPORTED)])
    c.each([({n: HALF}, ARG) for n in PARAM_FAMILIES])


# ---- csrc/sasrec_strip.hip, sasrec_strip_px.hip ----------------------------------------------------------------------------------------
STRIP_SHAPES = [(dict(B=0), ARG), (dict(B=-3), ARG), (dict(T=0), ARG), (dict(T=-7), ARG), (dict(D=0), UNSUPPORTED), (dict(D=-128), UNSUPPORTED),
                (dict(D=96), UNSUPPORTED), (dict(D=256), UNSUPPORTED), (dict(B=4096, T=1024), UNSUPPORTED)]


def test_the_forward_strips():
    c = Form("amid_sas_strip_qkv_fwd_f32", T=100)
    assert c.all_null() == ARG
    c.each_null(["x", "ln_w", "ln_b", "w_in", "b_in", "qn", "q", "k", "v"])
    c.each(STRIP_SHAPES)
    c = Form("amid_sas_strip_oproj_ffn_fwd_f32", T=100)
    assert c.all_null() == ARG
    c.each_null(["o", "qn", "w_o", "b_o", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "r", "y", "h", "xo"])
    c.each_null(["nln_b", "nw_in", "nb_in", "nqn", "nq", "nk", "nv"])           # the next layer's epilogue with an operand missing
    c.each(STRIP_SHAPES)
    c.each(STRIP_SHAPES, nln_w=None, nln_b=None, nw_in=None, nb_in=None, nqn=None, nq=None, nk=None, nv=None)      # the last layer's form
    c.each([(dict(train=1, step_state=None), ARG)])


def test_the_inference_forward_strips():                                       # (more of them: tests/test_cabi_eval_long.py)
    c = Form("amid_sas_strip_qkv_fwd_gather_infer_f32", T=100)
    assert c.all_null() == ARG
    c.each([(dict(B=4096, T=1024), UNSUPPORTED), (dict(live=None, D=96), UNSUPPORTED), (dict(ln_w=HALF), ARG)])
    c = Form("amid_sas_strip_oproj_ffn_fwd_infer_f32", T=100)
    assert c.all_null() == ARG
    c.each([(dict(B=4096, T=1024), UNSUPPORTED), (dict(nw_in=HALF), ARG), (dict(w2=HALF), ARG)])


FFN_BWD_PTRS = ["dxo", "h", "r", "ln_w", "w1T", "w2T", "woT", "dpre2", "dpre1", "dr", "d_o", "ln_part"]
# a rider: the plan is read (not checked) once the phase is one the launch can carry; no phase this launch carries is asked for here
FFN_RIDER = [(dict(sort_phase=0), ARG), (dict(sort_phase=5), ARG), (dict(sort_phase=-1), ARG), (dict(sort_phase=1), UNSUPPORTED),
             (dict(sort_phase=3), UNSUPPORTED), (dict(sort_phase=4), UNSUPPORTED)]


@pytest.mark.parametrize("entry", ["amid_sas_strip_ffn_bwd_f32", "amid_sas_strip_ffn_bwd_sort_f32"])
def test_the_feed_forward_backward_strip(entry):
    c = Form(entry, T=100)
    if "sort_plan" in c.names:
        c.set(sort_phase=2)
    assert c.all_null() == ARG
    c.each_null(FFN_BWD_PTRS)
    c.each(STRIP_SHAPES + [(dict(D=64, mma_bf16=1), UNSUPPORTED), (dict(D=64, mma_bf16=3), UNSUPPORTED), (dict(D=64, mma_bf16=3, B=0), UNSUPPORTED),
                           (dict(train=1, step_state=None), ARG), (dict(tmq=None, live=None, B=0), ARG)])
    if "sort_plan" in c.names:
        c.each_null(["sort_plan"])
        c.each(FFN_RIDER + [(dict(sort_phase=2, B=0), ARG), (dict(sort_phase=0, D=96), ARG), (dict(sort_phase=2, D=96), UNSUPPORTED)])


def test_the_feed_forward_backward_strip_on_pieces():
    c = Form("amid_sas_strip_ffn_bwd_px_f32", T=100, sort_plan=None)
    assert c.all_null() == ARG
    c.each_null(FFN_BWD_PTRS)
    c.each([(dict(B=0), ARG), (dict(B=-3), ARG), (dict(T=0), ARG), (dict(D=0), UNSUPPORTED), (dict(D=64), UNSUPPORTED), (dict(D=96), UNSUPPORTED),
            (dict(B=4096, T=1024), UNSUPPORTED), (dict(train=1, step_state=None), ARG), (dict(train=1, p_drop=0.1), UNSUPPORTED),
            (dict(train=1, p_drop=0.1, B=0), UNSUPPORTED), (dict(ln_stat=None, tmq=None, live=None, B=0), ARG)])
    c.each([(dict(sort_phase=p), UNSUPPORTED) for p in (0, 1, 3, 4, 5)], sort_plan=P)
    c.each([(dict(sort_phase=2, B=0), ARG)], sort_plan=P)


QKV_BWD_PTRS = ["dq", "dk", "dv", "dr", "x", "ln_w", "wqT", "wkT", "wvT", "ln_part"]
QKV_BWD_FFN = ["fr", "fln_w", "fw1T", "fw2T", "fwoT", "fdpre2", "fdpre1", "fdr", "fd_o", "fln_part"]
NO_FFN = dict(fh=None, fr=None, fln_w=None, fw1T=None, fw2T=None, fwoT=None, fdpre2=None, fdpre1=None, fdr=None, fd_o=None, fln_part=None)


@pytest.mark.parametrize("entry", ["amid_sas_strip_qkv_bwd_f32", "amid_sas_strip_qkv_bwd_sort_f32"])
def test_the_projection_backward_strip(entry):
    c = Form(entry, T=100)
    no_ffn = dict(NO_FFN)
    if "sort_plan" in c.names:                                                  # (the phase the launch carries: 3 with the feed-forward, 4 without)
        c.set(sort_phase=3)
        no_ffn["sort_phase"] = 4
    assert c.all_null() == ARG
    c.each_null(QKV_BWD_PTRS + QKV_BWD_FFN)                                     # (with fh: the fused feed-forward's operands are required)
    c.each_null(QKV_BWD_PTRS + ["dx"], **no_ffn)                                # (without: dx is)
    c.each_null(["dx"], B=0)                                                    # (with: it is not written)
    for form in ({}, no_ffn):
        c.each(STRIP_SHAPES + [(dict(D=64, mma_bf16=1), UNSUPPORTED), (dict(D=64, mma_bf16=3, B=0), UNSUPPORTED)], **form)
    c.each([(dict(train=1, step_state=None), ARG), (dict(train=1, step_state=None, B=0, **no_ffn), ARG)])
    if "sort_plan" in c.names:
        c.each_null(["sort_plan"])
        c.each([(dict(sort_phase=0), ARG), (dict(sort_phase=5), ARG), (dict(sort_phase=1), UNSUPPORTED), (dict(sort_phase=2), UNSUPPORTED),
                (dict(sort_phase=4), UNSUPPORTED), (dict(sort_phase=3, B=0), ARG), (dict(sort_phase=3, D=96), UNSUPPORTED)])
        c.each([(dict(sort_phase=0), ARG), (dict(sort_phase=3), UNSUPPORTED), (dict(sort_phase=2), UNSUPPORTED), (dict(sort_phase=4, T=0), ARG)], **NO_FFN)


def test_the_projection_backward_strip_with_the_scorer_sums():
    c = Form("amid_sas_strip_qkv_bwd_sort_scorer_f32", T=100, sort_phase=3, mma_bf16=3)
    assert c.all_null() == ARG
    c.each_null(QKV_BWD_PTRS + ["fh"] + QKV_BWD_FFN + ["sort_plan", "hidg", "u", "items", "dW1", "db1", "dW2", "db2"])
    off4 = ctypes.c_void_p(P.value + 4)
    c.each([(dict(NI=0), ARG), (dict(NI=-1), ARG), (dict(hid=0), ARG), (dict(hid=-32), ARG), (dict(dW1=off4), ARG), (dict(u=off4), ARG),
            (dict(items=off4), ARG), (dict(train=1, step_state=None), ARG)])
    c.each([(c_, code) for c_, code in STRIP_SHAPES if "D" not in c_] + [(dict(D=64), UNSUPPORTED), (dict(D=96), UNSUPPORTED), (dict(D=0), UNSUPPORTED)])
    c.each([(dict(sort_phase=0), ARG), (dict(sort_phase=5), ARG), (dict(sort_phase=2), UNSUPPORTED), (dict(sort_phase=4), UNSUPPORTED),
            (dict(mma_bf16=0), UNSUPPORTED), (dict(mma_bf16=2), UNSUPPORTED), (dict(mma_bf16=3, D=64), UNSUPPORTED)])


def test_the_projection_backward_strip_with_the_embedding_backward():
    c = Form("amid_sas_strip_qkv_bwd_emb_f32", T=100, sort_plan=None)
    assert c.all_null() == ARG
    c.each_null(QKV_BWD_PTRS + ["dx", "emb_tmq"])
    c.each(STRIP_SHAPES + [(dict(D=64, mma_bf16=3), UNSUPPORTED), (dict(train=1, step_state=None), ARG), (dict(train=1, step_state=None, B=0), ARG)])
    c.each([(dict(sort_phase=0), ARG), (dict(sort_phase=5), ARG), (dict(sort_phase=3), UNSUPPORTED), (dict(sort_phase=2), UNSUPPORTED),
            (dict(sort_phase=4, B=0), ARG)], sort_plan=P)


SEQ_BWD_LAYERS = ["h", "r", "x", "q", "k", "v", "o", "stats", "dpre2", "dpre1", "dr", "dq", "dk", "dv", "ln1_part", "ln2_part"]
SEQ_BWD_PARAMS = ["ln1_w", "ln2_w", "wqT", "wkT", "wvT", "woT", "w1T", "w2T"]


def test_the_one_launch_backward():
    c = Form("amid_sas_seq_bwd_f32")
    assert c.all_null() == ARG
    c.each_null(["dxo", "live", "d_o", "dx"] + SEQ_BWD_LAYERS + SEQ_BWD_PARAMS)
    c.each(SEQ_SHAPES)
    c.each([({n: HOLE}, ARG) for n in SEQ_BWD_LAYERS] + [({n: HALF}, ARG) for n in SEQ_BWD_PARAMS])
    c.each([(dict(train=1, step_state=None), ARG), (dict(tmq=None, D=96), UNSUPPORTED)])


# ---- csrc/bert_strip.hip, bert_seq_infer.hip -------------------------------------------------------------------------------------------
BERT_SHAPES = [(dict(B=0), ARG), (dict(B=-3), ARG), (dict(T=0), ARG), (dict(T=-7), ARG), (dict(B=4096, T=1024), UNSUPPORTED),
               (dict(B=1024, T=600), UNSUPPORTED)]           # ([2 B T, 128] within 2 GiB, and so the four times wider feed-forward tensors)
BERT_DROP = [(dict(train=1, step_state=None), ARG), (dict(train=1, p_drop=0.5), UNSUPPORTED), (dict(train=1, p_drop=0.5, B=0), UNSUPPORTED)]


@pytest.mark.parametrize("entry", ["amid_bert_strip_qkv_fwd_f32", "amid_bert_strip_qkv_fwd_pro_f32", "amid_bert_strip_qkv_fwd_pro_p3_f32"])
def test_the_bert_projection_strip(entry):
    c = Form(entry, T=50)
    if "n_keys" in c.names:
        c.set(n_keys=8)
    w3 = "w3_img" if "w3_img" in c.names else "w3"
    assert c.all_null() == ARG
    c.each_null(["x", "la", "lb", w3, "b3", "q", "k", "v"])
    c.each(BERT_SHAPES + [(dict(y=None, live=None, B=0), ARG)])                 # (y is optional: not stored)
    if "n_tr" in c.names:
        c.each(BERT_SHAPES, seq_d2=None, key_keep=None)
        c.each([(dict(n_tr=-1), ARG), (dict(n_tr=25), ARG), (dict(n_tr=2, tr_src=None), ARG), (dict(n_tr=2, tr_dst=None), ARG),
                (dict(n_tr=2, tr_rows=None), ARG), (dict(n_tr=2, tr_cols=None), ARG), (dict(n_tr=2, tr_src=HALF), ARG), (dict(n_tr=2, tr_dst=HALF), ARG),
                (dict(key_keep=None), ARG), (dict(n_keys=0), ARG), (dict(n_keys=-5), ARG), (dict(n_tr=2, n_keys=8, B=0), ARG)], n_keys=8)
        bad = (ctypes.c_int * 4)(64, 96, 64, 64)
        zero = (ctypes.c_int * 4)(64, 0, 64, 64)
        c.each([(dict(tr_rows=bad), ARG), (dict(tr_cols=bad), ARG), (dict(tr_rows=zero), ARG), (dict(tr_cols=zero), ARG)], n_tr=2, n_keys=8)


@pytest.mark.parametrize("entry", ["amid_bert_strip_oproj_ffn_fwd_f32", "amid_bert_strip_oproj_ffn_fwd_p3_f32"])
def test_the_bert_feed_forward_strip(entry):
    c = Form(entry, T=50, p_drop=0.1)
    img = "_img" if "wo_img" in c.names else ""
    assert c.all_null() == ARG
    c.each_null(["o", "x", "wo" + img, "bo", "la", "lb", "w1" + img, "b1", "w2" + img, "b2", "x2"])
    c.each_null(["nlb", "nw3" + img, "nb3", "nq", "nk", "nv"])
    last = dict(nla=None, nlb=None, nb3=None, ny=None, nq=None, nk=None, nv=None, **{"nw3" + img: None})
    for form in ({}, last, dict(x1=None, y2=None, pre=None, h=None, ny=None, live=None)):      # (the saved tensors are optional)
        c.each(BERT_SHAPES + BERT_DROP, **form)


@pytest.mark.parametrize("entry", ["amid_bert_strip_ffn_bwd_f32", "amid_bert_strip_ffn_bwd_p3_f32"])
def test_the_bert_feed_forward_backward_strip(entry):
    c = Form(entry, T=50, p_drop=0.1)
    img = "_img" if "w2T_img" in c.names else ""
    assert c.all_null() == ARG
    c.each_null(["dx2", "pre", "x1", "la", "w2T" + img, "w1T" + img, "woT" + img, "dz", "dpre", "dx1", "dt", "d_o", "ln_part"])
    c.each(BERT_SHAPES + BERT_DROP)


@pytest.mark.parametrize("entry", ["amid_bert_strip_qkv_bwd_f32", "amid_bert_strip_qkv_bwd_p3_f32"])
def test_the_bert_projection_backward_strip(entry):
    c = Form(entry, T=50, p_drop=0.1)
    img = "_img" if "wT3_img" in c.names else ""
    ffn = ["fx1", "fla", "fw2T" + img, "fw1T" + img, "fwoT" + img, "fdz", "fdpre", "fdx1", "fdt", "fd_o", "fln_part"]
    none = {n: None for n in ["fpre"] + ffn}
    assert c.all_null() == ARG
    c.each_null(["dq", "dk", "dv", "dx1", "x", "la", "wT3" + img, "ln_part"] + ffn)
    c.each_null(["dq", "dk", "dv", "dx1", "x", "la", "wT3" + img, "ln_part", "dx"], **none)
    c.each_null(["dx"], B=0)
    c.each(BERT_SHAPES + BERT_DROP)
    c.each(BERT_SHAPES + [(dict(zero_dead=1, B=0), ARG), (dict(train=1, p_drop=0.5, B=0), ARG)], **none)      # (no dropout site without the feed-forward)


def test_the_bert_one_launch_inference_encoder():
    c = Form("amid_bert_seq_fwd_gather_infer_f32", T=50)
    fams = ["la1", "lb1", "w3_img", "b3", "wo_img", "bo", "la2", "lb2", "w1_img", "b1", "w2_img", "b2"]
    assert c.all_null() == ARG
    c.each_null(["x_out", "live", "table", "idx_all", "seq_d2"] + fams)
    c.each([(dict(B=0), ARG), (dict(B=-3), ARG), (dict(T=0), ARG), (dict(T=-7), ARG), (dict(n_rows=0), ARG), (dict(n_rows=-1), ARG),
            (dict(T=65), UNSUPPORTED), (dict(B=1 << 20, T=64), UNSUPPORTED)])
    c.each([({n: HALF}, ARG) for n in fams])
