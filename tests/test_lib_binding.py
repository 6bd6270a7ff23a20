"""CPU-side checks of the binding by parameter name (amid_amd/_lib.py Binder, _Lib.call_named): what include/amid_hip.h must keep true for
the engines' named pointer tables, the binding rules on a synthetic header, and one real entry point called by name (no GPU: it refuses
its null pointer before anything is launched)."""
import ast
import ctypes
import os
import re

import pytest

from amid_amd import _lib
from amid_amd.engine import SASREC_FAMILIES

SEQ_FORWARDS = ("amid_sas_seq_fwd_f32", "amid_sas_seq_fwd_bf16w_f32", "amid_sas_seq_fwd_split_f32", "amid_sas_seq_fwd_split_lnstat_f32",
                "amid_sas_seq_fwd_split_lnstat_head_f32", "amid_sas_seq_fwd_gather_f32", "amid_sas_seq_fwd_gather_p1_f32",
                "amid_sas_seq_fwd_gather_head_f32", "amid_sas_seq_fwd_gather_head_p1_f32", "amid_sas_seq_fwd_gather_infer_f32",
                "amid_sas_seq_fwd_split_infer_f32")
FAMILIES = ("ln1_w", "ln1_b", "w_in", "b_in", "w_o", "b_o", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")
SAVED = ("qn|ln_stat", "q", "k", "v", "o", "stats", "r", "y", "h")


def test_every_prototype_names_its_parameters_uniquely():
    protos = _lib.parse_header()
    assert len(protos) >= 200
    for entry, (_, argtypes, names) in protos.items():
        assert len(names) == len(argtypes), entry
        assert len(set(names)) == len(names), entry


def test_one_launch_forwards_spell_the_families_and_saved_tensors_alike():
    protos = _lib.parse_header()
    assert tuple(n for n, _ in SASREC_FAMILIES) == FAMILIES          # the engines' one list is the header's
    for entry in SEQ_FORWARDS:
        names = protos[entry][2]
        at = names.index(FAMILIES[0])
        assert tuple(names[at:at + 12]) == FAMILIES, entry           # contiguous, in this order
        saved = [n for n in names if n in ("qn", "ln_stat", "q", "k", "v", "o", "stats", "r", "y", "h")]
        assert not ("qn" in saved and "ln_stat" in saved), entry
        it = iter(SAVED)                                             # a subsequence of SAVED
        assert all(any(n in s.split("|") for s in it) for n in saved), (entry, saved)


# ---- one vocabulary: the C type every name supplied by a shared table has wherever it is bound by name.  The NAMES are collected from the
# table builders' sources (_table_names), so a key added to a table must be declared here; the types are the declaration.  What this cannot
# see: the header is nearly all void* and int, so a name that is one type but two things at two entries passes (profiles/launch_trace.md
# names the known ones, `workspace` and `p`); the check is of types and of the retired spellings, not of meaning.
_P, _I, _F, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
VOCABULARY = dict(
    dict.fromkeys(("grad_rows", "pos_sorted", "seg_off", "seg_of", "workspace", "uniq_grad", "uniq_ids", "n_uniq", "p", "m", "v", "g", "table",
                   "m_tab", "v_tab", "last", "dpos0", "dpos1", "idx_all", "pos0", "pos1", "xg", "tmq", "step_state", "stream", "x", "qn", "q", "k",
                   "o", "stats", "r", "y", "h", "xo", "dq", "dk", "dv", "dr", "dpre1", "dpre2", "ln_w", "ln_b", "w_in", "b_in", "i_node", "neg",
                   "seq_d1", "seq_d2", "in_pack", "idx_c", "row_c", "live", "domain", "err_flag", "pool", "w_src", "w16_dst", "w16t_dst",
                   "out_ids", "dense_src", "dense_dst", "domain_id", "pool_d1", "pool_d2", "own_items", "own_off", "rows", "ln_part", "d_o",
                   "wqT", "wkT", "wvT", "w1T", "w2T", "woT"), _P),
    **dict.fromkeys(("B", "T", "D", "n_item_rows", "train", "in_words", "n_neg", "n_pool", "n_w", "w_planes", "n_out", "pad_id", "n_pool_d1",
                     "n_pool_d2", "hid", "layer"), _I),
    **dict.fromkeys(("n", "n_rows", "pool_stride", "phase", "dense_n"), _LL), p_drop=_F)
# the shared tables' builders in amid_amd/engine.py (a table spelled with a prefix at some entries: the prefix)
TABLE_BUILDERS = dict(_marshal="", _pool_batch="", _seg="", _uniq="", _saved="", _grads="", _qkv_block="n", _ffn_bwd_block="f", _qkv_bwd_block="",
                      _adam_dense="", _adam_rows="", _dpos="", _k1_head="", _w16_riders="", _pack_block="", _catalog="")
DRIVERS = ("engine.py", "engine_bert.py", "engine_dp.py")
# left positional on purpose: the InnerComp and BERT-comp entry points of 20 or more parameters
POSITIONAL_WIDE = {"amid_inc_embed_fwd_f32", "amid_inc_embed_fwd_shard_f32", "amid_inc_bwd_f32", "amid_inc_bwd_shard_f32",
                   "amid_bert_comp_fwd_shard_f32", "amid_bert_comp_bwd_f32", "amid_bert_comp_bwd_shard_f32"}
_ROOT = os.path.dirname(os.path.abspath(_lib.__file__))


def _table_names():
    """builder -> the names its table supplies, read from its source: the keywords of its dict(...) calls and the string tuples its
    comprehensions run over."""
    out = {}
    for fn in ast.walk(ast.parse(open(os.path.join(_ROOT, "engine.py")).read())):
        if isinstance(fn, ast.FunctionDef) and fn.name in TABLE_BUILDERS:
            names = set()
            for n in ast.walk(fn):
                if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "dict":
                    names |= {k.arg for k in n.keywords if k.arg}
                if isinstance(n, (ast.DictComp, ast.ListComp, ast.GeneratorExp)):
                    for g in n.generators:
                        if isinstance(g.iter, ast.Tuple):
                            names |= {e.value for e in g.iter.elts if isinstance(e, ast.Constant) and isinstance(e.value, str)}
            out[fn.name] = names
    return out


def _launch_sites(protos):
    """(file, line, "call" | "call_named", the declared entry points the site's first argument can name -- None where the name cannot be
    read from the source) of every launch in the drivers.  An f-string's holes and a suffix added to the name are expanded against the
    header: anything declared that fits."""
    def pattern(n):
        if isinstance(n, ast.Constant) and isinstance(n.value, str):
            return re.escape(n.value)
        if isinstance(n, ast.JoinedStr):
            return "".join(pattern(v) if isinstance(v, ast.Constant) else r"\w*" for v in n.values)
        if isinstance(n, ast.BinOp) and isinstance(n.op, ast.Add):
            return pattern(n.left) + pattern(n.right)
        if isinstance(n, ast.IfExp):
            return "(?:" + pattern(n.body) + "|" + pattern(n.orelse) + ")"
        return r"\w*"

    for name in DRIVERS:
        for c in ast.walk(ast.parse(open(os.path.join(_ROOT, name)).read())):
            if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr in ("call", "call_named") and c.args:
                pat = pattern(c.args[0])
                readable = all(alt.startswith("amid_") for alt in pat.replace("(?:", "").replace(")", "").split("|"))
                yield name, c.lineno, c.func.attr, sorted(e for e in protos if re.fullmatch(pat, e)) if readable else None


def test_a_shared_table_name_means_one_thing_wherever_it_is_bound():
    protos = _lib.parse_header()
    tables = _table_names()
    assert set(tables) == set(TABLE_BUILDERS) and all(tables.values())
    supplied = set()
    for builder, names in tables.items():
        assert names <= set(VOCABULARY), (builder, sorted(names - set(VOCABULARY)))         # a new key: declare its type
        supplied |= names
    assert supplied == set(VOCABULARY), sorted(set(VOCABULARY) - supplied)                 # ... and nothing declared that no table supplies
    spelled = dict(VOCABULARY)                                                              # + the prefixed blocks' names
    for builder, pre in TABLE_BUILDERS.items():
        spelled.update({pre + n: VOCABULARY[n] for n in tables[builder]} if pre else {})
    sites = list(_launch_sites(protos))
    assert all(entries for _, _, how, entries in sites if how == "call_named")              # every named site names something declared
    bound = {e for _, _, how, entries in sites if how == "call_named" for e in entries}
    assert len(bound) >= 80
    for entry in sorted(bound):
        _, argtypes, names = protos[entry]
        for n, t in zip(names, argtypes):
            if n in spelled:
                assert t is spelled[n], (entry, n, t)
    for entry, (_, _, names) in protos.items():
        # the step state has one name: what the caller passes self.step_state for
        assert not {"rng_state", "step_state_to_bump"} & set(names), entry
        # ... the replay K1 takes it a second time, as the state its Adam coefficients come from: a name of that entry alone
        assert ("adam_state" in names) == (entry == "amid_embed_fwd_replay_f32"), entry
        # m, v are the DENSE moments: beside a table with step stamps the moments are m_tab, v_tab
        if "table" in names and "last" in names:
            assert "m_tab" in names and "v_tab" in names, entry
        if "table" in names and "m" in names:
            assert "m_tab" in names and "v_tab" in names, entry


def test_no_wide_entry_point_is_launched_positionally():
    protos = _lib.parse_header()
    wide, unread = set(), []
    for name, line, how, entries in _launch_sites(protos):
        if how == "call" and entries is None:
            unread.append((name, line))             # a name the check cannot read could be any entry, a wide one included
        elif how == "call":
            wide |= {e for e in entries if len(protos[e][2]) >= 20}
    assert not unread, unread
    assert wide == POSITIONAL_WIDE


def test_prefixed_and_absent_blocks_bind_on_a_synthetic_header():
    protos = _lib.parse_prototypes("int amid_toy2_f32(const float* q, const float* ln_w, int layer, float* nq, const float* nln_w, int nlayer, void* stream);")
    b = _lib.Binder(protos)
    blk = dict(q="Q", ln_w="W", layer=1, unused="U")
    nxt = _lib.prefixed("n", blk)
    assert nxt == dict(nq="Q", nln_w="W", nlayer=1, nunused="U") and blk["q"] == "Q"
    assert b.bind("amid_toy2_f32", (blk, nxt), dict(stream=7)) == ("Q", "W", 1, "Q", "W", 1, 7)
    # an absent block: every pointer an explicit null, the by-value parameters as given; names the entry does not take are ignored
    none = _lib.absent(nxt, nlayer=0)
    assert none == dict(nq=None, nln_w=None, nlayer=0, nunused=None)
    assert b.bind("amid_toy2_f32", (blk, none), dict(stream=7)) == ("Q", "W", 1, None, None, 0, 7)
    with pytest.raises(TypeError, match=r"amid_toy2_f32.*'nq'.*not supplied"):          # a prefix that is not the entry's: nothing binds silently
        b.bind("amid_toy2_f32", (blk, _lib.prefixed("f", blk)), dict(stream=7, nlayer=0, nln_w=None))
    with pytest.raises(TypeError, match=r"amid_toy2_f32.*'q'.*2 times"):               # an unprefixed block beside itself
        b.bind("amid_toy2_f32", (blk, blk, nxt), dict(stream=7))


SYNTHETIC = """
/* a comment with amid_not_this(int a); */
int amid_toy_f32(int n, const float* const* w1, const float* x,   // trailing
                 float* const* q, float eps, void* stream);
int amid_other(void);
"""


def test_binding_rules_on_a_synthetic_header():
    protos = _lib.parse_prototypes(SYNTHETIC)
    assert sorted(protos) == ["amid_other", "amid_toy_f32"]
    assert protos["amid_toy_f32"][2] == ["n", "w1", "x", "q", "eps", "stream"] and protos["amid_other"][2] == []
    b = _lib.Binder(protos)
    fams, saved = dict(w1="W1", b1="B1"), dict(y="Y", q="Q")
    # the order is the prototype's, not the call's; names the entry does not take (b1, y) are ignored; None is a value
    assert b.bind("amid_toy_f32", (saved, fams), dict(stream=7, eps=0.5, x=None, n=2)) == (2, "W1", None, "Q", 0.5, 7)
    assert b.bind("amid_toy_f32", (fams, saved), dict(eps=0.5, n=2, x=None, stream=7)) == (2, "W1", None, "Q", 0.5, 7)
    assert b.bind("amid_toy_f32", (dict(w1="other", b1=0), saved), dict(stream=7, eps=0.5, x=None, n=2))[1] == "other"      # (the cached order reads the call's values)
    assert b.bind("amid_other", (), {}) == ()
    with pytest.raises(TypeError, match=r"amid_toy_f32.*'y'"):                 # an explicit name that is no parameter
        b.bind("amid_toy_f32", (fams, saved), dict(n=2, x=None, eps=0.5, stream=7, y=1))
    with pytest.raises(TypeError, match=r"amid_toy_f32.*'x'.*not supplied"):
        b.bind("amid_toy_f32", (fams, saved), dict(n=2, eps=0.5, stream=7))
    with pytest.raises(TypeError, match=r"amid_toy_f32.*'q'.*2 times"):        # by two tables
        b.bind("amid_toy_f32", (fams, saved, dict(q="again")), dict(n=2, x=None, eps=0.5, stream=7))
    with pytest.raises(TypeError, match=r"amid_toy_f32.*'w1'.*2 times"):       # by a table and by name
        b.bind("amid_toy_f32", (fams, saved), dict(n=2, x=None, eps=0.5, stream=7, w1="again"))
    with pytest.raises(TypeError, match="amid_nowhere"):
        b.bind("amid_nowhere", (), {})


def test_a_real_entry_point_called_by_name_reports_through_amid_error():
    L = _lib.lib()
    seen = []
    orig = L.call
    L.call = lambda name, *a: (seen.append((name, a)), orig(name, *a))[1]          # (the spy the GPU tests hang on the positional call)
    try:
        ptrs = dict.fromkeys(("ln_w", "ln_b", "table", "ids", "w1", "b1", "w2", "b2", "labels", "domain_id", "u", "p", "rank", "rank_raw",
                              "loss_part", "stream"))
        with pytest.raises(_lib.AmidError) as e:
            L.call_named("amid_eval_head_f32", ptrs, dict(unused=1), x=None, B=4, T=40, NI=100, D=128, hid=32, eps=1e-8, fix_value=1e-7)
        assert e.value.fn == "amid_eval_head_f32" and e.value.code == -1            # AMID_ERR_ARG: nothing was launched
        with pytest.raises(TypeError, match="amid_eval_head_f32.*'x'"):
            L.call_named("amid_eval_head_f32", ptrs, B=4, T=40, NI=100, D=128, hid=32, eps=1e-8, fix_value=1e-7)
    finally:
        del L.call
    assert [n for n, _ in seen] == ["amid_eval_head_f32"]                           # the unbound call never reached the library
    assert seen[0][1] == (None,) * 11 + (4, 40, 100, 128, 32, 1e-8, 1e-7) + (None,) * 6
