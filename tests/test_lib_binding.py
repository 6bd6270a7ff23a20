"""CPU-side checks of the binding by parameter name (amid_amd/_lib.py Binder, _Lib.call_named): what include/amid_hip.h must keep true for
the engines' named pointer tables, the binding rules on a synthetic header, and one real entry point called by name (no GPU: it refuses
its null pointer before anything is launched)."""
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
