"""CPU-side pin of what the backward strip entry points answer for products mode 4 (the N-split build on bf16 pieces,
csrc/sasrec_strip_px.hip) and of amid_sas_strip_qkv_bwd_px_f32's argument checks: every code is decided before a device is touched; no
case passes every check (that call would launch)."""
import pytest

from amid_amd import _lib
from tests.test_cabi_launch_forms import ARG, UNSUPPORTED, Form

FFN = ["amid_sas_strip_ffn_bwd_f32", "amid_sas_strip_ffn_bwd_sort_f32"]
QKV = ["amid_sas_strip_qkv_bwd_f32", "amid_sas_strip_qkv_bwd_sort_f32", "amid_sas_strip_qkv_bwd_scorer_f32", "amid_sas_strip_qkv_bwd_sort_scorer_f32"]


def test_the_n_split_entry_is_declared_and_exported():
    assert "amid_sas_strip_qkv_bwd_px_f32" in _lib.declared_symbols()
    assert _lib.lib()._fn["amid_sas_strip_qkv_bwd_px_f32"] is not None


@pytest.mark.parametrize("entry", FFN + QKV + ["amid_sas_strip_qkv_bwd_emb_f32"])
def test_mode_4_needs_d_128_and_dropout_one_half(entry):
    phase = 2 if entry in FFN else 3 if "sort" in entry else 0
    c = Form(entry, mma_bf16=4, train=1, **(dict(sort_phase=phase) if "sort_phase" in Form(entry).names else {}))
    rate = "emb_p_drop" if entry.endswith("_emb_f32") else "p_drop"
    if entry.endswith("_emb_f32"):
        c.set(sort_plan=None)
    c.each([(dict(D=64), UNSUPPORTED), (dict(D=96), UNSUPPORTED), ({rate: 0.1}, UNSUPPORTED), ({rate: 0.25}, UNSUPPORTED), (dict(B=0), ARG),
            (dict(T=0), ARG), (dict(B=4096, T=1024), UNSUPPORTED)])


def test_the_n_split_projection_backward_entry():
    c = Form("amid_sas_strip_qkv_bwd_px_f32", train=1, sort_plan=None, hidg=None, emb_tmq=None)
    assert c.all_null() == ARG
    c.each_null(["dq", "dk", "dv", "dr", "x", "ln_w", "wqT", "wkT", "wvT", "ln_part"])
    c.each([(dict(D=64), UNSUPPORTED), (dict(D=0), UNSUPPORTED), (dict(B=0), ARG), (dict(T=0), ARG), (dict(B=4096, T=1024), UNSUPPORTED),
            (dict(p_drop=0.1), UNSUPPORTED), (dict(train=1, step_state=None), ARG)])
    # the fused feed-forward chain: every operand, its rider's phase, the scorer sums only with it
    c.each_null(["fr", "fln_w", "fw1T", "fw2T", "fwoT", "fdpre2", "fdpre1", "fdr", "fd_o", "fln_part"])
    plan = c.good["dq"]                                  # (stands in for a packed sort plan: rejected before it is read beyond its phase)
    c.each([(dict(sort_plan=plan, sort_phase=0), ARG), (dict(sort_plan=plan, sort_phase=5), ARG), (dict(sort_plan=plan, sort_phase=2), UNSUPPORTED),
            (dict(sort_plan=plan, sort_phase=4), UNSUPPORTED)])
    hid = dict(hidg=c.good["dq"])
    c.each([({**hid, "fh": None}, ARG), ({**hid, "u": None}, ARG), ({**hid, "dW1": None}, ARG), ({**hid, "NI": 0}, ARG), ({**hid, "hid": 0}, ARG)])
    # without the fused chain: dx is written; the embedding epilogue's dropout rate; phase 4
    e = Form("amid_sas_strip_qkv_bwd_px_f32", train=1, sort_plan=None, hidg=None, fh=None)
    e.each([(dict(dx=None), ARG), (dict(emb_p_drop=0.1), UNSUPPORTED), (dict(sort_plan=plan, sort_phase=3), UNSUPPORTED),
            (dict(emb_tmq=None, dx=None), ARG)])
