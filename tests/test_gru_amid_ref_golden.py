"""Pins tests/gru_amid_ref.py (the fp64 restatement of GRU4Rec with isInC / isItC / isDR every GPU test of the variants compares against) to
the golden vectors produced by running the reference itself (tests/golden/make_golden_gru_amid.py: g17 isItC, g18 isInC, g19 all three), at
the bars of tests/test_gru_ref_golden.py.  CPU only."""
import pytest
import torch

from tests import gru_amid_ref as ref

FIXTURES = ("g17_gru4rec_itc", "g18_gru4rec_inc", "g19_gru4rec_inc_itc_dr")


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def grads_of(z, pre):
    return {k[len(pre):]: torch.from_numpy(z[k]) for k in z if k.startswith(pre)}


def check_grads(grads, G):
    assert G
    for k, g in G.items():
        assert rel_err(grads[k], g) < 5e-5 or float((grads[k] - g).abs().max()) < 1e-8, k


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_names_order_and_shapes(name):
    z, P, _ = ref.load_golden(name)
    fl = ref.golden_flags(z)
    s = ref.gru4rec_amid_param_shapes(int(z["n_items"]), int(z["D"]), int(z["hid"]), int(z["bs"]), fl["isInC"], fl["isItC"], fl["isDR"])
    assert list(s) == [str(n) for n in z["names"]]                       # the reference's state_dict, in its order
    G = grads_of(z, "GE/" if fl["isDR"] else "G/")
    assert set(G) == set(s) and all(tuple(G[k].shape) == s[k] for k in s)
    assert list(s)[0] == "item_emb_layer.emb_item.weight" and list(s)[-1].endswith(("predictModule.fc.2.bias", "predict_gfunc.fc.2.bias"))


@pytest.mark.parametrize("name", FIXTURES)
def test_the_fixture_exercises_its_gates(name):
    z, P, batch = ref.load_golden(name)
    fl = ref.golden_flags(z)
    assert 0 < int(batch["domain_id"].sum()) < batch["domain_id"].numel()
    taps = {}
    ref.gru4rec_amid_forward({k: v.double() for k, v in P.items()}, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"],
                             taps=taps, **fl)
    mods = (["inc_d1", "inc_d2"] if fl["isInC"] else []) + (["itc_d1", "itc_d2"] if fl["isItC"] else [])
    assert mods
    for mname in mods:
        gate = taps[mname]["gate"]
        assert 0 < float(gate.sum()) < gate.numel(), mname
        assert taps[mname]["margin"] > 0.01, mname
    assert abs(min(taps[mname]["margin"] for mname in mods) - float(z["gate_margin"])) < 1e-5


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_logits_loss_and_grads(name):
    z, P, batch = ref.load_golden(name)
    loss, (p1, p2), grads = ref.loss_and_grads(P, batch, **ref.golden_flags(z))
    assert rel_err(p1, z["p1"]) < 1e-6 and rel_err(p2, z["p2"]) < 1e-6
    assert abs(float(loss) - float(z["loss"])) < 1e-6 * max(1.0, abs(float(z["loss"])))
    check_grads(grads, grads_of(z, "G/"))


def test_g19_six_outputs_both_objectives():
    z, P, batch = ref.load_golden(FIXTURES[2])
    fl = ref.golden_flags(z)
    for which, pre, key in (("e", "GE/", None), ("r", "GR/", "loss_dr_r")):
        loss, outs, grads = ref.loss_and_grads(P, batch, which=which, dr_e_w=float(z["dr_e_w"]), **fl)
        assert len(outs) == 6
        for o, k in zip(outs, ("p1", "p2", "ips1", "ips2", "g1", "g2")):
            assert rel_err(o, z[k]) < 1e-6, k
        want = float(z[key]) if key else float(z["loss_cls"]) + float(z["dr_e_w"]) * float(z["loss_dr_e"])
        assert abs(float(loss) - want) < 1e-6 * max(1.0, abs(want))
        check_grads(grads, grads_of(z, pre))
