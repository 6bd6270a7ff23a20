"""Pins tests/gru_ref.py (the fp64 restatement of GRU4Rec every GPU test of the model compares against) to the golden vector produced by
running the reference itself (tests/golden/make_golden_gru.py), at the bars tests/test_oracle_golden.py uses for the other models.  CPU only."""
import os

import numpy as np
import torch

from tests import gru_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def load():
    z = np.load(os.path.join(GOLDEN, "g16_gru4rec.npz"), allow_pickle=False)
    batch = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("B/")}
    batch["label"] = torch.from_numpy(z["labels"])
    G = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("G/")}
    return z, gru_ref.golden_params(z), batch, G


def test_state_dict_names_and_shapes():
    s = gru_ref.gru4rec_param_shapes(300, 128, 16)
    assert list(s)[:5] == ["item_emb_layer.emb_item.weight", "gru1.weight_ih_l0", "gru1.weight_hh_l0", "gru1.bias_ih_l0", "gru1.bias_hh_l0"]
    assert s["gru2.weight_hh_l0"] == (384, 128) and s["gru2.bias_ih_l0"] == (384,) and s["predictModule.fc.0.weight"] == (16, 256)
    z, _, _, G = load()
    assert set(G) == set(s)


def test_g16_logits_loss_and_grads():
    z, P, batch, G = load()
    assert 0 < int(batch["domain_id"].sum()) < batch["domain_id"].numel()
    loss, (p1, p2), grads = gru_ref.loss_and_grads(P, batch)
    assert rel_err(p1, z["p1"]) < 1e-6 and rel_err(p2, z["p2"]) < 1e-6
    assert abs(float(loss) - float(z["loss"])) < 1e-6 * max(1.0, abs(float(z["loss"])))
    assert G
    for k, g in G.items():
        assert rel_err(grads[k], g) < 5e-5 or float((grads[k] - g).abs().max()) < 1e-8, k
    pad = int(z["n_items"]) - 1               # the pad id's row is an ordinary trained row
    assert float(G["item_emb_layer.emb_item.weight"][pad].abs().max()) > 0


def test_hand_stepped_layer_is_nn_gru_and_sees_the_mutants():
    g = torch.Generator().manual_seed(3)
    D, k = 128, 1.0 / 128 ** 0.5
    x = torch.randn(3, 4, D, generator=g, dtype=torch.float64)
    w = [(torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k for s in ((3 * D, D), (3 * D, D), (3 * D,), (3 * D,))]
    ref = gru_ref.gru_layer(x, *w)
    taps = gru_ref.gru_taps(x, *w)
    assert float((taps["h"] - ref).abs().max()) < 1e-13
    assert torch.equal(taps["hprev"][:, 1:], taps["h"][:, :-1]) and float(taps["hprev"][:, 0].abs().max()) == 0.0
    for mutant in ("swap_rz", "bhn_outside"):
        assert float((gru_ref.gru_taps(x, *w, mutant=mutant)["h"] - ref).abs().max()) > 1e-3 * float(ref.abs().max()), mutant
