"""The bf16x3_fwd precision on the BUTD engine (rgqa_config.arch = 1), host side: the engine is created, its parameter table is the bf16x3
engine's, and malformed BUTD configurations are still refused.  No GPU needed."""
import pytest

from rgqa_amd.engine import Engine

BUTD = dict(arch=1, vocab_size=3001, hidden=1024, emb_dim=300, feat_dim=2048, pos_dim=4, num_answers=1842, heads=1, inter=8,
            l_layers=0, x_layers=0, r_layers=0, hidden_dropout=0.0, attn_dropout=0.0)


def table(e):
    return [(sp.name, tuple(sp.shape), sp.offset) for sp in e.specs]


def test_butd_bf16x3_fwd_engine_is_created_with_the_bf16x3_parameter_table():
    e = Engine(precision="bf16x3_fwd", **BUTD)
    ref = Engine(precision="bf16x3", **BUTD)
    assert e.precision == "bf16x3_fwd"
    assert len(e.specs) > 0 and table(e) == table(ref)
    assert e.arena_elems == ref.arena_elems
    names = {sp.name for sp in e.specs}
    assert {"q_enc.rnn.weight_hh_l0", "q_enc.rnn.weight_ih_l0", "ans_classifier.3.weight_v", "w_emb.emb.weight"} <= names


def test_butd_bf16x3_fwd_short_name():
    assert table(Engine(precision="x3fwd", **BUTD)) == table(Engine(precision="bf16x3_fwd", **BUTD))


@pytest.mark.parametrize("bad", [dict(hidden=96), dict(hidden=0), dict(feat_dim=2046), dict(pos_dim=5), dict(num_answers=0), dict(vocab_size=1),
                                 dict(hidden_dropout=1.0)])
def test_butd_bf16x3_fwd_rejects_bad_configs(bad):
    cfg = dict(BUTD)
    cfg.update(bad)
    with pytest.raises(Exception):
        Engine(precision="bf16x3_fwd", **cfg)
