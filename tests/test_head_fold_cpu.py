"""CPU: where the folded head tail applies (UserModel.head_fold_applies: a host-side decision that never looks at the row count)
and the host-side validation of nrm_head_fold / nrm_head_fold_bwd (nothing is launched)."""
import ctypes

import torch

from news_recommendation_model_amd import ops
from news_recommendation_model_amd.modules import MLP, UserModel


def _model():
    torch.manual_seed(0)
    return UserModel(3)


def test_fold_applies_to_the_default_model_and_is_switched_off_by_env(monkeypatch):
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    m = _model()
    width = m.bn.num_features
    assert width % 4 == 0 and m.head_fold_applies(width)
    assert not m.head_fold_applies(width + 4)                             # rows the first layer does not take
    monkeypatch.setenv("NRM_HEAD_FOLD", "0")
    assert not m.head_fold_applies(width)
    monkeypatch.setenv("NRM_HEAD_FOLD", "1")
    assert m.head_fold_applies(width)


def test_fold_needs_fp32_dense_arithmetic(monkeypatch):
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    m = _model()
    try:
        ops.set_dense_arithmetic("bf16x3")
        assert not m.head_fold_applies(m.bn.num_features)
    finally:
        ops.set_dense_arithmetic(None)
    assert m.head_fold_applies(m.bn.num_features)


def test_hooks_substituted_layers_and_other_activations_keep_the_two_call_path(monkeypatch):
    monkeypatch.delenv("NRM_HEAD_FOLD", raising=False)
    width = _model().bn.num_features
    for where in ("mlp", "out_mlp", "mlp.fc2", "out_mlp.fc1", "mlp.fc1", "out_mlp.fc2"):
        for kind in ("forward", "forward_pre", "backward"):
            m = _model()
            mod = m.get_submodule(where)
            handle = {"forward": lambda: mod.register_forward_hook(lambda *a: None),
                      "forward_pre": lambda: mod.register_forward_pre_hook(lambda *a: None),
                      "backward": lambda: mod.register_full_backward_hook(lambda *a: None)}[kind]()
            assert not m.head_fold_applies(width), (where, kind)
            handle.remove()
            assert m.head_fold_applies(width), (where, kind)
    m = _model()
    m.mlp = MLP(width, width, "relu")
    assert not m.head_fold_applies(width)
    m = _model()
    m.out_mlp.activation = torch.nn.GELU(approximate="tanh")
    assert not m.head_fold_applies(width)
    m = _model()

    class Lin(torch.nn.Linear):
        pass
    m.out_mlp.fc1 = Lin(width, width // 4)
    assert not m.head_fold_applies(width)
    m = _model()
    m.mlp.fc2 = torch.nn.Linear(width // 4, width, bias=False)
    assert not m.head_fold_applies(width)
    m = _model().double()
    assert not m.head_fold_applies(width)


def test_shape_rule_takes_hidden_widths_that_are_no_multiple_of_4():
    r = torch.zeros
    ok = ops.head_fold_shapes_ok
    assert ok(1608, r(402, 1608), r(1608, 402), r(1608), r(402, 1608), r(402), r(1, 402))
    assert ok(24, r(6, 24), r(24, 6), r(24), r(6, 24), r(6), r(1, 6))
    assert not ok(26, r(6, 26), r(26, 6), r(26), r(6, 26), r(6), r(1, 6))             # folded width not a multiple of 4
    assert not ok(24, r(6, 24), r(28, 6), r(28), r(6, 24), r(6), r(1, 6))             # layers do not chain
    assert not ok(24, r(6, 24), r(24, 6), None, r(6, 24), r(6), r(1, 6))


def test_entry_points_validate_on_the_host(lib):
    fake = ctypes.c_void_p(0x1000)
    assert lib.nrm_head_fold(None, None, fake, None, 6, 24, 6, fake, fake, fake, None) != 0 and b"null" in lib.nrm_last_error()
    assert lib.nrm_head_fold(fake, None, fake, None, 6, 26, 6, fake, fake, fake, None) != 0 and b"multiple of 4" in lib.nrm_last_error()
    assert lib.nrm_head_fold(ctypes.c_void_p(0x1004), None, fake, None, 6, 24, 6, fake, fake, fake, None) != 0
    assert lib.nrm_head_fold_bwd(None, 8, fake, fake, fake, fake, 6, 24, 6, fake, fake, fake, fake, None) != 0 and b"null" in lib.nrm_last_error()
    assert lib.nrm_head_fold_bwd(fake, 6, fake, fake, fake, None, 6, 24, 6, fake, fake, fake, fake, None) != 0 and b"ldp" in lib.nrm_last_error()
    assert lib.nrm_head_fold_bwd(fake, 4, fake, fake, fake, fake, 6, 24, 6, fake, fake, fake, fake, None) != 0
