"""CPU-side checks of what Model decides before it touches a device: which architecture a config selects
(riser_amd.model.select_architecture), the one state-dict conversion (riser_amd._family.load_state), and the attributes
every Model has whichever arm built it - or none has yet."""
import itertools
import types

import numpy as np

SECTIONS = ("cnn", "resnet", "tcn", "tcnbot", "cnn_rnn")
MODELS = (None, "cnn", "resnet", "tcn", "tcn-bot", "cnn-rnn", "nonsense")       # None: no `model` attribute at all


def _selected_before(config) -> str:
    """the conditionals Model.__init__ opened with before select_architecture existed, as they stood: each arm's constructor
    call replaced by the name of the architecture it built"""
    kind = getattr(config, "model", None)
    if kind == "cnn-rnn" or (kind is None and not hasattr(config, "cnn") and hasattr(config, "cnn_rnn")):
        return "cnn-rnn"
    is_resnet = kind == "resnet" or (not hasattr(config, "cnn") and hasattr(config, "resnet"))
    if not is_resnet and (kind == "tcn-bot" or (kind != "tcn" and not hasattr(config, "cnn") and hasattr(config, "tcnbot"))):
        return "tcn-bot"
    if not is_resnet and (kind == "tcn" or (not hasattr(config, "cnn") and hasattr(config, "tcn"))):
        return "tcn"
    if is_resnet:
        return "resnet"
    return "cnn"


def _configs():
    for model in MODELS:
        for r in range(len(SECTIONS) + 1):
            for present in itertools.combinations(SECTIONS, r):
                fields = {s: types.SimpleNamespace() for s in present}
                if model is not None:
                    fields["model"] = model
                yield model, present, types.SimpleNamespace(**fields)


def test_select_architecture_truth_table():
    from riser_amd.model import select_architecture
    seen, n = set(), 0
    for model, present, config in _configs():
        got = select_architecture(config)
        assert got == _selected_before(config), (model, present, got)
        seen.add(got)
        n += 1
    assert n == 7 * 32
    assert seen == {"cnn-rnn", "tcn-bot", "tcn", "resnet", "cnn"}


def test_select_architecture_quirks():
    """the precedence rules worth a name, one config each"""
    from riser_amd.model import select_architecture
    ns = types.SimpleNamespace
    assert select_architecture(ns(cnn=ns(), resnet=ns(), tcn=ns(), tcnbot=ns(), cnn_rnn=ns())) == "cnn"     # `cnn` beats presence
    assert select_architecture(ns(model="tcn", tcnbot=ns(), tcn=ns())) == "tcn"         # `model: tcn` silences the tcnbot section
    assert select_architecture(ns(tcnbot=ns(), tcn=ns())) == "tcn-bot"
    assert select_architecture(ns(model="tcn-bot", resnet=ns())) == "resnet"            # resnet-ness silences both TCN rules
    assert select_architecture(ns(model="tcn", resnet=ns())) == "resnet"
    assert select_architecture(ns(model="nonsense", tcn=ns())) == "tcn"                 # an unknown name: the sections decide
    assert select_architecture(ns(model="nonsense")) == "cnn"
    assert select_architecture(ns(model="nonsense", cnn_rnn=ns())) == "cnn"             # ... but cnn_rnn only without `model`
    assert select_architecture(ns(model="cnn-rnn", cnn=ns())) == "cnn-rnn"              # a named kind needs no section here


def test_load_state_dicts_and_path(tmp_path):
    import torch
    from riser_amd._family import load_state
    rng = np.random.default_rng(5)
    arrays = {"a.weight": rng.standard_normal((3, 2, 3)).astype(np.float32), "a.bias": rng.standard_normal(3).astype(np.float32),
              "n": np.arange(4, dtype=np.int64)}
    as_torch = {k: torch.from_numpy(v.copy()) for k, v in arrays.items()}
    mixed = {k: (as_torch[k] if i % 2 else v) for i, (k, v) in enumerate(arrays.items())}
    path = str(tmp_path / "state.pth")
    torch.save(as_torch, path)
    for state in (as_torch, arrays, mixed, path):
        got = load_state(state)
        assert list(got) == list(arrays)
        for k, v in arrays.items():
            assert type(got[k]) is np.ndarray and got[k].dtype == v.dtype and np.array_equal(got[k], v), k
    as_torch["g"] = torch.ones(2, requires_grad=True)                                    # a parameter saved with its graph flag
    assert np.array_equal(load_state(as_torch)["g"], np.ones(2, dtype=np.float32))


def test_model_class_defaults():
    """a Model no arm has built yet answers every question asked of a built one, and closes"""
    from riser_amd.model import Model
    m = object.__new__(Model)
    assert m._h is None and m._seq is None and m.is_half is False
    assert m._lib_dtype is None and m._canonical is None and m._twin_source is None
    assert m._fc_positions == 0 and m._fc_hidden == 0
    assert m.close() is None
    assert m._h is None and m._seq is None
    assert callable(Model.autotune) and Model.autotune.__qualname__ == "Model.autotune"


def test_capture_needs_the_native_handle():
    """a family-backed Model has no `_h`: layer_rows and capture_layer refuse as layer_info does, before any library call"""
    import pytest
    from riser_amd.model import Model
    m = object.__new__(Model)
    with pytest.raises(NotImplementedError):
        m.layer_rows((4096, 5000), 1)
    with pytest.raises(NotImplementedError):
        with m.capture_layer(1, None):
            pass
