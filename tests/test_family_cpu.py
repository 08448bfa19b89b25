"""FamilyNet (riser_amd/_family.py) without a GPU: the four device-program classes refuse an unknown dtype before they ask for a
device, and their mode tables agree on the names of fp32."""
import pytest

from riser_amd import _native as nv
from riser_amd._family import FamilyNet
from riser_amd.crnn import CRNNNet
from riser_amd.gconv import GConvNet
from riser_amd.resnet import SeqNet
from riser_amd.tcn import TCNNet

# constructor arguments in front of (device, dtype): never looked at when the dtype is refused
CLASSES = {TCNNet: (None, None, None), CRNNNet: (None,), GConvNet: (None,), SeqNet: (None, 0, None, None, 0)}
SECOND_MODE = {TCNNet: "bf16x3", CRNNNet: "f16x3", GConvNet: "bf16x3", SeqNet: "bf16x3"}


@pytest.mark.parametrize("cls", list(CLASSES), ids=lambda c: c.__name__)
def test_unknown_dtype_is_refused_before_any_gpu_call(cls, monkeypatch):
    def no_gpu_call():
        raise AssertionError("the dtype is validated after the device was asked for")
    monkeypatch.setattr(nv, "require_gpu", no_gpu_call)
    monkeypatch.setattr(nv, "lib", no_gpu_call)
    for dt in ("int8", "f16", "F32", "", None):
        with pytest.raises(ValueError, match="dtype"):
            cls(*CLASSES[cls], device=None, dtype=dt)
    net = cls.__new__(cls)                          # set_mode on a net without a handle: refused before the library is called
    net._h = None
    with pytest.raises(ValueError, match="dtype"):
        net.set_mode("int8")


@pytest.mark.parametrize("cls", list(CLASSES), ids=lambda c: c.__name__)
def test_mode_table(cls):
    assert issubclass(cls, FamilyNet) and cls._PREFIX.startswith("rs_")
    names = {cls._MODES[n][0] for n in ("f32", "f32w", "fp32")}
    assert names == {"f32"}
    assert {cls._MODES[n][1] for n in ("f32", "fp32")} == {nv.RS_F32} and cls._MODES["f32w"][1] == nv.RS_F32W
    second = SECOND_MODE[cls]
    assert cls._MODES[second] == (second, getattr(nv, "RS_" + second.upper()))
    assert set(cls._MODES) == {"f32", "f32w", "fp32", second}
    for fn in ("create", "destroy", "set_mode", "max_batch", "workspace_bytes", "forward_ragged"):
        assert f"{cls._PREFIX}_{fn}" in nv.SYMBOLS
