"""What FamilyNet (riser_amd/_family.py) owns for the four device-program classes, each on its smallest net: the refusal of a
non-contiguous input, the split of a batch beyond max_batch, the growth of the workspace, close(), and the handle of a net
whose mode switch is refused at construction.  Results are compared as int32 views: equal means bit for bit."""
import types

import numpy as np
import pytest
import torch

from riser_amd import _native as nv
from riser_amd import crnn as CR
from riser_amd import gconv as G
from riser_amd import resnet as RN
from riser_amd import synth
from riser_amd import tcn as T
from tests import gconv_ref
from tests import test_resnet_shapes as TR

pytestmark = pytest.mark.gpu
LD = 256
LENS = [LD, LD - 1, 120, 131, 200]                   # every read above every net's minimum
RESNET = "s1_w8_np56"                                # test_resnet_shapes.py's smallest basic config: 12 and 56 channels, three blocks


def _tcn(dev, bottleneck):
    cfg = dict(in_channels=1, n_filters=20, kernel=3, dilation=2, n_layers=2, dropout=0.2, n_classes=2)
    sd = synth.make_tcn_state_dict(31, cfg, bottleneck)
    return T.TCNNet(*T.build_tcn_program(sd, types.SimpleNamespace(**cfg), bottleneck), device=dev)


def _crnn(dev):
    cfg = dict(n_conv_layers=2, channels=[6, 20], kernels=[5, 3], cell="lstm", hidden=24, n_rec_layers=1, bidirectional=True,
               dropout=0.2, n_classes=2)
    return CR.CRNNNet(CR.build_crnn_program(synth.make_crnn_state_dict(32, cfg), types.SimpleNamespace(**cfg)), device=dev)


def _gconv_prog(channels, kernels, depth):
    cfg = dict(n_layers=len(channels), depth=depth, channels=channels, kernels=kernels)
    return G.build_gconv_program(gconv_ref.make_state_dict(cfg, 33), gconv_ref.cnn_config(cfg))


def _gconv(dev):
    return G.GConvNet(_gconv_prog([6, 20], [5, 3], 2), device=dev)


def _resnet(dev):
    cfg, sd, prog, nb, fw, fb, c_last = TR.program(RESNET)
    return RN.SeqNet(prog, nb, fw, fb, c_last, device=dev)


MAKERS = {"tcn": lambda d: _tcn(d, False), "tcn_bot": lambda d: _tcn(d, True), "crnn": _crnn, "gconv": _gconv, "resnet": _resnet}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def batch(dev):
    """five reads in rows of LD samples, NaN behind every read: made once and left unchanged"""
    rng = np.random.default_rng(34)
    rows = np.full((len(LENS), LD), np.nan, np.float32)
    for b, L in enumerate(LENS):
        rows[b, :L] = rng.standard_normal(L).astype(np.float32)
    return torch.from_numpy(rows).to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev)


@pytest.fixture(params=list(MAKERS))
def net(request, dev):
    n = MAKERS[request.param](dev)
    yield n
    n.close()


def _bits(net, x, ln):
    probs, logits = net.forward_ragged(x, ln, return_logits=True)
    out = probs.cpu().numpy().view(np.int32), logits.cpu().numpy().view(np.int32)
    assert np.isfinite(out[1].view(np.float32)).all()
    return out


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_non_contiguous_input_is_refused_before_any_call(net, batch, monkeypatch):
    x, ln = batch
    view = x[:, ::2]
    assert not view.is_contiguous()

    def no_call(name):
        raise AssertionError(f"rs_*_{name} was asked for")
    monkeypatch.setattr(net, "_fn", no_call)
    with pytest.raises(ValueError, match="contiguous"):
        net.forward_ragged(view, ln)


def test_split_batch_keeps_its_bits(net, batch, monkeypatch):
    x, ln = batch
    whole = _bits(net, x, ln)
    monkeypatch.setattr(type(net), "max_batch", lambda self, L: 2)
    assert _same(_bits(net, x, ln), whole)


def test_workspace_grows_once(net, batch):
    x, ln = batch
    first = _bits(net, x[:2], ln[:2])
    small = net._ws
    _bits(net, x, ln)
    big = net._ws
    assert big is not small and big.numel() > small.numel()
    assert _same(_bits(net, x[:2], ln[:2]), first)
    assert net._ws is big


def test_close_twice_then_forward_is_refused_by_the_library(net, batch):
    x, ln = batch
    _bits(net, x, ln)
    net.close()
    net.close()
    assert net._h is None and net._ws is None
    with pytest.raises(nv.NativeError, match="rs_status -1"):          # RS_ERR_ARG: the null-handle check
        net.forward_ragged(x, ln)
    with pytest.raises(nv.NativeError, match="rs_status -1"):
        net.forward(x)


def test_refused_mode_at_construction_closes_the_handle(dev, batch):
    """a conv whose fp32 tile fits LDS and whose split form does not (tests/test_gconv_x3_cpu.py: x3_layout(8, 16, 73))"""
    x, ln = batch
    prog = _gconv_prog([8, 16], [5, 73], 1)
    net = G.GConvNet.__new__(G.GConvNet)
    with pytest.raises(nv.NativeError, match="rs_gconv_set_mode.*LDS"):
        net.__init__(prog, device=dev, dtype="bf16x3")
    assert net._h is None and net.dtype == "f32"
    live = G.GConvNet(prog, device=dev)              # the same net in fp32: the refusal leaves handle and mode as they were
    before = _bits(live, x, ln)
    with pytest.raises(nv.NativeError, match="rs_gconv_set_mode.*LDS"):
        live.set_mode("bf16x3")
    assert live._h is not None and live.dtype == "f32" and _same(_bits(live, x, ln), before)
    live.close()
