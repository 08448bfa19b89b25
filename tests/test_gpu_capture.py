"""Model.layer_rows and Model.capture_layer, the one layer-capture ritual every diagnostic and layer-wise test goes through:
the hook is off after the block whatever happened inside it, the library is told the buffer's size in BYTES whatever the
tensor's dtype, and the row count is the packed layout's.  The shipped 12-layer net on three ragged reads just over its
4096-sample minimum."""
import numpy as np
import pytest
import torch

from riser_amd import synth

pytestmark = pytest.mark.gpu

LENS = (4096, 4500, 5000)
PATTERN = 0xA5


@pytest.fixture(scope="module")
def rig():
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda", 0)
    m = Model(synth.make_state_dict(1), synth.Config(), None, "m", device=dev)
    sigs = [synth.make_signals(20260103, 1, n, first_read=900 + i)[0] for i, n in enumerate(LENS)]
    yield m, pack_reads(sigs, dev), dev
    m.close()


def _pattern(m, lens, layer, dtype, dev):
    """a buffer of conv layer `layer`'s output size in bytes, as `dtype`, every byte PATTERN"""
    rows, cp, fmt = m.layer_rows(lens, layer)
    assert fmt == 0 and m.dtype == "f32w"                               # fp32 rows: 4 bytes per padded channel
    nbytes = rows * cp * 4
    return torch.full((nbytes,), PATTERN, dtype=torch.uint8, device=dev).view(dtype)


def _bytes(t):
    return t.view(torch.uint8).cpu().numpy()


class _Boom(Exception):
    pass


def test_capture_layer_is_off_after_an_exception(rig):
    m, (sig, off, ln, lens), dev = rig
    cap = _pattern(m, lens, 1, torch.float32, dev)
    with pytest.raises(_Boom):
        with m.capture_layer(1, cap):
            first = m.classify_raw(sig, off, ln, lens).cpu().numpy()
            raise _Boom()
    assert not (_bytes(cap) == PATTERN).all()                           # the hook was on inside the block
    cap.view(torch.uint8).fill_(PATTERN)
    again = m.classify_raw(sig, off, ln, lens).cpu().numpy()
    torch.cuda.synchronize(dev)
    assert (_bytes(cap) == PATTERN).all(), "a call after the block wrote into the capture buffer"
    assert np.array_equal(again, first)


def test_capture_layer_counts_bytes_not_elements(rig):
    m, (sig, off, ln, lens), dev = rig
    got = {}
    for dtype in (torch.float32, torch.int16, torch.uint8):
        cap = _pattern(m, lens, 1, dtype, dev)
        with m.capture_layer(1, cap) as inside:
            assert inside is cap
            m.classify_raw(sig, off, ln, lens)
        got[dtype] = _bytes(cap)
    assert got[torch.float32].size == got[torch.int16].size == got[torch.uint8].size
    assert np.array_equal(got[torch.int16], got[torch.float32])
    assert np.array_equal(got[torch.uint8], got[torch.float32])
    # and those bytes are the whole layer: the last row of the last read's blocks is padding, written as zeros
    rows, cp, _ = m.layer_rows(lens, 1)
    assert not got[torch.float32].reshape(rows, cp * 4)[-1].any()


@pytest.mark.parametrize("lens", [LENS, (5000,) * 4], ids=["ragged", "uniform"])
def test_layer_rows_is_the_formula_it_replaces(rig, lens):
    m = rig[0]
    info = m.layer_info()
    for i in (1, 6, 11):
        U = m.block_samples(i)
        want = int(m.block_bases(lens, i)[-1]) * (U >> (i + 1))         # what every capture site computed by hand
        assert want == sum(n // U + 1 for n in lens) * (U >> (i + 1))
        assert m.layer_rows(lens, i) == (want, info[i]["cp_out"], info[i]["rows_format"])
        assert m.layer_rows(np.asarray(lens, dtype=np.int32), i) == m.layer_rows(list(lens), i)

