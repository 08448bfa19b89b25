"""The overflow guard's host pieces, without a GPU: the `on_overflow` keyword of SequencerControl, the mapping that withholds
the decisions of a saturated batch, the launcher's flag, and the predicate that says which dtype names are half precision."""
import logging
import types

import numpy as np
import pytest
import torch

from riser_amd import _native as nv
from riser_amd.fake_client import FakeClient

TRY_AGAIN, ACCEPT, REJECT, NO_DECISION = nv.RS_TRY_AGAIN, nv.RS_ACCEPT, nv.RS_REJECT, nv.RS_NO_DECISION


def _control(**kw):
    from riser_amd.control import SequencerControl
    proc = types.SimpleNamespace(device=torch.device("cuda", 0))          # the constructor only records the device
    return SequencerControl(FakeClient([]), [], proc, logging.getLogger("guard"), "unused", **kw)


def test_on_overflow_keyword():
    """three values construct, "warn" is the default, anything else is a ValueError in the constructor"""
    assert _control().on_overflow == "warn"
    for mode in ("warn", "reclassify", "try_again"):
        ctl = _control(on_overflow=mode)
        assert ctl.on_overflow == mode
        assert ctl.saturated_batches == ctl.reclassified_batches == ctl.withheld_batches == 0
        assert ctl.twins == ()                                         # no model, no twin; nothing touched the device
    for bad in ("bogus", "", None, "Warn"):
        with pytest.raises(ValueError, match="on_overflow"):
            _control(on_overflow=bad)


def test_withhold_decisions():
    """below max_len accept / reject -> try_again; at max_len -> no_decision; the undecided stay; a new array comes back"""
    from riser_amd.control import withhold_decisions
    max_len = 8615
    dec = np.array([ACCEPT, REJECT, TRY_AGAIN, NO_DECISION, ACCEPT, REJECT, TRY_AGAIN, NO_DECISION, ACCEPT], dtype=np.uint8)
    lens = np.array([4096, 8614, 5000, 8615, 8615, 8615, 8615, 8615, 9000], dtype=np.int32)
    before = dec.copy()
    out = withhold_decisions(dec, lens, max_len)
    assert out.tolist() == [TRY_AGAIN, TRY_AGAIN, TRY_AGAIN, NO_DECISION, NO_DECISION, NO_DECISION, TRY_AGAIN, NO_DECISION,
                            NO_DECISION]
    assert np.array_equal(dec, before) and out is not dec and out.dtype == np.uint8
    assert not np.isin(out, (ACCEPT, REJECT)).any()
    empty = withhold_decisions(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int32), max_len)
    assert empty.shape == (0,)
    # every combination of decision and side of max_len
    for d in (TRY_AGAIN, ACCEPT, REJECT, NO_DECISION):
        for n, want_decided in ((max_len - 1, TRY_AGAIN), (max_len, NO_DECISION)):
            got = int(withhold_decisions(np.array([d], dtype=np.uint8), np.array([n]), max_len)[0])
            assert got == (want_decided if d in (ACCEPT, REJECT) else d)


def test_launcher_flag():
    from riser_amd.launch import parse_args
    assert parse_args([]).on_overflow == "warn"
    for mode in ("warn", "reclassify", "try_again"):
        assert parse_args(["--on-overflow", mode]).on_overflow == mode
    with pytest.raises(SystemExit):
        parse_args(["--on-overflow", "bogus"])


def test_half_precision_is_a_property_of_the_library_dtype():
    """an alias of a half-precision mode is half precision: the predicate looks at the library dtype a name maps to"""
    from riser_amd.model import Model, is_half_dtype
    for name in ("f16", "fp16", "float16", "f16x3", "f16xf8"):
        assert is_half_dtype(name), name
    for name in ("f32", "f32w", "bf16", "bf16x3", "fp32", "float32", "bfloat16", "f32_winograd", "no_such_mode"):
        assert not is_half_dtype(name), name
    assert Model.HALF_MODES == ("f16", "f16x3", "f16xf8") and all(is_half_dtype(n) for n in Model.HALF_MODES)
    # the property of a model follows the library dtype it was created with (no device needed to ask)
    m = object.__new__(Model)
    assert not m.is_half
    m._lib_dtype = nv.RS_F16
    assert m.is_half
    m._lib_dtype = nv.RS_BF16X3
    assert not m.is_half
