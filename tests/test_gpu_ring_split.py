"""The 16-bit ring kernel's head + tail launches (RS_RING_TAIL_SPLIT=1), which no default run takes: same bits as one launch."""
import re

import pytest
import torch

from riser_amd import synth
from riser_amd.model import Model
from riser_amd.preprocess import pack_reads

from conftest import hooked_model

# the smallest batch of 16000-sample reads at which the planner splits a ring layer once every candidate split priced below one
# launch is taken (a split needs more than one round of tiles over the CUs: layer 5 at 129 reads in split precision, layer 7 at
# 257 in plain f16; one read fewer and no layer splits)
SMALLEST = {"bf16x3": 129, "f16": 257}
SPLIT_ENV = {"RS_RING_TAIL_SPLIT": "1", "RS_THIN_H16_ROWS": "0", "RS_TAIL_MARGIN": "10", "RS_TAIL_DEBUG": "1"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16x3", "f16"])
def test_ring_head_and_tail_launches_keep_the_bits(dev, capfd, dtype):
    """Probabilities and logits of a run with ring layers split into a head and a tail launch equal those of a default run on
    the same inputs BIT FOR BIT.  That holds because, within one mode, the accumulation order of an output does not depend on
    the tile shape that computes it (include/riser_amd.h, rs_autotune: "results are bit-identical whatever shape runs") - which
    is what "same bits" means here: one mode, any launch plan."""
    B = SMALLEST[dtype]
    sd = synth.make_state_dict(1)
    sig, off, ln, lh = pack_reads(list(synth.make_signals(20260103, B, 16000)), dev)
    m = Model(sd, synth.Config(), None, "m", dtype=dtype, device=dev)
    want = m.classify_raw(sig, off, ln, lh, return_logits=True)
    torch.cuda.synchronize(dev)
    m.close()
    split = hooked_model(SPLIT_ENV, sd, dtype, dev)
    capfd.readouterr()
    got = split.classify_raw(sig, off, ln, lh, return_logits=True)
    torch.cuda.synchronize(dev)
    err = capfd.readouterr().err
    split.close()
    layers = [int(v) for v in re.findall(r"\[tail-split\] layer (\d+) \(ring\):", err)]
    print(f"\nRING_SPLIT {dtype} {B} reads: head + tail launches in layers {layers}")
    assert layers, (f"no ring layer ran as head + tail launches at {B} reads: SMALLEST holds for 256 CUs and the cost constants of "
                    f"csrc/conv_ring_h16.hip (a layer's tiles first exceed one round of the CUs one read past 128 / 256)", err[-2000:])
    assert not re.findall(r"\[tail-split\] layer (\d+):", err)          # the fp32 kernels' form of the line is not the ring's
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
