"""Parity of the HIP path (through the C ABI) against the CPU oracle and the golden fixtures
recorded from the reference.  Bars: normalise / polyA / decisions bit-exact; probabilities
within 1e-3 of the reference's fp32 torch-CPU path (north_star), labels identical at 0.9."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest
import torch

from oracle import riser_oracle as ro
from riser_amd import _native as nv
from riser_amd import synth
from riser_amd.fake_client import FakeClient, FakeRead

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-3          # north_star: class probabilities within 1e-3 (fp32)
SIG_SEED = 20260103


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def proc(dev):
    from riser_amd.preprocess import Kit, SignalProcessor
    return SignalProcessor(Kit.create_from_version("RNA004"), device=dev)


_models = {}


def get_model(seed, dev, target="mRNA"):
    from riser_amd.model import Model
    if seed not in _models:
        _models[seed] = Model(synth.make_state_dict(seed), synth.Config(), logging.getLogger("t"), target, device=dev)
    return _models[seed]


# ------------------------------------------------------------------------------------------
# normalise
# ------------------------------------------------------------------------------------------
def test_normalise_golden_bit_exact(proc, golden_dir):
    g = np.load(os.path.join(golden_dir, "normalise.npz"))
    names = [str(n) for n in g["names"]]
    sigs = [g[f"{n}.sig"] for n in names]
    outs, stats = proc.mad_normalise_batch(sigs, return_stats=True)
    for i, n in enumerate(names):
        want = g[f"{n}.out"]
        assert np.array_equal(stats[i], g[f"{n}.stats"]), n
        if want.dtype == np.int64:                         # mad == 0 -> zeros
            assert not outs[i].any(), n
        else:
            assert np.array_equal(outs[i], want), n
        one = proc.mad_normalise(sigs[i])                  # the reference's single-read surface
        assert one.dtype == want.dtype and np.array_equal(one, want), n


def test_normalise_random_vs_oracle(proc):
    rng = np.random.default_rng(5)
    sigs = []
    for i in range(40):
        n = int(rng.integers(2, 20000))
        kind = i % 4
        if kind == 0:        # full int16 range: exercises the two-pass (shift > 0) select
            s = rng.integers(-32768, 32768, n)
        elif kind == 1:      # narrow, many ties
            s = rng.integers(480, 520, n)
        elif kind == 2:      # heavy tails
            s = (500 + 40 * rng.standard_t(2, n)).clip(-32768, 32767)
        else:
            s = synth.make_signals(SIG_SEED + i, 1, n)[0]
        sigs.append(np.asarray(s, dtype=np.int16))
    sigs.append(np.array([7], dtype=np.int16))
    sigs.append(np.array([-32768, 32767, 0, 0, 1], dtype=np.int16))
    outs = proc.mad_normalise_batch(sigs)
    for s, o in zip(sigs, outs):
        w = ro.mad_normalise(s)
        assert np.array_equal(o, w.astype(np.float64)), (len(s), s[:8])


def test_normalise_adversarial_small_arrays(proc):
    """Many short, adversarial reads in one launch: heavy ties (MAD = 0 and near-0), two-valued signals, outlier
    runs touching both ends, half-integer medians, extreme int16 values, lengths 1..400 - every one bit-exact
    (values and dtype rule) against the oracle restatement of riser/preprocess.py:108-147."""
    rng = np.random.default_rng(20261003)
    sigs = []
    for i in range(600):
        n = int(rng.integers(1, 400))
        kind = i % 8
        if kind == 0:
            s = np.full(n, int(rng.integers(-300, 900)))                          # constant: MAD = 0
        elif kind == 1:
            s = rng.choice([500, 501], size=n)                                     # two values, many ties
        elif kind == 2:
            s = rng.integers(495, 506, n)
            s[rng.random(n) < 0.3] = int(rng.integers(1500, 4000))                 # dense spikes: runs of outliers
        elif kind == 3:
            s = rng.integers(400, 600, n)
            k = int(rng.integers(1, 6))
            s[:k] = 4000                                                           # outlier run at the left end
            s[-k:] = -2000                                                         # ... and at the right end
        elif kind == 4:
            s = rng.choice([-32768, 32767, 0], size=n)
        elif kind == 5:
            s = np.sort(rng.integers(0, 50, n))                                    # sorted: median between equal neighbours
        elif kind == 6:
            s = rng.integers(500, 503, n)
            s[rng.integers(0, n)] = 30000                                          # one huge spike, MAD of 0 or 1
        else:
            s = (500 + 60 * rng.standard_normal(n)).round()
        sigs.append(np.asarray(s, dtype=np.int16))
    outs, stats = proc.mad_normalise_batch(sigs, return_stats=True)
    for s, o, st in zip(sigs, outs, stats):
        w = ro.mad_normalise(s)
        assert np.array_equal(o, np.asarray(w, dtype=np.float64)), (len(s), s[:10])
        med = np.median(s)
        assert st[0] == med and st[1] == np.median(np.abs(s - med)), (len(s), st)


def test_normalise_max_length_and_errors(proc):
    s = synth.make_signals(3, 1, 65536)[0]
    assert np.array_equal(proc.mad_normalise(s), ro.mad_normalise(s))
    with pytest.raises(ValueError):
        proc.mad_normalise(np.zeros(0, dtype=np.int16))
    with pytest.raises(ValueError):
        proc.mad_normalise(np.zeros(65537, dtype=np.int16))
    z = proc.mad_normalise(np.zeros(10, dtype=np.float32))               # float input is accepted; mad == 0 -> int64 zeros
    assert z.dtype == np.int64 and not z.any()


def test_normalise_fp32_device_output(proc, dev):
    from riser_amd.preprocess import pack_reads
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=i)[0] for i, n in enumerate((4096, 5001, 9000))]
    sig, off, ln, lens = pack_reads(sigs, dev)
    x = proc.normalise_device(sig, off, ln, 3, 9000, pad_to=12288).cpu().numpy()
    for i, s in enumerate(sigs):
        w = ro.mad_normalise(s).astype(np.float32)
        assert np.array_equal(x[i, :len(s)], w) and not x[i, len(s):].any()


def test_normalise_float_inputs_golden(proc, golden_dir):
    """SignalProcessor.mad_normalise on float16 / float32 / float64 signals (riser/preprocess.py:108-115 accepts any
    numeric array; the retrain path feeds pA-scaled floats): dtype and bits of the reference, singly and batched; long
    doubles and mixed batches are refused"""
    g = np.load(os.path.join(golden_dir, "normalise_float.npz"))
    cases = synth.normalise_float_cases()
    for name, x in cases:
        want = g[f"{name}.out"]
        got = proc.mad_normalise(x.copy())
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    for dt in ("float16", "float32", "float64"):
        pick = [(n, x) for n, x in cases if n.endswith(dt) and "mad0" not in n]
        outs = proc.mad_normalise_float_batch([x for _, x in pick])
        for (n, _), o in zip(pick, outs):
            assert np.array_equal(o, g[f"{n}.out"]), n
    with pytest.raises(TypeError):
        proc.mad_normalise(np.ones(100, dtype=np.longdouble))
    with pytest.raises(TypeError):
        proc.mad_normalise_float_batch([np.ones(10, np.float32), np.ones(10, np.float64)])
    with pytest.raises(ValueError):
        proc.mad_normalise(np.zeros(0, dtype=np.float32))


SMALL_FLOAT_LENGTHS = (2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023)
TIED_ADC = (470, 485, 500, 515, 540)


def small_float_reads(dt):
    """per length a noisy read (mixed sign, an outlier at each end and a run of three where n > 8) and a read of five distinct
    values: with n / 5 samples on each, the two middle order statistics of an even n are equal, of the values and of their
    deviations.  Two or three samples with a non-zero MAD are all distinct, so those lengths draw without replacement."""
    rng = np.random.default_rng(20261019)
    base, tied = [], []
    for n in SMALL_FLOAT_LENGTHS:
        s = 500 + rng.integers(-15, 16, (4, n)).sum(0)
        if n > 8:
            s[0], s[n - 1] = 2500, -900
            s[n // 2: n // 2 + 3] = (2000, -1500, 2200)
        base.append((s * 0.17548 - 80.0).astype(dt))
        t = rng.choice(np.array(TIED_ADC), size=n, replace=n > 3)
        tied.append((t * 0.17548 - 80.0).astype(dt))
    return base, tied


@pytest.mark.parametrize("dt", ["float16", "float32", "float64"])
def test_normalise_float_small_shapes(proc, dt):
    """rs_normalise_float below the 3690 samples of the golden cases, where the shared select's wave-level edges sit: partly
    filled waves, waves without an element, and the next_same / min-reduction branch of an even n; one batch per dtype, each row
    and its (median, MAD) bit for bit against the oracle and numpy"""
    base, tied = small_float_reads(dt)
    for x in tied[3:]:
        if len(x) % 2 == 0:
            v = np.sort(x)
            assert v[len(x) // 2 - 1] == v[len(x) // 2], len(x)
    reads = base + tied
    outs, stats = proc.mad_normalise_float_batch(reads, return_stats=True)
    for x, o, st in zip(reads, outs, stats):
        med = np.median(x)
        mad = np.median(np.abs(x - med))
        assert mad != 0 and np.isfinite(x).all(), len(x)                      # no row takes the int64-zeros path
        want = ro.mad_normalise(x)
        assert want.dtype == x.dtype and np.isfinite(want).all(), len(x)
        assert o.dtype == want.dtype and np.array_equal(o, want), (dt, len(x))
        assert st[0] == med and st[1] == mad, (dt, len(x), st)


# ------------------------------------------------------------------------------------------
# polyA
# ------------------------------------------------------------------------------------------
def test_polya_golden(proc, golden_dir):
    cases = np.load(os.path.join(golden_dir, "polya.npz"))["cases"]
    sigs = [synth.make_raw_read(int(s), int(r), int(n), bool(p)) for s, r, n, p, _ in cases]
    got = proc.get_polyA_end_batch(sigs)
    assert np.array_equal(got, cases[:, 4])
    assert proc.get_polyA_end(sigs[3]) is None and proc.get_polyA_end(sigs[0]) == cases[0, 4]
    assert proc.get_polyA_end(np.zeros(100, dtype=np.int16)) is None          # shorter than one window
    cache = {}
    trimmed, ok = proc.trim_polyA(sigs[0], "r0", cache)
    assert ok and cache == {"r0": int(cases[0, 4])} and len(trimmed) == len(sigs[0]) - cases[0, 4] - 1


def test_polya_edge_cases_golden(proc, golden_dir):
    """the reference's answers on the corners of the window rule, incl. reads longer than 65536 samples and the
    kernel's own 128-window table boundary; as single reads and as one ragged batch"""
    g = np.load(os.path.join(golden_dir, "polya.npz"))
    want = g["edge_ends"]
    cases = synth.polya_edge_cases()
    assert [n for n, _ in cases] == [str(n) for n in g["edge_names"]]
    got = proc.get_polyA_end_batch([s for _, s in cases])
    assert np.array_equal(got, want), dict(zip(g["edge_names"], zip(got, want)))
    for (name, s), w in zip(cases, want):
        e = proc.get_polyA_end(s)
        assert (-1 if e is None else e) == w, name


def test_polya_random_vs_oracle(proc):
    rng = np.random.default_rng(11)
    sigs = [synth.make_raw_read(1234, i, int(rng.integers(600, 30000)), bool(i % 3)) for i in range(48)]
    got = proc.get_polyA_end_batch(sigs)
    for s, e in zip(sigs, got):
        w = ro.polya_end(s)
        assert e == (-1 if w is None else w)


def test_polya_resume_equals_full_scan(proc, dev):
    """rs_polya_end_resume: 160 reads seen again and again, longer each time (300 ... 2600 more samples per visit, as a read
    that stays in its pore between ReadUntil batches) - scanning only the new windows from the state of the previous visit
    gives, at EVERY visit, the end the oracle finds on the whole prefix, and the state a scan from the first sample returns.
    Reads with and without a poly(A), threshold-riding windows (the fuzz generator), visits that add less than one window,
    a state that belongs to a longer read (ignored), and reads past the kernel's 128-window table."""
    from riser_amd.preprocess import pack_reads
    rng = np.random.default_rng(20260109)
    reads = [synth.make_raw_read(977, i, int(rng.integers(3000, 30000)), bool(i % 4)) for i in range(120)]
    for k in range(36):                                                       # windows whose MAD / mean ride the thresholds
        level, parts = float(rng.integers(300, 700)), []
        for w in range(int(rng.integers(6, 50))):
            level = min(max(level * float(rng.choice([1.0, 1.0, 1.21, 1.25, 0.8])), 150.0), 6000.0)
            parts.append(np.round(rng.normal(level, 29.65 * float(rng.uniform(0.93, 1.07)), 500)))
        reads.append(np.clip(np.concatenate(parts), -32768, 32767).astype(np.int16))
    reads += [synth.make_raw_read(978, i, 70000 + 777 * i, bool(i % 2)) for i in range(4)]   # > 128 windows
    B = len(reads)
    seen = np.array([int(rng.integers(200, 1500)) for _ in reads])
    state = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    for visit in range(14):
        pre = [r[:n] for r, n in zip(reads, seen)]
        sig, off, ln, _ = pack_reads(pre, dev)
        ends, state_out = proc.polyA_end_device(sig, off, ln, B, state_in=state)
        full, state_full = proc.polyA_end_device(sig, off, ln, B, state_in=torch.zeros_like(state))
        ends = ends.cpu().numpy()
        want = np.array([-1 if (e := ro.polya_end(p)) is None else e for p in pre])
        assert np.array_equal(ends, want), (visit, np.flatnonzero(ends != want)[:8])
        assert np.array_equal(full.cpu().numpy(), want)
        none = want < 0                                                       # the state is only defined while no end is found
        assert torch.equal(state_out[torch.from_numpy(none).to(dev)], state_full[torch.from_numpy(none).to(dev)]), visit
        assert np.array_equal(state_out.cpu().numpy()[none, 0], (seen // 500)[none])
        state = state_out
        seen = np.minimum(seen + rng.integers(300, 2600, size=B) * (rng.random(B) < 0.85), [len(r) for r in reads])
    # a state that claims more windows than the read has is not the read's: scanned whole
    pre = [r[:1700] for r in reads[:8]]
    sig, off, ln, _ = pack_reads(pre, dev)
    bogus = torch.tensor([[40, 1500, 1, 1]] * 8, dtype=torch.int32, device=dev)
    ends, _ = proc.polyA_end_device(sig, off, ln, 8, state_in=bogus)
    assert np.array_equal(ends.cpu().numpy(), [-1 if (e := ro.polya_end(p)) is None else e for p in pre])


def test_polya_fuzz_threshold_windows(proc):
    """400 reads built so that the detector's decisions hang on the EXACT window statistics: every 500-sample window has a
    MAD within a few percent of the rule's threshold (20) and a mean within a few percent of the +20 % step the start rule
    looks for - heavy ties (values quantised to 1 ... 8 counts), constant windows, windows with int16 extremes.  A window
    median or MAD off by one half count (the in-register sort, the sorted-window MAD formula of csrc/polya.hip) moves the
    end index of many of them."""
    rng = np.random.default_rng(20260108)
    sigs = []
    for k in range(400):
        nw = int(rng.integers(3, 60))
        level = float(rng.integers(300, 700))
        parts = []
        for w in range(nw):
            level *= float(rng.choice([1.0, 1.0, 1.19, 1.21, 1.25, 0.8, 0.9]))
            level = min(max(level, 150.0), 6000.0)
            sd = 29.65 * float(rng.uniform(0.93, 1.07))                       # MAD = 0.6745 sd: 18.6 ... 21.4
            q = int(rng.choice([1, 1, 2, 4, 8]))
            x = np.round(rng.normal(level, sd, 500) / q) * q
            r = rng.random()
            if r < 0.05:
                x[:] = np.round(level)                                        # constant window: MAD 0
            elif r < 0.10:
                x[rng.integers(0, 500, size=3)] = rng.choice([-32768, 32767])
            elif r < 0.15:
                x[:251] = np.round(level) - 20; x[251:] = np.round(level) + 21   # MAD exactly at / next to the threshold
            parts.append(x)
        tail = rng.normal(level, 30, int(rng.integers(0, 500)))               # a last partial window (ignored by the rule)
        sigs.append(np.clip(np.concatenate(parts + [tail]), -32768, 32767).astype(np.int16))
    got = proc.get_polyA_end_batch(sigs)
    want = np.array([-1 if (e := ro.polya_end(s)) is None else e for s in sigs])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want > 0).sum() > 100 and (want < 0).sum() > 20                   # both outcomes are exercised


# ------------------------------------------------------------------------------------------
# network
# ------------------------------------------------------------------------------------------
def test_forward_golden(dev, golden_dir):
    net = np.load(os.path.join(golden_dir, "network.npz"))
    worst = 0.0
    for seed, L, B, first in net["cases"]:
        tag = f"s{seed}_L{L}_B{B}_r{first}"
        sigs = synth.make_signals(int(net["sig_seed"][0]), int(B), int(L), first_read=int(first))
        m = get_model(int(seed), dev)
        xs = [ro.mad_normalise(s) for s in sigs]
        probs, logits = m.classify_batch(xs, return_logits=True)
        probs, logits = probs.cpu().numpy(), logits.cpu().numpy()
        want = net[f"{tag}.probs"]
        err = float(np.abs(probs - want).max())
        worst = max(worst, err)
        assert err < PROB_TOL, (tag, err)
        assert np.array_equal(probs[:, 1] > 0.9, want[:, 1] > 0.9), tag
        assert np.allclose(logits, net[f"{tag}.logits"], atol=2e-3), tag
    print("worst |dp| vs reference:", worst)


def test_classify_single_read_surface(dev):
    """Model.classify(signal) keeps riser/model.py:22-28: Tensor[2] on the device, (p_off, p_on)."""
    m = get_model(1, dev)
    s = synth.make_signals(SIG_SEED, 1, 8615, first_read=3)[0]
    x = ro.mad_normalise(s)
    p = m.classify(x)
    assert isinstance(p, torch.Tensor) and p.shape == (2,) and p.dtype == torch.float32 and p.is_cuda
    p_off, p_on = p
    want = ro.classify(synth.make_state_dict(1), x)
    assert abs(p_on.item() - want[1]) < PROB_TOL and abs(p_off.item() + p_on.item() - 1) < 1e-6
    assert bool(p_on > 0.9) == bool(want[1] > 0.9)
    z = m.classify(np.zeros(4096, dtype=np.int64))          # the mad == 0 array of the reference
    assert abs(z[1].item() - ro.classify(synth.make_state_dict(1), np.zeros(4096, dtype=np.int64))[1]) < PROB_TOL


def test_mixed_lengths_batch_and_permutation(dev):
    m = get_model(2, dev)
    lens = [4096, 4097, 4099, 5000, 6023, 6024, 8191, 8192, 8193, 8615, 11999, 12048, 15999, 16000, 16383, 16384, 20001]
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=50 + i)[0] for i, n in enumerate(lens)]
    xs = [ro.mad_normalise(s) for s in sigs]
    sd = synth.make_state_dict(2)
    want = np.stack([ro.classify(sd, x) for x in xs])
    got = m.classify_batch(xs).cpu().numpy()
    assert np.abs(got - want).max() < PROB_TOL
    perm = np.random.default_rng(0).permutation(len(xs))
    got_p = m.classify_batch([xs[i] for i in perm]).cpu().numpy()
    assert np.array_equal(got_p, got[perm]), "per-read result must not depend on batch position"
    for i in (0, 9, 16):
        assert np.array_equal(m.classify_batch([xs[i]]).cpu().numpy()[0], got[i]), "batch of 1 == batched"


def test_fused_raw_path_vs_oracle(dev):
    from riser_amd.preprocess import pack_reads
    m = get_model(3, dev)
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=200 + i)[0] for i, n in enumerate((16000, 4096, 12000, 8000, 9999))]
    sig, off, ln, lens = pack_reads(sigs, dev)
    got = m.classify_raw(sig, off, ln, lens).cpu().numpy()
    want = ro.classify_reads(synth.make_state_dict(3), sigs)
    assert np.abs(got - want).max() < PROB_TOL
    # a trim is an offset: classify sigs[0][1234:1234+8000] in place
    off2 = torch.tensor([1234], dtype=torch.int64, device=dev)
    ln2 = torch.tensor([8000], dtype=torch.int32, device=dev)
    got2 = m.classify_raw(sig, off2, ln2, np.array([8000], dtype=np.int32)).cpu().numpy()
    want2 = ro.classify_reads(synth.make_state_dict(3), [sigs[0][1234:9234]])
    assert np.abs(got2 - want2).max() < PROB_TOL


def test_too_short_and_bad_args(dev):
    m = get_model(1, dev)
    with pytest.raises(ValueError):
        m.classify(np.zeros(4095))                           # torch raises in max_pool1d for the reference
    with pytest.raises(ValueError):
        m.classify_batch([])
    L = nv.lib()
    x = torch.zeros((1, 4096), device=dev)
    ln = torch.tensor([4096], dtype=torch.int32, device=dev)
    out = torch.zeros((1, 2), device=dev)
    ws = torch.zeros(1024, dtype=torch.uint8, device=dev)
    rc = L.rs_forward(m._h, x.data_ptr(), 4096, ln.data_ptr(), None, 1, 4096, 4096, ws.data_ptr(), ws.numel(), out.data_ptr(), None, None)
    assert rc == -5 and b"workspace" in L.rs_last_error()
    h = C.c_void_p()
    ch = (C.c_int32 * 2)(4, 4)
    w = np.zeros(64, dtype=np.float32)
    wp = (C.c_void_p * 2)(w.ctypes.data, w.ctypes.data)
    assert L.rs_model_create(2, ch, 3, wp, wp, w.ctypes.data, w.ctypes.data, 0, 0, C.byref(h)) == -1     # n_classes != 2


def test_small_custom_network(dev):
    """the kernels are generic over the channel list (config.cnn.channels), not only the shipped one."""
    from riser_amd.model import Model
    rng = np.random.default_rng(3)
    channels = [8, 13, 21, 40, 70, 17]
    sd, c_in = {}, 1
    for i, c in enumerate(channels):
        sd[f"layers.{i}.0.weight"] = (rng.standard_normal((c, c_in, 3)) * np.sqrt(2.0 / (3 * c_in))).astype(np.float32)
        sd[f"layers.{i}.0.bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        c_in = c
    sd["classifier.2.weight"] = rng.standard_normal((2, c_in)).astype(np.float32)
    sd["classifier.2.bias"] = rng.standard_normal(2).astype(np.float32)
    cfg = synth.Config(synth.CnnConfig(channels=channels, kernels=[3] * 6))
    m = Model(sd, cfg, None, "x", device=dev)
    xs = [rng.standard_normal(n).astype(np.float64) for n in (64, 65, 100, 777, 2048)]
    got = m.classify_batch(xs).cpu().numpy()
    want = np.stack([ro.classify(sd, x) for x in xs])
    assert np.abs(got - want).max() < 1e-4
    m.close()


# ------------------------------------------------------------------------------------------
# 16-bit MFMA conv variants (BASELINE configs 3 / 5), fp32 accumulate.
#   bf16x3 / f16x3  split precision (hi + lo pairs, three MFMAs per product): THE 16-bit modes that claim configs 3 / 5.
#                   Bar = north_star's: probabilities within 1e-3 of the reference, accept / reject labels identical.
#   f16 / bf16      plain 16-bit activations + weights: labelled "fast, approximate"; they do NOT meet 1e-3
#                   (measured 7e-3 / 6e-2 worst over 512 reads) and are tested against their own measured envelope.
# ------------------------------------------------------------------------------------------
X3_TOL = 1e-3                                # north_star
# what the split-precision modes achieve on these weights (a regression guard, not the specification): bf16x3 carries 16
# mantissa bits, f16x3 22 - all of them since its weights are packed with a power-of-two scale (round 4: 3.5e-5 before)
# f16xf8 (round 6): f16x3 whose wide layers (7-11) evaluate the cross terms hi*lo + lo*hi as one block-scaled e4m3 product on the
# 8-bit MFMA - CPU emulation of every rounding (tools/fp8_cross_accuracy.py): 2.4e-4 with ALL tiled layers in that form
X3_ACHIEVED = {"bf16x3": 3e-4, "f16x3": 3e-5, "f16xf8": 4e-4}
H16_TOL = {"f16": 2e-2, "bf16": 1.5e-1, "bf16x3": X3_TOL, "f16x3": X3_TOL, "f16xf8": X3_TOL}


@pytest.mark.parametrize("dtype", ["bf16x3", "f16x3", "f16xf8"])
def test_split_precision_forward_vs_reference(dev, golden_dir, dtype):
    """every golden case of the reference (14 (seed, length, batch) cases incl. 64 x 6024 and 32 x 16000), through
    rs_forward (conv0 kernel + ring kernel on layers 1-11) and through rs_classify on the raw signals: probabilities
    within 1e-3, labels at 0.9 identical - the same bars as the fp32 path"""
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    net = np.load(os.path.join(golden_dir, "network.npz"))
    models = {}
    worst = 0.0
    for seed, L, B, first in net["cases"]:
        tag = f"s{seed}_L{L}_B{B}_r{first}"
        seed = int(seed)
        if seed not in models:
            models[seed] = Model(synth.make_state_dict(seed), synth.Config(), None, "m", dtype=dtype, device=dev)
        sigs = synth.make_signals(int(net["sig_seed"][0]), int(B), int(L), first_read=int(first))
        want = net[f"{tag}.probs"]
        probs = models[seed].classify_batch([ro.mad_normalise(s) for s in sigs]).cpu().numpy()
        sig, off, ln, lh = pack_reads(list(sigs), dev)
        fused = models[seed].classify_raw(sig, off, ln, lh).cpu().numpy()
        for got in (probs, fused):
            assert np.isfinite(got).all()
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err < X3_TOL, (tag, err)
            assert np.array_equal(got[:, 1] > 0.9, want[:, 1] > 0.9), tag
    print(f"{dtype}: worst |dp| {worst:.2e} over the golden cases, no label differs")
    assert worst < X3_ACHIEVED[dtype], (dtype, worst)
    for m in models.values():
        m.close()


@pytest.mark.parametrize("dtype", ["bf16x3", "f16x3", "f16xf8"])
def test_split_precision_full_size_batch(dev, dtype):
    """BASELINE config 3 / 5 shapes at full size: 512 x 16000 (and the mixed 2 s / 3 s / 4 s batch) in split precision,
    ALL 512 reads against the oracle (and against the library's own fp32 path), plus the size-independent properties:
    idempotence, sub-batch and read-order invariance, bit for bit."""
    from conftest import oracle_bench_batch
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    B, L = 512, 16000
    sd = synth.make_state_dict(1)
    m = Model(sd, synth.Config(), None, "m", dtype=dtype, device=dev)
    ref = get_model(1, dev)
    sigs = synth.make_signals(SIG_SEED, B, L)
    sig, off, ln, lens = pack_reads(list(sigs), dev)
    for name in ("full", "mixed"):
        if name == "mixed":
            lens = np.array([(8000, 12000, 16000)[i % 3] for i in range(B)], dtype=np.int32)
            off = torch.from_numpy(np.arange(B, dtype=np.int64) * L).to(dev)
            ln = torch.from_numpy(lens).to(dev)
        got = m.classify_raw(sig, off, ln, lens).cpu().numpy()
        oracle = oracle_bench_batch(1, name)
        assert np.abs(got - oracle).max() < X3_TOL, (name, float(np.abs(got - oracle).max()))
        assert np.array_equal(got[:, 1] > 0.9, oracle[:, 1] > 0.9), name
        want = ref.classify_raw(sig, off, ln, lens).cpu().numpy()
        assert np.abs(got - want).max() < X3_ACHIEVED[dtype], (name, float(np.abs(got - want).max()))
        assert np.array_equal(got, m.classify_raw(sig, off, ln, lens).cpu().numpy())
        idx = torch.arange(100, 164, device=dev)
        part = m.classify_raw(sig, off[idx].contiguous(), ln[idx].contiguous(), lens[100:164]).cpu().numpy()
        assert np.array_equal(part, got[100:164])
        ridx = torch.arange(B - 1, -1, -1, device=dev)
        rev = m.classify_raw(sig, off[ridx].contiguous(), ln[ridx].contiguous(), lens[::-1].copy()).cpu().numpy()
        assert np.array_equal(rev[::-1], got)
    assert (got[:, 1] > 0.9).sum() > 10 and (got[:, 1] < 0.1).sum() > 10
    m.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_h16_forward_vs_reference(dev, golden_dir, dtype):
    """probabilities of the 16-bit paths against the reference's fp32 golden values; label flips
    at 0.9 are counted and must stay rare and confined to reads within the tolerance of 0.9."""
    from riser_amd.model import Model
    net = np.load(os.path.join(golden_dir, "network.npz"))
    tol = H16_TOL[dtype]
    models = {}
    worst, flips, total = 0.0, 0, 0
    for seed, L, B, first in net["cases"]:
        tag = f"s{seed}_L{L}_B{B}_r{first}"
        seed = int(seed)
        if seed not in models:
            models[seed] = Model(synth.make_state_dict(seed), synth.Config(), None, "m", dtype=dtype, device=dev)
        sigs = synth.make_signals(int(net["sig_seed"][0]), int(B), int(L), first_read=int(first))
        xs = [ro.mad_normalise(s) for s in sigs]
        probs = models[seed].classify_batch(xs).cpu().numpy()
        want = net[f"{tag}.probs"]
        assert np.isfinite(probs).all()
        err = np.abs(probs - want).max(axis=1)
        worst = max(worst, float(err.max()))
        assert err.max() < tol, (tag, float(err.max()))
        fl = (probs[:, 1] > 0.9) != (want[:, 1] > 0.9)
        assert (np.abs(want[fl, 1] - 0.9) < tol).all(), "a flipped label must sit within tol of the threshold"
        flips += int(fl.sum())
        total += len(fl)
    print(f"{dtype}: worst |dp| {worst:.2e}, label flips {flips}/{total}")
    assert flips <= max(2, total // 25)
    for m in models.values():
        m.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16", "bf16x3", "f16x3", "f16xf8"])
def test_h16_mixed_lengths_and_determinism(dev, dtype):
    from riser_amd.model import Model
    m = Model(synth.make_state_dict(2), synth.Config(), None, "m", dtype=dtype, device=dev)
    lens = [4096, 4097, 5000, 6024, 8000, 8615, 12000, 16000, 16001, 20000]
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=300 + i)[0] for i, n in enumerate(lens)]
    xs = [ro.mad_normalise(s) for s in sigs]
    want = np.stack([ro.classify(synth.make_state_dict(2), x) for x in xs])
    got = m.classify_batch(xs).cpu().numpy()
    assert np.abs(got - want).max() < H16_TOL[dtype]
    perm = np.random.default_rng(1).permutation(len(xs))
    assert np.array_equal(m.classify_batch([xs[i] for i in perm]).cpu().numpy(), got[perm])
    assert np.array_equal(m.classify_batch([xs[3]]).cpu().numpy()[0], got[3])
    m.close()


# ------------------------------------------------------------------------------------------
# decision + control loop
# ------------------------------------------------------------------------------------------
def test_decide_matches_reference_rule(dev):
    rng = np.random.default_rng(9)
    B, nm = 257, 3
    p_on = rng.random((nm, B)).astype(np.float32)
    p_on[:, :40] = np.float32(0.9)                           # exactly at the threshold: strict >
    probs = np.stack([1 - p_on, p_on], axis=2).astype(np.float32)
    lens = rng.choice([5000, 8614, 8615, 9000], B).astype(np.int32)
    for mode in ("enrich", "deplete"):
        for thr in (0.9, 0.5):
            out = torch.empty(B, dtype=torch.uint8, device=dev)
            pt = torch.from_numpy(probs).to(dev)
            lt = torch.from_numpy(lens).to(dev)
            nv.check(nv.lib().rs_decide(pt.data_ptr(), nm, B, lt.data_ptr(), 8615, thr,
                                        nv.RS_ENRICH if mode == "enrich" else nv.RS_DEPLETE, out.data_ptr(), None), "d")
            got = out.cpu().numpy()
            for b in range(B):
                t32 = torch.tensor(thr)                      # torch compares fp32 tensor > python float
                want = ro.decide([p for p in probs[:, b, 1]], [p for p in probs[:, b, 0]], float(np.float32(thr)), mode, int(lens[b]), 8615)
                assert nv.DECISION_NAMES[got[b]] == want, (mode, thr, b)


def _build_batches(script, seed):
    return [[(ch, FakeRead(rid_s, synth.make_raw_read(seed, rid, n, bool(polya)), number))
             for ch, rid_s, rid, n, polya, number in b] for b in script]


def test_control_loop_golden(dev, proc, golden_dir, tmp_path):
    """replay the scripted ReadUntil batches through the batched SequencerControl and compare
    with what the reference's per-read loop wrote / sent (riser/control.py:11-124)."""
    from riser_amd.control import SequencerControl
    with open(os.path.join(golden_dir, "control.json")) as f:
        g = json.load(f)
    log = logging.getLogger("ctl")
    for k, run in enumerate(g["runs"]):
        models = [get_model(s, dev) for s in run["seeds"]]
        for mdl, t in zip(models, ("mRNA", "mtRNA", "globin")):
            mdl.target = t
        client = FakeClient(_build_batches(g["script"], g["raw_seed"]))
        out = str(tmp_path / f"run{k}")
        ctl = SequencerControl(client, models, proc, log, out)
        ctl.start()
        ctl.target(run["mode"], 1.0, run["threshold"])
        ctl.finish()
        assert client.started and client.was_reset and client.warnings == run["warnings"]
        lines = open(out + ".csv").read().strip().split("\n")
        assert lines[0] == run["header"] and len(lines) - 1 == len(run["rows"])
        for ln, want in zip(lines[1:], run["rows"]):
            p = ln.split(",")
            assert (p[1], int(p[2]), int(p[3]), p[4]) == (want["read_id"], want["channel"], want["sig_length"], want["models"])
            got_p = [float(v) for v in p[5].split(";")]
            assert np.allclose(got_p, want["prob_targets"], atol=PROB_TOL)
            assert float(p[6]) == want["threshold"] and p[7] == want["mode"]
            assert p[8] == want["decision"], (run["mode"], run["seeds"], run["threshold"], want, got_p)
        assert [[list(x) for x in b] for b in client.rejected] == run["rejected"]
        assert [[list(x) for x in b] for b in client.finished] == run["finished"]
        assert client.unblock_durations == run["unblock"]


# ------------------------------------------------------------------------------------------
# BASELINE size (512 x 16000): every read against the oracle, and the size-independent properties
# ------------------------------------------------------------------------------------------
def test_full_size_batch_properties(dev):
    from riser_amd.preprocess import pack_reads
    from conftest import oracle_bench_batch
    m = get_model(1, dev)
    B, L = 512, 16000
    sigs = synth.make_signals(SIG_SEED, B, L)
    sig, off, ln, lens = pack_reads(list(sigs), dev)
    full = m.classify_raw(sig, off, ln, lens).cpu().numpy()
    assert np.isfinite(full).all() and np.allclose(full.sum(1), 1.0, atol=1e-6)
    # (a) idempotence: same call, same bits
    assert np.array_equal(full, m.classify_raw(sig, off, ln, lens).cpu().numpy())
    # (b) sub-batch consistency: reads 100..163 classified alone give the same bits
    idx = torch.arange(100, 164, device=dev)
    part = m.classify_raw(sig, off[idx].contiguous(), ln[idx].contiguous(), lens[100:164]).cpu().numpy()
    assert np.array_equal(part, full[100:164])
    # (c) reversed read order
    ridx = torch.arange(B - 1, -1, -1, device=dev)
    rev = m.classify_raw(sig, off[ridx].contiguous(), ln[ridx].contiguous(), lens[::-1].copy()).cpu().numpy()
    assert np.array_equal(rev[::-1], full)
    # (d) ALL 512 reads against the oracle (numpy normalise + torch-CPU conv stack), and four of them against the
    # independent numpy restatement of the conv stack
    oracle = oracle_bench_batch(1, "full")
    assert np.abs(full - oracle).max() < PROB_TOL, float(np.abs(full - oracle).max())
    assert np.array_equal(full[:, 1] > 0.9, oracle[:, 1] > 0.9)
    pick = [0, 17, 255, 511]
    want = ro.classify_reads(synth.make_state_dict(1), sigs[pick])
    assert np.abs(full[pick] - want).max() < PROB_TOL
    assert np.array_equal(full[pick, 1] > 0.9, want[:, 1] > 0.9)
    # the population must be discriminating, or the checks above prove little
    assert (full[:, 1] > 0.9).sum() > 10 and (full[:, 1] < 0.1).sum() > 10
    # (e) the tile ORDER of the persistent walk (XCD blocks as gm x gn rectangles at this size) must not change a bit:
    # n-major order (RS_NO_RECT_ORDER) gives identical probabilities, fp32 Winograd and f16
    from riser_amd.model import Model
    mh = Model(synth.make_state_dict(1), synth.Config(), None, "m", dtype="f16", device=dev)
    md = Model(synth.make_state_dict(1), synth.Config(), None, "m", dtype="f32", device=dev)      # direct fp32 lowering
    half = mh.classify_raw(sig, off, ln, lens).cpu().numpy()
    direct = md.classify_raw(sig, off, ln, lens).cpu().numpy()
    assert np.abs(direct - full).max() < 1e-4
    from conftest import hooked_model
    for dt, want_bits in (("f32w", full), ("f16", half), ("f32", direct)):
        mo = hooked_model({"RS_NO_RECT_ORDER": "1"}, synth.make_state_dict(1), dt, dev)
        assert np.array_equal(want_bits, mo.classify_raw(sig, off, ln, lens).cpu().numpy()), dt
        mo.close()
    md.close()
    # (f) the 16-bit path against fp32 and the oracle (the ring kernel's bit-for-bit cross-check against the round-1
    # register-staged kernel ran through round 3; that kernel is gone, the weights-resident kernel is checked against the
    # ring kernel in test_gpu_packed.py)
    assert np.abs(half - full).max() < 2e-2
    assert np.abs(half[pick] - want).max() < 2e-2
    mh.close()
