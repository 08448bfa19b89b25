"""The CNN-RNN's f16x3 mode (rs_crnn_set_mode(RS_F16X3), csrc/crnn/x3.hpp): the gate GEMMs whose input is a hidden state run
as hi*hi + lo*hi + hi*lo on the f16 MFMA.  On the CPU a numpy emulation of that arithmetic (tests/crnn_x3_ref.py) sets the bar
and shows that it has teeth; on the GPU the device program is held to the reference's golden logits, to float64, to the
emulation and to its own solo runs bit for bit.

The bar.  E[config] is the emulation's largest gap, in units of max(1, |logit|), to the reference's golden logits and to
float64 over all golden lengths, measured on the CPU when this file was written (emulation vs float64 / vs golden):
    lstm_bi_r2 7.4e-9 / 1.9e-8, gru_bi_r1_c1 2.8e-8 / 1.7e-7, lstm_uni_r3 8.1e-9 / 2.8e-8, gru_uni_r2_h130 1.9e-7 / 2.1e-7,
    lstm_bi_h130 2.9e-8 / 2.0e-7, gru_bi_r2 1.4e-7 / 2.0e-7
(the gap to the golden logits is mostly the reference's own fp32 rounding).  The device bar of a config is
max(10 E[config], its fp32 bar): ten times the emulation's gap because the MFMA sums a 32-wide k-block in its own order in
fp32 and the recurrence feeds every step's rounding into the next; the fp32 bar as a floor because the fp32 parts of the
mode are still there.  E holds the larger of the two figures rounded up to two digits.  The bench nets and the shape-sweep configs have no golden logits: they take E_MAX, the largest E.
"""
import ctypes as C
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import crnn as R
from riser_amd import synth
from tests import crnn_ref, crnn_x3_ref as X3
from tests import test_crnn as TC
from tests import test_crnn_shapes as TS

E = {"lstm_bi_r2": 2.0e-8, "gru_bi_r1_c1": 1.7e-7, "lstm_uni_r3": 2.8e-8, "gru_uni_r2_h130": 2.1e-7, "lstm_bi_h130": 2.0e-7,
     "gru_bi_r2": 2.0e-7}
E_MAX = max(E.values())
F32_BAR = 2e-6                                       # test_crnn.tol: the golden configs' and the bench nets' fp32 bar


def bar(name) -> float:
    """the device bar of a config, x max(1, |logit|)"""
    if name in TS.CONFIGS:
        return max(10 * E_MAX, TS.TOL[name])
    return max(10 * E.get(name, E_MAX), F32_BAR)


def gap(got, ref) -> float:
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def held(tag, name, got, ref):
    g = gap(got, ref)
    print(f"\nCRNN_X3_GAP {name} {tag} max|got-ref|/scale {g:.3e} (bar {bar(name):.1e})")
    assert g <= bar(name), (name, tag, g)


def labels_agree(got, ref, margin):
    """labels equal wherever the reference's two logits differ by more than `margin`"""
    sure = np.abs(ref[:, 1] - ref[:, 0]) > margin
    return np.array_equal((got[:, 1] > got[:, 0])[sure], (ref[:, 1] > ref[:, 0])[sure])


def _golden(golden_dir, name):
    g, cfg, sd = TC._load(golden_dir, name)
    return g, cfg, sd, R.build_crnn_program(sd, TC._ns(cfg))


# ------------------------------------------------------------------------------------------------ CPU: the emulation
@pytest.mark.parametrize("name", TC.NAMES)
def test_emulation_matches_reference_and_float64(golden_dir, name):
    g, cfg, sd, prog = _golden(golden_dir, name)
    worst = 0.0
    for L in cfg["lengths"]:
        x = TC._inputs(L)
        em = X3.forward(prog, x)
        wl, f64 = g[f"{name}.L{L}.logits"], crnn_ref.forward(prog, x)
        worst = max(worst, gap(em, wl), gap(em, f64))
        assert labels_agree(em, wl.astype(np.float64), 10 * E[name]), L
    print(f"\nCRNN_X3_EMULATION {name} E {worst:.3e}")
    assert worst <= E[name], worst


def test_split_gemm_is_not_plain_f16():
    """on the gate GEMM alone: h in (-1, 1) against gate weights, the split at least 100x closer to float64 than plain f16"""
    rng = np.random.default_rng(7)
    a = np.tanh(rng.standard_normal((64, 128))).astype(np.float32)
    w = (rng.standard_normal((512, 128)) * 0.09).astype(np.float32)
    want = a.astype(np.float64) @ w.astype(np.float64).T
    e3 = np.abs(X3.x3_matmul_f16(a, w) - want).max()
    e1 = np.abs(X3.plain_matmul_f16(a, w) - want).max()
    print(f"\nCRNN_X3_GEMM split {e3:.3e} plain {e1:.3e}")
    assert e3 <= 1e-2 * e1, (e3, e1)
    # weights of any magnitude: the packer's scale is exact
    for s in (2.0 ** -30, 2.0 ** 20):
        assert np.allclose(X3.x3_matmul_f16(a, w * np.float32(s)), X3.x3_matmul_f16(a, w) * s, rtol=1e-12, atol=0)


def test_lo_halves_matter_end_to_end(golden_dir):
    """plain f16 operands are at least 100x farther from float64 than the split on the logits; measured ratios (plain / split):
    at 4097 samples lstm_bi_r2 3100, gru_bi_r1_c1 5200, lstm_uni_r3 5700, gru_uni_r2_h130 2500, lstm_bi_h130 4900, gru_bi_r2
    2900 - no config is left out"""
    ok = 0
    for name in TC.NAMES:
        g, cfg, sd, prog = _golden(golden_dir, name)
        x = TC._inputs(4097)
        f64 = crnn_ref.forward(prog, x)
        e3, e1 = gap(X3.forward(prog, x), f64), gap(X3.forward(prog, x, mutant="plain_f16"), f64)
        print(f"\nCRNN_X3_PLAIN {name} split {e3:.3e} plain {e1:.3e} ratio {e1 / e3:.0f}")
        ok += e3 <= 1e-2 * e1
    assert ok >= 4


def test_mutants_miss_the_bar_and_configs_are_alive(golden_dir):
    miss = {m: 0.0 for m in X3.MUTANTS}
    for name in TC.NAMES:
        g, cfg, sd, prog = _golden(golden_dir, name)
        lg = []
        for L in cfg["lengths"][-2:]:                # 4097 and 12000: the recurrence has steps to compound over
            x = TC._inputs(L)
            f64 = crnn_ref.forward(prog, x)
            with np.errstate(over="ignore"):
                for m in X3.MUTANTS:
                    d = gap(X3.forward(prog, x, mutant=m), f64) / bar(name)
                    miss[m] = max(miss[m], d)
                    if m == "first_proj_split":      # the scope line is about range, not accuracy
                        assert d <= 1.0, (name, L, d)
        for L in cfg["lengths"]:
            lg.append(crnn_ref.forward(prog, TC._inputs(L)))
        lg = np.concatenate(lg)
        assert (lg.max(0) - lg.min(0)).min() > 1000 * bar(name), name
    print("\nCRNN_X3_MUTANTS miss / bar " + ", ".join(f"{m} {v:.1f}" for m, v in miss.items()))
    for m in X3.DEFECTS:
        assert miss[m] > 10, (m, miss[m])


def test_abi_set_mode_without_a_gpu():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    lib = nv.lib()
    assert "rs_crnn_set_mode" in nv.SYMBOLS and hasattr(lib, "rs_crnn_set_mode")
    assert lib.rs_version() == (2 << 16) | 9
    for dt in (nv.RS_F16X3, nv.RS_F32, nv.RS_BF16X3, nv.RS_F16, 99, -1):
        assert lib.rs_crnn_set_mode(None, dt) == nv.RS_ERR_ARG
        assert b"rs_crnn_set_mode" in lib.rs_last_error()


@pytest.mark.parametrize("dtype", ["bf16x3", "f16", "bf16", "f16xf8"])
def test_net_refuses_other_dtypes_before_touching_a_device(dtype):
    sd, cfg = TC._sd_cfg("lstm")
    prog = R.build_crnn_program(sd, types.SimpleNamespace(**cfg))
    with pytest.raises(ValueError, match="f32.*f16x3"):
        R.CRNNNet(prog, device=None, dtype=dtype)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _cfg_sd(golden_dir, name):
    """(cfg, sd, prog) of a golden config, a bench net or a shape-sweep config"""
    if name in TS.CONFIGS:
        return TS.program(name)
    if name.startswith("bench_"):
        cfg, sd = TC._bench(name[6:])
    else:
        _, cfg, sd = TC._load(golden_dir, name)
    return cfg, sd, R.build_crnn_program(sd, types.SimpleNamespace(**{k: cfg[k] for k in TC.CFG_KEYS}))


def _model(golden_dir, name, dtype="f16x3"):
    from riser_amd.model import Model
    cfg, sd, prog = _cfg_sd(golden_dir, name)
    ns = types.SimpleNamespace(**{k: cfg[k] for k in TC.CFG_KEYS})
    return Model(sd, types.SimpleNamespace(model="cnn-rnn", cnn_rnn=ns), None, "mRNA", dtype=dtype, device=_dev()), prog


@pytest.mark.gpu
@pytest.mark.parametrize("name", TC.NAMES)
def test_device_matches_reference_float64_emulation_and_differs_from_fp32(golden_dir, name):
    import torch
    g, cfg, sd, prog = _golden(golden_dir, name)
    m, _ = _model(golden_dir, name)
    m32, _ = _model(golden_dir, name, "f32")
    assert m.dtype == "f16x3" and m._seq.dtype == "f16x3" and m.min_length == cfg["min_length"]
    for L in cfg["lengths"]:
        x = TC._inputs(L)
        wl, wp = g[f"{name}.L{L}.logits"], g[f"{name}.L{L}.probs"]
        probs, logits = m.classify_batch(x, return_logits=True)
        lg, pr = logits.cpu().numpy(), probs.cpu().numpy()
        held(f"L{L} reference", name, lg, wl)
        held(f"L{L} float64", name, lg, crnn_ref.forward(prog, x))
        held(f"L{L} emulation", name, lg, X3.forward(prog, x))
        # p1 = sigmoid(l1 - l0), slope at most 1/4: two logits within bar x scale of the reference's move it by at most
        # half of bar x scale
        assert np.abs(pr - wp).max() <= 0.5 * bar(name) * max(1.0, float(np.abs(wl).max())) + 1e-7, L
        assert labels_agree(lg, wl.astype(np.float64), 10 * E[name]), L
        fb = m.forward_batch(torch.from_numpy(x).to(m.device), np.full(3, L, dtype=np.int32)).cpu().numpy()
        assert np.array_equal(fb, pr)
        for i in range(3):
            assert np.array_equal(m.classify(x[i]).cpu().numpy(), pr[i]), (L, i)
        if L >= 4097:                                # another arithmetic: not the fp32 model's bits, and inside the bar of it
            l32 = m32.classify_batch(x, return_logits=True)[1].cpu().numpy()
            d = gap(lg, l32)
            print(f"\nCRNN_X3_VS_F32 {name} L{L} {d:.3e}")
            assert 0 < d < bar(name), (L, d)
    assert not m.saturated()
    m.close()
    m32.close()


def _nan_padded(sigs):
    """(x [B, ld] with NaN behind every read, rows 64 longer than the longest read; int32 lengths) on the device"""
    return TS._pack(sigs)


def _run(net, sigs):
    x, ln = _nan_padded(sigs)
    p, l = net.forward_ragged(x, ln, return_logits=True)
    return p.cpu().numpy(), l.cpu().numpy()


def _sweep_reads(golden_dir, name):
    if name in TS.CONFIGS:
        return TS.reads(name), TS.reference(name)
    _, _, prog = _cfg_sd(golden_dir, name)
    rng = np.random.default_rng(sum(name.encode()))
    lens = TC._sweep_lengths(R.min_length(prog), prog, rng)
    sigs = [ro.mad_normalise(synth.make_signals(20260103, 1, n, first_read=300 + i)[0]).astype(np.float32)
            for i, n in enumerate(lens)]
    return sigs, crnn_ref.forward_ragged(prog, sigs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TC.NAMES + ["bench_lstm", "bench_gru"] + TS.NAMES)
def test_ragged_sweep_against_float64_and_solo_bits(golden_dir, name):
    m, prog = _model(golden_dir, name)
    net = m._seq
    sigs, want = _sweep_reads(golden_dir, name)
    assert len(sigs) == 77
    probs, logits = _run(net, sigs)
    assert np.isfinite(logits).all() and np.isfinite(probs).all()
    held("ragged float64", name, logits, want)
    p2, l2 = m.classify_batch(sigs, return_logits=True)          # zero-padded rows: the same bits
    assert TS._same(l2.cpu().numpy(), logits)
    for i, s in enumerate(sigs):
        p1, l1 = TS._solo(net, s)
        assert TS._same(l1, logits[i]) and TS._same(p1, probs[i]), (name, i, len(s))
        pc, lc = m.classify_batch([s], return_logits=True)        # the public entry points, every read
        assert TS._same(lc.cpu().numpy()[0], logits[i]) and TS._same(pc.cpu().numpy()[0], probs[i]), (name, i, len(s))
        assert TS._same(m.classify(s).cpu().numpy(), probs[i]), (name, i, len(s))
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", TS.NAMES)
def test_tile_forms_and_poisoned_workspace(name):
    m, prog = _model(None, name)
    net = m._seq
    pool = TS.short_reads(name, 17, 4)
    solo = [TS._solo(net, s) for s in pool]
    want = crnn_ref.forward_ragged(prog, pool)
    for B in (1, 15, 16, 17):
        probs, logits = _run(net, pool[:B])
        held(f"B{B}", name, logits, want[:B])
        for i in range(B):
            assert TS._same(logits[i], solo[i][1]) and TS._same(probs[i], solo[i][0]), (B, i)
    probs, logits = _run(net, pool)
    rp, rl = _run(net, pool[::-1])
    assert TS._same(rp[::-1], probs) and TS._same(rl[::-1], logits)
    mn = m.min_length
    fixed = TS.signal(58)[TS.MAX_LEN - (mn + 700):]
    p0, l0 = TS._solo(net, fixed)
    for slot in range(16):
        others = TS.short_reads(name, 15, 100 + slot)
        probs, logits = _run(net, others[:slot] + [fixed] + others[slot:])
        assert TS._same(logits[slot], l0) and TS._same(probs[slot], p0), slot
        assert np.isfinite(logits).all()
    # a workspace of NaN bytes before and after a larger batch
    small = TS.short_reads(name, 5, 1)
    first = _run(net, small)
    net._ws.fill_(0xFF)
    again = _run(net, small)
    assert TS._same(first[0], again[0]) and TS._same(first[1], again[1])
    big = TS.short_reads(name, 21, 2, hi=4000)
    big_first = _run(net, big)
    again = _run(net, small)
    assert TS._same(first[0], again[0]) and TS._same(first[1], again[1])
    net._ws.fill_(0xFF)
    again, big_again = _run(net, small), _run(net, big)
    assert TS._same(first[0], again[0]) and TS._same(first[1], again[1])
    assert TS._same(big_first[0], big_again[0]) and TS._same(big_first[1], big_again[1])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_bench_net_512_raw_reads_against_fp32(cell):
    from riser_amd.preprocess import pack_reads
    name = f"bench_{cell}"
    m, prog = _model(None, name)
    m32, _ = _model(None, name, "f32")
    sigs = synth.make_signals(20260103, 512, 16000)
    sig, off, ln, lh = pack_reads(sigs, m.device)
    p3, l3 = m.classify_raw(sig, off, ln, lh, return_logits=True)
    p32, l32 = m32.classify_raw(sig, off, ln, lh, return_logits=True)
    p3, p32 = p3.cpu().numpy(), p32.cpu().numpy()
    held("512 fp32 model", name, l3.cpu().numpy(), l32.cpu().numpy().astype(np.float64))
    sure = np.abs(p32[:, 1] - 0.5) > bar(name)
    assert sure.sum() > 400
    assert np.array_equal((p3[:, 1] > 0.5)[sure], (p32[:, 1] > 0.5)[sure])
    assert not m.saturated()
    m.close()
    m32.close()


@pytest.mark.gpu
def test_mode_switch_leaves_no_residue(golden_dir):
    from riser_amd import _native as nv
    lib = nv.lib()
    for name in ("lstm_bi_r2", "gru_uni_r2_h130"):
        m, prog = _model(golden_dir, name, "f32")
        fresh32, _ = _model(golden_dir, name, "f32")
        net = m._seq
        sigs = [TS.signal(i)[TS.MAX_LEN - n:] for i, n in enumerate((300, 4097, 2000, 9000))]
        want32 = _run(fresh32._seq, sigs)
        ws32, mb32 = lib.rs_crnn_workspace_bytes(net._h, 4, 9064), lib.rs_crnn_max_batch(net._h, 9064)
        assert TS._same(_run(net, sigs)[1], want32[1])
        net.set_mode("f16x3")
        first3 = _run(net, sigs)
        assert not TS._same(first3[1], want32[1])
        assert lib.rs_crnn_workspace_bytes(net._h, 4, 9064) == ws32 > 0 and lib.rs_crnn_max_batch(net._h, 9064) == mb32 > 0
        for bad in (nv.RS_BF16X3, nv.RS_F16, nv.RS_BF16, nv.RS_F16XF8, 99):
            assert lib.rs_crnn_set_mode(net._h, bad) == nv.RS_ERR_ARG and b"rs_crnn_set_mode" in lib.rs_last_error()
        again3 = _run(net, sigs)                     # the mode was kept
        assert TS._same(again3[0], first3[0]) and TS._same(again3[1], first3[1])
        net.set_mode("f32")
        back = _run(net, sigs)
        assert TS._same(back[0], want32[0]) and TS._same(back[1], want32[1])
        net.set_mode("f16x3")
        again3 = _run(net, sigs)
        assert TS._same(again3[0], first3[0]) and TS._same(again3[1], first3[1])
        m.close()
        fresh32.close()


@pytest.mark.gpu
def test_set_mode_refuses_weights_that_are_not_finite(golden_dir):
    from riser_amd import _native as nv
    _, cfg, sd = TC._load(golden_dir, "gru_bi_r1_c1")
    sd = dict(sd)
    w = np.array(sd["rec_layers.0.weight_hh_l0"], dtype=np.float32)
    w[1, 2] = np.inf
    sd["rec_layers.0.weight_hh_l0"] = w
    prog = R.build_crnn_program(sd, TC._ns(cfg))
    net = R.CRNNNet(prog, device=_dev(), dtype="f32")
    assert nv.lib().rs_crnn_set_mode(net._h, nv.RS_F16X3) == nv.RS_ERR_ARG
    assert b"rs_crnn_set_mode" in nv.lib().rs_last_error() and net.dtype == "f32"
    with pytest.raises(nv.NativeError, match="rs_crnn_set_mode.*not finite"):
        R.CRNNNet(prog, device=_dev(), dtype="f16x3")
    net.close()


@pytest.mark.gpu
def test_ensemble_with_a_tcn_and_a_convnet(golden_dir):
    import torch
    from riser_amd import _native as nv
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    dev = _dev()
    crnn, _ = _model(golden_dir, "lstm_bi_r2")
    tcfg = synth.TCN_BENCH_CFG
    tcn = Model(synth.make_tcn_state_dict(5, tcfg), types.SimpleNamespace(model="tcn", tcn=types.SimpleNamespace(**tcfg)),
                None, "b", dtype="bf16x3", device=dev)
    cnn = Model(synth.make_state_dict(1), synth.Config(), None, "c", device=dev)
    models = [crnn, tcn, cnn]
    sigs = TC._raw_reads([4096, 5000, 8615, 4300, 12000, 16000, 6000], first=900)
    sig, off, ln, lh = pack_reads(sigs, dev)
    dec = torch.empty(len(sigs), dtype=torch.uint8, device=dev)
    probs = classify_raw_ensemble(models, sig, off, ln, lh, decision=dec, max_len=12000, threshold=0.6)
    for k, m in enumerate(models):
        assert torch.equal(probs[k], m.classify_raw(sig, off, ln, lh))
    want = torch.empty_like(dec)
    p2 = probs.contiguous()
    nv.check(nv.lib().rs_decide(p2.data_ptr(), 3, len(sigs), ln.data_ptr(), 12000, 0.6, nv.RS_ENRICH, want.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
    assert torch.equal(dec, want)
    for m in models:
        m.close()


@pytest.mark.gpu
def test_get_models_and_sequencer_control_run_the_mode(tmp_path, golden_dir):
    import logging
    import torch
    from riser_amd import Kit, SequencerControl, SignalProcessor
    from riser_amd import _native as nv
    from riser_amd.fake_client import FakeClient, FakeRead
    from riser_amd.modeldir import get_models
    d, cfg, sd = TC._write_model_dir(tmp_path, golden_dir)
    dev = _dev()
    (m,) = get_models(["mRNA"], logging.getLogger("t"), "RNA004", model_dir=d, dtype="f16x3", device=dev)
    assert m._h is None and isinstance(m._seq, R.CRNNNet) and m.dtype == "f16x3"
    rng = np.random.default_rng(12)
    batches = [[(ch, FakeRead(f"id-{b * 7 + ch}", synth.make_raw_read(56, b * 7 + ch, int(rng.integers(3000, 24000)),
                                                                      polya=((b * 7 + ch) % 4 != 0))))
                for ch in range(1, 25)] for b in range(2)]
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    out = str(tmp_path / "o")
    ctl = SequencerControl(FakeClient(batches), [m], proc, logging.getLogger("c"), out)
    ctl.start(); ctl.target("enrich", 0.5, 0.9); ctl.finish()
    lines = open(out + ".csv").read().strip().split("\n")
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) > 10
    names = {"try_again": nv.RS_TRY_AGAIN, "accept": nv.RS_ACCEPT, "reject": nv.RS_REJECT, "no_decision": nv.RS_NO_DECISION}
    p1 = np.array([[float(v) for v in r[5].split(";")] for r in rows], dtype=np.float32)
    probs = torch.from_numpy(np.stack([1 - p1[:, 0], p1[:, 0]], axis=1)[None].copy()).to(dev)
    lens = torch.tensor([int(r[3]) for r in rows], dtype=torch.int32, device=dev)
    dec = torch.empty(len(rows), dtype=torch.uint8, device=dev)
    nv.check(nv.lib().rs_decide(probs.data_ptr(), 1, len(rows), lens.data_ptr(), ro.kit_max_length("RNA004"), 0.9,
                                nv.RS_ENRICH, dec.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
    for r, dk in zip(rows, dec.cpu().numpy()):
        q = float(r[5])
        if abs(q - 0.9) < 1e-4 or abs(1 - q - 0.9) < 1e-4:
            continue
        assert names[r[8]] == dk, r
    assert not m.saturated()
    m.close()


@pytest.mark.gpu
def test_batch_beyond_max_batch_is_split_and_never_saturates(golden_dir, monkeypatch):
    m, prog = _model(golden_dir, "lstm_bi_r2")
    lens = [4097, 300, 16000, 125, 9000, 70, 12000]
    sigs = [ro.mad_normalise(s).astype(np.float32) for s in TC._raw_reads(lens, first=40)]
    whole = m.classify_batch(sigs).cpu().numpy()
    assert m.max_batch(16000) > len(sigs)
    monkeypatch.setattr(type(m._seq), "max_batch", lambda self, L: 3)
    split = m.classify_batch(sigs).cpu().numpy()
    assert np.array_equal(whole, split)
    monkeypatch.undo()
    # inputs at the normaliser's limits: no f16 operand of the mode can overflow
    rng = np.random.default_rng(3)
    hard = [np.where(rng.random(n) < 0.5, -3.5, 3.5).astype(np.float32) for n in (4097, 9000)]
    p, lg = m.classify_batch(hard, return_logits=True)
    assert np.isfinite(p.cpu().numpy()).all() and not m.saturated()
    held("inputs at +-3.5", "lstm_bi_r2", lg.cpu().numpy(), crnn_ref.forward_ragged(prog, hard))
    m.close()
