"""The CNN-RNN's four kernels (csrc/crnn.hip) across the shape classes their index arithmetic branches on, against float64.

Every decision of the device program that depends on a shape - the hidden size's tiles over the eight waves and whether W_hh
stays in registers, the pad columns of a sequence buffer and the projection's k-panels over them, the conv's column groups,
input pitch in LDS and tap loop - is a class tag of `shape_tags`, a pure-Python mirror of that arithmetic.  The configs below
are chosen so that together they hit every tag (a CPU test holds the union to the full list).  Each config runs on the device:
  sweep       one ragged batch of 77 reads in rows 64 samples longer than the longest read, NaN behind every read, held to
              float64 (crnn_ref.forward_ragged) within TOL[config] x max(1, |logit|), probabilities within 1e-5, and every
              read equal to its solo run bit for bit;
  workspace   the same call on a workspace filled with 0xFF bytes (NaN everywhere), before and after a larger batch used it;
  tiles       batches of 1 / 15 / 16 / 17 reads, one long read among minimum-length ones, a tile of one-step reads, one read
              in each of a tile's 16 slots, the batch reversed;
  clamp       a length beyond the pitch, below the network minimum and negative, in the middle of a tile;
  grouped     Model's group-by-length branch.
The mistakes a device program could make here are mutants of the float64 forward (crnn_ref.DEVICE_MUTANTS): each must miss by
more than ten times its config's tolerance.  Six edge configs are pinned to the reference's own ConvRecNet
(tests/golden/crnn_edges.npz) on the CPU."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import crnn as R
from riser_amd import synth
from tests import crnn_ref

_C = lambda ch, ks, cell, H, r, bi: dict(n_conv_layers=len(ch), channels=ch, kernels=ks, cell=cell, hidden=H, n_rec_layers=r,
                                         bidirectional=bi, dropout=0.2, n_classes=2)
CONFIGS = {
    # one wave has a tile; K = 5 into layers 1-3 (1 mod 4, below one k-panel); taps 1 (single) and 2 over 10 input channels
    # (2 mod 4, LDS pitch 12 not bumped); 13 output channels (3 pad columns)
    "h5_gru_uni_k1": _C([10, 13], [1, 2], "gru", 5, 2, False),
    # K = 7 (3 mod 4); taps 2 (single) and 1 over 6 input channels (pitch 8 bumped to 12); 9 output channels
    "h7_lstm_uni_k2": _C([6, 9], [2, 1], "lstm", 7, 2, False),
    # hidden 16 exactly: no pad unit; a 13-tap single-channel conv (padded to 16 taps); 12 input channels (pitch 12, not bumped)
    "h16_gru_bi_k13": _C([12, 20], [13, 3], "gru", 16, 2, True),
    # K = 17: one column into the second k-panel, 1 mod 4
    "h17_lstm_uni": _C([8, 16], [5, 3], "lstm", 17, 2, False),
    # 7 of 8 waves have a tile; 100 output channels (a second column group of 48) and 100 input channels (pitch 100)
    "h112_lstm_bi_c100": _C([16, 100, 20], [5, 3, 3], "lstm", 112, 1, True),
    # the first cache-fed size: 9 tiles, wave 0 takes two; K = 129 into layers 1-3
    "h129_lstm_uni": _C([8, 16, 32], [5, 4, 3], "lstm", 129, 2, False),
    # 16 tiles: two full rounds over the waves
    "h256_lstm_bi": _C([8, 16, 32, 32], [9, 7, 5, 3], "lstm", 256, 1, True),
    # 17 tiles: a third round for wave 0; hidden 260 pads to 272; K = 260 (4 into the 17th k-panel)
    "h260_gru_uni": _C([8, 16, 32, 64], [9, 7, 5, 3], "gru", 260, 2, False),
    # the cap: 62 208 B of LDS
    "h320_gru_bi": _C([8, 16, 32, 64], [9, 7, 5, 3], "gru", 320, 1, True),
    # 130 output channels (three column groups, 2 pad columns) behind a 19-tap kernel over 8 channels
    "c130_k19_gru_bi": _C([8, 130], [3, 19], "gru", 24, 1, True),
    # six conv layers, widths 2 mod 4 with both pitches; K = 66 (2 into the fifth k-panel)
    "six_convs_lstm_bi": _C([4, 6, 8, 10, 12, 14], [3, 2, 3, 1, 3, 2], "lstm", 33, 2, True),
}
NAMES = list(CONFIGS)
SEED = {n: 5100 + i for i, n in enumerate(NAMES)}
GAIN = 2.0
N_READS = 77
MAX_LEN = 16000
PAD = 64                                             # the ragged batch's row pitch: this much above the longest read

# fp32 device against float64, x max(1, |logit|), per config: 4x the largest gap measured on an MI355X over every call of this
# file on the config (the 77-read sweep and the tile forms), rounded up to one digit, and not below TOL_FLOOR; the loosest is
# a third of the 2e-5 the CNN-RNN was held to before.  Measured:
GAP = {"h5_gru_uni_k1": 4.3e-08, "h7_lstm_uni_k2": 1.5e-08, "h16_gru_bi_k13": 1.5e-07, "h17_lstm_uni": 3.5e-08,
       "h112_lstm_bi_c100": 4.7e-07, "h129_lstm_uni": 1.3e-07, "h256_lstm_bi": 8.5e-07, "h260_gru_uni": 1.3e-06,
       "h320_gru_bi": 1.4e-06, "c130_k19_gru_bi": 3.6e-07, "six_convs_lstm_bi": 5.0e-08}
# two fp32 ulps of a logit near 1: below this a bound measures the rounding of the logit itself (half an ulp, 6e-8), which a
# different but equally valid expf / tanhf would move
TOL_FLOOR = 2e-7
TOL = {"h5_gru_uni_k1": 2e-7, "h7_lstm_uni_k2": 2e-7, "h16_gru_bi_k13": 6e-7, "h17_lstm_uni": 2e-7, "h112_lstm_bi_c100": 2e-6,
       "h129_lstm_uni": 6e-7, "h256_lstm_bi": 4e-6, "h260_gru_uni": 6e-6, "h320_gru_bi": 6e-6, "c130_k19_gru_bi": 2e-6,
       "six_convs_lstm_bi": 2e-7}


# ------------------------------------------------------------------------------------------------ the shape mirror
def _cp4(c):
    return (c + 3) & ~3


def _p16(c):
    return (c + 15) & ~15


RES_HIDDEN, MAX_HIDDEN = 128, 320      # pinned by behaviour: 128 and 129 both match float64, 320 runs, 321 is refused

ALL_TAGS = {
    # hidden: Hp = p16(H), HT = Hp / 16 tiles over 8 waves, W_hh in registers up to 128
    "H<16", "H=16", "HT=7", "HT=9", "HT=16", "HT=17", "H=320", "H%16!=0", "rec:resident", "rec:cache",
    # K = ndir * H into a later layer: the sequence buffer's pitch cp4(K) has pad columns nobody writes
    "K%4=1", "K%4=3", "K<16", "K just above 16n", "K%16=0",
    # conv output: np = p16(c_out), ceil(np / 64) column groups, pitch cp4(c_out)
    "conv:c_out%4!=0", "conv:ng=1", "conv:ng=2 partial", "conv:ng=3",
    # conv input: cpi = cp4(c_in), LDS pitch bumped by 4 when cpi / 4 is even
    "conv:c_in%4!=0", "conv:pitch bumped", "conv:pitch unbumped",
    # taps: one input channel pads them to 4; more channels loop over them
    "conv:single k=1", "conv:single k=2", "conv:single k%4=1 k>9", "conv:multi k=1", "conv:multi k=2", "conv:multi k>=19",
    "conv:layers>4",
    "lstm:uni", "lstm:bi", "gru:uni", "gru:bi",
}


def shape_tags(cfg) -> set:
    """the classes of csrc/crnn.hip's shape arithmetic that a config runs"""
    tags = set()
    H, ndir = cfg["hidden"], 2 if cfg["bidirectional"] else 1
    assert 1 <= H <= MAX_HIDDEN
    HT = _p16(H) // 16
    tags.add("rec:resident" if H <= RES_HIDDEN else "rec:cache")
    tags |= {t for t, on in (("H<16", H < 16), ("H=16", H == 16), ("H=320", H == MAX_HIDDEN), ("H%16!=0", H % 16 != 0)) if on}
    if HT in (7, 9, 16, 17):
        tags.add(f"HT={HT}")
    if cfg["n_rec_layers"] ** 2 >= 2:                # a layer reads the previous layer's sequence
        K = ndir * H
        tags |= {t for t, on in (("K%4=1", K % 4 == 1), ("K%4=3", K % 4 == 3), ("K<16", K < 16), ("K%16=0", K % 16 == 0),
                                 ("K just above 16n", K > 16 and 1 <= K % 16 <= 4)) if on}
    n = cfg["n_conv_layers"]
    if n > 4:
        tags.add("conv:layers>4")
    c_in = 1
    for c_out, k in zip(cfg["channels"][:n], cfg["kernels"][:n]):
        ng = (_p16(c_out) + 63) // 64
        tags.add("conv:ng=2 partial" if ng == 2 and _p16(c_out) < 128 else f"conv:ng={ng}")
        if c_out % 4:
            tags.add("conv:c_out%4!=0")
        if c_in == 1:
            tags |= {t for t, on in (("conv:single k=1", k == 1), ("conv:single k=2", k == 2),
                                     ("conv:single k%4=1 k>9", k % 4 == 1 and k > 9)) if on}
        else:
            cpi = _cp4(c_in)
            tags.add("conv:pitch bumped" if (cpi // 4) % 2 == 0 else "conv:pitch unbumped")
            if c_in % 4:
                tags.add("conv:c_in%4!=0")
            tags |= {t for t, on in (("conv:multi k=1", k == 1), ("conv:multi k=2", k == 2), ("conv:multi k>=19", k >= 19)) if on}
        c_in = c_out
    tags.add(f"{cfg['cell']}:{'bi' if cfg['bidirectional'] else 'uni'}")
    return tags


# ------------------------------------------------------------------------------------------------ programs, reads, float64
_CACHE = {}


def _ns(cfg):
    return types.SimpleNamespace(**cfg)


def program(name):
    """(cfg, sd, prog) of a sweep config: synth weights of its seed, gain 2"""
    if name not in _CACHE:
        cfg = CONFIGS[name]
        sd = synth.make_crnn_state_dict(SEED[name], cfg, gain=GAIN)
        _CACHE[name] = (cfg, sd, R.build_crnn_program(sd, _ns(cfg)))
    return _CACHE[name]


def odd_pool_length(prog, start):
    L0 = start
    while True:
        L, odd = L0, False
        for cv in prog["convs"]:
            odd |= (L - cv["k"] + 1) % 2 == 1
            L = (L - cv["k"] + 1) // 2
        if odd:
            return L0
        L0 += 1


def sweep_lengths(name):
    """77 read lengths: the minimum, one more, an odd-pool length, 4096, 4097, 8615, 16000 and seeded random ones"""
    prog = program(name)[2]
    mn = R.min_length(prog)
    fixed = [mn, mn + 1, odd_pool_length(prog, mn + 2), 4096, 4097, 8615, MAX_LEN]
    rng = np.random.default_rng(sum(map(ord, name)))
    return fixed + [int(v) for v in rng.integers(mn, MAX_LEN + 1, N_READS - len(fixed))]


_SIGNALS = {}


def signal(i):
    """normalised synthetic read i of 16000 samples; a read of n samples is the last n of one"""
    if i not in _SIGNALS:
        s = synth.make_signals(20260105, 1, MAX_LEN, first_read=7300 + i)[0]
        _SIGNALS[i] = ro.mad_normalise(s).astype(np.float32)
    return _SIGNALS[i]


def reads(name):
    return [signal(i)[MAX_LEN - n:] for i, n in enumerate(sweep_lengths(name))]


_REF = {}


def reference(name):
    """float64 logits of the sweep's 77 reads"""
    if name not in _REF:
        _REF[name] = crnn_ref.forward_ragged(program(name)[2], reads(name))
    return _REF[name]


def short_reads(name, n, seed, hi=1500):
    """n reads of seeded lengths from the minimum to `hi` above it (cheap on both sides): the tile-form batches"""
    mn = R.min_length(program(name)[2])
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    return [signal(40 + (seed + i) % 37)[MAX_LEN - int(L):] for i, L in enumerate(rng.integers(mn, mn + hi + 1, n))]


# ------------------------------------------------------------------------------------------------ CPU
def test_configs_reach_every_shape_class():
    got = set().union(*(shape_tags(CONFIGS[n]) for n in NAMES))
    assert got == ALL_TAGS, sorted(got ^ ALL_TAGS)
    cells = {(c["cell"], c["bidirectional"]) for c in CONFIGS.values()}
    assert len(cells) == 4


def test_tolerances_are_never_looser_than_before():
    assert set(TOL) == set(GAP) == set(NAMES)
    for n in NAMES:
        assert TOL[n] <= 2e-5, n
        assert TOL[n] == TOL_FLOOR or 3 * GAP[n] <= TOL[n] <= 6 * GAP[n], n  # about 4x the measured gap


@pytest.mark.parametrize("name", NAMES)
def test_config_is_alive(name):
    """a config whose features die in the ReLUs gives every read the same logits and would pass any kernel: the float64
    logits of the 77 reads spread by more than 1000 tolerances, and no two reads of the sweep share their logits"""
    lg = reference(name)
    assert np.isfinite(lg).all()
    spread = (lg.max(0) - lg.min(0)).min()
    assert spread > 1000 * TOL[name], spread
    assert len({tuple(r) for r in lg}) == N_READS


@pytest.mark.parametrize("name", NAMES)
def test_ragged_float64_equals_per_read_forwards(name):
    prog = program(name)[2]
    sel = reads(name)[:3] + short_reads(name, 5, 3)
    want = np.concatenate([crnn_ref.forward(prog, r[None]) for r in sel])
    assert np.abs(crnn_ref.forward_ragged(prog, sel) - want).max() < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_device_mutants_are_caught_at_the_sweep_tolerances(name):
    """every applicable device-shaped mutant moves some logit of the sweep by more than 10x the config's tolerance"""
    cfg, _, prog = program(name)
    idx = list(range(7)) + [20, 41]                  # the fixed lengths and two random ones
    sel = [reads(name)[i] for i in idx]
    base = reference(name)[idx]
    scale = np.maximum(1.0, np.abs(base))
    applied = 0
    for mutant in crnn_ref.DEVICE_MUTANTS:
        if not crnn_ref.device_mutant_applies(cfg, mutant):
            continue
        applied += 1
        miss = (np.abs(crnn_ref.forward_ragged(prog, sel, mutant=mutant) - base) / scale).max()
        assert miss > 10 * TOL[name], (mutant, miss)
    assert applied >= 4


def test_every_device_mutant_applies_somewhere():
    for mutant in crnn_ref.DEVICE_MUTANTS:
        assert any(crnn_ref.device_mutant_applies(CONFIGS[n], mutant) for n in NAMES), mutant
    for n in NAMES:                                  # where a mutant is said not to apply it is the identity
        cfg, _, prog = program(n)
        sel = short_reads(n, 4, 9, hi=300)
        base = crnn_ref.forward_ragged(prog, sel)
        for mutant in crnn_ref.DEVICE_MUTANTS:
            if not crnn_ref.device_mutant_applies(cfg, mutant):
                assert np.array_equal(crnn_ref.forward_ragged(prog, sel, mutant=mutant), base), (n, mutant)


EDGES = ["h5_gru_uni_k1", "c130_k19_gru_bi", "six_convs_lstm_bi", "h112_lstm_bi_c100", "h129_lstm_uni", "h320_gru_bi"]
EDGE_TOL = 3e-6                                      # float64 against the reference's fp32 forward: about 4x the 7.1e-7 measured when the fixture was made


def edge_lengths(prog):
    mn = R.min_length(prog)
    return [mn, mn + 1, odd_pool_length(prog, mn + 2), 4097]


@pytest.mark.parametrize("name", EDGES)
def test_edge_configs_match_the_reference(golden_dir, name):
    """the float64 forward pinned to the reference's own ConvRecNet (tests/golden/crnn_edges.npz) on edge configs of the
    sweep: the same config and weights (rebuilt from the seed, checked by their digest)"""
    g = np.load(os.path.join(golden_dir, "crnn_edges.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    lens, seed, gain, sha = cfg.pop("lengths"), cfg.pop("seed"), cfg.pop("gain"), cfg.pop("sd_sha16")
    assert cfg == CONFIGS[name] and seed == SEED[name] and gain == GAIN
    _, sd, prog = program(name)
    assert synth.state_dict_sha16(sd) == sha
    assert lens == edge_lengths(prog)
    for L in lens:
        sigs = synth.make_signals(20260103, 3, L, first_read=60)
        x = np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)
        lg = crnn_ref.forward(prog, x)
        assert np.abs(lg - g[f"{name}.L{L}.logits"]).max() < EDGE_TOL, L
        assert np.abs(ro.softmax(lg) - g[f"{name}.L{L}.probs"]).max() < EDGE_TOL, L


def _create(prog):
    """rs_crnn_create on a host program -> (status, handle value): the argument checks run before a device is touched"""
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    lib = nv.lib()
    convs = (R._Conv * len(prog["convs"]))()
    for i, cv in enumerate(prog["convs"]):
        co, ci, k = cv["w"].shape
        convs[i] = R._Conv(ci, co, k, 0, cv["w"].ctypes.data, cv["b"].ctypes.data)
    layers = (R._Layer * len(prog["layers"]))()
    for i, lay in enumerate(prog["layers"]):
        s = layers[i]
        s.cell, s.in_dim, s.hidden = R.CELLS[lay["cell"]], lay["in_dim"], lay["hidden"]
        s.bidirectional, s.relu_after = int(lay["bidirectional"]), int(lay["relu_after"])
        for d in range(2 if lay["bidirectional"] else 1):
            s.w_ih[d], s.w_hh[d] = lay["w_ih"][d].ctypes.data, lay["w_hh"][d].ctypes.data
            s.b_ih[d], s.b_hh[d] = lay["b_ih"][d].ctypes.data, lay["b_hh"][d].ctypes.data
    h = C.c_void_p()
    rc = lib.rs_crnn_create(convs, len(convs), layers, len(layers), prog["fc_w"].ctypes.data, prog["fc_b"].ctypes.data,
                            int(prog["out_dim"]), 0, C.byref(h))
    return rc, h.value, lib.rs_last_error()


@pytest.mark.parametrize("what,cfg", [
    ("hidden 321", _C([8, 16], [5, 3], "gru", 321, 1, False)),
    ("a 17th conv layer", _C([4] * 17, [1] * 17, "gru", 8, 1, False)),
    # 128 input channels: LDS pitch 132 floats, 64 + k - 1 rows: 61 taps fill 65 472 B, 62 taps need 66 000
    ("a conv tile beyond 64 KB of LDS", _C([128, 8], [3, 62], "lstm", 8, 1, False)),
])
def test_create_refuses_beyond_the_caps(what, cfg):
    from riser_amd import _native as nv
    prog = R.build_crnn_program(synth.make_crnn_state_dict(1, cfg), _ns(cfg))
    rc, handle, msg = _create(prog)
    assert rc == nv.RS_ERR_ARG and not handle, what
    assert b"rs_crnn_create" in msg, msg


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _model(name):
    from riser_amd.model import Model
    cfg, sd, _ = program(name)
    return Model(sd, types.SimpleNamespace(model="cnn-rnn", cnn_rnn=_ns(cfg)), None, "mRNA", device=_dev())


def _pack(sigs, ld=None, lens=None):
    """(x [B, ld] with NaN behind every read, int32 lengths) on the device"""
    import torch
    ld = ld or max(len(s) for s in sigs) + PAD
    x = torch.full((len(sigs), ld), float("nan"), dtype=torch.float32)
    for i, s in enumerate(sigs):
        x[i, :len(s)] = torch.from_numpy(np.ascontiguousarray(s))
    ln = torch.tensor([len(s) for s in sigs] if lens is None else lens, dtype=torch.int32)
    return x.to(_dev()), ln.to(_dev())


def _run(net, sigs, ld=None, lens=None):
    """(probs, logits) as numpy of one forward_ragged call on NaN-padded rows"""
    x, ln = _pack(sigs, ld, lens)
    p, l = net.forward_ragged(x, ln, return_logits=True)
    return p.cpu().numpy(), l.cpu().numpy()


def _solo(net, s):
    import torch
    p, l = net.forward(torch.from_numpy(np.ascontiguousarray(s))[None].to(_dev()), return_logits=True)
    return p.cpu().numpy()[0], l.cpu().numpy()[0]


def _same(a, b):
    """bit for bit, NaN included"""
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _check_f64(name, tag, logits, probs, want):
    scale = np.maximum(1.0, np.abs(want))
    gap = float((np.abs(logits - want) / scale).max())
    dp = float(np.abs(probs - ro.softmax(want)).max())
    print(f"\nCRNN_SWEEP {name} {tag} max|dev-f64|/scale {gap:.3e} probs {dp:.3e}")
    assert gap < TOL[name] and dp < 1e-5, (name, tag, gap, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_sweep(name):
    m = _model(name)
    net = m._seq
    sigs = reads(name)
    assert m.min_length == len(sigs[0]) == R.min_length(program(name)[2])
    probs, logits = _run(net, sigs)                  # classify_batch pads with zeros: the rows here end in NaN
    assert np.isfinite(logits).all() and np.isfinite(probs).all()
    _check_f64(name, "ragged", logits, probs, reference(name))
    for i, s in enumerate(sigs):                     # every read alone, bit for bit
        p1, l1 = _solo(net, s)
        assert _same(l1, logits[i]) and _same(p1, probs[i]), (name, i, len(s))
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_poisoned_workspace(name):
    """the workspace comes from torch.empty and is reused across calls: no kernel may read a cell that this call has not
    written.  Filled with 0xFF bytes every float of it is a NaN."""
    m = _model(name)
    net = m._seq
    small = short_reads(name, 5, 1)
    first = _run(net, small)
    assert np.isfinite(first[1]).all()
    net._ws.fill_(0xFF)
    again = _run(net, small)
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    big = short_reads(name, 21, 2, hi=4000)
    size = net._ws.numel()
    big_first = _run(net, big)
    assert net._ws.numel() > size                    # the larger batch has grown it and left its own values behind
    again = _run(net, small)
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    net._ws.fill_(0xFF)
    again, big_again = _run(net, small), _run(net, big)
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    assert _same(big_first[0], big_again[0]) and _same(big_first[1], big_again[1])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_tile_forms(name):
    m = _model(name)
    net = m._seq
    prog = program(name)[2]
    mn = m.min_length
    pool = short_reads(name, 17, 4)
    solo = [_solo(net, s) for s in pool]
    want = crnn_ref.forward_ragged(prog, pool)
    for B in (1, 15, 16, 17):                        # below, exactly and one above a read tile
        probs, logits = _run(net, pool[:B])
        _check_f64(name, f"B{B}", logits, probs, want[:B])
        for i in range(B):
            assert _same(logits[i], solo[i][1]) and _same(probs[i], solo[i][0]), (B, i)
    # the batch reversed: the rows reversed
    probs, logits = _run(net, pool)
    rp, rl = _run(net, pool[::-1])
    assert _same(rp[::-1], probs) and _same(rl[::-1], logits)
    # one long read among minimum-length ones (one step each, 15 reads wait for the whole recurrence); 16 one-step reads
    ones = [signal(60 + i)[MAX_LEN - mn:] for i in range(16)]
    long_read = signal(59)[MAX_LEN - (mn + 3000):]
    for tag, batch in (("long+15min", ones[:7] + [long_read] + ones[7:15]), ("16min", ones)):
        probs, logits = _run(net, batch)
        _check_f64(name, tag, logits, probs, crnn_ref.forward_ragged(prog, batch))
        for i, s in enumerate(batch):
            p1, l1 = _solo(net, s)
            assert _same(l1, logits[i]) and _same(p1, probs[i]), (tag, i)
    # one fixed read in each of the 16 slots of a tile of otherwise random reads: the same bits in every position
    fixed = signal(58)[MAX_LEN - (mn + 700):]
    p0, l0 = _solo(net, fixed)
    for slot in range(16):
        others = short_reads(name, 15, 100 + slot)
        batch = others[:slot] + [fixed] + others[slot:]
        probs, logits = _run(net, batch)
        assert _same(logits[slot], l0) and _same(probs[slot], p0), slot
        assert np.isfinite(logits).all()
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_length_clamp(name):
    """crnn_len clamps a length to [0, ld]; a read too short for the net gets NaN from last_row_head_kernel (family/head.hpp) and disturbs nobody.
    Defined behaviour of the device program (Model refuses such batches first, so this goes through CRNNNet)."""
    m = _model(name)
    net = m._seq
    mn = m.min_length
    pool = short_reads(name, 16, 5)
    ld = max(len(s) for s in pool)                   # read 3 fills its row: every sample up to the pitch is its own
    pool[3] = signal(57)[MAX_LEN - ld:]
    lens = [len(s) for s in pool]
    base = _run(net, pool, ld=ld)
    over = _run(net, pool, ld=ld, lens=[ld + 1000 if i == 3 else n for i, n in enumerate(lens)])
    assert _same(base[0], over[0]) and _same(base[1], over[1])
    bad = {5: mn - 1, 9: -7}
    probs, logits = _run(net, pool, ld=ld, lens=[bad.get(i, n) for i, n in enumerate(lens)])
    for i in range(16):
        if i in bad:
            assert np.isnan(logits[i]).all() and np.isnan(probs[i]).all(), i
        else:
            assert _same(logits[i], base[1][i]) and _same(probs[i], base[0][i]), i
            p1, l1 = _solo(net, pool[i])
            assert _same(l1, logits[i]) and _same(p1, probs[i]), i
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_grouped_path_gives_the_ragged_bits(name):
    """Model._seq_forward groups the reads by length for an x that is not contiguous (forward_batch itself refuses such an x,
    so the branch is driven directly): one uniform call per length, the ragged call's bits"""
    import torch
    m = _model(name)
    pool = short_reads(name, 6, 6)
    pool = pool + [signal(50 + i)[MAX_LEN - len(s):] for i, s in enumerate(pool[:4])]     # four lengths twice
    x, ln = _pack(pool)
    lens = np.array([len(s) for s in pool], dtype=np.int32)
    probs, logits = m.forward_batch(x, lens, return_logits=True)
    wide = torch.full((len(pool), x.shape[1] + 8), float("nan"), dtype=torch.float32, device=x.device)
    wide[:, :x.shape[1]] = x
    view = wide[:, :x.shape[1]]
    assert not view.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        m.forward_batch(view, lens)
    gp, gl = m._seq_forward(view, lens, True, None)
    assert torch.equal(gp, probs) and torch.equal(gl, logits)
    r = m._seq.forward_ragged(x, ln, return_logits=True)
    assert torch.equal(r[0], probs) and torch.equal(r[1], logits)
    m.close()
