"""float64 numpy forward of the reference ConvRecNet (riser/nets/cnn_rnn.py) from a folded program (riser_amd.crnn), and
mutants of it: the deliberate mistakes a device program could make, which the tests show the tolerances would catch.

    forward(prog, x)                    x: [B, L] (one length) -> logits [B, 2] float64
    forward(prog, x, one_step=False)    the last layer's backward direction over the whole sequence, read at t = T - 1
    forward(prog, x, mutant=name)       name in MUTANTS: mistakes in the model's semantics
    forward_ragged(prog, reads)         reads of any lengths in one batch -> logits [N, 2] float64
    forward_ragged(prog, reads, mutant=name)    name in DEVICE_MUTANTS: mistakes in a device program's indexing - the
                                        alignment of a ragged tile, the pool pairs, the pad columns and the k-panels
"""
import numpy as np

MUTANTS = ("bhn_folded", "lstm_gates_reordered", "no_module_relu", "n_layers_not_squared", "bwd_unreversed",
           "last_bwd_full_sequence")


def mutant_applies(cfg, name) -> bool:
    return {"bhn_folded": cfg["cell"] == "gru", "lstm_gates_reordered": cfg["cell"] == "lstm",
            "no_module_relu": cfg["n_rec_layers"] >= 2, "n_layers_not_squared": cfg["n_rec_layers"] >= 2,
            "bwd_unreversed": bool(cfg["bidirectional"]), "last_bwd_full_sequence": bool(cfg["bidirectional"])}[name]


# mistakes shaped like csrc/crnn.hip: most show only in a batch of reads of different lengths
DEVICE_MUTANTS = ("unstarted_reads_step", "bwd_from_padded_end", "last_bwd_row_of_longest", "pool_pairs_shifted", "pool_ceil",
                  "pad_column_leak", "ktail_dropped")


def device_mutant_applies(cfg, name) -> bool:
    """False where the mutant is the identity on every batch of the config"""
    H, ndir, n2 = cfg["hidden"], 2 if cfg["bidirectional"] else 1, cfg["n_rec_layers"] ** 2
    if name in ("bwd_from_padded_end", "last_bwd_row_of_longest"):
        return bool(cfg["bidirectional"])
    if name == "pad_column_leak":                          # a later layer reads a sequence whose pitch has pad columns
        return n2 >= 2 and (ndir * H) % 4 != 0
    if name == "ktail_dropped":
        ks = [cfg["channels"][cfg["n_conv_layers"] - 1]] + ([ndir * H] if n2 >= 2 else [])
        return H % 16 != 0 or any(k % 16 != 0 for k in ks)
    return True


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def conv_front(prog, x, mutant=None):
    """[B, L] -> [B, T, C] float64: valid conv + bias -> max_pool(2, 2) (floor) -> relu per layer"""
    h = np.asarray(x, dtype=np.float64)[:, None, :]                       # [B, C, L]
    for cv in prog["convs"]:
        w = cv["w"].astype(np.float64)
        co, ci, k = w.shape
        B, C, L = h.shape
        Q = L - k + 1
        if Q < 2:
            raise RuntimeError(f"conv / max_pool: {L} samples into a kernel of {k} leave no pooled output")
        win = np.lib.stride_tricks.sliding_window_view(h, k, axis=2)     # [B, C, Q, k]
        a = np.ascontiguousarray(win.transpose(0, 2, 1, 3)).reshape(B * Q, C * k)
        y = (a @ w.reshape(co, ci * k).T).reshape(B, Q, co) + cv["b"].astype(np.float64)
        P = Q // 2
        if mutant == "pool_pairs_shifted":                 # pairs (1, 2), (3, 4), ...; a missing partner is left out
            y = np.maximum(y[:, 1:2 * P:2], y[:, np.minimum(np.arange(2, 2 * P + 1, 2), Q - 1)])
        elif mutant == "pool_ceil" and Q % 2:              # the trailing odd position is kept as a pool of one
            y = np.concatenate([np.maximum(y[:, 0:2 * P:2], y[:, 1:2 * P:2]), y[:, Q - 1:Q]], axis=1)
        else:
            y = np.maximum(y[:, 0:2 * P:2], y[:, 1:2 * P:2])
        h = np.maximum(y, 0.0).transpose(0, 2, 1)
    return np.ascontiguousarray(h.transpose(0, 2, 1))                     # [B, T, C]


def _run_dir(lay, d, x, reverse, steps=None, mutant=None):
    """one direction of one layer over x [B, T, D] -> outputs [B, T, H] in time order (only the steps run are filled)"""
    cell, H = lay["cell"], lay["hidden"]
    wih, whh = lay["w_ih"][d].astype(np.float64), lay["w_hh"][d].astype(np.float64)
    bih, bhh = lay["b_ih"][d].astype(np.float64), lay["b_hh"][d].astype(np.float64)
    B, T, _ = x.shape
    xp = x @ wih.T + bih                                                  # [B, T, G]
    h = np.zeros((B, H))
    c = np.zeros((B, H))
    out = np.zeros((B, T, H))
    order = list(range(T - 1, -1, -1)) if reverse else list(range(T))
    if steps is not None:
        order = order[:steps]
    for t in order:
        hh = h @ whh.T
        if cell == "lstm":
            gx = xp[:, t] + hh + bhh
            i, f, g, o = (gx[:, j * H:(j + 1) * H] for j in range(4))
            if mutant == "lstm_gates_reordered":
                i, f = f, i
            c = _sig(f) * c + _sig(i) * np.tanh(g)
            h = _sig(o) * np.tanh(c)
        else:
            xr, xz, xn = (xp[:, t, j * H:(j + 1) * H] for j in range(3))
            hr, hz, hn = (hh[:, j * H:(j + 1) * H] for j in range(3))
            br, bz, bn = (bhh[j * H:(j + 1) * H] for j in range(3))
            r, z = _sig(xr + hr + br), _sig(xz + hz + bz)
            n = np.tanh(xn + bn + r * hn) if mutant == "bhn_folded" else np.tanh(xn + r * (hn + bn))
            h = (1.0 - z) * n + z * h
        out[:, t] = h
    return out


def forward(prog, x, one_step=True, mutant=None):
    """logits [B, 2] float64 of reads x [B, L] (one common length)"""
    h = conv_front(prog, x)
    layers = prog["layers"]
    if mutant == "n_layers_not_squared":                   # one layer per module instead of n_rec_layers
        n = int(round(np.sqrt(len(layers))))
        layers = [dict(layers[m * n], relu_after=True) for m in range(n)]
    T = h.shape[1]
    for li, lay in enumerate(layers):
        last = li == len(layers) - 1
        outs = [_run_dir(lay, 0, h, False, mutant=mutant)]
        if lay["bidirectional"]:
            if mutant == "bwd_unreversed":
                outs.append(_run_dir(lay, 1, h, False, mutant=mutant))
            elif mutant == "last_bwd_full_sequence" and last:
                full = _run_dir(lay, 1, h, True, mutant=mutant)
                o = np.zeros_like(full)
                o[:, T - 1] = full[:, 0]                   # the final state of the backward pass (it ends at t = 0)
                outs.append(o)
            else:
                outs.append(_run_dir(lay, 1, h, True, steps=1 if (last and one_step) else None, mutant=mutant))
        h = np.concatenate(outs, axis=2)
        relu = lay["relu_after"] and not (mutant == "no_module_relu" and not last)
        if relu:
            h = np.maximum(h, 0.0)
    return h[:, -1, :] @ prog["fc_w"].astype(np.float64).T + prog["fc_b"].astype(np.float64)


def forward_ragged(prog, reads, mutant=None):
    """logits [N, 2] of reads of any lengths in one batch: the conv front per read, then every layer over the batch with the
    reads' sequences aligned to end on the same step, a read that has not started holding h = c = 0"""
    assert mutant is None or mutant in DEVICE_MUTANTS, mutant
    feats = [conv_front(prog, np.asarray(r)[None], mutant)[0] for r in reads]
    T = np.array([f.shape[0] for f in feats])
    N, Tm = len(reads), int(T.max())
    h = np.zeros((N, Tm, feats[0].shape[1]))
    for i, f in enumerate(feats):
        h[i, Tm - T[i]:] = f                                              # aligned: read i's step q at row Tm - T_i + q
    layers = prog["layers"]
    for li, lay in enumerate(layers):
        last = li == len(layers) - 1
        H = lay["hidden"]
        K = h.shape[2]
        outs = []
        for d in range(2 if lay["bidirectional"] else 1):
            wih, whh = lay["w_ih"][d].astype(np.float64), lay["w_hh"][d].astype(np.float64)
            bih, bhh = lay["b_ih"][d].astype(np.float64), lay["b_hh"][d].astype(np.float64)
            if mutant == "ktail_dropped":                                 # the last partial 16-wide k-panel is skipped
                if K % 16:
                    wih = wih.copy()
                    wih[:, 16 * (K // 16):] = 0.0
                if H % 16:
                    whh = whh.copy()
                    whh[:, 16 * (H // 16):] = 0.0
            # starting at the tile's last row, a shorter read first steps over the zero rows behind its end: the aligned
            # order below, with the steps before its start run and not held
            padded_end = mutant == "bwd_from_padded_end" and d == 1
            if d == 1:                                                    # each read's own sequence, reversed, aligned
                x = np.zeros_like(h)
                for i in range(N):
                    x[i, Tm - T[i]:] = h[i, Tm - T[i]:][::-1]
            else:
                x = h
            xp = x @ wih.T + bih
            if mutant == "pad_column_leak" and li > 0 and K % 4:          # the pitch's first pad column holds 1 and meets
                xp = xp + wih[:, K - 1]                                   # the last real column's weights
            hs, cs = np.zeros((N, H)), np.zeros((N, H))
            o = np.zeros((N, Tm, H))
            steps = range(Tm - 1, Tm) if (last and d == 1) else range(Tm)
            for s in steps:
                live = (s >= Tm - T)[:, None]
                if mutant == "unstarted_reads_step" or padded_end:
                    live = np.ones((N, 1), dtype=bool)
                if last and d == 1:                                      # one step from zero, at each read's last position
                    g = xp[:, 0] if padded_end else np.stack([xp[i, Tm - T[i]] for i in range(N)])
                    if mutant == "last_bwd_row_of_longest":               # row Tmax - 1 of a shorter read: behind its end
                        g = np.where((T < Tm)[:, None], bih, g)
                else:
                    g = xp[:, s]
                if lay["cell"] == "lstm":
                    g = g + hs @ whh.T + bhh
                    i_, f_, g_, o_ = (g[:, j * H:(j + 1) * H] for j in range(4))
                    c2 = _sig(f_) * cs + _sig(i_) * np.tanh(g_)
                    h2 = _sig(o_) * np.tanh(c2)
                else:
                    hh = hs @ whh.T
                    r = _sig(g[:, :H] + hh[:, :H] + bhh[:H])
                    z = _sig(g[:, H:2 * H] + hh[:, H:2 * H] + bhh[H:2 * H])
                    n = np.tanh(g[:, 2 * H:] + r * (hh[:, 2 * H:] + bhh[2 * H:]))
                    h2, c2 = (1.0 - z) * n + z * hs, cs
                hs, cs = np.where(live, h2, hs), np.where(live, c2, cs)
                o[:, s] = hs
            o[np.arange(Tm)[None, :] < (Tm - T)[:, None]] = 0.0           # rows before a read's start are not its own
            if d == 1 and not last:                                     # back to time order
                for i in range(N):
                    o[i, Tm - T[i]:] = o[i, Tm - T[i]:][::-1].copy()
            outs.append(o)
        h = np.concatenate(outs, axis=2)
        if lay["relu_after"]:
            h = np.maximum(h, 0.0)
    return h[:, -1, :] @ prog["fc_w"].astype(np.float64).T + prog["fc_b"].astype(np.float64)
