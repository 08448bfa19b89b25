"""Float64 reference of the ResNet forward, the numpy emulation of its split-precision (bf16x3) arithmetic, mutants of both -
bugs a device program could plausibly have, which the tests must be able to tell apart - and a mirror of the launch planner of
csrc/seqnet.hip (rs_seqnet_create's fusion and packing, the forward's per-op decisions).  A plain module the ResNet tests import."""
import numpy as np

from oracle import resnet_oracle as rr
from riser_amd import resnet as RN

MUTANTS = rr.MUTANTS                                  # flags of the float64 forward
X3_MUTANTS = ("bf16_plain", "no_lohi")                # flags of the emulation: hi.hi only; without the lo(activation).hi(weight) term


# ------------------------------------------------------------------------------------------------ float64
def f64_ragged(sd, cfg, reads, mutant=None):
    """float64 logits [n, 2] of reads of their own lengths: each read through the reference forward alone"""
    return np.concatenate([rr.resnet_forward(sd, cfg, np.asarray(r)[None], mutant=mutant) for r in reads])


# ------------------------------------------------------------------------------------------------ planner mirror
LDS_CAP = 160 * 1024
WINDOW = 0x7FFFFFFF
FAMILIES = ("stem_pool", "basic_block", "bottleneck", "conv_mfma_lds", "conv_mfma", "conv_scalar", "maxpool")


def _r(v, m):
    return (v + m - 1) // m * m


def _dead_after(ops, after, buf):
    for o in ops[after + 1:]:
        if o["src"] == buf or o.get("add", -1) == buf:
            return False
        if o["dst"] == buf:
            return True
    return True


class Program:
    """what rs_seqnet_create makes of a build_program program: per op the unfused MFMA packing (nt, wq) and the fused launches
    (fuse_program) with their fp32 and split-precision pitches and LDS footprints.  env: the create-time switches
    (nofuse, scalar, bneck_x3, window)."""

    def __init__(self, prog, n_buffers, c_last, nofuse=False, scalar=False, bneck_x3=False, window=WINDOW):
        self.n_buffers, self.c_last, self.bneck_x3, self.window = n_buffers, c_last, bneck_x3, min(window, WINDOW)
        self.scalar = scalar
        ops = []
        for p in prog:
            o = dict(kind=p["kind"], src=p["src"], dst=p["dst"], add=p.get("add", -1), pad=int(p.get("pad", 1)), fuse=0, skip=0)
            if p["kind"] == 0:
                co, ci, k = p["w"].shape
                o.update(c_in=ci, c_out=co, k=k, stride=p["stride"], relu=int(p["relu"]))
                nt = (co + 15) // 16
                o["wq"] = nt <= 5 and _r(k * ci, 16) * nt * 16 * 4 <= 96 * 1024
                o["nt"] = nt if o["wq"] else 0
            ops.append(o)
        self.ops = ops
        if not nofuse and not scalar:
            self._fuse()

    def _fuse(self):
        ops = self.ops
        k = 0
        while k < len(ops):
            o = ops[k]
            if o["kind"] != 0:
                k += 1
                continue
            if (o["c_in"] == 1 and o["relu"] and o["add"] < 0 and o["wq"] and k + 1 < len(ops) and ops[k + 1]["kind"] == 1
                    and ops[k + 1]["pad"] == 1 and ops[k + 1]["src"] == o["dst"] and _dead_after(ops, k + 1, o["dst"])):
                o.update(fuse=1, skip=1, f_dst=ops[k + 1]["dst"], x=True)
                k += 1
                continue
            k1, ksc = k, None
            if o["k"] == 1 and o["pad"] == 0 and not o["relu"] and o["add"] < 0 and k + 2 < len(ops):
                ksc, k1 = k, k + 1
            if k1 + 1 >= len(ops):
                k += 1
                continue
            c1, c2 = ops[k1], ops[k1 + 1]
            X = ops[ksc]["src"] if ksc is not None else c1["src"]
            res = ops[ksc]["dst"] if ksc is not None else X
            conv = lambda q: q["kind"] == 0
            shape_ok = (conv(c1) and conv(c2) and c1["k"] == 3 and c1["pad"] == 1 and c1["relu"] and c1["add"] < 0
                        and c1["src"] == X and c2["k"] == 3 and c2["pad"] == 1 and c2["stride"] == 1 and c2["relu"]
                        and c2["src"] == c1["dst"] and c2["add"] == res and c2["c_in"] == c1["c_out"] and c2["c_out"] == c1["c_out"]
                        and c2["dst"] != X and c1["dst"] != X
                        and ((ops[ksc]["stride"] == c1["stride"] and ops[ksc]["c_in"] == c1["c_in"] and ops[ksc]["c_out"] == c1["c_out"])
                             if ksc is not None else (c1["stride"] == 1 and c1["c_in"] == c1["c_out"])))
            if not shape_ok:
                if k1 + 2 >= len(ops):
                    k += 1
                    continue
                d1, d2, d3 = ops[k1], ops[k1 + 1], ops[k1 + 2]
                bn_ok = (conv(d1) and conv(d2) and conv(d3) and d1["k"] == 1 and d1["pad"] == 0 and d1["stride"] == 1 and d1["relu"]
                         and d1["add"] < 0 and d1["src"] == X and d2["k"] == 3 and d2["pad"] == 1 and d2["relu"] and d2["add"] < 0
                         and d2["src"] == d1["dst"] and d2["c_in"] == d1["c_out"] and d2["c_out"] == d1["c_out"] and d3["k"] == 1
                         and d3["pad"] == 0 and d3["stride"] == 1 and d3["relu"] and d3["src"] == d2["dst"] and d3["add"] == res
                         and d3["c_in"] == d2["c_out"] and d3["dst"] != X and d1["dst"] != X and d2["dst"] != X
                         and ((ops[ksc]["stride"] == d2["stride"] and ops[ksc]["c_in"] == d1["c_in"] and ops[ksc]["c_out"] == d3["c_out"])
                              if ksc is not None else (d2["stride"] == 1 and d1["c_in"] == d3["c_out"])))
                if not bn_ok or d2["stride"] not in (1, 2):
                    k += 1
                    continue
                if (not _dead_after(ops, k1 + 2, d1["dst"]) or not _dead_after(ops, k1 + 2, d2["dst"])
                        or (ksc is not None and not _dead_after(ops, k1 + 2, res))):
                    k += 1
                    continue
                c_in, c_mid, c_out = d1["c_in"], d1["c_out"], d3["c_out"]
                ntm, nto = (c_mid + 15) // 16, (c_out + 15) // 16
                if ntm > 2 or nto > 5:
                    k += 1
                    continue
                Cmp = _r(c_mid, 4)
                if (Cmp // 4) % 2 == 0:
                    Cmp += 4
                NPm, NPo = _r(c_mid, 4), _r(c_out, 4)
                Ksc = c_in if ksc is not None else 0
                w_floats = (_r(c_in, 16) + _r(3 * Cmp, 16)) * NPm + (_r(Cmp, 16) + _r(Ksc, 16)) * NPo
                if (w_floats + 2 * (128 + 4) * Cmp) * 4 > LDS_CAP:
                    k += 1
                    continue
                Cmx = _r(c_mid, 8)
                while Cmx % 16 != 8:
                    Cmx += 8
                S1, S2, S3, Sscx = (c_in + 31) // 32, (3 * Cmx + 31) // 32, (Cmx + 31) // 32, (Ksc + 31) // 32
                xbytes = ((S1 + S2) * 4 * NPm * 8 + (S3 + Sscx) * 4 * NPo * 8) * 4
                o.update(fuse=3, skip=k1 + 2 - k, f_dst=d3["dst"], f_cin=c_in, f_cout=c_out, f_cmid=c_mid, f_stride=d2["stride"],
                         f_ntm=ntm, f_nt=nto, f_np=NPo, f_cp=Cmp, f_wbytes=4 * w_floats,
                         x=xbytes + 2 * (128 + 4) * Cmx * 4 <= LDS_CAP, x_cp=Cmx, x_wbytes=xbytes)
                k = k1 + 3
                continue
            if not _dead_after(ops, k1 + 1, c1["dst"]) or (ksc is not None and not _dead_after(ops, k1 + 1, res)):
                k += 1
                continue
            c_in, c_out = c1["c_in"], c1["c_out"]
            nt = (c_out + 15) // 16
            if nt > 5:
                k += 1
                continue
            NP = 16 * nt
            if (_r(3 * c_in, 16) + _r(3 * (c_out + 7), 16) + _r(c_in, 16)) * NP * 4 > 60 * 1024:
                NP = _r(c_out, 4)
            Cp = _r(c_out, 4)
            if (Cp // 4) % 2 == 0:
                Cp += 4
            Ksc = c_in if ksc is not None else 0
            w_floats = (_r(3 * c_in, 16) + _r(3 * Cp, 16) + _r(Ksc, 16)) * NP
            if (w_floats + (64 + 4) * Cp) * 4 > LDS_CAP:
                k += 1
                continue
            Cpx = _r(c_out, 8)
            while Cpx % 16 != 8:
                Cpx += 8
            S = (3 * c_in + 31) // 32 + (3 * Cpx + 31) // 32 + (Ksc + 31) // 32
            NPx = 16 * nt
            if S * 128 * NPx > 60 * 1024:
                NPx = _r(c_out, 4)
            wbytes = S * 128 * NPx
            o.update(fuse=2, skip=k1 + 1 - k, f_dst=c2["dst"], f_cin=c_in, f_cout=c_out, f_stride=c1["stride"], f_nt=nt, f_np=NP,
                     f_cp=Cp, f_wbytes=4 * w_floats, x=wbytes + (64 + 4) * Cpx * 4 <= LDS_CAP, x_np=NPx, x_cp=Cpx, x_wbytes=wbytes)
            k = k1 + 2

    def ragged_ok(self):
        k = 0
        while k < len(self.ops):
            if not 1 <= self.ops[k]["fuse"] <= 3:
                return False
            k += 1 + self.ops[k]["skip"]
        return len(self.ops) <= 63

    def x3_ok(self):
        """rs_seqnet_set_mode(RS_BF16X3) accepts the program: one fused residual block with a split-precision packing"""
        return any(o["fuse"] in (2, 3) and o["x"] for o in self.ops)

    def shapes(self, L):
        """per op (t_in, t_out, c_in, c_out), or None where the forward refuses the length"""
        T, C = {0: L}, {0: 1}
        out = []
        for o in self.ops:
            t = T.get(o["src"], -1)
            if t < 0:
                return None
            if o["kind"] == 0:
                if t + 2 * o["pad"] < o["k"]:
                    return None
                to, c = (t + 2 * o["pad"] - o["k"]) // o["stride"] + 1, o["c_out"]
            else:
                to, c = (t // 2 + 1 if o["pad"] else t // 2), C[o["src"]]
            if to < 1:
                return None
            if o["add"] >= 0 and (T.get(o["add"]) != to or C.get(o["add"]) != c):
                return None
            out.append((t, to, C[o["src"]], c))
            T[o["dst"]], C[o["dst"]] = to, c
        return out

    def min_length(self):
        L = 1
        while self.shapes(L) is None:
            L += 1
        return L

    def plan(self, B, L, mode="f32", ragged=False):
        """the launch list rs_seqnet_launch_plan returns: dicts of rs_seq_launch's fields (family by name).  Raises ValueError
        where the forward refuses."""
        x3 = mode == "bf16x3"
        if x3 and not self.x3_ok():
            raise ValueError("set_mode refuses bf16x3")
        if ragged and not self.ragged_ok():
            raise ValueError("not ragged_ok")
        shp = self.shapes(L)
        if shp is None:
            raise ValueError("too short")
        W, out, k = self.window, [], 0
        while k < len(self.ops):
            o = self.ops[k]
            l = dict(op=k, n_ops=1, family=None, nt=0, ntm=0, mtw=0, waves=0, np=0, cp=0, x3=0)
            f, s = o["fuse"], o["skip"]
            if f == 1 and B * 2 * shp[k + 1][1] < W and B * shp[k][0] * 4 < W:
                l.update(family="stem_pool", nt=o["nt"], np=16 * o["nt"], x3=int(x3))
            elif f == 2 and B * shp[k + s][0] * o["f_cout"] * 4 < W and B * shp[k + s - 1][0] * o["f_cin"] * 4 < W:
                t_out = shp[k + s - 1][1]
                if x3 and o["x"]:
                    l.update(x3=1, np=o["x_np"], cp=o["x_cp"])
                    l.update(block_tile(o["x_wbytes"], 4 * o["x_cp"], t_out))
                else:
                    l.update(np=o["f_np"], cp=o["f_cp"])
                    l.update(block_tile(o["f_wbytes"], 4 * o["f_cp"], t_out))
                l.update(family="basic_block", nt=o["f_nt"])
            elif f == 3 and B * shp[k + s - 2][0] * o["f_cin"] * 4 < W and B * shp[k + s - 1][1] * o["f_cout"] * 4 < W:
                bx = x3 and self.bneck_x3 and o["x"]
                l.update(family="bottleneck", ntm=o["f_ntm"], nt=o["f_nt"], np=o["f_np"], cp=o["x_cp"] if bx else o["f_cp"], x3=int(bx))
            elif ragged:
                raise ValueError("a fused launch beyond the buffer window")
            elif o["kind"] == 0 and self.scalar:
                l.update(family="conv_scalar")
            elif o["kind"] == 0 and o["wq"] and B * shp[k][0] * o["c_in"] * 4 < W:
                l.update(family="conv_mfma_lds", nt=o["nt"], np=16 * o["nt"])
            elif o["kind"] == 0:
                co = o["c_out"]
                l.update(family="conv_mfma", nt=1 if co <= 16 else 2 if co <= 32 else 4, np=_r(co, 4))
            else:
                l.update(family="maxpool")
            if l["family"] in ("stem_pool", "basic_block", "bottleneck"):
                l["n_ops"] = 1 + s
            out.append(l)
            k += l["n_ops"]
        return out


def block_tile(w_bytes, row_bytes, t_out):
    """(mtw, waves) of a basic block: csrc/seqnet.hip block_tile"""
    lds_of = lambda rows: w_bytes + (rows + 4) * row_bytes

    def waste(rows):
        to = rows - 2
        n = (t_out + to - 1) // to
        return (n * to - t_out) / (n * to)
    mtw, waves = 1, 4
    if LDS_CAP // lds_of(64) < 2:
        if lds_of(128) <= LDS_CAP:
            waves = 8
    elif LDS_CAP // lds_of(128) >= 2 and waste(128) < 0.06:
        mtw = 2
    return dict(mtw=mtw, waves=waves)


def instantiation(l):
    """the kernel instantiation of a launch, e.g. 'basic_block_x3<2,1,8>'"""
    f = l["family"] + ("_x3" if l["x3"] else "")
    if l["family"] == "basic_block":
        return f"{f}<{l['nt']},{l['mtw']},{l['waves']}>"
    if l["family"] == "bottleneck":
        return f"{f}<{l['ntm']},{l['nt']}>"
    if l["family"] in ("stem_pool", "conv_mfma_lds", "conv_mfma"):
        return f"{f}<{l['nt']}>"
    return f


def all_instantiations():
    """every kernel instantiation the forward can launch (its dispatch tables)"""
    s = set()
    for nt in range(1, 6):
        for x in ("", "_x3"):
            s.add(f"stem_pool{x}<{nt}>")
            for mw in ("1,4", "2,4", "1,8"):
                s.add(f"basic_block{x}<{nt},{mw}>")
            for ntm in (1, 2):
                s.add(f"bottleneck{x}<{ntm},{nt}>")
        s.add(f"conv_mfma_lds<{nt}>")
    return s | {"conv_mfma<1>", "conv_mfma<2>", "conv_mfma<4>", "conv_scalar", "maxpool"}


# ------------------------------------------------------------------------------------------------ split-precision emulation
def bf16(v):
    """fp32 -> the fp32 value of its bf16 rounding, to nearest even (v_cvt_pk_bf16_f32, the host packer's bf16_rne)"""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def split(v):
    """fp32 -> (hi, lo) bf16 values as float64: hi = bf16(v), lo = bf16(v - hi)"""
    v = np.asarray(v, dtype=np.float32)
    hi = bf16(v)
    return hi.astype(np.float64), bf16(v - hi).astype(np.float64)


def _conv(x, w, stride, pad):
    """float64 conv1d, x [C, T] -> [Co, T_out] (no bias)"""
    import torch
    import torch.nn.functional as F
    return F.conv1d(torch.from_numpy(x)[None], torch.from_numpy(w), stride=stride, padding=pad)[0].numpy()


def _conv_x3(x, w, stride, pad, mutant=None):
    """the device's split product of fp32 activations x [C, T] and fp32 weights w: hi.hi + lo.hi + hi.lo, every bf16 product
    exact in float64"""
    xh, xl = split(x)
    wh, wl = split(w)
    y = _conv(xh, wh, stride, pad)
    if mutant == "bf16_plain":
        return y
    if mutant != "no_lohi":
        y = y + _conv(xl, wh, stride, pad)
    return y + _conv(xh, wl, stride, pad)


def _pool(h, pad):
    C, T = h.shape
    if pad:
        hp = np.full((C, T + 2), -np.inf)
        hp[:, 1:T + 1] = h
        To = T // 2 + 1
    else:
        hp, To = h, T // 2
    return np.maximum(hp[:, 0:2 * To:2], hp[:, 1:2 * To:2])


def x3_forward(prog, fw, fb, pm, x, mutant=None):
    """emulated bf16x3 logits [2] of one read x: prog = build_program's folded fp32 program, pm = its Program (the launch plan
    says which launches run split); the stem and every split block as the x3 kernels compute them (bias, ReLU, pooling and
    the identity shortcut in fp32 / float64, activations stored as fp32 between launches), every other launch in float64"""
    assert mutant is None or mutant in X3_MUTANTS
    plan = pm.plan(1, len(x), "bf16x3")
    buf = {0: np.asarray(x, dtype=np.float32)[None, :].astype(np.float64)}
    W = lambda o: o["w"].astype(np.float64)
    for l in plan:
        k = l["op"]
        ops = prog[k:k + l["n_ops"]]
        if l["x3"] and l["family"] == "stem_pool":
            o = ops[0]
            h = np.maximum(_conv_x3(buf[o["src"]], o["w"], o["stride"], o["pad"], mutant) + o["b"][:, None], 0)
            buf[ops[1]["dst"]] = _pool(h.astype(np.float32).astype(np.float64), 1)
        elif l["x3"]:
            sc = ops[0] if len(ops) == (3 if l["family"] == "basic_block" else 4) else None
            body = ops[1:] if sc is not None else ops
            X = buf[body[0]["src"]]
            h = X
            for i, o in enumerate(body):
                last = i == len(body) - 1
                acc = _conv_x3(h, o["w"], o["stride"], o["pad"], mutant) + o["b"][:, None]
                if not last:
                    h = np.maximum(acc, 0).astype(np.float32).astype(np.float64)
            if sc is not None:
                acc = acc + _conv_x3(X, sc["w"], sc["stride"], 0, mutant) + sc["b"][:, None]
            else:
                acc = acc + X
            buf[body[-1]["dst"]] = np.maximum(acc, 0).astype(np.float32).astype(np.float64)
        else:
            for o in ops:
                if o["kind"] == 0:
                    y = _conv(buf[o["src"]], W(o), o["stride"], o["pad"]) + o["b"][:, None]
                    if o["add"] >= 0:
                        y = y + buf[o["add"]]
                    buf[o["dst"]] = (np.maximum(y, 0) if o["relu"] else y).astype(np.float32).astype(np.float64)
                else:
                    buf[o["dst"]] = _pool(buf[o["src"]], o.get("pad", 1))
    last = prog[plan[-1]["op"] + plan[-1]["n_ops"] - 1]["dst"]
    return buf[last].mean(axis=1) @ fw.astype(np.float64).T + fb.astype(np.float64)


def x3_ragged(sd, cfg, reads, mutant=None, bneck_x3=False):
    """emulated bf16x3 logits [n, 2] of reads of their own lengths (bneck_x3: the program created under RS_SEQ_BNECK_X3=1)"""
    import types
    prog, nb, fw, fb, c_last = RN.build_program(sd, types.SimpleNamespace(**cfg))
    pm = Program(prog, nb, c_last, bneck_x3=bneck_x3)
    return np.stack([x3_forward(prog, fw, fb, pm, r, mutant) for r in reads])


def skeleton(cfg):
    """(prog, n_buffers, c_last) with build_program's op list for a config, weights as zero arrays of the right shapes: what
    the planner mirror needs to enumerate configs without building their weights"""
    z = lambda co, ci, k: np.zeros((co, ci, k), np.float32)
    ops = [dict(kind=0, src=0, dst=1, add=-1, w=z(cfg["channels"][0], 1, cfg["kernel"]), b=None, stride=cfg["stride"],
                pad=cfg["padding"], relu=1), dict(kind=1, src=1, dst=2, add=-1, pad=1)]
    cur, in_ch, nb = 2, cfg["channels"][0], 7
    for i in range(cfg["n_layers"]):
        out_ch = cfg["channels"][i]
        for j in range(cfg["blocks"][i]):
            stride = 2 if (i > 0 and j == 0) else 1
            free = [k for k in range(1, nb) if k != cur]
            res = cur
            if in_ch != out_ch or stride != 1:
                res = free.pop()
                ops.append(dict(kind=0, src=cur, dst=res, add=-1, w=z(out_ch, in_ch, 1), stride=stride, pad=0, relu=0))
            if cfg["block"] == "bottleneck":
                mid = out_ch // 4
                t1, t2, t3 = free.pop(), free.pop(), free.pop()
                ops += [dict(kind=0, src=cur, dst=t1, add=-1, w=z(mid, in_ch, 1), stride=1, pad=0, relu=1),
                        dict(kind=0, src=t1, dst=t2, add=-1, w=z(mid, mid, 3), stride=stride, pad=1, relu=1),
                        dict(kind=0, src=t2, dst=t3, add=res, w=z(out_ch, mid, 1), stride=1, pad=0, relu=1)]
                cur = t3
            else:
                t1, t2 = free.pop(), free.pop()
                ops += [dict(kind=0, src=cur, dst=t1, add=-1, w=z(out_ch, in_ch, 3), stride=stride, pad=1, relu=1),
                        dict(kind=0, src=t1, dst=t2, add=res, w=z(out_ch, out_ch, 3), stride=1, pad=1, relu=1)]
                cur = t2
            in_ch = out_ch
    return ops, nb, in_ch
