"""The pixel step (vlg/image_engine.py over vlg/gridnet.py, vlg/hned.py, vlg/vgg_loss.py) as a contract: the launches of one
ImageEngine.forward + backward, in order, with the NAME of the buffer behind every pointer operand and the flags word, plus one
stage function per launch kind.  Plain module: test infrastructure, nothing collected.

schedule() is restated from the reference's structure - oracle/gridnet_spec.py (forward, block_list), oracle/hned_spec.py,
oracle/vgg_spec.py and image_engine.py's docstring for the two ends - NOT read from net.tape, vgg.ops or the HED op list: the
schedule is what those are held to (tests/image_trace.py).  Rules the graph alone gives:
  forward   a sum of two branches is the RESID epilogue of the last convolution of the lateral block (lateral_in: of the block,
            its shortcut convolution runs first); a PReLU, and the trunks' ReLU, is applied on load by the consuming convolution
            (slope operand; activated channels = the tensor's own, never its AddCoords lanes)
  backward  per convolution, last to first: weight gradient; data gradient (skipped only for the network input without a
            PReLU); vlg_add_rows into the residual branch.  ACCUM / accumulate = an earlier launch of this backward already
            wrote that gradient tensor.  DPRELU = an activation precedes the convolution.  CIN4 = the trunks' image layer.
            One vlg_reduce_slabs_table, then one vlg_sum_partials_table.  "_bf16" on every 3x3 convolution, on nothing else,
            exactly under precision == "bf16".
Names: "g:<conv key>" is the output of that GridNet convolution ("g:x" the input, "g:<block>.up.0" an upsampled tensor),
"d.<tensor>" its gradient, "g.p:<state_dict key>" a parameter, "slab:<key>" / "da:<key>" a convolution's regions of the
weight-gradient and slope-gradient arenas; "hed:" / "vgg:" likewise for the frozen trunks; x10, f3, seg3, img, img_raw, seg,
dimg, dtmp, dseg, losses[k], scratch and batch:<key> are the engine's NCHW buffers.

Stage functions take the launch's named inputs and a dtype: float64 is the reference, float32 torch-CPU's own error.  The
convolution reference IS test_hip_conv_bf16._ref (activation in fp32, operands rounded to bf16 or not, the fp32 path's epilogues);
conv_parts restates it only for the other dtypes (tests/test_image_trace_cpu.py holds the two equal at float64).  Resampling,
pooling and the HED / VGG heads are test_hip_pixel_ops' references, the four image losses oracle/image_step_spec's expressions
(the checker compares those launches with oracle/image_ref.py, as the kernels' own tests do).
emulate() chains the stage functions into the record format image_trace.trace writes on the GPU."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import test_hip_conv_bf16 as CB
import test_hip_pixel_ops as PX
from oracle import gridnet_spec as GS
from oracle import hned_spec as HS
from oracle import image_step_spec as IS
from oracle import vgg_spec as VS
from vlg.hip import CEPI_ACCUM, CEPI_CIN4, CEPI_DPRELU, CEPI_RESID      # include/vlg_hip.h VLG_CEPI_*

W_L1, W_STYLE, W_CE = 40.0, 20.0, 10.0                                  # reference src/trainer.py:248-250
IMG_MEAN, IMG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)        # trainer.py:122-123
OUT_MEAN, OUT_STD = (-0.03, -0.088, -0.188), (0.448, 0.448, 0.450)      # trainer.py:120-121
BGR_MEAN = (104.00698793, 116.66876762, 122.67891434)                   # hned.py:74-76
BATCH_KEYS = ("e1", "seg1", "frame1", "frame2", "seg2", "e2", "frame3", "seg3")
F32, F64 = torch.float32, torch.float64


def _ceil32(c):
    return (c + 31) // 32 * 32


def _f32(v):
    return float(np.float32(v))


def const(values):
    """the name of a host array of floats (the affine kernels' shift / scale operands), by value"""
    return "c(%s)" % ",".join("%.9g" % _f32(v) for v in values)


class Geo:
    """padded geometry of one resolution level (vlg/gridnet.py _Geo): (b, H+2, W+2) rows between W+2+40 guard rows"""

    def __init__(self, b, H, W):
        self.b, self.H, self.W = b, H, W
        self.wp = W + 2
        self.rows = b * (H + 2) * (W + 2)
        self.guard = self.wp + 40


class Shape:
    def __init__(self, b, H, W):
        self.b, self.H, self.W = b, H, W

    def geo(self, level):
        return Geo(self.b, self.H >> level, self.W >> level)


class Ten:
    """a padded channels-last tensor of the contract: C channels (+2 AddCoords lanes) in cp = ceil32 lanes"""

    def __init__(self, name, level, C, coord=False):
        self.name, self.level, self.C, self.coord = name, level, C, coord
        self.cin = C + (2 if coord else 0)
        self.cp = _ceil32(self.cin)

    def numel(self, sh):
        g = sh.geo(self.level)
        return (g.rows + 2 * g.guard) * self.cp

    def grid(self, flat, sh):
        g = sh.geo(self.level)
        return flat[g.guard * self.cp:(g.guard + g.rows) * self.cp].view(g.b, g.H + 2, g.W + 2, self.cp)

    def nchw(self, flat, sh, C=None):
        return self.grid(flat, sh)[:, 1:-1, 1:-1, :self.cin if C is None else C].permute(0, 3, 1, 2).contiguous()

    def pack(self, x, sh, base=None):
        """x (b, C', H, W) into lanes [0, C') of the interior of a copy of base (default: zeros)"""
        flat = torch.zeros(self.numel(sh), dtype=x.dtype) if base is None else base.clone()
        self.grid(flat, sh)[:, 1:-1, 1:-1, :x.shape[1]] = x.permute(0, 2, 3, 1)
        return flat

    def grad(self):
        return Ten("d." + self.name, self.level, self.cin)


class Conv:
    def __init__(self, net, key, x, out, stride=1, slope=None, resid=None, cin4=False):
        self.net, self.key, self.x, self.out, self.stride, self.slope, self.resid, self.cin4 = net, key, x, out, stride, slope, resid, cin4
        self.cin, self.cout = x.cin, out.C
        self.act = x.C                       # activated channels: the tensor's own, never its AddCoords lanes
        self.wname, self.bname = "%s.p:%s.weight" % (net, key), "%s.p:%s.bias" % (net, key)
        self.sname = None if slope is None else "%s.p:%s" % (net, slope)
        self.slab_stride = out.cp * 9 * x.cp + out.cp


# ------------------------------------------------------------------------------------------------ graphs
def grid_graph(arch, filters, n_channels=10, seg_out=20, img_out=3):
    """GridNet.forward / CoordGridNet.forward as oracle/gridnet_spec.forward writes them -> (ops, x, seg, img); ops are
    ("conv", Conv) | ("up", src, dst) in launch order."""
    coord = arch == "CoordGridNet"
    f = tuple(filters)
    kinds = {name: (kind, li, lo) for name, kind, li, lo in GS.block_list()}
    ops = []

    def conv(key, x, cout, stride=1, prelu=None, resid=None, out_coord=False):
        out = Ten("g:" + key, x.level + (1 if stride == 2 else 0), cout, out_coord)
        ops.append(("conv", Conv("g", key, x, out, stride, prelu, resid)))
        return out

    def block(name, kind, x, cout, resid=None):
        if kind == "up":
            u = Ten("g:%s.up.0" % name, x.level - 1, x.C)
            ops.append(("up", x, u))
            t = conv(name + ".up.2", u, cout, prelu=name + ".up.1.weight")
            return conv(name + ".up.4", t, cout, prelu=name + ".up.3.weight", resid=resid)
        t = conv(name + ".conv.1", x, cout, 2 if kind == "down" else 1, prelu=name + ".conv.0.weight")
        return conv(name + ".conv.3", t, cout, prelu=name + ".conv.2.weight", resid=resid)

    def grid(name, x, resid=None):
        kind, li, lo = kinds[name]
        assert x.level == li and x.C == f[li], name
        return block(name, kind, x, f[lo], resid)

    xin = Ten("g:x", 0, n_channels, coord)
    if coord:
        t = conv("lateral_in.conv.0.conv", xin, f[0], out_coord=True)
        s = conv("lateral_in.conv2.conv", xin, f[0])
        x0 = conv("lateral_in.conv.2.conv", t, f[0], prelu="lateral_in.conv.1.weight", resid=s)
    else:
        s = conv("lateral_in.conv2", xin, f[0])
        x0 = block("lateral_in", "lateral", xin, f[0], resid=s)
    x1 = grid("down_00", x0)
    x2 = grid("down_10", x1)
    for i in range(1, 6):
        if i < 3:
            x0 = grid("lateral_0%d" % (i - 1), x0)
            x1 = grid("lateral_1%d" % (i - 1), x1, resid=grid("down_0%d" % i, x0))
            x2 = grid("lateral_2%d" % (i - 1), x2, resid=grid("down_1%d" % i, x1))
        else:
            x2 = grid("lateral_2%d" % (i - 1), x2)
            x1 = grid("lateral_1%d" % (i - 1), x1, resid=grid("up_1%d" % i, x2))
            x0 = grid("lateral_0%d" % (i - 1), x0, resid=grid("up_0%d" % i, x1))
    seg = block("lateral_out_seg", "lateral", x0, seg_out)
    img = block("lateral_out_img", "lateral", x0, img_out)
    return ops, xin, seg, img


def hed_graph():
    """oracle/hned_spec.forward's trunk -> (ops, x, feats); ops are ("conv", Conv) | ("pool", src, dst)."""
    ops, feats = [], []
    t = x = Ten("hed:x", 0, 3)
    for si, (name, cin, cout, idx) in enumerate(HS.STAGES):
        if si > 0:
            p = Ten("hed:pool%d" % si, si, cin)
            ops.append(("pool", t, p))
            t = p
        for j, i in enumerate(idx):
            first = si == 0 and j == 0
            o = Ten("hed:%s.%d" % (name, i), si, cout)
            ops.append(("conv", Conv("hed", "%s.%d" % (name, i), t, o, slope=None if first else "_zero", cin4=first)))
            t = o
        feats.append(t)
    return ops, x, feats


def vgg_graph():
    """oracle/vgg_spec.features -> (ops, x, feat)"""
    ops, idx, level = [], 0, 0
    t = x = Ten("vgg:x", 0, 3)
    for v in VS.CFG:
        if v == "M":
            level += 1
            p = Ten("vgg:pool%d" % level, level, t.C)
            ops.append(("pool", t, p))
            t = p
            idx += 1
        else:
            first = idx == 0
            o = Ten("vgg:features.%d" % idx, level, v)
            ops.append(("conv", Conv("vgg", "features.%d" % idx, t, o, slope=None if first else "_zero", cin4=first)))
            t = o
            idx += 2
    return ops, x, t


class Contract:
    """Everything the schedule fixes for one engine configuration (no sizes: those are a Shape)."""

    def __init__(self, arch, filters, with_hed=False, with_vgg=False, precision="fp32"):
        assert arch in ("GridNet", "CoordGridNet") and precision in ("fp32", "bf16")
        self.arch, self.filters, self.with_hed, self.with_vgg, self.precision = arch, tuple(filters), with_hed, with_vgg, precision
        self.coord = arch == "CoordGridNet"
        self.bf16 = precision == "bf16"
        self.ops, self.x, self.seg, self.img = grid_graph(arch, filters)
        self.convs = [op[1] for op in self.ops if op[0] == "conv"]
        self.tens = {}
        for c in self.convs:
            for t in (c.x, c.out):
                self.tens[t.name] = t
        for op in self.ops:
            if op[0] == "up":
                self.tens[op[2].name] = op[2]
        # parameter layout (vlg/gridnet.py: [cout_p][9][cin_p] + [cout_p] per convolution in launch order, then 4 floats a slope)
        self.off, off = {}, 0
        for c in self.convs:
            self.off[c.wname], self.off[c.bname] = off, off + c.out.cp * 9 * c.x.cp
            off += c.slab_stride
        for c in self.convs:
            if c.slope:
                self.off[c.sname] = off
                off += 4
        self.n_params_padded = off
        self.nets = {"g": self}
        if with_hed:
            self.hed = Trunk("hed")
            self.nets["hed"] = self.hed
        if with_vgg:
            self.vgg = Trunk("vgg")
            self.nets["vgg"] = self.vgg
        self.schedule = _schedule(self)

    def sym(self, name):
        return name + "_bf16" if self.bf16 else name

    # ---- parameters in the kernels' flat layout
    def pack_params(self, sd, dt=F32):
        return _pack(self, sd, dt)

    def padded_lanes(self):
        """bool mask over the flat parameter layout: True on every lane that holds no parameter - lanes >= cin of every tap,
        rows >= cout, bias lanes >= cout, the 3 floats behind each slope - from the reference's shapes and the 32-lane rule."""
        shapes = GS.param_shapes(filters=self.filters, coord=self.coord)
        pad = torch.ones(self.n_params_padded, dtype=torch.bool)
        seen = set()
        for c in self.convs:
            cout, cin = shapes[c.key + ".weight"][:2]
            assert (cout,) == tuple(shapes[c.key + ".bias"])
            cin_p, cout_p = _ceil32(cin), _ceil32(cout)
            o = self.off[c.wname]
            pad[o:o + cout_p * 9 * cin_p].view(cout_p, 9, cin_p)[:cout, :, :cin] = False
            pad[self.off[c.bname]:self.off[c.bname] + cout] = False
            seen |= {c.key + ".weight", c.key + ".bias"}
            if c.slope:
                assert tuple(shapes[c.slope]) == (1,)
                pad[self.off[c.sname]] = False
                seen.add(c.slope)
        assert seen == set(shapes), "the contract's parameters are not the reference's"
        return pad


class Trunk:
    """a frozen trunk's graph and flat parameter layout (vlg/hned.py, vlg/vgg_loss.py)"""

    def __init__(self, net):
        self.net = net
        if net == "hed":
            self.ops, self.x, self.feats = hed_graph()
        else:
            self.ops, self.x, self.feat = vgg_graph()
        self.convs = [op[1] for op in self.ops if op[0] == "conv"]
        self.off, off = {}, 0
        for c in self.convs:
            self.off[c.wname], self.off[c.bname] = off, off + c.out.cp * 9 * c.x.cp
            off += c.slab_stride
        if net == "hed":
            for name, (_, _, cout, _) in zip(HS.SCORES, HS.STAGES):
                self.off["hed.p:%s.weight" % name], self.off["hed.p:%s.bias" % name] = off, off + cout
                off += cout + 4
            self.off["hed.p:moduleCombine.0.weight"], self.off["hed.p:moduleCombine.0.bias"] = off, off + 8
            off += 12
        self.off[net + ".p:_zero"] = off
        self.n_params_padded = off + 4

    def pack_params(self, sd, dt=F32):
        flat = _pack(self, sd, dt)
        if self.net == "hed":
            for name in HS.SCORES + ("moduleCombine.0",):
                for part in (".weight", ".bias"):
                    v = sd[name + part].to(dt).flatten()
                    o = self.off["hed.p:" + name + part]
                    flat[o:o + v.numel()] = v
        return flat


def _pack(net, sd, dt):
    flat = torch.zeros(net.n_params_padded, dtype=dt)
    for c in net.convs:
        wp = torch.zeros(c.out.cp, 9, c.x.cp, dtype=dt)
        wp[:c.cout, :, :c.cin] = sd[c.key + ".weight"].to(dt).permute(0, 2, 3, 1).reshape(c.cout, 9, c.cin)
        o = net.off[c.wname]
        flat[o:o + wp.numel()] = wp.flatten()
        flat[net.off[c.bname]:net.off[c.bname] + c.cout] = sd[c.key + ".bias"].to(dt)
        if c.slope and c.slope != "_zero":
            flat[net.off[c.sname]] = sd[c.slope].to(dt).flatten()[0]
    return flat


def conv_params(net, flat, c):
    """(weight (cout,cin,3,3), bias (cout,), slope float | None) of convolution c out of the flat buffer"""
    o = net.off[c.wname]
    w = flat[o:o + c.out.cp * 9 * c.x.cp].view(c.out.cp, 3, 3, c.x.cp)[:c.cout, :, :, :c.cin].permute(0, 3, 1, 2).contiguous()
    b = flat[net.off[c.bname]:net.off[c.bname] + c.cout].clone()
    return w, b, None if c.sname is None else float(flat[net.off[c.sname]])


def unpack_slab(c, v):
    """one [cout_p][9][cin_p] + [cout_p] block -> (dW (cout,cin,3,3), db (cout,))"""
    n = c.out.cp * 9 * c.x.cp
    return v[:n].view(c.out.cp, 3, 3, c.x.cp)[:c.cout, :, :, :c.cin].permute(0, 3, 1, 2).contiguous(), v[n:n + c.cout].clone()


def pack_slab(c, dw, db):
    v = torch.zeros(c.slab_stride, dtype=dw.dtype)
    n = c.out.cp * 9 * c.x.cp
    v[:n].view(c.out.cp, 9, c.x.cp)[:c.cout, :, :c.cin] = dw.permute(0, 2, 3, 1).reshape(c.cout, 9, c.cin)
    v[n:n + c.cout] = db
    return v


# ------------------------------------------------------------------------------------------------ the schedule
def schedule(arch, filters, with_hed, with_vgg, precision):
    return Contract(arch, filters, with_hed, with_vgg, precision).schedule


def _E(stage, entry, kind, ops, flags=None, **meta):
    return dict(stage=stage, entry=entry, kind=kind, ops=tuple(ops), flags=flags, **meta)


def _conv_fwd(c, conv, pre=""):
    n, lv = conv.net, (conv.out.level, conv.x.level)
    flags = (CEPI_RESID if conv.resid is not None else 0) | (CEPI_CIN4 if conv.cin4 else 0)
    return _E(pre + conv.key, c.sym("vlg_conv3x3_fwd"), "conv_fwd",
              (conv.x.name, conv.wname, conv.bname, conv.out.name, conv.resid.name if conv.resid is not None else None,
               "%s.mask[%d]" % (n, lv[0]), conv.sname, "%s.rowtab[%d]" % (n, lv[1]) if conv.stride == 2 else None, "*"),
              flags, conv=conv)


def _conv_dgrad(c, conv, accum, with_da=True):
    n = conv.net
    flags = (CEPI_ACCUM if accum else 0) | (CEPI_DPRELU if conv.slope else 0)
    return _E(conv.key + " dgrad", c.sym("vlg_conv3x3_dgrad"), "conv_dgrad",
              ("d." + conv.out.name, conv.wname, "d." + conv.x.name, conv.x.name, "%s.mask[%d]" % (n, conv.x.level), conv.sname,
               "da:" + conv.key if conv.slope and with_da else None, "%s.taps[%d]" % (n, conv.x.level) if conv.stride == 2 else None,
               "*"), flags, conv=conv, with_da=bool(conv.slope and with_da))


def _trunk_features(c, t, src, tag):
    out = [_E("%s input (%s)" % (t.net, tag), "vlg_nchw_to_padded", "to_padded", (src, t.x.name), ten=t.x, C=3)]
    for op in t.ops:
        if op[0] == "pool":
            out.append(_E("%s (%s)" % (op[2].name, tag), "vlg_maxpool2x2", "pool_fwd", (op[1].name, op[2].name), src=op[1], dst=op[2]))
        else:
            out.append(_conv_fwd(c, op[1], "(%s) " % tag))
    return out


def _schedule(c):
    S = []
    # ---- HED edges of frame1, frame2 under no-grad (image_engine.py: fused map = output [5])
    if c.with_hed:
        h = c.hed
        for k, frame in ((1, "frame1"), (2, "frame2")):
            tag = "e%d" % k
            S.append(_E("hed affine (%s)" % tag, "vlg_affine_nchw", "affine",
                        ("batch:" + frame, "hed.pre", const([m / 255.0 for m in BGR_MEAN]), const([255.0] * 3)),
                        shift=[m / 255.0 for m in BGR_MEAN], scale=[255.0] * 3, C=3))
            S += _trunk_features(c, h, "hed.pre", tag)
            for i, (name, f) in enumerate(zip(HS.SCORES, h.feats)):
                S.append(_E("hed %s (%s)" % (name, tag), "vlg_score1x1_relu", "score",
                            (f.name, "hed.p:%s.weight" % name, "hed.p:%s.bias" % name, "hed.score[%d]" % i), ten=f, score=name, level=i))
            S.append(_E("hed head (%s)" % tag, "vlg_hed_head", "hed_head",
                        tuple("hed.score[%d]" % i for i in range(5)) + ("hed.p:moduleCombine.0.weight", "hed.p:moduleCombine.0.bias",
                                                                        "hed.out[%d]" % k), out="hed.out[%d]" % k))
    # ---- the input, the grid, the output affine
    edges = ("hed.out[1][5]", "hed.out[2][5]") if c.with_hed else ("batch:e1", "batch:e2")
    S.append(_E("prep_input", "vlg_prep_input", "prep_input",
                ("*" if c.with_hed else "batch:e1", "batch:seg1", "batch:frame1", "batch:frame2", "batch:seg2",
                 "*" if c.with_hed else "batch:e2", "batch:frame3", "batch:seg3", "x10", "f3", "seg3"), "*", edges=edges))
    S.append(_E("g input", "vlg_nchw_to_padded", "to_padded", ("x10", c.x.name), ten=c.x, C=c.x.C))
    for op in c.ops:
        if op[0] == "up":
            S.append(_E(op[2].name, "vlg_upsample2x_fwd", "up_fwd", (op[1].name, op[2].name), src=op[1], dst=op[2]))
        else:
            S.append(_conv_fwd(c, op[1]))
    S.append(_E("seg out", "vlg_padded_to_nchw", "to_nchw", (c.seg.name, "seg"), ten=c.seg))
    S.append(_E("img out", "vlg_padded_to_nchw", "to_nchw", (c.img.name, "img_raw"), ten=c.img))
    istd = [1.0 / s for s in OUT_STD]
    S.append(_E("img affine", "vlg_affine_nchw", "affine", ("img_raw", "img", const(OUT_MEAN), const(istd)),
                shift=OUT_MEAN, scale=istd, div=OUT_STD, C=3))
    # ---- losses: value and gradient in one pass, weights as grad_scale; dimg collects the image terms
    S.append(_E("l1", "vlg_l1_mean", "loss", ("img", "f3", "dimg", "losses[0]", "scratch"), loss="l1", weight=W_L1))
    S.append(_E("gradient loss", "vlg_gradient_loss", "loss", ("img", "f3", "dtmp", "losses[1]", "scratch"), loss="gd", weight=W_STYLE))
    S.append(_E("dimg += gradient loss", "vlg_add_rows", "add", ("dimg", "dtmp"), 1))
    S.append(_E("ssim", "vlg_ssim_loss", "loss", ("img", "f3", "dtmp", "losses[2]", "scratch"), loss="ssim", weight=W_STYLE))
    S.append(_E("dimg += ssim", "vlg_add_rows", "add", ("dimg", "dtmp"), 1))
    S.append(_E("ce", "vlg_ce_nchw", "loss", ("seg", "seg3", "dseg", "losses[3]", "scratch"), loss="ce", weight=W_CE))
    if c.with_vgg:
        v = c.vgg
        S += _trunk_features(c, v, "f3", "target")
        tgt = Ten("vgg:feat_tgt", v.feat.level, v.feat.C)
        S.append(_E("vgg keep target", "vlg_add_rows", "add_rows_padded", (tgt.name, v.feat.name), 0, src=v.feat, dst=tgt))
        S += _trunk_features(c, v, "img", "output")
        S.append(_E("vgg l1", "vlg_l1_relu_padded", "l1_relu", (v.feat.name, tgt.name, "d." + v.feat.name, "vgg.loss", "vgg.scratch"),
                    a=v.feat, b=tgt, weight=W_STYLE))
        for op in reversed(v.ops):
            if op[0] == "pool":
                S.append(_E(op[2].name + " bwd", "vlg_maxpool2x2_bwd", "pool_bwd", (op[1].name, "d." + op[2].name, "d." + op[1].name),
                            src=op[1], dst=op[2]))
            else:
                S.append(_conv_dgrad(c, op[1], False, with_da=False))
        S.append(_E("vgg dimg", "vlg_padded_to_nchw", "to_nchw", ("d." + v.x.name, "vgg.dimg"), ten=v.x.grad(), C=3))
        S.append(_E("dimg += vgg", "vlg_add_rows", "add", ("dimg", "vgg.dimg"), 1))
    # ---- backward: d/d img_raw, the two head gradients, the grid last to first
    S.append(_E("d img affine", "vlg_affine_nchw", "affine", ("dimg", "dtmp", const([0.0] * 3), const(istd)),
                shift=[0.0] * 3, scale=istd, div=OUT_STD, C=3))
    written = set()
    for t, src in ((c.seg, "dseg"), (c.img, "dtmp")):
        S.append(_E("d." + t.name + " seed", "vlg_nchw_to_padded", "to_padded", (src, "d." + t.name), ten=t.grad(), C=t.C))
        written.add(t.name)
    for op in reversed(c.ops):
        if op[0] == "up":
            _, src, dst = op
            S.append(_E(dst.name + " bwd", "vlg_upsample2x_bwd", "up_bwd", ("d." + dst.name, "d." + src.name),
                        1 if src.name in written else 0, src=src, dst=dst))
            written.add(src.name)
            continue
        conv = op[1]
        assert conv.out.name in written, "no gradient reaches " + conv.key
        S.append(_E(conv.key + " wgrad", c.sym("vlg_conv3x3_wgrad"), "conv_wgrad",
                    ("d." + conv.out.name, conv.x.name, "slab:" + conv.key, "g.rowtab[%d]" % conv.x.level if conv.stride == 2 else None,
                     conv.sname), None, conv=conv))
        if conv.x is not c.x or conv.slope:
            S.append(_conv_dgrad(c, conv, conv.x.name in written))
            written.add(conv.x.name)
        if conv.resid is not None:
            S.append(_E(conv.key + " resid", "vlg_add_rows", "add_rows_padded", ("d." + conv.resid.name, "d." + conv.out.name),
                        1 if conv.resid.name in written else 0, src=conv.out.grad(), dst=conv.resid.grad()))
            written.add(conv.resid.name)
    S.append(_E("reduce slabs", "vlg_reduce_slabs_table", "reduce_slabs", ("g.reduce_table",)))
    S.append(_E("sum slope partials", "vlg_sum_partials_table", "sum_partials", ("g.da_table",)))
    return S


# ------------------------------------------------------------------------------------------------ stage functions
def conv_parts(x, w, bias, slope, act, stride, resid, r, rounded, dt=F64, pure=False):
    """(y, dx, da, da_scale, dW, db) of one convolution and of sum(y * r).  float64: test_hip_conv_bf16._ref itself.  Other
    dtypes (float32 = torch-CPU's own error; pure=True = no fp32 activation, for the fp64 chain that is held to the oracle) restate
    it with that dtype's arithmetic."""
    if dt == F64 and not pure:
        return CB._ref(x, w, bias, slope, act, stride, resid, r, rounded)
    xt = x.to(dt)
    xa = xt if slope is None else torch.cat([F.prelu(xt[:, :act], torch.tensor([slope], dtype=dt)), xt[:, act:]], dim=1)
    q = (lambda t: t.float().to(torch.bfloat16).to(dt)) if rounded else (lambda t: t.to(dt))
    xq, wq, rq = q(xa), q(w), q(r)
    y = F.conv2d(xq, wq, bias.to(dt), stride=stride, padding=1)
    if resid is not None:
        y = y + resid.to(dt)
    dxa = torch.nn.grad.conv2d_input(tuple(x.shape), wq, rq, stride=stride, padding=1)
    dx = dxa.clone()
    dx[:, act:] = 0
    da = da_scale = None
    if slope is not None:
        xd = xt[:, :act]
        neg = ~(xd > 0)
        dx[:, :act] = torch.where(neg, dxa[:, :act] * slope, dxa[:, :act])
        terms = dxa[:, :act] * xd
        da, da_scale = terms[neg].sum(), float(terms.abs()[neg].sum())
    dw = torch.nn.grad.conv2d_weight(xq, tuple(w.shape), rq, stride=stride, padding=1)
    return y, dx, da, da_scale, dw, r.to(dt).sum((0, 2, 3))


def prep_input(b, flip, dt=F64):
    """trainer.py:193-206 as oracle/image_step_spec.step_losses writes it -> (x10, f3, seg3)"""
    mean, std = torch.tensor(IMG_MEAN)[None, :, None, None], torch.tensor(IMG_STD)[None, :, None, None]
    f1, f2, f3 = ((b[k].to(dt) - mean) / std for k in ("frame1", "frame2", "frame3"))
    x = torch.cat([b["e1"].to(dt), b["seg1"].to(dt), f1, f2, b["seg2"].to(dt), b["e2"].to(dt)], dim=1)
    seg3 = b["seg3"]
    if flip:
        x, f3, seg3 = torch.flip(x, [3]), torch.flip(f3, [3]), torch.flip(seg3, [2])
    return x.contiguous(), f3.contiguous(), seg3.contiguous()


def affine(x, shift, scale, dt=F64, div=None):
    """(x - shift[c]) * scale[c] with the launch's fp32 constants; div (pure fp64 chain only): (x - shift) / div, the
    oracle's own expression"""
    C = x.shape[1]
    sh = torch.tensor(list(shift), dtype=F32).view(1, C, *([1] * (x.dim() - 2)))
    if div is not None:
        return (x.to(dt) - sh) / torch.tensor(list(div), dtype=F32).view_as(sh)
    return (x.to(dt) - sh.to(dt)) * torch.tensor(list(scale), dtype=F32).view_as(sh).to(dt)


def image_loss(kind, a, b, weight, dt=F64):
    """value and d(weight * value)/da of one of the four losses (trainer.py:248-250, loss.py:20-25, 68-91)"""
    x = a.to(dt).clone().requires_grad_(True)
    if kind == "l1":
        v = F.l1_loss(x, b.to(dt))
    elif kind == "gd":
        v = IS.gradient_loss(x, b.to(dt))
    elif kind == "ssim":
        v = IS.ssim_loss(x, b.to(dt))
    else:
        v = F.cross_entropy(x, b)
    (weight * v).backward()
    return v.detach(), x.grad


def image_loss_c(kind, a, b):
    """the plain-C oracle on the same fp32 inputs (what the kernels' own tests compare with): (value, gradient at scale 1)"""
    from oracle import image_ref as R
    fn = {"l1": R.l1_mean, "gd": R.gradient_loss, "ssim": R.ssim_loss, "ce": R.ce_nchw}[kind]
    v, g = fn(a.numpy(), b.numpy())
    return float(v), torch.from_numpy(g)


def hed_scores(ten, feat, w, bias, dt=F64):
    """relu(x) . w + b over the C real lanes -> (value, sum |terms| + |b|)"""
    terms = F.relu(feat.to(dt)) * w.to(dt).view(1, -1, 1, 1)
    return terms.sum(1) + bias.to(dt), terms.abs().sum(1) + bias.to(dt).abs()


def run(e, c, sh, get, dt=F64, rounded=False, pure=False, flip=0):
    """The stage function of launch e on its named inputs (get(name) -> the buffer as the launch found it) -> logical outputs:
    padded tensors as (b, C, H, W), NCHW buffers as they are, conv_wgrad as {"dw", "db"}, conv_dgrad also {"da", "da_scale"}."""
    k = e["kind"]
    if k in ("reduce_slabs", "sum_partials"):         # sums of the arena's regions: emulate / image_trace.check do them in place
        return {}
    if k == "to_padded":
        return {"y": get(e["ops"][0]).to(dt)[:, :e["C"]]}
    if k == "to_nchw":
        t = e["ten"]
        return {"y": t.nchw(get(e["ops"][0]), sh, e.get("C", t.C)).to(dt)}
    if k in ("conv_fwd", "conv_dgrad", "conv_wgrad"):
        conv = e["conv"]
        net = c.nets[conv.net]
        w, bias, slope = conv_params(net, get(conv.net + ".params"), conv)
        x = conv.x.nchw(get(conv.x.name), sh)
        go = sh.geo(conv.out.level)
        if k == "conv_fwd":
            r = torch.zeros(go.b, conv.cout, go.H, go.W)
            resid = None if conv.resid is None else conv.resid.nchw(get(conv.resid.name), sh, conv.cout)
        else:
            r = conv.out.grad().nchw(get("d." + conv.out.name), sh, conv.cout)
            resid = None
        y, dx, da, da_scale, dw, db = conv_parts(x, w, bias, slope, conv.act, conv.stride, resid, r, rounded, dt, pure)
        if k == "conv_fwd":
            return {"y": y}
        if k == "conv_wgrad":
            return {"dw": dw, "db": db}
        if e["flags"] & CEPI_ACCUM:
            dx = dx + conv.x.grad().nchw(get("d." + conv.x.name), sh).to(dt)
        return {"dx": dx, "da": da, "da_scale": da_scale}
    if k == "up_fwd":
        return {"y": PX._up(e["src"].nchw(get(e["src"].name), sh, e["src"].cp).to(dt))}
    if k == "up_bwd":
        src, dst = e["src"], e["dst"]
        g = dst.grad().nchw(get("d." + dst.name), sh, dst.cp)
        gs = sh.geo(src.level)
        dx = PX._up_t(g.double(), gs.H, gs.W) if dt == F64 else _up_t32(g, gs.H, gs.W)
        if e["flags"]:
            dx = dx + src.grad().nchw(get("d." + src.name), sh, src.cp).to(dt)
        return {"dx": dx}
    if k == "add_rows_padded":
        src, dst = e["src"], e["dst"]
        y = src.nchw(get(src.name), sh, src.cp)
        return {"y": (dst.nchw(get(dst.name), sh, dst.cp) + y if e["flags"] else y).to(dt)}
    if k == "add":
        dst, src = get(e["ops"][0]), get(e["ops"][1])
        return {"y": (dst + src).to(dt)}
    if k == "affine":
        return {"y": affine(get(e["ops"][0]), e["shift"], e["scale"], dt, e.get("div") if pure else None)}
    if k == "prep_input":
        b = {key: get("batch:" + key) for key in BATCH_KEYS if key not in ("e1", "e2")}
        for key, name in zip(("e1", "e2"), e["edges"]):
            b[key] = get(name[:-3])[5].unsqueeze(1) if name.endswith("[5]") else get(name)
        x, f3, seg3 = prep_input(b, flip, dt)
        return {"x10": x, "f3": f3, "seg3": seg3}
    if k == "loss":
        v, g = image_loss(e["loss"], get(e["ops"][0]), get(e["ops"][1]), e["weight"], dt)
        return {"value": v, "grad": g}
    if k == "pool_fwd":
        return {"y": F.max_pool2d(e["src"].nchw(get(e["src"].name), sh, e["src"].cp).to(dt), 2)}
    if k == "pool_bwd":
        src, dst = e["src"], e["dst"]
        _, dx = PX._pool_ref(src.nchw(get(src.name), sh, src.cp), dst.grad().nchw(get("d." + dst.name), sh, dst.cp))
        return {"dx": dx.to(dt)}
    if k == "score":
        t = e["ten"]
        p = get("hed.params")
        o = c.hed.off
        v, mag = hed_scores(t, t.nchw(get(t.name), sh, t.C), p[o["hed.p:%s.weight" % e["score"]]:][:t.C],
                            p[o["hed.p:%s.bias" % e["score"]]:][:1], dt)
        return {"y": v, "mag": mag}
    if k == "hed_head":
        p, o = get("hed.params"), c.hed.off
        s = [get("hed.score[%d]" % i) for i in range(5)]
        cw, cb = p[o["hed.p:moduleCombine.0.weight"]:][:5], p[o["hed.p:moduleCombine.0.bias"]:][:1]
        if dt == F64:
            y, up_abs = PX._hed_ref(s, cw, cb, sh.H, sh.W)
            return {"y": y, "up_abs": up_abs, "cw": cw, "cb": cb}
        up = [F.interpolate(t.unsqueeze(1), size=(sh.H, sh.W), mode="bilinear", align_corners=False).squeeze(1) for t in s]
        return {"y": torch.stack([torch.sigmoid(u) for u in up] + [torch.sigmoid(cb + sum(cw[i] * up[i] for i in range(5)))])}
    if k == "l1_relu":
        a, b = e["a"], e["b"]
        xa, xb = a.nchw(get(a.name), sh, a.C), b.nchw(get(b.name), sh, b.C)
        if dt == F64:
            v, g = PX._l1_relu_ref(xa, xb, e["weight"])
        else:
            x = xa.clone().requires_grad_(True)
            v = F.l1_loss(F.relu(x), F.relu(xb), reduction="sum") / xa.numel()
            (e["weight"] * v).backward()
            v, g = v.detach(), x.grad
        return {"value": v, "grad": g}
    raise KeyError(k)


def adam_step(p, g, m, v, step, lr, beta1, beta2, eps, dt=F64):
    """torch.optim.Adam's update (reference src/trainer.py:83,258) of the flat buffers -> (p, m, v)"""
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    return p - (lr / (1 - beta1 ** step)) * m / (v.sqrt() / math.sqrt(1 - beta2 ** step) + eps), m, v


def _up_t32(g, h, w):
    x = torch.zeros(g.shape[0], g.shape[1], h, w, dtype=g.dtype, requires_grad=True)
    PX._up(x).backward(g)
    return x.grad


# ------------------------------------------------------------------------------------------------ the emulated trace
def coords(ten, sh, dt=F32):
    """the two AddCoords lanes as vlg_fill_coords leaves them (oracle/gridnet_spec.add_coords)"""
    g = sh.geo(ten.level)
    return GS.add_coords(torch.zeros(g.b, 0, g.H, g.W))[:, -2:].to(dt)


def initial_state(c, sh, params, batch, dt=F32, trunk_params=None):
    """name -> buffer before the step: zero padded tensors (AddCoords lanes filled), flat parameters, the batch"""
    cur = {}
    for t in c.tens.values():
        flat = torch.zeros(t.numel(sh), dtype=dt)
        if t.coord:
            t.grid(flat, sh)[:, 1:-1, 1:-1, t.C:t.C + 2] = coords(t, sh, dt).permute(0, 2, 3, 1)
        cur[t.name] = flat
    cur["g.params"] = c.pack_params(params, dt)
    for net, sd in (trunk_params or {}).items():
        cur[net + ".params"] = c.nets[net].pack_params(sd, dt)
    for k, v in batch.items():
        cur["batch:" + k] = v.to(dt) if v.is_floating_point() else v
    return cur


def emulate(c, sh, params, batch, dt=F32, mutate=None, flip=0, pure=False, trunk_params=None):
    """The stage functions chained in dtype dt under contract c -> (records, state) in image_trace.trace's format.
    mutate(e, cur, out, rec) may change the buffers a launch wrote (out: name -> buffer), its record, or - silently, as a stray
    write would - the memory cur (name -> buffer) itself; everything after is computed from what it left.  Slabs: one per image of the batch (what a weight-gradient launch's row ranges are to the checker)."""
    cur = initial_state(c, sh, params, batch, dt, trunk_params)
    init = {k: v.clone() for k, v in cur.items()}
    slab_off, da_off, off, doff = {}, {}, 0, 0
    for conv in c.convs:
        slab_off[conv.key], da_off[conv.key] = off, doff
        off += sh.b * conv.slab_stride
        doff += 4 if conv.slope else 0
    cur["grads_ext"] = torch.zeros(c.n_params_padded + 8, dtype=dt)
    records = []

    def get(n):
        return cur[n]

    def zeros_like_ten(t):
        return cur[t.name] if t.name in cur else torch.zeros(t.numel(sh), dtype=dt)

    for e in c.schedule:
        k, ops = e["kind"], e["ops"]
        rounded = c.bf16 and k.startswith("conv_")
        o = run(e, c, sh, get, dt, rounded, pure, flip)
        out = {}
        if k == "to_padded":
            t = e["ten"]
            out[t.name] = t.pack(o["y"], sh, zeros_like_ten(t))
        elif k in ("to_nchw", "add", "affine"):
            out[ops[0] if k == "add" else ops[1]] = o["y"]
        elif k in ("conv_fwd", "up_fwd", "pool_fwd"):
            t = e["conv"].out if k == "conv_fwd" else e["dst"]
            out[t.name] = t.pack(o["y"], sh, zeros_like_ten(t))
        elif k in ("up_bwd", "pool_bwd"):
            t = e["src"].grad()
            out[t.name] = t.pack(o["dx"], sh)
        elif k == "add_rows_padded":
            out[e["dst"].name] = e["dst"].pack(o["y"], sh)
        elif k == "conv_dgrad":
            conv = e["conv"]
            t = conv.x.grad()
            out[t.name] = t.pack(o["dx"], sh)
            if e["with_da"]:
                part = torch.zeros(4, dtype=dt)
                part[0] = o["da"]
                out["da:" + conv.key] = part
        elif k == "conv_wgrad":
            conv = e["conv"]
            per = []
            for i in range(sh.b):           # one slab per image: the same launch on that image alone
                sub = Shape(1, sh.H, sh.W)
                one = lambda n, i=i: _image(c, sh, n, cur[n], i)
                oi = run(e, c, sub, one, dt, rounded, pure, flip)
                per.append(pack_slab(conv, oi["dw"], oi["db"]))
            out["slab:" + conv.key] = torch.cat(per)
        elif k == "prep_input":
            out["x10"], out["f3"], out["seg3"] = o["x10"], o["f3"], o["seg3"]
        elif k == "loss":
            out[ops[2]], out[ops[3]] = o["grad"], o["value"].reshape(1).to(dt)
        elif k == "l1_relu":
            t = e["a"].grad()
            out[t.name], out["vgg.loss"] = t.pack(o["grad"], sh), o["value"].reshape(1).to(dt)
        elif k == "score":
            out[ops[3]] = o["y"]
        elif k == "hed_head":
            out[e["out"]] = o["y"]
        elif k == "reduce_slabs":
            g = cur["grads_ext"].clone()
            for conv in c.convs:
                v = cur["slab:" + conv.key].view(sh.b, conv.slab_stride).sum(0)
                g[c.off[conv.wname]:c.off[conv.wname] + conv.slab_stride] = v
            out["grads_ext"] = g
        elif k == "sum_partials":
            g = cur["grads_ext"].clone()
            for conv in c.convs:
                if conv.slope:
                    g[c.off[conv.sname]] = cur["da:" + conv.key].sum()
            out["grads_ext"] = g
        else:
            raise KeyError(k)
        rec = dict(name=e["entry"], flags=e["flags"], ops=e["ops"], out=out)
        if k == "prep_input":
            rec["flags"] = flip
        elif k == "conv_wgrad":
            rec["region"] = (slab_off[e["conv"].key], sh.b, e["conv"].slab_stride)
        elif k == "reduce_slabs":
            rec["arena"] = {"slab:" + conv.key: cur["slab:" + conv.key] for conv in c.convs}
        elif k == "sum_partials":
            rec["arena"] = {"da:" + conv.key: cur["da:" + conv.key] for conv in c.convs if conv.slope}
        if mutate is not None:
            mutate(e, cur, out, rec)
        for n, v in out.items():
            if n.startswith("losses["):
                cur["grads_ext"] = cur["grads_ext"].clone()
                cur["grads_ext"][c.n_params_padded + int(n[7])] = v[0]
            cur[n] = v
        if k == "l1_relu":
            cur["grads_ext"] = cur["grads_ext"].clone()
            cur["grads_ext"][c.n_params_padded + 4] = cur["vgg.loss"][0]
        records.append(rec)
    return records, dict(init=init, final=cur, flip=flip)


def _image(c, sh, name, buf, i):
    """image i of the batch out of a named buffer (padded tensors keep their guard rows; flat parameters pass through)"""
    t = c.tens.get(name[2:] if name.startswith("d.") else name)
    if t is None:
        return buf
    if name.startswith("d."):
        t = t.grad()
    return t.pack(t.nchw(buf, sh, t.cp)[i:i + 1], Shape(1, sh.H, sh.W))
