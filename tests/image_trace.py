"""Trace one ImageEngine.forward + backward launch by launch, and check every launch against fp64 evaluated on the values that
launch read (the stage functions of image_stages.py).  Plain module: test infrastructure, nothing collected.

trace(engine, batch, flip)  installs a recorder as vlg.hip.tracer - every launch of the pixel step goes through vlg.hip.call - for
    one forward + backward and restores the previous value.  The context manager it hands out synchronises on exit and records the
    entry point, the flags word, the NAME of the buffer behind every pointer argument, and CPU clones of what the launch wrote: a
    padded tensor whole (guard rows included), a weight-gradient launch its n_slabs x slab_stride region.  Two names on one
    pointer is an assertion failure.  Buffers the step allocates on the way (seg, img_raw, the HED maps, the VGG term's dimg) are
    named after the run from the tensors the three nets returned; they are written once.
check(records, engine_state, contract, batch)  walks image_stages' schedule next to the records.  Per launch:
    contract    entry point, flags word and every operand name; a failure reads "[<stage>] ..."
    values      fp32 convolutions   helpers.vs_cpu32 against fp64 on the launch's own inputs (4 x torch-CPU fp32's own error +
                                    the 2^-20 floor) for y, dx, dW, db; the slope gradient, ONE number, the same
                                    on its natural scale: 4 x torch-CPU fp32's error + 2^-20 of da_scale = sum |terms| (the scale
                                    test_hip_conv_bf16 uses), and never more than the 1e-5 of da_scale the bf16 kernel is held to
                bf16 convolutions   test_hip_conv_bf16's TOL = 1e-5 of scale against fp64 on the bf16-rounded operands (the slope
                                    gradient on its da_scale), and DISCRIMINATE = 10 x further from the unrounded result - asserted
                                    where the two references themselves differ by >= 100 x TOL, so it cannot fail for lack of signal
                                    (y, dx, dW and the slope gradient; db is summed from the fp32 dOut, so no rounding shows in
                                    it; the sum behind the slope gradient averages the rounding out, so its condition is rarely
                                    met and test_hip_conv_bf16 itself only prints that figure)
                bitwise             layout kernels, add_rows, the max-pool and its gradient, the affine maps
                derived EPS bounds  test_hip_pixel_ops': upsample, score1x1, HED head, L1-of-ReLU, sum_partials
                image losses        test_hip_image_ops.test_losses_match_c_oracle's bars against oracle/image_ref.py
                weight gradients    fp64 sum of the slab snapshot against fp64 dW | db; the reduced grads range against the fp64
                                    sum of those slabs at test_reduce_slabs' 1e-5
    arena       when a table reduction runs, every region is bitwise the snapshot taken after its own launch; regions are disjoint
    invariants  of every padded tensor a launch wrote, exact: guard and halo rows 0.0, lanes at or beyond the tensor's channels
                0.0, AddCoords lanes bitwise what vlg_fill_coords left (and that within 2 EPS of the formula)
    After backward every padded lane of net.grads is exactly 0.0 and the 8 floats behind them are the loss parts and zeros.
No bar here is new and none is read off a GPU result."""
import ctypes

import torch

import image_stages as IS
import test_hip_conv_bf16 as CB
import test_hip_pixel_ops as PX
from helpers import check_close, vs_cpu32

F32, F64 = torch.float32, torch.float64
EPS = PX.EPS
# the header's name of the argument a record keeps as its flags (its position: vlg.hip.param_index)
_FLAGS_PARAM = {"vlg_conv3x3_fwd": "epilogue", "vlg_conv3x3_dgrad": "epilogue", "vlg_upsample2x_bwd": "accumulate",
                "vlg_add_rows": "accumulate", "vlg_prep_input": "flip"}
_WRITES = {"vlg_nchw_to_padded": (1,), "vlg_padded_to_nchw": (1,), "vlg_conv3x3_fwd": (3,), "vlg_conv3x3_dgrad": (2, 6),
           "vlg_conv3x3_wgrad": (2,), "vlg_upsample2x_fwd": (1,), "vlg_upsample2x_bwd": (1,), "vlg_add_rows": (0,),
           "vlg_maxpool2x2": (1,), "vlg_maxpool2x2_bwd": (2,), "vlg_score1x1_relu": (3,), "vlg_hed_head": (7,),
           "vlg_l1_relu_padded": (2, 3), "vlg_l1_mean": (2, 3), "vlg_gradient_loss": (2, 3), "vlg_ssim_loss": (2, 3),
           "vlg_ce_nchw": (2, 3), "vlg_affine_nchw": (1,), "vlg_prep_input": (8, 9, 10), "vlg_reduce_slabs_table": (),
           "vlg_sum_partials_table": ()}


def _base(name):
    return name[:-5] if name.endswith("_bf16") else name


class _Names:
    """pointer -> name and name -> the device tensor to snapshot, for everything a launch of this engine can point at"""

    def __init__(self, engine, batch):
        self.by_ptr, self.snap = {}, {}
        net = engine.net
        self._pts("g", net.x, [(op.key, op.out) for op in net.tape if not isinstance(op, tuple)])
        for op in net.tape:
            if isinstance(op, tuple):
                user = [o for o in net.tape if not isinstance(o, tuple) and o.x is op[2]]
                assert len(user) == 1 and user[0].key.endswith(".up.2")
                self._pt("g:%s.up.0" % user[0].key[:-5], op[2])
        for l, g in enumerate(net.geo):
            self._geo("g", l, g)
        for op in net.tape:
            if isinstance(op, tuple):
                continue
            self.add(net.params.data_ptr() + 4 * op.w_off, "g.p:%s.weight" % op.key)
            self.add(net.params.data_ptr() + 4 * op.b_off, "g.p:%s.bias" % op.key)
            self.add(net.slabs.data_ptr() + 4 * op.slab_off, "slab:" + op.key, net.slabs[op.slab_off:op.slab_off + op.n_slabs * op.slab_stride])
            if op.prelu:
                self.add(net.da_part.data_ptr() + 4 * op.da_off, "da:" + op.key, net.da_part[op.da_off:op.da_off + op.da_n])
        for k, off in net.p_off.items():
            self.add(net.params.data_ptr() + 4 * off, "g.p:" + k)
        self.add(net.reduce_table.data_ptr(), "g.reduce_table")
        if net.da_table is not None:
            self.add(net.da_table.data_ptr(), "g.da_table")
        if net.ws is not None:
            self.add(net.ws.data_ptr(), "g.ws")
        self.snap["g.params"] = net.params
        n = net.n_params_padded
        for k in range(net.TAIL_EXTRA):
            self.add(net.grads_ext.data_ptr() + 4 * (n + k), "losses[%d]" % k, net.grads_ext[n + k:n + k + 1])
        for name in ("x10", "f3", "seg3", "img", "dimg", "dtmp", "dseg", "scratch"):
            self.add(getattr(engine, name).data_ptr(), name, getattr(engine, name))
        for k, t in batch.items():
            self.add(t.data_ptr(), "batch:" + k, t)
        hed, vgg = engine.hed, engine.vgg
        if hed is not None:
            self._pts("hed", hed.x, [(c[0], c[2]) for c in hed.convs])
            for si, (_, pooled) in hed.pools.items():
                self._pt("hed:pool%d" % si, pooled)
            self._trunk("hed", hed)
            self.add(hed.pre.data_ptr(), "hed.pre", hed.pre)
            for k, t in enumerate(hed.score):
                self.add(t.data_ptr(), "hed.score[%d]" % k, t)
        if vgg is not None:
            self._pts("vgg", vgg.x, [(op[1], op[3]) for op in vgg.ops if op[0] == "conv"])
            for i, op in enumerate([op for op in vgg.ops if op[0] == "pool"]):
                self._pt("vgg:pool%d" % (i + 1), op[2])
            self._pt("vgg:feat_tgt", vgg.feat_tgt)
            self._trunk("vgg", vgg)
            self.add(vgg.loss.data_ptr(), "vgg.loss", vgg.loss)
            self.add(vgg.scratch.data_ptr(), "vgg.scratch")

    def add(self, p, name, tensor=None):
        assert p not in self.by_ptr, "two names on one pointer: %s and %s" % (self.by_ptr[p], name)
        assert name not in self.snap, "two buffers named " + name
        self.by_ptr[p] = name
        if tensor is not None:
            self.snap[name] = tensor

    def _pt(self, name, t):
        self.add(t.ptr, name, t.buf)
        if t.grad is not None:
            self.add(t.grad.ptr, "d." + name, t.grad.buf)

    def _pts(self, net, x, outs):
        self._pt(net + ":x", x)
        for key, t in outs:
            self._pt("%s:%s" % (net, key), t)

    def _geo(self, net, l, g):
        self.add(g.mask.data_ptr(), "%s.mask[%d]" % (net, l))
        if g.down_rowtab is not None:
            self.add(g.down_rowtab.data_ptr(), "%s.rowtab[%d]" % (net, l))
            self.add(g.down_taptabs.data_ptr(), "%s.taps[%d]" % (net, l))

    def _trunk(self, net, t):
        for l, g in enumerate(t.geo):
            self._geo(net, l, g)
        for k, off in t.off.items():
            self.add(t.params.data_ptr() + 4 * off, "%s.p:%s" % (net, k))
        if t.ws is not None:
            self.add(t.ws.data_ptr(), net + ".ws")
        self.snap[net + ".params"] = t.params


def trace(engine, batch, flip):
    """engine.forward(batch, flip) + engine.backward() under the recorder -> (records, engine_state); engine_state holds every
    named buffer before ("init") and after ("final") the step."""
    from vlg import hip
    names = _Names(engine, batch)
    clone = lambda t: t.detach().cpu().clone()
    init = {n: clone(t) for n, t in names.snap.items()}
    records, late = [], {}                 # late: pointer -> name of a buffer allocated during the step (named after it)
    net, kept = engine.net, []

    class Recorder:
        def __init__(self, name, args):
            self.name, self.args = name, args

        def __enter__(self):
            return self

        def __exit__(self, etype, *_):
            if etype is not None:
                return False
            torch.cuda.synchronize()
            name, args, base = self.name, self.args, _base(self.name)
            types = hip.SIGNATURES[name][1]
            ops, out = [], {}
            for i, (a, ty) in enumerate(list(zip(args, types))[:-1]):
                if ty is not ctypes.c_void_p:
                    continue
                if isinstance(a, ctypes.Array):
                    ops.append(IS.const(list(a)))
                    continue
                n = None if a == 0 else names.by_ptr.get(a, ("late", a))
                ops.append(n)
                if i in _WRITES[base] and n is not None:
                    out[n] = clone(names.snap[n]) if n in names.snap else None
            at = lambda param: args[hip.param_index(name, param)]
            rec = dict(name=name, flags=at(_FLAGS_PARAM[base]) if base in _FLAGS_PARAM else None, ops=ops, out=out)
            if base == "vlg_conv3x3_wgrad":
                rec["region"] = ((at("slabs") - net.slabs.data_ptr()) // 4, out[ops[2]].numel() // at("slab_stride"), at("slab_stride"))
            elif base == "vlg_reduce_slabs_table":
                out["grads_ext"] = clone(net.grads_ext)
                rec["arena"] = {n: clone(t) for n, t in names.snap.items() if n.startswith("slab:")}
            elif base == "vlg_sum_partials_table":
                out["grads_ext"] = clone(net.grads_ext)
                rec["arena"] = {n: clone(t) for n, t in names.snap.items() if n.startswith("da:")}
            records.append(rec)
            return False

    def keep(obj, attr, label):
        fn = getattr(obj, attr)

        def wrapped(*a, **k):
            r = fn(*a, **k)
            kept.append((label, r))
            return r
        setattr(obj, attr, wrapped)                      # instance attribute: this engine only

    wrapped = [(engine.net, "forward", "net")]
    if engine.hed is not None:
        wrapped.append((engine.hed, "forward", "hed"))
    if engine.vgg is not None:
        wrapped.append((engine.vgg, "loss_and_grad", "vgg"))
    for w in wrapped:
        keep(*w)
    previous = hip.tracer
    hip.tracer = Recorder
    try:
        engine.forward(batch, flip)
        engine.backward()
        torch.cuda.synchronize()
    finally:
        hip.tracer = previous
        for obj, attr, _ in wrapped:
            delattr(obj, attr)
    fresh, n_hed = {}, 0
    for label, r in kept:
        if label == "net":
            fresh["seg"], fresh["img_raw"] = r
        elif label == "hed":
            n_hed += 1
            fresh["hed.out[%d]" % n_hed] = r
        else:
            fresh["vgg.dimg"] = r[1]
    # These buffers exist only once the step runs, so they are cloned here, after it, on the assumption that each is WRITTEN
    # ONCE: a stray second write would be attributed to the first launch.  Asserted below as far as the launches show it (each
    # is the output of exactly one recorded launch); a write outside vlg.hip.call would show as a value failure at its consumer.
    for n, t in fresh.items():
        assert t.data_ptr() not in names.by_ptr, "two names on one pointer: %s and %s" % (names.by_ptr[t.data_ptr()], n)
        late[t.data_ptr()] = n
    for rec in records:
        rec["ops"] = tuple("?" if isinstance(n, tuple) and n[1] not in late else late[n[1]] if isinstance(n, tuple) else n
                           for n in rec["ops"])
        for n in [n for n in rec["out"] if isinstance(n, tuple)]:
            rec["out"].pop(n)
            if n[1] in late:
                rec["out"][late[n[1]]] = clone(fresh[late[n[1]]])
    for n in fresh:
        writers = [rec["name"] for rec in records if n in rec["out"]]
        assert len(writers) == 1, "%s is written by %s: it is snapshotted once, after the step" % (n, writers or "no launch")
    final = {n: clone(t) for n, t in names.snap.items()}
    final["grads_ext"] = clone(net.grads_ext)
    return records, dict(init=init, final=final, flip=1 if flip else 0)


# ------------------------------------------------------------------------------------------------ the checker
def _all_tens(c):
    tens = {}
    for e in c.schedule:
        cands = [e.get(k) for k in ("ten", "src", "dst", "a", "b")]
        if "conv" in e:
            cands += [e["conv"].x, e["conv"].out, e["conv"].resid]
        for t in cands:
            if t is not None and not t.name.startswith("d."):
                tens[t.name] = t
    return tens


def invariants(t, buf, sh, init=None):
    """exact: guard rows, halo rows and the lanes at or beyond the tensor's channels are 0.0; AddCoords lanes are bitwise what
    vlg_fill_coords left (init) and that is within 2 EPS of the formula (test_hip_pixel_ops.test_layout_round_trip)"""
    g = sh.geo(t.level)
    assert buf.numel() == t.numel(sh), "%s holds %d floats, the contract's geometry %d" % (t.name, buf.numel(), t.numel(sh))
    n0, n1 = g.guard * t.cp, (g.guard + g.rows) * t.cp
    assert bool((buf[:n0] == 0).all()) and bool((buf[n1:] == 0).all()), "%s: guard rows are not 0.0" % t.name
    v = t.grid(buf, sh)
    for halo in (v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1]):
        assert bool((halo == 0).all()), "%s: halo rows are not 0.0" % t.name
    assert bool((v[..., t.cin:] == 0).all()), "%s: lanes >= %d are not 0.0" % (t.name, t.cin)
    if t.coord:
        lanes = v[:, 1:-1, 1:-1, t.C:t.C + 2]
        assert torch.equal(lanes, t.grid(init, sh)[:, 1:-1, 1:-1, t.C:t.C + 2]), "%s: AddCoords lanes changed" % t.name
        PX.within(lanes, IS.coords(t, sh, F64).permute(0, 2, 3, 1), 2 * EPS, t.name + " AddCoords lanes")


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


def _conv_values(c, e, sh, get, got, log):
    """got: key -> tensor for the keys of this launch (y | dx, da | dw, db)"""
    bf = c.bf16
    plain = IS.run(e, c, sh, get, F64, False)
    want = IS.run(e, c, sh, get, F64, True) if bf else plain
    cpu = IS.run(e, c, sh, get, F32, bf) if (log is not None or not bf) else None
    for key, g in got.items():
        what = "%s %s" % (e["kind"][5:], key)
        if key == "da":
            w, scale = float(want["da"]), max(want["da_scale"], 1e-12)
            if log is not None:
                log.append((e["stage"], what, abs(g - w), abs(float(cpu["da"]) - w)))
            assert g == g, "slope gradient not finite"
            if bf:
                err = abs(g - w) / scale
                assert err <= CB.TOL, "slope gradient %.9g, fp64 on rounded operands %.9g (scale %.3g)" % (g, w, scale)
                if abs(float(plain["da"]) - w) / scale >= 100 * CB.TOL:
                    e_plain = abs(g - float(plain["da"])) / scale
                    assert e_plain >= CB.DISCRIMINATE * max(err, 1e-9), "slope gradient: %.3e vs unrounded is not >> %.3e" % (e_plain, err)
            else:        # vs_cpu32 on the quantity's natural scale, and never looser than what the bf16 kernel is held to
                bar = min(4 * abs(float(cpu["da"]) - w) + 2.0 ** -20 * scale, CB.TOL * scale)
                assert abs(g - w) <= bar, "slope gradient %.9g, fp64 %.9g: |err| %.3e > %.3e (4 x torch-CPU fp32's %.3e + 2^-20 of scale %.3g)" % (
                    g, w, abs(g - w), bar, abs(float(cpu["da"]) - w), scale)
            continue
        if log is not None:
            log.append((e["stage"], what, _err(g, want[key]), _err(cpu[key], want[key])))
        bad = ~torch.isfinite(g)
        assert not bool(bad.any()), "%s: %d elements not finite" % (what, int(bad.sum()))
        if not bf:
            vs_cpu32(g, plain[key], cpu[key], what)
            continue
        err = CB._err(g, want[key])
        assert err <= CB.TOL, "%s: %.3e of scale against the bf16-operand reference (bar %.0e)" % (what, err, CB.TOL)
        if key != "db" and CB._err(plain[key], want[key]) >= 100 * CB.TOL:       # (db comes from the fp32 dOut: nothing to discriminate)
            e_plain = CB._err(g, plain[key])
            assert e_plain >= CB.DISCRIMINATE * max(err, 1e-9), "%s: %.3e vs unrounded is not >> %.3e: operands not rounded to bf16?" % (
                what, e_plain, err)


def _loss_values(e, get, value, grad, log):
    a, b, w = get(e["ops"][0]), get(e["ops"][1]), e["weight"]
    rv, rg = IS.image_loss_c(e["loss"], a, b)
    if log is not None:
        v64, g64 = IS.image_loss(e["loss"], a, b, w, F64)
        v32, g32 = IS.image_loss(e["loss"], a, b, w, F32)
        log.append((e["stage"], "loss value", abs(float(value) - float(v64)), abs(float(v32) - float(v64))))
        log.append((e["stage"], "loss grad", _err(grad, g64), _err(g32, g64)))
    assert abs(float(value) - rv) <= 1e-4 * max(abs(rv), 1e-6), "value %.9g, C oracle %.9g" % (float(value), rv)
    atol = 1e-9 if e["loss"] == "ce" else w * 2e-7 * max(1.0, 1e3 / a.numel())
    check_close(grad, w * rg.double(), rtol=1e-4, atol=atol, what="gradient")


def check(records, engine_state, c, batch, log=None):
    """See the module docstring.  `log`, a list, receives (stage, output, max |err| vs fp64, torch-CPU fp32's) per output."""
    b, _, H, W = batch["frame1"].shape
    sh = IS.Shape(b, H, W)
    sched = c.schedule
    assert [r["name"] for r in records] == [e["entry"] for e in sched], "the launches are not the contract's schedule: %s" % (
        [(e["stage"], r["name"], e["entry"]) for r, e in zip(records, sched) if r["name"] != e["entry"]][:3] or (len(records), len(sched)),)
    init, flip = engine_state["init"], engine_state["flip"]
    cur = dict(init)
    tens = _all_tens(c)
    regions, losses = {}, {}

    def ten_of(name):
        return tens[name[2:]].grad() if name.startswith("d.") else tens[name]

    for e, r in zip(sched, records):
        k, out = e["kind"], r["out"]
        get = cur.__getitem__
        try:
            assert e["flags"] == "*" or r["flags"] == e["flags"], "flags word %s, contract %s" % (r["flags"], e["flags"])
            assert len(r["ops"]) == len(e["ops"]) and all(w == "*" or g == w for g, w in zip(r["ops"], e["ops"])), \
                "operands %s, contract %s" % (r["ops"], e["ops"])
            if k == "prep_input":
                assert r["flags"] == flip, "flip %s, asked for %s" % (r["flags"], flip)
            for n, t in out.items():
                assert t is not None, "%s was written and no snapshot of it exists" % n
                if n in tens or (n.startswith("d.") and n[2:] in tens):
                    invariants(ten_of(n), t, sh, init.get(n))
            if k == "to_padded":
                t = e["ten"]
                assert torch.equal(t.nchw(out[t.name], sh, e["C"]), get(e["ops"][0])[:, :e["C"]]), "not bitwise the NCHW source"
            elif k == "to_nchw":
                t = e["ten"]
                assert torch.equal(out[e["ops"][1]], t.nchw(get(t.name), sh, e.get("C", t.C))), "not bitwise the padded source"
            elif k == "conv_fwd":
                t = e["conv"].out
                _conv_values(c, e, sh, get, {"y": t.nchw(out[t.name], sh, t.C)}, log)
            elif k == "conv_dgrad":
                conv = e["conv"]
                t = conv.x.grad()
                got = {"dx": t.nchw(out[t.name], sh)}
                assert ("da:" + conv.key in out) == e["with_da"]
                if e["with_da"]:
                    got["da"] = float(out["da:" + conv.key].double().sum())
                _conv_values(c, e, sh, get, got, log)
            elif k == "conv_wgrad":
                conv = e["conv"]
                off, n, stride = r["region"]
                assert stride == conv.slab_stride, "slab stride %d, contract %d" % (stride, conv.slab_stride)
                for other, (o2, n2, s2) in regions.items():
                    assert off + n * stride <= o2 or o2 + n2 * s2 <= off, "slab region overlaps that of %s" % other
                regions[conv.key] = r["region"]
                s64 = out["slab:" + conv.key].view(n, stride).double()
                pad = IS.pack_slab(conv, torch.ones(conv.cout, conv.cin, 3, 3), torch.ones(conv.cout)) == 0
                assert bool((s64[:, pad] == 0).all()), "a padded weight-gradient lane is not 0.0"
                dw, db = IS.unpack_slab(conv, s64.sum(0))
                _conv_values(c, e, sh, get, {"dw": dw, "db": db}, log)
            elif k in ("up_fwd", "up_bwd"):
                src, dst = e["src"], e["dst"]
                gs = sh.geo(src.level)
                kk = 2 * max(gs.H, gs.W)
                w64, w32 = IS.run(e, c, sh, get, F64), IS.run(e, c, sh, get, F32)
                if k == "up_fwd":        # test_hip_pixel_ops.test_upsample2x: (4k + 8) EPS max|x|
                    got, want, cpu = dst.nchw(out[dst.name], sh, dst.cp), w64["y"], w32["y"]
                    bar = (4 * kk + 8) * EPS * float(src.nchw(get(src.name), sh, src.cp).abs().max())
                else:                    # 16 (2k + 8) EPS max|g|; accumulate adds the prior contents with one rounding
                    got, want, cpu = src.grad().nchw(out["d." + src.name], sh, src.cp), w64["dx"], w32["dx"]
                    bar = 16 * (2 * kk + 8) * EPS * float(dst.grad().nchw(get("d." + dst.name), sh, dst.cp).abs().max())
                    if e["flags"]:
                        bar = bar + EPS * want.abs()
                if log is not None:
                    log.append((e["stage"], k, _err(got, want), _err(cpu, want)))
                PX.within(got, want, bar, k)
            elif k == "add_rows_padded":
                src, dst = e["src"], e["dst"]
                want = src.grid(get(src.name), sh)
                if e["flags"]:
                    want = dst.grid(get(dst.name), sh) + want
                assert torch.equal(dst.grid(out[dst.name], sh), want), "not bitwise %s" % ("prior + source" if e["flags"] else "the source")
            elif k == "add":
                assert torch.equal(out[e["ops"][0]], get(e["ops"][0]) + get(e["ops"][1])), "not bitwise prior + source"
            elif k == "affine":
                assert torch.equal(out[e["ops"][1]], IS.run(e, c, sh, get, F32)["y"]), "not bitwise (x - shift) * scale"
            elif k == "prep_input":
                want = IS.run(e, c, sh, get, F64, flip=flip)
                for n in ("x10", "f3"):
                    check_close(out[n], want[n], rtol=1e-6, atol=1e-6, what=n)
                assert torch.equal(out["seg3"], want["seg3"]), "seg3"
            elif k == "loss":
                losses[e["ops"][3]] = out[e["ops"][3]]
                _loss_values(e, get, out[e["ops"][3]][0], out[e["ops"][2]], log)
            elif k in ("pool_fwd", "pool_bwd"):
                src, dst = e["src"], e["dst"]
                want = IS.run(e, c, sh, get, F64)
                if k == "pool_fwd":
                    assert torch.equal(dst.nchw(out[dst.name], sh, dst.cp).double(), want["y"]), "max-pool value"
                else:
                    assert torch.equal(src.grad().nchw(out["d." + src.name], sh, src.cp).double(), want["dx"]), "max-pool gradient routing"
            elif k == "score":       # test_score1x1_relu: C + 2 roundings relative to sum |terms| + |b|
                want, cpu = IS.run(e, c, sh, get, F64), IS.run(e, c, sh, get, F32)
                got = out[e["ops"][3]]
                if log is not None:
                    log.append((e["stage"], k, _err(got, want["y"]), _err(cpu["y"], want["y"])))
                PX.within(got, want["y"], (e["ten"].C + 2) * EPS * want["mag"], "score1x1")
            elif k == "hed_head":    # test_hed_head's bars
                want, cpu = IS.run(e, c, sh, get, F64), IS.run(e, c, sh, get, F32)
                got, up_abs, cw, cb = out[e["out"]], want["up_abs"], want["cw"], want["cb"]
                if log is not None:
                    log.append((e["stage"], k, _err(got, want["y"]), _err(cpu["y"], want["y"])))
                for i in range(5):
                    PX.within(got[i], want["y"][i], 4e-7 + 0.25 * 6 * EPS * up_abs[i], "d%d" % (i + 1))
                arg = sum(abs(float(cw[i])) * up_abs[i] for i in range(5))
                PX.within(got[5], want["y"][5], 4e-7 + 0.25 * (6 * EPS * arg + 7 * EPS * (arg + abs(float(cb)))), "fuse")
            elif k == "l1_relu":     # test_l1_relu_padded's bars
                a = e["a"]
                want, cpu = IS.run(e, c, sh, get, F64), IS.run(e, c, sh, get, F32)
                v, g = out["vgg.loss"], a.grad().nchw(out["d." + a.name], sh, a.C)
                losses["losses[4]"] = v
                n4 = sh.geo(a.level).rows * a.cp // 4
                kk = -(-n4 // (min(4096, -(-n4 // 256)) * 256))
                if log is not None:
                    log.append((e["stage"], "value", _err(v, want["value"]), _err(cpu["value"], want["value"])))
                    log.append((e["stage"], "grad", _err(g, want["grad"]), _err(cpu["grad"], want["grad"])))
                PX.within(v, want["value"].view(1), (4 * kk + 40) * EPS * want["value"].abs(), "L1-of-ReLU value")
                PX.within(g, want["grad"], 2 * EPS * want["grad"].abs(), "L1-of-ReLU gradient")
            elif k in ("reduce_slabs", "sum_partials"):
                for n, t in r["arena"].items():
                    assert n in cur and torch.equal(t, cur[n]), "%s was overwritten after its own launch" % n
                g = out["grads_ext"]
                for conv in c.convs:
                    if k == "reduce_slabs":
                        o = c.off[conv.wname]
                        want = cur["slab:" + conv.key].view(-1, conv.slab_stride).double().sum(0)
                        check_close(g[o:o + conv.slab_stride], want, rtol=1e-5, atol=1e-5, what="grads of " + conv.key)
                    elif conv.slope:     # test_sum_partials: ceil(n / 256) serial adds + an 8-level tree, relative to sum |p|
                        p = cur["da:" + conv.key].double()
                        PX.within(g[c.off[conv.sname]].view(1), p.sum().view(1), (-(-p.numel() // 256) + 10) * EPS * p.abs().sum(),
                                  "slope gradient " + conv.slope)
            else:
                raise KeyError(k)
            cur.update(out)
        except AssertionError as err:
            raise AssertionError("[%s] %s" % (e["stage"], err)) from None
    # ---- after backward
    g = engine_state["final"]["grads_ext"]
    assert torch.equal(g, cur["grads_ext"]), "grads_ext changed after the last launch"
    n = c.n_params_padded
    assert g.numel() == n + 8, "grads_ext holds %d floats, the contract's layout %d + 8" % (g.numel(), n)
    bad = c.padded_lanes() & (g[:n] != 0)
    assert not bool(bad.any()), "%d padded lanes of the gradient are not 0.0 (first at %d)" % (int(bad.sum()), int(bad.nonzero()[0]))
    want = torch.zeros(8, dtype=g.dtype)
    for i in range(5):
        if "losses[%d]" % i in losses:
            want[i] = losses["losses[%d]" % i][0]
    assert torch.equal(g[n:], want), "the 8 floats behind the gradient are %s, the loss parts %s" % (g[n:].tolist(), want.tolist())
