"""Trace one forward_backward of a LayoutEngine launch by launch, and check every launch against fp64 evaluated on the
values that launch read (the stage functions of step_stages.py).  Plain module: test infrastructure, nothing collected.

trace(engine, batch)  replaces engine._timed - the single launch point - on that ONE instance by a wrapper that launches,
    synchronises and records the launch's family, entry point, flags word, the NAME of the engine buffer behind every
    pointer argument, and clones of the buffers the backward reuses (dx, dh, du, dqkv, dout, delta).  The state before a
    launch is the snapshot after the previous one; forward buffers persist and are read, with the gradients, at the end.
check(records, state, cfg, contract, batch)  walks step_stages.schedule next to the records.  Per launch: entry point,
    family, flags word and operand names are the contract's (a stale buffer, a master weight in place of its bf16
    shadow, a wrong epilogue or storage bit fail HERE, by name); every stored tensor has the contract's dtype; every
    output is within the project's per-kernel bars of fp64 on the launch's own inputs:
      computed outputs   helpers.vs_cpu32 - 4 x torch-CPU fp32's error against fp64 of the same stage function + the
                         2^-20 floor, a bf16 output one bf16 rounding more.  The bf16 per-clip attention rounds P and dS
                         on chip, as matrix operands: the few elements whose rounding fp64 cannot decide
                         (step_stages.flip_step, ~1 in 3 000) may round either way, and what they can move an output by
                         is taken off the GPU's and off torch-CPU fp32's error alike before that same comparison
      loss               test_hip_layout_ops._loss_check
      gathers and masks  bitwise: dout rows of padded slots are 0.0; so are the dqkv rows of padded slots (their dO is
                         exactly 0, so anything there would have come from ANOTHER query through a masked key)
      parameter gradients  test_hip_gemm_paths.check_wgrad's bar (1e-4 / 1e-5 after 1 / sqrt(M)), native fp32 dW also 4 x
                         torch-CPU fp32's error
    A failure is an AssertionError whose message starts with "[<stage>]".
Dropout (an engine built with dropout > 0, a Contract with dropout=(p, seed, k)): trace also clones per launch the three
    buffers a dropout step rewrites before it ends (ybranch, x[0] - overwritten in place by site 0 -, ddrop) and records the
    scalar arguments of the fused entry points and, after each synchronisation, the device counter.  check holds a fused launch
    to the above - names (a stale dx where ddrop belongs fails by name), the bars of the plain layer-norm stages on x_out, h,
    mean, rstd / dx, ddrop - and to: thr, scale, seed equal to dropout_ref.plan / the contract's seed, site the schedule's;
    the counter at k after every launch, k + 1 after the advance; the dropped set EXACTLY dropout_ref.keep_mask's
    (_dropped_set_fwd, _dropped_set_bwd: the rules of test_hip_dropout's kernel tests).
Options (step_stages' module docstring, "Options"; tests/test_hip_step_trace_options.py): trace names the engine's own batch
    buffers (mix_cls, mix_box, aug_*), class_weights, box_nll_scratch, the three step counters and lse by ROW; it records the
    scalar arguments of the loss_ext, box_nll, mix and augment launches and, after every launch, every counter that exists.
    A Gaussian-head step also snapshots loss_out per launch (the NLL launch adds to what the loss launch left).  A
    scheduled-sampling step snapshots, per launch, every buffer that launch names: pass 2 overwrites what pass 1 wrote.
    check holds each new launch to names, family, dtypes, shapes and to
      scalars    equal to the restatement's plan (sched_ref.thr_max, augment_ref.threshold, BOX_S_MIN / BOX_S_MAX,
                 box_nll_weight, label_smoothing, the GIoU flag, 64-bit seeds), floats as the C ABI's fp32
      counters   every counter at its own k after every launch before its advance, k + 1 after it
      augment    all four outputs bitwise augment_ref.augment's (test_hip_augment's rule); the caller's tensors unmodified
      sched mix  test_hip_sched_mix._check's rule on the `out` the launch read
      loss_ext   test_hip_layout_loss_ext.check with that file's floors; padded and dropped rows of dout exactly 0
      box_nll    boxhead_ref.check_nll; padding columns 0 and the loss launch's columns of dout bit for bit as they were;
                 loss_out[0] = the loss launch's total + w_nll * box_nll to test_hip_box_nll's 2^-23
      frame_*    what the clip kinds get: vs_cpu32 per dq / dk / dv, dqkv rows of padded slots 0, flip slack under bf16
Storage contract: DESIGN.md, "Layout step: storage contract of the reduced-precision modes"."""
import math

import torch

import boxhead_ref
import step_stages as SS
from helpers import check_close, vs_cpu32
from oracle import layout_spec as O

BF = torch.bfloat16
# the header's name of a GEMM call's flags word (its position: vlg.hip.param_index)
_FLAGS_PARAM = {"vlg_linear_fwd": "epilogue", "vlg_linear_dgrad": "epilogue", "vlg_linear_wgrad": "flags", "vlg_linear_dgrad_wgrad": "epilogue"}


def _buffers(engine, batch, M):
    """name -> device tensor of everything a launch can point at; the engine's own batch buffers (mix_*, aug_*) in the public
    (B,T,N[,4]) shape of the tensors they stand for"""
    cfg = engine.cfg
    L = cfg.n_layers
    shape = tuple(batch["slot_class"].shape)
    b = {}
    for l in range(L + 1):
        b["x[%d]" % l] = engine.x[l][:M]
    for n in ("h1", "qkv", "att", "xmid", "h2", "u", "gl"):
        for l in range(L):
            b["%s[%d]" % (n, l)] = getattr(engine, n)[l][:M]
    for i in range(2 * L + 1):
        b["stats[%d].mean" % i], b["stats[%d].rstd" % i] = engine.stats[i][0][:M], engine.stats[i][1][:M]
    for n in ("xf", "out", "dout", "dx", "dh", "du", "dqkv"):
        b[n] = getattr(engine, n)[:M]
    n_clip = sum(k.per_clip for k in engine.attn)
    if n_clip:                                               # by lse ROW (vlg.attention.lse_rows): the layer itself for "clip"
        for row in range(n_clip):
            b["lse[%d]" % row] = engine.lse[row][:cfg.n_heads * M]
        b["delta"] = engine.delta[:cfg.n_heads * M]
    for n in engine.layout:
        b["p:" + n] = engine.p(n)
        if engine.params_bf16 is not None:
            b["pb:" + n] = engine.view(engine.params_bf16, n)
    for k, t in batch.items():
        b["batch:" + k] = t
    b["loss_out"], b["loss_scratch"] = engine.loss_out, engine.loss_scratch
    if engine.drop_step is not None:                         # an engine built with dropout > 0
        b["ybranch"], b["ddrop"], b["drop_step"] = engine.ybranch[:M], engine.ddrop[:M], engine.drop_step
    if engine.sched_counter is not None:                     # ... with scheduled sampling
        b["mix_cls"], b["mix_box"], b["sched_step"] = engine.mix_cls[:M].view(shape), engine.mix_box[:M].view(shape + (4,)), engine.sched_counter
    if engine.aug_counter is not None:                       # ... with augmentation
        b["aug_cls"], b["aug_valid"], b["aug_step"] = engine.aug_cls[:M].view(shape), engine.aug_valid[:M].view(shape), engine.aug_counter
        b["aug_box"], b["aug_tgt_box"] = engine.aug_box[:M].view(shape + (4,)), engine.aug_tgt_box[:M].view(shape + (4,))
    if engine.class_weights is not None:
        b["class_weights"] = engine.class_weights
    if cfg.gaussian_box:
        b["box_nll_scratch"] = engine.box_nll_scratch
    return b


# the scalar arguments that launch_scalars names, by their parameter names in include/vlg_hip.h
_SCALAR_PARAMS = {"vlg_layout_loss_ext": ("label_smoothing", "flags"),
                  "vlg_layout_box_nll": ("s_min", "s_max", "w_nll"),
                  "vlg_layout_mix_inputs": ("thr_max", "ramp_steps", "temperature", "top_k", "seed"),
                  "vlg_layout_augment": ("thr_flip", "thr_drop", "zoom", "shift", "jitter", "seed")}


def trace(engine, batch):
    """Run engine.forward_backward(batch) under the recording wrapper -> (records, state)."""
    from ctypes import c_uint32, c_void_p
    from vlg import hip
    B, T, N = batch["slot_class"].shape
    M = B * T * N
    bufs = _buffers(engine, batch, M)
    by_ptr = {t.data_ptr(): n for n, t in bufs.items()}
    assert len(by_ptr) == len(bufs), "two buffers share a pointer"
    records = []
    launch = engine._timed                                   # the bound method
    counters = {n: bufs[n] for n in SS.COUNTERS if n in bufs}
    snapshots = SS.snapshot_names("drop_step" in bufs, engine.cfg.gaussian_box)
    every = "sched_step" in bufs         # scheduled sampling: pass 2 overwrites pass 1's buffers - snapshot whatever a launch names
    caller = {k: t.detach().cpu().clone() for k, t in batch.items()}

    def recording(family, flops, name, *args, nbytes=0.0):
        launch(family, flops, name, *args, nbytes=nbytes)
        torch.cuda.synchronize()
        types = hip.SIGNATURES[name][1]
        ops = tuple(None if a == 0 else by_ptr.get(a, "arena") for a, ty in list(zip(args, types))[:-1] if ty is c_void_p)
        rec = dict(family=family, name=name, flags=args[hip.param_index(name, _FLAGS_PARAM[name])] if name in _FLAGS_PARAM else None,
                   ops=ops, scalars=None)
        if every:
            rec["after"] = dict(records[-1]["after"] if records else {})
            rec["after"].update({n: bufs[n].detach().cpu().clone() for n in set(ops) if n in bufs and not n.startswith(SS.FIXED) and n not in counters})
        else:
            rec["after"] = {n: bufs[n].detach().cpu().clone() for n in snapshots if n in bufs}
        if name in _SCALAR_PARAMS:
            rec["scalars"] = {k: args[hip.param_index(name, k)] for k in _SCALAR_PARAMS[name]}
        elif "dropout" in name and c_uint32 in types:        # the fused entry points: (uint32 thr, float scale, uint64 seed, int site)
            i = types.index(c_uint32)
            rec["scalars"] = dict(zip(("thr", "scale", "seed", "site"), args[i:i + 4]))
        rec["counters"] = {n: int(t.item()) for n, t in counters.items()}
        records.append(rec)

    engine._timed = recording                                # instance attribute: this engine only
    try:
        engine.forward_backward(batch)
        torch.cuda.synchronize()
    finally:
        del engine._timed
    state = {n: t.detach().cpu().clone() for n, t in bufs.items()
             if n not in SS.BACKWARD_BUFFERS + ("ybranch", "ddrop") and not n.startswith("batch:")}
    state["loss"] = state.pop("loss_out")
    state["grads"] = {n: g.detach().cpu().clone() for n, g in engine.named_grads().items()}
    state["caller"] = ({k: t.detach().cpu().clone() for k, t in batch.items()}, caller)      # after the step, before it
    return records, state


def _param_grad_bar(got, want64, cpu32, M, what, native_dw):
    """test_hip_gemm_paths.check_wgrad: 1e-4 relative / 1e-5 absolute after the 1 / sqrt(M) scale; a native fp32 dW also
    within 4 x torch-CPU fp32's own error (_vs_cpu_fp32)."""
    sc = math.sqrt(M)
    check_close(got / sc, want64 / sc, rtol=1e-4, atol=1e-5, what=what)
    if native_dw:
        from test_hip_gemm_paths import _vs_cpu_fp32
        _vs_cpu_fp32(got, want64, cpu32, what)


def _less(t, want64, slack):
    """t moved towards want64 by at most slack, elementwise (a NaN stays a NaN)"""
    err = t.double() - want64
    return want64 + torch.sign(err) * (err.abs() - slack).clamp(min=0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dropped_set_fwd(x_out, y, resid, keep, scale):
    """test_hip_dropout.test_forward_kernel's rule on a fused forward launch: the elements of x_out that are bitwise resid
    (+0.0 without one) are EXACTLY the complement of the reference mask.  That test keeps |y| >= 0.1 so that a kept element
    always moves its residual; here y is what the step computed, and a kept element with |y * scale| <= 2^-23 |resid| (half
    an ulp of resid is at most 2^-24 |resid|; the factor 2 covers the product's rounding), or y = 0 at site 0, cannot show
    that it was kept.  Those - of the order of one element in 10^7 - are left out; every other element decides."""
    base = torch.zeros_like(x_out) if resid is None else resid
    dropped = _bits(x_out) == _bits(base)
    silent = keep & (y.double().abs() * scale <= 2.0 ** -23 * base.double().abs())
    wrong = (dropped != ~keep) & ~silent
    assert not bool(wrong.any()), "the dropped set of x_out differs from the reference mask in %d elements" % int(wrong.sum())


def _dropped_set_bwd(ddrop, dx, keep, scale):
    """test_hip_dropout.test_backward_kernel's rule: ddrop is bitwise 0 on the reference's dropped set and within 1 ulp of
    fp32(dx * scale), of the dx this launch stored, elsewhere"""
    assert bool((_bits(ddrop)[~keep] == 0).all()), "ddrop is not exactly 0 on the dropped set"
    want = dx * torch.tensor(scale, dtype=torch.float32)
    lo, hi = (torch.nextafter(want, torch.full_like(want, s * float("inf"))) for s in (-1, 1))
    ok = (ddrop >= lo) & (ddrop <= hi)
    assert bool(ok[keep].all()), "ddrop off by more than 1 ulp from dx * scale in %d kept elements" % int((~ok[keep]).sum())


def _f32(v):
    """a scalar argument as the C ABI receives it: a float rounded to fp32, an integer as it is"""
    return torch.tensor(v, dtype=torch.float32).item() if isinstance(v, float) else v


def _check_loss(e, cfg, c, got, get, B, T, N, stage):
    """the loss launch: test_hip_layout_ops._loss_check, or - any loss option on - test_hip_layout_loss_ext.check with that
    file's floors, on the 24 columns and four values the launch owns; dout rows of padded and dropped slots exactly 0"""
    nc = cfg.n_classes
    pad = SS.to_rows(get(e["valid"])[..., None])[:, 0] == 0
    dout, loss = got["dout"][:, :nc + 4], got["loss_out"][:4]
    assert bool((dout[pad] == 0).all()), "dout rows of padded slots are not exactly 0"
    o = SS.from_rows(get("out"), B, T, N)
    lb = dict(tgt_class=get(e["tgt_class"]), tgt_box=get(e["tgt_box"]), valid=get(e["valid"]))
    if c.loss is None:
        from test_hip_layout_ops import _loss_check
        _loss_check(loss, dout, o[..., :nc], o[..., nc:nc + 4], lb)
    else:
        import test_hip_layout_loss_ext as X
        weights, eps, overlap = c.loss
        ref, floors = X.reference_on(o[..., :nc], o[..., nc:nc + 4], lb, O.SMOOTH_L1_BETA,
                                     None if weights is None else torch.as_tensor(weights, dtype=torch.float32), eps,
                                     X.GIOU if overlap == "giou" else 0)
        X.check(loss, dout, ref, floors, stage)


def _check_box_nll(cfg, c, got, get, ref, stage):
    """the NLL launch: boxhead_ref.check_nll on the scale columns and loss_out[4:6]; bitwise: the loss launch's columns of dout
    and loss_out[1:4] as they were (the mean is detached), the padding columns and loss_out[6:8] zero; loss_out[0] = the loss
    launch's total + w_nll * box_nll in fp32 from the launch's own box_nll (test_hip_box_nll's bar: 2^-23 relative)"""
    nc = cfg.n_classes
    dout, lo, dout0, lo0 = got["dout"], got["loss_out"], get("dout"), get("loss_out")
    assert torch.equal(_bits(dout[:, :nc + 4]), _bits(dout0[:, :nc + 4])), "the NLL launch changed the class or mean columns of dout"
    assert bool((dout[:, nc + 8:] == 0).all()), "the padding columns' gradient is not exactly 0"
    boxhead_ref.check_nll(dout[:, nc + 4:nc + 8], lo[4], lo[5], ref, stage)
    assert float(lo[6]) == 0.0 and float(lo[7]) == 0.0 and torch.equal(_bits(lo[1:4]), _bits(lo0[1:4])), "loss_out[1:4] / [6:8] touched"
    want0 = lo0[0].float() + torch.tensor(c.box_nll_weight, dtype=torch.float32) * lo[4].float()
    assert abs(float(lo[0]) - float(want0)) <= 2.0 ** -23 * abs(float(want0)), "total %r, the loss launch's + w_nll * box_nll = %r" % (
        float(lo[0]), float(want0))


def _check_mix(e, cfg, c, got, want, get, detail, stage, log):
    """test_hip_sched_mix._check's rule on the `out` the launch read: classes exact off the restatement's near draws (fewer than
    1 % of the draws, that file's cap), replaced boxes within vs_cpu32 of the fp64 sigmoid, every other token bit-equal"""
    nc = cfg.n_classes
    rep, near = detail["replaced"], detail["near"]
    got_c, got_b, cls, box = got["mix_cls"], got["mix_box"], get(e["cls"]), get(e["box"])
    B, T, N = cls.shape
    assert torch.equal(got_c[~near], want["mix_cls"][~near]), "%d mixed classes differ from the restatement's" % int(
        (got_c != want["mix_cls"])[~near].sum())
    assert bool(((got_c[rep] >= 0) & (got_c[rep] < nc)).all()), "a replaced class outside [0, n_classes)"
    assert torch.equal(got_c[~rep], cls[~rep]) and torch.equal(_bits(got_b[~rep].float()), _bits(box[~rep])), "an untouched token changed"
    if bool(rep.any()):
        src32 = torch.sigmoid(get("out").float()[:, nc:nc + 4])                     # torch-CPU fp32 yardstick, gathered like the fp64 value
        b, t, n = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(N), indexing="ij")
        rows = ((b * N + n) * T + (t - 1))[rep]
        vs_cpu32(got_b[rep], want["mix_box"][rep], src32[rows], "boxes of replaced tokens")
    assert not bool(near.any()) or int(near.sum()) < 0.01 * int(rep.sum()), "%d of %d draws within the margin of a boundary" % (
        int(near.sum()), int(rep.sum()))
    if log is not None:
        log.append((stage, "draws left out", float(near.sum()), float(rep.sum())))


def _check_augment(got, want, state):
    """test_hip_augment's rule: all four outputs bitwise augment_ref.augment's; the caller's tensors are only read"""
    for n, t in got.items():
        w = want[n]
        same = torch.equal(t, w) if not t.is_floating_point() else torch.equal(_bits(t.float()), _bits(w.float()))
        assert same, "%s differs from augment_ref.augment in %d elements" % (n, int((t != w).sum()))
    after, before = state["caller"]
    for k, t in before.items():
        assert torch.equal(after[k], t), "the launch modified the caller's %s" % k


def check(records, state, cfg, c, batch, log=None):
    """See the module docstring.  `log`, a list, receives (stage, output, max |err| vs fp64, torch-CPU fp32's) per output."""
    B, T, N = batch["slot_class"].shape
    M = B * T * N
    sched = SS.schedule(cfg, c)
    assert [r["name"] for r in records] == [e["entry"] for e in sched], "the launches are not the contract's schedule: %s" % (
        [(r["name"], e["entry"]) for r, e in zip(records, sched) if r["name"] != e["entry"]][:3] or (len(records), len(sched)),)
    prev, pending, counters = {}, [], c.counters()
    for e, r in zip(sched, records):
        stage = e["stage"]
        try:
            assert r["family"] == e["family"], "family %s, contract %s" % (r["family"], e["family"])
            assert r["flags"] == e.get("flags"), "flags word %s, contract %s" % (r["flags"], e.get("flags"))
            assert len(r["ops"]) == len(e["ops"]) and all(w == "*" or g == w for g, w in zip(r["ops"], e["ops"])), \
                "operands %s, contract %s" % (r["ops"], e["ops"])

            def get(n):
                if n.startswith("batch:"):
                    return batch[n[6:]]
                return prev[n] if c.snap(n) else state["loss"] if n == "loss_out" else state[n]

            def val(dt):
                return lambda n: None if n is None else get(n).to(dt) if get(n).is_floating_point() else get(n)

            if e["kind"] == "advance":
                counters[e["counter"]] += 1
            assert r["counters"] == counters, "the step counters read %s after this launch, contract %s" % (r["counters"], counters)
            scalars = SS.launch_scalars(cfg, c, e)
            if scalars is not None:
                seen = None if r["scalars"] is None else {k: _f32(v) for k, v in r["scalars"].items()}
                assert seen == {k: _f32(v) for k, v in scalars.items()}, "scalar arguments %s, contract %s" % (r["scalars"], scalars)
            want, detail = {}, {torch.float64: {}, torch.float32: {}}
            for dt in (torch.float64, torch.float32):
                want[dt] = SS.run_stage(e, cfg, c, batch, val(dt), detail[dt])
            (o64, g64), (o32, g32) = want[torch.float64], want[torch.float32]
            slack = {}
            if c.store_bf16 and e["kind"] in ("clip_fwd", "clip_bwd", "frame_fwd", "frame_bwd"):      # P and dS are rounded on chip: step_stages.flip_step
                slack = SS.operand_flip_slack(e["kind"], detail[torch.float64], detail[torch.float32], B, T, N)
            got = {n: (r["after"][n] if c.snap(n) else state["loss"] if n == "loss_out" else state[n]) for n in o64}
            for n, t in got.items():
                assert t.dtype == c.dtype(n), "%s is stored as %s, contract %s" % (n, t.dtype, c.dtype(n))
                assert t.shape == o64[n].shape, "%s has shape %s, contract %s" % (n, tuple(t.shape), tuple(o64[n].shape))
            if "site" in e:
                keep, scale = SS.site_mask(c, M, cfg.d, e["site"])
                if e["kind"] == "drop_ln_fwd":
                    _dropped_set_fwd(got[e["x_out"]], get(e["y"]), None if e["resid"] is None else get(e["resid"]), keep, scale)
                else:
                    _dropped_set_bwd(got["ddrop"], got["dx"], keep, scale)
            if e["kind"] == "loss":
                if log is not None:
                    nc = cfg.n_classes + 4
                    log.append((stage, "dout", float((got["dout"][:, :nc].double() - o64["dout"][:, :nc]).abs().max()),
                                float((o32["dout"][:, :nc].double() - o64["dout"][:, :nc]).abs().max())))
                _check_loss(e, cfg, c, got, get, B, T, N, stage)
            elif e["kind"] == "box_nll":
                _check_box_nll(cfg, c, got, get, detail[torch.float64]["nll"], stage)
            elif e["kind"] == "sched_mix":
                _check_mix(e, cfg, c, got, o64, get, detail[torch.float64], stage, log)
            elif e["kind"] == "augment":
                _check_augment(got, o64, state)
            else:
                for n, t in got.items():
                    is16, sl = t.dtype == BF, slack.get(n.split("[")[0])
                    t = t.double()
                    if sl is not None:
                        t, o32[n] = _less(t, o64[n], sl), _less(o32[n], o64[n], sl)
                    if log is not None:
                        log.append((stage, n, float((t.double() - o64[n]).abs().max()), float((o32[n].double() - o64[n]).abs().max())))
                    if n == "dqkv":
                        d = cfg.d
                        pad = SS.to_rows(get(e["pad"])[..., None])[:, 0] == 0
                        assert bool((t[pad] == 0).all()), "dqkv rows of padded slots are not exactly 0: a masked key got a gradient"
                        for i, part in enumerate(("dq", "dk", "dv")):
                            sl = slice(i * d, (i + 1) * d)
                            vs_cpu32(t[:, sl], o64[n][:, sl], o32[n][:, sl], part, bf16=is16)
                    else:
                        vs_cpu32(t, o64[n], o32[n], n, bf16=is16)
            pending += [(stage, n, g64[n], g32[n]) for n in g64]
            prev = r["after"]
        except AssertionError as err:
            raise AssertionError("[%s] %s" % (stage, err)) from None
    assert sorted(n for _, n, _, _ in pending) == sorted(state["grads"]), "a parameter has no launch as its gradient's source"
    for stage, n, w64, w32 in pending:
        try:
            got = state["grads"][n]
            assert bool(torch.isfinite(got).all()), "grad %s not finite" % n
            native = c.precision == "fp32" and n.endswith("_w") and n.split(".")[-1] in ("qkv_w", "proj_w", "ff1_w", "ff2_w", "head_w")
            if log is not None:
                log.append((stage, "grad " + n, float((got.double() - w64).abs().max()), float((w32.double() - w64).abs().max())))
            _param_grad_bar(got, w64, w32, M, "grad " + n, native)
        except AssertionError as err:
            raise AssertionError("[%s] %s" % (stage, err)) from None
