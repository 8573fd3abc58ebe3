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
Storage contract: DESIGN.md, "Layout step: storage contract of the reduced-precision modes"."""
import math

import torch

import step_stages as SS
from helpers import check_close, vs_cpu32

BF = torch.bfloat16
_FLAGS_AT = {"vlg_linear_fwd": 12, "vlg_linear_dgrad": 10, "vlg_linear_wgrad": 10, "vlg_linear_dgrad_wgrad": 15}


def _buffers(engine, batch, M):
    """name -> device tensor of everything a launch can point at"""
    cfg = engine.cfg
    L = cfg.n_layers
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
    if cfg.attention == "clip":
        for l in range(L):
            b["lse[%d]" % l] = engine.lse[l][:cfg.n_heads * M]
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
    return b


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
    dropout = "drop_step" in bufs
    snapshots = SS.BACKWARD_BUFFERS + (SS.DROPOUT_BUFFERS if dropout else ())

    def recording(family, flops, name, *args, nbytes=0.0):
        launch(family, flops, name, *args, nbytes=nbytes)
        torch.cuda.synchronize()
        types = hip.SIGNATURES[name][1]
        ops = tuple(None if a == 0 else by_ptr.get(a, "arena") for a, ty in list(zip(args, types))[:-1] if ty is c_void_p)
        rec = dict(family=family, name=name, flags=args[_FLAGS_AT[name]] if name in _FLAGS_AT else None, ops=ops,
                   after={n: bufs[n].detach().cpu().clone() for n in snapshots if n in bufs})
        if dropout:                                          # the fused entry points: (uint32 thr, float scale, uint64 seed, int site)
            i = types.index(c_uint32) if c_uint32 in types else None
            rec["scalars"] = None if i is None else dict(zip(("thr", "scale", "seed", "site"), args[i:i + 4]))
            rec["drop_step"] = int(engine.drop_step.item())
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


def check(records, state, cfg, c, batch, log=None):
    """See the module docstring.  `log`, a list, receives (stage, output, max |err| vs fp64, torch-CPU fp32's) per output."""
    B, T, N = batch["slot_class"].shape
    M = B * T * N
    sched = SS.schedule(cfg, c)
    assert [r["name"] for r in records] == [e["entry"] for e in sched], "the launches are not the contract's schedule: %s" % (
        [(r["name"], e["entry"]) for r, e in zip(records, sched) if r["name"] != e["entry"]][:3] or (len(records), len(sched)),)
    pad = SS.to_rows(batch["valid"][..., None])[:, 0] == 0
    prev, pending = {}, []
    for e, r in zip(sched, records):
        stage = e["stage"]
        try:
            assert r["family"] == e["family"], "family %s, contract %s" % (r["family"], e["family"])
            assert r["flags"] == e.get("flags"), "flags word %s, contract %s" % (r["flags"], e.get("flags"))
            assert len(r["ops"]) == len(e["ops"]) and all(w == "*" or g == w for g, w in zip(r["ops"], e["ops"])), \
                "operands %s, contract %s" % (r["ops"], e["ops"])

            def get(n):
                return prev[n] if n in c.snapshots else state["loss"] if n == "loss_out" else state[n]

            if c.dropout is not None:
                k = c.dropout[2] + (e["kind"] == "advance")
                assert r["drop_step"] == k, "the step counter reads %s after this launch, contract %d" % (r["drop_step"], k)
                if "site" in e:
                    assert r["scalars"] == SS.dropout_scalars(c, e["site"]), "mask arguments %s, contract %s" % (
                        r["scalars"], SS.dropout_scalars(c, e["site"]))
            want, detail = {}, {torch.float64: {}, torch.float32: {}}
            for dt in (torch.float64, torch.float32):
                want[dt] = SS.run_stage(e, cfg, c, batch, lambda n: None if n is None else get(n).to(dt), detail[dt])
            (o64, g64), (o32, g32) = want[torch.float64], want[torch.float32]
            slack = {}
            if c.store_bf16 and e["kind"] in ("clip_fwd", "clip_bwd"):      # P and dS are rounded on chip: step_stages.flip_step
                slack = SS.operand_flip_slack(e["kind"], detail[torch.float64], detail[torch.float32], B, T, N)
            got = {n: (r["after"][n] if n in c.snapshots else state["loss"] if n == "loss_out" else state[n]) for n in o64}
            for n, t in got.items():
                assert t.dtype == c.dtype(n), "%s is stored as %s, contract %s" % (n, t.dtype, c.dtype(n))
            if "site" in e:
                keep, scale = SS.site_mask(c, M, cfg.d, e["site"])
                if e["kind"] == "drop_ln_fwd":
                    _dropped_set_fwd(got[e["x_out"]], get(e["y"]), None if e["resid"] is None else get(e["resid"]), keep, scale)
                else:
                    _dropped_set_bwd(got["ddrop"], got["dx"], keep, scale)
            if e["kind"] == "loss":
                from test_hip_layout_ops import _loss_check
                assert bool((got["dout"][pad] == 0).all()), "dout rows of padded slots are not exactly 0"
                o = SS.from_rows(get("out"), B, T, N)
                _loss_check(got["loss_out"], got["dout"], o[..., :cfg.n_classes], o[..., cfg.n_classes:], batch)
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
