"""Trace one LayoutEngine.rollout / rollout_samples call launch by launch, and check every launch against fp64 evaluated on the
values that launch read (the stage functions of rollout_stages.py and step_stages.py).  Plain module: test infrastructure,
nothing collected.  The method is step_trace.py's; generation overwrites almost every buffer in place, so the snapshot rule is
scheduled sampling's: after every launch, clone every engine-owned buffer that launch names.

trace(engine, slot_class, slot_box, samples=None, sample0=0, **rollout_kw)  replaces engine._timed - the single launch point -
    on that ONE instance by a wrapper that launches, synchronises and records family, entry point, flags word, the scalar
    arguments by header name (vlg.hip.param_index: leading dimensions, T, t_read, p, ldo, pos, steps, step, the decode knobs,
    clips, sample0) and, behind every pointer argument, the name and row offset of an engine buffer (rollout_stages' names).
    engine._rollout is wrapped too: logits, gen_cls and gen_box are allocated inside it, so pointers into them are resolved when
    the pass returns, and what it returns is cloned per pass (a rollout_samples call makes several).  The window buffers are
    cloned before the first launch of each pass.
check(records, state, cfg, contract, prompt, passes=None)  walks rollout_stages.rollout_schedule beside the records.  A failure
    is an AssertionError whose message starts with "[pass <k> frame <i> <launch>]".  Per launch:
      identity    entry point, family, flags word, operand names with offsets and scalars are the schedule's; stored dtypes the
                  contract's; as many launches as the schedule has
      prompt      before the first launch of a pass the window is the prompt rule (rollout_stages.initial_window), bitwise
      encoder     embedding, layer-norm, projections, per-slot step, per-slot window attention: helpers.vs_cpu32 against the
                  stage function in fp64 on the launch's own inputs (torch-CPU fp32 of the same function as the yardstick), a bf16
                  output one rounding more; projection operands rounded per contract.  Per-clip / frame window attention:
                  step_trace.check's rule for those kinds (step_stages.operand_flip_slack under bf16).  Clip and frame step:
                  test_hip_clip_attention_step.under_bar (fp32: vs_cpu32; bf16: rel-L2 1e-2, 2^-6 of the largest value)
      the cache   after a cached q k v launch the 3d columns of position p of each of the B*N cache rows are the product and
                  EVERY other element of qkv[l] is bit for bit what it was; an attention step leaves qkv[l] untouched
      head        vs_cpu32 against test_hip_layout_decode._head_ref's arithmetic on the fp32 master weights
      decode      on the logits[i] the launch read: classes equal the fp64 rule's (decode_ref / boxhead_ref / samples_ref)
                  outside its exclusion width, boxes within 1e-6 (a drawn box: boxhead_ref.box_bar), kept padded slots keep id
                  and box bitwise; bitwise: the appended frame, valid, the compact grow.cls / grow.box copy, gen_*[:, i], every
                  other frame of the window as it was - or the slid window: frames 1 .. T-1 of the other buffer, then the new one
      tie cap     at most 1 % of a case's decoded tokens inside the exclusion width: asserted"""
import torch

import rollout_stages as RS
import step_stages as SS
from helpers import vs_cpu32
from step_trace import _bits, _f32, _less

BF = torch.bfloat16
_DECODE_SCALARS = ("ld", "pos", "steps", "step", "temperature", "top_k", "box_temperature", "seed", "keep_padded", "clips", "sample0")


def _scalar_names(name, params):
    if name == "vlg_embed_fwd":
        want = ("T",)
    elif name == "vlg_linear_fwd":
        want = ("lda", "ldw", "ldc")
    elif name.startswith("vlg_head_"):
        want = ("T", "t_read")
    elif "_step" in name:
        want = ("p", "ldo")
    elif name.startswith("vlg_layout_decode"):
        want = _DECODE_SCALARS
    else:
        want = ()
    return tuple(n for n in want if n in params)


def _pass_buffers(engine, B, N, grown):
    """name -> device view of every engine-owned buffer a launch of this pass can point at (rollout_stages' names)"""
    cfg = engine.cfg
    T, L = cfg.T, cfg.n_layers
    M, BN = B * T * N, B * N
    b = {}
    for k, (cls, box, valid) in enumerate(engine._windows()):
        b["win%d.cls" % k], b["win%d.box" % k], b["win%d.valid" % k] = cls[:M].view(B, T, N), box[:M].view(B, T, N, 4), valid[:M].view(B, T, N)
    for l in range(L + 1):
        b["x[%d]" % l] = engine.x[l][:M]
    for n in ("h1", "qkv", "att", "xmid", "h2", "u", "gl"):
        for l in range(L):
            b["%s[%d]" % (n, l)] = getattr(engine, n)[l][:M]
    for i in range(2 * L):
        b["stats[%d].mean" % i], b["stats[%d].rstd" % i] = engine.stats[i][0][:M], engine.stats[i][1][:M]
    for row in range(sum(k.per_clip for k in engine.attn)):
        b["lse[%d]" % row] = engine.lse[row][:cfg.n_heads * M]
    if grown:
        g = engine._grow_buffers()
        b["grow.cls"], b["grow.box"] = g["cls"][:BN].view(B, N), g["box"][:BN].view(B, N, 4)
        for n in ("xa", "xb", "xmid", "h", "att", "u", "gl"):
            b["grow." + n] = g[n][:BN]
        b["grow.stat.mean"], b["grow.stat.rstd"] = g["stat"][0][:BN], g["stat"][1][:BN]
    return b


def trace(engine, slot_class, slot_box, samples=None, sample0=0, **rollout_kw):
    """Run engine.rollout(slot_class, slot_box, return_logits=True, **rollout_kw) - with `samples`, engine.rollout_samples -
    under the recording wrappers -> (records, state).  state: passes = [dict(before = the windows before the first launch,
    logits, gen_cls, gen_box as that _rollout call returned them, B)], params = {"p:..." / "pb:...": tensor}, result = what
    the call returned (device tensors)."""
    from ctypes import c_void_p
    from vlg import hip
    fixed = {}
    for n in engine.layout:
        fixed["p:" + n] = engine.p(n)
        if engine.params_bf16 is not None:
            fixed["pb:" + n] = engine.view(engine.params_bf16, n)
    records, passes = [], []
    launch, rollout = engine._timed, engine._rollout
    live = {}                                                # the pass in flight: bufs, ranges, its records

    def ranges(bufs):
        return sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), n, t) for n, t in bufs.items())

    def resolve(a, table):
        if a == 0:
            return None
        for lo, hi, n, t in table:
            if lo <= a < hi:
                off = (a - lo) // t.element_size()
                unit = t.shape[-1] if t.dim() >= 2 else 1
                return n if off == 0 else "%s+%d" % (n, off // unit) if off % unit == 0 else "%s+%de" % (n, off)
        return a                                             # logits / gen_*: resolved when the pass returns

    def recording(family, flops, name, *args, nbytes=0.0):
        if not live["records"]:
            live["before"] = {n: t.detach().cpu().clone() for n, t in live["bufs"].items() if n.startswith("win")}
        launch(family, flops, name, *args, nbytes=nbytes)
        torch.cuda.synchronize()
        types, params = hip.SIGNATURES[name][1], hip.PARAMS[name]
        ops = tuple(resolve(a, live["table"]) for a, ty in list(zip(args, types))[:-1] if ty is c_void_p)
        rec = dict(family=family, name=name, ops=ops, flags=args[hip.param_index(name, "epilogue")] if name == "vlg_linear_fwd" else None)
        names = _scalar_names(name, params)
        rec["scalars"] = {k: args[hip.param_index(name, k)] for k in names} if names else None
        rec["after"] = {n.split("+")[0]: live["bufs"][n.split("+")[0]].detach().cpu().clone() for n in set(ops)
                        if isinstance(n, str) and n.split("+")[0] in live["bufs"]}
        rec["pass"] = len(passes)
        live["records"].append(rec)

    def one_pass(slot_class, slot_box, steps, *a, **kw):
        B, P, N = slot_class.shape
        bufs = _pass_buffers(engine, B, N, P < engine.cfg.T)
        live.update(bufs=bufs, table=ranges(dict(bufs, **fixed)), records=[], before=None)
        out = rollout(slot_class, slot_box, steps, *a, **kw)
        torch.cuda.synchronize()
        gen_cls, gen_box, logits = out
        late = {gen_cls.data_ptr(): "gen_cls", gen_box.data_ptr(): "gen_box"}
        row = logits[0].numel() * logits.element_size()
        late.update({logits.data_ptr() + i * row: "logits[%d]" % i for i in range(logits.shape[0])})
        for r in live["records"]:
            r["ops"] = tuple(late.get(n, "?") if isinstance(n, int) else n for n in r["ops"])
        records.extend(live["records"])
        passes.append(dict(before=live["before"], logits=logits.detach().cpu().clone(), gen_cls=gen_cls.detach().cpu().clone(),
                           gen_box=gen_box.detach().cpu().clone(), B=B))
        return out

    engine._timed, engine._rollout = recording, one_pass      # instance attributes: this engine only
    try:
        if samples is None:
            result = engine.rollout(slot_class, slot_box, return_logits=True, **rollout_kw)
        else:
            result = engine.rollout_samples(slot_class, slot_box, samples=samples, sample0=sample0, return_logits=True, **rollout_kw)
        torch.cuda.synchronize()
    finally:
        del engine._timed, engine._rollout
    state = dict(passes=passes, params={n: t.detach().cpu().clone() for n, t in fixed.items()}, result=result)
    return records, state


# ------------------------------------------------------------------------------------------------------------ the checker
def _frac32(got, w64, w32, bf16):
    """the error of vs_cpu32's comparison as a fraction of its bar"""
    err = (got.double() - w64).abs()
    if bf16:
        err = err - 2.0 ** -8 * w64.abs()
    bar = 4 * float((w32.double() - w64).abs().max()) + 2.0 ** -20 * float(w64.abs().max())
    return float(err.max()) / bar if bar > 0 else (0.0 if float(err.max()) <= 0 else float("inf"))


def _same(a, b):
    """bitwise, NaN included"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    if a.dtype == BF:
        return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
    return torch.equal(_bits(a), _bits(b))


def _check_prompt(cfg, before, pc, pb):
    wc, wb, wv = RS.initial_window(cfg, pc, pb)
    P = pc.shape[1]
    assert torch.equal(before["win0.cls"][:, :P], pc) and _same(before["win0.box"][:, :P], pb), "the prompt's frames are not copied"
    assert torch.equal(before["win0.cls"], wc) and _same(before["win0.box"], wb), "frames after the history: not the reserved id and zero boxes"
    assert _same(before["win0.valid"], wv), "valid is not (class < n_classes)"


def _check_decode(e, r, cfg, c, ps, cur, log):
    """-> the number of tokens inside the exclusion width"""
    T, nc, i, w, pos = cfg.T, cfg.n_classes, e["i"], e["win"], e["pos"]
    h = T if pos is None else pos
    wc, wb, wv = cur[w + ".cls"], cur[w + ".box"], cur[w + ".valid"]
    want_c, want_b, near = RS.decode_frame(cfg, c, ps["logits"][i], wc[:, :h], wb[:, :h], i)
    gen_c, gen_b = ps["gen_cls"][:, i], ps["gen_box"][:, i]
    after = r["after"]
    assert gen_c.dtype == torch.int64 and gen_b.dtype == torch.float32, "gen_cls / gen_box stored as %s / %s" % (gen_c.dtype, gen_b.dtype)
    assert torch.equal(gen_c[~near], want_c[~near]), "%d classes differ from the rule on the logits the launch read" % int(
        (gen_c != want_c)[~near].sum())
    berr, bar = float((gen_b.double() - want_b).abs().max()), RS.box_bar(c)
    log.append(("decode box", berr / bar))
    assert bool(torch.isfinite(gen_b).all()) and berr <= bar, "boxes off the rule by %.3e (bar %.1e)" % (berr, bar)
    pad = wc[:, h - 1] >= nc
    if c.knobs["keep_padded"]:
        assert torch.equal(gen_c[pad], wc[:, h - 1][pad]) and _same(gen_b[pad], wb[:, h - 1][pad]), "a padded slot did not keep its id and box"
        assert bool((gen_c[~pad] < nc).all()), "a decoded class outside [0, n_classes)"
    else:
        assert bool(((gen_c >= 0) & (gen_c < nc)).all()), "a decoded class outside [0, n_classes)"
    if pos is not None:
        ac, ab, av = after[w + ".cls"], after[w + ".box"], after[w + ".valid"]
        others = [t for t in range(T) if t != pos]
        assert torch.equal(ac[:, others], wc[:, others]) and _same(ab[:, others], wb[:, others]) and _same(av[:, others], wv[:, others]), \
            "a frame other than %d of the window changed" % pos
        assert torch.equal(ac[:, pos], gen_c) and _same(ab[:, pos], gen_b), "frame %d of the window is not the generated frame" % pos
        assert _same(av[:, pos], (gen_c < nc).float()), "valid of the appended frame is not (class < n_classes)"
        assert torch.equal(after["grow.cls"], gen_c) and _same(after["grow.box"], gen_b), "the compact grow.cls / grow.box copy is not the new frame"
    else:
        nw = e["new"]
        assert torch.equal(after[w + ".cls"], wc) and _same(after[w + ".box"], wb), "the slide modified the window it read"
        want_cls = torch.cat([wc[:, 1:], gen_c[:, None]], 1)
        assert torch.equal(after[nw + ".cls"], want_cls) and _same(after[nw + ".box"], torch.cat([wb[:, 1:], gen_b[:, None]], 1)), \
            "the next window is not frames 1 .. T-1 and the generated frame"
        assert _same(after[nw + ".valid"], (want_cls < nc).float()), "valid of the next window is not (class < n_classes)"
    return int(near.sum())


def check(records, state, cfg, c, prompt, passes=None, log=None):
    """See the module docstring.  prompt = (cls (B,P,N), box (B,P,N,4)) on the CPU; passes: vlg.samples.sample_passes' list for a
    rollout_samples trace (None: one rollout() call under `c` as it is).  `log`, a list, receives (launch kind, the error as a
    fraction of its bar) per compared output.  -> (tokens inside the exclusion width, decoded tokens)."""
    from test_hip_clip_attention_step import bf16_model, under_bar
    pc, pb = prompt
    B0, P, N = pc.shape
    T, d = cfg.T, cfg.d
    log = [] if log is None else log
    plan = [(c, 1)] if passes is None else [(c.for_pass(B0, first, k), k) for first, k in passes]
    assert len(state["passes"]) == len(plan), "%d passes, contract %d" % (len(state["passes"]), len(plan))
    cur, n_near, n_tokens = dict(state["params"]), 0, 0
    for j, ((cj, k), ps) in enumerate(zip(plan, state["passes"])):
        B = k * B0
        BN, steps = B * N, ps["logits"].shape[0]
        sched = RS.rollout_schedule(cfg, cj, P, steps)
        recs = [r for r in records if r["pass"] == j]
        try:
            assert ps["B"] == B, "the pass ran %d clips, contract %d" % (ps["B"], B)
            _check_prompt(cfg, ps["before"], pc.repeat(k, 1, 1), pb.repeat(k, 1, 1, 1))
        except AssertionError as err:
            raise AssertionError("[pass %d prompt] %s" % (j, err)) from None
        cur.update(ps["before"])
        n_tokens += steps * BN
        for e, r in zip(sched, recs):
            stage = "pass %d %s" % (j, e["stage"])
            try:
                assert r["name"] == e["entry"], "entry point %s, contract %s" % (r["name"], e["entry"])
                assert r["family"] == e["family"], "family %s, contract %s" % (r["family"], e["family"])
                assert r["flags"] == e.get("flags"), "flags word %s, contract %s" % (r["flags"], e.get("flags"))
                assert tuple(r["ops"]) == tuple(e["ops"]), "operands %s, contract %s" % (r["ops"], e["ops"])
                seen = None if r["scalars"] is None else {n: _f32(v) for n, v in r["scalars"].items()}
                want = None if e["scalars"] is None else {n: _f32(v) for n, v in e["scalars"].items()}
                assert seen == want, "scalar arguments %s, contract %s" % (r["scalars"], e["scalars"])
                for n, t in r["after"].items():
                    assert t.dtype == cj.dtype(n), "%s is stored as %s, contract %s" % (n, t.dtype, cj.dtype(n))
                if e["kind"].startswith("decode"):
                    n_near += _check_decode(e, r, cfg, cj, ps, cur, log)
                    cur.update(r["after"])
                    continue

                def get(n):
                    return ps["logits"][int(n[7:-1])] if n.startswith("logits[") else cur[n]

                def val(dt):
                    return lambda n: None if n is None else get(n).to(dt) if get(n).is_floating_point() else get(n)

                detail = {torch.float64: {}, torch.float32: {}}
                o64, o32 = (RS.run_stage(e, cfg, cj, B, N, val(dt), detail[dt]) for dt in (torch.float64, torch.float32))
                kind, label = e["kind"], e["stage"].split(" ")[-1].split(".")[-1] + ("" if e["encoder"] == "window" else " (step)")
                slack = {}
                if cj.store_bf16 and kind in ("clip_fwd", "frame_fwd"):
                    slack = SS.operand_flip_slack(kind, detail[torch.float64], detail[torch.float32], B, T, N)
                if kind.endswith("_step") and kind.split("_")[0] in ("slot", "clip", "frame"):
                    q = "qkv[%d]" % e["l"]
                    assert _same(r["after"][q], cur[q]), "the attention step modified %s" % q
                for n in o64:
                    got = get(n) if n.startswith("logits[") else r["after"][n]
                    is16 = got.dtype == BF
                    if e.get("scatter") is not None and n == e["c"]:      # the strided store into the cache
                        p = e["scatter"]
                        a3, b3 = got.view(BN, T, 3 * d), cur[n].view(BN, T, 3 * d)
                        others = [t for t in range(T) if t != p]
                        assert _same(a3[:, others].contiguous(), b3[:, others].contiguous()), \
                            "%s changed outside position %d (%d elements)" % (n, p, int((a3[:, others].float() != b3[:, others].float()).sum()))
                        got = a3[:, p]
                    assert got.shape == o64[n].shape, "%s has shape %s, contract %s" % (n, tuple(got.shape), tuple(o64[n].shape))
                    if kind in ("clip_step", "frame_step"):
                        g3, w64, w32 = (t.view(B, N, d) for t in (got.float(), o64[n], o32[n]))
                        if is16:
                            top = float(w64.abs().max())
                            log.append((label, max(float((g3.double() - w64).norm() / w64.norm()) / 1e-2, float((g3.double() - w64).abs().max()) / (2.0 ** -6 * top))))
                        else:
                            log.append((label, _frac32(g3, w64, w32, False)))
                        model = bf16_model(RS._cache(val(torch.float64)("qkv[%d]" % e["l"]), B, T, N), val(torch.float64)(e["valid"]), e["p"]) \
                            if is16 and kind == "clip_step" else None
                        under_bar(g3, w64, w32, is16, stage, model)
                        continue
                    t, w32 = got.double(), o32[n]
                    sl = slack.get(n.split("[")[0])
                    if sl is not None:
                        t, w32 = _less(t, o64[n], sl), _less(w32, o64[n], sl)
                    log.append((label, _frac32(t, o64[n], w32, is16)))
                    vs_cpu32(t, o64[n], w32, n, bf16=is16)
                cur.update(r["after"])
            except AssertionError as err:
                raise AssertionError("[%s] %s" % (stage, err)) from None
        assert len(recs) == len(sched), "[pass %d] %d launches, contract %d" % (j, len(recs), len(sched))
    assert n_near <= 0.01 * n_tokens, "[tie cap] %d of %d decoded tokens inside the exclusion width" % (n_near, n_tokens)
    return n_near, n_tokens


def summary(log):
    """worst fraction of its bar per launch kind"""
    worst = {}
    for k, f in log:
        worst[k] = max(worst.get(k, 0.0), f)
    return ", ".join("%s %.2f" % (k, f) for k, f in sorted(worst.items()))
