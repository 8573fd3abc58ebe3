"""Stage references of generation: the schedule of launches one LayoutEngine._rollout call makes (rollout_schedule), one pure
function per launch kind the training step lacks (tensors in, tensors out, generic in dtype, outputs unrounded) and
`emulate_rollout`, which chains them along the schedule - the CPU stand-in for the engine.  Plain module: test
infrastructure only, nothing collected.  It follows step_stages.py and takes from it every launch that is the same: the window
encode IS step_stages.forward_launches without the final norm and the head projection.

Storage contract: step_stages' docstring, with the generation facts of vlg/engine.py (_grow_buffers, _rollout):
  bf16       the compact buffers grow.h, grow.att, grow.u, grow.gl are bf16 in memory beside h1, qkv, att, h2, u, gl;
             grow.xa, grow.xb, grow.xmid, grow.stat are fp32
  head       vlg_head_frame / vlg_head_last_frame run on the fp32 MASTER weights (p:lnf_g, p:lnf_b, p:head_w, p:head_b) in every mode
  outputs    logits, gen_box, the windows' box and valid are fp32; gen_cls, the windows' cls and grow.cls int64

Buffer names.  The two window buffers ping-pong BY NAME: win0.cls / win0.box / win0.valid and win1.*, in the public (B,T,N[,4])
shape.  grow.cls (B,N), grow.box (B,N,4) and grow.xa, xb, xmid, h, att, u, gl (B*N rows), grow.stat.mean / .rstd are the compact
set of the cached step.  Where the engine passes an interior pointer the name carries the offset in rows: qkv[l]+p (position p of
the [B*N*T, 3d] cache, written with ldc = T*3d), p:time_emb+p, logits[i].

A cached step (LayoutEngine._encode_step) at position p is _encode with T = 1 on the compact set: the embedding of grow.cls /
grow.box with time_emb row p into grow.xa; per layer l the norm of x[l] (xa for even l, xb for odd) into grow.h and grow.stat, the
q k v product scattered into qkv[l] at position p, the layer kind's _step entry from the cache into grow.att, proj + residual
into grow.xmid, the norm into grow.h, ff1 into grow.gl / grow.u, ff2 + residual into x[l+1].  1 + 7 L launches, as on the window."""
import torch

import boxhead_ref
import decode_ref as D
import samples_ref
import step_stages as SS
from oracle import layout_spec as O
from vlg.attention import cached_by_default, layer_kinds
from vlg.engine import grow_schedule

BF = SS.BF
COMPACT_BF16 = ("grow.h", "grow.att", "grow.u", "grow.gl")
WINDOW_KINDS = ("embed_fwd", "ln_fwd", "linear_fwd", "slot_fwd", "clip_fwd", "frame_fwd")
MASK64 = SS.MASK64
KNOBS = dict(temperature=0.0, top_k=0, seed=0, keep_padded=False, box_temperature=0.0)


class GenContract:
    """step_stages.Contract (precision, attention, masked: `base`) and what generation adds: clip_cache (the opt-in cached step
    of per-clip attention), gaussian (cfg.gaussian_box: the _ext decode entries), the decode knobs (temperature, top_k, seed,
    keep_padded, box_temperature), cache (rollout's argument) and samples = (clips, sample0) of ONE pass of rollout_samples
    (the _samples entries) or None."""

    def __init__(self, precision, attention="slot", masked=False, clip_cache=False, gaussian=False, cache=None, samples=None, **knobs):
        assert not set(knobs) - set(KNOBS), knobs
        self.base = SS.Contract(precision, attention, masked)
        self.precision, self.attention, self.masked = precision, attention, self.base.masked
        self.store_bf16, self.round_operands, self.gemm_flags, self.sfx = (self.base.store_bf16, self.base.round_operands,
                                                                           self.base.gemm_flags, self.base.sfx)
        self.clip_cache, self.gaussian, self.cache, self.samples = bool(clip_cache), bool(gaussian), cache, samples
        self.knobs = dict(KNOBS, **knobs)
        self.knobs["seed"] = int(self.knobs["seed"]) & MASK64
        self.cacheable = self.clip_cache or cached_by_default(attention)

    def for_pass(self, clips, first, k):
        """the contract of one pass of rollout_samples: k samples from sample index `first` of `clips` prompts"""
        return GenContract(self.precision, self.attention, self.masked, self.clip_cache, self.gaussian, self.cache,
                           None if (k == 1 and first == 0) else (clips, first), **self.knobs)      # (one sample from index 0 IS rollout())

    def cached(self, P, T):
        return P < T and self.cacheable and (self.cache is None or bool(self.cache))

    def dtype(self, buf):
        base = buf.split("[")[0].split("+")[0]
        if base.endswith(".cls") or base == "gen_cls":
            return torch.int64
        if base.startswith("pb:"):
            return BF
        if base.startswith(("win", "grow.")) or base in ("logits", "gen_box"):
            return BF if self.store_bf16 and base in COMPACT_BF16 else torch.float32
        return self.base.dtype(buf)

    def bits(self, a=None, b=None, out=None):
        is16 = lambda n: n is not None and (self.store_bf16 if n is True else self.dtype(n) == BF)
        return (SS.EPI_A_BF16 if is16(a) else 0) | (SS.EPI_B_BF16 if is16(b) else 0) | (SS.EPI_OUT_BF16 if is16(out) else 0)

    def weight(self, name):
        return self.base.weight(name)

    @property
    def decode_suffix(self):
        return "_samples" if self.samples is not None else "_ext" if self.gaussian else ""


# ------------------------------------------------------------------------------------------------ the schedule
def _step_launches(out, cfg, c, tag, p, valid):
    """the launches of LayoutEngine._encode_step at position p -> the name of the compact residual stream that leaves it"""
    L, d, ff, T = cfg.n_layers, cfg.d, cfg.d_ff, cfg.T
    kinds = layer_kinds(c.attention, L)
    W = lambda n: "p:" + n
    xs = ["grow.xa", "grow.xb"] * L + ["grow.xa"]
    stat = ("grow.stat.mean", "grow.stat.rstd")

    def ln(stage, x, gname):
        out.append(dict(stage=tag + stage, kind="ln_step", family="ln_fwd", entry="vlg_layernorm_fwd" + c.sfx, x=x, g=gname,
                        ops=(x, W(gname), W(gname[:-1] + "b"), "grow.h") + stat, scalars=None))

    def lin(stage, a, wname, cbuf, n, k, epi, aux_in=None, aux_out=None, scatter=None):
        cop = cbuf if scatter is None else "%s+%d" % (cbuf, scatter)
        out.append(dict(stage=tag + stage, kind="linear_step", family="gemm_fwd", entry="vlg_linear_fwd", a=a, w=wname, c=cbuf, epi=epi,
                        aux_in=aux_in, aux_out=aux_out, scatter=scatter, flags=epi | c.gemm_flags | c.bits(a, True, cbuf),
                        ops=(a, c.weight(wname), W(wname[:-1] + "b"), cop, aux_in, aux_out),
                        scalars=dict(lda=k, ldw=k, ldc=n if scatter is None else T * 3 * d)))

    out.append(dict(stage=tag + "embedding", kind="embed_step", family="embed_fwd", entry="vlg_embed_fwd", p=p, x=xs[0],
                    ops=("grow.cls", "grow.box", W("cls_emb"), W("box_w"), W("box_b"), "p:time_emb" + ("+%d" % p if p else ""), xs[0]),
                    scalars=dict(T=1)))
    epi_ff1 = SS.EPI_BIAS | SS.EPI_GELU | (SS.EPI_GELU_GRAD if c.base.gelu_grad_saved else 0)
    for l in range(L):
        pre, qkv, k = "l%d." % l, "qkv[%d]" % l, kinds[l]
        ln(pre + "ln1", xs[l], pre + "ln1_g")
        lin(pre + "qkv", "grow.h", pre + "qkv_w", qkv, 3 * d, d, SS.EPI_BIAS, scatter=p)
        short = k.family.split("_")[1] if k.per_clip else "slot"
        ops = (qkv, valid, "grow.att") if k.per_clip else (qkv, "grow.att")
        out.append(dict(stage=tag + pre + "attention", kind=short + "_step", family=k.family + "_step", entry=k.stem + "_step" + c.sfx,
                        l=l, p=p, valid=valid if k.per_clip else None, ops=ops, scalars=dict(p=p, ldo=d)))
        lin(pre + "proj", "grow.att", pre + "proj_w", "grow.xmid", d, d, SS.EPI_BIAS | SS.EPI_RESID, aux_in=xs[l])
        ln(pre + "ln2", "grow.xmid", pre + "ln2_g")
        lin(pre + "ff1", "grow.h", pre + "ff1_w", "grow.gl", ff, d, epi_ff1, aux_out="grow.u")
        lin(pre + "ff2", "grow.gl", pre + "ff2_w", xs[l + 1], d, ff, SS.EPI_BIAS | SS.EPI_RESID, aux_in="grow.xmid")
    return xs[L]


def decode_scalars(cfg, c, i, steps, pos):
    """the scalar arguments of the decode launch of generated frame i, by their names in include/vlg_hip.h"""
    k = c.knobs
    s = dict(steps=steps, step=i, temperature=float(k["temperature"]), top_k=int(k["top_k"]), seed=k["seed"], keep_padded=int(bool(k["keep_padded"])))
    if pos is not None:
        s["pos"] = pos
    if c.decode_suffix:
        s.update(ld=cfg.n_out, box_temperature=float(k["box_temperature"]))
    if c.samples is not None:
        s.update(clips=int(c.samples[0]), sample0=int(c.samples[1]))
    return s


def rollout_schedule(cfg, c, P, steps):
    """The launches of one LayoutEngine._rollout call from a prompt of P frames, in order, on vlg.engine.grow_schedule.  Each
    entry: stage ("frame i <launch>"), frame (i), family, entry, ops (pointer arguments by name, None = NULL), flags (projection
    calls), scalars (by header name; None: none recorded), kind + what its stage function takes.  Per generated frame: the
    encoder - the window ("window": step_stages.forward_launches on the current window buffer, through x[L]) or the cached step
    ("step": _step_launches) -, the head on frame t_read (vlg_head_frame while the window grows, vlg_head_last_frame at T-1 and on
    a compact stream, T = 1) and the decode launch: append at pos in place, or the slide into the other window buffer."""
    T, L = cfg.T, cfg.n_layers
    out, cur = [], 0
    sfx = c.decode_suffix
    for i, (encoder, t_read, pos) in enumerate(grow_schedule(P, T, steps, c.cached(P, T))):
        w, nw, tag, frame = "win%d" % cur, "win%d" % (cur ^ 1), "frame %d " % i, []
        valid = w + ".valid" if c.masked else None
        if encoder == "step":
            x, Tx, named = _step_launches(frame, cfg, c, tag, t_read, valid), 1, False
        else:
            SS.forward_launches(frame, cfg, c.base, tag, False, w + ".cls", w + ".box", valid, final=False)
            shapes = {"qkv": (3 * cfg.d, cfg.d), "proj": (cfg.d, cfg.d), "ff1": (cfg.d_ff, cfg.d), "ff2": (cfg.d, cfg.d_ff)}
            for e in frame:         # the scalars the trace records: T of the embedding, a projection's leading dimensions
                n, k = shapes.get(e["stage"].split(".")[-1], (0, 0))
                e["scalars"] = dict(T=T) if e["kind"] == "embed_fwd" else dict(lda=k, ldw=k, ldc=n) if e["kind"] == "linear_fwd" else None
            x, Tx, named = "x[%d]" % L, T, t_read < T - 1
        frame.append(dict(stage=tag + "head", kind="head", family="head_last", entry="vlg_head_frame" if named else "vlg_head_last_frame",
                          x=x, T=Tx, t_read=t_read if Tx == T else 0, i=i,
                          ops=(x, "p:lnf_g", "p:lnf_b", "p:head_w", "p:head_b", "logits[%d]" % i),
                          scalars=dict(T=Tx, t_read=t_read) if named else dict(T=Tx)))
        dec = dict(stage=tag + "decode", family="decode", i=i, pos=pos, win=w, scalars=decode_scalars(cfg, c, i, steps, pos))
        if pos is not None:
            frame.append(dict(dec, kind="decode_append", entry="vlg_layout_decode_append" + sfx,
                              ops=("logits[%d]" % i, w + ".cls", w + ".box", w + ".valid", "gen_cls", "gen_box", "grow.cls", "grow.box")))
        else:
            frame.append(dict(dec, kind="decode_slide", entry="vlg_layout_decode" + sfx, new=nw,
                              ops=("logits[%d]" % i, w + ".cls", w + ".box", nw + ".cls", nw + ".box", nw + ".valid", "gen_cls", "gen_box")))
            cur ^= 1
        for e in frame:
            e["frame"], e["encoder"] = i, encoder
        out += frame
    return out


# ------------------------------------------------------------------------------------------------ stage functions
def embed_step(cls_emb, box_w, box_b, time_emb, p, frame_cls, frame_box):
    """the embedding of ONE position: frame_cls (B,N), frame_box (B,N,4) with time_emb row p -> (B*N, d), rows (b, n)"""
    params = {"cls_emb": cls_emb, "box_w": box_w, "box_b": box_b, "time_emb": time_emb[p:p + 1]}
    return SS.to_rows(O.embed(params, frame_cls[:, None], frame_box[:, None].to(cls_emb.dtype)))


def _cache(qkv, B, T, N):
    """the [B*N*T, 3d] cache in the public (B,T,N,3d) order"""
    return SS.from_rows(qkv, B, T, N)


def slot_step(qkv, p, B, T, N, newest=True):
    """per-slot step: the query of position p against the keys of positions <= p of its own sequence (test_hip_attention_step._ref).
    newest False (a mutation): the keys of positions < p alone"""
    seq = qkv.view(B * N, T, -1)
    if not newest:      # the query of position p in the place of position p-1's: it then sees the keys 0 .. p-1
        d = qkv.shape[1] // 3
        seq = torch.cat([seq[:, :p - 1], torch.cat([seq[:, p:p + 1, :d], seq[:, p - 1:p, d:]], -1)], 1)
        p = p - 1
    return O.temporal_attention(seq[:, :p + 1].permute(1, 0, 2)[None], qkv.shape[1] // 192)[0, p]


def clip_step(qkv, valid, p, B, T, N):
    """per-clip step: every slot of the frames <= p under valid (clip_step_ref.step_ref) -> (B*N, d)"""
    from clip_step_ref import step_ref
    return step_ref(_cache(qkv, B, T, N), valid, p, qkv.dtype).reshape(B * N, -1)


def frame_step(qkv, valid, p, B, T, N):
    """frame step: frame p's own rows under frame_walk.visible (test_hip_frame_attention_step.frame_step_ref) -> (B*N, d)"""
    from test_hip_frame_attention_step import frame_step_ref
    return frame_step_ref(_cache(qkv, B, T, N), valid, p, qkv.dtype).reshape(B * N, -1)


def head_frame(x, gamma, beta, w, b, BN, T, t_read):
    """the head on frame t_read of a [BN*T, d] residual stream: test_hip_layout_decode._head_ref's arithmetic"""
    from test_hip_layout_decode import _head_ref
    return _head_ref(x, gamma, beta, w, b, torch.arange(BN) * T + t_read, x.dtype)


def decode_frame(cfg, c, logits, cls_hist, box_hist, step, **over):
    """the frame a decode launch draws from `logits` (B*N, n_out) and the history cls_hist (B,h,N) / box_hist whose last frame is
    the newest: decode_ref.next_frame, boxhead_ref.next_frame for a Gaussian head, samples_ref.next_frame for a pass of samples
    -> (classes (B,N) int64, boxes (B,N,4) float64, near (B,N)).  over: knobs a mutation changes (also clips, sample0)."""
    k = dict(c.knobs, **{n: v for n, v in over.items() if n in KNOBS})
    nc = cfg.n_classes
    if c.samples is not None:
        return samples_ref.next_frame(logits, cls_hist, box_hist, nc, step, k["temperature"], k["top_k"], k["seed"], k["keep_padded"],
                                      k["box_temperature"], over.get("clips", c.samples[0]), over.get("sample0", c.samples[1]))
    if c.gaussian:
        return boxhead_ref.next_frame(logits, cls_hist, box_hist, nc, step, k["temperature"], k["top_k"], k["seed"], k["keep_padded"],
                                      k["box_temperature"])
    return D.next_frame(logits[:, :nc + 4], cls_hist, box_hist, nc, step, k["temperature"], k["top_k"], k["seed"], k["keep_padded"])


def box_bar(c):
    """|box - rule| allowed: 1e-6 for sigmoid(raw) (test_hip_layout_decode), boxhead_ref.box_bar for a drawn box (test_hip_decode_box)"""
    tau = float(c.knobs["box_temperature"])
    return 1e-6 if tau == 0.0 else boxhead_ref.box_bar(tau)


def run_stage(e, cfg, c, B, N, val, detail=None):
    """One schedule entry of the encoder or the head on the values val(name) hands out -> {buffer name: unrounded tensor}.  The
    scattered q k v product comes back compact, (B*N, 3d), under the cache's name (entry["scatter"] = its position)."""
    T, k = cfg.T, e["kind"]
    rnd = SS.bf if c.round_operands else SS.ident
    if k in WINDOW_KINDS:
        return SS.run_stage(e, cfg, c.base, {"slot_class": torch.empty(B, T, N)}, val, detail)[0]
    if k == "embed_step":
        return {e["x"]: embed_step(val("p:cls_emb"), val("p:box_w"), val("p:box_b"), val("p:time_emb"), e["p"], val("grow.cls"), val("grow.box"))}
    if k == "ln_step":
        y, mean, rstd = SS.ln_fwd(val(e["x"]), val("p:" + e["g"]), val("p:" + e["g"][:-1] + "b"))
        return {"grow.h": y, "grow.stat.mean": mean, "grow.stat.rstd": rstd}
    if k == "linear_step":
        out, aux = SS.linear_fwd(val(e["a"]), val(c.weight(e["w"])), val("p:" + e["w"][:-1] + "b"), rnd,
                                 val(e["aux_in"]) if e["epi"] & SS.EPI_RESID else None, SS.epi_modes(e["epi"])[0])
        return {e["c"]: out} if aux is None else {e["c"]: out, e["aux_out"]: aux}
    if k == "slot_step":
        return {"grow.att": slot_step(val("qkv[%d]" % e["l"]), e["p"], B, T, N)}
    if k == "clip_step":
        return {"grow.att": clip_step(val("qkv[%d]" % e["l"]), val(e["valid"]), e["p"], B, T, N)}
    if k == "frame_step":
        return {"grow.att": frame_step(val("qkv[%d]" % e["l"]), val(e["valid"]), e["p"], B, T, N)}
    if k == "head":
        return {"logits[%d]" % e["i"]: head_frame(val(e["x"]), val("p:lnf_g"), val("p:lnf_b"), val("p:head_w"), val("p:head_b"), B * N, e["T"], e["t_read"])}
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------ the chain
def initial_window(cfg, prompt_cls, prompt_box):
    """the prompt rule (LayoutEngine._rollout): the prompt's frames, then the reserved id, zero boxes; valid = (class < n_classes)"""
    B, P, N = prompt_cls.shape
    cls = torch.full((B, cfg.T, N), cfg.n_classes, dtype=torch.int64)
    box = torch.zeros(B, cfg.T, N, 4)
    cls[:, :P], box[:, :P] = prompt_cls, prompt_box
    return cls, box, (cls < cfg.n_classes).float()


def scatter(full, compact, p, T, ld=None):
    """the strided store of a cached q k v launch: row r of `compact` into position p of cache row r (ldc = T*3d); ld: another
    leading dimension (a mutation)"""
    out, w = full.clone(), compact.shape[1]
    flat = out.view(-1)
    ld = T * w if ld is None else ld
    for r in range(compact.shape[0]):
        flat[p * w + r * ld:p * w + r * ld + w] = compact[r].to(out.dtype)
    return out


def emulate_rollout(cfg, c, params, prompt, steps, dtype, mutate=None, force=None, st=None, pass_index=0):
    """Chain the stage functions along rollout_schedule for one _rollout call from prompt = (cls (B,P,N), box (B,P,N,4)), storing
    as the contract says (bf16 buffers as torch.bfloat16, integers as they are, everything else in `dtype`) -> (records, state)
    in the format of rollout_trace.trace.  Free-running: every frame is drawn by the decoding rule, in fp64, from the chain's own
    logits; force = (gen_cls, gen_box) (B,steps,N[,4]) teacher-forces the frames instead.  In float64 this is the emulated
    oracle of the mode.  mutate(entry, val, outputs, record, run) may change what a launch leaves behind and what its record
    says (the checker's own test; run.cfg / run.c: the configuration and this pass's contract); it returns None or a dict of overrides of how the result is stored: scatter (position), ld,
    pos, slide_from, skip (names not stored).  run(entry) evaluates a (changed) entry.  st: the buffers a previous pass left."""
    pc, pb = prompt
    B, P, N = pc.shape
    T, nc, BN = cfg.T, cfg.n_classes, B * N
    if st is None:
        st = {"p:" + k: v.to(dtype) for k, v in params.items()}
        st.update({"pb:" + k: v.to(BF) for k, v in params.items()})
    st = dict(st)
    w0 = initial_window(cfg, pc, pb.to(dtype))
    st["win0.cls"], st["win0.box"], st["win0.valid"] = w0[0], w0[1].to(dtype), w0[2].to(dtype)
    for n, t in (("win1.cls", w0[0]), ("win1.box", st["win0.box"]), ("win1.valid", st["win0.valid"])):
        st.setdefault(n, torch.zeros_like(t))
    before = {n: st[n].clone() for n in st if n.startswith("win")}
    st["logits"] = torch.zeros(steps, BN, cfg.n_out, dtype=dtype)
    st["gen_cls"], st["gen_box"] = torch.zeros(B, steps, N, dtype=torch.int64), torch.zeros(B, steps, N, 4, dtype=dtype)
    val = lambda n: None if n is None else st[n].to(dtype) if st[n].is_floating_point() else st[n]
    store = lambda n, t: t if not t.is_floating_point() else t.to(BF if c.dtype(n) == BF else dtype)

    def run(e):
        return run_stage(e, cfg, c, B, N, val)

    run.cfg, run.c = cfg, c                                   # (what a mutation of a decode launch needs to draw the frame again)
    records, near_total = [], 0
    for e in rollout_schedule(cfg, c, P, steps):
        rec = dict(family=e["family"], name=e["entry"], flags=e.get("flags"), ops=e["ops"], scalars=None if e["scalars"] is None else dict(e["scalars"]))
        rec["pass"] = pass_index
        i = e["frame"]
        if e["kind"].startswith("decode"):
            w, pos = e["win"], e["pos"]
            h = T if pos is None else pos
            if force is not None:
                o = {"cls": force[0][:, i], "box": force[1][:, i].to(dtype), "near": torch.zeros(B, N, dtype=torch.bool)}
            else:
                fc, fb, near = decode_frame(cfg, c, st["logits"][i], st[w + ".cls"][:, :h], st[w + ".box"][:, :h], i)
                o = {"cls": fc, "box": fb.to(dtype), "near": near}
            ov = (mutate(e, val, o, rec, run) if mutate is not None else None) or {}
            near_total += int(o["near"].sum())
            fc, fb = o["cls"], o["box"].to(dtype)
            new = {"gen_cls": st["gen_cls"].clone(), "gen_box": st["gen_box"].clone()}
            new["gen_cls"][:, i], new["gen_box"][:, i] = fc, fb
            if pos is not None:
                pos = ov.get("pos", pos)
                new.update({w + ".cls": st[w + ".cls"].clone(), w + ".box": st[w + ".box"].clone(), w + ".valid": st[w + ".valid"].clone()})
                new[w + ".cls"][:, pos], new[w + ".box"][:, pos], new[w + ".valid"][:, pos] = fc, fb, (fc < nc).to(dtype)
                new["grow.cls"], new["grow.box"] = fc.clone(), fb.clone()
            else:
                nw, s0 = e["new"], ov.get("slide_from", 1)
                new[nw + ".cls"] = torch.cat([st[w + ".cls"][:, s0:s0 + T - 1], fc[:, None]], 1)
                new[nw + ".box"] = torch.cat([st[w + ".box"][:, s0:s0 + T - 1], fb[:, None]], 1)
                new[nw + ".valid"] = (new[nw + ".cls"] < nc).to(dtype)
            for n in ov.get("skip", ()):
                new.pop(n, None)
            st.update(new)
        else:
            o = run(e)
            ov = (mutate(e, val, o, rec, run) if mutate is not None else None) or {}
            for n, t in o.items():
                t = t.t if isinstance(t, SS.Raw) else store(n, t)
                if e.get("scatter") is not None and n == e["c"]:
                    t = scatter(st[n] if n in st else torch.zeros(BN * T, 3 * cfg.d, dtype=t.dtype), t, ov.get("scatter", e["scatter"]), T, ov.get("ld"))
                if n.startswith("logits["):
                    st["logits"] = st["logits"].clone()
                    st["logits"][i] = t
                else:
                    st[n] = t
        rec["after"] = {n.split("+")[0]: st[n.split("+")[0]] for n in e["ops"]
                        if n is not None and not n.startswith(("p:", "pb:", "logits", "gen_"))}
        records.append(rec)
    state = dict(st=st, passes=[dict(before=before, logits=st["logits"], gen_cls=st["gen_cls"], gen_box=st["gen_box"], B=B)],
                 params={k: v for k, v in st.items() if k.startswith(("p:", "pb:"))}, near=near_total)
    return records, state


def emulate_samples(cfg, c, params, prompt, steps, dtype, passes, mutate=None):
    """emulate_rollout for every pass of a rollout_samples call: passes = vlg.samples.sample_passes' list of (first sample, samples);
    the prompt is replicated sample-major, as the engine replicates it -> (records, state) with one entry of state["passes"] each."""
    pc, pb = prompt
    records, state, st = [], None, None
    for j, (first, k) in enumerate(passes):
        r, s = emulate_rollout(cfg, c.for_pass(pc.shape[0], first, k), params, (pc.repeat(k, 1, 1), pb.repeat(k, 1, 1, 1)), steps, dtype,
                               mutate, st=st, pass_index=j)
        st = s["params"]
        records += r
        if state is None:
            state = s
        else:
            state["passes"] += s["passes"]
            state["near"] += s["near"]
    return records, state
