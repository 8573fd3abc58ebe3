"""CPU restatement of the Gaussian box head in fp64 (include/vlg_hip.h, "Gaussian box head" and the box rule of
vlg_layout_decode_ext; DESIGN.md "Gaussian box head"): the negative log-likelihood with its closed-form gradient, and the
sampled boxes of decoding.  Plain module: test infrastructure, nothing collected.  THE yardstick of the new kernels.

Definition, for head-output row m = (b*N + n)*T + t with its target at (b, t, n) and C classes:
    mu_k = sigmoid(out[m, C+k])   (a CONSTANT: no gradient to the mean)      g_k = sigmoid(out[m, C+4+k])
    s_k = S_MIN + (S_MAX - S_MIN) g_k,  sigma_k = exp(s_k)                   e_k = (tgt_k - mu_k) exp(-s_k)
    nll_m = 1/4 sum_k (e_k^2 / 2 + s_k + ln(2 pi) / 2)                       cover_m = 1/4 sum_k [|tgt_k - mu_k| <= sigma_k]
    cnt = max(sum valid, 1);  box_nll = 1/cnt sum_m valid_m nll_m;  box_cover likewise
    dout[m, C+4+k] = w_nll valid_m/cnt 1/4 (1 - e_k^2) (S_MAX - S_MIN) g_k (1 - g_k);  every other column 0
Box rule of decoding: tau == 0: sigmoid(raw mean).  tau > 0: (x0..x3) = Philox4x32-10 on counter (token, step, 5, 0);
u_i = (x_i >> 8) * 2^-24 + 2^-25 evaluated in FP32 (rounds above 2^23; may give 1.0), then fp64: z0 = sqrt(-2 ln u0)
cos(2 pi u1), z1 = ... sin(2 pi u1), z2, z3 from u2, u3;  box_k = clamp(mu_k + tau sigma_k z_k, 0, 1)."""
import math

import numpy as np
import torch

import decode_ref
import philox_ref as P

S_MIN, S_MAX = -7.0, 0.0                 # vlg.spec.BOX_S_MIN / BOX_S_MAX (the CPU test checks they agree)
BOX_STREAM = P.BOX_NORMAL                # the Philox counter's third word of the box draw
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
EPS32 = 2.0 ** -24                       # half an fp32 ulp at 1


def rows_of(x, B, T, N):
    """a (B,T,N,...) tensor in the public order -> (B*N*T, ...) in the row order m = (b*N + n)*T + t"""
    x = x.view(B, T, N, -1).permute(0, 2, 1, 3)
    return x.reshape(B * N * T, -1)


def nll_terms(out, tgt_box, valid, B, T, N, C, s_min=S_MIN, s_max=S_MAX):
    """out (M, ld), tgt_box (B,T,N,4), valid (B,T,N), any float dtype -> fp64 per-row terms (dict of (M,4) / (M,) tensors).
    Differentiable in out: autograd of box_nll() below IS the definition's gradient."""
    o = out.double()
    tg, w = rows_of(tgt_box.double(), B, T, N), rows_of(valid.double(), B, T, N)[:, 0]
    mu = torch.sigmoid(o[:, C:C + 4]).detach()
    g = torch.sigmoid(o[:, C + 4:C + 8])
    s = s_min + (s_max - s_min) * g
    e = (tg - mu) * torch.exp(-s)
    nll = 0.25 * (0.5 * e * e + s + HALF_LOG_2PI).sum(dim=1)
    cover = 0.25 * ((tg - mu).abs() <= torch.exp(s)).double().sum(dim=1)
    cnt = max(float(w.sum()), 1.0)
    return dict(mu=mu, g=g, s=s, e=e, nll=nll, cover=cover, w=w, cnt=cnt, df=tg - mu)


def box_nll(out, tgt_box, valid, B, T, N, C, s_min=S_MIN, s_max=S_MAX):
    """(box_nll, box_cover) as fp64 scalars (box_nll differentiable in out)"""
    t = nll_terms(out, tgt_box, valid, B, T, N, C, s_min, s_max)
    return (t["w"] * t["nll"]).sum() / t["cnt"], (t["w"] * t["cover"]).sum() / t["cnt"]


def box_nll_closed(out, tgt_box, valid, B, T, N, C, w_nll=1.0, s_min=S_MIN, s_max=S_MAX):
    """the closed form the kernel evaluates -> dict(nll, cover, dscale (M,4) = dout[:, C+4:C+8], and the error scales below)"""
    with torch.no_grad():
        t = nll_terms(out, tgt_box, valid, B, T, N, C, s_min, s_max)
        e2 = t["e"] ** 2
        x = out.double()[:, C + 4:C + 8]
        gg = torch.sigmoid(x) * torch.sigmoid(-x)         # g (1 - g) without the cancellation of 1 - g at large |x|
        coef = (w_nll * t["w"] / t["cnt"] * 0.25)[:, None] * (s_max - s_min) * gg
        inv_sigma = torch.exp(-t["s"])
        # what one fp32 rounding of mu (|mu| <= 1), of e and of e^2 moves: d(e^2) ~ (1 + e^2 + 2 |e| / sigma) * 2^-24
        cond = 1.0 + e2 + 2.0 * t["e"].abs() * inv_sigma
        return dict(nll=(t["w"] * t["nll"]).sum() / t["cnt"], cover=(t["w"] * t["cover"]).sum() / t["cnt"],
                    dscale=coef * (1.0 - e2), grad_unit=coef * cond * EPS32,
                    nll_unit=float((t["w"][:, None] * 0.25 * (0.5 * cond + t["s"].abs() + 1.0)).sum() / t["cnt"]) * EPS32,
                    # coordinates whose coverage flag an fp32 evaluation may decide differently
                    cover_near=int((t["w"][:, None] * ((t["df"].abs() - torch.exp(t["s"])).abs() <= 8 * EPS32)).sum()),
                    cnt=t["cnt"])


# ---- bars of the NLL kernel (DESIGN.md "Gaussian box head" records the measured maxima behind them) --------------------
# error of dout[:, C+4:C+8] in units of grad_unit, of box_nll in units of nll_unit: 4 x the largest seen on the GPU over the
# cases of tests/test_hip_box_nll.py and tests/test_hip_boxhead_step.py (largest seen: 5.92 units at 40 000 tokens for the
# gradient - about 3 fp32 ulp of its conditioning, the expected floor - and 0.50 for box_nll)
GRAD_BAR_UNITS = 24.0
NLL_BAR_UNITS = 2.0


def check_nll(got_dscale, got_nll, got_cover, ref, what=""):
    """the bars: gradient RELATIVE to |1 - e^2|'s own conditioning (grad_unit), scalars likewise; returns the measured maxima"""
    err = (got_dscale.double().cpu() - ref["dscale"]).abs()
    unit = ref["grad_unit"]
    ratio = float((err / unit.clamp_min(1e-300))[unit > 0].max()) if bool((unit > 0).any()) else 0.0
    zero_ok = bool((err[unit == 0] == 0).all())
    nll_ratio = abs(float(got_nll) - float(ref["nll"])) / max(ref["nll_unit"], 1e-300) if ref["nll_unit"] > 0 else abs(float(got_nll))
    cover_err = abs(float(got_cover) - float(ref["cover"]))
    print("box_nll %s: gradient error %.3f units, nll error %.3f units, cover error %.3g (near-boundary coordinates %d)"
          % (what, ratio, nll_ratio, cover_err, ref["cover_near"]))
    assert zero_ok, "%s: a gradient that must be exactly 0 is not" % what
    assert ratio <= GRAD_BAR_UNITS, "%s: gradient off by %.3f units of its conditioning (bar %g)" % (what, ratio, GRAD_BAR_UNITS)
    assert nll_ratio <= NLL_BAR_UNITS, "%s: box_nll off by %.3f units (bar %g)" % (what, nll_ratio, NLL_BAR_UNITS)
    # coverage counts flags: a coordinate within 8 * 2^-24 of its boundary may fall either way, the rest is a sum of quarters
    assert cover_err <= 0.25 * ref["cover_near"] / ref["cnt"] + 16 * EPS32, \
        "%s: box_cover %r vs %r" % (what, float(got_cover), float(ref["cover"]))
    return ratio, nll_ratio


# ---- sampled boxes ---------------------------------------------------------------------------------------------------------
uniforms32 = P.unit32   # u of Philox words as the kernels form it: fp32 arithmetic, as float64


def normals(tokens, step, seed):
    """(R, 4) float64: z0..z3 of every token index in `tokens` at `step` under `seed`"""
    return normals_of_words(P.words(tokens, step, BOX_STREAM, seed))


def normals_of_words(x):
    u = [uniforms32(w) for w in x]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def sampled_boxes(out_last, n_classes, step, box_temperature, seed, s_min=S_MIN, s_max=S_MAX):
    """out_last (R, >= C+8) rows [logits | raw mean | raw scale | ...], row r = token r -> boxes (R, 4) float64.
    The temperature is the fp32 value a kernel is handed."""
    o = out_last.detach().cpu().double()
    C = n_classes
    mu = torch.sigmoid(o[:, C:C + 4])
    if box_temperature == 0:
        return mu
    sigma = torch.exp(s_min + (s_max - s_min) * torch.sigmoid(o[:, C + 4:C + 8]))
    z = torch.from_numpy(normals(np.arange(o.shape[0]), step, seed))
    return (mu + float(np.float32(box_temperature)) * sigma * z).clamp(0.0, 1.0)


def box_bar(box_temperature):
    """|box - reference| allowed: fp32 Box-Muller against fp64 on the same u differs by at most 1.9e-6 (1.6e7 draws),
    sigma <= 1, the sigmoid adds ~1e-7 and the clamp is continuous"""
    return 1e-5 * max(1.0, float(box_temperature))


def next_frame(out_last, cls_in, box_in, n_classes, step, temperature=0.0, top_k=0, seed=0, keep_padded=False,
               box_temperature=0.0):
    """decode_ref.next_frame for rows with a scale: out_last (B*N, ld >= C+4; >= C+8 with box_temperature > 0).  The class is
    decode_ref's draw on the logits, untouched by the box draw; kept slots keep their box."""
    B, T, N = cls_in.shape
    cls, _, near = decode_ref.next_frame(out_last[:, :n_classes + 4], cls_in, box_in, n_classes, step, temperature, top_k, seed,
                                         keep_padded)
    box = sampled_boxes(out_last, n_classes, step, box_temperature, seed).view(B, N, 4)
    if keep_padded:
        pad = cls_in[:, -1] >= n_classes
        box = torch.where(pad[..., None], box_in[:, -1].double(), box)
    return cls, box, near
