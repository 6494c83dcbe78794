"""Plain-torch references of the individual ops (test infrastructure only; run on the GPU for speed): fp32 for attention
(ref_attention), float64 for the row ops (ref_ln_fwd, ref_ln_bwd, ref_ce, ref_adam, ref_gelu / ref_dgelu), each computed from
the very input bits the kernel gets (fp32 and bf16 inputs widened, never re-rounded)."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def bf(x):
    """round-trip through bf16 (so kernel and reference see identical operand values)"""
    return x.to(torch.bfloat16).float()


def ref_attention(q, k, v, pk, pq, relidx, mask, scale, drop_keep=None):
    """q,k,v: [B,nh,S,64] fp32; pk,pq: [nh,R,64]; relidx int64 [2S-1]; mask [B,S] 0/1.
    Returns ctx [B,nh,S,64], lse [B,nh,S] (SURVEY App. C formula)."""
    B, nh, S, d = q.shape
    i = torch.arange(S, device=q.device)
    idx = relidx.long()[(i[:, None] - i[None, :]) + S - 1]  # [S,S]
    c2p = torch.einsum("bhid,hrd->bhir", q, pk)  # [B,nh,S,R]
    c2p = torch.gather(c2p, 3, idx[None, None].expand(B, nh, S, S))
    p2c = torch.einsum("bhjd,hrd->bhjr", k, pq)  # [B,nh,S(j),R]
    p2c = torch.gather(p2c, 3, idx.t()[None, None].expand(B, nh, S, S)).transpose(2, 3)  # [b,h,i,j] = KPQ[j, idx(i,j)]
    s = (torch.einsum("bhid,bhjd->bhij", q, k) + c2p + p2c) * scale
    m = mask.bool()
    m2 = m[:, None, :, None] & m[:, None, None, :]
    s = s.masked_fill(~m2, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)
    p = torch.where(m2, p, torch.zeros_like(p))
    p = torch.nan_to_num(p, nan=0.0)
    if drop_keep is not None:
        p = p * drop_keep
    return torch.einsum("bhij,bhjd->bhid", p, v), lse


def heads(x, B, S, nh):
    """[B*S, nh*64] -> [B,nh,S,64]"""
    return x.view(B, S, nh, 64).permute(0, 2, 1, 3)


def unheads(x):
    B, nh, S, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, nh * d)


def stats(name, got, ref):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    return (f"{name}: max_abs_err={err.max().item():.3e} mean_abs_err={err.mean().item():.3e} "
            f"ref_absmax={ref.abs().max().item():.3e} ref_std={ref.std().item():.3e}")


# ------------------------------------------------------------------------------------------------ float64 row-op references
def ref_ln_fwd(*, y=None, keep=None, r_plain=None, r_norm=None, gamma, beta, eps, rowmask=None):
    """fbl_ln_fwd in float64: t = dropout(y) + r_plain + LN_r(r_t) * r_rowmask, out = LN(t) * rowmask.
    keep: multiplicative dropout mask of y (0 or 1/(1-p)); r_norm = (t, stats [N,2] = (mean, rstd), gamma, beta, rowmask|None).
    Returns dict(t, mean, rstd, out, ax) -- ax = sum of the magnitudes of t's addends (what one fp32 rounding of t scales with)."""
    t, ax = 0.0, 0.0
    if y is not None:
        a = y.double() * (keep.double() if keep is not None else 1.0)
        t, ax = t + a, ax + a.abs()
    if r_plain is not None:
        t, ax = t + r_plain.double(), ax + r_plain.double().abs()
    if r_norm is not None:
        rt, rs, rg, rb, rm = r_norm
        st = rs.double()
        m = rm.double()[:, None] if rm is not None else 1.0
        t = t + ((rt.double() - st[:, :1]) * st[:, 1:] * rg.double()[None] + rb.double()[None]) * m
        ax = ax + ((rt.double().abs() + st[:, :1].abs()) * st[:, 1:].abs() * rg.double().abs()[None] + rb.double().abs()[None]) * m
    H = t.shape[1]
    mean = t.sum(1, keepdim=True) / H
    var = ((t - mean) ** 2).sum(1, keepdim=True) / H
    rstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    om = rowmask.double()[:, None] if rowmask is not None else 1.0
    out = ((t - mean) * rstd * gamma.double()[None] + beta.double()[None]) * om
    return dict(t=t, mean=mean[:, 0], rstd=rstd[:, 0], out=out, ax=ax)


def ref_ln_materialize(t, stats, gamma, beta, rowmask=None, add_bcast=None, S=1):
    """fbl_ln_materialize in float64 from the given t / stats bits; returns (out, mag) -- mag: magnitudes of the terms"""
    st = stats.double()
    om = rowmask.double()[:, None] if rowmask is not None else 1.0
    c = (t.double() - st[:, :1]) * st[:, 1:] * gamma.double()[None]
    out = (c + beta.double()[None]) * om
    mag = ((t.double().abs() + st[:, :1].abs()) * st[:, 1:].abs() * gamma.double().abs()[None] + beta.double().abs()[None]) * om
    if add_bcast is not None:
        p = add_bcast.double()[torch.arange(t.shape[0], device=t.device) % S]
        out, mag = out + p, mag + p.abs()
    return out, mag + out.abs()


def ref_ln_bwd(dout, t, stats, gamma, rowmask=None, keep=None):
    """fbl_ln_bwd in float64 from the given (t, stats) bits.  Returns dict: dt, dy (= dt * keep), the per-row terms of the
    three column sums (tg = dout*mask*xhat, tb = dout*mask, dy), and mag = rstd * (|g| + mean|g| + |xhat| mean|g xhat|), the scale of dt."""
    st = stats.double()
    mean, rstd = st[:, :1], st[:, 1:]
    om = rowmask.double()[:, None] if rowmask is not None else 1.0
    dd = dout.double() * om
    xh = (t.double() - mean) * rstd
    g = dd * gamma.double()[None]
    H = t.shape[1]
    s1 = g.sum(1, keepdim=True) / H
    s2 = (g * xh).sum(1, keepdim=True) / H
    dt = rstd * (g - s1 - xh * s2)
    dy = dt * keep.double() if keep is not None else dt
    # (the means of |g| and |g xhat|, not |s1| and |s2|: a row sum that cancels is still only as good as the sum of its magnitudes)
    mag = rstd.abs() * (g.abs() + g.abs().sum(1, keepdim=True) / H + xh.abs() * (g * xh).abs().sum(1, keepdim=True) / H)
    return dict(dt=dt, dy=dy, tg=dd * xh, tb=dd, mag=mag, xh=xh)


def ref_ce(logits, labels):
    """float64 cross entropy of logits [N, V] (the V real columns) with ignore label < 0.
    Returns dict(lse [N], p [N, V] softmax, terms [N] = lse - logit[label] (0 on ignored rows), count)"""
    x = logits.double()
    lse = torch.logsumexp(x, 1)
    lab = labels.long()
    on = lab >= 0
    xl = x.gather(1, lab.clamp(min=0)[:, None])[:, 0]
    terms = torch.where(on, lse - xl, torch.zeros_like(lse))
    return dict(lse=lse, x=x, terms=terms, count=int(on.sum()), on=on)


def ref_adam(p, g, m, v, *, lr, b1, b2, eps, wd, step, clip):
    """one fbl_adam_flat step in float64 (torch.optim.Adam's formula, L2 weight decay folded into the gradient); in place"""
    gi = g * clip
    if wd != 0.0:
        gi = gi + wd * p
    m.mul_(b1).add_(gi, alpha=1.0 - b1)
    v.mul_(b2).add_(gi * gi, alpha=1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p.sub_((lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)))


def ref_gelu(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ref_dgelu(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
