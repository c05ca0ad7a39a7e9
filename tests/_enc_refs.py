"""Plain float64 restatements of the operations behind the encoder-side kernels: LayerNorm with the row map
(vit_misc.hip), multi-head attention (attention.hip) and the blockwise similarity head (head.hip), and the input
generators of tests/test_gpu_encoder_kernels.py.

Written from the operations' definitions (nn.LayerNorm, nn.MultiheadAttention's scaled-dot-product core, F.normalize /
softmax / expectation) and from the layouts include/ebc_hip.h documents.  tests/test_enc_refs_cpu.py pins them to
torch's own float64 ops and autograd, and checks that every generator stays inside its stated condition.  Everything
here is CPU float64; each function takes the kernel's literal inputs (16-bit operands widened to float64)."""
import math

import torch

F64 = torch.float64
HD = 64                     # attention head dim


def rounded(x, dt):
    """x rounded once to dtype dt, widened back to float64."""
    return x.to(dt).to(F64)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_rows(M, rpg, gstride, goff):
    """Source row of dense row r: (r // rpg) * gstride + goff + r % rpg; rpg <= 0 is the identity."""
    r = torch.arange(M)
    if rpg <= 0:
        return r
    return (r // rpg) * gstride + goff + r % rpg


def layernorm_fwd(x, gamma, beta, M, rpg, gstride, goff, eps):
    """Dense y [M][D], mean [M], rstd [M] of the mapped rows of x (biased variance as the mean squared deviation)."""
    xs = x.to(F64)[ln_rows(M, rpg, gstride, goff)]
    mean = xs.mean(1)
    var = ((xs - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (xs - mean[:, None]) * rstd[:, None] * gamma.to(F64) + beta.to(F64)
    return {"y": y, "mean": mean, "rstd": rstd, "var": var, "xs": xs}


def layernorm_bwd(dy, x, mean, rstd, gamma, dx_in, M, rpg, gstride, goff, dx_out0):
    """dx = dx_in + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma, xhat = (x - mean) * rstd, from the
    statistics the kernel is handed.  dy, mean and rstd are dense (row r); x and dx_in are read, and the result written,
    at the mapped row.  Returns a copy of dx_out0 with the mapped rows replaced (every other row untouched) and the
    intermediate terms the error bound is built from (dense rows)."""
    rows = ln_rows(M, rpg, gstride, goff)
    xs = x.to(F64)[rows]
    g = dy.to(F64)[:M] * gamma.to(F64)
    xh = (xs - mean.to(F64)[:M, None]) * rstd.to(F64)[:M, None]
    s1 = g.mean(1, keepdim=True)
    s2 = (g * xh).mean(1, keepdim=True)
    core = rstd.to(F64)[:M, None] * (g - s1 - xh * s2)
    din = dx_in.to(F64)[rows] if dx_in is not None else torch.zeros_like(core)
    out = dx_out0.to(F64).clone()
    out[rows] = core + din
    return {"dx": out, "rows": rows, "g": g, "xh": xh, "s1": s1, "s2": s2, "din": din, "dense": core + din}


# ------------------------------------------------------------------------------------------------ attention
def split_qkv(qkv, B, L, H):
    """packed [B*L][3*H*64] -> q, k, v, each [B][H][L][64] (float64)."""
    t = qkv.to(F64).view(B, L, 3, H, HD).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def heads(x, B, L, H):
    """[B*L][H*64] -> [B][H][L][64]."""
    return x.to(F64).view(B, L, H, HD).permute(0, 2, 1, 3)


def unheads(x):
    """[B][H][L][64] -> [B*L][H*64]."""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * HD)


def pack_qkv(q, k, v):
    """q, k, v [B][H][L][64] -> packed [B*L][3*H*64]."""
    B, H, L, _ = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * HD)


def attention_fwd(q, k, v):
    """o [B][H][L][64] = softmax(q k^T / 8) v and lse [B][H][L] = log sum exp of the scaled scores."""
    s = q @ k.transpose(-1, -2) / 8.0
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    return {"o": (p @ v) / l, "lse": (m + torch.log(l)).squeeze(-1), "s": s, "m": m, "p": p, "l": l}


def attention_bwd(q, k, v, dout, out, lse):
    """The backward restated on the kernel's own inputs: P = exp(s - lse), delta = rowsum(dout * out),
    dS = P (dP - delta), dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO.  All [B][H][L][.]."""
    s = q @ k.transpose(-1, -2) / 8.0
    P = torch.exp(s - lse.to(F64)[..., None])
    delta = (dout * out).sum(-1)
    dP = dout @ v.transpose(-1, -2)
    dS = P * (dP - delta[..., None])
    return {"dq": dS @ k / 8.0, "dk": dS.transpose(-1, -2) @ q / 8.0, "dv": P.transpose(-1, -2) @ dout,
            "delta": delta, "P": P, "dP": dP, "dS": dS, "s": s}


# --- attention input generators
def hadamard(n):
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def selection_codes():
    """128 codes of 64 entries +-4: the rows of the 64 x 64 Hadamard matrix and their negatives.  code_a . code_b is
    1024 (a = b), -1024 (a = b +- 64) or 0."""
    h = 4.0 * hadamard(64)
    return torch.cat([h, -h], 0)


def selection_inputs(B, L, H, seed):
    """Selection inputs.  Key j of (crop b, head h) has the index a = (j + 5 h + 11 b) % 128 and is the sum of two
    codes, code[a] + code[next(a)] (entries 0 or +-8; next(a) is the following code of the same sign), so it scores
    128 after the 1/8 scale with the queries carrying either code, and 0 or -128 with every other one.  Query i carries
    the single code of index (37 i + 3 h + 7 b) % 128 (L < 128: the index of key (37 i + 3 h + 7 b) % L), so it attends
    to m keys, two different ones in every 128: exp(0 - 128) is 2^-184.7, below the smallest f32 denormal, so every
    other probability is exactly 0 in every dtype and the m keys get 1 / m each.  The matching keys differ, so
    dQ = sum_j dS_j k_j / 8 does not cancel.  37 is coprime to 128 and to every L < 128 used: the queries of one (crop,
    head) put a maximum on every key position.  Values and dout have 4 entries of +-1 a row, the rest 0.
    Returns packed qkv [B*L][3*H*64], dout [B*L][H*64] and mult [B][H][L], the m of each query."""
    g = torch.Generator().manual_seed(seed)
    codes = selection_codes()
    j = torch.arange(L)
    q = torch.empty(B, H, L, HD, dtype=F64)
    k = torch.empty(B, H, L, HD, dtype=F64)
    for b in range(B):
        for h in range(H):
            a = (j + 5 * h + 11 * b) % 128
            k[b, h] = codes[a] + codes[(a + 1) % 64 + 64 * (a // 64)]
            t = 37 * j + 3 * h + 7 * b
            q[b, h] = codes[a[t % L]] if L < 128 else codes[t % 128]
    mult = ((q @ k.transpose(-1, -2)) == 1024.0).sum(-1)

    def sparse(shape):
        x = torch.zeros(shape, dtype=F64)
        pos = torch.rand(shape, generator=g).argsort(-1)[..., :4]
        x.scatter_(-1, pos, torch.randint(0, 2, pos.shape, generator=g).to(F64) * 2 - 1)
        return x
    v, dout = sparse((B, H, L, HD)), sparse((B, H, L, HD))
    return pack_qkv(q, k, v), unheads(dout), mult


def selection_reference(q, k, v, dout, mult):
    """The attention of selection inputs with every probability below 2^-149 set to exactly 0, which is what every
    dtype computes: P = 1 / m on the m keys that score 128, and the forward / backward of that P.  Sums of a few dyadic
    terms throughout: exact in float64."""
    s = q @ k.transpose(-1, -2) / 8.0
    P = (s == 128.0).to(F64) / mult[..., None].to(F64)
    o = P @ v
    delta = (dout * o).sum(-1)
    dS = P * (dout @ v.transpose(-1, -2) - delta[..., None])
    return {"o": o, "lse": 128.0 + torch.log(mult.to(F64)), "P": P, "dS": dS, "delta": delta, "dq": dS @ k / 8.0,
            "dk": dS.transpose(-1, -2) @ q / 8.0, "dv": P.transpose(-1, -2) @ dout}


def drift_inputs(B, L, H, kind, seed):
    """Peaked / drifting softmax inputs, q, k, v [B][H][L][64], all inside the f16 range.

    Base: q, k normal with std 0.5 in dims 16..63 and 0 in dims 0..15 (scores of std ~0.2), v normal.  On top of it
      "rising"   q[0] = 8 and k_j[0] = level(block(j)): the score of key j gains level, 30 more from each block of
                 keys to the next (block = 256 keys, the streamed kernels' chunk; 64 keys when L <= 256).  A last block
                 of fewer than 16 keys gains 4 instead of 30, so that no row collapses onto one key.
      "falling"  the same levels in reverse order.
      "peak"     key t0 + c of the last (partial) 16-key tile carries 5 * Hadamard16[c] in dims 0..15, key c of the
                 first tile 3.5 * Hadamard16[c], every other key 0; query i carries Hadamard16[i % n_last].  Its one
                 dominant key, in the last partial tile, gains 5 * 16 / 8 = 10, one runner-up in the first tile 7.
    """
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, HD, generator=g, dtype=F64) * 0.5
    k = torch.randn(B, H, L, HD, generator=g, dtype=F64) * 0.5
    v = torch.randn(B, H, L, HD, generator=g, dtype=F64) * 1.5
    q[..., :16] = 0
    k[..., :16] = 0
    j = torch.arange(L)
    if kind in ("rising", "falling"):
        blk = 256 if L > 256 else 64
        nblk = -(-L // blk)
        level = [0.0]
        for c in range(1, nblk):
            short = c == nblk - 1 and L - c * blk < 16
            level.append(level[-1] + (4.0 if short else 30.0))
        level = torch.tensor(level, dtype=F64)
        if kind == "falling":
            level = level.flip(0)
        q[..., 0] = 8.0
        k[..., 0] = level[j // blk]
    elif kind == "peak":
        t0 = 16 * ((L - 1) // 16)
        n_last = L - t0
        assert t0 >= 16
        h16 = hadamard(16)
        k[..., :16, :16] = 3.5 * h16
        k[..., t0:, :16] = 5.0 * h16[:n_last]
        q[..., :16] = h16[j % n_last]
    else:
        raise ValueError(kind)
    return q, k, v


# ------------------------------------------------------------------------------------------------ head
def head_fwd(Z, text, logit_scale, anchors, B, HW):
    """logits [B][NB][HW] = exp(logit_scale) * normalize(Z) . normalize(text) (F.normalize: x / max(||x||, 1e-12)),
    exp [B][HW] = sum_k softmax_k(logits) * anchors_k, and the per-pixel terms the backward and the bounds use."""
    Z, text, anchors = Z.to(F64), text.to(F64), anchors.to(F64)
    nrm = torch.sqrt((Z * Z).sum(1))
    den = torch.clamp(nrm, min=1e-12)
    zn = Z / den[:, None]
    tn = text / torch.clamp(torch.sqrt((text * text).sum(1)), min=1e-12)[:, None]
    s = math.exp(float(logit_scale))
    lg = s * (zn @ tn.t())                                     # [P][NB]
    mx = lg.max(1, keepdim=True).values
    pe = torch.exp(lg - mx)
    pr = pe / pe.sum(1, keepdim=True)
    e = (pr * anchors).sum(1)
    NB = text.shape[0]
    return {"logits": lg.view(B, HW, NB).permute(0, 2, 1).contiguous(), "exp": e.view(B, HW), "lg": lg, "pr": pr, "e": e,
            "zn": zn, "tn": tn, "nrm": nrm, "den": den, "s": s}


def head_bwd(Z, text, logit_scale, anchors, dlogits, dexp, gscale, B, HW):
    """dZ [P][embed], dbias = column sums of dZ, dscale = d / d logit_scale, for the upstream gradients dlogits
    [B][NB][HW], dexp [B][HW], both scaled by gscale.  F.normalize backward: dz = (dzn - zn <zn, dzn>) / ||z||, and
    dzn / 1e-12 where the norm is clamped."""
    f = head_fwd(Z, text, logit_scale, anchors, B, HW)
    NB = text.shape[0]
    anchors = anchors.to(F64)
    dlg = dlogits.to(F64).view(B, NB, HW).permute(0, 2, 1).reshape(B * HW, NB) * gscale
    de = dexp.to(F64).reshape(B * HW, 1) * gscale
    dl = dlg + de * f["pr"] * (anchors - f["e"][:, None])
    dzn = f["s"] * (dl @ f["tn"])
    clamped = f["nrm"] <= 1e-12
    dot = torch.where(clamped, torch.zeros_like(f["nrm"]), (f["zn"] * dzn).sum(1))
    dz = (dzn - f["zn"] * dot[:, None]) / f["den"][:, None]
    f.update({"dz": dz, "dbias": dz.sum(0), "dscale": (dl * f["lg"]).sum(), "dl": dl, "dlg": dlg, "de": de, "dzn": dzn,
              "dot": dot})
    return f
