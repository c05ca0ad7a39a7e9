"""Plain float64 restatements of the operations behind the text-tower kernels (text.hip): causal multi-head attention
forward and backward, the column sums / LayerNorm parameter gradients, the token + position embedding and its dense
backward, and a numpy restatement of the host-side prompt index (Lt, the inverted index of the embedding gather).

Written from the operations' definitions (the scaled-dot-product core of nn.MultiheadAttention under CLIP's causal mask,
text_encoder.py:33-39; nn.Embedding; nn.LayerNorm's parameter gradients) and the layouts include/ebc_hip.h documents.
Everything is CPU float64 / numpy; each function takes the kernel's literal inputs."""
import numpy as np
import torch

F64 = torch.float64


def causal(L):
    """[L][L] bool, True on the support j <= i."""
    return torch.ones(L, L, dtype=torch.bool).tril()


def attention_causal_fwd(q, k, v):
    """o [B][H][L][64] = softmax over keys j <= i of (q k^T / 8) v, lse [B][H][L]; p is zero off the support."""
    L = q.shape[2]
    mask = causal(L)
    s = q @ k.transpose(-1, -2) / 8.0
    sm = s.masked_fill(~mask, float("-inf"))
    m = sm.max(-1, keepdim=True).values
    p = torch.exp(sm - m)
    l = p.sum(-1, keepdim=True)
    return {"o": (p @ v) / l, "lse": (m + torch.log(l)).squeeze(-1), "s": s, "m": m, "p": p, "l": l, "mask": mask}


def attention_causal_bwd(q, k, v, dout, out, lse):
    """The backward on the kernel's own inputs: P = exp(s - lse) on the support (0 off it), delta = rowsum(dout * out),
    dS = P (dP - delta), dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO."""
    L = q.shape[2]
    mask = causal(L)
    s = q @ k.transpose(-1, -2) / 8.0
    P = torch.exp(s - lse.to(F64)[..., None]) * mask
    delta = (dout * out).sum(-1)
    dP = dout @ v.transpose(-1, -2)
    dS = P * (dP - delta[..., None])
    return {"dq": dS @ k / 8.0, "dk": dS.transpose(-1, -2) @ q / 8.0, "dv": P.transpose(-1, -2) @ dout,
            "delta": delta, "P": P, "dP": dP, "dS": dS, "s": s, "mask": mask}


def ln_param_grad(dy, x, mean, rstd):
    """dgamma = sum_r dy xhat, dbeta = sum_r dy, xhat = (x - mean) rstd from the statistics handed over; also the
    terms."""
    t = dy.to(F64) * ((x.to(F64) - mean.to(F64)[:, None]) * rstd.to(F64)[:, None])
    return {"dgamma": t.sum(0), "dbeta": dy.to(F64).sum(0), "terms": t}


def embed_fwd(tok, pos, ids):
    """x [NB][Lt][D] = tok[ids] + pos[:Lt]."""
    return tok[ids.long()] + pos[:ids.shape[1]]


def embed_bwd(dx, ids, vocab, context):
    """Dense dtok [vocab][D] and dpos [context][D] of dx [NB][Lt][D] (float64), with the sums of absolute terms."""
    NB, Lt, D = dx.shape
    dx = dx.to(F64)
    dtok = torch.zeros(vocab, D, dtype=F64)
    atok = torch.zeros(vocab, D, dtype=F64)
    flat = ids.reshape(-1).long()
    dtok.index_add_(0, flat, dx.reshape(-1, D))
    atok.index_add_(0, flat, dx.reshape(-1, D).abs())
    dpos = torch.zeros(context, D, dtype=F64)
    apos = torch.zeros(context, D, dtype=F64)
    dpos[:Lt] = dx.sum(0)
    apos[:Lt] = dx.abs().sum(0)
    count = torch.bincount(flat, minlength=vocab)
    return {"dtok": dtok, "atok": atok, "dpos": dpos, "apos": apos, "count": count}


def inverted_index(ids):
    """The inverted index of the gather ids.reshape(-1): uniq ascending, offs [nu + 1], rows = for each unique id the
    positions holding it, ascending."""
    flat = np.asarray(ids).reshape(-1)
    uniq = np.unique(flat)
    rows, offs = [], [0]
    for u in uniq:
        r = np.nonzero(flat == u)[0]
        rows.extend(int(x) for x in r)
        offs.append(len(rows))
    return {"uniq": uniq.astype(np.int32), "offs": np.asarray(offs, np.int32), "rows": np.asarray(rows, np.int32)}


def prompt_index(tokens):
    """numpy restatement of ebc_amd.text.prompt_index: tokens [NB][context] int -> eot [NB] (argmax of each row: the
    EOT token carries the largest id, text_encoder.py:52), Lt = max eot + 1, ids = tokens[:, :Lt] and their inverted
    index."""
    tokens = np.asarray(tokens)
    eot = tokens.argmax(1)
    Lt = int(eot.max()) + 1
    ids = tokens[:, :Lt]
    return {"eot": eot.astype(np.int32), "Lt": Lt, "ids": np.ascontiguousarray(ids).astype(np.int32), **inverted_index(ids)}
