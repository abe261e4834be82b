"""An independent statement of SAM's prompt encoder and mask decoder in plain torch, parametrised by dtype: written from the
operator's description (include/f3dgs.h), not from the reference's text.  W is {name: tensor} with the reference's
parameter names.  The prompt encoding and the dense positional encoding are float32 whatever the dtype, as the reference's are
(its encoder casts to float itself); the transformer, the upscaler and the heads run in `dtype`."""
import math

import numpy as np
import torch
import torch.nn.functional as F

PE = "prompt_encoder."
MD = "mask_decoder."
TWO_PI = 2 * np.pi


def as_torch(weights, device=None):
    return {k: torch.as_tensor(v, device=device) for k, v in weights.items()}


def _angles(W, xy):
    """xy (..., 2) float32 in [0, 1] -> the (..., 256) embedding [sin | cos] of 2 pi ((2 xy - 1) G)"""
    g = W[PE + "pe_layer.positional_encoding_gaussian_matrix"].float()
    a = TWO_PI * ((2 * xy - 1) @ g)
    return torch.cat([torch.sin(a), torch.cos(a)], -1)


def dense_pe(W, h, w):
    """(h w, 256) float32: the cell centres ((j + 0.5) / w, (i + 0.5) / h)"""
    y = (torch.arange(h, dtype=torch.float32) + 0.5) / h
    x = (torch.arange(w, dtype=torch.float32) + 0.5) / w
    xy = torch.stack([x[None, :].expand(h, w), y[:, None].expand(h, w)], -1)
    return _angles(W, xy).reshape(h * w, 256)


def sparse_tokens(W, coords, labels, boxes, input_size):
    """(B, n', 256) float32: the points (label 1 / 0: + point embedding 1 / 0; -1: not_a_point alone), then the pad point if no box
    is given, then the two box corners (+ point embeddings 2, 3).  coords (B, n, 2) pixels of the input image, or None."""
    ih, iw = input_size
    scale = torch.tensor([iw, ih], dtype=torch.float32)
    emb = lambda i: W[PE + f"point_embeddings.{i}.weight"].float()[0]
    nap = W[PE + "not_a_point_embed.weight"].float()[0]
    parts = []
    if coords is not None:
        coords, labels = torch.as_tensor(coords, dtype=torch.float32), torch.as_tensor(labels)
        e = _angles(W, (coords + 0.5) / scale)
        e = torch.where((labels == -1)[..., None], nap.expand_as(e), e)
        e = e + (labels == 0)[..., None] * emb(0) + (labels == 1)[..., None] * emb(1)
        parts.append(e)
        if boxes is None:
            parts.append(nap.expand(coords.shape[0], 1, 256))
    if boxes is not None:
        corners = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 2, 2)
        e = _angles(W, (corners + 0.5) / scale)
        parts.append(e + torch.stack([emb(2), emb(3)]))
    return torch.cat(parts, 1)


def _attention(W, prefix, q, k, v, info=None):
    lin = lambda x, n: x @ W[f"{prefix}.{n}.weight"].T + W[f"{prefix}.{n}.bias"]
    q, k, v = lin(q, "q_proj"), lin(k, "k_proj"), lin(v, "v_proj")
    heads = lambda x: x.reshape(x.shape[0], x.shape[1], 8, -1).transpose(1, 2)
    q, k, v = heads(q), heads(k), heads(v)
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if info is not None:
        info["max_score"] = max(info.get("max_score", 0.0), float(s.abs().max()))
    o = torch.softmax(s, -1) @ v
    return lin(o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1), "out_proj")


def _norm(W, prefix, x, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), W[prefix + ".weight"], W[prefix + ".bias"], eps)


def decode(weights, features, sparse, multimask, dtype=torch.float64, pe=None, device=None, want_info=True):
    """(low_res (B, m, 4h, 4w), iou (B, m), info) in `dtype`.  features (256, h, w), sparse (B, n', 256) the prompt tokens.
    info["max_score"]: the largest |score| of the token -> image attentions (a host read each; want_info=False leaves it out).
    device: where the chain runs (tools/sam_decoder_bench.py times it on the GPU); the positional encoding is made on the host."""
    W32 = as_torch(weights, device)
    W = {k: v.to(dtype) for k, v in W32.items()}
    features, sparse = torch.as_tensor(features, device=device), torch.as_tensor(sparse, device=device)
    C, h, w = features.shape
    B = sparse.shape[0]
    pe = (dense_pe({k: v.cpu() for k, v in W32.items() if "gaussian_matrix" in k}, h, w) if pe is None else torch.as_tensor(pe)).to(device=device, dtype=dtype)
    out_tokens = torch.cat([W[MD + "iou_token.weight"], W[MD + "mask_tokens.weight"]], 0)
    tokens = torch.cat([out_tokens[None].expand(B, -1, -1), sparse.to(dtype)], 1)
    src = (features.to(dtype) + W[PE + "no_mask_embed.weight"].reshape(256, 1, 1)).reshape(256, h * w).T
    keys = src[None].expand(B, -1, -1)
    queries, info = tokens, ({} if want_info else None)
    T = MD + "transformer."
    for l in range(2):
        p = f"{T}layers.{l}."
        if l == 0:
            queries = _attention(W, p + "self_attn", queries, queries, queries)
        else:
            q = queries + tokens
            queries = queries + _attention(W, p + "self_attn", q, q, queries)
        queries = _norm(W, p + "norm1", queries)
        queries = _norm(W, p + "norm2", queries + _attention(W, p + "cross_attn_token_to_image", queries + tokens, keys + pe, keys, info))
        hidden = torch.relu(queries @ W[p + "mlp.lin1.weight"].T + W[p + "mlp.lin1.bias"])
        queries = _norm(W, p + "norm3", queries + hidden @ W[p + "mlp.lin2.weight"].T + W[p + "mlp.lin2.bias"])
        keys = _norm(W, p + "norm4", keys + _attention(W, p + "cross_attn_image_to_token", keys + pe, queries + tokens, queries))
    queries = _norm(W, T + "norm_final_attn", queries + _attention(W, T + "final_attn_token_to_image", queries + tokens, keys + pe, keys, info))
    # upscaler: a 2x2 stride-2 transposed convolution places, for every input cell, a 2x2 block: out[o, 2i + a, 2j + b]
    up = MD + "output_upscaling."

    def conv_t(x, weight, bias):                       # x (B, hh, ww, Cin) -> (B, 2hh, 2ww, Cout)
        y = torch.einsum("bijc,couv->biujvo", x, weight) + bias
        return y.reshape(x.shape[0], 2 * x.shape[1], 2 * x.shape[2], -1)

    x = conv_t(keys.reshape(B, h, w, 256), W[up + "0.weight"], W[up + "0.bias"])
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    x = (x - mean) / torch.sqrt(var + 1e-6) * W[up + "1.weight"] + W[up + "1.bias"]
    x = F.gelu(x)
    x = F.gelu(conv_t(x, W[up + "3.weight"], W[up + "3.bias"]))          # (B, 4h, 4w, 32)

    def mlp(prefix, v):
        for i in range(3):
            v = v @ W[f"{prefix}.layers.{i}.weight"].T + W[f"{prefix}.layers.{i}.bias"]
            if i < 2:
                v = torch.relu(v)
        return v

    hyper = torch.stack([mlp(MD + f"output_hypernetworks_mlps.{i}", queries[:, 1 + i]) for i in range(4)], 1)      # (B, 4, 32)
    masks = torch.einsum("bmc,byxc->bmyx", hyper, x)
    iou = mlp(MD + "iou_prediction_head", queries[:, 0])
    sel = slice(1, 4) if multimask else slice(0, 1)
    return masks[:, sel], iou[:, sel], info
