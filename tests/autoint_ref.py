"""Restatements of the reference's TransformerAttentionLayer / AutoIntLayer (3.DCN/CustomLayers.py:1012-1139) for the
AutoInt tests.

* ``attention_numpy``: an fp64 numpy reading.  Head h takes the columns [h d, (h+1) d) by slicing, the softmax runs over
  the batch axis with the max subtracted, the residual and the ReLU follow.
* ``attention_einsum``: the same reading in torch (einsum per head), for its autograd gradients.
* ``attention_torch``: a transcription in the reference's op order -- tensordot, split/stack, matmul, softmax on axis 1,
  matmul, split/concat/squeeze, residual, ReLU -- runnable in any dtype (fp64 is the tests' reference, fp32 measures
  what a float32 evaluation of the same ops loses).
* ``attention_keyaxis``: the "obvious" reading with the softmax over the keys j, which the reference does NOT compute;
  the tests use it to show that their inputs can tell the two apart.
* ``autoint_layer_torch``: the whole AutoIntLayer: embedding lookup, continuous fields last, the attention layers,
  Flatten, MLPLayer (relu), Dense(1, sigmoid).
"""
import numpy as np
import torch


def attention_numpy(X, Wq, Wk, Wv, H, res=1, Wres=None, scaling=False):
    """X [B,F,E] -> (y, o): o = attention before the residual, y = relu(o (+ X | + X Wres)).  res 0 / 1 / 2."""
    X = np.asarray(X, np.float64)
    B, F, E = X.shape
    d = E // H
    Q, K, V = X @ Wq, X @ Wk, X @ Wv
    o = np.zeros_like(X)
    for h in range(H):
        cols = slice(h * d, (h + 1) * d)
        S = np.einsum("bic,bjc->bij", Q[:, :, cols], K[:, :, cols])
        if scaling:
            S = S / np.sqrt(d)
        S = S - S.max(axis=0, keepdims=True)                 # softmax over the BATCH axis
        P = np.exp(S)
        P /= P.sum(axis=0, keepdims=True)
        o[:, :, cols] = np.einsum("bij,bjc->bic", P, V[:, :, cols])
    z = o + (X if res == 1 else (X @ Wres if res == 2 else 0.0))
    return np.maximum(z, 0.0), o


def attention_einsum(X, Wq, Wk, Wv, H, res=1, Wres=None, scaling=False, return_o=False):
    B, F, E = X.shape
    d = E // H
    Q, K, V = X @ Wq, X @ Wk, X @ Wv
    outs = []
    for h in range(H):
        cols = slice(h * d, (h + 1) * d)
        S = torch.einsum("bic,bjc->bij", Q[:, :, cols], K[:, :, cols])
        if scaling:
            S = S / np.sqrt(d)
        P = torch.exp(S - S.max(dim=0, keepdim=True).values)
        P = P / P.sum(dim=0, keepdim=True)
        outs.append(torch.einsum("bij,bjc->bic", P, V[:, :, cols]))
    o = torch.cat(outs, dim=-1)
    z = o + (X if res == 1 else (X @ Wres if res == 2 else 0.0))
    return (torch.relu(z), o) if return_o else torch.relu(z)


def attention_torch(X, Wq, Wk, Wv, H, use_res=True, res_learnable=False, Wres=None, scaling=False, return_o=False):
    """3.DCN/CustomLayers.py:1035-1067 op for op."""
    querys = torch.tensordot(X, Wq, dims=([-1], [0]))
    keys = torch.tensordot(X, Wk, dims=([-1], [0]))
    values = torch.tensordot(X, Wv, dims=([-1], [0]))
    querys = torch.stack(torch.split(querys, X.shape[-1] // H, dim=-1))       # tf.split(x, H, -1): H equal parts
    keys = torch.stack(torch.split(keys, X.shape[-1] // H, dim=-1))
    values = torch.stack(torch.split(values, X.shape[-1] // H, dim=-1))
    inner = torch.matmul(querys, keys.transpose(-1, -2))                      # (H, B, F, F)
    if scaling:
        inner = inner / (X.shape[-1] // H) ** 0.5
    scores = torch.softmax(inner, dim=1)                                      # axis 1: the batch axis
    result = torch.matmul(scores, values)
    result = torch.cat(torch.split(result, 1, dim=0), dim=-1)                 # tf.split(result, H) along axis 0
    result = torch.squeeze(result, 0)
    o = result
    if use_res and res_learnable:
        result = result + torch.tensordot(X, Wres, dims=([-1], [0]))
    elif use_res and not res_learnable:
        result = result + X
    result = torch.relu(result)
    return (result, o) if return_o else result


def attention_keyaxis(X, Wq, Wk, Wv, H, scaling=False):
    """The per-example reading softmax(axis=-1) (over the keys); returns o before the residual."""
    querys = torch.stack(torch.split(X @ Wq, X.shape[-1] // H, dim=-1))
    keys = torch.stack(torch.split(X @ Wk, X.shape[-1] // H, dim=-1))
    values = torch.stack(torch.split(X @ Wv, X.shape[-1] // H, dim=-1))
    inner = torch.matmul(querys, keys.transpose(-1, -2))
    if scaling:
        inner = inner / (X.shape[-1] // H) ** 0.5
    result = torch.matmul(torch.softmax(inner, dim=-1), values)
    return torch.squeeze(torch.cat(torch.split(result, 1, dim=0), dim=-1), 0)


def assemble(embed, X_cate, cemb, X_cont):
    """3.DCN/CustomLayers.py:1119-1125: concat[embedding(X_cate), cemb[None] * X_cont[..., None]] on axis 1."""
    X_cate_emb = embed[X_cate]
    if X_cont is None or X_cont.shape[1] == 0:
        return X_cate_emb
    X_cont_emb = cemb.unsqueeze(0) * X_cont.unsqueeze(-1)
    return torch.cat([X_cate_emb, X_cont_emb], dim=1)


def assemble_dense(x_cate_emb, cemb, X_cont):
    """The same concatenation from already gathered categorical rows [B,Fc,E]."""
    if X_cont is None or X_cont.shape[1] == 0:
        return x_cate_emb
    return torch.cat([x_cate_emb, cemb.unsqueeze(0) * X_cont.unsqueeze(-1)], dim=1)


def assemble_np(args):
    """fp64 X [B,F,E] from the tests' (x_cate_emb, x_cont, cemb, ...) tuple."""
    x, xc, ce = (np.asarray(a, np.float64) for a in args[:3])
    return np.concatenate([x, ce[None] * xc[:, :, None]], axis=1)


def autoint_layer_torch(p, X_cate, X_cont, num_heads=2, scaling=False):
    """p: embed [V,E], cemb [C,E], att: list of (Wq, Wk, Wv), dnn_k / dnn_b lists, out_k, out_b -> sigmoid [B,1]."""
    x = assemble(p["embed"], X_cate, p["cemb"], X_cont)
    for Wq, Wk, Wv in p["att"]:
        x = attention_torch(x, Wq, Wk, Wv, num_heads, scaling=scaling)
    h = x.reshape(x.shape[0], -1)                                             # Flatten
    for k, b in zip(p["dnn_k"], p["dnn_b"]):
        h = torch.relu(h @ k + b)
    return torch.sigmoid(h @ p["out_k"] + p["out_b"])


def reference_main_input():
    """The input of AutoIntLayer's docstring example (3.DCN/CustomLayers.py:1073-1080): ids 0 .. 29 in ten columns,
    three continuous columns."""
    names = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
    X_cate = np.arange(30, dtype=np.int64).reshape(10, 3).T.copy()             # column k = [3k, 3k+1, 3k+2]
    X_cont = np.array([[0.2, 5.3, -3.8], [7.8, 1.2, -19.6], [4.9, 8.0, 4.2]])
    return names, X_cate, X_cont
