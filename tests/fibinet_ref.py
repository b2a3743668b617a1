"""fp64 restatements of the reference's FiBiNet interaction (3.DCN/CustomLayers.py:888-1011), written twice so that the
pair order, the weight each pair uses and the dnn_in column layout are pinned by two independent readings:

  fibinet_numpy   einsum per pair on the SENet identity A_i A_j p_ij (numpy, values only)
  fibinet_torch   the reference's op order on torch-CPU (differentiable): SENet applied to the inputs (:968-981), split,
                  tensordot, multiply, concat per bilinear pass (:1000-1011), then the concat of both passes, Flatten
                  and the concat with X_cont (:946-948)
Weights: S0 [F,mid], S1 [mid,F]; Ws a list of [E,E] in parameter order (1 / F-1 / P for 'all' / 'each' /
'interaction').
"""
import itertools

import numpy as np
import torch


def pairs(F):
    return list(itertools.combinations(range(F), 2))


def weight_of(bilinear_type, k, i):
    """Index into Ws of pair k = (i, j) (:1003-1008)."""
    return {"all": 0, "each": i, "interaction": k}[bilinear_type]


def senet_numpy(x, S0, S1):
    Z = x.mean(axis=-1)
    H1 = np.maximum(Z @ S0, 0.0)
    return np.maximum(H1 @ S1, 0.0), H1


def fibinet_numpy(x, x_cont, S0, S1, Ws, bilinear_type):
    """-> dnn_in [B, 2PE + C] (fp64)."""
    x = np.asarray(x, np.float64)
    B, F, E = x.shape
    A, _ = senet_numpy(x, np.asarray(S0, np.float64), np.asarray(S1, np.float64))
    raw, sen = [], []
    for k, (i, j) in enumerate(pairs(F)):
        Wk = np.asarray(Ws[weight_of(bilinear_type, k, i)], np.float64)
        p = np.einsum("bd,de,be->be", x[:, i], Wk, x[:, j])
        raw.append(p)
        sen.append(A[:, i:i + 1] * A[:, j:j + 1] * p)
    return np.concatenate(raw + sen + [np.asarray(x_cont, np.float64).reshape(B, -1)], axis=1)


def senet_torch(inputs, S0, S1):
    """SENetLayer.call (:975-981): Z = reduce_mean(inputs, -1), A = MLPLayer([mid, F], relu, no bias)(Z),
    V = inputs * expand_dims(A, 2)."""
    Z = torch.mean(inputs, dim=-1)
    A = torch.relu(torch.relu(Z @ S0) @ S1)
    return inputs * A.unsqueeze(2)


def bilinear_torch(inputs, Ws, bilinear_type):
    """BilinearInteractionLayer.call (:1000-1011)."""
    F = inputs.shape[1]
    field_list = torch.split(inputs, 1, dim=1)                     # F x [B,1,E]
    p = []
    for k, (i, j) in enumerate(itertools.combinations(range(F), 2)):
        w = Ws[weight_of(bilinear_type, k, i)]
        p.append(torch.tensordot(field_list[i], w, dims=([2], [0])) * field_list[j])
    return torch.cat(p, dim=1)                                     # [B,P,E]


def fibinet_torch(x_emb, x_cont, S0, S1, Ws, bilinear_type):
    """FiBiNetLayer.call (:941-948) up to dnn_input: differentiable in x_emb, S0, S1 and Ws."""
    senet_output = senet_torch(x_emb, S0, S1)
    raw = bilinear_torch(x_emb, Ws, bilinear_type)
    sen = bilinear_torch(senet_output, Ws, bilinear_type)
    dnn_input = torch.cat([raw, sen], dim=1).reshape(x_emb.shape[0], -1)
    return torch.cat([dnn_input, x_cont.reshape(x_emb.shape[0], -1)], dim=1)


def fibinet_layer_torch(p, X, X_cont, bilinear_type, act="relu"):
    """The whole FiBiNetLayer.call on torch-CPU fp64.  p: embed, S0, S1, Ws, dnn_k[i], dnn_b[i], out_k, out_b."""
    X_emb = p["embed"][X]
    h = fibinet_torch(X_emb, X_cont, p["S0"], p["S1"], p["Ws"], bilinear_type)
    for k, b in zip(p["dnn_k"], p["dnn_b"]):
        h = h @ k + b
        if act == "relu":
            h = torch.relu(h)
    return torch.sigmoid(h @ p["out_k"] + p["out_b"])
