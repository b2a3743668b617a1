"""fp64 restatements of the reference's CINLayer and XDeepFMRankingLayer (3.DCN/CustomLayers.py:308-417), written
twice so that the m*H_k + n ordering of the CIN weights is pinned by two independent readings:

  cin_numpy        einsum('bme,bne,mnh->bhe') with W_k reshaped [F, H_k, H_{k+1}]
  cin_torch_lines  a line-by-line transcription of CINLayer.call on torch-CPU: per-e matmul(X0, Xi^T), reshape
                   [E, B, F*H], transpose, width-1 conv1d, transpose
"""
import numpy as np
import torch


def cin_numpy(x0, Ws):
    """x0 [B,F,E], Ws: [(1, F*H_k, H_{k+1})] -> (cin_part [B, sum H], states [B, sum H, E]), fp64."""
    x0 = np.asarray(x0, np.float64)
    B, F, E = x0.shape
    xk, outs = x0, []
    for W in Ws:
        W = np.asarray(W, np.float64)
        Hk, Hn = xk.shape[1], W.shape[-1]
        xk = np.einsum("bme,bne,mnh->bhe", x0, xk, W.reshape(F, Hk, Hn))
        outs.append(xk)
    states = np.concatenate(outs, axis=1)
    return states.sum(axis=-1), states


def cin_torch_lines(inputs, cin_W):
    """CINLayer.call (3.DCN/CustomLayers.py:396-417) on torch tensors; differentiable."""
    embedding_dim = inputs.shape[-1]
    field_num = [inputs.shape[1]] + [w.shape[-1] for w in cin_W]
    res_list = [inputs]
    X0 = torch.split(inputs, 1, dim=-1)                       # E x [B, F, 1]
    for i, size in enumerate(field_num[1:]):
        Xi = torch.split(res_list[-1], 1, dim=-1)             # E x [B, H_i, 1]
        x = torch.stack([torch.matmul(a, b.transpose(1, 2)) for a, b in zip(X0, Xi)])   # [E, B, F, H_i]
        x = torch.reshape(x, (embedding_dim, -1, field_num[0] * field_num[i]))         # [E, B, F*H_i]
        x = x.permute(1, 0, 2)                                                          # [B, E, F*H_i]
        # tf.nn.conv1d(x, filters (1, F*H_i, H_{i+1}), stride 1, 'VALID'): channels-last, width-1 filter
        x = torch.nn.functional.conv1d(x.permute(0, 2, 1), cin_W[i][0].t().unsqueeze(-1)).permute(0, 2, 1)
        x = x.permute(0, 2, 1)                                                          # [B, H_{i+1}, E]
        res_list.append(x)
    res = torch.cat(res_list[1:], dim=1)
    return torch.sum(res, dim=-1)


def xdeepfm_forward(p, X, X_cont, act="relu"):
    """XDeepFMRankingLayer.call (3.DCN/CustomLayers.py:337-374) on torch-CPU fp64.  p: dict of tensors named like the
    layer's parameters (w, embed, dense_k[i], dense_b[i], cin_W[k], out_k, out_b); X [B,F] int64, X_cont [B,C]."""
    B = X.shape[0]
    linear_part = p["w"][X].sum(dim=1)                                   # [B,1]
    X_emb = p["embed"][X]                                                # [B,F,E]
    h = torch.cat([X_cont, X_emb.reshape(B, -1)], dim=1)
    for k, b in zip(p["dense_k"], p["dense_b"]):
        h = h @ k + b
        if act == "relu":
            h = torch.relu(h)
    cin_part = cin_torch_lines(X_emb, p["cin_W"])
    z = torch.cat([linear_part, h, cin_part], dim=1) @ p["out_k"] + p["out_b"]
    return torch.sigmoid(z)
