"""Plain-torch statements of the PCTDM block (reference infer_module/pctdm_infer_module.py), any dtype, autograd: shared by
tests/test_pctdm_cpu.py (float64, against the fixtures) and tests/test_gpu_pctdm.py (float64 and float32, against the kernels).  Written
from the definitions, not from the kernels: an LSTM with gate order i, f, g, o and zero initial state; the second direction walks from the
last position and its outputs are stored at the positions they belong to; max over the two direction halves; softmax inside each team."""
import torch

H, I = 1000, 1024


def lstm(pre, w_hh, variant=None):
    """pre [R, S, D, 4H] (input projection, biases included), w_hh [D, 4H, H] -> (h [R, S, D*H], cells [R, S, D, H], gates [R, S, D, 4H])"""
    R, S, D, h4 = pre.shape
    h = h4 // 4
    outs, cells, gates = [], [], []
    for d in range(D):
        hs, cs, gs = [None] * S, [None] * S, [None] * S
        hv = pre.new_zeros((R, h))
        cv = pre.new_zeros((R, h))
        order = range(S) if d == 0 else range(S - 1, -1, -1)
        for k, pos in enumerate(order):
            z = pre[:, pos, d] + hv @ w_hh[d].t()
            a, b, c, o = z[:, :h], z[:, h:2 * h], z[:, 2 * h:3 * h], z[:, 3 * h:]
            if variant == "gate_order_igfo":
                b, c = c, b
            gi, gf, gg, go = torch.sigmoid(a), torch.sigmoid(b), torch.tanh(c), torch.sigmoid(o)
            cv = gf * cv + gi * gg
            hv = go * torch.tanh(cv)
            slot = k if (variant == "reverse_not_realigned" and d == 1) else pos
            hs[slot], cs[slot], gs[slot] = hv, cv, torch.cat([gi, gf, gg, go], -1)
        outs.append(torch.stack(hs, 1))
        cells.append(torch.stack(cs, 1))
        gates.append(torch.stack(gs, 1))
    return torch.cat(outs, -1), torch.stack(cells, 2), torch.stack(gates, 2)


def pool(lstm_out, variant=None):
    """lstm_out [G, N, 2H] -> (pooled [G, N, H], winner bool [G, N, H], context [G, H])"""
    G, N, h2 = lstm_out.shape
    h = h2 // 2
    a, b = lstm_out[..., :h], lstm_out[..., h:]
    if variant == "max_over_adjacent_players":                              # what "MaxPool2d((2, 1)) over the players" would be
        both = torch.maximum(lstm_out[:, 0::2], lstm_out[:, 1::2])           # [G, N/2, 2H] -> the reference's shape again
        pooled = both.reshape(G, N, h)
        return pooled, None, pooled.mean(1)
    pooled = torch.maximum(a, b)
    return pooled, b > a, pooled.mean(1)


def attention(pooled, src, ctx, w_e, b_e, variant=None):
    """-> (y [G, N, H], gamma [G, N]); w_e [H], b_e scalar tensor"""
    G, N, h = pooled.shape
    score = torch.tanh(src + ctx[:, None]) @ w_e + b_e
    if variant == "softmax_over_all_players":
        gamma = torch.softmax(score, -1)
    else:
        gamma = torch.softmax(score.reshape(G, 2, N // 2), -1).reshape(G, N)
    if variant == "no_residual":
        return pooled * gamma[..., None], gamma
    return pooled + pooled * gamma[..., None], gamma


def module(p, x, variant=None):
    """the whole block: p = state dict of PCTDM (any dtype), x [B, T, N, 1024] -> dict of every stage; out [B*T, 2000]"""
    B, T, N, _ = x.shape
    G = B * T
    xs = x.reshape(G, N, -1)
    pre = torch.stack([xs @ p["Bi_Lstm.weight_ih_l0" + s].t() + p["Bi_Lstm.bias_ih_l0" + s] + p["Bi_Lstm.bias_hh_l0" + s]
                       for s in ("", "_reverse")], 2)
    w_hh = torch.stack([p["Bi_Lstm.weight_hh_l0"], p["Bi_Lstm.weight_hh_l0_reverse"]], 0)
    lstm_out, _, gates = lstm(pre, w_hh, variant)
    pooled, winner, context = pool(lstm_out, variant)
    src = pooled @ p["att_source_weights.0.weight"].t() + p["att_source_weights.0.bias"]
    ctx = context @ p["att_context_weights.0.weight"].t() + p["att_context_weights.0.bias"]
    y, gamma = attention(pooled, src, ctx, p["att_extra_weights.0.weight"][0], p["att_extra_weights.0.bias"][0], variant)
    y2 = y.reshape(2 * G, N // 2, -1)
    pre2 = (y2 @ p["Intra_Group_LSTM.weight_ih_l0"].t() + p["Intra_Group_LSTM.bias_ih_l0"] + p["Intra_Group_LSTM.bias_hh_l0"])[:, :, None]
    feas, _, gates2 = lstm(pre2, p["Intra_Group_LSTM.weight_hh_l0"][None], "gate_order_igfo" if variant == "gate_order_igfo" else None)
    last = feas[:, 0 if variant == "last_step_from_first_position" else -1]
    return dict(out=last.reshape(G, -1), lstm_out=lstm_out, pooled=pooled, winner=winner, gamma=gamma, gates=gates, gates2=gates2)
