"""The BiLSTM pose decoder's oracle, restatement and seeded fixture inputs (tests/test_host_bilstm.py, tests/test_gpu_bilstm.py,
tools/make_golden_bilstm.py).

`decoder_fp64` restates PoseDecoderBiLSTM (Contrastive_Stage/models/Generator.py:7-31, torch's nn.LSTM semantics) in numpy fp64.
`decoder_fp32_emulated` restates it in fp32 in the arithmetic order of csrc/dc_bilstm.hip: b_ih + b_hh folded (fp64, rounded once),
the input projection one k-ascending fma chain from 0 with the bias added behind it, the recurrence's chain seeded with that G and
running k = 0 .. 127, the head's layers as chains from 0 plus bias.  Neither is the code under test; both are independent of torch.
"""
import zlib

import numpy as np

H = 128
CASES = {128: (1, 2, 3, 30, 33, 150, 1800), 20: (1, 31, 150, 900), 7: (5,)}      # input size -> clip lengths (B = 2 each)
GENERATOR_CASES = ((30, 88), (150, 450))                                          # (T, Tm) of the full CNN-LSTM generator
B = 2
STORE_HIDDEN_T = 150                                                              # the fixture holds the reference's LSTM outputs up to here
FILES = {128: "g17_bilstm_in128.npz", 20: "g17_bilstm_in20.npz", 7: "g17_bilstm_in7.npz", "gen": "g17_bilstm_gen.npz"}
HIDDEN_FILES = {128: "g17_bilstm_in128_hidden.npz", 20: "g17_bilstm_in20_hidden.npz", 7: "g17_bilstm_in7_hidden.npz"}


def features(input_size, T, batch=B, seed=17):
    """The seeded decoder input fp32 [batch, T, input_size] of a case: standard normal draws that belong to (input size, T, clip)."""
    out = np.empty((batch, T, input_size), np.float32)
    for b in range(batch):
        g = np.random.default_rng([seed, input_size, T, b])
        out[b] = g.standard_normal((T, input_size)).astype(np.float32)
    return out


def digest(sd):
    """crc32 over every entry's bytes, in order: the fixture's check that the seeded weights are the ones it was made with."""
    c = 0
    for k, v in sd.items():
        c = zlib.crc32(np.ascontiguousarray(v).tobytes(), zlib.crc32(k.encode(), c))
    return c


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _name(leaf, layer, d):
    return f"LSTM.{leaf}_l{layer}" + ("_reverse" if d else "")


def lstm_fp64(sd, x, layers=2, gates=None, every=False):
    """nn.LSTM(In, 128, num_layers=2, bidirectional, batch_first) in eval mode with h0 = c0 = 0: x [B, T, In] -> [B, T, 256] fp64 after
    `layers` layers (`every`: the list of every layer's output).  `gates` (a list): receives every layer and direction's
    pre-activations [B, T, 512]."""
    x = np.asarray(x, np.float64)
    outs = []
    for layer in range(layers):
        Bn, T, _ = x.shape
        out = np.zeros((Bn, T, 2 * H))
        for d in range(2):
            wih, whh = (np.asarray(sd[_name(n, layer, d)], np.float64) for n in ("weight_ih", "weight_hh"))
            bias = np.asarray(sd[_name("bias_ih", layer, d)], np.float64) + np.asarray(sd[_name("bias_hh", layer, d)], np.float64)
            G = x @ wih.T + bias
            h, c = np.zeros((Bn, H)), np.zeros((Bn, H))
            pre = np.zeros((Bn, T, 4 * H))
            for s in range(T):
                t = T - 1 - s if d else s
                a = G[:, t] + h @ whh.T
                pre[:, t] = a
                i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
                c = _sig(f) * c + _sig(i) * np.tanh(g)
                h = _sig(o) * np.tanh(c)
                out[:, t, d * H:(d + 1) * H] = h
            if gates is not None:
                gates.append(pre)
        x = out
        outs.append(out)
    return outs if every else x


def head_fp64(sd, hid):
    y = np.asarray(hid, np.float64)
    for i in (0, 2):
        y = np.maximum(y @ np.asarray(sd[f"out.{i}.weight"], np.float64).T + np.asarray(sd[f"out.{i}.bias"], np.float64), 0.0)
    return _sig(y @ np.asarray(sd["out.4.weight"], np.float64).T + np.asarray(sd["out.4.bias"], np.float64))


def decoder_fp64(sd, x):
    """-> (poses [B, T, 26], LSTM output after layer 1, after layer 2), all fp64."""
    h1, h2 = lstm_fp64(sd, x, 2, every=True)
    return head_fp64(sd, h2), h1, h2


def _fma(a, w, x):
    """fl32(a + w x) with the product exact (fp64 holds a product of two fp32 exactly): one fused multiply-add step of a chain."""
    return (a.astype(np.float64) + w.astype(np.float64) * x.astype(np.float64)).astype(np.float32)


def _chain(x, W, bias=None, seed=None):
    """y[..., o] = (seed or 0) then fma over k ascending of W[o, k] x[..., k], then + bias: fp32 at every step."""
    x, W = np.asarray(x, np.float32), np.asarray(W, np.float32)
    a = np.zeros(x.shape[:-1] + (W.shape[0],), np.float32) if seed is None else seed.astype(np.float32)
    for k in range(W.shape[1]):
        a = _fma(a, W[:, k], x[..., k:k + 1])
    return a if bias is None else a + np.asarray(bias, np.float32)


def _sig32(x):
    return (np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def lstm_fp32_emulated(sd, x, layers=2, every=False):
    x = np.asarray(x, np.float32)
    outs = []
    for layer in range(layers):
        Bn, T, _ = x.shape
        G, whh = [], []
        for d in range(2):
            bias = (np.asarray(sd[_name("bias_ih", layer, d)], np.float64) + np.asarray(sd[_name("bias_hh", layer, d)], np.float64)).astype(np.float32)
            G.append(_chain(x, sd[_name("weight_ih", layer, d)], bias))
            whh.append(np.asarray(sd[_name("weight_hh", layer, d)], np.float32))
        whh = np.stack(whh)                                   # [2, 512, 128]
        h, c = np.zeros((2, Bn, H), np.float32), np.zeros((2, Bn, H), np.float32)
        out = np.zeros((Bn, T, 2 * H), np.float32)
        for s in range(T):
            a = np.stack([G[0][:, s], G[1][:, T - 1 - s]])    # [2, B, 512]: the chain's seed
            for k in range(H):
                a = _fma(a, whh[:, None, :, k], h[:, :, k:k + 1])
            i, f, g, o = a[..., :H], a[..., H:2 * H], a[..., 2 * H:3 * H], a[..., 3 * H:]
            c = _fma(_sig32(i) * np.tanh(g, dtype=np.float32), _sig32(f), c)
            h = _sig32(o) * np.tanh(c, dtype=np.float32)
            out[:, s, :H], out[:, T - 1 - s, H:] = h[0], h[1]
        x = out
        outs.append(out)
    return outs if every else x


def head_fp32_emulated(sd, hid):
    y = np.asarray(hid, np.float32)
    for i in (0, 2):
        y = np.maximum(_chain(y, sd[f"out.{i}.weight"], sd[f"out.{i}.bias"]), np.float32(0))
    return _sig32(_chain(y, sd["out.4.weight"], sd["out.4.bias"]))


def decoder_fp32_emulated(sd, x):
    """-> (poses, LSTM output after layer 1, after layer 2), fp32, in the kernels' arithmetic order."""
    h1, h2 = lstm_fp32_emulated(sd, x, 2, every=True)
    return head_fp32_emulated(sd, h2), h1, h2


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def case_key(T):
    return f"T{T}"
