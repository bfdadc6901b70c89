#!/usr/bin/env python3
"""Generate tests/golden/g17_bilstm*.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_bilstm.py [reference Contrastive_Stage dir]     (default: beside oracle/make_golden.py's REF; ~2 min)

What it does
  1. imports the reference's Contrastive_Stage/models/Generator.py on the CPU;
  2. loads the seeded synthetic weights with load_state_dict(strict=True) into PoseDecoderBiLSTM(In, 26) for In = 128, 20 and 7
     (synthetic.synthetic_bilstm_state_dict), into Generator_CVPR_LSTM (the In = 20 weights under `lstm.`) and into a Generator whose
     `tcn` is replaced by PoseDecoderBiLSTM(128, 26) (synthetic.synthetic_m2sgan_bilstm_state_dict), eval();
  3. stores the reference's fp32 poses of every case of tests/helpers_bilstm.py (CASES, GENERATOR_CASES; inputs regenerated from
     their seeds by the tests) and, for T <= 150, its LSTM outputs after one layer (a one-layer nn.LSTM with the layer-0 weights)
     and after both, in files of their own (fp32 noise does not compress; every file stays under the 1 MiB limit);
  4. stores per case `ref_vs_fp64` and `emul_vs_fp64` for the poses, the hidden states after layer 1 and after layer 2: the max-abs
     deviation of the reference's fp32 values and of the fp32 restatement in the kernels' arithmetic order
     (helpers_bilstm.decoder_fp32_emulated) from the fp64 oracle (helpers_bilstm.decoder_fp64) - two independent fp32 evaluations
     of the same recurrence, the unit of the GPU tests' tolerance.  For the full generator the restatement follows the kernels in the
     features too: their music half comes from the reference's MusicEncoder run in the arithmetic of the split format that the
     generator's handle pins (`split_format_encoder`: operands as hi + lo of two bf16 values, three products per term);
  5. asserts, on the reference alone, that a test on this fixture can fail (see `can_fail`).

The files pin the weights by key list, shapes and a digest.  Only data is written; no reference source text is copied.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def tt(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def bf16_split(t):
    """t ~ hi + lo, two bf16 values (16 significant bits): how csrc/dc_music.hip's split format holds an operand."""
    hi = t.to(torch.bfloat16).to(t.dtype)
    return hi, (t - hi).to(torch.bfloat16).to(t.dtype)


class SplitConv(torch.nn.Module):
    """A convolution of the reference's MusicEncoder with the eval-mode BatchNorm behind it, in the split format's arithmetic: the
    BatchNorm folded into the weights (fp64, rounded once), weights and input each as hi + lo of two bf16 values, the product as
    hi hi + lo hi + hi lo (three products per term, lo lo dropped), sums in fp32."""

    def __init__(self, conv, bn):
        super().__init__()
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = conv.weight.double() * s.reshape(-1, *([1] * (conv.weight.dim() - 1)))
        self.conv = conv
        self.wh, self.wl = bf16_split(w.float())
        self.bias = ((conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()).float()

    def forward(self, x):
        xh, xl = bf16_split(x)
        f = self.conv._conv_forward
        return f(xh, self.wh, self.bias) + f(xl, self.wh, None) + f(xh, self.wl, None)


def split_format_encoder(enc):
    """A copy of the reference's MusicEncoder `enc` (fp32, eval) that computes in the split format of csrc/dc_music.hip, the format the
    generator's handle pins: every convolution a SplitConv, every activation a layer reads or adds as its residual held as hi + lo."""
    import copy
    enc = copy.deepcopy(enc)
    layers = [m for m in enc.modules() if type(m).__name__ == "Conv2dResLayer"]
    assert len(layers) == 7
    for m in layers:
        m.conv2d_layer[0], m.conv2d_layer[1] = SplitConv(m.conv2d_layer[0], m.conv2d_layer[1]), torch.nn.Identity()
        if isinstance(m.residual, torch.nn.Sequential):
            m.residual[0], m.residual[1] = SplitConv(m.residual[0], m.residual[1]), torch.nn.Identity()
        m.register_forward_pre_hook(lambda mod, args: (sum(bf16_split(args[0])),))
    enc.conv4[0], enc.conv4[1] = SplitConv(enc.conv4[0], enc.conv4[1]), torch.nn.Identity()
    return enc


def can_fail(L, ref_mod, sd, input_size):
    """Asserted on the reference module alone, at T = 30 (B = 2)."""
    x = torch.from_numpy(L.features(input_size, 30))
    with torch.no_grad():
        pose = ref_mod(x).numpy()
        assert pose.min() < 0.2 and pose.max() > 0.8, (pose.min(), pose.max())
        # every gate: pre-activations of both signs on at least 10 % of (frame, unit) pairs (fp64 restatement of the same weights)
        gates = []
        L.lstm_fp64(sd, x.numpy(), 2, gates)
        for pre in gates:
            for q in range(4):
                a = pre[..., q * L.H:(q + 1) * L.H]
                assert (a > 0).mean() >= 0.1 and (a < 0).mean() >= 0.1, (q, (a > 0).mean())
        # the recurrence matters
        import copy
        cut = copy.deepcopy(ref_mod)
        for n, p in cut.LSTM.named_parameters():
            if n.startswith("weight_hh"):
                p.zero_()
        assert np.abs(cut(x).numpy() - pose).max() > 1e-2
        # both directions reach the far end of the clip
        xl, xf = x.clone(), x.clone()
        xl[:, -1] += 1.0
        xf[:, 0] += 1.0
        back, fwd = np.abs(ref_mod(xl).numpy()[:, 0] - pose[:, 0]).max(), np.abs(ref_mod(xf).numpy()[:, -1] - pose[:, -1]).max()
        assert back > 1e-3 and fwd > 1e-3, (back, fwd)
        # time reversal of the input is not time reversal of the output (the two directions have weights of their own)
        rev = ref_mod(torch.flip(x, dims=[1])).numpy()
        assert np.abs(rev[:, ::-1] - pose).max() > 1e-2
    return float(pose.min()), float(pose.max()), float(back), float(fwd)


def main():
    from oracle.make_golden import REF
    import helpers_bilstm as L
    import helpers_m2sgan as HG
    from diffusion_conductor_amd.generator import bilstm_shapes, m2sgan_bilstm_shapes
    from diffusion_conductor_amd.synthetic import synthetic_bilstm_state_dict, synthetic_m2sgan_bilstm_state_dict
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(REF)), "Contrastive_Stage")
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    sys.path.insert(0, ref)
    warnings.filterwarnings("ignore", category=FutureWarning)
    warnings.filterwarnings("ignore", category=UserWarning)
    from models.Generator import Generator, Generator_CVPR_LSTM, PoseDecoderBiLSTM
    torch.set_num_threads(8)

    def devs(sd, x, pose32, h1_32, h2_32):
        p64, a64, b64 = L.decoder_fp64(sd, x)
        pe, ae, be = L.decoder_fp32_emulated(sd, x)
        return (np.array([L.max_abs(pose32, p64), L.max_abs(h1_32, a64), L.max_abs(h2_32, b64)]),
                np.array([L.max_abs(pe, p64), L.max_abs(ae, a64), L.max_abs(be, b64)]))

    for input_size, lengths in L.CASES.items():
        sd = synthetic_bilstm_state_dict(0, input_size)
        net = PoseDecoderBiLSTM(input_size, 26)
        net.load_state_dict(tt(sd), strict=True)
        net.eval()
        keys = list(net.state_dict().keys())
        assert keys == list(bilstm_shapes(input_size)), "param spec order differs from the reference module's"
        assert [tuple(v.shape) for v in net.state_dict().values()] == list(bilstm_shapes(input_size).values())
        one = torch.nn.LSTM(input_size, 128, num_layers=1, bidirectional=True, batch_first=True)
        one.load_state_dict({k[5:]: v for k, v in tt(sd).items() if "_l0" in k}, strict=True)
        out = {"keys": np.array(keys), "shapes": np.array([str(tuple(v.shape)) for v in net.state_dict().values()]),
               "weight_digest": np.int64(L.digest(sd)), "lengths": np.array(lengths)}
        hid = {}
        if input_size != 7:
            out["can_fail"] = np.array(can_fail(L, net, sd, input_size))
        for T in lengths:
            x = L.features(input_size, T)
            with torch.no_grad():
                pose = net(torch.from_numpy(x)).numpy()
                h2 = net.LSTM(torch.from_numpy(x))[0].numpy()
                h1 = one(torch.from_numpy(x))[0].numpy()
            assert pose.shape == (L.B, T, 26) and pose.dtype == np.float32
            n = L.case_key(T)
            out[f"pose_{n}"] = pose
            if T <= L.STORE_HIDDEN_T:
                hid[f"hidden1_{n}"], hid[f"hidden2_{n}"] = h1, h2
            out[f"ref_vs_fp64_{n}"], out[f"emul_vs_fp64_{n}"] = devs(sd, x, pose, h1, h2)
            print(f"In={input_size} T={T}: ref_vs_fp64 {out[f'ref_vs_fp64_{n}']}  emul_vs_fp64 {out[f'emul_vs_fp64_{n}']}", flush=True)
        if input_size == 20:                                   # Generator_CVPR_LSTM is this decoder under `lstm.`
            g = Generator_CVPR_LSTM()
            g.load_state_dict({"lstm." + k: v for k, v in tt(sd).items()}, strict=True)
            g.eval()
            out["cvpr_keys"] = np.array(list(g.state_dict().keys()))
            x = L.features(20, 31)
            with torch.no_grad():
                assert np.array_equal(g(torch.from_numpy(x), None).numpy().reshape(L.B, 31, 26), out["pose_T31"])
        np.savez(os.path.join(GOLDEN, L.FILES[input_size]), **out)
        np.savez(os.path.join(GOLDEN, L.HIDDEN_FILES[input_size]), **hid)

    # the CNN-LSTM baseline: Generator with self.tcn = PoseDecoderBiLSTM(128, 26) (Generator.py:58)
    sd = synthetic_m2sgan_bilstm_state_dict(0)
    net = Generator()
    net.tcn = PoseDecoderBiLSTM(128, 26)
    net.load_state_dict(tt(sd), strict=True)
    net.eval()
    keys = list(net.state_dict().keys())
    assert keys == list(m2sgan_bilstm_shapes()), "param spec order differs from the reference module's"
    assert [tuple(v.shape) for v in net.state_dict().values()] == list(m2sgan_bilstm_shapes().values())
    dec = {k[4:]: v for k, v in sd.items() if k.startswith("tcn.")}
    out = {"keys": np.array(keys), "shapes": np.array([str(tuple(v.shape)) for v in net.state_dict().values()]),
           "weight_digest": np.int64(L.digest(sd)), "cases": np.array(L.GENERATOR_CASES)}
    # The restatement of the full generator follows the kernels' arithmetic in both halves: the decoder's fp32 order, and for the
    # features the number format of the music encoder the generator's handle pins - the split format (hi + lo of two bf16 values per
    # operand, three products per term), modelled on the reference's own encoder; the noise branch is plain fp32 on both sides.
    split_enc = split_format_encoder(net.music_encoder)
    for T, Tm in L.GENERATOR_CASES:
        mel, z = HG.fixture_inputs(T, Tm)
        with torch.no_grad():
            pose = net(torch.from_numpy(mel), torch.from_numpy(z)).numpy().reshape(L.B, T, 26)
            feat = net.features(torch.from_numpy(mel), torch.from_numpy(z)).numpy()
            feat_split = np.concatenate([split_enc(torch.from_numpy(mel)).numpy(), feat[..., 64:]], axis=2)
        f64 = HG.oracle_features(sd, mel, z)
        p64 = L.decoder_fp64(dec, f64)[0]
        pe = L.decoder_fp32_emulated(dec, feat_split)[0]
        pd = L.decoder_fp32_emulated(dec, feat)[0]               # the decoder's restatement alone, on the reference's fp32 features
        print(f"generator T={T}: features vs fp64: the reference's fp32 {L.max_abs(feat, f64):.3e}, the split-format restatement "
              f"{L.max_abs(feat_split, f64):.3e}", flush=True)
        n = HG.case_name(T, Tm)
        out[f"pose_{n}"], out[f"pose64_{n}"] = pose, p64
        out[f"ref_vs_fp64_{n}"], out[f"emul_vs_fp64_{n}"] = np.float64(L.max_abs(pose, p64)), np.float64(L.max_abs(pe, p64))
        out[f"decoder_emul_vs_fp64_{n}"] = np.float64(L.max_abs(pd, p64))
        print(f"generator T={T}: ref_vs_fp64 {out[f'ref_vs_fp64_{n}']}  emul_vs_fp64 {out[f'emul_vs_fp64_{n}']}  "
              f"decoder_emul_vs_fp64 {out[f'decoder_emul_vs_fp64_{n}']}", flush=True)
    np.savez(os.path.join(GOLDEN, L.FILES["gen"]), **out)
    for f in list(L.FILES.values()) + list(L.HIDDEN_FILES.values()):
        size = os.path.getsize(os.path.join(GOLDEN, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == "__main__":
    main()
