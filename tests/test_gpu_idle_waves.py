"""The barrier-only path of a clip's padding waves in the wide plain layer kernel (k_layer, layer_idle_wave;
dc_sampler_set_idle_wave_path): clip-aligned units pad a clip to whole 256-token workgroups, and a wave of the last workgroup that has
no tokens issues its shares of the weight-image copies, takes part in the combine, the barriers and the record tail, and does nothing
else.  Nothing such a wave computed has ever reached an output, so the setting must not move a single bit: every case runs with the
path on (the default) and off (the waves run the whole layer, as before the setting existed) and asks for torch.equal and status 0.

DC_NO_NARROW=1 forces the wide 8-wave form at sizes a test can afford.  One fresh child process per environment (captured loops and
single evaluations; eager loops under DC_DISABLE_GRAPH=1) runs all its cases and prints one JSON line each.

Shapes (clip stride = frames padded to whole 32-token groups):
  3 x 264  stride 288 = 9 groups: the second workgroup of a clip has ONE active wave, on a partial last group, and 7 padding waves -
           the situation of the headline's 32 x 1800 (57 groups)
  3 x 480  15 groups: 7 active waves and 1 padding wave
  2 x 512  16 groups: no padding wave - the control, the setting changes nothing
  3 x 264 ragged, lengths 263 / 258 / 131: the one active wave of the second workgroup sees 7, 2 and 0 valid rows
A DDIM loop of 4 steps with the default precise tail is, in fp16: two plain steps whose last layer does the next step's front work
(embed_next), the plain step in front of the split one (no embed_next: its last layer ends behind the output projection), and the split
step, which the setting does not touch.  In bf16 the default tail (6) covers a loop of 4 steps entirely, so the bf16 shape runs a
loop of 8 steps as well (2 plain + 6 split)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (precision, B, frames, lengths or None, steps; 0 steps = one evaluation through forward)
CAPTURED = {
    "fp16_3x264": ("fp16", 3, 264, None, 4),
    "fp16_3x480": ("fp16", 3, 480, None, 4),
    "fp16_2x512_control": ("fp16", 2, 512, None, 4),
    "fp16_3x264_ragged": ("fp16", 3, 264, [263, 258, 131], 4),
    "bf16_3x264": ("bf16", 3, 264, None, 4),
    "bf16_3x264_8steps": ("bf16", 3, 264, None, 8),
    "fp16_3x264_forward": ("fp16", 3, 264, [263, 258, 131], 0),
}
EAGER = {
    "fp16_3x264_eager": ("fp16", 3, 264, [263, 258, 131], 4),
}


def _child(names):
    """Runs in the child process: each named case with the path on and off -> one JSON line per case."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import make_model, xf_pair
    from diffusion_conductor_amd import native
    from diffusion_conductor_amd.sampler import betas_for_alpha_bar
    from diffusion_conductor_amd.synthetic import batch_noise
    import math

    cases = dict(CAPTURED, **EAGER)
    models = {}
    for name in names:
        prec, B, T, length, S = cases[name]
        if prec not in models:
            models[prec] = make_model(prec)
        m = models[prec]
        xfp, xf = xf_pair(B, T, first=3)
        nat = m.set_conditioning(xfp.cuda().contiguous(), xf.cuda().contiguous(), length if length is not None else [T] * B)
        x = torch.from_numpy(batch_noise(B, T, first=3)).cuda()
        if S:
            betas = np.asarray(betas_for_alpha_bar(S, lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2), np.float64)
            coef = native.ddim_coefficients(np.cumprod(1.0 - betas))
            run = lambda: nat.ddim_loop(x, coef)[0]
        else:
            t = torch.tensor([(131 * b + 5) % 1000 for b in range(B)])
            run = lambda: nat.denoise(x, t)
        res, status = {}, {}
        for on in (True, False, True):          # (the third run: back on, through the key's bit once more)
            nat.set_idle_wave_path(on)
            out = run()
            torch.cuda.synchronize()
            status[on] = nat.status()
            if on in res:
                assert torch.equal(res[on], out), "two runs of one setting differ"
            res[on] = out.clone()
        nat.set_idle_wave_path(True)
        print(json.dumps({"case": name, "stride": nat.clip_stride(), "equal": bool(torch.equal(res[True], res[False])),
                          "finite": bool(torch.isfinite(res[True]).all()), "moved": bool(not torch.equal(res[True], x)),
                          "max_abs_diff": float((res[True] - res[False]).abs().max()),
                          "status_on": int(status[True]), "status_off": int(status[False])}), flush=True)


def _run_children(names, extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DC_")}
    env.update(DC_NO_NARROW="1", **extra_env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *names], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            out[d["case"]] = d
    return out


@pytest.fixture(scope="module")
def captured():
    return _run_children(list(CAPTURED), {})


@pytest.fixture(scope="module")
def eager():
    return _run_children(list(EAGER), {"DC_DISABLE_GRAPH": "1"})


def _check(d, frames):
    print(d)
    assert d["stride"] == (frames + 31) // 32 * 32
    assert d["finite"] and d["moved"]
    assert d["status_on"] == 0 and d["status_off"] == 0
    assert d["equal"], d


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CAPTURED))
def test_idle_wave_path_changes_no_bit(captured, name):
    """Captured DDIM loops (and one evaluation through forward, out_mode 0): x0 with the padding waves' barrier-only path on and off is
    bit-identical, status 0 both ways."""
    _check(captured[name], CAPTURED[name][2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EAGER))
def test_idle_wave_path_changes_no_bit_eager(eager, name):
    """The same loop enqueued on the stream itself (DC_DISABLE_GRAPH=1)."""
    _check(eager[name], EAGER[name][2])


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2:])
