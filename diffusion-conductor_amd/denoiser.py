"""Drop-in for the reference's ``MotionTransformer`` on the sampling path.

Mirrors Diffusion_Stage/models/transformer.py:360-497: same constructor keywords, the same
``state_dict`` keys (so ``load_state_dict`` takes the reference's ``state['encoder']``), and
``forward`` / ``encode_music`` / ``generate_src_mask`` with the reference's argument meaning.
``forward`` and ``encode_music`` (the one-time MusicEncoder conv stack, transformer.py:289-340,
447-459) run entirely in libdc_ddim.so (hand-written gfx950 kernels); there is no PyTorch-op or
CPU fallback for either.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from .native import NativeSampler
from .param_spec import DenoiserConfig, param_shapes


class _Node(nn.Module):
    """Anonymous container so that parameter paths equal the reference's state_dict keys."""


def _build_tree(root: nn.Module, shapes):
    for name, shape in shapes.items():
        parts = name.split(".")
        node = root
        for p in parts[:-1]:
            if p not in node._modules:
                node.add_module(p, _Node())
            node = node._modules[p]
        leaf = parts[-1]
        if leaf in ("running_mean", "running_var"):
            node.register_buffer(leaf, torch.ones(shape) if leaf == "running_var" else torch.zeros(shape))
        elif leaf == "num_batches_tracked":
            node.register_buffer(leaf, torch.tensor(0, dtype=torch.long))
        else:
            node.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))


class MotionTransformer(nn.Module):
    def __init__(self, input_feats, num_frames=240, latent_dim=16, ff_size=64, num_layers=8, num_heads=8,
                 dropout=0, activation="gelu", device="cuda", text_num_heads=4, music_model_path=None,
                 no_eff=False, precision="fp16", max_timesteps=1000, **kargs):
        # `no_clip=` and other reference-only keywords are swallowed by **kargs, as in the reference.
        super().__init__()
        if dropout != 0:
            raise NotImplementedError("sampling path only: dropout must be 0 (reference default)")
        self.cfg = DenoiserConfig(input_feats=input_feats, num_frames=num_frames, latent_dim=latent_dim,
                                  ff_size=ff_size, num_layers=num_layers, num_heads=num_heads, no_eff=bool(no_eff))
        self.num_frames, self.latent_dim, self.ff_size = num_frames, latent_dim, ff_size
        self.num_layers, self.num_heads, self.input_feats = num_layers, num_heads, input_feats
        self.time_embed_dim = latent_dim * 4
        self.device = device
        # precision: "fp16" (default) | "mixed" | "bf16x3" | "bf16" | "auto".  "auto" starts in fp16 and, the first time a
        # sampling loop reports a non-finite x0 (fp16 operands overflow beyond +-65504), rebuilds the sampler in "mixed"
        # (bf16-range operands) and re-runs that loop; the switch is sticky for this module (numerics_fallback).
        if precision not in ("fp16", "mixed", "bf16x3", "bf16", "auto"):
            raise ValueError(f"unknown precision {precision!r}")
        if no_eff and precision not in ("fp16", "auto"):
            raise ValueError(f"no_eff=True (full T x T attention, transformer.py:198-287) is built for precision='fp16' only, not {precision!r}: "
                             "bf16 attention operands leave 1 - 2e-3 on x0 (outside the 1e-3 parity bound), the split precisions have no full-attention kernels")
        self.precision = precision
        self.active_precision = "fp16" if precision == "auto" else precision
        self.check_numerics = True          # one dc_sampler_status per sampling loop (a stream synchronisation)
        self.max_timesteps = max_timesteps
        _build_tree(self, param_shapes(self.cfg))
        if music_model_path is not None:
            # transformer.py:394-401: seed the MusicEncoder from the stage-1 checkpoint
            base = torch.load(music_model_path, map_location="cpu")
            sub = {k.replace("module.music_encoder.", "music_encoder."): v for k, v in base.items()
                   if k.startswith("module.music_encoder")}
            self.load_state_dict(sub, strict=False)
        self._native = None
        self._native_dirty = True
        self._cond_key = None
        self.eval()

    # ---- weights ------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._native_dirty = True
        return out

    def _ensure_native(self, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("MotionTransformer.forward runs only on an MI355X (gfx950) device; "
                               "there is no CPU path (use oracle/ for CPU reference results)")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if self._native is None or self._native.device != idx:
            if self._native is not None:
                self._native.close()
            self._native = NativeSampler(self.cfg, self.active_precision, self.max_timesteps, idx)
            if self.encoder_format is not None:
                self._native.set_encoder_format(self.encoder_format)
            if self.precise_tail is not None:
                self._native.set_precise_tail(self.precise_tail)
            if self._combine_exchange is not None:
                self._native.set_combine_exchange(self._combine_exchange)
            if self._precise_forward:
                self._native.set_precise_forward(True)
            self._native_dirty = True
        if self._native_dirty:
            self._native.load_state_dict(self.state_dict())
            self._native_dirty = False
            self._cond_key = None
        return self._native

    def numerics_fallback(self, status):
        """Called by the sampler when dc_sampler_status reported `status` after a loop.  Returns True when the module has
        switched to a mode that can hold the values (the caller re-runs the loop on the fresh sampler), False when there is
        none: only precision="auto" switches, only from fp16, and only for a non-finite x0 - a FiLM value outside the fp16
        storage range is outside every mode."""
        from . import native
        # (exactly NONFINITE: with the saturation bit the values are outside every mode, and no other bit is a precision problem)
        if self.precision != "auto" or self.active_precision != "fp16" or status != native.STATUS_NONFINITE or self.cfg.no_eff:
            return False          # (full attention exists in fp16 only: nothing to fall back to)
        if self._native is not None:
            self._native.close()
        self._native = None
        self._cond_key = None
        self.active_precision = "mixed"
        return True

    # ---- reference surface ----------------------------------------------------------------
    def generate_src_mask(self, T, length):
        """transformer.py:461-467 (vectorised)."""
        length = torch.as_tensor(length)
        return (torch.arange(T)[None, :] < length.cpu()[:, None]).float()

    def encode_music(self, text, device):
        """transformer.py:447-459 in eval mode: mel [B,Tm,128] -> (x_proj, x), each [B,Tm/3,64]."""
        if self.training:
            raise NotImplementedError("sampling path only: call .eval() (training-time token dropout not built)")
        nat = self._ensure_native(device)
        if text.dim() != 3:
            raise ValueError("mel must be [B, Tm, 128]")
        if (not text.is_cuda and text.dtype == torch.float32 and text.is_contiguous() and text.is_pinned()
                and text.shape[0] >= 2 * self.h2d_chunk):
            return self._encode_music_pipelined(nat, text, torch.device(device))
        mel = text.to(device=device, dtype=torch.float32).contiguous()
        return nat.encode_music(mel)

    # MusicEncoder activation format: None = the library's choice by precision ("f16": one fp16 plane beside an fp16 / bf16 denoiser,
    # 3.7e-4 at the encoder's output and half the time; "split": two bf16 planes, 6e-6, beside the split-operand precisions); set before
    # the first forward / encode_music.  DC_ME_PREC=f16|split in the environment overrides it.
    encoder_format = None
    # fp16 precision: the sampling loops' last `precise_tail` model evaluations on split fp16 operands (include/dc_ddim.h,
    # dc_sampler_set_precise_tail); set before the first forward.  DC_PRECISE_TAIL=k in the environment overrides it.
    precise_tail = None       # None: the library's default (1 for fp16, 6 for bf16)

    # Small batches (at most one 64-token unit per CU): whether a clip's workgroups share the attention combine inside a layer launch
    # (None / True: the library's default) or every workgroup combines alone (False: no in-launch wait - for a GPU shared with other
    # work, several samplers on streams of one process, or loops whose status nobody reads; dc_ddim.h, dc_sampler_set_combine_exchange).
    _combine_exchange = None

    @property
    def combine_exchange(self):
        return self._combine_exchange

    @combine_exchange.setter
    def combine_exchange(self, on):
        self._combine_exchange = None if on is None else bool(on)
        if self._native is not None:
            self._native.set_combine_exchange(True if on is None else bool(on))

    # forward() on split operands (the precise tail's evaluation form; dc_ddim.h, dc_sampler_set_precise_forward): the sampler's
    # step-through path switches it on for the loops whose update keeps the evaluations' error (EPSILON / PREVIOUS_X models, cond_fn).
    _precise_forward = False

    @property
    def precise_forward(self):
        return self._precise_forward

    @precise_forward.setter
    def precise_forward(self, on):
        self._precise_forward = bool(on)
        if self._native is not None:
            self._native.set_precise_forward(bool(on))

    h2d_chunk = 8        # a pinned host batch of at least 2 x this many clips is copied in chunks beside the encoder
    h2d_schedule = (8, 8, 4)     # ... of B/8, B/8, B/4 clips and the rest: the first copy is the only one the encoder waits for

    @staticmethod
    def _h2d_bounds(B, sizes):
        """[lo, hi) clip ranges of the host-to-device copies: the given sizes in turn, the last one taking whatever is left."""
        out, lo = [], 0
        for i, n in enumerate(sizes):
            if lo >= B:
                break
            hi = min(lo + max(1, int(n)), B) if i + 1 < len(sizes) else B
            out.append((lo, hi))
            lo = hi
        if lo < B:
            out.append((lo, B))
        return out

    def _encode_music_pipelined(self, nat, mel_host, device):
        """A pinned host batch: the mel spectrograms cross PCIe in chunks on a copy stream while the MusicEncoder works on the
        chunks that have landed - most of the 1.8 ms the 88 MB of a 32-clip batch take hide behind the convolutions."""
        B, Tm, _ = mel_host.shape
        T = (Tm - 1) // 3 + 1
        if device.index is None:              # "cuda" never equals a tensor's "cuda:0": the buffer and the stream would be re-made per call
            device = torch.device("cuda", torch.cuda.current_device())
        cur = torch.cuda.current_stream(device)
        if getattr(self, "_copy_stream", None) is None or self._copy_stream.device != device:
            self._copy_stream = torch.cuda.Stream(device)
        cs = self._copy_stream
        # Two device-side staging buffers of the module's own, used alternately and reused call after call (a fresh 88-MB tensor per call
        # goes through the caching allocator's cross-stream bookkeeping and, whenever that ends in a hipMalloc, costs the call 6 ms).
        # The copy stream waits only for the encode that last READ the slot (two calls ago), not for whatever the compute stream is
        # doing: a caller that enqueues batch k + 1 while batch k's loop runs (evaluate.py) gets its mel across PCIe beside that loop.
        slots = getattr(self, "_mel_slots", None)
        n = mel_host.numel()
        if slots is None or slots[0][0].device != device:
            slots = self._mel_slots = [[None, None], [None, None]]      # [staging tensor, event: its last reader is done]
            for sl in slots:
                sl[0] = torch.empty(0, dtype=torch.float32, device=device)
            self._mel_turn = 0
        self._mel_turn ^= 1
        sl = slots[self._mel_turn]
        if sl[0].numel() < n:
            sl[0] = torch.empty(n, dtype=torch.float32, device=device)
            cs.wait_stream(cur)                   # (a fresh allocation is ordered on `cur`)
        mel = sl[0][:n].view(tuple(mel_host.shape))
        xf_proj = torch.empty((B, T, 64), dtype=torch.float32, device=device)
        xf_out = torch.empty_like(xf_proj)
        if sl[1] is not None:
            cs.wait_event(sl[1])                  # the encode that read this slot (possibly on another stream) is done with it
        events = []
        sched = os.environ.get("DC_H2D_CHUNKS")          # diagnostic: explicit chunk sizes, e.g. "4,12,16"
        # default: growing chunks (32 clips: 4, 4, 8, 16) - the first copy is the only one the encoder waits for and every later one
        # is shorter than the encode it runs beside.  With the 2.1-ms fp16-plane encoder, end to end at bs=32: 38.3 ms against 38.7 for
        # round 3's "8, then the rest" (then the best for a 4.4-ms encoder) and 38.5 for four of 8 (profiles/r05_ab_h2d_chunks.txt)
        sizes = [int(v) for v in sched.split(",")] if sched else [max(1, B // d) for d in self.h2d_schedule] + [B]
        with torch.cuda.stream(cs):
            for lo, hi in self._h2d_bounds(B, sizes):
                mel[lo:hi].copy_(mel_host[lo:hi], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cs)
                events.append((lo, hi, ev))
        for lo, hi, ev in events:
            cur.wait_event(ev)
            nat.encode_music(mel[lo:hi], out=(xf_proj[lo:hi], xf_out[lo:hi]))
        sl[1] = torch.cuda.Event()
        sl[1].record(cur)
        return xf_proj, xf_out

    def null_conditioning(self):
        """The null pair (null_proj[64], null_out[64]) of classifier-free guidance: the all-masked limit of the reference's token
        dropout (transformer.py:389,451-459 zeroes a token's music features before `proj`), null_out = 0 and null_proj = proj(0) =
        proj.bias.  The reference has no sampling counterpart."""
        return self.get_parameter("proj.bias").detach().float().cpu().reshape(64), torch.zeros(64)

    def set_conditioning(self, xf_proj, xf_out, length=None, guided=False, takes=1, windows=None):
        """`guided`: the conditioning of a guided loop (include/dc_ddim.h, dc_sampler_set_conditioning_guided) with null_conditioning().
        `takes`: samples per music (dc_sampler_set_conditioning_takes): the loops then run takes x the musics, take-major.
        `windows`: (starts [W], weights fp32 [W, T], L) - the features are the W x B windows of B pieces of L frames, window-major, and
        the loops run over the pieces (dc_sampler_set_conditioning_windows); set on every call (the plan is part of it)."""
        nat = self._ensure_native(xf_proj.device)
        if windows is not None:
            self._cond_key = None
            starts, weights, L = windows
            nat.set_conditioning_windows(xf_proj.contiguous().float(), xf_out.contiguous().float(), starts, weights, L,
                                         null=self.null_conditioning() if guided else None)
            return nat
        T = xf_proj.shape[1]
        if length is None:
            length = [T] * xf_proj.shape[0]
        ln = tuple(int(v) for v in (length.tolist() if hasattr(length, "tolist") else length))
        # The reference passes the same xf_proj/xf_out tensors on every step; recompute the step-invariant
        # part only when they change.  Identity is by object (held alive here), never by data_ptr - the
        # caching allocator hands the same address to a new tensor.
        k = self._cond_key
        same = (k is not None and k[0] is xf_proj and k[1] is xf_out and k[2] == (xf_proj._version, xf_out._version)
                and k[3] == ln and k[4] == bool(guided) and k[5] == int(takes))
        if not same:
            self._cond_key = None
            nat.set_conditioning(xf_proj.contiguous().float(), xf_out.contiguous().float(), list(ln),
                                 null=self.null_conditioning() if guided else None, takes=int(takes))
            self._cond_key = (xf_proj, xf_out, (xf_proj._version, xf_out._version), ln, bool(guided), int(takes))
        return nat

    def forward(self, x, timesteps, length=None, text=None, xf_proj=None, xf_out=None):
        """transformer.py:469-497.  x [B,T,P] (or [B,T,J,2]); timesteps [B]; returns [B,T,P]."""
        B, T = x.shape[0], x.shape[1]
        if xf_proj is None or xf_out is None:
            if text is None:
                raise ValueError("need xf_proj/xf_out or text (mel)")
            xf_proj, xf_out = self.encode_music(text, x.device)
        if x.dim() == 4:
            x = torch.flatten(x, start_dim=2, end_dim=3)
        nat = self.set_conditioning(xf_proj, xf_out, length)
        return nat.denoise(x.contiguous().float(), timesteps).view(B, T, -1).contiguous()
